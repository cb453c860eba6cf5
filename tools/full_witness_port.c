/* The host loop that gb_prove_partition replaces, for tools/partition_witness_times.py to time: a PORT to C, written for this
 * tool, of what PartitionWitness::full_witness does (iop/witness.rs:359-371) - one thread, rows outside, wires inside, every
 * target a dependent read values[representative_map[row * num_wires + column]] and a strided write wire_values[column][row].
 * It is not the reference's Rust: no Option, no Vec<Vec<F>>, one flat output block. */
#include <stddef.h>
#include <stdint.h>

void full_witness_u64(const uint64_t* values, const uint64_t* representative_map, uint64_t degree, uint64_t num_wires, uint64_t* out) {
    for (uint64_t i = 0; i < degree; i++)
        for (uint64_t j = 0; j < num_wires; j++) out[j * degree + i] = values[representative_map[i * num_wires + j]];
}

void full_witness_u32(const uint32_t* values, const uint64_t* representative_map, uint64_t degree, uint64_t num_wires, uint32_t* out) {
    for (uint64_t i = 0; i < degree; i++)
        for (uint64_t j = 0; j < num_wires; j++) out[j * degree + i] = values[representative_map[i * num_wires + j]];
}
