// The slot map of gb_circuit_set_partition (include/goldibear_gpu.h): from ProverOnlyCircuitData.representative_map
// (plonk/circuit_data.rs:454), indexed by Target::index (iop/target.rs:55-60: wire (row, col) -> row * num_wires + col, virtual
// target i -> degree * num_wires + i), to what PartitionWitness::full_witness (iop/witness.rs:359-371) needs on the device.
//
// A "slot" is a representative that at least one WIRE cell points to; slots are ranked in ascending target index, so that the
// compaction staged[k] = values[reps[k]] streams through `values` front to back.  A representative no wire cell uses - most
// virtual targets - gets no slot and its value never leaves the host.
//
// Host code without HIP dependencies: tests/sanitize/partition_map.cpp compiles it alone with the sanitizers.
#ifndef GOLDIBEAR_PARTITION_MAP_HPP
#define GOLDIBEAR_PARTITION_MAP_HPP

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace gbk {
namespace partition {

enum MapStatus { MAP_OK = 0, MAP_INVALID = 1, MAP_UNSUPPORTED = 4 };   // the values of GB_OK / GB_ERR_INVALID / GB_ERR_UNSUPPORTED

struct SlotMap {
    uint64_t num_targets = 0, num_cells = 0;
    std::vector<uint32_t> reps;        // [K] the representatives that wire cells use, ascending
    std::vector<uint32_t> slots;       // [num_cells] row-major [n][num_wires] like the map: cell -> index into reps
    std::vector<uint64_t> shared;      // bit k: more than one wire cell reads slot k
    std::vector<uint32_t> pi_reps;     // representative_map[public_input_targets[i]] (any target: it need not have a slot)
    bool is_shared(uint32_t k) const { return (shared[k >> 6] >> (k & 63)) & 1; }
};

// mark, rank, validate.  *msg names what was refused.
inline MapStatus build_slot_map(const uint64_t* representative_map, uint64_t num_targets, uint64_t num_cells,
                                const uint64_t* public_input_targets, uint64_t num_public_inputs, uint64_t expected_public_inputs,
                                SlotMap* out, const char** msg) {
    const char* unused;
    if (!msg) msg = &unused;
    if (!representative_map || !out || (num_public_inputs && !public_input_targets)) { *msg = "null argument"; return MAP_INVALID; }
    if (num_targets < num_cells) { *msg = "num_targets is below degree * num_wires: the map must cover every wire"; return MAP_INVALID; }
    if (num_public_inputs != expected_public_inputs) { *msg = "Number of public inputs doesn't match circuit data."; return MAP_INVALID; }
    if (num_targets >> 32) { *msg = "2^32 targets or more: slots are 32-bit"; return MAP_UNSUPPORTED; }
    for (uint64_t t = 0; t < num_targets; t++)
        if (representative_map[t] >= num_targets) { *msg = "representative_map entry out of range"; return MAP_INVALID; }
    for (uint64_t i = 0; i < num_public_inputs; i++)
        if (public_input_targets[i] >= num_targets) { *msg = "public input target out of range"; return MAP_INVALID; }
    SlotMap m;
    m.num_targets = num_targets;
    m.num_cells = num_cells;
    std::vector<uint8_t> uses(num_targets, 0);   // wire cells per representative, saturating at 2
    for (uint64_t cell = 0; cell < num_cells; cell++) {
        uint8_t& u = uses[representative_map[cell]];
        if (u < 2) u++;
    }
    std::vector<uint32_t> rank(num_targets, 0);
    for (uint64_t t = 0; t < num_targets; t++)
        if (uses[t]) {
            rank[t] = (uint32_t)m.reps.size();
            m.reps.push_back((uint32_t)t);
        }
    m.shared.assign((m.reps.size() + 63) / 64, 0);
    for (size_t k = 0; k < m.reps.size(); k++)
        if (uses[m.reps[k]] > 1) m.shared[k >> 6] |= (uint64_t)1 << (k & 63);
    m.slots.resize(num_cells);
    for (uint64_t cell = 0; cell < num_cells; cell++) m.slots[cell] = rank[representative_map[cell]];
    m.pi_reps.resize(num_public_inputs);
    for (uint64_t i = 0; i < num_public_inputs; i++) m.pi_reps[i] = (uint32_t)representative_map[public_input_targets[i]];
    *out = std::move(m);
    *msg = "";
    return MAP_OK;
}

}  // namespace partition
}  // namespace gbk
#endif
