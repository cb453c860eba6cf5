// What the generator schedule (generator_schedule.hpp, host) hands to the generator kernels (generators.hpp, device): plain words,
// no HIP and no field code, so that either side compiles without the other.
//
// An Op is one scheduled generator.  Its dependencies and outputs are class indices in `args` (the dense class index of the
// schedule: the slots of partition_map.hpp first), in the order the generator's gate lays its wires out; an output entry carries
// what the schedule resolved for it: store (plain index), check (OUT_CHECK set: compare with the stored value, do not write) or
// OUT_SKIP (written or checked by another Op of the same generator).
#ifndef GOLDIBEAR_GENERATOR_OPS_HPP
#define GOLDIBEAR_GENERATOR_OPS_HPP

#include <stdint.h>

namespace gbk {
namespace gen {

// record kinds: the values of GB_GEN_* (include/goldibear_gpu.h)
enum Kind : uint32_t {
    GEN_ARITHMETIC = 0,
    GEN_ARITHMETIC_EXTENSION = 1,
    GEN_MUL_EXTENSION = 2,
    GEN_CONSTANT = 3,
    GEN_BASE_SPLIT = 4,
    GEN_REDUCING = 5,
    GEN_REDUCING_EXTENSION = 6,
    GEN_RANDOM_ACCESS = 7,
    GEN_POSEIDON_MDS = 8,
    GEN_COSET_INTERPOLATION = 9,
    GEN_EXPONENTIATION = 10,
    GEN_POSEIDON = 11,
    GEN_POSEIDON2_BABYBEAR = 12,
    GEN_ADD_MANY = 13,
    GEN_APPLY_MAT4 = 14,
    GEN_POSEIDON2_INTERNAL = 15,
    GEN_COPY = 16,
    GEN_NUM_KINDS = 17,   // gate generators and Copy: 17 .. 31 are reserved and refused
    // gadget generators: a head record (gate = the parameter, a = the number of targets, b = 0) and ceil(a / 2) GEN_TARGETS
    // continuation records that carry two targets each, in the order given beside the kind
    GEN_EQUALITY = 32,             // x, y, equal, inv
    GEN_NONZERO_TEST = 33,         // to_test, dummy
    GEN_QUOTIENT_OR_ZERO = 34,     // numerator, denominator, quotient
    GEN_QUOTIENT_EXTENSION = 35,   // numerator[D], denominator[D], quotient[D]
    GEN_SPLIT = 36,                // integer, bits[0..64]
    GEN_WIRE_SPLIT = 37,           // integer, the WIRE_SUM target of each gate; parameter num_limbs
    GEN_LOW_HIGH = 38,             // integer, low, high; parameter n_log
    GEN_BASE_SUM = 39,             // sum, limbs[1..]; parameter B
    GEN_TARGETS = 40,              // continuation
    GEN_GADGET_FIRST = GEN_EQUALITY,
    GEN_GADGET_END = GEN_TARGETS   // one past the last head kind
};

constexpr uint32_t GROUP = 256;   // the chain kernel's workgroup: a level up to this wide stays inside a chain launch
// the kinds generators.hpp evaluates (generator_schedule.hpp refuses the others): every gate generator, Copy and the gadget heads
constexpr bool built_kind(uint32_t kind) { return kind < GEN_NUM_KINDS || (kind >= GEN_GADGET_FIRST && kind < GEN_GADGET_END); }
constexpr uint32_t OUT_CHECK = 0x80000000u, OUT_SKIP = 0xFFFFFFFFu, MAX_CLASSES = 0x7FFFFFFFu;

struct Op {
    uint32_t kind;      // Kind
    uint32_t record;    // index of the gb_generator record (error reports)
    uint32_t in_off;    // args[in_off .. in_off + num_in): dependency classes
    uint32_t num_in;
    uint32_t out_off;   // args[out_off .. out_off + num_out): output classes | OUT_CHECK, or OUT_SKIP
    uint32_t num_out;
    uint32_t p0, p1;    // the gate's parameters as its evaluator reads them; a gadget generator's parameter is p0
    uint64_t k[2];      // the row's constants, canonical words
};

// the device error word: code (0 = none), record index, class
enum Error : uint32_t {
    ERR_NONE = 0,
    ERR_SET_TWICE = 1,        // "Partition containing ... was set twice with different values" (iop/witness.rs:340-350)
    ERR_SWAP_NOT_BOOLEAN = 2,  // PoseidonGenerator / Poseidon2BabyBearGenerator: assert!(swap == 0 || swap == 1)
    ERR_ACCESS_INDEX = 3,      // RandomAccessGenerator: index >= vec_size
    ERR_SPLIT_TOO_LARGE = 4,   // BaseSplitGenerator: "Integer too large to fit in given number of limbs"; SplitGenerator and
                               // WireSplitGenerator: the reference's debug_assert_eq!(integer_value, 0, ..)
    ERR_DIVIDE_BY_ZERO = 5,    // QuotientGeneratorExtension: num / dem with dem == 0 ("Tried to invert zero")
    ERR_NOT_BOOLEAN = 6        // BaseSumGenerator: get_bool_target, "not a bool"
};
constexpr uint32_t ERROR_WORDS = 4;   // code, record, class, 0

struct Launch {
    uint32_t first_level;   // index into level_off (level 1 of the schedule is index 0)
    uint32_t num_levels;    // chain: a run of narrow levels in one workgroup; level kernel: 1
    uint32_t chain;
};

struct DeviceSchedule {   // the schedule's arrays on the device
    const Op* ops;
    const uint32_t *args, *level_off;
};

}  // namespace gen
}  // namespace gbk
#endif
