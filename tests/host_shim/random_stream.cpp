// csrc/random_stream.hpp compiled for the CPU: the block function, the two u128 -> field reductions, the element rule and the range
// check, on caller-supplied inputs.  No value is compared here: tests/test_random_stream_host.py holds the expected words, from
// tests/random_stream.py and Python integers.
//   random_stream <in> <out>
// in (u64 words): a sequence of records, each starting with its kind
//   1 block:   seed[4] (the 32 bytes as four little-endian u64), nonce[3], counter        -> 8 words: the block's 64 bytes
//   2 reduce:  field (0 Goldilocks, 1 BabyBear), lo, hi                                    -> 1 word: (lo + 2^64 hi) mod p
//   3 range:   field, seed[4], nonce[3], first, count                                      -> range_ok, then (if ok) count words
//   4 element: field, seed[4], nonce[3], e                                                 -> 1 word: element e alone
// Exit status 3 on a malformed file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "random_stream.hpp"
#include "random_stream_case.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!random_case::read_words(argv[1], &in)) return 3;
    if (!random_case::run(in, &out, random_case::on_host)) return 3;
    return random_case::write_words(argv[2], out) ? 0 : 3;
}
