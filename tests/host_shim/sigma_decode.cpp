// csrc/sigma_decode.hpp compiled for the CPU: decode_value (the coset match and the two-level discrete logarithm) over the tables
// build_dlog_tables / build_coset_tables make, on caller-supplied values.  No value is compared here:
// tests/test_sigma_decode_host.py holds the expected cells, from Python integers.
//   sigma_decode <in> <out>
// in (u64 words): the field (0 Goldilocks, 1 BabyBear), the number of cases, then per case
//   lg, num_routed, raw, count, k_is[num_routed] (canonical), values[count] (canonical; raw = 1: the device words themselves)
// out: per case the result of build_coset_tables (1: distinct cosets), then per value col', row' - or ~0, 0 for "no cell".
// Exit status 3 on a malformed file.
#include <cstdint>
#include <cstdio>

#include "sigma_decode.hpp"
#include "sigma_decode_case.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!sigma_case::read_words(argv[1], &in) || in.size() < 2) return 3;
    const bool ok = in[0] == 0 ? sigma_case::run<gbk::GlF>(in, &out, sigma_case::on_host<gbk::GlF>)
                               : sigma_case::run<gbk::BbF>(in, &out, sigma_case::on_host<gbk::BbF>);
    if (!ok) return 3;
    return sigma_case::write_words(argv[2], out) ? 0 : 3;
}
