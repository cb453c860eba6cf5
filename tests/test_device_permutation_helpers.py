"""The helpers of the permutation headers - poseidon_gl: to_mont, from_mont, add_rc, mul_lazy, mul_add_lazy, reduce128_lazy, sbox,
fold_halves, sub_lazy, fold_rows_rare_carry<12> (no lane / one lane / every lane of a wave carries), mds_layer_mfma<0 / 8>,
partial_group<4 / 2>; poseidon_gl_coop: add_lazy (pairs that force the second carry), row_sum; poseidon2_bb: sbox7, external_layer
<false / true>, internal_round, renorm, renorm_lazy, canonical_out; poseidon2_bb_coop: sbox7, external_layer - built for gfx950 from
the headers and run on edge operands squared plus 2^16 seeded operands per scalar function (edge states plus 2^13 .. 2^14 seeded
states for the functions on states), any u64 where the header says "any u64 in", against 128-bit integer arithmetic written in the
program itself (tests/device/permutation_helpers.hip), with the result ranges the headers state.  tests/test_device_field_edges.py
does the same for the gl:: / bb:: arithmetic underneath."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_permutation_helpers_match_128_bit_host_arithmetic(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    exe = tmp_path / "permutation_helpers"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "device", "permutation_helpers.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"cases=(\d+) mismatches=0\b", out.stdout)
    # ten scalar Goldilocks functions and five BabyBear ones on 2^16 seeded operands each, before the edges and the states
    assert m and int(m.group(1)) >= 15 * (1 << 16), out.stdout
