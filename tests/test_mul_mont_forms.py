"""gl::mul_mont_lazy of csrc/gl_field.hpp (the 14-instruction Montgomery product: the fold's final conditional "- EPS" is an
add-with-carry and a subtract-with-borrow on the borrow flag, gl::mont_fold_flags) returns the same u64 word as
mont_fold(mul_limbs(a, b)), the form it replaces, for both FIVE forms: compiled for the CPU from the header itself (the host
overloads of the flag helpers model the device instructions limb by limb, flags as bits), on the carry edges squared, on pairs
built so that (m2.hi, 0) - b does not borrow (probability ~2^-32 on random operands: the rare branch of the 13-instruction form
that tools/microbench_mulmod.hip keeps as M10 / M12, and an edge of the fold's subtraction either way), and on 10^6 seeded random
pairs."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc


def test_new_product_is_the_old_word_on_edges_and_random_pairs(tmp_path):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path / "mul_mont_forms"
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = [CLANG, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "mul_mont_forms.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), "1000000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout
    m = re.search(r"pairs=(\d+) by0=(\d+) by0_nonzero_low=(\d+) constructed=(\d+)", out.stdout)
    assert m, out.stdout
    pairs, by0, by0_nonzero_low, constructed = map(int, m.groups())
    assert pairs >= 1000000 + 27 * 27
    # the no-borrow branch was taken, and not only by products whose low half is zero
    assert by0 >= 1 and by0_nonzero_low >= 2 * constructed >= 2


@pytest.mark.gpu
def test_device_product_matches_the_host_forms_on_the_edge_set(tmp_path):
    """the same pairs through a one-product kernel built for gfx950 from the header: the inline-asm carry chain itself"""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    exe = tmp_path / "mul_mont_edges"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "device", "mul_mont_edges.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout
    m = re.search(r"pairs=(\d+) by0=(\d+) by0_nonzero_low=(\d+)", out.stdout)
    assert m and int(m.group(1)) >= 27 * 27 and int(m.group(3)) >= 2, out.stdout
