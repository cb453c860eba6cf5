"""The register DFTs under every commitment - csrc/dft_gl.hpp's mul_pow2 / dft16 / dft32 / dft_small / layer64, csrc/dft_bb.hpp's dft16 /
dft32 / dft_small / layer64 and csrc/ntt_outer.hpp's dft_r - compiled for the CPU (tests/host_shim/register_dfts.cpp) and run on the
cases of tests/host_shim/register_dft_cases.hpp: for every butterfly layer and every ordered pair of carry-edge values an input pulled
back so that the pair stands on the two sides of that layer's butterflies, vectors of edge values, random vectors; expected outputs
from the plain O(R^2) sum in 128-bit arithmetic, compared as words.  The whole-transform tests (test_gpu_transform_dispatch.py,
test_gpu_commit_fuzz.py) reach these branches with probability ~2^-32 per operation.  tests/test_device_register_dfts.py runs the same
cases on the GPU, where the field headers take their instruction-level branches."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> butterfly layers (dft_r and mul_pow2: one set of edge cases); both directions of each
_DFTS = {"dft16": 4, "dft32": 5, "dft_small1": 1, "dft_small2": 2, "dft_small3": 3,
         "layer64_h32_o0": 1, "layer64_h16_o0": 1, "layer64_h16_o32": 1,   # the (H, O) of ntt_passes.hpp's k_intt16_p2w and of dft32
         "dft_r1": 1, "dft_r2": 1, "dft_r3": 1, "dft_r4": 1}
DFT_LAYERS = {"%s_%s_%s" % (f, name, d): layers for f in ("gl", "bb") for name, layers in _DFTS.items() for d in ("fwd", "inv")}
SHIFTS = ["gl_mul_pow2_%d" % k for k in range(96)]
EDGES = {"gl": 200, "bb": 15}   # |E| of register_dft_cases.hpp: the issue's lists, duplicates and values >= p dropped


def check_output(stdout):
    """every function of the lists above with mismatches=0 and no fewer cases than layers |E|^2 + 2^15 (mul_pow2: |E| + 2^12)"""
    edges = {f: int(n) for f, n in re.findall(r"^(gl|bb)_edges=(\d+)$", stdout, re.M)}
    assert edges == EDGES, stdout[:2000]
    lines = {name: (int(n), int(m)) for name, n, m in re.findall(r"^(\w+) cases=(\d+) mismatches=(\d+)\b", stdout, re.M)}
    bad = {name: v for name, v in lines.items() if v[1]}
    assert not bad, stdout[:4000]
    for name, layers in DFT_LAYERS.items():
        assert name in lines, name
        assert lines[name][0] >= layers * edges[name[:2]] ** 2 + (1 << 15), (name, lines[name])
    for name in SHIFTS:
        assert name in lines, name
        assert lines[name][0] >= edges["gl"] + (1 << 12), (name, lines[name])
    assert len(lines) == len(DFT_LAYERS) + len(SHIFTS), sorted(set(lines) - set(DFT_LAYERS) - set(SHIFTS))


def test_register_dfts_match_the_plain_sum_on_pulled_back_edge_inputs(tmp_path):
    shim = os.path.join(ROOT, "tests", "host_shim")
    clang = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
    if not os.path.exists(clang):
        pytest.skip("needs the ROCm clang++ as the host compiler")
    exe = tmp_path / "register_dfts"
    cmd = [clang, "-O2", "-std=c++17", "-pthread", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "register_dfts.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:] + out.stderr)
    check_output(out.stdout)
