"""The device arithmetic under the prover kernels - gl::add / sub / mul / fold160, GlF::mul_lazy / mulc / emul / einv, bb::add / sub /
mul / reduce / reduce_lazy / mul_lazy / mul_signed / reduce_signed, BbF::add_lazy, BbF::acc_mac2 (the inline-assembly path, which
the host shim of tests/test_device_headers_on_host.py never compiles) / acc_finish, BbF::emul / einv - built for gfx950 from the
headers and run on the carry edges squared plus 2^16 seeded random operands per function, against 128-bit integer arithmetic
written in the program itself (tests/device/field_edges.hip).  tests/test_mul_mont_forms.py does the same for gl::mul_mont_lazy."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_device_field_arithmetic_matches_128_bit_host_arithmetic_on_the_edge_sets(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    exe = tmp_path / "field_edges"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "device", "field_edges.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"cases=(\d+) mismatches=0\b", out.stdout)
    assert m and int(m.group(1)) >= 20 * (1 << 16), out.stdout
