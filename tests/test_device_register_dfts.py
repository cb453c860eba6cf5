"""The register DFTs of csrc/dft_gl.hpp, csrc/dft_bb.hpp and csrc/ntt_outer.hpp's dft_r built for gfx950 and run on the GPU
(tests/device/register_dfts.hip), one thread per case, on the cases of tests/host_shim/register_dft_cases.hpp - the ones
tests/test_register_dfts_host.py runs on the CPU, where the field headers' instruction-level branches are not compiled.  Every
function of that test's lists must report mismatches=0 on no fewer cases than the lists require."""
import os
import subprocess

import pytest

from test_register_dfts_host import check_output

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_register_dfts_on_the_device_match_the_plain_sum_on_pulled_back_edge_inputs(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    exe = tmp_path / "register_dfts"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
           "-o", str(exe), os.path.join(ROOT, "tests", "device", "register_dfts.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:] + out.stderr)
    check_output(out.stdout)
