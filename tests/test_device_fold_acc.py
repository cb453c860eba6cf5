"""csrc/fold_acc.hpp's FoldAcc<GlF> / FoldAcc<BbF> and gl::fold160 built for gfx950 from the headers alone and run on the GPU
(tests/device/fold_acc.hip), one thread per chain, on the chains of tests/host_shim/fold_acc_cases.hpp - the ones
tests/test_fold_acc_host.py runs on the CPU, where the field headers' instruction-level branches are not compiled.  Every family
must report mismatches=0 on exactly the chains the CPU runner has, with no census class empty."""
import os
import subprocess

import pytest

from test_fold_acc_host import check_output

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fold_sums_on_the_device_match_exact_integers_on_pulled_back_edge_and_random_chains(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    exe = tmp_path / "fold_acc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
           "-o", str(exe), os.path.join(ROOT, "tests", "device", "fold_acc.hip")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:] + out.stderr)
    check_output(out.stdout)
