"""csrc/random_stream.hpp on the GPU from the header alone (tests/device/random_stream.hip, a stand-alone device program): the
ChaCha20 block on the three known answers, the two u128 -> field reductions on the carry-edge list against Python integers, and
the element rule on the known-answer blocks and on ranges with ragged ends up to the last element the block counter reaches -
the same word file the host build answers in tests/test_random_stream_host.py.  -m gpu only."""
import os
import subprocess

import numpy as np
import pytest

import random_stream_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("random_stream_dev") / "random_stream"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "random_stream.hip")],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RC.FIELDS))
def test_device_functions_equal_the_restatement(device_exe, tmp_path, name):
    words, want = RC.all_records(name)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    words.tofile(src)
    out = subprocess.run([device_exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    got = np.fromfile(dst, dtype=np.uint64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first difference at output word %d: %#x, expected %#x" % (bad[0], got[bad[0]], want[bad[0]])
