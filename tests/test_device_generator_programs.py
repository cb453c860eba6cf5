"""The generator kernels with generator programs (csrc/generators.hpp: k_generate_level<F, true>, k_generate_chain<F, true>, the
registers of gen_program in dynamic LDS) on the GPU, built for gfx950 from the headers alone (tests/device/generator_programs.hip)
and run on the circuits of tests/generator_program_cases.py, against GeneratorProgram.evaluate at every target, both fields: the
cases tests/test_generator_programs.py runs on the host - among them a level of 257 program generators (two workgroups of the
level kernel) and a chain of 5 narrow levels inside one launch of the chain kernel."""
import os
import subprocess

import numpy as np
import pytest

import generator_cases as GC
import generator_program_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("generator_programs_dev") / "generator_programs"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-I", os.path.join(ROOT, "tests", "sanitize"), "-o", str(out), os.path.join(ROOT, "tests", "device", "generator_programs.hip")],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("field", sorted(PC.FIELDS))
def test_the_interpreter_on_the_device_equals_the_mirror(exe, tmp_path, field):
    cases, check = PC.all_cases(field)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    check(GC.read_values(np.fromfile(dst, dtype=np.uint64), len(cases)))
