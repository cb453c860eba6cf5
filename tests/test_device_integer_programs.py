"""The integer operations of a generator program (IDIV, IREM, SHR, AND, LT: csrc/generators.hpp gen_integer_op) in the generator
kernels on the GPU, built for gfx950 from the headers alone (tests/device/generator_programs.hip) and run on the circuits of
tests/integer_program_cases.py, against GeneratorProgram.evaluate at every target and against plain Python integers at every
operand pair, both fields: every operation over the cross product of the edge operands and the shift amounts in one level of more
than 256 generators (two workgroups of k_generate_level<F, true>), a chain of 5 narrow levels that hands integer results from
level to level (k_generate_chain<F, true>), and IDIV and IREM by zero, each in a circuit of its own, reporting code 9 with the
index of its record."""
import os
import subprocess

import numpy as np
import pytest

import generator_cases as GC
import integer_program_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("integer_programs_dev") / "generator_programs"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-I", os.path.join(ROOT, "tests", "sanitize"), "-o", str(out), os.path.join(ROOT, "tests", "device", "generator_programs.hip")],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("field", sorted(IC.FIELDS))
def test_the_integer_operations_on_the_device_equal_the_mirror(exe, tmp_path, field):
    cases, check = IC.all_cases(field)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    check(GC.read_values(np.fromfile(dst, dtype=np.uint64), len(cases)))
