"""Generator programs without a GPU: the Python mirror (plonky2_goldibear_amd/generator_program.py) on its own, and the
interpreter of csrc/generators.hpp (gen_program, field_sqrt) compiled for the CPU (tests/host_shim/generator_programs.cpp) on the
schedules csrc/generator_schedule.hpp makes of the circuits of tests/generator_program_cases.py, against GeneratorProgram.evaluate
at every target, both fields: ADD / SUB / MUL at the carry edges, INV, INV_OR_ZERO, IS_ZERO, SQRT (0, the square of the
generator of the full 2-power subgroup, 64 random squares), a program that uses all 32 registers, a level of 257 program
generators mixed with copies, a chain of 5 narrow levels, constants at rows 0 and n - 1, outputs in written classes, and the three
errors with the index of their head record."""
import os
import subprocess

import numpy as np
import pytest

import generator_cases as GC
import generator_program_cases as PC
from plonky2_goldibear_amd import GeneratorProgram, ProgramGenerator, native as N
from plonky2_goldibear_amd import generator_program as GP
from plonky2_goldibear_amd.gate_program import field_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc


@pytest.mark.parametrize("field", sorted(PC.FIELDS))
def test_the_mirror_runs_what_it_packs(field):
    p = field_order(field)
    # EqualityGenerator and NonzeroTestGenerator, branch-free
    eq = GeneratorProgram.from_function(lambda d, c, ops: [ops.is_zero(d[0] - d[1]), ops.inv_or_zero(d[0] - d[1])], 2, 2, 0, field)
    assert eq.evaluate([5, 5]) == [1, 0] and eq.evaluate([7, 5]) == [0, pow(2, p - 2, p)]
    nz = GeneratorProgram.from_function(lambda d, c, ops: [ops.inv_or_zero(d[0]) + ops.is_zero(d[0])], 1, 1, 0, field)
    assert nz.evaluate([0]) == [1] and nz.evaluate([p - 1]) == [p - 1]
    k = GeneratorProgram.from_function(lambda d, c, ops: [d[0] * d[1] * c[0] + 3, 7, d[1]], 2, 3, 1, field)
    assert (k.num_in, k.num_out, k.num_constants) == (2, 3, 1) and k.words[1] == 3
    assert k.evaluate([p - 1, 2], [5]) == [(3 - 10) % p, 7, 2]
    # the opcode field: codes 0-3 in the low bits with bits 56-63 zero, the unary operations above them
    for word in k.instructions:
        assert word >> 56 == 0
    assert {GP.decode_opcode(w) for w in eq.instructions} == {GP.OP_SUB, GP.OP_IS_ZERO, GP.OP_INV_OR_ZERO, GP.OP_OUT}
    assert all(w >> 60 == 0 and (w >> 32) & 0xFFFFFF == 0 for w in eq.instructions if GP.decode_opcode(w) >= GP.OP_OUT)
    sq = GeneratorProgram.from_function(lambda d, c, ops: [ops.sqrt(d[0])], 1, 1, 0, field)
    z = GP.TWO_ADIC_GENERATOR[field]
    assert pow(z, 1 << (GP.TWO_ADICITY[field] - 1), p) == p - 1
    for x in (0, 1, 4, z * z % p, pow(12345, 2, p)):
        r = sq.evaluate([x])[0]
        assert r * r % p == x
    with pytest.raises(GP.NoSquareRootError, match="unwrap"):
        sq.evaluate([PC.NON_RESIDUE[field]])
    with pytest.raises(GP.InvertZeroError, match="Tried to invert zero"):
        GeneratorProgram.from_function(lambda d, c, ops: [ops.inv(d[0])], 1, 1, 0, field).evaluate([0])
    with pytest.raises(ValueError):
        ProgramGenerator("g", k, [("v", 0), ("v", 1)], [("v", 2)] * 3)          # reads constants: needs its row
    assert PC.all_registers_program(field).num_regs == 32


@pytest.mark.parametrize("field", sorted(PC.FIELDS))
def test_build_leaves_a_program_generator_as_it_is(field):
    """one ProgramGenerator handed to two builders whose rows carry different constants: each built circuit reads its own"""
    import gadget_cases as GA
    import generator_program_circuits as GPC
    from plonky2_goldibear_amd import GateProgram, ProgramGate
    from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, PartialWitness, wire
    p = field_order(field)
    constraints = GateProgram.from_constraints(lambda w, c: [w[2] - (w[0] * w[1] * c[0] + 3)], num_wires=3, num_constants=1, field=field)
    gate = ProgramGate("MulAddThreeGate", constraints)                      # no generators of its own
    program = GPC.mul_add_three_gate(field).generators(0, [0])[0].generator_program
    shared = ProgramGenerator("MulAddThreeGenerator", program, [wire(0, 0), wire(0, 1)], [wire(0, 2)], row=0)
    built = []
    for k in (5, 7):
        b = CircuitBuilder(GA.config(field))
        assert b.add_gate(gate, constants=[k]) == 0
        b.add_simple_generator(shared)
        built.append(b.build())
    assert shared.constants == []
    pw = PartialWitness()
    pw.set_target(wire(0, 0), p - 1)
    pw.set_target(wire(0, 1), 11)
    for k, c in zip((5, 7), built):
        wires, _ = c.generate_witness(pw)
        assert int(wires[2, 0]) == (k * (p - 1) * 11 + 3) % p


@pytest.mark.parametrize("field", sorted(PC.FIELDS))
def test_constants_columns_lie_behind_every_selector_column(field):
    """a gate set that needs two selector columns: constants_columns, what gb_circuit_set_generators receives, starts behind both,
    and holds at a program generator's row the constants its mirror reads"""
    import gadget_cases as GA
    import generator_program_circuits as GPC
    b, _ = GPC.mul_add_three_circuit(GA.config(field), 4, public_output=True)
    c = b.build()
    assert c.num_selectors == 2 and c.degree_bits == 3
    gens = [g for g in c.generators if getattr(g, "generator_program", None) is not None]
    assert [g.row for g in gens] == [0, 1, 2, 3]
    for g in gens:
        assert [int(c.constants_columns[j][g.row]) for j in range(g.generator_program.num_constants)] == g.constants == [5 + 3 * g.row]
        assert int(c.constants_sigmas[1][g.row]) != g.constants[0]          # the second selector column holds the gate's index
    one, _ = GPC.mul_add_three_circuit(GA.config(field), 5)
    assert one.build().num_selectors == 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    shim = os.path.join(ROOT, "tests", "host_shim")
    out = tmp_path_factory.mktemp("generator_programs_host") / "generator_programs"
    subprocess.run([CLANG, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim, "-I", os.path.join(ROOT, "tests", "sanitize"),
                    "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(out), os.path.join(shim, "generator_programs.cpp")],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.parametrize("field", sorted(PC.FIELDS))
def test_the_interpreter_on_the_host_equals_the_mirror(exe, tmp_path, field):
    cases, check = PC.all_cases(field)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    check(GC.read_values(np.fromfile(dst, dtype=np.uint64), len(cases)))
