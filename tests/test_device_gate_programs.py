"""gates::run_program<F, BaseAlg<F>> on the GPU with its register file in LDS (csrc/gates.hpp LdsRegs - the way k_gate_programs
runs a constraint program), built for gfx950 from the headers (tests/device/gate_program_eval.hip) and run on caller-supplied
rows: the fields' carry-edge words and random words as wires and constants.  The emitted constraints must equal
GateProgram.evaluate, the restatement on Python integers.  Programs: gates of tests/gate_programs.py and a synthetic one that
uses all 32 registers, all four operand spaces and the literals 0, 1, p - 1, 2^32 - 1 and 2^32 (reduced mod p for BabyBear); it is
written word by word, because the assembler folds a literal 0 away and the device has to read one.
Row counts 1, 63, 64, 65, 300: a partial wave, the wave boundaries, more than one workgroup."""
import os
import subprocess

import numpy as np
import pytest

from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import recursion_gates as R
from plonky2_goldibear_amd.gate_program import GATE_PROGRAM, OP_ADD, OP_EMIT, OP_MUL, OP_SUB, SPACE_CONST, SPACE_LIT, SPACE_REG, SPACE_WIRE, GateProgram

from plonky2_goldibear_amd.prover import VerifierCircuitData

import gate_programs as GP
from wired_circuits import edge_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {N.GB_GOLDILOCKS: GL, N.GB_BABYBEAR: BB}


def ins(op, dst=0, a=0, b=0):
    return op | dst << 2 | a << 8 | b << 32


def opnd(space, index):
    return space | index << 2


LIT_ZERO = 0   # index of the literal 0 in the synthetic program's table


def all_registers_program(field):
    """Written word by word (the assembler would fold a literal 0 away): r0..r30 = w[i] * c[i % 2] + lit[i % 5] stay live to the
    end next to r31, which holds the running sum and then each further constraint; every literal is read by ADD, SUB and MUL."""
    p = GP.P[field]
    lits = [0, 1, p - 1, (2**32 - 1) % p, 2**32 % p]
    reg, wire, const, lit = [lambda i, s=s: opnd(s, i) for s in (SPACE_REG, SPACE_WIRE, SPACE_CONST, SPACE_LIT)]
    code = []
    for i in range(31):
        code += [ins(OP_MUL, i, wire(i), const(i % 2)), ins(OP_ADD, i, reg(i), lit(i % 5))]
    code += [ins(OP_ADD, 31, reg(0), reg(1))] + [ins(OP_ADD, 31, reg(31), reg(i)) for i in range(2, 31)] + [ins(OP_EMIT, 0, reg(31))]
    for i in range(15):
        code += [ins(OP_MUL, 31, reg(i), reg(30 - i)), ins(OP_SUB, 31, reg(31), lit(i % 5)), ins(OP_MUL, 31, lit((i + 2) % 5), reg(31)),
                 ins(OP_EMIT, 0, reg(31))]
    code += [ins(OP_MUL, 31, lit(LIT_ZERO), wire(0)), ins(OP_EMIT, 0, reg(31)),                       # 0 * w0
             ins(OP_SUB, 31, lit(LIT_ZERO), reg(7)), ins(OP_ADD, 31, reg(31), lit(LIT_ZERO)), ins(OP_EMIT, 0, reg(31)),   # 0 - r7 + 0
             ins(OP_EMIT, 0, lit(LIT_ZERO)), ins(OP_EMIT, 0, wire(30)), ins(OP_EMIT, 0, const(1))]
    num_constraints = sum(1 for w in code if w & 3 == OP_EMIT)
    return GateProgram([31 | 2 << 32, num_constraints | 4 << 32, 32 | len(lits) << 32, len(code)] + lits + code, field)


def programs(field):
    gl = field == N.GB_GOLDILOCKS
    gates = [R.RandomAccessGate(4 if gl else 3, 4, 2, field), R.ReducingExtensionGate(33 if gl else 7, field), R.BaseSumGate(10, 4)]
    return [all_registers_program(field)] + [GP.program_of(g, field) for g in gates]


def test_the_synthetic_program_uses_every_register_and_space():
    for field in FIELDS:
        prog = all_registers_program(field)
        p = GP.P[field]
        assert prog.num_regs == 32 and prog.num_instrs == len(prog.instructions)
        assert prog.literals == [0, 1, p - 1, (2**32 - 1) % p, 2**32 % p] and len(set(prog.literals)) == 5
        assert prog.literals[LIT_ZERO] == 0
        written, read = set(), {s: set() for s in (SPACE_REG, SPACE_WIRE, SPACE_CONST, SPACE_LIT)}
        for word in prog.instructions:
            op = word & 3
            for shift in (8,) if op == OP_EMIT else (8, 32):
                o = (word >> shift) & 0xFFFFFF
                read[o & 3].add(o >> 2)
            if op != OP_EMIT:
                written.add((word >> 2) & 63)
        assert written == read[SPACE_REG] == set(range(32))
        assert read[SPACE_WIRE] == set(range(31)) and read[SPACE_CONST] == {0, 1}
        assert read[SPACE_LIT] == set(range(5))                  # the literal 0 among them
        # the words are well formed: evaluate() raises on a register read before it is written or an index out of range
        out = prog.evaluate(list(range(1, 32)), [3, 5])
        assert len(out) == prog.num_constraints == 21 and out[16] == 0 and out[18] == 0
        # and the library's own validation accepts them (gb_verifier_create_programs touches no device)
        hout = 4 if field == N.GB_GOLDILOCKS else 8
        VerifierCircuitData(3, [(0, 0, 0, 0, 2, 0, 0), (GATE_PROGRAM, 0, 0, 0, 2, 0, 0)], np.ones(80, dtype=np.uint64),
                            np.zeros((16, hout), dtype=np.uint64), np.zeros(hout, dtype=np.uint64), field=field, programs=[prog])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("gate_program_eval") / "gate_program_eval"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "gate_program_eval.hip")], check=True, capture_output=True, text=True)
    return str(out)


def rows(field, prog, nrows, seed):
    """[num_wires + num_constants][nrows]: the edge words first (every column starts at another one), then random words"""
    F = FIELDS[field]
    ev = np.array(edge_values(F), dtype=np.uint64)
    ncols = prog.num_wires + prog.num_constants
    vals = F.fill(seed, ncols * nrows).astype(np.uint64).reshape(ncols, nrows)
    k = min(nrows, len(ev))
    for col in range(ncols):
        vals[col, :k] = np.roll(ev, -col)[:k]
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_device_interpreter_equals_the_python_restatement(exe, tmp_path, field, nrows):
    for k, prog in enumerate(programs(field)):
        vals = rows(field, prog, nrows, 100 * field + k)
        head = [field, nrows, prog.num_wires, prog.num_constants, prog.num_constraints, prog.num_regs, prog.num_literals, prog.num_instrs]
        src, dst = tmp_path / ("in%d.bin" % k), tmp_path / ("out%d.bin" % k)
        np.concatenate([np.array(head + prog.literals + prog.instructions, dtype=np.uint64), vals.reshape(-1)]).tofile(src)
        out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        got = np.fromfile(dst, dtype=np.uint64).reshape(prog.num_constraints, nrows)
        nw = prog.num_wires
        for j in range(nrows):
            want = prog.evaluate([int(x) for x in vals[:nw, j]], [int(x) for x in vals[nw:, j]])
            assert [int(x) for x in got[:, j]] == want, (k, j)
