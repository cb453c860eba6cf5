"""GB_GATE_PROGRAM on the host: custom gates handed over as constraint programs (include/goldibear_gpu.h "constraint
programs", plonky2_goldibear_amd/gate_program.py).  gb_verifier_create_programs touches no device, so all of this runs
without a GPU.

The reference's own serialized recursion proof (tests/golden/recursive_verifier_gl_*.bin) must still verify when the gates of
its circuit are replaced by programs (tests/gate_programs.py writes them), and must fail the vanishing identity as soon as one
operand of one program is changed: the interpreter (csrc/gates.hpp run_program over ExtAlg) is pinned by the reference's numbers
exactly as the built-in evaluators are."""
import os

import numpy as np
import pytest

from oracle import verifier as V
from plonky2_goldibear_amd import VerifierCircuitData, VerifyError, native as N
from plonky2_goldibear_amd import recursion_gates as R
from plonky2_goldibear_amd.circuit_builder import ArithmeticGate
from plonky2_goldibear_amd.gate_program import (GATE_PROGRAM, HEADER_WORDS, OP_ADD, OP_EMIT, OP_MUL, OP_SUB, SPACE_CONST, SPACE_LIT,
                                                SPACE_REG, SPACE_WIRE, GateProgram)

import gate_programs as GP
from test_abi_verify_fixture import _fixture_circuit

GL = N.GB_GOLDILOCKS
# gb_gate.kind of the eight fixture gates the helper restates -> the gate object of (param, param2, param3)
FIXTURE_KINDS = {
    3: lambda p, p2, p3: ArithmeticGate(p),
    6: lambda p, p2, p3: R.ArithmeticExtensionGate(p, GL),
    7: lambda p, p2, p3: R.MulExtensionGate(p, GL),
    8: lambda p, p2, p3: R.BaseSumGate(p, p2 or 2),
    9: lambda p, p2, p3: R.ReducingGate(p, GL),
    10: lambda p, p2, p3: R.ReducingExtensionGate(p, GL),
    11: lambda p, p2, p3: R.RandomAccessGate(p, p2, p3, GL),
    12: lambda p, p2, p3: R.PoseidonMdsGate(),
}


@pytest.fixture(scope="module")
def fixture_gates(golden_dir):
    common = open(os.path.join(golden_dir, "recursive_verifier_gl_common_data.bin"), "rb").read()
    return [tuple(g) for g in V.read_gates(common, V.read_common_data(common))]


def as_programs(gates, kinds):
    """the gate table with the entries of `kinds` turned into program gates, and their programs in table order"""
    out, programs = [], []
    for g in gates:
        g = tuple(g) + (0,) * (7 - len(g))
        if g[0] in kinds:
            programs.append(GP.program_of(FIXTURE_KINDS[g[0]](g[1], g[5], g[6]), GL))
            g = (GATE_PROGRAM, len(programs) - 1) + g[2:5] + (0, 0)
        out.append(g)
    return out, programs


def test_the_fixture_has_the_eight_gates(fixture_gates):
    assert set(FIXTURE_KINDS) <= {g[0] for g in fixture_gates}


@pytest.mark.parametrize("kinds", [(k,) for k in sorted(FIXTURE_KINDS)] + [tuple(sorted(FIXTURE_KINDS))])
def test_reference_proof_verifies_with_gates_as_programs(golden_dir, fixture_gates, kinds):
    gates, programs = as_programs(fixture_gates, kinds)
    assert len(programs) == len(kinds)
    circ, cd, raw = _fixture_circuit(golden_dir, gates=gates, programs=programs)
    assert circ.verify(raw)
    assert circ.verify_compressed(circ.compress(raw))
    circ.free()


def _mutated(prog):
    """one wire operand of the first instruction that has one, moved to the next wire column"""
    words = list(prog.words)
    first = HEADER_WORDS + prog.num_literals
    for i in range(first, len(words)):
        for shift in (8, 32):
            o = (words[i] >> shift) & 0xFFFFFF
            if (o & 3) == SPACE_WIRE and not (shift == 32 and (words[i] & 3) == OP_EMIT):
                new = SPACE_WIRE | (((o >> 2) + 1) % prog.num_wires) << 2
                words[i] = words[i] & ~(0xFFFFFF << shift) | new << shift
                return GateProgram(words, prog.field)
    raise AssertionError("no wire operand")


@pytest.mark.parametrize("kind", sorted(FIXTURE_KINDS))
def test_every_program_is_pinned(golden_dir, fixture_gates, kind):
    gates, programs = as_programs(fixture_gates, (kind,))
    circ, cd, raw = _fixture_circuit(golden_dir, gates=gates, programs=[_mutated(programs[0])])
    with pytest.raises(VerifyError, match="vanishing"):
        circ.verify(raw)
    circ.free()


def test_a_changed_literal_is_pinned(golden_dir, fixture_gates):
    gates, programs = as_programs(fixture_gates, (12,))   # PoseidonMdsGate: the MDS entries are its literals
    words = list(programs[0].words)
    words[HEADER_WORDS] = (words[HEADER_WORDS] + 1) % GP.P[GL]
    circ, cd, raw = _fixture_circuit(golden_dir, gates=gates, programs=[words])
    with pytest.raises(VerifyError, match="vanishing"):
        circ.verify(raw)


# ---------------------------------------------------------------------------------------------- the assembler
@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_assembler_equals_direct_evaluation(field):
    p = GP.P[field]
    rng = np.random.default_rng(11 + field)
    for gate in GP.helper_gates(field):
        fn = GP.constraints_of(gate, field)
        prog = GateProgram.from_constraints(fn, gate.num_wires, gate.num_constants, field)
        assert prog.num_regs <= 32 and prog.degree == gate.degree and prog.num_constraints == gate.num_constraints, gate.id
        for _ in range(50):
            w = [int(x) for x in rng.integers(0, p, gate.num_wires, dtype=np.uint64)]
            c = [int(x) for x in rng.integers(0, p, gate.num_constants, dtype=np.uint64)]
            assert prog.evaluate(w, c) == [int(v) % p for v in fn(w, c)], gate.id
        # the same gate written twice (two separate runs of the function, constraint by constraint): every subexpression is
        # shared, only the EMITs double
        twice = GateProgram.from_constraints(lambda w, c: [e for pair in zip(fn(w, c), fn(w, c)) for e in pair], gate.num_wires,
                                             gate.num_constants, field)
        assert twice.num_instrs - twice.num_constraints == prog.num_instrs - prog.num_constraints, gate.id
        assert twice.num_regs <= 32


def test_assembler_limits():
    with pytest.raises(ValueError, match="registers"):   # 40 products, all live until the last constraint
        GateProgram.from_constraints(lambda w, c: (lambda t: [sum(t)] + t)([w[i] * w[i + 1] for i in range(40)]), 41, 0, GL)
    with pytest.raises(ValueError, match="degree"):
        GateProgram.from_constraints(lambda w, c: [w[0] * w[1] * w[2]], 3, 0, GL, degree=2)
    with pytest.raises(IndexError):
        GateProgram.from_constraints(lambda w, c: [w[3]], 3, 0, GL)


# ---------------------------------------------------------------------------------------------- validation at create
def opnd(space, index):
    return space | index << 2


def ins(op, dst=0, a=0, b=0):
    return op | dst << 2 | a << 8 | b << 32


def program(instrs, num_wires=4, num_constants=1, num_constraints=1, degree=2, num_regs=2, lits=(5,)):
    return [num_wires | num_constants << 32, num_constraints | degree << 32, num_regs | len(lits) << 32, len(instrs)] + list(lits) + list(instrs)


W0, W1, R0, R1 = opnd(SPACE_WIRE, 0), opnd(SPACE_WIRE, 1), opnd(SPACE_REG, 0), opnd(SPACE_REG, 1)
GOOD = [ins(OP_MUL, 0, W0, W1), ins(OP_ADD, 1, R0, opnd(SPACE_LIT, 0)), ins(OP_SUB, 0, R1, opnd(SPACE_CONST, 0)), ins(OP_EMIT, 0, R0)]


def make_verifier(programs, gates=None, **kw):
    """an 8-row Goldilocks verifier object over [NoopGate, program 0] in one selector group"""
    gates = gates or [(0, 0, 0, 0, 2, 0, 0), (GATE_PROGRAM, 0, 0, 0, 2, 0, 0)]
    return VerifierCircuitData(3, gates, np.ones(80, dtype=np.uint64), np.zeros((16, 4), dtype=np.uint64),
                               np.zeros(4, dtype=np.uint64), programs=programs, **kw)


def test_a_valid_hand_written_program_is_accepted():
    make_verifier([program(GOOD)]).free()
    assert GateProgram(program(GOOD), GL).evaluate([3, 4, 0, 0], [7]) == [3 * 4 + 5 - 7]


BAD_PROGRAMS = {
    "register read before it is written": program([ins(OP_ADD, 0, R1, W0)] + GOOD[1:]),
    "register index out of range (destination)": program([ins(OP_MUL, 2, W0, W1)] + GOOD[1:]),
    "register index out of range (operand)": program(GOOD[:3] + [ins(OP_EMIT, 0, opnd(SPACE_REG, 2))]),
    "wire index out of range": program([ins(OP_MUL, 0, W0, opnd(SPACE_WIRE, 4))] + GOOD[1:]),
    "constant index out of range": program(GOOD[:2] + [ins(OP_SUB, 0, R1, opnd(SPACE_CONST, 1))] + GOOD[3:]),
    "literal index out of range": program(GOOD[:1] + [ins(OP_ADD, 1, R0, opnd(SPACE_LIT, 1))] + GOOD[2:]),
    "non-canonical literal": program(GOOD, lits=(GP.P[GL],)),
    "fewer EMITs than constraints": program(GOOD, num_constraints=2),
    "more EMITs than constraints": program(GOOD + [ins(OP_EMIT, 0, R0)]),
    "too many registers": program(GOOD, num_regs=33),
    "too many instructions": program(GOOD[:3] * 1366 + GOOD[3:]),
    "too many literals": program(GOOD, lits=(1,) * 257),
    "too many constraints": program(GOOD[:3] + GOOD[3:] * 1025, num_constraints=1025),
    "degree bound above the declared degree": program(GOOD, degree=1),
    "declared degree plus filter degree above the quotient degree factor": program(GOOD, degree=9),
}


@pytest.mark.parametrize("name", sorted(BAD_PROGRAMS))
def test_validation_rejects(name):
    with pytest.raises(N.ShapeError, match=r"program 0\b"):
        make_verifier([BAD_PROGRAMS[name]])


def test_validation_names_the_instruction():
    with pytest.raises(N.ShapeError, match=r"program 1 instruction 2\b.*constant 1"):
        make_verifier([program(GOOD), BAD_PROGRAMS["constant index out of range"]])


def test_filter_degree_counts_the_group_and_the_selector_columns():
    noop = (0, 0, 0, 0, 2, 0, 0)
    make_verifier([program(GOOD, degree=8)]).free()                      # 8 + 1 other gate in the group = 9 = 8 + 1
    with pytest.raises(N.ShapeError, match="program 0"):                 # two selector columns: one more factor
        make_verifier([program(GOOD, degree=8)], gates=[noop, (GATE_PROGRAM, 0, 0, 0, 2, 0, 0), (0, 0, 1, 2, 3, 0, 0)], num_selectors=2)


def test_gate_param_must_name_a_program():
    with pytest.raises(N.ShapeError, match="program 1 of 1"):
        make_verifier([program(GOOD)], gates=[(0, 0, 0, 0, 2, 0, 0), (GATE_PROGRAM, 1, 0, 0, 2, 0, 0)])
    with pytest.raises(N.ShapeError, match="more than 16"):
        make_verifier([program(GOOD)] * 17)


def test_truncated_and_misdescribed_tables():
    with pytest.raises(N.ShapeError, match="program 0"):
        make_verifier([program(GOOD)[:-1]])
    with pytest.raises(N.ShapeError, match="program 0"):
        make_verifier([program(GOOD)[:3]])
    with pytest.raises(N.ShapeError, match="program 0 instruction 0"):
        make_verifier([program([GOOD[0] | 1 << 60] + GOOD[1:])])


def test_the_old_entry_point_has_no_program_table():
    gates = [(0, 0, 0, 0, 2, 0, 0), (GATE_PROGRAM, 0, 0, 0, 2, 0, 0)]
    with pytest.raises(N.ShapeError, match="program"):
        make_verifier(None, gates=gates)
    with pytest.raises(N.GoldibearError) as e:      # an unknown kind is still "unsupported", through either entry point
        make_verifier(None, gates=[gates[0], (99, 1, 0, 0, 2, 0, 0)])
    assert e.value.status == N.GB_ERR_UNSUPPORTED
    with pytest.raises(N.GoldibearError) as e:
        make_verifier([program(GOOD)], gates=[gates[0], (99, 1, 0, 0, 2, 0, 0)])
    assert e.value.status == N.GB_ERR_UNSUPPORTED


def test_no_programs_is_the_old_entry_point(golden_dir, fixture_gates):
    circ, cd, raw = _fixture_circuit(golden_dir, programs=[])
    assert circ.verify(raw)
    with pytest.raises(N.ShapeError, match="program 0 of 0"):
        make_verifier([])
