"""Constraint systems over committed oracles, the host side (plonky2_goldibear_amd/constraints.py, csrc/constraint_system.hpp,
gb_constraint_eval): the assembler's words round-trip; every refusal of the validator is produced from Python for both fields
(through gb_constraint_eval, which needs no device; the refusals that need a live oracle are in tests/test_gpu_constraint_quotient.py);
the degree rule at its boundary; and gb_constraint_eval against ConstraintProgram.evaluate over the extension field.  No GPU."""
import numpy as np
import pytest

import constraint_cases as CC
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.constraints import ConstraintProgram, cell_word, constraint_eval, pack_constraint_programs
from wired_circuits import edge_values

FIELDS = [pytest.param(GL, N.GB_GOLDILOCKS, id="goldilocks"), pytest.param(BB, N.GB_BABYBEAR, id="babybear")]
OP_ADD, OP_SUB, OP_MUL, OP_EMIT = 0, 1, 2, 3
REG, CELL, INPUT, LIT = 0, 1, 2, 3


def ins(op, dst, a, b=(0, 0)):
    return op | dst << 2 | (a[0] | a[1] << 2) << 8 | (b[0] | b[1] << 2) << 32


def raw_program(cells, num_params, lits, instrs, num_constraints=None, degree=8, num_regs=4, num_inputs=None):
    emits = sum(1 for w in instrs if w & 3 == OP_EMIT)
    return [len(cells) | (3 + num_params if num_inputs is None else num_inputs) << 32,
            (emits if num_constraints is None else num_constraints) | degree << 32, num_regs | len(lits) << 32, len(instrs)] + \
        list(lits) + [cell_word(*c) for c in cells] + list(instrs)


def grand_product(tag):
    """Z(wx) (b + gamma) - Z(x) (a + gamma) and L_first (Z - 1): a, b, Z in three oracles, gamma a param"""
    return ConstraintProgram.from_constraints(
        lambda cell, param, x, l_first, l_last: [cell[3] * (cell[1] + param[0]) - cell[2] * (cell[0] + param[0]), l_first * (cell[2] - 1)],
        cells=[(0, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1)], num_params=2, field=tag)


def reads_everything(tag):
    """X, L_first, L_last and a param in one program"""
    return ConstraintProgram.from_constraints(
        lambda cell, param, x, l_first, l_last: [x * cell[0] - l_last * param[1] + 5, (l_first + l_last) * (cell[1] - x) * cell[0], param[0] - param[1]],
        cells=[(1, 0, 2), (0, 3, 0)], num_params=2, field=tag)


@pytest.mark.parametrize("F,tag", FIELDS)
def test_assembled_words_round_trip(F, tag):
    pr = grand_product(tag)
    assert pr.cells == [(0, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1)] and (pr.num_cells, pr.num_inputs, pr.num_params) == (4, 5, 2)
    assert pr.num_constraints == 2 and pr.degree == 2
    again = ConstraintProgram(pr.words, tag)
    assert again.words == pr.words and len(pr.words) == 4 + pr.num_literals + 4 + pr.num_instrs
    words, offsets = pack_constraint_programs([pr, reads_everything(tag)])
    assert list(offsets) == [0, len(pr.words), len(pr.words) + len(reads_everything(tag).words)]
    assert [int(x) for x in words[:len(pr.words)]] == pr.words
    # a param has degree 0, the built-in inputs degree 1
    assert reads_everything(tag).degree == 3
    # evaluate: the packed words against the expressions, on integers
    P = F.P
    vals = [3, P - 1, 5, 7]
    got = pr.evaluate(vals, [11, 0], 2, 9, 0)
    assert got == [(7 * (P - 1 + 11) - 5 * (3 + 11)) % P, 9 * 4 % P]
    assert cell_word(3, 0x12345678, 0xFFFF) == 3 | 0x12345678 << 16 | 0xFFFF << 48
    with pytest.raises(ValueError):
        cell_word(1 << 16, 0, 0)
    with pytest.raises(ValueError, match="degree"):
        ConstraintProgram.from_constraints(lambda c, p, x, lf, ll: [c[0] * c[0] * x], cells=[(0, 0, 0)], num_params=0, field=tag, degree=2)


def _eval_ref(F, programs, cell_values, params, zeta, alphas, degree_bits):
    _, lf, ll = CC.ext_inputs(F, degree_bits, zeta)
    cons, at = [], 0
    for pr in programs:
        vals = [CC.ExtInt(F, v) for v in cell_values[at:at + pr.num_cells]]
        at += pr.num_cells
        got = pr.evaluate(vals, list(params), CC.ExtInt(F, zeta), CC.ExtInt(F, lf), CC.ExtInt(F, ll), coerce=lambda v: v)
        cons += [c.v if isinstance(c, CC.ExtInt) else F.efrom(c) for c in got]
    return [CC.fold_ext(F, cons, a) for a in alphas]


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("zeta_kind", ["random", "edges"])
@pytest.mark.parametrize("F,tag", FIELDS)
def test_constraint_eval_matches_evaluate_over_the_extension(F, tag, zeta_kind, nch):
    """two programs (the numbering crosses a program boundary), one of them reading X, L_first, L_last and a param"""
    degree_bits = 5
    programs = [grand_product(tag), reads_everything(tag)]
    rng = np.random.default_rng(7 + nch)
    ev = edge_values(F)
    pick = (lambda: int(rng.integers(0, F.P, dtype=np.uint64))) if zeta_kind == "random" else (lambda: ev[int(rng.integers(0, len(ev)))])
    zeta = tuple(pick() for _ in range(F.D))
    if zeta_kind == "edges":
        zeta = (zeta[0],) + zeta[1:-1] + (F.P - 1,)   # outside the base field, so outside the subgroup
    cell_values = [tuple(pick() for _ in range(F.D)) for _ in range(6)]
    params = [pick(), ev[-1]]
    alphas = [pick() for _ in range(nch - 1)] + [F.P - 1]
    got = constraint_eval(tag, degree_bits, programs, cell_values, params, zeta, alphas)
    want = _eval_ref(F, programs, cell_values, params, zeta, alphas, degree_bits)
    assert got.dtype == F.dtype and [tuple(int(x) for x in r) for r in got] == [tuple(w) for w in want]


def _refused(tag, programs, match, degree_bits=4, num_params=1, cell_values=None, params=None, zeta=None, alphas=(3,)):
    d = 2 if tag == N.GB_GOLDILOCKS else 4
    total = sum(int(p[0]) & 0xFFFFFFFF for p in programs)
    with pytest.raises(N.ShapeError, match=match):
        constraint_eval(tag, degree_bits, programs, [(1,) * d] * total if cell_values is None else cell_values,
                        [2] * num_params if params is None else params, (5,) + (1,) * (d - 1) if zeta is None else zeta, list(alphas))


@pytest.mark.parametrize("F,tag", FIELDS)
def test_every_malformed_table_is_refused(F, tag):
    cells = [(0, 0, 0), (1, 2, 3)]
    good = raw_program(cells, 1, [7], [ins(OP_MUL, 0, (CELL, 0), (INPUT, 3)), ins(OP_ADD, 1, (REG, 0), (LIT, 0)), ins(OP_EMIT, 0, (REG, 1))])
    d = 2 if tag == N.GB_GOLDILOCKS else 4
    assert constraint_eval(tag, 4, [good], [(1,) * d] * 2, [2], (5,) + (1,) * (d - 1), [3]).shape == (1, d)

    def prog(instrs, **kw):
        return raw_program(cells, 1, [7], instrs, **kw)
    emit0 = ins(OP_EMIT, 0, (CELL, 0))
    # what gb_circuit_create_programs refuses
    _refused(tag, [], "at least one program")
    _refused(tag, [good] * 17, "more than 16")
    _refused(tag, [good[:3]], "is no program")
    _refused(tag, [good[:-1]], "the header describes")
    _refused(tag, [good + [emit0]], "the header describes")
    _refused(tag, [prog([emit0], num_regs=33)], "over the limits")
    _refused(tag, [raw_program(cells, 1, [0] * 257, [emit0])], "over the limits")
    _refused(tag, [[good[0], good[1], good[2], good[3] | 1 << 32] + good[4:]], "header word 3")
    _refused(tag, [prog([ins(OP_EMIT, 0, (REG, 0))])], "program 0 instruction 0: register 0 is read before it is written")
    _refused(tag, [prog([ins(OP_ADD, 4, (CELL, 0), (CELL, 1)), emit0])], "instruction 0: register 4 of 4")
    _refused(tag, [prog([ins(OP_ADD, 0, (REG, 9), (CELL, 1)), emit0])], "register 9 of 4")
    _refused(tag, [prog([ins(OP_EMIT, 0, (CELL, 2))])], "instruction 0: cell 2 of 2")
    _refused(tag, [prog([ins(OP_EMIT, 0, (INPUT, 4))])], "input 4 of 4")
    _refused(tag, [prog([ins(OP_EMIT, 0, (LIT, 1))])], "literal 1 of 1")
    _refused(tag, [raw_program(cells, 1, [F.P], [emit0])], "literal 0 is not canonical")
    _refused(tag, [prog([emit0, emit0], num_constraints=1)], "2 EMITs")
    _refused(tag, [prog([ins(OP_EMIT, 1, (CELL, 0))])], "EMIT with a destination")
    _refused(tag, [prog([emit0 | 1 << 56])], "bits 56-63")
    _refused(tag, [prog([ins(OP_MUL, 0, (CELL, 0), (CELL, 1)), ins(OP_EMIT, 0, (REG, 0))], degree=1)], "constraint 0 has degree bound 2")
    _refused(tag, [good, prog([ins(OP_EMIT, 0, (CELL, 7))])], "program 1 instruction 0: cell 7")
    # what the cells and the inputs add
    _refused(tag, [raw_program([(16, 0, 0)], 1, [], [emit0])], "program 0 cell 0: oracle_index 16 of 16")
    _refused(tag, [raw_program([(0, 0, 16)], 1, [], [emit0])], "cell 0: row_offset 16 is not below n = 16")
    _refused(tag, [prog([emit0], num_inputs=5)], "num_inputs is 5")
    _refused(tag, [good], "param 0 is not below p", params=[F.P])
    _refused(tag, [good], "alpha 1 is not below p", alphas=(1, F.P))
    _refused(tag, [good], "num_challenges 0", alphas=())
    _refused(tag, [good], "num_challenges 17", alphas=(1,) * 17)
    _refused(tag, [good], "non-canonical coordinate in zeta", zeta=(F.P,) + (0,) * (d - 1))
    _refused(tag, [good], "non-canonical coordinate in cell_values", cell_values=[(1,) * d, (F.P,) + (0,) * (d - 1)])
    with pytest.raises(N.GoldibearError, match="subgroup") as e:
        constraint_eval(tag, 4, [good], [(1,) * d] * 2, [2], F.efrom(F.two_adic_generator(4)), [3])
    assert e.value.status == N.GB_ERR_OPENING_IN_SUBGROUP
    # the message of a null-context call is there to be read
    assert N.load().gb_constraint_eval(None, 7, 4, None, None, 0, None, None, 0, None, None, 0, None) == N.GB_ERR_INVALID
    assert b"unknown field" in N.load().gb_last_error(None)
