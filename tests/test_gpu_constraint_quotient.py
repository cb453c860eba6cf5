"""gb_constraint_quotient on the device against the restatement on Python integers (tests/constraint_cases.py: the oracle's LDE,
ConstraintProgram.evaluate at every point of the quotient domain, the fold, the division by Z_H, the oracle's coset inverse
transform, the chunks - equal byte for byte), the identity a verifier checks through gb_constraint_eval, a Fibonacci trace proved and
verified end to end through this library alone, and the refusals that need a live oracle.  -m gpu only."""
import numpy as np
import pytest

import constraint_cases as CC
import fri_instances as FI
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, MerkleTree, PolynomialBatch, ShapeError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import prove_openings, verify_fri_proof, verify_fri_proofs
from plonky2_goldibear_amd.constraints import ConstraintProgram, cell_word, constraint_eval, constraint_quotient
from wired_circuits import edge_values

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": GL, "babybear": BB}
RATE_BITS = 3
WIDTHS = (3, 5, 2)          # three oracles of different widths, the second one committed with salts
SALTED = (False, True, False)
OP_ADD, OP_SUB, OP_MUL, OP_EMIT = 0, 1, 2, 3
REG, CELL, INPUT, LIT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def ins(op, dst, a, b=(0, 0)):
    return op | dst << 2 | (a[0] | a[1] << 2) << 8 | (b[0] | b[1] << 2) << 32


def synthetic_program(F, tag, n):
    """32 registers, written word by word: every register is loaded from a cell and a second operand of every space, the
    registers meet in products (degree 2) and one constraint reaches degree 3; row offsets 0, 1, 2 and n - 1"""
    cells = [(0, 0, 0), (0, 2, 1), (1, 4, 2), (1, 0, n - 1), (2, 1, 0), (2, 0, 1), (0, 1, n - 1)]
    lits = [F.P - 1, 3, (F.P + 1) // 2]
    w = []
    for r in range(32):
        second = [(CELL, (r + 3) % len(cells)), (LIT, r % 3), (INPUT, 3 + r % 2), (INPUT, r % 3)][r % 4]
        w.append(ins(OP_ADD if r & 1 else OP_SUB, r, (CELL, r % len(cells)), second))
    for r in range(16):
        w += [ins(OP_MUL, r, (REG, r), (REG, 31 - r)), ins(OP_EMIT, 0, (REG, r))]
    for r in range(16):
        w += [ins(OP_ADD, 16 + r, (REG, 16 + r), (REG, r)), ins(OP_EMIT, 0, (REG, 16 + r))]
    w += [ins(OP_MUL, 0, (REG, 0), (CELL, 6)), ins(OP_EMIT, 0, (REG, 0)), ins(OP_EMIT, 0, (LIT, 1)), ins(OP_EMIT, 0, (INPUT, 4))]
    words = [len(cells) | 5 << 32, 35 | 3 << 32, 32 | len(lits) << 32, len(w)] + lits + [cell_word(*c) for c in cells] + w
    return ConstraintProgram(words, tag)


def system(F, tag, n, synthetic=True):
    """the programs of the parity tests over the three oracles, two params (gamma and one more)"""
    grand = ConstraintProgram.from_constraints(
        lambda cell, param, x, l_first, l_last: [cell[3] * (cell[1] + param[0]) - cell[2] * (cell[0] + param[0]), l_first * (cell[2] - 1)],
        cells=[(0, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1)], num_params=2, field=tag)
    tail = ConstraintProgram.from_constraints(
        lambda cell, param, x, l_first, l_last: [l_last * (cell[0] - param[1]) + x * cell[1] * cell[2], x * x * x - cell[1]],
        cells=[(1, 3, 2), (2, 1, n - 1), (0, 2, 0)], num_params=2, field=tag)
    return ([synthetic_program(F, tag, n)] if synthetic else []) + [grand, tail]


def witness(F, width, n, seed):
    """carry-edge values next to random ones"""
    ev = np.array(edge_values(F), dtype=F.dtype)
    rng = np.random.default_rng(seed)
    vals = F.fill(seed, width * n).reshape(width, n)
    mask = rng.random((width, n)) < 0.4
    vals[mask] = ev[rng.integers(0, len(ev), size=int(mask.sum()))]
    return vals


_TABLES = {}


def tables(F, degree_bits):
    """per (field, size): the witness, the salts, the programs, and every constraint on the 2^3-blow-up domain - computed once"""
    key = (F.name, degree_bits)
    if key not in _TABLES:
        n, tag = 1 << degree_bits, FI.field_tag(F)
        vals = [witness(F, w, n, 100 * degree_bits + o) for o, w in enumerate(WIDTHS)]
        salts = [F.fill(0x5A17 + o, 4 * (n << RATE_BITS)).reshape(4, -1) if s else None for o, s in enumerate(SALTED)]
        ldes = [CC.lde_natural(F, v, RATE_BITS, s)[1] for v, s in zip(vals, salts)]
        programs = system(F, tag, n, synthetic=degree_bits < 13)
        params = [edge_values(F)[-1], int(F.fill(77, 1)[0])]
        cons = CC.constraint_values(F, programs, ldes, degree_bits, RATE_BITS, 3, params)
        _TABLES[key] = dict(vals=vals, salts=salts, programs=programs, params=params, cons=cons)
    return _TABLES[key]


def commit_all(ctx, F, t):
    return [PolynomialBatch.from_values(ctx, v, RATE_BITS, 0, salts=s, field=FI.field_tag(F)) for v, s in zip(t["vals"], t["salts"])]


def alphas_for(F, nch, seed):
    ev = edge_values(F)
    return [ev[-1]] + [int(x) for x in F.fill(seed, nch - 1)] if nch > 1 else [int(F.fill(seed, 1)[0])]


PARITY = [(2, 1, 1), (2, 3, 2), (6, 1, "slices"), (6, 3, 1), (6, 3, 2), (13, 1, 2), (13, 3, 1)]


@pytest.mark.parametrize("degree_bits,qb,nch", PARITY)
@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_quotient_matches_the_restatement(ctx, field_name, degree_bits, qb, nch):
    """degree_bits 2: below a wave, masked lanes; 6: one wave per coset; 13: the inverse transform in two passes.  qb 1: the
    domain is a strict subset of the LDE.  "slices": 5 challenges (Goldilocks) / 11 (BabyBear), more than a compiled width."""
    F = FIELDS[field_name]
    nch = (5 if F is GL else 11) if nch == "slices" else nch
    t = tables(F, degree_bits)
    alphas = alphas_for(F, nch, 31 * degree_bits + qb)
    want = CC.expected_chunks(F, CC.subsample(t["cons"], 3, qb), degree_bits, qb, alphas)
    oracles = commit_all(ctx, F, t)
    got = constraint_quotient(ctx, oracles, t["programs"], t["params"], alphas, qb)
    assert got.dtype == want.dtype and got.shape == want.shape == (nch << qb, 1 << degree_bits)
    assert got.tobytes() == want.tobytes()
    dev = constraint_quotient(ctx, oracles, t["programs"], t["params"], alphas, qb, device=True)
    assert dev.is_cuda and dev.cpu().numpy().view(F.dtype).tobytes() == want.tobytes()
    for b in oracles:
        b.free()


# ----------------------------------------------------------------------------- the identity
FIB_BITS, FIB_QB = 6, 1


def fib_program(F):
    return ConstraintProgram.from_constraints(CC.fibonacci_constraints(F, FIB_BITS), cells=CC.FIB_CELLS, num_params=2, field=FI.field_tag(F))


def fib_cell_values(F, trace, zeta):
    """the openings of FIB_CELLS through gb_batch_eval_ext: at zeta, and at w zeta for the next row"""
    here = trace.eval_ext(np.array(zeta, dtype=F.dtype))
    there = trace.eval_ext(np.array(F.escale(zeta, F.two_adic_generator(FIB_BITS)), dtype=F.dtype))
    return [here[0], here[1], there[0], there[1]], here, there


def identity_holds(F, prog, chunks, cell_values, params, zeta, alphas):
    folded = constraint_eval(FI.field_tag(F), FIB_BITS, [prog], cell_values, params, zeta, alphas)
    zh = CC.ext_inputs(F, FIB_BITS, zeta)[0]
    R = 1 << FIB_QB
    return [tuple(int(x) for x in folded[c]) == F.emul(zh, CC.quotient_at(F, chunks[c * R:(c + 1) * R], FIB_BITS, zeta))
            for c in range(len(alphas))]


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_identity_on_a_satisfied_and_on_a_broken_trace(ctx, field_name):
    F = FIELDS[field_name]
    tag, n = FI.field_tag(F), 1 << FIB_BITS
    prog = fib_program(F)
    params, alphas = [F.P - 2, 5], alphas_for(F, 2, 9)
    zeta = tuple(int(x) for x in F.fill(4242, F.D))
    values = CC.fibonacci_trace(F, FIB_BITS, *params)
    trace = PolynomialBatch.from_values(ctx, values, RATE_BITS, 1, field=tag)
    chunks = constraint_quotient(ctx, [trace], [prog], params, alphas, FIB_QB)
    # the constraints have degree at most 2 n - 2, so the quotient has degree at most n - 2
    for c in range(2):
        assert not chunks[2 * c + 1].any() and chunks[2 * c][n - 1] == 0 and chunks[2 * c].any()
    cells, _, _ = fib_cell_values(F, trace, zeta)
    assert identity_holds(F, prog, chunks, cells, params, zeta, alphas) == [True, True]
    # one cell changed: the call still succeeds, and the identity fails
    values[1, 17] = (int(values[1, 17]) + 1) % F.P
    broken = PolynomialBatch.from_values(ctx, values, RATE_BITS, 1, field=tag)
    bad_chunks = constraint_quotient(ctx, [broken], [prog], params, alphas, FIB_QB)
    cells, _, _ = fib_cell_values(F, broken, zeta)
    assert identity_holds(F, prog, bad_chunks, cells, params, zeta, alphas) == [False, False]
    trace.free()
    broken.free()


# ----------------------------------------------------------------------------- end to end
def fib_prove(ctx, F, a0, a1, fri):
    """trace commitment -> alphas -> constraint_quotient -> quotient commitment -> zeta -> openings -> prove_openings"""
    tag, nch = FI.field_tag(F), 2
    prog = fib_program(F)
    trace = PolynomialBatch.from_values(ctx, CC.fibonacci_trace(F, FIB_BITS, a0, a1), RATE_BITS, 1, field=tag)
    ch = F.Challenger()
    ch.observe_elements([a0, a1])
    ch.observe_cap(trace.merkle_tree.cap)
    alphas = ch.get_n_challenges(nch)
    chunks = constraint_quotient(ctx, [trace], [prog], [a0, a1], alphas, FIB_QB)
    quotient = PolynomialBatch.from_coeffs(ctx, chunks, RATE_BITS, 1, field=tag)
    ch.observe_cap(quotient.merkle_tree.cap)
    zeta = ch.get_extension_challenge(F.D)
    cells, here, there = fib_cell_values(F, trace, zeta)
    q_open = quotient.eval_ext(np.array(zeta, dtype=F.dtype))
    inst = FI.instance_from_tuples((2, nch << FIB_QB), (False, False), [
        (zeta, [(0, 0), (0, 1)] + [(1, i) for i in range(nch << FIB_QB)]),
        (F.escale(zeta, F.two_adic_generator(FIB_BITS)), [(0, 0), (0, 1)])])
    openings = [np.concatenate([here, q_open]), there]
    for op in openings:
        ch.observe_elements(op.ravel())
    before = FI.challenger_tuple(ch, F)
    proof, _ = prove_openings(inst, [trace, quotient], before, fri)
    caps = [trace.merkle_tree.cap, quotient.merkle_tree.cap]
    trace.free()
    quotient.free()
    return dict(inst=inst, openings=openings, before=before, caps=caps, proof=proof, alphas=alphas, zeta=zeta, cells=cells,
                q_open=q_open, params=[a0, a1], prog=prog)


def fib_verify(F, p, fri):
    """verify_fri_proof plus the identity: folded_c == Z_H(zeta) sum_i zeta^(n i) chunk_(c,i)(zeta), from the opened values"""
    tag = FI.field_tag(F)
    assert verify_fri_proof(p["inst"], p["openings"], p["before"], p["caps"], p["proof"], fri, field=tag)
    folded = constraint_eval(tag, FIB_BITS, [p["prog"]], p["cells"], p["params"], p["zeta"], p["alphas"])
    zh = CC.ext_inputs(F, FIB_BITS, p["zeta"])[0]
    zn, R = F.epow(p["zeta"], 1 << FIB_BITS), 1 << FIB_QB
    for c in range(len(p["alphas"])):
        acc = F.zero
        for i in reversed(range(R)):
            acc = F.eadd(F.emul(acc, zn), tuple(int(x) for x in p["q_open"][c * R + i]))
        if tuple(int(x) for x in folded[c]) != F.emul(zh, acc):
            return False
    return True


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_fibonacci_proved_and_verified_through_this_library(ctx, field_name):
    F = FIELDS[field_name]
    fri = FI.fri_params(FIB_BITS, RATE_BITS, 1, [2, 2], 2, 6)
    proofs = [fib_prove(ctx, F, 3 + 5 * i, (F.P - 1 - i) % F.P, fri) for i in range(8)]
    assert all(fib_verify(F, p, fri) for p in proofs)
    res = verify_fri_proofs(ctx, [(p["inst"], p["openings"], p["before"], p["caps"], p["proof"]) for p in proofs], fri, field=FI.field_tag(F))
    assert [bool(r) for r in res] == [True] * 8
    # another first row is another statement: the identity fails for it
    wrong = dict(proofs[0], params=[4, proofs[0]["params"][1]])
    assert not fib_verify(F, wrong, fri)


# ----------------------------------------------------------------------------- refusals that need a live oracle
@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_refusals_leave_the_context_usable(ctx, field_name):
    F = FIELDS[field_name]
    tag, degree_bits, qb = FI.field_tag(F), 2, 1
    t = tables(F, degree_bits)
    alphas = alphas_for(F, 1, 5)
    want = CC.expected_chunks(F, CC.subsample(t["cons"], 3, qb), degree_bits, qb, alphas)
    oracles = commit_all(ctx, F, t)

    def still_right():
        assert constraint_quotient(ctx, oracles, t["programs"], t["params"], alphas, qb).tobytes() == want.tobytes()

    def refused(match, orcs=None, programs=None, qb_=qb, params=None, alphas_=None):
        with pytest.raises(ShapeError, match=match):
            constraint_quotient(ctx, oracles if orcs is None else orcs, t["programs"] if programs is None else programs,
                                t["params"] if params is None else params, alphas if alphas_ is None else alphas_, qb_)
        still_right()

    def one(cells, fn=lambda cell, param, x, l_first, l_last: [cell[0] - param[0]], degree=None):
        return [ConstraintProgram.from_constraints(fn, cells=cells, num_params=2, field=tag, degree=degree)]
    still_right()
    refused("polynomial_index 5 out of range for oracle 1 .*salt columns", programs=one([(1, WIDTHS[1], 0)]))
    refused("oracle_index 3 of 3", programs=one([(3, 0, 0)]))
    refused("row_offset 4 is not below n = 4", programs=one([(0, 0, 4)]))
    other_size = PolynomialBatch.from_values(ctx, witness(F, 2, 8, 1), RATE_BITS, 0, field=tag)
    refused("oracle 2 differs from oracle 0 in degree_bits or rate_bits", orcs=oracles[:2] + [other_size])
    tree = MerkleTree.new(ctx, witness(F, 3, 4, 2).T.copy(), 0, field=tag)
    refused("oracle 1 is a stand-alone Merkle tree", orcs=[oracles[0], tree._b, oracles[2]])
    refused("oracle 0 is null", orcs=[None] + oracles[1:])
    ctx2 = GpuContext(0)
    foreign = PolynomialBatch.from_values(ctx2, t["vals"][2], RATE_BITS, 0, field=tag)
    refused("oracle 2 belongs to another context or field", orcs=oracles[:2] + [foreign])
    foreign.free()
    ctx2.close()
    other_field = PolynomialBatch.from_values(ctx, witness(BB if F is GL else GL, 2, 4, 3), RATE_BITS, 0, field=N.GB_BABYBEAR if F is GL else N.GB_GOLDILOCKS)
    refused("oracle 2 belongs to another context or field", orcs=oracles[:2] + [other_field])
    refused("quotient_degree_bits 4 above the oracles' rate_bits 3", qb_=4)
    refused("quotient_degree_bits 0 outside", qb_=0)
    refused("quotient_degree_bits 5 outside", qb_=5)
    refused("num_challenges 17", alphas_=[1] * 17)
    refused("num_challenges 0", alphas_=[])
    refused("more than GB_MAX_CONSTRAINT_ORACLES", orcs=[oracles[0]] * 17)
    refused("num_inputs is 5", params=t["params"] + [1])
    refused("param 1 is not below p", params=[1, F.P])
    refused("alpha 0 is not below p", alphas_=[F.P])
    # the degree rule at its boundary: 2^qb + 1 = 3 is accepted, 4 refused - as a bound of the constraints and as a declared degree
    cube = one([(0, 0, 0)], lambda cell, param, x, l_first, l_last: [cell[0] * cell[0] * x])
    assert constraint_quotient(ctx, oracles, cube, t["params"], alphas, qb).shape == (2, 4)
    refused("degree 4 is above 2\\^quotient_degree_bits \\+ 1 = 3", programs=one([(0, 0, 0)], lambda cell, param, x, l_first, l_last: [cell[0] * cell[0] * x * x]))
    refused("degree 4 is above", programs=one([(0, 0, 0)], degree=4))
    for b in oracles + [other_size, other_field]:
        b.free()
    tree.free()
