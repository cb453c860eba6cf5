"""gb_fri_verify_batch: gb_fri_verify of many proofs on one instance shape, the query rounds on the device through the general
layout (csrc/kernels.hpp FriVerifyLayout), for both fields.

Every case compares, per item, (status, check, text) with gb_fri_verify on that item alone and the accept-or-reject kind with the
yardstick on Python integers (tests/fri_instances.py verify_fri_instance), and asserts through gb_fri_verify_batch_counts that the
regular items were decided by the kernels - not by the host walk that answers for irregular items and for shapes past the limits.
-m gpu only."""
import copy
import os
import struct

import numpy as np
import pytest

import fri_batch_helpers as H
import fri_instances as FI
from oracle import verifier as V
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, PolynomialBatch, native as N, prove_openings, verify_fri_proofs
from plonky2_goldibear_amd.fri import fri_verify_batch_counts

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": GL, "babybear": BB}
BOTH = pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
OK = (N.GB_OK, N.GB_VCHECK_NONE, H.NONE, H.NONE)
DEVICE_CHECKS = {N.GB_VCHECK_NONE, N.GB_VCHECK_INITIAL_PATH, N.GB_VCHECK_CONSISTENCY, N.GB_VCHECK_LAYER_PATH, N.GB_VCHECK_FINAL_POLY}


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- items: commit, open, transcript (as tests/test_gpu_fri_openings.py)
def _commit(ctx, F, values, rate_bits, cap_height, salted, seed):
    n = values.shape[1]
    salts = F.fill(0xA17 + seed, 4 * (n << rate_bits)).reshape(4, -1) if salted else None
    return PolynomialBatch.from_values(ctx, values, rate_bits, cap_height, salts=salts, field=FI.field_tag(F))


def _openings(F, inst, oracles):
    out = []
    for batch in inst.batches:
        z, ev, vals = np.array(batch.point, dtype=F.dtype), {}, []
        for p in batch.polynomials:
            if p.oracle_index not in ev:
                ev[p.oracle_index] = oracles[p.oracle_index].eval_ext(z)
            vals.append(ev[p.oracle_index][p.polynomial_index])
        out.append(np.array(vals, dtype=F.dtype))
    return out


def _transcript(F, caps, openings, seed):
    ch = F.Challenger()
    ch.observe_element(seed)
    for cap in caps:
        ch.observe_cap(cap)
    for op in openings:
        ch.observe_elements(op.ravel())
    return ch


class Made:
    """one proof: the instance with this item's points, the arrays of the call (H.Item), the proof as a dict, the oracle's Challenger"""

    def __init__(self, F, inst, item, fri, ch):
        self.F, self.inst, self.item, self.fri, self.ch = F, inst, item, fri, ch

    def but(self, edit=None, **changes):
        """a copy with the proof dict edited (and re-serialised) and / or arrays of the item replaced"""
        m = Made(self.F, self.inst, self.item.copy(**changes), copy.deepcopy(self.fri), self.ch)
        if edit is not None:
            edit(m.fri)
            m.item.proof = FI.write_fri_proof(self.F, m.fri)
        return m


def _with_points(F, inst, seed):
    rng = np.random.default_rng(seed)
    inst = copy.deepcopy(inst)
    for b in inst.batches:
        b.point = tuple(int(x) for x in rng.integers(1, F.P, size=F.D, dtype=np.uint64))
    return inst


def _make(ctx, F, inst, params, seed, kind="random"):
    fld = FI.field_tag(F)
    db, r, cap_h = params.degree_bits, params.config.rate_bits, params.config.cap_height
    oracles = [_commit(ctx, F, FI.oracle_values(F, o.num_polys, db, 1000 * seed + 10 * i, kind), r, cap_h, bool(params.hiding and o.blinding), seed + i)
               for i, o in enumerate(inst.oracles)]
    caps = [np.array(b.merkle_tree.cap, copy=True) for b in oracles]
    openings = _openings(F, inst, oracles)
    ch = _transcript(F, caps, openings, seed)
    before = FI.challenger_tuple(ch, F)
    proof, _ = prove_openings(inst, oracles, before, params)
    for b in oracles:
        b.free()
    return Made(F, inst, H.Item(fld, inst, openings, before, caps, proof), FI.read_fri_proof(F, proof, inst, params), ch)


def _bump(F, x):
    return (int(x) + 1) % F.P


def _indices(m, params):
    return FI.fri_challenges(m.F, FI.clone_challenger(m.ch), m.fri, params)[0]["fri_query_indices"]


# ----------------------------------------------------------------------------- the comparison every case runs
def _yardstick(m, params):
    """-> None (accepted) or the kind of the check that failed"""
    F, it = m.F, m.item
    inst = copy.deepcopy(m.inst)
    openings, at = [], 0
    for b, batch in enumerate(inst.batches):
        batch.point = tuple(int(x) for x in it.points[b])
        k = len(batch.polynomials)
        openings.append([tuple(int(x) for x in e) for e in it.openings[at:at + k]])
        at += k
    try:
        FI.verify_fri_instance(F, inst, openings, [it.caps[o] for o in range(it.caps.shape[0])], FI.clone_challenger(m.ch), it.proof, params)
        return None
    except FI.FriReject as e:
        return e.kind


def _run(ctx, F, shape, params, made, host=(), yardstick=True):
    """the batch call on `made`; every item against gb_fri_verify alone and the yardstick; the hook's counts: the items at the
    indices `host` are the host's, every other one the device's.  -> [(status, check, query_round, index)]"""
    fld = FI.field_tag(F)
    dev0, host0 = fri_verify_batch_counts(ctx)
    st, res = H.raw_batch(ctx.handle, fld, shape, params, [m.item for m in made])
    dev1, host1 = fri_verify_batch_counts(ctx)
    assert st == (N.GB_OK if all(r[0] == N.GB_OK for r in res) else N.GB_ERR_VERIFY), H.last_error(ctx.handle)
    assert (dev1 - dev0, host1 - host0) == (len(made) - len(set(host)), len(set(host))), "device / host items"
    for i, (m, r) in enumerate(zip(made, res)):
        alone = H.single(ctx.handle, fld, shape, params, m.item)
        assert r[0] == alone[0], "item %d: %r, gb_fri_verify %r" % (i, r, alone)
        assert H.check_text(r[1]) == alone[1], "item %d: %r, gb_fri_verify %r" % (i, r, alone)
        assert (r[1] == N.GB_VCHECK_NONE) == (r[0] == N.GB_OK)
        if i not in host:
            assert r[1] in DEVICE_CHECKS, "item %d: %r" % (i, r)
        if yardstick and r[0] != N.GB_ERR_INVALID:
            kind = _yardstick(m, params)
            assert kind == (None if r[0] == N.GB_OK else FI.kind_of_message(H.check_text(r[1]))), "item %d: %r, the yardstick %r" % (i, r, kind)
    return res


# ----------------------------------------------------------------------------- a. the minimum
@BOTH
def test_the_minimum(ctx, field_name):
    """one oracle, one column, one batch, 2^2 rows; no layer, one of arity 2, one of arity 4 - through the Python door"""
    F = FIELDS[field_name]
    fld = FI.field_tag(F)
    shape = FI.instance_from_tuples((1,), (False,), [((1,) * F.D, [(0, 0)])])
    for bits, nqr in (([], 4), ([1], 5), ([2], 4)):
        params = FI.fri_params(2, 1, 0, bits, 2, nqr)
        made = [_make(ctx, F, _with_points(F, shape, 40 + s), params, seed=3 + s, kind="edges") for s in range(3)]
        assert _run(ctx, F, shape, params, made) == [OK] * 3
        dev0, host0 = fri_verify_batch_counts(ctx)
        door = verify_fri_proofs(ctx, [(m.inst, [m.item.openings], m.item.challenger, list(m.item.caps), m.item.proof) for m in made], params, field=fld)
        assert [(r.ok, r.status, r.check, r.text, r.query_round, r.index) for r in door] == [(True, 0, 0, "", None, None)] * 3
        assert fri_verify_batch_counts(ctx) == (dev0 + 3, host0)
    assert H.raw_batch(ctx.handle, fld, shape, params, [made[0].item], num_items=0, null_tables=("points", "results"))[0] == N.GB_OK


# ----------------------------------------------------------------------------- b. general instances
GENERAL = {"goldilocks": ([2, 1], 28), "babybear": ([1, 1, 1], 5)}
_general_cache = {}


def _general(ctx, field_name, skip=None, count=9):
    """`count` items of the general shape (three oracles of 1, 9 salted and 37 columns, five batches, hiding, cap_height 1, 2^5 rows,
    proof_of_work_bits 8): own points, oracle values and transcript seeds.  Made once per shape and never changed."""
    key = (field_name, skip)
    if key not in _general_cache:
        F = FIELDS[field_name]
        bits, nqr = GENERAL[field_name]
        params = FI.fri_params(5, 2, 1, bits, 8, nqr, hiding=True)
        shape = FI.general_instance(F, 5, seed=5 + (skip or 0), skip_oracle=skip)
        made = [_make(ctx, F, _with_points(F, shape, 70 + s), params, seed=20 + s) for s in range(count)]
        _general_cache[key] = (F, shape, params, made)
    return _general_cache[key]


@BOTH
def test_general_instances(ctx, field_name):
    F, shape, params, made = _general(ctx, field_name)
    assert _run(ctx, F, shape, params, made[:8]) == [OK] * 8


@BOTH
def test_an_oracle_no_batch_names_still_has_its_path_checked(ctx, field_name):
    F, shape, params, made = _general(ctx, field_name, skip=1, count=8)
    assert _run(ctx, F, shape, params, made) == [OK] * 8

    def leaf(fri):
        vals = fri["query_round_proofs"][2]["initial_trees_proof"][1][0]
        vals[4] = _bump(F, vals[4])
    res = _run(ctx, F, shape, params, made[:3] + [made[3].but(leaf)] + made[4:6])
    assert res == [OK] * 3 + [(N.GB_ERR_VERIFY, N.GB_VCHECK_INITIAL_PATH, 2, 1)] + [OK] * 2


# ----------------------------------------------------------------------------- c. constructed rejections
def _leaf(F, k, o, word=0):
    def edit(fri):
        vals = fri["query_round_proofs"][k]["initial_trees_proof"][o][0]
        vals[word] = _bump(F, vals[word])
    return edit


def _shorter_path(k, o):
    def edit(fri):
        vals, path = fri["query_round_proofs"][k]["initial_trees_proof"][o]
        fri["query_round_proofs"][k]["initial_trees_proof"][o] = (vals, path[:-1])
    return edit


def _first_failing_nonce(m, params):
    """the first nonce above the proof's own that the proof of work refuses (the yardstick's pow_ok on the transcript's response)"""
    F = m.F
    _, before_pow = FI.fri_challenges(F, FI.clone_challenger(m.ch), m.fri, params)
    cand = m.fri["pow_witness"] + 1
    while True:
        c2 = FI.clone_challenger(before_pow)
        c2.observe_element(cand)
        if not V.pow_ok(c2.get_challenge(), params.config.proof_of_work_bits, F):
            return cand
        cand += 1


@BOTH
def test_constructed_rejections(ctx, field_name):
    F, shape, params, made = _general(ctx, field_name)
    bits = params.reduction_arity_bits
    lg_n = params.degree_bits + params.config.rate_bits
    nqr = params.config.num_query_rounds
    k_last = nqr - 1
    V_, I_ = N.GB_ERR_VERIFY, N.GB_ERR_INVALID
    cases = []   # (Made, expected result, decided by the host)

    cases.append((made[0], OK, False))
    cases.append((made[1].but(_leaf(F, 3, 2, word=36)), (V_, N.GB_VCHECK_INITIAL_PATH, 3, 2), False))

    def sibling(fri):
        h = fri["query_round_proofs"][2]["initial_trees_proof"][1][1][0]
        h[1] = _bump(F, h[1])
    cases.append((made[2].but(sibling), (V_, N.GB_VCHECK_INITIAL_PATH, 2, 1), False))

    def two_rounds(fri):
        _leaf(F, 1, 0)(fri)
        _leaf(F, 4, 0)(fri)
    cases.append((made[3].but(two_rounds), (V_, N.GB_VCHECK_INITIAL_PATH, 1, 0), False))
    cases.append((made[4], OK, False))

    def layer_sibling(fri):
        h = fri["query_round_proofs"][2]["steps"][1][1][0]
        h[0] = _bump(F, h[0])
    cases.append((made[5].but(layer_sibling), (V_, N.GB_VCHECK_LAYER_PATH, 2, 1), False))

    # a coset word of layer 1 in the last round: beside the queried position, and at it
    m = made[6]
    xi = _indices(m, params)[k_last] >> bits[0]
    within = xi & ((1 << bits[1]) - 1)

    def coset_word(pos):
        def edit(fri):
            evals = fri["query_round_proofs"][k_last]["steps"][1][0]
            evals[pos] = (_bump(F, evals[pos][0]),) + tuple(evals[pos][1:])
        return edit
    cases.append((m.but(coset_word(within ^ 1)), (V_, N.GB_VCHECK_LAYER_PATH, k_last, 1), False))
    cases.append((m.but(coset_word(within)), (V_, N.GB_VCHECK_CONSISTENCY, k_last, 1), False))

    # an opening: the transcript has observed the honest one, so only the first consistency check moves
    op = made[7].item.openings.copy()
    op[3, 0] = _bump(F, op[3, 0])
    cases.append((made[7].but(openings=op), (V_, N.GB_VCHECK_CONSISTENCY, 0, 0), False))

    # a cap word: the first round whose index falls under that cap entry (an entry round 0 does not use, where there is one)
    m = made[8]
    entries = [x >> (lg_n - params.config.cap_height) for x in _indices(m, params)]
    entry = next((e for e in entries if e != entries[0]), entries[0])
    caps = m.item.caps.copy()
    caps[2, entry, 1] = _bump(F, caps[2, entry, 1])
    cases.append((m.but(caps=caps), (V_, N.GB_VCHECK_INITIAL_PATH, entries.index(entry), 2), False))

    # the proof of work
    def nonce(fri):
        fri["pow_witness"] = _first_failing_nonce(made[0], params)
    cases.append((made[0].but(nonce), (V_, N.GB_VCHECK_POW, H.NONE, H.NONE), True))

    # irregular items: the host's verdicts
    good = made[4]
    word = F.elem_bytes
    p_word = struct.pack("<Q" if word == 8 else "<I", F.P)
    cases.append((good.but(proof=good.item.proof[:-9]), (I_, N.GB_VCHECK_TRUNCATED, H.NONE, H.NONE), True))
    cases.append((good.but(proof=good.item.proof + b"\0"), (I_, N.GB_VCHECK_TRAILING, H.NONE, H.NONE), True))
    cases.append((good.but(proof=good.item.proof[:2 * word] + p_word + good.item.proof[3 * word:]), (I_, N.GB_VCHECK_NON_CANONICAL, H.NONE, H.NONE), True))
    cases.append((good.but(_shorter_path(1, 2)), (I_, N.GB_VCHECK_INITIAL_PATH_LEN, 1, 2), True))
    cases.append((made[2], OK, False))

    res = _run(ctx, F, shape, params, [c[0] for c in cases], host=[i for i, c in enumerate(cases) if c[2]])
    assert res == [c[1] for c in cases]
    seen = {r[1] for r in res}

    # without layers the combined evaluation is compared with the final polynomial directly
    flat = FI.fri_params(5, 2, 1, [], 8, 3, hiding=True)
    m0, m1, m2 = (_make(ctx, F, _with_points(F, shape, 90 + s), flat, seed=60 + s) for s in range(3))
    op = m1.item.openings.copy()
    op[0, F.D - 1] = _bump(F, op[0, F.D - 1])
    res = _run(ctx, F, shape, flat, [m0, m1.but(openings=op), m2])
    assert res == [OK, (V_, N.GB_VCHECK_FINAL_POLY, 0, H.NONE), OK]
    seen |= {r[1] for r in res}

    assert seen == {N.GB_VCHECK_NONE, N.GB_VCHECK_INITIAL_PATH, N.GB_VCHECK_LAYER_PATH, N.GB_VCHECK_CONSISTENCY, N.GB_VCHECK_FINAL_POLY,
                    N.GB_VCHECK_POW, N.GB_VCHECK_TRUNCATED, N.GB_VCHECK_TRAILING, N.GB_VCHECK_NON_CANONICAL, N.GB_VCHECK_INITIAL_PATH_LEN}


# ----------------------------------------------------------------------------- d. many batches
@BOTH
def test_many_batches(ctx, field_name):
    """40 columns opened in shuffled order at 8 points"""
    F = FIELDS[field_name]
    shape = FI.many_runs_instance(F, seed=5)
    params = FI.fri_params(5, 2, 2, [2], 4, 5)
    made = [_make(ctx, F, _with_points(F, shape, 30 + s), params, seed=80 + s) for s in range(4)]
    op = made[2].item.openings.copy()
    op[40 * 7 + 39, 0] = _bump(F, op[40 * 7 + 39, 0])   # the last entry of the last batch
    made[2] = made[2].but(openings=op)
    assert _run(ctx, F, shape, params, made) == [OK, OK, (N.GB_ERR_VERIFY, N.GB_VCHECK_CONSISTENCY, 0, 0), OK]


# ----------------------------------------------------------------------------- e. chunks
@BOTH
def test_chunks(ctx, field_name):
    F, shape, params, made = _general(ctx, field_name)
    items = list(made)
    items[0] = items[0].but(_leaf(F, 1, 1))
    op = items[4].item.openings.copy()
    op[0, 0] = _bump(F, op[0, 0])
    items[4] = items[4].but(openings=op)
    items[8] = items[8].but(_leaf(F, 0, 2, word=7))
    whole = _run(ctx, F, shape, params, items, yardstick=False)
    assert [r[1] for r in whole] == [N.GB_VCHECK_INITIAL_PATH] + [0] * 3 + [N.GB_VCHECK_CONSISTENCY] + [0] * 3 + [N.GB_VCHECK_INITIAL_PATH]
    ctx.set_option("verify_chunk_bytes", 4096)
    try:
        assert _run(ctx, F, shape, params, items, yardstick=False) == whole
    finally:
        ctx.set_option("verify_chunk_bytes", 8 << 20)


# ----------------------------------------------------------------------------- f. the reference's proof
def test_the_reference_proof(ctx, golden_dir):
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    pr, pis = V.read_proof_with_pis(rd("recursive_verifier_gl_proof.bin"), cd)
    cfg, fc, fp = cd["config"], cd["config"]["fri_config"], cd["fri_params"]
    c = cfg["num_challenges"]
    ch = GL.Challenger()                     # plonk/get_challenges.rs:26-60, up to and including observe_openings
    ch.observe_hash(vd["circuit_digest"])
    ch.observe_hash(GL.hash_no_pad(np.asarray(pis, dtype=np.uint64)))
    ch.observe_cap(pr["wires_cap"]); ch.get_n_challenges(2 * c)
    ch.observe_cap(pr["zs_cap"]); ch.get_n_challenges(c)
    ch.observe_cap(pr["quotient_cap"])
    zeta = ch.get_extension_challenge(2)
    openings = V.fri_openings(pr["openings"])
    for batch in openings:
        ch.observe_elements([x for e in batch for x in e])
    params = FI.fri_params(fp["degree_bits"], fc["rate_bits"], fc["cap_height"], fp["reduction_arity_bits"], fc["proof_of_work_bits"],
                           fc["num_query_rounds"], hiding=fp["hiding"])
    caps = [vd["constants_sigmas_cap"], pr["wires_cap"], pr["zs_cap"], pr["quotient_cap"]]
    inst = FI.plonk_instance(cd, zeta)
    fri = pr["opening_proof"]
    good = Made(GL, inst, H.Item(N.GB_GOLDILOCKS, inst, openings, FI.challenger_tuple(ch, GL), caps, FI.write_fri_proof(GL, fri)), fri, ch)

    # tests/test_fri_instances.py _mutations, those that change proof bytes
    def leaf(f):
        f["query_round_proofs"][2]["initial_trees_proof"][1][0][3] = _bump(GL, f["query_round_proofs"][2]["initial_trees_proof"][1][0][3])

    def sibling(f):
        f["query_round_proofs"][1]["initial_trees_proof"][2][1][0][1] = _bump(GL, f["query_round_proofs"][1]["initial_trees_proof"][2][1][0][1])

    def layer_eval(f):
        evals = f["query_round_proofs"][0]["steps"][1][0]
        evals[5] = (evals[5][0], _bump(GL, evals[5][1]))

    def final(f):
        f["final_poly"][3] = (_bump(GL, f["final_poly"][3][0]), f["final_poly"][3][1])

    def nonce(f):
        f["pow_witness"] = _bump(GL, f["pow_witness"])

    made = [good] + [good.but(e) for e in (leaf, sibling, layer_eval, final, nonce)]
    res = _run(ctx, GL, inst, params, made, host=[4, 5])   # (the final polynomial and the nonce move the proof-of-work response)
    assert res[0] == OK and all(r[0] == N.GB_ERR_VERIFY for r in res[1:])
    assert res[1] == (N.GB_ERR_VERIFY, N.GB_VCHECK_INITIAL_PATH, 2, 1) and res[2] == (N.GB_ERR_VERIFY, N.GB_VCHECK_INITIAL_PATH, 1, 2)
    assert res[3][1] in (N.GB_VCHECK_CONSISTENCY, N.GB_VCHECK_LAYER_PATH) and res[3][2:] == (0, 1)
    assert res[4][1] == res[5][1] == N.GB_VCHECK_POW


# ----------------------------------------------------------------------------- g. past the device limits
@BOTH
@pytest.mark.parametrize("over", ["oracles", "batches"])
def test_past_the_device_limits(ctx, field_name, over):
    """65 one-column oracles, or 65 batches, at 2^2 rows: every item is walked on the host, with the same answers"""
    F = FIELDS[field_name]
    rng = np.random.default_rng(11)
    pt = lambda: tuple(int(x) for x in rng.integers(1, F.P, size=F.D, dtype=np.uint64))
    if over == "oracles":
        shape = FI.instance_from_tuples((1,) * 65, (False,) * 65, [(pt(), [(o, 0) for o in range(65)])])
    else:
        shape = FI.instance_from_tuples((1,), (False,), [(pt(), [(0, 0)]) for _ in range(65)])
    params = FI.fri_params(2, 1, 0, [1], 2, 3)
    made = [_make(ctx, F, _with_points(F, shape, 50 + s), params, seed=7 + s) for s in range(2)]
    op = made[1].item.openings.copy()
    op[64, 0] = _bump(F, op[64, 0])
    made[1] = made[1].but(openings=op)
    res = _run(ctx, F, shape, params, made, host=[0, 1])
    assert res == [OK, (N.GB_ERR_VERIFY, N.GB_VCHECK_CONSISTENCY, 0, 0)]


# ----------------------------------------------------------------------------- h. repeatability and the transcript
@BOTH
def test_the_same_call_twice_and_the_callers_transcripts(ctx, field_name):
    F, shape, params, made = _general(ctx, field_name)
    items = [made[0].item, made[1].but(_leaf(F, 2, 2)).item, made[2].item]
    fld = FI.field_tag(F)
    first = H.raw_batch(ctx.handle, fld, shape, params, items, with_challengers=True)
    second = H.raw_batch(ctx.handle, fld, shape, params, items, with_challengers=True)
    assert first[0] == N.GB_ERR_VERIFY and first[1] == [OK, (N.GB_ERR_VERIFY, N.GB_VCHECK_INITIAL_PATH, 2, 2), OK]
    assert first[:2] == second[:2]
    assert first[2] == first[3] == second[2] == second[3], "the call advanced a caller's challenger"
