"""gb_fri_prove_openings / gb_fri_verify: PolynomialBatch::prove_openings (fri/oracle.rs:187-246) and verify_fri_proof
(fri/verifier.rs:67-250) on any FriInstanceInfo, on the GPU and for both fields.

  * the PLONK instance written out by hand gives gb_prove_openings' bytes and transcript;
  * general instances (tests/fri_instances.py) are accepted by the Python restatement of the reference's verifier and by
    gb_fri_verify, carry the final polynomial computed on Python integers and the smallest nonce, and are reproducible;
  * a changed word is rejected by both verifiers for the same kind of reason;
  * every argument error of the header is reported, with the caller's transcript left alone.
-m gpu only."""
import copy
import ctypes as C

import numpy as np
import pytest

import fri_instances as FI
from oracle import plonk_dummy as D
from oracle import verifier as V
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GoldibearError, GpuContext, MerkleTree, PolynomialBatch, ShapeError, VerifyError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import prove_openings, verify_fri_proof
from plonky2_goldibear_amd.fri import FriBatchInfo, FriInstanceInfo, FriOracleInfo, FriPolynomialInfo, _challenger_state, _challenger_tuple
from wired_circuits import wired_dummy_circuit

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": GL, "babybear": BB}


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- 1. the PLONK instance through the general door
def _config(F, **kw):
    kw = dict(dict(proof_of_work_bits=4, num_query_rounds=8), **kw)
    return D.CircuitConfig(**kw) if F is GL else D.CircuitConfig.babybear(**kw)


def _plonk_oracles(ctx, F, kind, degree_bits, zk, bits, seed):
    """-> (CircuitData, [constants_sigmas, wires, zs, quotient], zeta, the oracle's Challenger after observe_openings).
    kind "dummy" / "wired": the circuit's own witness through gb_zs_partial_products and gb_quotient_polys.  kind "shape":
    DummyCircuit starts at 2^3 rows, and gb_prove_openings asks its batches for their shape only - random oracles of the
    circuit's shape at 2^2."""
    tag, cfg = FI.field_tag(F), _config(F)
    n, r, cap_h, c = 1 << degree_bits, cfg.rate_bits, cfg.cap_height, cfg.num_challenges
    kw = dict(num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=c,
              arity_bits=cfg.arity_bits, proof_of_work_bits=cfg.proof_of_work_bits, num_query_rounds=cfg.num_query_rounds, field=tag,
              zero_knowledge=zk, reduction_arity_bits=bits)
    salts = F.fill(0x5A17 + seed, 3 * 4 * (n << r)).reshape(3, 4, n << r) if zk else [None] * 3
    ch = F.Challenger()
    nchunks = -(-cfg.num_routed_wires // cfg.max_quotient_degree_factor)
    if kind == "shape":
        ncs = 1 + cfg.num_constants + cfg.num_routed_wires
        gpu = CircuitData(ctx, degree_bits, F.fill(seed, ncs * n).reshape(ncs, n), F.fill(seed + 1, cfg.num_routed_wires), **kw)
        wires = PolynomialBatch.from_values(ctx, F.fill(seed + 2, cfg.num_wires * n).reshape(-1, n), r, cap_h, salts=salts[0], field=tag)
        zs = PolynomialBatch.from_values(ctx, F.fill(seed + 3, c * nchunks * n).reshape(-1, n), r, cap_h, salts=salts[1], field=tag)
        quot = PolynomialBatch.from_coeffs(ctx, F.fill(seed + 4, c * cfg.max_quotient_degree_factor * n).reshape(-1, n), r, cap_h,
                                           salts=salts[2], field=tag)
        for b in (wires, zs, quot):
            ch.observe_cap(b.merkle_tree.cap)
    else:
        if kind == "wired":
            circ, w, wkw = wired_dummy_circuit(F, cfg, degree_bits, seed, dense="edges")
            kw.update(gate_constant=wkw["gate_constant"], gate_pi=wkw["gate_pi"])
        else:
            circ = D.DummyCircuit(degree_bits, cfg, F=F)
            w = circ.witness(seed=seed)
            kw.update(gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI)
        gpu = CircuitData(ctx, degree_bits, circ.constants_sigmas, circ.k_is, **kw)
        pi_hash = F.hash_no_pad(np.zeros(0, dtype=F.dtype))
        ch.observe_hash(gpu.circuit_digest)
        ch.observe_hash(pi_hash)
        wires = PolynomialBatch.from_values(ctx, w, r, cap_h, salts=salts[0], field=tag)
        ch.observe_cap(wires.merkle_tree.cap)
        betas, gammas = ch.get_n_challenges(c), ch.get_n_challenges(c)
        zs = PolynomialBatch.from_values(ctx, gpu.zs_partial_products(w, betas, gammas), r, cap_h, salts=salts[1], field=tag)
        ch.observe_cap(zs.merkle_tree.cap)
        alphas = ch.get_n_challenges(c)
        quot = PolynomialBatch.from_coeffs(ctx, gpu.quotient_polys(wires, zs, pi_hash, betas, gammas, alphas), r, cap_h, salts=salts[2],
                                           field=tag)
        ch.observe_cap(quot.merkle_tree.cap)
    zeta = ch.get_extension_challenge(F.D)
    cs = gpu.constants_sigmas_commitment
    zeta_next = F.escale(zeta, F.two_adic_generator(degree_bits))
    ev = lambda b, z: b.eval_ext(np.array(z, dtype=F.dtype))
    for part in (ev(cs, zeta), ev(wires, zeta), ev(zs, zeta), ev(quot, zeta), ev(zs, zeta_next)[:c]):
        ch.observe_elements(part)
    return gpu, [cs, wires, zs, quot], zeta, ch


def _plonk_instance_by_hand(F, oracles, zeta, degree_bits, c, zk):
    """get_fri_instance(zeta) (plonk/circuit_data.rs:438-520)"""
    infos = [FriOracleInfo(b.num_polys, bool(zk and i > 0)) for i, b in enumerate(oracles)]
    every = [p for i, b in enumerate(oracles) for p in FriPolynomialInfo.from_range(i, range(b.num_polys))]
    zeta_next = F.escale(zeta, F.two_adic_generator(degree_bits))
    return FriInstanceInfo(infos, [FriBatchInfo(zeta, every), FriBatchInfo(zeta_next, FriPolynomialInfo.from_range(2, range(c)))])


PLONK_CASES = [
    # 2^2: below one 16-byte vector per lane of a workgroup; 2^11: across the division's 1024-coefficient blocks; 2^13: several
    # workgroups per column.  "stock" = ConstantArityBits' list; [1, 1, 1] sums past degree_bits 2, where [1] stands in.
    ("goldilocks", "shape", 2, False, []), ("goldilocks", "shape", 2, True, [1]),
    ("goldilocks", "dummy", 5, False, "stock"), ("goldilocks", "wired", 5, True, [1, 1, 1]),
    ("goldilocks", "dummy", 11, False, [1, 1, 1]), ("goldilocks", "wired", 11, False, "stock"),
    ("goldilocks", "dummy", 13, True, []), ("goldilocks", "wired", 13, False, []), ("goldilocks", "dummy", 13, False, "stock"),
    ("goldilocks", "wired", 13, False, [1, 1, 1]),
    ("babybear", "shape", 2, False, []), ("babybear", "shape", 2, False, [1]),
    ("babybear", "dummy", 5, False, [1, 1, 1]), ("babybear", "wired", 5, True, "stock"),
    ("babybear", "dummy", 11, False, "stock"), ("babybear", "wired", 11, False, []),
    ("babybear", "dummy", 13, False, []), ("babybear", "wired", 13, True, [1, 1, 1]), ("babybear", "wired", 13, False, "stock"),
]


@pytest.mark.parametrize("field_name,kind,degree_bits,zk,bits", PLONK_CASES)
def test_plonk_instance_through_the_general_door(ctx, field_name, kind, degree_bits, zk, bits):
    F = FIELDS[field_name]
    gpu, oracles, zeta, ch = _plonk_oracles(ctx, F, kind, degree_bits, zk, None if bits == "stock" else bits, seed=100 + degree_bits)
    cfg = _config(F)
    arity = gpu.reduction_arity_bits
    assert arity == (D.reduction_arity_bits(cfg, degree_bits) if bits == "stock" else bits)
    inst = _plonk_instance_by_hand(F, oracles, zeta, degree_bits, cfg.num_challenges, zk)
    params = FI.fri_params(degree_bits, cfg.rate_bits, cfg.cap_height, arity, cfg.proof_of_work_bits, cfg.num_query_rounds, hiding=zk)
    before = FI.challenger_tuple(ch, F)
    want, want_after = gpu.prove_openings(oracles[1], oracles[2], oracles[3], zeta, before)
    got, got_after = prove_openings(inst, oracles, before, params)
    assert got == want
    assert got_after == want_after
    assert PolynomialBatch.prove_openings(inst, oracles, before, params) == (want, want_after)
    for b in oracles[1:]:
        b.free()
    gpu.free()


# ----------------------------------------------------------------------------- 2 - 4. general instances
def _commit(ctx, F, values, rate_bits, cap_height, salted, seed):
    n = values.shape[1]
    salts = F.fill(0xA17 + seed, 4 * (n << rate_bits)).reshape(4, -1) if salted else None
    return PolynomialBatch.from_values(ctx, values, rate_bits, cap_height, salts=salts, field=FI.field_tag(F))


def _openings(F, inst, oracles):
    """FriOpenings through gb_batch_eval_ext: per batch [size][D]"""
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


def _as_tuples(openings):
    return [[tuple(int(x) for x in e) for e in op] for op in openings]


def _open_and_check(F, inst, oracles, params, seed):
    tag = FI.field_tag(F)
    caps = [b.merkle_tree.cap for b in oracles]
    openings = _openings(F, inst, oracles)
    ch = _transcript(F, caps, openings, seed)
    before = FI.challenger_tuple(ch, F)
    proof, after = prove_openings(inst, oracles, before, params)
    assert (proof, after) == prove_openings(inst, oracles, before, params), "two calls, two answers"
    fri = FI.read_fri_proof(F, proof, inst, params)
    assert FI.write_fri_proof(F, fri) == proof
    # the reference's verifier, restated, accepts - and leaves the transcript where the prover left it
    vch = FI.clone_challenger(ch)
    assert FI.verify_fri_instance(F, inst, _as_tuples(openings), caps, vch, fri, params)
    assert FI.challenger_tuple(vch, F) == after
    assert verify_fri_proof(inst, openings, before, caps, proof, params, field=tag)
    # the final polynomial on Python integers, with the proof's own challenges
    chal, before_pow = FI.fri_challenges(F, FI.clone_challenger(ch), fri, params)
    coeffs = [b.polynomials for b in oracles]
    assert fri["final_poly"] == FI.final_poly_ref(F, inst, coeffs, chal["fri_alpha"], chal["fri_betas"], params.reduction_arity_bits)
    # the smallest nonce (fri/prover.rs:136-188 as this library reads it: the minimum)
    assert V.pow_ok(chal["fri_pow_response"], params.config.proof_of_work_bits, F)
    for cand in range(fri["pow_witness"]):
        c2 = FI.clone_challenger(before_pow)
        c2.observe_element(cand)
        assert not V.pow_ok(c2.get_challenge(), params.config.proof_of_work_bits, F), "nonce %d passes too" % cand
    return dict(caps=caps, openings=openings, challenger=ch, before=before, proof=proof, fri=fri)


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_the_minimum(ctx, field_name):
    """one oracle, one column, one batch, 2^2 rows"""
    F = FIELDS[field_name]
    b = _commit(ctx, F, FI.oracle_values(F, 1, 2, 5, "edges"), 1, 0, False, 0)
    inst = FI.instance_from_tuples((1,), (False,), [(tuple(int(x) for x in F.fill(9, F.D) + 1), [(0, 0)])])
    for bits, nqr in (([], 4), ([1], 5), ([2], 4)):
        _open_and_check(F, inst, [b], FI.fri_params(2, 1, 0, bits, 2, nqr), seed=3)
    b.free()


def _general_oracles(ctx, F, degree_bits, seed, kind, rate_bits=2, cap_height=1):
    return [_commit(ctx, F, FI.oracle_values(F, npolys, degree_bits, seed + 10 * i, kind), rate_bits, cap_height, blind, seed + i)
            for i, (npolys, blind) in enumerate(zip(FI.GENERAL_NUM_POLYS, FI.GENERAL_BLINDING))]


@pytest.mark.parametrize("field_name,degree_bits,values,skip,bits,nqr", [
    ("goldilocks", 5, "random", None, [2, 1], 28), ("goldilocks", 5, "edges", 0, [], 9),
    ("goldilocks", 11, "edges", None, [4, 4], 6), ("goldilocks", 11, "random", 1, [3, 2, 1], 4),
    ("babybear", 5, "edges", None, [1, 1, 1], 28), ("babybear", 5, "random", 1, [5], 7),
    ("babybear", 11, "random", None, [3, 3, 3], 6), ("babybear", 11, "edges", 0, [4], 4),
])
def test_general_instances(ctx, field_name, degree_bits, values, skip, bits, nqr):
    """three oracles (1, 9 salted, 37 columns), five batches = two passes of four slots; whole ranges, every third column,
    descending, shuffled, a polynomial twice in a batch, one polynomial in every batch, and (skip) an oracle in no batch"""
    F = FIELDS[field_name]
    oracles = _general_oracles(ctx, F, degree_bits, 7 * degree_bits, values)
    inst = FI.general_instance(F, degree_bits, seed=degree_bits + (skip or 0), skip_oracle=skip)
    _open_and_check(F, inst, oracles, FI.fri_params(degree_bits, 2, 1, bits, 3, nqr, hiding=True), seed=11)
    for b in oracles:
        b.free()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_more_runs_than_fit_anywhere_small(ctx, field_name):
    """a 40-column oracle in shuffled order at 8 points: some 320 runs of one column, two passes"""
    F = FIELDS[field_name]
    b = _commit(ctx, F, FI.oracle_values(F, 40, 5, 77, "random"), 2, 2, False, 0)
    inst = FI.many_runs_instance(F, seed=5)
    _open_and_check(F, inst, [b], FI.fri_params(5, 2, 2, [2], 4, 5), seed=13)
    b.free()


# ----------------------------------------------------------------------------- 5. rejected for the right reason
def _mutate(F, rng, fri, openings, caps):
    """one word of the proof, the openings or the caps, plus one (still a canonical element) -> what was changed"""
    fri, openings, caps = copy.deepcopy(fri), [op.copy() for op in openings], [c.copy() for c in caps]
    bump = lambda x: (int(x) + 1) % F.P
    q = fri["query_round_proofs"][int(rng.integers(len(fri["query_round_proofs"])))]
    where = ["opening", "cap", "layer cap", "leaf", "sibling", "evaluation", "layer sibling", "final", "nonce"][int(rng.integers(9))]
    if where == "opening":
        op = openings[int(rng.integers(len(openings)))]
        i, k = int(rng.integers(op.shape[0])), int(rng.integers(F.D))
        op[i, k] = bump(op[i, k])
    elif where == "cap":
        cap = caps[int(rng.integers(len(caps)))]
        i, k = int(rng.integers(cap.shape[0])), int(rng.integers(F.hout))
        cap[i, k] = bump(cap[i, k])
    elif where == "layer cap":
        cap = fri["commit_phase_merkle_caps"][int(rng.integers(len(fri["commit_phase_merkle_caps"])))]
        h = cap[int(rng.integers(len(cap)))]
        k = int(rng.integers(F.hout))
        h[k] = bump(h[k])
    elif where == "leaf":
        vals = q["initial_trees_proof"][int(rng.integers(len(q["initial_trees_proof"])))][0]
        i = int(rng.integers(len(vals)))
        vals[i] = bump(vals[i])
    elif where == "sibling":
        path = q["initial_trees_proof"][int(rng.integers(len(q["initial_trees_proof"])))][1]
        h = path[int(rng.integers(len(path)))]
        k = int(rng.integers(F.hout))
        h[k] = bump(h[k])
    elif where == "evaluation":
        evals = q["steps"][int(rng.integers(len(q["steps"])))][0]
        i, k = int(rng.integers(len(evals))), int(rng.integers(F.D))
        evals[i] = tuple(bump(x) if j == k else x for j, x in enumerate(evals[i]))
    elif where == "layer sibling":
        path = q["steps"][int(rng.integers(len(q["steps"])))][1]
        h = path[int(rng.integers(len(path)))]
        k = int(rng.integers(F.hout))
        h[k] = bump(h[k])
    elif where == "final":
        i, k = int(rng.integers(len(fri["final_poly"]))), int(rng.integers(F.D))
        fri["final_poly"][i] = tuple(bump(x) if j == k else x for j, x in enumerate(fri["final_poly"][i]))
    else:
        fri["pow_witness"] = bump(fri["pow_witness"])
    return where, fri, openings, caps


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_a_rejected_proof_is_rejected_for_the_right_reason(ctx, field_name):
    F = FIELDS[field_name]
    tag = FI.field_tag(F)
    oracles = _general_oracles(ctx, F, 5, 21, "random")
    inst = FI.general_instance(F, 5, seed=8)
    params = FI.fri_params(5, 2, 1, [2, 1], 3, 5, hiding=True)
    good = _open_and_check(F, inst, oracles, params, seed=17)
    rng = np.random.default_rng(64)
    seen = set()
    for _ in range(64):
        where, fri, openings, caps = _mutate(F, rng, good["fri"], good["openings"], good["caps"])
        try:
            FI.verify_fri_instance(F, inst, _as_tuples(openings), caps, FI.clone_challenger(good["challenger"]), fri, params)
            want = None
        except FI.FriReject as e:
            want = e.kind
        try:
            verify_fri_proof(inst, openings, good["before"], caps, FI.write_fri_proof(F, fri), params, field=tag, ctx=ctx)
            got = None
        except VerifyError as e:
            got = FI.kind_of_message(str(e))
        assert got == want, "a changed %s: the library says %r, the yardstick %r" % (where, got, want)
        seen.add(want)
    # what one changed word can reach: a leaf, sibling or cap breaks a Merkle path; an opening or the queried evaluation breaks the
    # consistency check; the final polynomial and the nonce are observed by the transcript, so they move the proof-of-work response
    # (and the query indices behind it).  The final evaluation alone fails only with two coordinated changes.
    assert {"merkle", "consistency", "pow"} <= seen
    # (test_final_evaluation_is_checked reaches it another way)
    for b in oracles:
        b.free()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_final_evaluation_is_checked(ctx, field_name):
    """The last check of verify_fri_proof (fri/verifier.rs:240-247), which no single changed word reaches: with no reduction layer
    the proof is the opened rows, final_poly and the nonce, and final_poly is compared with fri_combine_initial directly.  One
    changed OPENING then leaves the transcript, the proof of work and every Merkle path alone (the caller's challenger has observed
    the honest openings; it is passed by value) and both verifiers must stop at the final evaluation."""
    F = FIELDS[field_name]
    tag = FI.field_tag(F)
    oracles = _general_oracles(ctx, F, 5, 31, "random")
    inst = FI.general_instance(F, 5, seed=9)
    params = FI.fri_params(5, 2, 1, [], 3, 4, hiding=True)
    good = _open_and_check(F, inst, oracles, params, seed=19)
    openings = [op.copy() for op in good["openings"]]
    openings[3][7, 0] = (int(openings[3][7, 0]) + 1) % F.P
    with pytest.raises(FI.FriReject) as e:
        FI.verify_fri_instance(F, inst, _as_tuples(openings), good["caps"], FI.clone_challenger(good["challenger"]), good["fri"], params)
    assert e.value.kind == "final"
    with pytest.raises(VerifyError, match="Final polynomial"):
        verify_fri_proof(inst, openings, good["before"], good["caps"], good["proof"], params, field=tag, ctx=ctx)
    for b in oracles:
        b.free()


# ----------------------------------------------------------------------------- 6. errors
def _raw_call(ctx, F, handles, points, sizes, polys, bits, challenger, pow_bits=2, nqr=4, cap=1 << 20):
    """gb_fri_prove_openings itself -> (status, message, challenger afterwards, size reported, bytes)"""
    tag = FI.field_tag(F)
    cs, w = _challenger_state(challenger, tag)
    arr = (C.c_void_p * max(len(handles), 1))(*handles)
    pts = np.ascontiguousarray(points, dtype=F.dtype)
    sz, pl, ar = (np.ascontiguousarray(a, dtype=np.uint32) for a in (sizes, polys, bits))
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_size_t()
    st = ctx._lib.gb_fri_prove_openings(ctx.handle, arr, len(handles), pts.ctypes.data, u32p(sz), len(sz), u32p(pl), u32p(ar), len(ar),
                                        pow_bits, nqr, C.byref(cs), buf.ctypes.data if cap else None, cap, C.byref(n))
    msg = ctx._lib.gb_last_error(ctx.handle)
    return st, (msg.decode() if msg else ""), _challenger_tuple(cs, w), n.value, buf[: n.value].tobytes() if st == N.GB_OK else None


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_errors(ctx, field_name):
    F = FIELDS[field_name]
    tag, OF = FI.field_tag(F), BB if F is GL else GL
    lg, r, cap_h = 5, 2, 1
    a = _commit(ctx, F, FI.oracle_values(F, 3, lg, 1, "random"), r, cap_h, False, 0)
    b = _commit(ctx, F, FI.oracle_values(F, 2, lg, 2, "random"), r, cap_h, True, 1)          # salted: rows of 2 + 4 words
    point = [int(x) for x in F.fill(3, F.D) + 1]
    ch = F.Challenger()
    ch.observe_elements(F.fill(4, 11))
    chal = FI.challenger_tuple(ch, F)
    good = dict(handles=[a.handle, b.handle], points=[point, point[::-1]], sizes=[3, 2], polys=[(0, 0), (0, 1), (1, 1), (1, 0), (0, 2)], bits=[2])

    def raw(**kw):
        return _raw_call(ctx, F, challenger=chal, **dict(good, **kw))

    def refused(status, needle, **kw):
        st, msg, after, _, _ = raw(**kw)
        assert st == status and needle in msg and msg, (st, msg)
        assert after == chal, "the challenger moved on an error"

    st, _, after_good, size, plain = raw()
    assert st == N.GB_OK and len(plain) == size and after_good != chal
    refused(N.GB_ERR_INVALID, "at least one oracle", handles=[])
    refused(N.GB_ERR_INVALID, "at least one batch", sizes=[])
    refused(N.GB_ERR_INVALID, "opens no polynomial", sizes=[5, 0])
    refused(N.GB_ERR_INVALID, "is null", handles=[a.handle, None])
    ctx2 = GpuContext(0)
    foreign = _commit(ctx2, F, FI.oracle_values(F, 2, lg, 2, "random"), r, cap_h, False, 0)
    refused(N.GB_ERR_INVALID, "another context", handles=[a.handle, foreign.handle])
    foreign.free()
    ctx2.close()
    other = _commit(ctx, OF, FI.oracle_values(OF, 2, lg, 2, "random"), r, cap_h, False, 0)
    refused(N.GB_ERR_INVALID, "field", handles=[a.handle, other.handle])
    other.free()
    tree = MerkleTree.new(ctx, F.fill(5, 3 << (lg + r)).reshape(-1, 3), cap_h, field=tag)
    refused(N.GB_ERR_INVALID, "stand-alone Merkle tree", handles=[a.handle, tree._b.handle])
    tree.free()
    for what, shape in (("degree_bits", (lg + 1, r, cap_h)), ("rate_bits", (lg, r + 1, cap_h)), ("cap_height", (lg, r, cap_h + 1))):
        odd = _commit(ctx, F, FI.oracle_values(F, 2, shape[0], 2, "random"), shape[1], shape[2], False, 0)
        refused(N.GB_ERR_INVALID, "differs from oracle 0", handles=[a.handle, odd.handle])
        odd.free()
    refused(N.GB_ERR_INVALID, "oracle_index 2", polys=[(0, 0), (0, 1), (2, 1), (1, 0), (0, 2)])
    refused(N.GB_ERR_INVALID, "polynomial_index 3", polys=[(0, 0), (0, 3), (1, 1), (1, 0), (0, 2)])
    refused(N.GB_ERR_INVALID, "salt columns are not polynomials", polys=[(0, 0), (0, 1), (1, 2), (1, 0), (0, 2)])
    for bits in ([9], [0], [3, 3]):   # outside [1, 8], and past degree_bits: what gb_circuit_set_fri_reduction_arity_bits refuses
        refused(N.GB_ERR_INVALID, "FRI reduction", bits=bits)
    refused(N.GB_ERR_INVALID, "num_query_rounds is zero", nqr=0)
    refused(N.GB_ERR_INVALID, "GB_MAX_FRI_QUERY_ROUNDS", nqr=4097)
    refused(N.GB_ERR_INVALID, "non-canonical coordinate", points=[point, [F.P] + point[1:]])
    refused(N.GB_ERR_UNSUPPORTED, "1 / z", points=[point, [0] * F.D])
    assert raw(bits=[])[0] == N.GB_OK                                      # the empty list is a list
    # the Python mirror sees what it can before the call
    inst = FI.instance_from_tuples((3, 2), (False, True), [(point, [(0, 0), (0, 1), (1, 1)]), (point[::-1], [(1, 0), (0, 2)])])
    params = FI.fri_params(lg, r, cap_h, [2], 2, 4, hiding=True)
    assert prove_openings(inst, [a, b], chal, params) == (plain, after_good)
    for bad_inst in (FI.instance_from_tuples((4, 2), (False, True), [(point, [(0, 0)])]),
                     FI.instance_from_tuples((3, 2), (False, False), [(point, [(0, 0)])]),
                     FI.instance_from_tuples((3, 2, 1), (False, True, False), [(point, [(0, 0)])])):
        with pytest.raises(ShapeError):
            prove_openings(bad_inst, [a, b], chal, params)
    with pytest.raises(ShapeError):
        prove_openings(inst, [a, None], chal, params)
    with pytest.raises(GoldibearError) as e:
        prove_openings(FI.instance_from_tuples((3, 2), (False, True), [([0] * F.D, [(0, 0)])]), [a, b], chal, params)
    assert e.value.status == N.GB_ERR_UNSUPPORTED and e.value.challenger == chal
    # a size query, then a call with that size: the bytes and the transcript of a plain call
    for cap in (0, 100):
        st, msg, after, need, _ = raw(cap=cap)
        assert st == N.GB_ERR_BUFFER_TOO_SMALL and need == size and after == chal
    st, _, after, need, exact = raw(cap=size)
    assert st == N.GB_OK and exact == plain and after == after_good
    # and the context that refused all of the above still proves
    assert raw()[4] == plain
    a.free()
    b.free()
