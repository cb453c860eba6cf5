"""gb_verify_batch (include/goldibear_gpu.h; csrc/verify_batch_host.inc, csrc/kernels_verify.hip): the query rounds of many proofs
checked on the device.  The contract is gb_verify's own answer, proof by proof: every case here calls gb_verify on each proof and
gb_verify_batch on the whole list and compares (status, text) pair by pair - and, where the mutation's place is known, the query
round and the oracle / layer the result names.  gb_verify's texts carry no round, so those come from the mutation itself."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import plonk_dummy as D
from oracle import verifier as V
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, native as N
from plonky2_goldibear_amd.circuit_builder import CircuitConfig
from plonky2_goldibear_amd.prover import CircuitData

import gate_programs as GP
from circuits import poly_chain_circuit, recursion_gates_circuit
from test_abi_verify_fixture import _fixture_circuit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def host_verdicts(circuit_handle, err_ctx, proofs):
    """gb_verify, one proof at a time: (status, the text it leaves in gb_last_error)"""
    lib = N.load()
    out = []
    for p in proofs:
        buf = np.frombuffer(bytes(p) or b"\0", dtype=np.uint8)
        st = lib.gb_verify(circuit_handle, buf.ctypes.data, len(p))
        out.append((st, (lib.gb_last_error(err_ctx) or b"").decode() if st else ""))
    return out


def compare(ctx, circuit_handle, err_ctx, proofs):
    want = host_verdicts(circuit_handle, err_ctx, proofs)
    got = N.verify_batch(ctx.handle, circuit_handle, proofs)
    assert len(got) == len(proofs)
    for i, (r, (st, text)) in enumerate(zip(got, want)):
        assert (r.status, r.text) == (st, text), "proof %d: batch %r, gb_verify %r" % (i, r, (st, text))
        assert r.ok == (st == N.GB_OK) and (r.check == 0) == r.ok
    return got


# ------------------------------------------------------------------------------------ the reference's own recursion proof, mutated
@pytest.fixture(scope="module")
def fixture(golden_dir):
    circ, cd, raw = _fixture_circuit(golden_dir)
    proof, pis = V.read_proof_with_pis(raw, cd)
    assert V.write_proof_with_pis(proof, pis) == raw
    yield circ, cd, raw, proof, pis
    circ.free()


def _bump(x):
    return (int(x) + 1) % V.P


def _mutations(proof, pis, raw):
    """[(name, bytes, expectation)], expectation = None or (check, query_round, index) where the place of the failure is known"""
    nqr = len(proof["opening_proof"]["query_round_proofs"])
    nl = len(proof["opening_proof"]["commit_phase_merkle_caps"])
    out = []

    def mutate(name, fn, expect=None, pis_=None):
        p = copy.deepcopy(proof)
        fn(p)
        out.append((name, V.write_proof_with_pis(p, pis if pis_ is None else pis_), expect))

    def rounds(p):
        return p["opening_proof"]["query_round_proofs"]

    def set_row(r, o, k, value=None):
        def fn(p):
            vals, path = rounds(p)[r]["initial_trees_proof"][o]
            vals = list(vals)
            vals[k] = _bump(vals[k]) if value is None else value
            rounds(p)[r]["initial_trees_proof"][o] = (vals, path)
        return fn

    def set_sibling(r, o, level):
        def fn(p):
            vals, path = rounds(p)[r]["initial_trees_proof"][o]
            path = [list(h) for h in path]
            path[level][1] = _bump(path[level][1])
            rounds(p)[r]["initial_trees_proof"][o] = (vals, path)
        return fn

    def set_step_row(r, li, k):
        def fn(p):
            evals, path = rounds(p)[r]["steps"][li]
            evals = [tuple(e) for e in evals]
            evals[k] = (_bump(evals[k][0]),) + tuple(evals[k][1:])
            rounds(p)[r]["steps"][li] = (evals, path)
        return fn

    def set_step_sibling(r, li, level):
        def fn(p):
            evals, path = rounds(p)[r]["steps"][li]
            path = [list(h) for h in path]
            path[level][0] = _bump(path[level][0])
            rounds(p)[r]["steps"][li] = (evals, path)
        return fn

    def cap_word(p):
        cap = [list(h) for h in p["wires_cap"]]
        cap[1][2] = _bump(cap[1][2])
        p["wires_cap"] = cap

    def opening(p):
        w0 = p["openings"]["wires"][17]
        p["openings"]["wires"][17] = (_bump(w0[0]), w0[1])

    def pow_witness(p):
        p["opening_proof"]["pow_witness"] = _bump(p["opening_proof"]["pow_witness"])

    def final_coeff(p):
        f = [tuple(e) for e in p["opening_proof"]["final_poly"]]
        f[3] = (f[3][0], _bump(f[3][1]))
        p["opening_proof"]["final_poly"] = f

    def head_word(value):
        def fn(p):
            cap = [list(h) for h in p["zs_cap"]]
            cap[0][0] = value
            p["zs_cap"] = cap
        return fn

    mutate("cap word", cap_word)
    mutate("opening", opening, (N.GB_VCHECK_VANISHING, None, None))
    mutate("pow witness", pow_witness)
    mutate("final polynomial coefficient", final_coeff)
    if len(pis):
        mutate("public input", lambda p: None, pis_=[_bump(pis[0])] + list(pis[1:]))
    mutate("public input count", lambda p: None, (N.GB_VCHECK_PI_COUNT, None, None), pis_=list(pis) + [0])
    for v in (V.P, 2 ** 64 - 1):
        mutate("non-canonical head word %x" % v, head_word(v), (N.GB_VCHECK_NON_CANONICAL, None, None))
    out.append(("truncated", raw[:-9], (N.GB_VCHECK_TRUNCATED, None, None)))
    out.append(("trailing byte", raw + b"\0", (N.GB_VCHECK_TRAILING, None, None)))
    out.append(("empty", b"", (N.GB_VCHECK_TRUNCATED, None, None)))

    def short_path(p):
        vals, path = rounds(p)[3]["initial_trees_proof"][2]
        rounds(p)[3]["initial_trees_proof"][2] = (vals, path[:-2])
    mutate("short path", short_path, (N.GB_VCHECK_INITIAL_PATH_LEN, 3, 2))

    for r in (0, nqr - 1):
        for v in (V.P, 2 ** 64 - 1):
            mutate("non-canonical word %x in round %d" % (v, r), set_row(r, 1, 5, v), (N.GB_VCHECK_NON_CANONICAL, None, None))
        for o in range(4):
            mutate("row element, oracle %d, round %d" % (o, r), set_row(r, o, 1), (N.GB_VCHECK_INITIAL_PATH, r, o))
        # salts are hashed but never combined: only the path check sees them
        mutate("salt word, round %d" % r, set_row(r, 1, -1), (N.GB_VCHECK_INITIAL_PATH, r, 1))
        mutate("bottom sibling, round %d" % r, set_sibling(r, 2, 0), (N.GB_VCHECK_INITIAL_PATH, r, 2))
        mutate("top sibling, round %d" % r, set_sibling(r, 3, -1), (N.GB_VCHECK_INITIAL_PATH, r, 3))
        for li in (0, nl - 1):
            # (which element of the coset the query reads depends on the index: the consistency check or the layer's path fails)
            mutate("step row, layer %d, round %d" % (li, r), set_step_row(r, li, 0), ("layer", r, li))
            if len(rounds(proof)[r]["steps"][li][1]):
                mutate("step sibling, layer %d, round %d" % (li, r), set_step_sibling(r, li, -1), (N.GB_VCHECK_LAYER_PATH, r, li))

    def two(p):   # a later round's Merkle sibling and an earlier round's step row: the earlier one is reported
        set_sibling(nqr - 3, 0, 2)(p)
        set_step_row(5, 1, 0)(p)
    mutate("two mutations", two, ("layer", 5, 1))
    return out


def test_mutations_of_the_reference_proof(ctx, fixture):
    circ, cd, raw, proof, pis = fixture
    muts = _mutations(proof, pis, raw)
    proofs = []
    for _, b, _ in muts:   # interleaved with honest copies, which must come back GB_OK: a failing neighbour leaves them alone
        proofs += [b, raw]
    got = compare(ctx, circ.handle, None, proofs)
    for k, (name, _, expect) in enumerate(muts):
        bad, good = got[2 * k], got[2 * k + 1]
        assert good.ok, name
        assert not bad.ok, name
        if expect is None:
            continue
        check, qr, idx = expect
        if check == "layer":
            assert bad.check in (N.GB_VCHECK_CONSISTENCY, N.GB_VCHECK_LAYER_PATH), (name, bad)
        else:
            assert bad.check == check, (name, bad)
        assert (bad.query_round, bad.index) == (qr, idx), (name, bad)
    # the salted rows still verify unmutated (the fixture is zero-knowledge), and a verifier object without a context of its own
    # is served by the caller's
    assert cd["fri_params"]["hiding"] and circ.verify_batch(ctx, [raw])[0].ok


@pytest.mark.parametrize("count", [1, 3, 65])
def test_batch_sizes(ctx, fixture, count):
    circ, cd, raw, proof, pis = fixture
    bad = bytearray(raw)
    bad[len(raw) // 2] ^= 1
    proofs = [bytes(bad) if i % 7 == 2 else raw for i in range(count)]
    got = compare(ctx, circ.handle, None, proofs)
    assert [r.ok for r in got] == [i % 7 != 2 for i in range(count)]


def test_chunks_and_repetition(ctx, fixture):
    circ, cd, raw, proof, pis = fixture
    muts = [b for _, b, e in _mutations(proof, pis, raw) if e and e[1] is not None][:5]
    fails = [i % 2 == 1 or i == 8 for i in range(9)]              # a failing proof in each of the five chunks below
    proofs = [muts[i // 2] if fails[i] else raw for i in range(9)]
    whole = compare(ctx, circ.handle, None, proofs)
    ctx.set_option("verify_chunk_bytes", 2 * len(raw) + len(raw) // 2)   # two proofs per chunk: five chunks
    try:
        first = compare(ctx, circ.handle, None, proofs)
        again = compare(ctx, circ.handle, None, proofs)
        ctx.set_option("verify_chunk_bytes", 4096)                       # less than one proof: a chunk still holds one
        single = compare(ctx, circ.handle, None, proofs)
    finally:
        ctx.set_option("verify_chunk_bytes", 8 << 20)
    key = lambda rs: [(r.status, r.check, r.query_round, r.index) for r in rs]
    assert key(first) == key(again) == key(whole) == key(single)
    assert [r.ok for r in whole] == [not f for f in fails]
    with pytest.raises(N.ShapeError):
        ctx.set_option("verify_chunk_bytes", 100)


def test_the_query_rounds_run_on_the_device(ctx, fixture):
    """the timing scopes: one upload, one launch of each kernel per chunk that holds a regular proof - a proof that fails on the
    host (here: truncated) or whose paths have another length (walked on the host) sends nothing"""
    circ, cd, raw, proof, pis = fixture
    short = copy.deepcopy(proof)
    vals, path = short["opening_proof"]["query_round_proofs"][3]["initial_trees_proof"][2]
    short["opening_proof"]["query_round_proofs"][3]["initial_trees_proof"][2] = (vals, path[:-2])
    irregular = V.write_proof_with_pis(short, pis)
    scopes = ("verify batch: host stage", "verify batch: upload", "verify batch: paths", "verify batch: queries")
    ctx.set_profiling(True)
    try:
        for proofs, launches in (([raw, raw[:-9], raw], 1), ([raw[:-9], irregular], 0), ([raw], 1)):
            ctx.scope_reset()
            got = circ.verify_batch(ctx, proofs)
            assert [r.ok for r in got] == [p is raw for p in proofs]
            counts = [ctx.scope_ms(s)[1] for s in scopes]
            assert counts == [1, launches, launches, launches], (counts, launches)
        ctx.set_option("verify_chunk_bytes", 4096)   # a proof per chunk
        ctx.scope_reset()
        assert all(r.ok for r in circ.verify_batch(ctx, [raw] * 3))
        assert [ctx.scope_ms(s)[1] for s in scopes] == [3, 3, 3, 3]
    finally:
        ctx.set_option("verify_chunk_bytes", 8 << 20)
        ctx.set_profiling(False)
        ctx.scope_reset()


def test_arguments(ctx, fixture):
    circ, cd, raw, proof, pis = fixture
    lib = N.load()
    buf = np.frombuffer(raw, dtype=np.uint8)
    ptrs, lens, res = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(raw)), (N.gb_verify_result * 1)()
    resp = C.cast(res, C.c_void_p)
    assert lib.gb_verify_batch(ctx.handle, circ.handle, ptrs, lens, 1, 0, resp) == N.GB_OK and res[0].status == N.GB_OK
    assert lib.gb_verify_batch(ctx.handle, circ.handle, ptrs, lens, 1, 1, resp) == N.GB_ERR_INVALID and b"flags" in lib.gb_last_error(ctx.handle)
    assert lib.gb_verify_batch(ctx.handle, circ.handle, None, None, 0, 0, None) == N.GB_OK
    assert lib.gb_verify_batch(ctx.handle, circ.handle, None, lens, 1, 0, resp) == N.GB_ERR_INVALID
    assert lib.gb_verify_batch(ctx.handle, circ.handle, ptrs, None, 1, 0, resp) == N.GB_ERR_INVALID
    assert lib.gb_verify_batch(ctx.handle, circ.handle, ptrs, lens, 1, 0, None) == N.GB_ERR_INVALID
    assert lib.gb_verify_batch(ctx.handle, None, ptrs, lens, 1, 0, resp) == N.GB_ERR_INVALID
    assert lib.gb_verify_batch(ctx.handle, circ.handle, (C.c_void_p * 1)(None), lens, 1, 0, resp) == N.GB_ERR_INVALID
    # a circuit of another context
    other = GpuContext(0)
    try:
        circ_d = D.DummyCircuit(5)
        gpu = _gpu(other, circ_d, N.GB_GOLDILOCKS)
        p = gpu.prove(circ_d.witness(seed=3))
        assert gpu.verify_batch([p])[0].ok
        with pytest.raises(N.ShapeError, match="different context"):
            N.verify_batch(ctx.handle, gpu.handle, [p])
        gpu.free()
    finally:
        other.close()
    # a bad proof among good ones: GB_ERR_VERIFY, and the message names the first
    bad = raw[:-9]
    ptrs2 = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    lens2, res2 = (C.c_size_t * 2)(len(raw), len(bad)), (N.gb_verify_result * 2)()
    assert lib.gb_verify_batch(ctx.handle, circ.handle, ptrs2, lens2, 2, 0, C.cast(res2, C.c_void_p)) == N.GB_ERR_VERIFY
    assert b"1 of 2" in lib.gb_last_error(ctx.handle) and res2[0].status == N.GB_OK and res2[1].status == N.GB_ERR_INVALID


# ------------------------------------------------------------------------------------ the device prover's own proofs, small shapes
def _field(name):
    return (GL, N.GB_GOLDILOCKS, D.CircuitConfig) if name == "goldilocks" else (BB, N.GB_BABYBEAR, D.CircuitConfig.babybear)


def _gpu(ctx, circ, tag, bits=None, zero_knowledge=False):
    cfg = circ.cfg
    return CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                       num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                       max_quotient_degree_factor=cfg.max_quotient_degree_factor, rate_bits=cfg.rate_bits, cap_height=cfg.cap_height,
                       proof_of_work_bits=cfg.proof_of_work_bits, num_query_rounds=cfg.num_query_rounds, arity_bits=cfg.arity_bits,
                       final_poly_bits=cfg.final_poly_bits, gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI, field=tag,
                       reduction_arity_bits=bits, zero_knowledge=zero_knowledge)


def _flipped(proof):
    """the honest proof and copies with one byte flipped, at places spread over the query rounds (which fill all but the ends)"""
    out = [proof]
    for num in (3, 5, 8):
        b = bytearray(proof)
        b[len(b) * num // 10] ^= 1
        out.append(bytes(b))
    return out


# (degree_bits, config, reduction list or None, zero-knowledge); the dummy circuit starts at 2^3 rows (2^2: test_four_rows)
SHAPES = [
    (3, {}, None, False),                                   # no FRI layer: the reduction list is empty
    (4, {}, None, False),
    (5, {}, [1, 1, 1], False),                              # a layer leaf of exactly H words (hash_or_noop) in both fields
    (4, {}, [3], False),                                    # the layer's tree exactly as high as the cap: a path of length zero
    (5, dict(cap_height=0), [2, 1], False),
    (6, {}, [2], True),                                     # salted rows
    (7, dict(num_query_rounds=70), [3], False),             # a proof spans waves
    (12, {}, [8, 3], False),
    (13, {}, [5, 6, 1], False),
]


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
@pytest.mark.parametrize("degree_bits,kw,bits,zk", SHAPES)
def test_device_proofs_of_the_dummy_circuit(ctx, field_name, degree_bits, kw, bits, zk):
    F, tag, mk = _field(field_name)
    circ = D.DummyCircuit(degree_bits, mk(**kw), check_security=False, F=F)
    if bits is not None:
        circ.reduction_arity_bits = list(bits)
    else:
        bits_ = circ.reduction_arity_bits
        assert degree_bits > 4 or not bits_
    gpu = _gpu(ctx, circ, tag, bits, zk)
    proof = None
    for attempt in range(6):   # (BabyBear: a zero denominator of the permutation argument is a natural event; next witness)
        try:
            proof = gpu.prove_once(circ.witness(seed=degree_bits + 100 * attempt), seed=bytes(range(32)) if zk else None)
            break
        except N.PermArgZeroError:
            continue
    assert proof is not None
    got = compare(ctx, gpu.handle, ctx.handle, _flipped(proof))
    assert got[0].ok and not any(r.ok for r in got[1:])
    gpu.free()


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_four_rows(ctx, field):
    """degree_bits 2 (the dummy circuit starts at 2^3 rows): a builder circuit of one multiply-add, no FRI layer"""
    cfg = CircuitConfig.standard_recursion_config_gl() if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow()
    b, pw = poly_chain_circuit(cfg, 1)
    c = b.build(ctx)
    assert c.degree_bits == 2
    w, pis = c.generate_witness(pw)
    proof = c.data.prove(w, pis)
    got = compare(ctx, c.data.handle, ctx.handle, _flipped(proof))
    assert got[0].ok and not any(r.ok for r in got[1:])
    c.data.free()


def test_babybear_recursion_gates_circuit(ctx):
    b, pw, rows = recursion_gates_circuit(N.GB_BABYBEAR, seed=11, public_inputs=True)
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    proof = c.data.prove(w, pis, random_wire=(c.random_wire[1], c.random_wire[0]))
    got = compare(ctx, c.data.handle, ctx.handle, _flipped(proof))
    assert got[0].ok and not any(r.ok for r in got[1:])
    c.data.free()


def test_a_circuit_with_program_gates(ctx):
    b, pw = recursion_gates_circuit(N.GB_GOLDILOCKS, seed=5)[:2]
    GP.with_program_gates(b)
    c = b.build(ctx)
    from plonky2_goldibear_amd.gate_program import GATE_PROGRAM
    assert any(g[0] == GATE_PROGRAM for g in c.gate_table)
    w, pis = c.generate_witness(pw)
    proof = c.data.prove(w, pis, random_wire=(c.random_wire[1], c.random_wire[0]))
    got = compare(ctx, c.data.handle, ctx.handle, _flipped(proof))
    assert got[0].ok and not any(r.ok for r in got[1:])
    c.data.free()
