"""gb_verify_compressed_batch (include/goldibear_gpu.h; csrc/verify_batch_host.inc, csrc/verify_compressed.hpp, csrc/kernels_verify.hip):
compressed proofs checked as they stand, the query rounds on the device.  The yardstick is the host's own gb_verify_compressed, proof
by proof: (status, text) must agree for every proof of every batch; where the proof still decompresses, the check, the query round and
the oracle / layer must be what gb_verify_batch reports on the decompressed bytes.  Compressed bytes come from gb_proof_compress
(tests/test_compression.py pins it to oracle/compression.py); structured mutations go through the oracle's reader and writer."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import compression as Z
from oracle import plonk_dummy as D
from oracle import verifier as V
from oracle.fields import GL
from plonky2_goldibear_amd import GpuContext, native as N
from plonky2_goldibear_amd.circuit_builder import CircuitConfig

from circuits import poly_chain_circuit, recursion_gates_circuit
from test_abi_verify_fixture import _fixture_circuit
from test_gpu_verify_batch import SHAPES as BATCH_SHAPES, _field, _gpu

pytestmark = pytest.mark.gpu

SCOPES = ("verify compressed batch: host stage", "verify compressed batch: upload", "verify compressed batch: queries",
          "verify compressed batch: paths")
SHAPES = [s for s in BATCH_SHAPES if s[0] != 13 and not (s[0] == 4 and s[2] is None)]   # the small ones, and one 2^12 with arity 2^8


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def host_verdicts(handle, err_ctx, proofs):
    """gb_verify_compressed, one proof at a time: (status, the text it leaves in gb_last_error)"""
    lib = N.load()
    out = []
    for p in proofs:
        buf = np.frombuffer(bytes(p) or b"\0", dtype=np.uint8)
        st = lib.gb_verify_compressed(handle, buf.ctypes.data, len(p))
        out.append((st, (lib.gb_last_error(err_ctx) or b"").decode() if st else ""))
    return out


def decompressed(handle, p):
    """gb_proof_decompress, or None where it refuses"""
    lib = N.load()
    buf = np.frombuffer(bytes(p) or b"\0", dtype=np.uint8)
    out = np.empty(1 << 20, dtype=np.uint8)
    n = C.c_size_t()
    if lib.gb_proof_decompress(handle, buf.ctypes.data, len(p), out.ctypes.data, out.size, C.byref(n)) != N.GB_OK:
        return None
    return out[:n.value].tobytes()


def compare(ctx, handle, err_ctx, proofs):
    want = host_verdicts(handle, err_ctx, proofs)
    got = N.verify_compressed_batch(ctx.handle, handle, proofs)
    assert len(got) == len(proofs)
    full = [decompressed(handle, p) for p in proofs]
    plain = iter(N.verify_batch(ctx.handle, handle, [f for f in full if f is not None]))
    for i, (r, (st, text)) in enumerate(zip(got, want)):
        assert (r.status, r.text) == (st, text), "proof %d: batch %r, gb_verify_compressed %r" % (i, r, (st, text))
        assert r.ok == (st == N.GB_OK) and (r.check == 0) == r.ok
        if full[i] is not None:
            b = next(plain)
            assert (r.status, r.check, r.query_round, r.index) == (b.status, b.check, b.query_round, b.index), (i, r, b)
    return got


def counted(ctx, handle, err_ctx, proofs, launches):
    """compare() with the timing scopes counted: `launches` uploads and launches of each kernel"""
    ctx.set_profiling(True)
    try:
        ctx.scope_reset()
        got = N.verify_compressed_batch(ctx.handle, handle, proofs)
        counts = [ctx.scope_ms(s)[1] for s in SCOPES]
        assert counts == [1, launches, launches, launches], counts
    finally:
        ctx.set_profiling(False)
        ctx.scope_reset()
    again = compare(ctx, handle, err_ctx, proofs)
    assert [(r.status, r.check, r.query_round, r.index) for r in got] == [(r.status, r.check, r.query_round, r.index) for r in again]
    return got


# ------------------------------------------------------------------------------------ what the query indices force to be shared
def trees_of(indices, lgN, cap_height, arity):
    """per tree (the oracles' one, then each layer's): (leaf index per query round, levels below the cap)"""
    out = [(list(indices), lgN - cap_height)]
    shift = 0
    for ab in arity:
        shift += ab
        out.append(([i >> shift for i in indices], lgN - shift - cap_height))
    return out


def dedup_cases(indices, lgN, cap_height, arity):
    """which of the cases (a)..(e) of shared data these indices produce"""
    found = set()
    if len(set(indices)) < len(indices):
        found.add("a")
    for leaves, levels in trees_of(indices, lgN, cap_height, arity):
        for level in range(levels):
            nodes = [i >> level for i in leaves]
            held = set(nodes)
            if any(n ^ 1 in held for n in nodes):
                found.add("b")
            below = {}
            for leaf, n in zip(leaves, nodes):
                below.setdefault(n, set()).add(leaf)
            for n, ls in below.items():
                if (len(ls) > 1 or nodes.count(n) > 1) and n ^ 1 not in held:
                    found.add("c")   # a node of several query rounds takes a stored sibling
    shift = 0
    for ab in arity:
        cosets = {}
        for i in indices:
            cosets.setdefault(i >> (shift + ab), []).append((i >> shift) & ((1 << ab) - 1))
        for ws in cosets.values():
            if len(set(ws)) > 1:
                found.add("d")
            if len(ws) > len(set(ws)):
                found.add("e")
        shift += ab
    return found


# ------------------------------------------------------------------------------------ structured mutations of a compressed proof
def mutations(cpr, pis, small, F, lgN, cap_height, arity):
    """[(name, bytes, check or None, regular)]: `regular` mutations keep every path as long as the indices demand, so the device
    must decide them"""
    fri = cpr["opening_proof"]
    indices = fri["indices"]
    bump = lambda x: (int(x) + 1) % F.P
    out = []

    def mutate(name, fn, check=None, regular=False, pis_=None):
        p = copy.deepcopy(cpr)
        fn(p["opening_proof"], p)
        out.append((name, Z.write_compressed_proof_with_pis(p, pis if pis_ is None else pis_, F), check, regular))

    first = indices[0]
    for o in range(4):
        def row(f, p, o=o, value=None):
            vals, path = f["initial_trees_proofs"][first][o]
            vals = list(vals)
            vals[1] = bump(vals[1]) if value is None else value
            f["initial_trees_proofs"][first][o] = (vals, path)
        mutate("row word, oracle %d" % o, row, N.GB_VCHECK_INITIAL_PATH, True)
    mutate("non-canonical row word", lambda f, p: row(f, p, 1, F.P), N.GB_VCHECK_NON_CANONICAL)

    # stored siblings: the entry with the longest stored path per tree - its last sibling lies highest, where most query rounds pass
    def sibling(tree, key, o, level):
        def fn(f, p):
            if tree == 0:
                vals, path = f["initial_trees_proofs"][key][o]
            else:
                vals, path = f["steps"][tree - 1][key]
            path = [list(h) for h in path]
            path[level][0] = bump(path[level][0])
            if tree == 0:
                f["initial_trees_proofs"][key][o] = (vals, path)
            else:
                f["steps"][tree - 1][key] = (vals, path)
        return fn

    def length(tree, key, o, delta):
        def fn(f, p):
            if tree == 0:
                vals, path = f["initial_trees_proofs"][key][o]
            else:
                vals, path = f["steps"][tree - 1][key]
            path = [list(h) for h in path]
            path = path[:-1] if delta < 0 else path + [[1] * len(path[0])]
            if tree == 0:
                f["initial_trees_proofs"][key][o] = (vals, path)
            else:
                f["steps"][tree - 1][key] = (vals, path)
        return fn

    stores = [(0, k, 2, e[2][1]) for k, e in fri["initial_trees_proofs"].items()]
    for li, st in enumerate(fri["steps"]):
        stores += [(li + 1, k, 0, e[1]) for k, e in st.items()]
    for tree in range(1 + len(arity)):
        mine = [s for s in stores if s[0] == tree and len(s[3])]
        if not mine:
            continue
        t, key, o, path = max(mine, key=lambda s: len(s[3]))
        kind = N.GB_VCHECK_INITIAL_PATH if tree == 0 else N.GB_VCHECK_LAYER_PATH
        mutate("bottom sibling, tree %d" % tree, sibling(t, key, o, 0), kind, True)
        mutate("top sibling, tree %d" % tree, sibling(t, key, o, -1), kind, True)
        mutate("missing sibling, tree %d" % tree, length(t, key, o, -1), N.GB_VCHECK_COMPRESSED_MISSING_SIBLING)
        mutate("surplus sibling, tree %d" % tree, length(t, key, o, +1), 0)

    # a stored evaluation of a coset that several query rounds share, at the place a later one reads
    shift = 0
    for li, ab in enumerate(arity):
        seen = {}
        for k, i in enumerate(indices):
            coset, within = i >> (shift + ab), (i >> shift) & ((1 << ab) - 1)
            if coset in seen and seen[coset] != within:
                at = seen[coset]

                def ev(f, p, li=li, coset=coset, j=within - (within > at)):
                    evals, path = f["steps"][li][coset]
                    evals = [tuple(e) for e in evals]
                    evals[j] = (bump(evals[j][0]),) + tuple(evals[j][1:])
                    f["steps"][li][coset] = (evals, path)
                mutate("evaluation in a shared coset, layer %d" % li, ev, "layer", True)
                break
            seen.setdefault(coset, within)
        shift += ab
    for li in range(len(arity)):
        def ev0(f, p, li=li):
            coset = min(f["steps"][li])
            evals, path = f["steps"][li][coset]
            evals = [tuple(e) for e in evals]
            evals[0] = (bump(evals[0][0]),) + tuple(evals[0][1:])
            f["steps"][li][coset] = (evals, path)
        mutate("evaluation, layer %d" % li, ev0, "layer", True)

    other = next((k for k, i in enumerate(indices) if i != indices[0]), None)
    if other is not None:
        def swap(f, p):
            f["indices"][0], f["indices"][other] = f["indices"][other], f["indices"][0]
        mutate("stored index", swap, N.GB_VCHECK_COMPRESSED_INDICES)

    def opening(f, p):
        w0 = p["openings"]["wires"][3]
        p["openings"]["wires"][3] = (bump(w0[0]),) + tuple(w0[1:])
    # (an opening, the witness and the final polynomial are part of the transcript: in this form the stored indices give them away
    # before the vanishing identity, the proof of work or a fold is looked at - whatever gb_verify_compressed says holds)
    mutate("opening", opening)

    def pow_witness(f, p):
        f["pow_witness"] = bump(f["pow_witness"])
    mutate("pow witness", pow_witness)

    def final_coeff(f, p):
        c = [tuple(e) for e in f["final_poly"]]
        c[-1] = (bump(c[-1][0]),) + tuple(c[-1][1:])
        f["final_poly"] = c
    mutate("final polynomial", final_coeff)
    mutate("public input count", lambda f, p: None, N.GB_VCHECK_PI_COUNT, pis_=list(pis) + [0])
    out.append(("truncated", small[:-9], None, False))   # (into the public inputs, which have no count: a truncation or a remainder)
    out.append(("cut in the entries", small[:len(small) // 2], N.GB_VCHECK_TRUNCATED, False))
    out.append(("trailing byte", small + b"\0", N.GB_VCHECK_COMPRESSED_TRAILING, False))
    out.append(("empty", b"", N.GB_VCHECK_TRUNCATED, False))
    return out


def run_mutations(ctx, handle, err_ctx, small, cd, F):
    fp = cd["fri_params"]
    arity = list(fp["reduction_arity_bits"])
    lgN = fp["degree_bits"] + fp["config"]["rate_bits"]
    cap_height = fp["config"]["cap_height"]
    cpr, pis = Z.read_compressed_proof_with_pis(small, cd, F)
    assert Z.write_compressed_proof_with_pis(cpr, pis, F) == small
    muts = mutations(cpr, pis, small, F, lgN, cap_height, arity)
    # the regular ones - row, sibling and evaluation words - in a batch of their own whose kernels are counted: one chunk, one
    # upload, one launch of each kernel, and no host walk behind it
    regular = [m for m in muts if m[3]]
    assert regular
    got = counted(ctx, handle, err_ctx, [small] + [m[1] for m in regular], 1)
    assert got[0].ok
    for (name, _, check, _), r in zip(regular, got[1:]):
        assert not r.ok and r.status == N.GB_ERR_VERIFY, (name, r)
        if check == "layer":
            assert r.check in (N.GB_VCHECK_CONSISTENCY, N.GB_VCHECK_LAYER_PATH), (name, r)
        else:
            assert r.check == check, (name, r)
        assert r.query_round is not None and r.index is not None, (name, r)
    rest = [m for m in muts if not m[3]]
    proofs = []
    for m in rest:   # interleaved with honest copies: a failing neighbour leaves them alone
        proofs += [m[1], small]
    got = compare(ctx, handle, err_ctx, proofs)
    for k, (name, _, check, _) in enumerate(rest):
        bad, good = got[2 * k], got[2 * k + 1]
        assert good.ok, name
        if check is not None:
            assert bad.check == check, (name, bad)
        assert bad.ok == (check == 0), (name, bad)
    return cpr


# ------------------------------------------------------------------------------------ the reference's own recursion proof
@pytest.fixture(scope="module")
def fixture(golden_dir):
    circ, cd, raw = _fixture_circuit(golden_dir)
    small = circ.compress(raw)
    assert circ.decompress(small) == raw
    yield circ, cd, raw, small
    circ.free()


def test_mutations_of_the_reference_proof(ctx, fixture):
    circ, cd, raw, small = fixture
    cpr = run_mutations(ctx, circ.handle, None, small, cd, GL)
    fp = cd["fri_params"]
    found = dedup_cases(cpr["opening_proof"]["indices"], fp["degree_bits"] + fp["config"]["rate_bits"], fp["config"]["cap_height"],
                        fp["reduction_arity_bits"])
    assert "b" in found or "c" in found   # 28 paths towards 16 cap entries share nodes
    assert circ.verify_compressed_batch(ctx, [small])[0].ok


def test_the_lowest_round_that_passes_a_shared_sibling_is_blamed(ctx, fixture):
    """a stored sibling of the wires tree beside a node that several query rounds have merged into: every one of them fails, and
    the first is named"""
    circ, cd, raw, small = fixture
    cpr, pis = Z.read_compressed_proof_with_pis(small, cd)
    fri = cpr["opening_proof"]
    indices = fri["indices"]
    fp = cd["fri_params"]
    levels = fp["degree_bits"] + fp["config"]["rate_bits"] - fp["config"]["cap_height"]
    hits = []
    for key, entry in fri["initial_trees_proofs"].items():
        path = entry[1][1]
        if not path:
            continue
        # which level the entry's last sibling stands at: replay the rule for this entry's first query round
        k = indices.index(key)
        took = [lv for lv in range(levels)
                if (key >> lv) ^ 1 not in {i >> lv for i in indices} and k == min(j for j, i in enumerate(indices) if i >> lv == key >> lv)]
        assert len(took) == len(path)
        for nth, lv in enumerate(took):
            rounds = [j for j, i in enumerate(indices) if i >> lv == key >> lv]
            if len(rounds) > 1:
                hits.append((key, nth, rounds))
    assert hits
    key, nth, rounds = hits[0]
    assert min(rounds) == indices.index(key)
    vals, path = fri["initial_trees_proofs"][key][1]
    path = [list(h) for h in path]
    path[nth][2] = (path[nth][2] + 1) % V.P
    fri["initial_trees_proofs"][key][1] = (vals, path)
    bad = Z.write_compressed_proof_with_pis(cpr, pis)
    r = counted(ctx, circ.handle, None, [small, bad, small], 1)[1]
    assert (r.check, r.query_round, r.index) == (N.GB_VCHECK_INITIAL_PATH, min(rounds), 1)


@pytest.mark.parametrize("count", [1, 3, 65])
def test_batch_sizes(ctx, fixture, count):
    circ, cd, raw, small = fixture
    bad = bytearray(small)
    bad[len(small) // 2] ^= 1
    bad_at = {1} if count == 3 else {i for i in range(count) if i % 7 == 2}   # failing proofs in the middle
    proofs = [bytes(bad) if i in bad_at else small for i in range(count)]
    want = host_verdicts(circ.handle, None, [small, bytes(bad)])
    assert want[0][0] == N.GB_OK and want[1][0] != N.GB_OK
    got = N.verify_compressed_batch(ctx.handle, circ.handle, proofs)
    assert len(got) == count
    for i, r in enumerate(got):
        assert (r.status, r.text) == want[i in bad_at], (i, r)


def test_chunks(ctx, fixture):
    circ, cd, raw, small = fixture
    bad = bytearray(small)
    bad[len(small) // 3] ^= 4
    proofs = [small, bytes(bad), small]
    whole = compare(ctx, circ.handle, None, proofs)
    ctx.set_option("verify_chunk_bytes", 4096)   # less than one proof: a chunk still holds one
    ctx.set_profiling(True)
    try:
        ctx.scope_reset()
        single = N.verify_compressed_batch(ctx.handle, circ.handle, [small] * 3)
        assert [ctx.scope_ms(s)[1] for s in SCOPES] == [3, 3, 3, 3] and all(r.ok for r in single)
        ctx.set_profiling(False)
        single = compare(ctx, circ.handle, None, proofs)
    finally:
        ctx.set_option("verify_chunk_bytes", 8 << 20)
        ctx.set_profiling(False)
        ctx.scope_reset()
    key = lambda rs: [(r.status, r.check, r.query_round, r.index) for r in rs]
    assert key(whole) == key(single) and [r.ok for r in whole] == [True, False, True]


def test_host_decided_proofs_send_nothing(ctx, fixture):
    """a truncated proof ends in the parser, a proof with a surplus sibling is walked on the host: no upload, no kernel"""
    circ, cd, raw, small = fixture
    cpr, pis = Z.read_compressed_proof_with_pis(small, cd)
    key = next(k for k, e in cpr["opening_proof"]["initial_trees_proofs"].items() if e[0][1])
    vals, path = cpr["opening_proof"]["initial_trees_proofs"][key][0]
    cpr["opening_proof"]["initial_trees_proofs"][key][0] = (vals, [list(h) for h in path] + [[7, 7, 7, 7]])
    surplus = Z.write_compressed_proof_with_pis(cpr, pis)
    got = counted(ctx, circ.handle, None, [small[:-9], surplus], 0)
    assert [r.ok for r in got] == [False, True]
    got = counted(ctx, circ.handle, None, [small[:-9], small, surplus], 1)
    assert [r.ok for r in got] == [False, True, True]


def test_arguments(ctx, fixture):
    circ, cd, raw, small = fixture
    lib = N.load()
    buf = np.frombuffer(small, dtype=np.uint8)
    ptrs, lens, res = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(small)), (N.gb_verify_result * 1)()
    resp = C.cast(res, C.c_void_p)
    call = lib.gb_verify_compressed_batch
    assert call(ctx.handle, circ.handle, ptrs, lens, 1, 0, resp) == N.GB_OK and res[0].status == N.GB_OK
    assert call(None, circ.handle, ptrs, lens, 1, 0, resp) == N.GB_ERR_INVALID and b"null ctx" in lib.gb_last_error(None)
    assert call(ctx.handle, circ.handle, ptrs, lens, 1, 1, resp) == N.GB_ERR_INVALID
    assert b"gb_verify_compressed_batch: flags" in lib.gb_last_error(ctx.handle)
    assert call(ctx.handle, circ.handle, None, None, 0, 0, None) == N.GB_OK
    assert call(ctx.handle, circ.handle, None, lens, 1, 0, resp) == N.GB_ERR_INVALID
    assert call(ctx.handle, circ.handle, ptrs, lens, 1, 0, None) == N.GB_ERR_INVALID
    assert call(ctx.handle, None, ptrs, lens, 1, 0, resp) == N.GB_ERR_INVALID
    assert call(ctx.handle, circ.handle, (C.c_void_p * 1)(None), lens, 1, 0, resp) == N.GB_ERR_INVALID
    other = GpuContext(0)
    try:
        circ_d = D.DummyCircuit(5)
        gpu = _gpu(other, circ_d, N.GB_GOLDILOCKS)
        p = gpu.compress(gpu.prove(circ_d.witness(seed=3)))
        assert gpu.verify_compressed_batch([p])[0].ok
        with pytest.raises(N.ShapeError, match="different context"):
            N.verify_compressed_batch(ctx.handle, gpu.handle, [p])
        gpu.free()
    finally:
        other.close()
    ptrs2 = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    lens2, res2 = (C.c_size_t * 2)(len(small), len(small) - 9), (N.gb_verify_result * 2)()
    assert call(ctx.handle, circ.handle, ptrs2, lens2, 2, 0, C.cast(res2, C.c_void_p)) == N.GB_ERR_VERIFY
    assert b"1 of 2" in lib.gb_last_error(ctx.handle) and res2[0].status == N.GB_OK and res2[1].status == N.GB_ERR_INVALID


# ------------------------------------------------------------------------------------ the device prover's own proofs, small shapes
_PROOFS = {}


def shape_proof(ctx, field_name, shape):
    """(circuit on the device, oracle circuit, compressed proof) of one shape; proved once"""
    key = (field_name,) + tuple(map(repr, shape))
    if key not in _PROOFS:
        degree_bits, kw, bits, zk = shape
        F, tag, mk = _field(field_name)
        circ = D.DummyCircuit(degree_bits, mk(**kw), check_security=False, F=F)
        if bits is not None:
            circ.reduction_arity_bits = list(bits)
        circ.zero_knowledge = zk
        gpu = _gpu(ctx, circ, tag, bits, zk)
        proof = None
        for attempt in range(6):   # (BabyBear: a zero denominator of the permutation argument is a natural event; next witness)
            try:
                proof = gpu.prove_once(circ.witness(seed=degree_bits + 100 * attempt), seed=bytes(range(32)) if zk else None)
                break
            except N.PermArgZeroError:
                continue
        assert proof is not None
        small = gpu.compress(proof)
        assert gpu.decompress(small) == proof
        _PROOFS[key] = (gpu, circ, small, proof)
    return _PROOFS[key]


def shape_indices(field_name, shape, circ, small, proof):
    """the transcript's query indices, from the oracle's verifier - the compressed proof stores the same"""
    F = _field(field_name)[0]
    cd = circ.common_data()
    cpr, pis = Z.read_compressed_proof_with_pis(small, cd, F)
    stored = cpr["opening_proof"]["indices"]
    if not shape[3]:
        pr, pis2 = V.read_proof_with_pis(proof, cd, F)
        assert list(V.get_challenges(pr, pis2, circ.circuit_digest, cd, F)["fri_query_indices"]) == list(stored)
    return stored, cd


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "2^%d-%s%s" % (s[0], s[2], "-zk" if s[3] else ""))
def test_device_proofs_of_the_dummy_circuit(ctx, field_name, shape):
    gpu, circ, small, proof = shape_proof(ctx, field_name, shape)
    F = _field(field_name)[0]
    indices, cd = shape_indices(field_name, shape, circ, small, proof)
    run_mutations(ctx, gpu.handle, ctx.handle, small, cd, F)


def test_every_way_of_sharing_occurs_in_some_shape(ctx):
    """a condition on the inputs: (a) a repeated index, (b) sibling nodes, (c) a merged node that takes a stored sibling, (d) one
    coset at two positions, (e) one coset at one position - each in at least one of the shapes above"""
    found = set()
    for field_name in ("goldilocks", "babybear"):
        for shape in SHAPES:
            gpu, circ, small, proof = shape_proof(ctx, field_name, shape)
            indices, cd = shape_indices(field_name, shape, circ, small, proof)
            fp = cd["fri_params"]
            found |= dedup_cases(indices, fp["degree_bits"] + fp["config"]["rate_bits"], fp["config"]["cap_height"],
                                 fp["reduction_arity_bits"])
    assert found == set("abcde"), found


def _flipped(small):
    out = [small]
    for num in (3, 5, 8):
        b = bytearray(small)
        b[len(b) * num // 10] ^= 1
        out.append(bytes(b))
    return out


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_four_rows(ctx, field):
    cfg = CircuitConfig.standard_recursion_config_gl() if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow()
    b, pw = poly_chain_circuit(cfg, 1)
    c = b.build(ctx)
    assert c.degree_bits == 2
    w, pis = c.generate_witness(pw)
    small = c.data.compress(c.data.prove(w, pis))
    got = compare(ctx, c.data.handle, ctx.handle, _flipped(small))
    assert got[0].ok and not any(r.ok for r in got[1:]) and c.verify_compressed_batch([small])[0].ok
    c.data.free()


def test_babybear_recursion_gates_circuit(ctx):
    b, pw, rows = recursion_gates_circuit(N.GB_BABYBEAR, seed=11, public_inputs=True)
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    small = c.data.compress(c.data.prove(w, pis, random_wire=(c.random_wire[1], c.random_wire[0])))
    got = counted(ctx, c.data.handle, ctx.handle, _flipped(small), 1)
    assert got[0].ok and not any(r.ok for r in got[1:])
    c.data.free()
