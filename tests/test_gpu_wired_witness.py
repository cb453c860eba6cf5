"""The prover kernels on data that is not zero and wiring that is not the identity (tests/wired_circuits.py), bit for bit against the
CPU oracle or an integer reference:
  * whole proofs and the stage entry points on the wired dummy circuit with carry-edge and with random witnesses, at 2^6 rows (less
    than one 256-row block), 2^10 (four blocks: k_zs_quotients' plain block mapping, one scan block) and 2^12 (sixteen blocks: the
    XCD-grouped mapping, four scan blocks, so k_zs_scan_totals and k_zs_finalize's carry-in multiply values that are not 1);
  * gb_zs_partial_products at challenges built from the edge values, chosen for the sums w + gamma they cause (w + gamma = p, in
    (p, 2^64), = 2^64, above it), against zs_partial_products_ref.  The census shows that the inputs reach those branches; the
    kernel multiplies w + gamma + ... lazily, so a sum that is merely left unreduced does not change its output
    (tests/test_device_field_edges.py checks the addition's own word);
  * gb_batch_eval_ext at structured points and coefficients;
  * MerkleTree.new over edge-word leaves, 2^10 and 2^15 of them, at widths on either side of the digest width and the sponge rate
    (2^10: cooperative leaf kernels for leaves that are hashed; 2^15: lane-per-leaf; the digest levels stay cooperative).
-m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GpuContext, MerkleTree, PermArgZeroError, PolynomialBatch, VerifyError
from plonky2_goldibear_amd import native as N
from test_gpu_merkle_tree import bb_levels_of
from test_gpu_stage_abi import prove_by_stages
import wired_circuits as W

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": (GL, N.GB_GOLDILOCKS), "babybear": (BB, N.GB_BABYBEAR)}


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _config(F):
    return D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)


def _wired(ctx, F, degree_bits, seed, dense):
    circ, w, kw = W.wired_dummy_circuit(F, _config(F), degree_bits, seed, dense)
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    circ.set_cap(gpu.constants_sigmas_cap)
    return circ, w, gpu


@pytest.mark.parametrize("dense", ["edges", "random"])
@pytest.mark.parametrize("degree_bits", [6, 10, 12])
@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_wired_proof_and_stages_equal_the_oracle_prover(ctx, field_name, degree_bits, dense):
    F, tag = FIELDS[field_name]
    circ, w, gpu = _wired(ctx, F, degree_bits, 200 + degree_bits, dense)
    dump, mid = {}, {}
    want, dbg = D.prove_cpu(circ, w, dump=dump)
    c = circ.cfg.num_challenges
    assert (dump["zs_partial_products"][:c] != 1).sum(axis=1).min() >= circ.n // 4   # the permutation argument has work to do
    assert gpu.prove(w) == want
    got = prove_by_stages(gpu, circ, w, [], tag, mid)
    assert mid["betas"] == [int(x) for x in dbg[:c]] and mid["gammas"] == [int(x) for x in dbg[c:2 * c]]
    bad = np.argwhere(mid["zs_partial_products"] != dump["zs_partial_products"])
    assert bad.size == 0, "zs_partial_products: first difference at (column, row) %r" % (bad[0].tolist(),)
    bad = np.argwhere(mid["quotient_chunks"] != dump["quotient_chunks"])
    assert bad.size == 0, "quotient_chunks: first difference at (column, coefficient) %r" % (bad[0].tolist(),)
    assert got == want
    assert gpu.verify(want) and D.verify(circ, want)
    # one member of a copy class changed: the proof the GPU then makes is refused by gb_verify, as by the oracle's verifier
    broken = gpu.prove(W.break_copy_constraint(circ, w))
    with pytest.raises(VerifyError, match="vanishing polynomial identity"):
        gpu.verify(broken)
    with pytest.raises(AssertionError, match="vanishing"):
        D.verify(circ, broken)
    gpu.free()


def _challenge_sets(F):
    """three (betas, gammas) per field from edge_values: beta = 1, p - 1 and 2^32 (2^27 for BabyBear) among them; the gammas meet
    witness values w with w + gamma = p, = 2^64 and on either side (w = p - 1, 2^63, p - 2^32, 2^32 .. are all in the witness)"""
    p = F.P
    if F is GL:
        return [([1, p - 1], [1, 2**63]),
                ([2**32, p - 2**32], [2**32, p - 1]),
                ([(p + 1) // 2, 2], [p - 2**32 + 1, 2**32 - 1])]
    ev = W.edge_values(BB)
    return [([1, p - 1, 2**27, ev[9], 2, (p + 1) // 2], [1, p - 1, 2**27 + 1, ev[13], (p - 1) // 2, p - 2]),
            ([ev[13], 2**27 + 1, 1, p - 2, ev[11], p - 1], [ev[9], ev[10], 2, 2**27, (p + 1) // 2, ev[12]]),
            ([(p - 1) // 2, ev[12], ev[10], p - 1, 1, 2**27], [p - 1, 1, ev[11], ev[13], 2**27, ev[9]])]


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_zs_partial_products_at_edge_challenges(ctx, field_name):
    F, tag = FIELDS[field_name]
    degree_bits = 11
    # (seed 311 gives BabyBear a cell with w = sigma = p - 1, whose denominator w + beta sigma + gamma is 0 whenever gamma = beta + 1)
    circ, w, gpu = _wired(ctx, F, degree_bits, 311 if F is GL else 312, "edges")
    nr, chunk = circ.cfg.num_routed_wires, circ.cfg.max_quotient_degree_factor
    ev = set(W.edge_values(F))
    refs, total = [], dict.fromkeys(W.CENSUS_CLASSES, 0)
    for betas, gammas in _challenge_sets(F):
        assert set(betas) | set(gammas) <= ev
        ref, census = W.zs_partial_products_ref(F, w, circ.sigma, circ.k_is, betas, gammas, degree_bits, chunk)
        refs.append((betas, gammas, ref))
        for k, v in census.items():
            total[k] += v
    print("census of w + gamma:", total)
    # every kind of sum the device addition distinguishes occurs (BabyBear words are below p: their sum stays below 2p)
    reachable = W.CENSUS_CLASSES if F is GL else W.CENSUS_CLASSES[:3]
    assert all(total[k] > 0 for k in reachable), total
    for betas, gammas, ref in refs:
        got = gpu.zs_partial_products(w, betas, gammas)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "betas %r gammas %r: first difference at (column, row) %r" % (betas, gammas, bad[0].tolist())
    # a denominator that vanishes only through the wrap: w = p - 1, gamma = 1, beta = 0
    assert (w[:nr] == F.P - 1).any()
    c = circ.cfg.num_challenges
    with pytest.raises(PermArgZeroError):
        gpu.zs_partial_products(w, [0] + [1] * (c - 1), [1] * c)
    gpu.free()


_horner = {}   # (field, column bytes, z) -> value; the batches of one field share columns across the parametrised shapes


def _eval_ref(F, column, z):
    key = (F.name, column.tobytes(), z)
    if key not in _horner:
        _horner[key] = W.horner_ext(F, column, z)
    return _horner[key]


@pytest.mark.parametrize("ncols", [1, 3, 17])
@pytest.mark.parametrize("log_n", [4, 8, 12])
@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_eval_ext_at_structured_points(ctx, field_name, log_n, ncols):
    F, tag = FIELDS[field_name]
    p, n, d = F.P, 1 << log_n, F.D
    ev = np.array(W.edge_values(F), dtype=F.dtype)
    top = np.zeros((ncols, n), dtype=F.dtype)
    top[:, n - 1] = [p - 1 if c % 2 == 0 else 1 for c in range(ncols)]
    batches = {"all p - 1": np.full((ncols, n), p - 1, dtype=F.dtype),
               "edge cycle": ev[np.arange(ncols * n) % len(ev)].reshape(ncols, n),
               "top coefficient only": top}
    pad = (0,) * (d - 1)
    points = [(0,) + pad, (1,) + pad, (p - 1,) + pad, (0, 1) + (0,) * (d - 2), (p - 1,) * d, (F.two_adic_generator(log_n),) + pad,
              (2**32 % p,) * d]
    for name, coeffs in batches.items():
        b = PolynomialBatch.from_coeffs(ctx, coeffs, 1, 0, field=tag)
        for z in points:
            got = b.eval_ext(np.array(z, dtype=F.dtype))
            for c in range(ncols):
                assert tuple(int(x) for x in got[c]) == _eval_ref(F, coeffs[c], z), "%s, column %d, z = %r" % (name, c, z)
        b.free()


def _edge_leaves(F, L, width):
    """leaves[r][c] = edge_values[(offset_r + c * stride_r) mod len]: every row cycles through the edge words from its own offset"""
    ev = np.array(W.edge_values(F), dtype=F.dtype)
    rng = np.random.default_rng(9000 + 31 * L + width)
    off, stride = rng.integers(0, len(ev), L), rng.integers(1, len(ev), L)
    return ev[(off[:, None] + np.arange(width)[None, :] * stride[:, None]) % len(ev)]


def _path_indices(L):
    return [0, L - 1] + [int(i) for i in np.random.default_rng(L).integers(0, L, 64)]


@pytest.mark.parametrize("width", [5, 8, 9, 17])
@pytest.mark.parametrize("L", [1 << 10, 1 << 15], ids=["2^10-leaves", "2^15-leaves"])
def test_goldilocks_tree_over_edge_words(ctx, L, width):
    leaves = _edge_leaves(GL, L, width)
    ref = O.MerkleTree(leaves, 4)
    t = MerkleTree.new(ctx, leaves, 4)
    assert np.array_equal(t.cap, ref.cap)
    assert np.array_equal(t.digests, ref.digests)
    for i in _path_indices(L):
        row, sib = t.get(i), t.prove(i)
        assert np.array_equal(row, leaves[i]) and np.array_equal(sib, ref.prove(i)), "leaf %d" % i
        assert O.merkle_verify(row, i, ref.cap, sib)
    t.free()


@pytest.mark.parametrize("width", [5, 8, 9, 17])
@pytest.mark.parametrize("L", [1 << 10, 1 << 15], ids=["2^10-leaves", "2^15-leaves"])
def test_babybear_tree_over_edge_words(ctx, L, width):
    from oracle import oracle_bb as B
    leaves = _edge_leaves(BB, L, width)
    levels = bb_levels_of(leaves)
    layers = (L.bit_length() - 1) - 4
    cap = levels[layers]
    t = MerkleTree.new(ctx, leaves, 4, field=N.GB_BABYBEAR)
    assert np.array_equal(t.cap, cap)
    for i in _path_indices(L):
        row, sib = t.get(i), t.prove(i)
        assert np.array_equal(row, leaves[i]), "leaf %d" % i
        assert np.array_equal(sib, np.stack([levels[k][(i >> k) ^ 1] for k in range(layers)])), "path %d" % i
        assert B.merkle_verify(row, i, cap, sib)
    t.free()
