"""MerkleTree.new (gb_merkle_tree_*) against the CPU oracle, bit for bit, both fields: the cap, then get(i) / prove(i) - every leaf
up to 1024 leaves, else 64 seeded indices plus 0 and L - 1 - and every path through merkle_verify.

Goldilocks: oracle.MerkleTree (cap, prove, and the whole `digests` vector in the reference's layout).  BabyBear: the tree is built
here from oracle_bb.hash_or_noop and two_to_one, level by level; every digest below the cap is the sibling of some path, so "every
path" covers every digest.  Shapes: one leaf; one leaf wider than a digest; cap = 0, 1, log L (no digests at all); leaf widths on
either side of the digest width (hash_or_noop's two branches) and of the sponge rate (8) and twice it; 2^16 leaves: the first
level above the cooperative kernels' limit (COOP_MAX_STATES).  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B
from plonky2_goldibear_amd import GpuContext, MerkleTree, PolynomialBatch, ShapeError
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _indices(L, seed):
    if L <= 1024:
        return range(L)
    return [0, L - 1] + [int(i) for i in np.random.default_rng(seed).integers(0, L, 64)]


def _shapes(widths, wide):
    return ([(1, 1, 0), (1, wide, 0), (2, 5, 0), (2, 5, 1), (16, 4, 4)] + [(1024, w, c) for w in widths for c in (0, 4)] +
            [(1 << 15, wide, 4), (1 << 16, 9, 0)])


def _ids(shapes):
    return ["%dx%d-cap%d" % s for s in shapes]


GL_SHAPES = _shapes((1, 4, 5, 8, 9, 16, 17, 135), 135)
BB_SHAPES = _shapes((1, 8, 9, 16, 17, 167), 167)

_bb_levels = {}   # (L, width) -> (leaves, [level 0 .. root]); shared by the cap heights of a shape, never modified


def bb_levels_of(leaves):
    """[level 0 .. root] of the BabyBear tree over `leaves`, from oracle_bb.hash_or_noop and two_to_one"""
    levels = [np.stack([B.hash_or_noop(r) for r in leaves])]
    while levels[-1].shape[0] > 1:
        d = levels[-1]
        levels.append(np.stack([B.two_to_one(d[2 * i], d[2 * i + 1]) for i in range(d.shape[0] // 2)]))
    return levels


def _bb_tree(L, width):
    if (L, width) not in _bb_levels:
        leaves = B.fill(7000 + 31 * L + width, L * width).reshape(L, width)
        leaves[0, 0], leaves[L - 1, width - 1] = 0, B.BB_P - 1
        _bb_levels[(L, width)] = (leaves, bb_levels_of(leaves))
    return _bb_levels[(L, width)]


def _check_paths(t, leaves, cap, prove, verify, seed):
    L = leaves.shape[0]
    for i in _indices(L, seed):
        row, sib = t.get(i), t.prove(i)
        assert np.array_equal(row, leaves[i]), "get(%d)" % i
        assert np.array_equal(sib, prove(i)), "prove(%d)" % i
        assert verify(row, i, cap, sib), "merkle_verify(%d)" % i


@pytest.mark.parametrize("L,width,cap_height", GL_SHAPES, ids=_ids(GL_SHAPES))
def test_goldilocks_tree(ctx, L, width, cap_height):
    leaves = O.splitmix64_fill(6000 + 31 * L + width, L * width).reshape(L, width)
    leaves[0, 0], leaves[L - 1, width - 1] = 0, O.GL_P - 1
    ref = O.MerkleTree(leaves, cap_height)
    t = MerkleTree.new(ctx, leaves, cap_height)
    assert np.array_equal(t.cap, ref.cap)
    got = t.digests
    assert got.shape == ref.digests.shape and np.array_equal(got, ref.digests)
    _check_paths(t, leaves, ref.cap, ref.prove, O.merkle_verify, L + width)
    assert np.array_equal(t.leaves, leaves)
    t.free()


@pytest.mark.parametrize("L,width,cap_height", BB_SHAPES, ids=_ids(BB_SHAPES))
def test_babybear_tree(ctx, L, width, cap_height):
    leaves, levels = _bb_tree(L, width)
    layers = (L.bit_length() - 1) - cap_height
    cap = levels[layers]

    def prove(i):
        return np.stack([levels[k][(i >> k) ^ 1] for k in range(layers)]) if layers else np.zeros((0, 8), dtype=np.uint32)
    t = MerkleTree.new(ctx, leaves, cap_height, field=N.GB_BABYBEAR)
    assert np.array_equal(t.cap, cap)
    _check_paths(t, leaves, cap, prove, B.merkle_verify, L + width)
    assert t.digests.shape == (2 * (L - (1 << cap_height)), 8)
    t.free()


@pytest.mark.parametrize("field,mod", [(N.GB_GOLDILOCKS, O), (N.GB_BABYBEAR, B)], ids=["goldilocks", "babybear"])
def test_tree_over_a_commitments_leaves_is_the_commitments_tree(ctx, field, mod):
    n, ncols = 1 << 12, 20
    coeffs = (O.splitmix64_fill(8000, ncols * n) if field == N.GB_GOLDILOCKS else B.fill(8000, ncols * n)).reshape(ncols, n)
    b = PolynomialBatch.from_coeffs(ctx, coeffs, 3, 4, field=field)
    leaves = b.merkle_tree.leaves
    t = MerkleTree.new(ctx, leaves, 4, field=field)
    assert np.array_equal(t.cap, b.merkle_tree.cap)
    assert np.array_equal(t.digests, b.merkle_tree.digests)
    for i in (0, 12345, (1 << 15) - 1):
        assert np.array_equal(t.get(i), b.merkle_tree.get(i)) and np.array_equal(t.prove(i), b.merkle_tree.prove(i))
    # the handle is a batch without polynomials: what needs coefficients says so instead of reading a null block
    out = np.zeros(n, dtype=leaves.dtype)
    assert ctx._lib.gb_batch_coeffs(t._b.handle, 0, out.ctypes.data) == N.GB_ERR_INVALID


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_device_leaves_and_p3_words(ctx, field):
    import torch
    gl = field == N.GB_GOLDILOCKS
    L, width = 1 << 11, 37
    leaves = (O.splitmix64_fill(8100, L * width) if gl else B.fill(8100, L * width)).reshape(L, width)
    host = MerkleTree.new(ctx, leaves, 3, field=field)
    dev = MerkleTree.new(ctx, torch.from_numpy(leaves.view(np.int64 if gl else np.int32)).cuda(), 3, field=field)
    if gl:
        words = leaves.copy()
        small = leaves < np.uint64((1 << 64) - O.GL_P)
        words[small] += np.uint64(O.GL_P)
        ref = O.MerkleTree(leaves, 3)
        assert np.array_equal(host.cap, ref.cap) and np.array_equal(host.digests, ref.digests)
    else:
        words = ((leaves.astype(np.uint64) << np.uint64(32)) % np.uint64(B.BB_P)).astype(np.uint32)
    p3 = MerkleTree.new(ctx, words, 3, field=field, p3_repr=True)
    for t in (dev, p3):
        assert np.array_equal(t.cap, host.cap) and np.array_equal(t.digests, host.digests)
        assert np.array_equal(t.get(L - 1), leaves[L - 1]) and np.array_equal(t.prove(77), host.prove(77))


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_errors(ctx, field):
    dt = np.uint64 if field == N.GB_GOLDILOCKS else np.uint32
    leaves = np.arange(8 * 5, dtype=dt).reshape(8, 5)
    with pytest.raises(ShapeError, match=r"cap_height=4 should be at most log2\(leaves.len\(\)\)=3"):
        MerkleTree.new(ctx, leaves, 4, field=field)
    h = C.c_void_p()
    assert ctx._lib.gb_merkle_tree_create(ctx.handle, field, leaves.ctypes.data, 3, 0, 0, 0, C.byref(h)) == N.GB_ERR_INVALID
    assert not h.value
    assert ctx._lib.gb_merkle_tree_create(ctx.handle, 2, leaves.ctypes.data, 3, 5, 0, 0, C.byref(h)) == N.GB_ERR_INVALID
    assert ctx._lib.gb_merkle_tree_create(ctx.handle, field, None, 3, 5, 0, 0, C.byref(h)) == N.GB_ERR_INVALID
    with pytest.raises(ShapeError):
        MerkleTree.new(ctx, leaves[:6], 0, field=field)       # not a power of two
    t = MerkleTree.new(ctx, leaves, 1, field=field)
    with pytest.raises(ShapeError):
        t.get(8)
    assert np.array_equal(t.get(7), leaves[7]) and t.prove(7).shape == (2, 4 if field == N.GB_GOLDILOCKS else 8)
    f, ll, w, ch = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert ctx._lib.gb_merkle_tree_info(t._b.handle, C.byref(f), C.byref(ll), C.byref(w), C.byref(ch)) == N.GB_OK
    assert (f.value, ll.value, w.value, ch.value) == (field, 3, 5, 1)
    n = C.c_uint32()
    assert ctx._lib.gb_merkle_tree_leaf(t._b.handle, 3, None, None, C.byref(n)) == N.GB_OK and n.value == 2


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_freed_trees_give_their_blocks_back_to_the_pool(field):
    """free, then create again, 32 times on one (fresh) context: a freed tree's blocks (and a host tree's upload block) go back to
    the context's pool, so the same few device blocks serve every tree - a leak would show as ever new addresses (and in the end
    as GB_ERR_OOM)"""
    dt = np.uint64 if field == N.GB_GOLDILOCKS else np.uint32
    L, width = 1 << 12, 1000
    leaves = (O.splitmix64_fill(8200, L * width) % np.uint64(B.BB_P)).astype(dt).reshape(L, width)
    ctx = GpuContext(0)
    try:
        cap0, seen = None, set()
        for k in range(32):
            t = MerkleTree.new(ctx, leaves, 2, field=field)
            a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert ctx._lib.gb_batch_device_ptrs(t._b.handle, C.byref(a), C.byref(b), C.byref(c)) == N.GB_OK
            assert a.value is None and b.value and c.value       # no coefficients; leaves; digest levels
            seen |= {b.value, c.value}
            cap = t.cap
            cap0 = cap if cap0 is None else cap0
            assert np.array_equal(cap, cap0)
            t.free()
        assert len(seen) <= 3, "the 32 trees used %d different device blocks" % len(seen)   # leaves, upload (same size), levels
    finally:
        ctx.close()
