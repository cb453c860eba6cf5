"""The product's permutations on states pulled back from chosen round words (tests/permutation_states.py), against the oracle.

ctx.permute (k_gl_poseidon_permute: permute_mont_mfma_grouped; k_bb_permute: poseidon2_bb::permute) runs every generated input in two
layouts: as generated, so the lanes of a wave differ, and a seeded subset of 320 states with each state repeated 64 times and
aligned to a wave, so all lanes of a wave take the same data-dependent path (the wave-uniform any_carry branch of the MDS folds
included).  The oracle's value is computed once per distinct state.

MerkleTree.new hashes leaves made of the zero-capacity states, cap_height 0, whole `digests` vector against the oracle's tree:
  Goldilocks (kernels_merkle.hip, COOP_MAX_STATES = 16384; leaves wider than 4 are hashed)
    L = 1024:  k_gl_merkle_leaves_coop (poseidon_gl_coop::permute), every level k_gl_merkle_level_coop
    L = 2^15:  k_gl_merkle_leaves - width 8: one permutation with zero_capacity; width 16: capacity_only + zero_capacity, then a
               full one - and k_gl_merkle_level_coop for every level (the first has 2^14 nodes, not above the limit)
  BabyBear (kernels_bb.hip, BB_COOP_MAX_STATES = 16384; leaves of width <= 8 are NOT hashed: hash_or_noop copies them, so at
  width 8 the structured words first meet a permutation in the first level's two_to_one, as words 0..15 of a full state)
    L = 1024:  width 16: k_bb_merkle_leaves_coop (poseidon2_bb_coop::permute); every level k_bb_merkle_level_coop
    L = 2^15:  width 16: k_bb_merkle_leaves (permute_scaled, renorm_lazy on the capacity, permute_scaled, canonical_out);
               k_bb_merkle_level_coop for every level
-m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B
from plonky2_goldibear_amd import GpuContext, MerkleTree
from plonky2_goldibear_amd import native as N

import permutation_states as PS

pytestmark = pytest.mark.gpu

FIELD_ID = {PS.GL: N.GB_GOLDILOCKS, PS.BB: N.GB_BABYBEAR}
DTYPE = {PS.GL: np.uint64, PS.BB: np.uint32}
REPEATED = 320


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


_inputs, _wanted = {}, {}


def inputs(field):
    if field not in _inputs:
        _inputs[field] = np.array(PS.all_inputs(field), dtype=DTYPE[field])
    return _inputs[field]


def wanted(field):
    """the oracle's permutation of every generated input, once"""
    if field not in _wanted:
        f = O.poseidon if field == PS.GL else B.poseidon2
        _wanted[field] = np.stack([f(st) for st in inputs(field)])
    return _wanted[field]


def describe(field, k):
    ts = PS.targets(field) + PS.zero_capacity_targets(field)
    t = ts[k]
    return "%s state %d: round %d %s %s words %s" % (field, k, t.round, t.where, t.shape, {i: hex(w) for i, w in t.words.items()})


@pytest.mark.parametrize("field", [PS.GL, PS.BB])
def test_permute_as_generated(ctx, field):
    st, want = inputs(field), wanted(field)
    assert st.shape[0] == len(PS.targets(field)) + len(PS.zero_capacity_targets(field)) and st.shape[0] % 64 != 0   # a ragged last wave
    got = ctx.permute(st, field=FIELD_ID[field])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d states differ; first: %s" % (bad.size, describe(field, int(bad[0])))


@pytest.mark.parametrize("field", [PS.GL, PS.BB])
def test_permute_one_state_per_wave(ctx, field):
    st, want = inputs(field), wanted(field)
    pick = np.sort(np.random.default_rng(20261019).choice(st.shape[0], REPEATED, replace=False))
    got = ctx.permute(np.repeat(st[pick], 64, axis=0), field=FIELD_ID[field])
    assert got.shape == (64 * REPEATED, st.shape[1])
    bad = np.flatnonzero((got != np.repeat(want[pick], 64, axis=0)).any(axis=1))
    assert bad.size == 0, "%d lanes differ; first: lane %d of %s" % (bad.size, int(bad[0]) % 64, describe(field, int(pick[bad[0] // 64])))


# ------------------------------------------------------------------ Merkle trees over zero-capacity leaves
def leaves_of(field, L, width):
    """row j: the rate words of zero-capacity state j mod n; at width 16 a seeded second block behind them"""
    zc = np.array([t.input[:8] for t in PS.zero_capacity_targets(field)], dtype=DTYPE[field])
    rows = zc[np.arange(L) % zc.shape[0]]
    if width == 16:
        fill = O.splitmix64_fill(9200 + L, 8 * L) if field == PS.GL else B.fill(9200 + L, 8 * L)
        rows = np.concatenate([rows, fill.reshape(L, 8).astype(DTYPE[field])], axis=1)
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("L", [1024, 1 << 15])
def test_goldilocks_tree_over_zero_capacity_states(ctx, L, width):
    leaves = leaves_of(PS.GL, L, width)
    ref = O.MerkleTree(leaves, 0)
    t = MerkleTree.new(ctx, leaves, 0)
    got, cap = t.digests, t.cap
    t.free()
    assert np.array_equal(cap, ref.cap)
    bad = np.flatnonzero((got != ref.digests).any(axis=1))
    assert got.shape == ref.digests.shape and bad.size == 0, "%d digests differ; first at %d" % (bad.size, int(bad[0]))


@pytest.mark.parametrize("width", [8, 16])
@pytest.mark.parametrize("L", [1024, 1 << 15])
def test_babybear_tree_over_zero_capacity_states(ctx, L, width):
    leaves = leaves_of(PS.BB, L, width)
    levels = PS.levels_of(B, leaves)
    want = PS.reference_layout(levels)
    t = MerkleTree.new(ctx, leaves, 0, field=N.GB_BABYBEAR)
    got, cap = t.digests, t.cap
    t.free()
    assert np.array_equal(cap, levels[-1])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and bad.size == 0, "%d digests differ; first at %d" % (bad.size, int(bad[0]))
