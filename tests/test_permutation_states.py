"""tests/permutation_states.py checked on the CPU: the round-by-round models equal the oracle's permutations (reference KATs, the
states of tests/test_oracle_bb.py and 200 seeded states per field), and every generated input is canonical, reaches its target
exactly at the stated place when run forward, carries the intended device word (value * scale == word), and - for the hash
kernels' states - has a zero capacity."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B

import permutation_states as PS

FIELDS = [PS.GL, PS.BB]


def oracle_permute(field, state):
    if field == PS.GL:
        return [int(x) for x in O.poseidon(np.array(state, dtype=np.uint64))]
    return [int(x) for x in B.poseidon2(np.array(state, dtype=np.uint32))]


def test_goldilocks_model_equals_the_oracle(kats):
    for v in kats["poseidon12"]:
        assert PS.permute(PS.GL, v["input"]) == [int(x) for x in v["output"]]
        assert oracle_permute(PS.GL, v["input"]) == [int(x) for x in v["output"]]
    rnd = O.splitmix64_fill(4100, 12 * 200).reshape(200, 12)
    for st in rnd:
        assert PS.permute(PS.GL, st) == oracle_permute(PS.GL, st)


def test_babybear_model_equals_the_oracle():
    P = PS.BB_P
    for st in ([0] * 16, list(range(16)), [P - 1] * 16, B.fill(3, 16).tolist()):
        assert PS.permute(PS.BB, st) == oracle_permute(PS.BB, st)
    rnd = B.fill(4200, 16 * 200).reshape(200, 16)
    for st in rnd:
        assert PS.permute(PS.BB, st) == oracle_permute(PS.BB, st)


def test_babybear_scales_restate_the_plan():
    """the kappa sequence: round 0's s-box inputs are plain values (Montgomery input, one reduction), every later place follows from
    kappa -> kappa^7 (s-box) and kappa -> kappa / 2^32 (layer); the internal rounds share one scale"""
    P, s = PS.BB_P, PS.bb_scales()
    r_inv = pow(1 << 32, -1, P)
    assert s[(0, PS.SBOX_IN)] == 1
    for r in list(range(3)) + list(range(17, 20)):
        k_in, k_out = s[(r, PS.SBOX_IN)] * r_inv % P, s[(r, PS.MDS_IN)] * r_inv % P       # kappa = scale / R
        assert k_out == pow(k_in, 7, P)
        assert s[(r + 1, PS.SBOX_IN)] == k_out * r_inv % P * (1 << 32) % P
    assert len({s[(r, PS.SBOX_IN)] for r in range(4, 18)}) == 1
    assert s[(4, PS.SBOX_IN)] == s[(3, PS.MDS_IN)] * r_inv % P
    assert s["final"] == s[(20, PS.MDS_IN)] * r_inv % P


@pytest.mark.parametrize("field", FIELDS)
def test_every_target_is_reached(field):
    m = PS.model(field)
    ts = PS.targets(field) + PS.zero_capacity_targets(field)
    assert len(PS.targets(field)) == {PS.GL: 12 * 2 * (90 + 22), PS.BB: 10 * 2 * (63 + 13)}[field]
    assert len(PS.zero_capacity_targets(field)) == {PS.GL: 72, PS.BB: 40}[field]
    n_exact = 0
    for k, t in enumerate(ts):
        assert len(t.input) == m.width and all(0 <= x < m.p for x in t.input), k
        at = PS.forward_to(field, t.input, t.round, t.where)
        scale = m.scale(t.round, t.where)
        for i, w in t.words.items():
            assert at[i] == t.values[i], (k, t.round, t.where, t.shape, i)
            assert at[i] * scale % m.p == w, (k, t.round, t.where, t.shape, i)
            n_exact += t.exact[i]
        if t.shape.startswith("zero_capacity"):
            assert all(x == 0 for x in t.input[8:]) and len(t.words) == 8, k
    # Goldilocks words at or above 2^32 - 1 have one u64 representative; BabyBear's signed / lazy words never do
    assert (n_exact > 0) == (field == PS.GL)
    # every placement, every word of the set at each, and word 0 alone in every partial / internal round
    for r in range(m.rounds):
        for where in (PS.SBOX_IN, PS.MDS_IN):
            here = [t for t in PS.targets(field) if (t.round, t.where) == (r, where)]
            assert {t.shape for t in here} == set(PS.SHAPES) | (set() if m.is_full(r) else {PS.WORD0_ONLY})
            for shape in {t.shape for t in here}:
                firsts = [t.words[min(t.words)] if shape != "one_word" else next(iter(t.words.values())) for t in here if t.shape == shape]
                assert sorted(firsts) == sorted(PS.WORDS[field]), (r, where, shape)


@pytest.mark.parametrize("field", FIELDS)
def test_the_lists_are_fixed(field):
    a = [t.input for t in PS.targets(field)]
    PS.targets.cache_clear()
    assert a == [t.input for t in PS.targets(field)]
    assert len(PS.all_inputs(field)) == len(PS.targets(field)) + len(PS.zero_capacity_targets(field))


def test_pull_back_inverts_forward_on_random_states():
    for field in FIELDS:
        m = PS.model(field)
        rnd = O.splitmix64_fill(4300, 64 * m.width).reshape(64, m.width)
        for k, st in enumerate(rnd):
            st = [int(x) % m.p for x in st]
            r, where = k % m.rounds, (PS.SBOX_IN, PS.MDS_IN)[k // m.rounds % 2]
            assert PS.back_to_input(field, PS.forward_to(field, st, r, where), r, where) == st


def test_reference_layout_is_the_oracles():
    leaves = O.splitmix64_fill(9100, 64 * 9).reshape(64, 9)
    assert np.array_equal(PS.reference_layout(PS.levels_of(O, leaves)), O.MerkleTree(leaves, 0).digests)
