"""The cooperative Poseidon-12 kernels (csrc/poseidon_gl_coop.hpp: one state per 16-lane row, thirty rounds of one shape) through
the product's doors, against the CPU oracle, bit for bit.  Every tree of at most 2^14 leaves runs all its levels in
k_gl_merkle_level_coop and its sponges in k_gl_merkle_leaves_coop / k_gl_fri_leaves_coop, so the shapes are small.

  * two_to_one on chosen words: leaves of width 4 are not hashed (hash_or_noop), their words ARE the inputs of the first level's
    two_to_one.  Words from {0, 1, 2^32 - 1, 2^32, 2^32 + 1, p - 1, p - 2^32, 2^63, seeded}: sibling leaves that are all one such
    word (a node with p - 1 in all eight input words among them), leaves that mix them per word, seeded leaves.  Every digest of
    every level and the cap.
  * leaf sponges at widths 5, 8, 9, 16, 17, 135: ragged, exact and chained absorptions, the capacity carried across permutations.
  * FRI-shaped leaves: prove() with FriReductionStrategy::Fixed lists [1], [3], [4] at sizes whose first FRI tree has 2^5 leaves;
    the proof bytes - FRI caps, the opened leaves and their paths among them - equal the CPU oracle prover's.  (A leaf of
    arity 2 is four words and is not hashed: that case reaches the level kernel only.)
  * the reference's first Poseidon known answer (all-zero state) as a width-8 leaf of zeros: one absorption into a zero capacity
    is one permutation of that state.  The other three known answers start from a non-zero capacity, which no door of the product
    hands to these kernels directly; tests/test_device_permutation_states.py drives full states through
    poseidon_gl_coop::permute, and tests/test_device_headers_on_host.py checks the thirty-round form against the fast form.
-m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import plonk_dummy as D
from oracle.fields import GL
from plonky2_goldibear_amd import CircuitData, GpuContext, MerkleTree, fri_params as FP, native as N

pytestmark = pytest.mark.gpu

P = O.GL_P
WORDS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P - (1 << 32), 1 << 63]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def chosen_leaves(L, width, seed):
    """[L][width]: rows 2i, 2i + 1 (i < 8) are all WORDS[i] - siblings, so a width-4 node sees one word eight times -, the next
    eight rows mix the words (row r, word j: WORDS[(r + 3 j) % 8]), then seeded rows alternate with seeded rows in which every
    other word is a chosen one."""
    leaves = O.splitmix64_fill(seed, L * width).reshape(L, width)
    for i, w in enumerate(WORDS):
        leaves[2 * i] = leaves[2 * i + 1] = w
    for r in range(16, 24):
        leaves[r] = [WORDS[(r + 3 * j) % 8] for j in range(width)]
    for r in range(25, L, 2):
        leaves[r, ::2] = [WORDS[(r + j) % 8] for j in range(len(leaves[r, ::2]))]
    assert int(leaves.max()) < P
    return leaves


def check_tree(ctx, leaves, cap_height):
    ref = O.MerkleTree(leaves, cap_height)
    t = MerkleTree.new(ctx, leaves, cap_height)
    try:
        assert np.array_equal(t.cap, ref.cap)
        got = t.digests
        assert got.shape == ref.digests.shape and np.array_equal(got, ref.digests)   # every digest of every level below the cap
    finally:
        t.free()


@pytest.mark.parametrize("cap_height", [0, 4])
@pytest.mark.parametrize("log_leaves", [5, 6, 9])
def test_two_to_one_on_chosen_words(ctx, log_leaves, cap_height):
    leaves = chosen_leaves(1 << log_leaves, 4, 9100 + log_leaves)
    assert (leaves[10:12] == P - 1).all()            # node 5 of the first level: p - 1 in all eight input words
    check_tree(ctx, leaves, cap_height)


@pytest.mark.parametrize("width", [5, 8, 9, 16, 17, 135])
def test_leaf_sponges_on_chosen_words(ctx, width):
    leaves = chosen_leaves(64, width, 9200 + width)
    want = np.stack([O.hash_no_pad(r) for r in leaves])
    t = MerkleTree.new(ctx, leaves, 6)               # cap = the leaf digests themselves
    try:
        assert np.array_equal(t.cap, want)
    finally:
        t.free()
    check_tree(ctx, leaves, 0)


@pytest.mark.parametrize("degree_bits,arity_bits", [(3, 1), (5, 3), (6, 4)])
def test_fri_shaped_leaves(ctx, degree_bits, arity_bits):
    cfg = D.CircuitConfig(num_challenges=2, proof_of_work_bits=4, num_query_rounds=8)
    assert (degree_bits + cfg.rate_bits) - arity_bits == 5          # leaves of the first FRI tree
    bits = FP.reduction_arity_bits(("fixed", [arity_bits]), degree_bits, cfg.rate_bits, cfg.cap_height, cfg.num_query_rounds)
    assert list(bits) == [arity_bits]
    circ = D.DummyCircuit(degree_bits, cfg, F=GL)
    circ.reduction_arity_bits = list(bits)
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                      num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                      arity_bits=cfg.arity_bits, proof_of_work_bits=cfg.proof_of_work_bits, num_query_rounds=cfg.num_query_rounds,
                      gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI, field=N.GB_GOLDILOCKS, reduction_arity_bits=bits)
    try:
        circ.set_cap(gpu.constants_sigmas_cap)
        w = circ.witness(seed=40 + degree_bits)
        got = gpu.prove(w)
        assert got == D.prove_cpu(circ, w)[0]
        assert D.verify(circ, got)
    finally:
        gpu.free()


def test_known_answer_through_a_leaf_of_zeros(ctx, kats):
    kat = kats["poseidon12"][0]
    assert not any(kat["input"])
    leaves = np.zeros((8, 8), dtype=np.uint64)
    t = MerkleTree.new(ctx, leaves, 3)
    try:
        assert np.array_equal(t.cap, np.tile(np.array(kat["output"][:4], dtype=np.uint64), (8, 1)))
    finally:
        t.free()
