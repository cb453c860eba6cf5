"""tests/wired_circuits.py pinned to the CPU oracle (no GPU): the wired dummy circuit with its carry-edge witness is proved by the
oracle prover and accepted by the oracle verifier, the integer restatement of the permutation argument equals the oracle
prover's own Z / partial-product values at the transcript's challenges, the wiring is not trivial (Z moves), and a broken copy
constraint is caught."""
import functools

import numpy as np
import pytest

from oracle import plonk_dummy as D
from oracle.fields import BB, GL
import wired_circuits as W

CASES = [("goldilocks", 6), ("goldilocks", 10), ("babybear", 6), ("babybear", 10)]


def config(F):
    return D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)


@functools.lru_cache(maxsize=None)
def _proved(field_name, degree_bits):
    F = GL if field_name == "goldilocks" else BB
    circ, w, _ = W.wired_dummy_circuit(F, config(F), degree_bits, seed=100 + degree_bits, dense="edges")
    dump = {}
    proof, dbg = D.prove_cpu(circ, w, dump=dump)
    return F, circ, w, proof, dbg, dump


def test_edge_values_are_canonical_and_distinct():
    for F, count in ((GL, 15), (BB, 14)):
        ev = W.edge_values(F)
        assert len(ev) == len(set(ev)) == count and all(0 <= v < F.P for v in ev)
    assert [v * 2**32 % BB.P for v in W.edge_values(BB)[9:]] == W.bb_edge_words() == [1, 2, 2**27, BB.P - 2, BB.P - 1]


@pytest.mark.parametrize("field_name,degree_bits", CASES)
def test_copy_classes_are_a_permutation_that_the_witness_respects(field_name, degree_bits):
    F, circ, w, _, _, _ = _proved(field_name, degree_bits)
    n, nr, p = circ.n, circ.cfg.num_routed_wires, F.P
    ident = {int(circ.k_is[j]) * int(circ.subgroup[r]) % p: (j, r) for j in range(nr) for r in range(n)}
    assert len(ident) == nr * n
    sig = circ.sigma
    images = {ident[int(sig[j, r])] for j in range(nr) for r in range(n)}
    assert len(images) == nr * n                                                 # sigma is a permutation of the routed cells
    moved = 0
    for j in range(nr):
        for r in range(n):
            j2, r2 = ident[int(sig[j, r])]
            assert w[j, r] == w[j2, r2]                                          # the witness is constant on every cycle
            moved += (j2, r2) != (j, r)
    assert moved >= nr * n // 2                                                  # sizes 1..5, uniform: 1/15 of the cells are fixed points
    cells, starts, sizes = circ.copy_classes
    assert sizes.min() == 1 and sizes.max() == 5
    ev = set(W.edge_values(F))
    noop = [r for r in range(n) if r not in (circ.pi_row, circ.const_row)]
    assert {int(v) for v in w[:, noop].ravel()} == ev                            # every edge value occurs, nothing else does


@pytest.mark.parametrize("field_name,degree_bits", CASES)
def test_oracle_proves_and_verifies_and_the_integer_reference_equals_its_dump(field_name, degree_bits):
    F, circ, w, proof, dbg, dump = _proved(field_name, degree_bits)
    assert D.verify(circ, proof)
    c = circ.cfg.num_challenges
    betas, gammas = [int(x) for x in dbg[:c]], [int(x) for x in dbg[c:2 * c]]
    ref, census = W.zs_partial_products_ref(F, w, circ.sigma, circ.k_is, betas, gammas, degree_bits, circ.cfg.max_quotient_degree_factor)
    assert ref.shape == dump["zs_partial_products"].shape and np.array_equal(ref, dump["zs_partial_products"])
    assert sum(census.values()) == c * circ.cfg.num_routed_wires * circ.n
    # the wiring is not trivial: Z moves (on the dummy circuit it is 1 on all but two rows)
    zs = dump["zs_partial_products"][:c]
    assert (zs[:, 0] == 1).all()
    assert (zs != 1).sum(axis=1).min() >= circ.n // 4


def test_reference_raises_on_a_denominator_that_vanishes_through_the_wrap():
    F, circ, w, _, _, _ = _proved("goldilocks", 6)
    assert (w[:circ.cfg.num_routed_wires] == F.P - 1).any()
    with pytest.raises(ZeroDivisionError):
        W.zs_partial_products_ref(F, w, circ.sigma, circ.k_is, [0, 1], [1, 1], 6, 8)


def test_census_sees_each_kind_of_sum():
    w = np.array([[1, GL.P - 1, 2**63, (GL.P + 1) // 2]], dtype=np.uint64)
    sigma, k_is = np.array([[5, 6, 7, 8]], dtype=np.uint64), [1]
    _, census = W.zs_partial_products_ref(GL, w, sigma, k_is, [1, 1], [1, 2**63], 2, 8)
    # + 1: 2, p, 2^63 + 1, (p + 3) / 2;  + 2^63: 2^63 + 1, p - 1 + 2^63 > 2^64, 2^64, 2^64 - 2^31 + 1 in (p, 2^64)
    assert census == dict(below_p=4, equal_p=1, between=1, equal_top=1, above_top=1)
    wb = np.array([[0, 1, BB.P - 1, 2]], dtype=np.uint32)
    _, census = W.zs_partial_products_ref(BB, wb, sigma.astype(np.uint32), k_is, [1], [BB.P - 1], 2, 8)
    words = [(v << 32) % BB.P + ((BB.P - 1) << 32) % BB.P for v in (0, 1, BB.P - 1, 2)]
    assert census == dict(below_p=sum(s < BB.P for s in words), equal_p=sum(s == BB.P for s in words),
                          between=sum(s > BB.P for s in words), equal_top=0, above_top=0)
    assert census["equal_p"] == 1 and census["below_p"] >= 1 and census["between"] >= 1


def test_a_broken_copy_constraint_does_not_verify():
    """The oracle PROVER has no check of its own on the identity vanishing(zeta) = Z_H(zeta) * quotient(zeta) (it returns bytes for
    any witness whose denominators are nonzero); the oracle VERIFIER's check of it is what refuses the proof."""
    F, circ, w, _, _, _ = _proved("goldilocks", 6)
    col, row = W.class_member(circ, 2)
    assert col < circ.cfg.num_routed_wires and row not in (circ.pi_row, circ.const_row)
    bad = W.break_copy_constraint(circ, w)
    assert (bad != w).sum() == 1
    proof, _ = D.prove_cpu(circ, bad)
    with pytest.raises(AssertionError, match=r"vanishing\(zeta\) != Z_H\(zeta\) \* quotient\(zeta\)"):
        D.verify(circ, proof)
