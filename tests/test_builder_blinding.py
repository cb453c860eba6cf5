"""CircuitBuilder.blind in the builder mirror (plonk/circuit_builder.rs:875-980), without a GPU:
  * blinding_counts is a fixpoint of the reference's loop - the counts fit the power of two they were computed for and the next
    smaller one does not hold the gates with ITS counts - in both fields under a stock config, the small num_query_rounds = 2
    config (tests/zk_circuits.py) and a config whose first estimate has to double;
  * structure: a power of two of rows; exactly regular * num_wires + z * num_routed new random-value targets, in creation order
    (row by row, wire by wire; a pair's first row only); z * num_routed new copies, each between equal columns of adjacent
    rows.  As in the reference the copies are CopyGenerators (generate_copy), not copy constraints: the sigma columns of the
    blinding rows are the identity, which the test states;
  * a zero_knowledge = False build of the factorial circuit is what it was: the constants_sigmas bytes of a config object that
    has never heard of the field;
  * the oracle prover takes the blinded factorial circuit's gate set: its salted proof of the blinded witness, with the salts of
    a seed (tests/random_stream.py), is accepted by the oracle verifier and by gb_verify on the host."""
import hashlib

import numpy as np
import pytest

import circuits as CS
import random_stream as RS
import zk_circuits as Z
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import VerifierCircuitData
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import (CircuitBuilder, CircuitConfig, NoopGate, _CopyGenerator, _RandomValueGenerator,
                                                   wire)

FIELDS = {"goldilocks": N.GB_GOLDILOCKS, "babybear": N.GB_BABYBEAR}
SEED = bytes((13 * i + 7) & 0xFF for i in range(32))


def reference_counts(b, num_gates):
    """circuit_builder.rs:879-922 written out again, on the builder's own fri list -> (regular, z, degree)"""
    D_ = b.F.ext_degree
    degree = 1
    while degree < num_gates:
        degree *= 2
    while True:
        arities = [1 << x for x in b.fri_reduction_arity_bits(degree.bit_length() - 1)]
        final = degree
        for a in arities:
            final //= a
        fri = b.config.num_query_rounds * (1 + D_ * sum(a - 1 for a in arities) + D_ * final)
        regular, z = D_ + fri, 2 * D_ + fri
        if num_gates + regular + 2 * z <= degree:
            return regular, z, degree
        degree *= 2


def with_gates(cfg, num_gates):
    b = CircuitBuilder(cfg)
    for _ in range(num_gates):
        b.add_gate(NoopGate())
    return b


CONFIGS = {
    "stock": lambda f: Z.config(f),
    "small": lambda f: Z.small_config(f),
    # 100 gates: the first estimate, 2^7, cannot even hold the rows of one query round
    "doubling": lambda f: Z.config(f, num_query_rounds=4, security_bits=25),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_blinding_counts_are_a_fixpoint(field, name):
    b = with_gates(CONFIGS[name](FIELDS[field]), 100)
    regular, z = b.blinding_counts()
    want_regular, want_z, degree = reference_counts(b, 100)
    assert (regular, z) == (want_regular, want_z)
    assert (regular, z) == b.num_blinding_gates(degree) and 100 + regular + 2 * z <= degree
    assert degree > 128, "the first estimate has to double"
    r2, z2 = b.num_blinding_gates(degree // 2)
    assert 100 + r2 + 2 * z2 > degree // 2                      # the next smaller power of two does not fit
    assert z == regular + b.F.ext_degree
    if name == "stock":
        assert degree >= 1 << 14
    if name == "small":
        assert 1 << 7 <= degree <= 1 << 9


def test_the_stock_goldilocks_numbers():
    """28 queries, arities 16 16 16 at 2^14 rows, 4 final coefficients: 28 (1 + 2 * 45 + 2 * 4) = 2772 values per opening"""
    b = with_gates(CircuitConfig.standard_recursion_zk_config_gl(), 100)
    assert b.config.zero_knowledge and b.blinding_counts() == (2774, 2776)
    assert CircuitConfig.standard_recursion_zk_config_bb().zero_knowledge and CircuitConfig.standard_recursion_zk_config_bb().num_wires == 167
    assert not CircuitConfig.standard_recursion_config_gl().zero_knowledge


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_structure_of_the_blinded_circuit(field):
    tag = FIELDS[field]
    b, _ = Z.factorial(Z.small_config(tag))
    plain_b, _ = Z.factorial(Z.small_config(tag, zero_knowledge=False))
    c, plain = b.build(), plain_b.build()
    cfg = c.config
    nw, nr = cfg.num_wires, cfg.num_routed_wires
    n = 1 << c.degree_bits
    assert n & (n - 1) == 0 and c.degree_bits == (8 if field == "goldilocks" else 9)
    # the rows: the unblinded circuit's gates (before its padding), then `regular` rows, then `z` pairs, then padding - all NoopGate
    noop = c.gate_ids.index("NoopGate")
    first = next(r for r in range(n) if all(g == noop for g in c.row_gates[r:]))
    regular, z, degree = reference_counts(b, first)
    assert degree == n and first + regular + 2 * z <= n
    assert [plain.gate_ids[g] for g in plain.row_gates[:first]] == [c.gate_ids[g] for g in c.row_gates[:first]]
    # the random-value targets: what the unblinded circuit has (the PublicInputGate's wires), then the blinding cells in creation order
    want = [wire(first + r, w) for r in range(regular) for w in range(nw)]
    want += [wire(first + regular + 2 * k, w) for k in range(z) for w in range(nr)]
    assert len(want) == regular * nw + z * nr
    assert c.random_targets == plain.random_targets + want
    assert c.blinding_targets == want
    # the copies: one per routed wire of every pair, from the first row to the same column of the second
    copies = [(g.src, g.dst) for g in c.generators if isinstance(g, _CopyGenerator)]
    old = [(g.src, g.dst) for g in plain.generators if isinstance(g, _CopyGenerator)]
    new = copies[len(old):]
    assert copies[:len(old)] == old and len(new) == z * nr
    assert new == [(wire(first + regular + 2 * k, w), wire(first + regular + 2 * k + 1, w)) for k in range(z) for w in range(nr)]
    assert all(s[2] == d[2] and d[1] == s[1] + 1 for s, d in new)
    # ... which are generators, as in the reference (generate_copy): no copy constraint, the blinding rows' sigmas are the identity
    assert len(b.copy_constraints) == len(plain_b.copy_constraints)
    sigma = c.constants_sigmas[c.num_selectors + c.max_constants:]
    subgroup = b.F._powers(b.F.two_adic_generator(c.degree_bits), n)
    for col in (0, nr - 1):
        ident = b.F._mul(subgroup, c.k_is[col])
        assert (sigma[col, first:first + regular + 2 * z] == ident[first:first + regular + 2 * z]).all()
    # the witness: the blinding cells hold values, a pair's rows agree, everything else in those rows is zero
    _, pw = Z.factorial(Z.small_config(tag))
    w, pis = c.generate_witness(pw, np.random.default_rng(5))
    zrows = first + regular
    assert (w[:, first:zrows] != 0).mean() > 0.99
    assert (w[:nr, zrows:zrows + 2 * z:2] == w[:nr, zrows + 1:zrows + 2 * z:2]).all() and (w[:nr, zrows:zrows + 2 * z] != 0).mean() > 0.99
    assert not w[nr:, zrows:zrows + 2 * z].any() and not w[:, zrows + 2 * z:].any()
    assert pis[1] == int(np.prod([i for i in range(2, 22)], dtype=object)) % b.F.p


def test_a_build_without_zero_knowledge_is_unchanged():
    """the factorial circuit of tests/circuits.py: under a config with zero_knowledge = False, and under a config object without the
    attribute at all (what a caller's pickled or hand-made config looks like), build() gives the same bytes"""
    b, _ = CS.factorial_circuit(count=60)
    c = b.build()
    b2, _ = CS.factorial_circuit(count=60)
    del b2.config.__dict__["zero_knowledge"]
    c2 = b2.build()
    assert c.constants_sigmas.tobytes() == c2.constants_sigmas.tobytes() and c.degree_bits == c2.degree_bits == 6
    assert not c.blinding_targets and len(c.random_targets) == c.config.num_wires - 4
    # pinned: sha256 of the bytes as the parent commit built them
    assert hashlib.sha256(c.constants_sigmas.tobytes()).hexdigest() == FACTORIAL_60_SHA256


FACTORIAL_60_SHA256 = "92735bf3d73bc8fb3f4f12d3fd15974b6f46b36f51bdec4945809f832a90b2ad"


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_oracle_prover_and_host_verifier_take_the_blinded_circuit(field):
    tag = FIELDS[field]
    F = GL if tag == N.GB_GOLDILOCKS else BB
    b, pw = Z.factorial(Z.small_config(tag))
    c = b.build()
    w, pis = c.generate_witness(pw, np.random.default_rng(3))
    oc = CS.oracle_circuit(c, len(pis))
    oc.zero_knowledge = True
    salts = RS.salts(SEED, F, (1 << c.degree_bits) << c.config.rate_bits)
    proof = D.prove_cpu(oc, w, pis, salts=salts)[0]
    assert D.verify(oc, proof)
    cfg = c.config
    v = VerifierCircuitData(c.degree_bits, c.gate_table, c.k_is, oc.constants_sigmas_cap, oc.circuit_digest, num_wires=cfg.num_wires,
                            num_routed_wires=cfg.num_routed_wires, num_constants=c.max_constants, num_challenges=cfg.num_challenges,
                            arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits, num_query_rounds=cfg.num_query_rounds,
                            num_selectors=c.num_selectors, zero_knowledge=True, field=tag, num_public_inputs=len(pis))
    assert v.verify(proof)
