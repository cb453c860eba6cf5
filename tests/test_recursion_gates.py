"""Host mirror of the recursion gate set (plonky2_goldibear_amd/recursion_gates.py) against the oracle's evaluators, which the
reference's regression proof pins (tests/test_oracle_fixture.py): on a generated witness every constraint of every row
evaluates to zero (the reference's generator <-> eval_unfiltered contract), a perturbed wire breaks its gate, and the gate
ids / sort order / selector groups of a recursion-shaped gate set come out as in the reference's fixture.  No GPU."""
import numpy as np
import pytest

from oracle import gates as G
from oracle import verifier as V
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N

from circuits import recursion_gates_circuit


def _row_constraints(c, F, wires, row):
    sel = c.num_selectors
    consts = [F.efrom(int(c.constants_sigmas[sel + i, row])) for i in range(c.max_constants)]
    w = [F.efrom(int(v)) for v in wires[:, row]]
    sel_vals = [int(c.constants_sigmas[i, row]) for i in range(sel)]
    out = {}
    for gi, g in enumerate(c.gate_table):
        if g[0] in (G.NOOP, G.PUBLIC_INPUT) or sel_vals[g[2]] != gi:
            continue
        out[gi] = G.eval_unfiltered(F, g, w, consts, None)
    return out


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_generated_witness_satisfies_every_gate(field):
    F = GL if field == N.GB_GOLDILOCKS else BB
    b, pw, rows = recursion_gates_circuit(field)
    c = b.build()
    wires, pis = c.generate_witness(pw)
    kinds = {g[0] for g in c.gate_table}
    want = {G.ARITHMETIC_EXTENSION, G.MUL_EXTENSION, G.BASE_SUM, G.REDUCING, G.REDUCING_EXTENSION, G.RANDOM_ACCESS,
            G.COSET_INTERPOLATION, G.EXPONENTIATION, G.ADD_MANY, G.APPLY_MAT4} | (
        {G.POSEIDON_MDS} if F is GL else {G.POSEIDON2_INTERNAL_PERMUTATION})
    assert want <= kinds
    seen = set()
    for row in range(1 << c.degree_bits):
        for gi, cons in _row_constraints(c, F, wires, row).items():
            g = c.gate_table[gi]
            assert len(cons) == G.num_constraints(g, F.hout, F.D), c.gate_ids[gi]
            assert all(x == F.zero for x in cons), "%s row %d" % (c.gate_ids[gi], row)
            seen.add(g[0])
    assert want <= seen
    # a perturbed dependent wire breaks exactly its own row's gate
    for name, row in rows.items():
        gate = b.gate_instances[row][0]
        col = gate.num_wires - 1
        bad = wires.copy()
        bad[col, row] = (int(bad[col, row]) + 1) % F.P
        cons = _row_constraints(c, F, bad, row)
        assert any(x != F.zero for v in cons.values() for x in v), name


def test_gate_order_and_selector_groups_match_the_reference_fixture(golden_dir):
    """The fixture's CommonCircuitData lists its gates sorted by (degree, id) with selectors_info; a builder holding the same
    gate structs must produce the same order and groups (circuit_builder.rs:1194-1196, gates/selectors.rs:125-209)."""
    import os
    from plonky2_goldibear_amd import recursion_gates as R
    from plonky2_goldibear_amd.circuit_builder import (ArithmeticGate, CircuitConfig, NoopGate, PoseidonGate, PublicInputGate,
                                                       selector_polynomials)
    common = open(os.path.join(golden_dir, "recursive_verifier_gl_common_data.bin"), "rb").read()
    cd = V.read_common_data(common)
    ref = V.read_gates(common, cd)
    cfg = CircuitConfig.standard_recursion_config_gl()
    mine = [NoopGate(), PoseidonGate(), PublicInputGate(4), ArithmeticGate.new_from_config(cfg), R.PoseidonMdsGate(),
            R.BaseSumGate(63, 2), R.ReducingExtensionGate(32), R.ReducingGate(43), R.ArithmeticExtensionGate.new_from_config(cfg),
            R.MulExtensionGate.new_from_config(cfg), R.RandomAccessGate.new_from_config(cfg, 4),
            R.CosetInterpolationGate(4, max_degree=6)]
    gates = sorted(mine, key=lambda g: (g.degree, g.id))
    _, sel, groups = selector_polynomials(gates, [(gates[0], [])], cfg.max_quotient_degree_factor + 1, GL.P)
    got = [(g.kind, g.param, sel[i], groups[sel[i]][0], groups[sel[i]][1], getattr(g, "param2", 0), getattr(g, "param3", 0))
           for i, g in enumerate(gates)]
    assert got == ref
    assert cd["num_gate_constraints"] == max(g.num_constraints for g in gates)
    # the interpolation gate's weights are the serialized ones
    ci = next(g for g in gates if g.kind == G.COSET_INTERPOLATION)
    assert ci.barycentric_weights == G.barycentric_weights(GL, 4)[1]
    assert (ci.degree, ci.num_intermediates) == (6, 2)


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_oracle_prover_evaluates_the_recursion_gates_on_the_coset(field):
    """The CPU oracle prover with the gate terms of oracle/plonk_dummy.gate_constraint_terms (every gate of the recursion set at
    every LDE point, evaluators of oracle/gates.py): its proof satisfies the vanishing identity under the pinned verifier, and a
    witness that breaks one gate row does not - the oracle side of tests/test_gpu_recursion_gates.py, runnable without a GPU."""
    from oracle import plonk_dummy as PD
    from circuits import oracle_circuit, recursion_gates_circuit
    b, pw, rows = recursion_gates_circuit(field, seed=11)
    c = b.build(None)
    w, pis = c.generate_witness(pw)
    oc = oracle_circuit(c, len(pis))
    terms = PD.gate_constraint_terms(oc, w, pis)
    n, r = 1 << c.degree_bits, oc.cfg.rate_bits
    assert terms.shape[0] == n << r and terms.any()       # off the subgroup the constraint polynomials do not vanish
    proof, _ = PD.prove_cpu(oc, w, pis)
    assert PD.verify(oc, proof)
    row = rows["coset_interpolation"]
    gate = b.gate_instances[row][0]
    bad = w.copy()
    bad[gate.num_wires - 1, row] = (int(bad[gate.num_wires - 1, row]) + 1) % oc.F.P
    with pytest.raises(AssertionError, match="vanishing"):
        PD.verify(oc, PD.prove_cpu(oc, bad, pis)[0])


# ---- every parameter gb_circuit_create_gates accepts: tests/gate_variants.py
VARIANT_CIRCUITS = ["random_access", "interpolation", "rest0", "rest1", "rest2"]


def host_verifier(c, oc):
    """the product's host verifier (gb_verifier_create: no device) for a built circuit and its oracle twin"""
    from plonky2_goldibear_amd.prover import VerifierCircuitData
    cfg = c.config
    digest = oc.circuit_digest      # commits constants||sigmas on the CPU: the cap comes with it
    return VerifierCircuitData(c.degree_bits, c.gate_table, c.k_is, oc.constants_sigmas_cap, digest, num_wires=cfg.num_wires,
                               num_routed_wires=cfg.num_routed_wires, num_constants=c.max_constants, num_challenges=cfg.num_challenges,
                               max_quotient_degree_factor=cfg.max_quotient_degree_factor, rate_bits=cfg.rate_bits,
                               cap_height=cfg.cap_height, proof_of_work_bits=cfg.proof_of_work_bits,
                               num_query_rounds=cfg.num_query_rounds, arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits,
                               num_selectors=c.num_selectors, field=cfg.field, num_public_inputs=len(c.public_inputs))


def test_variant_circuits_hold_every_buildable_variant_once():
    import gate_variants as GV
    for field in GV.FIELDS:
        cfg, sets = GV.config(field), GV.variant_sets(field)
        assert list(sets) == VARIANT_CIRCUITS
        held = [g for s in sets.values() for g in s]
        assert sorted(held) == sorted(g for g in GV.grid(field) if GV.buildable(cfg, g)) and len(set(held)) == len(held)
        ra = sorted({g[1] for g in sets["random_access"]})
        assert ra == list(range(7 if field == N.GB_GOLDILOCKS else 6))            # bits limited by the routed wires
        ci = {(g[1], g[5]) for g in sets["interpolation"]}
        want = {(bits, d) for bits in range(1, 5) for d in GV.interpolation_degrees(bits)
                if d <= cfg.max_quotient_degree_factor and GV.gate_object(field, (G.COSET_INTERPOLATION, bits, 0, 0, 1, d, 0)).num_wires <= cfg.num_wires}
        assert ci == want and {b for b, _ in ci} == {1, 2, 3, 4}
        assert len(held) == {N.GB_GOLDILOCKS: 79, N.GB_BABYBEAR: 74}[field]


@pytest.mark.parametrize("name", VARIANT_CIRCUITS)
@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_gate_variants_through_the_builder_the_oracle_prover_and_the_host_verifier(field, name):
    """One row of every buildable parameterisation (tests/gate_variants.py): the generated witness makes every oracle constraint
    zero, a perturbed last wire breaks its own gate, the oracle prover's proof is accepted by the oracle verifier and by the
    product's host verifier (csrc/gates.hpp over the extension algebra), and a proof of a perturbed witness is refused with
    "vanishing" by both."""
    import gate_variants as GV
    from oracle import plonk_dummy as PD
    from plonky2_goldibear_amd import VerifyError
    from circuits import oracle_circuit
    F = GL if field == N.GB_GOLDILOCKS else BB
    b, pw, rows = GV.variant_circuit(field, name, seed=5)
    c = b.build(None)
    assert c.degree_bits <= 5 and len(c.gate_table) <= GV.MAX_GATES
    wires, pis = c.generate_witness(pw)
    assert {gi for row in rows.values() for gi in _row_constraints(c, F, wires, row)} >= \
        {c.gate_ids.index(b.gate_instances[row][0].id) for row in rows.values()}
    for row in range(1 << c.degree_bits):
        for gi, cons in _row_constraints(c, F, wires, row).items():
            assert len(cons) == G.num_constraints(c.gate_table[gi], F.hout, F.D), c.gate_ids[gi]
            assert all(x == F.zero for x in cons), "%s row %d" % (c.gate_ids[gi], row)
    for vname, row in rows.items():
        gate = b.gate_instances[row][0]
        bad = wires.copy()
        bad[gate.num_wires - 1, row] = (int(bad[gate.num_wires - 1, row]) + 1) % F.P
        cons = _row_constraints(c, F, bad, row)
        assert list(cons) == [c.gate_ids.index(gate.id)] and any(x != F.zero for x in cons[list(cons)[0]]), vname
    oc = oracle_circuit(c, len(pis))
    ver = host_verifier(c, oc)
    proof, _ = PD.prove_cpu(oc, wires, pis)
    assert PD.verify(oc, proof)
    assert ver.verify(proof)
    # the last variant row of the circuit, perturbed: the identity fails under both verifiers
    vname, row = list(rows.items())[-1]
    gate = b.gate_instances[row][0]
    bad = wires.copy()
    bad[gate.num_wires - 1, row] = (int(bad[gate.num_wires - 1, row]) + 1) % F.P
    bad_proof = PD.prove_cpu(oc, bad, pis)[0]
    with pytest.raises(AssertionError, match="vanishing"):
        PD.verify(oc, bad_proof)
    with pytest.raises(VerifyError, match="vanishing"):
        ver.verify(bad_proof)
    ver.free()


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_what_the_verifier_create_accepts_and_refuses(field):
    """build_gate_set (csrc/prover_host.inc) through gb_verifier_create, which needs no device: a CosetInterpolationGate is
    accepted exactly at subgroup_bits <= 4 with a degree with_max_degree() yields (computed in tests/gate_variants.py), a
    RandomAccessGate at bits <= 6 with at least one copy, a BaseSumGate up to base max_quotient_degree_factor, and every gate
    only when its wires fit the configuration."""
    import gate_variants as GV
    from plonky2_goldibear_amd.prover import VerifierCircuitData
    F, cfg = GV.FIELDS[field], GV.config(field)

    def create(gates):
        return VerifierCircuitData(3, gates, np.ones(cfg.num_routed_wires, dtype=F.dtype), np.zeros((16, F.hout), dtype=F.dtype),
                                   np.zeros(F.hout, dtype=F.dtype), num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires,
                                   num_challenges=cfg.num_challenges, arity_bits=cfg.arity_bits, field=field)

    seen = GV.check_acceptance(field, create)
    assert seen["ok"] >= 25 and seen["refused"] >= 50 and seen["needs"] >= 5, seen
