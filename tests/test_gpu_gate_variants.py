"""GPU prove() of circuits that hold one row of every gate parameterisation gb_circuit_create_gates accepts and the builder can
place (tests/gate_variants.py variant_circuits): RandomAccessGate at bits 0..6, CosetInterpolationGate at every subgroup size and
degree, BaseSumGate at bases 2..8, one-coefficient ReducingGates, one-bit ExponentiationGates and so on - where
tests/test_gpu_recursion_gates.py runs one parameterisation per gate.  Each circuit is a gate set the host-balanced plan of
k_gate_constraints_tiled has not seen.

Per circuit: the proof equals the CPU oracle prover's byte for byte (its gate terms come from oracle/gates.py on the whole
coset), the quotient chunk coefficients equal the oracle's dump, gb_verify and the oracle verifier accept, and one perturbed row
per gate kind is refused by both.  The interpolation circuits run once more at 5 (Goldilocks) and 11 (BabyBear) challenges:
the gate kernels' sliced launches with their t0 / nterms offsets; the BabyBear random-access circuit (arithmetic plus small
gates) once more at 7 challenges, where the tiled kernel's partial sums need more LDS columns than the staged wires (area > nw).
-m gpu only."""
import pytest

from oracle import plonk_dummy as PD
from plonky2_goldibear_amd import GpuContext, VerifyError
from plonky2_goldibear_amd import native as N

import gate_variants as GV
from circuits import oracle_circuit

pytestmark = pytest.mark.gpu

VARIANT_CIRCUITS = ["random_access", "interpolation", "rest0", "rest1", "rest2"]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def check_circuit(ctx, field, name, stages, perturb, **cfg_kw):
    b, pw, rows = GV.variant_circuit(field, name, seed=9, **cfg_kw)
    c = b.build(ctx)
    assert c.degree_bits <= 5 and len(c.gate_table) <= GV.MAX_GATES
    w, pis = c.generate_witness(pw)
    proof = c.data.prove(w, pis)
    oc = oracle_circuit(c, len(pis))
    assert (c.data.circuit_digest == oc.circuit_digest).all()
    oc.set_cap(c.data.constants_sigmas_cap)
    dump, mid = {}, {}
    want, _ = PD.prove_cpu(oc, w, pis, dump=dump)
    assert proof == want
    if stages:
        from test_gpu_stage_abi import prove_by_stages
        assert prove_by_stages(c.data, oc, w, pis, field, mid) == want
        assert (mid["zs_partial_products"] == dump["zs_partial_products"]).all()
        assert (mid["quotient_chunks"] == dump["quotient_chunks"]).all()
    assert c.data.verify(proof)
    assert PD.verify(oc, proof)
    # one perturbed row per gate kind: the proof fails the identity under both verifiers
    p = GV.FIELDS[field].P
    seen = set()
    for vname, row in rows.items() if perturb else ():
        gate = b.gate_instances[row][0]
        if gate.kind in seen:
            continue
        seen.add(gate.kind)
        bad = w.copy()
        bad[gate.num_wires - 1, row] = (int(bad[gate.num_wires - 1, row]) + 1) % p
        bad_proof = c.data.prove(bad, pis)
        with pytest.raises(VerifyError, match="vanishing"):
            c.data.verify(bad_proof)
        with pytest.raises(AssertionError, match="vanishing"):
            PD.verify(oc, bad_proof)
    c.data.free()
    return seen


@pytest.mark.parametrize("name", VARIANT_CIRCUITS)
@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_variant_circuits_equal_the_oracle_prover(ctx, field, name):
    seen = check_circuit(ctx, field, name, stages=True, perturb=True)
    assert seen == {g[0] for g in GV.variant_sets(field)[name]}


@pytest.mark.parametrize("field,name,num_challenges", [(N.GB_GOLDILOCKS, "interpolation", 5), (N.GB_BABYBEAR, "interpolation", 11),
                                                       (N.GB_BABYBEAR, "random_access", 7)])
def test_variant_circuits_at_other_challenge_counts(ctx, field, name, num_challenges):
    """interpolation: a challenge count without a compiled kernel width (csrc/challenge_slices.hpp) - every slice evaluates the
    gates again with its own t0 / nterms.  random_access: 7 partial sums per challenge (kernels_gates.hip make_tiled_plan:
    area = max(nw, 7 * num_challenges)) outgrow the widest short gate's wires, so the selector / constant columns are staged
    behind the partial sums, not behind the wires."""
    if name == "random_access":
        widest = max(GV.shape(field, g)[0] for g in GV.variant_sets(field)[name])
        assert max(widest, 4 * (GV.config(field).num_routed_wires // 4)) < 7 * num_challenges   # the set's gates, the builder's ArithmeticGate
    check_circuit(ctx, field, name, stages=True, perturb=False, num_challenges=num_challenges)
