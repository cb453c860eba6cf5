"""The lane-per-point gate kernel k_gate_constraints<F, C, LIGHT_GATES> (csrc/kernels_gates.hip: the `else` of the short-gate
dispatch) through prove().  The tiled kernel takes every quotient domain that is a multiple of 64 points, so no other test runs it.

Natural route: builder circuits with a 32-point quotient domain - 4 rows at max_quotient_degree_factor 8, 8 rows at factor 4 -
with a PublicInputGate, a ConstantGate and ArithmeticGate rows, both fields.  Proof bytes and quotient chunks equal the CPU
oracle prover's, both verifiers accept, and the library's launch counter (include/goldibear_gpu_test_hooks.h:
gb_test_gate_fallback_launches) rises during prove() with nothing forced; the same shape at 64 points leaves it alone.

Forced route (gb_test_force_gate_fallback): the five gate-variant circuits of tests/test_gpu_gate_variants.py and its 5- / 11-challenge
interpolation circuits (sliced launches: the kernel's t0 / nterms offsets) against the oracle prover, the counter rising by one per
challenge slice and quotient computation and standing still once the hook is off; and the recursion gate set at 512 rows - 4096
points, sixteen 256-thread workgroups - whose forced proof must be the tiled route's, byte for byte.  -m gpu only."""
import ctypes as C

import pytest

from oracle import plonk_dummy as PD
from plonky2_goldibear_amd import GpuContext
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import ArithmeticGate, ConstantGate, NoopGate, PublicInputGate

import gate_variants as GV
from circuits import oracle_circuit, poly_chain_circuit, recursion_gates_circuit
from test_gpu_gate_variants import VARIANT_CIRCUITS, check_circuit

pytestmark = pytest.mark.gpu

FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def force_fallback(ctx, on):
    N.check(ctx._lib.gb_test_force_gate_fallback(ctx.handle, int(on)), ctx.handle)


def fallback_launches(ctx):
    n = C.c_uint64()
    N.check(ctx._lib.gb_test_gate_fallback_launches(ctx.handle, C.byref(n)), ctx.handle)
    return n.value


@pytest.fixture
def forced(ctx):
    force_fallback(ctx, True)
    yield ctx
    force_fallback(ctx, False)


def challenge_slices(field, num_challenges):
    """csrc/challenge_slices.hpp for the gate kernels (Goldilocks widths 1..4, BabyBear 4..10, slices of at most 4 / 8)"""
    lo, hi, smax = (1, 4, 4) if field == N.GB_GOLDILOCKS else (4, 10, 8)
    return 1 if lo <= num_challenges <= hi else -(-num_challenges // smax)


def small_circuit(field, rows, factor):
    """y <- y * y + x chains: ArithmeticGate rows, the ConstantGate row of the final value, the PublicInputGate row build() adds (no
    public inputs, so no hash gate), no-ops up to `rows`"""
    cfg = GV.config(field, max_quotient_degree_factor=factor)
    ops_per_row = cfg.num_routed_wires // 4
    arithmetic_rows = 1 if rows == 4 else 3
    b, pw = poly_chain_circuit(cfg, ops_per_row * (arithmetic_rows - 1) + 2)
    return b, pw, arithmetic_rows


def prove_against_the_oracle(ctx, b, pw):
    """-> (proof bytes, launches during prove() alone); the proof and the quotient chunks equal the oracle prover's, both verifiers accept"""
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    before = fallback_launches(ctx)
    proof = c.data.prove(w, pis)
    during_prove = fallback_launches(ctx) - before
    oc = oracle_circuit(c, len(pis))
    assert (c.data.circuit_digest == oc.circuit_digest).all()
    oc.set_cap(c.data.constants_sigmas_cap)
    dump, mid = {}, {}
    want, _ = PD.prove_cpu(oc, w, pis, dump=dump)
    assert proof == want
    from test_gpu_stage_abi import prove_by_stages
    assert prove_by_stages(c.data, oc, w, pis, c.config.field, mid) == want
    assert (mid["quotient_chunks"] == dump["quotient_chunks"]).all()
    assert c.data.verify(proof)
    assert PD.verify(oc, proof)
    c.data.free()
    return c, proof, during_prove


@pytest.mark.parametrize("rows,factor", [(4, 8), (8, 4)])
@pytest.mark.parametrize("field", FIELDS)
def test_a_32_point_quotient_domain_takes_the_lane_per_point_kernel(ctx, field, rows, factor):
    b, pw, arithmetic_rows = small_circuit(field, rows, factor)
    c, _, during_prove = prove_against_the_oracle(ctx, b, pw)
    assert 1 << c.degree_bits == rows and rows * factor == 32
    if field == N.GB_BABYBEAR:
        assert (31 - c.degree_bits) * c.config.num_challenges >= 100
    kinds = [type(g[0]) for g in b.gate_instances]
    assert kinds.count(ArithmeticGate) == arithmetic_rows and kinds.count(ConstantGate) >= 1 and kinds.count(PublicInputGate) == 1
    assert kinds.count(NoopGate) == rows - arithmetic_rows - kinds.count(ConstantGate) - 1
    assert during_prove == challenge_slices(field, c.config.num_challenges)   # nothing forced


@pytest.mark.parametrize("field", FIELDS)
def test_the_same_circuit_at_64_points_takes_the_tiled_kernel(ctx, field):
    b, pw, _ = small_circuit(field, 8, 8)
    before = fallback_launches(ctx)
    c, _, during_prove = prove_against_the_oracle(ctx, b, pw)
    assert c.degree_bits == 3 and c.config.max_quotient_degree_factor == 8
    assert during_prove == 0 and fallback_launches(ctx) == before


@pytest.mark.parametrize("name", VARIANT_CIRCUITS)
@pytest.mark.parametrize("field", FIELDS)
def test_variant_circuits_through_the_forced_fallback_equal_the_oracle_prover(forced, field, name):
    ctx = forced
    before = fallback_launches(ctx)
    check_circuit(ctx, field, name, stages=True, perturb=False)
    # prove() and the stage entry point gb_quotient_polys: one launch per challenge slice each
    assert fallback_launches(ctx) - before == 2 * challenge_slices(field, GV.config(field).num_challenges)
    force_fallback(ctx, False)
    before = fallback_launches(ctx)
    b, pw, _ = small_circuit(field, 8, 8)   # 64 points: the tiled kernel again
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    assert c.data.verify(c.data.prove(w, pis))
    c.data.free()
    assert fallback_launches(ctx) == before


@pytest.mark.parametrize("field,num_challenges", [(N.GB_GOLDILOCKS, 5), (N.GB_BABYBEAR, 11)])
def test_sliced_launches_through_the_forced_fallback(forced, field, num_challenges):
    """a challenge count without a compiled kernel width: two slices, each with its own alpha powers, qv block and t0 / nterms"""
    ctx = forced
    slices = challenge_slices(field, num_challenges)
    assert slices == 2
    before = fallback_launches(ctx)
    check_circuit(ctx, field, "interpolation", stages=True, perturb=False, num_challenges=num_challenges)
    assert fallback_launches(ctx) - before == 2 * slices


def test_the_widest_gate_has_as_many_constraints_as_the_fold_sums_were_checked_for(ctx):
    """csrc/fold_acc.hpp FOLD_ACC_MAX_TERMS = 4096: a gate has no more constraints than wires, and gb_circuit_create_gates takes at most
    4096 wires, as gb_verifier_create does - BaseSumGate with 4095 limbs (4096 constraints) is accepted, a 4097-wire config is not"""
    import numpy as np
    from plonky2_goldibear_amd import ShapeError
    from plonky2_goldibear_amd.prover import CircuitData
    cs, k = np.zeros((1 + 2 + 80, 8), dtype=np.uint64), np.ones(80, dtype=np.uint64)
    gates = [(GV.G.NOOP, 0, 0, 0, 2, 0, 0), (GV.G.BASE_SUM, 4095, 0, 0, 2, 2, 0)]
    CircuitData(ctx, 3, cs, k, gates=gates, num_selectors=1, num_wires=4096).free()
    with pytest.raises(ShapeError, match="4096 wires"):
        CircuitData(ctx, 3, cs, k, gates=gates, num_selectors=1, num_wires=4097)


@pytest.mark.parametrize("field", FIELDS)
def test_forced_and_tiled_routes_give_the_same_proof_over_several_workgroups(ctx, field):
    """the recursion gate set (one row of each gate) padded to 512 rows: 4096 quotient points, sixteen workgroups of the
    lane-per-point kernel, 64 of the tiled one"""
    b, pw, _ = recursion_gates_circuit(field, seed=11, public_inputs=True)
    x = b.add_virtual_target()
    pw.set_target(x, 3)
    y = x
    for _ in range(260 * (b.config.num_routed_wires // 4)):   # 260 ArithmeticGate rows
        y = b.mul_add(y, y, x)
    c = b.build(ctx)
    assert c.degree_bits == 9
    w, pis = c.generate_witness(pw)
    before = fallback_launches(ctx)
    tiled = c.data.prove(w, pis)
    assert fallback_launches(ctx) == before
    force_fallback(ctx, True)
    try:
        forced_proof = c.data.prove(w, pis)
    finally:
        force_fallback(ctx, False)
    assert fallback_launches(ctx) - before == challenge_slices(field, c.config.num_challenges)
    assert forced_proof == tiled
    assert c.data.verify(forced_proof)
    assert PD.verify(oracle_circuit(c, len(pis)), forced_proof)
    c.data.free()
