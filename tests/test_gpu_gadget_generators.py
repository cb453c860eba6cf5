"""Circuits built with the gadgets of circuit_builder.py (is_equal, split_le, le_sum, split_low_high, div_extension, select),
proved from the inputs alone: their generators - EqualityGenerator, QuotientOrZeroGenerator, QuotientGeneratorExtension,
WireSplitGenerator, LowHighGenerator, BaseSumGenerator, handed over as head and continuation records - run on the device
(gb_circuit_set_generators, gb_generate_partition, gb_prove_inputs).  The oracle is the builder mirror; every comparison is exact;
gb_verify is the independent check, since the gadgets' own constraints pin every generated value.

  * every circuit of tests/gadget_cases.py at degree_bits 3..7, both fields: generation == the mirror at every target,
    prove_inputs bytes == prove bytes, verified;
  * one of them as a zero-knowledge circuit with salts;
  * a zero denominator and a limb that is no bool are GB_ERR_INVALID with the reference's message, and the same circuit proves a
    good witness afterwards;
  * a circuit without gadget records proves as before."""
import numpy as np
import pytest

import circuits as CS
import gadget_cases as GA
import gate_variants as GV
from plonky2_goldibear_amd import CircuitData, GpuContext, ShapeError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, PartialWitness

pytestmark = pytest.mark.gpu
SEED = 23
FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def check_circuit(c, pw, what):
    want = c.generate_partition_witness(pw, np.random.default_rng(SEED))
    got = c.generate_partition_device(pw, np.random.default_rng(SEED))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d targets differ, first %d: %d, mirror %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    info = c.data.generators_info()
    assert info["num_unrunnable"] == 0, what
    by_partition = c.prove(pw, np.random.default_rng(SEED))
    proof = c.prove_inputs(pw, np.random.default_rng(SEED))
    assert proof == by_partition, what
    assert c.verify(proof), what
    return info


@pytest.mark.parametrize("degree_bits", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("field", FIELDS, ids=["goldilocks", "babybear"])
def test_gadget_circuits_prove_from_their_inputs(ctx, field, degree_bits):
    reached = set()
    for name, b, pw in GA.builder_circuits(field, degree_bits):
        c = b.build(ctx)
        assert degree_bits <= c.degree_bits <= 7, name
        reached.add(c.degree_bits)
        # (the arithmetic branch of le_sum is the one circuit without a gadget generator)
        assert any(r[0] == N.GB_GEN_TARGETS for r in c.generator_records()) == (name != "le_sum, arithmetic branch"), name
        info = check_circuit(c, pw, "%s (field %d, 2^%d rows)" % (name, field, c.degree_bits))
        assert info["num_launches"] == 1, (name, info)
        c.data.free()
    assert degree_bits in reached


@pytest.mark.parametrize("field", FIELDS, ids=["goldilocks", "babybear"])
def test_a_zero_knowledge_circuit_with_salts(ctx, field):
    F = GV.FIELDS[field]
    name, b, pw = next(x for x in GA.builder_circuits(field, 5) if x[0] == "split_low_high")
    built = b.build()
    cfg = built.config
    gpu = CircuitData(ctx, built.degree_bits, built.constants_sigmas, built.k_is, num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires,
                      num_constants=built.max_constants, num_challenges=cfg.num_challenges, max_quotient_degree_factor=cfg.max_quotient_degree_factor,
                      rate_bits=cfg.rate_bits, cap_height=cfg.cap_height, proof_of_work_bits=cfg.proof_of_work_bits,
                      num_query_rounds=cfg.num_query_rounds, arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits,
                      num_selectors=built.num_selectors, field=field, gates=built.gate_table, num_public_inputs=len(built.public_inputs),
                      zero_knowledge=True)
    n_lde = (1 << built.degree_bits) << cfg.rate_bits
    salts = F.fill(0x5A17, 3 * 4 * n_lde).reshape(3, 4, n_lde)
    gpu.set_partition(built.representative_map, built.public_input_targets)
    inputs = list(pw.values) + [t for t in built.random_targets if t not in pw.values]
    gpu.set_generators(built.generator_records(), [built.target_index(t) for t in inputs], built.constants_columns)
    built._input_targets = inputs
    values = built.generate_partition_witness(pw, np.random.default_rng(SEED))
    want = gpu.prove_partition_once(values, salts)
    got = gpu.prove_inputs_once(built.input_values(pw, np.random.default_rng(SEED)), salts=salts)
    assert got == want
    assert gpu.verify(got)
    with pytest.raises(ShapeError):
        gpu.prove_inputs_once(built.input_values(pw, np.random.default_rng(SEED)))      # a zero-knowledge circuit needs its salts
    gpu.free()


@pytest.mark.parametrize("field", FIELDS, ids=["goldilocks", "babybear"])
def test_a_zero_denominator_and_a_limb_that_is_no_bool(ctx, field):
    D = GV.FIELDS[field].D
    # div_extension by zero
    b, pw, bad = CircuitBuilder(GA.config(field)), PartialWitness(), PartialWitness()
    x, y = b.add_virtual_extension_target(), b.add_virtual_extension_target()
    b.register_public_inputs(list(b.div_extension(x, y)))
    for k in range(D):
        for w, den in ((pw, 7 + k), (bad, 0)):
            w.set_target(x[k], 11 + k)
            w.set_target(y[k], den)
    c = b.build(ctx)
    c.set_generators(pw=pw)
    with pytest.raises(ShapeError, match="Tried to invert zero") as e:
        c.prove_inputs(bad)
    head = next(i for i, r in enumerate(c.generator_records()) if r[0] == N.GB_GEN_QUOTIENT_EXTENSION)
    assert "generator record %d:" % head in str(e.value)
    assert "target %d)" % c.representative_map[c.target_index(y[0])] in str(e.value)
    with pytest.raises(ShapeError, match="Tried to invert zero"):
        c.generate_partition_device(bad)
    with pytest.raises(AssertionError):
        c.generate_partition_witness(bad)
    check_circuit(c, pw, "div_extension after a refused witness")
    c.data.free()
    # le_sum over a "bit" that is 2
    b, pw, bad = CircuitBuilder(GA.config(field)), PartialWitness(), PartialWitness()
    bits = b.add_virtual_targets(b.config.num_routed_wires // 4 + 2)
    b.register_public_input(b.le_sum(bits))
    for i, t in enumerate(bits):
        pw.set_target(t, i & 1)
        bad.set_target(t, 2 if i == 5 else i & 1)
    c = b.build(ctx)
    c.set_generators(pw=pw)
    with pytest.raises(ShapeError, match="not a bool") as e:
        c.prove_inputs(bad)
    head = next(i for i, r in enumerate(c.generator_records()) if r[0] == N.GB_GEN_BASE_SUM)
    assert "generator record %d:" % head in str(e.value)
    with pytest.raises(AssertionError):
        c.generate_partition_witness(bad)
    check_circuit(c, pw, "le_sum after a refused witness")
    c.data.free()


def test_circuits_without_gadget_records_prove_as_before(ctx):
    """the factorial circuit has none: its schedule and its proof are what they were; beside it a circuit of split_le, is_equal
    and div_extension proves through prove_inputs with the bytes of prove"""
    b, pw = CS.factorial_circuit(count=60)
    c = b.build(ctx)
    assert all(r[0] <= N.GB_GEN_COPY for r in c.generator_records())
    info = check_circuit(c, pw, "factorial")
    assert info["num_launches"] == 1 and info["num_levels"] > 30, info
    c.data.free()
    b, pw = CircuitBuilder(GA.config(N.GB_GOLDILOCKS)), PartialWitness()
    x, y = b.add_virtual_target(), b.add_virtual_target()
    bits = b.split_le(x, 40)
    e = b.is_equal(b.le_sum(bits[:30]), y)
    q = b.div_extension(b.convert_to_ext(x), (y, e) )
    b.register_public_inputs([e] + list(q))
    pw.set_target(x, 0xFEDCBA9876)
    pw.set_target(y, 0xFEDCBA9876 & (2**30 - 1))
    c = b.build(ctx)
    info = check_circuit(c, pw, "split_le, is_equal and div_extension")
    assert c.generate_witness(pw)[1][0] == 1
    c.data.free()
