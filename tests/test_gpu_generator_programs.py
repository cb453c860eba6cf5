"""Circuits whose generators are generator programs (GB_GEN_PROGRAM, gb_circuit_set_generator_programs), proved from the inputs
alone: tests/generator_program_circuits.py's MulAddThreeGate rows (a program gate with its generator program), the poly-chain
circuit with program gates AND generator programs, and examples/square_root.rs, both fields, 2^3 .. 2^6 rows.  The oracle is the
builder mirror, whose ProgramGenerator.run is GeneratorProgram.evaluate; every comparison is exact.

  * generation on the device == the mirror's partition witness at every target; prove_inputs bytes == prove bytes; gb_verify
    accepts; oracle/plonk_dummy.py's verifier accepts where it knows the gates (the square-root circuit, and the poly chain, whose
    proof is byte for byte that of the circuit with built-in gates; the oracle has no program gates, so not MulAddThreeGate);
  * the MulAddThreeGate rows in a circuit with two selector columns: the row constants come from the columns behind both;
  * the square-root circuit as a zero-knowledge circuit with salts;
  * INV of zero, SQRT of a non-residue and a program output that disagrees with an input of its class are GB_ERR_INVALID with the
    index of the head record, and the same circuit proves a good witness afterwards;
  * the programs are replaced and dropped as include/goldibear_gpu.h says."""
import numpy as np
import pytest

import circuits as CS
import gadget_cases as GA
import gate_variants as GV
import generator_program_cases as PC
import generator_program_circuits as GPC
from oracle import plonk_dummy as PD
from plonky2_goldibear_amd import CircuitData, GpuContext, ShapeError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import PartialWitness
from plonky2_goldibear_amd.generator_program import field_sqrt

pytestmark = pytest.mark.gpu
SEED = 29
FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]
IDS = ["goldilocks", "babybear"]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def check_circuit(c, pw, what, oracle_as=None):
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
    if oracle_as is not None:
        assert PD.verify(CS.oracle_circuit(oracle_as, len(c.public_inputs)), proof), what
    return proof


def program_heads(c):
    return [i for i, r in enumerate(c.generator_records()) if r[0] == N.GB_GEN_PROGRAM]


@pytest.mark.parametrize("degree_bits", [3, 4, 5, 6])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_mul_add_three_gate_rows_with_their_generator_program(ctx, field, degree_bits):
    rows = (1 << degree_bits) - 3
    b, pw = GPC.mul_add_three_circuit(GA.config(field), rows)
    c = b.build(ctx)
    assert c.degree_bits == degree_bits and len(c.generator_programs) == 1 and len(program_heads(c)) == rows
    check_circuit(c, pw, "MulAddThreeGate (field %d, 2^%d rows)" % (field, degree_bits))
    assert c.data.generators_info()["num_levels"] >= rows      # every row waits for the one before it
    c.data.free()


@pytest.mark.parametrize("degree_bits", [3, 5])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_row_constants_behind_two_selector_columns(ctx, field, degree_bits):
    """The MulAddThreeGate rows with their last output a public input: the permutation gate joins the gate set, which then needs two
    selector columns, and the programs' constants are read at rows 0 .. rows - 1 of the columns behind both.  Either neighbour of
    the right column holds other values at every program row, so a column offset that is off by one cannot pass."""
    rows = (1 << degree_bits) - 4
    b, pw = GPC.mul_add_three_circuit(GA.config(field), rows, public_output=True)
    c = b.build(ctx)
    assert c.num_selectors == 2 and c.degree_bits == degree_bits and len(c.public_inputs) == 1
    heads = [r for r in c.generator_records() if r[0] == N.GB_GEN_PROGRAM]
    assert [int(h[3]) for h in heads] == list(range(rows))                 # the rows whose constants the programs read
    cs = c.constants_sigmas
    assert np.array_equal(c.constants_columns, cs[2:2 + c.max_constants])
    for row in range(rows):
        k = 5 + 3 * row
        assert int(cs[2][row]) == k and int(cs[1][row]) != k and int(cs[3][row]) != k
    check_circuit(c, pw, "MulAddThreeGate behind two selectors (field %d, 2^%d rows)" % (field, degree_bits))
    c.data.free()


@pytest.mark.parametrize("degree_bits", [3, 6])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_poly_chain_with_program_gates_and_generator_programs(ctx, field, degree_bits):
    cfg = GA.config(field)
    steps = (3 if degree_bits == 3 else 40) * ArithmeticOps(cfg)
    b0, b1, pw = GPC.poly_chain_pair(cfg, steps)
    c0, c1 = b0.build(ctx), b1.build(ctx)
    assert c1.degree_bits == degree_bits and len(program_heads(c1)) == steps and not program_heads(c0)
    proof = check_circuit(c1, pw, "poly chain (field %d, 2^%d rows)" % (field, degree_bits), oracle_as=c0)
    assert proof == c0.prove_inputs(pw, np.random.default_rng(SEED))     # the built-in generators give the same bytes
    c0.data.free()
    c1.data.free()


def ArithmeticOps(cfg):
    from plonky2_goldibear_amd.circuit_builder import ArithmeticGate
    return ArithmeticGate.new_from_config(cfg).num_ops


@pytest.mark.parametrize("degree_bits", [3, 5])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_square_root_example(ctx, field, degree_bits):
    p = GV.FIELDS[field].P
    b, pw, x, x_squared = GPC.square_root_circuit(GA.config(field), pow(0xC0FFEE, 2, p), pad_to=1 << degree_bits)
    c = b.build(ctx)
    assert c.degree_bits == degree_bits
    check_circuit(c, pw, "square root (field %d)" % field, oracle_as=c)
    root = int(c.generate_partition_device(pw)[c.representative_map[c.target_index(x)]])
    assert root * root % p == pow(0xC0FFEE, 2, p) and root == field_sqrt(pow(0xC0FFEE, 2, p), field)
    c.data.free()


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_square_root_as_a_zero_knowledge_circuit_with_salts(ctx, field):
    F = GV.FIELDS[field]
    b, pw, x, x_squared = GPC.square_root_circuit(GA.config(field), 49, pad_to=32)
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
    gpu.set_generator_programs(built.generator_programs)
    inputs = list(pw.values) + [t for t in built.random_targets if t not in pw.values]
    gpu.set_generators(built.generator_records(), [built.target_index(t) for t in inputs], built.constants_columns)
    built._input_targets = inputs
    values = built.generate_partition_witness(pw, np.random.default_rng(SEED))
    want = gpu.prove_partition_once(values, salts)
    got = gpu.prove_inputs_once(built.input_values(pw, np.random.default_rng(SEED)), salts=salts)
    assert got == want
    assert gpu.verify(got)
    gpu.free()


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_errors_name_the_head_record_and_leave_the_circuit_usable(ctx, field):
    p = GV.FIELDS[field].P
    # INV of zero
    b, y = GPC.inverse_circuit(GA.config(field))
    pw, bad = PartialWitness(), PartialWitness()
    pw.set_target(y, 12345)
    bad.set_target(y, 0)
    c = b.build(ctx)
    c.set_generators(pw=pw)
    (head,) = program_heads(c)
    for run in (c.prove_inputs, c.generate_partition_device):
        with pytest.raises(ShapeError, match="Tried to invert zero") as e:
            run(bad)
        assert "generator record %d:" % head in str(e.value)
    with pytest.raises(ArithmeticError, match="Tried to invert zero"):
        c.generate_partition_witness(bad)
    check_circuit(c, pw, "inverse after a refused witness")
    c.data.free()
    # SQRT of a non-residue; then x given as an input too: the other root satisfies x * x = x_squared, the generator disagrees
    square = pow(777, 2, p)
    b, pw, x, x_squared = GPC.square_root_circuit(GA.config(field), square)
    bad = PartialWitness()
    bad.set_target(x_squared, PC.NON_RESIDUE[field])
    c = b.build(ctx)
    c.set_generators(pw=pw)
    (head,) = program_heads(c)
    with pytest.raises(ShapeError, match="non-residue") as e:
        c.prove_inputs(bad)
    assert "generator record %d:" % head in str(e.value) and "unwrap" in str(e.value)
    with pytest.raises(ArithmeticError, match="unwrap"):
        c.generate_partition_witness(bad)
    check_circuit(c, pw, "square root after a non-residue")
    root = field_sqrt(square, field)
    good, bad = PartialWitness(), PartialWitness()
    for w, v in ((good, root), (bad, p - root)):
        w.set_target(x_squared, square)
        w.set_target(x, v)
    c.set_generators(pw=good)
    with pytest.raises(ShapeError, match="was set twice with different values") as e:
        c.prove_inputs(bad)
    assert "generator record %d:" % head in str(e.value)
    assert "target %d " % c.representative_map[c.target_index(x)] in str(e.value)
    check_circuit(c, good, "square root with x as an input")
    c.data.free()


def test_programs_are_replaced_and_dropped_as_the_header_says(ctx):
    field = N.GB_GOLDILOCKS
    b, pw, x, x_squared = GPC.square_root_circuit(GA.config(field), 81)
    c = b.build(ctx)
    records = c.generator_records()
    inputs = [c.target_index(t) for t in list(pw.values) + c.random_targets]
    (head,) = program_heads(c)
    with pytest.raises(ShapeError, match="gb_circuit_set_partition has not been called"):
        c.data.set_generator_programs(c.generator_programs)
    c.data.set_partition(c.representative_map, c.public_input_targets)
    with pytest.raises(ShapeError, match="generator record %d: no generator programs are set" % head):
        c.data.set_generators(records, inputs, c.constants_columns)
    bad = list(c.generator_programs[0].words)
    bad[-1] |= 1 << 63
    with pytest.raises(ShapeError, match="generator program 0 instruction %d: bits 60-63" % (c.generator_programs[0].num_instrs - 1)):
        c.data.set_generator_programs([bad])
    c.data.set_generator_programs(c.generator_programs)
    c.data.set_generators(records, inputs, c.constants_columns)
    assert c.data.generators_info()["num_unrunnable"] == 0
    c.data.set_generator_programs(c.generator_programs)            # again: the schedule built on the old ones is dropped
    with pytest.raises(ShapeError, match="gb_circuit_set_generators has not been called"):
        c.data.generators_info()
    c.data.set_generator_programs([])                               # cleared
    with pytest.raises(ShapeError, match="no generator programs are set"):
        c.data.set_generators(records, inputs, c.constants_columns)
    c.data.set_generator_programs(c.generator_programs)
    c.data.set_partition(c.representative_map, c.public_input_targets)   # drops the programs with the schedule
    with pytest.raises(ShapeError, match="no generator programs are set"):
        c.data.set_generators(records, inputs, c.constants_columns)
    c._partition_set = True
    check_circuit(c, pw, "after the programs were set again")
    # kinds 41..47 stay refused as unsupported
    with pytest.raises(N.GoldibearError, match="kind 47 is no built generator kind"):
        c.data.set_generators([(47, 0, 0, 0)], inputs, c.constants_columns)
    c.data.free()
