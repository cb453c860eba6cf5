"""Circuits whose generators use the integer operations of a generator program, proved from their inputs alone (-m gpu only):

  * mul_add_split_gate rows (plonky2_goldibear_amd/integer_gadgets.py) at 2^3 and 2^5 rows with inputs at the range edges, both
    fields: generation on the device equals the mirror at every target, prove_inputs(pw) == prove(pw) byte for byte, verify
    accepts, check_inputs reports nothing; with the literal 2^half_bits - 1 of the generator replaced by 2^half_bits - 2,
    check_inputs names the gate's first constraint at the rows whose a * b + c is odd, and nothing else;
  * twins that the oracle judges: tests/gadget_cases.py's split_le circuit with its built-in generators (WireSplitGenerator,
    BaseSplitGenerator) against the same gates and wiring with both splits done by programs (ops.low_bits / ops.shr, ops.bits),
    for x in {0, 1, p - 1}; its div_extension circuit with QuotientGeneratorExtension against a program written with ops.ext.
    Equal proof bytes, and oracle/plonk_dummy.py's verifier accepts them;
  * div_rem and is_less_than at num_bits = 16 on (0, 1), (65535, 1), (65535, 65535), (12345, 678): the proofs verify and carry
    q, r and lt; y = 0 is GB_ERR_INVALID with "attempt to divide by zero" and the record's index, and the next proof on the same
    circuit succeeds.  div_rem at 16 bits runs on Goldilocks alone: on BabyBear q * y + r can reach 2^32 - 2^16 > p, the equation
    would hold modulo p only, and div_rem refuses the width (tests/test_integer_programs.py); BabyBear runs is_less_than at 16
    bits and div_rem at 15 bits on operands that fit;
  * README.md's u32 example, line for line."""
import numpy as np
import pytest

import circuits as CS
import gadget_cases as GA
from oracle import plonk_dummy as PD
from plonky2_goldibear_amd import GeneratorProgram, GpuContext, ProgramGenerator, ShapeError, div_rem, is_less_than, mul_add_split_gate
from plonky2_goldibear_amd import generator_program as GP
from plonky2_goldibear_amd import integer_gadgets as IG
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import (CircuitBuilder, PartialWitness, _QuotientExtensionGenerator, _WireSplitGenerator,
                                                   wire)
from plonky2_goldibear_amd.gate_program import field_order
from plonky2_goldibear_amd.recursion_gates import BaseSumGate

pytestmark = pytest.mark.gpu
SEED = 31
FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]
IDS = ["goldilocks", "babybear"]
rng = lambda: np.random.default_rng(SEED)


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def check_circuit(c, pw, what, oracle_as=None):
    want = c.generate_partition_witness(pw, rng())
    got = c.generate_partition_device(pw, rng())
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d targets differ, first %d: %d, mirror %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    assert c.data.generators_info()["num_unrunnable"] == 0, what
    by_partition = c.prove(pw, rng())
    proof = c.prove_inputs(pw, rng())
    assert proof == by_partition, what
    assert c.verify(proof), what
    violations, res = c.check_inputs(pw, rng())
    assert violations == [] and res.num_gate_violations == 0 and res.num_copy_violations == 0, (what, violations)
    if oracle_as is not None:
        assert PD.verify(CS.oracle_circuit(oracle_as, len(c.public_inputs)), proof), what
    return proof


# ------------------------------------------------------------------------------------------------ the gate from its inputs
def split_rows_circuit(field, degree_bits, generator_program=None):
    """rows of mul_add_split_gate, each with inputs of its own at the range edges -> (builder, partial witness, [(row, a, b, c)])"""
    b, pw = CircuitBuilder(GA.config(field)), PartialWitness()
    gate = mul_add_split_gate(field, generator_program=generator_program)
    top = (1 << IG.HALF_BITS[field]) - 1
    edge = [(top, top, top), (0, 0, 0), (top, 1, 0), (1, 1, top), (top - 1, 3, 5), (1, top, top), (top, top, 0), (0, top, 1)]
    rows = []
    for k in range((1 << degree_bits) - 4):      # build() adds the public-input gate, the public inputs' hash and a ConstantGate
        row = b.add_gate(gate)
        for col, v in enumerate(edge[k % len(edge)]):
            t = b.add_virtual_target()
            b.connect(t, wire(row, col))
            pw.set_target(t, v)
        rows.append((row,) + edge[k % len(edge)])
    b.register_public_inputs([wire(rows[0][0], 3), wire(rows[-1][0], 4)])
    return b, pw, rows


@pytest.mark.parametrize("degree_bits", [3, 5])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_mul_add_split_gate_rows_from_their_inputs(ctx, field, degree_bits):
    h = IG.HALF_BITS[field]
    b, pw, rows = split_rows_circuit(field, degree_bits)
    c = b.build(ctx)
    assert c.degree_bits == degree_bits and len(c.generator_programs) == 1
    what = "MulAddSplitGate (field %d, 2^%d rows)" % (field, degree_bits)
    check_circuit(c, pw, what)
    wires, _ = c.generate_witness(pw, rng())
    for row, a, bb, cc in rows:
        x = a * bb + cc
        assert (int(wires[3, row]), int(wires[4, row])) == (x & ((1 << h) - 1), x >> h), what
    c.data.free()
    # a generator that masks with 2^h - 2: low loses its bit 0, the limbs follow low, so the first constraint alone breaks
    prog = IG.mul_add_split_program(field)
    top = (1 << h) - 1
    assert prog.literals.count(top) == 1
    words = list(prog.words)
    words[GP.HEADER_WORDS + prog.literals.index(top)] = top - 1
    b, pw, rows = split_rows_circuit(field, degree_bits, generator_program=GeneratorProgram(words, field))
    c = b.build(ctx)
    violations, res = c.check_inputs(pw, rng(), max_violations=64)
    odd = [row for row, a, bb, cc in rows if (a * bb + cc) & 1]
    assert odd and sorted(v.row for v in violations) == odd and res.num_gate_violations == len(odd) and res.num_copy_violations == 0
    assert all(v.kind == N.GB_VIOLATION_GATE and v.index == 0 and v.value == 1 for v in violations)
    first = min(violations, key=lambda v: v.row)
    assert first.describe(c) == "row %d: MulAddSplitGate { half_bits: %d }, constraint 0 = 1" % (odd[0], h)
    c.data.free()


# ------------------------------------------------------------------------------------------------ twins
class ProgramBaseSumGate(BaseSumGate):
    """BaseSumGate<2> with its id and parameters, the BaseSplitGenerator a generator program"""

    def __init__(self, num_limbs, field):
        super().__init__(num_limbs, 2)
        self.split = GeneratorProgram.from_function(lambda d, c, ops: ops.bits(d[0], num_limbs), 1, num_limbs, 0, field)

    def generators(self, row, constants):
        return [ProgramGenerator("BaseSplitGenerator", self.split, [wire(row, 0)], [wire(row, 1 + i) for i in range(self.num_limbs)])]


def with_program_splits(b):
    """the builder's BaseSumGate<2> rows and WireSplitGenerators with programs in the generators' places"""
    field, cache = b.config.field, {}

    def conv(g):
        if not (isinstance(g, BaseSumGate) and g.base == 2):
            return g
        if g.id not in cache:
            cache[g.id] = ProgramBaseSumGate(g.num_limbs, field)
        return cache[g.id]

    b.gates = {conv(g) for g in b.gates}
    for inst in b.gate_instances:
        inst[0] = conv(inst[0])

    def wire_split(g):
        n, L = len(g.gates), g.num_limbs
        prog = GeneratorProgram.from_function(lambda d, c, ops: [ops.low_bits(ops.shr(d[0], k * L), L) for k in range(n)], 1, n, 0, field)
        return ProgramGenerator("WireSplitGenerator", prog, [g.integer], [wire(row, 0) for row in g.gates])

    b.generators = [wire_split(g) if isinstance(g, _WireSplitGenerator) else g for g in b.generators]
    return b


def with_program_quotients(b):
    field = b.config.field
    D = GP.EXT_W[field][0]
    prog = GeneratorProgram.from_function(lambda d, c, ops: (ops.ext(d[:D]) / ops.ext(d[D:])).coords, 2 * D, D, 0, field)
    b.generators = [ProgramGenerator("QuotientGeneratorExtension", prog, g.numerator + g.denominator, g.quotient)
                    if isinstance(g, _QuotientExtensionGenerator) else g for g in b.generators]
    return b


def gadget_circuit(field, name):
    (hit,) = [(b, pw) for n, b, pw in GA.builder_circuits(field, 3) if n == name]
    return hit


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_split_le_twin_with_program_splits(ctx, field):
    p = field_order(field)
    name = "split_le, %d bits" % GA.top_bits(field)
    (b0, _), (b1, _) = gadget_circuit(field, name), gadget_circuit(field, name)
    assert sum(isinstance(g, _WireSplitGenerator) for g in b1.generators) == 1
    with_program_splits(b1)
    c0, c1 = b0.build(ctx), b1.build(ctx)
    assert c1.degree_bits == c0.degree_bits and len(c1.generator_programs) >= 2 and not c0.generator_programs
    assert np.array_equal(c0.constants_sigmas, c1.constants_sigmas) and c0.gate_ids == c1.gate_ids
    for x in (0, 1, p - 1):
        pw = PartialWitness()
        pw.set_target(("v", 0), x)
        proof = check_circuit(c1, pw, "split_le twin (field %d, x = %d)" % (field, x), oracle_as=c0)
        assert proof == c0.prove_inputs(pw, rng())
        _, pis = c1.generate_witness(pw, rng())
        assert [int(v) for v in pis] == [x & 1, x >> (GA.top_bits(field) - 1)]
    c0.data.free()
    c1.data.free()


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_div_extension_twin_with_ops_ext(ctx, field):
    (b0, pw), (b1, _) = gadget_circuit(field, "div_extension"), gadget_circuit(field, "div_extension")
    assert sum(isinstance(g, _QuotientExtensionGenerator) for g in b1.generators) >= 2
    with_program_quotients(b1)
    c0, c1 = b0.build(ctx), b1.build(ctx)
    assert len(c1.generator_programs) == 1 and not c0.generator_programs
    proof = check_circuit(c1, pw, "div_extension twin (field %d)" % field, oracle_as=c0)
    assert proof == c0.prove_inputs(pw, rng())
    c0.data.free()
    c1.data.free()


# ------------------------------------------------------------------------------------------------ div_rem and is_less_than
def head_record_of(c, generator_id):
    """the index of the head record of the built circuit's first generator with this id"""
    at = 0
    for g in c.generators:
        r = g.record(c)
        if getattr(g, "id", None) == generator_id:
            return at
        at += len(r) if isinstance(r, list) else (r is not None)
    raise KeyError(generator_id)


def witness(x, y, xv, yv):
    pw = PartialWitness()
    pw.set_target(x, xv)
    pw.set_target(y, yv)
    return pw


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_div_rem_and_is_less_than(ctx, field):
    gl = field == N.GB_GOLDILOCKS
    b = CircuitBuilder(GA.config(field))
    x, y = b.add_virtual_target(), b.add_virtual_target()
    lt = is_less_than(b, x, y, 16)
    outs = [lt]
    if gl:
        outs += list(div_rem(b, x, y, 16))
    b.register_public_inputs(outs)
    c = b.build(ctx)
    for xv, yv in ((0, 1), (65535, 1), (65535, 65535), (12345, 678)):
        what = "div_rem / is_less_than (field %d, %d, %d)" % (field, xv, yv)
        pw = witness(x, y, xv, yv)
        check_circuit(c, pw, what)
        _, pis = c.generate_witness(pw, rng())
        assert [int(v) for v in pis] == [int(xv < yv)] + ([xv // yv, xv % yv] if gl else []), what
    if gl:
        head = head_record_of(c, "DivRemGenerator")
        assert c.generator_records()[head][0] == N.GB_GEN_PROGRAM
        bad = witness(x, y, 12345, 0)
        for run in (c.prove_inputs, c.generate_partition_device):
            with pytest.raises(ShapeError, match="attempt to divide by zero") as e:
                run(bad)
            assert "generator record %d:" % head in str(e.value) and "IDIV / IREM in a generator program" in str(e.value)
        with pytest.raises(GP.IntegerDivideByZeroError, match="attempt to divide by zero"):
            c.generate_partition_witness(bad)
        check_circuit(c, witness(x, y, 12345, 678), "div_rem after a division by zero")
    c.data.free()


def test_div_rem_on_babybear_at_15_bits(ctx):
    field = N.GB_BABYBEAR
    b = CircuitBuilder(GA.config(field))
    x, y = b.add_virtual_target(), b.add_virtual_target()
    b.register_public_inputs(list(div_rem(b, x, y, 15)))
    c = b.build(ctx)
    head = head_record_of(c, "DivRemGenerator")
    for xv, yv in ((0, 1), (32767, 1), (32767, 32767), (32767 * 32767 + 32766, 32767), (12345, 678)):
        pw = witness(x, y, xv, yv)
        check_circuit(c, pw, "div_rem (BabyBear, %d, %d)" % (xv, yv))
        _, pis = c.generate_witness(pw, rng())
        assert [int(v) for v in pis] == [xv // yv, xv % yv]
    with pytest.raises(ShapeError, match="attempt to divide by zero") as e:
        c.prove_inputs(witness(x, y, 5, 0))
    assert "generator record %d:" % head in str(e.value)
    check_circuit(c, witness(x, y, 12345, 678), "div_rem after a division by zero (BabyBear)")
    c.data.free()


# ------------------------------------------------------------------------------------------------ README.md, "u32 arithmetic"
def test_readme_u32_example(ctx):
    from plonky2_goldibear_amd import GB_GOLDILOCKS
    from plonky2_goldibear_amd.circuit_builder import CircuitConfig

    builder, pw = CircuitBuilder(CircuitConfig.standard_recursion_config_gl()), PartialWitness()
    row = builder.add_gate(mul_add_split_gate(GB_GOLDILOCKS))          # a * b + c = low + 2^32 * high
    a, b, c = builder.add_virtual_targets(3)
    for col, t in enumerate((a, b, c)):
        builder.connect(t, wire(row, col))
    low, high = wire(row, 3), wire(row, 4)
    q, r = div_rem(builder, high, builder.constant(1000), 32)           # high = q * 1000 + r, r < 1000
    builder.register_public_inputs([low, q, r])
    pw.set_target(a, 0xFFFFFFFF)
    pw.set_target(b, 0xFFFFFFFE)
    pw.set_target(c, 12345)
    circuit = builder.build(ctx)
    proof = circuit.prove_inputs(pw)                                    # every generator runs on the device
    assert proof == circuit.prove(pw) and circuit.verify(proof)

    x = 0xFFFFFFFF * 0xFFFFFFFE + 12345
    _, pis = circuit.generate_witness(pw)
    assert [int(v) for v in pis] == [x & 0xFFFFFFFF, (x >> 32) // 1000, (x >> 32) % 1000]
    circuit.data.free()
