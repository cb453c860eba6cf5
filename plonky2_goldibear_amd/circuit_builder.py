"""Host-side mirror of the reference's CircuitBuilder / PartialWitness for the gate set the GPU prover evaluates.

What a Rust host already has (plonky2/src/plonk/circuit_builder.rs, gadgets/arithmetic.rs, iop/generator.rs), restated in
Python so that circuits other than the dummy one - the reference's `factorial` example is the model
(plonky2/examples/factorial.rs) - can be built, witnessed and handed to `gb_circuit_create_gates` / `gb_prove`:

    builder = CircuitBuilder(CircuitConfig.standard_recursion_config_gl())
    x = builder.add_virtual_target(); y = builder.mul(x, builder.constant(3)); builder.register_public_input(y)
    data = builder.build(ctx)                   # CircuitData: constants||sigmas committed on the GPU
    pw = PartialWitness(); pw.set_target(x, 5)
    proof = data.prove_inputs(pw)               # witness generation, full_witness() and prove() on the GPU
    proof = data.prove(pw)                      # the same bytes: witness generation on the host (gb_prove_partition)
    data.verify(proof)

Gates: NoopGate, ConstantGate, PublicInputGate, ArithmeticGate (gates/arithmetic_base.rs) and the in-circuit hash of the
configuration - PoseidonGate (gates/poseidon_goldilocks.rs) for Goldilocks, Poseidon2BabyBearGate (gates/poseidon2_babybear.rs)
for BabyBear - which `build()` itself needs as soon as a circuit has public inputs, because it hashes them in-circuit
(circuit_builder.rs:1126-1137).  The other gates of the recursion circuits are in recursion_gates.py (add_gate() takes them).
Gadgets, laid out as the reference lays them out, with their SimpleGenerators (add_simple_generator; each has deps, run(w, p) and
record(built), for these a head tuple and the continuation tuples that carry the targets): is_equal, inverse_or_zero, not_ / and_ /
or_ / select / _if, assert_bool (gadgets/arithmetic.rs, select.rs); split_le, split_le_base, le_sum, range_check, low_bits,
split_low_high (split_join.rs, split_base.rs, range_check.rs); extension targets - tuples of D targets - with
arithmetic_extension, mul / add / sub / div / div_add / inverse_extension, and base div / inverse through them
(arithmetic_extension.rs).  A BoolTarget is the target itself.
Not the GPU hot path: plain Python integers.
"""
import os
import re

import numpy as np

from . import native as N
from .dummy_circuit import BB_P, P as GL_P, bb_mul, bb_powers, gl_mul, gl_powers
from .prover import prove_with_retries

GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_POSEIDON, GATE_POSEIDON2_BABYBEAR = 0, 1, 2, 3, 4, 5  # gb_gate.kind


class CircuitConfig:
    """plonk/circuit_data.rs:63-93"""

    def __init__(self, field=N.GB_GOLDILOCKS, num_wires=135, num_routed_wires=80, num_constants=2, num_challenges=2,
                 max_quotient_degree_factor=8, rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28,
                 arity_bits=4, final_poly_bits=5, security_bits=100, fri_reduction_strategy=None, zero_knowledge=False):
        """fri_reduction_strategy: None = FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) (every stock
        configuration); ("fixed", [bits..]) or ("min_size", max_arity_bits or None) as in fri/reduction_strategies.rs:11-25.
        zero_knowledge: build() adds the blinding rows of CircuitBuilder::blind and the proofs are salted (seed=)"""
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def reduction_arity_bits(self, degree_bits):
        """FriConfig::fri_params' list for a circuit of 2^degree_bits rows (fri/mod.rs; None = let the library derive it)"""
        if self.fri_reduction_strategy is None:
            return None
        from . import fri_params
        return fri_params.reduction_arity_bits(self.fri_reduction_strategy, degree_bits, self.rate_bits, self.cap_height, self.num_query_rounds)

    @classmethod
    def standard_recursion_config_gl(cls, **kw):
        """circuit_data.rs:102-116"""
        return cls(**kw)

    @classmethod
    def standard_recursion_zk_config_gl(cls, **kw):
        """circuit_data.rs:175-180"""
        return cls.standard_recursion_config_gl(**dict(kw, zero_knowledge=True))

    @classmethod
    def standard_recursion_zk_config_bb(cls, **kw):
        """circuit_data.rs:181-186 (standard_recursion_config_bb is the narrow BabyBear config, :118-120)"""
        return cls.recursion_config_bb_narrow(**dict(kw, zero_knowledge=True))

    @classmethod
    def recursion_config_bb_narrow(cls, **kw):
        """circuit_data.rs:131-139"""
        d = dict(field=N.GB_BABYBEAR, num_wires=167, num_routed_wires=41, arity_bits=3, num_challenges=6)
        d.update(kw)
        return cls(**d)


class _Field:
    def __init__(self, field):
        gl = field == N.GB_GOLDILOCKS
        self.field, self.p = field, GL_P if gl else BB_P
        self.order_bits, self.ext_degree, self.hout = (64, 2, 4) if gl else (31, 4, 8)
        self.generator = 7 if gl else 31
        self.dtype = np.uint64 if gl else np.uint32
        self._two_adic = (1753635133440165772, 32) if gl else (0x1a427a41, 27)
        self._mul, self._powers = (gl_mul, gl_powers) if gl else (bb_mul, bb_powers)

    def two_adic_generator(self, bits):
        g, a = self._two_adic
        return pow(g, 1 << (a - bits), self.p)


# --------------------------------------------------------------------------------------------- gates
class Gate:
    kind, param, degree, num_constants, num_constraints = None, 0, 0, 0, 0
    num_ops = 1

    def __eq__(self, o):
        return self.id == o.id

    def __hash__(self):
        return hash(self.id)

    def generators(self, row, constants):
        return []

    def extra_constant_wires(self):
        return []


class NoopGate(Gate):
    """gates/noop.rs"""
    kind, id = GATE_NOOP, "NoopGate"
    num_wires = 0


class ConstantGate(Gate):
    """gates/constant.rs:22-140"""
    kind, degree = GATE_CONSTANT, 1

    def __init__(self, num_consts):
        self.param = self.num_constants = self.num_constraints = self.num_wires = num_consts
        self.id = "ConstantGate { num_consts: %d }" % num_consts

    def extra_constant_wires(self):
        return [(i, i) for i in range(self.param)]


class PublicInputGate(Gate):
    """gates/public_input.rs:24-110: wires 0..H are the public-inputs hash"""
    kind, degree = GATE_PUBLIC_INPUT, 1

    def __init__(self, hout):
        self.param = self.num_constraints = self.num_wires = hout
        self.id = "PublicInputGate<%d>" % hout


class ArithmeticGate(Gate):
    """gates/arithmetic_base.rs:27-190: num_ops x (out = c0 * m0 * m1 + c1 * addend) on wires 4i..4i+3"""
    kind, degree, num_constants = GATE_ARITHMETIC, 3, 2

    def __init__(self, num_ops):
        self.param = self.num_ops = self.num_constraints = num_ops
        self.num_wires = 4 * num_ops
        self.id = "ArithmeticGate { num_ops: %d }" % num_ops

    @classmethod
    def new_from_config(cls, cfg):
        return cls(cfg.num_routed_wires // 4)

    def generators(self, row, constants):
        return [_ArithmeticGenerator(row, constants[0], constants[1], i) for i in range(self.num_ops)]


class PoseidonGate(Gate):
    """gates/poseidon_goldilocks.rs:37-434: one width-12 permutation per row; wires 0..11 in, 12..23 out, 24 swap,
    25..28 delta, then the s-box inputs of full rounds 1..3, the 22 partial rounds and full rounds 4..7."""
    kind, degree = GATE_POSEIDON, 7
    WIRE_SWAP, START_DELTA, START_FULL_0 = 24, 25, 29
    START_PARTIAL = START_FULL_0 + 12 * 3
    START_FULL_1 = START_PARTIAL + 22
    num_wires = START_FULL_1 + 12 * 4            # 135
    num_constraints = 12 * 7 + 22 + 12 + 1 + 4   # 123
    id = "PoseidonGate(PhantomData<p3_goldilocks::goldilocks::Goldilocks>)<WIDTH=12>"

    def generators(self, row, constants):
        return [_PoseidonGenerator(row)]


class Poseidon2BabyBearGate(Gate):
    """gates/poseidon2_babybear.rs:48-147, 473-497: num_ops width-16 Poseidon2 permutations per row; per op 33 routed wires
    (16 in, 16 out, swap) for all ops first, then per op 133 non-routed wires (8 deltas, the s-box inputs of full rounds 1..3,
    of the 13 internal rounds and of full rounds 4..7).  recursion_config_bb_narrow (167 wires, 41 routed) fits one op."""
    kind, degree = GATE_POSEIDON2_BABYBEAR, 7
    ROUTED, NON_ROUTED = 33, 8 + 16 * 7 + 13

    def __init__(self, num_ops):
        self.param = self.num_ops = num_ops
        self.num_wires = (self.ROUTED + self.NON_ROUTED) * num_ops
        self.num_constraints = (1 + 8 + 16 * 7 + 13 + 16) * num_ops
        # Debug of the gate struct; the type name inside PhantomData is p3's (BabyBear is an alias of MontyField31<..>).  Only
        # the relative order of ids within one degree matters (circuit_builder.rs:1195-1196) and this is the only degree-7 gate.
        self.id = ("Poseidon2BabyBearGate { num_ops: %d, _phantom: PhantomData<p3_monty_31::monty_31::MontyField31<"
                   "p3_baby_bear::baby_bear::BabyBearParameters>> }<WIDTH=16>" % num_ops)

    @classmethod
    def new_from_config(cls, cfg):
        return cls(min(cfg.num_wires // (cls.ROUTED + cls.NON_ROUTED), cfg.num_routed_wires // cls.ROUTED))

    def generators(self, row, constants):
        return [_Poseidon2Generator(row, self.num_ops, op) for op in range(self.num_ops)]


# --------------------------------------------------------------------------------------------- targets, generators
def wire(row, column):
    return ("w", row, column)


class _ArithmeticGenerator:
    def __init__(self, row, c0, c1, i):
        self.row, self.c0, self.c1, self.i = row, c0, c1, i
        self.deps = [wire(row, 4 * i), wire(row, 4 * i + 1), wire(row, 4 * i + 2)]

    def record(self, built):
        return (N.GB_GEN_ARITHMETIC, built.row_gates[self.row], self.row, self.i)

    def run(self, w, p):
        m0, m1, a = (w.get(t) for t in self.deps)
        w.set(wire(self.row, 4 * self.i + 3), (m0 * m1 * self.c0 + a * self.c1) % p)


class _ConstantGenerator:
    """iop/generator.rs ConstantGenerator"""
    deps = []

    def __init__(self, row, constant_index, wire_index):
        self.row, self.constant_index, self.wire_index, self.constant = row, constant_index, wire_index, 0

    def record(self, built):
        return (N.GB_GEN_CONSTANT, built.row_gates[self.row], self.row, self.constant_index)

    def run(self, w, p):
        w.set(wire(self.row, self.wire_index), self.constant)


class _RandomValueGenerator:
    deps = []

    def __init__(self, target, blinding=False):
        self.target, self.blinding = target, blinding   # blinding: a cell of CircuitBuilder.blind's rows (filled from a seed)

    def record(self, built):
        return None   # its target is an input: random values are the host's (determinism contract)

    def run(self, w, p):
        if self.blinding and w.has(self.target):
            return    # the value of the seed's stream is there already (BuiltCircuit._run_generators)
        w.set(self.target, w.random())


class _CopyGenerator:
    """iop/generator.rs CopyGenerator: dst = src"""

    def __init__(self, src, dst):
        self.src, self.dst, self.deps = src, dst, [src]

    def record(self, built):
        return (N.GB_GEN_COPY, 0, built.target_index(self.src), built.target_index(self.dst))

    def run(self, w, p):
        w.set(self.dst, w.get(self.src))


class _GadgetGenerator:
    """A SimpleGenerator of a gadget: its operands are arbitrary targets.  record() is a head tuple (kind, parameter, number of
    targets, 0) and the GB_GEN_TARGETS continuation tuples that carry the targets two by two (include/goldibear_gpu.h)."""
    kind, param = None, 0

    def targets(self):
        raise NotImplementedError

    def record(self, built):
        return N.gadget_records(self.kind, self.param, [built.target_index(t) for t in self.targets()])


class _EqualityGenerator(_GadgetGenerator):
    """gadgets/arithmetic.rs:425-452"""
    kind = N.GB_GEN_EQUALITY

    def __init__(self, x, y, equal, inv):
        self.x, self.y, self.equal, self.inv, self.deps = x, y, equal, inv, [x, y]

    def targets(self):
        return [self.x, self.y, self.equal, self.inv]

    def run(self, w, p):
        x, y = w.get(self.x), w.get(self.y)
        w.set(self.equal, int(x == y))
        w.set(self.inv, pow((x - y) % p, p - 2, p) if x != y else 0)


class _NonzeroTestGenerator(_GadgetGenerator):
    """iop/generator.rs:400-428"""
    kind = N.GB_GEN_NONZERO_TEST

    def __init__(self, to_test, dummy):
        self.to_test, self.dummy, self.deps = to_test, dummy, [to_test]

    def targets(self):
        return [self.to_test, self.dummy]

    def run(self, w, p):
        v = w.get(self.to_test)
        w.set(self.dummy, 1 if v == 0 else pow(v, p - 2, p))


class _QuotientOrZeroGenerator(_GadgetGenerator):
    """gadgets/arithmetic.rs:487-511"""
    kind = N.GB_GEN_QUOTIENT_OR_ZERO

    def __init__(self, numerator, denominator, quotient):
        self.numerator, self.denominator, self.quotient, self.deps = numerator, denominator, quotient, [numerator, denominator]

    def targets(self):
        return [self.numerator, self.denominator, self.quotient]

    def run(self, w, p):
        num, den = w.get(self.numerator), w.get(self.denominator)
        w.set(self.quotient, 0 if den == 0 else num * pow(den, p - 2, p) % p)


class _QuotientExtensionGenerator(_GadgetGenerator):
    """gadgets/arithmetic_extension.rs:507-532; the operands are D-tuples of targets"""
    kind = N.GB_GEN_QUOTIENT_EXTENSION

    def __init__(self, field, numerator, denominator, quotient):
        self.field, self.numerator, self.denominator, self.quotient = field, list(numerator), list(denominator), list(quotient)
        self.deps = self.numerator + self.denominator

    def targets(self):
        return self.numerator + self.denominator + self.quotient

    def run(self, w, p):
        from .recursion_gates import Ext
        E = Ext(self.field)
        num, den = tuple(w.get(t) for t in self.numerator), tuple(w.get(t) for t in self.denominator)
        assert any(den), "Tried to invert zero"
        for t, v in zip(self.quotient, E.mul(num, E.inv(den))):
            w.set(t, v)


class _SplitGenerator(_GadgetGenerator):
    """gadgets/split_join.rs:67-97"""
    kind = N.GB_GEN_SPLIT

    def __init__(self, integer, bits):
        self.integer, self.bits, self.deps = integer, list(bits), [integer]

    def targets(self):
        return [self.integer] + self.bits

    def run(self, w, p):
        v = w.get(self.integer)
        for b in self.bits:
            w.set(b, v & 1)
            v >>= 1
        assert v == 0, "Integer too large to fit in given number of bits"


class _WireSplitGenerator(_GadgetGenerator):
    """gadgets/split_join.rs:118-161: `gates` are the rows of the BaseSumGate<2>s"""
    kind = N.GB_GEN_WIRE_SPLIT

    def __init__(self, integer, gates, num_limbs):
        self.integer, self.gates, self.num_limbs, self.deps = integer, list(gates), num_limbs, [integer]
        self.param = num_limbs

    def targets(self):
        return [self.integer] + [wire(row, 0) for row in self.gates]

    def run(self, w, p):
        v = w.get(self.integer)
        for row in self.gates:
            truncated = v
            if self.num_limbs < 64:
                truncated = v & ((1 << self.num_limbs) - 1)
                v >>= self.num_limbs
            else:
                v = 0
            w.set(wire(row, 0), truncated)
        assert v == 0, "Integer too large to fit in %d many `BaseSumGate`s" % len(self.gates)


class _LowHighGenerator(_GadgetGenerator):
    """gadgets/range_check.rs:89-115"""
    kind = N.GB_GEN_LOW_HIGH

    def __init__(self, integer, n_log, low, high):
        self.integer, self.n_log, self.low, self.high, self.deps = integer, n_log, low, high, [integer]
        self.param = n_log

    def targets(self):
        return [self.integer, self.low, self.high]

    def run(self, w, p):
        v = w.get(self.integer)
        w.set(self.low, v & ((1 << self.n_log) - 1))
        w.set(self.high, v >> self.n_log)


class _BaseSumGenerator(_GadgetGenerator):
    """gadgets/split_base.rs:84-116: the limbs are BoolTargets whatever the base"""
    kind = N.GB_GEN_BASE_SUM

    def __init__(self, row, limbs, base=2):
        self.row, self.limbs, self.base, self.deps = row, list(limbs), base, list(limbs)
        self.param = base

    def targets(self):
        return [wire(self.row, 0)] + self.limbs

    def run(self, w, p):
        acc = 0
        for t in reversed(self.limbs):
            limb = w.get(t)
            assert limb in (0, 1), "not a bool"
            acc = (acc * self.base + limb) % p
        w.set(wire(self.row, 0), acc)


class _PoseidonGenerator:
    """gates/poseidon_goldilocks.rs:436-531"""

    def __init__(self, row):
        self.row = row
        self.deps = [wire(row, c) for c in range(12)] + [wire(row, PoseidonGate.WIRE_SWAP)]

    def record(self, built):
        return (N.GB_GEN_POSEIDON, built.row_gates[self.row], self.row, 0)

    def run(self, w, p):
        G, row = PoseidonGate, self.row
        state = [w.get(wire(row, c)) for c in range(12)]
        swap = w.get(wire(row, G.WIRE_SWAP))
        assert swap in (0, 1)
        for i in range(4):
            w.set(wire(row, G.START_DELTA + i), swap * (state[i + 4] - state[i]) % p)
        if swap:
            state = state[4:8] + state[0:4] + state[8:]
        out = poseidon_gate_trace(state)
        for col, v in out.items():
            w.set(wire(row, col), v)


class _Poseidon2Generator:
    """gates/poseidon2_babybear.rs:536-676"""

    def __init__(self, row, num_ops, op):
        self.row, self.num_ops, self.op = row, num_ops, op
        self.deps = [wire(row, 33 * op + c) for c in range(16)] + [wire(row, 33 * op + 32)]

    def record(self, built):
        return (N.GB_GEN_POSEIDON2_BABYBEAR, built.row_gates[self.row], self.row, self.op)

    def run(self, w, p):
        row, op = self.row, self.op
        state = [w.get(t) for t in self.deps[:16]]
        swap = w.get(self.deps[16])
        assert swap in (0, 1)
        start_delta = self.num_ops * 33 + op * 133
        for i in range(8):
            w.set(wire(row, start_delta + i), swap * (state[i + 8] - state[i]) % p)
        if swap:
            state = state[8:] + state[:8]
        for col, v in poseidon2_gate_trace(state, start_delta + 8, 33 * op + 16).items():
            w.set(wire(row, col), v)


_POSEIDON_TABLES = None


def _poseidon_tables():
    """The Poseidon-12 tables of csrc/poseidon_constants.h (generated from hash/poseidon_goldilocks.rs by tools/gen_constants.py)."""
    global _POSEIDON_TABLES
    if _POSEIDON_TABLES is None:
        text = open(os.path.join(os.path.dirname(__file__), "csrc", "poseidon_constants.h")).read()
        tabs = {}
        for m in re.finditer(r"#define (?:GL_POSEIDON|BB_POSEIDON2)_(\w+)_LIST \\\n((?:[^\n]*\\\n)*[^\n]*)", text):
            tabs[m.group(1)] = [int(x.rstrip("uUlL"), 0) for x in re.findall(r"0x[0-9a-fA-F]+[uUlL]*|\d+[uUlL]*", m.group(2))]
        _POSEIDON_TABLES = tabs
    return _POSEIDON_TABLES


def poseidon_gate_trace(state):
    """The permutation exactly as PoseidonGenerator runs it (fast partial rounds), returning {wire column: value} for the
    s-box-input and output wires of the gate."""
    T, p, G = _poseidon_tables(), GL_P, PoseidonGate
    rc, circ, diag = T["ALL_ROUND_CONSTANTS"], T["MDS_CIRC"], T["MDS_DIAG"]
    out = {}

    def mds(s):
        return [(sum(s[(i + r) % 12] * circ[i] for i in range(12)) + s[r] * diag[r]) % p for r in range(12)]

    s = list(state)
    ctr = 0
    for r in range(4):
        s = [(s[i] + rc[12 * ctr + i]) % p for i in range(12)]
        if r:
            for i in range(12):
                out[G.START_FULL_0 + 12 * (r - 1) + i] = s[i]
        s = mds([pow(x, 7, p) for x in s])
        ctr += 1
    s = [(s[i] + T["FAST_PARTIAL_FIRST_ROUND_CONSTANT"][i]) % p for i in range(12)]
    init = T["FAST_PARTIAL_ROUND_INITIAL_MATRIX"]
    s = [s[0]] + [sum(s[r] * init[(r - 1) * 11 + (c - 1)] for r in range(1, 12)) % p for c in range(1, 12)]
    for r in range(22):
        out[G.START_PARTIAL + r] = s[0]
        s[0] = pow(s[0], 7, p)
        if r < 21:
            s[0] = (s[0] + T["FAST_PARTIAL_ROUND_CONSTANTS"][r]) % p
        d = (s[0] * (circ[0] + diag[0]) + sum(s[i] * T["FAST_PARTIAL_ROUND_W_HATS"][r * 11 + i - 1] for i in range(1, 12))) % p
        s = [d] + [(s[0] * T["FAST_PARTIAL_ROUND_VS"][r * 11 + i - 1] + s[i]) % p for i in range(1, 12)]
    ctr += 22
    for r in range(4):
        s = [(s[i] + rc[12 * ctr + i]) % p for i in range(12)]
        for i in range(12):
            out[G.START_FULL_1 + 12 * r + i] = s[i]
        s = mds([pow(x, 7, p) for x in s])
        ctr += 1
    for i in range(12):
        out[12 + i] = s[i]
    return out


def poseidon2_gate_trace(state, start_full_0, out0):
    """The width-16 Poseidon2 permutation as Poseidon2BabyBearGenerator runs it (gates/poseidon2_babybear.rs:608-676),
    returning {wire column: value} for the s-box-input wires (from start_full_0) and the outputs (from out0)."""
    T, p = _poseidon_tables(), BB_P
    ext, internal = T["EXTERNAL_CONSTANTS"], T["INTERNAL_CONSTANTS"]
    shifts = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]
    out = {}

    def external(s):
        s = list(s)
        for i in range(0, 16, 4):
            x0, x1, x2, x3 = s[i:i + 4]
            s[i:i + 4] = [2 * x0 + 3 * x1 + x2 + x3, x0 + 2 * x1 + 3 * x2 + x3, x0 + x1 + 2 * x2 + 3 * x3, 3 * x0 + x1 + x2 + 2 * x3]
        sums = [sum(s[k::4]) for k in range(4)]
        return [(s[i] + sums[i % 4]) % p for i in range(16)]

    s = external(state)
    for r in range(4):
        s = [(s[i] + ext[16 * r + i]) % p for i in range(16)]
        if r:
            for i in range(16):
                out[start_full_0 + 16 * (r - 1) + i] = s[i]
        s = external([pow(x, 7, p) for x in s])
    start_partial = start_full_0 + 48
    for r in range(13):
        s[0] = (s[0] + internal[r]) % p
        out[start_partial + r] = s[0]
        s[0] = pow(s[0], 7, p)
        s = [x * 943718400 % p for x in s]
        part = sum(s[1:]) % p
        full = (part + s[0]) % p
        s = [(part - s[0]) % p] + [(full + (s[i + 1] << shifts[i])) % p for i in range(15)]
    start_full_1 = start_partial + 13
    for r in range(4, 8):
        s = [(s[i] + ext[16 * r + i]) % p for i in range(16)]
        for i in range(16):
            out[start_full_1 + 16 * (r - 4) + i] = s[i]
        s = external([pow(x, 7, p) for x in s])
    for i in range(16):
        out[out0 + i] = s[i]
    return out


class PartialWitness:
    """iop/witness.rs PartialWitness: target -> value"""

    def __init__(self):
        self.values = {}

    def set_target(self, target, value):
        self.values[target] = int(value)


class _PartitionWitness:
    """iop/witness.rs:288-357: one value per copy class (representative)"""

    def __init__(self, find, p, rng):
        self.find, self.p, self.rng, self.v = find, p, rng, {}

    def get(self, t):
        return self.v[self.find(t)]

    def has(self, t):
        return self.find(t) in self.v

    def set(self, t, value):
        r = self.find(t)
        value %= self.p
        if r in self.v and self.v[r] != value:
            raise ValueError("Partition containing %r was set twice with different values: %d != %d" % (t, self.v[r], value))
        self.v[r] = value

    def random(self):
        return int(self.rng.integers(0, self.p, dtype=np.uint64))


# --------------------------------------------------------------------------------------------- builder
class CircuitBuilder:
    """plonk/circuit_builder.rs:142-1409 (no lookups; base arithmetic goes through ArithmeticGate, use_base_arithmetic_gate = true
    as in every stock configuration).  Under a zero_knowledge config build() runs blind() before it pads."""

    def __init__(self, config):
        self.config, self.F = config, _Field(config.field)
        c = config
        # check_fri_security_bits (circuit_builder.rs:266-290)
        ext_bits = self.F.order_bits * self.F.ext_degree
        if min(ext_bits, c.num_query_rounds * c.rate_bits + c.proof_of_work_bits) < c.security_bits:
            raise ValueError("FRI params fall short of target security")
        self.gates, self.gate_instances = set(), []   # instances: [gate, constants]
        self.public_inputs, self.virtual_target_index = [], 0
        self.copy_constraints, self.generators = [], []
        self.constants_to_targets, self.targets_to_constants = {}, {}
        self.base_arithmetic_results, self.current_slots, self.constant_generators = {}, {}, []
        self.arithmetic_results = {}   # of arithmetic_extension
        self.random_wire = None

    # ---- targets
    def add_virtual_target(self):
        self.virtual_target_index += 1
        return ("v", self.virtual_target_index - 1)

    def add_virtual_targets(self, n):
        return [self.add_virtual_target() for _ in range(n)]

    def add_virtual_public_input(self):
        t = self.add_virtual_target()
        self.register_public_input(t)
        return t

    def register_public_input(self, t):
        self.public_inputs.append(t)

    def register_public_inputs(self, ts):
        for t in ts:
            self.register_public_input(t)

    def num_gates(self):
        return len(self.gate_instances)

    def is_routable(self, t):
        return t[0] == "v" or t[2] < self.config.num_routed_wires

    def generate_copy(self, src, dst):
        """gadgets/arithmetic.rs generate_copy: a CopyGenerator, no copy constraint"""
        self.generators.append(_CopyGenerator(src, dst))

    def connect(self, x, y):
        if not (self.is_routable(x) and self.is_routable(y)):
            raise ValueError("Tried to route a wire that isn't routable")
        self.copy_constraints.append((x, y))

    def assert_zero(self, x):
        self.connect(x, self.zero())

    def assert_one(self, x):
        self.connect(x, self.one())

    def constant(self, c):
        c = int(c) % self.F.p
        t = self.constants_to_targets.get(c)
        if t is None:
            t = self.add_virtual_target()
            self.constants_to_targets[c] = t
            self.targets_to_constants[t] = c
        return t

    def zero(self):
        return self.constant(0)

    def one(self):
        return self.constant(1)

    def two(self):
        return self.constant(2)

    def neg_one(self):
        return self.constant(self.F.p - 1)

    def target_as_constant(self, t):
        return self.targets_to_constants.get(t)

    # ---- gates
    def add_gate(self, gate, constants=()):
        """circuit_builder.rs:478-514"""
        cfg = self.config
        if gate.num_wires > cfg.num_wires or gate.num_constants > cfg.num_constants:
            raise ValueError("%s does not fit the CircuitConfig" % gate.id)
        consts = list(constants) + [0] * (gate.num_constants - len(constants))
        row = len(self.gate_instances)
        self.constant_generators += [_ConstantGenerator(row, ci, wi) for ci, wi in gate.extra_constant_wires()]
        self.gates.add(gate)
        self.gate_instances.append([gate, consts])
        return row

    def add_gate_to_gate_set(self, gate):
        self.gates.add(gate)

    def find_slot(self, gate, params, constants):
        """circuit_builder.rs:821-852"""
        slots = self.current_slots.setdefault(gate.id, {})
        key = tuple(params)
        if key in slots:
            gate_idx, slot_idx = slots[key]
        else:
            gate_idx, slot_idx = self.add_gate(gate, constants), 0
        if slot_idx == gate.num_ops - 1:
            slots.pop(key, None)
        else:
            slots[key] = (gate_idx, slot_idx + 1)
        return gate_idx, slot_idx

    # ---- gadgets/arithmetic.rs
    def arithmetic(self, const_0, const_1, m0, m1, addend):
        p = self.F.p
        const_0, const_1 = const_0 % p, const_1 % p
        r = self._arithmetic_special_cases(const_0, const_1, m0, m1, addend)
        if r is not None:
            return r
        op = (const_0, const_1, m0, m1, addend)
        if op in self.base_arithmetic_results:
            return self.base_arithmetic_results[op]
        gate = ArithmeticGate.new_from_config(self.config)
        row, i = self.find_slot(gate, (const_0, const_1), (const_0, const_1))
        self.connect(m0, wire(row, 4 * i))
        self.connect(m1, wire(row, 4 * i + 1))
        self.connect(addend, wire(row, 4 * i + 2))
        out = wire(row, 4 * i + 3)
        self.base_arithmetic_results[op] = out
        return out

    def _arithmetic_special_cases(self, c0, c1, m0, m1, addend):
        """gadgets/arithmetic.rs:112-165"""
        p = self.F.p
        zero = self.zero()
        k0, k1, ka = self.target_as_constant(m0), self.target_as_constant(m1), self.target_as_constant(addend)
        first_zero = c0 == 0 or m0 == zero or m1 == zero
        second_zero = c1 == 0 or addend == zero
        first_const = 0 if first_zero else (k0 * k1 * c0 % p if k0 is not None and k1 is not None else None)
        second_const = 0 if second_zero else (ka * c1 % p if ka is not None else None)
        if first_const is not None and second_const is not None:
            return self.constant((first_const + second_const) % p)
        if first_zero and c1 == 1:
            return addend
        if second_zero:
            if k0 is not None and k0 * c0 % p == 1:
                return m1
            if k1 is not None and k1 * c0 % p == 1:
                return m0
        return None

    def mul(self, x, y):
        return self.arithmetic(1, 0, x, y, x)

    def add(self, x, y):
        return self.arithmetic(1, 1, x, self.one(), y)

    def sub(self, x, y):
        return self.arithmetic(1, self.F.p - 1, x, self.one(), y)

    def mul_add(self, x, y, z):
        return self.arithmetic(1, 1, x, y, z)

    def mul_sub(self, x, y, z):
        return self.arithmetic(1, self.F.p - 1, x, y, z)

    def neg(self, x):
        return self.mul(x, self.neg_one())

    def square(self, x):
        return self.mul(x, x)

    def mul_const(self, c, x):
        return self.mul(self.constant(c), x)

    def add_const(self, x, c):
        return self.add(x, self.constant(c))

    def mul_many(self, terms):
        acc = self.one()
        for t in terms:
            acc = self.mul(acc, t)
        return acc

    def mul_const_add(self, c, x, y):
        return self.mul_add(self.constant(c), x, y)

    def add_many(self, terms):
        """gadgets/arithmetic.rs:204-234: ADD_MANY_THRESHOLD = 23 addends fill one operation of an AddManyGate"""
        from .recursion_gates import AddManyGate
        terms, threshold = list(terms), 23
        if len(terms) == threshold:
            gate = AddManyGate.new_from_config(self.config, threshold)
            row, i = self.find_slot(gate, (), ())
            for k, t in enumerate(terms):
                self.connect(t, wire(row, (gate.num_addends + 1) * i + k))
            return wire(row, (gate.num_addends + 1) * i + gate.num_addends)
        if len(terms) < threshold:
            acc = self.zero()
            for t in terms:
                acc = self.add(acc, t)
            return acc
        return self.add_many([self.add_many(terms[k:k + threshold]) for k in range(0, len(terms), threshold)])

    # ---- generators of gadgets.  A BoolTarget is the target itself: new_unsafe adds nothing to the circuit.
    def add_simple_generator(self, generator):
        """circuit_builder.rs add_simple_generator: an object with deps, run(w, p) and record(built)"""
        self.generators.append(generator)

    def add_virtual_bool_target_unsafe(self):
        return self.add_virtual_target()

    def add_virtual_bool_target_safe(self):
        b = self.add_virtual_target()
        self.assert_bool(b)
        return b

    def inverse_or_zero(self, x):
        """gadgets/arithmetic.rs:366-376"""
        inv, one = self.add_virtual_target(), self.one()
        self.add_simple_generator(_QuotientOrZeroGenerator(one, x, inv))
        return self.mul(one, inv)

    def not_(self, b):
        return self.sub(self.one(), b)

    def and_(self, b1, b2):
        return self.mul(b1, b2)

    def or_(self, b1, b2):
        res_minus_b2 = self.arithmetic(self.F.p - 1, 1, b1, b2, b1)
        return self.add(res_minus_b2, b2)

    def _if(self, b, x, y):
        not_b = self.not_(b)
        maybe_x = self.mul(b, x)
        return self.mul_add(not_b, y, maybe_x)

    def select(self, b, x, y):
        """gadgets/select.rs:36-39"""
        tmp = self.mul_sub(b, y, y)
        return self.mul_sub(b, x, tmp)

    def is_equal(self, x, y):
        """gadgets/arithmetic.rs:404-422"""
        zero = self.zero()
        equal = self.add_virtual_bool_target_unsafe()
        not_equal = self.not_(equal)
        inv = self.add_virtual_target()
        self.add_simple_generator(_EqualityGenerator(x, y, equal, inv))
        diff = self.sub(x, y)
        not_equal_check = self.mul(equal, diff)
        diff_normalized = self.mul(diff, inv)
        equal_check = self.sub(diff_normalized, not_equal)
        self.connect(not_equal_check, zero)
        self.connect(equal_check, zero)
        return equal

    def assert_bool(self, b):
        """gadgets/range_check.rs:82-86"""
        self.connect(self.mul_sub(b, b, b), self.zero())

    # ---- gadgets/split_join.rs, split_base.rs, range_check.rs
    def _base_sum_gate_from_config(self, base=2):
        """BaseSumGate::<B>::new_from_config (gates/base_sum.rs:37-41)"""
        from .recursion_gates import BaseSumGate
        limbs, cur = 0, 1   # log_floor(ORDER - 1, B)
        while cur * base <= min(self.F.p - 1, (1 << 64) - 1):
            limbs, cur = limbs + 1, cur * base
        return BaseSumGate(min(limbs, self.config.num_routed_wires - 1), base)

    def split_le(self, integer, num_bits):
        """gadgets/split_join.rs:27-64 -> num_bits little-endian BoolTargets, limb wires of k BaseSumGate<2> rows"""
        if num_bits == 0:
            return []
        gate = self._base_sum_gate_from_config()
        k = -(-num_bits // gate.num_limbs)
        rows = [self.add_gate(gate) for _ in range(k)]
        bits = [wire(row, 1 + i) for row in rows for i in range(gate.num_limbs)]
        for b in bits[num_bits:]:
            self.assert_zero(b)
        bits = bits[:num_bits]
        acc = self.zero()
        for row in reversed(rows):
            acc = self.mul_const_add(pow(2, gate.num_limbs, self.F.p), acc, wire(row, 0))
        self.connect(acc, integer)
        self.add_simple_generator(_WireSplitGenerator(integer, rows, gate.num_limbs))
        return bits

    def split_le_base(self, x, num_limbs, base):
        """gadgets/split_base.rs:23-30"""
        from .recursion_gates import BaseSumGate
        row = self.add_gate(BaseSumGate(num_limbs, base))
        self.connect(x, wire(row, 0))
        return [wire(row, 1 + i) for i in range(num_limbs)]

    def le_sum(self, bits):
        """gadgets/split_base.rs:39-81: arithmetic operations while they fit one ArithmeticGate, else a BaseSumGate<2> row whose
        limbs are connected to the bits and whose sum a BaseSumGenerator sets"""
        bits = list(bits)
        num_bits = len(bits)
        if num_bits > (self.F.p).bit_length() - 1:
            raise ValueError("%d bits may overflow the field" % num_bits)
        if num_bits == 0:
            return self.zero()
        if num_bits - 1 <= ArithmeticGate.new_from_config(self.config).num_ops:
            two = self.two()
            total = bits[-1]
            for bit in reversed(bits[:-1]):
                total = self.mul_add(two, total, bit)
            return total
        if 1 + num_bits > self.config.num_routed_wires:
            raise ValueError("Not enough routed wires.")
        gate = self._base_sum_gate_from_config()
        row = self.add_gate(gate)
        for i, bit in enumerate(bits):
            self.connect(bit, wire(row, 1 + i))
        for i in range(num_bits, gate.num_limbs):
            self.assert_zero(wire(row, 1 + i))
        self.add_simple_generator(_BaseSumGenerator(row, bits, 2))
        return wire(row, 0)

    def range_check(self, x, n_log):
        self.split_le(x, n_log)

    def low_bits(self, x, num_low_bits, are_noncanonical_indices_ok, num_bits):
        """gadgets/range_check.rs:28-57; F::ORDER = 2^EXP0 - 2^EXP1 + 1"""
        exp0, exp1 = (64, 32) if self.config.field == N.GB_GOLDILOCKS else (31, 27)
        assert num_bits <= exp0
        res = self.split_le(x, num_bits)
        if not are_noncanonical_indices_ok:
            one = self.one()
            lo_sum, hi_sum = self.add_many(res[:exp1]), self.add_many(res[exp1:])
            hi_shifted = self.add_const(hi_sum, exp0 - exp1)
            y = self.inverse_or_zero(hi_shifted)
            maybe_0 = self.arithmetic(1, self.F.p - 1, hi_shifted, y, one)
            self.assert_zero(self.mul(maybe_0, lo_sum))
        return res[:num_low_bits]

    def split_low_high(self, x, n_log, num_bits):
        """gadgets/range_check.rs:61-80"""
        low, high = self.add_virtual_target(), self.add_virtual_target()
        self.add_simple_generator(_LowHighGenerator(x, n_log, low, high))
        self.range_check(low, n_log)
        self.range_check(high, num_bits - n_log)
        pow2 = self.constant(1 << n_log)
        self.connect(x, self.mul_add(high, pow2, low))
        return low, high

    # ---- gadgets/arithmetic_extension.rs: an ExtensionTarget is a tuple of D targets
    def add_virtual_extension_target(self):
        return tuple(self.add_virtual_targets(self.F.ext_degree))

    def constant_extension(self, c):
        return tuple(self.constant(x) for x in c)

    def zero_extension(self):
        return self.constant_extension((0,) * self.F.ext_degree)

    def one_extension(self):
        return self.constant_extension((1,) + (0,) * (self.F.ext_degree - 1))

    def convert_to_ext(self, t):
        return (t,) + (self.zero(),) * (self.F.ext_degree - 1)

    def connect_extension(self, src, dst):
        for s, d in zip(src, dst):
            self.connect(s, d)

    def target_as_constant_ext(self, t):
        c = tuple(self.target_as_constant(x) for x in t)
        return None if None in c else c

    def arithmetic_extension(self, const_0, const_1, m0, m1, addend):
        """gadgets/arithmetic_extension.rs:27-113: a slot of an ArithmeticExtensionGate, or of a MulExtensionGate for a zero addend"""
        from .recursion_gates import ArithmeticExtensionGate, Ext, MulExtensionGate
        p, E = self.F.p, Ext(self.config.field)
        D = E.D
        const_0, const_1 = const_0 % p, const_1 % p
        m0, m1, addend = tuple(m0), tuple(m1), tuple(addend)
        r = self._arithmetic_extension_special_cases(E, const_0, const_1, m0, m1, addend)
        if r is not None:
            return r
        op = (const_0, const_1, m0, m1, addend)
        if op in self.arithmetic_results:
            return self.arithmetic_results[op]
        if self.target_as_constant_ext(addend) == E.zero:
            gate = MulExtensionGate.new_from_config(self.config)
            row, i = self.find_slot(gate, (const_0,), (const_0,))
            operands = (m0, m1)
        else:
            gate = ArithmeticExtensionGate.new_from_config(self.config)
            row, i = self.find_slot(gate, (const_0, const_1), (const_0, const_1))
            operands = (m0, m1, addend)
        base = gate.OPERANDS * D * i
        for j, operand in enumerate(operands):
            self.connect_extension(operand, tuple(wire(row, base + j * D + k) for k in range(D)))
        out = tuple(wire(row, base + (gate.OPERANDS - 1) * D + k) for k in range(D))
        self.arithmetic_results[op] = out
        return out

    def _arithmetic_extension_special_cases(self, E, c0, c1, m0, m1, addend):
        """gadgets/arithmetic_extension.rs:118-171"""
        zero = self.zero_extension()
        k0, k1, ka = self.target_as_constant_ext(m0), self.target_as_constant_ext(m1), self.target_as_constant_ext(addend)
        first_zero = c0 == 0 or m0 == zero or m1 == zero
        second_zero = c1 == 0 or addend == zero
        first_const = E.zero if first_zero else (E.scale(E.mul(k0, k1), c0) if k0 is not None and k1 is not None else None)
        second_const = E.zero if second_zero else (E.scale(ka, c1) if ka is not None else None)
        if first_const is not None and second_const is not None:
            return self.constant_extension(E.add(first_const, second_const))
        if first_zero and c1 == 1:
            return addend
        if second_zero:
            if k0 is not None and E.scale(k0, c0) == E.one:
                return m1
            if k1 is not None and E.scale(k1, c0) == E.one:
                return m0
        return None

    def add_extension(self, a, b):
        return self.arithmetic_extension(1, 1, self.one_extension(), a, b)

    def sub_extension(self, a, b):
        return self.arithmetic_extension(1, self.F.p - 1, self.one_extension(), a, b)

    def mul_extension(self, a, b):
        return self.arithmetic_extension(1, 0, a, b, self.zero_extension())

    def mul_add_extension(self, a, b, c):
        return self.arithmetic_extension(1, 1, a, b, c)

    def div_add_extension(self, x, y, z):
        """gadgets/arithmetic_extension.rs:479-498: x / y + z"""
        inv, one = self.add_virtual_extension_target(), self.one_extension()
        self.add_simple_generator(_QuotientExtensionGenerator(self.config.field, one, y, inv))
        self.connect_extension(self.mul_extension(y, inv), one)
        return self.mul_add_extension(x, inv, z)

    def div_extension(self, x, y):
        return self.div_add_extension(x, y, self.zero_extension())

    def inverse_extension(self, x):
        return self.div_extension(self.one_extension(), x)

    def div(self, x, y):
        """gadgets/arithmetic.rs:353-357"""
        return self.div_extension(self.convert_to_ext(x), self.convert_to_ext(y))[0]

    def inverse(self, x):
        return self.inverse_extension(self.convert_to_ext(x))[0]

    # ---- hashing (plonk/config.rs:135-166, hash/poseidon_goldilocks.rs:1116-1143)
    def permute(self, state):
        if self.config.field != N.GB_GOLDILOCKS:
            # hash/poseidon2_babybear.rs:183-213: a slot of a Poseidon2BabyBearGate
            gate = Poseidon2BabyBearGate.new_from_config(self.config)
            if gate.num_ops != 1:
                raise NotImplementedError("Poseidon2BabyBearGate with several operations per row (complete_wires) is not restated")
            row, op = self.find_slot(gate, (), ())
            self.connect(self.zero(), wire(row, 33 * op + 32))
            for i in range(16):
                self.connect(state[i], wire(row, 33 * op + i))
            return [wire(row, 33 * op + 16 + i) for i in range(16)]
        row = self.add_gate(PoseidonGate())
        self.connect(self.zero(), wire(row, PoseidonGate.WIRE_SWAP))   # swap = _false()
        for i in range(12):
            self.connect(state[i], wire(row, i))
        return [wire(row, 12 + i) for i in range(12)]

    def hash_n_to_hash_no_pad(self, inputs):
        width = 12 if self.config.field == N.GB_GOLDILOCKS else 16
        state = [self.zero()] * width
        for c in range(0, len(inputs), 8):
            chunk = inputs[c:c + 8]
            state[:len(chunk)] = chunk
            state = self.permute(state)
        return state[:self.F.hout]

    # ---- build (circuit_builder.rs:1110-1378)
    def build(self, ctx=None, wiring="host"):
        """wiring: "host" - the forest and the sigma columns by the loops below (_forest, _sigma); "device" - by
        wiring.sigma_polys on `ctx` (gb_wiring_sigmas): the same sigma values, and a representative map whose representatives
        are the lowest target of every class, which the built circuit then uses throughout"""
        if wiring not in ("host", "device"):
            raise ValueError("wiring is \"host\" or \"device\"")
        if wiring == "device" and ctx is None:
            raise ValueError("wiring=\"device\" needs a GPU context")
        cfg, F = self.config, self.F
        p = F.p
        pi_hash = self.hash_n_to_hash_no_pad(list(self.public_inputs))
        pi_gate = self.add_gate(PublicInputGate(F.hout))
        for i, h in enumerate(pi_hash):
            self.connect(h, wire(pi_gate, i))
        # randomize_unused_pi_wires (:1064-1080)
        for w in range(F.hout, cfg.num_wires):
            if w == cfg.num_wires - 1:
                self.random_wire = (pi_gate, w)
            self.generators.append(_RandomValueGenerator(wire(pi_gate, w)))
        while len(self.constants_to_targets) > len(self.constant_generators):
            self.add_gate(ConstantGate(cfg.num_constants))
        for (c, t), gen in zip(sorted(self.constants_to_targets.items()), self.constant_generators):
            self.gate_instances[gen.row][1][gen.constant_index] = c
            self.connect(wire(gen.row, gen.wire_index), t)
            gen.constant = c
            self.generators.append(gen)
        if getattr(cfg, "zero_knowledge", False):                          # blind_and_pad (:924-932)
            self.blind()
        while len(self.gate_instances) & (len(self.gate_instances) - 1):
            self.add_gate(NoopGate())
        degree = len(self.gate_instances)
        degree_bits = degree.bit_length() - 1
        if F.order_bits * F.ext_degree - degree_bits < cfg.security_bits:
            raise ValueError("The degree of the extension is not enough for the soundness of the evaluation point")
        if (F.order_bits - degree_bits) * cfg.num_challenges < cfg.security_bits:
            raise ValueError("The number of challenges is not sufficient for the soundness of permutation argument and "
                             "combining constraints")
        gates = sorted(self.gates, key=lambda g: (g.degree, g.id))
        sel_cols, selector_indices, groups = selector_polynomials(gates, self.gate_instances, cfg.max_quotient_degree_factor + 1, p)
        max_constants = max(g.num_constants for g in gates)
        consts = np.zeros((max_constants, degree), dtype=F.dtype)
        for row, (_, kc) in enumerate(self.gate_instances):
            for i, c in enumerate(kc):
                consts[i, row] = c
        k_is = np.array([pow(F.generator, i, p) for i in range(cfg.num_routed_wires)], dtype=F.dtype)
        subgroup = F._powers(F.two_adic_generator(degree_bits), degree)
        representative_map = None
        if wiring == "device":
            sigma, representative_map, find = self._wiring_on_device(ctx, degree_bits, k_is)
        else:
            find = self._forest()
            sigma = self._sigma(find, degree, k_is, subgroup)
        constants_sigmas = np.concatenate([np.array(sel_cols, dtype=F.dtype).reshape(len(groups), degree), consts, sigma])
        # gate generators, dropping the unused operations of partly filled gates (:1252-1270)
        incomplete = {}
        for slots in self.current_slots.values():
            for gate_idx, slot_idx in slots.values():
                incomplete[gate_idx] = slot_idx
        gens = list(self.generators)
        for row, (g, kc) in enumerate(self.gate_instances):
            gg = g.generators(row, kc)
            if row in incomplete:
                gg = gg[:incomplete[row]]
            gens += gg
        # the constraint programs of the gate set's program gates (gate_program.ProgramGate), numbered in sorted order
        # (a program gate's `param` is its index here; the gate object may serve other builders and is left as it is)
        programs, params = [], []
        for g in gates:
            if getattr(g, "program", None) is not None:
                params.append(len(programs))
                programs.append(g.program)
            else:
                params.append(g.param)
        # the generator programs of the generators (generator_program.ProgramGenerator), the distinct ones numbered in the order of
        # the generators; a program generator reads the constants of its row: the built circuit holds a copy bound to them
        # (the generator object may serve other builders, or this one built again, and is left as it is)
        generator_programs, seen = [], set()
        for i, gen in enumerate(gens):
            prog = getattr(gen, "generator_program", None)
            if prog is None:
                continue
            if tuple(prog.words) not in seen:
                seen.add(tuple(prog.words))
                generator_programs.append(prog)
            if gen.row is not None:
                kc = [int(c) for c in self.gate_instances[gen.row][1]]
                gens[i] = gen.bound_to((kc + [0] * prog.num_constants)[:prog.num_constants])
        gate_table = [(g.kind, params[i], selector_indices[i], groups[selector_indices[i]][0], groups[selector_indices[i]][1],
                       getattr(g, "param2", 0), getattr(g, "param3", 0)) for i, g in enumerate(gates)]
        return BuiltCircuit(ctx, cfg, F, degree_bits, constants_sigmas, k_is, gate_table, len(groups), max_constants, gens, find,
                            list(self.public_inputs), self.random_wire, [g.id for g in gates],
                            sorted({t for ab in self.copy_constraints for t in ab if t[0] == "w"}), programs=programs or None,
                            copy_targets=sorted({t for ab in self.copy_constraints for t in ab}),
                            num_virtual_targets=self.virtual_target_index,
                            row_gates=[gates.index(g) for g, _ in self.gate_instances], generator_programs=generator_programs,
                            representative_map=representative_map)

    # ---- zero-knowledge blinding (circuit_builder.rs:875-980)
    def fri_reduction_arity_bits(self, degree_bits):
        """self.fri_params(degree_bits).reduction_arity_bits (:855-859; hiding does not enter the list)"""
        from . import fri_params
        c = self.config
        strategy = c.fri_reduction_strategy or ("constant", c.arity_bits, c.final_poly_bits)
        return fri_params.reduction_arity_bits(strategy, degree_bits, c.rate_bits, c.cap_height, c.num_query_rounds)

    def num_blinding_gates(self, degree_estimate):
        """:879-898 -> (regular_poly_openings, z_openings): the polynomial values one opening reveals, for a degree estimate"""
        D = self.F.ext_degree
        arities = [1 << b for b in self.fri_reduction_arity_bits(degree_estimate.bit_length() - 1)]
        total_fri_folding_points = sum(a - 1 for a in arities)
        product = 1
        for a in arities:
            product *= a
        final_poly_coeffs = degree_estimate // product
        fri_openings = self.config.num_query_rounds * (1 + D * total_fri_folding_points + D * final_poly_coeffs)
        return D + fri_openings, 2 * D + fri_openings   # zeta; zeta and g zeta

    def blinding_counts(self):
        """:903-922: the counts for the smallest power of two that holds the gates and their own blinding rows"""
        num_gates = len(self.gate_instances)
        degree_estimate = 1 << max(0, (num_gates - 1).bit_length())   # 1 << log2_ceil(num_gates)
        while True:
            regular_poly_openings, z_openings = self.num_blinding_gates(degree_estimate)
            # one random element per opened value; Z takes two rows each, a copy between them
            if num_gates + regular_poly_openings + 2 * z_openings <= degree_estimate:
                return regular_poly_openings, z_openings
            degree_estimate *= 2

    def blind(self):
        """:934-980: `regular` NoopGate rows with a random value on every wire, then `z` pairs of NoopGate rows with a random value
        on every routed wire of the first and generate_copy to the same wire of the second (a CopyGenerator, as in the
        reference: no copy constraint, so the sigma columns are those of the unblinded circuit's wiring)"""
        regular_poly_openings, z_openings = self.blinding_counts()
        cfg = self.config
        for _ in range(regular_poly_openings):
            row = self.add_gate(NoopGate())
            for w in range(cfg.num_wires):
                self.generators.append(_RandomValueGenerator(wire(row, w), blinding=True))
        for _ in range(z_openings):
            gate_1 = self.add_gate(NoopGate())
            gate_2 = self.add_gate(NoopGate())
            for w in range(cfg.num_routed_wires):
                self.generators.append(_RandomValueGenerator(wire(gate_1, w), blinding=True))
                self.generate_copy(wire(gate_1, w), wire(gate_2, w))
        return regular_poly_openings, z_openings

    def _wiring_on_device(self, ctx, degree_bits, k_is):
        """the copy constraints as pairs of Target::index -> (sigma, representative map, find) from wiring.sigma_polys; `find`
        reads the map, so the Python witness path places a class's value where the map says its representative is"""
        from .wiring import sigma_polys
        nw, cells = self.config.num_wires, self.config.num_wires << degree_bits

        def index(t):
            return t[1] * nw + t[2] if t[0] == "w" else cells + t[1]

        pairs = np.array([(index(a), index(b)) for a, b in self.copy_constraints], dtype=np.uint64).reshape(-1, 2)
        sigma, rep, _ = sigma_polys(ctx, self.config.field, degree_bits, nw, self.config.num_routed_wires, k_is, pairs,
                                    cells + self.virtual_target_index)

        def find(t):
            r = int(rep[index(t)])
            return wire(r // nw, r % nw) if r < cells else ("v", r - cells)

        return sigma, rep, find

    def _forest(self):
        """Disjoint sets over the targets that appear in copy constraints (plonk/permutation_argument.rs:13-101)."""
        parent = {}

        def find(t):
            root = t
            while parent.get(root, root) != root:
                root = parent[root]
            while parent.get(t, t) != t:
                parent[t], t = root, parent[t]
            return root

        for a, b in self.copy_constraints:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[rb] = ra
        return find

    def _sigma(self, find, degree, k_is, subgroup):
        """sigma_vecs (:1005-1040): identity, then every copy class's routed wires, in (row, column) order, point to the next."""
        F, nr = self.F, self.config.num_routed_wires
        sig = np.empty((nr, degree), dtype=F.dtype)
        for j in range(nr):
            sig[j] = F._mul(subgroup, k_is[j])
        classes = {}
        touched = set()
        for a, b in self.copy_constraints:
            touched.add(a)
            touched.add(b)
        for t in touched:
            if t[0] == "w" and t[2] < nr:
                classes.setdefault(find(t), []).append((t[1], t[2]))
        for members in classes.values():
            members.sort()
            for i, (row, col) in enumerate(members):
                nrow, ncol = members[(i + 1) % len(members)]
                sig[col, row] = int(k_is[ncol]) * int(subgroup[nrow]) % F.p
        return sig


def selector_polynomials(gates, instances, max_degree, p):
    """gates/selectors.rs:125-209 -> (selector columns, selector_indices, groups as (start, end))"""
    n, num_gates = len(instances), len(gates)
    index = {g.id: i for i, g in enumerate(gates)}
    max_gate_degree = gates[-1].degree
    if max_gate_degree + num_gates - 1 <= max_degree:
        return [[index[g.id] for g, _ in instances]], [0] * num_gates, [(0, num_gates)]
    if max_gate_degree >= max_degree:
        raise ValueError("%s has too high degree. Consider increasing `quotient_degree_factor`." % gates[-1].id)
    groups, start = [], 0
    while start < num_gates:
        size = 0
        while start + size < num_gates and size + gates[start + size].degree < max_degree:
            size += 1
        groups.append((start, start + size))
        start += size
    group = [next(k for k, (a, b) in enumerate(groups) if a <= i < b) for i in range(num_gates)]
    unused = 0xFFFFFFFF % p
    cols = [[unused] * n for _ in groups]
    for j, (g, _) in enumerate(instances):
        i = index[g.id]
        cols[group[i]][j] = i
    return cols, group, groups


class BuiltCircuit:
    """CircuitData (plonk/circuit_data.rs:153-300) for a built circuit: prove(PartialWitness) / verify(proof)."""

    def __init__(self, ctx, cfg, F, degree_bits, constants_sigmas, k_is, gate_table, num_selectors, max_constants, generators, find,
                 public_inputs, random_wire, gate_ids, copy_wires, programs=None, copy_targets=(), num_virtual_targets=0, row_gates=(),
                 generator_programs=(), representative_map=None):
        self.config, self.F, self.degree_bits, self.programs = cfg, F, degree_bits, programs
        self.constants_sigmas, self.k_is, self.gate_table, self.gate_ids = constants_sigmas, k_is, gate_table, gate_ids
        self.num_selectors, self.max_constants = num_selectors, max_constants
        self.generators, self.find, self.public_inputs, self.random_wire = generators, find, public_inputs, random_wire
        self.copy_wires = copy_wires
        # every target a copy constraint names (wires and virtual targets) and the count of virtual targets: what
        # representative_map is built from
        self.copy_targets, self.num_virtual_targets = copy_targets, num_virtual_targets
        self._representative_map, self._partition_set = representative_map, False   # (a map from wiring.sigma_polys, or built on demand)
        self.row_gates = row_gates          # per row: the index of its gate in gate_table (what a gb_generator record names)
        self.generator_programs = list(generator_programs)   # what a GB_GEN_PROGRAM record names by index
        self._generator_program_index = {tuple(pr.words): i for i, pr in enumerate(self.generator_programs)}
        self._inputs = None                 # set_generators: the targets whose values the host supplies per proof
        self._input_set = frozenset()
        self._blinding_targets = self._blinding_split = None
        self.data = None
        if ctx is not None:
            from .prover import CircuitData
            self.data = CircuitData(ctx, degree_bits, constants_sigmas, k_is, num_wires=cfg.num_wires,
                                    num_routed_wires=cfg.num_routed_wires, num_constants=max_constants,
                                    num_challenges=cfg.num_challenges, max_quotient_degree_factor=cfg.max_quotient_degree_factor,
                                    rate_bits=cfg.rate_bits, cap_height=cfg.cap_height, proof_of_work_bits=cfg.proof_of_work_bits,
                                    num_query_rounds=cfg.num_query_rounds, arity_bits=cfg.arity_bits,
                                    final_poly_bits=cfg.final_poly_bits, num_selectors=num_selectors, field=cfg.field,
                                    gates=gate_table, num_public_inputs=len(public_inputs),
                                    zero_knowledge=bool(getattr(cfg, "zero_knowledge", False)),
                                    reduction_arity_bits=cfg.reduction_arity_bits(degree_bits), programs=programs)

    @property
    def blinding_targets(self):
        """the random-value targets of the blinding rows (CircuitBuilder.blind), in creation order: with seed=, target i takes
        element i of the stream (seed, (GB_STREAM_BLINDING, 0, 0))"""
        if self._blinding_targets is None:
            self._blinding_targets = [g.target for g in self.generators if isinstance(g, _RandomValueGenerator) and g.blinding]
        return self._blinding_targets

    def blinding_values(self, seed):
        """the values of blinding_targets under `seed`: one call of random_elements on the circuit's context"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        from .polynomial_batch import random_elements
        return random_elements(self.data.ctx, self.config.field, seed, (N.GB_STREAM_BLINDING, 0, 0), 0, len(self.blinding_targets))

    def _run_generators(self, pw, rng=None, seed=None):
        """generate_partial_witness (iop/generator.rs:25-117) -> the partition witness: one value per copy class.  seed: the
        blinding rows take their values from the seed's stream instead of `rng`"""
        p = self.F.p
        w = _PartitionWitness(self.find, p, rng or np.random.default_rng(0))
        for t, v in pw.values.items():
            w.set(t, v)
        if seed is not None and self.blinding_targets:
            for t, v in zip(self.blinding_targets, self.blinding_values(seed).tolist()):
                w.set(t, v)
        pending = list(self.generators)
        while pending:
            rest = []
            for g in pending:
                if all(w.has(t) for t in g.deps):
                    g.run(w, p)
                else:
                    rest.append(g)
            if len(rest) == len(pending):
                break   # the remaining generators wait on targets nobody sets; their wires stay zero like unset wires
            pending = rest
        return w

    def generate_witness(self, pw, rng=None, seed=None):
        """generate_partial_witness + full_witness (iop/generator.rs:25-117, iop/witness.rs:359-371)
        -> (wire_values [num_wires][n], public input values)"""
        w = self._run_generators(pw, rng, seed)
        # full_witness: every wire carries the value of its copy class; unset wires are zero
        wires = np.zeros((self.config.num_wires, 1 << self.degree_bits), dtype=self.F.dtype)
        for rep, v in w.v.items():
            if rep[0] == "w":
                wires[rep[2], rep[1]] = v
        for t in self.copy_wires:
            r = self.find(t)
            if r in w.v:
                wires[t[2], t[1]] = w.v[r]
        return wires, [w.get(t) for t in self.public_inputs]

    # ---- the partition witness as the reference holds it (iop/witness.rs:318-372, plonk/circuit_data.rs:454)
    def target_index(self, t):
        """Target::index (iop/target.rs:55-60): wire (row, column) -> row * num_wires + column, virtual i -> n * num_wires + i"""
        if t[0] == "w":
            return t[1] * self.config.num_wires + t[2]
        return (self.config.num_wires << self.degree_bits) + t[1]

    @property
    def num_targets(self):
        return (self.config.num_wires << self.degree_bits) + self.num_virtual_targets

    @property
    def representative_map(self):
        """ProverOnlyCircuitData.representative_map: target index -> the index of its copy class's representative"""
        if self._representative_map is None:
            m = np.arange(self.num_targets, dtype=np.uint64)
            for t in self.copy_targets:
                m[self.target_index(t)] = self.target_index(self.find(t))
            self._representative_map = m
        return self._representative_map

    @property
    def public_input_targets(self):
        return np.array([self.target_index(t) for t in self.public_inputs], dtype=np.uint64)

    def generate_partition_witness(self, pw, rng=None, seed=None):
        """generate_partial_witness (iop/generator.rs:25-117) -> PartitionWitness.values as a dense array, one entry per target:
        the class's value at its representative, zero everywhere else (unwrap_or(ZERO)).  No expansion: full_witness() is
        gb_prove_partition's first step."""
        w = self._run_generators(pw, rng, seed)
        values = np.zeros(self.num_targets, dtype=self.F.dtype)
        for rep, v in w.v.items():
            values[self.target_index(rep)] = v
        return values

    def prove(self, pw, rng=None, seed=None):
        """seed (32 bytes; a zero-knowledge circuit needs one, and one per proof): the blinding rows' values and the salts of the
        three commitments are the seed's streams (include/goldibear_gpu.h: GB_STREAM_BLINDING, GB_STREAM_SALTS)"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        if not self._partition_set:
            self.data.set_partition(self.representative_map, self.public_input_targets)
            self._partition_set = True
        values = self.generate_partition_witness(pw, rng, seed)
        col_row = rep = None
        if self.random_wire:
            col_row = (self.random_wire[1], self.random_wire[0])
            rep = self.representative_map[self.target_index(wire(*self.random_wire))]
        return self.data.prove_partition(values, representative=rep, random_wire=col_row, rng=rng, seed=seed)

    # ---- prove() from the inputs alone: the generators run on the device (include/goldibear_gpu.h gb_circuit_set_generators)
    @property
    def random_targets(self):
        """the targets of the RandomValueGenerators, in the order the mirror draws them"""
        return [g.target for g in self.generators if isinstance(g, _RandomValueGenerator)]

    def generator_records(self):
        """prover_only.generators as gb_generator tuples (kind, gate, a, b), flat: a gate generator or a CopyGenerator is one
        tuple, a gadget generator its head and continuation tuples in a row; a RandomValueGenerator has none"""
        out = []
        for g in self.generators:
            r = g.record(self)
            if isinstance(r, list):
                out += r
            elif r is not None:
                out.append(r)
        return out

    def generator_program_index(self, program):
        return self._generator_program_index[tuple(program.words)]

    @property
    def constants_columns(self):
        return self.constants_sigmas[self.num_selectors:self.num_selectors + self.max_constants]

    def set_generators(self, input_targets=None, pw=None):
        """hand the generators over once.  input_targets: the targets whose values the host supplies per proof; the default is
        the targets of `pw` plus the random-value targets"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        if input_targets is None:
            if pw is None:
                raise ValueError("set_generators needs input_targets, or a PartialWitness to take them from")
            input_targets = list(pw.values) + [t for t in self.random_targets if t not in pw.values]
        if not self._partition_set:
            self.data.set_partition(self.representative_map, self.public_input_targets)
            self._partition_set = True
        if self.generator_programs:
            self.data.set_generator_programs(self.generator_programs)
        self.data.set_generators(self.generator_records(), [self.target_index(t) for t in input_targets], self.constants_columns)
        self._input_targets = list(input_targets)

    def input_values(self, pw, rng=None, seed=None):
        """the per-proof inputs in the order of set_generators' input_targets: the partial witness, and for the random-value
        targets the values the mirror's RandomValueGenerators would draw from `rng` - except, with seed=, the blinding rows':
        those are the seed's stream (blinding_values), placed in one indexed assignment"""
        rng = rng or np.random.default_rng(0)
        extra = [t for t in pw.values if t not in self._input_set]
        if extra:
            raise ValueError("the partial witness sets %d targets that are no inputs of the schedule (first: %r): call "
                             "set_generators again with these targets" % (len(extra), extra[0]))
        blind = self._blinding_inputs()
        drawn = {g.target: int(rng.integers(0, self.F.p, dtype=np.uint64)) for g in self.generators
                 if isinstance(g, _RandomValueGenerator) and not g.blinding} if blind is not None else \
                {t: int(rng.integers(0, self.F.p, dtype=np.uint64)) for t in self.random_targets}
        out = np.zeros(len(self._input_targets), dtype=self.F.dtype)
        others = enumerate(self._input_targets)
        if blind is not None:
            positions, ordinals, others = blind
            vals = self.blinding_values(seed) if seed is not None else \
                rng.integers(0, self.F.p, size=len(self.blinding_targets), dtype=np.uint64).astype(self.F.dtype)
            out[positions] = vals[ordinals]
        for i, t in others:
            if t in pw.values:
                out[i] = pw.values[t] % self.F.p
            elif t in drawn:
                out[i] = drawn[t]
            else:
                raise ValueError("the partial witness has no value for input target %r of the schedule" % (t,))
        return out

    def _blinding_inputs(self):
        """(positions among the schedule's inputs, ordinals among blinding_targets, the (position, target) of every other input)
        of the blinding targets that are inputs and that the partial witness does not set - None for a circuit without blinding
        rows; computed once per set_generators"""
        if not self.blinding_targets:
            return None
        if self._blinding_split is None:
            ordinal = {t: k for k, t in enumerate(self.blinding_targets)}
            hit = [(i, ordinal[t]) for i, t in enumerate(self._input_targets) if t in ordinal]
            others = [(i, t) for i, t in enumerate(self._input_targets) if t not in ordinal]
            self._blinding_split = (np.array([i for i, _ in hit], dtype=np.int64), np.array([k for _, k in hit], dtype=np.int64), others)
        return self._blinding_split

    def generate_partition_device(self, pw, rng=None, seed=None):
        """generate_partition_witness on the device -> PartitionWitness.values as a dense array, one entry per target"""
        if self._input_targets is None:
            self.set_generators(pw=pw)
        got = self.data.generate_partition(self.input_values(pw, rng, seed))
        values = np.zeros(self.num_targets, dtype=self.F.dtype)
        values[self.data.generator_classes().astype(np.int64)] = got
        return values

    def prove_inputs(self, pw, rng=None, seed=None):
        """prove() (plonk/prover.rs:136-226): the generators, full_witness() and the proof on the device, with the reference's
        retry loop - after InvZeroPermArg the random wire's input is drawn again.  seed: as for prove()"""
        if self._input_targets is None:
            self.set_generators(pw=pw)
        values = self.input_values(pw, rng, seed)
        rw = self.random_wire or None
        t = wire(*rw) if rw else None

        def redraw(val):
            values[self._input_targets.index(t)] = val

        return prove_with_retries(self.data, redraw if t in self._input_set else None,
                                  lambda hint: self.data.prove_inputs_once(values, retry_wire=hint, seed=seed),
                                  (rw[1], rw[0]) if rw else None, rng=rng, salted=seed is not None,   # (salted: the full computation)
                                  nothing_to_redraw="Permutation argument division by zero but the random wire is no input to randomize")

    # ---- does the witness these generators make satisfy the circuit?  (include/goldibear_gpu.h gb_check_partition / gb_check_inputs)
    def check(self, pw, rng=None, max_violations=16, seed=None):
        """the host generators as in prove(), the expansion and the check on the device -> (violations, result); the violations
        are native.Violation objects (describe(self) names the gate), an empty list means satisfied"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        if not self._partition_set:
            self.data.set_partition(self.representative_map, self.public_input_targets)
            self._partition_set = True
        return self.data.check_partition(self.generate_partition_witness(pw, rng, seed), max_violations=max_violations)

    def check_inputs(self, pw, rng=None, max_violations=16, seed=None):
        """the device generators as in prove_inputs(), then the check: what a generator program that disagrees with its gate
        program breaks, by row, gate and constraint"""
        if self._input_targets is None:
            self.set_generators(pw=pw)
        return self.data.check_inputs(self.input_values(pw, rng, seed), max_violations=max_violations)

    # ---- the copy constraints from sigma alone (include/goldibear_gpu.h gb_circuit_decode_sigmas / gb_circuit_copy_classes)
    def decode_sigmas(self):
        """CircuitData.decode_sigmas of the built circuit: the sigma columns read back as copy classes -> SigmaInfo; with the
        partition set (check(), prove_partition()), also that the representative map describes the same wiring"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        return self.data.decode_sigmas()

    def copy_classes(self):
        """CircuitData.copy_classes: per wire cell row * num_wires + column the lowest cell of its copy class"""
        if self.data is None:
            raise ValueError("the circuit was built without a GPU context")
        return self.data.copy_classes()

    @property
    def _input_targets(self):
        return self._inputs

    @_input_targets.setter
    def _input_targets(self, targets):
        self._inputs = None if targets is None else list(targets)
        self._input_set = frozenset(self._inputs or ())
        self._blinding_split = None

    def verify(self, proof):
        return self.data.verify(proof)

    def verify_batch(self, proofs):
        """CircuitData.verify_batch: one native.VerifyResult per proof, the query rounds checked on the device"""
        return self.data.verify_batch(proofs)

    def verify_compressed_batch(self, proofs):
        """CircuitData.verify_compressed_batch: one native.VerifyResult per compressed proof, checked as they stand on the device"""
        return self.data.verify_compressed_batch(proofs)
