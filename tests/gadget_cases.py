"""Cases for the gadget generators (Equality, NonzeroTest, QuotientOrZero, QuotientExtension, Split, WireSplit, LowHigh, BaseSum:
record kinds 32..39, include/goldibear_gpu.h), beside tests/generator_cases.py: the same word file, the same harness programs
(tests/sanitize/generator_schedule.cpp, tests/host_shim/generators.cpp, tests/device/generators.hip), compiled from here.  The
oracle is the builder mirror's generator classes (plonky2_goldibear_amd/circuit_builder.py).

Independent records live on a stub circuit of ONE wire per row, one NoopGate and an identity representative map: target i is
wire (i, 0), so every operand of a gadget generator - and the WIRE_SUM wire (row, 0) that WireSplitGenerator and BaseSumGenerator
name by row - is simply a target index."""
import os
import subprocess

import numpy as np

import gate_variants as GV
import generator_cases as GC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import circuit_builder as CB
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness, wire
from wired_circuits import edge_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "plonky2_goldibear_amd", "csrc")
KINDS = ("equality", "nonzero_test", "quotient_or_zero", "quotient_extension", "split", "wire_split", "low_high", "base_sum")
ERR_SPLIT_TOO_LARGE, ERR_DIVIDE_BY_ZERO, ERR_NOT_BOOLEAN = 4, 5, 6   # csrc/generator_ops.hpp


# ------------------------------------------------------------------------------------------------ the harness programs
def compile_sanitize(out):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "generator_schedule.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return str(out)


def compile_host_shim(out):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run([CLANG, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim, "-I", os.path.join(ROOT, "tests", "sanitize"),
                    "-I", CSRC, "-o", str(out), os.path.join(shim, "generators.cpp")], check=True, capture_output=True, text=True)
    return str(out)


def compile_device(out):
    assert os.path.exists(HIPCC), "needs hipcc"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "sanitize"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "generators.hip")], check=True, capture_output=True, text=True)
    return str(out)


def run_values(exe, tmp_path, cases, mode=None, tag="", public=None):
    """cases through the host shim (mode None) or the device harness (mode "plan" / "level", which also writes each case's
    `public` gathered public inputs: default none) -> GC.read_values, stdout"""
    src, dst = tmp_path / ("in%s.bin" % tag), tmp_path / ("out%s.bin" % tag)
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)] + ([mode] if mode else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    got = np.fromfile(dst, dtype=np.uint64)
    return GC.read_values(got, len(cases), gathered=(public or [0] * len(cases)) if mode else None), out.stdout


# ------------------------------------------------------------------------------------------------ independent records
class _Stub:
    """what record() asks of a built circuit, on the one-wire stub"""

    @staticmethod
    def target_index(t):
        assert t[0] == "w" and t[2] == 0
        return t[1]


def _t(i):
    return wire(i, 0)


def _field_edges(F):
    p = F.P
    e = list(edge_values(F))
    if F is GV.FIELDS[N.GB_GOLDILOCKS]:
        e += [2**32 - 1, 2**32, p - 2**32]
    return [int(x) % p for x in e]


def _pairs(F, a):
    """the operand pairs of Equality / QuotientOrZero"""
    p = F.P
    out = [(0, 0), (0, p - 1), (p - 1, 0), (1, 0), (a, a), (a, (a + 1) % p)]
    if F is GV.FIELDS[N.GB_GOLDILOCKS]:
        s = [2**32 - 1, 2**32, p - 2**32]
        out += [(x, y) for x in s for y in s] + [(x, 0) for x in s] + [(0, x) for x in s]
    return out


# per kind: the shapes (what decides the record's length and parameter) that instances() cycles through
SPLIT_BITS = (1, 2, 31, 64)                    # 64 bits: 65 targets, an odd count whose last continuation record is padded
WIRE_SPLIT_SHAPES = ((1, 1), (1, 3), (31, 1), (31, 3), (63, 1), (63, 3), (64, 1), (64, 2))   # (num_limbs, gates)
LOW_HIGH_LOGS = (0, 1, 31, 63)
BASE_SUM_SHAPES = ((1, 2), (2, 2), (63, 2), (64, 2), (1, 3), (2, 255), (63, 3), (64, 255))   # (limbs, base)


def _capacity(limbs, gates):
    return 64 if limbs >= 64 else min(64, limbs * gates)


def make(field, kind, shape, base, operands):
    """one generator whose targets start at target `base` -> (generator, {input target: value}, number of targets)"""
    F = GV.FIELDS[field]
    D = F.D
    if kind == "equality":
        g = CB._EqualityGenerator(_t(base), _t(base + 1), _t(base + 2), _t(base + 3))
        return g, {_t(base): operands[0], _t(base + 1): operands[1]}, 4
    if kind == "nonzero_test":
        return CB._NonzeroTestGenerator(_t(base), _t(base + 1)), {_t(base): operands[0]}, 2
    if kind == "quotient_or_zero":
        g = CB._QuotientOrZeroGenerator(_t(base), _t(base + 1), _t(base + 2))
        return g, {_t(base): operands[0], _t(base + 1): operands[1]}, 3
    if kind == "quotient_extension":
        ts = [_t(base + k) for k in range(3 * D)]
        g = CB._QuotientExtensionGenerator(field, ts[:D], ts[D:2 * D], ts[2 * D:])
        return g, dict(zip(ts[:2 * D], operands)), 3 * D
    if kind == "split":
        g = CB._SplitGenerator(_t(base), [_t(base + 1 + k) for k in range(shape)])
        return g, {_t(base): operands[0]}, 1 + shape
    if kind == "wire_split":
        limbs, gates = shape
        g = CB._WireSplitGenerator(_t(base), [base + 1 + k for k in range(gates)], limbs)
        return g, {_t(base): operands[0]}, 1 + gates
    if kind == "low_high":
        return CB._LowHighGenerator(_t(base), shape, _t(base + 1), _t(base + 2)), {_t(base): operands[0]}, 3
    assert kind == "base_sum"
    limbs, b = shape
    ts = [_t(base + 1 + k) for k in range(limbs)]
    return CB._BaseSumGenerator(base, ts, b), dict(zip(ts, operands)), 1 + limbs


def operands(field, kind, count, seed):
    """`count` (shape, operands) of one kind: the shapes in turn; per shape the edge operands first, then random ones"""
    F = GV.FIELDS[field]
    p, D = F.P, F.D
    rng = np.random.default_rng(seed)
    rnd = lambda hi=p: int(rng.integers(0, hi, dtype=np.uint64)) if hi <= 2**63 else int(rng.integers(0, 2**64, dtype=np.uint64)) % hi
    edges = _field_edges(F)
    a = 0x1234567 % p
    shapes = {"split": SPLIT_BITS, "wire_split": WIRE_SPLIT_SHAPES, "low_high": LOW_HIGH_LOGS, "base_sum": BASE_SUM_SHAPES}.get(kind, (None,))
    out = []
    for i in range(count):
        shape, rnd_no = shapes[i % len(shapes)], i // len(shapes)
        if kind in ("equality", "quotient_or_zero"):
            table = _pairs(F, a)
            if rnd_no < len(table):
                ops = table[rnd_no]
            else:
                x = rnd()
                ops = (x, x if rnd_no % 4 == 0 else rnd())
        elif kind == "nonzero_test":
            ops = (edges[rnd_no] if rnd_no < len(edges) else rnd(),)
        elif kind == "quotient_extension":
            num = [rnd() for _ in range(D)]
            table = [num + [rnd(p - 1) + 1] + [0] * (D - 1),          # a base-field-only denominator
                     num + [0] + [rnd(p - 1) + 1 for _ in range(D - 1)],   # c[0] = 0
                     num + [p - 1] * D,
                     [0] * D + [rnd() for _ in range(D - 1)] + [1],      # numerator zero
                     [p - 1] * D + [p - 1] * D]
            ops = table[rnd_no] if rnd_no < len(table) else num + [rnd() for _ in range(D - 1)] + [rnd(p - 1) + 1]
        elif kind in ("split", "wire_split"):
            bits = shape if kind == "split" else _capacity(*shape)
            top = min(1 << bits, p)
            table = [0, 1, top - 1, (1 << (bits - 1)) % top] + [e for e in edges if e < top]
            ops = (table[rnd_no] if rnd_no < len(table) else rnd(top),)
        elif kind == "low_high":
            ops = (edges[rnd_no] if rnd_no < len(edges) else rnd(),)
        else:
            limbs = shape[0]
            table = [[1] * limbs, [0] * limbs, [k & 1 for k in range(limbs)], [1] + [0] * (limbs - 1), [0] * (limbs - 1) + [1]]
            ops = table[rnd_no] if rnd_no < len(table) else [int(x) for x in rng.integers(0, 2, limbs)]
        out.append((shape, ops))
    return out


def failing(field, kind):
    """one instance whose run_once panics in the reference -> (shape, operands, error code, index of the offending target among
    the generator's targets), or None for a kind that cannot fail"""
    F = GV.FIELDS[field]
    D = F.D
    if kind == "quotient_extension":
        return None, [5] * D + [0] * D, ERR_DIVIDE_BY_ZERO, D
    if kind == "split":
        return 1, (2,), ERR_SPLIT_TOO_LARGE, 0
    if kind == "wire_split":
        return (1, 3), (8,), ERR_SPLIT_TOO_LARGE, 0
    if kind == "base_sum":
        return (3, 2), [1, 2, 0], ERR_NOT_BOOLEAN, 2     # targets: sum, limb 0, limb 1 (= 2), limb 2
    return None


def instances(field, kind, count, seed):
    """-> [(generator, inputs)] laid end to end over the stub's targets, and the number of targets used"""
    out, base = [], 0
    for shape, ops in operands(field, kind, count, seed):
        g, inputs, width = make(field, kind, shape, base, ops)
        out.append((g, inputs))
        base += width
    return out, base


def mirror(field, insts):
    """the mirror's run() on every instance -> {target index: value} of everything set"""
    p = GV.FIELDS[field].P
    w = CB._PartitionWitness(lambda t: t, p, None)
    for g, inputs in insts:
        for t, v in inputs.items():
            w.set(t, v)
        g.run(w, p)
    return {t[1]: v for t, v in w.v.items()}


def pack_instances(field, insts, num_targets_used):
    F = GV.FIELDS[field]
    degree_bits = max(2, (max(1, num_targets_used) - 1).bit_length())
    n = 1 << degree_bits
    records, inputs, values = [], [], []
    for g, inp in insts:
        records += g.record(_Stub)
        for t, v in inp.items():
            inputs.append(_Stub.target_index(t))
            values.append(v)
    return GC.pack(n, 1, degree_bits, F.P, F.D, np.arange(n, dtype=np.uint64), [], [(0, 0, 0, 0)], np.zeros((0, n), dtype=np.uint64),
                   records, inputs, values)


def assert_values(r, want, what):
    """a result of run_values on a stub case against mirror()"""
    assert not isinstance(r, int), "%s: refused with status %r" % (what, r)
    assert r["err"] == [0, 0, 0, 0], "%s: error word %r" % (what, r["err"])
    assert r["num_unrunnable"] == 0, what
    expect = np.zeros(len(r["values"]), dtype=np.uint64)
    assert np.array_equal(r["class_reps"], np.arange(len(expect))), what      # identity map: class k is target k
    for t, v in want.items():
        expect[t] = v
    bad = np.nonzero(r["values"] != expect)[0]
    assert not len(bad), "%s: %d targets differ, first at %d: %d, mirror %d" % (what, len(bad), bad[0], r["values"][bad[0]], expect[bad[0]])


# ------------------------------------------------------------------------------------------------ builder circuits
def config(field, **kw):
    return CircuitConfig.standard_recursion_config_gl(**kw) if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow(**kw)


def _pad(b, degree_bits):
    """NoopGates up to just below 2^degree_bits rows, leaving room for what build() adds (the public-input gate, the hash of the
    public inputs and the constants' gates)"""
    if degree_bits is None:
        return
    b.zero()                                                 # the hash's padding and swap wire: a constant before the count below
    consts = max(0, len(b.constants_to_targets) - len(b.constant_generators))
    room = 1 + -(-len(b.public_inputs) // 8) + -(-consts // b.config.num_constants)
    while b.num_gates() + room < (1 << degree_bits):
        b.add_gate(CB.NoopGate())


def top_bits(field):
    return 64 if field == N.GB_GOLDILOCKS else 31


def builder_circuits(field, degree_bits=None):
    """[(name, builder, partial witness)]: one circuit per gadget, laid out as the reference's gadgets lay them out"""
    F = GV.FIELDS[field]
    p, D = F.P, F.D
    out = []

    def circuit(name, fill):
        b, pw = CircuitBuilder(config(field)), PartialWitness()
        fill(b, pw)
        _pad(b, degree_bits)
        out.append((name, b, pw))

    def equal(x_value, y_value):
        def fill(b, pw):
            x, y = b.add_virtual_target(), b.add_virtual_target()
            e = b.is_equal(x, y)
            b.register_public_input(e)
            b.register_public_input(b.select(e, x, b.constant(77)))
            pw.set_target(x, x_value)
            pw.set_target(y, y_value)
        return fill

    circuit("is_equal, equal inputs", equal(p - 2, p - 2))
    circuit("is_equal, unequal inputs", equal(p - 2, 3))

    def split(bits, value):
        def fill(b, pw):
            x = b.add_virtual_target()
            got = b.split_le(x, bits)
            b.register_public_input(got[0])
            b.register_public_input(got[-1])
            pw.set_target(x, value)
        return fill

    circuit("split_le, 1 bit", split(1, 1))
    circuit("split_le, %d bits" % top_bits(field), split(top_bits(field), p - 1))

    def le_sum(num_bits):
        def fill(b, pw):
            bits = b.add_virtual_targets(num_bits)
            b.register_public_input(b.le_sum(bits))
            for i, t in enumerate(bits):
                pw.set_target(t, (0xB5A3C96 >> (i % 28)) & 1)
        return fill

    ops = CB.ArithmeticGate.new_from_config(config(field)).num_ops
    circuit("le_sum, arithmetic branch", le_sum(ops + 1))
    circuit("le_sum, BaseSumGate branch", le_sum(ops + 2))

    def low_high(b, pw):
        x = b.add_virtual_target()
        low, high = b.split_low_high(x, 5, 20)
        b.register_public_inputs([low, high])
        pw.set_target(x, 0xABCDE)

    circuit("split_low_high", low_high)

    def div(b, pw):
        x, y = b.add_virtual_extension_target(), b.add_virtual_extension_target()
        q = b.div_extension(x, y)
        b.register_public_inputs(list(q))
        b.register_public_input(b.div(x[0], y[1]))
        b.register_public_input(b.inverse_or_zero(x[1]))
        b.register_public_inputs(list(b.sub_extension(b.add_extension(q, x), y)))
        for k in range(D):
            pw.set_target(x[k], (p - 1 - k) % p)
            pw.set_target(y[k], 3 + 5 * k)

    circuit("div_extension", div)

    def select(b, pw):
        c, x, y = b.add_virtual_bool_target_safe(), b.add_virtual_target(), b.add_virtual_target()
        s = b.select(c, x, y)
        t = b._if(b.not_(c), x, y)
        b.register_public_inputs([s, t, b.or_(c, b.and_(c, b.is_equal(s, t)))])
        pw.set_target(c, 1)
        pw.set_target(x, p - 1)
        pw.set_target(y, 2)

    circuit("select", select)

    def low_bits(b, pw):
        x, y = b.add_virtual_target(), b.add_virtual_target()
        b.register_public_inputs(b.low_bits(x, 3, False, top_bits(field)))      # add_many over the low and the high bits
        b.register_public_inputs(b.split_le_base(y, 4, 3))
        b.register_public_input(b.inverse(y))
        pw.set_target(x, p - 3)
        pw.set_target(y, 50)

    circuit("low_bits", low_bits)
    return out


def chain_rounds(min_levels):
    """a round is at least five levels: LowHigh, WireSplit / BaseSplit, BaseSum, Equality and the arithmetic that joins them"""
    return -(-min_levels // 5) + 1


def chained_gadgets(field, min_levels):
    """split_low_high -> split_le -> le_sum (BaseSumGate branch) -> is_equal, the result fed into the next round, until the
    dependency chain is at least `min_levels` long -> (builder, pw)"""
    n_log, num_bits = (24, 30) if field == N.GB_GOLDILOCKS else (12, 20)
    b, pw = CircuitBuilder(config(field)), PartialWitness()
    x = b.add_virtual_target()
    pw.set_target(x, (1 << num_bits) - 5)
    for _ in range(chain_rounds(min_levels)):
        low, high = b.split_low_high(x, n_log, num_bits)
        s = b.le_sum(b.split_le(low, n_log))
        e = b.is_equal(s, low)
        x = b.add(s, e)
    b.register_public_input(x)
    return b, pw
