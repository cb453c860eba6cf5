"""Circuits with program generators for the harnesses that run without the library (tests/host_shim/generator_programs.cpp,
tests/device/generator_programs.hip): the word file of tests/sanitize/program_case.hpp, and what the generators must produce,
computed with GeneratorProgram.evaluate in plain Python.  Every target is its own copy class (identity map).  No GPU code."""
import numpy as np

import generator_cases as GC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.generator_program import TWO_ADIC_GENERATOR, GeneratorProgram, field_sqrt
from plonky2_goldibear_amd.gate_program import field_order

FIELDS = {N.GB_GOLDILOCKS: "goldilocks", N.GB_BABYBEAR: "babybear"}
EXT_DEGREE = {N.GB_GOLDILOCKS: 2, N.GB_BABYBEAR: 4}
NON_RESIDUE = {N.GB_GOLDILOCKS: 7, N.GB_BABYBEAR: 31}      # the fields' multiplicative generators
ERR_SET_TWICE, ERR_DIVIDE_BY_ZERO, ERR_NO_SQUARE_ROOT = 1, 5, 7   # csrc/generator_ops.hpp
OUT_SKIP = 0xFFFFFFFF


def edges(field):
    """the carry edges of tests/test_device_field_edges.py that are field elements: 0, 1, p - 1, 2^32 - 1, 2^32, and for BabyBear
    the Montgomery edge words (R = 2^32 mod p, R^2, their negatives, (p + 1) / 2)"""
    p = field_order(field)
    if field == N.GB_GOLDILOCKS:
        return [0, 1, p - 1, 2**32 - 1, 2**32, 2**32 + 1, p - 2**32]
    r = 2**32 % p
    return [0, 1, p - 1, (2**32 - 1) % p, r, r * r % p, p - r, (p + 1) // 2]


class Circuit:
    """virtual targets, program generators and copies; degree_bits 3, two wires, two constants columns"""

    def __init__(self, field, seed=1, degree_bits=3):
        self.field, self.p, self.degree_bits, self.num_wires = field, field_order(field), degree_bits, 2
        rng = np.random.default_rng(seed)
        self.constants = [[int(rng.integers(0, self.p, dtype=np.uint64)) for _ in range(1 << degree_bits)] for _ in range(2)]
        self.next_target = self.num_wires << degree_bits
        self.programs, self.records, self.gens, self.inputs = [], [], [], {}

    def virtual(self):
        self.next_target += 1
        return self.next_target - 1

    def input(self, value):
        t = self.virtual()
        self.inputs[t] = int(value) % self.p
        return t

    def program_index(self, prog):
        for i, q in enumerate(self.programs):
            if q.words == prog.words:
                return i
        self.programs.append(prog)
        return len(self.programs) - 1

    def add_to(self, prog, deps, outs, row=0):
        """-> the index of the head record"""
        head = len(self.records)
        targets = list(deps) + list(outs)
        self.records.append((N.GB_GEN_PROGRAM, self.program_index(prog), len(targets), row if prog.num_constants else 0))
        self.records += N.gadget_records(0, 0, targets)[1:]
        self.gens.append(("program", prog, list(deps), list(outs), row))
        return head

    def add(self, prog, deps, row=0):
        outs = [self.virtual() for _ in range(prog.num_out)]
        self.add_to(prog, deps, outs, row)
        return outs

    def copy(self, src):
        dst = self.virtual()
        self.records.append((N.GB_GEN_COPY, 0, src, dst))
        self.gens.append(("copy", None, [src], [dst], 0))
        return dst

    def expected(self):
        """target -> value, the generators run as generate_partial_witness runs them (a disagreement raises)"""
        v, pending = dict(self.inputs), list(self.gens)
        while pending:
            rest = []
            for g in pending:
                kind, prog, deps, outs, row = g
                if not all(t in v for t in deps):
                    rest.append(g)
                    continue
                got = [v[deps[0]]] if kind == "copy" else prog.evaluate([v[t] for t in deps], [col[row] for col in self.constants])
                for t, x in zip(outs, got):
                    assert v.setdefault(t, x) == x, "target %d set twice with different values" % t
            assert len(rest) < len(pending), "generators that cannot run"
            pending = rest
        return v

    def pack(self):
        words, offsets = [], [0]
        for pr in self.programs:
            words += pr.words
            offsets.append(len(words))
        inputs = sorted(self.inputs)
        case = GC.pack(self.next_target, self.num_wires, self.degree_bits, self.p, EXT_DEGREE[self.field], np.arange(self.next_target), [], [],
                       self.constants, self.records, inputs, values=[self.inputs[t] for t in inputs])
        return np.concatenate([np.array([len(self.programs)] + offsets + words, dtype=np.uint64), case])


def all_registers_program(field):
    """d0 - (d0*2 - (d0*3 - ...)): the left operand of every subtraction stays live while the right one is computed - 32 registers"""
    def fn(d, c, ops):
        terms = [d[0] * (i + 2) for i in range(31)]
        acc = d[1] * 5
        for t in reversed(terms):
            acc = t - acc
        return [acc]
    prog = GeneratorProgram.from_function(fn, 2, 1, 0, field)
    assert prog.num_regs == 32, prog.num_regs
    return prog


def arithmetic_circuit(field):
    """everything that ends without an error, in one schedule -> (Circuit, what each part must show)"""
    p = field_order(field)
    P = lambda fn, i, o, k=0: GeneratorProgram.from_function(fn, i, o, k, field)
    c = Circuit(field)
    n = 1 << c.degree_bits
    binops = P(lambda d, k, ops: [d[0] + d[1], d[0] - d[1], d[0] * d[1]], 2, 3)
    unary = P(lambda d, k, ops: [ops.inv_or_zero(d[0]), ops.is_zero(d[0]), ops.sqrt(d[0] * d[0])], 1, 3)
    inv = P(lambda d, k, ops: [ops.inv(d[0])], 1, 1)
    sqrt = P(lambda d, k, ops: [ops.sqrt(d[0])], 1, 1)
    consts = P(lambda d, k, ops: [d[0] * k[0] + k[1]], 1, 1, 2)
    step = P(lambda d, k, ops: [(d[0] * d[0] + 3) * ops.inv_or_zero(d[0] + 1) - ops.is_zero(d[0])], 1, 1)
    es = [c.input(e) for e in edges(field)]
    for a in es:
        for b in es:
            c.add(binops, [a, b])
        c.add(unary, [a])
    for x in (1, p - 1, 2, 12345):
        c.add(inv, [c.input(x)])
    rng = np.random.default_rng(5 + field)
    z = TWO_ADIC_GENERATOR[field]
    roots = []
    for x in [0, z * z % p] + [int(r) * int(r) % p for r in rng.integers(1, p, 64, dtype=np.uint64)]:
        roots.append((x, c.add(sqrt, [c.input(x)])[0]))
    c.add(all_registers_program(field), [c.input(3), c.input(p - 2)])
    for row in (0, n - 1, 3):
        c.add(consts, [c.input(row + 11)], row=row)
    # a level of 257 program generators (two workgroups of the level kernel), mixed with copies, then a chain of 5 narrow levels
    wide = [c.input(int(v)) for v in rng.integers(0, p, 257, dtype=np.uint64)]
    firsts = [c.add(step, [t])[0] for t in wide]
    copies = [c.copy(t) for t in wide[:40]]
    for t in firsts[:3] + copies[:2]:
        for _ in range(5):
            t = c.add(step, [t])[0]
    # an output in an input's class that agrees; two programs of one level writing one class (the second compares one level on,
    # and its other output is written by the first op: OUT_SKIP in both ops)
    x = c.input(77)
    c.add_to(step, [x], [c.input(step.evaluate([77])[0])])
    two = P(lambda d, k, ops: [d[0] + 9, d[0] * d[0]], 1, 2)
    shared = c.virtual()
    c.add_to(two, [x], [c.virtual(), shared])
    c.add_to(two, [x], [c.virtual(), shared])
    return c, roots


def error_circuits(field):
    """-> [(name, Circuit, error code, index of the head record, the class's target or None)]"""
    p = field_order(field)
    P = lambda fn, i, o, k=0: GeneratorProgram.from_function(fn, i, o, k, field)
    inv = P(lambda d, k, ops: [ops.inv(d[0] - 5)], 1, 1)
    sqrt = P(lambda d, k, ops: [ops.sqrt(d[0])], 1, 1)
    out = []
    for name, prog, value, code in (("INV of zero", inv, 5, ERR_DIVIDE_BY_ZERO), ("SQRT of a non-residue", sqrt, NON_RESIDUE[field], ERR_NO_SQUARE_ROOT)):
        c = Circuit(field)
        c.add(sqrt, [c.input(4)])
        c.copy(c.input(1))
        head = c.add_to(prog, [c.input(value)], [c.virtual()])
        out.append((name, c, code, head, None))
    c = Circuit(field)
    c.add(sqrt, [c.input(9)])
    wrong = c.input(10)
    head = c.add_to(sqrt, [c.input(16)], [wrong])      # sqrt(16) is 4 or p - 4, never 10
    assert field_sqrt(16, field) in (4, p - 4)
    out.append(("an output that disagrees with an input of its class", c, ERR_SET_TWICE, head, wrong))
    return out


def all_cases(field):
    """-> (the cases of one word file, a checker of read_values' result for it)"""
    good, roots = arithmetic_circuit(field)
    bad = error_circuits(field)
    want = good.expected()

    def check(res):
        r = res[0]
        assert not isinstance(r, int), "refused with status %r" % (r,)
        assert r["err"] == [0, 0, 0, 0] and r["num_unrunnable"] == 0, r["err"]
        assert r["num_levels"] == 6 and r["num_launches"] == 2, (r["num_levels"], r["num_launches"])   # the wide level, then a chain of 5
        got = {int(t): int(v) for t, v in zip(r["class_reps"], r["values"])}
        diff = [t for t in want if got[t] != want[t]]
        assert not diff, "%d targets differ, first %d: %d, mirror %d" % (len(diff), diff[0], got[diff[0]], want[diff[0]])
        for x, t in roots:
            assert got[t] * got[t] % good.p == x
        for (name, c, code, head, target), r in zip(bad, res[1:]):
            assert not isinstance(r, int), name
            assert r["err"][:2] == [code, head], (name, r["err"])
            cls = r["err"][2]
            assert cls == OUT_SKIP if target is None else int(r["class_reps"][cls]) == target, (name, r["err"])

    return [good.pack()] + [c.pack() for _, c, _, _, _ in bad], check
