"""Circuits whose program generators use the integer operations (IDIV, IREM, SHR, AND, LT), for the harnesses of
tests/generator_program_cases.py (tests/host_shim/generator_programs.cpp, tests/device/generator_programs.hip read the same word
file), and what they must produce: GeneratorProgram.evaluate, which tests/test_integer_programs.py holds against plain Python
integers first.  No GPU code."""
import generator_program_cases as PC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.generator_program import GeneratorProgram
from plonky2_goldibear_amd.gate_program import field_order

FIELDS = PC.FIELDS
ERR_INTEGER_DIVIDE_BY_ZERO = 9   # csrc/generator_ops.hpp
OPS = ("idiv", "irem", "shr", "and_", "lt")
SHIFTS = lambda p: [0, 1, 31, 32, 33, 63, 64, 65, p - 1]


def edges(field):
    """where a 64-bit divide built from 32-bit pieces, a Montgomery round trip and a shift guard can go wrong"""
    p = field_order(field)
    if field == N.GB_GOLDILOCKS:
        return [0, 1, 2, 3, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, p - 2, p - 1]
    return [0, 1, 2, 3, 2**15, 2**27, 2**27 + 1, 2**30, (p - 1) // 2, p - 2, p - 1]


def operand_pairs(field, op):
    """the full cross product of the edges; SHR over the shift amounts too; no division by zero"""
    es = edges(field)
    pairs = [(a, b) for a in es for b in es]
    if op == "shr":
        pairs += [(a, s) for a in es for s in SHIFTS(field_order(field))]
    return [(a, b) for a, b in pairs if b or op not in ("idiv", "irem")]


def binary_program(field, op):
    return GeneratorProgram.from_function(lambda d, c, ops: [getattr(ops, op)(d[0], d[1])], 2, 1, 0, field)


def plain(op, a, b):
    """the operation on Python integers, written apart from generator_program.integer_op"""
    if op == "idiv":
        return a // b
    if op == "irem":
        return a - (a // b) * b
    if op == "shr":
        return a // 2**b if b < 64 else 0
    if op == "and_":
        return sum(1 << i for i in range(64) if (a >> i) & (b >> i) & 1)
    return 1 if a < b else 0


def step_program(field):
    """one link of the chain: integer results feed field and integer operations of the next level"""
    def fn(d, c, ops):
        t = d[0]
        q = ops.idiv(t * t + 3, ops.and_(t, 0xFFFF) + 1)
        return [q + ops.irem(t, 1000003) * ops.lt(q, t) + ops.shr(t, ops.and_(q, 31))]
    return GeneratorProgram.from_function(fn, 1, 1, 0, field)


def good_circuit(field):
    """-> (Circuit, [(op, a, b, output target)]): level 1 holds every pair of every operation (more than 256 generators: two
    workgroups of the level kernel), then a chain of 5 narrow levels that hand integer results on"""
    c = PC.Circuit(field)
    p = c.p
    inputs = {}

    def inp(v):
        if v not in inputs:
            inputs[v] = c.input(v)
        return inputs[v]

    table = []
    for op in OPS:
        prog = binary_program(field, op)
        for a, b in operand_pairs(field, op):
            table.append((op, a, b, c.add(prog, [inp(a), inp(b)])[0]))
    assert len(table) > 256
    # operands that are literals, and a shift amount computed from a dependency
    lits = GeneratorProgram.from_function(lambda d, k, ops: [ops.shr(d[0], 3), ops.idiv(d[0], 7), ops.irem(p - 1, ops.shr(d[0], 1) + 1), ops.lt(5, d[0]),
                                                             ops.shr(d[0], ops.and_(d[0], 63)), ops.and_(ops.shr(p - 1, 1), d[0])], 1, 6, 0, field)
    firsts = [c.add(lits, [inp(a)])[0] for a in edges(field)]
    step = step_program(field)
    for t in firsts[3:8]:
        for _ in range(5):
            t = c.add(step, [t])[0]
    return c, table


def error_circuits(field):
    """-> [(name, Circuit, error code, index of the head record)]: IDIV by zero and IREM by zero, each in a circuit of its own,
    behind generators that run"""
    out = []
    for op in ("idiv", "irem"):
        c = PC.Circuit(field)
        prog = binary_program(field, op)
        c.add(prog, [c.input(9), c.input(4)])
        c.copy(c.input(1))
        zero = GeneratorProgram.from_function(lambda d, k, ops: [getattr(ops, op)(d[0], d[1] - 5)], 2, 1, 0, field)
        head = c.add_to(zero, [c.input(77), c.input(5)], [c.virtual()])
        out.append((op.upper() + " by zero", c, ERR_INTEGER_DIVIDE_BY_ZERO, head))
    return out


def all_cases(field):
    """-> (the cases of one word file, a checker of read_values' result for it)"""
    good, table = good_circuit(field)
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
        for op, a, b, t in table:
            assert got[t] == plain(op, a, b), (op, a, b, got[t])
        for (name, c, code, head), r in zip(bad, res[1:]):
            assert not isinstance(r, int), name
            assert r["err"][:3] == [code, head, PC.OUT_SKIP], (name, r["err"])

    return [good.pack()] + [c.pack() for _, c, _, _ in bad], check
