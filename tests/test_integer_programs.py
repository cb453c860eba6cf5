"""The integer operations of a generator program (IDIV, IREM, SHR, AND, LT: plonky2_goldibear_amd/generator_program.py,
csrc/generators.hpp gen_integer_op, csrc/generator_programs.hpp) without a GPU:

  * the mirror GeneratorProgram.evaluate against plain Python integers over the full cross product of the edge operands of
    tests/integer_program_cases.py, the shift amounts among them, both fields; division by zero raises; the tracer folds and
    commutes nothing, and a shift amount may be a dependency, a literal or a computed value;
  * the interpreter compiled for the CPU (tests/host_shim/generator_programs.cpp) as a stand-alone program under
    AddressSanitizer and UndefinedBehaviorSanitizer on the circuits of integer_program_cases.py - a level of more than 256
    generators, a chain of 5 narrow levels, IDIV and IREM by zero with code 9 and their record - equal to the mirror at every target;
  * the checker on the new opcodes in a stand-alone program under the sanitizers (tests/sanitize/integer_programs.cpp);
  * ops.ext against oracle/fields.py: products and inverses of random elements and of elements with zero coordinates, one INV
    per inverse, the inverse of zero raising what INV raises;
  * mul_add_split_gate: its constraints vanish on its generator's outputs at the range edges and do not with one limb changed;
    the gadgets refuse widths at which their equations could wrap."""
import os
import subprocess

import numpy as np
import pytest

import generator_cases as GC
import integer_program_cases as IC
from oracle import fields as OF
from plonky2_goldibear_amd import GeneratorProgram, mul_add_split_gate, native as N
from plonky2_goldibear_amd import generator_program as GP
from plonky2_goldibear_amd import integer_gadgets as IG
from plonky2_goldibear_amd.gate_program import field_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
FIELDS = sorted(IC.FIELDS)
ORACLE = {N.GB_GOLDILOCKS: OF.GL, N.GB_BABYBEAR: OF.BB}


@pytest.mark.parametrize("field", FIELDS)
def test_the_mirror_equals_plain_integers(field):
    p = field_order(field)
    assert set(IC.SHIFTS(p)) <= {b for _, b in IC.operand_pairs(field, "shr")}
    for op in IC.OPS:
        prog = IC.binary_program(field, op)
        assert GP.decode_opcode(prog.instructions[0]) == {"idiv": 16, "irem": 17, "shr": 18, "and_": 19, "lt": 20}[op]
        pairs = IC.operand_pairs(field, op)
        assert len(pairs) >= len(IC.edges(field)) * (len(IC.edges(field)) - 1)
        for a, b in pairs:
            (got,) = prog.evaluate([a, b])
            assert got == IC.plain(op, a, b) and 0 <= got < p, (op, a, b, got)
    for op in ("idiv", "irem"):
        for a in IC.edges(field):
            with pytest.raises(GP.IntegerDivideByZeroError, match="attempt to divide by zero"):
                IC.binary_program(field, op).evaluate([a, 0])
    assert issubclass(GP.IntegerDivideByZeroError, ArithmeticError)


@pytest.mark.parametrize("field", FIELDS)
def test_the_tracer_folds_nothing_it_should_not(field):
    p = field_order(field)
    P = lambda fn, i, o: GeneratorProgram.from_function(fn, i, o, 0, field)
    # two integers stay two literals: the operation is in the program, not folded by the tracer
    lits = P(lambda d, c, ops: [ops.idiv(7, 2), ops.shr(p - 1, 1), ops.lt(3, 3), ops.and_(6, 3), ops.irem(7, 4)], 0, 5)
    assert [GP.decode_opcode(w) for w in lits.instructions if GP.decode_opcode(w) != GP.OP_OUT] == [16, 18, 20, 19, 17]
    assert lits.evaluate([]) == [3, (p - 1) >> 1, 0, 2, 3]
    # the operands are not swapped, and x op x is not simplified
    order = P(lambda d, c, ops: [ops.lt(d[1], d[0]), ops.lt(d[0], d[1]), ops.idiv(d[0], d[0]), ops.and_(d[1], d[0]), ops.and_(d[0], d[1])], 2, 5)
    assert order.evaluate([5, 9]) == [0, 1, 1, 1, 1] and order.num_instrs == 10
    # equal subexpressions are one node; registers are reused after the last use
    shared = P(lambda d, c, ops: [ops.shr(d[0], 4) + ops.shr(d[0], 4), ops.shr(d[0], 4) * 3], 1, 2)
    assert sum(GP.decode_opcode(w) == GP.OP_SHR for w in shared.instructions) == 1
    assert shared.evaluate([0x123]) == [0x24, 0x36]
    # the shift amount as a dependency, a literal and a computed value
    amount = P(lambda d, c, ops: [ops.shr(d[0], d[1]), ops.shr(d[0], 5), ops.shr(d[0], ops.and_(d[1], 3) + 60)], 2, 3)
    assert amount.evaluate([p - 1, 33]) == [(p - 1) >> 33, (p - 1) >> 5, (p - 1) >> 61]
    assert amount.evaluate([p - 1, 63]) == [(p - 1) >> 63, (p - 1) >> 5, (p - 1) >> 63]
    assert amount.evaluate([p - 1, 64]) == [0, (p - 1) >> 5, (p - 1) >> 60]
    assert amount.evaluate([p - 1, p - 1]) == [0, (p - 1) >> 5, (p - 1) >> 60]
    # the sugar
    sugar = P(lambda d, c, ops: [ops.low_bits(d[0], 12), ops.bit(d[0], 0), ops.bit(d[0], 5), ops.bit(d[0], d[1]), ops.select(ops.lt(d[0], d[1]), 11, 22),
                                 ops.select(ops.lt(d[1], d[0]), 11, 22)] + ops.bits(d[0], 8), 2, 14)
    x = 0xABCDE
    assert sugar.evaluate([x, 7]) == [x & 0xFFF, x & 1, (x >> 5) & 1, (x >> 7) & 1, 22, 11] + [(x >> i) & 1 for i in range(8)]
    assert {GP.decode_opcode(w) for w in sugar.instructions} <= {GP.OP_ADD, GP.OP_SUB, GP.OP_MUL, GP.OP_OUT, GP.OP_SHR, GP.OP_AND, GP.OP_LT}
    with pytest.raises(ValueError):
        P(lambda d, c, ops: [ops.low_bits(d[0], 64)], 1, 1)


def compile_sanitized(out, source, *flags):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    subprocess.run([CLANG, "-O1", "-g1", "-std=c++17"] + SANITIZE + list(flags) +
                   ["-I", os.path.join(ROOT, "tests", "sanitize"), "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(out), source],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    shim = os.path.join(ROOT, "tests", "host_shim")
    return compile_sanitized(tmp_path_factory.mktemp("integer_programs_host") / "generator_programs", os.path.join(shim, "generator_programs.cpp"),
                             "-include", os.path.join(shim, "shim.h"), "-I", shim)


@pytest.mark.parametrize("field", FIELDS)
def test_the_interpreter_on_the_host_equals_the_mirror_under_the_sanitizers(exe, tmp_path, field):
    cases, check = IC.all_cases(field)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    check(GC.read_values(np.fromfile(dst, dtype=np.uint64), len(cases)))


def test_the_checker_on_the_integer_opcodes_under_the_sanitizers(tmp_path):
    exe = compile_sanitized(tmp_path / "integer_programs", os.path.join(ROOT, "tests", "sanitize", "integer_programs.cpp"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    assert "all checks held" in out.stdout


@pytest.mark.parametrize("field", FIELDS)
def test_ext_equals_the_oracle_field(field):
    F = ORACLE[field]
    p, D = F.P, F.D
    assert GP.EXT_W[field] == (D, F.W)
    P = lambda fn, o: GeneratorProgram.from_function(fn, 2 * D, o, 0, field)
    mul = P(lambda d, c, ops: (ops.ext(d[:D]) * ops.ext(d[D:])).coords, D)
    inv = P(lambda d, c, ops: ops.ext(d[:D]).inv().coords, D)
    div = P(lambda d, c, ops: (ops.ext(d[:D]) / ops.ext(d[D:])).coords, D)
    mix = P(lambda d, c, ops: ((ops.ext(d[:D]) + ops.ext(d[D:])) * d[0] - ops.ext(d[D:]) * 3 + 1).coords, D)
    for prog in (inv, div):
        assert [GP.decode_opcode(w) for w in prog.instructions].count(GP.OP_INV) == 1
        assert GP.OP_INV_OR_ZERO not in [GP.decode_opcode(w) for w in prog.instructions]
    rng = np.random.default_rng(11 + field)
    rnd = lambda: tuple(int(v) for v in rng.integers(0, p, D, dtype=np.uint64))
    elements = [rnd() for _ in range(12)] + [(p - 1,) * D, F.one]
    for k in range(1, 1 << D):      # every pattern of zero coordinates but all zero
        elements.append(tuple(int(rng.integers(1, p, dtype=np.uint64)) if k >> i & 1 else 0 for i in range(D)))
    for i, a in enumerate(elements):
        b = elements[(i * 7 + 3) % len(elements)]
        assert tuple(mul.evaluate(a + b)) == F.emul(a, b)
        assert tuple(inv.evaluate(a + b)) == F.einv(a)
        assert F.emul(tuple(inv.evaluate(a + b)), a) == F.one
        assert tuple(div.evaluate(a + b)) == F.ediv(a, b)
        assert tuple(mix.evaluate(a + b)) == F.eadd(F.esub(F.escale(F.eadd(a, b), a[0]), F.escale(b, 3)), F.one)
        assert tuple(mul.evaluate(a + F.zero)) == F.zero
    with pytest.raises(GP.InvertZeroError, match="Tried to invert zero"):
        inv.evaluate(F.zero + F.one)
    with pytest.raises(GP.InvertZeroError, match="Tried to invert zero"):
        div.evaluate(F.one + F.zero)
    with pytest.raises(ValueError):
        P(lambda d, c, ops: ops.ext(d[:D + 1]).coords, D)


@pytest.mark.parametrize("field", FIELDS)
def test_mul_add_split_gate_constraints_vanish_on_its_generator(field):
    p, h = field_order(field), IG.HALF_BITS[field]
    assert h == (32 if field == N.GB_GOLDILOCKS else 14)
    gate = mul_add_split_gate(field)
    (gen,) = gate.generators(0, [])
    prog = gen.generator_program
    assert gate.num_wires == 5 + h == 3 + prog.num_out and gate.num_constraints == 3 + h and gate.degree == 4
    assert {GP.decode_opcode(w) for w in prog.instructions} == {GP.OP_MUL, GP.OP_ADD, GP.OP_AND, GP.OP_SHR, GP.OP_OUT}
    top = (1 << h) - 1
    for a, b, c in ((top, top, top), (0, 0, 0), (top, 1, 0), (1, 1, top), (top - 1, 3, 5)):
        outs = prog.evaluate([a, b, c])
        x = a * b + c
        assert x < p and outs[:2] == [x & top, x >> h]
        assert outs[2:] == [(half >> 2 * i) & 3 for half in outs[:2] for i in range(h // 2)]
        wires = [a, b, c] + outs
        assert gate.program.evaluate(wires, []) == [0] * gate.num_constraints
        for limb in (0, h // 2 - 1, h // 2, h - 1):          # one limb changed: its half's sum, and for a 4 its own range
            for value in ((wires[5 + limb] + 1) % 4, 4):
                bad = list(wires)
                bad[5 + limb] = value
                got = gate.program.evaluate(bad, [])
                assert got[1 + limb // (h // 2)] != 0 and got[0] == 0
                assert (got[3 + limb] != 0) == (value == 4)
    if field == N.GB_GOLDILOCKS:
        assert top * top + top == p - 1
    # the limbs come from the halves: a generator with another mask fails the first constraint alone
    words = [top - 1 if w == top else w for w in prog.words]
    assert words != prog.words
    outs = GeneratorProgram(words, field).evaluate([top, 1, 0])
    got = gate.program.evaluate([top, 1, 0] + outs, [])
    assert got[0] != 0 and not any(got[1:])


def test_the_gadgets_refuse_widths_that_could_wrap():
    from plonky2_goldibear_amd.circuit_builder import CircuitBuilder
    import gadget_cases as GA
    with pytest.raises(ValueError):
        mul_add_split_gate(N.GB_BABYBEAR, 16)
    with pytest.raises(ValueError):
        mul_add_split_gate(N.GB_GOLDILOCKS, 34)
    with pytest.raises(ValueError):
        mul_add_split_gate(N.GB_GOLDILOCKS, 7)
    assert mul_add_split_gate(N.GB_GOLDILOCKS, 16).num_wires == 21 and mul_add_split_gate(N.GB_GOLDILOCKS, 16) == mul_add_split_gate(N.GB_GOLDILOCKS, 16)
    assert mul_add_split_gate(N.GB_GOLDILOCKS, 16) != mul_add_split_gate(N.GB_GOLDILOCKS)
    b = CircuitBuilder(GA.config(N.GB_BABYBEAR))
    x, y = b.add_virtual_target(), b.add_virtual_target()
    with pytest.raises(ValueError):
        IG.div_rem(b, x, y, 16)            # (2^16 - 1)^2 + 2^16 - 1 > p: q * y + r could wrap
    with pytest.raises(ValueError):
        IG.is_less_than(b, x, y, 30)       # 2^31 > p
    assert b.num_gates() == 0 and not b.generators
    q, r = IG.div_rem(b, x, y, 15)
    assert [g.id for g in b.generators if isinstance(g, GP.ProgramGenerator)] == ["DivRemGenerator", "LessThanGenerator"]
