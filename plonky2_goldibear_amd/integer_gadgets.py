"""u32-style gates and gadgets whose witness generators are generator programs with the integer operations (generator_program.py:
IDIV, IREM, SHR, AND, LT on the canonical representatives), so that a circuit with them proves from its inputs alone.

    gate = mul_add_split_gate(N.GB_GOLDILOCKS)            # a * b + c = low + 2^32 * high, both halves in two-bit limbs
    row = builder.add_gate(gate)
    q, r = div_rem(builder, x, y, 16)                     # x = q * y + r, r < y
    lt = is_less_than(builder, x, y, 16)

The constraints are polynomial (a GateProgram, ArithmeticGate rows and BaseSumGate range checks); only the generators read a
target as an integer.  Not the GPU hot path.
"""
from . import native as N
from .circuit_builder import wire
from .gate_program import GateProgram, ProgramGate, field_order
from .generator_program import GeneratorProgram, ProgramGenerator

HALF_BITS = {N.GB_GOLDILOCKS: 32, N.GB_BABYBEAR: 14}


def _half_bits(field, half_bits):
    h = HALF_BITS[field] if half_bits is None else half_bits
    # (2^h - 1)^2 + 2^h - 1 = 2^(2h) - 2^h: the largest a * b + c of operands below 2^h must be a field element
    if h <= 0 or h % 2 or (1 << 2 * h) - (1 << h) >= field_order(field):
        raise ValueError("half_bits = %d: an even number of bits with 2^(2h) - 2^h below the field's order" % h)
    return h


def mul_add_split_program(field, half_bits=None):
    """the generator of mul_add_split_gate: (a, b, c) -> low, high, the limbs of low, the limbs of high.  The limbs are read off
    the halves, not off the product."""
    h = _half_bits(field, half_bits)

    def fn(d, c, ops):
        x = d[0] * d[1] + d[2]
        low, high = ops.low_bits(x, h), ops.shr(x, h)
        return [low, high] + [ops.and_(half if i == 0 else ops.shr(half, 2 * i), 3) for half in (low, high) for i in range(h // 2)]

    return GeneratorProgram.from_function(fn, num_in=3, num_out=2 + h, num_constants=0, field=field)


def mul_add_split_gate(field, half_bits=None, generator_program=None):
    """u32 multiply-add with a carry.  Wires: a, b, c, low, high, then half_bits two-bit limbs (half_bits / 2 of low, then of
    high, least significant first).  Constraints: a * b + c - (low + 2^half_bits * high); each half minus its limb sum;
    l (l - 1)(l - 2)(l - 3) for each limb.  half_bits defaults to 32 for Goldilocks - (2^32 - 1)^2 + 2^32 - 1 = p - 1, the product
    cannot wrap - and to 14 for BabyBear (2^28 + 2^14 < p).  a, b and c below 2^half_bits are the caller's to ensure.
    generator_program: another program in mul_add_split_program's place (tests)."""
    h = _half_bits(field, half_bits)
    n = h // 2

    def constraints(w, c):
        a, b, cc, low, high = w[0], w[1], w[2], w[3], w[4]
        limbs = [[w[5 + k * n + i] for i in range(n)] for k in range(2)]
        out = [a * b + cc - (low + high * (1 << h))]
        for half, ls in zip((low, high), limbs):
            acc = ls[-1]
            for l in reversed(ls[:-1]):
                acc = acc * 4 + l
            out.append(half - acc)
        return out + [l * (l - 1) * (l - 2) * (l - 3) for ls in limbs for l in ls]

    program = GateProgram.from_constraints(constraints, num_wires=5 + h, num_constants=0, field=field)
    generator = generator_program or mul_add_split_program(field, h)
    return ProgramGate("MulAddSplitGate { half_bits: %d }" % h, program, generators=lambda row, consts: [
        ProgramGenerator("MulAddSplitGenerator", generator, [wire(row, 0), wire(row, 1), wire(row, 2)],
                         [wire(row, 3 + i) for i in range(2 + h)])])


def is_less_than(builder, x, y, num_bits):
    """-> a bool target that is 1 iff x < y, for x and y of num_bits bits (both are range-checked).  The generator is LT; the
    constraint: y - x - 1 + (1 - lt) * 2^num_bits has num_bits bits, which for x < y (y - x - 1 in [0, 2^n - 2]) forces lt = 1
    and for x >= y (y - x - 1 in [-2^n, -1]) forces lt = 0.  Needs 2^(num_bits + 1) below the field's order."""
    p = builder.F.p
    if num_bits <= 0 or (1 << (num_bits + 1)) >= p:
        raise ValueError("num_bits = %d: 2^(num_bits + 1) must be below the field's order" % num_bits)
    program = GeneratorProgram.from_function(lambda d, c, ops: [ops.lt(d[0], d[1])], num_in=2, num_out=1, num_constants=0,
                                             field=builder.config.field)
    lt = builder.add_virtual_bool_target_safe()
    builder.add_simple_generator(ProgramGenerator("LessThanGenerator", program, [x, y], [lt]))
    builder.range_check(x, num_bits)
    builder.range_check(y, num_bits)
    diff = builder.arithmetic(p - (1 << num_bits), 1, lt, builder.one(), builder.sub(y, x))   # y - x - lt * 2^n
    builder.range_check(builder.add_const(diff, (1 << num_bits) - 1), num_bits)
    return lt


def div_rem(builder, x, y, num_bits):
    """-> (q, r) with x = q * y + r and r < y, for q, r and y of num_bits bits.  One generator program (IDIV, IREM); y = 0 has
    no witness: the generator reports "attempt to divide by zero".  q * y + r is at most 2^(2 num_bits) - 2^num_bits, which must
    be below the field's order, so that the equation holds over the integers."""
    if num_bits <= 0 or (1 << 2 * num_bits) - (1 << num_bits) >= builder.F.p:
        raise ValueError("num_bits = %d: 2^(2 num_bits) - 2^num_bits must be below the field's order" % num_bits)
    program = GeneratorProgram.from_function(lambda d, c, ops: [ops.idiv(d[0], d[1]), ops.irem(d[0], d[1])], num_in=2, num_out=2,
                                             num_constants=0, field=builder.config.field)
    q, r = builder.add_virtual_target(), builder.add_virtual_target()
    builder.add_simple_generator(ProgramGenerator("DivRemGenerator", program, [x, y], [q, r]))
    builder.connect(builder.mul_add(q, y, r), x)
    builder.range_check(q, num_bits)
    builder.assert_one(is_less_than(builder, r, y, num_bits))   # range-checks r and y
    return q, r
