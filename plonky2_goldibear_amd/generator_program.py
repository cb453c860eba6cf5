"""Witness generators as data: generator programs for GB_GEN_PROGRAM (include/goldibear_gpu.h, "generator programs").

The reference hands a custom witness generator over as code in two places: `Gate::generators()` of a gate of the user's own
(plonky2/src/gates/gate.rs) and `CircuitBuilder::add_simple_generator` (examples/square_root.rs).  A generator whose run_once is
field arithmetic on its dependencies - with an inverse, a zero test or a square root here and there - is a straight-line program,
the counterpart of the constraint programs of gate_program.py and in their word layout; the library runs it in the generator
kernels (csrc/generators.hpp gen_program), so that a circuit with such generators proves from its inputs alone.

    prog = GeneratorProgram.from_function(lambda d, c, ops: [d[0] * d[1] * c[0] + 3], num_in=2, num_out=1, num_constants=1,
                                          field=N.GB_GOLDILOCKS)
    gate = ProgramGate("MulAddThreeGate", constraints, generators=lambda row, consts: [
        ProgramGenerator("MulAddThreeGenerator", prog, [wire(row, 0), wire(row, 1)], [wire(row, 2)], row=row)])

A generator that reads a target as an integer - a u32 multiply-add's low and high halves, a borrow, a comparison, range-check
limbs, div_rem - uses the integer operations ops.idiv / irem / shr / and_ / lt (opcodes 16 .. 20, on the canonical
representatives; integer_gadgets.py builds gates and gadgets on them), and ops.ext spells extension arithmetic out in base
operations.

`from_function` traces the callable on the DAG of gate_program.py (hash-consed, registers allocated by last use); `evaluate`
runs the packed words on Python integers, and is what ProgramGenerator.run calls: the host path prove(pw) and the device path
prove_inputs(pw) share one definition.  Not the GPU hot path.
"""
import numpy as np

from . import native as N
from .gate_program import (HEADER_WORDS, MAX_INSTRS, MAX_LITERALS, MAX_REGS, SPACE_CONST, SPACE_LIT, SPACE_REG, SPACE_WIRE, Expr,
                           _Column, _Dag, _operand, field_order)

MAX_GENERATOR_PROGRAMS, MAX_TARGETS = 256, 1024
OP_ADD, OP_SUB, OP_MUL, OP_OUT, OP_INV, OP_INV_OR_ZERO, OP_IS_ZERO, OP_SQRT = range(8)
OP_IDIV, OP_IREM, OP_SHR, OP_AND, OP_LT = range(16, 21)   # on the canonical representatives, as integers; 8 .. 15 are no opcodes
SPACE_DEP = SPACE_WIRE   # space 1 indexes the dependencies
_INTEGER = {"idiv": OP_IDIV, "irem": OP_IREM, "shr": OP_SHR, "and": OP_AND, "lt": OP_LT}
_BINARY = dict({"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL}, **_INTEGER)
EXT_W = {N.GB_GOLDILOCKS: (2, 7), N.GB_BABYBEAR: (4, 11)}   # the extension x^D - W: (D, W)
_UNARY = {"inv": OP_INV, "inv_or_zero": OP_INV_OR_ZERO, "is_zero": OP_IS_ZERO, "sqrt": OP_SQRT}
TWO_ADICITY = {N.GB_GOLDILOCKS: 32, N.GB_BABYBEAR: 27}
TWO_ADIC_GENERATOR = {N.GB_GOLDILOCKS: 1753635133440165772, N.GB_BABYBEAR: 0x1a427a41}   # csrc/gl_field.hpp, csrc/bb_field.hpp


class InvertZeroError(ArithmeticError):
    """INV of zero: the reference's "Tried to invert zero\""""


class NoSquareRootError(ArithmeticError):
    """SQRT of a non-residue: examples/square_root.rs sqrt(x).unwrap() on None"""


class IntegerDivideByZeroError(ArithmeticError):
    """IDIV or IREM by zero: Rust's panic, "attempt to divide by zero\""""


def integer_op(op, a, b):
    """IDIV / IREM / SHR / AND / LT on two canonical representatives; every result is <= a or 0 or 1, so canonical"""
    if op in (OP_IDIV, OP_IREM):
        if b == 0:
            raise IntegerDivideByZeroError("attempt to divide by zero (IDIV / IREM in a generator program)")
        return a // b if op == OP_IDIV else a % b
    if op == OP_SHR:
        return 0 if b >= 64 else a >> b
    return a & b if op == OP_AND else int(a < b)


def encode_opcode(op):
    """the opcode's bits in an instruction word: (w & 3) | ((w >> 56) & 0xF) << 2"""
    return (op & 3) | (op >> 2) << 56


def decode_opcode(word):
    return (word & 3) | ((word >> 56) & 0xF) << 2


def field_sqrt(x, field):
    """sqrt of examples/square_root.rs:185-219 step for step, with z = two_adic_generator(TWO_ADICITY); None for a non-residue"""
    p, s = field_order(field), TWO_ADICITY[field]
    x %= p
    if x == 0:
        return 0
    if pow(x, (p - 1) // 2, p) != 1:
        return None
    t = (p - 1) >> s
    z = TWO_ADIC_GENERATOR[field]
    w = pow(x, (t - 1) // 2, p)
    x = w * x % p
    b = x * w % p
    v = s
    while b != 1:
        k, b2k = 0, b
        while b2k != 1:
            b2k = b2k * b2k % p
            k += 1
        w = z
        for _ in range(v - k - 1):
            w = w * w % p
        z = w * w % p
        b = b * z % p
        x = x * w % p
        v = k
    return x


class Ext:
    """An extension element over x^D - W as its D coordinate expressions (`coords`), spelled out in base operations: + - *,
    scaling by a base expression or integer, inv() and /.  The inverse goes through the norm down to the base field - one INV,
    which raises on zero what INV raises."""

    def __init__(self, ops, coords):
        self._ops, self.coords = ops, [ops._dag.coerce(c) for c in coords]
        if len(self.coords) != ops.ext_degree:
            raise ValueError("%d coordinates for an extension of degree %d" % (len(self.coords), ops.ext_degree))

    def _same(self, o):
        return isinstance(o, Ext) and o._ops is self._ops

    def _new(self, coords):
        return Ext(self._ops, coords)

    def _lift(self, o):
        return o if self._same(o) else self._new([o] + [0] * (len(self.coords) - 1))

    def __add__(self, o):
        return self._new([a + b for a, b in zip(self.coords, self._lift(o).coords)])

    __radd__ = __add__

    def __sub__(self, o):
        return self._new([a - b for a, b in zip(self.coords, self._lift(o).coords)])

    def __rsub__(self, o):
        return self._lift(o) - self

    def __neg__(self):
        return self._new([0 - a for a in self.coords])

    def __mul__(self, o):
        if not self._same(o):   # a base expression or an integer scales
            return self._new([a * o for a in self.coords])
        d, w = len(self.coords), self._ops.ext_w
        out = [0] * d
        for i, a in enumerate(self.coords):
            for j, b in enumerate(o.coords):
                out[(i + j) % d] = out[(i + j) % d] + (a * b if i + j < d else a * b * w)
        return self._new(out)

    __rmul__ = __mul__

    def inv(self):
        w, c = self._ops.ext_w, self.coords
        if len(c) == 2:      # (a0 + a1 x)(a0 - a1 x) = a0^2 - W a1^2
            conj, norm = [c[0], 0 - c[1]], c[0] * c[0] - c[1] * c[1] * w
        else:                # a = A + B x over y = x^2, y^2 = W: a (A - B x) = A^2 - y B^2 = n0 + n1 y, whose norm is n0^2 - W n1^2
            n0 = c[0] * c[0] + c[2] * c[2] * w - 2 * w * (c[1] * c[3])
            n1 = 2 * (c[0] * c[2]) - c[1] * c[1] - c[3] * c[3] * w
            half = self._new([c[0], 0 - c[1], c[2], 0 - c[3]]) * self._new([n0, 0, 0 - n1, 0])
            conj, norm = half.coords, n0 * n0 - n1 * n1 * w
        ninv = self._ops.inv(norm)
        return self._new([x * ninv for x in conj])

    def __truediv__(self, o):
        return self * self._lift(o).inv()

    def __rtruediv__(self, o):
        return self._lift(o) * self.inv()


class _Ops:
    """the operations of a generator program beyond + - *, on the expressions of one trace: the unary field operations, the
    binary integer operations (no folding: two integer arguments become two literals) and what is spelled out in those"""

    def __init__(self, dag, field=None):
        self._dag, self.field = dag, field
        self.ext_degree, self.ext_w = EXT_W.get(field, (0, 0))

    def _integer(self, kind, x, y):
        return self._dag.node((kind, self._dag.coerce(x).i, self._dag.coerce(y).i))

    def idiv(self, x, y):
        """floor(x / y) of the canonical representatives; y = 0 is an error"""
        return self._integer("idiv", x, y)

    def irem(self, x, y):
        """x mod y of the canonical representatives; y = 0 is an error"""
        return self._integer("irem", x, y)

    def shr(self, x, amount):
        """floor(x / 2^amount); the amount is a value like any other, 0 from 64 on"""
        return self._integer("shr", x, amount)

    def and_(self, x, y):
        return self._integer("and", x, y)

    def lt(self, x, y):
        """1 if x < y as integers, else 0"""
        return self._integer("lt", x, y)

    def low_bits(self, x, n):
        """x mod 2^n (n an integer with 2^n - 1 below the field's order)"""
        if not 0 <= n or (1 << n) - 1 >= self._dag.p:
            raise ValueError("2^%d - 1 is no field element" % n)
        return self.and_(x, (1 << n) - 1)

    def bit(self, x, i):
        return self.and_(x if isinstance(i, int) and i == 0 else self.shr(x, i), 1)

    def bits(self, x, n):
        """the n low bits of x, least significant first"""
        return [self.bit(x, i) for i in range(n)]

    def select(self, c, x, y):
        """x where c is 1, y where c is 0"""
        return c * (x - y) + y

    def ext(self, coords):
        """D expressions as one extension element (Ext)"""
        return Ext(self, coords)

    def _unary(self, kind, x):
        return self._dag.node((kind, self._dag.coerce(x).i))

    def inv(self, x):
        return self._unary("inv", x)

    def inv_or_zero(self, x):
        return self._unary("inv_or_zero", x)

    def is_zero(self, x):
        return self._unary("is_zero", x)

    def sqrt(self, x):
        return self._unary("sqrt", x)


class GeneratorProgram:
    """A packed generator program.  `words` is what crosses the ABI (header, literals, instructions)."""

    def __init__(self, words, field):
        self.words, self.field, self.p = [int(x) for x in words], field, field_order(field)
        w = self.words
        self.num_in, self.num_constants = w[0] & 0xFFFFFFFF, w[0] >> 32
        self.num_out = w[1] & 0xFFFFFFFF
        self.num_regs, self.num_literals = w[2] & 0xFFFFFFFF, w[2] >> 32
        self.num_instrs = w[3]

    @property
    def literals(self):
        return self.words[HEADER_WORDS:HEADER_WORDS + self.num_literals]

    @property
    def instructions(self):
        return self.words[HEADER_WORDS + self.num_literals:]

    @classmethod
    def from_function(cls, fn, num_in, num_out, num_constants, field):
        """fn(deps, consts, ops) -> the num_out outputs in order, built from deps[i], consts[i] and integers with + - * and
        ops.inv / ops.inv_or_zero / ops.is_zero / ops.sqrt, the integer operations ops.idiv / ops.irem / ops.shr / ops.and_ /
        ops.lt with ops.low_bits / ops.bit / ops.bits / ops.select built from them, and ops.ext"""
        if num_in + num_out > MAX_TARGETS:
            raise ValueError("%d dependencies and %d outputs, together at most %d" % (num_in, num_out, MAX_TARGETS))
        dag = _Dag(field_order(field))
        outs = [dag.coerce(e) for e in fn(_Column(dag, "w", num_in), _Column(dag, "c", num_constants), _Ops(dag, field))]
        if len(outs) != num_out:
            raise ValueError("the function returned %d outputs, not %d" % (len(outs), num_out))
        nodes = dag.nodes

        def is_op(i):
            return nodes[i][0] in _BINARY or nodes[i][0] in _UNARY

        # schedule: the operations each output needs, operands first, in the order of the outputs
        stream, seen = [], set()
        for e in outs:
            stack = [(e.i, False)]
            while stack:
                i, done = stack.pop()
                if not is_op(i):
                    continue
                if done:
                    stream.append(("op", i))
                elif i not in seen:
                    seen.add(i)
                    stack += [(i, True)] + [(j, False) for j in reversed(nodes[i][1:])]
            stream.append(("out", e.i))
        last = {}
        for pos, (what, i) in enumerate(stream):
            for j in (nodes[i][1:] if what == "op" else (i,)):
                if is_op(j):
                    last[j] = pos
        lits, lit_index = [], {}

        def operand(j):
            k = nodes[j]
            if k[0] == "w":
                return _operand(SPACE_DEP, k[1])
            if k[0] == "c":
                return _operand(SPACE_CONST, k[1])
            if k[0] == "lit":
                if k[1] not in lit_index:
                    lit_index[k[1]] = len(lits)
                    lits.append(k[1])
                return _operand(SPACE_LIT, lit_index[k[1]])
            return _operand(SPACE_REG, reg[j])

        reg, free, num_regs, instrs = {}, [], 0, []
        for pos, (what, i) in enumerate(stream):
            if what == "out":
                instrs.append(OP_OUT | operand(i) << 8)
                users = (i,)
            else:
                users = nodes[i][1:]
                packed = [operand(j) for j in users]
            for j in set(users):     # registers whose value dies here are free for the destination (operands are read first)
                if j in reg and last.get(j) == pos:
                    free.append(reg.pop(j))
            if what == "op":
                if free:
                    free.sort(reverse=True)
                    r = free.pop()
                else:
                    r, num_regs = num_regs, num_regs + 1
                    if num_regs > MAX_REGS:
                        raise ValueError("more than %d registers live at once" % MAX_REGS)
                reg[i] = r
                kind = nodes[i][0]
                op = _BINARY[kind] if kind in _BINARY else _UNARY[kind]
                instrs.append(encode_opcode(op) | r << 2 | packed[0] << 8 | (packed[1] << 32 if len(packed) > 1 else 0))
        if len(instrs) > MAX_INSTRS:
            raise ValueError("%d instructions, at most %d" % (len(instrs), MAX_INSTRS))
        if len(lits) > MAX_LITERALS:
            raise ValueError("%d literals, at most %d" % (len(lits), MAX_LITERALS))
        return cls([num_in | num_constants << 32, num_out, num_regs | len(lits) << 32, len(instrs)] + lits + instrs, field)

    def evaluate(self, deps, consts=()):
        """the outputs for one set of dependency values: the packed words, decoded and run on Python integers"""
        p, lits, regs, out = self.p, self.literals, [None] * self.num_regs, []

        def load(o):
            space, idx = o & 3, o >> 2
            v = regs[idx] if space == SPACE_REG else int(deps[idx]) % p if space == SPACE_DEP else \
                int(consts[idx]) % p if space == SPACE_CONST else lits[idx]
            if v is None:
                raise ValueError("register %d read before it is written" % idx)
            return v

        for word in self.instructions:
            op, dst, a = decode_opcode(word), (word >> 2) & 63, load((word >> 8) & 0xFFFFFF)
            if op == OP_OUT:
                out.append(a)
            elif op in (OP_ADD, OP_SUB, OP_MUL):
                b = load((word >> 32) & 0xFFFFFF)
                regs[dst] = (a + b) % p if op == OP_ADD else (a - b) % p if op == OP_SUB else a * b % p
            elif op in _INTEGER.values():
                regs[dst] = integer_op(op, a, load((word >> 32) & 0xFFFFFF))
            elif op == OP_INV:
                if a == 0:
                    raise InvertZeroError("Tried to invert zero")
                regs[dst] = pow(a, p - 2, p)
            elif op == OP_INV_OR_ZERO:
                regs[dst] = pow(a, p - 2, p)
            elif op == OP_IS_ZERO:
                regs[dst] = int(a == 0)
            elif op == OP_SQRT:
                r = field_sqrt(a, self.field)
                if r is None:
                    raise NoSquareRootError("called `Option::unwrap()` on a `None` value")
                regs[dst] = r
            else:
                raise ValueError("unknown opcode %d" % op)
        return out


def pack_generator_programs(programs):
    """[GeneratorProgram | list of words] -> (program_words uint64, program_offsets uint32[num_programs + 1])"""
    words, offsets = [], [0]
    for pr in programs:
        words += [int(x) for x in (pr.words if isinstance(pr, GeneratorProgram) else pr)]
        offsets.append(len(words))
    return np.array(words or [0], dtype=np.uint64), np.array(offsets, dtype=np.uint32)


class ProgramGenerator:
    """A SimpleGenerator whose run_once is a generator program: `deps` and `outs` are the targets of its dependencies and
    outputs (wires or virtual targets), `row` the row whose constants the program reads (None for a program without constants).
    For CircuitBuilder.add_simple_generator, and what a ProgramGate's generators(row, constants) callable returns.
    CircuitBuilder.build() numbers the distinct programs and gives the built circuit a copy bound to the row's constants
    (bound_to); the object handed to the builder is not changed."""

    def __init__(self, id, program, deps, outs, row=None):
        if len(deps) != program.num_in or len(outs) != program.num_out:
            raise ValueError("%s: %d dependencies and %d outputs, the program has %d and %d" %
                             (id, len(deps), len(outs), program.num_in, program.num_out))
        if program.num_constants and row is None:
            raise ValueError("%s: the program reads constants; name the row" % id)
        self.id, self.generator_program, self.deps, self.outs = id, program, list(deps), list(outs)
        self.row = row if program.num_constants else None
        self.constants = []

    def bound_to(self, constants):
        """a copy of this generator that reads `constants`, the constants of its row in one built circuit"""
        g = ProgramGenerator(self.id, self.generator_program, self.deps, self.outs, self.row)
        g.constants = list(constants)
        return g

    def record(self, built):
        targets = [built.target_index(t) for t in self.deps + self.outs]
        head = (N.GB_GEN_PROGRAM, built.generator_program_index(self.generator_program), len(targets), self.row or 0)
        return [head] + N.gadget_records(0, 0, targets)[1:]

    def run(self, w, p):
        for t, v in zip(self.outs, self.generator_program.evaluate([w.get(t) for t in self.deps], self.constants)):
            w.set(t, v)
