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
SPACE_DEP = SPACE_WIRE   # space 1 indexes the dependencies
_BINARY = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL}
_UNARY = {"inv": OP_INV, "inv_or_zero": OP_INV_OR_ZERO, "is_zero": OP_IS_ZERO, "sqrt": OP_SQRT}
TWO_ADICITY = {N.GB_GOLDILOCKS: 32, N.GB_BABYBEAR: 27}
TWO_ADIC_GENERATOR = {N.GB_GOLDILOCKS: 1753635133440165772, N.GB_BABYBEAR: 0x1a427a41}   # csrc/gl_field.hpp, csrc/bb_field.hpp


class InvertZeroError(ArithmeticError):
    """INV of zero: the reference's "Tried to invert zero\""""


class NoSquareRootError(ArithmeticError):
    """SQRT of a non-residue: examples/square_root.rs sqrt(x).unwrap() on None"""


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


class _Ops:
    """the unary operations of a generator program, on the expressions of one trace"""

    def __init__(self, dag):
        self._dag = dag

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
        ops.inv / ops.inv_or_zero / ops.is_zero / ops.sqrt"""
        if num_in + num_out > MAX_TARGETS:
            raise ValueError("%d dependencies and %d outputs, together at most %d" % (num_in, num_out, MAX_TARGETS))
        dag = _Dag(field_order(field))
        outs = [dag.coerce(e) for e in fn(_Column(dag, "w", num_in), _Column(dag, "c", num_constants), _Ops(dag))]
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
