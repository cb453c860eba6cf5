"""Custom gates as data: constraint programs for GB_GATE_PROGRAM (include/goldibear_gpu.h, "constraint programs").

The reference's extension point is the `Gate` trait (plonky2/src/gates/gate.rs:53-272: eval_unfiltered, degree,
num_constraints).  A constraint of any gate is a polynomial in the row's wires and constants, so a straight-line program of
add / sub / mul describes the gate as data; the library runs it in the quotient kernel (csrc/kernels_gates.hip k_gate_programs)
and in gb_verify (csrc/gates.hpp run_program), the same words in both.

    prog = GateProgram.from_constraints(lambda w, c: [w[2] - (w[0] * w[1] * c[0] + 3)], num_wires=3, num_constants=1,
                                        field=N.GB_GOLDILOCKS)
    gate = ProgramGate("MulAddThreeGate", prog)
    row = builder.add_gate(gate, constants=[5])

`from_constraints` runs the callable once on symbolic wires: equal subexpressions become one node (hash-consing), the DAG is
scheduled in the order of the constraints, registers are allocated by last use (at most 32 live) and the instructions are
packed into the words the ABI takes.  `evaluate` runs the packed words on Python integers - an independent restatement of the
interpreter for tests and witness checks.  Not the GPU hot path.
"""
import numpy as np

from . import native as N
from .circuit_builder import Gate
from .dummy_circuit import BB_P, P as GL_P

GATE_PROGRAM = 18  # gb_gate.kind
MAX_PROGRAMS, MAX_INSTRS, MAX_REGS, MAX_LITERALS, MAX_CONSTRAINTS = 16, 4096, 32, 256, 1024
OP_ADD, OP_SUB, OP_MUL, OP_EMIT = 0, 1, 2, 3
SPACE_REG, SPACE_WIRE, SPACE_CONST, SPACE_LIT = 0, 1, 2, 3
HEADER_WORDS = 4
_OPS = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL}


def field_order(field):
    return GL_P if field == N.GB_GOLDILOCKS else BB_P


class _Dag:
    """The nodes of one assembly, hash-consed: a key is built once, so equal subexpressions are one node."""

    def __init__(self, p):
        self.p, self.nodes, self.index = p, [], {}

    def node(self, key):
        i = self.index.get(key)
        if i is None:
            i = self.index[key] = len(self.nodes)
            self.nodes.append(key)
        return Expr(self, i)

    def lit(self, v):
        return self.node(("lit", int(v) % self.p))

    def coerce(self, x):
        if isinstance(x, Expr):
            if x.dag is not self:
                raise ValueError("expression of another program")
            return x
        return self.lit(x)

    def op(self, kind, a, b):
        a, b = self.coerce(a), self.coerce(b)
        ka, kb = self.nodes[a.i], self.nodes[b.i]
        if ka[0] == "lit" and kb[0] == "lit":   # literals fold
            v = {"add": ka[1] + kb[1], "sub": ka[1] - kb[1], "mul": ka[1] * kb[1]}[kind]
            return self.lit(v)
        if kind == "add" and kb == ("lit", 0) or kind == "sub" and kb == ("lit", 0) or kind == "mul" and kb == ("lit", 1):
            return a
        if kind == "add" and ka == ("lit", 0) or kind == "mul" and ka == ("lit", 1):
            return b
        if kind == "mul" and (ka == ("lit", 0) or kb == ("lit", 0)):
            return self.lit(0)
        if kind != "sub" and a.i > b.i:         # add and mul commute: one key for both orders
            a, b = b, a
        return self.node((kind, a.i, b.i))


class Expr:
    """A symbolic value over w[i], c[i] and integer literals; +, -, * build the DAG."""
    __slots__ = ("dag", "i")

    def __init__(self, dag, i):
        self.dag, self.i = dag, i

    def __add__(self, o):
        return self.dag.op("add", self, o)

    def __radd__(self, o):
        return self.dag.op("add", o, self)

    def __sub__(self, o):
        return self.dag.op("sub", self, o)

    def __rsub__(self, o):
        return self.dag.op("sub", o, self)

    def __mul__(self, o):
        return self.dag.op("mul", self, o)

    def __rmul__(self, o):
        return self.dag.op("mul", o, self)

    def __neg__(self):
        return self.dag.op("sub", 0, self)


class _Column:
    def __init__(self, dag, space, n):
        self.dag, self.space, self.n = dag, space, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self.n))]
        if not 0 <= i < self.n:
            raise IndexError("%s[%d] of %d" % (self.space, i, self.n))
        return self.dag.node((self.space, int(i)))


def _operand(space, index):
    return space | (index << 2)


class GateProgram:
    """A packed constraint program.  `words` is what crosses the ABI (header, literals, instructions)."""

    def __init__(self, words, field):
        self.words, self.field, self.p = [int(x) for x in words], field, field_order(field)
        w = self.words
        self.num_wires, self.num_constants = w[0] & 0xFFFFFFFF, w[0] >> 32
        self.num_constraints, self.degree = w[1] & 0xFFFFFFFF, w[1] >> 32
        self.num_regs, self.num_literals = w[2] & 0xFFFFFFFF, w[2] >> 32
        self.num_instrs = w[3]
        self.max_live = self.num_regs

    @property
    def literals(self):
        return self.words[HEADER_WORDS:HEADER_WORDS + self.num_literals]

    @property
    def instructions(self):
        return self.words[HEADER_WORDS + self.num_literals:]

    @classmethod
    def from_constraints(cls, fn, num_wires, num_constants, field, degree=None):
        """fn(w, c) -> the constraints in the order of eval_unfiltered, built from w[i], c[i] and integers with + - *.
        degree: Gate::degree() when it is to be declared higher than the bound of the constraints."""
        dag = _Dag(field_order(field))
        outs = [dag.coerce(e) for e in fn(_Column(dag, "w", num_wires), _Column(dag, "c", num_constants))]
        degree, num_regs, lits, instrs = assemble(dag, outs, degree)
        header = [num_wires | num_constants << 32, len(outs) | degree << 32, num_regs | len(lits) << 32, len(instrs)]
        prog = cls(header + lits + instrs, field)
        return prog

    def evaluate(self, wires, constants=()):
        """The constraints of one row on Python integers: the packed words, decoded and run."""
        return run_words(self.p, self.literals, self.num_regs, self.instructions, wires, constants)


def assemble(dag, outs, degree=None, leaf_degree=lambda key: 1):
    """The constraints `outs` of one DAG as a program: schedule, registers, literals -> (degree, num_regs, literals, instruction
    words).  Leaves are ("w", i) (operand space 1) and ("c", i) (operand space 2) nodes; leaf_degree(key) is the degree bound of one
    (wires and constants: 1)."""
    if len(outs) > MAX_CONSTRAINTS:
        raise ValueError("%d constraints, at most %d" % (len(outs), MAX_CONSTRAINTS))
    nodes = dag.nodes
    # degree bounds: literal 0, wire and constant 1, add / sub the maximum, mul the sum
    deg = [0] * len(nodes)
    for i, k in enumerate(nodes):    # operands are created before the node that uses them
        deg[i] = 0 if k[0] == "lit" else leaf_degree(k) if k[0] in "wc" else deg[k[1]] + deg[k[2]] if k[0] == "mul" else max(deg[k[1]], deg[k[2]])
    bound = max([deg[e.i] for e in outs] or [0])
    if degree is None:
        degree = bound
    if bound > degree:
        raise ValueError("a constraint has degree bound %d, above the declared degree %d" % (bound, degree))
    # schedule: the operations each constraint needs, operands first, in the order of the constraints
    stream, seen = [], set()
    for e in outs:
        stack = [(e.i, False)]
        while stack:
            i, done = stack.pop()
            if nodes[i][0] not in _OPS:
                continue
            if done:
                stream.append(("op", i))
            elif i not in seen:
                seen.add(i)
                stack += [(i, True), (nodes[i][2], False), (nodes[i][1], False)]
        stream.append(("emit", e.i))
    # last use of every operation's value: a position in the stream of operations and EMITs
    last = {}
    for pos, (what, i) in enumerate(stream):
        for j in (nodes[i][1:] if what == "op" else (i,)):
            if nodes[j][0] in _OPS:
                last[j] = pos
    lits, lit_index = [], {}

    def operand(j):
        k = nodes[j]
        if k[0] == "w":
            return _operand(SPACE_WIRE, k[1])
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
        if what == "emit":
            instrs.append(OP_EMIT | operand(i) << 8)
            users = (i,)
        else:
            kind, a, b = nodes[i]
            oa, ob = operand(a), operand(b)
            users = (a, b)
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
                    raise ValueError("more than %d registers live at once; emit constraints earlier or split the gate" % MAX_REGS)
            reg[i] = r
            instrs.append(_OPS[kind] | r << 2 | oa << 8 | ob << 32)
    if len(instrs) > MAX_INSTRS:
        raise ValueError("%d instructions, at most %d" % (len(instrs), MAX_INSTRS))
    if len(lits) > MAX_LITERALS:
        raise ValueError("%d literals, at most %d" % (len(lits), MAX_LITERALS))
    return degree, num_regs, lits, instrs


def run_words(p, lits, num_regs, instructions, wires, constants=(), coerce=int):
    """Instruction words on Python integers: operand space 1 reads `wires`, space 2 `constants` -> the emitted values.  coerce: what
    an operand is made of (int; the identity runs the words on any values that have + - * and % p)"""
    regs, out = [None] * num_regs, []

    def load(o):
        space, idx = o & 3, o >> 2
        v = regs[idx] if space == SPACE_REG else coerce(wires[idx]) if space == SPACE_WIRE else \
            coerce(constants[idx]) if space == SPACE_CONST else lits[idx]
        if v is None:
            raise ValueError("register %d read before it is written" % idx)
        return v

    for word in instructions:
        op, dst, a = word & 3, (word >> 2) & 63, load((word >> 8) & 0xFFFFFF)
        if op == OP_EMIT:
            out.append(a % p)
            continue
        b = load((word >> 32) & 0xFFFFFF)
        regs[dst] = (a + b) % p if op == OP_ADD else (a - b) % p if op == OP_SUB else a * b % p
    return out


def pack_programs(programs):
    """[GateProgram | list of words] -> (program_words uint64, program_offsets uint32[num_programs + 1])"""
    words, offsets = [], [0]
    for pr in programs:
        words += [int(x) for x in (pr.words if isinstance(pr, GateProgram) else pr)]
        offsets.append(len(words))
    return np.array(words or [0], dtype=np.uint64), np.array(offsets, dtype=np.uint32)


class ProgramGate(Gate):
    """A gate of the user's own: `id` is the reference gate's id() string (it orders the gate set, circuit_builder.rs:1194-1196),
    the constraints are `program`; generators(row, constants) -> the row's witness generators, as for the built-in gates.
    CircuitBuilder.build() numbers the programs of the gate set in sorted order; that number is the gate's `param` in the
    built circuit's gate table (the gate object itself is not changed, so it may be added to several builders)."""
    kind = GATE_PROGRAM

    def __init__(self, id, program, generators=None, degree=None, num_ops=1, extra_constant_wires=()):
        self.id, self.program = id, program
        self.num_wires, self.num_constants = program.num_wires, program.num_constants
        self.num_constraints = program.num_constraints
        self.degree = program.degree if degree is None else degree
        if self.degree != program.degree:
            raise ValueError("the gate's degree is the one its program declares (%d)" % program.degree)
        self.num_ops, self._generators, self._extra = num_ops, generators, list(extra_constant_wires)
        self.param = 0

    def generators(self, row, constants):
        return self._generators(row, constants) if self._generators else []

    def extra_constant_wires(self):
        return self._extra
