"""Circuits whose witness generators are generator programs (plonky2_goldibear_amd/generator_program.py), for the tests of
GB_GEN_PROGRAM through the library: a circuit of MulAddThreeGate rows (a gate of the user's own, constraints and generator both
as data), the poly-chain circuit with its ArithmeticGate as a program gate WITH generator programs (tests/gate_programs.py
with_program_gates leaves the built-in generators in place), and examples/square_root.rs.  No GPU code."""
from circuits import poly_chain_circuit
import gate_programs as GP
from plonky2_goldibear_amd import GateProgram, GeneratorProgram, ProgramGate, ProgramGenerator
from plonky2_goldibear_amd.circuit_builder import ArithmeticGate, CircuitBuilder, NoopGate, PartialWitness, wire


def mul_add_three_gate(field):
    """out = c0 * a * b + 3 with a a bit: README's example gate, completed with its generator"""
    constraints = GateProgram.from_constraints(lambda w, c: [w[2] - (w[0] * w[1] * c[0] + 3), w[0] * (w[0] - 1)],
                                               num_wires=3, num_constants=1, field=field)
    generator = GeneratorProgram.from_function(lambda d, c, ops: [d[0] * d[1] * c[0] + 3], num_in=2, num_out=1, num_constants=1, field=field)
    return ProgramGate("MulAddThreeGate", constraints, generators=lambda row, consts: [
        ProgramGenerator("MulAddThreeGenerator", generator, [wire(row, 0), wire(row, 1)], [wire(row, 2)], row=row)])


def mul_add_three_circuit(config, rows, pad_to=None, public_output=False):
    """`rows` MulAddThreeGate rows, each with its own constant, the output of one the second factor of the next; the last output
    is tied to its value as a constant.  public_output: the last output is a public input too, so build() hashes it and the gate
    set gains the permutation gate, whose degree of 7 leaves no room for five gates under one selector: the built circuit has two
    selector columns in front of its constants columns.  -> (builder, partial witness)"""
    b, pw = CircuitBuilder(config), PartialWitness()
    p, gate = b.F.p, mul_add_three_gate(config.field)
    start = b.add_virtual_target()
    pw.set_target(start, 6)
    val, prev = 6, start
    for r in range(rows):
        k, bit = 5 + 3 * r, (r + 1) & 1
        row = b.add_gate(gate, constants=[k])
        a = b.add_virtual_target()
        pw.set_target(a, bit)
        b.connect(a, wire(row, 0))
        b.connect(prev, wire(row, 1))
        prev, val = wire(row, 2), (k * bit * val + 3) % p
    b.connect(prev, b.constant(val))
    if public_output:
        b.register_public_input(prev)
    # build() adds the public-input gate and one ConstantGate, and for a public input one permutation row
    while pad_to and b.num_gates() + 2 + bool(public_output) < pad_to:
        b.add_gate(NoopGate())
    return b, pw


def with_generated_program_gates(builder):
    """tests/gate_programs.py with_program_gates for the ArithmeticGate, whose generators become generator programs too: one
    program (m0 * m1 * c0 + addend * c1) for every operation of every row"""
    field = builder.config.field
    program = GeneratorProgram.from_function(lambda d, c, ops: [d[0] * d[1] * c[0] + d[2] * c[1]], num_in=3, num_out=1, num_constants=2, field=field)
    cache = {}

    def conv(g):
        if not isinstance(g, ArithmeticGate):
            return g
        if g.id not in cache:
            def generators(row, consts, num_ops=g.num_ops):
                return [ProgramGenerator("ArithmeticBaseGenerator", program, [wire(row, 4 * i + k) for k in range(3)], [wire(row, 4 * i + 3)], row=row)
                        for i in range(num_ops)]
            cache[g.id] = ProgramGate(g.id, GP.program_of(g, field), generators=generators, degree=g.degree, num_ops=g.num_ops)
        return cache[g.id]

    builder.gates = {conv(g) for g in builder.gates}
    for inst in builder.gate_instances:
        inst[0] = conv(inst[0])
    return builder


def poly_chain_pair(config, steps):
    """-> (the poly-chain circuit's builder as it is, the same with program gates and generator programs, partial witness)"""
    b0, pw = poly_chain_circuit(config, steps)
    b1, _ = poly_chain_circuit(config, steps)
    return b0, with_generated_program_gates(b1), pw


def sqrt_program(field):
    return GeneratorProgram.from_function(lambda d, c, ops: [ops.sqrt(d[0])], num_in=1, num_out=1, num_constants=0, field=field)


def square_root_circuit(config, x_squared_value, pad_to=None):
    """examples/square_root.rs: x is a virtual target, x_squared = x * x a public input; the SquareRootGenerator computes x from
    x_squared outside the circuit.  -> (builder, partial witness, x, x_squared)"""
    b, pw = CircuitBuilder(config), PartialWitness()
    x = b.add_virtual_target()
    x_squared = b.square(x)
    b.register_public_input(x_squared)
    b.add_simple_generator(ProgramGenerator("SquareRootGenerator", sqrt_program(config.field), [x_squared], [x]))
    pw.set_target(x_squared, x_squared_value)
    while pad_to and b.num_gates() + 4 < pad_to:
        b.add_gate(NoopGate())
    return b, pw, x, x_squared


def inverse_circuit(config):
    """y_inv = 1 / y by a generator program with INV (the reference's inverse() divides and panics on zero); y * y_inv = 1 is
    constrained.  -> (builder, y)"""
    b = CircuitBuilder(config)
    y, y_inv = b.add_virtual_target(), b.add_virtual_target()
    prog = GeneratorProgram.from_function(lambda d, c, ops: [ops.inv(d[0])], num_in=1, num_out=1, num_constants=0, field=config.field)
    b.add_simple_generator(ProgramGenerator("InverseGenerator", prog, [y], [y_inv]))
    b.connect(b.mul(y, y_inv), b.one())
    return b, y

