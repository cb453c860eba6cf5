"""Built-in gates written a second time as constraint programs (plonky2_goldibear_amd/gate_program.py), for the tests of
GB_GATE_PROGRAM: each function below restates a reference gate's eval_unfiltered with + - * on w[i], c[i] and integers, so it
runs on symbolic wires (GateProgram.from_constraints) and on Python integers alike (the direct evaluation the assembler is
compared against).  The reference lines are the ones csrc/gates.hpp lists:

    ArithmeticGate           gates/arithmetic_base.rs:83-100      ArithmeticExtensionGate  gates/arithmetic_extension.rs:82-100
    MulExtensionGate         gates/multiplication_extension.rs:77-94   BaseSumGate<B>      gates/base_sum.rs:77-93
    ReducingGate             gates/reducing.rs:89-115             ReducingExtensionGate    gates/reducing_extension.rs:95-120
    RandomAccessGate         gates/random_access.rs:150-200       PoseidonMdsGate          gates/poseidon_goldilocks_mds.rs:152-180
    AddManyGate              gates/add_many.rs:80-90              ExponentiationGate       gates/exponentiation.rs:99-135
    ApplyMat4Gate            gates/apply_mat4.rs:80-108

A D-tuple of wires is an element of F[x]/(x^D - W) (plonk/vars.rs); its product is spelled out in base operations."""
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import recursion_gates as R
from plonky2_goldibear_amd.circuit_builder import ArithmeticGate, _poseidon_tables
from plonky2_goldibear_amd.gate_program import GateProgram, ProgramGate

P = {N.GB_GOLDILOCKS: 0xFFFFFFFF00000001, N.GB_BABYBEAR: 2013265921}
EXT = {N.GB_GOLDILOCKS: (2, 7), N.GB_BABYBEAR: (4, 11)}   # D, W


def tup(w, start, D):
    return [w[start + k] for k in range(D)]


def ext_mul(a, b, W):
    D, out = len(a), []
    for k in range(D):
        lo = sum(a[i] * b[k - i] for i in range(k + 1))
        hi = sum(a[i] * b[k + D - i] for i in range(k + 1, D))
        out.append(lo + W * hi if k + 1 < D else lo)
    return out


def ext_add(a, b):
    return [x + y for x, y in zip(a, b)]


def ext_sub(a, b):
    return [x - y for x, y in zip(a, b)]


def ext_scale(a, s):
    return [x * s for x in a]


def arithmetic(num_ops):
    def fn(w, c):
        return [w[4 * i + 3] - (w[4 * i] * w[4 * i + 1] * c[0] + w[4 * i + 2] * c[1]) for i in range(num_ops)]
    return fn


def arithmetic_extension(num_ops, field, with_addend=True):
    D, W = EXT[field]
    stride = (4 if with_addend else 3) * D

    def fn(w, c):
        out = []
        for i in range(num_ops):
            m0, m1 = tup(w, stride * i, D), tup(w, stride * i + D, D)
            computed = ext_scale(ext_mul(m0, m1, W), c[0])
            if with_addend:
                computed = ext_add(computed, ext_scale(tup(w, stride * i + 2 * D, D), c[1]))
            out += ext_sub(tup(w, stride * i + stride - D, D), computed)
        return out
    return fn


def base_sum(num_limbs, base):
    def fn(w, c):
        acc = 0
        for i in reversed(range(num_limbs)):
            acc = acc * base + w[1 + i]
        out = [acc - w[0]]
        for i in range(num_limbs):
            prod = w[1 + i]
            for b in range(1, base):
                prod = prod * (w[1 + i] - b)
            out.append(prod)
        return out
    return fn


def reducing(num_coeffs, field, extension_coeffs):
    D, W = EXT[field]
    start_coeffs = 3 * D
    start_accs = start_coeffs + num_coeffs * (D if extension_coeffs else 1)

    def fn(w, c):
        alpha, acc, out = tup(w, D, D), tup(w, 2 * D, D), []
        for i in range(num_coeffs):
            coeff = tup(w, start_coeffs + i * D, D) if extension_coeffs else [w[start_coeffs + i]] + [0] * (D - 1)
            acc_i = tup(w, 0 if i == num_coeffs - 1 else start_accs + D * i, D)
            out += ext_sub(ext_add(ext_mul(acc, alpha, W), coeff), acc_i)
            acc = acc_i
        return out
    return fn


def random_access(bits, num_copies, num_extra):
    vec = 1 << bits
    routed = (2 + vec) * num_copies + num_extra

    def fn(w, c):
        out = []
        for copy in range(num_copies):
            base, bit0 = (2 + vec) * copy, routed + copy * bits
            b = [w[bit0 + i] for i in range(bits)]
            out += [x * (x - 1) for x in b]
            rec = 0
            for i in reversed(range(bits)):
                rec = rec + rec + b[i]
            out.append(rec - w[base])
            items = [w[base + 2 + i] for i in range(vec)]
            for lvl in range(bits):
                items = [x + b[lvl] * (y - x) for x, y in zip(items[0::2], items[1::2])]
            out.append(items[0] - w[base + 1])
        out += [c[i] - w[(2 + vec) * num_copies + i] for i in range(num_extra)]
        return out
    return fn


def poseidon_mds():
    D, W = EXT[N.GB_GOLDILOCKS]
    T = _poseidon_tables()
    circ, diag = T["MDS_CIRC"], T["MDS_DIAG"]

    def fn(w, c):
        out = []
        for r in range(12):
            res = ext_scale(tup(w, r * D, D), circ[0] + diag[r])
            for i in range(1, 12):
                res = ext_add(res, ext_scale(tup(w, ((r + i) % 12) * D, D), circ[i]))
            out += ext_sub(tup(w, (12 + r) * D, D), res)
        return out
    return fn


def add_many(num_addends, num_ops):
    def fn(w, c):
        return [sum(w[(num_addends + 1) * i + j] for j in range(num_addends)) - w[(num_addends + 1) * i + num_addends]
                for i in range(num_ops)]
    return fn


def exponentiation(nbits):
    def fn(w, c):
        base, prev, out = w[0], 1, []
        for i in range(nbits):
            bit, inter = w[1 + (nbits - i - 1)], w[2 + nbits + i]
            out.append(prev * (bit * base + (1 - bit)) - inter)
            prev = inter * inter
        out.append(w[1 + nbits] - w[2 + nbits + nbits - 1])
        return out
    return fn


def apply_mat4(num_ops, field):
    D, _ = EXT[field]

    def fn(w, c):
        out = []
        for op in range(num_ops):
            base = op * 8 * D
            x = [tup(w, base + i * D, D) for i in range(4)]
            t01, t23 = ext_add(x[0], x[1]), ext_add(x[2], x[3])
            t0123 = ext_add(t01, t23)
            t01123, t01233 = ext_add(t0123, x[1]), ext_add(t0123, x[3])
            new = [ext_add(t01123, t01), ext_add(t01123, ext_add(x[2], x[2])), ext_add(t01233, t23),
                   ext_add(t01233, ext_add(x[0], x[0]))]
            for i in range(4):
                out += ext_sub(tup(w, base + (4 + i) * D, D), new[i])
        return out
    return fn


def constraints_of(gate, field):
    """the constraint function of a built-in gate object (circuit_builder / recursion_gates), or None when the helper has none"""
    if isinstance(gate, ArithmeticGate):
        return arithmetic(gate.num_ops)
    if isinstance(gate, R.MulExtensionGate):
        return arithmetic_extension(gate.num_ops, field, False)
    if isinstance(gate, R.ArithmeticExtensionGate):
        return arithmetic_extension(gate.num_ops, field, True)
    if isinstance(gate, R.BaseSumGate):
        return base_sum(gate.num_limbs, gate.base)
    if isinstance(gate, R.ReducingGate):
        return reducing(gate.num_coeffs, field, gate.EXTENSION_COEFFS)
    if isinstance(gate, R.RandomAccessGate):
        return random_access(gate.bits, gate.num_copies, gate.num_extra_constants)
    if isinstance(gate, R.PoseidonMdsGate):
        return poseidon_mds()
    if isinstance(gate, R.AddManyGate):
        return add_many(gate.num_addends, gate.num_ops)
    if isinstance(gate, R.ExponentiationGate):
        return exponentiation(gate.num_power_bits)
    if isinstance(gate, R.ApplyMat4Gate):
        return apply_mat4(gate.num_ops, field)
    return None


def program_of(gate, field):
    fn = constraints_of(gate, field)
    return None if fn is None else GateProgram.from_constraints(fn, gate.num_wires, gate.num_constants, field)


def program_gate(gate, field):
    """the same gate - id, degree, constant count, generators - with its constraints as a program; None if not covered"""
    prog = program_of(gate, field)
    if prog is None:
        return None
    return ProgramGate(gate.id, prog, generators=gate.generators, degree=gate.degree, num_ops=gate.num_ops,
                       extra_constant_wires=gate.extra_constant_wires())


def with_program_gates(builder):
    """Replace every gate of a CircuitBuilder that the helper covers by its program form, before build().  The ids are the
    same, so the sort order, the selectors and the circuit digest are."""
    field, cache = builder.config.field, {}

    def conv(g):
        if g.id not in cache:
            cache[g.id] = program_gate(g, field) or g
        return cache[g.id]

    builder.gates = {conv(g) for g in builder.gates}
    for inst in builder.gate_instances:
        inst[0] = conv(inst[0])
    return builder


def helper_gates(field):
    """one instance of every gate the helper writes, sized as the recursion configurations size them"""
    gl = field == N.GB_GOLDILOCKS
    gates = [ArithmeticGate(20 if gl else 10), R.ArithmeticExtensionGate(10 if gl else 2, field), R.MulExtensionGate(13 if gl else 3, field),
             R.BaseSumGate(63 if gl else 30, 2), R.BaseSumGate(10, 4), R.ReducingGate(43 if gl else 29, field),
             R.ReducingExtensionGate(33 if gl else 7, field), R.RandomAccessGate(4 if gl else 3, 4, 2, field),
             R.AddManyGate(7, 10 if gl else 5), R.ExponentiationGate(66 if gl else 39, field), R.ApplyMat4Gate(5 if gl else 1, field)]
    if gl:
        gates.append(R.PoseidonMdsGate())
    return gates
