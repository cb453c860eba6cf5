"""Circuits as gb_circuit_set_partition / gb_circuit_set_generators receive them, for the generator harnesses that run without the
library (tests/sanitize/generator_schedule.cpp, tests/host_shim/generators.cpp): the word file of tests/sanitize/schedule_case.hpp,
the schedule those programs write back, and a three-kind interpreter of it (Arithmetic, Constant, Copy) in plain Python.  The
oracle is always the builder mirror (BuiltCircuit._run_generators / generate_partition_witness).  No GPU code."""
import numpy as np

from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness

OK, INVALID, UNSUPPORTED = 0, 1, 4
GROUP = 256                      # csrc/generator_ops.hpp
OUT_CHECK, OUT_SKIP = 0x80000000, 0xFFFFFFFF


def pack(num_targets, num_wires, degree_bits, order, ext_degree, rep_map, pis, gates, constants, records, inputs, values=None,
         group_width=GROUP):
    """one case of the word file; gates = [(kind, param, param2, param3)], records = [(kind, gate, a, b)], constants [k][n]"""
    u = lambda x: np.asarray(x, dtype=np.uint64).reshape(-1)
    constants = u(constants)
    n = 1 << degree_bits
    assert constants.size % n == 0
    head = [num_targets, num_wires, degree_bits, constants.size // n, ext_degree, order, len(pis), len(gates), len(records), len(inputs),
            group_width, 0 if values is None else 1]
    parts = [u(head), u(rep_map), u(pis), u([x for g in gates for x in g]), constants, u([x for r in records for x in r]), u(inputs)]
    if values is not None:
        assert len(values) == len(inputs)
        parts.append(u(values))
    return np.concatenate(parts)


def built_inputs(built, pw):
    """the default input targets of BuiltCircuit.set_generators"""
    return list(pw.values) + [t for t in built.random_targets if t not in pw.values]


def pack_built(built, input_targets, values=None, records=None, **kw):
    """a BuiltCircuit (built without a context) as a case"""
    F = built.F
    gates = [(g[0], g[1], g[5], g[6]) for g in built.gate_table]
    return pack(built.num_targets, built.config.num_wires, built.degree_bits, F.p, F.ext_degree, built.representative_map,
                built.public_input_targets, gates, built.constants_columns, built.generator_records() if records is None else records,
                [built.target_index(t) for t in input_targets], values, **kw)


def write(path, cases):
    np.concatenate([np.array([len(cases)], dtype=np.uint64)] + list(cases)).tofile(path)


def read_schedule(out, pos, num_inputs, num_public_inputs):
    """one dump of schedule_case::dump -> (dict or status, new position)"""
    status = int(out[pos])
    pos += 1
    if status:
        return status, pos
    names = ("num_classes", "num_slots", "num_levels", "num_unrunnable", "num_checks", "num_launches", "num_ops")
    s = {k: int(v) for k, v in zip(names, out[pos:pos + 7])}
    pos += 7

    def take(count):
        nonlocal pos
        v = [int(x) for x in out[pos:pos + count]]
        pos += count
        return v

    s["class_reps"] = take(s["num_classes"])
    s["input_cls"], s["input_first"], s["input_free"] = take(num_inputs), take(num_inputs), take(num_inputs)
    s["pi_cls"] = take(num_public_inputs)
    s["launches"] = [tuple(take(3)) for _ in range(s["num_launches"])]
    s["level_off"] = take(s["num_levels"] + 1)
    ops = []
    for _ in range(s["num_ops"]):
        kind, record, p0, p1, k0, k1 = take(6)
        ins = take(take(1)[0])
        outs = take(take(1)[0])
        ops.append(dict(kind=kind, record=record, p0=p0, p1=p1, k=(k0, k1), ins=ins, outs=outs))
    s["ops"] = ops
    return s, pos


def level_of_op(s, index):
    """1-based level of op `index`"""
    return next(l for l in range(s["num_levels"]) if s["level_off"][l] <= index < s["level_off"][l + 1]) + 1


def interpret(s, input_values, p):
    """run a schedule of Arithmetic / Constant / Copy ops the way the kernels do - level by level, a store writes, a check
    compares - and return (values per class, [(record, class)] of failed checks).  Reads see only what EARLIER levels stored."""
    values = [0] * s["num_classes"]
    for i, cl in enumerate(s["input_cls"]):
        if s["input_first"][i] == i:
            values[cl] = int(input_values[i])
    failed = []
    for l in range(s["num_levels"]):
        before = list(values)
        for op in s["ops"][s["level_off"][l]:s["level_off"][l + 1]]:
            x = [before[c] for c in op["ins"]]
            if op["kind"] == N.GB_GEN_ARITHMETIC:
                v = (x[0] * x[1] * op["k"][0] + x[2] * op["k"][1]) % p
            elif op["kind"] == N.GB_GEN_CONSTANT:
                v = op["k"][0]
            elif op["kind"] == N.GB_GEN_COPY:
                v = x[0]
            else:
                raise ValueError("interpret() knows three kinds, not %d" % op["kind"])
            (w,) = op["outs"]
            if w == OUT_SKIP:
                continue
            if w & OUT_CHECK:
                if before[w & ~OUT_CHECK] != v:
                    failed.append((op["record"], w & ~OUT_CHECK))
            else:
                values[w] = v
    return values, failed


def mirror_class_values(built, s, pw, rng=None):
    """the mirror's partition witness at the classes of a schedule"""
    want = built.generate_partition_witness(pw, rng)
    return [int(want[t]) for t in s["class_reps"]]


def read_values(got, count, gathered=None):
    """the output of tests/host_shim/generators.cpp (gathered=None) or tests/device/generators.hip (gathered = [public inputs per
    case]) -> per case a status or dict(class_reps, values, err, num_levels, num_launches, num_unrunnable, public)"""
    res, pos = [], 0
    for k in range(count):
        status = int(got[pos])
        pos += 1
        if status:
            res.append(status)
            continue
        nc, levels, launches, unrunnable = (int(x) for x in got[pos:pos + 4])
        pos += 4
        reps = got[pos:pos + nc].astype(np.int64)
        values = got[pos + nc:pos + 2 * nc]
        err = [int(x) for x in got[pos + 2 * nc:pos + 2 * nc + 4]]
        pos += 2 * nc + 4
        public = None
        if gathered is not None:
            public = got[pos:pos + gathered[k]]
            pos += gathered[k]
        res.append(dict(class_reps=reps, values=values, err=err, num_levels=levels, num_launches=launches, num_unrunnable=unrunnable,
                        public=public))
    assert pos == len(got)
    return res


# ------------------------------------------------------------------------------------------------ synthetic circuits for the kernels
class _Rows:
    """what a generator's record() asks of a built circuit: rows that all hold gate 0 of a one-gate table, an identity map"""

    def __init__(self, num_wires, nrows):
        self.num_wires, self.row_gates = num_wires, [0] * nrows

    def target_index(self, t):
        assert t[0] == "w"
        return t[1] * self.num_wires + t[2]


def instance_rows(field, gate, nrows, seed):
    """`nrows` independent rows of one gate of tests/gate_variants.py's grid, every generator of the row listed: the rows' input
    wires carry the fields' carry-edge words, then random words (gate_variants.rows), narrowed only where the reference asserts
    (an access index below the vector size, a value that fits its limbs, a boolean swap, a nonzero coset shift).
    -> None for a gate without generators, else dict(gate, gens per row, input targets per row, values {target: word}, constants)"""
    import gate_variants as GV
    from oracle import gates as G
    from plonky2_goldibear_amd.circuit_builder import _ConstantGenerator, wire
    g = GV.gate_object(field, gate)
    F = GV.FIELDS[field]
    nw, nc, _ = GV.shape(field, gate)
    vals = GV.rows(field, gate, nrows, seed)
    kind = gate[0]
    if kind == G.RANDOM_ACCESS:
        for copy in range(g.num_copies):
            vals[g.wire_access_index(copy)] %= g.vec_size
    elif kind == G.BASE_SUM:
        vals[0] %= min(g.base ** g.num_limbs, F.P)
    elif kind == G.POSEIDON:
        vals[24] &= 1
    elif kind == G.POSEIDON2_BABYBEAR:
        for op in range(g.num_ops):
            vals[33 * op + 32] &= 1
    elif kind == G.COSET_INTERPOLATION:
        vals[0][vals[0] == 0] = 1
    rows = []
    for j in range(nrows):
        consts = [int(vals[nw + i, j]) for i in range(nc)]
        gens = list(g.generators(j, consts))
        for ci, wi in g.extra_constant_wires():
            cg = _ConstantGenerator(j, ci, wi)
            cg.constant = consts[ci]
            gens.append(cg)
        deps = []
        for gen in gens:
            for t in gen.deps:
                if t not in deps:
                    deps.append(t)
        rows.append((gens, deps, {t: int(vals[t[2], j]) for t in deps}))
    if not rows[0][0]:
        return None
    return dict(gate=gate, rows=rows, constants=vals[nw:nw + nc], num_wires=nw, field=field)


def mirror_row(inst, j, p):
    """the mirror's generators on row j -> {target: value} of everything set"""
    from plonky2_goldibear_amd.circuit_builder import _PartitionWitness
    gens, deps, values = inst["rows"][j]
    w = _PartitionWitness(lambda t: t, p, None)
    for t, v in values.items():
        w.set(t, v)
    for gen in gens:
        gen.run(w, p)
    return w.v


def pack_instances(inst, nrows, p, ext_degree):
    """the first nrows rows as a case: identity representative map over a one-gate circuit"""
    degree_bits = max(2, (nrows - 1).bit_length())
    n, nw = 1 << degree_bits, inst["num_wires"]
    stub = _Rows(nw, nrows)
    gate = inst["gate"]
    records, inputs, values = [], [], []
    for j in range(nrows):
        gens, deps, vals = inst["rows"][j]
        records += [gen.record(stub) for gen in gens]
        inputs += [stub.target_index(t) for t in deps]
        values += [vals[t] for t in deps]
    consts = np.zeros((inst["constants"].shape[0], n), dtype=np.uint64)
    consts[:, :nrows] = inst["constants"][:, :nrows]
    return pack(n * nw, nw, degree_bits, p, ext_degree, np.arange(n * nw, dtype=np.uint64), [], [(gate[0], gate[1], gate[5], gate[6])],
                consts, records, inputs, values)


def arithmetic_chain(field, depth, width, seed):
    """`width` independent chains of `depth` ArithmeticGate{1} rows: the output of a row is joined (copy class) to the first
    multiplicand of the row `width` further on, so level l of the schedule is rows l * width .. (l + 1) * width.
    -> (case words, expected {target: value} from the mirror's _ArithmeticGenerator)"""
    import gate_variants as GV
    from plonky2_goldibear_amd.circuit_builder import _ArithmeticGenerator, _PartitionWitness, wire
    from wired_circuits import edge_values
    F = GV.FIELDS[field]
    rows = depth * width
    degree_bits = max(2, (rows - 1).bit_length())
    n = 1 << degree_bits
    rep = np.arange(4 * n, dtype=np.uint64)
    for r in range(rows - width):
        rep[4 * (r + width)] = 4 * r + 3
    words = F.fill(seed, 5 * rows).astype(np.uint64)
    ev = np.array(edge_values(F), dtype=np.uint64)
    words[:min(len(ev), len(words))] = ev[:len(words)]
    consts = np.zeros((2, n), dtype=np.uint64)
    consts[0, :rows], consts[1, :rows] = words[3 * rows:4 * rows], words[4 * rows:5 * rows]
    find = lambda t: ("w", int(rep[4 * t[1] + t[2]]) // 4, int(rep[4 * t[1] + t[2]]) % 4)
    w = _PartitionWitness(find, F.P, None)
    inputs, values, records = [], [], []
    for r in range(rows):
        cols = (0, 1, 2) if r < width else (1, 2)
        for c in cols:
            inputs.append(4 * r + c)
            values.append(int(words[c * rows + r]))
            w.set(wire(r, c), values[-1])
        records.append((N.GB_GEN_ARITHMETIC, 0, r, 0))
    for r in range(rows):
        _ArithmeticGenerator(r, int(consts[0, r]), int(consts[1, r]), 0).run(w, F.P)
    case = pack(4 * n, 4, degree_bits, F.P, F.D, rep, [], [(3, 1, 0, 0)], consts, records, inputs, values)
    return case, {4 * t[1] + t[2]: v for t, v in w.v.items()}


# ------------------------------------------------------------------------------------------------ builder circuits
def wide_between_chains(width, chain=5, config=None):
    """a chain, then `width` independent operations that all read its end, then a chain over their sum's first terms"""
    b = CircuitBuilder(config or CircuitConfig.standard_recursion_config_gl())
    x = b.add_virtual_target()
    y = x
    for _ in range(chain):
        y = b.mul_add(y, y, x)
    factors = b.add_virtual_targets(width)      # inputs: distinct constants would make level 1 (the ConstantGenerators) wide
    wide = [b.mul_add(y, f, x) for f in factors]
    z = wide[0]
    for t in wide[1:chain]:
        z = b.mul_add(z, z, t)
    pw = PartialWitness()
    pw.set_target(x, 3)
    for i, f in enumerate(factors):
        pw.set_target(f, 1000 + 7 * i)
    return b, pw


def copy_circuit(second_value=None):
    """u, v inputs; two CopyGenerators write t (no copy constraint joins anything): t <- u and t <- v"""
    b = CircuitBuilder(CircuitConfig.standard_recursion_config_gl())
    u, v, t = b.add_virtual_target(), b.add_virtual_target(), b.add_virtual_target()
    b.generate_copy(u, t)
    b.generate_copy(v, t)
    out = b.mul(t, t)
    pw = PartialWitness()
    pw.set_target(u, 11)
    pw.set_target(v, 11 if second_value is None else second_value)
    return b, pw, (u, v, t, out)
