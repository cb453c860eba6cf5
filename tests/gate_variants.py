"""The gate evaluators of csrc/gates.hpp at every parameter gb_circuit_create_gates accepts (prover_host.inc build_gate_set), in
one place: the grid of gate tuples, the rows the evaluators are run on, the oracle's answer, the word file the two harnesses
(tests/device/gate_eval.hip, tests/host_shim/gate_eval.cpp) read, and small circuits that hold one row of every buildable
variant.  No GPU code."""
import numpy as np

from oracle import gates as G
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import recursion_gates as R
from plonky2_goldibear_amd.circuit_builder import (ArithmeticGate, CircuitBuilder, CircuitConfig, ConstantGate, PartialWitness,
                                                   Poseidon2BabyBearGate, PoseidonGate, PublicInputGate, wire)

from wired_circuits import edge_values

FIELDS = {N.GB_GOLDILOCKS: GL, N.GB_BABYBEAR: BB}
GRID_SIZE = {N.GB_GOLDILOCKS: 89, N.GB_BABYBEAR: 90}
HEAVY, LIGHT = 1, 2   # gates::GateSubset: the quotient kernel's two launches
ROW_COUNTS = (1, 63, 64, 65, 300)

# (group_start, group_end, many_selectors) of the filter each grid entry is given in turn: groups of 1, 2 and 7 gates, with one
# and with several selector columns
FILTER_SHAPES = [(gs, gs + size, many) for many in (0, 1) for gs, size in ((0, 1), (4, 2), (3, 7))]


def interpolation_degrees(bits):
    """every degree CosetInterpolationGate::with_max_degree can yield (coset_interpolation.rs:70-99): the minimal degree for the
    number of intermediates that a requested maximum d' = 2 .. 2^bits leads to"""
    npts = 1 << bits
    out = set()
    for want in range(2, npts + 1):
        n_int = (npts - 2) // (want - 1)
        out.add((npts - 2) // (n_int + 1) + 2)
    return sorted(out)


def grid(field):
    """gate tuples (kind, param, selector, group_start, group_end, param2, param3).  The selector group of entry t is
    FILTER_SHAPES[t % 6], its own index own_index(gate) lies inside the group, its selector column is 0 or 1."""
    gl = field == N.GB_GOLDILOCKS
    g = [(G.CONSTANT, n, 0, 0) for n in (1, 2, 5)]
    g += [(G.PUBLIC_INPUT, 0, 0, 0)]
    g += [(G.ARITHMETIC, n, 0, 0) for n in (1, 3, 20)]
    g += [(G.POSEIDON, 0, 0, 0)] if gl else [(G.POSEIDON2_BABYBEAR, n, 0, 0) for n in (1, 2)]
    g += [(G.ARITHMETIC_EXTENSION, n, 0, 0) for n in (1, 3, 10)]
    g += [(G.MUL_EXTENSION, n, 0, 0) for n in (1, 4, 13)]
    g += [(G.BASE_SUM, limbs, base, 0) for base in (2, 3, 4, 5, 7, 8) for limbs in (1, 2, 17)]
    g += [(G.BASE_SUM, 63 if gl else 30, 2, 0), (G.BASE_SUM, 9, 0, 0)]     # param2 = 0 is read as base 2
    g += [(G.REDUCING, n, 0, 0) for n in (1, 2, 43)]
    g += [(G.REDUCING_EXTENSION, n, 0, 0) for n in (1, 2, 33)]
    g += [(G.RANDOM_ACCESS, bits, copies, extra) for bits in range(7) for copies, extra in ((1, 0), (2, 1), (3, 2))]
    g += [(G.POSEIDON_MDS, 0, 0, 0)] if gl else []
    g += [(G.COSET_INTERPOLATION, bits, d, 0) for bits in range(1, 5) for d in interpolation_degrees(bits)]
    g += [(G.EXPONENTIATION, n, 0, 0) for n in (1, 2, 13, 66)]
    g += [(G.ADD_MANY, a, ops, 0) for a, ops in ((1, 1), (1, 9), (2, 3), (7, 10), (40, 1))]
    g += [(G.APPLY_MAT4, n, 0, 0) for n in (1, 5)]
    g += [] if gl else [(G.POSEIDON2_INTERNAL_PERMUTATION, 0, 0, 0)]
    out = []
    for t, (kind, param, p2, p3) in enumerate(g):
        gs, ge, many = FILTER_SHAPES[t % len(FILTER_SHAPES)]
        out.append((kind, param, many * (t % 2), gs, ge, p2, p3))
    return out


def many_selectors(t):
    """whether grid entry t is filtered as in a circuit with several selector columns"""
    return FILTER_SHAPES[t % len(FILTER_SHAPES)][2]


def own_index(gate, t):
    """the gate's own index inside its selector group: first, last or in between, by its place t in the grid"""
    return gate[3] + (t // len(FILTER_SHAPES)) % (gate[4] - gate[3])


def oracle_gate(gate):
    """the tuple oracle/gates.py reads: it has no default for BaseSumGate's base"""
    if gate[0] == G.BASE_SUM and gate[5] == 0:
        return gate[:5] + (2,) + gate[6:]
    return gate


def subset(gate):
    return HEAVY if gate[0] in (G.POSEIDON, G.POSEIDON2_BABYBEAR) else LIGHT


def gate_object(field, gate):
    """the builder's gate struct (circuit_builder.py / recursion_gates.py) of a tuple: layouts, counts, witness generators"""
    kind, param, p2, p3 = gate[0], gate[1], gate[5], gate[6]
    F = FIELDS[field]
    if kind == G.CONSTANT:
        return ConstantGate(param)
    if kind == G.PUBLIC_INPUT:
        return PublicInputGate(F.hout)
    if kind == G.ARITHMETIC:
        return ArithmeticGate(param)
    if kind == G.POSEIDON:
        return PoseidonGate()
    if kind == G.POSEIDON2_BABYBEAR:
        return Poseidon2BabyBearGate(param)
    if kind == G.ARITHMETIC_EXTENSION:
        return R.ArithmeticExtensionGate(param, field)
    if kind == G.MUL_EXTENSION:
        return R.MulExtensionGate(param, field)
    if kind == G.BASE_SUM:
        return R.BaseSumGate(param, p2 or 2)
    if kind == G.REDUCING:
        return R.ReducingGate(param, field)
    if kind == G.REDUCING_EXTENSION:
        return R.ReducingExtensionGate(param, field)
    if kind == G.RANDOM_ACCESS:
        return R.RandomAccessGate(param, p2, p3, field)
    if kind == G.POSEIDON_MDS:
        return R.PoseidonMdsGate()
    if kind == G.COSET_INTERPOLATION:
        g = R.CosetInterpolationGate(param, field, max_degree=p2)
        assert g.degree == p2, (param, p2, g.degree)
        return g
    if kind == G.EXPONENTIATION:
        return R.ExponentiationGate(param, field)
    if kind == G.ADD_MANY:
        return R.AddManyGate(param, p2)
    if kind == G.APPLY_MAT4:
        return R.ApplyMat4Gate(param, field)
    if kind == G.POSEIDON2_INTERNAL_PERMUTATION:
        return R.Poseidon2InternalPermutationGate()
    raise ValueError(kind)


def shape(field, gate):
    """(num_wires, num_constants, num_constraints) by the builder's gate structs"""
    g = gate_object(field, gate)
    return g.num_wires, g.num_constants, g.num_constraints


def rows(field, gate, nrows, seed, width=1):
    """[num_wires + num_constants + 1][nrows * width] canonical words, as tests/test_device_gate_programs.py builds its rows: the
    edge words first (every column starts at another one), then random words.  The last column is the selector: the gate's own
    index is not known here, so the caller overwrites its first entries (selector_column)."""
    F = FIELDS[field]
    ev = np.array(edge_values(F), dtype=np.uint64)
    nw, nc, _ = shape(field, gate)
    ncols, n = nw + nc + 1, nrows * width
    vals = F.fill(seed, ncols * n).astype(np.uint64).reshape(ncols, n)
    k = min(n, len(ev))
    for col in range(ncols):
        vals[col, :k] = np.roll(ev, -col)[:k]
    return vals


def selector_column(field, gate, own, vals, width=1):
    """the selector column of rows(): the gate's own index, another index of its group, UNUSED_SELECTOR mod p, the edge words,
    then indices in and around the group and random words"""
    F = FIELDS[field]
    sel = vals[-1].reshape(-1, width)
    ev = edge_values(F)
    other = gate[3] if own != gate[3] else gate[4] - 1
    first = [own, other, G.UNUSED_SELECTOR % F.P] + ev + list(range(gate[3] - 1 if gate[3] else 0, gate[4] + 2))
    for j, v in enumerate(first[:len(sel)]):
        sel[j, 0] = v
        if width > 1 and j < 3:
            sel[j, 1:] = 0      # on the subgroup the selector is a base value: there the filter is exactly zero or not
    return vals


PI_HASH_SEED = 0x51


def pi_hash(field):
    F = FIELDS[field]
    ev = edge_values(F)
    return ([ev[-1], ev[4], 0] + [int(x) for x in F.fill(PI_HASH_SEED, F.hout)])[:F.hout]


def interpolation_tables(field):
    """GateSet::subgroup16 and inv_pow2 as canonical values, from the oracle's field: two_adic_subgroup(4) and 1 / 2^b"""
    F = FIELDS[field]
    g = F.two_adic_generator(4)
    return [pow(g, i, F.P) for i in range(16)], [F.finv(1 << b) for b in range(5)]


HEADER_WORDS, GATE_WORDS = 33, 13


def pack(field, nrows, width, entries):
    """the harnesses' input: entries = [(gate, own index, many selectors, values of rows(), ..)]"""
    F = FIELDS[field]
    sub, inv = interpolation_tables(field)
    words = [np.array([field, nrows, len(entries), width] + (pi_hash(field) + [0] * 8)[:8] + sub + inv, dtype=np.uint64)]
    assert len(words[0]) == HEADER_WORDS
    for gate, own, many, vals in (e[:4] for e in entries):
        nw, nc, ncons = shape(field, gate)
        assert vals.shape == (nw + nc + 1, nrows * width)
        words.append(np.array(list(gate) + [subset(gate), own, many, nw, nc, ncons], dtype=np.uint64))
        words.append(vals.reshape(-1))
    return np.concatenate(words)


def unpack(field, nrows, width, entries, out):
    """the harnesses' output -> per entry (figures, counts [nrows], constraints [ncons][nrows][width], filter [nrows][width]);
    figures = (num_wires, num_constraints, num_constants) of gates::num_* for the tuple"""
    res, pos = [], 0
    for gate in (e[0] for e in entries):
        ncons = shape(field, gate)[2]
        figures = tuple(int(x) for x in out[pos:pos + 3])
        pos += 3
        counts = out[pos:pos + nrows]
        pos += nrows
        cons = out[pos:pos + ncons * nrows * width].reshape(ncons, nrows, width)
        pos += ncons * nrows * width
        filt = out[pos:pos + nrows * width].reshape(nrows, width)
        pos += nrows * width
        res.append((figures, counts, cons, filt))
    assert pos == len(out), (pos, len(out))
    return res


def reference(field, gate, own, many, vals, nrows, width):
    """oracle/gates.py on every row -> (constraints [nrows][ncons] of D-tuples, filters [nrows] of D-tuples).  width 1: base values
    passed as F.efrom(v); width D: every wire, constant and selector a D-tuple."""
    F = FIELDS[field]
    nw, nc, ncons = shape(field, gate)
    og = oracle_gate(gate)
    pih = pi_hash(field)
    cols = [[int(x) for x in c] for c in vals]
    if width == 1:
        el = lambda col, j: (cols[col][j],) + (0,) * (F.D - 1)
    else:
        el = lambda col, j: tuple(cols[col][j * width:(j + 1) * width])
    cons, filt = [], []
    for j in range(nrows):
        w = [el(c, j) for c in range(nw)]
        k = [el(nw + c, j) for c in range(nc)]
        out = G.eval_unfiltered(F, og, w, k, pih)
        assert len(out) == ncons == G.num_constraints(og, F.hout, F.D), gate
        cons.append(out)
        filt.append(G.compute_filter(F, own, og, el(nw + nc, j), many))
    return cons, filt


_CASES = {}


def cases(field, width=1, nrows=max(ROW_COUNTS), indices=None):
    """-> [(gate, own index, many selectors, values, reference)] for the grid entries `indices` (default: all), each computed once
    per (field, width, nrows).  A smaller row count of the same width takes the first rows of these (prefix): one reference serves
    every row count."""
    gates = grid(field)
    out = []
    for t in range(len(gates)) if indices is None else indices:
        key = (field, width, nrows, t)
        if key not in _CASES:
            gate, own, many = gates[t], own_index(gates[t], t), many_selectors(t)
            vals = selector_column(field, gate, own, rows(field, gate, nrows, 1000 * field + t, width), width)
            _CASES[key] = (gate, own, many, vals, reference(field, gate, own, many, vals, nrows, width))
        out.append(_CASES[key])
    return out


def prefix(entries, nrows, width=1):
    """the first nrows rows of cases()"""
    return [(gate, own, many, np.ascontiguousarray(vals[:, :nrows * width]), (ref[0][:nrows], ref[1][:nrows]))
            for gate, own, many, vals, ref in entries]


def compare(field, nrows, width, entries, out):
    """the harness output against the references of `entries`; -> list of mismatch descriptions (empty when all is equal)"""
    F = FIELDS[field]
    bad = []
    got = unpack(field, nrows, width, entries, out)
    for (gate, own, many, vals, (cons, filt)), (figures, counts, gcons, gfilt) in zip(entries, got):
        nw, nc, ncons = shape(field, gate)
        if figures != (nw, ncons, nc):
            bad.append("%r: gates::num_wires / num_constraints / num_constants %r, the builder's %r" % (gate, figures, (nw, ncons, nc)))
        if not (counts == ncons).all():
            bad.append("%r: emitted %r constraints, expected %d" % (gate, sorted(set(int(x) for x in counts)), ncons))
            continue
        for j in range(nrows):
            want = [c[:width] for c in cons[j]]
            if width == 1 and any(any(c[1:]) for c in cons[j]):
                bad.append("%r row %d: the oracle's output has higher extension coordinates on base inputs" % (gate, j))
            have = [tuple(int(x) for x in gcons[i, j]) for i in range(ncons)]
            if have != want:
                i = next(i for i in range(ncons) if have[i] != want[i])
                bad.append("%r row %d constraint %d: %r, oracle %r" % (gate, j, i, have[i], want[i]))
                break
        for j in range(nrows):
            if width == 1 and any(filt[j][1:]):
                bad.append("%r row %d: the oracle's filter has higher extension coordinates on a base selector" % (gate, j))
            if tuple(int(x) for x in gfilt[j]) != filt[j][:width]:
                bad.append("%r row %d filter (own index %d): %r, oracle %r" % (gate, j, own, tuple(int(x) for x in gfilt[j]), filt[j][:width]))
                break
    return bad



# ------------------------------------------------------------------------------------------------ the variants through the product
MAX_GATES = 24            # csrc/gate_set.hpp
VARIANTS_PER_CIRCUIT = 18  # + NoopGate, PublicInputGate, the builder's ArithmeticGate and ConstantGate, the hash gate <= MAX_GATES


def config(field, **cfg_kw):
    gl = field == N.GB_GOLDILOCKS
    return CircuitConfig.standard_recursion_config_gl(**cfg_kw) if gl else CircuitConfig.recursion_config_bb_narrow(**cfg_kw)


def buildable(cfg, gate):
    """whether CircuitBuilder can hold a row of the tuple's gate under cfg.  Not: the gates build() places itself (PublicInputGate,
    and through the public inputs' hash PoseidonGate / Poseidon2BabyBearGate with one operation), the base-0 spelling of
    BaseSumGate (the same struct as base 2), a gate with more wires or constants than the config, a degree the selector
    grouping refuses (selectors.rs:125-209), a RandomAccessGate whose routed part exceeds the routed wires."""
    if gate[0] in (G.PUBLIC_INPUT, G.POSEIDON, G.POSEIDON2_BABYBEAR) or (gate[0] == G.BASE_SUM and gate[5] == 0):
        return False
    g = gate_object(cfg.field, gate)
    if g.num_wires > cfg.num_wires or g.num_constants > cfg.num_constants or g.degree > cfg.max_quotient_degree_factor:
        return False
    return gate[0] != G.RANDOM_ACCESS or g.num_routed <= cfg.num_routed_wires


def add_variant_row(b, pw, g, rng):
    """one row of gate struct g with random inputs; the generators fill the rest -> row"""
    p, D, kind = b.F.p, b.F.ext_degree, g.kind
    rnd = lambda: int(rng.integers(0, p, dtype=np.uint64))
    row = b.add_gate(g, [rnd() for _ in range(g.num_constants)] if kind in (G.ARITHMETIC, G.ARITHMETIC_EXTENSION, G.MUL_EXTENSION) else ())

    def fill(cols):
        for c in cols:
            pw.set_target(wire(row, c), rnd())

    if kind == G.ARITHMETIC:
        fill([4 * i + k for i in range(g.num_ops) for k in range(3)])
    elif kind == G.ARITHMETIC_EXTENSION:
        fill([4 * D * i + k for i in range(g.num_ops) for k in range(3 * D)])
    elif kind == G.MUL_EXTENSION:
        fill([3 * D * i + k for i in range(g.num_ops) for k in range(2 * D)])
    elif kind == G.BASE_SUM:
        pw.set_target(wire(row, 0), int(rng.integers(0, min(g.base ** g.num_limbs, p, 1 << 62))))
    elif kind in (G.REDUCING, G.REDUCING_EXTENSION):
        fill(range(D, 3 * D + g.num_coeffs * g.coeff_width))
    elif kind == G.RANDOM_ACCESS:
        for copy in range(g.num_copies):
            items = [rnd() for _ in range(g.vec_size)]
            idx = int(rng.integers(0, g.vec_size))
            pw.set_target(wire(row, g.wire_access_index(copy)), idx)
            pw.set_target(wire(row, g.wire_claimed_element(copy)), items[idx])
            for i, v in enumerate(items):
                pw.set_target(wire(row, g.wire_list_item(i, copy)), v)
    elif kind == G.POSEIDON_MDS:
        fill(range(12 * D))
    elif kind == G.COSET_INTERPOLATION:
        fill([0] + list(range(1, 1 + g.num_points * D)) + list(range(g.start_point, g.start_point + D)))
    elif kind == G.EXPONENTIATION:
        fill([0])
        for i in range(g.num_power_bits):
            pw.set_target(wire(row, 1 + i), int(rng.integers(0, 2)))
    elif kind == G.ADD_MANY:
        fill([(g.num_addends + 1) * i + j for i in range(g.num_ops) for j in range(g.num_addends)])
    elif kind == G.APPLY_MAT4:
        fill([8 * D * op + k for op in range(g.num_ops) for k in range(4 * D)])
    elif kind == G.POSEIDON2_INTERNAL_PERMUTATION:
        fill(range(16 * D))
    else:
        assert kind == G.CONSTANT, kind     # its wires are the builder's: build() hands the circuit's constants to them
    return row


def variant_name(gate):
    return "%s(%s)" % ({v: k.lower() for k, v in vars(G).items() if k.isupper() and isinstance(v, int) and v < 18 and k != "UNUSED_SELECTOR"}[gate[0]],
                       ",".join(str(x) for x in (gate[1], gate[5], gate[6])))


def variant_sets(field, **cfg_kw):
    """{circuit name: [grid tuples]}: the random-access variants, the interpolation variants, the rest in runs of at most
    VARIANTS_PER_CIRCUIT - every buildable() entry of grid(field) exactly once"""
    cfg = config(field, **cfg_kw)
    ok = [g for g in grid(field) if buildable(cfg, g)]
    sets = {"random_access": [g for g in ok if g[0] == G.RANDOM_ACCESS], "interpolation": [g for g in ok if g[0] == G.COSET_INTERPOLATION]}
    rest = [g for g in ok if g[0] not in (G.RANDOM_ACCESS, G.COSET_INTERPOLATION)]
    for k in range(0, len(rest), VARIANTS_PER_CIRCUIT):
        sets["rest%d" % (k // VARIANTS_PER_CIRCUIT)] = rest[k:k + VARIANTS_PER_CIRCUIT]
    return sets


def variant_circuit(field, name, seed=1, **cfg_kw):
    """-> (builder, partial witness, {variant name: row}): one row of every gate of variant_sets()[name] next to a short arithmetic
    chain.  The first "rest" circuit has public inputs, so build() adds the configuration's hash gate.  The extra constants of
    the RandomAccessGate rows and the ConstantGate rows are left to the builder: it hands the circuit's constants to them."""
    cfg = config(field, **cfg_kw)
    b = CircuitBuilder(cfg)
    rng = np.random.default_rng(seed)
    pw = PartialWitness()
    x = b.add_virtual_target()
    y = b.mul_add(x, x, b.constant(5))
    y = b.mul_add(y, b.constant(3), b.constant(7))
    pw.set_target(x, 3)
    if name == "rest0":
        b.register_public_input(x)
        b.register_public_input(y)
    rows = {}
    for gate in variant_sets(field, **cfg_kw)[name]:
        rows[variant_name(gate)] = add_variant_row(b, pw, gate_object(field, gate), rng)
    return b, pw, rows


def variant_circuits(field, seed=1, **cfg_kw):
    """several small circuits (builder, partial witness, {name: row}) that together hold one row of every buildable variant"""
    return [variant_circuit(field, name, seed, **cfg_kw) for name in variant_sets(field, **cfg_kw)]


# ------------------------------------------------------------------------------------------------ what create accepts and refuses
def acceptance_cases(field):
    """[(gate tuple in a two-gate set [NoopGate, gate], verdict)] under the field's stock configuration: "ok", "refused"
    (GB_ERR_UNSUPPORTED or GB_ERR_INVALID) or "needs" (refused because the gate has more wires than the config, the message says
    what it needs).  The interpolation degrees come from interpolation_degrees(), not from the product."""
    cfg = config(field)
    tup = lambda kind, param, p2=0, p3=0: (kind, param, 0, 0, 2, p2, p3)

    def fits(gate):
        return "ok" if gate_object(field, gate).num_wires <= cfg.num_wires else "needs"

    out = []
    for bits in range(1, 6):
        for degree in range(1, (1 << bits) + 2):
            gate = tup(G.COSET_INTERPOLATION, bits, degree)
            out.append((gate, fits(gate) if bits <= 4 and degree in interpolation_degrees(bits) else "refused"))
    for bits in range(7):
        for copies, extra in ((1, 0), (3, 2)):
            gate = tup(G.RANDOM_ACCESS, bits, copies, extra)
            out.append((gate, fits(gate)))
    out += [(tup(G.RANDOM_ACCESS, 7, 1, 0), "refused"), (tup(G.RANDOM_ACCESS, 3, 0, 0), "refused"), (tup(G.RANDOM_ACCESS, 3, 0, 2), "refused")]
    assert cfg.max_quotient_degree_factor == 8
    out += [(tup(G.BASE_SUM, 4, 8), "ok"), (tup(G.BASE_SUM, 4, 9), "refused"), (tup(G.BASE_SUM, 4, 0), "ok"), (tup(G.BASE_SUM, 0, 2), "refused")]
    for gate in (tup(G.REDUCING, 60), tup(G.ARITHMETIC, 40), tup(G.ARITHMETIC, 50), tup(G.EXPONENTIATION, 66), tup(G.EXPONENTIATION, 83),
                 tup(G.ADD_MANY, 40, 1), tup(G.ADD_MANY, 40, 5), tup(G.APPLY_MAT4, 5), tup(G.APPLY_MAT4, 9)):
        out.append((gate, fits(gate)))
    return out


def check_acceptance(field, create):
    """create(gates) builds a circuit object over the gate set or raises; -> the verdicts seen, for the caller to count"""
    import pytest
    seen = {"ok": 0, "refused": 0, "needs": 0}
    for gate, verdict in acceptance_cases(field):
        gates = [(G.NOOP, 0, 0, 0, 2, 0, 0), gate]
        if verdict == "ok":
            create(gates).free()
        else:
            with pytest.raises(N.GoldibearError) as e:
                create(gates)
            assert e.value.status in (N.GB_ERR_UNSUPPORTED, N.GB_ERR_INVALID), (gate, str(e.value))
            assert ("needs" in str(e.value) and "wires" in str(e.value)) == (verdict == "needs"), (gate, str(e.value))
        seen[verdict] += 1
    return seen
