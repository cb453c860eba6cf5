"""gb_check_witness / gb_check_partition / gb_check_inputs on the GPU (csrc/kernels_check.hip): does a witness satisfy its circuit,
and where not - row, gate, constraint, value; the copy constraints of a circuit with a partition; the option "check_witness".
Every expected list comes from tests/witness_check_cases.py - oracle/gates.py's compute_filter and eval_unfiltered on the witness
rows, GateProgram.evaluate for program gates, numpy over the representative map for copies - never from the checker.  Both fields;
the circuits have 2^3 .. 2^10 rows.  -m gpu only."""
import numpy as np
import pytest

import circuits as CS
import gadget_cases as GA
import gate_variants as GV
import generator_program_circuits as GPC
import partition_cases as PC
import wired_circuits as W
import witness_check_cases as WC
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import (CircuitData, GateProgram, GeneratorProgram, GpuContext, ProgramGate, ProgramGenerator, ShapeError,
                                   VerifyError)
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, NoopGate, PartialWitness, wire

pytestmark = pytest.mark.gpu
SEED = 31
FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]
IDS = ["goldilocks", "babybear"]
ALL = 1 << 16     # a capacity no list of these tests reaches


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def rng():
    return np.random.default_rng(SEED)


def assert_satisfied(got, copies=1):
    violations, res = got
    assert violations == []
    assert (res.num_gate_violations, res.num_selector_violations, res.num_copy_violations, res.num_listed) == (0, 0, 0, 0)
    assert res.copies_checked == copies


def assert_reported(got, want, copies=1, capacity=ALL):
    """the listed violations are the first `capacity` of `want` and the counts are those of all of `want`"""
    violations, res = got
    WC.same(violations, want[:capacity])
    assert (res.num_gate_violations, res.num_selector_violations, res.num_copy_violations) == WC.counts(want)
    assert res.num_listed == len(violations) and res.copies_checked == copies


def with_partition(c):
    if not c._partition_set:
        c.data.set_partition(c.representative_map, c.public_input_targets)
        c._partition_set = True
    return c


# ------------------------------------------------------------------------------------------------ 1. satisfied witnesses
def satisfied_circuits(field):
    """name -> (builder, partial witness)"""
    cfg = GA.config(field)
    out = {name: GV.variant_circuit(field, name, seed=9)[:2] for name in GV.variant_sets(field)}
    out["mul_add_three"] = GPC.mul_add_three_circuit(cfg, 5)
    out["mul_add_three_two_selectors"] = GPC.mul_add_three_circuit(cfg, 4, public_output=True)
    out["poly_chain_programs"] = (lambda pair: (pair[1], pair[2]))(GPC.poly_chain_pair(cfg, 3 * GPC.ArithmeticGate.new_from_config(cfg).num_ops))
    out["square_root"] = GPC.square_root_circuit(cfg, pow(0xC0FFEE, 2, GV.FIELDS[field].P), pad_to=8)[:2]
    out["gadget_select"] = next((b, pw) for name, b, pw in GA.builder_circuits(field) if name == "select")
    return out


SATISFIED = ["random_access", "interpolation", "rest0", "rest1", "rest2", "mul_add_three", "mul_add_three_two_selectors",
             "poly_chain_programs", "square_root", "gadget_select"]


@pytest.mark.parametrize("name", SATISFIED)
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_satisfied_witnesses(ctx, field, name):
    b, pw = satisfied_circuits(field)[name]
    c = b.build(ctx)
    assert_satisfied(c.check(pw, rng()))
    assert_satisfied(c.check_inputs(pw, rng()))
    assert c.verify(c.prove(pw, rng()))
    c.data.free()


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_satisfied_zero_knowledge_circuit(ctx, field):
    F = GV.FIELDS[field]
    circ = D.DummyCircuit(6, F=F) if F is GL else D.DummyCircuit(6, D.CircuitConfig.babybear(6), F=BB)
    circ.zero_knowledge = True
    cfg = circ.cfg
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires,
                      num_constants=cfg.num_constants, num_challenges=cfg.num_challenges, arity_bits=cfg.arity_bits, field=field,
                      zero_knowledge=True)
    w = circ.witness(seed=4)
    m, values = PC.partition_of_witness(w, None, 4)
    gpu.set_partition(m)
    reps = np.unique(m[:circ.n * cfg.num_wires])
    gpu.set_generators([], reps, np.zeros((cfg.num_constants, circ.n), dtype=np.uint64))
    assert_satisfied(gpu.check_partition(values))
    assert_satisfied(gpu.check_inputs(values[reps.astype(np.int64)]))
    assert_satisfied(gpu.check_witness(w))
    n_lde = circ.n << cfg.rate_bits
    assert gpu.verify(gpu.prove_partition(values, salts=F.fill(0x5A17, 3 * 4 * n_lde).reshape(3, 4, n_lde)))
    gpu.free()


# ------------------------------------------------------------------------------------------------ 2. one broken cell per gate variant
def broken_cell(c, b, w, pis, row):
    """(column, broken matrix): 1 added to the highest wire of the row's gate whose change changes the oracle's constraint list"""
    F = GV.FIELDS[c.config.field]
    gate = b.gate_instances[row][0]
    g = c.row_gates[row]
    pih = WC.pi_hash(F, pis)
    consts = c.constants_sigmas[c.num_selectors:c.num_selectors + c.max_constants, row]
    before = WC.constraints(F, c.gate_table[g], w[:, row], consts, pih, c.programs)
    for col in range(gate.num_wires - 1, -1, -1):
        bad = w.copy()
        bad[col, row] = (int(bad[col, row]) + 1) % F.P
        if WC.constraints(F, c.gate_table[g], bad[:, row], consts, pih, c.programs) != before:
            return col, bad
    raise AssertionError("no wire of row %d changes its gate's constraints" % row)


@pytest.mark.parametrize("name", ["random_access", "interpolation", "rest0", "rest1", "rest2"])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_one_broken_cell_per_gate_variant(ctx, field, name):
    b, pw, rows = GV.variant_circuit(field, name, seed=9)
    c = with_partition(b.build(ctx))
    w, pis = c.generate_witness(pw)
    assert_satisfied(c.data.check_witness(w, pis))
    proved = 0
    for vname, row in rows.items():
        col, bad = broken_cell(c, b, w, pis, row)
        want = WC.expected(c, bad, pis)
        assert any(v.kind == N.GB_VIOLATION_GATE and v.row == row for v in want), vname
        assert_reported(c.data.check_witness(bad, pis, max_violations=ALL), want)
        if name == "rest1" and proved < 3:     # what the checker predicts: the proof of this matrix cannot verify
            proved += 1
            with pytest.raises(VerifyError, match="vanishing"):
                c.data.verify(c.data.prove_once(bad, pis))
    c.data.free()


# ------------------------------------------------------------------------------------------------ 3. launch boundaries (gb_circuit_create)
def _dummy_config(F):
    return D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)


def constant_rows_circuit(ctx, F, degree_bits, seed):
    """wired_dummy_circuit with every NoopGate row turned into a ConstantGate row whose constants are the row's first wires: the
    witness stays a satisfying one, and the ConstantGate's row list has n - 1 entries, row 0 and row n - 1 among them"""
    circ, w, kw = W.wired_dummy_circuit(F, _dummy_config(F), degree_bits, seed, "edges")
    cs = circ.constants_sigmas.copy()
    nc = circ.cfg.num_constants
    rows = np.flatnonzero(cs[0] == circ.GATE_NOOP)
    cs[0, rows] = circ.GATE_CONSTANT
    cs[1:1 + nc, rows] = w[:nc, rows]
    circ.constants_sigmas = cs
    return circ, w, CircuitData(ctx, circ.degree_bits, cs, circ.k_is, **kw)


@pytest.mark.parametrize("degree_bits", [3, 6, 8, 10])
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_launch_boundaries(ctx, field, degree_bits):
    F = GV.FIELDS[field]
    circ, w, gpu = constant_rows_circuit(ctx, F, degree_bits, seed=degree_bits)
    n = circ.n
    assert_satisfied(gpu.check_witness(w), copies=0)
    constant_rows = np.flatnonzero(circ.constants_sigmas[0] == circ.GATE_CONSTANT)
    assert len(constant_rows) == n - 1 and constant_rows[0] == 0 and constant_rows[-1] == n - 1
    for rows in ([0], [n - 1], constant_rows):
        bad = w.copy()
        bad[1, rows] = (bad[1, rows].astype(object) + 1) % F.P
        want = WC.expected_dummy(circ, bad)
        assert [v.row for v in want] == list(rows) and all(v.index == 1 and v.gate == circ.GATE_CONSTANT for v in want)
        assert_reported(gpu.check_witness(bad, max_violations=ALL), want, copies=0)
        assert_reported(gpu.check_witness(bad, max_violations=4), want, copies=0, capacity=4)
        assert_reported(gpu.check_witness(bad, max_violations=0), want, copies=0, capacity=0)
    gpu.free()


# ------------------------------------------------------------------------------------------------ 4. many violations
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_many_violations(ctx, field):
    F = GV.FIELDS[field]
    cfg = GA.config(field)
    b, pw = CircuitBuilder(cfg), PartialWitness()
    x = b.add_virtual_target()
    pw.set_target(x, 3)
    y = x
    for i in range(400):
        y = b.mul_add(y, b.constant(2 + i % 5), x)
    for k in range(6):
        t = b.add_virtual_target()
        pw.set_target(t, 1000 + 77 * k)
        b.range_check(t, 12)
    b.register_public_input(y)
    while b.num_gates() < 1000:
        b.add_gate(NoopGate())
    c = with_partition(b.build(ctx))
    assert c.degree_bits == 10
    w, pis = c.generate_witness(pw)
    assert_satisfied(c.data.check_witness(w, pis))
    pick = np.random.default_rng(SEED)
    bad = w.copy()
    used = np.flatnonzero([g.kind != 0 for g, _ in b.gate_instances])       # rows that hold a gate with constraints
    for _ in range(37):      # three in four among the wires of a row's gate, the rest anywhere in the matrix
        row, width = int(pick.integers(0, 1 << 10)), cfg.num_wires
        if pick.integers(0, 4):
            row = int(used[pick.integers(0, len(used))])
            width = b.gate_instances[row][0].num_wires
        col = int(pick.integers(0, width))
        bad[col, row] = (int(bad[col, row]) + 1 + int(pick.integers(0, 5))) % F.P
    want = WC.expected(c, bad, pis)
    assert WC.counts(want)[0] >= 3 and WC.counts(want)[2] >= 3
    first = c.data.check_witness(bad, pis, max_violations=ALL)
    assert_reported(first, want)
    second = c.data.check_witness(bad, pis, max_violations=ALL)      # the cached preparation
    assert_reported(second, want)
    c.data.free()


# ------------------------------------------------------------------------------------------------ 5. copy constraints
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_copy_constraints(ctx, field):
    F = GV.FIELDS[field]
    circ, w, kw = W.wired_dummy_circuit(F, _dummy_config(F), 6, 7, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    nw, n = w.shape
    cells, starts, sizes = circ.copy_classes
    t = int(np.flatnonzero(sizes >= 3)[0])
    members = sorted(int(r) * nw + int(col) for col, r in (divmod(int(x), n) for x in cells[starts[t]:starts[t] + sizes[t]]))
    m, _ = PC.partition_of_witness(w, circ.copy_classes, 4)
    gpu.set_partition(m)
    assert_satisfied(gpu.check_witness(w))

    def broken(cell, also_pi_row=False):
        bad = w.copy()
        bad[cell % nw, cell // nw] = (int(bad[cell % nw, cell // nw]) + 1) % F.P
        if also_pi_row:
            bad[0, circ.pi_row] = 5
        return bad

    def want_for(bad, rep_map):
        return WC.expected_dummy(circ, bad) + (WC.copy_violations(rep_map, bad) if rep_map is not None else [])

    # a member that is not the first: that cell alone, with both cells and both values
    bad = broken(members[1])
    want = want_for(bad, m)
    assert [(v.kind, v.row * nw + v.index, v.other_row * nw + v.other_wire) for v in want] == [(N.GB_VIOLATION_COPY, members[1], members[0])]
    assert want[0].value == (want[0].other_value + 1) % F.P
    assert_reported(gpu.check_witness(bad, max_violations=ALL), want)
    # the first cell: every other member
    bad = broken(members[0], also_pi_row=True)
    want = want_for(bad, m)
    assert [v.row * nw + v.index for v in want if v.kind == N.GB_VIOLATION_COPY] == members[1:] and WC.counts(want)[0] == 1
    assert_reported(gpu.check_witness(bad, max_violations=ALL), want)
    # a second valid map - other representatives for the same classes - and one without classes: the cache is rebuilt
    m2, _ = PC.partition_of_witness(w, circ.copy_classes, 5)
    assert (m2 != m).any()
    gpu.set_partition(m2)
    assert_reported(gpu.check_witness(bad, max_violations=ALL), want_for(bad, m2))
    ident = np.arange(nw * n, dtype=np.uint64)
    gpu.set_partition(ident)
    assert_reported(gpu.check_witness(bad, max_violations=ALL), want_for(bad, ident))
    assert WC.counts(want_for(bad, ident)) == (1, 0, 0)
    gpu.free()
    # the same circuit without a partition: copies are not checked, and the result says so
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    assert_reported(gpu.check_witness(bad, max_violations=ALL), want_for(bad, None), copies=0)
    gpu.free()


# ------------------------------------------------------------------------------------------------ 6. disagreeing programs
def disagreeing_circuit(field, generator_adds):
    """two MulAddThreeGate rows (out = c0 * a * b + 3, a a bit) with a NoopGate row between them and a public input, so that the
    circuit has two selector columns; the generator program adds `generator_adds` -> (builder, pw, rows, [(a, b, c0)])"""
    cfg = GA.config(field)
    b, pw = CircuitBuilder(cfg), PartialWitness()
    constraints = GateProgram.from_constraints(lambda w, c: [w[2] - (w[0] * w[1] * c[0] + 3), w[0] * (w[0] - 1)],
                                               num_wires=3, num_constants=1, field=field)
    generator = GeneratorProgram.from_function(lambda d, c, ops: [d[0] * d[1] * c[0] + generator_adds], num_in=2, num_out=1,
                                               num_constants=1, field=field)
    gate = ProgramGate("MulAddThreeGate", constraints, generators=lambda row, consts: [
        ProgramGenerator("MulAddThreeGenerator", generator, [wire(row, 0), wire(row, 1)], [wire(row, 2)], row=row)])
    rows, operands = [], [(1, 6, 5), (1, 11, 8)]
    for a, x, k in operands:
        row = b.add_gate(gate, constants=[k])
        ta, tx = b.add_virtual_target(), b.add_virtual_target()
        pw.set_target(ta, a)
        pw.set_target(tx, x)
        b.connect(ta, wire(row, 0))
        b.connect(tx, wire(row, 1))
        rows.append(row)
        b.add_gate(NoopGate())
    pub = b.add_virtual_target()
    pw.set_target(pub, 9)
    b.register_public_input(pub)
    return b, pw, rows, operands


@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_a_generator_program_that_disagrees_with_its_gate_program(ctx, field):
    F = GV.FIELDS[field]
    b, pw, rows, operands = disagreeing_circuit(field, generator_adds=4)
    c = b.build(ctx)
    assert c.num_selectors == 2 and rows[0] != rows[1]
    g = c.gate_ids.index("MulAddThreeGate")
    want = []
    for row, (a, x, k) in zip(rows, operands):
        value = c.programs[c.gate_table[g][1]].evaluate([a, x, (k * a * x + 4) % F.P], [k])[0]
        assert value == 1
        want.append(N.Violation(N.GB_VIOLATION_GATE, gate=g, row=row, index=0, value=value))
    by_inputs = c.check_inputs(pw, rng())
    assert_reported(by_inputs, want)
    assert_reported(c.check(pw, rng()), want)
    assert by_inputs[0][0].describe(c) == "row %d: MulAddThreeGate, constraint 0 = 1" % rows[0]
    c.data.free()
    # the same circuit with the generator the gate asks for
    b, pw, rows, _ = disagreeing_circuit(field, generator_adds=3)
    c = b.build(ctx)
    assert_satisfied(c.check_inputs(pw, rng()))
    c.data.free()


# ------------------------------------------------------------------------------------------------ 7. public inputs
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_a_changed_public_input(ctx, field):
    F = GV.FIELDS[field]
    b, pw, _ = GV.variant_circuit(field, "rest0", seed=9)
    c = with_partition(b.build(ctx))
    w, pis = c.generate_witness(pw)
    assert len(pis) == 2
    assert_satisfied(c.data.check_witness(w, pis))
    other = [pis[0], (pis[1] + 1) % F.P]
    want = WC.expected(c, w, other)
    good, bad_hash = WC.pi_hash(F, pis), WC.pi_hash(F, other)
    word = next(i for i in range(F.hout) if good[i] != bad_hash[i])
    pi_gate = next(i for i, g in enumerate(c.gate_table) if g[0] == 2)
    pi_row = c.row_gates.index(pi_gate)
    assert [v.as_tuple() for v in want] == [N.Violation(N.GB_VIOLATION_GATE, gate=pi_gate, row=pi_row, index=word,
                                                        value=(good[word] - bad_hash[word]) % F.P).as_tuple()]
    assert_reported(c.data.check_witness(w, other), want)
    c.data.free()


# ------------------------------------------------------------------------------------------------ 8. selector violation
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_selector_violation(ctx, field):
    F = GV.FIELDS[field]
    circ, w, kw = W.wired_dummy_circuit(F, _dummy_config(F), 5, 3, "edges")
    cs = circ.constants_sigmas.copy()
    cs[0, circ.pi_row] = 7           # names no gate of the group {0, 1, 2}
    circ.constants_sigmas = cs
    gpu = CircuitData(ctx, circ.degree_bits, cs, circ.k_is, **kw)
    bad = w.copy()
    bad[0, circ.pi_row] = 5          # would break the PublicInputGate, were it evaluated on that row
    bad[0, circ.const_row] = 9       # and this breaks the ConstantGate, on a row whose selector is sound
    want = WC.expected_dummy(circ, bad)
    assert [(v.kind, v.row, v.index, v.value) for v in want] == [(N.GB_VIOLATION_SELECTOR, circ.pi_row, 0, 7),
                                                                 (N.GB_VIOLATION_GATE, circ.const_row, 0, F.P - 9)]
    assert_reported(gpu.check_witness(bad), want, copies=0)
    gpu.free()


# ------------------------------------------------------------------------------------------------ 9. the option
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_option_check_witness(ctx, field):
    b, pw, rows = GV.variant_circuit(field, "rest1", seed=9)
    c = with_partition(b.build(ctx))
    w, pis = c.generate_witness(pw)
    row = next(iter(rows.values()))
    _, bad = broken_cell(c, b, w, pis, row)
    want = WC.expected(c, bad, pis)
    bd, bpw, brows, _ = disagreeing_circuit(field, generator_adds=4)
    cd = bd.build(ctx)
    cd.set_generators(pw=bpw)
    inputs = cd.input_values(bpw, rng())
    wanted_inputs = cd.check_inputs(bpw, rng())[0]
    try:
        ctx.set_option("check_witness", 1)
        with pytest.raises(N.UnsatisfiedError) as e:
            c.data.prove_once(bad, pis)
        assert e.value.status == N.GB_ERR_UNSATISFIED == 20 and e.value.violations[0] == want[0]
        with pytest.raises(N.UnsatisfiedError) as e:
            cd.data.prove_inputs_once(inputs)
        assert e.value.status == 20 and e.value.violations[0] == wanted_inputs[0] and wanted_inputs[0].row == brows[0]
        assert c.data.verify(c.data.prove_once(w, pis))          # a satisfying witness is proved as before
    finally:
        ctx.set_option("check_witness", 0)
    proof = c.data.prove_once(bad, pis)                          # today's behaviour: bytes that cannot verify
    with pytest.raises(VerifyError, match="vanishing"):
        c.data.verify(proof)
    assert isinstance(cd.data.prove_inputs_once(inputs), bytes)
    c.data.free()
    cd.data.free()


def test_a_check_between_a_failed_attempt_and_its_retry(ctx):
    """for gb_prove_retry a check is another call in between: the retry after it is the full computation, with the same bytes"""
    circ, w, kw = W.wired_dummy_circuit(GL, _dummy_config(GL), 6, 5, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    want = gpu.prove_once(w)
    gpu.arm_perm_arg_failure()
    with pytest.raises(N.PermArgZeroError):
        gpu.prove_once(w)
    assert_satisfied(gpu.check_witness(w), copies=0)
    assert gpu.prove_once(w, retry_wire=(circ.cfg.num_wires - 1, circ.pi_row)) == want
    assert gpu.verify(want)
    gpu.free()


# ------------------------------------------------------------------------------------------------ 10. input forms
@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_input_forms(ctx, field):
    F = GV.FIELDS[field]
    b, pw, rows = GV.variant_circuit(field, "rest2", seed=9)
    c = with_partition(b.build(ctx))
    w, pis = c.generate_witness(pw)
    values = c.generate_partition_witness(pw)
    row = next(iter(rows.values()))
    col, bad = broken_cell(c, b, w, pis, row)
    want = WC.expected(c, bad, pis)
    assert_reported(c.data.check_witness(bad, pis, max_violations=ALL), want)
    # the device matrix of expand_partition, with the same cell broken on the device
    dev = c.data.expand_partition(values)
    assert_satisfied(c.data.check_witness(dev, pis))
    v = int(bad[col, row])
    dev[col, row] = v - (1 << (8 * dev.element_size())) if v >> (8 * dev.element_size() - 1) else v
    import torch
    torch.cuda.current_stream(dev.device).synchronize()
    assert_reported(c.data.check_witness(dev, pis, max_violations=ALL), want)
    # the reference's in-memory words
    if F is GL:
        words = bad.copy()
        small = bad < np.uint64((1 << 64) - F.P)
        words[small] = bad[small] + np.uint64(F.P)
    else:
        words = ((bad.astype(np.uint64) << np.uint64(32)) % np.uint64(F.P)).astype(F.dtype)
    assert_reported(c.data.check_witness(words, pis, max_violations=ALL, p3_repr=True), want)
    # an element that is not below p
    over = w.copy()
    over[3, 1] = F.P
    with pytest.raises(ShapeError, match="non-canonical witness element"):
        c.data.check_witness(over, pis)
    vals = values.copy()
    vals[int(c.representative_map[c.target_index(wire(row, 0))])] = F.P
    with pytest.raises(ShapeError, match="non-canonical witness element"):
        c.data.check_partition(vals)
    assert_satisfied(c.data.check_partition(values))
    c.data.free()
