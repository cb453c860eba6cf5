"""prove() from the inputs alone (include/goldibear_gpu.h: gb_circuit_set_generators, gb_circuit_generators_info,
gb_generate_partition, gb_prove_inputs, gb_prove_inputs_retry): the witness generators run on the device.  The oracle is the
builder mirror (BuiltCircuit.generate_partition_witness); every comparison is exact.

  * gb_generate_partition == the mirror at every class, gb_prove_inputs bytes == gb_prove_partition bytes on the mirror's values,
    verified: every circuit of tests/gate_variants.py (one row of every buildable gate variant), both fields; the factorial,
    Fibonacci, BabyBear public-input and recursion-gates circuits; a circuit with a level wider than a workgroup between two
    chains (three launches);
  * a CopyGenerator onto an input: GB_ERR_INVALID "set twice" with another value, success with the same;
  * the reference's asserts - a PoseidonGate row with swap = 2, a RandomAccessGate index == vec_size - are GB_ERR_INVALID and the
    circuit proves a good witness afterwards; a non-canonical input; calls before gb_circuit_set_generators; a program gate's
    record (GB_ERR_UNSUPPORTED);
  * a zero-knowledge circuit with salts; the retry after InvZeroPermArg == gb_prove_partition_retry, with and without kept
    state; the retry across the fronts (csrc/witness_host.inc: gb_prove_partition_retry builds on a matrix gb_prove_inputs kept,
    gb_prove_inputs_retry does not build on one gb_prove_partition kept); a circuit that never calls gb_circuit_set_generators proves as before and runs no generator scope;
  * more inputs than one slice of the page-locked upload holds (1 MB: 131 072 Goldilocks / 262 144 BabyBear words)."""
import ctypes as C

import numpy as np
import pytest

from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GpuContext, PermArgZeroError, ShapeError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import recursion_gates as R
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, NoopGate, PartialWitness, PoseidonGate, wire
import circuits as CS
import gate_programs as GP
import gate_variants as GV
import generator_cases as GC
import partition_cases as PC
import wired_circuits as W

pytestmark = pytest.mark.gpu
SEED = 23


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def check_circuit(c, pw, what):
    """generation == the mirror at every class; prove_inputs == prove_partition on the mirror's values; verified"""
    want = c.generate_partition_witness(pw, np.random.default_rng(SEED))
    got = c.generate_partition_device(pw, np.random.default_rng(SEED))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d targets differ, first %d: %d, mirror %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
    info = c.data.generators_info()
    assert info["num_unrunnable"] == 0, what
    by_partition = c.prove(pw, np.random.default_rng(SEED))
    proof = c.prove_inputs(pw, np.random.default_rng(SEED))
    assert proof == by_partition, what
    assert c.verify(proof), what
    return info


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_variant_circuits(ctx, field):
    for name in GV.variant_sets(field):
        b, pw, rows = GV.variant_circuit(field, name)
        c = b.build(ctx)
        assert 3 <= c.degree_bits <= 7
        check_circuit(c, pw, "%s (field %d)" % (name, field))
        c.data.free()


def test_builder_circuits(ctx):
    for name, (b, pw) in (("factorial", CS.factorial_circuit(count=60)), ("fibonacci", CS.fibonacci_circuit(terms=40)),
                          ("babybear_public_input", CS.babybear_public_input_circuit(steps=30))):
        c = b.build(ctx)
        info = check_circuit(c, pw, name)
        assert info["num_launches"] == 1 and info["num_levels"] > 30, (name, info)    # a dependent chain: one launch
        c.data.free()


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_recursion_gates_circuit(ctx, field):
    b, pw, _ = CS.recursion_gates_circuit(field, seed=9)
    c = b.build(ctx)
    check_circuit(c, pw, "recursion_gates_circuit")
    c.data.free()


def test_a_level_wider_than_a_workgroup_between_two_chains(ctx):
    b, pw = GC.wide_between_chains(300)
    c = b.build(ctx)
    info = check_circuit(c, pw, "chain, 300 wide, chain")
    assert info["num_launches"] == 3
    c.data.free()


def test_copy_onto_an_input(ctx):
    for other, ok in ((5, True), (6, False)):
        b = CircuitBuilder(CircuitConfig.standard_recursion_config_gl())
        u, t = b.add_virtual_target(), b.add_virtual_target()
        b.generate_copy(u, t)
        b.mul(t, t)
        pw = PartialWitness()
        pw.set_target(u, 5)
        pw.set_target(t, other)
        c = b.build(ctx)
        if ok:
            check_circuit(c, pw, "copy onto an equal input")
            assert c.data.generators_info()["num_checks"] == 1
        else:
            with pytest.raises(ShapeError, match="set twice with different values"):
                c.prove_inputs(pw)
            with pytest.raises(ValueError, match="set twice"):
                c.generate_partition_witness(pw)
        c.data.free()
    # two generators onto one target
    b, pw, _ = GC.copy_circuit(second_value=12)
    c = b.build(ctx)
    with pytest.raises(ShapeError, match="set twice with different values"):
        c.prove_inputs(pw)
    c.data.free()


def test_the_asserts_of_the_reference_and_a_good_witness_afterwards(ctx):
    cfg = CircuitConfig.standard_recursion_config_gl()
    # PoseidonGate: swap = 2
    b, pw, bad = CircuitBuilder(cfg), PartialWitness(), PartialWitness()
    row = b.add_gate(PoseidonGate())
    for p in (pw, bad):
        for col in range(12):
            p.set_target(wire(row, col), 100 + col)
    pw.set_target(wire(row, PoseidonGate.WIRE_SWAP), 1)
    bad.set_target(wire(row, PoseidonGate.WIRE_SWAP), 2)
    c = b.build(ctx)
    c.set_generators(pw=pw)
    with pytest.raises(ShapeError, match="swap wire"):
        c.prove_inputs(bad)
    check_circuit(c, pw, "PoseidonGate row after a refused one")
    c.data.free()
    # RandomAccessGate: index == vec_size
    b, pw, bad = CircuitBuilder(cfg), PartialWitness(), PartialWitness()
    g = R.RandomAccessGate(2, 1, 0)
    row = b.add_gate(g)
    for p, idx in ((pw, g.vec_size - 1), (bad, g.vec_size)):
        p.set_target(wire(row, g.wire_access_index(0)), idx)
        for i in range(g.vec_size):
            p.set_target(wire(row, g.wire_list_item(i, 0)), 50 + i)
        p.set_target(wire(row, g.wire_claimed_element(0)), 50 + g.vec_size - 1)
    c = b.build(ctx)
    c.set_generators(pw=pw)
    with pytest.raises(ShapeError, match="Access index"):
        c.prove_inputs(bad)
    check_circuit(c, pw, "RandomAccessGate row after a refused one")
    c.data.free()


def test_errors(ctx):
    b, pw = CS.poly_chain_circuit(CircuitConfig.standard_recursion_config_gl(), 9)
    c = b.build(ctx)
    lib, n = ctx._lib, C.c_size_t()
    buf = np.empty(1 << 20, dtype=np.uint8)
    inputs = GC.built_inputs(c, pw)
    c._input_targets = inputs
    values = c.input_values(pw, np.random.default_rng(SEED))

    def prove(v, flags=0):
        return lib.gb_prove_inputs(c.data.handle, v.ctypes.data, flags, None, buf.ctypes.data, buf.size, C.byref(n))

    # before gb_circuit_set_partition / gb_circuit_set_generators
    u64p = C.POINTER(C.c_uint64)
    targets = np.array([c.target_index(t) for t in inputs], dtype=np.uint64)
    consts = np.ascontiguousarray(c.constants_columns, dtype=np.uint64)
    assert lib.gb_circuit_set_generators(c.data.handle, None, 0, targets.ctypes.data_as(u64p), len(targets), consts.ctypes.data_as(u64p), 0) == N.GB_ERR_INVALID
    assert b"gb_circuit_set_partition" in lib.gb_last_error(ctx.handle)
    c.data.set_partition(c.representative_map, c.public_input_targets)
    c._partition_set = True
    assert prove(values) == N.GB_ERR_INVALID and b"gb_circuit_set_generators" in lib.gb_last_error(ctx.handle)
    assert lib.gb_circuit_generators_info(c.data.handle, None, None, None, None, None) == N.GB_ERR_INVALID
    assert lib.gb_circuit_set_generators(c.data.handle, None, 0, targets.ctypes.data_as(u64p), len(targets), consts.ctypes.data_as(u64p), 8) == N.GB_ERR_INVALID
    c.set_generators(inputs)
    want = c.prove(pw, np.random.default_rng(SEED))
    assert prove(values) == N.GB_OK and buf[:n.value].tobytes() == want
    assert prove(values, N.GB_INPUT_DEVICE) == N.GB_ERR_INVALID and prove(values, 4) == N.GB_ERR_INVALID
    v = values.copy()
    v[0] = np.uint64(GL.P)
    assert prove(v) == N.GB_ERR_INVALID and b"non-canonical witness element" in lib.gb_last_error(ctx.handle)
    assert prove(values) == N.GB_OK and buf[:n.value].tobytes() == want
    # the words of the reference's field types
    p3 = values.copy()
    small = values < np.uint64((1 << 64) - GL.P)
    p3[small] = values[small] + np.uint64(GL.P)
    assert prove(p3, N.GB_INPUT_P3_REPR) == N.GB_OK and buf[:n.value].tobytes() == want
    # gb_circuit_set_partition drops the schedule
    c.data.set_partition(c.representative_map, c.public_input_targets)
    assert prove(values) == N.GB_ERR_INVALID
    c.data.free()
    # a program gate's generators are not built
    b, pw = CS.poly_chain_circuit(CircuitConfig.standard_recursion_config_gl(), 9)
    c = GP.with_program_gates(b).build(ctx)
    assert any(g[0] == 18 for g in c.gate_table)
    with pytest.raises(N.GoldibearError) as e:
        c.set_generators(pw=pw)
    assert e.value.status == N.GB_ERR_UNSUPPORTED and "program gates" in str(e.value)
    assert c.verify(c.prove(pw))          # such a circuit stays on the partition path
    c.data.free()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_zero_knowledge_circuit_with_salts(ctx, field_name):
    F, tag = {"goldilocks": (GL, N.GB_GOLDILOCKS), "babybear": (BB, N.GB_BABYBEAR)}[field_name]
    circ = D.DummyCircuit(6, F=F) if F is GL else D.DummyCircuit(6, D.CircuitConfig.babybear(6), F=BB)
    circ.zero_knowledge = True
    n_lde = circ.n << circ.cfg.rate_bits
    salts = F.fill(0x5A17, 3 * 4 * n_lde).reshape(3, 4, n_lde)
    cfg = circ.cfg
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                      num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                      arity_bits=cfg.arity_bits, field=tag, zero_knowledge=True)
    w = circ.witness(seed=4)
    m, values = PC.partition_of_witness(w, None, 4)
    gpu.set_partition(m)
    # every class a wire reads is an input: the dummy circuit's witness is the host's
    reps = np.unique(m[:circ.n * cfg.num_wires])
    gpu.set_generators([], reps, np.zeros((cfg.num_constants, circ.n), dtype=np.uint64))
    want = gpu.prove_partition(values, salts=salts)
    assert gpu.prove_inputs_once(values[reps.astype(np.int64)], salts=salts) == want
    with pytest.raises(ShapeError):
        gpu.prove_inputs_once(values[reps.astype(np.int64)])          # a zero-knowledge circuit needs its salts
    assert gpu.verify(want)
    gpu.free()


@pytest.mark.parametrize("degree_bits", [6, 16])
def test_retry_after_inv_zero_perm_arg(ctx, degree_bits):
    # ((64 - degree_bits) * num_challenges >= 100, circuit_builder.rs:1190-1192: three challenges from 2^15 rows on)
    b, pw = CS.factorial_circuit(count=60, num_challenges=3 if degree_bits >= 15 else 2)
    while b.num_gates() < (1 << degree_bits) - 40:
        b.add_gate(NoopGate())
    c = b.build(ctx)
    assert c.degree_bits == degree_bits
    c.set_generators(pw=pw)
    data, nw = c.data, c.config.num_wires
    rw = (c.random_wire[1], c.random_wire[0])                     # (column, row)
    rw_target = c.target_index(wire(*c.random_wire))
    rw_input = c._input_targets.index(wire(*c.random_wire))
    v0 = c.generate_partition_witness(pw, np.random.default_rng(SEED))
    i0 = c.input_values(pw, np.random.default_rng(SEED))
    v, i = v0.copy(), i0.copy()
    v[rw_target] = i[rw_input] = np.uint64(0xFEDCBA9876543210 % GL.P)
    want = data.prove_partition_once(v)
    assert data.prove_inputs_once(i) == want
    data.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        data.prove_partition_once(v0)
    assert data.prove_partition_once(v, retry_wire=rw) == want      # gb_prove_partition_retry
    data.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        data.prove_inputs_once(i0)
    ctx.set_profiling(True)
    ctx.scope_reset()
    assert data.prove_inputs_once(i, retry_wire=rw) == want         # gb_prove_inputs_retry
    # where the failed attempt kept its state (>= 2^19 leaves) the retry re-draws one cell of the kept matrix: no generator runs
    kept = degree_bits == 16
    assert ctx.scope_ms("run generators")[1] == (0 if kept else 1)
    ctx.set_profiling(False)
    # a retry with nothing kept (another proof in between) is the full computation
    data.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        data.prove_inputs_once(i0)
    assert data.prove_inputs_once(i0) != want
    assert data.prove_inputs_once(i, retry_wire=rw) == want
    # the mirror's loop draws the random wire's input again
    data.arm_perm_arg_failure()
    proof = c.prove_inputs(pw, np.random.default_rng(5))
    assert data.perm_arg_retries == 1 and c.verify(proof)
    data.free()
    ctx.trim()


def test_retry_across_the_partition_and_inputs_fronts(ctx):
    """What a failed attempt keeps is one state, whichever front kept it (2^16 rows: the smallest size at which one does).
    (a) gb_prove_inputs fails, gb_prove_partition_retry builds on its matrix - it needs the matrix alone, the public inputs are
    read off `values`: no expansion runs.  (b) gb_prove_partition fails, gb_prove_inputs_retry does not build on its matrix - no
    public inputs were kept with it: the generators run, the full computation.  Either way the bytes are those of the re-drawn
    witness proved from the matrix."""
    b, pw = CS.factorial_circuit(count=60, num_challenges=3)
    while b.num_gates() < (1 << 16) - 40:
        b.add_gate(NoopGate())
    c = b.build(ctx)
    assert c.degree_bits == 16
    c.set_generators(pw=pw)
    data = c.data
    rw = (c.random_wire[1], c.random_wire[0])                     # (column, row)
    rw_target = c.target_index(wire(*c.random_wire))
    rw_input = c._input_targets.index(wire(*c.random_wire))
    v0 = c.generate_partition_witness(pw, np.random.default_rng(SEED))
    i0 = c.input_values(pw, np.random.default_rng(SEED))
    wires, pis = c.generate_witness(pw, np.random.default_rng(SEED))
    v, i = v0.copy(), i0.copy()
    v[rw_target] = i[rw_input] = wires[rw] = np.uint64(0xFEDCBA9876543210 % GL.P)
    want = data.prove_once(wires, pis)
    ctx.set_profiling(True)
    data.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        data.prove_inputs_once(i0)
    ctx.scope_reset()
    assert data.prove_partition_once(v, retry_wire=rw) == want      # (a)
    assert ctx.scope_ms("partition expansion")[1] == 0
    data.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        data.prove_partition_once(v0)
    ctx.scope_reset()
    assert data.prove_inputs_once(i, retry_wire=rw) == want         # (b)
    assert ctx.scope_ms("run generators")[1] == 1
    ctx.set_profiling(False)
    data.free()
    ctx.trim()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_a_circuit_without_generators_proves_as_before(ctx, field_name):
    F, tag = {"goldilocks": (GL, N.GB_GOLDILOCKS), "babybear": (BB, N.GB_BABYBEAR)}[field_name]
    cfg = D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)
    circ, w, kw = W.wired_dummy_circuit(F, cfg, 6, 41, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    circ.set_cap(gpu.constants_sigmas_cap)
    m, values = PC.partition_of_witness(w, circ.copy_classes, 41)
    gpu.set_partition(m)
    want = D.prove_cpu(circ, w)[0]                                  # the oracle prover: what these entry points gave before
    ctx.set_profiling(True)
    ctx.scope_reset()
    assert gpu.prove(w) == want and gpu.prove_partition(values) == want
    assert ctx.scope_ms("run generators")[1] == 0
    ctx.set_profiling(False)
    # and with a schedule set, the two entry points are what they were
    reps = np.unique(m[:circ.n * circ.cfg.num_wires])
    gpu.set_generators([], reps, np.zeros((kw.get("num_constants", cfg.num_constants), circ.n), dtype=np.uint64))
    assert gpu.prove_inputs_once(values[reps.astype(np.int64)]) == want
    assert gpu.prove(w) == want and gpu.prove_partition(values) == want
    gpu.free()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_more_inputs_than_one_upload_slice(ctx, field_name):
    """every class of a 2^11-row wired circuit as an input: 276 480 / 342 016 cells, so the inputs go up in several slices, the last
    one partial; a non-canonical word in the last slice is still found"""
    F, tag = {"goldilocks": (GL, N.GB_GOLDILOCKS), "babybear": (BB, N.GB_BABYBEAR)}[field_name]
    cfg = D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)
    circ, w, kw = W.wired_dummy_circuit(F, cfg, 11, 43, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    m, values = PC.partition_of_witness(w, circ.copy_classes, 43)
    gpu.set_partition(m)
    reps = np.unique(m[:circ.n * circ.cfg.num_wires]).astype(np.int64)
    slice_words = (1 << 20) // values.itemsize
    assert len(reps) > slice_words and len(reps) % slice_words
    gpu.set_generators([], reps, np.zeros((kw.get("num_constants", cfg.num_constants), circ.n), dtype=np.uint64))
    want = gpu.prove_partition(values)
    inputs = values[reps]
    assert gpu.prove_inputs_once(inputs) == want
    bad = inputs.copy()
    bad[-1] = F.P
    with pytest.raises(ShapeError, match="non-canonical witness element"):
        gpu.prove_inputs_once(bad)
    assert gpu.prove_inputs_once(inputs) == want
    gpu.free()
