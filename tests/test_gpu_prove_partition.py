"""prove() from the reference's own witness object (include/goldibear_gpu.h: gb_circuit_set_partition, gb_prove_partition,
gb_prove_partition_retry, gb_expand_partition): PartitionWitness.values - one value per copy class - and
ProverOnlyCircuitData.representative_map go in, full_witness() runs on the device.
  * gb_expand_partition on the wired dummy circuit (tests/wired_circuits.py; its copy_classes give the partition, every class's
    value handed to a representative chosen by seed, some of them virtual targets) equals the witness matrix, from canonical and
    from p3 words, and gb_commit_values on that device matrix yields the cap of the host matrix;
  * proof bytes: gb_prove_partition == gb_prove on the expanded matrix == the oracle prover, both fields at 2^3, 2^6 and 2^12
    rows; the factorial circuit and a circuit of the recursion gate set through BuiltCircuit.prove (public inputs read through the
    map); a zero-knowledge circuit with salts; every proof accepted by gb_verify;
  * 2^16 rows, rate 8, 135 wires - the segmented wires commitment of >= 2^19 leaves - against gb_prove (the oracle is too slow
    there for a test of seconds);
  * the retry after InvZeroPermArg (armed through the test hook): gb_prove_partition_retry == gb_prove_partition on the re-drawn
    values == gb_prove_retry on the matrix, at 2^16 rows (state is kept) and 2^6 (none is);
  * errors: prove before set_partition, GB_INPUT_DEVICE, a value >= p in a used entry - and in an unused one, which is not looked at.
-m gpu."""
import ctypes as C

import numpy as np
import pytest

from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GpuContext, PermArgZeroError, PolynomialBatch, ShapeError
from plonky2_goldibear_amd import native as N
import circuits as CS
import partition_cases as PC
import wired_circuits as W

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": (GL, N.GB_GOLDILOCKS), "babybear": (BB, N.GB_BABYBEAR)}


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _config(F, degree_bits=0):
    # ((64 - degree_bits) * num_challenges >= 100, circuit_builder.rs:1190-1192: three challenges from 2^15 rows on)
    return D.CircuitConfig(num_challenges=3 if degree_bits >= 15 else 2) if F is GL else D.CircuitConfig.babybear(6)


def _wired(ctx, F, degree_bits, seed, dense="random"):
    """-> (oracle circuit, matrix, GPU circuit with the partition set, representative_map, values)"""
    circ, w, kw = W.wired_dummy_circuit(F, _config(F, degree_bits), degree_bits, seed, dense)
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    circ.set_cap(gpu.constants_sigmas_cap)
    m, values = PC.partition_of_witness(w, circ.copy_classes, seed)
    assert np.array_equal(PC.expand(m, values, circ.n, circ.cfg.num_wires), w)
    cells = circ.n * circ.cfg.num_wires
    reps = set(m[:cells].tolist())
    assert any(r >= cells for r in reps) and not set(range(cells, len(m))) <= reps   # virtual representatives, and unused ones
    gpu.set_partition(m)
    return circ, w, gpu, m, values


def _p3(a, F):
    """the same elements as the reference's field types hold them in memory"""
    if F is GL:
        out = a.copy()
        small = a < np.uint64((1 << 64) - GL.P)
        out[small] = a[small] + np.uint64(GL.P)
        return out
    return ((a.astype(np.uint64) << np.uint64(32)) % np.uint64(BB.P)).astype(np.uint32)


@pytest.mark.parametrize("degree_bits", [6, 12])
@pytest.mark.parametrize("field_name", sorted(FIELDS))
def test_expand_partition_is_the_witness_matrix_and_commits_to_its_cap(ctx, field_name, degree_bits):
    F, tag = FIELDS[field_name]
    circ, w, gpu, m, values = _wired(ctx, F, degree_bits, 700 + degree_bits, "edges")
    view = np.uint64 if F is GL else np.uint32
    dev = gpu.expand_partition(values)
    assert np.array_equal(dev.cpu().numpy().view(view), w)
    assert np.array_equal(gpu.expand_partition(_p3(values, F), p3_repr=True).cpu().numpy().view(view), w)
    host = PolynomialBatch.from_values(ctx, w, circ.cfg.rate_bits, circ.cfg.cap_height, field=tag)
    got = PolynomialBatch.from_values(ctx, dev, circ.cfg.rate_bits, circ.cfg.cap_height, field=tag)
    assert np.array_equal(got.merkle_tree.cap, host.merkle_tree.cap)
    # the stage that follows it in a host-driven prover loop reads the same buffer
    c = circ.cfg.num_challenges
    betas, gammas = [3 + i for i in range(c)], [11 + i for i in range(c)]
    assert np.array_equal(np.asarray(gpu.zs_partial_products(dev, betas, gammas).cpu()).view(view), gpu.zs_partial_products(w, betas, gammas))
    got.free(); host.free(); gpu.free()


@pytest.mark.parametrize("degree_bits", [3, 6, 12])
@pytest.mark.parametrize("field_name", sorted(FIELDS))
def test_partition_proof_bytes_equal_the_matrix_proof_and_the_oracle(ctx, field_name, degree_bits):
    F, tag = FIELDS[field_name]
    circ, w, gpu, m, values = _wired(ctx, F, degree_bits, 800 + degree_bits)
    want = D.prove_cpu(circ, w)[0]
    assert gpu.prove(w) == want
    got = gpu.prove_partition(values)
    assert got == want
    assert gpu.prove_partition(_p3(values, F), p3_repr=True) == want
    assert gpu.verify(got) and D.verify(circ, got)
    gpu.free()


def test_factorial_circuit_through_built_circuit_prove(ctx):
    b, pw = CS.factorial_circuit(count=60)
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    proof = c.prove(pw)                                       # generate_partition_witness + prove_partition
    assert proof == c.data.prove(w, pis)
    oc = CS.oracle_circuit(c, len(pis))
    oc.set_cap(c.data.constants_sigmas_cap)
    assert proof == D.prove_cpu(oc, w, pis)[0]
    assert c.verify(proof) and D.verify(oc, proof)
    assert [int(x) for x in np.frombuffer(proof[-16:], dtype=np.uint64)] == [int(x) for x in pis]   # read through the map


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_recursion_gate_set_through_built_circuit_prove(ctx, field):
    b, pw, _ = CS.recursion_gates_circuit(field, seed=9)
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    proof = c.prove(pw)
    assert proof == c.data.prove(w, pis)
    oc = CS.oracle_circuit(c, len(pis))
    oc.set_cap(c.data.constants_sigmas_cap)
    assert proof == D.prove_cpu(oc, w, pis)[0]
    assert c.verify(proof)


@pytest.mark.parametrize("field_name", sorted(FIELDS))
def test_zero_knowledge_circuit_with_salts(ctx, field_name):
    F, tag = FIELDS[field_name]
    circ = D.DummyCircuit(6, F=F) if F is GL else D.DummyCircuit(6, D.CircuitConfig.babybear(6), F=BB)
    circ.zero_knowledge = True
    n_lde = circ.n << circ.cfg.rate_bits
    salts = F.fill(0x5A17, 3 * 4 * n_lde).reshape(3, 4, n_lde)
    cfg = circ.cfg
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                      num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                      arity_bits=cfg.arity_bits, field=tag, zero_knowledge=True)
    circ.set_cap(gpu.constants_sigmas_cap)
    w = circ.witness(seed=4)
    m, values = PC.partition_of_witness(w, None, 4)
    gpu.set_partition(m)
    want = D.prove_cpu(circ, w, salts=salts)[0]
    assert gpu.prove(w, salts=salts) == want
    assert gpu.prove_partition(values, salts=salts) == want
    assert gpu.prove_partition(_p3(values, F), salts=_p3(np.ascontiguousarray(salts).reshape(-1), F), p3_repr=True) == want
    with pytest.raises(ShapeError):
        gpu.prove_partition(values)          # a zero-knowledge circuit needs its salts
    assert gpu.verify(want)
    gpu.free()


def test_segmented_wires_commitment_at_2_to_the_16_rows(ctx):
    """2^16 rows at rate 8 = 2^19 leaves, 135 wires: the wires commitment hashes its leaves in column segments and keeps the sponge
    state for the retry - fed here from the expanded device matrix"""
    circ, w, gpu, m, values = _wired(ctx, GL, 16, 816)
    assert circ.cfg.num_wires == 135 and circ.cfg.rate_bits == 3
    want = gpu.prove(w)
    assert gpu.prove_partition(values) == want
    assert gpu.verify(want)
    gpu.free()
    ctx.trim()


@pytest.mark.parametrize("degree_bits", [6, 16])
def test_retry_after_inv_zero_perm_arg(ctx, degree_bits):
    circ, w0, gpu, m, v0 = _wired(ctx, GL, degree_bits, 900 + degree_bits)
    nw = circ.cfg.num_wires
    rw = (nw - 1, circ.pi_row)                                  # (column, row): the last wire of the PublicInputGate row
    rep = int(m[circ.pi_row * nw + nw - 1])
    assert (m[:nw * circ.n] == rep).sum() == 1                  # alone in its class, as prover_data.random_wire is
    w, v = w0.copy(), v0.copy()
    w[rw] = v[rep] = np.uint64(0xFEDCBA9876543210 % GL.P)
    want = gpu.prove_once(w)
    assert gpu.prove_partition_once(v) == want
    gpu.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        gpu.prove_partition_once(v0)
    ctx.set_profiling(True)
    ctx.scope_reset()
    assert gpu.prove_partition_once(v, retry_wire=rw) == want
    # where the failed attempt kept its state (>= 2^19 leaves) the retry re-draws one cell of the kept matrix and transforms one
    # column: nothing is expanded again; at 2^6 rows nothing was kept and the retry is the full computation
    kept = degree_bits == 16
    assert ctx.scope_ms("compute full witness")[1] == 1
    assert ctx.scope_ms("partition expansion")[1] == (0 if kept else 1)
    ctx.set_profiling(False)
    gpu.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        gpu.prove_once(w0)
    assert gpu.prove_once(w, retry_wire=rw) == want
    # a retry with nothing kept (another proof in between) is the full computation
    gpu.arm_perm_arg_failure()
    with pytest.raises(PermArgZeroError):
        gpu.prove_partition_once(v0)
    assert gpu.prove_once(w0) != want
    assert gpu.prove_partition_once(v, retry_wire=rw) == want
    # the retry loop of the mirror: the re-drawn value goes into `values` at the representative
    vals = v0.copy()
    gpu.arm_perm_arg_failure()
    proof = gpu.prove_partition(vals, representative=rep, random_wire=rw, rng=np.random.default_rng(5))
    assert gpu.perm_arg_retries == 1 and vals[rep] != v0[rep] and gpu.verify(proof)
    assert proof == gpu.prove_once(PC.expand(m, vals, circ.n, nw))
    gpu.free()
    ctx.trim()


def test_errors(ctx):
    circ, w, kw = W.wired_dummy_circuit(GL, _config(GL), 6, 61, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    m, values = PC.partition_of_witness(w, circ.copy_classes, 61)
    lib, n = ctx._lib, C.c_size_t()
    buf = np.empty(1 << 20, dtype=np.uint8)

    def prove(v, flags=0):
        return lib.gb_prove_partition(gpu.handle, v.ctypes.data, flags, None, buf.ctypes.data, buf.size, C.byref(n))

    assert prove(values) == N.GB_ERR_INVALID and b"gb_circuit_set_partition" in lib.gb_last_error(ctx.handle)
    cells = circ.n * circ.cfg.num_wires
    u64p = C.POINTER(C.c_uint64)
    assert lib.gb_circuit_set_partition(gpu.handle, m.ctypes.data_as(u64p), cells - 1, None, 0) == N.GB_ERR_INVALID
    assert lib.gb_circuit_set_partition(gpu.handle, m.ctypes.data_as(u64p), 1 << 32, None, 0) == N.GB_ERR_UNSUPPORTED
    bad = m.copy()
    bad[5] = len(m)
    assert lib.gb_circuit_set_partition(gpu.handle, bad.ctypes.data_as(u64p), len(m), None, 0) == N.GB_ERR_INVALID
    one = np.array([len(m)], dtype=np.uint64)
    assert lib.gb_circuit_set_partition(gpu.handle, m.ctypes.data_as(u64p), len(m), one.ctypes.data_as(u64p), 1) == N.GB_ERR_INVALID
    assert prove(values) == N.GB_ERR_INVALID                                  # still not set
    gpu.set_partition(m)
    want = gpu.prove(w)
    assert prove(values) == N.GB_OK and buf[:n.value].tobytes() == want
    assert prove(values, N.GB_INPUT_DEVICE) == N.GB_ERR_INVALID
    assert prove(values, 4) == N.GB_ERR_INVALID
    used = np.unique(m[:cells]).astype(np.int64)
    unused = np.setdiff1d(np.arange(len(m)), used)
    assert unused.size > 0
    v = values.copy()
    v[unused] = np.uint64(GL.P)                                               # never read: not looked at
    assert prove(v) == N.GB_OK and buf[:n.value].tobytes() == want
    v = values.copy()
    v[used[len(used) // 2]] = np.uint64(GL.P)
    assert prove(v) == N.GB_ERR_INVALID and b"non-canonical witness element" in lib.gb_last_error(ctx.handle)
    dev_out = gpu.expand_partition(values)
    assert np.array_equal(dev_out.cpu().numpy().view(np.uint64), w)
    with pytest.raises(ShapeError):
        gpu.expand_partition(v)
    gpu.free()
