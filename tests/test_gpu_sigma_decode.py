"""gb_circuit_decode_sigmas / gb_circuit_copy_classes on the GPU (csrc/kernels_sigma.hip, csrc/sigma_host.inc): the copy permutation
read back out of the sigma columns, its cycles as copy classes, the witness check on them, the refusals and the comparison with a
partition.  Expected labels, counts and violations come from numpy over the class lists the sigmas were built from
(tests/sigma_cases.py) - never from the decoder.  Both fields; 2^2 .. 2^13 rows.  -m gpu only.

Two things differ from a first reading of the wiring helpers:
  * oracle.plonk_dummy.DummyCircuit wires a class of its own - the public-input row's first H wires and the constant row's wire 0 -
    which tests/wired_circuits.py's `copy_classes` does not list.  The sigmas hold it, so the expected labels and every partition
    compared with the sigmas include it (sigma_cases.full_copy_classes).
  * a circuit whose sigma is not a permutation cannot produce a proof that verifies, before or after a refused decode: the refusal
    tests check that prove() on the handle returns the bytes it returned before the refusal, and that those verify where the
    circuit itself is sound (the k_is and flags refusals)."""
import os
import subprocess

import numpy as np
import pytest

import partition_cases as PC
import sigma_cases as SC
import sigma_decode_cases as SD
import wired_circuits as W
import witness_check_cases as WC
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GpuContext, ShapeError, SigmaInfo, VerifyError
from plonky2_goldibear_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [GL, BB]
IDS = ["goldilocks", "babybear"]
ALL = 1 << 16


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def dummy_config(F):
    return D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6)


def make(ctx, circ, kw):
    return CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)


def assert_info(info, classes, n, nr, compared=0):
    want = SC.info_of(classes, n, nr)
    assert isinstance(info, SigmaInfo)
    assert {k: getattr(info, k) for k in want} == want
    assert info.compared_partition == compared
    assert 1 <= info.rounds <= max(1, int(np.ceil(np.log2(want["largest_class"])))) + 1


def assert_decodes_to(gpu, classes, n, nw, nr, compared=0):
    info = gpu.decode_sigmas()
    assert_info(info, classes, n, nr, compared)
    got, want = gpu.copy_classes(), SC.labels_of(classes, n, nw)
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first difference at cell %d: %d, expected %d" % (bad[0], got[bad[0]], want[bad[0]])
    nonrouted = (np.arange(n * nw) % nw) >= nr
    assert (got[nonrouted] == np.arange(n * nw)[nonrouted]).all()
    return info


# ------------------------------------------------------------------------------------------------ 0. the device build of the header
@pytest.fixture(scope="module")
def device_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("sigma_decode_dev") / "sigma_decode"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "sigma_decode.hip")],
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SD.FIELDS))
def test_device_functions_decode_the_case_table(device_exe, tmp_path, name):
    F = SD.FIELDS[name]
    table = SD.cases(F)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    SD.pack(F, table).tofile(src)
    out = subprocess.run([device_exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    bad = SD.compare(table, np.fromfile(dst, dtype=np.uint64))
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------------------------------------------ 1. labels equal the builder's classes
@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits", [2, 3, 5, 13])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_labels_equal_the_builders_classes(ctx, F, degree_bits):
    if degree_bits == 2:   # DummyCircuit starts at 2^3 rows: 2^2 NoopGate rows of the small configuration
        circ = SC.SmallRoutedCircuit(F, degree_bits=2, num_routed=5, num_wires=9, seed=11)
        kw, classes = circ.gpu_kwargs, circ.copy_classes
    else:
        circ, _, kw = W.wired_dummy_circuit(F, dummy_config(F), degree_bits, 7, "random")
        classes = SC.full_copy_classes(circ)
    gpu = make(ctx, circ, kw)
    assert_decodes_to(gpu, classes, circ.n, circ.cfg.num_wires, circ.cfg.num_routed_wires)
    gpu.free()


@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_labels_with_three_routed_wires(ctx, F):
    circ = SC.SmallRoutedCircuit(F, degree_bits=4, num_routed=3, num_wires=5, seed=3)
    gpu = make(ctx, circ, circ.gpu_kwargs)
    assert_decodes_to(gpu, circ.copy_classes, circ.n, 5, 3)
    gpu.free()


@pytest.mark.gpu
def test_labels_where_the_tables_lie_in_global_memory(ctx):
    """2^23 Goldilocks rows: the discrete-log tables (2^12 entries, 72 KiB) no longer fit the decode kernel's LDS budget, so the
    kernel reads them from global memory - its other instantiation.  One wire, so that the circuit stays small; rows 0 and n - 1
    are wired.  (BabyBear reaches that size at 2^25 rows, past what its two-adicity leaves for a rate of 8.)"""
    circ = SC.SingleWireCircuit(GL, 23)
    gpu = make(ctx, circ, circ.gpu_kwargs)
    info = assert_decodes_to(gpu, circ.copy_classes, circ.n, 1, 1)
    assert info.largest_class == 300 and info.num_classes == 1001
    gpu.free()


# ------------------------------------------------------------------------------------------------ 2. long and awkward cycles
def wide_config(F):
    return D.CircuitConfig(num_challenges=2) if F is GL else D.CircuitConfig.babybear(6, num_wires=135, num_routed_wires=80)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.AWKWARD)
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_long_and_awkward_cycles(ctx, F, name):
    cfg = wide_config(F)
    base = D.DummyCircuit(10, cfg, F=F)
    lists = SC.awkward_classes(name, base.n, base.pi_row, base.const_row)
    circ, kw = SC.circuit_from_classes(F, cfg, 10, lists)
    n, nw = circ.n, cfg.num_wires
    assert (cfg.num_wires, cfg.num_routed_wires) == (135, 80)
    longest = max(len(c) for c in lists)
    assert longest == {"two_columns": 2 * (n - 2), "cycle_64": 64, "cycle_65": 65}[name]
    first = lists[0]   # lowest in cell order is not lowest in sigma's order
    assert min(first) != min(first, key=lambda c: (c % n) * nw + c // n)
    gpu = make(ctx, circ, kw)
    info = assert_decodes_to(gpu, SC.full_copy_classes(circ), n, nw, cfg.num_routed_wires)
    assert info.largest_class == longest and info.rounds <= int(np.ceil(np.log2(longest))) + 1
    gpu.free()


# ------------------------------------------------------------------------------------------------ 3. the check agrees with the partition path
def copy_test_circuit(F):
    """the circuit and the broken witnesses of tests/test_gpu_witness_check.py's copy test"""
    circ, w, kw = W.wired_dummy_circuit(F, dummy_config(F), 6, 7, "random")
    nw, n = w.shape
    cells, starts, sizes = circ.copy_classes
    t = int(np.flatnonzero(sizes >= 3)[0])
    members = sorted(int(r) * nw + int(col) for col, r in (divmod(int(x), n) for x in cells[starts[t]:starts[t] + sizes[t]]))

    def broken(cell, also_pi_row=False):
        bad = w.copy()
        bad[cell % nw, cell // nw] = (int(bad[cell % nw, cell // nw]) + 1) % F.P
        if also_pi_row:
            bad[0, circ.pi_row] = 5
        return bad

    return circ, w, kw, [broken(members[1]), broken(members[0], also_pi_row=True)]


def reported(got):
    violations, res = got
    return ([v.as_tuple() for v in violations], (res.num_gate_violations, res.num_selector_violations, res.num_copy_violations, res.num_listed))


@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_the_check_agrees_with_the_partition_path(ctx, F):
    circ, w, kw, broken = copy_test_circuit(F)
    classes = SC.full_copy_classes(circ)
    m, _ = PC.partition_of_witness(w, classes, 4)
    by_partition, by_sigma, neither = make(ctx, circ, kw), make(ctx, circ, kw), make(ctx, circ, kw)
    by_partition.set_partition(m)
    by_sigma.decode_sigmas()
    labels = SC.labels_of(classes, circ.n, circ.cfg.num_wires).astype(np.uint64)
    for gpu, copies in ((by_partition, 1), (by_sigma, 2), (neither, 0)):
        violations, res = gpu.check_witness(w)
        assert violations == [] and res.copies_checked == copies and res.num_copy_violations == 0
    for i, bad in enumerate(broken):
        want = WC.expected_dummy(circ, bad) + WC.copy_violations(labels, bad)
        assert WC.counts(want)[2] >= 1 and WC.counts(want)[0] == i
        a, b = by_partition.check_witness(bad, max_violations=ALL), by_sigma.check_witness(bad, max_violations=ALL)
        WC.same(b[0], want)
        assert reported(a) == reported(b)
        assert (a[1].copies_checked, b[1].copies_checked) == (1, 2)
        c = neither.check_witness(bad, max_violations=ALL)
        assert c[1].copies_checked == 0 and c[1].num_copy_violations == 0
        # a short list: the same first entries, the same exact counts
        a, b = by_partition.check_witness(bad, max_violations=2), by_sigma.check_witness(bad, max_violations=2)
        assert reported(a) == reported(b) and b[1].num_copy_violations == WC.counts(want)[2]
    for gpu in (by_partition, by_sigma, neither):
        gpu.free()


# ------------------------------------------------------------------------------------------------ 4. "check_witness" in front of gb_prove
@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_check_witness_option_on_a_circuit_without_a_partition(ctx, F):
    circ, w, kw = W.wired_dummy_circuit(F, dummy_config(F), 6, 5, "random")
    bad = W.break_copy_constraint(circ, w)
    labels = SC.labels_of(SC.full_copy_classes(circ), circ.n, circ.cfg.num_wires).astype(np.uint64)
    want = WC.copy_violations(labels, bad)
    assert want and not WC.expected_dummy(circ, bad)
    gpu = make(ctx, circ, kw)
    plain = gpu.prove_once(w)
    assert gpu.verify(plain)
    try:
        ctx.set_option("check_witness", 1)
        proof = gpu.prove_once(bad)                       # today's behaviour: nothing knows the wiring
        with pytest.raises(VerifyError, match="vanishing"):
            gpu.verify(proof)
        gpu.decode_sigmas()
        with pytest.raises(N.UnsatisfiedError) as e:
            gpu.prove_once(bad)
        assert e.value.status == N.GB_ERR_UNSATISFIED and e.value.violations[0] == want[0]
        assert "row %d, wire %d" % (want[0].row, want[0].index) in str(e.value)
        assert gpu.prove_once(w) == plain                 # the intact witness: the bytes of the unchecked proof
    finally:
        ctx.set_option("check_witness", 0)
    gpu.free()


# ------------------------------------------------------------------------------------------------ 5. refusals
def refusal_circuit(F):
    circ, w, kw = W.wired_dummy_circuit(F, dummy_config(F), 3, 2, "random")
    return circ, w, kw, circ.cfg.num_routed_wires, circ.cfg.num_wires


def with_sigma_value(circ, col, row, value):
    cs = circ.constants_sigmas.copy()
    cs[circ.num_constants + col, row] = value
    return cs


def assert_refused_and_usable(ctx, gpu, w, match, soundly_wired):
    before = gpu.prove_once(w)
    with pytest.raises(ShapeError, match=match) as e:
        gpu.decode_sigmas()
    assert e.value.status == N.GB_ERR_INVALID
    with pytest.raises(ShapeError, match="have not been decoded"):
        gpu.copy_classes()
    assert gpu.prove_once(w) == before
    if soundly_wired:
        assert gpu.verify(before)
    violations, res = gpu.check_witness(w)
    assert violations == [] and res.copies_checked == 0
    gpu.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["zero", "unrouted_coset", "shared_target"])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_refused_sigma_values(ctx, F, case):
    circ, w, kw, nr, nw = refusal_circuit(F)
    p, n = F.P, circ.n
    col, row = 2, 3
    if case == "zero":
        value, match = 0, r"names no routed cell at row 3, wire 2: the value 0 "
    elif case == "unrouted_coset":
        value = pow(F.generator, nr, p) * pow(F.two_adic_generator(3), 5, p) % p
        match = r"names no routed cell at row 3, wire 2: the value %d " % value
    else:
        other_col, other_row = 7, 1                   # the lower cell of the two in row * num_wires + col order
        value = int(circ.sigma[other_col, other_row])
        assert value != int(circ.sigma[col, row])
        tcol, trow = SD.expect(F, 3, [int(k) for k in circ.k_is], value)
        match = r"not a permutation: row 1, wire 7 and another cell both go to row %d, wire %d$" % (trow, tcol)
    gpu = CircuitData(ctx, 3, with_sigma_value(circ, col, row, value), circ.k_is, **kw)
    assert_refused_and_usable(ctx, gpu, w, match, soundly_wired=False)


def rewired_for(circ, F, k_new):
    """the circuit's constants_sigmas with every sigma value re-encoded for other k_is: the same cells, named through k_new"""
    p, n = F.P, circ.n
    k_old = [int(k) for k in circ.k_is]
    sub = [int(s) for s in circ.subgroup]
    cell_of = {k * s % p: (c, r) for c, k in enumerate(k_old) for r, s in enumerate(sub)}
    cs = circ.constants_sigmas.copy()
    for c in range(len(k_old)):
        for r in range(n):
            tc, tr = cell_of[int(circ.sigma[c, r])]
            cs[circ.num_constants + c, r] = k_new[tc] * sub[tr] % p
    return cs


@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_refused_k_is_and_flags(ctx, F):
    circ, w, kw, nr, nw = refusal_circuit(F)
    k_new = [int(k) for k in circ.k_is]
    k_new[1] = k_new[0] * F.two_adic_generator(3) % F.P       # the coset of entry 0 again
    # the witness is constant on every class and the wiring is unchanged, so the proof still verifies: the k_is are merely useless
    gpu = CircuitData(ctx, 3, rewired_for(circ, F, k_new), np.array(k_new, dtype=F.dtype), **kw)
    assert_refused_and_usable(ctx, gpu, w, "k_is do not name distinct cosets", soundly_wired=True)
    gpu = make(ctx, circ, kw)
    before = gpu.prove_once(w)
    with pytest.raises(ShapeError, match="flags must be 0"):
        gpu.decode_sigmas(flags=1)
    with pytest.raises(ShapeError, match="have not been decoded"):
        gpu.copy_classes()
    assert gpu.prove_once(w) == before and gpu.verify(before)
    assert_decodes_to(gpu, SC.full_copy_classes(circ), circ.n, nw, nr)   # and nothing stands in the way of a proper call
    gpu.free()


# ------------------------------------------------------------------------------------------------ 6. partition comparison
@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_partition_comparison(ctx, F):
    circ, w, kw, broken = copy_test_circuit(F)
    n, nw, nr = circ.n, circ.cfg.num_wires, circ.cfg.num_routed_wires
    classes = SC.full_copy_classes(circ)
    cells, starts, sizes = classes
    labels = SC.labels_of(classes, n, nw).astype(np.uint64)
    # two representative choices for the same classes: both agree with the sigmas, whichever is set when the sigmas are decoded
    m4, _ = PC.partition_of_witness(w, classes, 4)
    m5, _ = PC.partition_of_witness(w, classes, 5)
    assert (m4 != m5).any()
    gpu = make(ctx, circ, kw)
    gpu.set_partition(m4)
    assert_decodes_to(gpu, classes, n, nw, nr, compared=1)
    gpu.set_partition(m5)                                  # the labels stay; the new map is compared on the next call
    assert gpu.decode_sigmas().compared_partition == 1
    gpu.free()
    gpu = make(ctx, circ, kw)
    assert gpu.decode_sigmas().compared_partition == 0
    gpu.set_partition(m5)
    assert gpu.decode_sigmas().compared_partition == 1
    gpu.free()

    def cell_index(c):
        return (int(c) % n) * nw + int(c) // n

    big = [int(t) for t in np.flatnonzero(sizes >= 2)[:2]]
    members = [sorted(cell_index(c) for c in cells[starts[t]:starts[t] + sizes[t]]) for t in big]
    # two classes merged: the class with the higher first cell now starts at the other's
    merged = m4.copy()
    for c in members[1]:
        merged[c] = m4[members[0][0]]
    moved = members[1] if members[0][0] < members[1][0] else members[0]
    # one cell left out of its class: it stands alone (the first cell left out: the rest start at the second)
    alone = m4.copy()
    left = members[0][1]
    if int(m4[left]) == left:                              # the cell represents its class: hand the class to another member
        for c in members[0]:
            alone[c] = members[0][0]
    alone[left] = left
    for wrong, where, first_by_partition in ((merged, moved[0], min(members[0][0], members[1][0])), (alone, left, left)):
        gpu = make(ctx, circ, kw)
        gpu.set_partition(wrong)
        match = r"partition and sigma disagree at row %d, wire %d \(partition: first cell %d, sigma: first cell %d\)" % (
            where // nw, where % nw, first_by_partition, int(labels[where]))
        with pytest.raises(ShapeError, match=match):
            gpu.decode_sigmas()
        with pytest.raises(ShapeError, match="have not been decoded"):
            gpu.copy_classes()
        # the partition-based check works as before, on the map it was given
        for bad in [w] + broken:
            want = WC.expected_dummy(circ, bad) + WC.copy_violations(wrong, bad)
            violations, res = gpu.check_witness(bad, max_violations=ALL)
            WC.same(violations, want)
            assert res.copies_checked == 1 and res.num_copy_violations == WC.counts(want)[2]
        gpu.free()


# ------------------------------------------------------------------------------------------------ 7. idempotence and lifetime
@pytest.mark.gpu
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_idempotence_and_lifetime(ctx, F):
    circ, w, kw, broken = copy_test_circuit(F)
    gpu = make(ctx, circ, kw)
    first = gpu.decode_sigmas()
    labels = gpu.copy_classes()
    ctx.set_profiling(True)
    try:
        ctx.scope_reset()
        assert gpu.decode_sigmas() == first                # no device work: no timing scope has run
        assert all(ctx.scope_ms("decode sigmas: " + s)[1] == 0 for s in ("decode", "classes", "compare"))
    finally:
        ctx.set_profiling(False)
    assert (gpu.copy_classes() == labels).all()
    assert gpu.check_witness(broken[0])[1].copies_checked == 2
    ctx.trim()
    violations, res = gpu.check_witness(broken[0])         # the check decodes nothing by itself
    assert res.copies_checked == 0 and res.num_copy_violations == 0
    with pytest.raises(ShapeError, match="have not been decoded"):
        gpu.copy_classes()
    assert gpu.decode_sigmas() == first
    assert (gpu.copy_classes() == labels).all()
    res = gpu.check_witness(broken[0])[1]
    assert res.copies_checked == 2 and res.num_copy_violations == 1
    gpu.free()
