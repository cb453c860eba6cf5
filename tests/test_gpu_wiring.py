"""gb_wiring_sigmas on the GPU (csrc/kernels_wiring.hip, csrc/wiring_host.inc): copy constraints turned into sigma columns and a
representative map.  Expected maps, sigmas and counts come from tests/wiring_cases.py - a plain Python union-find and Python
integers - and, for builder circuits, from CircuitBuilder._sigma; never from the code under test.  Both fields; 2^2 .. 2^13 rows
(2^16 for the one-wire shapes).  -m gpu only.

`rounds` of gb_wiring_info is not compared: the lock-free merges leave the forest in a shape that depends on the order the device
ran them in, and the number of compression passes with it (include/goldibear_gpu.h says so); it is only required to be at least 1.
Every other count, the map and the sigmas are compared in full."""
import functools

import numpy as np
import pytest

import gadget_cases as GA
import generator_program_circuits as GPC
import wiring_cases as WC
from circuits import babybear_public_input_circuit, factorial_circuit, oracle_circuit
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GoldibearError, GpuContext, ShapeError, WiringInfo, sigma_polys, wiring
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import ArithmeticGate
from plonky2_goldibear_amd.gate_program import GATE_PROGRAM

pytestmark = pytest.mark.gpu
FIELDS = [GL, BB]
IDS = ["goldilocks", "babybear"]
TILE = wiring.SORT_TILE
SEED = 23


def tag(F):
    return N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def family_cases(degree_bits, wires):
    return {c.name: c for c in WC.families(degree_bits, wires, TILE)}


def run(ctx, F, case, device=False):
    return sigma_polys(ctx, tag(F), case.degree_bits, case.num_wires, case.num_routed, WC.k_is_of(F, case.num_routed), case.pairs,
                       case.num_targets, device=device)


def assert_equals_expected(F, case, got):
    sig, rep, info = got
    want_rep, _, _, want_info = WC.structure(case)
    assert isinstance(info, WiringInfo) and info.rounds >= 1
    assert {k: getattr(info, k) for k in want_info} == want_info, case
    assert rep.dtype == np.uint64 and np.array_equal(rep, want_rep), case
    want = WC.sigmas(case, F)
    assert sig.dtype == want.dtype and sig.shape == want.shape
    bad = np.argwhere(sig != want)
    assert not len(bad), "%r: %d values differ, first at wire %d, row %d" % (case, len(bad), bad[0][0], bad[0][1])


# ------------------------------------------------------------------------------------------------ 1. the case families
SMALL_NAMES = ["no_pairs", "one_pair", "self_pair", "same_pair_thrice", "random_1_to_5", "all_path_ascending", "all_path_descending",
               "all_path_shuffled", "all_star_highest", "row_and_column", "virtual_chain_of_three", "virtual_only_class", "virtual_unused",
               "exactly_the_wire_targets"]


@pytest.mark.parametrize("degree_bits", [2, 3, 5, 10])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_case_families_at_nine_wires(ctx, F, degree_bits):
    cases = family_cases(degree_bits, WC.SMALL)
    names = SMALL_NAMES + (["awkward_pair"] if degree_bits >= 5 else []) + (
        ["sizes_around_wave_and_tile", "straddles_a_tile_boundary"] if degree_bits == 10 else [])
    assert set(names) == set(cases)
    for name in names:
        assert_equals_expected(F, cases[name], run(ctx, F, cases[name]))


@pytest.mark.parametrize("name", ["all_path_ascending", "all_path_descending", "awkward_pair", "sizes_around_wave_and_tile",
                                  "straddles_a_tile_boundary", "virtual_chain_of_three", "exactly_the_wire_targets"])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_case_families_at_standard_width(ctx, F, name):
    case = family_cases(10, WC.STANDARD)[name]
    assert_equals_expected(F, case, run(ctx, F, case))


@pytest.mark.parametrize("name", ["random_1_to_5", "all_path_shuffled", "all_star_highest"])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_the_largest_shape(ctx, F, name):
    """2^13 rows of 135 / 80 wires: 1.1 M cells, 655 360 of them routed - for the two all-in-one-class cases in ONE class: the
    deepest chains and the heaviest contention the union-find sees, and a sort whose every key is equal"""
    case = family_cases(13, WC.STANDARD)[name]
    assert_equals_expected(F, case, run(ctx, F, case))


@pytest.mark.parametrize("num_wires", [1, 2])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_one_routed_wire_at_65536_rows(ctx, F, num_wires):
    """labels below 2^16 with one wire - two digits, the third pass skipped - and up to 2^17 - 2 with two wires, one routed: three
    digits; classes through the rows whose labels lie on both sides of the digit boundaries"""
    case = WC.single_wire(16, num_wires)
    assert wiring_passes(case.cells) == (2 if num_wires == 1 else 3)
    got = run(ctx, F, case)
    assert got[2].largest_class == 300 and got[2].num_classes == 1002
    assert_equals_expected(F, case, got)


def wiring_passes(limit):
    return (max(limit - 1, 0).bit_length() + 7) // 8


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_three_runs_give_the_same_bytes(ctx, F):
    case = family_cases(13, WC.STANDARD)["all_path_shuffled"]
    first = run(ctx, F, case)
    for _ in range(2):
        sig, rep, info = run(ctx, F, case)
        assert sig.tobytes() == first[0].tobytes() and rep.tobytes() == first[1].tobytes()
        assert info._replace(rounds=0) == first[2]._replace(rounds=0)


# ------------------------------------------------------------------------------------------------ 3. device output
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_device_output_equals_host_output(ctx, F):
    import torch
    for case in (family_cases(5, WC.SMALL)["random_1_to_5"], family_cases(10, WC.STANDARD)["sizes_around_wave_and_tile"]):
        host = run(ctx, F, case)
        dev = run(ctx, F, case, device=True)
        assert isinstance(dev[0], torch.Tensor) and dev[0].is_cuda and tuple(dev[0].shape) == host[0].shape
        assert dev[0].cpu().numpy().view(host[0].dtype).tobytes() == host[0].tobytes()
        assert np.array_equal(dev[1], host[1]) and dev[2]._replace(rounds=0) == host[2]._replace(rounds=0)


def builder_pairs(b, built):
    return np.array([(built.target_index(x), built.target_index(y)) for x, y in b.copy_constraints], dtype=np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_a_circuit_from_device_columns_has_the_same_cap(ctx, F):
    """gb_circuit_create_gates_cols(.., GB_INPUT_DEVICE) with the sigma columns named where gb_wiring_sigmas wrote them"""
    import torch
    b, _ = factorial_circuit(count=60) if F is GL else babybear_public_input_circuit(steps=30)
    built = b.build(ctx)
    cfg = built.config
    sig, rep, _ = sigma_polys(ctx, cfg.field, built.degree_bits, cfg.num_wires, cfg.num_routed_wires, built.k_is, builder_pairs(b, built),
                              built.num_targets, device=True)
    head = built.constants_sigmas[:built.num_selectors + built.max_constants]
    signed = np.int64 if F is GL else np.int32
    cols = [torch.from_numpy(np.ascontiguousarray(c).view(signed)).to(sig.device) for c in head] + [sig[j] for j in range(sig.shape[0])]
    torch.cuda.synchronize()
    kw = dict(num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires, num_constants=built.max_constants,
              num_challenges=cfg.num_challenges, max_quotient_degree_factor=cfg.max_quotient_degree_factor, rate_bits=cfg.rate_bits,
              cap_height=cfg.cap_height, proof_of_work_bits=cfg.proof_of_work_bits, num_query_rounds=cfg.num_query_rounds,
              arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits, num_selectors=built.num_selectors, field=cfg.field,
              gates=built.gate_table, num_public_inputs=len(built.public_inputs),
              reduction_arity_bits=cfg.reduction_arity_bits(built.degree_bits))
    gpu = CircuitData(ctx, built.degree_bits, cols, built.k_is, **kw)
    assert np.array_equal(gpu.constants_sigmas_cap, built.data.constants_sigmas_cap)
    assert np.array_equal(gpu.circuit_digest, built.data.circuit_digest)
    gpu.free()
    built.data.free()


# ------------------------------------------------------------------------------------------------ 4. against the decoder
def bare_circuit(ctx, F, case, sig):
    """a circuit of NoopGate rows around the given sigma columns (as tests/sigma_cases.py SmallRoutedCircuit makes one)"""
    cfg = D.CircuitConfig(num_challenges=2 if F is GL else 6, num_wires=case.num_wires, num_routed_wires=case.num_routed,
                          arity_bits=4 if F is GL else 3)
    cs = np.concatenate([np.zeros((1 + cfg.num_constants, case.n), dtype=F.dtype), sig])
    return CircuitData(ctx, case.degree_bits, cs, WC.k_is_of(F, case.num_routed), num_wires=case.num_wires,
                       num_routed_wires=case.num_routed, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                       arity_bits=cfg.arity_bits, gate_constant=1, gate_pi=2, field=tag(F))


@pytest.mark.parametrize("shape", [(5, WC.SMALL, "random_1_to_5"), (10, WC.SMALL, "sizes_around_wave_and_tile"),
                                   (10, WC.STANDARD, "all_path_shuffled"), (10, WC.STANDARD, "virtual_chain_of_three"),
                                   (13, WC.STANDARD, "random_1_to_5")], ids=lambda s: "%s-2^%d-%dw" % (s[2], s[0], s[1][0]))
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_the_decoder_reads_the_same_wiring_back(ctx, F, shape):
    case = family_cases(shape[0], shape[1])[shape[2]]
    sig, rep, info = run(ctx, F, case)
    gpu = bare_circuit(ctx, F, case, sig)
    gpu.set_partition(rep)
    back = gpu.decode_sigmas()
    assert back.compared_partition == 1
    assert (back.moved_cells, back.num_classes, back.largest_class) == (info.moved_cells, info.num_classes, info.largest_class)
    assert np.array_equal(gpu.copy_classes().astype(np.uint64), rep[:case.cells])
    gpu.free()


# ------------------------------------------------------------------------------------------------ 5. through the builder
def range_check_circuit(field):
    return next((b, pw) for name, b, pw in GA.builder_circuits(field, 6) if name == "split_low_high")


def program_gate_circuit(field):
    """a multiply-add chain whose gates are constraint programs and whose generators are generator programs"""
    cfg = GA.config(field)
    _, b, pw = GPC.poly_chain_pair(cfg, 40 * ArithmeticGate.new_from_config(cfg).num_ops)
    return b, pw


BUILDER_CIRCUITS = {
    "factorial": lambda field: factorial_circuit(count=60) if field == N.GB_GOLDILOCKS else babybear_public_input_circuit(steps=30),
    "range_check": range_check_circuit,
    "program_gate": program_gate_circuit,
}


@pytest.mark.parametrize("name", sorted(BUILDER_CIRCUITS))
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_the_builder_with_device_wiring_gives_the_same_circuit_and_proof(ctx, F, name):
    b0, pw = BUILDER_CIRCUITS[name](tag(F))
    b1, _ = BUILDER_CIRCUITS[name](tag(F))
    host, dev = b0.build(ctx), b1.build(ctx, wiring="device")
    assert dev.constants_sigmas.dtype == host.constants_sigmas.dtype and np.array_equal(dev.constants_sigmas, host.constants_sigmas)
    assert np.array_equal(dev.data.constants_sigmas_cap, host.data.constants_sigmas_cap)
    # the map's representatives are the class minima; it names the same classes as the host forest
    hm, dm = host.representative_map, dev.representative_map
    assert np.array_equal(dm[dm.astype(np.int64)], dm) and (dm <= np.arange(dm.size, dtype=np.uint64)).all()
    assert np.array_equal(dm[hm.astype(np.int64)], dm) and np.array_equal(hm[dm.astype(np.int64)], hm)
    want = host.prove_inputs(pw, np.random.default_rng(SEED))
    got = dev.prove_inputs(pw, np.random.default_rng(SEED))
    assert got == want
    assert dev.prove(pw, np.random.default_rng(SEED)) == host.prove(pw, np.random.default_rng(SEED)) == want   # the Python witness path
    assert dev.verify(got) and host.verify(got)
    if name == "factorial":
        oc = oracle_circuit(dev, len(dev.public_inputs))
        oc.set_cap(dev.data.constants_sigmas_cap)
        assert D.verify(oc, got)
    assert any(g[0] == GATE_PROGRAM for g in dev.gate_table) == (name == "program_gate")
    host.data.free()
    dev.data.free()


def test_the_builder_refuses_device_wiring_without_a_context():
    b, _ = factorial_circuit(count=3)
    with pytest.raises(ValueError):
        b.build(None, wiring="device")
    with pytest.raises(ValueError):
        b.build(None, wiring="gpu")


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.fixture(scope="module")
def prover(ctx):
    b, pw = factorial_circuit(count=20)
    c = b.build(ctx)
    yield c, pw, c.prove(pw)
    c.data.free()


def call(ctx, field=N.GB_GOLDILOCKS, degree_bits=3, num_wires=9, num_routed=5, k_is=None, pairs=((0, 1),), num_targets=None, flags=0,
         null=()):
    """gb_wiring_sigmas as it is, so that every argument can be wrong"""
    import ctypes as C
    dt = np.uint64 if field != N.GB_BABYBEAR else np.uint32
    k = np.array([pow(7, i, 2013265921) for i in range(max(num_routed, 1))] if k_is is None else k_is, dtype=dt)
    p = np.array(pairs, dtype=np.uint64).reshape(-1, 2)
    cells = num_wires << degree_bits
    nt = cells + 2 if num_targets is None else num_targets
    sig = np.zeros(max(num_routed, 1) << min(degree_bits, 20), dtype=dt)
    rep = np.zeros(min(nt, 1 << 20), dtype=np.uint64)
    info = N.gb_wiring_info()
    args = dict(k_is=k.ctypes.data, pairs=p.ctypes.data_as(C.POINTER(C.c_uint64)), sigmas=sig.ctypes.data)
    for name in null:
        args[name] = None
    return ctx._lib.gb_wiring_sigmas(ctx.handle, field, degree_bits, num_wires, num_routed, args["k_is"], args["pairs"], len(p), nt, flags,
                                     args["sigmas"], rep.ctypes.data_as(C.POINTER(C.c_uint64)), C.cast(C.pointer(info), C.c_void_p))


def last_error(ctx):
    return ctx._lib.gb_last_error(ctx.handle).decode()


CELLS = 9 << 3
REFUSALS = [
    ("null k_is", dict(null=("k_is",)), N.GB_ERR_INVALID, "null argument"),
    ("null pairs", dict(null=("pairs",)), N.GB_ERR_INVALID, "null argument"),
    ("null sigmas_out", dict(null=("sigmas",)), N.GB_ERR_INVALID, "null argument"),
    ("field tag", dict(field=2), N.GB_ERR_INVALID, "unknown field tag"),
    ("no routed wires", dict(num_routed=0), N.GB_ERR_INVALID, "num_routed_wires"),
    ("more routed than wires", dict(num_routed=10), N.GB_ERR_INVALID, "num_routed_wires"),
    ("too few targets", dict(num_targets=CELLS - 1), N.GB_ERR_INVALID, "below degree * num_wires"),
    ("k_is not canonical", dict(k_is=[1, 7, 0xFFFFFFFF00000001, 343, 2401]), N.GB_ERR_INVALID, "k_is[2]"),
    ("k_is not canonical, babybear", dict(field=N.GB_BABYBEAR, k_is=[1, 31, 961, 2013265921, 5]), N.GB_ERR_INVALID, "k_is[3]"),
    ("pair out of range", dict(pairs=[(0, 1), (2, 3), (CELLS + 2, 0), (1, 2), (0, CELLS + 9)]), N.GB_ERR_INVALID,
     "copy constraint 2 names target %d" % (CELLS + 2)),
    ("pair not routable", dict(pairs=[(0, 1), (9, 9 + 5), (1, 2), (8, 0)]), N.GB_ERR_INVALID,
     "Tried to route a wire that isn't routable: copy constraint 1, target 14 (row 1, wire 5)"),
    ("flags", dict(flags=2), N.GB_ERR_INVALID, "flags other than GB_INPUT_DEVICE"),
    ("flags, high bit", dict(flags=0x101), N.GB_ERR_INVALID, "flags other than GB_INPUT_DEVICE"),
    ("2^32 targets", dict(num_targets=1 << 32), N.GB_ERR_UNSUPPORTED, "2^32 targets"),
    ("two-adicity, goldilocks", dict(degree_bits=33, num_wires=1, num_routed=1, num_targets=1 << 40), N.GB_ERR_UNSUPPORTED, "two-adicity"),
    ("two-adicity, babybear", dict(field=N.GB_BABYBEAR, degree_bits=28, num_wires=1, num_routed=1, num_targets=1 << 28),
     N.GB_ERR_UNSUPPORTED, "two-adicity"),
]


@pytest.mark.parametrize("what,kw,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_what_is_wrong_and_leave_the_context_usable(ctx, prover, what, kw, status, message):
    assert call(ctx) == N.GB_OK
    assert call(ctx, **kw) == status
    assert message in last_error(ctx), last_error(ctx)
    c, pw, proof = prover
    again = c.prove(pw)
    assert again == proof and c.verify(again)
    assert call(ctx) == N.GB_OK


def test_the_python_wrapper_raises(ctx):
    with pytest.raises(ShapeError, match="isn't routable"):
        sigma_polys(ctx, N.GB_GOLDILOCKS, 3, 9, 5, WC.k_is_of(GL, 5), [(0, 5)], CELLS)
    with pytest.raises(GoldibearError) as e:
        sigma_polys(ctx, N.GB_GOLDILOCKS, 3, 9, 5, WC.k_is_of(GL, 5), [], 1 << 32)
    assert e.value.status == N.GB_ERR_UNSUPPORTED
