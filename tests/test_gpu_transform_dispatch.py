"""Every dispatch branch of the transform layer (csrc/ntt_passes.hpp, kernels_ntt16.hip, kernels_bb16.hip, ntt_outer.hpp) against the
CPU oracle's transforms: the cases of tests/transform_cases.py through PolynomialBatch.  Coefficients against ifft, leaves against the
bit-reversed coset_fft (shift 7 / 31) of the coefficients padded to N - every one of them, except where a case is "sampled".
The passes are bit-exact integer code: a wrong twiddle, coset factor or column offset shows in every case that reaches it.

The oracle's transforms are single-threaded C calls that release the GIL, so the reference work of the selected cases (inputs included)
runs on a pool of the host's CPU share (never more than $OMP_NUM_THREADS), started with the module, while the GPU goes through the
cases in order.  -m gpu."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import transform_cases as T
from oracle import oracle as O
from oracle import oracle_bb as B
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, PolynomialBatch
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu

FIELD = {T.GL: (GL, O, N.GB_GOLDILOCKS, np.int64), T.BB: (BB, B, N.GB_BABYBEAR, np.int32)}


def _cases(*kinds):
    return [pytest.param(c, id=c.id) for c in T.CASES if c.kind in kinds]


def _seed(case):
    return sum(ord(ch) * 131 ** i for i, ch in enumerate(case.id)) % (1 << 32)


def _dense(F, seed, ncols, log_n):
    """seeded dense field elements (F.fill), ~2 % of them 0 or p - 1"""
    v = F.fill(seed, ncols << log_n)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, v.size, max(1, v.size // 50))
    v[idx] = np.where(rng.random(idx.size) < 0.5, 0, F.P - 1).astype(F.dtype)
    return v.reshape(ncols, 1 << log_n)


def _rows(rng, log_N, r):
    """the first and the last LDE point, and 64 more, two on each of the 2^r cosets (r <= 5): point i is leaf bitrev(i), whose
    coset is bitrev of i's low r bits"""
    return [0, (1 << log_N) - 1] + [int(rng.integers(0, 1 << (log_N - r))) << r | (k % (1 << r)) for k in range(64)]


def _reference(case):
    """the case's input and what the GPU must return, from the CPU oracle"""
    F, mod, _, _ = FIELD[case.field]
    n, r, P, shift = 1 << case.log_n, case.rate_bits, F.P, T.SHIFT[case.field]
    rng = np.random.default_rng(_seed(case))
    if case.kind == "rate":
        m = _dense(F, _seed(case), case.ncols, case.log_n)
        return dict(input=m, coeffs=m, leaves=T.lde_leaves_ref(mod, shift, m, r))
    if case.kind in ("values", "outer"):
        m = _dense(F, _seed(case), case.ncols, case.log_n)
        coeffs = np.stack([mod.ifft(v) for v in m])
        return dict(input=m, coeffs=coeffs, leaves=T.lde_leaves_ref(mod, shift, coeffs, r))
    if case.kind == "inv_groups":
        m = _dense(F, _seed(case), case.ncols, case.log_n)
        return dict(input=m, cols={c: mod.ifft(m[c]) for c in case.check})
    if case.kind == "sampled":   # one column: the polynomial at shift w_N^i as a dot product with its powers
        m = _dense(F, _seed(case), 1, case.log_n)
        c64, w_N = m[0].astype(np.uint64), F.two_adic_generator(case.log_n + r)
        want = {}
        for i in _rows(rng, case.log_n + r, r):
            x = shift * pow(w_N, i, P) % P
            want[i] = [int(((c64 * mod.powers(x, n).astype(np.uint64)) % np.uint64(P)).sum() % np.uint64(P))]
        return dict(input=m, coeffs=m, rows=want)
    if case.kind == "outer_groups":   # sparse: a_1 x^k1 + a_2 x^k2 + a_3 x^k3 per column, exponents from one shared set of six
        exps = [0, 1 + int(rng.integers(0, 1000)), 4096 + int(rng.integers(0, 1 << 20)), n // 2 + int(rng.integers(0, n // 4)),
                n - 1 - int(rng.integers(0, 1000)), int(rng.integers(1 << 21, n // 2))]
        assert len(set(exps)) == 6
        w_n = F.two_adic_generator(case.log_n)
        seqs = [mod.powers(pow(w_n, k, P), n) for k in exps]      # (w_n^k)^i, i < n
        polys, m = [], np.empty((case.ncols, n), dtype=F.dtype)
        coeffs = np.zeros((case.ncols, n), dtype=F.dtype)
        for c in range(case.ncols):
            poly = {exps[(c + j) % 6]: int(rng.integers(1, P)) for j in range(3)}
            acc = np.zeros(n, dtype=np.uint64)
            for k, a in poly.items():
                acc += mod.scale_vec(seqs[exps.index(k)], a).astype(np.uint64)
                coeffs[c, k] = a
            m[c] = (acc % np.uint64(P)).astype(F.dtype)
            polys.append(poly)
        w_N = F.two_adic_generator(case.log_n + r)
        want = {}
        for i in _rows(rng, case.log_n + r, r):
            x = shift * pow(w_N, i, P) % P
            want[i] = [sum(a * pow(x, k, P) for k, a in poly.items()) % P for poly in polys]
        return dict(input=m, coeffs=coeffs, rows=want)
    raise AssertionError(case.kind)


class _References:
    """reference work of the cases this session runs, started at once on `workers` threads, outer steps (the longest) first"""

    def __init__(self, cases, workers):
        self.pool = ThreadPoolExecutor(workers)
        self.futures = {}
        for c in sorted(cases, key=lambda c: c.kind not in ("outer", "outer_groups")):
            self.futures[c.id] = self.pool.submit(_reference, c)

    def get(self, case):
        f = self.futures.pop(case.id, None) or self.pool.submit(_reference, case)
        return f.result()


@pytest.fixture(scope="module")
def refs(request):
    workers = O.host_cpu_share()
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        workers = max(1, min(workers, int(os.environ["OMP_NUM_THREADS"])))
    B.lib()   # the oracle's ctypes handle and argument types, once, before any worker thread asks for them
    mine = [it.callspec.params["case"] for it in request.session.items
            if getattr(it, "module", None) is not None and it.module.__name__ == __name__ and hasattr(it, "callspec")]
    r = _References(mine, workers)
    yield r
    r.pool.shutdown(wait=True, cancel_futures=True)


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _commit(ctx, case, m, route):
    _, _, tag, view = FIELD[case.field]
    make = PolynomialBatch.from_coeffs if route == "coeffs" else PolynomialBatch.from_values
    if route == "device":
        import torch
        m = torch.from_numpy(np.ascontiguousarray(m).view(view)).cuda()
    elif route == "host_cols":
        m = [np.array(col, copy=True) for col in m]
    return make(ctx, m, case.rate_bits, 4, field=tag)


def _check_coeffs(gpu, case, want, cols=None, route=""):
    for c in (range(case.ncols) if cols is None else cols):
        got = gpu.polynomial(c)
        bad = np.flatnonzero(got != want[c])
        assert bad.size == 0, "%s %s: column %d, %d coefficients differ, first %d" % (case.id, route, c, bad.size, bad[0])


def _check_leaves(gpu, case, want):
    got = gpu.merkle_tree.leaves
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d of %d leaves differ, first %d" % (case.id, bad.size, got.shape[0], bad[0])


def _check_rows(gpu, case, want):
    for i, w in want.items():
        got = [int(v) for v in gpu.get_lde_values(i, 1)]
        assert got == w, (case.id, i, [c for c in range(len(w)) if got[c] != w[c]])


def _done(ctx, gpu, case):
    gpu.free()
    if case.log_n > 21:
        ctx.trim()


@pytest.mark.parametrize("case", _cases("rate", "values", "outer"))
def test_every_coefficient_and_leaf(ctx, refs, case):
    """from_coeffs (the forward pass alone) or from_values: every coefficient, every leaf"""
    ref = refs.get(case)
    gpu = _commit(ctx, case, ref.pop("input"), case.route)
    _check_coeffs(gpu, case, ref["coeffs"])
    _check_leaves(gpu, case, ref["leaves"])
    _done(ctx, gpu, case)


@pytest.mark.parametrize("case", _cases("sampled"))
def test_lde_rate_sampled(ctx, refs, case):
    """2^27 points: every coefficient, 66 get_lde_values rows over all 32 cosets against the polynomial evaluated directly"""
    ref = refs.get(case)
    gpu = _commit(ctx, case, ref.pop("input"), case.route)
    _check_coeffs(gpu, case, ref["coeffs"])
    _check_rows(gpu, case, ref["rows"])
    _done(ctx, gpu, case)


@pytest.mark.parametrize("case", _cases("inv_groups"))
def test_inverse_column_groups(ctx, refs, case):
    """g + 1 columns or more in one transform call: column 0 and the columns on either side of each group boundary against ifft,
    on every route; the routes' caps equal (the same matrix: equal leaves, so every column's coefficients agree)"""
    g = T.intt_group_cols(case.field, case.log_n)
    routes = case.route if isinstance(case.route, tuple) else (case.route,)
    ref = refs.get(case)
    caps = []
    for route in routes:
        if route.startswith("host"):   # an upload chunk wider than g, with a group boundary inside it
            assert any(cc > g and c0 // g != (c0 + cc - 1) // g for c0, cc in T.upload_chunks(case.field, case.ncols)), case.id
        gpu = _commit(ctx, case, ref["input"], route)
        _check_coeffs(gpu, case, ref["cols"], case.check, route)
        caps.append(gpu.merkle_tree.cap)
        _done(ctx, gpu, case)
    for route, cap in zip(routes[1:], caps[1:]):
        assert (cap == caps[0]).all(), "%s: the %s route's cap differs from the %s route's" % (case.id, route, routes[0])


@pytest.mark.parametrize("case", _cases("outer_groups"))
def test_outer_lde_column_groups(ctx, refs, case):
    """9 sparse columns of 2^23 rows on a fresh context: ensure_big_work sizes the outer step's work buffer for 8 columns of this size
    and ensure() only grows it (a larger case before, on the same context, would leave room for all 9), so outer::lde_columns runs
    two work groups.  Every coefficient, and 66 get_lde_values rows over all 2^r cosets - each row holds all 9 columns, the 9th from
    the second group - against the polynomials evaluated directly."""
    ref = refs.get(case)
    ctx.trim()
    fresh = GpuContext(0)
    try:
        gpu = _commit(fresh, case, ref.pop("input"), case.route)
        _check_coeffs(gpu, case, ref["coeffs"])
        _check_rows(gpu, case, ref["rows"])
        gpu.free()
    finally:
        fresh.close()
