"""Whole transforms on structured columns: PolynomialBatch.from_values / from_coeffs on inputs built from the carry edges of the limb
arithmetic instead of dense seeded data, at the smallest row count of every arithmetic class of the transform layer
(tests/transform_cases.py's _INV / _PA).  Every coefficient against the oracle's ifft, every leaf against
transform_cases.lde_leaves_ref.  tests/test_gpu_transform_dispatch.py checks dispatch, tables and index math on dense data, where a
Goldilocks edge branch fires with probability ~2^-32 per operation; tests/test_device_register_dfts.py checks the register DFTs one
function at a time.  Here the same edge words go through the passes as they are launched - tables, LDS layouts and all.

The patterns are the COLUMNS of one batch (P = the field's order, n rows, w = two_adic_generator(log_n)):
  0      all P - 1
  1, 2   P - 1, 0, P - 1, 0, ... and its shift by one
  3, 4   P - 1 at index 0 only; at index n - 1 only
  5      P - 1 where i = 0 mod 16, else 0
  6, 7   (P - 1) w^(ik) for k = 1 and k = n / 2 + 1: values of a monomial - the inverse transform's butterflies cancel to exact zeros
         layer after layer and one coefficient survives
  8      the edge values of tests/host_shim/register_dft_cases.hpp repeated with period |E| (also the one column of the "coeffs" route)
  9      fft(column 8) by the oracle: the inverse transform's LAST layer writes the edge words
Routes: "host" everywhere; "device" for BabyBear from 2^16 rows (bb_intt_columns_canonical / k_intt16_p1<BbF, true>, another first
pass); "coeffs" = from_coeffs on column 8.  -m gpu."""
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

# rows -> rate: the smallest size of each class - single tile, LDS radix-2, radix-16 without a middle pass, dft_small<1..3>, the
# radix-16 middle pass, the dft32 middle pass, the radix-64 layers
SIZES = {12: 1, 13: 1, 16: 1, 17: 1, 18: 1, 19: 1, 20: 1, 21: 0, 22: 0}


def edge_values(field):
    """the canonical edge values of tests/host_shim/register_dft_cases.hpp (Gl::edges / Bb::edges), in its order"""
    F = FIELD[field][0]
    P, e = F.P, []
    if field == T.GL:
        e += [0, 1, 2, P - 1, P - 2] + [(1 << 32) + d for d in range(-2, 3)] + [P - (1 << 32) + d for d in range(-2, 3)]
        e += [(1 << 63) + d for d in range(-1, 2)] + [0xFFFFFFFEFFFFFFFF, 0x7FFFFFFF00000000]
        for k in range(64):
            e += [1 << k, (1 << k) - 1, P - (1 << k)]
    else:
        e += [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 27, (1 << 27) - 1, (1 << 27) + 1, P - (1 << 27)]
        rinv = pow(1 << 32, P - 2, P)   # the values whose Montgomery word is 0, 1, p - 1, (p -+ 1) / 2
        e += [w * rinv % P for w in (0, 1, P - 1, (P - 1) // 2, (P + 1) // 2)]
    out = []
    for x in e:
        if 0 <= x < P and x not in out:
            out.append(x)
    return out


def test_edge_values_are_the_case_generators():
    assert len(edge_values(T.GL)) == 200 and len(edge_values(T.BB)) == 15   # |E| as tests/test_register_dfts_host.py requires it


def columns(field, log_n):
    F, mod, _, _ = FIELD[field]
    n, P = 1 << log_n, F.P
    i = np.arange(n)
    w = F.two_adic_generator(log_n)
    tile = np.resize(np.array(edge_values(field), dtype=F.dtype), n)

    def top_where(mask):
        a = np.zeros(n, dtype=F.dtype)
        a[mask] = P - 1
        return a
    cols = [top_where(i >= 0), top_where(i % 2 == 0), top_where(i % 2 == 1), top_where(i == 0), top_where(i == n - 1), top_where(i % 16 == 0)]
    cols += [mod.scale_vec(mod.powers(pow(w, k, P), n), P - 1) for k in (1, n // 2 + 1)]
    cols += [tile, mod.fft(tile)]
    return np.stack([np.asarray(c, dtype=F.dtype) for c in cols])


def _workers():
    workers = O.host_cpu_share()
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        workers = max(1, min(workers, int(os.environ["OMP_NUM_THREADS"])))
    return workers


_latest = {}   # the one (field, log_n) whose routes are running: computed once, shared unchanged


def reference(field, log_n):
    if (field, log_n) not in _latest:
        F, mod, _, _ = FIELD[field]
        r, shift, n = SIZES[log_n], T.SHIFT[field], 1 << log_n
        B.lib()   # the oracle's ctypes handles, once, before any worker thread asks for them
        O.lib()
        m = columns(field, log_n)

        def column(c):   # the oracle's transforms are single-threaded C calls that release the GIL
            coeffs = mod.ifft(m[c])
            return coeffs, T.lde_leaves_ref(mod, shift, coeffs, r)[:, 0]

        with ThreadPoolExecutor(_workers()) as pool:
            tile_leaves = pool.submit(T.lde_leaves_ref, mod, shift, m[8], r)
            done = list(pool.map(column, range(m.shape[0])))
            ref = dict(values=m, coeffs=np.stack([d[0] for d in done]), leaves=np.stack([d[1] for d in done], axis=1),
                       tile_leaves=tile_leaves.result())
        # what the patterns are for, checked on the reference itself: the monomials' one coefficient, the edge words of column 9
        for c, k in ((6, 1), (7, n // 2 + 1)):
            want = np.zeros(n, dtype=F.dtype)
            want[k] = F.P - 1
            assert (ref["coeffs"][c] == want).all()
        assert (ref["coeffs"][9] == m[8]).all()
        for a in ref.values():
            a.setflags(write=False)
        _latest.clear()
        _latest[(field, log_n)] = ref
    return _latest[(field, log_n)]


def _routes(field, log_n):
    return ["host"] + (["device"] if field == T.BB and log_n >= 16 else []) + ["coeffs"]


CASES = [pytest.param(f, lg, route, id="%s-2^%d-r%d-%s" % (f, lg, SIZES[lg], route))
         for f in (T.GL, T.BB) for lg in sorted(SIZES) for route in _routes(f, lg)]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()
    _latest.clear()


def _differ(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d differ, first at %d: got %d, expected %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("field,log_n,route", CASES)
def test_structured_columns_every_coefficient_and_leaf(ctx, field, log_n, route):
    _, _, tag, view = FIELD[field]
    ref, r = reference(field, log_n), SIZES[log_n]
    if route == "coeffs":
        coeffs, leaves = ref["values"][8:9], ref["tile_leaves"]
        gpu = PolynomialBatch.from_coeffs(ctx, np.array(coeffs), r, 4, field=tag)
    else:
        coeffs, leaves = ref["coeffs"], ref["leaves"]
        m = np.array(ref["values"])
        if route == "device":
            import torch
            m = torch.from_numpy(m.view(view)).cuda()
        gpu = PolynomialBatch.from_values(ctx, m, r, 4, field=tag)
    for c in range(coeffs.shape[0]):
        _differ(gpu.polynomial(c), coeffs[c], "%s 2^%d %s: coefficients of column %d" % (field, log_n, route, c))
    got = gpu.merkle_tree.leaves
    assert got.shape == leaves.shape
    for c in range(leaves.shape[1]):
        _differ(got[:, c], leaves[:, c], "%s 2^%d %s: leaves of column %d" % (field, log_n, route, c))
    gpu.free()
    if log_n > 21:
        ctx.trim()
