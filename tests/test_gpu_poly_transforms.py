"""gb_fft / gb_ifft / gb_lde (plonky2_goldibear_amd.polynomial) against the CPU oracle's transforms, bit for bit, both fields.
Every output element is compared.  Inputs are seeded (splitmix64_fill / oracle_bb.fill); the last column of every input is
structured: a run of p - 1, a run of 0, an all-equal run, then dense values.

Dispatch of the new passes (csrc/kernels_poly.hip), and the cases on either side of each boundary:
  leaf order -> natural order: one workgroup per column up to 2^12 OUTPUT elements, 64 x 64 tiles from 2^13 - log_n 12 | 13 of the
    size cases (rate 0); the rate cases (12, 1) and (12, 3) take the tiles after a 2^12-row transform, (4, 3) the small path;
  coset_ifft's scaling: shift^-i = lo[i % 4096] * hi[i / 4096], the second factor from i = 4096 on - log_n 12 | 13 again.
The transforms underneath are commit()'s (tests/test_gpu_transform_dispatch.py has their branches); what is new here is the order,
the layouts, the scaling and the shift tables.  -m gpu."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, ShapeError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd import polynomial as P

pytestmark = pytest.mark.gpu

ODD = 0x0123456789ABCDEF   # an unstructured shift (reduced mod p)


class Fd:
    def __init__(self, F, mod, tag, gen, idt):
        self.F, self.mod, self.tag, self.gen, self.idt, self.P, self.dt, self.D = F, mod, tag, gen, idt, F.P, F.dtype, F.D
        self.odd = ODD % F.P

    def mul(self, a, b):
        """element-wise product mod p of two canonical arrays"""
        if self.tag == N.GB_BABYBEAR:
            return ((a.astype(np.uint64) * b.astype(np.uint64)) % np.uint64(self.P)).astype(self.dt)
        return np.array([int(x) * int(y) % self.P for x, y in zip(a.tolist(), b.tolist())], dtype=self.dt)

    def fft(self, c, shift=None, zero_factor=0):
        return self.mod.fft(c, zero_factor) if shift is None else self.mod.coset_fft(c, shift, zero_factor)

    def ifft(self, v, shift=None):
        if shift is None:
            return self.mod.ifft(v)
        if self.tag == N.GB_GOLDILOCKS:
            return O.coset_ifft(v, shift)
        # ifft(v)[i] * shift^-i (the same formula equals oracle.coset_ifft over Goldilocks)
        return self.mul(B.ifft(v), B.powers(pow(shift, self.P - 2, self.P), v.size))

    def lde(self, v, rate_bits, shift=None):
        pad = np.zeros(v.size << rate_bits, dtype=self.dt)
        pad[:v.size] = self.mod.ifft(v)
        return self.fft(pad, shift, rate_bits)

    def input(self, seed, ncols, log_n):
        n = 1 << log_n
        m = self.F.fill(seed, ncols * n).reshape(ncols, n).astype(self.dt)
        s, q = m[-1], n // 4
        if n >= 4:
            s[:q], s[q:2 * q], s[2 * q:3 * q] = self.P - 1, 0, s[2 * q]
        else:
            s[:] = [self.P - 1, 0][:n]
        return m

    def device(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a).view(self.idt)).cuda()

    def host(self, t):
        return t.cpu().numpy().view(self.dt)


FIELDS = {"goldilocks": Fd(GL, O, N.GB_GOLDILOCKS, 7, np.int64), "babybear": Fd(BB, B, N.GB_BABYBEAR, 31, np.int32)}
BOTH = pytest.mark.parametrize("fname", sorted(FIELDS))


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


def _rows(f, fn, m, *a):
    return np.stack([fn(v, *a) for v in m])


# ---- sizes: log_n, columns.  2^21, 2^22: the widest native passes; 2^23: the outer radix step
SIZES = [(lg, 3) for lg in (0, 1, 2, 3, 7, 12, 13, 15, 16)] + [(17, 2), (19, 2), (20, 2), (21, 1), (22, 1), (23, 1)]


@BOTH
@pytest.mark.parametrize("log_n,ncols", SIZES, ids=["2^%dx%d" % s for s in SIZES])
def test_fft_and_ifft_at_every_size(ctx, fname, log_n, ncols):
    """fft and ifft without a shift, and with shifts: up to 2^17 rows the generator and the unstructured shift for both directions;
    above, one of the two (by the parity of log_n) to keep the oracle's share of the case at seconds.  coset_ifft is also taken
    back through coset_fft."""
    f = FIELDS[fname]
    m = f.input(1000 + log_n, ncols, log_n)
    shifts = [None] + ([f.gen, f.odd] if log_n <= 17 else [f.odd if log_n & 1 else f.gen])
    for sh in shifts:
        got = P.fft(ctx, m, field=f.tag) if sh is None else P.coset_fft(ctx, m, sh, field=f.tag)
        _eq(got, _rows(f, f.fft, m, sh), "fft shift=%r" % sh)
        got = P.ifft(ctx, m, field=f.tag) if sh is None else P.coset_ifft(ctx, m, sh, field=f.tag)
        _eq(got, _rows(f, f.ifft, m, sh), "ifft shift=%r" % sh)
        if sh is not None:
            _eq(P.coset_fft(ctx, got, sh, field=f.tag), m, "coset_fft(coset_ifft) shift=%r" % sh)


@BOTH
@pytest.mark.parametrize("log_n", [7, 13])
def test_shift_one_is_no_shift(ctx, fname, log_n):
    f = FIELDS[fname]
    m = f.input(1100 + log_n, 3, log_n)
    _eq(P.coset_fft(ctx, m, 1, field=f.tag), P.fft(ctx, m, field=f.tag), "coset_fft(1)")
    _eq(P.coset_ifft(ctx, m, 1, field=f.tag), P.ifft(ctx, m, field=f.tag), "coset_ifft(1)")
    _eq(P.lde_onto_coset(ctx, m, 1, shift=1, field=f.tag), P.lde(ctx, m, 1, field=f.tag), "lde_onto_coset(shift 1)")
    _eq(P.fft(ctx, m, field=f.tag), _rows(f, f.fft, m), "fft")


RATES = [(lg, r) for lg in (0, 4, 12, 13, 16) for r in (1, 3)] + [(20, 2)]


@BOTH
@pytest.mark.parametrize("log_n,rate_bits", RATES, ids=["2^%d-r%d" % s for s in RATES])
def test_rates_fft_and_lde(ctx, fname, log_n, rate_bits):
    """gb_fft with rate_bits against fft / coset_fft of the zero-padded coefficients (zero_factor = rate_bits: the reference's
    zero-tail shortcut, the same result as without it); gb_lde against ifft -> pad -> fft / coset_fft"""
    f = FIELDS[fname]
    ncols = 2 if log_n < 20 else 1
    n = 1 << log_n
    m = f.input(1200 + 8 * log_n + rate_bits, ncols, log_n)
    pad = np.zeros((ncols, n << rate_bits), dtype=f.dt)
    pad[:, :n] = m
    if log_n == 4:
        _eq(_rows(f, f.fft, pad, None, rate_bits), _rows(f, f.fft, pad, None, 0), "the oracle's zero_factor")
    for sh in (None, f.odd if rate_bits == 1 else f.gen):
        got = P.fft(ctx, m, rate_bits, field=f.tag) if sh is None else P.coset_fft(ctx, m, sh, rate_bits, field=f.tag)
        _eq(got, _rows(f, f.fft, pad, sh, rate_bits), "fft rate shift=%r" % sh)
    _eq(P.lde(ctx, m, rate_bits, field=f.tag), _rows(f, f.lde, m, rate_bits), "lde")
    sh = f.gen if rate_bits == 1 else f.odd
    got = P.lde_onto_coset(ctx, m, rate_bits, field=f.tag) if sh == f.gen else P.lde_onto_coset(ctx, m, rate_bits, shift=sh, field=f.tag)
    _eq(got, _rows(f, f.lde, m, rate_bits, sh), "lde_onto_coset shift=%r" % sh)


@BOTH
@pytest.mark.parametrize("log_n", [0, 5, 13, 16])
def test_extension_elements(ctx, fname, log_n):
    """ext = 1: [ncols][n][D] interleaved words.  The transforms are F-linear maps whose matrix entries (twiddles, shift powers,
    n^-1) lie in the base field, and an extension element is sum_k x_k X^k over the base field: so the transform of a vector of
    extension elements is, coordinate by coordinate, the base-field transform of that coordinate's vector."""
    f = FIELDS[fname]
    n, D = 1 << log_n, f.D
    coords = f.input(1300 + log_n, 2 * D, log_n)               # [2 D][n]: column c, coordinate k at row c D + k
    m = np.ascontiguousarray(coords.reshape(2, D, n).transpose(0, 2, 1))   # [2][n][D]

    def ref(fn, *a):
        r = _rows(f, fn, coords, *a)
        return np.ascontiguousarray(r.reshape(2, D, -1).transpose(0, 2, 1))
    for sh in (None, f.odd):
        got = P.fft(ctx, m, field=f.tag, ext=True) if sh is None else P.coset_fft(ctx, m, sh, field=f.tag, ext=True)
        _eq(got, ref(f.fft, sh), "ext fft shift=%r" % sh)
        got = P.ifft(ctx, m, field=f.tag, ext=True) if sh is None else P.coset_ifft(ctx, m, sh, field=f.tag, ext=True)
        _eq(got, ref(f.ifft, sh), "ext ifft shift=%r" % sh)
    _eq(P.lde(ctx, m, 1, field=f.tag, ext=True), ref(f.lde, 1), "ext lde")
    _eq(P.lde_onto_coset(ctx, m, 1, field=f.tag, ext=True), ref(f.lde, 1, f.gen), "ext lde_onto_coset")
    _eq(P.fft(ctx, m[0], field=f.tag, ext=True), ref(f.fft)[0], "ext fft of one [n][D] polynomial")


@BOTH
@pytest.mark.parametrize("log_n", [12, 16])
def test_routes_device_and_in_place(ctx, fname, log_n):
    """the host block is every other test's route; here a device tensor in and out, and out == cols on the device and on the host"""
    f = FIELDS[fname]
    m = f.input(1400 + log_n, 3, log_n)
    want_f, want_i = _rows(f, f.fft, m, f.gen), _rows(f, f.ifft, m, f.odd)
    want_l = _rows(f, f.lde, m, 2, f.gen)
    d = f.device(m)
    out = P.coset_fft(ctx, d, f.gen, field=f.tag)
    lde = P.lde_onto_coset(ctx, d, 2, field=f.tag)
    ctx.synchronize()
    assert out.is_cuda and out.data_ptr() != d.data_ptr()
    _eq(f.host(out), want_f, "device fft")
    _eq(f.host(lde), want_l, "device lde")
    _eq(f.host(d), m, "the device input is left alone")
    assert P.coset_ifft(ctx, d, f.odd, field=f.tag, out=d) is d
    ctx.synchronize()
    _eq(f.host(d), want_i, "device ifft in place")
    d = f.device(m)
    P.coset_fft(ctx, d, f.gen, field=f.tag, out=d)
    ctx.synchronize()
    _eq(f.host(d), want_f, "device fft in place")
    h = m.copy()
    assert P.coset_fft(ctx, h, f.gen, field=f.tag, out=h) is h
    _eq(h, want_f, "host fft in place")
    one = P.fft(ctx, m[1], field=f.tag)
    _eq(one, f.fft(m[1]), "one polynomial [n]")


@BOTH
def test_p3_repr_host_input(ctx, fname):
    """GB_INPUT_P3_REPR: the reference's field types as they lie in memory - p3-goldilocks any u64 representative (x + p where it
    fits), p3-monty-31 the Montgomery word x 2^32 mod p; the output is canonical"""
    f = FIELDS[fname]
    m = f.input(1500, 2, 13)
    if f.tag == N.GB_GOLDILOCKS:
        w = m.copy()
        small = m < np.uint64((1 << 64) - f.P)
        assert small.any()
        w[small] += np.uint64(f.P)
    else:
        w = ((m.astype(np.uint64) << np.uint64(32)) % np.uint64(f.P)).astype(f.dt)
    _eq(P.coset_fft(ctx, w, f.gen, 1, field=f.tag, p3_repr=True), P.coset_fft(ctx, m, f.gen, 1, field=f.tag), "p3 fft")
    _eq(P.ifft(ctx, w, field=f.tag, p3_repr=True), _rows(f, f.ifft, m), "p3 ifft")


@BOTH
def test_errors(ctx, fname):
    f = FIELDS[fname]
    lib, h = ctx._lib, ctx.handle
    m = f.input(1600, 1, 4)
    out = np.zeros(16 << 3, dtype=f.dt)
    ta = f.F.two_adicity
    word = C.c_uint64 if f.tag == N.GB_GOLDILOCKS else C.c_uint32
    p, o = m.ctypes.data, out.ctypes.data
    # log_n + rate_bits above the two-adicity (before anything is read: the blocks are far too small)
    assert lib.gb_fft(h, f.tag, p, o, 1, 4, ta - 3, 0, None, 0) == N.GB_ERR_INVALID
    assert lib.gb_lde(h, f.tag, p, o, 1, ta, 1, 0, None, 0) == N.GB_ERR_INVALID
    assert lib.gb_ifft(h, f.tag, p, o, 1, ta + 1, 0, None, 0) == N.GB_ERR_INVALID
    assert lib.gb_fft(h, f.tag, p, o, 1, 4, 0xFFFFFFFE, 0, None, 0) == N.GB_ERR_INVALID
    for bad in (0, f.P):
        s = word(bad)
        assert lib.gb_fft(h, f.tag, p, o, 1, 4, 0, 0, C.byref(s), 0) == N.GB_ERR_INVALID
        assert lib.gb_ifft(h, f.tag, p, o, 1, 4, 0, C.byref(s), 0) == N.GB_ERR_INVALID
        assert lib.gb_lde(h, f.tag, p, o, 1, 4, 1, 0, C.byref(s), 0) == N.GB_ERR_INVALID
        with pytest.raises(ShapeError):
            P.coset_fft(ctx, m, bad, field=f.tag)
    assert lib.gb_fft(h, 2, p, o, 1, 4, 0, 0, None, 0) == N.GB_ERR_INVALID
    assert b"field" in lib.gb_last_error(h)
    assert lib.gb_fft(h, f.tag, p, o, 1, 4, 0, 2, None, 0) == N.GB_ERR_INVALID            # ext is 0 or 1
    assert lib.gb_fft(h, f.tag, p, o, 1, 4, 0, 0, None, 4) == N.GB_ERR_INVALID            # unknown flag bit
    assert lib.gb_fft(h, f.tag, p, o, 1, 4, 0, 0, None, N.GB_INPUT_DEVICE | N.GB_INPUT_P3_REPR) == N.GB_ERR_INVALID
    assert lib.gb_fft(h, f.tag, None, o, 1, 4, 0, 0, None, 0) == N.GB_ERR_INVALID
    assert lib.gb_fft(h, f.tag, p, None, 1, 4, 0, 0, None, 0) == N.GB_ERR_INVALID
    # ncols = 0: GB_OK, nothing touched (not even looked at: the pointers are null)
    before = out.copy()
    assert lib.gb_fft(h, f.tag, p, o, 0, 4, 3, 0, None, 0) == N.GB_OK
    assert lib.gb_ifft(h, f.tag, None, None, 0, 4, 0, None, 0) == N.GB_OK
    assert lib.gb_lde(h, f.tag, None, None, 0, 4, 1, 1, None, 0) == N.GB_OK
    assert np.array_equal(out, before)
    with pytest.raises(ShapeError):
        P.fft(ctx, np.zeros((2, 12), dtype=f.dt), field=f.tag)    # not a power of two


@BOTH
def test_many_caller_chosen_shifts_on_one_context(ctx, fname):
    """the tables of a shift other than 1 and the generator are built for the call and released with it (the context's cache is
    keyed by the shift and never evicts): two dozen shifts in a row on device tensors, each result checked"""
    f = FIELDS[fname]
    m = f.input(1700, 1, 13)
    d = f.device(m)
    for k in range(24):
        sh = (f.odd + 977 * k) % f.P
        out = P.coset_fft(ctx, d, sh, field=f.tag)
        back = P.coset_ifft(ctx, out, sh, field=f.tag)
        ctx.synchronize()
        _eq(f.host(back), m, "round trip, shift %d" % sh)
        if k % 8 == 0:
            _eq(f.host(out), _rows(f, f.fft, m, sh), "shift %d" % sh)
