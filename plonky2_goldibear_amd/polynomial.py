"""The reference's polynomial transforms on their own, over the C ABI (gb_fft / gb_ifft / gb_lde).

Same names and meaning as field/src/polynomial/mod.rs: PolynomialCoeffs::fft / coset_fft (:264-295, after .lde(rate_bits),
:201-203) and PolynomialValues::ifft / coset_ifft / lde / lde_onto_coset (:57-88).  Everything is in natural order and canonical
words, bit-identical to the reference.

Arrays: one polynomial [n] or a matrix [ncols][n]; with ext=True the last axis holds the D coordinates of an extension element
([n][D] / [ncols][n][D], D = 2 Goldilocks, 4 BabyBear - PolynomialCoeffs<F::Extension>).  A numpy array (host) gives a numpy
array; a torch CUDA tensor of the field's word size (device) gives a tensor on the same device, enqueued on the context's stream
(ctx.synchronize() before another stream reads it).  out=: write there instead - the input itself for a transform in place
(same length only).  `shift` is a canonical base-field element or None.
"""
import ctypes as C

import numpy as np

from . import native as N
from .polynomial_batch import _as_input, _dtype

GENERATOR = {N.GB_GOLDILOCKS: 7, N.GB_BABYBEAR: 31}   # F::generator(): the coset of lde_onto_coset and of every commitment
EXT_DEGREE = {N.GB_GOLDILOCKS: 2, N.GB_BABYBEAR: 4}


def _run(name, ctx, x, rate_bits, shift, field, ext, out, p3_repr):
    if field not in EXT_DEGREE:
        raise N.ShapeError(N.GB_ERR_INVALID, "unknown field tag")
    ptr, shape, flags, keep = _as_input(x, field)
    d = EXT_DEGREE[field] if ext else 1
    lead = len(shape) - (1 if ext else 0)
    if lead not in (1, 2) or (ext and shape[-1] != d):
        raise N.ShapeError(N.GB_ERR_INVALID, "expected [n] or [ncols][n] elements%s" % (" of %d coordinates" % d if ext else ""))
    ncols, n = (1, shape[0]) if lead == 1 else shape[:2]
    log_n = int(n).bit_length() - 1
    if n == 0 or (1 << log_n) != n:
        raise N.ShapeError(N.GB_ERR_INVALID, "polynomial length must be a power of two (util log2_strict)")
    oshape = tuple(shape[:lead - 1]) + (n << rate_bits,) + ((d,) if ext else ())
    if out is None:
        if flags & N.GB_INPUT_DEVICE:
            import torch
            out = torch.empty(oshape, dtype=x.dtype, device=x.device)
        else:
            out = np.empty(oshape, dtype=_dtype(field))
    optr, osh, oflags, okeep = _as_input(out, field)
    if tuple(osh) != oshape or oflags != flags or (oflags == N.GB_INPUT_HOST and okeep is not out):
        raise N.ShapeError(N.GB_ERR_INVALID, "out must be a contiguous %r block of the field's words in the input's memory space" % (oshape,))
    sh = None if shift is None else C.byref((C.c_uint64 if field == N.GB_GOLDILOCKS else C.c_uint32)(int(shift)))
    if shift is not None and not 0 <= int(shift) < (1 << (64 if field == N.GB_GOLDILOCKS else 32)):
        raise N.ShapeError(N.GB_ERR_INVALID, "shift must be a canonical base-field element")
    if p3_repr:
        flags |= N.GB_INPUT_P3_REPR
    fn = getattr(ctx._lib, name)
    args = (ctx.handle, field, ptr, optr, ncols, log_n) + (() if name == "gb_ifft" else (rate_bits,)) + (int(bool(ext)), sh, flags)
    N.check(fn(*args), ctx.handle)
    del keep
    return out


def fft(ctx, coeffs, rate_bits=0, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialCoeffs::lde(rate_bits).fft(): coefficients [..][n] -> values on H_N, N = n << rate_bits"""
    return _run("gb_fft", ctx, coeffs, rate_bits, None, field, ext, out, p3_repr)


def coset_fft(ctx, coeffs, shift, rate_bits=0, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialCoeffs::coset_fft(shift) (after .lde(rate_bits)): values[i] = P(shift * w_N^i)"""
    return _run("gb_fft", ctx, coeffs, rate_bits, shift, field, ext, out, p3_repr)


def ifft(ctx, values, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialValues::ifft: values on H_n -> coefficients"""
    return _run("gb_ifft", ctx, values, 0, None, field, ext, out, p3_repr)


def coset_ifft(ctx, values, shift, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialValues::coset_ifft(shift): values on shift * H_n -> coefficients"""
    return _run("gb_ifft", ctx, values, 0, shift, field, ext, out, p3_repr)


def lde(ctx, values, rate_bits, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialValues::lde(rate_bits): values on H_n -> values on H_N"""
    return _run("gb_lde", ctx, values, rate_bits, None, field, ext, out, p3_repr)


def lde_onto_coset(ctx, values, rate_bits, shift=None, field=N.GB_GOLDILOCKS, ext=False, out=None, p3_repr=False):
    """PolynomialValues::lde_onto_coset(rate_bits): values on H_n -> values on g * H_N (shift: another coset than F::generator()'s)"""
    return _run("gb_lde", ctx, values, rate_bits, GENERATOR[field] if shift is None else shift, field, ext, out, p3_repr)
