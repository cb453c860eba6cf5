"""Copy constraints -> sigma columns and representative map on the device (include/goldibear_gpu.h: gb_wiring_sigmas).

"generate sigma polynomials" of CircuitBuilder::build (plonk/circuit_builder.rs:1005-1040, plonk/permutation_argument.rs): the
classes of the targets under the pairs, the lowest target index of every class as its representative, and the sigma columns in
which the routed wire cells of a class, in ascending row * num_wires + column order, each name the next.  Target indices are
Target::index: wire (row, column) is row * num_wires + column, virtual target i is degree * num_wires + i.
"""
import collections
import ctypes as C

import numpy as np

from . import native as N
from .polynomial_batch import _dtype

# the entries one workgroup of the stable radix sort ranks (csrc/wiring.hpp: SORT_TILE) - also the tile of the compaction that
# precedes it.  Tests place classes around its multiples.
SORT_TILE = 1024

WiringInfo = collections.namedtuple("WiringInfo", [name for name, _ in N.gb_wiring_info._fields_ if name != "reserved"])
WiringInfo.__doc__ = "gb_wiring_info: what sigma_polys made (rounds is a diagnostic that depends on the device's schedule)"


def sigma_polys(ctx, field, degree_bits, num_wires, num_routed_wires, k_is, copy_constraints, num_targets, device=False):
    """-> (sigmas [num_routed_wires][2^degree_bits] canonical values on H, representative_map [num_targets] u64, WiringInfo).
    copy_constraints: [num_copies][2] target indices.  device=True: the sigmas are a torch tensor on the context's device (the
    field's words as int64 / int32), written on the context's stream - what the column pointers of a device circuit may name."""
    if field not in (N.GB_GOLDILOCKS, N.GB_BABYBEAR):
        raise N.ShapeError(N.GB_ERR_INVALID, "unknown field tag")
    dt = _dtype(field)
    k = np.ascontiguousarray(k_is, dtype=dt)
    if k.shape != (num_routed_wires,):
        raise N.ShapeError(N.GB_ERR_INVALID, "k_is must have num_routed_wires entries")
    pairs = np.ascontiguousarray(copy_constraints, dtype=np.uint64).reshape(-1, 2)
    n = 1 << degree_bits
    if device:
        import torch
        sig = torch.empty((num_routed_wires, n), dtype=torch.int64 if dt == np.uint64 else torch.int32, device="cuda:%d" % ctx.device)
        sptr, flags = sig.data_ptr(), N.GB_INPUT_DEVICE
    else:
        sig = np.empty((num_routed_wires, n), dtype=dt)
        sptr, flags = sig.ctypes.data, N.GB_INPUT_HOST
    rep = np.empty(int(num_targets) if 0 <= int(num_targets) < 1 << 32 else 0, dtype=np.uint64)
    info = N.gb_wiring_info()
    N.check(ctx._lib.gb_wiring_sigmas(ctx.handle, field, degree_bits, num_wires, num_routed_wires, k.ctypes.data,
                                      pairs.ctypes.data_as(C.POINTER(C.c_uint64)), len(pairs), int(num_targets), flags, sptr,
                                      rep.ctypes.data_as(C.POINTER(C.c_uint64)), C.cast(C.pointer(info), C.c_void_p)), ctx.handle)
    return sig, rep, WiringInfo(*[int(getattr(info, name)) for name in WiringInfo._fields])
