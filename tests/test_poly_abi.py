"""The stand-alone transform and Merkle-tree entry points (gb_fft / gb_ifft / gb_lde, gb_merkle_tree_*) without a device: they are
exported, bound, and answer GB_ERR_INVALID - not a crash - to null arguments; gb_merkle_tree_free(NULL) is GB_OK.  No GPU needed."""
import ctypes as C

import numpy as np

from plonky2_goldibear_amd import native as N

NAMES = ("gb_fft", "gb_ifft", "gb_lde", "gb_merkle_tree_create", "gb_merkle_tree_free", "gb_merkle_tree_info", "gb_merkle_tree_cap",
         "gb_merkle_tree_leaf", "gb_merkle_tree_digests")


def test_the_nine_entry_points_are_exported_and_bound():
    lib = N.load()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), "missing export: " + name


def test_transforms_reject_null_arguments_without_gpu():
    lib = N.load()
    buf = np.zeros(16, dtype=np.uint64)
    p = buf.ctypes.data
    for field in (N.GB_GOLDILOCKS, N.GB_BABYBEAR):
        # NULL ctx with every other argument in order, then NULL cols / out as well
        for cols, out in ((p, p), (None, p), (p, None), (None, None)):
            assert lib.gb_fft(None, field, cols, out, 1, 4, 0, 0, None, 0) == N.GB_ERR_INVALID
            assert lib.gb_ifft(None, field, cols, out, 1, 4, 0, None, 0) == N.GB_ERR_INVALID
            assert lib.gb_lde(None, field, cols, out, 1, 3, 1, 0, None, 0) == N.GB_ERR_INVALID
    assert b"null" in lib.gb_last_error(None)


def test_merkle_tree_rejects_null_arguments_without_gpu():
    lib = N.load()
    leaves = np.zeros((4, 5), dtype=np.uint64)
    h = C.c_void_p()
    assert lib.gb_merkle_tree_create(None, 0, leaves.ctypes.data, 2, 5, 0, 0, C.byref(h)) == N.GB_ERR_INVALID and not h.value
    assert lib.gb_merkle_tree_create(None, 0, None, 2, 5, 0, 0, C.byref(h)) == N.GB_ERR_INVALID
    assert lib.gb_merkle_tree_create(None, 0, None, 2, 5, 0, 0, None) == N.GB_ERR_INVALID
    assert lib.gb_merkle_tree_free(None) == N.GB_OK
    u = C.c_uint32()
    assert lib.gb_merkle_tree_info(None, C.byref(u), C.byref(u), C.byref(u), C.byref(u)) == N.GB_ERR_INVALID
    out = np.zeros(64, dtype=np.uint64)
    assert lib.gb_merkle_tree_cap(None, out.ctypes.data) == N.GB_ERR_INVALID
    assert lib.gb_merkle_tree_leaf(None, 0, out.ctypes.data, out.ctypes.data, C.byref(u)) == N.GB_ERR_INVALID
    assert lib.gb_merkle_tree_digests(None, out.ctypes.data) == N.GB_ERR_INVALID


def test_python_mirror_exports_the_primitives():
    import plonky2_goldibear_amd as P
    for name in ("fft", "ifft", "coset_fft", "coset_ifft", "lde", "lde_onto_coset"):
        assert callable(getattr(P, name)), name
    assert callable(P.MerkleTree.new)
