"""The cases of tests/test_gpu_transform_dispatch.py: one row per commitment, with the transform launch sites it reaches (written as
in csrc/ntt_passes.hpp, lde_passes.hpp, kernels_ntt16.hip, kernels_bb16.hip and ntt_outer.hpp) and why it is there.  tests/test_transform_dispatch_table.py
extracts the launch sites from those sources and fails when one of them is named by no case (or by the allow-list below).

Plain data plus the reference helper both tests use (lde_leaves_ref: the CPU oracle's transforms, no GPU code).

Routes: "host" one host block, "host_cols" separately allocated host columns, "device" a device tensor (one inverse transform over all
columns), "coeffs" from_coeffs from a host block (the forward pass alone).
Kinds:  "rate"         every coefficient and every leaf against the oracle ("sampled": >= 64 get_lde_values rows over every coset,
                       evaluated directly)
        "values"       from_values: every coefficient against ifft, every leaf against coset_fft
        "inv_groups"   ncols > g, the inverse transform's column group (for_intt_groups): column 0 and the columns on either side of
                       every group boundary a transform call crosses (`check`) against ifft; caps equal between the routes
        "outer"        one dense column, N = 2^26: every coefficient and every leaf
        "outer_groups" 9 sparse columns of 2^23 rows: two work groups of outer::lde_columns; every coefficient, sampled rows
"""
from collections import namedtuple

Case = namedtuple("Case", "id field log_n rate_bits ncols route kind sites why check")
Case.__new__.__defaults__ = ((),)   # check: the columns compared against ifft (inv_groups)

GL, BB = "goldilocks", "babybear"
SHIFT = {GL: 7, BB: 31}

# ---- launch sites by size, as written in the sources
_INV = {   # intt_group / intt_columns_r16 (ntt_passes.hpp), both fields
    13: ("k_intt_p1<F>", "k_intt_p3<F>"),
    14: ("k_intt_p1<F>", "k_intt_p3<F>"),
    15: ("k_intt_p1<F>", "k_intt_p3<F>"),
    16: ("k_intt16_p1<F, WB>", "k_intt16_p3<F>"),
    17: ("k_intt16_p1<F, WB>", "k_intt16_p2s<F, 1>", "k_intt16_p3<F>"),
    18: ("k_intt16_p1<F, WB>", "k_intt16_p2s<F, 2>", "k_intt16_p3<F>"),
    19: ("k_intt16_p1<F, WB>", "k_intt16_p2s<F, 3>", "k_intt16_p3<F>"),
    20: ("k_intt16_p1<F, WB>", "k_intt16_p2<F>", "k_intt16_p3<F>"),
    21: ("k_intt16_p1<F, WB>", "k_intt16_p2w<F, 5>", "k_intt16_p3<F>"),
    22: ("k_intt16_p1<F, WB>", "k_intt16_p2w<F, 6>", "k_intt16_p3<F>"),
}
_PA_F = {   # lde_pa_r16 (lde_passes.hpp), both fields; then lde_pb_r16
    13: "k_lde_pa_small<F, 1>", 14: "k_lde_pa_small<F, 2>", 15: "k_lde_pa_small<F, 3>", 16: "k_lde_pa_small<F, 4>",
    17: "k_lde_pa16xs<F, 1>", 18: "k_lde_pa16xs<F, 2>", 19: "k_lde_pa16xs<F, 3>", 20: "k_lde_pa16x2<F>", 21: "k_lde_pa32<F, 1>",
}
_PA = {   # 2^22 rows: lde_pa_rows22, per field (kernels_ntt16.hip / kernels_bb16.hip)
    GL: {**_PA_F, 22: "k_lde_pa32<GlF, 2>"},
    BB: {**_PA_F, 22: "k_bb_lde_pa16x2w"},
}
_PB = {GL: "k_gl_lde_pb16", BB: "k_bb_lde_pb16"}
NATIVE_LOG, OUTER_MAX_BITS = 22, 4   # kernels.hpp: NTT_NATIVE_LOG, NTT_OUTER_MAX_BITS


def lde_sites(field, log_n):
    if log_n > NATIVE_LOG:
        K = min(log_n - NATIVE_LOG, OUTER_MAX_BITS)
        return ("k_deinterleave<F, %d>" % K,) + lde_sites(field, log_n - K) + ("k_lde_combine<F, %d>" % K,)
    return (_PA[field][log_n], _PB[field])


def inv_sites(log_n):
    if log_n > NATIVE_LOG:
        K = min(log_n - NATIVE_LOG, OUTER_MAX_BITS)
        return ("k_deinterleave<F, %d>" % K,) + inv_sites(log_n - K) + ("k_intt_combine<F, %d>" % K,)
    return _INV[log_n]


def values_sites(field, log_n):
    return inv_sites(log_n) + lde_sites(field, log_n)


def intt_group_cols(field, log_n):
    """g of for_intt_groups: INTT_GROUP (16) 8-byte words' worth of columns, halved per doubling above 2^20 rows (from 2^18 rows up)"""
    g0 = 16 if field == GL else 32
    return g0 >> (log_n - 20) if log_n > 20 else g0


def upload_chunks(field, ncols):
    """(c0, columns) of a host batch's upload chunks: api.hip upload_chunk, first chunk 4 (Goldilocks) / 8 (BabyBear) columns"""
    c, out, c0 = (4 if field == GL else 8), [], 0
    while c0 < ncols:
        cc = min(c if c0 < 2 * c else 2 * c if c0 < 4 * c else 16, ncols - c0)
        out.append((c0, cc))
        c0 += cc
    return out


CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


# ---- rates on the strided LDE passes, from_coeffs: rate 0 plus one other rate (not 3, the rate every other test uses) per size
_RATES = {   # log_n: (Goldilocks' other rate, BabyBear's other rate); N <= 2^24
    13: (5, 6), 14: (6, 5), 15: (1, 2), 16: (2, 1), 17: (1, 2), 18: (4, 1), 19: (2, 1), 20: (1, 2), 21: (1, 2), 22: (2, 1),
}
for _lg, (_rg, _rb) in sorted(_RATES.items()):
    for _f, _r in ((GL, _rg), (BB, _rb)):
        _nc0, _nc1 = (3, 1) if _f == GL else (1, 3)
        _add("%s-coeffs-2^%d-r0" % (_f, _lg), _f, _lg, 0, _nc0, "coeffs", "rate", lde_sites(_f, _lg),
             "rate 0: one coset, the coset loops of the strided pass run once")
        _add("%s-coeffs-2^%d-r%d" % (_f, _lg, _r), _f, _lg, _r, _nc1, "coeffs", "rate", lde_sites(_f, _lg),
             "rate %d: %d cosets of pow_lo / pow_hi" % (_r, 1 << _r))
_add("babybear-coeffs-2^22-r5", BB, 22, 5, 1, "coeffs", "sampled", lde_sites(BB, 22),
     "BabyBear's two-adicity edge (2^27 points); k_bb_lde_pa16x2w reads the 2^20-row cosets of rate 7")

# ---- from_values below the outer step: the inverse passes of every size class not reached by the group cases
_add("goldilocks-values-2^13-r1-host", GL, 13, 1, 2, "host", "values", values_sites(GL, 13), "LDS radix-2 inverse passes")
_add("babybear-values-2^15-r2-host_cols", BB, 15, 2, 2, "host_cols", "values", values_sites(BB, 15), "LDS radix-2 inverse passes")
_add("goldilocks-values-2^16-r0-device", GL, 16, 0, 2, "device", "values", values_sites(GL, 16), "radix-16 inverse, no middle pass")
_add("babybear-values-2^16-r1-device", BB, 16, 1, 2, "device", "values", values_sites(BB, 16),
     "canonical-input radix-16 inverse (k_intt16_p1<F, WB> with WB)")
_add("babybear-values-2^17-r0-host", BB, 17, 0, 2, "host", "values", values_sites(BB, 17), "radix-2 middle pass")
_add("goldilocks-values-2^17-r2-host", GL, 17, 2, 2, "host", "values", values_sites(GL, 17), "radix-2 middle pass")
_add("goldilocks-values-2^19-r1-device", GL, 19, 1, 2, "device", "values", values_sites(GL, 19), "radix-8 middle pass")
_add("babybear-values-2^19-r0-host_cols", BB, 19, 0, 2, "host_cols", "values", values_sites(BB, 19), "radix-8 middle pass")

# ---- inverse column groups: g + 1 columns from a device tensor (one transform call over all columns); host input where an upload
# chunk is wider than g
for _f, _lg in ((GL, 18), (GL, 20), (GL, 21), (GL, 22), (BB, 18), (BB, 20), (BB, 21), (BB, 22)):
    _g = intt_group_cols(_f, _lg)
    _add("%s-groups-2^%dx%d-device" % (_f, _lg, _g + 1), _f, _lg, 1, _g + 1, "device", "inv_groups", values_sites(_f, _lg),
         "g = %d: the group loop%s" % (_g, ", bb_intt_columns_canonical over two groups" if _f == BB else ""), check=(0, _g - 1, _g))
_add("goldilocks-groups-2^22x13-host", GL, 22, 0, 13, ("host", "device"), "inv_groups", values_sites(GL, 22),
     "upload chunk of 5 columns at column 8, g = 4: one transform call crosses 11|12; the device route crosses 3|4, 7|8, 11|12",
     check=(0, 11, 12))
_add("babybear-groups-2^22x25-host_cols", BB, 22, 0, 25, ("host_cols", "device"), "inv_groups", values_sites(BB, 22),
     "upload chunk of 9 columns at column 16, g = 8: one transform call crosses 23|24; the device route crosses 7|8, 15|16, 23|24",
     check=(0, 23, 24))

# ---- the outer radix step, one dense column, N = 2^26: every K = 1..4 in both fields (BabyBear's K = 1: the column-group case)
for _f, _lg in ((GL, 23), (GL, 24), (GL, 25), (GL, 26), (BB, 24), (BB, 25), (BB, 26)):
    _add("%s-outer-2^%d-r%d" % (_f, _lg, 26 - _lg), _f, _lg, 26 - _lg, 1, "host", "outer", values_sites(_f, _lg),
         "outer step K = %d around 2^22-row transforms" % (_lg - NATIVE_LOG))
_add("babybear-outer-groups-2^23x9-r3", BB, 23, 3, 9, "device", "outer_groups", values_sites(BB, 23),
     "9 columns, ensure_big_work sized for 8: two work groups of outer::lde_columns (fresh context)")

# ---- launch sites covered elsewhere: element-wise kernels and the single-tile transforms (<= 2^12 rows), with the test that runs them
ALLOWED = {
    "k_ntt_small<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (from_values, 2^0 .. 2^12 rows)",
    "k_lde_pb<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (every leaf, 2^0 .. 2^12 rows, rates 0 .. 8)",
    "k_gather_row<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (MerkleTree.get / get_lde_values rows)",
    "k_transpose_to_rows<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (merkle_tree.leaves)",
    "k_bitrev_copy<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (salted batches)",
    "k_reduce_words<F>": "tests/test_gpu_commit_fuzz.py::test_random_commit_shape (p3_block / p3_cols inputs)",
}


def bit_reversed(x):
    """x[bitrev(j)] for j < x.size (a power of two), as two half-width permutations and a transpose: i = hi 2^b + lo has
    bitrev(i) = bitrev_b(lo) 2^a + bitrev_a(hi)"""
    import numpy as np
    lg = int(x.size).bit_length() - 1
    a, b = lg // 2, lg - lg // 2

    def perm(k):
        i, p = np.arange(1 << k), np.zeros(1 << k, dtype=np.int64)
        for bit in range(k):
            p |= ((i >> bit) & 1) << (k - 1 - bit)
        return p
    return np.ascontiguousarray(x.reshape(1 << a, 1 << b)[perm(a)][:, perm(b)].T).reshape(-1)


def lde_leaves_ref(mod, shift, coeffs, rate_bits):
    """leaves of from_coeffs(coeffs, rate_bits): [N][ncols], leaf j = the LDE point shift * w_N^bitrev(j) - per column the
    bit-reversed coset_fft of the coefficients padded to N.  `mod`: oracle.oracle or oracle.oracle_bb."""
    import numpy as np
    coeffs = np.atleast_2d(coeffs)
    ncols, n = coeffs.shape
    N = n << rate_bits
    out = np.empty((N, ncols), dtype=coeffs.dtype)
    for c in range(ncols):
        pad = np.zeros(N, dtype=coeffs.dtype)
        pad[:n] = coeffs[c]
        out[:, c] = bit_reversed(mod.coset_fft(pad, shift, rate_bits))
    return out
