"""The case table of tests/test_gpu_transform_dispatch.py against the sources: every transform launch site of ntt_passes.hpp,
lde_passes.hpp, kernels_ntt16.hip, kernels_bb16.hip and ntt_outer.hpp (hipLaunchKernelGGL's kernel with its literal template arguments, GB_PAS(KK)
expanded by its call sites) is named by a case of tests/transform_cases.py or sits in its allow-list - a new launch site without a
case fails here.  And the GPU test's reference helper (leaves = bit-reversed coset_fft of the padded coefficients) against the
oracle's own PolynomialBatch.from_coeffs, so that the large comparisons rest on a layout that has itself been checked.  CPU only."""
import os
import re

import numpy as np
import pytest

import transform_cases as T
from oracle.fields import BB, GL

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plonky2_goldibear_amd", "csrc")
SOURCES = ("ntt_passes.hpp", "lde_passes.hpp", "kernels_ntt16.hip", "kernels_bb16.hip", "ntt_outer.hpp")


def _kernel_arg(text, i):
    """the first argument of the call whose '(' is at text[i - 1]: a kernel name with its template arguments, maybe parenthesised"""
    while text[i].isspace():
        i += 1
    if text[i] == "(":
        depth, j = 0, i
        while True:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            if depth == 0:
                return text[i + 1:j]
            j += 1
    depth, j = 0, i
    while depth or text[j] not in ",)":
        depth += {"<": 1, ">": -1}.get(text[j], 0)
        j += 1
    return text[i:j]


def _normalise(site):
    return re.sub(r"\s+", "", site).replace(",", ", ")


def launch_sites(text):
    """hipLaunchKernelGGL kernels of one source, function-like macros expanded by their call sites"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    sites = set()
    macro = re.compile(r"#define\s+(\w+)\((\w+)\)((?:[^\n]*\\\n)*[^\n]*)")
    for m in list(macro.finditer(text)):
        name, param, body = m.groups()
        if "hipLaunchKernelGGL" not in body:
            continue
        rest = text[:m.start()] + text[m.end():]
        calls = re.findall(r"\b%s\(([^()]*)\)" % name, rest)
        assert calls, "macro %s launches a kernel but is never called" % name
        for k in body.split("hipLaunchKernelGGL(")[1:]:
            for arg in calls:
                sites.add(_normalise(re.sub(r"\b%s\b" % param, arg.strip(), _kernel_arg(k, 0))))
    text = macro.sub("", text)
    for m in re.finditer(r"\bhipLaunchKernelGGL\(", text):
        sites.add(_normalise(_kernel_arg(text, m.end())))
    return sites


def source_sites():
    out = {}
    for f in SOURCES:
        with open(os.path.join(CSRC, f)) as fh:
            for s in launch_sites(fh.read()):
                out.setdefault(s, []).append(f)
    return out


def _field_of(site):
    """the field a launch site runs in: k_gl_* / k_bb_* and the templates written with GlF / BbF one, the templates over F both"""
    args = re.findall(r"\b(GlF|BbF)\b", site)
    if site.startswith("k_gl_") or "GlF" in args:
        return {T.GL}
    if site.startswith("k_bb_") or "BbF" in args:
        return {T.BB}
    return {T.GL, T.BB}


def test_every_launch_site_has_a_case():
    """every launch site is named by a case in each field it runs in (GlF and BbF instantiations are different code), or allow-listed"""
    src = source_sites()
    named = {(s, c.field) for c in T.CASES for s in c.sites}
    missing = sorted("%s (%s)" % (s, f) for s in src if s not in T.ALLOWED for f in sorted(_field_of(s)) if (s, f) not in named)
    assert not missing, "launch sites without a case in tests/transform_cases.py: %s" % missing
    wrong = sorted("%s: %s" % (c.id, s) for c in T.CASES for s in c.sites if c.field not in _field_of(s))
    assert not wrong, "cases that name another field's kernels: %s" % wrong
    named = {s for s, _ in named}
    stale = sorted(s for s in named | set(T.ALLOWED) if s not in src)
    assert not stale, "names in tests/transform_cases.py that are no launch site of %s: %s" % (", ".join(SOURCES), stale)
    assert not named & set(T.ALLOWED), "allow-listed sites are for what no case reaches"


def test_extraction_finds_the_known_shapes():
    """the extractor itself: GB_PAS expanded for 2^17 .. 2^19 rows, the outer step's launch switches for K = 1 .. 4, the field of a
    site that names one in its template arguments"""
    src = source_sites()
    for kk in (1, 2, 3):
        assert "k_lde_pa16xs<F, %d>" % kk in src
    for k in ("k_deinterleave", "k_intt_combine", "k_lde_combine"):
        for K in range(1, T.OUTER_MAX_BITS + 1):
            assert "%s<F, %d>" % (k, K) in src
    assert "k_intt16_p1<F, WB>" in src and "k_bb_lde_pa16x2w" in src
    assert _field_of("k_lde_pa32<GlF, 2>") == {T.GL} and _field_of("k_lde_pa32<F, 1>") == {T.GL, T.BB}
    assert _field_of("k_bb_lde_pa16x2w") == {T.BB} and "k_lde_pa32<GlF, 2>" in src
    assert len(src) == len(set(src))
    assert not [s for s in src if "KK" in s or "hipLaunch" in s]


def test_case_table_shape():
    """what the issue of this table asks of it, so that a later edit cannot thin it out unnoticed"""
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    for f in (T.GL, T.BB):
        rates = [c for c in T.CASES if c.field == f and c.kind in ("rate", "sampled")]
        for lg in range(13, 23):
            here = {c.rate_bits for c in rates if c.log_n == lg}
            assert 0 in here and here - {0, 3}, (f, lg, here)
            assert all(c.route == "coeffs" and (c.log_n + c.rate_bits <= 24 or c.kind == "sampled") for c in rates)
        assert {c.ncols for c in rates} == {1, 3}
        outer = [c for c in T.CASES if c.field == f and c.kind == "outer"]
        assert len(outer) >= 2 and all(c.log_n + c.rate_bits == 26 and c.ncols == 1 for c in outer)
    assert {0, 1, 5} <= {c.rate_bits for c in T.CASES if c.field == T.BB and c.log_n == 22 and c.kind in ("rate", "sampled")}
    assert {c.log_n - 22 for c in T.CASES if c.kind == "outer"} == {1, 2, 3, 4}
    for c in T.CASES:
        if c.kind == "inv_groups":
            g = T.intt_group_cols(c.field, c.log_n)
            assert c.log_n >= 18 and c.ncols > g and 0 in c.check, c.id
            assert all(b in c.check and b - 1 in c.check for b in range(g, c.ncols, g) if not isinstance(c.route, tuple)), c.id
    for f, lg, g in ((T.GL, 18, 16), (T.GL, 20, 16), (T.GL, 21, 8), (T.GL, 22, 4), (T.BB, 18, 32), (T.BB, 20, 32), (T.BB, 21, 16),
                     (T.BB, 22, 8)):
        assert T.intt_group_cols(f, lg) == g
        assert any(c.kind == "inv_groups" and c.field == f and c.log_n == lg and c.ncols == g + 1 and c.route == "device"
                   for c in T.CASES), (f, lg)
    assert T.upload_chunks(T.GL, 13) == [(0, 4), (4, 4), (8, 5)] and T.upload_chunks(T.BB, 25) == [(0, 8), (8, 8), (16, 9)]
    for f in (T.GL, T.BB):   # the host route where an upload chunk is wider than g, and the device route on the same matrix
        g = T.intt_group_cols(f, 22)
        assert any(c.kind == "inv_groups" and c.field == f and c.log_n == 22 and isinstance(c.route, tuple) and "device" in c.route
                   and any(cc > g for _, cc in T.upload_chunks(f, c.ncols)) for c in T.CASES), f
    og = [c for c in T.CASES if c.kind == "outer_groups"]
    assert og and all(c.log_n == 23 and c.ncols == 9 and c.rate_bits == 3 and c.route == "device" for c in og)


@pytest.mark.parametrize("F", [GL, BB], ids=lambda F: F.name)
def test_reference_leaves_equal_oracle_batch(F):
    """lde_leaves_ref(coeffs, rate) == oracle PolynomialBatch.from_coeffs(coeffs, rate).leaves, 2^0 .. 2^10 rows, rates 0 .. 4; and
    get_lde_values(i, 1) is the polynomial at shift * w_N^i (what the sampled GPU checks evaluate)"""
    shift = T.SHIFT[F.name]
    for lg in range(0, 11):
        for r in range(0, 5):
            coeffs = F.fill(1000 * lg + r, 2 << lg).reshape(2, 1 << lg)
            coeffs[1, 0], coeffs[0, -1] = 0, F.P - 1
            cpu = F.mod.PolynomialBatch.from_coeffs(coeffs, r, 0)
            assert (T.lde_leaves_ref(F.mod, shift, coeffs, r) == cpu.leaves).all(), (lg, r)
            Nn = 1 << (lg + r)
            w_N = F.two_adic_generator(lg + r)
            for i in {0, 1, Nn - 1, Nn // 3}:
                x = shift * pow(w_N, i, F.P) % F.P
                want = [sum(int(a) * pow(x, k, F.P) for k, a in enumerate(col)) % F.P for col in coeffs]
                assert [int(v) for v in cpu.get_lde_values(i, 1)] == want, (lg, r, i)
