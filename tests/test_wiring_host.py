"""csrc/wiring.hpp on the CPU (tests/host_shim/wiring.cpp): the functions gb_wiring_sigmas' kernels are made of - root finding and
the hook rule, the digit and pass-skipping arithmetic, the successor from sorted runs, the numberings, the sigma value of a
target - probed one by one, and the passes of kernels_wiring.hip emulated over them sequentially on the case families of
tests/wiring_cases.py at 2^2 .. 2^10 rows.  Expected values come from wiring_cases (a plain Python union-find, Python integers).
A second build of the same program under AddressSanitizer and UndefinedBehaviorSanitizer runs the same file: a stand-alone host
program, nothing preloaded."""
import os
import re
import subprocess

import numpy as np
import pytest

import wiring_cases as WC
from oracle.fields import BB, GL
from plonky2_goldibear_amd import wiring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
SANITIZE = ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
FIELDS = {"goldilocks": GL, "babybear": BB}
TILE = wiring.SORT_TILE


def build(path, flags):
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = [CLANG, "-std=c++17", *flags, "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(path), os.path.join(shim, "wiring.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("wiring") / "wiring"
    done = build(exe, ["-O2"])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("wiring_san") / "wiring"
    done = build(exe, SANITIZE)
    if done.returncode != 0 and ("asan" in done.stderr or "ubsan" in done.stderr or "sanitizer" in done.stderr.lower()):
        pytest.skip("the sanitizer runtime cannot be linked here: " + done.stderr.strip().splitlines()[-1])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


# ---- the probes: (op, a, b, c, d) and the expected word, from Python integers
def find_root_by_splitting(a, b, count):
    """the chain parent[t] = t - min(t, b): the root of a, every node passed pointed at its grandparent -> root << 40 | sum"""
    parent = [t - min(t, b) for t in range(count)]
    x = a
    while parent[x] != x:
        p = parent[x]
        if parent[p] == p:
            x = p
            break
        parent[x] = min(parent[x], parent[p])
        x = p
    return x << 40 | sum(parent)


def probes():
    out = []
    for limit in [0, 1, 2, 3, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 32) - 1, 1 << 32]:
        bits = max(limit - 1, 0).bit_length()
        out += [((0, limit, 0, 0, 0), bits), ((1, limit, 0, 0, 0), (bits + 7) // 8)]
    for key in [0, 1, 255, 256, 0x01020304, 0xFFFFFFFF, 0x80000000, 65535, 65536]:
        out += [((2, key, ps, 0, 0), (key >> (8 * ps)) & 255) for ps in range(4)]
    # successor_index(i, m, next has the same label, run length)
    for i, m, same, run, want in [(0, 2, 1, 2, 1), (1, 2, 0, 2, 0), (4, 9, 1, 3, 5), (5, 9, 0, 3, 3), (8, 9, 0, 9, 0), (8, 9, 1, 2, 7),
                                  (7, 9, 0, 2, 6), (1023, 2048, 1, 4, 1024), (1024, 2048, 0, 4, 1021), (3, 9, 0, 7, 3)]:
        out.append(((3, i, m, same, run), want))
    for a, b in [(1, 2), (2, 1), (0, 0xFFFFFFFF), (7, 7), (1 << 31, (1 << 31) - 1)]:
        out.append(((4, a, b, 0, 0), max(a, b) << 32 | min(a, b)))
    # check_pair over 4 rows of 9 wires, 5 routed: cells = 36
    shape = 9 << 32 | 5
    for a, b, nt, want in [(0, 35, 36, 2), (0, 31, 36, 0), (36, 0, 36, 1), (36, 0, 37, 0), (5, 0, 40, 2), (4, 39, 40, 0), (0, 40, 40, 1),
                           (8, 40, 40, 1), (1 << 40, 0, 40, 1), (13, 13, 36, 0), (14, 14, 36, 2), (36, 38, 39, 0)]:
        out.append(((5, a, b, nt, shape), want))
    for lg, nw in [(2, 9), (10, 135), (16, 1), (0, 3)]:
        n = 1 << lg
        for cell in sorted({0, nw - 1, nw % (n * nw), n * nw - 1, (n // 2) * nw + nw // 2}):
            idx = (cell % nw) * n + cell // nw
            out += [((6, cell, lg, nw, 0), idx), ((7, idx, lg, nw, 0), cell)]
    for j, nr, nw in [(0, 5, 9), (4, 5, 9), (5, 5, 9), (79, 80, 135), (80, 80, 135), (12345, 80, 135), (7, 1, 1), (7, 1, 2)]:
        out.append(((8, j, nr, nw, 0), (j // nr) * nw + j % nr))
    for a, b, count in [(0, 1, 1), (9, 1, 10), (999, 1, 1000), (999, 3, 1000), (5, 0, 10), (1000, 7, 5000)]:
        out.append(((9, a, b, count, 0), find_root_by_splitting(a, b, count)))
    return out


def emulated_cases():
    out = []
    for lg in (2, 3, 5, 10):
        out += WC.families(lg, WC.SMALL, TILE)
    out.append(WC.Case("one_wire", 10, (1, 1), WC.path(np.arange(0, 1024, 3)), 1))
    out.append(WC.Case("standard_width", 4, WC.STANDARD, WC.random_classes(4, WC.STANDARD, 11), 5))
    return out


def run_file(exe, tmp_path, F, cases):
    table = probes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    WC.pack(F, [q for q, _ in table], cases).tofile(src)
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, (done.returncode, done.stdout[-3000:] + done.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.uint64)
    bad = ["probe %r: got %d, expected %d" % (q, int(g), want) for (q, want), g in zip(table, got[:len(table)]) if int(g) != want]
    assert not bad, "\n".join(bad[:10])
    pos = len(table)
    for case in cases:
        rep, _, _, info = WC.structure(case)
        routed = case.n * case.num_routed
        assert got[pos:pos + 2].tolist() == [0, 0], case
        passes, moved, classes, largest, merged = (int(v) for v in got[pos + 2:pos + 7])
        assert passes >= 1, case
        assert dict(routed_cells=routed, moved_cells=moved, num_classes=classes, largest_class=largest, merged_targets=merged) == info, case
        pos += 7
        assert np.array_equal(got[pos:pos + case.num_targets], rep), case
        pos += case.num_targets
        assert np.array_equal(got[pos:pos + routed], WC.sigmas(case, F).ravel().astype(np.uint64)), case
        pos += routed
    assert pos == got.size


def test_the_cases_cover_what_they_should():
    names = {c.name for c in emulated_cases()}
    assert {"no_pairs", "self_pair", "all_star_highest", "all_path_shuffled", "awkward_pair", "sizes_around_wave_and_tile",
            "straddles_a_tile_boundary", "virtual_chain_of_three", "virtual_only_class", "exactly_the_wire_targets"} <= names
    case = next(c for c in emulated_cases() if c.name == "sizes_around_wave_and_tile")
    _, moved_from, _, info = WC.structure(case)
    assert info["largest_class"] == TILE + 1 and info["num_classes"] == 6 and moved_from.size == 63 + 64 + 65 + 3 * TILE
    case = next(c for c in emulated_cases() if c.name == "all_path_descending" and c.degree_bits == 5)
    rep, _, _, info = WC.structure(case)
    assert info["largest_class"] == info["moved_cells"] == 32 * 5 and rep[8 * 9 + 4] == 0 and rep[8 * 9 + 5] == 8 * 9 + 5


def test_the_python_tile_constant_is_the_kernels():
    text = open(os.path.join(ROOT, "plonky2_goldibear_amd", "csrc", "wiring.hpp")).read()
    assert int(re.search(r"constexpr u32 SORT_TILE = (\d+);", text).group(1)) == TILE


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_probes_and_emulated_passes_equal_python(plain, tmp_path, name):
    run_file(plain, tmp_path, FIELDS[name], emulated_cases())


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_the_same_file_under_the_sanitizers(sanitized, tmp_path, name):
    run_file(sanitized, tmp_path, FIELDS[name], emulated_cases())


def test_bad_pairs_are_named_by_their_lowest_index(plain, tmp_path):
    cells = 4 * 9
    cases = [WC.Case("range", 2, WC.SMALL, [(0, 1), (1, cells + 3), (2, 3), (cells + 9, 0)], 3),
             WC.Case("routable", 2, WC.SMALL, [(0, 1), (9 + 5, 0), (1, 8)], 3),
             WC.Case("both", 2, WC.SMALL, [(5, 0), (0, cells + 3)], 3)]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    WC.pack(GL, [], cases).tofile(src)
    assert subprocess.run([plain, str(src), str(dst)], capture_output=True, text=True, timeout=300).returncode == 0
    assert np.fromfile(dst, dtype=np.uint64).tolist() == [1, 1, 2, 1, 1, 1]


def test_a_truncated_file_is_refused(plain, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    WC.pack(GL, [q for q, _ in probes()], emulated_cases()[:3])[:-3].tofile(src)
    assert subprocess.run([plain, str(src), str(dst)], capture_output=True, text=True, timeout=300).returncode == 3
