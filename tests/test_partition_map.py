"""The slot-map builder of gb_circuit_set_partition (csrc/partition_map.hpp: mark, rank, validate) as a stand-alone C++ program
under AddressSanitizer + UndefinedBehaviorSanitizer (tests/sanitize/partition_map.cpp, its own main: nothing is loaded into
Python), against the numpy restatement in tests/partition_cases.py: identity, one class (K = 1), representatives that are virtual
targets, the class joining cell (0, 0) and cell (n - 1, num_wires - 1), unused virtual targets, a seeded random partition - and
every input the header says is refused.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import partition_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OK, INVALID, UNSUPPORTED = 0, 1, 4
SHAPES = [(4, 3), (32, 33), (64, 135), (128, 167)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    out = tmp_path_factory.mktemp("partition_map") / "partition_map"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "partition_map.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return str(out)


def _case(m, cells, pis=(), want_pi=None, num_targets=None):
    m, pis = np.asarray(m, dtype=np.uint64), np.asarray(pis, dtype=np.uint64)
    head = [len(m) if num_targets is None else num_targets, cells, len(pis), len(pis) if want_pi is None else want_pi, len(m)]
    return np.concatenate([np.array(head, dtype=np.uint64), m, pis])


def _run(exe, tmp_path, cases):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([np.array([len(cases)], dtype=np.uint64)] + cases).tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return np.fromfile(dst, dtype=np.uint64)


def test_accepted_maps_equal_the_restatement(exe, tmp_path):
    cases, wants = [], []
    for n, nw in SHAPES:
        cells = n * nw
        for name, m in PC.maps(n, nw).items():
            rng = np.random.default_rng(cells)
            pis = rng.integers(0, len(m), 3).astype(np.uint64)   # any target may be a public input, virtual ones included
            cases.append(_case(m, cells, pis))
            wants.append((name, n, nw, m, pis))
    got = _run(exe, tmp_path, cases)
    at = 0
    seen_k1 = seen_virtual = seen_unused = False
    for name, n, nw, m, pis in wants:
        cells = n * nw
        reps, slots, shared = PC.slot_map(m, cells)
        assert got[at] == OK, (name, n, nw)
        K = int(got[at + 1])
        at += 2
        assert K == len(reps), (name, n, nw)
        assert np.array_equal(got[at:at + K], reps), (name, n, nw)
        at += K
        assert np.array_equal(got[at:at + cells], slots), (name, n, nw)
        at += cells
        assert np.array_equal(got[at:at + K].astype(bool), shared), (name, n, nw)
        at += K
        assert np.array_equal(got[at:at + len(pis)], m[pis.astype(np.int64)]), (name, n, nw)
        at += len(pis)
        seen_k1 |= K == 1
        seen_virtual |= bool((reps >= cells).any())
        seen_unused |= len(m) > cells and not set(range(cells, len(m))) <= set(reps.tolist())
        if name == "corners_joined_unused_virtuals":
            assert slots[0] == slots[cells - 1] and K == cells - 1 and shared[slots[0]]
    assert at == len(got) and seen_k1 and seen_virtual and seen_unused


def test_every_refused_input_is_refused(exe, tmp_path):
    n, nw = 8, 5
    cells = n * nw
    ident = np.arange(cells + 4, dtype=np.uint64)
    bad_cell, bad_virtual = ident.copy(), ident.copy()
    bad_cell[7] = len(ident)            # a wire cell's entry one past the end
    bad_virtual[cells + 1] = 1 << 40    # an entry of a virtual target no wire uses
    cases = [
        (_case(ident[:cells - 1], cells), INVALID),                           # num_targets < n * num_wires
        (_case(bad_cell, cells), INVALID),
        (_case(bad_virtual, cells), INVALID),
        (_case(ident, cells, [len(ident)]), INVALID),                         # a public-input target >= num_targets
        (_case(ident, cells, [0, 1], want_pi=3), INVALID),                    # a count that differs from cfg.num_public_inputs
        (_case(ident, cells, [], want_pi=1), INVALID),
        (_case(ident, cells, [cells + 3, 0]), OK),
    ]
    got = _run(exe, tmp_path, [c for c, _ in cases])
    at = 0
    for i, (c, want) in enumerate(cases):
        assert got[at] == want, "case %d" % i
        at += 1
        if want == OK:
            K = int(got[at])
            at += 1 + K + cells + K + 2
    assert at == len(got)


def test_two_to_the_32_targets_are_unsupported(exe, tmp_path):
    """num_targets >= 2^32 is GB_ERR_UNSUPPORTED, answered before an entry of the map is read: the case hands over 64 entries and
    claims 2^32 and 2^32 + 5 (a read past them would be the sanitizer's to report)"""
    ident = np.arange(64, dtype=np.uint64)
    got = _run(exe, tmp_path, [_case(ident, 40, num_targets=1 << 32), _case(ident, 40, num_targets=(1 << 32) + 5)])
    assert got.tolist() == [UNSUPPORTED, UNSUPPORTED]
