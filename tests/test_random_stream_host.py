"""The keyed element stream on the CPU: tests/random_stream.py (the plain-Python restatement) against the known answers - the block
of RFC 8439 2.3.2 and two blocks recorded with `openssl enc -chacha20` (counter 0xffffffff; seed, nonce and counter all ones) - and
csrc/random_stream.hpp built as a host program (tests/host_shim/random_stream.cpp) against the restatement: the blocks, the two
u128 -> field reductions at their carry edges against Python integers, single elements, and ranges that start and end inside
blocks up to the last element the 32-bit block counter reaches; a range past it is refused by the check the ABI uses.  A second
build of the same program under AddressSanitizer and UndefinedBehaviorSanitizer runs the same file: a stand-alone host program,
nothing preloaded.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import random_stream as RS
import random_stream_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
SANITIZE = ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build(path, flags):
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = [CLANG, "-std=c++17", *flags, "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(path), os.path.join(shim, "random_stream.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("random_stream") / "random_stream"
    done = build(exe, ["-O2"])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("random_stream_san") / "random_stream"
    done = build(exe, SANITIZE)
    if done.returncode != 0 and ("asan" in done.stderr or "ubsan" in done.stderr or "sanitizer" in done.stderr.lower()):
        pytest.skip("the sanitizer runtime cannot be linked here: " + done.stderr.strip().splitlines()[-1])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


def run_file(exe, tmp_path, words, want):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    words.tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.uint64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first difference at output word %d: %#x, expected %#x" % (bad[0], got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_the_restatement_reproduces_the_rfc_block():
    seed, nonce, counter, hexed = RS.KATS[0]
    assert (seed, nonce, counter) == (bytes(range(32)), (0x09000000, 0x4a000000, 0), 1)
    assert RS.block(seed, counter, nonce).hex() == hexed and hexed.startswith("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c06803")
    x = 0xc47120a31fdd0f5015593bd1e4e7f110
    assert RS.element(seed, nonce, 4, RS.GL_P) == x % RS.GL_P and RS.element(seed, nonce, 4, RS.BB_P) == x % RS.BB_P
    assert RS.element(seed, nonce, 5, RS.GL_P) == 0x4e6cd4c39aaa2204_0368c033c7f4d1c7 % RS.GL_P


def test_the_restatement_reproduces_the_recorded_openssl_blocks():
    assert RS.KATS[1][2] == 0xFFFFFFFF and RS.KATS[2][0] == b"\xff" * 32 and RS.KATS[2][1] == (0xFFFFFFFF,) * 3
    for seed, nonce, counter, hexed in RS.KATS:
        assert RS.block(seed, counter, nonce).hex() == hexed
        many = RS.blocks(seed, [counter, 0, counter], nonce)       # the numpy lanes elements() uses
        assert many[0].tobytes().hex() == hexed and many[2].tobytes().hex() == hexed
        assert many[1].tobytes() == RS.block(seed, 0, nonce)


def test_ranges_are_position_wise():
    """elements() walks blocks; element() computes one position: the same values, so a range depends on nothing outside it"""
    for p in (RS.GL_P, RS.BB_P):
        whole = RS.elements(RC.SEED, RC.NONCE, 0, 40, p)
        assert [int(v) for v in whole] == [RS.element(RC.SEED, RC.NONCE, e, p) for e in range(40)]
        assert (RS.elements(RC.SEED, RC.NONCE, 5, 30, p) == whole[5:35]).all()
        assert all(int(v) < p for v in whole)


def test_salts_and_blinding_name_their_streams():
    class F:
        P = RS.BB_P
    s = RS.salts(RC.SEED, F, 8)
    assert s.shape == (3, 4, 8) and s.dtype == np.uint32
    assert int(s[2, 3, 5]) == RS.element(RC.SEED, (RS.STREAM_SALTS, 2, 3), 5, RS.BB_P)
    b = RS.blinding(RC.SEED, F, 9)
    assert int(b[8]) == RS.element(RC.SEED, (RS.STREAM_BLINDING, 0, 0), 8, RS.BB_P)


def test_the_edge_list_covers_what_it_should():
    for p in (RS.GL_P, RS.BB_P):
        e = RS.reduction_edges(p)
        for x in (0, p - 1, p, p + 1, 2**64 - 1, 2**64, p * 2**64, p * 2**64 - 1, 2**96 - 1, 2**96, 2**128 - 1, (p - 1) * (2**64 + 1)):
            assert x in e
    e = RS.reduction_edges(RS.BB_P)
    for bound in (2**31, 2**32, 2**62, 2**64):
        k = bound // RS.BB_P
        assert k * RS.BB_P in e and (k + 1) * RS.BB_P in e


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.mark.parametrize("name", sorted(RC.FIELDS))
def test_header_equals_the_restatement(plain, tmp_path, name):
    run_file(plain, tmp_path, *RC.all_records(name))


@pytest.mark.parametrize("name", sorted(RC.FIELDS))
def test_the_same_file_under_the_sanitizers(sanitized, tmp_path, name):
    run_file(sanitized, tmp_path, *RC.all_records(name))


def test_the_last_reachable_range_and_the_first_refused_one():
    assert (2**34 - 6, 6) in RC.RANGES and (2**34 - 6, 7) in RC.REFUSED
    words, want = RC.range_records("goldilocks")
    assert list(want[-len(RC.REFUSED):]) == [0] * len(RC.REFUSED)


def test_a_truncated_file_is_refused(plain, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    RC.all_records("goldilocks")[0][:-1].tofile(src)
    assert subprocess.run([plain, str(src), str(dst)], capture_output=True, text=True, timeout=300).returncode == 3
