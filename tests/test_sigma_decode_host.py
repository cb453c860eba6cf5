"""csrc/sigma_decode.hpp on the CPU (tests/host_shim/sigma_decode.cpp): the coset match and the two-level discrete logarithm that
gb_circuit_decode_sigmas runs per sigma value, over tests/sigma_decode_cases.py - every element of H for lg 1 .. 12, the rows
around the split and seeded rows at lg 13, 20, 27 (and 32 for Goldilocks), every column of 1, 3 and 80 routed wires, the values
that name no cell, k_is that name a coset twice.  Expected cells come from Python integers.  A second build of the same program
under AddressSanitizer and UndefinedBehaviorSanitizer runs the same cases: a stand-alone host program, nothing preloaded."""
import os
import subprocess

import numpy as np
import pytest

import sigma_decode_cases as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
SANITIZE = ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build(path, flags):
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = [CLANG, "-std=c++17", *flags, "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(path), os.path.join(shim, "sigma_decode.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def tables():
    return {name: SD.cases(F) for name, F in SD.FIELDS.items()}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("sigma_decode") / "sigma_decode"
    done = build(exe, ["-O2"])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    exe = tmp_path_factory.mktemp("sigma_decode_san") / "sigma_decode"
    done = build(exe, SANITIZE)
    if done.returncode != 0 and ("asan" in done.stderr or "ubsan" in done.stderr or "sanitizer" in done.stderr.lower()):
        pytest.skip("the sanitizer runtime cannot be linked here: " + done.stderr.strip().splitlines()[-1])
    assert done.returncode == 0, done.stderr[-3000:]
    return str(exe)


def run_cases(exe, tmp_path, F, table):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    SD.pack(F, table).tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    bad = SD.compare(table, np.fromfile(dst, dtype=np.uint64))
    assert not bad, "\n".join(bad[:10])


def test_the_table_covers_what_it_should(tables):
    for name, F in SD.FIELDS.items():
        t = tables[name]
        lgs = {c["lg"] for c in t}
        assert set(range(1, 13)) | {13, 20, 27} <= lgs and (32 in lgs) == (name == "goldilocks")
        assert {len(c["k_is"]) for c in t} >= {1, 3, 80}
        assert sum(want is SD.NO_CELL for c in t for want in c["expected"]) >= 3
        for lg, c in zip(range(1, 13), t):   # all of H
            assert c["lg"] == lg and [cell for cell in c["expected"]] == [(0, r) for r in range(1 << lg)]
    assert any(c["raw"] for c in tables["babybear"])


@pytest.mark.parametrize("name", sorted(SD.FIELDS))
def test_decoded_cells_equal_python(plain, tables, tmp_path, name):
    run_cases(plain, tmp_path, SD.FIELDS[name], tables[name])


@pytest.mark.parametrize("name", sorted(SD.FIELDS))
def test_the_same_cases_under_the_sanitizers(sanitized, tables, tmp_path, name):
    run_cases(sanitized, tmp_path, SD.FIELDS[name], tables[name])


def test_a_truncated_file_is_refused(plain, tables, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    SD.pack(SD.FIELDS["goldilocks"], tables["goldilocks"])[:-3].tofile(src)
    assert subprocess.run([plain, str(src), str(dst)], capture_output=True, text=True, timeout=300).returncode == 3
