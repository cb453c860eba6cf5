"""csrc/constraint_system.hpp - the validator of gb_constraint_quotient / gb_constraint_eval, the code that reads an untrusted program
table - compiled alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/sanitize/constraint_system.cpp, its own main: the
test builds and runs that executable, nothing is loaded into Python): the valid tables of the other constraint tests, every
truncation of them, seeded corruptions, and the degree rule at its boundary.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.constraints import ConstraintProgram, pack_constraint_programs
from test_constraint_programs import grand_product, reads_everything

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
OK, INVALID = 0, 1
FIELDS = [pytest.param(GL, N.GB_GOLDILOCKS, id="goldilocks"), pytest.param(BB, N.GB_BABYBEAR, id="babybear")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    out = tmp_path_factory.mktemp("constraint_system") / "constraint_system"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "constraint_system.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return str(out)


def _case(F, words, offsets, num_programs=None, polys=(4, 4, 4), num_rows=64, num_params=2, max_degree=0, has_polys=True):
    p = list(polys) + [0] * (16 - len(polys))
    head = [F.P, len(polys), int(has_polys)] + p + [num_rows, num_params, max_degree, len(offsets) - 1 if num_programs is None else num_programs]
    return np.array(head + [len(offsets)] + [int(x) for x in offsets] + [len(words)] + [int(x) for x in words], dtype=np.uint64)


def _run(exe, tmp_path, cases):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([np.array([len(cases)], dtype=np.uint64)] + cases).tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr[-4000:])
    return np.fromfile(dst, dtype=np.uint64).reshape(len(cases), 8), out.stderr.splitlines()


@pytest.mark.parametrize("F,tag", FIELDS)
def test_valid_truncated_and_corrupted_tables(exe, tmp_path, F, tag):
    programs = [grand_product(tag), reads_everything(tag)]
    words, offsets = pack_constraint_programs(programs)
    words, offsets = [int(x) for x in words], [int(x) for x in offsets]
    cases = [_case(F, words, offsets), _case(F, words, offsets, has_polys=False)]
    # every truncation: the table ends early and the last offset says so
    cuts = list(range(len(words)))
    for cut in cuts:
        offs = [o for o in offsets if o < cut] + [cut] if cut else [0, 0]     # the programs that are still whole, then the cut one
        cases.append(_case(F, words[:cut], offs))
    rng = np.random.default_rng(11)
    corrupted = 200
    for _ in range(corrupted):
        w = list(words)
        for _ in range(int(rng.integers(1, 4))):
            i = int(rng.integers(0, len(w)))
            w[i] ^= 1 << int(rng.integers(0, 64))
        cases.append(_case(F, w, offsets))
    got, log = _run(exe, tmp_path, cases)
    total_cells, total_cons = sum(p.num_cells for p in programs), sum(p.num_constraints for p in programs)
    for row in got[:2]:
        assert row.tolist() == [OK, total_cells, total_cons, max(p.num_regs for p in programs), 1, sum(p.num_instrs for p in programs),
                                total_cells, sum(p.num_literals for p in programs)]
    for cut, row in zip(cuts, got[2:2 + len(cuts)]):
        whole = cut in offsets and cut > 0     # a cut at a program boundary leaves a valid, shorter system
        assert row[0] == (OK if whole else INVALID), (cut, row, log[2 + cut])
    assert set(got[2 + len(cuts):, 0].tolist()) <= {OK, INVALID}
    assert (got[2 + len(cuts):, 0] == INVALID).sum() > corrupted // 4     # most single-bit flips break an index, a count or a literal


@pytest.mark.parametrize("F,tag", FIELDS)
def test_degree_rule_at_its_boundary_and_the_shape_checks(exe, tmp_path, F, tag):
    def power(k):   # cell^k: degree bound k
        def fn(cell, param, x, l_first, l_last):
            e = cell[0]
            for _ in range(k - 1):
                e = e * cell[0]
            return [e]
        return ConstraintProgram.from_constraints(fn, cells=[(0, 0, 0)], num_params=0, field=tag)
    cases, want = [], []
    for qb in (1, 2, 3, 4):
        for d, st in (((1 << qb) + 1, OK), ((1 << qb) + 2, INVALID)):
            w, o = pack_constraint_programs([power(d)])
            cases.append(_case(F, w, o, polys=(1,), num_params=0, max_degree=(1 << qb) + 1))
            want.append(st)
    # a declared degree above the bound counts, whatever the constraints reach
    hi = ConstraintProgram.from_constraints(lambda c, p, x, lf, ll: [c[0]], cells=[(0, 0, 0)], num_params=0, field=tag, degree=4)
    w, o = pack_constraint_programs([hi])
    cases += [_case(F, w, o, polys=(1,), num_params=0, max_degree=3), _case(F, w, o, polys=(1,), num_params=0, max_degree=5)]
    want += [INVALID, OK]
    # polynomial index at the oracle's count (the salt columns), oracle index at the count, row offset at n, another param count
    one = ConstraintProgram.from_constraints(lambda c, p, x, lf, ll: [c[0] - p[0]], cells=[(1, 3, 63)], num_params=1, field=tag)
    w, o = pack_constraint_programs([one])
    cases += [_case(F, w, o, polys=(1, 4), num_params=1), _case(F, w, o, polys=(1, 3), num_params=1), _case(F, w, o, polys=(9,), num_params=1),
              _case(F, w, o, polys=(1, 4), num_params=1, num_rows=63), _case(F, w, o, polys=(1, 4), num_params=2),
              _case(F, w, o, polys=(1, 3), num_params=1, has_polys=False)]
    want += [OK, INVALID, INVALID, INVALID, INVALID, OK]
    got, log = _run(exe, tmp_path, cases)
    assert got[:, 0].tolist() == want, log
    assert "polynomial_index 3 out of range for oracle 1" in log[len(want) - 5] and "salt columns" in log[len(want) - 5]
    assert "row_offset 63 is not below n = 63" in log[len(want) - 3]
