"""The witness check without a GPU: the three entry points are exported, gb_violation is 48 bytes and the ctypes structures match
the header's field order, Violation.describe formats as documented, and the GB_HD row logic of csrc/witness_check.hpp - the
active-gate test for selector groups of 1, 2 and 7 gates, the first failing constraint, selector violations and the host twin of
the row-list count / scan / fill - agrees with tests/witness_check_cases.py in a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/sanitize/witness_check.cpp; nothing preloaded)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import witness_check_cases as WC
from oracle import gates as G
from plonky2_goldibear_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
C_TYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def header_struct(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goldibear_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    return [(decl.split()[1], C_TYPES[decl.split()[0]]) for decl in (d.strip() for d in body.split(";")) if decl]


def test_entry_points_are_exported_and_bound():
    lib = N.load()
    for name in ("gb_check_witness", "gb_check_partition", "gb_check_inputs"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert lib.gb_check_witness(None, None, 0, None, 0, None, 0, None) == N.GB_ERR_INVALID
    assert lib.gb_check_partition(None, None, 0, None, 0, None) == N.GB_ERR_INVALID
    assert lib.gb_check_inputs(None, None, 0, None, 0, None) == N.GB_ERR_INVALID
    assert b"null" in lib.gb_last_error(None)


def test_structures_match_the_header():
    assert C.sizeof(N.gb_violation) == 48
    assert [(n, t) for n, t in N.gb_violation._fields_] == header_struct("gb_violation")
    assert [(n, t) for n, t in N.gb_check_result._fields_] == header_struct("gb_check_result")
    assert C.sizeof(N.gb_check_result) == 32
    src = open(os.path.join(ROOT, "include", "goldibear_gpu.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(GB_(?:ERR_UNSATISFIED|VIOLATION_[A-Z]+))\s+(\d+)", src)}
    assert consts == {"GB_ERR_UNSATISFIED": N.GB_ERR_UNSATISFIED, "GB_VIOLATION_GATE": N.GB_VIOLATION_GATE,
                      "GB_VIOLATION_SELECTOR": N.GB_VIOLATION_SELECTOR, "GB_VIOLATION_COPY": N.GB_VIOLATION_COPY}
    assert N.Violation.FIELDS == tuple(n for n, _ in N.gb_violation._fields_)


def test_violation_describe_and_the_message_of_an_unsatisfied_error():
    class Built:
        gate_ids = ["NoopGate", "MulAddThreeGate"]

    gate = N.Violation(N.GB_VIOLATION_GATE, gate=1, row=5, index=0, value=1)
    assert gate.describe(Built) == "row 5: MulAddThreeGate, constraint 0 = 1"
    assert gate.describe() == "row 5: gate 1, constraint 0 = 1"
    sel = N.Violation(N.GB_VIOLATION_SELECTOR, row=9, index=0, value=7)
    assert sel.describe(Built) == "row 9: selector column 0 holds 7, which names no gate of its group"
    copy = N.Violation(N.GB_VIOLATION_COPY, row=3, index=2, other_wire=1, other_row=0, value=8, other_value=7)
    assert copy.describe(Built) == "row 3, wire 2 = 8 differs from the first cell of its copy class, row 0, wire 1 = 7"
    # what gb_last_error says after GB_ERR_UNSATISFIED is read back into the first violation
    for v, text in ((gate, "gate violation at row 5: gate 1, constraint 0 = 1"),
                    (sel, "selector violation at row 9: selector column 0 holds 7, which names no gate of its group"),
                    (copy, "copy violation at row 3, wire 2 = 8: the first cell of its class (row 0, wire 1) holds 7")):
        e = N.UnsatisfiedError(N.GB_ERR_UNSATISFIED, "the witness does not satisfy the circuit: ..; the first: " + text)
        assert e.status == 20 and e.violations == [v]
    assert N.UnsatisfiedError(20, "no location").violations == []
    assert gate == N.Violation.from_struct(N.gb_violation(1, 1, 5, 0, 0, 0, 1, 0)) and gate != sel


# ------------------------------------------------------------------------------------------------ the row logic on the host
# selector groups of 1, 2 and 7 gates behind three selector columns, and a group of 2 behind a single one (no UNUSED factor)
THREE_COLUMNS = [(G.ARITHMETIC, 2, 0, 0, 1, 0, 0), (G.CONSTANT, 2, 1, 1, 3, 0, 0), (G.PUBLIC_INPUT, 0, 1, 1, 3, 0, 0),
                 (G.NOOP, 0, 2, 3, 10, 0, 0), (G.ARITHMETIC, 1, 2, 3, 10, 0, 0), (G.BASE_SUM, 3, 2, 3, 10, 2, 0),
                 (G.ADD_MANY, 2, 2, 3, 10, 2, 0), (G.CONSTANT, 1, 2, 3, 10, 0, 0), (G.EXPONENTIATION, 2, 2, 3, 10, 0, 0),
                 (G.ARITHMETIC, 3, 2, 3, 10, 0, 0)]
ONE_COLUMN = [(G.CONSTANT, 2, 0, 0, 2, 0, 0), (G.ARITHMETIC, 2, 0, 0, 2, 0, 0)]
NUM_WIRES, NUM_CONSTANTS, ROWS = 12, 2, 200


def host_case(field, gate_table, num_selectors, seed):
    """selector columns with every kind of value (an index of the group, UNUSED_SELECTOR, indices of other groups, field edges),
    wires that satisfy a row's gate entirely, up to its second constraint, or not at all -> (selectors, constants, wires, pi hash)"""
    F = WC.FIELDS[field]
    rng = np.random.default_rng(seed)
    rnd = lambda *shape: rng.integers(0, F.P, size=shape, dtype=np.uint64)
    sel = np.zeros((num_selectors, ROWS), dtype=np.uint64)
    consts, wires = rnd(NUM_CONSTANTS, ROWS), rnd(NUM_WIRES, ROWS)
    pih = [int(x) for x in rnd(F.hout)]
    for col in range(num_selectors):
        start, end = WC.column_group(gate_table, col)
        choices = list(range(start, end)) * 3 + [G.UNUSED_SELECTOR % F.P, end, (start - 1) % F.P, F.P - 1, 77]
        sel[col] = [choices[i] for i in rng.integers(0, len(choices), size=ROWS)]
    for row in range(ROWS):
        how = row % 3               # 0: satisfied, 1: satisfied but for the last wire of the gate's last operation, 2: random
        for col in range(num_selectors):
            g = WC.active_gate(F, gate_table, num_selectors, col, int(sel[col, row]))
            if how == 2 or g in (WC.NO_GATE, WC.BAD_SELECTOR) or col != num_selectors - 1:
                continue            # (the wires are shared by the columns: the last column's gate is the one they are laid out for)
            kind, param = gate_table[g][0], gate_table[g][1]
            w, k = wires[:, row], [int(c) for c in consts[:, row]]
            if kind == G.CONSTANT:
                w[:param] = consts[:param, row]
            elif kind == G.PUBLIC_INPUT:
                w[:F.hout] = pih
            elif kind == G.ARITHMETIC:
                for i in range(param):
                    w[4 * i + 3] = (int(w[4 * i]) * int(w[4 * i + 1]) * k[0] + int(w[4 * i + 2]) * k[1]) % F.P
            elif kind == G.BASE_SUM:
                w[1:4] = [1, 0, 1]
                w[0] = 5
            elif kind == G.ADD_MANY:
                for i in range(2):
                    w[3 * i + 2] = (int(w[3 * i]) + int(w[3 * i + 1])) % F.P
            elif kind == G.EXPONENTIATION:
                w[1:3] = [1, 0]                                   # power bits, little-endian: exponent 1
                w[4] = 1                                          # intermediate 0: the high bit is 0
                w[5] = w[0]                                       # intermediate 1: 1^2 * base
                w[3] = w[0]                                       # output
            if how == 1 and G.num_constraints(gate_table[g], F.hout, F.D) > 1:
                last = {G.CONSTANT: param - 1, G.PUBLIC_INPUT: F.hout - 1, G.ARITHMETIC: 4 * (param - 1) + 3, G.BASE_SUM: 3, G.ADD_MANY: 5,
                        G.EXPONENTIATION: 3}[kind]
                w[last] = (int(w[last]) + 2) % F.P
    return sel, consts, wires, pih


@pytest.fixture(scope="module")
def witness_check_exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    exe = tmp_path_factory.mktemp("witness_check") / "witness_check"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-include", os.path.join(ROOT, "tests", "host_shim", "shim.h"),
                    "-I", os.path.join(ROOT, "tests", "host_shim"), "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), os.path.join(ROOT, "tests", "sanitize", "witness_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.mark.parametrize("shape", ["three_columns", "one_column"])
@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR], ids=["goldilocks", "babybear"])
def test_row_logic_on_the_host_under_the_sanitizers(witness_check_exe, tmp_path, field, shape):
    F = WC.FIELDS[field]
    gate_table, nsel = (THREE_COLUMNS, 3) if shape == "three_columns" else (ONE_COLUMN, 1)
    sel, consts, wires, pih = host_case(field, gate_table, nsel, seed=7 + field)
    words = [field, ROWS, len(gate_table), nsel, NUM_CONSTANTS, NUM_WIRES] + (pih + [0] * 8)[:8]
    words += [x for g in gate_table for x in g]
    blob = np.concatenate([np.array(words, dtype=np.uint64), sel.reshape(-1), consts.reshape(-1), wires.reshape(-1)])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    blob.tofile(src)
    out = subprocess.run([witness_check_exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.uint64)
    codes = {WC.NO_GATE: 0xFFFFFFFF, WC.BAD_SELECTOR: 0xFFFFFFFE}
    seen = {"satisfied": 0, "first": 0, "later": 0, WC.NO_GATE: 0, WC.BAD_SELECTOR: 0}
    pos = 0
    for row in range(ROWS):
        for col in range(nsel):
            g = WC.active_gate(F, gate_table, nsel, col, int(sel[col, row]))
            want = [codes.get(g, g), 0xFFFFFFFF, 0]
            if g in codes:
                seen[g] += 1
            else:
                f = WC.first_failure(F, gate_table[g], wires[:, row], consts[:, row], pih)
                if f:
                    want[1:] = list(f)
                seen["satisfied" if not f else "first" if f[0] == 0 else "later"] += 1
            assert [int(x) for x in got[pos:pos + 3]] == want, (row, col, g)
            pos += 3
    if nsel == 1:      # a single selector column has no UNUSED factor in its filters: UNUSED_SELECTOR names no gate either
        assert seen.pop(WC.NO_GATE) == 0
    assert all(seen.values()), seen
    cnt, off, rows = WC.row_lists(F, gate_table, nsel, sel)
    assert [int(x) for x in got[pos:]] == cnt + off + rows
    assert cnt[-1] > 0 and sum(c > 0 for c in cnt[:-1]) >= len(gate_table) - 1
