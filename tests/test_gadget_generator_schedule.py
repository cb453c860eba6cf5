"""The scheduler (csrc/generator_schedule.hpp) on the records of the gadget generators - a head record and its GB_GEN_TARGETS
continuation records (include/goldibear_gpu.h) - as the stand-alone program of tests/test_generator_schedule.py under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/sanitize/generator_schedule.cpp, its own main: nothing is loaded into
Python): every refusal one by one, random record arrays cut at every length, and the levels, stores and checks of builder
circuits.  CPU only."""
import numpy as np
import pytest

import gadget_cases as GA
import generator_cases as GC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, PartialWitness

NT = 64          # targets of the stub circuit: one wire per row, 64 rows, identity map
HEADS = range(N.GB_GEN_EQUALITY, N.GB_GEN_TARGETS)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return GA.compile_sanitize(tmp_path_factory.mktemp("gadget_schedule") / "generator_schedule")


def stub(records, inputs=(0, 1, 2, 3, 4, 5, 6, 7), ext_degree=2):
    p = 0xFFFFFFFF00000001 if ext_degree == 2 else 2013265921
    return GC.pack(NT, 1, 6, p, ext_degree, np.arange(NT, dtype=np.uint64), [], [(0, 0, 0, 0)], np.zeros((0, NT), dtype=np.uint64),
                   list(records), list(inputs))


def run(exe, tmp_path, cases, num_inputs=8):
    """-> per case a status or a schedule dict, and the program's output"""
    import subprocess
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:] + out.stderr[-4000:])
    got, pos, res = np.fromfile(dst, dtype=np.uint64), 0, []
    for _ in cases:
        s, pos = GC.read_schedule(got, pos, num_inputs, 0)
        res.append(s)
    assert pos == len(got)
    return res, out.stdout


def test_every_kind_is_parsed_into_dependencies_and_outputs(exe, tmp_path):
    R = N.gadget_records
    # targets 0..7 are inputs; everything a record writes lies above them
    recs = (R(N.GB_GEN_EQUALITY, 0, [0, 1, 10, 11]) + R(N.GB_GEN_NONZERO_TEST, 0, [2, 12]) + R(N.GB_GEN_QUOTIENT_OR_ZERO, 0, [3, 4, 13]) +
            R(N.GB_GEN_QUOTIENT_EXTENSION, 0, [0, 1, 2, 3, 14, 15]) + R(N.GB_GEN_SPLIT, 0, [5, 16, 17, 18]) +
            R(N.GB_GEN_WIRE_SPLIT, 7, [6, 19, 20]) + R(N.GB_GEN_LOW_HIGH, 9, [7, 21, 22]) + R(N.GB_GEN_BASE_SUM, 3, [23, 0, 1, 2]) +
            [(N.GB_GEN_COPY, 0, 23, 24)])
    (s,), _ = run(exe, tmp_path, [stub(recs)])
    assert not isinstance(s, int)
    heads = [i for i, r in enumerate(recs) if r[0] != N.GB_GEN_TARGETS]
    want = {N.GB_GEN_EQUALITY: ([0, 1], [10, 11], 0), N.GB_GEN_NONZERO_TEST: ([2], [12], 0), N.GB_GEN_QUOTIENT_OR_ZERO: ([3, 4], [13], 0),
            N.GB_GEN_QUOTIENT_EXTENSION: ([0, 1, 2, 3], [14, 15], 0), N.GB_GEN_SPLIT: ([5], [16, 17, 18], 0),
            N.GB_GEN_WIRE_SPLIT: ([6], [19, 20], 7), N.GB_GEN_LOW_HIGH: ([7], [21, 22], 9), N.GB_GEN_BASE_SUM: ([0, 1, 2], [23], 3),
            N.GB_GEN_COPY: ([23], [24], 0)}
    assert sorted(op["kind"] for op in s["ops"]) == sorted(want)
    reps = s["class_reps"]
    for i, op in enumerate(s["ops"]):
        ins, outs, param = want[op["kind"]]
        assert [reps[c] for c in op["ins"]] == ins and [reps[c] for c in op["outs"]] == outs, op
        assert op["record"] in heads and recs[op["record"]][0] == op["kind"]      # the head's index, continuation records counted
        assert op["p0"] == param, op
        assert GC.level_of_op(s, i) == (2 if op["kind"] == N.GB_GEN_COPY else 1)  # the copy reads the BaseSumGenerator's sum
    assert s["num_levels"] == 2 and s["num_unrunnable"] == 0 and s["num_checks"] == 0


def test_every_malformed_sequence_is_refused_with_its_record_index(exe, tmp_path):
    R, T = N.gadget_records, N.GB_GEN_TARGETS
    good = R(N.GB_GEN_EQUALITY, 0, [0, 1, 10, 11])
    copy = (N.GB_GEN_COPY, 0, 0, 30)
    cases = [
        ([copy] + good, GC.OK, None),
        ([copy, (T, 0, 0, 1)], GC.INVALID, 1),                                              # a continuation with no head
        ([copy] + good + [(T, 0, 0, 1)], GC.INVALID, 4),                                    # .. or one too many behind a generator
        ([copy] + good[:2], GC.INVALID, 1),                                                 # the continuation runs past the end
        ([copy] + good[:1], GC.INVALID, 1),
        ([copy, good[0], good[1], copy], GC.INVALID, 1),                                    # .. or meets another kind
        ([copy, good[0], good[1], good[0]], GC.INVALID, 1),
        ([copy, (N.GB_GEN_EQUALITY, 0, 4, 1)] + good[1:], GC.INVALID, 1),                   # non-zero b in a head
        ([copy, good[0], (T, 1, 0, 1), good[2]], GC.INVALID, 1),                            # non-zero gate in a continuation
        ([copy] + R(N.GB_GEN_NONZERO_TEST, 0, [0, 10])[:1] + [(T, 0, 0, NT)], GC.INVALID, 1),   # a target >= num_targets
        ([copy] + R(N.GB_GEN_NONZERO_TEST, 0, [0, 10])[:1] + [(T, 0, NT, 10)], GC.INVALID, 1),
        ([copy, (N.GB_GEN_LOW_HIGH, 3, 3, 0), (T, 0, 0, 10), (T, 0, 11, 5)], GC.INVALID, 1),    # non-zero padding
        ([copy, (N.GB_GEN_LOW_HIGH, 3, 3, 0), (T, 0, 0, 10), (T, 0, 11, 0)], GC.OK, None),
        ([copy, (N.GB_GEN_SPLIT, 0, 1, 0), (T, 0, NT, 0)], GC.INVALID, 1),                  # the last target of an odd count is checked too
        ([(17, 0, 0, 0)], GC.UNSUPPORTED, 0),                                               # 17 .. 31 stay reserved
        ([(31, 0, 4, 0)] + good[1:], GC.UNSUPPORTED, 0),
        ([(41, 0, 0, 0)], GC.UNSUPPORTED, 0),
    ]
    # a count that does not fit the kind: 4, 2, 3, 3 D; 1..65; >= 2; 3; >= 2
    fits = {N.GB_GEN_EQUALITY: [4], N.GB_GEN_NONZERO_TEST: [2], N.GB_GEN_QUOTIENT_OR_ZERO: [3], N.GB_GEN_QUOTIENT_EXTENSION: [6],
            N.GB_GEN_SPLIT: list(range(1, 66)), N.GB_GEN_WIRE_SPLIT: list(range(2, 70)), N.GB_GEN_LOW_HIGH: [3],
            N.GB_GEN_BASE_SUM: list(range(2, 70))}
    param = {N.GB_GEN_WIRE_SPLIT: 5, N.GB_GEN_LOW_HIGH: 5, N.GB_GEN_BASE_SUM: 2}
    for kind in HEADS:
        for count in (0, 1, 2, 3, 4, 5, 6, 7, 12, 64, 65, 66):
            targets = [0] + list(range(10, 9 + count)) if kind != N.GB_GEN_BASE_SUM else [10] + [0] * (count - 1)
            targets = targets[:count]
            if kind in (N.GB_GEN_EQUALITY, N.GB_GEN_QUOTIENT_OR_ZERO) and count >= 2:
                targets[1] = 1
            if kind == N.GB_GEN_QUOTIENT_EXTENSION and count == 6:
                targets = [0, 1, 2, 3, 10, 11]
            recs = R(kind, param.get(kind, 0), [t % NT for t in targets])
            cases.append(([copy] + recs, GC.OK if count in fits[kind] else GC.INVALID, 1))
    cases.append(([copy] + R(N.GB_GEN_QUOTIENT_EXTENSION, 0, list(range(12))), GC.INVALID, 1))     # 3 D with D = 2 is 6, not 12
    # a parameter out of range
    for kind, bad, ok in ((N.GB_GEN_WIRE_SPLIT, [0], [1, 63, 64, 65, 2**32 - 1]), (N.GB_GEN_LOW_HIGH, [64, 65, 2**32 - 1], [0, 63]),
                          (N.GB_GEN_BASE_SUM, [0, 1], [2, 3, 2**32 - 1]), (N.GB_GEN_EQUALITY, [1], [0]), (N.GB_GEN_NONZERO_TEST, [7], [0]),
                          (N.GB_GEN_QUOTIENT_OR_ZERO, [1], [0]), (N.GB_GEN_QUOTIENT_EXTENSION, [2], [0]), (N.GB_GEN_SPLIT, [1], [0])):
        count = fits[kind][0] if kind not in (N.GB_GEN_SPLIT,) else 3
        targets = [0, 1, 2, 3][:count - 1] + [20] if kind != N.GB_GEN_BASE_SUM else [20, 0]
        if kind == N.GB_GEN_QUOTIENT_EXTENSION:
            targets = [0, 1, 2, 3, 20, 21]
        if kind in (N.GB_GEN_SPLIT, N.GB_GEN_WIRE_SPLIT, N.GB_GEN_LOW_HIGH):
            targets = [0] + list(range(20, 19 + count))
        for v in bad:
            cases.append(([copy] + R(kind, v, targets), GC.INVALID, 1))
        for v in ok:
            cases.append(([copy] + R(kind, v, targets), GC.OK, None))
    res, text = run(exe, tmp_path, [stub(r) for r, _, _ in cases])
    lines = {int(l.split(":")[0].split()[1]): l for l in text.splitlines() if l.startswith("case ")}
    for i, ((recs, want, index), s) in enumerate(zip(cases, res)):
        status = s if isinstance(s, int) else GC.OK
        assert status == want, "case %d %r: status %d, expected %d\n%s" % (i, recs[:4], status, want, lines.get(i))
        if want != GC.OK:
            assert "generator record %d:" % index in lines[i], lines[i]
    # with D = 4 a QuotientGeneratorExtension takes twelve targets
    res, _ = run(exe, tmp_path, [stub(R(N.GB_GEN_QUOTIENT_EXTENSION, 0, list(range(8)) + [20, 21, 22, 23]), ext_degree=4),
                                 stub(R(N.GB_GEN_QUOTIENT_EXTENSION, 0, [0, 1, 2, 3, 20, 21]), ext_degree=4)])
    assert not isinstance(res[0], int) and res[1] == GC.INVALID


def test_random_record_arrays_cut_at_every_length(exe, tmp_path):
    """heads, continuations and gate records mixed at random, valid and not, and every prefix of each array: nothing is read past
    the records that were passed (the harness holds exactly that many, under AddressSanitizer), and whatever is accepted is a
    schedule the kernels can run (schedule_case::sound in the harness: exit status 6 otherwise)"""
    rng = np.random.default_rng(2024)
    R, T = N.gadget_records, N.GB_GEN_TARGETS
    cases = []
    for trial in range(60):
        recs = []
        wrong = trial % 3 == 0      # two arrays in three hold well-formed records only: their prefixes end inside a continuation
        while len(recs) < 24:
            roll = int(rng.integers(0, 16)) if wrong else int(rng.integers(4, 16))
            kind = int(rng.integers(N.GB_GEN_EQUALITY, N.GB_GEN_TARGETS))
            count = {N.GB_GEN_EQUALITY: 4, N.GB_GEN_NONZERO_TEST: 2, N.GB_GEN_QUOTIENT_OR_ZERO: 3, N.GB_GEN_QUOTIENT_EXTENSION: 6,
                     N.GB_GEN_LOW_HIGH: 3}.get(kind, int(rng.integers(2, 9)))
            param = {N.GB_GEN_WIRE_SPLIT: 3, N.GB_GEN_LOW_HIGH: 7, N.GB_GEN_BASE_SUM: 2}.get(kind, 0)
            if roll == 0:
                count = int(rng.integers(0, 9))
            if roll == 1:
                param = int(rng.integers(0, 2**32))
            targets = [int(x) for x in rng.integers(0, NT + (roll == 2), count)]
            if roll < 12:
                g = R(kind, param, targets)
                if roll == 3:
                    g[0] = (kind, param, int(rng.integers(0, 2**40)), 0)      # a count the continuation does not have
                recs += g
            elif roll == 12 and wrong:
                recs.append((T, int(rng.integers(0, 2)), int(rng.integers(0, NT)), int(rng.integers(0, NT))))
            elif roll == 13 and wrong:
                recs.append((int(rng.integers(0, 48)), int(rng.integers(0, 3)), int(rng.integers(0, NT + 2)), int(rng.integers(0, NT + 2))))
            else:
                recs.append((N.GB_GEN_COPY, 0, int(rng.integers(0, NT)), int(rng.integers(0, NT))))
        for cut in range(len(recs) + 1):
            cases.append(stub(recs[:cut]))
    res, _ = run(exe, tmp_path, cases)
    statuses = [s if isinstance(s, int) else GC.OK for s in res]
    assert set(statuses) == {GC.OK, GC.INVALID, GC.UNSUPPORTED}
    assert statuses.count(GC.OK) > 100      # the empty prefixes alone are 60


def _schedule_built(exe, tmp_path, b, pw):
    import subprocess
    built = b.build()
    inputs = GC.built_inputs(built, pw)
    src, dst = tmp_path / "b_in.bin", tmp_path / "b_out.bin"
    GC.write(src, [GC.pack_built(built, inputs)])
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    s, pos = GC.read_schedule(np.fromfile(dst, dtype=np.uint64), 0, len(inputs), len(built.public_inputs))
    assert not isinstance(s, int), out.stdout
    return built, s


def _levels(s, kind):
    return sorted(GC.level_of_op(s, i) for i, op in enumerate(s["ops"]) if op["kind"] == kind)


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_split_low_high_runs_low_high_then_wire_split_then_base_split(exe, tmp_path, field):
    # twelve routed wires: a BaseSumGate of 11 limbs, so range_check(low, 16) takes two rows and range_check(high, 24) three, and
    # their sums are the WireSplitGenerators' to set
    b, pw = CircuitBuilder(GA.config(field, num_routed_wires=12)), PartialWitness()
    x = b.add_virtual_target()
    low, high = b.split_low_high(x, 16, 40 if field == N.GB_GOLDILOCKS else 30)
    pw.set_target(x, 0x2ABCDEF1)
    built, s = _schedule_built(exe, tmp_path, b, pw)
    assert _levels(s, N.GB_GEN_LOW_HIGH) == [1]
    assert _levels(s, N.GB_GEN_WIRE_SPLIT) == [2, 2]          # range_check(low) and range_check(high)
    assert _levels(s, N.GB_GEN_BASE_SPLIT) == [3] * (5 if field == N.GB_GOLDILOCKS else 4)
    assert s["num_unrunnable"] == 0 and s["num_launches"] == 1 and s["num_checks"] > 0      # the limbs past the bits are zero's
    # the LowHighGenerator's record is a head: kind, n_log, three targets
    recs = built.generator_records()
    (lh,) = [op for op in s["ops"] if op["kind"] == N.GB_GEN_LOW_HIGH]
    assert recs[lh["record"]] == (N.GB_GEN_LOW_HIGH, 16, 3, 0) and lh["p0"] == 16
    assert recs[lh["record"] + 1][0] == recs[lh["record"] + 2][0] == N.GB_GEN_TARGETS
    assert recs[lh["record"] + 1][2] == built.target_index(x)
    wsp = [op for op in s["ops"] if op["kind"] == N.GB_GEN_WIRE_SPLIT]
    assert sorted(len(op["outs"]) for op in wsp) == [2, 3 if field == N.GB_GOLDILOCKS else 2] and all(op["p0"] == 11 for op in wsp)
    # with the stock configuration one BaseSumGate row holds all the bits: split_le's accumulator IS that row's sum, so the sum is
    # connected to `low` itself; the BaseSplitGenerator runs beside the WireSplitGenerator, which only compares
    b, pw = CircuitBuilder(GA.config(field)), PartialWitness()
    x = b.add_virtual_target()
    b.split_low_high(x, 5, 20)
    pw.set_target(x, 0xABCDE)
    built, s = _schedule_built(exe, tmp_path, b, pw)
    assert _levels(s, N.GB_GEN_LOW_HIGH) == [1] and _levels(s, N.GB_GEN_WIRE_SPLIT) == [2, 2]
    assert all(op["outs"][0] & GC.OUT_CHECK for op in s["ops"] if op["kind"] == N.GB_GEN_WIRE_SPLIT)
    assert set(_levels(s, N.GB_GEN_BASE_SPLIT)) <= {2, 3} and 2 in _levels(s, N.GB_GEN_BASE_SPLIT)


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_the_base_split_of_a_le_sum_row_checks_the_limbs_connected_to_it(exe, tmp_path, field):
    b, pw = CircuitBuilder(GA.config(field)), PartialWitness()
    x = b.add_virtual_target()
    num_bits = b.config.num_routed_wires // 4 + 2          # past what one ArithmeticGate holds: the BaseSumGate branch
    bits = b.split_le(x, num_bits)
    b.le_sum(bits)
    pw.set_target(x, (1 << num_bits) - 3)
    built, s = _schedule_built(exe, tmp_path, b, pw)
    (bs,) = [i for i, op in enumerate(s["ops"]) if op["kind"] == N.GB_GEN_BASE_SUM]
    split_ops = [(GC.level_of_op(s, i), op) for i, op in enumerate(s["ops"]) if op["kind"] == N.GB_GEN_BASE_SPLIT]
    row_a, row_b = sorted({op["record"] for _, op in split_ops})          # build() lists the gate generators row by row
    a_ops, b_ops = [(l, op) for l, op in split_ops if op["record"] == row_a], [(l, op) for l, op in split_ops if op["record"] == row_b]
    # the row of split_le stores its first num_bits limbs (the others are connected to the constant zero)
    a_level, a_op = min(a_ops, key=lambda lo: lo[0])
    stored = a_op["outs"][:num_bits]
    assert all(w != GC.OUT_SKIP and not w & GC.OUT_CHECK for w in stored)
    # the BaseSumGenerator reads exactly these classes, a level later, and stores the sum
    assert s["ops"][bs]["ins"] == stored and GC.level_of_op(s, bs) == a_level + 1 and not s["ops"][bs]["outs"][0] & GC.OUT_CHECK
    # and the le_sum row's BaseSplitGenerator, one level after the sum, only compares: the connected limbs and the zero ones
    assert all(l > GC.level_of_op(s, bs) for l, _ in b_ops)
    b_words = [w for _, op in b_ops for w in op["outs"] if w != GC.OUT_SKIP]
    assert all(w & GC.OUT_CHECK for w in b_words) and {w & ~GC.OUT_CHECK for w in b_words} >= set(stored)
    assert s["num_checks"] >= len(b_words) >= num_bits and s["num_unrunnable"] == 0
