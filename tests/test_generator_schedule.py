"""The scheduler of gb_circuit_set_generators (csrc/generator_schedule.hpp: classes, levels, statically resolved writers, launch
plan, validation) as a stand-alone C++ program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/sanitize/generator_schedule.cpp, its own main: nothing is loaded into Python).  The schedules it writes back are run by a
small interpreter in Python (tests/generator_cases.py) and compared with the builder mirror's generate_partition_witness; the
levels, launches, stores and checks of hand-made circuits are compared with what the header promises.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import circuits as CS
import generator_cases as GC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GL_P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    out = tmp_path_factory.mktemp("generator_schedule") / "generator_schedule"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "generator_schedule.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return str(out)


def _run(exe, tmp_path, cases):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return np.fromfile(dst, dtype=np.uint64), out.stdout


def _schedule(exe, tmp_path, built, pw, inputs=None, **kw):
    inputs = GC.built_inputs(built, pw) if inputs is None else inputs
    got, _ = _run(exe, tmp_path, [GC.pack_built(built, inputs, **kw)])
    s, pos = GC.read_schedule(got, 0, len(inputs), len(built.public_inputs))
    assert pos == len(got)
    return s, inputs


def _arith_config(**kw):
    return CircuitConfig.standard_recursion_config_gl(**kw)


def _check_against_mirror(built, s, inputs, pw, seed=3):
    built._input_targets = list(inputs)   # what set_generators would keep
    iv = built.input_values(pw, np.random.default_rng(seed))
    got, failed = GC.interpret(s, iv, built.F.p)
    assert not failed
    assert got == GC.mirror_class_values(built, s, pw, np.random.default_rng(seed))
    return got


def test_slots_come_first_and_levels_follow_the_dependencies(exe, tmp_path):
    b, pw = CS.poly_chain_circuit(_arith_config(), 7)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    cells = built.config.num_wires << built.degree_bits
    reps = sorted(set(int(x) for x in built.representative_map[:cells]))
    assert s["class_reps"][:s["num_slots"]] == reps                       # the slots of partition_map.hpp, unchanged
    extra = s["class_reps"][s["num_slots"]:]
    assert extra == sorted(extra) and all(t >= cells for t in extra)       # then what only virtual targets use, ascending
    assert s["num_unrunnable"] == 0
    # y <- y * y + x seven times: seven arithmetic levels behind one another; the constants run in level 1
    arith = [GC.level_of_op(s, i) for i, op in enumerate(s["ops"]) if op["kind"] == N.GB_GEN_ARITHMETIC]
    assert sorted(arith) == list(range(1, 8)) and s["num_levels"] >= 7
    for l in range(s["num_levels"]):                                       # within a level: sorted by kind
        kinds = [op["kind"] for op in s["ops"][s["level_off"][l]:s["level_off"][l + 1]]]
        assert kinds == sorted(kinds)
    _check_against_mirror(built, s, inputs, pw)


def test_a_600_deep_chain_is_one_launch(exe, tmp_path):
    b, pw = CS.poly_chain_circuit(_arith_config(), 600)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    assert s["num_levels"] >= 600 and s["num_launches"] == 1 and s["launches"][0] == (0, s["num_levels"], 1)
    _check_against_mirror(built, s, inputs, pw)


def test_chain_wide_chain_is_three_launches(exe, tmp_path):
    b, pw = GC.wide_between_chains(300)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    widths = [s["level_off"][l + 1] - s["level_off"][l] for l in range(s["num_levels"])]
    assert max(widths) >= 300 and sum(w > GC.GROUP for w in widths) == 1
    assert [l[2] for l in s["launches"]] == [1, 0, 1]
    wide_at = widths.index(max(widths))
    assert s["launches"][1] == (wide_at, 1, 0) and s["launches"][0] == (0, wide_at, 1)
    assert s["launches"][2] == (wide_at + 1, s["num_levels"] - wide_at - 1, 1)
    _check_against_mirror(built, s, inputs, pw)
    # the same circuit under a narrower workgroup: every level that is wider than it becomes a launch of its own
    s2, _ = _schedule(exe, tmp_path, built, pw, group_width=4)
    for first, count, chain in s2["launches"]:
        w = [s2["level_off"][first + k + 1] - s2["level_off"][first + k] for k in range(count)]
        assert all(x <= 4 for x in w) if chain else (count == 1 and w[0] > 4)
    assert _check_against_mirror(built, s2, inputs, pw) is not None


def test_two_writers_are_one_store_and_one_check_a_level_later(exe, tmp_path):
    b, pw, (u, v, t, out) = GC.copy_circuit()
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    t_cls = s["class_reps"].index(built.target_index(t))
    writers = [(GC.level_of_op(s, i), op["outs"][0]) for i, op in enumerate(s["ops"]) if op["kind"] == N.GB_GEN_COPY]
    assert sorted(writers) == [(1, t_cls), (2, t_cls | GC.OUT_CHECK)]      # first in record order stores; the other compares, later
    assert s["num_checks"] == 1
    reader = next(i for i, op in enumerate(s["ops"]) if op["kind"] == N.GB_GEN_ARITHMETIC and t_cls in op["ins"])
    assert GC.level_of_op(s, reader) == 2                                   # one level after the store, not after the check
    _check_against_mirror(built, s, inputs, pw)
    # different values: the check fails (witness.rs:340-350), where the mirror raises
    b, pw, (u, v, t, out) = GC.copy_circuit(second_value=12)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    built._input_targets = list(inputs)
    failed = GC.interpret(s, built.input_values(pw), built.F.p)[1]
    assert [cl for record, cl in failed] == [s["class_reps"].index(built.target_index(t))]
    with pytest.raises(ValueError, match="set twice"):
        built.generate_partition_witness(pw)


def test_a_writer_of_an_input_class_becomes_a_check(exe, tmp_path):
    b = CircuitBuilder(_arith_config())
    u, t = b.add_virtual_target(), b.add_virtual_target()
    b.generate_copy(u, t)
    b.mul(t, t)
    pw = PartialWitness()
    pw.set_target(u, 5)
    pw.set_target(t, 5)          # t is an input AND the copy's destination
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    t_cls = s["class_reps"].index(built.target_index(t))
    (copy,) = [op for op in s["ops"] if op["kind"] == N.GB_GEN_COPY]
    assert copy["outs"] == [t_cls | GC.OUT_CHECK] and s["num_checks"] == 1
    _check_against_mirror(built, s, inputs, pw)


def test_an_unrunnable_generator_is_counted_and_left_out(exe, tmp_path):
    b = CircuitBuilder(_arith_config())
    x, never = b.add_virtual_target(), b.add_virtual_target()
    y = b.mul(x, x)
    z = b.mul(never, y)          # `never` is set by nobody: this generator cannot run, nor can what reads its output
    b.mul(z, z)
    pw = PartialWitness()
    pw.set_target(x, 9)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    assert s["num_unrunnable"] == 2
    assert sum(op["kind"] == N.GB_GEN_ARITHMETIC for op in s["ops"]) == 1
    _check_against_mirror(built, s, inputs, pw)      # their wires stay zero, as in the mirror


def test_two_inputs_of_one_class_and_untouched_inputs(exe, tmp_path):
    b = CircuitBuilder(_arith_config())
    x, y = b.add_virtual_target(), b.add_virtual_target()
    b.connect(x, y)
    b.mul(x, y)
    pw = PartialWitness()
    pw.set_target(x, 4)
    pw.set_target(y, 4)
    built = b.build()
    s, inputs = _schedule(exe, tmp_path, built, pw)
    assert s["input_cls"][0] == s["input_cls"][1] and s["input_first"][:2] == [0, 0]
    # the random wire: nothing reads or writes its class
    rw = inputs.index(wire(*built.random_wire))
    assert s["input_free"][rw] == 1 and s["input_free"][0] == 0
    _check_against_mirror(built, s, inputs, pw)


def test_every_refused_table_is_refused(exe, tmp_path):
    b, pw = CS.poly_chain_circuit(_arith_config(), 3)
    built = b.build()
    inputs = GC.built_inputs(built, pw)
    recs = built.generator_records()
    nt, n = built.num_targets, 1 << built.degree_bits
    arith = next(r for r in recs if r[0] == N.GB_GEN_ARITHMETIC)
    const = next(r for r in recs if r[0] == N.GB_GEN_CONSTANT)
    ngates = len(built.gate_table)
    num_ops = built.gate_table[arith[1]][1]
    program_gates = [(18, 0, 0, 0)]

    def case(records=None, inp=None, **kw):
        tg = [built.target_index(t) for t in inputs] if inp is None else inp
        # (target indices are handed over raw, to reach the ones out of range)
        c = GC.pack(nt, built.config.num_wires, built.degree_bits, built.F.p, built.F.ext_degree, built.representative_map,
                    built.public_input_targets, kw.pop("gates", [(g[0], g[1], g[5], g[6]) for g in built.gate_table]),
                    built.constants_columns, recs if records is None else records, tg, **kw)
        return c

    first = built.target_index(inputs[0])
    cases = [
        (case(), GC.OK),
        (case(records=[(N.GB_GEN_COPY, 0, nt, 0)]), GC.INVALID),                                   # a target >= num_targets
        (case(records=[(N.GB_GEN_COPY, 0, 0, nt)]), GC.INVALID),
        (case(inp=[nt]), GC.INVALID),
        (case(records=[(arith[0], ngates, arith[2], 0)]), GC.INVALID),                             # gate index out of range
        (case(records=[(arith[0], const[1], arith[2], 0)]), GC.INVALID),                           # a gate of another kind
        (case(records=[(N.GB_GEN_POSEIDON, arith[1], arith[2], 0)]), GC.INVALID),
        (case(records=[(arith[0], arith[1], n, 0)]), GC.INVALID),                                  # row
        (case(records=[(arith[0], arith[1], arith[2], num_ops)]), GC.INVALID),                     # operation
        (case(records=[(const[0], const[1], const[2], built.gate_table[const[1]][1])]), GC.INVALID),  # constant index
        (case(inp=[first, first]), GC.INVALID),                                                    # an input listed twice
        (case(records=[(17, 0, 0, 0)]), GC.UNSUPPORTED),                                           # no such kind
        (case(records=[(N.GB_GEN_ARITHMETIC, 0, 0, 0)], gates=program_gates), GC.UNSUPPORTED),     # a program gate's generator
    ]
    got, text = _run(exe, tmp_path, [c for c, _ in cases])
    pos = 0
    for i, (c, want) in enumerate(cases):
        assert int(got[pos]) == want, "case %d: %d\n%s" % (i, int(got[pos]), text)
        if want == GC.OK:
            _, pos = GC.read_schedule(got, pos, len(inputs), len(built.public_inputs))
        else:
            pos += 1
    assert pos == len(got)
    assert "listed twice" in text and "program gates" in text and "row out of range" in text
