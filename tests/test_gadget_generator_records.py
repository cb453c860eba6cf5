"""The evaluators of the gadget generators (csrc/generators.hpp: gen_equality .. gen_base_sum, record kinds 32..39) on the HOST,
through tests/host_shim/generators.cpp as tests/test_generator_records.py runs the gate generators: scheduled by
csrc/generator_schedule.hpp, run op by op, compared with the builder mirror's generator classes at every class.  Every
comparison is exact.

  * every kind at every shape and edge operand of tests/gadget_cases.py, both fields, as independent records;
  * the reference's panics - a zero denominator, a limb that is no bool, a value past its bits - end in the error word, with
    the head record's index and the offending class, where the mirror asserts;
  * circuits built with the gadgets of circuit_builder.py (is_equal, split_le, le_sum, split_low_high, div_extension, select).
CPU only."""
import numpy as np
import pytest

import gadget_cases as GA
import generator_cases as GC
import gate_variants as GV
from plonky2_goldibear_amd import native as N

SEED = 23
FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return GA.compile_host_shim(tmp_path_factory.mktemp("gadget_generators_host") / "generators")


@pytest.mark.parametrize("field", FIELDS)
def test_every_kind_equals_the_mirror_at_every_class(exe, tmp_path, field):
    cases, wants = [], []
    for k, kind in enumerate(GA.KINDS):
        insts, used = GA.instances(field, kind, 160, 100 * field + k)
        cases.append(GA.pack_instances(field, insts, used))
        wants.append(GA.mirror(field, insts))
    res, text = GA.run_values(exe, tmp_path, cases)
    for kind, r, want in zip(GA.KINDS, res, wants):
        GA.assert_values(r, want, "%s (field %d)\n%s" % (kind, field, text))
        assert r["num_levels"] == 1


def test_the_cases_hold_what_they_promise():
    """the shapes and edges the issue lists are in the first 160 instances of each kind"""
    for field in FIELDS:
        p, D = GV.FIELDS[field].P, GV.FIELDS[field].D
        ops = {kind: GA.operands(field, kind, 160, 1) for kind in GA.KINDS}
        pairs = {o for _, o in ops["equality"]}
        assert {(0, 0), (0, p - 1), (p - 1, 0), (1, 0)} <= pairs and any(x == y and x > 1 for x, y in pairs) and any(y == x + 1 for x, y in pairs)
        if field == N.GB_GOLDILOCKS:
            assert {(2**32 - 1, 2**32), (2**32, p - 2**32), (p - 2**32, 0)} <= pairs
        assert {o for _, o in ops["quotient_or_zero"]} >= {(0, 0), (1, 0), (0, p - 1)}
        assert {o[0] for _, o in ops["nonzero_test"]} >= {0, 1, p - 1}
        dens = [tuple(o[D:]) for _, o in ops["quotient_extension"]]
        assert any(d[0] and not any(d[1:]) for d in dens) and any(not d[0] and all(d[1:]) for d in dens) and (p - 1,) * D in dens
        assert any(not any(o[:D]) for _, o in ops["quotient_extension"])
        assert {s for s, _ in ops["split"]} == {1, 2, 31, 64} and (64, (p - 1,)) in ops["split"] and (31, (2**31 - 1 if p > 2**31 else p - 1,)) in ops["split"]
        assert {s for s, _ in ops["wire_split"]} >= {(1, 1), (1, 3), (31, 3), (63, 1), (63, 3), (64, 1), (64, 2)}
        assert ((64, 2), (p - 1,)) in ops["wire_split"]
        assert {s for s, _ in ops["low_high"]} == {0, 1, 31, 63} and (63, (p - 1,)) in ops["low_high"]
        assert {s for s, _ in ops["base_sum"]} >= {(1, 2), (2, 2), (63, 2), (64, 2)} and {s[1] for s, _ in ops["base_sum"]} == {2, 3, 255}
        assert ((64, 2), [1] * 64) in ops["base_sum"]


@pytest.mark.parametrize("field", FIELDS)
def test_edge_semantics_word_for_word(exe, tmp_path, field):
    """what the header promises of the integer kinds, against plain arithmetic instead of the mirror"""
    p = GV.FIELDS[field].P
    v = p - 1
    made = [GA.make(field, "wire_split", (64, 2), 0, (v,)), GA.make(field, "low_high", 0, 10, (v,)), GA.make(field, "base_sum", (64, 2), 20, [1] * 64),
            GA.make(field, "nonzero_test", None, 90, (0,)), GA.make(field, "quotient_or_zero", None, 94, (5, 0)),
            GA.make(field, "equality", None, 100, (v, v))]
    insts = [(g, i) for g, i, _ in made]
    (r,), _ = GA.run_values(exe, tmp_path, [GA.pack_instances(field, insts, 104)])
    val = lambda t: int(r["values"][t])
    assert r["err"] == [0, 0, 0, 0]
    assert (val(1), val(2)) == (v, 0)                       # num_limbs = 64: the first sum takes the whole value, the second is 0
    assert (val(11), val(12)) == (0, v)                     # n_log = 0
    assert val(20) == (2**64 - 1) % p                       # 64 one-limbs wrap mod p
    assert val(91) == 1 and val(96) == 0 and (val(102), val(103)) == (1, 0)


@pytest.mark.parametrize("field", FIELDS)
def test_the_panics_of_the_reference_end_in_the_error_word(exe, tmp_path, field):
    p = GV.FIELDS[field].P
    cases, meta = [], []
    for kind in GA.KINDS:
        f = GA.failing(field, kind)
        if f is None:
            continue
        shape, ops, code, offender = f
        # two good generators in front: the failing head is record 2 + their continuation records, not generator 2
        good, used = GA.instances(field, kind, 2, 5)
        g, inputs, width = GA.make(field, kind, shape, used, ops)
        head = sum(len(x.record(GA._Stub)) for x, _ in good)
        cases.append(GA.pack_instances(field, good + [(g, inputs)], used + width))
        meta.append((kind, g, inputs, code, head, GA._Stub.target_index(g.targets()[offender])))
    assert {m[3] for m in meta} == {GA.ERR_SPLIT_TOO_LARGE, GA.ERR_DIVIDE_BY_ZERO, GA.ERR_NOT_BOOLEAN}
    res, _ = GA.run_values(exe, tmp_path, cases)
    for (kind, g, inputs, code, head, target), r in zip(meta, res):
        assert not isinstance(r, int), kind
        assert r["err"][:2] == [code, head], (kind, r["err"])
        assert int(r["class_reps"][r["err"][2]]) == target, (kind, r["err"])
        with pytest.raises(AssertionError):                      # the mirror's assert
            GA.mirror(field, [(g, inputs)])


@pytest.mark.parametrize("field", FIELDS)
def test_builder_circuits_equal_the_mirror_at_every_class(exe, tmp_path, field):
    circuits = [(name, b.build(), pw) for name, b, pw in GA.builder_circuits(field)]
    cases, kinds = [], set()
    for name, built, pw in circuits:
        inputs = GC.built_inputs(built, pw)
        built._input_targets = list(inputs)
        cases.append(GC.pack_built(built, inputs, values=built.input_values(pw, np.random.default_rng(SEED))))
        kinds |= {r[0] for r in built.generator_records()}
    assert kinds >= {N.GB_GEN_EQUALITY, N.GB_GEN_QUOTIENT_OR_ZERO, N.GB_GEN_QUOTIENT_EXTENSION, N.GB_GEN_WIRE_SPLIT, N.GB_GEN_LOW_HIGH,
                     N.GB_GEN_BASE_SUM, N.GB_GEN_TARGETS, N.GB_GEN_BASE_SPLIT, N.GB_GEN_ARITHMETIC_EXTENSION, N.GB_GEN_MUL_EXTENSION}
    res, text = GA.run_values(exe, tmp_path, cases)
    for (name, built, pw), r in zip(circuits, res):
        what = "%s (field %d)\n%s" % (name, field, text)
        assert not isinstance(r, int), "%s: refused with status %r" % (what, r)
        assert r["err"][0] == 0, "%s: error word %r" % (what, r["err"])
        assert r["num_unrunnable"] == 0, what
        want = built.generate_partition_witness(pw, np.random.default_rng(SEED)).astype(np.uint64)
        bad = np.nonzero(r["values"] != want[r["class_reps"]])[0]
        assert not len(bad), "%s: %d classes differ, first at target %d: %d, mirror %d" % (
            what, len(bad), r["class_reps"][bad[0]], r["values"][bad[0]], want[r["class_reps"][bad[0]]])
        covered = np.zeros(len(want), dtype=bool)
        covered[r["class_reps"]] = True
        assert not want[~covered].any(), what
        # the gadgets' own constraints pin the generated values: the public inputs say what was computed
        assert r["num_launches"] == 1


@pytest.mark.parametrize("field", FIELDS)
def test_the_gadgets_compute_what_they_say(field):
    """the mirror itself against plain arithmetic on the public inputs of tests/gadget_cases.py's circuits"""
    p = GV.FIELDS[field].P
    got = {}
    for name, b, pw in GA.builder_circuits(field):
        built = b.build()
        got[name] = built.generate_witness(pw)[1]
    assert got["is_equal, equal inputs"] == [1, p - 2] and got["is_equal, unequal inputs"] == [0, 77]
    assert got["split_le, 1 bit"] == [1, 1]
    top = GA.top_bits(field)
    assert got["split_le, %d bits" % top] == [(p - 1) & 1, (p - 1) >> (top - 1)]
    ops = 20 if field == N.GB_GOLDILOCKS else 10
    for name, nbits in (("le_sum, arithmetic branch", ops + 1), ("le_sum, BaseSumGate branch", ops + 2)):
        assert got[name] == [sum(((0xB5A3C96 >> (i % 28)) & 1) << i for i in range(nbits))]
    assert got["split_low_high"] == [0xABCDE & 31, 0xABCDE >> 5]
    assert got["select"] == [p - 1, 2, 1]
    assert got["low_bits"] == [((p - 3) >> i) & 1 for i in range(3)] + [2, 1, 2, 1, pow(50, p - 2, p)]      # 50 = 1212 in base 3
    q = got["div_extension"]
    D = GV.FIELDS[field].D
    from plonky2_goldibear_amd.recursion_gates import Ext
    E = Ext(field)
    x, y = tuple((p - 1 - k) % p for k in range(D)), tuple(3 + 5 * k for k in range(D))
    assert E.mul(tuple(q[:D]), y) == x and q[D] * 8 % p == x[0] and q[D + 1] * x[1] % p == 1
