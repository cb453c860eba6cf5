"""The evaluators of the gadget generators (csrc/generators.hpp, record kinds 32..39) in the generator kernels on the GPU, built
for gfx950 from the headers alone (tests/device/generators.hip) as tests/test_device_generators.py runs the gate generators.  The
oracle is the builder mirror; every comparison is exact and at every class.

  * k_generate_level: every kind as 1, 63, 64, 65 and 300 independent records of tests/gadget_cases.py - a partial wave, the
    wave's edges, more than one workgroup - the edge operands first, then random ones;
  * k_generate_chain: split_low_high -> split_le -> le_sum -> is_equal, round after round, 40 levels and more in ONE launch,
    values handed from level to level inside the kernel."""
import numpy as np
import pytest

import gadget_cases as GA
import generator_cases as GC
import gate_variants as GV
from plonky2_goldibear_amd import native as N

FIELDS = [N.GB_GOLDILOCKS, N.GB_BABYBEAR]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return GA.compile_device(tmp_path_factory.mktemp("gadget_generators_dev") / "generators")


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_level_kernel_equals_the_mirror_for_every_gadget_kind(exe, tmp_path, field):
    top = max(GV.ROW_COUNTS)
    per_kind = [GA.instances(field, kind, top, 300 * field + k)[0] for k, kind in enumerate(GA.KINDS)]
    for count in GV.ROW_COUNTS:
        cases, wants = [], []
        for insts in per_kind:
            part = insts[:count]
            used = 1 + max(GA._Stub.target_index(t) for g, _ in part for t in g.targets())
            cases.append(GA.pack_instances(field, part, used))
            wants.append(GA.mirror(field, part))
        res, text = GA.run_values(exe, tmp_path, cases, "level", str(count))
        for kind, r, want in zip(GA.KINDS, res, wants):
            what = "%s, %d records (field %d)\n%s" % (kind, count, field, text)
            GA.assert_values(r, want, what)
            assert r["num_levels"] == 1, what


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_the_error_word_from_the_level_kernel(exe, tmp_path, field):
    """one failing record behind 299 good ones: the error word names its head record and the offending class; nothing faults"""
    cases, meta = [], []
    for kind in GA.KINDS:
        f = GA.failing(field, kind)
        if f is None:
            continue
        shape, ops, code, offender = f
        good, used = GA.instances(field, kind, 299, 7)
        g, inputs, width = GA.make(field, kind, shape, used, ops)
        cases.append(GA.pack_instances(field, good + [(g, inputs)], used + width))
        meta.append((kind, code, sum(len(x.record(GA._Stub)) for x, _ in good), GA._Stub.target_index(g.targets()[offender])))
    res, _ = GA.run_values(exe, tmp_path, cases, "level")
    for (kind, code, head, target), r in zip(meta, res):
        assert not isinstance(r, int), kind
        assert r["err"][:2] == [code, head] and int(r["class_reps"][r["err"][2]]) == target, (kind, r["err"])


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_forty_levels_of_chained_gadgets_are_one_launch(exe, tmp_path, field):
    b, pw = GA.chained_gadgets(field, 40)
    built = b.build()
    inputs = GC.built_inputs(built, pw)
    built._input_targets = list(inputs)
    case = GC.pack_built(built, inputs, values=built.input_values(pw, np.random.default_rng(5)))
    (r,), text = GA.run_values(exe, tmp_path, [case], "plan", public=[len(built.public_inputs)])
    assert not isinstance(r, int), text
    assert [int(v) for v in r["public"]] == built.generate_witness(pw, np.random.default_rng(5))[1]      # k_gather_public
    assert r["err"] == [0, 0, 0, 0] and r["num_unrunnable"] == 0
    assert r["num_levels"] >= 40 and r["num_launches"] == 1          # one launch of the chain kernel
    kinds = {rec[0] for rec in built.generator_records()}
    assert kinds >= {N.GB_GEN_LOW_HIGH, N.GB_GEN_WIRE_SPLIT, N.GB_GEN_BASE_SUM, N.GB_GEN_EQUALITY, N.GB_GEN_BASE_SPLIT}
    want = built.generate_partition_witness(pw, np.random.default_rng(5)).astype(np.uint64)
    bad = np.nonzero(r["values"] != want[r["class_reps"]])[0]
    assert not len(bad), "%d classes differ, first at target %d: %d, mirror %d" % (
        len(bad), r["class_reps"][bad[0]], r["values"][bad[0]], want[r["class_reps"][bad[0]]])
    covered = np.zeros(len(want), dtype=bool)
    covered[r["class_reps"]] = True
    assert not want[~covered].any()


def test_the_chain_is_forty_levels_deep_on_the_host():
    """no GPU: the mirror runs the chained circuit, and its last value is what the rounds compute"""
    for field in FIELDS:
        b, pw = GA.chained_gadgets(field, 40)
        built = b.build()
        n_log, num_bits = (24, 30) if field == N.GB_GOLDILOCKS else (12, 20)
        x = (1 << num_bits) - 5
        for _ in range(GA.chain_rounds(40)):
            x = (x & ((1 << n_log) - 1)) + 1
        assert built.generate_witness(pw)[1] == [x]
