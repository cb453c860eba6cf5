"""The generator kernels (csrc/generators.hpp: k_scatter_inputs, k_generate_level<F>, k_generate_chain<F>, k_gather_public) on the
GPU, built for gfx950 from the headers alone (tests/device/generators.hip) and run on the schedule csrc/generator_schedule.hpp
makes of described circuits.  The oracle is the builder mirror's generators (circuit_builder.py, recursion_gates.py), every
comparison exact and at every class.

  * every generator kind over the gate parameters of tests/gate_variants.py's grid, on 1, 63, 64, 65 and 300 independent rows
    through k_generate_level: a partial wave, the wave's edges, more than one workgroup.  Inputs: the fields' carry-edge words,
    then random words.  The grid is cut into batches (the pure-Python mirror on 300 rows is the cost); a batch computes the
    mirror's rows once and every smaller count takes the first of them.
  * k_generate_chain on arithmetic chains 1, 2, 257 and 600 levels deep, each with levels one generator wide and levels as wide
    as the workgroup: one launch each, values handed from level to level inside the kernel."""
import os
import subprocess

import numpy as np
import pytest

import gate_variants as GV
import generator_cases as GC
from plonky2_goldibear_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = 8


def batch(field, b):
    return list(range(b, GV.GRID_SIZE[field], BATCHES))


def test_the_batches_cover_every_generator_kind():
    """no GPU: the grid holds a gate for every gate generator kind of the field and the batches cover the grid"""
    for field in GV.FIELDS:
        gates = GV.grid(field)
        assert sorted(t for b in range(BATCHES) for t in batch(field, b)) == list(range(len(gates)))
        kinds = set()
        for gate in gates:
            inst = GC.instance_rows(field, gate, 1, 1)
            if inst is None:
                assert gate[0] == 2, gate     # PublicInputGate: its wires are set through copy constraints, it has no generator
                continue
            stub = GC._Rows(inst["num_wires"], 1)
            kinds |= {gen.record(stub)[0] for gen in inst["rows"][0][0]}
        field_only = {N.GB_GEN_POSEIDON2_BABYBEAR, N.GB_GEN_POSEIDON2_INTERNAL} if field == N.GB_GOLDILOCKS else {N.GB_GEN_POSEIDON, N.GB_GEN_POSEIDON_MDS}
        assert kinds == set(range(16)) - field_only


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("generators_dev") / "generators"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-I", os.path.join(ROOT, "tests", "sanitize"), "-o", str(out), os.path.join(ROOT, "tests", "device", "generators.hip")],
                   check=True, capture_output=True, text=True)
    return str(out)


def run_device(exe, tmp_path, cases, mode, tag=""):
    src, dst = tmp_path / ("in%s.bin" % tag), tmp_path / ("out%s.bin" % tag)
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst), mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return GC.read_values(np.fromfile(dst, dtype=np.uint64), len(cases), gathered=[0] * len(cases))


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(BATCHES))
@pytest.mark.parametrize("field", sorted(GV.FIELDS))
def test_level_kernel_equals_the_mirror_for_every_kind(exe, tmp_path, field, b):
    F = GV.FIELDS[field]
    top = max(GV.ROW_COUNTS)
    insts = [i for i in (GC.instance_rows(field, GV.grid(field)[t], top, 2000 * field + t) for t in batch(field, b)) if i is not None]
    assert insts
    want = [[GC.mirror_row(inst, j, F.P) for j in range(top)] for inst in insts]
    for nrows in GV.ROW_COUNTS:
        res = run_device(exe, tmp_path, [GC.pack_instances(inst, nrows, F.P, F.D) for inst in insts], "level", str(nrows))
        for inst, rows, r in zip(insts, want, res):
            what = "%r, %d rows" % (inst["gate"], nrows)
            assert not isinstance(r, int), "%s: refused with status %r" % (what, r)
            assert r["err"] == [0, 0, 0, 0] and r["num_unrunnable"] == 0 and r["num_levels"] == 1, what
            nw = inst["num_wires"]
            expect = np.zeros(len(r["values"]), dtype=np.uint64)
            assert np.array_equal(r["class_reps"], np.arange(len(expect)))      # identity map: class k is target k
            for j in range(nrows):
                for t, v in rows[j].items():
                    expect[t[1] * nw + t[2]] = v
            bad = np.nonzero(r["values"] != expect)[0]
            assert not len(bad), "%s: %d words differ, first at row %d wire %d: %d, mirror %d" % (
                what, len(bad), bad[0] // nw, bad[0] % nw, r["values"][bad[0]], expect[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, GC.GROUP])
@pytest.mark.parametrize("field", sorted(GV.FIELDS))
def test_chain_kernel_hands_values_from_level_to_level(exe, tmp_path, field, width):
    depths = (1, 2, 257, 600)
    built = [GC.arithmetic_chain(field, d, width, 77 + d) for d in depths]
    res = run_device(exe, tmp_path, [c for c, _ in built], "plan")
    for d, (_, want), r in zip(depths, built, res):
        what = "depth %d, width %d" % (d, width)
        assert not isinstance(r, int), what
        assert r["err"] == [0, 0, 0, 0] and r["num_unrunnable"] == 0, what
        assert r["num_levels"] == d and r["num_launches"] == 1, what          # one launch of the chain kernel
        expect = np.zeros(len(r["values"]), dtype=np.uint64)
        index = {int(t): k for k, t in enumerate(r["class_reps"])}
        for t, v in want.items():
            expect[index[t]] = v
        bad = np.nonzero(r["values"] != expect)[0]
        assert not len(bad), "%s: %d classes differ, first at target %d" % (what, len(bad), r["class_reps"][bad[0]])
