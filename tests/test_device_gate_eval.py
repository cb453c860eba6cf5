"""gates::eval_gate<F, BaseAlg<F>, LIGHT_GATES | HEAVY_GATES> and gates::filter<F, BaseAlg<F>> on the GPU (csrc/gates.hpp as the
quotient kernel's two launches instantiate it: device Montgomery forms, mds_layer_gl_base, the `#pragma unroll 1` loops), built
for gfx950 from the header alone (tests/device/gate_eval.hip) and run on caller-supplied rows: the fields' carry-edge words and
random words as wires, constants and selector values.  For every gate of tests/gate_variants.py's grid - every parameter
gb_circuit_create_gates accepts, where prove() only ever sees one parameterisation per gate, on LDE values - the emitted
constraints equal oracle/gates.py eval_unfiltered on F.efrom(v) exactly (all higher coordinates zero, the count equal to
num_constraints), and the filter equals compute_filter for groups of 1, 2 and 7 gates with one and several selector columns.
Row counts 1, 63, 64, 65, 300: a partial wave, the wave boundaries, more than one workgroup.

The grid is cut into batches so that a case stays at a few seconds (the pure-Python oracle on 300 rows is the cost); a batch
computes its reference once, for 300 rows, and every smaller row count takes the first rows of it: one file, one process and
one launch per gate for each row count."""
import os
import subprocess

import numpy as np
import pytest

import gate_variants as GV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = 8


def batch(field, b):
    return list(range(b, GV.GRID_SIZE[field], BATCHES))


def test_the_batches_cover_the_grid_and_every_filter_shape():
    for field in GV.FIELDS:
        gates = GV.grid(field)
        assert len(gates) == GV.GRID_SIZE[field] and len(set(g[:2] + g[5:] for g in gates)) == len(gates)
        assert sorted(t for b in range(BATCHES) for t in batch(field, b)) == list(range(len(gates)))
        shapes = {(g[3], g[4], GV.many_selectors(t)) for t, g in enumerate(gates)}
        assert shapes == set(GV.FILTER_SHAPES) and {g[4] - g[3] for g in gates} == {1, 2, 7}
        # the gate's own index: first, last and inside its group
        places = {(GV.own_index(g, t) - g[3], g[4] - g[3]) for t, g in enumerate(gates)}
        assert {(0, 1), (0, 2), (1, 2), (0, 7), (6, 7), (3, 7)} <= places
        assert {GV.subset(g) for g in gates} == {GV.HEAVY, GV.LIGHT}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("gate_eval") / "gate_eval"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "gate_eval.hip")], check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(BATCHES))
@pytest.mark.parametrize("field", sorted(GV.FIELDS))
def test_device_evaluators_and_filter_equal_the_oracle(exe, tmp_path, field, b):
    full = GV.cases(field, 1, max(GV.ROW_COUNTS), batch(field, b))
    assert len(full) == len(batch(field, b)) >= GV.GRID_SIZE[field] // BATCHES
    for nrows in GV.ROW_COUNTS:
        entries = GV.prefix(full, nrows)
        src, dst = tmp_path / ("in%d.bin" % nrows), tmp_path / ("out%d.bin" % nrows)
        GV.pack(field, nrows, 1, entries).tofile(src)
        out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
        bad = GV.compare(field, nrows, 1, entries, np.fromfile(dst, dtype=np.uint64))
        assert not bad, "%d rows: %s" % (nrows, "\n".join(bad[:10]))
