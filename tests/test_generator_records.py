"""The generator records of the builder mirror (each _...Generator.record(), circuit_builder.py / recursion_gates.py) run on the
HOST: csrc/generator_schedule.hpp schedules them and csrc/generators.hpp's evaluators - the code of the generator kernels,
compiled for the CPU by tests/host_shim/generators.cpp - run the schedule.  The result must equal the mirror's
generate_partition_witness at every class, for every circuit of tests/gate_variants.py (one row of every buildable gate variant,
both fields) and for the recursion-gates circuit.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import circuits as CS
import gate_variants as GV
import generator_cases as GC
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import PartialWitness, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
SEED = 17


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    shim = os.path.join(ROOT, "tests", "host_shim")
    out = tmp_path_factory.mktemp("generators_host") / "generators"
    subprocess.run([CLANG, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim, "-I", os.path.join(ROOT, "tests", "sanitize"),
                    "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(out), os.path.join(shim, "generators.cpp")],
                   check=True, capture_output=True, text=True)
    return str(out)


def run_host(exe, tmp_path, circuits):
    """circuits = [(built, pw)] -> per circuit (status or dict(class_reps, values, err, ...), the mirror's input values)"""
    cases, metas = [], []
    for built, pw in circuits:
        inputs = GC.built_inputs(built, pw)
        built._input_targets = list(inputs)
        iv = built.input_values(pw, np.random.default_rng(SEED))
        cases.append(GC.pack_built(built, inputs, values=iv))
        metas.append(iv)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GC.write(src, cases)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return GC.read_values(np.fromfile(dst, dtype=np.uint64), len(circuits))


def assert_equals_mirror(built, pw, r, what):
    assert not isinstance(r, int), "%s: refused with status %r" % (what, r)
    assert r["err"][0] == 0, "%s: error word %r" % (what, r["err"])
    assert r["num_unrunnable"] == 0, what
    want = built.generate_partition_witness(pw, np.random.default_rng(SEED)).astype(np.uint64)
    bad = np.nonzero(r["values"] != want[r["class_reps"]])[0]
    assert not len(bad), "%s: %d classes differ, first at target %d: %d, mirror %d" % (
        what, len(bad), r["class_reps"][bad[0]], r["values"][bad[0]], want[r["class_reps"][bad[0]]])
    # and nothing the mirror set lies outside the schedule's classes
    covered = np.zeros(len(want), dtype=bool)
    covered[r["class_reps"]] = True
    assert not want[~covered].any(), what


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_variant_circuits_equal_the_mirror_at_every_class(exe, tmp_path, field):
    names = list(GV.variant_sets(field))
    circuits = []
    for name in names:
        b, pw, rows = GV.variant_circuit(field, name)
        circuits.append((b.build(), pw))
    kinds = set()
    for (built, pw), r, name in zip(circuits, run_host(exe, tmp_path, circuits), names):
        assert_equals_mirror(built, pw, r, "%s (field %d)" % (name, field))
        kinds |= {rec[0] for rec in built.generator_records()}
    # every gate generator kind of the field has run (Copy has no gate: tests/test_generator_schedule.py)
    field_only = {N.GB_GEN_POSEIDON2_BABYBEAR, N.GB_GEN_POSEIDON2_INTERNAL} if field == N.GB_GOLDILOCKS else {N.GB_GEN_POSEIDON, N.GB_GEN_POSEIDON_MDS}
    assert kinds == set(range(16)) - field_only, sorted(set(range(16)) - field_only - kinds)


@pytest.mark.parametrize("field", [N.GB_GOLDILOCKS, N.GB_BABYBEAR])
def test_recursion_gates_circuit_equals_the_mirror(exe, tmp_path, field):
    b, pw, rows = CS.recursion_gates_circuit(field)
    built = b.build()
    (r,) = run_host(exe, tmp_path, [(built, pw)])
    assert_equals_mirror(built, pw, r, "recursion_gates_circuit (field %d)" % field)


def test_hash_chains_and_public_inputs(exe, tmp_path):
    """the builder's own circuits: the public inputs' hash runs through PoseidonGate / Poseidon2BabyBearGate rows whose inputs are
    other generators' outputs"""
    circuits = []
    for b, pw in (CS.factorial_circuit(count=40), CS.fibonacci_circuit(terms=30), CS.babybear_public_input_circuit(steps=20)):
        circuits.append((b.build(), pw))
    for (built, pw), r in zip(circuits, run_host(exe, tmp_path, circuits)):
        assert_equals_mirror(built, pw, r, "builder circuit")
        assert r["num_launches"] == 1      # chains of narrow levels: one launch


def test_the_asserts_of_the_reference_end_in_the_error_word(exe, tmp_path):
    """a PoseidonGate row with swap = 2, a RandomAccessGate index equal to vec_size, a BaseSumGate value past its limbs"""
    from plonky2_goldibear_amd import recursion_gates as R
    from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PoseidonGate
    cfg = CircuitConfig.standard_recursion_config_gl()
    circuits, want = [], []
    # swap = 2
    b, pw = CircuitBuilder(cfg), PartialWitness()
    row = b.add_gate(PoseidonGate())
    for c in range(12):
        pw.set_target(wire(row, c), c + 1)
    pw.set_target(wire(row, PoseidonGate.WIRE_SWAP), 2)
    circuits.append((b.build(), pw))
    want.append((2, wire(row, PoseidonGate.WIRE_SWAP)))
    # access index == vec_size
    b, pw = CircuitBuilder(cfg), PartialWitness()
    g = R.RandomAccessGate(2, 1, 0)
    row = b.add_gate(g)
    pw.set_target(wire(row, g.wire_access_index(0)), g.vec_size)
    circuits.append((b.build(), pw))
    want.append((3, wire(row, g.wire_access_index(0))))
    # 9 does not fit three bits
    b, pw = CircuitBuilder(cfg), PartialWitness()
    row = b.add_gate(R.BaseSumGate(3, 2))
    pw.set_target(wire(row, 0), 9)
    circuits.append((b.build(), pw))
    want.append((4, wire(row, 0)))
    for (built, pw), r, (code, target) in zip(circuits, run_host(exe, tmp_path, circuits), want):
        assert r["err"][0] == code
        assert r["class_reps"][r["err"][2]] == built.representative_map[built.target_index(target)]
        assert built.generator_records()[r["err"][1]][2] == target[1]     # the record of that row
        with pytest.raises(AssertionError):
            built.generate_partition_witness(pw)                          # the mirror's assert
