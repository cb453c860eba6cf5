"""The device-side permutation header compiled for the CPU (g++, tests/host_shim) and compared with the host mirror on random and
extreme states: the signed / lazy / offset bookkeeping of csrc/poseidon2_bb.hpp is integer arithmetic that does not need a GPU
to be checked, and its failures would be data dependent."""
import os
import subprocess

import numpy as np
import pytest

import permutation_states as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poseidon2_bb_lane_permutation_matches_host_mirror(tmp_path):
    exe = tmp_path / "poseidon2_bb_lane"
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = ["g++", "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "poseidon2_bb_lane.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), "200000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout


def test_bb_wide_accumulators_match_montgomery_sums(tmp_path):
    exe = tmp_path / "bb_wide_acc"
    shim = os.path.join(ROOT, "tests", "host_shim")
    clang = "/opt/rocm/lib/llvm/bin/clang++"   # field_traits.hpp pulls in gl_field.hpp, whose limb code uses clang's __builtin_addc
    if not os.path.exists(clang):
        pytest.skip("needs the ROCm clang++ as the host compiler")
    cmd = [clang, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "bb_wide_acc.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout


def test_challenge_slices_cover_every_count(tmp_path):
    """csrc/challenge_slices.hpp: how a num_challenges without a compiled kernel width is split into launches"""
    exe = tmp_path / "challenge_slices"
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe),
           os.path.join(shim, "challenge_slices.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout


def test_host_transcript_permutation_matches_the_defining_form(tmp_path):
    """csrc/poseidon_gl_host.hpp (the Fiat-Shamir transcript's Poseidon-12: fast partial rounds with the sparse v / w_hat / M_init
    constants, MDS rows in 128-bit accumulators) == the naive 30-round definition written from the round constants and the MDS matrix
    alone, canonical outputs, on random and extreme states"""
    exe = tmp_path / "poseidon_gl_host_forms"
    shim = os.path.join(ROOT, "tests", "host_shim")
    clang = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
    if not os.path.exists(clang):
        pytest.skip("needs the ROCm clang++ as the host compiler")
    cmd = [clang, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "poseidon_gl_host_forms.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), "20000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout


def test_poseidon2_bb_steps_keep_their_bounds_on_pulled_back_states(tmp_path):
    """csrc/poseidon2_bb.hpp's permute_scaled one step at a time (tests/host_shim/poseidon2_bb_steps.cpp) on the BabyBear states of
    tests/permutation_states.py and 50 000 random ones: the stated bounds after every step, the chosen word at its place (which
    checks the scale sequence the Python model restates), equality with permute_scaled and with the host mirror at the end"""
    exe = tmp_path / "poseidon2_bb_steps"
    shim = os.path.join(ROOT, "tests", "host_shim")
    cmd = ["g++", "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "poseidon2_bb_steps.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    m = PS.model(PS.BB)
    records = []
    for t in PS.targets(PS.BB) + PS.zero_capacity_targets(PS.BB):
        # one word per state: any word in the external rounds; inside the internal rounds words 1..15 carry per-round offsets
        index = min(t.words) if m.is_full(t.round) else (0 if 0 in t.words else None)
        records.append(list(t.input) + [2 * t.round + (t.where == PS.MDS_IN)] + ([index, t.words[index]] if index is not None else [0xFFFFFFFF, 0]))
    probed = sum(1 for r in records if r[17] != 0xFFFFFFFF)
    assert probed >= len(records) * 3 // 4
    np.array(records, dtype=np.uint32).tofile(tmp_path / "states.bin")
    out = subprocess.run([str(exe), str(tmp_path / "states.bin"), "50000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "states=%d " % (len(records) + 50000) in out.stdout and "place_checks=%d " % probed in out.stdout and "mismatches=0" in out.stdout


HOST_GATE_ROWS = 24   # past the longest list of edge words: every column has passed through all of them


@pytest.fixture(scope="module")
def gate_eval_exe(tmp_path_factory):
    shim = os.path.join(ROOT, "tests", "host_shim")
    clang = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
    if not os.path.exists(clang):
        pytest.skip("needs the ROCm clang++ as the host compiler")
    exe = tmp_path_factory.mktemp("gate_eval_host") / "gate_eval"
    cmd = [clang, "-O2", "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "gate_eval.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(exe)


@pytest.mark.parametrize("algebra", ["base", "extension"])
@pytest.mark.parametrize("field", [0, 1])
def test_gate_evaluators_equal_the_oracle_over_both_algebras(gate_eval_exe, tmp_path, field, algebra):
    """csrc/gates.hpp's eval_gate and filter over BaseAlg<F> (the quotient kernel's algebra, wires F.efrom(v)) and ExtAlg<F> (what
    gb_verify runs at zeta: every wire, constant and selector a D-tuple of edge or random words, all D output coordinates compared)
    == oracle/gates.py eval_unfiltered / compute_filter, for every gate of tests/gate_variants.py's grid - every parameter
    gb_circuit_create_gates accepts, where tests/test_verifier_differential.py and the reference's fixture hold one
    parameterisation per gate.  Also gates::num_wires / num_constraints / num_constants against recursion_gates.py's figures and
    the oracle's num_constraints, for the whole grid."""
    import gate_variants as GV
    F = GV.FIELDS[field]
    width = 1 if algebra == "base" else F.D
    entries = GV.cases(field, width, HOST_GATE_ROWS)
    assert len(entries) == GV.GRID_SIZE[field] == {0: 89, 1: 90}[field]   # no entry drops out silently
    assert HOST_GATE_ROWS > len(GV.edge_values(F)) + 3
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    GV.pack(field, HOST_GATE_ROWS, width, entries).tofile(src)
    out = subprocess.run([gate_eval_exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    assert "gates=%d rows=%d width=%d" % (len(entries), HOST_GATE_ROWS, width) in out.stdout
    bad = GV.compare(field, HOST_GATE_ROWS, width, entries, np.fromfile(dst, dtype=np.uint64))
    assert not bad, "\n".join(bad[:10])
