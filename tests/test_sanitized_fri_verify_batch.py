"""The host stage of gb_fri_verify_batch - the item's canonical checks, the FriProof parser (csrc/verifier_host.inc), the transcript,
the proof of work, the regularity test and the stage itself (csrc/verify_batch_host.inc) - under AddressSanitizer +
UndefinedBehaviorSanitizer: the host-only build of the library's host code (tests/sanitize/build_fri_verify_batch.py) is driven by a
stand-alone mutation loop (tests/sanitize/fuzz_fri_verify_batch.cpp) with a NULL context, so no device is touched.  An item's proof is
truncated, bit-flipped, spliced, extended and given shorter and longer path-length bytes (the true ones, found from the shape;
also in pairs that keep the proof's length), its points, openings and caps a word >= p;
what the host stage decides must be what gb_fri_verify says, and what it leaves to a device must have passed the parser, the proof
of work and the regularity test.  CPU only; nothing is loaded into Python."""
import os
import subprocess
import sys

import pytest

import fri_batch_helpers as H
import fri_instances as FI
from oracle import plonk_dummy as D
from oracle import verifier as V
from oracle.fields import BB, GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "sanitize"))


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang++ to build the sanitized harness with")
    import build_fri_verify_batch as SB
    return SB.build()


def _run(harness, case, iterations, seed):
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([harness, case, str(iterations), str(seed)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "fuzz ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    return out.stdout


def _counts(line):
    """(host decided, left to the device, items of the shape's own length that gb_fri_verify refuses for a path of the wrong length:
    the case the regularity test exists for)"""
    return (int(line.split("host decided ")[1].split(",")[0]), int(line.split("left to the device ")[1].split(";")[0]),
            int(line.split("irregular at the shape's length ")[1].split()[0]))


def test_mutated_reference_proof(harness, tmp_path, golden_dir):
    """the reference's own Goldilocks recursion proof (recursion/regression_test_data.rs) as a general instance"""
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    inst, params, item, _ = H.plonk_item(GL, cd, vd["circuit_digest"], vd["constants_sigmas_cap"], rd("recursive_verifier_gl_proof.bin"))
    case = str(tmp_path / "reference.case")
    H.write_case(case, FI.field_tag(GL), inst, params, item)
    decided, left, irregular = _counts(_run(harness, case, 60, 29))
    assert decided > 100 and left > 10 and irregular > 0   # both ends of the host stage were reached, and the regularity test


def test_mutated_babybear_dummy_circuit_proof(harness, tmp_path):
    """a 2^5-row BabyBear dummy-circuit proof from the CPU oracle prover, described as its PLONK instance"""
    circ = D.DummyCircuit(5, F=BB)
    proof, _ = D.prove_cpu(circ, circ.witness(seed=3))
    assert D.verify(circ, proof)
    cap = [[int(x) for x in h] for h in circ.constants_sigmas_cap]
    inst, params, item, _ = H.plonk_item(BB, circ.common_data(), circ.circuit_digest, cap, proof)
    case = str(tmp_path / "tiny.case")
    H.write_case(case, FI.field_tag(BB), inst, params, item)
    decided, left, irregular = _counts(_run(harness, case, 150, 23))
    assert decided > 100 and left > 20 and irregular > 0
