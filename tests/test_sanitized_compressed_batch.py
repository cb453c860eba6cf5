"""The host stage of gb_verify_compressed_batch - the shared parser of compressed proofs (csrc/compress_host.inc), the sibling count
(csrc/verify_compressed.hpp) and the stage itself (csrc/verify_batch_host.inc) - under AddressSanitizer + UndefinedBehaviorSanitizer:
the host-only build of the library's host code (tests/sanitize/build_compressed_batch.py) is driven by a stand-alone mutation loop
(tests/sanitize/fuzz_compressed_batch.cpp) with a NULL context, so no device is touched.  Compressed proofs of tiny circuits are
truncated, bit-flipped, spliced, extended and given shorter and longer paths; what the host stage decides must be what
gb_verify_compressed says, and what it leaves to a device must have passed the parser, the index comparison and the sibling count.
CPU only; nothing is loaded into Python."""
import os
import subprocess
import sys

import pytest

from oracle import plonk_dummy as D
from oracle.fields import BB, GL

from test_sanitized_parsers import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "sanitize"))


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("no ROCm clang++ to build the sanitized harness with")
    import build_compressed_batch as SB
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


@pytest.mark.parametrize("F,lg,kw", [
    (GL, 5, {}),
    (BB, 5, {}),
    (GL, 6, dict(rate_bits=6, cap_height=0, arity_bits=6, final_poly_bits=0, num_query_rounds=6)),
], ids=["goldilocks", "babybear", "goldilocks-cap0-arity64"])
def test_mutated_compressed_proofs_of_a_tiny_circuit(harness, tmp_path, F, lg, kw):
    cfg = (D.CircuitConfig(**kw) if F is GL else D.CircuitConfig.babybear(**kw)) if kw else None
    circ = D.DummyCircuit(lg, cfg, F=F) if cfg is not None else D.DummyCircuit(lg, F=F)
    proof, _ = D.prove_cpu(circ, circ.witness(seed=3))
    assert D.verify(circ, proof)
    c = circ.cfg
    words = [0 if F is GL else 1, circ.degree_bits, c.num_wires, c.num_routed_wires, c.num_constants, c.num_challenges,
             c.max_quotient_degree_factor, c.rate_bits, c.cap_height, c.proof_of_work_bits, c.num_query_rounds, c.arity_bits,
             c.final_poly_bits, circ.num_selectors, 0, 0, 0, 0]
    case = str(tmp_path / "tiny.case")
    _case(case, words, circ.gate_table, circ.k_is, circ.constants_sigmas_cap, circ.circuit_digest, proof, F.dtype)
    line = _run(harness, case, 150, 11 + lg + F.D)
    decided = int(line.split("host decided ")[1].split(",")[0])
    left = int(line.split("left to the device ")[1].split(";")[0])
    assert decided > 100 and left > 20, line   # both ends of the host stage were reached
