"""The parser of constraint programs - untrusted words handed to gb_verifier_create_programs (csrc/prover_host.inc
parse_programs) - and the interpreter gb_verify runs on what was accepted, under AddressSanitizer + UndefinedBehaviorSanitizer:
a stand-alone program (tests/sanitize/fuzz_gate_programs.cpp, its own main) linked with a host-only build of the library's host
code mutates the programs of the reference's recursion fixture (tests/gate_programs.py: eight of its gates as programs) -
truncation, index flips, offset-table corruption, oversized headers - and every call must come back with a status and no
sanitizer report.  CPU only; no GPU is touched."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import verifier as V
from plonky2_goldibear_amd.gate_program import pack_programs

from test_gate_programs import FIXTURE_KINDS, as_programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "sanitize")
CSRC = os.path.join(ROOT, "plonky2_goldibear_amd", "csrc")
OUT = os.path.join(HERE, "_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
COMMON = ["-std=c++17", "-O0", "-g1", "-fPIC", "-w", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def build_harness():
    """csrc/api.hip (all of the library's host code, no kernels) host-only with the sanitizers, linked with the harness and the
    library's ordinary kernel objects, which are never called here"""
    sys.path.insert(0, ROOT)
    from plonky2_goldibear_amd import build as B
    B.build_library()
    os.makedirs(OUT, exist_ok=True)
    exe, api, src = os.path.join(OUT, "fuzz_gate_programs"), os.path.join(OUT, "api_gate_programs.hip.o"), os.path.join(HERE, "fuzz_gate_programs.cpp")
    inputs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [src, os.path.join(ROOT, "include", "goldibear_gpu.h"), __file__]
    if os.path.exists(exe) and all(os.path.getmtime(p) < os.path.getmtime(exe) for p in inputs):
        return exe
    objs = [os.path.join(B.OBJDIR, os.path.basename(s) + ".o") for s in B.sources() if not s.endswith("api.hip")]
    subprocess.check_call([CLANG, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950"] + COMMON + SAN +
                          ["-c", os.path.join(CSRC, "api.hip"), "-o", api])
    subprocess.check_call([CLANG] + COMMON + SAN + [src, api] + objs + ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness():
    assert os.path.exists(CLANG), "needs the ROCm clang++ that builds the library (a missing compiler must not hide this test)"
    return build_harness()


def test_program_table_mutations(harness, golden_dir, tmp_path):
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    common = rd("recursive_verifier_gl_common_data.bin")
    cd = V.read_common_data(common)
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    gates, programs = as_programs(V.read_gates(common, cd), tuple(FIXTURE_KINDS))
    words, offsets = pack_programs(programs)
    cfg, fc = cd["config"], cd["config"]["fri_config"]
    nsel = len(cd["selectors_info"]["groups"])
    cfg_words = [0, cd["fri_params"]["degree_bits"], cfg["num_wires"], cfg["num_routed_wires"], cd["num_constants"] - nsel,
                 cfg["num_challenges"], cd["quotient_degree_factor"], fc["rate_bits"], fc["cap_height"], fc["proof_of_work_bits"],
                 fc["num_query_rounds"], 4, 5, nsel, 0, 0, 1 if cd["fri_params"]["hiding"] else 0, cd["num_public_inputs"]]
    proof = rd("recursive_verifier_gl_proof.bin")
    case = str(tmp_path / "programs.case")
    with open(case, "wb") as f:
        f.write(struct.pack("<18I", *cfg_words))
        f.write(struct.pack("<I", len(gates)))
        for g in gates:
            f.write(struct.pack("<7I", *g))
        for part in (cd["k_is"], vd["constants_sigmas_cap"], vd["circuit_digest"]):
            f.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
        f.write(struct.pack("<I", len(programs)))
        f.write(offsets.tobytes())
        f.write(words.tobytes())
        f.write(struct.pack("<Q", len(proof)))
        f.write(proof)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:allocator_may_return_null=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([harness, case, "2000", str(0x9A7E5)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "fuzz ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    # the loop reached the parser's refusals, accepted tables that then fail the identity, and accepted harmless mutants
    created, refused = (int(x) for x in out.stdout.split("create ok/invalid = ")[1].split(";")[0].split("/"))
    v_ok, v_invalid, v_verify = (int(x) for x in out.stdout.split("verify ok/invalid/verify = ")[1].split()[0].split("/"))
    assert refused > 1000 and created > 100 and v_verify > 50, out.stdout
    assert v_ok + v_invalid + v_verify == created
