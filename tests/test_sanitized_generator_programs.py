"""tests/sanitize/generator_programs.cpp: the validator of gb_circuit_set_generator_programs (csrc/generator_programs.hpp) and the
GEN_PROGRAM head record of csrc/generator_schedule.hpp in a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer - every refusal with its index, truncated and bit-flipped tables and record arrays in allocations of
exactly the length handed over, the level order around a program generator and the row constants.  No GPU, nothing preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_validator_and_head_record_under_the_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "needs the ROCm clang++"
    exe = tmp_path / "generator_programs"
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "generator_programs.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:] + out.stderr[-3000:])
    assert "all checks held" in out.stdout
