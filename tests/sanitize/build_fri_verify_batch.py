"""The harness fuzz_fri_verify_batch.cpp linked with the HOST-ONLY, sanitized build of the library's host code that build.py makes
for fuzz_host_parsers.cpp (the same api.hip object and kernel-unit objects; nothing of them runs on a device here).
Output: tests/sanitize/_build/fuzz_fri_verify_batch."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import build as SB  # noqa: E402

EXE = os.path.join(SB.OUT, "fuzz_fri_verify_batch")
SRC = os.path.join(HERE, "fuzz_fri_verify_batch.cpp")


def build(force=False):
    base = SB.build(force)   # api.hip.o under the sanitizers, the kernel units' ordinary objects
    if not force and os.path.exists(EXE) and all(os.path.getmtime(p) < os.path.getmtime(EXE) for p in (base, SRC, __file__)):
        return EXE
    from plonky2_goldibear_amd import build as B
    objs = [os.path.join(B.OBJDIR, os.path.basename(src) + ".o") for src in B.sources() if not src.endswith("api.hip")]
    objs.append(os.path.join(SB.OUT, "api.hip.o"))
    subprocess.check_call([SB.CLANG] + SB.COMMON + SB.SAN + [SRC] + objs + ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE])
    return EXE


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
