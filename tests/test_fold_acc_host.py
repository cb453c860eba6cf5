"""The unreduced alpha-fold sums of the gate kernels - csrc/fold_acc.hpp's FoldAcc<GlF> (a 160-bit sum of 128-bit products, finished
by gl::fold160) and FoldAcc<BbF> (a 96-bit sum with a finish() of its own) - and gl::fold160 itself, compiled for the CPU
(tests/host_shim/fold_acc.cpp) and run on the chains of tests/host_shim/fold_acc_cases.hpp: chains built backwards from the sum they
must stand at before finish() or mid-chain (every combination of the limb edges, the top limb a gate's constraint count can
produce, sums congruent to 0, 1, p - 1, the sums on either side of each wrap inside BabyBear's finish()), edge-valued chains and
2^14 seeded random chains per field, of 1..17, 123 and 4096 terms; expected words from exact integers, compared as words.  The proofs
reach these sums with random words: a dropped carry or a missing second subtraction is a 2^-32 event there.  The runner's census
says how many chains reached each target class and each branch of fold160, and fails on an empty class.
tests/test_device_fold_acc.py runs the same chains on the GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family -> chains: what fold_acc_cases.hpp builds (seeded, the same on every machine); the device runner must report the same
CASES = {"gl_fold_acc": 49387, "bb_fold_acc": 39723, "gl_fold160": 59755}
RANDOM_CHAINS = 1 << 14
FOLD160_BRANCHES = {"fold160_neither", "fold160_c1_only_final_carry", "fold160_c1_only_no_final_carry",
                    "fold160_B_only_cl_borrows_final_carry", "fold160_B_only_cl_borrows_no_final_carry", "fold160_c1_and_B",
                    "fold160_cs", "fold160_bw"}
LENGTHS = {"length_%d" % n for n in (1, 2, 3, 4, 5, 16, 17, 123, 4096)}
EDGE_CHAINS = {"edge_all_largest_products", "edge_all_zero_products", "edge_alternating_products"}
MID_CHAIN = {"mid_chain_carry_fires", "mid_chain_carry_one_short"}
CENSUS = {
    "gl_fold_acc": {"target_limbs_l4_0", "target_limbs_l4_1", "target_limbs_l4_2", "target_limbs_l4_top", "target_0_mod_p",
                    "target_1_mod_p", "target_p_minus_1_mod_p", "target_listed_sum", "acc_carry_k0", "acc_carry_k1", "acc_carry_k2",
                    "acc_carry_k3"} | MID_CHAIN | EDGE_CHAINS | LENGTHS | FOLD160_BRANCHES
                   | {"mid_chain_%s_limbs_%d_%d" % (f, i, j) for f in ("fires", "short") for i in range(4) for j in range(i, 4)},
    "bb_fold_acc": {"target_words_hi_0", "target_words_hi_1", "target_words_hi_2", "target_words_hi_top", "target_0_mod_p",
                    "target_p_minus_1_mod_p", "target_finish_sums", "acc_carry_into_hi", "finish_mid_below_p", "finish_mid_in_p_2p",
                    "finish_mid_from_2p"} | MID_CHAIN | EDGE_CHAINS | LENGTHS
                   | {"finish_mid_%s_%s" % (m, a) for m in ("below_p", "in_p_2p", "from_2p")
                      for a in ("no_add_wraps", "first_add_wraps", "second_add_wraps", "both_adds_wrap")}
                   | {"mid_chain_%s_limbs_%d_%d" % (f, i, j) for f in ("fires", "short") for i in range(2) for j in range(i, 2)},
    "gl_fold160": FOLD160_BRANCHES,
}


def check_output(stdout):
    """every family with mismatches=0 on exactly the chains of CASES, 2^14 random chains per field, and every census class of the lists
    above present and not empty"""
    lines = {name: (int(n), int(m)) for name, n, m in re.findall(r"^(\w+) cases=(\d+) mismatches=(\d+)\b", stdout, re.M)}
    assert set(lines) == set(CASES), stdout[-4000:]
    for name, want in CASES.items():
        assert lines[name][1] == 0, stdout[-4000:]
        assert lines[name][0] == want, (name, lines[name])
    kinds = {name: (int(p), int(e), int(r)) for name, p, e, r in re.findall(r"^(\w+) chains: pulled=(\d+) edge=(\d+) random=(\d+)", stdout, re.M)}
    assert set(kinds) == {"gl_fold_acc", "bb_fold_acc"}
    for name, (pulled, edge, random) in kinds.items():
        assert random >= RANDOM_CHAINS and edge >= RANDOM_CHAINS and pulled > 0, (name, pulled, edge, random)
    census = {}
    for name, cls, n in re.findall(r"^census (\w+) (\w+)=(\d+)$", stdout, re.M):
        census.setdefault(name, {})[cls] = int(n)
    for name, classes in CENSUS.items():
        assert classes <= set(census.get(name, {})), (name, sorted(classes - set(census.get(name, {}))))
        empty = sorted(c for c, n in census[name].items() if n == 0)
        assert not empty, (name, empty)
    assert re.search(r"^total mismatches=0$", stdout, re.M), stdout[-2000:]


def test_fold_sums_match_exact_integers_on_pulled_back_edge_and_random_chains(tmp_path):
    shim = os.path.join(ROOT, "tests", "host_shim")
    clang = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
    if not os.path.exists(clang):
        pytest.skip("needs the ROCm clang++ as the host compiler")
    exe = tmp_path / "fold_acc"
    cmd = [clang, "-O2", "-std=c++17", "-pthread", "-include", os.path.join(shim, "shim.h"), "-I", shim,
           "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", str(exe), os.path.join(shim, "fold_acc.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-4000:] + out.stderr)
    check_output(out.stdout)
