"""csrc/verify_query.hpp - the checks of one FRI query round that gb_verify and the batch verifier's kernels share - compiled for
the CPU (tests/host_shim/verify_query.cpp) and run on word files derived from the reference's own recursion proof: the honest
proof and mutations of its query rounds, final polynomial and caps.  Per query round the verdict (which check fails first) equals
that of oracle/verifier.py's verify_fri on that round alone.  The program is built twice: plain, and as a stand-alone executable
under AddressSanitizer + UndefinedBehaviorSanitizer, which runs the same files.  CPU only; nothing is loaded into Python."""
import copy
import os
import subprocess

import numpy as np
import pytest

from oracle import verifier as V
from oracle.fields import GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
NONE = 2 ** 64 - 1


def _build(out, extra):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run([CLANG, "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim, "-I",
                    os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), os.path.join(shim, "verify_query.cpp"), "-o", str(out)] + extra,
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("verify_query")
    return (_build(d / "verify_query", ["-O2"]),
            _build(d / "verify_query_san", ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                            "-fno-omit-frame-pointer"]))


@pytest.fixture(scope="module")
def reference(golden_dir):
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    proof, pis = V.read_proof_with_pis(rd("recursive_verifier_gl_proof.bin"), cd)
    chal = V.get_challenges(proof, pis, vd["circuit_digest"], cd)   # the honest transcript: the per-round checks are given it
    return cd, vd, proof, chal


def _words(cd, vd, proof, chal):
    F = GL
    cfg, fp, fri = cd["config"], cd["fri_params"], proof["opening_proof"]
    c = cfg["num_challenges"]
    salt = V.SALT_SIZE if fp["hiding"] else 0
    widths = [cd["num_constants"] + cfg["num_routed_wires"], cfg["num_wires"], c * (1 + cd["num_partial_products"]),
              c * cd["quotient_degree_factor"]]
    row_widths = [widths[0]] + [w + salt for w in widths[1:]]
    bits = fp["reduction_arity_bits"]
    alpha = chal["fri_alpha"]
    _, batches = V.fri_instance(cd, chal["plonk_zeta"])
    openings = V.fri_openings(proof["openings"])
    w = [len(fri["query_round_proofs"]), fp["degree_bits"] + cfg["fri_config"]["rate_bits"], cfg["fri_config"]["cap_height"], len(bits),
         len(fri["final_poly"]), len(batches[0][1]), len(batches[1][1])] + widths + row_widths + list(bits)
    ext = lambda e: [int(x) for x in e]
    w += ext(alpha)
    for b in openings:
        w += ext(V.reduce_with_alpha(alpha, b)[0])
    for _, polys in batches:
        w += ext(F.epow(alpha, len(polys)))
    for point, _ in batches:
        w += ext(point)
    for b in chal["fri_betas"]:
        w += ext(b)
    for e in fri["final_poly"]:
        w += ext(e)
    w += [int(x) for x in chal["fri_query_indices"]]
    for cap in [vd["constants_sigmas_cap"], proof["wires_cap"], proof["zs_cap"], proof["quotient_cap"]] + fri["commit_phase_merkle_caps"]:
        w += [int(x) for h in cap for x in h]
    for rp in fri["query_round_proofs"]:
        for vals, path in rp["initial_trees_proof"]:
            w += [int(x) for x in vals] + [int(x) for h in path for x in h]
        for evals, path in rp["steps"]:
            w += [int(x) for e in evals for x in e] + [int(x) for h in path for x in h]
    return np.array(w, dtype=np.uint64)


def _oracle_verdicts(cd, vd, proof, chal):
    """verify_fri on each query round alone: the position (verify_query.hpp) of the check its assertion names, or NONE"""
    out = []
    caps = [vd["constants_sigmas_cap"], proof["wires_cap"], proof["zs_cap"], proof["quotient_cap"]]
    nl = len(cd["fri_params"]["reduction_arity_bits"])
    cd1 = copy.deepcopy(cd)
    cd1["config"]["fri_config"]["num_query_rounds"] = 1
    for x, rp in zip(chal["fri_query_indices"], proof["opening_proof"]["query_round_proofs"]):
        one = dict(proof, opening_proof=dict(proof["opening_proof"], query_round_proofs=[rp]))
        try:
            V.verify_fri(one, dict(chal, fri_query_indices=[x]), caps, cd1)
            out.append(NONE)
        except AssertionError as e:
            msg = str(e)
            if msg.startswith("initial Merkle path"):
                bad = [o for o, ((vals, path), cap) in enumerate(zip(rp["initial_trees_proof"], caps)) if not GL.merkle_verify(vals, x, cap, path)]
                out.append(bad[0])
            elif msg.startswith("FRI consistency"):
                out.append(4 + 2 * int(msg.split("layer ")[1].rstrip(")")))
            elif msg.startswith("FRI layer Merkle path"):
                # (the message carries no layer: the first layer whose path fails, every earlier check having passed)
                xi, layer = x, None
                for li, ab in enumerate(cd["fri_params"]["reduction_arity_bits"]):
                    evals, path = rp["steps"][li]
                    if not GL.merkle_verify([v for e in evals for v in e], xi >> ab, proof["opening_proof"]["commit_phase_merkle_caps"][li], path):
                        layer = li
                        break
                    xi >>= ab
                out.append(4 + 2 * layer + 1)
            else:
                assert msg.startswith("Final polynomial"), msg
                out.append(4 + 2 * nl)
    return out


def _bump(x):
    return (int(x) + 1) % V.P


def _mutations(proof):
    nqr = len(proof["opening_proof"]["query_round_proofs"])
    nl = len(proof["opening_proof"]["commit_phase_merkle_caps"])
    out = [("honest", proof)]

    def mutate(name, fn):
        p = copy.deepcopy(proof)
        fn(p["opening_proof"]["query_round_proofs"], p)
        out.append((name, p))

    for r in (0, nqr - 1):
        for o in range(4):
            def row(q, p, o=o):
                vals, path = q[r]["initial_trees_proof"][o]
                q[r]["initial_trees_proof"][o] = ([_bump(vals[0])] + list(vals[1:]), path)
            mutate("row %d/%d" % (r, o), row)

        def salt(q, p):
            vals, path = q[r]["initial_trees_proof"][1]
            q[r]["initial_trees_proof"][1] = (list(vals[:-1]) + [_bump(vals[-1])], path)
        mutate("salt %d" % r, salt)
        for level in (0, -1):
            def sib(q, p, level=level):
                vals, path = q[r]["initial_trees_proof"][2]
                path = [list(h) for h in path]
                path[level][3] = _bump(path[level][3])
                q[r]["initial_trees_proof"][2] = (vals, path)
            mutate("sibling %d/%d" % (r, level), sib)
        for li in (0, nl - 1):
            for k in (0, 5):   # (one of the coset's elements may be the one the query reads: consistency, else the layer's path)
                def step(q, p, li=li, k=k):
                    evals, path = q[r]["steps"][li]
                    evals = [tuple(e) for e in evals]
                    evals[k] = (evals[k][0], _bump(evals[k][1]))
                    q[r]["steps"][li] = (evals, path)
                mutate("step row %d/%d/%d" % (r, li, k), step)
            if len(proof["opening_proof"]["query_round_proofs"][r]["steps"][li][1]):
                def ssib(q, p, li=li):
                    evals, path = q[r]["steps"][li]
                    path = [list(h) for h in path]
                    path[0][0] = _bump(path[0][0])
                    q[r]["steps"][li] = (evals, path)
                mutate("step sibling %d/%d" % (r, li), ssib)

    def final(q, p):
        f = [tuple(e) for e in p["opening_proof"]["final_poly"]]
        f[1] = (_bump(f[1][0]), f[1][1])
        p["opening_proof"]["final_poly"] = f
    mutate("final polynomial", final)

    def layer_cap(q, p):
        caps = p["opening_proof"]["commit_phase_merkle_caps"]
        caps[nl - 1] = [[_bump(x) for x in h] for h in caps[nl - 1]]
    mutate("last layer's cap", layer_cap)

    def two(q, p):
        vals, path = q[nqr - 3]["initial_trees_proof"][0]
        q[nqr - 3]["initial_trees_proof"][0] = ([_bump(vals[0])] + list(vals[1:]), path)
        evals, path = q[5]["steps"][1]
        q[5]["steps"][1] = ([(e[0], _bump(e[1])) for e in evals], path)
    mutate("two rounds", two)
    return out


def _run(exe, tmp_path, words):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    words.tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    return [int(x) for x in np.fromfile(dst, dtype=np.uint64)]


def test_per_query_verdicts_equal_the_oracle_s(exes, reference, tmp_path):
    cd, vd, proof, chal = reference
    plain, sanitized = exes
    seen = set()
    for name, p in _mutations(proof):
        words = _words(cd, vd, p, chal)
        got = _run(plain, tmp_path, words)
        want = _oracle_verdicts(cd, vd, p, chal)
        assert got == want, name
        assert _run(sanitized, tmp_path, words) == want, name + " (sanitized build)"
        if name == "honest":
            assert set(got) == {NONE}
        else:
            assert set(got) != {NONE}, name
        seen |= set(got)
    nl = len(cd["fri_params"]["reduction_arity_bits"])
    # every kind of check has failed somewhere: the four oracles' paths, a consistency check, a layer's path, the final polynomial
    assert {0, 1, 2, 3, 4 + 2 * nl} <= seen and any(4 <= s < 4 + 2 * nl and s % 2 == 0 for s in seen) \
        and any(4 <= s < 4 + 2 * nl and s % 2 == 1 for s in seen)


def test_a_malformed_file_is_refused(exes, reference, tmp_path):
    cd, vd, proof, chal = reference
    words = _words(cd, vd, proof, chal)
    for exe in exes:
        for bad in (words[:-1], np.concatenate([words, words[:1]]), words[:3]):
            src = tmp_path / "bad.bin"
            bad.tofile(src)
            assert subprocess.run([exe, str(src), str(tmp_path / "o.bin")], capture_output=True, timeout=120).returncode == 3
