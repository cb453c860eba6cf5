"""What gb_verify_batch costs beside a loop of gb_verify (include/goldibear_gpu.h), on two shapes: the reference's own recursion
proof (tests/golden, Goldilocks, 28 query rounds, salted, three FRI layers) and a proof of the BabyBear recursion-gates circuit
(tests/circuits.py).  Nothing here has a pass mark; the figures go into DESIGN.md section 8.

    python tools/verify_batch_times.py [--sizes 1 8 64 512 2048] [--reps 5] [--out profiles/verify_batch_times.txt]
    python tools/verify_batch_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

Per shape and batch size, after one warm-up of every call that is timed, medians of --reps, the legs alternated in one process:
  * wall time (host clock; every call ends in its result) of a loop of gb_verify on one thread, of the same loop split over
    "copy_threads" threads (the fair comparison: the batch's host stage uses those threads), and of gb_verify_batch with the
    default "verify_chunk_bytes" and with one chunk for the whole batch (no chunk's host stage beside another's kernels);
  * with profiling on, the scopes "verify batch: upload / paths / queries" (HIP events, gb_ctx_scope_ms; sums over the chunks)
    and the wall time of the call less those as the host stage's share.
Every proof of a batch is its own copy in memory.
--bench-parent: `python bench.py --gpus 1` in this tree and in a built checkout of the parent commit, alternated, each run a fresh
process - the headline path does not call the new code."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SCOPES = ("verify batch: upload", "verify batch: paths", "verify batch: queries")
COPY_THREADS = 4   # the context's default


def median(xs):
    return sorted(xs)[len(xs) // 2]


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def shapes(ctx):
    from oracle import verifier as V
    from plonky2_goldibear_amd import VerifierCircuitData, native as N
    from circuits import recursion_gates_circuit
    g = os.path.join(ROOT, "tests", "golden")
    rd = lambda n: open(os.path.join(g, n), "rb").read()
    common = rd("recursive_verifier_gl_common_data.bin")
    cd, vd = V.read_common_data(common), V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    cfg, fc = cd["config"], cd["config"]["fri_config"]
    nsel = len(cd["selectors_info"]["groups"])
    circ = VerifierCircuitData(cd["fri_params"]["degree_bits"], V.read_gates(common, cd), np.array(cd["k_is"], dtype=np.uint64),
                               np.array(vd["constants_sigmas_cap"], dtype=np.uint64), np.array(vd["circuit_digest"], dtype=np.uint64),
                               num_wires=cfg["num_wires"], num_routed_wires=cfg["num_routed_wires"],
                               num_constants=cd["num_constants"] - nsel, num_challenges=cfg["num_challenges"],
                               max_quotient_degree_factor=cd["quotient_degree_factor"], rate_bits=fc["rate_bits"],
                               cap_height=fc["cap_height"], proof_of_work_bits=fc["proof_of_work_bits"],
                               num_query_rounds=fc["num_query_rounds"], arity_bits=4, final_poly_bits=5, num_selectors=nsel,
                               zero_knowledge=cd["fri_params"]["hiding"], num_public_inputs=cd["num_public_inputs"])
    yield "goldilocks, the reference's recursion proof", circ.handle, rd("recursive_verifier_gl_proof.bin"), circ
    b, pw, _ = recursion_gates_circuit(N.GB_BABYBEAR, seed=11, public_inputs=True)
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    proof = c.data.prove(w, pis, random_wire=(c.random_wire[1], c.random_wire[0]))
    yield "babybear, recursion-gates circuit", c.data.handle, proof, c


def measure(ctx, lib, name, handle, proof, sizes, reps, out):
    from plonky2_goldibear_amd import native as N
    append(out, ["", "== %s: %d proof bytes" % (name, len(proof))])
    for n in sizes:
        bufs = [np.frombuffer(bytearray(proof), dtype=np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_size_t * n)(*[len(proof)] * n)
        res = (N.gb_verify_result * n)()
        resp = C.cast(res, C.c_void_p)

        def loop(lo=0, hi=n):
            for i in range(lo, hi):
                assert lib.gb_verify(handle, ptrs[i], lens[i]) == N.GB_OK

        def threaded():
            k = min(COPY_THREADS, n)
            ts = [threading.Thread(target=loop, args=(n * t // k, n * (t + 1) // k)) for t in range(k)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()

        def batch():
            assert lib.gb_verify_batch(ctx.handle, handle, ptrs, lens, n, 0, resp) == N.GB_OK

        def one_chunk():
            ctx.set_option("verify_chunk_bytes", 1 << 30)
            try:
                batch()
            finally:
                ctx.set_option("verify_chunk_bytes", 8 << 20)

        legs = (("gb_verify loop, 1 thread", loop), ("gb_verify loop, %d threads" % COPY_THREADS, threaded),
                ("gb_verify_batch", batch), ("gb_verify_batch, one chunk", one_chunk))
        times = {k: [] for k, _ in legs}
        for rep in range(reps + 1):   # the first round is the warm-up
            for k, fn in legs:
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: median(v[1:]) for k, v in times.items()}
        ctx.set_profiling(True)
        scope = {s: [] for s in SCOPES}
        walls = []
        for rep in range(reps + 1):
            ctx.scope_reset()
            t0 = time.perf_counter()
            batch()
            walls.append((time.perf_counter() - t0) * 1e3)
            for s in SCOPES:
                scope[s].append(ctx.scope_ms(s)[0])
        ctx.set_profiling(False)
        ctx.scope_reset()
        sc = {s: median(v[1:]) for s, v in scope.items()}
        wall = median(walls[1:])
        dev = sum(sc.values())
        append(out, ["batch of %4d: " % n + "; ".join("%s %.3f ms" % (k, med[k]) for k, _ in legs),
                     "               per proof: " + "; ".join("%.1f us" % (med[k] * 1e3 / n) for k, _ in legs),
                     "               profiled call %.3f ms: " % wall + "; ".join("%s %.3f" % (s.split(": ")[1], sc[s]) for s in SCOPES) +
                     "; the call less these (host stage not hidden behind kernels) %.3f ms = %.0f %%" % (wall - dev, 100 * (wall - dev) / wall)])


def bench_value(tree, steps):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2"], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_times.txt"))
    ap.add_argument("--bench-parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=10)
    a = ap.parse_args()
    if a.bench_parent:
        vals = {"parent": [], "this": []}
        for _ in range(a.rounds):
            vals["parent"].append(bench_value(a.bench_parent, a.bench_steps))
            vals["this"].append(bench_value(ROOT, a.bench_steps))
        append(a.out, ["", "== bench.py --gpus 1 --steps %d --warmup 2, `value` (proofs/s), alternated, each run a fresh process" % a.bench_steps,
                       "parent commit: " + " / ".join("%.3f" % v for v in vals["parent"]),
                       "this commit:   " + " / ".join("%.3f" % v for v in vals["this"])])
        return
    from plonky2_goldibear_amd import GpuContext, native as N
    lib = N.load()
    ctx = GpuContext(0)
    append(a.out, ["gb_verify_batch beside gb_verify: tools/verify_batch_times.py --sizes %s --reps %d" % (" ".join(map(str, a.sizes)), a.reps),
                   "wall times: host clock, medians of %d after a warm-up, legs alternated; scopes: HIP events" % a.reps])
    keep = []
    for name, handle, proof, owner in shapes(ctx):
        keep.append(owner)
        measure(ctx, lib, name, handle, proof, a.sizes, a.reps, a.out)
    for owner in keep:
        getattr(owner, "data", owner).free()
    ctx.close()


if __name__ == "__main__":
    main()
