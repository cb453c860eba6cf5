"""What gb_verify_compressed_batch costs beside what a holder of compressed proofs could do without it (include/goldibear_gpu.h), on
the two shapes of tools/verify_batch_times.py: the reference's own recursion proof and a proof of the BabyBear recursion-gates
circuit, both compressed by gb_proof_compress.  Nothing here has a pass mark; the figures go into DESIGN.md section 8.

    python tools/verify_compressed_batch_times.py [--sizes 1 8 64 512 2048] [--reps 5] [--out profiles/verify_compressed_batch_times.txt]
    python tools/verify_compressed_batch_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

Per shape and batch size, one session, after one warm-up of every call that is timed, medians of --reps, the legs alternated in one
process; wall times are the host clock's and every call ends in its result:
  1. a loop of gb_verify_compressed, on one thread and split over "copy_threads" threads;
  2. gb_proof_decompress per proof on "copy_threads" threads, then one gb_verify_batch of the results;
  3. gb_verify_compressed_batch - and, with profiling on, its scopes (HIP events, gb_ctx_scope_ms; sums over the chunks) and the
     wall time of the call less those as the host stage's share;
  4. for scale, gb_verify_batch on proofs that are decompressed already.
Every proof of a batch is its own copy in memory.
--bench-parent: as tools/verify_batch_times.py - the headline path does not call the new code."""
import argparse
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from verify_batch_times import COPY_THREADS, append, bench_value, median, shapes  # noqa: E402

SCOPES = ("verify compressed batch: upload", "verify compressed batch: queries", "verify compressed batch: paths")


def copies(data, n):
    bufs = [np.frombuffer(bytearray(data), dtype=np.uint8) for _ in range(n)]
    return bufs, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[len(data)] * n)


def measure(ctx, lib, name, handle, proof, small, sizes, reps, out):
    from plonky2_goldibear_amd import native as N
    append(out, ["", "== %s: %d proof bytes, %d compressed" % (name, len(proof), len(small))])
    for n in sizes:
        keep_c, cptrs, clens = copies(small, n)
        keep_p, pptrs, plens = copies(proof, n)
        res = (N.gb_verify_result * n)()
        resp = C.cast(res, C.c_void_p)
        outs = [np.empty(len(proof) + 64, dtype=np.uint8) for _ in range(n)]
        optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        olens = (C.c_size_t * n)()

        def split(fn):
            k = min(COPY_THREADS, n)
            ts = [threading.Thread(target=fn, args=(n * t // k, n * (t + 1) // k)) for t in range(k)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()

        def loop(lo=0, hi=n):
            for i in range(lo, hi):
                assert lib.gb_verify_compressed(handle, cptrs[i], clens[i]) == N.GB_OK

        def decompress(lo, hi):
            for i in range(lo, hi):
                got = C.c_size_t()
                assert lib.gb_proof_decompress(handle, cptrs[i], clens[i], optrs[i], outs[i].size, C.byref(got)) == N.GB_OK
                olens[i] = got.value

        def decompress_then_batch():
            split(decompress)
            assert lib.gb_verify_batch(ctx.handle, handle, optrs, olens, n, 0, resp) == N.GB_OK

        def compressed_batch():
            assert lib.gb_verify_compressed_batch(ctx.handle, handle, cptrs, clens, n, 0, resp) == N.GB_OK

        def plain_batch():
            assert lib.gb_verify_batch(ctx.handle, handle, pptrs, plens, n, 0, resp) == N.GB_OK

        legs = (("1. gb_verify_compressed loop, 1 thread", loop),
                ("1. gb_verify_compressed loop, %d threads" % COPY_THREADS, lambda: split(loop)),
                ("2. gb_proof_decompress on %d threads + gb_verify_batch" % COPY_THREADS, decompress_then_batch),
                ("3. gb_verify_compressed_batch", compressed_batch),
                ("4. gb_verify_batch of decompressed proofs", plain_batch))
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
            compressed_batch()
            walls.append((time.perf_counter() - t0) * 1e3)
            for s in SCOPES:
                scope[s].append(ctx.scope_ms(s)[0])
        ctx.set_profiling(False)
        ctx.scope_reset()
        sc = {s: median(v[1:]) for s, v in scope.items()}
        wall = median(walls[1:])
        dev = sum(sc.values())
        three, four = med[legs[3][0]], med[legs[4][0]]
        append(out, ["batch of %4d:" % n] +
               ["    %-58s %10.3f ms  %9.1f us per proof" % (k, med[k], med[k] * 1e3 / n) for k, _ in legs] +
               ["    leg 3 / leg 4 = %.2f; leg 3 against the faster of legs 1 and 2: %.2fx" % (
                   three / four, min(med[legs[1][0]], med[legs[0][0]], med[legs[2][0]]) / three),
                "    profiled call %.3f ms: " % wall + "; ".join("%s %.3f" % (s.split(": ")[1], sc[s]) for s in SCOPES) +
                "; the call less these (host stage not hidden behind kernels) %.3f ms = %.0f %%" % (wall - dev, 100 * (wall - dev) / wall)])
        del keep_c, keep_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_compressed_batch_times.txt"))
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
    append(a.out, ["gb_verify_compressed_batch beside the host's ways: tools/verify_compressed_batch_times.py --sizes %s --reps %d" % (
                       " ".join(map(str, a.sizes)), a.reps),
                   "wall times: host clock, medians of %d after a warm-up, legs alternated in one process; scopes: HIP events" % a.reps])
    keep = []
    for name, handle, proof, owner in shapes(ctx):
        keep.append(owner)
        small = getattr(owner, "data", owner).compress(proof)
        measure(ctx, lib, name, handle, proof, small, a.sizes, a.reps, a.out)
    for owner in keep:
        getattr(owner, "data", owner).free()
    ctx.close()


if __name__ == "__main__":
    main()
