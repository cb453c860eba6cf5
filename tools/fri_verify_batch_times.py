"""What gb_fri_verify_batch costs beside a loop of gb_fri_verify, and what the general layout's tables cost beside the PLONK layout
of gb_verify_batch on the same proofs (include/goldibear_gpu.h), on two shapes, each described as a general instance: the
reference's own recursion proof (tests/golden, Goldilocks, 28 query rounds) and a proof of the BabyBear recursion-gates circuit
(tests/circuits.py).  Nothing here has a pass mark; the figures go into DESIGN.md section 8.  The method is tools/verify_batch_times.py's.

    python tools/fri_verify_batch_times.py [--sizes 1 64 512 2048] [--reps 5] [--out profiles/fri_verify_batch_times.txt]
    python tools/fri_verify_batch_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

Per shape and batch size, after one warm-up of every call that is timed, medians of --reps, the legs alternated in one process:
  * wall time (host clock; every call ends in its results) of a loop of gb_fri_verify on one thread and split over "copy_threads"
    threads, of gb_fri_verify_batch, and of gb_verify_batch on the whole proofs the FRI parts were taken from;
  * with profiling on, the scopes "upload / paths / queries" of both batch calls (HIP events, gb_ctx_scope_ms; sums over the
    chunks) and their ratios: the same device work through the tables in device memory and through the fixed layout.
Every item of a batch is its own copy in memory.
--bench-parent: `python bench.py --gpus 1` in this tree and in a built checkout of the parent commit, alternated, each run a fresh
process - the headline path does not call the new code."""
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

PARTS = ("upload", "paths", "queries")


def items(name, proof, owner):
    """the whole proof's FRI part as an item on the circuit's PLONK instance -> (field, instance, params, Item)"""
    import fri_batch_helpers as H
    from oracle import verifier as V
    from oracle.fields import BB, GL
    if name.startswith("goldilocks"):
        g = os.path.join(ROOT, "tests", "golden")
        rd = lambda n: open(os.path.join(g, n), "rb").read()
        cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
        vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
        return (GL,) + H.plonk_item(GL, cd, vd["circuit_digest"], vd["constants_sigmas_cap"], proof)[:3]
    from circuits import oracle_circuit
    oc = oracle_circuit(owner, len(owner.public_inputs))
    cap = [[int(x) for x in h] for h in np.asarray(owner.data.constants_sigmas_cap).reshape(-1, 8)]
    return (BB,) + H.plonk_item(BB, oc.common_data(), np.asarray(owner.data.circuit_digest), cap, proof)[:3]


def measure(ctx, lib, name, handle, proof, owner, sizes, reps, out):
    import fri_batch_helpers as H
    import fri_instances as FI
    from plonky2_goldibear_amd import native as N
    from plonky2_goldibear_amd.fri import _challenger_state, _flatten, _u32p
    from plonky2_goldibear_amd.prover import gb_challenger_state
    F, inst, params, item = items(name, proof, owner)
    fld = FI.field_tag(F)
    assert H.single(ctx.handle, fld, inst, params, item) == (N.GB_OK, ""), "the item does not verify alone"
    _, bsizes, polys = _flatten(inst, fld)
    nump, blind, arity = H.shape_arrays(inst, params)
    cs = _challenger_state(item.challenger, fld)[0]
    append(out, ["", "== %s: %d FriProof bytes of %d proof bytes, %d oracles, %d batches, %d polynomial entries" % (
        name, len(item.proof), len(proof), len(nump), len(bsizes), len(polys))])
    shape = (fld, params.degree_bits, params.config.rate_bits, params.config.cap_height, int(bool(params.hiding)), _u32p(nump), _u32p(blind), len(nump))
    tail = (_u32p(arity), len(arity), params.config.proof_of_work_bits, params.config.num_query_rounds)
    for n in sizes:
        copies = [item.copy(proof=bytes(bytearray(item.proof))) for _ in range(n)]
        fbufs = [np.frombuffer(bytearray(c.proof), dtype=np.uint8) for c in copies]
        tabs = [(C.c_void_p * n)(*[getattr(c, k).ctypes.data for c in copies]) for k in ("points", "openings", "caps")]
        fptrs = (C.c_void_p * n)(*[b.ctypes.data for b in fbufs])
        flens = (C.c_size_t * n)(*[len(item.proof)] * n)
        chs = (gb_challenger_state * n)(*[cs] * n)
        bufs = [np.frombuffer(bytearray(proof), dtype=np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (C.c_size_t * n)(*[len(proof)] * n)
        res = (N.gb_verify_result * n)()
        resp = C.cast(res, C.c_void_p)

        def loop(lo=0, hi=n):
            for i in range(lo, hi):
                st = lib.gb_fri_verify(None, *shape, tabs[0][i], _u32p(bsizes), len(bsizes), _u32p(polys), tabs[1][i], tabs[2][i], *tail,
                                       C.byref(chs[i]), fptrs[i], flens[i])
                assert st == N.GB_OK

        def threaded():
            k = min(COPY_THREADS, n)
            ts = [threading.Thread(target=loop, args=(n * t // k, n * (t + 1) // k)) for t in range(k)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()

        def fri_batch():
            st = lib.gb_fri_verify_batch(ctx.handle, *shape, _u32p(bsizes), len(bsizes), _u32p(polys), *tail, tabs[0], tabs[1], tabs[2],
                                         C.cast(chs, C.c_void_p), fptrs, flens, n, 0, resp)
            assert st == N.GB_OK, H.last_error(ctx.handle)

        def plonk_batch():
            assert lib.gb_verify_batch(ctx.handle, handle, ptrs, lens, n, 0, resp) == N.GB_OK

        legs = (("gb_fri_verify loop, 1 thread", loop), ("gb_fri_verify loop, %d threads" % COPY_THREADS, threaded),
                ("gb_fri_verify_batch", fri_batch), ("gb_verify_batch (whole proofs)", plonk_batch))
        times = {k: [] for k, _ in legs}
        for rep in range(reps + 1):   # the first round is the warm-up
            for k, fn in legs:
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: median(v[1:]) for k, v in times.items()}
        ctx.set_profiling(True)
        sc = {}
        for prefix, fn in (("fri verify batch", fri_batch), ("verify batch", plonk_batch)):   # alternated call by call below
            sc[prefix] = {p: [] for p in PARTS}
        for rep in range(reps + 1):
            for prefix, fn in (("fri verify batch", fri_batch), ("verify batch", plonk_batch)):
                ctx.scope_reset()
                fn()
                for p in PARTS:
                    sc[prefix][p].append(ctx.scope_ms("%s: %s" % (prefix, p))[0])
        ctx.set_profiling(False)
        ctx.scope_reset()
        m = {prefix: {p: median(v[1:]) for p, v in d.items()} for prefix, d in sc.items()}
        append(out, ["batch of %4d: " % n + "; ".join("%s %.3f ms" % (k, med[k]) for k, _ in legs),
                     "               per proof: " + "; ".join("%.1f us" % (med[k] * 1e3 / n) for k, _ in legs),
                     "               loop on 1 thread / gb_fri_verify_batch = %.1f, on %d threads / gb_fri_verify_batch = %.1f" % (
                         med[legs[0][0]] / med[legs[2][0]], COPY_THREADS, med[legs[1][0]] / med[legs[2][0]]),
                     "               scopes (ms) general / PLONK layout: " + "; ".join(
                         "%s %.3f / %.3f = %.2f" % (p, m["fri verify batch"][p], m["verify batch"][p],
                                                    m["fri verify batch"][p] / max(m["verify batch"][p], 1e-9)) for p in PARTS)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_verify_batch_times.txt"))
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
    append(a.out, ["gb_fri_verify_batch beside gb_fri_verify and gb_verify_batch: tools/fri_verify_batch_times.py --sizes %s --reps %d" % (
        " ".join(map(str, a.sizes)), a.reps),
                   "wall times: host clock, medians of %d after a warm-up, legs alternated; scopes: HIP events" % a.reps])
    keep = []
    for name, handle, proof, owner in shapes(ctx):
        keep.append(owner)
        measure(ctx, lib, name, handle, proof, owner, a.sizes, a.reps, a.out)
    for owner in keep:
        getattr(owner, "data", owner).free()
    ctx.close()


if __name__ == "__main__":
    main()
