"""What a salted proof costs, and what the seed saves: gb_prove_salted on the zero-knowledge dummy circuit (oracle/plonk_dummy.py),
both fields, 2^12, 2^16 and 2^20 rows.  Nothing here has a pass mark; the figures go into DESIGN.md sections 4 and 8.

    python tools/seeded_salts_times.py [--log-rows 12 16 20] [--reps 5] [--out profiles/seeded_salts_times.txt]
    python tools/seeded_salts_times.py --kernel-only [--reps 5]          (the run to put under a kernel trace)
    python tools/seeded_salts_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

Per field and size, wall time (host clock around calls that end in a synchronised read-back) of four legs, alternated in one
process, medians of --reps after one warm-up of each:
  * salted, page-locked   gb_prove_salted from a page-locked witness and page-locked host salts that are already in memory
  * salted + host draw    the same, with the draw of the [3][4][N] salts included: numpy's Generator.integers on one core (NOT the
                          reference's Rust RNG: a stand-in for "the host draws them"), written into the page-locked block
  * seeded                GB_SALTS_FROM_SEED: 32 bytes cross the bus, k_random_elements writes the columns
  * unsalted              gb_prove on the same circuit without zero_knowledge, for scale
--kernel-only: gb_random_elements into a device buffer of 12 * 2^23 Goldilocks elements (the salts of a 2^20-row, rate-3 proof)
and a plain fill of the same bytes (torch's fill_ kernel: one store per element, nothing computed), --reps times each - to be run under a kernel trace,
which has the kernels' own times; this mode prints only host-side event times for orientation.
--bench-parent: `python bench.py --gpus 1` in this tree and in a built checkout of the parent commit, alternated, each run a fresh
process - the headline path does not call the new code."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SEED = bytes(range(32))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def measure(ctx, F, tag, name, lg, reps, out):
    from oracle import plonk_dummy as D
    from oracle.fields import GL
    from plonky2_goldibear_amd import CircuitData
    ch = -(-100 // (F.order_bits - lg))                                   # circuit_builder.rs:1190-1192
    cfg = D.CircuitConfig(num_challenges=max(2, ch)) if F is GL else D.CircuitConfig.babybear(max(6, ch))
    circ = D.DummyCircuit(lg, cfg, F=F)
    kw = dict(num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants,
              num_challenges=cfg.num_challenges, arity_bits=cfg.arity_bits, field=tag)
    zk = CircuitData(ctx, lg, circ.constants_sigmas, circ.k_is, zero_knowledge=True, **kw)
    plain = CircuitData(ctx, lg, circ.constants_sigmas, circ.k_is, **kw)
    w = circ.witness(seed=lg)
    n_lde = circ.n << cfg.rate_bits
    pinned_w = ctx.host_alloc(w.shape, w.dtype)
    pinned_w[...] = w
    salts = ctx.host_alloc((3, 4, n_lde), w.dtype)
    rng = np.random.default_rng(lg)

    def draw():
        salts[...] = rng.integers(0, F.P, size=salts.shape, dtype=np.uint64).astype(w.dtype, copy=False)

    def salted_with_draw():
        draw()
        return zk.prove_once(pinned_w, salts=salts)

    draw()
    legs = (("salted, page-locked", lambda: zk.prove_once(pinned_w, salts=salts)),
            ("salted + host draw", salted_with_draw),
            ("seeded", lambda: zk.prove_once(pinned_w, seed=SEED)),
            ("unsalted", lambda: plain.prove_once(pinned_w)))
    # InvZeroPermArg (GB_ERR_PERM_ARG_ZERO; with a 31-bit field and 2^20 rows about one proof in five) depends on the challenges
    # and so on the salts: the warm-up looks for a witness every leg proves, and a timed run that hits it - the host-draw leg has
    # new salts every time - is left out and counted
    from plonky2_goldibear_amd import PermArgZeroError
    for attempt in range(16):
        try:
            sizes = [len(call()) for _, call in legs]                    # warm-up of every leg
            break
        except PermArgZeroError:
            zk.drop_retry()
            plain.drop_retry()
            pinned_w[...] = circ.witness(seed=1000 * (attempt + 1) + lg)
    else:
        raise RuntimeError("no witness found that every leg proves")
    wall = {k: [] for k, _ in legs}
    left_out = 0
    for _ in range(reps):
        for k, call in legs:
            t0 = time.perf_counter()
            try:
                call()
            except PermArgZeroError:
                zk.drop_retry()
                left_out += 1
                continue
            wall[k].append((time.perf_counter() - t0) * 1e3)
    lines = ["%s 2^%d rows, rate %d: salts [3][4][2^%d] = %.1f MB; proof %d bytes salted, %d unsalted" % (
        name, lg, cfg.rate_bits, lg + cfg.rate_bits, salts.nbytes / 1e6, sizes[0], sizes[3])]
    for k, _ in legs:
        lines.append("  %-20s median %9.3f ms   (all runs: %s)" % (k, median(wall[k]), " ".join("%.2f" % t for t in wall[k])))
    lines.append("  seeded - salted, page-locked = %+.3f ms; seeded - unsalted = %+.3f ms; host draw alone = %+.3f ms" % (
        median(wall["seeded"]) - median(wall["salted, page-locked"]), median(wall["seeded"]) - median(wall["unsalted"]),
        median(wall["salted + host draw"]) - median(wall["salted, page-locked"])))
    if left_out:
        lines.append("  (%d timed runs ended in InvZeroPermArg and are left out)" % left_out)
    append(out, lines)
    ctx.host_free(pinned_w)
    ctx.host_free(salts)
    zk.free()
    plain.free()
    ctx.trim()


def kernel_only(ctx, reps):
    import torch
    from plonky2_goldibear_amd import native as N, random_elements
    count = 12 << 23
    buf = torch.empty(count, dtype=torch.int64, device="cuda:%d" % ctx.device)
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        random_elements(ctx, N.GB_GOLDILOCKS, SEED, (1, 0, 0), 0, count, device=True)
        t1 = time.perf_counter()
        buf.fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print("gb_random_elements of %d Goldilocks elements (%.0f MB, allocation included) %.3f ms; fill of the same bytes %.3f ms" % (
            count, count * 8 / 1e6, (t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_salts_times.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--bench-parent", metavar="TREE")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=10)
    a = ap.parse_args()
    if a.bench_parent:     # (no GPU context in this process: the two trees' bench.py runs are its children)
        from gate_program_times import bench_parent
        return 0 if bench_parent(os.path.abspath(a.bench_parent), a.rounds, a.bench_steps, a.out) else 1
    from csrc_hash import csrc_sha16
    from oracle.fields import BB, GL
    from plonky2_goldibear_amd import GpuContext, native as N
    ctx = GpuContext(0)
    if a.kernel_only:
        kernel_only(ctx, a.reps)
        ctx.close()
        return 0
    append(a.out, ["# tools/seeded_salts_times.py, csrc %s, %s: zero-knowledge dummy circuit, wall times in ms" % (csrc_sha16(), time.strftime("%Y-%m-%d"))])
    for F, tag, name in ((GL, N.GB_GOLDILOCKS, "goldilocks"), (BB, N.GB_BABYBEAR, "babybear")):
        for lg in a.log_rows:
            measure(ctx, F, tag, name, lg, a.reps, a.out)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
