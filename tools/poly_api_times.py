#!/usr/bin/env python3
"""Times of the stand-alone entry points (gb_fft / gb_ifft / gb_lde, gb_merkle_tree_create) on device-resident data, next to the
commitment's own scopes at the same shape.  Recorded, not asserted: profiles/poly_api_times.txt.

  transforms   2^20 rows x 32 columns (Goldilocks) / x 64 columns (BabyBear): gb_fft rate 0 and 3, gb_ifft, gb_lde rate 3.
               Comparison: the "FFT + blinding" / "IFFT" scope of gb_commit_coeffs / gb_commit_values at that shape
               (gb_ctx_scope_ms) and a plain device-to-device copy of the output bytes.  Budget of a natural-order call: that
               scope plus TWO such copies - the extra pass moves every output element once in and once out.
  merkle       gb_merkle_tree_create from device leaves, 2^20 x 135 (Goldilocks) / x 167 (BabyBear), against the
               "build Merkle tree" scope of gb_commit_coeffs with log_n + rate_bits = 20 and that width, plus two copies of the leaves.

One process; every call is timed with device events on the context's stream after warm-up runs (median of --reps); every step runs
under its own time limit (--step-timeout seconds: the process ends there, nothing is started after an overrun).
    timeout -k 10 600 python tools/poly_api_times.py --out profiles/poly_api_times.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/poly_api_times.py --only goldilocks:fft_r3 --reps 1   (a run of its own)
    timeout -k 10 300 python tools/poly_api_times.py --fri      (the opening proof, see fri_openings; APPENDS to profiles/fri_instance_times.txt)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/poly_api_times.py --fri --only goldilocks:fri --reps 3
"""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LOG_N, RATE, CAP = 20, 3, 4
FIELDS = {"goldilocks": (0, 32, 135, np.int64, 0xFFFFFFFF00000001), "babybear": (1, 64, 167, np.int32, 0x78000001)}


def _overrun(signum, frame):
    sys.stderr.write("step ran past its time limit: stopping\n")
    os._exit(124)


FRI_SHAPES = {   # the benchmark's circuits: (field tag, wires, routed wires, challenges, FRI arity bits)
    "goldilocks": (0, 135, 80, 3, 4), "babybear": (1, 167, 41, 10, 3)}


def fri_openings(args, ctx, timed, rand, say):
    """--fri: the opening proof of the benchmark's FRI instance at 2^20 rows - four oracles of the circuit's widths over random
    device-resident columns (272 columns for Goldilocks) - through gb_prove_openings and through gb_fri_prove_openings with the
    same instance written out as oracles and batches; both give the same bytes.  --only FIELD:fri runs the general call alone."""
    from oracle.fields import BB, GL
    from plonky2_goldibear_amd import CircuitData, PolynomialBatch, prove_openings
    from plonky2_goldibear_amd.fri import FriBatchInfo, FriConfig, FriInstanceInfo, FriOracleInfo, FriParams, FriPolynomialInfo
    say("fri openings  2^%d rows, rate %d, cap %d, device-resident oracles; reps %d (median), warm-up %d" % (LOG_N, RATE, CAP, args.reps, args.warmup))
    for name, (tag, nw, nr, nch, ab) in FRI_SHAPES.items():
        want = args.only.split(":") if args.only else None
        if want and want[0] != name:
            continue
        _, _, _, idt, p = FIELDS[name]
        n, d, w = 1 << LOG_N, (2, 4)[tag], (12, 16)[tag]
        widths = [1 + 2 + nr, nw, nch * -(-nr // 8), nch * 8]
        k_is = np.array([7 * i % p for i in range(1, nr + 1)], dtype=np.uint64 if tag == 0 else np.uint32)
        gpu = CircuitData(ctx, LOG_N, rand((widths[0], n), idt, p), k_is, num_wires=nw, num_routed_wires=nr, num_challenges=nch,
                          arity_bits=ab, field=tag)
        oracles = [gpu.constants_sigmas_commitment] + [
            (PolynomialBatch.from_coeffs if i == 3 else PolynomialBatch.from_values)(ctx, rand((widths[i], n), idt, p), RATE, CAP, field=tag)
            for i in (1, 2, 3)]
        zeta = [0x9E3779B1 * i % p for i in range(3, 3 + d)]
        zeta_next = [int(x) * (GL, BB)[tag].two_adic_generator(LOG_N) % p for x in zeta]   # g zeta
        every = [q for i in range(4) for q in FriPolynomialInfo.from_range(i, range(widths[i]))]
        inst = FriInstanceInfo([FriOracleInfo(x, False) for x in widths],
                               [FriBatchInfo(zeta, every), FriBatchInfo(zeta_next, FriPolynomialInfo.from_range(2, range(nch)))])
        params = FriParams(FriConfig(RATE, CAP, 16, 28), False, LOG_N, gpu.reduction_arity_bits)
        chal = ([5] * w, [], [])
        general = lambda: prove_openings(inst, oracles, chal, params)
        if want:
            for _ in range(args.reps):
                general()
            ctx.synchronize()
            return
        plonk = lambda: gpu.prove_openings(oracles[1], oracles[2], oracles[3], zeta, chal)
        same = general()[0] == plonk()[0]
        tg, tp = timed(general), timed(plonk)
        cols = sum(widths)
        say("%s  %d columns in 4 oracles: gb_prove_openings %.3f ms, gb_fri_prove_openings %.3f ms, same bytes: %s" % (name, cols, tp, tg, same))
        nbytes = cols * n * (8, 4)[tag] + 2 * n * d * (8, 4)[tag]   # every column once, two slots written
        say("%s  k_reduce_batches expected traffic %.2f GB = %.3f ms at 5.4 TB/s" % (name, nbytes / 1e9, nbytes / 5.4e9))
        for b in oracles[1:]:
            b.free()
        gpu.free()
        ctx.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/poly_api_times.txt (rewritten); with --fri profiles/fri_instance_times.txt (appended to)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--only", default=None, help="FIELD:STEP - run one step (for a profiler run); nothing is written")
    ap.add_argument("--fri", action="store_true", help="time gb_fri_prove_openings next to gb_prove_openings instead (see fri_openings)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fri_instance_times.txt" if args.fri else "poly_api_times.txt")

    import torch
    from csrc_hash import csrc_sha16
    from plonky2_goldibear_amd import GpuContext, MerkleTree, PolynomialBatch
    from plonky2_goldibear_amd import polynomial as P
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured here")
    signal.signal(signal.SIGALRM, _overrun)
    ctx = GpuContext(0)
    stream = torch.cuda.ExternalStream(ctx.stream)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """median milliseconds of fn() on the context's stream, device events, after warm-up"""
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        signal.alarm(0)
        return statistics.median(ms)

    def scope(commit, names):
        """the commitment's scopes at the same shape: milliseconds per commit, median over reps"""
        signal.alarm(args.step_timeout)
        for _ in range(args.warmup):
            commit().free()
        ctx.set_profiling(True)
        per = {n: [] for n in names}
        for _ in range(args.reps):
            ctx.scope_reset()
            commit().free()
            for n in names:
                per[n].append(ctx.scope_ms(n)[0])
        ctx.set_profiling(False)
        ctx.scope_reset()
        signal.alarm(0)
        return {n: statistics.median(v) for n, v in per.items()}

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def run():
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)      # contiguous, same type: one device-to-device hipMemcpyAsync
        return timed(run)

    def rand(shape, idt, p):
        g = torch.Generator(device="cuda").manual_seed(1)
        return (torch.randint(0, min(p, 1 << 62), shape, generator=g, device="cuda", dtype=torch.int64) % p).to(
            torch.int64 if idt == np.int64 else torch.int32)

    if args.fri:
        fri_openings(args, ctx, timed, rand, say)
        if not args.only:
            with open(args.out, "a") as f:   # next to the alternation's figures, which stay
                f.write("\n" + "\n".join(lines) + "\n")
        ctx.close()
        return
    say("poly_api_times  csrc %s  reps %d (median), warm-up %d, device events on the context's stream" % (csrc_sha16(), args.reps, args.warmup))
    for name, (tag, ncols, width, idt, p) in FIELDS.items():
        n = 1 << LOG_N
        want = args.only.split(":") if args.only else None
        if want and want[0] != name:
            continue
        x = rand((ncols, n), idt, p)
        out0, out3 = torch.empty_like(x), torch.empty((ncols, n << RATE), dtype=x.dtype, device="cuda")
        steps = {
            "fft_r0": lambda: P.fft(ctx, x, 0, field=tag, out=out0),
            "fft_r3": lambda: P.fft(ctx, x, RATE, field=tag, out=out3),
            "ifft": lambda: P.ifft(ctx, x, field=tag, out=out0),
            "lde_r3": lambda: P.lde(ctx, x, RATE, field=tag, out=out3),
        }
        leaves = None

        def tree():
            MerkleTree.new(ctx, leaves, CAP, field=tag).free()
        steps["merkle_tree_create"] = tree
        if want:
            if want[1] == "merkle_tree_create":
                leaves = rand((n, width), idt, p)
            for _ in range(args.reps):
                steps[want[1]]()
            ctx.synchronize()
            return
        t = {k: timed(f) for k, f in steps.items() if k != "merkle_tree_create"}
        c0, c3 = copy_ms(out0.numel() * out0.element_size()), copy_ms(out3.numel() * out3.element_size())
        s0 = scope(lambda: PolynomialBatch.from_coeffs(ctx, x, 0, CAP, field=tag), ["FFT + blinding"])
        s3 = scope(lambda: PolynomialBatch.from_coeffs(ctx, x, RATE, CAP, field=tag), ["FFT + blinding"])
        sv = scope(lambda: PolynomialBatch.from_values(ctx, x, RATE, CAP, field=tag), ["IFFT", "FFT + blinding"])
        say("")
        say("%s  2^%d rows x %d columns, device-resident" % (name, LOG_N, ncols))
        say("  %-22s %9s   %s" % ("call", "ms", "comparison: commitment scope + 2 x device-to-device copy of the output = budget"))

        def row(call, ms, what, sc, cp):
            budget = sc + 2 * cp
            say("  %-22s %9.3f   %s %.3f + 2 x %.3f = %.3f   %s" % (call, ms, what, sc, cp, budget, "within" if ms <= budget else "OVER"))
        row("gb_fft rate 0", t["fft_r0"], '"FFT + blinding"', s0["FFT + blinding"], c0)
        row("gb_fft rate 3", t["fft_r3"], '"FFT + blinding"', s3["FFT + blinding"], c3)
        row("gb_ifft", t["ifft"], '"IFFT"', sv["IFFT"], c0)
        row("gb_lde rate 3", t["lde_r3"], '"IFFT" + "FFT + blinding"', sv["IFFT"] + sv["FFT + blinding"], c3)
        del out0, out3, x
        leaves = rand((n, width), idt, p)
        tm = timed(tree)
        cl = copy_ms(leaves.numel() * leaves.element_size())
        cw = rand((width, 1 << (LOG_N - RATE)), idt, p)
        sm = scope(lambda: PolynomialBatch.from_coeffs(ctx, cw, RATE, CAP, field=tag), ["build Merkle tree"])
        say("%s  2^%d leaves x %d, device leaves" % (name, LOG_N, width))
        row("gb_merkle_tree_create", tm, '"build Merkle tree" (2^%d rows, rate %d)' % (LOG_N - RATE, RATE), sm["build Merkle tree"], cl)
        del leaves, cw
        ctx.trim()
    if not args.only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
