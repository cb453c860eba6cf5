"""What gb_constraint_quotient costs (include/goldibear_gpu.h, "constraint systems over committed oracles"), on two systems and two
sizes per field, next to the quotient stage of a program-gate circuit timed in the same session.  Nothing here has a pass mark;
the figures go into DESIGN.md sections 4 and 8.  The method is tools/verify_batch_times.py's: HIP events for the scopes
(gb_ctx_scope_ms), medians of --reps after a warm-up, one session.

    python tools/constraint_quotient_times.py [--log-rows 14 20] [--reps 5] [--out profiles/constraint_quotient_times.txt]

Systems (device-resident oracles, chunks written to a device block):
  * fibonacci: one oracle of 2 columns, 4 constraints (tests/constraint_cases.py), quotient_degree_bits 1;
  * wide: two oracles of 50 columns, 50 constraints of degree 3 in two programs (250 instructions, 200 cells) -
    a_i(x) b_i(x) a_(i+1)(w x) - b_(7i)(x) gamma - quotient_degree_bits 2.
Per system: the scopes "constraint quotient: values" (the L_0 table when a program reads it, and k_constraint_quotient) and
"constraint quotient: IFFT", the wall time of the call, and values-scope time per point and per interpreted instruction.
The program-gate circuit is tools/gate_program_times.py's (the recursion gate set with its short gates as programs), at the
smaller size only: its scope "compute quotient polys" covers k_gate_constraints, k_gate_programs, k_quotient and the same tail."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from verify_batch_times import append, median  # noqa: E402

RATE_BITS, NCH = 2, 2
WIDE_COLS = 50


def systems(F, tag, degree_bits):
    import constraint_cases as CC
    from plonky2_goldibear_amd.constraints import ConstraintProgram
    fib = ConstraintProgram.from_constraints(CC.fibonacci_constraints(F, degree_bits), cells=CC.FIB_CELLS, num_params=2, field=tag)

    def half(lo):
        idx = list(range(lo, lo + WIDE_COLS // 2))
        cells = [(0, i, 0) for i in idx] + [(1, i, 0) for i in idx] + [(0, (i + 1) % WIDE_COLS, 1) for i in idx] + [(1, 7 * i % WIDE_COLS, 0) for i in idx]
        k = len(idx)
        return ConstraintProgram.from_constraints(
            lambda cell, param, x, l_first, l_last: [cell[j] * cell[k + j] * cell[2 * k + j] - cell[3 * k + j] * param[0] for j in range(k)],
            cells=cells, num_params=2, field=tag)
    return {"fibonacci": ([fib], [2], 1), "wide": ([half(0), half(WIDE_COLS // 2)], [WIDE_COLS, WIDE_COLS], 2)}


def random_columns(F, ctx, cols, n, seed):
    """device-resident canonical values (what a prover that keeps its trace on the device hands over)"""
    import torch
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, F.P, size=(cols, n), dtype=np.uint64).astype(F.dtype)
    return torch.from_numpy(vals.view(np.int64 if F.elem_bytes == 8 else np.int32)).to("cuda:%d" % ctx.device)


def measure(ctx, F, tag, degree_bits, reps, out):
    from plonky2_goldibear_amd import PolynomialBatch
    from plonky2_goldibear_amd.constraints import constraint_quotient
    n = 1 << degree_bits
    for name, (programs, widths, qb) in systems(F, tag, degree_bits).items():
        oracles = [PolynomialBatch.from_values(ctx, random_columns(F, ctx, w, n, 5 + o), RATE_BITS, 4, field=tag) for o, w in enumerate(widths)]
        params, alphas = [3, 5], [int(x) for x in F.fill(1, NCH)]
        instrs = sum(p.num_instrs for p in programs)
        vals, ifft, wall = [], [], []
        for rep in range(reps + 1):   # the first round is the warm-up
            ctx.scope_reset()
            t0 = time.perf_counter()
            constraint_quotient(ctx, oracles, programs, params, alphas, qb, device=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            vals.append(ctx.scope_ms("constraint quotient: values")[0])
            ifft.append(ctx.scope_ms("constraint quotient: IFFT")[0])
        v, i, w = median(vals[1:]), median(ifft[1:]), median(wall[1:])
        points = n << qb
        append(out, ["%-10s %-9s 2^%d rows, qb %d, %d challenges, %d columns, %d constraints, %d instructions, %d cells: "
                     "values %.3f ms, IFFT %.3f ms, call %.3f ms; values per point %.2f ns, per point and instruction %.1f ps" % (
                         F.name, name, degree_bits, qb, NCH, sum(widths), sum(p.num_constraints for p in programs), instrs,
                         sum(p.num_cells for p in programs), v, i, w, v * 1e6 / points, v * 1e9 / points / instrs)])
        for b in oracles:
            b.free()
        ctx.trim()


def program_gate_circuit(ctx, F, tag, log_rows, reps, out):
    """tools/gate_program_times.py's circuit with its short gates as programs: the scope "compute quotient polys" of prove()"""
    import gate_programs as GP
    from circuits import recursion_gates_circuit
    from plonky2_goldibear_amd.circuit_builder import NoopGate
    b, pw, _ = recursion_gates_circuit(tag, seed=9)
    while b.num_gates() < (1 << log_rows) - 64:
        b.add_gate(NoopGate())
    GP.with_program_gates(b)
    progs = [g.program for g in b.gates if hasattr(g, "program")]
    c = b.build(ctx)
    w, pis = c.generate_witness(pw)
    ms = []
    for rep in range(reps + 1):
        ctx.scope_reset()
        c.data.prove(w.copy(), pis, random_wire=(c.random_wire[1], c.random_wire[0]))
        ms.append(ctx.scope_ms("compute quotient polys")[0])
    cfg = c.data.cfg
    points = (1 << c.degree_bits) * cfg.max_quotient_degree_factor
    instrs = sum(p.num_instrs for p in progs)
    m = median(ms[1:])
    append(out, ["%-10s program-gate circuit 2^%d rows, quotient degree factor %d, %d challenges, %d program gates, %d instructions: "
                 "compute quotient polys %.3f ms (all gate kernels, k_quotient and the tail); per point %.2f ns, per point and "
                 "interpreted instruction at most %.1f ps" % (F.name, c.degree_bits, cfg.max_quotient_degree_factor, cfg.num_challenges,
                                                              len(progs), instrs, m, m * 1e6 / points, m * 1e9 / points / max(instrs, 1))])
    c.data.free()
    ctx.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[14, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_quotient_times.txt"))
    a = ap.parse_args()
    from oracle.fields import BB, GL
    from plonky2_goldibear_amd import GpuContext, native as N
    ctx = GpuContext(0)
    ctx.set_profiling(True)
    append(a.out, ["gb_constraint_quotient: tools/constraint_quotient_times.py --log-rows %s --reps %d" % (" ".join(map(str, a.log_rows)), a.reps),
                   "scopes: HIP events, medians of %d after a warm-up, one session; oracles at rate_bits %d, device-resident; chunks to a device block" % (
                       a.reps, RATE_BITS)])
    for F, tag in ((GL, N.GB_GOLDILOCKS), (BB, N.GB_BABYBEAR)):
        for lg in a.log_rows:
            measure(ctx, F, tag, lg, a.reps, a.out)
        program_gate_circuit(ctx, F, tag, min(a.log_rows), a.reps, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
