"""What interpreting a gate costs: the "compute quotient polys" scope (gb_ctx_scope_ms) of the recursion gate-set circuit
(tests/circuits.py recursion_gates_circuit) padded to 2^14 rows, with the built-in evaluators of csrc/gates.hpp against the same
gates as constraint programs (tests/gate_programs.py; GB_GATE_PROGRAM, k_gate_programs), both fields, alternated three times in
one process after a warm-up.  There is no pass mark: the compiled evaluators win; the ratio goes into DESIGN.md section 4.

    python tools/gate_program_times.py [--log-rows 14] [--rounds 3] [--out profiles/gate_program_times.txt]
    python tools/gate_program_times.py --once programs|builtin --field 0|1    # two proofs of one form, for a profiler run
    python tools/gate_program_times.py --kernel-stats DIR/p_kernel_stats.csv --label "programs goldilocks"
    python tools/gate_program_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

The kernel times (k_gate_programs / k_gate_constraints_tiled) come from a kernel-trace run of its own of the --once mode
(rocprofv3 --kernel-trace --stats -d DIR -o p -- python tools/gate_program_times.py --once programs); --kernel-stats copies the
gate kernels' rows of its statistics into the output file (tools/rocpd_kernel_stats.py makes the CSV from the profiler's
database); the SQ counters recorded beside them are `rocprofv3 --pmc ... --kernel-include-regex k_gate_programs` runs of the same
--once mode, one run per counter set and never together with tracing, summarised by tools/pmc_sq_summary.py.  --bench-parent runs `python bench.py --gpus 1` in this tree and in a
built checkout of the parent commit, alternated, each run a fresh process, and records `value` of every run: the headline
circuit has no program gates, so this commit's values must lie inside the spread of the parent's runs of the same session."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from plonky2_goldibear_amd import GpuContext, native as N   # noqa: E402
from plonky2_goldibear_amd.circuit_builder import NoopGate    # noqa: E402

SCOPE = "compute quotient polys"


def circuit(ctx, field, log_rows, programs):
    import gate_programs as GP
    from circuits import recursion_gates_circuit
    b, pw, _ = recursion_gates_circuit(field, seed=9)
    while b.num_gates() < (1 << log_rows) - 64:   # build() adds the hash, public-input and constant rows and pads to 2^log_rows
        b.add_gate(NoopGate())
    if programs:
        GP.with_program_gates(b)
    c = b.build(ctx)
    assert c.degree_bits == log_rows, c.degree_bits
    w, pis = c.generate_witness(pw)
    return c, w, pis


def quotient_ms(ctx, c, w, pis):
    ctx.scope_reset()
    proof = c.data.prove(w.copy(), pis, random_wire=(c.random_wire[1], c.random_wire[0]))
    ms, count = ctx.scope_ms(SCOPE)
    assert count == 1, count
    return ms, proof


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def kernel_stats(path, label, out):
    """the gate kernels' rows of a rocprofv3 --kernel-trace --stats run (Name, Calls, TotalDurationNs, AverageNs, ...)"""
    lines = ["kernel trace, %s (%s): calls, average us, total us" % (label, os.path.basename(path))]
    for r in csv.DictReader(open(path)):
        if "k_gate_" in r["Name"] or "k_quotient" in r["Name"]:
            lines.append("  %-60s %4d %10.1f %10.1f" % (r["Name"].split("(")[0].replace("void gbk::", ""), int(r["Calls"]),
                                                       float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))
    append(out, lines)


def bench_parent(parent, rounds, steps, out):
    """bench.py on this tree and on the parent's, alternated; each run is a fresh process"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "3"]
    values = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this", ROOT)):
            run = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            values[name].append(json.loads(run.stdout.strip().splitlines()[-1])["value"])
            print(name, values[name][-1], flush=True)
    lo, hi = min(values["parent"]), max(values["parent"])
    inside = [lo <= v <= hi for v in values["this"]]
    append(out, ["bench.py --gpus 1 --steps %d --warmup 3, parent commit and this commit alternated (%d rounds), `value` in proofs/s:" % (steps, rounds),
                 "  parent %s" % " ".join("%.3f" % v for v in values["parent"]),
                 "  this   %s" % " ".join("%.3f" % v for v in values["this"]),
                 "  spread of the parent's runs %.3f .. %.3f; this commit's runs inside it: %s; above it: %s; below it: %s" % (
                     lo, hi, sum(inside), sum(v > hi for v in values["this"]), sum(v < lo for v in values["this"]))])
    return all(v >= lo for v in values["this"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=14)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_program_times.txt"))
    ap.add_argument("--once", choices=["programs", "builtin"])
    ap.add_argument("--field", type=int, default=0)
    ap.add_argument("--kernel-stats", metavar="CSV")
    ap.add_argument("--label", default="")
    ap.add_argument("--bench-parent", metavar="TREE")
    ap.add_argument("--bench-steps", type=int, default=10)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.label, a.out)
    if a.bench_parent:     # (no GPU context in this process: the two trees' bench.py runs are its children)
        return 0 if bench_parent(os.path.abspath(a.bench_parent), a.rounds, a.bench_steps, a.out) else 1
    ctx = GpuContext(0)
    ctx.set_profiling(True)
    if a.once:
        c, w, pis = circuit(ctx, a.field, a.log_rows, a.once == "programs")
        for _ in range(2):
            print("%s field %d: %s %.3f ms" % (a.once, a.field, SCOPE, quotient_ms(ctx, c, w, pis)[0]))
        return
    lines = ["# tools/gate_program_times.py: \"%s\" scope, recursion gate set padded to 2^%d rows, %s" %
             (SCOPE, a.log_rows, time.strftime("%Y-%m-%d"))]
    for field, name in ((N.GB_GOLDILOCKS, "goldilocks"), (N.GB_BABYBEAR, "babybear")):
        forms = {"builtin": circuit(ctx, field, a.log_rows, False), "programs": circuit(ctx, field, a.log_rows, True)}
        proofs = {k: quotient_ms(ctx, *v)[1] for k, v in forms.items()}   # warm-up
        assert proofs["builtin"] == proofs["programs"], "the two forms must give the same proof bytes"
        times = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, v in forms.items():
                times[k].append(quotient_ms(ctx, *v)[0])
        regs = [p.num_regs for p in forms["programs"][0].programs]
        lines.append("%s: builtin %s ms; programs %s ms; ratio of medians %.2f; %d programs, %d instructions, registers max %d" % (
            name, " ".join("%.3f" % t for t in times["builtin"]), " ".join("%.3f" % t for t in times["programs"]),
            sorted(times["programs"])[len(times["programs"]) // 2] / sorted(times["builtin"])[len(times["builtin"]) // 2],
            len(regs), sum(p.num_instrs for p in forms["programs"][0].programs), max(regs)))
        for c, _, _ in forms.values():
            c.data.free()
    append(a.out, lines)


if __name__ == "__main__":
    sys.exit(main())
