"""What generate_partial_witness costs on the device: gb_prove_inputs (include/goldibear_gpu.h) next to gb_prove_partition on the
same circuits, one MI355X.

    python tools/witness_generation_times.py [--reps 5] [--out profiles/witness_generation_times.txt]
    python tools/witness_generation_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

For each circuit, appended to --out:
  * the schedule: generators, levels, launches, classes (gb_circuit_generators_info);
  * the scopes "run generators" (upload of the inputs, the generator launches, the read-back of public inputs and error word) and
    "compute full witness" (here the expansion alone) of gb_prove_inputs: HIP events (gb_ctx_scope_ms), medians of --reps proofs
    after a warm-up; "run generators" divided by the number of levels for the circuits that are one dependent chain;
  * wall time (host clock around calls that end in a synchronised read-back, profiling off) of gb_prove_inputs next to
    gb_prove_partition on the mirror's values, the two alternated in one process, --reps of each;
  * beside them the Python mirror's _run_generators time for the same circuit (a Python loop, NOT the reference's Rust
    generate_partial_witness, which nobody has measured on this hardware).
Circuits: a range-check circuit - range_check(x, 32) on a fresh input per check, that is a WireSplitGenerator and BaseSumGate rows -
at 2^12 and 2^14 rows, both fields (--only-range-checks stops there); tests/circuits.py recursion_gates_circuit (both fields),
factorial_circuit, and a wide arithmetic circuit - 20 independent multiply-adds per row - at 2^12, 2^14 and 2^16 rows.
--bench-parent: bench.py on this tree and on a tree of the parent commit (built), alternated, each run a fresh process; the tree
--only-generator-programs: the wide arithmetic circuit of either field at 2^12 and 2^14 rows twice - as it is (compiled
generators, GB_GEN_ARITHMETIC records) and with its ArithmeticGate as a program gate whose generators are generator programs
(tests/generator_program_circuits.py; GB_GEN_PROGRAM records, interpreted) - and the ratio of the two "run generators" scopes.
that goes first alternates from round to round.  --bench-control TREE2 puts a second copy of the parent's tree in this tree's place:
what the comparison says about two identical trees.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SCOPES = ("run generators", "compute full witness")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def wide_arithmetic_circuit(log_rows, field=None):
    """every row an ArithmeticGate with 20 (BabyBear: the narrow configuration's) independent operations x * y + z_i on inputs:
    one level, as wide as it gets"""
    from plonky2_goldibear_amd import native as N
    from plonky2_goldibear_amd.circuit_builder import ArithmeticGate, CircuitBuilder, CircuitConfig, PartialWitness
    # ((64 - degree_bits) * num_challenges >= 100, circuit_builder.rs:1190-1192)
    cfg = CircuitConfig.recursion_config_bb_narrow() if field == N.GB_BABYBEAR else \
        CircuitConfig.standard_recursion_config_gl(num_challenges=3 if log_rows >= 15 else 2)
    b = CircuitBuilder(cfg)
    pw = PartialWitness()
    ops = ((1 << log_rows) - 8) * ArithmeticGate.new_from_config(cfg).num_ops
    x, y = b.add_virtual_targets(2)
    pw.set_target(x, 1000003)
    pw.set_target(y, 998244353)
    for i in range(ops):
        z = b.add_virtual_target()     # a distinct addend per operation (the builder shares equal operations): an input
        pw.set_target(z, 7 + 3 * i)
        b.mul_add(x, y, z)
    return b, pw


def range_check_circuit(field, log_rows):
    """range_check(x_i, 32) on a fresh input per check until the rows are full: every check is a WireSplitGenerator (a head and
    a continuation record) over one BaseSumGate row of 63 limbs (Goldilocks) or two of 30 (BabyBear, whose accumulator also
    takes an ArithmeticGate operation), and a BaseSplitGenerator per row"""
    from plonky2_goldibear_amd import native as N
    from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness
    cfg = CircuitConfig.standard_recursion_config_gl() if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow()
    b, pw = CircuitBuilder(cfg), PartialWitness()
    i = 0
    while b.num_gates() < (1 << log_rows) - 8:
        x = b.add_virtual_target()
        pw.set_target(x, (0x9E3779B9 * (i + 1)) % min(1 << 32, b.F.p))
        b.range_check(x, 32)
        i += 1
    return b, pw


def measure(ctx, name, b, pw, reps, out, chain=False, mirror_reps=3):
    c = b.build(ctx)
    c.set_generators(pw=pw)
    info = c.data.generators_info()
    rng = lambda: np.random.default_rng(11)
    values = c.generate_partition_witness(pw, rng())
    inputs = c.input_values(pw, rng())
    data = c.data
    want = data.prove_partition_once(values)                        # warm-up of both paths, and the bytes agree
    assert data.prove_inputs_once(inputs) == want
    ctx.set_profiling(True)
    scopes = {s: [] for s in SCOPES}
    for _ in range(reps):
        ctx.scope_reset()
        data.prove_inputs_once(inputs)
        for s in SCOPES:
            ms, count = ctx.scope_ms(s)
            assert count == 1, (s, count)
            scopes[s].append(ms)
    ctx.set_profiling(False)
    wall = {"inputs": [], "partition": []}
    for _ in range(reps):
        for k, call in (("partition", lambda: data.prove_partition_once(values)), ("inputs", lambda: data.prove_inputs_once(inputs))):
            t0 = time.perf_counter()
            call()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    mirror = []
    for _ in range(min(reps, mirror_reps)):
        t0 = time.perf_counter()
        c._run_generators(pw, rng())
        mirror.append((time.perf_counter() - t0) * 1e3)
    gen = median(scopes[SCOPES[0]])
    lines = [
        "%s: 2^%d rows x %d wires, %d generator records, %d inputs, %d classes; %d levels in %d launches, %d checks, %d unrunnable" % (
            name, c.degree_bits, c.config.num_wires, len(c.generator_records()), len(inputs), info["num_classes"], info["num_levels"],
            info["num_launches"], info["num_checks"], info["num_unrunnable"]),
        "  run generators %.3f ms, compute full witness (expansion alone) %.3f ms (medians of %d; all runs: %s)" % (
            gen, median(scopes[SCOPES[1]]), reps, " ".join("%.3f" % t for t in scopes[SCOPES[0]])),
    ]
    if chain:
        lines.append("  a dependent chain in one workgroup: %.2f us per level" % (gen * 1e3 / max(1, info["num_levels"])))
    lines += [
        "  wall, alternated: gb_prove_inputs %s ms; gb_prove_partition %s ms; medians %.3f - %.3f = %+.3f ms" % (
            " ".join("%.2f" % t for t in wall["inputs"]), " ".join("%.2f" % t for t in wall["partition"]),
            median(wall["inputs"]), median(wall["partition"]), median(wall["inputs"]) - median(wall["partition"])),
        "  host data per proof: %d input words against %d words of PartitionWitness.values" % (len(inputs), len(values)),
        "  python mirror _run_generators (not the reference's Rust): %.1f ms" % median(mirror),
    ]
    append(out, lines)
    data.free()
    ctx.trim()
    return gen


def bench_parent(parent, rounds, steps, out, this=ROOT, label="this commit", extra=()):
    """bench.py on this tree and on the parent's, each run a fresh process, alternated - and the tree that goes first alternates
    from round to round too, so that neither tree always runs on the device the other has just warmed up"""
    import json
    import subprocess
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "3"] + list(extra)
    values, order = {"parent": [], "this": []}, []
    for r in range(rounds):
        pair = (("parent", parent), ("this", this))
        for name, tree in (pair if r % 2 == 0 else pair[::-1]):
            run = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            values[name].append(json.loads(run.stdout.strip().splitlines()[-1])["value"])
            order.append(name[0])
            print(name, values[name][-1], flush=True)
    lo, hi = min(values["parent"]), max(values["parent"])
    inside = [lo <= v <= hi for v in values["this"]]
    append(out, ["bench.py --gpus 1 --steps %d --warmup 3%s, parent commit and %s alternated (%d rounds, run order %s), `value` in "
                 "proofs/s:" % (steps, "".join(" " + x for x in extra), label, rounds, "".join(order)),
                 "  parent %s" % " ".join("%.3f" % v for v in values["parent"]),
                 "  this   %s" % " ".join("%.3f" % v for v in values["this"]),
                 "  spread of the parent's runs %.3f .. %.3f; the other tree's runs inside it: %d; above it: %d; below it: %d" % (
                     lo, hi, sum(inside), sum(v > hi for v in values["this"]), sum(v < lo for v in values["this"]))])
    return all(v >= lo for v in values["this"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_generation_times.txt"))
    ap.add_argument("--wide-log-rows", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--range-check-log-rows", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--only-range-checks", action="store_true", help="the range-check circuits alone")
    ap.add_argument("--only-generator-programs", action="store_true",
                    help="the wide arithmetic circuit with compiled generators and with generator programs, both fields")
    ap.add_argument("--program-log-rows", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--bench-parent", metavar="TREE")
    ap.add_argument("--bench-control", metavar="TREE", help="with --bench-parent: compare TREE, a second copy of the parent, instead of this tree")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-extra", nargs="*", default=[], metavar="FLAG",
                    help="further bench.py flags for both trees, without their dashes (no-cpu-baseline no-babybear ..): legs to leave out; `value` is the headline leg either way")
    a = ap.parse_args()
    a.bench_extra = ["--" + x for x in a.bench_extra]
    if a.bench_parent:     # (no GPU context in this process: the two trees' bench.py runs are its children)
        if a.bench_control:   # the noise of the comparison itself: a second copy of the parent's tree in this commit's place
            ok = bench_parent(os.path.abspath(a.bench_parent), a.rounds, a.bench_steps, a.out, os.path.abspath(a.bench_control),
                              "a second copy of the parent commit (control)", extra=a.bench_extra)
        else:
            ok = bench_parent(os.path.abspath(a.bench_parent), a.rounds, a.bench_steps, a.out, extra=a.bench_extra)
        return 0 if ok else 1
    import circuits as CS
    from csrc_hash import csrc_sha16
    from plonky2_goldibear_amd import GpuContext, native as N
    ctx = GpuContext(0)
    append(a.out, ["# tools/witness_generation_times.py, csrc %s, %s: times in ms" % (csrc_sha16(), time.strftime("%Y-%m-%d"))])
    if a.only_generator_programs:
        import generator_program_circuits as GPC
        for lg in a.program_log_rows:
            for field, fname in ((N.GB_GOLDILOCKS, "goldilocks"), (N.GB_BABYBEAR, "babybear")):
                b, pw = wide_arithmetic_circuit(lg, field)
                compiled = measure(ctx, "wide arithmetic circuit, compiled generators (%s)" % fname, b, pw, a.reps, a.out, mirror_reps=1)
                b, pw = wide_arithmetic_circuit(lg, field)
                GPC.with_generated_program_gates(b)
                interpreted = measure(ctx, "wide arithmetic circuit, program gates with generator programs (%s)" % fname, b, pw, a.reps, a.out,
                                      mirror_reps=1)
                append(a.out, ["  interpreted / compiled generators, \"run generators\" at 2^%d rows (%s): %.3f / %.3f ms = %.2fx" % (
                    lg, fname, interpreted, compiled, interpreted / compiled)])
        ctx.close()
        return 0
    for lg in a.range_check_log_rows:
        for field, fname in ((N.GB_GOLDILOCKS, "goldilocks"), (N.GB_BABYBEAR, "babybear")):
            b, pw = range_check_circuit(field, lg)
            measure(ctx, "range-check circuit, range_check(x, 32) per input (%s)" % fname, b, pw, a.reps, a.out)
    if a.only_range_checks:
        ctx.close()
        return 0
    for field, fname in ((N.GB_GOLDILOCKS, "goldilocks"), (N.GB_BABYBEAR, "babybear")):
        b, pw, _ = CS.recursion_gates_circuit(field, seed=9)
        measure(ctx, "recursion_gates_circuit (%s)" % fname, b, pw, a.reps, a.out)
    b, pw = CS.factorial_circuit(count=99)
    measure(ctx, "factorial_circuit (99 factors)", b, pw, a.reps, a.out, chain=True)
    b, pw = CS.factorial_circuit(count=4000)
    measure(ctx, "factorial_circuit (4000 factors)", b, pw, a.reps, a.out, chain=True)
    for lg in a.wide_log_rows:
        b, pw = wide_arithmetic_circuit(lg)
        measure(ctx, "wide arithmetic circuit", b, pw, a.reps, a.out)
    ctx.close()


if __name__ == "__main__":
    sys.exit(main())
