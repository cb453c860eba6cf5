"""What the witness check costs: gb_check_witness (include/goldibear_gpu.h) next to the quotient stage and the whole proof of the
same circuit, one MI355X.

    python tools/witness_check_times.py [--reps 7] [--out profiles/witness_check_times.txt] [--log-rows 12 14] [--dummy-log-rows 20]

For each circuit, appended to --out:
  * "check witness: prepare" of the FIRST check on the circuit (the selector and constant columns transformed to values on H,
    the row list of every gate) and "check witness" of that call and of --reps later ones (HIP events, gb_ctx_scope_ms): the
    launches of every gate that has rows, the copy pass where the circuit has a partition, the read-back of the counts; and the
    launches inside it one by one - per gate kind (GB_GATE_*), the copy pass, the pass that looks for words not below p - so that
    the file says which launch dominates;
  * wall time of gb_check_witness on the satisfying device matrix (host clock around a call that ends in a synchronised
    read-back, profiling off), --reps calls after a warm-up;
  * next to them, same process, option "check_witness" off: the scope "compute quotient polys" of gb_prove and the wall time of
    the whole gb_prove on the same device matrix.
The check evaluates one gate per row on n points, the quotient stage every gate on 8 n points.
Circuits: tools/bench_recursion_shape.py's recursion-gate-set circuit at 2^12 and 2^14 rows, with its partition (copies are
checked); the benchmark's dummy circuit (plain gb_circuit_create, no partition) at 2^20 rows; both fields."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

PREPARE, CHECK, QUOTIENT = "check witness: prepare", "check witness", "compute quotient polys"
# with profiling on, check_host.inc times every launch inside "check witness": the gate launches by gate kind (GB_GATE_*)
PARTS = ["check witness: canonical words", "check witness: copies"] + ["check witness: gate kind %d" % k for k in range(19)]


def median(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return "%.3f (min %.3f, max %.3f; %s)" % (median(xs), min(xs), max(xs), " ".join("%.3f" % x for x in xs))


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def measure(ctx, name, data, wd, pis, reps, out):
    """data: a CircuitData nothing has been checked on yet; wd: the satisfying witness as a device tensor"""
    ctx.set_option("check_witness", 0)
    proof = data.prove(wd, pis)                 # warm-up of the prover's shapes; the witness is a satisfying one
    assert data.verify(proof)
    ctx.set_profiling(True)
    ctx.scope_reset()
    violations, res = data.check_witness(wd, pis)
    assert violations == [] and res.num_gate_violations == 0 and res.num_copy_violations == 0
    prepare, n_prep = ctx.scope_ms(PREPARE)
    first, _ = ctx.scope_ms(CHECK)
    assert n_prep == 1
    steady, quotient, parts = [], [], {}
    for _ in range(reps):
        ctx.scope_reset()
        data.check_witness(wd, pis)
        ms, count = ctx.scope_ms(CHECK)
        assert count == 1 and ctx.scope_ms(PREPARE)[1] == 0      # the preparation is cached
        steady.append(ms)
        for part in PARTS:                                       # the launches inside the scope, each between two events
            ms, count = ctx.scope_ms(part)
            if count:
                parts.setdefault(part, []).append((ms, count))
    for _ in range(reps):
        ctx.scope_reset()
        data.prove(wd, pis)
        quotient.append(ctx.scope_ms(QUOTIENT)[0])
    ctx.set_profiling(False)
    wall = {"check": [], "prove": []}
    for _ in range(reps):
        for k, call in (("check", lambda: data.check_witness(wd, pis)), ("prove", lambda: data.prove(wd, pis))):
            ctx.synchronize()
            t0 = time.perf_counter()
            call()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    append(out, [
        "%s: 2^%d rows x %d wires, copies %s" % (name, data.cfg.degree_bits, data.cfg.num_wires, "checked" if res.copies_checked else "not checked (no partition)"),
        "  first call: \"check witness: prepare\" %.3f ms, \"check witness\" %.3f ms" % (prepare, first),
        "  steady \"check witness\", median of %d: %s" % (reps, spread(steady)),
        "  its launches (medians; a gate kind's launches added up): " + ", ".join(
            "%s %.3f%s" % (part.split(": ")[1], median([ms for ms, _ in v]), " (%d launches)" % v[0][1] if v[0][1] > 1 else "")
            for part, v in sorted(parts.items(), key=lambda kv: -median([ms for ms, _ in kv[1]]))),
        "  \"compute quotient polys\" of gb_prove, median of %d: %s" % (reps, spread(quotient)),
        "  steady check / quotient stage: %.3f" % (median(steady) / median(quotient)),
        "  wall, alternated, option check_witness off: gb_check_witness %s ms; gb_prove %s ms" % (spread(wall["check"]), spread(wall["prove"])),
    ])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_check_times.txt"))
    ap.add_argument("--log-rows", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--dummy-log-rows", type=int, nargs="*", default=[20])
    a = ap.parse_args()
    import torch
    from circuits import recursion_gates_circuit
    from csrc_hash import csrc_sha16
    from oracle import plonk_dummy as D
    from oracle.fields import BB
    from plonky2_goldibear_amd import CircuitData, GpuContext, native as N
    from plonky2_goldibear_amd.circuit_builder import NoopGate
    ctx = GpuContext(0)
    append(a.out, ["# tools/witness_check_times.py, csrc %s, %s: times in ms" % (csrc_sha16(), time.strftime("%Y-%m-%d"))])
    fields = ((N.GB_GOLDILOCKS, "goldilocks", np.int64), (N.GB_BABYBEAR, "babybear", np.int32))
    for lg in a.log_rows:
        for field, fname, view in fields:
            # circuit_builder.rs:1190-1192: (F::bits() - degree_bits) * num_challenges >= 100
            challenges = (2 if lg <= 14 else 3) if field == N.GB_GOLDILOCKS else max(6, -(-100 // (31 - lg)))
            b, pw, _ = recursion_gates_circuit(field, seed=lg, num_challenges=challenges)
            while b.num_gates() < (1 << lg) - 8:
                b.add_gate(NoopGate())
            c = b.build(ctx)
            assert c.degree_bits == lg
            c.data.set_partition(c.representative_map, c.public_input_targets)
            w, pis = c.generate_witness(pw)
            wd = torch.from_numpy(w.view(view)).to("cuda:0")
            measure(ctx, "recursion-gate-set circuit, %d gates (%s)" % (len(c.gate_table), fname), c.data, wd, pis, a.reps, a.out)
            c.data.free()
            ctx.trim()
    for lg in a.dummy_log_rows:
        for field, fname, view in fields:
            if field == N.GB_GOLDILOCKS:
                circ = D.DummyCircuit(lg, D.CircuitConfig(num_challenges=3), check_security=False)
            else:
                circ = D.DummyCircuit(lg, D.CircuitConfig.babybear(10), check_security=False, F=BB)
            cfg = circ.cfg
            data = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                               num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                               arity_bits=cfg.arity_bits, field=field)
            wd = None
            for seed in range(1, 9):      # a witness that meets a zero denominator (BabyBear) would be re-drawn: take the next
                wd = torch.from_numpy(circ.witness(seed=seed).view(view)).to("cuda:0")
                try:
                    data.prove_once(wd)
                    break
                except N.PermArgZeroError:
                    data.drop_retry()
            measure(ctx, "the benchmark's dummy circuit (%s)" % fname, data, wd, (), a.reps, a.out)
            data.free()
            ctx.trim()
    ctx.close()


if __name__ == "__main__":
    sys.exit(main())
