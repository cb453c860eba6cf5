"""What "compute full witness" costs on the device and on the host: gb_prove_partition (include/goldibear_gpu.h) on the wired dummy
circuit (tests/wired_circuits.py; the partition from its copy classes, tests/partition_cases.py), both fields, 2^12, 2^16 and 2^20
rows.  Nothing here has a pass mark; the figures go into DESIGN.md sections 4 and 8.

    python tools/partition_witness_times.py [--log-rows 12 16 20] [--reps 5] [--out profiles/partition_witness_times.txt]
    python tools/partition_witness_times.py --bench-parent PARENT_TREE [--rounds 3] [--bench-steps 10]

Per field and size, after one warm-up of every call that is timed:
  * the scope "compute full witness" (HIP events, gb_ctx_scope_ms) of gb_prove_partition and its parts "partition compaction" /
    "partition upload" / "partition expansion", medians of --reps proofs; the kernel's bytes/s against its own traffic per cell:
    a 4-byte slot read, an element read and an element written (4 + 8 + 8 Goldilocks, 4 + 4 + 4 BabyBear);
  * wall time (host clock around calls that end in a synchronised read-back, profiling off) of gb_prove_partition next to gb_prove
    from the PAGE-LOCKED matrix, alternated in one process: the difference is what the compact upload costs for not being
    overlapped with the first transforms, as the column chunks of a host matrix are;
  * the host expansion it replaces: tools/full_witness_port.c, a single-threaded C port of the reference's loop (not the
    reference's Rust), compiled by this tool with `cc -O2`; and beside it the Python mirror's own expansion at 2^12 rows
    (BuiltCircuit.generate_witness less generate_partition_witness on the factorial circuit: the loop over copy_wires).
--bench-parent: `python bench.py --gpus 1` in this tree and in a built checkout of the parent commit, alternated, each run a fresh
process - the headline path does not call the new code."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SCOPES = ("compute full witness", "partition compaction", "partition upload", "partition expansion")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def host_port():
    src, bindir = os.path.join(ROOT, "tools", "full_witness_port.c"), os.path.join(ROOT, "tools", "bin")
    os.makedirs(bindir, exist_ok=True)
    lib = os.path.join(bindir, "libfull_witness_port.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", lib, src])
    return C.CDLL(lib)


def host_expansion_ms(port, F, m, values, n, nw, reps):
    out = np.empty((nw, n), dtype=F.dtype)
    fn = port.full_witness_u64 if values.itemsize == 8 else port.full_witness_u32
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn(values.ctypes.data, m.ctypes.data, n, nw, out.ctypes.data)
        times.append((time.perf_counter() - t0) * 1e3)
    return median(times[1:]), out


def measure(ctx, F, tag, name, lg, reps, port, out):
    from oracle import plonk_dummy as D
    from oracle.fields import GL
    from plonky2_goldibear_amd import CircuitData
    import partition_cases as PC
    import wired_circuits as W
    ch = -(-100 // (F.order_bits - lg))                                   # circuit_builder.rs:1190-1192
    cfg = D.CircuitConfig(num_challenges=max(2, ch)) if F is GL else D.CircuitConfig.babybear(max(6, ch))
    circ, w, kw = W.wired_dummy_circuit(F, cfg, lg, 4000 + lg, "random")
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, **kw)
    m, values = PC.partition_of_witness(w, circ.copy_classes, 4000 + lg)
    n, nw = circ.n, cfg.num_wires
    cells = n * nw
    K = np.unique(m[:cells]).size
    gpu.set_partition(m)
    pinned = ctx.host_alloc(w.shape, w.dtype)
    pinned[...] = w
    host_ms, expanded = host_expansion_ms(port, F, m, values, n, nw, reps)
    assert np.array_equal(expanded, w)
    want = gpu.prove_once(pinned)                                         # warm-up of both paths, and the bytes agree
    assert gpu.prove_partition_once(values) == want
    ctx.set_profiling(True)
    scopes = {s: [] for s in SCOPES}
    for _ in range(reps):
        ctx.scope_reset()
        gpu.prove_partition_once(values)
        for s in SCOPES:
            ms, count = ctx.scope_ms(s)
            assert count == 1, (s, count)
            scopes[s].append(ms)
    ctx.set_profiling(False)
    wall = {"partition": [], "matrix": []}
    for _ in range(reps):
        for k, call in (("matrix", lambda: gpu.prove_once(pinned)), ("partition", lambda: gpu.prove_partition_once(values))):
            t0 = time.perf_counter()
            call()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {s: median(v) for s, v in scopes.items()}
    traffic = cells * (4 + 2 * values.itemsize)
    kms = med["partition expansion"]
    dw = median(wall["partition"]) - median(wall["matrix"])
    append(out, [
        "%s 2^%d rows x %d wires: %d targets, K = %d slots (%.1f MB staged against %.1f MB of matrix)" % (
            name, lg, nw, len(m), K, K * values.itemsize / 1e6, cells * values.itemsize / 1e6),
        "  compute full witness %.3f ms = compaction %.3f + upload %.3f + kernel %.3f (medians of %d; all runs: %s)" % (
            med[SCOPES[0]], med[SCOPES[1]], med[SCOPES[2]], kms, reps, " ".join("%.3f" % t for t in scopes[SCOPES[0]])),
        "  k_expand_partition: %.1f MB of traffic in %.3f ms = %.0f GB/s" % (traffic / 1e6, kms, traffic / kms / 1e6),
        "  wall, alternated: gb_prove_partition %s ms; gb_prove (page-locked matrix) %s ms; medians %.3f - %.3f = %+.3f ms" % (
            " ".join("%.2f" % t for t in wall["partition"]), " ".join("%.2f" % t for t in wall["matrix"]),
            median(wall["partition"]), median(wall["matrix"]), dw),
        "  host expansion it replaces (tools/full_witness_port.c, one thread, cc -O2; a port, not the reference's Rust): %.3f ms" % host_ms,
    ])
    ctx.host_free(pinned)
    gpu.free()
    ctx.trim()


def python_mirror(out, reps):
    """the mirror's own expansion: generate_witness less generate_partition_witness (both run the generators)"""
    import circuits as CS
    b, pw = CS.factorial_circuit(count=4000)
    c = b.build(None)
    t = {"matrix": [], "partition": []}
    for _ in range(reps):
        for k, fn in (("matrix", c.generate_witness), ("partition", c.generate_partition_witness)):
            t0 = time.perf_counter()
            fn(pw)
            t[k].append((time.perf_counter() - t0) * 1e3)
    append(out, ["python mirror, factorial circuit of 2^%d rows: generate_witness %.1f ms, generate_partition_witness %.1f ms (medians of "
                 "%d): the expansion loop over copy_wires is the difference, %.1f ms" % (
                     c.degree_bits, median(t["matrix"]), median(t["partition"]), reps, median(t["matrix"]) - median(t["partition"]))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_witness_times.txt"))
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
    port = host_port()
    ctx = GpuContext(0)
    append(a.out, ["# tools/partition_witness_times.py, csrc %s, %s: wired dummy circuit, times in ms" % (csrc_sha16(), time.strftime("%Y-%m-%d"))])
    for F, tag, name in ((GL, N.GB_GOLDILOCKS, "goldilocks"), (BB, N.GB_BABYBEAR, "babybear")):
        for lg in a.log_rows:
            measure(ctx, F, tag, name, lg, a.reps, port, a.out)
    python_mirror(a.out, a.reps)
    ctx.close()


if __name__ == "__main__":
    sys.exit(main())
