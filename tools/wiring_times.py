"""What making the wiring costs: gb_wiring_sigmas (include/goldibear_gpu.h) next to two host baselines written for this purpose and
next to gb_circuit_create of the same circuit, one process, one MI355X.

    python tools/wiring_times.py [--reps 3] [--out profiles/wiring_times.txt] [--log-rows 12 16 20] [--path-log-rows 16]

Shapes: the standard 135-wire / 80-routed-wire configuration; every routed cell in a seeded random class of 1 to 5 cells except one
class of n / 4 cells (the shape tools/sigma_decode_times.py decodes, so the two directions can be read side by side), the pairs of
all classes shuffled; and at --path-log-rows ONE class of all routed cells, given as a shuffled path - the worst case of the
union-find.  For each shape and field, appended to --out:
  * the timing scopes of one call (HIP events, gb_ctx_scope_ms; the read-backs between the launches are inside the scopes);
  * wall time of the synchronised call with host outputs (sigmas and map copied back) and with the sigmas left on the device (the
    map is copied back either way), --reps calls each after a warm-up; medians;
  * wall time of gb_circuit_create from a device matrix that holds those sigmas: the step this stage precedes;
  * the single-threaded C++ baseline tools/wiring_baseline.cpp (union-find, std::stable_sort by label, one product per cell) on the
    same machine's CPU (--reps runs, one run at 2^18 rows and above), and up to --python-log-rows the Python CircuitBuilder._forest + _sigma.
Nothing here is on a path bench.py times."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCOPES = ["wiring: upload", "wiring: classes", "wiring: order", "wiring: sigmas"]
WIRES = (135, 80)


def spread(xs):
    return "%.3f (min %.3f, max %.3f; %s)" % (sorted(xs)[len(xs) // 2], min(xs), max(xs), " ".join("%.3f" % x for x in xs))


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def build_baseline():
    exe = os.path.join(ROOT, "tools", "bin", "wiring_baseline")
    src = os.path.join(ROOT, "tools", "wiring_baseline.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        shim = os.path.join(ROOT, "tests", "host_shim")   # lets a host compiler read the field headers of csrc/
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O2", "-include", os.path.join(shim, "shim.h"), "-I", shim,
                               "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), "-o", exe, src])
    return exe


def pairs_of(degree_bits, kind, seed):
    nw, nr = WIRES
    n = 1 << degree_bits
    rng = np.random.default_rng(seed)
    rc = (np.arange(n, dtype=np.int64)[:, None] * nw + np.arange(nr, dtype=np.int64)[None, :]).ravel()
    if kind == "path":
        pairs, sizes = np.stack([rc[:-1], rc[1:]], axis=1), np.array([rc.size])
    else:
        cells = rc[rng.permutation(rc.size)]
        sizes = rng.integers(1, 6, size=cells.size)
        sizes[0] = n // 4
        sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells.size)) + 1]
        sizes[-1] -= int(sizes.sum()) - cells.size
        keep = np.ones(cells.size - 1, dtype=bool)
        keep[np.cumsum(sizes)[:-1] - 1] = False
        pairs = np.stack([cells[:-1][keep], cells[1:][keep]], axis=1)
    return np.ascontiguousarray(pairs[rng.permutation(len(pairs))].astype(np.uint64)), sizes


def python_baseline(F, field, degree_bits, pairs, k_is):
    from plonky2_goldibear_amd import native as N
    from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, wire
    cfg = CircuitConfig.standard_recursion_config_gl() if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow(
        num_wires=WIRES[0], num_routed_wires=WIRES[1])
    b = CircuitBuilder(cfg)
    nw = WIRES[0]
    b.copy_constraints = [(wire(int(x) // nw, int(x) % nw), wire(int(y) // nw, int(y) % nw)) for x, y in pairs.tolist()]
    subgroup = b.F._powers(b.F.two_adic_generator(degree_bits), 1 << degree_bits)
    t0 = time.perf_counter()
    find = b._forest()
    t1 = time.perf_counter()
    sig = b._sigma(find, 1 << degree_bits, k_is, subgroup)
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, sig


def measure(ctx, F, degree_bits, kind, pairs, sizes, args, exe):
    import torch
    from oracle import plonk_dummy as PD
    from oracle.fields import GL
    from plonky2_goldibear_amd import CircuitData, sigma_polys
    from plonky2_goldibear_amd import native as N
    nw, nr = WIRES
    n = 1 << degree_bits
    field = N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR
    k_is = np.array([pow(F.generator, i, F.P) for i in range(nr)], dtype=F.dtype)
    num_targets = n * nw

    def call(device):
        ctx.synchronize()
        t0 = time.perf_counter()
        got = sigma_polys(ctx, field, degree_bits, nw, nr, k_is, pairs, num_targets, device=device)
        return got, (time.perf_counter() - t0) * 1e3

    (sig, rep, info), _ = call(False)                        # warm-up: the context's tables for this size, the pool's blocks
    ctx.set_profiling(True)
    ctx.scope_reset()
    call(False)
    scopes = [ctx.scope_ms(s)[0] for s in SCOPES]
    ctx.set_profiling(False)
    host_out = [call(False)[1] for _ in range(args.reps)]
    dev_out = []
    for _ in range(args.reps):
        (dsig, _, _), ms = call(True)
        dev_out.append(ms)
    lines = ["", "%s, 2^%d rows, %d wires, %d routed, %s: %d pairs, %d moved cells in %d classes, the largest %d; %d passes" % (
        F.name, degree_bits, nw, nr, kind, len(pairs), info.moved_cells, info.num_classes, info.largest_class, info.rounds),
        "  scopes, ms: upload %.3f, classes %.3f, order %.3f, sigmas %.3f; sum %.3f" % (*scopes, sum(scopes)),
        "  gb_wiring_sigmas, host sigmas and map, wall ms   %s" % spread(host_out),
        "  gb_wiring_sigmas, device sigmas, wall ms         %s" % spread(dev_out)]
    assert info.largest_class == int(sizes.max())
    # gb_circuit_create of a circuit with these sigmas, from a device matrix
    need = -(-100 // (F.order_bits - degree_bits))
    cfg = PD.CircuitConfig(num_challenges=max(2, need)) if F is GL else PD.CircuitConfig.babybear(max(6, need), num_wires=nw, num_routed_wires=nr)
    head = torch.zeros((1 + cfg.num_constants, n), dtype=dsig.dtype, device=dsig.device)
    cs_dev = torch.cat([head, dsig]).contiguous()
    torch.cuda.synchronize()
    kw = dict(num_wires=nw, num_routed_wires=nr, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges, arity_bits=cfg.arity_bits,
              gate_constant=1, gate_pi=2, field=field)
    create = []
    for i in range(args.reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        data = CircuitData(ctx, degree_bits, cs_dev, k_is, **kw)
        create.append((time.perf_counter() - t0) * 1e3)
        data.free()
    lines.append("  gb_circuit_create, device matrix, wall ms        %s" % spread(create[1:]))
    lines.append("  wiring (device sigmas) / create                  %.2f" % (sorted(dev_out)[len(dev_out) // 2] / sorted(create[1:])[args.reps // 2]))
    del cs_dev, dsig, head
    # the host baselines
    path = os.path.join(ROOT, "tools", "bin", "wiring_case.bin")
    np.concatenate([np.array([0 if F is GL else 1, degree_bits, nw, nr, num_targets, len(pairs)], dtype=np.uint64), k_is.astype(np.uint64),
                    pairs.ravel()]).tofile(path)
    done = subprocess.run([exe, path, str(args.reps if degree_bits < 18 else 1)], capture_output=True, text=True)   # (seconds a run above)
    os.remove(path)
    if done.returncode == 0:
        rows = [[float(v) for v in line.split()[:4]] for line in done.stdout.strip().splitlines()]
        mid = sorted(rows, key=lambda r: r[3])[len(rows) // 2]
        lines.append("  C++ baseline, one thread, ms: classes %.3f, order %.3f, sigmas %.3f; total %.3f (totals: %s)" % (
            *mid, " ".join("%.3f" % r[3] for r in rows)))
    else:
        lines.append("  C++ baseline: exit status %d" % done.returncode)
    if degree_bits <= args.python_log_rows:
        forest_ms, sigma_ms, py = python_baseline(F, field, degree_bits, pairs, k_is)
        assert np.array_equal(py, sig), "the Python builder's sigmas differ"
        lines.append("  Python _forest + _sigma, ms: %.1f + %.1f = %.1f (sigmas equal the device's)" % (forest_ms, sigma_ms, forest_ms + sigma_ms))
    append(args.out, lines)
    ctx.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wiring_times.txt"))
    ap.add_argument("--log-rows", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--path-log-rows", type=int, nargs="*", default=[16])
    ap.add_argument("--python-log-rows", type=int, default=12)
    ap.add_argument("--fields", nargs="*", default=["goldilocks", "babybear"])
    args = ap.parse_args()
    from oracle.fields import BB, GL
    from plonky2_goldibear_amd import GpuContext
    exe = build_baseline()
    ctx = GpuContext(0)
    append(args.out, ["gb_wiring_sigmas next to host baselines and gb_circuit_create (tools/wiring_times.py, --reps %d); wall times: median "
                      "(min, max; every call)" % args.reps])
    for kind, sizes_lg in (("classes of 1 to 5 and one of n / 4", args.log_rows), ("path", args.path_log_rows)):
        for lg in sizes_lg:
            pairs, sizes = pairs_of(lg, "path" if kind == "path" else "classes", 0x5167 + lg)
            for name in args.fields:
                measure(ctx, GL if name == "goldilocks" else BB, lg, kind, pairs, sizes, args, exe)
    ctx.close()


if __name__ == "__main__":
    main()
