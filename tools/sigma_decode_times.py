"""What decoding the sigmas costs: gb_circuit_decode_sigmas (include/goldibear_gpu.h) next to gb_circuit_create of the same circuit
in the same process, one MI355X.

    python tools/sigma_decode_times.py [--reps 3] [--out profiles/sigma_decode_times.txt] [--log-rows 12 16 20]

Circuits: the dummy gate set in the standard 135-wire / 80-routed-wire configuration, both fields, every routed cell of a NoopGate
row wired into a seeded random copy class of 1 to 5 cells (as tests/wired_circuits.py does) except one class of n / 4 cells, so that
the class pass has a long cycle to close.  For each circuit, appended to --out:
  * wall time of gb_circuit_create (host clock; the call ends synchronised) from the host matrix and from a matrix already on the
    device, --reps calls each after a warm-up that builds the context's tables for the size;
  * the timing scopes of gb_circuit_decode_sigmas on a fresh handle (HIP events, gb_ctx_scope_ms; the read-backs between the
    launches are inside the scopes): "decode sigmas: decode", "decode sigmas: classes", and with a partition set "decode sigmas:
    compare"; the rounds the class pass ran; there is no transform scope - the sigma values on H are resident with the circuit;
  * wall time of the whole call, profiling off, on --reps further fresh handles.
The decode happens once per circuit, so the yardstick is the circuit's own creation.  Nothing here is on a path bench.py times."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCOPES = ["decode sigmas: decode", "decode sigmas: classes", "decode sigmas: compare"]


def spread(xs):
    return "%.3f (min %.3f, max %.3f; %s)" % (sorted(xs)[len(xs) // 2], min(xs), max(xs), " ".join("%.3f" % x for x in xs))


def append(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def wired_constants_sigmas(F, cfg, degree_bits, seed):
    """-> (DummyCircuit, constants_sigmas, class sizes, identity partition map with the classes' first members as representatives)"""
    from oracle import plonk_dummy as PD
    base = PD.DummyCircuit(degree_bits, cfg, F=F, check_security=False)
    n, nr, nw = base.n, cfg.num_routed_wires, cfg.num_wires
    rng = np.random.default_rng(seed)
    noop = np.ones(n, dtype=bool)
    noop[[base.pi_row, base.const_row]] = False
    rows = np.flatnonzero(noop)
    cells = (np.arange(nr)[:, None] * n + rows[None, :]).ravel()
    cells = cells[rng.permutation(cells.size)]
    sizes = rng.integers(1, 6, size=cells.size)
    sizes[0] = n // 4
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells.size)) + 1]
    sizes[-1] -= int(sizes.sum()) - cells.size
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    nxt = np.arange(1, cells.size + 1)
    nxt[starts + sizes - 1] = starts
    ident = base.sigma.ravel()
    sigma = ident.copy()
    sigma[cells] = ident[cells[nxt]]
    cs = np.concatenate([base.constants_sigmas[:base.num_constants], sigma.reshape(nr, n)]).astype(F.dtype)
    # ProverOnlyCircuitData.representative_map for the same wiring: target row * num_wires + col, the class's first listed member
    col, row = np.divmod(cells, n)
    idx = row * nw + col
    m = np.arange(n * nw, dtype=np.uint64)
    m[idx] = np.repeat(idx[starts], sizes).astype(np.uint64)
    H = F.hout
    own = np.array([base.pi_row * nw + j for j in range(H)] + [base.const_row * nw], dtype=np.int64)
    m[own] = own[0]
    return base, cs, sizes, m


def measure(ctx, F, degree_bits, reps, out):
    import torch
    from oracle import plonk_dummy as PD
    from oracle.fields import GL
    from plonky2_goldibear_amd import CircuitData
    from plonky2_goldibear_amd import native as N
    need = -(-100 // (F.order_bits - degree_bits))
    cfg = PD.CircuitConfig(num_challenges=max(2, need)) if F is GL else PD.CircuitConfig.babybear(max(6, need), num_wires=135, num_routed_wires=80)
    base, cs, sizes, rep_map = wired_constants_sigmas(F, cfg, degree_bits, 0x5167 + degree_bits)
    kw = dict(num_wires=cfg.num_wires, num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants,
              num_challenges=cfg.num_challenges, arity_bits=cfg.arity_bits, gate_constant=base.GATE_CONSTANT, gate_pi=base.GATE_PI,
              field=N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR)
    cs_dev = torch.from_numpy(cs.view(np.int64 if cs.itemsize == 8 else np.int32)).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()

    def create(src):
        t0 = time.perf_counter()
        data = CircuitData(ctx, degree_bits, src, base.k_is, **kw)
        return data, (time.perf_counter() - t0) * 1e3

    create(cs)[0].free()                                    # the context's tables for this size, the pool's blocks
    from_host, from_device = [], []
    for _ in range(reps):
        for src, into in ((cs, from_host), (cs_dev, from_device)):
            data, ms = create(src)
            into.append(ms)
            data.free()
    lines = ["", "%s, 2^%d rows, %d wires, %d routed (%d routed cells, %d classes of two cells or more, the largest %d)" % (
        F.name, degree_bits, cfg.num_wires, cfg.num_routed_wires, cfg.num_routed_wires << degree_bits, int((sizes >= 2).sum()) + 1,
        int(sizes.max())),
        "  gb_circuit_create, host matrix, wall ms        %s" % spread(from_host),
        "  gb_circuit_create, device matrix, wall ms      %s" % spread(from_device)]
    # the scopes, once without and once with a partition to compare against
    for with_partition in (False, True):
        data, _ = create(cs_dev)
        if with_partition:
            data.set_partition(rep_map)
        ctx.set_profiling(True)
        ctx.scope_reset()
        info = data.decode_sigmas()
        ms = [ctx.scope_ms(s)[0] for s in SCOPES]
        ctx.set_profiling(False)
        assert info.largest_class == int(sizes.max()) and info.compared_partition == int(with_partition)
        lines.append("  scopes%s, ms: decode %.3f, classes %.3f (%d rounds), compare %.3f; sum %.3f" % (
            " with a partition" if with_partition else "", ms[0], ms[1], info.rounds, ms[2], sum(ms)))
        data.free()
    walls = []
    for _ in range(reps):
        data, _ = create(cs_dev)
        ctx.synchronize()
        t0 = time.perf_counter()
        data.decode_sigmas()
        walls.append((time.perf_counter() - t0) * 1e3)
        data.free()
    lines.append("  gb_circuit_decode_sigmas, no partition, wall ms %s" % spread(walls))
    lines.append("  decode / create from a device matrix           %.2f" % (sorted(walls)[len(walls) // 2] / sorted(from_device)[len(from_device) // 2]))
    append(out, lines)
    del cs_dev
    ctx.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_decode_times.txt"))
    ap.add_argument("--log-rows", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--fields", nargs="*", default=["goldilocks", "babybear"])
    args = ap.parse_args()
    from oracle.fields import BB, GL
    from plonky2_goldibear_amd import GpuContext
    ctx = GpuContext(0)
    append(args.out, ["gb_circuit_decode_sigmas next to gb_circuit_create (tools/sigma_decode_times.py, --reps %d); wall times: median "
                      "(min, max; every call)" % args.reps])
    for name in args.fields:
        for lg in args.log_rows:
            measure(ctx, GL if name == "goldilocks" else BB, lg, args.reps, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
