"""Representative maps for the partition-witness tests (no GPU code) and the slot map restated in numpy.

A map is ProverOnlyCircuitData.representative_map: u64[num_targets], indexed by Target::index - wire (row, col) ->
row * num_wires + col, virtual target i -> n * num_wires + i.  slot_map() restates csrc/partition_map.hpp: the representatives that
wire cells use, ascending ("slots"), and the slot of every wire cell."""
import numpy as np


def slot_map(rep_map, cells):
    """-> (reps [K] ascending, slots [cells], shared [K] bool: more than one wire cell reads the slot)"""
    used = np.asarray(rep_map[:cells], dtype=np.int64)
    reps, slots, counts = np.unique(used, return_inverse=True, return_counts=True)
    return reps.astype(np.uint32), slots.astype(np.uint32).reshape(-1), counts > 1


def expand(rep_map, values, n, num_wires):
    """full_witness (iop/witness.rs:359-371): [num_wires][n]"""
    cells = n * num_wires
    return np.ascontiguousarray(values[np.asarray(rep_map[:cells], dtype=np.int64)].reshape(n, num_wires).T)


def random_partition(n, num_wires, num_virtual, seed):
    """classes of 1 to 5 wire cells; a third of the classes of two cells or more are represented by a virtual target of their own
    (as a virtual target connected to wires is when the forest makes it the root); the other virtual targets stay unused"""
    rng = np.random.default_rng(seed)
    cells = n * num_wires
    m = np.arange(cells + num_virtual, dtype=np.uint64)
    order = rng.permutation(cells)
    sizes = rng.integers(1, 6, size=cells)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells)) + 1]
    sizes[-1] -= int(sizes.sum()) - cells
    start, virt = 0, 0
    for s in sizes:
        members = order[start:start + s]
        start += s
        rep = int(members[rng.integers(0, s)])
        if s >= 2 and virt < num_virtual and rng.integers(0, 3) == 0:
            rep = cells + virt
            virt += 2   # every other virtual target stays unused
        m[members] = rep
    return m


def maps(n, num_wires, seed=1):
    """name -> map: the structured maps of the slot-map tests and one seeded random partition"""
    cells = n * num_wires
    nv = max(4, cells // 8)
    ident = np.arange(cells, dtype=np.uint64)
    out = {"identity": ident.copy()}
    one = np.full(cells, cells - 1 if cells > 1 else 0, dtype=np.uint64)
    out["one_class"] = one
    virt = np.arange(cells + nv, dtype=np.uint64)
    virt[:cells] = cells + (np.arange(cells) % nv)          # every cell is represented by a virtual target
    out["virtual_representatives"] = virt
    corner = np.arange(cells + nv, dtype=np.uint64)          # (0, 0) joins (n - 1, num_wires - 1); the virtual targets are unused
    corner[0] = cells - 1
    out["corners_joined_unused_virtuals"] = corner
    out["random_partition"] = random_partition(n, num_wires, nv, seed + 31 * n + num_wires)
    return out


def field_values(F, count, seed, p3=False):
    """canonical values with 0, 1, p - 1 among them; p3: the in-memory words of the reference's field types for the SAME values -
    Goldilocks x + p wherever that fits in 64 bits, BabyBear the Montgomery words.  -> (canonical, words to hand over)"""
    p = F.P
    v = np.asarray(F.fill(seed, count), dtype=F.dtype).copy()
    v[:min(count, 3)] = np.array([0, 1, p - 1], dtype=F.dtype)[:min(count, 3)]
    if count > 8:
        v[count // 2], v[count - 1] = p - 1, 1
    if not p3:
        return v, v.copy()
    if v.itemsize == 8:
        w = v.copy()
        small = v < np.uint64((1 << 64) - p)
        w[small] = v[small] + np.uint64(p)
        return v, w
    return v, ((v.astype(np.uint64) << np.uint64(32)) % np.uint64(p)).astype(F.dtype)


def partition_of_witness(w, copy_classes, seed, num_virtual=64):
    """A PartitionWitness for the matrix w [num_wires][n] of a circuit whose copy classes are `copy_classes` = (cells, starts,
    sizes) with cells as col * n + row (tests/wired_circuits.py): every class's value sits at ONE representative chosen by seed -
    a member cell, or for about a third of the classes of two cells or more a virtual target of its own (every other virtual
    target stays unused); cells outside the classes represent themselves.  -> (representative_map, values), so that
    expand(map, values) == w."""
    nw, n = w.shape
    cells_total = nw * n
    rng = np.random.default_rng(seed)
    m = np.arange(cells_total + num_virtual, dtype=np.uint64)
    values = np.zeros(cells_total + num_virtual, dtype=w.dtype)
    values[:cells_total] = w.T.reshape(-1)                        # target index row * num_wires + col
    if copy_classes is not None:
        cells, starts, sizes = copy_classes
        col, row = np.divmod(np.asarray(cells, dtype=np.int64), n)
        idx = row * nw + col
        rep = idx[starts + rng.integers(0, sizes)]
        virtual = np.flatnonzero((sizes >= 2) & (rng.integers(0, 3, size=sizes.size) == 0))[:num_virtual // 2]
        rep[virtual] = cells_total + 2 * np.arange(virtual.size)
        values[rep] = values[idx[starts]]
        m[idx] = np.repeat(rep, sizes)
        dead = np.setdiff1d(idx, rep)                             # members that represent nobody: their entry is never read
        values[dead] = 0
    return m, values
