"""Copy constraints and what gb_wiring_sigmas must make of them (no GPU code, nothing from the code under test).

A case is a shape (degree_bits, num_wires, num_routed_wires, virtual targets) and a list of pairs of target indices - wire
(row, column) is row * num_wires + column, virtual target i is degree * num_wires + i.  `structure` computes, once per case and for
both fields, the classes with a plain Python union-find whose roots are arbitrary (it hooks as the reference does), the
representative map as the class minimum, the routed wire cells of every class in sorted (row, column) order with each one's
successor, and the counts of gb_wiring_info; `sigmas` then computes the values with Python integers,
k_is[col'] * pow(w, row', p) % p."""
import functools

import numpy as np

STANDARD = (135, 80)   # standard_recursion_config's wires
SMALL = (9, 5)         # tests/sigma_cases.py SmallRoutedCircuit's proportions


class Case:
    def __init__(self, name, degree_bits, wires, pairs, num_virtual=0):
        self.name, self.degree_bits, self.n = name, degree_bits, 1 << degree_bits
        self.num_wires, self.num_routed = wires
        self.pairs = np.array(pairs, dtype=np.uint64).reshape(-1, 2)
        self.cells = self.n * self.num_wires
        self.num_targets = self.cells + num_virtual

    def __repr__(self):
        return "%s-2^%d-%dw" % (self.name, self.degree_bits, self.num_wires)


def routed_cells(degree_bits, wires):
    """the routed wire cells in ascending cell order"""
    nw, nr = wires
    rows = np.arange(1 << degree_bits, dtype=np.int64)
    return (rows[:, None] * nw + np.arange(nr, dtype=np.int64)[None, :]).ravel()


def path(cells):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([cells[:-1], cells[1:]], axis=1)


def classes_of_sizes(rng, cells, sizes):
    """pairs that make classes of the given sizes out of the first sum(sizes) of `cells`, each class a path in the order given,
    the pairs of all of them shuffled"""
    sizes = np.asarray(sizes, dtype=np.int64)
    pairs = path(cells[:int(sizes.sum())])
    pairs = np.delete(pairs, np.cumsum(sizes)[:-1] - 1, axis=0)   # no pair from a class's last cell to the next class's first
    return pairs[rng.permutation(len(pairs))]


def random_classes(degree_bits, wires, seed):
    """seeded classes of 1 to 5 cells covering every routed cell"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(routed_cells(degree_bits, wires))
    sizes = rng.integers(1, 6, size=cells.size)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells.size)) + 1]
    sizes[-1] -= int(sizes.sum()) - cells.size
    return classes_of_sizes(rng, cells, [int(s) for s in sizes if s > 0])


def families(degree_bits, wires, tile, seed=0x51C):
    """the case families of a shape that has room for them; n >= 4"""
    nw, nr = wires
    n = 1 << degree_bits
    rc = routed_cells(degree_bits, wires)
    rng = np.random.default_rng(seed + degree_bits)
    cell = lambda row, col: row * nw + col   # noqa: E731
    cells = n * nw
    a, b = cell(1, 0), cell(2, min(1, nr - 1))
    mk = lambda name, pairs, nv=3: Case(name, degree_bits, wires, pairs, nv)   # noqa: E731
    out = [mk("no_pairs", []), mk("one_pair", [(a, b)]), mk("self_pair", [(a, a)]), mk("same_pair_thrice", [(a, b), (a, b), (b, a)]),
           mk("random_1_to_5", random_classes(degree_bits, wires, seed)),
           mk("all_path_ascending", path(rc)), mk("all_path_descending", path(rc[::-1])),
           mk("all_path_shuffled", path(rc)[rng.permutation(rc.size - 1)]),
           mk("all_star_highest", np.stack([np.full(rc.size - 1, rc[-1]), rc[:-1]], axis=1)),
           mk("row_and_column", [(cell(3, 0), cell(3, nr - 1)), (cell(3, nr - 1), cell(3, nr // 2)), (cell(1, nr - 1), cell(2, nr - 1)),
                                 (cell(3, nr - 1), cell(3, nr - 1)), (cell(0, nr - 1), cell(2, nr - 1))]),
           mk("virtual_chain_of_three", [(a, cells), (cells + 2, b), (cells + 1, cells), (cells + 1, cells + 2)]),
           mk("virtual_only_class", [(cells + 4, cells + 2), (cells + 2, cells + 3), (a, b)], 6),
           mk("virtual_unused", [(a, b), (cells + 1, b)], 40),
           mk("exactly_the_wire_targets", [(a, b), (b, cell(3, 0))], 0)]
    if n >= 16 and nr >= 5:   # lowest in row * num_wires + col order: (row 2, wire 4); lowest in col * n + row order: (row 9, wire 3)
        out.append(mk("awkward_pair", [(cell(9, 3), cell(2, 4)), (cell(5, 1), cell(4, 2))]))
    if rc.size >= 3 * tile + 63 + 64 + 65 + 8:
        shuffled = rng.permutation(rc)
        out.append(mk("sizes_around_wave_and_tile", classes_of_sizes(rng, shuffled, [63, 64, 65, tile - 1, tile, tile + 1])))
        # every routed cell is kept, so a cell's place in the compacted list is its place among the routed cells: one class lies
        # across the first tile boundary, one across the second, the rest are neighbours in twos
        straddle = [rc[tile - 2:tile + 2], rc[2 * tile - 1:2 * tile + 1]]
        rest = np.concatenate([rc[:tile - 2], rc[tile + 2:2 * tile - 1], rc[2 * tile + 1:]])
        rest = rest[:rest.size & ~1].reshape(-1, 2)
        out.append(mk("straddles_a_tile_boundary", np.concatenate([path(straddle[0]), path(straddle[1]), rest])))
    return out


def single_wire(degree_bits, num_wires, seed=5):
    """2^degree_bits rows with ONE routed wire (of num_wires): seeded cycles of 2 to 5 rows, one of 300 that holds the first and
    the last row, and one through the rows around every digit boundary of the label"""
    n = 1 << degree_bits
    rng = np.random.default_rng(seed)
    edge = sorted({r for d in (8, 16, 24) for r in ((1 << d) // num_wires - 1, (1 << d) // num_wires, (1 << d) // num_wires + 1)
                   if 0 < r < n - 1})
    free = np.setdiff1d(np.arange(1, n - 1), edge)
    sizes = [int(s) for s in rng.integers(2, 6, size=1000)]
    rows = rng.choice(free, size=298 + sum(sizes), replace=False)
    pairs = [path(np.concatenate([[0, n - 1], rows[:298]]) * num_wires), path(np.array(edge, dtype=np.int64) * num_wires),
             classes_of_sizes(rng, rows[298:] * num_wires, sizes)]
    return Case("single_routed_wire", degree_bits, (num_wires, 1), np.concatenate(pairs), 2)


@functools.lru_cache(maxsize=None)
def _structure(case_key):
    case = _CASES[case_key]
    nw, nr, n = case.num_wires, case.num_routed, case.n
    parent = {}

    def find(t):
        root = t
        while parent.get(root, root) != root:
            root = parent[root]
        while parent.get(t, t) != t:
            parent[t], t = root, parent[t]
        return root

    for x, y in case.pairs.tolist():
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[ry] = rx
    touched = np.unique(case.pairs).astype(np.int64)
    rep = np.arange(case.num_targets, dtype=np.uint64)
    moved_from = moved_to = np.zeros(0, dtype=np.int64)
    sizes = np.zeros(0, dtype=np.int64)
    if touched.size:
        roots = np.array([find(t) for t in touched.tolist()], dtype=np.int64)
        order = np.lexsort((touched, roots))           # by class, inside a class by target index = by (row, column)
        members, roots = touched[order], roots[order]
        heads = np.concatenate([[True], roots[1:] != roots[:-1]])
        group = np.cumsum(heads) - 1
        rep[members] = members[heads][group]          # the class minimum
        routed = (members < case.cells) & (members % nw < nr)
        rc, g = members[routed], group[routed]
        if rc.size:
            first = np.concatenate([[True], g[1:] != g[:-1]])
            starts = np.flatnonzero(first)
            sizes = np.diff(np.concatenate([starts, [rc.size]]))
            nxt = np.arange(1, rc.size + 1)
            nxt[starts + sizes - 1] = starts
            big = np.repeat(sizes >= 2, sizes)
            moved_from, moved_to = rc[big], rc[nxt][big]
    big_sizes = sizes[sizes >= 2]
    info = dict(routed_cells=n * nr, moved_cells=int(big_sizes.sum()), num_classes=int(big_sizes.size),
                largest_class=int(big_sizes.max()) if big_sizes.size else 1,
                merged_targets=int((rep != np.arange(case.num_targets, dtype=np.uint64)).sum()))
    return rep, moved_from, moved_to, info


_CASES = {}


def structure(case):
    """-> (representative map, the moved cells, their successors (both as cell numbers), the gb_wiring_info counts)"""
    _CASES[repr(case)] = case
    return _structure(repr(case))


def k_is_of(F, num_routed):
    return np.array([pow(F.generator, i, F.P) for i in range(num_routed)], dtype=F.dtype)


def sigmas(case, F):
    """[num_routed][n] with Python integers"""
    p, n, nw = F.P, case.n, case.num_wires
    w, sub = F.two_adic_generator(case.degree_bits), [1] * case.n
    for i in range(1, n):
        sub[i] = sub[i - 1] * w % p
    ks = [int(k) for k in k_is_of(F, case.num_routed)]
    sig = np.array([[k * s % p for s in sub] for k in ks], dtype=F.dtype)
    _, moved_from, moved_to, _ = structure(case)
    for src, dst in zip(moved_from.tolist(), moved_to.tolist()):
        sig[src % nw, src // nw] = ks[dst % nw] * sub[dst // nw] % p   # sub[r] = pow(w, r, p)
    return sig


def pack(F, probes, cases):
    """the word file of tests/host_shim/wiring.cpp (the format is there): probes are (op, a, b, c, d) tuples"""
    words = [np.array([0 if F.order_bits == 64 else 1, len(probes)], dtype=np.uint64),
             np.array(probes, dtype=np.uint64).reshape(-1, 5).ravel(), np.array([len(cases)], dtype=np.uint64)]
    for case in cases:
        words.append(np.array([case.degree_bits, case.num_wires, case.num_routed, case.num_targets, len(case.pairs)], dtype=np.uint64))
        words.append(k_is_of(F, case.num_routed).astype(np.uint64))
        words.append(case.pairs.ravel())
    return np.concatenate(words)
