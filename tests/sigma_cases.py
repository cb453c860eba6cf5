"""Sigmas built from explicit class lists, and what gb_circuit_decode_sigmas must read back out of them (no GPU code).

On top of oracle.plonk_dummy.DummyCircuit, the way tests/wired_circuits.py's wired_dummy_circuit does it: a class is a list of
routed cells of NoopGate rows, each cell col * n + row (sigma's own numbering), in the order sigma walks them - sigma(cell t) names
cell t + 1, the last names the first.  DummyCircuit wires one class of its own, {(pi_row, 0 .. H - 1), (const_row, 0)}, which
wired_dummy_circuit's `copy_classes` does not list: full_copy_classes adds it, so that labels, counts and a partition made from the
result describe ALL of the circuit's wiring, as the sigmas do."""
import numpy as np

from oracle import plonk_dummy as PD
from oracle.fields import GL
from plonky2_goldibear_amd import native as N


def dummy_class(circ):
    """DummyCircuit's own copy class, as col * n + row"""
    H = circ.F.hout
    return np.array([j * circ.n + circ.pi_row for j in range(H)] + [circ.const_row], dtype=np.int64)


def full_copy_classes(circ):
    """circ.copy_classes with the dummy circuit's own class behind them -> (cells, starts, sizes)"""
    cells, starts, sizes = circ.copy_classes
    own = dummy_class(circ)
    return (np.concatenate([np.asarray(cells, dtype=np.int64), own]), np.concatenate([starts, [len(cells)]]).astype(np.int64),
            np.concatenate([sizes, [len(own)]]).astype(np.int64))


def labels_of(classes, n, num_wires):
    """per wire cell row * num_wires + col: the lowest cell of its class; cells in no class label themselves"""
    cells, starts, sizes = classes
    col, row = np.divmod(np.asarray(cells, dtype=np.int64), n)
    idx = row * num_wires + col
    labels = np.arange(n * num_wires, dtype=np.int64)
    if len(idx):
        firsts = np.minimum.reduceat(idx, np.asarray(starts, dtype=np.int64))
        labels[idx] = np.repeat(firsts, sizes)
    return labels.astype(np.uint32)


def info_of(classes, n, num_routed):
    """the gb_sigma_info fields that depend on the classes alone"""
    sizes = np.asarray(classes[2], dtype=np.int64)
    big = sizes[sizes >= 2]
    return dict(routed_cells=n * num_routed, moved_cells=int(big.sum()), num_classes=int(big.size),
                largest_class=int(big.max()) if big.size else 1)


def circuit_from_classes(F, cfg, degree_bits, class_lists):
    """-> (oracle-side BuiltCircuit with copy_classes = the lists, keyword arguments of the GPU CircuitData)"""
    base = PD.DummyCircuit(degree_bits, cfg, F=F)
    n, nr, nw = base.n, cfg.num_routed_wires, cfg.num_wires
    cells = np.array([c for cl in class_lists for c in cl], dtype=np.int64)
    sizes = np.array([len(cl) for cl in class_lists], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    assert sizes.min() >= 1 and len(set(cells.tolist())) == cells.size and cells.max() < nr * n
    assert not np.isin(cells % n, [base.pi_row, base.const_row]).any(), "only NoopGate rows are free to wire"
    nxt = np.arange(1, cells.size + 1)
    nxt[starts + sizes - 1] = starts
    ident = base.sigma.ravel().copy()
    sigma = ident.copy()
    sigma[cells] = ident[cells[nxt]]
    constants_sigmas = np.concatenate([base.constants_sigmas[:base.num_constants], sigma.reshape(nr, n)]).astype(F.dtype)
    circ = PD.BuiltCircuit(cfg, F, degree_bits, constants_sigmas, base.k_is, base.gate_table, 1, 0)
    circ.pi_row, circ.const_row, circ.subgroup = base.pi_row, base.const_row, base.subgroup
    circ.copy_classes = (cells, starts, sizes)
    kw = dict(num_wires=nw, num_routed_wires=nr, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
              arity_bits=cfg.arity_bits, gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI,
              field=N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR)
    return circ, kw


AWKWARD = ("two_columns", "cycle_64", "cycle_65")


def awkward_classes(name, n, pi_row, const_row, seed=0xC1C1E):
    """class lists for 2^10 rows or more.  Always: a 2-cycle whose lowest cell in row * num_wires + col order - (wire 5, row 2) - is
    not its lowest in col * n + row order - (wire 4, row 9); a 2-cycle inside row 20 and one inside wire 8.  Then
      two_columns   one cycle through every NoopGate-row cell of wires 0 and 1 in seeded random order
      cycle_64      the longest cycle has exactly 2^6 cells (wires 2 and 3, seeded)
      cycle_65      the longest has 2^6 + 1"""
    rng = np.random.default_rng(seed)
    rows = np.array([r for r in range(n) if r not in (pi_row, const_row)], dtype=np.int64)
    out = [[5 * n + 2, 4 * n + 9], [6 * n + 20, 7 * n + 20], [8 * n + 30, 8 * n + 31]]
    if name == "two_columns":
        cells = np.concatenate([rows, n + rows])
        out.append(cells[rng.permutation(cells.size)].tolist())
    else:
        cells = np.concatenate([2 * n + rows, 3 * n + rows])
        out.append(cells[rng.permutation(cells.size)][:64 if name == "cycle_64" else 65].tolist())
    return out


class SmallRoutedCircuit:
    """2^degree_bits NoopGate rows with fewer routed wires than DummyCircuit's public-input row needs: every routed cell is in a
    seeded random class of 1 to 5 cells.  Nothing is proved on it; it has the attributes the decode tests read."""

    def __init__(self, F, degree_bits=4, num_routed=3, num_wires=5, seed=3):
        self.F, self.degree_bits, self.n = F, degree_bits, 1 << degree_bits
        self.cfg = PD.CircuitConfig(num_challenges=2 if F is GL else 6, num_wires=num_wires, num_routed_wires=num_routed,
                                    arity_bits=4 if F is GL else 3)
        n, p = self.n, F.P
        rng = np.random.default_rng(seed)
        self.k_is = np.array([pow(F.generator, i, p) for i in range(num_routed)], dtype=F.dtype)
        w, sub = F.two_adic_generator(degree_bits), [1] * n
        for i in range(1, n):
            sub[i] = sub[i - 1] * w % p
        ident = np.array([int(k) * s % p for k in self.k_is for s in sub], dtype=F.dtype)
        cells = rng.permutation(num_routed * n).astype(np.int64)
        sizes = rng.integers(1, 6, size=cells.size)
        sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells.size)) + 1]
        sizes[-1] -= int(sizes.sum()) - cells.size
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        nxt = np.arange(1, cells.size + 1)
        nxt[starts + sizes - 1] = starts
        sigma = ident.copy()
        sigma[cells] = ident[cells[nxt]]
        self.copy_classes = (cells, starts, sizes.astype(np.int64))
        self.constants_sigmas = np.concatenate([np.zeros((1 + self.cfg.num_constants, n), dtype=F.dtype), sigma.reshape(num_routed, n)])
        self.gpu_kwargs = dict(num_wires=num_wires, num_routed_wires=num_routed, num_constants=self.cfg.num_constants,
                               num_challenges=self.cfg.num_challenges, arity_bits=self.cfg.arity_bits, gate_constant=1, gate_pi=2,
                               field=N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR)


class SingleWireCircuit:
    """2^degree_bits NoopGate rows of ONE wire, routed: sigma is the identity but for `num_cycles` seeded cycles of 2 to 5 rows and
    one of `long_cycle` rows.  For the sizes at which the decode kernel reads its tables from global memory, where a circuit of
    the usual width would not fit a test; vectorised, nothing is proved on it."""

    def __init__(self, F, degree_bits, num_cycles=1000, long_cycle=300, seed=5):
        self.F, self.degree_bits, self.n = F, degree_bits, 1 << degree_bits
        need = -(-100 // (F.order_bits - degree_bits))      # circuit_builder.rs:1191-1192
        self.cfg = PD.CircuitConfig(num_challenges=max(need, 2 if F is GL else 6), num_wires=1, num_routed_wires=1,
                                    arity_bits=4 if F is GL else 3)
        n = self.n
        rng = np.random.default_rng(seed)
        self.k_is = np.array([1], dtype=F.dtype)
        ident = F.mod.powers(F.two_adic_generator(degree_bits), n)
        sizes = np.concatenate([[long_cycle], rng.integers(2, 6, size=num_cycles)]).astype(np.int64)
        cells = np.concatenate([[0, n - 1], 1 + rng.choice(n - 2, size=int(sizes.sum()) - 2, replace=False)]).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        nxt = np.arange(1, cells.size + 1)
        nxt[starts + sizes - 1] = starts
        sigma = ident.copy()
        sigma[cells] = ident[cells[nxt]]
        self.copy_classes = (cells, starts, sizes)
        self.constants_sigmas = np.concatenate([np.zeros((1 + self.cfg.num_constants, n), dtype=F.dtype), sigma[None, :]])
        self.gpu_kwargs = dict(num_wires=1, num_routed_wires=1, num_constants=self.cfg.num_constants,
                               num_challenges=self.cfg.num_challenges, arity_bits=self.cfg.arity_bits, gate_constant=1, gate_pi=2,
                               field=N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR)
