"""Dense, carry-edge inputs for the prover tests (no GPU code).

oracle/plonk_dummy.py's DummyCircuit proves an all-zero witness under a sigma that is the identity on all but H + 1 cells: on
every other row the permutation argument's numerator w + beta k_j x + gamma and denominator w + beta sigma_j + gamma are the same
word, every chunk quotient is 1 and Z is 1.  Here the same gate set gets real wiring - every routed cell of a NoopGate row joins
a seeded random copy class - and a witness that is constant on each class, with values from the fields' carry edges or from the
SplitMix64 stream; and the permutation argument is restated on Python integers (zs_partial_products_ref), so that the stage can
be checked at challenges chosen for the additions they cause, not only at the transcript's."""
import numpy as np

from oracle import plonk_dummy as PD
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N


def edge_values(F):
    """canonical field elements on the edges of the device arithmetic's carries and selections"""
    p = F.P
    if F is GL:
        return [0, 1, 2, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**48, 2**63, p - 2**32, p - 2**32 + 1, (p - 1) // 2, (p + 1) // 2,
                p - 2, p - 1]
    r_inv = pow(2**32, p - 2, p)   # the device keeps BabyBear as Montgomery words x 2^32 mod p
    return ([0, 1, 2, 2**27, 2**27 + 1, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1] +
            [word * r_inv % p for word in bb_edge_words()])


def bb_edge_words():
    """the device (Montgomery) words that edge_values(BB) adds to its canonical edges"""
    p = BB.P
    return [1, 2, 2**27, p - 2, p - 1]


def _values(F, dense, seed, count, start=0):
    if dense == "edges":
        ev = np.array(edge_values(F), dtype=F.dtype)
        return ev[(start + np.arange(count)) % len(ev)]
    assert dense == "random", dense
    return F.fill(seed, count)


def wired_dummy_circuit(F, cfg, degree_bits, seed, dense="edges"):
    """-> (oracle-side BuiltCircuit, witness [num_wires][n], keyword arguments of the GPU CircuitData).

    DummyCircuit's constants, selector, public-input and constant rows; every routed cell of a NoopGate row (those after the
    constant row too) is put into a seeded random copy class of 1 to 5 cells, sigma(cell) = k_is[col'] * subgroup[row'] of the
    class's next cell.  The witness is constant on each class: class t holds edge_values[t mod len] (dense="edges") or the t-th
    F.fill value (dense="random"); the non-routed wires of the NoopGate rows hold independent values of the same kind.  The circuit
    carries `copy_classes`: (cells, starts, sizes) with cells[starts[t] : starts[t] + sizes[t]] = class t as col * n + row."""
    base = PD.DummyCircuit(degree_bits, cfg, F=F)
    n, nr, nw = base.n, cfg.num_routed_wires, cfg.num_wires
    rng = np.random.default_rng(seed)
    noop = np.ones(n, dtype=bool)
    noop[[base.pi_row, base.const_row]] = False
    noop_rows = np.flatnonzero(noop)
    cells = (np.arange(nr)[:, None] * n + noop_rows[None, :]).ravel()
    cells = cells[rng.permutation(cells.size)]
    sizes = rng.integers(1, 6, size=cells.size)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), cells.size)) + 1]
    sizes[-1] -= int(sizes.sum()) - cells.size
    assert sizes.sum() == cells.size and sizes.min() >= 1 and sizes.max() <= 5
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    nxt = np.arange(1, cells.size + 1)
    nxt[starts + sizes - 1] = starts                       # the last cell of a class points back to its first
    ident = base.sigma.ravel().copy()                      # k_is[col] * subgroup[row] on every NoopGate row
    sigma = ident.copy()
    sigma[cells] = ident[cells[nxt]]
    sigma = sigma.reshape(nr, n)
    nconst = base.num_constants
    constants_sigmas = np.concatenate([base.constants_sigmas[:nconst], sigma]).astype(F.dtype)
    circ = PD.BuiltCircuit(cfg, F, degree_bits, constants_sigmas, base.k_is, base.gate_table, 1, 0)
    circ.pi_row, circ.const_row, circ.subgroup = base.pi_row, base.const_row, base.subgroup
    circ.copy_classes = (cells, starts, sizes)

    w = base.witness(seed=seed)
    class_of = np.repeat(np.arange(sizes.size), sizes)
    routed = w[:nr].reshape(-1)
    routed[cells] = _values(F, dense, 0x5EED0000 + seed, sizes.size)[class_of]
    w[:nr] = routed.reshape(nr, n)
    free = _values(F, dense, 0x5EED8000 + seed, (nw - nr) * noop_rows.size, start=7).reshape(nw - nr, noop_rows.size)
    w[nr:, noop_rows] = free
    gpu_kwargs = dict(num_wires=nw, num_routed_wires=nr, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                      arity_bits=cfg.arity_bits, gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI,
                      field=N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR)
    return circ, w, gpu_kwargs


def class_member(circ, min_size=2):
    """(col, row) of one cell of the first copy class with at least min_size cells"""
    cells, starts, sizes = circ.copy_classes
    t = int(np.flatnonzero(sizes >= min_size)[0])
    return divmod(int(cells[starts[t]]), circ.n)


def break_copy_constraint(circ, witness):
    """a copy of the witness with one cell of a class of at least two cells changed"""
    col, row = class_member(circ)
    bad = witness.copy()
    bad[col, row] = (int(bad[col, row]) + 1) % circ.F.P
    return bad


CENSUS_CLASSES = ("below_p", "equal_p", "between", "equal_top", "above_top")


def zs_partial_products_ref(F, witness, sigma, k_is, betas, gammas, degree_bits, chunk):
    """all_wires_permutation_partial_products (plonk/prover.rs:305-329, 478-560) on Python integers.

    Per row x = subgroup[row] and challenge: numerators w_j + beta k_j x + gamma and denominators w_j + beta sigma_j[row] + gamma
    over the routed wires, the chunk quotients prod(numerators) * pow(prod(denominators), p - 2, p) per `chunk` wires, Z as the
    exclusive prefix product of the rows' quotients, the partial products Z * q_0 .. q_m.  -> (values, census): values is
    [c * nchunks][n] in k_zs_finalize's column order (every Z, then each challenge's nchunks - 1 partial products); census counts
    the base-field additions w + gamma by the integer sum s of the DEVICE words (canonical u64 for Goldilocks, top = 2^64;
    Montgomery words for BabyBear, top = 2p): s < p, s = p, p < s < top, s = top, s > top.  Raises ZeroDivisionError on a zero
    denominator (ProverError::InvZeroPermArg)."""
    from collections import Counter
    p, n = F.P, 1 << degree_bits
    nr = len(k_is)
    c, nchunks = len(betas), -(-nr // chunk)
    k_is = [int(k) for k in k_is]
    wrows = [[int(v) for v in r] for r in np.asarray(witness)[:nr].T]
    srows = [[int(v) for v in r] for r in np.asarray(sigma).T]
    spans = [(m * chunk, min((m + 1) * chunk, nr)) for m in range(nchunks)]
    g = F.two_adic_generator(degree_bits)
    sub = [1] * n
    for i in range(1, n):
        sub[i] = sub[i - 1] * g % p
    if F is GL:
        top, word = 1 << 64, lambda v: v
    else:
        top, word = 2 * p, lambda v: (v << 32) % p
    census = dict.fromkeys(CENSUS_CLASSES, 0)
    wwords = Counter(word(v) for r in wrows for v in r)
    out = np.zeros((c * nchunks, n), dtype=F.dtype)
    for i, (beta, gamma) in enumerate(zip(betas, gammas)):
        beta, gamma = int(beta), int(gamma)
        gword = word(gamma)
        for v, count in wwords.items():
            s = v + gword
            census[CENSUS_CLASSES[(s >= p) + (s > p) + (s >= top) + (s > top)]] += count
        z = 1
        for row in range(n):
            bx = beta * sub[row] % p
            wr, sr = wrows[row], srows[row]
            acc = z
            out[i, row] = z
            for m, (j0, j1) in enumerate(spans):
                num = den = 1
                for wv, sv, k in zip(wr[j0:j1], sr[j0:j1], k_is[j0:j1]):
                    wg = wv + gamma
                    num = num * (wg + bx * k) % p
                    den = den * (wg + beta * sv) % p
                if den == 0:   # p is prime: some factor w_j + beta sigma_j + gamma is 0 mod p
                    raise ZeroDivisionError("InvZeroPermArg: challenge %d, row %d, wires %d..%d" % (i, row, j0, j1 - 1))
                acc = acc * num % p * pow(den, p - 2, p) % p
                if m < nchunks - 1:
                    out[c + i * (nchunks - 1) + m, row] = acc
            z = acc
    return out, census


def horner_ext(F, coeffs, z):
    """p.to_extension().eval(z) (plonk/proof.rs:359-363) by Horner's rule in oracle/fields.py's extension arithmetic"""
    z = tuple(int(x) for x in z)
    acc = F.zero
    for t in range(len(coeffs) - 1, -1, -1):
        acc = F.eadd(F.emul(z, acc), F.efrom(int(coeffs[t])))
    return acc
