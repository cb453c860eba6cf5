"""Constraint systems for the gb_constraint_quotient / gb_constraint_eval tests, and the expected quotient on Python integers
(no GPU code, not a test file; imports from oracle/ only - the programs are handed in and only their `evaluate`, `cells` and
`num_constraints` are used).

The expected result, the same way every time (expected_chunks): the oracle's LDE of the committed columns; the programs' evaluate()
on Python integers at every point of the quotient domain; the fold with the powers of alpha; the division by Z_H; the oracle's
coset inverse transform; the split into chunks.  Equal byte for byte - nothing here has a tolerance.
"""
import numpy as np

from oracle.fields import BB, GL  # noqa: F401


def reverse_bits(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def lde_natural(F, values, rate_bits, salts=None):
    """the oracle's commitment of [ncols][n] values -> (batch, lde) with lde[col][i] = P_col(g w_N^i) as Python ints"""
    batch = F.mod.PolynomialBatch.from_values(np.ascontiguousarray(values, dtype=F.dtype), rate_bits, 0, salts)
    bits = batch.degree_log + rate_bits
    order = [reverse_bits(i, bits) for i in range(1 << bits)]
    ncols = len(values)
    lde = [[int(v) for v in batch.leaves[order, c]] for c in range(ncols)]
    return batch, lde


def quotient_points(F, degree_bits, qb):
    """x_i = g w_Q^i, i < n 2^qb"""
    w = F.two_adic_generator(degree_bits + qb)
    xs, x = [], F.generator
    for _ in range(1 << (degree_bits + qb)):
        xs.append(x)
        x = x * w % F.P
    return xs


def batch_inverse(F, vals):
    """1 / v for every v (none zero): one inversion and three products each"""
    P, pre, acc = F.P, [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % P
    inv, out = F.finv(acc), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * vals[i] % P
    return out


def l_first_table(F, degree_bits, xs):
    """L_0(x) = Z_H(x) / (n (x - 1)) for every x of xs"""
    n, P = 1 << degree_bits, F.P
    den = batch_inverse(F, [n * (x - 1) % P for x in xs])
    return [(pow(x, n, P) - 1) * d % P for x, d in zip(xs, den)]


def constraint_values(F, programs, ldes, degree_bits, rate_bits, qb, params):
    """every constraint of every program at every point of the quotient domain: [n 2^qb][total constraints] Python ints.
    ldes[o]: lde_natural's table of oracle o (rate 2^rate_bits)."""
    Q = 1 << (degree_bits + qb)
    step = 1 << (rate_bits - qb)
    xs = quotient_points(F, degree_bits, qb)
    lf = l_first_table(F, degree_bits, xs)
    out = []
    for i, x in enumerate(xs):
        row = []
        for pr in programs:
            cells = [ldes[o][k][((i + (off << qb)) % Q) * step] for o, k, off in pr.cells]
            row += pr.evaluate(cells, params, x, lf[i], lf[(i + (1 << qb)) % Q])   # L_last(x) = L_first(w_n x): the next row's point
        out.append(row)
    return out


def coset_ifft(F, values):
    """PolynomialValues::coset_ifft(F::generator()) through the oracle's ifft: coefficients of the polynomial with these values on g H"""
    coeffs = F.mod.ifft(np.array(values, dtype=F.dtype))
    g_inv, s, out = F.finv(F.generator), 1, []
    for c in coeffs:
        out.append(int(c) * s % F.P)
        s = s * g_inv % F.P
    return out


def expected_chunks(F, cons, degree_bits, qb, alphas):
    """cons: constraint_values' table -> [len(alphas) 2^qb][n] array of the field's dtype"""
    P, n = F.P, 1 << degree_bits
    xs = quotient_points(F, degree_bits, qb)
    zh_inv = [F.finv((pow(x, n, P) - 1) % P) for x in xs[:1 << qb]]   # Z_H(g w_Q^i) depends on i mod 2^qb only
    rows = []
    for a in alphas:
        q = []
        for i, row in enumerate(cons):
            acc = 0
            for c in reversed(row):
                acc = (acc * a + c) % P
            q.append(acc * zh_inv[i & ((1 << qb) - 1)] % P)
        coeffs = coset_ifft(F, q)
        rows += [coeffs[m * n:(m + 1) * n] for m in range(1 << qb)]
    return np.array(rows, dtype=F.dtype)


def subsample(cons, qb_from, qb_to):
    """the table of the 2^qb_to-blow-up domain out of the one of the 2^qb_from domain (the smaller domain is every 2^(from - to)-th point)"""
    return cons[::1 << (qb_from - qb_to)]


# ----------------------------------------------------------------------------- extension-field evaluation
def eval_poly_ext(F, coeffs, z):
    acc = F.zero
    for c in reversed([int(v) for v in coeffs]):
        acc = F.eadd(F.emul(acc, z), F.efrom(c))
    return acc


def ext_inputs(F, degree_bits, zeta):
    """(Z_H(zeta), L_first(zeta), L_last(zeta)) as extension elements"""
    n = 1 << degree_bits
    zh = F.esub(F.epow(zeta, n), F.one)

    def l0(x):
        return F.emul(zh, F.einv(F.escale(F.esub(x, F.one), n)))
    return zh, l0(zeta), l0(F.escale(zeta, F.two_adic_generator(degree_bits)))


class ExtInt:
    """an extension element that ConstraintProgram.evaluate's integer arithmetic (+ - * %, int()) runs on"""
    __slots__ = ("F", "v")

    def __init__(self, F, v):
        self.F, self.v = F, tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else F.efrom(int(v))

    def _c(self, o):
        return o if isinstance(o, ExtInt) else ExtInt(self.F, o)

    def __add__(self, o):
        return ExtInt(self.F, self.F.eadd(self.v, self._c(o).v))

    __radd__ = __add__

    def __sub__(self, o):
        return ExtInt(self.F, self.F.esub(self.v, self._c(o).v))

    def __rsub__(self, o):
        return ExtInt(self.F, self.F.esub(self._c(o).v, self.v))

    def __mul__(self, o):
        return ExtInt(self.F, self.F.emul(self.v, self._c(o).v))

    __rmul__ = __mul__

    def __mod__(self, p):
        return self

    def __int__(self):
        raise TypeError("an extension element is no integer")


def fold_ext(F, cons, alpha):
    acc = F.zero
    for c in reversed(cons):
        acc = F.eadd(F.escale(acc, alpha), c)
    return acc


def quotient_at(F, chunks, degree_bits, zeta):
    """sum_i zeta^(n i) chunk_i(zeta) for the chunks of one challenge"""
    zn = F.epow(zeta, 1 << degree_bits)
    acc = F.zero
    for ch in reversed(list(chunks)):
        acc = F.eadd(F.emul(acc, zn), eval_poly_ext(F, ch, zeta))
    return acc


# ----------------------------------------------------------------------------- the Fibonacci trace
def fibonacci_trace(F, degree_bits, a0, a1):
    """two columns: row r holds (f_r, f_(r+1)), f_0 = a0, f_1 = a1"""
    a, b, cols = a0 % F.P, a1 % F.P, ([], [])
    for _ in range(1 << degree_bits):
        cols[0].append(a)
        cols[1].append(b)
        a, b = b, (a + b) % F.P
    return np.array(cols, dtype=F.dtype)


FIB_CELLS = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)]


def fibonacci_constraints(F, degree_bits):
    """fn for ConstraintProgram.from_constraints over FIB_CELLS, params (a0, a1): the transitions hold on every row but the last
    (times X - w^(n-1)), the first row holds the params (times L_first)"""
    w_last = pow(F.two_adic_generator(degree_bits), (1 << degree_bits) - 1, F.P)

    def fn(cell, param, x, l_first, l_last):
        return [(x - w_last) * (cell[2] - cell[1]), (x - w_last) * (cell[3] - cell[0] - cell[1]),
                l_first * (cell[0] - param[0]), l_first * (cell[1] - param[1])]
    return fn
