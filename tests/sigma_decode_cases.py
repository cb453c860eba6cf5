"""The case table of csrc/sigma_decode.hpp for tests/host_shim/sigma_decode.cpp (CPU) and tests/device/sigma_decode.hip (gfx950):
sigma values to decode and the cell each names, from Python integers (pow) - never from the code under test.  No GPU code."""
import numpy as np

from oracle.fields import BB, GL

FIELDS = {"goldilocks": GL, "babybear": BB}
NO_CELL = None
SEED = 0x51634A


def low_bits(lg):
    return (lg + 1) // 2


def expect(F, lg, k_is, v):
    """(col', row') with v = k_is[col'] w^row', or NO_CELL - by exhaustive search over H (small lg only)"""
    p, n = F.P, 1 << lg
    vn = pow(v, n, p)
    cols = [j for j, k in enumerate(k_is) if pow(k, n, p) == vn]
    if not cols:
        return NO_CELL
    x = v * pow(k_is[cols[0]], p - 2, p) % p
    w, y = F.two_adic_generator(lg), 1
    for row in range(n):
        if y == x:
            return cols[0], row
        y = y * w % p
    raise AssertionError("an n-th root of unity outside H")


def case(F, lg, k_is, values, expected, raw=False):
    p, n = F.P, 1 << lg
    k_is = [int(k) for k in k_is]
    return dict(lg=lg, k_is=k_is, values=[int(v) for v in values], expected=list(expected), raw=raw,
                distinct=all(k % p for k in k_is) and len({pow(k, n, p) for k in k_is}) == len(k_is))


def cases(F):
    p, g = F.P, F.generator
    rng = np.random.default_rng(SEED)
    out = []
    # every element of H, lg 1 .. 12
    for lg in range(1, 13):
        w, n = F.two_adic_generator(lg), 1 << lg
        vals, x = [], 1
        for _ in range(n):
            vals.append(x)
            x = x * w % p
        out.append(case(F, lg, [1], vals, [(0, r) for r in range(n)]))
    # large groups: the rows around the split lg = a + b and 256 seeded ones
    for lg in [13, 20, 27] + ([32] if F is GL else []):
        w, n, a = F.two_adic_generator(lg), 1 << lg, low_bits(lg)
        rows = [0, 1, (1 << a) - 1, 1 << a, n // 2, n - 1] + [int(r) for r in rng.integers(0, n, size=256)]
        out.append(case(F, lg, [1], [pow(w, r, p) for r in rows], [(0, r) for r in rows]))
    # the coset match: every column of R = 1, 3, 80 routed wires, a few rows each; once in a group past the 12 bits
    for nr, lg in [(1, 5), (3, 5), (80, 5), (80, 16)]:
        w, n = F.two_adic_generator(lg), 1 << lg
        k_is = [pow(g, i, p) for i in range(nr)]
        cells = [(c, r) for c in range(nr) for r in sorted({0, 1, n - 1, (7 * c + 3) % n})]
        out.append(case(F, lg, k_is, [k_is[c] * pow(w, r, p) % p for c, r in cells], cells))
    # no cell: 0, g^R w, a value of H times a shift that is in no routed coset - between values that are cells
    lg, nr = 5, 3
    w, n = F.two_adic_generator(lg), 1 << lg
    k_is = [pow(g, i, p) for i in range(nr)]
    outside = [0, pow(g, nr, p) * w % p, pow(w, 9, p) * pow(g, nr + 7, p) % p]
    inside = [k_is[2] * pow(w, 9, p) % p, k_is[0]]
    vals = [inside[0]] + outside + [inside[1]]
    want = [expect(F, lg, k_is, v) for v in vals]
    assert want == [(2, 9), NO_CELL, NO_CELL, NO_CELL, (0, 0)]
    out.append(case(F, lg, k_is, vals, want))
    if F is BB:
        mont = [(v << 32) % p for v in vals]
        # the device words themselves: the same elements, the same answers
        out.append(case(F, lg, k_is, mont, want, raw=True))
        # the Montgomery words read as canonical values: other elements - whatever Python says they are
        out.append(case(F, lg, k_is, mont, [expect(F, lg, k_is, v) for v in mont]))
    # k_is that name a coset twice (entry 1 = entry 0 times w), and a zero entry: refused by the table builder
    out.append(case(F, lg, [k_is[0], k_is[0] * w % p, k_is[2]], [], []))
    out.append(case(F, lg, [k_is[0], 0, k_is[2]], [], []))
    assert [c["distinct"] for c in out[-2:]] == [False, False] and all(c["distinct"] for c in out[:-2])
    return out


def pack(F, table):
    words = [0 if F is GL else 1, len(table)]
    for c in table:
        words += [c["lg"], len(c["k_is"]), int(c["raw"]), len(c["values"])] + c["k_is"] + c["values"]
    return np.array(words, dtype=np.uint64)


def compare(table, out):
    """-> a list of differences between the program's output words and the table"""
    bad, pos = [], 0
    out = [int(x) for x in out]
    for i, c in enumerate(table):
        if pos >= len(out):
            return bad + ["case %d: the output ends early" % i]
        if out[pos] != int(c["distinct"]):
            bad.append("case %d (lg %d): distinct cosets %d, expected %d" % (i, c["lg"], out[pos], c["distinct"]))
        pos += 1
        for v, want in zip(c["values"], c["expected"]):
            got = None if out[pos] == 2**64 - 1 else (out[pos], out[pos + 1])
            pos += 2
            if got != want:
                bad.append("case %d (lg %d, %d routed): value %d decodes to %r, expected %r" % (i, c["lg"], len(c["k_is"]), v, got, want))
    if pos != len(out):
        bad.append("%d output words, expected %d" % (len(out), pos))
    return bad
