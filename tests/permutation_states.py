"""Inputs that put a CHOSEN word in front of a chosen s-box or linear layer of Poseidon-12 (Goldilocks) and Poseidon2-16 (BabyBear).

A pattern at the input of a permutation does not survive the first constant layer, so neither the s-boxes nor the byte-plane cuts,
MFMA chains, row sums and lazy-offset rounds behind it ever see it.  The permutations are bijections: a state at any place inside
can be pulled back - inverse linear layer (Gaussian elimination mod p), inverse s-box x^(7^-1 mod p-1), minus the constants - to
the input that produces it.  This module holds round-by-round models of both permutations on Python integers (constants read from
csrc/poseidon_constants.h, linear layers restated from csrc/poseidon_gl_host.hpp / poseidon2_bb_host.hpp: circ + diag, M_E, M_I),
their inverses, and seeded lists of such inputs.  It chooses INPUTS only: every expected output in the tests comes from the oracle.

Places.  Round r of Poseidon-12 is r = 0..29 (4 full, 22 partial, 4 full); of Poseidon2, r = 0..20 (external 0..3, internal 4..16,
external 17..20, the initial M_E in front of round 0).  `sbox_in` is the state after round r's constants, `mds_in` the state after
round r's s-boxes; in partial / internal rounds only word 0 goes through the s-box.

Targets are DEVICE words where the device header defines the form:
  * Goldilocks (csrc/poseidon_gl.hpp): the state is in Montgomery form, word = value * 2^64 mod p.  A word W in [2^32 - 1, p) has
    one u64 representative (W + p does not fit), so a register that holds the value holds exactly W.  For W < 2^32 - 1 both W and
    W + p are representatives and the target is the VALUE only.  The grouped and cooperative forms materialise only word 0 inside
    the partial rounds (the rest lives in a sparse / pending form), hence the "word 0 only" shape there.
  * BabyBear (csrc/poseidon2_bb.hpp): word = kappa * 2^32 * value mod p with the scale kappa that make_plan tracks (restated in
    bb_scales).  The words are signed (within +-1.03 p) or lazy (in (0, 2p), or below LAZY_MAX with a per-round offset on words
    1..15 of the internal rounds), so the representative is never unique: the target is the value whose word is CONGRUENT to W.
Every Target records place, shape, the intended words and the true values; tests/test_permutation_states.py runs each input forward
and checks that it arrives.

Not a test file.  Generation of all lists takes a few seconds; the lists are cached."""
import functools
import os
import random
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "plonky2_goldibear_amd", "csrc", "poseidon_constants.h")

GL, BB = "goldilocks", "babybear"
GL_P = 0xFFFFFFFF00000001
BB_P = 2013265921
SBOX_IN, MDS_IN = "sbox_in", "mds_in"


def grab(name):
    """the numbers of a *_LIST macro of csrc/poseidon_constants.h (as tools/gen_poseidon_groups.py reads them)"""
    text = open(HDR).read()
    m = re.search(r"#define " + name + r"_LIST \\\n((?:.*\\\n)*.*)\n", text)
    return [int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\b\d+\b", re.sub(r"ULL|u\b", "", m.group(1)))]


# ------------------------------------------------------------------ linear algebra mod p
def mat_vec(m, v, p):
    return [sum(a * b for a, b in zip(row, v)) % p for row in m]


def solve(m, rhs, p):
    """x with m x = rhs (mod p) by Gaussian elimination, or None when m is singular"""
    n = len(m)
    a = [list(row) + [r] for row, r in zip(m, rhs)]
    for c in range(n):
        piv = next((r for r in range(c, n) if a[r][c] % p), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, p)
        a[c] = [x * inv % p for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % p for x, y in zip(a[r], a[c])]
    return [a[r][n] for r in range(n)]


def inverse(m, p):
    n = len(m)
    cols = [solve(m, [int(i == j) for i in range(n)], p) for j in range(n)]
    assert all(c is not None for c in cols), "singular linear layer"
    return [[cols[j][i] for j in range(n)] for i in range(n)]


def matrix_of(layer, n, p):
    """the matrix of a linear map given as a function on lists"""
    cols = [layer([int(i == j) for i in range(n)]) for j in range(n)]
    return [[cols[j][i] % p for j in range(n)] for i in range(n)]


# ------------------------------------------------------------------ Poseidon-12 over Goldilocks
class Poseidon12:
    field, p, width, rounds = GL, GL_P, 12, 30

    def __init__(self):
        circ, diag = grab("GL_POSEIDON_MDS_CIRC"), grab("GL_POSEIDON_MDS_DIAG")
        self.rc = grab("GL_POSEIDON_ALL_ROUND_CONSTANTS")
        assert len(circ) == 12 and len(diag) == 12 and len(self.rc) == 360
        # csrc/poseidon_gl_host.hpp / poseidon_gl.hpp: res[q] = sum_i s[(i + q) % 12] CIRC[i] + s[q] DIAG[q]
        self.m = [[circ[(i - q) % 12] + (diag[q] if i == q else 0) for i in range(12)] for q in range(12)]
        self.m_inv = inverse(self.m, self.p)
        self.inv7 = pow(7, -1, self.p - 1)

    def is_full(self, r):
        return r < 4 or r >= 26

    def add_constants(self, s, r, sign=1):
        return [(x + sign * self.rc[12 * r + i]) % self.p for i, x in enumerate(s)]

    def first_layer(self, s):                          # nothing in front of round 0
        return list(s)

    def first_layer_inv(self, s):
        return list(s)

    def linear(self, s, r):
        return mat_vec(self.m, s, self.p)

    def linear_inv(self, s, r):
        return mat_vec(self.m_inv, s, self.p)

    def scale(self, r, where):
        """device word = scale * value mod p at (r, where)"""
        return (1 << 64) % self.p

    def unique_word(self, w):
        return (1 << 32) - 1 <= w < self.p


# ------------------------------------------------------------------ Poseidon2-16 over BabyBear
BB_SHIFTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]


class Poseidon2:
    field, p, width, rounds = BB, BB_P, 16, 21

    def __init__(self):
        p = self.p
        self.ext, self.int = grab("BB_POSEIDON2_EXTERNAL_CONSTANTS"), grab("BB_POSEIDON2_INTERNAL_CONSTANTS")
        assert len(self.ext) == 128 and len(self.int) == 13
        self.m_e = matrix_of(self.external_layer, 16, p)
        self.m_i = matrix_of(self.internal_layer, 16, p)
        self.m_e_inv, self.m_i_inv = inverse(self.m_e, p), inverse(self.m_i, p)
        self.inv7 = pow(7, -1, p - 1)
        self.scales = bb_scales()

    def external_layer(self, s):
        """M_E (csrc/poseidon2_bb_host.hpp external_layer): [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]] per block of four, then
        every word gets the sum of its column class"""
        p, n = self.p, []
        for b in range(0, 16, 4):
            x0, x1, x2, x3 = s[b:b + 4]
            n += [2 * x0 + 3 * x1 + x2 + x3, x0 + 2 * x1 + 3 * x2 + x3, x0 + x1 + 2 * x2 + 3 * x3, 3 * x0 + x1 + x2 + 2 * x3]
        sums = [n[k] + n[4 + k] + n[8 + k] + n[12 + k] for k in range(4)]
        return [(n[i] + sums[i & 3]) % p for i in range(16)]

    def internal_layer(self, s):
        """M_I (internal_layer): s *= 2^-32; full = sum s; s_0 <- full - 2 s_0; s_i <- full + 2^shift_(i-1) s_i"""
        p = self.p
        s = [x * pow(1 << 32, -1, p) % p for x in s]
        full = sum(s) % p
        return [(full - 2 * s[0]) % p] + [(full + (s[i + 1] << BB_SHIFTS[i])) % p for i in range(15)]

    def is_full(self, r):
        return r < 4 or r >= 17

    def add_constants(self, s, r, sign=1):
        p = self.p
        if self.is_full(r):
            e = r if r < 4 else r - 13
            return [(x + sign * self.ext[16 * e + i]) % p for i, x in enumerate(s)]
        return [(s[0] + sign * self.int[r - 4]) % p] + list(s[1:])

    def first_layer(self, s):
        return self.external_layer(s)

    def first_layer_inv(self, s):
        return mat_vec(self.m_e_inv, s, self.p)

    def linear(self, s, r):
        return self.external_layer(s) if self.is_full(r) else self.internal_layer(s)

    def linear_inv(self, s, r):
        return mat_vec(self.m_e_inv if self.is_full(r) else self.m_i_inv, s, self.p)

    def scale(self, r, where):
        return self.scales[(r, where)]

    def unique_word(self, w):
        return False


def bb_scales():
    """(round, place) -> the factor between a true value and the device word of csrc/poseidon2_bb.hpp at that place, mod p:
    kappa * 2^32 with the kappa sequence of plan::make_plan restated.  An external layer is one Montgomery reduction (kappa / R),
    an s-box is kappa^7; inside the internal rounds the state stays at one common scale (the single s-box is followed by a
    multiplication by kappa^-6), so `mds_in` of an internal round is kappa^7 for word 0 - the s-box's output as sbox7 leaves it."""
    p = BB_P
    big_r = (1 << 32) % p
    r_inv = pow(big_r, -1, p)
    out = {}
    k = r_inv                                  # Montgomery input (kappa = 1) through the initial layer
    for r in range(4):
        out[(r, SBOX_IN)] = k * big_r % p
        k = pow(k, 7, p)
        out[(r, MDS_IN)] = k * big_r % p
        k = k * r_inv % p
    for r in range(4, 17):
        out[(r, SBOX_IN)] = k * big_r % p
        out[(r, MDS_IN)] = pow(k, 7, p) * big_r % p
    for r in range(17, 21):
        out[(r, SBOX_IN)] = k * big_r % p
        k = pow(k, 7, p)
        out[(r, MDS_IN)] = k * big_r % p
        k = k * r_inv % p
    out["final"] = k * big_r % p               # what renorm / canonical_out divide out
    return out


@functools.lru_cache(maxsize=None)
def model(field):
    return Poseidon12() if field == GL else Poseidon2()


# ------------------------------------------------------------------ forward and backward
def _sboxes(m, s, r, e):
    if m.is_full(r):
        return [pow(x, e, m.p) for x in s]
    return [pow(s[0], e, m.p)] + list(s[1:])


def forward_to(field, state, r, where):
    """the state at (round r, where) on the way from the input `state`"""
    m = model(field)
    s = m.first_layer([int(x) % m.p for x in state])
    for q in range(r + 1):
        s = m.add_constants(s, q)
        if q == r and where == SBOX_IN:
            return s
        s = _sboxes(m, s, q, 7)
        if q == r:
            assert where == MDS_IN
            return s
        s = m.linear(s, q)


def permute(field, state):
    """the whole permutation, round by round"""
    m = model(field)
    return m.linear(forward_to(field, state, m.rounds - 1, MDS_IN), m.rounds - 1)


def back_to_input(field, target_state, r, where):
    """the input whose state at (round r, where) is `target_state` (true values, not device words)"""
    m = model(field)
    s = [int(x) % m.p for x in target_state]
    if where == MDS_IN:
        s = _sboxes(m, s, r, m.inv7)
    else:
        assert where == SBOX_IN
    s = m.add_constants(s, r, -1)
    for q in range(r - 1, -1, -1):
        s = m.linear_inv(s, q)
        s = _sboxes(m, s, q, m.inv7)
        s = m.add_constants(s, q, -1)
    return m.first_layer_inv(s)


def value_of_word(field, word, r, where):
    m = model(field)
    return word * pow(m.scale(r, where), -1, m.p) % m.p


# ------------------------------------------------------------------ the word sets
GL_WORDS = [0, 1, 0xFFFFFFFF, 0x100000000, GL_P - 1, 0xFFFFFFFEFFFFFFFF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0x00FF00FF00FF00FF,
            0xFF00FF00FF00FF00, 0x80007FFF0100FF80, (GL_P - 1) // 2]
BB_WORDS = [0, 1, BB_P - 1, (BB_P - 1) // 2, (BB_P + 1) // 2, 1 << 27, (1 << 27) - 1, (1 << 31) % BB_P, 0x7F7F7F7F % BB_P, 0x80808080 % BB_P]
WORDS = {GL: GL_WORDS, BB: BB_WORDS}
assert all(w < GL_P for w in GL_WORDS) and all(w < BB_P for w in BB_WORDS)

SHAPES = ("all_equal", "one_word", "alternating")
WORD0_ONLY = "word0_only"

# input: the canonical state to permute; (round, where): the place; shape; words: position -> the intended device word there;
# values: the same positions -> the true value (word / scale); exact: the device register must hold exactly that word
Target = namedtuple("Target", "field input round where shape words values exact")


def _target(field, r, where, shape, words, rng):
    m = model(field)
    state, values = [], {}
    for i in range(m.width):
        if i in words:
            values[i] = value_of_word(field, words[i], r, where)
            state.append(values[i])
        else:
            state.append(rng.randrange(m.p))
    exact = {i: m.unique_word(w) for i, w in words.items()}
    return Target(field, back_to_input(field, state, r, where), r, where, shape, dict(words), values, exact)


@functools.lru_cache(maxsize=None)
def targets(field):
    """every word of the field's set, at sbox_in and mds_in of every round, in the three shapes - all words equal; one word set
    (its position cycles with the round), the rest seeded random; two words of the set alternating - and in partial / internal
    rounds also as word 0 alone.  A fixed list."""
    m = model(field)
    words = WORDS[field]
    rng = random.Random(0x5EED0 + m.width)
    out = []
    for r in range(m.rounds):
        for where in (SBOX_IN, MDS_IN):
            for k, w in enumerate(words):
                w2 = words[(k + 1) % len(words)]
                out.append(_target(field, r, where, "all_equal", {i: w for i in range(m.width)}, rng))
                out.append(_target(field, r, where, "one_word", {(r + k) % m.width: w}, rng))
                out.append(_target(field, r, where, "alternating", {i: (w2 if i & 1 else w) for i in range(m.width)}, rng))
                if not m.is_full(r):
                    out.append(_target(field, r, where, WORD0_ONLY, {0: w}, rng))
    n_partial = sum(1 for r in range(m.rounds) if not m.is_full(r))
    assert len(out) == len(words) * 2 * (3 * m.rounds + n_partial), len(out)
    assert {(t.round, t.where) for t in out} == {(r, wh) for r in range(m.rounds) for wh in (SBOX_IN, MDS_IN)}
    return tuple(out)


def _zero_capacity_input(field, place, subset, words):
    """the input with a zero capacity (words 8..) whose s-box inputs at `subset` (8 positions) of round `place` (0, or 1 for
    Goldilocks: in front of the second non-linear layer) have the device words `words`; None if the 8 x 8 system is singular"""
    m = model(field)
    p = m.p
    want = [value_of_word(field, w, place, SBOX_IN) for w in words]
    if field == GL and place == 0:
        assert list(subset) == list(range(8))
        return [(v - m.rc[i]) % p for i, v in enumerate(want)] + [0] * 4
    if field == GL:
        # sbox_in(1) = M y + rc_1 with y = (x + rc_0)^7 and y_8..11 = rc_0[8..11]^7 known
        y_cap = [pow(m.rc[i], 7, p) for i in range(8, 12)]
        rhs = [(want[k] - m.rc[12 + q] - sum(m.m[q][8 + j] * y_cap[j] for j in range(4))) % p for k, q in enumerate(subset)]
        y = solve([[m.m[q][i] for i in range(8)] for q in subset], rhs, p)
        if y is None:
            return None
        return [(pow(v, m.inv7, p) - m.rc[i]) % p for i, v in enumerate(y)] + [0] * 4
    assert place == 0                                   # sbox_in(0) = M_E x + ext_0 with x_8..15 = 0
    rhs = [(want[k] - m.ext[q]) % p for k, q in enumerate(subset)]
    x = solve([[m.m_e[q][i] for i in range(8)] for q in subset], rhs, p)
    return None if x is None else x + [0] * 8


@functools.lru_cache(maxsize=None)
def zero_capacity_targets(field):
    """states whose capacity words are 0 on entry (what the hash kernels permute) with 8 chosen s-box inputs: Goldilocks at round 0
    (words 0..7) and in front of the second non-linear layer (8 of the 12 round-1 inputs, through the 8 x 8 system of the first
    MDS layer); BabyBear at 8 of the 16 round-0 inputs, through the initial M_E.  Per word of the set: that word eight times, and
    eight consecutive words of the set starting with it.  A singular subset is replaced by the next one, never dropped."""
    m = model(field)
    words = WORDS[field]
    placements = [(0, 0), (1, 0), (1, 4)] if field == GL else [(0, 0), (0, 8)]    # (round, first position of the subset)
    out = []
    for place, first in placements:
        for k, w in enumerate(words):
            for shape, ws in (("all_equal", [w] * 8), ("consecutive", [words[(k + j) % len(words)] for j in range(8)])):
                for shift in range(m.width):
                    subset = sorted((first + shift + j) % m.width for j in range(8)) if (place, field) != (0, GL) else list(range(8))
                    x = _zero_capacity_input(field, place, subset, ws)
                    if x is not None:
                        break
                assert x is not None, "no solvable 8-subset"
                wd = dict(zip(subset, ws))
                out.append(Target(field, x, place, SBOX_IN, "zero_capacity_" + shape, wd,
                                  {q: value_of_word(field, v, place, SBOX_IN) for q, v in wd.items()}, {q: m.unique_word(v) for q, v in wd.items()}))
    assert len(out) == len(placements) * len(words) * 2, len(out)
    assert all(all(x == 0 for x in t.input[8:]) for t in out)
    return tuple(out)


def all_inputs(field):
    """[count][width] canonical inputs of targets() followed by zero_capacity_targets(), as a list of lists"""
    return [list(t.input) for t in targets(field)] + [list(t.input) for t in zero_capacity_targets(field)]


# ------------------------------------------------------------------ Merkle trees of the oracle, level by level
def reference_layout(levels):
    """levels [0 .. root] -> the reference's `digests` vector for cap_height 0 (hash/merkle_tree.rs:200-217): node t of level k is
    the (t & 1) child of pair t >> 1, at 2 ((pair << (k + 1)) + 2^k - 1) + (t & 1)"""
    n = levels[0].shape[0]
    out = np.zeros((2 * (n - 1), levels[0].shape[1]), dtype=levels[0].dtype)
    for k, lv in enumerate(levels[:-1]):
        t = np.arange(lv.shape[0])
        out[2 * (((t >> 1) << (k + 1)) + (1 << k) - 1) + (t & 1)] = lv
    return out


def levels_of(mod, leaves):
    """[level 0 .. root] of the tree over `leaves` from the oracle module's hash_or_noop and two_to_one"""
    levels = [np.stack([mod.hash_or_noop(r) for r in leaves])]
    while levels[-1].shape[0] > 1:
        d = levels[-1]
        levels.append(np.stack([mod.two_to_one(d[2 * i], d[2 * i + 1]) for i in range(d.shape[0] // 2)]))
    return levels
