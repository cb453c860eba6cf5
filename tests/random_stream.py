"""The keyed element stream of csrc/random_stream.hpp restated in plain Python (integers and the struct module only): the ChaCha20
block function of RFC 8439 2.3, the element rule (byte quarter e & 3 of block e >> 2 as a little-endian 128-bit integer, mod p),
and the two streams the library draws from a seed - the salts of a zero-knowledge proof and a circuit's blinding values.  Nothing
here imports the package: the tests compare the library, the header's host build and its device build with this text."""
import struct

import numpy as np

GL_P = 0xFFFFFFFF00000001
BB_P = 2013265921
STREAM_SALTS, STREAM_BLINDING = 1, 2
SALT_SIZE = 4
MASK = 0xFFFFFFFF


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & MASK


def _quarter_round(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & MASK; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & MASK; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & MASK; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & MASK; s[b] = _rotl(s[b] ^ s[c], 7)


def block(seed, counter, nonce):
    """the 64 serialized bytes of the ChaCha20 block: key `seed` (32 bytes), block counter, three nonce WORDS"""
    seed = bytes(seed)
    assert len(seed) == 32 and len(nonce) == 3 and 0 <= counter <= MASK
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(struct.unpack("<8I", seed)) + [counter] + [int(x) & MASK for x in nonce]
    s = list(init)
    for _ in range(10):
        _quarter_round(s, 0, 4, 8, 12); _quarter_round(s, 1, 5, 9, 13); _quarter_round(s, 2, 6, 10, 14); _quarter_round(s, 3, 7, 11, 15)
        _quarter_round(s, 0, 5, 10, 15); _quarter_round(s, 1, 6, 11, 12); _quarter_round(s, 2, 7, 8, 13); _quarter_round(s, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & MASK for a, b in zip(s, init)])


def quarters(seed, counter, nonce):
    """the block's four 128-bit integers"""
    b = block(seed, counter, nonce)
    return [int.from_bytes(b[16 * i:16 * i + 16], "little") for i in range(4)]


def element(seed, nonce, e, p):
    assert 0 <= e >> 2 <= MASK
    return quarters(seed, e >> 2, nonce)[e & 3] % p


def blocks(seed, counters, nonce):
    """block() for an array of counters at once (numpy uint32 lanes; the same rounds): -> [len(counters)][64] bytes"""
    counters = np.asarray(counters, dtype=np.uint32)
    init = [np.full(counters.shape, v, dtype=np.uint32) for v in
            [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(struct.unpack("<8I", bytes(seed))) + [0] + [int(x) & MASK for x in nonce]]
    init[12] = counters.copy()
    s = [v.copy() for v in init]

    def rotl(x, n):
        return (x << np.uint32(n)) | (x >> np.uint32(32 - n))

    def qr(a, b, c, d):
        s[a] = s[a] + s[b]; s[d] = rotl(s[d] ^ s[a], 16)
        s[c] = s[c] + s[d]; s[b] = rotl(s[b] ^ s[c], 12)
        s[a] = s[a] + s[b]; s[d] = rotl(s[d] ^ s[a], 8)
        s[c] = s[c] + s[d]; s[b] = rotl(s[b] ^ s[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    words = np.stack([a + b for a, b in zip(s, init)], axis=-1).astype("<u4")
    return words.view(np.uint8).reshape(len(counters), 64)


def elements(seed, nonce, first, count, p):
    """elements first .. first + count - 1 as a numpy array of the field's word.  The blocks come from blocks() - block() on
    numpy lanes, compared with it by tests/test_random_stream_host.py; the reduction is Python's % on 128-bit integers"""
    dt = np.uint64 if p == GL_P else np.uint32
    if count == 0:
        return np.zeros(0, dtype=dt)
    b0, b1 = first >> 2, (first + count - 1) >> 2
    assert 0 <= b0 <= b1 <= MASK
    raw = blocks(seed, np.arange(b0, b1 + 1, dtype=np.uint64).astype(np.uint32), nonce).tobytes()
    skip = first - 4 * b0
    return np.array([int.from_bytes(raw[16 * i:16 * i + 16], "little") % p for i in range(skip, skip + count)], dtype=dt)


def salts(seed, F, n_lde):
    """[3][SALT_SIZE][n_lde]: salt element [s][j][t] = element t of the stream (seed, (STREAM_SALTS, s, j))"""
    return np.stack([np.stack([elements(seed, (STREAM_SALTS, s, j), 0, n_lde, F.P) for j in range(SALT_SIZE)]) for s in range(3)])


def blinding(seed, F, count):
    """the first `count` elements of the stream (seed, (STREAM_BLINDING, 0, 0)): blinding value i, in creation order of the targets"""
    return elements(seed, (STREAM_BLINDING, 0, 0), 0, count, F.P)


# ---- known answers: (seed, nonce words, counter, the block's bytes).  The first is RFC 8439 2.3.2; the other two were recorded
# with `openssl enc -chacha20 -K <seed> -iv <counter LE || nonce words LE>` over 64 zero bytes (OpenSSL 3.0.2).
KATS = [
    (bytes(range(32)), (0x09000000, 0x4a000000, 0), 1,
     "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e"),
    (bytes(range(32)), (0x01020304, 0x05060708, 0x090a0b0c), 0xFFFFFFFF,
     "79755b3d3f6a6a6f576d1731f9a30f05854de224f651f64e0b2e40f6ffe91410b1c704ffdedc743512ad8e70751819cd559772be7332e85a94d4a23acde2d77d"),
    (b"\xff" * 32, (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), 0xFFFFFFFF,
     "d72b21cfa4b6b0c41d61f62b8a11159c6a4f63bc56c2035796c7ad37811121bbec56d54a530f3a933dd28a50feb23bfaf64f405be985f3718bdf4683e96be749"),
]


def reduction_edges(p):
    """128-bit integers at the carry edges of the u128 -> field reductions"""
    e = [0, p - 1, p, p + 1, 2**64 - 1, 2**64, p * 2**64, p * 2**64 - 1, 2**96 - 1, 2**96, 2**128 - 1, (p - 1) * (2**64 + 1)]
    if p == BB_P:   # multiples of p around 2^31, 2^32, 2^62, 2^64 (and their neighbours)
        for bound in (2**31, 2**32, 2**62, 2**64, 2**96, 2**127):
            k = bound // p
            for m in (k * p, (k + 1) * p):
                e += [m - 1, m, m + 1]
    else:
        for k in (2**32 - 1, 2**32, 2**32 + 1, 2**63 // p + 1):
            e += [k * p - 1, k * p, k * p + 1]
        e += [2**64 + p - 1, 2**64 + p, (2**32 - 1) << 96, ((2**32 - 1) << 96) | (2**64 - 1), (2**32 - 1) << 64, 2**127]
    return [x for x in e if 0 <= x < 2**128]


def u128_words(x):
    return [(x >> (32 * i)) & MASK for i in range(4)]
