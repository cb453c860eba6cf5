"""The word files that tests/host_shim/random_stream.cpp and tests/device/random_stream.hip read (tests/host_shim/
random_stream_case.hpp has the format), and what they must answer - from tests/random_stream.py and Python integers."""
import numpy as np

import random_stream as RS

FIELDS = {"goldilocks": (0, RS.GL_P), "babybear": (1, RS.BB_P)}
BLOCK, REDUCE, RANGE, ELEMENT = 1, 2, 3, 4
SEED = bytes((7 * i + 3) & 0xFF for i in range(32))
NONCE = (0x80000001, 0x00C0FFEE, 0xFFFFFFFE)   # every word non-zero
# (first, count): inside one block, across a block boundary, whole blocks, ragged at both ends over many blocks, the last blocks
RANGES = [(0, 1), (3, 2), (4, 4), (5, 1030), (2**34 - 6, 6)]
REFUSED = [(2**34 - 6, 7), (2**34, 1), (2**64 - 1, 2), (5, 2**64 - 3)]


def _key_words(seed, nonce):
    return [int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)] + [int(x) for x in nonce]


def block_records():
    """the three known-answer blocks -> (words, expected words)"""
    words, want = [], []
    for seed, nonce, counter, hexed in RS.KATS:
        words += [BLOCK] + _key_words(seed, nonce) + [counter]
        raw = bytes.fromhex(hexed)
        want += [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(8)]
    return words, want


def reduce_records(name):
    tag, p = FIELDS[name]
    words, want = [], []
    for x in RS.reduction_edges(p):
        words += [REDUCE, tag, x & (2**64 - 1), x >> 64]
        want.append(x % p)
    return words, want


def kat_element_records(name):
    """elements 4 c .. 4 c + 3 of the known-answer blocks: the block's quarters mod p"""
    tag, p = FIELDS[name]
    words, want = [], []
    for seed, nonce, counter, hexed in RS.KATS:
        raw = bytes.fromhex(hexed)
        for i in range(4):
            words += [ELEMENT, tag] + _key_words(seed, nonce) + [4 * counter + i]
            want.append(int.from_bytes(raw[16 * i:16 * i + 16], "little") % p)
    return words, want


def range_records(name, refused=True):
    tag, p = FIELDS[name]
    words, want = [], []
    for first, count in RANGES:
        words += [RANGE, tag] + _key_words(SEED, NONCE) + [first, count]
        want += [1] + [int(v) for v in RS.elements(SEED, NONCE, first, count, p)]
    for first, count in (REFUSED if refused else []):
        words += [RANGE, tag] + _key_words(SEED, NONCE) + [first, count]
        want += [0]
    return words, want


def all_records(name):
    words, want = [], []
    for w, x in (block_records(), reduce_records(name), kat_element_records(name), range_records(name)):
        words += w
        want += x
    return np.array(words, dtype=np.uint64), np.array(want, dtype=np.uint64)
