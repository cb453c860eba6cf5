"""csrc/verify_compressed.hpp - how the query rounds of a compressed proof share Merkle nodes: the count the host stage of
gb_verify_compressed_batch classifies a proof by (sibling_counts), the rule its kernel climbs a tree by (sibling_source) and the climb
itself (climb_level, the sequential form of the kernel's level loop) - compiled for the CPU (tests/host_shim/verify_compressed.cpp)
and run over random index sets: tree heights 0..8, cap heights 0..4, 1..70 query rounds, duplicates included.  The answers are
oracle/compression.py's: how many siblings compress_merkle_proofs leaves every query, which sibling decompress_merkle_proofs hands it
at every level, and the tree's own cap.  The program is built twice: plain, and as a stand-alone executable under AddressSanitizer +
UndefinedBehaviorSanitizer, which runs the same file.  CPU only; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from oracle import compression as Z
from oracle import oracle as O
from oracle.fields import GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"   # gl_field.hpp's limb code uses clang's __builtin_addc
NONE = 2 ** 64 - 1
WIDTH = 7   # a leaf that is hashed (more than four words)


def _build(out, extra):
    assert os.path.exists(CLANG), "needs the ROCm clang++ as the host compiler"
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run([CLANG, "-std=c++17", "-include", os.path.join(shim, "shim.h"), "-I", shim, "-I",
                    os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"), os.path.join(shim, "verify_compressed.cpp"), "-o", str(out)] + extra,
                   check=True, capture_output=True, text=True)
    return str(out)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("verify_compressed")
    return (_build(d / "verify_compressed", ["-O2"]),
            _build(d / "verify_compressed_san", ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                 "-fno-omit-frame-pointer"]))


def _cases():
    """(height, cap_height, indices, tree, full proofs, compressed proofs)"""
    rng = np.random.default_rng(2024)
    trees = {}
    out = []
    for height in range(9):
        for cap_height in range(min(height, 4) + 1):
            key = (height, cap_height)
            leaves = O.splitmix64_fill(100 * height + cap_height, WIDTH << height).reshape(1 << height, WIDTH) % np.uint64(GL.P)
            trees[key] = tree = O.MerkleTree(leaves, cap_height)
            for n in (1, 2, 3, 28, 64, 65, 70):
                span = 1 << height if n % 2 else max(1, (1 << height) // 3)   # a narrow range: more duplicates and neighbours
                idx = [int(x) for x in rng.integers(0, span, n)]
                proofs = [[[int(x) for x in s] for s in tree.prove(i)][:height - cap_height] for i in idx]
                comp = Z.compress_merkle_proofs(cap_height, idx, proofs)
                out.append((height, cap_height, idx, tree, proofs, comp))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _words(cases):
    w = [len(cases)]
    for height, cap_height, idx, tree, proofs, comp in cases:
        w += [height, cap_height, len(idx), WIDTH] + idx
        for i in idx:
            w += [int(x) for x in tree.leaves[i]]
        for p in comp:
            w.append(len(p))
            for h in p:
                w += [int(x) for x in h]
    return np.array(w, dtype=np.uint64)


def _run(exe, tmp_path, words):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    words.tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(dst, dtype=np.uint64)


def test_the_cases_cover_duplicates_siblings_and_merges(cases):
    dup = sib = merged = 0
    for height, cap_height, idx, tree, proofs, comp in cases:
        dup += len(set(idx)) < len(idx)
        for level in range(height - cap_height):
            nodes = [i >> level for i in idx]
            sib += any(n ^ 1 in nodes for n in nodes)
            merged += any(nodes.count(n) > 1 and n ^ 1 not in nodes for n in set(nodes))
    assert dup > 20 and sib > 100 and merged > 100


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_counts_sources_and_nodes_are_the_oracle_s(exes, cases, tmp_path, which):
    got = _run(exes[which], tmp_path, _words(cases))
    at = 0
    for height, cap_height, idx, tree, proofs, comp in cases:
        n, levels = len(idx), height - cap_height
        tag = (height, cap_height, idx)
        # how many siblings each query's own path holds
        assert [int(x) for x in got[at:at + n]] == [len(p) for p in comp], tag
        at += n
        # what the oracle re-inflates is what the proofs were
        assert Z.decompress_merkle_proofs(GL, [tree.leaves[i] for i in idx], idx, comp, height, cap_height) == proofs
        took = [0] * n
        for level in range(levels):
            nodes = [i >> level for i in idx]
            step = [0] * n
            for k in range(n):
                sibling, first = int(got[at]), int(got[at + 1])
                used = [int(x) for x in got[at + 2:at + 6]]
                at += 6
                holders = [j for j, x in enumerate(nodes) if x == nodes[k] ^ 1]
                assert sibling == (holders[0] if holders else NONE), tag
                assert first == nodes.index(nodes[k]), tag
                if not holders:   # the next stored sibling of the first query with this node
                    assert used == comp[first][took[first]], tag
                    step[k] = first == k
                assert used == proofs[k][level], (tag, level, k)   # the sibling of the full path, wherever it came from
            took = [a + b for a, b in zip(took, step)]
        assert took == [len(p) for p in comp], tag
        for k in range(n):   # the nodes that result: the tree's cap entries
            assert [int(x) for x in got[at:at + 4]] == [int(x) for x in tree.cap[idx[k] >> levels]], (tag, k)
            at += 4
    assert at == len(got)


def test_a_path_that_holds_too_little_is_refused_not_read_past(exes, cases, tmp_path):
    """(the host stage never sends such a proof to the device; the shim says so instead of reading behind the path)"""
    height, cap_height, idx, tree, proofs, comp = next(c for c in cases if any(len(p) > 0 for p in c[5]))
    k = next(i for i, p in enumerate(comp) if p)
    short = [p[:-1] if i == k else p for i, p in enumerate(comp)]
    words = _words([(height, cap_height, idx, tree, proofs, short)])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    words.tofile(src)
    for exe in exes:
        assert subprocess.run([exe, str(src), str(dst)], capture_output=True).returncode == 4
