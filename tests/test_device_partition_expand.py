"""k_expand_partition<F> (csrc/partition_expand.hpp: the gather-and-transpose behind gb_prove_partition) on the GPU, built for
gfx950 from the header alone (tests/device/partition_expand.hip) - its output equals the numpy gather exactly, for both fields, at
every combination of
  * degree_bits 2, 5, 6, 7, 10: the tile has 64 rows, so n = 4 and 32 are below one tile of rows (4 is the prover's smallest
    degree: one 16-byte store group of BabyBear rows), 64 is exactly one, 128 and 1024 are several workgroups;
  * num_wires 3, 32, 33, 135, 167: below, at and one past the 32 columns of a tile, and the stock configurations' widths;
  * the maps of tests/partition_cases.py: identity, one class, virtual representatives, the corners joined with unused virtual
    targets, a seeded random partition with classes of 1 to 5 cells;
  * values with 0, 1, p - 1 among them and, at every other target, the word the reference's field types hold in memory
    (GB_INPUT_P3_REPR: x + p where it fits in 64 bits, BabyBear's Montgomery word) - the kernel copies words as they are; that
    the host compaction canonicalises them is checked through the ABI in tests/test_gpu_prove_partition.py.
One process per (field, degree_bits): the five widths and five maps of it are a few milliseconds of GPU time each."""
import os
import subprocess

import numpy as np
import pytest

import partition_cases as PC
from oracle.fields import BB, GL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"goldilocks": (GL, 0), "babybear": (BB, 1)}
DEGREE_BITS = [2, 5, 6, 7, 10]
NUM_WIRES = [3, 32, 33, 135, 167]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("partition_expand") / "partition_expand"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "partition_expand.hip")], check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits", DEGREE_BITS)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_device_expansion_equals_the_numpy_gather(exe, tmp_path, field, degree_bits):
    F, tag = FIELDS[field]
    n = 1 << degree_bits
    cases, words = [], []
    for nw in NUM_WIRES:
        for name, m in PC.maps(n, nw).items():
            reps, slots, _ = PC.slot_map(m, n * nw)
            canon, in_memory = PC.field_values(F, len(m), 77 + nw, p3=True)
            values = np.where(np.arange(len(m)) % 2 == 0, canon, in_memory)
            cases.append((name, nw, PC.expand(m, values, n, nw)))
            words += [np.array([degree_bits, nw, len(reps)], dtype=np.uint64), slots.astype(np.uint64),
                      values[reps.astype(np.int64)].astype(np.uint64)]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([np.array([tag, len(cases)], dtype=np.uint64)] + words).tofile(src)
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout + out.stderr)
    got = np.fromfile(dst, dtype=F.dtype)
    assert got.size == sum(w.size for _, _, w in cases)
    at = 0
    for name, nw, want in cases:
        g = got[at:at + want.size].reshape(nw, n)
        at += want.size
        bad = np.argwhere(g != want)
        assert bad.size == 0, "%s, %d wires: first difference at (column, row) %r" % (name, nw, bad[0].tolist())
