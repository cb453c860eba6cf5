"""bench.py --dump-outputs: what the timed path computed, as float .npy files that hold every word exactly, within 64 MB; and the
plain / --full split of the line (the launch path with the GPU work stubbed out: GB_BENCH_STUB=1).  No GPU needed."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_words_survive_the_float_conversion():
    b = _bench()
    u8 = np.arange(256, dtype=np.uint8)
    f = b._exact_float(u8)
    assert f.dtype == np.float32 and (f.astype(np.uint8) == u8).all()
    u32 = np.array([0, 1, 2013265920, 0xFFFFFFFF], dtype=np.uint32)
    f = b._exact_float(u32)
    assert f.dtype == np.float64 and (f.astype(np.uint64) == u32).all()
    u64 = np.array([[0, 1], [0xFFFFFFFF00000000, 0xFFFFFFFF00000001 - 1]], dtype=np.uint64)
    f = b._exact_float(u64)
    assert f.dtype == np.float64 and f.shape == (2, 2, 2)
    back = (f[..., 0].astype(np.uint64) << np.uint64(32)) | f[..., 1].astype(np.uint64)
    assert (back == u64).all()
    assert (b._exact_float(u64.view(np.int64)) == f).all()


def test_proof_bytes_are_dumped_one_per_float(tmp_path):
    b = _bench()
    proof = bytes(range(256)) * 3 + b"\x07"
    arrays = b.proof_outputs([proof], 0, 1)
    assert list(arrays) == ["proof"]
    b.dump_outputs(str(tmp_path), arrays, 1)
    got = np.load(str(tmp_path / "proof.npy"))
    assert got.dtype == np.float32 and bytes(got.astype(np.uint8)) == proof
    assert sorted(b.proof_outputs([proof, proof], 1, 2)) == ["proof_rank1_lane0", "proof_rank1_lane1"]


class _FakeBatch:
    """the accessors of plonky2_goldibear_amd.PolynomialBatch that batch_outputs reads, at the commit workload's size"""
    degree_log, rate_bits, cap_height, num_polys = 20, 3, 4, 135

    class merkle_tree:
        cap = np.arange(16 * 4, dtype=np.uint64).reshape(16, 4)

    def polynomial(self, col):
        return np.arange(1 << self.degree_log, dtype=np.uint64) * np.uint64(col + 1)

    def get_lde_values(self, index, step):
        return np.full(self.num_polys, index * step, dtype=np.uint64)

    def _leaf(self, i):
        return np.full(self.num_polys, i, dtype=np.uint64), np.full((19, 4), i, dtype=np.uint64)


def test_commit_sample_is_fixed_and_within_the_limit():
    b = _bench()
    one, two = b.batch_outputs(_FakeBatch(), 0, 1), b.batch_outputs(_FakeBatch(), 0, 1)
    assert sorted(one) == ["cap", "coeffs_sample", "lde_rows_sample", "leaf_rows_sample", "merkle_paths_sample"]
    assert all((one[k] == two[k]).all() for k in one)     # the same sample every run
    assert all(a.dtype == np.float64 for a in one.values())
    assert sum(a.nbytes for a in one.values()) <= b.DUMP_LIMIT_BYTES


def test_dump_refuses_more_than_the_limit(tmp_path):
    b = _bench()
    big = {"x": np.zeros(b.DUMP_LIMIT_BYTES // 8 + 1, dtype=np.float64)}
    with pytest.raises(SystemExit):
        b.dump_outputs(str(tmp_path), big, 1)
    assert not os.listdir(str(tmp_path))


def test_plain_line_and_full_option():
    """the launch path accepts --full; --steps sets the number of timed steps and ms_per_step is one of them"""
    env = dict(os.environ, GB_BENCH_STUB="1", GB_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", *extra],
                           env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        j = json.loads(lines[0])
        assert j["steps"] == 4 and j["ms_per_step"] > 0
        for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert k in j
