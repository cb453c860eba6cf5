"""The six permutation forms of the headers, each in a kernel of its own (tests/device/permutation_states.hip, built for gfx950 at
test time), on the states pulled back from chosen round words (tests/permutation_states.py), every output word against the oracle:
permute_mont_mfma_grouped with capacity_only false and true (words 8..11 compared), and both again with zero_capacity on the
zero-capacity states; poseidon_gl_coop::permute; poseidon2_bb::permute; permute_scaled + canonical_out; poseidon2_bb_coop::permute.
The product reaches the cooperative forms and the two flags only through the sponges of the tree kernels; here they meet full
states.  State counts 1, 63, 65 (a partial wave, a wave and one lane, the clamped lanes of the last block) and the full lists."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B

import permutation_states as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DTYPE = {PS.GL: np.uint64, PS.BB: np.uint32}
FORMS = {PS.GL: ("permute_mont_mfma_grouped", "permute_mont_mfma_grouped capacity_only", "poseidon_gl_coop::permute"),
         PS.BB: ("poseidon2_bb::permute", "permute_scaled + canonical_out", "poseidon2_bb_coop::permute")}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "needs hipcc"
    out = tmp_path_factory.mktemp("permutation_states") / "permutation_states"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_goldibear_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "device", "permutation_states.hip")], check=True, capture_output=True, text=True)
    return str(out)


_cache = {}


def states_and_oracle(field, zero_capacity):
    """([count][width] inputs, the oracle's outputs), computed once"""
    if (field, zero_capacity) not in _cache:
        ts = PS.zero_capacity_targets(field) if zero_capacity else PS.targets(field) + PS.zero_capacity_targets(field)
        st = np.array([t.input for t in ts], dtype=DTYPE[field])
        f = O.poseidon if field == PS.GL else B.poseidon2
        _cache[(field, zero_capacity)] = (st, np.stack([f(s) for s in st]))
    return _cache[(field, zero_capacity)]


def run(exe, tmp_path, field, st, zero_capacity):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([0 if field == PS.GL else 1, st.shape[0], int(zero_capacity)], dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(st).tobytes())
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.fromfile(dst, dtype=DTYPE[field]).reshape(3, st.shape[0], st.shape[1])


def compare(field, got, want):
    for k, form in enumerate(FORMS[field]):
        g, w = got[k], want
        if "capacity_only" in form:
            g, w = g[:, 8:], w[:, 8:]
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, "%s: %d of %d states differ, first %d" % (form, bad.size, g.shape[0], int(bad[0]))


@pytest.mark.parametrize("count", [1, 63, 65, None], ids=["1", "63", "65", "all"])
@pytest.mark.parametrize("field", [PS.GL, PS.BB])
def test_every_form_equals_the_oracle(exe, tmp_path, field, count):
    st, want = states_and_oracle(field, False)
    if count is not None:
        # from the end of the list: the zero-capacity states and the last rounds' targets
        st, want = st[-count:], want[-count:]
    compare(field, run(exe, tmp_path, field, st, False), want)


@pytest.mark.parametrize("count", [65, None], ids=["65", "all"])
def test_grouped_forms_with_the_zero_capacity_flag(exe, tmp_path, count):
    st, want = states_and_oracle(PS.GL, True)
    assert not st[:, 8:].any()
    if count is not None:
        st, want = st[:count], want[:count]
    compare(PS.GL, run(exe, tmp_path, PS.GL, st, True), want)
