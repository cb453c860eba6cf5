"""Zero-knowledge proofs whose salts come from a seed (GB_SALTS_FROM_SEED; include/goldibear_gpu.h: gb_prove_salted): the library
generates the salt columns on the device, and the proof bytes are those of the same call with the salt matrix the restatement
(tests/random_stream.py: salts) computes from the seed - and those of the oracle prover with that matrix.  The shapes of
tests/test_zero_knowledge.py: Goldilocks 2^5 and 2^10 rows, BabyBear 2^6 and 2^11; from a host witness, from a device witness,
from separately allocated columns, through prove_partition and prove_inputs_once; both verifiers; determinism; refusals.
-m gpu only."""
import ctypes as C

import numpy as np
import pytest

import partition_cases as PC
import random_stream as RS
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import CircuitData, GpuContext, ShapeError
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu

SEED = bytes((29 * i + 1) & 0xFF for i in range(32))
SHAPES = [(GL, 5), (GL, 10), (BB, 6), (BB, 11)]
IDS = ["gl5", "gl10", "bb6", "bb11"]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def _oracle_circuit(F, degree_bits, zero_knowledge=True):
    circ = D.DummyCircuit(degree_bits, F=F) if F is GL else D.DummyCircuit(degree_bits, D.CircuitConfig.babybear(6), F=BB)
    circ.zero_knowledge = zero_knowledge
    return circ


def _gpu_circuit(ctx, circ, zero_knowledge=True):
    cfg = circ.cfg
    gpu = CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                      num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants, num_challenges=cfg.num_challenges,
                      arity_bits=cfg.arity_bits, field=N.GB_GOLDILOCKS if circ.F is GL else N.GB_BABYBEAR, zero_knowledge=zero_knowledge)
    circ.set_cap(gpu.constants_sigmas_cap)
    return gpu


@pytest.fixture(scope="module")
def cases(ctx):
    """per shape, once: the circuit on both sides, a witness, the salts of SEED and the oracle prover's proof with them"""
    made = {}

    def get(F, degree_bits):
        key = (F.P, degree_bits)
        if key not in made:
            circ = _oracle_circuit(F, degree_bits)
            gpu = _gpu_circuit(ctx, circ)
            w = circ.witness(seed=9)
            salts = RS.salts(SEED, F, circ.n << circ.cfg.rate_bits)
            made[key] = (circ, gpu, w, salts, D.prove_cpu(circ, w, salts=salts)[0])
        return made[key]

    yield get
    for _, gpu, _, _, _ in made.values():
        gpu.free()


@pytest.mark.parametrize("F,degree_bits", SHAPES, ids=IDS)
def test_seeded_proof_bytes_equal_the_salted_proof_and_the_oracle(ctx, cases, F, degree_bits):
    import torch
    circ, gpu, w, salts, want = cases(F, degree_bits)
    assert salts.shape == (3, 4, circ.n << circ.cfg.rate_bits) and int(salts.max()) < F.P
    got = gpu.prove(w, seed=SEED)
    assert got == gpu.prove(w, salts=salts)
    assert got == want
    assert gpu.verify(got) and D.verify(circ, got)
    # a device witness: the seed stays a host pointer
    wd = torch.from_numpy(w.view(np.int64 if F is GL else np.int32)).to("cuda:0")
    assert gpu.prove(wd, seed=SEED) == want
    assert gpu.prove_once(wd, seed=SEED) == want
    # separately allocated columns (gb_prove_salted_cols)
    assert gpu.prove([np.array(c, copy=True) for c in w], seed=SEED) == want


@pytest.mark.parametrize("F,degree_bits", SHAPES, ids=IDS)
def test_determinism_and_other_seeds(ctx, cases, F, degree_bits):
    circ, gpu, w, salts, want = cases(F, degree_bits)
    assert gpu.prove(w, seed=SEED) == want and gpu.prove(w, seed=bytearray(SEED)) == want       # the same seed: the same bytes
    other = bytes([SEED[0] ^ 0x80]) + SEED[1:]
    again = gpu.prove(w, seed=other)
    assert again != want and len(again) == len(want)
    assert gpu.verify(again) and D.verify(circ, again)
    if degree_bits <= 6:   # (the oracle prover takes seconds at the larger shapes: its proof with SEED is the one shared above)
        assert again == D.prove_cpu(circ, w, salts=RS.salts(other, F, circ.n << circ.cfg.rate_bits))[0]
    from oracle import verifier as V
    assert V.read_proof_with_pis(again, circ.common_data(), F)[1] == V.read_proof_with_pis(want, circ.common_data(), F)[1]


@pytest.mark.parametrize("F,degree_bits", [(GL, 5), (BB, 6)], ids=["gl5", "bb6"])
def test_through_the_partition_and_the_inputs(ctx, cases, F, degree_bits):
    circ, _, w, salts, want = cases(F, degree_bits)
    gpu = _gpu_circuit(ctx, circ)
    m, values = PC.partition_of_witness(w, None, 4)
    gpu.set_partition(m)
    assert gpu.prove_partition(values, seed=SEED) == want
    assert gpu.prove_partition_once(values, seed=SEED) == gpu.prove_partition(values, salts=salts)
    reps = np.unique(m[:circ.n * circ.cfg.num_wires])
    gpu.set_generators([], reps, np.zeros((circ.cfg.num_constants, circ.n), dtype=np.uint64))
    assert gpu.prove_inputs_once(values[reps.astype(np.int64)], seed=SEED) == want
    with pytest.raises(ShapeError):
        gpu.prove_partition(values)          # without the flag nothing changes: a zero-knowledge circuit needs its salts
    with pytest.raises(ShapeError):
        gpu.prove_inputs_once(values[reps.astype(np.int64)])
    gpu.free()


@pytest.mark.parametrize("F,degree_bits", [(GL, 5), (BB, 6)], ids=["gl5", "bb6"])
def test_refusals(ctx, cases, F, degree_bits):
    circ, gpu, w, salts, want = cases(F, degree_bits)
    with pytest.raises(ShapeError, match="exclusive"):
        gpu.prove(w, seed=SEED, salts=salts)
    with pytest.raises(ShapeError, match="32 bytes"):
        gpu.prove(w, seed=SEED[:31])
    with pytest.raises(ShapeError):
        gpu.prove(w)                          # still refused without salts
    # the flag with a null seed, through the ABI - on the entry points that have a salts argument and on one that has none
    lib = N.load()
    buf = np.empty(1 << 20, dtype=np.uint8)
    n = C.c_size_t()
    flags = N.GB_INPUT_HOST | N.GB_SALTS_FROM_SEED
    assert lib.gb_prove_salted(gpu.handle, w.ctypes.data, flags, None, 0, None, buf.ctypes.data, buf.size, C.byref(n)) == N.GB_ERR_INVALID
    assert lib.gb_prove(gpu.handle, w.ctypes.data, flags, None, 0, buf.ctypes.data, buf.size, C.byref(n)) == N.GB_ERR_INVALID
    assert lib.gb_prove(gpu.handle, w.ctypes.data, 8, None, 0, buf.ctypes.data, buf.size, C.byref(n)) == N.GB_ERR_INVALID   # an unknown bit
    assert gpu.prove(w, seed=SEED) == want    # the circuit still proves
    # the flag on a circuit that is not zero-knowledge: the error salts on such a circuit get
    plain_circ = _oracle_circuit(F, degree_bits, zero_knowledge=False)
    plain = _gpu_circuit(ctx, plain_circ, zero_knowledge=False)
    with pytest.raises(ShapeError, match="without zero_knowledge") as with_salts:
        plain.prove(w, salts=salts)
    with pytest.raises(ShapeError, match="without zero_knowledge") as with_seed:
        plain.prove(w, seed=SEED)
    assert str(with_seed.value) == str(with_salts.value)
    unsalted = plain.prove(w)
    assert unsalted == D.prove_cpu(plain_circ, w)[0] and plain.verify(unsalted)
    plain.free()
