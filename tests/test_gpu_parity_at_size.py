"""Parity AT THE BASELINE SIZES, bit for bit, through the C ABI.  -m gpu only.

* prove(): GPU proof BYTES == the CPU oracle prover's at 2^14 ... 2^19 rows (an oracle run per case, on the box's host cores) and
  at 2^20 rows (configs[2] Goldilocks num_challenges 3; configs[3] BabyBear num_challenges 10) - the claim
  north_star makes ("bit-exact against the reference CPU prover's Proof bytes", plonk/prover.rs:228-447).  At 2^20 rows the
  oracle's proof is a committed golden vector (round 6: tests/golden/bench_proof_sha256.json, made by
  tests/golden/make_bench_proof_golden.py - the oracle prover on the same circuit and witness, in the build container): the
  two oracle runs of that size cost 2.3 of the GPU test step's 15 minutes, and tests/test_gpu_large_sizes.py now runs the oracle at
  2^21 rows.
* PolynomialBatch::from_values (fri/oracle.rs:68-123) at n = 2^20, N = 2^23: EVERY coefficient, EVERY leaf of every
  column, EVERY digest and the cap against the oracle's batch - this is the only size that runs the 2^20-row NTT kernels
  (k_lde_pa16x2<F>), so a sampled check is not enough there.
The oracle needs about a minute per 2^20-row proof on the GPU box's 16 host cores."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import oracle_bb as B
from oracle import plonk_dummy as D
from oracle.fields import BB, GL
from plonky2_goldibear_amd import GB_BABYBEAR, CircuitData, GpuContext, PolynomialBatch
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    O.use_host_cpu_share()
    c = GpuContext(0)
    yield c
    c.close()


def _gpu_circuit(ctx, circ, tag):
    cfg = circ.cfg
    return CircuitData(ctx, circ.degree_bits, circ.constants_sigmas, circ.k_is, num_wires=cfg.num_wires,
                       num_routed_wires=cfg.num_routed_wires, num_constants=cfg.num_constants,
                       num_challenges=cfg.num_challenges, max_quotient_degree_factor=cfg.max_quotient_degree_factor,
                       rate_bits=cfg.rate_bits, cap_height=cfg.cap_height, proof_of_work_bits=cfg.proof_of_work_bits,
                       num_query_rounds=cfg.num_query_rounds, arity_bits=cfg.arity_bits, final_poly_bits=cfg.final_poly_bits,
                       gate_constant=circ.GATE_CONSTANT, gate_pi=circ.GATE_PI, field=tag)


@pytest.mark.parametrize("field_name,degree_bits,num_challenges", [
    ("goldilocks", 14, 2), ("babybear", 15, 7),      # 2^14 / 2^15 rows: k_lde_pa_small<F, K>, the LDS radix-2 inverse transform
    ("goldilocks", 16, 3), ("babybear", 16, 7),
    ("goldilocks", 17, 3), ("babybear", 17, 8),      # 2^17 / 2^19 rows: the mixed radix-2/4/8 middle passes, k_lde_pa16xs<F, K>
    ("goldilocks", 18, 3), ("babybear", 19, 9),      # (2^18 BabyBear and 2^19 Goldilocks: the same kernels; from_values parity in test_gpu_parity.py)
])
def test_proof_bytes_match_oracle_at_size(ctx, field_name, degree_bits, num_challenges):
    if field_name == "goldilocks":
        F, tag, cfg = GL, N.GB_GOLDILOCKS, D.CircuitConfig(num_challenges=num_challenges)
    else:
        F, tag, cfg = BB, N.GB_BABYBEAR, D.CircuitConfig.babybear(num_challenges)
    circ = D.DummyCircuit(degree_bits, cfg, F=F)
    gpu = _gpu_circuit(ctx, circ, tag)
    # the oracle prover commits constants||sigmas itself (the build() share); the GPU's cap only spares the Python side a second
    # CPU commitment for the digest - prove_cpu() asserts that it IS the cap of the oracle's own commitment (cap and digest are
    # oracle-pinned, not GPU-vs-GPU), and the proof bytes depend on the oracle's commitment through the openings and the queries
    circ.set_cap(gpu.constants_sigmas_cap)
    assert (gpu.circuit_digest == circ.circuit_digest).all()
    w = circ.witness(seed=degree_bits)
    # a BabyBear witness meets a zero denominator now and then (InvZeroPermArg, prover.rs:512-514): the retry loop re-draws the random
    # wire IN PLACE (prover.rs:183-226), and the oracle then proves the witness the GPU's proof was made from
    got = gpu.prove(w, random_wire=(cfg.num_wires - 1, circ.pi_row), rng=np.random.default_rng(degree_bits))
    want, _ = D.prove_cpu(circ, w)
    assert len(got) == len(want)
    assert got == want, "first differing byte at %d" % next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
    assert (gpu.constants_sigmas_cap == D.prove_cpu.last_cs_cap).all()    # (what prove_cpu asserted, spelled out)
    assert gpu.verify(got)
    if degree_bits == 16:
        # the same proof through the column-pointer ABI: MatrixWitness.wire_values as the reference holds it (iop/witness.rs:277-279),
        # num_wires separately allocated pageable columns -> gb_prove_cols, staged by the library's page-locked ring
        cols = [np.array(c, copy=True) for c in w]
        assert gpu.prove(cols) == want
    gpu.free()
    ctx.trim()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_full_batch_2pow20_every_leaf_and_digest(ctx, field_name):
    """n = 2^20, rate 3, cap 4, 9 columns (two sponge absorptions per leaf for Goldilocks, a ragged second one for both):
    the whole batch against the oracle."""
    log_n, ncols = 20, 9
    seed = 0xC0FFEE ^ (ncols << 32) ^ log_n
    if field_name == "goldilocks":
        vals = O.splitmix64_fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        cpu = O.PolynomialBatch.from_values(vals, 3, 4)
        gpu = PolynomialBatch.from_values(ctx, vals, 3, 4)
    else:
        vals = B.fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        cpu = B.PolynomialBatch.from_values(vals, 3, 4)
        gpu = PolynomialBatch.from_values(ctx, vals, 3, 4, field=GB_BABYBEAR)
    assert (gpu.merkle_tree.cap == cpu.cap).all()
    assert (gpu.polynomials == cpu.polynomials).all()
    leaves = gpu.merkle_tree.leaves
    assert leaves.shape == cpu.leaves.shape == (1 << 23, ncols)
    bad = np.flatnonzero((leaves != cpu.leaves).any(axis=1))
    assert bad.size == 0, "%d leaves differ, first %d" % (bad.size, bad[0])
    del leaves
    dig = gpu.merkle_tree.digests
    assert dig.shape == cpu.digests.shape
    assert (dig == cpu.digests).all()
    # the prover's view of the same data (plonk/prover.rs:822-831)
    for i in (0, 1, (1 << 20) - 1, 777777):
        assert (gpu.get_lde_values(i, 8) == cpu.get_lde_values(i, 8)).all()
    gpu.free()
    # the same batch from a device-resident matrix (one launch per pass over all columns instead of upload chunks): identical
    # coefficients and tree
    import torch
    dev = torch.from_numpy(vals.view(np.int64 if vals.dtype == np.uint64 else np.int32)).cuda()
    g2 = PolynomialBatch.from_values(ctx, dev, 3, 4, field=N.GB_GOLDILOCKS if field_name == "goldilocks" else GB_BABYBEAR)
    assert (g2.merkle_tree.cap == cpu.cap).all()
    assert (g2.polynomial(ncols - 1) == cpu.polynomials[ncols - 1]).all() and (g2.polynomial(0) == cpu.polynomials[0]).all()
    g2.free()
    ctx.trim()


@pytest.mark.parametrize("field_name,rate_bits", [("goldilocks", 1), ("goldilocks", 2), ("babybear", 1), ("babybear", 2)])
def test_2pow20_rows_at_other_rates(ctx, field_name, rate_bits):
    """The 2^20-row passes (k_lde_pa16x2<F>'s coset loop, pb16, the 16-column inverse-transform groups) at rate_bits 1 and 2 - every
    stock configuration uses 3, so nothing else runs them with fewer cosets: 3 columns, the whole batch against the
    oracle.  Also the place where a non-canonical word stored by the twiddle chains (mul_mont on a lazy operand) would show."""
    log_n, ncols = 20, 3
    seed = 0xFACE ^ (rate_bits << 40)
    if field_name == "goldilocks":
        vals = O.splitmix64_fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        cpu = O.PolynomialBatch.from_values(vals, rate_bits, 4)
        gpu = PolynomialBatch.from_values(ctx, vals, rate_bits, 4)
    else:
        vals = B.fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        cpu = B.PolynomialBatch.from_values(vals, rate_bits, 4)
        gpu = PolynomialBatch.from_values(ctx, vals, rate_bits, 4, field=GB_BABYBEAR)
    assert (gpu.merkle_tree.cap == cpu.cap).all()
    assert (gpu.polynomials == cpu.polynomials).all()
    assert (gpu.merkle_tree.leaves == cpu.leaves).all()
    assert (gpu.merkle_tree.digests == cpu.digests).all()
    gpu.free()
    ctx.trim()


@pytest.mark.parametrize("field_name", ["goldilocks", "babybear"])
def test_proof_bytes_match_golden_at_2pow20(ctx, field_name):
    """BASELINE configs[2] / configs[3] themselves: prove() of the 2^20-row dummy circuit, proof bytes == the CPU oracle prover's -
    through the golden SHA-256 of the oracle's proof for the same circuit and witness (tests/golden/bench_proof_sha256.json; the
    generating script also checks the product-side and oracle-side generators element for element), the constants/sigmas cap and the
    circuit digest likewise; from one page-locked block and from separately allocated pageable columns (gb_prove_cols)."""
    import hashlib
    import json
    import os
    from plonky2_goldibear_amd import dummy_circuit as DC
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bench_proof_sha256.json")))["%s_2p20" % field_name]
    lg, ch = g["log_n"], g["num_challenges"]
    if field_name == "goldilocks":
        cs, k_is, pi_row, _ = DC.build_dummy_circuit(lg)
        gpu = CircuitData(ctx, lg, cs, k_is, num_challenges=ch)
        w = DC.dummy_witness(lg, pi_row, seed=g["witness_seed"])
    else:
        cs, k_is, pi_row, _ = DC.build_dummy_circuit_bb(lg)
        gpu = CircuitData(ctx, lg, cs, k_is, num_wires=167, num_routed_wires=41, num_challenges=ch, arity_bits=3, field=GB_BABYBEAR)
        w = DC.dummy_witness_bb(lg, pi_row, seed=g["witness_seed"])
    del cs
    assert [int(x) for x in gpu.circuit_digest] == g["circuit_digest"]
    assert hashlib.sha256(np.ascontiguousarray(gpu.constants_sigmas_cap).tobytes()).hexdigest() == g["constants_sigmas_cap_sha256"]
    proof = gpu.prove_once(w)            # (the golden seed is one that meets no zero denominator)
    assert len(proof) == g["proof_len"] and hashlib.sha256(proof).hexdigest() == g["sha256"]
    assert gpu.verify(proof)
    assert gpu.prove_once([np.array(c, copy=True) for c in w]) == proof
    gpu.free()
    ctx.trim()


@pytest.mark.parametrize("field_name,ncols,salted", [
    ("goldilocks", 33, False), ("goldilocks", 40, False), ("goldilocks", 64, False), ("goldilocks", 70, False),
    ("goldilocks", 97, True), ("goldilocks", 135, False), ("babybear", 33, False), ("babybear", 44, True),
    ("babybear", 71, False), ("babybear", 96, False), ("babybear", 167, False),
])
def test_host_input_leaf_sponge_in_segments(ctx, field_name, ncols, salted):
    """Host input with more than 32 columns and >= 2^19 leaves: commit() hashes the leaves in 32-column segments while later
    columns are still crossing PCIe (sponge state parked between segments, ragged last absorptions of every residue, salt
    columns in the last segment).  Cap, sampled leaves / paths and every digest equal the oracle's."""
    log_n = 16
    seed = 0xABCD ^ (ncols << 8)
    if field_name == "goldilocks":
        vals = O.splitmix64_fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        salts = O.splitmix64_fill(seed + 1, 4 << (log_n + 3)).reshape(4, -1) if salted else None
        cpu = O.PolynomialBatch.from_values(vals, 3, 4, salts=salts)
        gpu = PolynomialBatch.from_values(ctx, vals, 3, 4, salts=salts)
        dev_tensor = lambda a: __import__("torch").from_numpy(a.view(np.int64)).to("cuda:0")
    else:
        vals = B.fill(seed, ncols << log_n).reshape(ncols, 1 << log_n)
        salts = B.fill(seed + 1, 4 << (log_n + 3)).reshape(4, -1) if salted else None
        cpu = B.PolynomialBatch.from_values(vals, 3, 4, salts=salts)
        gpu = PolynomialBatch.from_values(ctx, vals, 3, 4, salts=salts, field=GB_BABYBEAR)
        dev_tensor = lambda a: __import__("torch").from_numpy(a.view(np.int32)).to("cuda:0")
    assert (gpu.merkle_tree.cap == cpu.cap).all()
    assert (gpu.merkle_tree.digests == cpu.digests).all()
    for i in (0, 1, 77777, (1 << 19) - 1):
        row, sib = gpu._leaf(i)
        assert (row == cpu.leaves[i]).all() and (sib == cpu.prove(i)).all()
    # the same batch from device-resident input takes the unsegmented kernel: identical tree
    dev = PolynomialBatch.from_values(ctx, dev_tensor(vals), 3, 4, salts=None if salts is None else dev_tensor(salts),
                                      field=gpu.field)
    assert (dev.merkle_tree.cap == cpu.cap).all()
    gpu.free()
    dev.free()
    ctx.trim()
