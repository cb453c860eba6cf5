"""GPU prove() of circuits whose gates are constraint programs (GB_GATE_PROGRAM: csrc/kernels_gates.hip k_gate_programs, the
interpreter of csrc/gates.hpp run_program with its registers in LDS).

A built-in gate rewritten as a program (tests/gate_programs.py) keeps its id, so the sorted gate set, the selectors and the
circuit digest stay what they were; field sums are exact, so the proof bytes must be IDENTICAL to the built-in evaluator's - which
tests/test_gpu_recursion_gates.py pins against the oracle prover.  A gate with no built-in counterpart (u32 multiply-add with
two-bit limbs) is proved, verified and tampered with; two different assemblies of it give the same bytes.  -m gpu only."""
import numpy as np
import pytest

from oracle.fields import BB, GL
from plonky2_goldibear_amd import GpuContext, PolynomialBatch, VerifyError
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness, wire
from plonky2_goldibear_amd.gate_program import GATE_PROGRAM, GateProgram, ProgramGate

import gate_programs as GP
from circuits import factorial_circuit, poly_chain_circuit, recursion_gates_circuit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def both_forms(ctx, make):
    """make() -> (builder, partial witness): the circuit as it is and with its covered gates as programs, and one witness"""
    b0, pw = make()
    b1, _ = make()
    GP.with_program_gates(b1)
    c0, c1 = b0.build(ctx), b1.build(ctx)
    assert any(g[0] == GATE_PROGRAM for g in c1.gate_table) and not any(g[0] == GATE_PROGRAM for g in c0.gate_table)
    assert [g[2:5] for g in c0.gate_table] == [g[2:5] for g in c1.gate_table] and c0.gate_ids == c1.gate_ids
    w, pis = c0.generate_witness(pw)
    return c0, c1, w, pis


def assert_same_bytes(ctx, make):
    c0, c1, w, pis = both_forms(ctx, make)
    assert (c0.constants_sigmas == c1.constants_sigmas).all()
    assert (c0.data.circuit_digest == c1.data.circuit_digest).all() and (c0.data.constants_sigmas_cap == c1.data.constants_sigmas_cap).all()
    rw = (c0.random_wire[1], c0.random_wire[0])
    want = c0.data.prove(w.copy(), pis, random_wire=rw)
    got = c1.data.prove(w.copy(), pis, random_wire=rw)
    assert got == want
    assert c1.data.verify(got) and c0.data.verify(got)
    c0.data.free()
    c1.data.free()


GL_T, BB_T = N.GB_GOLDILOCKS, N.GB_BABYBEAR


@pytest.mark.parametrize("field,num_challenges", [(GL_T, 2), (GL_T, 5), (BB_T, 6), (BB_T, 11)])
def test_recursion_gate_set_as_programs_gives_the_same_bytes(ctx, field, num_challenges):
    assert_same_bytes(ctx, lambda: recursion_gates_circuit(field, seed=5, num_challenges=num_challenges)[:2])


@pytest.mark.parametrize("num_challenges", [2, 5])
def test_factorial_as_programs_gives_the_same_bytes(ctx, num_challenges):
    assert_same_bytes(ctx, lambda: factorial_circuit(count=60, num_challenges=num_challenges))


def test_quotient_domain_a_strict_prefix_of_the_lde(ctx):
    """rate_bits 4 at quotient degree factor 8: the quotient is computed on every second LDE point (stride_bits != log_n + 3)"""
    assert_same_bytes(ctx, lambda: recursion_gates_circuit(GL_T, seed=6, rate_bits=4, num_query_rounds=21)[:2])


def test_four_rows_less_than_one_wave(ctx):
    def make():
        b, pw = poly_chain_circuit(CircuitConfig.standard_recursion_config_gl(), 1)
        return b, pw
    c0, c1, w, pis = both_forms(ctx, make)
    assert c0.degree_bits == 2
    assert c1.data.prove(w.copy(), pis) == c0.data.prove(w.copy(), pis)
    c0.data.free()
    c1.data.free()


def make_512():
    return factorial_circuit(count=900)


def test_512_rows_several_workgroups(ctx):
    c0, c1, w, pis = both_forms(ctx, make_512)
    assert c0.degree_bits == 9
    proof = c1.data.prove(w.copy(), pis)
    assert proof == c0.data.prove(w.copy(), pis) and c1.data.verify(proof)
    c0.data.free()
    c1.data.free()


def test_quotient_polys_stage_gives_the_same_chunks(ctx):
    """gb_quotient_polys (the stage ABI) on the 2^9-row circuit: program form and built-in form, same challenges"""
    c0, c1, w, pis = both_forms(ctx, make_512)
    cfg = c0.config
    pi_hash = GL.hash_no_pad(np.asarray(pis, dtype=np.uint64))
    betas, gammas, alphas = [3, 2**40 + 7], [11, GL.P - 5], [2**33 + 1, 12345678901234567]
    chunks = []
    for c in (c0, c1):
        wires = PolynomialBatch.from_values(ctx, w, cfg.rate_bits, cfg.cap_height, field=GL_T)
        zv = c.data.zs_partial_products(w, betas, gammas)
        zs = PolynomialBatch.from_values(ctx, zv, cfg.rate_bits, cfg.cap_height, field=GL_T)
        chunks.append(np.array(c.data.quotient_polys(wires, zs, pi_hash, betas, gammas, alphas)))
        wires.free()
        zs.free()
        c.data.free()
    assert chunks[0].shape == (2 * cfg.max_quotient_degree_factor, 512) and (chunks[0] == chunks[1]).all()


# ---------------------------------------------------------------------------------------------- a gate with no built-in counterpart
class U32MulAdd:
    """num_ops x (m0 * m1 + addend = lo + 2^h hi) with lo and hi in L two-bit limbs each.  Per operation the wires m0, m1, addend,
    lo, hi, then the 2 L limbs (lo's first, little-endian).  Constraints: for every operation the product check and the two
    recombinations; then for every operation its 2 L limb range checks prod_{k<4} (limb - k), degree 4."""

    def __init__(self, field, num_ops=3):
        self.field, self.num_ops = field, num_ops
        self.h, self.L = (32, 16) if field == GL_T else (12, 6)
        self.per_op = 5 + 2 * self.L
        self.num_wires = self.per_op * num_ops

    def limb(self, op, j):
        return self.per_op * op + 5 + j

    def plain(self, w, c):
        L, out = self.L, []
        for op in range(self.num_ops):
            m0, m1, addend, lo, hi = (w[self.per_op * op + k] for k in range(5))
            out.append(m0 * m1 + addend - (lo + 2**self.h * hi))
            out.append(sum(4**j * w[self.limb(op, j)] for j in range(L)) - lo)
            out.append(sum(4**j * w[self.limb(op, L + j)] for j in range(L)) - hi)
        for op in range(self.num_ops):
            for j in range(2 * L):
                x = w[self.limb(op, j)]
                out.append(x * (x - 1) * (x - 2) * (x - 3))
        return out

    def other_form(self, w, c):
        """the same constraints in the same order, written differently: Horner recombination over s = limb - 1, which the range
        checks of up to seven limbs per operation share - those values stay live from the recombinations to the range checks"""
        L, out, s = self.L, [], {}
        shared = min(7, L)   # per operation: 21 (Goldilocks) / 18 (BabyBear) values next to the sums in flight
        for op in range(self.num_ops):
            m0, m1, addend, lo, hi = (w[self.per_op * op + k] for k in range(5))
            out.append((addend - lo) + (m1 * m0 - hi * 2**self.h))
            for half, target in ((0, lo), (1, hi)):
                acc = 0
                for j in reversed(range(L)):
                    x = w[self.limb(op, half * L + j)]
                    if half == 0 and j < shared:
                        s[op, j] = x - 1
                        x = s[op, j] + 1
                    acc = acc * 4 + x
                out.append(acc - target)
        for op in range(self.num_ops):
            for j in range(2 * L):
                x = w[self.limb(op, j)]
                if (op, j) in s:
                    out.append((x * s[op, j]) * ((s[op, j] - 1) * (s[op, j] - 2)))
                else:
                    out.append((x * (x - 3)) * ((x - 2) * (x - 1)))
        return out

    def program(self, form="plain"):
        return GateProgram.from_constraints(getattr(self, form), self.num_wires, 0, self.field)

    def row(self, rng):
        """an integer witness of one row"""
        vals = []
        bits = 32 if self.field == GL_T else 11
        for _ in range(self.num_ops):
            m0, m1, addend = (int(rng.integers(0, 1 << bits)) for _ in range(3))
            v = m0 * m1 + addend
            lo, hi = v & ((1 << self.h) - 1), v >> self.h
            assert hi < 1 << self.h
            vals += [m0, m1, addend, lo, hi] + [(lo >> 2 * j) & 3 for j in range(self.L)] + [(hi >> 2 * j) & 3 for j in range(self.L)]
        return vals


def u32_circuit(ctx, field, form="plain", rows=25):
    G = U32MulAdd(field)
    cfg = CircuitConfig.standard_recursion_config_gl() if field == GL_T else CircuitConfig.recursion_config_bb_narrow()
    prog = G.program(form)
    assert prog.degree == 4 and prog.num_constraints == G.num_ops * (3 + 2 * G.L)
    gate = ProgramGate("U32MulAddGate { num_ops: %d, limb_bits: 2 }" % G.num_ops, prog)
    b = CircuitBuilder(cfg)
    rng = np.random.default_rng(17)
    pw, values = PartialWitness(), []
    for _ in range(rows):
        r = b.add_gate(gate)
        vals = G.row(rng)
        values.append((r, vals))
        for col, v in enumerate(vals):
            pw.set_target(wire(r, col), v)
    c = b.build(ctx)
    assert c.degree_bits == 5
    w, pis = c.generate_witness(pw)
    return G, prog, c, w, pis, values


@pytest.mark.parametrize("field", [GL_T, BB_T])
def test_u32_multiply_add_gate(ctx, field):
    G, prog, c, w, pis, values = u32_circuit(ctx, field)
    p = GP.P[field]
    for r, vals in values:
        assert [int(x) for x in w[:G.num_wires, r]] == vals
        assert not any(prog.evaluate(vals))
    proof = c.data.prove(w.copy(), pis)
    assert c.data.verify(proof)
    assert c.data.verify_compressed(c.data.compress(proof))
    assert c.data.prove(w.copy(), pis) == proof
    r, vals = values[7]
    col = G.limb(1, 3)
    for new in ((vals[col] + 1) % 4, 5):   # still a two-bit limb: only the recombination breaks; 5: the range check breaks
        bad = w.copy()
        bad[col, r] = new
        assert any(prog.evaluate([int(x) for x in bad[:G.num_wires, r]])) and new % p != vals[col]
        with pytest.raises(VerifyError, match="vanishing"):
            c.data.verify(c.data.prove(bad, pis))
    c.data.free()


@pytest.mark.parametrize("field", [GL_T, BB_T])
def test_equivalent_programs_give_equal_bytes(ctx, field):
    G, prog, c, w, pis, values = u32_circuit(ctx, field)
    G2, prog2, c2, w2, pis2, _ = u32_circuit(ctx, field, "other_form")
    assert prog2.num_regs >= 24 and prog2.words != prog.words
    assert (w == w2).all() and (c.constants_sigmas == c2.constants_sigmas).all()
    r, vals = values[3]
    assert prog2.evaluate(vals) == prog.evaluate(vals)
    bad = list(vals)
    bad[G.limb(0, 2)] = 7
    assert prog2.evaluate(bad) == prog.evaluate(bad) and any(prog.evaluate(bad))
    proof = c.data.prove(w.copy(), pis)
    assert c2.data.prove(w2.copy(), pis2) == proof and c2.data.verify(proof)
    c.data.free()
    c2.data.free()
