"""Circuits under zero-knowledge configs for tests/test_builder_blinding.py and tests/test_gpu_builder_zero_knowledge.py: the
factorial circuit of plonky2/examples/factorial.rs in either field, and the configs.

SMALL: num_query_rounds = 2 with arity 2 and a final polynomial of at most 4 coefficients, so that blind()'s rows are few: one
opening reveals 2 (1 + D (folding points + final coefficients)) values per FRI query set - at 2^8 Goldilocks rows 44 regular rows
and 46 pairs (136 rows), at 2^9 BabyBear rows 94 and 98 pairs (290 rows) - and the factorial circuit below lands on 2^8 rows
(Goldilocks) and 2^9 (BabyBear).  security_bits is lowered to what two query rounds give (2 * 3 + 16 bits); nothing else differs
from the stock configs."""
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import CircuitBuilder, CircuitConfig, PartialWitness

SMALL = dict(num_query_rounds=2, security_bits=20, arity_bits=1, final_poly_bits=2)


def config(field, zero_knowledge=True, **kw):
    make = CircuitConfig.standard_recursion_config_gl if field == N.GB_GOLDILOCKS else CircuitConfig.recursion_config_bb_narrow
    return make(**dict(kw, zero_knowledge=zero_knowledge))


def small_config(field, zero_knowledge=True):
    return config(field, zero_knowledge, **SMALL)


def factorial(cfg, start=1, count=20):
    """cur = initial * 2 * 3 * ...; public inputs (initial, result) -> (builder, partial witness)"""
    b = CircuitBuilder(cfg)
    initial = b.add_virtual_target()
    cur = initial
    for i in range(2, 2 + count):
        cur = b.mul(cur, b.constant(i))
    b.register_public_input(initial)
    b.register_public_input(cur)
    pw = PartialWitness()
    pw.set_target(initial, start)
    return b, pw
