"""Zero-knowledge circuits from the builder mirror on the GPU: the factorial circuit under the small zero-knowledge config of
tests/zk_circuits.py (2^8 Goldilocks rows, 2^9 BabyBear rows) with seed=, and one stock-config Goldilocks circuit (2^14 rows,
596 570 blinding values).
  * prove_inputs(pw, seed=s) == prove(pw, seed=s), accepted by verify; a build with wiring="device" gives the same bytes;
  * check_inputs(pw, seed=s): no violations, the copy constraints checked through the partition (copies_checked = 1);
  * the generated partition: every blinding cell holds the value of the seed's stream (tests/random_stream.py: blinding) for its
    ordinal, and the second row of every Z pair equals the first;
  * the same seed gives the same bytes, another seed other bytes; a zero-knowledge circuit without a seed is refused.
-m gpu only."""
import numpy as np
import pytest

import random_stream as RS
import zk_circuits as Z
from plonky2_goldibear_amd import GpuContext, ShapeError
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": (N.GB_GOLDILOCKS, RS.GL_P), "babybear": (N.GB_BABYBEAR, RS.BB_P)}
SEED = bytes((17 * i + 9) & 0xFF for i in range(32))
RNG = 77


class _P:
    def __init__(self, p):
        self.P = p


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(ctx):
    made = {}

    def get(field, wiring="host"):
        if (field, wiring) not in made:
            b, pw = Z.factorial(Z.small_config(FIELDS[field][0]))
            made[field, wiring] = (b.build(ctx, wiring=wiring), pw)
        return made[field, wiring]

    yield get
    for c, _ in made.values():
        c.data.free()


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_prove_inputs_equals_prove_and_verifies(ctx, built, field):
    c, pw = built(field)
    assert c.degree_bits <= 10 and c.config.zero_knowledge and len(c.blinding_targets) > 0
    by_host = c.prove(pw, rng=np.random.default_rng(RNG), seed=SEED)
    by_device = c.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED)
    assert by_device == by_host
    assert c.verify(by_device)
    assert c.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED) == by_device          # the same seed: the same bytes
    other = c.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=bytes(32))
    assert other != by_device and len(other) == len(by_device) and c.verify(other)
    pi_bytes = 2 * (8 if FIELDS[field][0] == N.GB_GOLDILOCKS else 4)
    assert other[-pi_bytes:] == by_device[-pi_bytes:]                                          # the same public inputs
    # wiring="device": the same sigma columns, the same bytes
    d, _ = built(field, "device")
    assert d.constants_sigmas.tobytes() == c.constants_sigmas.tobytes()
    assert d.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED) == by_device
    assert d.prove(pw, rng=np.random.default_rng(RNG), seed=SEED) == by_device
    with pytest.raises(ShapeError):
        c.prove_inputs(pw, rng=np.random.default_rng(RNG))                                     # zero-knowledge needs its seed
    assert c.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED) == by_device          # and still proves


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_check_inputs_and_the_generated_partition(ctx, built, field):
    c, pw = built(field)
    tag, p = FIELDS[field]
    violations, res = c.check_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED)
    assert violations == [] and res.copies_checked == 1 and res.num_copy_violations == 0 and res.num_gate_violations == 0
    violations, res = c.check(pw, rng=np.random.default_rng(RNG), seed=SEED)
    assert violations == [] and res.copies_checked == 1
    values = c.generate_partition_device(pw, rng=np.random.default_rng(RNG), seed=SEED)
    want = RS.blinding(SEED, _P(p), len(c.blinding_targets))
    cells = np.array([c.target_index(t) for t in c.blinding_targets], dtype=np.int64)
    assert (c.representative_map[cells] == cells.astype(np.uint64)).all()                      # blinding cells stand alone
    bad = np.flatnonzero(values[cells] != want)
    assert bad.size == 0, "blinding value %d is %d, the stream has %d" % (bad[0], values[cells][bad[0]], want[bad[0]])
    assert (c.blinding_values(SEED) == want).all()
    # the Z pairs: the second row's routed wires equal the first's
    nw, nr = c.config.num_wires, c.config.num_routed_wires
    regular = (len(c.blinding_targets) - nr * c_pairs(c)) // nw
    first_pair_row = int(cells[regular * nw]) // nw
    for k in range(c_pairs(c)):
        r = first_pair_row + 2 * k
        a = values[r * nw:r * nw + nr]
        b = values[(r + 1) * nw:(r + 1) * nw + nr]
        assert (a == b).all() and (a == want[regular * nw + k * nr:regular * nw + (k + 1) * nr]).all()
    assert int(cells[-1]) // nw == first_pair_row + 2 * (c_pairs(c) - 1)
    # the host path places the same values
    host = c.generate_partition_witness(pw, rng=np.random.default_rng(RNG), seed=SEED)
    assert (host[cells] == want).all()


def c_pairs(c):
    """z of the built circuit: regular * num_wires + z * num_routed targets with z = regular + D"""
    nw, nr, D = c.config.num_wires, c.config.num_routed_wires, c.F.ext_degree
    z = (len(c.blinding_targets) + D * nw) // (nw + nr)
    assert (z - D) * nw + z * nr == len(c.blinding_targets)
    return z


def test_stock_goldilocks_config_at_2_14_rows(ctx):
    b, pw = Z.factorial(Z.config(N.GB_GOLDILOCKS))
    c = b.build(ctx)
    assert c.degree_bits == 14 and len(c.blinding_targets) == 2774 * 135 + 2776 * 80
    proof = c.prove_inputs(pw, rng=np.random.default_rng(RNG), seed=SEED)
    assert c.verify(proof)
    c.data.free()
