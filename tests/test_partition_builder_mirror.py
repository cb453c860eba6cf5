"""CircuitBuilder.build records ProverOnlyCircuitData.representative_map and the public-input targets with the reference's
indexing (Target::index, iop/target.rs:55-60: wire (row, col) -> row * num_wires + col, virtual i -> n * num_wires + i), and
BuiltCircuit.generate_partition_witness returns PartitionWitness.values without expanding them: values[representative_map[...]]
reshaped and transposed IS generate_witness's matrix, and the public inputs read through the map are the returned ones.
Factorial, fibonacci and a BabyBear circuit.  CPU only: the circuits are built without a context."""
import numpy as np
import pytest

import circuits as CS
import partition_cases as PC

CASES = {"factorial": lambda: CS.factorial_circuit(count=40), "fibonacci": lambda: CS.fibonacci_circuit(terms=40),
         "babybear": lambda: CS.babybear_public_input_circuit(steps=20)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_partition_witness_expands_to_the_matrix(name):
    b, pw = CASES[name]()
    built = b.build(None)
    nw, n = built.config.num_wires, 1 << built.degree_bits
    cells = nw * n
    m = built.representative_map
    assert m.dtype == np.uint64 and m.shape == (built.num_targets,) and built.num_targets == cells + b.virtual_target_index
    assert b.virtual_target_index > 0 and int(m.max()) < built.num_targets
    assert np.array_equal(m[m.astype(np.int64)], m)                       # a representative represents itself
    wires, pis = built.generate_witness(pw, np.random.default_rng(5))
    values = built.generate_partition_witness(pw, np.random.default_rng(5))
    assert values.dtype == wires.dtype and values.shape == (built.num_targets,)
    assert np.array_equal(PC.expand(m, values, n, nw), wires)
    assert (wires != 0).sum() > n                                          # (not a comparison of zeros)
    t = built.public_input_targets
    assert len(t) == len(pis) > 0 and (t >= cells).any()                   # registered on virtual targets (and on wires)
    assert [int(v) for v in values[m[t.astype(np.int64)].astype(np.int64)]] == [int(v) for v in pis]
    # the virtual public inputs are connected to PublicInputGate-hashed wires: their classes reach wire cells
    reps, _, _ = PC.slot_map(m, cells)
    assert set(m[t.astype(np.int64)].tolist()) <= set(reps.tolist())
    # the random wire is alone in its class: what gb_prove_partition_retry re-draws is one cell
    row, col = built.random_wire
    assert (m[:cells] == m[row * nw + col]).sum() == 1
