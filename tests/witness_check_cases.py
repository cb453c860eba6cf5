"""What the witness check (gb_check_witness, csrc/kernels_check.hip) has to report, from code that does not know the checker:
oracle/gates.py's compute_filter and eval_unfiltered on every row of the witness, GateProgram.evaluate for program gates, and a
few lines of numpy over the representative map for the copy constraints.  Shared by tests/test_gpu_witness_check.py, the ABI
test and the sanitized host program's driver.  No GPU code."""
import numpy as np

from oracle import gates as G
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.gate_program import GATE_PROGRAM
from plonky2_goldibear_amd.native import Violation

FIELDS = {N.GB_GOLDILOCKS: GL, N.GB_BABYBEAR: BB}
NO_GATE, BAD_SELECTOR = "unused", "bad"


def pi_hash(F, public_inputs):
    """the public inputs' hash as gb_prove computes it (plonk/prover.rs:244)"""
    return [int(x) for x in F.hash_no_pad(np.asarray(list(public_inputs), dtype=F.dtype))]


def column_group(gate_table, col):
    """(group_start, group_end) of the gates that share selector column col"""
    for g in gate_table:
        if g[2] == col:
            return g[3], g[4]
    return None


def active_gate(F, gate_table, num_selectors, col, s):
    """the gate whose filter (oracle/gates.py compute_filter, gates/gate.rs:391-404) is non-zero where selector column col holds
    s; NO_GATE where every filter of the group is zero (UNUSED_SELECTOR); BAD_SELECTOR where s is neither an index of the group nor
    UNUSED_SELECTOR: every filter of the group is non-zero there"""
    many = num_selectors > 1
    grp = column_group(gate_table, col)
    members = [g for g in range(*grp) if gate_table[g][2] == col] if grp else []
    live = [g for g in members if any(G.compute_filter(F, g, gate_table[g], F.efrom(int(s)), many))]
    if int(s) in members:
        assert live == [int(s)], (col, s, live)
        return int(s)
    if many and int(s) == G.UNUSED_SELECTOR % F.P:
        assert live == []
        return NO_GATE
    assert live == members     # no factor of any filter vanishes: the group's gates would all be active
    return BAD_SELECTOR


def constraints(F, gate, wires, consts, pih, programs=None):
    """eval_unfiltered of one row as base-field integers, in the order gates.hpp and oracle/gates.py share"""
    if gate[0] == GATE_PROGRAM:
        return [int(c) % F.P for c in programs[gate[1]].evaluate([int(w) for w in wires], [int(k) for k in consts])]
    out = G.eval_unfiltered(F, tuple(gate), [F.efrom(int(w)) for w in wires], [F.efrom(int(k)) for k in consts], pih)
    assert not any(any(c[1:]) for c in out)    # base-field wires give base-field constraints
    return [int(c[0]) for c in out]


def first_failure(F, gate, wires, consts, pih, programs=None):
    """(index, value) of the first constraint that is not zero, or None"""
    for i, c in enumerate(constraints(F, gate, wires, consts, pih, programs)):
        if c:
            return i, c
    return None


def gate_and_selector_violations(F, gate_table, num_selectors, num_constants, constants_sigmas, witness, public_inputs=(), programs=None):
    """-> (selector violations by (row, column), gate violations by (row, gate)) over every row"""
    cs = np.asarray(constants_sigmas)
    w = np.asarray(witness)
    pih = pi_hash(F, public_inputs)
    sel, gate = [], []
    for row in range(w.shape[1]):
        for col in range(num_selectors):
            s = int(cs[col, row])
            g = active_gate(F, gate_table, num_selectors, col, s)
            if g == BAD_SELECTOR:
                sel.append(Violation(N.GB_VIOLATION_SELECTOR, row=row, index=col, value=s))
            elif g != NO_GATE:
                f = first_failure(F, gate_table[g], w[:, row], cs[num_selectors:num_selectors + num_constants, row], pih, programs)
                if f:
                    gate.append(Violation(N.GB_VIOLATION_GATE, gate=g, row=row, index=f[0], value=f[1]))
    return sel, sorted(gate, key=lambda v: (v.row, v.gate))


def copy_violations(representative_map, witness):
    """every wire cell whose value differs from the value of the first cell (lowest row * num_wires + column) of its class, by
    cell index; the classes are those of the representative map"""
    w = np.asarray(witness)
    nw, n = w.shape
    cells = np.arange(nw * n)
    reps = np.asarray(representative_map)[:nw * n].astype(np.int64)
    first = np.full(len(representative_map), nw * n, dtype=np.int64)
    np.minimum.at(first, reps, cells)
    vals = w.T.reshape(-1)                   # by cell index
    fc = first[reps]
    return [Violation(N.GB_VIOLATION_COPY, row=c // nw, index=c % nw, other_wire=int(fc[c]) % nw, other_row=int(fc[c]) // nw,
                      value=int(vals[c]), other_value=int(vals[fc[c]])) for c in np.flatnonzero(vals != vals[fc])]


def expected(built, witness, public_inputs=(), copies=True):
    """the full, ordered list for a circuit of circuit_builder.BuiltCircuit: selector, gate, then copy violations"""
    F = FIELDS[built.config.field]
    sel, gate = gate_and_selector_violations(F, built.gate_table, built.num_selectors, built.max_constants, built.constants_sigmas,
                                             witness, public_inputs, built.programs)
    return sel + gate + (copy_violations(built.representative_map, witness) if copies else [])


def expected_dummy(circ, witness, public_inputs=()):
    """the same for a circuit of plain gb_circuit_create (oracle/plonk_dummy.py BuiltCircuit: one selector column, the gate index
    is the selector value); no partition, so no copy violations"""
    return sum(gate_and_selector_violations(circ.F, circ.gate_table, 1, circ.cfg.num_constants, circ.constants_sigmas, witness,
                                            public_inputs), [])


def counts(violations):
    """(gate, selector, copy) counts of a list"""
    return tuple(sum(v.kind == k for v in violations) for k in (N.GB_VIOLATION_GATE, N.GB_VIOLATION_SELECTOR, N.GB_VIOLATION_COPY))


def same(got, want):
    """compare two lists of violations, with a readable message"""
    assert [v.as_tuple() for v in got] == [v.as_tuple() for v in want], "\n got  %r\n want %r" % (got[:6], want[:6])


def row_lists(F, gate_table, num_selectors, selector_columns):
    """the row list of every gate and the list of rows with a selector violation (ascending), as the preparation builds them:
    -> (counts [num_gates + 1], offsets [num_gates + 2], rows)"""
    sel = np.asarray(selector_columns)
    lists = [[] for _ in range(len(gate_table) + 1)]
    for row in range(sel.shape[1]):
        bad = False
        for col in range(num_selectors):
            g = active_gate(F, gate_table, num_selectors, col, int(sel[col, row]))
            if g == BAD_SELECTOR:
                bad = True
            elif g != NO_GATE:
                lists[g].append(row)
        if bad:
            lists[-1].append(row)
    cnt = [len(x) for x in lists]
    return cnt, [sum(cnt[:i]) for i in range(len(cnt) + 1)], [r for x in lists for r in x]
