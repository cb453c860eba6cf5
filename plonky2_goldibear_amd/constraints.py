"""Constraint systems over committed oracles: the quotient stage for a host that proves with PolynomialBatch and fri.py and has
constraints of its own - a circuit with lookup terms, a STARK over this FRI (include/goldibear_gpu.h, "constraint systems over
committed oracles").

A constraint is a polynomial in CELLS - (oracle, polynomial, rows ahead) of the committed oracles - the point X, the Lagrange
polynomials of the first and the last row, and base-field params (the caller's challenges and public values).  A program is a list
of constraints as straight-line code, built on the expression DAG of gate_program.py:

    fib = ConstraintProgram.from_constraints(
        lambda cell, param, x, l_first, l_last: [(x - w_last) * (cell[2] - cell[1]), (x - w_last) * (cell[3] - cell[0] - cell[1]),
                                                 l_first * (cell[0] - param[0]), l_first * (cell[1] - param[1])],
        cells=[(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)], num_params=2, field=N.GB_GOLDILOCKS)
    chunks = constraint_quotient(ctx, [trace], [fib], params=[a0, a1], alphas=alphas, quotient_degree_bits=1)   # on the GPU
    folded = constraint_eval(N.GB_GOLDILOCKS, degree_bits, [fib], cell_values, [a0, a1], zeta, alphas)             # on the host

The constraints of program 0, then program 1, ... are numbered 0, 1, 2, ...; challenge c folds them as sum_i alphas[c]^i *
constraint_i.  `constraint_quotient` returns the quotient of that sum by Z_H = X^n - 1 as degree-n coefficient chunks, ready for
PolynomialBatch.from_coeffs; `constraint_eval` the folded sums at zeta from opened values, which a verifier compares with
Z_H(zeta) * sum_i zeta^(n i) * chunk_i(zeta).  `evaluate` runs the packed words on Python integers - an independent restatement
of the interpreter for tests.  Not the GPU hot path.
"""
import ctypes as C

import numpy as np

from . import native as N
from .gate_program import HEADER_WORDS, _Column, _Dag, assemble, field_order, run_words
from .polynomial_batch import _dtype

MAX_ORACLES, MAX_CELLS, MAX_PARAMS = 16, 4096, 4096
INPUT_X, INPUT_L_FIRST, INPUT_L_LAST, NUM_BUILTIN_INPUTS = 0, 1, 2, 3


def cell_word(oracle_index, polynomial_index, row_offset=0):
    """oracle_index in bits 0-15, polynomial_index in bits 16-47, row_offset (rows ahead, modulo n) in bits 48-63"""
    if not (0 <= oracle_index < 1 << 16 and 0 <= polynomial_index < 1 << 32 and 0 <= row_offset < 1 << 16):
        raise ValueError("cell (%d, %d, %d) does not fit a cell word" % (oracle_index, polynomial_index, row_offset))
    return int(oracle_index) | int(polynomial_index) << 16 | int(row_offset) << 48


class ConstraintProgram:
    """A packed constraint program over cells.  `words` is what crosses the ABI: header, literals, cell words, instructions."""

    def __init__(self, words, field):
        self.words, self.field, self.p = [int(x) for x in words], field, field_order(field)
        w = self.words
        self.num_cells, self.num_inputs = w[0] & 0xFFFFFFFF, w[0] >> 32
        self.num_constraints, self.degree = w[1] & 0xFFFFFFFF, w[1] >> 32
        self.num_regs, self.num_literals = w[2] & 0xFFFFFFFF, w[2] >> 32
        self.num_instrs = w[3]
        self.num_params = self.num_inputs - NUM_BUILTIN_INPUTS

    @property
    def literals(self):
        return self.words[HEADER_WORDS:HEADER_WORDS + self.num_literals]

    @property
    def cells(self):
        """[(oracle_index, polynomial_index, row_offset)]"""
        at = HEADER_WORDS + self.num_literals
        return [(w & 0xFFFF, (w >> 16) & 0xFFFFFFFF, w >> 48) for w in self.words[at:at + self.num_cells]]

    @property
    def instructions(self):
        return self.words[HEADER_WORDS + self.num_literals + self.num_cells:]

    @classmethod
    def from_constraints(cls, fn, cells, num_params, field, degree=None):
        """fn(cell, param, x, l_first, l_last) -> the constraints, built from cell[i], param[k], x, l_first, l_last and integers
        with + - *.  cells: [(oracle_index, polynomial_index, row_offset)], the program's cell table.  degree: the degree to
        declare when it is to be higher than the bound of the constraints (literal and param 0; cell, x, l_first, l_last 1;
        + and - the maximum, * the sum)."""
        cells = [tuple(int(v) for v in c) for c in cells]
        if len(cells) > MAX_CELLS:
            raise ValueError("%d cells, at most %d" % (len(cells), MAX_CELLS))
        if not 0 <= num_params <= MAX_PARAMS:
            raise ValueError("%d params, at most %d" % (num_params, MAX_PARAMS))
        dag = _Dag(field_order(field))
        inputs = _Column(dag, "c", NUM_BUILTIN_INPUTS + num_params)
        outs = [dag.coerce(e) for e in fn(_Column(dag, "w", len(cells)), inputs[NUM_BUILTIN_INPUTS:], inputs[INPUT_X],
                                          inputs[INPUT_L_FIRST], inputs[INPUT_L_LAST])]
        degree, num_regs, lits, instrs = assemble(
            dag, outs, degree, leaf_degree=lambda key: 0 if key[0] == "c" and key[1] >= NUM_BUILTIN_INPUTS else 1)
        header = [len(cells) | (NUM_BUILTIN_INPUTS + num_params) << 32, len(outs) | degree << 32, num_regs | len(lits) << 32, len(instrs)]
        return cls(header + lits + [cell_word(*c) for c in cells] + instrs, field)

    def evaluate(self, cell_values, params, x, l_first, l_last, coerce=int):
        """The constraints at one point on Python integers: the packed words, decoded and run.  cell_values in cell-table order.
        coerce: what an operand is made of - int, or the identity to run the words on values of another ring that have + - * and
        % p (the tests run extension-field elements through the same words)."""
        if len(cell_values) != self.num_cells or len(params) != self.num_params:
            raise ValueError("%d cell values and %d params expected" % (self.num_cells, self.num_params))
        return run_words(self.p, self.literals, self.num_regs, self.instructions, cell_values, [x, l_first, l_last] + list(params), coerce)


def pack_constraint_programs(programs):
    """[ConstraintProgram | list of words] -> (program_words uint64, program_offsets uint32[num_programs + 1])"""
    words, offsets = [], [0]
    for pr in programs:
        words += [int(x) for x in (pr.words if isinstance(pr, ConstraintProgram) else pr)]
        offsets.append(len(words))
    return np.array(words or [0], dtype=np.uint64), np.array(offsets, dtype=np.uint32)


def _words(values, field, what):
    """canonical-width words of a list of ints, as they are: the library checks them against p"""
    dt = _dtype(field)
    vals = [int(v) for v in values]
    if any(v < 0 or v >> (8 * np.dtype(dt).itemsize) for v in vals):
        raise N.ShapeError(N.GB_ERR_INVALID, "%s has an entry that is no field word" % what)
    return np.array(vals, dtype=dt)


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def constraint_quotient(ctx, oracles, programs, params, alphas, quotient_degree_bits, device=False):
    """gb_constraint_quotient: the quotient of the alpha-folded constraints of `programs` over the LDEs of `oracles`
    (PolynomialBatch commitments on `ctx`) -> [len(alphas) * 2^quotient_degree_bits][n] canonical coefficients, chunk i of
    challenge c at row c * 2^quotient_degree_bits + i; a host array, or with device=True a torch tensor on the context's device."""
    oracles = list(oracles)
    handles = (C.c_void_p * max(len(oracles), 1))(*[getattr(b, "handle", None) for b in oracles])
    first = next((b for b in oracles if b is not None), None)
    fld = first.field if first is not None else N.GB_GOLDILOCKS
    n = 1 << (first.degree_log if first is not None and hasattr(first, "degree_log") else 0)
    words, offsets = pack_constraint_programs(programs)
    par, al = _words(params, fld, "params"), _words(alphas, fld, "alphas")
    rows = len(al) << min(int(quotient_degree_bits), 8)
    if device:
        import torch
        out = torch.empty((rows, n), dtype=torch.int64 if fld == N.GB_GOLDILOCKS else torch.int32, device="cuda:%d" % ctx.device)
        optr, flags = out.data_ptr(), N.GB_INPUT_DEVICE
    else:
        out = np.empty((rows, n), dtype=_dtype(fld))
        optr, flags = out.ctypes.data, N.GB_INPUT_HOST
    st = ctx._lib.gb_constraint_quotient(ctx.handle, handles, len(oracles), _u64p(words), _u32p(offsets), len(offsets) - 1,
                                         par.ctypes.data if par.size else None, par.size, al.ctypes.data if al.size else None, al.size,
                                         int(quotient_degree_bits), flags, optr)
    N.check(st, ctx.handle)
    return out


def constraint_eval(field, degree_bits, programs, cell_values, params, zeta, alphas, ctx=None):
    """gb_constraint_eval, on the host: the folded constraints at the extension point zeta from opened values ->
    [len(alphas)][D] canonical words, NOT divided by Z_H.  cell_values: [total cells][D] in cell-table order, program after
    program (a cell with row offset k: its polynomial's opening at zeta * w_n^k); zeta: [D]."""
    d = 2 if field == N.GB_GOLDILOCKS else 4
    dt = _dtype(field)
    words, offsets = pack_constraint_programs(programs)
    par, al = _words(params, field, "params"), _words(alphas, field, "alphas")
    cv = _words(np.asarray(cell_values, dtype=object).reshape(-1), field, "cell_values").reshape(-1, d)
    z = _words(zeta, field, "zeta")
    if z.shape != (d,):
        raise N.ShapeError(N.GB_ERR_INVALID, "zeta must have %d coordinates" % d)
    total = sum(pr.num_cells if isinstance(pr, ConstraintProgram) else int(pr[0]) & 0xFFFFFFFF for pr in programs)
    if cv.shape[0] != total:
        raise N.ShapeError(N.GB_ERR_INVALID, "%d cell values for %d cells" % (cv.shape[0], total))
    out = np.zeros((max(al.size, 1), d), dtype=dt)
    h = ctx.handle if ctx is not None else None
    st = N.load().gb_constraint_eval(h, field, int(degree_bits), _u64p(words), _u32p(offsets), len(offsets) - 1,
                                     cv.ctypes.data if cv.size else None, par.ctypes.data if par.size else None, par.size,
                                     z.ctypes.data, al.ctypes.data if al.size else None, al.size, out.ctypes.data)
    N.check(st, h)
    return out[:al.size]
