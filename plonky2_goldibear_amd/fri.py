"""The polynomial commitment scheme on its own: PolynomialBatch::prove_openings on any FriInstanceInfo and verify_fri_proof.

Same names and fields as plonky2/src/fri/structure.rs (FriInstanceInfo, FriOracleInfo, FriBatchInfo, FriPolynomialInfo) and
plonky2/src/fri/mod.rs (FriConfig, FriParams).  A host that keeps the reference's prover loop - a circuit with lookup tables,
a STARK over this crate's FRI - commits with PolynomialBatch.from_values / from_coeffs, evaluates with eval_ext, and opens here:

    proof, challenger = prove_openings(instance, oracles, challenger, fri_params)      # on the GPU
    verify_fri_proof(instance, openings, challenger, initial_merkle_caps, proof, fri_params)   # on the host

A challenger is (sponge_state, input_buffer, output_buffer) of canonical ints, as CircuitData.prove_openings takes it; points
and openings are D canonical words each.
"""
import ctypes as C
from dataclasses import dataclass, field as _field
from typing import List, Sequence

import numpy as np

from . import native as N
from .polynomial_batch import PolynomialBatch, _dtype
from .prover import gb_challenger_state


@dataclass
class FriOracleInfo:
    num_polys: int
    blinding: bool


@dataclass
class FriPolynomialInfo:
    oracle_index: int       # index into FriInstanceInfo.oracles
    polynomial_index: int   # index of the polynomial within that oracle

    @staticmethod
    def from_range(oracle_index, polynomial_indices):
        """structure.rs:60-71"""
        return [FriPolynomialInfo(oracle_index, int(i)) for i in polynomial_indices]


@dataclass
class FriBatchInfo:
    point: Sequence[int]                  # F::Extension: D canonical words
    polynomials: List[FriPolynomialInfo]


@dataclass
class FriInstanceInfo:
    oracles: List[FriOracleInfo]
    batches: List[FriBatchInfo]


@dataclass
class FriConfig:
    rate_bits: int
    cap_height: int
    proof_of_work_bits: int
    num_query_rounds: int
    reduction_strategy: tuple = None      # fri_params.reduction_arity_bits' strategy tuple; FriParams carries the list itself


@dataclass
class FriParams:
    config: FriConfig
    hiding: bool
    degree_bits: int
    reduction_arity_bits: List[int] = _field(default_factory=list)


def _challenger_state(challenger, fld):
    st, inp, outb = challenger
    w = 12 if fld == N.GB_GOLDILOCKS else 16
    if len(st) != w or len(inp) > 8 or len(outb) > 8:
        raise N.ShapeError(N.GB_ERR_INVALID, "challenger state has the wrong shape")
    cs = gb_challenger_state()
    for i, v in enumerate(st):
        cs.sponge_state[i] = int(v)
    for i, v in enumerate(inp):
        cs.input_buffer[i] = int(v)
    for i, v in enumerate(outb):
        cs.output_buffer[i] = int(v)
    cs.input_len, cs.output_len = len(inp), len(outb)
    return cs, w


def _challenger_tuple(cs, w):
    return ([int(cs.sponge_state[i]) for i in range(w)], [int(cs.input_buffer[i]) for i in range(cs.input_len)],
            [int(cs.output_buffer[i]) for i in range(cs.output_len)])


def _flatten(instance, fld):
    """-> (points [num_batches][D], batch_sizes, polynomials [sum][2]) as the C ABI takes an instance"""
    d = 2 if fld == N.GB_GOLDILOCKS else 4
    pts = np.zeros((len(instance.batches), d), dtype=_dtype(fld))
    for b, batch in enumerate(instance.batches):
        p = [int(x) for x in batch.point]
        if len(p) != d:
            raise N.ShapeError(N.GB_ERR_INVALID, "the point of batch %d must have %d coordinates" % (b, d))
        if any(x < 0 or x >= (1 << (8 * pts.itemsize)) for x in p):
            raise N.ShapeError(N.GB_ERR_INVALID, "the point of batch %d has a coordinate that is no field word" % b)
        pts[b] = p
    sizes = np.array([len(b.polynomials) for b in instance.batches], dtype=np.uint32)
    polys = np.array([[p.oracle_index, p.polynomial_index] for b in instance.batches for p in b.polynomials],
                     dtype=np.int64).reshape(-1, 2)
    if polys.size and (polys.min() < 0 or polys.max() >= 1 << 32):
        raise N.ShapeError(N.GB_ERR_INVALID, "oracle_index / polynomial_index out of range")
    return pts, sizes, np.ascontiguousarray(polys, dtype=np.uint32)


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def prove_openings(instance, oracles, challenger, fri_params, out_cap=None):
    """PolynomialBatch::prove_openings (fri/oracle.rs:187-246) -> (FriProof bytes, challenger afterwards).
    oracles: the PolynomialBatch of every instance.oracles[i], committed on one context; `challenger`: the transcript after the
    openings were observed.  On any error the challenger handed back is the one passed in.  out_cap (tests): the capacity
    handed to the library; 0 is a size query (raises, status GB_ERR_BUFFER_TOO_SMALL, with the size in e.fri_proof_len)."""
    oracles = list(oracles)
    if not oracles or len(oracles) != len(instance.oracles):
        raise N.ShapeError(N.GB_ERR_INVALID, "one PolynomialBatch per FriOracleInfo is expected")
    for i, (info, b) in enumerate(zip(instance.oracles, oracles)):
        if b is None or not isinstance(b, PolynomialBatch):
            raise N.ShapeError(N.GB_ERR_INVALID, "oracle %d is not a PolynomialBatch" % i)
        if info.num_polys != b.num_polys:
            raise N.ShapeError(N.GB_ERR_INVALID, "oracle %d: FriOracleInfo.num_polys = %d, the batch has %d polynomials" % (i, info.num_polys, b.num_polys))
        if bool(info.blinding) != b.blinding:
            raise N.ShapeError(N.GB_ERR_INVALID, "oracle %d: FriOracleInfo.blinding does not match the batch's salts" % i)
    ctx, fld = oracles[0].ctx, oracles[0].field
    if fri_params.degree_bits != oracles[0].degree_log or fri_params.config.rate_bits != oracles[0].rate_bits or \
            fri_params.config.cap_height != oracles[0].cap_height:
        raise N.ShapeError(N.GB_ERR_INVALID, "FriParams (degree_bits, rate_bits, cap_height) differ from the oracles'")
    pts, sizes, polys = _flatten(instance, fld)
    cs, w = _challenger_state(challenger, fld)
    handles = (C.c_void_p * len(oracles))(*[b.handle for b in oracles])
    arity = np.array(list(fri_params.reduction_arity_bits), dtype=np.uint32)
    lib = ctx._lib
    n = C.c_size_t()

    def call(buf, cap):
        return lib.gb_fri_prove_openings(ctx.handle, handles, len(oracles), pts.ctypes.data, _u32p(sizes), len(sizes), _u32p(polys),
                                         _u32p(arity), len(arity), fri_params.config.proof_of_work_bits,
                                         fri_params.config.num_query_rounds, C.byref(cs), buf, cap, C.byref(n))
    if out_cap is None:   # a buffer that holds any ordinary FriProof; a larger one is proved again into the size the library names
        buf = np.empty(8 << 20, dtype=np.uint8)
        st = call(buf.ctypes.data, buf.size)
        if st == N.GB_ERR_BUFFER_TOO_SMALL:
            buf = np.empty(n.value, dtype=np.uint8)
            st = call(buf.ctypes.data, buf.size)
    else:
        buf = np.empty(max(int(out_cap), 1), dtype=np.uint8)
        st = call(buf.ctypes.data if out_cap else None, int(out_cap))
    try:
        N.check(st, ctx.handle)
    except N.GoldibearError as e:
        e.fri_proof_len, e.challenger = n.value, _challenger_tuple(cs, w)
        raise
    return buf[: n.value].tobytes(), _challenger_tuple(cs, w)


def verify_fri_proof(instance, openings, challenger, initial_merkle_caps, proof, params, field=N.GB_GOLDILOCKS, ctx=None):
    """verify_fri_proof (fri/verifier.rs:67-250), on the host: True, or raises VerifyError naming the failed check (ShapeError for
    malformed bytes or arguments).  openings: FriOpenings - per batch the values of its polynomials at its point, [size][D];
    initial_merkle_caps: per oracle [2^cap_height][H]; challenger: the transcript after the openings were observed (not advanced)."""
    fld = field
    d = 2 if fld == N.GB_GOLDILOCKS else 4
    hh = 4 if fld == N.GB_GOLDILOCKS else 8
    dt = _dtype(fld)
    pts, sizes, polys = _flatten(instance, fld)
    if len(openings) != len(instance.batches):
        raise N.ShapeError(N.GB_ERR_INVALID, "one list of openings per batch is expected")
    flat = []
    for b, (vals, batch) in enumerate(zip(openings, instance.batches)):
        v = np.ascontiguousarray(vals, dtype=dt).reshape(-1, d)
        if v.shape[0] != len(batch.polynomials):
            raise N.ShapeError(N.GB_ERR_INVALID, "batch %d: %d openings for %d polynomials" % (b, v.shape[0], len(batch.polynomials)))
        flat.append(v)
    op = np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros((0, d), dtype=dt)
    if len(initial_merkle_caps) != len(instance.oracles):
        raise N.ShapeError(N.GB_ERR_INVALID, "one Merkle cap per oracle is expected")
    cap_h = params.config.cap_height
    caps = np.ascontiguousarray(np.stack([np.ascontiguousarray(c, dtype=dt).reshape(-1, hh) for c in initial_merkle_caps]))
    if caps.shape[1] != 1 << cap_h:
        raise N.ShapeError(N.GB_ERR_INVALID, "a Merkle cap has 2^cap_height digests")
    nump = np.array([o.num_polys for o in instance.oracles], dtype=np.uint32)
    blind = np.array([1 if o.blinding else 0 for o in instance.oracles], dtype=np.uint32)
    arity = np.array(list(params.reduction_arity_bits), dtype=np.uint32)
    cs, _ = _challenger_state(challenger, fld)
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    h = ctx.handle if ctx is not None else None
    st = N.load().gb_fri_verify(h, fld, params.degree_bits, params.config.rate_bits, cap_h, int(bool(params.hiding)), _u32p(nump),
                                _u32p(blind), len(nump), pts.ctypes.data, _u32p(sizes), len(sizes), _u32p(polys), op.ctypes.data,
                                caps.ctypes.data, _u32p(arity), len(arity), params.config.proof_of_work_bits,
                                params.config.num_query_rounds, C.byref(cs), buf.ctypes.data, buf.size)
    N.check(st, h)
    return True


def _shape_of(instance):
    """what the items of verify_fri_proofs must share: everything of the instance but its points"""
    return ([(int(o.num_polys), bool(o.blinding)) for o in instance.oracles],
            [[(int(p.oracle_index), int(p.polynomial_index)) for p in b.polynomials] for b in instance.batches])


def verify_fri_proofs(ctx, items, params, field=N.GB_GOLDILOCKS):
    """gb_fri_verify_batch: verify_fri_proof of many proofs on ONE instance shape, the query rounds on the device of `ctx` ->
    [native.VerifyResult], one per item.  items: (instance, openings, challenger, initial_merkle_caps, proof) as verify_fri_proof
    takes them; the instances must agree in everything but their points (ShapeError names the first item that differs - group
    proofs of several shapes by shape).  A failing proof is reported, not raised, as in verify_batch; malformed arguments raise."""
    fld = field
    d = 2 if fld == N.GB_GOLDILOCKS else 4
    hh = 4 if fld == N.GB_GOLDILOCKS else 8
    dt = _dtype(fld)
    items = list(items)
    n = len(items)
    if not n:
        return []
    first = items[0][0]
    shape = _shape_of(first)
    _, sizes, polys = _flatten(first, fld)
    cap_h = params.config.cap_height
    keep = []   # the arrays the pointer tables name
    pts_t, op_t, cap_t, proof_t = ((C.c_void_p * n)() for _ in range(4))
    lens = (C.c_size_t * n)()
    chs = (gb_challenger_state * n)()
    empty = np.zeros(1, dtype=np.uint8)
    for i, (instance, openings, challenger, caps, proof) in enumerate(items):
        if i and _shape_of(instance) != shape:
            raise N.ShapeError(N.GB_ERR_INVALID, "item %d: its instance differs from item 0's in more than the points" % i)
        pts, _, _ = _flatten(instance, fld)
        if len(openings) != len(instance.batches):
            raise N.ShapeError(N.GB_ERR_INVALID, "item %d: one list of openings per batch is expected" % i)
        flat = []
        for b, (vals, batch) in enumerate(zip(openings, instance.batches)):
            v = np.ascontiguousarray(vals, dtype=dt).reshape(-1, d)
            if v.shape[0] != len(batch.polynomials):
                raise N.ShapeError(N.GB_ERR_INVALID, "item %d, batch %d: %d openings for %d polynomials" % (i, b, v.shape[0], len(batch.polynomials)))
            flat.append(v)
        op = np.ascontiguousarray(np.concatenate(flat))
        if len(caps) != len(instance.oracles):
            raise N.ShapeError(N.GB_ERR_INVALID, "item %d: one Merkle cap per oracle is expected" % i)
        cp = np.ascontiguousarray(np.stack([np.ascontiguousarray(c, dtype=dt).reshape(-1, hh) for c in caps]))
        if cp.shape[1] != 1 << cap_h:
            raise N.ShapeError(N.GB_ERR_INVALID, "item %d: a Merkle cap has 2^cap_height digests" % i)
        buf = np.frombuffer(bytes(proof), dtype=np.uint8)
        keep.append((pts, op, cp, buf))
        pts_t[i], op_t[i], cap_t[i] = pts.ctypes.data, op.ctypes.data, cp.ctypes.data
        proof_t[i] = buf.ctypes.data if buf.size else empty.ctypes.data   # (an empty proof is a truncated one, not a missing argument)
        lens[i] = buf.size
        chs[i] = _challenger_state(challenger, fld)[0]
    nump = np.array([o.num_polys for o in first.oracles], dtype=np.uint32)
    blind = np.array([1 if o.blinding else 0 for o in first.oracles], dtype=np.uint32)
    arity = np.array(list(params.reduction_arity_bits), dtype=np.uint32)
    res = (N.gb_verify_result * n)()
    lib = N.load()
    h = ctx.handle if ctx is not None else None
    st = lib.gb_fri_verify_batch(h, fld, params.degree_bits, params.config.rate_bits, cap_h, int(bool(params.hiding)), _u32p(nump),
                                 _u32p(blind), len(nump), _u32p(sizes), len(sizes), _u32p(polys), _u32p(arity), len(arity),
                                 params.config.proof_of_work_bits, params.config.num_query_rounds, pts_t, op_t, cap_t,
                                 C.cast(chs, C.c_void_p), proof_t, lens, n, 0, C.cast(res, C.c_void_p))
    if st not in (N.GB_OK, N.GB_ERR_VERIFY):
        N.check(st, h)
    return [N.VerifyResult(r.status, r.check, (lib.gb_verify_check_text(r.check) or b"").decode(), r.query_round, r.index) for r in res]


def fri_verify_batch_counts(ctx):
    """gb_fri_verify_batch_counts -> (device_items, host_items) of verify_fri_proofs on `ctx` since it was created"""
    dev, host = C.c_uint64(), C.c_uint64()
    N.check(N.load().gb_fri_verify_batch_counts(ctx.handle, C.byref(dev), C.byref(host)), ctx.handle)
    return dev.value, host.value


PolynomialBatch.prove_openings = staticmethod(prove_openings)
