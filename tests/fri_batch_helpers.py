"""gb_fri_verify_batch through ctypes, as the tests of the batch call need it (no GPU code, not a test file): the raw call with
every table in the caller's hands - so that a NULL context, a NULL table or a changed word can be passed - and gb_fri_verify on
one item for comparison."""
import ctypes as C

import numpy as np

from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.fri import _challenger_state, _flatten, _u32p
from plonky2_goldibear_amd.polynomial_batch import _dtype
from plonky2_goldibear_amd.prover import gb_challenger_state

NONE = 0xFFFFFFFF


def dims(fld):
    """(D, H) of the field"""
    return (2, 4) if fld == N.GB_GOLDILOCKS else (4, 8)


class Item:
    """one item's arrays: points [num_batches][D], openings [sum][D], caps [num_oracles][2^cap_height][H], challenger tuple, bytes"""

    def __init__(self, fld, instance, openings, challenger, caps, proof):
        d, hh = dims(fld)
        dt = _dtype(fld)
        self.points = _flatten(instance, fld)[0]
        self.openings = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=dt).reshape(-1, d) for v in openings]))
        self.caps = np.ascontiguousarray(np.stack([np.asarray(c, dtype=dt).reshape(-1, hh) for c in caps]))
        self.challenger = challenger
        self.proof = bytes(proof)

    def copy(self, **changes):
        it = Item.__new__(Item)
        it.points, it.openings, it.caps = self.points.copy(), self.openings.copy(), self.caps.copy()
        it.challenger, it.proof = self.challenger, self.proof
        for k, v in changes.items():
            setattr(it, k, v)
        return it


def shape_arrays(instance, params):
    nump = np.array([o.num_polys for o in instance.oracles], dtype=np.uint32)
    blind = np.array([1 if o.blinding else 0 for o in instance.oracles], dtype=np.uint32)
    arity = np.array(list(params.reduction_arity_bits), dtype=np.uint32)
    return nump, blind, arity


def raw_batch(ctx_handle, fld, instance, params, items, flags=0, num_items=None, null_tables=(), null_entries=(), with_challengers=False):
    """-> (status, [(status, check, query_round, index)]).  null_tables: names among points / openings / caps / challengers /
    proofs / lens / results passed as NULL; null_entries: (table name, item) pairs whose entry is NULL.  with_challengers: also the
    bytes of the challenger states as they were handed over and as the call left them."""
    lib = N.load()
    _, sizes, polys = _flatten(instance, fld)
    nump, blind, arity = shape_arrays(instance, params)
    n = len(items)
    tabs = {k: (C.c_void_p * max(n, 1))() for k in ("points", "openings", "caps", "proofs")}
    lens = (C.c_size_t * max(n, 1))()
    chs = (gb_challenger_state * max(n, 1))()
    keep = []
    for i, it in enumerate(items):
        buf = np.frombuffer(it.proof if it.proof else b"\0", dtype=np.uint8)
        keep.append(buf)
        tabs["points"][i], tabs["openings"][i], tabs["caps"][i] = it.points.ctypes.data, it.openings.ctypes.data, it.caps.ctypes.data
        tabs["proofs"][i] = buf.ctypes.data
        lens[i] = len(it.proof)
        chs[i] = _challenger_state(it.challenger, fld)[0]
    for name, i in null_entries:
        tabs[name][i] = None
    res = (N.gb_verify_result * max(n, 1))()
    for r in res:
        r.status, r.check = 0xAAAA, 0xAAAA
    arg = lambda name, v: None if name in null_tables else v
    chs_before = bytes(chs)
    st = lib.gb_fri_verify_batch(ctx_handle, fld, params.degree_bits, params.config.rate_bits, params.config.cap_height,
                                 int(bool(params.hiding)), _u32p(nump), _u32p(blind), len(nump), _u32p(sizes), len(sizes), _u32p(polys),
                                 _u32p(arity), len(arity), params.config.proof_of_work_bits, params.config.num_query_rounds,
                                 arg("points", tabs["points"]), arg("openings", tabs["openings"]), arg("caps", tabs["caps"]),
                                 arg("challengers", C.cast(chs, C.c_void_p)), arg("proofs", tabs["proofs"]), arg("lens", lens),
                                 n if num_items is None else num_items, flags, arg("results", C.cast(res, C.c_void_p)))
    out = [(r.status, r.check, r.query_round, r.index) for r in res[:n]]
    return (st, out, chs_before, bytes(chs)) if with_challengers else (st, out)


def single(ctx_handle, fld, instance, params, it):
    """gb_fri_verify on one item -> (status, message)"""
    lib = N.load()
    _, sizes, polys = _flatten(instance, fld)
    nump, blind, arity = shape_arrays(instance, params)
    cs = _challenger_state(it.challenger, fld)[0]
    buf = np.frombuffer(it.proof if it.proof else b"\0", dtype=np.uint8)
    st = lib.gb_fri_verify(ctx_handle, fld, params.degree_bits, params.config.rate_bits, params.config.cap_height, int(bool(params.hiding)),
                           _u32p(nump), _u32p(blind), len(nump), it.points.ctypes.data, _u32p(sizes), len(sizes), _u32p(polys),
                           it.openings.ctypes.data, it.caps.ctypes.data, _u32p(arity), len(arity), params.config.proof_of_work_bits,
                           params.config.num_query_rounds, C.byref(cs), buf.ctypes.data, len(it.proof))
    msg = lib.gb_last_error(ctx_handle) if st else b""
    return st, (msg or b"").decode()


def plonk_item(F, cd, circuit_digest, constants_sigmas_cap, raw):
    """a PLONK proof's FRI part as an item on the circuit's instance (fri_instance(cd, zeta), plonk/circuit_data.rs:438-520)
    -> (instance, params, Item, FriProof dict)"""
    import fri_instances as FI
    from oracle import verifier as V
    pr, pis = V.read_proof_with_pis(raw, cd, F)
    cfg, fc, fp = cd["config"], cd["config"]["fri_config"], cd["fri_params"]
    c = cfg["num_challenges"]
    ch = F.Challenger()                     # plonk/get_challenges.rs:26-60, up to and including observe_openings
    ch.observe_hash(circuit_digest)
    ch.observe_hash(F.hash_no_pad(np.asarray(pis, dtype=F.dtype)))
    ch.observe_cap(pr["wires_cap"]); ch.get_n_challenges(2 * c)
    ch.observe_cap(pr["zs_cap"]); ch.get_n_challenges(c)
    ch.observe_cap(pr["quotient_cap"])
    zeta = ch.get_extension_challenge(F.D)
    openings = V.fri_openings(pr["openings"])
    for batch in openings:
        ch.observe_elements([x for e in batch for x in e])
    params = FI.fri_params(fp["degree_bits"], fc["rate_bits"], fc["cap_height"], fp["reduction_arity_bits"], fc["proof_of_work_bits"],
                           fc["num_query_rounds"], hiding=fp["hiding"])
    caps = [constants_sigmas_cap, pr["wires_cap"], pr["zs_cap"], pr["quotient_cap"]]
    inst = FI.plonk_instance(cd, zeta, F)
    fri = pr["opening_proof"]
    item = Item(FI.field_tag(F), inst, openings, FI.challenger_tuple(ch, F), caps, FI.write_fri_proof(F, fri))
    return inst, params, item, fri


def write_case(path, fld, instance, params, item):
    """the case file of tests/sanitize/fuzz_fri_verify_batch.cpp: ten u32 of the shape, its lists, then one item's arrays"""
    _, sizes, polys = _flatten(instance, fld)
    nump, blind, arity = shape_arrays(instance, params)
    head = np.array([fld, params.degree_bits, params.config.rate_bits, params.config.cap_height, int(bool(params.hiding)), len(nump),
                     len(sizes), len(arity), params.config.proof_of_work_bits, params.config.num_query_rounds], dtype=np.uint32)
    with open(path, "wb") as f:
        for a in (head, nump, blind, sizes, polys, arity):
            f.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        f.write(bytes(_challenger_state(item.challenger, fld)[0]))
        for a in (item.points, item.openings, item.caps):
            f.write(a.tobytes())
        f.write(np.array([len(item.proof)], dtype=np.uint64).tobytes())
        f.write(item.proof)


def check_text(check):
    return (N.load().gb_verify_check_text(check) or b"").decode()


def last_error(ctx_handle=None):
    return (N.load().gb_last_error(ctx_handle) or b"").decode()
