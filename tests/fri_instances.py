"""FRI instances for the opening tests, and their yardsticks on Python integers (no GPU code, not a test file).

  * seeded FriInstanceInfo descriptions over three oracles (general_instance) and one that falls apart into more runs than any
    small table holds (many_runs_instance);
  * final_poly_ref: PolynomialBatch::prove_openings' final polynomial (fri/oracle.rs:208-224) and the coefficient fold of
    fri_committed_trees (fri/prover.rs:83-133) in oracle/fields.py's arithmetic;
  * verify_fri_instance: oracle.verifier.verify_fri with the instance handed in instead of taken from fri_instance(cd, zeta) -
    the same reduce_with_alpha, compute_evaluation, pow_ok, F.merkle_verify and Reader.  It names the kind of the check that failed.
"""
import copy
import struct

import numpy as np

from oracle import verifier as V
from oracle.fields import BB, GL
from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.fri import FriBatchInfo, FriConfig, FriInstanceInfo, FriOracleInfo, FriParams, FriPolynomialInfo

KINDS = ("pow", "merkle", "consistency", "final")


class FriReject(Exception):
    def __init__(self, kind, detail=""):
        super().__init__("%s %s" % (kind, detail))
        self.kind = kind


def kind_of_message(msg):
    """the kind of check a GB_ERR_VERIFY message of the library names"""
    for needle, kind in (("proof of work", "pow"), ("Merkle path does not lead", "merkle"), ("consistency", "consistency"),
                         ("Final polynomial", "final")):
        if needle in msg:
            return kind
    raise AssertionError("unrecognised verifier message: %r" % msg)


def field_tag(F):
    return N.GB_GOLDILOCKS if F is GL else N.GB_BABYBEAR


def clone_challenger(ch):
    return ch.clone() if hasattr(ch, "clone") else copy.deepcopy(ch)


def challenger_tuple(ch, F):
    """(sponge_state, input_buffer, output_buffer) of the oracle's Challenger objects (iop/challenger.rs:18-31)"""
    if F is BB:
        return [int(x) for x in ch.state], list(ch.inp), list(ch.out)
    raw = ch.state()   # C struct {state[12], in[8], int nin, out[8], int nout} as u64 words
    nin, nout = int(raw[20]) & 0xFFFFFFFF, int(raw[29]) & 0xFFFFFFFF
    return [int(x) for x in raw[:12]], [int(x) for x in raw[12:12 + nin]], [int(x) for x in raw[21:21 + nout]]


def fri_params(degree_bits, rate_bits, cap_height, arity, pow_bits, nqr, hiding=False):
    return FriParams(FriConfig(rate_bits, cap_height, pow_bits, nqr), hiding, degree_bits, list(arity))


def instance_from_tuples(num_polys, blinding, batches):
    """batches: [(point, [(oracle_index, polynomial_index)])]"""
    return FriInstanceInfo([FriOracleInfo(n, b) for n, b in zip(num_polys, blinding)],
                           [FriBatchInfo(tuple(int(x) for x in pt), [FriPolynomialInfo(o, p) for o, p in polys]) for pt, polys in batches])


# ----------------------------------------------------------------------------- the seeded instances
GENERAL_NUM_POLYS = (1, 9, 37)
GENERAL_BLINDING = (False, True, False)


def _random_ext(F, rng):
    return tuple(int(x) for x in rng.integers(1, F.P, size=F.D, dtype=np.uint64))


def general_instance(F, degree_bits, seed, skip_oracle=None):
    """Three oracles of 1, 9 and 37 polynomials (the second one salted), five batches - two passes of the reduction kernel's four
    slots.  Lists: a whole range; every third column; a range in descending order; a seeded shuffle; one polynomial twice in one
    batch; polynomial (2, 5) in all five batches.  Points: random extension elements, a base-field element embedded in the
    extension, and g z of batch 0's z.  skip_oracle: an oracle that no batch names (its polynomials are dropped from the lists)."""
    rng = np.random.default_rng(seed)
    z0 = _random_ext(F, rng)
    g = F.two_adic_generator(degree_bits)
    every = (2, 5)
    batches = [
        (z0, [(0, 0)] + [(1, i) for i in range(9)] + [(2, i) for i in range(37)]),                 # whole ranges (every among them)
        (F.escale(z0, g), [(2, i) for i in range(0, 37, 3)] + [every]),                            # every third column
        (F.efrom(int(rng.integers(2, F.P, dtype=np.uint64))), [(2, i) for i in range(30, 3, -1)]),   # descending (every among them)
        (_random_ext(F, rng), [(o, int(i)) for o, i in
                               np.array([(1, i) for i in range(9)] + [(2, i) for i in range(37)])[rng.permutation(46)]]),   # a shuffle
        (_random_ext(F, rng), [(1, 4), (2, 8), (1, 4), every, (0, 0), (2, 9), (2, 10), (2, 8)]),   # (1, 4) and (2, 8) twice
    ]
    if skip_oracle is not None:
        batches = [(pt, [q for q in polys if q[0] != skip_oracle]) for pt, polys in batches]
        assert all(polys for _, polys in batches)
    else:
        assert all(every in polys for _, polys in batches)
    return instance_from_tuples(GENERAL_NUM_POLYS, GENERAL_BLINDING, batches)


def many_runs_instance(F, seed, ncols=40, npoints=8):
    """one oracle of `ncols` polynomials opened in shuffled order at `npoints` points: ncols * npoints runs of length one (unless
    the shuffle leaves neighbours in place), two passes"""
    rng = np.random.default_rng(seed)
    batches = [(_random_ext(F, rng), [(0, int(i)) for i in rng.permutation(ncols)]) for _ in range(npoints)]
    return instance_from_tuples((ncols,), (False,), batches)


def oracle_values(F, num_polys, degree_bits, seed, kind):
    """[num_polys][n] canonical values: a SplitMix64 stream, or the fields' carry-edge values in a seeded order"""
    n = 1 << degree_bits
    if kind == "random":
        return F.fill(seed, num_polys * n).reshape(num_polys, n)
    from wired_circuits import edge_values
    ev = np.array(edge_values(F), dtype=F.dtype)
    return ev[np.random.default_rng(seed).integers(0, len(ev), size=(num_polys, n))]


# ----------------------------------------------------------------------------- prove_openings on Python integers
def _reduce_polys_base(F, alpha, cols):
    """ReducingFactor::reduce_polys_base (util/reducing.rs:89-103): sum_j alpha^j cols[j], -> n extension elements"""
    n = len(cols[0])
    acc = [np.zeros(n, dtype=object) for _ in range(F.D)]
    a = F.one
    for col in cols:
        c = np.array([int(x) for x in col], dtype=object)
        for k in range(F.D):
            if a[k]:
                acc[k] = acc[k] + a[k] * c
        a = F.emul(a, alpha)
    return [tuple(int(acc[k][t]) % F.P for k in range(F.D)) for t in range(n)]


def _divide_by_linear(F, coeffs, z):
    """PolynomialCoeffs::divide_by_linear (polynomial/division.rs:75-88): the quotient of (f - f(z)) / (X - z), padded back to len(f)"""
    n = len(coeffs)
    q = [F.zero] * n
    run = F.zero
    for t in range(n - 1, 0, -1):
        run = F.eadd(coeffs[t], F.emul(z, run))
        q[t - 1] = run
    return q


def final_poly_ref(F, instance, oracle_coeffs, alpha, betas, arity_bits):
    """fri/oracle.rs:208-224 then the folds of fri/prover.rs:83-133 with the proof's betas -> FriProof.final_poly.
    oracle_coeffs[o]: [num_polys][n] canonical coefficients of oracle o."""
    final = None
    for batch in instance.batches:
        cols = [oracle_coeffs[p.oracle_index][p.polynomial_index] for p in batch.polynomials]
        comp = _reduce_polys_base(F, alpha, cols)
        quotient = _divide_by_linear(F, comp, tuple(batch.point))
        if final is None:
            final = quotient                                     # alpha.shift_poly of the empty polynomial
        else:
            sh = F.epow(alpha, len(cols))
            final = [F.eadd(F.emul(f, sh), q) for f, q in zip(final, quotient)]
    for ab, beta in zip(arity_bits, betas):
        arity = 1 << ab
        pw = [F.one]
        for _ in range(arity - 1):
            pw.append(F.emul(pw[-1], beta))
        folded = []
        for i in range(0, len(final), arity):                    # reduce_with_powers(chunk, beta)
            acc = F.zero
            for k in range(arity):
                acc = F.eadd(acc, F.emul(final[i + k], pw[k]))
            folded.append(acc)
        final = folded
    return final


# ----------------------------------------------------------------------------- FriProof bytes
def read_fri_proof(F, data, instance, params):
    """util/serialization/mod.rs:1679-1695 read side -> the dict oracle.verifier uses for opening_proof"""
    r = V.Reader(data, F)
    cap_h, arity = params.config.cap_height, params.reduction_arity_bits
    fri = dict(commit_phase_merkle_caps=[r.cap(cap_h) for _ in arity], query_round_proofs=[])
    widths = [o.num_polys + (V.SALT_SIZE if params.hiding and o.blinding else 0) for o in instance.oracles]
    for _ in range(params.config.num_query_rounds):
        initial = [(r.field_vec(w), r.merkle_proof()) for w in widths]
        steps = [(r.ext_vec(1 << ab), r.merkle_proof()) for ab in arity]
        fri["query_round_proofs"].append(dict(initial_trees_proof=initial, steps=steps))
    fri["final_poly"] = r.ext_vec(1 << (params.degree_bits - sum(arity)))
    fri["pow_witness"] = r.field()
    assert r.done(), "trailing bytes in proof"
    return fri


def write_fri_proof(F, fri):
    out = bytearray()
    fmt = "<Q" if F.elem_bytes == 8 else "<I"

    def fv(xs):
        for x in xs:
            out.extend(struct.pack(fmt, int(x)))

    for c in fri["commit_phase_merkle_caps"]:
        for h in c:
            fv(h)
    for q in fri["query_round_proofs"]:
        for vals, path in q["initial_trees_proof"]:
            fv(vals)
            out.append(len(path))
            for h in path:
                fv(h)
        for evals, path in q["steps"]:
            for e in evals:
                fv(e)
            out.append(len(path))
            for h in path:
                fv(h)
    for e in fri["final_poly"]:
        fv(e)
    fv([fri["pow_witness"]])
    return bytes(out)


def fri_challenges(F, ch, fri, params):
    """fri/challenges.rs:24-68 on `ch`, the transcript after the openings were observed (advanced).  Also returns the challenger
    as it stood in front of the proof-of-work witness."""
    alpha = ch.get_extension_challenge(F.D)
    betas = []
    for cap in fri["commit_phase_merkle_caps"]:
        ch.observe_cap(cap)
        betas.append(ch.get_extension_challenge(F.D))
    ch.observe_elements([x for e in fri["final_poly"] for x in e])
    before_pow = clone_challenger(ch)
    ch.observe_element(fri["pow_witness"])
    resp = ch.get_challenge()
    lde = 1 << (params.degree_bits + params.config.rate_bits)
    idx = [ch.get_challenge() % lde for _ in range(params.config.num_query_rounds)]
    return dict(fri_alpha=alpha, fri_betas=betas, fri_pow_response=resp, fri_query_indices=idx), before_pow


def verify_fri_instance(F, instance, openings, initial_caps, ch, proof, params):
    """verify_fri_proof (fri/verifier.rs:67-250) = oracle.verifier.verify_fri with the instance passed in.  openings: per batch a
    list of extension elements; initial_caps: per oracle a list of digests; ch: the oracle's Challenger after the openings were
    observed (it is advanced); proof: FriProof bytes or the dict of read_fri_proof.  Raises FriReject(kind), kind in KINDS."""
    fri = proof if isinstance(proof, dict) else read_fri_proof(F, proof, instance, params)
    P_ = F.P
    chal, _ = fri_challenges(F, ch, fri, params)
    log_n = params.degree_bits + params.config.rate_bits
    if not V.pow_ok(chal["fri_pow_response"], params.config.proof_of_work_bits, F):
        raise FriReject("pow")
    alpha = chal["fri_alpha"]
    reduced_openings = [V.reduce_with_alpha(alpha, [tuple(int(x) for x in e) for e in b], F)[0] for b in openings]
    for x_index, rp in zip(chal["fri_query_indices"], fri["query_round_proofs"]):
        for o, ((vals, path), cap) in enumerate(zip(rp["initial_trees_proof"], initial_caps)):
            if not F.merkle_verify(vals, x_index, cap, path):
                raise FriReject("merkle", "initial tree %d" % o)
        subgroup_x = F.generator * pow(F.two_adic_generator(log_n), V.reverse_bits(x_index, log_n), P_) % P_
        total = F.zero   # fri_combine_initial (fri/verifier.rs:121-165)
        for batch, red_open in zip(instance.batches, reduced_openings):
            evs = []
            for p in batch.polynomials:
                vals = rp["initial_trees_proof"][p.oracle_index][0]
                salted = params.hiding and instance.oracles[p.oracle_index].blinding
                unsalted = vals[: len(vals) - (V.SALT_SIZE if salted else 0)]
                evs.append(F.efrom(unsalted[p.polynomial_index]))
            red, count = V.reduce_with_alpha(alpha, evs, F)
            total = F.emul(F.epow(alpha, count), total)
            total = F.eadd(total, F.ediv(F.esub(red, red_open), F.esub(F.efrom(subgroup_x), tuple(batch.point))))
        old_eval = total
        xi = x_index
        for i, ab in enumerate(params.reduction_arity_bits):
            evals, path = rp["steps"][i]
            coset_index, within = xi >> ab, xi & ((1 << ab) - 1)
            if tuple(evals[within]) != tuple(old_eval):
                raise FriReject("consistency", "layer %d" % i)
            old_eval = V.compute_evaluation(subgroup_x, within, ab, evals, chal["fri_betas"][i], F)
            flat = [x for e in evals for x in e]
            if not F.merkle_verify(flat, coset_index, fri["commit_phase_merkle_caps"][i], path):
                raise FriReject("merkle", "layer %d" % i)
            subgroup_x = pow(subgroup_x, 1 << ab, P_)
            xi = coset_index
        acc = F.zero
        for cf in reversed(fri["final_poly"]):
            acc = F.eadd(F.emul(acc, F.efrom(subgroup_x)), cf)
        if tuple(acc) != tuple(old_eval):
            raise FriReject("final")
    return True


def plonk_instance(cd, zeta, F=GL):
    """oracle.verifier.fri_instance(cd, zeta) as a FriInstanceInfo"""
    blinding, batches = V.fri_instance(cd, zeta, F)
    cfg = cd["config"]
    c = cfg["num_challenges"]
    num_polys = [cd["num_constants"] + cfg["num_routed_wires"], cfg["num_wires"], c * (1 + cd["num_partial_products"]),
                 c * cd["quotient_degree_factor"]]
    return instance_from_tuples(num_polys, blinding, batches)
