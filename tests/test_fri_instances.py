"""verify_fri_proof on any FriInstanceInfo, without a GPU: the yardstick of the opening tests (tests/fri_instances.py
verify_fri_instance) and the library's gb_fri_verify, both on the reference's OWN serialized recursion proof
(recursion/regression_test_data.rs) described as a general instance - fri_instance(cd, zeta) written out as oracles and batches."""
import copy

import numpy as np
import pytest

import fri_instances as FI
from oracle import verifier as V
from oracle.fields import GL
from plonky2_goldibear_amd import ShapeError, VerifyError, verify_fri_proof
from plonky2_goldibear_amd.fri import FriPolynomialInfo


@pytest.fixture(scope="module")
def reference_proof(golden_dir):
    import os
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    raw = rd("recursive_verifier_gl_proof.bin")
    pr, pis = V.read_proof_with_pis(raw, cd)
    cfg, fc, fp = cd["config"], cd["config"]["fri_config"], cd["fri_params"]
    c = cfg["num_challenges"]
    ch = GL.Challenger()                     # plonk/get_challenges.rs:26-60, up to and including observe_openings
    ch.observe_hash(vd["circuit_digest"])
    ch.observe_hash(GL.hash_no_pad(np.asarray(pis, dtype=np.uint64)))
    ch.observe_cap(pr["wires_cap"]); ch.get_n_challenges(2 * c)
    ch.observe_cap(pr["zs_cap"]); ch.get_n_challenges(c)
    ch.observe_cap(pr["quotient_cap"])
    zeta = ch.get_extension_challenge(2)
    openings = V.fri_openings(pr["openings"])
    for batch in openings:
        ch.observe_elements([x for e in batch for x in e])
    params = FI.fri_params(fp["degree_bits"], fc["rate_bits"], fc["cap_height"], fp["reduction_arity_bits"], fc["proof_of_work_bits"],
                           fc["num_query_rounds"], hiding=fp["hiding"])
    caps = [vd["constants_sigmas_cap"], pr["wires_cap"], pr["zs_cap"], pr["quotient_cap"]]
    fri = pr["opening_proof"]
    fri_bytes = FI.write_fri_proof(GL, fri)
    assert fri_bytes in raw and FI.read_fri_proof(GL, fri_bytes, FI.plonk_instance(cd, zeta), params) == fri
    return dict(instance=FI.plonk_instance(cd, zeta), openings=openings, caps=caps, challenger=ch, fri=fri, params=params)


def _bump(x):
    return (int(x) + 1) % GL.P


def _mutations(ref):
    """one word changed in: an opening, an initial leaf, a sibling, a layer evaluation, the final polynomial, the nonce
    -> (name, openings, fri dict)"""
    out = []
    op = copy.deepcopy(ref["openings"])
    op[0][17] = (_bump(op[0][17][0]), op[0][17][1])
    out.append(("opening", op, ref["fri"]))

    def changed(edit):
        fri = copy.deepcopy(ref["fri"])
        edit(fri)
        return fri

    def leaf(fri):
        fri["query_round_proofs"][2]["initial_trees_proof"][1][0][3] = _bump(fri["query_round_proofs"][2]["initial_trees_proof"][1][0][3])

    def sibling(fri):
        fri["query_round_proofs"][1]["initial_trees_proof"][2][1][0][1] = _bump(fri["query_round_proofs"][1]["initial_trees_proof"][2][1][0][1])

    def layer_eval(fri):
        evals = fri["query_round_proofs"][0]["steps"][1][0]
        evals[5] = (evals[5][0], _bump(evals[5][1]))

    def final(fri):
        fri["final_poly"][3] = (_bump(fri["final_poly"][3][0]), fri["final_poly"][3][1])

    def nonce(fri):
        fri["pow_witness"] = _bump(fri["pow_witness"])

    for name, edit in (("initial leaf", leaf), ("sibling", sibling), ("layer evaluation", layer_eval), ("final polynomial", final),
                       ("nonce", nonce)):
        out.append((name, ref["openings"], changed(edit)))
    return out


def test_the_yardstick_is_pinned_by_the_reference(reference_proof):
    ref = reference_proof
    check = lambda op, fri: FI.verify_fri_instance(GL, ref["instance"], op, ref["caps"], FI.clone_challenger(ref["challenger"]), fri, ref["params"])
    assert check(ref["openings"], ref["fri"])
    for name, op, fri in _mutations(ref):
        with pytest.raises(FI.FriReject):
            check(op, fri)
            pytest.fail("accepted the proof with a changed " + name)


def _gb_fri_verify(ref, op, fri_bytes, instance=None):
    return verify_fri_proof(instance or ref["instance"], [np.array(b, dtype=np.uint64) for b in op], FI.challenger_tuple(ref["challenger"], GL),
                            [np.array(c, dtype=np.uint64) for c in ref["caps"]], fri_bytes, ref["params"])   # ctx = None: no device


def test_gb_fri_verify_on_the_reference_proof(reference_proof):
    ref = reference_proof
    assert _gb_fri_verify(ref, ref["openings"], FI.write_fri_proof(GL, ref["fri"]))
    for name, op, fri in _mutations(ref):
        with pytest.raises(VerifyError):
            _gb_fri_verify(ref, op, FI.write_fri_proof(GL, fri))
            pytest.fail("accepted the proof with a changed " + name)
    # by value: the caller's transcript is where it was, and the same call gives the same answer
    assert _gb_fri_verify(ref, ref["openings"], FI.write_fri_proof(GL, ref["fri"]))


def test_gb_fri_verify_argument_errors_are_not_verdicts(reference_proof):
    ref = reference_proof
    good = FI.write_fri_proof(GL, ref["fri"])
    for bad in (good[:-9], good[:100], b"", good + b"\0"):
        with pytest.raises(ShapeError):
            _gb_fri_verify(ref, ref["openings"], bad)
    for nqr, needle in ((0, "num_query_rounds is zero"), (4097, "GB_MAX_FRI_QUERY_ROUNDS"), (len(good) + 1 if len(good) < 4096 else 4096, "truncated")):
        params = copy.deepcopy(ref["params"])
        params.config.num_query_rounds = nqr
        with pytest.raises(ShapeError, match=needle):
            verify_fri_proof(ref["instance"], [np.array(b, dtype=np.uint64) for b in ref["openings"]], FI.challenger_tuple(ref["challenger"], GL),
                             [np.array(c, dtype=np.uint64) for c in ref["caps"]], good, params)
    inst = copy.deepcopy(ref["instance"])
    inst.batches[1].polynomials[0] = FriPolynomialInfo(2, inst.oracles[2].num_polys)          # one past the last polynomial
    with pytest.raises(ShapeError, match="polynomial_index"):
        _gb_fri_verify(ref, ref["openings"], good, inst)
    inst.batches[1].polynomials[0] = FriPolynomialInfo(4, 0)
    with pytest.raises(ShapeError, match="oracle_index"):
        _gb_fri_verify(ref, ref["openings"], good, inst)
