"""gb_fri_verify_batch's host stage without a device (a NULL context: the call answers GB_ERR_INVALID, and `results` holds what the
host stage decided), on the reference's own recursion proof (recursion/regression_test_data.rs) described as a general instance
the way tests/test_fri_instances.py does.  Every item the host decides has gb_fri_verify's status and text; the untouched proof is
left to the device: GB_ERR_INVALID with check 0."""
import copy
import os
import struct

import numpy as np
import pytest

import fri_batch_helpers as H
import fri_instances as FI
from oracle import verifier as V
from oracle.fields import GL
from plonky2_goldibear_amd import native as N

GLF = N.GB_GOLDILOCKS


@pytest.fixture(scope="module")
def reference(golden_dir):
    rd = lambda n: open(os.path.join(golden_dir, n), "rb").read()
    cd = V.read_common_data(rd("recursive_verifier_gl_common_data.bin"))
    vd = V.read_verifier_data(rd("recursive_verifier_gl_verifier_data.bin"))
    pr, pis = V.read_proof_with_pis(rd("recursive_verifier_gl_proof.bin"), cd)
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
    inst = FI.plonk_instance(cd, zeta)
    fri = pr["opening_proof"]
    item = H.Item(GLF, inst, openings, FI.challenger_tuple(ch, GL), caps, FI.write_fri_proof(GL, fri))
    return dict(instance=inst, params=params, fri=fri, item=item)


def test_the_host_stage_decides_what_gb_fri_verify_decides(reference):
    ref = reference
    inst, params, good = ref["instance"], ref["params"], ref["item"]
    proof = good.proof
    p_word = struct.pack("<Q", GL.P)
    short = copy.deepcopy(ref["fri"])                 # round 3, oracle 2: the path without its last sibling, the length byte one less
    vals, path = short["query_round_proofs"][3]["initial_trees_proof"][2]
    short["query_round_proofs"][3]["initial_trees_proof"][2] = (vals, path[:-1])
    short = FI.write_fri_proof(GL, short)
    assert len(short) == len(proof) - 32
    nonce = copy.deepcopy(ref["fri"])
    nonce["pow_witness"] = (nonce["pow_witness"] + 1) % GL.P
    items = [
        ("good", good, None),
        ("truncated", good.copy(proof=proof[:-9]), (N.GB_ERR_INVALID, N.GB_VCHECK_TRUNCATED, H.NONE, H.NONE)),
        ("trailing", good.copy(proof=proof + b"\0"), (N.GB_ERR_INVALID, N.GB_VCHECK_TRAILING, H.NONE, H.NONE)),
        ("word = p", good.copy(proof=proof[:64] + p_word + proof[72:]), (N.GB_ERR_INVALID, N.GB_VCHECK_NON_CANONICAL, H.NONE, H.NONE)),
        ("path length", good.copy(proof=short), (N.GB_ERR_INVALID, N.GB_VCHECK_INITIAL_PATH_LEN, 3, 2)),
        ("nonce", good.copy(proof=FI.write_fri_proof(GL, nonce)), (N.GB_ERR_VERIFY, N.GB_VCHECK_POW, H.NONE, H.NONE)),
        ("good again", good.copy(), None),
    ]
    bad_open = good.copy()
    bad_open.openings[5, 1] = GL.P
    items.append(("opening = p", bad_open, (N.GB_ERR_INVALID, N.GB_VCHECK_NON_CANONICAL, H.NONE, H.NONE)))
    bad_cap = good.copy()
    bad_cap.caps[1, 0, 0] = GL.P + 1
    items.append(("cap word > p", bad_cap, (N.GB_ERR_INVALID, N.GB_VCHECK_NON_CANONICAL, H.NONE, H.NONE)))
    st, res = H.raw_batch(None, GLF, inst, params, [it for _, it, _ in items])
    assert st == N.GB_ERR_INVALID and H.last_error() == "null ctx"
    for (name, it, want), got in zip(items, res):
        alone = H.single(None, GLF, inst, params, it)
        if want is None:   # only a device could decide: gb_fri_verify accepts it, the host stage found nothing
            assert alone[0] == N.GB_OK, name
            assert got == (N.GB_ERR_INVALID, N.GB_VCHECK_NONE, H.NONE, H.NONE), name
            continue
        assert got == want, "%s: %r" % (name, got)
        assert got[0] == alone[0], "%s: gb_fri_verify answers %r" % (name, alone)
        if name not in ("opening = p", "cap word > p"):   # (gb_fri_verify names the argument there; the check has one text)
            assert H.check_text(got[1]) == alone[1], name


def test_a_challenger_the_library_cannot_read(reference):
    """gb_fri_verify refuses a proof with fewer bytes than query rounds first, then a challenger state with a word >= p; the item
    gets the same status in the same order.  The second refusal has no GB_VCHECK code: check 0 with GB_ERR_INVALID, which without
    a context is also the answer for an item left to the device - with one, that item gets the device's verdict."""
    ref = reference
    inst, params, good = ref["instance"], ref["params"], ref["item"]
    state, inp, outb = good.challenger
    bad = good.copy(challenger=([GL.P] + list(state[1:]), inp, outb))
    short = bad.copy(proof=good.proof[:params.config.num_query_rounds - 1])
    st, res = H.raw_batch(None, GLF, inst, params, [bad, short, good.copy(proof=good.proof[:5])])
    assert st == N.GB_ERR_INVALID
    assert res == [(N.GB_ERR_INVALID, N.GB_VCHECK_NONE, H.NONE, H.NONE)] + [(N.GB_ERR_INVALID, N.GB_VCHECK_TRUNCATED, H.NONE, H.NONE)] * 2
    alone = [H.single(None, GLF, inst, params, it) for it in (bad, short)]
    assert alone[0][0] == N.GB_ERR_INVALID and "challenger" in alone[0][1]
    assert alone[1][0] == N.GB_ERR_INVALID and alone[1][1].startswith(H.check_text(N.GB_VCHECK_TRUNCATED))
