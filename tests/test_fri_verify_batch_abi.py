"""gb_fri_verify_batch: the arguments (no GPU).  An error of the shared shape is no verdict - it fails the call with gb_fri_verify's
status and message and leaves `results` alone; a NULL context, a flag, a NULL table or entry are GB_ERR_INVALID; the Python door
refuses items whose instances differ in more than their points."""
import copy

import pytest

import fri_batch_helpers as H
import fri_instances as FI
from plonky2_goldibear_amd import ShapeError, native as N, verify_fri_proofs
from plonky2_goldibear_amd.fri import FriPolynomialInfo

GLF = N.GB_GOLDILOCKS
UNTOUCHED = (0xAAAA, 0xAAAA)


def _good():
    inst = FI.instance_from_tuples((3,), (False,), [((1, 2), [(0, 0), (0, 1)])])
    params = FI.fri_params(3, 1, 0, [1], 0, 2)
    item = H.Item(GLF, inst, [[(5, 6), (7, 8)]], ([0] * 12, [], []), [[[1, 2, 3, 4]]], b"\x01" * 50)
    return inst, params, item


def test_a_null_context_is_invalid_and_still_answers():
    inst, params, item = _good()
    st, res = H.raw_batch(None, GLF, inst, params, [item, item])
    assert st == N.GB_ERR_INVALID and H.last_error() == "null ctx"
    # the host stage ran: 50 bytes of 0x01 are a truncated proof
    assert res == [(N.GB_ERR_INVALID, N.GB_VCHECK_TRUNCATED, H.NONE, H.NONE)] * 2


def test_flags_must_be_zero():
    inst, params, item = _good()
    st, res = H.raw_batch(None, GLF, inst, params, [item], flags=1)
    assert st == N.GB_ERR_INVALID and "flags must be 0" in H.last_error()
    assert [r[:2] for r in res] == [UNTOUCHED]


@pytest.mark.parametrize("table", ["points", "openings", "caps", "challengers", "proofs", "lens", "results"])
def test_a_null_table_is_invalid(table):
    inst, params, item = _good()
    st, res = H.raw_batch(None, GLF, inst, params, [item], null_tables=(table,))
    assert st == N.GB_ERR_INVALID and H.last_error() == "null argument"
    assert [r[:2] for r in res] == [UNTOUCHED]


@pytest.mark.parametrize("table", ["points", "openings", "caps", "proofs"])
def test_a_null_entry_is_invalid(table):
    inst, params, item = _good()
    st, res = H.raw_batch(None, GLF, inst, params, [item, item, item], null_entries=((table, 1),))
    assert st == N.GB_ERR_INVALID and "null entry for item 1" in H.last_error()
    assert [r[:2] for r in res] == [UNTOUCHED] * 3


def test_no_items_need_no_tables():
    inst, params, item = _good()
    st, _ = H.raw_batch(None, GLF, inst, params, [item], num_items=0, null_tables=("points", "openings", "caps", "challengers", "proofs", "lens", "results"))
    assert st == N.GB_ERR_INVALID and H.last_error() == "null ctx"   # (with a context: GB_OK - tests/test_gpu_fri_verify_batch.py)
    # the shape is still checked
    bad = copy.deepcopy(params)
    bad.config.num_query_rounds = 0
    st, _ = H.raw_batch(None, GLF, inst, bad, [item], num_items=0)
    assert st == N.GB_ERR_INVALID and "num_query_rounds is zero" in H.last_error()


def _shape_errors():
    inst, params, _ = _good()

    def with_params(**kw):
        p = copy.deepcopy(params)
        for k, v in kw.items():
            if k in ("degree_bits", "reduction_arity_bits"):
                setattr(p, k, v)
            else:
                setattr(p.config, k, v)
        return inst, p

    def with_poly(o, k):
        i2 = copy.deepcopy(inst)
        i2.batches[0].polynomials[1] = FriPolynomialInfo(o, k)
        return i2, params

    return {
        "no oracle": (FI.instance_from_tuples((), (), [((1, 2), [(0, 0)])]), params),
        "no batch": (FI.instance_from_tuples((3,), (False,), []), params),
        "empty batch": (FI.instance_from_tuples((3,), (False,), [((1, 2), [(0, 0)]), ((3, 4), [])]), params),
        "oracle index": with_poly(1, 0),
        "polynomial index": with_poly(0, 3),
        "arity bits zero": with_params(reduction_arity_bits=[0]),
        "arity bits nine": with_params(degree_bits=12, reduction_arity_bits=[9]),
        "arities past the degree": with_params(reduction_arity_bits=[2, 2]),
        "layer below the cap": with_params(cap_height=4, reduction_arity_bits=[1]),
        "proof of work bits": with_params(proof_of_work_bits=32),
        "no query rounds": with_params(num_query_rounds=0),
        "too many query rounds": with_params(num_query_rounds=4097),
        "two-adicity": with_params(degree_bits=32),
        "cap height": with_params(cap_height=5, reduction_arity_bits=[]),
    }


@pytest.mark.parametrize("name", sorted(_shape_errors()))
def test_shape_errors_are_gb_fri_verifys(name):
    inst, params = _shape_errors()[name]
    _, _, item = _good()
    want = H.single(None, GLF, inst, params, item)
    assert want[0] == N.GB_ERR_INVALID and want[1], "gb_fri_verify accepts the shape: " + name
    st, res = H.raw_batch(None, GLF, inst, params, [item, item])
    assert (st, H.last_error()) == want
    assert [r[:2] for r in res] == [UNTOUCHED] * 2, "a shape error left verdicts behind"


def test_the_python_door_names_the_item_whose_instance_differs():
    inst, params, _ = _good()
    other = copy.deepcopy(inst)
    other.batches[0].polynomials[1] = FriPolynomialInfo(0, 2)
    moved = FI.instance_from_tuples((3,), (False,), [((9, 9), [(0, 0), (0, 1)])])   # other points alone: the same shape
    item = lambda i: (i, [[(5, 6), (7, 8)]], ([0] * 12, [], []), [[[1, 2, 3, 4]]], b"\x01" * 50)
    with pytest.raises(ShapeError, match="item 2"):
        verify_fri_proofs(None, [item(inst), item(moved), item(other), item(other)], params)
    with pytest.raises(ShapeError, match="null ctx"):   # the shapes agree: the call is made, and refuses the missing context
        verify_fri_proofs(None, [item(inst), item(moved)], params)
    assert verify_fri_proofs(None, [], params) == []
