"""gb_verify_batch / gb_verify_check_text without a device (include/goldibear_gpu.h): what the entry points answer before they touch
one, the check codes and their texts, and the binding's struct.  The cases that need a context are in tests/test_gpu_verify_batch.py."""
import ctypes as C
import os
import re

import numpy as np

from plonky2_goldibear_amd import VerifyResult, native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "goldibear_gpu.h")).read()


def test_a_null_context_is_refused_before_anything_else():
    lib = N.load()
    raw = np.zeros(16, dtype=np.uint8)
    ptrs, lens, res = (C.c_void_p * 1)(raw.ctypes.data), (C.c_size_t * 1)(16), (N.gb_verify_result * 1)()
    assert lib.gb_verify_batch(None, None, ptrs, lens, 1, 0, C.cast(res, C.c_void_p)) == N.GB_ERR_INVALID
    assert b"null ctx" in lib.gb_last_error(None)
    assert lib.gb_verify_batch(None, None, None, None, 0, 0, None) == N.GB_ERR_INVALID   # also for an empty batch
    assert lib.gb_verify_batch(None, None, ptrs, lens, 1, 7, C.cast(res, C.c_void_p)) == N.GB_ERR_INVALID


def test_check_codes_and_texts_match_the_header():
    lib = N.load()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    codes = {k: int(v) for k, v in re.findall(r"#define\s+(GB_VCHECK_[A-Z_]+)\s+(\d+)", src)}
    assert len(codes) == 14 and sorted(codes.values()) == list(range(14))
    for name, value in codes.items():
        assert getattr(N, name) == value, name
        text = lib.gb_verify_check_text(value).decode()
        assert (text == "") == (name == "GB_VCHECK_NONE"), name
    assert lib.gb_verify_check_text(14) == b"" and lib.gb_verify_check_text(0xFFFFFFFF) == b""
    # the texts are the ones gb_verify leaves (csrc/verifier_host.inc throws them through the same table)
    assert "vanishing" in lib.gb_verify_check_text(N.GB_VCHECK_VANISHING).decode()
    assert "proof of work" in lib.gb_verify_check_text(N.GB_VCHECK_POW).decode()
    assert "wrong length" in lib.gb_verify_check_text(N.GB_VCHECK_INITIAL_PATH_LEN).decode()
    assert "truncated" in lib.gb_verify_check_text(N.GB_VCHECK_TRUNCATED).decode()


def test_the_result_struct_is_the_header_s():
    m = re.search(r"typedef struct gb_verify_result \{(.*?)\} gb_verify_result;", _header(), flags=re.S)
    fields = re.findall(r"uint32_t\s+(\w+);", m.group(1))
    assert fields == [n for n, _ in N.gb_verify_result._fields_] == ["status", "check", "query_round", "index"]
    assert C.sizeof(N.gb_verify_result) == 16
    r = VerifyResult(N.GB_ERR_VERIFY, N.GB_VCHECK_FINAL_POLY, "x", 3, 0xFFFFFFFF)
    assert not r.ok and not r and r.query_round == 3 and r.index is None
    assert VerifyResult(N.GB_OK, 0, "", 0xFFFFFFFF, 0xFFFFFFFF).ok


def test_gb_verify_answers_through_the_shared_table(golden_dir):
    """gb_verify's own statuses and texts on the reference's proof - the host walk now runs the checks of csrc/verify_query.hpp"""
    from oracle import verifier as V
    from test_abi_verify_fixture import _fixture_circuit
    lib = N.load()
    circ, cd, raw = _fixture_circuit(golden_dir)
    proof, pis = V.read_proof_with_pis(raw, cd)

    def verdict(b):
        buf = np.frombuffer(b, dtype=np.uint8)
        st = lib.gb_verify(circ.handle, buf.ctypes.data, len(b))
        return st, lib.gb_last_error(None).decode() if st else ""

    assert verdict(raw) == (N.GB_OK, "")
    q = proof["opening_proof"]["query_round_proofs"]
    evals, path = q[7]["steps"][1]
    for k in range(len(evals)):   # every element of one coset in turn: the consistency check for one of them, the layer's path for the rest
        p2 = dict(proof, opening_proof=dict(proof["opening_proof"], query_round_proofs=list(q)))
        ev = list(evals)
        ev[k] = ((ev[k][0] + 1) % V.P, ev[k][1])
        p2["opening_proof"]["query_round_proofs"][7] = dict(q[7], steps=[q[7]["steps"][0], (ev, path)] + q[7]["steps"][2:])
        st, text = verdict(V.write_proof_with_pis(p2, pis))
        assert st == N.GB_ERR_VERIFY and text in (lib.gb_verify_check_text(N.GB_VCHECK_CONSISTENCY).decode(),
                                                  lib.gb_verify_check_text(N.GB_VCHECK_LAYER_PATH).decode())
    circ.free()
