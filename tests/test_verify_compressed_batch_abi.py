"""gb_verify_compressed_batch without a device (include/goldibear_gpu.h): what the entry point answers before it touches one, the
check codes only a compressed proof can fail on and their texts, and the binding's result.  The cases that need a context are in
tests/test_gpu_verify_compressed_batch.py."""
import ctypes as C
import re

import numpy as np

from plonky2_goldibear_amd import VerifyResult, native as N

from test_verify_batch_abi import _header


def test_a_null_context_is_refused_before_anything_else():
    lib = N.load()
    raw = np.zeros(16, dtype=np.uint8)
    ptrs, lens, res = (C.c_void_p * 1)(raw.ctypes.data), (C.c_size_t * 1)(16), (N.gb_verify_result * 1)()
    assert lib.gb_verify_compressed_batch(None, None, ptrs, lens, 1, 0, C.cast(res, C.c_void_p)) == N.GB_ERR_INVALID
    assert b"null ctx" in lib.gb_last_error(None)
    assert lib.gb_verify_compressed_batch(None, None, None, None, 0, 0, None) == N.GB_ERR_INVALID   # also for an empty batch
    assert lib.gb_verify_compressed_batch(None, None, ptrs, lens, 1, 7, C.cast(res, C.c_void_p)) == N.GB_ERR_INVALID


def test_a_verifier_object_without_a_context_still_needs_the_caller_s(golden_dir):
    from test_abi_verify_fixture import _fixture_circuit
    lib = N.load()
    circ, cd, raw = _fixture_circuit(golden_dir)
    small = np.frombuffer(circ.compress(raw), dtype=np.uint8)
    ptrs, lens, res = (C.c_void_p * 1)(small.ctypes.data), (C.c_size_t * 1)(small.size), (N.gb_verify_result * 1)()
    assert lib.gb_verify_compressed_batch(None, circ.handle, ptrs, lens, 1, 0, C.cast(res, C.c_void_p)) == N.GB_ERR_INVALID
    assert b"null ctx" in lib.gb_last_error(None)
    circ.free()


def test_the_new_check_codes_and_their_texts(golden_dir):
    lib = N.load()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    codes = {k: int(v) for k, v in re.findall(r"(GB_VCHECK_COMPRESSED_[A-Z_]+)\s*=\s*(\d+)", src)}
    assert sorted(codes.values()) == [16, 17, 18]
    for name, value in codes.items():
        assert getattr(N, name) == value, name
        assert lib.gb_verify_check_text(value) != b"", name
    assert lib.gb_verify_check_text(14) == b"" and lib.gb_verify_check_text(15) == b"" and lib.gb_verify_check_text(19) == b""
    # the texts are the ones gb_verify_compressed leaves, byte for byte
    text = lambda c: lib.gb_verify_check_text(c).decode()
    assert text(N.GB_VCHECK_COMPRESSED_INDICES) == "the compressed proof's query indices are not the transcript's"
    assert text(N.GB_VCHECK_COMPRESSED_MISSING_SIBLING) == "compressed Merkle proof is missing a sibling"
    assert text(N.GB_VCHECK_COMPRESSED_TRAILING) == "trailing bytes in compressed proof" != text(N.GB_VCHECK_TRAILING)


def test_gb_verify_compressed_answers_through_the_shared_table(golden_dir):
    """gb_verify_compressed on the reference's proof, compressed: its statuses and texts for what only this form can fail on"""
    from oracle import compression as Z
    from test_abi_verify_fixture import _fixture_circuit
    lib = N.load()
    circ, cd, raw = _fixture_circuit(golden_dir)
    small = circ.compress(raw)
    cpr, pis = Z.read_compressed_proof_with_pis(small, cd)

    def verdict(b):
        buf = np.frombuffer(bytes(b) or b"\0", dtype=np.uint8)
        st = lib.gb_verify_compressed(circ.handle, buf.ctypes.data, len(b))
        return st, lib.gb_last_error(None).decode() if st else ""

    text = lambda c: lib.gb_verify_check_text(c).decode()
    assert verdict(small) == (N.GB_OK, "")
    assert verdict(small + b"\0") == (N.GB_ERR_INVALID, text(N.GB_VCHECK_COMPRESSED_TRAILING))
    assert verdict(small + bytes(8)) == (N.GB_ERR_INVALID, text(N.GB_VCHECK_PI_COUNT))
    assert verdict(small[:-9]) == (N.GB_ERR_INVALID, text(N.GB_VCHECK_TRUNCATED))
    fri = cpr["opening_proof"]
    idx = fri["indices"]
    other = next(k for k, i in enumerate(idx) if i != idx[0])
    swapped = dict(cpr, opening_proof=dict(fri, indices=[idx[other]] + idx[1:other] + [idx[0]] + idx[other + 1:]))
    assert verdict(Z.write_compressed_proof_with_pis(swapped, pis)) == (N.GB_ERR_VERIFY, text(N.GB_VCHECK_COMPRESSED_INDICES))
    key = next(k for k, e in fri["initial_trees_proofs"].items() if e[3][1])
    entry = list(fri["initial_trees_proofs"][key])
    entry[3] = (entry[3][0], entry[3][1][:-1])
    short = dict(cpr, opening_proof=dict(fri, initial_trees_proofs=dict(fri["initial_trees_proofs"], **{})))
    short["opening_proof"]["initial_trees_proofs"][key] = entry
    assert verdict(Z.write_compressed_proof_with_pis(short, pis)) == (N.GB_ERR_INVALID, text(N.GB_VCHECK_COMPRESSED_MISSING_SIBLING))
    entry[3] = (entry[3][0], list(fri["initial_trees_proofs"][key][3][1]) + [[5, 5, 5, 5]])   # a surplus sibling is ignored
    assert verdict(Z.write_compressed_proof_with_pis(short, pis)) == (N.GB_OK, "")
    circ.free()


def test_the_result_mapping():
    r = VerifyResult(N.GB_ERR_INVALID, N.GB_VCHECK_COMPRESSED_MISSING_SIBLING, "x", 0xFFFFFFFF, 0xFFFFFFFF)
    assert not r.ok and r.query_round is None and r.index is None and r.check == 17
    assert callable(N.verify_compressed_batch)
    from plonky2_goldibear_amd.circuit_builder import BuiltCircuit
    from plonky2_goldibear_amd.prover import CircuitData, VerifierCircuitData
    for cls in (CircuitData, VerifierCircuitData, BuiltCircuit):
        assert callable(getattr(cls, "verify_compressed_batch")), cls
