"""ctypes binding of libgoldibear_gpu.so - exactly the symbols include/goldibear_gpu.h declares.

There is no fallback: if the HIP library is missing or fails to load this raises, so a GPU test
can never pass on a silent CPU path.
"""
import ctypes as C
import os

from . import build as _build

# Several contexts proving at once (one stream and one host thread each - recursion-sized proofs cannot fill the GPU alone) need
# a hardware queue each to overlap: the HIP runtime maps streams onto GPU_MAX_HW_QUEUES queues, 4 unless the environment says
# otherwise, and reads the variable when it initialises - so it is set here, before anything touches the GPU, unless the host has
# chosen a value (tools/bench_recursion_shape.py --inflight 6: 576 proofs/s on 4 queues, 831 on 8).  A C host sets it itself
# (INTEGRATION.md).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

GB_OK, GB_ERR_INVALID, GB_ERR_HIP, GB_ERR_OOM, GB_ERR_UNSUPPORTED = 0, 1, 2, 3, 4
GB_ERR_PERM_ARG_ZERO, GB_ERR_OPENING_IN_SUBGROUP, GB_ERR_BUFFER_TOO_SMALL, GB_ERR_VERIFY = 16, 17, 18, 19
GB_ERR_UNSATISFIED = 20   # gb_check_*, and gb_prove* under the option "check_witness": the witness does not satisfy the circuit
GB_VIOLATION_GATE, GB_VIOLATION_SELECTOR, GB_VIOLATION_COPY = 1, 2, 3
# gb_verify_result.check: the check gb_verify names (gb_verify_batch)
(GB_VCHECK_NONE, GB_VCHECK_TRUNCATED, GB_VCHECK_NON_CANONICAL, GB_VCHECK_PI_IMPLAUSIBLE, GB_VCHECK_PI_COUNT, GB_VCHECK_TRAILING,
 GB_VCHECK_VANISHING, GB_VCHECK_POW, GB_VCHECK_INITIAL_PATH_LEN, GB_VCHECK_INITIAL_PATH, GB_VCHECK_CONSISTENCY,
 GB_VCHECK_LAYER_PATH_LEN, GB_VCHECK_LAYER_PATH, GB_VCHECK_FINAL_POLY) = range(14)
# what a compressed proof alone can fail on (gb_verify_compressed_batch)
GB_VCHECK_COMPRESSED_INDICES, GB_VCHECK_COMPRESSED_MISSING_SIBLING, GB_VCHECK_COMPRESSED_TRAILING = 16, 17, 18
GB_GOLDILOCKS, GB_BABYBEAR = 0, 1
GB_INPUT_HOST, GB_INPUT_DEVICE = 0, 1
GB_INPUT_P3_REPR = 2   # host elements are the reference's field types as they lie in memory (p3 words), not canonical values
GB_SALTS_FROM_SEED = 4   # gb_prove_salted* / gb_prove_partition / gb_prove_inputs: `salts` is a host pointer to 32 seed bytes
GB_SALT_SIZE = 4
GB_SEED_SIZE = 32
GB_STREAM_SALTS, GB_STREAM_BLINDING = 1, 2   # nonce[0] of the library's own streams (gb_random_elements)

_vp, _u32, _u64, _sz, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int32
_pvp = C.POINTER(C.c_void_p)
_cols = C.POINTER(C.c_void_p)   # const void* const*: one pointer per separately allocated column

# name -> (restype, argtypes); kept in step with include/goldibear_gpu.h (tests/test_abi.py checks it)
SIGNATURES = {
    "gb_ctx_create": (_i32, [C.c_int, _pvp]),
    "gb_ctx_destroy": (_i32, [_vp]),
    "gb_last_error": (C.c_char_p, [_vp]),
    "gb_ctx_synchronize": (_i32, [_vp]),
    "gb_ctx_trim": (_i32, [_vp]),
    "gb_ctx_stream": (_i32, [_vp, _pvp]),
    "gb_ctx_set_profiling": (_i32, [_vp, _i32]),
    "gb_ctx_scope_ms": (_i32, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "gb_ctx_scope_reset": (_i32, [_vp]),
    "gb_ctx_set_option": (_i32, [_vp, C.c_char_p, C.c_int64]),
    "gb_host_alloc": (_i32, [_vp, _sz, _pvp]),
    "gb_host_free": (_i32, [_vp, _vp]),
    "gb_host_register": (_i32, [_vp, _vp, _sz]),
    "gb_host_unregister": (_i32, [_vp, _vp]),
    "gb_commit_values_cols": (_i32, [_vp, _u32, _cols, _sz, _u32, _u32, _u32, _vp, _u32, _pvp]),
    "gb_commit_coeffs_cols": (_i32, [_vp, _u32, _cols, _sz, _u32, _u32, _u32, _vp, _u32, _pvp]),
    "gb_commit_values": (_i32, [_vp, _u32, _vp, _sz, _u32, _u32, _u32, _vp, _u32, _pvp]),
    "gb_commit_coeffs": (_i32, [_vp, _u32, _vp, _sz, _u32, _u32, _u32, _vp, _u32, _pvp]),
    "gb_batch_free": (_i32, [_vp]),
    "gb_batch_info": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_sz), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gb_batch_cap": (_i32, [_vp, _vp]),
    "gb_batch_coeffs": (_i32, [_vp, _sz, _vp]),
    "gb_batch_lde_values": (_i32, [_vp, _u64, _u64, _vp]),
    "gb_batch_leaf": (_i32, [_vp, _u64, _vp, _vp, C.POINTER(_u32)]),
    "gb_batch_digests": (_i32, [_vp, _vp]),
    "gb_batch_leaves": (_i32, [_vp, _vp]),
    "gb_batch_device_ptrs": (_i32, [_vp, _pvp, _pvp, _pvp]),
    "gb_batch_eval_ext": (_i32, [_vp, _vp, _vp]),
    "gb_verify": (_i32, [_vp, _vp, _sz]),
    "gb_verify_batch": (_i32, [_vp, _vp, _cols, C.POINTER(_sz), _u32, _u32, _vp]),
    "gb_verify_check_text": (C.c_char_p, [_u32]),
    "gb_verify_compressed_batch": (_i32, [_vp, _vp, _cols, C.POINTER(_sz), _u32, _u32, _vp]),
    "gb_proof_compress": (_i32, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_proof_decompress": (_i32, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_verify_compressed": (_i32, [_vp, _vp, _sz]),
    "gb_verifier_create": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _pvp]),
    "gb_pow_grind": (_i32, [_vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "gb_permute": (_i32, [_vp, _u32, _vp, _vp, _u64]),
    "gb_random_elements": (_i32, [_vp, _u32, C.POINTER(C.c_uint8), C.POINTER(_u32), _u64, _u64, _u32, _vp]),
    "gb_circuit_create": (_i32, [_vp, _vp, _vp, _vp, _u32, _pvp]),
    "gb_circuit_create_gates": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _pvp]),
    "gb_circuit_create_cols": (_i32, [_vp, _vp, _cols, _vp, _u32, _pvp]),
    "gb_circuit_create_gates_cols": (_i32, [_vp, _vp, _vp, _u32, _cols, _vp, _u32, _pvp]),
    "gb_circuit_create_programs": (_i32, [_vp, _vp, _vp, _u32, C.POINTER(_u64), C.POINTER(_u32), _u32, _vp, _vp, _u32, _pvp]),
    "gb_circuit_create_programs_cols": (_i32, [_vp, _vp, _vp, _u32, C.POINTER(_u64), C.POINTER(_u32), _u32, _cols, _vp, _u32, _pvp]),
    "gb_verifier_create_programs": (_i32, [_vp, _vp, _vp, _u32, C.POINTER(_u64), C.POINTER(_u32), _u32, _vp, _vp, _vp, _pvp]),
    "gb_circuit_free": (_i32, [_vp]),
    "gb_circuit_verifier_data": (_i32, [_vp, _vp, _vp]),
    "gb_circuit_constants_sigmas_commitment": (_i32, [_vp, _pvp]),
    "gb_circuit_set_fri_reduction_arity_bits": (_i32, [_vp, C.POINTER(_u32), _u32]),
    "gb_circuit_fri_reduction_arity_bits": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "gb_zs_partial_products": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "gb_quotient_polys": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "gb_prove_openings": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    "gb_fri_prove_openings": (_i32, [_vp, _pvp, _u32, _vp, C.POINTER(_u32), _u32, C.POINTER(_u32), C.POINTER(_u32), _u32, _u32, _u32, _vp, _vp,
                                     _sz, C.POINTER(_sz)]),
    "gb_fri_verify": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), _u32, _vp, C.POINTER(_u32), _u32,
                             C.POINTER(_u32), _vp, _vp, C.POINTER(_u32), _u32, _u32, _u32, _vp, _vp, _sz]),
    "gb_fri_verify_batch": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), _u32, C.POINTER(_u32), _u32,
                                   C.POINTER(_u32), C.POINTER(_u32), _u32, _u32, _u32, _cols, _cols, _cols, _vp, _cols, C.POINTER(_sz), _u32,
                                   _u32, _vp]),
    "gb_fri_verify_batch_counts": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gb_constraint_quotient": (_i32, [_vp, _pvp, _u32, C.POINTER(_u64), C.POINTER(_u32), _u32, _vp, _u32, _vp, _u32, _u32, _u32, _vp]),
    "gb_constraint_eval": (_i32, [_vp, _u32, _u32, C.POINTER(_u64), C.POINTER(_u32), _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "gb_prove": (_i32, [_vp, _vp, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_retry": (_i32, [_vp, _vp, _u32, _u32, _u64, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_circuit_drop_retry": (_i32, [_vp]),
    "gb_prove_salted": (_i32, [_vp, _vp, _u32, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_cols": (_i32, [_vp, _cols, _u32, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_retry_cols": (_i32, [_vp, _cols, _u32, _u32, _u64, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_salted_cols": (_i32, [_vp, _cols, _u32, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz)]),
    "gb_zs_partial_products_cols": (_i32, [_vp, _cols, _u32, _vp, _vp, _vp]),
    "gb_circuit_set_partition": (_i32, [_vp, C.POINTER(_u64), _u64, C.POINTER(_u64), _sz]),
    "gb_prove_partition": (_i32, [_vp, _vp, _u32, _vp, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_partition_retry": (_i32, [_vp, _vp, _u32, _u32, _u64, _vp, _sz, C.POINTER(_sz)]),
    "gb_expand_partition": (_i32, [_vp, _vp, _u32, _vp]),
    "gb_circuit_set_generators": (_i32, [_vp, _vp, _u64, C.POINTER(_u64), _u64, C.POINTER(_u64), _u32]),
    "gb_circuit_set_generator_programs": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u32), _u32]),
    "gb_circuit_generators_info": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gb_circuit_generator_classes": (_i32, [_vp, C.POINTER(_u64), _u64]),
    "gb_generate_partition": (_i32, [_vp, _vp, _u32, _vp]),
    "gb_prove_inputs": (_i32, [_vp, _vp, _u32, _vp, _vp, _sz, C.POINTER(_sz)]),
    "gb_prove_inputs_retry": (_i32, [_vp, _vp, _u32, _u32, _u64, _vp, _sz, C.POINTER(_sz)]),
    "gb_check_witness": (_i32, [_vp, _vp, _u32, C.POINTER(_u64), _sz, _vp, _sz, _vp]),
    "gb_check_partition": (_i32, [_vp, _vp, _u32, _vp, _sz, _vp]),
    "gb_check_inputs": (_i32, [_vp, _vp, _u32, _vp, _sz, _vp]),
    "gb_circuit_decode_sigmas": (_i32, [_vp, _u32, _vp]),
    "gb_circuit_copy_classes": (_i32, [_vp, C.POINTER(_u32)]),
    "gb_wiring_sigmas": (_i32, [_vp, _u32, _u32, _u32, _u32, _vp, C.POINTER(_u64), _u64, _u64, _u32, _vp, C.POINTER(_u64), _vp]),
    "gb_fft": (_i32, [_vp, _u32, _vp, _vp, _sz, _u32, _u32, _u32, _vp, _u32]),
    "gb_ifft": (_i32, [_vp, _u32, _vp, _vp, _sz, _u32, _u32, _vp, _u32]),
    "gb_lde": (_i32, [_vp, _u32, _vp, _vp, _sz, _u32, _u32, _u32, _vp, _u32]),
    "gb_merkle_tree_create": (_i32, [_vp, _u32, _vp, _u32, _u32, _u32, _u32, _pvp]),
    "gb_merkle_tree_free": (_i32, [_vp]),
    "gb_merkle_tree_info": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gb_merkle_tree_cap": (_i32, [_vp, _vp]),
    "gb_merkle_tree_leaf": (_i32, [_vp, _u64, _vp, _vp, C.POINTER(_u32)]),
    "gb_merkle_tree_digests": (_i32, [_vp, _vp]),
}
# gb_generator.kind (include/goldibear_gpu.h GB_GEN_*)
(GB_GEN_ARITHMETIC, GB_GEN_ARITHMETIC_EXTENSION, GB_GEN_MUL_EXTENSION, GB_GEN_CONSTANT, GB_GEN_BASE_SPLIT, GB_GEN_REDUCING,
 GB_GEN_REDUCING_EXTENSION, GB_GEN_RANDOM_ACCESS, GB_GEN_POSEIDON_MDS, GB_GEN_COSET_INTERPOLATION, GB_GEN_EXPONENTIATION, GB_GEN_POSEIDON,
 GB_GEN_POSEIDON2_BABYBEAR, GB_GEN_ADD_MANY, GB_GEN_APPLY_MAT4, GB_GEN_POSEIDON2_INTERNAL, GB_GEN_COPY) = range(17)
# the gadget generators: a head record (kind, parameter, number of targets, 0) and GB_GEN_TARGETS continuation records
(GB_GEN_EQUALITY, GB_GEN_NONZERO_TEST, GB_GEN_QUOTIENT_OR_ZERO, GB_GEN_QUOTIENT_EXTENSION, GB_GEN_SPLIT, GB_GEN_WIRE_SPLIT,
 GB_GEN_LOW_HIGH, GB_GEN_BASE_SUM, GB_GEN_TARGETS) = range(32, 41)
# a generator program's head: (kind, program index, number of targets, the row of its constants), then GB_GEN_TARGETS records
GB_GEN_PROGRAM = 48


def gadget_records(kind, param, targets):
    """one gadget generator as gb_generator tuples: the head, then ceil(len(targets) / 2) continuation records of two targets"""
    targets = [int(t) for t in targets]
    padded = targets + [0] * (len(targets) & 1)
    return [(kind, int(param), len(targets), 0)] + [(GB_GEN_TARGETS, 0, padded[i], padded[i + 1]) for i in range(0, len(padded), 2)]
# include/goldibear_gpu_test_hooks.h: exports for the test suite, outside the product ABI
TEST_HOOK_SIGNATURES = {
    "gb_test_arm_perm_arg_failure": (_i32, [_vp]),
    "gb_test_force_gate_fallback": (_i32, [_vp, C.c_int]),
    "gb_test_gate_fallback_launches": (_i32, [_vp, C.POINTER(_u64)]),
}

_lib = None


def library_path():
    return _build.LIB


def load():
    """Load the in-tree HIP library (raises if it has not been built - no CPU fallback)."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the gfx950 HIP library is the only implementation; there is no CPU fallback)" % path)
        # PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one
        # process cannot both open the GPU.  Importing torch first makes the dynamic loader bind
        # this library's NEEDED libamdhip64.so.7 to the copy torch already loaded.
        import torch  # noqa: F401
        lib = C.CDLL(path)
        for name, (res, args) in list(SIGNATURES.items()) + list(TEST_HOOK_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


class GoldibearError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("gb_status=%d: %s" % (status, message))
        self.status = status


class PermArgZeroError(GoldibearError):
    """GB_ERR_PERM_ARG_ZERO: ProverError::InvZeroPermArg (plonk/prover.rs:512-514) - re-randomise and retry."""


class TooManyPermArgFailuresError(GoldibearError):
    """ProverError::TooManyPermArgFailures (plonk/prover.rs:188-192, 226): MAX_PERM_ARG_RETRIES attempts failed, or
    the circuit has no random wire to re-randomise."""


class VerifyError(GoldibearError):
    """GB_ERR_VERIFY: the proof does not verify (the message names the failed check)."""


class ShapeError(GoldibearError, ValueError):
    """GB_ERR_INVALID: where the reference would assert!/panic! on a shape violation."""


# ---- the witness check (include/goldibear_gpu.h: gb_check_witness, gb_check_partition, gb_check_inputs)
class gb_violation(C.Structure):
    _fields_ = [("kind", _u32), ("gate", _u32), ("row", _u64), ("index", _u32), ("other_wire", _u32), ("other_row", _u64),
                ("value", _u64), ("other_value", _u64)]


class gb_check_result(C.Structure):
    _fields_ = [("num_gate_violations", _u64), ("num_selector_violations", _u64), ("num_copy_violations", _u64),
                ("copies_checked", _u32), ("num_listed", _u32)]


class gb_verify_result(C.Structure):
    _fields_ = [("status", _u32), ("check", _u32), ("query_round", _u32), ("index", _u32)]


class VerifyResult:
    """one gb_verify_result of gb_verify_batch: `status` is what gb_verify returns for the proof, `text` what it leaves in
    gb_last_error; query_round / index are None where the check has none"""
    __slots__ = ("ok", "status", "check", "text", "query_round", "index")

    def __init__(self, status, check, text, query_round, index):
        self.ok, self.status, self.check, self.text = status == GB_OK, int(status), int(check), text
        self.query_round = None if query_round == 0xFFFFFFFF else int(query_round)
        self.index = None if index == 0xFFFFFFFF else int(index)

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "VerifyResult(ok=%r, status=%d, check=%d, text=%r, query_round=%r, index=%r)" % (
            self.ok, self.status, self.check, self.text, self.query_round, self.index)


def verify_batch(ctx_handle, circuit_handle, proofs, entry="gb_verify_batch"):
    """gb_verify_batch on a list of proof byte strings -> [VerifyResult]; a failing proof is reported, not raised - malformed
    arguments (and HIP / memory errors) still raise"""
    import numpy as np
    lib = load()
    bufs = [np.frombuffer(bytes(p), dtype=np.uint8) for p in proofs]
    n = len(bufs)
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    # (an empty proof still needs a non-NULL pointer: it is a truncated proof, not a missing argument)
    empty = np.zeros(1, dtype=np.uint8)
    for i, b in enumerate(bufs):
        if not b.size:
            ptrs[i] = empty.ctypes.data
    lens = (C.c_size_t * max(n, 1))(*[b.size for b in bufs])
    res = (gb_verify_result * max(n, 1))()
    st = getattr(lib, entry)(ctx_handle, circuit_handle, ptrs, lens, n, 0, C.cast(res, C.c_void_p))
    if st not in (GB_OK, GB_ERR_VERIFY):
        check(st, ctx_handle)
    return [VerifyResult(r.status, r.check, (lib.gb_verify_check_text(r.check) or b"").decode(), r.query_round, r.index)
            for r in res[:n]]


def verify_compressed_batch(ctx_handle, circuit_handle, proofs):
    """gb_verify_compressed_batch on a list of CompressedProofWithPublicInputs byte strings -> [VerifyResult]: status and text are
    gb_verify_compressed's, query_round / index what verify_batch reports on the decompressed proof"""
    return verify_batch(ctx_handle, circuit_handle, proofs, entry="gb_verify_compressed_batch")


class gb_sigma_info(C.Structure):
    _fields_ = [("routed_cells", _u64), ("moved_cells", _u64), ("num_classes", _u64), ("largest_class", _u64), ("rounds", _u32),
                ("compared_partition", _u32)]


class gb_wiring_info(C.Structure):
    _fields_ = [("routed_cells", _u64), ("moved_cells", _u64), ("num_classes", _u64), ("largest_class", _u64), ("merged_targets", _u64),
                ("rounds", _u32), ("reserved", _u32)]


class Violation:
    """one gb_violation: kind (GB_VIOLATION_*) and the fields that kind uses (the others are zero)"""
    FIELDS = tuple(name for name, _ in gb_violation._fields_)
    __slots__ = FIELDS

    def __init__(self, kind, gate=0, row=0, index=0, other_wire=0, other_row=0, value=0, other_value=0):
        for name, v in zip(self.FIELDS, (kind, gate, row, index, other_wire, other_row, value, other_value)):
            setattr(self, name, int(v))

    @classmethod
    def from_struct(cls, s):
        return cls(*[getattr(s, name) for name in cls.FIELDS])

    def as_tuple(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def __eq__(self, other):
        return isinstance(other, Violation) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def __repr__(self):
        return "Violation(%s)" % ", ".join("%s=%d" % (name, getattr(self, name)) for name in self.FIELDS)

    def describe(self, built=None):
        """one line: the gate's id string from built.gate_ids (circuit_builder.BuiltCircuit; without it the gate's index), the row
        and the constraint; a copy violation prints both cells"""
        if self.kind == GB_VIOLATION_GATE:
            ids = getattr(built, "gate_ids", None)
            name = ids[self.gate] if ids is not None and self.gate < len(ids) else "gate %d" % self.gate
            return "row %d: %s, constraint %d = %d" % (self.row, name, self.index, self.value)
        if self.kind == GB_VIOLATION_SELECTOR:
            return "row %d: selector column %d holds %d, which names no gate of its group" % (self.row, self.index, self.value)
        return "row %d, wire %d = %d differs from the first cell of its copy class, row %d, wire %d = %d" % (
            self.row, self.index, self.value, self.other_row, self.other_wire, self.other_value)


def _parse_first_violation(message):
    """the violation gb_last_error names after GB_ERR_UNSATISFIED (csrc/check_host.inc describe_violation)"""
    import re
    m = re.search(r"gate violation at row (\d+): gate (\d+), constraint (\d+) = (\d+)", message)
    if m:
        row, gate, index, value = map(int, m.groups())
        return [Violation(GB_VIOLATION_GATE, gate=gate, row=row, index=index, value=value)]
    m = re.search(r"selector violation at row (\d+): selector column (\d+) holds (\d+)", message)
    if m:
        row, col, value = map(int, m.groups())
        return [Violation(GB_VIOLATION_SELECTOR, row=row, index=col, value=value)]
    m = re.search(r"copy violation at row (\d+), wire (\d+) = (\d+): the first cell of its class \(row (\d+), wire (\d+)\) holds (\d+)", message)
    if m:
        row, w, value, orow, ow, ovalue = map(int, m.groups())
        return [Violation(GB_VIOLATION_COPY, row=row, index=w, other_wire=ow, other_row=orow, value=value, other_value=ovalue)]
    return []


class UnsatisfiedError(GoldibearError):
    """GB_ERR_UNSATISFIED: the witness breaks a gate, a selector or a copy constraint.  `violations`: what the call listed - from
    gb_prove* under the option "check_witness" the first one, read off the message."""

    def __init__(self, status, message, violations=None):
        super().__init__(status, message)
        self.violations = list(violations) if violations is not None else _parse_first_violation(message)


def check(status, ctx_handle=None):
    if status == GB_OK:
        return
    msg = load().gb_last_error(ctx_handle)
    msg = msg.decode() if msg else ""
    cls = {GB_ERR_INVALID: ShapeError, GB_ERR_PERM_ARG_ZERO: PermArgZeroError, GB_ERR_VERIFY: VerifyError,
           GB_ERR_UNSATISFIED: UnsatisfiedError}.get(status, GoldibearError)
    raise cls(status, msg)
