"""Host-side mirror of the reference's circuit/prover entry points, over the C ABI.

`CircuitData` stands for what `CircuitBuilder::build()` returns (plonk/circuit_builder.rs:1373-1378):
`prover_only` (constants_sigmas_commitment resident on the GPU, sigmas, circuit_digest) and
`verifier_only` (constants_sigmas_cap, circuit_digest).  `prove(witness, public_inputs)` is
`prove_with_partition_witness` (plonk/prover.rs:160-447) from an already generated
`MatrixWitness.wire_values` matrix to `ProofWithPublicInputs` bytes.
"""
import collections
import ctypes as C
import sys
import weakref

import numpy as np

from . import native as N
from .polynomial_batch import _as_columns, _as_input, _dtype, _live_contexts, is_column_list  # noqa: F401

_live_circuits = weakref.WeakSet()


class gb_circuit_config(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in (
        "field", "degree_bits", "num_wires", "num_routed_wires", "num_constants", "num_challenges",
        "max_quotient_degree_factor", "rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds",
        "arity_bits", "final_poly_bits", "num_selectors", "gate_constant", "gate_pi", "zero_knowledge", "num_public_inputs")]


class gb_challenger_state(C.Structure):
    """Challenger<F, H> by value (iop/challenger.rs:18-31); include/goldibear_gpu.h"""
    _fields_ = [("sponge_state", C.c_uint64 * 16), ("input_buffer", C.c_uint64 * 8), ("output_buffer", C.c_uint64 * 8),
                ("input_len", C.c_uint32), ("output_len", C.c_uint32)]


class gb_gate(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("kind", "param", "selector_index", "group_start", "group_end", "param2", "param3")]


def _program_table(programs):
    """gate_program.pack_programs: the flat word and offset arrays of the *_programs entry points"""
    from .gate_program import pack_programs
    return pack_programs(programs)


class _ProofBytesOps:
    """compress / decompress / verify_compressed over the C ABI (plonk/proof.rs:96-140, 183-265), shared by CircuitData and
    VerifierCircuitData; all three run on the host."""

    def _bytes_call(self, fn, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        out = np.empty(max(1 << 16, 2 * buf.size), dtype=np.uint8)
        n = C.c_size_t()
        N.check(fn(self.handle, buf.ctypes.data, buf.size, out.ctypes.data, out.size, C.byref(n)), getattr(getattr(self, "ctx", None), "handle", None))
        return out[: n.value].tobytes()

    def compress(self, proof_bytes):
        """ProofWithPublicInputs::compress -> CompressedProofWithPublicInputs bytes"""
        return self._bytes_call(self._lib.gb_proof_compress, proof_bytes)

    def decompress(self, compressed_bytes):
        """CompressedProofWithPublicInputs::decompress -> ProofWithPublicInputs bytes"""
        return self._bytes_call(self._lib.gb_proof_decompress, compressed_bytes)

    def verify_compressed(self, compressed_bytes):
        """CompressedProofWithPublicInputs::verify; True, or raises VerifyError / ShapeError"""
        buf = np.frombuffer(bytes(compressed_bytes), dtype=np.uint8)
        N.check(self._lib.gb_verify_compressed(self.handle, buf.ctypes.data, buf.size), getattr(getattr(self, "ctx", None), "handle", None))
        return True


class _FriParamsOps:
    """FriParams.reduction_arity_bits of a circuit object (gb_circuit_set_fri_reduction_arity_bits / its getter)"""

    def set_reduction_arity_bits(self, bits):
        arr = (C.c_uint32 * max(1, len(bits)))(*[int(b) for b in bits])
        N.check(self._lib.gb_circuit_set_fri_reduction_arity_bits(self.handle, arr, len(bits)), getattr(getattr(self, "ctx", None), "handle", None))

    @property
    def reduction_arity_bits(self):
        arr, n = (C.c_uint32 * 32)(), C.c_uint32()
        N.check(self._lib.gb_circuit_fri_reduction_arity_bits(self.handle, arr, C.byref(n)), getattr(getattr(self, "ctx", None), "handle", None))
        return [int(arr[i]) for i in range(n.value)]


NO_RANDOM_WIRE = "Permutation argument division by zero but no random wire was given to randomize the witness"


def prove_with_retries(data, redraw, prove_once, retry_wire, rng=None, salted=False, p3_repr=False, nothing_to_redraw=NO_RANDOM_WIRE):
    """The retry loop of prove_with_partition_witness (plonk/prover.rs:183-226) around one front's proof proper.  When the
    permutation argument hits a zero denominator (ProverError::InvZeroPermArg - with a 31-bit field and 2^20 rows about one proof
    in five) the reference overwrites `random_wire` with a fresh F::rand() and tries again, at most 3 attempts.
    data: the CircuitData (field, perm_arg_retries, drop_retry).  redraw(value): write the fresh value where this front keeps the
    random wire - None where it has nothing to re-draw (the error text is nothing_to_redraw).  prove_once(hint) -> proof bytes,
    raising PermArgZeroError; hint is retry_wire on the second and third attempts - they differ from the failed one in that wire
    only, and the library rebuilds just its column where it kept the rest - and None on the first and whenever salts or a seed
    are in play (salted: the full computation).  retry_wire None: the circuit has no random wire.  One rng draw per retry."""
    data.perm_arg_retries = 0
    for attempt in range(data.MAX_PERM_ARG_RETRIES):
        if attempt > 0:
            if redraw is None:
                raise N.TooManyPermArgFailuresError(N.GB_ERR_PERM_ARG_ZERO, nothing_to_redraw)
            rng = rng or np.random.default_rng()
            p = 0xFFFFFFFF00000001 if data.field == N.GB_GOLDILOCKS else 2013265921
            val = int(rng.integers(0, p, dtype=np.uint64))
            if p3_repr and data.field == N.GB_BABYBEAR:
                val = (val << 32) % p   # the Montgomery word of p3's BabyBear
            redraw(val)
            data.perm_arg_retries = attempt
        try:
            return prove_once(retry_wire if attempt > 0 and not salted else None)
        except N.PermArgZeroError:
            if retry_wire is None:   # no retry will follow: do not keep the failed attempt's commitment on the device
                data.drop_retry()
    data.drop_retry()   # giving up: the failed attempt's wires commitment and witness copy (~12 GB at 2^20 rows) go back
    raise N.TooManyPermArgFailuresError(N.GB_ERR_PERM_ARG_ZERO, "ProverError::TooManyPermArgFailures")


SigmaInfo = collections.namedtuple("SigmaInfo", [name for name, _ in N.gb_sigma_info._fields_])
SigmaInfo.__doc__ = "gb_sigma_info: what CircuitData.decode_sigmas found"


class CircuitData(_ProofBytesOps, _FriParamsOps):
    """Defaults are standard_recursion_config_gl (plonk/circuit_data.rs:102-116); `CircuitData.babybear(...)`
    fills in recursion_config_bb_narrow (:131-139)."""

    @classmethod
    def babybear(cls, ctx, degree_bits, constants_sigmas, k_is, *, num_challenges=6, **kw):
        d = dict(num_wires=167, num_routed_wires=41, arity_bits=3, num_challenges=num_challenges, field=N.GB_BABYBEAR)
        d.update(kw)
        return cls(ctx, degree_bits, constants_sigmas, k_is, **d)

    def __init__(self, ctx, degree_bits, constants_sigmas, k_is, *, num_wires=135, num_routed_wires=80, num_constants=2,
                 num_challenges=2, max_quotient_degree_factor=8, rate_bits=3, cap_height=4, proof_of_work_bits=16,
                 num_query_rounds=28, arity_bits=4, final_poly_bits=5, num_selectors=1, gate_constant=1, gate_pi=2,
                 field=N.GB_GOLDILOCKS, gates=None, zero_knowledge=False, num_public_inputs=0, reduction_arity_bits=None, p3_repr=False,
                 programs=None):
        """`gates` = None: the dummy circuit's gate set, given by the selector values gate_constant / gate_pi
        (gb_circuit_create).  Otherwise CommonCircuitData.gates with selectors_info, one tuple
        (kind, param, selector_index, group_start, group_end) per gate in sorted order (gb_circuit_create_gates; what
        circuit_builder.CircuitBuilder.build() passes); num_constants then counts the constant columns after the selectors.
        `programs`: the constraint programs of the GATE_PROGRAM entries (gate_program.GateProgram objects or their words), entry
        `param` of a program gate indexing this list (gb_circuit_create_programs)."""
        self.ctx, self._lib = ctx, ctx._lib
        self.field, self._dt = field, _dtype(field)
        hout = 4 if field == N.GB_GOLDILOCKS else 8
        self.cfg = gb_circuit_config(field, degree_bits, num_wires, num_routed_wires, num_constants, num_challenges,
                                     max_quotient_degree_factor, rate_bits, cap_height, proof_of_work_bits,
                                     num_query_rounds, arity_bits, final_poly_bits, num_selectors, gate_constant, gate_pi,
                                     1 if zero_knowledge else 0, num_public_inputs)
        cs_cols = is_column_list(constants_sigmas)   # constants_sigmas_vecs as build() holds them: one allocation per column
        ptr, shape, flags, keep = _as_columns(constants_sigmas, field) if cs_cols else _as_input(constants_sigmas, field)
        want = (num_selectors + num_constants + num_routed_wires, 1 << degree_bits)
        if tuple(shape) != want:
            raise N.ShapeError(N.GB_ERR_INVALID, "constants_sigmas must be %r, got %r" % (want, tuple(shape)))
        k = np.ascontiguousarray(k_is, dtype=self._dt)
        if k.shape != (num_routed_wires,):
            raise N.ShapeError(N.GB_ERR_INVALID, "k_is must have num_routed_wires entries")
        if flags == N.GB_INPUT_DEVICE:
            import torch
            kd = torch.from_numpy(k.view(np.int64 if k.itemsize == 8 else np.int32)).to("cuda:%d" % ctx.device)
            kptr, keep2 = kd.data_ptr(), kd
        else:
            kptr, keep2 = k.ctypes.data, k
        h = C.c_void_p()
        if p3_repr:   # constants_sigmas and k_is are the field types' in-memory words (host input)
            flags |= N.GB_INPUT_P3_REPR
        if gates is None:
            fn = self._lib.gb_circuit_create_cols if cs_cols else self._lib.gb_circuit_create
            N.check(fn(ctx.handle, C.byref(self.cfg), ptr, kptr, flags, C.byref(h)), ctx.handle)
        elif programs is None:
            arr = (gb_gate * len(gates))(*[gb_gate(*g) for g in gates])
            fn = self._lib.gb_circuit_create_gates_cols if cs_cols else self._lib.gb_circuit_create_gates
            N.check(fn(ctx.handle, C.byref(self.cfg), arr, len(gates), ptr, kptr, flags, C.byref(h)), ctx.handle)
        else:
            arr = (gb_gate * len(gates))(*[gb_gate(*g) for g in gates])
            words, offsets = _program_table(programs)
            fn = self._lib.gb_circuit_create_programs_cols if cs_cols else self._lib.gb_circuit_create_programs
            N.check(fn(ctx.handle, C.byref(self.cfg), arr, len(gates), words.ctypes.data_as(C.POINTER(C.c_uint64)),
                       offsets.ctypes.data_as(C.POINTER(C.c_uint32)), len(programs), ptr, kptr, flags, C.byref(h)), ctx.handle)
        del keep, keep2
        self.handle = h
        cap = np.empty((1 << cap_height, hout), dtype=self._dt)
        dig = np.empty(hout, dtype=self._dt)
        N.check(self._lib.gb_circuit_verifier_data(h, cap.ctypes.data, dig.ctypes.data), ctx.handle)
        self.constants_sigmas_cap, self.circuit_digest = cap, dig
        self._proof_buf = None
        _live_circuits.add(self)
        if reduction_arity_bits is not None:   # FriReductionStrategy::Fixed / MinSize (fri_params.py); None = ConstantArityBits
            self.set_reduction_arity_bits(reduction_arity_bits)

    MAX_PERM_ARG_RETRIES = 3  # plonk/prover.rs:183

    @staticmethod
    def _seed_bytes(seed, salts):
        """the 32 seed bytes of GB_SALTS_FROM_SEED as a buffer ctypes can point to (None without a seed)"""
        if seed is None:
            return None
        if salts is not None:
            raise N.ShapeError(N.GB_ERR_INVALID, "seed= and salts= are exclusive: the seed is what the salts are generated from")
        raw = bytes(seed)
        if len(raw) != N.GB_SEED_SIZE:
            raise N.ShapeError(N.GB_ERR_INVALID, "seed must be %d bytes, got %d" % (N.GB_SEED_SIZE, len(raw)))
        return C.create_string_buffer(raw, N.GB_SEED_SIZE)

    def prove(self, witness, public_inputs=(), random_wire=None, rng=None, salts=None, p3_repr=False, seed=None):
        """prove_with_partition_witness (plonk/prover.rs:160-226): the retry loop around the proof proper.  When the
        permutation argument hits a zero denominator (ProverError::InvZeroPermArg - with a 31-bit field and 2^20 rows
        about one proof in five) the reference overwrites `random_wire` (circuit_builder.rs:1073-1075: the last wire of the
        PublicInputGate row, given here as (column, row)) with a fresh F::rand() and tries again, at most 3 attempts.
        `witness` is modified in place in that case, like the reference's `witness.wire_values`.  `witness`: the [num_wires][n]
        matrix, or MatrixWitness.wire_values as the reference holds it - a list of num_wires separately allocated columns
        (gb_prove_cols).  p3_repr: host elements are the reference's in-memory words (GB_INPUT_P3_REPR).  seed: 32 bytes the
        library generates a zero-knowledge circuit's salts from, on the device (GB_SALTS_FROM_SEED) - one seed per proof."""
        self._seed_bytes(seed, salts)

        def redraw(val):
            col, row = random_wire
            if is_column_list(witness) and isinstance(witness[col], np.ndarray):
                witness[col][row] = val
            elif isinstance(witness, np.ndarray):
                witness[col, row] = val
            else:  # torch device tensor(s) holding the same-width integer bit pattern
                t = witness[col] if is_column_list(witness) else witness
                sval = val - (1 << (8 * t.element_size())) if val >> (8 * t.element_size() - 1) else val
                if is_column_list(witness):
                    t[row] = sval
                else:
                    t[col, row] = sval
                # that write is on torch's current stream; the library reads the column on its own stream: order them
                import torch
                torch.cuda.current_stream(t.device).synchronize()

        return prove_with_retries(self, redraw if random_wire is not None else None,
                                  lambda hint: self.prove_once(witness, public_inputs, salts, retry_wire=hint, p3_repr=p3_repr, seed=seed),
                                  tuple(random_wire) if random_wire is not None else None, rng=rng,
                                  salted=salts is not None or seed is not None, p3_repr=p3_repr)

    def drop_retry(self):
        """release what an attempt that ended in PermArgZeroError keeps on the device for the incremental retry"""
        if self.handle:
            N.check(self._lib.gb_circuit_drop_retry(self.handle), self.ctx.handle)

    def arm_perm_arg_failure(self):
        """TEST HOOK (include/goldibear_gpu_test_hooks.h): the next prove_once raises PermArgZeroError once its Z computation is
        done, keeping what gb_prove_retry builds on - the only way to drive the retry path of a 64-bit field"""
        N.check(self._lib.gb_test_arm_perm_arg_failure(self.handle), self.ctx.handle)

    def prove_once(self, witness, public_inputs=(), salts=None, retry_wire=None, p3_repr=False, seed=None):
        """internal_prove_with_partition_witness (plonk/prover.rs:228-447); raises PermArgZeroError.  A circuit created with
        zero_knowledge=True takes `salts`: [3][4][N] canonical elements (the F::rand_vec columns of the wires / Zs / quotient
        commitments, fri/oracle.rs:144-148), in the same memory space as the witness - or `seed`: 32 bytes (host) from which the
        library generates those columns on the device (GB_SALTS_FROM_SEED: element [s][j][t] = element t of the stream
        (seed, (GB_STREAM_SALTS, s, j)) of random_elements)."""
        sbuf = self._seed_bytes(seed, salts)
        cols = is_column_list(witness)
        ptr, shape, flags, keep = _as_columns(witness, self.field) if cols else _as_input(witness, self.field)
        lib, sfx = self._lib, "_cols" if cols else ""
        if p3_repr:
            flags |= N.GB_INPUT_P3_REPR
        want = (self.cfg.num_wires, 1 << self.cfg.degree_bits)
        if tuple(shape) != want:
            raise N.ShapeError(N.GB_ERR_INVALID, "witness must be %r, got %r" % (want, tuple(shape)))
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        sptr = None
        if salts is not None and sbuf is None:
            sptr, sshape, sflags, skeep = _as_input(np.reshape(salts, (3 * N.GB_SALT_SIZE, -1)) if isinstance(salts, np.ndarray)
                                                    else salts.reshape(3 * N.GB_SALT_SIZE, -1), self.field)
            if tuple(sshape) != (3 * N.GB_SALT_SIZE, 1 << (self.cfg.degree_bits + self.cfg.rate_bits)) or sflags != (flags & N.GB_INPUT_DEVICE):
                raise N.ShapeError(N.GB_ERR_INVALID, "salts must be [3][4][N] in the same memory space as the witness")
        got = self._prove_call("gb_prove", ptr, flags, (pis.ctypes.data if pis.size else None, pis.size), sptr, retry_wire, sbuf,
                               salted_name="gb_prove_salted", sfx=sfx)
        del keep
        return got

    def _prove_call(self, name, ptr, flags, mid, salts_ptr, retry_wire, sbuf, salted_name=None, sfx=""):
        """The one proof call behind prove_once / prove_partition_once / prove_inputs_once -> proof bytes.  `name`(handle, ptr, flags,
        *mid, salts, out, cap, len) is the front's entry; `name`_retry takes (wire, row) behind the flags and no salts - the attempt
        after a failure, never with salts or a seed; salted_name: the entry that takes the salts where `name` itself takes none
        (gb_prove); sfx: "_cols" for the entries that take a column list.  sbuf: the seed buffer of _seed_bytes, which goes where
        the salts go, under GB_SALTS_FROM_SEED."""
        if self._proof_buf is None:
            self._proof_buf = np.empty(8 << 20, dtype=np.uint8)
        n = C.c_size_t()
        out = (self._proof_buf.ctypes.data, self._proof_buf.size, C.byref(n))
        if sbuf is not None:
            flags, salts_ptr = flags | N.GB_SALTS_FROM_SEED, C.cast(sbuf, C.c_void_p)
        if salts_ptr is None and retry_wire is not None:   # (wire, row): the one element re-drawn since the attempt that failed
            st = getattr(self._lib, name + "_retry" + sfx)(self.handle, ptr, flags, int(retry_wire[0]), int(retry_wire[1]), *mid, *out)
        elif salts_ptr is None and salted_name is not None:
            st = getattr(self._lib, name + sfx)(self.handle, ptr, flags, *mid, *out)
        else:
            st = getattr(self._lib, (salted_name or name) + sfx)(self.handle, ptr, flags, *mid, salts_ptr, *out)
        N.check(st, self.ctx.handle)
        return self._proof_buf[: n.value].tobytes()

    def _host_salts(self, salts):
        """[3][4][N] host salts of a witness front -> (pointer, the array that owns it); (None, None) without salts"""
        if salts is None:
            return None, None
        sa = np.ascontiguousarray(salts, dtype=self._dt).reshape(3 * N.GB_SALT_SIZE, -1)
        if sa.shape[1] != 1 << (self.cfg.degree_bits + self.cfg.rate_bits):
            raise N.ShapeError(N.GB_ERR_INVALID, "salts must be [3][4][N]")
        return sa.ctypes.data, sa

    # ---- prove() from the partition witness (include/goldibear_gpu.h: gb_circuit_set_partition, gb_prove_partition*)
    def set_partition(self, representative_map, public_input_targets=()):
        """ProverOnlyCircuitData.representative_map (plonk/circuit_data.rs:454), indexed by Target::index - wire (row, column) ->
        row * num_wires + column, virtual target i -> n * num_wires + i - and the target indices of prover_data.public_inputs"""
        m = np.ascontiguousarray(representative_map, dtype=np.uint64)
        t = np.ascontiguousarray(public_input_targets, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        N.check(self._lib.gb_circuit_set_partition(self.handle, m.ctypes.data_as(u64p), m.size,
                                                   t.ctypes.data_as(u64p) if t.size else None, t.size), self.ctx.handle)
        self.num_targets = int(m.size)

    def _partition_values(self, values, p3_repr):
        v = np.ascontiguousarray(values, dtype=self._dt)
        if v.shape != (getattr(self, "num_targets", -1),):
            raise N.ShapeError(N.GB_ERR_INVALID, "values must have one entry per target of the map given to set_partition")
        return v, (N.GB_INPUT_P3_REPR if p3_repr else N.GB_INPUT_HOST)

    def prove_partition_once(self, values, salts=None, retry_wire=None, p3_repr=False, seed=None):
        """internal_prove_with_partition_witness from PartitionWitness.values (None as zero): full_witness() runs on the device.
        salts / seed as for prove_once (both host)."""
        sbuf = self._seed_bytes(seed, salts)
        v, flags = self._partition_values(values, p3_repr)
        sptr, keep = self._host_salts(salts) if sbuf is None else (None, None)
        return self._prove_call("gb_prove_partition", v.ctypes.data, flags, (), sptr, retry_wire, sbuf)

    def prove_partition(self, values, representative=None, random_wire=None, rng=None, salts=None, p3_repr=False, seed=None):
        """prove_with_partition_witness (plonk/prover.rs:160-226) on the reference's own witness object: the retry loop of prove()
        over gb_prove_partition / gb_prove_partition_retry.  random_wire = (column, row) as for prove(); `representative` is the
        entry of `values` that holds it (representative_map[row * num_wires + column]), re-drawn in place after InvZeroPermArg."""
        self._seed_bytes(seed, salts)

        def redraw(val):
            values[int(representative)] = val

        return prove_with_retries(self, redraw if random_wire is not None and representative is not None else None,
                                  lambda hint: self.prove_partition_once(values, salts, retry_wire=hint, p3_repr=p3_repr, seed=seed),
                                  random_wire, rng=rng, salted=salts is not None or seed is not None, p3_repr=p3_repr)

    def expand_partition(self, values, p3_repr=False):
        """partition_witness.full_witness() (iop/witness.rs:359-371) alone: -> a torch device tensor [num_wires][n] of canonical
        words (as int64 / int32 bit patterns), usable as the device input of commits and of zs_partial_products"""
        import torch
        v, flags = self._partition_values(values, p3_repr)
        out = torch.empty((self.cfg.num_wires, 1 << self.cfg.degree_bits), dtype=torch.int64 if self._dt == np.uint64 else torch.int32,
                          device="cuda:%d" % self.ctx.device)
        torch.cuda.current_stream(out.device).synchronize()
        N.check(self._lib.gb_expand_partition(self.handle, v.ctypes.data, flags, out.data_ptr()), self.ctx.handle)
        N.check(self._lib.gb_ctx_synchronize(self.ctx.handle), self.ctx.handle)
        return out

    # ---- prove() from the inputs alone (include/goldibear_gpu.h: gb_circuit_set_generators, gb_generate_partition, gb_prove_inputs*)
    GENERATOR_DTYPE = np.dtype([("kind", "<u4"), ("gate", "<u4"), ("a", "<u8"), ("b", "<u8")])   # gb_generator

    def set_generators(self, records, input_targets, constants):
        """prover_only.generators as gb_generator records [(kind, gate, a, b)], the target indices whose values the host supplies
        per proof, and the circuit's constants columns [num_constants][n]; after set_partition.  A gadget generator is several
        records in a row (native.gadget_records: a head, then its GB_GEN_TARGETS continuation): the list is flat"""
        words = np.array(records, dtype=np.uint64).reshape(-1, 4)
        rec = np.zeros(len(words), dtype=self.GENERATOR_DTYPE)
        for k, name in enumerate(("kind", "gate", "a", "b")):
            rec[name] = words[:, k]
        t = np.ascontiguousarray(input_targets, dtype=np.uint64)
        k = np.ascontiguousarray(constants, dtype=np.uint64)
        if k.size != self.cfg.num_constants << self.cfg.degree_bits:
            raise N.ShapeError(N.GB_ERR_INVALID, "constants must be [num_constants][n]")
        u64p = C.POINTER(C.c_uint64)
        N.check(self._lib.gb_circuit_set_generators(self.handle, rec.ctypes.data if rec.size else None, rec.size,
                                                    t.ctypes.data_as(u64p) if t.size else None, t.size,
                                                    k.ctypes.data_as(u64p) if k.size else None, 0), self.ctx.handle)
        self.num_inputs = int(t.size)

    def set_generator_programs(self, programs):
        """the circuit's generator programs (generator_program.GeneratorProgram or lists of words), which the GB_GEN_PROGRAM
        records of set_generators name by index; after set_partition and before set_generators.  An empty list clears them."""
        from .generator_program import pack_generator_programs
        words, offsets = pack_generator_programs(programs)
        N.check(self._lib.gb_circuit_set_generator_programs(self.handle, words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                            offsets.ctypes.data_as(C.POINTER(C.c_uint32)), len(offsets) - 1),
                self.ctx.handle)

    def generators_info(self):
        """-> dict(num_levels, num_launches, num_unrunnable, num_checks, num_classes) of the schedule"""
        names = ("num_levels", "num_launches", "num_unrunnable", "num_checks", "num_classes")
        out = [C.c_uint32() for _ in names]
        N.check(self._lib.gb_circuit_generators_info(self.handle, *[C.byref(x) for x in out]), self.ctx.handle)
        return {k: int(v.value) for k, v in zip(names, out)}

    def generator_classes(self):
        """the representative target of every class of the schedule, in the order of generate_partition's values"""
        out = np.zeros(self.generators_info()["num_classes"], dtype=np.uint64)
        N.check(self._lib.gb_circuit_generator_classes(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size), self.ctx.handle)
        return out

    def _input_values(self, input_values, p3_repr):
        v = np.ascontiguousarray(input_values, dtype=self._dt)
        if v.shape != (getattr(self, "num_inputs", -1),):
            raise N.ShapeError(N.GB_ERR_INVALID, "input_values must have one entry per input target given to set_generators")
        return v, (N.GB_INPUT_P3_REPR if p3_repr else N.GB_INPUT_HOST)

    def generate_partition(self, input_values, p3_repr=False):
        """generate_partial_witness (iop/generator.rs:25-106) on the device -> a host array, one canonical value per class of
        generator_classes()"""
        import torch
        v, flags = self._input_values(input_values, p3_repr)
        out = torch.empty(max(1, self.generators_info()["num_classes"]), dtype=torch.int64 if self._dt == np.uint64 else torch.int32,
                          device="cuda:%d" % self.ctx.device)
        torch.cuda.current_stream(out.device).synchronize()
        N.check(self._lib.gb_generate_partition(self.handle, v.ctypes.data if v.size else None, flags, out.data_ptr()), self.ctx.handle)
        N.check(self._lib.gb_ctx_synchronize(self.ctx.handle), self.ctx.handle)
        return out.cpu().numpy().view(self._dt)[:self.generators_info()["num_classes"]]

    def prove_inputs_once(self, input_values, salts=None, retry_wire=None, p3_repr=False, seed=None):
        """prove() (plonk/prover.rs:136-158) from the inputs: the generators, full_witness() and the proof on the device.
        salts / seed as for prove_once (both host)."""
        sbuf = self._seed_bytes(seed, salts)
        v, flags = self._input_values(input_values, p3_repr)
        sptr, keep = self._host_salts(salts) if sbuf is None else (None, None)
        return self._prove_call("gb_prove_inputs", v.ctypes.data if v.size else None, flags, (), sptr, retry_wire, sbuf)

    # ---- does the witness satisfy the circuit?  (include/goldibear_gpu.h: gb_check_witness, gb_check_partition, gb_check_inputs)
    def _check_call(self, call, max_violations):
        """-> (violations, result): the listed violations as native.Violation objects (an empty list: satisfied) and the counts"""
        cap = int(max_violations)
        out = (N.gb_violation * max(1, cap))()
        res = N.gb_check_result()
        st = call(C.cast(out, C.c_void_p) if cap else None, cap, C.cast(C.pointer(res), C.c_void_p))
        if st not in (N.GB_OK, N.GB_ERR_UNSATISFIED):
            N.check(st, self.ctx.handle)
        return [N.Violation.from_struct(out[i]) for i in range(res.num_listed)], res

    def check_witness(self, witness, public_inputs=(), max_violations=16, p3_repr=False):
        """evaluate every active gate's constraints on the rows of `witness` ([num_wires][n], host or device as for prove) and, on
        a circuit with a partition, the copy constraints: -> (violations, result), at most max_violations listed - selector
        violations by (row, column), gate violations by (row, gate), copy violations by cell - the counts of `result` exact"""
        ptr, shape, flags, keep = _as_input(witness, self.field)
        if p3_repr:
            flags |= N.GB_INPUT_P3_REPR
        want = (self.cfg.num_wires, 1 << self.cfg.degree_bits)
        if tuple(shape) != want:
            raise N.ShapeError(N.GB_ERR_INVALID, "witness must be %r, got %r" % (want, tuple(shape)))
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        pis_ptr = pis.ctypes.data_as(C.POINTER(C.c_uint64)) if pis.size else None
        got = self._check_call(lambda out, cap, res: self._lib.gb_check_witness(self.handle, ptr, flags, pis_ptr, pis.size, out, cap, res),
                               max_violations)
        del keep
        return got

    def check_partition(self, values, max_violations=16, p3_repr=False):
        """the same from PartitionWitness.values: the expansion of prove_partition, then the check"""
        v, flags = self._partition_values(values, p3_repr)
        return self._check_call(lambda out, cap, res: self._lib.gb_check_partition(self.handle, v.ctypes.data, flags, out, cap, res),
                                max_violations)

    def check_inputs(self, input_values, max_violations=16, p3_repr=False):
        """the same from the inputs: the generators and the expansion of prove_inputs on the device, then the check"""
        v, flags = self._input_values(input_values, p3_repr)
        vp = v.ctypes.data if v.size else None
        return self._check_call(lambda out, cap, res: self._lib.gb_check_inputs(self.handle, vp, flags, out, cap, res), max_violations)

    # ---- the copy constraints from sigma alone (include/goldibear_gpu.h: gb_circuit_decode_sigmas, gb_circuit_copy_classes)
    def decode_sigmas(self, flags=0):
        """read the copy permutation back out of the sigma columns on the device and keep its cycles as copy classes -> SigmaInfo.
        From then on check_witness - and prove* under the option "check_witness" - check the copy constraints of a circuit that
        has no partition (copies_checked = 2); with a partition set, the partition's classes are compared with the decoded ones
        (ShapeError names the first cell where they differ).  A repeated call does no device work."""
        info = N.gb_sigma_info()
        N.check(self._lib.gb_circuit_decode_sigmas(self.handle, flags, C.cast(C.pointer(info), C.c_void_p)), self.ctx.handle)
        return SigmaInfo(*[int(getattr(info, name)) for name, _ in N.gb_sigma_info._fields_])

    def copy_classes(self):
        """after decode_sigmas: u32[2^degree_bits * num_wires], per wire cell row * num_wires + column the lowest cell of its copy
        class (a non-routed wire and a cell sigma does not move: itself)"""
        out = np.empty(self.cfg.num_wires << self.cfg.degree_bits, dtype=np.uint32)
        N.check(self._lib.gb_circuit_copy_classes(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32))), self.ctx.handle)
        return out

    @property
    def constants_sigmas_commitment(self):
        """ProverOnlyCircuitData.constants_sigmas_commitment (plonk/circuit_data.rs:532-534): a PolynomialBatch view that the
        circuit keeps owning."""
        from .polynomial_batch import PolynomialBatch
        h = C.c_void_p()
        N.check(self._lib.gb_circuit_constants_sigmas_commitment(self.handle, C.byref(h)), self.ctx.handle)
        return PolynomialBatch(self.ctx, h, borrowed=True)

    # ---- the stages of prove() one at a time, for a host that keeps the reference's prover loop and Challenger
    def _nzs(self):
        c = self.cfg
        return c.num_challenges * (-(-c.num_routed_wires // c.max_quotient_degree_factor))

    def _challenges(self, xs):
        a = np.ascontiguousarray(xs, dtype=self._dt)
        if a.shape != (self.cfg.num_challenges,):
            raise N.ShapeError(N.GB_ERR_INVALID, "expected num_challenges field elements")
        return a

    def zs_partial_products(self, witness, betas, gammas, p3_repr=False):
        """wires_permutation_partial_products_and_zs for every challenge (plonk/prover.rs:305-329, 449-546) ->
        [num_challenges * (1 + num_partial_products)][n] values, Zs first; host array for a host witness, device tensor for a
        device one.  Raises PermArgZeroError (InvZeroPermArg)."""
        cols = is_column_list(witness)
        ptr, shape, flags, keep = _as_columns(witness, self.field) if cols else _as_input(witness, self.field)
        n = 1 << self.cfg.degree_bits
        if tuple(shape) != (self.cfg.num_wires, n):
            raise N.ShapeError(N.GB_ERR_INVALID, "witness must be [num_wires][n]")
        b, g = self._challenges(betas), self._challenges(gammas)
        dev = flags == N.GB_INPUT_DEVICE
        if p3_repr:
            flags |= N.GB_INPUT_P3_REPR
        if dev:
            import torch
            w0 = witness[0] if cols else witness
            out = torch.empty((self._nzs(), n), dtype=w0.dtype, device=w0.device)
            optr = out.data_ptr()
        else:
            out = np.empty((self._nzs(), n), dtype=self._dt)
            optr = out.ctypes.data
        fn = self._lib.gb_zs_partial_products_cols if cols else self._lib.gb_zs_partial_products
        N.check(fn(self.handle, ptr, flags, b.ctypes.data, g.ctypes.data, optr), self.ctx.handle)
        del keep
        return out

    def quotient_polys(self, wires, zs_partial_products, public_inputs_hash, betas, gammas, alphas):
        """compute_quotient_polys + the split into chunks (plonk/prover.rs:345-376, 712-926): `wires` / `zs_partial_products` are
        the PolynomialBatch commitments of this proof -> [num_challenges * quotient_degree_factor][n] coefficients (host)."""
        hout = 4 if self.field == N.GB_GOLDILOCKS else 8
        ph = np.ascontiguousarray(public_inputs_hash, dtype=self._dt)
        if ph.shape != (hout,):
            raise N.ShapeError(N.GB_ERR_INVALID, "public_inputs_hash must have NUM_HASH_OUT_ELTS elements")
        b, g, a = self._challenges(betas), self._challenges(gammas), self._challenges(alphas)
        out = np.empty((self.cfg.num_challenges * self.cfg.max_quotient_degree_factor, 1 << self.cfg.degree_bits), dtype=self._dt)
        N.check(self._lib.gb_quotient_polys(self.handle, wires.handle, zs_partial_products.handle, ph.ctypes.data, b.ctypes.data,
                                            g.ctypes.data, a.ctypes.data, N.GB_INPUT_HOST, out.ctypes.data), self.ctx.handle)
        return out

    def prove_openings(self, wires, zs_partial_products, quotient, zeta, challenger, out_cap=None):
        """PolynomialBatch::prove_openings on this circuit's FRI instance (fri/oracle.rs:187-246, plonk/prover.rs:422-437).
        `challenger` = (sponge_state, input_buffer, output_buffer) after observe_openings, canonical ints.
        -> (FriProof bytes, challenger afterwards in the same form).  `out_cap` (tests): capacity handed to the library instead
        of the wrapper's own buffer; when it is too small the call raises (status GB_ERR_BUFFER_TOO_SMALL) after recording the
        size the library asked for in `last_fri_proof_len` and the challenger it handed back in `last_challenger`."""
        d = 2 if self.field == N.GB_GOLDILOCKS else 4
        z = np.ascontiguousarray(zeta, dtype=self._dt)
        if z.shape != (d,):
            raise N.ShapeError(N.GB_ERR_INVALID, "zeta must have %d coordinates" % d)
        st, inp, outb = challenger
        w = 12 if self.field == N.GB_GOLDILOCKS else 16
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
        if self._proof_buf is None:
            self._proof_buf = np.empty(8 << 20, dtype=np.uint8)
        n = C.c_size_t()
        cap = self._proof_buf.size if out_cap is None else min(int(out_cap), self._proof_buf.size)
        st = self._lib.gb_prove_openings(self.handle, wires.handle, zs_partial_products.handle, quotient.handle, z.ctypes.data,
                                         C.byref(cs), self._proof_buf.ctypes.data if cap else None, cap, C.byref(n))
        after = ([int(cs.sponge_state[i]) for i in range(w)], [int(cs.input_buffer[i]) for i in range(cs.input_len)],
                 [int(cs.output_buffer[i]) for i in range(cs.output_len)])
        self.last_fri_proof_len, self.last_challenger = n.value, after
        N.check(st, self.ctx.handle)
        return self._proof_buf[: n.value].tobytes(), after

    def verify(self, proof_bytes):
        """CircuitData::verify (plonk/circuit_data.rs:290-300 -> plonk/verifier.rs:17-128): True, or raises VerifyError naming
        the failed check (ShapeError for malformed bytes).  Runs on the host, like the reference's verifier."""
        buf = np.frombuffer(bytes(proof_bytes), dtype=np.uint8)
        N.check(self._lib.gb_verify(self.handle, buf.ctypes.data, buf.size), self.ctx.handle)
        return True

    def verify_batch(self, proofs):
        """verify() of many proofs of this circuit at once, the query rounds on the device (gb_verify_batch): a list of
        native.VerifyResult, one per proof - status and text are verify()'s; a failing proof is reported, not raised."""
        return N.verify_batch(self.ctx.handle, self.handle, proofs)

    def verify_compressed_batch(self, proofs):
        """verify_compressed() of many compressed proofs of this circuit at once, checked as they stand on the device
        (gb_verify_compressed_batch): a list of native.VerifyResult, one per proof - status and text are verify_compressed()'s."""
        return N.verify_compressed_batch(self.ctx.handle, self.handle, proofs)

    def free(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self._lib.gb_circuit_free(self.handle)
        self.handle = None

    def __del__(self):
        if not sys.is_finalizing():
            self.free()


class VerifierCircuitData(_ProofBytesOps, _FriParamsOps):
    """VerifierCircuitData (plonk/circuit_data.rs:358-380): CommonCircuitData + VerifierOnlyCircuitData, enough to verify and
    nothing else.  Built on gb_verifier_create, which touches no device - usable without a GPU context."""

    def __init__(self, degree_bits, gates, k_is, constants_sigmas_cap, circuit_digest, *, num_wires=135, num_routed_wires=80,
                 num_constants=2, num_challenges=2, max_quotient_degree_factor=8, rate_bits=3, cap_height=4,
                 proof_of_work_bits=16, num_query_rounds=28, arity_bits=4, final_poly_bits=5, num_selectors=1,
                 zero_knowledge=False, field=N.GB_GOLDILOCKS, num_public_inputs=0, reduction_arity_bits=None, programs=None):
        """`gates`: (kind, param, selector_index, group_start, group_end[, param2, param3]) per gate, sorted as in
        CommonCircuitData.gates; num_constants counts the constant columns after the selectors; reduction_arity_bits:
        FriParams.reduction_arity_bits when the strategy is not ConstantArityBits(arity_bits, final_poly_bits); programs: the
        constraint programs of the GATE_PROGRAM entries, as for CircuitData (gb_verifier_create_programs)."""
        self._lib = N.load()
        self.field, self._dt = field, _dtype(field)
        hout = 4 if field == N.GB_GOLDILOCKS else 8
        self.cfg = gb_circuit_config(field, degree_bits, num_wires, num_routed_wires, num_constants, num_challenges,
                                     max_quotient_degree_factor, rate_bits, cap_height, proof_of_work_bits, num_query_rounds,
                                     arity_bits, final_poly_bits, num_selectors, 0, 0, 1 if zero_knowledge else 0,
                                     num_public_inputs)
        k = np.ascontiguousarray(k_is, dtype=self._dt)
        cap = np.ascontiguousarray(constants_sigmas_cap, dtype=self._dt)
        dig = np.ascontiguousarray(circuit_digest, dtype=self._dt)
        if k.shape != (num_routed_wires,) or cap.shape != (1 << cap_height, hout) or dig.shape != (hout,):
            raise N.ShapeError(N.GB_ERR_INVALID, "k_is / constants_sigmas_cap / circuit_digest have the wrong shape")
        arr = (gb_gate * len(gates))(*[gb_gate(*g) for g in gates])
        h = C.c_void_p()
        if programs is None:
            N.check(self._lib.gb_verifier_create(None, C.byref(self.cfg), arr, len(gates), k.ctypes.data, cap.ctypes.data,
                                                 dig.ctypes.data, C.byref(h)))
        else:
            words, offsets = _program_table(programs)
            N.check(self._lib.gb_verifier_create_programs(None, C.byref(self.cfg), arr, len(gates),
                                                          words.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                          offsets.ctypes.data_as(C.POINTER(C.c_uint32)), len(programs),
                                                          k.ctypes.data, cap.ctypes.data, dig.ctypes.data, C.byref(h)))
        self.handle = h
        if reduction_arity_bits is not None:
            self.set_reduction_arity_bits(reduction_arity_bits)

    def verify(self, proof_bytes):
        """plonk/verifier.rs:17-128; True, or raises VerifyError naming the failed check."""
        buf = np.frombuffer(bytes(proof_bytes), dtype=np.uint8)
        N.check(self._lib.gb_verify(self.handle, buf.ctypes.data, buf.size))
        return True

    def verify_batch(self, ctx, proofs):
        """verify() of many proofs at once on the device of `ctx` (a GpuContext; the object itself has none): a list of
        native.VerifyResult, one per proof - a failing proof is reported, not raised."""
        return N.verify_batch(getattr(ctx, "handle", None), self.handle, proofs)

    def verify_compressed_batch(self, ctx, proofs):
        """gb_verify_compressed_batch with this verifier object as the circuit and `ctx`'s device: a list of native.VerifyResult,
        one per compressed proof - a failing proof is reported, not raised."""
        return N.verify_compressed_batch(getattr(ctx, "handle", None), self.handle, proofs)

    def free(self):
        if getattr(self, "handle", None):
            self._lib.gb_circuit_free(self.handle)
        self.handle = None

    def __del__(self):
        if not sys.is_finalizing():
            self.free()
