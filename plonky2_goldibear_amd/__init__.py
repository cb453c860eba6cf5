"""plonky2_goldibear_amd - MI355X (gfx950) implementation of the plonky2_goldibear commitment hot path.

csrc/      hand-written HIP kernels + the C ABI declared in include/goldibear_gpu.h
native     ctypes binding of that ABI (no fallback: raises if the library is missing)
polynomial_batch  host-side mirror of PolynomialBatch / MerkleTree (fri/oracle.rs, hash/merkle_tree.rs)
fri         the polynomial commitment scheme on its own: prove_openings on any FriInstanceInfo, verify_fri_proof, verify_fri_proofs (fri/oracle.rs, fri/verifier.rs)
constraints the quotient of a caller's own constraints over any committed oracles, and the same constraints at the verifier's point: constraint_quotient, constraint_eval
polynomial  the transforms on their own: fft / ifft / coset_fft / coset_ifft / lde / lde_onto_coset (field/src/polynomial/mod.rs)
wiring      copy constraints -> sigma columns and representative map on the device: sigma_polys (plonk/permutation_argument.rs)
"""
from .native import GB_BABYBEAR, GB_GOLDILOCKS, GoldibearError, ShapeError  # noqa: F401
from .native import PermArgZeroError, TooManyPermArgFailuresError, VerifyError  # noqa: F401
from .native import UnsatisfiedError, VerifyResult, Violation  # noqa: F401
from .polynomial_batch import GpuContext, MerkleTree, PolynomialBatch, random_elements  # noqa: F401
from .polynomial import coset_fft, coset_ifft, fft, ifft, lde, lde_onto_coset  # noqa: F401
from .prover import CircuitData, SigmaInfo, VerifierCircuitData  # noqa: F401
from .wiring import WiringInfo, sigma_polys  # noqa: F401
from .fri import FriBatchInfo, FriConfig, FriInstanceInfo, FriOracleInfo, FriParams, FriPolynomialInfo  # noqa: F401
from .fri import prove_openings, verify_fri_proof, verify_fri_proofs  # noqa: F401
from .gate_program import GateProgram, ProgramGate, pack_programs  # noqa: F401
from .constraints import ConstraintProgram, constraint_eval, constraint_quotient, pack_constraint_programs  # noqa: F401
from .generator_program import GeneratorProgram, ProgramGenerator, pack_generator_programs  # noqa: F401
from .integer_gadgets import div_rem, is_less_than, mul_add_split_gate  # noqa: F401
