"""The retry loop of prove_with_partition_witness (plonk/prover.rs:183-226) as the three fronts share it - prover.prove_with_retries
under CircuitData.prove, CircuitData.prove_partition and BuiltCircuit.prove_inputs - driven with stubs: a "prove once" that raises
PermArgZeroError k times and then returns bytes, a seeded generator.  What it pins: one draw per retry and nothing else drawn (the
proofs other tests pin depend on the stream), the Montgomery word of p3's BabyBear, perm_arg_retries, a hint on the second and
third attempts only and never with salts or a seed, drop_retry exactly when the loop gives up or no random wire exists, and the
texts of the two "nothing to re-draw" errors.  CPU only: no library call is made."""
import numpy as np
import pytest

from plonky2_goldibear_amd import native as N
from plonky2_goldibear_amd.circuit_builder import BuiltCircuit, wire
from plonky2_goldibear_amd.prover import CircuitData, prove_with_retries

GL_P, BB_P = 0xFFFFFFFF00000001, 2013265921
FIELDS = [pytest.param(N.GB_GOLDILOCKS, False, id="goldilocks"), pytest.param(N.GB_BABYBEAR, True, id="babybear-p3")]
SEED = 20240611
RW = (7, 3)   # (column, row)
NO_RANDOM_WIRE = "Permutation argument division by zero but no random wire was given to randomize the witness"
NO_RANDOM_INPUT = "Permutation argument division by zero but the random wire is no input to randomize"
GIVING_UP = "ProverError::TooManyPermArgFailures"


def _draws(field, p3, count):
    """the first `count` values a retry writes: one rng.integers(0, p, dtype=uint64) each, p3 BabyBear as its Montgomery word"""
    p = GL_P if field == N.GB_GOLDILOCKS else BB_P
    rng = np.random.default_rng(SEED)
    vals = [int(rng.integers(0, p, dtype=np.uint64)) for _ in range(count)]
    return [(v << 32) % p for v in vals] if p3 and field == N.GB_BABYBEAR else vals


class _Data:
    MAX_PERM_ARG_RETRIES = 3

    def __init__(self, field):
        self.field, self.drops, self.perm_arg_retries = field, 0, None

    def drop_retry(self):
        self.drops += 1


class _Once:
    """prove once: PermArgZeroError on the first k calls, then bytes; records the hint of every call"""

    def __init__(self, k):
        self.k, self.hints = k, []

    def __call__(self, hint):
        self.hints.append(hint)
        if len(self.hints) <= self.k:
            raise N.PermArgZeroError(N.GB_ERR_PERM_ARG_ZERO, "InvZeroPermArg")
        return b"proof"


def _check(k, once, drawn, data, rng, field, p3, salted, hint, call):
    """the outcome of a loop over a front that can re-draw: k < 3 failures end in the proof, 3 in TooManyPermArgFailures"""
    if k < 3:
        assert call() == b"proof"
    else:
        with pytest.raises(N.TooManyPermArgFailuresError, match=GIVING_UP):
            call()
    attempts = min(k + 1, 3)
    assert drawn == _draws(field, p3, attempts - 1)
    assert data.perm_arg_retries == attempts - 1
    assert once.hints == [None] + [None if salted else hint] * (attempts - 1)
    assert data.drops == (1 if k == 3 else 0)          # only when the loop gives up
    # nothing else was drawn: the generator stands where `attempts - 1` draws leave an identically seeded one
    p = GL_P if field == N.GB_GOLDILOCKS else BB_P
    want = np.random.default_rng(SEED)
    for _ in range(attempts - 1):
        want.integers(0, p, dtype=np.uint64)
    assert int(rng.integers(0, 1 << 62)) == int(want.integers(0, 1 << 62))


@pytest.mark.parametrize("salted", [False, True])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("field,p3", FIELDS)
def test_shared_loop(field, p3, k, salted):
    data, once, drawn, rng = _Data(field), _Once(k), [], np.random.default_rng(SEED)
    _check(k, once, drawn, data, rng, field, p3, salted, RW,
           lambda: prove_with_retries(data, drawn.append, once, RW, rng=rng, salted=salted, p3_repr=p3))


@pytest.mark.parametrize("field,p3", FIELDS)
def test_shared_loop_with_nothing_to_redraw(field, p3):
    # no random wire: the failed attempt's state is dropped at once, then the error of the second attempt
    data, once = _Data(field), _Once(1)
    with pytest.raises(N.TooManyPermArgFailuresError, match=NO_RANDOM_WIRE):
        prove_with_retries(data, None, once, None, rng=np.random.default_rng(SEED), p3_repr=p3)
    assert (once.hints, data.drops, data.perm_arg_retries) == ([None], 1, 0)
    # a random wire that this front cannot re-draw: its own text, and nothing dropped
    data, once = _Data(field), _Once(1)
    with pytest.raises(N.TooManyPermArgFailuresError, match=NO_RANDOM_INPUT):
        prove_with_retries(data, None, once, RW, rng=np.random.default_rng(SEED), p3_repr=p3, nothing_to_redraw=NO_RANDOM_INPUT)
    assert (once.hints, data.drops, data.perm_arg_retries) == ([None], 0, 0)
    # and without a failure neither matters
    data = _Data(field)
    assert prove_with_retries(data, None, _Once(0), None) == b"proof" and data.drops == 0


# ---- the same through the three fronts that use it: stub objects, no library behind them
def _circuit_data(field, once_name, once):
    d = object.__new__(CircuitData)
    d.handle, d.field, d.drops = None, field, 0
    d.drop_retry = lambda: setattr(d, "drops", d.drops + 1)
    setattr(d, once_name, once)
    return d


class _Fronts:
    """each: (k, field, p3, salts, seed, random wire given) -> (data, once, drawn values, rng, call, hint a retry passes)"""

    @staticmethod
    def matrix(k, field, p3, salts, seed, rw=True):
        once = _Once(k)
        d = _circuit_data(field, "prove_once", lambda w, pis, salts, retry_wire, p3_repr, seed: once(retry_wire))
        drawn, rng = [], np.random.default_rng(SEED)

        class Rec(np.ndarray):   # the values land in witness[column, row]
            def __setitem__(self, key, val):
                assert key == RW
                drawn.append(int(val))
        witness = np.zeros((8, 4), dtype=np.uint64).view(Rec)
        return d, once, drawn, rng, lambda: d.prove(witness, (), random_wire=RW if rw else None, rng=rng, salts=salts, p3_repr=p3,
                                                    seed=seed), RW

    @staticmethod
    def partition(k, field, p3, salts, seed, rw=True, representative=5):
        once = _Once(k)
        d = _circuit_data(field, "prove_partition_once", lambda v, salts, retry_wire, p3_repr, seed: once(retry_wire))
        drawn, rng = [], np.random.default_rng(SEED)

        class Rec(list):
            def __setitem__(self, key, val):
                assert key == 5
                drawn.append(int(val))
        values = Rec([0] * 8)
        return d, once, drawn, rng, lambda: d.prove_partition(values, representative, RW if rw else None, rng=rng, salts=salts,
                                                              p3_repr=p3, seed=seed), RW

    @staticmethod
    def inputs(k, field, p3, salts, seed, rw=True, is_input=True):
        once = _Once(k)
        d = _circuit_data(field, "prove_inputs_once", lambda v, retry_wire, seed: once(retry_wire))
        drawn, rng = [], np.random.default_rng(SEED)

        class Rec(list):
            def __setitem__(self, key, val):
                assert key == 1
                drawn.append(int(val))
        b = object.__new__(BuiltCircuit)
        b.data, b.random_wire = d, ((RW[1], RW[0]) if rw else None)           # BuiltCircuit keeps (row, column)
        b._input_targets = [wire(0, 0), wire(RW[1], RW[0]) if is_input else wire(0, 1)]
        b.input_values = lambda pw, rng, seed: Rec([0, 0])

        class _F:
            p = GL_P if field == N.GB_GOLDILOCKS else BB_P
        b.F = _F
        return d, once, drawn, rng, lambda: b.prove_inputs(None, rng=rng, seed=seed), RW


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("field,p3", FIELDS)
@pytest.mark.parametrize("front,how", [("matrix", "plain"), ("matrix", "salts"), ("matrix", "seed"), ("partition", "plain"),
                                       ("partition", "salts"), ("partition", "seed"), ("inputs", "plain"), ("inputs", "seed")])
def test_fronts_share_the_loop(front, how, field, p3, k):
    salts = object() if how == "salts" else None
    seed = bytes(range(32)) if how == "seed" else None
    p3 = p3 and front != "inputs"     # prove_inputs takes canonical inputs: no p3 words
    d, once, drawn, rng, call, hint = getattr(_Fronts, front)(k, field, p3, salts, seed)
    _check(k, once, drawn, d, rng, field, p3, how != "plain", hint, call)


@pytest.mark.parametrize("field,p3", FIELDS)
def test_fronts_with_nothing_to_redraw(field, p3):
    for front, kw, text, drops in (("matrix", dict(rw=False), NO_RANDOM_WIRE, 1), ("partition", dict(rw=False), NO_RANDOM_WIRE, 1),
                                   ("partition", dict(representative=None), NO_RANDOM_WIRE, 0),
                                   ("inputs", dict(rw=False), NO_RANDOM_INPUT, 1), ("inputs", dict(is_input=False), NO_RANDOM_INPUT, 0)):
        d, once, drawn, rng, call, _ = getattr(_Fronts, front)(1, field, p3 and front != "inputs", None, None, **kw)
        with pytest.raises(N.TooManyPermArgFailuresError, match=text):
            call()
        assert (once.hints, drawn, d.drops, d.perm_arg_retries) == ([None], [], drops, 0), (front, kw)
