"""gb_random_elements on the GPU (csrc/kernels_random.hip: k_random_elements) against tests/random_stream.py, both fields, host and
device destination: counts below, at and above a block, ranges that start at every position of a block and at the last lane of
a wave, several workgroups with ragged ends, 2^16 + 1 elements, the last elements the block counter reaches, nonces with every
word non-zero; the known answers through the library; two seeds one bit apart; the bytes past `count` of an over-allocated device
destination; the refusals.  -m gpu only."""
import ctypes as C

import numpy as np
import pytest

import random_stream as RS
from plonky2_goldibear_amd import GpuContext, ShapeError, random_elements
from plonky2_goldibear_amd import native as N

pytestmark = pytest.mark.gpu

FIELDS = {"goldilocks": (N.GB_GOLDILOCKS, RS.GL_P), "babybear": (N.GB_BABYBEAR, RS.BB_P)}
SEED = bytes((11 * i + 5) & 0xFF for i in range(32))
NONCE = (0xDEADBEEF, 0x00000001, 0x80000000)
COUNTS = [1, 3, 4, 5, 1023, 4 * 256 * 3 + 5, 2**16 + 1]
FIRSTS = [0, 1, 2, 3, 4 * 64 - 1]


@pytest.fixture(scope="module")
def ctx():
    c = GpuContext(0)
    yield c
    c.close()


def on_host(t, field):
    return t.cpu().numpy().view(np.uint64 if field == N.GB_GOLDILOCKS else np.uint32)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: first difference at element %d: %#x, expected %#x" % (what, bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def reference():
    """one stretch of the stream per field, computed once: every range below is a slice of it"""
    top = max(FIRSTS) + max(COUNTS)
    return {name: RS.elements(SEED, NONCE, 0, top, p) for name, (_, p) in FIELDS.items()}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_ranges_equal_the_restatement(ctx, reference, name, device):
    field, p = FIELDS[name]
    for first in FIRSTS:
        for count in COUNTS:
            got = random_elements(ctx, field, SEED, NONCE, first, count, device=device)
            got = on_host(got, field) if device else got
            assert_same(got, reference[name][first:first + count], "first %d, count %d" % (first, count))
    assert int(reference[name].max()) < p


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_the_last_elements_of_a_stream(ctx, name, device):
    field, p = FIELDS[name]
    first, count = 2**34 - 9, 9
    got = random_elements(ctx, field, SEED, NONCE, first, count, device=device)
    assert_same(on_host(got, field) if device else got, RS.elements(SEED, NONCE, first, count, p), "the last nine elements")


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_known_answers_through_the_library(ctx, name):
    field, p = FIELDS[name]
    for seed, nonce, counter, hexed in RS.KATS:
        raw = bytes.fromhex(hexed)
        want = [int.from_bytes(raw[16 * i:16 * i + 16], "little") % p for i in range(4)]
        assert [int(v) for v in random_elements(ctx, field, seed, nonce, 4 * counter, 4)] == want
    seed, nonce, _, _ = RS.KATS[0]
    assert int(random_elements(ctx, field, seed, nonce, 4, 1)[0]) == 0xc47120a31fdd0f5015593bd1e4e7f110 % p


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_one_bit_of_the_seed_changes_everything(ctx, name):
    field, p = FIELDS[name]
    other = bytes([SEED[0] ^ 1]) + SEED[1:]
    a, b = random_elements(ctx, field, SEED, NONCE, 0, 4096), random_elements(ctx, field, other, NONCE, 0, 4096)
    assert_same(b, RS.elements(other, NONCE, 0, 4096, p), "the other seed")
    # unrelated: no position agrees (4096 draws from >= 2^30 values: a coincidence has probability < 2^-18), and the differences
    # are spread over the whole range - about half of them (as integers mod p) above p / 2
    assert not (a == b).any()
    diff = (a.astype(object) - b.astype(object)) % p
    upper = sum(1 for d in diff if d > p // 2)
    assert 4096 * 0.4 < upper < 4096 * 0.6
    # and another nonce word is another stream
    for k in range(3):
        n2 = list(NONCE)
        n2[k] ^= 1
        assert not (random_elements(ctx, field, SEED, n2, 0, 256) == a[:256]).any()


@pytest.mark.parametrize("first,count", [(0, 4), (0, 5), (3, 1023), (1, 4 * 256 * 3 + 5), (8, 1024)])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_bytes_past_count_are_untouched(ctx, name, first, count):
    import torch
    field, p = FIELDS[name]
    dt = torch.int64 if field == N.GB_GOLDILOCKS else torch.int32
    pad = 64
    buf = torch.full((count + pad,), -0x5A5A5A5B, dtype=dt, device="cuda:0")
    torch.cuda.synchronize()
    lib = N.load()
    sbuf = (C.c_uint8 * 32).from_buffer_copy(SEED)
    nbuf = (C.c_uint32 * 3)(*NONCE)
    N.check(lib.gb_random_elements(ctx.handle, field, sbuf, nbuf, first, count, N.GB_INPUT_DEVICE, buf.data_ptr()), ctx.handle)
    ctx.synchronize()
    got = on_host(buf, field)
    assert_same(got[:count], RS.elements(SEED, NONCE, first, count, p), "the range")
    fill = np.array([-0x5A5A5A5B], dtype=np.int64 if field == N.GB_GOLDILOCKS else np.int32).view(got.dtype)[0]
    assert (got[count:] == fill).all()


def test_refusals(ctx):
    import torch
    lib = N.load()
    sbuf = (C.c_uint8 * 32).from_buffer_copy(SEED)
    nbuf = (C.c_uint32 * 3)(*NONCE)
    out = np.zeros(16, dtype=np.uint64)
    ok = (ctx.handle, N.GB_GOLDILOCKS, sbuf, nbuf, 0, 4, N.GB_INPUT_HOST, out.ctypes.data)

    def status(**change):
        names = ("ctx", "field", "seed", "nonce", "first", "count", "flags", "out")
        args = [change.get(k, v) for k, v in zip(names, ok)]
        return lib.gb_random_elements(*args)

    assert status() == N.GB_OK and [int(v) for v in out[:4]] == [int(v) for v in RS.elements(SEED, NONCE, 0, 4, RS.GL_P)]
    assert status(seed=None) == N.GB_ERR_INVALID
    assert status(nonce=None) == N.GB_ERR_INVALID
    assert status(out=None) == N.GB_ERR_INVALID
    assert status(field=2) == N.GB_ERR_INVALID
    assert status(flags=N.GB_INPUT_P3_REPR) == N.GB_ERR_INVALID and status(flags=N.GB_SALTS_FROM_SEED) == N.GB_ERR_INVALID
    assert status(first=2**34 - 6, count=6) == N.GB_OK
    assert status(first=2**34 - 6, count=7) == N.GB_ERR_INVALID          # its last block index would be 2^32
    assert status(first=2**34, count=1) == N.GB_ERR_INVALID
    assert status(first=2**64 - 1, count=2) == N.GB_ERR_INVALID          # first + count wraps
    assert status(first=2**34, count=0) == N.GB_OK
    dev = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    assert status(flags=N.GB_INPUT_DEVICE, out=dev.data_ptr() + 8) == N.GB_ERR_INVALID   # not 16-byte aligned
    assert status(flags=N.GB_INPUT_DEVICE, out=dev.data_ptr()) == N.GB_OK
    with pytest.raises(ShapeError, match="2\\^34"):
        random_elements(ctx, N.GB_BABYBEAR, SEED, NONCE, 2**34 - 6, 7)
    with pytest.raises(ShapeError, match="32 bytes"):
        random_elements(ctx, N.GB_BABYBEAR, SEED[:31], NONCE, 0, 4)
    with pytest.raises(ShapeError, match="field"):
        random_elements(ctx, 2, SEED, NONCE, 0, 4)
    # the context still works
    assert [int(v) for v in random_elements(ctx, N.GB_BABYBEAR, SEED, NONCE, 0, 4)] == [int(v) for v in RS.elements(SEED, NONCE, 0, 4, RS.BB_P)]
