"""RngStream after the move to bulk generation (csrc/host/dsfmt19937.cpp): peek fills its buffer a generator block (382 doubles) at a
time and drops the consumed front in large pieces.  The stream must stay the reference's, position by position, for every
interleaving of rand01 / peek / consume / serialize -> deserialize.  detsdw_rng_replay drives one RngStream through a script and
returns every draw it showed at its stream position; the result must equal detsdw_rng_fill (single draws only) and the Python
restatement of the generator (oracle/dsfmt_oracle.py) exactly.  Host only."""
import ctypes as C
import os

import numpy as np
import pytest

R, P, CN, RT = 0, 1, 2, 3          # DETSDW_RNG_RAND01, _PEEK, _CONSUME, _ROUNDTRIP (include/detsdw_host.h)
BLOCK = 382                        # doubles per gen_rand_all of dSFMT-19937


@pytest.fixture(scope="module")
def lib():
    import detqmc_amd
    if not os.path.exists(detqmc_amd.LIB_PATH):
        from detqmc_amd.build import build
        build(verbose=False)
    return detqmc_amd.load()


def _replay(lib, seed, pidx, script, cap):
    op = np.array([s[0] for s in script], dtype=np.int32)
    arg = np.array([s[1] for s in script], dtype=np.uint64)
    out = np.full(cap, np.nan)
    nout = C.c_size_t(0)
    rc = lib.detsdw_rng_replay(seed, pidx, op.ctypes.data_as(C.POINTER(C.c_int32)), arg.ctypes.data_as(C.POINTER(C.c_uint64)), len(script),
                               out.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(nout))
    return rc, out[:nout.value]


def _fill(lib, seed, pidx, n):
    out = np.zeros(n)
    assert lib.detsdw_rng_fill(seed, pidx, out.ctypes.data_as(C.POINTER(C.c_double)), n) == 0
    return out


def _walk(script):
    """(final stream position, highest position shown) of a script; asserts that every consume stays inside what a peek showed"""
    pos = shown = high = 0
    for op, a in script:
        if op == R:
            pos += a
            shown = max(0, shown - a)
        elif op == P:
            shown = max(shown, a)
        elif op == CN:
            assert a <= shown, "test script consumes what no peek has shown"
            pos += a
            shown -= a
        high = max(high, pos + shown)
    return pos, high


# every case the bulk path can get wrong: a peek that starts inside a partly used generator block (odd and even counts of single
# draws before it), peek sizes 1, 381, 382, 383 and 2 * 382 + 1 around the block, consume(0), consume of the whole buffer, single
# draws served from the buffer, a serialize round trip with a half-consumed buffer and one with an empty one
SCRIPT_BLOCKS = [
    (R, 3), (P, 1), (CN, 1),                       # peek after an odd number of rand01
    (P, BLOCK - 1), (CN, 0), (CN, BLOCK - 1),      # consume(0), then the whole buffer
    (P, BLOCK), (R, 5), (CN, BLOCK - 5),           # single draws out of the buffer, then the rest of it
    (R, 1), (P, BLOCK + 1), (CN, 100),
    (RT, 0),                                       # 283 buffered draws travel through serialize
    (R, 7), (P, 2 * BLOCK + 1), (CN, 2 * BLOCK + 1),
    (R, 2), (P, 2 * BLOCK + 1), (CN, BLOCK), (P, 1), (CN, 1),
    (RT, 0), (P, 1000), (CN, 383), (P, 1), (R, 1), (P, BLOCK), (CN, BLOCK),
    (RT, 0),                                       # ... and the rest of the 1000, shown but not consumed
    (R, BLOCK + 1),
    (RT, 0), (R, 4), (P, BLOCK), (CN, BLOCK), (RT, 0), (R, 3),      # empty buffer through serialize
]


def _sweeps(need, consumed, host_draws):
    """the look-ahead schedule of the sweeps: push one window, then per sweep peek two windows, consume a prefix, a few host draws"""
    s = [(P, need)]
    for c, h in zip(consumed, host_draws):
        s += [(P, 2 * need), (CN, c), (R, h)]
    return s


SCRIPT_SWEEPS = _sweeps(500, [350, 0, 500, 381, 382, 383, 499, 1], [0, 3, 0, 1, 501, 0, 2, 0])


@pytest.mark.parametrize("seed,pidx", [(1020304050, 1), (7, 4)])
@pytest.mark.parametrize("script", [SCRIPT_BLOCKS, SCRIPT_SWEEPS], ids=["blocks", "sweeps"])
def test_replay_equals_single_draws_and_oracle(lib, script, seed, pidx):
    from dsfmt_oracle import RngWrapper
    _, high = _walk(script)
    rc, got = _replay(lib, seed, pidx, script, high + 8)
    assert rc == 0
    assert got.size == high and not np.isnan(got).any(), "every position up to the last one shown must have been seen"
    assert np.array_equal(got, _fill(lib, seed, pidx, high))
    ref = RngWrapper(seed, pidx)
    assert np.array_equal(got, np.array([ref.rand01() for _ in range(high)]))


def test_roundtrip_keeps_the_position(lib):
    """the draw count and the buffered draws survive serialize -> deserialize: the positions reported after it continue the stream"""
    script = [(R, 11), (P, 600), (CN, 300), (RT, 0), (R, 1), (P, 10)]
    rc, got = _replay(lib, 5, 2, script, 2000)
    assert rc == 0 and got.size == 11 + 600
    assert np.array_equal(got, _fill(lib, 5, 2, got.size))


def test_replay_refuses_bad_scripts(lib):
    assert _replay(lib, 1, 1, [(P, 10), (CN, 11)], 100)[0] == -1       # consume past the peek
    assert _replay(lib, 1, 1, [(R, 101)], 100)[0] == -1                # position beyond the output
    assert _replay(lib, 1, 1, [(9, 0)], 100)[0] == -1                  # unknown op
