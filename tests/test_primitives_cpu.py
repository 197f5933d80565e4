"""CPU-only checks of the primitive-test machinery (tests/primitives.py): the elementwise bound and the sentinel check have teeth,
the test-only shim library loads and exports its entry points, and launch_gemm's branch selection (host code) is what
tests/test_gpu_primitives.py assumes."""
import ctypes
import os

import numpy as np
import pytest

import primitives as P
from conftest import relerr


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(P.LIB_PATH):
        from detqmc_amd.build import build
        build(verbose=False)
    return P.lib()


def test_planted_error_fails_elementwise_bound_but_passes_relerr():
    """a relative error of 1e-12 in one small entry of a product: invisible to a max-norm relerr < 1e-13, caught elementwise"""
    rng = np.random.default_rng(0)
    n = 64
    A = rng.random((n, n)) + 1j * rng.random((n, n))
    A[5] *= 1e-4                                            # row 5 of A B is four decades below the rest
    B = rng.random((n, n)) + 1j * rng.random((n, n))
    ref, rerr = P.matmul_ref(A, B)
    P.check_elementwise(ref, ref, P.elementwise_bound(A, B), rerr)
    bad = ref.copy()
    bad[5, 7] *= 1 + 1e-12
    assert relerr(bad, ref) < 1e-13
    with pytest.raises(AssertionError, match="elementwise bound exceeded at \\(5, 7\\)"):
        P.check_elementwise(bad, ref, P.elementwise_bound(A, B), rerr)


def test_exact_matmul_is_exact():
    rng = np.random.default_rng(1)
    A, B = P.int_matrix(rng, 30, 40), P.int_matrix(rng, 40, 20)
    assert np.array_equal(P.exact_matmul(A, B), (A.astype(np.clongdouble) @ B.astype(np.clongdouble)).astype(complex))


def _arena():
    ar = P.Arena(3, gap=512)
    ar.mat("A", 5, 4, 7)
    ar.mat("C", 6, 3, 8, kind="out")
    ar.vec("w", 10, np.int32, kind="scratch")
    ar.layout()
    for b in range(3):
        ar.set("A", np.arange(20).reshape(5, 4) + 1j, b)
        ar.set("C", np.zeros((6, 3)), b)
    return ar


def test_sentinel_check_reports_a_single_changed_byte():
    cases = [("gap between chains", lambda ar: ar.cs * 2 - 1, "gap"),
             ("slack row of an input", lambda ar: ar.cs + ar.ops["A"]["off"] + 16 * 5 + 3, "operand A"),
             ("slack row of an output", lambda ar: ar.ops["C"]["off"] + 16 * (8 + 6), "operand C"),
             ("input element", lambda ar: 2 * ar.cs + ar.ops["A"]["off"] + 16 * 8, "chain 2, operand A")]
    for what, where, pattern in cases:
        ar = _arena()
        ar.snapshot()
        ar.buf.view(np.uint8)[where(ar)] ^= 1
        with pytest.raises(AssertionError, match=pattern):
            ar.check()
    ar = _arena()
    ar.snapshot()
    ar.set("C", np.ones((6, 3)), 1)                         # outputs and scratch may change
    ar.fill("w", 7, 2)
    ar.check()
    ar.buf.view(np.uint8)[ar.ops["C"]["off"] + 16 * 6] ^= 1  # ... but not the slack row below C
    with pytest.raises(AssertionError, match="operand C"):
        ar.check()


def test_sentinels_are_nan():
    ar = _arena()
    gap = ar.buf.view(np.float64)[(ar.cs - 8) // 8]
    assert np.isnan(gap) and ar.buf[-1] == P.SENTINEL


def test_shim_loads_and_exports(shim):
    for name in P.SYMBOLS:
        assert hasattr(shim, name), name
    # the library resolves the launchers from libdetqmc_amd.so next to it (no second copy of the kernels)
    with open(P.LIB_PATH, "rb") as f:
        assert b"libdetqmc_amd.so" in f.read()


def test_gemm_plan_selection(shim):
    """the branches tests/test_gpu_primitives.py claims to reach, from the host-side selection shared with launch_gemm"""
    from test_gpu_primitives import TILE_CASES

    def spec(M, N, K, **kw):
        s = P.PrimGemm()
        for f, _ in P.PrimGemm._fields_:
            setattr(s, f, -1 if f in ("A", "B", "C", "Kdev", "kscale", "rowscale", "colscale", "a_kgather", "part") else 0)
        s.A, s.B, s.C, s.M, s.N, s.K = 0, 0, 0, M, N, K
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    for (M, N, K, nb), want in TILE_CASES:
        assert P.gemm_plan(spec(M, N, K), nb) == want
    assert P.gemm_plan(spec(64, 64, 2304, part=0), 1) == dict(tile=32, ksplit=8, xcd=0)       # eight M x N slices by default
    assert P.gemm_plan(spec(64, 64, 2304, part=0, part_count=32 * 64 * 64), 1)["ksplit"] == 32
    assert P.gemm_plan(spec(64, 64, 2304, part=0, part_count=3 * 64 * 64), 1)["ksplit"] == 3
    assert P.gemm_plan(spec(64, 64, 511, part=0), 1)["ksplit"] == 1
    for opt in ("Kdev", "kscale", "rowscale", "colscale"):
        assert P.gemm_plan(spec(64, 64, 2304, part=0, **{opt: 0}), 1)["ksplit"] == 1, opt
    assert P.gemm_plan(spec(64, 64, 2304, part=0, b_lower=1), 1)["ksplit"] == 1
    assert P.gemm_plan(spec(64, 64, 2304, part=0), 64)["ksplit"] == 1                         # 256 workgroups: no split
    assert P.gemm_plan(spec(1040, 1040, 64), 1)["tile"] == 64 and P.gemm_plan(spec(1040, 32, 64), 8)["tile"] == 32
