"""The whole-tile path of the complex GEMM (k_zgemm, FULL: no bounds work, operands requested two k-steps ahead) against the generic
kernel and against exact references, through the test-only entry dqmc_prim_gemm_path, which forces one path or the other for the same
arguments and reports the one that ran.

The whole-tile path issues the same MFMAs on the same operands in the same order as the generic kernel, so for ANY operands C must be
bit-identical between the two (np.array_equal); integer operands against int64 arithmetic catch a mistake both paths would share.
K = 16 ... 80 is one to five k-steps: the prologue alone, both register sets, both parities of the LDS buffer, the pair loop and both
tails behind it.  Arena.check() runs after every launch: nothing outside C is written."""
import ctypes

import numpy as np
import pytest

import primitives as P
from test_gpu_primitives import _built, _gemm_case, _gemm_expected_exact, _gemm_operands  # noqa: F401  (_built: module fixture)

pytestmark = pytest.mark.gpu

GENERIC, FULL = 0, 1
OPS = [(0, 0), (0, 1), (1, 0), (1, 1)]
KS = (16, 32, 48, 64, 80)
# (M = N, chains, tile, XCD-grouped grid): 64-tile kernel on both grid layouts (>= 256 tiles of 64 x 64), 32-tile kernel
SHAPES = {"t64_xcd": (256, 16, 64, 1), "t64_gridz": (256, 17, 64, 0), "t32": (64, 8, 32, 1)}


def run_path(ar, spec, path):
    fn = P.lib().dqmc_prim_gemm_path
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(P.PrimGemm), ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    ran = ctypes.c_int(-1)
    rc, msg = ar.call("dqmc_prim_gemm_path", ctypes.byref(spec), path, ctypes.byref(ran))
    assert rc == 0, msg
    ar.check()
    return ran.value


def both_paths(ar, spec, nb, what):
    """the same arena through the generic kernel and through the whole-tile path; returns C per chain of the whole-tile run"""
    before = ar.buf.copy()
    assert run_path(ar, spec, GENERIC) == GENERIC, what
    ref = [ar.get("C", b) for b in range(nb)]
    ar.buf[...] = before
    assert run_path(ar, spec, FULL) == FULL, what + ": the whole-tile path was refused"
    got = [ar.get("C", b) for b in range(nb)]
    for b in range(nb):
        assert np.array_equal(got[b], ref[b]), "%s chain %d: %d entries differ, max |diff| %.3e" % (
            what, b, int(np.sum(got[b] != ref[b])), np.max(np.abs(got[b] - ref[b])))
    return got


def check_plan(spec, nb, tile, xcd):
    plan = P.gemm_plan(spec, nb)
    assert (plan["tile"], plan["ksplit"], plan["xcd"]) == (tile, 1, xcd), plan


@pytest.mark.parametrize("opA,opB", OPS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fullpath_bit_identical(shape, opA, opB):
    n, nb, tile, xcd = SHAPES[shape]
    for K in KS:
        ar, spec, ins = _gemm_case(n, n, K, nb, opA, opB, data="rand", seed=K + 7 * opA + 3 * opB)
        check_plan(spec, nb, tile, xcd)
        both_paths(ar, spec, nb, "%s K %d op %d%d" % (shape, K, opA, opB))


EPILOGUES = {"scales": dict(rowscale=1, colscale=1), "scales_acc": dict(rowscale=1, colscale=1, accumulate=1), "negate": dict(negate=1)}


@pytest.mark.parametrize("name", sorted(EPILOGUES))
@pytest.mark.parametrize("shape", ["t64_xcd", "t32"])
def test_fullpath_epilogues_bit_identical(shape, name):
    n, nb, tile, xcd = SHAPES[shape]
    ar, spec, ins = _gemm_case(n, n, 48, nb, 1, 0, opts=EPILOGUES[name], data="rand", seed=11)
    check_plan(spec, nb, tile, xcd)
    both_paths(ar, spec, nb, shape + " " + name)


# lower-triangular op(B): the k loop of a column tile starts at its first column (kbeg != 0 for all but the first column of tiles).
# (shape, K - N, gathered A): the chained factor of a stabilisation step is gather + lower + colscale at K = N; lower alone and a
# contraction longer than N (rows below the triangle are dense) are the other ways into the same code
LOWER = [("t64_xcd", 0, 1), ("t32", 0, 1), ("t64_xcd", 0, 0), ("t32", 0, 0), ("t64_xcd", 64, 0), ("t32", 32, 1)]


def _lower_case(shape, extra, gather, data, seed):
    n, nb, tile, xcd = SHAPES[shape]
    opts = dict(b_lower=1, colscale=1)
    if gather:
        opts["a_kgather"] = 1
    ar, spec, ins = _gemm_case(n, n, n + extra, nb, 0, 1, opts=opts, data=data, seed=seed)
    check_plan(spec, nb, tile, xcd)
    return nb, opts, ar, spec, ins


@pytest.mark.parametrize("shape,extra,gather", LOWER)
def test_fullpath_lower_bit_identical(shape, extra, gather):
    nb, opts, ar, spec, ins = _lower_case(shape, extra, gather, "rand", 5)
    what = "%s lower K = N + %d gather %d" % (shape, extra, gather)
    got = both_paths(ar, spec, nb, what)
    for b in (0, nb - 1):
        Aop, Bop = _gemm_operands(ins[b], spec, opts)
        ref, ref_err = P.matmul_ref(Aop, Bop)
        cs = ins[b]["colscale"][None, :]
        P.check_elementwise(got[b], ref * cs, P.elementwise_bound(Aop, Bop) * cs, ref_err * cs, "%s chain %d" % (what, b))


@pytest.mark.parametrize("shape,extra,gather", LOWER)
def test_fullpath_lower_exact(shape, extra, gather):
    nb, opts, ar, spec, ins = _lower_case(shape, extra, gather, "int", 9)
    assert run_path(ar, spec, FULL) == FULL
    for b, d in enumerate(ins):
        assert np.array_equal(ar.get("C", b), _gemm_expected_exact(d, spec, opts)), "chain %d" % b


@pytest.mark.parametrize("opA,opB", OPS)
@pytest.mark.parametrize("shape", ["t64_gridz", "t32"])
def test_fullpath_exact(shape, opA, opB):
    """integer operands: every product and sum is exact in fp64, so C equals the int64 reference bit for bit"""
    n, nb, tile, xcd = SHAPES[shape]
    ar, spec, ins = _gemm_case(n, n, 80, nb, opA, opB, data="int", seed=3 + opA + 2 * opB)
    check_plan(spec, nb, tile, xcd)
    assert run_path(ar, spec, FULL) == FULL
    for b, d in enumerate(ins):
        assert np.array_equal(ar.get("C", b), _gemm_expected_exact(d, spec, {})), "chain %d" % b


@pytest.mark.parametrize("M,K", [(250, 64), (256, 40), (250, 40)])
def test_routing_ragged_goes_generic(M, K):
    """a ragged M or a K that is no multiple of 16: the whole-tile path is refused, the generic kernel computes the product"""
    nb, N = 16, 256
    ar, spec, ins = _gemm_case(M, N, K, nb, 0, 1, data="rand", seed=M + K)
    assert run_path(ar, spec, FULL) == GENERIC
    for b in (0, nb - 1):
        Aop, Bop = _gemm_operands(ins[b], spec, {})
        ref, ref_err = P.matmul_ref(Aop, Bop)
        P.check_elementwise(ar.get("C", b), ref, P.elementwise_bound(Aop, Bop), ref_err, "M %d K %d chain %d" % (M, K, b))


@pytest.mark.parametrize("name", ["Kdev", "kscale", "split_k", "tagged_gather"])
def test_routing_options_go_generic(name):
    """a contraction length read on the device, a k-scale, split-K or a gathered A inside a factorisation (tag; there is no such
    whole-tile kernel): the generic kernel, whatever path is asked for"""
    if name == "split_k":
        M, K, nb, opts = 64, 512, 8, dict(part=64 * 64 * 8)
    elif name == "tagged_gather":
        M, K, nb, opts = 256, 64, 16, dict(a_kgather=1, tag=1)
    else:
        M, K, nb, opts = 256, 64, 16, (dict(Kdev=48) if name == "Kdev" else dict(kscale=1))
    ar, spec, ins = _gemm_case(M, M, K, nb, 0, 0, opts=opts, data="int", seed=2)
    if name == "split_k":
        assert P.gemm_plan(spec, nb)["ksplit"] > 1
    assert run_path(ar, spec, FULL) == GENERIC
    for b, d in enumerate(ins):
        assert np.array_equal(ar.get("C", b), _gemm_expected_exact(d, spec, opts)), "chain %d" % b
