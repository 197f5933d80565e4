"""The stabilisation layer at kernel level: the UdV / UDT chain factorisations (decompose, decompose_chained: udv_dev, udt_dev and their
glue kernels) and the Green assembly from two factorisations (green_from_udv, green_from_eye: the scale-split Z and its three routes),
on synthetic factorisations with prescribed grading, against exact values from multiprecision (tests/stab_reference.py).

Bound, in every metric: the device's error against the exact value is at most 100 x the error of the plain fp64 CPU restatement of the
same operation (the yardstick, computed in the same run from the same inputs) against the exact value, and never has to be below
n_g 2^-53.  A case is admitted only where the yardstick's own error is at most 1e-9 (tests/test_stab_reference_cpu.py asserts that for
every case used here), so no device bound exceeds 1e-7.  Nothing is measured against the code under test.  Every test prints the
device / yardstick figures per metric before it asserts; the largest ratios are recorded in DESIGN.md."""
import functools

import numpy as np
import pytest

import stab_reference as sr
from conftest import relerr, relerr_blocks

pytestmark = pytest.mark.gpu

SEED = sr.SEED
L_OF = {32: 4, 72: 6, 128: 8, 200: 10}                       # n_g = 2 L^2 (O(2))
MODES = {"qr1": dict(stabilisation="qr", qrVariant=1), "qr2": dict(stabilisation="qr", qrVariant=2), "svd": dict(stabilisation="svd")}
ROUTES = {"lu": dict(stabilisation="qr"), "reflectors": dict(stabilisation="qr", greenVariant=1, qrVariant=1),
          "explicit_q": dict(stabilisation="qr", greenVariant=1, qrVariant=2), "svd": dict(stabilisation="svd")}


@functools.lru_cache(maxsize=None)
def _ctx(n, mode, nchains=1, td=False, opdim=2):
    from detqmc_amd import KernelContext
    kw = dict(MODES[mode] if mode in MODES else ROUTES[mode])
    ctx = KernelContext(opdim, L_OF[n], 4, 2, 0.1, delaySteps=4, nchains=nchains, timeDisplaced=td, tdParticleHole=td, **kw)
    assert ctx.ng == n
    if td:
        ctx.set_timedisplaced(True)
    _OPEN.append(ctx)
    return ctx


_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """the contexts are shared by the tests of this file (one per size, mode and batch) and closed when it is done"""
    yield
    while _OPEN:
        _OPEN.pop().close()
    _ctx.cache_clear()


def _fallbacks(ctx):
    return int(ctx.schedule_info().cholqr_fallbacks)


def _report(tag, dev, yard, n):
    """prints device, yardstick and ratio per metric; returns the list of metrics out of bound (or yardsticks out of admission)"""
    bad = []
    for k in sorted(dev):
        ratio = dev[k] / max(yard[k], n * sr.U64 / sr.FACTOR)
        ok = dev[k] <= sr.bound(yard[k], n) and yard[k] <= sr.ADMISSION
        print("STAB %-44s %-8s device %.2e  yardstick %.2e  ratio %7.2f  bound %.2e%s"
              % (tag, k, dev[k], yard[k], ratio, sr.bound(yard[k], n), "" if ok else "   <-- FAIL"))
        if not ok:
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------
# decompositions
# ------------------------------------------------------------------------------------------------
def _ways(case):
    """the three ways the grading enters: (name, M, colscale, rowscale, kind, exact M' in long double, exact log|det M'|)"""
    W, cs, Ms = case["W"], case["cs"], case["Ms"]
    Wh = W.conj().T.copy()
    return [("baked", Ms, None, None, 0, sr.scaled_ld(Ms), case["logdet_baked"]),
            ("colscale", W, cs, None, 0, sr.scaled_ld(W, cs=cs), case["logdet"]),
            ("rowscale_L", Wh, None, cs, 1, sr.scaled_ld(Wh, rs=cs), case["logdet"])]


def _structure(U, d, Vt, kind, mode, yard, tag):
    """what holds exactly or nearly so beyond the metrics"""
    n = len(d)
    assert np.all(np.isfinite(d)) and np.all(d > 0), tag
    if mode == "svd":
        assert np.all(np.diff(d) <= 0), tag + ": d must be descending"
        return
    T = (Vt if kind == 0 else U).conj().T                     # T = D^-1 R P^T
    Ty = (yard[2] if kind == 0 else yard[0]).conj().T
    perm, lower, diag = sr.udt_structure(T)
    assert sorted(perm.tolist()) == list(range(n)), tag
    assert lower == 0.0, tag + ": T[:, perm] must be exactly upper triangular"
    assert diag <= 8 * sr.U64, tag + ": |diag T[:, perm]| must be 1 (%.2e)" % diag
    cd, cy = np.linalg.cond(T), np.linalg.cond(Ty)
    print("STAB %-44s cond(T) device %.3f  yardstick %.3f" % (tag, cd, cy))
    assert cd <= 10 * cy, tag


def _decompose_and_check(ctx, mode, n, M, cs, rs, kind, Mp, logdet, yard, tag, sv_exact=None):
    before = _fallbacks(ctx)
    U, d, Vt, _ = ctx.decompose(M[None], None if cs is None else cs[None], None if rs is None else rs[None], kind)
    if mode == "qr2":                                         # what actually ran: Cholesky-QR2 panels, or the in-call Householder fallback
        print("STAB %-44s Householder fallbacks in this call: %d" % (tag, _fallbacks(ctx) - before))
    U, d, Vt = U[0], d[0], Vt[0]
    m = "svd" if mode == "svd" else "qr"
    dev = sr.decomposition_metrics(U, d, Vt, Mp, kind, m, logdet)
    ref = sr.decomposition_metrics(*yard, Mp, kind, m, logdet)
    if sv_exact is not None:
        dev["sv_rel"] = float(np.max(np.abs(d - sv_exact) / sv_exact))
        ref["sv_rel"] = float(np.max(np.abs(yard[1] - sv_exact) / sv_exact))
    bad = _report(tag, dev, ref, n)
    _structure(U, d, Vt, kind, mode, yard, tag)
    return bad


DECOMP_CASES = [(n, g, mode) for n in sr.DECOMP_SIZES for mode in MODES for g in sr.DECOMP_GRADINGS["svd" if mode == "svd" else "qr"]]


@pytest.mark.parametrize("n,g,mode", DECOMP_CASES)
def test_decompose_graded(n, g, mode):
    """unitarity, graded (column- resp. row-wise) residual and log-determinant of the factorisation of W diag(cs), the grading baked
    into M, given as colscale, and given as rowscale of the adjoint with the L-type factorisation; the structure of T in QR mode"""
    ctx = _ctx(n, mode)
    case = sr.decomposition_case(n, g, SEED)
    bad = []
    for name, M, cs, rs, kind, Mp, logdet in _ways(case):
        yard = sr.decomposition_yardstick(n, g, SEED, "svd" if mode == "svd" else "qr", kind)
        bad += [(name, k) for k in _decompose_and_check(ctx, mode, n, M, cs, rs, kind, Mp, logdet, yard, "decomp n=%d g=%d %s %s" % (n, g, mode, name))]
    assert not bad, bad


@pytest.mark.parametrize("g", sr.DECOMP_GRADINGS["svd"])
def test_svd_relative_accuracy(g):
    """SVD mode, n_g = 32: EVERY singular value of W diag(cs) is relatively accurate against mp.svd_c (scales as colscale, and as
    rowscale of the adjoint: the device then works on the transpose)"""
    n = 32
    ctx = _ctx(n, "svd")
    case = sr.decomposition_case(n, g, SEED)
    bad = []
    for name, M, cs, rs, kind, Mp, logdet in _ways(case)[1:]:
        yard = sr.decomposition_yardstick(n, g, SEED, "svd", kind)
        bad += _decompose_and_check(ctx, "svd", n, M, cs, rs, kind, Mp, logdet, yard, "svdrel n=32 g=%d %s" % (g, name), sv_exact=case["sv"])
    assert not bad, bad


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", ["identity", "perm_diag", "equal_norms"])
def test_decompose_ties(which, mode):
    """equal column norms (the tie-break of k_rank): M = 1, a permutation times a diagonal, two columns of equal norm; both kinds"""
    n = 32
    ctx = _ctx(n, mode)
    M = sr.tie_matrices(n)[which]
    logdet = sr.logdet_longdouble(M)
    m = "svd" if mode == "svd" else "qr"
    bad = []
    for kind in (0, 1):
        A = M if kind == 0 else M.conj().T.copy()
        yard = (sr.yardstick_udt if m == "qr" else sr.yardstick_svd)(A, kind)
        tag = "ties %s %s kind=%d" % (which, mode, kind)
        U, d, Vt, _ = ctx.decompose(A[None], kind=kind)
        dev = sr.decomposition_metrics(U[0], d[0], Vt[0], sr.scaled_ld(A), kind, m, logdet)
        ref = sr.decomposition_metrics(*yard, sr.scaled_ld(A), kind, m, logdet)
        bad += [(kind, k) for k in _report(tag, dev, ref, n)]
        if which == "equal_norms":                        # on the other two R has exact zeros: the pattern does not show perm
            _structure(U[0], d[0], Vt[0], kind, mode, yard, tag)
        else:
            assert np.all(d[0] > 0) and (m == "qr" or np.all(np.diff(d[0]) <= 0))
    assert not bad, bad


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n,g", sr.CHAINED_CASES)
def test_decompose_chained(n, g, mode):
    """decompose_chained (QR mode: k_udt_lazy and the gathered triangular product): the returned non-unitary factor is Aold times the
    new one -- U d V_t^H = M' Aold^H (R-type, column-wise) resp. Aold M' (L-type, row-wise), M' in long double.  The graded columns
    come in shuffled order here, so that the ranking permutation is neither the identity nor its own inverse"""
    ctx = _ctx(n, mode)
    m = "svd" if mode == "svd" else "qr"
    bad = []
    for name, M, cs, rs, kind, Aold in sr.chained_operands(n, g, SEED):
        Mp, Al = sr.scaled_ld(M, cs=cs, rs=rs), np.array(Aold, dtype=np.clongdouble)
        P = Mp @ Al.conj().T if kind == 0 else Al @ Mp
        yard = sr.chained_yardstick(M, cs, rs, kind, Aold, m)
        U, d, Vt, _ = ctx.decompose(M[None], None if cs is None else cs[None], None if rs is None else rs[None], kind, Aold[None])
        dev = sr.decomposition_metrics(U[0], d[0], Vt[0], Mp, kind, m, None, product=P)
        ref = sr.decomposition_metrics(*yard, Mp, kind, m, None, product=P)
        bad += [(name, k) for k in _report("chained n=%d g=%d %s %s" % (n, g, mode, name), dev, ref, n)]
        # the unchained call on the same operands gives the same unitary factor and scales
        U0, d0, V0, _ = ctx.decompose(M[None], None if cs is None else cs[None], None if rs is None else rs[None], kind)
        Q, Q0 = (U[0], U0[0]) if kind == 0 else (Vt[0], V0[0])
        assert np.array_equal(d[0], d0[0]) and np.array_equal(Q, Q0)
        if m == "qr":
            perm = sr.udt_structure((V0[0] if kind == 0 else U0[0]).conj().T)[0]
            assert not np.array_equal(perm, np.arange(n)) and not np.array_equal(perm[perm], np.arange(n)), "the case must permute"
    assert not bad, bad


@pytest.mark.parametrize("mode,nchains", [("qr1", 3), ("qr2", 3), ("svd", 3), ("qr1", 8), ("svd", 8)])
def test_decompose_batch(mode, nchains):
    """every chain its own matrix, scales and (SVD mode) orientation; every chain meets its own bound; Householder QR mode: each
    chain's output is bit for bit that of the same operands in a context of one chain"""
    n, g = 32, 8
    ctx = _ctx(n, mode, nchains)
    M, cs, rs = sr.batch_operands(n, g, nchains)
    U, d, Vt, _ = ctx.decompose(M, cs, rs, 0)
    m = "svd" if mode == "svd" else "qr"
    bad = []
    for b in range(nchains):
        Mp = sr.scaled_ld(M[b], cs=cs[b], rs=rs[b])
        yard, axis = sr.batch_yardstick(M, cs, rs, b, m)
        dev = sr.decomposition_metrics(U[b], d[b], Vt[b], Mp, 0, m, None)
        ref = sr.decomposition_metrics(*yard, Mp, 0, m, None)
        dev["res"] = sr.graded_residual(sr.product_ld(U[b], d[b], Vt[b]), Mp, axis)
        ref["res"] = sr.graded_residual(sr.product_ld(*yard), Mp, axis)
        bad += [(b, k) for k in _report("batch %s nchains=%d chain %d" % (mode, nchains, b), dev, ref, n)]
        if m == "svd":
            assert np.all(np.diff(d[b]) <= 0)
    assert not bad, bad
    if mode == "qr1" and nchains == 3:
        one = _ctx(n, mode, 1)
        for b in range(nchains):
            U1, d1, V1, _ = one.decompose(M[b][None], cs[b][None], rs[b][None], 0)
            assert np.array_equal(U1[0], U[b]) and np.array_equal(d1[0], d[b]) and np.array_equal(V1[0], Vt[b]), "chain %d" % b


# ------------------------------------------------------------------------------------------------
# Green assembly
# ------------------------------------------------------------------------------------------------
def _check_route(ctx, route):
    si = ctx.schedule_info()                                  # both flags report the QR mode's choices: 0 in SVD mode
    assert bool(si.green_lu) == (route == "lu"), route
    assert bool(si.qr_block_gram_schmidt) == (route == "explicit_q"), route


def _green_yardstick(L, R, n, route, td):
    """SVD mode: G and sv follow the reference's SVD formula, the time-displaced functions the scale-split Z"""
    y = sr.yardstick_green(L, R, n)
    if route == "svd":
        ys = sr.yardstick_green_svd(L, R, n)
        y["G"], y["logdet"] = ys["G"], ys["logdet"]
    return y if td else {"G": y["G"], "logdet": y["logdet"]}


def _green_check(ctx, route, n, cases, td, tag):
    """cases: one (L, R, exact) per chain of ctx"""
    def stack(i):
        return None if cases[0][i] is None else tuple(np.array([c[i][j] for c in cases]) for j in range(3))
    before = _fallbacks(ctx)
    out = ctx.green_from_factors(stack(0), stack(1), td=td, g0=td)
    if route == "explicit_q":                                 # a failed Cholesky-QR panel would have sent the call down the reflector route
        assert _fallbacks(ctx) == before, tag + ": the explicit-Q route fell back to Householder reflectors"
    bad = []
    for b, (L, R, exact) in enumerate(cases):
        got = {k: v[b] for k, v in out.items() if k != "sv"}
        assert np.all(out["sv"][b] > 0)
        got["logdet"] = sr.log_sum(out["sv"][b])
        dev = sr.green_errors(got, exact, n, relerr, relerr_blocks)
        ref = sr.green_errors(_green_yardstick(L, R, n, route, td), exact, n, relerr, relerr_blocks)
        assert set(dev) == set(ref)
        bad += [(b, k) for k in _report("%s chain %d" % (tag, b), dev, ref, n)]
    assert not bad, bad


GREEN_CASES = [(route, g, slots) for route in ROUTES for slots in sr.GREEN_SLOTS for g in sr.green_gradings(route, slots)]


@pytest.mark.parametrize("route,g,slots", GREEN_CASES)
def test_green_from_factors(route, g, slots):
    """G, G(tau,0), G(0,tau), G(0) (both slots) and sum log sv against the exact (1 + B_R B_L)^-1 and its products, per route"""
    n = 32
    td = slots == "both"
    ctx = _ctx(n, route, 1, td)
    _check_route(ctx, route)
    # SVD mode, one slot: greenFromEye_and_UdV takes both factors of the slot as unitary (they are, when an SVD made them)
    case = sr.green_case(n, g, SEED, slots, route == "svd" and slots != "both")
    _green_check(ctx, route, n, [case], td, "green %s g=%d %s" % (route, g, slots))


@pytest.mark.parametrize("n,g,route", sr.GOLDEN_GPU_CASES)
def test_green_larger_case_against_the_fixture(n, g, route):
    """n_g = 72 (a tail QR panel, a second block Gram-Schmidt panel, more than one LU panel), both slots, against the committed exact
    values: g = 40 on the LU and the reflector route, g = 8 on all three QR-mode routes.  The explicit-Q route does not run at g = 40:
    measured on an MI355X it gives G to 8.0e-12 and G(0,tau) to 9.3e-12 there, 133 and 119 x the yardstick, and its numpy restatement
    the same figures -- the loss is the route's (stab_reference.GOLDEN_FILES), so its grading is shrunk to the next one of the list"""
    import os
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, sr.golden_file(n, g)))
    ctx = _ctx(n, route, 1, True)
    _check_route(ctx, route)
    _green_check(ctx, route, n, [sr.golden_case(z, n, g)], True, "green n=%d g=%d %s" % (n, g, route))


def test_green_batch_mixed_grading():
    """three chains with g = 0, 40 and 120 side by side"""
    n = 32
    ctx = _ctx(n, "lu", 3, True)
    _green_check(ctx, "lu", n, [sr.green_case(n, g, SEED, "both") for g in (0, 40, 120)], True, "green batch lu")


def test_green_opdim1():
    """an O(1) context (n_g = 2 N as well, its own kernel instantiations of the B-multiply aside)"""
    n = 32
    ctx = _ctx(n, "lu", 1, False, 1)
    _green_check(ctx, "lu", n, [sr.green_case(n, 40, SEED, "both")], False, "green opdim=1 lu g=40")


def test_context_is_void_afterwards_and_recovers():
    """after either call G is stale and no advance is accepted; dqmc_udv_setup brings the context back to the G it had"""
    from detqmc_amd import KernelContext
    ctx = KernelContext(2, 4, 4, 2, 0.1, delaySteps=4, stabilisation="qr")
    try:
        rng = np.random.default_rng(3)
        ctx.set_fields(rng.standard_normal((5, 16, 2)))
        ctx.setupUdVStorage_and_calculateGreen()
        g0 = ctx.g
        L, R, _ = sr.green_case(32, 0, SEED, "both")
        ctx.green_from_factors(tuple(x[None] for x in L), tuple(x[None] for x in R))
        with pytest.raises(RuntimeError):
            ctx.g
        with pytest.raises(RuntimeError):
            ctx.advanceDownGreen(ctx.n)
        ctx.setupUdVStorage_and_calculateGreen()
        assert np.array_equal(ctx.g, g0)
        ctx.decompose(L[0][None])
        with pytest.raises(RuntimeError):
            ctx.g
        ctx.setupUdVStorage_and_calculateGreen()
        assert np.array_equal(ctx.g, g0)
    finally:
        ctx.close()
