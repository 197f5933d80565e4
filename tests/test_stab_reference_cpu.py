"""tests/stab_reference.py against itself and against plain numpy (no GPU): the exact values do not depend on the working precision,
reduce to numpy and to td_reference where those are accurate, and every case of tests/test_gpu_stabilisation.py meets the admission
condition -- the fp64 yardstick's own error against the exact value is at most 1e-9 in every metric, so no device bound (100 x the
yardstick's error) exceeds 1e-7.  The yardstick table is printed (pytest -s shows it)."""
import mpmath as mp
import numpy as np
import pytest

import stab_reference as sr
from conftest import relerr, relerr_blocks

N = sr.GREEN_N


@pytest.mark.parametrize("g", [0, 120])
def test_exact_values_do_not_depend_on_the_precision(g):
    """precision p = 14 g + 200 bits and 2 p agree to 1e-25, relative to the largest entry of each matrix"""
    L, R = sr.slot_pair(N, g, sr.SEED)
    p = sr.precision_bits(g)
    a, b = sr.exact_green_mp(L, R, N, p), sr.exact_green_mp(L, R, N, 2 * p)
    with mp.workprec(2 * p):
        for x, y in zip(a[:4], b[:4]):
            scale = max(abs(y[i, j]) for i in range(N) for j in range(N))
            worst = max(abs(x[i, j] - y[i, j]) for i in range(N) for j in range(N)) / scale
            assert worst < mp.mpf("1e-25"), mp.nstr(worst, 5)
        assert abs(a[4] - b[4]) < mp.mpf("1e-25") * max(1, abs(b[4]))
    if g == 0:
        W, cs = sr.graded_input(N, 40, sr.SEED)
        with mp.workprec(2 * sr.precision_bits(40)):
            hi = mp.log(abs(mp.det(sr.to_mp(W) * sr.to_mp(cs))))
            assert abs(mp.mpf(str(sr.exact_logdet_mp(W, cs, 40))) - hi) < 1e-17 * abs(hi)      # the long double it is returned as


def test_ungraded_values_agree_with_numpy():
    L, R = sr.slot_pair(N, 0, sr.SEED)
    for slots, (l, r) in {"both": (L, R), "R": (None, R), "L": (L, None)}.items():
        ex = sr.exact_green(l, r, N, 0)
        BL = np.eye(N) if l is None else (l[0] * l[1]) @ l[2].conj().T
        BR = np.eye(N) if r is None else (r[0] * r[1]) @ r[2].conj().T
        G = np.linalg.inv(np.eye(N) + BR @ BL)
        for k, v in {"G": G, "GT0": G @ BR, "G0T": -BL @ G, "G00": np.eye(N) - BL @ G @ BR}.items():
            assert relerr(v, ex[k]) < 1e-12, (slots, k)
        assert abs(float(ex["logdet"]) - np.linalg.slogdet(np.eye(N) + BR @ BL)[1]) < 1e-12 * N
    W, cs = sr.graded_input(N, 0, sr.SEED)
    case = sr.decomposition_case(N, 0, sr.SEED)
    assert relerr(np.linalg.svd(W * cs, compute_uv=False), case["sv"]) < 1e-12
    assert abs(float(case["logdet"]) - np.linalg.slogdet(W * cs)[1]) < 1e-12 * N
    assert abs(float(sr.logdet_longdouble(W, cs) - case["logdet"])) < 1e-15 * N


def test_conventions_agree_with_td_reference_at_beta_2():
    """B_R = B(tau,0), B_L = B(beta,tau) of a physical chain at beta = 2, factorised by LAPACK: the exact values are td_reference's
    direct inverses (which are accurate there), signs and ordering included"""
    from td_reference import Chain, make_oracle
    opdim, Lx, m, tau = 2, 4, 20, 10
    rng = np.random.default_rng(5)
    ora = make_oracle(rng.standard_normal((m + 1, Lx * Lx, opdim)), opdim=opdim, L=Lx, beta=m * 0.1, dtau=0.1, s=5, delaySteps=4)
    chain = Chain(ora)
    n = ora.ng
    assert n == N
    g, gt0, g0t = chain.greens(tau)

    def slot(B):
        U, d, Vh = np.linalg.svd(B)
        return U, d, Vh.conj().T
    ex = sr.exact_green(slot(chain.B(m, tau)), slot(chain.B(tau, 0)), n, 2)
    assert relerr(ex["G"], g) < 1e-10 and relerr(ex["GT0"], gt0) < 1e-10 and relerr(ex["G0T"], g0t) < 1e-10
    g00 = np.linalg.inv(np.eye(n) + chain.B(m, tau) @ chain.B(tau, 0))          # G(0) of the same configuration
    assert relerr(ex["G00"], g00) < 1e-10


def _table(tag, err):
    print("YARD %-40s %s" % (tag, "  ".join("%s %.1e" % kv for kv in sorted(err.items()))))
    bad = {k: v for k, v in err.items() if not v <= sr.ADMISSION}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("mode", ["qr", "svd"])
@pytest.mark.parametrize("slots", sr.GREEN_SLOTS)
def test_admission_green(mode, slots):
    for g in sr.GREEN_GRADINGS[mode]:
        L, R, ex = sr.green_case(N, g, sr.SEED, slots, mode == "svd" and slots != "both")
        y = sr.yardstick_green(L, R, N)
        if mode == "svd":
            y.update(sr.yardstick_green_svd(L, R, N))
        _table("green %s g=%d %s" % (mode, g, slots), sr.green_errors(y, ex, N, relerr, relerr_blocks))


def _route_ratio(L, R, ex, n, explicit_q=False):
    y = sr.green_errors(sr.yardstick_green(L, R, n), ex, n, relerr, relerr_blocks)
    q = sr.green_qr_route_restated(L, R, n, explicit_q)
    cond = q.pop("condZ")
    e = sr.green_errors(q, ex, n, relerr, relerr_blocks)
    return max(e[k] / max(y[k], n * sr.U64 / sr.FACTOR) for k in e), cond


@pytest.mark.parametrize("slots", sr.GREEN_SLOTS)
def test_qr_route_cases_are_those_the_route_itself_can_meet(slots):
    """the plain numpy restatement of the QR routes stays within 100 x the yardstick on every case the QR routes are tested on, and
    does not on the case left to the LU route alone (g = 120, both slots: cond Z = 2e5)"""
    for g in sr.GREEN_GRADINGS["qr"]:
        L, R, ex = sr.green_case(N, g, sr.SEED, slots)
        used = g in sr.green_gradings("reflectors", slots)
        for explicit_q in (False, True):
            ratio, cond = _route_ratio(L, R, ex, N, explicit_q)
            print("YARD qr route restated (%s) g=%d %s: cond Z %.1e, worst error / yardstick %.1f, %s"
                  % ("Cholesky-QR2 Q" if explicit_q else "Householder", g, slots, cond, ratio, "used" if used else "LU route only"))
            assert (ratio <= sr.FACTOR) == used
        assert sr.green_gradings("lu", slots) == sr.GREEN_GRADINGS["qr"] and sr.green_gradings("explicit_q", slots) == sr.green_gradings("reflectors", slots)


def test_fixtures_have_not_drifted():
    """the committed exact values: the n_g = 32, g = 40 case regenerated from its stored inputs by the code path that wrote the file is
    the file's bit for bit; the stored inputs of every case carry their checksum and are the generator's up to rounding; every case
    the GPU file runs from a fixture meets the admission condition, and the restatement of its route stays within 100 x the yardstick"""
    import os
    from conftest import GOLDEN
    files = {name: np.load(os.path.join(GOLDEN, name)) for name in sr.GOLDEN_FILES}
    for name in files:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 2 ** 20
    z = files[sr.golden_file(32, 40)]
    Ls, Rs, _ = sr.golden_case(z, 32, 40)
    for k, v in sr.golden_payload(32, 40, inputs=(Ls, Rs)).items():      # multiprecision: the same bits on every machine
        assert np.array_equal(v, z[k]), k
    for n, g, route in sr.GOLDEN_GPU_CASES:
        L, R, ex = sr.golden_case(files[sr.golden_file(n, g)], n, g)
        _table("green n=%d g=%d both (fixture)" % (n, g), sr.green_errors(sr.yardstick_green(L, R, n), ex, n, relerr, relerr_blocks))
        if route != "lu":
            ratio, cond = _route_ratio(L, R, ex, n, route == "explicit_q")
            print("YARD qr route restated (%s) n=%d g=%d: cond Z %.1e, worst error / yardstick %.1f" % (route, n, g, cond, ratio))
            assert ratio <= sr.FACTOR
    # for the record, not asserted (it sits at the bound): the explicit-Q restatement on the case that route is spared
    L, R, ex = sr.golden_case(files[sr.golden_file(72, 40)], 72, 40)
    print("YARD qr route restated (explicit_q) n=72 g=40, not run on the device: worst error / yardstick %.1f" % _route_ratio(L, R, ex, 72, True)[0])


def test_long_double_logdet_agrees_with_mp_det_at_72():
    """log|det M'| comes from mp.det at n_g = 32 and from a long-double LU above: the two agree at n_g = 72, g = 40 to a small
    fraction of the smallest bound the value is used with (n_g 2^-53 per n_g)"""
    n, g = 72, 40
    W, cs = sr.graded_input(n, g, sr.SEED)
    err = float(abs(sr.logdet_longdouble(W, cs) - sr.exact_logdet_mp(W, cs, g))) / n
    print("YARD logdet long double vs mp.det n=72 g=40: %.1e per n_g" % err)
    assert err < 0.01 * sr.U64


def test_svd_formula_with_lapack_fails_beyond_g_3():
    """why SVD-mode assembly is tested at g in {0, 2} only: the reference's own formula with LAPACK loses G on these inputs"""
    L, R, ex = sr.green_case(N, 8, sr.SEED, "both")
    err = relerr(sr.yardstick_green_svd(L, R, N)["G"], ex["G"])
    print("YARD svd formula g=8: relerr of G %.1e" % err)
    assert err > 1e-6


@pytest.mark.parametrize("mode", ["qr", "svd"])
@pytest.mark.parametrize("n", sr.DECOMP_SIZES)
def test_admission_decompositions(n, mode):
    for g in sr.DECOMP_GRADINGS[mode]:
        case = sr.decomposition_case(n, g, sr.SEED)
        Mp = sr.scaled_ld(case["W"], cs=case["cs"])
        for kind in (0, 1):
            yard = sr.decomposition_yardstick(n, g, sr.SEED, mode, kind)
            err = sr.decomposition_metrics(*yard, Mp if kind == 0 else Mp.conj().T, kind, mode, case["logdet"])
            if mode == "svd" and case["sv"] is not None:
                err["sv_rel"] = float(np.max(np.abs(yard[1] - case["sv"]) / case["sv"]))
            if mode == "qr":
                T = (yard[2] if kind == 0 else yard[0]).conj().T
                perm, lower, diag = sr.udt_structure(T)
                assert lower == 0.0 and diag <= 4 * sr.U64
                print("YARD decomp n=%d g=%d kind=%d cond(T) %.3f" % (n, g, kind, np.linalg.cond(T)))
            _table("decomp %s n=%d g=%d kind=%d" % (mode, n, g, kind), err)
    for (nc, gc) in sr.CHAINED_CASES:
        if nc != n:
            continue
        for name, M, cs, rs, kind, Aold in sr.chained_operands(n, gc, sr.SEED):
            Mp, Al = sr.scaled_ld(M, cs=cs, rs=rs), np.array(Aold, dtype=np.clongdouble)
            yard = sr.chained_yardstick(M, cs, rs, kind, Aold, mode)
            err = sr.decomposition_metrics(*yard, Mp, kind, mode, None, product=Mp @ Al.conj().T if kind == 0 else Al @ Mp)
            _table("chained %s n=%d g=%d %s" % (mode, n, gc, name), err)
            if mode == "qr":                                   # the point of the shuffle: a ranking permutation that is no involution
                plain = sr.yardstick_udt(np.asarray(Mp, dtype=complex), kind)
                perm = sr.udt_structure((plain[2] if kind == 0 else plain[0]).conj().T)[0]
                assert not np.array_equal(perm[perm], np.arange(n))


@pytest.mark.parametrize("mode", ["qr", "svd"])
def test_admission_ties_and_batches(mode):
    """the remaining operands of the GPU file: the tie matrices (both kinds) and the batches of 3 and 8 chains"""
    n = 32
    for which, M in sr.tie_matrices(n).items():
        logdet = sr.logdet_longdouble(M)
        for kind in (0, 1):
            A = M if kind == 0 else M.conj().T.copy()
            yard = (sr.yardstick_udt if mode == "qr" else sr.yardstick_svd)(A, kind)
            _table("ties %s %s kind=%d" % (which, mode, kind), sr.decomposition_metrics(*yard, sr.scaled_ld(A), kind, mode, logdet))
    M, cs, rs = sr.batch_operands(n, 8, 8)
    for b in range(8):
        Mp = sr.scaled_ld(M[b], cs=cs[b], rs=rs[b])
        yard, axis = sr.batch_yardstick(M, cs, rs, b, mode)
        err = sr.decomposition_metrics(*yard, Mp, 0, mode, None)
        err["res"] = sr.graded_residual(sr.product_ld(*yard), Mp, axis)
        _table("batch %s chain %d" % (mode, b), err)
