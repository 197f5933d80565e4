"""Anchors tests/model_reference.py (the long-double reference the GPU model-kernel tests compare with) to the committed goldens
of the real reference and to the CPU oracle, so that it cannot drift together with the kernels.  CPU only."""
import math

import numpy as np
import pytest

from conftest import load_golden, oracle_params, relerr
from detsdw_oracle import DetSDWOracle, SDWParams, make_test_matrix
import model_reference as mr
from model_reference import LEFT, RIGHT, ModelReference, bmult_c, check_bound, shift_c

GOLD = ["o2_L4", "o2_L4_s7", "o2_L4_flux", "o2_L4_apbc", "o1_L4", "o3_L4", "o2_L6_seed", "o2_L8_b5", "o2_L8_flux",
        "o2_L8_apbc_flux", "o2_L4_dense", "o2_L4_dense_flux"]


def _pars_kw(op):
    return dict(opdim=op.opdim, L=op.L, beta=op.beta, dtau=op.dtau, s=op.s, lambda_=op.lambda_, txhor=op.txhor, txver=op.txver,
                tyhor=op.tyhor, tyver=op.tyver, mu=op.mu, mux=op.mux, muy=op.muy, bc=op.bc, weakZflux=op.weakZflux,
                checkerboard=op.checkerboard, cdwU=op.cdwU, r=op.r, c=op.c, u=op.u, phi2bosons=op.phi2bosons,
                delaySteps=op.delaySteps)


def _c(ref, nslices, cdw=False):
    if ref.p.checkerboard:
        return bmult_c(ref.MSF, nslices, cdw)
    return nslices * (mr.dense_c(ref.N, 1) + 4 * (ref.MSF + 2) + 2)


@pytest.mark.parametrize("name", GOLD)
def test_apply_B_vs_golden(name):
    """the real reference's single-slice and chain products of make_test_matrix at the fixture's own field"""
    g = load_golden(name)
    op = oracle_params(g["params"])
    ref = ModelReference(mr.make_lattice(**_pars_kw(op)))
    phi = np.transpose(g["init_phi"], (2, 0, 1))
    A = make_test_matrix(ref.ng)
    k = int(g["bmult_k"][0])
    ch, sh = ref.cosh_sinh(phi)
    if "init_coshTermPhi" in g:
        # the reference's own fp64 caches: cosh and sinh / |phi| of an argument with three roundings (sum of squares, sqrt, two
        # products) and a libm call each: a handful of u
        assert np.max(np.abs(ch[1:].astype(float) - g["init_coshTermPhi"].T[1:]) / g["init_coshTermPhi"].T[1:]) < 16 * mr.U
        assert np.max(np.abs(sh[1:].astype(float) - g["init_sinhTermPhi"].T[1:]) / g["init_sinhTermPhi"].T[1:]) < 16 * mr.U
    cases = [("bmult_left", LEFT, 0, k, k - 1), ("bmult_right", RIGHT, 0, k, k - 1)]
    if "bmult_leftinv" in g:
        cases += [("bmult_leftinv", LEFT, 1, k, k - 1), ("bmult_rightinv", RIGHT, 1, k, k - 1)]
    if "bchain_left" in g:
        k2 = int(g["bchain_k2"][0])
        cases += [("bchain_left", LEFT, 0, k2, 0), ("bchain_leftinv", LEFT, 1, k2, 0), ("bchain_right", RIGHT, 0, k2, 0),
                  ("bchain_rightinv", RIGHT, 1, k2, 0)]
    for key, side, inv, kk2, kk1 in cases:
        val, comp = ref.apply_B(A, side, inv, kk2, kk1, phi)
        check_bound(g[key], val, comp, _c(ref, kk2 - kk1), what=f"{name} {key}")
    if "bdense_k" in g and not op.checkerboard:
        val, comp = ref.apply_B(np.eye(ref.ng), LEFT, 0, k, k - 1, phi)
        check_bound(g["bdense_k"], val, comp, _c(ref, 1), what=f"{name} bdense_k")


CASES = [
    dict(opdim=2, L=4), dict(opdim=2, L=6, bc="apbc-x", mux=-0.3, muy=0.7, txhor=-1.1, txver=-0.4, tyhor=0.6, tyver=0.9),
    dict(opdim=2, L=6, weakZflux=True, bc="apbc-xy"), dict(opdim=1, L=4, mux=0.2, muy=-0.6), dict(opdim=3, L=4, bc="apbc-y"),
    dict(opdim=3, L=6, mux=-0.3, muy=0.7), dict(opdim=2, L=4, cdwU=0.7), dict(opdim=3, L=4, cdwU=0.5),
    dict(opdim=2, L=4, checkerboard=False), dict(opdim=2, L=4, checkerboard=False, weakZflux=True),
    dict(opdim=3, L=4, checkerboard=False, txhor=0.0, txver=0.0, tyhor=0.0, tyver=0.0, mux=-0.3, muy=0.7),     # the reference's scalar short cut
]
IDS = ["-".join(f"{k}{v}" for k, v in c.items()) for c in CASES]


def _random_case(kw, seed):
    kw = dict(beta=0.4, dtau=0.1, s=2, delaySteps=4, **kw)
    op = SDWParams(**kw).finalize()
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-1.5, 1.5, (op.m + 1, op.N, op.opdim))
    phi[0] = 0.0
    cdwl = rng.choice([-2, -1, 1, 2], (op.m + 1, op.N)).astype(np.int32)
    ora = DetSDWOracle(SDWParams(**kw).finalize(), phi=phi, cdwl=cdwl)
    ref = ModelReference(mr.make_lattice(**kw))
    n = ref.ng
    A = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * np.exp(rng.uniform(-3, 3, (n, 1))) \
        * np.exp(rng.uniform(-3, 3, (1, n)))
    return ora, ref, phi, cdwl, A


@pytest.mark.parametrize("kw", CASES, ids=IDS)
def test_apply_B_and_shift_vs_oracle(kw):
    ora, ref, phi, cdwl, A = _random_case(kw, 5)
    cdw = bool(kw.get("cdwU"))
    fn = {(LEFT, 0): ora.leftMultiplyBmat, (LEFT, 1): ora.leftMultiplyBmatInv, (RIGHT, 0): ora.rightMultiplyBmat,
          (RIGHT, 1): ora.rightMultiplyBmatInv}
    for (side, inv), f in fn.items():
        for k2, k1 in ((3, 2), (ref.m, 0)):
            if not ref.p.checkerboard and inv:
                continue                 # the oracle's dense inverse is numpy's inv of a product: no elementwise bound applies to it
            val, comp = ref.apply_B(A, side, inv, k2, k1, phi, cdwl)
            check_bound(f(A, k2, k1), val, comp, _c(ref, k2 - k1, cdw), what=f"side {side} inv {inv} B({k2},{k1})")
    ora.g = A
    val, comp = ref.shift_green(A)
    c = shift_c() if ref.p.checkerboard else mr.dense_c(ref.N, 2)
    check_bound(ora.shiftGreenSymmetric(), val, comp, c, what="shiftGreenSymmetric")


@pytest.mark.parametrize("kw", [c for c in CASES if c.get("checkerboard", True)], ids=[i for c, i in zip(CASES, IDS) if c.get("checkerboard", True)])
def test_inverse_is_inverse(kw):
    """B^-1 B = 1 and B B^-1 = 1 in long double, both sides.  The long-double arithmetic adds nothing visible; what remains is that
    the fp64 plaquette tables of the two signs are inverses of each other only to their own rounding: every entry is a product
    of two libm cosh / sinh values (at most 1 ulp = 2 u each, one more u for the product: 5 u), three passes per slice and
    direction: 3 x 2 x 5 u = 30 u per slice of the chain, times the magnitude companion of the round trip."""
    ora, ref, phi, cdwl, A = _random_case(kw, 6)
    eps = float(np.finfo(np.longdouble).eps)
    for side in (LEFT, RIGHT):
        for first in (0, 1):
            v1, _ = ref.apply_B(A, side, first, ref.m, 0, phi, cdwl)
            v2, comp = ref.apply_B(v1, side, 1 - first, ref.m, 0, phi, cdwl)
            _, comp2 = ref.apply_B(mr.abs1(v1), side, 1 - first, ref.m, 0, phi, cdwl)
            err = np.abs(v2 - A).astype(float)
            assert np.all(err <= (30 * ref.m * mr.U + bmult_c(ref.MSF, 2 * ref.m, True) * eps) * comp2), (side, first, float(np.max(err / comp2)))


def test_exact_family_tables():
    """what the exact GPU cases rely on: lambda = 0 makes the caches cosh = 1, sinh / |phi| = 0; zero hoppings make every plaquette
    factor the identity matrix (flux included); mu = 0 makes the band factors 1"""
    for flux in (False, True):
        kw = dict(opdim=2, L=6, beta=0.4, dtau=0.1, s=2, delaySteps=4, lambda_=0.0, txhor=0.0, txver=0.0, tyhor=0.0, tyver=0.0,
                  mux=0.0, muy=0.0, weakZflux=flux, bc="apbc-xy")
        phi = np.random.default_rng(1).uniform(-1, 1, (5, 36, 2))
        ora = DetSDWOracle(SDWParams(**kw).finalize(), phi=phi)
        assert np.array_equal(ora.coshTermPhi[1:], np.ones((4, 36))) and np.array_equal(ora.sinhTermPhi[1:], np.zeros((4, 36)))
        for key, mats in ora.plaq_mats.items():
            assert np.array_equal(mats, np.broadcast_to(np.eye(4), mats.shape)), key
        assert math.exp(ora.dtau * ora.mu_band[0]) == 1.0 and math.exp(-ora.dtau * ora.mu_band[1]) == 1.0
        for sign in (-1, +1):
            assert np.array_equal(ora.evMatrix(sign, phi[1, 0], 1.0, 0.0), np.eye(2))
        A = make_test_matrix(ora.ng)
        for f in (ora.leftMultiplyBmat, ora.leftMultiplyBmatInv, ora.rightMultiplyBmat, ora.rightMultiplyBmatInv):
            assert np.array_equal(f(A, 4, 0), A)
        ref = ModelReference(mr.make_lattice(**kw))
        val, _ = ref.apply_B(A, RIGHT, 1, 4, 0, phi)
        assert np.array_equal(val.astype(complex), A)


def _fourier(ref, S, bc, m):
    """the host-side step of finishMeasurements: kOcc[k] = 2 - sum_bins Re(e^{i k d} S(d)) / (m N)"""
    L, N = ref.L, ref.N
    d = np.arange(-(L - 1), L)
    offx = 0.5 if bc in ("apbc-x", "apbc-xy") else 0.0
    offy = 0.5 if bc in ("apbc-y", "apbc-xy") else 0.0
    out = np.zeros((2, N))
    for ks in range(N):
        kx = -math.pi + (ks % L + offx) * 2 * math.pi / L
        ky = -math.pi + (ks // L + offy) * 2 * math.pi / L
        ph = np.exp(1j * (ky * d[:, None] + kx * d[None, :]))
        for band in (0, 1):
            out[band, ks] = 2.0 - float(np.real(np.sum(ph * S[band].astype(complex)))) / (m * N)
    return out


@pytest.mark.parametrize("name", ["o2_L4_fmeas", "o2_L4_fmeas_apbc_flux", "o3_L4_fmeas", "o1_L4_fmeas"])
def test_measure_vs_golden(name):
    """the oracle walks the fixture's trajectory; at every measured slice the reference's accumulators are taken from the oracle's
    G, and after the host-side normalisation / Fourier step they must give the real reference's observables"""
    g = load_golden(name)
    op = oracle_params(g["params"])
    o = DetSDWOracle(op)
    ref = ModelReference(mr.make_lattice(**_pars_kw(op)))
    N, W2 = ref.N, (2 * ref.L - 1) ** 2
    acc = {}
    orig = o.measureFermionic

    def hooked(k):
        val, _ = ref.measure_accum(ref.shift_green(o.g)[0])
        acc["v"] = acc.get("v", 0) + val
        orig(k)
    o.measureFermionic = hooked
    i = 1
    while f"sweep{i}_phi" in g:
        o.sweepThermalization()
        i += 1
    j = 1
    while f"meas{j}_phi" in g:
        acc.clear()
        o.sweep(True)
        v = acc["v"].astype(float)
        m = ref.m
        assert v[3] == m
        TOL = 1e-10
        for key, got in (("greenK0", v[0] / m), ("greenLocal", v[1] / m), ("occDiffSq", v[2] / m)):
            assert abs(got - g[f"meas{j}_{key}"][0]) < TOL * max(1.0, abs(g[f"meas{j}_{key}"][0])), key
        assert relerr(v[4:4 + N] / m, g[f"meas{j}_pairPlus"].ravel()) < TOL
        assert relerr(v[4 + N:4 + 2 * N] / m, g[f"meas{j}_pairMinus"].ravel()) < TOL
        S = (v[4 + 2 * N::2] + 1j * v[5 + 2 * N::2]).reshape(2, 2 * ref.L - 1, 2 * ref.L - 1)
        kocc = _fourier(ref, S, op.bc, m)
        assert relerr(kocc[0], g[f"meas{j}_kOccX"].ravel()) < TOL
        assert relerr(kocc[1], g[f"meas{j}_kOccY"].ravel()) < TOL
        j += 1
    assert j > 1
    val, _ = ref.shift_green(o.g)
    assert relerr(val.astype(complex), g["final_shiftGreenSymmetric"]) < 1e-12


@pytest.mark.parametrize("opdim,L", [(1, 4), (2, 4), (3, 4), (2, 6), (3, 6)])
def test_measure_vs_oracle_general_matrix(opdim, L):
    """a general complex gs (every term of every observable O(1)), not a physical one"""
    kw = dict(opdim=opdim, L=L, beta=0.4, dtau=0.1, s=2, delaySteps=4, turnoffFermionMeasurements=False)
    o = DetSDWOracle(SDWParams(**kw).finalize())
    kw.pop("turnoffFermionMeasurements")
    ref = ModelReference(mr.make_lattice(**kw))
    rng = np.random.default_rng(opdim * 10 + L)
    n, N = ref.ng, ref.N
    gs = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    o.initMeasurements()
    o.shiftGreenSymmetric = lambda: gs
    o.measureFermionic(1)
    val, mag = ref.measure_accum(gs)
    v = val.astype(float)
    # the oracle sums in fp64 in numpy's order: t terms of a sum are off by at most t u sum|terms|
    assert abs(v[0] - o.greenK0) <= n * n * mr.U * mag[0]
    assert abs(v[1] - o.greenLocal) <= (n + 2) * mr.U * mag[1]
    assert abs(v[2] - o.occDiffSq) <= (16 * N + 8) * mr.U * mag[2]
    assert np.all(np.abs(v[4:4 + N] - o.pairPlus) <= 24 * mr.U * mag[4:4 + N])
    assert np.all(np.abs(v[4 + N:4 + 2 * N] - o.pairMinus) <= 24 * mr.U * mag[4 + N:4 + 2 * N])
    S = (v[4 + 2 * N::2] + 1j * v[5 + 2 * N::2]).reshape(2, 2 * L - 1, 2 * L - 1)
    kocc = _fourier(ref, S, "pbc", 1)
    assert relerr(2.0 - kocc[0], o.kOccX / N) < 1e-13 and relerr(2.0 - kocc[1], o.kOccY / N) < 1e-13
    # every bin against its definition, site pair by site pair
    Sd = np.zeros((2, 2 * L - 1, 2 * L - 1), dtype=complex)
    B = o._gl1_blocks(gs)
    for i in range(N):
        for jj in range(N):
            dy, dx = i // L - jj // L, i % L - jj % L
            Sd[0, dy + L - 1, dx + L - 1] += B[0][0][i, jj] + B[2][2][i, jj]
            Sd[1, dy + L - 1, dx + L - 1] += B[3][3][i, jj] + B[1][1][i, jj]
    assert relerr(S, Sd) < 1e-13


@pytest.mark.parametrize("opdim", [1, 2, 3])
@pytest.mark.parametrize("phi2bosons", [False, True])
def test_field_sums_vs_oracle(opdim, phi2bosons):
    kw = dict(opdim=opdim, L=4, beta=0.6, dtau=0.1, s=2, delaySteps=4, r=-0.7, c=2.5, u=1.3, phi2bosons=phi2bosons)
    phi = np.random.default_rng(opdim).uniform(-2, 2, (7, 16, opdim))
    o = DetSDWOracle(SDWParams(**kw).finalize(), phi=phi)
    ref = ModelReference(mr.make_lattice(**kw))
    val, mag = ref.phi_action(phi, -0.7)
    assert abs(float(val) - o.phiAction()) <= 8 * 6 * 16 * mr.U * mag
    val, mag = ref.phi_sq_sum(phi)
    assert abs(0.5 * 0.1 * float(val) - o.get_exchange_action_contribution()) <= (6 * 16 * opdim + 2) * mr.U * 0.05 * mag
    ch, sh = ref.cosh_sinh(phi)
    assert np.max(np.abs(ch[1:].astype(float) / o.coshTermPhi[1:] - 1)) < 16 * mr.U
    assert np.max(np.abs(sh[1:].astype(float) / o.sinhTermPhi[1:] - 1)) < 16 * mr.U
