"""GPU tests of the Hubbard replica's equal-time and time-displaced correlators (HubbardParams.equalTimeCorrelators /
timeDisplacedCorrelators; dqmc_hubbard_* in include/dqmc_hip.h).  The numpy reference is tests/hubbard_corr_reference.py, itself checked
against Fock-space traces by tests/test_hubbard_corr_reference_cpu.py.

Shapes: L = 4 (one ragged workgroup of the displacement walk) and L = 6 (N = 36: two workgroups, the second ragged; TDP_PARTS = 8 does
not divide L); beta = 2, dtau = 0.1, s = 7 (s does not divide m = 20, n = 3: two interior boundaries); 3 chains (chain strides).
Tolerances: 1e-9 on replica-level channels = the project's 1e-10 on G carried through products of two or three entries; 1e-12 at kernel
level, where the same G enters both sides and only the summation order differs."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import hubbard_corr_reference as R
from conftest import relerr

pytestmark = pytest.mark.gpu
EINVAL = -1
BETA, DTAU, S = 2.0, 0.1, 7
EQ = ["greenUpCorr", "greenDnCorr", "chargeCorr", "spinZZCorr", "spinXXCorr", "pairSCorr", "pairSxCorr", "pairDCorr"]
TD = ["greenUpTau", "greenDnTau", "chargeTau", "spinZZTau", "spinXXTau", "pairSTau"]
SCALARS = ["occUp", "occDn", "occTotal", "occDouble", "localMoment", "eKinetic", "ePotential", "eTotal"]


def _params(L, **over):
    from detqmc_amd import HubbardParams
    kw = dict(L=L, beta=BETA, dtau=DTAU, s=S, U=4.0, mu=0.0)
    kw.update(over)
    return HubbardParams(**kw)


def _ctx(rep):
    from detqmc_amd.model import _CtxView
    inf = rep.info

    class _I:        # what _CtxView reads
        opdim, L, m, s, N, MSF, n_g, n = 1, inf.L, inf.m, inf.s, inf.N, 2, 2 * inf.N, inf.n
    return _CtxView(rep.lib, rep.lib.dethubbard_ctx(rep.h), _I)


def _eq(rep):
    return np.stack([rep.observable_vector(nm) for nm in EQ])


def _td(rep):
    return np.stack([rep.observable_vector(nm) for nm in TD], axis=1)        # (n-1, 6, N)


def _make_oracle(pars, b):
    """DetHubbardOracle whose measure also accumulates the reference correlators from its own G, and whose advances record the
    time-displaced reference from the field as it stands when the advance ends on an interior boundary"""
    from dethubbard_oracle import DetHubbardOracle, HubbardParams as OP

    class CorrOracle(DetHubbardOracle):
        recording = False

        def initMeasurements(self):
            super().initMeasurements()
            self.eq_sum = np.zeros((8, self.N))
            self.td_sum = np.zeros((self.n - 1, 6, self.N))
            self.td_count = np.zeros(self.n - 1, dtype=int)
            self.recording = True

        def measure(self):
            super().measure()
            self.eq_sum += R.eq_corr(self.g[0], self.g[1], self.L)

        def finishMeasurements(self):
            super().finishMeasurements()
            self.recording = False
            self.eq_corr = self.eq_sum / (self.m * self.N)
            assert np.all(self.td_count == 1)
            self.td_corr = self.td_sum / self.N

        def _boundary(self, j):
            if not self.recording or j < 1 or j > self.n - 1:
                return
            four = [R.displaced_greens([self.computeBmat(k, k - 1, gc) for k in range(1, self.m + 1)], self.s * j) for gc in (0, 1)]
            assert relerr(four[0][2], self.g[0]) < 1e-9          # the reference's G(tau) is the oracle's own G at the boundary
            gt0, g0t, gtt, g00 = ([four[gc][i] for gc in (0, 1)] for i in range(4))
            self.td_sum[j - 1] += R.td_corr(gt0, g0t, gtt, g00, self.L)
            self.td_count[j - 1] += 1

        def advanceDownGreen(self, l):
            super().advanceDownGreen(l)
            self._boundary(l - 1)

        def advanceUpGreen(self, l):
            super().advanceUpGreen(l)
            self._boundary(l + 1)

    return CorrOracle(OP(L=pars.L, d=2, beta=pars.beta, dtau=pars.dtau, s=pars.s, t=pars.t, U=pars.U, mu=pars.mu, checkerboard=pars.checkerboard,
                         rngSeed=pars.rngSeed, simindex=pars.simindex + b))


@pytest.mark.parametrize("L,stab,cb,mu", [(4, "svd", False, 0.0), (4, "qr", True, 0.0), (6, "qr", False, -0.5), (6, "svd", True, 0.0)])
def test_replica_correlators_match_the_oracle(L, stab, cb, mu):
    from detqmc_amd import DetHubbard
    pars = _params(L, stabilisation=stab, checkerboard=cb, mu=mu, equalTimeCorrelators=True, timeDisplacedCorrelators=True)
    nch = 3
    rep = DetHubbard(pars, nchains=nch)
    oras = [_make_oracle(pars, b) for b in range(nch)]
    inf = rep.info
    assert (inf.m, inf.s, inf.n) == (20, 7, 3)
    assert np.allclose(rep.tau_grid(), [0.7, 1.4])
    for sweep in (0, 1):                                  # the first goes down, the second up
        rep.sweep(True)
        for b, o in enumerate(oras):
            o.sweep(True)
            rep.select(b)
            assert np.array_equal(rep.auxfield[:, 1:], o.auxfield[:, 1:]), (sweep, b)
            eq, td = _eq(rep), _td(rep)
            for ci, nm in enumerate(EQ):
                e = relerr(eq[ci], o.eq_corr[ci])
                print(f"sweep {sweep} chain {b} {nm}: relerr {e:.2e}")
                assert e < 1e-9, (sweep, b, nm, e)
            for j in range(inf.n - 1):
                for ci, nm in enumerate(TD):
                    e = relerr(td[j, ci], o.td_corr[j, ci])
                    print(f"sweep {sweep} chain {b} {nm}[{j}]: relerr {e:.2e}")
                    assert e < 1e-9, (sweep, b, nm, j, e)
    rep.close()


@pytest.mark.parametrize("L", [4, 6])
def test_equal_time_kernel_matches_numpy_and_is_bit_reproducible(L):
    from detqmc_amd import DetHubbard
    nch = 3
    rep = DetHubbard(_params(L), nchains=nch)
    ctx = _ctx(rep)
    N = L * L
    rng = np.random.default_rng(100 + L)
    gs = []
    for b in range(nch):
        g = np.full((2 * N, 2 * N), np.nan + 1j * np.nan)          # the off-diagonal blocks must never be read
        gu, gd = rng.standard_normal((N, N)), rng.standard_normal((N, N))
        g[:N, :N], g[N:, N:] = gu, gd
        gs.append((gu, gd))
        ctx.select_chain(b)
        ctx.set_green(g, 20)
    ctx.hubbard_set_equal_time_correlators(True)
    assert rep.lib.dqmc_hubbard_eq_accum_size(ctx.h) == 1 + 8 * N
    runs = []
    for _ in range(2):
        ctx.measure_reset()
        ctx.measure_slice()
        blocks = []
        for b in range(nch):
            ctx.select_chain(b)
            blocks.append(ctx.hubbard_eq_read())
        runs.append(blocks)
    for b, (gu, gd) in enumerate(gs):
        blk = runs[0][b]
        assert blk[0] == 1.0
        ref = R.eq_corr(gu, gd, L)
        got = blk[1:].reshape(8, N)
        for ci, nm in enumerate(R.EQ_NAMES):
            e = relerr(got[ci], ref[ci])
            print(f"L {L} chain {b} {nm}: relerr {e:.2e}")
            assert e < 1e-12, (b, nm, e)
        assert np.array_equal(runs[1][b], blk)
    # two samples add up, and the switch off leaves the block alone
    ctx.measure_slice()
    ctx.hubbard_set_equal_time_correlators(False)
    ctx.measure_slice()
    ctx.select_chain(1)
    blk2 = ctx.hubbard_eq_read()
    assert blk2[0] == 2.0 and relerr(blk2[1:], 2 * runs[0][1][1:]) < 1e-14
    ctx.close()
    rep.close()


def _free_greens(L, t, mu, beta, tau):
    """(G(tau,0), G(0,tau), G(0)) of free fermions on the periodic L x L lattice, N x N each (the same for both spins; G(tau) = G(0))"""
    N = L * L
    kx, ky = np.meshgrid(2 * np.pi * np.arange(L) / L, 2 * np.pi * np.arange(L) / L)
    eps = (-2.0 * t * (np.cos(kx) + np.cos(ky)) - mu).ravel()
    kxs, kys = kx.ravel(), ky.ravel()
    x, y = np.arange(N) % L, np.arange(N) // L
    ph = np.exp(1j * (np.outer(x, kxs) + np.outer(y, kys)))                    # [site, k]
    build = lambda w: ((ph * w[None, :]) @ ph.conj().T).real / N
    f = 1.0 / (1.0 + np.exp(-beta * eps))                                      # <c c^+>
    return build(np.exp(-tau * eps) * f), build(-np.exp(tau * eps) * (1.0 - f)), build(f)


@pytest.mark.parametrize("stab", ["svd", "qr"])
def test_free_fermion_limit_is_exact(stab):
    """U = 0: the propagators do not depend on the field, e^{-dtau T} is exact without the checkerboard break-up"""
    from detqmc_amd import DetHubbard
    L, mu = 4, -0.5
    rep = DetHubbard(_params(L, U=0.0, mu=mu, stabilisation=stab, equalTimeCorrelators=True, timeDisplacedCorrelators=True), nchains=3)
    inf = rep.info
    refs_td = []
    for j in range(1, inf.n):
        gt0, g0t, g00 = _free_greens(L, 1.0, mu, inf.beta, j * inf.s * inf.dtau)
        refs_td.append(R.td_corr([gt0, gt0], [g0t, g0t], [g00, g00], [g00, g00], L) / inf.N)
    g00 = _free_greens(L, 1.0, mu, inf.beta, 0.0)[2]
    ref_eq = R.eq_corr(g00, g00, L) / inf.N
    for sweep in (0, 1):
        rep.sweep(True)
        for b in (0, 2):
            rep.select(b)
            eq, td = _eq(rep), _td(rep)
            for ci, nm in enumerate(EQ):
                e = relerr(eq[ci], ref_eq[ci])
                print(f"sweep {sweep} chain {b} {nm}: relerr {e:.2e}")
                assert e < 1e-9, (sweep, b, nm, e)
            for j in range(inf.n - 1):
                for ci, nm in enumerate(TD):
                    e = relerr(td[j, ci], refs_td[j][ci])
                    print(f"sweep {sweep} chain {b} {nm}[{j}]: relerr {e:.2e}")
                    assert e < 1e-9, (sweep, b, nm, j, e)
    rep.close()


@pytest.mark.parametrize("L,cb,mu", [(4, True, 0.0), (6, False, -0.5)])
def test_correlators_tie_to_the_scalar_observables(L, cb, mu):
    from detqmc_amd import DetHubbard
    pars = _params(L, checkerboard=cb, mu=mu, equalTimeCorrelators=True)
    rep = DetHubbard(pars, nchains=3)
    rep.sweepThermalization()
    rep.sweep(True)
    for b in range(3):
        rep.select(b)
        o = rep.observables
        gu, gd = rep.observable_vector("greenUpCorr"), rep.observable_vector("greenDnCorr")
        nn = [1, L - 1, L, (L - 1) * L]
        ties = [(4 * rep.observable_vector("spinZZCorr")[0], o.localMoment), (rep.observable_vector("chargeCorr")[0], o.occTotal + 2 * o.occDouble),
                (gu[0], 1 - o.occUp), (pars.t * sum(gu[d] + gd[d] for d in nn) - pars.mu * o.occTotal, o.eKinetic)]
        for got, want in ties:
            print(f"L {L} chain {b}: {got!r} vs {want!r}")
            assert np.isclose(got, want, rtol=1e-10, atol=0.0), (b, got, want)
    rep.close()


@pytest.mark.parametrize("stab", ["svd", "qr"])
def test_the_flags_change_nothing_else(stab):
    from detqmc_amd import DetHubbard
    runs = []
    for eq, td in [(False, False), (True, False), (False, True), (True, True)]:
        rep = DetHubbard(_params(4, stabilisation=stab, equalTimeCorrelators=eq, timeDisplacedCorrelators=td), nchains=2)
        rep.select(1)
        trace = []
        rep.sweepThermalization()
        trace.append((rep.auxfield, None, None))
        for _ in range(2):
            rep.sweep(True)
            o = rep.observables
            trace.append((rep.auxfield, np.array([getattr(o, nm) for nm in SCALARS]), rep.zcorr))
        runs.append(trace)
        rep.close()
    for other in runs[1:]:
        for (f0, s0, z0), (f1, s1, z1) in zip(runs[0], other):
            assert np.array_equal(f0, f1)
            if s0 is not None:
                assert np.allclose(s1, s0, rtol=1e-10, atol=1e-12) and np.allclose(z1, z0, rtol=1e-10, atol=1e-12)


def test_refusals():
    from detqmc_amd import DetHubbard, DqmcError, KernelContext, _lib
    lib = _lib.load()
    buf = np.zeros(4096)
    dp = buf.ctypes.data_as(_lib._DP)
    # readers without the flag, and before a measurement sweep
    rep = DetHubbard(_params(4))
    rep.sweep(True)
    assert lib.dethubbard_get_eq_correlators(rep.h, dp) == EINVAL and b"DETHUBBARD_MEASURE_EQ" in lib.dethubbard_last_error()
    assert lib.dethubbard_get_td_correlators(rep.h, dp) == EINVAL and b"DETHUBBARD_MEASURE_TD" in lib.dethubbard_last_error()
    with pytest.raises(DqmcError):
        rep.observable_vector("spinZZCorr")
    with pytest.raises(KeyError):
        rep.observable_vector("noSuchCorr")
    h = lib.dethubbard_ctx(rep.h)
    assert lib.dqmc_hubbard_td_accum_size(h) == 0 and lib.dqmc_hubbard_measure_timedisplaced(h, 1) == EINVAL
    assert lib.dqmc_set_timedisplaced(h, 1) == EINVAL
    rep.close()
    rep = DetHubbard(_params(4, equalTimeCorrelators=True, timeDisplacedCorrelators=True))
    assert lib.dethubbard_get_eq_correlators(rep.h, dp) == EINVAL and lib.dethubbard_get_td_correlators(rep.h, dp) == EINVAL
    rep.sweepThermalization()
    assert lib.dethubbard_get_eq_correlators(rep.h, dp) == EINVAL
    # SDW time-displaced entries on a Hubbard context that has the reservation
    h = lib.dethubbard_ctx(rep.h)
    assert lib.dqmc_hubbard_td_accum_size(h) == 2 * (1 + 6 * 16)
    for nm in ("", "_pair", "_ph", "_current", "_band", "_custom", "_custom_pair", "_green_matrix"):
        assert getattr(lib, "dqmc_measure_timedisplaced" + nm)(h, 1) == EINVAL, nm
        assert b"SDW model" in lib.dqmc_last_error(), nm
    assert lib.dqmc_measure_timedisplaced_segment(h, 1) == EINVAL and lib.dqmc_measure_timedisplaced_ends(h) == EINVAL
    assert lib.dqmc_set_equal_time_correlators(h, 1) == EINVAL
    assert lib.dqmc_hubbard_measure_timedisplaced(h, 0) == EINVAL          # no such boundary
    assert lib.dqmc_hubbard_measure_timedisplaced(h, 1) == EINVAL          # no pair has been computed for it
    rep.close()
    # the new kernel entries on an SDW context
    sdw = KernelContext(2, 4, 20, 10, 0.1, timeDisplaced=True, tdParticleHole=True)
    assert lib.dqmc_hubbard_set_equal_time_correlators(sdw.h, 1) == EINVAL and b"Hubbard model" in lib.dqmc_last_error()
    assert lib.dqmc_hubbard_measure_timedisplaced(sdw.h, 1) == EINVAL and b"Hubbard model" in lib.dqmc_last_error()
    assert lib.dqmc_hubbard_eq_accum_size(sdw.h) == 0 and lib.dqmc_hubbard_td_accum_size(sdw.h) == 0
    assert lib.dqmc_hubbard_eq_read_host(sdw.h, dp) == EINVAL and lib.dqmc_hubbard_td_read_host(sdw.h, dp) == EINVAL
    sdw.close()
    # an unknown flag bit
    p = _lib.dethubbard_params(L=4, d=2, s=7, beta=2.0, dtau=0.1, t=1.0, U=4.0, measureFlags=4)
    out = C.c_void_p()
    assert lib.dethubbard_create(C.byref(p), 1, C.byref(out)) == EINVAL and b"measureFlags" in lib.dethubbard_last_error()
    # every other value of the two create-time fields stays refused for the Hubbard model
    for tdv, phv in [(1, 0), (0, 1), (2, 1), (1, 2), (1 | _lib.DQMC_TD_EVERY_SLICE, 1), (1, 1 | _lib.DQMC_TD_PH_BAND)]:
        kp = _lib.dqmc_params(opdim=1, L=4, m=20, s=7, delaySteps=1, cb_none=1, model=1, dtau=0.1, txhor=1.0, u=4.0, accRatio=0.5,
                              timedisplaced=tdv, td_particle_hole=phv)
        assert lib.dqmc_create_batch(C.byref(kp), 1, C.byref(out)) == EINVAL, (tdv, phv)
