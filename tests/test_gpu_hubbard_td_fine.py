"""GPU tests of the Hubbard replica's every-slice tau grid and its Matsubara transforms (HubbardParams.timeDisplacedEverySlice;
DQMC_TD_HUB_EVERY_SLICE, dqmc_hubbard_measure_timedisplaced_segment / _ends, dqmc_hubbard_td_matsubara_host).  The numpy
side is tests/hubbard_td_fine_reference.py, checked on the CPU by tests/test_hubbard_td_fine_cpu.py.

Shapes: L = 4 (one ragged workgroup of the displacement walk) and L = 6 (two workgroups, the second ragged); dtau = 0.1, U = 4, 3 chains;
(m, s) = (20, 7): s does not divide m, n = 3; (10, 5): s divides m, n = 2; (22, 5): a top segment of two slices; nfreq = 1, 3, 9 (a ragged
second tile of the eight-frequency tiles) and m.
Tolerances: 1e-9 at replica level (the project's 1e-10 on G carried through products of two or three entries), 1e-10 for the same
arithmetic in another order, 10 e_ref against direct inverses, 1e-12 where the same matrices enter both sides."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import hubbard_corr_reference as R
import hubbard_td_fine_reference as F
import td_matsubara_reference as M
import test_gpu_hubbard_correlators as T
from conftest import relerr

pytestmark = pytest.mark.gpu
EINVAL = -1
FINE = [nm + "TauFine" for nm in F.FINE_NAMES]
MATS = [nm + "Tau" for nm in F.FINE_NAMES]
NFREQ = lambda m: (1, 3, 9, m)


def _params(L, m, s, **over):
    kw = dict(beta=m * 0.1, s=s, timeDisplacedCorrelators=True, timeDisplacedEverySlice=True)
    kw.update(over)
    return dataclasses.replace(T._params(L), **kw)


def _fine(rep):
    return np.stack([rep.observable_vector(nm) for nm in FINE], axis=1)        # (m+1, 8, N)


def _make_oracle(pars, b):
    """the correlator test's oracle, subclassed again: an advance that ends on an interior boundary also records the rows of that
    boundary's segment, the closing advance rows 0 and m, each from direct inverses of the field as it stands"""
    from dethubbard_oracle import HubbardParams as OP
    base = type(T._make_oracle(pars, b))

    class FineOracle(base):
        def initMeasurements(self):
            super().initMeasurements()
            self.fine_sum = np.zeros((self.m + 1, 8, self.N))
            self.fine_count = np.zeros(self.m + 1, dtype=int)

        def finishMeasurements(self):
            super().finishMeasurements()
            assert np.all(self.fine_count == 1)
            self.fine_corr = self.fine_sum / self.N

        def _boundary(self, j):
            super()._boundary(j)
            if not self.recording:
                return
            if 1 <= j <= self.n - 1:
                up, down = F.segment_slices(j, self.m, self.s)
                rows = up + down
            else:
                rows = [0, self.m]
            Bs = F.oracle_bs(self)
            for k in rows:
                four = [F.displaced_greens(Bs[gc], k) for gc in (0, 1)]
                gt0, g0t, gtt, g00 = ([four[gc][i] for gc in (0, 1)] for i in range(4))
                self.fine_sum[k] += F.td_corr(gt0, g0t, gtt, g00, self.L)
                self.fine_count[k] += 1

    return FineOracle(OP(L=pars.L, d=2, beta=pars.beta, dtau=pars.dtau, s=pars.s, t=pars.t, U=pars.U, mu=pars.mu,
                         checkerboard=pars.checkerboard, rngSeed=pars.rngSeed, simindex=pars.simindex + b))


# ---- 5. the replica against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,stab,cb,mu,m,s", [(4, "svd", False, 0.0, 20, 7), (4, "qr", True, 0.0, 20, 7), (6, "qr", False, -0.5, 20, 7),
                                              (6, "svd", True, 0.0, 20, 7), (4, "qr", False, 0.0, 22, 5)])
def test_replica_fine_rows_match_the_oracle(L, stab, cb, mu, m, s):
    from detqmc_amd import DetHubbard
    pars = _params(L, m, s, stabilisation=stab, checkerboard=cb, mu=mu)
    nch = 3
    rep = DetHubbard(pars, nchains=nch)
    oras = [_make_oracle(pars, b) for b in range(nch)]
    inf = rep.info
    assert (inf.m, inf.s) == (m, s)
    assert np.allclose(rep.tau_grid(fine=True), 0.1 * np.arange(m + 1), rtol=1e-15, atol=0)
    worst = 0.0
    for sweep in (0, 1):                                  # the first goes down, the second up
        rep.sweep(True)
        for b, o in enumerate(oras):
            o.sweep(True)
            rep.select(b)
            assert np.array_equal(rep.auxfield[:, 1:], o.auxfield[:, 1:]), (sweep, b)
            fine = _fine(rep)
            assert fine.shape == (m + 1, 8, inf.N)
            for k in range(m + 1):
                for ci, nm in enumerate(FINE):
                    e = relerr(fine[k, ci], o.fine_corr[k, ci])
                    worst = max(worst, e)
                    assert e < 1e-9, (sweep, b, nm, k, e)
    print(f"L {L} {stab} cb {cb} mu {mu} (m, s) = ({m}, {s}): largest error of the every-slice rows {worst:.2e}")
    rep.close()


# ---- 6., 7. work copies and contraction at kernel level ---------------------------------------------------------------------------
def _blocks(z, N):
    return z[:N, :N].real, z[N:, N:].real


def _junk(z, N):
    """everything of an n_g x n_g matrix that a block-diagonal real matrix does not have: the off-diagonal spin blocks and all imaginary parts"""
    out = z.copy()
    out[:N, :N] = 1j * z[:N, :N].imag
    out[N:, N:] = 1j * z[N:, N:].imag
    return out


def _walk(L, m, s, stab, cb, mu, check):
    """a fresh replica's context walked down without updates; at every interior boundary the coarse row, the segment and (check) every
    comparison of tests 6 and 7; at the end the end rows from a G with NaN in its off-diagonal spin blocks.  Returns the blocks"""
    from detqmc_amd import DetHubbard
    nch = 3
    pars = _params(L, m, s, stabilisation=stab, checkerboard=cb, mu=mu)
    rep = DetHubbard(pars, nchains=nch)
    ctx = T._ctx(rep)
    N = L * L
    worst = dict(a=0.0, b=0.0, row=0.0, coarse=0.0, off=0.0, off_in=0.0, off_err=0.0)
    Bs, Bfull = [], []
    for b in range(nch):
        o = T._make_oracle(pars, b)
        rep.select(b)
        assert np.array_equal(rep.auxfield[:, 1:], o.auxfield[:, 1:])
        Bs.append(F.oracle_bs(o))
        Bfull.append([np.block([[u, np.zeros((N, N))], [np.zeros((N, N)), d]]) for u, d in zip(*Bs[-1])])
    e_ref = F.e_ref() if check else 0.0
    ctx.set_timedisplaced(True)
    ctx.measure_reset()

    def state():
        return ctx.g, ctx.green_timedisplaced()[1], ctx.green_timedisplaced()[2], ctx.green0_timedisplaced()[1]

    def read(b):
        ctx.select_chain(b)
        blk = ctx.hubbard_td_fine_read()
        return blk[:m + 1], blk[m + 1:].reshape(m + 1, 8, N)

    def at(j):
        ctx.hubbard_measure_timedisplaced(j)
        up, down = F.segment_slices(j, m, s)
        if check:
            copies = {}
            for b in range(nch):
                ctx.select_chain(b)
                g, gt0, g0t, g00 = state()
                # The off-diagonal spin blocks (and the imaginary parts) of the copies.  B_k is block diagonal and real, so they follow from
                # those of the boundary's matrices alone: exactly zero in, exactly zero out; and where the advance's own matrices carry
                # rounding-size entries there (the pivoted QR of the 2N x 2N matrix), the copies' entries are those entries
                # propagated, to the 1e-10 of the same arithmetic in another order -- nothing else is ever written there
                junk_in = max(np.abs(_junk(z, N)).max() for z in (g, gt0, g0t))
                worst["off_in"] = max(worst["off_in"], junk_in)
                for k in up + down:
                    ctx.td_fine_propagate(j, k)
                    sl, f_t0, f_0t, f_tt = ctx.green_td_fine()
                    assert sl == k
                    junk = [_junk(z, N) for z in (f_t0, f_0t, f_tt)]
                    worst["off"] = max(worst["off"], max(np.abs(z).max() for z in junk))
                    if junk_in == 0.0:
                        assert all(not z.any() for z in junk), (b, j, k)
                    else:
                        full = F.propagate(Bfull[b], (gt0, g0t, g), j * s, k)
                        worst["off_err"] = max(worst["off_err"], max(relerr(z, _junk(y, N)) for z, y in zip(junk, full)))
                    copies[b, k] = (f_t0, f_0t, f_tt, g00)
                    for gc in (0, 1):
                        blk = lambda z: _blocks(z, N)[gc]
                        ref_a = F.propagate(Bs[b][gc], (blk(gt0), blk(g0t), blk(g)), j * s, k)
                        ref_b = F.displaced_greens(Bs[b][gc], k)[:3]
                        worst["a"] = max(worst["a"], max(relerr(blk(x), y) for x, y in zip((f_t0, f_0t, f_tt), ref_a)))
                        worst["b"] = max(worst["b"], max(relerr(blk(x), y) for x, y in zip((f_t0, f_0t, f_tt), ref_b)))
            before = []
            for b in range(nch):
                ctx.select_chain(b)
                before.append(state())
            ctx.select_chain(0)
        ctx.hubbard_measure_timedisplaced_segment(j)
        if check:
            assert ctx.green_td_fine()[0] == (down[-1] if down else up[-1])
            for b in range(nch):
                ctx.select_chain(b)
                for x, y in zip(before[b], state()):             # G, G(tau,0), G(0,tau), G(0) of the sweep are only read
                    assert np.array_equal(x, y)
                cnt, rows = read(b)
                for k in up + down:
                    f_t0, f_0t, f_tt, g00 = copies[b, k]
                    ref = F.td_corr(_blocks(f_t0, N), _blocks(f_0t, N), _blocks(f_tt, N), _blocks(g00, N), L)
                    assert cnt[k] == 1.0
                    for ci in range(8):
                        worst["row"] = max(worst["row"], relerr(rows[k, ci], ref[ci]))
                coarse = ctx.hubbard_td_read()[ctx.n - 1:].reshape(ctx.n - 1, 6, N)
                for ci in range(6):                              # bit-identical inputs, another instantiation of the walk
                    worst["coarse"] = max(worst["coarse"], relerr(rows[j * s, ci], coarse[j - 1, ci]))
            ctx.select_chain(0)

    for k in range(m, (ctx.n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    for l in range(ctx.n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        at(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    gs = []
    for b in range(nch):                                         # the ends entry reads G element by element: plant NaN where it must not look
        ctx.select_chain(b)
        g = ctx.g
        gs.append(_blocks(g, N))
        g[:N, N:] = np.nan + 1j * np.nan
        g[N:, :N] = np.nan + 1j * np.nan
        ctx.set_green(g, 0)
    before = []
    for b in range(nch):
        ctx.select_chain(b)
        before.append(state())
    ctx.select_chain(0)
    ctx.hubbard_measure_timedisplaced_ends()
    for b in range(nch):                                         # the ends call only reads them too; bytewise, G carries the NaN
        ctx.select_chain(b)
        for x, y in zip(before[b], state()):
            assert x.tobytes() == y.tobytes()
    out = [read(b) for b in range(nch)]
    if check:
        eye = np.eye(N)
        for b, (gu, gd) in enumerate(gs):
            cnt, rows = out[b]
            assert np.array_equal(cnt, np.ones(m + 1)), cnt
            assert np.all(np.isfinite(rows))
            for k, (t0, ot) in ((0, (lambda x: x, lambda x: x - eye)), (m, (lambda x: eye - x, lambda x: -x))):
                ref = F.td_corr((t0(gu), t0(gd)), (ot(gu), ot(gd)), (gu, gd), (gu, gd), L)
                for ci in range(8):
                    worst["row"] = max(worst["row"], relerr(rows[k, ci], ref[ci]))
        print(f"L {L} (m, s) = ({m}, {s}) {stab} cb {cb}: work copies vs numpy steps {worst['a']:.2e}, vs direct inverses {worst['b']:.2e} "
              f"(10 e_ref = {10 * e_ref:.2e}); rows vs numpy {worst['row']:.2e}; row j s vs coarse row j {worst['coarse']:.2e}; "
              f"largest off-diagonal spin block entry of the work copies {worst['off']:.2e}, of the sweep's own G, G(tau,0), G(0,tau) {worst['off_in']:.2e}, "
              f"copies' entries against the propagated ones {worst['off_err']:.2e}")
        assert worst["a"] <= 1e-10 and worst["b"] <= 10 * e_ref
        assert worst["row"] <= 1e-12 and worst["coarse"] <= 1e-12
        assert worst["off_err"] <= 1e-10
        if worst["off_in"] == 0.0:
            assert worst["off"] == 0.0
    ctx.close()
    rep.close()
    return out


@pytest.mark.parametrize("L,m,s,stab,cb,mu", [(4, 20, 7, "svd", False, 0.0), (6, 22, 5, "qr", True, 0.0), (6, 10, 5, "qr", False, -0.5)])
def test_work_copies_and_contraction_at_kernel_level(L, m, s, stab, cb, mu):
    first = _walk(L, m, s, stab, cb, mu, True)
    again = _walk(L, m, s, stab, cb, mu, False)
    for (c0, r0), (c1, r1) in zip(first, again):
        assert np.array_equal(c0, c1) and np.array_equal(r0, r1)


# ---- 8. Matsubara transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,m,s", [(4, 20, 7), (6, 10, 5), (6, 22, 5)])
def test_matsubara_matches_numpy_on_the_block(L, m, s):
    from detqmc_amd import DetHubbard, _lib
    nch, N = 3, L * L
    rep = DetHubbard(_params(L, m, s, stabilisation="qr"), nchains=nch)
    ctx = T._ctx(rep)
    rep.sweep(True)
    blocks = []
    for b in range(nch):
        ctx.select_chain(b)
        blk = ctx.hubbard_td_fine_read()
        assert blk.size == (m + 1) * (1 + 8 * N) == rep.lib.dqmc_hubbard_td_fine_accum_size(ctx.h)
        assert np.array_equal(blk, ctx.measure_td_fine_read(0))            # the block also answers as channel 0 of the generic reader
        blocks.append(blk[m + 1:].reshape(m + 1, 8, N) / (blk[:m + 1, None, None] * N))
    worst = 0.0
    for nfreq in NFREQ(m):
        assert rep.lib.dqmc_hubbard_td_matsubara_size(ctx.h, nfreq) == nch * 8 * nfreq * N * 2
        got = ctx.hubbard_td_matsubara(nfreq)
        assert np.array_equal(got, ctx.hubbard_td_matsubara(nfreq))
        for b in range(nch):
            rep.select(b)
            for ci, nm in enumerate(MATS):
                ref = F.transform(ci, blocks[b][:, ci, :], L, 0.1, nfreq)
                e = np.max(np.abs(got[b, ci] - ref)) / np.max(np.abs(ref))
                worst = max(worst, e)
                assert e <= 1e-10, (nfreq, b, nm, e)
                assert np.array_equal(rep.matsubara_all(nm, nfreq)[b], got[b, ci]) and np.array_equal(rep.matsubara(nm, nfreq), got[b, ci])
    print(f"L {L} (m, s) = ({m}, {s}): largest error of the transforms {worst:.2e}")
    for ferm in (False, True):
        assert np.allclose(rep.matsubara_frequencies(5, fermionic=ferm), M.frequencies(m, 0.1, 5, ferm), rtol=1e-15, atol=0)
    # a block without samples: refused, out untouched
    ctx.measure_reset()
    out = np.full(nch * 8 * 3 * N * 2, 7.0)
    assert rep.lib.dqmc_hubbard_td_matsubara_host(ctx.h, 3, out.ctypes.data_as(_lib._DP)) == EINVAL and np.all(out == 7.0)
    ctx.close()
    rep.close()


@pytest.mark.parametrize("L", [4, 6])
def test_free_fermion_limit(L):
    """U = 0, no checkerboard break-up: the rows of greenUp are the free propagator, their transform its closed form"""
    from detqmc_amd import DetHubbard
    m, s, mu = 20, 7, -0.5
    rep = DetHubbard(_params(L, m, s, U=0.0, mu=mu, stabilisation="qr"), nchains=3)
    rows = F.free_green_rows(L, 1.0, mu, m, 0.1)
    for sweep in (0, 1):
        rep.sweep(True)
        for b in (0, 2):
            rep.select(b)
            for nm in ("greenUp", "greenDn"):
                e = relerr(rep.observable_vector(nm + "TauFine"), rows)
                print(f"L {L} sweep {sweep} chain {b} {nm}TauFine: relerr {e:.2e}")
                assert e < 1e-9, (sweep, b, nm, e)
            for nfreq in NFREQ(m):
                want = F.free_green_matsubara(L, 1.0, mu, m, 0.1, nfreq)
                e = np.max(np.abs(rep.matsubara("greenUpTau", nfreq) - want)) / np.max(np.abs(want))
                print(f"L {L} sweep {sweep} chain {b} matsubara(greenUpTau, {nfreq}): relerr {e:.2e}")
                assert e < 1e-9, (sweep, b, nfreq, e)
    rep.close()


# ---- 9. nothing else moves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stab", ["svd", "qr"])
def test_the_flag_changes_nothing_else(stab):
    from detqmc_amd import DetHubbard
    runs, launches = [], []
    fams = ("bmult", "gemm", "decomp", "decide", "other", "gather", "flush")
    for fine in (False, True):
        rep = DetHubbard(_params(4, 20, 7, stabilisation=stab, equalTimeCorrelators=True, timeDisplacedEverySlice=fine), nchains=2)
        ctx = T._ctx(rep)
        rep.select(1)
        trace = []
        rep.sweepThermalization()
        trace.append((rep.auxfield, rep.info.rngDrawn))
        for _ in range(2):
            rep.sweep(True)
            o = rep.observables
            trace.append((rep.auxfield, rep.info.rngDrawn, np.array([getattr(o, nm) for nm in T.SCALARS]), rep.zcorr, T._eq(rep), T._td(rep)))
        ctx.profile_enable(False)                            # clears the launch counters; they count without timing too
        for _ in range(2):
            rep.sweepThermalization()
        pr = ctx.profile_read()
        launches.append([pr[f][1] for f in fams])
        runs.append(trace)
        ctx.close()
        rep.close()
    print("launches per family, two thermalisation sweeps: without the flag", launches[0], "with it", launches[1])
    assert launches[0] == launches[1] and sum(launches[0]) > 0
    for a, b in zip(*runs):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_series_on_a_handle_with_the_flag():
    from detqmc_amd import DetHubbard, DqmcError
    lens = []
    for fine in (False, True):
        rep = DetHubbard(_params(4, 20, 7, equalTimeCorrelators=True, timeDisplacedEverySlice=fine), nchains=2)
        rep.series_begin(1, 4, host_copy=False)
        rep.sweep(True)
        lens.append((rep.series_info()[2], rep.series_state().parts))
        if fine:
            with pytest.raises(DqmcError) as e:
                rep.observable_vector("spinZZTauFine")
            assert "NO_HOST_COPY" in str(e.value)
            assert rep.matsubara("spinZZTau", 3).shape == (3, 16) and rep.matsubara_all("pairDTau", 2).shape == (2, 2, 16)
        rep.series_end()
        rep.close()
    assert lens[0] == lens[1]


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from detqmc_amd import DetHubbard, DqmcError, KernelContext, _lib
    lib = _lib.load()
    buf = np.full(1 << 16, 3.0)
    dp = buf.ctypes.data_as(_lib._DP)
    out = C.c_void_p()
    for flags, s in [(4, 7), (5, 7), (8, 7), (12, 7), (6, 20), (6, 25)]:
        p = _lib.dethubbard_params(L=4, d=2, s=s, m=20, dtau=0.1, t=1.0, U=4.0, measureFlags=flags)
        assert lib.dethubbard_create(C.byref(p), 1, C.byref(out)) == EINVAL and b"measureFlags" in lib.dethubbard_last_error(), (flags, s)
    hub = dict(opdim=1, L=4, m=20, s=7, delaySteps=1, cb_none=1, model=1, dtau=0.1, txhor=1.0, u=4.0, accRatio=0.5)
    fine_bit = _lib.DQMC_TD_HUB_EVERY_SLICE
    for tdv, phv, over in [(fine_bit, 1, {}), (2 | fine_bit, 1, {}), (1 | fine_bit, 0, {}), (1 | fine_bit, 1, dict(s=20))]:
        kp = _lib.dqmc_params(**{**hub, **over}, timedisplaced=tdv, td_particle_hole=phv)
        assert lib.dqmc_create_batch(C.byref(kp), 1, C.byref(out)) == EINVAL, (tdv, phv, over)
    for ph in (False, True):                                                       # the bit on an SDW context
        with pytest.raises(DqmcError) as e:
            KernelContext(2, 4, 20, 5, 0.1, timeDisplaced=1 | fine_bit, tdParticleHole=ph)
        assert e.value.code == EINVAL and "timedisplaced" in str(e.value)
    # every new entry on an SDW context, which has the SDW every-slice reservation
    sdw = KernelContext(2, 4, 20, 5, 0.1, timeDisplaced=True, tdParticleHole=True, tdEverySlice=True)
    for call in (lambda: lib.dqmc_hubbard_measure_timedisplaced_segment(sdw.h, 1), lambda: lib.dqmc_hubbard_measure_timedisplaced_ends(sdw.h),
                 lambda: lib.dqmc_hubbard_td_fine_read_host(sdw.h, dp), lambda: lib.dqmc_hubbard_td_matsubara_host(sdw.h, 1, dp)):
        assert call() == EINVAL and b"Hubbard model" in lib.dqmc_last_error()
    assert lib.dqmc_hubbard_td_fine_accum_size(sdw.h) == 0 and lib.dqmc_hubbard_td_matsubara_size(sdw.h, 1) == 0
    sdw.close()
    # the SDW every-slice entries on a Hubbard context with the reservation; the new ones away from their preconditions
    rep = DetHubbard(_params(4, 20, 7))
    h = lib.dethubbard_ctx(rep.h)
    for call in (lambda: lib.dqmc_measure_timedisplaced_segment(h, 1), lambda: lib.dqmc_measure_timedisplaced_ends(h),
                 lambda: lib.dqmc_measure_td_matsubara_host(h, 2, 1, dp)):
        assert call() == EINVAL and b"SDW model" in lib.dqmc_last_error()
    assert lib.dqmc_measure_td_matsubara_size(h, 2, 1) == 0 and lib.dqmc_measure_td_fine_accum_size(h, 1) == 0
    assert lib.dqmc_measure_td_fine_read_host(h, 1, dp) == EINVAL
    ctx = T._ctx(rep)
    before = ctx.hubbard_td_fine_read()
    assert lib.dqmc_hubbard_measure_timedisplaced_segment(h, 1) == EINVAL            # no boundary pair exists yet
    assert lib.dqmc_hubbard_measure_timedisplaced_segment(h, 0) == EINVAL and lib.dqmc_hubbard_measure_timedisplaced_segment(h, 3) == EINVAL
    assert lib.dqmc_td_fine_propagate(h, 1, 7) == EINVAL
    ctx.wrapDownGreen(20)                                                          # slice 19: neither 0 nor m
    assert lib.dqmc_hubbard_measure_timedisplaced_ends(h) == EINVAL
    for nfreq in (0, 21):
        assert lib.dqmc_hubbard_td_matsubara_size(h, nfreq) == 0 and lib.dqmc_hubbard_td_matsubara_host(h, nfreq, dp) == EINVAL
    assert lib.dqmc_hubbard_td_matsubara_host(h, 3, dp) == EINVAL                   # no row has a sample
    assert np.array_equal(ctx.hubbard_td_fine_read(), before) and np.all(buf == 3.0)
    ctx.close()
    rep.close()
    # the getters before a measurement sweep, after a thermalisation sweep, and without the flag
    rep = DetHubbard(_params(4, 20, 7))
    calls = (lambda: lib.dethubbard_get_td_fine_correlators(rep.h, dp), lambda: lib.dethubbard_get_matsubara(rep.h, 3, dp),
             lambda: lib.dethubbard_get_matsubara_all(rep.h, 3, dp))
    assert all(call() == EINVAL for call in calls)
    rep.sweep(True)
    assert all(call() == 0 for call in calls)
    assert lib.dethubbard_get_matsubara(rep.h, 0, dp) == EINVAL and lib.dethubbard_get_matsubara(rep.h, 21, dp) == EINVAL
    buf[:] = 3.0
    rep.sweepThermalization()
    assert all(call() == EINVAL for call in calls) and np.all(buf == 3.0)
    with pytest.raises(KeyError):
        rep.matsubara("noSuchTau", 1)
    rep.close()
    rep = DetHubbard(_params(4, 20, 7, timeDisplacedEverySlice=False))
    rep.sweep(True)
    assert all(call() == EINVAL for call in calls) and b"DETHUBBARD_MEASURE_TD_FINE" in lib.dethubbard_last_error()
    h = lib.dethubbard_ctx(rep.h)
    assert lib.dqmc_hubbard_td_fine_accum_size(h) == 0 and lib.dqmc_hubbard_measure_timedisplaced_ends(h) == EINVAL
    assert lib.dqmc_td_fine_propagate(h, 1, 7) == EINVAL
    rep.close()
