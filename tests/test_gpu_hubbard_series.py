"""The measurement series of the Hubbard replica (DQMC_SERIES_HUB_*, dqmc_series_hubbard_derived_host, dethubbard_series_*,
DetHubbard.series_*) against numpy (tests/hubbard_series_reference.py) on the vectors, blocks and bins the device itself returns.

Shapes (those of tests/test_gpu_hubbard_correlators.py): L = 4 (N = 16, less than a wave) and L = 6 (N = 36, no power of two, 8 does not
divide L); beta = 2, dtau = 0.1, s = 7 (n = 3: two tau rows); U = 4, mu = -0.5; 3 chains, default seed, simindex 0 .. 2; one thermalisation
sweep, then 6 measurement sweeps into bins of 2, maxBins = 3.

Tolerances (every comparison prints its figure first; a "row" is one [N] vector, or the eight scalars):
  C halves of parts 15 / 16, zcorr      bit for bit: both sides make one division by the same double; bins = (0 + a + b) / 2
  S halves                              1e-12 of the row's largest magnitude: the cosine sum runs in another order
  scalars                               1e-13 absolute: O(1) values from a handful of operations that may contract differently
  mean / err                            1e-13 / 1e-10 of the row's largest error, after asserting that the bins differ from their mean by
                                        more than 1e-3 of the row's scale (the reasoning of tests/test_gpu_series.py)
  R values, S_spin                      1e-12 absolute, after asserting |S_X(Q)| > 1e-3 of its row's largest magnitude
  errors of R and S_spin                1e-10 of the entry's largest error over the chains
  xi                                    NaN pattern equal to numpy's; finite values 1e-9, finite errors 1e-8 absolute, after asserting
                                        |root argument| > 1e-6 for the mean and every leave-one-out set: 1e-12 on the argument divided by
                                        2 sqrt(1e-6), and 2 sin(pi / L) >= 1 at L <= 6.  xi is not compared at Q = (1, 0).
The long-run test: the issue's configuration (binSize 1, maxBins 4, re-binning on, 10 sweeps) never holds the four closed bins that two
levels of the binning analysis need (a series that re-bins itself at maxBins = 4 shows at most three), so there the second level is
asserted to be refused and the first is compared; the two-level comparison runs on a second series of the same handle with maxBins = 8."""
import functools

import numpy as np
import pytest

import hubbard_series_reference as hr
import series_long_reference as slr
import series_reference as sr

pytestmark = pytest.mark.gpu
EINVAL = -1
BETA, DTAU, S_STAB, NCH, SWEEPS, BIN, MAXBINS = 2.0, 0.1, 7, 3, 6, 2, 3
EQ = [x + "Corr" for x in hr.EQ]
EQSQ = [x + "Sq" for x in hr.EQ]
TD = [x + "Tau" for x in hr.TD]
TDSQ = [x + "TauSq" for x in hr.TD]
HUB_PARTS = 0x1c000


def _params(L, **over):
    from detqmc_amd import HubbardParams
    kw = dict(L=L, beta=BETA, dtau=DTAU, s=S_STAB, U=4.0, mu=-0.5, equalTimeCorrelators=True, timeDisplacedCorrelators=True)
    kw.update(over)
    return HubbardParams(**kw)


def _ctx(rep):
    from detqmc_amd.model import _CtxView
    inf = rep.info

    class _I:        # what _CtxView reads
        opdim, L, m, s, N, MSF, n_g, n = 1, inf.L, inf.m, inf.s, inf.N, 2, 2 * inf.N, inf.n
    return _CtxView(rep.lib, rep.lib.dethubbard_ctx(rep.h), _I)


def _scalars(rep):
    o = rep.observables
    return np.array([getattr(o, nm) for nm in hr.SCALARS])


def _vectors(rep, corr=True):
    """every vector of the selected chain's last measurement sweep, by series name; the S(q) parts by numpy"""
    d = {"scalars": _scalars(rep), "zcorr": rep.zcorr}
    if corr:
        L = rep.info.L
        for nm in EQ + TD:
            d[nm] = rep.observable_vector(nm)
            d[nm + "Sq" if nm.endswith("Tau") else nm[:-4] + "Sq"] = sr.structure_factor_ref(d[nm], L)
    return d


def _names(eq=True, td=True):
    return ["scalars", "zcorr"] + (EQ + EQSQ if eq else []) + (TD + TDSQ if td else [])


def _qs(L):
    return [(L // 2, L // 2), (0, 0), (1, 0)]


@functools.lru_cache(maxsize=None)
def _run(L, mode="copy", nchains=NCH, simindex=0):
    """one thermalisation sweep, then 6 measurement sweeps: mode "none" (no series), "copy" (a series), "nocopy" (host_copy=False).
    Returns the vectors of every sweep and chain, the final field and rngDrawn, and for a series its bins, statistics and derived tables
    (each read twice)"""
    from detqmc_amd import DetHubbard, DqmcError
    rep = DetHubbard(_params(L, simindex=simindex), nchains=nchains)
    out = dict(rec=[], raised=[])
    try:
        rep.sweepThermalization()
        if mode != "none":
            rep.series_begin(BIN, MAXBINS, host_copy=(mode == "copy"))
            assert rep.series_is_open()
        for _ in range(SWEEPS):
            rep.sweep(True)
            row = []
            for b in range(nchains):
                rep.select(b)
                row.append(_vectors(rep, corr=(mode != "nocopy")))
                if mode == "nocopy":
                    for nm in ("spinZZCorr", "chargeTau"):
                        with pytest.raises(DqmcError) as e:
                            rep.observable_vector(nm)
                        out["raised"].append(str(e.value))
            out["rec"].append(row)
        out["field"], out["drawn"] = [], []
        for b in range(nchains):
            rep.select(b)
            out["field"].append(rep.auxfield)
            out["drawn"].append(rep.info.rngDrawn)
        if mode != "none":
            assert rep.series_info() == (3, 0, 8 + L * L + 16 * L * L + 24 * L * L)
            out["bins"] = []
            for b in range(nchains):
                rep.select(b)
                out["bins"].append({nm: rep.series_bins(nm) for nm in _names()})
            ctx = _ctx(rep)
            for key in ("stats", "stats2"):
                out[key] = {nm: rep.series_stats_all(nm) for nm in _names()}
            for key in ("derived", "derived2"):
                out[key] = {Q: ctx.series_hubbard_derived(Q) for Q in _qs(L)}
            out["named"] = {nm: rep.series_derived_all(nm) for nm in ("R_spinZZ", "xi_spin", "R_pairD", "S_spin", "xi_greenUp")}
            rep.select(1 % nchains)
            out["stats_sel"] = rep.series_stats("spinZZSq")
            rep.series_end()
            assert not rep.series_is_open()
    finally:
        rep.close()
    return out


@pytest.mark.parametrize("L", [4, 6])
def test_sample_kernels(L):
    from detqmc_amd import DetHubbard
    N, rows = L * L, 2
    rep = DetHubbard(_params(L), nchains=NCH)
    try:
        ctx = _ctx(rep)
        rep.sweep(True)

        def blocks():
            out = []
            for b in range(NCH):
                ctx.select_chain(b)
                out.append((ctx.measure_read(), ctx.hubbard_eq_read(), ctx.hubbard_td_read(), ctx.g))
            return out
        before = blocks()
        ctx.series_begin(1, 2, 0, HUB_PARTS)
        lay = [ctx.series_layout(p) for p in (14, 15, 16)]
        assert lay == [(0, 8 + N), (8 + N, 16 * N), (8 + 17 * N, 12 * rows * N)]
        assert ctx.series_info() == (0, 0, 8 + 17 * N + 12 * rows * N) and ctx.series_state().nfreq == 0
        ctx.series_add_sweep()
        assert ctx.series_info()[:2] == (1, 0)
        figs = dict(scalars=0.0, sq=0.0, tausq=0.0)
        for b in range(NCH):
            ctx.select_chain(b)
            smp = ctx.series_bins(0, 1)[0]
            rep.select(b)
            figs["scalars"] = max(figs["scalars"], np.abs(smp[:8] - _scalars(rep)).max())
            assert np.array_equal(smp[8:8 + N], rep.zcorr)
            c = np.stack([rep.observable_vector(nm) for nm in EQ])
            eq = smp[lay[1][0]:lay[1][0] + 16 * N].reshape(2, 8, N)
            assert np.array_equal(eq[0], c), b
            figs["sq"] = max(figs["sq"], sr.rows_close(eq[1], sr.structure_factor_ref(c, L), 1e-12, N))
            ct = np.stack([rep.observable_vector(nm) for nm in TD], axis=1)              # (n-1, 6, N)
            td = smp[lay[2][0]:].reshape(2, rows, 6, N)
            assert np.array_equal(td[0], ct), b
            figs["tausq"] = max(figs["tausq"], sr.rows_close(td[1], sr.structure_factor_ref(ct, L), 1e-12, N))
            # the restatement from the raw blocks gives the same sample
            ref = np.concatenate([hr.scalars_from_block(before[b][0], N, 1.0, 4.0, -0.5), hr.eq_sample_from_block(before[b][1], L),
                                  hr.td_sample_from_block(before[b][2], L, rows)])
            assert np.abs(smp[:8] - ref[:8]).max() <= 1e-13 and np.array_equal(smp[8:8 + 9 * N], ref[8:8 + 9 * N])
        print(f"L {L}: scalars {figs['scalars']:.2e} absolute (bound 1e-13); S(q) {figs['sq']:.2e}, S(q, tau) {figs['tausq']:.2e} of the row (bound 1e-12)")
        assert figs["scalars"] <= 1e-13
        after = blocks()
        for x, y in zip(before, after):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        ctx.series_end()
    finally:
        rep.close()


def _row(nm, N):
    return 8 if nm == "scalars" else N


@pytest.mark.parametrize("L", [4, 6])
def test_host_series_against_recorded_vectors(L):
    N = L * L
    run = _run(L)
    figs = dict(scal=0.0, sq=0.0, mean=0.0, err=0.0, spread=np.inf)
    for b in range(NCH):
        for nm in _names():
            recs = np.array([run["rec"][i][b][nm] for i in range(SWEEPS)])
            want = np.array([(recs[2 * k] + recs[2 * k + 1]) / 2.0 for k in range(3)])
            bins = run["bins"][b][nm]
            assert bins.shape == want.shape, nm
            if nm == "scalars":
                figs["scal"] = max(figs["scal"], np.abs(bins - want).max())
            elif nm.endswith("Sq"):
                figs["sq"] = max(figs["sq"], sr.rows_close(bins, want, 1e-12, N))
            else:
                assert np.array_equal(bins, want), (b, nm)
            # statistics against the jackknife of the device's own bins; the condition first, row by row
            rmean, rerr = sr.jackknife(bins)
            rl = _row(nm, N)
            dev = np.abs(bins - rmean).reshape(3, -1, rl).max(axis=(0, 2))
            scale = np.abs(rmean).reshape(-1, rl).max(axis=1)
            figs["spread"] = min(figs["spread"], (dev / scale).min())
            assert np.all(dev > 1e-3 * scale), (b, nm, dev / scale)
            mean, err = run["stats"][nm][0][b], run["stats"][nm][1][b]
            figs["mean"] = max(figs["mean"], sr.rows_close(mean, rmean, 1e-13, rl))
            figs["err"] = max(figs["err"], sr.rows_close(err, rerr, 1e-10, rl))
    print(f"L {L}: bins vs pair means: scalars {figs['scal']:.2e} absolute (bound 1e-13), S parts {figs['sq']:.2e} of the row (bound 1e-12); "
          f"smallest spread {figs['spread']:.2e} of the row's scale (floor 1e-3); mean {figs['mean']:.2e} (bound 1e-13), err {figs['err']:.2e} (bound 1e-10)")
    assert figs["scal"] <= 1e-13
    assert np.array_equal(run["stats_sel"][0], run["stats"]["spinZZSq"][0][1]) and np.array_equal(run["stats_sel"][1], run["stats"]["spinZZSq"][1][1])
    # derived quantities
    R_ENT, XI_ENT = list(range(8)) + [16, 17], list(range(8, 16)) + [18]
    for Q in _qs(L):
        val, err = run["derived"][Q]
        ref = [hr.derived(np.stack([run["bins"][b][nm] for nm in EQSQ], axis=1), L, Q) for b in range(NCH)]
        rv, re = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        for b in range(NCH):
            sq = np.stack([run["bins"][b][nm] for nm in EQSQ], axis=1)                   # [B][8][N]
            x = hr.triples(sq, L, Q)[:, :, :8]
            loo = np.array([x.mean(axis=0)] + [(x.sum(axis=0) - x[k]) / 2.0 for k in range(3)])
            rowmax = np.abs(sq.mean(axis=0)).max(axis=1)
            den = np.abs(loo[:, 0, :]).min(axis=0) / rowmax
            print(f"L {L} Q {Q} chain {b}: smallest |S_X(Q)| {den.min():.2e} of its row (floor 1e-3)")
            assert np.all(den > 1e-3), (Q, b, den)
            if Q != (1, 0):
                args = hr.root_arguments(sq, L, Q)
                print(f"L {L} Q {Q} chain {b}: smallest |root argument| {np.abs(args).min():.2e} (floor 1e-6), negative in {int((args < 0).any(axis=0).sum())} of 9 channels")
                assert np.all(np.abs(args) > 1e-6), (Q, b)
        fr = np.abs(val[:, R_ENT] - rv[:, R_ENT]).max()
        top = np.abs(re[:, R_ENT]).max(axis=0)
        fe = (np.abs(err[:, R_ENT] - re[:, R_ENT]).max(axis=0) / top).max()
        print(f"L {L} Q {Q}: R and S_spin values {fr:.2e} absolute (bound 1e-12), their errors {fe:.2e} of the entry's largest error (bound 1e-10)")
        assert np.all(np.isfinite(val[:, R_ENT])) and np.all(np.isfinite(err[:, R_ENT])) and fr <= 1e-12 and fe <= 1e-10
        if Q == (1, 0):
            continue
        xv, xe, rxv, rxe = val[:, XI_ENT], err[:, XI_ENT], rv[:, XI_ENT], re[:, XI_ENT]
        assert np.array_equal(np.isnan(xv), np.isnan(rxv)) and np.array_equal(np.isnan(xe), np.isnan(rxe)), Q
        okv, oke = ~np.isnan(rxv), ~np.isnan(rxe)
        fv = np.abs(xv[okv] - rxv[okv]).max() if okv.any() else 0.0
        fe = np.abs(xe[oke] - rxe[oke]).max() if oke.any() else 0.0
        print(f"L {L} Q {Q}: xi finite in {int(okv.sum())} of {okv.size} values, {int(oke.sum())} errors; values {fv:.2e} (bound 1e-9), errors {fe:.2e} (bound 1e-8)")
        assert fv <= 1e-9 and fe <= 1e-8
    # the named access and its default Q
    pipi, zero = run["derived"][(L // 2, L // 2)], run["derived"][(0, 0)]
    for nm, (tab, at) in dict(R_spinZZ=(pipi, 3), xi_spin=(pipi, 18), S_spin=(pipi, 16), R_pairD=(zero, 7), xi_greenUp=(zero, 8)).items():
        assert np.array_equal(run["named"][nm][0], tab[0][:, at], equal_nan=True) and np.array_equal(run["named"][nm][1], tab[1][:, at], equal_nan=True), nm


@pytest.mark.parametrize("L", [4, 6])
def test_chain_of_a_batch_equals_a_single_chain_handle(L):
    run = _run(L)
    for b in range(NCH):
        one = _run(L, "copy", 1, b)
        for nm in _names():
            assert np.array_equal(one["bins"][0][nm], run["bins"][b][nm]), (b, nm)
            for k in (0, 1):
                assert np.array_equal(one["stats"][nm][k][0], run["stats"][nm][k][b]), (b, nm, k)
        for Q in _qs(L):
            for k in (0, 1):
                assert np.array_equal(one["derived"][Q][k][0], run["derived"][Q][k][b], equal_nan=True), (b, Q, k)


@pytest.mark.parametrize("L", [4, 6])
def test_the_chain_does_not_depend_on_the_series(L):
    none, copy, nocopy = _run(L, "none"), _run(L), _run(L, "nocopy")
    for other in (copy, nocopy):
        for b in range(NCH):
            assert np.array_equal(other["field"][b], none["field"][b]) and other["drawn"][b] == none["drawn"][b]
            for i in range(SWEEPS):
                for nm in ("scalars", "zcorr"):
                    assert np.array_equal(other["rec"][i][b][nm], none["rec"][i][b][nm]), (b, i, nm)
    for b in range(NCH):
        for i in range(SWEEPS):
            for nm in EQ + TD:
                assert np.array_equal(copy["rec"][i][b][nm], none["rec"][i][b][nm]), (b, i, nm)
    assert len(nocopy["raised"]) == 2 * SWEEPS * NCH and all("NO_HOST_COPY" in msg for msg in nocopy["raised"])
    for b in range(NCH):
        for nm in _names():
            assert np.array_equal(nocopy["bins"][b][nm], copy["bins"][b][nm]), (b, nm)


@pytest.mark.parametrize("L", [4, 6])
def test_statistics_are_bit_reproducible(L):
    run = _run(L)
    for nm in _names():
        for k in (0, 1):
            assert np.array_equal(run["stats"][nm][k], run["stats2"][nm][k])
    for Q in _qs(L):
        for k in (0, 1):
            assert np.array_equal(run["derived"][Q][k], run["derived2"][Q][k], equal_nan=True)


def _raises(fn, frag=None):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == EINVAL
    if frag:
        assert frag in str(e.value), str(e.value)


def test_refusals():
    from detqmc_amd import DetHubbard, KernelContext, _lib
    lib = _lib.load()
    L, N = 4, 16
    begin = lib.dqmc_series_begin
    # kernel level, a Hubbard context with both blocks' reservations but the equal-time block never enabled
    rep = DetHubbard(_params(L))
    h = lib.dethubbard_ctx(rep.h)
    ctx = _ctx(rep)
    for parts in (1, 0x3fdf, 64, HUB_PARTS | 1, HUB_PARTS | 32, 0x20000, HUB_PARTS | 0x20000, 0, -1):
        assert begin(h, 2, 3, 0, parts) == EINVAL, parts
    assert lib.dqmc_hubbard_eq_accum_size(h) == 0
    assert begin(h, 2, 3, 0, 0x8000) == EINVAL and b"never been enabled" in lib.dqmc_last_error()
    assert begin(h, 0, 3, 0, 0x4000) == EINVAL and begin(h, 2, 1, 0, 0x4000) == EINVAL
    assert lib.dqmc_series_info(h, None, None, None) == EINVAL          # nothing was opened
    assert begin(h, 2, 3, 5, 0x4000 | 0x10000) == 0                       # nfreq is ignored
    assert ctx.series_state().nfreq == 0 and ctx.series_info() == (0, 0, 8 + N + 24 * N)
    assert begin(h, 2, 3, 0, 0x4000) == EINVAL                           # a second begin
    _raises(lambda: ctx.series_layout(15))
    _raises(lambda: ctx.series_hubbard_derived((0, 0)))                   # no equal-time part
    ctx.series_end()
    rep.close()
    # bit 16 without the time-displaced reservation
    rep = DetHubbard(_params(L, timeDisplacedCorrelators=False))
    h = lib.dethubbard_ctx(rep.h)
    assert begin(h, 2, 3, 0, 0x10000) == EINVAL and begin(h, 2, 3, 0, HUB_PARTS) == EINVAL
    assert lib.dqmc_series_info(h, None, None, None) == EINVAL
    # host level: the parts follow from the handle; a name whose part the series lacks
    _raises(lambda: rep.series_begin(0, 3))
    _raises(lambda: rep.series_begin(2, 1))
    assert lib.dethubbard_series_begin(rep.h, 2, 3, 2) == EINVAL and lib.dethubbard_series_begin(rep.h, 2, 3, 3) == EINVAL     # unknown flag bits
    _raises(rep.series_info)
    rep.series_begin(2, 3)
    assert rep.series_info() == (0, 0, 8 + N + 16 * N)
    _raises(lambda: rep.series_begin(2, 3))
    _raises(lambda: rep.series_stats("chargeTau"), "time-displaced")
    _raises(lambda: rep.series_bins("greenUpTauSq", 0, 1), "time-displaced")
    with pytest.raises(KeyError):
        rep.series_stats("noSuchSq")
    assert lib.dethubbard_series_stats(rep.h, 30, np.zeros(64).ctypes.data_as(_lib._DP), np.zeros(64).ctypes.data_as(_lib._DP)) == EINVAL
    assert lib.dethubbard_series_configure(rep.h, 4) == EINVAL                       # an unknown option
    rep.series_end()
    _raises(rep.series_end)
    rep.close()
    # measureFlags = 0: a scalars-only series
    rep = DetHubbard(_params(L, equalTimeCorrelators=False, timeDisplacedCorrelators=False))
    rep.series_begin(1, 2)
    assert rep.series_info() == (0, 0, 8 + N) and rep.series_state().parts == 0x4000
    _raises(lambda: rep.series_stats("spinZZSq"), "equal-time")
    _raises(lambda: rep.series_derived_all("R_spin"), "equal-time")
    rep.sweep(True)
    _raises(lambda: rep.series_stats("scalars"), "two closed bins")        # one closed bin
    rep.sweep(True)
    mean, err = rep.series_stats("scalars")
    assert np.abs(mean[2] - (mean[0] + mean[1])) < 1e-14 and np.all(np.isfinite(err))
    rep.close()                                                            # destroy ends the open series
    # the full handle: statistics and derived with one closed bin, Q outside the lattice, the 7th sweep on a full series
    rep = DetHubbard(_params(L))
    rep.sweepThermalization()
    rep.series_begin(BIN, MAXBINS)
    for i in range(SWEEPS):
        if i == 2:
            assert rep.series_info()[:2] == (1, 0)
            _raises(lambda: rep.series_stats("zcorr"), "two closed bins")
            _raises(lambda: rep.series_derived_all("R_spin"), "two closed bins")
        rep.sweep(False)                                                   # adds nothing
        rep.sweepThermalization()
        rep.sweep(True)
    assert rep.series_info()[:2] == (3, 0)
    for Q in ((L, 0), (0, L), (-1, 0), (0, -1)):
        _raises(lambda: rep.series_derived_all("R_spin", Q), "0 .. L-1")
    field, drawn, st = rep.auxfield, rep.info.rngDrawn, rep.series_state()
    _raises(lambda: rep.sweep(True), "full")
    assert np.array_equal(rep.auxfield, field) and rep.info.rngDrawn == drawn and rep.series_state().samples == st.samples == SWEEPS
    rep.sweepThermalization()                                              # other sweeps go on
    v, e = rep.series_derived_all("S_spin")
    assert np.all(np.isfinite(v)) and np.all(e > 0)
    rep.series_end()
    rep.sweep(True)                                                        # after the end sweeps go on and the getters work
    assert rep.observable_vector("spinZZCorr").shape == (N,) and rep.observable_vector("chargeTau").shape == (2, N)
    # a series without host copies, ended: the getters refuse stale vectors until the next measurement sweep
    rep.series_begin(BIN, MAXBINS, host_copy=False)
    _raises(lambda: rep.observable_vector("spinZZCorr"), "NO_HOST_COPY")
    rep.sweep(True)
    assert rep.observables.valid == 1 and rep.zcorr.shape == (N,)
    rep.series_end()
    _raises(lambda: rep.observable_vector("spinZZCorr"), "no measurement")
    rep.sweep(True)
    assert rep.observable_vector("spinZZCorr").shape == (N,)
    rep.close()
    # an SDW context keeps its mask
    sdw = KernelContext(2, 4, 20, 10, 0.1)
    sdw.set_equal_time_correlators(True)
    sdw.set_equal_time_correlators(False)
    for parts in (0x4000, 0x8000, 0x10000, HUB_PARTS, 1 | 0x4000):
        assert begin(sdw.h, 2, 3, 0, parts) == EINVAL, parts
    assert lib.dqmc_series_info(sdw.h, None, None, None) == EINVAL
    sdw.series_begin(2, 3, 0, 1)
    assert sdw.series_info() == (0, 0, 10 * N)
    assert lib.dqmc_series_hubbard_derived_host(sdw.h, 0, 0, np.zeros(64).ctypes.data_as(_lib._DP), np.zeros(64).ctypes.data_as(_lib._DP)) == EINVAL
    sdw.series_end()
    sdw.close()


def _state_tuple(st):
    return tuple(getattr(st, f) for f, _ in st._fields_)


def test_long_run_and_checkpoint(tmp_path):
    from detqmc_amd import DetHubbard, binning_analysis
    L, N, nch, total = 4, 16, 2, 10
    f_state, f_series = str(tmp_path / "state.bin"), str(tmp_path / "series.bin")

    def begin(rep, maxBins=4):
        rep.series_begin(1, maxBins, auto_rebin=True, track_variance=True)

    def snapshot(rep):
        ctx = _ctx(rep)
        st, data = ctx.series_export()
        out = dict(state=_state_tuple(rep.series_state()), export=data, bins=[], binning=rep.series_binning_all("spinZZSq", 1))
        for b in range(nch):
            rep.select(b)
            out["bins"].append({nm: rep.series_bins(nm) for nm in _names()})
        return out

    a = DetHubbard(_params(L), nchains=nch)
    b = None
    try:
        a.sweepThermalization()                            # with it the checkpoint falls on an even sweep, as the state file needs
        begin(a)
        zz = []
        for i in range(total):
            a.sweep(True)
            row = []
            for c in range(nch):
                a.select(c)
                row.append(a.observable_vector("spinZZCorr"))
            zz.append(row)
            if i == 4:
                a.save_state(f_state)
                a.series_save(f_series)
                mid = snapshot(a)
        st = a.series_state()
        # 4 bins of 1 -> 2 of 2; 2 more -> 4 -> 2 of 4; two sweeps in the open bin
        assert (st.bin_size, st.bins_closed, st.sweeps_in_open_bin, st.rebins, st.samples, st.max_bins) == (4, 2, 2, 2, 10, 4)
        smp = sr.structure_factor_ref(np.array(zz), L)                                   # [sweep][chain][N]
        pred = slr.series_run(np.transpose(smp, (1, 0, 2)), 1, 4, True)
        assert (pred["bin_size"], pred["in_open"], pred["samples"], pred["rebins"]) == (4, 2, 10, 2)
        fin = snapshot(a)
        for c in range(nch):
            fig = sr.rows_close(fin["bins"][c]["spinZZSq"], pred["bins"][c], 1e-12, N)
        print(f"re-binned spinZZSq bins against the numpy series: {fig:.2e} of the row (bound 1e-12)")
        _raises(lambda: a.series_binning_all("spinZZSq", 2), "two merged bins")          # two closed bins: one level only
        err1, tau1 = fin["binning"]
        ctx = _ctx(a)
        off = ctx.series_layout(15)[0] + (8 + 3) * N
        S = st.sample_len
        exp = fin["export"].reshape(-1, nch, S)
        m2 = exp[-1][:, off:off + N]
        for c in range(nch):
            rerr, rtau = slr.binning(fin["bins"][c]["spinZZSq"], 4, 1, m2=m2[c], samples=10)
            perr, ptau = binning_analysis(fin["bins"][c]["spinZZSq"], 4, variance=m2[c] / 9.0)
            cpu = float(np.abs(ptau / rtau - 1.0).max())
            fe, ft = sr.rows_close(err1[c], rerr, 1e-10, N), float(np.abs(tau1[c] / rtau - 1.0).max())
            print(f"chain {c}: one-level binning err {fe:.2e} (bound 1e-10), tau {ft:.2e} relative (bound {max(100 * cpu, 1e-9):.2e})")
            assert ft <= max(100.0 * cpu, 1e-9)
        # the resumed run: a second handle with the same parameters
        b = DetHubbard(_params(L), nchains=nch)
        b.load_state(f_state)
        begin(b)
        b.series_load(f_series)
        got = snapshot(b)
        assert got["state"] == mid["state"] and np.array_equal(got["export"], mid["export"])
        for i in range(5, total):
            b.sweep(True)
        got = snapshot(b)
        assert got["state"] == fin["state"]
        for c in range(nch):
            b.select(c)
            a.select(c)
            assert np.array_equal(b.auxfield, a.auxfield) and b.info.rngDrawn == a.info.rngDrawn
            for nm in _names():
                assert np.array_equal(got["bins"][c][nm], fin["bins"][c][nm]), (c, nm)
        assert np.array_equal(got["export"], fin["export"]), "open bin or variance buffers differ from the uninterrupted run"
        assert np.array_equal(got["binning"][0], fin["binning"][0]) and np.array_equal(got["binning"][1], fin["binning"][1])
        # refused loads leave the series as it was: other parts, options that maxBins of the open series cannot take
        b.series_end()
        b.series_begin(1, 3)
        _raises(lambda: b.series_load(f_series), "maxBins")
        assert _state_tuple(b.series_state())[:8] == (1, 3, 0, HUB_PARTS, 0, 0, 0, nch)
        b.close()
        b = DetHubbard(_params(L, timeDisplacedCorrelators=False), nchains=nch)
        begin(b)
        _raises(lambda: b.series_load(f_series), "parts")
        assert b.series_info()[:2] == (0, 0)
        b.close()
        b = DetHubbard(_params(L), nchains=1)
        begin(b)
        _raises(lambda: b.series_load(f_series), "chains")
        b.close()
        b = None
        # two levels of the binning analysis need four closed bins: a second series of the same handle with maxBins = 8
        a.series_end()
        begin(a, 8)
        for i in range(total):
            a.sweep(True)
        st = a.series_state()
        assert (st.bin_size, st.bins_closed, st.sweeps_in_open_bin, st.rebins, st.samples) == (2, 5, 0, 1, 10)
        err2, tau2 = a.series_binning_all("spinZZSq", 2)
        m2 = _ctx(a).series_export()[1].reshape(-1, nch, S)[-1][:, off:off + N]
        for c in range(nch):
            a.select(c)
            bins = a.series_bins("spinZZSq")
            rerr, rtau = slr.binning(bins, 2, 2, m2=m2[c], samples=10)
            perr, ptau = binning_analysis(bins, 2, variance=m2[c] / 9.0)
            cpu = float(np.abs(ptau / rtau - 1.0).max())
            fe = max(sr.rows_close(err2[c, l], rerr[l], 1e-10, N) for l in range(2))
            ft = float(np.abs(tau2[c] / rtau - 1.0).max())
            print(f"chain {c}: two-level binning err {fe:.2e} of the row's largest error (bound 1e-10), tau {ft:.2e} relative (bound {max(100 * cpu, 1e-9):.2e})")
            assert ft <= max(100.0 * cpu, 1e-9)
    finally:
        a.close()
        if b is not None:
            b.close()
