"""The measurement series over a long run: re-binning (dqmc_series_rebin, DQMC_SERIES_AUTO_REBIN), the running variance
(DQMC_SERIES_TRACK_VARIANCE), the binning analysis with tau_int (dqmc_series_binning_host), export / import and the series file
(detsdw_series_save / _load).

Kernel level.  Real samples come from a down pass on prescribed fields (tests/test_gpu_series_route.py: the amplitude grows with the
sweep and the chain); the device's own samples are the bins of a series with bin_size = 1.  Merging two bins is (a + b) * 0.5, adding a
sample and closing a bin are the operations of k_series_accum: numpy repeats all of them bit for bit, so bins are compared with
np.array_equal against tests/series_long_reference.py.  Synthetic bins go in through series_import.

Bounds that are not bit-equality:
  * auto re-binned bins against a plain series with bin_size 4: the summation order differs; 1e-14 of the largest |sample| of the row
    (the bound of test_gpu_series.test_host_series_vs_recorded_vectors for two forms of the same sample).
  * w, m2 against the two-pass mean and sum of squared deviations of the device's own samples: 100 x the deviation of the numpy Welford
    recurrence from the two-pass value on these samples, or 1e-13 of the row's scale if that is larger (the margin covers fma
    contraction on the device).  Measured on the MI355X, identity / routed: the numpy recurrence lies 3.5e-16 / 4.1e-16 (w) and
    6.6e-15 / 6.9e-15 (m2) of the row's scale from the two-pass value, so the bounds are 1e-13 (w) and 6.6e-13 / 6.9e-13 (m2); the device
    lies 3.5e-16 / 4.1e-16 (w) and 6.6e-15 / 7.0e-15 (m2) away.
  * binning errors: 1e-10 of the row's largest error, the bound of test_gpu_series for k_series_stats.
  * tau: 100 x the deviation between the two numpy forms (series_long_reference.binning and detqmc_amd.binning_analysis), or 1e-9
    relative if that is larger.  Measured: the two numpy forms give identical bits on these data (0.0), so the bound is 1e-9; the device
    lies 8.9e-16 away (errors: 2.5e-16 of the row's largest error).
The binning test imports samples = 125 with two samples in the open bin of 40 bins of 3: the import takes the counters as they are given
and tau uses `samples` for sigma^2 only."""
import dataclasses
import functools

import numpy as np
import pytest

import series_long_reference as slr
import series_reference as sr

pytestmark = pytest.mark.gpu

L, N, M, S_STAB, NCH, NFREQ, PARTS = 4, 16, 20, 5, 4, 3, 31
NSWEEPS, MAXBINS = 8, 4
EINVAL = -1
AUTO, TRACK = 1, 2
IDENTITY = list(range(NCH))
CYCLES = ([1, 2, 3, 0], [2, 0, 3, 1])                      # the two 4-cycles of tests/test_gpu_series_route.py
ROUTES = [CYCLES[i % 2] for i in range(NSWEEPS)]           # a new route before every sweep
STATE_FIELDS = ("bin_size", "max_bins", "nfreq", "parts", "flags", "bins_closed", "sweeps_in_open_bin", "nb", "samples", "rebins",
                "sample_len")


def _phi(sweep, chain):
    phi = np.random.default_rng(1000 * L + 10 * sweep + chain).uniform(-1.0, 1.0, (M + 1, N, 2)) * (0.5 + 0.5 * sweep + 0.2 * chain)
    phi[0] = 0.0
    return phi


def _context(nchains):
    from detqmc_amd import KernelContext
    return KernelContext(2, L, M, S_STAB, 0.1, delaySteps=4, stabilisation="qr", nchains=nchains, timeDisplaced=2, tdParticleHole=True,
                         tdCurrent=True, tdEverySlice=True)


def _fill(ctx, phis):
    """new fields, then one down pass without updates that refills every block (tests/test_gpu_series.py)"""
    m, s, n = ctx.m, ctx.s, ctx.n
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.set_equal_time_correlators(True)
    ctx.measure_reset()
    for k in range(m, (n - 1) * s, -1):
        ctx.measure_slice()
        ctx.wrapDownGreen(k)
    ctx.set_equal_time_correlators(False)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        ctx.measure_timedisplaced_segment(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


def _raises(fn, code=EINVAL):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == code
    return True


def _st(st):
    return {f: int(getattr(st, f)) for f in STATE_FIELDS}


def _state(template, **changes):
    from detqmc_amd._lib import dqmc_series_state
    st = dqmc_series_state()
    for f in STATE_FIELDS:
        setattr(st, f, changes.get(f, getattr(template, f)))
    return st


def _export(ctx):
    """dict(state, raw, bins [closed][slot][S], open [slot][S], and w, m2 [slot][S] if the variance is tracked)"""
    st, raw = ctx.series_export()
    nb, S, B = st.nb, st.sample_len, st.bins_closed
    n = nb * S
    rec = dict(state=_st(st), raw=raw, bins=raw[:B * n].reshape(B, nb, S), open=raw[B * n:(B + 1) * n].reshape(nb, S))
    if st.flags & TRACK:
        rec["w"], rec["m2"] = raw[(B + 1) * n:(B + 2) * n].reshape(nb, S), raw[(B + 2) * n:].reshape(nb, S)
    else:
        assert raw.size == (B + 1) * n
    return rec


def _same(a, b):
    return a["state"] == b["state"] and np.array_equal(a["raw"], b["raw"])


def _pack(bins, open_bin, w=None, m2=None):
    parts = [np.ravel(bins), np.ravel(open_bin)] + ([np.ravel(w), np.ravel(m2)] if w is not None else [])
    return np.concatenate(parts)


def _rows(layout):
    rows = [(x * N, N) for x in range(10)]
    for ch in range(4):
        off, ln = layout[1 + ch]
        rows += [(off + r * 2 * N, 2 * N) for r in range(ln // (2 * N))]
    return rows


def _open_series(ctx, nchains, bin_size, max_bins):
    """the blocks must exist before a series can be opened: one fill, then begin"""
    _fill(ctx, [_phi(0, c) for c in range(nchains)])
    ctx.series_begin(bin_size, max_bins, NFREQ, PARTS)
    return ctx.series_state()


def _synthetic(nslots, S, B, seed):
    """bins [B][slot][S], open [slot][S], w, m2 [slot][S]: another base and amplitude per slot"""
    rng = np.random.default_rng(seed)
    base = np.array([2.0 + 1.5 * s for s in range(nslots)])[None, :, None]
    amp = np.array([0.1 * (s + 1) for s in range(nslots)])[None, :, None]
    bins = base + amp * rng.standard_normal((B, nslots, S))
    open_bin = (base + amp * rng.standard_normal((1, nslots, S)))[0] * 2.0
    w = (base + 0.01 * amp * rng.standard_normal((1, nslots, S)))[0]
    m2 = (124.0 * 3.0 * amp * amp * rng.uniform(0.8, 1.2, (1, nslots, S)))[0]
    return bins, open_bin, w, m2


# ---- real samples ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _samples():
    """[sweep][chain][S]: the device's own samples, as the bins of a series with bin_size = 1; also what a plain series does when it is
    full, and a plain series with bin_size 4 on the same fields"""
    ctx = _context(NCH)
    try:
        _fill(ctx, [_phi(0, c) for c in range(NCH)])
        ctx.series_begin(1, NSWEEPS, NFREQ, PARTS)
        layout = [ctx.series_layout(p) for p in range(5)]
        for i in range(NSWEEPS):
            if i:
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
            ctx.series_add_sweep()
        st = ctx.series_state()
        assert (st.bins_closed, st.samples, st.rebins, st.flags, st.bin_size) == (NSWEEPS, NSWEEPS, 0, 0, 1)
        smp = _export(ctx)["bins"].copy()
        _raises(ctx.series_add_sweep)                        # full, and no auto re-binning: refused as ever
        ctx.series_end()
        _raises(lambda: ctx.series_begin(1, NSWEEPS, NFREQ, 32))     # the options are no bits of the parts mask
        ctx.series_begin(4, 2, NFREQ, PARTS)                 # a plain series with bin_size 4, the fields in the same order
        for i in range(NSWEEPS):
            _fill(ctx, [_phi(i, c) for c in range(NCH)])
            ctx.series_add_sweep()
        plain4 = _export(ctx)["bins"].copy()
        ctx.series_end()
    finally:
        ctx.close()
    smp.setflags(write=False)
    return smp, layout, plain4


@functools.lru_cache(maxsize=None)
def _auto_run(routed):
    """bin_size 1, max_bins 4, both options, 8 sweeps; the export after every sweep"""
    ctx = _context(NCH)
    recs = []
    try:
        st0 = _open_series(ctx, NCH, 1, MAXBINS)
        ctx.series_configure(auto_rebin=True, track_variance=True)
        assert ctx.series_state().flags == AUTO | TRACK and st0.flags == 0
        ptr, S = ctx.series_sample_device()
        rows = [ptr + 8 * b * S for b in range(NCH)]
        for i in range(NSWEEPS):
            if i:
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
            if routed:
                before = _st(ctx.series_state())
                ctx.series_form_sample()
                assert _st(ctx.series_state()) == before     # forming moves no counter and never re-bins
                src = [None] * NCH
                for c, s in enumerate(ROUTES[i]):
                    src[s] = rows[c]
                ctx.series_accumulate(src)
            else:
                ctx.series_add_sweep()
            recs.append(_export(ctx))
        if not routed:
            _raises(lambda: ctx.series_configure(auto_rebin=False))      # not empty any more
            assert ctx.series_state().flags == AUTO | TRACK
        ctx.series_end()
    finally:
        ctx.close()
    return recs


def _expected_run(routed, upto=NSWEEPS):
    smp = _samples()[0]
    per_slot = slr.routed_samples(smp, ROUTES if routed else [IDENTITY] * NSWEEPS)
    return per_slot, slr.series_run(per_slot[:, :upto], 1, MAXBINS, True)


@pytest.mark.parametrize("routed", [False, True])
def test_auto_rebin_on_real_samples(routed):
    recs = _auto_run(routed)
    S = recs[0]["state"]["sample_len"]
    want_counters = [(1, 1), (2, 1), (3, 1), (2, 2), (2, 2), (3, 2), (3, 2), (2, 4)]          # (bins closed, bin_size) after every sweep
    want_open = [0, 0, 0, 0, 1, 0, 1, 0]
    for i, rec in enumerate(recs):
        st = rec["state"]
        assert (st["bins_closed"], st["bin_size"]) == want_counters[i] and st["sweeps_in_open_bin"] == want_open[i], (i, st)
        assert st["bins_closed"] < MAXBINS and st["samples"] == i + 1 and st["rebins"] == (0 if i < 3 else 1 if i < 7 else 2)
        assert st["flags"] == AUTO | TRACK and st["max_bins"] == MAXBINS and st["nb"] == NCH and st["sample_len"] == S
        _, want = _expected_run(routed, i + 1)
        assert np.array_equal(rec["bins"].transpose(1, 0, 2), want["bins"]), i
        assert np.array_equal(rec["open"], want["open"]), i
    if not routed:
        smp, layout, plain4 = _samples()
        worst = 0.0
        for s in range(NCH):
            for off, ln in _rows(layout):
                sl = slice(off, off + ln)
                worst = max(worst, sr.rows_close(recs[-1]["bins"][:, s, sl], plain4[:, s, sl], 1e-14, ln, scale=np.abs(smp[:, s, sl]).max(axis=0)))
        print(f"auto re-binned bins against a plain series with bin_size 4: {worst:.2e} of the row's largest |sample| (bound 1e-14)")


@pytest.mark.parametrize("routed", [False, True])
def test_running_variance_on_real_samples(routed):
    recs = _auto_run(routed)
    layout = _samples()[1]
    per_slot, _ = _expected_run(routed)
    if routed:
        assert not np.array_equal(per_slot, _expected_run(False)[0])
    figs = {}
    for s in range(NCH):
        mean, m2 = slr.two_pass(per_slot[s])
        ww, wm2 = slr.welford(per_slot[s])
        for off, ln in _rows(layout):
            sl = slice(off, off + ln)
            for nm, ref, cpu, dev in (("w", mean[sl], ww[sl], recs[-1]["w"][s, sl]), ("m2", m2[sl], wm2[sl], recs[-1]["m2"][s, sl])):
                scale = np.abs(ref).max()
                assert scale > 0
                c, d = np.abs(cpu - ref).max() / scale, np.abs(dev - ref).max() / scale
                figs[nm] = tuple(max(a, b) for a, b in zip(figs.get(nm, (0.0, 0.0)), (c, d)))
    for nm, (c, d) in figs.items():
        bound = max(100.0 * c, 1e-13)
        print(f"routed={routed} {nm}: numpy Welford against two-pass {c:.2e}, device against two-pass {d:.2e} of the row's scale (bound {bound:.2e})")
        assert d <= bound, (nm, d, bound)


def test_continuation_from_an_export_gives_the_same_bits():
    recs = _auto_run(False)
    cut = 3
    ctx = _context(NCH)
    try:
        _fill(ctx, [_phi(cut, c) for c in range(NCH)])
        ctx.series_begin(1, MAXBINS, NFREQ, PARTS)
        st = _state(ctx.series_state(), **recs[cut - 1]["state"])
        ctx.series_import(st, recs[cut - 1]["raw"])
        assert _same(_export(ctx), recs[cut - 1])
        for i in range(cut, NSWEEPS):
            if i > cut:
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
            ctx.series_add_sweep()
            assert _same(_export(ctx), recs[i]), i
        ctx.series_end()
    finally:
        ctx.close()


# ---- synthetic bins -------------------------------------------------------------------------------------------------------------------
NSLOTS, NBINS, BIG = 3, 40, 64


def test_export_import_round_trip_and_refusals():
    ctx = _context(NSLOTS)
    rng = np.random.default_rng(77)
    try:
        for fn in (ctx.series_state, ctx.series_rebin, ctx.series_export, lambda: ctx.series_binning(1), ctx.series_configure):
            _raises(fn)                                      # no series open
        st0 = _open_series(ctx, NSLOTS, 2, 6)
        S = st0.sample_len
        assert _st(st0) == dict(bin_size=2, max_bins=6, nfreq=NFREQ, parts=PARTS, flags=0, bins_closed=0, sweeps_in_open_bin=0, nb=NSLOTS,
                                samples=0, rebins=0, sample_len=S) and S == 1024
        assert ctx.lib.dqmc_series_configure(ctx.h, 4) == EINVAL and ctx.series_state().flags == 0           # an unknown option
        st = _state(st0, bin_size=5, flags=TRACK, bins_closed=3, sweeps_in_open_bin=1, samples=16, rebins=2)
        data = rng.standard_normal((3 + 1 + 2) * NSLOTS * S)
        ctx.series_import(st, data)
        got = _export(ctx)
        assert np.array_equal(got["raw"], data) and got["state"] == dict(_st(st), max_bins=6)
        assert ctx.series_info() == (3, 1, S)
        n = NSLOTS * S
        refusals = [("len", st, data[:-1]),
                    ("parts", _state(st, parts=15), data),
                    ("nfreq", _state(st, nfreq=NFREQ - 1), data),
                    ("chains", _state(st, nb=NSLOTS + 1), data),
                    ("bins_closed >= max_bins", _state(st, bins_closed=6), rng.standard_normal((6 + 3) * n)),
                    ("sweeps_in_open_bin >= bin_size", _state(st, sweeps_in_open_bin=5), data),
                    ("unknown flag", _state(st, flags=4 | TRACK), data)]
        for what, bad, buf in refusals:
            _raises(lambda: ctx.series_import(bad, buf))
            assert _same(_export(ctx), got), what
        _raises(lambda: ctx.series_configure(track_variance=True))           # bins are there: the series is not empty
        assert _same(_export(ctx), got)
        ctx.series_end()
        ctx.series_begin(2, 5, NFREQ, PARTS)                 # an odd max_bins cannot re-bin by itself
        _raises(lambda: ctx.series_configure(auto_rebin=True))
        ctx.series_configure(track_variance=True)
        empty = _export(ctx)
        assert empty["state"]["flags"] == TRACK and not empty["raw"].any()
        _raises(lambda: ctx.series_import(_state(st, flags=AUTO | TRACK), data))
        assert _same(_export(ctx), empty)
        ctx.series_import(st, data)                          # the same state is fine without the option
        assert np.array_equal(_export(ctx)["raw"], data)
        ctx.series_end()
    finally:
        ctx.close()


def test_rebin_on_synthetic_bins():
    ctx = _context(NSLOTS)
    try:
        st0 = _open_series(ctx, NSLOTS, 3, BIG)
        S = st0.sample_len
        bins, open_bin, _, _ = _synthetic(NSLOTS, S, NBINS, 1)
        ctx.series_import(_state(st0, bins_closed=NBINS, sweeps_in_open_bin=2, samples=3 * NBINS + 2), _pack(bins, open_bin))
        want, size = bins, 3
        for k in (1, 2, 3):
            ctx.series_rebin()
            want, size = slr.rebinned(want), 2 * size
            rec = _export(ctx)
            assert np.array_equal(rec["bins"], want), k
            assert np.array_equal(rec["open"], open_bin), k
            assert rec["state"] == dict(_st(st0), bins_closed=NBINS >> k, bin_size=size, rebins=k, sweeps_in_open_bin=2, samples=3 * NBINS + 2)
        assert want.shape[0] == 5 and not np.array_equal(want[0, 0], want[0, 1])
        _raises(ctx.series_rebin)                            # five bins: odd
        assert _same(_export(ctx), rec)
        ctx.series_import(_state(st0, bin_size=1 << 30), _pack(bins[:0], open_bin))
        rec = _export(ctx)
        _raises(ctx.series_rebin)                            # the bin size cannot double any more
        assert _same(_export(ctx), rec)
        ctx.series_import(_state(st0, bin_size=7, sweeps_in_open_bin=4), _pack(bins[:0], open_bin))
        ctx.series_rebin()                                   # no closed bin: only the bin size doubles
        rec = _export(ctx)
        assert rec["state"] == dict(_st(st0), bin_size=14, rebins=1, sweeps_in_open_bin=4) and np.array_equal(rec["open"], open_bin)
        ctx.series_end()
    finally:
        ctx.close()


def _binning_reference(bins, m2, levels, bin_size, samples):
    """err, tau [levels][slot][S] of the reference, slot by slot"""
    out = [slr.binning(bins[:, s], bin_size, levels, m2=m2[s], samples=samples) for s in range(bins.shape[1])]
    return np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out], axis=1)


def _compare_binning(got_err, got_tau, ref_err, ref_tau, layout, figs):
    for l in range(ref_err.shape[0]):
        for s in range(ref_err.shape[1]):
            for off, ln in _rows(layout):
                sl = slice(off, off + ln)
                top = ref_err[l, s, sl].max()
                figs["err"] = max(figs.get("err", 0.0), np.abs(got_err[l, s, sl] - ref_err[l, s, sl]).max() / top)
    figs["tau"] = max(figs.get("tau", 0.0), np.abs(got_tau / ref_tau - 1.0).max())


def test_binning_on_synthetic_bins():
    from detqmc_amd import binning_analysis
    ctx = _context(NSLOTS)
    try:
        st0 = _open_series(ctx, NSLOTS, 3, BIG)
        S = st0.sample_len
        layout = [ctx.series_layout(p) for p in range(5)]
        bins, open_bin, w, m2 = _synthetic(NSLOTS, S, NBINS, 2)
        st = _state(st0, flags=TRACK, bins_closed=NBINS, sweeps_in_open_bin=2, samples=125)
        ctx.series_import(st, _pack(bins, open_bin, w, m2))
        before = _export(ctx)
        for levels in (0, 13, 6):                            # out of range twice; 40 >> 5 = 1: fewer than two merged bins at the top
            _raises(lambda: ctx.series_binning(levels))
            _raises(lambda: ctx.series_binning(levels, tau=False))
        err, tau = ctx.series_binning(4)
        err2, tau2 = ctx.series_binning(4)
        assert np.array_equal(err, err2) and np.array_equal(tau, tau2) and np.array_equal(ctx.series_binning(4, tau=False), err)
        assert _same(_export(ctx), before)                   # the bins are only read
        ref_err, ref_tau = _binning_reference(bins, m2, 4, 3, 125)
        assert ref_err.shape == err.shape == tau.shape == (4, NSLOTS, S)
        # the data: every row spreads, and the errors of a row are of one size -- within a factor of 10 while a level has ten bins or
        # more; an error from the five bins of level 3 scatters like a chi with 4 degrees of freedom, a factor of 100 covers a row of it
        mean0 = bins.mean(axis=0)
        for s in range(NSLOTS):
            for off, ln in _rows(layout):
                sl = slice(off, off + ln)
                assert np.abs(bins[:, s, sl] - mean0[s, sl]).max() > 1e-3 * np.abs(mean0[s, sl]).max()
                for l in range(4):
                    assert ref_err[l, s, sl].max() < (10.0 if l < 3 else 100.0) * ref_err[l, s, sl].min(), (l, s, off)
        # the two numpy forms against each other set the bound of tau
        e_pkg, t_pkg = binning_analysis(bins, 3, variance=m2 / 124.0)
        cpu = np.abs(t_pkg[:4] / ref_tau - 1.0).max()
        tau_bound = max(100.0 * cpu, 1e-9)
        figs = {}
        _compare_binning(err, tau, ref_err, ref_tau, layout, figs)
        print(f"binning, 40 bins, 4 levels: err {figs['err']:.2e} of the row's largest error (bound 1e-10); tau {figs['tau']:.2e} relative, "
              f"the two numpy forms differ by {cpu:.2e} (bound {tau_bound:.2e})")
        assert figs["err"] <= 1e-10 and figs["tau"] <= tau_bound
        assert 0.05 < np.median(tau[0]) < 5.0
        # level l against the jackknife of the statistics kernel after l merges
        worst = 0.0
        for l in range(4):
            if l:
                ctx.series_rebin()
            serr = ctx.series_stats()[1]
            for s in range(NSLOTS):
                for off, ln in _rows(layout):
                    sl = slice(off, off + ln)
                    worst = max(worst, sr.rows_close(err[l, s, sl], serr[s, sl], 1e-10, ln))
        print(f"binning level l against series_stats after l calls of series_rebin: {worst:.2e} of the row's largest error (bound 1e-10)")

        # 37 bins, five levels: 37 >> 4 = 2; levels 1 .. 4 use 36, 36, 32, 32 bins and never see the tail
        bins37 = bins[:37].copy()
        st37 = _state(st, bins_closed=37)
        ctx.series_import(st37, _pack(bins37, open_bin, w, m2))
        e37, t37 = ctx.series_binning(5)
        r_err, r_tau = _binning_reference(bins37, m2, 5, 3, 125)
        figs = {}
        _compare_binning(e37, t37, r_err, r_tau, layout, figs)
        print(f"binning, 37 bins, 5 levels: err {figs['err']:.2e} (bound 1e-10), tau {figs['tau']:.2e} (bound {tau_bound:.2e})")
        assert figs["err"] <= 1e-10 and figs["tau"] <= tau_bound
        for alter, same_from in ((36, 1), (33, 3)):
            other = bins37.copy()
            other[alter] += 1.0
            ctx.series_import(st37, _pack(other, open_bin, w, m2))
            eo, to = ctx.series_binning(5)
            assert np.array_equal(eo[same_from:], e37[same_from:]) and np.array_equal(to[same_from:], t37[same_from:]), alter
            assert not np.array_equal(eo[same_from - 1], e37[same_from - 1]), alter        # the altered bin did go in
        _raises(lambda: ctx.series_binning(6))

        # tau needs the variance, and at least two samples
        ctx.series_import(_state(st, flags=0), _pack(bins, open_bin))
        _raises(lambda: ctx.series_binning(2))
        assert np.array_equal(ctx.series_binning(2, tau=False), err[:2])
        ctx.series_import(_state(st, samples=1), _pack(bins, open_bin, w, m2))
        _raises(lambda: ctx.series_binning(2))
        # no variance in an element: tau is NaN there, the errors are untouched
        m2z = m2.copy()
        m2z[1, 5] = 0.0
        ctx.series_import(st, _pack(bins, open_bin, w, m2z))
        ez, tz = ctx.series_binning(4)
        assert np.array_equal(ez, err) and np.isnan(tz[:, 1, 5]).all() and np.isnan(tz).sum() == 4
        ctx.series_end()
    finally:
        ctx.close()

    # a chain of a batch gives the bits of the same chain alone
    one = _context(1)
    try:
        st1 = _open_series(one, 1, 3, BIG)
        for s in range(NSLOTS):
            one.series_import(_state(st1, flags=TRACK, bins_closed=NBINS, sweeps_in_open_bin=2, samples=125),
                              _pack(bins[:, s], open_bin[s], w[s], m2[s]))
            e1, t1 = one.series_binning(4)
            assert np.array_equal(e1[:, 0], err[:, s]) and np.array_equal(t1[:, 0], tau[:, s]), s
        one.series_end()
    finally:
        one.close()


# ---- host level -----------------------------------------------------------------------------------------------------------------------
H_NFREQ, H_BIN, H_MAXBINS = 2, 2, 4
H_NAMES = ("sdwCorr", "sdwSq", "sdwTau", "currentXTau", "currentYTau")
H_R = (-1.0, -0.9, -0.8, -0.7)
H_ROUTE = [1, 2, 3, 0]
H_BEFORE, H_AFTER = 3, 6
TOL = 1e-10                                                  # test_checkpoint_resume_continues_the_same_chain: a resumed chain recomputes G


def _host_params(rvals):
    from detqmc_amd import SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", fermionMeasurements=True,
                  equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=True, timeDisplacedEverySlice=True, rngSeed=4711)
    return [dataclasses.replace(p, simindex=b, r=r) for b, r in enumerate(rvals)]


def _f64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


def _host_snapshot(batch):
    """state, route, {name: [slot][bin][len]} and the exported open bin, w, m2 [slot][S] of all kernel contexts"""
    st = _st(batch.series_state())
    nb = st["bins_closed"]
    ex = [_export(kc) for kc in batch.kernel_contexts()]
    return dict(state=st, route=batch.series_route(),
                bins={nm: np.array([_f64(batch.chain(b).series_bins(nm)).reshape(nb, -1) for b in range(len(batch))]) if nb else None
                      for nm in H_NAMES},
                **{k: np.concatenate([e[k] for e in ex]) for k in ("open", "w", "m2")})


def _same_snapshot(a, b):
    return (a["state"] == b["state"] and a["route"] == b["route"] and all(np.array_equal(a[k], b[k]) for k in ("open", "w", "m2"))
            and all(np.array_equal(a["bins"][nm], b["bins"][nm]) for nm in H_NAMES))


def _sweeps_after(batch):
    snaps = []
    for _ in range(H_AFTER):
        batch.sweep(True)
        snaps.append(_host_snapshot(batch))
    return snaps, [batch.chain(b).phi for b in range(len(batch))], [batch.chain(b).info.rngDrawn for b in range(len(batch))]


def test_checkpointed_run_continues_the_series(tmp_path):
    from detqmc_amd import DetSDWBatch
    ck, sf = tmp_path / "state.ckpt", tmp_path / "series.bin"
    a = DetSDWBatch(_host_params(H_R), sub_batches=2)
    try:
        a.sweepThermalization()                              # with the three measurement sweeps an even number: the resume rule of save_state
        a.series_begin(H_BIN, H_MAXBINS, H_NFREQ, auto_rebin=True, track_variance=True)
        a.series_route(H_ROUTE)
        for _ in range(H_BEFORE):
            a.sweep(True)
        a.save_state(ck)
        a.series_save(sf)
        saved = _host_snapshot(a)
        assert saved["state"] == dict(saved["state"], bins_closed=1, sweeps_in_open_bin=1, bin_size=H_BIN, samples=3, rebins=0, nb=4,
                                      flags=AUTO | TRACK)
        snaps_a, phi_a, rng_a = _sweeps_after(a)
    finally:
        a.close()
    b = DetSDWBatch(_host_params(H_R), sub_batches=1)
    try:
        b.load_state(ck)
        b.series_begin(H_BIN, H_MAXBINS, H_NFREQ)
        b.series_load(sf)
        assert _same_snapshot(_host_snapshot(b), saved)
        snaps_b, phi_b, rng_b = _sweeps_after(b)
    finally:
        b.close()
    assert rng_a == rng_b and all(np.array_equal(x, y) for x, y in zip(phi_a, phi_b))
    want = [(2, 2, 0), (2, 2, 1), (3, 2, 0), (3, 2, 1), (2, 4, 0), (2, 4, 1)]           # (bins closed, bin size, sweeps in the open bin)
    worst = 0.0
    for i, (sa, sb) in enumerate(zip(snaps_a, snaps_b)):
        assert sa["state"] == sb["state"] and sa["route"] == sb["route"] == H_ROUTE
        assert (sa["state"]["bins_closed"], sa["state"]["bin_size"], sa["state"]["sweeps_in_open_bin"]) == want[i]
        for nm in H_NAMES:
            rowlen = 16 if nm in H_NAMES[:2] else 32
            if i < 4:                                        # bin 0 was closed before the save and is not merged yet
                assert np.array_equal(sa["bins"][nm][:, 0], sb["bins"][nm][:, 0]), (i, nm)
                assert np.array_equal(sa["bins"][nm][:, 0], saved["bins"][nm][:, 0]), (i, nm)
            worst = max(worst, sr.rows_close(sb["bins"][nm], sa["bins"][nm], TOL, rowlen))
        for k in ("w", "m2"):
            worst = max(worst, sr.rows_close(sb[k], sa[k], TOL, N))
    print(f"resumed against uninterrupted series, bins, w and m2 after every sweep: {worst:.2e} of the row's scale (bound {TOL:.0e})")


def test_refused_loads_and_the_statistics_cache(tmp_path):
    from detqmc_amd import DetSDWBatch, binning_analysis, jackknife
    good, two, trunc, parts, early = (tmp_path / f for f in ("good.bin", "two.bin", "trunc.bin", "parts.bin", "early.bin"))
    small = DetSDWBatch(_host_params(H_R[:2]), sub_batches=1)
    try:
        small.sweepThermalization()
        small.series_begin(1, 8, H_NFREQ, track_variance=True)
        small.sweep(True)
        small.series_save(two)
    finally:
        small.close()
    batch = DetSDWBatch(_host_params(H_R), sub_batches=2)
    try:
        batch.sweepThermalization()
        _raises(lambda: batch.series_load(two))              # no series is open
        _raises(batch.series_state)
        _raises(lambda: batch.series_begin(1, 7, H_NFREQ, auto_rebin=True))      # an odd maxBins: refused, and no series stays open
        assert not batch.series_is_open()
        batch.series_begin(1, 8, H_NFREQ, track_variance=True)
        batch.series_route(H_ROUTE)
        for i in range(4):
            batch.sweep(True)
            if i == 1:
                batch.series_save(early)                     # two bins of one sample
                early_bins = _host_snapshot(batch)["bins"]["sdwSq"]
        batch.series_save(good)
        raw = good.read_bytes()
        trunc.write_bytes(raw[:-8])
        edited = bytearray(raw)                              # the parts field of the header: magic [8], version int32, then the ints of the state
        assert int.from_bytes(edited[24:28], "little") == PARTS
        edited[24:28] = (PARTS & ~16).to_bytes(4, "little")
        parts.write_bytes(bytes(edited))
        snap = _host_snapshot(batch)
        assert snap["state"]["bins_closed"] == 4 and snap["state"]["samples"] == 4
        for f in (two, parts, trunc, tmp_path / "missing.bin"):
            _raises(lambda: batch.series_load(f))
            assert _same_snapshot(_host_snapshot(batch), snap), f.name

        # statistics and binning of every slot against the package's numpy forms on the slot's bins
        S = snap["state"]["sample_len"]
        sl = slice(7 * N, 8 * N)                             # S_sdw(q) inside a sample: the equal-time part comes first, C_X(d) [5][N] then S_X(q) [5][N]
        mean, err = batch.series_stats_all("sdwSq")
        berr, btau = batch.series_binning_all("sdwSq", 2)
        assert berr.shape == btau.shape == (4, 2, N) and snap["m2"].shape == (4, S)
        cpu = 0.0
        for b in range(4):
            bins = batch.chain(b).series_bins("sdwSq")
            assert np.array_equal(bins, snap["bins"]["sdwSq"][b])
            rmean, rerr = jackknife(bins)
            sr.rows_close(mean[b], rmean, 1e-13, N)
            sr.rows_close(err[b], rerr, 1e-10, N)
            perr, ptau = binning_analysis(bins, 1, variance=snap["m2"][b, sl] / 3.0)
            rref = slr.binning(bins, 1, 2, m2=snap["m2"][b, sl], samples=4)
            cpu = max(cpu, np.abs(ptau / rref[1] - 1.0).max())
            for l in range(2):
                sr.rows_close(berr[b, l], perr[l], 1e-10, N)
            assert np.abs(btau[b] / ptau - 1.0).max() <= max(100.0 * cpu, 1e-9)
            e1, t1 = batch.chain(b).series_binning("sdwSq", 2)
            assert np.array_equal(e1, berr[b]) and np.array_equal(t1, btau[b])
            assert np.abs(berr[b, 0] - err[b]).max() <= 1e-10 * err[b].max()
        # statistics, an explicit re-bin, statistics: those of the merged bins
        batch.series_rebin()
        st = _st(batch.series_state())
        assert (st["bins_closed"], st["bin_size"], st["rebins"]) == (2, 2, 1)
        mean2, err2 = batch.series_stats_all("sdwSq")
        berr2, _ = batch.series_binning_all("sdwSq", 1)
        for b in range(4):
            merged = slr.rebinned(snap["bins"]["sdwSq"][b])
            assert np.array_equal(batch.chain(b).series_bins("sdwSq"), merged)
            rmean, rerr = jackknife(merged)
            sr.rows_close(mean2[b], rmean, 1e-13, N)
            sr.rows_close(err2[b], rerr, 1e-10, N)
            sr.rows_close(berr2[b, 0], rerr, 1e-10, N)
            assert not np.array_equal(err2[b], err[b])
        # a load passes by the accumulate too.  Two closed bins are cached; the early file holds two OTHER bins: no stale statistics
        batch.series_load(early)
        assert _st(batch.series_state())["bins_closed"] == 2 and batch.series_route() == H_ROUTE
        mean_e, err_e = batch.series_stats_all("sdwSq")
        for b in range(4):
            assert np.array_equal(batch.chain(b).series_bins("sdwSq"), early_bins[b])
            rmean, rerr = jackknife(early_bins[b])
            sr.rows_close(mean_e[b], rmean, 1e-13, N)
            sr.rows_close(err_e[b], rerr, 1e-10, N)
            assert not np.array_equal(err_e[b], err2[b])
        # back to the four bins, and the statistics are those of the four bins again
        batch.series_load(good)
        assert _same_snapshot(_host_snapshot(batch), snap)
        mean3, err3 = batch.series_stats_all("sdwSq")
        berr3, btau3 = batch.series_binning_all("sdwSq", 2)
        assert np.array_equal(mean3, mean) and np.array_equal(err3, err) and np.array_equal(berr3, berr) and np.array_equal(btau3, btau)
        batch.series_end()
        _raises(lambda: batch.series_load(good))             # no series is open
    finally:
        batch.close()
