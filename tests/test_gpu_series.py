"""The measurement series on the device (dqmc_series_*, DetSDWBatch.series_*): bins of samples accumulated over sweeps, jackknife
statistics and the jackknifed correlation ratio and rho_s, against numpy (tests/series_reference.py) on the blocks and bins the device
itself returns.

Tolerances (every comparison prints its figure first; a "row" is one [N] vector of the equal-time part or one (component, frequency)
row of a Matsubara part, and a figure is the largest deviation divided by the largest magnitude of the reference's row):
  bins, C(d) and Matsubara parts   bit for bit: one division resp. the same kernel on the same input, then (0 + a + b) / 2
  bins, S(q)                       1e-12: N cosine terms of one sign pattern summed in another order
  mean                             1e-13: B = 3 terms, a different rounding of the division
  err, errors of R and rho_s       1e-10 of the row's largest error, after asserting that the bins differ by more than 1e-3 of the
                                   row's scale and |S_X(Q)| > 1e-3 of its row's scale: the cancellation in x_(b) - mean then costs at
                                   most ~ 1e-13 relative
  values of R and rho_s            1e-12 absolute: O(1) functions of three or four means that agree to 1e-13
  host level, bins                 1e-14: the pair means of the vectors the host layer formed from the same blocks"""
import dataclasses
import functools

import numpy as np
import pytest

import series_reference as sr

pytestmark = pytest.mark.gpu

M, S_STAB, NCH, BIN, MAXBINS, NFREQ, PARTS = 20, 5, 3, 2, 3, 3, 31
NCOMP = (2, 2, 3, 2)
EINVAL = -1


def _phi(N, seed, amp):
    phi = np.random.default_rng(seed).uniform(-amp, amp, (M + 1, N, 2))
    phi[0] = 0.0
    return phi


def _context(L, nchains):
    from detqmc_amd import KernelContext
    return KernelContext(2, L, M, S_STAB, 0.1, delaySteps=4, stabilisation="qr", nchains=nchains, timeDisplaced=2, tdParticleHole=True,
                         tdCurrent=True, tdEverySlice=True)


def _fill(ctx, phis):
    """new fields, then one down pass without updates that refills every block: the equal-time block from the slices of the top
    segment (count = s), the every-slice blocks from all segments and both ends"""
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


def _blocks(ctx, nchains):
    """per chain: (equal-time block, the four fine blocks, G)"""
    out = []
    for b in range(nchains):
        ctx.select_chain(b)
        out.append((ctx.measure_eq_read(), [ctx.measure_td_fine_read(ch) for ch in range(4)], ctx.g))
    ctx.select_chain(0)
    return out


def _expected_sample(ctx, nchains, blocks, layout):
    """[chain][S] from the existing readers: C(d) and numpy's S(q), and the Matsubara kernel's own host output"""
    N, L = ctx.N, ctx.L
    S = layout[4][0] + layout[4][1]
    out = np.zeros((nchains, S))
    mats = [ctx.measure_td_matsubara(ch, NFREQ) for ch in range(4)]
    for b in range(nchains):
        c = sr.eq_correlators_from_block(blocks[b][0], N)
        out[b, :5 * N] = c.ravel()
        out[b, 5 * N:10 * N] = sr.structure_factor_ref(c, L).ravel()
        for ch in range(4):
            off, ln = layout[1 + ch]
            out[b, off:off + ln] = mats[ch][b].ravel().view(np.float64)
    return out


def _raises(fn, code=EINVAL):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == code
    return True


@functools.lru_cache(maxsize=None)
def _scenario(L, chains):
    """chains = tuple of chain indices (seeds) the context holds.  Six fills and add_sweep calls; returns what the tests compare."""
    N, nb = L * L, len(chains)
    ctx = _context(L, nb)
    rec = dict(N=N, L=L, nb=nb, checks={})
    try:
        # the field amplitude grows from fill to fill: the charge correlator hardly depends on the configuration at a fixed amplitude
        # (5e-4 of its scale between two draws from [-1, 1]), and statistics of nearly equal bins would test nothing
        fills = [[_phi(N, 1000 * L + 10 * i + c, 0.5 + 0.5 * i) for c in chains] for i in range(BIN * MAXBINS + 1)]
        _fill(ctx, fills[0])
        ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS)
        rec["checks"]["second_begin"] = _raises(lambda: ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS))
        layout = [ctx.series_layout(p) for p in range(5)]
        rec["layout"] = layout
        assert layout[0] == (0, 10 * N)
        for ch in range(4):
            assert layout[1 + ch] == (layout[ch][0] + layout[ch][1], NCOMP[ch] * NFREQ * N * 2)
        S = layout[4][0] + layout[4][1]
        assert ctx.series_info() == (0, 0, S)
        samples = []
        for i in range(BIN * MAXBINS):
            if i:
                _fill(ctx, fills[i])
            before = _blocks(ctx, nb)
            samples.append(_expected_sample(ctx, nb, before, layout))
            ctx.series_add_sweep()
            after = _blocks(ctx, nb)
            for x, y in zip(before, after):                  # the series reads the blocks only
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])
                assert all(np.array_equal(p, q) for p, q in zip(x[1], y[1]))
            assert ctx.series_info() == ((i + 1) // BIN, (i + 1) % BIN, S)
            if i == 1:                                       # one closed bin
                rec["checks"]["stats_one_bin"] = _raises(ctx.series_stats) and _raises(ctx.series_derived)
                one = ctx.series_bins()
                ctx.measure_reset()                          # keeps the series ...
                assert ctx.series_info() == (1, 0, S) and np.array_equal(ctx.series_bins(), one)
                rec["checks"]["empty_blocks"] = _raises(ctx.series_add_sweep)     # ... and empties the blocks
                assert ctx.series_info() == (1, 0, S) and np.array_equal(ctx.series_bins(), one)
        _fill(ctx, fills[-1])
        bins = []
        for b in range(nb):
            ctx.select_chain(b)
            bins.append(ctx.series_bins())
        rec["checks"]["full"] = _raises(ctx.series_add_sweep)
        assert ctx.series_info() == (MAXBINS, 0, S)
        for b in range(nb):
            ctx.select_chain(b)
            assert np.array_equal(ctx.series_bins(), bins[b])
            assert np.array_equal(ctx.series_bins(1, 1)[0], bins[b][1])
        ctx.select_chain(0)
        _raises(lambda: ctx.series_bins(2, 2))
        rec["bins"] = np.array(bins)                         # [chain][bin][S]
        rec["samples"] = np.array(samples)                   # [sweep][chain][S]
        rec["stats"] = ctx.series_stats()
        rec["stats2"] = ctx.series_stats()
        rec["derived"] = ctx.series_derived()
        rec["derived2"] = ctx.series_derived()
        ctx.series_end()
        _raises(ctx.series_info)
        ctx.series_begin(1, 2, 0, 1)                         # a new series after the end: equal-time part only, nfreq ignored
        assert ctx.series_info() == (0, 0, 10 * N)
        _raises(lambda: ctx.series_layout(4))
    finally:
        ctx.close()
    return rec


def _rows(rec):
    """(offset, row length) of every row of a sample"""
    N = rec["N"]
    rows = [(x * N, N) for x in range(10)]
    for ch in range(4):
        off, ln = rec["layout"][1 + ch]
        rows += [(off + r * 2 * N, 2 * N) for r in range(ln // (2 * N))]
    return rows


@pytest.mark.parametrize("L", [4, 6])
def test_bins(L):
    rec = _scenario(L, tuple(range(NCH)))
    N = rec["N"]
    smp, bins = rec["samples"], rec["bins"]
    worst = 0.0
    for b in range(NCH):
        for k in range(MAXBINS):
            want = (smp[2 * k, b] + smp[2 * k + 1, b]) / 2
            got = bins[b, k]
            assert np.array_equal(got[:5 * N], want[:5 * N]), (b, k)
            assert np.array_equal(got[10 * N:], want[10 * N:]), (b, k)
            assert np.abs(want[:5 * N]).max() > 1e-6 and np.abs(want[10 * N:]).max() > 1e-6
            worst = max(worst, sr.rows_close(got[5 * N:10 * N], want[5 * N:10 * N], 1e-12, N))
    print(f"L={L}: C(d) and Matsubara parts of {NCH * MAXBINS} bins bit-identical; S(q) part: {worst:.2e} of the row's magnitude (bound 1e-12)")
    assert all(rec["checks"][k] for k in ("second_begin", "stats_one_bin", "empty_blocks", "full"))


@pytest.mark.parametrize("L", [4, 6])
def test_statistics_and_derived(L):
    rec = _scenario(L, tuple(range(NCH)))
    N = rec["N"]
    bins = rec["bins"]
    mean, err = rec["stats"]
    assert np.array_equal(mean, rec["stats2"][0]) and np.array_equal(err, rec["stats2"][1])
    assert np.array_equal(rec["derived"][0], rec["derived2"][0]) and np.array_equal(rec["derived"][1], rec["derived2"][1])
    rows = _rows(rec)
    wm = we = 0.0
    for b in range(NCH):
        rmean, rerr = sr.jackknife(bins[b])
        for off, ln in rows:
            sl = slice(off, off + ln)
            scale = np.abs(rmean[sl]).max()
            spread = np.abs(bins[b][:, sl] - rmean[sl]).max()
            assert spread > 1e-3 * scale, (b, off, spread, scale)     # the samples differ: no comparison of zero errors
            wm = max(wm, sr.rows_close(mean[b, sl], rmean[sl], 1e-13, ln))
            we = max(we, sr.rows_close(err[b, sl], rerr[sl], 1e-10, ln))
    print(f"L={L}: mean {wm:.2e} (bound 1e-13), err {we:.2e} of the row's largest error (bound 1e-10)")
    val, derr = rec["derived"]
    assert val.shape == (NCH, 6)
    off3 = rec["layout"][4][0]
    fs = [functools.partial(lambda x, X, pair: sr.correlation_ratio(x[(5 + X) * N:(6 + X) * N], L, pairing=pair), X=X, pair=X >= 3) for X in range(5)]
    fs.append(lambda x: sr.rho_s(x[off3:off3 + 2 * N:2], x[off3 + NFREQ * 2 * N:off3 + NFREQ * 2 * N + 2 * N:2], L))
    ref = np.array([[sr.jackknife(bins[b], f) for f in fs] for b in range(NCH)])     # [chain][entry][value, err]
    for b in range(NCH):
        m_b = sr.jackknife(bins[b])[0]
        for X in range(5):
            row = m_b[(5 + X) * N:(6 + X) * N]
            Q = 0 if X >= 3 else (L // 2) * L + L // 2
            assert abs(row[Q]) > 1e-3 * np.abs(row).max(), (b, X)    # no ratio with a vanishing denominator
    dv = np.abs(val - ref[:, :, 0]).max()
    de = (np.abs(derr - ref[:, :, 1]).max(axis=0) / ref[:, :, 1].max(axis=0)).max()
    print(f"L={L}: R_X and rho_s: values {dv:.2e} (bound 1e-12), errors {de:.2e} of the entry's largest error (bound 1e-10); "
          f"R_sdw = {val[0, 2]:.6f} +- {derr[0, 2]:.6f}, rho_s = {val[0, 5]:.6f} +- {derr[0, 5]:.6f}")
    assert np.all(ref[:, :, 1] > 0.0)
    assert dv <= 1e-12 and de <= 1e-10


@pytest.mark.parametrize("L", [4, 6])
def test_chain_of_a_batch_equals_a_single_chain(L):
    rec = _scenario(L, tuple(range(NCH)))
    for b in range(NCH):
        one = _scenario(L, (b,))
        assert np.array_equal(one["bins"][0], rec["bins"][b]), b
        for k in (0, 1):
            assert np.array_equal(one["stats"][k][0], rec["stats"][k][b]), (b, k)
            assert np.array_equal(one["derived"][k][0], rec["derived"][k][b]), (b, k)


def test_begin_error_paths():
    from detqmc_amd import DetHubbard, HubbardParams, KernelContext
    L, N = 4, 16
    ctx = _context(L, 1)
    try:
        _raises(lambda: ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS))        # the equal-time block has never been enabled
        _raises(ctx.series_add_sweep)
        _raises(ctx.series_end)
        ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS & ~1)                    # the Matsubara parts alone
        assert ctx.series_info() == (0, 0, (2 + 2 + 3 + 2) * NFREQ * N * 2)
        _raises(lambda: ctx.series_layout(0))
        _raises(ctx.series_add_sweep)                                        # rows without a sample
        assert ctx.series_info()[:2] == (0, 0)
        ctx.series_end()
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_correlators(False)
        for bad in (dict(parts=0), dict(parts=32), dict(bin_size=0), dict(max_bins=1), dict(nfreq=0), dict(nfreq=M + 1)):
            kw = dict(dict(bin_size=BIN, max_bins=MAXBINS, nfreq=NFREQ, parts=PARTS), **bad)
            _raises(lambda: ctx.series_begin(**kw))
        _raises(ctx.series_info)
    finally:
        ctx.close()
    ctx = KernelContext(2, L, M, S_STAB, 0.1, delaySteps=4, stabilisation="qr")   # no every-slice blocks
    try:
        ctx.set_equal_time_correlators(True)
        _raises(lambda: ctx.series_begin(BIN, MAXBINS, NFREQ, 3))
        ctx.series_begin(BIN, MAXBINS, 0, 1)
        ctx.series_end()
    finally:
        ctx.close()
    rep = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        assert rep.lib.dqmc_series_begin(rep.lib.dethubbard_ctx(rep.h), BIN, MAXBINS, NFREQ, 1) == EINVAL
    finally:
        rep.close()


# ---- host level ----------------------------------------------------------------------------------------------------------------------
H_NFREQ, H_SWEEPS = 2, 6
H_NAMES = ("sdwCorr", "sdwSq", "sdwTau", "currentXTau", "currentYTau")


@functools.lru_cache(maxsize=None)
def _host_run(sub_batches, series, host_copy=True):
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", fermionMeasurements=True,
                  equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=True, timeDisplacedEverySlice=True, rngSeed=4711)
    batch = DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)], sub_batches=sub_batches)
    rec = dict(vec={nm: [] for nm in H_NAMES})
    try:
        assert batch.sub_batches == sub_batches
        batch.sweepThermalization()
        if series:
            batch.series_begin(BIN, MAXBINS, H_NFREQ, host_copy=host_copy)
            with pytest.raises(DqmcError):
                batch.series_begin(BIN, MAXBINS, H_NFREQ)
        for i in range(H_SWEEPS):
            batch.sweepThermalization()
            if i % 2:
                batch.sweep(False)
            batch.sweep(True)
            if series:
                assert batch.series_info()[:2] == ((i + 1) // BIN, (i + 1) % BIN)
            if series and not host_copy:
                with pytest.raises(DqmcError, match="NO_HOST_COPY"):
                    batch.chain(0).observable_vector("sdwCorr")
                with pytest.raises(DqmcError, match="NO_HOST_COPY"):
                    batch.chain(1).observable_vector("pairMinusSq")
                batch.chain(0).observable_vector("pairPlus")
            else:
                for nm in H_NAMES[:2]:
                    rec["vec"][nm].append([batch.chain(b).observable_vector(nm) for b in range(2)])
            for nm in H_NAMES[2:]:
                rec["vec"][nm].append(batch.matsubara_all(nm, H_NFREQ))
        rec["phi"] = [batch.chain(b).phi for b in range(2)]
        rec["rng"] = [batch.chain(b).info.rngDrawn for b in range(2)]
        if series:
            with pytest.raises(DqmcError, match="full"):
                batch.sweep(True)                            # refused before anything changes
            assert np.array_equal(batch.chain(0).phi, rec["phi"][0]) and batch.chain(0).info.rngDrawn == rec["rng"][0]
            rec["bins"] = {nm: [batch.chain(b).series_bins(nm) for b in range(2)] for nm in H_NAMES}
            rec["stats_all"] = {nm: batch.series_stats_all(nm) for nm in H_NAMES}
            rec["stats"] = {nm: [batch.chain(b).series_stats(nm) for b in range(2)] for nm in H_NAMES}
            rec["derived"] = {nm: batch.series_derived_all(nm) for nm in ("R_sdw", "rhoS", "R_pairPlus")}
            batch.series_end()
            batch.sweep(True)                                # the series is gone: sweeps go on, the vectors are back
            assert batch.chain(0).observable_vector("sdwCorr").any()
    finally:
        batch.close()
    return rec


def _f64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_series_vs_recorded_vectors(sub_batches):
    rec = _host_run(sub_batches, True)
    N, L = 16, 4
    for nm in H_NAMES:
        per_sweep = np.array([[_f64(np.asarray(v[b])).ravel() for b in range(2)] for v in rec["vec"][nm]])    # [sweep][chain][len]
        rowlen = N if nm in H_NAMES[:2] else 2 * N
        for b in range(2):
            want = (per_sweep[0::2, b] + per_sweep[1::2, b]) / 2
            got = _f64(rec["bins"][nm][b]).reshape(MAXBINS, -1)
            fb = sr.rows_close(got, want, 1e-14, rowlen)
            rmean, rerr = sr.jackknife(want)
            mean, err = (_f64(x).ravel() for x in rec["stats"][nm][b])
            assert np.abs(want - rmean).max() > 1e-3 * np.abs(rmean).max()
            fm = sr.rows_close(mean, rmean, 1e-13, rowlen)
            fe = sr.rows_close(err, rerr, 1e-10, rowlen)
            print(f"sub_batches={sub_batches} {nm} chain {b}: bins {fb:.2e} (1e-14), mean {fm:.2e} (1e-13), err {fe:.2e} (1e-10)")
            for k in (0, 1):
                assert np.array_equal(rec["stats_all"][nm][k][b], rec["stats"][nm][b][k])
    sq = np.array(rec["vec"]["sdwSq"])                                   # [sweep][chain][N]
    lx, ly = (np.array(rec["vec"][nm])[:, :, 0, :] for nm in ("currentXTau", "currentYTau"))    # [sweep][chain][N] at frequency 0
    for b in range(2):
        sb = (sq[0::2, b] + sq[1::2, b]) / 2
        assert np.all(np.abs(sb[:, 2 * L + 2]) > 1e-3 * np.abs(sb).max())
        rv, re = sr.jackknife(sb, lambda s: sr.correlation_ratio(s, L))
        v, e = (x[b] for x in rec["derived"]["R_sdw"])
        cur = np.concatenate([(lx[0::2, b] + lx[1::2, b]) / 2, (ly[0::2, b] + ly[1::2, b]) / 2], axis=1)
        qv, qe = sr.jackknife(cur.real, lambda x: sr.rho_s(x[:N], x[N:], L))
        w, f = (x[b] for x in rec["derived"]["rhoS"])
        print(f"chain {b}: R_sdw {v:.10f} +- {e:.3e} (numpy {rv:.10f} +- {re:.3e}), rho_s {w:.10f} +- {f:.3e} (numpy {qv:.10f} +- {qe:.3e})")
        assert re > 0 and qe > 0
        assert abs(v - rv) <= 1e-12 and abs(e - re) <= 1e-10 * re
        assert abs(w - qv) <= 1e-12 and abs(f - qe) <= 1e-10 * qe
        assert np.isfinite(rec["derived"]["R_pairPlus"][0][b])


def test_host_series_changes_no_trajectory_and_needs_no_host_copy():
    plain, with_series, no_copy, two = _host_run(1, False), _host_run(1, True), _host_run(1, True, False), _host_run(2, True)
    for other in (with_series, no_copy, two):
        assert other["rng"] == plain["rng"]
        assert all(np.array_equal(a, b) for a, b in zip(other["phi"], plain["phi"]))
    for nm in H_NAMES:
        for k in (0, 1):
            assert np.array_equal(no_copy["stats_all"][nm][k], with_series["stats_all"][nm][k]), nm
            assert np.array_equal(two["stats_all"][nm][k], with_series["stats_all"][nm][k]), nm     # the grouping changes no bit
        assert all(np.array_equal(a, b) for a, b in zip(no_copy["bins"][nm], with_series["bins"][nm]))
    for nm in ("sdwCorr", "sdwTau"):                         # the series changes no observable of a sweep either
        assert np.array_equal(np.array(plain["vec"][nm]), np.array(with_series["vec"][nm]))


def test_host_series_needs_an_option():
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    p = SDWParams(opdim=2, L=4, beta=1.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    batch = DetSDWBatch([p])
    try:
        with pytest.raises(DqmcError, match="equalTimeCorrelators or timeDisplacedEverySlice"):
            batch.series_begin(2, 3)
        with pytest.raises(DqmcError):
            batch.series_info()
    finally:
        batch.close()
    batch = DetSDWBatch([dataclasses.replace(p, equalTimeCorrelators=True)])
    try:
        batch.series_begin(1, 2)                             # nfreq ignored: no every-slice channel
        batch.sweep(True); batch.sweep(True)
        mean, err = batch.series_stats_all("chargeSq")
        assert mean.shape == (1, 16) and np.all(err >= 0) and err.any()
        with pytest.raises(DqmcError):
            batch.series_stats_all("sdwTau")
        with pytest.raises(DqmcError):
            batch.series_derived_all("rhoS")
        assert np.isfinite(batch.series_derived_all("R_charge")[0]).all()
    finally:
        batch.close()
