"""The order-parameter part of the measurement series on the device (DQMC_SERIES_PHI, k_series_phi_sample, dqmc_series_phi_derived_host,
DetSDWBatch.series_begin(phi=True)): chi_phi(q, i omega_n) and the five scalars formed from the field itself, against the direct sum of
tests/series_phi_reference.py, and everything downstream of the sample (bins, routed accumulate, re-binning, running variance, export /
import, statistics) against the numpy restatements the other series tests use, on the device's own samples.

Tolerance of a sample (every comparison prints its figure first).  With eps = 2^-52, a = max |phi| and K = m N,
    |device - reference| <= 4 opdim (K + 64) eps a^2      per chi element and per quadratic scalar.
Derivation: A_d(n, q) is a K-term sum of products phi * phase, |phi| <= a, |phase| <= 1, divided by K.  Summed in any order with phases
from a table good to a few eps, its error is at most (K + 64) eps a: K - 1 additions, and the 64 covers the products, the table, the
two spatial stages and the division.  |A_d| <= a, so | |A_d + dA_d|^2 - |A_d|^2 | <= 2 a (K + 64) eps a to first order; the sum over d
gives opdim of them, and the last factor 2 is for the rounding of the numpy reference itself.  It is a worst-case bound; a typical
deviation is some 10^3 times smaller.  For |phibar| = sqrt(chi(0, 0)) the bound is divided by the value (d sqrt(x) = dx / (2 sqrt(x))),
for |phibar|^4 = (|phibar|^2)^2 it is multiplied by 2 a^2 (d x^2 = 2 x dx, x <= a^2).  The host's normMeanPhi and associatedEnergy sum
in another order and get the same bound.
Statistics: the tolerances tests/test_gpu_series.py states for the same operations -- mean 1e-13 of the row's magnitude, err and the
errors of derived quantities 1e-10 of the largest error, derived values 1e-12.
Bins, routed bins, auto re-binned bins, the open bin, the running mean w and export / import: bit for bit.  The running m2 is compared
bit for bit too, against the recurrence of series_long_reference.welford with the update m2 += d (x - w) rounded once: k_series_welford
contracts it into one fused multiply-add (the docstring of tests/test_gpu_series_long.py records the effect), so the plain numpy
recurrence, which rounds twice, cannot give its bits; whether it does is printed as a diagnostic."""
import dataclasses
import fractions
import functools

import numpy as np
import pytest

import series_long_reference as slr
import series_phi_reference as spr
import series_reference as sr
import series_route_reference as srr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
EINVAL = -1
PHI = 64


def _raises(fn, code=EINVAL):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == code
    return True


def _field(seed, m, N, opdim, amp=1.0, offset=0.0):
    phi = amp * (offset + np.random.default_rng(seed).uniform(-1.0, 1.0, (m + 1, N, opdim)))
    phi[0] = 0.0
    return phi


def _ctx(opdim, L, m, nchains=1):
    from detqmc_amd import KernelContext
    s = 5 if m % 5 == 0 and m > 5 else (m + 1) // 2
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, stabilisation="qr", nchains=nchains)


def _set(ctx, phis):
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)


def _all_bins(ctx, nchains):
    """[slot][bin][S]"""
    out = []
    for b in range(nchains):
        ctx.select_chain(b)
        out.append(ctx.series_bins())
    ctx.select_chain(0)
    return np.array(out)


def _compare(got, phi, L, nfreq, label, want=None):
    """one part vector (chi then scalars) against the reference at the bound of the module docstring; prints the figures"""
    m, N, opdim = phi.shape[0] - 1, phi.shape[1], phi.shape[2]
    a = np.abs(phi[1:]).max()
    tol = spr.rounding_bound(opdim, m, N, a)
    if want is None:
        want = spr.sample_direct(phi, L, nfreq)
    nc = nfreq * N
    assert got.shape == want.shape == (nc + 5,)
    dchi = np.abs(got[:nc] - want[:nc]).max()
    dsc = np.abs(got[nc:] - want[nc:])
    bounds = np.array([tol / want[nc], tol, tol * 2.0 * a * a, tol, tol])
    print(f"{label}: chi {dchi:.2e}, scalars " + " ".join(f"{d:.2e}/{b:.2e}" for d, b in zip(dsc, bounds)) + f" (bound {tol:.2e}, a = {a:.3f})")
    assert np.abs(want[:nc]).max() > 0 and dchi <= tol
    assert np.all(dsc <= bounds)
    assert got[nc + 1] == got[0]                            # |phibar|^2 carries the bits of chi(0, 0)


# ---- kernel level: the sample ---------------------------------------------------------------------------------------------------------
# (opdim, L, m, nfreq, seeds of the chains): N below a wave; N no multiple of 64, odd m, nfreq = m; three chains; N > 256 with two
# frequency groups (five frequencies, four to a group)
SHAPES = [(1, 4, 10, 3, (0,)), (3, 6, 7, 7, (0,)), (2, 16, 20, 3, (0, 1, 2)), (1, 20, 5, 5, (0,))]


def _shape_field(opdim, L, m, seed):
    return _field(1000 * L + 10 * m + seed, m, L * L, opdim, amp=0.5 + 0.5 * seed)


@functools.lru_cache(maxsize=None)
def _sample_case(opdim, L, m, nfreq, seeds):
    N, nb = L * L, len(seeds)
    ctx = _ctx(opdim, L, m, nb)
    rec = dict(phis=[_shape_field(opdim, L, m, sd) for sd in seeds])
    try:
        _set(ctx, rec["phis"])
        if (L, m) == (20, 5):
            _raises(lambda: ctx.series_begin(1, 4, 9, PHI))  # nfreq is not clipped to m
            _raises(ctx.series_info)
        ctx.series_begin(1, 4, nfreq, PHI)
        rec["layout"] = ctx.series_layout(6)
        rec["info"] = ctx.series_info()
        rec["state"] = (ctx.series_state().parts, ctx.series_state().nfreq)
        for p in range(6):
            _raises(lambda: ctx.series_layout(p))
        ctx.series_add_sweep()
        ctx.series_form_sample()
        ctx.series_form_sample()                             # forming twice is allowed; the second accumulate takes the last one
        ctx.series_accumulate()
        rec["bins"] = _all_bins(ctx, nb)                     # [chain][2][S]: bin_size 1, so the bins are the samples
        ctx.series_end()
    finally:
        ctx.close()
    return rec


@pytest.mark.parametrize("opdim,L,m,nfreq,seeds", SHAPES)
def test_sample_against_the_direct_sum(opdim, L, m, nfreq, seeds):
    rec = _sample_case(opdim, L, m, nfreq, seeds)
    N = L * L
    assert rec["layout"] == (0, nfreq * N + 5) and rec["info"] == (0, 0, nfreq * N + 5) and rec["state"] == (PHI, nfreq)
    for b in range(len(seeds)):
        assert np.array_equal(rec["bins"][b][0], rec["bins"][b][1]), b      # two calls, identical bits
        _compare(rec["bins"][b][0], rec["phis"][b], L, nfreq, f"opdim {opdim} L {L} m {m} nfreq {nfreq} chain {b}")


def test_chain_of_a_batch_equals_a_single_chain():
    opdim, L, m, nfreq, seeds = SHAPES[2]
    rec = _sample_case(opdim, L, m, nfreq, seeds)
    for b, sd in enumerate(seeds):
        one = _sample_case(opdim, L, m, nfreq, (sd,))
        assert np.array_equal(one["bins"][0], rec["bins"][b]), b


def test_plane_wave_on_the_device():
    opdim, L, m, n0, q0, nfreq = 3, 6, 7, 1, (1, 2), 3
    N, K = L * L, 7 * 36
    ctx = _ctx(opdim, L, m)
    try:
        ctx.set_fields(spr.plane_wave(L, m, opdim, n0, q0))
        ctx.series_begin(1, 2, nfreq, PHI)
        ctx.series_add_sweep()
        chi = ctx.series_bins()[0][:nfreq * N].reshape(nfreq, N)
        ctx.series_end()
    finally:
        ctx.close()
    peak = q0[1] * L + q0[0]
    rel = abs(chi[n0, peak] - 0.25 * opdim) / (0.25 * opdim)
    rest = chi.copy()
    rest[n0, peak] = 0.0
    tol = spr.rounding_bound(opdim, m, N, 1.0)
    print(f"plane wave: peak {chi[n0, peak]!r} ({rel:.2e} relative, bound {(K + 64) * EPS:.2e}), largest other element {rest.max():.2e} (bound {tol:.2e})")
    assert rel <= (K + 64) * EPS and rest.max() <= tol
    assert chi[n0, ((-q0[1]) % L) * L + (-q0[0]) % L] <= tol and chi[n0, q0[0] * L + q0[1]] <= tol


# ---- kernel level: next to the fermionic parts ---------------------------------------------------------------------------------------
F_M, F_S, F_NFREQ = 20, 5, 3


def _fermionic_fill(ctx, phi):
    """tests/test_gpu_series.py: new fields, then one down pass without updates that refills every block"""
    m, s, n = ctx.m, ctx.s, ctx.n
    ctx.set_fields(phi)
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


def test_part_alone_equals_the_part_behind_the_fermionic_parts():
    from detqmc_amd import KernelContext
    L, N = 4, 16
    ctx = KernelContext(2, L, F_M, F_S, 0.1, delaySteps=4, stabilisation="qr", timeDisplaced=2, tdParticleHole=True, tdCurrent=True,
                        tdEverySlice=True)
    try:
        phi = _field(77, F_M, N, 2)
        _fermionic_fill(ctx, phi)
        _raises(lambda: ctx.series_begin(1, 2, F_NFREQ, 32 | PHI))
        ctx.series_begin(1, 2, F_NFREQ, 31 | PHI)
        last = ctx.series_layout(4)
        off, ln = ctx.series_layout(6)
        assert (off, ln) == (last[0] + last[1], F_NFREQ * N + 5) and ctx.series_info() == (0, 0, off + ln)
        _raises(lambda: ctx.series_layout(5))
        ctx.series_add_sweep()
        both = ctx.series_bins()[0]
        ctx.series_end()
        ctx.series_begin(1, 2, F_NFREQ, 31)                  # the same series without the part: the other parts keep their bits
        ctx.series_add_sweep()
        without = ctx.series_bins()[0]
        _raises(lambda: ctx.series_layout(6))
        _raises(ctx.series_phi_derived)
        ctx.series_end()
        ctx.series_begin(1, 2, F_NFREQ, PHI)
        ctx.series_add_sweep()
        alone = ctx.series_bins()[0]
        ctx.series_end()
    finally:
        ctx.close()
    assert np.array_equal(both[off:], alone) and np.array_equal(both[:off], without) and np.abs(without).max() > 0
    _compare(alone, phi, L, F_NFREQ, "next to the fermionic parts")


def test_begin_error_paths():
    ctx = _ctx(1, 4, 10)
    try:
        for bad in (dict(parts=32), dict(parts=32 | PHI), dict(parts=128 | PHI), dict(nfreq=0), dict(nfreq=11), dict(bin_size=0), dict(max_bins=1)):
            kw = dict(dict(bin_size=1, max_bins=4, nfreq=3, parts=PHI), **bad)
            _raises(lambda: ctx.series_begin(**kw))
            _raises(ctx.series_info)
        _raises(lambda: ctx.series_begin(1, 4, 3, 1 | PHI))  # the equal-time block has never been enabled
        ctx.set_fields(_field(9, 10, 16, 1, offset=0.5))
        ctx.series_begin(1, 4, 10, PHI)                      # nfreq = m
        _raises(ctx.series_phi_derived)                      # no closed bin
        ctx.series_add_sweep()
        _raises(ctx.series_phi_derived)                      # one closed bin
        ctx.series_add_sweep()
        v, e = ctx.series_phi_derived()
        assert v.shape == (1, 6) and np.all(np.isfinite(v)) and np.all(e == 0.0)     # the same field twice: no spread
        assert np.isnan(ctx.series_derived()[0]).all()       # the fermionic derived quantities have no part here
        ctx.series_end()
    finally:
        ctx.close()


# ---- kernel level: statistics and derived quantities -----------------------------------------------------------------------------------
ST_L, ST_M, ST_NCH, ST_BIN, ST_MAXBINS, ST_NFREQ = 4, 10, 2, 2, 3, 2


@functools.lru_cache(maxsize=None)
def _stats_case():
    """3 bins of 2 samples; the field is amplitude x (0.5 + noise) with the amplitude growing from sweep to sweep, so that the bins differ
    and chi(0, 0) stays well above its neighbours (a real xi)"""
    N = ST_L * ST_L
    ctx = _ctx(2, ST_L, ST_M, ST_NCH)
    try:
        ctx.series_begin(ST_BIN, ST_MAXBINS, ST_NFREQ, PHI)
        for i in range(ST_BIN * ST_MAXBINS):
            _set(ctx, [_field(300 + 10 * i + c, ST_M, N, 2, amp=0.6 + 0.3 * i + 0.1 * c, offset=0.5) for c in range(ST_NCH)])
            ctx.series_add_sweep()
        rec = dict(bins=_all_bins(ctx, ST_NCH), stats=ctx.series_stats(), stats2=ctx.series_stats(), derived=ctx.series_phi_derived(),
                   derived2=ctx.series_phi_derived())
        _raises(ctx.series_add_sweep)                        # full
        ctx.series_end()
    finally:
        ctx.close()
    return rec


def test_statistics_and_derived():
    rec = _stats_case()
    N, L = ST_L * ST_L, ST_L
    bins = rec["bins"]
    mean, err = rec["stats"]
    assert all(np.array_equal(x, y) for x, y in zip(rec["stats"] + rec["derived"], rec["stats2"] + rec["derived2"]))
    rows = [(n * N, N) for n in range(ST_NFREQ)] + [(ST_NFREQ * N + j, 1) for j in range(5)]
    wm = we = 0.0
    for b in range(ST_NCH):
        rmean, rerr = sr.jackknife(bins[b])
        for off, ln in rows:
            sl = slice(off, off + ln)
            assert np.abs(bins[b][:, sl] - rmean[sl]).max() > 1e-3 * np.abs(rmean[sl]).max(), (b, off)
            wm = max(wm, sr.rows_close(mean[b, sl], rmean[sl], 1e-13, ln))
            we = max(we, sr.rows_close(err[b, sl], rerr[sl], 1e-10, ln))
    print(f"mean {wm:.2e} (bound 1e-13), err {we:.2e} of the row's largest error (bound 1e-10)")
    val, derr = rec["derived"]
    assert val.shape == (ST_NCH, 6)
    fs = spr.derived_functions(L, N, ST_M * 0.1, ST_NFREQ)
    ref = np.array([[sr.jackknife(bins[b], f) for f in fs] for b in range(ST_NCH)])      # [chain][entry][value, err]
    assert np.all(np.isfinite(ref)) and np.all(ref[:, :, 1] > 0.0)
    dv = np.abs(val - ref[:, :, 0]).max()
    de = (np.abs(derr - ref[:, :, 1]).max(axis=0) / ref[:, :, 1].max(axis=0)).max()
    print(f"derived: values {dv:.2e} (bound 1e-12), errors {de:.2e} of the entry's largest error (bound 1e-10); chain 0: "
          + ", ".join(f"{v:.6f} +- {e:.2e}" for v, e in zip(val[0], derr[0])))
    assert dv <= 1e-12 and de <= 1e-10


# ---- kernel level: routed accumulate, auto re-bin, running variance, export / import with the part present -----------------------------
LG_L, LG_M, LG_NCH, LG_NFREQ, LG_SWEEPS, LG_MAXBINS = 4, 10, 3, 2, 8, 4
LG_ROUTES = [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [1, 0, 2], [2, 1, 0], [1, 2, 0], [0, 1, 2]]


def _lg_fields(i):
    return [_field(500 + 10 * i + c, LG_M, LG_L * LG_L, 2, amp=0.5 + 0.2 * i + 0.1 * c) for c in range(LG_NCH)]


def _export(ctx):
    st, raw = ctx.series_export()
    nb, S, B = st.nb, st.sample_len, st.bins_closed
    n = nb * S
    rec = dict(state={f: getattr(st, f) for f, _ in st._fields_}, st=st, raw=raw, bins=raw[:B * n].reshape(B, nb, S),
               open=raw[B * n:(B + 1) * n].reshape(nb, S))
    if raw.size > (B + 1) * n:
        rec["w"], rec["m2"] = raw[(B + 1) * n:(B + 2) * n].reshape(nb, S), raw[(B + 2) * n:].reshape(nb, S)
    return rec


@functools.lru_cache(maxsize=None)
def _long_case():
    ctx = _ctx(2, LG_L, LG_M, LG_NCH)
    rec = {}
    try:
        ctx.series_begin(1, LG_SWEEPS, LG_NFREQ, PHI)        # the device's own samples: bin size 1
        for i in range(LG_SWEEPS):
            _set(ctx, _lg_fields(i))
            ctx.series_add_sweep()
        rec["samples"] = np.ascontiguousarray(_all_bins(ctx, LG_NCH).transpose(1, 0, 2))     # [sweep][chain][S]
        ctx.series_end()
        ctx.series_begin(2, LG_MAXBINS, LG_NFREQ, PHI)       # routed, bins of two
        ptr, S = ctx.series_sample_device()
        rows = [ptr + 8 * b * S for b in range(LG_NCH)]
        for i in range(LG_SWEEPS):
            _set(ctx, _lg_fields(i))
            ctx.series_form_sample()
            src = [None] * LG_NCH
            for c, s in enumerate(LG_ROUTES[i]):
                src[s] = rows[c]
            ctx.series_accumulate(src)
        rec["routed"] = _all_bins(ctx, LG_NCH)
        ctx.series_end()
        ctx.series_begin(1, LG_MAXBINS, LG_NFREQ, PHI)       # auto re-bin and the running variance, exported after every sweep
        ctx.series_configure(auto_rebin=True, track_variance=True)
        rec["exports"] = []
        for i in range(LG_SWEEPS):
            _set(ctx, _lg_fields(i))
            ctx.series_add_sweep()
            rec["exports"].append(_export(ctx))
        ctx.series_end()
        cut = 3                                              # a new series goes on from the export after sweep `cut`
        ctx.series_begin(1, LG_MAXBINS, LG_NFREQ, PHI)
        ctx.series_import(rec["exports"][cut - 1]["st"], rec["exports"][cut - 1]["raw"])
        rec["reimported"] = _export(ctx)
        for i in range(cut, LG_SWEEPS):
            _set(ctx, _lg_fields(i))
            ctx.series_add_sweep()
        rec["continued"] = _export(ctx)
        ctx.series_end()
        ctx.set_equal_time_correlators(True)                 # allocates the block: a series with another mask can open
        ctx.set_equal_time_correlators(False)
        ctx.series_begin(1, LG_MAXBINS, LG_NFREQ, 1 | PHI)
        before = _export(ctx)
        _raises(lambda: ctx.series_import(rec["exports"][cut - 1]["st"], rec["exports"][cut - 1]["raw"]))     # parts and length differ
        rec["refused_unchanged"] = np.array_equal(_export(ctx)["raw"], before["raw"]) and _export(ctx)["state"] == before["state"]
        ctx.series_end()
    finally:
        ctx.close()
    return rec


def test_routed_accumulate_with_the_part():
    rec = _long_case()
    want = srr.routed_bins(rec["samples"], LG_ROUTES, 2)
    plain = srr.routed_bins(rec["samples"], [[0, 1, 2]] * LG_SWEEPS, 2)
    for s in range(LG_NCH):
        assert np.array_equal(rec["routed"][s], want[s]), s
        assert not np.array_equal(want[s], plain[s]), s


def test_auto_rebin_with_the_part():
    rec = _long_case()
    per_slot = slr.routed_samples(rec["samples"], [[0, 1, 2]] * LG_SWEEPS)
    for i, ex in enumerate(rec["exports"]):
        want = slr.series_run(per_slot[:, :i + 1], 1, LG_MAXBINS, True)
        st = ex["state"]
        assert (st["bin_size"], st["sweeps_in_open_bin"], st["samples"], st["rebins"]) == (want["bin_size"], want["in_open"], want["samples"], want["rebins"]), i
        assert st["parts"] == PHI and st["nfreq"] == LG_NFREQ and st["bins_closed"] == want["bins"].shape[1] < LG_MAXBINS
        assert np.array_equal(ex["bins"].transpose(1, 0, 2), want["bins"]), i
        assert np.array_equal(ex["open"], want["open"]), i
    assert rec["exports"][-1]["state"]["rebins"] == 2


def _fused_welford(samples):
    """Welford's recurrence of series_long_reference.welford with m2 += d (x - w) rounded once (a fused multiply-add), in exact rational
    arithmetic; everything else is rounded operation by operation as there"""
    x = np.asarray(samples, dtype=np.float64)
    w, m2 = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    F = fractions.Fraction
    for i in range(x.shape[0]):
        d = x[i] - w
        w = w + d / float(i + 1)
        e = x[i] - w
        m2 = np.array([float(F(float(dd)) * F(float(ee)) + F(float(mm))) for dd, ee, mm in zip(d.ravel(), e.ravel(), m2.ravel())]).reshape(m2.shape)
    return w, m2


def test_running_variance_with_the_part():
    rec = _long_case()
    last = rec["exports"][-1]
    for s in range(LG_NCH):
        smp = rec["samples"][:, s]
        ww, wm2 = slr.welford(smp)
        _, fm2 = _fused_welford(smp)
        mean, m2 = slr.two_pass(smp)
        print(f"slot {s}: w against the two-pass mean {np.abs(last['w'][s] - mean).max() / np.abs(mean).max():.2e}, m2 against the two-pass value "
              f"{np.abs(last['m2'][s] - m2).max() / np.abs(m2).max():.2e} of the row's scale; m2 equals the plain recurrence: "
              f"{np.array_equal(last['m2'][s], wm2)}, the fused one: {np.array_equal(last['m2'][s], fm2)}")
        assert np.array_equal(last["w"][s], ww), s
        assert np.abs(m2).max() > 0
        assert np.array_equal(last["m2"][s], fm2), s         # the fused update, the one the build produces


def test_export_import_with_the_part():
    rec = _long_case()
    cut = 3
    assert np.array_equal(rec["reimported"]["raw"], rec["exports"][cut - 1]["raw"]) and rec["reimported"]["state"] == rec["exports"][cut - 1]["state"]
    assert np.array_equal(rec["continued"]["raw"], rec["exports"][-1]["raw"]) and rec["continued"]["state"] == rec["exports"][-1]["state"]
    assert rec["refused_unchanged"]


# ---- host level ------------------------------------------------------------------------------------------------------------------------
H_L, H_N, H_M, H_NCH, H_NFREQ, H_SWEEPS, H_MAXBINS = 4, 16, 10, 4, 3, 4, 8
H_R = (-1.0, -0.9, -0.8, -0.7)


def _host_params(kind, rvals=H_R):
    from detqmc_amd import SDWParams
    kw = dict(opdim=2, L=H_L, beta=1.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", fermionMeasurements=True, rngSeed=4711)
    if kind == "o3":
        kw["opdim"] = 3
    elif kind == "nofm":
        kw["fermionMeasurements"] = False
    elif kind == "eq":
        kw["equalTimeCorrelators"] = True
    p = SDWParams(**kw)
    return [dataclasses.replace(p, simindex=b, r=r) for b, r in enumerate(rvals)]


def _host_bins(batch, nbins):
    """[slot][bin][nfreq N + 5]: 'phiChi' and 'phiScalars' behind each other, as in the sample row"""
    out = []
    for b in range(H_NCH):
        chi = batch.chain(b).series_bins("phiChi")
        sc = batch.chain(b).series_bins("phiScalars")
        assert chi.shape == (nbins, H_NFREQ, H_N) and sc.shape == (nbins, 5)
        out.append(np.concatenate([chi.reshape(nbins, -1), sc], axis=1))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _host_run(kind, sub_batches, series):
    from detqmc_amd import DetSDWBatch
    batch = DetSDWBatch(_host_params(kind), sub_batches=sub_batches)
    rec = dict(phis=[], obs=[])
    try:
        assert batch.sub_batches == sub_batches
        batch.sweepThermalization()
        if series:
            batch.series_begin(1, H_MAXBINS, nfreq=H_NFREQ, phi=True, track_variance=True)
        for i in range(H_SWEEPS):
            if i % 2:
                batch.sweep(False)
            batch.sweep(True)
            rec["phis"].append([batch.chain(b).phi for b in range(H_NCH)])
            rec["obs"].append([(batch.chain(b).observables.normMeanPhi, batch.chain(b).observables.associatedEnergy) for b in range(H_NCH)])
            if series:
                assert batch.series_info()[:2] == (i + 1, 0)
        rec["rng"] = [batch.chain(b).info.rngDrawn for b in range(H_NCH)]
        if series:
            assert batch.series_info()[2] == (10 * H_N if kind == "eq" else 0) + H_NFREQ * H_N + 5
            rec["bins"] = _host_bins(batch, H_SWEEPS)
            rec["stats_all"] = {nm: batch.series_stats_all(nm) for nm in ("phiChi", "phiScalars")}
            rec["stats"] = {nm: [batch.chain(b).series_stats(nm) for b in range(H_NCH)] for nm in ("phiChi", "phiScalars")}
            rec["derived"] = {nm: batch.series_derived_all(nm) for nm in ("binderPhi", "binderRatioPhi", "chiPhi", "chiPhiConnected", "R_phi", "xiPhi")}
            rec["binning_all"] = {nm: batch.series_binning_all(nm, 2) for nm in ("phiChi", "phiScalars")}
            rec["binning"] = {nm: [batch.chain(b).series_binning(nm, 2) for b in range(H_NCH)] for nm in ("phiChi", "phiScalars")}
            batch.series_end()
    finally:
        batch.close()
    return rec


HOST_RUNS = [("o2", 1), ("o2", 2), ("o3", 1), ("nofm", 1), ("eq", 1)]


@pytest.mark.parametrize("kind,sub_batches", HOST_RUNS)
def test_host_bins_against_the_fields_and_the_host_scalars(kind, sub_batches):
    rec = _host_run(kind, sub_batches, True)
    nc = H_NFREQ * H_N
    from detqmc_amd import phi_sample
    for i in range(H_SWEEPS):
        for b in range(H_NCH):
            phi = rec["phis"][i][b]
            chi, sc = phi_sample(phi, H_L, H_NFREQ)
            got = rec["bins"][b][i]
            _compare(got, phi, H_L, H_NFREQ, f"{kind} sub_batches {sub_batches} sweep {i} chain {b}", want=np.concatenate([chi.ravel(), sc]))
            a = np.abs(phi[1:]).max()
            tol = spr.rounding_bound(phi.shape[2], H_M, H_N, a)
            norm, assoc = rec["obs"][i][b]
            print(f"    host normMeanPhi {abs(got[nc] - norm):.2e} (bound {tol / norm:.2e}), associatedEnergy {abs(got[nc + 4] - assoc):.2e} (bound {tol:.2e})")
            assert abs(got[nc] - norm) <= tol / norm and abs(got[nc + 4] - assoc) <= tol
    for nm, sl in (("phiChi", slice(0, nc)), ("phiScalars", slice(nc, nc + 5))):
        for b in range(H_NCH):
            rmean, rerr = sr.jackknife(rec["bins"][b][:, sl])
            mean, err = (x.ravel() for x in rec["stats"][nm][b])
            sr.rows_close(mean, rmean, 1e-13, mean.size)
            sr.rows_close(err, rerr, 1e-10, err.size)
            for k in (0, 1):
                assert np.array_equal(rec["stats_all"][nm][k][b], rec["stats"][nm][b][k])
            # the binning analysis reads the same slice: two levels over the four bins, errors against numpy at the bound of the statistics
            berr, btau = rec["binning"][nm][b]
            shape = (2, H_NFREQ, H_N) if nm == "phiChi" else (2, 5)
            assert berr.shape == btau.shape == shape and np.all(np.isfinite(berr)) and np.all(np.isfinite(btau)) and np.all(btau > 0)
            want_err, _ = slr.binning(rec["bins"][b][:, sl], 1, 2)
            sr.rows_close(berr.reshape(2, -1), want_err, 1e-10, want_err.shape[1])
            assert np.array_equal(berr[0].ravel(), err)      # level 0 is the error of series_stats
            for k in (0, 1):
                assert np.array_equal(rec["binning_all"][nm][k][b], rec["binning"][nm][b][k])
    beta = H_M * 0.1
    fs = dict(zip(("binderPhi", "binderRatioPhi", "chiPhi", "chiPhiConnected", "R_phi", "xiPhi"), spr.derived_functions(H_L, H_N, beta, H_NFREQ)))
    for b in range(H_NCH):
        rv, re = sr.jackknife(rec["bins"][b], fs["binderPhi"])
        v, e = (x[b] for x in rec["derived"]["binderPhi"])
        print(f"chain {b}: binderPhi {v:.10f} +- {e:.3e} (numpy {rv:.10f} +- {re:.3e})")
        assert np.isfinite(v) and np.isfinite(e) and re > 0
        assert abs(v - rv) <= 1e-12 and abs(e - re) <= 1e-10 * re
        for nm in ("binderRatioPhi", "chiPhi", "chiPhiConnected", "R_phi"):
            rv, re = sr.jackknife(rec["bins"][b], fs[nm])
            v, e = (x[b] for x in rec["derived"][nm])
            assert abs(v - rv) <= 1e-12 * max(1.0, abs(rv)) and abs(e - re) <= 1e-10 * re, nm
        rv = sr.jackknife(rec["bins"][b], fs["xiPhi"])[0]
        v = rec["derived"]["xiPhi"][0][b]
        assert (np.isnan(v) and np.isnan(rv)) or abs(v - rv) <= 1e-12 * max(1.0, abs(rv))


def test_host_series_changes_no_trajectory_and_no_grouping_changes_a_bit():
    plain, one, two = _host_run("o2", 1, False), _host_run("o2", 1, True), _host_run("o2", 2, True)
    for other in (one, two):
        assert other["rng"] == plain["rng"] and other["obs"] == plain["obs"]
        for x, y in zip(other["phis"], plain["phis"]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert np.array_equal(one["bins"], two["bins"])
    for nm in ("phiChi", "phiScalars"):
        for k in (0, 1):
            assert np.array_equal(one["stats_all"][nm][k], two["stats_all"][nm][k]), nm
    for nm in one["derived"]:
        assert np.array_equal(one["derived"][nm], two["derived"][nm], equal_nan=True), nm
    for nm in ("phiChi", "phiScalars"):
        for k in (0, 1):
            assert np.array_equal(one["binning_all"][nm][k], two["binning_all"][nm][k]), nm
    nofm_plain = _host_run("nofm", 1, False)
    nofm = _host_run("nofm", 1, True)
    assert nofm["rng"] == nofm_plain["rng"] and all(np.array_equal(p, q) for x, y in zip(nofm["phis"], nofm_plain["phis"]) for p, q in zip(x, y))


def test_host_refusals_and_names():
    from detqmc_amd import DetSDWBatch, DqmcError, _lib
    batch = DetSDWBatch(_host_params("o2")[:1])
    try:
        with pytest.raises(DqmcError, match="equalTimeCorrelators or timeDisplacedEverySlice"):
            batch.series_begin(2, 3)                         # without the flag nothing changes
        with pytest.raises(DqmcError):
            batch.series_begin(2, 3, nfreq=0, phi=True)      # the part needs 1 <= nfreq <= m
        with pytest.raises(DqmcError):
            batch.series_begin(2, 3, nfreq=H_M + 1, phi=True)
        with pytest.raises(DqmcError):
            batch.series_info()
        assert batch.lib.detsdw_series_begin(batch.h, 2, 3, 1, 4) != 0          # an unknown flag stays refused
        batch.series_begin(1, 4, nfreq=2, phi=True)
        batch.sweep(True)
        batch.sweep(True)
        with pytest.raises(DqmcError):
            batch.series_stats_all("sdwSq")                  # no equal-time part
        with pytest.raises(DqmcError):
            batch.series_derived_all("R_sdw")
        out = np.zeros(H_NFREQ * H_N)
        batch.chain(0)._sel()
        for which in (32, 33):                               # names of the series only
            assert batch.lib.detsdw_get_observable_vector(batch.chain(0).h, which, out.ctypes.data_as(_lib._DP)) != 0
        assert batch.series_stats_all("phiScalars")[0].shape == (1, 5)
        batch.series_end()
    finally:
        batch.close()
    batch = DetSDWBatch(_host_params("eq")[:1])
    try:
        batch.series_begin(1, 4, nfreq=2)                    # a series without the part
        batch.sweep(True)
        batch.sweep(True)
        for fn in (lambda: batch.series_stats_all("phiChi"), lambda: batch.chain(0).series_bins("phiScalars"),
                   lambda: batch.series_derived_all("binderPhi"), lambda: batch.series_derived_all("xiPhi")):
            with pytest.raises(DqmcError):
                fn()
        assert np.isfinite(batch.series_derived_all("R_charge")[0]).all()
        batch.series_end()
    finally:
        batch.close()


def test_host_series_file_round_trip_and_mismatch(tmp_path):
    from detqmc_amd import DetSDWBatch, DqmcError
    path = tmp_path / "phi.series"
    batch = DetSDWBatch(_host_params("eq"))
    try:
        batch.sweepThermalization()
        batch.series_begin(1, H_MAXBINS, nfreq=H_NFREQ, phi=True)
        batch.series_route([1, 0, 3, 2])
        for _ in range(3):
            batch.sweep(True)
        bins = _host_bins(batch, 3)
        sq = np.array([batch.chain(b).series_bins("sdwSq") for b in range(H_NCH)])
        batch.series_save(path)
        batch.series_end()
        batch.series_begin(1, H_MAXBINS, nfreq=H_NFREQ, phi=True)
        batch.series_load(path)
        assert batch.series_route() == [1, 0, 3, 2] and batch.series_info()[:2] == (3, 0)
        assert np.array_equal(_host_bins(batch, 3), bins)
        assert np.array_equal(np.array([batch.chain(b).series_bins("sdwSq") for b in range(H_NCH)]), sq)
        batch.series_end()
        batch.series_begin(1, H_MAXBINS, nfreq=H_NFREQ)      # the same handle without the part
        batch.series_route([3, 2, 1, 0])
        batch.sweep(True)
        own = np.array([batch.chain(b).series_bins("sdwSq") for b in range(H_NCH)])
        st = batch.series_state()
        with pytest.raises(DqmcError, match="parts"):
            batch.series_load(path)
        st2 = batch.series_state()
        assert all(getattr(st, f) == getattr(st2, f) for f, _ in st._fields_) and batch.series_route() == [3, 2, 1, 0]
        assert np.array_equal(np.array([batch.chain(b).series_bins("sdwSq") for b in range(H_NCH)]), own)
        batch.series_end()
    finally:
        batch.close()


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_phi_scalars_routed_by_replica_exchange(sub_batches):
    from detqmc_amd import DetSDWBatch, pt
    rvals = [-1.0, -1.0, -0.8, -0.8]          # equal neighbours: the swaps 0 <-> 1 and 2 <-> 3 are certain and need no draw
    batch = DetSDWBatch(_host_params("o2", rvals), sub_batches=sub_batches)
    nsweeps, nc = 4, H_NFREQ * H_N
    try:
        state = pt.ExchangeState.create(rvals, 0, 1, n_local=H_NCH)
        reps = [pt.ReplicaAdapter(batch.chain(b)) for b in range(H_NCH)]
        batch.sweepThermalization()
        batch.series_begin(1, H_MAXBINS, nfreq=H_NFREQ, phi=True)
        held, obs, phis = [], [], []
        for i in range(nsweeps):
            held.append(list(state.local_parameter_indices))
            assert batch.series_route() == held[-1]
            batch.sweep(True)
            obs.append([(batch.chain(b).observables.normMeanPhi, batch.chain(b).observables.associatedEnergy) for b in range(H_NCH)])
            phis.append([batch.chain(b).phi for b in range(H_NCH)])
            new = pt.replica_exchange_step(reps, state, None, route_series=True)
            assert new == state.local_parameter_indices and batch.series_route() == new
        assert any(h != list(range(H_NCH)) for h in held)
        bins = _host_bins(batch, nsweeps)
        for i in range(nsweeps):
            for c in range(H_NCH):
                s = held[i][c]
                got = bins[s][i]
                _compare(got, phis[i][c], H_L, H_NFREQ, f"sub_batches {sub_batches} sweep {i} chain {c} -> slot {s}", want=_host_sample_of(phis[i][c]))
                tol = spr.rounding_bound(2, H_M, H_N, np.abs(phis[i][c][1:]).max())
                norm, assoc = obs[i][c]
                assert abs(got[nc] - norm) <= tol / norm and abs(got[nc + 4] - assoc) <= tol
        batch.series_end()
    finally:
        batch.close()


def _host_sample_of(phi):
    from detqmc_amd import phi_sample
    chi, sc = phi_sample(phi, H_L, H_NFREQ)
    return np.concatenate([chi.ravel(), sc])
