"""Band-resolved charge correlators bandDiff (n_x - n_y) and bandMix on the device: the time-displaced kernel against numpy on the
device's own four matrices, the block's bookkeeping, every slice, the Matsubara transform of channel 4, the equal-time block, the two
series parts with their correlation ratios, and the host level (tests/band_reference.py).

Tolerances are the project's: relerr < 1e-10 for a kernel against numpy on the device's own matrices, bit equality wherever a text
says so, and the bounds of tests/test_gpu_td_fine.py, test_gpu_td_matsubara.py and test_gpu_series.py where those files set one.
Every test prints its figures before it asserts."""
import dataclasses
import functools

import numpy as np
import pytest

import series_reference as sr
import td_fine_reference as tf
from conftest import relerr
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu

EINVAL = -1
# (opdim, L, m, s, checkerboard, bc, weakZflux); the L = 6 cases have N = 36: two workgroups and a partial tile of bins
KERNEL_CASES = [
    (1, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "pbc", False),
    (3, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "apbc-xy", False),
    (2, 4, 20, 5, False, "pbc", False),
    (3, 4, 20, 5, False, "pbc", False),
    (2, 4, 20, 5, True, "pbc", True),
    (2, 6, 20, 5, True, "pbc", False),
    (3, 6, 20, 5, True, "pbc", False),
]
EQ_CASES = [c for c in KERNEL_CASES if c[1] == 4] + [(2, 6, 20, 5, True, "pbc", False)]


def _context(opdim, L, m, s, band=True, ph=True, td=1, every=False, checkerboard=True, bc="pbc", weakZflux=False, nchains=1, **kw):
    from detqmc_amd import KernelContext
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, bc=bc, weakZflux=weakZflux, stabilisation="qr", checkerboard=checkerboard,
                         nchains=nchains, timeDisplaced=td, tdParticleHole=ph, tdBand=band, tdEverySlice=every, **kw)


def _start(ctx, phis):
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.measure_reset()


def _block(acc, n, N, j):
    """(count, bandDiff sums, bandMix sums) of boundary j"""
    off = (n - 1) + (j - 1) * 2 * N
    return acc[j - 1], acc[off:off + N], acc[off + N:off + 2 * N]


def _raises(fn, code=EINVAL):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == code
    return True


# ---- 1. kernel against numpy on the device's own matrices -------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", KERNEL_CASES)
def test_kernel_vs_numpy_on_device_matrices(opdim, L, m, s, cb, bc, flux):
    from band_reference import band_correlators
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    got = {}
    for band in (True, False):
        ctx = _context(opdim, L, m, s, band=band, checkerboard=cb, bc=bc, weakZflux=flux)
        try:
            n = ctx.n
            assert ctx.lib.dqmc_measure_td_band_accum_size(ctx.h) == ((n - 1) * (1 + 2 * N) if band else 0)
            assert ctx.lib.dqmc_measure_td_ph_accum_size(ctx.h) == (n - 1) * (1 + 3 * N)
            _start(ctx, [phi])
            target = n - 2                               # tau = 10; the other boundaries must stay untouched
            ref = {}

            def at(j):
                if j != target:
                    return
                gtt = ctx.g
                sl, gt0, g0t = ctx.green_timedisplaced()
                sl0, g00 = ctx.green0_timedisplaced()
                assert sl == s * j and sl0 == s * j
                if band:
                    ref["c"] = band_correlators(ora, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])
                    ctx.measure_timedisplaced_band(j)    # before the particle-hole call here, after it in the preconditions test
                ctx.measure_timedisplaced_ph(j)
                assert np.array_equal(ctx.g, gtt)        # the measurements leave G alone

            _walk_down(ctx, at)
            got[band] = ctx.measure_td_ph_read()
            if not band:
                continue
            acc = ctx.measure_td_band_read()
            assert acc.shape == ((n - 1) * (1 + 2 * N),)
            cnt, *rows = _block(acc, n, N, target)
            assert cnt == 1.0
            errs = [relerr(v / N, r) for v, r in zip(rows, ref["c"])]
            print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux} j={target}: bandDiff {errs[0]:.2e} bandMix {errs[1]:.2e} "
                  f"(max|C| {np.abs(ref['c'][0]).max():.3f}, {np.abs(ref['c'][1]).max():.3f})")
            for r in ref["c"]:
                assert np.abs(r).max() > 1e-6            # not a comparison of zeros
            assert max(errs) < 1e-10, errs
            for j in range(1, n):
                if j != target:
                    c0, *rest = _block(acc, n, N, j)
                    assert c0 == 0.0 and not any(v.any() for v in rest), j
        finally:
            ctx.close()
    assert np.array_equal(got[True], got[False]) and got[True].any()      # the particle-hole block does not see the flag


# ---- 2. accumulation, reproducibility, batching ------------------------------------------------------------------------------------
def _measure_all(ctx, phis, twice_at=None):
    _start(ctx, phis)
    grabbed = {}

    def at(j):
        ctx.measure_timedisplaced_band(j)
        if j == twice_at:
            ctx.select_chain(0)
            grabbed["once"] = ctx.measure_td_band_read()
            ctx.measure_timedisplaced_band(j)

    _walk_down(ctx, at)
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append(ctx.measure_td_band_read())
    return out, grabbed.get("once")


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_and_reproducibility(opdim):
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 93 + opdim), _random_phi(opdim, N, m, 193 + opdim)]
    blocks = []
    for rep in range(2):
        ctx = _context(opdim, 6, m, s)
        try:
            (acc,), once = _measure_all(ctx, phis[:1], twice_at=2)
            n = ctx.n
            c1, *v1 = _block(once, n, N, 2)
            c2, *v2 = _block(acc, n, N, 2)
            assert c1 == 1.0 and c2 == 2.0
            for a, b in zip(v1, v2):
                assert np.array_equal(b, a + a) and np.any(a != 0.0)      # v + v is exact
            assert list(acc[:n - 1]) == [1.0, 2.0, 1.0]
            blocks.append(acc)
        finally:
            ctx.close()
    assert np.array_equal(blocks[0], blocks[1])                            # two fresh contexts: bit-identical
    singles = []
    for phi in phis:
        ctx = _context(opdim, 6, m, s)
        try:
            singles.append(_measure_all(ctx, [phi])[0][0])
        finally:
            ctx.close()
    ctx = _context(opdim, 6, m, s, nchains=2)
    try:
        both, _ = _measure_all(ctx, phis)
    finally:
        ctx.close()
    assert not np.array_equal(singles[0], singles[1])
    assert np.array_equal(both[0], singles[0]) and np.array_equal(both[1], singles[1])


# ---- 3. every slice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,m", [(2, 20), (3, 20), (2, 22), (3, 22)])
def test_every_slice(opdim, m):
    """one pass over all segments and the ends: every row count is 1, row j s is the coarse row j bit for bit; rows 0, m and one
    interior row against numpy on the device's own matrices (1e-10, the bound of tests/test_gpu_td_fine.py::test_kernel_rows for its
    particle-hole channel) and against direct inverses of the oracle's chain: rows 0 and m from G(0) alone (1e-10, the parity bound on
    G), the interior row within 10 e_ref, that file's bound for anything propagated without stabilisation."""
    from band_reference import band_correlators
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    L, s = 4, 5
    N = L * L
    phi = _random_phi(opdim, N, m, 41 * opdim + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    chain = Chain(ora)
    ctx = _context(opdim, L, m, s, every=True)

    def ref_of(gtt, gt0, g0t, g00):
        return np.concatenate(band_correlators(ora, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])) * N

    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 4) == (m + 1) * (1 + 2 * N)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == 0
        _start(ctx, [phi])
        kin = s + 2                                      # reached from boundary 1 by two upward steps
        dev = {}

        def at(j):
            if j == 1:
                g00 = ctx.green0_timedisplaced()[1]
                ctx.td_fine_propagate(1, kin)
                _, f_t0, f_0t, f_tt = ctx.green_td_fine()
                dev[kin] = ref_of(f_tt, f_t0, f_0t, g00)
            ctx.measure_timedisplaced_band(j)
            ctx.measure_timedisplaced_segment(j)

        _walk_down(ctx, at)
        ctx.advanceDownGreen(1)
        g, one = ctx.g, np.eye(ctx.ng)
        dev[0], dev[m] = ref_of(g, g, g - one, g), ref_of(g, one - g, -g, g)
        ctx.measure_timedisplaced_ends()
        fine = ctx.measure_td_fine_read(4)
        cnt, rows = fine[:m + 1], fine[m + 1:].reshape(m + 1, 2 * N)
        assert np.array_equal(cnt, np.ones(m + 1))
        coarse = ctx.measure_td_band_read()
        assert np.array_equal(coarse[:n - 1], np.ones(n - 1))
        crow = coarse[n - 1:].reshape(n - 1, 2 * N)
        for j in range(1, n):
            assert np.array_equal(rows[j * s], crow[j - 1]) and crow[j - 1].any(), j
        gd = chain.greens(m)[0]                          # G(beta) = G(0) by the direct inverse
        direct = {0: ref_of(gd, gd, gd - one, gd), m: ref_of(gd, one - gd, -gd, gd)}
        d_tt, d_t0, d_0t = chain.greens(kin)
        direct[kin] = ref_of(d_tt, d_t0, d_0t, four_greens(chain, kin)[3])
        e_ref = tf.e_ref()
        for k in (0, kin, m):
            e_dev, e_dir = relerr(rows[k], dev[k]), relerr(rows[k], direct[k])
            bound = 10 * e_ref if k == kin else 1e-10
            print(f"O({opdim}) m={m} row {k}: vs numpy on device matrices {e_dev:.2e} (1e-10), vs direct inverses {e_dir:.2e} ({bound:.2e})")
            assert np.abs(dev[k][:N]).max() > 1e-6 and np.abs(dev[k][N:]).max() > 1e-6
            assert e_dev < 1e-10 and e_dir < bound, (k, e_dev, e_dir)
    finally:
        ctx.close()


# ---- 4. Matsubara transform of channel 4 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim", [2, 3])
def test_matsubara_channel_4(opdim):
    import td_matsubara_reference as tm
    L, m, s, nfreq = 4, 20, 5, 3
    N = L * L
    ctx = _context(opdim, L, m, s, every=True)
    try:
        _start(ctx, [_random_phi(opdim, N, m, 57 + opdim)])
        _walk_down(ctx, ctx.measure_timedisplaced_segment)
        ctx.advanceDownGreen(1)
        ctx.measure_timedisplaced_ends()
        assert ctx.lib.dqmc_measure_td_matsubara_size(ctx.h, 4, nfreq) == 2 * nfreq * N * 2
        fine = ctx.measure_td_fine_read(4)
        a = ctx.measure_td_matsubara(4, nfreq)
        b = ctx.measure_td_matsubara(4, nfreq)
        assert a.shape == (1, 2, nfreq, N) and np.array_equal(a, b)
        assert np.array_equal(ctx.measure_td_fine_read(4), fine)           # the transform reads the block only
        rows = fine[m + 1:].reshape(m + 1, 2, N) / (N * fine[:m + 1, None, None])
        for comp, nm in enumerate(("bandDiff", "bandMix")):
            ref = tm.bosonic(rows[:, comp], L, 0.1, nfreq)
            e = relerr(a[0, comp], ref)
            print(f"O({opdim}) {nm}: chi(q, i omega_n) vs numpy on the block {e:.2e} (bound 1e-10)")
            assert np.abs(ref).max() > 1e-6 and e <= 1e-10
    finally:
        ctx.close()
    ctx = _context(opdim, L, m, s, band=False, every=True)                # no block for the channel
    try:
        assert ctx.lib.dqmc_measure_td_matsubara_size(ctx.h, 4, nfreq) == 0
        _raises(lambda: ctx.measure_td_matsubara(4, nfreq))
        _raises(lambda: ctx.measure_td_fine_read(4))
    finally:
        ctx.close()


# ---- 5. equal time -----------------------------------------------------------------------------------------------------------------
def _walk_to(ctx, k_stop):
    m, s, n = ctx.m, ctx.s, ctx.n
    for k in range(m, (n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(n)
    for k in range((n - 1) * s, k_stop, -1):
        ctx.wrapDownGreen(k)


@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", EQ_CASES)
def test_equal_time_vs_numpy_on_device_matrix(opdim, L, m, s, cb, bc, flux):
    from band_reference import eq_band_correlators, eq_band_delta
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, band=False, ph=False, td=0, checkerboard=cb, bc=bc, weakZflux=flux)    # a run-time switch: no flag
    try:
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        _walk_to(ctx, (ctx.n - 1) * s - 2)
        ctx.set_equal_time_correlators(True)
        ctx.measure_reset()
        ctx.measure_slice()
        old_off = ctx.measure_eq_read()
        slice_off = ctx.measure_read()
        assert ctx.lib.dqmc_measure_eq_band_accum_size(ctx.h) == 0
        _raises(ctx.measure_eq_band_read)
        ctx.set_equal_time_band(True)
        assert ctx.lib.dqmc_measure_eq_band_accum_size(ctx.h) == 1 + 2 * N
        ctx.measure_reset()
        g = ctx.g
        gs = shift_symmetric(ora, g)
        ref = eq_band_correlators(ora, gs)
        ctx.measure_slice()
        assert np.array_equal(ctx.g, g)
        assert np.array_equal(ctx.measure_eq_read(), old_off) and np.array_equal(ctx.measure_read(), slice_off)   # the old blocks: same bits
        acc = ctx.measure_eq_band_read()
        assert acc.shape == (1 + 2 * N,) and acc[0] == 1.0
        got = [acc[1:1 + N] / N, acc[1 + N:] / N]
        errs = [relerr(v, r) for v, r in zip(got, ref)]
        delta = eq_band_delta(ora, gs)
        e0 = [abs(v[0] - r[0]) / abs(r[0]) for v, r in zip(got, ref)]
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux}: bandDiff {errs[0]:.2e} bandMix {errs[1]:.2e}; d = 0 bin {e0[0]:.2e} {e0[1]:.2e} "
              f"(delta term {delta:.3f} of {ref[0][0]:.3f}, {ref[1][0]:.3f})")
        assert all(np.abs(r).max() > 1e-6 for r in ref) and abs(delta) > 0.1
        assert max(errs) < 1e-10 and max(e0) < 1e-10
        # the switches are independent: the band block alone, and a reset clears it
        ctx.set_equal_time_correlators(False)
        ctx.measure_slice()
        assert np.array_equal(ctx.measure_eq_read(), old_off) and ctx.measure_eq_band_read()[0] == 2.0
        assert np.array_equal(ctx.measure_eq_band_read()[1:], 2.0 * acc[1:])
        ctx.set_equal_time_band(False)
        ctx.measure_slice()
        assert ctx.measure_eq_band_read()[0] == 2.0
        ctx.measure_reset()
        assert not ctx.measure_eq_band_read().any()
    finally:
        ctx.close()


# ---- 6. series ---------------------------------------------------------------------------------------------------------------------
SER_M, SER_S, SER_NFREQ = 10, 5, 2
OLD_PARTS = 1 | 8 | 64                                   # equal-time, Matsubara of the particle-hole channel, order parameter


def _ser_fill(ctx, phis):
    """new fields and one down pass without updates that refills every block"""
    m, s, n = ctx.m, ctx.s, ctx.n
    _start(ctx, phis)
    ctx.set_equal_time_correlators(True)
    ctx.set_equal_time_band(True)
    for k in range(m, (n - 1) * s, -1):
        ctx.measure_slice()
        ctx.wrapDownGreen(k)
    ctx.set_equal_time_correlators(False)
    ctx.set_equal_time_band(False)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        ctx.measure_timedisplaced_segment(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


@functools.lru_cache(maxsize=None)
def _series_scenario():
    """L = 4, m = 10, s = 5, two chains, four fills.  The same fills feed three series one after the other -- the old parts alone with
    bins of one sample, all parts with bins of one sample (the samples themselves) and all parts with bins of two -- the blocks of a
    fill being bit-reproducible (test 2 and the tests of the other channels)."""
    L, N, nb = 4, 16, 2
    ctx = _context(2, L, SER_M, SER_S, every=True, nchains=nb)
    rec = dict(N=N, L=L, nb=nb)
    fills = [[_random_phi(2, N, SER_M, 7000 + 10 * i + c) * (0.5 + 0.5 * i) for c in range(nb)] for i in range(4)]
    new = OLD_PARTS | 128 | 256
    try:
        _ser_fill(ctx, fills[0])
        rec["parts32"] = _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, 32)) and _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, new | 32)) \
            and _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, new | 512))

        def run(parts, bin_size, max_bins):
            ctx.series_begin(bin_size, max_bins, SER_NFREQ, parts)
            layout = {p: ctx.series_layout(p) for p in range(9) if parts & (1 << p)}
            for p in range(9):
                if not parts & (1 << p):
                    _raises(lambda: ctx.series_layout(p))
            blocks = []
            for i, f in enumerate(fills):
                _ser_fill(ctx, f)
                if parts & 256:
                    per = []
                    for b in range(nb):
                        ctx.select_chain(b)
                        per.append((ctx.measure_eq_band_read(), ctx.measure_td_fine_read(4)))
                    ctx.select_chain(0)
                    blocks.append((per, ctx.measure_td_matsubara(4, SER_NFREQ)))
                ctx.series_add_sweep()
            bins = []
            for b in range(nb):
                ctx.select_chain(b)
                bins.append(ctx.series_bins())
            ctx.select_chain(0)
            return layout, ctx.series_info()[2], np.array(bins), blocks

        rec["old"] = run(OLD_PARTS, 1, 4)
        ctx.series_end()
        rec["one"] = run(new, 1, 4)
        ctx.series_end()
        rec["two"] = run(new, 2, 3)
        rec["stats"] = ctx.series_stats()
        rec["derived"] = ctx.series_band_derived()
        rec["derived2"] = ctx.series_band_derived()
        rec["old_derived"] = ctx.series_derived()
        st, exp = ctx.series_export()
        ctx.series_end()
        ctx.series_begin(2, 3, SER_NFREQ, new)
        _raises(ctx.series_band_derived)                 # fewer than two closed bins
        ctx.series_import(st, exp)
        bins = []
        for b in range(nb):
            ctx.select_chain(b)
            bins.append(ctx.series_bins())
        ctx.select_chain(0)
        rec["imported"] = (np.array(bins), ctx.series_stats(), ctx.series_band_derived())
        ctx.series_end()
        ctx.series_begin(1, 2, SER_NFREQ, OLD_PARTS)
        rec["no_part"] = _raises(ctx.series_band_derived)
        ctx.series_end()
    finally:
        ctx.close()
    return rec


def test_series_layout_and_old_parts():
    rec = _series_scenario()
    N = rec["N"]
    (lo, So, bo, _), (ln, Sn, bn, _) = rec["old"], rec["one"]
    assert rec["parts32"]
    assert lo == {p: ln[p] for p in lo}                  # the old parts keep their offsets ...
    assert So == 10 * N + 3 * SER_NFREQ * N * 2 + SER_NFREQ * N + 5
    assert ln[7] == (So, 2 * SER_NFREQ * N * 2) and ln[8] == (So + ln[7][1], 4 * N) and Sn == ln[8][0] + 4 * N
    assert np.array_equal(bn[:, :, :So], bo) and bo.any()      # ... and their bits


def test_series_bins_are_the_accumulated_samples():
    rec = _series_scenario()
    N, L, nb = rec["N"], rec["L"], rec["nb"]
    layout, S, samples, blocks = rec["one"]
    off7, off8 = layout[7][0], layout[8][0]
    worst = 0.0
    for i, (per, mats) in enumerate(blocks):
        for b in range(nb):
            eqb, _ = per[b]
            c = eqb[1:].reshape(2, N) / (float(N) * eqb[0])
            got = samples[b, i]
            assert np.array_equal(got[off8:off8 + 2 * N], c.ravel()) and np.abs(c).max() > 1e-6
            worst = max(worst, sr.rows_close(got[off8 + 2 * N:off8 + 4 * N], sr.structure_factor_ref(c, L).ravel(), 1e-12, N))
            assert np.array_equal(got[off7:off8], mats[b].ravel().view(np.float64)) and mats[b].any()
    print(f"samples: C(d) and the Matsubara part bit-identical to the readers; S(q): {worst:.2e} of the row's magnitude (bound 1e-12)")
    _, S2, bins2, _ = rec["two"]
    assert S2 == S and bins2.shape == (nb, 2, S)
    for b in range(nb):
        for k in range(2):
            assert np.array_equal(bins2[b, k], (samples[b, 2 * k] + samples[b, 2 * k + 1]) / 2.0), (b, k)
    ib, istats, ider = rec["imported"]
    assert np.array_equal(ib, bins2)
    assert all(np.array_equal(x, y) for x, y in zip(istats, rec["stats"]))
    assert all(np.array_equal(x, y) for x, y in zip(ider, rec["derived"]))


def test_series_statistics_and_ratios():
    """mean, err and the three R against the numpy jackknife over the closed bins, at the bounds of tests/test_gpu_series.py: mean 1e-13,
    err 1e-10 of the row's largest error, values of R 1e-12 absolute, errors of R 1e-10 of the entry's largest error"""
    from band_reference import correlation_ratios
    rec = _series_scenario()
    N, L, nb = rec["N"], rec["L"], rec["nb"]
    layout, S, bins, _ = rec["two"]
    off8 = layout[8][0]
    mean, err = rec["stats"]
    val, derr = rec["derived"]
    assert val.shape == (nb, 3) and np.array_equal(val, rec["derived2"][0]) and np.array_equal(derr, rec["derived2"][1])
    assert rec["no_part"]
    assert np.all(np.isfinite(rec["old_derived"][0][:, :5]))               # the old ratios are still served next to the new parts
    wm = we = 0.0
    ref = np.zeros((nb, 3, 2))
    for b in range(nb):
        rmean, rerr = sr.jackknife(bins[b])
        for r in range(4):
            sl = slice(off8 + r * N, off8 + (r + 1) * N)
            assert np.abs(bins[b][:, sl] - rmean[sl]).max() > 1e-3 * np.abs(rmean[sl]).max()     # the bins differ
            wm = max(wm, sr.rows_close(mean[b, sl], rmean[sl], 1e-13, N))
            we = max(we, sr.rows_close(err[b, sl], rerr[sl], 1e-10, N))
        for e in range(3):
            f = functools.partial(lambda x, e: correlation_ratios(x[off8 + 2 * N:off8 + 3 * N], x[off8 + 3 * N:off8 + 4 * N], L)[e], e=e)
            ref[b, e] = sr.jackknife(bins[b], f)
        sq = rmean[off8 + 2 * N:off8 + 4 * N].reshape(2, N)
        Q = (L // 2) * L + L // 2
        for row, q in ((sq[0], Q), (sq[0], 0), (sq[1], Q)):
            assert abs(row[q]) > 1e-3 * np.abs(row).max()                  # no ratio with a vanishing denominator
    dv = np.abs(val - ref[:, :, 0]).max()
    de = (np.abs(derr - ref[:, :, 1]).max(axis=0) / ref[:, :, 1].max(axis=0)).max()
    print(f"mean {wm:.2e} (1e-13), err {we:.2e} (1e-10); R_dCDW, R_nematic, R_bandMix = {val[0]} +- {derr[0]}: values {dv:.2e} (1e-12), "
          f"errors {de:.2e} of the entry's largest error (1e-10)")
    assert np.all(ref[:, :, 1] > 0.0)
    assert dv <= 1e-12 and de <= 1e-10


# ---- 7. host level -----------------------------------------------------------------------------------------------------------------
def _batch(band, seed=4712, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=True,
                  bandCorrelators=band, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


OLD_VECTORS = ("kOccX", "kOccY", "pairPlus", "pairMinus", "greenKTauX", "greenKTauY", "chargeTau", "spinZTau", "sdwTau", "chargeTauQ0",
               "spinZTauQ0", "sdwTauQ0", "chargeCorr", "spinZCorr", "sdwCorr", "pairPlusCorr", "pairMinusCorr", "chargeSq", "spinZSq",
               "sdwSq", "pairPlusSq", "pairMinusSq")
BAND_VECTORS = ("bandDiffTau", "bandMixTau", "bandDiffTauQ0", "bandMixTauQ0", "bandDiffCorr", "bandMixCorr", "bandDiffSq", "bandMixSq")


def test_host_level():
    from band_reference import band_correlators
    from detqmc_amd import DqmcError
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    a, b = _batch(False), _batch(True)
    try:
        for it in range(3):
            if it == 0:
                a.sweepThermalization(); b.sweepThermalization()
                continue
            before = [b.chain(c).phi.copy() for c in range(2)]
            a.sweep(True); b.sweep(True)
            for c in range(2):
                ra, rb = a.chain(c), b.chain(c)
                assert np.array_equal(ra.phi, rb.phi) and np.array_equal(ra.g, rb.g)
                assert ra.info.rngDrawn == rb.info.rngDrawn
                for nm in OLD_VECTORS:
                    assert np.array_equal(ra.observable_vector(nm), rb.observable_vector(nm)), nm
                info = rb.info
                n, s = info.n, info.s
                after = rb.phi.copy()
                down = info.lastSweepDir == -1
                vec = [rb.observable_vector(nm) for nm in BAND_VECTORS[:2]]
                q0 = [rb.observable_vector(nm) for nm in BAND_VECTORS[2:4]]
                assert all(v.shape == (n - 1, 16) for v in vec) and all(q.shape == (n - 1,) for q in q0)
                worst = 0.0
                for j in range(1, n):
                    tau = s * j
                    phi = before[c].copy()
                    if down:
                        phi[tau + 1:] = after[tau + 1:]
                    else:
                        phi[1:tau + 1] = after[1:tau + 1]
                    ora = make_oracle(phi, opdim=2, L=4, beta=2.0, dtau=0.1, s=s, delaySteps=4, r=b.pars_list[c].r)
                    ref = band_correlators(ora, *[shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)])
                    for v, q, r in zip(vec, q0, ref):
                        worst = max(worst, relerr(v[j - 1], r))
                        assert abs(q[j - 1] - v[j - 1].sum()) <= 1e-14 * max(1.0, np.abs(v[j - 1]).max()), (c, j)
                print(f"chain {c} down={down}: bandDiffTau / bandMixTau vs direct inverses, worst relerr {worst:.2e}")
                assert worst < 1e-10, (c, down, worst)
                for nm in BAND_VECTORS[4:]:
                    v = rb.observable_vector(nm)
                    assert v.shape == (16,) and np.abs(v).max() > 1e-6
                    with pytest.raises(DqmcError):
                        ra.observable_vector(nm)
                for nm in BAND_VECTORS[:4]:
                    with pytest.raises(DqmcError):
                        ra.observable_vector(nm)
                sq = [rb.observable_vector(nm) for nm in BAND_VECTORS[6:]]
                cd = [rb.observable_vector(nm) for nm in BAND_VECTORS[4:6]]
                for x, y in zip(sq, cd):
                    sr.rows_close(x, sr.structure_factor_ref(y, 4), 1e-12, 16)
    finally:
        a.close(); b.close()


def test_host_level_options():
    from detqmc_amd import DetSDW, DqmcError, SDWParams, _lib
    from detqmc_amd.model import _host_params
    kw = dict(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    with pytest.raises(ValueError):
        DetSDW(SDWParams(bandCorrelators=True, **kw))
    lib = _lib.load()
    for field, value in (("timeDisplacedParticleHole", 0x100), ("fermionMeasurements", 1 | 0x200), ("timeDisplacedParticleHole", 1 | 0x200)):
        p = _host_params(SDWParams(timeDisplacedMeasurements=True, **kw))
        setattr(p, field, value)                         # the flag without what it rides on, an unknown bit
        h = _lib.C.c_void_p()
        assert lib.detsdw_create(_lib.C.byref(p), _lib.C.byref(h)) == EINVAL, (field, value)
    rep = DetSDW(SDWParams(equalTimeCorrelators=True, bandCorrelators=True, **kw))      # equal-time alone
    try:
        rep.sweep(True)
        assert np.abs(rep.observable_vector("bandDiffSq")).max() > 1e-6
        with pytest.raises(DqmcError):
            rep.observable_vector("bandDiffTau")
    finally:
        rep.close()


# ---- 8. preconditions --------------------------------------------------------------------------------------------------------------
def test_preconditions_and_reset():
    from detqmc_amd import DqmcError, KernelContext
    phi = _random_phi(2, 16, 20, 3)
    for bad in dict(td=0, ph=True), dict(td=1, ph=False):                 # the flag without timedisplaced / without td_particle_hole >= 1
        with pytest.raises(DqmcError) as e:
            _context(2, 4, 20, 5, **bad)
        assert e.value.code == EINVAL
    ctx = _context(2, 4, 20, 5, band=False)
    try:
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)
        _raises(lambda: ctx.measure_timedisplaced_band(3))                # no block
        _raises(ctx.measure_td_band_read)
    finally:
        ctx.close()
    from detqmc_amd import DetHubbard, HubbardParams
    hub = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        h = hub.lib.dethubbard_ctx(hub.h)
        assert hub.lib.dqmc_set_equal_time_band(h, 1) == EINVAL and hub.lib.dqmc_measure_eq_band_accum_size(h) == 0
        assert hub.lib.dqmc_measure_timedisplaced_band(h, 1) == EINVAL and hub.lib.dqmc_measure_td_band_accum_size(h) == 0
    finally:
        hub.close()
    ctx = _context(2, 4, 20, 5)
    try:
        _start(ctx, [phi])
        _raises(lambda: ctx.measure_timedisplaced_band(3))                # no pair exists yet
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                                           # tau = 15, j = 3
        for j in (0, 2, 4):
            _raises(lambda: ctx.measure_timedisplaced_band(j))
        ctx.measure_timedisplaced_ph(3)
        ctx.measure_timedisplaced_band(3)                                 # after the particle-hole call, either order
        ctx.measure_timedisplaced(3)
        ctx.measure_timedisplaced_band(3)
        acc = ctx.measure_td_band_read()
        assert list(acc[:3]) == [0.0, 0.0, 2.0] and acc[3 + 2 * 32:].any() and not acc[3:3 + 2 * 32].any()
        assert list(ctx.measure_td_ph_read()[:3]) == [0.0, 0.0, 1.0]
        ctx.set_equal_time_band(True)
        ctx.measure_slice()
        assert ctx.measure_eq_band_read()[0] == 1.0
        ctx.wrapDownGreen(15)
        _raises(lambda: ctx.measure_timedisplaced_band(3))                # G has left the boundary
        ctx.measure_reset()
        assert not ctx.measure_td_band_read().any() and not ctx.measure_eq_band_read().any()
    finally:
        ctx.close()
