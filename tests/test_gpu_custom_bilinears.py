"""User-defined bilinear correlators on the device: the time-displaced and equal-time kernels against numpy on the device's own matrices
(tests/custom_reference.py) with four, three and one matrix set, agreement with every fixed particle-hole channel, the blocks'
bookkeeping, every slice and the Matsubara transform of channel 5, the preconditions, the series parts 9 and 10 with the correlation
ratio at a caller-chosen Q, and the host level: vectors, routed series, file round trip.

Tolerances are the project's: relerr < 1e-10 for a kernel against numpy on the device's own matrices, bit equality wherever a text says
so, and the bounds of tests/test_gpu_td_fine.py where that file sets one.  Every test prints its figures before it asserts."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import series_reference as sr
import td_fine_reference as tf
from conftest import relerr
from custom_reference import CUSTOM_MS, M_NX, M_RAND, M_SX_BANDX, M_SY_BANDY, custom_correlators, eq_custom_correlators
from test_gpu_band_correlators import EINVAL, KERNEL_CASES, _context, _raises, _start
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu


def _rows(acc, nrows, count, N):
    """(counts [nrows], sums [nrows][count][N]) of a time-displaced block"""
    return acc[:nrows], acc[nrows:].reshape(nrows, count, N)


# ---- 1. kernels against numpy on the device's own matrices -------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", KERNEL_CASES)
def test_kernels_vs_numpy_on_device_matrices(opdim, L, m, s, cb, bc, flux):
    """all four matrices in one launch, time-displaced at tau = 10 and equal-time on the G of the same boundary"""
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, band=False, checkerboard=cb, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == 0 and ctx.lib.dqmc_measure_eq_custom_accum_size(ctx.h) == 0
        ctx.set_custom_bilinears(CUSTOM_MS)
        assert np.array_equal(ctx.get_custom_bilinears(), np.array(CUSTOM_MS))
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == (n - 1) * (1 + 4 * N)
        assert ctx.lib.dqmc_measure_eq_custom_accum_size(ctx.h) == 1 + 4 * N
        _start(ctx, [phi])
        target = n - 2
        ref = {}

        def at(j):
            if j != target:
                return
            gtt = ctx.g
            _, gt0, g0t = ctx.green_timedisplaced()
            _, g00 = ctx.green0_timedisplaced()
            sh = [shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)]
            ref["td"] = custom_correlators(ora, CUSTOM_MS, *sh)
            ref["eq"] = eq_custom_correlators(ora, CUSTOM_MS, sh[0])
            ctx.measure_timedisplaced_custom(j)
            ctx.set_equal_time_custom(True)
            ctx.measure_slice()
            ctx.set_equal_time_custom(False)
            assert np.array_equal(ctx.g, gtt)            # the measurements leave G alone

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_read(), n - 1, 4, N)
        eq = ctx.measure_eq_custom_read()
        assert eq[0] == 1.0 and list(cnt) == [1.0 if j == target else 0.0 for j in range(1, n)]
        e_td = [relerr(rows[target - 1, c] / N, ref["td"][c]) for c in range(4)]
        e_eq = [relerr(eq[1 + c * N:1 + (c + 1) * N] / N, ref["eq"][c]) for c in range(4)]
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux}: time-displaced {['%.1e' % e for e in e_td]} "
              f"(max|C| {['%.3f' % np.abs(r).max() for r in ref['td']]}), equal-time {['%.1e' % e for e in e_eq]} "
              f"(max|C| {['%.3f' % np.abs(r).max() for r in ref['eq']]})")
        assert all(np.abs(r).max() > 1e-6 for r in ref["td"] + ref["eq"])
        assert max(e_td) < 1e-10 and max(e_eq) < 1e-10
        assert not np.delete(rows, target - 1, axis=0).any()           # the other boundaries stay untouched
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim", [1, 2, 3])
@pytest.mark.parametrize("which", [(3,), (2, 0, 1)])
def test_one_and_three_matrices(opdim, which):
    """count = 1 (a matrix with two entries: most of the non-zero mask is clear) and count = 3 in another order"""
    from td_reference import make_oracle, shift_symmetric
    L, m, s = 4, 20, 5
    N = L * L
    Ms = [CUSTOM_MS[i] for i in which]
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    ctx = _context(opdim, L, m, s, band=False)
    try:
        ctx.set_custom_bilinears(Ms)
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == (ctx.n - 1) * (1 + len(Ms) * N)
        _start(ctx, [phi])
        ref = {}

        def at(j):
            if j != 2:
                return
            sh = [shift_symmetric(ora, g) for g in (ctx.g, *ctx.green_timedisplaced()[1:], ctx.green0_timedisplaced()[1])]
            ref["td"] = custom_correlators(ora, Ms, *sh)
            ref["eq"] = eq_custom_correlators(ora, Ms, sh[0])
            ctx.measure_timedisplaced_custom(j)
            ctx.set_equal_time_custom(True)
            ctx.measure_slice()
            ctx.set_equal_time_custom(False)

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_read(), ctx.n - 1, len(Ms), N)
        eq = ctx.measure_eq_custom_read()
        assert eq.shape == (1 + len(Ms) * N,) and eq[0] == 1.0 and list(cnt) == [0.0, 1.0, 0.0]
        e_td = [relerr(rows[1, c] / N, ref["td"][c]) for c in range(len(Ms))]
        e_eq = [relerr(eq[1 + c * N:1 + (c + 1) * N] / N, ref["eq"][c]) for c in range(len(Ms))]
        print(f"O({opdim}) matrices {which}: time-displaced {e_td}, equal-time {e_eq}")
        assert all(np.abs(r).max() > 1e-6 for r in ref["td"] + ref["eq"])
        assert max(e_td) < 1e-10 and max(e_eq) < 1e-10
    finally:
        ctx.close()


# ---- 2. agreement with the fixed channels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_agreement_with_the_fixed_channels(opdim):
    """M = 1, M_SPINZ, M_BAND, M_MIX against charge / spinZ / bandDiff / bandMix and the mean of M_x, M_y[, M_z] against sdw, time-displaced
    and equal-time, relerr 1e-10: two kernels that evaluate the same sum in different orders"""
    from band_reference import M_BAND, M_MIX
    from td_ph_reference import M_CHARGE, M_SDW, M_SPINZ
    L, m, s = 4, 20, 5
    N = L * L
    ctx = _context(opdim, L, m, s, band=True)
    sets = ([M_CHARGE, M_SPINZ, M_BAND, M_MIX], list(M_SDW[:opdim]))
    got = []
    try:
        _start(ctx, [_random_phi(opdim, N, m, 811 + opdim)])
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_band(True)

        def at(j):
            if j != 2:
                return
            ctx.measure_timedisplaced_ph(j)
            ctx.measure_timedisplaced_band(j)
            for Ms in sets:
                ctx.set_custom_bilinears(Ms)             # replaces the matrices and their blocks
                ctx.set_equal_time_custom(True)
                ctx.measure_timedisplaced_custom(j)
                ctx.measure_slice()
                got.append((_rows(ctx.measure_td_custom_read(), ctx.n - 1, len(Ms), N)[1][1], ctx.measure_eq_custom_read()[1:].reshape(len(Ms), N)))
                ctx.set_equal_time_custom(False)
            ctx.set_equal_time_correlators(False)
            ctx.set_equal_time_band(False)

        _walk_down(ctx, at)
        ph = _rows(ctx.measure_td_ph_read(), ctx.n - 1, 3, N)[1][1]
        band = _rows(ctx.measure_td_band_read(), ctx.n - 1, 2, N)[1][1]
        eq, eqb = ctx.measure_eq_read(), ctx.measure_eq_band_read()
        assert eq[0] == 2.0 and eqb[0] == 2.0            # measure_slice ran twice with the same G: the sums are exact doubles
        eq, eqb = eq[1:1 + 3 * N].reshape(3, N) / 2.0, eqb[1:].reshape(2, N) / 2.0
        (td_a, eq_a), (td_b, eq_b) = got
        pairs = {"chargeTau": (td_a[0], ph[0]), "spinZTau": (td_a[1], ph[1]), "bandDiffTau": (td_a[2], band[0]), "bandMixTau": (td_a[3], band[1]),
                 "sdwTau": (td_b.mean(axis=0), ph[2]), "chargeCorr": (eq_a[0], eq[0]), "spinZCorr": (eq_a[1], eq[1]),
                 "bandDiffCorr": (eq_a[2], eqb[0]), "bandMixCorr": (eq_a[3], eqb[1]), "sdwCorr": (eq_b.mean(axis=0), eq[2])}
        errs = {k: relerr(a, b) for k, (a, b) in pairs.items()}
        print(f"O({opdim}): " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert all(np.abs(b).max() > 1e-6 for _, b in pairs.values())
        assert max(errs.values()) < 1e-10, errs
    finally:
        ctx.close()


# ---- 3. bookkeeping ----------------------------------------------------------------------------------------------------------------
def _measure_all(ctx, phis, Ms, twice_at=None, other=False):
    if Ms is not None:
        ctx.set_custom_bilinears(Ms)
    _start(ctx, phis)
    grabbed = {}

    def at(j):
        if Ms is not None:
            ctx.measure_timedisplaced_custom(j)
        if other:
            ctx.measure_timedisplaced_ph(j)
            ctx.measure_timedisplaced_band(j)
            ctx.measure_timedisplaced(j)
        if j == twice_at:
            ctx.select_chain(0)
            grabbed["once"] = ctx.measure_td_custom_read()
            ctx.measure_timedisplaced_custom(j)

    _walk_down(ctx, at)
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append(ctx.measure_td_custom_read() if Ms is not None else None)
    ctx.select_chain(0)
    return out, grabbed.get("once")


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_reproducibility_and_batching(opdim):
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 93 + opdim + 100 * c) for c in range(3)]
    blocks = []
    for rep in range(2):
        ctx = _context(opdim, 6, m, s, band=False)
        try:
            (acc,), once = _measure_all(ctx, phis[:1], CUSTOM_MS, twice_at=2)
            n = ctx.n
            (c1, v1), (c2, v2) = _rows(once, n - 1, 4, N), _rows(acc, n - 1, 4, N)
            assert list(c1) == [0.0, 1.0, 1.0] and list(c2) == [1.0, 2.0, 1.0]
            assert np.array_equal(v2[1], v1[1] + v1[1]) and np.array_equal(v2[2], v1[2]) and all(v1[1, c].any() for c in range(4))
            blocks.append(acc)
        finally:
            ctx.close()
    assert np.array_equal(blocks[0], blocks[1])                            # two fresh contexts: bit-identical
    ctx = _context(opdim, 6, m, s, band=False, nchains=3)
    try:
        three, _ = _measure_all(ctx, phis, CUSTOM_MS)
    finally:
        ctx.close()
    singles = []
    for phi in phis:
        ctx = _context(opdim, 6, m, s, band=False)
        try:
            singles.append(_measure_all(ctx, [phi], CUSTOM_MS)[0][0])
        finally:
            ctx.close()
    assert all(np.array_equal(three[b], singles[b]) for b in range(3))     # 1 chain against 3 chains
    assert not np.array_equal(singles[0], singles[1]) and not np.array_equal(singles[1], singles[2])


@pytest.mark.parametrize("opdim", [2, 3])
def test_other_blocks_do_not_see_the_option(opdim):
    """G, the per-slice block and the particle-hole / band / G(k, tau) / equal-time blocks: the same bits with matrices set and measured
    as without"""
    N, m, s = 16, 20, 5
    phi = _random_phi(opdim, N, m, 5 + opdim)
    seen = []
    for Ms in (None, CUSTOM_MS):
        ctx = _context(opdim, 4, m, s, band=True)
        try:
            _measure_all(ctx, [phi], Ms, other=True)
            ctx.set_equal_time_correlators(True)
            ctx.set_equal_time_band(True)
            if Ms is not None:
                ctx.set_equal_time_custom(True)
            ctx.measure_slice()
            seen.append([ctx.g, ctx.measure_read(), ctx.measure_td_read(), ctx.measure_td_ph_read(), ctx.measure_td_band_read(),
                         ctx.measure_eq_read(), ctx.measure_eq_band_read()])
        finally:
            ctx.close()
    for a, b in zip(*seen):
        assert np.array_equal(a, b) and a.any()


# ---- 4. every slice and the Matsubara transform of channel 5 -----------------------------------------------------------------------
@pytest.mark.parametrize("opdim,m", [(2, 20), (3, 22)])
def test_every_slice_and_matsubara(opdim, m):
    """one pass over all segments and the ends: every row count is 1, row j s is the coarse row j bit for bit; rows 0, m and one interior
    row against numpy on the device's own matrices (1e-10) and against direct inverses of the oracle's chain: rows 0 and m from G(0) alone
    (1e-10), the interior row within 10 e_ref -- the bounds of tests/test_gpu_td_fine.py.  Then the Matsubara transform of channel 5
    against numpy on the block, 1e-10."""
    import td_matsubara_reference as tm
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    L, s, nfreq = 4, 5, 3
    N = L * L
    phi = _random_phi(opdim, N, m, 41 * opdim + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    chain = Chain(ora)
    ctx = _context(opdim, L, m, s, band=False, every=True)

    def ref_of(gtt, gt0, g0t, g00):
        return np.array(custom_correlators(ora, CUSTOM_MS, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])) * N

    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == 0 and ctx.lib.dqmc_measure_td_matsubara_size(ctx.h, 5, nfreq) == 0
        ctx.set_custom_bilinears(CUSTOM_MS)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == (m + 1) * (1 + 4 * N)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 6) == 0
        _start(ctx, [phi])
        kin = s + 2
        dev = {}

        def at(j):
            if j == 1:
                g00 = ctx.green0_timedisplaced()[1]
                ctx.td_fine_propagate(1, kin)
                _, f_t0, f_0t, f_tt = ctx.green_td_fine()
                dev[kin] = ref_of(f_tt, f_t0, f_0t, g00)
            ctx.measure_timedisplaced_custom(j)
            ctx.measure_timedisplaced_segment(j)

        _walk_down(ctx, at)
        ctx.advanceDownGreen(1)
        g, one = ctx.g, np.eye(ctx.ng)
        dev[0], dev[m] = ref_of(g, g, g - one, g), ref_of(g, one - g, -g, g)
        ctx.measure_timedisplaced_ends()
        fine = ctx.measure_td_fine_read(5)
        cnt, rows = _rows(fine, m + 1, 4, N)
        assert np.array_equal(cnt, np.ones(m + 1))
        ccnt, crow = _rows(ctx.measure_td_custom_read(), n - 1, 4, N)
        assert np.array_equal(ccnt, np.ones(n - 1))
        for j in range(1, n):
            assert np.array_equal(rows[j * s], crow[j - 1]) and crow[j - 1].any(), j
        gd = chain.greens(m)[0]
        direct = {0: ref_of(gd, gd, gd - one, gd), m: ref_of(gd, one - gd, -gd, gd)}
        d_tt, d_t0, d_0t = chain.greens(kin)
        direct[kin] = ref_of(d_tt, d_t0, d_0t, four_greens(chain, kin)[3])
        e_ref = tf.e_ref()
        for k in (0, kin, m):
            e_dev, e_dir = relerr(rows[k], dev[k]), relerr(rows[k], direct[k])
            bound = 10 * e_ref if k == kin else 1e-10
            print(f"O({opdim}) m={m} row {k}: vs numpy on device matrices {e_dev:.2e} (1e-10), vs direct inverses {e_dir:.2e} ({bound:.2e})")
            assert all(np.abs(dev[k][c]).max() > 1e-6 for c in range(4))
            assert e_dev < 1e-10 and e_dir < bound, (k, e_dev, e_dir)
        assert ctx.lib.dqmc_measure_td_matsubara_size(ctx.h, 5, nfreq) == 4 * nfreq * N * 2
        a = ctx.measure_td_matsubara(5, nfreq)
        b = ctx.measure_td_matsubara(5, nfreq)
        assert a.shape == (1, 4, nfreq, N) and np.array_equal(a, b)
        assert np.array_equal(ctx.measure_td_fine_read(5), fine)           # the transform reads the block only
        for comp in range(4):
            ref = tm.bosonic(rows[:, comp] / N, L, 0.1, nfreq)
            e = relerr(a[0, comp], ref)
            print(f"O({opdim}) matrix {comp}: chi(q, i omega_n) vs numpy on the block {e:.2e} (bound 1e-10)")
            assert np.abs(ref).max() > 1e-6 and e <= 1e-10
        ctx.set_custom_bilinears([])                                       # removes every block
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == 0 and ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == 0
        _raises(lambda: ctx.measure_td_matsubara(5, nfreq))
        _raises(lambda: ctx.measure_td_fine_read(5))
    finally:
        ctx.close()


# ---- 5. preconditions --------------------------------------------------------------------------------------------------------------
def _snapshot(ctx):
    return [ctx.get_custom_bilinears(), ctx.measure_td_custom_read(), ctx.measure_eq_custom_read()]


def test_preconditions_and_reset():
    phi = _random_phi(2, 16, 20, 3)
    ctx = _context(2, 4, 20, 5, band=False)
    try:
        _raises(lambda: ctx.set_equal_time_custom(True))                  # no matrix is set
        _raises(lambda: ctx.measure_td_custom_read())
        ctx.set_custom_bilinears([M_RAND, M_NX])
        _start(ctx, [phi])
        _raises(lambda: ctx.measure_timedisplaced_custom(3))              # no pair exists yet
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                                           # tau = 15, j = 3
        ctx.measure_timedisplaced_custom(3)
        ctx.set_equal_time_custom(True)
        ctx.measure_slice()
        before = _snapshot(ctx)
        assert before[1][2] == 1.0 and before[2][0] == 1.0 and before[1][3 + 2 * 32:].any() and not before[1][3:3 + 2 * 32].any()
        nonherm, nan, zero = M_RAND.copy(), M_RAND.copy(), np.zeros((4, 4), dtype=complex)
        nonherm[0, 1] = complex(np.nextafter(nonherm[0, 1].real, 9.0), nonherm[0, 1].imag)       # one ulp off conj(M[1, 0])
        nan[2, 2] = np.nan
        inf = M_RAND.copy()
        inf[1, 3], inf[3, 1] = np.inf, np.inf
        for bad in ([nonherm], [M_NX, nan], [zero], [M_NX, zero], [inf], [M_NX] * 5):
            _raises(lambda: ctx.set_custom_bilinears(bad))
            assert all(np.array_equal(x, y) for x, y in zip(_snapshot(ctx), before))
        for j in (0, 2, 4):
            _raises(lambda: ctx.measure_timedisplaced_custom(j))
            assert all(np.array_equal(x, y) for x, y in zip(_snapshot(ctx), before))
        ctx.measure_timedisplaced_ph(3)
        ctx.measure_timedisplaced_custom(3)                               # after the particle-hole call, either order
        assert list(ctx.measure_td_custom_read()[:3]) == [0.0, 0.0, 2.0] and list(ctx.measure_td_ph_read()[:3]) == [0.0, 0.0, 1.0]
        ctx.wrapDownGreen(15)
        _raises(lambda: ctx.measure_timedisplaced_custom(3))              # G has left the boundary
        ctx.measure_reset()
        assert not ctx.measure_td_custom_read().any() and not ctx.measure_eq_custom_read().any()
        assert np.array_equal(ctx.get_custom_bilinears(), np.array([M_RAND, M_NX]))      # a reset clears sums, not matrices
        ctx.set_custom_bilinears([M_SY_BANDY])                            # a second call replaces the blocks, cleared
        assert ctx.measure_td_custom_read().shape == (3 * (1 + 16),) and not ctx.measure_eq_custom_read().any()
        ctx.measure_slice()                                               # the switch survives the replacement
        assert ctx.measure_eq_custom_read()[0] == 1.0
        ctx.set_custom_bilinears([])
        assert ctx.get_custom_bilinears().shape == (0, 4, 4)
        _raises(lambda: ctx.measure_eq_custom_read())
        ctx.measure_slice()                                               # and is off once no matrix is left
    finally:
        ctx.close()
    ctx = _context(2, 4, 20, 5, band=False, ph=False)                     # without td_particle_hole: equal time only
    try:
        ctx.set_custom_bilinears([M_SX_BANDX])
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == 0 and ctx.lib.dqmc_measure_eq_custom_accum_size(ctx.h) == 17
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)
        _raises(lambda: ctx.measure_timedisplaced_custom(3))
    finally:
        ctx.close()
    from detqmc_amd import DetHubbard, HubbardParams
    hub = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        h = hub.lib.dethubbard_ctx(hub.h)
        m = np.ascontiguousarray(M_NX)
        cnt = C.c_int(7)
        assert hub.lib.dqmc_set_custom_bilinears(h, 1, m.ctypes.data) == EINVAL
        assert hub.lib.dqmc_get_custom_bilinears(h, C.byref(cnt), None) == EINVAL and cnt.value == 7
        assert hub.lib.dqmc_set_equal_time_custom(h, 1) == EINVAL and hub.lib.dqmc_measure_eq_custom_accum_size(h) == 0
        assert hub.lib.dqmc_measure_timedisplaced_custom(h, 1) == EINVAL and hub.lib.dqmc_measure_td_custom_accum_size(h) == 0
    finally:
        hub.close()


# ---- 6. series parts 9 and 10 ------------------------------------------------------------------------------------------------------
SER_M, SER_S, SER_NFREQ = 10, 5, 2
OLD_PARTS = 1 | 8 | 64                                   # equal-time, Matsubara of the particle-hole channel, order parameter
SER_MS = (M_RAND, M_NX, M_SX_BANDX)
SER_SCALES = (0.5, 1.0, 3.5, 4.0)
SER_Q = (1, 3)                                           # a caller-chosen Q away from (pi, pi)


def _ser_fill(ctx, phis):
    """new fields and one down pass without updates that refills every block"""
    m, s, n = ctx.m, ctx.s, ctx.n
    _start(ctx, phis)
    ctx.set_equal_time_correlators(True)
    ctx.set_equal_time_custom(True)
    for k in range(m, (n - 1) * s, -1):
        ctx.measure_slice()
        ctx.wrapDownGreen(k)
    ctx.set_equal_time_correlators(False)
    ctx.set_equal_time_custom(False)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        ctx.measure_timedisplaced_segment(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


@functools.lru_cache(maxsize=None)
def _series_scenario():
    """L = 4, m = 10, s = 5, two chains, three matrices, four fills.  The same fills feed three series one after the other -- the old parts
    alone with bins of one sample, all parts with bins of one sample (the samples themselves) and all parts with bins of two -- the blocks
    of a fill being bit-reproducible."""
    L, N, nb = 4, 16, 2
    ctx = _context(2, L, SER_M, SER_S, band=False, every=True, nchains=nb)
    rec = dict(N=N, L=L, nb=nb)
    # the field scale differs much between the two halves of the fills: the sector-crossing matrix depends weakly on the field, and the
    # bins of two must differ by more than 1e-3 of their size (test_series_statistics_and_ratio, the floor of tests/test_gpu_series.py)
    fills = [[_random_phi(2, N, SER_M, 9000 + 10 * i + c) * SER_SCALES[i] for c in range(nb)] for i in range(4)]
    new = OLD_PARTS | 512 | 1024
    try:
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_correlators(False)
        rec["no_matrices"] = _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, 512)) and _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, 1024))
        ctx.set_custom_bilinears(SER_MS)
        _ser_fill(ctx, fills[0])
        rec["bad_masks"] = _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, new | 32)) and _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, new | 2048)) \
            and _raises(lambda: ctx.series_begin(1, 4, SER_NFREQ, new | 128))        # an unknown bit, and a band part without its block

        def run(parts, bin_size, max_bins):
            ctx.series_begin(bin_size, max_bins, SER_NFREQ, parts)
            layout = {p: ctx.series_layout(p) for p in range(11) if parts & (1 << p)}
            for p in range(12):
                if not parts & (1 << p):
                    _raises(lambda: ctx.series_layout(p))
            blocks = []
            for f in fills:
                _ser_fill(ctx, f)
                if parts & 1024:
                    per = []
                    for b in range(nb):
                        ctx.select_chain(b)
                        per.append(ctx.measure_eq_custom_read())
                    ctx.select_chain(0)
                    blocks.append((per, ctx.measure_td_matsubara(5, SER_NFREQ)))
                ctx.series_add_sweep()
            bins = []
            for b in range(nb):
                ctx.select_chain(b)
                bins.append(ctx.series_bins())
            ctx.select_chain(0)
            return layout, ctx.series_info()[2], np.array(bins), blocks

        rec["old"] = run(OLD_PARTS, 1, 4)
        ctx.set_custom_bilinears(SER_MS[:1])                 # a series without a custom part does not pin the matrices
        ctx.set_custom_bilinears(SER_MS)
        ctx.series_end()
        rec["one"] = run(new, 1, 4)
        ctx.series_end()
        rec["two"] = run(new, 2, 3)
        before = [ctx.get_custom_bilinears(), ctx.measure_eq_custom_read(), ctx.measure_td_fine_read(5), ctx.series_bins()]
        rec["set_while_open"] = _raises(lambda: ctx.set_custom_bilinears(SER_MS[:2])) and _raises(lambda: ctx.set_custom_bilinears([]))
        after = [ctx.get_custom_bilinears(), ctx.measure_eq_custom_read(), ctx.measure_td_fine_read(5), ctx.series_bins()]
        rec["unchanged"] = all(np.array_equal(x, y) for x, y in zip(before, after))
        rec["stats"] = ctx.series_stats()
        rec["derived"] = [ctx.series_custom_derived(), ctx.series_custom_derived(SER_Q), ctx.series_custom_derived(SER_Q)]
        rec["bad_q"] = _raises(lambda: ctx.series_custom_derived((4, 0))) and _raises(lambda: ctx.series_custom_derived((0, -1)))
        rec["old_derived"] = ctx.series_derived()
        st, exp = ctx.series_export()
        ctx.series_end()
        ctx.series_begin(2, 3, SER_NFREQ, new)
        _raises(ctx.series_custom_derived)                   # fewer than two closed bins
        ctx.series_import(st, exp)
        bins = []
        for b in range(nb):
            ctx.select_chain(b)
            bins.append(ctx.series_bins())
        ctx.select_chain(0)
        rec["imported"] = (np.array(bins), ctx.series_stats(), ctx.series_custom_derived(SER_Q))
        ctx.series_end()
        ctx.series_begin(1, 2, SER_NFREQ, OLD_PARTS)
        rec["no_part"] = _raises(ctx.series_custom_derived)
        ctx.series_end()
    finally:
        ctx.close()
    return rec


def test_series_layout_and_old_parts():
    rec = _series_scenario()
    N = rec["N"]
    (lo, So, bo, _), (ln, Sn, bn, _) = rec["old"], rec["one"]
    assert rec["no_matrices"] and rec["bad_masks"] and rec["set_while_open"] and rec["unchanged"]
    assert lo == {p: ln[p] for p in lo}                  # the old parts keep their offsets ...
    assert So == 10 * N + 3 * SER_NFREQ * N * 2 + SER_NFREQ * N + 5
    assert ln[9] == (So, 3 * SER_NFREQ * N * 2) and ln[10] == (So + ln[9][1], 6 * N) and Sn == ln[10][0] + 6 * N
    assert np.array_equal(bn[:, :, :So], bo) and bo.any()      # ... and their bits


def test_series_bins_are_the_accumulated_samples():
    rec = _series_scenario()
    N, L, nb = rec["N"], rec["L"], rec["nb"]
    layout, S, samples, blocks = rec["one"]
    off9, off10 = layout[9][0], layout[10][0]
    worst = 0.0
    for i, (per, mats) in enumerate(blocks):
        for b in range(nb):
            c = per[b][1:].reshape(3, N) / (float(N) * per[b][0])
            got = samples[b, i]
            assert np.array_equal(got[off10:off10 + 3 * N], c.ravel()) and all(np.abs(x).max() > 1e-6 for x in c)
            worst = max(worst, sr.rows_close(got[off10 + 3 * N:off10 + 6 * N], sr.structure_factor_ref(c, L).ravel(), 1e-12, N))
            assert np.array_equal(got[off9:off10], mats[b].ravel().view(np.float64)) and all(mats[b, k].any() for k in range(3))
    print(f"samples: C(d) and the Matsubara part bit-identical to the readers; S(q): {worst:.2e} of the row's magnitude (bound 1e-12)")
    _, S2, bins2, _ = rec["two"]
    assert S2 == S and bins2.shape == (nb, 2, S)
    for b in range(nb):
        for k in range(2):
            assert np.array_equal(bins2[b, k], (samples[b, 2 * k] + samples[b, 2 * k + 1]) / 2.0), (b, k)
    ib, istats, ider = rec["imported"]
    assert np.array_equal(ib, bins2)
    assert all(np.array_equal(x, y) for x, y in zip(istats, rec["stats"]))
    assert all(np.array_equal(x, y) for x, y in zip(ider, rec["derived"][1]))


def test_series_statistics_and_ratio():
    """mean, err and R at (pi, pi) and at the caller's Q against the numpy jackknife over the closed bins, at the bounds of
    tests/test_gpu_series.py: mean 1e-13, err 1e-10 of the row's largest error, values of R 1e-12 absolute, errors of R 1e-10 of the
    entry's largest error"""
    from custom_reference import correlation_ratio
    rec = _series_scenario()
    N, L, nb = rec["N"], rec["L"], rec["nb"]
    layout, S, bins, _ = rec["two"]
    off10 = layout[10][0]
    mean, err = rec["stats"]
    assert rec["no_part"] and rec["bad_q"]
    assert all(np.array_equal(x, y) for x, y in zip(rec["derived"][1], rec["derived"][2]))
    assert np.all(np.isfinite(rec["old_derived"][0][:, :5]))               # the old ratios are still served next to the new parts
    wm = we = 0.0
    for b in range(nb):
        rmean, rerr = sr.jackknife(bins[b])
        for r in range(6):
            sl = slice(off10 + r * N, off10 + (r + 1) * N)
            assert np.abs(bins[b][:, sl] - rmean[sl]).max() > 1e-3 * np.abs(rmean[sl]).max()     # the bins differ
            wm = max(wm, sr.rows_close(mean[b, sl], rmean[sl], 1e-13, N))
            we = max(we, sr.rows_close(err[b, sl], rerr[sl], 1e-10, N))
    for (val, derr), (qx, qy) in zip(rec["derived"][:2], ((L // 2, L // 2), SER_Q)):
        assert val.shape == (nb, 3)
        ref = np.zeros((nb, 3, 2))
        for b in range(nb):
            for e in range(3):
                sl = slice(off10 + (3 + e) * N, off10 + (4 + e) * N)
                ref[b, e] = sr.jackknife(bins[b], functools.partial(lambda x, sl: correlation_ratio(x[sl], L, qx, qy), sl=sl))
                row = sr.jackknife(bins[b])[0][sl]
                assert abs(row[qy * L + qx]) > 1e-3 * np.abs(row).max()    # no ratio with a vanishing denominator
        dv = np.abs(val - ref[:, :, 0]).max()
        de = (np.abs(derr - ref[:, :, 1]).max(axis=0) / ref[:, :, 1].max(axis=0)).max()
        print(f"Q = ({qx}, {qy}): R = {val[0]} +- {derr[0]}: values {dv:.2e} (1e-12), errors {de:.2e} of the entry's largest error (1e-10)")
        assert np.all(ref[:, :, 1] > 0.0)
        assert dv <= 1e-12 and de <= 1e-10
    print(f"mean {wm:.2e} (1e-13), err {we:.2e} (1e-10)")


# ---- 7. host level -----------------------------------------------------------------------------------------------------------------
def _batch(sub_batches, every=False, seed=4712, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=True,
                  timeDisplacedEverySlice=every, bandCorrelators=True, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)], sub_batches=sub_batches)


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_level(sub_batches):
    """a batch with matrices set against one without: the chains, G, the random numbers and every vector the band host test reads keep
    their bits; the custom vectors against numpy from direct inverses of the mixed field configuration of each boundary (1e-10), against
    the fixed band channels for M_BAND / M_MIX (1e-10), and their structure factors against the cosine sum (1e-12)"""
    from band_reference import M_BAND, M_MIX
    from detqmc_amd import DqmcError
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    from test_gpu_band_correlators import BAND_VECTORS, OLD_VECTORS
    Ms = [M_RAND, M_BAND, M_SX_BANDX, M_MIX]
    a, b = _batch(sub_batches), _batch(sub_batches)
    try:
        assert b.sub_batches == sub_batches
        a.sweepThermalization(); b.sweepThermalization()
        with pytest.raises(DqmcError):
            b.chain(0).observable_vector("custom0Tau")            # nothing is set yet
        b.set_custom_bilinears(Ms)
        for it in range(2):
            before = [b.chain(c).phi.copy() for c in range(2)]
            a.sweep(True); b.sweep(True)
            for c in range(2):
                ra, rb = a.chain(c), b.chain(c)
                assert np.array_equal(ra.phi, rb.phi) and np.array_equal(ra.g, rb.g) and ra.info.rngDrawn == rb.info.rngDrawn
                for nm in OLD_VECTORS + BAND_VECTORS:
                    assert np.array_equal(ra.observable_vector(nm), rb.observable_vector(nm)), nm
                with pytest.raises(DqmcError):
                    ra.observable_vector("custom0Tau")
                info = rb.info
                n, s = info.n, info.s
                after, down = rb.phi.copy(), info.lastSweepDir == -1
                vec = [rb.observable_vector(f"custom{k}Tau") for k in range(4)]
                q0 = [rb.observable_vector(f"custom{k}TauQ0") for k in range(4)]
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
                    ref = custom_correlators(ora, Ms, *[shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)])
                    for v, q, r in zip(vec, q0, ref):
                        worst = max(worst, relerr(v[j - 1], r))
                        assert abs(q[j - 1] - v[j - 1].sum()) <= 1e-14 * max(1.0, np.abs(v[j - 1]).max()), (c, j)
                fixed = max(relerr(vec[1], rb.observable_vector("bandDiffTau")), relerr(vec[3], rb.observable_vector("bandMixTau")),
                            relerr(rb.observable_vector("custom1Corr"), rb.observable_vector("bandDiffCorr")),
                            relerr(rb.observable_vector("custom3Sq"), rb.observable_vector("bandMixSq")))
                print(f"sub-batches {sub_batches} chain {c} down={down}: custom Tau vs direct inverses {worst:.2e}, vs the band channels {fixed:.2e}")
                assert worst < 1e-10 and fixed < 1e-10
                for k in range(4):
                    cd, sq = rb.observable_vector(f"custom{k}Corr"), rb.observable_vector(f"custom{k}Sq")
                    assert cd.shape == (16,) and np.abs(cd).max() > 1e-6
                    sr.rows_close(sq, sr.structure_factor_ref(cd, 4), 1e-12, 16)
        b.set_custom_bilinears(Ms[:2])                           # fewer matrices: the vectors of the others are gone
        b.sweep(True)
        assert b.chain(0).observable_vector("custom1Tau").shape == (3, 16)
        with pytest.raises(DqmcError):
            b.chain(0).observable_vector("custom2Tau")
        with pytest.raises(KeyError):
            b.chain(0).observable_vector("custom4Tau")
    finally:
        a.close(); b.close()


def test_host_level_options():
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    kw = dict(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    rep = DetSDWBatch([SDWParams(**kw)])                          # neither family the matrices could ride on
    try:
        with pytest.raises(DqmcError) as e:
            rep.set_custom_bilinears([M_NX])
        assert e.value.code == EINVAL and "equalTimeCorrelators" in str(e.value)
    finally:
        rep.close()
    rep = DetSDWBatch([SDWParams(equalTimeCorrelators=True, **kw)])   # equal time alone
    try:
        for bad in ([M_NX + 1j * M_SX_BANDX], [np.zeros((4, 4))], [M_NX] * 5):
            with pytest.raises(DqmcError):
                rep.set_custom_bilinears(bad)
        rep.set_custom_bilinears([M_NX])
        rep.sweep(True)
        assert np.abs(rep.chain(0).observable_vector("custom0Sq")).max() > 1e-6
        with pytest.raises(DqmcError):
            rep.chain(0).observable_vector("custom0Tau")
    finally:
        rep.close()


def test_host_level_series(tmp_path):
    """a routed series over three sweeps: the bins of the custom parts are the vectors / Matsubara transforms of the sweeps in the routed
    slots, R_custom at a caller-chosen Q against the numpy jackknife (1e-12), the file round trip, and the refusals"""
    from custom_reference import correlation_ratio
    from detqmc_amd import DqmcError
    Ms = [M_RAND, M_NX]
    b = _batch(2, every=True)
    path = str(tmp_path / "series.bin")
    try:
        b.sweepThermalization()
        b.set_custom_bilinears(Ms)
        b.sweep(True)                                             # before the series: the every-slice twins and the side effects of a set
        for c in range(2):
            r = b.chain(c)
            n, s, m = r.info.n, r.info.s, r.info.m
            for k in range(2):
                coarse, fine = r.observable_vector(f"custom{k}Tau"), r.observable_vector(f"custom{k}TauFine")
                q0, q0f = r.observable_vector(f"custom{k}TauQ0"), r.observable_vector(f"custom{k}TauQ0Fine")
                assert coarse.shape == (n - 1, 16) and fine.shape == (m + 1, 16) and q0.shape == (n - 1,) and q0f.shape == (m + 1,)
                for j in range(1, n):                             # row j s of the fine block is the coarse row j, bit for bit
                    assert np.array_equal(fine[j * s], coarse[j - 1]) and q0f[j * s] == q0[j - 1] and coarse[j - 1].any(), (c, k, j)
                assert np.all(np.abs(q0f - fine.sum(axis=1)) <= 1e-14 * np.maximum(1.0, np.abs(fine).max(axis=1))) and fine[0].any() and fine[m].any()
            with pytest.raises(KeyError):
                r.observable_vector("custom0CorrFine")
        charge = b.matsubara_all("chargeTau", 2)
        assert b.matsubara_all("custom1Tau", 2).any()
        b.set_custom_bilinears(Ms)                                # clears the custom blocks; the other channels' transforms stay valid
        assert np.array_equal(b.matsubara_all("chargeTau", 2), charge)
        with pytest.raises(DqmcError):
            b.matsubara_all("custom1Tau", 2)                      # its rows have no sample until the next measurement sweep
        b.series_begin(1, 4, nfreq=2)
        b.series_route([1, 0])
        seen = []
        for it in range(3):
            b.sweep(True)
            seen.append([(b.chain(c).observable_vector("custom0Corr"), b.chain(c).observable_vector("custom1Sq"),
                          b.chain(c).matsubara("custom1Tau", 2)) for c in range(2)])
        allm = b.matsubara_all("custom1Tau", 2)
        assert np.array_equal(allm[0], seen[-1][0][2]) and np.array_equal(allm[1], seen[-1][1][2])
        for c in range(2):
            slot = b.chain(1 - c)                                 # chain c fed slot 1 - c
            corr, sq, mats = slot.series_bins("custom0Corr"), slot.series_bins("custom1Sq"), slot.series_bins("custom1Tau")
            assert corr.shape == (3, 16) and mats.shape == (3, 2, 16)
            for it in range(3):
                sr.rows_close(corr[it], seen[it][c][0], 1e-14, 16)
                sr.rows_close(sq[it], seen[it][c][1], 1e-12, 16)
                assert np.array_equal(mats[it], seen[it][c][2]) and mats[it].any()
        mean, err = b.series_stats_all("custom1Sq")
        val, verr = b.series_derived_all("R_custom1", Q=(1, 0))
        dflt = b.series_derived_all("R_custom1")
        for c in range(2):
            bins = b.chain(c).series_bins("custom1Sq")
            rm, re_ = sr.jackknife(bins)
            sr.rows_close(mean[c], rm, 1e-13, 16)
            sr.rows_close(err[c], re_, 1e-10, 16)
            rv, rerr = sr.jackknife(bins, lambda x: correlation_ratio(x, 4, 1, 0))
            dv, dd = sr.jackknife(bins, lambda x: correlation_ratio(x, 4, 2, 2))
            print(f"slot {c}: R_custom1(1, 0) = {val[c]:.6f} +- {verr[c]:.2e} (numpy {rv:.6f} +- {rerr:.2e}), at (pi, pi) {dflt[0][c]:.6f}")
            assert abs(val[c] - rv) <= 1e-12 and abs(verr[c] - rerr) <= 1e-10 * rerr and abs(dflt[0][c] - dv) <= 1e-12
        with pytest.raises(DqmcError):
            b.series_derived_all("R_custom2")                     # no such matrix
        with pytest.raises(DqmcError):
            b.set_custom_bilinears([M_NX])                        # the open series holds their parts
        b.series_save(path)
        kept = [b.chain(c).series_bins("custom0Corr") for c in range(2)]
        b.series_end()
        b.series_begin(1, 4, nfreq=2)
        b.series_load(path)
        assert b.series_route() == [1, 0]
        assert all(np.array_equal(b.chain(c).series_bins("custom0Corr"), kept[c]) for c in range(2))
        b.series_end()
        b.set_custom_bilinears([M_RAND, M_SX_BANDX])              # same count, another matrix
        b.series_begin(1, 4, nfreq=2)
        with pytest.raises(DqmcError) as e:
            b.series_load(path)
        assert e.value.code == EINVAL and "bilinears" in str(e.value)
        b.series_end()
    finally:
        b.close()


def test_host_level_no_host_copy_and_fine_on_device():
    """NO_HOST_COPY and timeDisplacedFineOnDevice with matrices set behave as for the band channels: the equal-time vectors and the
    'Fine' twins are refused with the band ones, the coarse vectors, the Matsubara transforms and the series serve everything; the
    matrices cannot be set while such a series is open"""
    from detqmc_amd import DqmcError
    b = _batch(1, every=True, timeDisplacedFineOnDevice=True)
    try:
        b.sweepThermalization()
        b.set_custom_bilinears([M_RAND, M_SX_BANDX])
        b.series_begin(1, 4, nfreq=2, host_copy=False)
        with pytest.raises(DqmcError) as e:
            b.set_custom_bilinears([M_NX])
        assert e.value.code == EINVAL
        for it in range(2):
            b.sweep(True)
        r = b.chain(1)
        for nm in ("bandDiffCorr", "custom0Corr", "bandMixSq", "custom1Sq", "bandDiffTauFine", "custom0TauFine", "bandMixTauQ0Fine", "custom1TauQ0Fine"):
            with pytest.raises(DqmcError):
                r.observable_vector(nm)
        n = r.info.n
        assert r.observable_vector("custom1Tau").shape == (n - 1, 16) and r.observable_vector("custom1Tau").any()
        corr, sq, mats = r.series_bins("custom0Corr"), r.series_bins("custom1Sq"), r.series_bins("custom1Tau")
        assert corr.shape == (2, 16) and sq.shape == (2, 16) and mats.shape == (2, 2, 16)
        assert all(np.abs(x).max() > 1e-6 for x in (corr[0], corr[1], sq[1], mats[1])) and not np.array_equal(corr[0], corr[1])
        assert np.array_equal(mats[1], r.matsubara("custom1Tau", 2))      # the last sweep's transform, from the block that stayed on the device
        for k in range(2):
            sr.rows_close(r.series_bins("custom0Sq")[k], sr.structure_factor_ref(corr[k], 4), 1e-12, 16)
        b.series_end()
        b.set_custom_bilinears([M_NX])                           # allowed again
        b.sweep(True)
        assert np.abs(r.observable_vector("custom0Corr")).max() > 1e-6
    finally:
        b.close()
