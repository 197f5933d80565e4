"""User-defined pair operators on the device: the two kernels against numpy on the device's own matrices
(tests/custom_pair_reference.py), the fixed pairing channels and the stencil / on-site agreement, reproducibility, batching and the
channel -> row mapping, every slice and the Matsubara transform, independence of everything that existed, the refusals, the series
parts, and the host level: vectors, Matsubara by name, a routed series with R_customPair at a chosen Q, the file round trip.

Tolerances are the project's: relerr < 1e-10 for a kernel against numpy on the device's own matrices, 1e-13 of the largest entry
between two kernels that evaluate the same sums, bit equality wherever a text says so, and the bounds of tests/test_gpu_td_fine.py where
that file sets one.  Every test prints its figures before it asserts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import custom_pair_reference as cp
import series_reference as sr
import td_fine_reference as tf
from conftest import relerr
from custom_reference import M_NX, M_RAND, correlation_ratio
from test_gpu_band_correlators import EINVAL, KERNEL_CASES, _context, _raises, _start
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu


def _rows(acc, nrows, count, N):
    """(counts [nrows], sums [nrows][count][N]) of a time-displaced block"""
    return acc[:nrows], acc[nrows:].reshape(nrows, count, N)


def _same_ops(got, ops):
    return len(got) == len(ops) and all(np.array_equal(g, w) for a, b in zip(got, ops) for g, w in zip(a, cp.as_arrays(b)))


def _measure_both(ctx, j):
    """time-displaced at boundary j and equal-time on the G of the same boundary"""
    ctx.measure_timedisplaced_custom_pair(j)
    ctx.set_equal_time_custom_pair(True)
    ctx.measure_slice()
    ctx.set_equal_time_custom_pair(False)


def _maxrel(a, b):
    """largest deviation in units of the largest entry"""
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ---- 1. kernels against numpy on the device's own matrices -------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,s,cbd,bc,flux", KERNEL_CASES)
def test_kernels_vs_numpy_on_device_matrices(opdim, L, m, s, cbd, bc, flux):
    """all four operators in one launch (the stencil kernel; under flux four on-site operators: the on-site kernel), time-displaced at
    boundary n - 2 and equal-time on the G of the same boundary; the context has no particle-hole blocks: timedisplaced >= 1 is enough"""
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cbd, weakZflux=flux, delaySteps=4)
    ops = cp.pair_ops(flux)
    ctx = _context(opdim, L, m, s, band=False, ph=False, checkerboard=cbd, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        ctx.set_custom_pair_operators(ops)
        assert _same_ops(ctx.get_custom_pair_operators(), ops)
        assert ctx.lib.dqmc_measure_td_custom_pair_accum_size(ctx.h) == (n - 1) * (1 + 4 * N)
        assert ctx.lib.dqmc_measure_eq_custom_pair_accum_size(ctx.h) == 1 + 4 * N
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == 0 and ctx.lib.dqmc_measure_td_ph_accum_size(ctx.h) == 0
        _start(ctx, [phi])
        target = n - 2
        ref = {}

        def at(j):
            if j != target:
                return
            gtt = ctx.g
            ref["td"] = cp.pair_correlators(ora, ops, shift_symmetric(ora, ctx.green_timedisplaced()[1]))
            ref["eq"] = cp.pair_correlators(ora, ops, shift_symmetric(ora, gtt))
            _measure_both(ctx, j)
            assert np.array_equal(ctx.g, gtt)            # the measurements leave G alone

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_pair_read(), n - 1, 4, N)
        eq = ctx.measure_eq_custom_pair_read()
        assert eq[0] == 1.0 and list(cnt) == [1.0 if j == target else 0.0 for j in range(1, n)]
        e_td = [relerr(rows[target - 1, c] / N, ref["td"][c]) for c in range(4)]
        e_eq = [relerr(eq[1 + c * N:1 + (c + 1) * N] / N, ref["eq"][c]) for c in range(4)]
        print(f"O({opdim}) L={L} {bc} cb={cbd} flux={flux}: time-displaced {['%.1e' % e for e in e_td]} "
              f"(max|C| {['%.3f' % np.abs(r).max() for r in ref['td']]}), equal-time {['%.1e' % e for e in e_eq]} "
              f"(max|C| {['%.3f' % np.abs(r).max() for r in ref['eq']]})")
        assert all(np.abs(r).max() > 1e-6 for r in ref["td"] + ref["eq"])
        assert max(e_td) < 1e-10 and max(e_eq) < 1e-10
        assert not np.delete(rows, target - 1, axis=0).any()           # the other boundaries stay untouched
    finally:
        ctx.close()


# ---- 2. cross-checks on the same context -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,flux", [(1, False), (2, False), (3, False), (2, True)])
def test_fixed_channels_and_stencil_vs_onsite(opdim, flux):
    """on one context at one boundary: the 's' and 'd_band' rows are the pair block of dqmc_measure_timedisplaced_pair (and the
    pairPlus / pairMinus rows of the equal-time block) divided by 4, and the stencil kernel with zero bond parts on some operators
    equals the on-site kernel on those operators: 1e-13 of the largest entry"""
    from detqmc_amd import pair_operator
    L, m, s = 4, 20, 5
    N = L * L
    phi = _random_phi(opdim, N, m, 911 + opdim)
    site = [pair_operator("s"), pair_operator("d_band"), cp.P_ONSITE]
    ctx = _context(opdim, L, m, s, band=False, ph=False, td=2, weakZflux=flux)
    got = {}
    try:
        _start(ctx, [phi])

        def at(j):
            if j != 2:
                return
            ctx.measure_timedisplaced_pair(j)
            ctx.set_equal_time_correlators(True)
            ctx.set_custom_pair_operators(site)           # the on-site kernel
            ctx.set_equal_time_custom_pair(True)
            ctx.measure_timedisplaced_custom_pair(j)
            ctx.measure_slice()
            ctx.set_equal_time_correlators(False)
            got["site"] = (_rows(ctx.measure_td_custom_pair_read(), ctx.n - 1, 3, N)[1][1], ctx.measure_eq_custom_pair_read()[1:].reshape(3, N))
            if not flux:
                ctx.set_custom_pair_operators([cp.P_RAND] + site)       # the stencil kernel, the same three behind a bond operator
                assert ctx.measure_eq_custom_pair_read()[0] == 0.0      # a replacement clears the block and keeps the switch
                ctx.measure_timedisplaced_custom_pair(j)
                ctx.set_equal_time_correlators(False)
                ctx.measure_slice()
                got["bond"] = (_rows(ctx.measure_td_custom_pair_read(), ctx.n - 1, 4, N)[1][1][1:], ctx.measure_eq_custom_pair_read()[1 + N:].reshape(3, N))

        _walk_down(ctx, at)
        pair = ctx.measure_td_pair_read()
        off = (ctx.n - 1) + 1 * 2 * N
        plus, minus = pair[off:off + N], pair[off + N:off + 2 * N]
        eqb = ctx.measure_eq_read()
        assert pair[1] == 1.0 and eqb[0] == 1.0
        td_s, eq_s = got["site"]
        errs = {"s td": _maxrel(4 * td_s[0], plus), "d_band td": _maxrel(4 * td_s[1], minus),
                "s eq": _maxrel(4 * eq_s[0], eqb[1 + 3 * N:1 + 4 * N]), "d_band eq": _maxrel(4 * eq_s[1], eqb[1 + 4 * N:1 + 5 * N])}
        if not flux:
            td_b, eq_b = got["bond"]
            for c, name in enumerate(("s", "d_band", "onsite")):
                errs[f"stencil {name} td"] = _maxrel(td_b[c], td_s[c])
                errs[f"stencil {name} eq"] = _maxrel(eq_b[c], eq_s[c])
        print(f"O({opdim}) flux={flux}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        assert min(np.abs(x).max() for x in (plus, minus, td_s[2], eq_s[2])) > 1e-6
        assert max(errs.values()) < 1e-13, errs
    finally:
        ctx.close()


# ---- 3. reproducibility, batching, the mask and the channel -> row mapping ---------------------------------------------------------
def _measure_all(ctx, phis, ops, passes=1):
    ctx.set_custom_pair_operators(ops)
    out = []
    for _ in range(passes):
        _start(ctx, phis)

        def at(j):
            _measure_both(ctx, j)

        _walk_down(ctx, at)
        per = []
        for b in range(len(phis)):
            ctx.select_chain(b)
            per.append((ctx.measure_td_custom_pair_read(), ctx.measure_eq_custom_pair_read()))
        ctx.select_chain(0)
        out.append(per)
    return out


@pytest.mark.parametrize("opdim,bonds", [(2, True), (3, True), (2, False)])
def test_reproducibility_and_batching(opdim, bonds):
    """two identical measurement passes give bit-identical blocks; two chains in one context equal two single-chain contexts"""
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 97 + opdim + 100 * c) for c in range(2)]
    ops = cp.pair_ops(flux=not bonds)
    ctx = _context(opdim, 6, m, s, band=False, ph=False, nchains=2)
    try:
        first, second = _measure_all(ctx, phis, ops, passes=2)
    finally:
        ctx.close()
    for b in range(2):
        assert np.array_equal(first[b][0], second[b][0]) and np.array_equal(first[b][1], second[b][1])
        assert np.array_equal(first[b][0][:ctx.n - 1], np.ones(ctx.n - 1)) and first[b][1][0] == ctx.n - 1
        assert all(r.any() for r in _rows(first[b][0], ctx.n - 1, 4, N)[1].reshape(-1, N))
    singles = []
    for phi in phis:
        ctx = _context(opdim, 6, m, s, band=False, ph=False)
        try:
            singles.append(_measure_all(ctx, [phi], ops)[0][0])
        finally:
            ctx.close()
    assert all(np.array_equal(first[b][k], singles[b][k]) for b in range(2) for k in range(2))
    assert not np.array_equal(singles[0][0], singles[1][0]) and not np.array_equal(singles[0][1], singles[1][1])


@pytest.mark.parametrize("opdim", [1, 2, 3])
@pytest.mark.parametrize("which", [(1,), (2,), (2, 0, 3), (2, 1, 2), (3, 2, 2, 2), (2, 2, 2, 0)])
def test_mask_and_channel_mapping(opdim, which):
    """one, three and four operators with the bond-carrying ones in different positions (index 2 is the on-site-only operator, which
    takes part in the stencil launch through the mask; (2,) alone runs the on-site kernel): every channel lands in its row"""
    from td_reference import make_oracle, shift_symmetric
    L, m, s = 4, 20, 5
    N = L * L
    ops = [cp.pair_ops()[i] for i in which]
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    ctx = _context(opdim, L, m, s, band=False, ph=False)
    try:
        ctx.set_custom_pair_operators(ops)
        assert ctx.lib.dqmc_measure_td_custom_pair_accum_size(ctx.h) == (ctx.n - 1) * (1 + len(ops) * N)
        _start(ctx, [phi])
        ref = {}

        def at(j):
            if j != 2:
                return
            ref["td"] = cp.pair_correlators(ora, ops, shift_symmetric(ora, ctx.green_timedisplaced()[1]))
            ref["eq"] = cp.pair_correlators(ora, ops, shift_symmetric(ora, ctx.g))
            _measure_both(ctx, j)

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_pair_read(), ctx.n - 1, len(ops), N)
        eq = ctx.measure_eq_custom_pair_read()
        assert eq.shape == (1 + len(ops) * N,) and eq[0] == 1.0 and list(cnt) == [0.0, 1.0, 0.0]
        e_td = [relerr(rows[1, c] / N, ref["td"][c]) for c in range(len(ops))]
        e_eq = [relerr(eq[1 + c * N:1 + (c + 1) * N] / N, ref["eq"][c]) for c in range(len(ops))]
        print(f"O({opdim}) operators {which}: time-displaced {e_td}, equal-time {e_eq}")
        assert all(np.abs(r).max() > 1e-6 for r in ref["td"] + ref["eq"])
        assert max(e_td) < 1e-10 and max(e_eq) < 1e-10
    finally:
        ctx.close()


# ---- 4. every slice and the Matsubara transform ------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,m", [(2, 20), (3, 22)])
def test_every_slice_and_matsubara(opdim, m):
    """one pass over all segments and the ends: every row count is 1, row j s of the fine block is the coarse row j bit for bit; rows 0, m
    and one interior row against numpy on the device's own matrices (1e-10) and against direct inverses of the oracle's chain: rows 0
    and m from G(0) alone (1e-10), the interior row within 10 e_ref -- the bounds of tests/test_gpu_td_fine.py.  Then
    matsubara(channel 6, 4 frequencies) against the numpy transform of the fine block, 1e-10."""
    import td_matsubara_reference as tm
    from td_reference import Chain, make_oracle, shift_symmetric
    L, s, nfreq = 4, 5, 4
    N = L * L
    ops = cp.pair_ops()
    phi = _random_phi(opdim, N, m, 43 * opdim + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    chain = Chain(ora)
    ctx = _context(opdim, L, m, s, band=False, ph=False, every=True)

    def ref_of(gt0):
        return np.array(cp.pair_correlators(ora, ops, shift_symmetric(ora, gt0))) * N

    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 6) == 0
        ctx.set_custom_pair_operators(ops)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 6) == (m + 1) * (1 + 4 * N)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == 0 and ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == 0
        _start(ctx, [phi])
        kin = s + 2
        dev = {}

        def at(j):
            if j == 1:
                ctx.td_fine_propagate(1, kin)
                dev[kin] = ref_of(ctx.green_td_fine()[1])
            ctx.measure_timedisplaced_custom_pair(j)
            ctx.measure_timedisplaced_segment(j)

        _walk_down(ctx, at)
        ctx.advanceDownGreen(1)
        g, one = ctx.g, np.eye(ctx.ng)
        dev[0], dev[m] = ref_of(g), ref_of(one - g)
        ctx.measure_timedisplaced_ends()
        fine = ctx.measure_td_fine_read(6)
        cnt, rows = _rows(fine, m + 1, 4, N)
        assert np.array_equal(cnt, np.ones(m + 1))
        ccnt, crow = _rows(ctx.measure_td_custom_pair_read(), n - 1, 4, N)
        assert np.array_equal(ccnt, np.ones(n - 1))
        for j in range(1, n):
            assert np.array_equal(rows[j * s], crow[j - 1]) and crow[j - 1].any(), j
        gd = chain.greens(m)[0]
        direct = {0: ref_of(gd), m: ref_of(one - gd), kin: ref_of(chain.greens(kin)[1])}
        e_ref = tf.e_ref()
        for k in (0, kin, m):
            e_dev, e_dir = relerr(rows[k], dev[k]), relerr(rows[k], direct[k])
            bound = 10 * e_ref if k == kin else 1e-10
            print(f"O({opdim}) m={m} row {k}: vs numpy on device matrices {e_dev:.2e} (1e-10), vs direct inverses {e_dir:.2e} ({bound:.2e})")
            assert all(np.abs(dev[k][c]).max() > 1e-6 for c in range(4))
            assert e_dev < 1e-10 and e_dir < bound, (k, e_dev, e_dir)
        a = ctx.measure_td_matsubara(6, nfreq)
        assert a.shape == (1, 4, nfreq, N) and np.array_equal(a, ctx.measure_td_matsubara(6, nfreq))
        assert np.array_equal(ctx.measure_td_fine_read(6), fine)           # the transform reads the block only
        for comp in range(4):
            ref = tm.bosonic(rows[:, comp] / N, L, 0.1, nfreq)
            e = relerr(a[0, comp], ref)
            print(f"O({opdim}) operator {comp}: P(q, i omega_n) vs numpy on the block {e:.2e} (bound 1e-10)")
            assert np.abs(ref).max() > 1e-6 and e <= 1e-10
    finally:
        ctx.close()


# ---- 5. with no pair operator set nothing changes; the two custom families are independent -----------------------------------------
def _all_blocks(ctx):
    out = [ctx._read_block(ctx.lib.dqmc_measure_accum_size, ctx.lib.dqmc_measure_read_host), ctx.measure_td_pair_read(), ctx.measure_td_ph_read(),
           ctx.measure_td_band_read(), ctx.measure_td_custom_read(), ctx.measure_eq_read(), ctx.measure_eq_band_read(), ctx.measure_eq_custom_read()]
    out += [ctx.measure_td_fine_read(ch) for ch in (0, 1, 2, 4, 5)]
    return out


def _full_pass(ctx, phi, touch):
    """a down pass with every channel at every boundary and on every slice; touch(ctx, j) runs at every boundary"""
    ctx.set_custom_bilinears([M_RAND, M_NX])
    _start(ctx, [phi])
    for f in (ctx.set_equal_time_correlators, ctx.set_equal_time_band, ctx.set_equal_time_custom):
        f(True)

    def at(j):
        touch(ctx, j)
        for f in (ctx.measure_timedisplaced, ctx.measure_timedisplaced_pair, ctx.measure_timedisplaced_ph, ctx.measure_timedisplaced_band,
                  ctx.measure_timedisplaced_custom, ctx.measure_timedisplaced_segment):
            f(j)
        ctx.measure_slice()

    _walk_down(ctx, at)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()
    return _all_blocks(ctx), ctx.g


def test_no_operator_set_changes_nothing_and_the_families_are_independent():
    """every existing block and G after a full measurement pass: a context that never saw the call, one where pair operators were set
    and removed again before the pass, and one that measures pair operators at every boundary beside the rest -- all bit-identical.
    After count = 0 the sizes are 0 again; setting the bilinears leaves the pair blocks' bits alone."""
    L, m, s = 4, 20, 5
    phi = _random_phi(2, L * L, m, 5)
    results = []

    def nothing(ctx, j):
        pass

    def set_and_remove(ctx, j):
        if j == ctx.n - 1:
            sizes = lambda: [ctx.lib.dqmc_measure_td_custom_pair_accum_size(ctx.h), ctx.lib.dqmc_measure_eq_custom_pair_accum_size(ctx.h),
                             ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 6)]
            assert sizes() == [0, 0, 0]
            ctx.set_custom_pair_operators(cp.pair_ops())
            assert sizes() == [(ctx.n - 1) * (1 + 64), 1 + 64, (m + 1) * (1 + 64)]
            ctx.set_custom_pair_operators([])
            assert sizes() == [0, 0, 0] and ctx.get_custom_pair_operators() == []
            _raises(lambda: ctx.set_equal_time_custom_pair(True))
            _raises(lambda: ctx.measure_timedisplaced_custom_pair(j))
            _raises(lambda: ctx.measure_td_custom_pair_read())

    kept = {}

    def beside(ctx, j):
        if j == ctx.n - 1:
            ctx.set_custom_pair_operators(cp.pair_ops())
            ctx.set_equal_time_custom_pair(True)                         # the pass's own measure_slice fills the equal-time block
        if j == 2:                                                       # the reverse: the bilinears' setter leaves the pair blocks alone
            before = (ctx.measure_td_custom_pair_read(), ctx.measure_eq_custom_pair_read(), ctx.get_custom_pair_operators())
            assert before[0].any() and before[1].any()
            kept["bilinear blocks cleared"] = True
            ctx.set_custom_bond_bilinears([(M_RAND, None, None), (M_NX, None, None)])     # replaces and clears the bilinears' blocks
            assert not ctx.measure_td_custom_read().any() and ctx.set_equal_time_custom(True) is None
            assert np.array_equal(ctx.measure_td_custom_pair_read(), before[0]) and np.array_equal(ctx.measure_eq_custom_pair_read(), before[1])
            assert _same_ops(ctx.get_custom_pair_operators(), before[2])
        ctx.measure_timedisplaced_custom_pair(j)

    for touch in (nothing, set_and_remove, beside):
        ctx = _context(2, L, m, s, td=2, every=True)
        try:
            results.append(_full_pass(ctx, phi, touch))
            if touch is beside:
                pair_td = ctx.measure_td_custom_pair_read()
                assert np.array_equal(pair_td[:ctx.n - 1], np.ones(ctx.n - 1)) and ctx.measure_eq_custom_pair_read()[0] == ctx.n - 1
                assert np.array_equal(ctx.measure_td_fine_read(6)[:m + 1], np.ones(m + 1))
        finally:
            ctx.close()
    (base, g0), (removed, g1), (with_pair, g2) = results
    assert np.array_equal(g0, g1) and np.array_equal(g0, g2)
    assert all(np.array_equal(x, y) and x.any() for x, y in zip(base, removed))
    # the third context replaced the bilinears at boundary 2 (which clears their blocks): every block but theirs is bit-identical
    custom = (4, 7, 12)
    assert all(np.array_equal(x, y) for k, (x, y) in enumerate(zip(base, with_pair)) if k not in custom)
    assert kept["bilinear blocks cleared"] and all(not np.array_equal(base[k], with_pair[k]) for k in custom)


# ---- 6. preconditions and refusals ---------------------------------------------------------------------------------------------------
def _snapshot(ctx):
    got = ctx.get_custom_pair_operators()
    return [np.array([op[k] for op in got]) for k in range(3)] + [ctx.measure_td_custom_pair_read(), ctx.measure_eq_custom_pair_read()]


def _unchanged(ctx, before):
    return all(np.array_equal(x, y) for x, y in zip(_snapshot(ctx), before))


def test_preconditions():
    """every refusal leaves operators, blocks and switches untouched"""
    from detqmc_amd import DqmcError
    phi = _random_phi(2, 16, 20, 3)
    ctx = _context(2, 4, 20, 5, band=False, ph=False)
    try:
        _raises(lambda: ctx.set_equal_time_custom_pair(True))             # no operator yet
        _raises(lambda: ctx.measure_td_custom_pair_read())
        ops = [cp.P_SYM_BOND, cp.P_ONSITE]
        ctx.set_custom_pair_operators(ops)
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                                           # tau = 15, j = 3
        _raises(lambda: ctx.measure_timedisplaced_custom_pair(2))         # not the boundary the pair belongs to
        _measure_both(ctx, 3)
        ctx.set_equal_time_custom_pair(True)
        before = _snapshot(ctx)
        assert before[3][2] == 1.0 and before[4][0] == 1.0 and before[3][3 + 2 * 32:].any() and not before[3][3:3 + 2 * 32].any()
        F0, Fx, Fy = cp.P_RAND
        nan, inf = Fx.copy(), F0.copy()
        nan[2, 1] = np.nan
        inf[0, 3] = np.inf
        sym = cp.P_SYM_BOND[0]
        zero = np.zeros((4, 4))
        for bad in ([cp.P_ONSITE, (F0, nan, None)], [(inf, None, Fy)], [(None, None, None)], [cp.P_ONSITE, (sym, zero, None)], [(sym, None, None)],
                    [cp.P_ONSITE] * 5):
            _raises(lambda: ctx.set_custom_pair_operators(bad))
            assert _unchanged(ctx, before)
        ctx.measure_slice()                                               # the switch is still on
        assert ctx.measure_eq_custom_pair_read()[0] == 2.0
        ctx.set_custom_pair_operators([(sym, Fx, None)])                  # a symmetric F0 with a bond part is legal
        got = ctx.get_custom_pair_operators()
        assert len(got) == 1 and np.array_equal(got[0][0], sym) and np.array_equal(got[0][1], Fx) and not got[0][2].any()
        assert not ctx.measure_td_custom_pair_read().any() and ctx.measure_td_custom_pair_read().shape == (3 * (1 + 16),)
        # an open series with a pair part holds the operators; a series without one does not
        ctx.series_begin(1, 2, 0, 4096)
        before = _snapshot(ctx)
        _raises(lambda: ctx.set_custom_pair_operators([cp.P_ONSITE]))
        _raises(lambda: ctx.set_custom_pair_operators([]))
        assert _unchanged(ctx, before)
        ctx.series_end()
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_correlators(False)
        ctx.series_begin(1, 2, 0, 1)
        ctx.set_custom_pair_operators([cp.P_ONSITE])
        ctx.series_end()
    finally:
        ctx.close()
    ctx = _context(2, 4, 20, 5, band=False, ph=False, weakZflux=True)     # the flux rule: any bond entry, on-site operators stay legal
    try:
        ctx.set_custom_pair_operators([cp.P_ONSITE])
        before = _snapshot(ctx)
        tiny = np.zeros((4, 4), dtype=complex)
        tiny[1, 1] = 1e-300
        for bad in ([cp.P_RAND], [(None, tiny, None)], [cp.P_ONSITE, (cp.P_RAND[0], None, tiny)]):
            with pytest.raises(DqmcError) as e:
                ctx.set_custom_pair_operators(bad)
            assert e.value.code == EINVAL and "weakZflux" in str(e.value)
            assert _unchanged(ctx, before)
        ctx.set_custom_pair_operators([cp.P_S, (cp.P_RAND[0], np.zeros((4, 4)), None)])
    finally:
        ctx.close()
    from detqmc_amd import DetHubbard, HubbardParams
    hub = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        h = hub.lib.dethubbard_ctx(hub.h)
        f = np.ascontiguousarray(cp.P_RAND[0])
        cnt = C.c_int(7)
        assert hub.lib.dqmc_set_custom_pair_operators(h, 1, f.ctypes.data, f.ctypes.data, None) == EINVAL
        assert hub.lib.dqmc_get_custom_pair_operators(h, C.byref(cnt), None, None, None) == EINVAL and cnt.value == 7
        assert hub.lib.dqmc_set_equal_time_custom_pair(h, 1) == EINVAL
    finally:
        hub.close()


# ---- 7. the series parts at the kernel level ---------------------------------------------------------------------------------------
def test_series_parts():
    """parts 2048 and 4096 are refused without operators and accepted with them; a mask without them keeps its S and offsets; the rows hold
    the bin means of C(d), S(q) and the Matsubara transform; series_custom_pair_derived is correlation_ratio on the bins (numpy
    jackknife of tests/series_reference.py, 1e-12)"""
    L, m, s, nfreq = 4, 20, 5, 2
    N = L * L
    ops = [cp.P_RAND, cp.P_ONSITE, cp.P_S]
    ctx = _context(2, L, m, s, band=False, ph=False, every=True)
    try:
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_correlators(False)
        for parts in (2048, 4096, 1 | 4096, 1 | 2048 | 4096):
            _raises(lambda: ctx.series_begin(1, 4, nfreq, parts))
        _raises(lambda: ctx.series_begin(1, 4, nfreq, 1 | 32))            # bit 5 stays unknown
        _raises(lambda: ctx.series_begin(1, 4, nfreq, 1 | 8192))
        ctx.series_begin(1, 4, nfreq, 1)
        plain = (ctx.series_info()[2], ctx.series_layout(0))
        ctx.series_end()
        ctx.set_custom_pair_operators(ops)
        ctx.series_begin(1, 4, nfreq, 1)
        assert (ctx.series_info()[2], ctx.series_layout(0)) == plain
        _raises(lambda: ctx.series_layout(11))
        _raises(lambda: ctx.series_custom_pair_derived())
        ctx.series_end()
        ctx.series_begin(1, 4, nfreq, 1 | 2048 | 4096)
        S = ctx.series_info()[2]
        (o11, l11), (o12, l12) = ctx.series_layout(11), ctx.series_layout(12)
        assert (o11, l11, o12, l12, S) == (plain[0], 3 * nfreq * N * 2, plain[0] + 3 * nfreq * N * 2, 2 * 3 * N, plain[0] + 3 * nfreq * N * 2 + 6 * N)
        _raises(lambda: ctx.series_custom_pair_derived())                 # fewer than two closed bins
        seen = []
        for it in range(3):
            phi = _random_phi(2, N, m, 60 + it)
            _start(ctx, [phi])
            ctx.set_equal_time_correlators(True)

            def at(j):
                ctx.measure_timedisplaced_segment(j)
                _measure_both(ctx, j)

            _walk_down(ctx, at)
            ctx.set_equal_time_correlators(False)
            ctx.advanceDownGreen(1)
            ctx.measure_timedisplaced_ends()
            eq = ctx.measure_eq_custom_pair_read()
            seen.append((eq[1:].reshape(3, N) / (eq[0] * N), ctx.measure_td_matsubara(6, nfreq)[0]))
            ctx.series_add_sweep()
        bins = ctx.series_bins()
        assert bins.shape == (3, S)
        for it in range(3):
            corr, mats = seen[it]
            sr.rows_close(bins[it, o12:o12 + 3 * N].reshape(3, N), corr, 1e-14, N)
            sr.rows_close(bins[it, o12 + 3 * N:o12 + 6 * N].reshape(3, N), sr.structure_factor_ref(corr, L), 1e-12, N)
            assert np.array_equal(bins[it, o11:o11 + l11].view(np.complex128).reshape(3, nfreq, N), mats) and mats.any()
        for Q in ((0, 0), (1, 0), (2, 2)):
            val, err = ctx.series_custom_pair_derived(Q)
            assert val.shape == (1, 3)
            for c in range(3):
                rv, rerr = sr.jackknife(bins[:, o12 + (3 + c) * N:o12 + (4 + c) * N], lambda x: correlation_ratio(x, L, *Q))
                print(f"Q={Q} operator {c}: R = {val[0, c]:.6f} +- {err[0, c]:.2e} (numpy {rv:.6f} +- {rerr:.2e})")
                assert abs(val[0, c] - rv) <= 1e-12 * max(1.0, abs(rv)) and abs(err[0, c] - rerr) <= 1e-10 * rerr
        _raises(lambda: ctx.series_custom_pair_derived((4, 0)))
        _raises(lambda: ctx.series_custom_derived())                      # the series has no part of the bilinears
        ctx.series_end()
    finally:
        ctx.close()


# ---- 8. host level -----------------------------------------------------------------------------------------------------------------
def _batch(sub_batches, every=False, seed=4713, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedEverySlice=every,
                  rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)], sub_batches=sub_batches)


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_level_vectors_and_matsubara(tmp_path, sub_batches):
    """after real measurement sweeps: the chains, G and the random numbers are those of a batch without operators; pair_operator('s')
    gives pairPlusTau / 4 and pairPlusCorr / 4 (1e-13 of the largest entry), Sq is the cosine sum of Corr (1e-12), TauQ0 the row sum;
    matsubara_all('customPair{c}Tau') against the numpy transform of the fine vector (1e-10) and against pairPlusTau's / 4.  Then, with
    the operators removed again, a series file of the one batch has the bytes of the other's: no pair part, no block"""
    import td_matsubara_reference as tm
    from detqmc_amd import pair_operator
    a, b = _batch(sub_batches, every=True), _batch(sub_batches, every=True)
    ops = [pair_operator("s"), cp.P_RAND, pair_operator("d_bond")]
    try:
        a.sweepThermalization(); b.sweepThermalization()
        b.set_custom_pair_operators(ops)
        assert _same_ops(b.get_custom_pair_operators(), ops) and a.get_custom_pair_operators() == []
        a.sweep(True); b.sweep(True)
        mats = [b.matsubara_all(f"customPair{k}Tau", 3) for k in range(3)]
        plus = b.matsubara_all("pairPlusTau", 3)
        assert mats[0].shape == (2, 3, 16)
        for c in range(2):
            ra, rb = a.chain(c), b.chain(c)
            assert np.array_equal(ra.phi, rb.phi) and np.array_equal(ra.g, rb.g) and ra.info.rngDrawn == rb.info.rngDrawn
            n, m = rb.info.n, rb.info.m
            errs = {"Tau": _maxrel(4 * rb.observable_vector("customPair0Tau"), rb.observable_vector("pairPlusTau")),
                    "TauFine": _maxrel(4 * rb.observable_vector("customPair0TauFine"), rb.observable_vector("pairPlusTauFine")),
                    "Corr": _maxrel(4 * rb.observable_vector("customPair0Corr"), rb.observable_vector("pairPlusCorr")),
                    "Sq": _maxrel(4 * rb.observable_vector("customPair0Sq"), rb.observable_vector("pairPlusSq")),
                    "matsubara": _maxrel(4 * mats[0][c], plus[c])}
            print(f"sub-batches {sub_batches} chain {c}: 4 x customPair0 vs pairPlus " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
            assert max(errs.values()) < 1e-13, errs
            for k in range(3):
                tau, q0 = rb.observable_vector(f"customPair{k}Tau"), rb.observable_vector(f"customPair{k}TauQ0")
                fine = rb.observable_vector(f"customPair{k}TauFine")
                cd, sq = rb.observable_vector(f"customPair{k}Corr"), rb.observable_vector(f"customPair{k}Sq")
                assert tau.shape == (n - 1, 16) and q0.shape == (n - 1,) and fine.shape == (m + 1, 16) and cd.shape == (16,)
                assert np.abs(q0 - tau.sum(axis=1)).max() <= 1e-14 * max(1.0, np.abs(tau).max()) and np.abs(cd).max() > 1e-6
                assert all(np.array_equal(fine[j * rb.info.s], tau[j - 1]) for j in range(1, n))
                sr.rows_close(sq, sr.structure_factor_ref(cd, 4), 1e-12, 16)
                ref = tm.bosonic(fine, 4, 0.1, 3)
                e = relerr(mats[k][c], ref)
                print(f"  operator {k}: matsubara vs numpy on the fine vector {e:.1e} (1e-10)")
                assert np.abs(ref).max() > 1e-6 and e <= 1e-10
                assert np.array_equal(rb.matsubara(f"customPair{k}Tau", 3), mats[k][c])
            _raises(lambda: rb.observable_vector("customPair3Tau"))          # not set
            _raises(lambda: ra.observable_vector("customPair0Tau"))
        # no pair part: the file keeps its bytes
        b.set_custom_pair_operators([])
        assert b.get_custom_pair_operators() == []
        files = [str(tmp_path / f) for f in ("a.bin", "b.bin")]
        for batch, path in zip((a, b), files):
            batch.series_begin(1, 4, nfreq=2)
            batch.sweep(True)
            batch.series_save(path)
            batch.series_end()
        assert open(files[0], "rb").read() == open(files[1], "rb").read()
    finally:
        a.close(); b.close()


def test_host_level_options():
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    kw = dict(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    rep = DetSDWBatch([SDWParams(**kw)])                          # neither family the operators could ride on
    try:
        with pytest.raises(DqmcError) as e:
            rep.set_custom_pair_operators([cp.P_S])
        assert e.value.code == EINVAL and "equalTimeCorrelators" in str(e.value)
    finally:
        rep.close()
    rep = DetSDWBatch([SDWParams(equalTimeCorrelators=True, **kw)])   # equal time alone
    try:
        for bad in ([(None, None, None)], [(cp.P_SYM_BOND[0], None, None)], [cp.P_S] * 5):
            with pytest.raises(DqmcError):
                rep.set_custom_pair_operators(bad)
        assert rep.get_custom_pair_operators() == []
        rep.set_custom_pair_operators([cp.P_SYM_BOND])
        rep.sweep(True)
        assert np.abs(rep.chain(0).observable_vector("customPair0Sq")).max() > 1e-6
        with pytest.raises(DqmcError):
            rep.chain(0).observable_vector("customPair0Tau")
        rep.series_begin(1, 4, host_copy=False)                  # a NO_HOST_COPY series refuses the setter, nothing changes
        with pytest.raises(DqmcError) as e:
            rep.set_custom_pair_operators([cp.P_RAND])
        assert e.value.code == EINVAL and "NO_HOST_COPY" in str(e.value)
        assert _same_ops(rep.get_custom_pair_operators(), [cp.P_SYM_BOND])
        rep.series_end()
        rep.set_custom_pair_operators([cp.P_RAND])
    finally:
        rep.close()


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_level_series(tmp_path, sub_batches):
    """a routed series over three sweeps with pair operators beside custom bilinears with a bond part: the bins of the pair parts are the
    vectors / Matsubara transforms of the sweeps in the routed slots, series_stats_all is the numpy jackknife of the bins,
    R_customPair1 at a chosen Q against the numpy jackknife of tests/series_reference.py (1e-12), and the file: the round trip, and the
    refusal of a file written with other pair operators, the series left as it was"""
    import custom_bond_reference as cb
    from detqmc_amd import DqmcError
    ops = [cp.P_SYM_BOND, cp.P_RAND]
    b = _batch(sub_batches, every=True, timeDisplacedParticleHole=True)
    path = str(tmp_path / "pair.bin")
    try:
        b.sweepThermalization()
        b.set_custom_bond_bilinears([cb.B_RAND])                  # the bilinears' bond block precedes the pair block in the file
        b.set_custom_pair_operators(ops)
        assert _same_ops(b.get_custom_bond_bilinears(), [cb.B_RAND]) and _same_ops(b.get_custom_pair_operators(), ops)
        b.series_begin(1, 4, nfreq=2)
        b.series_route([1, 0])
        seen = []
        for it in range(3):
            b.sweep(True)
            seen.append([(b.chain(c).observable_vector("customPair1Corr"), b.chain(c).observable_vector("customPair1Sq"),
                          b.chain(c).matsubara("customPair1Tau", 2), b.chain(c).observable_vector("custom0Corr")) for c in range(2)])
        for c in range(2):
            slot = b.chain(1 - c)                                 # chain c fed slot 1 - c
            corr, sq, mats = slot.series_bins("customPair1Corr"), slot.series_bins("customPair1Sq"), slot.series_bins("customPair1Tau")
            assert corr.shape == (3, 16) and mats.shape == (3, 2, 16)
            for it in range(3):
                sr.rows_close(corr[it], seen[it][c][0], 1e-14, 16)
                sr.rows_close(sq[it], seen[it][c][1], 1e-12, 16)
                assert np.array_equal(mats[it], seen[it][c][2]) and mats[it].any()
                sr.rows_close(slot.series_bins("custom0Corr")[it], seen[it][c][3], 1e-14, 16)
        mean, err = b.series_stats_all("customPair0Sq")
        assert mean.shape == (2, 16)
        for c in range(2):
            rm, re_ = sr.jackknife(b.chain(c).series_bins("customPair0Sq"))
            assert np.abs(mean[c] - rm).max() <= 1e-13 * np.abs(rm).max() and np.abs(err[c] - re_).max() <= 1e-10 * np.abs(re_).max()
        val, verr = b.series_derived_all("R_customPair1", Q=(1, 0))
        for c in range(2):
            bins = b.chain(c).series_bins("customPair1Sq")
            rv, rerr = sr.jackknife(bins, lambda x: correlation_ratio(x, 4, 1, 0))
            print(f"slot {c}: R_customPair1(1, 0) = {val[c]:.6f} +- {verr[c]:.2e} (numpy {rv:.6f} +- {rerr:.2e})")
            assert abs(val[c] - rv) <= 1e-12 * max(1.0, abs(rv)) and abs(verr[c] - rerr) <= 1e-10 * rerr
        _raises(lambda: b.series_derived_all("R_customPair2"))    # not set
        with pytest.raises(DqmcError):
            b.set_custom_pair_operators([cp.P_S])                 # the open series holds their parts
        b.series_save(path)
        kept = [b.chain(c).series_bins("customPair1Corr") for c in range(2)]
        b.series_end()
        b.series_begin(1, 4, nfreq=2)
        b.series_load(path)                                       # the round trip
        assert b.series_route() == [1, 0]
        assert all(np.array_equal(b.chain(c).series_bins("customPair1Corr"), kept[c]) for c in range(2))
        b.series_end()
        for wrong in ([cp.P_SYM_BOND, (cp.P_RAND[0], 2.0 * cp.P_RAND[1], cp.P_RAND[2])], [cp.P_RAND, cp.P_SYM_BOND]):
            b.set_custom_pair_operators(wrong)
            b.series_begin(1, 4, nfreq=2)
            b.sweep(True)
            state = [b.chain(c).series_bins("customPair1Corr") for c in range(2)]
            with pytest.raises(DqmcError) as e:
                b.series_load(path)
            assert e.value.code == EINVAL and "pair operators" in str(e.value)
            assert all(np.array_equal(b.chain(c).series_bins("customPair1Corr"), state[c]) for c in range(2))     # the series is as it was
            b.series_end()
        b.set_custom_pair_operators(ops[:1])                      # another count: another sample length, refused as well
        b.series_begin(1, 4, nfreq=2)
        with pytest.raises(DqmcError):
            b.series_load(path)
        b.series_end()
    finally:
        b.close()
