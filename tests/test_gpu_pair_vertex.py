"""The averaged Green's function block, its series part and the bubble / vertex kernels on the device (kernel level): the block against
numpy on the device's own matrices (tests/pair_vertex_reference.py), coarse against fine, reproducibility and batching, neutrality of the
switch, the refusals, the series part, the derived kernels on injected bins against the numpy jackknife, and the exact limit of a free
matrix, where the bubble is the pair correlator itself and Gamma Pbar vanishes.

Tolerances: 1e-10 for a kernel against numpy on the device's own matrices and the bounds of tests/test_gpu_td_fine.py for rows against
direct inverses (the bounds of channel 6); bit equality wherever a text says so; for the derived kernels 100 x the float64-vs-longdouble
figure of the reference (tests/test_pair_vertex_cpu.py), floor 1e-12.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_pair_reference as cp
import pair_vertex_reference as pv
import td_fine_reference as tf
from conftest import relerr
from test_gpu_band_correlators import EINVAL, _context, _raises, _start
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu

CASES = [(1, 4, 20, "pbc"), (2, 4, 20, "apbc-x"), (2, 4, 20, "apbc-xy"), (3, 4, 20, "apbc-xy"), (2, 6, 10, "apbc-xy"), (3, 6, 10, "pbc")]


def _R(opdim):
    return 4 if opdim == 3 else 2


def _rows(acc, nrows, N, R):
    """(counts [nrows], raw sums [nrows][N][R][R] complex) of a block"""
    return acc[:nrows], acc[nrows:].view(np.complex128).reshape(nrows, N, R, R)


def _full_pass(ctx, coarse=True):
    """a down pass: every boundary (coarse call and segment), then the ends"""
    def at(j):
        if coarse:
            ctx.measure_timedisplaced_green_matrix(j)
        ctx.measure_timedisplaced_segment(j)

    _walk_down(ctx, at)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


# ---- (a) the block -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,bc", CASES)
def test_block_vs_numpy_coarse_and_fine(opdim, L, m, bc):
    """coarse and fine rows against numpy on the device's own shifted G(tau,0) (1e-10) and against direct inverses of the oracle's chain:
    rows 0 and m from G(0) alone (1e-10), an interior row within 10 e_ref; row j s of the fine block is coarse row j bit for bit"""
    from td_reference import Chain, make_oracle, shift_symmetric
    s, N, R = 5, L * L, _R(opdim)
    phi = _random_phi(opdim, N, m, 71 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, delaySteps=4)
    chain = Chain(ora)
    ctx = _context(opdim, L, m, s, band=False, ph=False, every=True, bc=bc)

    def ref_of(gt0):
        return pv.bin_green(shift_symmetric(ora, gt0), L, bc)

    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == 0 and ctx.lib.dqmc_measure_td_green_matrix_accum_size(ctx.h) == 0
        ctx.set_green_matrix(True)
        row = 2 * R * R * N
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == (m + 1) * (1 + row)
        assert ctx.lib.dqmc_measure_td_green_matrix_accum_size(ctx.h) == (n - 1) * (1 + row)
        assert ctx.lib.dqmc_measure_td_matsubara_size(ctx.h, 7, 1) == 0
        _start(ctx, [phi])
        kin = s + 2 if m > 2 * s else s - 2
        dev = {}

        def at(j):
            if j == 1:
                ctx.td_fine_propagate(1, kin)
                dev[kin] = ref_of(ctx.green_td_fine()[1])
            dev[("c", j)] = ref_of(ctx.green_timedisplaced()[1])
            ctx.measure_timedisplaced_green_matrix(j)
            ctx.measure_timedisplaced_segment(j)

        _walk_down(ctx, at)
        ctx.advanceDownGreen(1)
        g, one = ctx.g, np.eye(ctx.ng)
        dev[0], dev[m] = ref_of(g), ref_of(one - g)
        ctx.measure_timedisplaced_ends()
        cnt, rows = _rows(ctx.measure_td_fine_read(7), m + 1, N, R)
        ccnt, crow = _rows(ctx.measure_td_green_matrix_read(), n - 1, N, R)
        assert np.array_equal(cnt, np.ones(m + 1)) and np.array_equal(ccnt, np.ones(n - 1))
        for j in range(1, n):
            e = relerr(crow[j - 1], dev[("c", j)])
            assert np.array_equal(rows[j * s], crow[j - 1]) and e < 1e-10, (j, e)
        gd = chain.greens(m)[0]
        direct = {0: ref_of(gd), m: ref_of(one - gd), kin: ref_of(chain.greens(kin)[1])}
        e_ref = tf.e_ref()
        for k in (0, kin, m):
            e_dev, e_dir = relerr(rows[k], dev[k]), relerr(rows[k], direct[k])
            bound = 10 * e_ref if k == kin else 1e-10
            print(f"O({opdim}) L={L} m={m} {bc} row {k}: vs numpy on device matrices {e_dev:.2e} (1e-10), vs direct inverses {e_dir:.2e} ({bound:.2e}); "
                  f"max |Gbar| {np.abs(dev[k]).max():.3f}")
            assert np.abs(dev[k]).max() > 1e-3 and e_dev < 1e-10 and e_dir < bound, (k, e_dev, e_dir)
        _raises(lambda: ctx.measure_td_matsubara(7, 1))
        ctx.measure_reset()
        assert not ctx.measure_td_fine_read(7).any() and not ctx.measure_td_green_matrix_read().any()
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim", [2, 3])
def test_block_reproducibility_and_batching(opdim):
    """two identical passes give bit-identical blocks; two chains in one context equal two single-chain contexts (N = 36: a second,
    partly filled block of bins)"""
    L, m, s = 6, 10, 5
    phis = [_random_phi(opdim, L * L, m, 5 + opdim + 100 * c) for c in range(2)]

    def run(phis, passes):
        ctx = _context(opdim, L, m, s, band=False, ph=False, every=True, bc="apbc-xy", nchains=len(phis))
        out = []
        try:
            ctx.set_green_matrix(True)
            for _ in range(passes):
                _start(ctx, phis)
                _full_pass(ctx)
                per = []
                for b in range(len(phis)):
                    ctx.select_chain(b)
                    per.append((ctx.measure_td_green_matrix_read(), ctx.measure_td_fine_read(7)))
                ctx.select_chain(0)
                out.append(per)
        finally:
            ctx.close()
        return out

    first, second = run(phis, 2)
    singles = [run([phi], 1)[0][0] for phi in phis]
    for b in range(2):
        for k in range(2):
            assert first[b][k].any() and np.array_equal(first[b][k], second[b][k]) and np.array_equal(first[b][k], singles[b][k])
    assert not np.array_equal(singles[0][1], singles[1][1])


# ---- (b) neutrality ----------------------------------------------------------------------------------------------------------------
def test_switch_leaves_everything_else_alone():
    """with the switch off channel 7 has no block; every other block, G and the launch count of a full measurement pass equal those of
    the same context with the switch on, bit for bit, apart from the launches of the new kernel itself (one per row)"""
    L, m, s = 4, 20, 5
    phi = _random_phi(2, L * L, m, 5)
    ops = cp.pair_ops()
    results = []
    for on in (False, True):
        ctx = _context(2, L, m, s, td=2, every=True)
        try:
            ctx.set_custom_pair_operators(ops)
            if on:
                ctx.set_green_matrix(True)
            assert (ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) != 0) == on
            _start(ctx, [phi])
            ctx.set_equal_time_correlators(True)
            ctx.profile_enable(True)

            def at(j):
                for f in (ctx.measure_timedisplaced, ctx.measure_timedisplaced_pair, ctx.measure_timedisplaced_ph, ctx.measure_timedisplaced_band,
                          ctx.measure_timedisplaced_custom_pair, ctx.measure_timedisplaced_segment):
                    f(j)
                ctx.measure_slice()

            _walk_down(ctx, at)
            ctx.advanceDownGreen(1)
            ctx.measure_timedisplaced_ends()
            pr = ctx.profile_read()
            launches = [pr[nm][1] for nm in ("bmult", "gemm", "decomp", "decide", "other", "gather", "flush")]
            blocks = [ctx._read_block(ctx.lib.dqmc_measure_accum_size, ctx.lib.dqmc_measure_read_host), ctx.measure_td_pair_read(), ctx.measure_td_ph_read(),
                      ctx.measure_td_band_read(), ctx.measure_td_custom_pair_read(), ctx.measure_eq_read()]
            blocks += [ctx.measure_td_fine_read(ch) for ch in (0, 1, 2, 4, 6)]
            results.append((blocks, ctx.g, launches))
            if on:
                ctx.set_green_matrix(False)
                assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == 0 and ctx.lib.dqmc_measure_td_green_matrix_accum_size(ctx.h) == 0
                _raises(lambda: ctx.measure_td_green_matrix_read())
        finally:
            ctx.close()
    (off_blocks, g0, l0), (on_blocks, g1, l1) = results
    assert np.array_equal(g0, g1) and all(np.array_equal(x, y) and x.any() for x, y in zip(off_blocks, on_blocks))
    extra = [b - a for a, b in zip(l0, l1)]
    print(f"launches per family off {l0}, on {l1}")
    assert sum(extra) == m + 1 and sorted(extra)[-1] == m + 1            # the fine rows; the coarse call was not made


# ---- (c) refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    from detqmc_amd import DetHubbard, HubbardParams, KernelContext
    L, m, s = 4, 20, 5
    N = L * L
    hub = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        assert hub.lib.dqmc_set_green_matrix(hub.lib.dethubbard_ctx(hub.h), 1) == EINVAL
    finally:
        hub.close()
    ctx = _context(2, L, m, s, band=False, ph=False, every=True, weakZflux=True)
    try:
        _raises(lambda: ctx.set_green_matrix(True))
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == 0
    finally:
        ctx.close()
    ctx = KernelContext(2, L, m, s, 0.1, delaySteps=4, stabilisation="qr")           # no timedisplaced
    try:
        _raises(lambda: ctx.set_green_matrix(True))
    finally:
        ctx.close()
    ctx = _context(2, L, m, s, band=False, ph=False, every=True)
    try:
        ctx.set_custom_pair_operators([cp.P_RAND])
        _raises(lambda: ctx.series_begin(1, 4, 2, 2048 | 8192))          # bit 13 without the switch
        _raises(lambda: ctx.measure_timedisplaced_green_matrix(1))
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 4, 2, 8192)                                  # the part alone is a series; the vertex needs bit 11 as well
        v = np.full(5 + m, 7.0)
        dp = v.ctypes.data_as(C.POINTER(C.c_double))
        assert ctx.lib.dqmc_series_pair_vertex_size(ctx.h) == 0
        assert ctx.lib.dqmc_series_pair_vertex_host(ctx.h, 0, 0, dp, dp) == EINVAL and np.all(v == 7.0)
        _raises(lambda: ctx.set_green_matrix(False))                     # switch-off under an open part
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 7) == (m + 1) * (1 + 8 * N)
        ctx.series_end()
        ctx.series_begin(1, 4, 2, 2048 | 8192)
        assert ctx.lib.dqmc_series_pair_vertex_size(ctx.h) == 5 + m
        phi = _random_phi(2, N, m, 9)
        _start(ctx, [phi])
        _full_pass(ctx, coarse=False)
        ctx.series_add_sweep()
        assert ctx.lib.dqmc_series_pair_vertex_host(ctx.h, 0, 0, dp, dp) == EINVAL and np.all(v == 7.0)      # B < 2
        ctx.series_add_sweep()
        for Q in ((L, 0), (0, L), (-1, 0), (0, -1)):
            assert ctx.lib.dqmc_series_pair_vertex_host(ctx.h, Q[0], Q[1], dp, dp) == EINVAL and np.all(v == 7.0)
        val, err = ctx.series_pair_vertex((0, 0))
        assert val.shape == (1, 1, 5 + m) and np.all(np.isfinite(val)) and np.all(err == 0.0)      # two identical bins
        ctx.series_end()
        ctx.set_green_matrix(False)
    finally:
        ctx.close()


# ---- (d) the series part -----------------------------------------------------------------------------------------------------------
def test_series_part():
    """a mask without bit 13 keeps S and its offsets; the rows of part 13 are the bin means of the normalised block; re-binning and the
    export / import round trip treat the part like every other"""
    L, m, s, nfreq = 4, 20, 5, 2
    N, R = L * L, 2
    ctx = _context(2, L, m, s, band=False, ph=False, every=True, bc="apbc-x")
    try:
        ctx.set_custom_pair_operators([cp.P_RAND, cp.P_ONSITE])
        ctx.series_begin(1, 4, nfreq, 2048)
        plain = (ctx.series_info()[2], ctx.series_layout(11))
        ctx.series_end()
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 4, nfreq, 2048)
        assert (ctx.series_info()[2], ctx.series_layout(11)) == plain
        _raises(lambda: ctx.series_layout(13))
        ctx.series_end()
        ctx.series_begin(1, 8, nfreq, 2048 | 8192)
        S = ctx.series_info()[2]
        row = (m + 1) * 2 * R * R * N
        assert ctx.series_layout(11) == plain[1] and ctx.series_layout(13) == (plain[0], row) and S == plain[0] + row
        ctx.series_configure(track_variance=True)
        seen = []
        for it in range(4):
            _start(ctx, [_random_phi(2, N, m, 60 + it)])
            _full_pass(ctx, coarse=False)
            cnt, rows = _rows(ctx.measure_td_fine_read(7), m + 1, N, R)
            seen.append(rows / (N * cnt[:, None, None, None]))
            ctx.series_add_sweep()
        bins = ctx.series_bins()
        o13 = plain[0]
        for it in range(4):
            assert np.array_equal(bins[it, o13:].view(np.complex128).reshape(m + 1, N, R, R), seen[it])
        mean, err = ctx.series_stats()
        ref = np.array(seen).mean(axis=0).reshape(-1).view(np.float64)
        e = np.abs(mean[0, o13:] - ref).max() / np.abs(ref).max()
        print(f"series mean of part 13 vs numpy: {e:.2e}")
        assert e < 1e-14 and np.all(err[0, o13:] > 0)
        st, data = ctx.series_export()
        assert st.parts == (2048 | 8192) and st.sample_len == S
        ctx.series_rebin()
        merged = ctx.series_bins()
        assert merged.shape == (2, S) and np.array_equal(merged[0, o13:], (bins[0, o13:] + bins[1, o13:]) * 0.5)
        ctx.series_end()
        ctx.series_begin(1, 8, nfreq, 2048 | 8192)
        ctx.series_import(st, data)
        assert np.array_equal(ctx.series_bins(), bins) and np.array_equal(ctx.series_export()[1], data)
        ctx.series_end()
    finally:
        ctx.close()


# ---- (e) the derived kernels on injected bins --------------------------------------------------------------------------------------
def _import_bins(ctx, gb, cb, nchains=1):
    """closed bins from CPU-generated parts 11 and 13, the same for every slot; returns the packed bins [B][S]"""
    B = gb.shape[0]
    st = ctx.series_state()
    S = st.sample_len
    (o11, l11), (o13, l13) = ctx.series_layout(11), ctx.series_layout(13)
    packed = np.zeros((B, S))
    packed[:, o11:o11 + l11] = np.ascontiguousarray(cb).reshape(B, -1).view(np.float64)
    packed[:, o13:o13 + l13] = np.ascontiguousarray(gb).reshape(B, -1).view(np.float64)
    data = np.concatenate([np.repeat(packed[:, None, :], nchains, axis=1).reshape(-1), np.zeros(nchains * S)])
    st.bins_closed, st.sweeps_in_open_bin, st.samples = B, 0, B
    ctx.series_import(st, data)
    return packed


@pytest.mark.parametrize("opdim,L,m,bc", pv.VERTEX_CASES)
def test_derived_kernels_on_injected_bins(opdim, L, m, bc):
    """B = 6 CPU-generated bins (a translation-covariant mean plus 1 % noise) through series_import: value and err of all outputs at
    Q = (0,0) and (1,2) against the numpy jackknife of tests/pair_vertex_reference.py, values against max |value| and errors against max err;
    bound 100 x the float64-vs-longdouble figure of the reference, floor 1e-12.  Two calls give identical bits, and three slots in one
    context give the single-slot bits"""
    s = 5
    ops = pv.vertex_ops()
    gb, cb = pv.vertex_bins(L, m, _R(opdim), len(ops))
    got = {}
    for nchains in (1, 3):
        ctx = _context(opdim, L, m, s, band=False, ph=False, every=True, bc=bc, nchains=nchains)
        try:
            ctx.set_custom_pair_operators(ops)
            ctx.set_green_matrix(True)
            ctx.series_begin(1, 8, pv.VERTEX_NFREQ, 2048 | 8192)
            _import_bins(ctx, gb, cb, nchains)
            for Q in pv.VERTEX_QS:
                v, e = ctx.series_pair_vertex(Q)
                v2, e2 = ctx.series_pair_vertex(Q)
                assert np.array_equal(v, v2) and np.array_equal(e, e2) and v.shape == (nchains, len(ops), 5 + m)
                got[(nchains, Q)] = (v, e)
            ctx.series_end()
        finally:
            ctx.close()
    bound = pv.gpu_bound()
    for Q in pv.VERTEX_QS:
        v, e = got[(1, Q)]
        for b in range(3):
            assert np.array_equal(got[(3, Q)][0][b], v[0]) and np.array_equal(got[(3, Q)][1][b], e[0])
        rv, re_ = pv.jackknife_outputs(gb, cb[:, :, 0, Q[1] * L + Q[0]].real, ops, L, bc, 0.1, Q)
        dv, de = np.abs(v[0] - rv).max() / np.abs(rv).max(), np.abs(e[0] - re_).max() / np.abs(re_).max()
        print(f"O({opdim}) L={L} {bc} Q={Q}: values {dv:.2e} of max |value| {np.abs(rv).max():.3e}, errors {de:.2e} of max err {re_.max():.3e} (bound {bound:.1e})")
        assert np.all(re_[:, 1:] > 0) and dv < bound and de < bound


def test_vertex_nan_for_a_vanishing_denominator():
    """P = 0 in every bin: Gamma and Gamma Pbar are NaN, P and Pbar are not"""
    L, m, s = 4, 20, 5
    ops = [cp.P_ONSITE]
    gb, cb = pv.vertex_bins(L, m, 2, 1, seed=3)
    cb[...] = 0.0
    ctx = _context(2, L, m, s, band=False, ph=False, every=True)
    try:
        ctx.set_custom_pair_operators(ops)
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 8, pv.VERTEX_NFREQ, 2048 | 8192)
        _import_bins(ctx, gb, cb)
        v, e = ctx.series_pair_vertex((0, 0))
        assert v[0, 0, 0] == 0.0 and np.isfinite(v[0, 0, 1]) and v[0, 0, 1] != 0.0 and np.all(np.isnan(v[0, 0, 2:4])) and np.all(np.isnan(e[0, 0, 2:4]))
        assert np.all(np.isfinite(v[0, 0, 4:])) and np.all(e[0, 0, 4:] > 0)
        ctx.series_end()
    finally:
        ctx.close()


# ---- (f) the exact limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,bc", [(1, 4, 20, "pbc"), (2, 4, 20, "apbc-x"), (2, 4, 20, "apbc-xy"), (3, 4, 20, "apbc-xy"), (2, 6, 10, "apbc-xy"),
                                          (3, 6, 10, "pbc")])
@pytest.mark.parametrize("which", ["ops", "d_bond"])
def test_exact_limit_of_the_free_matrix(opdim, L, m, bc, which):
    """P-bar(d, tau_k) per d and its cosine sums: a free, translation-invariant matrix on the device (the field 1e-150: phi = 0 itself divides 0 / 0 in the field terms, as in the
    reference; the dense propagator: the checkerboard break-up is invariant under even translations only), no updates, all rows measured twice into two bins: <G> is G, so the bubble Pbar_c(Q, tau_k) equals the cosine sum of the
    channel-6 row / (N count), and Gamma Pbar_c = Pbar_c / P_c - 1 = 0, for every operator; within the bound of the derived-kernel test,
    relative to the largest |Pbar_c(Q, tau_k)| resp. to 1.  Fails for a wrong sign, sector or stencil"""
    from detqmc_amd import pair_bubble, pair_operator
    s, N = 5, L * L
    ops = cp.pair_ops() if which == "ops" else [pair_operator("d_bond"), cp.P_RAND, cp.P_SYM_BOND]
    phi = np.full((m + 1, N, opdim), pv.FREE_PHI)
    phi[0] = 0.0
    ctx = _context(opdim, L, m, s, band=False, ph=False, every=True, bc=bc, checkerboard=False)
    bound = pv.gpu_bound()
    try:
        ctx.set_custom_pair_operators(ops)
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 4, 1, 2048 | 8192)
        for _ in range(2):
            _start(ctx, [phi])
            _full_pass(ctx, coarse=False)
            ctx.series_add_sweep()
        fine = ctx.measure_td_fine_read(6)
        cnt, rows = fine[:m + 1], fine[m + 1:].reshape(m + 1, len(ops), N)
        assert np.array_equal(cnt, np.ones(m + 1))
        # per d: the bubble of the device's own part-13 bin (the numpy twin of the bubble kernel) against the channel-6 row / (N count)
        o13, l13 = ctx.series_layout(13)
        gbar = ctx.series_bins()[0, o13:o13 + l13].view(np.complex128).reshape(m + 1, N, _R(opdim), _R(opdim))
        per_d = pair_bubble(gbar, ops, L, bc)                             # [m+1, count, N]
        e_d = np.abs(per_d - rows / N).max(axis=(0, 2)) / np.abs(rows / N).max(axis=(0, 2))
        print(f"O({opdim}) L={L} {bc} {which}: Pbar(d, tau) of the part-13 bin vs channel 6, per d: {['%.1e' % x for x in e_d]} (bound {bound:.1e})")
        assert e_d.max() < bound
        for Q in ((0, 0), (1, 2)):
            val, err = ctx.series_pair_vertex(Q)
            ref = np.einsum("kcd,d->ck", rows / N, pv.cos_table(L, Q))
            e_row = np.abs(val[0, :, 4:] - ref).max(axis=1) / np.abs(ref).max(axis=1)
            e_gp = np.abs(val[0, :, 3])
            print(f"O({opdim}) L={L} {bc} {which} Q={Q}: Pbar(Q, tau) vs channel 6 {['%.1e' % x for x in e_row]}, |Gamma Pbar| {['%.1e' % x for x in e_gp]}, "
                  f"max |Pbar(Q, tau)| {['%.3f' % x for x in np.abs(ref).max(axis=1)]} (bound {bound:.1e})")
            assert np.abs(ref).max(axis=1).min() > 1e-6 and e_row.max() < bound and e_gp.max() < bound
            assert np.all(err == 0.0)                                    # two identical bins
        ctx.series_end()
    finally:
        ctx.close()
