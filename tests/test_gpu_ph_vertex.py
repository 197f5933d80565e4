"""The particle-hole bubble and vertex of the user-defined bilinears on the device (kernel level): the derived kernels on injected bins
against the package's numpy route (detqmc_amd.ph_bubble, ph_one_body, jackknife), reproducibility and batching, the exact limit of a free
matrix -- where the bubble is the connected part of channel 5 itself and Gamma chibar vanishes --, NaN on a vanishing denominator, the
refusals and the neutrality of the call.

Tolerances: for the derived kernels 100 x the float64-vs-longdouble figure of the reference (tests/test_ph_vertex_cpu.py); 1e-11 of the
largest entry for the exact limit; bit equality wherever a text says so.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_bond_reference as cb
import pair_vertex_reference as pv
import ph_bubble_reference as ph
from custom_reference import M_NX, M_RAND, M_SX_BANDX
from test_gpu_band_correlators import EINVAL, _context, _raises, _start
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu

PARTS = 512 | 8192                                          # DQMC_SERIES_MATS_CUSTOM | DQMC_SERIES_GREEN_MATRIX


def _R(opdim):
    return 4 if opdim == 3 else 2


def _full_pass(ctx):
    """a down pass: every segment, then the ends"""
    _walk_down(ctx, ctx.measure_timedisplaced_segment)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


def _import_bins(ctx, gb, chb, nchains=1):
    """closed bins from CPU-generated parts 9 and 13, the same for every slot"""
    B = gb.shape[0]
    st = ctx.series_state()
    S = st.sample_len
    (o9, l9), (o13, l13) = ctx.series_layout(9), ctx.series_layout(13)
    packed = np.zeros((B, S))
    packed[:, o9:o9 + l9] = np.ascontiguousarray(chb).reshape(B, -1).view(np.float64)
    packed[:, o13:o13 + l13] = np.ascontiguousarray(gb).reshape(B, -1).view(np.float64)
    data = np.concatenate([np.repeat(packed[:, None, :], nchains, axis=1).reshape(-1), np.zeros(nchains * S)])
    st.bins_closed, st.sweeps_in_open_bin, st.samples = B, 0, B
    ctx.series_import(st, data)
    return packed


# ---- (a) the derived kernels on injected bins --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bond", "onsite"])
@pytest.mark.parametrize("opdim,L,m,bc", ph.VERTEX_CASES)
def test_derived_kernels_on_injected_bins(opdim, L, m, bc, which):
    """B = 5 CPU-generated bins through series_import: value and err of all 6 + m outputs at Q = (0,0), (2,2) and (1,2) against ph_bubble /
    ph_one_body with detqmc_amd.jackknife, values against max |value| and errors against max err; bound 100 x the float64-vs-longdouble
    figure of the reference.  Two calls give identical bits, and three slots in one context give the single-slot bits.  'bond': the four
    operators, with the measurement kernels' table; 'onsite': the two on-site ones alone, with the table the first call builds"""
    s = 3
    sel = slice(0, 4) if which == "bond" else slice(2, 4)
    ops = ph.vertex_ops()[sel]
    gb, chb = ph.vertex_bins(L, m, _R(opdim), bc)
    chb = chb[:, sel]
    got = {}
    for nchains in (1, 3):
        ctx = _context(opdim, L, m, s, band=False, every=True, bc=bc, nchains=nchains)
        try:
            ctx.set_custom_bond_bilinears(ops)
            ctx.set_green_matrix(True)
            ctx.series_begin(1, 8, ph.VERTEX_NFREQ, PARTS)
            assert ctx.lib.dqmc_series_ph_vertex_size(ctx.h) == nchains * len(ops) * (6 + m)
            _import_bins(ctx, gb, chb, nchains)
            for Q in ph.VERTEX_QS:
                v, e = ctx.series_ph_vertex(Q)
                v2, e2 = ctx.series_ph_vertex(Q)
                assert np.array_equal(v, v2) and np.array_equal(e, e2) and v.shape == (nchains, len(ops), 6 + m)
                got[(nchains, Q)] = (v, e)
            ctx.series_end()
        finally:
            ctx.close()
    bound = ph.gpu_bound()
    for Q in ph.VERTEX_QS:
        v, e = got[(1, Q)]
        for b in range(3):
            assert np.array_equal(got[(3, Q)][0][b], v[0]) and np.array_equal(got[(3, Q)][1][b], e[0])
        rv, re_ = ph.twin_jackknife(gb, chb[:, :, 0, Q[1] * L + Q[0]].real, ops, L, bc, ph.VERTEX_DTAU, Q)
        dv, de = np.abs(v[0] - rv).max() / np.abs(rv).max(), np.abs(e[0] - re_).max() / np.abs(re_).max()
        print(f"O({opdim}) L={L} {bc} {which} Q={Q}: values {dv:.2e} of max |value| {np.abs(rv).max():.3e}, errors {de:.2e} of max err {re_.max():.3e} "
              f"(bound {bound:.1e})")
        assert np.all(re_[:, :4] > 0) and dv < bound and de < bound


def test_vertex_nan_for_a_vanishing_denominator():
    """chi = 0 in every bin (part 9 zero, Q != 0 so that D = 0): Gamma and Gamma chibar are NaN, chi, chibar, D and the rows are not"""
    L, m, s = 4, ph.VERTEX_M, 3
    ops = ph.vertex_ops()[2:3]
    gb, chb = ph.vertex_bins(L, m, 2, "pbc")
    chb = 0.0 * chb[:, 2:3]
    ctx = _context(2, L, m, s, band=False, every=True)
    try:
        ctx.set_custom_bond_bilinears(ops)
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 8, ph.VERTEX_NFREQ, PARTS)
        _import_bins(ctx, gb, chb)
        v, e = ctx.series_ph_vertex((1, 2))
        assert v[0, 0, 0] == 0.0 and np.isfinite(v[0, 0, 1]) and v[0, 0, 1] != 0.0 and np.all(np.isnan(v[0, 0, 2:4])) and np.all(np.isnan(e[0, 0, 2:4]))
        assert v[0, 0, 4] == 0.0 and np.all(np.isfinite(v[0, 0, 5:])) and np.all(e[0, 0, 5:] > 0)
        ctx.series_end()
    finally:
        ctx.close()


# ---- (b) the exact limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,bc", [(1, 4, 10, "pbc"), (2, 4, 10, "apbc-x"), (2, 4, 10, "apbc-xy"), (3, 4, 10, "apbc-xy"), (2, 6, 10, "apbc-xy"),
                                          (3, 6, 10, "pbc")])
@pytest.mark.parametrize("which", ["bond", "onsite"])
def test_exact_limit_of_the_free_matrix(opdim, L, m, bc, which):
    """a free, translation-invariant matrix on the device (field 1e-150, dense propagator), no updates, all rows measured twice into two
    bins: <G> is G, so chibar_c(d, tau_k) equals the channel-5 row / (N count) minus Re(obar obar) per d -- the device's own G(0,tau)
    against -G(tau_{m-k},0): a wrong sign or index of the relation fails here --, chibar_c(Q, tau_k) equals its cosine sums, and
    chi_c = chibar_c at Q = 0, where D is subtracted, and at Q = (L/2, L/2).  Every deviation relative to the largest entry, bound 1e-11"""
    from detqmc_amd import ph_bubble, ph_one_body
    s, N = 5, L * L
    ops = ph.vertex_ops() if which == "bond" else [(M_RAND, None, None), (M_SX_BANDX, None, None), (M_NX, None, None)]
    phi = np.full((m + 1, N, opdim), ph.FREE_PHI)
    phi[0] = 0.0
    ctx = _context(opdim, L, m, s, band=False, every=True, bc=bc, checkerboard=False)
    bound = 1e-11
    try:
        if which == "bond":
            ctx.set_custom_bond_bilinears(ops)
        else:
            ctx.set_custom_bilinears([op[0] for op in ops])
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 4, 1, PARTS)
        for _ in range(2):
            _start(ctx, [phi])
            _full_pass(ctx)
            ctx.series_add_sweep()
        fine = ctx.measure_td_fine_read(5)
        cnt, rows = fine[:m + 1], fine[m + 1:].reshape(m + 1, len(ops), N) / N
        assert np.array_equal(cnt, np.ones(m + 1))
        o13, l13 = ctx.series_layout(13)
        gbar = ctx.series_bins()[0, o13:o13 + l13].view(np.complex128).reshape(m + 1, N, _R(opdim), _R(opdim))
        obar = ph_one_body(gbar[0], ops, L, bc)
        conn = rows - (obar * obar).real[None, :, None]     # the connected part of channel 5 per site pair
        per_d = ph_bubble(gbar, ops, L, bc)                 # [m+1, count, N]
        top = np.maximum(np.abs(rows).max(axis=(0, 2)), np.abs(conn).max(axis=(0, 2)))
        e_d = np.abs(per_d - conn).max(axis=(0, 2)) / top
        print(f"O({opdim}) L={L} {bc} {which}: chibar(d, tau) of the part-13 bin vs channel 5 - Re(o o), per operator: {['%.1e' % x for x in e_d]}; "
              f"largest entry {['%.3f' % x for x in top]}, max |connected| {['%.3f' % x for x in np.abs(conn).max(axis=(0, 2))]} (bound {bound:.0e})")
        assert np.abs(conn).max(axis=(0, 2)).min() > 1e-6 and e_d.max() < bound
        for Q in ((0, 0), (L // 2, L // 2), (1, 2)):
            val, err = ctx.series_ph_vertex(Q)
            cq = pv.cos_table(L, Q)
            ref = np.einsum("kcd,d->ck", conn, cq)
            raw = np.einsum("kcd,d->ck", rows, cq)
            big = np.maximum(np.abs(ref).max(axis=1), np.abs(raw).max(axis=1))
            e_row = np.abs(val[0, :, 5:] - ref).max(axis=1) / big
            chi, chibar, D = val[0, :, 0], val[0, :, 1], val[0, :, 4]
            scale = np.maximum(np.maximum(np.abs(chi + D), np.abs(D)), np.abs(chibar))
            e_chi = np.abs(chibar - chi) / scale                                  # |Gamma chibar| |chi| / the largest entry
            d_ref = m * 0.1 * (obar * obar).real * (N if Q == (0, 0) else 0)
            e_D = np.abs(D - d_ref) / np.maximum(np.abs(d_ref).max(), 1.0)
            print(f"O({opdim}) L={L} {bc} {which} Q={Q}: chibar(Q, tau) vs channel 5 {['%.1e' % x for x in e_row]}, |chibar - chi| / largest "
                  f"{['%.1e' % x for x in e_chi]}, |Gamma chibar| {['%.1e' % x for x in np.abs(val[0, :, 3])]}, chi {['%.4f' % x for x in chi]}, "
                  f"D {['%.3f' % x for x in D]} ({['%.1e' % x for x in e_D]}) (bound {bound:.0e})")
            assert e_row.max() < bound and e_D.max() < bound
            if Q != (1, 2):
                assert e_chi.max() < bound
                well = np.abs(chi) > 1e-3 * scale                                 # Gamma chibar itself where chi is not a rounding residue
                assert well.any() and np.abs(val[0, well, 3]).max() < bound      # measured: at most 3.5e-12 (L = 6, D / chi = 80)
            assert np.all(err[~np.isnan(err)] == 0.0)                             # two identical bins
        ctx.series_end()
    finally:
        ctx.close()


# ---- (c) refusals ------------------------------------------------------------------------------------------------------------------
def _state(ctx):
    info = ctx.series_info()
    bins = ctx.series_bins() if info[0] else np.zeros(0)
    return [bins, ctx.g, np.array(info), ctx.measure_td_fine_read(5), ctx.measure_td_fine_read(7)]


def test_refusals_leave_everything_untouched():
    """a series without bit 9 or without bit 13, B < 2, Q outside 0 .. L-1: DQMC_EINVAL, the outputs untouched, bins, G, counts and blocks
    bit-identical; then the accepted call"""
    L, m, s = 4, 10, 5
    N = L * L
    phi = _random_phi(2, N, m, 13)
    ctx = _context(2, L, m, s, band=False, every=True)
    v = np.full(2 * (6 + m), 7.0)
    dp = v.ctypes.data_as(C.POINTER(C.c_double))

    def refused(qx=0, qy=0):
        before = _state(ctx)
        ok = ctx.lib.dqmc_series_ph_vertex_host(ctx.h, qx, qy, dp, dp) == EINVAL and np.all(v == 7.0)
        return ok and all(np.array_equal(x, y) for x, y in zip(before, _state(ctx)))

    try:
        ctx.set_custom_bond_bilinears([cb.B_RAND, cb.B_ONSITE])
        ctx.set_green_matrix(True)
        assert ctx.lib.dqmc_series_ph_vertex_size(ctx.h) == 0 and ctx.lib.dqmc_series_ph_vertex_host(ctx.h, 0, 0, dp, dp) == EINVAL      # no series
        for parts in (512, 8192):
            ctx.series_begin(1, 4, 2, parts)
            _start(ctx, [phi])
            _full_pass(ctx)
            ctx.series_add_sweep()
            ctx.series_add_sweep()
            assert ctx.lib.dqmc_series_ph_vertex_size(ctx.h) == 0 and refused(), parts
            ctx.series_end()
        ctx.series_begin(1, 4, 2, PARTS)
        assert ctx.lib.dqmc_series_ph_vertex_size(ctx.h) == 2 * (6 + m)
        _start(ctx, [phi])
        _full_pass(ctx)
        assert refused()                                                   # B = 0
        ctx.series_add_sweep()
        assert refused()                                                   # B = 1
        ctx.series_add_sweep()
        for Q in ((L, 0), (0, L), (-1, 0), (0, -1)):
            assert refused(*Q), Q
        before = _state(ctx)
        val, err = ctx.series_ph_vertex((0, 0))
        assert val.shape == (1, 2, 6 + m) and np.all(np.isfinite(val)) and np.all(err == 0.0)      # two identical bins
        assert all(np.array_equal(x, y) for x, y in zip(before, _state(ctx)))
        _raises(lambda: ctx.set_custom_bilinears([M_RAND]))              # the open series holds bit 9: the table stays valid
        ctx.series_end()
        ctx.set_green_matrix(False)
    finally:
        ctx.close()


def test_lds_limit_is_refused():
    """O(3), L = 18: the two rows need 4 R^2 N doubles + 8 KiB = 170 KiB > 152 KiB: DQMC_EINVAL, the outputs untouched, nothing launched"""
    L, m, s = 18, 4, 2
    N = L * L
    ctx = _context(3, L, m, s, band=False, every=True)
    try:
        ctx.set_custom_bilinears([M_NX])
        ctx.set_green_matrix(True)
        ctx.series_begin(1, 4, 1, PARTS)
        _import_bins(ctx, np.zeros((2, m + 1, N, 4, 4), dtype=complex), np.zeros((2, 1, 1, N), dtype=complex))
        assert ctx.series_info()[0] == 2
        ctx.profile_enable(True)
        v = np.full(6 + m, 7.0)
        dp = v.ctypes.data_as(C.POINTER(C.c_double))
        assert ctx.lib.dqmc_series_ph_vertex_host(ctx.h, 0, 0, dp, dp) == EINVAL and np.all(v == 7.0)
        pr = ctx.profile_read()
        assert sum(pr[nm][1] for nm in ("bmult", "gemm", "decomp", "decide", "other", "gather", "flush")) == 0
        ctx.series_end()
    finally:
        ctx.close()


# ---- (d) neutrality ----------------------------------------------------------------------------------------------------------------
def test_call_leaves_every_block_and_launch_alone():
    """two contexts run the same three measurement passes into a series; one of them asks for the vertex after the second pass.  Blocks,
    bins, statistics and G are bit-identical, and the launches differ by the call's own three (bin means and the two kernels)"""
    L, m, s = 4, 10, 5
    phis = [_random_phi(2, L * L, m, 50 + it) for it in range(3)]
    results = []
    for call in (False, True):
        ctx = _context(2, L, m, s, band=False, every=True, bc="apbc-x")
        try:
            ctx.set_custom_bond_bilinears([cb.B_RAND, cb.B_DDW])
            ctx.set_green_matrix(True)
            ctx.series_begin(1, 4, 2, PARTS)
            ctx.profile_enable(True)
            for it, phi in enumerate(phis):
                _start(ctx, [phi])
                _full_pass(ctx)
                ctx.series_add_sweep()
                if call and it == 1:
                    val, _ = ctx.series_ph_vertex((0, 0))
                    assert np.all(np.isfinite(val[:, :, [0, 1, 4]]))
            pr = ctx.profile_read()
            launches = [pr[nm][1] for nm in ("bmult", "gemm", "decomp", "decide", "other", "gather", "flush")]
            blocks = [ctx.measure_td_fine_read(5), ctx.measure_td_fine_read(7), ctx.series_bins(), ctx.g] + list(ctx.series_stats())
            results.append((blocks, launches))
            ctx.series_end()
        finally:
            ctx.close()
    (b0, l0), (b1, l1) = results
    extra = [y - x for x, y in zip(l0, l1)]
    print(f"launches per family without the call {l0}, with it {l1}")
    assert all(np.array_equal(x, y) and x.any() for x, y in zip(b0, b1))
    assert sum(extra) == 3 and sorted(extra)[-1] == 3
