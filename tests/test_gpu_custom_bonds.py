"""Bond parts of the user-defined bilinears on the device: the stencil kernels against numpy on the device's own matrices
(tests/custom_bond_reference.py), agreement with the on-site custom kernel and with the current kernel, reproducibility, batching and
the channel -> row mapping, every slice and the Matsubara transform, the preconditions, and the host level: vectors, a routed series
with R_custom at a chosen Q, the file round trip.

Tolerances are the project's: relerr < 1e-10 for a kernel against numpy on the device's own matrices, bit equality wherever a text says
so, and the bounds of tests/test_gpu_td_fine.py where that file sets one.  Every test prints its figures before it asserts."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

import custom_bond_reference as cb
import series_reference as sr
import td_fine_reference as tf
from conftest import relerr
from custom_reference import M_NX, M_RAND, M_SX_BANDX
from test_gpu_band_correlators import EINVAL, _context, _raises, _start
from test_gpu_td_particle_hole import _random_phi, _walk_down

pytestmark = pytest.mark.gpu

HOP = types.SimpleNamespace(txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)      # the hoppings of a KernelContext


def _rows(acc, nrows, count, N):
    """(counts [nrows], sums [nrows][count][N]) of a time-displaced block"""
    return acc[:nrows], acc[nrows:].reshape(nrows, count, N)


def _same_ops(got, ops):
    return len(got) == len(ops) and all(np.array_equal(g, w) for a, b in zip(got, ops) for g, w in zip(a, cb.as_arrays(b)))


def _shifted(ctx, ora):
    from td_reference import shift_symmetric
    return [shift_symmetric(ora, g) for g in (ctx.g, *ctx.green_timedisplaced()[1:], ctx.green0_timedisplaced()[1])]


def _measure_both(ctx, j):
    """time-displaced at boundary j and equal-time on the G of the same boundary"""
    ctx.measure_timedisplaced_custom(j)
    ctx.set_equal_time_custom(True)
    ctx.measure_slice()
    ctx.set_equal_time_custom(False)


# ---- 1. kernels against numpy on the device's own matrices -------------------------------------------------------------------------
# (opdim, L, checkerboard, bc, flux).  L = 4: A (+) mu wraps and the stencils of A and B overlap for most d; L = 6: N = 36 is no multiple
# of the 32 bins
KERNEL_CASES = [(1, 4, True, "pbc", False), (2, 4, True, "pbc", False), (3, 4, True, "pbc", False), (2, 4, True, "apbc-xy", False),
                (2, 4, False, "pbc", False), (2, 4, True, "pbc", True), (2, 6, True, "apbc-x", False), (3, 6, True, "pbc", False)]


@pytest.mark.parametrize("opdim,L,cbd,bc,flux", KERNEL_CASES)
def test_kernels_vs_numpy_on_device_matrices(opdim, L, cbd, bc, flux):
    """all four operators in one launch, time-displaced at tau = 10 and equal-time on the G of the same boundary"""
    from td_reference import make_oracle
    m, s, N = 20, 5, L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cbd, weakZflux=flux, delaySteps=4)
    ops = cb.bond_ops(ora.pars, flux)
    ctx = _context(opdim, L, m, s, band=False, checkerboard=cbd, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        ctx.set_custom_bond_bilinears(ops)
        assert _same_ops(ctx.get_custom_bond_bilinears(), ops)
        assert np.array_equal(ctx.get_custom_bilinears(), np.array([cb.as_arrays(op)[0] for op in ops]))
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == (n - 1) * (1 + 4 * N)
        assert ctx.lib.dqmc_measure_eq_custom_accum_size(ctx.h) == 1 + 4 * N
        _start(ctx, [phi])
        target = n - 2
        ref = {}

        def at(j):
            if j != target:
                return
            gtt = ctx.g
            sh = _shifted(ctx, ora)
            ref["td"] = cb.bond_correlators(ora, ops, *sh)
            ref["eq"] = cb.eq_bond_correlators(ora, ops, sh[0])
            _measure_both(ctx, j)
            assert np.array_equal(ctx.g, gtt)            # the measurements leave G alone

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_read(), n - 1, 4, N)
        eq = ctx.measure_eq_custom_read()
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


# ---- 2. agreement with the kernels that exist --------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,flux", [(1, False), (2, False), (3, False), (2, True)])
def test_agreement_with_existing_kernels(opdim, flux):
    """B_ONSITE inside a bond set against the on-site custom kernel alone, bond_current(x / y) against Lambda_xx / Lambda_yy of the
    current kernel, and the bond kinetic energy: relerr 1e-10, kernels that evaluate the same sums in different orders.

    The kinetic sums, x and y.  sum_d of the bond_kinetic row is (1/N) Re W[K, K] of the total operator K = sum_A k_mu(A), that is
    Re o_tau[K] o_0[K] minus the connected part tr(K gt0 K g0t) -- there is no row of the block that is sum_A o(A) alone.  So the check
    has two halves that meet in numpy's o_tau[K] on the device's matrices: the current kernel's kinetic sum is its real part, and the
    row sum plus numpy's connected part is Re o_tau[K] o_0[K]."""
    from detqmc_amd import bond_current, bond_kinetic
    from td_ph_reference import expand
    from td_reference import make_oracle
    from test_gpu_td_current import _block
    from test_gpu_td_current import _context as _current_context
    L, m, s = 4, 20, 5
    N = L * L
    phi = _random_phi(opdim, N, m, 811 + opdim)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, weakZflux=flux, delaySteps=4)
    ops = [bond_current(HOP, "x"), cb.B_ONSITE, bond_current(HOP, "y"), bond_kinetic(HOP, "x")]
    kin_ops = [bond_kinetic(HOP, "y"), bond_kinetic(HOP, "x")]            # a second set at the same boundary: k_y, and k_x in another row
    ctx = _current_context(opdim, L, m, s, weakZflux=flux)
    got = {}
    try:
        _start(ctx, [phi])

        def at(j):
            if j != 2:
                return
            full = [expand(ora, g) for g in _shifted(ctx, ora)]
            for mu in "xy":
                K = cb.dense_operators(bond_kinetic(HOP, mu), cb.link_table(L, "pbc", flux), L).sum(axis=0)
                o_tau, o_0 = [complex(cb.one_body_all(g, K[None])[0]) for g in (full[0], full[3])]
                got[mu] = (o_tau, o_0, complex(np.einsum("pq,qp->", K @ full[1], K @ full[2])))
            ctx.measure_timedisplaced_current(j)
            ctx.set_custom_bond_bilinears(ops)
            _measure_both(ctx, j)
            got["bond"] = (_rows(ctx.measure_td_custom_read(), ctx.n - 1, 4, N)[1][1], ctx.measure_eq_custom_read()[1:].reshape(4, N))
            ctx.set_custom_bond_bilinears(kin_ops)
            ctx.measure_timedisplaced_custom(j)
            got["kin"] = _rows(ctx.measure_td_custom_read(), ctx.n - 1, 2, N)[1][1]
            ctx.set_custom_bilinears([M_RAND])
            _measure_both(ctx, j)
            got["site"] = (_rows(ctx.measure_td_custom_read(), ctx.n - 1, 1, N)[1][1], ctx.measure_eq_custom_read()[1:].reshape(1, N))

        _walk_down(ctx, at)
        c1, lx, ly, kx, ky = _block(ctx.measure_td_current_read(), ctx.n, N, 2)
        assert c1 == 1.0
        (td_b, eq_b), (td_s, eq_s) = got["bond"], got["site"]
        assert np.array_equal(got["kin"][1], td_b[3]) and td_b[3].any()      # k_x: the same bits in row 1 of two as in row 3 of four
        errs = {"onsite td": relerr(td_b[1], td_s[0]), "onsite eq": relerr(eq_b[1], eq_s[0]), "Lambda_xx": relerr(td_b[0], lx),
                "Lambda_yy": relerr(td_b[2], ly)}
        figures = []
        for mu, dev_k, row in (("x", kx, td_b[3]), ("y", ky, got["kin"][0])):
            o_tau, o_0, conn = got[mu]
            row_sum = row.sum()                          # N sum_d C(d) = Re W[K, K]
            errs[f"kinetic_{mu} sum vs Re o_tau[K]"] = abs(dev_k - o_tau.real) / abs(dev_k)
            errs[f"k_{mu} row sum + conn vs o_tau o_0"] = abs(row_sum + conn.real - (o_tau * o_0).real) / abs(row_sum)
            figures.append(f"kinetic_{mu} {dev_k:.4f}, row sum {row_sum:.4f}, conn {conn.real:.4f}")
            assert abs(dev_k) > 1e-3 and abs(conn.real) > 1e-3 and abs(row_sum) > 1e-3
        print(f"O({opdim}) flux={flux}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + "; " + "; ".join(figures))
        assert min(np.abs(x).max() for x in (td_s[0], eq_s[0], lx, ly)) > 1e-6
        assert max(errs.values()) < 1e-10, errs
    finally:
        ctx.close()


# ---- 3. reproducibility, batching, the mask and the channel -> row mapping ---------------------------------------------------------
def _measure_all(ctx, phis, ops, passes=1):
    ctx.set_custom_bond_bilinears(ops)
    out = []
    for _ in range(passes):
        _start(ctx, phis)

        def at(j):
            _measure_both(ctx, j)

        _walk_down(ctx, at)
        per = []
        for b in range(len(phis)):
            ctx.select_chain(b)
            per.append((ctx.measure_td_custom_read(), ctx.measure_eq_custom_read()))
        ctx.select_chain(0)
        out.append(per)
    return out


@pytest.mark.parametrize("opdim", [2, 3])
def test_reproducibility_and_batching(opdim):
    """two identical measurement passes give bit-identical blocks; three chains in one context equal three single-chain contexts"""
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 93 + opdim + 100 * c) for c in range(3)]
    ops = cb.bond_ops(HOP)
    ctx = _context(opdim, 6, m, s, band=False, nchains=3)
    try:
        first, second = _measure_all(ctx, phis, ops, passes=2)
    finally:
        ctx.close()
    for b in range(3):
        assert np.array_equal(first[b][0], second[b][0]) and np.array_equal(first[b][1], second[b][1])
        assert np.array_equal(first[b][0][:ctx.n - 1], np.ones(ctx.n - 1)) and first[b][1][0] == ctx.n - 1
        assert all(r.any() for r in _rows(first[b][0], ctx.n - 1, 4, N)[1].reshape(-1, N))
    singles = []
    for phi in phis:
        ctx = _context(opdim, 6, m, s, band=False)
        try:
            singles.append(_measure_all(ctx, [phi], ops)[0][0])
        finally:
            ctx.close()
    assert all(np.array_equal(first[b][k], singles[b][k]) for b in range(3) for k in range(2))
    assert not np.array_equal(singles[0][0], singles[1][0]) and not np.array_equal(singles[1][1], singles[2][1])


@pytest.mark.parametrize("opdim", [1, 2, 3])
@pytest.mark.parametrize("which", [(2,), (3, 1, 0), (3, 0, 3), (0, 3, 3, 3), (3, 3, 3, 1)])
def test_mask_and_channel_mapping(opdim, which):
    """one, three and four operators with the bond-carrying ones in different positions (index 3 is the on-site-only operator, which
    takes part in the stencil launch through the mask): every channel lands in its row"""
    from td_reference import make_oracle
    L, m, s = 4, 20, 5
    N = L * L
    ops = [cb.bond_ops(HOP)[i] for i in which]
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    ctx = _context(opdim, L, m, s, band=False)
    try:
        ctx.set_custom_bond_bilinears(ops)
        assert ctx.lib.dqmc_measure_td_custom_accum_size(ctx.h) == (ctx.n - 1) * (1 + len(ops) * N)
        _start(ctx, [phi])
        ref = {}

        def at(j):
            if j != 2:
                return
            sh = _shifted(ctx, ora)
            ref["td"] = cb.bond_correlators(ora, ops, *sh)
            ref["eq"] = cb.eq_bond_correlators(ora, ops, sh[0])
            _measure_both(ctx, j)

        _walk_down(ctx, at)
        cnt, rows = _rows(ctx.measure_td_custom_read(), ctx.n - 1, len(ops), N)
        eq = ctx.measure_eq_custom_read()
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
    matsubara(channel 5, 4 frequencies) against the numpy transform of the fine block, 1e-10."""
    import td_matsubara_reference as tm
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    L, s, nfreq = 4, 5, 4
    N = L * L
    ops = cb.bond_ops(HOP)
    phi = _random_phi(opdim, N, m, 41 * opdim + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    chain = Chain(ora)
    ctx = _context(opdim, L, m, s, band=False, every=True)

    def ref_of(gtt, gt0, g0t, g00):
        return np.array(cb.bond_correlators(ora, ops, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])) * N

    try:
        n = ctx.n
        ctx.set_custom_bond_bilinears(ops)
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 5) == (m + 1) * (1 + 4 * N)
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
        a = ctx.measure_td_matsubara(5, nfreq)
        assert a.shape == (1, 4, nfreq, N) and np.array_equal(a, ctx.measure_td_matsubara(5, nfreq))
        assert np.array_equal(ctx.measure_td_fine_read(5), fine)           # the transform reads the block only
        for comp in range(4):
            ref = tm.bosonic(rows[:, comp] / N, L, 0.1, nfreq)
            e = relerr(a[0, comp], ref)
            print(f"O({opdim}) operator {comp}: chi(q, i omega_n) vs numpy on the block {e:.2e} (bound 1e-10)")
            assert np.abs(ref).max() > 1e-6 and e <= 1e-10
    finally:
        ctx.close()


# ---- 5. preconditions --------------------------------------------------------------------------------------------------------------
def _snapshot(ctx):
    got = ctx.get_custom_bond_bilinears()
    return [np.array([op[k] for op in got]) for k in range(3)] + [ctx.get_custom_bilinears(), ctx.measure_td_custom_read(), ctx.measure_eq_custom_read()]


def _unchanged(ctx, before):
    return all(np.array_equal(x, y) for x, y in zip(_snapshot(ctx), before))


def test_preconditions():
    """every refusal leaves matrices, blocks and switches untouched; set_custom_bilinears after a bond set restores the old kernels:
    the result equals, bit for bit, a fresh context that never saw a bond part"""
    from detqmc_amd import DqmcError
    phi = _random_phi(2, 16, 20, 3)

    def to_boundary_3(ctx):
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                                           # tau = 15, j = 3

    ctx = _context(2, 4, 20, 5, band=False)
    try:
        ops = [cb.B_DDW, cb.B_ONSITE]
        ctx.set_custom_bond_bilinears(ops)
        to_boundary_3(ctx)
        _measure_both(ctx, 3)
        ctx.set_equal_time_custom(True)
        before = _snapshot(ctx)
        assert before[4][2] == 1.0 and before[5][0] == 1.0 and before[4][3 + 2 * 32:].any() and not before[4][3:3 + 2 * 32].any()
        M0, Mx, My = cb.B_RAND
        nonherm = M0.copy()
        nonherm[0, 1] = complex(np.nextafter(nonherm[0, 1].real, 9.0), nonherm[0, 1].imag)       # one ulp off conj(M0[1, 0])
        nan, inf = Mx.copy(), My.copy()
        nan[2, 1] = np.nan
        inf[0, 3] = np.inf
        zero = np.zeros((4, 4))
        for bad in ([(nonherm, Mx, My)], [cb.B_DDW, (M0, nan, None)], [(M0, None, inf)], [(None, None, None)], [cb.B_DDW, (zero, zero, None)],
                    [cb.B_DDW] * 5):
            _raises(lambda: ctx.set_custom_bond_bilinears(bad))
            assert _unchanged(ctx, before)
        ctx.measure_slice()                                               # the switch is still on
        assert ctx.measure_eq_custom_read()[0] == 2.0
        ctx.set_custom_bond_bilinears([(None, Mx, None)])                 # M0 = 0 with a bond part is legal
        got = ctx.get_custom_bond_bilinears()
        assert len(got) == 1 and not got[0][0].any() and np.array_equal(got[0][1], Mx) and not got[0][2].any()
        assert not ctx.measure_td_custom_read().any() and ctx.measure_td_custom_read().shape == (3 * (1 + 16),)
        # back to the on-site kernels
        ctx.set_custom_bilinears([M_RAND, M_NX])
        assert _same_ops(ctx.get_custom_bond_bilinears(), [(M_RAND, None, None), (M_NX, None, None)])
        ctx.set_equal_time_custom(False)
        _measure_both(ctx, 3)
        after_bond = [ctx.measure_td_custom_read(), ctx.measure_eq_custom_read()]
        ctx.set_custom_bond_bilinears([])                                 # count = 0 removes everything
        assert ctx.get_custom_bond_bilinears() == [] and ctx.get_custom_bilinears().shape == (0, 4, 4)
        _raises(lambda: ctx.measure_eq_custom_read())
    finally:
        ctx.close()
    ctx = _context(2, 4, 20, 5, band=False)                               # a fresh context that never saw a bond part
    try:
        ctx.set_custom_bilinears([M_RAND, M_NX])
        to_boundary_3(ctx)
        _measure_both(ctx, 3)
        fresh = [ctx.measure_td_custom_read(), ctx.measure_eq_custom_read()]
        assert all(np.array_equal(x, y) and x.any() for x, y in zip(after_bond, fresh))
        # an open series with a custom part holds the operators
        ctx.set_equal_time_correlators(True)
        ctx.set_equal_time_correlators(False)
        ctx.series_begin(1, 2, 2, 1 | 1024)
        before = _snapshot(ctx)
        _raises(lambda: ctx.set_custom_bond_bilinears([cb.B_DDW]))
        _raises(lambda: ctx.set_custom_bond_bilinears([]))
        assert _unchanged(ctx, before)
        ctx.series_end()
        ctx.set_custom_bond_bilinears([cb.B_DDW])
    finally:
        ctx.close()
    ctx = _context(2, 4, 20, 5, band=False, weakZflux=True)               # the flux rule
    try:
        ctx.set_custom_bond_bilinears([cb.B_RAND_FLUX])
        before = _snapshot(ctx)
        offx = np.zeros((4, 4), dtype=complex)
        offx[0, 1] = 1e-300
        for bad in ([cb.B_RAND], [(None, offx, None)], [cb.B_RAND_FLUX, (M_RAND, None, offx.T)]):
            with pytest.raises(DqmcError) as e:
                ctx.set_custom_bond_bilinears(bad)
            assert e.value.code == EINVAL and "weakZflux" in str(e.value)
            assert _unchanged(ctx, before)
        ctx.set_custom_bond_bilinears([(M_SX_BANDX, np.diag(np.diag(cb.B_RAND[1])), None)])       # an off-diagonal M0 stays legal
        ctx.set_custom_bilinears([M_SX_BANDX])
    finally:
        ctx.close()
    from detqmc_amd import DetHubbard, HubbardParams
    hub = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        h = hub.lib.dethubbard_ctx(hub.h)
        m = np.ascontiguousarray(M_NX)
        cnt = C.c_int(7)
        assert hub.lib.dqmc_set_custom_bond_bilinears(h, 1, m.ctypes.data, m.ctypes.data, None) == EINVAL
        assert hub.lib.dqmc_get_custom_bond_bilinears(h, C.byref(cnt), None, None, None) == EINVAL and cnt.value == 7
    finally:
        hub.close()


# ---- 6. host level -----------------------------------------------------------------------------------------------------------------
def _batch(sub_batches, every=False, seed=4712, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=True,
                  timeDisplacedEverySlice=every, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)], sub_batches=sub_batches)


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_level_vectors(sub_batches):
    """custom{c}Tau / Corr / Sq after real measurement sweeps: Tau against numpy from direct inverses of the mixed field configuration of
    each boundary (1e-10), Corr non-zero with Sq its cosine sum (1e-12); the chains, G and the random numbers are those of a batch
    without operators"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    a, b = _batch(sub_batches), _batch(sub_batches)
    try:
        ops = cb.bond_ops(b.pars_list[0])
        a.sweepThermalization(); b.sweepThermalization()
        b.set_custom_bond_bilinears(ops)
        assert _same_ops(b.get_custom_bond_bilinears(), ops)
        for it in range(2):
            before = [b.chain(c).phi.copy() for c in range(2)]
            a.sweep(True); b.sweep(True)
            for c in range(2):
                ra, rb = a.chain(c), b.chain(c)
                assert np.array_equal(ra.phi, rb.phi) and np.array_equal(ra.g, rb.g) and ra.info.rngDrawn == rb.info.rngDrawn
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
                    ref = cb.bond_correlators(ora, ops, *[shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)])
                    for v, q, r in zip(vec, q0, ref):
                        worst = max(worst, relerr(v[j - 1], r))
                        assert abs(q[j - 1] - v[j - 1].sum()) <= 1e-14 * max(1.0, np.abs(v[j - 1]).max()), (c, j)
                print(f"sub-batches {sub_batches} chain {c} down={down}: custom Tau vs direct inverses {worst:.2e} (1e-10)")
                assert worst < 1e-10
                for k in range(4):
                    cd, sq = rb.observable_vector(f"custom{k}Corr"), rb.observable_vector(f"custom{k}Sq")
                    assert cd.shape == (16,) and np.abs(cd).max() > 1e-6
                    sr.rows_close(sq, sr.structure_factor_ref(cd, 4), 1e-12, 16)
    finally:
        a.close(); b.close()


def test_host_level_options():
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    kw = dict(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    rep = DetSDWBatch([SDWParams(**kw)])                          # neither family the operators could ride on
    try:
        with pytest.raises(DqmcError) as e:
            rep.set_custom_bond_bilinears([cb.B_DDW])
        assert e.value.code == EINVAL and "equalTimeCorrelators" in str(e.value)
    finally:
        rep.close()
    rep = DetSDWBatch([SDWParams(equalTimeCorrelators=True, **kw)])   # equal time alone
    try:
        for bad in ([(None, None, None)], [(cb.B_RAND[1], None, None)], [cb.B_DDW] * 5):
            with pytest.raises(DqmcError):
                rep.set_custom_bond_bilinears(bad)
        assert rep.get_custom_bond_bilinears() == []
        rep.set_custom_bond_bilinears([cb.B_DDW])
        rep.sweep(True)
        assert np.abs(rep.chain(0).observable_vector("custom0Sq")).max() > 1e-6
        with pytest.raises(DqmcError):
            rep.chain(0).observable_vector("custom0Tau")
        rep.series_begin(1, 4, host_copy=False)                  # a NO_HOST_COPY series refuses the setter, nothing changes
        with pytest.raises(DqmcError) as e:
            rep.set_custom_bond_bilinears([cb.B_RAND])
        assert e.value.code == EINVAL and "NO_HOST_COPY" in str(e.value)
        assert _same_ops(rep.get_custom_bond_bilinears(), [cb.B_DDW])
        rep.series_end()
        rep.set_custom_bond_bilinears([cb.B_RAND])
    finally:
        rep.close()


@pytest.mark.parametrize("opdim,beta", [(2, 2.0), (3, 2.2)])
def test_host_matsubara_by_name(opdim, beta):
    """matsubara("custom{c}Tau", 4) of a measurement sweep (m = 20 and m = 22, s = 5) against the numpy transform of the fine vector
    'custom{c}TauFine', the bound of tests/test_gpu_td_matsubara.py: 1e-10"""
    import td_matsubara_reference as tm
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=opdim, L=4, beta=beta, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True,
                  timeDisplacedMeasurements=True, timeDisplacedParticleHole=True, timeDisplacedEverySlice=True, rngSeed=77 + opdim)
    b = DetSDWBatch([p])
    try:
        ops = cb.bond_ops(p)
        b.sweepThermalization()
        b.set_custom_bond_bilinears(ops)
        b.sweep(True)
        r = b.chain(0)
        m = r.info.m
        assert m == round(beta / 0.1)
        errs = []
        for c in range(4):
            fine = r.observable_vector(f"custom{c}TauFine")
            ref = tm.bosonic(fine, 4, 0.1, 4)
            dev = r.matsubara(f"custom{c}Tau", 4)
            assert fine.shape == (m + 1, 16) and dev.shape == (4, 16) and np.abs(ref).max() > 1e-6
            errs.append(relerr(dev, ref))
        print(f"O({opdim}) m={m}: matsubara('custom{{c}}Tau', 4) vs numpy on the fine vector {['%.1e' % e for e in errs]} (1e-10)")
        assert max(errs) <= 1e-10
    finally:
        b.close()


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_level_series(tmp_path, sub_batches):
    """a routed series over three sweeps with bond operators: the bins of the custom parts are the vectors / Matsubara transforms of the
    sweeps in the routed slots, R_custom0 at a chosen Q against the numpy jackknife of tests/series_reference.py (1e-12), and the file:
    the round trip with bond parts, byte identity without, and the refusal of a file with another Mx"""
    from custom_reference import correlation_ratio
    from detqmc_amd import DqmcError
    ops = [cb.B_RAND, cb.B_ONSITE]
    b = _batch(sub_batches, every=True)
    path, plain, plain2 = [str(tmp_path / f) for f in ("bond.bin", "site_a.bin", "site_b.bin")]
    try:
        b.sweepThermalization()
        b.set_custom_bond_bilinears(ops)
        b.series_begin(1, 4, nfreq=2)
        b.series_route([1, 0])
        seen = []
        for it in range(3):
            b.sweep(True)
            seen.append([(b.chain(c).observable_vector("custom0Corr"), b.chain(c).observable_vector("custom0Sq"),
                          b.chain(c).matsubara("custom0Tau", 2)) for c in range(2)])
        for c in range(2):
            slot = b.chain(1 - c)                                 # chain c fed slot 1 - c
            corr, sq, mats = slot.series_bins("custom0Corr"), slot.series_bins("custom0Sq"), slot.series_bins("custom0Tau")
            assert corr.shape == (3, 16) and mats.shape == (3, 2, 16)
            for it in range(3):
                sr.rows_close(corr[it], seen[it][c][0], 1e-14, 16)
                sr.rows_close(sq[it], seen[it][c][1], 1e-12, 16)
                assert np.array_equal(mats[it], seen[it][c][2]) and mats[it].any()
        val, verr = b.series_derived_all("R_custom0", Q=(1, 0))
        for c in range(2):
            bins = b.chain(c).series_bins("custom0Sq")
            rv, rerr = sr.jackknife(bins, lambda x: correlation_ratio(x, 4, 1, 0))
            print(f"slot {c}: R_custom0(1, 0) = {val[c]:.6f} +- {verr[c]:.2e} (numpy {rv:.6f} +- {rerr:.2e})")
            assert abs(val[c] - rv) <= 1e-12 and abs(verr[c] - rerr) <= 1e-10 * rerr
        with pytest.raises(DqmcError):
            b.set_custom_bond_bilinears([cb.B_DDW])               # the open series holds their parts
        b.series_save(path)
        kept = [b.chain(c).series_bins("custom0Corr") for c in range(2)]
        b.series_end()
        b.series_begin(1, 4, nfreq=2)
        b.series_load(path)                                       # the round trip with bond parts
        assert b.series_route() == [1, 0]
        assert all(np.array_equal(b.chain(c).series_bins("custom0Corr"), kept[c]) for c in range(2))
        b.series_end()
        other = [(cb.B_RAND[0], 2.0 * cb.B_RAND[1], cb.B_RAND[2]), cb.B_ONSITE]     # another Mx
        for wrong in (other, None):
            if wrong is None:
                b.set_custom_bilinears([cb.B_RAND[0], M_RAND])    # the same M0 and no bond part
            else:
                b.set_custom_bond_bilinears(wrong)
            b.series_begin(1, 4, nfreq=2)
            b.sweep(True)
            state = [b.chain(c).series_bins("custom0Corr") for c in range(2)]
            with pytest.raises(DqmcError) as e:
                b.series_load(path)
            assert e.value.code == EINVAL and "bond parts" in str(e.value)
            assert all(np.array_equal(b.chain(c).series_bins("custom0Corr"), state[c]) for c in range(2))     # the series is as it was
            if wrong is None:
                b.series_save(plain)
            b.series_end()
        # no bond part: the bytes of a file written through set_custom_bilinears, and such a file is refused by a handle with bond parts
        b.set_custom_bond_bilinears([(cb.B_RAND[0], None, None), (M_RAND, None, np.zeros((4, 4)))])
        b.series_begin(1, 4, nfreq=2)
        b.series_load(plain)
        b.series_save(plain2)
        b.series_end()
        data = open(plain, "rb").read()
        assert data == open(plain2, "rb").read()
        b.series_begin(1, 4, nfreq=2)
        for tail in (b"\0" * 2, b"\0" * 8):                     # neither a bond block nor the end of the file: said so, not taken for bond parts
            open(plain2, "wb").write(data + tail)
            with pytest.raises(DqmcError) as e:
                b.series_load(plain2)
            assert "bond parts" not in str(e.value) and ("truncated" in str(e.value) or "longer" in str(e.value))
        b.series_end()
        b.set_custom_bond_bilinears([cb.B_RAND, (M_RAND, None, None)])
        b.series_begin(1, 4, nfreq=2)
        with pytest.raises(DqmcError) as e:
            b.series_load(plain)
        assert e.value.code == EINVAL and "bond parts" in str(e.value)
        b.series_end()
    finally:
        b.close()
