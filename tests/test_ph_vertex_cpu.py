"""The particle-hole bubble and vertex of the user-defined bilinears, the part that needs no GPU: sign and index of
gbar(0,tau_k) = -gbar(tau_{m-k},0) on the free matrix of the oracle, the B = 0 shortcut of the numpy twin detqmc_amd.ph_bubble against the
full double sum of tests/ph_bubble_reference.py, the algebraic symmetry of the bubble, the precision of the reference on the bins the GPU
test injects, and the entry points.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_bond_reference as cb
import pair_vertex_reference as pv
import ph_bubble_reference as ph

BCS = ("pbc", "apbc-x", "apbc-y", "apbc-xy")


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("opdim", [2, 3])
def test_sign_and_index_of_the_relation(opdim, bc):
    """free matrix (field 1e-150, dense propagator), L = 4, m = 6: -G(tau_{m-k}, 0) equals the directly computed G(0, tau_k) for every
    k = 0 .. m, the ends with the rows of k_td_ends (G, 1 - G and G - 1, -G); bound 1e-11 as the Wick checks of the pair-vertex test.  A
    wrong sign or index (k for m - k) fails by order one"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle
    L, m, s = 4, 6, 3
    phi = np.full((m + 1, L * L, opdim), ph.FREE_PHI)
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=False, delaySteps=4)
    chain = Chain(ora)
    G = four_greens(chain, m)[3]                            # G(0)
    one = np.eye(G.shape[0])
    gt0, g0t = {0: G, m: one - G}, {0: G - one, m: -G}
    for k in range(1, m):
        _, gt0[k], g0t[k], _ = four_greens(chain, k)
    worst, wrong = 0.0, np.inf
    for k in range(m + 1):
        worst = max(worst, np.abs(-gt0[m - k] - g0t[k]).max())
        if 2 * k != m:
            wrong = min(wrong, np.abs(-gt0[k] - g0t[k]).max(), np.abs(gt0[m - k] - g0t[k]).max())
    print(f"O({opdim}) {bc}: max |-G(tau_(m-k),0) - G(0,tau_k)| {worst:.2e} (1e-11); the smallest deviation of a wrong index or sign {wrong:.2e}")
    assert worst < 1e-11 and wrong > 1e-3


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("bc", BCS)
def test_b0_shortcut_and_numpy_twin(R, bc):
    """detqmc_amd.ph_bubble evaluates the site pair (d, 0) only; on a random translation-covariant block it equals the full double sum of
    the reference (bond_correlators_full on the rebuilt dense matrices, one-body product subtracted) for B_RAND, B_DDW, B_ONSITE and the
    sector-crossing M_SX_BANDX: 1e-13 of the largest entry per operator.  ph_one_body likewise.  Leading axes are carried along"""
    from detqmc_amd import ph_bubble, ph_one_body
    L, m = 4, 3
    rng = np.random.default_rng(31 * R + len(bc))
    g = pv.covariant_gbar(L, m, R, bc, rng)
    ops = ph.vertex_ops()
    ref = ph.bubbles(g, ops, L, bc)
    got = ph_bubble(g, ops, L, bc)
    top = np.abs(ref).max(axis=(0, 2))
    e = np.abs(got - ref).max(axis=(0, 2)) / top
    oref, ogot = ph.one_body(g[0], ops, L, bc), ph_one_body(g[0], ops, L, bc)
    eo = np.abs(ogot - oref).max() / np.abs(oref).max()
    print(f"R={R} {bc}: max |shortcut - double sum| / max |chibar| per operator {['%.1e' % x for x in e]}, max |chibar| {['%.3f' % x for x in top]}; "
          f"one-body {eo:.2e}, |obar| {['%.3f' % abs(x) for x in oref]}")
    assert got.shape == (m + 1, len(ops), L * L) and top.min() > 1e-3 and e.max() < 1e-13
    assert ogot.shape == (len(ops),) and eo < 1e-13
    two = ph_bubble(np.stack([g, 2.0 * g]), ops[:2], L, bc)                 # a leading axis; the bubble is quadratic in g
    assert two.shape == (2, m + 1, 2, L * L) and np.abs(two[0] - got[:, :2]).max() < 1e-13 * top.max()
    assert np.abs(two[1] - 4.0 * got[:, :2]).max() < 1e-12 * top.max()
    assert ph_one_body(np.stack([g[0], g[1]]), ops, L, bc).shape == (2, len(ops))
    with pytest.raises(ValueError):
        ph_bubble(g[:, :-1], ops, L, bc)
    with pytest.raises(ValueError):
        ph_bubble(g, ops, L, "open")
    with pytest.raises(ValueError):
        ph_bubble(g[0], ops, L, bc)                         # the tau axis is missing


@pytest.mark.parametrize("L,R", [(4, 2), (4, 4), (6, 2)])
@pytest.mark.parametrize("bc", ["pbc", "apbc-xy"])
def test_bubble_symmetry_on_random_bins(L, R, bc):
    """chibar_c(d, tau_k) = chibar_c(-d, tau_{m-k}) for any block, by the cyclicity of the trace and translation covariance: algebraic, not
    physical.  1e-13 of the largest entry"""
    from detqmc_amd import ph_bubble
    m = 5
    rng = np.random.default_rng(7 * L + R)
    g = pv.covariant_gbar(L, m, R, bc, rng)
    ops = ph.vertex_ops()
    x = ph_bubble(g, ops, L, bc)
    N = L * L
    dx, dy = np.arange(N) % L, np.arange(N) // L
    minus = ((-dy) % L) * L + (-dx) % L
    e = np.abs(x - x[::-1][:, :, minus]).max() / np.abs(x).max()
    asym = np.abs(x - x[:, :, minus]).max() / np.abs(x).max()
    print(f"L={L} R={R} {bc}: max |chibar(d, tau_k) - chibar(-d, tau_(m-k))| / max |chibar| = {e:.2e}; without the tau reflection {asym:.2e}")
    assert e < 1e-13 and asym > 1e-3


def test_reference_precision_on_the_injected_bins():
    """the reference on the bins the GPU test injects (L = 4, R = 2 and 4, pbc and apbc-xy), in float64 and in np.longdouble: the largest
    difference, values against max |value| and errors against max err per output column class, is the figure the GPU bound is 100 x of.
    Measured: values 2.3e-16 .. 3.0e-15 at the twelve (case, Q); errors 2.0e-14 .. 7.59e-13, the largest at O(2) pbc Q = (1, 2); recorded,
    rounded up, as ph_bubble_reference.REFERENCE_PRECISION = 7.6e-13, so the GPU bound is 7.6e-11.  The package's own numpy route
    (ph_bubble, ph_one_body, jackknife) agrees with the float64 reference within that GPU bound (measured: at most 3.4e-13).  The long
    double pass takes about a minute"""
    worst = 0.0
    for opdim, L, m, bc in ph.VERTEX_CASES:
        ops = ph.vertex_ops()
        gb, chb = ph.vertex_bins(L, m, 4 if opdim == 3 else 2, bc)
        P = {Q: chb[:, :, 0, Q[1] * L + Q[0]].real for Q in ph.VERTEX_QS}
        ld = ph.jackknife_outputs_qs(gb, P, ops, L, bc, ph.VERTEX_DTAU, np.longdouble)
        f64 = ph.jackknife_outputs_qs(gb, P, ops, L, bc, ph.VERTEX_DTAU, np.float64)
        for Q in ph.VERTEX_QS:
            (v64, e64), (vld, eld) = f64[Q], ld[Q]
            dv = float(np.abs(v64 - vld).max() / np.abs(vld).max())
            de = float(np.abs(e64 - eld).max() / np.abs(eld).max())
            vt, et = ph.twin_jackknife(gb, P[Q], ops, L, bc, ph.VERTEX_DTAU, Q)
            tv = float(np.abs(vt - v64).max() / np.abs(v64).max())
            te = float(np.abs(et - e64).max() / np.abs(e64).max())
            print(f"O({opdim}) L={L} {bc} Q={Q}: float64 vs longdouble, values {dv:.2e} of max |value| {float(np.abs(vld).max()):.3e}, "
                  f"errors {de:.2e} of max err {float(eld.max()):.3e}; numpy twin vs float64 reference {tv:.2e}, {te:.2e}; "
                  f"min |chi| {np.abs(v64[:, 0]).min():.2f}")
            assert np.all(np.isfinite(v64)) and np.all(e64[:, :4] > 0) and np.all(e64[:, 5:] > 0)
            # D: only at Q = 0 (the sector-crossing matrix has obar = 0 for R = 2: the blocks between the sectors vanish)
            assert (np.all(e64[:3, 4] > 0) and np.all(v64[:3, 4] != 0)) if Q == (0, 0) else not v64[:, 4].any()
            assert tv < ph.gpu_bound() and te < ph.gpu_bound()
            worst = max(worst, dv, de)
    print(f"largest relative difference {worst:.2e}; recorded {ph.REFERENCE_PRECISION:.1e}; GPU bound {ph.gpu_bound():.1e}")
    assert worst <= ph.REFERENCE_PRECISION


def test_library_and_python_layer_carry_the_entry_points():
    """the new symbols are exported and bound, NULL handles are refused with nothing touched, no struct changed its size, the names"""
    import detqmc_amd
    from detqmc_amd import KernelContext, _lib, model
    lib = _lib.load()
    bound = {s[0] for s in _lib.SYMBOLS}
    for sym in ("dqmc_series_ph_vertex_size", "dqmc_series_ph_vertex_host", "detsdw_series_ph_vertex"):
        assert hasattr(lib, sym) and sym in bound, sym
    out = np.zeros(4)
    dp = out.ctypes.data_as(_lib._DP)
    assert lib.dqmc_series_ph_vertex_size(None) == 0 and lib.dqmc_series_ph_vertex_host(None, 0, 0, dp, dp) == -1 and not out.any()
    assert lib.detsdw_series_ph_vertex(None, 0, 0, 0, dp, dp) == -1 and not out.any()
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264 and C.sizeof(_lib.dqmc_series_state) == 56
    assert callable(KernelContext.series_ph_vertex)
    assert callable(detqmc_amd.ph_bubble) and callable(detqmc_amd.ph_one_body)
    for name in ("series_ph_bubble_all", "series_derived_all"):
        assert callable(getattr(detqmc_amd.DetSDWBatch, name)), name
    for c in range(4):
        for e, nm in enumerate(("vertexCustom", "bubbleCustom", "gammaCustom", "gammaBubbleCustom", "disconnectedCustom")):
            assert model.ph_vertex_quantity(f"{nm}{c}") == (e, c)
            assert model.pair_vertex_quantity(f"{nm}{c}") is None and model.custom_ratio(f"{nm}{c}") is None
            assert model.custom_observable(f"{nm}{c}") is None
        assert model.ph_vertex_quantity(f"gammaCustomPair{c}") is None and model.ph_vertex_quantity(f"R_custom{c}") is None
    for bad in ("gammaCustom4", "gammaCustom", "GammaCustom0", "gammaBubbleCustom00", "bubbleCustomPair0", "custom0Tau", ""):
        assert model.ph_vertex_quantity(bad) is None, bad
