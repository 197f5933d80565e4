"""The averaged Green's function block, the pairing bubble and the vertex, the part that needs no GPU: the sign convention of the block on
the free matrix of the oracle, bin -> rebuild, the bubble of a translation-covariant matrix against the Wick form itself, the B = 0
shortcut, the numpy twin detqmc_amd.pair_bubble, the precision of the reference on the bins the GPU test injects, and the entry points.
Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_pair_reference as cp
import pair_vertex_reference as pv

BCS = ("pbc", "apbc-x", "apbc-y", "apbc-xy")


def _free(opdim, bc, L=4, m=20, s=5, tau=10):
    """the oracle's free matrix and its shifted G(tau, 0).  phi = 0 itself divides 0 / 0 in sinh(lambda dtau |phi|) / |phi|, in the oracle as in
    the reference; phi = 1e-150 (its square is still a normal number) leaves every field term 150 orders below the last bit of the hopping part: the same matrices.
    The dense propagator e^{-dtau K} is used: the checkerboard break-up is invariant under even translations only, which moves the summand
    by O(dtau^3) (1e-4 here) from site to site -- part of the Trotter error, not of the convention under test"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    phi = np.full((m + 1, L * L, opdim), pv.FREE_PHI)
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=False, delaySteps=4)
    return ora, shift_symmetric(ora, four_greens(Chain(ora), tau)[1])


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("opdim", [2, 3])
def test_sign_convention_on_the_free_matrix(opdim, bc):
    """sigma(B, d) g~((B (+) d) r; B c) of the free matrix does not depend on B (1e-13), bin -> rebuild gives the matrix back (1e-13), and
    without the sign the spread is of order one wherever a direction is antiperiodic: a wrong convention fails"""
    from td_ph_reference import expand
    ora, gs = _free(opdim, bc)
    L, N = ora.L, ora.N
    s = pv.summand(gs, L, bc)
    spread = np.abs(s - s[0]).max()
    plain = pv.summand(gs, L, "pbc")
    spread_plain = np.abs(plain - plain[0]).max()
    back = np.abs(pv.rebuild(pv.bin_green(gs, L, bc) / N, L, bc) - expand(ora, gs)).max()
    print(f"O({opdim}) {bc}: spread over B {spread:.2e} (without sigma {spread_plain:.2e}), max |g| {np.abs(gs).max():.3f}, bin -> rebuild {back:.2e}")
    assert np.abs(gs).max() > 0.1 and spread < 1e-13 and back < 1e-13
    assert bc == "pbc" or spread_plain > 1e-3


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_bubble_of_a_covariant_matrix_is_the_wick_form(opdim, bc):
    """for the free matrix the bubble of the binned block equals pair_correlators_full on the matrix itself; the bound of the Wick checks
    of tests/test_custom_pair_cpu.py, 1e-11"""
    from detqmc_amd import pair_operator
    ora, gs = _free(opdim, bc)
    for ops in (cp.pair_ops(), [pair_operator("d_bond")]):
        ref = np.array(cp.pair_correlators(ora, ops, gs))
        got = pv.bubble(pv.bin_green(gs, ora.L, bc) / ora.N, ops, ora.L, bc)
        e = np.abs(got - ref).max()
        print(f"O({opdim}) {bc}, {len(ops)} operators: max |bubble - Wick| {e:.2e}, max |C| {np.abs(ref).max():.3f}")
        assert np.abs(ref).max() > 1e-6 and e < 1e-11


@pytest.mark.parametrize("L,R", [(4, 2), (4, 4), (6, 2), (6, 4)])
@pytest.mark.parametrize("bc", BCS)
def test_b0_shortcut_and_numpy_twin(L, R, bc):
    """detqmc_amd.pair_bubble evaluates the site pair (d, 0) only; on a random translation-covariant block it equals the full double sum of
    the test reference: 1e-13 of the largest entry.  Leading axes are carried along"""
    from detqmc_amd import pair_bubble, pair_operator
    rng = np.random.default_rng(17 * L + R)
    g = pv.covariant_gbar(L, 2, R, bc, rng)
    ops = cp.pair_ops() + [pair_operator("d_bond")]
    ref = np.array([pv.bubble(g[k], ops, L, bc) for k in range(3)])
    got = pair_bubble(g, ops, L, bc)
    e = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"L={L} R={R} {bc}: max |shortcut - double sum| / max |Pbar| = {e:.2e}, max |Pbar| {np.abs(ref).max():.3f}")
    assert got.shape == (3, len(ops), L * L) and e < 1e-13
    one = pair_bubble(g[1], ops[:2], L, bc)                 # numpy may order the contraction differently without the leading axis
    assert one.shape == (2, L * L) and np.abs(one - got[1, :2]).max() < 1e-13 * np.abs(ref).max()
    with pytest.raises(ValueError):
        pair_bubble(g[:, :-1], ops, L, bc)
    with pytest.raises(ValueError):
        pair_bubble(g, ops, L, "open")


def test_reference_precision_on_the_injected_bins():
    """the reference of the GPU test of the derived kernels on its own bins (both cases: the R = 2 and the R = 4 row), in float64 and in
    np.longdouble: the largest difference, values against max |value| and errors against max err, is the figure the GPU bound is 100 x
    of (floor 1e-12).  Measured: values 1.4e-16 .. 6.6e-16; errors 4.05e-14 and 1.75e-14 (O(2)), 1.55e-14 and
    1.53e-14 (O(3)) at the two Q; the largest, 4.05e-14, is recorded as pair_vertex_reference.REFERENCE_PRECISION = 4.3e-14 (what an earlier
    ordering of the same reference sums gave, rounded up), so the GPU bound is 4.3e-12.  The long double pass takes about a minute."""
    worst = 0.0
    for opdim, L, m, bc in pv.VERTEX_CASES:
        ops = pv.vertex_ops()
        gb, cb = pv.vertex_bins(L, m, 4 if opdim == 3 else 2, len(ops))
        P = {Q: cb[:, :, 0, Q[1] * L + Q[0]].real for Q in pv.VERTEX_QS}
        ld = pv.jackknife_outputs_qs(gb, P, ops, L, bc, 0.1, np.longdouble)
        for Q in pv.VERTEX_QS:
            v64, e64 = pv.jackknife_outputs(gb, P[Q], ops, L, bc, 0.1, Q)
            vld, eld = ld[Q]
            dv = float(np.abs(v64 - vld).max() / np.abs(vld).max())
            de = float(np.abs(e64 - eld).max() / np.abs(eld).max())
            print(f"O({opdim}) L={L} {bc} Q={Q}: float64 vs longdouble, values {dv:.2e} of max |value| {float(np.abs(vld).max()):.3e}, "
                  f"errors {de:.2e} of max err {float(eld.max()):.3e}")
            assert np.all(np.isfinite(v64)) and np.all(e64[:, 1:] > 0)
            worst = max(worst, dv, de)
    print(f"largest relative difference {worst:.2e}; recorded {pv.REFERENCE_PRECISION:.1e}; GPU bound {pv.gpu_bound():.1e}")
    assert worst <= pv.REFERENCE_PRECISION


def test_library_and_python_layer_carry_the_entry_points():
    """the new symbols are exported and bound, NULL handles are refused, no struct changed its size, the constants have their values"""
    import detqmc_amd
    from detqmc_amd import KernelContext, _lib, model
    lib = _lib.load()
    bound = {s[0] for s in _lib.SYMBOLS}
    for sym in ("dqmc_set_green_matrix", "dqmc_measure_timedisplaced_green_matrix", "dqmc_measure_td_green_matrix_accum_size",
                "dqmc_measure_td_green_matrix_read_host", "dqmc_series_pair_vertex_size", "dqmc_series_pair_vertex_host"):
        assert hasattr(lib, sym) and sym in bound, sym
    out = np.zeros(4)
    dp = out.ctypes.data_as(_lib._DP)
    assert lib.dqmc_set_green_matrix(None, 1) == -1 and lib.dqmc_measure_timedisplaced_green_matrix(None, 1) == -1
    assert lib.dqmc_measure_td_green_matrix_accum_size(None) == 0 and lib.dqmc_measure_td_green_matrix_read_host(None, dp) == -1
    assert lib.dqmc_series_pair_vertex_size(None) == 0 and lib.dqmc_series_pair_vertex_host(None, 0, 0, dp, dp) == -1 and not out.any()
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264 and C.sizeof(_lib.dqmc_series_state) == 56
    assert _lib.DQMC_SERIES_GREEN_MATRIX == 8192 == model.SERIES_GREEN_MATRIX
    for name in ("set_green_matrix", "measure_timedisplaced_green_matrix", "measure_td_green_matrix_read", "series_pair_vertex"):
        assert callable(getattr(KernelContext, name)), name
    assert callable(detqmc_amd.pair_bubble)
    # the host layer and the names
    for sym in ("detsdw_set_green_matrix", "detsdw_series_pair_vertex"):
        assert hasattr(lib, sym) and sym in bound, sym
    assert lib.detsdw_set_green_matrix(None, 1) == -1 and lib.detsdw_series_pair_vertex(None, 0, 0, 0, dp, dp) == -1 and not out.any()
    for name in ("set_green_matrix", "series_pair_bubble_all"):
        assert callable(getattr(detqmc_amd.DetSDWBatch, name)), name
    assert model.GREEN_MATRIX_OBS == 74
    for c in range(4):
        for e, nm in enumerate(("vertexCustomPair", "bubbleCustomPair", "gammaCustomPair", "gammaBubbleCustomPair")):
            assert model.pair_vertex_quantity(f"{nm}{c}") == (e, c)
            assert model.custom_pair_ratio(f"{nm}{c}") is None and model.custom_pair_observable(f"{nm}{c}") is None
    for bad in ("gammaCustomPair4", "gammaCustomPair", "GammaCustomPair0", "gammaBubbleCustomPair00", "bubbleCustom0", "R_customPair0", ""):
        assert model.pair_vertex_quantity(bad) is None, bad
