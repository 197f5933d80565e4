"""User-defined bilinear correlators, the part that needs no GPU: the general-M Wick reference against exact diagonalisation (a dense
and two sector-crossing matrices, M^2 != 1), inputs on which the GPU comparison at 1e-10 can tell a wrong kernel from a right one, and
the entry points in the built library and the Python layer."""
import ctypes as C

import numpy as np
import pytest

from custom_reference import CUSTOM_MS, M_NX, M_RAND, M_SX_BANDX, M_SY_BANDY, correlation_ratio, custom_correlators, custom_wick, eq_custom_correlators
from test_band_correlators_cpu import _kernel_test_inputs
from test_td_particle_hole_cpu import _exp_herm, _fock_operators


def test_the_four_matrices():
    assert np.array_equal(M_RAND, M_RAND.conj().T) and np.count_nonzero(M_RAND) == 16 and np.abs(M_RAND.imag).max() > 0.1
    assert np.abs(M_RAND @ M_RAND - np.eye(4)).max() > 0.5                 # the delta term needs M^2, not 1
    assert M_SX_BANDX[0, 2] == M_SX_BANDX[2, 0] == 1 and np.count_nonzero(M_SX_BANDX) == 2
    assert np.array_equal(np.diag(M_NX), [1, 0, 1, 0]) and np.count_nonzero(M_NX) == 2
    assert M_SY_BANDY[1, 3] == 1j and M_SY_BANDY[3, 1] == -1j and np.count_nonzero(M_SY_BANDY) == 2
    for M in CUSTOM_MS:
        assert np.array_equal(M, M.conj().T)


@pytest.mark.parametrize("nfac,cut", [(4, 2), (5, 1)])
def test_wick_against_exact_many_body(nfac, cut):
    """2 sites x 4 flavours on the 256-dimensional Fock space, as tests/test_band_correlators_cpu.py does for its matrices:
    Tr[U_l O_i U_r O_j] / Tr[U] against W^M and the equal-time form against Tr[U O_i O_j] / Tr[U], every site pair, for the dense random
    matrix and the two sector-crossing ones.  numpy fp64 on O(1) numbers: 1e-11, the bound of that file."""
    from eq_corr_reference import wick_eq
    from td_ph_reference import greens_from_b, wick
    ns, nm = 2, 8
    rng = np.random.default_rng(900 * nfac + cut)
    c = _fock_operators(nm)
    cd = [x.conj().T for x in c]
    hs = []
    for _ in range(nfac):
        h = rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm))
        h = 0.5 * (h + h.conj().T)
        hs.append(h / np.linalg.norm(h, 2))
    Us = [_exp_herm(sum(h[a, b] * cd[a] @ c[b] for a in range(nm) for b in range(nm))) for h in hs]
    Bs = [_exp_herm(h) for h in hs]

    def prod(fs, lo, hi, dim):
        out = np.eye(dim, dtype=complex)
        for k in range(lo, hi):
            out = fs[k] @ out
        return out

    Ur, Ul = prod(Us, 0, cut, 2 ** nm), prod(Us, cut, nfac, 2 ** nm)
    gtt, gt0, g0t, g00 = greens_from_b(prod(Bs, 0, cut, nm), prod(Bs, cut, nfac, nm))
    Z = np.trace(Ul @ Ur)
    worst = worst_eq = 0.0
    for M in (M_RAND, M_SX_BANDX, M_SY_BANDY, M_NX):
        O = [sum(M[a, b] * cd[a * ns + i] @ c[b * ns + i] for a in range(4) for b in range(4) if M[a, b] != 0) for i in range(ns)]
        W = wick(gtt, gt0, g0t, g00, M, ns)
        Weq = wick_eq(g00, M, ns)
        for i in range(ns):
            for j in range(ns):
                worst = max(worst, abs(np.trace(Ul @ O[i] @ Ur @ O[j]) / Z - W[i, j]))
                worst_eq = max(worst_eq, abs(np.trace(Ul @ Ur @ O[i] @ O[j]) / Z - Weq[i, j]))
    print(f"{nfac} factors, cut {cut}: worst |ED - Wick| = {worst:.2e}, equal time {worst_eq:.2e}")
    assert worst < 1e-11 and worst_eq < 1e-11


@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_discriminating_inputs(opdim):
    """the inputs of the GPU kernel test (L = 4, m = 20, s = 5, tau = 10): every matrix has a correlator far above the 1e-6 floor that
    test asserts, time-displaced and equal-time, and W of the random matrix has an imaginary part between 5e-3 and 0.13 -- a kernel that
    drops a conjugate somewhere moves Re W by that much and cannot pass at 1e-10"""
    ora, gs = _kernel_test_inputs(opdim)
    td = custom_correlators(ora, CUSTOM_MS, *gs)
    eq = eq_custom_correlators(ora, CUSTOM_MS, gs[0])
    mtd, meq = [np.abs(c).max() for c in td], [np.abs(c).max() for c in eq]
    im = np.abs(custom_wick(ora, M_RAND, *gs).imag).max()
    print(f"O({opdim}): max|C_td| {mtd}, max|C_eq| {meq}, max|Im W(M_RAND)| {im:.3e}")
    assert min(mtd) >= 0.15 and min(meq) >= 0.47
    assert 5e-3 <= im <= 0.13


def test_correlation_ratio_picks_the_columns():
    L = 4
    s = np.arange(L * L, dtype=float) + 1.0
    assert correlation_ratio(s, L, 2, 2) == 1.0 - 0.5 * (s[2 * L + 3] + s[3 * L + 2]) / s[2 * L + 2]
    assert correlation_ratio(s, L, 3, 1) == 1.0 - 0.5 * (s[1 * L + 0] + s[2 * L + 3]) / s[1 * L + 3]


def test_library_and_python_layer_carry_the_entry_points():
    from detqmc_amd import KernelContext, _lib, model
    lib = _lib.load()
    for sym in ("dqmc_set_custom_bilinears", "dqmc_get_custom_bilinears", "dqmc_measure_timedisplaced_custom", "dqmc_measure_td_custom_accum_size",
                "dqmc_measure_td_custom_read_host", "dqmc_set_equal_time_custom", "dqmc_measure_eq_custom_accum_size",
                "dqmc_measure_eq_custom_read_host", "dqmc_series_custom_derived_host"):
        assert hasattr(lib, sym), sym
    # what can be refused without a context is refused, and nothing is read or written
    m = np.ascontiguousarray(M_NX)
    n = C.c_int(5)
    out = np.zeros(4)
    dp = out.ctypes.data_as(_lib._DP)
    assert lib.dqmc_set_custom_bilinears(None, 1, m.ctypes.data) == -1 and lib.dqmc_get_custom_bilinears(None, C.byref(n), None) == -1 and n.value == 5
    assert lib.dqmc_measure_timedisplaced_custom(None, 1) == -1 and lib.dqmc_set_equal_time_custom(None, 1) == -1
    assert lib.dqmc_measure_td_custom_accum_size(None) == 0 and lib.dqmc_measure_eq_custom_accum_size(None) == 0
    assert lib.dqmc_measure_td_custom_read_host(None, dp) == -1 and lib.dqmc_measure_eq_custom_read_host(None, dp) == -1
    assert lib.dqmc_series_custom_derived_host(None, 0, 0, dp, dp) == -1 and not out.any()
    # no struct changes: the matrices are run-time state of a context
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264 and C.sizeof(_lib.dqmc_series_state) == 56
    assert (_lib.DQMC_CUSTOM_MAX, _lib.DQMC_SERIES_MATS_CUSTOM, _lib.DQMC_SERIES_EQ_CUSTOM) == (4, 512, 1024)
    assert (model.SERIES_MATS_CUSTOM, model.SERIES_EQ_CUSTOM) == (512, 1024) and model.SERIES_EQ_BAND == 256
    for name in ("set_custom_bilinears", "get_custom_bilinears", "measure_timedisplaced_custom", "measure_td_custom_read", "set_equal_time_custom",
                 "measure_eq_custom_read", "series_custom_derived"):
        assert callable(getattr(KernelContext, name)), name
    a = model._custom_matrices([M_NX, M_RAND.T])                          # any layout in, C-contiguous (count, 4, 4) out
    assert a.shape == (2, 4, 4) and a.flags.c_contiguous and a.dtype == np.complex128 and np.array_equal(a[1], M_RAND.T)
    assert model._custom_matrices([]).shape == (0, 4, 4)


def test_python_name_parsing():
    """every name of the custom observables maps to the index the host header gives it, every other name is rejected"""
    import os
    import re

    from conftest import ROOT
    from detqmc_amd import model
    hdr = open(os.path.join(ROOT, "include", "detsdw_host.h")).read()
    base = {kind: int(re.search(rf"\b{macro}\s*=\s*(\d+)", hdr).group(1))
            for kind, macro in (("Tau", "DETSDW_OBS_CUSTOMTAU"), ("TauQ0", "DETSDW_OBS_CUSTOMTAU_Q0"), ("Corr", "DETSDW_OBS_CUSTOMCORR"),
                                ("Sq", "DETSDW_OBS_CUSTOMSQ"))}
    assert base == {"Tau": 42, "TauQ0": 46, "Corr": 50, "Sq": 54} == model.CUSTOM_OBS_BASE
    seen = set()
    for kind, b in base.items():
        for c in range(4):
            assert model.custom_observable(f"custom{c}{kind}") == (kind, b + c), (kind, c)
            seen.add(b + c)
    assert seen == set(range(42, 58))                                      # sixteen distinct indices right behind bandMixSq = 41
    assert max(list(model.MATSUBARA.values()) + list(model.EQ_CORRELATORS.values()) + list(model.BAND_EQ_CORRELATORS.values())
               + list(model.SERIES_PHI_OBS.values())) == 41
    for bad in ("customXTau", "custom4Tau", "custom-1Tau", "custom0Foo", "custom0", "custom0tau", "custom0TauFine", "custom00Tau", "Custom0Tau",
                "custom0Tau ", "xcustom0Tau", "bandDiffTau", "chargeCorr", ""):
        assert model.custom_observable(bad) is None, bad
    # the Matsubara readers take the Tau kind alone, next to the fixed names
    assert [model._matsubara_index(f"custom{c}Tau") for c in range(4)] == [42, 43, 44, 45]
    assert model._matsubara_index("chargeTau") == 10 and model._matsubara_index("bandMixTau") == 35
    for bad in ("custom2Corr", "custom2Sq", "custom2TauQ0", "custom4Tau", "chargeCorr"):
        with pytest.raises(KeyError):
            model._matsubara_index(bad)
    # the derived quantity
    assert [model.custom_ratio(f"R_custom{c}") for c in range(4)] == [0, 1, 2, 3]
    for bad in ("R_custom4", "R_custom", "R_custom01", "R_customX", "r_custom0", "R_custom0 ", "R_charge", "R_dCDW", "custom0Sq"):
        assert model.custom_ratio(bad) is None, bad
    assert not any(k.startswith("R_custom") for k in model.SERIES_DERIVED)     # no second route to the same name
