"""CPU side of the Hubbard replica's every-slice tau grid and its Matsubara transforms: the Wick forms of the two bond
channels in imaginary time against Fock-space traces (the 2 x 2 machinery of tests/test_hubbard_corr_reference_cpu.py), the float64
propagation identities against direct inverses, the transforms' references against the closed form, and the ABI.

e_ref, the largest max-norm relative error of the float64 propagation over the three (m, s) cases at L = 4 and 6, both spins, every
slice of every segment and both ends: 2.2e-12 (L = 6, (m, s) = (22, 5); 8.1e-15 at (10, 5); printed by test_propagation_reproduces_direct_inverses; 10 e_ref <= 1e-10 is asserted)."""
import ctypes as C

import numpy as np
import pytest

import hubbard_corr_reference as R
import hubbard_td_fine_reference as F
import td_matsubara_reference as M
from test_hubbard_corr_reference_cpu import L as L2, M_SLICES, _brute, system  # noqa: F401  (system: the module's fixture)

UP, DN = 0, 1


@pytest.mark.parametrize("l", [1, 2])
def test_displaced_bond_pair_wick_forms_match_fock_space_traces(system, l):
    Bs = [[system["B"][k][s] for k in range(M_SLICES)] for s in (UP, DN)]
    four = [R.displaced_greens(Bs[s], l) for s in (UP, DN)]
    gt0, g0t, gtt, g00 = ([four[s][i] for s in (UP, DN)] for i in range(4))
    ref = F.td_channels(gt0, g0t, gtt, g00, L2)
    assert ref.shape[0] == 8 and F.FINE_NAMES[6:] == ["pairSx", "pairD"]
    brute = _brute(system, F.FINE_NAMES, l)
    for ci, name in enumerate(F.FINE_NAMES):
        assert np.max(np.abs(ref[ci] - brute[ci])) < 1e-10, name
    assert np.max(np.abs(F.td_corr(gt0, g0t, gtt, g00, L2) - R.bin_sum(brute, L2))) < 1e-10
    assert np.array_equal(ref[:6], R.td_channels(gt0, g0t, gtt, g00))


def test_direct_reference_is_the_correlator_tests_reference_with_a_stable_g0t():
    """F.displaced_greens against R.displaced_greens: three matrices bit for bit at every slice; G(0,tau) to 1e-12 while B(tau,0) is well
    conditioned (tau <= 0.5), and the figures of the helper's docstring beyond"""
    ora = F.thermalised_oracle(6, 22, 5)
    Bs = F.oracle_bs(ora)[0]
    for l in range(ora.m + 1):
        a, b = F.displaced_greens(Bs, l), R.displaced_greens(Bs, l)
        for i in (0, 2, 3):
            assert np.array_equal(a[i], b[i]), (l, i)
        e = np.max(np.abs(a[1] - b[1])) / np.max(np.abs(a[1]))
        if l in (0, 5, 10, 15, 20, 21, 22):
            print(f"l {l}: G(0,tau) of the two forms differs by {e:.1e}")
        if l <= 5:
            assert e < 1e-12, (l, e)
    # small well-conditioned matrices, where both forms are exact: they agree to rounding
    rng = np.random.default_rng(5)
    small = [np.eye(4) + 0.3 * rng.standard_normal((4, 4)) for _ in range(3)]
    for l in range(4):
        for x, y in zip(F.displaced_greens(small, l), R.displaced_greens(small, l)):
            assert np.max(np.abs(x - y)) < 1e-14


@pytest.mark.parametrize("m,s", F.MS_CASES)
def test_every_slice_is_hit_exactly_once(m, s):
    assert F.coverage(m, s) == list(range(m + 1))


def test_propagation_reproduces_direct_inverses():
    worst = 0.0
    for L in (4, 6):
        for m, s in F.MS_CASES:
            e = F.propagation_error(F.thermalised_oracle(L, m, s))
            print(f"L {L} (m, s) = ({m}, {s}): e_ref {e:.2e}")
            worst = max(worst, e)
    print(f"e_ref = {worst:.2e}")
    assert worst == F.e_ref()
    assert 10 * worst <= 1e-10


@pytest.mark.parametrize("L,m", [(4, 20), (6, 22)])
def test_transform_references(L, m):
    rng = np.random.default_rng(7 + L)
    fine = rng.standard_normal((m + 1, L * L))
    for nfreq in (1, 3, 9, m):
        # the fermionic reference is the spatial sum with e^{-i k d} followed by the fermionic time sum
        got = F.fermionic_k(fine, L, F.DTAU, nfreq)
        x, y = np.arange(L * L) % L, np.arange(L * L) // L
        ph = np.exp(-2j * np.pi * (np.outer(x, x) + np.outer(y, y)) / L)        # [k][d]
        gk = fine @ ph.T                                                         # G(k, tau_k), complex; M.fermionic takes real rows
        want = M.fermionic(gk.real, F.DTAU, nfreq) + 1j * M.fermionic(gk.imag, F.DTAU, nfreq)
        assert np.allclose(got, want, rtol=0, atol=1e-12 * np.abs(got).max())
        # the bosonic one differs from it in the frequencies alone
        assert F.transform(2, fine, L, F.DTAU, nfreq).shape == (nfreq, L * L)
    # free dispersion: the rows transform to the closed form
    mu = -0.5
    rows = F.free_green_rows(L, 1.0, mu, m, F.DTAU)
    for nfreq in (1, 3, 9, m):
        got, want = F.fermionic_k(rows, L, F.DTAU, nfreq), F.free_green_matsubara(L, 1.0, mu, m, F.DTAU, nfreq)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), nfreq
    assert np.allclose(M.frequencies(m, F.DTAU, 3, True), (2 * np.arange(3) + 1) * np.pi / (m * F.DTAU), rtol=1e-15)


def test_abi_symbols_constants_and_struct_sizes():
    from detqmc_amd import _lib
    lib = _lib.load()
    assert _lib.DQMC_TD_HUB_EVERY_SLICE == 0x400 and _lib.DETHUBBARD_MEASURE_TD_FINE == 4
    assert (C.sizeof(_lib.dqmc_params), C.sizeof(_lib.detsdw_params), C.sizeof(_lib.dethubbard_params), C.sizeof(_lib.dqmc_series_state)) == (192, 264, 80, 56)
    buf = np.zeros(16)
    dp = buf.ctypes.data_as(_lib._DP)
    assert lib.dqmc_hubbard_measure_timedisplaced_segment(None, 1) == -1 and b"null" in lib.dqmc_last_error()
    assert lib.dqmc_hubbard_measure_timedisplaced_ends(None) == -1
    assert lib.dqmc_hubbard_td_fine_accum_size(None) == 0 and lib.dqmc_hubbard_td_matsubara_size(None, 1) == 0
    assert lib.dqmc_hubbard_td_fine_counts_host(None, dp) == -1
    assert lib.dqmc_hubbard_td_fine_read_host(None, dp) == -1 and lib.dqmc_hubbard_td_matsubara_host(None, 1, dp) == -1
    assert lib.dethubbard_get_td_fine_correlators(None, dp) == -1 and b"null" in lib.dethubbard_last_error()
    assert lib.dethubbard_get_matsubara(None, 1, dp) == -1 and lib.dethubbard_get_matsubara_all(None, 1, dp) == -1
    assert np.all(buf == 0.0)


@pytest.mark.parametrize("eq,word", [(False, 6), (True, 7)])
def test_every_slice_parameter_reaches_dethubbard_create(eq, word):
    import detqmc_amd
    from detqmc_amd import DetHubbard, DqmcError, HubbardParams, _lib
    seen = {}

    class _Spy:                                          # the loaded library with dethubbard_create replaced by a recorder
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def dethubbard_create(self, p, nchains, out):
            seen["flags"] = C.cast(p, C.POINTER(_lib.dethubbard_params)).contents.measureFlags
            return -1

    real = detqmc_amd.model.load
    detqmc_amd.model.load = lambda: _Spy(real())
    try:
        with pytest.raises(DqmcError):
            DetHubbard(HubbardParams(L=4, beta=2.0, equalTimeCorrelators=eq, timeDisplacedCorrelators=True, timeDisplacedEverySlice=True))
    finally:
        detqmc_amd.model.load = real
    assert seen["flags"] == word
