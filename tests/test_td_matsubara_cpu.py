"""CPU checks of the Matsubara transforms: the numpy restatement (tests/td_matsubara_reference.py) against the closed form of a single
site, superfluid_stiffness on synthetic arrays, and the new entry points of the built library (exported, bound, loud on a null handle)."""
import ctypes as C
import os

import numpy as np
import pytest

import td_matsubara_reference as tm


@pytest.fixture(scope="module")
def lib():
    import detqmc_amd
    if not os.path.exists(detqmc_amd.LIB_PATH):
        from detqmc_amd.build import build
        build(verbose=False)
    return detqmc_amd.load()


@pytest.mark.parametrize("m", [10, 7])
def test_reference_against_the_closed_form_of_a_single_site(m):
    """C(d, tau) = delta(d, d0) e^{a tau}: the transform is the trapezoid sum of a geometric series times e^{-i q d0}"""
    L, dtau, a, nfreq = 4, 0.1, -0.7, m
    d0x, d0y = 3, 1
    fine = np.zeros((m + 1, L * L))
    fine[:, d0y * L + d0x] = np.exp(a * dtau * np.arange(m + 1))
    chi = tm.bosonic(fine, L, dtau, nfreq)
    g = tm.fermionic(fine, dtau, nfreq)
    assert chi.shape == g.shape == (nfreq, L * L)
    worst = 0.0
    for n in range(nfreq):
        cb = tm.closed_form(a, 2 * np.pi * n / (m * dtau), dtau, m)
        cf = tm.closed_form(a, (2 * n + 1) * np.pi / (m * dtau), dtau, m)
        for qy in range(L):
            for qx in range(L):
                ref = cb * np.exp(-2j * np.pi * (qx * d0x + qy * d0y) / L)
                worst = max(worst, abs(chi[n, qy * L + qx] - ref))
        ref = np.zeros(L * L, dtype=complex)
        ref[d0y * L + d0x] = cf
        worst = max(worst, np.abs(g[n] - ref).max())
    print(f"m = {m}: largest absolute deviation from the closed form {worst:.2e} (values of order {dtau * m:.1f})")
    assert worst < 1e-13


def test_frequencies_and_weights():
    assert np.array_equal(tm.weights(3), [0.5, 1.0, 1.0, 0.5])
    assert np.allclose(tm.frequencies(10, 0.1, 3, False), [0.0, 2 * np.pi, 4 * np.pi], rtol=1e-15)
    assert np.allclose(tm.frequencies(10, 0.1, 2, True), [np.pi, 3 * np.pi], rtol=1e-15)


def test_superfluid_stiffness_on_synthetic_arrays():
    from detqmc_amd import superfluid_stiffness
    L, nfreq = 4, 3
    rng = np.random.default_rng(7)
    xx = rng.normal(size=(nfreq, L * L)) + 1j * rng.normal(size=(nfreq, L * L))
    yy = rng.normal(size=(nfreq, L * L)) + 1j * rng.normal(size=(nfreq, L * L))
    want = 0.125 * (xx[0, 1] - xx[0, L] + yy[0, L] - yy[0, 1]).real      # q = (1, 0) -> column 1, q = (0, 1) -> column L
    assert superfluid_stiffness(xx, yy, L) == want
    # only the zero-frequency row and the two smallest q enter
    xx2, yy2 = xx.copy(), yy.copy()
    xx2[1:] = 0.0; yy2[1:] = 0.0
    keep = np.zeros(L * L, dtype=bool); keep[[1, L]] = True
    xx2[:, ~keep] = 0.0; yy2[:, ~keep] = 0.0
    assert superfluid_stiffness(xx2, yy2, L) == want
    # a longitudinal-only response Lxx(q) = a qx^2 / |q|^2, Lyy(q) = a qy^2 / |q|^2: rho_s = a / 4
    a = 1.7
    lx, ly = np.zeros((1, L * L)), np.zeros((1, L * L))
    for qy in range(L):
        for qx in range(L):
            if qx or qy:
                lx[0, qy * L + qx] = a * qx * qx / (qx * qx + qy * qy)
                ly[0, qy * L + qx] = a * qy * qy / (qx * qx + qy * qy)
    assert abs(superfluid_stiffness(lx, ly, L) - a / 4) < 1e-15
    # leading (chain) axes are kept
    batch = superfluid_stiffness(np.stack([xx, 2 * xx]), np.stack([yy, 2 * yy]), L)
    assert batch.shape == (2,) and batch[0] == want and batch[1] == 2 * want


def test_new_symbols_resolve_and_reject_null_handles(lib):
    from detqmc_amd._lib import SYMBOLS
    bound = {s[0] for s in SYMBOLS}
    for nm in ("dqmc_measure_td_matsubara_host", "dqmc_measure_td_matsubara_size", "detsdw_get_matsubara", "detsdw_get_matsubara_all"):
        assert hasattr(lib, nm) and nm in bound, nm
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.detsdw_get_matsubara(None, 6, 1, p) == -1
    assert b"null" in lib.detsdw_last_error()
    assert lib.detsdw_get_matsubara_all(None, 6, 1, p) == -1
    assert lib.dqmc_measure_td_matsubara_host(None, 1, 1, p) == -1
    assert lib.dqmc_measure_td_matsubara_size(None, 1, 1) == 0
    assert not buf.any()


def test_fine_on_device_needs_every_slice():
    """the parameter check runs before any device is touched"""
    import detqmc_amd
    from detqmc_amd import DqmcError, SDWParams
    from detqmc_amd._lib import DETSDW_TD_FINE_ON_DEVICE
    assert DETSDW_TD_FINE_ON_DEVICE == 0x200
    assert SDWParams().timeDisplacedFineOnDevice is False
    with pytest.raises(DqmcError) as e:
        detqmc_amd.DetSDW(SDWParams(L=4, beta=1.0, fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedFineOnDevice=True))
    assert e.value.code == -1 and "timeDisplacedFineOnDevice" in str(e.value)
