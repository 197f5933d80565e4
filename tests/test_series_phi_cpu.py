"""detqmc_amd.phi_sample, the numpy restatement of the order-parameter part of a series sample (DQMC_SERIES_PHI), against the direct sum
of tests/series_phi_reference.py, against np.fft with the sign and index mapping written out, on a plane wave and on Parseval's
identity; and the six derived functions on synthetic bins against detqmc_amd.jackknife.  No GPU."""
import numpy as np
import pytest

import series_phi_reference as spr
from detqmc_amd import jackknife, phi_sample


def _field(seed, L, m, opdim, amp=1.5):
    phi = np.random.default_rng(seed).uniform(-amp, amp, (m + 1, L * L, opdim))
    phi[0] = 7.0                                            # slice 0 is never read: a value that would show
    return phi


@pytest.mark.parametrize("opdim,L,m,nfreq", [(1, 4, 10, 3), (3, 6, 7, 7), (2, 5, 4, 1)])
def test_phi_sample_agrees_with_the_direct_sum_and_with_fft(opdim, L, m, nfreq):
    phi = _field(100 * L + m, L, m, opdim)
    N = L * L
    chi, sc = phi_sample(phi, L, nfreq)
    assert chi.shape == (nfreq, N) and sc.shape == (5,)
    want = spr.sample_direct(phi, L, nfreq)
    tol = spr.rounding_bound(opdim, m, N, np.abs(phi[1:]).max())
    assert np.abs(chi.ravel() - want[:nfreq * N]).max() <= tol
    assert np.abs(sc[[1, 3, 4]] - want[nfreq * N:][[1, 3, 4]]).max() <= tol
    assert abs(sc[0] - want[nfreq * N]) <= tol / want[nfreq * N]
    assert sc[1] == chi[0, 0] and sc[0] == np.sqrt(chi[0, 0]) and sc[2] == sc[1] * sc[1]
    # np.fft: ifft along time is (1/m) sum_t f[t] e^{+2 pi i n t / m} with t = k - 1, so A carries the extra phase e^{+2 pi i n / m} of
    # k = t + 1; fft2 over (y, x) is sum e^{-2 pi i (qy y + qx x) / L}, to be divided by N.  Output index [n][qy][qx] = column qy L + qx.
    f = phi[1:].reshape(m, L, L, opdim)
    a = np.fft.fft2(np.fft.ifft(f, axis=0), axes=(1, 2)) / N
    a = a * np.exp(2j * np.pi * np.arange(m) / m)[:, None, None, None]
    chi_fft = (np.abs(a) ** 2).sum(axis=3).reshape(m, N)[:nfreq]
    assert np.abs(chi - chi_fft).max() <= tol
    a_direct = np.einsum("k,kr->", np.exp(2j * np.pi * 1 * np.arange(1, m + 1) / m), phi[1:, :, 0]) / (m * N) if nfreq > 1 else None
    if a_direct is not None:                                # the phase of A itself, not only its modulus, at (n, q) = (1, 0)
        assert abs(a[1, 0, 0, 0] - a_direct) <= 1e-14 * np.abs(phi).max()


def test_phi_sample_refuses_bad_shapes():
    phi = _field(1, 4, 5, 2)
    for L, nfreq in ((3, 1), (4, 0), (4, 6)):
        with pytest.raises(ValueError):
            phi_sample(phi, L, nfreq)


def test_plane_wave_peaks_where_the_signs_say():
    L, m, n0, q0 = 6, 7, 1, (1, 2)
    N = L * L
    for opdim in (1, 3):
        chi, sc = phi_sample(spr.plane_wave(L, m, opdim, n0, q0), L, 3)
        peak = q0[1] * L + q0[0]
        assert abs(chi[n0, peak] - 0.25 * opdim) <= 1e-14
        rest = chi.copy()
        rest[n0, peak] = 0.0
        assert rest.max() <= 1e-28                          # (1e-14)^2: every other A is rounding noise
        minus = ((-q0[1]) % L) * L + (-q0[0]) % L
        transposed = q0[0] * L + q0[1]
        assert chi[n0, minus] <= 1e-28 and chi[n0, transposed] <= 1e-28
    # with every frequency in range the partner of the cosine shows up at (m - n0, -q0) and nowhere else
    chi, _ = phi_sample(spr.plane_wave(L, m, 1, n0, q0), L, m)
    assert abs(chi[m - n0, minus] - 0.25) <= 1e-14 and abs(chi.sum() - 0.5) <= 1e-13


@pytest.mark.parametrize("opdim,L,m", [(2, 4, 6), (3, 5, 3)])
def test_parseval(opdim, L, m):
    phi = _field(7 * L + m, L, m, opdim)
    N = L * L
    chi, sc = phi_sample(phi, L, m)
    assert abs(chi.sum() - 2.0 * sc[4]) <= 1e-13 * sc[4]
    assert abs(sc[3] - N * chi[:, 0].sum()) <= 1e-13 * sc[3]


def test_derived_functions_on_synthetic_bins():
    L, nfreq, beta, B = 4, 2, 1.5, 5
    N = L * L
    bins = np.zeros((B, nfreq * N + 5))
    for b in range(B):
        chi, sc = phi_sample(0.4 + (1.0 + 0.2 * b) * _field(50 + b, L, 6, 2, 0.5), L, nfreq)
        bins[b] = np.concatenate([chi.ravel(), sc])
    fs = spr.derived_functions(L, N, beta, nfreq)
    mean = bins.sum(axis=0) / B
    loo = np.array([(bins.sum(axis=0) - bins[b]) / (B - 1) for b in range(B)])
    sc0 = nfreq * N
    closed = [1.0 - mean[sc0 + 2] / (3.0 * mean[sc0 + 1] ** 2), mean[sc0 + 2] / mean[sc0 + 1] ** 2, beta * N * mean[sc0 + 1],
              beta * N * (mean[sc0 + 1] - mean[sc0] ** 2), 1.0 - 0.5 * (mean[1] + mean[L]) / mean[0],
              np.sqrt(mean[0] / (0.5 * (mean[1] + mean[L])) - 1.0) / (2.0 * np.sin(np.pi / L))]
    for e, f in enumerate(fs):
        val, err = jackknife(bins, f)
        theta = np.array([f(x) for x in loo])
        want_err = np.sqrt((B - 1) / B * ((theta - theta.mean()) ** 2).sum())
        assert np.isfinite(val) and err > 0.0, e
        assert abs(val - closed[e]) <= 1e-13 * max(1.0, abs(closed[e])), e
        assert abs(err - want_err) <= 1e-10 * want_err, e
    assert 0.0 < closed[0] < 2.0 / 3.0 + 1e-12 and closed[1] >= 1.0 - 1e-12     # <m^4> >= <m^2>^2
    # xi is NaN where chi0 < the mean of its neighbours
    x = mean.copy()
    x[0] = 0.1 * x[1]
    assert np.isnan(fs[5](x)) and np.isfinite(fs[4](x))
