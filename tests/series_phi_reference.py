"""Direct-sum numpy reference of the order-parameter part of the measurement series (DQMC_SERIES_PHI, include/dqmc_hip.h).  Deliberately
plain: one explicit phase array per (n, q), no FFT, no code shared with detqmc_amd (its phi_sample is one of the things tested against
this file).

What is restated, from the reference implementation's offline tools:
  computeCorrelations_fft (src/mainsdwcorr.cpp:457-507): per component d a temporal transform with sign +1 normalised by m (:471-483),
      a spatial one with sign -1 normalised by N (:485-492), and corr_ft += |phi_ft|^2 summed over d (:495-497).  The time index there
      runs over the m stored slices; here it is k = 1 .. m, which changes A_d by the phase e^{i 2 pi n / m} and |A_d|^2 not at all.
  computePhiSusceptibilityEqualTime (src/mainsdweqtimesusc.cpp:188-203): (N / m) sum_k sum_d ((1/N) sum_r phi_d(r, k))^2.
  binderObservable / binderRatioObservable (src/mrpt-jk.cpp:584-587): 1 - <m^4> / (3 <m^2>^2) and <m^4> / <m^2>^2.
Fields are (m+1, N, opdim) with site r = y L + x; slice 0 is never read."""
import numpy as np


def chi_direct(phi, L, nfreq):
    """chi[n][qy L + qx] = sum_d |(1/K) sum_k sum_r phi_d(r, k) exp(i 2 pi n k / m - i 2 pi (qx x + qy y) / L)|^2, K = m N"""
    phi = np.asarray(phi, dtype=np.float64)
    m, N, opdim = phi.shape[0] - 1, phi.shape[1], phi.shape[2]
    assert N == L * L and 1 <= nfreq <= m
    f = phi[1:]                                             # [k - 1][r][d]
    k = np.arange(1, m + 1)[:, None]
    x, y = (np.arange(N) % L)[None, :], (np.arange(N) // L)[None, :]
    chi = np.zeros((nfreq, N))
    for n in range(nfreq):
        for qy in range(L):
            for qx in range(L):
                phase = np.exp(1j * (2.0 * np.pi * n * k / m - 2.0 * np.pi * (qx * x + qy * y) / L))      # [k][r]
                a = (phase[:, :, None] * f).sum(axis=(0, 1)) / (m * N)
                chi[n, qy * L + qx] = (np.abs(a) ** 2).sum()
    return chi


def scalars_direct(phi, L, chi00):
    """(|phibar|, |phibar|^2, |phibar|^4, equal-time susceptibility, associatedEnergy); |phibar|^2 = chi(0, 0) is handed in"""
    phi = np.asarray(phi, dtype=np.float64)
    m, N = phi.shape[0] - 1, phi.shape[1]
    f = phi[1:]
    eqt = 0.0
    for kk in range(m):
        mag = f[kk].sum(axis=0) / N                         # [d]
        eqt += float(np.dot(mag, mag))
    eqt *= N / m
    return np.array([np.sqrt(chi00), chi00, chi00 * chi00, eqt, (f * f).sum() / (2.0 * N * m)])


def sample_direct(phi, L, nfreq):
    """the part as it sits in a sample row: chi [nfreq][N] flattened, then the five scalars"""
    chi = chi_direct(phi, L, nfreq)
    return np.concatenate([chi.ravel(), scalars_direct(phi, L, chi[0, 0])])


def plane_wave(L, m, opdim, n0, q0):
    """phi_d(r, k) = cos(2 pi n0 k / m - 2 pi (q0x x + q0y y) / L) for every d, slice 0 zero: (m+1, N, opdim)"""
    N = L * L
    k = np.arange(m + 1)[:, None]
    x, y = (np.arange(N) % L)[None, :], (np.arange(N) // L)[None, :]
    w = np.cos(2.0 * np.pi * n0 * k / m - 2.0 * np.pi * (q0[0] * x + q0[1] * y) / L)
    w[0] = 0.0
    return np.repeat(w[:, :, None], opdim, axis=2)


def derived_functions(L, N, beta, nfreq):
    """the six functions of one part vector x (chi [nfreq][N] then the scalars) of dqmc_series_phi_derived_host, in its order"""
    sc = nfreq * N

    def binder(x):
        return 1.0 - x[sc + 2] / (3.0 * x[sc + 1] * x[sc + 1])

    def binder_ratio(x):
        return x[sc + 2] / (x[sc + 1] * x[sc + 1])

    def chi_phi(x):
        return beta * N * x[sc + 1]

    def chi_phi_connected(x):
        return beta * N * (x[sc + 1] - x[sc] * x[sc])

    def r_phi(x):
        return 1.0 - 0.5 * (x[1] + x[L]) / x[0]

    def xi_phi(x):
        arg = x[0] / (0.5 * (x[1] + x[L])) - 1.0
        return np.sqrt(arg) / (2.0 * np.sin(np.pi / L)) if arg >= 0.0 else np.nan

    return [binder, binder_ratio, chi_phi, chi_phi_connected, r_phi, xi_phi]


def rounding_bound(opdim, m, N, a):
    """4 opdim (K + 64) eps a^2, K = m N, a = max |phi|: the bound on |device - reference| of one chi element or quadratic scalar.
    Derivation: A_d is a K-term sum of products phi * phase with |phi| <= a, |phase| <= 1, divided by K; summed in any order with
    phases from a table good to a few eps, its error is at most (K + 64) eps a (K - 1 additions, and the 64 covers the products, the
    table, the two spatial stages and the division), and |A_d| <= a.  Then | |A_d + dA_d|^2 - |A_d|^2 | <= 2 a (K + 64) eps a to first
    order, the sum over d gives opdim of them, and the factor 2 on top is for the rounding of the numpy reference itself."""
    return 4.0 * opdim * (m * N + 64.0) * 2.0 ** -52 * a * a
