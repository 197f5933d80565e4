"""numpy restatement of the Matsubara transforms of the every-slice observables (include/detsdw_host.h, detsdw_get_matsubara).

Input: the '...Fine' arrays of DetSDW.observable_vector, shape (m+1, N): row k = tau_k = k dtau, k = 0 .. m.  Trapezoid weights over the
closed grid, w_0 = w_m = 1/2.

  bosonic(fine, L, dtau, nfreq)    chi(q, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i q d} C(d, tau_k),  omega_n = 2 pi n / beta,
                                   column d = dy L + dx in, column qy L + qx out, q = (2 pi / L)(qx, qy)
  fermionic(fine, dtau, nfreq)     G(k, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} G(k, tau_k),  omega_n = (2n+1) pi / beta, columns unchanged
"""
import numpy as np

FERMIONIC = ("greenKTauX", "greenKTauY")
BOSONIC = ("pairPlusTau", "pairMinusTau", "chargeTau", "spinZTau", "sdwTau", "currentXTau", "currentYTau")


def weights(m):
    w = np.ones(m + 1)
    w[0] = w[m] = 0.5
    return w


def frequencies(m, dtau, nfreq, fermionic):
    n = np.arange(nfreq)
    return ((2 * n + 1) if fermionic else 2 * n) * np.pi / (m * dtau)


def _time_sum(rows, dtau, nfreq, fermionic):
    m = rows.shape[0] - 1
    tau = dtau * np.arange(m + 1)
    omega = frequencies(m, dtau, nfreq, fermionic)
    return dtau * (weights(m)[None, :] * np.exp(1j * omega[:, None] * tau[None, :])) @ rows


def bosonic(fine, L, dtau, nfreq):
    fine = np.asarray(fine, dtype=np.float64)
    assert fine.shape[1] == L * L
    q = 2 * np.pi * np.arange(L) / L
    d = np.arange(L)
    e1 = np.exp(-1j * q[:, None] * d[None, :])                  # [q][d] along one direction
    # F[qy L + qx, dy L + dx] = e^{-i (qx dx + qy dy)}
    F = np.einsum("ab,cd->acbd", e1, e1).reshape(L * L, L * L)   # (qy, qx, dy, dx)
    return _time_sum(fine @ F.T, dtau, nfreq, False)


def fermionic(fine, dtau, nfreq):
    return _time_sum(np.asarray(fine, dtype=np.float64).astype(np.complex128), dtau, nfreq, True)


def transform(name, fine, L, dtau, nfreq):
    return fermionic(fine, dtau, nfreq) if name in FERMIONIC else bosonic(fine, L, dtau, nfreq)


def closed_form(a, omega, dtau, m):
    """dtau sum_k w_k e^{(a + i omega) k dtau}: the trapezoid sum of e^{a tau} e^{i omega tau}, a geometric series minus half its ends"""
    z = np.exp((a + 1j * omega) * dtau)
    return dtau * ((z ** (m + 1) - 1) / (z - 1) - (1 + z ** m) / 2)
