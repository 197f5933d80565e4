"""TEST INFRASTRUCTURE ONLY.  Numpy side of the Hubbard replica's every-slice tau grid (DQMC_TD_HUB_EVERY_SLICE): the eight
displaced channels, the slice coverage rule, the float64 single-slice propagation of (G(tau,0), G(0,tau), G(tau)) per spin with its
error e_ref against direct inverses (displaced_greens below: hubbard_corr_reference.displaced_greens with a stable G(0,tau)), and the fermionic transform G_s(k, i omega_n).

Conventions: those of tests/hubbard_corr_reference.py; Bs = [B_1, .., B_m] of one spin."""
import functools

import numpy as np

import hubbard_corr_reference as R
import td_matsubara_reference as M
from conftest import relerr

FINE_NAMES = R.EQ_NAMES
# (m, s): s does not divide m, n = 3 / s divides m, n = 2 / a top segment of two slices
MS_CASES = [(20, 7), (10, 5), (22, 5)]
DTAU = 0.1


def displaced_greens(Bs, l):
    """(G(tau_l,0), G(0,tau_l), G(tau_l), G(0)) of one spin by explicit products and direct inverses in extended precision:
    hubbard_corr_reference.displaced_greens with one change.  That function forms G(0,tau) = -(1 - G(0)) B(l,0)^-1 through the inverse
    of B(l,0), whose condition number grows like e^{2 tau W}: 2.9e3 at tau = 0.5, 2.6e9 at tau = 1.5, 1.7e13 at tau = 2.2 for the L = 6
    field of thermalised_oracle(6, 22, 5), where its G(0,tau) is off by 5.7e-14, 5.1e-11 and, at tau = 2.1, 7.7e-9.  It was written for
    the interior boundaries of beta = 2; the every-slice rows reach tau = beta.  Here the same quantity is formed without that inverse,
        -(1 - G(0)) B(l,0)^-1 = -[1 + B(m,0)]^-1 B(m,l) B(l,0) B(l,0)^-1 = -G(0) B(m,l).
    The other three matrices are those of the original bit for bit (tests/test_hubbard_td_fine_cpu.py checks both statements)."""
    ld = np.longdouble
    eye = np.eye(Bs[0].shape[0], dtype=ld)
    lo, hi = eye.copy(), eye.copy()
    for k in range(l):
        lo = Bs[k].astype(ld) @ lo                 # B(l, 0)
    for k in range(l, len(Bs)):
        hi = Bs[k].astype(ld) @ hi                 # B(m, l)
    g00 = R._inverse(eye + hi @ lo)
    gtt = R._inverse(eye + lo @ hi)
    return tuple(np.asarray(x, dtype=np.float64) for x in (lo @ g00, -(g00 @ hi), gtt, g00))


def td_channels(gt0, g0t, gtt, g00, L):
    """[8][N][N] in the order FINE_NAMES: the six of R.td_channels, then <Delta^f_A(tau) Delta^f+_B(0)> = 1/4 G_up(tau,0)(A, B)
    sum f_dl f_dl' G_dn(tau,0)(A + dl, B + dl') for the extended-s and the d-wave form factor"""
    six = R.td_channels(gt0, g0t, gtt, g00)
    return np.concatenate([six, np.stack([R.bond_pair(gt0[0], gt0[1], R.F_EXT_S, L), R.bond_pair(gt0[0], gt0[1], R.F_D_WAVE, L)])])


def td_corr(gt0, g0t, gtt, g00, L):
    """raw bins [8][N] of one configuration and time slice"""
    return R.bin_sum(td_channels(gt0, g0t, gtt, g00, L), L)


def segment_slices(j, m, s):
    """(slices reached upward from boundary j, in order; slices reached downward, in order)"""
    return list(range(j * s, min((j + 1) * s, m))), (list(range(s - 1, 0, -1)) if j == 1 else [])


def coverage(m, s):
    n = -(-m // s)
    hit = [0, m]
    for j in range(1, n):
        up, down = segment_slices(j, m, s)
        hit += up + down
    return sorted(hit)


def step(Bs, triple, k, direction):
    """(G(t,0), G(0,t), G(t)) of one spin from slice k to k + 1 (direction +1) or to k - 1 (-1), float64"""
    gt0, g0t, gtt = triple
    inv = np.linalg.inv
    if direction > 0:
        B = Bs[k]                                        # B_{k+1}
        return B @ gt0, g0t @ inv(B), B @ gtt @ inv(B)
    B = Bs[k - 1]                                        # B_k
    return inv(B) @ gt0, g0t @ B, inv(B) @ gtt @ B


def propagate(Bs, triple, k0, k):
    q = k0
    while q < k:
        triple = step(Bs, triple, q, +1)
        q += 1
    while q > k:
        triple = step(Bs, triple, q, -1)
        q -= 1
    return triple


def oracle_bs(ora):
    """[spin][k - 1] = B_k of the oracle's field as it stands"""
    return [[ora.computeBmat(k, k - 1, gc) for k in range(1, ora.m + 1)] for gc in (0, 1)]


def propagation_error(ora):
    """largest max-norm relative error, over both spins, all slices of all segments and both ends, of the float64 propagation from the
    boundary's direct matrices (the ends: from G(0) by the end-row identities) against direct inverses at the slice itself"""
    m, s, n = ora.m, ora.s, ora.n
    worst = 0.0
    for Bs in oracle_bs(ora):
        for j in range(1, n):
            gt0, g0t, gtt, _ = displaced_greens(Bs, j * s)
            up, down = segment_slices(j, m, s)
            for k in up + down:
                d = displaced_greens(Bs, k)
                got = propagate(Bs, (gt0, g0t, gtt), j * s, k)
                worst = max(worst, max(relerr(a, b) for a, b in zip(got, d[:3])))
        g = displaced_greens(Bs, 0)[3]
        eye = np.eye(g.shape[0])
        for k, got in ((0, (g, g - eye, g)), (m, (eye - g, -g, g))):
            d = displaced_greens(Bs, k)
            worst = max(worst, max(relerr(a, b) for a, b in zip(got, d[:3])))
    return worst


@functools.lru_cache(maxsize=None)
def thermalised_oracle(L, m, s):
    """DetHubbardOracle after one thermalisation sweep, built once per process and left unchanged"""
    from dethubbard_oracle import DetHubbardOracle, HubbardParams as OP
    ora = DetHubbardOracle(OP(L=L, d=2, beta=m * DTAU, dtau=DTAU, s=s, t=1.0, U=4.0, mu=0.0, checkerboard=False, rngSeed=4711 + L, simindex=0))
    ora.sweepThermalization()
    return ora


@functools.lru_cache(maxsize=None)
def e_ref():
    return max(propagation_error(thermalised_oracle(L, m, s)) for L in (4, 6) for (m, s) in MS_CASES)


def fermionic_k(fine, L, dtau, nfreq):
    """G(k, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i k d} G(d, tau_k), omega_n = (2n+1) pi / beta; (m+1, N) -> (nfreq, N)"""
    fine = np.asarray(fine, dtype=np.float64)
    q = 2 * np.pi * np.arange(L) / L
    e1 = np.exp(-1j * q[:, None] * np.arange(L)[None, :])
    F = np.einsum("ab,cd->acbd", e1, e1).reshape(L * L, L * L)       # F[qy L + qx, dy L + dx]
    return M._time_sum(fine @ F.T, dtau, nfreq, True)


def transform(ch, fine, L, dtau, nfreq):
    return fermionic_k(fine, L, dtau, nfreq) if ch < 2 else M.bosonic(fine, L, dtau, nfreq)


def dispersion(L, t, mu):
    """eps_k at column ky L + kx"""
    k = 2 * np.pi * np.arange(L) / L
    return (-2.0 * t * (np.cos(k)[None, :] + np.cos(k)[:, None]) - mu).ravel()


def free_green_rows(L, t, mu, m, dtau):
    """C(d, tau_k) = (1/N) sum_k e^{i k d} e^{-tau eps_k} / (1 + e^{-beta eps_k}) of free fermions, (m+1, N): the greenUp / greenDn rows"""
    eps = dispersion(L, t, mu)
    beta = m * dtau
    gk = np.exp(-np.outer(dtau * np.arange(m + 1), eps)) / (1.0 + np.exp(-beta * eps))[None, :]
    q = 2 * np.pi * np.arange(L) / L
    e1 = np.exp(1j * np.arange(L)[:, None] * q[None, :])              # [d][k]
    Finv = np.einsum("ab,cd->acbd", e1, e1).reshape(L * L, L * L)     # [dy L + dx, ky L + kx]
    return (gk @ Finv.T).real / (L * L)


def free_green_matsubara(L, t, mu, m, dtau, nfreq):
    """the trapezoid transform of e^{-tau eps_k} / (1 + e^{-beta eps_k}) in closed form, (nfreq, N)"""
    eps = dispersion(L, t, mu)
    omega = M.frequencies(m, dtau, nfreq, True)
    return M.closed_form(-eps[None, :], omega[:, None], dtau, m) / (1.0 + np.exp(-m * dtau * eps))[None, :]
