"""numpy reference of the band-resolved charge correlators bandDiff and bandMix (tests only).

Two spin-singlet bilinears of the two-band model in the band-spin order XUP, YDOWN, XDOWN, YUP:

    M_BAND = diag(+1, -1, +1, -1)                       n_x - n_y: nematic at q = 0, d-wave charge-density wave at q = (pi, pi)
    M_MIX: (0,3) = (3,0) = (1,2) = (2,1) = +1           sum_s psi^+_xs psi_ys + h.c.

Everything is built on the general Wick form of tests/td_ph_reference.py (imported, not restated): time-displaced from the four shifted
matrices of a boundary, equal-time from one matrix in every role (tests/eq_corr_reference.py), where the delta term of M^2 = 1 is
tr_4 g(B; B) in the d = 0 bin."""
import numpy as np

from eq_corr_reference import wick_eq
from td_ph_reference import bin_periodic, expand, one_body, wick

M_BAND = np.diag([1.0, -1.0, 1.0, -1.0]).astype(complex)
M_MIX = np.zeros((4, 4), dtype=complex)
M_MIX[0, 3] = M_MIX[3, 0] = M_MIX[1, 2] = M_MIX[2, 1] = 1.0
BAND_MS = (M_BAND, M_MIX)
NAMES = ("bandDiff", "bandMix")


def band_correlators(ora, gtt_s, gt0_s, g0t_s, g00_s):
    """(bandDiff, bandMix), each of length N, from the four SHIFTED engine matrices"""
    full = [expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)]
    return tuple(bin_periodic(wick(*full, M, ora.N), ora.L) for M in BAND_MS)


def connected_part(ora, M, gtt_s, gt0_s, g0t_s, g00_s):
    """sum_abcd M_ab M_cd g0t(B d; A a) gt0(A b; B c), N x N, entry (A, B): the disconnected product minus W"""
    full = [expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)]
    return np.outer(one_body(full[0], M, ora.N), one_body(full[3], M, ora.N)) - wick(*full, M, ora.N)


def band_one_body(ora, g_s):
    """(o^M_BAND(A), o^M_MIX(A)), complex of length N each, of one shifted equal-time engine matrix"""
    full = expand(ora, g_s)
    return tuple(one_body(full, M, ora.N) for M in BAND_MS)


def eq_band_correlators(ora, gs):
    """(bandDiff, bandMix), each of length N, from ONE shifted engine matrix in every role, the delta term included"""
    full = expand(ora, gs)
    return tuple(bin_periodic(wick_eq(full, M, ora.N), ora.L) for M in BAND_MS)


def eq_band_delta(ora, gs):
    """what the delta term adds to the d = 0 bin of C(d), for either matrix (M^2 = 1): (1/N) Re tr gs over all four flavours"""
    return float(np.trace(expand(ora, gs)).real) / ora.N


def correlation_ratios(sq_band, sq_mix, L):
    """(R_dCDW, R_nematic, R_bandMix) from the structure factors S(q), last axis qy L + qx: R = 1 - (S(Q + dx) + S(Q + dy)) / (2 S(Q))
    for bandDiff at Q = (L/2, L/2), bandDiff at Q = (0, 0) and bandMix at Q = (L/2, L/2)"""
    def ratio(s, Q):
        s = np.asarray(s)
        q1 = (Q + 1) % L
        return 1.0 - 0.5 * (s[..., Q * L + q1] + s[..., q1 * L + Q]) / s[..., Q * L + Q]
    return ratio(sq_band, L // 2), ratio(sq_band, 0), ratio(sq_mix, L // 2)
