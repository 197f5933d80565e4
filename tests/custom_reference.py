"""numpy reference of the user-defined bilinear correlators (tests only).

Any Hermitian 4 x 4 matrix M in the band-spin order XUP, YDOWN, XDOWN, YUP, on the general Wick form of tests/td_ph_reference.py and its
equal-time form of tests/eq_corr_reference.py (imported, not restated).  The four matrices the tests set at once:

    M_RAND     Hermitian part of default_rng(2024) normals: dense, complex, M^2 != 1
    M_SX_BANDX sigma_x of band x, (0,2) = (2,0) = 1: couples the stored (XUP, YDOWN) sector of OPDIM < 3 to its conjugate
    M_NX       diag(1, 0, 1, 0): n_x alone, tr M != 0, M^2 = M
    M_SY_BANDY sigma_y of band y, (1,3) = i, (3,1) = -i: sector crossing and imaginary"""
import numpy as np

from eq_corr_reference import wick_eq
from td_ph_reference import bin_periodic, expand, wick


def _rand():
    rng = np.random.default_rng(2024)
    a = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
    return 0.5 * (a + a.conj().T)


M_RAND = _rand()
M_SX_BANDX = np.zeros((4, 4), dtype=complex)
M_SX_BANDX[0, 2] = M_SX_BANDX[2, 0] = 1.0
M_NX = np.diag([1.0, 0.0, 1.0, 0.0]).astype(complex)
M_SY_BANDY = np.zeros((4, 4), dtype=complex)
M_SY_BANDY[1, 3], M_SY_BANDY[3, 1] = 1j, -1j
CUSTOM_MS = (M_RAND, M_SX_BANDX, M_NX, M_SY_BANDY)


def custom_wick(ora, M, gtt_s, gt0_s, g0t_s, g00_s):
    """W^M, N x N complex, from the four SHIFTED engine matrices"""
    return wick(*[expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)], M, ora.N)


def custom_correlators(ora, Ms, gtt_s, gt0_s, g0t_s, g00_s):
    """C^M(d), length N each, for every matrix of Ms from the four SHIFTED engine matrices"""
    full = [expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)]
    return [bin_periodic(wick(*full, M, ora.N), ora.L) for M in Ms]


def eq_custom_correlators(ora, Ms, gs):
    """the same from ONE shifted engine matrix in every role, the delta term included"""
    full = expand(ora, gs)
    return [bin_periodic(wick_eq(full, M, ora.N), ora.L) for M in Ms]


def correlation_ratio(sq, L, qx, qy):
    """R = 1 - (S(Q + dx) + S(Q + dy)) / (2 S(Q)) at Q = (qx, qy); sq with last axis qy L + qx"""
    sq = np.asarray(sq)
    return 1.0 - 0.5 * (sq[..., qy * L + (qx + 1) % L] + sq[..., ((qy + 1) % L) * L + qx]) / sq[..., qy * L + qx]
