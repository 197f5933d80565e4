"""numpy restatement of the Hubbard parts of the measurement series (DQMC_SERIES_HUB_*, dqmc_series_hubbard_derived_host;
include/dqmc_hip.h): the sample of one sweep from the raw blocks and the nineteen derived quantities with their jackknife errors.
Deliberately plain: explicit loops, and the jackknife and the cosine sum are those of tests/series_reference.py."""
import numpy as np

import series_reference as sr

SCALARS = ("occUp", "occDn", "occTotal", "occDouble", "localMoment", "eKinetic", "ePotential", "eTotal")
EQ = ("greenUp", "greenDn", "charge", "spinZZ", "spinXX", "pairS", "pairSx", "pairD")
TD = EQ[:6]
DERIVED = tuple("R_" + x for x in EQ) + tuple("xi_" + x for x in EQ) + ("S_spin", "R_spin", "xi_spin")


def scalars_from_block(a, N, t, U, mu):
    """part 14 from the block of the per-slice observables a[0 .. 5 + N]: the eight scalars of finishMeasurements with cnt = a[5] for the
    number of slices, then zcorr = a[6 + j] / cnt"""
    a = np.asarray(a, dtype=np.float64)
    cnt, Nf = a[5], float(N)
    occUp = 1.0 - (1.0 / (Nf * cnt)) * a[0]
    occDn = 1.0 - (1.0 / (Nf * cnt)) * a[1]
    occTotal = occUp + occDn
    occDouble = 1.0 + (1.0 / (Nf * cnt)) * (a[4] - a[0] - a[1])
    eKinetic = (t / (Nf * cnt)) * (a[2] + a[3]) - mu * occTotal
    ePotential = U * occDouble
    return np.concatenate([[occUp, occDn, occTotal, occDouble, occTotal - 2 * occDouble, eKinetic, ePotential, eKinetic + ePotential],
                           a[6:6 + N] / cnt])


def eq_sample_from_block(block, L):
    """part 15 from the block count, [8][N] raw sums: C_X(d) = sum / (double(N) count) [8][N], then S_X(q) [8][N]"""
    block = np.asarray(block, dtype=np.float64)
    N = L * L
    c = block[1:].reshape(8, N) / (float(N) * block[0])
    return np.concatenate([c.ravel(), sr.structure_factor_ref(c, L).ravel()])


def td_sample_from_block(block, L, rows):
    """part 16 from the block count[rows], [rows][6][N] raw sums: C_X(d, tau_j) = sum / (double(N) count_j) [rows][6][N], then S_X(q, tau_j)"""
    block = np.asarray(block, dtype=np.float64)
    N = L * L
    c = np.zeros((rows, 6, N))
    for j in range(rows):
        c[j] = block[rows + j * 6 * N: rows + (j + 1) * 6 * N].reshape(6, N) / (float(N) * block[j])
    return np.concatenate([c.ravel(), sr.structure_factor_ref(c, L).ravel()])


def q_points(L, Q):
    """columns of S(Q), S(Q + x), S(Q + y), indices mod L"""
    qx, qy = Q
    return [qy * L + qx, qy * L + (qx + 1) % L, ((qy + 1) % L) * L + qx]


def ratio_f(x):
    """R = 1 - Sbar / S(Q) of x = (S(Q), S(Q + x), S(Q + y)) along the leading axis; NaN where S(Q) vanishes"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x[0] != 0.0, 1.0 - 0.5 * (x[1] + x[2]) / x[0], np.nan)


def root_argument(x):
    """S(Q) / Sbar - 1, the argument of xi's root; NaN where Sbar vanishes"""
    x = np.asarray(x, dtype=np.float64)
    sbar = 0.5 * (x[1] + x[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sbar != 0.0, x[0] / sbar - 1.0, np.nan)


def xi_f(x, L):
    """xi = sqrt(S(Q) / Sbar - 1) / (2 sin(pi / L)); NaN where the argument is negative or Sbar vanishes"""
    arg = root_argument(x)
    with np.errstate(invalid="ignore"):
        return np.where(arg >= 0.0, np.sqrt(np.where(arg >= 0.0, arg, 0.0)), np.nan) / (2.0 * np.sin(np.pi / L))


def _nan_rule(value, err):
    """err is NaN where the value is (a NaN leave-one-out value has made it NaN already)"""
    return value, np.where(np.isnan(value), np.nan, err)


def triples(bins_sq, L, Q):
    """bins_sq [B][8][N] -> x [B][3][9]: S(Q), S(Q + x), S(Q + y) of the eight channels and of spin = spinZZ + 2 spinXX, bin by bin"""
    b = np.asarray(bins_sq, dtype=np.float64)
    x = b[:, :, q_points(L, Q)]                                       # [B][8][3]
    spin = x[:, 3] + 2.0 * x[:, 4]
    return np.transpose(np.concatenate([x, spin[:, None, :]], axis=1), (0, 2, 1))


def derived(bins_sq, L, Q, jack=sr.jackknife):
    """(value [19], err [19]) of dqmc_series_hubbard_derived_host for one chain from its closed bins of S_X(q), [B][8][N]"""
    x = triples(bins_sq, L, Q)
    rv, re = _nan_rule(*jack(x, ratio_f))
    xv, xe = _nan_rule(*jack(x, lambda v: xi_f(v, L)))
    sv, se = jack(x[:, 0, 8])
    return (np.concatenate([rv[:8], xv[:8], [sv, rv[8], xv[8]]]), np.concatenate([re[:8], xe[:8], [se, re[8], xe[8]]]))


def root_arguments(bins_sq, L, Q):
    """the root's argument for the mean and every leave-one-out set, [B + 1][9] (eight channels, then spin)"""
    x = triples(bins_sq, L, Q)
    B = x.shape[0]
    mean = x.sum(axis=0) / B
    return np.array([root_argument(mean)] + [root_argument((B * mean - x[b]) / (B - 1)) for b in range(B)])
