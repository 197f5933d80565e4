"""numpy restatement of the measurement series (dqmc_series_*, include/dqmc_hip.h): the sample of one sweep from the raw blocks, the
jackknife over bin means and the two derived quantities.  Deliberately plain: explicit loops over the bins, no shared code with
detqmc_amd.jackknife."""
import numpy as np

EQ_NAMES = ("charge", "spinZ", "sdw", "pairPlus", "pairMinus")


def eq_correlators_from_block(block, N):
    """C_X(d) [5, N] of one chain's equal-time block [count, 5 N raw sums]: sum / (double(N) count), one division"""
    block = np.asarray(block, dtype=np.float64)
    return block[1:].reshape(5, N) / (float(N) * block[0])


def structure_factor_ref(c, L):
    """S(q) = sum_d cos(q d) C(d), column qy L + qx, q = 2 pi (qx, qy) / L, d = (dx, dy) at index dy L + dx; the phase index is
    reduced mod L in integers; leading axes are kept"""
    c = np.asarray(c, dtype=np.float64)
    out = np.zeros_like(c)
    for qy in range(L):
        for qx in range(L):
            acc = 0.0
            for dy in range(L):
                for dx in range(L):
                    acc = acc + np.cos(2.0 * np.pi * ((qx * dx + qy * dy) % L) / L) * c[..., dy * L + dx]
            out[..., qy * L + qx] = acc
    return out


def correlation_ratio(sq, L, pairing=False):
    """R = 1 - 1/2 [S(Q + dx) + S(Q + dy)] / S(Q); Q = (L/2, L/2), or (0, 0) for the pairing channels; last axis qy L + qx"""
    sq = np.asarray(sq, dtype=np.float64)
    Q = 0 if pairing else L // 2
    Q1 = (Q + 1) % L
    return 1.0 - 0.5 * (sq[..., Q * L + Q1] + sq[..., Q1 * L + Q]) / sq[..., Q * L + Q]


def rho_s(lxx0, lyy0, L):
    """rho_s = 1/8 Re [Lxx(1,0) - Lxx(0,1) + Lyy(0,1) - Lyy(1,0)] from the frequency-0 rows (last axis qy L + qx)"""
    lxx0, lyy0 = np.asarray(lxx0), np.asarray(lyy0)
    return 0.125 * np.real(lxx0[..., 1] - lxx0[..., L] + lyy0[..., L] - lyy0[..., 1])


def jackknife(bins, f=None):
    """(value, err) over the leading axis of bins (B bin means): mean = (1/B) sum x_b, x_(b) = (B mean - x_b) / (B - 1);
    f None: value = mean, err = sqrt((B-1)/B sum (x_(b) - mean)^2); else value = f(mean), theta_(b) = f(x_(b)),
    err = sqrt((B-1)/B sum (theta_(b) - mean of theta)^2)"""
    x = np.asarray(bins, dtype=np.float64)
    B = x.shape[0]
    assert B >= 2
    mean = np.zeros(x.shape[1:])
    for b in range(B):
        mean = mean + x[b]
    mean = mean / B
    loo = [(B * mean - x[b]) / (B - 1) for b in range(B)]
    if f is None:
        acc = np.zeros(x.shape[1:])
        for b in range(B):
            acc = acc + (loo[b] - mean) ** 2
        return mean, np.sqrt((B - 1) / B * acc)
    theta = [np.asarray(f(v), dtype=np.float64) for v in loo]
    tbar = sum(theta) / B
    acc = np.zeros(np.shape(tbar))
    for b in range(B):
        acc = acc + (theta[b] - tbar) ** 2
    return np.asarray(f(mean), dtype=np.float64), np.sqrt((B - 1) / B * acc)


def jackknife_explicit(bins, f=None):
    """the same from the definition: theta_(b) = f(mean of all bins but b), recomputed from the bins that remain"""
    x = np.asarray(bins, dtype=np.float64)
    B = x.shape[0]
    f = f or (lambda v: v)
    theta = np.array([f(np.delete(x, b, axis=0).mean(axis=0)) for b in range(B)])
    return f(x.mean(axis=0)), np.sqrt((B - 1) / B * ((theta - theta.mean(axis=0)) ** 2).sum(axis=0))


def rows_close(got, ref, rel, rowlen, scale=None):
    """largest |got - ref| / (largest |scale| of its row) over rows of rowlen consecutive elements of the last axis; asserts <= rel and
    returns the figure.  scale defaults to ref"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = ref if scale is None else np.asarray(scale, dtype=np.float64)
    g, r, s = (a.reshape(-1, rowlen) for a in (got, ref, scale))
    top = np.abs(s).max(axis=1)
    assert np.all(top > 0.0), "a row of zeros: nothing to compare"
    worst = float((np.abs(g - r).max(axis=1) / top).max())
    assert worst <= rel, (worst, rel)
    return worst
