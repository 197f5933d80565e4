"""numpy restatement of the measurement series over a long run (dqmc_series_rebin, DQMC_SERIES_AUTO_REBIN, DQMC_SERIES_TRACK_VARIANCE,
dqmc_series_binning_host; include/dqmc_hip.h).  Deliberately plain: explicit loops over bins, levels and sweeps, and no code shared with
detqmc_amd (its binning_analysis is one of the things tested against this file)."""
import numpy as np


def rebinned(bins):
    """bins[B][...] with B even -> [B/2][...]: out[k] = (bins[2k] + bins[2k+1]) * 0.5, two IEEE operations"""
    bins = np.asarray(bins, dtype=np.float64)
    B = bins.shape[0]
    if B % 2:
        raise ValueError("an odd number of bins cannot be merged")
    out = np.zeros((B // 2,) + bins.shape[1:])
    for k in range(B // 2):
        out[k] = (bins[2 * k] + bins[2 * k + 1]) * 0.5
    return out


def jackknife_err(y):
    """err of dqmc_series_stats_host over the leading axis, in index order"""
    B = y.shape[0]
    assert B >= 2
    total = np.zeros(y.shape[1:])
    for b in range(B):
        total = total + y[b]
    mean = total / B
    tot = B * mean
    acc = np.zeros(y.shape[1:])
    for b in range(B):
        d = (tot - y[b]) / (B - 1) - mean
        acc = acc + d * d
    return np.sqrt((B - 1) / B * acc)


def cascade(bins, levels):
    """[y^0, ..., y^(levels-1)]: y^0 = bins, y^l = the first 2 (B_(l-1) // 2) bins of y^(l-1) merged in pairs; B_l = B >> l"""
    y = np.asarray(bins, dtype=np.float64)
    out = [y]
    for _ in range(1, levels):
        half = y.shape[0] // 2
        y = rebinned(y[:2 * half])
        out.append(y)
    return out


def binning(bins, bin_size, levels, m2=None, samples=None):
    """err[levels][...] and, with m2 and samples, tau[levels][...] = 1/2 err_l^2 (B_l 2^l bin_size) / sigma^2, sigma^2 = m2 / (samples - 1),
    NaN where sigma^2 is not > 0; without them tau is None"""
    ys = cascade(bins, levels)
    if ys[-1].shape[0] < 2:
        raise ValueError("the top level needs at least two merged bins")
    err = np.array([jackknife_err(y) for y in ys])
    if m2 is None:
        return err, None
    var = np.asarray(m2, dtype=np.float64) / (samples - 1)
    tau = np.full(err.shape, np.nan)
    ok = var > 0
    for l, y in enumerate(ys):
        t = 0.5 * err[l] * err[l] * (float(y.shape[0]) * float(2 ** l) * float(bin_size))
        tau[l][ok] = t[ok] / var[ok]
    return err, tau


def two_pass(samples):
    """(mean, sum of (x - mean)^2) over the leading axis: the mean first, then the deviations from it"""
    x = np.asarray(samples, dtype=np.float64)
    n = x.shape[0]
    total = np.zeros(x.shape[1:])
    for i in range(n):
        total = total + x[i]
    mean = total / n
    m2 = np.zeros(x.shape[1:])
    for i in range(n):
        m2 = m2 + (x[i] - mean) ** 2
    return mean, m2


def welford(samples):
    """(w, m2) of Welford's recurrence in the order of the kernel: n += 1; d = x - w; w += d / n; m2 += d (x - w)"""
    x = np.asarray(samples, dtype=np.float64)
    w, m2 = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for i in range(x.shape[0]):
        d = x[i] - w
        w = w + d / float(i + 1)
        m2 = m2 + d * (x[i] - w)
    return w, m2


def routed_samples(samples, routes):
    """samples[sweep][chain][S], routes[sweep][chain] = slot -> [slot][sweep][S]: what every slot received, in sweep order"""
    samples = np.asarray(samples, dtype=np.float64)
    nsweeps, nchains, S = samples.shape
    out = np.zeros((nchains, nsweeps, S))
    for i in range(nsweeps):
        assert sorted(routes[i]) == list(range(nchains))
        for c in range(nchains):
            out[routes[i][c], i] = samples[i, c]
    return out


def series_run(per_slot, bin_size, max_bins, auto_rebin, state=None):
    """The series of ONE set of slots fed per_slot[slot][sweep][S] sweep by sweep: open += x from 0.0; the bin_size-th sample closes the
    bin with one division; with auto_rebin the close that makes max_bins bins merges neighbouring bins (bin_size doubles, the open bin
    stays).  Without auto_rebin a sweep on a full series raises.  state: the dict a former call returned, to go on from.
    Returns dict(bins [slot][closed][S], open [slot][S], bin_size, in_open, samples, rebins)."""
    per_slot = np.asarray(per_slot, dtype=np.float64)
    nslots, nsweeps, S = per_slot.shape
    if state is None:
        state = dict(bins=np.zeros((nslots, 0, S)), open=np.zeros((nslots, S)), bin_size=bin_size, in_open=0, samples=0, rebins=0)
    bins = [list(state["bins"][s]) for s in range(nslots)]
    open_bin = np.array(state["open"], dtype=np.float64)
    bin_size, in_open, samples, rebins = state["bin_size"], state["in_open"], state["samples"], state["rebins"]
    for i in range(nsweeps):
        if len(bins[0]) >= max_bins:
            raise RuntimeError("the series is full")
        for s in range(nslots):
            open_bin[s] = open_bin[s] + per_slot[s, i]
        samples += 1
        in_open += 1
        if in_open == bin_size:
            for s in range(nslots):
                bins[s].append(open_bin[s] / float(bin_size))
                open_bin[s] = 0.0
            in_open = 0
            if auto_rebin and len(bins[0]) == max_bins:
                for s in range(nslots):
                    bins[s] = list(rebinned(np.array(bins[s])))
                bin_size *= 2
                rebins += 1
    return dict(bins=np.array([np.array(b).reshape(-1, S) for b in bins]), open=open_bin, bin_size=bin_size, in_open=in_open,
                samples=samples, rebins=rebins)


def ar1(seed, n, rho, mean):
    """x_t = mean + z_t, z_t = rho z_(t-1) + sqrt(1 - rho^2) e_t with unit normal e_t and z_0 from the stationary law; exact
    integrated autocorrelation time 1/2 (1 + rho) / (1 - rho)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n)
    z = np.zeros(n)
    z[0] = e[0]
    c = np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        z[t] = rho * z[t - 1] + c * e[t]
    return mean + z
