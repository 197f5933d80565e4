"""numpy restatement of the routed measurement series (dqmc_series_form_sample / dqmc_series_accumulate, detsdw_series_route): the
sample of chain c of a sweep goes to slot route[c] of that sweep; a slot's open bin sums its samples in call order from 0.0 and the
bin_size-th one closes the bin with one division.  Deliberately plain: explicit loops, the operations of k_series_accum in its order."""
import numpy as np


def check_route(route, nchains):
    """the route as a list of ints; ValueError unless it is a permutation of 0 .. nchains-1"""
    route = [int(s) for s in route]
    if len(route) != nchains or sorted(route) != list(range(nchains)):
        raise ValueError("the route must be a permutation of 0 .. %d: %r" % (nchains - 1, route))
    return route


def routed_bins(samples, routes, bin_size):
    """samples[sweep][chain][S], routes[sweep][chain] = slot of that chain's sample, bin_size >= 1 -> bins[slot][bin][S] with
    bins[slot][k] = ((0.0 + s_1) + s_2 ...) / bin_size over the slot's samples of sweeps k bin_size .. (k + 1) bin_size - 1, in sweep
    order.  Sweeps beyond the last full bin stay in the open bin and are not returned."""
    samples = np.asarray(samples, dtype=np.float64)
    nsweeps, nchains, S = samples.shape
    if len(routes) != nsweeps:
        raise ValueError("one route per sweep")
    if bin_size < 1:
        raise ValueError("bin_size must be at least 1")
    bins = np.zeros((nchains, nsweeps // bin_size, S))
    open_bin = np.zeros((nchains, S))
    for i in range(nsweeps):
        route = check_route(routes[i], nchains)
        for c in range(nchains):
            open_bin[route[c]] = open_bin[route[c]] + samples[i, c]
        if (i + 1) % bin_size == 0:
            for s in range(nchains):
                bins[s, i // bin_size] = open_bin[s] / float(bin_size)
                open_bin[s] = 0.0
    return bins
