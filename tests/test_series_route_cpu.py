"""The numpy side of the routed measurement series (tests/series_route_reference.py) and the route_series switch of
pt.replica_exchange_step where it needs no device: no GPU."""
import numpy as np
import pytest

import series_route_reference as srr


def test_hand_written_two_chains_two_sweeps():
    # sweep 0: identity; sweep 1: swapped.  Slot 0 = chain 0 then chain 1, slot 1 = chain 1 then chain 0.  Powers of two and small
    # integers: every sum and the halving are exact, so the expectation is written down, not computed
    samples = [[[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]],
               [[0.5, 0.25, 3.0], [64.0, 128.0, 5.0]]]
    bins = srr.routed_bins(samples, [[0, 1], [1, 0]], 2)
    assert bins.shape == (2, 1, 3)
    assert np.array_equal(bins[0, 0], [(1.0 + 64.0) / 2, (2.0 + 128.0) / 2, (4.0 + 5.0) / 2])
    assert np.array_equal(bins[1, 0], [(8.0 + 0.5) / 2, (16.0 + 0.25) / 2, (32.0 + 3.0) / 2])
    one = srr.routed_bins(samples, [[0, 1], [1, 0]], 1)      # bin_size 1: the bins are the routed samples themselves
    assert np.array_equal(one[0], [samples[0][0], samples[1][1]]) and np.array_equal(one[1], [samples[0][1], samples[1][0]])


def test_direction_of_a_cycle():
    # route[c] is the SLOT of chain c, not the chain of slot c: a 3-cycle tells the two apart
    samples = np.arange(3.0).reshape(1, 3, 1) + 10.0         # chain c holds 10 + c
    bins = srr.routed_bins(samples, [[1, 2, 0]], 1)
    assert [bins[s, 0, 0] for s in range(3)] == [12.0, 10.0, 11.0]


@pytest.mark.parametrize("bin_size", [1, 2, 3])
def test_identity_route_gives_the_per_chain_bins(bin_size):
    rng = np.random.default_rng(11)
    nsweeps, nch, S = 7, 3, 5
    smp = rng.normal(size=(nsweeps, nch, S))
    bins = srr.routed_bins(smp, [list(range(nch))] * nsweeps, bin_size)
    assert bins.shape == (nch, nsweeps // bin_size, S)       # the sweeps beyond the last full bin stay open
    for c in range(nch):
        for k in range(nsweeps // bin_size):
            acc = np.zeros(S)
            for i in range(k * bin_size, (k + 1) * bin_size):
                acc = acc + smp[i, c]
            assert np.array_equal(bins[c, k], acc / bin_size)


def test_order_of_the_sum_is_the_call_order():
    # (0 + a) + b with a + b rounding differently from b + a is impossible, but ((0 + a) + b) + c differs from (0 + c) + (a + b)
    a, b, c = 1.0, 2.0 ** -53, 2.0 ** -53
    got = srr.routed_bins([[[a]], [[b]], [[c]]], [[0]] * 3, 3)[0, 0, 0]
    assert got == ((0.0 + a) + b + c) / 3.0 and got != (a + (b + c)) / 3.0


def test_permutation_check():
    assert srr.check_route((2, 0, 1), 3) == [2, 0, 1]
    for bad in ([0, 0, 1], [0, 1], [0, 1, 3], [-1, 0, 1], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            srr.check_route(bad, 3)
    with pytest.raises(ValueError):
        srr.routed_bins(np.zeros((2, 2, 1)), [[0, 1], [1, 1]], 1)
    with pytest.raises(ValueError):
        srr.routed_bins(np.zeros((2, 2, 1)), [[0, 1]], 1)


class _Rep:
    """stand-in replica with the exchange surface of pt.py; not a chain of a DetSDWBatch"""

    def __init__(self, r):
        self.r, self.cd = r, b"\0" * 8

    def get_exchange_parameter_value(self):
        return self.r

    def set_exchange_parameter_value(self, v):
        self.r = v

    def get_exchange_action_contribution(self):
        return 1.0

    def get_control_data(self):
        return self.cd

    def set_control_data(self, blob):
        self.cd = blob

    def rand01(self):
        raise AssertionError("equal neighbours: the swap needs no draw")


class _TwoRanks:
    """stand-in torch.distributed of world size 2 whose collectives must never be reached"""

    def get_rank(self):
        return 0

    def get_world_size(self):
        return 2

    def all_gather(self, *a):
        raise AssertionError("collective reached")

    broadcast = all_gather


def test_route_series_refuses_an_ensemble_across_ranks_and_ignores_other_replicas():
    from detqmc_amd import pt
    rvals = [-1.0, -1.0]
    with pytest.raises(ValueError, match="route_series"):
        pt.replica_exchange_step([_Rep(-1.0)], pt.ExchangeState.create(rvals, 0, 2, n_local=1), _TwoRanks(), route_series=True)
    # replicas that are not the chains of one batch: the switch changes nothing
    out = []
    for flag in (False, True):
        reps = [_Rep(r) for r in rvals]
        st = pt.ExchangeState.create(rvals, 0, 1, n_local=2)
        out.append((pt.replica_exchange_step(reps, st, None, route_series=flag), st.par_swapUpAccepted, [r.r for r in reps]))
    assert out[0] == out[1] and out[0][0] == [1, 0]
