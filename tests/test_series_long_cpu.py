"""The reference of the long-run series (tests/series_long_reference.py) against what is known exactly, and detqmc_amd.binning_analysis
against the reference.  No GPU.

tau at level 6 (bins of 64 samples) of 2^14 samples: over seeds 0 .. 199 the reference gives [3.4, 5.0] with mean 4.17 for AR(1) with
rho = 0.8 (exact: 4.5; bins of 64 still lose a little of the tail) and [0.38, 0.64] for white noise (exact: 0.5).  The tests fix seeds
0 .. 9 and assert [3.0, 5.6] and [0.3, 0.75]."""
import numpy as np
import pytest

import series_long_reference as slr

NSAMPLES, LEVELS = 2 ** 14, 9


def _tau(x, levels=LEVELS):
    x = np.asarray(x).reshape(-1, 1)
    _, m2 = slr.two_pass(x)
    err, tau = slr.binning(x, 1, levels, m2=m2, samples=x.shape[0])
    return err[:, 0], tau[:, 0]


@pytest.mark.parametrize("seed", range(10))
def test_ar1_autocorrelation_time(seed):
    _, tau = _tau(slr.ar1(seed, NSAMPLES, 0.8, 3.0))
    print(f"seed {seed}: tau by level {np.round(tau, 3)} (exact 4.5)")
    assert 3.0 <= tau[6] <= 5.6
    assert tau[0] < tau[2] < tau[4]                          # the plateau is approached from below


@pytest.mark.parametrize("seed", range(10))
def test_white_noise_autocorrelation_time(seed):
    _, tau = _tau(np.random.default_rng(seed).standard_normal(NSAMPLES))
    print(f"seed {seed}: tau by level {np.round(tau, 3)} (exact 0.5)")
    assert 0.3 <= tau[6] <= 0.75


def test_level_zero_is_one_half():
    for seed in range(10):
        for x in (slr.ar1(seed, 1000, 0.8, 3.0), np.random.default_rng(seed).standard_normal(777)):
            _, tau = _tau(x, 1)
            assert abs(tau[0] - 0.5) <= 1e-12, (seed, tau[0])


def test_rebinned_is_level_one_of_the_cascade():
    rng = np.random.default_rng(5)
    for B in (2, 40, 37, 64):
        bins = rng.standard_normal((B, 3, 7))
        even = bins[:2 * (B // 2)]
        ys = slr.cascade(bins, 2)
        assert ys[1].shape[0] == B // 2
        assert np.array_equal(slr.rebinned(even), ys[1])
        assert np.array_equal(ys[1][0], (bins[0] + bins[1]) * 0.5)
    with pytest.raises(ValueError):
        slr.rebinned(rng.standard_normal((3, 2)))


def test_welford_against_two_pass():
    x = np.random.default_rng(11).standard_normal((125, 6)) * np.arange(1, 7) + 40.0
    mean, m2 = slr.two_pass(x)
    w, wm2 = slr.welford(x)
    assert np.abs(w - mean).max() <= 1e-13 * np.abs(mean).max()
    assert np.abs(wm2 - m2).max() <= 1e-12 * np.abs(m2).max()
    assert np.abs(m2 / 124 - x.var(axis=0, ddof=1)).max() <= 1e-12 * m2.max() / 124


def test_series_run_rebins_like_explicit_merging():
    rng = np.random.default_rng(2)
    smp = rng.standard_normal((2, 8, 5))                     # [slot][sweep][S]
    run = slr.series_run(smp, 1, 4, True)
    assert (run["bin_size"], run["in_open"], run["samples"], run["rebins"]) == (4, 0, 8, 2) and run["bins"].shape == (2, 2, 5)
    for s in range(2):
        a = slr.rebinned(slr.rebinned(smp[s, :4]))           # sweeps 1 .. 4 closed one by one, merged at sweep 4 and again at sweep 8
        p56, p78 = ((0.0 + smp[s, 4]) + smp[s, 5]) / 2.0, ((0.0 + smp[s, 6]) + smp[s, 7]) / 2.0
        assert np.array_equal(run["bins"][s, 0], a[0]) and np.array_equal(run["bins"][s, 1], (p56 + p78) * 0.5)
    with pytest.raises(RuntimeError):
        slr.series_run(smp, 1, 4, False)
    # a run interrupted after sweep 3 and continued gives the same bits
    part = slr.series_run(smp[:, :3], 1, 4, True)
    rest = slr.series_run(smp[:, 3:], 1, 4, True, state=part)
    assert np.array_equal(rest["bins"], run["bins"]) and rest["bin_size"] == 4


def test_binning_analysis_of_the_package_against_the_reference():
    from detqmc_amd import binning_analysis
    rng = np.random.default_rng(9)
    for B, levels in ((40, 5), (37, 5), (2, 1)):
        bins = 2.0 + rng.standard_normal((B, 3, 8))
        m2 = rng.uniform(50.0, 150.0, (3, 8))
        m2[1, 2] = 0.0                                        # no variance: tau is NaN there
        err, tau = slr.binning(bins, 3, levels, m2=m2, samples=125)
        e1 = binning_analysis(bins, 3)
        e2, t2 = binning_analysis(bins, 3, variance=m2 / 124)
        assert e1.shape == e2.shape == t2.shape == err.shape == (levels, 3, 8)
        assert np.abs(e1 - err).max() <= 1e-12 * err.max() and np.array_equal(e1, e2)
        assert np.isnan(t2[:, 1, 2]).all() and np.isnan(tau[:, 1, 2]).all()
        ok = ~np.isnan(tau)
        assert np.array_equal(ok, ~np.isnan(t2)) and np.abs(t2[ok] / tau[ok] - 1.0).max() <= 1e-11
    with pytest.raises(ValueError):
        binning_analysis(np.zeros((1, 4)), 1)
