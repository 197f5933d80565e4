"""The numpy side of the measurement series (tests/series_reference.py) and detqmc_amd.jackknife: no GPU."""
import numpy as np
import pytest

import series_reference as sr


def _bins(B=7, n=16, seed=5):
    rng = np.random.default_rng(seed)
    return 3.0 + rng.normal(size=(B, n))


def test_reference_jackknife_vs_explicit_leave_one_out():
    L = 4
    x = _bins(n=L * L)
    x[:, (L // 2) * L + L // 2] += 4.0                       # S(Q) well away from zero
    mean, err = sr.jackknife(x)
    emean, eerr = sr.jackknife_explicit(x)
    assert np.abs(mean - emean).max() <= 1e-14 * np.abs(emean).max()
    assert np.abs(err - eerr).max() <= 1e-12 * eerr.max()
    f = lambda s: sr.correlation_ratio(s, L)
    val, rerr = sr.jackknife(x, f)
    eval_, ererr = sr.jackknife_explicit(x, f)
    assert rerr > 1e-3
    assert abs(val - eval_) <= 1e-14 and abs(rerr - ererr) <= 1e-12 * ererr


@pytest.mark.parametrize("B", [2, 3, 9])
def test_linear_quantities_give_the_standard_error(B):
    x = _bins(B=B, n=11, seed=B)
    mean, err = sr.jackknife(x)
    want = np.sqrt(((x - x.mean(axis=0)) ** 2).sum(axis=0) / (B * (B - 1)))
    assert np.abs(err - want).max() <= 1e-13 * want.max()
    lin = lambda v: 2.0 * v[..., 0] - v[..., 3]
    val, lerr = sr.jackknife(x, lin)
    y = lin(x)
    assert abs(val - y.mean()) <= 1e-13 * abs(y.mean())
    assert abs(lerr - np.sqrt(((y - y.mean()) ** 2).sum() / (B * (B - 1)))) <= 1e-13 * lerr


def test_package_jackknife_matches_the_reference():
    from detqmc_amd import jackknife
    L = 4
    x = _bins(B=5, n=2 * L * L, seed=11).reshape(5, 2, L * L)
    x[:, :, (L // 2) * L + L // 2] += 4.0
    x[:, :, 0] += 4.0
    for f in (None, lambda s: sr.correlation_ratio(s, L), lambda s: sr.correlation_ratio(s, L, pairing=True)):
        got, ref = jackknife(x, f), sr.jackknife(x, f)
        for g, r in zip(got, ref):
            assert np.shape(g) == np.shape(r)
            assert np.abs(np.asarray(g) - r).max() <= 1e-13 * np.abs(r).max()
    with pytest.raises(ValueError):
        jackknife(x[:1])


@pytest.mark.parametrize("L", [4, 6])
def test_correlation_ratio_of_perfect_order_and_of_no_order(L):
    d = np.arange(L * L)
    stag = (-1.0) ** (d % L + d // L)
    s = sr.structure_factor_ref(stag, L)
    assert abs(s[(L // 2) * L + L // 2] - L * L) < 1e-12 and abs(sr.correlation_ratio(s, L) - 1.0) < 1e-13
    delta = np.zeros(L * L)
    delta[0] = 1.0
    assert abs(sr.correlation_ratio(sr.structure_factor_ref(delta, L), L)) < 1e-13
    assert abs(sr.correlation_ratio(sr.structure_factor_ref(np.ones(L * L), L), L, pairing=True) - 1.0) < 1e-13


@pytest.mark.parametrize("L", [4, 6])
def test_reference_structure_factor_vs_package(L):
    from detqmc_amd import structure_factor
    c = np.random.default_rng(L).normal(size=(3, L * L))
    ref, got = sr.structure_factor_ref(c, L), structure_factor(c, L)
    assert np.abs(ref - got).max() <= 1e-13 * np.abs(ref).max()


def test_sample_normalisation_and_rho_s():
    N = 16
    block = np.concatenate([[3.0], np.arange(5 * N, dtype=np.float64)])
    c = sr.eq_correlators_from_block(block, N)
    assert c.shape == (5, N) and c[1, 2] == (N + 2) / (16.0 * 3.0)
    from detqmc_amd import superfluid_stiffness
    rng = np.random.default_rng(1)
    xx, yy = (rng.normal(size=(2, 3, N)) + 1j * rng.normal(size=(2, 3, N)) for _ in range(2))
    assert np.array_equal(sr.rho_s(xx[:, 0], yy[:, 0], 4), superfluid_stiffness(xx, yy, 4))
