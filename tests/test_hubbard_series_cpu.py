"""CPU checks of the Hubbard measurement series: the numpy reference (tests/hubbard_series_reference.py) against the jackknife taken from
its definition, the NaN rule of the derived quantities on constructed bins, the sample restatement against detqmc_amd.structure_factor,
and the new C entry points' handling of a null handle (the one test here that needs the built library)."""
import ctypes as C
import os

import numpy as np
import pytest

import hubbard_series_reference as hr
import series_reference as sr


def _bins(seed, B, L, lo=0.5):
    """[B][8][N] positive structure factors that fall off from Q = (0, 0) and (L/2, L/2): every root argument is positive"""
    rng = np.random.default_rng(seed)
    N = L * L
    peak = np.full(N, 1.0)
    peak[0] = peak[(L // 2) * L + L // 2] = 3.0
    return peak[None, None, :] * (1.0 + lo * rng.uniform(-0.2, 0.2, (B, 8, N)))


@pytest.mark.parametrize("L,B", [(4, 3), (6, 5)])
def test_derived_under_both_jackknives(L, B):
    bins = _bins(10 + L, B, L)
    for Q in [(L // 2, L // 2), (0, 0)]:
        assert np.all(hr.root_arguments(bins, L, Q) > 0.0)
        v1, e1 = hr.derived(bins, L, Q)
        v2, e2 = hr.derived(bins, L, Q, jack=sr.jackknife_explicit)
        fig = max(np.abs(v1 - v2).max(), np.abs(e1 - e2).max())
        print(f"L {L} Q {Q}: jackknife vs its definition {fig:.2e} (bound 1e-12)")
        assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1)) and fig <= 1e-12
    # Q = (1, 0): S(Q) is no peak, the root's argument is negative for some channel -- both forms agree on where the NaNs are
    v1, e1 = hr.derived(bins, L, (1, 0))
    v2, e2 = hr.derived(bins, L, (1, 0), jack=sr.jackknife_explicit)
    assert np.array_equal(np.isnan(v1), np.isnan(v2)) and np.array_equal(np.isnan(e1), np.isnan(e2))
    ok = ~np.isnan(e1)
    assert np.abs(v1[ok] - v2[ok]).max() <= 1e-12 and np.abs(e1[ok] - e2[ok]).max() <= 1e-12


def test_nan_rule():
    L, N, B = 4, 16, 3
    Q = (2, 2)
    q0, q1, q2 = hr.q_points(L, Q)
    bins = np.ones((B, 8, N))
    bins[:, :, q0] = 3.0
    # channel 2: one leave-one-out set has a negative argument (bins 1 and 2 alone give S(Q) < Sbar), the mean does not
    bins[:, 2, q0] = [9.0, 0.5, 0.5]
    args = hr.root_arguments(bins, L, Q)
    assert args[0, 2] > 0.0 and args[1, 2] < 0.0 and args[2, 2] > 0.0 and args[3, 2] > 0.0
    v, e = hr.derived(bins, L, Q)
    assert np.isfinite(v[8 + 2]) and np.isnan(e[8 + 2])
    assert np.isfinite(v[2]) and np.isfinite(e[2])                     # R of the same channel is defined everywhere
    others = [i for i in range(19) if i != 8 + 2]
    assert np.all(np.isfinite(v[others])) and np.all(np.isfinite(e[others]))
    # channel 5: the mean itself has a negative argument
    bins[:, 5, q0] = [0.5, 0.6, 0.7]
    v, e = hr.derived(bins, L, Q)
    assert np.isnan(v[8 + 5]) and np.isnan(e[8 + 5]) and np.isfinite(v[5]) and np.isfinite(e[5])
    others = [i for i in range(19) if i not in (8 + 2, 8 + 5)]
    assert np.all(np.isfinite(v[others])) and np.all(np.isfinite(e[others]))
    # the mean negative but no leave-one-out set computed from fewer bins can rescue the error: B = 2 with both sets positive is impossible,
    # so the rule "err is NaN where the value is" is exercised through the value above; a vanishing denominator is NaN as well
    bins[:, 6, q0] = 0.0
    v, e = hr.derived(bins, L, Q)
    assert np.isnan(v[6]) and np.isnan(e[6])
    bins[:, 7, q1] = -bins[:, 7, q2]
    v, e = hr.derived(bins, L, Q)
    assert np.isnan(v[8 + 7]) and np.isnan(e[8 + 7]) and np.isfinite(v[7])
    # the spin entries follow spinZZ + 2 spinXX
    assert v[16] == bins[:, 3, q0].mean() + 2.0 * bins[:, 4, q0].mean()


@pytest.mark.parametrize("L", [4, 6])
def test_sample_restatement_against_structure_factor(L):
    from detqmc_amd import structure_factor
    N, rows = L * L, 2
    rng = np.random.default_rng(20 + L)
    eq = np.concatenate([[20.0], rng.standard_normal(8 * N) * 20.0])
    got = hr.eq_sample_from_block(eq, L).reshape(2, 8, N)
    c = eq[1:].reshape(8, N) / (N * eq[0])
    assert np.array_equal(got[0], c)
    fig = sr.rows_close(got[1], structure_factor(c, L), 1e-12, N)
    td = np.concatenate([[1.0, 1.0], rng.standard_normal(rows * 6 * N)])
    got = hr.td_sample_from_block(td, L, rows).reshape(2, rows, 6, N)
    c = td[rows:].reshape(rows, 6, N) / N
    assert np.array_equal(got[0], c)
    fig = max(fig, sr.rows_close(got[1], structure_factor(c, L), 1e-12, N))
    print(f"L {L}: S(q) of the restatement vs detqmc_amd.structure_factor {fig:.2e} of the row (bound 1e-12)")
    a = np.concatenate([[3.0, 4.0, 5.0, 6.0, 1.5, 20.0], rng.standard_normal(N)])
    s = hr.scalars_from_block(a, N, 1.0, 4.0, -0.5)
    assert s.shape == (8 + N,) and np.array_equal(s[8:], a[6:] / 20.0)
    assert s[2] == s[0] + s[1] and s[7] == s[5] + s[6] and s[6] == 4.0 * s[3]


def test_null_handle_is_rejected_by_the_series_entry_points():
    import detqmc_amd
    if not os.path.exists(detqmc_amd.LIB_PATH):
        from detqmc_amd.build import build
        build(verbose=False)
    lib = detqmc_amd.load()
    dp = np.zeros(64).ctypes.data_as(C.POINTER(C.c_double))
    st = detqmc_amd._lib.dqmc_series_state()
    calls = [lambda: lib.dethubbard_series_begin(None, 2, 3, 0), lambda: lib.dethubbard_series_info(None, None, None, None),
             lambda: lib.dethubbard_series_stats(None, 0, dp, dp), lambda: lib.dethubbard_series_stats_all(None, 0, dp, dp),
             lambda: lib.dethubbard_series_read_bins(None, 0, 0, 1, dp), lambda: lib.dethubbard_series_derived_all(None, 0, 0, dp, dp),
             lambda: lib.dethubbard_series_configure(None, 0), lambda: lib.dethubbard_series_rebin(None),
             lambda: lib.dethubbard_series_get_state(None, C.byref(st)), lambda: lib.dethubbard_series_binning(None, 0, 1, dp, dp),
             lambda: lib.dethubbard_series_binning_all(None, 0, 1, dp, dp), lambda: lib.dethubbard_series_save(None, b"x"),
             lambda: lib.dethubbard_series_load(None, b"x"), lambda: lib.dethubbard_series_end(None)]
    for call in calls:
        assert call() == -1
        assert b"null" in lib.dethubbard_last_error()
    assert lib.dqmc_series_hubbard_derived_host(None, 0, 0, dp, dp) == -1 and b"null" in lib.dqmc_last_error()
