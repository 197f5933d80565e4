"""Wrap-error diagnostics without a GPU: the numpy reference of the compare (tests/green_check_reference.py) against a brute-force double
loop at n_g = 8, and the Python decoding of the table layout (detqmc_amd.model.green_check_decode / green_check_worst) on a synthetic block."""
import math

import numpy as np
import pytest

import green_check_reference as ref


def _brute(Gw, Gf, N):
    n = Gf.shape[0]
    out = dict(maxAbs=-1.0, argmax=0, maxSiteDiag=0.0, sumAbs=0.0, maxFresh=0.0, nonfinite=0)
    for col in range(n):
        for row in range(n):
            w, f = complex(Gw[row, col]), complex(Gf[row, col])
            if not all(math.isfinite(x) for x in (w.real, w.imag, f.real, f.imag)):
                out["nonfinite"] += 1
                d = math.inf
            else:
                dx, dy = w.real - f.real, w.imag - f.imag
                d = math.sqrt(dx * dx + dy * dy)
                out["sumAbs"] += d
                if row % N == col % N:
                    out["maxSiteDiag"] = max(out["maxSiteDiag"], d)
                out["maxFresh"] = max(out["maxFresh"], math.sqrt(f.real * f.real + f.imag * f.imag))
            if d > out["maxAbs"]:
                out["maxAbs"], out["argmax"] = d, row + col * n
    return out


def _pair(seed, n=8):
    rng = np.random.default_rng(seed)
    Gf = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    E = 1e-12 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return Gf + E, Gf


def _assert_same(got, want, n):
    assert got["argmax"] == want["argmax"] and got["nonfinite"] == want["nonfinite"]
    for k in ("maxAbs", "maxSiteDiag", "maxFresh"):
        assert got[k] == want[k], k                      # same operations on both sides: the same bits
    assert abs(got["sumAbs"] - want["sumAbs"]) <= ref.tol_sum(n) * want["sumAbs"]


@pytest.mark.parametrize("N", [2, 4])
def test_reference_against_double_loop(N):
    Gw, Gf = _pair(5)
    _assert_same(ref.green_diff(Gw, Gf, N), _brute(Gw, Gf, N), 8)
    # planted on the site diagonal of another block, then off it
    for (row, col), on_site in (((1 + N, 1), True), ((3, 6) if N == 4 else (2, 5), False)):
        Gw2 = Gw.copy()
        Gw2[row, col] += 1e-9
        got = ref.green_diff(Gw2, Gf, N)
        _assert_same(got, _brute(Gw2, Gf, N), 8)
        assert got["argmax"] == row + 8 * col
        assert (got["maxSiteDiag"] == got["maxAbs"]) == on_site


def test_reference_zero_difference_and_ties():
    _, Gf = _pair(6)
    got = ref.green_diff(Gf, Gf, 4)
    assert got == dict(maxAbs=0.0, argmax=0, maxSiteDiag=0.0, sumAbs=0.0, maxFresh=got["maxFresh"], nonfinite=0)
    Gf0 = np.zeros_like(Gf)
    Gw = Gf0.copy()
    Gw[5, 2] = 0.5
    Gw[1, 6] = 0.5j                                      # the same difference later in column-major order
    got = ref.green_diff(Gw, Gf0, 4)
    assert got["argmax"] == 5 + 8 * 2 and got["maxAbs"] == 0.5 and got["maxFresh"] == 0.0
    _assert_same(got, _brute(Gw, Gf0, 4), 8)


def test_reference_does_not_hide_a_nan():
    Gw, Gf = _pair(7)
    clean = ref.green_diff(Gw, Gf, 4)
    Gw[6, 3] = complex(np.nan, 0.0)
    Gf2 = Gf.copy()
    Gf2[0, 7] = complex(0.0, np.inf)
    got = ref.green_diff(Gw, Gf2, 4)
    assert got["nonfinite"] == 2 and got["maxAbs"] == math.inf and got["argmax"] == 6 + 8 * 3
    assert math.isfinite(got["sumAbs"]) and math.isfinite(got["maxSiteDiag"]) and math.isfinite(got["maxFresh"])
    assert got["sumAbs"] < clean["sumAbs"]
    _assert_same(got, _brute(Gw, Gf2, 4), 8)


def test_log_spread():
    assert ref.log_spread([4.0, 1.0, 2.0]) == math.log(4.0)


def test_decode_synthetic_table():
    from detqmc_amd.model import GREEN_CHECK_FIELDS, green_check_decode, green_check_worst
    chains, n, ng = 2, 3, 8
    assert len(GREEN_CHECK_FIELDS) == 11
    raw = np.zeros((chains, 2, n + 1, 11))
    # chain 0, down sweep, boundary 2: three samples
    raw[0, 0, 2] = [3, 1e-9, 4e-9, 6e-9, 2e-9, 9e-10, 5e-9, 5 + 8 * 6, 0, 12.5, 30.0]
    # chain 1, up sweep, boundary 3: one sample with a non-finite entry
    raw[1, 1, 3] = [1, np.inf, np.inf, np.inf, 1e-8, 1e-9, np.inf, 7 + 8 * 7, 2, 3.0, 0.0]
    raw[1, 0, 0] = [2, 1e-7, 2e-7, 3e-7, 1e-7, 4e-8, 1e-7, 0, 0, 1.0, 0.0]
    d = green_check_decode(raw, ng)
    assert set(d) == {"count", "lastMaxAbs", "maxAbs", "meanMaxAbs", "maxSiteDiag", "meanAbs", "maxRel", "argmax", "nonfinite",
                      "logScaleSpread", "logSvSpread"}
    for k, v in d.items():
        assert v.shape == ((chains, 2, n + 1, 2) if k == "argmax" else (chains, 2, n + 1)), k
    assert d["count"].dtype.kind == "i" and d["count"][0, 0, 2] == 3 and d["count"].sum() == 6
    assert d["lastMaxAbs"][0, 0, 2] == 1e-9 and d["maxAbs"][0, 0, 2] == 4e-9
    assert d["meanMaxAbs"][0, 0, 2] == 6e-9 / 3 and d["meanAbs"][0, 0, 2] == 9e-10 / 3
    assert d["maxSiteDiag"][0, 0, 2] == 2e-9 and d["maxRel"][0, 0, 2] == 5e-9
    assert tuple(d["argmax"][0, 0, 2]) == (5, 6) and tuple(d["argmax"][1, 1, 3]) == (7, 7) and tuple(d["argmax"][1, 0, 0]) == (0, 0)
    assert d["nonfinite"][1, 1, 3] == 2 and d["nonfinite"].sum() == 2
    assert d["logScaleSpread"][0, 0, 2] == 12.5 and d["logSvSpread"][0, 0, 2] == 30.0
    # rows without a sample: zeros, not 0 / 0
    assert d["meanMaxAbs"][0, 1, 1] == 0.0 and d["meanAbs"][0, 1, 1] == 0.0
    assert green_check_worst(d) == [(4e-9, 0, 2, 5, 6), (math.inf, 1, 3, 7, 7)]
    with pytest.raises(ValueError):
        green_check_decode(raw[..., :10], ng)
