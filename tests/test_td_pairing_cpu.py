"""Time-displaced pairing correlators, the part that needs no GPU: the test-side reference is anchored to the oracle's (fixture-pinned)
equal-time pairPlus / pairMinus, and the built library and the Python parameters carry the new option."""
import numpy as np
import pytest


@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_pair_terms_match_the_oracles_equal_time_pairing(opdim):
    """one measureFermionic call adds Re [T+-(i, 0) + T+-(0, i)] to pairPlus / pairMinus: the same operations in the same order, so the
    difference is rounding only (1e-13 relative)"""
    from conftest import relerr
    from td_pair_reference import pair_terms
    from td_reference import make_oracle
    N, m = 16, 10
    phi = np.random.default_rng(77 + opdim).uniform(-1.0, 1.0, (m + 1, N, opdim))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=4, beta=1.0, dtau=0.1, s=5, delaySteps=4)
    ora.initMeasurements()
    gs = ora.shiftGreenSymmetric()
    ora.measureFermionic(ora.currentTimeslice)
    plus, minus = pair_terms(ora, gs)
    assert plus.shape == (N, N) and minus.shape == (N, N) and np.iscomplexobj(plus)
    ref_plus = np.real(plus[:, 0] + plus[0, :])
    ref_minus = np.real(minus[:, 0] + minus[0, :])
    ep, em = relerr(ref_plus, ora.pairPlus), relerr(ref_minus, ora.pairMinus)
    print(f"O({opdim}): pairPlus {ep:.2e} pairMinus {em:.2e}")
    assert np.max(np.abs(ora.pairPlus)) > 1e-3            # not a comparison of zeros
    assert ep < 1e-13 and em < 1e-13


def test_pair_correlators_are_the_translation_average():
    """C(d) against an explicit loop over B, and the bin convention dy L + dx with A = B (+) d"""
    from td_pair_reference import pair_correlators, pair_terms
    from td_reference import make_oracle
    N, L, m = 16, 4, 10
    phi = np.random.default_rng(5).uniform(-1.0, 1.0, (m + 1, N, 3))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=3, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4)
    gs = ora.shiftGreenSymmetric()
    plus, minus = pair_terms(ora, gs)
    cp, cm = pair_correlators(ora, gs)
    for d in range(N):
        dx, dy = d % L, d // L
        sp = sm = 0.0
        for b in range(N):
            a = ((b // L + dy) % L) * L + (b % L + dx) % L
            sp += plus[a, b].real
            sm += minus[a, b].real
        assert abs(cp[d] - sp / N) < 1e-13 and abs(cm[d] - sm / N) < 1e-13      # summation order only: N eps sum|T| / N


def test_library_and_parameters_carry_the_option():
    from detqmc_amd import SDWParams, _lib
    from detqmc_amd.model import DetSDW
    lib = _lib.load()
    for sym in ("dqmc_measure_timedisplaced_pair", "dqmc_measure_td_pair_accum_size", "dqmc_measure_td_pair_read_host"):
        assert hasattr(lib, sym), sym
    assert lib.dqmc_measure_td_pair_accum_size(None) == 0
    assert lib.dqmc_measure_timedisplaced_pair(None, 1) != 0
    with pytest.raises(ValueError, match="timeDisplacedPairing needs timeDisplacedMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, timeDisplacedPairing=True))
