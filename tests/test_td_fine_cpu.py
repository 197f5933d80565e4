"""Every-slice time-displaced measurements, the part that needs no GPU: the propagation and end-point identities in numpy float64 with
the oracle's B matrices, the slice coverage rule, the option's parameter rule, and e_ref (printed), the error of the unstabilised
float64 propagation that the GPU test's bound against direct inverses is a multiple of."""
import numpy as np
import pytest

import td_fine_reference as tf
from conftest import relerr


@pytest.mark.parametrize("name", tf.CPU_CASES)
def test_propagation_identities(name):
    """G(tau_{k+-1},0), G(0,tau_{k+-1}), G(tau_{k+-1}) from those of slice k: propagating Chain.greens(tau_j) by the oracle's B
    matrices reproduces Chain.greens(k) on every slice of every segment.  Both sides are float64 numpy; neither is stabilised, so the
    error grows with the conditioning of the at most s - 1 factors: 1e-9 at beta = 2."""
    err = tf.case_e_ref(name)
    print(f"case {name}: propagation vs direct inverse, largest relative error {err:.2e}")
    assert err < 1e-9


def test_e_ref():
    e = tf.e_ref()
    print(f"e_ref = {e:.3e} (largest over {', '.join(tf.CPU_CASES)})")
    assert 0.0 < e < 1e-9


@pytest.mark.parametrize("name", ["a2", "a3", "d", "g"])
def test_end_point_identities(name):
    """G(0+,0) = G(0), G(0,0+) = G(0) - 1, G(beta-,0) = 1 - G(0), G(0,beta-) = -G(0): the limits of the direct formulas, taken one
    slice inside and propagated out with B_1 resp. B_m"""
    _, _, m, s, _ = tf.CASES[name]
    ch = tf.case_chain(name)[2]
    g0 = np.linalg.inv(np.eye(ch.ora.ng) + ch.B(m, 0))
    one = np.eye(ch.ora.ng)
    gtt, gt0, g0t = ch.greens(1)
    t0, ot, tt = tf.step(ch.Bk, (gt0, g0t, gtt), 1, -1)
    assert max(relerr(t0, g0), relerr(ot, g0 - one), relerr(tt, g0)) < 1e-10
    gtt, gt0, g0t = ch.greens(m - 1)
    t0, ot, tt = tf.step(ch.Bk, (gt0, g0t, gtt), m - 1, +1)
    assert max(relerr(t0, one - g0), relerr(ot, -g0), relerr(tt, g0)) < 1e-10


@pytest.mark.parametrize("m,s", [(20, 5), (22, 5), (10, 5)])
def test_every_slice_is_hit_exactly_once(m, s):
    assert tf.coverage(m, s) == list(range(m + 1))


def test_option_needs_timedisplaced_measurements():
    from detqmc_amd import DqmcError, SDWParams, _lib
    from detqmc_amd.model import DetSDW
    with pytest.raises(DqmcError, match="timeDisplacedEverySlice needs timeDisplacedMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, timeDisplacedEverySlice=True))
    # the option travels as a flag bit: the structs keep their bytes
    import ctypes as C
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264
    assert _lib.DQMC_TD_EVERY_SLICE == 0x100 and _lib.DETSDW_TD_EVERY_SLICE == 0x100
    lib = _lib.load()
    assert lib.dqmc_measure_td_fine_accum_size(None, 0) == 0
    assert lib.detsdw_get_tau_grid_fine(None, (C.c_double * 4)()) != 0
