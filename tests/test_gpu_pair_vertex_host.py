"""The averaged Green's function and the pair vertex at the host level: three interacting chains, real measurement sweeps; the vector
greenMatrixTau, the series part, the derived quantities by name against the numpy evaluation of the series bins (the bound of the
derived-kernel test, tests/pair_vertex_reference.py), routing, and the series file.  Every test prints its figures before it asserts."""
import dataclasses

import numpy as np
import pytest

import custom_pair_reference as cp
import pair_vertex_reference as pv
from test_gpu_band_correlators import EINVAL

pytestmark = pytest.mark.gpu

L, M, NFREQ = 4, 20, 2


def _batch(sub_batches=1, every=True, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=L, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", bc="apbc-xy",
                  fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedEverySlice=every, rngSeed=991, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8), dataclasses.replace(p, simindex=2, r=0.4)], sub_batches=sub_batches)


def _ops():
    from detqmc_amd import pair_operator
    return [pair_operator("d_bond"), cp.P_RAND]


def _reference(b, slot, c, Q, ops):
    """numpy jackknife of the series bins of one slot for operator c"""
    g = b.chain(slot).series_bins("greenMatrixTau")
    chi = np.array([b.chain(slot).series_bins(f"customPair{k}Tau") for k in range(len(ops))])        # [count, B, nfreq, N]
    P = chi[:, :, 0, Q[1] * L + Q[0]].real.T
    return [x[c] for x in pv.jackknife_outputs(g, P, ops, L, "apbc-xy", 0.1, Q)]


def _check(b, ops, Q, tag):
    bound = pv.gpu_bound()
    names = ("vertexCustomPair", "bubbleCustomPair", "gammaCustomPair", "gammaBubbleCustomPair")
    for c in range(len(ops)):
        got = [b.series_derived_all(f"{nm}{c}", Q=Q) for nm in names]
        bub = b.series_pair_bubble_all(c, Q)
        for slot in range(3):
            rv, re_ = _reference(b, slot, c, Q, ops)
            v = np.concatenate([[g[0][slot] for g in got], bub[0][slot]])
            e = np.concatenate([[g[1][slot] for g in got], bub[1][slot]])
            dv, de = np.abs(v - rv).max() / np.abs(rv).max(), np.abs(e - re_).max() / np.abs(re_).max()
            print(f"{tag} Q={Q} operator {c} slot {slot}: P {v[0]:.5f}, Pbar {v[1]:.5f}, Gamma Pbar {v[3]:.4f} +- {e[3]:.1e}; values {dv:.1e}, errors {de:.1e} "
                  f"(bound {bound:.1e})")
            assert dv < bound and de < bound
            if Q == (0, 0):                                       # an interacting field: Pbar is not P, seven orders above the bound
                assert abs(v[1] - v[0]) > 1e-5 * abs(v[0])        # (at Q = (1, 2) the difference is zero within its error bar)


@pytest.mark.parametrize("sub_batches", [1, 3])
def test_host_level_vertex_route_and_file(tmp_path, sub_batches):
    """gammaBubbleCustomPair{c} and its companions equal the numpy evaluation of series_bins; the same after series_route and, with
    identical bits, after series_save -> fresh batch -> series_load; a batch without the switch refuses the file"""
    from detqmc_amd import DqmcError
    ops = _ops()
    b = _batch(sub_batches)
    path = str(tmp_path / "vertex.bin")
    try:
        b.sweepThermalization()
        b.set_custom_pair_operators(ops)
        b.set_green_matrix(True)
        b.series_begin(1, 8, nfreq=NFREQ)
        for it in range(4):
            if it == 2:
                b.series_route([2, 0, 1])
            b.sweep(True)
        ch = b.chain(0)
        vec, fine = ch.observable_vector("greenMatrixTau"), ch.observable_vector("greenMatrixTauFine")
        assert vec.shape == (ch.info.n - 1, L * L, 4, 4) and fine.shape == (M + 1, L * L, 4, 4)
        assert all(np.array_equal(fine[j * 5], vec[j - 1]) for j in range(1, ch.info.n)) and np.abs(vec).max() > 1e-3
        assert np.array_equal(fine[:, :, 2:, 2:], np.conj(fine[:, :, :2, :2])) and not fine[:, :, :2, 2:].any() and not fine[:, :, 2:, :2].any()
        bins = b.chain(2).series_bins("greenMatrixTau")           # chain 0 feeds slot 2 since the route changed
        assert bins.shape == (4, M + 1, L * L, 2, 2) and np.array_equal(bins[3], fine[:, :, :2, :2])
        mean, err = b.series_stats_all("greenMatrixTau")
        assert mean.shape == (3, M + 1, L * L, 2, 2) and np.abs(mean[2] - bins.mean(axis=0)).max() < 1e-14
        for Q in ((0, 0), (1, 2)):
            _check(b, ops, Q, f"sub-batches {sub_batches}")
        kept = [b.series_derived_all("gammaBubbleCustomPair0", Q=(1, 2)), b.series_pair_bubble_all(1, (0, 0))]
        b.series_save(path)
        b.series_end()
    finally:
        b.close()
    b = _batch(sub_batches)
    try:
        b.set_custom_pair_operators(ops)
        b.series_begin(1, 8, nfreq=NFREQ)                         # without the switch: another parts word
        with pytest.raises(DqmcError) as e:
            b.series_load(path)
        assert e.value.code == EINVAL
        with pytest.raises(DqmcError):
            b.series_derived_all("gammaBubbleCustomPair0", Q=(0, 0))
        with pytest.raises(ValueError):
            b.series_derived_all("gammaBubbleCustomPair0")       # Q has no default for the vertex names
        b.series_end()
        b.set_green_matrix(True)
        b.series_begin(1, 8, nfreq=NFREQ)
        with pytest.raises(DqmcError):
            b.set_green_matrix(False)                             # the open series holds the part
        b.series_load(path)
        assert b.series_route() == [2, 0, 1]
        again = [b.series_derived_all("gammaBubbleCustomPair0", Q=(1, 2)), b.series_pair_bubble_all(1, (0, 0))]
        assert all(np.array_equal(x, y) for p, q in zip(kept, again) for x, y in zip(p, q))
        b.series_end()
        b.set_green_matrix(False)
    finally:
        b.close()


def test_host_level_options():
    """the setter needs timeDisplacedMeasurements; flux is refused by the kernel level; without timeDisplacedEverySlice the vector is
    filled and the series carries no part"""
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    kw = dict(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True)
    for pars in (SDWParams(equalTimeCorrelators=True, **kw), SDWParams(timeDisplacedMeasurements=True, weakZflux=True, **kw)):
        rep = DetSDWBatch([pars])
        try:
            with pytest.raises(DqmcError) as e:
                rep.set_green_matrix(True)
            assert e.value.code == EINVAL
        finally:
            rep.close()
    rep = DetSDWBatch([SDWParams(timeDisplacedMeasurements=True, equalTimeCorrelators=True, **kw)])
    try:
        rep.set_green_matrix(True)
        rep.set_custom_pair_operators([cp.P_RAND])
        rep.sweep(True)
        assert np.abs(rep.chain(0).observable_vector("greenMatrixTau")).max() > 1e-3
        with pytest.raises(DqmcError):
            rep.chain(0).observable_vector("greenMatrixTauFine")
        rep.series_begin(1, 4)
        with pytest.raises(DqmcError):
            rep.chain(0).series_bins("greenMatrixTau")
        with pytest.raises(DqmcError):
            rep.series_derived_all("bubbleCustomPair0", Q=(0, 0))
        rep.series_end()
    finally:
        rep.close()
