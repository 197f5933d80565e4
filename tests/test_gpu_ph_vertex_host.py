"""The particle-hole bubble and vertex at the host level: three interacting chains, real measurement sweeps; the derived quantities by
name against the numpy evaluation of the series bins (detqmc_amd.ph_bubble, ph_one_body, jackknife; the bound of the derived-kernel test,
tests/ph_bubble_reference.py), after series_route, and after series_save / series_load.  Every test prints its figures before it asserts."""
import dataclasses

import numpy as np
import pytest

import custom_bond_reference as cb
import ph_bubble_reference as ph

pytestmark = pytest.mark.gpu

L, M, NFREQ, BC = 4, 10, 2, "apbc-xy"
NAMES = ("vertexCustom", "bubbleCustom", "gammaCustom", "gammaBubbleCustom", "disconnectedCustom")


def _batch(sub_batches=1, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    kw = dict(opdim=2, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", bc=BC, fermionMeasurements=True,
              timeDisplacedMeasurements=True, timeDisplacedParticleHole=True, timeDisplacedEverySlice=True, rngSeed=577)
    kw.update(over)
    p = SDWParams(**kw)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8), dataclasses.replace(p, simindex=2, r=0.4)], sub_batches=sub_batches)


def _ops():
    return [cb.B_RAND, cb.B_ONSITE, cb.B_DDW]


def _reference(b, slot, c, Q, ops):
    """numpy jackknife of the series bins of one slot for operator c"""
    g = b.chain(slot).series_bins("greenMatrixTau")
    chi = np.array([b.chain(slot).series_bins(f"custom{k}Tau") for k in range(len(ops))])        # [count, B, nfreq, N]
    P = chi[:, :, 0, Q[1] * L + Q[0]].real.T
    return [x[c] for x in ph.twin_jackknife(g, P, ops, L, BC, 0.1, Q)]


def _check(b, ops, Q, tag):
    bound = ph.gpu_bound()
    for c in range(len(ops)):
        got = [b.series_derived_all(f"{nm}{c}", Q=Q) for nm in NAMES]
        bub = b.series_ph_bubble_all(c, Q)
        for slot in range(3):
            rv, re_ = _reference(b, slot, c, Q, ops)
            v = np.concatenate([[g[0][slot] for g in got], bub[0][slot]])
            e = np.concatenate([[g[1][slot] for g in got], bub[1][slot]])
            dv, de = np.abs(v - rv).max() / np.abs(rv).max(), np.abs(e - re_).max() / np.abs(re_).max()
            print(f"{tag} Q={Q} operator {c} slot {slot}: chi {v[0]:.5f}, chibar {v[1]:.5f}, Gamma chibar {v[3]:.4f} +- {e[3]:.1e}, D {v[4]:.4f}; "
                  f"values {dv:.1e}, errors {de:.1e} (bound {bound:.1e})")
            assert v.shape == (6 + M,) and np.all(np.isfinite(v)) and dv < bound and de < bound


@pytest.mark.parametrize("sub_batches", [1, 3])
def test_host_level_vertex_route_and_file(tmp_path, sub_batches):
    """vertexCustom{c} and its companions equal the numpy evaluation of series_bins; the same after series_route and, with identical
    bits, after series_save -> fresh batch -> series_load"""
    from detqmc_amd import DqmcError
    ops = _ops()
    b = _batch(sub_batches)
    path = str(tmp_path / "ph_vertex.bin")
    try:
        b.sweepThermalization()
        b.set_custom_bond_bilinears(ops)
        b.set_green_matrix(True)
        b.series_begin(1, 8, nfreq=NFREQ)
        for it in range(4):
            if it == 2:
                _check(b, ops, (0, 0), f"sub-batches {sub_batches}, two bins")
                b.series_route([2, 0, 1])
            b.sweep(True)
        for Q in ((0, 0), (L // 2, L // 2)):
            _check(b, ops, Q, f"sub-batches {sub_batches}, routed")
        with pytest.raises(ValueError):
            b.series_derived_all("gammaBubbleCustom0")           # Q has no default for the vertex names
        with pytest.raises(DqmcError):
            b.series_derived_all("bubbleCustom3", Q=(0, 0))      # no fourth matrix
        with pytest.raises(DqmcError):
            b.series_ph_bubble_all(0, (L, 0))
        kept = [b.series_derived_all("gammaBubbleCustom0", Q=(2, 2)), b.series_derived_all("disconnectedCustom1", Q=(0, 0)), b.series_ph_bubble_all(2, (0, 0))]
        b.series_save(path)
        b.series_end()
    finally:
        b.close()
    b = _batch(sub_batches)
    try:
        b.set_custom_bond_bilinears(ops)
        b.series_begin(1, 8, nfreq=NFREQ)                         # without the averaged Green's function: no vertex
        with pytest.raises(DqmcError):
            b.series_derived_all("gammaBubbleCustom0", Q=(0, 0))
        b.series_end()
        b.set_green_matrix(True)
        b.series_begin(1, 8, nfreq=NFREQ)
        b.series_load(path)
        assert b.series_route() == [2, 0, 1]
        again = [b.series_derived_all("gammaBubbleCustom0", Q=(2, 2)), b.series_derived_all("disconnectedCustom1", Q=(0, 0)), b.series_ph_bubble_all(2, (0, 0))]
        assert all(np.array_equal(x, y) for p, q in zip(kept, again) for x, y in zip(p, q))
        b.series_end()
        b.set_green_matrix(False)
    finally:
        b.close()


def test_host_level_options():
    """without timeDisplacedEverySlice the series carries no part 13, without matrices no part 9: the names are refused"""
    from detqmc_amd import DqmcError
    b = _batch(timeDisplacedEverySlice=False, equalTimeCorrelators=True)
    try:
        b.set_custom_bond_bilinears(_ops())
        b.set_green_matrix(True)
        b.sweep(True)
        b.series_begin(1, 4)
        with pytest.raises(DqmcError):
            b.series_derived_all("bubbleCustom0", Q=(0, 0))
        b.series_end()
    finally:
        b.close()
    b = _batch()
    try:
        b.set_green_matrix(True)
        b.series_begin(1, 4, nfreq=NFREQ)
        with pytest.raises(DqmcError):
            b.series_derived_all("vertexCustom0", Q=(0, 0))
        b.series_end()
    finally:
        b.close()
