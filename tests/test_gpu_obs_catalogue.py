"""Every observable name of detqmc_amd.model through the host replica's catalogue, at the smallest shape at which every branch exists:
L = 4, m = 12, s = 4 (two coarse rows, thirteen fine ones), apbc-x (a swapped x / y offset in kOcc or G(k, tau) would show), four chains
in two sub-batches (the chain's index inside its kernel context matters), one thermalisation and two measurement sweeps, every
measurement option on, two custom bilinears (one with a bond part), two pair operators, the averaged Green's function and a series with
binSize = 1, so that bin k is sweep k.  opdim = 3 and opdim = 1 cover the R = 4 and the R = 2 expansion of the Green matrix.

Tolerances: a ...TauQ0 is the sum of N = 16 entries of its ...Tau row, formed in another order than numpy's; a ...Sq is a cosine sum of
16 entries; a series sample is formed on the device from the same blocks by sums of at most 16 x 13 terms.  The roundoff of a sum of n
terms is at most n u sum |x_i|, u = 1.1e-16: below 1e-13 (n = 16) and 1e-12 (n = 208) of the sum of the absolute values of the terms,
which is the scale the differences are measured on -- the largest such sum in the array for the first two, the largest entry of the
reference for the series.  Every figure is printed before it is asserted."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, M, S, NFREQ, CHAINS = 4, 12, 4, 3, (0, 3)
EINVAL = -1


def _batch(opdim, **options):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=opdim, L=L, m=M, s=S, dtau=0.1, delaySteps=4, bc="apbc-x", stabilisation="qr", fermionMeasurements=True,
                  timeDisplacedMeasurements=True, rngSeed=4711, **options)
    return p, DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.05 * i) for i in range(4)], sub_batches=2)


def _names():
    from detqmc_amd import model
    names = [n for n in model.OBSERVABLES if n not in model.SERIES_PHI_OBS]
    return names + [f"{p}{c}{k}" for p in ("custom", "customPair") for c in range(2) for k in ("Tau", "TauQ0", "Corr", "Sq")]


def _with_twins(names):
    from detqmc_amd import model
    return names + [n + "Fine" for n in names if model.observable_index(n)[1].has_fine_twin]


@pytest.fixture(scope="module", params=[3, 1])
def run(request):
    """(opdim, info, per sweep and chain: name -> vector, per sweep and chain: name -> Matsubara transform, chain -> name -> series bins)"""
    from detqmc_amd import bond_kinetic, model, pair_operator
    opdim = request.param
    p, b = _batch(opdim, equalTimeCorrelators=True, bandCorrelators=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=True, timeDisplacedEverySlice=True)
    b.set_custom_bond_bilinears([(np.diag([1.0, -1.0, -1.0, 1.0]), None, None), bond_kinetic(p, "x")])
    b.set_custom_pair_operators([pair_operator("s"), pair_operator("d_bond")])
    b.set_green_matrix(True)
    b.series_begin(1, 4, nfreq=NFREQ, phi=True)
    b.sweepThermalization()
    names = _with_twins(_names())
    transformed = [n for n in _names() if model.observable_index(n)[1].has_matsubara]
    vectors, transforms = [], []
    for _ in range(2):
        b.sweep(True)
        vectors.append({c: {n: b.chain(c).observable_vector(n) for n in names} for c in CHAINS})
        transforms.append({c: {n: b.chain(c).matsubara(n, NFREQ) for n in transformed} for c in CHAINS})
    in_series = [n for n in _names() + list(model.SERIES_PHI_OBS) if model.observable_index(n)[1].series_part >= 0]
    bins = {c: {n: b.chain(c).series_bins(n) for n in in_series} for c in CHAINS}
    info = b.chain(0).info
    info = dict(N=info.N, m=info.m, n=info.n, opdim=info.opdim)
    b.close()
    return opdim, info, vectors, transforms, bins


def test_shapes_and_finiteness_of_every_name(run):
    from detqmc_amd import model
    opdim, info, vectors, _, bins = run
    assert (info["N"], info["m"], info["n"]) == (L * L, M, M // S)
    assert len(vectors[0][0]) == 43 - 2 + 16 + (18 + 4 + 8 + 1)     # the names that are set, and the twins of those that have one
    for name, v in vectors[1][3].items():
        fine = name.endswith("Fine")
        rows = M + 1 if fine else M // S - 1
        base = name[:-4] if fine else name
        want = ((rows, 16, 4, 4) if base == "greenMatrixTau" else (rows, 16) if base.endswith("Tau") or base.startswith("greenKTau")
                else (rows,) if base.endswith("TauQ0") or base.startswith("bondKinetic") else (16,))
        assert v.shape == want and v.dtype == (np.complex128 if base == "greenMatrixTau" else np.float64), name
        assert np.isfinite(v).all(), name
    R = 4 if opdim == 3 else 2
    for name, v in bins[3].items():
        kind = model.observable_index(name)[1].kind
        want = {model._lib.DETSDW_OBS_KIND_CORR: (16,), model._lib.DETSDW_OBS_KIND_SQ: (16,), model._lib.DETSDW_OBS_KIND_TAU: (NFREQ, 16),
                model._lib.DETSDW_OBS_KIND_GREEN_MATRIX: (M + 1, 16, R, R), model._lib.DETSDW_OBS_KIND_PHI_CHI: (NFREQ, 16),
                model._lib.DETSDW_OBS_KIND_PHI_SCALARS: (5,)}[kind]
        assert v.shape == (2,) + want and np.isfinite(v).all(), name


def test_row_sums_and_structure_factors(run):
    from detqmc_amd import structure_factor
    _, _, vectors, _, _ = run
    worst_q0 = worst_sq = 0.0
    for sweep in vectors:
        for c in CHAINS:
            v = sweep[c]
            for name in v:
                if "TauQ0" in name:
                    tau = v[name.replace("TauQ0", "Tau")]
                    e = np.abs(v[name] - tau.sum(-1)).max() / np.abs(tau).sum(-1).max()
                    worst_q0 = max(worst_q0, e)
                    assert e < 1e-13, (name, e)
                if name.endswith("Sq"):
                    corr = v[name[:-2] + "Corr"]
                    e = np.abs(v[name] - structure_factor(corr, L)).max() / np.abs(corr).sum()
                    worst_sq = max(worst_sq, e)
                    assert e < 1e-12, (name, e)
    print(f"...TauQ0 against ...Tau.sum(-1): {worst_q0:.1e} (bound 1e-13); ...Sq against structure_factor(...Corr): {worst_sq:.1e} (bound 1e-12)")


def test_series_bin_k_is_sweep_k(run):
    """binSize = 1: bin k holds the equal-time vector, the Matsubara transform or the stored Green matrix of measurement sweep k"""
    opdim, _, vectors, transforms, bins = run
    R = 4 if opdim == 3 else 2
    worst = {}
    for c in CHAINS:
        for name, got in bins[c].items():
            if name in ("phiChi", "phiScalars"):           # formed from the field: no vector of a sweep to compare with (tests/test_gpu_series_phi.py)
                continue
            for k in range(2):
                ref = (vectors[k][c]["greenMatrixTauFine"][..., :R, :R] if name == "greenMatrixTau"
                       else transforms[k][c][name] if name in transforms[k][c] else vectors[k][c][name])
                e = np.abs(got[k] - ref).max() / np.abs(ref).max()
                worst[name] = max(worst.get(name, 0.0), e)
    print("series bin k against sweep k, worst over chains and sweeps: " + ", ".join(f"{n} {e:.1e}" for n, e in sorted(worst.items())) + " (bound 1e-12)")
    assert len(worst) == 10 + 4 + 11 + 4 * 3 + 1
    for name, e in worst.items():
        assert e < 1e-12, (name, e)


def test_minimal_options_refuse_every_other_name():
    """fermionMeasurements and timeDisplacedMeasurements only: the four slice vectors and greenKTauX / Y are there, every other index of a
    name -- the order-parameter ones, the unset custom ones and every 'Fine' twin included -- is refused with ParameterWrong"""
    from detqmc_amd import DqmcError, model
    from detqmc_amd._lib import _DP, check
    _, b = _batch(3)
    b.sweepThermalization()
    b.sweep(True)
    there = ("kOccX", "kOccY", "pairPlus", "pairMinus", "greenKTauX", "greenKTauY")
    out = np.zeros(13 * 16 * 32)
    for name in _with_twins(_names() + list(model.SERIES_PHI_OBS)):
        for c in CHAINS:
            if name in there:
                v = b.chain(c).observable_vector(name)
                assert v.shape == ((16,) if name in there[:4] else (2, 16)) and np.isfinite(v).all() and np.abs(v).max() > 0
                continue
            b.chain(c)._sel()
            with pytest.raises(DqmcError) as err:
                check(b.lib.detsdw_get_observable_vector(b.h, model.observable_index(name)[0], out.ctypes.data_as(_DP)), host=True)
            assert err.value.code == EINVAL, name
    b.close()
