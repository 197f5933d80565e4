"""Pins tests/update_reference.py (the long-double slice the device is compared with in tests/test_gpu_update_slice.py) so that it
cannot drift together with the kernels: against the committed goldens of the reference program, against the fp64 oracle on prescribed
streams, and against a from-scratch route (one-shot Woodbury over all accepted sites, the reference program's checkAndLog idea).
Also checks, for EVERY row of the GPU case table, that the row's regime gives the acceptance pattern it was chosen for.  CPU only."""
import numpy as np
import pytest

import update_reference as ur
from conftest import load_golden, oracle_params, relerr
from detsdw_oracle import DetSDWOracle, SDWParams
from update_reference import CASES, CLD, ULD, RngSupplier, UpdateReference

TOL = 1e-10        # the goldens' own tolerance (tests/test_oracle_vs_golden.py)


def _proposal_of(pars):
    spm = pars.spinProposalMethod
    return "box" if spm == "box" else "rotate" if spm == "rotate_then_scale" else "rotate_and_scale"      # first sweep: performedSweeps = 0


@pytest.mark.parametrize("name", ["o2_L4", "o3_L4", "o1_L4_cdw", "o2_L4_cdw_slice", "o3_L4_rotscale"])
def test_reference_vs_golden_first_slice(name):
    """the first slice (k = m) of the fixture's own trajectory, its own dSFMT stream as supplier.  Fixtures that keep the slice
    (slice_phi_m ...) are compared with directly; o1_L4_cdw and o3_L4_rotscale keep whole sweeps only, there the fp64 oracle -- pinned
    to those sweeps by tests/test_oracle_vs_golden.py -- supplies the slice."""
    g = load_golden(name)
    o = DetSDWOracle(oracle_params(g["params"]))
    m = o.m
    ref = UpdateReference(o)
    res = ref.update_slice(m, o.phi, o.g, RngSupplier(o.rng), cdwl=o.cdwl if o.pars.cdwU else None, proposal=_proposal_of(o.pars),
                           repeat=o.pars.repeatUpdateInSlice, phiDelta=o.phiDelta, angleDelta=o.angleDelta, scaleDelta=o.scaleDelta)
    if "slice_phi_m" in g:
        phi_m, g_m, acc = g["slice_phi_m"], g["slice_g"], float(g["slice_accRatio"][0])
        cdwl_m = g["slice_cdwl_m"].reshape(-1) if "slice_cdwl_m" in g else None
    else:
        o2 = DetSDWOracle(oracle_params(g["params"]))
        o2.updateInSlice(m)
        phi_m, g_m, acc = o2.phi[m], o2.g, o2.lastAccRatioLocal_phi
        cdwl_m = o2.cdwl[m] if o2.pars.cdwU else None
        assert o2.rng.count == o.rng.count, "uniforms consumed"
    assert np.array_equal(res.phi_k, phi_m), "accept / reject decisions must agree"
    if cdwl_m is not None:
        assert np.array_equal(res.cdwl_k, cdwl_m), "accept / reject decisions of the cdwl pass must agree"
    assert relerr(res.G.astype(np.complex128), g_m) < TOL
    assert abs(res.accRatio - acc) < 1e-15


def _oracle_input(case, chain):
    """field and the fp64 oracle's Green's function of slice case["k"] (on the GPU the device's own G takes this place)"""
    phi, cdwl = ur.case_fields(case, chain)
    pars = SDWParams(beta=ur.M_SLICES * ur.DTAU, s=ur.S_SLICES, **ur.case_params(case)).finalize()
    o = DetSDWOracle(pars, phi=phi, cdwl=cdwl)
    n = o.n
    for kk in range(o.m, case["k"], -1):          # sweepDown's wraps and advances (detmodel.h:1333-1399)
        if kk == (n - 1) * o.s:
            o.advanceDownGreen(n)
        o.wrapDownGreen(kk)
    assert o.currentTimeslice == case["k"]
    return phi, cdwl, o.g


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_table_regimes_and_oracle_agreement(case):
    """every row of the GPU table: the regime cap holds ("all": every proposal accepted, "none": at most N / 8, "alternate": within
    N / 8 of N / 2), the special rows do what they were written for, and DetSDWOracle.updateInSlice_delayed driven by the recorded
    stream takes the same decisions and consumes the same number of uniforms."""
    N = case["L"] ** 2
    nulls = 0
    for chain in range(case["nchains"]):
        phi, cdwl, G = _oracle_input(case, chain)
        lat, res = ur.case_reference(case, chain, phi, cdwl, G)
        for acc in res.accepted[:case["repeat"]]:
            assert ur.regime_cap_ok(case["regimes"][chain], acc, N), (case["regimes"][chain], res.accepted, N)
        twin, consumed = ur.case_twin(case, chain, lat, phi, cdwl, G, res.stream)
        assert consumed == res.consumed == len(res.stream)
        if case["proposal"] == "box":
            assert np.array_equal(twin.phi, res.phi)
        else:
            assert np.max(np.abs(twin.phi - res.phi)) == 0.0       # same libm, same formulas: the oracle's own code forms the proposal
        if lat.pars.cdwU:
            assert np.array_equal(twin.cdwl[case["k"]], res.cdwl_k)
        assert abs(twin.lastAccRatioLocal_phi - res.accRatio) == 0.0
        assert relerr(twin.g, res.G.astype(np.complex128)) < 1e-12
        nulls += res.null_proposals
        if case["expect_dropped"]:
            assert res.dropped >= 1, "no proposal with new_r3 <= 0: choose another seed or a wider scaleDelta"
        if case["expect_direct"]:
            assert res.max_draws > 16, "no proposal consumed more than the prefetched window of 16 uniforms"
    if case["model"].get("cdwU"):
        assert nulls >= 1, "the cdwl stream must contain a null proposal"


@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_sequential_vs_one_shot_woodbury(opdim):
    """the sequential long-double result against G' = G + G[:,I] Delta_I (1 + (1 - G[I,I]) Delta_I)^-1 (G[I,:] - E_I) over all accepted
    sites I of the slice, solved at size MSF |I| <= 64 by the same elimination; and prod det M' = det(1 + (1 - G[I,I]) Delta_I).  Both
    sides are long double: 64 ulp of long double on the companion scale, nothing is measured here."""
    worst = 0.0
    for regime in ("all", "alternate"):
        case = ur._row("woodbury", opdim, 4, 16, regime)
        case["seed"] = 900 + opdim
        phi, cdwl, G = _oracle_input(case, 0)
        lat, res = ur.case_reference(case, 0, phi, cdwl, G)
        sites = [s for _, s in res.sites]
        assert lat.MSF * len(sites) <= 64 and len(sites) >= 8
        G1, det1 = ur.one_shot_woodbury(G, sites, res.deltas, lat.N, lat.MSF)
        err = np.abs(G1 - res.G).astype(np.float64)
        lim = 64 * ULD * res.comp
        worst = max(worst, float(np.max(err / lim)))
        assert np.all(err <= lim), float(np.max(err / lim))
        prod = CLD(1)
        mag = 1.0
        for d in res.dets:
            prod = prod * d
            mag *= float(abs(d.real) + abs(d.imag))
        assert float(abs(prod - det1)) <= 64 * ULD * max(mag, float(abs(det1)))
    print(f"RATIO woodbury o{opdim} {worst:.3f}")
