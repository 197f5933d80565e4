"""Band-resolved charge correlators bandDiff / bandMix, the part that needs no GPU: the Wick reference of tests/band_reference.py
against exact diagonalisation, the sector identities of the O(1) / O(2) models the kernels rely on, inputs that tell bandDiff from
4 x spinZ, and the options in the built library and the Python parameters."""
import numpy as np
import pytest

from test_td_particle_hole_cpu import _exp_herm, _fock_operators


@pytest.mark.parametrize("nfac,cut", [(4, 2), (5, 1)])
def test_wick_against_exact_many_body(nfac, cut):
    """2 sites x 4 flavours on the 256-dimensional Fock space, as tests/test_td_particle_hole_cpu.py does for its channels:
    Tr[U_l O_i U_r O_j] / Tr[U] against W^M for M_BAND and M_MIX, every site pair; and the equal-time form (one matrix, the delta term
    from g - 1) against Tr[U O_i O_j] / Tr[U].  numpy fp64 on O(1) numbers: 1e-11 covers the conditioning of the trace."""
    from band_reference import BAND_MS
    from eq_corr_reference import wick_eq
    from td_ph_reference import greens_from_b, wick
    ns, nm = 2, 8
    rng = np.random.default_rng(700 * nfac + cut)
    c = _fock_operators(nm)
    cd = [x.conj().T for x in c]
    hs = []
    for _ in range(nfac):
        h = rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm))
        h = 0.5 * (h + h.conj().T)
        hs.append(h / np.linalg.norm(h, 2))
    Us = [_exp_herm(sum(h[a, b] * cd[a] @ c[b] for a in range(nm) for b in range(nm))) for h in hs]
    Bs = [_exp_herm(h) for h in hs]

    def prod(fs, lo, hi, dim):
        out = np.eye(dim, dtype=complex)
        for k in range(lo, hi):
            out = fs[k] @ out
        return out

    Ur, Ul = prod(Us, 0, cut, 2 ** nm), prod(Us, cut, nfac, 2 ** nm)
    gtt, gt0, g0t, g00 = greens_from_b(prod(Bs, 0, cut, nm), prod(Bs, cut, nfac, nm))
    Z = np.trace(Ul @ Ur)
    worst = worst_eq = 0.0
    for M in BAND_MS:
        assert np.array_equal(M @ M, np.eye(4))                               # what the analytic delta term rests on
        O = [sum(M[a, b] * cd[a * ns + i] @ c[b * ns + i] for a in range(4) for b in range(4) if M[a, b] != 0) for i in range(ns)]
        W = wick(gtt, gt0, g0t, g00, M, ns)
        Weq = wick_eq(g00, M, ns)
        for i in range(ns):
            for j in range(ns):
                worst = max(worst, abs(np.trace(Ul @ O[i] @ Ur @ O[j]) / Z - W[i, j]))
                worst_eq = max(worst_eq, abs(np.trace(Ul @ Ur @ O[i] @ O[j]) / Z - Weq[i, j]))
    print(f"{nfac} factors, cut {cut}: worst |ED - Wick| = {worst:.2e}, equal time {worst_eq:.2e}")
    assert worst < 1e-11 and worst_eq < 1e-11


def _kernel_test_inputs(opdim, L=4, m=20, s=5, tau=10):
    """the four shifted matrices the GPU kernel test measures: fields uniform(-1, 1) with seed 300 opdim + L + m"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    phi = np.random.default_rng(300 * opdim + L + m).uniform(-1.0, 1.0, (m + 1, L * L, opdim))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    return ora, [shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)]


@pytest.mark.parametrize("opdim", [1, 2])
def test_sector_identities_and_discriminating_inputs(opdim):
    """OPDIM < 3: the connected part of bandDiff is 4 x that of spinZ (to 1e-14 of its size) and the bandMix one-body values are exact
    zeros, while the FULL bandDiff differs from 4 x spinZ by more than 1e-8 of its largest entry -- a kernel that takes Im for Re in the
    one-body value, or gets the conjugate sector's sign wrong, cannot pass the GPU comparison at 1e-10 on these inputs."""
    from band_reference import M_BAND, band_correlators, band_one_body, connected_part
    from td_ph_reference import M_SPINZ, ph_correlators
    ora, gs = _kernel_test_inputs(opdim)
    cb, cz = connected_part(ora, M_BAND, *gs), connected_part(ora, M_SPINZ, *gs)
    scale = np.abs(cb).max()
    assert scale > 1e-3
    dev = np.abs(cb - 4.0 * cz).max()
    print(f"O({opdim}): |conn(bandDiff) - 4 conn(spinZ)| = {dev:.2e} of {scale:.2e}")
    assert dev <= 1e-14 * scale
    for g in (gs[0], gs[3]):
        ob, om = band_one_body(ora, g)
        assert np.all(om == 0.0)                                              # structural: sums of exact zeros
        assert np.abs(ob.imag).max() <= 1e-15 * np.abs(ob).max() and np.abs(ob.real).max() > 1e-6   # n_x - n_y is small, not zero
    band, mix = band_correlators(ora, *gs)
    spinz = ph_correlators(ora, *gs)[1]
    diff = np.abs(band - 4.0 * spinz).max()
    print(f"O({opdim}): max|bandDiff| {np.abs(band).max():.3f}, max|bandMix| {np.abs(mix).max():.3f}, |bandDiff - 4 spinZ| {diff:.2e}")
    assert diff > 1e-8 * np.abs(band).max()
    assert np.abs(band).max() > 1e-6 and np.abs(mix).max() > 1e-6           # the floor the GPU test asserts


def test_equal_time_delta_term_and_ratios():
    """the equal-time form: the delta term is (1/N) Re tr_4 g in the d = 0 bin alone, and the three correlation ratios pick the
    columns the series kernel reads"""
    from band_reference import BAND_MS, correlation_ratios, eq_band_correlators, eq_band_delta
    from td_ph_reference import bin_periodic, expand, wick
    ora, gs = _kernel_test_inputs(2)
    g = gs[0]
    full = expand(ora, g)
    got = eq_band_correlators(ora, g)
    for M, c in zip(BAND_MS, got):
        nodelta = bin_periodic(wick(full, full, full, full, M, ora.N), ora.L)      # g in the role of g - 1: no delta term
        d = c - nodelta
        assert abs(d[0] - eq_band_delta(ora, g)) < 1e-13 and np.abs(d[1:]).max() < 1e-13
    L = 4
    s = np.arange(2 * L * L, dtype=float).reshape(2, L * L) + 1.0
    r = correlation_ratios(s[0], s[1], L)
    assert r[0] == 1.0 - 0.5 * (s[0, 2 * L + 3] + s[0, 3 * L + 2]) / s[0, 2 * L + 2]
    assert r[1] == 1.0 - 0.5 * (s[0, 1] + s[0, L]) / s[0, 0]
    assert r[2] == 1.0 - 0.5 * (s[1, 2 * L + 3] + s[1, 3 * L + 2]) / s[1, 2 * L + 2]


def test_library_and_parameters_carry_the_options():
    import ctypes as C
    from detqmc_amd import SDWParams, _lib
    from detqmc_amd import model
    from detqmc_amd.model import DetSDW
    lib = _lib.load()
    for sym in ("dqmc_measure_timedisplaced_band", "dqmc_measure_td_band_accum_size", "dqmc_measure_td_band_read_host",
                "dqmc_set_equal_time_band", "dqmc_measure_eq_band_accum_size", "dqmc_measure_eq_band_read_host",
                "dqmc_series_band_derived_host", "detsdw_series_band_derived"):
        assert hasattr(lib, sym), sym
    assert lib.dqmc_measure_td_band_accum_size(None) == 0 and lib.dqmc_measure_eq_band_accum_size(None) == 0
    assert lib.dqmc_measure_timedisplaced_band(None, 1) != 0 and lib.dqmc_set_equal_time_band(None, 1) != 0
    out = np.zeros(4)
    assert lib.dqmc_measure_td_band_read_host(None, out.ctypes.data_as(_lib._DP)) != 0
    assert lib.dqmc_series_band_derived_host(None, out.ctypes.data_as(_lib._DP), out.ctypes.data_as(_lib._DP)) != 0
    # the options travel as flag bits: the structs keep their sizes and their fields their offsets
    assert C.sizeof(_lib.dqmc_params) == 192 and _lib.dqmc_params.td_particle_hole.offset == 188
    assert C.sizeof(_lib.detsdw_params) == 264 and _lib.detsdw_params.timeDisplacedParticleHole.offset == 260
    assert C.sizeof(_lib.dqmc_series_state) == 56
    assert (_lib.DQMC_TD_PH_BAND, _lib.DETSDW_TD_PH_BAND, _lib.DETSDW_FM_EQ_BAND) == (0x100, 0x100, 0x200)
    assert (_lib.DQMC_SERIES_MATS_BAND, _lib.DQMC_SERIES_EQ_BAND) == (128, 256) == (model.SERIES_MATS_BAND, model.SERIES_EQ_BAND)
    assert [model.MATSUBARA[k] for k in ("bandDiffTau", "bandMixTau")] == [34, 35]
    assert [model.BAND_EQ_CORRELATORS[k] for k in ("bandDiffCorr", "bandMixCorr", "bandDiffSq", "bandMixSq")] == [38, 39, 40, 41]
    assert [model.SERIES_DERIVED[k] for k in ("R_dCDW", "R_nematic", "R_bandMix")] == [12, 13, 14]
    assert model.EQ_CORRELATORS["pairMinusSq"] == 31 and model.SERIES_DERIVED["xiPhi"] == 11      # existing indices keep their values
    # bandCorrelators needs one of the two families it rides on
    p = model._host_params(SDWParams(opdim=2, L=4, beta=2.0, s=5))
    assert p.fermionMeasurements == 0 and p.timeDisplacedParticleHole == 0
    with pytest.raises(ValueError, match="bandCorrelators needs timeDisplacedParticleHole or equalTimeCorrelators"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, bandCorrelators=True))
    kw = dict(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, bandCorrelators=True)
    p = model._host_params(SDWParams(timeDisplacedMeasurements=True, timeDisplacedParticleHole=True, **kw))
    assert p.timeDisplacedParticleHole == 1 | 0x100 and p.fermionMeasurements == 1
    p = model._host_params(SDWParams(equalTimeCorrelators=True, **kw))
    assert p.timeDisplacedParticleHole == 0 and p.fermionMeasurements == 1 | 0x100 | 0x200
    p = model._host_params(SDWParams(equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=True,
                                     timeDisplacedCurrent=True, **kw))
    assert p.timeDisplacedParticleHole == 2 | 0x100 and p.fermionMeasurements == 1 | 0x100 | 0x200
