"""Equal-time charge, spin-z, SDW and pairing correlators, the part that needs no GPU: the reference of tests/eq_corr_reference.py
against exact diagonalisation, the A <-> B symmetry and the cosine structure factor, and the option in the built library and the
Python parameters."""
import numpy as np
import pytest

from test_td_particle_hole_cpu import _exp_herm, _fock_operators


class _Full:
    """stand-in for the oracle's band-spin access on a FULL matrix of ns sites (the O(3) rule of _gl1_blocks)"""
    OPDIM = 3

    def __init__(self, ns):
        self.N = ns

    def _gl1_blocks(self, g):
        n = self.N
        return [[g[a * n:(a + 1) * n, b * n:(b + 1) * n] for b in range(4)] for a in range(4)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_against_exact_diagonalisation(seed):
    """2 sites x 4 flavours = 8 modes, 256-dimensional Fock space, rho = exp(-c^+ h c) / Z with a random Hermitian h.  <O^M_A O^M_B> for
    every M and site pair against wick_eq on G = <c c^+> = (1 + e^{-h})^-1, and the pairing expressions
        T+-(A, B) = -4 < D+-(A) D'+-(B) >,   D+- = D_X +- D_Y,  D_b(A) = c_(A b dn) c_(A b up),  D'_b(B) = c^+_(B b dn) c^+_(B b up)
    against pair_terms on the same G.  Bound: the 1e-11 of test_wick_formula_against_exact_diagonalisation (numpy fp64 on O(1) numbers,
    conditioning of the 256 x 256 trace)."""
    from eq_corr_reference import wick_eq
    from td_pair_reference import _bs, pair_terms
    from td_ph_reference import M_CHARGE, M_SDW, M_SPINZ
    ns, nm = 2, 8
    rng = np.random.default_rng(seed)
    c = _fock_operators(nm)
    cd = [x.conj().T for x in c]
    h = rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm))
    h = 0.5 * (h + h.conj().T)
    h *= 2.0 / np.linalg.norm(h, 2)
    rho = _exp_herm(sum(h[a, b] * cd[a] @ c[b] for a in range(nm) for b in range(nm)))
    Z = np.trace(rho)
    G = np.linalg.inv(np.eye(nm) + _exp_herm(h))
    for a in range(nm):
        for b in range(nm):
            assert abs(np.trace(rho @ c[a] @ cd[b]) / Z - G[a, b]) < 1e-11
    worst = 0.0
    for M in (M_CHARGE, M_SPINZ) + M_SDW:
        O = [sum(M[a, b] * cd[a * ns + i] @ c[b * ns + i] for a in range(4) for b in range(4) if M[a, b] != 0) for i in range(ns)]
        W = wick_eq(G, M, ns)
        for i in range(ns):
            for j in range(ns):
                worst = max(worst, abs(np.trace(rho @ O[i] @ O[j]) / Z - W[i, j]))
    tp, tm = pair_terms(_Full(ns), G)
    for sign, T in ((1.0, tp), (-1.0, tm)):
        D = [c[_bs(0, 1) * ns + i] @ c[_bs(0, 0) * ns + i] + sign * c[_bs(1, 1) * ns + i] @ c[_bs(1, 0) * ns + i] for i in range(ns)]
        Dp = [cd[_bs(0, 1) * ns + i] @ cd[_bs(0, 0) * ns + i] + sign * cd[_bs(1, 1) * ns + i] @ cd[_bs(1, 0) * ns + i] for i in range(ns)]
        for i in range(ns):
            for j in range(ns):
                worst = max(worst, abs(-4.0 * np.trace(rho @ D[i] @ Dp[j]) / Z - T[i, j]))
        assert np.abs(T).max() > 1e-3
    print(f"seed {seed}: worst |ED - reference| = {worst:.2e}")
    assert worst < 1e-11


def test_symmetry_and_structure_factor():
    """W(A, B) = W(B, A) for A != B on a random NON-Hermitian g (bilinears on different sites commute, and the Wick form keeps that
    term by term), hence C(d) = C(-d) and a real Fourier sum for the particle-hole channels.  The pairing sums T+-(A, B) and T+-(B, A)
    are complex conjugates only in the ensemble average, not per configuration.  For every channel the cosine sum equals the real part
    of the full complex Fourier sum.  All to rounding (fp64 sums of <= 4 N = 64 O(1) terms: 1e-12)"""
    from eq_corr_reference import fourier_full, structure_factor, wick_eq
    from td_pair_reference import pair_terms
    from td_ph_reference import M_CHARGE, M_SDW, M_SPINZ, bin_periodic
    from detqmc_amd import structure_factor as sf_public
    L, N = 4, 16
    rng = np.random.default_rng(8)
    g = 0.5 * np.eye(4 * N) + 0.2 * (rng.normal(size=(4 * N, 4 * N)) + 1j * rng.normal(size=(4 * N, 4 * N)))
    off = ~np.eye(N, dtype=bool)
    x, y = np.arange(N) % L, np.arange(N) // L
    minus = ((-y) % L) * L + (-x) % L
    Ws = [(wick_eq(g, M, N), True) for M in (M_CHARGE, M_SPINZ) + M_SDW] + [(T, False) for T in pair_terms(_Full(N), g)]
    for W, symmetric in Ws:
        assert np.abs(W[off]).max() > 1e-3
        c = bin_periodic(W, L)
        s = structure_factor(c, L)
        f = fourier_full(c, L)
        if symmetric:
            assert np.abs(W - W.T)[off].max() < 1e-12 * np.abs(W).max()
            assert np.abs(c - c[minus]).max() < 1e-12 * np.abs(c).max()
            assert np.abs(f.imag).max() < 1e-12 * np.abs(s).max()
        assert np.abs(s - f.real).max() < 1e-12 * np.abs(s).max()
        assert np.abs(sf_public(c, L) - s).max() < 1e-12 * np.abs(s).max()
    # leading axes are kept
    c2 = np.stack([bin_periodic(Ws[0][0], L), bin_periodic(Ws[1][0], L)])
    assert sf_public(c2, L).shape == (2, N) and np.abs(sf_public(c2, L)[1] - sf_public(c2[1], L)).max() < 1e-14     # summation order only


def test_eq_correlators_on_an_engine_matrix():
    """the O(2) sector rule: eq_correlators on a stored-sector matrix equals the full-matrix evaluation of diag(g, conj g), and the delta
    term is what distinguishes it from the plain product form at d = 0 only"""
    from eq_corr_reference import eq_correlators, wick_eq
    from td_ph_reference import M_CHARGE, bin_periodic, expand, wick
    from td_reference import make_oracle
    L, N, m = 4, 16, 10
    phi = np.random.default_rng(5).uniform(-1.0, 1.0, (m + 1, N, 2))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=2, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4)
    rng = np.random.default_rng(6)
    g = 0.5 * np.eye(2 * N) + 0.2 * (rng.normal(size=(2 * N, 2 * N)) + 1j * rng.normal(size=(2 * N, 2 * N)))
    out = eq_correlators(ora, g)
    assert len(out) == 5 and all(v.shape == (N,) and np.abs(v).max() > 1e-3 for v in out)
    full = expand(ora, g)
    assert np.array_equal(full[2 * N:, 2 * N:], np.conj(g)) and not full[:2 * N, 2 * N:].any()
    plain = bin_periodic(wick(full, full, full, full, M_CHARGE, N), L)
    diff = bin_periodic(wick_eq(full, M_CHARGE, N), L) - plain
    assert abs(diff[0] - np.trace(full).real / N) < 1e-12 and np.abs(diff[1:]).max() < 1e-12


def test_library_and_parameters_carry_the_option():
    import ctypes as C
    from detqmc_amd import SDWParams, _lib
    from detqmc_amd.model import DetSDW, EQ_CORRELATORS
    lib = _lib.load()
    for sym in ("dqmc_set_equal_time_correlators", "dqmc_measure_eq_accum_size", "dqmc_measure_eq_read_host"):
        assert hasattr(lib, sym), sym
    assert _lib.DETSDW_FM_EQ_CORRELATORS == 0x100
    assert lib.dqmc_measure_eq_accum_size(None) == 0
    assert lib.dqmc_set_equal_time_correlators(None, 1) != 0
    out = np.zeros(4)
    assert lib.dqmc_measure_eq_read_host(None, out.ctypes.data_as(_lib._DP)) != 0
    # a switch and a flag bit: the structs keep their size
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264
    assert sorted(EQ_CORRELATORS.values()) == list(range(22, 32))
    with pytest.raises(ValueError, match="equalTimeCorrelators needs fermionMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, equalTimeCorrelators=True))
