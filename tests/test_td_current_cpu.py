"""Time-displaced current-current correlators, the part that needs no GPU: the bond table against the oracle's hopping matrix, the Wick
formula for bond operators against exact diagonalisation, the free-fermion closed form, the binning, and the option in the built
library and the Python parameters (tests/td_current_reference.py)."""
import numpy as np
import pytest

from test_td_particle_hole_cpu import _exp_herm, _fock_operators


@pytest.mark.parametrize("bc,flux", [("pbc", False), ("apbc-xy", False), ("pbc", True)])
def test_bond_table_reproduces_the_oracle_hopping(bc, flux):
    """e^{-dtau K_band} with K rebuilt from the reference's own bond table against the oracle's _dense_propK, L = 4"""
    from td_current_reference import bond_table, hopping_from_bonds, neighbours
    from td_reference import make_oracle
    L, m = 4, 10
    phi = np.random.default_rng(1).uniform(-1.0, 1.0, (m + 1, L * L, 2))
    ora = make_oracle(phi, opdim=2, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4, bc=bc, weakZflux=flux, checkerboard=False)
    T, nbr = bond_table(ora), neighbours(L)
    props = ora._dense_propK()
    for band in (0, 1):
        K = hopping_from_bonds(T[:, band], nbr, ora.mu_band[band])      # flavours 0, 1 = stored sector of band X, Y
        assert np.abs(K - K.conj().T).max() == 0.0
        err = np.abs(_exp_herm(ora.dtau * K) - props[band]).max()
        print(f"{bc} flux={flux} band {band}: max |e^(-dtau K) - propK| = {err:.2e}")
        assert err < 1e-12
        # the conjugate sector carries the conjugate amplitudes
        assert np.array_equal(T[:, band + 2], np.conj(T[:, band]))
    if flux:
        assert np.abs(T.imag).max() > 0.1
    if bc == "apbc-xy":
        assert (T[0, 0].real < 0).sum() == L and (T[1, 0].real < 0).sum() == L      # txhor, txver < 0: -t > 0 except on wrapped bonds


@pytest.mark.parametrize("nfac,cut", [(4, 2), (5, 1), (6, 4)])
def test_bond_wick_against_exact_diagonalisation(nfac, cut):
    """4-site ring x 2 flavours = 8 modes, complex hoppings.  <O_A(tau) O_B(0)> = Tr[U_n .. U_(cut+1) O_A U_cut .. U_1 O_B] / Tr[U] for the
    current and the kinetic operator of every bond pair, against the general Wick formula (dense M) and its written-out bond form.
    Both sides are numpy fp64 on O(1) numbers with the same 256-dimensional trace: 1e-11."""
    from td_current_reference import bond_matrix, one_body_bond, one_body_dense, wick_bond, wick_dense
    from td_ph_reference import greens_from_b
    ns, F, nm = 4, 2, 8
    rng = np.random.default_rng(1000 * nfac + cut)
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
    gs = greens_from_b(prod(Bs, 0, cut, nm), prod(Bs, cut, nfac, nm))
    Z = np.trace(Ul @ Ur)
    T = rng.normal(size=(F, ns)) + 1j * rng.normal(size=(F, ns))         # complex hopping of bond i -> i + 1, per flavour
    nb = (np.arange(ns) + 1) % ns
    worst = 0.0
    for kind, a in (("current", 1j * T), ("kinetic", T)):
        Ms = [bond_matrix(a, nb, i, F) for i in range(ns)]
        for M in Ms:
            assert np.abs(M - M.conj().T).max() == 0.0 and np.trace(M) == 0.0
        Os = [sum(M[p, q] * cd[p] @ c[q] for p in range(nm) for q in range(nm) if M[p, q] != 0) for M in Ms]
        W = wick_bond(*gs, a, a, nb)
        ot, o0 = one_body_bond(gs[0], a, nb), one_body_bond(gs[3], a, nb)
        for i in range(ns):
            worst = max(worst, abs(np.trace(Ul @ Os[i] @ Ur) / Z - ot[i]), abs(np.trace(Ul @ Ur @ Os[i]) / Z - o0[i]))
            worst = max(worst, abs(one_body_dense(gs[0], Ms[i]) - ot[i]))
            for j in range(ns):
                ed = np.trace(Ul @ Os[i] @ Ur @ Os[j]) / Z
                worst = max(worst, abs(ed - wick_dense(*gs, Ms[i], Ms[j])), abs(ed - W[i, j]))
        assert np.abs(W).max() > 1e-3, kind
    print(f"{nfac} factors, cut {cut}: worst |ED - Wick| = {worst:.2e}")
    assert worst < 1e-11


def _free_greens(L, m, dtau, tau, pars):
    """four full Green's functions of the uncoupled model, from e^{-tau K} by direct inverses (no engine code path)"""
    from td_current_reference import FLAVOUR_BAND, bond_table_band, hopping_from_bonds, neighbours
    from td_ph_reference import greens_from_b
    N = L * L
    nbr = neighbours(L)
    T = np.zeros((2, 4, N), dtype=complex)
    bt0, bbt = np.zeros((4 * N, 4 * N), dtype=complex), np.zeros((4 * N, 4 * N), dtype=complex)
    for a in range(4):
        band = FLAVOUR_BAND[a]
        T[:, a] = bond_table_band(L, band, pars["txhor"], pars["txver"], pars["tyhor"], pars["tyver"])
        K = hopping_from_bonds(T[:, a], nbr, (pars["mux"], pars["muy"])[band])
        sl = slice(a * N, (a + 1) * N)
        bt0[sl, sl] = _exp_herm(tau * dtau * K)
        bbt[sl, sl] = _exp_herm((m - tau) * dtau * K)
    return greens_from_b(bt0, bbt), T


FREE = dict(txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0, mux=-0.5, muy=-0.3)


def test_free_fermions_conserved_current():
    """no coupling, periodic boundaries: the total current commutes with H, so sum_d Lambda_mumu(d, tau) is the same for every tau and
    equals (1/N) sum_{alpha, k} v^2 f (1 - f); the kinetic term equals (1/N) sum (-2 t cos k) f.  L = 4, beta = 2."""
    from td_current_reference import current_correlators_full, free_fermion_closed_form
    L, m, dtau = 4, 20, 0.1
    lam_ref, kin_ref = free_fermion_closed_form(L, m * dtau, **FREE)
    assert min(lam_ref) > 1e-2
    for tau in (5, 10, 15):
        gs, T = _free_greens(L, m, dtau, tau, FREE)
        lx, ly, kx, ky = current_correlators_full(*gs, T, L)
        errs = [abs(lx.sum() - lam_ref[0]), abs(ly.sum() - lam_ref[1]), abs(kx - kin_ref[0]), abs(ky - kin_ref[1])]
        print(f"tau = {tau}: Lxx {lx.sum():.12f} Lyy {ly.sum():.12f} kx {kx:.12f} ky {ky:.12f}; errors {max(errs):.1e}")
        assert max(errs) < 1e-12


def test_binning_against_an_explicit_loop():
    from td_current_reference import bond_table, current_correlators, neighbours, wick_bond
    from td_ph_reference import expand, four_greens
    from td_reference import Chain, make_oracle
    N, L, m = 16, 4, 10
    phi = np.random.default_rng(7).uniform(-1.0, 1.0, (m + 1, N, 2))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=2, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4, weakZflux=True)
    gs = four_greens(Chain(ora), 5)
    lx, ly, kx, ky = current_correlators(ora, *gs)
    full = [expand(ora, g) for g in gs]
    T, nbr = bond_table(ora), neighbours(L)
    for lam, d in ((lx, 0), (ly, 1)):
        W = wick_bond(*full, 1j * T[d], 1j * T[d], nbr[d])
        for bin_ in range(N):
            dx, dy = bin_ % L, bin_ // L
            acc = 0.0
            for b in range(N):
                a = ((b // L + dy) % L) * L + (b % L + dx) % L
                acc += W[a, b].real
            assert abs(lam[bin_] - acc / N) < 1e-13
        assert np.abs(lam).max() > 1e-3
    assert abs(kx) > 1e-3 and abs(ky) > 1e-3


def test_library_and_parameters_carry_the_option():
    import ctypes as C
    from detqmc_amd import SDWParams, _lib
    from detqmc_amd.model import DetSDW
    lib = _lib.load()
    for sym in ("dqmc_measure_timedisplaced_current", "dqmc_measure_td_current_accum_size", "dqmc_measure_td_current_read_host"):
        assert hasattr(lib, sym), sym
    assert lib.dqmc_measure_td_current_accum_size(None) == 0
    assert lib.dqmc_measure_timedisplaced_current(None, 1) != 0
    out = np.zeros(4)
    assert lib.dqmc_measure_td_current_read_host(None, out.ctypes.data_as(_lib._DP)) != 0
    # no new struct field: the option is value 2 of the particle-hole flag
    assert C.sizeof(_lib.dqmc_params) == 192 and _lib.dqmc_params.td_particle_hole.offset == 188
    assert C.sizeof(_lib.detsdw_params) == 264 and _lib.detsdw_params.timeDisplacedParticleHole.offset == 260
    base = dict(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, timeDisplacedMeasurements=True)
    with pytest.raises(ValueError, match="timeDisplacedCurrent needs timeDisplacedParticleHole"):
        DetSDW(SDWParams(timeDisplacedCurrent=True, **base))
    from detqmc_amd.model import _host_params
    assert _host_params(SDWParams(timeDisplacedParticleHole=True, timeDisplacedCurrent=True, **base)).timeDisplacedParticleHole == 2
    assert _host_params(SDWParams(timeDisplacedParticleHole=True, **base)).timeDisplacedParticleHole == 1
