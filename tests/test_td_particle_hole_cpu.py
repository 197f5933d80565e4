"""Time-displaced particle-hole correlators, the part that needs no GPU: the Wick formula of tests/td_ph_reference.py against exact
diagonalisation, the identity that gives G(0) of a boundary's own field configuration, and the option in the built library and the
Python parameters."""
import numpy as np
import pytest


def _fock_operators(nmodes):
    """Jordan-Wigner annihilators c_a, a = 0 .. nmodes-1, as dense 2^nmodes matrices"""
    a = np.array([[0.0, 1.0], [0.0, 0.0]])
    z = np.diag([1.0, -1.0])
    ops = []
    for k in range(nmodes):
        m = np.ones((1, 1))
        for q in range(nmodes):
            m = np.kron(m, z if q < k else a if q == k else np.eye(2))
        ops.append(m.astype(complex))
    return ops


def _exp_herm(h, sign=-1.0):
    w, v = np.linalg.eigh(h)
    return (v * np.exp(sign * w)) @ v.conj().T


@pytest.mark.parametrize("nfac,cut", [(4, 2), (5, 1), (6, 4)])
def test_wick_formula_against_exact_diagonalisation(nfac, cut):
    """2 sites x 4 flavours = 8 modes, 256-dimensional Fock space; U = prod_k exp(-c^+ h_k c).  <O_i(tau) O_j(0)> =
    Tr[U_n .. U_(cut+1) O_i U_cut .. U_1 O_j] / Tr[U] against W from the four single-particle Green's functions, for every M and
    every site pair.  Both sides are numpy fp64 on O(1) numbers: 1e-11 covers the conditioning of the 256 x 256 trace."""
    from td_ph_reference import M_CHARGE, M_SPINZ, M_SDW, greens_from_b, wick
    ns, nm = 2, 8
    rng = np.random.default_rng(100 * nfac + cut)
    c = _fock_operators(nm)
    cd = [x.conj().T for x in c]
    hs = []
    for _ in range(nfac):
        h = rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm))
        h = 0.5 * (h + h.conj().T)
        hs.append(h / np.linalg.norm(h, 2))                        # spectral norm 1
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
    # the conventions themselves, element by element
    for a in range(nm):
        for b in range(nm):
            assert abs(np.trace(Ul @ c[a] @ Ur @ cd[b]) / Z - gt0[a, b]) < 1e-11
            assert abs(-np.trace(Ul @ cd[b] @ Ur @ c[a]) / Z - g0t[a, b]) < 1e-11
            assert abs(np.trace(Ul @ Ur @ c[a] @ cd[b]) / Z - g00[a, b]) < 1e-11
            assert abs(np.trace(Ul @ c[a] @ cd[b] @ Ur) / Z - gtt[a, b]) < 1e-11
    worst = 0.0
    for M in (M_CHARGE, M_SPINZ) + M_SDW:
        O = [sum(M[a, b] * cd[a * ns + i] @ c[b * ns + i] for a in range(4) for b in range(4) if M[a, b] != 0) for i in range(ns)]
        W = wick(gtt, gt0, g0t, g00, M, ns)
        for i in range(ns):
            for j in range(ns):
                ed = np.trace(Ul @ O[i] @ Ur @ O[j]) / Z
                worst = max(worst, abs(ed - W[i, j]))
    print(f"{nfac} factors, cut {cut}: worst |ED - Wick| = {worst:.2e}")
    assert worst < 1e-11


def test_green0_identity_with_svd_factors():
    """1 - G(0) = [U_l Dlmin] Z^-1 [Drmin V_r^H] with Z = Drmax^-1 (U_r^H V_l) Dlmax^-1 + Drmin (V_r^H U_l) Dlmin, SVD factors of the
    oracle's chains, O(2), L = 4, m = 20, s = 5, every interior boundary, against the direct inverse (1e-10, the parity level)"""
    from conftest import relerr
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle
    N, m, s = 16, 20, 5
    phi = np.random.default_rng(21).uniform(-1.0, 1.0, (m + 1, N, 2))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=2, L=4, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    ch = Chain(ora)
    for j in range(1, m // s):
        tau = s * j
        ur, dr, vrh = np.linalg.svd(ch.B(tau, 0))
        ul, dl, vlh = np.linalg.svd(ch.B(m, tau))
        vr, vl = vrh.conj().T, vlh.conj().T
        rmax_inv, rmin = 1.0 / np.maximum(dr, 1.0), np.minimum(dr, 1.0)
        lmax_inv, lmin = 1.0 / np.maximum(dl, 1.0), np.minimum(dl, 1.0)
        Z = (rmax_inv[:, None] * (ur.conj().T @ vl) * lmax_inv[None, :]) + (rmin[:, None] * (vr.conj().T @ ul) * lmin[None, :])
        Zi = np.linalg.inv(Z)
        g00 = np.eye(ora.ng) - (ul * lmin[None, :]) @ Zi @ (rmin[:, None] * vr.conj().T)
        gtt, gt0, g0t, g00_ref = four_greens(ch, tau)
        e = relerr(g00, g00_ref)
        print(f"tau = {tau}: G(0) from the split factors vs direct inverse {e:.2e}")
        assert e < 1e-10
        # the other three members of the family, same factors
        assert relerr((vl * lmax_inv[None, :]) @ Zi @ (rmax_inv[:, None] * ur.conj().T), gtt) < 1e-10
        assert relerr((vl * lmax_inv[None, :]) @ Zi @ (rmin[:, None] * vr.conj().T), gt0) < 1e-10
        assert relerr(-(ul * lmin[None, :]) @ Zi @ (rmax_inv[:, None] * ur.conj().T), g0t) < 1e-10


def test_binning_and_channel_average():
    """C(d) against an explicit loop, and sdw = mean of the first OPDIM inter-band spin bilinears"""
    from td_ph_reference import M_X, M_Y, bin_periodic, expand, four_greens, ph_correlators, wick
    from td_reference import Chain, make_oracle
    N, L, m = 16, 4, 10
    phi = np.random.default_rng(5).uniform(-1.0, 1.0, (m + 1, N, 2))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=2, L=L, beta=1.0, dtau=0.1, s=5, delaySteps=4)
    gs = four_greens(Chain(ora), 5)
    ch, sz, sdw = ph_correlators(ora, *gs)
    full = [expand(ora, g) for g in gs]
    Wx, Wy = wick(*full, M_X, N), wick(*full, M_Y, N)
    for d in range(N):
        dx, dy = d % L, d // L
        acc = 0.0
        for b in range(N):
            a = ((b // L + dy) % L) * L + (b % L + dx) % L
            acc += 0.5 * (Wx[a, b].real + Wy[a, b].real)
        assert abs(sdw[d] - acc / N) < 1e-13                                # summation order only
    assert np.allclose(bin_periodic(Wx, L).sum(), Wx.real.sum() / N)
    assert np.abs(ch).max() > 1e-3 and np.abs(sz).max() > 1e-3 and np.abs(sdw).max() > 1e-3


def test_library_and_parameters_carry_the_option():
    import ctypes as C
    from detqmc_amd import SDWParams, _lib
    from detqmc_amd.model import DetSDW
    lib = _lib.load()
    for sym in ("dqmc_measure_timedisplaced_ph", "dqmc_measure_td_ph_accum_size", "dqmc_measure_td_ph_read_host",
                "dqmc_get_green0_timedisplaced_host"):
        assert hasattr(lib, sym), sym
    assert lib.dqmc_measure_td_ph_accum_size(None) == 0
    assert lib.dqmc_measure_timedisplaced_ph(None, 1) != 0
    out = np.zeros(4)
    assert lib.dqmc_measure_td_ph_read_host(None, out.ctypes.data_as(_lib._DP)) != 0
    # the flag took a reserved slot: the structs keep their size and the older fields their offsets
    assert C.sizeof(_lib.dqmc_params) == 192 and _lib.dqmc_params.td_particle_hole.offset == 188
    assert C.sizeof(_lib.detsdw_params) == 264 and _lib.detsdw_params.timeDisplacedParticleHole.offset == 260
    with pytest.raises(ValueError, match="timeDisplacedParticleHole needs timeDisplacedMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, fermionMeasurements=True, timeDisplacedParticleHole=True))
