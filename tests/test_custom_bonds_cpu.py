"""Bond parts of the user-defined bilinears, the part that needs no GPU: the conventions of tests/custom_bond_reference.py against the
references that exist -- the on-site custom correlators, the current-current correlators and the bond kinetic energy, a brute-force
<O_A O_B> over the stencil with explicit deltas -- on oracle matrices; inputs on which the GPU comparison cannot pass trivially; and the
entry points in the built library and the Python layer.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_bond_reference as cb
from conftest import relerr

# (opdim, L, checkerboard, bc, flux): the cases of the GPU kernel test
GPU_CASES = [(1, 4, True, "pbc", False), (2, 4, True, "pbc", False), (3, 4, True, "pbc", False), (2, 4, True, "apbc-xy", False),
             (2, 4, False, "pbc", False), (2, 4, True, "pbc", True), (2, 6, True, "apbc-x", False), (3, 6, True, "pbc", False)]


def _inputs(opdim, L=4, m=20, s=5, tau=10, bc="pbc", flux=False, checkerboard=True):
    """an oracle and its four shifted matrices at tau: fields uniform(-1, 1) with the seed of the GPU kernel test"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    phi = np.random.default_rng(300 * opdim + L + m).uniform(-1.0, 1.0, (m + 1, L * L, opdim))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=checkerboard, weakZflux=flux, delaySteps=4)
    return ora, [shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)]


def test_the_operators():
    from detqmc_amd import SDWParams, bond_current, bond_kinetic
    M0, Mx, My = cb.B_RAND
    assert np.array_equal(M0, M0.conj().T) and all(np.count_nonzero(m) == 16 and np.abs(m.imag).max() > 0.1 for m in cb.B_RAND)
    assert np.abs(Mx - Mx.conj().T).max() > 0.5 and np.abs(My - My.conj().T).max() > 0.5      # the bond parts are not Hermitian
    assert all(np.count_nonzero(m - np.diag(np.diag(m))) == 0 for m in cb.B_RAND_FLUX[1:]) and cb.B_RAND_FLUX[0] is M0
    assert cb.B_DDW[0] is None and np.array_equal(cb.B_DDW[1], -cb.B_DDW[2]) and cb.B_ONSITE[1] is None and cb.B_ONSITE[2] is None
    p = SDWParams(L=4, beta=2.0, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)
    for mu, t in (("x", (1.0, -0.5, 1.0, -0.5)), ("y", (0.5, -1.0, 0.5, -1.0))):            # -t of band x, y, x, y
        k, j = bond_kinetic(p, mu), bond_current(p, mu)
        on, off = (1, 2) if mu == "x" else (2, 1)
        assert k[0] is None and j[0] is None and k[off] is None and j[off] is None
        assert np.array_equal(k[on], np.diag(t)) and np.array_equal(j[on], 1j * np.diag(t))
        assert np.array_equal(bond_kinetic(p, 0 if mu == "x" else 1)[on], k[on])
    with pytest.raises(ValueError):
        bond_kinetic(p, "z")


@pytest.mark.parametrize("opdim", [2, 3])
def test_dense_form_against_wick_dense(opdim):
    """wick_all (all pairs at once) is wick_dense of the dense matrices, pair by pair: 1e-13 of the largest |W|"""
    from td_current_reference import wick_dense
    from td_ph_reference import expand
    ora, gs = _inputs(opdim)
    full = [expand(ora, g) for g in gs]
    u = cb.link_table(ora.L, ora.pars.bc, ora.pars.weakZflux)
    O = cb.dense_operators(cb.B_RAND, u, ora.L)
    assert all(np.array_equal(o, o.conj().T) for o in O)                       # Hermitian with a non-Hermitian bond part
    W = cb.wick_all(*full, O)
    worst = max(abs(W[A, B] - wick_dense(*full, O[A], O[B])) for A, B in ((0, 0), (0, 1), (5, 4), (3, 15), (12, 0), (9, 6)))
    print(f"O({opdim}): wick_all vs wick_dense {worst:.2e} of {np.abs(W).max():.2e}")
    assert worst < 1e-13 * np.abs(W).max()


@pytest.mark.parametrize("opdim", [2, 3])
def test_onsite_operator_is_the_custom_reference(opdim):
    """(a) B_ONSITE gives custom_correlators / eq_custom_correlators of tests/custom_reference.py: 1e-13"""
    from custom_reference import M_RAND, custom_correlators, eq_custom_correlators
    ora, gs = _inputs(opdim)
    e_td = relerr(cb.bond_correlators(ora, [cb.B_ONSITE], *gs)[0], custom_correlators(ora, [M_RAND], *gs)[0])
    e_eq = relerr(cb.eq_bond_correlators(ora, [cb.B_ONSITE], gs[0])[0], eq_custom_correlators(ora, [M_RAND], gs[0])[0])
    print(f"O({opdim}): B_ONSITE vs the on-site reference: time-displaced {e_td:.2e}, equal-time {e_eq:.2e} (1e-13)")
    assert e_td < 1e-13 and e_eq < 1e-13


@pytest.mark.parametrize("opdim,bc,flux", [(2, "pbc", False), (2, "apbc-xy", False), (2, "pbc", True), (3, "pbc", False), (3, "apbc-xy", False)])
def test_current_and_kinetic_are_the_current_reference(opdim, bc, flux):
    """(b) bond_current / bond_kinetic give Lambda_xx, Lambda_yy and the bond kinetic sums of tests/td_current_reference.py: 1e-12"""
    from detqmc_amd import bond_current, bond_kinetic
    from td_current_reference import current_correlators
    from td_ph_reference import expand
    ora, gs = _inputs(opdim, bc=bc, flux=flux)
    lx, ly, kx, ky = current_correlators(ora, *gs)
    got = cb.bond_correlators(ora, [bond_current(ora.pars, "x"), bond_current(ora.pars, "y")], *gs)
    u = cb.link_table(ora.L, bc, flux)
    kin = [float(cb.one_body_all(expand(ora, gs[0]), cb.dense_operators(bond_kinetic(ora.pars, mu), u, ora.L)).real.sum()) / ora.N for mu in "xy"]
    errs = [relerr(got[0], lx), relerr(got[1], ly), abs(kin[0] - kx) / abs(kx), abs(kin[1] - ky) / abs(ky)]
    print(f"O({opdim}) {bc} flux={flux}: Lxx {errs[0]:.2e} Lyy {errs[1]:.2e} kx {errs[2]:.2e} ky {errs[3]:.2e} (1e-12); "
          f"max|L| {np.abs(lx).max():.3f} {np.abs(ly).max():.3f}, k {kx:.3f} {ky:.3f}")
    assert min(np.abs(lx).max(), np.abs(ly).max(), abs(kx), abs(ky)) > 1e-3
    assert max(errs) < 1e-12


@pytest.mark.parametrize("opdim,bc,flux", [(2, "pbc", False), (2, "apbc-xy", True), (3, "pbc", False)])
def test_equal_time_against_brute_force_with_explicit_deltas(opdim, bc, flux):
    """(c) W from (g, g, g - 1, g) is <O_A O_B> expanded over the twelve (site, flavour) indices of each stencil,
    <c^+_i c_j c^+_k c_l> = (d_ij - g_ji)(d_kl - g_lk) + (d_il - g_li) g_jk with the deltas written out on the global indices, for site
    pairs at d = 0, +-x, +-y, +-(x - y) (stencils that share sites) and two that do not: 1e-13 of the largest |W|"""
    from td_current_reference import neighbours
    from td_ph_reference import expand
    ora, gs = _inputs(opdim, bc=bc, flux=flux)
    L, N = ora.L, ora.N
    g = expand(ora, gs[0])
    op = cb.B_RAND_FLUX if flux else cb.B_RAND
    O = cb.dense_operators(op, cb.link_table(L, bc, flux), L)
    W = cb.wick_all(g, g, g - np.eye(4 * N), g, O)
    nbr = neighbours(L)

    def stencil(A):
        return np.array([a * N + s for a in range(4) for s in (A, nbr[0, A], nbr[1, A])])

    def site(x, y):
        return (y % L) * L + x % L

    B = site(1, 2)
    pairs = [(site(1 + dx, 2 + dy), B) for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, -1), (-1, 1), (2, 0), (2, 2))]
    worst = 0.0
    for A, B in pairs:
        si, sk = stencil(A), stencil(B)
        OA, OB = O[A][np.ix_(si, si)], O[B][np.ix_(sk, sk)]
        for sub, whole in ((OA, O[A]), (OB, O[B])):                              # nothing outside the stencil
            assert np.isclose(np.abs(sub).sum(), np.abs(whole).sum(), rtol=1e-14)
        d_AA, d_BB, d_AB = (si[:, None] == si[None, :]) * 1.0, (sk[:, None] == sk[None, :]) * 1.0, (si[:, None] == sk[None, :]) * 1.0
        n_ij = d_AA - g[np.ix_(si, si)].T                                        # <c^+_i c_j>, i, j in the stencil of A
        n_kl = d_BB - g[np.ix_(sk, sk)].T
        n_il = d_AB - g[np.ix_(sk, si)].T                                        # <c^+_i c_l> = d_il - g_li
        h_jk = g[np.ix_(si, sk)]                                                 # <c_j c^+_k>
        brute = np.einsum("ij,ij->", OA, n_ij) * np.einsum("kl,kl->", OB, n_kl) + np.einsum("ij,kl,il,jk->", OA, OB, n_il, h_jk)
        worst = max(worst, abs(brute - W[A, B]))
    print(f"O({opdim}) {bc} flux={flux}: worst |brute force - W| = {worst:.2e} of {np.abs(W).max():.2e}")
    assert worst < 1e-13 * np.abs(W).max()


@pytest.mark.parametrize("opdim,L,checkerboard,bc,flux", GPU_CASES)
def test_gpu_cases_have_no_vanishing_block(opdim, L, checkerboard, bc, flux):
    """(d) every reference block of the GPU kernel test is far above the 1e-6 floor that test asserts, and W of B_RAND and B_DDW has an
    imaginary part a dropped conjugate would move into the result"""
    ora, gs = _inputs(opdim, L=L, bc=bc, flux=flux, checkerboard=checkerboard)
    ops = cb.bond_ops(ora.pars, flux)
    td, eq = cb.bond_correlators(ora, ops, *gs), cb.eq_bond_correlators(ora, ops, gs[0])
    mtd, meq = [np.abs(c).max() for c in td], [np.abs(c).max() for c in eq]
    print(f"O({opdim}) L={L} {bc} cb={checkerboard} flux={flux}: max|C_td| {['%.3e' % x for x in mtd]}, max|C_eq| {['%.3e' % x for x in meq]}")
    assert min(mtd) > 1e-6 and min(meq) > 1e-6


def test_library_and_python_layer_carry_the_entry_points():
    """(e) the new symbols are exported and bound, nothing is read or written without a context, no struct changed its size"""
    from detqmc_amd import DetSDWBatch, KernelContext, _lib, model
    lib = _lib.load()
    bound = {s[0] for s in _lib.SYMBOLS}
    for sym in ("dqmc_set_custom_bond_bilinears", "dqmc_get_custom_bond_bilinears", "detsdw_set_custom_bond_bilinears", "detsdw_get_custom_bond_bilinears"):
        assert hasattr(lib, sym) and sym in bound, sym
    m = np.ascontiguousarray(cb.B_RAND[0])
    n = C.c_int(5)
    assert lib.dqmc_set_custom_bond_bilinears(None, 1, m.ctypes.data, None, None) == -1
    assert lib.dqmc_get_custom_bond_bilinears(None, C.byref(n), None, None, None) == -1 and n.value == 5
    assert lib.detsdw_set_custom_bond_bilinears(None, 1, m.ctypes.data, None, None) == -1
    assert lib.detsdw_get_custom_bond_bilinears(None, C.byref(n), None, None, None) == -1 and n.value == 5
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264 and C.sizeof(_lib.dqmc_series_state) == 56
    for cls in (KernelContext, DetSDWBatch):
        for name in ("set_custom_bond_bilinears", "get_custom_bond_bilinears", "set_custom_bilinears"):
            assert callable(getattr(cls, name)), (cls, name)
    m0, mx, my = model._custom_bond_operators([cb.B_RAND, cb.B_DDW, cb.B_ONSITE])
    assert all(a.shape == (3, 4, 4) and a.flags.c_contiguous and a.dtype == np.complex128 for a in (m0, mx, my))
    assert np.array_equal(mx[0], cb.B_RAND[1]) and not m0[1].any() and np.array_equal(my[1], cb.B_DDW[2]) and not mx[2].any() and not my[2].any()
    assert all(a.shape == (0, 4, 4) for a in model._custom_bond_operators([]))
    with pytest.raises(ValueError):
        model._custom_bond_operators([(m, None)])
