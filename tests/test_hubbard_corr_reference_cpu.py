"""The numpy Wick forms of tests/hubbard_corr_reference.py against brute force, so that kernel and test cannot share a sign error:
a 2 x 2 lattice (8 fermion modes, a 256-dimensional Fock space with explicit operator matrices), m = 3 slices of random real one-body
exponents per spin, rho = prod_k e^{-c^+ h_k c}; every one of the 8 + 6 operator definitions evaluated as a trace, the displaced
operator inserted after slice 1 and after slice 2.  Also: the Python parameters reach dethubbard_create in the measureFlags word."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import hubbard_corr_reference as R

L, N, M_SLICES = 2, 4, 3
UP, DN = 0, 1


def _fock_operators(nmodes):
    """annihilators c_0 .. c_{nmodes-1} as 2^nmodes matrices (Jordan-Wigner)"""
    a = np.array([[0.0, 1.0], [0.0, 0.0]])
    z = np.diag([1.0, -1.0])
    ops = []
    for i in range(nmodes):
        m = np.array([[1.0]])
        for j in range(nmodes):
            m = np.kron(m, z if j < i else a if j == i else np.eye(2))
        ops.append(m)
    return ops


@pytest.fixture(scope="module")
def system():
    rng = np.random.default_rng(20260101)
    c = _fock_operators(2 * N)
    cd = [x.T for x in c]
    mode = lambda spin, site: spin * N + site
    for i in range(2 * N):                               # the algebra itself
        for j in range(2 * N):
            anti = c[i] @ cd[j] + cd[j] @ c[i]
            assert np.allclose(anti, np.eye(256) * (i == j)) and np.allclose(c[i] @ c[j] + c[j] @ c[i], 0)
    h = 0.5 * rng.standard_normal((M_SLICES, 2, N, N))   # h[k][spin]: real, not symmetric
    U, B = [], []
    for k in range(M_SLICES):
        quad = sum(h[k, s, i, j] * cd[mode(s, i)] @ c[mode(s, j)] for s in (UP, DN) for i in range(N) for j in range(N))
        U.append(sla.expm(-quad))
        B.append([sla.expm(-h[k, s]) for s in (UP, DN)])
    return dict(c=c, cd=cd, mode=mode, U=U, B=B)


def _site_operators(sy):
    """per site: the operators O_A and their adjoints O^+_A of every channel, in the order R.EQ_NAMES; spinXX is the pair (S^+, S^-)"""
    c, cd, mode = sy["c"], sy["cd"], sy["mode"]
    nb = R.neighbours(L)
    out = []
    for A in range(N):
        cu, cdn = c[mode(UP, A)], c[mode(DN, A)]
        nu, nd = cu.T @ cu, cdn.T @ cdn
        sp = cu.T @ cdn                                  # S^+ = c^+_up c_dn
        pair = lambda f: 0.5 * sum(f[q] * cu @ c[mode(DN, nb[q, A])] for q in range(4))
        out.append(dict(greenUp=cu, greenDn=cdn, charge=nu + nd, spinZZ=0.5 * (nu - nd), spinP=sp, spinM=sp.T, pairS=cu @ cdn,
                        pairSx=pair(R.F_EXT_S), pairD=pair(R.F_D_WAVE)))
    return out


def _brute(sy, names, l):
    """X[ch][A][B] = tr[U_m .. U_{l+1} O_A U_l .. U_1 O^+_B] / tr[U_m .. U_1]  (l = 0: equal time)"""
    U = sy["U"]
    lo, hi = np.eye(256), np.eye(256)
    for k in range(l):
        lo = U[k] @ lo
    for k in range(l, M_SLICES):
        hi = U[k] @ hi
    Z = np.trace(hi @ lo)
    ops = _site_operators(sy)
    X = np.zeros((len(names), N, N))
    for ci, name in enumerate(names):
        for A in range(N):
            for B in range(N):
                if name == "spinXX":
                    t = 0.25 * (np.trace(hi @ ops[A]["spinP"] @ lo @ ops[B]["spinM"]) + np.trace(hi @ ops[A]["spinM"] @ lo @ ops[B]["spinP"]))
                else:
                    t = np.trace(hi @ ops[A][name] @ lo @ ops[B][name].T)
                X[ci, A, B] = t / Z
    return X


def test_equal_time_wick_forms_match_fock_space_traces(system):
    Bs = [[system["B"][k][s] for k in range(M_SLICES)] for s in (UP, DN)]
    g = [R.displaced_greens(Bs[s], 1)[3] for s in (UP, DN)]          # G(0) of both spins
    ref = R.eq_channels(g[UP], g[DN], L)
    brute = _brute(system, R.EQ_NAMES, 0)
    for ci, name in enumerate(R.EQ_NAMES):
        assert np.max(np.abs(ref[ci] - brute[ci])) < 1e-10, name
    assert np.max(np.abs(R.eq_corr(g[UP], g[DN], L) - R.bin_sum(brute, L))) < 1e-10


@pytest.mark.parametrize("l", [1, 2])
def test_time_displaced_wick_forms_match_fock_space_traces(system, l):
    Bs = [[system["B"][k][s] for k in range(M_SLICES)] for s in (UP, DN)]
    four = [R.displaced_greens(Bs[s], l) for s in (UP, DN)]
    gt0, g0t, gtt, g00 = ([four[s][i] for s in (UP, DN)] for i in range(4))
    # the convention of the second function, on its own: G(0,tau)(A, B) = -<c^+_B(tau) c_A(0)>
    c, cd, mode, U = system["c"], system["cd"], system["mode"], system["U"]
    lo, hi = np.eye(256), np.eye(256)
    for k in range(l):
        lo = U[k] @ lo
    for k in range(l, M_SLICES):
        hi = U[k] @ hi
    Z = np.trace(hi @ lo)
    for s in (UP, DN):
        for A in range(N):
            for B in range(N):
                assert abs(-np.trace(hi @ cd[mode(s, B)] @ lo @ c[mode(s, A)]) / Z - g0t[s][A, B]) < 1e-10
    ref = R.td_channels(gt0, g0t, gtt, g00)
    brute = _brute(system, R.TD_NAMES, l)
    for ci, name in enumerate(R.TD_NAMES):
        assert np.max(np.abs(ref[ci] - brute[ci])) < 1e-10, name
    assert np.max(np.abs(R.td_corr(gt0, g0t, gtt, g00, L) - R.bin_sum(brute, L))) < 1e-10


def test_bin_sum_is_the_periodic_site_difference():
    Lb = 4
    X = np.arange(16 * 16, dtype=float).reshape(16, 16)
    out = R.bin_sum(X, Lb)
    for d in range(16):
        s = 0.0
        for B in range(16):
            A = ((B // Lb + d // Lb) % Lb) * Lb + (B % Lb + d % Lb) % Lb
            s += X[A, B]
        assert out[d] == s


@pytest.mark.parametrize("eq,td,word", [(False, False, 0), (True, False, 1), (False, True, 2), (True, True, 3)])
def test_hubbard_params_reach_dethubbard_create_in_measure_flags(eq, td, word):
    import detqmc_amd
    from detqmc_amd import DetHubbard, DqmcError, HubbardParams, _lib
    # same offset and size as the word it replaces
    assert _lib.dethubbard_params.measureFlags.offset == 36 and _lib.dethubbard_params.measureFlags.size == 4
    assert C.sizeof(_lib.dethubbard_params) == 80
    seen = {}

    class _Spy:                                          # the loaded library with dethubbard_create replaced by a recorder
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def dethubbard_create(self, p, nchains, out):
            seen["flags"] = C.cast(p, C.POINTER(_lib.dethubbard_params)).contents.measureFlags
            return -1

    real = detqmc_amd.model.load
    detqmc_amd.model.load = lambda: _Spy(real())
    try:
        with pytest.raises(DqmcError):
            DetHubbard(HubbardParams(L=4, beta=2.0, equalTimeCorrelators=eq, timeDisplacedCorrelators=td))
    finally:
        detqmc_amd.model.load = real
    assert seen["flags"] == word
