"""numpy reference of the time-displaced current-current correlators and the bond kinetic energy (tests only).

Bond operators.  For a direction mu in {x, y}, a site i, its neighbour i' = i (+) mu and a flavour alpha, T_alpha(i) = K^alpha[i', i] is the
coefficient of c^+_{i' alpha} c_{i alpha} in the hopping matrix.  With a_alpha(i) = i T_alpha(i) (current j_mu(i)) or a_alpha(i) = T_alpha(i)
(bond kinetic energy k_mu(i)) the one-body matrix of the bond operator is

    M[i' alpha, i alpha] = a_alpha(i),     M[i alpha, i' alpha] = conj a_alpha(i),

Hermitian and traceless.  Wick's theorem in the form of tests/td_ph_reference.py (same Green's function conventions),

    o_t[M]       = tr M - sum_pq M_pq g_t(q, p)
    W[M_A, M_B]  = o_tau[M_A] o_0[M_B] - sum_pqrs (M_A)_pq (M_B)_rs g0t(s, p) gt0(q, r),

is written out here for that two-entry structure, vectorised over all sites (no dense M per bond): with A^1 = A', A^0 = A, a_1 = a,
a_0 = conj a and the same for B,

    o_t(A)     = - sum_alpha [ a_alpha(A) g_t(A alpha; A' alpha) + conj a_alpha(A) g_t(A' alpha; A alpha) ]
    conn(A, B) = sum_{alpha beta} sum_{u v} a_u^alpha(A) b_v^beta(B) g0t(B^(1-v) beta; A^u alpha) gt0(A^(1-u) alpha; B^v beta).

wick_dense is the general formula for arbitrary dense M (used to check the written-out form and, against exact diagonalisation, itself).
Full matrices: index = flavour * nsites + site, flavour order XUP, YDOWN, XDOWN, YUP for the lattice model."""
import math

import numpy as np

from td_ph_reference import bin_periodic, expand

FLAVOUR_BAND = (0, 1, 0, 1)          # XUP, YDOWN, XDOWN, YUP
FLAVOUR_CONJ = (False, False, True, True)


def neighbours(L):
    """nbr[mu, site] = site (+) mu, mu = 0: x, 1: y"""
    s = np.arange(L * L)
    x, y = s % L, s // L
    return np.stack([y * L + (x + 1) % L, ((y + 1) % L) * L + x])


def bond_table_band(L, band, txhor, txver, tyhor, tyver, bc="pbc", weakZflux=False):
    """T[mu, site] of one band's stored sector: -t, sign flipped on a bond that crosses an antiperiodic boundary, Peierls phase
    e^{+2 pi i y / N} on x bonds and e^{-2 pi i L x / N} on the y bonds that cross the boundary"""
    N = L * L
    s = np.arange(N)
    x, y = s % L, s // L
    hor, ver = ((txhor, txver), (tyhor, tyver))[band]
    tx = -hor * np.ones(N, dtype=complex)
    ty = -ver * np.ones(N, dtype=complex)
    if bc in ("apbc-x", "apbc-xy"):
        tx[x == L - 1] *= -1
    if bc in ("apbc-y", "apbc-xy"):
        ty[y == L - 1] *= -1
    if weakZflux:
        zm = 1.0 / N
        tx *= np.exp(2j * math.pi * zm * y)
        ty *= np.where(y == L - 1, np.exp(-2j * math.pi * zm * L * x), 1.0)
    return np.stack([tx, ty])


def bond_table(ora):
    """T[mu, flavour, site] for the four flavours of the oracle's model"""
    p = ora.pars
    bands = [bond_table_band(ora.L, b, p.txhor, p.txver, p.tyhor, p.tyver, p.bc, p.weakZflux) for b in (0, 1)]
    T = np.zeros((2, 4, ora.N), dtype=complex)
    for a in range(4):
        t = bands[FLAVOUR_BAND[a]]
        T[:, a] = np.conj(t) if FLAVOUR_CONJ[a] else t
    return T


def hopping_from_bonds(T, nbr, mu):
    """dense K = -mu 1 + sum_bonds [T(i) |i'><i| + h.c.] of one flavour; T[mu, site]"""
    N = T.shape[1]
    K = -mu * np.eye(N, dtype=complex)
    s = np.arange(N)
    for d in range(2):
        np.add.at(K, (nbr[d], s), T[d])
        np.add.at(K, (s, nbr[d]), np.conj(T[d]))
    return K


def bond_matrix(a, nb, i, nflav):
    """dense M of the bond operator at site i; a[flavour, site], nb[site]"""
    ns = a.shape[1]
    M = np.zeros((nflav * ns, nflav * ns), dtype=complex)
    for f in range(nflav):
        M[f * ns + nb[i], f * ns + i] += a[f, i]
        M[f * ns + i, f * ns + nb[i]] += np.conj(a[f, i])
    return M


def one_body_dense(g, M):
    return np.trace(M) - np.sum(M * g.T)


def wick_dense(gtt, gt0, g0t, g00, MA, MB):
    """W[M_A, M_B] of the general formula"""
    conn = np.einsum("pq,rs,sp,qr->", MA, MB, g0t, gt0)
    return one_body_dense(gtt, MA) * one_body_dense(g00, MB) - conn


def one_body_bond(g, a, nb):
    """o_t(A) for every site A; g full, a[flavour, site], nb[site]"""
    F, ns = a.shape
    G = g.reshape(F, ns, F, ns)
    f, s = np.arange(F)[:, None], np.arange(ns)[None, :]
    fwd = G[f, s, f, nb[None, :]]                   # g(A alpha; A' alpha)
    back = G[f, nb[None, :], f, s]                  # g(A' alpha; A alpha)
    return -np.sum(a * fwd + np.conj(a) * back, axis=0)


def wick_bond(gtt, gt0, g0t, g00, a, b, nb):
    """W[A, B], ns x ns complex, of the bond operators with coefficients a (time tau, site A) and b (time 0, site B) along nb"""
    F, ns = a.shape
    GT0 = gt0.reshape(F, ns, F, ns)
    G0T = g0t.reshape(F, ns, F, ns).transpose(2, 3, 0, 1)        # [alpha, A, beta, B] = g0t(B beta; A alpha)
    site = [np.arange(ns), nb]
    conn = np.zeros((ns, ns), dtype=complex)
    for u in (0, 1):
        au = a if u else np.conj(a)
        for v in (0, 1):
            bv = b if v else np.conj(b)
            X = G0T[:, site[u]][:, :, :, site[1 - v]]
            Y = GT0[:, site[1 - u]][:, :, :, site[v]]
            conn += np.einsum("aA,bB,aAbB,aAbB->AB", au, bv, X, Y)
    return np.outer(one_body_bond(gtt, a, nb), one_body_bond(g00, b, nb)) - conn


def current_correlators_full(gtt, gt0, g0t, g00, T, L):
    """from four FULL matrices and T[mu, flavour, site]: (Lambda_xx[N], Lambda_yy[N], kinetic_x, kinetic_y)"""
    nbr = neighbours(L)
    lam, kin = [], []
    for d in range(2):
        W = wick_bond(gtt, gt0, g0t, g00, 1j * T[d], 1j * T[d], nbr[d])
        lam.append(bin_periodic(W, L))
        kin.append(float(np.sum(one_body_bond(gtt, T[d], nbr[d]).real)) / (L * L))
    return lam[0], lam[1], kin[0], kin[1]


def current_correlators(ora, gtt_s, gt0_s, g0t_s, g00_s):
    """the same from the four SHIFTED engine matrices (n_g x n_g) of an oracle's model"""
    full = [expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)]
    return current_correlators_full(*full, bond_table(ora), ora.L)


def free_fermion_closed_form(L, beta, txhor, txver, tyhor, tyver, mux, muy):
    """((sum_d Lambda_xx, sum_d Lambda_yy), (kinetic_x, kinetic_y)) of the uncoupled model with periodic boundaries"""
    k = 2.0 * math.pi * np.arange(L) / L
    kx, ky = k[None, :], k[:, None]
    lam, kin = [0.0, 0.0], [0.0, 0.0]
    for a in range(4):
        hor, ver, mu = ((txhor, txver, mux), (tyhor, tyver, muy))[FLAVOUR_BAND[a]]
        eps = -mu - 2.0 * hor * np.cos(kx) - 2.0 * ver * np.cos(ky)
        f = 1.0 / (np.exp(beta * eps) + 1.0)
        for d, (t, kk) in enumerate(((hor, kx), (ver, ky))):
            lam[d] += float(np.sum((2.0 * t * np.sin(kk)) ** 2 * f * (1.0 - f))) / (L * L)
            kin[d] += float(np.sum(-2.0 * t * np.cos(kk) * f)) / (L * L)
    return tuple(lam), tuple(kin)
