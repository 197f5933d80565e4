"""TEST INFRASTRUCTURE ONLY.  Numpy restatement of the Hubbard replica's correlators (include/dqmc_hip.h, "Hubbard model: equal-time
and time-displaced correlators") from spin-resolved N x N matrices, and the four Green's functions of a boundary from explicit B
products and a direct inverse.  tests/test_hubbard_corr_reference_cpu.py checks every form here against traces over the Fock space.

Conventions: G_s(A, B) = <c_As c^+_Bs>; G(tau,0)(A, B) = <c_A(tau) c^+_B(0)>; G(0,tau)(A, B) = -<c^+_B(tau) c_A(0)>; sites A = y L + x;
a channel is a matrix X[A, B], its bins are sum_B X[B (+) d, B] at index dy L + dx."""
import numpy as np

EQ_NAMES = ["greenUp", "greenDn", "charge", "spinZZ", "spinXX", "pairS", "pairSx", "pairD"]
TD_NAMES = EQ_NAMES[:6]
F_EXT_S = np.array([1.0, 1.0, 1.0, 1.0])        # form factor on XPLUS, XMINUS, YPLUS, YMINUS
F_D_WAVE = np.array([1.0, 1.0, -1.0, -1.0])


def neighbours(L):
    """[4][N]: XPLUS, XMINUS, YPLUS, YMINUS, periodic"""
    N = L * L
    nb = np.zeros((4, N), dtype=int)
    for site in range(N):
        x, y = site % L, site // L
        nb[0, site] = y * L + (x + 1) % L
        nb[1, site] = y * L + (x - 1) % L
        nb[2, site] = ((y + 1) % L) * L + x
        nb[3, site] = ((y - 1) % L) * L + x
    return nb


def bin_sum(X, L):
    """out[dy L + dx] = sum_B X[B (+) d, B]; leading axes are kept"""
    N = L * L
    B = np.arange(N)
    bx, by = B % L, B // L
    out = np.zeros(X.shape[:-2] + (N,))
    for d in range(N):
        A = ((by + d // L) % L) * L + (bx + d % L) % L
        out[..., d] = X[..., A, B].sum(axis=-1)
    return out


def _particle_hole(g_up, g_dn, h_up, h_dn, n_a, n_b):
    """charge, spinZZ, spinXX from g_s[A, B] = <c_As c^+_Bs>, h_s[A, B] = <c^+_As c_Bs> (displaced or not) and the occupations
    n_a[s][A] of the left operator's time, n_b[s][B] of the right one's"""
    conn = h_up * g_up + h_dn * g_dn
    charge = np.outer(n_a[0] + n_a[1], n_b[0] + n_b[1]) + conn
    spin_zz = 0.25 * (np.outer(n_a[0] - n_a[1], n_b[0] - n_b[1]) + conn)
    spin_xx = 0.25 * (h_up * g_dn + h_dn * g_up)
    return charge, spin_zz, spin_xx


def bond_pair(g_up, g_dn, f, L):
    """<Delta^f_A Delta^f+_B> = 1/4 sum_{dl, dl'} f_dl f_dl' G_up(A, B) G_dn(A + dl, B + dl')"""
    nb = neighbours(L)
    st = np.zeros_like(g_dn)
    for q in range(4):
        for r in range(4):
            st += f[q] * f[r] * g_dn[np.ix_(nb[q], nb[r])]
    return 0.25 * g_up * st


def eq_channels(g_up, g_dn, L):
    """[8][N][N] in the order EQ_NAMES from the equal-time G of both spins"""
    eye = np.eye(g_up.shape[0])
    n = [1.0 - np.diag(g_up), 1.0 - np.diag(g_dn)]
    charge, spin_zz, spin_xx = _particle_hole(g_up, g_dn, eye - g_up.T, eye - g_dn.T, n, n)
    return np.stack([g_up, g_dn, charge, spin_zz, spin_xx, g_up * g_dn, bond_pair(g_up, g_dn, F_EXT_S, L), bond_pair(g_up, g_dn, F_D_WAVE, L)])


def td_channels(gt0, g0t, gtt, g00):
    """[6][N][N] in the order TD_NAMES; every argument is a pair (up, down) of N x N matrices: G(tau,0), G(0,tau), G(tau), G(0)"""
    n_tau = [1.0 - np.diag(gtt[0]), 1.0 - np.diag(gtt[1])]
    n_0 = [1.0 - np.diag(g00[0]), 1.0 - np.diag(g00[1])]
    charge, spin_zz, spin_xx = _particle_hole(gt0[0], gt0[1], -g0t[0].T, -g0t[1].T, n_tau, n_0)
    return np.stack([gt0[0], gt0[1], charge, spin_zz, spin_xx, gt0[0] * gt0[1]])


def eq_corr(g_up, g_dn, L):
    """raw bins [8][N] of one configuration"""
    return bin_sum(eq_channels(g_up, g_dn, L), L)


def td_corr(gt0, g0t, gtt, g00, L):
    """raw bins [6][N] of one configuration and boundary"""
    return bin_sum(td_channels(gt0, g0t, gtt, g00), L)


def _inverse(M):
    """Gauss-Jordan with partial pivoting in the dtype of M (numpy.linalg has no extended precision)"""
    n = M.shape[0]
    W = np.concatenate([M.copy(), np.eye(n, dtype=M.dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(W[c:, c])))
        if p != c:
            W[[c, p]] = W[[p, c]]
        W[c] = W[c] / W[c, c]
        f = W[:, c].copy()
        f[c] = 0
        W -= np.outer(f, W[c])
    return W[:, n:]


def displaced_greens(Bs, l):
    """(G(tau_l,0), G(0,tau_l), G(tau_l), G(0)) of one spin from its slice matrices Bs = [B_1, .., B_m], B(l, 0) = B_l .. B_1:
        G(0) = [1 + B(m,0)]^-1,  G(tau) = [1 + B(l,0) B(m,l)]^-1,  G(tau,0) = B(l,0) G(0),  G(0,tau) = -(1 - G(0)) B(l,0)^-1
    by explicit products and direct inverses in extended precision -- adequate while the scales of B(m,0) stay far inside its range
    (beta = 2 here), no substitute for the stabilised path at low temperature"""
    ld = np.longdouble
    N = Bs[0].shape[0]
    eye = np.eye(N, dtype=ld)
    lo, hi = eye.copy(), eye.copy()
    for k in range(l):
        lo = Bs[k].astype(ld) @ lo                 # B(l, 0)
    for k in range(l, len(Bs)):
        hi = Bs[k].astype(ld) @ hi                 # B(m, l)
    g00 = _inverse(eye + hi @ lo)
    gtt = _inverse(eye + lo @ hi)
    gt0 = lo @ g00
    g0t = -(eye - g00) @ _inverse(lo)
    return tuple(np.asarray(x, dtype=np.float64) for x in (gt0, g0t, gtt, g00))
