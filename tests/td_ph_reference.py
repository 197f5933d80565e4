"""numpy reference of the time-displaced particle-hole correlators (tests only).

For a site bilinear O^M_i = sum_ab c^+_ia M_ab c_ib (M a 4 x 4 matrix in band-spin space, order XUP, YDOWN, XDOWN, YUP) and the four
Green's functions of one boundary -- G(tau,0)_ab = <c_a(tau) c_b^+(0)>, G(0,tau)_ab = -<c_b^+(tau) c_a(0)>, G(tau) and G(0) = <c c^+> at
equal time -- Wick's theorem per field configuration gives

    o^M_t(A)  = tr M - sum_ab M_ab g_t(A b; A a)
    W^M(A, B) = o^M_tau(A) o^M_0(B) - sum_abcd M_ab M_cd g0t(B d; A a) gt0(A b; B c).

Everything here works on FULL matrices with index = flavour * nsites + site; matrices of the engine are expanded with the oracle's
_gl1_blocks (imported, not restated).  C(d) = (1/N) sum_B Re W(B (+) d, B) over the periodic site differences d = (dx, dy), bin dy L + dx."""
import numpy as np

M_CHARGE = np.eye(4, dtype=complex)
M_SPINZ = 0.5 * np.diag([1.0, -1.0, -1.0, 1.0]).astype(complex)
M_X = np.zeros((4, 4), dtype=complex)
M_Y = np.zeros((4, 4), dtype=complex)
M_Z = np.zeros((4, 4), dtype=complex)
M_X[0, 1] = M_X[1, 0] = M_X[2, 3] = M_X[3, 2] = 1.0
M_Y[0, 1], M_Y[1, 0], M_Y[2, 3], M_Y[3, 2] = -1j, 1j, 1j, -1j
M_Z[0, 3] = M_Z[3, 0] = 1.0
M_Z[1, 2] = M_Z[2, 1] = -1.0
M_SDW = (M_X, M_Y, M_Z)


def greens_from_b(bt0, bbt):
    """(G(tau), G(tau,0), G(0,tau), G(0)) by direct inverses from B(tau,0) and B(beta,tau)"""
    inv, eye = np.linalg.inv, np.eye(bt0.shape[0])
    return inv(eye + bt0 @ bbt), inv(inv(bt0) + bbt), -inv(bt0 + inv(bbt)), inv(eye + bbt @ bt0)


def four_greens(chain, tau):
    """the same for a td_reference.Chain at time slice tau"""
    return greens_from_b(chain.B(tau, 0), chain.B(chain.ora.m, tau))


def one_body(g, M, ns):
    """o^M(A), length ns, of an equal-time matrix g (full, 4 ns x 4 ns)"""
    G = g.reshape(4, ns, 4, ns)
    return np.trace(M) - np.einsum("ab,bAaA->A", M, G)


def wick(gtt, gt0, g0t, g00, M, ns):
    """W^M, ns x ns complex, entry (A, B); all four matrices full (4 ns x 4 ns)"""
    GT0, G0T = gt0.reshape(4, ns, 4, ns), g0t.reshape(4, ns, 4, ns)
    conn = np.einsum("ab,cd,dBaA,bAcB->AB", M, M, G0T, GT0)
    return np.outer(one_body(gtt, M, ns), one_body(g00, M, ns)) - conn


def expand(ora, g):
    """full 4N x 4N matrix of an engine matrix (n_g x n_g) by the access rule of the equal-time measurement"""
    return np.block([[np.asarray(b, dtype=complex) for b in row] for row in ora._gl1_blocks(g)])


def bin_periodic(W, L):
    """C(d) = (1/N) sum_B Re W(B (+) d, B), d = dy L + dx"""
    N = L * L
    x, y = np.arange(N) % L, np.arange(N) // L
    bins = ((y[:, None] - y[None, :]) % L) * L + (x[:, None] - x[None, :]) % L      # [A, B] -> dy L + dx
    c = np.zeros(N)
    np.add.at(c, bins, W.real)
    return c / N


def ph_correlators(ora, gtt_s, gt0_s, g0t_s, g00_s):
    """(charge, spinZ, sdw), each of length N, from the four SHIFTED engine matrices"""
    N, L, opdim = ora.N, ora.L, ora.OPDIM
    full = [expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)]
    out = [bin_periodic(wick(*full, M, N), L) for M in (M_CHARGE, M_SPINZ)]
    out.append(sum(bin_periodic(wick(*full, M, N), L) for M in M_SDW[:opdim]) / opdim)
    return tuple(out)
