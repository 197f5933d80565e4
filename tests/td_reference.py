"""Direct numpy reference for the time-displaced Green's functions (small beta only: plain inverses of B-matrix products).

The B matrices come from the CPU oracle (oracle/detsdw_oracle.py, imported, not restated); the symmetric shift is the
oracle's shiftGreenSymmetric applied to G(tau, 0)."""
import numpy as np

from detsdw_oracle import DetSDWOracle, SDWParams


def make_oracle(phi, **kw):
    """oracle replica with the given field (m+1, N, OPDIM); kw: oracle SDWParams (beta, dtau, s, ...)"""
    return DetSDWOracle(SDWParams(**kw).finalize(), phi=phi)


class Chain:
    """B(k2, k1) products of one field configuration from the oracle's single-slice B matrices"""

    def __init__(self, ora):
        self.ora = ora
        eye = np.eye(ora.ng, dtype=complex)
        self.Bk = [None] + [ora.leftMultiplyBmat(eye.copy(), k, k - 1) for k in range(1, ora.m + 1)]

    def B(self, k2, k1):
        out = np.eye(self.ora.ng, dtype=complex)
        for k in range(k1 + 1, k2 + 1):
            out = self.Bk[k] @ out
        return out

    def greens(self, tau):
        """G(tau), G(tau, 0) = [B(tau,0)^-1 + B(beta,tau)]^-1, G(0, tau) = -[B(tau,0) + B(beta,tau)^-1]^-1"""
        bt0, bbt = self.B(tau, 0), self.B(self.ora.m, tau)
        inv = np.linalg.inv
        g = inv(np.eye(self.ora.ng) + bt0 @ bbt)
        return g, inv(inv(bt0) + bbt), -inv(bt0 + inv(bbt))


def shift_symmetric(ora, g):
    """e^{-dtau K/2} g e^{+dtau K/2} (the oracle's shiftGreenSymmetric on another matrix)"""
    saved = ora.g
    ora.g = g
    try:
        return ora.shiftGreenSymmetric()
    finally:
        ora.g = saved


def green_k(ora, gs, bc="pbc"):
    """(G_X(k), G_Y(k)), k = site index of the kOcc grid: Re (1/2N) sum_spin sum_{a,b} e^{i k (r_a - r_b)} gs_{(a,band,spin),(b,band,spin)}"""
    L, N = ora.L, ora.N
    x, y = np.arange(N) % L, np.arange(N) // L
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    offx = 0.5 if bc in ("apbc-x", "apbc-xy") else 0.0
    offy = 0.5 if bc in ("apbc-y", "apbc-xy") else 0.0

    def blk(bs):
        if ora.OPDIM == 3:
            return gs[N * bs:N * (bs + 1), N * bs:N * (bs + 1)]
        if bs < 2:
            return gs[N * bs:N * (bs + 1), N * bs:N * (bs + 1)]
        return np.conj(gs[N * (bs - 2):N * (bs - 1), N * (bs - 2):N * (bs - 1)])

    # band-spin index (getBandSpin): X up 0, X down 2, Y up 3, Y down 1
    sectors = {0: blk(0) + blk(2), 1: blk(3) + blk(1)}
    out = np.zeros((2, N))
    for ks in range(N):
        kx = -np.pi + (ks % L + offx) * 2 * np.pi / L
        ky = -np.pi + (ks // L + offy) * 2 * np.pi / L
        ph = np.exp(1j * (kx * dx + ky * dy))
        for band in (0, 1):
            out[band, ks] = np.real(np.sum(ph * sectors[band])) / (2.0 * N)
    return out
