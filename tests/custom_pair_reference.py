"""numpy reference of the user-defined pair operators (tests only).

Operator c is (F0, Fx, Fy), complex 4 x 4 each in the band-spin order XUP, YDOWN, XDOWN, YUP, None = zero:

    Delta_A = sum_ab F0_ab c_{A a} c_{A b} + sum_{mu = x, y} u_mu(A) sum_ab Fmu_ab c_{A (+) mu, a} c_{A b}

u_mu(A) = +-1 the antiperiodic sign of the bond A -> A (+) mu: link_table of tests/custom_bond_reference.py without flux (bond parts are
refused under flux).  No Hermitian conjugate is added.  The dense coefficient matrix D_A over index = flavour * N + site is built here;

    P(A, B) = <Delta_A(tau) Delta_B^+(0)> = sum_kl [Y_A - Y_A^T]_kl conj(D_B)_kl,      Y_A = g^T D_A g

with g the full shifted G(tau, 0) (time-displaced) or the full shifted G of the slice (equal time: <c c c^+ c^+> has no delta term).
C(d) = (1/N) sum_B Re P(B (+) d, B) by bin_periodic."""
import numpy as np

from custom_bond_reference import link_table
from td_current_reference import neighbours
from td_ph_reference import bin_periodic, expand

XUP, YDOWN, XDOWN, YUP = 0, 1, 2, 3


def _part(M):
    return np.zeros((4, 4), dtype=complex) if M is None else np.asarray(M, dtype=complex)


def as_arrays(op):
    """(F0, Fx, Fy) with zeros for None"""
    return tuple(_part(m) for m in op)


def link_signs(L, bc="pbc"):
    """u[mu, site] = +-1"""
    return link_table(L, bc, False)[:, 0, :].real


def dense_pair_operators(op, u, L):
    """D[A], N x 4N x 4N complex, of the operator op = (F0, Fx, Fy): Delta_A = sum_ij D[A]_ij c_i c_j"""
    N = L * L
    nbr = neighbours(L)
    F0, Fb = _part(op[0]), (_part(op[1]), _part(op[2]))
    D = np.zeros((N, 4 * N, 4 * N), dtype=complex)
    for A in range(N):
        for a in range(4):
            for b in range(4):
                D[A, a * N + A, b * N + A] += F0[a, b]
                for mu in range(2):
                    D[A, a * N + nbr[mu, A], b * N + A] += u[mu, A] * Fb[mu][a, b]
    return D


def pair_wick_all(g, D, D2=None):
    """P[A, B] for all pairs from the full matrix g; D2 (default D) the operators of the conjugated factor.  Y - Y^T is antisymmetric, so
    only the antisymmetric part of D_B is contracted with it: the same sum, and exactly zero for a symmetric D_B"""
    Y = np.einsum("ik,Aij,jl->Akl", g, D, g, optimize=True)
    DB = D if D2 is None else D2
    return np.einsum("Akl,Bkl->AB", Y - Y.transpose(0, 2, 1), np.conj(0.5 * (DB - DB.transpose(0, 2, 1))), optimize=True)


def pair_correlators_full(ops, u, L, g):
    """C(d), length N, for every operator from one FULL matrix"""
    return [bin_periodic(pair_wick_all(g, dense_pair_operators(op, u, L)), L) for op in ops]


def pair_correlators(ora, ops, gs):
    """the same from ONE SHIFTED engine matrix (n_g x n_g) of an oracle's model: gt0 time-displaced, G of the slice at equal time"""
    return pair_correlators_full(ops, link_signs(ora.L, ora.pars.bc), ora.L, expand(ora, gs))


def expand_unconjugated(ora, gs):
    """expand with the conjugation of the second sector dropped (OPDIM < 3): what a kernel that forgets the sector rule would use"""
    blocks = [[np.asarray(b, dtype=complex) for b in row] for row in ora._gl1_blocks(gs)]
    for r in (XDOWN, YUP):
        for c in (XDOWN, YUP):
            blocks[r][c] = np.conj(blocks[r][c])
    return np.block(blocks)


# ---- the operators the tests set -----------------------------------------------------------------------------------------------------
def _rand():
    rng = np.random.default_rng(2026)
    return tuple(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)) for _ in range(3))


def _singlet():
    S = np.zeros((4, 4), dtype=complex)
    S[XUP, XDOWN] = S[YUP, YDOWN] = 1.0
    S[XDOWN, XUP] = S[YDOWN, YUP] = -1.0
    return S


P_RAND = _rand()                                            # dense random complex (F0, Fx, Fy)
_SYM = P_RAND[1] + P_RAND[1].T
P_SYM_BOND = (_SYM, _singlet(), 1j * _singlet())            # F0 symmetric (contributes nothing) plus a bond part
_F_S = np.zeros((4, 4), dtype=complex)
_F_S[XUP, XDOWN] = _F_S[YUP, YDOWN] = 1.0
_F_D = _F_S.copy()
_F_D[YUP, YDOWN] = -1.0
P_S = (_F_S, None, None)                                    # the operator of pairPlus
P_DBAND = (_F_D, None, None)                                # the operator of pairMinus
P_ONSITE = (P_RAND[2], None, None)                          # on-site only, dense
P_TRIPLET_X = (None, np.diag([0.0, 0.0, 0.0, 0.0]).astype(complex) + np.eye(4, k=2) + np.eye(4, k=-2), None)   # inter-sector, symmetric: x bonds only


def pair_ops(flux=False):
    """the four operators of one launch; under flux the bond-carrying ones are replaced by on-site ones"""
    if flux:
        return [P_ONSITE, P_S, P_DBAND, (P_RAND[0], None, None)]
    return [P_RAND, P_SYM_BOND, P_ONSITE, P_TRIPLET_X]
