"""numpy reference of the user-defined bilinears with nearest-neighbour bond parts (tests only).

Operator c is (M0, Mx, My), 4 x 4 each in the band-spin order XUP, YDOWN, XDOWN, YUP, M0 Hermitian, None = zero:

    O_A = sum_ab c^+_{A a} M0_ab c_{A b} + sum_{mu = x, y} sum_ab [ u^ab_mu(A) Mmu_ab c^+_{A (+) mu, a} c_{A b} + h.c. ]

u the unit-modulus link factor of the hopping bond: bond_table_band of tests/td_current_reference.py with every hopping set to -1
(T = -t u), complex conjugated for the flavours XDOWN, YUP like the amplitudes of bond_table.  Entry (a, b) takes flavour a's link, which
without flux is the same +-1 for every flavour; with flux only diagonal bond parts are defined.

The dense one-body matrix of O_A over index = flavour * N + site is built here; the correlators are the general Wick formula of
wick_dense (tests/td_current_reference.py) on it -- evaluated for all site pairs at once through tr(O_A gt0 O_B g0t), which
test_custom_bonds_cpu.py checks against wick_dense pair by pair -- binned by bin_periodic; equal time with (g, g, g - 1, g) as wick_eq."""
import numpy as np

from custom_reference import M_RAND
from td_current_reference import FLAVOUR_CONJ, bond_table_band, neighbours
from td_ph_reference import bin_periodic, expand


def link_table(L, bc="pbc", weakZflux=False):
    """u[mu, flavour, site] for the four flavours"""
    t = bond_table_band(L, 0, -1.0, -1.0, -1.0, -1.0, bc, weakZflux)          # -t = +1: the sign and the phase alone
    return np.stack([np.conj(t) if FLAVOUR_CONJ[a] else t for a in range(4)], axis=1)


def _part(M):
    return np.zeros((4, 4), dtype=complex) if M is None else np.asarray(M, dtype=complex)


def dense_operators(op, u, L):
    """O[A], N x 4N x 4N complex, of the operator op = (M0, Mx, My)"""
    N = L * L
    nbr = neighbours(L)
    M0, Mb = _part(op[0]), (_part(op[1]), _part(op[2]))
    O = np.zeros((N, 4 * N, 4 * N), dtype=complex)
    for A in range(N):
        for a in range(4):
            for b in range(4):
                O[A, a * N + A, b * N + A] += M0[a, b]
                for mu in range(2):
                    v = u[mu, a, A] * Mb[mu][a, b]
                    An = nbr[mu, A]
                    O[A, a * N + An, b * N + A] += v
                    O[A, b * N + A, a * N + An] += np.conj(v)
    return O


def one_body_all(g, O):
    """o(A) = tr O_A - sum_ij (O_A)_ij g(j; i) for every A"""
    return np.einsum("Aii->A", O) - np.einsum("Aij,ji->A", O, g)


def wick_all(gtt, gt0, g0t, g00, O):
    """W[A, B] = wick_dense(gtt, gt0, g0t, g00, O[A], O[B]) for all pairs: the connected part is tr(O_A gt0 O_B g0t)"""
    X, Y = O @ gt0, O @ g0t
    return np.outer(one_body_all(gtt, O), one_body_all(g00, O)) - np.einsum("Apq,Bqp->AB", X, Y)


def bond_correlators_full(ops, u, L, gtt, gt0, g0t, g00):
    """C(d), length N, for every operator from four FULL matrices"""
    return [bin_periodic(wick_all(gtt, gt0, g0t, g00, dense_operators(op, u, L)), L) for op in ops]


def _links(ora):
    return link_table(ora.L, ora.pars.bc, ora.pars.weakZflux)


def bond_correlators(ora, ops, gtt_s, gt0_s, g0t_s, g00_s):
    """the same from the four SHIFTED engine matrices (n_g x n_g) of an oracle's model"""
    return bond_correlators_full(ops, _links(ora), ora.L, *[expand(ora, g) for g in (gtt_s, gt0_s, g0t_s, g00_s)])


def eq_bond_correlators(ora, ops, gs):
    """equal time: ONE shifted engine matrix in every role, g - 1 in the role of g0t"""
    g = expand(ora, gs)
    return bond_correlators_full(ops, _links(ora), ora.L, g, g, g - np.eye(g.shape[0]), g)


# ---- the operators the tests set -----------------------------------------------------------------------------------------------------
def _rand():
    rng = np.random.default_rng(2025)
    a = [rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)) for _ in range(3)]
    return 0.5 * (a[0] + a[0].conj().T), a[1], a[2]


B_RAND = _rand()
B_RAND_FLUX = (B_RAND[0], np.diag(np.diag(B_RAND[1])), np.diag(np.diag(B_RAND[2])))
B_DDW = (None, 1j * np.eye(4), -1j * np.eye(4))
B_ONSITE = (M_RAND, None, None)


def bond_ops(pars, flux=False):
    """(B_RAND, B_KIN_X, B_DDW, B_ONSITE) for a model with the hoppings of pars; under flux B_RAND's bond parts are their diagonals"""
    from detqmc_amd import bond_kinetic
    return [B_RAND_FLUX if flux else B_RAND, bond_kinetic(pars, "x"), B_DDW, B_ONSITE]


def as_arrays(op):
    """(M0, Mx, My) with zeros for None"""
    return tuple(_part(m) for m in op)
