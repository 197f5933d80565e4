"""numpy reference of the equal-time charge, spin-z, SDW and pairing correlators (tests only).

Built on what exists: the Wick form of tests/td_ph_reference.py with one equal-time matrix g in every role,

    W^M(A, B) = wick(g, g, g - 1, g, M, N)(A, B) = o^M(A) o^M(B) + sum_abcd M_ab M_cd [delta_(Aa,Bd) - g(B d; A a)] g(A b; B c),

and the T+- of tests/td_pair_reference.py evaluated on g.  C(d) = (1/N) sum_B Re W(B (+) d, B) over the periodic site differences
d = (dx, dy), bin dy L + dx, and S(q) = sum_d cos(q . d) C(d), column qy L + qx with q = 2 pi (qx, qy) / L."""
import numpy as np

from td_pair_reference import pair_correlators
from td_ph_reference import M_CHARGE, M_SDW, M_SPINZ, bin_periodic, expand, wick

NAMES = ("charge", "spinZ", "sdw", "pairPlus", "pairMinus")


def wick_eq(gfull, M, ns):
    """W^M, ns x ns complex, entry (A, B), from ONE full equal-time matrix (4 ns x 4 ns, index = flavour * ns + site)"""
    return wick(gfull, gfull, gfull - np.eye(gfull.shape[0]), gfull, M, ns)


def eq_correlators(ora, gs):
    """(charge, spinZ, sdw, pairPlus, pairMinus), each of length N, from the SHIFTED engine matrix gs (n_g x n_g)"""
    N, L, opdim = ora.N, ora.L, ora.OPDIM
    full = expand(ora, gs)
    out = [bin_periodic(wick_eq(full, M, N), L) for M in (M_CHARGE, M_SPINZ)]
    out.append(sum(bin_periodic(wick_eq(full, M, N), L) for M in M_SDW[:opdim]) / opdim)
    out.extend(pair_correlators(ora, gs))
    return tuple(out)


def structure_factor(c, L):
    """S(q) = sum_d cos(q . d) C(d), explicit loops; c of length L^2"""
    N = L * L
    s = np.zeros(N)
    for q in range(N):
        qx, qy = q % L, q // L
        for d in range(N):
            dx, dy = d % L, d // L
            s[q] += np.cos(2.0 * np.pi * (qx * dx + qy * dy) / L) * c[d]
    return s


def fourier_full(c, L):
    """sum_d e^{-i q . d} C(d), complex, by the FFT: the full sum whose real part the cosine sum is"""
    return np.fft.fft2(np.asarray(c, dtype=complex).reshape(L, L)).reshape(-1)
