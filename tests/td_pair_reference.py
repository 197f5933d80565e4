"""numpy reference of the time-displaced pairing correlators (tests only).

T+-(A, B) are the pairPlus / pairMinus expressions of the oracle's measureFermionic (reference detsdwopdim.cpp:695-715), term for
term and in the same order, for every site pair at once; the band-spin access rule is the oracle's _gl1_blocks (imported, not restated).
C+-(d) = (1/N) sum_B Re T+-(B (+) d, B) over the periodic site differences d = (dx, dy), bin dy L + dx."""
import numpy as np

XUP, YDOWN, XDOWN, YUP = 0, 1, 2, 3
X, Y, UP, DN = 0, 1, 0, 1


def _bs(band, spin):
    """getBandSpin (detsdwopdim.h:268-273)"""
    if band == X:
        return XUP if spin == UP else XDOWN
    return YUP if spin == UP else YDOWN


def pair_terms(ora, gs):
    """(T+, T-), each N x N complex: entry (A, B) for the site pair (A, B) of the shifted matrix gs"""
    B = ora._gl1_blocks(gs)

    def gl(b1, s1, b2, s2):
        return np.asarray(B[_bs(b1, s1)][_bs(b2, s2)], dtype=complex)

    t = [gl(X, DN, X, UP) * gl(X, UP, X, DN), gl(X, DN, X, DN) * gl(X, UP, X, UP),
         gl(X, DN, Y, UP) * gl(X, UP, Y, DN), gl(X, DN, Y, DN) * gl(X, UP, Y, UP),
         gl(Y, DN, X, UP) * gl(Y, UP, X, DN), gl(Y, DN, X, DN) * gl(Y, UP, X, UP),
         gl(Y, DN, Y, UP) * gl(Y, UP, Y, DN), gl(Y, DN, Y, DN) * gl(Y, UP, Y, UP)]
    plus = -4.0 * (t[0] - t[1] + t[2] - t[3] + t[4] - t[5] + t[6] - t[7])
    minus = -4.0 * (t[0] - t[1] - t[2] + t[3] - t[4] + t[5] + t[6] - t[7])
    return plus, minus


def pair_correlators(ora, gs):
    """(C+, C-), each of length N: the translation average of Re T+- over the periodic site differences"""
    L, N = ora.L, ora.N
    plus, minus = pair_terms(ora, gs)
    x, y = np.arange(N) % L, np.arange(N) // L
    bins = ((y[:, None] - y[None, :]) % L) * L + (x[:, None] - x[None, :]) % L      # [A, B] -> dy L + dx
    cp, cm = np.zeros(N), np.zeros(N)
    np.add.at(cp, bins, plus.real)
    np.add.at(cm, bins, minus.real)
    return cp / N, cm / N
