"""Extended-precision reference of the model kernels: B-multiply chains, the symmetric Green's-function shift, the per-slice
fermionic accumulators and the small field kernels.  Plain numpy in long double (x87 80-bit: 64-bit significand), no GPU.

The lattice description (plaquette sites and 4 x 4 factors, neighbour table, chemical potentials, e^{sign dtau V} per site, the
dense half propagators of checkerboard = False) is taken from oracle/detsdw_oracle.py as float64 TABLES and promoted; what is
restated here is only how a kernel combines them.  tests/test_model_reference_cpu.py pins this file to the committed goldens
and to the oracle so that it cannot drift together with the kernels.

Every operation returns the value and its MAGNITUDE COMPANION: the same sequence of operations with every factor and the operand
replaced by its elementwise |re| + |im|.  A rounding-error bound of the operation is (operation count) x u x companion.

Conventions as in the oracle: matrices are [row, col], site = y L + x, block b of an n_g = MSF N matrix holds band b & 1,
phi is (m+1, N, OPDIM) with slice 0 unused."""
import math

import numpy as np

from detsdw_oracle import DetSDWOracle, SDWParams

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(np.longdouble).nmant >= 63, \
    "tests/model_reference.py needs an extended-precision long double (>= 64-bit significand); this platform's has %d bits" \
    % (np.finfo(np.longdouble).nmant + 1)
U = 2.0 ** -53                 # unit roundoff of fp64
LEFT, RIGHT = 0, 1


def abs1(a):
    """|re| + |im| in float64 (an upper bound of the modulus; the companions need no extended precision)"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.abs(a.real).astype(np.float64) + np.abs(a.imag).astype(np.float64)
    return np.abs(a).astype(np.float64)


def make_lattice(**kw):
    """The oracle's lattice and hopping tables for the given oracle SDWParams WITHOUT its constructor's field set-up and
    Green's function (an SVD chain of n_g^3 cost, out of reach at n_g = 2304 and not needed here)."""
    p = SDWParams(**kw).finalize()
    o = DetSDWOracle.__new__(DetSDWOracle)
    o.pars = p
    o.OPDIM = p.opdim
    o.MSF = 4 if p.opdim == 3 else 2
    o.N, o.L, o.m, o.s, o.n = p.N, p.L, p.m, p.s, p.n
    o.ng = o.MSF * o.N
    o.dtau = p.dtau
    o._setup_lattice()
    o._setup_hopping()
    return o


class ModelReference:
    def __init__(self, lat):
        self.lat = lat
        self.p = lat.pars
        self.N, self.L, self.m, self.MSF, self.ng, self.OPDIM = lat.N, lat.L, lat.m, lat.MSF, lat.ng, lat.OPDIM
        self.dtau = lat.dtau

    # ------------------------------------------------------------------ caches
    def cosh_sinh(self, phi):
        """k_cosh_sinh: cosh(lambda dtau |phi|), sinh(lambda dtau |phi|) / |phi| for slices 1..m (slice 0: zeros), long double"""
        ph = np.asarray(phi, dtype=LD)
        nrm = np.sqrt(np.sum(ph * ph, axis=2))
        a = LD(self.p.lambda_) * LD(self.dtau) * nrm
        ch = np.zeros_like(nrm)
        sh = np.zeros_like(nrm)
        ch[1:] = np.cosh(a[1:])
        sh[1:] = np.sinh(a[1:]) / nrm[1:]
        return ch, sh

    def cdw_terms(self, cdwl):
        """k_cdw_terms: cosh / sinh(sqrt(dtau) cdwU eta(l)) per (slice, site); eta from the oracle (detsdwopdim.h:1222-1235)"""
        l = np.asarray(cdwl)
        eta = np.zeros(l.shape, dtype=LD)
        s6 = np.sqrt(LD(6))
        eta[np.abs(l) == 1] = np.sqrt(2 * (3 - s6))
        eta[np.abs(l) == 2] = np.sqrt(2 * (3 + s6))
        eta = eta * np.sign(l)
        arg = np.sqrt(LD(self.dtau)) * LD(self.p.cdwU) * eta
        return np.cosh(arg), np.sinh(arg)

    # ------------------------------------------------------------------ sparse factors acting on the leading axis
    def _plaq(self, X, Xa, blk0, sub, mats, transpose):
        """rows blk0 + sites of every plaquette of subgroup `sub` <- 4 x 4 factor times those rows (all trailing columns at once);
        transpose: the factor transposed (a RIGHT multiply seen from the transposed operand)"""
        q = self.lat.plaq_sites[sub] + blk0                  # [P, 4]
        M = np.asarray(mats)
        if transpose:
            M = np.transpose(M, (0, 2, 1))
        Ml = M.astype(CLD)
        Ma = abs1(M)
        if self.p.weakZflux:
            # with flux the 4 x 4 factors come out of a Hermitian eigen-decomposition in fp64 (LAPACK in the oracle and the real
            # reference, Jacobi on the device's host side): accurate NORM-wise only, |dM_ij| <= p u ||M||_2 whatever |M_ij| is (some
            # entries are products of two sinh, a hundred times smaller than the norm), so the companion carries ||M||_2 in every entry
            Ma = Ma + np.linalg.norm(Ma, 2, axis=(1, 2))[:, None, None]
        rows = [X[q[:, c]] for c in range(4)]
        rowsa = [Xa[q[:, c]] for c in range(4)]
        for a in range(4):
            acc = Ml[:, a, 0, None] * rows[0]
            acca = Ma[:, a, 0, None] * rowsa[0]
            for c in range(1, 4):
                acc = acc + Ml[:, a, c, None] * rows[c]
                acca = acca + Ma[:, a, c, None] * rowsa[c]
            X[q[:, a]] = acc
            Xa[q[:, a]] = acca

    def _hop(self, X, Xa, sign, transpose):
        """e^{sign dtau K1/2} e^{sign dtau K0} e^{sign dtau K1/2} on every band block (detsdwopdim.cpp:1839-1869, 1948-1979)"""
        for b in range(self.MSF):
            band = b & 1
            for sub, half in ((1, True), (0, False), (1, True)):
                self._plaq(X, Xa, b * self.N, sub, self.lat.plaq_mats[(band, sub, half, sign)], transpose)

    def _V(self, sign, k, phi, ch, sh, cdw):
        """e^{sign dtau V(phi_k)} per site as [MSF, MSF, N] in long double: the oracle's evMatrix entry by entry"""
        M, N = self.MSF, self.N
        c = np.asarray(ch[k], dtype=LD)
        x = np.asarray(sh[k], dtype=LD)
        cd, cmd = c, c
        if cdw is not None:
            cC, sC = cdw[0][k], cdw[1][k]
            cd = c * cC - sign * sC
            cmd = c * cC + sign * sC
            x = x * cC
        p0 = np.asarray(phi[k, :, 0], dtype=LD)
        p1 = np.asarray(phi[k, :, 1], dtype=LD) if self.OPDIM > 1 else np.zeros(N, dtype=LD)
        b = (p0 - 1j * p1) * x
        bc = (p0 + 1j * p1) * x
        V = np.zeros((M, M, N), dtype=CLD)
        V[0, 0], V[1, 1] = cd, cmd
        V[0, 1], V[1, 0] = sign * b, sign * bc
        if self.OPDIM == 3:
            ax = np.asarray(phi[k, :, 2], dtype=LD) * x
            V[2, 2], V[3, 3] = cd, cmd
            V[0, 3] = V[3, 0] = sign * ax
            V[1, 2] = V[2, 1] = -sign * ax
            V[3, 2], V[2, 3] = sign * b, sign * bc
        return V

    def _mix(self, X, Xa, V, transpose):
        M, N = self.MSF, self.N
        Va = abs1(V)
        blocks = [X[b * N:(b + 1) * N].copy() for b in range(M)]
        blocksa = [Xa[b * N:(b + 1) * N].copy() for b in range(M)]
        for o in range(M):
            acc = 0
            acca = 0
            for b in range(M):
                v = V[b, o] if transpose else V[o, b]
                va = Va[b, o] if transpose else Va[o, b]
                acc = acc + v[:, None] * blocks[b]
                acca = acca + va[:, None] * blocksa[b]
            X[o * N:(o + 1) * N] = acc
            Xa[o * N:(o + 1) * N] = acca

    def _scale(self, X, Xa, sign):
        for b in range(self.MSF):
            f = np.exp(LD(sign) * LD(self.dtau) * LD(self.lat.mu_band[b & 1]))
            X[b * self.N:(b + 1) * self.N] *= f
            Xa[b * self.N:(b + 1) * self.N] *= float(f)

    def _dense_half(self):
        self.lat._dense_propK()
        return self.lat

    def apply_B(self, A, side, inverse, k2, k1, phi, cdwl=None, cosh=None, sinh=None):
        """B(k2, k1) A, B(k2, k1)^-1 A, A B(k2, k1), A B(k2, k1)^-1 as the chain of sparse slice factors
        B_k = e^{-dtau V_k} diag(e^{dtau mu_band}) e^{-dtau K}; returns (value [clongdouble], magnitude companion [float64]).
        cosh / sinh: the (m+1, N) caches to use instead of long-double ones computed from phi (the device's own, to leave the
        cache kernel out of a B-multiply comparison)."""
        assert 0 <= k1 < k2 <= self.m
        if cosh is None:
            cosh, sinh = self.cosh_sinh(phi)
        cdw = self.cdw_terms(cdwl) if self.p.cdwU else None
        right = side == RIGHT
        X = np.array(A, dtype=CLD)
        Xa = abs1(A)
        if right:                                  # A B = (B^T A^T)^T: the factors transposed, in reverse order
            X, Xa = np.ascontiguousarray(X.T), np.ascontiguousarray(Xa.T)
        ascending = (not inverse) if not right else bool(inverse)
        ks = range(k1 + 1, k2 + 1) if ascending else range(k2, k1, -1)
        hop_first = right == bool(inverse)         # B A and A B^-1: the hopping part meets the operand first
        sign = +1 if inverse else -1
        for k in ks:
            V = self._V(sign, k, phi, cosh, sinh, cdw)
            for stage in (0, 1):
                if (stage == 0) == hop_first:
                    if self.p.checkerboard:
                        self._hop(X, Xa, sign, right)
                    else:
                        self._dense_hop(X, Xa, sign, right, half=False)
                    if hop_first and self.p.checkerboard:
                        self._scale(X, Xa, -sign)
                else:
                    self._mix(X, Xa, V, right)
                    if not hop_first and self.p.checkerboard:
                        self._scale(X, Xa, -sign)
        if right:
            X, Xa = X.T, Xa.T
        return X, Xa

    def _dense_hop(self, X, Xa, sign, transpose, half):
        """checkerboard = False: the dense e^{sign dtau K} (mu inside K, setupPropK) per band block, from the oracle's eigen-decomposition"""
        N = self.N
        p = self.p
        if p.txhor == 0 and p.txver == 0 and p.tyhor == 0 and p.tyver == 0:
            # no hopping: K_band = -mu_band 1, the propagator is the scalar e^{-+dtau mu_band} (half: half the exponent); no O(N^3)
            # work.  The companion is the same |E| + ||E||_2 in every entry as below: f (x + the column sums of x)
            for b in range(self.MSF):
                f = np.exp(LD(-sign) * LD(0.5 if half else 1.0) * LD(self.dtau) * LD(self.lat.mu_band[b & 1]))
                X[b * N:(b + 1) * N] *= f
                xa = Xa[b * N:(b + 1) * N]
                Xa[b * N:(b + 1) * N] = float(f) * (xa + xa.sum(axis=0, keepdims=True))
            return
        lat = self._dense_half()
        for b in range(self.MSF):
            band = b & 1
            E = (lat._propK_half[band] if sign < 0 else lat._propK_half_inv[band]).astype(CLD)
            if not half:                       # the full step as the square of the half step: no float64 inverse
                E = np.matmul(E, E)
            if transpose:
                E = E.T
            X[b * N:(b + 1) * N] = np.matmul(E, X[b * N:(b + 1) * N])
            # the fp64 propagator is exact only NORM-wise (it comes out of an eigen-decomposition: |dE_ij| <= p(N) u ||E||_2 whatever
            # |E_ij| is), so its companion is |E| + ||E||_2 in every entry
            Ea = abs1(E)
            Xa[b * N:(b + 1) * N] = (Ea + np.linalg.norm(Ea, 2)) @ Xa[b * N:(b + 1) * N]

    def shift_green(self, G):
        """e^{-dtau K/2} G e^{+dtau K/2} with the half-step tables (detsdwopdim.cpp:4507-4612): right sub 1 then sub 0 with the
        + sign, then left sub 1 then sub 0 with the - sign; or the dense half propagators"""
        N = self.N
        X = np.ascontiguousarray(np.array(G, dtype=CLD).T)
        Xa = np.ascontiguousarray(abs1(G).T)
        for side_right in (True, False):
            sign = +1 if side_right else -1
            if self.p.checkerboard:
                for b in range(self.MSF):
                    for sub in (1, 0):
                        self._plaq(X, Xa, b * N, sub, self.lat.plaq_mats[(b & 1, sub, True, sign)], side_right)
            else:
                self._dense_hop(X, Xa, sign, side_right, half=True)
            if side_right:
                X, Xa = np.ascontiguousarray(X.T), np.ascontiguousarray(Xa.T)
        return X, Xa

    # ------------------------------------------------------------------ fermionic accumulators
    # BandSpin (detsdwopdim.h:223-232): XUP = 0, YDOWN = 1, XDOWN = 2, YUP = 3; getBandSpin(band, spin) (:268-273)
    @staticmethod
    def _bs(band, spin):
        return (0 if spin == 0 else 2) if band == 0 else (3 if spin == 0 else 1)

    def _block(self, gs, bs1, bs2):
        """N x N block <c_{bs1} c^dagger_{bs2}> of the full four-flavour Green's function.  O(3): gs holds all of it.  O(1) / O(2):
        gs holds the (XUP, YDOWN) sector; by the model's antiunitary symmetry the (XDOWN, YUP) sector is its complex conjugate and
        the two sectors do not mix (measure(), detsdwopdim.cpp:594-612)."""
        N = self.N
        if self.OPDIM == 3:
            return gs[bs1 * N:(bs1 + 1) * N, bs2 * N:(bs2 + 1) * N]
        if bs1 < 2 and bs2 < 2:
            return gs[bs1 * N:(bs1 + 1) * N, bs2 * N:(bs2 + 1) * N]
        if bs1 >= 2 and bs2 >= 2:
            return np.conj(gs[(bs1 - 2) * N:(bs1 - 1) * N, (bs2 - 2) * N:(bs2 - 1) * N])
        return np.zeros((N, N), dtype=CLD)

    def bins(self, gs):
        """S_band(dx, dy) = sum_{i - j = (dx, dy)} [g_band,up(i, j) + g_band,down(i, j)] over the (2L-1)^2 plain site differences;
        returns (S [2, W, W] complex, indexed [band, dy + L-1, dx + L-1], T [2, W, W, 2]: the sums of |re| and of |im| of the terms)"""
        L, N = self.L, self.N
        W = 2 * L - 1
        gs = np.asarray(gs, dtype=CLD)
        S = np.zeros((2, W, W), dtype=CLD)
        T = np.zeros((2, W, W, 2))
        for band in (0, 1):
            up, dn = self._block(gs, self._bs(band, 0), self._bs(band, 0)), self._block(gs, self._bs(band, 1), self._bs(band, 1))
            tre = np.abs(up.real).astype(float) + np.abs(dn.real).astype(float)
            tim = np.abs(up.imag).astype(float) + np.abs(dn.imag).astype(float)
            g = up + dn
            for i in range(N):
                iy, ix = divmod(i, L)
                # j = (jy, jx): dy + L-1 = iy - jy + L-1 runs from iy + L-1 down to iy
                S[band, iy:iy + L, ix:ix + L] += g[i].reshape(L, L)[::-1, ::-1]
                T[band, iy:iy + L, ix:ix + L, 0] += tre[i].reshape(L, L)[::-1, ::-1]
                T[band, iy:iy + L, ix:ix + L, 1] += tim[i].reshape(L, L)[::-1, ::-1]
        return S, T

    def bins_flat(self, gs):
        """the bins in the accumulator layout: S_X (re, im) per bin, then S_Y; and the matching sums of |terms|"""
        S, T = self.bins(gs)
        W2 = S.shape[1] * S.shape[2]
        val = np.zeros(4 * W2, dtype=LD)
        mag = np.zeros(4 * W2)
        for band in (0, 1):
            val[band * 2 * W2:(band + 1) * 2 * W2:2] = S[band].real.reshape(-1)
            val[band * 2 * W2 + 1:(band + 1) * 2 * W2:2] = S[band].imag.reshape(-1)
            mag[band * 2 * W2:(band + 1) * 2 * W2:2] = T[band, :, :, 0].reshape(-1)
            mag[band * 2 * W2 + 1:(band + 1) * 2 * W2:2] = T[band, :, :, 1].reshape(-1)
        return val, mag

    measure_td_bins = bins_flat

    def measure_accum(self, gs):
        """Every accumulator of one dqmc_measure_slice call from zero, in the layout of dqmc_measure_read_host:
        [greenK0, greenLocal, occDiffSq, count, pairPlus[N], pairMinus[N], S_X[2 W^2], S_Y[2 W^2]]; returns (values [long double],
        sums of the absolute values of the terms [float64]).  gs: a general complex n_g x n_g matrix."""
        N, L = self.N, self.L
        gs = np.asarray(gs, dtype=CLD)
        X, Y, UP, DN = 0, 1, 0, 1
        W2 = (2 * L - 1) ** 2
        val = np.zeros(4 + 2 * N + 4 * W2, dtype=LD)
        mag = np.zeros(4 + 2 * N + 4 * W2)
        # greenK0, greenLocal (:565-588): sum resp. trace over all four flavours; the conjugate sector doubles the real part
        f = 1 if self.OPDIM == 3 else 2
        val[0] = f * np.sum(gs.real)
        mag[0] = f * np.sum(np.abs(gs.real).astype(float))
        val[1] = f * np.sum(np.diag(gs).real) / (4 * LD(N))
        mag[1] = f * np.sum(np.abs(np.diag(gs).real).astype(float)) / (4.0 * N)
        val[3] = 1
        mag[3] = 1

        # occDiffSq (:866-897): per site, with g(b1 s1, b2 s2) = <c c^dagger> at equal sites
        def d(b1, s1, b2, s2):
            return np.diag(self._block(gs, self._bs(b1, s1), self._bs(b2, s2)))
        terms = [
            (-2, d(X, DN, X, UP), d(X, UP, X, DN)), (1, d(X, UP, X, UP), None),
            (2, d(X, DN, Y, DN), d(Y, DN, X, DN)), (2, d(X, UP, Y, DN), d(Y, DN, X, UP)),
            (1, d(Y, DN, Y, DN), None), (-2, d(X, UP, X, UP), d(Y, DN, Y, DN)),
            (2, d(X, DN, Y, UP), d(Y, UP, X, DN)), (2, d(X, UP, Y, UP), d(Y, UP, X, UP)),
            (-2, d(Y, DN, Y, UP), d(Y, UP, Y, DN)),
            (1, d(X, DN, X, DN), None), (2, d(X, DN, X, DN), d(X, UP, X, UP)),
            (-2, d(X, DN, X, DN), d(Y, DN, Y, DN)), (-2, d(X, DN, X, DN), d(Y, UP, Y, UP)),
            (1, d(Y, UP, Y, UP), None), (-2, d(X, UP, X, UP), d(Y, UP, Y, UP)), (2, d(Y, DN, Y, DN), d(Y, UP, Y, UP)),
        ]
        tot, tota = LD(0), 0.0
        for cf, a, b in terms:
            t = a if b is None else a * b
            ta = abs1(a) if b is None else abs1(a) * abs1(b)
            tot += cf * np.sum(t.real)
            tota += abs(cf) * float(np.sum(ta))
        val[2] = tot / LD(N)
        mag[2] = tota / N

        # pairing correlators (:661-722): site pairs (i, 0) and (0, i),
        # -4 sum_{b1 b2} (+-) [g(b1 dn, b2 up) g(b1 up, b2 dn) - g(b1 dn, b2 dn) g(b1 up, b2 up)], minus sign for b1 != b2 in pairMinus
        plus = np.zeros(N, dtype=LD)
        minus = np.zeros(N, dtype=LD)
        pmag = np.zeros(N)
        for pick in (lambda B: B[:, 0], lambda B: B[0, :]):
            def g(b1, s1, b2, s2):
                return pick(self._block(gs, self._bs(b1, s1), self._bs(b2, s2)))
            for b1 in (X, Y):
                for b2 in (X, Y):
                    t1 = g(b1, DN, b2, UP) * g(b1, UP, b2, DN)
                    t2 = g(b1, DN, b2, DN) * g(b1, UP, b2, UP)
                    P = (t1 - t2).real
                    plus += -4 * P
                    minus += -4 * P * (1 if b1 == b2 else -1)
                    pmag += 4 * (abs1(g(b1, DN, b2, UP)) * abs1(g(b1, UP, b2, DN)) + abs1(g(b1, DN, b2, DN)) * abs1(g(b1, UP, b2, UP)))
        val[4:4 + N], val[4 + N:4 + 2 * N] = plus, minus
        mag[4:4 + N] = mag[4 + N:4 + 2 * N] = pmag
        val[4 + 2 * N:], mag[4 + 2 * N:] = self.bins_flat(gs)
        return val, mag

    # ------------------------------------------------------------------ bosonic field kernels
    def phi_sq_sum(self, phi):
        """sum over slices 1..m, sites, components of phi^2 (get_exchange_action_contribution without its 1/2 dtau)"""
        ph = np.asarray(phi[1:], dtype=LD)
        v = np.sum(ph * ph)
        return v, float(v)

    def phi_action(self, phi, r):
        """phiAction (detsdwopdim.cpp:4242-4300) of the whole field for exchange parameter r; (value, sum of |terms|)"""
        p = self.p
        dtau, c, u, r = LD(self.dtau), LD(p.c), LD(p.u), LD(r)
        ph = np.asarray(phi[1:], dtype=LD)                   # [m, N, OPDIM]
        prev = np.roll(ph, 1, axis=0)                        # slice k-1, slice m below slice 1
        xn, yn = self.lat.neigh[0], self.lat.neigh[2]
        phisq = np.sum(ph * ph, axis=2)
        terms = [LD(0.5) * dtau * r * phisq]
        if not p.phi2bosons:
            td = (ph - prev) / dtau
            terms.append(dtau / (2 * c * c) * np.sum(td * td, axis=2))
            xd = ph - ph[:, xn]
            yd = ph - ph[:, yn]
            terms.append(LD(0.5) * dtau * np.sum(xd * xd, axis=2))
            terms.append(LD(0.5) * dtau * np.sum(yd * yd, axis=2))
            terms.append(LD(0.25) * dtau * u * phisq * phisq)
        val = sum(np.sum(t) for t in terms)
        mag = float(sum(np.sum(np.abs(t)) for t in terms))
        return val, mag


# ------------------------------------------------------------------------------------------------------------------------------
# rounding-error bounds (operation counts, not fitted to any output)
# ------------------------------------------------------------------------------------------------------------------------------
def bmult_c(MSF, nslices, cdw=False):
    """c of  |got - ref| <= c u companion + |ref| u  for a chain of nslices slices in fp64.

    A K-term complex product sum computed with (fused or plain) multiply-adds in any order is off by at most 4 (K + 2) u times
    sum |a|_1 |b|_1 (primitives.elementwise_bound; |z|_1 = |re| + |im| is what the companion is made of).  One slice is
      three plaquette passes, K = 4 each:                3 x 4 (4 + 2)    = 72
      the site mix e^{-+dtau V}, K = MSF:                4 (MSF + 2)      = 16 or 24
      the band factor e^{+-dtau mu}, one real multiply:                     1
      the fp64 rounding of the five tables on that path (three 4 x 4 factors, V, the band factor), one u per entry: 5
      cdwU != 0: V's diagonal is cosh x cdwC -+ cdwS, its off-diagonal sinh x cdwC -- one more product, one more sum, one more table: 3
    Errors of successive factors multiply, (1 + a u)(1 + b u) = 1 + (a + b) u + O(u^2); with c u < 1e-12 the second order is
    below 1e-24 relative and is covered by the |ref| u term."""
    return nslices * (72 + 4 * (MSF + 2) + 1 + 5 + (3 if cdw else 0))


def shift_c():
    """the symmetric shift: two half-step plaquette passes per side, 4 x 4 (4 + 2), plus one u for each of the four tables"""
    return 4 * 24 + 4


def dense_c(N, ngemm):
    """checkerboard = False: every hopping factor is a dense N x N product, 4 (N + 2) u each (elementwise_bound).  The fp64
    propagators come out of a Hermitian eigen-decomposition (Jacobi on the device's host side, LAPACK in the oracle): backward
    stable, |dE_ij| <= p(N) u ||E||_2 with p linear in N (Golub & Van Loan, sec. 8.5); the companion of a dense factor therefore
    carries ||E||_2 in every entry (ModelReference._dense_hop) and the same 4 (N + 2) serves as p(N)."""
    return ngemm * 4 * (N + 2)


def check_bound(got, ref, comp, c, what=""):
    """asserts |got - ref| <= c u comp + |ref| u elementwise; returns max err / bound"""
    ref64 = np.asarray(ref).astype(np.complex128 if np.iscomplexobj(ref) else np.float64)
    err = np.abs(np.asarray(got).astype(np.asarray(ref).dtype) - ref).astype(np.float64)
    lim = c * U * np.asarray(comp, dtype=np.float64) + np.abs(ref64) * U
    ratio = float(np.max(err / np.maximum(lim, 1e-300))) if err.size else 0.0
    bad = ~(err <= lim)
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: bound exceeded at %s: |err| = %.3e > %.3e (%d of %d entries, max err/bound %.2f)"
                             % (what, idx, err[idx], lim[idx], int(bad.sum()), bad.size, ratio))
    return ratio
