"""Synthetic factorisations with prescribed grading for the stabilisation layer (UdV / UDT factorisations, the Green assembly from two
factorisations), their exact values in multiprecision, and plain fp64 restatements of the same operations as yardsticks.  numpy, scipy
and mpmath only: nothing here touches the GPU or the library.

Conventions (dqmc_hip.h: dqmc_decompose_host, dqmc_green_from_factors_host; td_reference.Chain.greens):
    B_R = U_r d_r V_r^H (R-type, B(tau,0)),  B_L = U_l d_l V_l^H (L-type, B(beta,tau)); only U_r and V_l are unitary
    G = (1 + B_R B_L)^-1,  G(tau,0) = G B_R,  G(0,tau) = -B_L G,  G(0) = 1 - B_L G B_R
A missing slot is the identity.  The exact values are those of the fp64 inputs AS GIVEN (U_r only unitary to rounding, and so on): the
inputs go into mpmath bit for bit."""
import functools

import mpmath as mp
import numpy as np
import scipy.linalg as sla

U64 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------
# inputs, deterministic from (n, g, seed)
# ------------------------------------------------------------------------------------------------
def _gauss(rng, n):
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def unitary(rng, n):
    return np.linalg.qr(_gauss(rng, n))[0]


def general(rng, n):
    """a unitary times a unit-diagonal upper triangle with entries of size 1 / sqrt(n): well conditioned, far from unitary"""
    return unitary(rng, n) @ (np.eye(n) + np.triu(_gauss(rng, n), 1) / np.sqrt(2.0 * n))


def scales(rng, n, g):
    """sort(10^uniform(-g, g)), descending"""
    return np.sort(10.0 ** rng.uniform(-g, g, n))[::-1].copy()


def slot_pair(n, g, seed, all_unitary=False):
    """(L, R) = ((general U_l, d_l, unitary V_l), (unitary U_r, d_r, general V_r)); all_unitary: U_l and V_r unitary as well (what an
    SVD factorisation gives, and what the SVD-mode greenFromEye_and_UdV formula takes for granted)"""
    rng = np.random.default_rng([seed, n, int(g), int(all_unitary)])
    other = unitary if all_unitary else general
    L = (other(rng, n), scales(rng, n, g), unitary(rng, n))
    R = (unitary(rng, n), scales(rng, n, g), other(rng, n))
    return L, R


def graded_input(n, g, seed):
    """(W, cs): the column-graded matrix is W diag(cs); its adjoint diag(cs) W^H is the row-graded (L-type) input"""
    rng = np.random.default_rng([seed, n, int(g), 1])
    return general(rng, n), scales(rng, n, g)


def precision_bits(g):
    return int(14 * g + 200)


# ------------------------------------------------------------------------------------------------
# exact values (mpmath)
# ------------------------------------------------------------------------------------------------
def to_mp(a):
    a = np.asarray(a)
    if a.ndim == 1:
        return mp.diag([mp.mpf(float(x)) for x in a])
    return mp.matrix([[mp.mpc(float(x.real), float(x.imag)) for x in row] for row in np.asarray(a, dtype=complex)])


def ld(x):
    """a multiprecision real as a long double (a logarithm of a determinant near 1e4 has an fp64 ulp of 2e-12: more than the bounds)"""
    return np.longdouble(mp.nstr(x, 25))


def log_sum(v):
    """sum of the logarithms of fp64 values, in long double"""
    return np.sum(np.log(np.asarray(v, dtype=np.longdouble)))


def from_mp(m):
    return np.array([[complex(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def _slot_product(slot, n):
    if slot is None:
        return mp.eye(n)
    U, d, V = slot
    return to_mp(U) * to_mp(d) * to_mp(V).H


def exact_green(L, R, n, g, bits=None):
    """dict G, GT0, G0T, G00 (complex128, correctly rounded from the multiprecision value) and logdet = log|det(1 + B_R B_L)| (long double)"""
    with mp.workprec(bits or precision_bits(g)):
        BL, BR = _slot_product(L, n), _slot_product(R, n)
        A = mp.eye(n) + BR * BL
        G = mp.inverse(A)
        out = {"G": from_mp(G), "GT0": from_mp(G * BR), "G0T": from_mp(-(BL * G)), "G00": from_mp(mp.eye(n) - BL * G * BR),
               "logdet": ld(mp.log(abs(mp.det(A))))}
    return out


def exact_green_mp(L, R, n, bits):
    """the same values left in multiprecision (for the precision-doubling check): (G, GT0, G0T, G00, logdet), computed under `bits`"""
    with mp.workprec(bits):
        BL, BR = _slot_product(L, n), _slot_product(R, n)
        A = mp.eye(n) + BR * BL
        G = mp.inverse(A)
        return G, G * BR, -(BL * G), mp.eye(n) - BL * G * BR, mp.log(abs(mp.det(A)))


def exact_singular_values(W, cs, g):
    """singular values of W diag(cs), descending, correctly rounded: mp.svd_c"""
    with mp.workprec(precision_bits(g)):
        S = mp.svd_c(to_mp(W) * to_mp(cs), compute_uv=False)
        return np.array(sorted((float(S[i]) for i in range(len(S))), reverse=True))


def exact_logdet_mp(W, cs, g):
    with mp.workprec(precision_bits(g)):
        A = to_mp(W)
        return ld(mp.log(abs(mp.det(A * to_mp(cs) if cs is not None else A))))


def logdet_longdouble(W, cs=None):
    """log|det(W diag(cs))| by LU with partial pivoting in long double (for the sizes where mp.det takes too long; its own error,
    about n 2^-64, is 2^-11 of the smallest bound it is used with): column scales do not enter the pivot choice, so they are added
    as logarithms"""
    A = np.array(W, dtype=np.clongdouble)
    n = A.shape[0]
    acc = np.longdouble(0)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
        acc += np.log(np.abs(A[k, k]))
        if k + 1 < n:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k, k + 1:])
    return acc + (log_sum(cs) if cs is not None else 0)


@functools.lru_cache(maxsize=None)
def decomposition_case(n, g, seed):
    """one graded factorisation input and what its checks need, computed once per process: W, cs; the fp64 product Ms = W diag(cs)
    ("baked"); log|det| of W diag(cs) and of Ms as given (mp.det at n = 32, long-double LU above); the singular values of W diag(cs)
    from mp.svd_c at n = 32, g <= 40 (else None)"""
    W, cs = graded_input(n, g, seed)
    Ms = W * cs[None, :]
    if n <= 32:
        ld_scaled, ld_baked = exact_logdet_mp(W, cs, g), exact_logdet_mp(Ms, None, g)
    else:
        ld_scaled, ld_baked = logdet_longdouble(W, cs), logdet_longdouble(Ms)
    sv = exact_singular_values(W, cs, g) if n <= 32 and g <= 40 else None
    return {"W": W, "cs": cs, "Ms": Ms, "logdet": ld_scaled, "logdet_baked": ld_baked, "sv": sv}


@functools.lru_cache(maxsize=None)
def _yardstick_of_baked(n, g, seed, mode):
    Ms = decomposition_case(n, g, seed)["Ms"]
    return yardstick_udt(Ms, 0) if mode == "qr" else yardstick_svd(Ms, 0)


def decomposition_yardstick(n, g, seed, mode, kind):
    """the fp64 yardstick factorisation (U, d, V_t) of the baked input Ms (kind 0) or of its adjoint (kind 1): the L-type factorisation
    of Ms^H is the R-type one of Ms with the factors exchanged, so one run (cached: the Jacobi takes seconds) serves both"""
    U, d, Vt = _yardstick_of_baked(n, g, seed, mode)
    return (U, d, Vt) if kind == 0 else (Vt, d, U)


# ------------------------------------------------------------------------------------------------
# metrics of a factorisation  M' = U diag(d) V_t^H,  M' = diag(rs) M diag(cs) with the scales applied in long double
# ------------------------------------------------------------------------------------------------
def scaled_ld(M, cs=None, rs=None):
    A = np.array(M, dtype=np.clongdouble)
    if cs is not None:
        A = A * np.asarray(cs, dtype=np.longdouble)[None, :]
    if rs is not None:
        A = A * np.asarray(rs, dtype=np.longdouble)[:, None]
    return A


def product_ld(U, d, Vt):
    return (np.array(U, dtype=np.clongdouble) * np.asarray(d, dtype=np.longdouble)[None, :]) @ np.array(Vt, dtype=np.clongdouble).conj().T


def graded_residual(P, Mp, kind):
    """max over the columns (kind 0; the rows for kind 1) of |(P - M')[:, j]| / |M'[:, j]|, in long double"""
    axis = 0 if kind == 0 else 1
    num = np.sqrt(np.sum(np.abs(P - Mp) ** 2, axis=axis))
    den = np.sqrt(np.sum(np.abs(Mp) ** 2, axis=axis))
    return float(np.max(num / den))


def unitarity(Q):
    return float(np.max(np.abs(Q.conj().T @ Q - np.eye(Q.shape[0]))))


def udt_structure(T):
    """T = D^-1 R P^T of a pivoted QR: (perm, strictly-lower part of T[:, perm] (must be exactly 0), max | |diag| - 1 |).  perm is read
    off the zero pattern: column perm[j] has its last non-zero in row j"""
    n = T.shape[0]
    last = np.array([np.max(np.nonzero(T[:, c])[0]) if np.any(T[:, c]) else -1 for c in range(n)])
    perm = np.argsort(last, kind="stable")
    Tp = T[:, perm]
    return perm, float(np.max(np.abs(np.tril(Tp, -1)))), float(np.max(np.abs(np.abs(np.diag(Tp)) - 1.0)))


def decomposition_metrics(U, d, Vt, Mp, kind, mode, logdet_exact, product=None):
    """mode 'qr' or 'svd'.  Mp: the exact scaled input in long double; product: what U d V_t^H must equal if not Mp (chained steps).
    unit: the factor that must be unitary (both in SVD mode); res: graded residual; logdet: |sum log d + log|det T| - exact| / n"""
    n = len(d)
    Q, T = (U, Vt) if kind == 0 else (Vt, U)
    out = {"unit": max(unitarity(U), unitarity(Vt)) if mode == "svd" and product is None else unitarity(Q),
           "res": graded_residual(product_ld(U, d, Vt), Mp if product is None else product, kind)}
    if logdet_exact is not None:
        out["logdet"] = float(abs(log_sum(d) + np.longdouble(np.linalg.slogdet(T)[1]) - logdet_exact)) / n
    return out


# ------------------------------------------------------------------------------------------------
# yardsticks: fp64 restatements, the plain CPU versions
# ------------------------------------------------------------------------------------------------
def yardstick_udt(Ms, kind):
    """norm-ranked pivot-free UDT of the fp64 matrix Ms: the columns (rows for kind 1) sorted by norm, Householder QR without further
    pivoting, d = |diag R|, T = D^-1 R P^T.  Returns (U, d, V_t) in the library's convention"""
    A = Ms if kind == 0 else Ms.conj().T
    perm = np.argsort(-np.sqrt(np.sum(np.abs(A) ** 2, axis=0)), kind="stable")
    Q, R = sla.qr(A[:, perm], mode="economic")
    d = np.abs(np.diag(R))
    T = np.zeros_like(R)
    T[:, perm] = R / d[:, None]
    Tt = T.conj().T
    return (Q, d, Tt) if kind == 0 else (Tt, d, Q)


def jacobi_svd(A, max_sweeps=60):
    """cyclic one-sided Jacobi (Hestenes) with de Rijk's ordering: before column i is rotated against the columns behind it, the
    largest of those is swapped into place i.  Returns (U, d, V), A = U diag(d) V^H, d descending"""
    A = np.array(A, dtype=np.complex128)
    n = A.shape[1]
    V = np.eye(n, dtype=np.complex128)
    tol = np.sqrt(n) * 2.0 * U64
    for _ in range(max_sweeps):
        rotated = False
        for i in range(n - 1):
            k = i + int(np.argmax(np.sum(np.abs(A[:, i:]) ** 2, axis=0)))
            if k != i:
                A[:, [i, k]] = A[:, [k, i]]
                V[:, [i, k]] = V[:, [k, i]]
            for j in range(i + 1, n):
                ap, aq = A[:, i], A[:, j]
                gam = np.vdot(ap, aq)
                ag = abs(gam)
                al, be = np.vdot(ap, ap).real, np.vdot(aq, aq).real
                if ag <= tol * np.sqrt(al) * np.sqrt(be):
                    continue
                rotated = True
                zeta = (be - al) / (2.0 * ag)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t * (gam / ag)                     # the phase makes the rotated inner product real
                for X in (A, V):
                    xp = X[:, i].copy()
                    X[:, i] = c * xp - np.conj(s) * X[:, j]
                    X[:, j] = s * xp + c * X[:, j]
        if not rotated:
            break
    d = np.sqrt(np.sum(np.abs(A) ** 2, axis=0))
    order = np.argsort(-d, kind="stable")
    return A[:, order] / d[order][None, :], d[order], V[:, order]


def yardstick_svd(Ms, kind):
    """Jacobi SVD with the grading on the columns (the adjoint is factorised for kind 1).  Returns (U, d, V_t)"""
    if kind == 0:
        return jacobi_svd(Ms)
    V, d, U = jacobi_svd(Ms.conj().T)
    return U, d, V


def split_scales(d):
    d = np.asarray(d, dtype=float)
    return 1.0 / np.maximum(d, 1.0), np.minimum(d, 1.0)


def _eye_slot(n):
    return np.eye(n, dtype=complex), np.ones(n), np.eye(n, dtype=complex)


def yardstick_green(L, R, n):
    """the scale-split assembly with np.linalg.inv:  Z = Drmax^-1 (U_r^H V_l) Dlmax^-1 + Drmin (V_r^H U_l) Dlmin"""
    Ul, dl, Vl = L if L is not None else _eye_slot(n)
    Ur, dr, Vr = R if R is not None else _eye_slot(n)
    rmi, rmin = split_scales(dr)
    lmi, lmin = split_scales(dl)
    Z = rmi[:, None] * (Ur.conj().T @ Vl) * lmi[None, :] + rmin[:, None] * (Vr.conj().T @ Ul) * lmin[None, :]
    Zi = np.linalg.inv(Z)
    Amax, Amin = Vl * lmi[None, :], Ul * lmin[None, :]
    Bmax, Bmin = rmi[:, None] * Ur.conj().T, rmin[:, None] * Vr.conj().T
    return {"G": Amax @ Zi @ Bmax, "GT0": Amax @ Zi @ Bmin, "G0T": -(Amin @ Zi @ Bmax), "G00": np.eye(n) - Amin @ Zi @ Bmin,
            "logdet": np.longdouble(np.linalg.slogdet(Z)[1]) - log_sum(rmi) - log_sum(lmi)}


def yardstick_green_svd(L, R, n):
    """the reference's own formula (greenFromUdV, SVD mode) with LAPACK: G = V_l V diag(1/sv) (U_r U)^H from the SVD U sv V^H of
    U_r^H V_l + d_r (V_r^H U_l) d_l.  Only G and logdet = sum log sv"""
    Ul, dl, Vl = L if L is not None else _eye_slot(n)
    Ur, dr, Vr = R if R is not None else _eye_slot(n)
    X = Ur.conj().T @ Vl + dr[:, None] * (Vr.conj().T @ Ul) * dl[None, :]
    U, sv, Vh = np.linalg.svd(X)
    return {"G": (Vl @ Vh.conj().T / sv[None, :]) @ (Ur @ U).conj().T, "logdet": log_sum(sv)}


# ------------------------------------------------------------------------------------------------
# errors of a set of Green's functions against the exact ones
# ------------------------------------------------------------------------------------------------
def green_errors(got, exact, n, relerr, relerr_blocks):
    """every metric of the outputs present in `got`: relerr and relerr_blocks(bs = 8) per matrix, |logdet - exact| / n"""
    out = {}
    for k in ("G", "GT0", "G0T", "G00"):
        if k in got:
            out[k] = relerr(got[k], exact[k])
            out[k + "_blk"] = relerr_blocks(got[k], exact[k], bs=8)
    if "logdet" in got:
        out["logdet"] = float(abs(np.longdouble(got["logdet"]) - exact["logdet"])) / n
    return out


# the cases of tests/test_gpu_stabilisation.py (tests/test_stab_reference_cpu.py checks the admission condition on every one of them)
SEED = 7
DECOMP_SIZES = (32, 72, 128, 200)
DECOMP_GRADINGS = {"qr": (0, 8, 40, 120), "svd": (0, 8, 40)}
CHAINED_CASES = ((32, 8), (32, 40), (72, 40))
GREEN_N = 32
GREEN_GRADINGS = {"qr": (0, 8, 40, 120), "svd": (0, 2)}
GREEN_SLOTS = ("both", "R", "L")
# The QR routes of the assembly (reflectors, explicit Q) lose G(tau,0) to about cond(Z) u where Z is ill conditioned; the LU route
# and the yardstick do not.  That is a property of the route, not of its kernels: its plain numpy restatement
# (green_qr_route_restated) shows the same loss.  A case is used on the QR routes only if that restatement stays within FACTOR x
# the yardstick in every metric; at n = 32, seed 7 this excludes g = 120 with both slots (cond Z = 2e5, restatement 1e5 x the
# yardstick), which the LU route keeps.  tests/test_stab_reference_cpu.py asserts both halves of this.
GREEN_QR_ROUTES_EXCLUDED = ((120, "both"),)


def green_gradings(route, slots):
    """the gradings of test_green_from_factors for a route ('lu', 'reflectors', 'explicit_q', 'svd') and a slot choice"""
    if route == "svd":
        return GREEN_GRADINGS["svd"]
    return tuple(g for g in GREEN_GRADINGS["qr"] if route == "lu" or (g, slots) not in GREEN_QR_ROUTES_EXCLUDED)

def tie_matrices(n):
    """equal column norms: the identity, a permutation times a diagonal, and a general matrix with two columns of exactly equal norm in
    any summation order (small integers, the second a signed permutation of the first)"""
    rng = np.random.default_rng([SEED, n, 99])
    p = rng.permutation(n)
    pd = np.zeros((n, n), dtype=complex)
    pd[p, np.arange(n)] = 10.0 ** rng.uniform(-8, 8, n) * np.exp(2j * np.pi * rng.uniform(size=n))
    tie = general(rng, n)
    v = rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)
    tie[:, 5] = v
    tie[:, 17] = (v * rng.choice([1, -1, 1j, -1j], n))[rng.permutation(n)]
    return {"identity": np.eye(n, dtype=complex), "perm_diag": pd, "equal_norms": tie}


def batch_operands(n, g, nchains):
    """(M, colscale, rowscale) per chain: chain 0 column-graded, chain 1 row-graded, chain 2 ungraded, and so on with seeds of their own"""
    Ms, cs, rs = [], [], []
    one = np.ones(n)
    for b in range(nchains):
        W, s = graded_input(n, g, SEED + 10 * b)
        how = b % 3
        Ms.append(W if how != 1 else W.conj().T.copy())
        cs.append(s if how == 0 else one)
        rs.append(s if how == 1 else one)
    return np.array(Ms), np.array(cs), np.array(rs)


def batch_yardstick(M, cs, rs, b, mode):
    """chain b's yardstick (the call is R-type for every chain) and the axis its residual is graded along: SVD mode follows the grading
    (the device picks the orientation per chain), QR mode ranks the columns whatever the rows look like"""
    Ms = rs[b][:, None] * M[b] * cs[b][None, :]
    axis = 1 if (mode == "svd" and b % 3 == 1) else 0
    if mode == "svd":
        return yardstick_svd(Ms, axis), axis
    return yardstick_udt(Ms, 0), axis


def chained_operands(n, g, seed):
    """[(name, M, colscale, rowscale, kind, Aold)] of a chained step: W diag(cs) with the graded columns in shuffled order (the ranking
    permutation is then neither the identity nor an involution), as colscale with the R-type step and, the adjoint, as rowscale with
    the L-type step; Aold general"""
    W, cs = graded_input(n, g, seed)
    rng = np.random.default_rng([seed, n, int(g), 5])
    Aold = general(rng, n)
    q = rng.permutation(n)
    W, cs = np.ascontiguousarray(W[:, q]), cs[q].copy()
    return [("colscale", W, cs, None, 0, Aold), ("rowscale_L", W.conj().T.copy(), None, cs, 1, Aold)]


def chained_yardstick(M, cs, rs, kind, Aold, mode):
    """the yardstick factorisation of the scaled operand with its non-unitary factor multiplied by Aold in fp64"""
    Ms = M * (cs[None, :] if cs is not None else 1.0) * (rs[:, None] if rs is not None else 1.0)
    U, d, Vt = (yardstick_udt if mode == "qr" else yardstick_svd)(Ms, kind)
    return (U, d, Aold @ Vt) if kind == 0 else (Aold @ U, d, Vt)


ADMISSION = 1e-9        # a case is used only if the yardstick's own error against the exact value is at most this, in every metric
FACTOR = 100.0          # the device may be this much worse than the yardstick ...


def bound(yard_err, n):
    """... and never has to be better than n u"""
    return max(FACTOR * yard_err, n * U64)


@functools.lru_cache(maxsize=None)
def green_case(n, g, seed, slots, all_unitary=False):
    """(L, R, exact) of one Green case; slots: 'both', 'R' or 'L'.  Cached: the exact value is computed once per process"""
    L, R = slot_pair(n, g, seed, all_unitary)
    if slots == "R":
        L = None
    if slots == "L":
        R = None
    return L, R, exact_green(L, R, n, g)


# ------------------------------------------------------------------------------------------------
# the committed exact values of the larger case (oracle/make_stab_golden.py writes them, tests/golden/stab_n72_g40.npz)
# ------------------------------------------------------------------------------------------------
# Two files, each under the size limit for a committed file (they hold the six inputs as well: LAPACK and libm do not give the same
# bits on every machine, and the exact values belong to the inputs bit for bit): about 770 KB and 720 KB.
# stab_n72_g40.npz: (72, 40) for the LU and the reflector route, and (32, 40), which the CPU suite regenerates.
# stab_n72_g8.npz:  (72, 8) for all three QR-mode routes -- g shrunk for the explicit-Q route, as follows.
# n_g = 72, g = 40 (cond Z = 5e3) on the explicit-Q route: Q from Cholesky-QR2 panels is orthogonal to 4e-14 only, which R^-1 Q^H
# amplifies by cond(R).  An MI355X gives G and G(0,tau) to 8.0e-12 and 9.3e-12 there, 133 and 119 x the yardstick, and the route's
# numpy restatement (green_qr_route_restated, explicit_q) the same figures, about 100 x the yardstick: the loss is the route's, so
# that route gets the next smaller grading of the list, g = 8, where its restatement is within a few x (the CPU suite asserts
# admission for it).  SVD mode is out of the question at either grading (GREEN_GRADINGS: g <= 2): its time-displaced functions come
# from the scale-split Z, but only after G, whose Jacobi SVD does not converge at g = 40 (DQMC_ENOCONV).
GOLDEN_FILES = {"stab_n72_g40.npz": ((72, 40), (32, 40)), "stab_n72_g8.npz": ((72, 8),)}
GOLDEN_GPU_CASES = tuple((72, 40, r) for r in ("lu", "reflectors")) + tuple((72, 8, r) for r in ("lu", "reflectors", "explicit_q"))


def golden_file(n, g):
    return next(name for name, cases in GOLDEN_FILES.items() if (n, g) in cases)


INPUT_KEYS = ("Ul", "dl", "Vl", "Ur", "dr", "Vr")


def inputs_checksum(L, R):
    """sha256 over the bytes of the six input arrays"""
    import hashlib
    h = hashlib.sha256()
    for a in tuple(L) + tuple(R):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_payload(n, g, seed=SEED, inputs=None):
    """the arrays of one case as the fixture holds them, keys prefixed n{n}_: the six inputs (LAPACK and libm do not give the same bits
    on every machine, and the exact values belong to the inputs bit for bit), their checksum, the four matrices and the
    log-determinant.  inputs: (L, R) to use instead of the generated pair"""
    L, R = inputs or slot_pair(n, g, seed)
    ex = exact_green(L, R, n, g)
    out = {"n%d_%s" % (n, k): ex[k] for k in ("G", "GT0", "G0T", "G00")}
    out.update({"n%d_%s" % (n, k): a for k, a in zip(INPUT_KEYS, tuple(L) + tuple(R))})
    out["n%d_logdet" % n] = np.array(mp.nstr(mp.mpf(str(ex["logdet"])), 25))        # long double as text: npz files are portable
    out["n%d_inputs_sha256" % n] = np.array(inputs_checksum(L, R))
    return out


def golden_case(z, n, g, seed=SEED):
    """(L, R, exact) of a case held by the loaded fixture z.  The stored inputs must carry the recorded checksum and be what the
    generator makes on this machine up to rounding (1e-12)"""
    a = [z["n%d_%s" % (n, k)] for k in INPUT_KEYS]
    L, R = tuple(a[:3]), tuple(a[3:])
    assert inputs_checksum(L, R) == str(z["n%d_inputs_sha256" % n]), "the stored inputs do not carry the recorded checksum"
    for x, y in zip(L + R, sum(slot_pair(n, g, seed), ())):
        assert np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300 if x.ndim == 1 else np.max(np.abs(y)))) < 1e-12, "the generator no longer makes the stored inputs"
    ex = {k: z["n%d_%s" % (n, k)] for k in ("G", "GT0", "G0T", "G00")}
    ex["logdet"] = np.longdouble(str(z["n%d_logdet" % n]))
    return L, R, ex


def _bgs_cholqr2(A, nb=64):
    """block Gram-Schmidt (two passes against the columns before) with Cholesky-QR2 on each panel of nb columns: A = Q R"""
    n = A.shape[0]
    Q, Rm = np.zeros_like(A), np.zeros_like(A)
    for j0 in range(0, n, nb):
        b = min(nb, n - j0)
        Aj = A[:, j0:j0 + b].copy()
        if j0:
            W1 = Q[:, :j0].conj().T @ Aj
            Aj -= Q[:, :j0] @ W1
            W2 = Q[:, :j0].conj().T @ Aj
            Aj -= Q[:, :j0] @ W2
            Rm[:j0, j0:j0 + b] = W1 + W2
        R1 = np.linalg.cholesky(Aj.conj().T @ Aj).conj().T
        Aj = sla.solve_triangular(R1.T, Aj.T, lower=True).T
        R2 = np.linalg.cholesky(Aj.conj().T @ Aj).conj().T
        Q[:, j0:j0 + b] = sla.solve_triangular(R2.T, Aj.T, lower=True).T
        Rm[j0:j0 + b, j0:j0 + b] = R2 @ R1
    return Q, Rm


def green_qr_route_restated(L, R, n, explicit_q=False):
    """the QR routes of the device's assembly restated in numpy: Z P = Q R with the columns ranked by norm and no further pivoting
    (Householder; explicit_q: block Gram-Schmidt with Cholesky-QR2 panels of 64 columns, Q applied as a matrix), every left bracket
    times P R^-1, every right bracket behind Q^H.  Not a yardstick: it shows what the ROUTE (not its kernels) loses where Z is ill
    conditioned, cf. green_gradings"""
    Ul, dl, Vl = L if L is not None else _eye_slot(n)
    Ur, dr, Vr = R if R is not None else _eye_slot(n)
    rmi, rmin = split_scales(dr)
    lmi, lmin = split_scales(dl)
    Z = rmi[:, None] * (Ur.conj().T @ Vl) * lmi[None, :] + rmin[:, None] * (Vr.conj().T @ Ul) * lmin[None, :]
    perm = np.argsort(-np.sqrt(np.sum(np.abs(Z) ** 2, axis=0)), kind="stable")
    Q, Rr = _bgs_cholqr2(Z[:, perm]) if explicit_q else sla.qr(Z[:, perm])

    def left(X, sc):
        return sla.solve_triangular(Rr.T, ((X * sc[None, :])[:, perm]).T, lower=True).T

    def right(Yh, sc):
        return Q.conj().T @ (sc[:, None] * Yh.conj().T)
    Amax, Amin, Bmax, Bmin = left(Vl, lmi), left(Ul, lmin), right(Ur, rmi), right(Vr, rmin)
    return {"G": Amax @ Bmax, "GT0": Amax @ Bmin, "G0T": -(Amin @ Bmax), "G00": np.eye(n) - Amin @ Bmin,
            "logdet": log_sum(np.abs(np.diag(Rr))) - log_sum(rmi) - log_sum(lmi), "condZ": float(np.linalg.cond(Z))}
