"""numpy reference of the averaged Green's function block, the pairing bubble and the vertex (tests only).

The block bins an engine matrix gs (n_g x n_g, index = flavour N + site, the stored flavour block R = n_g / N) with the sign sigma:

    Gbar_rc(d) = sum_B sigma(B, d) gs((B (+) d) r; B c),     sigma(B, d) = -1 for each antiperiodic direction in which B + d wraps

rebuild() turns the normalised block back into the dense 4N x 4N matrix gbar(P r; Q c) = sigma(Q, P (-) Q) Gbar_rc(P (-) Q) (for R = 2
with the conjugate sector and the vanishing cross blocks), and the bubble is pair_correlators_full of tests/custom_pair_reference.py on
that matrix -- the full double sum over (A, B), no shortcut.  The tau quadrature, the vertex and the jackknife (tests/series_reference.py)
follow include/dqmc_hip.h.  Everything takes the dtype of its input, so that the same code runs in float64 and in np.longdouble."""
import numpy as np

import custom_pair_reference as cp
import series_reference as sr


FREE_PHI = 1e-150                                           # the field of the "phi = 0" tests (see test_pair_vertex_cpu._free)


def _apb(bc):
    return bc in ("apbc-x", "apbc-xy"), bc in ("apbc-y", "apbc-xy")


def sigma(L, bc):
    """sg[B, d] = +-1, d = dy L + dx"""
    N = L * L
    x, y = np.arange(N) % L, np.arange(N) // L
    apx, apy = _apb(bc)
    sx = np.where(apx & (x[:, None] + x[None, :] >= L), -1.0, 1.0)
    sy = np.where(apy & (y[:, None] + y[None, :] >= L), -1.0, 1.0)
    return sx * sy


def plus(L):
    """site index of B (+) d, [B, d]"""
    N = L * L
    x, y = np.arange(N) % L, np.arange(N) // L
    return ((y[:, None] + y[None, :]) % L) * L + (x[:, None] + x[None, :]) % L


def summand(gs, L, bc):
    """sigma(B, d) gs((B (+) d) r; B c) as [B, d, r, c]"""
    N = L * L
    R = gs.shape[0] // N
    G = np.asarray(gs).reshape(R, N, R, N)                   # [r, P, c, Q]
    B = np.arange(N)[:, None]
    # two index arrays separated by a slice: numpy puts their broadcast axes [B, d] first, the sliced axes r, c behind them
    return sigma(L, bc)[:, :, None, None] * G[:, plus(L), :, B]


def bin_green(gs, L, bc):
    """the raw block row Gbar[d, r, c] = sum over B of summand"""
    return summand(gs, L, bc).sum(axis=0)


def rebuild(gbar, L, bc):
    """dense 4N x 4N matrix from the NORMALISED block gbar[d, r, c] (R = 2 or 4), index = flavour N + site"""
    N = L * L
    g = np.asarray(gbar)
    R = g.shape[-1]
    x, y = np.arange(N) % L, np.arange(N) // L
    d = ((y[:, None] - y[None, :]) % L) * L + (x[:, None] - x[None, :]) % L          # [P, Q] -> P (-) Q
    sg = sigma(L, bc)[np.arange(N)[None, :], d]                                      # sigma(Q, P (-) Q) as [P, Q]
    blk = sg[:, :, None, None] * g[d]                                                # [P, Q, r, c]
    stored = blk.transpose(2, 0, 3, 1).reshape(R * N, R * N)
    if R == 4:
        return stored
    full = np.zeros((4 * N, 4 * N), dtype=stored.dtype)
    full[:2 * N, :2 * N] = stored
    full[2 * N:, 2 * N:] = np.conj(stored)
    return full


def bubble(gbar, ops, L, bc):
    """Pbar_c(d) [count, N] of one normalised block row, by the full double sum of the existing reference"""
    u = cp.link_signs(L, bc)
    return np.array(cp.pair_correlators_full(ops, u, L, rebuild(gbar, L, bc)))


def cos_table(L, Q):
    N = L * L
    x, y = np.arange(N) % L, np.arange(N) // L
    j = (Q[0] * x + Q[1] * y) % L
    return np.cos(2.0 * np.pi * np.arange(L) / L)[j]


def bubbles(gbar_rows, ops, L, bc):
    """Pbar_c(d, tau_k) as [m+1, count, N]: the expensive, Q-independent part of outputs()"""
    return np.array([bubble(row, ops, L, bc) for row in gbar_rows])


def outputs(gbar_rows, P, ops, L, bc, dtau, Q, bub=None):
    """[count, 5 + m] of one set of bin means: gbar_rows [m+1, N, R, R] the normalised block, P [count] = Re chi_c(Q, i omega_0):
    P, Pbar, Gamma, Gamma Pbar, then Pbar_c(Q, tau_k).  bub: bubbles() of the same rows, if the caller has them"""
    m = gbar_rows.shape[0] - 1
    bub = bubbles(gbar_rows, ops, L, bc) if bub is None else bub
    cq = cos_table(L, Q).astype(bub.dtype)
    pq = (bub @ cq).T                                       # [count, m+1]
    w = np.ones(m + 1, dtype=pq.dtype)
    w[0] = w[m] = 0.5
    pbar = dtau * (pq @ w)
    P = np.asarray(P, dtype=pq.dtype)
    return np.concatenate([np.stack([P, pbar, 1.0 / P - 1.0 / pbar, pbar / P - 1.0], axis=1), pq], axis=1)


def jackknife_outputs(gbins, pbins, ops, L, bc, dtau, Q, dtype=np.float64):
    """(value, err) [count, 5 + m] over B bins: gbins [B, m+1, N, R, R] complex, pbins [B, count]; the formulas of series_reference.jackknife
    in `dtype`"""
    cdt = np.complex128 if dtype == np.float64 else np.clongdouble
    g, p = np.asarray(gbins).astype(cdt), np.asarray(pbins).astype(dtype)
    B = g.shape[0]
    if dtype == np.float64:
        n = g[0].size * 2
        packed = np.concatenate([g.view(np.float64).reshape(B, n), p], axis=1)
        f = lambda v: outputs(v[:n].view(np.complex128).reshape(g.shape[1:]), v[n:], ops, L, bc, dtau, Q)
        return sr.jackknife(packed, f)
    return jackknife_outputs_qs(g, {Q: p}, ops, L, bc, dtau, dtype)[Q]


def jackknife_outputs_qs(gbins, pbins_of_q, ops, L, bc, dtau, dtype=np.longdouble):
    """the same for several Q at once, {Q: (value, err)}: the leave-one-out bubbles, which do not depend on Q, are formed once.
    pbins_of_q: {Q: pbins [B, count]}.  Written out in `dtype`, for the long double pass"""
    cdt = np.complex128 if dtype == np.float64 else np.clongdouble
    g = np.asarray(gbins).astype(cdt)
    B = g.shape[0]
    gm = g.sum(axis=0) / B
    loo = [(B * gm - g[b]) / (B - 1) for b in range(B)]
    bub_m, bub = bubbles(gm, ops, L, bc), [bubbles(x, ops, L, bc) for x in loo]
    out = {}
    for Q, pb in pbins_of_q.items():
        p = np.asarray(pb).astype(dtype)
        pm = p.sum(axis=0) / B
        theta = [outputs(loo[b], (B * pm - p[b]) / (B - 1), ops, L, bc, dtau, Q, bub[b]) for b in range(B)]
        tbar = sum(theta) / B
        acc = sum((t - tbar) ** 2 for t in theta)
        out[Q] = (outputs(gm, pm, ops, L, bc, dtau, Q, bub_m), np.sqrt(dtype(B - 1) / B * acc))
    return out


def covariant_gbar(L, m, R, bc, rng):
    """a random normalised block [m+1, N, R, R]: any such block defines a translation-covariant matrix through rebuild()"""
    N = L * L
    return (rng.normal(size=(m + 1, N, R, R)) + 1j * rng.normal(size=(m + 1, N, R, R))) / np.sqrt(N)


# ---- the injected bins of the derived-kernel tests (CPU and GPU share them) -------------------------------------------------------
VERTEX_B, VERTEX_NFREQ, VERTEX_QS = 6, 2, ((0, 0), (1, 2))
# largest relative difference between the float64 and the np.longdouble evaluation of the reference on these bins (values against
# max |value|, errors against max err), as test_reference_precision_on_the_injected_bins measures and asserts it; the GPU bound is 100 x
# this figure with a floor of 1e-12
REFERENCE_PRECISION = 4.3e-14


def gpu_bound():
    return max(100.0 * REFERENCE_PRECISION, 1e-12)


# (opdim, L, m, bc) of the injected-bins tests: the R = 2 row and the R = 4 row of the bubble kernel
VERTEX_CASES = [(2, 4, 20, "apbc-xy"), (3, 4, 20, "apbc-x")]


def vertex_ops():
    from detqmc_amd import pair_operator
    return [cp.P_RAND, cp.P_SYM_BOND, pair_operator("d_bond")]


def vertex_bins(L, m, R, count, seed=11):
    """B = 6 bins: a translation-covariant mean plus 1 % noise.  (gbins [B, m+1, N, R, R] complex, chibins [B, count, nfreq, N] complex with
    a real part around 1 so that P = Re chi(Q, i omega_0) stays away from zero)"""
    rng = np.random.default_rng(seed)
    N = L * L
    g0 = covariant_gbar(L, m, R, None, rng)
    chi0 = 1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=(count, VERTEX_NFREQ, N)) + 0.3j * rng.normal(size=(count, VERTEX_NFREQ, N))
    gb = np.array([g0 + 0.01 * np.abs(g0).max() * (rng.normal(size=g0.shape) + 1j * rng.normal(size=g0.shape)) for _ in range(VERTEX_B)])
    cb = np.array([chi0 + 0.01 * (rng.normal(size=chi0.shape) + 1j * rng.normal(size=chi0.shape)) for _ in range(VERTEX_B)])
    return gb, cb
