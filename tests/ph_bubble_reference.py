"""numpy reference of the particle-hole bubble and vertex of the user-defined bilinears (tests only).

From the normalised block of the averaged Green's function (tests/pair_vertex_reference.py: sigma, rebuild) the dense matrices

    gbar(tau_k, 0) = rebuild(row k),        gbar(0, tau_k) = -rebuild(row m - k)        (the cyclic invariance of the weight)

are formed, and the bubble is bond_correlators_full of tests/custom_bond_reference.py on them -- the full double sum over (A, B), no
shortcut -- with the one-body product it contains subtracted again.  The tau quadrature, the disconnected part D, the vertex and the
jackknife follow include/dqmc_hip.h.  Everything takes the dtype of its input, so that the same code runs in float64 and in
np.longdouble (bin_periodic returns float64: the per-d values are rounded once, everything behind them is not)."""
import numpy as np

import custom_bond_reference as cb
import pair_vertex_reference as pv
from custom_reference import M_SX_BANDX
from td_ph_reference import bin_periodic

FREE_PHI = pv.FREE_PHI
B_SX_BANDX = (M_SX_BANDX, None, None)                       # on-site, couples the stored sector of OPDIM < 3 to its conjugate


def links(L, bc):
    return cb.link_table(L, bc, False)


def one_body(g0, ops, L, bc):
    """obar_c [count] complex at site 0 from the normalised row 0, and the dense operators"""
    g = pv.rebuild(g0, L, bc)
    u = links(L, bc)
    return np.array([cb.one_body_all(g, cb.dense_operators(op, u, L))[0] for op in ops])


def bubble(gk, gmk, g0, ops, L, bc):
    """chibar_c(d) [count, N] of one tau: gk, gmk, g0 = rows k, m - k and 0 of the normalised block"""
    gt0, g0t, g00 = pv.rebuild(gk, L, bc), -pv.rebuild(gmk, L, bc), pv.rebuild(g0, L, bc)
    u = links(L, bc)
    full = cb.bond_correlators_full(ops, u, L, g00, gt0, g0t, g00)
    out = []
    for c, op in enumerate(ops):
        o = cb.one_body_all(g00, cb.dense_operators(op, u, L))
        out.append(full[c] - bin_periodic(np.outer(o, o), L))
    return np.array(out)


def bubbles(gbar_rows, ops, L, bc):
    """chibar_c(d, tau_k) as [m+1, count, N]: the expensive, Q-independent part of outputs()"""
    m = gbar_rows.shape[0] - 1
    return np.array([bubble(gbar_rows[k], gbar_rows[m - k], gbar_rows[0], ops, L, bc) for k in range(m + 1)])


def disconnected(obar, L, m, dtau, Q):
    """D_c = beta Re(obar_c^2) sum_d cos(Q d): beta N Re obar_c^2 at Q = 0, else 0"""
    o2 = (obar * obar).real
    return dtau * m * o2 * (L * L) if tuple(Q) == (0, 0) else 0 * o2


def outputs(gbar_rows, chi_raw, ops, L, bc, dtau, Q, bub=None, obar=None):
    """[count, 6 + m] of one set of bin means: gbar_rows [m+1, N, R, R] the normalised block, chi_raw [count] = Re chi_c(Q, i omega_0) of
    part 9: chi = chi_raw - D, chibar, Gamma, Gamma chibar, D, then chibar_c(Q, tau_k).  bub, obar: bubbles() and one_body() of the same
    rows, if the caller has them"""
    m = gbar_rows.shape[0] - 1
    bub = bubbles(gbar_rows, ops, L, bc) if bub is None else bub
    obar = one_body(gbar_rows[0], ops, L, bc) if obar is None else obar
    cq = pv.cos_table(L, Q).astype(gbar_rows.real.dtype)
    pq = (bub.astype(cq.dtype) @ cq).T                      # [count, m+1]
    w = np.ones(m + 1, dtype=pq.dtype)
    w[0] = w[m] = 0.5
    chibar = dtau * (pq @ w)
    D = disconnected(obar, L, m, dtau, Q)
    chi = np.asarray(chi_raw, dtype=pq.dtype) - D
    return np.concatenate([np.stack([chi, chibar, 1.0 / chi - 1.0 / chibar, chibar / chi - 1.0, D + 0 * chi], axis=1), pq], axis=1)


def jackknife_outputs_qs(gbins, chibins_of_q, ops, L, bc, dtau, dtype=np.float64):
    """{Q: (value, err)}, [count, 6 + m] each, over B bins: gbins [B, m+1, N, R, R] complex, chibins_of_q {Q: [B, count]}; the formulas of
    series_reference.jackknife written out in `dtype`; the leave-one-out bubbles, which do not depend on Q, are formed once"""
    cdt = np.complex128 if dtype == np.float64 else np.clongdouble
    g = np.asarray(gbins).astype(cdt)
    B = g.shape[0]
    gm = g.sum(axis=0) / B
    loo = [(B * gm - g[b]) / (B - 1) for b in range(B)]
    bub_m, bub = bubbles(gm, ops, L, bc), [bubbles(x, ops, L, bc) for x in loo]
    ob_m, ob = one_body(gm[0], ops, L, bc), [one_body(x[0], ops, L, bc) for x in loo]
    out = {}
    for Q, pb in chibins_of_q.items():
        p = np.asarray(pb).astype(dtype)
        pm = p.sum(axis=0) / B
        theta = [outputs(loo[b], (B * pm - p[b]) / (B - 1), ops, L, bc, dtau, Q, bub[b], ob[b]) for b in range(B)]
        tbar = sum(theta) / B
        acc = sum((t - tbar) ** 2 for t in theta)
        out[Q] = (outputs(gm, pm, ops, L, bc, dtau, Q, bub_m, ob_m), np.sqrt(dtype(B - 1) / B * acc))
    return out


def twin_jackknife(gbins, chibins, ops, L, bc, dtau, Q):
    """(value, err) [count, 6 + m] from the package's own numpy functions: detqmc_amd.ph_bubble, ph_one_body and jackknife on the packed
    bins (gbins [B, m+1, N, R, R] complex, chibins [B, count] = Re chi_c(Q, i omega_0)) -- what the GPU tests compare the device with"""
    from detqmc_amd import jackknife, ph_bubble, ph_one_body
    g, p = np.asarray(gbins, dtype=np.complex128), np.asarray(chibins, dtype=np.float64)
    B, m = g.shape[0], g.shape[1] - 1
    n = g[0].size * 2
    packed = np.concatenate([np.ascontiguousarray(g).view(np.float64).reshape(B, n), p], axis=1)
    cq = pv.cos_table(L, Q)
    w = np.ones(m + 1)
    w[0] = w[m] = 0.5

    def f(v):
        rows = v[:n].view(np.complex128).reshape(g.shape[1:])
        pq = (ph_bubble(rows, ops, L, bc) @ cq).T           # [count, m+1]
        chibar = dtau * (pq @ w)
        D = disconnected(ph_one_body(rows[0], ops, L, bc), L, m, dtau, Q)
        chi = v[n:] - D
        with np.errstate(divide="ignore", invalid="ignore"):
            gam, gb = 1.0 / chi - 1.0 / chibar, chibar / chi - 1.0
        return np.concatenate([np.stack([chi, chibar, gam, gb, D + 0 * chi], axis=1), pq], axis=1)

    return jackknife(packed, f)


# ---- the injected bins of the derived-kernel tests (CPU and GPU share them) -------------------------------------------------------
VERTEX_B, VERTEX_NFREQ, VERTEX_M, VERTEX_DTAU = 5, 2, 6, 0.1
VERTEX_QS = ((0, 0), (2, 2), (1, 2))
# (opdim, L, m, bc) of the injected-bins tests: the R = 2 and the R = 4 row of the bubble kernel, periodic and antiperiodic
VERTEX_CASES = [(2, 4, VERTEX_M, "pbc"), (2, 4, VERTEX_M, "apbc-xy"), (3, 4, VERTEX_M, "pbc"), (3, 4, VERTEX_M, "apbc-xy")]
# largest relative difference between the float64 and the np.longdouble evaluation of the reference on these bins (values against
# max |value|, errors against max err), as test_reference_precision_on_the_injected_bins measures and asserts it; the GPU bound of the
# derived kernels is 100 x this figure.  Measured: values 2.3e-16 .. 3.0e-15, errors 2.0e-14 .. 7.59e-13 (the jackknife errors of 0.1 %
# noise are differences of nearly equal numbers); the largest, rounded up
REFERENCE_PRECISION = 7.6e-13


def gpu_bound():
    return 100.0 * REFERENCE_PRECISION


def vertex_ops():
    return [cb.B_RAND, cb.B_DDW, cb.B_ONSITE, B_SX_BANDX]


def vertex_bins(L, m, R, bc, seed=20):
    """B = 5 bins: a translation-covariant mean plus 0.1 % noise (the seed: of 1 .. 40 the one whose mean block keeps every
    |chibar_c(Q)| largest against dtau sum_k w_k |chibar_c(Q, tau_k)|, 7 % -- 1 / chibar is as well conditioned as random blocks
    allow).  (gbins [B, m+1, N, R, R] complex, chibins [B, count, nfreq, N] complex;
    the real part at frequency 0 is 3 + D_c(Q) of the mean block plus noise, so that chi = Re chi - D stays away from zero as it does in
    a measured series, where part 9 carries the disconnected part)"""
    ops = vertex_ops()
    rng = np.random.default_rng(seed)
    N = L * L
    g0 = pv.covariant_gbar(L, m, R, None, rng)
    chi0 = 3.0 + 0.3 * rng.uniform(-1.0, 1.0, size=(len(ops), VERTEX_NFREQ, N)) + 0.3j * rng.normal(size=(len(ops), VERTEX_NFREQ, N))
    chi0[:, 0, 0] += disconnected(one_body(g0[0], ops, L, bc), L, m, VERTEX_DTAU, (0, 0))
    gb = np.array([g0 + 0.001 * np.abs(g0).max() * (rng.normal(size=g0.shape) + 1j * rng.normal(size=g0.shape)) for _ in range(VERTEX_B)])
    chb = np.array([chi0 + 0.01 * (rng.normal(size=chi0.shape) + 1j * rng.normal(size=chi0.shape)) for _ in range(VERTEX_B)])
    return gb, chb
