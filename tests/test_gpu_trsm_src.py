"""The right-hand triangular solve that reads its right-hand side where it lies (run_trsm_right_upper with a ColSrc): k_trsm_block and
the accumulate input of the spine products of trsm_rec take X[:, idx[j]] scale[idx[j]] at the first touch of every column block of the
destination, instead of a scaled / gathered copy made by k_gather_scale_cols or k_permute_scale_cols beforehand.  The value read is
formed with the copy kernels' single multiply per component, so the solve must return their bits; the destination's old content (NaN
sentinels) must not enter, the source must not change (Arena.check).  Then greenFromUdV end to end: the LU route, which now runs on
the first-touch source, against the QR route, which still copies."""
import ctypes

import numpy as np
import pytest

import primitives as P
from primitives import Arena

pytestmark = pytest.mark.gpu

GATHER, PERMUTE, SOURCE = 0, 1, 2


def _call(ar, n, trans, unit, idx, how):
    fn = P.lib().dqmc_prim_trsm_src
    vp, sz, i, ll, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p
    fn.argtypes = [vp, sz, i, sz, i, ll, ll, i, i, ll, ll, ll, i, cp, i]
    rc, msg = ar.call("dqmc_prim_trsm_src", n, ar.off("R"), ar.off("C"), trans, unit, ar.off("X"), ar.off(idx), ar.off("scale"), how)
    assert rc >= 0, msg
    ar.check()


def _solve(n, nb, trans, unit, Rs, Xs, scales, idxs, how):
    """idxs: per chain an index vector, or None (no index: columns in place).  C starts as NaN sentinels."""
    ar = Arena(nb)
    ar.mat("R", n, n)
    ar.mat("C", n, n, kind="out")
    ar.mat("X", n, n)
    ar.vec("scale", n, np.float64)
    if idxs is not None:
        ar.vec("idx", n, np.int32)
    ar.layout()
    for b in range(nb):
        S = Rs[b].conj().T.copy() if trans else Rs[b].copy()
        mask = np.tril(np.ones((n, n), bool), -1) if not trans else np.triu(np.ones((n, n), bool), 1)
        S[mask] = np.nan                                     # what the solve must not read
        if unit:
            np.fill_diagonal(S, np.nan)
        ar.set("R", S, b)
        ar.set("X", Xs[b], b)
        ar.set("scale", scales[b], b)
        if idxs is not None:
            ar.set("idx", idxs[b], b)
    _call(ar, n, trans, unit, "idx" if idxs is not None else None, how)
    return [ar.get("C", b) for b in range(nb)]


def _operands(n, nb, unit, seed):
    rng = np.random.default_rng(seed)
    Rs, Xs, scales = [], [], []
    for _ in range(nb):
        R = np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        np.fill_diagonal(R, 1.0 if unit else (2 + rng.random(n)) * np.exp(1j * rng.uniform(0, 6, n)))
        Rs.append(R)
        Xs.append(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        scales.append(10.0 ** rng.uniform(-8, 0, n))          # random mantissas: a multiply fused into the following add shows
    return rng, Rs, Xs, scales


def _same(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w).all(), what
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}, chain {b}: {len(bad)} elements differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


# n = 32: one diagonal block, no product; 72: ragged, the generic GEMM kernel; 128, 256: whole 32 x 32 tiles, two and three spine products
@pytest.mark.parametrize("n", [32, 72, 128, 256])
@pytest.mark.parametrize("trans,unit", [(0, 0), (1, 1)], ids=["upper", "lowerH-unit"])
@pytest.mark.parametrize("perm", ["identity", "random"])
def test_first_touch_source_gives_the_bits_of_copy_then_solve(n, trans, unit, perm):
    nb = 3
    rng, Rs, Xs, scales = _operands(n, nb, unit, 1000 * n + 10 * trans + (perm == "random"))
    ps = [np.arange(n, dtype=np.int32) if perm == "identity" else rng.permutation(n).astype(np.int32) for _ in range(nb)]
    # gather form: S[:, j] = X[:, p[j]] scale[p[j]]
    want = _solve(n, nb, trans, unit, Rs, Xs, scales, ps, GATHER)
    _same(_solve(n, nb, trans, unit, Rs, Xs, scales, ps, SOURCE), want, f"gather n={n}")
    # scatter form: S[:, p[j]] = X[:, j] scale[j], read as a gather through the inverse permutation
    want = _solve(n, nb, trans, unit, Rs, Xs, scales, ps, PERMUTE)
    inv = [np.argsort(p).astype(np.int32) for p in ps]
    _same(_solve(n, nb, trans, unit, Rs, Xs, scales, inv, SOURCE), want, f"scatter n={n}")
    if perm == "identity":                                    # no index vector at all: what the LU route's left half passes
        _same(_solve(n, nb, trans, unit, Rs, Xs, scales, None, SOURCE), _solve(n, nb, trans, unit, Rs, Xs, scales, None, PERMUTE),
              f"in place n={n}")


def test_first_touch_source_on_64x64_tiles():
    """n = 512 with 8 chains: the top product of the recursion (N = 256) is the one launch shape here that takes 64 x 64 whole tiles and
    the XCD-grouped grid, as every spine product of the 128-chain contexts does"""
    n, nb = 512, 8
    rng, Rs, Xs, scales = _operands(n, nb, 1, 77)
    ps = [rng.permutation(n).astype(np.int32) for _ in range(nb)]
    _same(_solve(n, nb, 1, 1, Rs, Xs, scales, ps, SOURCE), _solve(n, nb, 1, 1, Rs, Xs, scales, ps, GATHER), "n=512")


def test_green_from_udv_lu_route_against_qr_route():
    """O(2), L = 8 (n_g = 128), QR stabilisation: G(beta) and the G of every boundary of a down pass from the LU route (greenVariant
    left at its default: both halves solved from the first-touch source) against the Householder route (greenVariant = 1: copies).
    Two different factorisations of the same well-conditioned Z: 1e-10 relative, the parity tolerance of the fixtures."""
    from detqmc_amd import KernelContext
    from detqmc_amd.model import DOWN
    kw = dict(opdim=2, L=8, m=20, s=5, dtau=0.1, delaySteps=4, stabilisation="qr", nchains=3)
    lu, qr = KernelContext(**kw), KernelContext(greenVariant=1, **kw)
    try:
        assert lu.schedule_info().green_lu == 1 and qr.schedule_info().green_lu == 0
        for b in range(3):
            rng = np.random.default_rng(50 + b)
            phi = rng.uniform(-0.8, 0.8, (lu.m + 1, lu.N, 2))
            phi[0] = 0.0
            for c in (lu, qr):
                c.select_chain(b)
                c.set_fields(phi)
        for c in (lu, qr):
            c.setupUdVStorage_and_calculateGreen()
        n = lu.n
        for step in range(n + 1):
            for b in range(3):
                lu.select_chain(b)
                qr.select_chain(b)
                g1, g2 = lu.g, qr.g
                assert np.max(np.abs(g1 - g2)) <= 1e-10 * np.max(np.abs(g2)), (step, b)
            if step < n:
                l = n - step
                for c in (lu, qr):
                    for k in range(c.currentTimeslice, (l - 1) * 5 + 1, -1):
                        c.wrapDownGreen(k)
                    c.wrapSkip(DOWN, (l - 1) * 5 + 1)
                    c.advanceDownGreen(l)
    finally:
        lu.close()
        qr.close()
