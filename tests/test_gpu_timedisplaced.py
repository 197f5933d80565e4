"""Time-displaced Green's functions G(tau,0), G(0,tau) at the stabilisation boundaries and the G(k, tau) observable.

Small beta: against direct numpy inverses of the oracle's B products (tests/td_reference.py).  Large beta, where a direct
inverse is meaningless: the chain identities between neighbouring boundaries, with short products from dqmc_bmult_host."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

L4 = dict(L=4, dtau=0.1)


def _walk(ctx, on_boundary):
    """down pass then up pass with wrap / advance only; on_boundary(tau, direction) after every interior advance"""
    m, s, n = ctx.m, ctx.s, ctx.n
    for k in range(m, (n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        on_boundary(s * l, "down")
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    on_boundary(0, "down-end")
    ctx.reset_storage0()
    for l in range(0, n - 1):
        for k in range(l * s + 1, (l + 1) * s + 1):
            ctx.wrapUpGreen(k - 1)
        ctx.advanceUpGreen(l)
        on_boundary(s * (l + 1), "up")
    for k in range((n - 1) * s + 1, m + 1):
        ctx.wrapUpGreen(k - 1)
    ctx.advanceUpGreen(n - 1)


def _context(opdim, L, m, s, dtau, stab, checkerboard=True, bc="pbc", **tuning):
    from detqmc_amd import KernelContext
    return KernelContext(opdim, L, m, s, dtau, delaySteps=4, bc=bc, stabilisation=stab, checkerboard=checkerboard,
                         timeDisplaced=True, **tuning)


def _random_phi(opdim, N, m, seed):
    phi = np.random.default_rng(seed).uniform(-1.0, 1.0, (m + 1, N, opdim))
    phi[0] = 0.0
    return phi


# (opdim, m, s, checkerboard, bc, tuning)
CASES = [
    (1, 20, 5, True, "pbc", {}),
    (2, 20, 5, True, "pbc", {}),
    (3, 20, 5, True, "pbc", {}),
    (2, 22, 5, True, "pbc", {}),             # s does not divide m: the last block is shorter
    (3, 22, 5, True, "pbc", {}),
    (2, 20, 5, False, "pbc", {}),            # dense B (checkerboard = false)
    (3, 20, 5, False, "pbc", {}),
    (2, 20, 5, True, "apbc-xy", {}),
    (2, 20, 5, True, "pbc", {"greenVariant": 1}),                   # QR route (Householder, Q in reflector form)
    (3, 22, 5, True, "pbc", {"greenVariant": 1, "qrVariant": 2}),   # QR route with block Gram-Schmidt (explicit Q)
]


# green_variant / qr_variant are QR-mode choices: the SVD mode runs the cases without them
@pytest.mark.parametrize("stab,opdim,m,s,cb,bc,tuning",
                         [("svd",) + c for c in CASES if not c[-1]] + [("qr",) + c for c in CASES])
def test_timedisplaced_vs_direct_inverse(stab, opdim, m, s, cb, bc, tuning):
    from td_reference import Chain, make_oracle
    N = 16
    phi = _random_phi(opdim, N, m, 1000 * opdim + m)
    ora = make_oracle(phi, opdim=opdim, L=4, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, delaySteps=4)
    assert ora.m == m and ora.s == s
    ch = Chain(ora)
    ctx = _context(opdim, 4, m, s, 0.1, stab, checkerboard=cb, bc=bc, **tuning)
    try:
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        seen = []

        def check(tau, how):
            g_dev = ctx.g
            if how == "down-end":
                return
            sl, gt0, g0t = ctx.green_timedisplaced()
            assert sl == tau
            g, gt0_ref, g0t_ref = ch.greens(tau)
            assert relerr(g_dev, g) < 1e-10, (tau, how)
            e1, e2 = relerr(gt0, gt0_ref), relerr(g0t, g0t_ref)
            assert e1 < 1e-10 and e2 < 1e-10, (tau, how, e1, e2)
            seen.append((how, tau))

        _walk(ctx, check)
        n = -(-m // s)
        assert sorted(t for h, t in seen if h == "down") == [s * j for j in range(1, n)]
        assert sorted(t for h, t in seen if h == "up") == [s * j for j in range(1, n)]
    finally:
        ctx.close()


def _chain_identities(ctx, phi):
    """max relative error of the three chain identities over all boundaries of a down + up walk"""
    ctx.set_fields(phi)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    pairs = {}
    g0 = {}

    def grab(tau, how):
        if how == "down-end":
            g0["g"] = ctx.g
            return
        sl, gt0, g0t = ctx.green_timedisplaced()
        assert sl == tau
        pairs.setdefault(how, {})[tau] = (gt0, g0t)

    _walk(ctx, grab)
    s, n = ctx.s, ctx.n
    errs = []
    for how in ("down", "up"):
        P = pairs[how]
        for j in range(1, n - 1):
            t0, t1 = s * j, s * (j + 1)
            errs.append(relerr(ctx.leftMultiplyBmat(P[t0][0], t1, t0), P[t1][0]))
            errs.append(relerr(ctx.rightMultiplyBmatInv(P[t0][1], t1, t0), P[t1][1]))
    # G(tau_1, 0) = B(tau_1, 0) G(0): G(0) of the same field (the down pass ends at tau = 0)
    errs.append(relerr(ctx.leftMultiplyBmat(g0["g"], s, 0), pairs["down"][s][0]))
    return max(errs)


@pytest.mark.parametrize("stab", ["svd", "qr"])
def test_timedisplaced_chain_identities_beta10(stab):
    ctx = _context(2, 8, 100, 10, 0.1, stab)
    try:
        err = _chain_identities(ctx, _random_phi(2, 64, 100, 7))
        print(f"O(2) L=8 beta=10 {stab}: max chain-identity relerr {err:.2e}")
        assert err < 1e-8
    finally:
        ctx.close()


def test_timedisplaced_chain_identities_qr_route_ng576():
    ctx = _context(3, 12, 40, 10, 0.1, "qr")      # n_g = 576 > 512: the inverse inside greenFromUdV goes by QR
    try:
        assert ctx.schedule_info().green_lu == 0
        err = _chain_identities(ctx, _random_phi(3, 144, 40, 11))
        print(f"O(3) L=12 n_g=576 qr: max chain-identity relerr {err:.2e}")
        assert err < 1e-8
    finally:
        ctx.close()


def test_timedisplaced_needs_reservation_and_boundary():
    from detqmc_amd import DqmcError, KernelContext
    ctx = KernelContext(2, 4, 20, 5, 0.1, delaySteps=4)
    try:
        with pytest.raises(DqmcError):
            ctx.set_timedisplaced(True)
        assert ctx.lib.dqmc_measure_td_accum_size(ctx.h) == 0
    finally:
        ctx.close()
    ctx = _context(2, 4, 20, 5, 0.1, "qr")
    try:
        ctx.set_fields(_random_phi(2, 16, 20, 3))
        ctx.setupUdVStorage_and_calculateGreen()
        with pytest.raises(DqmcError):
            ctx.green_timedisplaced()             # nothing computed yet
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced(2)
        ctx.measure_timedisplaced(3)
        acc = ctx.measure_td_read()
        assert list(acc[:3]) == [0.0, 0.0, 1.0]
    finally:
        ctx.close()


def _batch(opdim, td, seed=4711, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    import dataclasses
    p = SDWParams(opdim=opdim, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, timeDisplacedMeasurements=td, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


@pytest.mark.parametrize("opdim", [2, 3])
def test_greenktau_observable_vs_direct(opdim):
    from td_reference import Chain, green_k, make_oracle, shift_symmetric
    batch = _batch(opdim, True)
    try:
        for _ in range(3):
            batch.sweepThermalization()
        dirs = set()
        for _ in range(2):
            before = [batch.chain(b).phi.copy() for b in range(2)]
            batch.sweep(True)
            for b in range(2):
                rep = batch.chain(b)
                after = rep.phi.copy()
                info = rep.info
                down = info.lastSweepDir == -1
                dirs.add(down)
                taus = rep.tau_grid()
                n, s = info.n, info.s
                assert np.allclose(taus, [j * s * 0.1 for j in range(1, n)])
                gx, gy = rep.observable_vector("greenKTauX"), rep.observable_vector("greenKTauY")
                assert gx.shape == (n - 1, 16) and gy.shape == (n - 1, 16)
                worst = 0.0
                for j in range(1, n):
                    tau = s * j
                    phi = before[b].copy()
                    if down:
                        phi[tau + 1:] = after[tau + 1:]      # slices above tau_j already updated
                    else:
                        phi[1:tau + 1] = after[1:tau + 1]    # slices up to tau_j already updated
                    ora = make_oracle(phi, opdim=opdim, L=4, beta=2.0, dtau=0.1, s=s, delaySteps=4,
                                      r=batch.pars_list[b].r)
                    _, gt0, _ = Chain(ora).greens(tau)
                    ref = green_k(ora, shift_symmetric(ora, gt0))
                    worst = max(worst, relerr(gx[j - 1], ref[0]), relerr(gy[j - 1], ref[1]))
                assert worst < 1e-10, (b, down, worst)
        assert dirs == {True, False}
    finally:
        batch.close()


def test_option_changes_nothing_else():
    over = dict(globalShift=True, wolffClusterUpdate=True, globalUpdateInterval=1)
    a, b = _batch(2, False, **over), _batch(2, True, **over)
    try:
        names = ("kOccX", "kOccY", "pairPlus", "pairMinus")
        scal = ("meanPhi", "normMeanPhi", "associatedEnergy", "phiRhoS_Gc", "phiRhoS_Gs", "greenK0", "greenLocal",
                "pairPlusMax", "pairMinusMax", "occDiffSq")
        for it in range(6):
            if it < 2:
                a.sweepThermalization(); b.sweepThermalization()
            else:
                a.sweep(True); b.sweep(True)
            for c in range(2):
                ra, rb = a.chain(c), b.chain(c)
                assert np.array_equal(ra.phi, rb.phi)
                ia, ib = ra.info, rb.info
                assert ia.rngDrawn == ib.rngDrawn
                assert ia.acceptedGlobalShifts == ib.acceptedGlobalShifts
                assert ia.acceptedWolffClusterUpdates == ib.acceptedWolffClusterUpdates
                assert np.array_equal(ra.g, rb.g)
                if it >= 2:
                    oa, ob = ra.observables, rb.observables
                    for f in scal:
                        assert np.array_equal(np.asarray(getattr(oa, f)), np.asarray(getattr(ob, f))), f
                    for nm in names:
                        assert np.array_equal(ra.observable_vector(nm), rb.observable_vector(nm)), nm
        ka, kb = a.kernel_context, b.kernel_context
        assert ka.lib.dqmc_measure_accum_size(ka.h) == kb.lib.dqmc_measure_accum_size(kb.h)
        assert ka.lib.dqmc_measure_td_accum_size(ka.h) == 0 and kb.lib.dqmc_measure_td_accum_size(kb.h) > 0
        assert a.chain(0).info.attemptedGlobalShifts > 0
    finally:
        a.close(); b.close()
