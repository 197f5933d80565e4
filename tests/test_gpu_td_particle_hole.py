"""Time-displaced particle-hole correlators (charge, spinZ, sdw): G(0) of a boundary's own field configuration on the device, the
kernel against numpy on the device's own four matrices, the accumulator block's bookkeeping, and the chargeTau / spinZTau / sdwTau
observables against direct inverses (tests/td_ph_reference.py)."""
import dataclasses

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


def _context(opdim, L, m, s, td=1, ph=True, stab="qr", checkerboard=True, bc="pbc", weakZflux=False, nchains=1, **tuning):
    from detqmc_amd import KernelContext
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, bc=bc, weakZflux=weakZflux, stabilisation=stab,
                         checkerboard=checkerboard, nchains=nchains, timeDisplaced=td, tdParticleHole=ph, **tuning)


def _random_phi(opdim, N, m, seed):
    phi = np.random.default_rng(seed).uniform(-1.0, 1.0, (m + 1, N, opdim))
    phi[0] = 0.0
    return phi


def _walk_down(ctx, on_boundary):
    """down pass with wrap / advance only; on_boundary(j) after every interior advance (tau = s j)"""
    m, s, n = ctx.m, ctx.s, ctx.n
    for k in range(m, (n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        on_boundary(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)


def _walk_up(ctx, on_boundary):
    """the up pass that follows a complete down pass"""
    m, s, n = ctx.m, ctx.s, ctx.n
    ctx.advanceDownGreen(1)
    ctx.reset_storage0()
    for l in range(0, n - 1):
        for k in range(l * s + 1, (l + 1) * s + 1):
            ctx.wrapUpGreen(k - 1)
        ctx.advanceUpGreen(l)
        on_boundary(l + 1)


def _block(acc, n, N, j):
    """(count, charge sums, spinZ sums, sdw sums) of boundary j"""
    off = (n - 1) + (j - 1) * 3 * N
    return acc[j - 1], acc[off:off + N], acc[off + N:off + 2 * N], acc[off + 2 * N:off + 3 * N]


# (stab, opdim, L, m, s, tuning, both directions)
G0_CASES = [
    ("qr", 2, 4, 20, 5, {}, True),
    ("qr", 3, 4, 20, 5, {}, True),
    ("svd", 2, 4, 20, 5, {}, True),
    ("svd", 3, 4, 20, 5, {}, True),
    ("qr", 2, 4, 20, 5, {"greenVariant": 1}, False),                   # QR route, Q in reflector form
    ("qr", 3, 4, 20, 5, {"greenVariant": 1, "qrVariant": 2}, False),   # QR route, explicit Q (block Gram-Schmidt)
    ("qr", 2, 16, 10, 5, {}, False),                                   # n_g = 512: LU route, one boundary
    ("qr", 3, 12, 10, 5, {}, False),                                   # n_g = 576 > 512: QR route
]


@pytest.mark.parametrize("stab,opdim,L,m,s,tuning,both", G0_CASES)
def test_green0_on_device(stab, opdim, L, m, s, tuning, both):
    """G(0) of the half-way configuration against the direct inverse and against the inverse-free identities
    G(tau,0) = B(tau,0) G(0) and G(0,tau) B(tau,0) = -(1 - G(0)), B(tau,0) from the oracle's chain product"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle
    N = L * L
    phi = _random_phi(opdim, N, m, 500 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4)
    ch = Chain(ora)
    ctx = _context(opdim, L, m, s, stab=stab, **tuning)
    try:
        if stab == "qr":                              # the route the case is meant to take
            assert ctx.schedule_info().green_lu == int(ctx.ng <= 512 and tuning.get("greenVariant") != 1)
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        seen = []

        def at(j):
            tau = s * j
            sl, gt0, g0t = ctx.green_timedisplaced()
            sl0, g00 = ctx.green0_timedisplaced()
            assert sl == tau and sl0 == tau
            ref = four_greens(ch, tau)
            bt0 = ch.B(tau, 0)
            e_dir = relerr(g00, ref[3])
            e_a = relerr(bt0 @ g00, gt0)
            e_b = relerr(g0t @ bt0, -(np.eye(ctx.ng) - g00))
            print(f"{stab} O({opdim}) L={L} tau={tau}: direct {e_dir:.2e}, B G(0) {e_a:.2e}, G(0,tau) B {e_b:.2e}")
            assert e_dir < 1e-10, (tau, e_dir)
            assert e_a < 1e-8 and e_b < 1e-8, (tau, e_a, e_b)
            seen.append(j)

        _walk_down(ctx, at)
        if both:
            _walk_up(ctx, at)
        n = ctx.n
        assert sorted(seen) == sorted(list(range(1, n)) * (2 if both else 1))
    finally:
        ctx.close()


# the case list of test_gpu_td_pairing.py::KERNEL_CASES: (opdim, L, m, s, checkerboard, bc, weakZflux)
KERNEL_CASES = [
    (1, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "pbc", False),
    (3, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "apbc-xy", False),
    (2, 4, 20, 5, False, "pbc", False),           # dense B (checkerboard = false)
    (3, 4, 20, 5, False, "pbc", False),
    (2, 4, 20, 5, True, "pbc", True),             # magnetic flux: complex plaquette matrices
    (2, 6, 20, 5, True, "pbc", False),            # N = 36: not a multiple of a wave, two workgroups per chain
    (3, 6, 20, 5, True, "pbc", False),
    (2, 16, 10, 5, True, "pbc", False),           # n_g = 512, one interior boundary
]


@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", KERNEL_CASES)
def test_kernel_vs_numpy_on_device_matrices(opdim, L, m, s, cb, bc, flux):
    from td_ph_reference import ph_correlators
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, checkerboard=cb, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_ph_accum_size(ctx.h) == (n - 1) * (1 + 3 * N)
        assert ctx.lib.dqmc_measure_td_pair_accum_size(ctx.h) == 0          # timedisplaced = 1 is enough
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        ctx.measure_reset()
        target = n - 1 if n == 2 else n - 2          # one boundary measured, the others must stay untouched
        ref = {}

        def at(j):
            if j != target:
                return
            gtt = ctx.g
            sl, gt0, g0t = ctx.green_timedisplaced()
            sl0, g00 = ctx.green0_timedisplaced()
            assert sl == s * j and sl0 == s * j
            ref["c"] = ph_correlators(ora, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])
            ctx.measure_timedisplaced_ph(j)
            assert np.array_equal(ctx.g, gtt)                                 # the measurement leaves G alone

        _walk_down(ctx, at)
        acc = ctx.measure_td_ph_read()
        assert acc.shape == ((n - 1) * (1 + 3 * N),)
        cnt, *got = _block(acc, n, N, target)
        assert cnt == 1.0
        errs = [relerr(v / N, r) for v, r in zip(got, ref["c"])]
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux} j={target}: charge {errs[0]:.2e} spinZ {errs[1]:.2e} sdw {errs[2]:.2e}")
        for r in ref["c"]:
            assert np.abs(r).max() > 1e-6                                      # not a comparison of zeros
        assert max(errs) < 1e-10, errs
        for j in range(1, n):
            if j != target:
                c0, *rest = _block(acc, n, N, j)
                assert c0 == 0.0 and not any(v.any() for v in rest), j
    finally:
        ctx.close()


def _measure_all(ctx, phis, twice_at=None):
    """down walk measuring every boundary; returns (block per chain, block of chain 0 right after the first measurement of twice_at)"""
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.measure_reset()
    grabbed = {}

    def at(j):
        ctx.measure_timedisplaced_ph(j)
        if j == twice_at:
            ctx.select_chain(0)
            grabbed["once"] = ctx.measure_td_ph_read()
            ctx.measure_timedisplaced_ph(j)

    _walk_down(ctx, at)
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append(ctx.measure_td_ph_read())
    return out, grabbed.get("once")


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_and_reproducibility(opdim):
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 91 + opdim), _random_phi(opdim, N, m, 191 + opdim)]
    blocks = []
    for rep in range(2):
        ctx = _context(opdim, 6, m, s)
        try:
            (acc,), once = _measure_all(ctx, phis[:1], twice_at=2)
            n = ctx.n
            c1, *v1 = _block(once, n, N, 2)
            c2, *v2 = _block(acc, n, N, 2)
            assert c1 == 1.0 and c2 == 2.0
            for a, b in zip(v1, v2):
                assert np.array_equal(b, a + a) and np.any(a != 0.0)      # v + v is exact
            assert list(acc[:n - 1]) == [1.0, 2.0, 1.0]
            blocks.append(acc)
        finally:
            ctx.close()
    assert np.array_equal(blocks[0], blocks[1])                            # two fresh contexts: bit-identical
    # two chains in one context against the two single-chain results
    singles = []
    for phi in phis:
        ctx = _context(opdim, 6, m, s)
        try:
            singles.append(_measure_all(ctx, [phi])[0][0])
        finally:
            ctx.close()
    ctx = _context(opdim, 6, m, s, nchains=2)
    try:
        both, _ = _measure_all(ctx, phis)
    finally:
        ctx.close()
    assert not np.array_equal(singles[0], singles[1])
    assert np.array_equal(both[0], singles[0]) and np.array_equal(both[1], singles[1])


def test_preconditions_and_reset():
    from detqmc_amd import DqmcError
    phi = _random_phi(2, 16, 20, 3)
    ctx = _context(2, 4, 20, 5, td=2, ph=False)
    try:
        assert ctx.lib.dqmc_measure_td_ph_accum_size(ctx.h) == 0
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        ctx.measure_timedisplaced_pair(3)
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_ph(3)
        with pytest.raises(DqmcError):
            ctx.measure_td_ph_read()
        with pytest.raises(DqmcError):
            ctx.green0_timedisplaced()
    finally:
        ctx.close()
    with pytest.raises(DqmcError):
        _context(2, 4, 20, 5, td=0, ph=True)      # the flag without timedisplaced
    with pytest.raises(DqmcError):
        _context(2, 4, 20, 5, td=3, ph=True)      # timedisplaced keeps rejecting 3
    ctx = _context(2, 4, 20, 5)
    try:
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_ph(3)       # nothing computed yet
        with pytest.raises(DqmcError):
            ctx.green0_timedisplaced()
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        for j in (0, 2, 4):
            with pytest.raises(DqmcError):
                ctx.measure_timedisplaced_ph(j)
        ctx.measure_timedisplaced_ph(3)
        ctx.measure_timedisplaced(3)              # next to the other measurement of the boundary, either order
        ctx.measure_timedisplaced_ph(3)
        acc = ctx.measure_td_ph_read()
        assert list(acc[:3]) == [0.0, 0.0, 2.0] and acc[3 + 2 * 48:].any() and not acc[3:3 + 2 * 48].any()
        assert list(ctx.measure_td_read()[:3]) == [0.0, 0.0, 1.0]
        ctx.wrapDownGreen(15)
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_ph(3)       # G has left the boundary
        ctx.measure_reset()
        assert not ctx.measure_td_ph_read().any()
    finally:
        ctx.close()


def test_flag_changes_nothing_else_at_kernel_level():
    """a context with the flag gives the same G, G(k, tau) bins and pairing block, bit for bit, as one without it"""
    phi = _random_phi(3, 16, 20, 17)
    got = []
    for ph in (False, True):
        ctx = _context(3, 4, 20, 5, td=2, ph=ph)
        try:
            ctx.set_fields(phi)
            ctx.setupUdVStorage_and_calculateGreen()
            ctx.set_timedisplaced(True)
            ctx.measure_reset()
            gs = []

            def at(j):
                if ph:
                    ctx.measure_timedisplaced_ph(j)
                ctx.measure_timedisplaced(j)
                ctx.measure_timedisplaced_pair(j)
                gs.append(ctx.g)
                gs.extend(ctx.green_timedisplaced()[1:])

            _walk_down(ctx, at)
            ctx.advanceDownGreen(1)
            gs.append(ctx.g)
            got.append((gs, ctx.measure_td_read(), ctx.measure_td_pair_read(), ctx.measure_read()))
        finally:
            ctx.close()
    (ga, ta, pa, ma), (gb, tb, pb, mb) = got
    assert len(ga) == len(gb) and all(np.array_equal(x, y) for x, y in zip(ga, gb))
    assert np.array_equal(ta, tb) and ta.any()
    assert np.array_equal(pa, pb) and pa.any()
    assert np.array_equal(ma, mb)


def _batch(ph, seed=4711, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=ph, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


NAMES = ("chargeTau", "spinZTau", "sdwTau")


def test_observables_vs_direct():
    from td_ph_reference import four_greens, ph_correlators
    from td_reference import Chain, make_oracle, shift_symmetric
    batch = _batch(True)
    try:
        for _ in range(3):
            batch.sweepThermalization()
        kc = batch.kernel_context
        kc.select_chain(0)
        assert kc.lib.dqmc_measure_td_ph_accum_size(kc.h) > 0 and not kc.measure_td_ph_read().any()   # thermalisation measures nothing
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
                n, s = info.n, info.s
                vec = [rep.observable_vector(nm) for nm in NAMES]
                q0 = [rep.observable_vector(nm + "Q0") for nm in NAMES]
                assert all(v.shape == (n - 1, 16) for v in vec) and all(q.shape == (n - 1,) for q in q0)
                worst = 0.0
                for j in range(1, n):
                    tau = s * j
                    phi = before[b].copy()
                    if down:
                        phi[tau + 1:] = after[tau + 1:]      # slices above tau_j already updated
                    else:
                        phi[1:tau + 1] = after[1:tau + 1]    # slices up to tau_j already updated
                    ora = make_oracle(phi, opdim=2, L=4, beta=2.0, dtau=0.1, s=s, delaySteps=4, r=batch.pars_list[b].r)
                    ref = ph_correlators(ora, *[shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)])
                    for v, q, r in zip(vec, q0, ref):
                        worst = max(worst, relerr(v[j - 1], r))
                        # the q = 0 sum is the plain row sum; the two summation orders differ by at most N eps max|row|
                        assert abs(q[j - 1] - v[j - 1].sum()) <= 1e-14 * max(1.0, np.abs(v[j - 1]).max()), (b, j)
                print(f"chain {b} down={down}: worst relerr {worst:.2e}")
                assert worst < 1e-10, (b, down, worst)
        assert dirs == {True, False}
    finally:
        batch.close()


def test_observables_need_the_option():
    from detqmc_amd import DqmcError
    batch = _batch(False)
    try:
        batch.sweepThermalization()
        batch.sweep(True)
        batch.chain(0).observable_vector("greenKTauX")
        for nm in NAMES:
            for suffix in ("", "Q0"):
                with pytest.raises(DqmcError):
                    batch.chain(0).observable_vector(nm + suffix)
    finally:
        batch.close()


def test_option_changes_nothing_else():
    over = dict(globalShift=True, wolffClusterUpdate=True, globalUpdateInterval=1)
    a, b = _batch(False, **over), _batch(True, **over)
    try:
        names = ("kOccX", "kOccY", "pairPlus", "pairMinus", "greenKTauX", "greenKTauY")
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
                    assert all(rb.observable_vector(nm).any() for nm in NAMES)
        ka, kb = a.kernel_context, b.kernel_context
        assert ka.lib.dqmc_measure_accum_size(ka.h) == kb.lib.dqmc_measure_accum_size(kb.h)
        assert ka.lib.dqmc_measure_td_accum_size(ka.h) == kb.lib.dqmc_measure_td_accum_size(kb.h) > 0
        assert ka.lib.dqmc_measure_td_ph_accum_size(ka.h) == 0 and kb.lib.dqmc_measure_td_ph_accum_size(kb.h) > 0
        assert a.chain(0).info.attemptedGlobalShifts > 0
    finally:
        a.close(); b.close()
