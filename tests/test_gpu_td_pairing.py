"""Time-displaced pairing correlators P+-(r, tau_j): the device kernel against numpy on the device's own G(tau_j, 0), the accumulator
block's bookkeeping, and the pairPlusTau / pairMinusTau observables against direct inverses (tests/td_pair_reference.py)."""
import dataclasses

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


def _context(opdim, L, m, s, td=2, checkerboard=True, bc="pbc", weakZflux=False, nchains=1):
    from detqmc_amd import KernelContext
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, bc=bc, weakZflux=weakZflux, stabilisation="qr",
                         checkerboard=checkerboard, nchains=nchains, timeDisplaced=td)


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


def _block(acc, n, N, j):
    """(count, T+ sums, T- sums) of boundary j"""
    off = (n - 1) + (j - 1) * 2 * N
    return acc[j - 1], acc[off:off + N], acc[off + N:off + 2 * N]


# (opdim, L, m, s, checkerboard, bc, weakZflux)
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
def test_kernel_vs_numpy_on_device_matrix(opdim, L, m, s, cb, bc, flux):
    from td_pair_reference import pair_correlators
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, checkerboard=cb, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_pair_accum_size(ctx.h) == (n - 1) * (1 + 2 * N)
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        ctx.measure_reset()
        target = n - 1 if n == 2 else n - 2          # one boundary measured, the others must stay untouched
        ref = {}

        def at(j):
            if j != target:
                return
            sl, gt0, _ = ctx.green_timedisplaced()
            assert sl == s * j
            ref["c"] = pair_correlators(ora, shift_symmetric(ora, gt0))
            ctx.measure_timedisplaced_pair(j)

        _walk_down(ctx, at)
        acc = ctx.measure_td_pair_read()
        assert acc.shape == ((n - 1) * (1 + 2 * N),)
        cnt, tp, tm = _block(acc, n, N, target)
        assert cnt == 1.0
        ep, em = relerr(tp / N, ref["c"][0]), relerr(tm / N, ref["c"][1])
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux} j={target}: C+ {ep:.2e} C- {em:.2e}")
        assert ep < 1e-10 and em < 1e-10
        for j in range(1, n):
            if j != target:
                c0, p0, m0 = _block(acc, n, N, j)
                assert c0 == 0.0 and not p0.any() and not m0.any(), j
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_and_reproducibility(opdim):
    N, m, s = 36, 20, 5
    phi = _random_phi(opdim, N, m, 91 + opdim)
    blocks = []
    for rep in range(2):
        ctx = _context(opdim, 6, m, s)
        try:
            ctx.set_fields(phi)
            ctx.setupUdVStorage_and_calculateGreen()
            ctx.set_timedisplaced(True)
            ctx.measure_reset()
            grabbed = {}

            def at(j):
                ctx.measure_timedisplaced_pair(j)
                if j == 2:
                    grabbed["once"] = ctx.measure_td_pair_read()
                    ctx.measure_timedisplaced_pair(j)

            _walk_down(ctx, at)
            acc = ctx.measure_td_pair_read()
            n = ctx.n
            c1, p1, m1 = _block(grabbed["once"], n, N, 2)
            c2, p2, m2 = _block(acc, n, N, 2)
            assert c1 == 1.0 and c2 == 2.0
            assert np.array_equal(p2, p1 + p1) and np.array_equal(m2, m1 + m1)       # v + v is exact
            assert np.any(p1 != 0.0) and np.any(m1 != 0.0)
            assert list(acc[:n - 1]) == [1.0, 2.0, 1.0]
            blocks.append(acc)
        finally:
            ctx.close()
    assert np.array_equal(blocks[0], blocks[1])


def test_preconditions_and_reset():
    from detqmc_amd import DqmcError
    phi = _random_phi(2, 16, 20, 3)
    ctx = _context(2, 4, 20, 5, td=1)
    try:
        assert ctx.lib.dqmc_measure_td_pair_accum_size(ctx.h) == 0
        assert ctx.lib.dqmc_measure_td_accum_size(ctx.h) > 0
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        ctx.measure_timedisplaced(3)
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_pair(3)
        with pytest.raises(DqmcError):
            ctx.measure_td_pair_read()
    finally:
        ctx.close()
    with pytest.raises(DqmcError):
        _context(2, 4, 20, 5, td=3)
    ctx = _context(2, 4, 20, 5)
    try:
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_pair(3)     # nothing computed yet
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        for j in (0, 2, 4):
            with pytest.raises(DqmcError):
                ctx.measure_timedisplaced_pair(j)
        ctx.measure_timedisplaced_pair(3)
        ctx.measure_timedisplaced(3)              # both measurements of one boundary, either order
        ctx.measure_timedisplaced_pair(3)
        acc = ctx.measure_td_pair_read()
        assert list(acc[:3]) == [0.0, 0.0, 2.0] and acc[3 + 2 * 32:].any()
        assert list(ctx.measure_td_read()[:3]) == [0.0, 0.0, 1.0]
        ctx.measure_reset()
        assert not ctx.measure_td_pair_read().any()
    finally:
        ctx.close()


def _batch(opdim, pairing, seed=4711, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=opdim, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedPairing=pairing, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


@pytest.mark.parametrize("opdim", [2, 3])
def test_pairtau_observable_vs_direct(opdim):
    from td_pair_reference import pair_correlators
    from td_reference import Chain, make_oracle, shift_symmetric
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
                n, s = info.n, info.s
                pp, pm = rep.observable_vector("pairPlusTau"), rep.observable_vector("pairMinusTau")
                qp, qm = rep.observable_vector("pairPlusTauQ0"), rep.observable_vector("pairMinusTauQ0")
                assert pp.shape == (n - 1, 16) and pm.shape == (n - 1, 16) and qp.shape == (n - 1,) and qm.shape == (n - 1,)
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
                    cp, cm = pair_correlators(ora, shift_symmetric(ora, gt0))
                    worst = max(worst, relerr(pp[j - 1], cp), relerr(pm[j - 1], cm))
                    # the q = 0 sum is the plain row sum; the two summation orders differ by at most N eps max|row| ~ 2e-15 max|row|
                    for q, row in ((qp[j - 1], pp[j - 1]), (qm[j - 1], pm[j - 1])):
                        assert abs(q - row.sum()) <= 1e-14 * max(1.0, np.abs(row).max()), (b, j)
                print(f"O({opdim}) chain {b} down={down}: worst relerr {worst:.2e}")
                assert worst < 1e-10, (b, down, worst)
        assert dirs == {True, False}
    finally:
        batch.close()


def test_pairtau_needs_the_option():
    from detqmc_amd import DqmcError
    batch = _batch(2, False)
    try:
        batch.sweepThermalization()
        batch.sweep(True)
        batch.chain(0).observable_vector("greenKTauX")
        for name in ("pairPlusTau", "pairMinusTau", "pairPlusTauQ0", "pairMinusTauQ0"):
            with pytest.raises(DqmcError):
                batch.chain(0).observable_vector(name)
    finally:
        batch.close()


def test_pairing_option_changes_nothing_else():
    over = dict(globalShift=True, wolffClusterUpdate=True, globalUpdateInterval=1)
    a, b = _batch(2, False, **over), _batch(2, True, **over)
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
                    assert rb.observable_vector("pairPlusTau").any()
        ka, kb = a.kernel_context, b.kernel_context
        assert ka.lib.dqmc_measure_accum_size(ka.h) == kb.lib.dqmc_measure_accum_size(kb.h)
        assert ka.lib.dqmc_measure_td_accum_size(ka.h) == kb.lib.dqmc_measure_td_accum_size(kb.h) > 0
        assert ka.lib.dqmc_measure_td_pair_accum_size(ka.h) == 0 and kb.lib.dqmc_measure_td_pair_accum_size(kb.h) > 0
        assert a.chain(0).info.attemptedGlobalShifts > 0
    finally:
        a.close(); b.close()
