"""Time-displaced current-current correlators Lambda_xx, Lambda_yy and the bond kinetic energy: the kernel against numpy on the device's
own four matrices, free fermions against the closed form, the accumulator block's bookkeeping, and the currentXTau / currentYTau /
bondKineticX / bondKineticY observables against direct inverses (tests/td_current_reference.py)."""
import dataclasses

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu


def _context(opdim, L, m, s, td=1, ph=2, stab="qr", checkerboard=True, bc="pbc", weakZflux=False, nchains=1, **kw):
    from detqmc_amd import KernelContext
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, bc=bc, weakZflux=weakZflux, stabilisation=stab,
                         checkerboard=checkerboard, nchains=nchains, timeDisplaced=td, tdParticleHole=ph, **kw)


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
    """(count, Lambda_xx sums, Lambda_yy sums, kinetic_x sum, kinetic_y sum) of boundary j"""
    off = (n - 1) + (j - 1) * (2 * N + 2)
    return acc[j - 1], acc[off:off + N], acc[off + N:off + 2 * N], acc[off + 2 * N], acc[off + 2 * N + 1]


def _start(ctx, phis):
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.measure_reset()


# (opdim, L, m, s, checkerboard, bc, weakZflux)
KERNEL_CASES = [
    (1, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "pbc", False),
    (3, 4, 20, 5, True, "pbc", False),
    (2, 4, 20, 5, True, "apbc-xy", False),        # sign flip on the wrapped bonds
    (2, 4, 20, 5, True, "pbc", True),             # flux: complex T, conjugate sector, phase on the boundary-crossing vertical bonds
    (2, 4, 20, 5, False, "pbc", False),           # dense B (checkerboard = false)
    (3, 4, 20, 5, False, "pbc", False),
    (2, 6, 20, 5, True, "pbc", False),            # N = 36: ragged second workgroup, x / y neighbours in different workgroups
    (3, 6, 20, 5, True, "pbc", False),
    (2, 16, 10, 5, True, "pbc", False),           # n_g = 512, one interior boundary
]


@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", KERNEL_CASES)
def test_kernel_vs_numpy_on_device_matrices(opdim, L, m, s, cb, bc, flux):
    from td_current_reference import current_correlators
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 700 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, checkerboard=cb, bc=bc, weakZflux=flux)
    try:
        n = ctx.n
        assert ctx.lib.dqmc_measure_td_current_accum_size(ctx.h) == (n - 1) * (1 + 2 * N + 2)
        assert ctx.lib.dqmc_measure_td_ph_accum_size(ctx.h) == (n - 1) * (1 + 3 * N)        # value 2 reserves what value 1 reserves
        _start(ctx, [phi])
        target = n - 1 if n == 2 else n - 2          # one boundary measured, the others must stay untouched
        ref = {}

        def at(j):
            if j != target:
                return
            gtt = ctx.g
            sl, gt0, g0t = ctx.green_timedisplaced()
            sl0, g00 = ctx.green0_timedisplaced()
            assert sl == s * j and sl0 == s * j
            ref["c"] = current_correlators(ora, *[shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)])
            ctx.measure_timedisplaced_current(j)
            assert np.array_equal(ctx.g, gtt)                                 # the measurement leaves G alone

        _walk_down(ctx, at)
        acc = ctx.measure_td_current_read()
        assert acc.shape == ((n - 1) * (1 + 2 * N + 2),)
        cnt, lx, ly, kx, ky = _block(acc, n, N, target)
        assert cnt == 1.0
        rx, ry, rkx, rky = ref["c"]
        errs = [relerr(lx / N, rx), relerr(ly / N, ry), relerr(kx / N, rkx), relerr(ky / N, rky)]
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux} j={target}: Lxx {errs[0]:.2e} Lyy {errs[1]:.2e} kx {errs[2]:.2e} ky {errs[3]:.2e}")
        for r in ref["c"]:
            assert np.abs(r).max() > 1e-6                                      # not a comparison of zeros
        assert max(errs) < 1e-10, errs
        for j in range(1, n):
            if j != target:
                c0, ax, ay, bx, by = _block(acc, n, N, j)
                assert c0 == 0.0 and not ax.any() and not ay.any() and bx == 0.0 and by == 0.0, j
        assert not ctx.measure_td_ph_read().any()                             # the particle-hole block is not touched
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim", [2, 3])
def test_free_fermions_on_device(opdim):
    """lambda = 0, dense hopping, periodic boundaries: the field decouples, the total current is conserved, and the row sums and the
    kinetic terms have closed forms (tests/td_current_reference.py).  The only error source is the engine's G: 1e-10."""
    from td_current_reference import free_fermion_closed_form
    L, m, s = 4, 20, 5
    N = L * L
    hop = dict(txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0, mux=-0.5, muy=-0.3)
    lam_ref, kin_ref = free_fermion_closed_form(L, m * 0.1, **hop)
    ctx = _context(opdim, L, m, s, checkerboard=False, lambda_=0.0, **hop)
    try:
        _start(ctx, [_random_phi(opdim, N, m, 40 + opdim)])
        _walk_down(ctx, ctx.measure_timedisplaced_current)
        acc = ctx.measure_td_current_read()
        n = ctx.n
        assert n - 1 == 3
        rows = []
        for j in range(1, n):
            cnt, lx, ly, kx, ky = _block(acc, n, N, j)
            assert cnt == 1.0
            rows.append((lx.sum() / N, ly.sum() / N, kx / N, ky / N))
            errs = [abs(rows[-1][0] / lam_ref[0] - 1), abs(rows[-1][1] / lam_ref[1] - 1), abs(rows[-1][2] / kin_ref[0] - 1), abs(rows[-1][3] / kin_ref[1] - 1)]
            print(f"O({opdim}) j={j}: Q0 x {rows[-1][0]:.13f} y {rows[-1][1]:.13f} kin x {rows[-1][2]:.13f} y {rows[-1][3]:.13f}; rel. errors {max(errs):.1e}")
            assert max(errs) < 1e-10, (j, errs)
        rows = np.array(rows)
        assert np.all(np.abs(rows - rows[0]) <= 1e-10 * np.abs(rows[0]))      # the same at all three boundaries
    finally:
        ctx.close()


def _measure_all(ctx, phis, twice_at=None):
    """down walk measuring every boundary; returns (block per chain, block of chain 0 right after the first measurement of twice_at)"""
    _start(ctx, phis)
    grabbed = {}

    def at(j):
        ctx.measure_timedisplaced_current(j)
        if j == twice_at:
            ctx.select_chain(0)
            grabbed["once"] = ctx.measure_td_current_read()
            ctx.measure_timedisplaced_current(j)

    _walk_down(ctx, at)
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append(ctx.measure_td_current_read())
    return out, grabbed.get("once")


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_and_reproducibility(opdim):
    N, m, s = 36, 20, 5
    phis = [_random_phi(opdim, N, m, 93 + opdim), _random_phi(opdim, N, m, 193 + opdim)]
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
    N = 16
    ctx = _context(2, 4, 20, 5, td=2, ph=1)                # value 1: no reservation
    try:
        assert ctx.lib.dqmc_measure_td_current_accum_size(ctx.h) == 0
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        ctx.measure_timedisplaced_ph(3)
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_current(3)
        with pytest.raises(DqmcError):
            ctx.measure_td_current_read()
    finally:
        ctx.close()
    for bad in (3, -1):
        with pytest.raises(DqmcError):
            _context(2, 4, 20, 5, ph=bad)
    with pytest.raises(DqmcError):
        _context(2, 4, 20, 5, td=0, ph=2)         # the flag without timedisplaced
    ctx = _context(2, 4, 20, 5, td=2)
    try:
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_current(3)  # nothing computed yet
        ctx.set_timedisplaced(True)
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                   # tau = 15, j = 3
        for j in (0, 2, 4):
            with pytest.raises(DqmcError):
                ctx.measure_timedisplaced_current(j)
        # either order with the other measurements of the boundary
        ctx.measure_timedisplaced_current(3)
        first = ctx.measure_td_current_read()
        ctx.measure_timedisplaced_ph(3)
        ctx.measure_timedisplaced_pair(3)
        ctx.measure_timedisplaced(3)
        ctx.measure_timedisplaced_current(3)
        acc = ctx.measure_td_current_read()
        assert list(acc[:3]) == [0.0, 0.0, 2.0] and not acc[3:3 + 2 * (2 * N + 2)].any()
        assert np.array_equal(acc[3 + 2 * (2 * N + 2):], 2.0 * first[3 + 2 * (2 * N + 2):]) and first[3 + 2 * (2 * N + 2):].all()
        ph_once = ctx.measure_td_ph_read()
        ctx.measure_timedisplaced_ph(3)           # ... and the particle-hole call after the current call
        assert np.array_equal(ctx.measure_td_ph_read(), 2.0 * ph_once) and ph_once.any()
        assert list(ctx.measure_td_read()[:3]) == [0.0, 0.0, 1.0]
        ctx.wrapDownGreen(15)
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_current(3)  # G has left the boundary
        ctx.measure_reset()
        assert not ctx.measure_td_current_read().any()
    finally:
        ctx.close()


def test_value_2_changes_nothing_else_at_kernel_level():
    """value 2 gives the same G, particle-hole block, pairing block and G(k, tau) bins, bit for bit, as value 1"""
    phi = _random_phi(3, 16, 20, 19)
    got = []
    for ph in (1, 2):
        ctx = _context(3, 4, 20, 5, td=2, ph=ph)
        try:
            _start(ctx, [phi])
            gs = []

            def at(j):
                if ph == 2:
                    ctx.measure_timedisplaced_current(j)
                ctx.measure_timedisplaced_ph(j)
                ctx.measure_timedisplaced(j)
                ctx.measure_timedisplaced_pair(j)
                gs.append(ctx.g)
                gs.extend(ctx.green_timedisplaced()[1:])
                gs.append(ctx.green0_timedisplaced()[1])

            _walk_down(ctx, at)
            ctx.advanceDownGreen(1)
            gs.append(ctx.g)
            got.append((gs, ctx.measure_td_read(), ctx.measure_td_pair_read(), ctx.measure_td_ph_read(), ctx.measure_read()))
        finally:
            ctx.close()
    (ga, ta, pa, ha, ma), (gb, tb, pb, hb, mb) = got
    assert len(ga) == len(gb) and all(np.array_equal(x, y) for x, y in zip(ga, gb))
    assert np.array_equal(ta, tb) and ta.any()
    assert np.array_equal(pa, pb) and pa.any()
    assert np.array_equal(ha, hb) and ha.any()
    assert np.array_equal(ma, mb)


def _batch(current, seed=4711, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=current, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


VEC = ("currentXTau", "currentYTau")
SCAL = ("bondKineticX", "bondKineticY")
NAMES = VEC + ("currentXTauQ0", "currentYTauQ0") + SCAL


def test_observables_vs_direct():
    from td_current_reference import current_correlators
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    batch = _batch(True)
    try:
        for _ in range(3):
            batch.sweepThermalization()
        kc = batch.kernel_context
        kc.select_chain(0)
        assert kc.lib.dqmc_measure_td_current_accum_size(kc.h) > 0 and not kc.measure_td_current_read().any()   # thermalisation measures nothing
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
                vec = [rep.observable_vector(nm) for nm in VEC]
                q0 = [rep.observable_vector(nm + "Q0") for nm in VEC]
                kin = [rep.observable_vector(nm) for nm in SCAL]
                assert all(v.shape == (n - 1, 16) for v in vec) and all(q.shape == (n - 1,) for q in q0 + kin)
                worst = 0.0
                for j in range(1, n):
                    tau = s * j
                    phi = before[b].copy()
                    if down:
                        phi[tau + 1:] = after[tau + 1:]      # slices above tau_j already updated
                    else:
                        phi[1:tau + 1] = after[1:tau + 1]    # slices up to tau_j already updated
                    ora = make_oracle(phi, opdim=2, L=4, beta=2.0, dtau=0.1, s=s, delaySteps=4, r=batch.pars_list[b].r)
                    ref = current_correlators(ora, *[shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)])
                    for mu in range(2):
                        worst = max(worst, relerr(vec[mu][j - 1], ref[mu]), relerr(kin[mu][j - 1], ref[2 + mu]))
                        # the q = 0 sum is the plain row sum: two summation orders of N terms differ by at most N eps sum|row|
                        assert abs(q0[mu][j - 1] - vec[mu][j - 1].sum()) <= 16 * np.finfo(float).eps * np.abs(vec[mu][j - 1]).sum(), (b, j)
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
        batch.chain(0).observable_vector("chargeTau")
        for nm in NAMES:
            with pytest.raises(DqmcError):
                batch.chain(0).observable_vector(nm)
    finally:
        batch.close()


def test_option_changes_nothing_else():
    over = dict(globalShift=True, wolffClusterUpdate=True, globalUpdateInterval=1)
    a, b = _batch(False, **over), _batch(True, **over)
    try:
        names = ("kOccX", "kOccY", "pairPlus", "pairMinus", "greenKTauX", "greenKTauY", "chargeTau", "spinZTau", "sdwTau",
                 "chargeTauQ0", "spinZTauQ0", "sdwTauQ0")
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
        assert ka.lib.dqmc_measure_td_ph_accum_size(ka.h) == kb.lib.dqmc_measure_td_ph_accum_size(kb.h) > 0
        assert ka.lib.dqmc_measure_td_current_accum_size(ka.h) == 0 and kb.lib.dqmc_measure_td_current_accum_size(kb.h) > 0
        assert a.chain(0).info.attemptedGlobalShifts > 0
    finally:
        a.close(); b.close()
