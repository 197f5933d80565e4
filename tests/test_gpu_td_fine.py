"""Time-displaced correlators on every time slice (dqmc_measure_timedisplaced_segment / _ends, the ...Fine observables): propagation
on the device against numpy on the device's own boundary matrices and against direct inverses, the kernel rows against the numpy
channel references, coarse == fine bit for bit, reproducibility, non-interference and the preconditions.

Every test prints its figures before it asserts."""
import dataclasses

import numpy as np
import pytest

import td_fine_reference as tf
from conftest import relerr

pytestmark = pytest.mark.gpu

STRIDE = lambda ch, N, L: (4 * (2 * L - 1) ** 2, 2 * N, 3 * N, 2 * N + 2)[ch]


def _context(name, nchains=1, every=True, **kw):
    from detqmc_amd import KernelContext
    opdim, L, m, s, opt = tf.CASES[name]
    opt = dict(opt)
    opt.setdefault("stabilisation", "qr")
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, nchains=nchains, timeDisplaced=2, tdParticleHole=True, tdCurrent=True,
                         tdEverySlice=every, **opt, **kw)


def _start(ctx, phis):
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.measure_reset()


def _walk_down(ctx, on_boundary):
    m, s, n = ctx.m, ctx.s, ctx.n
    for k in range(m, (n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        on_boundary(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)


def _walk_up(ctx, on_boundary):
    m, s, n = ctx.m, ctx.s, ctx.n
    ctx.reset_storage0()
    for l in range(0, n - 1):
        for k in range(l * s + 1, (l + 1) * s + 1):
            ctx.wrapUpGreen(k - 1)
        ctx.advanceUpGreen(l)
        on_boundary(l + 1)
    for k in range((n - 1) * s + 1, m + 1):
        ctx.wrapUpGreen(k - 1)
    ctx.advanceUpGreen(n - 1)


def _state(ctx):
    sl, gt0, g0t = ctx.green_timedisplaced()
    sl0, g00 = ctx.green0_timedisplaced()
    return ctx.g, gt0, g0t, g00


def _rows(acc, ch, N, L, m):
    st = STRIDE(ch, N, L)
    return acc[:m + 1], acc[m + 1:].reshape(m + 1, st)


# ---- 2. propagation on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tf.CASES))
def test_propagation_on_device(name):
    """Every slice of every segment: the device's triple against (a) the oracle's B_k applied in numpy to the device's own boundary
    matrices -- the same arithmetic in another order, 1e-10, the project's parity bound -- and (b) the direct inverses of
    Chain.greens(k), 10 x e_ref (tests/test_td_fine_cpu.py; neither route is stabilised, the margin covers a different but equally
    valid operation order).  The call leaves G, the boundary pair and G(0) bit-identical."""
    opdim, L, m, s, _ = tf.CASES[name]
    phi, ora, chain = tf.case_chain(name)
    e_ref = tf.e_ref()
    ctx = _context(name)
    worst = {"a": 0.0, "b": 0.0}
    try:
        _start(ctx, [phi])

        def at(j):
            before = _state(ctx)
            g, gt0, g0t, _ = before
            up, down = tf.segment_slices(j, m, s)
            for k in up + down:
                ctx.td_fine_propagate(j, k)
                sl, f_t0, f_0t, f_tt = ctx.green_td_fine()
                assert sl == k
                ref_a = tf.propagate(chain.Bk, (gt0, g0t, g), j * s, k)
                d_tt, d_t0, d_0t = chain.greens(k)
                worst["a"] = max(worst["a"], tf.triple_err((f_t0, f_0t, f_tt), ref_a))
                worst["b"] = max(worst["b"], tf.triple_err((f_t0, f_0t, f_tt), (d_t0, d_0t, d_tt)))
            ctx.measure_timedisplaced_segment(j)
            sl, *_ = ctx.green_td_fine()
            assert sl == (down[-1] if down else up[-1])
            for x, y in zip(before, _state(ctx)):
                assert np.array_equal(x, y)

        _walk_down(ctx, at)
        if name.startswith("a"):
            _walk_up(ctx, at)
        print(f"case {name}: device vs numpy on its own boundary matrices {worst['a']:.2e} (bound 1e-10); vs direct inverses "
              f"{worst['b']:.2e} (bound 10 e_ref = {10 * e_ref:.2e}; this case's own numpy figure "
              f"{tf.case_e_ref(name) if name in tf.CPU_CASES else float('nan'):.2e})")
        assert worst["a"] < 1e-10
        assert worst["b"] < 10 * e_ref
    finally:
        ctx.close()


# ---- 3. kernel rows ------------------------------------------------------------------------------------------------------------
def _channel_refs(ora, gtt, gt0, g0t, g00):
    from td_current_reference import current_correlators
    from td_pair_reference import pair_correlators
    from td_ph_reference import ph_correlators
    from td_reference import shift_symmetric
    N = ora.N
    s_tt, s_t0, s_0t, s_00 = [shift_symmetric(ora, g) for g in (gtt, gt0, g0t, g00)]
    lx, ly, kx, ky = current_correlators(ora, s_tt, s_t0, s_0t, s_00)
    return [tf.td_bins(ora, s_t0),
            np.concatenate(pair_correlators(ora, s_t0)) * N,
            np.concatenate(ph_correlators(ora, s_tt, s_t0, s_0t, s_00)) * N,
            np.concatenate([lx, ly, [kx, ky]]) * N]


@pytest.mark.parametrize("name", list(tf.CASES))
def test_kernel_rows(name):
    """The segments of boundary 1 (both directions) and, where there is one, boundary 2, and the ends: one interior row of each direction
    of boundary 1, one of boundary 2 and rows 0 and m of every channel against numpy on the device's own four shifted matrices, 1e-10;
    rows of the other segments stay empty."""
    opdim, L, m, s, _ = tf.CASES[name]
    N = L * L
    phi, ora, _ = tf.case_chain(name)
    ctx = _context(name)
    try:
        for ch in range(4):
            assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, ch) == (m + 1) * (1 + STRIDE(ch, N, L))
        _start(ctx, [phi])
        refs = {}
        # boundary 1: one slice reached upward, one reached downward; boundary 2 (if any): one slice in the middle of its segment
        picks = {1: (s + 2, 2), 2: (2 * s + 2,)}

        def at(j):
            if j not in picks or j > ctx.n - 1:
                return
            g00 = ctx.green0_timedisplaced()[1]
            for k in picks[j]:
                ctx.td_fine_propagate(j, k)
                _, f_t0, f_0t, f_tt = ctx.green_td_fine()
                refs[k] = _channel_refs(ora, f_tt, f_t0, f_0t, g00)
            ctx.measure_timedisplaced_segment(j)

        _walk_down(ctx, at)
        g = ctx.g
        one = np.eye(ctx.ng)
        refs[0] = _channel_refs(ora, g, g, g - one, g)
        refs[m] = _channel_refs(ora, g, one - g, -g, g)
        ctx.measure_timedisplaced_ends()
        assert ctx.green_td_fine()[0] == m
        assert np.array_equal(ctx.g, g)
        measured = set(range(0, min((3 if ctx.n > 2 else 2) * s, m))) | {m}
        assert len(refs) == (5 if ctx.n > 2 else 4)
        worst = 0.0
        for ch in range(4):
            cnt, rows = _rows(ctx.measure_td_fine_read(ch), ch, N, L, m)
            for k in range(m + 1):
                if k in measured:
                    assert cnt[k] == 1.0, (ch, k)
                else:
                    assert cnt[k] == 0.0 and not rows[k].any(), (ch, k)
            for k, ref in refs.items():
                assert np.abs(ref[ch]).max() > 1e-6          # not a comparison of zeros
                e = relerr(rows[k], ref[ch])
                worst = max(worst, e)
                assert e < 1e-10, (ch, k, e)
        print(f"case {name}: rows {sorted(refs)} of four channels vs numpy, largest relative error {worst:.2e}")
    finally:
        ctx.close()


# ---- 4. coarse == fine, 6. non-interference (host layer) ---------------------------------------------------------------------------
COARSE = ["greenKTauX", "greenKTauY", "pairPlusTau", "pairMinusTau", "pairPlusTauQ0", "pairMinusTauQ0", "chargeTau", "spinZTau",
          "sdwTau", "chargeTauQ0", "spinZTauQ0", "sdwTauQ0", "currentXTau", "currentYTau", "currentXTauQ0", "currentYTauQ0",
          "bondKineticX", "bondKineticY"]


def _batch(opdim, every, beta=2.0, stab="qr", chains=2, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=opdim, L=4, beta=beta, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation=stab,
                  fermionMeasurements=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=True, timeDisplacedEverySlice=every, rngSeed=815, **over)
    return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.2 * i) for i in range(chains)])


@pytest.mark.parametrize("opdim,beta,stab", [(2, 2.0, "qr"), (3, 2.0, "qr"), (2, 2.2, "svd")])
def test_coarse_rows_equal_fine_rows(opdim, beta, stab):
    batch = _batch(opdim, True, beta=beta, stab=stab)
    try:
        batch.sweepThermalization()
        for _ in range(2):                                   # one sweep of each direction
            batch.sweep(True)
            kc = batch.kernel_context
            for b in range(2):
                rep = batch.chain(b)
                info = rep.info
                m, s, n = info.m, info.s, info.n
                assert np.allclose(rep.tau_grid(fine=True), 0.1 * np.arange(m + 1), rtol=0, atol=1e-14)
                for nm in COARSE:
                    coarse, fine = rep.observable_vector(nm), rep.observable_vector(nm + "Fine")
                    assert fine.shape[0] == m + 1 and coarse.shape[0] == n - 1
                    for j in range(1, n):
                        assert np.array_equal(fine[j * s], coarse[j - 1]), (nm, j)
                    assert np.any(fine != 0.0)
                c = rep.observable_vector("chargeTauFine")
                # n(d) and n(0) commute: <n_d(beta-) n_0(0)> = <n_0(0) n_d(0)> = <n_d(0+) n_0(0)>
                assert relerr(c[0], c[m]) < 1e-10
                kc.select_chain(b)
                for ch in range(4):
                    assert np.array_equal(kc.measure_td_fine_read(ch)[:m + 1], np.ones(m + 1)), ch
    finally:
        batch.close()


def test_option_changes_nothing_else():
    a, b = _batch(2, False), _batch(2, True)
    try:
        for it in range(2):
            a.sweep(True); b.sweep(True)
        ka, kb = a.kernel_context, b.kernel_context
        fine_before = [kb.measure_td_fine_read(ch) for ch in range(4)]
        ka.profile_enable(False); kb.profile_enable(False)  # clears the launch counters of both contexts; they count without timing too
        for it in range(2):
            a.sweepThermalization(); b.sweepThermalization()
        # thermalisation sweeps launch none of the new calls: every kernel family's launch count is that of the context without the flag
        fams = ("bmult", "gemm", "decomp", "decide", "other", "gather", "flush")
        pa, pb = ka.profile_read(), kb.profile_read()
        la, lb = [pa[f][1] for f in fams], [pb[f][1] for f in fams]
        print("launches per family, two thermalisation sweeps: without the flag", la, "with it", lb)
        assert la == lb and sum(la) > 0
        for ch in range(4):
            assert np.array_equal(kb.measure_td_fine_read(ch), fine_before[ch])
        a.sweep(True); b.sweep(True)
        for c in range(2):
            ra, rb = a.chain(c), b.chain(c)
            assert np.array_equal(ra.phi, rb.phi)
            assert np.array_equal(ra.g, rb.g)
            assert ra.info.rngDrawn == rb.info.rngDrawn
            for nm in COARSE + ["kOccX", "kOccY", "pairPlus", "pairMinus"]:
                assert np.array_equal(ra.observable_vector(nm), rb.observable_vector(nm)), nm
        ka = a.kernel_context
        assert ka.lib.dqmc_measure_td_fine_accum_size(ka.h, 0) == 0
    finally:
        a.close(); b.close()


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------
def _measure_everything(ctx, phis):
    _start(ctx, phis)
    _walk_down(ctx, ctx.measure_timedisplaced_segment)
    ctx.measure_timedisplaced_ends()
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append([ctx.measure_td_fine_read(ch) for ch in range(4)])
    return out


@pytest.mark.parametrize("name", ["f2", "a3"])
def test_reproducible_and_independent_of_the_batch(name):
    opdim, L, m, s, _ = tf.CASES[name]
    phis = [tf.random_phi(opdim, L * L, m, 31), tf.random_phi(opdim, L * L, m, 32)]
    runs = []
    for rep in range(2):
        ctx = _context(name, nchains=2)
        try:
            runs.append(_measure_everything(ctx, phis))
        finally:
            ctx.close()
    singles = []
    for phi in phis:
        ctx = _context(name)
        try:
            singles.append(_measure_everything(ctx, [phi])[0])
        finally:
            ctx.close()
    for b in range(2):
        for ch in range(4):
            assert np.array_equal(runs[0][b][ch][:m + 1], np.ones(m + 1))
            assert np.array_equal(runs[0][b][ch], runs[1][b][ch]), (b, ch)
            assert np.array_equal(runs[0][b][ch], singles[b][ch]), (b, ch)
    assert not np.array_equal(singles[0][2], singles[1][2])


# ---- 7. preconditions --------------------------------------------------------------------------------------------------------------
def test_preconditions():
    from detqmc_amd import DetSDW, DqmcError, KernelContext, SDWParams
    phi = tf.random_phi(2, 16, 20, 5)
    ctx = _context("a2", every=False)
    try:
        _start(ctx, [phi])
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)
        with pytest.raises(DqmcError) as e:
            ctx.measure_timedisplaced_segment(3)            # the option is not set
        assert e.value.code == -1
        with pytest.raises(DqmcError):
            ctx.measure_timedisplaced_ends()
        assert ctx.lib.dqmc_measure_td_fine_accum_size(ctx.h, 0) == 0
    finally:
        ctx.close()
    ctx = _context("a2")
    try:
        _start(ctx, [phi])
        with pytest.raises(DqmcError):
            ctx.green_td_fine()                             # nothing propagated yet
        ctx.measure_timedisplaced_ends()                    # at tau = beta right after the set-up: allowed
        for k in range(20, 15, -1):
            ctx.wrapDownGreen(k)
        ctx.advanceDownGreen(4)                             # tau = 15, j = 3
        for bad in (2, 0, 4):
            with pytest.raises(DqmcError) as e:
                ctx.measure_timedisplaced_segment(bad)      # a wrong j
            assert e.value.code == -1
        with pytest.raises(DqmcError) as e:
            ctx.measure_timedisplaced_ends()                # away from tau = 0
        assert e.value.code == -1
        with pytest.raises(DqmcError):
            ctx.td_fine_propagate(3, 14)
        ctx.measure_timedisplaced_segment(3)
        ctx.wrapDownGreen(15)
        with pytest.raises(DqmcError) as e:
            ctx.measure_timedisplaced_segment(3)            # after a wrap the context has left the boundary
        assert e.value.code == -1
    finally:
        ctx.close()
    for bad in (0x200 | 1, 0x100, 0x100 | 3):               # an unknown bit, the flag without a level, an unknown level
        with pytest.raises(DqmcError) as e:
            KernelContext(2, 4, 20, 5, 0.1, delaySteps=4, timeDisplaced=bad)
        assert e.value.code == -1
    rep = DetSDW(SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", fermionMeasurements=True,
                           timeDisplacedMeasurements=True, timeDisplacedParticleHole=True))
    try:
        rep.sweep(True)
        rep.observable_vector("chargeTau")
        for nm in ("greenKTauXFine", "chargeTauFine", "pairPlusTauFine"):
            with pytest.raises(DqmcError):
                rep.observable_vector(nm)
        with pytest.raises(DqmcError):
            rep.tau_grid(fine=True)
    finally:
        rep.close()
