"""Equal-time charge, spin-z, SDW and pairing correlators (dqmc_set_equal_time_correlators): the kernel against numpy on the device's
own shifted matrix, against the time-displaced kernels at tau = 0, against free fermions, the block's bookkeeping, the switch, and the
'...Corr' / '...Sq' observables of the host layer against direct inverses (tests/eq_corr_reference.py)."""
import dataclasses

import numpy as np
import pytest

from conftest import relerr
from test_gpu_td_particle_hole import KERNEL_CASES, _random_phi, _walk_down

pytestmark = pytest.mark.gpu


def _context(opdim, L, m, s, checkerboard=True, bc="pbc", weakZflux=False, nchains=1, **kw):
    from detqmc_amd import KernelContext
    kw.setdefault("stabilisation", "qr")
    return KernelContext(opdim, L, m, s, 0.1, delaySteps=4, bc=bc, weakZflux=weakZflux, checkerboard=checkerboard, nchains=nchains, **kw)


def _rows(acc, N):
    """(count, [charge, spinZ, sdw, pairPlus, pairMinus] sums) of one chain's block"""
    assert acc.shape == (1 + 5 * N,)
    return acc[0], [acc[1 + c * N:1 + (c + 1) * N] for c in range(5)]


def _start(ctx, phis):
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()


def _walk_to(ctx, k_stop):
    """down pass with wrap / advance only until the context stands on slice k_stop of the last-but-one segment"""
    m, s, n = ctx.m, ctx.s, ctx.n
    for k in range(m, (n - 1) * s, -1):
        ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(n)
    for k in range((n - 1) * s, k_stop, -1):
        ctx.wrapDownGreen(k)


# ---- 1. kernel against numpy on the device's own matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,m,s,cb,bc,flux", KERNEL_CASES)
def test_kernel_vs_numpy_on_device_matrix(opdim, L, m, s, cb, bc, flux):
    from eq_corr_reference import NAMES, eq_correlators
    from td_reference import make_oracle, shift_symmetric
    N = L * L
    phi = _random_phi(opdim, N, m, 300 * opdim + L + m)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=cb, weakZflux=flux, delaySteps=4)
    ctx = _context(opdim, L, m, s, checkerboard=cb, bc=bc, weakZflux=flux)
    try:
        _start(ctx, [phi])
        _walk_to(ctx, (ctx.n - 1) * s - 2)              # an interior slice, two wraps below the last boundary
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 0
        ctx.set_equal_time_correlators(True)
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 1 + 5 * N
        ctx.measure_reset()
        g = ctx.g
        ref = eq_correlators(ora, shift_symmetric(ora, g))
        ctx.measure_slice()
        assert np.array_equal(ctx.g, g)                  # the measurement leaves G alone
        cnt, got = _rows(ctx.measure_eq_read(), N)
        assert cnt == 1.0
        errs = [relerr(v / N, r) for v, r in zip(got, ref)]
        print(f"O({opdim}) L={L} {bc} cb={cb} flux={flux}: " + " ".join(f"{nm} {e:.2e}" for nm, e in zip(NAMES, errs)))
        for r in ref:
            assert np.abs(r).max() > 1e-6                # not a comparison of zeros
        assert max(errs) < 1e-10, errs
    finally:
        ctx.close()


# ---- 2. agreement with the time-displaced kernels at tau = 0 -----------------------------------------------------------------------
@pytest.mark.parametrize("opdim", [2, 3])
def test_agrees_with_time_displaced_row_zero(opdim):
    """row 0 of the every-slice blocks is measured from (G(0), G(0) - 1): the same quantity from the other kernels"""
    L, m, s = 4, 20, 5
    N = L * L
    phi = _random_phi(opdim, N, m, 77 + opdim)
    ctx = _context(opdim, L, m, s, timeDisplaced=2, tdParticleHole=True, tdEverySlice=True)
    try:
        _start(ctx, [phi])
        ctx.set_timedisplaced(True)
        _walk_down(ctx, lambda j: None)                  # to tau = 0, no updates
        ctx.set_equal_time_correlators(True)
        ctx.measure_reset()
        ctx.measure_timedisplaced_ends()
        ctx.measure_slice()
        cnt, got = _rows(ctx.measure_eq_read(), N)
        assert cnt == 1.0
        ph = ctx.measure_td_fine_read(2)
        pr = ctx.measure_td_fine_read(1)
        assert ph[0] == 1.0 and pr[0] == 1.0
        fine = [ph[m + 1 + c * N:m + 1 + (c + 1) * N] for c in range(3)] + [pr[m + 1 + c * N:m + 1 + (c + 1) * N] for c in range(2)]
        errs = [relerr(a, b) for a, b in zip(got, fine)]
        print(f"O({opdim}): equal-time block vs fine row 0: " + " ".join(f"{e:.2e}" for e in errs))
        assert all(np.abs(f).max() > 1e-6 for f in fine)
        assert max(errs) < 1e-10, errs
    finally:
        ctx.close()


# ---- 3. free fermions --------------------------------------------------------------------------------------------------------------
def test_free_fermions():
    """lambda = 0, dense hopping: the field decouples, G = (1 + e^{-beta K})^-1 on every slice and commutes with the shift.  e^{-dtau K}
    is the oracle's single-slice B matrix at lambda = 0.  The only error source is the engine's G: 1e-10."""
    from eq_corr_reference import NAMES, eq_correlators
    from td_reference import Chain, make_oracle
    opdim, L, m, s = 2, 4, 20, 5
    N = L * L
    hop = dict(txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0, mux=-0.5, muy=-0.3)
    phi = _random_phi(opdim, N, m, 42)
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, checkerboard=False, delaySteps=4, lambda_=0.0, **hop)
    Bk = Chain(ora).Bk
    assert relerr(Bk[3], Bk[11]) < 1e-14                 # no field dependence left
    G = np.linalg.inv(np.eye(ora.ng) + np.linalg.matrix_power(Bk[1], m))
    ref = eq_correlators(ora, G)
    ctx = _context(opdim, L, m, s, checkerboard=False, lambda_=0.0, **hop)
    try:
        _start(ctx, [phi])
        _walk_to(ctx, (ctx.n - 1) * s - 2)
        ctx.set_equal_time_correlators(True)
        ctx.measure_reset()
        ctx.measure_slice()
        cnt, got = _rows(ctx.measure_eq_read(), N)
        errs = [relerr(v / N, r) for v, r in zip(got, ref)]
        print("free fermions: " + " ".join(f"{nm} {e:.2e}" for nm, e in zip(NAMES, errs)))
        assert cnt == 1.0 and all(np.abs(r).max() > 1e-6 for r in ref)
        assert max(errs) < 1e-10, errs
    finally:
        ctx.close()


# ---- 4. accumulation and reproducibility -------------------------------------------------------------------------------------------
def _measure(ctx, phis, twice=False):
    """one interior slice measured (twice: two calls); returns (block per chain, block of chain 0 after the first call)"""
    _start(ctx, phis)
    _walk_to(ctx, (ctx.n - 1) * ctx.s - 1)
    ctx.set_equal_time_correlators(True)
    ctx.measure_reset()
    ctx.measure_slice()
    ctx.select_chain(0)
    once = ctx.measure_eq_read()
    if twice:
        ctx.measure_slice()
    out = []
    for b in range(len(phis)):
        ctx.select_chain(b)
        out.append(ctx.measure_eq_read())
    return out, once


@pytest.mark.parametrize("opdim", [2, 3])
def test_accumulation_and_reproducibility(opdim):
    L, N, m, s = 6, 36, 20, 5
    phis = [_random_phi(opdim, N, m, 91 + opdim), _random_phi(opdim, N, m, 191 + opdim)]
    blocks = []
    for rep in range(2):
        ctx = _context(opdim, L, m, s)
        try:
            (acc,), once = _measure(ctx, phis[:1], twice=True)
            assert once[0] == 1.0 and acc[0] == 2.0
            assert np.array_equal(acc[1:], once[1:] + once[1:])             # v + v is exact
            for v in _rows(once, N)[1]:
                assert np.any(v != 0.0)
            blocks.append(acc)
        finally:
            ctx.close()
    assert np.array_equal(blocks[0], blocks[1])                              # two fresh contexts: bit-identical
    singles = []
    for phi in phis:
        ctx = _context(opdim, L, m, s)
        try:
            singles.append(_measure(ctx, [phi])[0][0])
        finally:
            ctx.close()
    ctx = _context(opdim, L, m, s, nchains=2)
    try:
        both, _ = _measure(ctx, phis)
    finally:
        ctx.close()
    assert not np.array_equal(singles[0], singles[1])
    assert np.array_equal(both[0], singles[0]) and np.array_equal(both[1], singles[1])


# ---- 5. the switch -----------------------------------------------------------------------------------------------------------------
def test_switch():
    from detqmc_amd import DetHubbard, DqmcError, HubbardParams
    opdim, L, m, s = 3, 4, 20, 5
    N = L * L
    phi = _random_phi(opdim, N, m, 17)

    def walk(ctx, mode):
        """measure_slice on the slices of the top segment; mode: None never enabled, False enabled then off, True on"""
        _start(ctx, [phi])
        if mode is not None:
            ctx.set_equal_time_correlators(True)
            ctx.set_equal_time_correlators(mode)
        ctx.measure_reset()
        for k in range(m, (ctx.n - 1) * s, -1):
            ctx.measure_slice()
            ctx.wrapDownGreen(k)
        return ctx.measure_read()

    ctx = _context(opdim, L, m, s)
    try:
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 0
        with pytest.raises(DqmcError) as e:
            ctx.measure_eq_read()
        assert e.value.code == -1                        # DQMC_EINVAL
        never = walk(ctx, None)
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 0
    finally:
        ctx.close()
    ctx = _context(opdim, L, m, s)
    try:
        off = walk(ctx, False)
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 1 + 5 * N
        assert not ctx.measure_eq_read().any()           # allocated, switched off: nothing written
    finally:
        ctx.close()
    ctx = _context(opdim, L, m, s)
    try:
        on = walk(ctx, True)
        acc = ctx.measure_eq_read()
        assert acc[0] == float(s) and all(v.any() for v in _rows(acc, N)[1])
        ctx.measure_reset()
        assert not ctx.measure_eq_read().any()
        assert ctx.lib.dqmc_measure_eq_accum_size(ctx.h) == 1 + 5 * N
    finally:
        ctx.close()
    assert never.any() and np.array_equal(never, off) and np.array_equal(never, on)
    rep = DetHubbard(HubbardParams(L=4, beta=1.0, dtau=0.1, s=5))
    try:
        h = rep.lib.dethubbard_ctx(rep.h)
        assert rep.lib.dqmc_set_equal_time_correlators(h, 1) == -1
        assert rep.lib.dqmc_measure_eq_accum_size(h) == 0
    finally:
        rep.close()


# ---- 6. host observables -----------------------------------------------------------------------------------------------------------
CORR = ("chargeCorr", "spinZCorr", "sdwCorr", "pairPlusCorr", "pairMinusCorr")
SQ = ("chargeSq", "spinZSq", "sdwSq", "pairPlusSq", "pairMinusSq")


def _batch(eq, seed=4711, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=1.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr",
                  fermionMeasurements=True, equalTimeCorrelators=eq, rngSeed=seed, **over)
    return DetSDWBatch([p, dataclasses.replace(p, simindex=1, r=-0.8)])


def test_option_changes_nothing_else():
    a, b = _batch(False), _batch(True)
    try:
        names = ("kOccX", "kOccY", "pairPlus", "pairMinus")
        scal = ("meanPhi", "normMeanPhi", "associatedEnergy", "phiRhoS_Gc", "phiRhoS_Gs", "greenK0", "greenLocal",
                "pairPlusMax", "pairMinusMax", "occDiffSq")
        for it in range(3):
            if it < 2:
                a.sweepThermalization(); b.sweepThermalization()
            else:
                kb = b.kernel_context
                assert kb.lib.dqmc_measure_eq_accum_size(kb.h) == 0          # thermalisation sweeps launch nothing new
                a.sweep(True); b.sweep(True)
            for c in range(2):
                ra, rb = a.chain(c), b.chain(c)
                assert np.array_equal(ra.phi, rb.phi)
                assert ra.info.rngDrawn == rb.info.rngDrawn
                assert np.array_equal(ra.g, rb.g)
        for c in range(2):
            ra, rb = a.chain(c), b.chain(c)
            oa, ob = ra.observables, rb.observables
            for f in scal:
                assert np.array_equal(np.asarray(getattr(oa, f)), np.asarray(getattr(ob, f))), f
            for nm in names:
                assert np.array_equal(ra.observable_vector(nm), rb.observable_vector(nm)), nm
            assert all(rb.observable_vector(nm).any() for nm in CORR + SQ)
    finally:
        a.close(); b.close()


def test_observables_vs_direct():
    """the '...Corr' vectors against G(tau_k) of the half-updated field by direct inverse, slice by slice (the new field on the side
    already swept, the old one on the other), shifted, through the reference; 1e-10, the bound of the time-displaced observables'
    direct inverses.  The '...Sq' vectors against structure_factor of the returned '...Corr': N = 16 terms of host arithmetic, 1e-12."""
    from detqmc_amd import structure_factor
    from eq_corr_reference import eq_correlators
    from td_reference import Chain, make_oracle, shift_symmetric
    batch = _batch(True)
    try:
        for _ in range(2):
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
                m, s = info.m, info.s
                vec = [rep.observable_vector(nm) for nm in CORR]
                sq = [rep.observable_vector(nm) for nm in SQ]
                assert all(v.shape == (16,) for v in vec + sq)
                ref = [np.zeros(16) for _ in CORR]
                for k in range(1, m + 1):
                    phi = before[b].copy()
                    if down:
                        phi[k:] = after[k:]              # slices k .. m already updated
                    else:
                        phi[1:k + 1] = after[1:k + 1]    # slices 1 .. k already updated
                    ora = make_oracle(phi, opdim=2, L=4, beta=1.0, dtau=0.1, s=s, delaySteps=4, r=batch.pars_list[b].r)
                    g = Chain(ora).greens(k)[0]
                    for acc, r in zip(ref, eq_correlators(ora, shift_symmetric(ora, g))):
                        acc += r / m
                errs = [relerr(v, r) for v, r in zip(vec, ref)]
                print(f"chain {b} down={down}: " + " ".join(f"{e:.2e}" for e in errs))
                assert max(errs) < 1e-10, (b, down, errs)
                for v, q in zip(vec, sq):
                    assert relerr(q, structure_factor(v, 4)) < 1e-12
        assert dirs == {True, False}
    finally:
        batch.close()


def test_observables_need_the_option():
    from detqmc_amd import DetSDW, DqmcError, SDWParams, _lib
    batch = _batch(False)
    try:
        batch.sweepThermalization()
        batch.sweep(True)
        batch.chain(0).observable_vector("pairPlus")
        for nm in CORR + SQ:
            with pytest.raises(DqmcError, match="equalTimeCorrelators"):
                batch.chain(0).observable_vector(nm)
            with pytest.raises(KeyError):
                batch.chain(0).observable_vector(nm + "Fine")
    finally:
        batch.close()
    batch = _batch(True)
    try:
        batch.sweep(True)
        out = np.zeros(16 * 21)
        for which in range(22, 32):                      # which | DETSDW_OBS_FINE stays an error
            assert batch.lib.detsdw_get_observable_vector(batch.h, which | _lib.DETSDW_OBS_FINE, out.ctypes.data_as(_lib._DP)) != 0
    finally:
        batch.close()
    # the bit without fermionMeasurements, and an unknown bit: ParameterWrong at creation
    from detqmc_amd.model import _host_params
    import ctypes as C
    lib = _lib.load()
    for fm in (_lib.DETSDW_FM_EQ_CORRELATORS, 2, 0x200 | 1):
        p = _host_params(SDWParams(opdim=2, L=4, beta=1.0, s=5))
        p.fermionMeasurements = fm
        h = C.c_void_p()
        assert lib.detsdw_create(C.byref(p), C.byref(h)) != 0, fm
    with pytest.raises(ValueError, match="equalTimeCorrelators needs fermionMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=1.0, s=5, equalTimeCorrelators=True))
