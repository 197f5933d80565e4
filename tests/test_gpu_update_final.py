"""dqmc_update_slice_final: the update of the last slice of a segment.  The dqmc_advance that follows rebuilds G from the UdV factors,
so the delayed-update block in which a chain finishes that slice is decided but neither gathered nor flushed, and G is stale until the
advance.  Everything except G must be what dqmc_update_slice_ex (+ dqmc_wrap_skip in a down sweep) leaves, bit for bit: fields, cosh /
sinh tables, every byte of the update state, currentTimeslice -- and after the advance G and its singular values as well.

L = 4 (N = 16), delaySteps = 4 without a proposal budget: a slice takes up to four decision rounds and the three chains of a context,
each with a field and uniforms of its own, finish in different ones."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, M, S, D, NCH = 4, 20, 5, 4, 3
N = L * L
NSEG = M // S
VARIANTS = {
    "o2": dict(opdim=2),
    "o3": dict(opdim=3),
    "o2-repeat2": dict(opdim=2, repeat=2),
    "o2-cdw": dict(opdim=2, cdwU=0.7),
}


def _make(seed, opdim=2, repeat=1, cdwU=0.0, **over):
    """one context at slice m with G(beta) built; per chain a field and a window of uniforms that lasts a whole sweep"""
    from detqmc_amd import KernelContext
    per_site = (opdim + 1) * repeat + (2 if cdwU else 0)
    ctx = KernelContext(opdim, L, M, S, 0.1, delaySteps=D, stabilisation="qr", nchains=NCH, cdwU=cdwU, rngWindowPerSite=per_site, **over)
    for b in range(NCH):
        rng = np.random.default_rng(seed + b)
        phi = rng.uniform(-0.9, 0.9, (M + 1, N, opdim))
        phi[0] = 0.0
        ctx.select_chain(b)
        ctx.set_fields(phi)
        if cdwU:
            ctx.set_cdwl(rng.choice([-2, -1, 1, 2], (M + 1, N)).astype(np.int32))
        ctx.push_uniforms(rng.random(per_site * N * M))
    ctx.setupUdVStorage_and_calculateGreen()
    return ctx


def _state(ctx, cdw, with_g):
    """everything the update leaves behind, per chain"""
    out = []
    for b in range(NCH):
        ctx.select_chain(b)
        phi, ch, sh = ctx.get_fields()
        item = [phi, ch, sh, np.frombuffer(bytes(ctx.update_state()), dtype=np.uint8)]
        if cdw:
            item.append(ctx.get_cdwl())
        if with_g:
            item += [ctx.g, ctx.g_inv_sv]
        out.append(item)
    return out


def _assert_same(a, b, what):
    for ch, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for i, (u, v) in enumerate(zip(x, y)):
            assert np.array_equal(u, v), f"{what}: chain {ch}, item {i} differs"


def _stale(ctx):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        ctx.g
    assert e.value.code == -1 and "stale" in str(e.value)


def _down_sweep_old(ctx, rep):
    """a whole down sweep through the entries of before: update + wrap, the last wrap of a segment skipped, then the advance"""
    from detqmc_amd.model import DOWN
    for l in range(NSEG, 0, -1):
        for k in range(l * S, (l - 1) * S, -1):
            ctx.updateInSlice(k, thermalization=True, repeat=rep)
            if k > (l - 1) * S + 1:
                ctx.wrapDownGreen(k)
            else:
                ctx.wrapSkip(DOWN, k)
        ctx.advanceDownGreen(l)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_down_sweep_segment_end(name):
    from detqmc_amd import DqmcError
    from detqmc_amd.model import DOWN
    kw = VARIANTS[name]
    rep, cdw = kw.get("repeat", 1), bool(kw.get("cdwU", 0.0))
    old, new = _make(11, **kw), _make(11, **kw)
    try:
        last = (NSEG - 1) * S + 1
        for k in range(M, last, -1):
            for c in (old, new):
                c.updateInSlice(k, thermalization=True, repeat=rep)
                c.wrapDownGreen(k)
        _assert_same(_state(new, cdw, True), _state(old, cdw, True), "before the segment end")
        # refused calls move nothing
        before = _state(new, cdw, True)
        with pytest.raises(DqmcError):
            new.updateInSliceFinal(last + 1, thermalization=True, repeat=rep, thenWrap=DOWN)     # k != currentTimeslice
        with pytest.raises(DqmcError):
            new.updateInSliceFinal(last, thermalization=True, repeat=rep, thenWrap=7)            # unknown direction
        assert new.currentTimeslice == last
        _assert_same(_state(new, cdw, True), before, "after refused calls")
        old.updateInSlice(last, thermalization=True, repeat=rep)
        old.wrapSkip(DOWN, last)
        new.updateInSliceFinal(last, thermalization=True, repeat=rep, thenWrap=DOWN)
        assert new.currentTimeslice == old.currentTimeslice == last - 1
        _stale(new)
        _assert_same(_state(new, cdw, False), _state(old, cdw, False), "after the last slice of the segment")
        old.advanceDownGreen(NSEG)
        new.advanceDownGreen(NSEG)
        _assert_same(_state(new, cdw, True), _state(old, cdw, True), "after the advance")
    finally:
        old.close()
        new.close()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_up_sweep_segment_end(name):
    kw = VARIANTS[name]
    rep, cdw = kw.get("repeat", 1), bool(kw.get("cdwU", 0.0))
    per_site = (kw["opdim"] + 1) * rep + (2 if cdw else 0)
    old, new = _make(23, **kw), _make(23, **kw)
    try:
        for c in (old, new):
            _down_sweep_old(c, rep)
            for b in range(NCH):                             # a fresh window for the up sweep
                c.select_chain(b)
                c.push_uniforms(np.random.default_rng(500 + b).random(per_site * N * M))
            c.reset_storage0()
            assert c.currentTimeslice == 0
        for k in range(1, S + 1):
            for c in (old, new):
                c.wrapUpGreen(k - 1)
                if k == S and c is new:
                    c.updateInSliceFinal(k, thermalization=True, repeat=rep)
                else:
                    c.updateInSlice(k, thermalization=True, repeat=rep)
        assert new.currentTimeslice == old.currentTimeslice == S
        _stale(new)
        _assert_same(_state(new, cdw, False), _state(old, cdw, False), "after the last slice of the segment")
        old.advanceUpGreen(0)
        new.advanceUpGreen(0)
        _assert_same(_state(new, cdw, True), _state(old, cdw, True), "after the advance")
    finally:
        old.close()
        new.close()


def test_pipelined_schedule_keeps_the_flush_and_wraps():
    """pipeline = 1 (needs a proposal budget): nothing is skipped -- the entry is update + plain wrap, G stays fresh"""
    from detqmc_amd.model import DOWN
    old, new = _make(31, pipeline=1, proposalBudget=8), _make(31, pipeline=1, proposalBudget=8)
    try:
        assert old.schedule_info().pipelined == 1 and new.schedule_info().pipelined == 1
        old.updateInSlice(M, thermalization=True)
        old.wrapDownGreen(M)
        new.updateInSliceFinal(M, thermalization=True, thenWrap=DOWN)
        assert new.currentTimeslice == old.currentTimeslice == M - 1
        _assert_same(_state(new, False, True), _state(old, False, True), "pipelined")
        old.updateInSlice(M - 1, thermalization=True)
        new.updateInSliceFinal(M - 1, thermalization=True)                  # no wrap asked for: the slice stays
        assert new.currentTimeslice == old.currentTimeslice == M - 1
        _assert_same(_state(new, False, True), _state(old, False, True), "pipelined, no wrap")
    finally:
        old.close()
        new.close()


# ------------------------------------------------------------------------------------------------------------------------------
# whole sweeps through the host layer against a twin driven slice by slice through the entries of before
# ------------------------------------------------------------------------------------------------------------------------------
def _batches(**over):
    from detqmc_amd import DetSDWBatch, SDWParams
    p0 = SDWParams(opdim=2, L=L, m=M, s=S, dtau=0.1, delaySteps=D, stabilisation="qr", pipeline=-1, **over)      # no global moves by default
    pars = [dataclasses.replace(p0, simindex=b, r=-1.0 + 0.1 * b) for b in range(NCH)]
    return DetSDWBatch(pars, sub_batches=1), DetSDWBatch(pars, sub_batches=1), pars


def _windows(pars):
    """the dSFMT stream of every chain behind the draws of its random field, long enough for two sweeps"""
    from dsfmt_oracle import RngWrapper
    out = []
    for p in pars:
        r = RngWrapper(p.rngSeed, p.simindex + 1)
        for _ in range(3 * N * M):
            r.rand01()
        out.append(np.array([r.rand01() for _ in range(2 * 3 * N * M)]))
    return out


def _twin_sweep(ctx, streams, pos, down, measure):
    """what DetSDW::sweepDown / sweepUp did before dqmc_update_slice_final: returns the new stream positions"""
    from detqmc_amd.model import DOWN
    for b in range(NCH):
        ctx.select_chain(b)
        ctx.push_uniforms(streams[b][pos[b]:pos[b] + 3 * N * M])

    def update(k):
        ctx.updateInSlice(k, thermalization=not measure)
        if measure:
            ctx.measure_slice()

    if down:
        for l in range(NSEG, 0, -1):
            if l < NSEG:
                ctx.advanceDownGreen(l + 1)
            for k in range(l * S, (l - 1) * S, -1):
                update(k)
                if k > (l - 1) * S + 1:
                    ctx.wrapDownGreen(k)
                else:
                    ctx.wrapSkip(DOWN, k)
        ctx.advanceDownGreen(1)
    else:
        ctx.reset_storage0()
        for l in range(NSEG):
            for k in range(l * S + 1, (l + 1) * S + 1):
                ctx.wrapUpGreen(k - 1)
                update(k)
            ctx.advanceUpGreen(l)
    new = []
    for b in range(NCH):
        ctx.select_chain(b)
        new.append(pos[b] + int(ctx.update_state().rng_consumed))
    return new


def _chain_state(ctx):
    out = []
    for b in range(NCH):
        ctx.select_chain(b)
        st = ctx.update_state()
        out.append([ctx.get_fields()[0], ctx.g, ctx.g_inv_sv, np.array([st.lastAccRatio, st.phiDelta]), np.array([st.rng_consumed])])
    return out


def test_thermalization_sweeps_walk_the_chain_of_the_old_entries():
    host, twin, pars = _batches()
    try:
        streams = _windows(pars)
        tctx = twin.kernel_context
        pos = [0] * NCH
        for down in (True, False):
            host.sweepThermalization()
            pos = _twin_sweep(tctx, streams, pos, down, measure=False)
            _assert_same(_chain_state(host.kernel_context), _chain_state(tctx), "down sweep" if down else "up sweep")
            for b in range(NCH):
                assert host.chain(b).info.lastAccRatioLocal_phi == _chain_state(tctx)[b][3][0]
    finally:
        host.close()
        twin.close()


def test_measured_sweep_does_not_skip():
    """sweep(True) with fermionMeasurements: measure(k) reads G right after the update of every slice, the segment ends included, so
    the plain entries stay -- the equal-time accumulators are those of the twin that measures after every old-style update"""
    host, twin, pars = _batches(fermionMeasurements=True)
    try:
        streams = _windows(pars)
        tctx = twin.kernel_context
        tctx.measure_reset()
        host.sweep(True)
        _twin_sweep(tctx, streams, [0] * NCH, True, measure=True)
        _assert_same(_chain_state(host.kernel_context), _chain_state(tctx), "measured down sweep")
        hctx = host.kernel_context
        for b in range(NCH):
            hctx.select_chain(b)
            tctx.select_chain(b)
            a, w = hctx.measure_read(), tctx.measure_read()
            assert a[3] == M and np.array_equal(a, w), f"chain {b}: equal-time accumulators differ"
    finally:
        host.close()
        twin.close()
