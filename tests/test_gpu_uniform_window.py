"""The splice kernel of the look-ahead on the uniforms (k_advance_uniforms) through its two entry points and a read-back of the
window: dqmc_stage_uniforms_tail_host uploads the draws behind the current window of every chain, dqmc_advance_uniforms builds the
next window on the device from the rest of the current one and that tail.  Pure copies of doubles: the result must EQUAL numpy
slicing of the known stream, for per-chain offsets at both ends of the range and in between, twice in a row so that both window
buffers take both roles, and a third time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH, NEED = 3, 40
OFFSETS = [(0, 1, 17), (39, 40, 40), (40, 0, 23)]


@pytest.fixture(scope="module")
def streams():
    return np.random.default_rng(20261020).random((NCH, 8 * NEED))


def _context(**kw):
    from detqmc_amd.model import KernelContext
    # window capacity = rng_window_per_site * N * m + 64 = 112 >= NEED
    return KernelContext(opdim=2, L=4, m=3, s=2, dtau=0.1, delaySteps=4, stabilisation="qr", nchains=NCH, rngWindowPerSite=1, **kw)


def _windows(ctx):
    out = []
    for b in range(NCH):
        ctx.select_chain(b)
        out.append(ctx.uniform_window(NEED))
    return np.array(out)


def test_splice_equals_slicing(streams):
    ctx = _context()
    try:
        start = np.zeros(NCH, dtype=np.int64)
        ctx.push_uniforms_all(streams[:, :NEED])
        assert np.array_equal(_windows(ctx), streams[:, :NEED])
        for step, offs in enumerate(OFFSETS):
            tail = np.array([streams[b, start[b] + NEED:start[b] + 2 * NEED] for b in range(NCH)])
            ctx.stage_uniforms_tail(tail)
            ctx.advance_uniforms(offs)
            start += np.array(offs)
            want = np.array([streams[b, start[b]:start[b] + NEED] for b in range(NCH)])
            assert np.array_equal(_windows(ctx), want), f"advance {step}, offsets {offs}"
            for b, st in enumerate(ctx.update_states_all()):
                assert (st.rng_consumed, st.rng_avail, st.error) == (0, NEED, 0), (step, b)
        si = ctx.schedule_info()
        assert (si.uniform_windows_advanced, si.uniform_windows_pushed) == (len(OFFSETS), 1)
    finally:
        ctx.close()


def test_cursor_fields_are_reset(streams):
    """a used-up window with the error flag set: the advance puts the three fields back whatever they held"""
    ctx = _context()
    try:
        ctx.push_uniforms_all(streams[:, :NEED])
        for b in range(NCH):
            ctx.select_chain(b)
            st = ctx.update_state()
            st.rng_consumed, st.rng_avail, st.error = 7 + b, 5, -4
            ctx.set_update_state(st)
        ctx.stage_uniforms_tail(streams[:, NEED:2 * NEED])
        ctx.advance_uniforms((7, 8, 9))
        for b, st in enumerate(ctx.update_states_all()):
            assert (st.rng_consumed, st.rng_avail, st.error) == (0, NEED, 0), b
        assert np.array_equal(_windows(ctx), np.array([streams[b, 7 + b:7 + b + NEED] for b in range(NCH)]))
    finally:
        ctx.close()


def test_refusals_launch_nothing(streams):
    from detqmc_amd._lib import DqmcError as KernelError
    ctx = _context()
    try:
        ctx.push_uniforms_all(streams[:, :NEED])

        def refused(fn, word):
            with pytest.raises(KernelError) as e:
                fn()
            assert e.value.code == -1 and word in str(e.value)

        refused(lambda: ctx.advance_uniforms((0, 0, 0)), "no tail")                       # nothing staged yet
        refused(lambda: ctx.stage_uniforms_tail(streams[:, :NEED - 1]), "size")           # not the window's size
        ctx.stage_uniforms_tail(streams[:, NEED:2 * NEED])
        refused(lambda: ctx.advance_uniforms((0, NEED + 1, 0)), "offset")                 # past the end of the window
        assert np.array_equal(_windows(ctx), streams[:, :NEED])
        for st in ctx.update_states_all():
            assert (st.rng_consumed, st.rng_avail, st.error) == (0, NEED, 0)
        assert ctx.schedule_info().uniform_windows_advanced == 0
        ctx.advance_uniforms((0, NEED, 0))                                                # the staged tail is still good
        assert np.array_equal(_windows(ctx)[1], streams[1, NEED:2 * NEED])
        refused(lambda: ctx.advance_uniforms((0, 0, 0)), "no tail")                       # ... and used up now
        ctx.push_uniforms_all(streams[:, :NEED])
        ctx.stage_uniforms_tail(streams[:, NEED:2 * NEED])
        ctx.push_uniforms_all(streams[:, :NEED])                                          # a push drops the staged tail
        refused(lambda: ctx.advance_uniforms((0, 0, 0)), "no tail")
    finally:
        ctx.close()
    off = _context(rngLookahead=-1)
    try:
        off.push_uniforms_all(streams[:, :NEED])
        with pytest.raises(KernelError) as e:
            off.stage_uniforms_tail(streams[:, NEED:2 * NEED])
        assert e.value.code == -1 and "look-ahead" in str(e.value)
        with pytest.raises(KernelError) as e:
            off.advance_uniforms((0, 0, 0))
        assert e.value.code == -1
        assert np.array_equal(_windows(off), streams[:, :NEED])
    finally:
        off.close()
