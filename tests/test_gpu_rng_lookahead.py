"""The look-ahead on the uniforms in the host schedule (DetSDW::beginLocalUpdates / stageLocalUpdates): the next
sweep's draws are generated and uploaded while the device sweeps and the window is spliced on the device.  The Markov chain must not
notice: with rngLookahead on and off (-1) the fields, the Green's function, the stream position, the adapted step size and the
acceptance must be the same bits after every sweep -- for box proposals, for the O(3) rotate_and_scale proposals that consume a
variable number of draws, and with the discrete cdwl field.  The counters of dqmc_get_schedule_info tell that the look-ahead really
ran: one full push per kernel context, every later window spliced."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWEEPS = 6
CASES = {
    "o2_box": dict(opdim=2),
    "o3_rotate_and_scale": dict(opdim=3, spinProposalMethod="rotate_and_scale", adaptScaleVariance=True),
    "o2_cdwU": dict(opdim=2, cdwU=0.5),
}


def _params(lookahead, **kw):
    from detqmc_amd import SDWParams
    p = SDWParams(L=4, beta=0.8, dtau=0.1, s=4, delaySteps=4, updateMethod="delayed", stabilisation="qr", rngSeed=8642,
                  rngLookahead=lookahead, **kw)
    return [dataclasses.replace(p, simindex=b, r=-1.0 + 0.1 * b) for b in range(4)]


def _snapshot(batch):
    out = []
    for b in range(len(batch)):
        c = batch.chain(b)
        i = c.info
        out.append(dict(phi=c.phi, g=c.g, rngDrawn=int(i.rngDrawn), phiDelta=i.phiDelta, acc=i.lastAccRatioLocal_phi, angleDelta=i.angleDelta,
                        scaleDelta=i.scaleDelta, shifts=(i.acceptedGlobalShifts, i.attemptedGlobalShifts), cdwl=c.cdwl))
    return out


def _same(a, b, skip=()):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in x if k not in skip)


def _sweep(batch, i):
    # the first half adapts the step sizes (phiDelta, angleDelta / scaleDelta move), the second half does not
    if i < SWEEPS // 2:
        batch.sweepThermalization()
    else:
        batch.sweep(False)


def _run(lookahead, between=None, **kw):
    """snapshots after every sweep and the (advanced, pushed) counters of every kernel context; between(batch, i) runs after sweep i"""
    from detqmc_amd import DetSDWBatch
    batch = DetSDWBatch(_params(lookahead, **kw), sub_batches=2)
    try:
        assert batch.sub_batches == 2
        snaps = []
        for i in range(SWEEPS):
            _sweep(batch, i)
            snaps.append(_snapshot(batch))
            if between:
                between(batch, i)
        si = [kc.schedule_info() for kc in batch.kernel_contexts()]
        return snaps, [(int(s.uniform_windows_advanced), int(s.uniform_windows_pushed)) for s in si]
    finally:
        batch.close()


@pytest.mark.parametrize("case", list(CASES))
def test_same_chain_with_and_without_lookahead(case):
    on, count_on = _run(0, **CASES[case])
    off, count_off = _run(-1, **CASES[case])
    for i in range(SWEEPS):
        assert _same(on[i], off[i]), f"sweep {i + 1}"
    assert on[0][0]["rngDrawn"] < on[-1][0]["rngDrawn"] and not np.array_equal(on[0][0]["phi"], on[-1][0]["phi"])
    # a build that always falls back to the full push fails here
    assert count_on == [(SWEEPS - 1, 1)] * 2
    assert count_off == [(0, SWEEPS)] * 2


def test_host_draws_between_sweeps():
    """global shift moves every second sweep (host draws at the head of a down sweep) and one draw by the caller between two sweeps:
    the offsets of the splice differ per chain and include them"""
    def between(batch, i):
        if i == 2:
            batch.chain(1).rand01()

    kw = dict(opdim=2, globalShift=True, globalUpdateInterval=2)
    on, count_on = _run(0, between, **kw)
    off, count_off = _run(-1, between, **kw)
    for i in range(SWEEPS):
        assert _same(on[i], off[i]), f"sweep {i + 1}"
    assert on[-1][0]["shifts"][1] > 0, "global moves must have been attempted"
    assert all(a + p == SWEEPS for a, p in count_on) and count_on == [(SWEEPS - 1, 1)] * 2
    assert count_off == [(0, SWEEPS)] * 2


def test_checkpoint_of_a_lookahead_run(tmp_path):
    """save_state after sweep 3 of a look-ahead run (its RNG record holds up to two windows of buffered draws), loaded into a fresh
    batch: sweeps 4 - 6 continue the uninterrupted run -- fields, stream position, step size and acceptance bit for bit.  A resumed
    replica rebuilds G(beta) from its fields and sweeps down next (the resume rule of save_state), so one thermalisation sweep goes
    first to make the sweeps before the save an even number, and G itself, recomputed from other factors, is compared between the
    resumed runs: the same bits whether the file was written and read with the look-ahead or without."""
    from detqmc_amd import DetSDWBatch

    def after(batch):
        snaps = []
        for _ in range(3):
            batch.sweep(False)
            snaps.append(_snapshot(batch))
        return snaps

    files, straight = {}, {}
    for la in (0, -1):
        files[la] = tmp_path / f"state{la}.ckpt"
        batch = DetSDWBatch(_params(la, opdim=2), sub_batches=2)
        try:
            batch.sweepThermalization()
            for _ in range(3):
                batch.sweep(False)
            batch.save_state(files[la])
            straight[la] = after(batch)
        finally:
            batch.close()
    assert all(_same(x, y) for x, y in zip(straight[0], straight[-1]))
    assert files[0].stat().st_size > files[-1].stat().st_size          # the buffered second window is in the file
    resumed = {}
    for written, read in ((0, 0), (0, -1), (-1, 0)):
        batch = DetSDWBatch(_params(read, opdim=2), sub_batches=2)
        try:
            batch.load_state(files[written])
            resumed[written, read] = after(batch)
            counts = [(int(s.uniform_windows_advanced), int(s.uniform_windows_pushed)) for s in (kc.schedule_info() for kc in batch.kernel_contexts())]
            assert counts == ([(2, 1)] * 2 if read == 0 else [(0, 3)] * 2)
        finally:
            batch.close()
    for key, snaps in resumed.items():
        for i in range(3):
            assert _same(snaps[i], straight[0][i], skip=("g",)), (key, i + 4)
            assert _same(snaps[i], resumed[0, 0][i]), (key, i + 4)
