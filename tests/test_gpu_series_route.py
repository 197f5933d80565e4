"""The measurement series routed by slot (dqmc_series_form_sample / _sample_device / _accumulate, detsdw_series_route,
pt.replica_exchange_step(route_series=True)).

Every kernel-level expectation is tests/series_route_reference.routed_bins of the samples the DEVICE formed: a run with bin_size = 1
and the identity closes one bin per sweep, and open / 1 is exact, so its bins are the samples.  A routed bin is ((0.0 + s_1) + s_2) / 2
of two such samples -- two IEEE operations that numpy repeats in the same order -- so every comparison is np.array_equal over the whole
row of S doubles.  The host-level routed test compares the same way against an unrouted host run on the same seeds.  Only the test with
replica exchange compares device samples against the vectors the host layer formed; it uses the bound of
test_gpu_series.test_host_series_vs_recorded_vectors for that comparison, 1e-14 of the row's scale.

The fields differ per sweep and per chain, and their amplitude grows with both (0.5 + 0.5 sweep + 0.2 chain): at a fixed amplitude the
charge correlator hardly depends on the configuration, and a routing error between two such samples could hide below the rounding."""
import dataclasses
import functools

import numpy as np
import pytest

import series_reference as sr
import series_route_reference as srr

pytestmark = pytest.mark.gpu

L, N, M, S_STAB, NCH, BIN, MAXBINS, NFREQ, PARTS = 4, 16, 20, 5, 4, 2, 3, 3, 31
NSWEEPS = BIN * MAXBINS
EINVAL = -1
IDENTITY = list(range(NCH))
# chain -> slot, one per sweep: two different 4-cycles (not their own inverse: a route applied backwards is caught) with the change in
# the middle of bin 0, the identity, and three involutions of which the last sends every chain to the other half of the chains
ROUTES = ([1, 2, 3, 0], [2, 0, 3, 1], [0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2], [2, 3, 0, 1])


def _phi(sweep, chain):
    phi = np.random.default_rng(1000 * L + 10 * sweep + chain).uniform(-1.0, 1.0, (M + 1, N, 2)) * (0.5 + 0.5 * sweep + 0.2 * chain)
    phi[0] = 0.0
    return phi


def _context(nchains):
    from detqmc_amd import KernelContext
    return KernelContext(2, L, M, S_STAB, 0.1, delaySteps=4, stabilisation="qr", nchains=nchains, timeDisplaced=2, tdParticleHole=True,
                         tdCurrent=True, tdEverySlice=True)


def _fill(ctx, phis):
    """new fields, then one down pass without updates that refills every block (tests/test_gpu_series.py)"""
    m, s, n = ctx.m, ctx.s, ctx.n
    for b, phi in enumerate(phis):
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.select_chain(0)
    ctx.setupUdVStorage_and_calculateGreen()
    ctx.set_timedisplaced(True)
    ctx.set_equal_time_correlators(True)
    ctx.measure_reset()
    for k in range(m, (n - 1) * s, -1):
        ctx.measure_slice()
        ctx.wrapDownGreen(k)
    ctx.set_equal_time_correlators(False)
    for l in range(n - 1, 0, -1):
        ctx.advanceDownGreen(l + 1)
        ctx.measure_timedisplaced_segment(l)
        for k in range(l * s, (l - 1) * s, -1):
            ctx.wrapDownGreen(k)
    ctx.advanceDownGreen(1)
    ctx.measure_timedisplaced_ends()


def _blocks(ctx, nchains):
    out = []
    for b in range(nchains):
        ctx.select_chain(b)
        out.append((ctx.measure_eq_read(), [ctx.measure_td_fine_read(ch) for ch in range(4)], ctx.g))
    ctx.select_chain(0)
    return out


def _same_blocks(x, y):
    return all(np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
               for a, b in zip(x, y))


def _all_bins(ctx, nchains):
    """[slot][bin][S]"""
    out = []
    for b in range(nchains):
        ctx.select_chain(b)
        out.append(ctx.series_bins())
    ctx.select_chain(0)
    return np.array(out)


def _raises(fn, code=EINVAL):
    from detqmc_amd import DqmcError
    with pytest.raises(DqmcError) as e:
        fn()
    assert e.value.code == code
    return True


def _rows_of(ctx, nchains):
    """device address of every chain's sample row"""
    ptr, S = ctx.series_sample_device()
    return [ptr + 8 * b * S for b in range(nchains)]


def _table(rows_by_chain, route):
    """source row of every slot: the row of the chain the route sends there"""
    src = [None] * len(route)
    for c, s in enumerate(route):
        src[s] = rows_by_chain[c]
    return src


@functools.lru_cache(maxsize=None)
def _samples():
    """[sweep][chain][S]: the device's own samples, as the bins of a series with bin_size = 1 and the identity"""
    ctx = _context(NCH)
    try:
        _fill(ctx, [_phi(0, c) for c in range(NCH)])
        ctx.series_begin(1, NSWEEPS, NFREQ, PARTS)
        for i in range(NSWEEPS):
            if i:
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
            ctx.series_add_sweep()
        S = ctx.series_info()[2]
        assert ctx.series_info() == (NSWEEPS, 0, S)
        bins = _all_bins(ctx, NCH)                           # [chain][sweep][S]
        layout = [ctx.series_layout(p) for p in range(5)]
        ctx.series_end()
    finally:
        ctx.close()
    smp = np.ascontiguousarray(bins.transpose(1, 0, 2))
    smp.setflags(write=False)
    return smp, layout


def _rows(layout):
    rows = [(x * N, N) for x in range(10)]
    for ch in range(4):
        off, ln = layout[1 + ch]
        rows += [(off + r * 2 * N, 2 * N) for r in range(ln // (2 * N))]
    return rows


@functools.lru_cache(maxsize=None)
def _routed_one_context():
    ctx = _context(NCH)
    try:
        _fill(ctx, [_phi(0, c) for c in range(NCH)])
        ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS)
        S = ctx.series_info()[2]
        rows = _rows_of(ctx, NCH)
        for i in range(NSWEEPS):
            if i:
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
            ctx.series_form_sample()
            assert ctx.series_info() == (i // BIN, i % BIN, S)          # forming moves no counter
            assert _rows_of(ctx, NCH) == rows                              # the address holds from begin to end
            ctx.series_accumulate(_table(rows, ROUTES[i]))
            assert ctx.series_info() == ((i + 1) // BIN, (i + 1) % BIN, S)
        rec = dict(bins=_all_bins(ctx, NCH), stats=ctx.series_stats(), derived=ctx.series_derived())
        ctx.series_end()
    finally:
        ctx.close()
    return rec


def test_routed_bins_one_context():
    smp, layout = _samples()
    rec = _routed_one_context()
    want = srr.routed_bins(smp, ROUTES, BIN)
    plain = srr.routed_bins(smp, [IDENTITY] * NSWEEPS, BIN)
    assert rec["bins"].shape == want.shape == (NCH, MAXBINS, smp.shape[2])
    for s in range(NCH):
        assert np.array_equal(rec["bins"][s], want[s]), s
    # the expectation is not the unrouted one: per slot and row, the largest difference over the bins against the row's scale
    least = np.inf
    for s in range(NCH):
        for off, ln in _rows(layout):
            sl = slice(off, off + ln)
            least = min(least, np.abs(want[s][:, sl] - plain[s][:, sl]).max() / np.abs(want[s][:, sl]).max())
    print(f"routed against unrouted bins: at least {least:.2e} of the row's scale in every row of every slot (must exceed 1e-3)")
    assert least > 1e-3


def test_routed_statistics_equal_a_single_chain_fed_the_slots_samples():
    rec = _routed_one_context()
    for s in range(NCH):
        ctx = _context(1)
        try:
            for i in range(NSWEEPS):
                _fill(ctx, [_phi(i, ROUTES[i].index(s))])    # the chain whose sample the route sent to slot s in sweep i
                if not i:
                    ctx.series_begin(BIN, MAXBINS, NFREQ, PARTS)
                ctx.series_add_sweep()
            assert np.array_equal(ctx.series_bins(), rec["bins"][s]), s
            stats, derived = ctx.series_stats(), ctx.series_derived()
            for k in (0, 1):
                assert np.array_equal(stats[k][0], rec["stats"][k][s]), (s, k)
                assert np.array_equal(derived[k][0], rec["derived"][k][s], equal_nan=True), (s, k)
            assert np.isfinite(derived[0]).all() and (stats[1] > 0).any()
        finally:
            ctx.close()


def test_routed_bins_across_two_contexts():
    one = _routed_one_context()
    half = NCH // 2
    A, B = _context(half), _context(half)
    try:
        for i in range(NSWEEPS):
            _fill(A, [_phi(i, c) for c in range(half)])
            _fill(B, [_phi(i, c) for c in range(half, NCH)])
            if not i:
                A.series_begin(BIN, MAXBINS, NFREQ, PARTS)
                B.series_begin(BIN, MAXBINS, NFREQ, PARTS)
            A.series_form_sample()
            B.series_form_sample()
            src = _table(_rows_of(A, half) + _rows_of(B, half), ROUTES[i])
            A.series_accumulate(src[:half])
            B.series_accumulate(src[half:])
        got = np.concatenate([_all_bins(A, half), _all_bins(B, half)])
        for s in range(NCH):
            assert np.array_equal(got[s], one["bins"][s]), s
    finally:
        A.close()
        B.close()


def test_identity_gives_the_bits_of_add_sweep_and_reads_the_blocks_only():
    recs = []
    for variant in ("add_sweep", "none", "own_rows"):
        ctx = _context(NCH)
        try:
            info = []
            for i in range(2 * BIN):
                _fill(ctx, [_phi(i, c) for c in range(NCH)])
                if not i:
                    ctx.series_begin(BIN, 2, NFREQ, PARTS)
                before = _blocks(ctx, NCH)
                if variant == "add_sweep":
                    ctx.series_add_sweep()
                else:
                    ctx.series_form_sample()
                    ctx.series_accumulate(None if variant == "none" else _rows_of(ctx, NCH))
                assert _same_blocks(before, _blocks(ctx, NCH)), (variant, i)
                info.append(ctx.series_info())
            recs.append((info, _all_bins(ctx, NCH)))
        finally:
            ctx.close()
    smp, _ = _samples()
    assert np.array_equal(recs[0][1], srr.routed_bins(smp[:2 * BIN], [IDENTITY] * (2 * BIN), BIN))
    for info, bins in recs[1:]:
        assert info == recs[0][0] and np.array_equal(bins, recs[0][1])


def test_error_paths_leave_the_series_as_it_was():
    ctx = _context(NCH)
    try:
        for fn in (ctx.series_form_sample, ctx.series_sample_device, ctx.series_accumulate, lambda: ctx.series_accumulate([1] * NCH)):
            _raises(fn)                                      # no series open
        _fill(ctx, [_phi(0, c) for c in range(NCH)])
        ctx.series_begin(1, 3, NFREQ, PARTS)
        S = ctx.series_info()[2]
        rows = _rows_of(ctx, NCH)
        ctx.series_add_sweep()
        state = (ctx.series_info(), _all_bins(ctx, NCH))
        assert state[0] == (1, 0, S)

        def unchanged():
            return ctx.series_info() == state[0] and np.array_equal(_all_bins(ctx, NCH), state[1])

        _raises(ctx.series_accumulate)                       # add_sweep has consumed its sample: nothing is formed
        _raises(lambda: ctx.series_accumulate(rows))
        assert unchanged()
        ctx.measure_reset()                                  # empty blocks: no sample can be formed ...
        _raises(ctx.series_form_sample)
        _raises(ctx.series_accumulate)                       # ... and a failed form_sample leaves none behind
        assert unchanged()
        _fill(ctx, [_phi(1, c) for c in range(NCH)])
        ctx.series_form_sample()
        ctx.series_form_sample()                             # forms the same sample again
        assert unchanged()
        _raises(lambda: ctx.series_accumulate(rows[:2] + [None] + rows[3:]))      # a null entry
        host = np.zeros(S)                                   # a host address: refused by the pointer check, nothing is launched with it
        _raises(lambda: ctx.series_accumulate(rows[:3] + [host.ctypes.data]))
        assert unchanged()
        with pytest.raises(ValueError):
            ctx.series_accumulate(rows[:2])
        ctx.series_accumulate(rows)                          # the sample is still formed after the refusals
        assert ctx.series_info() == (2, 0, S)
        first = state[1]
        state = (ctx.series_info(), _all_bins(ctx, NCH))
        assert np.array_equal(state[1][:, :1], first)        # the closed bin stayed, the new one is the second fill's sample
        assert np.array_equal(state[1][:, 1], _samples()[0][1])
        _raises(ctx.series_accumulate)                       # twice after one form_sample
        _raises(lambda: ctx.series_accumulate(rows))
        assert unchanged()
        ctx.series_form_sample()
        ctx.series_accumulate()
        state = (ctx.series_info(), _all_bins(ctx, NCH))
        assert state[0] == (3, 0, S)
        _raises(ctx.series_form_sample)                      # the series is full
        _raises(ctx.series_add_sweep)
        assert unchanged()
        assert np.array_equal(state[1][:, 1], state[1][:, 2])      # the same blocks formed again: the same sample
        ctx.series_end()
        for fn in (ctx.series_form_sample, ctx.series_sample_device, ctx.series_accumulate):
            _raises(fn)
    finally:
        ctx.close()


# ---- host level ----------------------------------------------------------------------------------------------------------------------
H_NFREQ = 2
H_NAMES = ("sdwCorr", "sdwSq", "sdwTau", "currentXTau", "currentYTau")
H_R = (-1.0, -0.9, -0.8, -0.7)


def _host_params(rvals):
    from detqmc_amd import SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, updateMethod="delayed", stabilisation="qr", fermionMeasurements=True,
                  equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                  timeDisplacedCurrent=True, timeDisplacedEverySlice=True, rngSeed=4711)
    return [dataclasses.replace(p, simindex=b, r=r) for b, r in enumerate(rvals)]


def _f64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


def _host_bins(batch, nbins):
    """{name: [slot][bin][len]}"""
    return {nm: np.array([_f64(batch.chain(b).series_bins(nm)).reshape(nbins, -1) for b in range(NCH)]) for nm in H_NAMES}


@functools.lru_cache(maxsize=None)
def _host_run(sub_batches, mode):
    """mode: 'plain' (no series), 'samples' (bin size 1, no route), 'routed' (bin size BIN, a new route before every measurement sweep)"""
    from detqmc_amd import DetSDWBatch, DqmcError
    batch = DetSDWBatch(_host_params(H_R), sub_batches=sub_batches)
    rec = {}
    try:
        assert batch.sub_batches == sub_batches
        batch.sweepThermalization()
        if mode == "routed":
            with pytest.raises(DqmcError):
                batch.series_route(IDENTITY)                 # no series is open
            with pytest.raises(DqmcError):
                batch.series_route()
        if mode == "samples":
            batch.series_begin(1, NSWEEPS, H_NFREQ)
        elif mode == "routed":
            batch.series_begin(BIN, MAXBINS, H_NFREQ)
            assert batch.series_route() == IDENTITY
        for i in range(NSWEEPS):
            batch.sweepThermalization()
            if i % 2:
                batch.sweep(False)
            if mode == "routed":
                batch.series_route(ROUTES[i])
                assert batch.series_route() == ROUTES[i]
                for bad in ([0, 1, 2, 2], [0, 1, 2, 4], [-1, 0, 1, 2]):
                    with pytest.raises(DqmcError, match="permutation"):
                        batch.series_route(bad)
                with pytest.raises(ValueError):
                    batch.series_route([0, 1, 2])
                assert batch.series_route() == ROUTES[i]     # a refused route changes nothing
            batch.sweep(True)
        rec["phi"] = [batch.chain(b).phi for b in range(NCH)]
        rec["rng"] = [batch.chain(b).info.rngDrawn for b in range(NCH)]
        if mode != "plain":
            rec["bins"] = _host_bins(batch, NSWEEPS if mode == "samples" else MAXBINS)
            batch.series_end()
        if mode == "routed":
            batch.series_begin(BIN, MAXBINS, H_NFREQ)        # a new series starts from the identity
            assert batch.series_route() == IDENTITY
            batch.series_end()
    finally:
        batch.close()
    return rec


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_host_routed_series(sub_batches):
    plain, samples, routed = (_host_run(sub_batches, mode) for mode in ("plain", "samples", "routed"))
    for other in (samples, routed):
        assert other["rng"] == plain["rng"]
        assert all(np.array_equal(a, b) for a, b in zip(other["phi"], plain["phi"]))
    for nm in H_NAMES:
        smp = samples["bins"][nm].transpose(1, 0, 2)         # [sweep][chain][len]
        want = srr.routed_bins(smp, ROUTES, BIN)
        plain_bins = srr.routed_bins(smp, [IDENTITY] * NSWEEPS, BIN)
        assert np.abs(want).max() > 0
        for s in range(NCH):
            assert np.array_equal(routed["bins"][nm][s], want[s]), (nm, s)
            assert not np.array_equal(want[s], plain_bins[s]), (nm, s)


def test_host_routed_series_does_not_depend_on_the_grouping():
    one, two = _host_run(1, "routed"), _host_run(2, "routed")
    for nm in H_NAMES:
        assert np.array_equal(one["bins"][nm], two["bins"][nm]), nm


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_series_routed_by_replica_exchange(sub_batches):
    from detqmc_amd import DetSDWBatch, pt
    rvals = [-1.0, -1.0, -0.8, -0.8]          # equal neighbours: delta = 0, probability exactly 1, the swaps 0 <-> 1 and 2 <-> 3 need no draw
    batch = DetSDWBatch(_host_params(rvals), sub_batches=sub_batches)
    try:
        state = pt.ExchangeState.create(rvals, 0, 1, n_local=NCH)
        reps = [pt.ReplicaAdapter(batch.chain(b)) for b in range(NCH)]
        batch.sweepThermalization()
        batch.series_begin(BIN, MAXBINS, H_NFREQ, host_copy=True)
        vec = {nm: [] for nm in H_NAMES}
        held = []
        for i in range(NSWEEPS):
            batch.sweepThermalization()
            held.append(list(state.local_parameter_indices))           # the parameter index every chain measures under
            assert batch.series_route() == held[-1]
            batch.sweep(True)
            for nm in H_NAMES[:2]:
                vec[nm].append([batch.chain(b).observable_vector(nm) for b in range(NCH)])
            for nm in H_NAMES[2:]:
                vec[nm].append(batch.matsubara_all(nm, H_NFREQ))
            new = pt.replica_exchange_step(reps, state, None, route_series=True)
            assert new == state.local_parameter_indices and batch.series_route() == new
            assert [batch.chain(b).get_exchange_parameter_value() for b in range(NCH)] == [rvals[k] for k in new]
        assert state.par_swapUpAccepted[0] == NSWEEPS and state.par_swapUpAccepted[2] == NSWEEPS
        assert sum(state.par_swapUpAccepted) >= 1 and any(h != IDENTITY for h in held)
        bins = _host_bins(batch, MAXBINS)
        for nm in H_NAMES:
            per_sweep = np.array([[_f64(np.asarray(v[b])).ravel() for b in range(NCH)] for v in vec[nm]])     # [sweep][chain][len]
            want = srr.routed_bins(per_sweep, held, BIN)
            rowlen = 16 if nm in H_NAMES[:2] else 32
            for s in range(NCH):
                fig = sr.rows_close(bins[nm][s], want[s], 1e-14, rowlen)
                print(f"sub_batches={sub_batches} {nm} slot {s}: bins against the routed host vectors {fig:.2e} of the row's scale (bound 1e-14)")
        batch.series_end()
        # without an open series the switch changes nothing; all parameters equal: every swap is certain, no draw decides
        out = []
        for flag in (False, True):
            st = pt.ExchangeState.create([-1.0] * NCH, 0, 1, n_local=NCH)
            out.append((pt.replica_exchange_step(reps, st, None, route_series=flag), list(st.par_swapUpAccepted)))
        assert out[0] == out[1] and out[0][1][:NCH - 1] == [1] * (NCH - 1)
    finally:
        batch.close()


def test_route_series_across_ranks_is_refused_before_any_collective():
    from detqmc_amd import DetSDWBatch, pt

    class TwoRanks:
        def get_rank(self):
            return 0

        def get_world_size(self):
            return 2

        def all_gather(self, *a):
            raise AssertionError("collective reached")

        broadcast = all_gather

    rvals = [-1.0, -1.0, -0.8, -0.8]
    batch = DetSDWBatch(_host_params(rvals[:2]), sub_batches=1)
    try:
        batch.series_begin(BIN, MAXBINS, H_NFREQ)
        reps = [pt.ReplicaAdapter(batch.chain(b)) for b in range(2)]
        with pytest.raises(ValueError, match="route_series"):
            pt.replica_exchange_step(reps, pt.ExchangeState.create(rvals, 0, 2, n_local=2), TwoRanks(), route_series=True)
        assert batch.series_route() == [0, 1]
    finally:
        batch.close()
