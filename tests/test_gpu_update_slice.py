"""Kernel-level test of the delayed-update slice -- k_update_decide (all launch shapes), k_update_gather, k_update_window and the
flush behind them -- against the long-double reference of tests/update_reference.py, which restates updateInSlice with an immediate
rank-MSF update per accepted proposal (no delay blocks, no W) and prescribes the acceptance pattern through the uniform stream.

A case: create the context, set a random field, build G with the context's own rebuild (and wraps / advances where k < m), read G
back -- that fp64 matrix is the reference's input, so the test isolates the slice --, run the reference to get the stream, push the
stream plus spare values that must not be consumed, call updateInSlice(k, thermalization = True, ...), compare.

Per chain: the field of slice k bit-identical (box, cdwl) or within 1e-13 relative (rotate / scale: libm against the device library,
kernels_update.hip), every other slice untouched, rng_consumed, lastAccRatio = accepted / N exactly, one sample added to the running
average, error = 0, the cosh / sinh caches within 4 ulp of the long-double values on the accepted sites and untouched elsewhere, the
schedule the row asked for, and G elementwise
    |G_dev - G_ld| <= c_slice u comp + 8 e64 + u |G_ld|.
comp = |G_in|_1 + sum_accepted |G[:,c] delta|_1 |M'^-1 (G[c,:] - E_c)|_1 is the magnitude companion, c_slice = sum_blocks 4 (K_b + 2)
with K_b = MSF x (accepted in block b) the operation count of a K_b-term complex product sum per flush (primitives.elementwise_bound;
the errors of successive flushes add) over the block structure the device uses.  e64 is the blockwise (16 x 16, max) error of the
fp64 oracle twin -- DetSDWOracle.updateInSlice_delayed on the same stream -- against the long-double result, spread over its block:
it carries what operation counts cannot, the conditioning of the M' solves and the cancellation in delta = e^{-dtau V'} e^{dtau V} - 1,
measured on the reference's own fp64 arithmetic, never on the kernel.  The factor 8 is the random-walk spread sqrt(64) between two
summation orders of the longest sum the kernel forms (MSF D = 64 terms, quad-split with DPP reductions, against numpy's order).

Every case prints `RATIO update <case> <max err/bound>`.  Largest ratio per group of the table, measured on an MI355X:
    depth 0.092   o1o3 0.053   shape 0.052   budget 0.074   pipeline 0.062   slices 0.040   options 0.044   cdw 0.034
    rotscale 0.073   batch 0.062
No group uses more than half of its bound; none uses more than a tenth: the 8 e64 term makes up 84 to 99 % of the bound (median
over the entries, on the three rows where it was looked at: depth L6 D32 none, depth L8 D32 all, o1o3 o3 L6 D16 alternate).
What the bound still sees: each of three one-line mutations of k_update_decide -- no patch-in of the just-accepted site for the last
band, the p / q tail started at i2 + 4 <= nI, no offset for the acceptance uniform behind an accepted proposal -- fails 47 to 95 of
the rows.

The table (tests/update_reference.CASES; tests/test_update_reference_cpu.py checks every row's regime on the CPU) holds the smallest
shapes at which each path exists, L <= 8."""
import numpy as np
import pytest

import update_reference as ur
from update_reference import CASES, CLD, M_SLICES, S_SLICES, DTAU

pytestmark = pytest.mark.gpu

ADAPT = {"box": ("box", "ra_samplesAdded"), "rotate": ("rotate", "rot_samplesAdded"), "scale": ("scale", "scl_samplesAdded"),
         "rotate_and_scale": ("rotate", "rot_samplesAdded")}
_done = {}           # case id -> the device's field of slice k per chain (the launch-shape pairs are compared bit for bit)


def _context(case, **over):
    from detqmc_amd import KernelContext
    kw = ur.case_params(case)
    cdw = bool(kw["cdwU"])
    # capacity of the window of pre-drawn uniforms as include/dqmc_hip.h prescribes for rotate / scale proposals: repeat x 8 (+ 2)
    window = 0 if case["proposal"] == "box" and case["repeat"] == 1 else case["repeat"] * 8 + (2 if cdw else 0)
    args = dict(m=M_SLICES, s=S_SLICES, nchains=case["nchains"], pipeline=case["pipeline"], proposalBudget=case["proposalBudget"],
                decideThreads=case["decideThreads"], rngWindowPerSite=window, r=case["r0"], **kw)
    args.update(over)
    return KernelContext(**args)


def _to_slice(ctx, k):
    """G of slice k by the context's own rebuild and sweepDown's wraps and advances (detmodel.h:1333-1399)"""
    ctx.setupUdVStorage_and_calculateGreen()
    n = ctx.n
    for kk in range(ctx.m, k, -1):
        if kk == (n - 1) * ctx.s:
            ctx.advanceDownGreen(n)
        ctx.wrapDownGreen(kk)
    assert ctx.currentTimeslice == k


def _ulps(got, ref_ld):
    ref64 = np.asarray(ref_ld).astype(np.float64)
    return np.abs(np.asarray(got).astype(ur.LD) - ref_ld).astype(np.float64) / np.spacing(np.abs(ref64))


def _run(case):
    """runs the row on the device, compares every chain with its own reference; returns the largest err / bound of G"""
    N, k, nb = case["L"] ** 2, case["k"], case["nchains"]
    box = case["proposal"] == "box"
    spare = ur.SPARE_BOX if box else ur.SPARE_WINDOW
    ctx = _context(case)
    try:
        cdw = bool(ur.case_params(case)["cdwU"])
        fields = [ur.case_fields(case, b) for b in range(nb)]
        for b in range(nb):
            ctx.select_chain(b)
            ctx.set_fields(fields[b][0])
            if cdw:
                ctx.set_cdwl(fields[b][1])
        _to_slice(ctx, k)
        refs = []
        for b in range(nb):
            ctx.select_chain(b)
            phi, cdwl = fields[b]
            G = np.array(ctx.g)
            phi_in, ch_in, sh_in = ctx.get_fields()
            assert np.array_equal(phi_in, phi)
            lat, res = ur.case_reference(case, b, phi, cdwl, G)
            pd, ad, sd, r = ur.case_step(case, b)
            st = ctx.update_state()
            st.phiDelta, st.angleDelta, st.scaleDelta = pd, ad, sd
            ctx.set_update_state(st)
            ctx.set_exchange_parameter(r)
            ctx.push_uniforms(np.concatenate([res.stream, np.full(spare, 0.5)]))
            refs.append((lat, res, G, ch_in, sh_in))
        adapt, counter = ADAPT[case["proposal"]]
        ctx.updateInSlice(k, thermalization=True, proposal=case["proposal"], adapt=adapt, repeat=case["repeat"])
        si = ctx.schedule_info()
        assert si.pipelined == (1 if case["pipeline"] == 1 else 0)
        assert si.proposal_budget == ur.default_budget(case["D"], case["proposalBudget"])
        assert (si.blocks_pipelined if case["pipeline"] == 1 else si.blocks_sequential) > 0
        assert (si.blocks_sequential if case["pipeline"] == 1 else si.blocks_pipelined) == 0
        worst = 0.0
        out = []
        for b in range(nb):
            ctx.select_chain(b)
            lat, res, G, ch_in, sh_in = refs[b]
            phi, cdwl = fields[b]
            what = f"{case['id']} chain {b}"
            st = ctx.update_state()                         # raises on error != 0
            assert st.error == 0
            assert st.rng_consumed == res.consumed, f"{what}: {st.rng_consumed} uniforms consumed, the reference drew {res.consumed}"
            assert st.rng_avail == res.consumed + spare
            assert st.lastAccRatio == res.accepted[case["repeat"] - 1] / N, what
            assert getattr(st, counter) == 1, what
            phi_out, ch_out, sh_out = ctx.get_fields()
            others = [kk for kk in range(M_SLICES + 1) if kk != k]
            assert np.array_equal(phi_out[others], phi[others]), f"{what}: a slice other than k changed"
            if box:
                assert np.array_equal(phi_out[k], res.phi_k), f"{what}: the field of slice k differs from the reference's"
            else:
                scale = np.sqrt(np.sum(res.phi_k ** 2, axis=1, keepdims=True))
                assert np.all(np.abs(phi_out[k] - res.phi_k) <= 1e-13 * scale), what
            if cdw:
                l_out = ctx.get_cdwl()
                assert np.array_equal(l_out[k], res.cdwl_k), f"{what}: the discrete field of slice k differs"
                assert np.array_equal(l_out[others][1:], cdwl[others][1:])
            touched = np.zeros(N, dtype=bool)
            for flags in res.decisions[:case["repeat"]]:
                touched |= np.array(flags, dtype=bool)
            assert np.array_equal(ch_out[others], ch_in[others]) and np.array_equal(sh_out[others], sh_in[others])
            assert np.array_equal(ch_out[k][~touched], ch_in[k][~touched]) and np.array_equal(sh_out[k][~touched], sh_in[k][~touched])
            if touched.any():
                assert np.max(_ulps(ch_out[k][touched], res.cosh_k[touched])) <= 4, what
                assert np.max(_ulps(sh_out[k][touched], res.sinh_k[touched])) <= 4, what
            twin, consumed = ur.case_twin(case, b, lat, phi, cdwl, G, res.stream)
            assert consumed == res.consumed
            bound = ur.green_bound(res, twin.g)
            err = np.abs(np.array(ctx.g).astype(CLD) - res.G).astype(np.float64)
            ratio = float(np.max(err / bound))
            worst = max(worst, ratio)
            bad = ~(err <= bound)
            assert not bad.any(), "%s: G exceeds its bound at %s (%d entries), max err/bound %.2f" \
                % (what, tuple(np.argwhere(bad)[0]), int(bad.sum()), ratio)
            out.append(phi_out[k].copy())
        _done[case["id"]] = out
        print(f"RATIO update {case['id']} {worst:.3f}")
        return worst
    finally:
        ctx.close()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_update_slice_vs_long_double(case):
    _run(case)


SHAPE_PAIRS = sorted({c["id"].replace("-nt256", "") for c in CASES if c["id"].endswith("-nt256")})


@pytest.mark.parametrize("pair", SHAPE_PAIRS)
def test_launch_shapes_agree_bit_for_bit(pair):
    """decideThreads = 256 and 512: the same field, bit for bit (the launch shape changes no result, include/dqmc_hip.h)"""
    outs = []
    for nt in (256, 512):
        cid = f"{pair}-nt{nt}"
        if cid not in _done:
            _run(next(c for c in CASES if c["id"] == cid))
        outs.append(_done[cid])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("kind,count", [("window", 32), ("guard", 200)])
def test_rng_overrun_in_box_muller_loop_is_reported(kind, count):
    """a scale proposal whose Box-Muller loop rejects pair after pair (u1 = u2 = 0.99): the check at the top of the proposal guarantees
    32 values, "window" pushes exactly that many, so the loop runs off the pushed window; "guard" pushes enough for the loop's guard of
    64 pairs to run out.  Both must be reported as DQMC_ERNG, as test_rng_window_exhaustion_is_reported pins for box proposals, and
    nothing of the proposal that ran dry may be kept: the field stays as it was.

    Before the fix the proposal went on with made-up uniforms (0.25, 0.25 -- an acceptable pair -- and 0.5 for the acceptance test)
    resp. with the logarithm of a rejected pair; the error was raised only by the check at the top of the NEXT proposal (the cursor
    had passed the end of the window by then), after the made-up proposal had been accepted into the field.  The step width is tiny
    here so that such a proposal has prob ~ 1 and would be accepted."""
    from detqmc_amd import DqmcError
    case = ur._row("overrun", 3, 4, 3, "all", proposal="scale")
    case["seed"] = 77
    ctx = _context(case)
    try:
        phi = ur.case_fields(case, 0)[0]
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        st = ctx.update_state()
        st.scaleDelta = 1e-3
        ctx.set_update_state(st)
        ctx.push_uniforms(np.full(count, 0.99))
        ctx.updateInSlice(M_SLICES, thermalization=True, proposal="scale", adapt="scale")
        with pytest.raises(DqmcError) as e:
            ctx.update_state()
        assert e.value.code == -4
        assert np.array_equal(ctx.get_fields()[0], phi), "a proposal formed from uniforms past the pushed window was accepted"
    finally:
        ctx.close()
