"""Wrap-error diagnostics on the GPU (dqmc_set_green_check, include/dqmc_hip.h): the compare kernel through the test shim against the
numpy reference (tests/green_check_reference.py), the table a context fills when a sweep of wraps and advances is walked by hand, a
planted error that must come back with its place and size, and the host layer: the Markov chain must not notice the switch.

Tolerances (green_check_reference): the maxima agree to a relative 8 * 2^-53 -- device and host differ by fused against unfused
multiply-adds and one square root per modulus -- and the sum to n_g^2 * 2^-53."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import green_check_reference as ref
import primitives as P

pytestmark = pytest.mark.gpu

OUT = ("maxAbs", "argmax", "maxSiteDiag", "sumAbs", "maxFresh", "nonfinite")
CHUNK = 2048                  # entries per workgroup of the compare kernel


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel through the shim
# ------------------------------------------------------------------------------------------------------------------------------
def _prim():
    lib = P.lib()
    vp, sz, i, ll, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p
    lib.dqmc_prim_green_diff.argtypes = [vp, sz, i, sz, ll, ll, ll, ll, i, i, i, cp, i]
    return lib


def _arena(nb, n, ld):
    ar = P.Arena(nb)
    ar.mat("Gw", n, n, ld=ld)
    ar.mat("Gf", n, n, ld=ld)
    ar.vec("part", 6 * -(-n * n // CHUNK), np.float64, kind="scratch")
    ar.vec("out", 6, np.float64, kind="out")
    return ar.layout()


def _run(ar, n, ld, N):
    _prim()
    rc, msg = ar.call("dqmc_prim_green_diff", ar.off("Gw"), ar.off("Gf"), ar.off("part"), ar.off("out"), n, ld, N)
    assert rc == 0, msg
    ar.check()
    return [dict(zip(OUT, ar.get("out", b))) for b in range(ar.nb)]


def _assert_matches(got, want, n, what):
    assert got["argmax"] == want["argmax"], (what, got, want)
    assert got["nonfinite"] == want["nonfinite"], (what, got, want)
    for k in ("maxAbs", "maxSiteDiag", "maxFresh"):
        assert got[k] == want[k] or abs(got[k] - want[k]) <= ref.TOL_MAX * want[k], (what, k, got[k], want[k])     # == : +inf
    assert abs(got["sumAbs"] - want["sumAbs"]) <= ref.tol_sum(n) * want["sumAbs"], (what, got["sumAbs"], want["sumAbs"])


def _operands(seed, nb, n):
    rng = np.random.default_rng(seed)
    Gf = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(nb)]
    # |E| <= 0.71e-12 everywhere; a planted entry is 2e-12
    E = [1e-12 * (rng.uniform(-0.5, 0.5, (n, n)) + 1j * rng.uniform(-0.5, 0.5, (n, n))) for _ in range(nb)]
    return Gf, E


SHAPES = {"o2_L4": (32, 32, 16), "o2_L6_ld80": (72, 80, 36), "o3_L4": (64, 64, 16)}


def _plants(n, N, nb):
    """name -> (row, col) per chain"""
    site = 3
    fixed = {"first": (0, 0), "last": (n - 1, n - 1), "site_diagonal_off_block": (site + N, site), "off_site_diagonal": (site + 1, n - 2)}
    out = {k: [v] * nb for k, v in fixed.items()}
    out["per_chain"] = [[(5, 1), (n - 1, 0), (0, n - 1)][b] for b in range(nb)]
    return out


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_planted_entry(shape, nb):
    n, ld, N = SHAPES[shape]
    Gf, E = _operands(17, nb, n)
    for name, where in _plants(n, N, nb).items():
        ar = _arena(nb, n, ld)
        want = []
        for b, (row, col) in enumerate(where):
            Eb = E[b].copy()
            Eb[row, col] = 2e-12
            ar.set("Gf", Gf[b], b)
            ar.set("Gw", Gf[b] + Eb, b)
            want.append(ref.green_diff(Gf[b] + Eb, Gf[b], N))
            assert want[-1]["argmax"] == row + col * n and want[-1]["nonfinite"] == 0
            others = np.delete(ref.modulus((Gf[b] + Eb) - Gf[b]).flatten(order="F"), row + col * n)
            assert want[-1]["maxAbs"] >= 2 * others.max()
            on_site = row % N == col % N
            assert (want[-1]["maxSiteDiag"] == want[-1]["maxAbs"]) == on_site, name
        for b, got in enumerate(_run(ar, n, ld, N)):
            _assert_matches(got, want[b], n, (shape, name, b))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_zero_difference(shape):
    n, ld, N = SHAPES[shape]
    Gf, _ = _operands(18, 3, n)
    ar = _arena(3, n, ld)
    for b in range(3):
        ar.set("Gf", Gf[b], b)
        ar.set("Gw", Gf[b], b)
    for b, got in enumerate(_run(ar, n, ld, N)):
        assert got["maxAbs"] == 0.0 and got["argmax"] == 0.0 and got["maxSiteDiag"] == 0.0 and got["sumAbs"] == 0.0 and got["nonfinite"] == 0.0
        want = ref.green_diff(Gf[b], Gf[b], N)
        assert abs(got["maxFresh"] - want["maxFresh"]) <= ref.TOL_MAX * want["maxFresh"]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_nan_in_one_chain_and_same_bits_twice(shape):
    n, ld, N = SHAPES[shape]
    Gf, E = _operands(19, 3, n)
    ar = _arena(3, n, ld)
    Gw = [Gf[b] + E[b] for b in range(3)]
    Gw[1][n // 2, n - 3] = complex(np.nan, 0.25)
    for b in range(3):
        ar.set("Gf", Gf[b], b)
        ar.set("Gw", Gw[b], b)
    got = _run(ar, n, ld, N)
    assert got[1]["nonfinite"] == 1 and got[1]["maxAbs"] == np.inf and got[1]["argmax"] == n // 2 + (n - 3) * n
    for b in range(3):
        _assert_matches(got[b], ref.green_diff(Gw[b], Gf[b], N), n, (shape, "nan", b))
        if b != 1:
            assert got[b]["nonfinite"] == 0 and np.isfinite(got[b]["maxAbs"])
    first = ar.buf.copy()
    _run(ar, n, ld, N)
    assert np.array_equal(ar.buf, first), "two launches on the same input differ (partials or results)"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. context level: a down sweep and an up sweep of wraps and advances walked by hand, fields fixed
# ------------------------------------------------------------------------------------------------------------------------------
L, M, S = 4, 22, 5
N = L * L
NSEG = -(-M // S)             # 5; the last segment has two slices
NG = 2 * N


def _context(stab, nb):
    from detqmc_amd import KernelContext
    ctx = KernelContext(2, L, M, S, 0.1, delaySteps=4, stabilisation=stab, nchains=nb)
    for b in range(nb):
        phi = np.random.default_rng(40 + b).uniform(-0.9, 0.9, (M + 1, N, 2))
        phi[0] = 0.0
        ctx.select_chain(b)
        ctx.set_fields(phi)
    ctx.setupUdVStorage_and_calculateGreen()
    return ctx


def _greens(ctx, nb):
    out = []
    for b in range(nb):
        ctx.select_chain(b)
        out.append(ctx.g)
    return out


def _advance(ctx, nb, direction, l, j, rec):
    """one advance with G read before and after; rec[(dir, j)] = per chain (Gw, Gf, d of storage[j], sv)"""
    before = _greens(ctx, nb)
    if direction == 0:
        ctx.advanceDownGreen(l)
    else:
        ctx.advanceUpGreen(l)
    after = _greens(ctx, nb)
    item = []
    for b in range(nb):
        ctx.select_chain(b)
        item.append((before[b], after[b], ctx.udv(j)[1], ctx.g_inv_sv))
    rec[(direction, j)] = item


def _walk_down(ctx, nb, rec, upto=0):
    """sweepDown without updates; stops after the advance that lands on storage index `upto`"""
    for k in range(M, (NSEG - 1) * S, -1):
        ctx.wrapDownGreen(k)
    for l in range(NSEG - 1, 0, -1):
        _advance(ctx, nb, 0, l + 1, l, rec)
        if l == upto:
            return
        for k in range(l * S, (l - 1) * S, -1):
            ctx.wrapDownGreen(k)
    _advance(ctx, nb, 0, 1, 0, rec)


def _walk_up(ctx, nb, rec):
    ctx.reset_storage0()
    for l in range(0, NSEG - 1):
        for k in range(l * S + 1, (l + 1) * S + 1):
            ctx.wrapUpGreen(k - 1)
        _advance(ctx, nb, 1, l, l + 1, rec)
    for k in range((NSEG - 1) * S + 1, M + 1):
        ctx.wrapUpGreen(k - 1)
    _advance(ctx, nb, 1, NSEG - 1, NSEG, rec)


@functools.lru_cache(maxsize=None)
def _walk(stab, nb):
    """(rec, table after the two sweeps, table after one more advance behind a skipped wrap); computed once, shared, never modified"""
    from detqmc_amd.model import DOWN
    ctx = _context(stab, nb)
    try:
        assert ctx.lib.dqmc_green_check_size(ctx.h) == 0
        ctx.set_green_check(True)
        assert ctx.lib.dqmc_green_check_size(ctx.h) == 2 * (NSEG + 1) * 11
        assert ctx.green_check()["count"].sum() == 0                 # dqmc_udv_setup took no sample, the switch-on cleared the table
        rec = {}
        _walk_down(ctx, nb, rec)
        _walk_up(ctx, nb, rec)
        table = ctx.green_check()
        # a second down sweep begins; the last wrap of the top segment is skipped: G is stale, the advance takes no sample
        for k in range(M, (NSEG - 1) * S + 1, -1):
            ctx.wrapDownGreen(k)
        ctx.wrapSkip(DOWN, (NSEG - 1) * S + 1)
        ctx.advanceDownGreen(NSEG)
        after_skip = ctx.green_check()
        ctx.green_check_reset()
        assert ctx.green_check()["count"].sum() == 0
        return rec, table, after_skip
    finally:
        ctx.close()


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("stab", ["qr", "svd"])
def test_context_table_of_a_hand_walked_sweep(stab, nb):
    rec, t, after_skip = _walk(stab, nb)
    visited = np.zeros((2, NSEG + 1), dtype=np.int64)
    visited[0, :NSEG] = 1                                            # down: j = 0 .. n-1
    visited[1, 1:] = 1                                               # up: j = 1 .. n
    assert set(rec) == {(d, j) for d in range(2) for j in range(NSEG + 1) if visited[d, j]}
    for b in range(nb):
        assert np.array_equal(t["count"][b], visited), (b, t["count"][b])
    for (d, j), item in rec.items():
        for b, (Gw, Gf, dj, sv) in enumerate(item):
            want = ref.green_diff(Gw, Gf, N)
            what = (stab, nb, d, j, b)
            assert want["nonfinite"] == 0 and t["nonfinite"][b, d, j] == 0
            assert abs(t["lastMaxAbs"][b, d, j] - want["maxAbs"]) <= ref.TOL_MAX * want["maxAbs"], what
            assert t["maxAbs"][b, d, j] == t["lastMaxAbs"][b, d, j] == t["meanMaxAbs"][b, d, j], what          # one sample
            assert abs(t["maxSiteDiag"][b, d, j] - want["maxSiteDiag"]) <= ref.TOL_MAX * want["maxSiteDiag"], what
            mean = want["sumAbs"] / NG ** 2
            assert abs(t["meanAbs"][b, d, j] - mean) <= (ref.tol_sum(NG) + ref.U) * mean, what
            rel = want["maxAbs"] / want["maxFresh"]
            assert abs(t["maxRel"][b, d, j] - rel) <= (2 * ref.TOL_MAX + ref.U) * rel, what
            assert want["maxAbs"] > 0 and want["maxAbs"] < 1e-6, what                       # a real wrap error, and a small one
            assert abs(t["logScaleSpread"][b, d, j] - ref.log_spread(dj)) <= 1e-12, what
            if stab == "svd":
                assert abs(t["logSvSpread"][b, d, j] - (np.log(sv.max()) - np.log(sv.min()))) <= 1e-12, what
            else:
                assert t["logSvSpread"][b, d, j] == 0.0
    # the advance behind dqmc_wrap_skip: no row moved
    for k in t:
        assert np.array_equal(after_skip[k], t[k]), k


def test_readers_need_the_switch():
    from detqmc_amd import DqmcError
    ctx = _context("qr", 1)
    try:
        for call in (ctx.green_check, ctx.green_check_reset):
            with pytest.raises(DqmcError) as e:
                call()
            assert e.value.code == -1
        ctx.set_green_check(True)
        ctx.set_green_check(True)                                    # a repeated call changes nothing
        ctx.green_check_reset()
        ctx.set_green_check(False)
        assert ctx.lib.dqmc_green_check_size(ctx.h) == 0
        with pytest.raises(DqmcError):
            ctx.green_check()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. a planted error comes back with its place and its size
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stab", ["qr", "svd"])
def test_planted_error_at_a_boundary(stab):
    _, t, _ = _walk(stab, 1)
    j = NSEG - 2                                                     # the second advance of the down sweep
    unplanted = t["maxAbs"][0, 0, j]
    row, col = 7, 21
    ctx = _context(stab, 1)
    try:
        ctx.set_green_check(True)
        _walk_down(ctx, 1, {}, upto=j + 1)
        for k in range((j + 1) * S, j * S, -1):
            ctx.wrapDownGreen(k)
        assert ctx.currentTimeslice == j * S
        g = ctx.g
        g[row, col] += 1e-3
        ctx.set_green(g, j * S)
        assert ctx.green_check()["count"][0, 0, j] == 0              # dqmc_set_green_host takes no sample itself
        ctx.advanceDownGreen(j + 1)
        got = ctx.green_check()
        assert got["count"][0, 0, j] == 1
        assert tuple(got["argmax"][0, 0, j]) == (row, col)
        assert abs(got["maxAbs"][0, 0, j] - 1e-3) <= unplanted, (got["maxAbs"][0, 0, j] - 1e-3, unplanted)
        assert got["maxSiteDiag"][0, 0, j] < 1e-6                    # (7, 21): not on the site diagonal
        assert ctx.green_check_raw().shape == (1, 2, NSEG + 1, 11)
    finally:
        ctx.close()


def _hubbard_ctx(rep):
    from detqmc_amd.model import _CtxView
    inf = rep.info

    class _I:
        opdim, L, m, s, N, MSF, n_g, n = 1, inf.L, inf.m, inf.s, inf.N, 2, 2 * inf.N, inf.n
    return _CtxView(rep.lib, rep.lib.dethubbard_ctx(rep.h), _I)


def test_planted_error_hubbard():
    from detqmc_amd import DetHubbard, HubbardParams
    pars = HubbardParams(L=4, beta=2.0, dtau=0.1, s=5, stabilisation="qr")
    row, col = 3, 9
    maxabs = []
    for plant in (False, True):
        rep = DetHubbard(pars)
        try:
            ctx = _hubbard_ctx(rep)
            m, s, n = ctx.m, ctx.s, ctx.n
            assert (m, s, n) == (20, 5, 4)
            ctx.set_green_check(True)
            for k in range(m, (n - 1) * s, -1):
                ctx.wrapDownGreen(k)
            if plant:
                g = ctx.g
                g[row, col] += 1e-3
                ctx.set_green(g, (n - 1) * s)
            ctx.advanceDownGreen(n)
            t = ctx.green_check()
            assert t["count"].sum() == 1 and t["count"][0, 0, n - 1] == 1
            maxabs.append(t["maxAbs"][0, 0, n - 1])
            if plant:
                assert tuple(t["argmax"][0, 0, n - 1]) == (row, col)
        finally:
            rep.close()
    assert 0 < maxabs[0] < 1e-6
    assert abs(maxabs[1] - 1e-3) <= maxabs[0], (maxabs[1] - 1e-3, maxabs[0])


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the chain is untouched
# ------------------------------------------------------------------------------------------------------------------------------
def _snapshot(batch):
    out = []
    for b in range(len(batch)):
        c = batch.chain(b)
        i = c.info
        out.append(dict(phi=c.phi, g=c.g, rngDrawn=int(i.rngDrawn), phiDelta=i.phiDelta, acc=i.lastAccRatioLocal_phi,
                        obs=np.frombuffer(bytes(c.observables), dtype=np.uint8)))
    return out


def _assert_same_chain(a, b, what):
    for ch, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert np.array_equal(x[k], y[k]), f"{what}: chain {ch}, {k} differs"


@pytest.mark.parametrize("stab", ["qr", "svd"])
def test_host_layer_chain_is_untouched(stab):
    from detqmc_amd import DetSDWBatch, DqmcError, SDWParams
    p = SDWParams(opdim=2, L=4, beta=2.0, dtau=0.1, s=5, delaySteps=4, stabilisation=stab, fermionMeasurements=True, rngSeed=97531)
    pars = [dataclasses.replace(p, simindex=b, r=-1.0 + 0.2 * b) for b in range(3)]
    plain, checked = DetSDWBatch(pars), DetSDWBatch(pars)
    try:
        n = plain.chain(0).info.n
        assert n == 4
        with pytest.raises(DqmcError):
            checked.green_check()                                    # the switch is off
        with pytest.raises(DqmcError):
            checked.green_check_reset()
        checked.set_green_check(True)
        start = _snapshot(plain)
        for i in range(6):
            for batch in (plain, checked):
                if i < 4:
                    batch.sweepThermalization()
                else:
                    batch.sweep(True)
            _assert_same_chain(_snapshot(checked), _snapshot(plain), f"sweep {i}")
        for a, b in zip(start, _snapshot(plain)):                    # the chains did move
            assert b["rngDrawn"] > a["rngDrawn"] and not np.array_equal(a["phi"], b["phi"]) and not np.array_equal(a["obs"], b["obs"])
        t = checked.green_check()
        want = np.zeros((2, n + 1), dtype=np.int64)
        want[0, :n] = 3                                              # sweeps alternate, the first goes down
        want[1, 1:] = 3
        for b in range(3):
            assert np.array_equal(t["count"][b], want), (b, t["count"][b])
        assert t["count"].sum() == 3 * 6 * n
        assert (t["nonfinite"] == 0).all() and (t["maxAbs"][t["count"] > 0] > 0).all() and t["maxAbs"].max() < 1e-6
        worst = checked.green_check_worst()
        assert len(worst) == 3
        for b, (mx, d, j, row, col) in enumerate(worst):
            assert mx == t["maxAbs"][b].max() == t["maxAbs"][b, d, j] and (row, col) == tuple(t["argmax"][b, d, j])
        with pytest.raises(RuntimeError):
            checked.chain(1).green_check()                           # the tables belong to the batch
        checked.green_check_reset()
        assert checked.green_check()["count"].sum() == 0
        # off again: the shortcuts are back and the chains stay in step
        checked.set_green_check(False)
        with pytest.raises(DqmcError):
            checked.green_check()
        for i in range(2):
            plain.sweepThermalization()
            checked.sweepThermalization()
        _assert_same_chain(_snapshot(checked), _snapshot(plain), "after switching off")
    finally:
        plain.close()
        checked.close()


def test_reader_is_chain_major_across_kernel_contexts():
    """four chains in one kernel context and in two: the same chains, so the same tables in handle order"""
    from detqmc_amd import DetSDWBatch, SDWParams
    p = SDWParams(opdim=2, L=4, beta=1.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr", rngSeed=2468)
    pars = [dataclasses.replace(p, simindex=b, r=-1.0 + 0.2 * b) for b in range(4)]
    tables = []
    for sub in (1, 2):
        batch = DetSDWBatch(pars, sub_batches=sub)
        try:
            assert batch.sub_batches == sub
            batch.set_green_check(True)
            batch.sweepThermalization()
            batch.sweepThermalization()
            tables.append(batch.green_check())
        finally:
            batch.close()
    assert tables[0]["count"].shape == (4, 2, 3) and (tables[0]["count"].sum(axis=(1, 2)) == 4).all()
    assert len({float(x) for x in tables[0]["maxAbs"][:, 0, 0]}) == 4             # four different chains
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[1][k]), k


def test_single_replica_surface():
    from detqmc_amd import DetSDW, SDWParams
    rep = DetSDW(SDWParams(opdim=2, L=4, beta=1.0, dtau=0.1, s=5, delaySteps=4, stabilisation="qr"))
    try:
        rep.set_green_check(True)
        rep.sweepThermalization()
        t = rep.green_check()
        assert t["count"].shape == (1, 2, 3) and np.array_equal(t["count"][0], [[1, 1, 0], [0, 0, 0]])
        (mx, d, j, row, col), = rep.green_check_worst()
        assert d == 0 and mx == t["maxAbs"][0, 0].max()
        rep.green_check_reset()
        assert rep.green_check()["count"].sum() == 0
    finally:
        rep.close()


def test_hubbard_chain_is_untouched():
    from detqmc_amd import DetHubbard, DqmcError, HubbardParams
    pars = HubbardParams(L=4, beta=2.0, dtau=0.1, s=5, stabilisation="qr")
    plain, checked = DetHubbard(pars, nchains=2), DetHubbard(pars, nchains=2)

    def snap(rep):
        out = []
        for b in range(2):
            rep.select(b)
            gu, gd = rep.green
            out.append(dict(aux=rep.auxfield, gu=gu, gd=gd, rng=int(rep.info.rngDrawn), obs=np.frombuffer(bytes(rep.observables), dtype=np.uint8)))
        return out
    try:
        with pytest.raises(DqmcError):
            checked.green_check()
        checked.set_green_check(True)
        for i in range(4):
            for rep in (plain, checked):
                rep.sweep(i >= 2)
            _assert_same_chain(snap(checked), snap(plain), f"sweep {i}")
        t = checked.green_check()
        n = checked.info.n
        want = np.zeros((2, n + 1), dtype=np.int64)
        want[0, :n] = 2
        want[1, 1:] = 2
        for b in range(2):
            assert np.array_equal(t["count"][b], want)
        assert (t["nonfinite"] == 0).all() and 0 < t["maxAbs"].max() < 1e-6
        assert len(checked.green_check_worst()) == 2
        checked.set_green_check(False)
        for rep in (plain, checked):
            rep.sweepThermalization()
        _assert_same_chain(snap(checked), snap(plain), "after switching off")
    finally:
        plain.close()
        checked.close()
