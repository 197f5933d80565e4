"""The direct path of the checkerboard B-multiply (k_bmult_direct, dqmc_tuning::bmult_path = 2): first plaquette pass from global
memory, last one to global memory, the sub-1 half steps on either side of a slice boundary fused.  It must give the bits of the
staged kernel k_bmult_chain (bmult_path = 1) for every launch it takes and fall back to it for dense and shift launches; the same
calls are held against the long-double reference of tests/model_reference.py so that "equal" is not "equally wrong".  Plus
dqmc_wrap_skip, the bookkeeping-only wrap of a down sweep's segment ends."""
import numpy as np
import pytest

import model_reference as mr
from model_reference import LEFT, RIGHT, ModelReference, bmult_c, check_bound

pytestmark = pytest.mark.gpu

M_SLICES, S_SLICES, DTAU = 8, 4, 0.1         # n = 2 stored UdV triples; chains of 1, 2, 3 and s slices fit
CHAINS = [(3, 2), (8, 6), (4, 1), (S_SLICES, 0)]            # k2 - k1 = 1, 2, 3, s
BASE = dict(mux=-0.3, muy=0.7, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)    # band-dependent mu, anisotropic hoppings


def _contexts(opdim, L, nchains=1, paths=(1, 2), m=M_SLICES, s=S_SLICES, **over):
    from detqmc_amd import KernelContext
    kw = dict(opdim=opdim, L=L, dtau=DTAU, delaySteps=4, lambda_=1.0, bc="pbc", weakZflux=False, checkerboard=True, cdwU=0.0, **BASE)
    kw.update(over)
    ctxs = [KernelContext(m=m, s=s, nchains=nchains, bmultPath=p, **kw) for p in paths]
    okw = {k: v for k, v in kw.items() if k != "stabilisation"}      # an execution choice of the device, unknown to the oracle
    ref = ModelReference(mr.make_lattice(beta=m * DTAU, s=s, **okw))
    assert ref.m == m and ref.ng == ctxs[0].ng
    return ctxs, ref


def _fields(ref, seed, scale=1.2):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-scale, scale, (ref.m + 1, ref.N, ref.OPDIM))
    phi[0] = 0.0
    cdwl = rng.choice([-2, -1, 1, 2], (ref.m + 1, ref.N)).astype(np.int32)
    return phi, cdwl


def _matrix(n, seed):
    """dense complex, rows and columns on different scales: an element taken from the wrong row tile or column is visible"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * np.exp(rng.uniform(-2, 2, (n, 1))) \
        * np.exp(rng.uniform(-2, 2, (1, n)))


def _set(ctx, ref, phi, cdwl):
    ctx.set_fields(phi)
    if ref.p.cdwU:
        ctx.set_cdwl(cdwl)


def _compare(tag, opdim, L, nchains, **over):
    """bmult_path = 2 against bmult_path = 1, bit for bit: both sides, both inverses, chains of 1, 2, 3 and s slices, every chain of
    the batch with a field of its own.  Chain 0's results under bmult_path = 2 also against the long-double reference within
    bmult_c's bound -- every call up to n_g = 1024, the calls of at most two slices above (there the reference, not the device,
    takes the time: the rule of test_gpu_model_kernels.py)."""
    (old, new), ref = _contexts(opdim, L, nchains, **over)
    try:
        fields = [_fields(ref, 1000 * L + 10 * opdim + b) for b in range(nchains)]
        for ctx in (old, new):
            for b in range(nchains):
                ctx.select_chain(b)
                _set(ctx, ref, *fields[b])
        A = _matrix(ref.ng, 7 * L + opdim)
        worst = 0.0
        for b in range(nchains):
            old.select_chain(b)
            new.select_chain(b)
            if b == 0:
                _, ch, sh = new.get_fields()
            for side in (LEFT, RIGHT):
                for inv in (0, 1):
                    for k2, k1 in CHAINS:
                        got = new.bmult(side, inv, k2, k1, A)
                        want = old.bmult(side, inv, k2, k1, A)
                        bad = np.argwhere(got != want)
                        assert bad.size == 0, (f"{tag} chain {b} side {side} inv {inv} B({k2},{k1}): {len(bad)} elements differ from "
                                               f"k_bmult_chain, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")
                        if b == 0 and (ref.ng <= 1024 or k2 - k1 <= 2):
                            phi, cdwl = fields[0]
                            val, comp = ref.apply_B(A, side, inv, k2, k1, phi, cdwl, cosh=ch, sinh=sh)
                            c = bmult_c(ref.MSF, k2 - k1, bool(ref.p.cdwU))
                            worst = max(worst, check_bound(got, val, comp, c, what=f"{tag} side {side} inv {inv} B({k2},{k1})"))
        print(f"RATIO bmult-direct {tag} {worst:.3f}")
    finally:
        old.close()
        new.close()


# (opdim, L, chains): what the size exercises
SIZES = [
    (2, 4, 1),      # P = 4: every plaquette of sub-lattice 1 wraps in x or y; fewer items than threads
    (2, 6, 1),      # P = 9, not a power of two
    (3, 4, 1),      # MSF = 4
    (3, 8, 1),      # MSF = 4, more than one item per thread
    (2, 16, 8),     # the headline launch shape; every chain has its own field
    (2, 16, 3),     # grid not a multiple of 8
    (3, 24, 1),     # RIGHT with fewer than 8 rows per tile (3 rows, 256 threads), LEFT one column per workgroup
]


@pytest.mark.parametrize("opdim,L,nchains", SIZES, ids=[f"o{o}-L{L}-b{b}" for o, L, b in SIZES])
def test_direct_matches_staged_kernel_and_reference(opdim, L, nchains):
    _compare(f"o{opdim}-L{L}-b{nchains}", opdim, L, nchains)


VARIANTS = [
    ("apbcxy", 2, 4, dict(bc="apbc-xy")),
    ("apbcxy", 2, 8, dict(bc="apbc-xy")),
    ("flux", 2, 4, dict(weakZflux=True)),                     # complex plaquette tables
    ("flux-apbcxy", 2, 8, dict(weakZflux=True, bc="apbc-xy")),
    ("cdw", 2, 8, dict(cdwU=0.7)),
    ("cdw", 3, 4, dict(cdwU=0.7)),
    ("flux-cdw", 2, 4, dict(weakZflux=True, cdwU=0.7)),
    ("o1", 1, 8, dict()),
]


@pytest.mark.parametrize("name,opdim,L,over", VARIANTS, ids=[f"{n}-o{o}-L{L}" for n, o, L, _ in VARIANTS])
def test_direct_variants(name, opdim, L, over):
    _compare(f"{name}-o{opdim}-L{L}", opdim, L, 1, **over)


# ------------------------------------------------------------------------------------------------------------------------------
# path selection
# ------------------------------------------------------------------------------------------------------------------------------
def test_dense_and_shift_launches_fall_back():
    """bmult_path = 2 on a dense (checkerboard = False) context, and in shift mode on a checkerboard one, runs k_bmult_chain: its bits"""
    (old, new), ref = _contexts(2, 4, checkerboard=False)
    try:
        phi, _ = _fields(ref, 5)
        A = _matrix(ref.ng, 5)
        for ctx in (old, new):
            ctx.set_fields(phi)
        for side in (LEFT, RIGHT):
            for inv in (0, 1):
                for k2, k1 in CHAINS:
                    assert np.array_equal(new.bmult(side, inv, k2, k1, A), old.bmult(side, inv, k2, k1, A)), (side, inv, k2, k1)
    finally:
        old.close()
        new.close()
    for opdim, L, over in ((2, 4, {}), (3, 8, {}), (2, 8, dict(weakZflux=True))):
        (old, new), ref = _contexts(opdim, L, **over)
        try:
            phi, _ = _fields(ref, 6)
            G = _matrix(ref.ng, 11 + L)
            for ctx in (old, new):
                ctx.set_fields(phi)
                ctx.set_green(G, M_SLICES)
            assert np.array_equal(new.shiftGreenSymmetric(), old.shiftGreenSymmetric()), (opdim, L, over)
        finally:
            old.close()
            new.close()


def test_automatic_path_gives_the_same_bits():
    """bmult_path = 0, whatever it picks per launch kind, is one of the two kernels"""
    (old, auto), ref = _contexts(2, 16, 3, paths=(1, 0))
    try:
        for b in range(3):
            for ctx in (old, auto):
                ctx.select_chain(b)
                ctx.set_fields(_fields(ref, 40 + b)[0])
        A = _matrix(ref.ng, 2)
        for side in (LEFT, RIGHT):
            for inv in (0, 1):
                for k2, k1 in CHAINS:
                    assert np.array_equal(auto.bmult(side, inv, k2, k1, A), old.bmult(side, inv, k2, k1, A)), (side, inv, k2, k1)
    finally:
        old.close()
        auto.close()


def test_unknown_path_is_refused_at_create():
    from detqmc_amd import KernelContext
    from detqmc_amd import DqmcError
    for bad in (3, -1):
        with pytest.raises(DqmcError) as e:
            KernelContext(2, 4, 20, 10, 0.1, bmultPath=bad)
        assert e.value.code == -1 and "bmult_path" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------
# dqmc_wrap_skip
# ------------------------------------------------------------------------------------------------------------------------------
def test_wrap_skip_marks_g_stale_until_the_advance_rebuilds_it():
    """O(2), L = 4, m = 20, s = 5: the last wrap of the top segment skipped on one context, done on its twin.  While G is stale the
    entries that read it refuse; after dqmc_advance(DOWN, n) both hold the same G, bit for bit."""
    from detqmc_amd import DqmcError
    from detqmc_amd.model import DOWN
    m, s = 20, 5
    (full, skip), ref = _contexts(2, 4, paths=(0, 0), m=m, s=s, stabilisation="qr")
    try:
        phi, _ = _fields(ref, 9, scale=0.8)
        for ctx in (full, skip):
            ctx.set_fields(phi)
            ctx.setupUdVStorage_and_calculateGreen()
        n = full.n
        last = (n - 1) * s + 1
        for k in range(m, last, -1):
            full.wrapDownGreen(k)
            skip.wrapDownGreen(k)
        assert np.array_equal(full.g, skip.g)
        full.wrapDownGreen(last)
        skip.wrapSkip(DOWN, last)
        assert skip.currentTimeslice == full.currentTimeslice == last - 1
        for call in (lambda: skip.g, lambda: skip.updateInSlice(last - 1), lambda: skip.wrapDownGreen(last - 1),
                     lambda: skip.wrapSkip(DOWN, last - 1), lambda: skip.shiftGreenSymmetric(), lambda: skip.measure_slice()):
            with pytest.raises(DqmcError) as e:
                call()
            assert e.value.code == -1 and "stale" in str(e.value)
        assert skip.currentTimeslice == last - 1, "a refused call must not move the context"
        full.advanceDownGreen(n)
        skip.advanceDownGreen(n)
        G = skip.g                                          # readable again
        assert np.array_equal(G, full.g)
        assert np.array_equal(skip.g_inv_sv, full.g_inv_sv)
        # the skipped wrap checks what dqmc_wrap checks
        with pytest.raises(DqmcError):
            skip.wrapSkip(DOWN, last)                       # currentTimeslice != k
        with pytest.raises(DqmcError):
            skip.wrapSkip(7, last - 1)                      # unknown direction
        assert np.array_equal(skip.g, G)
    finally:
        full.close()
        skip.close()
