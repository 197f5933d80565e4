"""The checkerboard B-multiply out of place (launch_bmult with a source: the chain steps of dqmc_advance UP and dqmc_udv_setup).  The
first pass of k_bmult_direct, and the stage-in loop of k_bmult_chain, read the operands from a second buffer; everything after that is
the in-place kernel.  So the result must have the bits of "copy, then multiply in place", the destination's old content (NaN patterns
here, dqmc_bmult_src_host) must not enter it, and the source must come back unchanged."""
import numpy as np
import pytest

import model_reference as mr
from model_reference import LEFT, ModelReference

pytestmark = pytest.mark.gpu

M_SLICES, S_SLICES, DTAU = 8, 4, 0.1
CHAINS = [(3, 2), (8, 6), (4, 1), (S_SLICES, 0)]            # k2 - k1 = 1, 2, 3, s
BASE = dict(mux=-0.3, muy=0.7, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)
NCHAINS = 3


def _context(opdim, L, path, **over):
    from detqmc_amd import KernelContext
    kw = dict(opdim=opdim, L=L, dtau=DTAU, delaySteps=4, lambda_=1.0, bc="pbc", weakZflux=False, checkerboard=True, cdwU=0.0, **BASE)
    kw.update(over)
    ctx = KernelContext(m=M_SLICES, s=S_SLICES, nchains=NCHAINS, bmultPath=path, **kw)
    ref = ModelReference(mr.make_lattice(beta=M_SLICES * DTAU, s=S_SLICES, **kw))
    assert ref.ng == ctx.ng
    return ctx, ref


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * np.exp(rng.uniform(-2, 2, (n, 1))) \
        * np.exp(rng.uniform(-2, 2, (1, n)))


# path 1: every launch on k_bmult_chain; path 0: LEFT chains of two or more slices on k_bmult_direct, single slices on k_bmult_chain
CASES = [(1, 4, {}), (2, 4, {}), (3, 4, {}), (2, 8, dict(weakZflux=True)), (2, 8, dict(bc="apbc-xy"))]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("opdim,L,over", CASES, ids=["o1-L4", "o2-L4", "o3-L4", "o2-L8-flux", "o2-L8-apbc"])
def test_out_of_place_has_the_bits_of_copy_then_in_place(opdim, L, over, path):
    ctx, ref = _context(opdim, L, path, **over)
    try:
        for b in range(NCHAINS):
            rng = np.random.default_rng(100 * L + 10 * opdim + b)
            phi = rng.uniform(-1.2, 1.2, (ref.m + 1, ref.N, ref.OPDIM))
            phi[0] = 0.0
            ctx.select_chain(b)
            ctx.set_fields(phi)
        A = _matrix(ref.ng, 3 * L + opdim)
        seen = set()
        for b in range(NCHAINS):
            ctx.select_chain(b)
            for inv in (0, 1):
                for k2, k1 in CHAINS:
                    want = ctx.bmult(LEFT, inv, k2, k1, A)
                    got, after = ctx.bmult_src(LEFT, inv, k2, k1, A)
                    assert np.isfinite(got).all(), (b, inv, k2, k1)
                    bad = np.argwhere(got != want)
                    assert bad.size == 0, f"chain {b} inv {inv} B({k2},{k1}): {len(bad)} elements differ, first at {tuple(bad[0])}"
                    assert np.array_equal(after, A), f"chain {b} inv {inv} B({k2},{k1}): the source changed"
                    seen.add(want.tobytes())
        # every chain has its own field, every call its own slices: no two results may coincide (a kernel that read the wrong chain or
        # ignored the source would still have to reproduce 24 different matrices)
        assert len(seen) == NCHAINS * 2 * len(CHAINS)
    finally:
        ctx.close()
