"""Kernel-level tests of the kernels that carry the model: k_bmult_chain (all launch shapes of launch_bmult, ragged tiles, LDS above
48 KiB, shift mode, batches), the Green's-function shift, k_measure_accum / k_measure_td and the small field kernels, each against
the long-double reference of tests/model_reference.py under an error bound derived from operation counts (never from kernel
output), plus exact cases that must reproduce their input value for value.  Every test prints `RATIO <family> <case> <max err/bound>`."""
import math
import os

import numpy as np
import pytest

import model_reference as mr
from model_reference import LEFT, RIGHT, ModelReference, U, bmult_c, check_bound, shift_c

pytestmark = pytest.mark.gpu

M_SLICES, S_SLICES, DTAU = 4, 2, 0.1        # storage is (n + 1) UdV triples of n_g^2: keep n = 2

# ------------------------------------------------------------------------------------------------------------------------------
# launch shapes: the documented rule of launch_bmult, and the rows the sizes below were chosen for
# ------------------------------------------------------------------------------------------------------------------------------
# (opdim, L): (n_g, LEFT nvec, LEFT ragged, RIGHT nvec, RIGHT ragged, RIGHT threads, RIGHT dynamic LDS bytes)
SHAPES = {
    (2, 10): (200, 11, 2, 8, 0, 512, 28800),
    (2, 14): (392, 6, 2, 8, 0, 512, 56448),
    (2, 20): (800, 3, 2, 8, 0, 512, 115200),
    (2, 24): (1152, 3, 0, 7, 4, 256, 147456),       # ragged RIGHT tile, LDS at the cap exactly
    (2, 26): (1352, 3, 2, 5, 2, 256, 129792),       # ragged RIGHT tile
    (3, 12): (576, 7, 2, 8, 0, 512, 82944),
    (3, 14): (784, 5, 4, 8, 0, 512, 112896),
    (3, 18): (1296, 3, 0, 6, 0, 256, 145152),
    (3, 22): (1936, 2, 0, 3, 1, 256, 123904),       # ragged RIGHT tile
    (3, 24): (2304, 1, 0, 3, 0, 256, 147456),
}
SMALL = [(2, 4), (3, 4), (2, 6), (3, 6), (2, 8), (3, 8), (2, 16), (3, 16)]      # RIGHT always 8 rows / 512 threads, never ragged
SIZES = SMALL + list(SHAPES)


def launch_shape(ng, P, side):
    """(nvec, ragged, threads, dynamic LDS bytes) by the rule documented in launch_bmult: LEFT max(n_g / 256, ceil(256 / P)) columns
    within 64 KiB; RIGHT 8 rows plus one padding row within 144 KiB; 512 threads for 8-row tiles, else 256.

    This is a HAND COPY of the rule in launch_bmult (kernels_bmult.hip): the C ABI does not report the launch shape, so nothing here
    is read from the library.  Whoever retunes launch_bmult updates this function with it; the table SHAPES then says which sizes
    have lost the shape they were chosen for.  The developer knobs that override the rule must be unset (_assert_shape)."""
    if side == LEFT:
        nvec = min(max(ng // 256, -(-256 // P)), ng, 65536 // (ng * 16))
        nvec = max(nvec, 1)
        return nvec, ng % nvec, 256, nvec * ng * 16
    nvec = max(min(8, 144 * 1024 // (ng * 16) - 1), 1)
    return nvec, ng % nvec, 512 if nvec >= 8 else 256, (nvec + 1) * ng * 16


def _assert_shape(opdim, L):
    for knob in ("DQMC_BMULT_NVEC_L", "DQMC_BMULT_NVEC_R", "DQMC_BMULT_THREADS_R"):
        assert not os.environ.get(knob), f"{knob} overrides the launch shape these cases were chosen for: unset it"
    MSF = 4 if opdim == 3 else 2
    ng, P = MSF * L * L, L * L // 4
    l, r = launch_shape(ng, P, LEFT), launch_shape(ng, P, RIGHT)
    key = (3 if opdim == 3 else 2, L)           # O(1) has the matrix size of O(2)
    if key in SHAPES:
        assert (ng, l[0], l[1], r[0], r[1], r[2], r[3]) == SHAPES[key], \
            "launch_bmult's rule no longer gives the launch shape this size was chosen for: re-choose the sizes"
    elif key in SMALL:
        assert r[:3] == (8, 0, 512)
    assert l[3] <= 65536 and r[3] <= 144 * 1024


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
BASE = dict(mux=-0.3, muy=0.7, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)    # band-dependent mu and anisotropic hoppings everywhere:
#                                                                                 a band mix-up or an ov / ovinv swap cannot cancel


def _params(opdim, L, **over):
    kw = dict(opdim=opdim, L=L, dtau=DTAU, delaySteps=4, lambda_=1.0, bc="pbc", weakZflux=False, checkerboard=True, cdwU=0.0, **BASE)
    kw.update(over)
    return kw


def _make(opdim, L, nchains=1, timeDisplaced=False, m=M_SLICES, s=S_SLICES, **over):
    from detqmc_amd import KernelContext
    kw = _params(opdim, L, **over)
    ctx = KernelContext(m=m, s=s, nchains=nchains, timeDisplaced=timeDisplaced, **kw)
    okw = {k: v for k, v in kw.items() if k != "stabilisation"}      # an execution choice of the device, unknown to the oracle
    ref = ModelReference(mr.make_lattice(beta=m * DTAU, s=s, **okw))
    assert ref.m == m and ref.ng == ctx.ng
    return ctx, ref


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


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_context():
    yield
    if "ctx" in _cache:
        _cache["ctx"].close()
    _cache.clear()


def _case(key, opdim, L, **over):
    """one context / reference / field / device caches per case, shared by the tests of both sides (they are adjacent)"""
    if _cache.get("key") != key:
        if "ctx" in _cache:
            _cache["ctx"].close()
        _cache.clear()
        ctx, ref = _make(opdim, L, **over)
        phi, cdwl = _fields(ref, 100 * L + opdim)
        _set(ctx, ref, phi, cdwl)
        _, ch, sh = ctx.get_fields()
        _cache.update(key=key, ctx=ctx, ref=ref, phi=phi, cdwl=cdwl, ch=ch, sh=sh, A=_matrix(ref.ng, L))
    c = _cache
    return c["ctx"], c["ref"], c["phi"], c["cdwl"], c["ch"], c["sh"], c["A"]


def _c(ref, nslices):
    if ref.p.checkerboard:
        return bmult_c(ref.MSF, nslices, bool(ref.p.cdwU))
    return nslices * (mr.dense_c(ref.N, 1) + 4 * (ref.MSF + 2) + 2)


def _bmult_against_reference(tag, ctx, ref, phi, cdwl, ch, sh, A, side, chains):
    worst = 0.0
    for inv in (0, 1):
        for k2, k1 in chains:
            got = ctx.bmult(side, inv, k2, k1, A)
            # the device's own cosh / sinh caches go into the reference: k_cosh_sinh has its own test below
            val, comp = ref.apply_B(A, side, inv, k2, k1, phi, cdwl, cosh=ch, sinh=sh)
            worst = max(worst, check_bound(got, val, comp, _c(ref, k2 - k1), what=f"{tag} inv {inv} B({k2},{k1})"))
    assert np.array_equal(ctx.bmult(side, 1, chains[-1][0], chains[-1][1], A), got), "the same call twice must give the same bits"
    print(f"RATIO bmult {tag} {worst:.3f}")


SIDE = {"left": LEFT, "right": RIGHT}


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("opdim,L", SIZES, ids=[f"o{o}-L{L}" for o, L in SIZES])
def test_bmult_vs_long_double(opdim, L, side):
    """all launch shapes: side x inverse, one slice (k = 3) and a chain: all m slices up to n_g = 1024, two slices above (the
    long-double reference, not the device, is what takes the time there)"""
    _assert_shape(opdim, L)
    ctx, ref, phi, cdwl, ch, sh, A = _case(("base", opdim, L), opdim, L)
    chain = (M_SLICES, 0) if ref.ng <= 1024 else (2, 0)
    _bmult_against_reference(f"o{opdim}-L{L}-{side}", ctx, ref, phi, cdwl, ch, sh, A, SIDE[side], [(3, 2), chain])


# each variant at a small, a ragged-RIGHT and a large size.  checkerboard = False stops at L = 10: its set-up diagonalises K on the
# host by cyclic Jacobi and its reference is a dense long-double product, both O(N^3); there the hopping part is a GEMM (tested in
# test_gpu_primitives.py) and k_bmult_chain only runs the site mix.
VARIANTS = [
    ("flux", dict(weakZflux=True), [(2, 4), (2, 24), (2, 26)]),
    ("flux-apbcxy", dict(weakZflux=True, bc="apbc-xy"), [(2, 6), (2, 24)]),
    ("apbcx", dict(bc="apbc-x"), [(2, 4), (3, 22), (2, 26)]),
    ("apbcxy", dict(bc="apbc-xy"), [(3, 4), (2, 24), (3, 24)]),
    ("cdw", dict(cdwU=0.7), [(2, 4), (3, 4), (3, 22), (2, 26)]),
    ("o1", dict(), [(1, 4), (1, 24), (1, 26)]),
    ("dense", dict(checkerboard=False), [(2, 4), (3, 4), (2, 10)]),
    ("dense-flux", dict(checkerboard=False, weakZflux=True), [(2, 4)]),
    # checkerboard = False at the ragged-RIGHT and large sizes, where the dense site-mix stage of k_bmult_chain runs with nv < nvec,
    # 256 threads and LDS above 48 KiB: without hopping K is diagonal, so the set-up converges at once and the reference of the
    # hopping part is a scalar per band; the site mix (lambda = 1, random phi) and the band factors are as everywhere else
    ("dense-nohop", dict(checkerboard=False, txhor=0.0, txver=0.0, tyhor=0.0, tyver=0.0), [(2, 4), (2, 24), (3, 22), (2, 26), (3, 24)]),
]
VCASES = [(name, over, o, L, side) for name, over, sizes in VARIANTS for o, L in sizes for side in ("left", "right")]


@pytest.mark.parametrize("name,over,opdim,L,side", VCASES, ids=[f"{n}-o{o}-L{L}-{s}" for n, _, o, L, s in VCASES])
def test_bmult_variants_vs_long_double(name, over, opdim, L, side):
    _assert_shape(opdim, L)
    ctx, ref, phi, cdwl, ch, sh, A = _case((name, opdim, L), opdim, L, **over)
    chains = [(2, 1), (M_SLICES, 0)] if ref.ng <= 1024 else [(2, 1), (2, 0)]
    _bmult_against_reference(f"{name}-o{opdim}-L{L}-{side}", ctx, ref, phi, cdwl, ch, sh, A, SIDE[side], chains)


# ------------------------------------------------------------------------------------------------------------------------------
# exact family: B_k = 1, then B_k = diag(e^{+-dtau mu_band})
# ------------------------------------------------------------------------------------------------------------------------------
ZERO_HOP = dict(txhor=0.0, txver=0.0, tyhor=0.0, tyver=0.0)


def _scaled(A, f, side, N):
    """A with row blocks (LEFT) resp. column blocks (RIGHT) times f[block & 1]: one fp64 rounding per component"""
    n = A.shape[0]
    fv = np.array([f[(i // N) & 1] for i in range(n)])
    fv = fv[:, None] if side == LEFT else fv[None, :]
    out = np.empty_like(A)
    out.real, out.imag = A.real * fv, A.imag * fv
    return out


EXACT = SIZES + [(1, 4), (1, 24)]


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("opdim,L", EXACT, ids=[f"o{o}-L{L}" for o, L in EXACT])
def test_bmult_exact_identity_and_band_factor(opdim, L, side):
    """lambda = 0 (cosh = 1, sinh / |phi| = 0: the site mix is the identity), zero hoppings (identity plaquette factors) and
    mu = 0 (band factors 1) make B_k the identity (tests/test_model_reference_cpu.py::test_exact_family_tables): every element
    of every tile must come back as the value it went in with.  With mu != 0 the result is A times e^{+-dtau mu_band} per band
    block, one rounding per component and slice; the factor is read off the device (B applied to the identity matrix)."""
    _assert_shape(opdim, L)
    sd = SIDE[side]
    for flux in ((False, True) if (opdim == 2 and L in (4, 24)) else (False,)):
        for mu in (dict(mux=0.0, muy=0.0), dict(mux=-0.3, muy=0.7)):
            ctx, ref = _make(opdim, L, lambda_=0.0, weakZflux=flux, bc="apbc-xy" if flux else "pbc", **ZERO_HOP, **mu)
            try:
                phi, _ = _fields(ref, 7)
                ctx.set_fields(phi)
                A = _matrix(ref.ng, 3 * L + opdim)
                eye = np.eye(ref.ng, dtype=complex)
                for inv in (0, 1):
                    D = ctx.bmult(sd, inv, 1, 0, eye)
                    f = [D[0, 0].real, D[ref.N, ref.N].real]
                    assert np.array_equal(D, _scaled(eye, f, sd, ref.N)), "B_k is not the expected diagonal matrix"
                    if mu["mux"] == 0.0:
                        assert f == [1.0, 1.0]
                    else:
                        sgn = -1.0 if inv else 1.0
                        assert f == [math.exp(sgn * DTAU * mu["mux"]), math.exp(sgn * DTAU * mu["muy"])]
                    for k2, k1 in ((3, 2), (M_SLICES, 0)):
                        want = A
                        for _ in range(k2 - k1):
                            want = _scaled(want, f, sd, ref.N)
                        got = ctx.bmult(sd, inv, k2, k1, A)
                        bad = np.argwhere(got != want)
                        assert bad.size == 0, (f"flux {flux} mu {mu} inv {inv} B({k2},{k1}): {len(bad)} elements differ, first at "
                                               f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
            finally:
                ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opdim,L,nb,over", [(2, 4, 3, {}), (3, 4, 8, {}), (2, 10, 8, {}), (2, 24, 3, {}), (3, 22, 3, {}),
                                             (2, 6, 3, dict(cdwU=0.7)), (2, 24, 3, dict(weakZflux=True))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_bmult_batch_matches_single_chain_twins(opdim, L, nb, over):
    """different fields per chain; chain b must equal, bit for bit, a single-chain context that was given chain b's fields"""
    batch, ref = _make(opdim, L, nchains=nb, **over)
    single, _ = _make(opdim, L, **over)
    try:
        fields = [_fields(ref, 50 + b) for b in range(nb)]
        for b in range(nb):
            batch.select_chain(b)
            _set(batch, ref, *fields[b])
        A = _matrix(ref.ng, 9)
        for b in range(nb):
            batch.select_chain(b)
            _set(single, ref, *fields[b])
            for side in (LEFT, RIGHT):
                for inv in (0, 1):
                    for k2, k1 in ((2, 1), (M_SLICES, 0)):
                        assert np.array_equal(batch.bmult(side, inv, k2, k1, A), single.bmult(side, inv, k2, k1, A)), (b, side, inv, k2)
            if b == 0:      # and chain 0 against the reference, so that "equal" is not "equally wrong"
                phi, cdwl = fields[0]
                _, ch, sh = single.get_fields()
                val, comp = ref.apply_B(A, RIGHT, 0, 2, 1, phi, cdwl, cosh=ch, sinh=sh)
                check_bound(batch.bmult(RIGHT, 0, 2, 1, A), val, comp, _c(ref, 1), what="batch chain 0")
    finally:
        batch.close()
        single.close()


# ------------------------------------------------------------------------------------------------------------------------------
# Green's-function shift
# ------------------------------------------------------------------------------------------------------------------------------
SHIFT = [(2, 4, {}), (2, 10, {}), (2, 16, {}), (2, 24, {}), (3, 12, {}), (3, 22, {}), (1, 10, {}),
         (2, 4, dict(weakZflux=True)), (2, 24, dict(weakZflux=True, bc="apbc-xy")), (2, 10, dict(bc="apbc-x")), (3, 22, dict(bc="apbc-xy")),
         (2, 4, dict(checkerboard=False)), (3, 4, dict(checkerboard=False)), (2, 10, dict(checkerboard=False, weakZflux=True))]


@pytest.mark.parametrize("opdim,L,over", SHIFT, ids=lambda v: str(v).replace(" ", ""))
def test_shift_green_vs_long_double(opdim, L, over):
    """shift mode of k_bmult_chain: half-step tables, sub-lattice 1 then 0, RIGHT with the + sign then LEFT with the - sign"""
    ctx, ref = _make(opdim, L, **over)
    try:
        ctx.set_fields(_fields(ref, 1)[0])
        G = _matrix(ref.ng, 11 + L)
        ctx.set_green(G, M_SLICES)
        got = ctx.shiftGreenSymmetric()
        val, comp = ref.shift_green(G)
        c = shift_c() if ref.p.checkerboard else mr.dense_c(ref.N, 2)
        r = check_bound(got, val, comp, c, what="shiftGreenSymmetric")
        assert np.array_equal(ctx.shiftGreenSymmetric(), got)
        assert np.array_equal(ctx.g, G), "the shift must not touch G"
        print(f"RATIO shift o{opdim}-L{L}-{over} {r:.3f}")
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim,L", [(2, 4), (2, 10), (2, 24), (2, 26), (3, 12), (3, 22), (3, 24)])
def test_shift_green_exact_with_zero_hopping(opdim, L):
    """no hopping: the half-step factors are identity matrices and the output is the input, value for value (mu and phi do not enter)"""
    for flux in ((False, True) if opdim == 2 and L in (4, 24) else (False,)):
        ctx, ref = _make(opdim, L, weakZflux=flux, **ZERO_HOP)
        try:
            ctx.set_fields(_fields(ref, 1)[0])
            G = _matrix(ref.ng, 5)
            ctx.set_green(G, M_SLICES)
            got = ctx.shiftGreenSymmetric()
            bad = np.argwhere(got != G)
            assert bad.size == 0, f"{len(bad)} elements differ, first at {tuple(bad[0])}"
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# measurement kernels
# ------------------------------------------------------------------------------------------------------------------------------
def measure_t(ref, samples=1):
    """t of  |acc - ref| <= t u sum|terms|  per accumulator of k_measure_accum, from its summation scheme (256 threads):
      greenK0     each thread adds ceil(n_g^2 / 2048) elements into each of 8 partial sums, 3 levels combine them, an 8-level tree
                  the threads, one more for the add into the accumulator
      greenLocal  ceil(n_g / 256) elements per thread, the tree, the division by 4 N, the add
      occDiffSq   16 terms per site (the polynomial written out), ceil(N / 256) sites per thread, the tree; a term is a complex
                  product (2 roundings per component) behind at most 3 roundings of the factored bracket and one scaling: 6;
                  the division by N, the add
      pair        16 products per entry, 6 roundings inside each as above, the add
      bins        a lane adds up to ceil(N / 8) sites of two terms each, 3 DPP levels, the add
    A second sample doubles the sums and adds one rounding."""
    N, ng, L = ref.N, ref.ng, ref.L
    W2 = (2 * L - 1) ** 2
    t = np.zeros(4 + 2 * N + 4 * W2)
    t[0] = -(-ng * ng // 2048) + 3 + 8 + 1
    t[1] = -(-ng // 256) + 8 + 2
    t[2] = 16 * -(-N // 256) + 8 + 6 + 2
    t[3] = 0
    t[4:4 + 2 * N] = 16 + 6 + 1
    t[4 + 2 * N:] = 2 * -(-N // 8) + 3 + 1
    return t + (samples - 1)


def _check_acc(got, val, mag, t, what):
    err = np.abs(got.astype(np.longdouble) - val).astype(float)
    lim = t * U * mag + np.abs(val.astype(float)) * U
    bad = np.argwhere(~(err <= lim))
    assert bad.size == 0, f"{what}: accumulator {int(bad[0][0])} off by {err[bad[0][0]]:.3e} > {lim[bad[0][0]]:.3e} ({len(bad)} entries)"
    return float(np.max(err / np.maximum(lim, 1e-300)))


MEAS = [(o, L) for L in (4, 6, 10, 16, 24) for o in (1, 2, 3)]


@pytest.mark.parametrize("opdim,L", MEAS, ids=[f"o{o}-L{L}" for o, L in MEAS])
def test_measure_accum_vs_long_double(opdim, L):
    """the device's own shifted matrix goes into the reference, so only k_measure_accum is compared; a general complex G makes
    every term of every observable O(1)"""
    ctx, ref = _make(opdim, L)
    try:
        ctx.set_fields(_fields(ref, 1)[0])
        n = ref.ng
        rng = np.random.default_rng(17 * L + opdim)
        G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        ctx.set_green(G, M_SLICES)
        gs = ctx.shiftGreenSymmetric()
        val, mag = ref.measure_accum(gs)
        assert len(val) == ctx.lib.dqmc_measure_accum_size(ctx.h)
        ctx.measure_reset()
        assert np.array_equal(ctx.measure_read(), np.zeros(len(val)))
        ctx.measure_slice()
        one = ctx.measure_read()
        assert one[3] == 1.0
        r1 = _check_acc(one, val, mag, measure_t(ref), "one sample")        # every bin (dx, dy) of both bands is in there
        ctx.measure_slice()
        two = ctx.measure_read()
        assert two[3] == 2.0
        r2 = _check_acc(two, 2 * val, 2 * mag, measure_t(ref, 2), "two samples")
        ctx.measure_reset()
        assert np.array_equal(ctx.measure_read(), np.zeros(len(val)))
        ctx.measure_slice()
        assert np.array_equal(ctx.measure_read(), one), "same input, same bits"
        print(f"RATIO measure o{opdim}-L{L} {max(r1, r2):.3f}")
    finally:
        ctx.close()


@pytest.mark.parametrize("opdim,L", [(2, 6), (3, 4), (1, 10)])
def test_measure_batch_matches_single_chain_twins(opdim, L):
    batch, ref = _make(opdim, L, nchains=3)
    single, _ = _make(opdim, L)
    try:
        n = ref.ng
        Gs = [_matrix(n, 30 + b) for b in range(3)]
        for b in range(3):
            batch.select_chain(b)
            batch.set_fields(_fields(ref, b)[0])
            batch.set_green(Gs[b], M_SLICES)
        batch.measure_reset()
        batch.measure_slice()
        for b in range(3):
            batch.select_chain(b)
            single.set_fields(_fields(ref, b)[0])
            single.set_green(Gs[b], M_SLICES)
            single.measure_reset()
            single.measure_slice()
            assert np.array_equal(batch.measure_read(), single.measure_read()), b
    finally:
        batch.close()
        single.close()


@pytest.mark.parametrize("opdim,L,m,s", [(1, 4, 20, 5), (2, 4, 20, 5), (3, 4, 20, 5), (2, 10, 15, 5), (3, 10, 15, 5)])
def test_measure_td_bins_vs_long_double(opdim, L, m, s):
    """k_measure_td at the boundaries j = n - 1 and j = 1 of a down pass: the bins of the shifted G(tau_j, 0) go into block j,
    count[j - 1] goes up by one, nothing else changes.  L = 10: 12 workgroups, 361 bins per band."""
    ctx, ref = _make(opdim, L, timeDisplaced=True, m=m, s=s, stabilisation="qr")
    try:
        n = ctx.n
        W2 = (2 * L - 1) ** 2
        phi = np.random.default_rng(opdim).uniform(-1, 1, (m + 1, ref.N, opdim))
        ctx.set_fields(phi)
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.set_timedisplaced(True)
        ctx.measure_reset()
        t = 2 * -(-ref.N // 8) + 3 + 1
        worst, seen = 0.0, []
        for k in range(m, (n - 1) * s, -1):
            ctx.wrapDownGreen(k)
        for l in range(n - 1, 0, -1):
            ctx.advanceDownGreen(l + 1)
            if l in (n - 1, 1):
                sl, gt0, _ = ctx.green_timedisplaced()
                assert sl == s * l
                g, ts = ctx.g, ctx.currentTimeslice
                ctx.set_green(gt0, ts)
                gs = ctx.shiftGreenSymmetric()           # the same kernels on the same bits as the shift inside the measurement
                ctx.set_green(g, ts)
                before = ctx.measure_td_read()
                ctx.measure_timedisplaced(l)
                after = ctx.measure_td_read()
                val, mag = ref.measure_td_bins(gs)
                lo = (n - 1) + (l - 1) * 4 * W2
                assert np.array_equal(before[lo:lo + 4 * W2], np.zeros(4 * W2))
                worst = max(worst, _check_acc(after[lo:lo + 4 * W2], val, mag, t, f"j = {l}"))
                changed = np.flatnonzero(after != before)
                assert after[l - 1] == before[l - 1] + 1.0
                assert set(changed) <= {l - 1} | set(range(lo, lo + 4 * W2)), "something outside block j changed"
                seen.append(l)
            for k in range(l * s, (l - 1) * s, -1):
                ctx.wrapDownGreen(k)
        assert seen == [n - 1, 1]
        print(f"RATIO measure_td o{opdim}-L{L} {worst:.3f}")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# field kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _check_caches(ctx, ref, phi, what):
    """k_cosh_sinh.  a = lambda dtau |phi| reaches the device with relative error e_a <= (OPDIM / 2 + 3) u (sum of squares OPDIM u,
    halved by the square root, the root itself, two products); cosh(a (1 + e)) = cosh a (1 + a tanh a e), |a tanh a| <= a; the
    device's cosh and sinh are taken as good to 2 ulp = 4 u (the accuracy the HIP math API documents for them is 1 to 2 ulp):
      cosh:        (a e_a + 4 u)
      sinh / |phi|: ((1 + a) e_a + 4 u + u [division] + (OPDIM / 2 + 1) u [|phi| itself])"""
    got_phi, ch, sh = ctx.get_fields()
    assert np.array_equal(got_phi[1:], phi[1:])
    rc, rs = ref.cosh_sinh(phi)
    a = (ref.p.lambda_ * ref.dtau * np.sqrt(np.sum(phi[1:] ** 2, axis=2)))
    ea = (ref.OPDIM / 2 + 3) * U
    ec = np.abs(ch[1:] - rc[1:]).astype(float) / rc[1:].astype(float)
    es = np.abs(sh[1:] - rs[1:]).astype(float) / rs[1:].astype(float)
    lc = a * ea + 4 * U
    ls = (1 + a) * ea + 5 * U + (ref.OPDIM / 2 + 1) * U
    assert np.all(ec <= lc), f"{what}: cosh cache off by {np.max(ec / lc):.2f} x bound"
    assert np.all(es <= ls), f"{what}: sinh cache off by {np.max(es / ls):.2f} x bound"
    return float(max(np.max(ec / lc), np.max(es / ls)))


FIELD = [(o, L, p2) for L in (4, 10, 24) for o in (1, 2, 3) for p2 in (False, True)]


@pytest.mark.parametrize("opdim,L,phi2bosons", FIELD, ids=[f"o{o}-L{L}-{'phi2' if p else 'full'}" for o, L, p in FIELD])
def test_field_kernels_vs_long_double(opdim, L, phi2bosons):
    nb = 3
    ctx, ref = _make(opdim, L, nchains=nb, phi2bosons=phi2bosons, c=2.5, u=1.3)
    try:
        rs = [-0.7, 0.4, 1.9]
        phis = []
        for b in range(nb):
            phi, _ = _fields(ref, 70 + b, scale=2.0)
            # one site with |phi| tiny but non-zero: a = 1e-10, the reference formula gives cosh = 1 and sinh(a) / |phi| =
            # lambda dtau (1 + a^2 / 6) = 0.1 to all digits (below |phi| ~ 1e-154 the squares underflow and the formula itself,
            # in the reference as on the device, is 0 / 0).  One site of order 10 / (lambda dtau): |phi| = 100, a = 10,
            # cosh = 11013.23..., sinh / |phi| = 110.13...
            phi[1, 0] = 0.0
            phi[1, 0, 0] = 1e-9
            phi[2, 1] = 0.0
            phi[2, 1, -1] = 10.0 / (1.0 * DTAU)
            phis.append(phi)
            ctx.select_chain(b)
            ctx.set_fields(phi)
            ctx.set_exchange_parameter(rs[b])
        worst = 0.0
        m, N = ref.m, ref.N
        # k_phi_action: 256 threads, ceil(m N / 256) (slice, site) pairs each, then an 8-level tree.  Inside a term: a difference, its
        # division by dtau, the square (which doubles what came before) and OPDIM additions, 4 + OPDIM; the coefficient
        # dtau / (2 c c) and its product, 4; phisq^2 carries 2 (OPDIM + 1) and three products: at most 2 OPDIM + 10 in any term;
        # four additions join the five terms of a pair
        t_action = (2 * opdim + 10) + 4 + -(-m * N // 256) + 8
        # k_phi_sq_sum: ceil(m OPDIM N / 256) squares per thread (one rounding each, one per add), the tree, times 1/2 dtau on the host
        t_sq = 2 * -(-m * opdim * N // 256) + 8 + 2
        act = ctx.phi_action_all()
        for b in range(nb):
            ctx.select_chain(b)
            worst = max(worst, _check_caches(ctx, ref, phis[b], f"chain {b}"))
            val, mag = ref.phi_action(phis[b], rs[b])
            assert abs(act[b] - val) <= t_action * U * mag, (b, float(abs(act[b] - val) / (t_action * U * mag)))
            worst = max(worst, float(abs(act[b] - val) / (t_action * U * mag)))
            val, mag = ref.phi_sq_sum(phis[b])
            ex = ctx.exchange_action()
            assert abs(ex - 0.5 * DTAU * val) <= t_sq * U * 0.5 * DTAU * mag
            worst = max(worst, float(abs(ex - 0.5 * DTAU * val) / (t_sq * U * 0.5 * DTAU * mag)))
        # k_phi_shift: one fp64 addition per component, slice 0 included; the caches follow
        sh = np.random.default_rng(5).uniform(-0.5, 0.5, (nb, opdim))
        ctx.shift_fields_all(sh)
        allphi = ctx.get_fields_all()
        for b in range(nb):
            want = phis[b] + sh[b][None, None, :]
            assert np.array_equal(allphi[b], want), b
            ctx.select_chain(b)
            worst = max(worst, _check_caches(ctx, ref, want, f"chain {b} after the shift"))
        print(f"RATIO fields o{opdim}-L{L}-{phi2bosons} {worst:.3f}")
    finally:
        ctx.close()
