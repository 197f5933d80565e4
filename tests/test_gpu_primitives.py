"""Kernel-level tests of the dense linear-algebra primitives (GEMM, delayed-update flush, LU, triangular solve, Householder and block
Gram-Schmidt QR) against plain references of the same operation, driven through the test-only entry points
(detqmc_amd/lib/libdqmc_primitives_test.so, tests/primitives.py) -- the launchers the product runs, on arenas with NaN sentinels
around every operand (Arena.check() after every launch).

Two kinds of reference:
  exact    small-integer entries, power-of-two scales and diagonals: every product, split-K sum and substitution is exact in fp64,
           so the result must be BIT-IDENTICAL to an int64 / numpy reference -- checks indexing in every branch at any size;
  rounding random and graded entries against a long-double (or float64 + its own bound) reference with the elementwise bound
           |C - C_ref| <= c (K + extra + 2) u sum_k |a_ik|_1 |b_kj|_1, c = 4 (primitives.elementwise_bound).
Every GEMM case asserts the branch it claims to reach (gemm_plan: tile, split factor, grid layout)."""
import numpy as np
import pytest

import primitives as P
from primitives import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import os
    if not os.path.exists(P.LIB_PATH):
        from detqmc_amd.build import build
        build(verbose=False)


# ------------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------------
def _gemm_case(M, N, K, nb, opA=0, opB=0, pad=3, opts=None, data="int", seed=0, shared=(), nan_chain=None):
    """lays out A, B, C (+ option operands) for nb chains, fills them, runs launch_gemm; returns (arena, spec, inputs per chain)"""
    opts = dict(opts or {})
    rng = np.random.default_rng(seed)
    ar = Arena(nb)
    Ar, Ac = (K, M) if opA else (M, K)
    Br, Bc = (N, K) if opB else (K, N)
    acols = Ac
    if "a_kgather" in opts:
        acols = Ac + 5                                   # gathered columns come from a wider A
    ar.mat("A", Ar, acols, Ar + pad, shared="A" in shared)
    ar.mat("B", Br, Bc, Br + pad, shared="B" in shared)
    ar.mat("C", M, N, M + pad, kind="out")
    names = {}
    for k in ("kscale", "rowscale", "colscale"):
        if k in opts:
            ar.vec(k, {"kscale": K, "rowscale": M, "colscale": N}[k], np.float64)
            names[k] = k
    if "a_kgather" in opts:
        ar.vec("a_kgather", K, np.int32)
        names["a_kgather"] = "a_kgather"
    if "Kdev" in opts:
        ar.vec("Kdev", 1, np.int32)
        names["Kdev"] = "Kdev"
    if "part" in opts:
        ar.vec("part", opts["part"], np.complex128, kind="scratch")
        names["part"] = "part"
    ar.layout()
    ins = []
    for b in range(nb):
        gen = (lambda r, c: P.int_matrix(rng, r, c)) if data == "int" else \
              (lambda r, c: rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c)))
        d = dict(A=gen(Ar, acols), B=gen(Br, Bc), C=gen(M, N))
        if opts.get("b_lower"):
            Bop = np.tril(P.op(d["B"], opB))             # op(B) lower triangular: k < j entries zero
            d["B"] = P.op(Bop, opB)
        if "kscale" in opts:
            d["kscale"] = 2.0 ** rng.integers(-3, 4, K) * rng.choice([-1, 1], K)
        if "rowscale" in opts:
            d["rowscale"] = 2.0 ** rng.integers(-3, 4, M)
        if "colscale" in opts:
            d["colscale"] = 2.0 ** rng.integers(-3, 4, N)
        if "a_kgather" in opts:
            d["a_kgather"] = rng.integers(0, acols, K).astype(np.int32)
        if "Kdev" in opts:
            d["Kdev"] = np.array([opts["Kdev"]], np.int32)
        if nan_chain is not None and b == nan_chain:
            d["A"] = np.full_like(d["A"], np.nan)
            d["B"] = np.full_like(d["B"], np.nan)
        for k in ("A", "B"):
            if b == 0 or k not in shared:
                ar.set(k, d[k], b)
        ar.set("C", d["C"], b)
        for k in ("kscale", "rowscale", "colscale", "a_kgather", "Kdev"):
            if k in d:
                ar.set(k, d[k], b)
        ins.append(d)
    if "A" in shared:
        for d in ins:
            d["A"] = ins[0]["A"]
    if "B" in shared:
        for d in ins:
            d["B"] = ins[0]["B"]
    kw = {k: v for k, v in opts.items() if k not in ("kscale", "rowscale", "colscale", "a_kgather", "Kdev", "part")}
    spec = P.gemm_spec(ar, A="A", B="B", C="C", opA=opA, opB=opB, M=M, N=N, K=K, sharedA="A" in shared, sharedB="B" in shared,
                       part_count=opts.get("part", 0) if "part" in opts else 0, **names, **kw)
    return ar, spec, ins


def op(X, o):
    return P.op(X, o)


def _gemm_operands(d, spec, opts):
    """op(A)[M x Keff] diag(kscale) and op(B)[Keff x N] as the kernel sees them"""
    K = spec.K
    if "Kdev" in opts:
        K = min(K, opts["Kdev"] * spec.Kmul)
    K = max(K, 0)
    A = d["A"]
    if "a_kgather" in opts:
        Aop = A[:, d["a_kgather"]]
    else:
        Aop = op(A, spec.opA)
    Aop = Aop[:, :K].copy()
    if "kscale" in opts:
        ks = d["kscale"][:K]
        Aop = Aop * (1.0 / ks if spec.kscale_invert else ks)[None, :]
    Bop = op(d["B"], spec.opB)[:K, :]
    return Aop, Bop


def _gemm_expected_exact(d, spec, opts):
    Aop, Bop = _gemm_operands(d, spec, opts)
    if Aop.shape[1] == 0:
        prod = np.zeros((spec.M, spec.N), complex)
    else:
        # dyadic entries (power-of-two k-scales): exact after scaling by 2^3 per factor
        s = 8.0 if "kscale" in opts else 1.0
        prod = P.exact_matmul(Aop * s, Bop) / s
    sc = np.ones((spec.M, spec.N))
    if "rowscale" in opts:
        sc = sc * d["rowscale"][:, None]
    if "colscale" in opts:
        sc = sc * d["colscale"][None, :]
    prod = prod * sc
    if spec.negate:
        prod = -prod
    return d["C"] + prod if spec.accumulate else prod


def _run_check_exact(ar, spec, ins, opts, what):
    P.run_gemm(ar, spec)
    for b, d in enumerate(ins):
        got = ar.get("C", b)
        exp = _gemm_expected_exact(d, spec, opts)
        assert np.array_equal(got, exp), "%s chain %d: max |err| %.3e" % (what, b, np.max(np.abs(got - exp)))


SHAPES = [(1, 15, 16), (17, 31, 33), (63, 64, 65), (200, 33, 513), (65, 200, 17), (15, 1040, 63), (513, 63, 200), (1040, 65, 31),
          (32, 16, 1), (64, 17, 32)]


@pytest.mark.parametrize("opA,opB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_exact_shapes(opA, opB):
    """ragged M, N, K with padded leading dimensions, all four op combinations, grid.z layout (nb = 3): bit-identical"""
    for (M, N, K) in SHAPES:
        ar, spec, ins = _gemm_case(M, N, K, 3, opA, opB, seed=M * 7 + N)
        plan = P.gemm_plan(spec, 3)
        assert plan["xcd"] == 0 and plan["ksplit"] == 1
        _run_check_exact(ar, spec, ins, {}, "M=%d N=%d K=%d ops=%d%d plan=%s" % (M, N, K, opA, opB, plan))


# (M, N, K, nb) -> expected plan: the 64-tile path by size (nb = 1) and by batch (nb = 8, 16), both grid layouts
TILE_CASES = [((1040, 1040, 40, 1), dict(tile=64, ksplit=1, xcd=0)),
              ((513, 520, 33, 1), dict(tile=32, ksplit=1, xcd=0)),
              ((200, 200, 64, 8), dict(tile=32, ksplit=1, xcd=1)),
              ((256, 256, 31, 16), dict(tile=64, ksplit=1, xcd=1)),
              ((513, 200, 17, 8), dict(tile=64, ksplit=1, xcd=1)),
              ((1100, 1040, 16, 3), dict(tile=64, ksplit=1, xcd=0)),
              ((100, 100, 48, 3), dict(tile=32, ksplit=1, xcd=0)),
              ((33, 1040, 65, 16), dict(tile=64, ksplit=1, xcd=1))]


@pytest.mark.parametrize("case", TILE_CASES, ids=lambda c: "M%d_N%d_K%d_nb%d" % c[0])
def test_gemm_exact_tiles_and_layouts(case):
    (M, N, K, nb), want = case
    for opA, opB in ((0, 0), (1, 1)):
        ar, spec, ins = _gemm_case(M, N, K, nb, opA, opB, seed=nb)
        assert P.gemm_plan(spec, nb) == want
        _run_check_exact(ar, spec, ins, {}, "tiles %s ops %d%d" % (want, opA, opB))


# every option alone and in the combinations production uses; (opts, spec fields)
OPTION_CASES = {
    "accumulate": dict(accumulate=1),
    "negate": dict(negate=1),
    "accumulate_negate": dict(accumulate=1, negate=1),
    "kscale": dict(kscale=1),
    "kscale_invert": dict(kscale=1, kscale_invert=1),
    "rowscale_only": dict(rowscale=1),
    "colscale_only": dict(colscale=1),
    "rowscale_colscale": dict(rowscale=1, colscale=1),
    "a_kgather": dict(a_kgather=1),
    "b_lower": dict(b_lower=1),
    "b_lower_accumulate_negate": dict(b_lower=1, accumulate=1, negate=1),
    "Kdev_below_K": dict(Kdev=7, Kmul=4),                  # K = min(K, 28)
    "Kdev_zero": dict(Kdev=0, Kmul=4),
    "Kdev_zero_accumulate": dict(Kdev=0, Kmul=4, accumulate=1),
    "Kdev_kscale_invert_accumulate_negate": dict(Kdev=9, Kmul=2, kscale=1, kscale_invert=1, accumulate=1, negate=1),
    "tag": dict(tag=1, accumulate=1, negate=1),
}


@pytest.mark.parametrize("name", sorted(OPTION_CASES))
@pytest.mark.parametrize("shape", [(70, 45, 50, 3), (200, 200, 40, 16)], ids=["tile32_z", "tile64_xcd"])
def test_gemm_exact_options(name, shape):
    M, N, K, nb = shape
    opts = dict(OPTION_CASES[name])
    opt_ops = {k: opts[k] for k in ("kscale", "rowscale", "colscale", "a_kgather", "Kdev") if k in opts}
    spec_kw = {k: v for k, v in opts.items() if k not in opt_ops}
    for opA, opB in ((0, 0), (1, 1), (0, 1)):
        if "a_kgather" in opts and opA:
            continue                                       # a_kgather: opA == 0 only
        ar, spec, ins = _gemm_case(M, N, K, nb, opA, opB, opts=dict(opt_ops, **spec_kw), seed=len(name))
        plan = P.gemm_plan(spec, nb)
        assert plan["tile"] == (64 if nb == 16 else 32) and plan["ksplit"] == 1
        _run_check_exact(ar, spec, ins, opts, "%s ops %d%d" % (name, opA, opB))


def test_gemm_exact_k_zero():
    """K = 0: C = 0 without accumulate, C untouched with it"""
    for acc in (0, 1):
        ar, spec, ins = _gemm_case(40, 24, 0, 3, opts=dict(accumulate=acc))
        _run_check_exact(ar, spec, ins, {}, "K=0 accumulate=%d" % acc)


@pytest.mark.parametrize("shared", ["A", "B"])
def test_gemm_exact_shared_operand(shared):
    for (M, N, K, nb) in ((50, 70, 33, 3), (200, 200, 40, 16)):
        ar, spec, ins = _gemm_case(M, N, K, nb, 0, 1, shared=(shared,), seed=5)
        _run_check_exact(ar, spec, ins, {}, "shared %s nb %d" % (shared, nb))


@pytest.mark.parametrize("K", [512, 520, 1023, 2304])
def test_gemm_exact_split_k(K):
    """split-K + k_gemm_reduce (a scratch buffer offered, K >= 512, few workgroups): slices of K whose length is not always a
    multiple of 16, with and without accumulate / negate in the reduction, and a part_count that caps the number of slices"""
    for (M, N, nb, cap, acc) in ((64, 64, 1, 8, 0), (70, 33, 3, 8, 1), (40, 64, 1, 3, 1), (64, 32, 8, 32, 0)):
        opts = dict(part=cap * M * N, accumulate=acc, negate=acc)
        ar, spec, ins = _gemm_case(M, N, K, nb, 1, 0, opts=opts, seed=K + M)
        plan = P.gemm_plan(spec, nb)
        wg = ((M + 31) // 32) * ((N + 31) // 32) * nb
        assert plan["tile"] == 32 and plan["ksplit"] == min(32, cap, K // 64, (512 + wg - 1) // wg) > 1, plan
        _run_check_exact(ar, spec, ins, dict(accumulate=acc), "split-K K=%d M=%d N=%d nb=%d %s" % (K, M, N, nb, plan))


def _graded(rng, r, c, decades=6):
    X = rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c))
    return X * (10.0 ** np.linspace(-decades / 2, decades / 2, r))[:, None] * (10.0 ** rng.uniform(-decades / 2, decades / 2, c))[None, :]


ROUND_CASES = [(64, 64, 64, 1, 0, 0), (200, 33, 513, 3, 1, 0), (63, 65, 1040, 1, 0, 1), (1040, 200, 31, 1, 1, 1), (256, 256, 64, 16, 0, 1)]


@pytest.mark.parametrize("case", ROUND_CASES, ids=lambda c: "M%d_N%d_K%d_nb%d_op%d%d" % c)
def test_gemm_rounding_elementwise(case):
    """graded random operands: elementwise bound against a long-double reference (float64 + its own bound when too large)"""
    M, N, K, nb, opA, opB = case
    ar, spec, ins = _gemm_case(M, N, K, nb, opA, opB, data="rand", seed=M + K)
    rng = np.random.default_rng(K)
    for b in range(nb):
        ins[b]["A"] = _graded(rng, *ins[b]["A"].shape)
        ins[b]["B"] = _graded(rng, *ins[b]["B"].shape)
        ar.set("A", ins[b]["A"], b)
        ar.set("B", ins[b]["B"], b)
    P.run_gemm(ar, spec)
    for b in range(nb):
        Aop, Bop = op(ins[b]["A"], opA), op(ins[b]["B"], opB)
        ref, rerr = P.matmul_ref(Aop, Bop)
        P.check_elementwise(ar.get("C", b), ref, P.elementwise_bound(Aop, Bop), rerr, "gemm %s chain %d" % (case, b))


def test_gemm_rounding_split_k():
    M, N, K = 64, 48, 2304
    ar, spec, ins = _gemm_case(M, N, K, 1, 1, 0, opts=dict(part=8 * M * N), data="rand", seed=3)
    ks = P.gemm_plan(spec, 1)["ksplit"]
    assert ks == 8
    P.run_gemm(ar, spec)
    Aop, Bop = op(ins[0]["A"], 1), op(ins[0]["B"], 0)
    ref, rerr = P.matmul_ref(Aop, Bop)
    P.check_elementwise(ar.get("C", 0), ref, P.elementwise_bound(Aop, Bop, extra=ks), rerr, "split-K")


@pytest.mark.parametrize("case", [(100, 70, 48, 0), (200, 200, 40, 0), (64, 64, 1040, 8 * 64 * 64)],
                         ids=["tile32", "tile64_batch", "split_k"])
def test_gemm_isolation_determinism(case):
    """chain 0 of a batch whose chain 1 is all NaN: same as two identical launches and (same branch) as chain 0 alone"""
    M, N, K, part = case
    opts = dict(part=part) if part else {}
    nb = 16 if M == 200 else 3
    runs = []
    for _ in range(2):
        ar, spec, ins = _gemm_case(M, N, K, nb, 0, 1, opts=opts, data="rand", seed=11, nan_chain=1)
        P.run_gemm(ar, spec)
        runs.append([ar.get("C", b) for b in range(nb)])
        plan_batch = P.gemm_plan(spec, nb)
    for b in range(nb):
        assert np.array_equal(runs[0][b], runs[1][b]) or b == 1, "two identical launches differ (chain %d)" % b
    assert np.all(np.isfinite(runs[0][0])) and np.all(np.isfinite(runs[0][2]))
    ar1, spec1, _ = _gemm_case(M, N, K, 1, 0, 1, opts=opts, data="rand", seed=11)
    plan1 = P.gemm_plan(spec1, 1)
    P.run_gemm(ar1, spec1)
    # the summation order is a function of (tile, ksplit) only; a larger batch may change either (64 tiles by batch, fewer
    # split-K slices once nb fills the chip): the launcher does not promise chain-alone identity then
    if (plan1["tile"], plan1["ksplit"]) == (plan_batch["tile"], plan_batch["ksplit"]):
        assert np.array_equal(ar1.get("C", 0), runs[0][0])
    else:
        Aop, Bop = _gemm_operands(_gemm_case(M, N, K, 1, 0, 1, data="rand", seed=11)[2][0], spec1, {})
        P.check_elementwise(runs[0][0], ar1.get("C", 0), 2 * P.elementwise_bound(Aop, Bop, extra=32), None, "batch vs alone")


# ------------------------------------------------------------------------------------------------------------------------------
# delayed-update flush  G += X GrT^T
# ------------------------------------------------------------------------------------------------------------------------------
def flush_kernel(n, Kmax):
    """the kernel launch_flush runs (shipped library, no developer knobs): k_flush_lds for n % 32 == 0 and Kmax <= 32, else k_flush,
    FULL when n % 32 == 0, the ragged form otherwise"""
    if n % 32 == 0:
        return "lds" if Kmax <= 32 else "full"
    return "ragged"


def _flush_case(n, Kmax, Kd, Kmul, nb, data="int", seed=0, nan_chain=None, pad=5):
    """Kd: device count (None: no Kdev); X, GrT are n x K8 (K8 = device K rounded up to 8, columns K .. K8 - 1 zero) and the columns
    beyond K8 are sentinels (a separate never-written region right behind them)"""
    K = Kmax if Kd is None else max(0, min(Kmax, Kd * Kmul))
    K8 = (K + 7) // 8 * 8
    rng = np.random.default_rng(seed)
    ar = Arena(nb)
    ld = n + pad
    ar.mat("X", n, max(K8, 1), ld)
    ar.mat("Xbeyond", ld, 8)                              # sentinels: what a read past column K8 - 1 of X would meet
    ar.mat("GrT", n, max(K8, 1), ld)
    ar.mat("Gbeyond", ld, 8)
    ar.mat("G", n, n, n + 3, kind="out")
    if Kd is not None:
        ar.vec("Kdev", 1, np.int32)
    ar.layout()
    ins = []
    for b in range(nb):
        if data == "int":
            X, Y, G = P.int_matrix(rng, n, K), P.int_matrix(rng, n, K), P.int_matrix(rng, n, n)
        else:
            X, Y, G = [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in ((n, K), (n, K), (n, n))]
        if nan_chain == b:
            X[:] = np.nan
        Xp = np.zeros((n, max(K8, 1)), complex)
        Yp = np.zeros((n, max(K8, 1)), complex)
        Xp[:, :K], Yp[:, :K] = X, Y
        ar.set("X", Xp, b)
        ar.set("GrT", Yp, b)
        ar.set("G", G, b)
        if Kd is not None:
            ar.set("Kdev", [Kd], b)
        ins.append((X, Y, G))
    return ar, ins, K


FLUSH_CASES = [(32, 8, None, 1, 1), (64, 16, 3, 4, 3), (72, 32, 5, 2, 8), (96, 32, 32, 1, 3), (128, 40, 9, 4, 1),
               (144, 64, 13, 4, 3), (160, 32, 7, 2, 8), (160, 64, 15, 4, 8), (512, 32, 8, 4, 3), (512, 64, 61, 1, 1),
               (1296, 64, 14, 4, 1), (96, 40, 10, 4, 3), (72, 8, 0, 4, 3), (512, 32, 0, 2, 8), (144, 64, 16, 4, 1),
               (33, 16, 3, 3, 3), (100, 40, 40, 1, 8)]


@pytest.mark.parametrize("case", FLUSH_CASES, ids=lambda c: "n%d_Kmax%d_Kd%s_Kmul%d_nb%d" % c)
def test_flush_exact(case):
    """bit-identical G + X GrT^T on integer data; K = 0 leaves G untouched; K not a multiple of 8; n = 32 (mod 64)"""
    n, Kmax, Kd, Kmul, nb = case
    ar, ins, K = _flush_case(n, Kmax, Kd, Kmul, nb, seed=n + Kmax)
    kern = flush_kernel(n, Kmax)
    for tag in (0, 1):
        P.run_flush(ar, n, Kmax, "Kdev" if Kd is not None else None, Kmul, tag)
        for b, (X, Y, G) in enumerate(ins):
            exp = G + (P.exact_matmul(X, Y.T) if K else 0)
            got = ar.get("G", b)
            assert np.array_equal(got, exp), "%s (%s) tag %d chain %d: max |err| %.3e" % (case, kern, tag, b, np.max(np.abs(got - exp)))
            ins[b] = (X, Y, exp)


def test_flush_kernels_reached():
    kinds = {flush_kernel(c[0], c[1]) for c in FLUSH_CASES}
    assert kinds == {"lds", "full", "ragged"}
    assert any(c[0] % 64 == 32 and flush_kernel(c[0], c[1]) == "lds" for c in FLUSH_CASES)
    assert any(c[0] % 64 == 32 and flush_kernel(c[0], c[1]) == "full" for c in FLUSH_CASES)


@pytest.mark.parametrize("case", [(160, 32, 7, 4, 3), (144, 64, 15, 4, 8), (100, 40, 9, 4, 3), (1296, 64, 16, 4, 1)],
                         ids=lambda c: "n%d_Kmax%d" % c[:2])
def test_flush_rounding_isolation_determinism(case):
    n, Kmax, Kd, Kmul, nb = case
    outs = []
    for _ in range(2):
        ar, ins, K = _flush_case(n, Kmax, Kd, Kmul, nb, data="rand", seed=1, nan_chain=1 if nb > 1 else None)
        P.run_flush(ar, n, Kmax, "Kdev", Kmul)
        outs.append([ar.get("G", b) for b in range(nb)])
    for b in range(nb):
        if b == 1 and nb > 1:
            continue
        assert np.array_equal(outs[0][b], outs[1][b])
        X, Y, G = ins[b]
        ref, rerr = P.matmul_ref(X, Y.T)
        P.check_elementwise(outs[0][b], ref + G, P.elementwise_bound(X, Y.T, extra=1) + P.U * np.abs(G), rerr, "flush chain %d" % b)
    ar1, _, _ = _flush_case(n, Kmax, Kd, Kmul, 1, data="rand", seed=1)
    P.run_flush(ar1, n, Kmax, "Kdev", Kmul)
    assert np.array_equal(ar1.get("G", 0), outs[0][0]), "chain 0 alone differs from chain 0 of the batch"


# ------------------------------------------------------------------------------------------------------------------------------
# LU
# ------------------------------------------------------------------------------------------------------------------------------
def _lu_run(mats):
    n = mats[0].shape[0]
    ar = P.lu_arena(len(mats), n)
    for b, A in enumerate(mats):
        ar.set("A", A, b)
    rc, msg = P.run_lu(ar, n)
    assert rc >= 0, msg
    return [(ar.get("A", b), ar.get("perm", b)) for b in range(len(mats))]


def _lu_check(A, LU, perm):
    n = A.shape[0]
    L = np.tril(LU, -1) + np.eye(n)
    Uu = np.triu(LU)
    assert sorted(perm.tolist()) == list(range(n))
    assert np.max(np.abs(np.tril(LU, -1))) <= 1 + 2.0 ** -40, "a multiplier exceeds 1: not partial pivoting"
    res = np.abs(A[perm] - L @ Uu)
    bound = 8 * n * P.U * (P.abs1(L) @ P.abs1(Uu))
    assert np.all(res <= bound), "backward error: max ratio %.2f" % np.max(res / bound)


@pytest.mark.parametrize("n", [32, 33, 64, 65, 100, 200, 256, 257, 511, 512])
def test_lu(n):
    rng = np.random.default_rng(n)
    mats = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(2)]
    outs = _lu_run(mats)
    for A, (LU, perm) in zip(mats, outs):
        _lu_check(A, LU, perm)
        pref, _ = P.lu_partial_pivot(A)
        assert np.array_equal(perm, pref), "permutation differs from plain partial pivoting"
    assert np.array_equal(_lu_run(mats[:1])[0][0], outs[0][0]), "chain 0 alone differs from chain 0 of the batch"


def test_lu_limit():
    ar = P.lu_arena(1, 513)
    ar.set("A", np.eye(513))
    rc, _ = P.run_lu(ar, 513)
    assert rc == -1


def test_lu_nan_row_skipped():
    """a row of NaN is never chosen as a pivot (its key is dropped): it ends in the last place, the other rows factor as usual"""
    n, r = 100, 37
    rng = np.random.default_rng(1)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A[r] = np.nan
    LU, perm = _lu_run([A])[0]
    assert perm[-1] == r
    L = np.tril(LU, -1)[: n - 1, : n - 1] + np.eye(n - 1)
    Uu = np.triu(LU)[: n - 1]
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(Uu))
    res = np.abs(A[perm[: n - 1]] - L @ Uu)
    assert np.all(res <= 8 * n * P.U * (P.abs1(L) @ P.abs1(Uu)))


@pytest.mark.parametrize("k", [-600, -300, 300, 600])
@pytest.mark.parametrize("n", [100, 300])
def test_lu_scale_invariance(n, k):
    """LU of 2^k A: the same pivots, the same L and 2^k U bit for bit -- also where |a|^2 leaves the normal range (|k| = 600)"""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    (LU0, p0), (LU1, p1) = _lu_run([A, np.ldexp(A.real, k) + 1j * np.ldexp(A.imag, k)])
    assert np.array_equal(p0, p1), "pivots of 2^%d A differ" % k
    assert np.array_equal(np.tril(LU1, -1), np.tril(LU0, -1))
    U0 = np.triu(LU0)
    assert np.array_equal(np.triu(LU1), np.ldexp(U0.real, k) + 1j * np.ldexp(U0.imag, k))


def test_lu_isolation_determinism():
    n = 200
    rng = np.random.default_rng(4)
    mats = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(3)]
    bad = np.full((n, n), np.nan, complex)
    r1 = _lu_run([mats[0], bad, mats[2]])
    r2 = _lu_run([mats[0], bad, mats[2]])
    alone = _lu_run([mats[0]])
    for b in (0, 2):
        assert np.array_equal(r1[b][0], r2[b][0]) and np.array_equal(r1[b][1], r2[b][1])
    assert np.array_equal(r1[0][0], alone[0][0]) and np.array_equal(r1[0][1], alone[0][1])


# ------------------------------------------------------------------------------------------------------------------------------
# triangular solve  C <- C R^-1
# ------------------------------------------------------------------------------------------------------------------------------
def _trsm_run(Rs, Cs, trans, unit):
    """Rs: the upper triangular matrices; stored as given (trans = 0) or as the lower triangle R^H (trans = 1).  Everything the solve
    must not read (the other triangle, a unit diagonal) is NaN."""
    n = Rs[0].shape[0]
    ar = Arena(len(Rs))
    ar.mat("R", n, n)
    ar.mat("C", n, n, kind="out")
    ar.layout()
    for b, (R, C) in enumerate(zip(Rs, Cs)):
        S = R.conj().T.copy() if trans else R.copy()
        mask = np.tril(np.ones((n, n), bool), -1) if not trans else np.triu(np.ones((n, n), bool), 1)
        S[mask] = np.nan
        if unit:
            np.fill_diagonal(S, np.nan)
        ar.set("R", S, b)
        ar.set("C", C, b)
    P.run_trsm(ar, n, trans, unit)
    return [ar.get("C", b) for b in range(len(Rs))]


def _int_upper(rng, n, unit, diag_exp=(0, 2)):
    R = np.triu(P.int_matrix(rng, n, n, -3, 3), 1)
    d = rng.choice([-1, 1], n) * 2.0 ** rng.integers(diag_exp[0], diag_exp[1] + 1, n)
    np.fill_diagonal(R, 1.0 if unit else d)
    return R


@pytest.mark.parametrize("n", [20, 45, 100, 200, 257])
@pytest.mark.parametrize("trans,unit", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_trsm_exact(n, trans, unit):
    """Y R = C with integer Y, R (diagonal +-1, +-2, +-4) and C = Y R: the solve is exact, Y comes back bit for bit.  n = 20 .. 257:
    no split up to four levels of the recursive halving"""
    rng = np.random.default_rng(n + 2 * trans + unit)
    R = _int_upper(rng, n, unit)
    Y = P.int_matrix(rng, n, n, -2, 2)
    C = P.exact_matmul(Y, R)
    got = _trsm_run([R, R], [C, C], trans, unit)
    for g in got:
        assert np.array_equal(g, Y), "max |err| %.3e" % np.max(np.abs(g - Y))


@pytest.mark.parametrize("n", [45, 200])
@pytest.mark.parametrize("trans,unit", [(0, 0), (1, 0), (0, 1)])
def test_trsm_rounding(n, trans, unit):
    """random R with a dominant diagonal: componentwise residual |Y R - C| <= c n u |Y| |R| (backward stable substitution)"""
    rng = np.random.default_rng(n)
    R = np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    np.fill_diagonal(R, 1.0 if unit else (2 + rng.random(n)) * np.exp(1j * rng.uniform(0, 6, n)))
    C = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    Y = _trsm_run([R], [C], trans, unit)[0]
    res = np.abs((Y.astype(np.clongdouble) @ R.astype(np.clongdouble) - C).astype(complex))
    assert np.all(res <= 8 * (n + 2) * P.U * (P.abs1(Y) @ P.abs1(R)) + 4 * P.U * np.abs(C))


def test_trsm_graded_diagonal():
    """diagonal +-2^e with e from -700 to 700 (|r_jj|^2 far outside the normal range): C R^-1 = C diag(r)^-1 exactly"""
    n = 90
    rng = np.random.default_rng(2)
    e = np.round(np.linspace(-700, 700, n)).astype(int)
    d = rng.choice([-1, 1], n) * np.ldexp(1.0, e)
    R = np.diag(d).astype(complex)
    C = P.int_matrix(rng, n, n)
    for trans in (0, 1):
        Y = _trsm_run([R], [C], trans, 0)[0]
        assert np.array_equal(Y, C / d[None, :]), "trans %d" % trans


@pytest.mark.parametrize("k", [-600, -300, 300, 600])
def test_trsm_scale_invariance(k):
    """C (2^k R)^-1 = 2^-k (C R^-1) bit for bit, random complex R (diagonal moduli outside [1e-154, 1e154] at |k| = 600)"""
    n = 100
    rng = np.random.default_rng(7)
    R = np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    np.fill_diagonal(R, (2 + rng.random(n)) * np.exp(1j * rng.uniform(0, 6, n)))
    C = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    Rk = np.ldexp(R.real, k) + 1j * np.ldexp(R.imag, k)
    for trans in (0, 1):
        Y0, Yk = _trsm_run([R, Rk], [C, C], trans, 0)
        assert np.array_equal(Yk, np.ldexp(Y0.real, -k) + 1j * np.ldexp(Y0.imag, -k)), "trans %d" % trans


def test_trsm_isolation_determinism():
    n = 100
    rng = np.random.default_rng(8)
    R = np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) + 3 * np.eye(n)
    C = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    bad = np.full((n, n), np.nan, complex)
    a = _trsm_run([R, bad, R], [C, bad, C], 0, 0)
    b = _trsm_run([R, bad, R], [C, bad, C], 0, 0)
    alone = _trsm_run([R], [C], 0, 0)[0]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[0], a[2])
    assert np.array_equal(a[0], alone)


# ------------------------------------------------------------------------------------------------------------------------------
# Householder QR (+ run_qr_apply_q) and block Gram-Schmidt QR
# ------------------------------------------------------------------------------------------------------------------------------
def _qr_checks(A, Q, R, tol, what):
    n = A.shape[0]
    assert np.all(np.tril(R, -1) == 0), "%s: R has a nonzero strict lower part" % what
    orth = np.linalg.norm(Q.conj().T @ Q - np.eye(n))
    assert orth <= tol * n, "%s: ||Q^H Q - I||_F = %.2e" % (what, orth)
    back = np.linalg.norm(A - Q @ R) / np.linalg.norm(A)
    assert back <= tol * n, "%s: ||A - QR|| / ||A|| = %.2e" % (what, back)


@pytest.mark.parametrize("n,nb", [(64, 1), (100, 2), (300, 2), (600, 1)])
def test_qr_householder(n, nb):
    rng = np.random.default_rng(n)
    mats = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(nb)]
    Cm = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    res = {}
    for trans in (0, 1):
        ar = P.qr_arena(nb, n, with_c=True)
        for b in range(nb):
            ar.set("A", mats[b], b)
            ar.set("C", Cm, b)
        P.run_qr(ar, n, apply_trans=trans)
        for b in range(nb):
            R, Q, C = ar.get("A", b), ar.get("Q", b), ar.get("C", b)
            _qr_checks(mats[b], Q, R, 1e-14, "Householder n=%d chain %d" % (n, b))
            ref = (Q.conj().T if trans else Q) @ Cm
            assert np.linalg.norm(C - ref) <= 1e-14 * n * np.linalg.norm(Cm), "apply_q trans %d" % trans
            res[(trans, b)] = (R, Q)
    assert np.array_equal(res[(0, 0)][0], res[(1, 0)][0]) and np.array_equal(res[(0, 0)][1], res[(1, 0)][1]), "not deterministic"
    ar = P.qr_arena(1, n)
    ar.set("A", mats[0])
    P.run_qr(ar, n)
    assert np.array_equal(ar.get("A"), res[(0, 0)][0]) and np.array_equal(ar.get("Q"), res[(0, 0)][1]), "chain 0 alone differs"


def _bgs(mats, part=True):
    n = mats[0].shape[0]
    ar = P.bgs_arena(len(mats), n, part_count=n * 64 * 8 if (part and n > 1024) else None)
    for b, A in enumerate(mats):
        ar.set("A", A, b)
    P.run_qr_bgs(ar, n)
    return [(ar.get("A", b), ar.get("Q", b), int(ar.get("err", b)[0])) for b in range(len(mats))]


def _well_conditioned(rng, n):
    """U diag(s) V^H with kappa = 100, columns then graded over three decades like pre-pivoted chain matrices (Gram-Schmidt and
    Cholesky-QR are invariant under column scaling)"""
    Qx, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    Qy, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return ((Qx * 10.0 ** np.linspace(0, -2, n)[None, :]) @ Qy.conj().T) * 10.0 ** np.linspace(0, -3, n)[None, :]


@pytest.mark.parametrize("n,nb", [(64, 1), (100, 2), (100, 8), (1040, 1), (1100, 2)])
def test_qr_bgs(n, nb):
    rng = np.random.default_rng(n + nb)
    mats = [_well_conditioned(rng, n) for _ in range(nb)]
    out = _bgs(mats)
    for b, (R, Q, err) in enumerate(out):
        assert err == 0
        _qr_checks(mats[b], Q, R, 1e-14, "BGS n=%d chain %d" % (n, b))
    again = _bgs(mats)
    for b in range(nb):
        assert np.array_equal(again[b][0], out[b][0]) and np.array_equal(again[b][1], out[b][1]), "not deterministic"
    if nb > 1 and n <= 1024:
        # no split-K below n = 1025: the products take the same branch for any nb, chain 0 alone is bit-identical.  (Above it the
        # split factor of the skinny products falls with nb -- a different summation order, no such promise.)
        alone = _bgs(mats[:1])[0]
        assert np.array_equal(alone[0], out[0][0]) and np.array_equal(alone[1], out[0][1])


def test_qr_bgs_chol_fail_flag():
    """the per-chain flag is set for exactly the chains whose input is rank-deficient inside a 64-column block (the Cholesky pivot
    test is relative to each column's norm after the projection on the earlier blocks: a column that depends on earlier blocks
    only leaves rounding noise behind, which passes it -- the resulting R has a tiny diagonal entry, as with Householder)"""
    n = 100
    rng = np.random.default_rng(9)
    mats = [_well_conditioned(rng, n) for _ in range(4)]
    mats[1][:, 90] = (1 + 1j) * mats[1][:, 70]              # rank-deficient: second (partial) block
    mats[3][:, 10] = 2 * mats[3][:, 5]                      # rank-deficient: first block
    out = _bgs(mats)
    assert [o[2] for o in out] == [0, 1, 0, 1]
    for b in (0, 2):
        _qr_checks(mats[b], out[b][1], out[b][0], 1e-14, "healthy chain %d next to failing ones" % b)
