"""ctypes driver of the test-only launcher entry points (detqmc_amd/lib/libdqmc_primitives_test.so) plus the references and error
bounds the primitive tests compare against.

An Arena holds the operands of nb chains at a chain stride cs bytes, laid out like the product's device arenas.  Every byte that is
not an operand is a NaN SENTINEL (slack rows below a matrix, the gap between chains, columns beyond what a kernel may read), and so are
the operand regions of chains that do not use them (a shared operand lives in chain 0 only).  After a launch Arena.check() asserts that
nothing outside the declared outputs and scratch regions changed: a write out of bounds stays inside the allocation and shows up as an
assertion naming the region and chain, not as a fault."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "detqmc_amd", "lib", "libdqmc_primitives_test.so")
SYMBOLS = ("dqmc_prim_gemm", "dqmc_prim_gemm_plan", "dqmc_prim_flush", "dqmc_prim_lu", "dqmc_prim_trsm", "dqmc_prim_qr",
           "dqmc_prim_qr_bgs")
SENTINEL = 0x7FF4DEADBEEF0001            # a quiet-bit-clear NaN payload that no arithmetic produces
U = 2.0 ** -53                           # unit roundoff of fp64
LU_SWAP_INTS = 128
QR_NB = 16


class PrimGemm(ctypes.Structure):
    _fields_ = [(f, ctypes.c_longlong) for f in (
        "A", "lda", "opA", "B", "ldb", "opB", "C", "ldc", "M", "N", "K",
        "Kdev", "Kmul", "kscale", "kscale_invert", "rowscale", "colscale",
        "accumulate", "negate", "sharedA", "sharedB", "a_kgather", "b_lower", "part", "part_count", "tag")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(LIB_PATH)
        vp, sz, i, ll, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p
        _lib.dqmc_prim_gemm_plan.argtypes = [ctypes.POINTER(PrimGemm), i, ctypes.POINTER(ctypes.c_int)]
        _lib.dqmc_prim_gemm.argtypes = [vp, sz, i, sz, ctypes.POINTER(PrimGemm), cp, i]
        _lib.dqmc_prim_flush.argtypes = [vp, sz, i, sz, ll, ll, i, ll, i, i, i, ll, i, i, cp, i]
        _lib.dqmc_prim_lu.argtypes = [vp, sz, i, sz, i, ll, ll, ll, ll, cp, i]
        _lib.dqmc_prim_trsm.argtypes = [vp, sz, i, sz, i, ll, ll, i, i, cp, i]
        _lib.dqmc_prim_qr.argtypes = [vp, sz, i, sz, i, ll, ll, ll, ll, ll, i, cp, i]
        _lib.dqmc_prim_qr_bgs.argtypes = [vp, sz, i, sz, i, ll, ll, ll, ll, ll, ll, cp, i]
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------
# arena
# ------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """Operands are declared first (mat / vec), then the arena is laid out on first use.  kind: 'in' (must come back unchanged),
    'out' (the rows x cols part may change, slack rows may not), 'scratch' (anything may change).  shared: chain 0 only."""

    def __init__(self, nb, gap=4096):
        self.nb, self.gap = nb, gap
        self.ops = {}
        self.size = 0
        self.buf = None

    def _add(self, name, nbytes, **kw):
        off = self.size
        self.size = (off + nbytes + 255) // 256 * 256
        self.ops[name] = dict(off=off, nbytes=nbytes, **kw)
        return name

    def mat(self, name, rows, cols, ld=None, kind="in", shared=False):
        """column-major complex rows x cols matrix with leading dimension ld (slack rows ld - rows stay sentinels)"""
        ld = rows if ld is None else ld
        assert ld >= max(rows, 1)
        return self._add(name, 16 * ld * max(cols, 1), rows=rows, cols=cols, ld=ld, dtype=np.complex128, kind=kind, shared=shared)

    def vec(self, name, count, dtype, kind="in", shared=False):
        dtype = np.dtype(dtype)
        return self._add(name, dtype.itemsize * max(count, 1), rows=count, cols=1, ld=count, dtype=dtype, kind=kind, shared=shared)

    def layout(self):
        if self.buf is None:
            self.cs = (self.size + self.gap + 255) // 256 * 256
            self.buf = np.full(self.nb * self.cs // 8, SENTINEL, dtype=np.uint64)
        return self

    def off(self, name):
        return self.ops[name]["off"] if name is not None else -1

    def _raw(self, name, chain):
        o = self.ops[name]
        start = chain * self.cs + o["off"]
        return self.buf.view(np.uint8)[start:start + o["nbytes"]]

    def _view(self, name, chain):
        o = self.ops[name]
        a = self._raw(name, chain).view(o["dtype"])
        if o["dtype"] == np.complex128:
            return a.reshape(max(o["cols"], 1), o["ld"]).T[:o["rows"], :o["cols"]]
        return a[:o["rows"]]

    def set(self, name, value, chain=0):
        self.layout()
        v = self._view(name, chain)
        v[...] = np.asarray(value).reshape(v.shape)

    def get(self, name, chain=0):
        return self._view(name, chain).copy()

    def fill(self, name, value, chain=0):
        """the whole region (slack included) set to value: workspaces the launcher expects zeroed"""
        self.layout()
        o = self.ops[name]
        self._raw(name, chain).view(o["dtype"])[...] = value

    def snapshot(self):
        self._before = self.buf.copy()

    def check(self):
        """every byte outside the outputs' rows x cols parts and the scratch regions is what it was before the launch"""
        before = self._before.view(np.uint8)
        after = self.buf.view(np.uint8)
        allowed = np.zeros(after.size, dtype=bool)
        for name, o in self.ops.items():
            if o["kind"] == "in":
                continue
            for b in range(1 if o["shared"] else self.nb):
                start = b * self.cs + o["off"]
                if o["kind"] == "scratch":
                    allowed[start:start + o["nbytes"]] = True
                else:
                    isz = np.dtype(o["dtype"]).itemsize
                    for j in range(max(o["cols"], 1)):
                        s = start + j * o["ld"] * isz
                        allowed[s:s + o["rows"] * isz] = True
        bad = np.nonzero((before != after) & ~allowed)[0]
        if bad.size:
            raise AssertionError("sentinel or input overwritten: " + self.locate(int(bad[0])) + " (%d bytes in all)" % bad.size)

    def locate(self, byte):
        chain, rel = divmod(byte, self.cs)
        for name, o in self.ops.items():
            if o["off"] <= rel < o["off"] + o["nbytes"]:
                return "chain %d, operand %s, byte %d of it" % (chain, name, rel - o["off"])
        return "chain %d, byte %d (gap between operands / chains)" % (chain, rel)

    def call(self, fn, *args):
        self.layout()
        self.snapshot()
        msg = ctypes.create_string_buffer(256)
        rc = getattr(lib(), fn)(self.buf.ctypes.data_as(ctypes.c_void_p), self.buf.nbytes, self.nb, self.cs, *args, msg, 256)
        return rc, msg.value.decode()


# ------------------------------------------------------------------------------------------------------------------------------
# launchers
# ------------------------------------------------------------------------------------------------------------------------------
def gemm_spec(ar, **kw):
    """PrimGemm from operand names (A, B, C, Kdev, kscale, rowscale, colscale, a_kgather, part) and scalars"""
    s = PrimGemm()
    for f, _ in PrimGemm._fields_:
        setattr(s, f, -1 if f in ("A", "B", "C", "Kdev", "kscale", "rowscale", "colscale", "a_kgather", "part") else 0)
    s.Kmul = 1
    for k, v in kw.items():
        if k in ("A", "B", "C", "Kdev", "kscale", "rowscale", "colscale", "a_kgather", "part"):
            setattr(s, k, ar.off(v) if v is not None else -1)
        else:
            setattr(s, k, int(v))
    for k in ("A", "B", "C"):
        name = kw.get(k)
        setattr(s, "ld" + k.lower(), kw.get("ld" + k.lower(), ar.ops[name]["ld"]))
    return s


def gemm_plan(spec, nb):
    out = (ctypes.c_int * 3)()
    lib().dqmc_prim_gemm_plan(ctypes.byref(spec), nb, out)
    return dict(tile=out[0], ksplit=out[1], xcd=out[2])


def run_gemm(ar, spec):
    rc, msg = ar.call("dqmc_prim_gemm", ctypes.byref(spec))
    assert rc == 0, msg
    ar.check()


def run_flush(ar, n, Kmax, Kdev=None, Kmul=1, tag=0):
    ld = ar.ops["X"]["ld"]
    rc, msg = ar.call("dqmc_prim_flush", ar.off("X"), ar.off("GrT"), ld, ar.off("G"), ar.ops["G"]["ld"], n, Kmax, ar.off(Kdev), Kmul, tag)
    assert rc == 0, msg
    ar.check()


def run_lu(ar, n):
    rc, msg = ar.call("dqmc_prim_lu", n, ar.off("A"), ar.off("perm"), ar.off("swaps"), ar.off("tneg"))
    if rc == 0:
        ar.check()
    return rc, msg


def lu_arena(nb, n, gap=4096):
    ar = Arena(nb, gap)
    ar.mat("A", n, n, kind="out")
    ar.vec("perm", n, np.int32, kind="out")
    ar.vec("swaps", LU_SWAP_INTS, np.int32, kind="scratch")
    ar.mat("tneg", n, 32, kind="scratch")
    return ar.layout()


def run_trsm(ar, n, trans=0, unit=0):
    rc, msg = ar.call("dqmc_prim_trsm", n, ar.off("R"), ar.off("C"), trans, unit)
    assert rc >= 0, msg
    ar.check()


def qr_arena(nb, n, with_c=False):
    ar = Arena(nb)
    ar.mat("A", n, n, kind="out")
    ar.mat("Q", n, n, kind="out")
    ar.mat("V", n, n, kind="scratch")
    ar.vec("T", ((n + QR_NB - 1) // QR_NB) * 2 * QR_NB * QR_NB, np.complex128, kind="scratch")
    if with_c:
        ar.mat("C", n, n, kind="out")
    ar.layout()
    for b in range(nb):
        ar.fill("V", 0, b)
        ar.fill("T", 0, b)
    return ar


def run_qr(ar, n, apply_trans=-1):
    rc, msg = ar.call("dqmc_prim_qr", n, ar.off("A"), ar.off("Q"), ar.off("V"), ar.off("T"),
                      ar.off("C") if apply_trans >= 0 else -1, max(apply_trans, 0))
    assert rc >= 0, msg
    ar.check()


def bgs_arena(nb, n, part_count=None):
    ar = Arena(nb)
    ar.mat("A", n, n, kind="out")
    ar.mat("Q", n, n, kind="out")
    ar.mat("V", n, n, kind="scratch")
    if part_count:
        ar.vec("part", part_count, np.complex128, kind="scratch")
    ar.vec("err", 1, np.int32, kind="out")
    ar.layout()
    for b in range(nb):
        ar.set("err", [0], b)
    return ar


def run_qr_bgs(ar, n):
    pc = ar.ops["part"]["rows"] if "part" in ar.ops else 0
    rc, msg = ar.call("dqmc_prim_qr_bgs", n, ar.off("A"), ar.off("Q"), ar.off("V"), ar.off("part") if pc else -1, pc, ar.off("err"))
    assert rc >= 0, msg
    ar.check()


# ------------------------------------------------------------------------------------------------------------------------------
# references and bounds
# ------------------------------------------------------------------------------------------------------------------------------
def op(X, o):
    return X.conj().T if o else X


def abs1(X):
    """|re| + |im| elementwise (the 1-norm of a complex number seen as a real pair)"""
    X = np.asarray(X)
    return np.abs(X.real) + np.abs(X.imag)


def matmul_ref(A, B):
    """A B and the error bound of that reference itself: exact enough in long double (64-bit mantissa) when the size allows it,
    float64 plus its own rounding bound (2 K u |A|_1 |B|_1) otherwise"""
    M, K = A.shape
    N = B.shape[1]
    if M * N * K <= 2 ** 24:
        ref = A.astype(np.clongdouble) @ B.astype(np.clongdouble)
        return ref.astype(np.complex128), np.zeros((M, N))
    return A @ B, 2.0 * (K + 2) * U * (abs1(A) @ abs1(B))


def elementwise_bound(A, B, extra=0, c=4.0):
    """componentwise rounding bound of a complex product computed with fp64 multiply-adds in any order, 3M (Karatsuba) or 4M:
    |C - C_exact|_ij <= c (K + extra) u sum_k |a_ik|_1 |b_kj|_1.  c = 4: the 3M imaginary part P3 - P1 - P2 carries the rounding of
    three real sums and of the two operand sums (a_r + a_i), (b_r + b_i); extra: further additions per entry (split-K slices,
    accumulation into C)."""
    K = A.shape[1]
    return c * (K + extra + 2) * U * (abs1(A) @ abs1(B))


def check_elementwise(got, ref, bound, ref_err=None, what=""):
    err = np.abs(got - ref)
    lim = bound + (ref_err if ref_err is not None else 0.0) + np.abs(ref) * U
    bad = ~(err <= lim)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: elementwise bound exceeded at (%d, %d): |err| = %.3e > %.3e (%d entries)"
                             % (what, i, j, err[i, j], lim[i, j], int(bad.sum())))


def int_matrix(rng, rows, cols, lo=-4, hi=4):
    return (rng.integers(lo, hi + 1, (rows, cols)) + 1j * rng.integers(lo, hi + 1, (rows, cols))).astype(np.complex128)


def exact_matmul(A, B):
    """product of complex matrices with integer (or dyadic, after scaling) entries in exact int64 arithmetic"""
    ar, ai = A.real.astype(np.int64), A.imag.astype(np.int64)
    br, bi = B.real.astype(np.int64), B.imag.astype(np.int64)
    assert np.array_equal(ar, A.real) and np.array_equal(ai, A.imag) and np.array_equal(br, B.real) and np.array_equal(bi, B.imag)
    return (ar @ br - ai @ bi).astype(np.float64) + 1j * (ar @ bi + ai @ br).astype(np.float64)


def lu_partial_pivot(A):
    """straightforward partial-pivoting LU (largest |a|^2, first index on ties): perm with P A = L U, and L \\ U in one matrix"""
    A = np.array(A, dtype=np.complex128)
    n = A.shape[0]
    perm = np.arange(n)
    for c in range(n):
        m = np.abs(A[c:, c]) ** 2
        p = c + int(np.argmax(m))
        if p != c:
            A[[c, p]] = A[[p, c]]
            perm[[c, p]] = perm[[p, c]]
        if A[c, c] != 0:
            A[c + 1:, c] /= A[c, c]
            A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c, c + 1:])
    return perm, A
