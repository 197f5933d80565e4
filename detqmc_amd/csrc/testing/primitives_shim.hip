// Test-only entry points into the internal launchers of libdetqmc_amd.so (tests/primitives.py, tests/test_gpu_primitives.py).
//
// Host code only: every function copies a caller-owned host ARENA to the device, runs ONE launcher on it with Launch{stream, nb, cs}
// (chain b's operands at b * cs bytes past chain 0's), synchronises, checks the HIP status and copies the whole arena back.  Operand
// positions are BYTE offsets into chain 0's part of the arena (-1: null pointer).  The launchers are the ones the product runs, linked
// from libdetqmc_amd.so, not a second copy.  Return value: 0, or a negative code with a message in msg.
#include "../dqmc_internal.h"
#include <stdio.h>
#include <string.h>

extern "C" {

// GEMM arguments (GemmArgs) as 64-bit integers; pointer fields are byte offsets (-1: null)
struct PrimGemm {
    long long A, lda, opA, B, ldb, opB, C, ldc, M, N, K;
    long long Kdev, Kmul, kscale, kscale_invert, rowscale, colscale;
    long long accumulate, negate, sharedA, sharedB, a_kgather, b_lower, part, part_count, tag;
};

}  // extern "C"

namespace {

template<class T> T* at(void* base, long long off) { return off < 0 ? nullptr : (T*)((char*)base + off); }

GemmArgs gemm_args(void* d, const PrimGemm& p) {
    GemmArgs g = GemmArgs();
    g.A = at<const cplx>(d, p.A); g.lda = (int)p.lda; g.opA = (int)p.opA;
    g.B = at<const cplx>(d, p.B); g.ldb = (int)p.ldb; g.opB = (int)p.opB;
    g.C = at<cplx>(d, p.C); g.ldc = (int)p.ldc;
    g.M = (int)p.M; g.N = (int)p.N; g.K = (int)p.K;
    g.Kdev = at<const int>(d, p.Kdev); g.Kmul = (int)p.Kmul;
    g.kscale = at<const double>(d, p.kscale); g.kscale_invert = (int)p.kscale_invert;
    g.rowscale = at<const double>(d, p.rowscale); g.colscale = at<const double>(d, p.colscale);
    g.accumulate = (int)p.accumulate; g.negate = (int)p.negate;
    g.sharedA = (int)p.sharedA; g.sharedB = (int)p.sharedB;
    g.a_kgather = at<const int>(d, p.a_kgather); g.b_lower = (int)p.b_lower;
    g.part = at<cplx>(d, p.part); g.part_count = (size_t)p.part_count;
    g.tag = (int)p.tag;
    return g;
}

int fail(char* msg, int msglen, int code, const char* what, hipError_t e) {
    if (msg && msglen > 0) snprintf(msg, (size_t)msglen, "%s: %s", what, e == hipSuccess ? "error" : hipGetErrorString(e));
    return code;
}

// arena in, fn(device arena, launch) -> int (>= 0 ok), arena out
template<class F>
int with_arena(void* host, size_t bytes, int nb, size_t cs, char* msg, int msglen, F fn) {
    if (msg && msglen > 0) msg[0] = 0;
    if (nb < 1 || (size_t)nb * cs > bytes) return fail(msg, msglen, -2, "arena smaller than nb * cs", hipSuccess);
    void* d = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return fail(msg, msglen, -3, "hipMalloc", e);
    int rc = 0;
    if ((e = hipStreamCreate(&st)) != hipSuccess) rc = fail(msg, msglen, -3, "hipStreamCreate", e);
    else if ((e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) != hipSuccess) rc = fail(msg, msglen, -3, "copy in", e);
    else {
        Launch lc;
        lc.st = st; lc.nb = nb; lc.cs = cs;
        const int r = fn(d, lc);
        if ((e = hipGetLastError()) != hipSuccess) rc = fail(msg, msglen, -4, "launch", e);
        else if ((e = hipStreamSynchronize(st)) != hipSuccess) rc = fail(msg, msglen, -4, "kernel", e);
        else if ((e = hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail(msg, msglen, -3, "copy out", e);
        else if (r < 0) rc = fail(msg, msglen, r, "launcher refused the arguments", hipSuccess);
    }
    if (st) (void)hipStreamDestroy(st);
    (void)hipFree(d);
    return rc;
}

}  // namespace

extern "C" {

// the branch launch_gemm takes for these arguments: out[0] tile (32 / 64), out[1] split-K slices (1: none), out[2] XCD-grouped grid
int dqmc_prim_gemm_plan(const PrimGemm* p, int nb, int* out) {
    // only the null-ness of the pointer fields matters to the plan: any non-null stand-in will do
    const GemmPlan g = gemm_plan(gemm_args((void*)16, *p), nb);
    out[0] = g.tile; out[1] = g.ksplit; out[2] = g.xcd;
    return 0;
}

int dqmc_prim_gemm(void* arena, size_t bytes, int nb, size_t cs, const PrimGemm* p, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        launch_gemm(lc, gemm_args(d, *p));
        return 0;
    });
}

// dqmc_prim_gemm with the kernel path forced: path 0 the generic kernel, 1 the whole-tile kernel where the arguments allow it, -1 as
// launch_gemm decides.  *ran: the path that ran (0 generic, 1 whole-tile)
int dqmc_prim_gemm_path(void* arena, size_t bytes, int nb, size_t cs, const PrimGemm* p, int path, int* ran, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        *ran = launch_gemm_path(lc, gemm_args(d, *p), path);
        return 0;
    });
}

// G += X GrT^T, K = min(Kmax, *Kdev * Kmul) (Kdev < 0: Kmax)
int dqmc_prim_flush(void* arena, size_t bytes, int nb, size_t cs, long long X, long long GrT, int ld, long long G, int ldc, int n,
                    int Kmax, long long Kdev, int Kmul, int tag, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        launch_flush(lc, at<const cplx>(d, X), at<const cplx>(d, GrT), ld, at<cplx>(d, G), ldc, n, Kmax, at<const int>(d, Kdev), Kmul, tag);
        return 0;
    });
}

// P A = L U in place (A n x n, ld n); perm: n ints, swaps: LU_SWAP_INTS ints, tneg: n * 32 complex (all per chain)
int dqmc_prim_lu(void* arena, size_t bytes, int nb, size_t cs, int n, long long A, long long perm, long long swaps, long long tneg,
                 char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        return run_lu(lc, n, at<cplx>(d, A), at<int>(d, perm), at<int>(d, swaps), at<cplx>(d, tneg));
    });
}

// C <- C R^-1 (R, C n x n, ld n; trans: R = (stored lower triangle)^H; unit: unit diagonal)
int dqmc_prim_trsm(void* arena, size_t bytes, int nb, size_t cs, int n, long long R, long long C, int trans, int unit,
                   char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        QrWork w = QrWork();
        return run_trsm_right_upper(lc, n, at<const cplx>(d, R), at<cplx>(d, C), w, trans, unit);
    });
}

// C <- S R^-1 with the right-hand side S = columns of X (n x n, ld n), scaled and gathered: idx n ints (< 0: none), scale n doubles (< 0:
// none).  how 0: k_gather_scale_cols writes S into C (S[:, j] = X[:, idx[j]] scale[idx[j]]; idx required), then the solve in place;
// how 1: k_permute_scale_cols (S[:, idx[j]] = X[:, j] scale[j]), then the solve in place; how 2: no copy -- the solve reads S through its
// first-touch column source, gather form (ColSrc), and only writes C
int dqmc_prim_trsm_src(void* arena, size_t bytes, int nb, size_t cs, int n, long long R, long long C, int trans, int unit,
                       long long X, long long idx, long long scale, int how, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        QrWork w = QrWork();
        const cplx* x = at<const cplx>(d, X);
        const int* ix = at<const int>(d, idx);
        const double* sc = at<const double>(d, scale);
        if (how == 2) {
            const ColSrc src = {x, n, ix, sc};
            return run_trsm_right_upper(lc, n, at<const cplx>(d, R), at<cplx>(d, C), w, trans, unit, &src);
        }
        if (how == 0) { if (!ix) return -2; launch_gather_scale_cols(lc, x, sc, ix, n, at<cplx>(d, C)); }
        else launch_permute_scale_cols(lc, x, sc, ix, n, at<cplx>(d, C));
        return run_trsm_right_upper(lc, n, at<const cplx>(d, R), at<cplx>(d, C), w, trans, unit);
    });
}

// Householder QR: A -> R in place, Q explicit (Q < 0: reflectors only); V (n * n) and T (ceil(n / 16) * 512 complex) zero on entry.
// C >= 0: afterwards C <- Q C (apply_trans 0) or Q^H C (1) from the reflectors (run_qr_apply_q).
int dqmc_prim_qr(void* arena, size_t bytes, int nb, size_t cs, int n, long long A, long long Q, long long V, long long T,
                 long long C, int apply_trans, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        QrWork w = QrWork();
        w.V = at<cplx>(d, V); w.T = at<cplx>(d, T);
        int r = run_qr(lc, n, at<cplx>(d, A), at<cplx>(d, Q), w);
        if (r >= 0 && C >= 0) r = run_qr_apply_q(lc, n, at<cplx>(d, C), w, apply_trans);
        return r;
    });
}

// block Gram-Schmidt QR: A -> R, Q explicit; V: n * n scratch; part: split-K scratch of part_count complex (< 0: none); err: one int
int dqmc_prim_qr_bgs(void* arena, size_t bytes, int nb, size_t cs, int n, long long A, long long Q, long long V, long long part,
                     long long part_count, long long err, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        QrWork w = QrWork();
        w.V = at<cplx>(d, V); w.part = at<cplx>(d, part); w.part_count = part < 0 ? 0 : (size_t)part_count; w.err = at<int>(d, err);
        return run_qr_bgs(lc, n, at<cplx>(d, A), at<cplx>(d, Q), w);
    });
}

// wrap-error compare (launch_green_diff): Gw against Gf, both n x n at leading dimension ld; N: sites (the site diagonal is row mod N ==
// col mod N); part: green_diff_partial_doubles(n) = 6 ceil(n^2 / 2048) doubles of scratch, out: 6 doubles (maxAbs, argmax, maxSiteDiag,
// sumAbs, maxFresh, nonfinite), all per chain at the chain stride
int dqmc_prim_green_diff(void* arena, size_t bytes, int nb, size_t cs, long long Gw, long long Gf, long long part, long long out,
                         int n, int ld, int N, char* msg, int msglen) {
    return with_arena(arena, bytes, nb, cs, msg, msglen, [&](void* d, const Launch& lc) {
        if (n < 1 || ld < n || N < 1 || Gw < 0 || Gf < 0 || part < 0 || out < 0) return -2;
        launch_green_diff(lc, at<const cplx>(d, Gw), cs, at<const cplx>(d, Gf), n, ld, N, at<double>(d, part), cs, at<double>(d, out), cs);
        return 0;
    });
}

}  // extern "C"
