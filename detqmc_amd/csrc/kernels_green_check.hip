// Wrap-error diagnostics (dqmc_set_green_check; dqmc_hip.h and DESIGN.md): the Green's function carried by wraps and updates, Gw, against
// the one just rebuilt from the UdV factors, Gf, for all chains in one stream-ordered pass of two launches.
//
//   k_green_diff_partial   streams both matrices once.  The n x n entries are numbered column-major, e = row + col n; workgroup w takes
//                          entries [w GD_CHUNK, (w + 1) GD_CHUNK), consecutive lanes consecutive rows of a column (one 16-byte load per
//                          matrix and entry, coalesced down the columns).  Thread -> wave (cross-lane exchange) -> workgroup (LDS), then
//                          one record of GD_FIELDS doubles per workgroup in the partials buffer.
//   k_green_diff_finalise  one workgroup per chain folds the records in a fixed order, writes the six results and, in the context, the
//                          scale spreads of the factorisation the advance stored and the sample's row of the table.
//
// No atomics and no last-arriving-block fence: the kernel boundary orders the two steps, every reduction has a fixed shape, so the
// same inputs give the same bits.  An entry where either matrix is not finite counts in `nonfinite`, enters maxAbs as +inf (a plain
// fmax would drop a NaN) and stays out of the other four results.
#include "dqmc_internal.h"
#include <math.h>
#include <algorithm>

enum { GD_THREADS = 256, GD_PER_THREAD = 8, GD_CHUNK = GD_THREADS * GD_PER_THREAD, GD_FIELDS = 6 };

// mx: max |Gw - Gf| and idx the smallest entry number that attains it; site: the same maximum over row mod N == col mod N; sum: sum of
// |Gw - Gf|; fresh: max |Gf|; bad: entries with a non-finite value.  mx = -1: nothing seen yet
struct GdAcc { double mx, idx, site, sum, fresh, bad; };

__device__ __forceinline__ GdAcc gd_empty() { return GdAcc{-1.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ GdAcc gd_combine(const GdAcc& a, const GdAcc& b) {
    GdAcc r;
    const bool tb = b.mx > a.mx || (b.mx == a.mx && b.idx < a.idx);
    r.mx = tb ? b.mx : a.mx;
    r.idx = tb ? b.idx : a.idx;
    r.site = fmax(a.site, b.site);
    r.sum = a.sum + b.sum;
    r.fresh = fmax(a.fresh, b.fresh);
    r.bad = a.bad + b.bad;
    return r;
}
__device__ __forceinline__ GdAcc gd_shfl_xor(const GdAcc& a, int off) {
    return GdAcc{__shfl_xor(a.mx, off, 64), __shfl_xor(a.idx, off, 64), __shfl_xor(a.site, off, 64),
                 __shfl_xor(a.sum, off, 64), __shfl_xor(a.fresh, off, 64), __shfl_xor(a.bad, off, 64)};
}
// every thread of the workgroup ends with the same record; red: GD_THREADS / 64 records
__device__ __forceinline__ GdAcc gd_block_reduce(GdAcc a, GdAcc* red) {
    for (int off = 1; off < 64; off <<= 1) a = gd_combine(a, gd_shfl_xor(a, off));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = a;
    __syncthreads();
    GdAcc r = red[0];
    for (int w = 1; w < GD_THREADS / 64; ++w) r = gd_combine(r, red[w]);
    return r;
}
__device__ __forceinline__ bool gd_finite(const cplx& v) { return isfinite(v.x) && isfinite(v.y); }

__global__ __launch_bounds__(GD_THREADS) void k_green_diff_partial(const cplx* __restrict__ Gw, size_t gw_stride, const cplx* __restrict__ Gf,
                                                                   int n, int ld, int N, double* __restrict__ part, size_t part_stride, size_t cs) {
    __shared__ GdAcc red[GD_THREADS / 64];
    Gw = (const cplx*)((const char*)Gw + (size_t)blockIdx.z * gw_stride);
    part = (double*)((char*)part + (size_t)blockIdx.z * part_stride);
    CHAIN(Gf);
    const size_t total = (size_t)n * n, base = (size_t)blockIdx.x * GD_CHUNK + threadIdx.x;
    cplx w[GD_PER_THREAD], f[GD_PER_THREAD];
#pragma unroll
    for (int i = 0; i < GD_PER_THREAD; ++i) {
        const size_t e = base + (size_t)i * GD_THREADS;
        if (e < total) {
            const size_t col = e / n, a = col * ld + (e - col * n);
            w[i] = Gw[a]; f[i] = Gf[a];
        } else w[i] = f[i] = make_double2(0.0, 0.0);
    }
    GdAcc acc = gd_empty();
#pragma unroll
    for (int i = 0; i < GD_PER_THREAD; ++i) {
        const size_t e = base + (size_t)i * GD_THREADS;
        if (e >= total) continue;
        GdAcc v = gd_empty();
        v.idx = (double)e;
        if (gd_finite(w[i]) && gd_finite(f[i])) {
            const size_t col = e / n, row = e - col * n;
            const double dx = w[i].x - f[i].x, dy = w[i].y - f[i].y;
            v.mx = sqrt(dx * dx + dy * dy);
            v.sum = v.mx;
            if (row % N == col % N) v.site = v.mx;
            v.fresh = sqrt(f[i].x * f[i].x + f[i].y * f[i].y);
        } else {
            v.mx = INFINITY;
            v.bad = 1.0;
        }
        acc = gd_combine(acc, v);
    }
    acc = gd_block_reduce(acc, red);
    if (threadIdx.x == 0) {
        double* p = part + (size_t)blockIdx.x * GD_FIELDS;
        p[0] = acc.mx; p[1] = acc.idx; p[2] = acc.site; p[3] = acc.sum; p[4] = acc.fresh; p[5] = acc.bad;
    }
}

// log(max v / min v) (quotient != 0) or log(max v) - log(min v) of n positive values, the same number in every thread; red: GD_THREADS doubles
__device__ __forceinline__ double gd_log_spread(const double* __restrict__ v, int n, int quotient, double* red) {
    double hi = -INFINITY, lo = INFINITY;
    for (int i = threadIdx.x; i < n; i += GD_THREADS) { hi = fmax(hi, v[i]); lo = fmin(lo, v[i]); }
    for (int off = 1; off < 64; off <<= 1) { hi = fmax(hi, __shfl_xor(hi, off, 64)); lo = fmin(lo, __shfl_xor(lo, off, 64)); }
    __syncthreads();                                    // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = hi; red[GD_THREADS / 64 + (threadIdx.x >> 6)] = lo; }
    __syncthreads();
    for (int w = 0; w < GD_THREADS / 64; ++w) { hi = fmax(hi, red[w]); lo = fmin(lo, red[GD_THREADS / 64 + w]); }
    return quotient ? log(hi / lo) : log(hi) - log(lo);
}

__global__ __launch_bounds__(GD_THREADS) void k_green_diff_finalise(const double* __restrict__ part, size_t part_stride, int nparts, int n,
                                                                    double* __restrict__ out, size_t out_stride, double* __restrict__ table,
                                                                    size_t table_stride, int row, const double* __restrict__ d,
                                                                    const double* __restrict__ sv, size_t cs) {
    __shared__ GdAcc red[GD_THREADS / 64];
    __shared__ double redd[2 * (GD_THREADS / 64)];
    part = (const double*)((const char*)part + (size_t)blockIdx.z * part_stride);
    out = (double*)((char*)out + (size_t)blockIdx.z * out_stride);
    CHAIN(d); CHAIN(sv);
    GdAcc acc = gd_empty();
    for (int p = threadIdx.x; p < nparts; p += GD_THREADS) {
        const double* q = part + (size_t)p * GD_FIELDS;
        acc = gd_combine(acc, GdAcc{q[0], q[1], q[2], q[3], q[4], q[5]});
    }
    acc = gd_block_reduce(acc, red);
    const double spread_d = (table && d) ? gd_log_spread(d, n, 1, redd) : 0.0;
    const double spread_sv = (table && sv) ? gd_log_spread(sv, n, 0, redd) : 0.0;
    if (threadIdx.x != 0) return;
    out[0] = acc.mx; out[1] = acc.idx; out[2] = acc.site; out[3] = acc.sum; out[4] = acc.fresh; out[5] = acc.bad;
    if (!table) return;
    double* t = (double*)((char*)table + (size_t)blockIdx.z * table_stride) + (size_t)row * DQMC_GREEN_CHECK_FIELDS;
    const double rel = acc.fresh > 0.0 ? acc.mx / acc.fresh : (acc.mx > 0.0 ? INFINITY : 0.0);
    t[0] += 1.0;
    t[1] = acc.mx;
    if (acc.mx > t[2]) { t[2] = acc.mx; t[7] = acc.idx; }
    t[3] += acc.mx;
    t[4] = fmax(t[4], acc.site);
    t[5] += acc.sum / ((double)n * (double)n);
    t[6] = fmax(t[6], rel);
    t[8] += acc.bad;
    t[9] = fmax(t[9], spread_d);
    t[10] = fmax(t[10], spread_sv);
}

// keep[chain][count] = the first count entries of every chain's G
__global__ void k_green_keep(const cplx* __restrict__ G, cplx* __restrict__ keep, size_t keep_stride, size_t count, size_t cs) {
    CHAIN(G);
    keep = (cplx*)((char*)keep + (size_t)blockIdx.z * keep_stride);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) keep[i] = G[i];
}

size_t green_diff_partial_doubles(int n) { return (((size_t)n * n + GD_CHUNK - 1) / GD_CHUNK) * GD_FIELDS; }

void launch_green_keep(const Launch& lc, const cplx* G, cplx* keep, size_t keep_stride, size_t count) {
    const int blocks = (int)std::min<size_t>(2048, (count + 255) / 256);
    hipLaunchKernelGGL(k_green_keep, dim3(blocks, 1, lc.nb), dim3(256), 0, lc.st, G, keep, keep_stride, count, lc.cs);
}

void launch_green_diff(const Launch& lc, const cplx* Gw, size_t gw_stride, const cplx* Gf, int n, int ld, int N, double* part,
                       size_t part_stride, double* out, size_t out_stride, const GreenCheckFold* fold) {
    const int nparts = (int)(green_diff_partial_doubles(n) / GD_FIELDS);
    hipLaunchKernelGGL(k_green_diff_partial, dim3(nparts, 1, lc.nb), dim3(GD_THREADS), 0, lc.st, Gw, gw_stride, Gf, n, ld, N, part,
                       part_stride, lc.cs);
    hipLaunchKernelGGL(k_green_diff_finalise, dim3(1, 1, lc.nb), dim3(GD_THREADS), 0, lc.st, (const double*)part, part_stride, nparts, n,
                       out, out_stride, fold ? fold->table : nullptr, fold ? fold->table_stride : 0, fold ? fold->row : 0,
                       fold ? fold->d : nullptr, fold ? fold->sv : nullptr, lc.cs);
}
