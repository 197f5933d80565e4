// The displacement walk of the binned measurement kernels, shared by kernels_measure.hip (SDW model) and kernels_hubbard.hip.
#pragma once
#include "dqmc_internal.h"

// The binned kernels below (every k_measure_* with TDP_BINS * TDP_PARTS threads) share one shape.  A workgroup owns 32 consecutive bins
// d = (dx, dy), the N periodic site differences, bin dy L + dx; thread (part, bin) walks the sites B = part, part + 8, ... in this order
// and sums its kernel's summand over the pairs (A = B (+) d, B), so the 32 lanes of a half wave read consecutive rows A of one column
// (runs of L elements between the periodic wraps).  BinWalk is that shape: the decode of threadIdx.x, the walk, and the reduction.
// The walk is a loop header,   for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) { the kernel's summand at st },
// so that the summand stays in the kernel's own loop body.
#define TDP_BINS 32
#define TDP_PARTS 8
// one step of the walk: the pair A = (ax, ay) = B (+) d, B = (bx, by); wx / wy: B + d left the lattice in x / y (the antiperiodic sign of
// k_measure_green_matrix)
struct BinSite { int A, B, ax, ay, bx, by; bool wx, wy; };
struct BinWalk {
    int lb, part, d, dx, dy;
    bool valid;                                             // d < N: the last workgroup's tile of bins may be ragged
    __device__ __forceinline__ BinWalk(int N, int L) {
        lb = threadIdx.x % TDP_BINS; part = threadIdx.x / TDP_BINS;
        d = blockIdx.x * TDP_BINS + lb;
        valid = d < N;
        dx = valid ? d % L : 0; dy = valid ? d / L : 0;
    }
    __device__ __forceinline__ void place(BinSite& st, int L) const {       // A = B (+) d
        st.ax = st.bx + dx; st.ay = st.by + dy;
        st.wx = st.ax >= L; st.wy = st.ay >= L;
        if (st.wx) st.ax -= L;
        if (st.wy) st.ay -= L;
        st.A = st.ay * L + st.ax;
    }
    __device__ __forceinline__ BinSite first(int N, int L) const {          // B = part; a thread without a bin starts at the end
        BinSite st;
        st.B = valid ? part : N;
        st.bx = part % L; st.by = part / L;
        place(st, L);
        return st;
    }
    __device__ __forceinline__ void next(BinSite& st, int L) const {        // B += 8, kept as (bx, by)
        st.B += TDP_PARTS;
        st.bx += TDP_PARTS % L; st.by += TDP_PARTS / L;
        if (st.bx >= L) { st.bx -= L; ++st.by; }
        place(st, L);
    }
    // The eight partial sums w[c] of every channel c < NCH meet in LDS, and ONE thread per (bin, channel) -- part c for channel c < nch --
    // adds them in the order part = 0 .. 7 and adds the result to dst[c pstride + d dstride]: one writer per accumulator, fixed order, no
    // atomics, reproducible bit for bit.  count: the row's sample counter, which thread 0 of workgroup 0 bumps; nullptr where the caller
    // counts elsewhere.  A caller with more than TDP_PARTS sums calls this once per TDP_PARTS of them, with a barrier in between.
    template<int NCH>
    __device__ __forceinline__ void reduce_add(const double* w, double (&red)[NCH][TDP_PARTS][TDP_BINS], int nch, double* dst, size_t pstride,
                                               size_t dstride, double* count) const {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) red[ch][part][lb] = w[ch];
        __syncthreads();
        if (part < nch && valid) {
            double s = red[part][0][lb];
#pragma unroll
            for (int q = 1; q < TDP_PARTS; ++q) s += red[part][q][lb];
            dst[(size_t)part * pstride + (size_t)d * dstride] += s;
        }
        if (count && blockIdx.x == 0 && threadIdx.x == 0) *count += 1.0;
    }
};
