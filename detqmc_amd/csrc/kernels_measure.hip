// Fermionic observables of one time slice, accumulated on the device from the shifted Green's function
// gs = e^{-dtau K/2} G e^{+dtau K/2} (shiftGreenSymmetric, reference src/detsdwopdim.cpp:4507-4612; the shift itself is
// two half-step plaquette passes per side in k_bmult_chain's shift mode, or two GEMMs with the dense half propagators).
//
// Replaces the G-dependent part of DetSDW::measure (src/detsdwopdim.cpp:545-899): greenK0 (sum of all entries),
// greenLocal (trace), occDiffSq, the pairing correlators pairPlus / pairMinus, and the momentum-space occupation
// kOccX / kOccY.  The reference evaluates kOcc with an O(N^3) loop of complex exponentials per slice; here a slice
// only bins  S_band(dx, dy) = sum_{i - j = (dx, dy)} [g_band,up(i, j) + g_band,down(i, j)]  over the (2L-1)^2 plain
// (not periodic: antiperiodic boundaries shift k by half a step) site differences, and the Fourier sum over the bins
// is done once per sweep on the host (detsdw.cpp).  Every accumulator has exactly one writer and a fixed summation
// order: results are reproducible bit for bit.
#include "dqmc_internal.h"
#include "bin_walk.h"
#include <type_traits>

size_t measure_accum_doubles(int N, int L) {
    const size_t nbins = (size_t)(2 * L - 1) * (2 * L - 1);
    return 4 + 2 * (size_t)N + 4 * nbins;
}

__device__ __forceinline__ cplx m_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx m_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx m_mul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cplx m_scale(double s, cplx a) { return make_double2(s * a.x, s * a.y); }
__device__ __forceinline__ cplx m_conj(cplx a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ double m_re_mul(cplx a, cplx b) { return a.x * b.x - a.y * b.y; }       // Re a b
__device__ __forceinline__ double m_re_mulc(cplx a, cplx b) { return a.x * b.x + a.y * b.y; }      // Re a conj b
__device__ __forceinline__ double m_abs2(cplx v) { return v.x * v.x + v.y * v.y; }
// the R x R flavour block e[r][c] = g(P r; Q c) = pe[c N ng + r N] of a matrix g, pe = g + Q ng + P.  Which form to call: a kernel that
// holds pe or the offset Q ng + P anyway (it reads the same pair from a second matrix, or its OPDIM < 3 branch loads from pe) hands that
// pointer in, so that all its loads share their address registers (k_measure_td_band<3> needs 26 VGPRs more otherwise); a kernel with no
// other use of the pointer names the pair
template<int R>
__device__ __forceinline__ void m_load_block(const cplx* __restrict__ pe, size_t ng, int N, cplx (&e)[R][R]) {
#pragma unroll
    for (int c2 = 0; c2 < R; ++c2)
#pragma unroll
        for (int r = 0; r < R; ++r) e[r][c2] = pe[(size_t)c2 * N * ng + (size_t)r * N];
}
template<int R>
__device__ __forceinline__ void m_load_block(const cplx* __restrict__ g, size_t ng, int N, int P, int Q, cplx (&e)[R][R]) {
    m_load_block(g + (size_t)Q * ng + (size_t)P, ng, N, e);
}

// f(std::integral_constant<int, OPDIM>) for the model's OPDIM: the one place a run-time opdim picks a kernel instantiation
template<class F>
static void dispatch_opdim(int opdim, F&& f) {
    if (opdim == 1) f(std::integral_constant<int, 1>{});
    else if (opdim == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// BandSpin: XUP = 0, YDOWN = 1, XDOWN = 2, YUP = 3 (detsdwopdim.h:223-232); gl1 of measure() (:594-612): for OPDIM < 3
// only the (XUP, YDOWN) sector is stored, the (XDOWN, YUP) sector is its complex conjugate, the rest vanishes
template<int OPDIM>
struct GreenAccess {
    const cplx* gs; int ng, N;
    __device__ __forceinline__ cplx operator()(int s1, int bs1, int s2, int bs2) const {
        if (OPDIM == 3) return gs[(size_t)(s2 + N * bs2) * ng + s1 + N * bs1];
        if (bs1 < 2 && bs2 < 2) return gs[(size_t)(s2 + N * bs2) * ng + s1 + N * bs1];
        if (bs1 >= 2 && bs2 >= 2) { cplx v = gs[(size_t)(s2 + N * (bs2 - 2)) * ng + s1 + N * (bs1 - 2)]; return make_double2(v.x, -v.y); }
        return make_double2(0.0, 0.0);
    }
};
// getBandSpin (detsdwopdim.h:268-273): band 0 = X, 1 = Y; spin 0 = up, 1 = down
__device__ __forceinline__ int m_bs(int band, int spin) { return band == 0 ? (spin == 0 ? 0 : 2) : (spin == 0 ? 3 : 1); }

__device__ __forceinline__ double block_sum(double v, double* red) {      // fixed-order tree over 256 threads
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// S_band(dx, dy) bins for the momentum-space occupation (:616-659): 8 lanes per bin, each takes every 8th site,
// partial sums combined in a fixed order by DPP row shifts (lane 7 of the group ends up with the total).  idx = this thread's
// place in the bin grid; S = S_X (re, im) followed by S_Y.  Called by whole workgroups (the DPP shifts read neighbour lanes).
template<int OPDIM>
__device__ __forceinline__ void accum_bins(const GreenAccess<OPDIM>& g1, int N, int L, int idx, double* S0) {
    auto gl = [&](int s1, int b1, int sp1, int s2, int b2, int sp2) { return g1(s1, m_bs(b1, sp1), s2, m_bs(b2, sp2)); };
    constexpr int UP = 0, DN = 1;
    const int W = 2 * L - 1, nbins = W * W;
    const int binlin = idx >> 3, part = idx & 7;
    const bool valid = binlin < 2 * nbins;
    const int band = valid ? binlin / nbins : 0, bin = valid ? binlin - band * nbins : 0;
    const int dx = bin % W - (L - 1), dy = bin / W - (L - 1);
    cplx s = make_double2(0.0, 0.0);
    if (valid)
        for (int i = part; i < N; i += 8) {
            const int ix = i % L, iy = i / L;
            const int jx = ix - dx, jy = iy - dy;
            if (jx < 0 || jx >= L || jy < 0 || jy >= L) continue;
            const int j = jy * L + jx;
            s = m_add(s, m_add(gl(i, band, UP, j, band, UP), gl(i, band, DN, j, band, DN)));
        }
    auto shr_add = [](double v, int ctrl_sel) {
        int lo = __double2loint(v), hi = __double2hiint(v), lo2, hi2;
        if (ctrl_sel == 1) { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xf, 0xf, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xf, 0xf, false); }
        else if (ctrl_sel == 2) { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xf, 0xf, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xf, 0xf, false); }
        else { lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xf, 0xf, false); hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xf, 0xf, false); }
        return v + __hiloint2double(hi2, lo2);
    };
    s.x = shr_add(s.x, 1); s.y = shr_add(s.y, 1);      // row_shr:1, 2, 4: lane l holds the sum of lanes l-7 .. l
    s.x = shr_add(s.x, 2); s.y = shr_add(s.y, 2);
    s.x = shr_add(s.x, 4); s.y = shr_add(s.y, 4);
    if (valid && part == 7) {
        double* S = S0 + (size_t)band * 2 * nbins;
        S[2 * bin] += s.x;
        S[2 * bin + 1] += s.y;
    }
}

template<int OPDIM>
__global__ __launch_bounds__(256) void k_measure_accum(DevModel dm, const cplx* __restrict__ gs, double* __restrict__ acc, size_t cs) {
    CHAIN(gs); CHAIN(acc);
    __shared__ double red[256];
    const int N = dm.N, ng = dm.ng, L = dm.L, tid = threadIdx.x;
    const GreenAccess<OPDIM> g1{gs, ng, N};
    auto gl = [&](int s1, int b1, int sp1, int s2, int b2, int sp2) { return g1(s1, m_bs(b1, sp1), s2, m_bs(b2, sp2)); };
    const int role = blockIdx.x;
    constexpr int X = 0, Y = 1, UP = 0, DN = 1;
    if (role == 0) {
        // greenK0 += [2] Re sum(gs), greenLocal += [2] Re tr(gs) / (4 N)   (:565-588)
        double s = 0.0, t = 0.0;
        const size_t total = (size_t)ng * ng;
        {   // one workgroup sums n_g^2 elements: eight independent partial sums keep eight loads per thread in flight
            double p[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            size_t idx = tid;
            for (; idx + 7 * 256 < total; idx += 8 * 256) {
#pragma unroll
                for (int u = 0; u < 8; ++u) p[u] += gs[idx + (size_t)u * 256].x;
            }
            for (; idx < total; idx += 256) p[0] += gs[idx].x;
            s = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
        }
        for (int i = tid; i < ng; i += 256) t += gs[(size_t)i * ng + i].x;
        s = block_sum(s, red);
        t = block_sum(t, red);
        if (tid == 0) {
            const double f = (OPDIM == 3) ? 1.0 : 2.0;
            acc[0] += f * s;
            acc[1] += f * t / (4.0 * N);
            acc[3] += 1.0;
        }
    } else if (role == 1) {
        // occDiffSq (:866-897)
        double c = 0.0;
        for (int i = tid; i < N; i += 256) {
            auto g = [&](int b1, int s1, int b2, int s2) { return gl(i, b1, s1, i, b2, s2); };
            cplx v = m_scale(-2.0, m_mul(g(X, DN, X, UP), g(X, UP, X, DN)));
            v = m_add(v, g(X, UP, X, UP));
            v = m_add(v, m_scale(2.0, m_mul(g(X, DN, Y, DN), g(Y, DN, X, DN))));
            v = m_add(v, m_scale(2.0, m_mul(g(X, UP, Y, DN), g(Y, DN, X, UP))));
            v = m_add(v, g(Y, DN, Y, DN));
            v = m_sub(v, m_scale(2.0, m_mul(g(X, UP, X, UP), g(Y, DN, Y, DN))));
            v = m_add(v, m_scale(2.0, m_mul(g(X, DN, Y, UP), g(Y, UP, X, DN))));
            v = m_add(v, m_scale(2.0, m_mul(g(X, UP, Y, UP), g(Y, UP, X, UP))));
            v = m_sub(v, m_scale(2.0, m_mul(g(Y, DN, Y, UP), g(Y, UP, Y, DN))));
            cplx f = make_double2(1.0, 0.0);
            f = m_add(f, m_scale(2.0, g(X, UP, X, UP)));
            f = m_sub(f, m_scale(2.0, g(Y, DN, Y, DN)));
            f = m_sub(f, m_scale(2.0, g(Y, UP, Y, UP)));
            v = m_add(v, m_mul(g(X, DN, X, DN), f));
            v = m_add(v, g(Y, UP, Y, UP));
            v = m_sub(v, m_scale(2.0, m_mul(g(X, UP, X, UP), g(Y, UP, Y, UP))));
            v = m_add(v, m_scale(2.0, m_mul(g(Y, DN, Y, DN), g(Y, UP, Y, UP))));
            c += v.x;
        }
        c = block_sum(c, red);
        if (tid == 0) acc[2] += c / (double)N;
    } else if (role == 2) {
        // pairPlus[i], pairMinus[i] (:661-722): site pairs (i, 0) and (0, i)
        for (int i = tid; i < N; i += 256) {
            cplx plus = make_double2(0.0, 0.0), minus = make_double2(0.0, 0.0);
            for (int pr = 0; pr < 2; ++pr) {
                const int A = pr == 0 ? i : 0, B = pr == 0 ? 0 : i;
                auto P = [&](int b1, int b2) {
                    return m_sub(m_mul(gl(A, b1, DN, B, b2, UP), gl(A, b1, UP, B, b2, DN)),
                                 m_mul(gl(A, b1, DN, B, b2, DN), gl(A, b1, UP, B, b2, UP)));
                };
                const cplx pxx = P(X, X), pxy = P(X, Y), pyx = P(Y, X), pyy = P(Y, Y);
                plus = m_add(plus, m_scale(-4.0, m_add(m_add(m_add(pxx, pxy), pyx), pyy)));
                minus = m_add(minus, m_scale(-4.0, m_add(m_sub(m_sub(pxx, pxy), pyx), pyy)));
            }
            acc[4 + i] += plus.x;
            acc[4 + N + i] += minus.x;
        }
    } else {
        accum_bins(g1, N, L, (role - 3) * 256 + tid, acc + 4 + 2 * N);
    }
}

void launch_measure_accum(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc) {
    const int nbins = (2 * hm.L - 1) * (2 * hm.L - 1);
    const dim3 grid(3 + (2 * nbins * 8 + 255) / 256, 1, lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_accum<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, gs, acc, lc.cs);
    });
}

// Time-displaced block (dqmc_measure_timedisplaced): the S_X / S_Y bins of gs = e^{-dtau K/2} G(tau_j, 0) e^{+dtau K/2} into the block of
// boundary j, and one sample counted.  Same bins, lanes and summation order as the equal-time kOcc bins above.
// Addressing of every time-displaced block below: count[rows], then row `row` at offset rows + row * stride.  The coarse blocks are
// written with (row, rows) = (j - 1, n - 1), the every-slice blocks (dqmc_measure_timedisplaced_segment / _ends) with (k, m + 1).
size_t measure_td_doubles(int L, int n) {
    const size_t nbins = (size_t)(2 * L - 1) * (2 * L - 1);
    return (size_t)(n - 1) * (1 + 4 * nbins);
}
// stride of one row of a time-displaced block: channel 0 G(k, tau) bins, 1 pairing, 2 particle-hole, 3 current, 4 band-resolved charge
size_t measure_td_row_doubles(int channel, int N, int L) {
    const size_t nbins = (size_t)(2 * L - 1) * (2 * L - 1);
    return channel == 0 ? 4 * nbins : channel == 2 ? 3 * (size_t)N : channel == 3 ? 2 * (size_t)N + 2 : 2 * (size_t)N;
}

template<int OPDIM>
__global__ __launch_bounds__(256) void k_measure_td(DevModel dm, const cplx* __restrict__ gs, double* __restrict__ acc, int row, int rows, size_t cs) {
    CHAIN(gs); CHAIN(acc);
    const int N = dm.N, L = dm.L, nbins = (2 * L - 1) * (2 * L - 1);
    const GreenAccess<OPDIM> g1{gs, dm.ng, N};
    accum_bins(g1, N, L, blockIdx.x * 256 + threadIdx.x, acc + rows + (size_t)row * 4 * nbins);
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[row] += 1.0;
}

void launch_measure_td(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, int row, int rows) {
    const int nbins = (2 * hm.L - 1) * (2 * hm.L - 1);
    const dim3 grid((2 * nbins * 8 + 255) / 256, 1, lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, gs, acc, row, rows, lc.cs);
    });
}

// BinWalk, the shape every binned kernel below shares (TDP_BINS * TDP_PARTS threads), lives in bin_walk.h

// Time-displaced pairing block (dqmc_measure_timedisplaced_pair): with gs = e^{-dtau K/2} G(tau_j, 0) e^{+dtau K/2} and the P(b1, b2) of
// role 2 of k_measure_accum above evaluated on gs for EVERY site pair (A, B),
//   T+(A, B) = -4 [P(X,X) + P(X,Y) + P(Y,X) + P(Y,Y)],   T-(A, B) = -4 [P(X,X) - P(X,Y) - P(Y,X) + P(Y,Y)],
// the block of boundary j receives  sum_B Re T+-(B (+) d, B)  for the N periodic site differences d = (dx, dy), bin dy L + dx (the 1 / N of
// the translation average is left to the reader of the block).  A pair (A, B) needs the 4 x 4 band-spin elements gs(A bs1; B bs2), each
// exactly once, so one launch streams gs once.  For OPDIM < 3 only the (XUP, YDOWN) sector e_rc = gs(A + N r; B + N c) is stored, the
// (XDOWN, YUP) sector is its conjugate and the mixed sectors vanish (GreenAccess), which leaves
//   P(X,X) = -|e_00|^2,  P(X,Y) = |e_01|^2,  P(Y,X) = |e_10|^2,  P(Y,Y) = -|e_11|^2:  four loads per pair instead of sixteen.
size_t measure_td_pair_doubles(int N, int n) { return (size_t)(n - 1) * (1 + 2 * (size_t)N); }

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_pair(DevModel dm, const cplx* __restrict__ gs, double* __restrict__ acc, int row, int rows, size_t cs) {
    CHAIN(gs); CHAIN(acc);
    __shared__ double red[2][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    double tp = 0.0, tm = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const cplx* p = gs + (size_t)st.B * ng + (size_t)st.A;
        if (OPDIM == 3) {
            // e[bs1][bs2], BandSpin XUP = 0, YDOWN = 1, XDOWN = 2, YUP = 3
            cplx e[4][4];
            m_load_block(p, ng, N, e);
            // Re P(b1, b2) with (dn1, up1) = band-spin rows of band b1, (up2, dn2) = band-spin columns of band b2
            auto P = [&](int dn1, int up1, int up2, int dn2) { return m_re_mul(e[dn1][up2], e[up1][dn2]) - m_re_mul(e[dn1][dn2], e[up1][up2]); };
            const double pxx = P(2, 0, 0, 2), pxy = P(2, 0, 3, 1), pyx = P(1, 3, 0, 2), pyy = P(1, 3, 3, 1);
            tp += -4.0 * (((pxx + pxy) + pyx) + pyy);
            tm += -4.0 * (((pxx - pxy) - pyx) + pyy);
        } else {
            const cplx e00 = p[0], e10 = p[N], e01 = p[(size_t)N * ng], e11 = p[(size_t)N * ng + N];
            const double pxx = -m_abs2(e00), pxy = m_abs2(e01), pyx = m_abs2(e10), pyy = -m_abs2(e11);
            tp += -4.0 * (((pxx + pxy) + pyx) + pyy);
            tm += -4.0 * (((pxx - pxy) - pyx) + pyy);
        }
    }
    const double w[2] = {tp, tm};                           // C+, C-
    bw.reduce_add(w, red, 2, acc + rows + (size_t)row * 2 * N, N, 1, acc + row);
}

void launch_measure_td_pair(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_pair<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, acc, row, rows, lc.cs);
    });
}

// Time-displaced particle-hole block (dqmc_measure_timedisplaced_ph; definitions in dqmc_hip.h and DESIGN.md 6e).  For a site bilinear
// O^M_i = sum_ab c^+_ia M_ab c_ib and the four shifted matrices of one boundary,
//   W^M(A, B) = o^M_tau(A) o^M_0(B) - sum_abcd M_ab M_cd g0t(B d; A a) gt0(A b; B c),     o^M_t(A) = tr M - sum_ab M_ab g_t(A b; A a).
// Every M used here has ONE non-zero entry per row, M(a, pi(a)) = m_a, so the connected part is
//   sum_{a, c} m_a m_c  gt0(A pi(a); B c)  g0t(B pi(c); A a)                                                     (16 products per M)
// and all coefficient products m_a m_c are real (M_y: m = i y with y = (-1, +1, +1, -1)).  The second factor is read from
// hs = (shifted G(0, tau))^H, written by the tile transpose that takes the shifted matrix out of the shift scratch anyway:
//   g0t(B d; A a) = conj hs(A a; B d),
// the SAME address pattern as gt0(A b; B c) -- lanes run over consecutive rows A of one column for both streams, and each matrix is read
// exactly once per launch.  Only Re W is binned, Re (x conj y) = x.re y.re + x.im y.im.
// OPDIM < 3: both matrices are diag(stored sector, its conjugate); all M of the channels in use (charge, spinZ, M_x, M_y) are block
// diagonal in that structure, so the second sector contributes the complex conjugate of the first: with e_rc = gt0(A + N r; B + N c),
// h_rc = hs(A + N r; B + N c), d_rc = Re e_rc conj h_rc and q_ac = Re e_(1-a)c conj h_a(1-c),
//   charge = 2 sum d_rc,   spinZ = (d_00 + d_11 - d_01 - d_10) / 2,   M_x = 2 (q_00 + q_01 + q_10 + q_11),   M_y = 2 (-q_00 + q_01 + q_10 - q_11):
// eight loads per pair, nothing multiplied by a structural zero.
size_t measure_td_ph_doubles(int N, int n) { return (size_t)(n - 1) * (1 + 3 * (size_t)N); }

#define TDPH_CH 5       // one-body values per site and time: charge, spinZ, M_x, M_y, M_z

// ob[t][channel][site] for one of the two equal-time matrices (t = 0: G(tau_j), t = 1: G(0)); gs is its shifted form
template<int OPDIM>
__global__ __launch_bounds__(256) void k_td_ph_onebody(DevModel dm, const cplx* __restrict__ gs, cplx* __restrict__ ob, int t, size_t cs) {
    CHAIN(gs); CHAIN(ob);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    const GreenAccess<OPDIM> g1{gs, dm.ng, N};
    auto g = [&](int r, int c2) { return g1(A, r, A, c2); };       // g(b, a) = g_t(A b; A a); constant indices: the zero sectors fold away
    cplx* o = ob + (size_t)t * TDPH_CH * N + A;
    const cplx tr = m_add(m_add(g(0, 0), g(1, 1)), m_add(g(2, 2), g(3, 3)));
    o[0] = make_double2(4.0 - tr.x, -tr.y);
    o[(size_t)N] = m_scale(-0.5, m_sub(m_add(g(0, 0), g(3, 3)), m_add(g(1, 1), g(2, 2))));
    o[(size_t)2 * N] = m_scale(-1.0, m_add(m_add(g(1, 0), g(0, 1)), m_add(g(3, 2), g(2, 3))));
    if (OPDIM >= 2) {       // tr M_y g = i (g01 - g10 + g32 - g23)
        const cplx v = m_add(m_sub(g(0, 1), g(1, 0)), m_sub(g(3, 2), g(2, 3)));
        o[(size_t)3 * N] = make_double2(v.y, -v.x);                // -i v
    }
    if (OPDIM == 3) o[(size_t)4 * N] = m_scale(-1.0, m_sub(m_add(g(3, 0), g(0, 3)), m_add(g(2, 1), g(1, 2))));
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_ph(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ hs,
                                                                        const cplx* __restrict__ ob, double* __restrict__ acc, int row, int rows, size_t cs) {
    CHAIN(gs); CHAIN(hs); CHAIN(ob); CHAIN(acc);
    // Not under BinWalk: the O(3) instantiation sits at 154 VGPRs, inside three waves per SIMD (168); under BinWalk as it stands it takes 169
    // and runs two (profiles/measure_walk_resources_parent_vs_this.txt).  The shape of BinWalk written out.
    __shared__ double red[3][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, tid = threadIdx.x;
    const size_t ng = (size_t)dm.ng;
    const int lb = tid % TDP_BINS, part = tid / TDP_BINS;
    const int d = blockIdx.x * TDP_BINS + lb;
    const bool valid = d < N;
    const int dx = valid ? d % L : 0, dy = valid ? d / L : 0;
    const cplx* ot = ob;                                    // o_tau(A)
    const cplx* o0 = ob + (size_t)TDPH_CH * N;              // o_0(B)
    auto rd = [](cplx a, cplx b) { return a.x * b.x + a.y * b.y; };       // Re a conj b
    auto re_mul = [](cplx a, cplx b) { return a.x * b.x - a.y * b.y; };   // Re a b
    double wc = 0.0, wz = 0.0, ws = 0.0;
    if (valid) {
        int bx = part % L, by = part / L;                   // site B = part + 8 i, kept as (bx, by)
        const int stepx = TDP_PARTS % L, stepy = TDP_PARTS / L;
        for (int B = part; B < N; B += TDP_PARTS) {
            int ax = bx + dx, ay = by + dy;
            if (ax >= L) ax -= L;
            if (ay >= L) ay -= L;
            const int A = ay * L + ax;
            const size_t off = (size_t)B * ng + (size_t)A;
            const cplx* pe = gs + off;
            const cplx* ph = hs + off;
            // disconnected parts
            const double dc = re_mul(ot[A], o0[B]), dz = re_mul(ot[N + A], o0[N + B]);
            double ds = re_mul(ot[2 * N + A], o0[2 * N + B]);
            if (OPDIM >= 2) ds += re_mul(ot[3 * N + A], o0[3 * N + B]);
            if (OPDIM == 3) ds += re_mul(ot[4 * N + A], o0[4 * N + B]);
            double cc, cz, cs2;
            if (OPDIM == 3) {
                cplx e[4][4];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[r][c2] = pe[(size_t)c2 * N * ng + (size_t)r * N];
                constexpr int pxy[4] = {1, 0, 3, 2}, pz[4] = {3, 2, 1, 0};
                constexpr double sz[4] = {1.0, -1.0, -1.0, 1.0};      // spinZ diagonal (x 2), the y of M_y and the m of M_z alike
                cc = 0.0; cz = 0.0;
                double cx = 0.0, cy = 0.0, cq = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    cplx h[4];                                        // h[dl] = hs(A a; B dl)
#pragma unroll
                    for (int dl = 0; dl < 4; ++dl) h[dl] = ph[(size_t)dl * N * ng + (size_t)a * N];
#pragma unroll
                    for (int c2 = 0; c2 < 4; ++c2) {
                        const double v = rd(e[a][c2], h[c2]);
                        cc += v;
                        cz += sz[a] * sz[c2] * v;
                        const double q = rd(e[pxy[a]][c2], h[pxy[c2]]);
                        cx += q;
                        cy += sz[a] * sz[c2] * q;                    // m_a m_c = -y_a y_c with y = -sz
                        cq += sz[a] * sz[c2] * rd(e[pz[a]][c2], h[pz[c2]]);
                    }
                }
                cz *= 0.25;
                cs2 = (cx - cy) + cq;
            } else {
                const size_t cN = (size_t)N * ng;
                const cplx e00 = pe[0], e10 = pe[N], e01 = pe[cN], e11 = pe[cN + N];
                const cplx h00 = ph[0], h10 = ph[N], h01 = ph[cN], h11 = ph[cN + N];
                const double d00 = rd(e00, h00), d11 = rd(e11, h11), d01 = rd(e01, h01), d10 = rd(e10, h10);
                cc = 2.0 * ((d00 + d11) + (d01 + d10));
                cz = 0.5 * ((d00 + d11) - (d01 + d10));
                const double q01 = rd(e11, h00), q10 = rd(e00, h11);
                if (OPDIM == 1) cs2 = 2.0 * ((rd(e10, h01) + rd(e01, h10)) + (q01 + q10));
                else cs2 = 4.0 * (q01 + q10);                        // M_x + M_y: the q_00 and q_11 terms cancel
            }
            wc += dc - cc;
            wz += dz - cz;
            ws += (ds - cs2) * (1.0 / OPDIM);
            bx += stepx; by += stepy;
            if (bx >= L) { bx -= L; ++by; }
        }
    }
    red[0][part][lb] = wc;
    red[1][part][lb] = wz;
    red[2][part][lb] = ws;
    __syncthreads();
    if (part < 3 && valid) {                                // part 0 writes charge of its bin, part 1 spinZ, part 2 sdw
        double s = red[part][0][lb];
#pragma unroll
        for (int q = 1; q < TDP_PARTS; ++q) s += red[part][q][lb];
        acc[rows + (size_t)row * 3 * N + (size_t)part * N + d] += s;
    }
    if (blockIdx.x == 0 && tid == 0) acc[row] += 1.0;
}

size_t measure_td_ph_onebody_cplx(int N) { return (size_t)2 * TDPH_CH * N; }

void launch_td_ph_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, int t) {
    const dim3 grid((hm.N + 255) / 256, 1, lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_td_ph_onebody<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, gs, ob, t, lc.cs);
    });
}

void launch_measure_td_ph(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* ob, double* acc, int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_ph<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, hs, ob, acc, row, rows, lc.cs);
    });
}

// Equal-time two-particle block (dqmc_set_equal_time_correlators; definitions in dqmc_hip.h and DESIGN.md 6e).  The Wick forms of
// k_measure_td_ph and k_measure_td_pair with ONE matrix gs = e^{-dtau K/2} G(tau_k) e^{+dtau K/2} in both roles: G(tau, 0) -> gs and
// G(0, tau) -> gs - 1, so
//   W^M(A, B) = o^M(A) o^M(B) - sum_abcd M_ab M_cd gs(B d; A a) gs(A b; B c) + delta_AB sum_bc (M^2)_cb gs(A b; A c).
// gs - 1 is never formed: M^2 = 1 for charge and every SDW component and 1/4 for spinZ, so the delta term is tr_4 gs(B; B) = 4 - o^charge(B)
// (times 1/4 for spinZ), added to the d = 0 bin from the one-body value already in hand.  The pairing sums T+-(A, B) contain gs(A .; B .)
// only and have no delta term.
// The transposed factor gs(B d; A a) is read directly: t_ac = gs[(A + N a) ng + B + N c] takes the place of conj hs(A a; B c) in
// k_measure_td_ph, Re e conj h -> Re e t.  With the 32 bins x 8 parts shape one step of a workgroup reads (row B, column B (+) d + N a) for
// eight consecutive rows B and 32 consecutive bins d: a band of about 39 columns x 8 rows, one aligned 128-byte line per column, whose
// eight elements are used in that step by the lanes (part p, bin d0 - p) -- fewer only at the band's edges and at the wraps of x.  The
// forward factor keeps the pattern of the time-displaced kernels (lanes over consecutive rows A of one column).  No transposed copy, no
// n_g^2 buffer.
// One-body values: k_eq_onebody writes ob[5][N] (the t = 0 half of k_td_ph_onebody's layout) from the same matrix, 5 N complex numbers.
// OPDIM < 3: the stored sector and its conjugate as in k_measure_td_ph and k_measure_td_pair -- eight loads per pair serve all five sums;
// O(3): the sixteen e and sixteen t of the full 4 x 4 blocks.
// Block of one chain (doubles): count, charge[N], spinZ[N], sdw[N], pairPlus[N], pairMinus[N]; it lives outside the chain arena, chain b
// at acc + b (1 + 5 N).
size_t measure_eq_doubles(int N) { return 1 + 5 * (size_t)N; }
size_t measure_eq_onebody_cplx(int N) { return (size_t)TDPH_CH * N; }

template<int OPDIM>
__global__ __launch_bounds__(256) void k_eq_onebody(DevModel dm, const cplx* __restrict__ gs, cplx* __restrict__ ob, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    const GreenAccess<OPDIM> g1{gs, dm.ng, N};
    auto g = [&](int r, int c2) { return g1(A, r, A, c2); };       // g(b, a) = gs(A b; A a)
    cplx* o = ob + (size_t)blockIdx.z * TDPH_CH * N + A;
    const cplx tr = m_add(m_add(g(0, 0), g(1, 1)), m_add(g(2, 2), g(3, 3)));
    o[0] = make_double2(4.0 - tr.x, -tr.y);
    o[(size_t)N] = m_scale(-0.5, m_sub(m_add(g(0, 0), g(3, 3)), m_add(g(1, 1), g(2, 2))));
    o[(size_t)2 * N] = m_scale(-1.0, m_add(m_add(g(1, 0), g(0, 1)), m_add(g(3, 2), g(2, 3))));
    if (OPDIM >= 2) {       // tr M_y g = i (g01 - g10 + g32 - g23)
        const cplx v = m_add(m_sub(g(0, 1), g(1, 0)), m_sub(g(3, 2), g(2, 3)));
        o[(size_t)3 * N] = make_double2(v.y, -v.x);                // -i v
    }
    if (OPDIM == 3) o[(size_t)4 * N] = m_scale(-1.0, m_sub(m_add(g(3, 0), g(0, 3)), m_add(g(2, 1), g(1, 2))));
}

#define EQ_CH 5         // binned sums: charge, spinZ, sdw, pairPlus, pairMinus
template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_eq_corr(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ ob,
                                                                          double* __restrict__ acc, size_t cs) {
    CHAIN(gs);
    ob += (size_t)blockIdx.z * TDPH_CH * dm.N;
    acc += (size_t)blockIdx.z * (1 + (size_t)EQ_CH * dm.N);
    // Not under BinWalk: the O(1) instantiation sits at 80 VGPRs, the limit of six waves per SIMD; under BinWalk as it stands it takes 85
    // and runs five (profiles/measure_walk_resources_parent_vs_this.txt).  The shape of BinWalk written out.
    __shared__ double red[EQ_CH][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, tid = threadIdx.x;
    const size_t ng = (size_t)dm.ng;
    const int lb = tid % TDP_BINS, part = tid / TDP_BINS;
    const int d = blockIdx.x * TDP_BINS + lb;
    const bool valid = d < N;
    const int dx = valid ? d % L : 0, dy = valid ? d / L : 0;
    auto re_mul = [](cplx a, cplx b) { return a.x * b.x - a.y * b.y; };   // Re a b
    auto abs2 = [](cplx v) { return v.x * v.x + v.y * v.y; };
    double wc = 0.0, wz = 0.0, ws = 0.0, tp = 0.0, tm = 0.0;
    if (valid) {
        int bx = part % L, by = part / L;                   // site B = part + 8 i, kept as (bx, by)
        const int stepx = TDP_PARTS % L, stepy = TDP_PARTS / L;
        for (int B = part; B < N; B += TDP_PARTS) {
            int ax = bx + dx, ay = by + dy;
            if (ax >= L) ax -= L;
            if (ay >= L) ay -= L;
            const int A = ay * L + ax;
            const cplx* pe = gs + (size_t)B * ng + (size_t)A;     // e_rc = gs(A + N r; B + N c) = pe[c N ng + r N]
            const cplx* pt = gs + (size_t)A * ng + (size_t)B;     // t_rc = gs(B + N c; A + N r) = pt[r N ng + c N]
            // disconnected parts
            const cplx ocB = ob[B];
            double dc = re_mul(ob[A], ocB), dz = re_mul(ob[N + A], ob[N + B]);
            double ds = re_mul(ob[2 * N + A], ob[2 * N + B]);
            if (OPDIM >= 2) ds += re_mul(ob[3 * N + A], ob[3 * N + B]);
            if (OPDIM == 3) ds += re_mul(ob[4 * N + A], ob[4 * N + B]);
            ds *= 1.0 / OPDIM;
            if (d == 0) {                                   // the delta term: tr_4 gs(B; B) for M^2 = 1
                const double tr = 4.0 - ocB.x;
                dc += tr; dz += 0.25 * tr; ds += tr;
            }
            double cc, cz, cs2, pxx, pxy, pyx, pyy;
            if (OPDIM == 3) {
                cplx e[4][4];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[r][c2] = pe[(size_t)c2 * N * ng + (size_t)r * N];
                // Re P(b1, b2) with (dn1, up1) = band-spin rows of band b1, (up2, dn2) = band-spin columns of band b2
                auto P = [&](int dn1, int up1, int up2, int dn2) { return re_mul(e[dn1][up2], e[up1][dn2]) - re_mul(e[dn1][dn2], e[up1][up2]); };
                pxx = P(2, 0, 0, 2); pxy = P(2, 0, 3, 1); pyx = P(1, 3, 0, 2); pyy = P(1, 3, 3, 1);
                constexpr int pxyp[4] = {1, 0, 3, 2}, pz[4] = {3, 2, 1, 0};
                constexpr double sz[4] = {1.0, -1.0, -1.0, 1.0};      // spinZ diagonal (x 2), the y of M_y and the m of M_z alike
                cc = 0.0; cz = 0.0;
                double cx = 0.0, cy = 0.0, cq = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    cplx t[4];                                        // t[dl] = gs(B dl; A a)
#pragma unroll
                    for (int dl = 0; dl < 4; ++dl) t[dl] = pt[(size_t)a * N * ng + (size_t)dl * N];
#pragma unroll
                    for (int c2 = 0; c2 < 4; ++c2) {
                        const double v = re_mul(e[a][c2], t[c2]);
                        cc += v;
                        cz += sz[a] * sz[c2] * v;
                        const double q = re_mul(e[pxyp[a]][c2], t[pxyp[c2]]);
                        cx += q;
                        cy += sz[a] * sz[c2] * q;                    // m_a m_c = -y_a y_c with y = -sz
                        cq += sz[a] * sz[c2] * re_mul(e[pz[a]][c2], t[pz[c2]]);
                    }
                }
                cz *= 0.25;
                cs2 = (cx - cy) + cq;
            } else {
                const size_t cN = (size_t)N * ng;
                const cplx e00 = pe[0], e10 = pe[N], e01 = pe[cN], e11 = pe[cN + N];
                const cplx t00 = pt[0], t10 = pt[cN], t01 = pt[N], t11 = pt[cN + N];
                const double d00 = re_mul(e00, t00), d11 = re_mul(e11, t11), d01 = re_mul(e01, t01), d10 = re_mul(e10, t10);
                cc = 2.0 * ((d00 + d11) + (d01 + d10));
                cz = 0.5 * ((d00 + d11) - (d01 + d10));
                const double q01 = re_mul(e11, t00), q10 = re_mul(e00, t11);
                if (OPDIM == 1) cs2 = 2.0 * ((re_mul(e10, t01) + re_mul(e01, t10)) + (q01 + q10));
                else cs2 = 4.0 * (q01 + q10);                        // M_x + M_y: the q_00 and q_11 terms cancel
                pxx = -abs2(e00); pxy = abs2(e01); pyx = abs2(e10); pyy = -abs2(e11);
            }
            wc += dc - cc;
            wz += dz - cz;
            ws += ds - cs2 * (1.0 / OPDIM);
            tp += -4.0 * (((pxx + pxy) + pyx) + pyy);
            tm += -4.0 * (((pxx - pxy) - pyx) + pyy);
            bx += stepx; by += stepy;
            if (bx >= L) { bx -= L; ++by; }
        }
    }
    red[0][part][lb] = wc;
    red[1][part][lb] = wz;
    red[2][part][lb] = ws;
    red[3][part][lb] = tp;
    red[4][part][lb] = tm;
    __syncthreads();
    if (part < EQ_CH && valid) {                            // part c writes channel c of its bin
        double s = red[part][0][lb];
#pragma unroll
        for (int q = 1; q < TDP_PARTS; ++q) s += red[part][q][lb];
        acc[1 + (size_t)part * N + d] += s;
    }
    if (blockIdx.x == 0 && tid == 0) acc[0] += 1.0;
}

void launch_measure_eq_corr(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, double* acc) {
    const dim3 g1((hm.N + 255) / 256, 1, lc.nb);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_eq_onebody<decltype(O)::value>), g1, dim3(256), 0, lc.st, hm, gs, ob, lc.cs);
        hipLaunchKernelGGL((k_measure_eq_corr<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, ob, acc, lc.cs);
    });
}

// Time-displaced current-current block (dqmc_measure_timedisplaced_current; definitions in dqmc_hip.h and DESIGN.md 6e).  A bond operator
// at site i in direction mu (i' = i (+) mu) has two one-body entries per flavour, M[i' a, i a] = m_a(i), M[i a, i' a] = conj m_a(i), with
// m = i T (current j_mu) or m = T (bond kinetic energy k_mu) and T_a(i) = K^a[i', i] from the bond table bt[mu][flavour][site].  With
// A^1 = A', A^0 = A, m_1 = m, m_0 = conj m the general Wick form reduces to
//   o_t(A)     = - sum_a [ m_a(A) g_t(A a; A' a) + conj m_a(A) g_t(A' a; A a) ]
//   conn(A, B) = sum_{a b} sum_{u v} m_u^a(A) m_v^b(B) g0t(B^(1-v) b; A^u a) gt0(A^(1-u) a; B^v b),      g0t(B b; A a) = conj hs(A a; B b).
// For the current, with c = T_a(A) T_b(B), d = T_a(A) conj T_b(B) and P_uv = conj hs(A^u a; B^(1-v) b) gt0(A^(1-u) a; B^v b):
//   Re conn = sum_{a b} [ -Re c P_11 + Re d P_10 + Re conj(d) P_01 - Re conj(c) P_00 ].
// Both directions of one (A, B, a, b) read gt0 and hs at the rows {A, Ax, Ay} x columns {B, Bx, By} without (Ax, By), (Ay, Bx): seven
// elements of each matrix.  OPDIM < 3: M is flavour diagonal and the conjugate sector carries -conj(M) for j, +conj(M) for k, while both
// matrices are diag(stored sector, its conjugate): the second sector contributes the complex conjugate of the first, so
//   Re conn = 2 Re conn_stored,   o[j] = -2 i Re sum_stored (x - y),   o[k] = -2 Re sum_stored (x + y),   x = T g(A; A'), y = conj T g(A'; A),
// and nothing is multiplied by a structural zero.  O(3) runs over the full 4 x 4 flavour pairs.
// Reuse instead of an LDS tile: the lanes of a half wave hold consecutive A of one column B, so
// Ax is the neighbouring 16 bytes of the same cache lines and Ay the row L further down the same column, which the lane of bin d + L reads
// in the same step; column Bx is the column of part + 1 of the same step and By the column this workgroup walks one (L / 8 steps) later:
// every re-read is served by the CU's L1 or the XCD's L2, and each matrix leaves HBM once per launch.
// Workgroup 0 also sums Re o_tau[k_mu] over the sites (fixed tree), the diamagnetic term.
size_t measure_td_current_doubles(int N, int n) { return (size_t)(n - 1) * (1 + 2 * (size_t)N + 2); }

#define TDC_OB 4        // one-body values per site and time: j_x, j_y, k_x, k_y
size_t measure_td_current_onebody_cplx(int N) { return (size_t)2 * TDC_OB * N; }
size_t measure_td_current_bond_cplx(int N, int opdim) { return (size_t)2 * (opdim == 3 ? 4 : 2) * N; }

// ob[t][j_x, j_y, k_x, k_y][site] for one of the two equal-time matrices (t = 0: G(tau_j), t = 1: G(0)); gs is its shifted form
template<int OPDIM>
__global__ __launch_bounds__(256) void k_td_current_onebody(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ bt,
                                                            cplx* __restrict__ ob, int t, size_t cs) {
    CHAIN(gs); CHAIN(ob);
    constexpr int MSF = OPDIM == 3 ? 4 : 2;
    const int N = dm.N, L = dm.L, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    const size_t ng = (size_t)dm.ng;
    const int ax = A % L, ay = A / L;
    cplx* o = ob + (size_t)t * TDC_OB * N + A;
#pragma unroll
    for (int mu = 0; mu < 2; ++mu) {
        const int An = mu == 0 ? ay * L + (ax + 1 == L ? 0 : ax + 1) : (ay + 1 == L ? 0 : ay + 1) * L + ax;
        cplx sm = make_double2(0.0, 0.0), sp = make_double2(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < MSF; ++a) {
            const cplx T = bt[(size_t)(mu * MSF + a) * N + A];
            const cplx x = m_mul(T, gs[(size_t)(An + N * a) * ng + A + N * a]);               // T g(A a; A' a)
            const cplx y = m_mul(m_conj(T), gs[(size_t)(A + N * a) * ng + An + N * a]);       // conj T g(A' a; A a)
            sm = m_add(sm, m_sub(x, y));
            sp = m_add(sp, m_add(x, y));
        }
        if (OPDIM == 3) {
            o[(size_t)mu * N] = make_double2(sm.y, -sm.x);                                    // -i sum (x - y)
            o[(size_t)(2 + mu) * N] = make_double2(-sp.x, -sp.y);
        } else {
            o[(size_t)mu * N] = make_double2(0.0, -2.0 * sm.x);
            o[(size_t)(2 + mu) * N] = make_double2(-2.0 * sp.x, 0.0);
        }
    }
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_current(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ hs,
                                                                             const cplx* __restrict__ bt, const cplx* __restrict__ ob,
                                                                             double* __restrict__ acc, int row, int rows, size_t cs) {
    CHAIN(gs); CHAIN(hs); CHAIN(ob); CHAIN(acc);
    constexpr int MSF = OPDIM == 3 ? 4 : 2;
    __shared__ double red[2][TDP_PARTS][TDP_BINS];
    __shared__ double redk[TDP_BINS * TDP_PARTS];
    const int N = dm.N, L = dm.L, tid = threadIdx.x;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    const cplx* ot = ob;                                    // o_tau(A)
    const cplx* o0 = ob + (size_t)TDC_OB * N;               // o_0(B)
    auto hce = [](cplx h, cplx e) { return make_double2(h.x * e.x + h.y * e.y, h.x * e.y - h.y * e.x); };      // conj(h) e
    double wx = 0.0, wy = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        // element offsets of the x and y neighbours: rows of A, columns of B
        const ptrdiff_t rx = st.ax + 1 == L ? 1 - L : 1, ry = st.ay + 1 == L ? (ptrdiff_t)L - N : L;
        const ptrdiff_t cx = (ptrdiff_t)(st.bx + 1 == L ? 1 - L : 1) * (ptrdiff_t)ng, cy = (ptrdiff_t)(st.by + 1 == L ? L - N : L) * (ptrdiff_t)ng;
        double sx = m_re_mul(ot[A], o0[B]), sy = m_re_mul(ot[N + A], o0[N + B]);      // disconnected parts
        double kx = 0.0, ky = 0.0;                                                    // connected parts
#pragma unroll
        for (int a = 0; a < MSF; ++a) {
            const cplx tax = bt[(size_t)a * N + A], tay = bt[(size_t)(MSF + a) * N + A];
#pragma unroll
            for (int b = 0; b < MSF; ++b) {
                const cplx tbx = bt[(size_t)b * N + B], tby = bt[(size_t)(MSF + b) * N + B];
                const size_t off = (size_t)(B + N * b) * ng + (size_t)(A + N * a);
                const cplx* pe = gs + off;
                const cplx* ph = hs + off;
                const cplx e00 = pe[0], h00 = ph[0];
                {   // mu = x: rows {A, Ax}, columns {B, Bx}
                    const cplx e10 = pe[rx], e01 = pe[cx], e11 = pe[rx + cx];
                    const cplx h10 = ph[rx], h01 = ph[cx], h11 = ph[rx + cx];
                    const cplx c = m_mul(tax, tbx), dd = m_mul(tax, m_conj(tbx));
                    // P_uv = conj hs(A^u; B^(1-v)) gt0(A^(1-u); B^v)
                    const cplx p11 = hce(h10, e01), p10 = hce(h11, e00), p01 = hce(h00, e11), p00 = hce(h01, e10);
                    kx += (m_re_mul(dd, p10) + m_re_mul(m_conj(dd), p01)) - (m_re_mul(c, p11) + m_re_mul(m_conj(c), p00));
                }
                {   // mu = y: rows {A, Ay}, columns {B, By}
                    const cplx e10 = pe[ry], e01 = pe[cy], e11 = pe[ry + cy];
                    const cplx h10 = ph[ry], h01 = ph[cy], h11 = ph[ry + cy];
                    const cplx c = m_mul(tay, tby), dd = m_mul(tay, m_conj(tby));
                    const cplx p11 = hce(h10, e01), p10 = hce(h11, e00), p01 = hce(h00, e11), p00 = hce(h01, e10);
                    ky += (m_re_mul(dd, p10) + m_re_mul(m_conj(dd), p01)) - (m_re_mul(c, p11) + m_re_mul(m_conj(c), p00));
                }
            }
        }
        if (OPDIM < 3) { kx *= 2.0; ky *= 2.0; }
        wx += sx - kx;
        wy += sy - ky;
    }
    double* blk = acc + rows + (size_t)row * (2 * (size_t)N + 2);
    const double w[2] = {wx, wy};                           // Lambda_xx, Lambda_yy
    bw.reduce_add(w, red, 2, blk, N, 1, nullptr);           // the count goes with the site sum below
    if (blockIdx.x == 0) {                                  // sum_A Re o_tau[k_mu(A)]
        double vx = 0.0, vy = 0.0;
        for (int A = tid; A < N; A += TDP_BINS * TDP_PARTS) { vx += ot[2 * N + A].x; vy += ot[3 * N + A].x; }
        vx = block_sum(vx, redk);
        vy = block_sum(vy, redk);
        if (tid == 0) {
            blk[2 * (size_t)N] += vx;
            blk[2 * (size_t)N + 1] += vy;
            acc[row] += 1.0;
        }
    }
}

void launch_td_current_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* bt, cplx* ob, int t) {
    const dim3 grid((hm.N + 255) / 256, 1, lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_td_current_onebody<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, gs, bt, ob, t, lc.cs);
    });
}

void launch_measure_td_current(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* bt, const cplx* ob, double* acc, int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_current<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, hs, bt, ob, acc, row, rows, lc.cs);
    });
}

// Band-resolved charge channels (dqmc_measure_timedisplaced_band, dqmc_set_equal_time_band; definitions in dqmc_hip.h and DESIGN.md 6e):
// the W^M(A, B) of k_measure_td_ph for the two spin-singlet bilinears
//   bandDiff  M_BAND = diag(+1, -1, +1, -1)                       n_x - n_y:  pi = identity, m = (+1, -1, +1, -1)
//   bandMix   M_MIX:  (0,3) = (3,0) = (1,2) = (2,1) = +1          sum_s psi^+_xs psi_ys + h.c.:  pi = (3, 2, 1, 0), m = 1
// in the one-entry-per-row form of that kernel, connected part sum_{a, c} m_a m_c gt0(A pi(a); B c) g0t(B pi(c); A a), and with the same
// prepared operands gs = shifted G(tau, 0), hs = (shifted G(0, tau))^H.  tr M = 0 for both.
// OPDIM < 3, with e_rc, h_rc and d_rc = Re e_rc conj h_rc of k_measure_td_ph:
//   bandDiff is sector diagonal with the sign pattern (+, -) inside BOTH sectors, so the conjugate sector doubles the stored one:
//     connected = 2 (d_00 + d_11 - d_01 - d_10)  (four times that of spinZ),   o = -2 Re (g_00 - g_11)  (spinZ: -i Im of the same number);
//   bandMix couples the stored sector to its conjugate: M_MIX g has no diagonal block, o = 0 exactly (written, not computed), and every
//   connected term takes one element of each sector -- e(A pi(a); B c) from the sector opposite to a, h(A a; B pi(c)) from a's own:
//     a in the stored sector:     conj e_(1-a)(1-c) conj h_a c,     a in the conjugate sector:  e_(1-a)(1-c) h_a c      (same real part)
//     connected = 2 Re (e_10 h_01 + e_11 h_00 + e_00 h_11 + e_01 h_10).
//   The eight loads of k_measure_td_ph serve both sums; nothing is multiplied by a structural zero.
// O(3): the sixteen e and sixteen h of the full blocks.
#define TDB_CH 2        // one-body values per site and time: bandDiff, bandMix
size_t measure_td_band_doubles(int N, int n) { return (size_t)(n - 1) * (1 + 2 * (size_t)N); }
size_t measure_td_band_onebody_cplx(int N) { return (size_t)2 * TDB_CH * N; }

// the two one-body values of site A from the shifted equal-time matrix gs
template<int OPDIM>
__device__ __forceinline__ void band_onebody(const cplx* __restrict__ gs, int ng, int N, int A, cplx& ob, cplx& om) {
    const cplx* p = gs + (size_t)A * ng + A;                // g(r, c) = gs(A r; A c) = p[c N ng + r N]
    const size_t cN = (size_t)N * ng;
    if (OPDIM == 3) {
        const cplx v = m_add(m_sub(p[0], p[cN + N]), m_sub(p[2 * cN + 2 * N], p[3 * cN + 3 * N]));
        ob = make_double2(-v.x, -v.y);
        const cplx w = m_add(m_add(p[3 * N], p[3 * cN]), m_add(p[cN + 2 * N], p[2 * cN + N]));      // g(3,0) + g(0,3) + g(2,1) + g(1,2)
        om = make_double2(-w.x, -w.y);
    } else {
        ob = make_double2(-2.0 * (p[0].x - p[cN + N].x), 0.0);
        om = make_double2(0.0, 0.0);
    }
}

// ob[t][bandDiff, bandMix][site] for one of the two equal-time matrices (t = 0: G(tau), t = 1: G(0)); gs is its shifted form
template<int OPDIM>
__global__ __launch_bounds__(256) void k_td_band_onebody(DevModel dm, const cplx* __restrict__ gs, cplx* __restrict__ ob, int t, size_t cs) {
    CHAIN(gs); CHAIN(ob);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx vb, vm;
    band_onebody<OPDIM>(gs, dm.ng, N, A, vb, vm);
    cplx* o = ob + (size_t)t * TDB_CH * N + A;
    o[0] = vb;
    o[(size_t)N] = vm;
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_band(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ hs,
                                                                          const cplx* __restrict__ ob, double* __restrict__ acc, int row, int rows, size_t cs) {
    CHAIN(gs); CHAIN(hs); CHAIN(ob); CHAIN(acc);
    __shared__ double red[TDB_CH][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    const cplx* ot = ob;                                    // o_tau(A)
    const cplx* o0 = ob + (size_t)TDB_CH * N;               // o_0(B)
    double wb = 0.0, wm = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        const size_t off = (size_t)B * ng + (size_t)A;
        const cplx* pe = gs + off;
        const cplx* ph = hs + off;
        double db, dmx, cb, cm;
        if (OPDIM == 3) {
            db = m_re_mul(ot[A], o0[B]);
            dmx = m_re_mul(ot[N + A], o0[N + B]);
            cplx e[4][4];
            m_load_block(pe, ng, N, e);
            constexpr int pz[4] = {3, 2, 1, 0};
            constexpr double sb[4] = {1.0, -1.0, 1.0, -1.0};
            cb = 0.0; cm = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                cplx h[4];                                        // h[dl] = hs(A a; B dl)
#pragma unroll
                for (int dl = 0; dl < 4; ++dl) h[dl] = ph[(size_t)dl * N * ng + (size_t)a * N];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) {
                    cb += sb[a] * sb[c2] * m_re_mulc(e[a][c2], h[c2]);
                    cm += m_re_mulc(e[pz[a]][c2], h[pz[c2]]);
                }
            }
        } else {
            db = ot[A].x * o0[B].x;                              // both real; the bandMix values are exact zeros
            dmx = 0.0;
            const size_t cN = (size_t)N * ng;
            const cplx e00 = pe[0], e10 = pe[N], e01 = pe[cN], e11 = pe[cN + N];
            const cplx h00 = ph[0], h10 = ph[N], h01 = ph[cN], h11 = ph[cN + N];
            const double d00 = m_re_mulc(e00, h00), d11 = m_re_mulc(e11, h11), d01 = m_re_mulc(e01, h01), d10 = m_re_mulc(e10, h10);
            cb = 2.0 * ((d00 + d11) - (d01 + d10));
            cm = 2.0 * ((m_re_mul(e10, h01) + m_re_mul(e01, h10)) + (m_re_mul(e11, h00) + m_re_mul(e00, h11)));
        }
        wb += db - cb;
        wm += dmx - cm;
    }
    const double w[TDB_CH] = {wb, wm};                      // bandDiff, bandMix
    bw.reduce_add(w, red, TDB_CH, acc + rows + (size_t)row * TDB_CH * N, N, 1, acc + row);
}

void launch_td_band_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, int t) {
    const dim3 grid((hm.N + 255) / 256, 1, lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_td_band_onebody<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, gs, ob, t, lc.cs);
    });
}

void launch_measure_td_band(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* ob, double* acc, int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_band<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, hs, ob, acc, row, rows, lc.cs);
    });
}

// Equal-time form (dqmc_set_equal_time_band): one matrix gs in both roles as in k_measure_eq_corr, the transposed factor read in place,
// t_ac = gs[(A + N a) ng + B + N c] for conj hs(A a; B c): Re e conj h -> Re e t, and in the bandMix sum of OPDIM < 3, where the two
// factors come from opposite sectors, Re e h -> Re e conj t.  M^2 = 1 for both matrices: the delta term tr_4 gs(B; B) goes to the d = 0
// bin from the third one-body value.  ob[chain][bandDiff, bandMix, tr_4 gs][N]; block of one chain: count, bandDiff[N], bandMix[N], both
// plain device arrays outside the arena.
#define EQB_OB 3
size_t measure_eq_band_doubles(int N) { return 1 + (size_t)TDB_CH * N; }
size_t measure_eq_band_onebody_cplx(int N) { return (size_t)EQB_OB * N; }

template<int OPDIM>
__global__ __launch_bounds__(256) void k_eq_band_onebody(DevModel dm, const cplx* __restrict__ gs, cplx* __restrict__ ob, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx vb, vm;
    band_onebody<OPDIM>(gs, dm.ng, N, A, vb, vm);
    const cplx* p = gs + (size_t)A * dm.ng + A;
    const size_t cN = (size_t)N * dm.ng;
    cplx tr;
    if (OPDIM == 3) tr = m_add(m_add(p[0], p[cN + N]), m_add(p[2 * cN + 2 * N], p[3 * cN + 3 * N]));
    else tr = make_double2(2.0 * (p[0].x + p[cN + N].x), 0.0);
    cplx* o = ob + (size_t)blockIdx.z * EQB_OB * N + A;
    o[0] = vb;
    o[(size_t)N] = vm;
    o[(size_t)2 * N] = tr;
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_eq_band(DevModel dm, const cplx* __restrict__ gs, const cplx* __restrict__ ob,
                                                                          double* __restrict__ acc, size_t cs) {
    CHAIN(gs);
    ob += (size_t)blockIdx.z * EQB_OB * dm.N;
    acc += (size_t)blockIdx.z * (1 + (size_t)TDB_CH * dm.N);
    __shared__ double red[TDB_CH][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    double wb = 0.0, wm = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        const cplx* pe = gs + (size_t)B * ng + (size_t)A;     // e_rc = gs(A + N r; B + N c) = pe[c N ng + r N]
        const cplx* pt = gs + (size_t)A * ng + (size_t)B;     // t_rc = gs(B + N c; A + N r) = pt[r N ng + c N]
        double db, dmx, cb, cm;
        if (OPDIM == 3) {
            db = m_re_mul(ob[A], ob[B]);
            dmx = m_re_mul(ob[N + A], ob[N + B]);
            cplx e[4][4];
            m_load_block(pe, ng, N, e);
            constexpr int pz[4] = {3, 2, 1, 0};
            constexpr double sb[4] = {1.0, -1.0, 1.0, -1.0};
            cb = 0.0; cm = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                cplx t[4];                                        // t[dl] = gs(B dl; A a)
#pragma unroll
                for (int dl = 0; dl < 4; ++dl) t[dl] = pt[(size_t)a * N * ng + (size_t)dl * N];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) {
                    cb += sb[a] * sb[c2] * m_re_mul(e[a][c2], t[c2]);
                    cm += m_re_mul(e[pz[a]][c2], t[pz[c2]]);
                }
            }
        } else {
            db = ob[A].x * ob[B].x;                              // both real; the bandMix values are exact zeros
            dmx = 0.0;
            const size_t cN = (size_t)N * ng;
            const cplx e00 = pe[0], e10 = pe[N], e01 = pe[cN], e11 = pe[cN + N];
            const cplx t00 = pt[0], t10 = pt[cN], t01 = pt[N], t11 = pt[cN + N];
            const double d00 = m_re_mul(e00, t00), d11 = m_re_mul(e11, t11), d01 = m_re_mul(e01, t01), d10 = m_re_mul(e10, t10);
            cb = 2.0 * ((d00 + d11) - (d01 + d10));
            cm = 2.0 * ((m_re_mulc(e10, t01) + m_re_mulc(e01, t10)) + (m_re_mulc(e11, t00) + m_re_mulc(e00, t11)));
        }
        if (bw.d == 0) {                                // the delta term: tr_4 gs(B; B) for M^2 = 1
            const double tr = ob[2 * N + B].x;
            db += tr; dmx += tr;
        }
        wb += db - cb;
        wm += dmx - cm;
    }
    const double w[TDB_CH] = {wb, wm};                      // bandDiff, bandMix
    bw.reduce_add(w, red, TDB_CH, acc + 1, N, 1, acc);
}

void launch_measure_eq_band(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, double* acc) {
    const dim3 g1((hm.N + 255) / 256, 1, lc.nb);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_eq_band_onebody<decltype(O)::value>), g1, dim3(256), 0, lc.st, hm, gs, ob, lc.cs);
        hipLaunchKernelGGL((k_measure_eq_band<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, ob, acc, lc.cs);
    });
}

// User-defined bilinears (dqmc_set_custom_bilinears; definitions in dqmc_hip.h and DESIGN.md 6e): the W^M(A, B) of k_measure_td_ph for up to
// DQMC_CUSTOM_MAX Hermitian 4 x 4 matrices that arrive as a kernel argument, all channels in ONE launch.  Per site pair the blocks
//   E_bc = g~(tau,0)(A b; B c)      and      T_da = g~(0,tau)(B d; A a) = conj hs(A a; B d)
// are loaded once (4 + 4 complex for OPDIM < 3, 16 + 16 for O(3)); the connected part of a channel is Re tr(M E M T), formed for a = 0 .. 3
// from row a of M E and column a of M T.  OPDIM < 3: only the (XUP, YDOWN) sector is stored, the (XDOWN, YUP) sector is its complex
// conjugate and the blocks between the sectors vanish (GreenAccess), which cst_E / cst_same resolve at compile time after unrolling -- a
// matrix that couples the sectors is as legal as any other.  A 16-bit mask per channel (bit 4 a + b: M_ab != 0) skips the structural
// zeros; it is uniform over the launch, so no wave diverges.  The blocks and the one-body scratch live outside the arena: chain b at
// acc + b * acs and ob + b * obs.
struct CustomMats { cplx m[DQMC_CUSTOM_MAX][4][4]; unsigned mask[DQMC_CUSTOM_MAX]; int count; };
size_t measure_custom_row_doubles(int count, int N) { return (size_t)count * N; }
size_t measure_td_custom_onebody_cplx(int count, int N) { return (size_t)2 * count * N; }
size_t measure_eq_custom_onebody_cplx(int count, int N) { return (size_t)2 * count * N; }

template<int OPDIM> __device__ __forceinline__ constexpr bool cst_same(int r, int c) { return OPDIM == 3 || ((r < 2) == (c < 2)); }
// element (r, c), r and c in the same sector, of the full 4 x 4 block whose stored part is x
template<int OPDIM, int R>
__device__ __forceinline__ cplx cst_E(const cplx (&x)[R][R], int r, int c) {
    if (OPDIM == 3 || r < 2) return x[r & (R - 1)][c & (R - 1)];
    const cplx v = x[r - 2][c - 2];
    return make_double2(v.x, -v.y);
}
__device__ __forceinline__ void cst_fma(cplx& acc, cplx a, cplx b) {
    acc.x = fma(a.x, b.x, fma(-a.y, b.y, acc.x));
    acc.y = fma(a.x, b.y, fma(a.y, b.x, acc.y));
}
// Re tr(M E M T); e[r][c] = E_rc, t[r][c] = T_rc of the stored part
template<int OPDIM, int R>
__device__ __forceinline__ double cst_connected(const cplx (&e)[R][R], const cplx (&t)[R][R], const cplx (&M)[4][4], unsigned mask) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        cplx x[4], y[4];                                    // x[c] = (M E)_ac, y[c] = (M T)_ca
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) x[c2] = y[c2] = make_double2(0.0, 0.0);
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (mask & (1u << (4 * a + b))) {
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2)
                    if (cst_same<OPDIM>(b, c2)) cst_fma(x[c2], M[a][b], cst_E<OPDIM, R>(e, b, c2));
            }
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
            for (int dl = 0; dl < 4; ++dl)
                if (cst_same<OPDIM>(dl, a) && (mask & (1u << (4 * c2 + dl)))) cst_fma(y[c2], M[c2][dl], cst_E<OPDIM, R>(t, dl, a));
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) s += x[c2].x * y[c2].x - x[c2].y * y[c2].y;
    }
    return s;
}
// tr M - sum_ab M_ab g(A b; A a) of site A from the shifted equal-time matrix gs; with tr M = 0 handed in: -sum_ab M_ab g(A b; A a)
template<int OPDIM>
__device__ __forceinline__ cplx cst_onebody(const cplx* __restrict__ gs, int ng, int N, int A, const cplx (&M)[4][4], unsigned mask, bool with_trace) {
    constexpr int R = OPDIM == 3 ? 4 : 2;
    cplx g[R][R];                                           // g(r, c) = gs(A r; A c)
    m_load_block(gs, (size_t)ng, N, A, A, g);
    cplx v = make_double2(0.0, 0.0);
    if (with_trace) v = m_add(m_add(M[0][0], M[1][1]), m_add(M[2][2], M[3][3]));
    cplx s = make_double2(0.0, 0.0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (cst_same<OPDIM>(b, a) && (mask & (1u << (4 * a + b)))) cst_fma(s, M[a][b], cst_E<OPDIM, R>(g, b, a));
    return m_sub(v, s);
}

// ob[chain][t][channel][site] for one of the two equal-time matrices (t = 0: G(tau), t = 1: G(0)); gs is its shifted form
template<int OPDIM>
__global__ __launch_bounds__(256) void k_td_custom_onebody(DevModel dm, CustomMats cm, const cplx* __restrict__ gs, cplx* __restrict__ ob, int t,
                                                           size_t obs, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx* o = ob + (size_t)blockIdx.z * obs + (size_t)t * cm.count * N + A;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
        if (ch < cm.count) o[(size_t)ch * N] = cst_onebody<OPDIM>(gs, dm.ng, N, A, cm.m[ch], cm.mask[ch], true);
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_custom(DevModel dm, CustomMats cm, const cplx* __restrict__ gs,
                                                                            const cplx* __restrict__ hs, const cplx* __restrict__ ob,
                                                                            double* __restrict__ acc, int row, int rows, size_t obs, size_t acs, size_t cs) {
    CHAIN(gs); CHAIN(hs);
    constexpr int R = OPDIM == 3 ? 4 : 2;
    ob += (size_t)blockIdx.z * obs;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, count = cm.count;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    const cplx* ot = ob;                                    // o_tau(A)
    const cplx* o0 = ob + (size_t)count * N;                // o_0(B)
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        const size_t off = (size_t)B * ng + (size_t)A;
        const cplx* ph = hs + off;
        cplx e[R][R], t[R][R];
        m_load_block(gs + off, ng, N, e);
#pragma unroll
        for (int c2 = 0; c2 < R; ++c2)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const cplx h = ph[(size_t)c2 * N * ng + (size_t)r * N];      // hs(A r; B c2) = conj T_(c2 r)
                t[c2][r] = make_double2(h.x, -h.y);
            }
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
            if (ch < count) {
                const cplx a = ot[(size_t)ch * N + A], b = o0[(size_t)ch * N + B];
                w[ch] += (a.x * b.x - a.y * b.y) - cst_connected<OPDIM, R>(e, t, cm.m[ch], cm.mask[ch]);
            }
    }
    bw.reduce_add(w, red, count, acc + rows + (size_t)row * count * N, N, 1, acc + row);
}

// the stencil kernels of the bond parts, further down
static void launch_td_custom_bond_onebody(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, cplx* ob, int t);
static void launch_measure_td_custom_bond(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, const cplx* hs,
                                          const cplx* ob, double* acc, size_t acs, int row, int rows);
static void launch_measure_eq_custom_bond(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, cplx* ob, double* acc);

static CustomMats custom_mats(int count, const cplx* M, const unsigned* mask) {
    CustomMats cm{};
    cm.count = count;
    for (int ch = 0; ch < count; ++ch) {
        cm.mask[ch] = mask[ch];
        for (int k = 0; k < 16; ++k) cm.m[ch][k / 4][k % 4] = M[16 * ch + k];
    }
    return cm;
}

void launch_td_custom_onebody(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* gs, cplx* ob, int t,
                              const CustomBond* bond) {
    if (bond) return launch_td_custom_bond_onebody(lc, hm, count, *bond, gs, ob, t);
    const CustomMats cm = custom_mats(count, M, mask);
    const dim3 grid((hm.N + 255) / 256, 1, lc.nb);
    const size_t obs = measure_td_custom_onebody_cplx(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_td_custom_onebody<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, cm, gs, ob, t, obs, lc.cs);
    });
}

void launch_measure_td_custom(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* gs, const cplx* hs,
                              const cplx* ob, double* acc, size_t acs, int row, int rows, const CustomBond* bond) {
    if (bond) return launch_measure_td_custom_bond(lc, hm, count, *bond, gs, hs, ob, acc, acs, row, rows);
    const CustomMats cm = custom_mats(count, M, mask);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    const size_t obs = measure_td_custom_onebody_cplx(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_custom<decltype(O)::value>), grid, block, 0, lc.st, hm, cm, gs, hs, ob, acc, row, rows, obs, acs, lc.cs);
    });
}

// Equal-time form (dqmc_set_equal_time_custom): one matrix gs in both roles as in k_measure_eq_band, the transposed factor read in place,
// T_da = gs(B d; A a) = gs[(A + N a) ng + B + N d].  M^2 = 1 is not assumed: the delta term sum_bc (M^2)_cb gs(B b; B c) goes to the d = 0
// bin from a one-body value of its own, formed with M^2 (cm2, trace left out) by the routine that forms o^M.
// ob[chain][o^M: count][delta: count][N]; block of one chain: count, then the channels [N] each.
template<int OPDIM>
__global__ __launch_bounds__(256) void k_eq_custom_onebody(DevModel dm, CustomMats cm, CustomMats cm2, const cplx* __restrict__ gs, cplx* __restrict__ ob,
                                                           size_t obs, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx* o = ob + (size_t)blockIdx.z * obs + A;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
        if (ch < cm.count) {
            o[(size_t)ch * N] = cst_onebody<OPDIM>(gs, dm.ng, N, A, cm.m[ch], cm.mask[ch], true);
            const cplx dl = cst_onebody<OPDIM>(gs, dm.ng, N, A, cm2.m[ch], cm2.mask[ch], false);     // -sum_bc (M^2)_cb gs(A b; A c)
            o[(size_t)(cm.count + ch) * N] = make_double2(-dl.x, -dl.y);
        }
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_eq_custom(DevModel dm, CustomMats cm, const cplx* __restrict__ gs,
                                                                            const cplx* __restrict__ ob, double* __restrict__ acc, size_t obs, size_t acs,
                                                                            size_t cs) {
    CHAIN(gs);
    constexpr int R = OPDIM == 3 ? 4 : 2;
    ob += (size_t)blockIdx.z * obs;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, count = cm.count;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        cplx e[R][R], t[R][R];
        m_load_block(gs, ng, N, A, B, e);                   // E_rc = gs(A r; B c)
        m_load_block(gs, ng, N, B, A, t);                   // T_rc = gs(B r; A c)
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
            if (ch < count) {
                const cplx a = ob[(size_t)ch * N + A], b = ob[(size_t)ch * N + B];
                double v = (a.x * b.x - a.y * b.y) - cst_connected<OPDIM, R>(e, t, cm.m[ch], cm.mask[ch]);
                if (bw.d == 0) v += ob[(size_t)(count + ch) * N + B].x;      // the delta term
                w[ch] += v;
            }
    }
    bw.reduce_add(w, red, count, acc + 1, N, 1, acc);
}

void launch_measure_eq_custom(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* M2, const unsigned* mask2,
                              const cplx* gs, cplx* ob, double* acc, const CustomBond* bond) {
    if (bond) return launch_measure_eq_custom_bond(lc, hm, count, *bond, gs, ob, acc);
    const CustomMats cm = custom_mats(count, M, mask), cm2 = custom_mats(count, M2, mask2);
    const dim3 g1((hm.N + 255) / 256, 1, lc.nb);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    const size_t obs = measure_eq_custom_onebody_cplx(count, hm.N), acs = 1 + measure_custom_row_doubles(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_eq_custom_onebody<decltype(O)::value>), g1, dim3(256), 0, lc.st, hm, cm, cm2, gs, ob, obs, lc.cs);
        hipLaunchKernelGGL((k_measure_eq_custom<decltype(O)::value>), grid, block, 0, lc.st, hm, cm, gs, ob, acc, obs, acs, lc.cs);
    });
}

// Bond parts of the user-defined bilinears (dqmc_set_custom_bond_bilinears; definitions in dqmc_hip.h and DESIGN.md 6e).  As a one-body
// matrix over (site, flavour) operator O_A has five 4 x 4 site blocks V_k(A) = f_k(A) W_k between the stencil sites A, Ax = A (+) x,
// Ay = A (+) y:
//   k    block (p, q)   W_k     f_k(A)              p: site of c^+, q: site of c
//   0    (A,  A)        M0      1
//   1    (Ax, A)        Mx      u_x(A)
//   2    (A,  Ax)       Mx^H    conj u_x(A)
//   3    (Ay, A)        My      u_y(A)
//   4    (A,  Ay)       My^H    conj u_y(A)
// u the link factor of the stored sector; the conjugate sector carries conj u, which is the stored-sector / conjugate-sector rule of cst_E
// once the factor multiplies the stored part of a block of g (with flux u is complex and every W_k, k > 0, diagonal; without it u = +-1
// and a W_k that couples the sectors is as legal as any other).  With E^(qr)_bc = gt0(A^q b; B^r c) and T^(sp)_da = g0t(B^s d; A^p a)
//   o_t(A)     = tr M0 - sum_k f_k sum_ab (W_k)_ab g_t(A^q b; A^p a)
//   conn(A, B) = sum_(k, k') Re f_k(A) f_k'(B) tr(W_k E^(qr) W_k' T^(sp)),        (p, q) of k at A, (r, s) of k' at B:
// 25 block pairs, each the Re tr(M E M T) of the on-site kernel with two different matrices.  The pair loop is a real loop (not unrolled:
// the body is the four channels' unrolled products already) and only its one E and one T block are live; the neighbour blocks are
// re-read from L1 / L2 by the argument above k_measure_td_current.  The blocks W_k, their non-zero masks and u come from a small device
// table indexed by the loop variables (uniform: scalar loads); parts[c] bit k = W_k of operator c is non-zero, so the pairs no operator
// needs are skipped before their loads and an on-site-only operator takes part in pair (0, 0) alone.
// Equal-time form: gt0 -> gs, g0t -> gs - 1, the 1 subtracted from the diagonal of T wherever B^s and A^p are the same site (d = 0,
// +-x, +-y, +-(x - y)) -- the delta term in full, no M^2 shortcut.
#define CSTB_K 5
size_t measure_custom_bond_table_cplx(int count, int N) { return (size_t)count * CSTB_K * 16 + 2 * (size_t)N; }
struct CustomBondArg { const cplx* tab; const unsigned* mk; unsigned parts[DQMC_CUSTOM_MAX]; int count; };

// Re tr(MA E MB T); e[r][c] = E_rc, t[r][c] = T_rc of the stored part, MA / MB row-major in device memory
template<int OPDIM, int R>
__device__ __forceinline__ double cstb_connected(const cplx (&e)[R][R], const cplx (&t)[R][R], const cplx* __restrict__ MA, unsigned ma,
                                                 const cplx* __restrict__ MB, unsigned mb) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!((ma >> (4 * a)) & 0xfu)) continue;            // row a of MA is empty
        cplx x[4], y[4];                                    // x[c] = (MA E)_ac, y[c] = (MB T)_ca
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) x[c2] = y[c2] = make_double2(0.0, 0.0);
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (ma & (1u << (4 * a + b))) {
                const cplx m = MA[4 * a + b];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2)
                    if (cst_same<OPDIM>(b, c2)) cst_fma(x[c2], m, cst_E<OPDIM, R>(e, b, c2));
            }
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
            for (int dl = 0; dl < 4; ++dl)
                if (cst_same<OPDIM>(dl, a) && (mb & (1u << (4 * c2 + dl)))) cst_fma(y[c2], MB[4 * c2 + dl], cst_E<OPDIM, R>(t, dl, a));
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) s += x[c2].x * y[c2].x - x[c2].y * y[c2].y;
    }
    return s;
}

// the sites (p, q) of block k at the stencil (S, Sx, Sy) and its link factor from (ux, uy)
__device__ __forceinline__ void cstb_block(int k, int S, int Sx, int Sy, cplx ux, cplx uy, int& p, int& q, cplx& f) {
    p = k == 1 ? Sx : k == 3 ? Sy : S;
    q = k == 2 ? Sx : k == 4 ? Sy : S;
    const cplx u = k < 3 ? ux : uy;
    f = k == 0 ? make_double2(1.0, 0.0) : make_double2(u.x, (k & 1) ? u.y : -u.y);
}
__device__ __forceinline__ void cstb_stencil(int L, int sx, int sy, int& Sx, int& Sy) {
    Sx = sy * L + (sx + 1 == L ? 0 : sx + 1);
    Sy = (sy + 1 == L ? 0 : sy + 1) * L + sx;
}

// o(A) of operator ch from the shifted equal-time matrix gs
template<int OPDIM>
__device__ __forceinline__ cplx cstb_onebody(const cplx* __restrict__ gs, size_t ng, int N, int L, int A, const CustomBondArg& cb, int ch) {
    constexpr int R = OPDIM == 3 ? 4 : 2;
    const cplx* __restrict__ V = cb.tab + (size_t)ch * CSTB_K * 16;
    const cplx* __restrict__ lk = cb.tab + (size_t)cb.count * CSTB_K * 16;
    int Ax, Ay;
    cstb_stencil(L, A % L, A / L, Ax, Ay);
    const cplx ux = lk[A], uy = lk[N + A];
    cplx s = make_double2(0.0, 0.0);
#pragma unroll 1
    for (int k = 0; k < CSTB_K; ++k) {
        if (!((cb.parts[ch] >> k) & 1u)) continue;
        int p, q;
        cplx f;
        cstb_block(k, A, Ax, Ay, ux, uy, p, q, f);
        const cplx* base = gs + (size_t)p * ng + (size_t)q;      // x[b][a] = f g(A^q b; A^p a)
        cplx x[R][R];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b) x[b][a] = m_mul(f, base[(size_t)a * N * ng + (size_t)b * N]);
        const cplx* __restrict__ M = V + 16 * k;
        const unsigned mask = cb.mk[ch * CSTB_K + k];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (cst_same<OPDIM>(b, a) && (mask & (1u << (4 * a + b)))) cst_fma(s, M[4 * a + b], cst_E<OPDIM, R>(x, b, a));
    }
    const cplx tr = m_add(m_add(V[0], V[5]), m_add(V[10], V[15]));
    return m_sub(tr, s);
}

// ob[chain][t][channel][site] as k_td_custom_onebody
template<int OPDIM>
__global__ __launch_bounds__(256) void k_td_custom_bond_onebody(DevModel dm, CustomBondArg cb, const cplx* __restrict__ gs, cplx* __restrict__ ob, int t,
                                                                size_t obs, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx* o = ob + (size_t)blockIdx.z * obs + (size_t)t * cb.count * N + A;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
        if (ch < cb.count) o[(size_t)ch * N] = cstb_onebody<OPDIM>(gs, (size_t)dm.ng, N, dm.L, A, cb, ch);
}
// ob[chain][channel][site]: the one set of values both factors of the equal-time form use
template<int OPDIM>
__global__ __launch_bounds__(256) void k_eq_custom_bond_onebody(DevModel dm, CustomBondArg cb, const cplx* __restrict__ gs, cplx* __restrict__ ob,
                                                                size_t obs, size_t cs) {
    CHAIN(gs);
    const int N = dm.N, A = blockIdx.x * 256 + threadIdx.x;
    if (A >= N) return;
    cplx* o = ob + (size_t)blockIdx.z * obs + A;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
        if (ch < cb.count) o[(size_t)ch * N] = cstb_onebody<OPDIM>(gs, (size_t)dm.ng, N, dm.L, A, cb, ch);
}

// the sums over B of Re W(B (+) d, B) of one thread's (bin, part); EQ: hs is not read, ot == o0
template<int OPDIM, bool EQ>
__device__ __forceinline__ void cstb_walk(const DevModel& dm, const CustomBondArg& cb, const cplx* __restrict__ gs, const cplx* __restrict__ hs,
                                          const cplx* __restrict__ ot, const cplx* __restrict__ o0, const BinWalk& bw, double (&w)[DQMC_CUSTOM_MAX]) {
    constexpr int R = OPDIM == 3 ? 4 : 2;
    const int N = dm.N, L = dm.L, count = cb.count;
    const size_t ng = (size_t)dm.ng, cN = (size_t)N * ng;
    const cplx* __restrict__ lk = cb.tab + (size_t)count * CSTB_K * 16;
    unsigned both[DQMC_CUSTOM_MAX];                         // bit 5 ka + kb: operator ch has the blocks ka and kb
    unsigned need = 0;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) {
        both[ch] = 0;
        if (ch < count)
            for (int ka = 0; ka < CSTB_K; ++ka)
                if ((cb.parts[ch] >> ka) & 1u) both[ch] |= (cb.parts[ch] & 0x1fu) << (CSTB_K * ka);
        need |= both[ch];
    }
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        int Ax, Ay, Bx, By;
        cstb_stencil(L, st.ax, st.ay, Ax, Ay);
        cstb_stencil(L, st.bx, st.by, Bx, By);
        const cplx uax = lk[A], uay = lk[N + A], ubx = lk[B], uby = lk[N + B];
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
            if (ch < count) {
                const cplx a = ot[(size_t)ch * N + A], b = o0[(size_t)ch * N + B];
                w[ch] += a.x * b.x - a.y * b.y;
            }
#pragma unroll 1
        for (int pr = 0; pr < CSTB_K * CSTB_K; ++pr) {
            if (!((need >> pr) & 1u)) continue;
            const int ka = pr / CSTB_K, kb = pr % CSTB_K;
            int p, q, r, s2;
            cplx fa, fb;
            cstb_block(ka, A, Ax, Ay, uax, uay, p, q, fa);
            cstb_block(kb, B, Bx, By, ubx, uby, r, s2, fb);
            const cplx f = m_mul(fa, fb);
            const cplx* pe = gs + (size_t)r * ng + (size_t)q;         // E_bc = gt0(A^q b; B^r c) = pe[c N ng + b N]
            cplx e[R][R], t[R][R];
#pragma unroll
            for (int c2 = 0; c2 < R; ++c2)
#pragma unroll
                for (int b = 0; b < R; ++b) e[b][c2] = m_mul(f, pe[(size_t)c2 * cN + (size_t)b * N]);
            if (EQ) {
                const cplx* pt = gs + (size_t)p * ng + (size_t)s2;    // T_da = gs(B^s d; A^p a) - delta = pt[a N ng + d N] - delta
                const double one = s2 == p ? 1.0 : 0.0;
#pragma unroll
                for (int a = 0; a < R; ++a)
#pragma unroll
                    for (int dl = 0; dl < R; ++dl) {
                        t[dl][a] = pt[(size_t)a * cN + (size_t)dl * N];
                        if (dl == a) t[dl][a].x -= one;
                    }
            } else {
                const cplx* ph = hs + (size_t)s2 * ng + (size_t)p;    // T_da = conj hs(A^p a; B^s d) = conj ph[d N ng + a N]
#pragma unroll
                for (int dl = 0; dl < R; ++dl)
#pragma unroll
                    for (int a = 0; a < R; ++a) {
                        const cplx h = ph[(size_t)dl * cN + (size_t)a * N];
                        t[dl][a] = make_double2(h.x, -h.y);
                    }
            }
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cb.tab + (size_t)ch * CSTB_K * 16;
                    w[ch] -= cstb_connected<OPDIM, R>(e, t, V + 16 * ka, cb.mk[ch * CSTB_K + ka], V + 16 * kb, cb.mk[ch * CSTB_K + kb]);
                }
        }
    }
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_td_custom_bond(DevModel dm, CustomBondArg cb, const cplx* __restrict__ gs,
                                                                                 const cplx* __restrict__ hs, const cplx* __restrict__ ob,
                                                                                 double* __restrict__ acc, int row, int rows, size_t obs, size_t acs,
                                                                                 size_t cs) {
    CHAIN(gs); CHAIN(hs);
    ob += (size_t)blockIdx.z * obs;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, count = cb.count;
    const BinWalk bw(N, dm.L);
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    cstb_walk<OPDIM, false>(dm, cb, gs, hs, ob, ob + (size_t)count * N, bw, w);
    bw.reduce_add(w, red, count, acc + rows + (size_t)row * count * N, N, 1, acc + row);
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_eq_custom_bond(DevModel dm, CustomBondArg cb, const cplx* __restrict__ gs,
                                                                                 const cplx* __restrict__ ob, double* __restrict__ acc, size_t obs,
                                                                                 size_t acs, size_t cs) {
    CHAIN(gs);
    ob += (size_t)blockIdx.z * obs;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, count = cb.count;
    const BinWalk bw(N, dm.L);
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    cstb_walk<OPDIM, true>(dm, cb, gs, gs, ob, ob, bw, w);
    bw.reduce_add(w, red, count, acc + 1, N, 1, acc);
}

static CustomBondArg custom_bond_arg(int count, const CustomBond& bond) {
    CustomBondArg cb{};
    cb.tab = bond.tab; cb.mk = bond.mk; cb.count = count;
    for (int ch = 0; ch < count; ++ch) cb.parts[ch] = bond.parts[ch];
    return cb;
}

static void launch_td_custom_bond_onebody(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, cplx* ob, int t) {
    const CustomBondArg cb = custom_bond_arg(count, bond);
    const dim3 grid((hm.N + 255) / 256, 1, lc.nb);
    const size_t obs = measure_td_custom_onebody_cplx(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_td_custom_bond_onebody<decltype(O)::value>), grid, dim3(256), 0, lc.st, hm, cb, gs, ob, t, obs, lc.cs);
    });
}

static void launch_measure_td_custom_bond(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, const cplx* hs,
                                          const cplx* ob, double* acc, size_t acs, int row, int rows) {
    const CustomBondArg cb = custom_bond_arg(count, bond);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    const size_t obs = measure_td_custom_onebody_cplx(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_td_custom_bond<decltype(O)::value>), grid, block, 0, lc.st, hm, cb, gs, hs, ob, acc, row, rows, obs, acs, lc.cs);
    });
}

static void launch_measure_eq_custom_bond(const Launch& lc, const DevModel& hm, int count, const CustomBond& bond, const cplx* gs, cplx* ob, double* acc) {
    const CustomBondArg cb = custom_bond_arg(count, bond);
    const dim3 g1((hm.N + 255) / 256, 1, lc.nb);
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    const size_t obs = measure_eq_custom_onebody_cplx(count, hm.N), acs = 1 + measure_custom_row_doubles(count, hm.N);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_eq_custom_bond_onebody<decltype(O)::value>), g1, dim3(256), 0, lc.st, hm, cb, gs, ob, obs, lc.cs);
        hipLaunchKernelGGL((k_measure_eq_custom_bond<decltype(O)::value>), grid, block, 0, lc.st, hm, cb, gs, ob, acc, obs, acs, lc.cs);
    });
}

// User-defined pair operators (dqmc_set_custom_pair_operators; definitions in dqmc_hip.h and DESIGN.md 6e):
//   Delta_A = sum_ab F0_ab c_(A a) c_(A b) + sum_mu u_mu(A) sum_ab Fmu_ab c_(A (+) mu, a) c_(A b),   P(A, B) = <Delta_A(tau) Delta_B^+(0)>.
// With E^(PQ)_rc = g~(P r; Q c) of ONE shifted matrix gs (g~(tau,0) time-displaced, g~ of the slice at equal time: <c c c^+ c^+> has no
// delta term) and the site blocks k = 0, x, y of an operator at the sites (A^k, A), Wick's theorem gives for the block pair (k, k')
//   direct   = sum_abcd F^k_ab E^(A^k B^k')_ac conj(F^k')_cd E^(A B)_bd
//   exchange = sum_abcd F^k_ab E^(A^k B)_ad   (F^k'^H)_dc    E^(A B^k')_bc
// and P = sum_(k, k') u_k(A) u_k'(B) (direct - exchange); both are the one form sum F_ab X_ac G_cd Y_bd (cpr_term).  No one-body scratch, no
// second matrix.  OPDIM < 3: the sector rule of cst_E / cst_same; a pair operator usually couples the sectors (XUP with XDOWN), which the
// rule resolves at compile time like any other entry.
// On-site form (no operator has a bond part): all four blocks are the one E = g~(A .; B .), loaded once per site pair, and
//   P = tr(F^T E (conj F - F^H) E^T) = 1/2 sum_ab Fa_ab [E conj(Fa) E^T]_ab,   Fa = F0 - F0^T
// (E conj(Fa) E^T is antisymmetric, so only the antisymmetric part of F0 contributes), every channel contracted from registers; Fa and
// its non-zero mask travel as a kernel argument, the mask branches are uniform over the launch.  The block is count[rows],
// then the rows [count][N]; the equal-time block is the same with rows = 1.  Blocks live outside the arena: chain b at acc + b * acs.
template<int OPDIM, int R>
__device__ __forceinline__ double cpr_onsite(const cplx (&e)[R][R], const cplx (&F)[4][4], unsigned mask) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!((mask >> (4 * a)) & 0xfu)) continue;          // row a of Fa is empty
        cplx x[4], y[4];                                    // x[d] = (E conj Fa)_ad, y[d] = (Fa E)_ad
#pragma unroll
        for (int dl = 0; dl < 4; ++dl) x[dl] = y[dl] = make_double2(0.0, 0.0);
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2)
            if (cst_same<OPDIM>(a, c2)) {
#pragma unroll
                for (int dl = 0; dl < 4; ++dl)
                    if (mask & (1u << (4 * c2 + dl))) cst_fma(x[dl], cst_E<OPDIM, R>(e, a, c2), make_double2(F[c2][dl].x, -F[c2][dl].y));
            }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (mask & (1u << (4 * a + b))) {
#pragma unroll
                for (int dl = 0; dl < 4; ++dl)
                    if (cst_same<OPDIM>(b, dl)) cst_fma(y[dl], F[a][b], cst_E<OPDIM, R>(e, b, dl));
            }
#pragma unroll
        for (int dl = 0; dl < 4; ++dl) s += x[dl].x * y[dl].x - x[dl].y * y[dl].y;
    }
    return 0.5 * s;
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_custom_pair(DevModel dm, CustomMats cm, const cplx* __restrict__ gs,
                                                                              double* __restrict__ acc, int row, int rows, size_t acs, size_t cs) {
    CHAIN(gs);
    constexpr int R = OPDIM == 3 ? 4 : 2;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, count = cm.count;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        cplx e[R][R];
        m_load_block(gs, ng, N, st.A, st.B, e);             // E_rc = gs(A r; B c)
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
            if (ch < count) w[ch] += cpr_onsite<OPDIM, R>(e, cm.m[ch], cm.mask[ch]);
    }
    bw.reduce_add(w, red, count, acc + rows + (size_t)row * count * N, N, 1, acc + row);
}

// Stencil form (at least one operator has a bond part).  Device table tab (measure_custom_pair_table_cplx complex, shared by the chains):
// per operator and site block k = 0, x, y the three forms F, conj F, F^H, V[count][3][3][4][4], then the link signs u[2][N] (real part;
// bond parts are refused under flux, so u = +-1).  mk[count][3][2]: the non-zero masks of F (and conj F) and of F^H.  parts[c] bit k:
// block k of operator c is non-zero.  The 9 block pairs run in a real loop, the two blocks of the direct term and then the two of the
// exchange term are the only ones live; the at most nine distinct neighbour blocks are re-read from L1 / L2.  Pairs no operator needs
// are skipped before their loads, an on-site-only operator takes part in pair (0, 0) alone.
#define CPR_K 3
size_t measure_custom_pair_table_cplx(int count, int N) { return (size_t)count * CPR_K * 3 * 16 + 2 * (size_t)N; }
struct CustomPairArg { const cplx* tab; const unsigned* mk; unsigned parts[DQMC_CUSTOM_MAX]; int count; };

// Re sum_abcd F_ab X_ac G_cd Y_bd; x[r][c], y[r][c] the stored parts, F / G row-major in device memory with masks mf / mg
template<int OPDIM, int R>
__device__ __forceinline__ double cpr_term(const cplx (&x)[R][R], const cplx (&y)[R][R], const cplx* __restrict__ F, unsigned mf,
                                           const cplx* __restrict__ G, unsigned mg) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (!((mf >> (4 * a)) & 0xfu)) continue;            // row a of F is empty
        cplx p[4], q[4];                                    // p[d] = (X G)_ad, q[d] = (F Y)_ad
#pragma unroll
        for (int dl = 0; dl < 4; ++dl) p[dl] = q[dl] = make_double2(0.0, 0.0);
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2)
            if (cst_same<OPDIM>(a, c2)) {
#pragma unroll
                for (int dl = 0; dl < 4; ++dl)
                    if (mg & (1u << (4 * c2 + dl))) cst_fma(p[dl], cst_E<OPDIM, R>(x, a, c2), G[4 * c2 + dl]);
            }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (mf & (1u << (4 * a + b))) {
                const cplx f = F[4 * a + b];
#pragma unroll
                for (int dl = 0; dl < 4; ++dl)
                    if (cst_same<OPDIM>(b, dl)) cst_fma(q[dl], f, cst_E<OPDIM, R>(y, b, dl));
            }
#pragma unroll
        for (int dl = 0; dl < 4; ++dl) s += p[dl].x * q[dl].x - p[dl].y * q[dl].y;
    }
    return s;
}

template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_custom_pair_bond(DevModel dm, CustomPairArg cp, const cplx* __restrict__ gs,
                                                                                   double* __restrict__ acc, int row, int rows, size_t acs, size_t cs) {
    CHAIN(gs);
    constexpr int R = OPDIM == 3 ? 4 : 2;
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[DQMC_CUSTOM_MAX][TDP_PARTS][TDP_BINS];
    const int N = dm.N, L = dm.L, count = cp.count;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    const cplx* __restrict__ lk = cp.tab + (size_t)count * CPR_K * 3 * 16;
    unsigned both[DQMC_CUSTOM_MAX];                         // bit 3 ka + kb: operator ch has the blocks ka and kb
    unsigned need = 0;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) {
        both[ch] = 0;
        if (ch < count)
            for (int ka = 0; ka < CPR_K; ++ka)
                if ((cp.parts[ch] >> ka) & 1u) both[ch] |= (cp.parts[ch] & 0x7u) << (CPR_K * ka);
        need |= both[ch];
    }
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const int A = st.A, B = st.B;
        int Ax, Ay, Bx, By;
        cstb_stencil(L, st.ax, st.ay, Ax, Ay);
        cstb_stencil(L, st.bx, st.by, Bx, By);
        const double uax = lk[A].x, uay = lk[N + A].x, ubx = lk[B].x, uby = lk[N + B].x;
#pragma unroll 1
        for (int pr = 0; pr < CPR_K * CPR_K; ++pr) {
            if (!((need >> pr) & 1u)) continue;
            const int ka = pr / CPR_K, kb = pr % CPR_K;
            const int p = ka == 1 ? Ax : ka == 2 ? Ay : A, r = kb == 1 ? Bx : kb == 2 ? By : B;
            const double f = (ka == 1 ? uax : ka == 2 ? uay : 1.0) * (kb == 1 ? ubx : kb == 2 ? uby : 1.0);
            cplx x[R][R], y[R][R];
            m_load_block(gs, ng, N, p, r, x);               // direct: E(A^k; B^k'), E(A; B)
            m_load_block(gs, ng, N, A, B, y);
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cp.tab + (size_t)ch * CPR_K * 3 * 16;
                    const unsigned* __restrict__ mk = cp.mk + ch * CPR_K * 2;
                    w[ch] += f * cpr_term<OPDIM, R>(x, y, V + 48 * ka, mk[2 * ka], V + 48 * kb + 16, mk[2 * kb]);
                }
            m_load_block(gs, ng, N, p, B, x);               // exchange: E(A^k; B), E(A; B^k')
            m_load_block(gs, ng, N, A, r, y);
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cp.tab + (size_t)ch * CPR_K * 3 * 16;
                    const unsigned* __restrict__ mk = cp.mk + ch * CPR_K * 2;
                    w[ch] -= f * cpr_term<OPDIM, R>(x, y, V + 48 * ka, mk[2 * ka], V + 48 * kb + 32, mk[2 * kb + 1]);
                }
        }
    }
    bw.reduce_add(w, red, count, acc + rows + (size_t)row * count * N, N, 1, acc + row);
}

void launch_measure_custom_pair(const Launch& lc, const DevModel& hm, int count, const cplx* Fa, const unsigned* mask, const cplx* gs, double* acc,
                                size_t acs, int row, int rows, const CustomPair* bond) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    if (bond) {
        CustomPairArg cp{};
        cp.tab = bond->tab; cp.mk = bond->mk; cp.count = count;
        for (int ch = 0; ch < count; ++ch) cp.parts[ch] = bond->parts[ch];
        dispatch_opdim(hm.opdim, [&](auto O) {
            hipLaunchKernelGGL((k_measure_custom_pair_bond<decltype(O)::value>), grid, block, 0, lc.st, hm, cp, gs, acc, row, rows, acs, lc.cs);
        });
        return;
    }
    const CustomMats cm = custom_mats(count, Fa, mask);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_custom_pair<decltype(O)::value>), grid, block, 0, lc.st, hm, cm, gs, acc, row, rows, acs, lc.cs);
    });
}

// The averaged Green's function block (dqmc_set_green_matrix; dqmc_hip.h and DESIGN.md 6e): from the shifted gs = g~(tau,0) the pair
// kernels read,
//   Gbar_rc(d) += sum_B sigma(B, d) gs((B (+) d) r; B c),   sigma = -1 for each antiperiodic direction in which B + d wraps,
// r, c over the stored flavour block (R = 2: the (XUP, YDOWN) sector, R = 4 for O(3)).  A thread keeps the 2 R^2 sums of its bin in
// registers, and the reduction over the parts runs in passes of TDP_PARTS components: part q writes component pass TDP_PARTS + q of its
// bin.  Block: count[rows], then the rows [N][R][R] (re, im); outside the arena: chain b at acc + b * acs.
size_t measure_green_matrix_row_doubles(int opdim, int N) { return (size_t)(opdim == 3 ? 32 : 8) * N; }
template<int OPDIM>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_measure_green_matrix(DevModel dm, const cplx* __restrict__ gs, double* __restrict__ acc,
                                                                               int row, int rows, size_t acs, size_t cs, int apbx, int apby) {
    CHAIN(gs);
    constexpr int R = OPDIM == 3 ? 4 : 2, NC = 2 * R * R;
    static_assert(NC % TDP_PARTS == 0, "the reduction runs in passes of TDP_PARTS components");
    acc += (size_t)blockIdx.z * acs;
    __shared__ double red[TDP_PARTS][TDP_PARTS][TDP_BINS];  // [component of the pass][part][bin]
    const int N = dm.N, L = dm.L;
    const size_t ng = (size_t)dm.ng;
    const BinWalk bw(N, L);
    double w[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) w[q] = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const double sg = ((st.wx && apbx) != (st.wy && apby)) ? -1.0 : 1.0;
        const cplx* pe = gs + (size_t)st.B * ng + (size_t)st.A;           // gs(A r; B c) = pe[c N ng + r N]
#pragma unroll
        for (int c2 = 0; c2 < R; ++c2)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const cplx v = pe[(size_t)c2 * N * ng + (size_t)r * N];
                w[2 * (r * R + c2)] += sg * v.x; w[2 * (r * R + c2) + 1] += sg * v.y;
            }
    }
#pragma unroll
    for (int pass = 0; pass < NC / TDP_PARTS; ++pass) {
        if (pass) __syncthreads();                          // red is free again
        bw.reduce_add(w + pass * TDP_PARTS, red, TDP_PARTS, acc + rows + (size_t)row * N * NC + pass * TDP_PARTS, 1, NC,
                      pass + 1 == NC / TDP_PARTS ? acc + row : nullptr);
    }
}
void launch_measure_green_matrix(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, size_t acs, int row, int rows, int apbx, int apby) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    dispatch_opdim(hm.opdim, [&](auto O) {
        hipLaunchKernelGGL((k_measure_green_matrix<decltype(O)::value>), grid, block, 0, lc.st, hm, gs, acc, row, rows, acs, lc.cs, apbx, apby);
    });
}

// Series part 13 (DQMC_SERIES_GREEN_MATRIX): the every-slice block of the kernel above normalised, out[k][N][R][R] (re, im) = row k /
// (double(N) count[k]) (one division); bad[chain] = 1 if a row of the chain has no sample.  Grid (row pieces, rows, chains).
__global__ __launch_bounds__(256) void k_series_green_sample(const double* __restrict__ fine, size_t chain_bytes, int rows, size_t rowlen, double Nd,
                                                             double* __restrict__ sample, size_t S, size_t off, double* __restrict__ bad) {
    const double* blk = (const double*)((const char*)fine + (size_t)blockIdx.z * chain_bytes);
    const int k = blockIdx.y;
    if (blockIdx.x == 0 && k == 0 && threadIdx.x == 0) {
        double flag = 0.0;
        for (int r = 0; r < rows; ++r) if (!(blk[r] >= 1.0)) flag = 1.0;
        bad[blockIdx.z] = flag;
    }
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rowlen) return;
    const double den = Nd * blk[k];
    sample[(size_t)blockIdx.z * S + off + (size_t)k * rowlen + i] = blk[rows + (size_t)k * rowlen + i] / den;
}
void launch_series_green_sample(const Launch& lc, const DevModel& hm, const double* fine, size_t chain_bytes, double* sample, size_t S, size_t off,
                                double* bad) {
    const size_t rowlen = measure_green_matrix_row_doubles(hm.opdim, hm.N);
    hipLaunchKernelGGL(k_series_green_sample, dim3((unsigned)((rowlen + 255) / 256), (unsigned)(hm.m + 1), (unsigned)lc.nb), dim3(256), 0, lc.st, fine,
                       chain_bytes, hm.m + 1, rowlen, (double)hm.N, sample, S, off, bad);
}

// Bubble and vertex of the pair operators from the series (dqmc_series_pair_vertex_host; dqmc_hip.h and DESIGN.md 6e), two kernels.
// k_series_pair_bubble, grid (row k = 0 .. m, jackknife index b = 0 .. B, slot), 256 threads: the row of part 13 for index b -- the
// leave-one-out mean x_(b) = (B mean - x_b) / (B - 1), b = B: the mean itself -- is staged in LDS as gbar[N][R][R]; then, with
//   gbar(P r; Q c) = sigma(Q, P (-) Q) gbar_rc(P (-) Q)
// in the place of the E blocks, thread d evaluates the contraction of k_measure_custom_pair_bond (cpr_term, the same table, masks and
// link signs) for the site pair (A, B) = (d, 0) -- gbar is translation-covariant, the summand does not depend on B -- and adds
// cos(Q d) Pbar_c(d) to its sum; a fixed tree over the 256 sums follows, and thread c writes pb[slot][b][k][c].
// k_series_pair_vertex, one thread per (slot, operator, output): the tau quadrature of pb and the jackknife over b in index order.
struct PairVertexShape { size_t S, off_g, off_chi; int L, N, m, nfreq, nb, B, count, qx, qy, apbx, apby; double dtau; };
size_t series_pair_bubble_lds_bytes(int opdim, int N) { return (measure_green_matrix_row_doubles(opdim, N) + (size_t)DQMC_CUSTOM_MAX * 256) * sizeof(double); }
// e[r][c] = the stored part of gbar(P .; Q .), P = (px, py) and Q = (qx, qy) reduced to 0 .. L-1
template<int R>
__device__ __forceinline__ void pvx_load(const cplx* __restrict__ g, int L, int apbx, int apby, int px, int py, int qx, int qy, cplx (&e)[R][R]) {
    int dx = px - qx, dy = py - qy;
    if (dx < 0) dx += L;
    if (dy < 0) dy += L;
    const double sg = ((apbx && qx + dx >= L) != (apby && qy + dy >= L)) ? -1.0 : 1.0;
    const cplx* p = g + (size_t)(dy * L + dx) * R * R;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c2 = 0; c2 < R; ++c2) e[r][c2] = make_double2(sg * p[r * R + c2].x, sg * p[r * R + c2].y);
}
template<int OPDIM>
__global__ __launch_bounds__(256) void k_series_pair_bubble(const double* __restrict__ bins, const double* __restrict__ mean,
                                                            const double* __restrict__ trig, CustomPairArg cp, PairVertexShape a,
                                                            double* __restrict__ pb) {
    constexpr int R = OPDIM == 3 ? 4 : 2;
    extern __shared__ __attribute__((aligned(16))) double pvx_sm[];
    const int N = a.N, L = a.L, tid = threadIdx.x, count = cp.count, B = a.B;
    const int k = blockIdx.x, b = blockIdx.y, slot = blockIdx.z;
    const size_t rowlen = (size_t)2 * R * R * N, n = (size_t)a.nb * a.S, base = (size_t)slot * a.S + a.off_g + (size_t)k * rowlen;
    double* red = pvx_sm + rowlen;                          // [DQMC_CUSTOM_MAX][256]
    for (size_t e = tid; e < rowlen; e += 256) {
        const double mu = mean[base + e];
        pvx_sm[e] = b < B ? ((double)B * mu - bins[(size_t)b * n + base + e]) / (double)(B - 1) : mu;
    }
    __syncthreads();
    const cplx* g = (const cplx*)pvx_sm;
    const cplx* __restrict__ lk = cp.tab + (size_t)count * CPR_K * 3 * 16;
    unsigned both[DQMC_CUSTOM_MAX];                         // bit 3 ka + kb: operator ch has the blocks ka and kb
    unsigned need = 0;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) {
        both[ch] = 0;
        if (ch < count)
            for (int ka = 0; ka < CPR_K; ++ka)
                if ((cp.parts[ch] >> ka) & 1u) both[ch] |= (cp.parts[ch] & 0x7u) << (CPR_K * ka);
        need |= both[ch];
    }
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    const int B1 = 1 % L;                                   // the neighbours of site B = 0: (1, 0) and (0, 1)
    const double ubx = lk[0].x, uby = lk[N].x;
    for (int d = tid; d < N; d += 256) {
        const int ax = d % L, ay = d / L;
        const int axp = ax + 1 == L ? 0 : ax + 1, ayp = ay + 1 == L ? 0 : ay + 1;
        const double uax = lk[d].x, uay = lk[N + d].x;
        double v[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int pr = 0; pr < CPR_K * CPR_K; ++pr) {
            if (!((need >> pr) & 1u)) continue;
            const int ka = pr / CPR_K, kb = pr % CPR_K;
            const int px = ka == 1 ? axp : ax, py = ka == 2 ? ayp : ay, rx = kb == 1 ? B1 : 0, ry = kb == 2 ? B1 : 0;
            const double f = (ka == 1 ? uax : ka == 2 ? uay : 1.0) * (kb == 1 ? ubx : kb == 2 ? uby : 1.0);
            cplx x[R][R], y[R][R];
            pvx_load<R>(g, L, a.apbx, a.apby, px, py, rx, ry, x);           // direct: gbar(A^k; B^k'), gbar(A; B)
            pvx_load<R>(g, L, a.apbx, a.apby, ax, ay, 0, 0, y);
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cp.tab + (size_t)ch * CPR_K * 3 * 16;
                    const unsigned* __restrict__ mk = cp.mk + ch * CPR_K * 2;
                    v[ch] += f * cpr_term<OPDIM, R>(x, y, V + 48 * ka, mk[2 * ka], V + 48 * kb + 16, mk[2 * kb]);
                }
            pvx_load<R>(g, L, a.apbx, a.apby, px, py, 0, 0, x);             // exchange: gbar(A^k; B), gbar(A; B^k')
            pvx_load<R>(g, L, a.apbx, a.apby, ax, ay, rx, ry, y);
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cp.tab + (size_t)ch * CPR_K * 3 * 16;
                    const unsigned* __restrict__ mk = cp.mk + ch * CPR_K * 2;
                    v[ch] -= f * cpr_term<OPDIM, R>(x, y, V + 48 * ka, mk[2 * ka], V + 48 * kb + 32, mk[2 * kb + 1]);
                }
        }
        const double cq = trig[(a.qx * ax + a.qy * ay) % L];
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) w[ch] += cq * v[ch];
    }
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) red[ch * 256 + tid] = w[ch];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                     // a fixed tree: the same order in every launch
        if (tid < h)
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) red[ch * 256 + tid] += red[ch * 256 + tid + h];
        __syncthreads();
    }
    if (tid < count) pb[(((size_t)slot * (B + 1) + b) * (a.m + 1) + k) * count + tid] = red[tid * 256];
}
// outputs per (slot, operator): 0 P = Re chi(Q, i omega_0) of part 11, 1 Pbar = dtau sum_k w_k pb, 2 Gamma = 1 / P - 1 / Pbar,
// 3 Gamma Pbar = Pbar / P - 1, then pb at k = 0 .. m; NaN where a denominator vanishes
__device__ __forceinline__ double pvx_f(int e, double P, double Pb) {
    if (e == 0) return P;
    if (e == 1) return Pb;
    if (P == 0.0 || (e == 2 && Pb == 0.0)) return nan("");
    return e == 2 ? 1.0 / P - 1.0 / Pb : Pb / P - 1.0;
}
__global__ __launch_bounds__(64) void k_series_pair_vertex(const double* __restrict__ bins, const double* __restrict__ pb, PairVertexShape a,
                                                           double* __restrict__ value, double* __restrict__ err) {
    const int per = 5 + a.m, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * a.count * per) return;
    const int slot = t / (a.count * per), c = (t / per) % a.count, e = t % per, B = a.B, m = a.m;
    const size_t n = (size_t)a.nb * a.S;
    const double* p = bins + (size_t)slot * a.S + a.off_chi + ((size_t)c * a.nfreq * a.N + (size_t)a.qy * a.L + a.qx) * 2;     // Re, frequency 0
    const double* r0 = pb + (size_t)slot * (B + 1) * (m + 1) * a.count + c;
    double sum = 0.0;
    for (int b = 0; b < B; ++b) sum += p[(size_t)b * n];
    const double mu = sum / (double)B, tot = (double)B * mu;
    auto theta = [&](int b) {
        const double* r = r0 + (size_t)b * (m + 1) * a.count;
        if (e >= 4) return r[(size_t)(e - 4) * a.count];
        double s = 0.0;
        for (int k = 0; k <= m; ++k) s += (k == 0 || k == m ? 0.5 : 1.0) * r[(size_t)k * a.count];
        return pvx_f(e, b < B ? (tot - p[(size_t)b * n]) / (double)(B - 1) : mu, a.dtau * s);
    };
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) tsum += theta(b);
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const double dl = theta(b) - tbar;
        acc += dl * dl;
    }
    value[t] = theta(B);
    err[t] = sqrt((double)(B - 1) / (double)B * acc);
}
// false: the lattice is too large for the bubble kernel's LDS, nothing was launched.  mean: the bin means [nb][S] (launch_series_stats)
bool launch_series_pair_vertex(const Launch& lc, const DevModel& hm, const double* bins, const double* mean, const double* trig, size_t S, int B,
                               int nfreq, size_t off_chi, size_t off_g, int count, const CustomPair& pair, int qx, int qy, int apbx, int apby,
                               double* pb, double* value, double* err) {
    const size_t lds = series_pair_bubble_lds_bytes(hm.opdim, hm.N);
    if (lds > 152 * 1024) return false;
    CustomPairArg cp{};
    cp.tab = pair.tab; cp.mk = pair.mk; cp.count = count;
    for (int ch = 0; ch < count; ++ch) cp.parts[ch] = pair.parts[ch];
    const PairVertexShape a{S, off_g, off_chi, hm.L, hm.N, hm.m, nfreq, lc.nb, B, count, qx, qy, apbx, apby, hm.dtau};
    const dim3 grid((unsigned)(hm.m + 1), (unsigned)(B + 1), (unsigned)lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        const void* fn = (const void*)k_series_pair_bubble<decltype(O)::value>;
        if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
        hipLaunchKernelGGL((k_series_pair_bubble<decltype(O)::value>), grid, dim3(256), lds, lc.st, bins, mean, trig, cp, a, pb);
    });
    const int total = lc.nb * count * (5 + hm.m);
    hipLaunchKernelGGL(k_series_pair_vertex, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, lc.st, bins, pb, a, value, err);
    return true;
}

// Particle-hole bubble and vertex of the user-defined bilinears from the series (dqmc_series_ph_vertex_host; dqmc_hip.h and DESIGN.md
// 6e), two kernels in the shape of the pair ones above.
// k_series_ph_bubble, grid (row k = 0 .. m, jackknife index b = 0 .. B, slot), 256 threads: rows k and m - k of part 13 for index b are
// staged in LDS (the leave-one-out mean as in k_series_pair_bubble); with
//   gbar(tau_k,0)(P r; Q c) = sigma(Q, P (-) Q) gbar_rc(P (-) Q; tau_k),      gbar(0,tau_k) = -gbar(tau_{m-k},0)
// (the cyclic invariance of the weight; the end rows carry the delta term) thread d evaluates the connected term of cstb_walk -- the
// same table, masks, link factors and cstb_connected -- for the site pair (A, B) = (d, 0), with E from row k and T from row m - k, and adds
// cos(Q d) chibar_c(d) to its sum; a fixed tree over the 256 sums follows, and thread c writes pb[slot][b][k][c].
// k_series_ph_vertex, one thread per (slot, operator, output): the one-body value obar_c of row 0 at site 0, the tau quadrature of pb and
// the jackknife over b in index order.
struct PhVertexShape { size_t S, off_g, off_chi; int L, N, m, nfreq, nb, B, count, qx, qy, apbx, apby, R; double dtau; };
size_t series_ph_bubble_lds_bytes(int opdim, int N) { return (2 * measure_green_matrix_row_doubles(opdim, N) + (size_t)DQMC_CUSTOM_MAX * 256) * sizeof(double); }
// the sites (p, q) of block k at the stencil S = (sx, sy), Sx = (sxp, sy), Sy = (sx, syp) as coordinates, and its link factor (cstb_block)
__device__ __forceinline__ void phv_block(int k, int sx, int sy, int sxp, int syp, cplx ux, cplx uy, int& px, int& py, int& qx, int& qy, cplx& f) {
    px = k == 1 ? sxp : sx; py = k == 3 ? syp : sy;
    qx = k == 2 ? sxp : sx; qy = k == 4 ? syp : sy;
    const cplx u = k < 3 ? ux : uy;
    f = k == 0 ? make_double2(1.0, 0.0) : make_double2(u.x, (k & 1) ? u.y : -u.y);
}
template<int OPDIM>
__global__ __launch_bounds__(256) void k_series_ph_bubble(const double* __restrict__ bins, const double* __restrict__ mean,
                                                          const double* __restrict__ trig, CustomBondArg cb, PhVertexShape a,
                                                          double* __restrict__ pb) {
    constexpr int R = OPDIM == 3 ? 4 : 2;
    extern __shared__ __attribute__((aligned(16))) double phv_sm[];
    const int N = a.N, L = a.L, tid = threadIdx.x, count = cb.count, B = a.B;
    const int k = blockIdx.x, b = blockIdx.y, slot = blockIdx.z;
    const size_t rowlen = (size_t)2 * R * R * N, n = (size_t)a.nb * a.S, part = (size_t)slot * a.S + a.off_g;
    double* red = phv_sm + 2 * rowlen;                      // [DQMC_CUSTOM_MAX][256]
    for (size_t e = tid; e < 2 * rowlen; e += 256) {        // row k, then row m - k
        const size_t src = part + (size_t)(e < rowlen ? k : a.m - k) * rowlen + (e < rowlen ? e : e - rowlen);
        const double mu = mean[src];
        phv_sm[e] = b < B ? ((double)B * mu - bins[(size_t)b * n + src]) / (double)(B - 1) : mu;
    }
    __syncthreads();
    const cplx* gk = (const cplx*)phv_sm;
    const cplx* gr = gk + (size_t)R * R * N;
    const cplx* __restrict__ lk = cb.tab + (size_t)count * CSTB_K * 16;
    unsigned both[DQMC_CUSTOM_MAX];                         // bit 5 ka + kb: operator ch has the blocks ka and kb
    unsigned need = 0;
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) {
        both[ch] = 0;
        if (ch < count)
            for (int ka = 0; ka < CSTB_K; ++ka)
                if ((cb.parts[ch] >> ka) & 1u) both[ch] |= (cb.parts[ch] & 0x1fu) << (CSTB_K * ka);
        need |= both[ch];
    }
    double w[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
    const int B1 = 1 % L;                                   // the neighbours of site B = 0: (1, 0) and (0, 1)
    const cplx ubx = lk[0], uby = lk[N];
    for (int d = tid; d < N; d += 256) {
        const int ax = d % L, ay = d / L;
        const int axp = ax + 1 == L ? 0 : ax + 1, ayp = ay + 1 == L ? 0 : ay + 1;
        const cplx uax = lk[d], uay = lk[N + d];
        double v[DQMC_CUSTOM_MAX] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int pr = 0; pr < CSTB_K * CSTB_K; ++pr) {
            if (!((need >> pr) & 1u)) continue;
            const int ka = pr / CSTB_K, kb = pr % CSTB_K;
            int px, py, qx, qy, rx, ry, sx, sy;
            cplx fa, fb;
            phv_block(ka, ax, ay, axp, ayp, uax, uay, px, py, qx, qy, fa);
            phv_block(kb, 0, 0, B1, B1, ubx, uby, rx, ry, sx, sy, fb);
            const cplx f = m_mul(fa, fb);
            cplx e[R][R], t[R][R];
            pvx_load<R>(gk, L, a.apbx, a.apby, qx, qy, rx, ry, e);          // E_bc = gbar(tau_k,0)(A^q b; B^r c)
            pvx_load<R>(gr, L, a.apbx, a.apby, sx, sy, px, py, t);          // T_da = -gbar(tau_{m-k},0)(B^s d; A^p a)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c2 = 0; c2 < R; ++c2) {
                    e[r][c2] = m_mul(f, e[r][c2]);
                    t[r][c2] = make_double2(-t[r][c2].x, -t[r][c2].y);
                }
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
                if ((both[ch] >> pr) & 1u) {
                    const cplx* __restrict__ V = cb.tab + (size_t)ch * CSTB_K * 16;
                    v[ch] -= cstb_connected<OPDIM, R>(e, t, V + 16 * ka, cb.mk[ch * CSTB_K + ka], V + 16 * kb, cb.mk[ch * CSTB_K + kb]);
                }
        }
        const double cq = trig[(a.qx * ax + a.qy * ay) % L];
#pragma unroll
        for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) w[ch] += cq * v[ch];
    }
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) red[ch * 256 + tid] = w[ch];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                     // a fixed tree: the same order in every launch
        if (tid < h)
#pragma unroll
            for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) red[ch * 256 + tid] += red[ch * 256 + tid + h];
        __syncthreads();
    }
    if (tid < count) pb[(((size_t)slot * (B + 1) + b) * (a.m + 1) + k) * count + tid] = red[tid * 256];
}
// outputs per (slot, operator): 0 chi = Re chi(Q, i omega_0) of part 9 - D, 1 chibar = dtau sum_k w_k pb, 2 Gamma = 1 / chi - 1 / chibar,
// 3 Gamma chibar = chibar / chi - 1, 4 D = beta Re(obar^2) sum_d cos(Q d), then pb at k = 0 .. m; NaN where a denominator vanishes
__device__ __forceinline__ double phv_f(int e, double chi, double chib, double D) {
    if (e == 0) return chi;
    if (e == 1) return chib;
    if (e == 4) return D;
    if (chi == 0.0 || (e == 2 && chib == 0.0)) return nan("");
    return e == 2 ? 1.0 / chi - 1.0 / chib : chib / chi - 1.0;
}
__global__ __launch_bounds__(64) void k_series_ph_vertex(const double* __restrict__ bins, const double* __restrict__ mean, const double* __restrict__ pb,
                                                         CustomBondArg cb, PhVertexShape a, double* __restrict__ value, double* __restrict__ err) {
    const int per = 6 + a.m, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * a.count * per) return;
    const int slot = t / (a.count * per), c = (t / per) % a.count, e = t % per, B = a.B, m = a.m, L = a.L, N = a.N, R = a.R;
    const size_t n = (size_t)a.nb * a.S;
    const double* p = bins + (size_t)slot * a.S + a.off_chi + ((size_t)c * a.nfreq * N + (size_t)a.qy * L + a.qx) * 2;     // Re, frequency 0
    const double* r0 = pb + (size_t)slot * (B + 1) * (m + 1) * a.count + c;
    const size_t g0 = (size_t)slot * a.S + a.off_g;         // row 0 of part 13
    const cplx* __restrict__ V = cb.tab + (size_t)c * CSTB_K * 16;
    const cplx* __restrict__ lk = cb.tab + (size_t)a.count * CSTB_K * 16;
    const cplx ux = lk[0], uy = lk[N];
    const int B1 = 1 % L;
    const double dsum = (a.qx == 0 && a.qy == 0) ? (double)N : 0.0;      // sum_d cos(Q d)
    unsigned parts = 0;                                     // cb.parts[c] without a run-time index into the kernel argument
#pragma unroll
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch)
        if (ch == c) parts = cb.parts[ch];
    double sum = 0.0;
    for (int b = 0; b < B; ++b) sum += p[(size_t)b * n];
    const double mu = sum / (double)B, tot = (double)B * mu;
    // obar of jackknife index b: tr M0 - sum_k f_k sum_ab (W_k)_ab gbar(A^q b; A^p a) at A = 0 (cstb_onebody on the rebuilt matrix)
    auto onebody = [&](int b) {
        cplx s = make_double2(0.0, 0.0);
        for (int k = 0; k < CSTB_K; ++k) {
            if (!((parts >> k) & 1u)) continue;
            int px, py, qx, qy;
            cplx f;
            phv_block(k, 0, 0, B1, B1, ux, uy, px, py, qx, qy, f);
            int dx = qx - px, dy = qy - py;                 // gbar(P = A^q .; Q = A^p .) = sigma(Q, P (-) Q) gbar(P (-) Q)
            if (dx < 0) dx += L;
            if (dy < 0) dy += L;
            const double sg = ((a.apbx && px + dx >= L) != (a.apby && py + dy >= L)) ? -1.0 : 1.0;
            const size_t blk = g0 + (size_t)(dy * L + dx) * 2 * R * R;
            const unsigned mask = cb.mk[c * CSTB_K + k];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    if (!(mask & (1u << (4 * i + j)))) continue;
                    if (R == 2 && (i < 2) != (j < 2)) continue;         // the blocks between the sectors vanish
                    const bool cj = R == 2 && i >= 2;                   // the conjugate sector
                    const size_t src = blk + (size_t)2 * ((j & (R - 1)) * R + (i & (R - 1)));    // element (j, i) of the stored block
                    double re = mean[src], im = mean[src + 1];
                    if (b < B) {
                        re = ((double)B * re - bins[(size_t)b * n + src]) / (double)(B - 1);
                        im = ((double)B * im - bins[(size_t)b * n + src + 1]) / (double)(B - 1);
                    }
                    cplx x = m_mul(f, make_double2(sg * re, sg * im));
                    if (cj) x.y = -x.y;
                    cst_fma(s, V[16 * k + 4 * i + j], x);
                }
        }
        return m_sub(m_add(m_add(V[0], V[5]), m_add(V[10], V[15])), s);
    };
    auto theta = [&](int b) {
        const double* r = r0 + (size_t)b * (m + 1) * a.count;
        if (e >= 5) return r[(size_t)(e - 5) * a.count];
        double s = 0.0;
        for (int k = 0; k <= m; ++k) s += (k == 0 || k == m ? 0.5 : 1.0) * r[(size_t)k * a.count];
        const cplx o = onebody(b);
        const double D = a.dtau * (double)m * (o.x * o.x - o.y * o.y) * dsum;
        return phv_f(e, (b < B ? (tot - p[(size_t)b * n]) / (double)(B - 1) : mu) - D, a.dtau * s, D);
    };
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) tsum += theta(b);
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const double dl = theta(b) - tbar;
        acc += dl * dl;
    }
    value[t] = theta(B);
    err[t] = sqrt((double)(B - 1) / (double)B * acc);
}
// false: the lattice is too large for the bubble kernel's LDS, nothing was launched.  mean: the bin means [nb][S] (launch_series_stats)
bool launch_series_ph_vertex(const Launch& lc, const DevModel& hm, const double* bins, const double* mean, const double* trig, size_t S, int B,
                             int nfreq, size_t off_chi, size_t off_g, int count, const CustomBond& bond, int qx, int qy, int apbx, int apby,
                             double* pb, double* value, double* err) {
    const size_t lds = series_ph_bubble_lds_bytes(hm.opdim, hm.N);
    if (lds > 152 * 1024) return false;
    const CustomBondArg cb = custom_bond_arg(count, bond);
    const PhVertexShape a{S, off_g, off_chi, hm.L, hm.N, hm.m, nfreq, lc.nb, B, count, qx, qy, apbx, apby, hm.opdim == 3 ? 4 : 2, hm.dtau};
    const dim3 grid((unsigned)(hm.m + 1), (unsigned)(B + 1), (unsigned)lc.nb);
    dispatch_opdim(hm.opdim, [&](auto O) {
        const void* fn = (const void*)k_series_ph_bubble<decltype(O)::value>;
        if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
        hipLaunchKernelGGL((k_series_ph_bubble<decltype(O)::value>), grid, dim3(256), lds, lc.st, bins, mean, trig, cb, a, pb);
    });
    const int total = lc.nb * count * (6 + hm.m);
    hipLaunchKernelGGL(k_series_ph_vertex, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, lc.st, bins, mean, pb, cb, a, value, err);
    return true;
}

// End rows of the every-slice blocks (dqmc_measure_timedisplaced_ends): from the equal-time G = G(0), one elementwise pass writes
//   tau = 0+:    G(0+,0) = G,          G(0,0+) = G - 1          -> a_t0, a_0t
//   tau = beta-: G(beta-,0) = 1 - G,   G(0,beta-) = -G          -> b_t0, b_0t
// and a copy of G (the equal-time function of both rows) -> gtt.  Threads past the end read element 0 and store nothing.
__global__ __launch_bounds__(256) void k_td_ends(const cplx* __restrict__ G, cplx* __restrict__ a_t0, cplx* __restrict__ a_0t,
                                                 cplx* __restrict__ b_t0, cplx* __restrict__ b_0t, cplx* __restrict__ gtt, int ng, size_t cs) {
    CHAIN(G); CHAIN(a_t0); CHAIN(a_0t); CHAIN(b_t0); CHAIN(b_0t); CHAIN(gtt);
    const size_t total = (size_t)ng * ng, gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = gid < total;
    const size_t idx = valid ? gid : 0;
    const cplx g = G[idx];
    const double one = (idx % (size_t)ng == idx / (size_t)ng) ? 1.0 : 0.0;
    if (valid) {
        a_t0[idx] = g;
        a_0t[idx] = make_double2(g.x - one, g.y);
        b_t0[idx] = make_double2(one - g.x, -g.y);
        b_0t[idx] = make_double2(-g.x, -g.y);
        gtt[idx] = g;
    }
}

void launch_td_ends(const Launch& lc, const cplx* G, cplx* a_t0, cplx* a_0t, cplx* b_t0, cplx* b_0t, cplx* gtt, int ng) {
    const size_t total = (size_t)ng * ng;
    const dim3 grid((unsigned)((total + 255) / 256), 1, lc.nb);
    hipLaunchKernelGGL(k_td_ends, grid, dim3(256), 0, lc.st, G, a_t0, a_0t, b_t0, b_0t, gtt, ng, lc.cs);
}

// Matsubara transforms of one every-slice block (dqmc_measure_td_matsubara_host; definitions in dqmc_hip.h and DESIGN.md 6e).  With the
// rows row_k[e] of one component (a correlator over the N periodic site differences, or the (2L-1)^2 complex bins of one band), their
// sample counts and the trapezoid weights w_0 = w_m = 1/2,
//   A_n[e] = sum_k w_k cos(phi_nk) row_k[e] / count_k,   B_n[e] = sum_k w_k sin(phi_nk) row_k[e] / count_k,   phi_nk = omega_n tau_k,
// followed by the spatial Fourier sum of A_n and B_n.  phi_nk is a rational multiple of pi: 2 pi (n k mod m) / m for the bosonic
// frequencies, pi ((2n+1) k mod 2m) / m for the fermionic ones; the index is reduced in integers and goes through sincospi, so the
// twiddles of a large n k are as exact as those of a small one.  The same holds for the spatial phases (index mod 2L).
// Shape: one workgroup per (frequency tile, component, chain).  A tile of nf <= TDM_FT frequencies keeps its weighted twiddles
// tw[f][k] in LDS; thread e walks the rows k = 0 .. m of column e (lanes read consecutive doubles of a row) with the 2 nf sums in
// registers, so a tile reads its component once, and leaves A and B in LDS.  There the separable transform runs per frequency: first
// over y (lanes along x, stride 1), then over x (table rows padded to an odd length, so that lanes on consecutive k_x hit different
// banks).  Correlators: chi = F(A) + i F(B) = F(A + i B) with e^{-i q d}, one complex transform.  Channel 0: A and B are complex and
// G = Re F(A) + i Re F(B) with the phases e^{+i k (d - (L-1))}, k = -pi + (kk + 1/2 on antiperiodic directions) 2 pi / L, of the host's
// greenKTau sum: two transforms, each writes its half of the output element.  One writer per output element, fixed summation order
// (k, then y, then x ascending), no atomics.  bad[chain] = 1 if a row of the chain has a count < 1 (written by workgroup (0, 0) alone).
// TDM_FT, TdmShape and the separable transform tdm_dft2: dqmc_internal.h (k_hubbard_td_matsubara shares them)
size_t measure_td_matsubara_lds_doubles(int ftile, int m, int L, int W, int rlen) {
    const int WP = W | 1;
    return (size_t)ftile * (m + 1) * 2 + 2 * (size_t)(2 * L * WP) + (size_t)2 * L * W + (size_t)ftile * 2 * rlen;
}

__global__ __launch_bounds__(256) void k_td_matsubara(const double* __restrict__ acc, double* __restrict__ out, double* __restrict__ bad,
                                                      TdmShape a, size_t cs) {
    CHAIN(acc);
    extern __shared__ double tdm_sm[];
    const int tid = threadIdx.x, comp = blockIdx.y, rows = a.m + 1, m = a.m, L = a.L, W = a.W, WP = a.WP, R = a.rlen;
    const int f0 = blockIdx.x * a.ftile, nf = a.nfreq - f0 < a.ftile ? a.nfreq - f0 : a.ftile;
    const bool fermionic = a.channel == 0;
    double* tw = tdm_sm;                                    // [ftile][rows] (w_k cos / count_k, w_k sin / count_k)
    double* tx = tw + (size_t)a.ftile * rows * 2;           // [L][WP] (cos, sin)
    double* ty = tx + (size_t)2 * L * WP;
    double* T = ty + (size_t)2 * L * WP;                    // [L][W] complex, between the two passes
    double* Z = T + (size_t)2 * L * W;                      // [ftile][A, B][R]
    int anybad = 0;
    for (int k = tid; k < rows; k += 256) anybad |= !(acc[k] >= 1.0);
    for (int i = tid; i < nf * rows; i += 256) {
        const int f = i / rows, k = i - f * rows, n = f0 + f;
        const long long red = fermionic ? ((long long)(2 * n + 1) * k) % (2 * m) : (2 * (((long long)n * k) % m));
        double s, c;
        sincospi((double)red / (double)m, &s, &c);
        const double w = ((k == 0 || k == m) ? 0.5 : 1.0) / acc[k];
        tw[2 * i] = w * c; tw[2 * i + 1] = w * s;
    }
    for (int i = tid; i < L * W; i += 256) {
        const int kk = i / W, d = i - kk * W;
        int numx, numy;                                     // phase = pi num / L
        if (fermionic) { numx = (d - (L - 1)) * (2 * kk + a.apbx - L); numy = (d - (L - 1)) * (2 * kk + a.apby - L); }
        else numx = numy = -2 * kk * d;
        numx %= 2 * L; if (numx < 0) numx += 2 * L;
        numy %= 2 * L; if (numy < 0) numy += 2 * L;
        double s, c;
        sincospi((double)numx / (double)L, &s, &c);
        tx[2 * (kk * WP + d)] = c; tx[2 * (kk * WP + d) + 1] = s;
        sincospi((double)numy / (double)L, &s, &c);
        ty[2 * (kk * WP + d)] = c; ty[2 * (kk * WP + d) + 1] = s;
    }
    anybad = __syncthreads_or(anybad);
    if (blockIdx.x == 0 && comp == 0 && tid == 0) bad[blockIdx.z] = anybad ? 1.0 : 0.0;
    // time step: column e of the component, rows in ascending order
    const double* rowsp = acc + rows + (size_t)comp * R;
    for (int e0 = 0; e0 < R; e0 += 256) {
        const int e = e0 + tid;
        const bool valid = e < R;
        const double* p = rowsp + (valid ? e : 0);
        double A[TDM_FT], B[TDM_FT];
#pragma unroll
        for (int f = 0; f < TDM_FT; ++f) { A[f] = 0.0; B[f] = 0.0; }
#pragma unroll 4
        for (int k = 0; k < rows; ++k) {
            const double v = p[(size_t)k * a.stride];
#pragma unroll
            for (int f = 0; f < TDM_FT; ++f)
                if (f < nf) { A[f] += tw[2 * (f * rows + k)] * v; B[f] += tw[2 * (f * rows + k) + 1] * v; }
        }
        if (valid) {
#pragma unroll
            for (int f = 0; f < TDM_FT; ++f)
                if (f < nf) { Z[(size_t)(2 * f) * R + e] = A[f]; Z[(size_t)(2 * f + 1) * R + e] = B[f]; }
        }
    }
    __syncthreads();
    double* o = out + (size_t)blockIdx.z * a.ocs + ((size_t)comp * a.nfreq + f0) * (size_t)a.N * 2;
    for (int f = 0; f < nf; ++f, o += (size_t)a.N * 2) {
        const double* zA = Z + (size_t)(2 * f) * R;
        const double* zB = zA + R;
        const double sc = a.scale;
        if (fermionic) {
            tdm_dft2(a, tx, ty, T, zA, zA + 1, 2, [&](int q, double re, double) { o[2 * q] = sc * re; });
            tdm_dft2(a, tx, ty, T, zB, zB + 1, 2, [&](int q, double re, double) { o[2 * q + 1] = sc * re; });
        } else {
            tdm_dft2(a, tx, ty, T, zA, zB, 1, [&](int q, double re, double im) { o[2 * q] = sc * re; o[2 * q + 1] = sc * im; });
        }
    }
}

// out: [chain][component][nfreq][N] (re, im), bad: [chain]; both plain device arrays outside the arena.  Returns false if not even one
// frequency of the lattice fits the LDS of a workgroup (nothing is launched then).  out_chain_stride (doubles): distance between the
// results of consecutive chains, 0 = packed (components * nfreq * N * 2); the measurement series hands in its sample buffer this way.
static int tdm_ftile(const DevModel& hm, int channel, int nfreq) {
    const int L = hm.L, N = hm.N, m = hm.m, W = channel == 0 ? 2 * L - 1 : L;
    const int rlen = channel == 0 ? 2 * W * W : N;
    const size_t budget = 152 * 1024;
    int ftile = nfreq < TDM_FT ? nfreq : TDM_FT;
    while (ftile >= 1 && measure_td_matsubara_lds_doubles(ftile, m, L, W, rlen) * sizeof(double) > budget) --ftile;
    return ftile;
}
bool td_matsubara_fits(const DevModel& hm, int channel, int nfreq) { return tdm_ftile(hm, channel, nfreq) >= 1; }
bool launch_td_matsubara(const Launch& lc, const DevModel& hm, const double* acc, int channel, int nfreq, int apbx, int apby,
                         double* out, double* bad, size_t out_chain_stride, int custom_count, size_t custom_chain_bytes) {
    const int L = hm.L, N = hm.N, m = hm.m, W = channel == 0 ? 2 * L - 1 : L;
    const int rlen = channel == 0 ? 2 * W * W : N, ncomp = channel >= 5 ? custom_count : channel == 2 ? 3 : 2;
    const int stride = channel >= 5 ? (int)measure_custom_row_doubles(custom_count, N) : (int)measure_td_row_doubles(channel, N, L);
    const int ftile = tdm_ftile(hm, channel, nfreq);
    if (ftile < 1) return false;
    const size_t lds = measure_td_matsubara_lds_doubles(ftile, m, L, W, rlen) * sizeof(double);
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_td_matsubara, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        (void)hipGetLastError();                            // the launch below then reports the problem
    TdmShape a{channel, ncomp, nfreq, ftile, m, L, N, W, W | 1, rlen, stride, apbx, apby,
               hm.dtau / (channel == 0 ? 2.0 * N : (double)N), out_chain_stride ? out_chain_stride : (size_t)ncomp * nfreq * N * 2};
    const dim3 grid((nfreq + ftile - 1) / ftile, ncomp, lc.nb);
    hipLaunchKernelGGL(k_td_matsubara, grid, dim3(256), lds, lc.st, acc, out, bad, a, channel >= 5 ? custom_chain_bytes : lc.cs);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Measurement series (dqmc_series_*, dqmc_hip.h): one sample per measurement sweep, accumulated into bins on the device.
// All buffers are plain device arrays outside the arena, chain b of a [nb][S] array at b * S.  Every kernel has one writer per output
// element, a fixed summation order and no atomics; no element of one chain depends on another chain or on the number of chains.
// ---------------------------------------------------------------------------------------------------------------------------------
// Equal-time part of the sample, for a block count, X[nch][N] (nch = 5: the equal-time correlators, 2: the band-resolved charge block):
// C_X(d) = sum / (N count) into out[X][d], S_X(q) = sum_d cos(q d) C_X(d) into out[nch + X][q], column
// qy L + qx.  One workgroup per (channel X, chain): C_X in LDS, then the separable cosine sum in the order of the host's finishFermionic --
// over dx into (Ac, As)[dy][qx], then over dy -- with the phase index reduced mod L in integers and cos / sin(2 pi j / L) from the table
// `trig` = (cos[L], sin[L]) the host computed.  bad[chain] = 1 if the block's count is < 1 (written by the workgroup of channel 0).
size_t series_eq_sample_lds_bytes(int L) { return ((size_t)3 * L * L + 2 * (size_t)L) * sizeof(double); }
__global__ __launch_bounds__(256) void k_series_eq_sample(const double* __restrict__ eqacc, size_t eq_n, int nch, const double* __restrict__ trig,
                                                          double* __restrict__ sample, size_t S, size_t off, double* __restrict__ bad, int L) {
    extern __shared__ double ses_sm[];
    const int tid = threadIdx.x, ch = blockIdx.x, N = L * L;
    const double* blk = eqacc + (size_t)blockIdx.z * eq_n;
    double* out = sample + (size_t)blockIdx.z * S + off;
    double* C = ses_sm;                                     // [N]
    double* Ac = C + N;                                     // [dy][qx]
    double* As = Ac + N;
    double* ct = As + N;                                    // [L]
    double* st = ct + L;
    const double cnt = blk[0];
    if (ch == 0 && tid == 0) bad[blockIdx.z] = cnt >= 1.0 ? 0.0 : 1.0;
    for (int j = tid; j < L; j += 256) { ct[j] = trig[j]; st[j] = trig[L + j]; }
    const double den = (double)N * cnt;
    for (int d = tid; d < N; d += 256) {
        const double v = blk[1 + (size_t)ch * N + d] / den;
        C[d] = v;
        out[(size_t)ch * N + d] = v;
    }
    __syncthreads();
    series_cosine_sum(C, Ac, As, ct, st, out + (size_t)(nch + ch) * N, L, tid);
}
// false: the lattice is too large for the kernel's LDS, nothing was launched
bool launch_series_eq_sample(const Launch& lc, const DevModel& hm, const double* eqacc, size_t eq_n, int nch, const double* trig, double* sample,
                             size_t S, size_t off, double* bad) {
    const size_t lds = series_eq_sample_lds_bytes(hm.L);
    if (lds > 152 * 1024) return false;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_series_eq_sample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        (void)hipGetLastError();
    hipLaunchKernelGGL(k_series_eq_sample, dim3(nch, 1, lc.nb), dim3(256), lds, lc.st, eqacc, eq_n, nch, trig, sample, S, off, bad, hm.L);
    return true;
}

// open += sample over the n = nb S elements; close != 0: closed = open / bin_size and the open bin is cleared
__global__ __launch_bounds__(256) void k_series_accum(const double* __restrict__ sample, double* __restrict__ open, double* __restrict__ closed,
                                                      size_t n, int close, double bin_size) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double o = open[i] + sample[i];
    if (close) { closed[i] = o / bin_size; open[i] = 0.0; }
    else open[i] = o;
}
void launch_series_accum(const Launch& lc, const double* sample, double* open, double* closed, size_t n, int close, int bin_size) {
    hipLaunchKernelGGL(k_series_accum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lc.st, sample, open, closed, n, close, (double)bin_size);
}
// The same with the sample of slot s read through a pointer table: open[s] += src[s][0 .. S).  Grid (ceil(S / 256), nb), one thread per
// element of a slot row; the rows src points to may lie in the sample buffer of another context of the same device.  The two operations
// of k_series_accum in the same order, so the identity table gives its bits.
__global__ __launch_bounds__(256) void k_series_accum_routed(const double* const* __restrict__ src, double* __restrict__ open,
                                                             double* __restrict__ closed, size_t S, int close, double bin_size) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const size_t i = (size_t)blockIdx.y * S + j;
    const double o = open[i] + src[blockIdx.y][j];
    if (close) { closed[i] = o / bin_size; open[i] = 0.0; }
    else open[i] = o;
}
void launch_series_accum_routed(const Launch& lc, const double* const* src, double* open, double* closed, size_t S, int close, int bin_size) {
    hipLaunchKernelGGL(k_series_accum_routed, dim3((unsigned)((S + 255) / 256), (unsigned)lc.nb), dim3(256), 0, lc.st, src, open, closed, S,
                       close, (double)bin_size);
}

// Jackknife over the B closed bins, bins[b][n]: mean = (sum_b x_b) / B, x_(b) = (B mean - x_b) / (B - 1),
// err = sqrt((B - 1) / B sum_b (x_(b) - mean)^2).  One thread per element, bins in index order.
__global__ __launch_bounds__(256) void k_series_stats(const double* __restrict__ bins, size_t n, int B, double* __restrict__ mean,
                                                      double* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int b = 0; b < B; ++b) sum += bins[(size_t)b * n + i];
    const double mu = sum / (double)B, tot = (double)B * mu;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        const double d = (tot - bins[(size_t)b * n + i]) / (double)(B - 1) - mu;
        acc += d * d;
    }
    mean[i] = mu;
    err[i] = sqrt((double)(B - 1) / (double)B * acc);
}
void launch_series_stats(const Launch& lc, const double* bins, size_t n, int B, double* mean, double* err) {
    hipLaunchKernelGGL(k_series_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lc.st, bins, n, B, mean, err);
}

// Jackknifed derived quantities, out[chain][6]: entries 0 .. 4 the correlation ratios R_X = 1 - (S_X(Q + dx) + S_X(Q + dy)) / (2 S_X(Q)),
// Q = (L/2, L/2) for charge, spinZ, sdw and (0, 0) for pairPlus, pairMinus; entry 5 rho_s = 1/8 [Lxx(1,0) - Lxx(0,1) + Lyy(0,1) - Lyy(1,0)]
// at frequency 0 (real parts).  value = f(mean); err about the mean of theta_(b) = f(x_(b)).  off_eq / off_cur: offset of the equal-time
// part / of the channel-3 Matsubara part inside a sample, -1 if the part is not in the series (NaN then).  One thread per (chain, entry).
struct SeriesDerivedShape { long long off_eq, off_cur; int L, N, nfreq, nb, B; size_t S; };
__device__ __forceinline__ double series_derived_f(int e, const double* x) {
    if (e < 5) return 1.0 - 0.5 * (x[1] + x[2]) / x[0];
    return 0.125 * (x[0] - x[1] + x[2] - x[3]);
}
__global__ __launch_bounds__(64) void k_series_derived(const double* __restrict__ bins, SeriesDerivedShape a, double* __restrict__ value,
                                                       double* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * 6) return;
    const int chain = t / 6, e = t - chain * 6, L = a.L, N = a.N;
    const long long off = e < 5 ? a.off_eq : a.off_cur;
    if (off < 0) { value[t] = nan(""); err[t] = nan(""); return; }
    size_t idx[4];
    int cnt;
    if (e < 5) {
        const int Q = e < 3 ? L / 2 : 0, qx1 = (Q + 1) % L, qy1 = (Q + 1) % L;
        const size_t base = (size_t)off + (size_t)(5 + e) * N;
        idx[0] = base + (size_t)Q * L + Q; idx[1] = base + (size_t)Q * L + qx1; idx[2] = base + (size_t)qy1 * L + Q; idx[3] = idx[0];
        cnt = 3;
    } else {
        const size_t xx = (size_t)off, yy = (size_t)off + (size_t)a.nfreq * N * 2;     // component 0 / 1, frequency 0, real parts
        idx[0] = xx + 2 * (size_t)(1 % N); idx[1] = xx + 2 * (size_t)(L % N); idx[2] = yy + 2 * (size_t)(L % N); idx[3] = yy + 2 * (size_t)(1 % N);
        cnt = 4;
    }
    const size_t n = (size_t)a.nb * a.S;
    const double* p = bins + (size_t)chain * a.S;
    const int B = a.B;
    double mu[4] = {0.0, 0.0, 0.0, 0.0}, tot[4], x[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < cnt; ++j) {
        double sum = 0.0;
        for (int b = 0; b < B; ++b) sum += p[(size_t)b * n + idx[j]];
        mu[j] = sum / (double)B; tot[j] = (double)B * mu[j];
    }
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < cnt; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        tsum += series_derived_f(e, x);
    }
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < cnt; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        const double d = series_derived_f(e, x) - tbar;
        acc += d * d;
    }
    value[t] = series_derived_f(e, mu);
    err[t] = sqrt((double)(B - 1) / (double)B * acc);
}
void launch_series_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, int nfreq, long long off_eq,
                           long long off_cur, double* value, double* err) {
    SeriesDerivedShape a{off_eq, off_cur, hm.L, hm.N, nfreq, lc.nb, B, S};
    hipLaunchKernelGGL(k_series_derived, dim3((unsigned)((lc.nb * 6 + 63) / 64)), dim3(64), 0, lc.st, bins, a, value, err);
}

// The jackknife of k_series_derived over the equal-time band part, out[chain][3] (dqmc_hip.h): R = 1 - (S(Q + dx) + S(Q + dy)) / (2 S(Q)) for
// 0: bandDiff at Q = (L/2, L/2), 1: bandDiff at Q = (0, 0), 2: bandMix at Q = (L/2, L/2).  off = offset of the part inside a sample,
// S_X(q) at off + (2 + X) N.  One thread per (chain, entry).
struct SeriesBandDerivedShape { size_t S, off; int L, N, nb, B; };
// value and jackknife error of R over the B closed bins of one chain (p: its row of bin 0, n: distance between bins) from the three
// sample entries idx = S(Q), S(Q + dx), S(Q + dy)
__device__ __forceinline__ void series_ratio_jackknife(const double* __restrict__ p, size_t n, int B, const size_t (&idx)[3], double& value, double& err) {
    double mu[3], tot[3], x[3];
    for (int j = 0; j < 3; ++j) {
        double sum = 0.0;
        for (int b = 0; b < B; ++b) sum += p[(size_t)b * n + idx[j]];
        mu[j] = sum / (double)B; tot[j] = (double)B * mu[j];
    }
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        tsum += series_derived_f(0, x);
    }
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        const double d = series_derived_f(0, x) - tbar;
        acc += d * d;
    }
    value = series_derived_f(0, mu);
    err = sqrt((double)(B - 1) / (double)B * acc);
}
__global__ __launch_bounds__(64) void k_series_band_derived(const double* __restrict__ bins, SeriesBandDerivedShape a, double* __restrict__ value,
                                                            double* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * 3) return;
    const int chain = t / 3, e = t - chain * 3, L = a.L, N = a.N;
    const int Q = e == 1 ? 0 : L / 2, q1 = (Q + 1) % L;
    const size_t base = a.off + (size_t)(2 + (e == 2 ? 1 : 0)) * N;
    const size_t idx[3] = {base + (size_t)Q * L + Q, base + (size_t)Q * L + q1, base + (size_t)q1 * L + Q};
    series_ratio_jackknife(bins + (size_t)chain * a.S, (size_t)a.nb * a.S, a.B, idx, value[t], err[t]);
}
// the same for the equal-time part of the user-defined bilinears, out[chain][count]: R of matrix e at the caller's Q = (qx, qy);
// S_e(q) at off + (count + e) N
struct SeriesCustomDerivedShape { size_t S, off; int L, N, nb, B, count, qx, qy; };
__global__ __launch_bounds__(64) void k_series_custom_derived(const double* __restrict__ bins, SeriesCustomDerivedShape a, double* __restrict__ value,
                                                              double* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * a.count) return;
    const int chain = t / a.count, e = t - chain * a.count, L = a.L;
    const size_t base = a.off + (size_t)(a.count + e) * a.N;
    const size_t idx[3] = {base + (size_t)a.qy * L + a.qx, base + (size_t)a.qy * L + (a.qx + 1) % L, base + (size_t)((a.qy + 1) % L) * L + a.qx};
    series_ratio_jackknife(bins + (size_t)chain * a.S, (size_t)a.nb * a.S, a.B, idx, value[t], err[t]);
}
void launch_series_custom_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, int count, int qx, int qy,
                                  double* value, double* err) {
    SeriesCustomDerivedShape a{S, off, hm.L, hm.N, lc.nb, B, count, qx, qy};
    hipLaunchKernelGGL(k_series_custom_derived, dim3((unsigned)((lc.nb * count + 63) / 64)), dim3(64), 0, lc.st, bins, a, value, err);
}
void launch_series_band_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, double* value, double* err) {
    SeriesBandDerivedShape a{S, off, hm.L, hm.N, lc.nb, B};
    hipLaunchKernelGGL(k_series_band_derived, dim3((unsigned)((lc.nb * 3 + 63) / 64)), dim3(64), 0, lc.st, bins, a, value, err);
}

// The derived quantities of a Hubbard series (dqmc_series_hubbard_derived_host), out[chain][19], from the S_X(q) half of the equal-time part
// (off: offset of the part, S_X(q) of channel X at off + (8 + X) N) at the caller's Q = (qx, qy):
//   0 .. 7   R_X = 1 - Sbar_X / S_X(Q), Sbar = 1/2 [S(Q + dx) + S(Q + dy)], for the eight channels (series_ratio_jackknife)
//   8 .. 15  xi_X = sqrt(S_X(Q) / Sbar_X - 1) / (2 sin(pi / L)), the definition of xi_phi above
//   16 .. 18 S(Q), R and xi of the rotation-summed spin channel S_spin = S_spinZZ + 2 S_spinXX, formed bin by bin
// value = f(bin mean), err = jackknife over theta_(b) = f(x_(b)) about their mean.  NaN rule: value is NaN where the root's argument of
// f(mean) is negative or a denominator vanishes; err is NaN where that holds for the mean or for any leave-one-out set; no other entry
// is affected.  One thread per (chain, entry), bins in index order.
struct SeriesHubbardDerivedShape { size_t S, off; int L, N, nb, B, qx, qy; double twosin; };
// kind 0: S(Q), 1: R, 2: xi
__device__ __forceinline__ double series_hubbard_derived_f(int kind, const double* x, double twosin) {
    if (kind == 0) return x[0];
    const double sbar = 0.5 * (x[1] + x[2]);
    if (kind == 1) return x[0] != 0.0 ? 1.0 - sbar / x[0] : nan("");
    if (sbar == 0.0) return nan("");
    const double arg = x[0] / sbar - 1.0;
    return arg >= 0.0 ? sqrt(arg) / twosin : nan("");
}
__global__ __launch_bounds__(64) void k_series_hubbard_derived(const double* __restrict__ bins, SeriesHubbardDerivedShape a, double* __restrict__ value,
                                                               double* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * 19) return;
    const int chain = t / 19, e = t - chain * 19, L = a.L, B = a.B;
    const size_t q[3] = {(size_t)a.qy * L + a.qx, (size_t)a.qy * L + (a.qx + 1) % L, (size_t)((a.qy + 1) % L) * L + a.qx};
    const size_t n = (size_t)a.nb * a.S;
    const double* p = bins + (size_t)chain * a.S;
    const int X = e < 16 ? (e & 7) : 3;                      // the spin entries: spinZZ (3) + 2 spinXX (4)
    const size_t base = a.off + (size_t)(8 + X) * a.N;
    const size_t idx[3] = {base + q[0], base + q[1], base + q[2]};
    if (e < 8) {
        series_ratio_jackknife(p, n, B, idx, value[t], err[t]);
        // the NaN rule for a vanishing S_X(Q), in the mean or in a leave-one-out set
        double sum = 0.0;
        for (int b = 0; b < B; ++b) sum += p[(size_t)b * n + idx[0]];
        const double mu = sum / (double)B, tot = (double)B * mu;
        bool bad = false;
        for (int b = 0; b < B; ++b) bad = bad || (tot - p[(size_t)b * n + idx[0]]) / (double)(B - 1) == 0.0;
        if (mu == 0.0) value[t] = nan("");
        if (mu == 0.0 || bad) err[t] = nan("");
        return;
    }
    const int kind = e < 16 ? 2 : e - 16;
    const double w = e < 16 ? 0.0 : 2.0;                     // weight of the spinXX column next to spinZZ's
    const size_t N = (size_t)a.N;
    double mu[3], tot[3], x[3];
    for (int j = 0; j < 3; ++j) {
        double sum = 0.0;
        for (int b = 0; b < B; ++b) {
            const double* r = p + (size_t)b * n + idx[j];
            sum += w != 0.0 ? r[0] + w * r[N] : r[0];
        }
        mu[j] = sum / (double)B; tot[j] = (double)B * mu[j];
    }
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) {
            const double* r = p + (size_t)b * n + idx[j];
            x[j] = (tot[j] - (w != 0.0 ? r[0] + w * r[N] : r[0])) / (double)(B - 1);
        }
        tsum += series_hubbard_derived_f(kind, x, a.twosin);
    }
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) {
            const double* r = p + (size_t)b * n + idx[j];
            x[j] = (tot[j] - (w != 0.0 ? r[0] + w * r[N] : r[0])) / (double)(B - 1);
        }
        const double d = series_hubbard_derived_f(kind, x, a.twosin) - tbar;
        acc += d * d;
    }
    const double v = series_hubbard_derived_f(kind, mu, a.twosin);
    value[t] = v;
    err[t] = v != v ? nan("") : sqrt((double)(B - 1) / (double)B * acc);      // a NaN theta_(b) has made acc NaN already
}
void launch_series_hubbard_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, int qx, int qy,
                                   double* value, double* err) {
    SeriesHubbardDerivedShape a{S, off, hm.L, hm.N, lc.nb, B, qx, qy, 2.0 * std::sin(M_PI / (double)hm.L)};
    hipLaunchKernelGGL(k_series_hubbard_derived, dim3((unsigned)((lc.nb * 19 + 63) / 64)), dim3(64), 0, lc.st, bins, a, value, err);
}

// ---- the order-parameter part of the sample (DQMC_SERIES_PHI): chi_phi(q, i omega_n) and five scalars straight from the field ----
// out[chain] = chi [nfreq][N] then the scalars [5] (dqmc_hip.h).  A_d(n, q) = (1/K) sum_k sum_r phi_d(r, k) e^{+i 2 pi n k / m}
// e^{-i q r}, chi = sum_d |A_d|^2, K = m N.  Grid (frequency groups, 1, chains), 256 threads; a group holds fg <= SPHI_FG consecutive
// frequencies.  Per component d:
//   stage 0  thread t owns sites t, t + 256, ... (coalesced loads) and walks k = 1 .. m upwards, four slices in flight, with the fg
//            complex accumulators in registers: phi is read once per group.  The phase index j = n k mod m is stepped in integers
//            (j += n, minus m on overflow), cos / sin(2 pi j / m) come from the host table `ttab` = (cos[m], sin[m]) kept in LDS.
//            T[f][y][x] goes to LDS.
//   stage 1  over x: U[f][y][qx] = sum_x T[f][y][x] (cos - i sin)(2 pi (qx x mod L) / L), table `trig` of the equal-time kernel
//   stage 2  over y: A[f][qy][qx] = sum_y U[f][y][qx] (cos - i sin)(2 pi (qy y mod L) / L) / K; the thread that owns element (f, q)
//            adds |A|^2 to chi[f][q] in LDS -- always the same thread, d in order: one writer, no atomics.
// Group 0 (it holds n = 0) forms the scalars from a second pass over the field, which the first pass left in the L2: wave w takes
// the rows (k, d) = w, w + 4, ..., its lanes the sites lane, lane + 64, ...; the site sum of a row is a butterfly over the wave (every
// lane ends with the same bits), sum phi^2 stays per lane until the end; the four wave results are added in wave order by thread 0.
// Nothing depends on another chain, on the number of chains or on the grouping of the frequencies.
constexpr int SPHI_FG = 4;
size_t series_phi_sample_lds_bytes(int L, int m, int fg) {
    return ((size_t)5 * fg * L * L + 2 * (size_t)L + 2 * (size_t)m + 8) * sizeof(double);
}
// frequencies per workgroup: as many as SPHI_FG while the tile stays within 64 KiB, a single one up to the 152 KiB of the other sample
// kernels; 0: even a single frequency does not fit
int series_phi_sample_fgroup(int L, int m, int nfreq) {
    for (int fg = nfreq < SPHI_FG ? nfreq : SPHI_FG; fg > 1; --fg)
        if (series_phi_sample_lds_bytes(L, m, fg) <= 64 * 1024) return fg;
    return series_phi_sample_lds_bytes(L, m, 1) <= 152 * 1024 ? 1 : 0;
}
struct SeriesPhiShape { int L, N, m, opdim, nfreq, fg; size_t S, off; };
__device__ __forceinline__ double sphi_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(256) void k_series_phi_sample(const double* __restrict__ phi, const double* __restrict__ trig,
                                                           const double* __restrict__ ttab, double* __restrict__ sample, SeriesPhiShape a,
                                                           size_t cs) {
    extern __shared__ __attribute__((aligned(16))) double sphi_sm[];
    CHAIN(phi);
    const int tid = threadIdx.x, L = a.L, N = a.N, m = a.m, OPD = a.opdim;
    const int n0 = blockIdx.x * a.fg, fg = min(a.fg, a.nfreq - n0), fN = fg * N;
    double* out = sample + (size_t)blockIdx.z * a.S + a.off;
    double* Tr = sphi_sm;                                   // [fg][y][x]
    double* Ti = Tr + (size_t)a.fg * N;
    double* Ur = Ti + (size_t)a.fg * N;                     // [fg][y][qx]
    double* Ui = Ur + (size_t)a.fg * N;
    double* chi = Ui + (size_t)a.fg * N;                    // [fg][q]
    double* ct = chi + (size_t)a.fg * N;                    // [L]
    double* st = ct + L;
    double* tc = st + L;                                    // [m]
    double* ts = tc + m;
    double* red = ts + m;                                   // [8]
    for (int j = tid; j < L; j += 256) { ct[j] = trig[j]; st[j] = trig[L + j]; }
    for (int j = tid; j < m; j += 256) { tc[j] = ttab[j]; ts[j] = ttab[m + j]; }
    for (int e = tid; e < fN; e += 256) chi[e] = 0.0;
    __syncthreads();
    const double K = (double)m * (double)N;
    const size_t kstride = (size_t)OPD * N;
    for (int d = 0; d < OPD; ++d) {
        for (int r = tid; r < N; r += 256) {
            const double* p = phi + kstride + (size_t)d * N + r;      // slice 1
            double are[SPHI_FG], aim[SPHI_FG];
            int j[SPHI_FG];
#pragma unroll
            for (int f = 0; f < SPHI_FG; ++f) { are[f] = 0.0; aim[f] = 0.0; j[f] = f < fg ? n0 + f : 0; }   // n k mod m at k = 1 (n < m)
            int k = 1;
            for (; k + 3 <= m; k += 4) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = p[(size_t)u * kstride];
                p += 4 * kstride;
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int f = 0; f < SPHI_FG; ++f)
                        if (f < fg) {
                            are[f] += v[u] * tc[j[f]]; aim[f] += v[u] * ts[j[f]];
                            j[f] += n0 + f; if (j[f] >= m) j[f] -= m;
                        }
            }
            for (; k <= m; ++k) {
                const double v = *p;
                p += kstride;
#pragma unroll
                for (int f = 0; f < SPHI_FG; ++f)
                    if (f < fg) {
                        are[f] += v * tc[j[f]]; aim[f] += v * ts[j[f]];
                        j[f] += n0 + f; if (j[f] >= m) j[f] -= m;
                    }
            }
#pragma unroll
            for (int f = 0; f < SPHI_FG; ++f)
                if (f < fg) { Tr[f * N + r] = are[f]; Ti[f * N + r] = aim[f]; }
        }
        __syncthreads();
        for (int e = tid; e < fN; e += 256) {
            const int f = e / N, i = e - f * N, y = i / L, qx = i - y * L;
            const double* tr = Tr + f * N + y * L;
            const double* ti = Ti + f * N + y * L;
            double sr = 0.0, si = 0.0;
            for (int x = 0; x < L; ++x) {
                const int jj = (qx * x) % L;
                const double c = ct[jj], s = st[jj];
                sr += tr[x] * c + ti[x] * s; si += ti[x] * c - tr[x] * s;
            }
            Ur[e] = sr; Ui[e] = si;
        }
        __syncthreads();
        for (int e = tid; e < fN; e += 256) {
            const int f = e / N, q = e - f * N, qy = q / L, qx = q - qy * L;
            const double* ur = Ur + f * N + qx;
            const double* ui = Ui + f * N + qx;
            double sr = 0.0, si = 0.0;
            for (int y = 0; y < L; ++y) {
                const int jj = (qy * y) % L;
                const double c = ct[jj], s = st[jj];
                sr += ur[y * L] * c + ui[y * L] * s; si += ui[y * L] * c - ur[y * L] * s;
            }
            sr /= K; si /= K;
            chi[e] += sr * sr + si * si;
        }
        // the next component's stage 0 writes T, which stage 2 does not read; its stage 1 writes U behind the barrier after stage 0
    }
    for (int e = tid; e < fN; e += 256) out[(size_t)n0 * N + e] = chi[e];
    if (blockIdx.x != 0) return;
    // the scalars: rows (k, d) of the field, k = 1 .. m, lie behind each other from phi + OPD N
    const int w = tid >> 6, lane = tid & 63, rows = m * OPD;
    double eqs = 0.0, sq = 0.0;
    for (int row = w; row < rows; row += 4) {
        const double* p = phi + kstride + (size_t)row * N;
        double s = 0.0;
        for (int r = lane; r < N; r += 64) { const double v = p[r]; s += v; sq += v * v; }
        s = sphi_wave_sum(s) / (double)N;
        eqs += s * s;
    }
    sq = sphi_wave_sum(sq);
    if (lane == 0) { red[w] = eqs; red[4 + w] = sq; }
    __syncthreads();
    if (tid == 0) {
        const double c0 = chi[0];
        double* sc = out + (size_t)a.nfreq * N;
        sc[0] = sqrt(c0); sc[1] = c0; sc[2] = c0 * c0;
        sc[3] = (((red[0] + red[1]) + red[2]) + red[3]) * ((double)N / (double)m);
        sc[4] = (((red[4] + red[5]) + red[6]) + red[7]) / (2.0 * (double)N * (double)m);
    }
}
// Once per series, on the series' device: lets the kernel use the whole 152 KiB, the ceiling of series_phi_sample_fgroup, so that no
// launch depends on an attribute call of its own and contexts with different tiles do not lower each other's limit
hipError_t series_phi_sample_prepare() {
    return hipFuncSetAttribute((const void*)k_series_phi_sample, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
}
// false: the lattice is too large for the kernel's LDS, nothing was launched (dqmc_series_begin refuses such a series)
bool launch_series_phi_sample(const Launch& lc, const DevModel& hm, const double* trig, const double* ttab, int nfreq, double* sample,
                              size_t S, size_t off) {
    const int fg = series_phi_sample_fgroup(hm.L, hm.m, nfreq);
    if (fg < 1) return false;
    const size_t lds = series_phi_sample_lds_bytes(hm.L, hm.m, fg);           // within the limit series_phi_sample_prepare has set
    SeriesPhiShape a{hm.L, hm.N, hm.m, hm.opdim, nfreq, fg, S, off};
    hipLaunchKernelGGL(k_series_phi_sample, dim3((unsigned)((nfreq + fg - 1) / fg), 1, lc.nb), dim3(256), lds, lc.st, hm.phi, trig, ttab,
                       sample, a, lc.cs);
    return true;
}
// The jackknife of k_series_derived over the order-parameter part, out[chain][6] (dqmc_hip.h): off = offset of the part inside a
// sample, x = (|phibar|, |phibar|^2, |phibar|^4) for entries 0 .. 3 and (chi0, chix, chiy) at frequency 0 for entries 4, 5.
struct SeriesPhiDerivedShape { size_t S, off; int L, N, nfreq, nb, B; double betaN, twosin; };
__device__ __forceinline__ double series_phi_derived_f(int e, const double* x, double betaN, double twosin) {
    switch (e) {
    case 0: return 1.0 - x[2] / (3.0 * x[1] * x[1]);
    case 1: return x[2] / (x[1] * x[1]);
    case 2: return betaN * x[1];
    case 3: return betaN * (x[1] - x[0] * x[0]);
    case 4: return 1.0 - 0.5 * (x[1] + x[2]) / x[0];
    default: {
        const double arg = x[0] / (0.5 * (x[1] + x[2])) - 1.0;
        return arg >= 0.0 ? sqrt(arg) / twosin : nan("");
    }
    }
}
__global__ __launch_bounds__(64) void k_series_phi_derived(const double* __restrict__ bins, SeriesPhiDerivedShape a, double* __restrict__ value,
                                                           double* __restrict__ err) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.nb * 6) return;
    const int chain = t / 6, e = t - chain * 6;
    size_t idx[3];
    if (e < 4) { const size_t sc = a.off + (size_t)a.nfreq * a.N; idx[0] = sc; idx[1] = sc + 1; idx[2] = sc + 2; }
    else { idx[0] = a.off; idx[1] = a.off + (size_t)(1 % a.N); idx[2] = a.off + (size_t)(a.L % a.N); }
    const size_t n = (size_t)a.nb * a.S;
    const double* p = bins + (size_t)chain * a.S;
    const int B = a.B;
    double mu[3], tot[3], x[3];
    for (int j = 0; j < 3; ++j) {
        double sum = 0.0;
        for (int b = 0; b < B; ++b) sum += p[(size_t)b * n + idx[j]];
        mu[j] = sum / (double)B; tot[j] = (double)B * mu[j];
    }
    double tsum = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        tsum += series_phi_derived_f(e, x, a.betaN, a.twosin);
    }
    const double tbar = tsum / (double)B;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < 3; ++j) x[j] = (tot[j] - p[(size_t)b * n + idx[j]]) / (double)(B - 1);
        const double d = series_phi_derived_f(e, x, a.betaN, a.twosin) - tbar;
        acc += d * d;
    }
    value[t] = series_phi_derived_f(e, mu, a.betaN, a.twosin);
    err[t] = sqrt((double)(B - 1) / (double)B * acc);
}
void launch_series_phi_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, int nfreq, size_t off,
                               double* value, double* err) {
    SeriesPhiDerivedShape a{S, off, hm.L, hm.N, nfreq, lc.nb, B, (double)hm.m * hm.dtau * (double)hm.N, 2.0 * std::sin(M_PI / (double)hm.L)};
    hipLaunchKernelGGL(k_series_phi_derived, dim3((unsigned)((lc.nb * 6 + 63) / 64)), dim3(64), 0, lc.st, bins, a, value, err);
}

// ---- long runs: re-binning, running variance, binning analysis (dqmc_series_rebin / _configure / _binning_host) ----------------
// closed[k] = (closed[2k] + closed[2k+1]) * 0.5 for k < half, in place over the n = nb S elements.  One thread per element walks k
// upwards: it reads bins 2k and 2k + 1 >= k of its own element after it wrote bins < k, and no other thread touches the element.
__global__ __launch_bounds__(256) void k_series_rebin(double* __restrict__ bins, size_t n, int half) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < half; ++k) {
        const double a = bins[(size_t)(2 * k) * n + i], b = bins[(size_t)(2 * k + 1) * n + i];
        bins[(size_t)k * n + i] = (a + b) * 0.5;
    }
}
void launch_series_rebin(const Launch& lc, double* bins, size_t n, int half) {
    hipLaunchKernelGGL(k_series_rebin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lc.st, bins, n, half);
}

// Welford's update of the running mean w and the sum of squared deviations m2 with the sample of every slot, cnt = the number of samples
// including this one: d = x - w; w += d / cnt; m2 += d (x - w).  Grid (ceil(S / 256), nb); src == nullptr: slot s takes row s of
// `sample`, otherwise the row src[s] (the table of k_series_accum_routed).  One writer per element.
__global__ __launch_bounds__(256) void k_series_welford(const double* __restrict__ sample, const double* const* __restrict__ src,
                                                        double* __restrict__ w, double* __restrict__ m2, size_t S, double cnt) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    const size_t i = (size_t)blockIdx.y * S + j;
    const double x = src ? src[blockIdx.y][j] : sample[i];
    const double d = x - w[i];
    const double wn = w[i] + d / cnt;
    w[i] = wn;
    m2[i] += d * (x - wn);
}
void launch_series_welford(const Launch& lc, const double* sample, const double* const* src, double* w, double* m2, size_t S, long long cnt) {
    hipLaunchKernelGGL(k_series_welford, dim3((unsigned)((S + 255) / 256), (unsigned)lc.nb), dim3(256), 0, lc.st, sample, src, w, m2, S,
                       (double)cnt);
}

// Binning analysis: level l holds B_l = B >> l merged bins y^l_k, y^0_k = closed bin k, y^l_k = (y^(l-1)_2k + y^(l-1)_(2k+1)) * 0.5 --
// what l calls of k_series_rebin would leave; closed bins beyond 2^l B_l never complete a merged bin of level l and do not enter it.
// err[l] = the jackknife error of k_series_stats over y^l_0 .. y^l_(B_l - 1); tau[l] = 1/2 err[l]^2 (B_l 2^l bin_size) / sigma^2 with
// sigma^2 = m2 / (samples - 1), NaN unless sigma^2 > 0 (tau == nullptr: not formed).  One thread per element streams the bins twice,
// once for the level means and once for the squared deviations: bin k is added to level 0, and whenever a level completes a pair the
// merged value moves one level up.  The half-finished pair of every level (carry) and the sums live in registers: the level loops run
// to the compile-time SERIES_MAX_LEVELS and are fully unrolled, so no array is indexed at run time.  Sums in index order, no atomics.
constexpr int SERIES_MAX_LEVELS = 12;
struct SeriesBinningShape { size_t n; int B, levels; double bin_size, samples; };
__global__ __launch_bounds__(256) void k_series_binning(const double* __restrict__ bins, const double* __restrict__ m2, SeriesBinningShape a,
                                                        double* __restrict__ err, double* __restrict__ tau) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t n = a.n;
    const int B = a.B, levels = a.levels;
    double carry[SERIES_MAX_LEVELS], sum[SERIES_MAX_LEVELS], mu[SERIES_MAX_LEVELS], tot[SERIES_MAX_LEVELS], inv[SERIES_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < SERIES_MAX_LEVELS; ++l) { carry[l] = 0.0; sum[l] = 0.0; }
    for (int k = 0; k < B; ++k) {
        double y = bins[(size_t)k * n + i];
        bool live = true;
#pragma unroll
        for (int l = 0; l < SERIES_MAX_LEVELS; ++l) {
            if (live && l < levels) {
                sum[l] += y;
                if ((k >> l) & 1) y = (carry[l] + y) * 0.5;      // the pair of level l is complete: its mean is the next value of level l + 1
                else { carry[l] = y; live = false; }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < SERIES_MAX_LEVELS; ++l) {
        const double Bl = (double)(B >> l);
        mu[l] = sum[l] / Bl; tot[l] = Bl * mu[l]; inv[l] = Bl - 1.0; sum[l] = 0.0; carry[l] = 0.0;
    }
    for (int k = 0; k < B; ++k) {
        double y = bins[(size_t)k * n + i];
        bool live = true;
#pragma unroll
        for (int l = 0; l < SERIES_MAX_LEVELS; ++l) {
            if (live && l < levels) {
                const double d = (tot[l] - y) / inv[l] - mu[l];
                sum[l] += d * d;
                if ((k >> l) & 1) y = (carry[l] + y) * 0.5;
                else { carry[l] = y; live = false; }
            }
        }
    }
    const double var = tau ? m2[i] / (a.samples - 1.0) : 0.0;
#pragma unroll
    for (int l = 0; l < SERIES_MAX_LEVELS; ++l) {
        if (l < levels) {
            const double Bl = (double)(B >> l);
            const double e = sqrt((Bl - 1.0) / Bl * sum[l]);
            err[(size_t)l * n + i] = e;
            if (tau) tau[(size_t)l * n + i] = var > 0.0 ? 0.5 * e * e * (Bl * (double)(1 << l) * a.bin_size) / var : nan("");
        }
    }
}
void launch_series_binning(const Launch& lc, const double* bins, const double* m2, size_t n, int B, int levels, int bin_size,
                           long long samples, double* err, double* tau) {
    SeriesBinningShape a{n, B, levels, (double)bin_size, (double)samples};
    hipLaunchKernelGGL(k_series_binning, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lc.st, bins, m2, a, err, tau);
}
