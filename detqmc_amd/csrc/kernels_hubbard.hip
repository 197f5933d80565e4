// Hubbard replica on gfx950 (BASELINE config 1; reference src/dethubbard.{h,cpp}).
//
// The reference keeps two real N x N Green's functions (spin up / down: DetModelGC<2, double, false>).  Here both live
// in ONE n_g = 2N block-diagonal matrix G = blockdiag(G_up, G_dn) stored like every other matrix of this library
// (complex fp64, imaginary parts zero), so that the whole stabilisation machinery -- dense-propagator B-multiplies on
// the MFMA GEMM, UdV / UDT factorisations, greenFromUdV, wrap / advance -- is shared with the SDW model:
//   B_k = blockdiag( diag(e^{+alpha s_k}) P, diag(e^{-alpha s_k}) P ),   P = proptmat = e^{-dtau T}   (dethubbard.cpp:823-849)
// What is specific to the model is in this file:
//   k_hubbard_vscale   the site-diagonal factor diag(e^{+-alpha s}) of B_k^{+-1} applied to rows (left) / columns (right)
//   k_hubbard_slice    updateInSlice (:141-172): N single-spin-flip proposals at RANDOM sites (randInt, with replacement),
//                      weightRatioSingleFlip (:858-874), Metropolis, rank-1 Sherman-Morrison update of both spin blocks
//                      (updateGreenFunctionWithFlip, :877-906) -- one workgroup per replica walks the whole slice
//   k_hubbard_measure  measure(timeslice) (:521-545): sums over G_ii, nearest-neighbour G_ij and the spin-z correlation
//   k_hubbard_corr_prep, k_hubbard_corr   equal-time and time-displaced correlators over all site differences (not in the reference)
//   k_hubbard_td_matsubara   chi_X(q, i omega_n) and G_s(k, i omega_n) of the every-slice block
#include "dqmc_internal.h"
#include "bin_walk.h"

__global__ void k_hubbard_vscale(DevModel dm, cplx* __restrict__ A, int lda, int right, double sgn, int k, size_t cs) {
    dm = chain_model(dm, cs); CHAIN(A);
    const int N = dm.N, ng = dm.ng;
    const double ep = dm.hub_exp_alpha[0], em = dm.hub_exp_alpha[1];       // e^{+alpha}, e^{-alpha}
    const double* s = dm.phi + (size_t)k * N;
    const size_t total = (size_t)ng * ng;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx % ng), j = (int)(idx / ng);
        const int e = right ? j : i;
        const double spin = (e < N) ? +1.0 : -1.0;                           // Spin::Up = +1 block 0, Spin::Down = -1 block 1
        const double x = sgn * spin * s[e < N ? e : e - N];                   // exponent is x * alpha, x = +-1
        const double f = x > 0.0 ? ep : em;
        cplx v = A[(size_t)j * lda + i];
        A[(size_t)j * lda + i] = make_double2(v.x * f, v.y * f);
    }
}
void launch_hubbard_vscale(const Launch& lc, const DevModel& hm, int side, int inverse, int k, cplx* A, int lda) {
    const size_t total = (size_t)hm.ng * hm.ng;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_hubbard_vscale, dim3(blocks, 1, lc.nb), dim3(256), 0, lc.st, hm, A, lda, side == DQMC_RIGHT ? 1 : 0,
                       inverse ? -1.0 : +1.0, k, lc.cs);
}

// e_m2a = exp(-2 alpha), e_p2a = exp(+2 alpha), computed by the host with the C library like the reference does
__global__ __launch_bounds__(256) void k_hubbard_slice(DevModel dm, DevUpdateState* __restrict__ us, const double* __restrict__ uniforms,
                                                        cplx* __restrict__ G, int k, double e_m2a, double e_p2a, size_t cs) {
    extern __shared__ double hsm[];                 // [2][N] columns G(:, site), [2][N] rows delta(site, :) - G(site, :)
    __shared__ int s_site, s_acc;
    __shared__ double s_fac[2];
    dm = chain_model(dm, cs); CHAIN(us); CHAIN(uniforms); CHAIN(G);
    const int N = dm.N, ng = dm.ng, tid = threadIdx.x;
    double* col = hsm;
    double* row = hsm + 2 * N;
    double* field = dm.phi + (size_t)k * N;
    unsigned long long cursor = 0, avail = 0;
    int accepted = 0;
    if (tid == 0) { cursor = us->pub.rng_consumed; avail = us->pub.rng_avail; }
    for (int count = 0; count < N; ++count) {
        if (tid == 0) {
            int site = -1, acc = 0;
            if (cursor < avail) {
                const double u = uniforms[cursor++];
                site = (int)(((double)(N - 1) - 0.0 + 1.0) * u);             // randInt(0, N-1): low + int((high - low + 1.0) * rand01())
                const double a = field[site];
                const double eu = a > 0.0 ? e_m2a : e_p2a;                    // exp(-2 alpha a)
                const double ed = a > 0.0 ? e_p2a : e_m2a;                    // exp(+2 alpha a)
                const double gu = G[(size_t)site * ng + site].x, gd = G[(size_t)(N + site) * ng + (N + site)].x;
                const double du = eu - 1.0, dd = ed - 1.0;
                const double ru = __dadd_rn(1.0, __dmul_rn(du, 1.0 - gu));    // weightRatioSingleFlip, no fma contraction
                const double rd = __dadd_rn(1.0, __dmul_rn(dd, 1.0 - gd));
                const double ratio = __dmul_rn(ru, rd);
                acc = ratio > 1.0;
                if (!acc) {
                    if (cursor < avail) acc = uniforms[cursor++] < ratio;
                    else site = -1;
                }
                if (site >= 0 && acc) {
                    s_fac[0] = du / ru;                                        // deltaSite / (1 + deltaSite (1 - g_ss))
                    s_fac[1] = dd / rd;
                    field[site] = -a;
                }
            }
            s_site = site; s_acc = acc;
        }
        __syncthreads();
        const int site = s_site, acc = s_acc;
        if (site < 0) break;                                                   // window ran dry (uniform decision)
        if (acc) {
            accepted += 1;
            for (int i = tid; i < N; i += 256) {
                col[i] = G[(size_t)site * ng + i].x;
                col[N + i] = G[(size_t)(N + site) * ng + (N + i)].x;
                row[i] = (i == site ? 1.0 : 0.0) - G[(size_t)i * ng + site].x;
                row[N + i] = (i == site ? 1.0 : 0.0) - G[(size_t)(N + i) * ng + (N + site)].x;
            }
            __syncthreads();
            const double f0 = s_fac[0], f1 = s_fac[1];
            for (int idx = tid; idx < N * N; idx += 256) {
                const int x = idx % N, y = idx / N;
                G[(size_t)y * ng + x].x -= __dmul_rn(__dmul_rn(col[x], f0), row[y]);
                G[(size_t)(N + y) * ng + (N + x)].x -= __dmul_rn(__dmul_rn(col[N + x], f1), row[N + y]);
            }
        }
        __syncthreads();                                                       // s_site / col / row are rewritten next round
    }
    if (tid == 0) {
        if (s_site < 0) us->pub.error = DQMC_ERNG;
        us->pub.rng_consumed = cursor;
        us->pub.lastAccRatio = (double)accepted / (double)N;
        us->updates_accepted += (unsigned long long)accepted;
    }
}
void launch_hubbard_slice(const Launch& lc, const DevModel& hm, DevUpdateState* us, const double* uniforms, cplx* G, int k,
                          double e_m2a, double e_p2a) {
    hipLaunchKernelGGL(k_hubbard_slice, dim3(1, 1, lc.nb), dim3(256), 4 * (size_t)hm.N * sizeof(double), lc.st, hm, us, uniforms, G, k,
                       e_m2a, e_p2a, lc.cs);
}

// acc: [0] sum G_ii up, [1] sum G_ii down, [2] sum G_<ij> up, [3] down, [4] sum G_ii,up G_ii,dn, [5] slices, [6 .. 6+N) zcorr
__global__ __launch_bounds__(256) void k_hubbard_measure(DevModel dm, const cplx* __restrict__ G, double* __restrict__ acc, size_t cs) {
    __shared__ double red[5][256];
    dm = chain_model(dm, cs); CHAIN(G); CHAIN(acc);
    const int N = dm.N, ng = dm.ng, tid = threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int site = tid; site < N; site += 256) {
        const double gu = G[(size_t)site * ng + site].x, gd = G[(size_t)(N + site) * ng + (N + site)].x;
        v[0] += gu; v[1] += gd; v[4] += gu * gd;
        for (int dir = 0; dir < 4; ++dir) {
            const int nb = dm.neigh[dir * N + site];
            v[2] += G[(size_t)nb * ng + site].x;                                // gUp(site, site_neigh)
            v[3] += G[(size_t)(N + nb) * ng + (N + site)].x;
        }
    }
    for (int q = 0; q < 5; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) for (int q = 0; q < 5; ++q) red[q][tid] += red[q][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        for (int q = 0; q < 5; ++q) acc[q] += red[q][0];
        acc[5] += 1.0;
    }
    const double u0 = G[0].x, d0 = G[(size_t)N * ng + N].x;
    for (int j = tid; j < N; j += 256) {
        double z;
        if (j == 0) z = -2.0 * u0 * d0 + u0 + d0;
        else {
            const double u0j = G[(size_t)j * ng].x, d0j = G[(size_t)(N + j) * ng + N].x;
            const double ujj = G[(size_t)j * ng + j].x, djj = G[(size_t)(N + j) * ng + (N + j)].x;
            z = u0 * ujj - u0 * djj + d0 * djj - d0 * ujj - u0j * u0j - d0j * d0j;
        }
        acc[6 + j] += z;
    }
}
void launch_hubbard_measure(const Launch& lc, const DevModel& hm, const cplx* G, double* acc) {
    hipLaunchKernelGGL(k_hubbard_measure, dim3(1, 1, lc.nb), dim3(256), 0, lc.st, hm, G, acc, lc.cs);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Equal-time and time-displaced correlators (dqmc_hubbard_* in dqmc_hip.h; definitions and layouts in DESIGN.md).  G_s(A, B) =
// <c_As c^+_Bs> is the .x half of spin block s of an n_g x n_g matrix (block 0 up, 1 down); the off-diagonal blocks are never read.
// Two launches per sample, all chains each:
//   k_hubbard_corr_prep   fills a per-chain scratch of doubles, everything the walk would otherwise read strided or sixteen-fold:
//                           tU, tD [N][N]   tX[B N + A] = T_s(B, A), the spin blocks of T transposed through a 32 x 32 LDS tile
//                           sS, sD [N][N]   sX[B N + A] = sum_{dl, dl'} f_dl f_dl' S_dn(A + dl, B + dl'), f = +1 (extended s) and
//                                           f = +1 on +-x, -1 on +-y (d wave); only with a stencil source S
//                           ob [4][N]       n_up, n_dn of the tau side (1 - Gt_s(A, A)), then of the 0 side (1 - G0_s(B, B))
//   k_hubbard_corr<TD>    the displacement walk of bin_walk.h: a workgroup of TDP_BINS * TDP_PARTS threads owns 32 displacements d,
//                         thread (part, d) sums the pairs (A = B (+) d, B), B = part, part + 8, ...; every load is one element per
//                         pair at B ld + A, consecutive in A over the lanes.  One writer per accumulator, fixed order, no atomics.
// The scratch and the blocks may live outside the arena: they carry chain strides of their own (bytes).
size_t hubbard_corr_scratch_doubles(int N) { return 4 * (size_t)N * N + 4 * (size_t)N; }
size_t hubbard_eq_doubles(int N) { return 1 + HUB_EQ_CH * (size_t)N; }
size_t hubbard_td_doubles(int N, int n) { return (size_t)(n - 1) * (1 + HUB_TD_CH * (size_t)N); }
size_t hubbard_td_fine_doubles(int N, int m) { return (size_t)(m + 1) * (1 + HUB_EQ_CH * (size_t)N); }

__global__ __launch_bounds__(256) void k_hubbard_corr_prep(DevModel dm, const cplx* __restrict__ T, const cplx* __restrict__ S,
                                                            const cplx* __restrict__ Gt, const cplx* __restrict__ G0,
                                                            double* __restrict__ sc, size_t cs, size_t scs) {
    __shared__ double tile[2][32][33];
    CHAIN(T); CHAIN(S); CHAIN(Gt); CHAIN(G0);
    sc = chain_ptr(sc, scs);
    const int N = dm.N, tx = threadIdx.x % 32, ty = threadIdx.x / 32;
    const size_t ng = (size_t)dm.ng, NN = (size_t)N * N;
    const int tiles = (N + 31) / 32, A0 = (blockIdx.x % tiles) * 32, B0 = (blockIdx.x / tiles) * 32;
    double *tU = sc, *tD = sc + NN, *sS = sc + 2 * NN, *sD = sc + 3 * NN, *ob = sc + 4 * NN;
    // lanes along B, the row index of T: tile[a][b] = T_s(B0 + b, A0 + a)
    for (int a = ty; a < 32; a += 8)
        if (A0 + a < N && B0 + tx < N) {
            tile[0][a][tx] = T[(size_t)(A0 + a) * ng + (B0 + tx)].x;
            tile[1][a][tx] = T[(size_t)(N + A0 + a) * ng + (N + B0 + tx)].x;
        }
    __syncthreads();
    // lanes along A
    for (int b = ty; b < 32; b += 8) {
        const int A = A0 + tx, B = B0 + b;
        if (A >= N || B >= N) continue;
        const size_t idx = (size_t)B * N + A;
        tU[idx] = tile[0][tx][b];
        tD[idx] = tile[1][tx][b];
        if (S) {
            double ss = 0.0, sd = 0.0;
            for (int q = 0; q < 4; ++q) {                                       // dl' on B: XPLUS, XMINUS, YPLUS, YMINUS
                const size_t col = (size_t)(N + dm.neigh[q * N + B]) * ng + N;
                const double xs = S[col + dm.neigh[A]].x + S[col + dm.neigh[N + A]].x;           // dl = +-x
                const double ys = S[col + dm.neigh[2 * N + A]].x + S[col + dm.neigh[3 * N + A]].x;   // dl = +-y
                ss += xs + ys;
                sd += q < 2 ? xs - ys : ys - xs;
            }
            sS[idx] = ss;
            sD[idx] = sd;
        }
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < N; i += 256) {
            ob[i] = 1.0 - Gt[(size_t)i * ng + i].x;
            ob[N + i] = 1.0 - Gt[(size_t)(N + i) * ng + (N + i)].x;
            ob[2 * N + i] = 1.0 - G0[(size_t)i * ng + i].x;
            ob[3 * N + i] = 1.0 - G0[(size_t)(N + i) * ng + (N + i)].x;
        }
}
void launch_hubbard_corr_prep(const Launch& lc, const DevModel& hm, const cplx* T, const cplx* S, const cplx* Gt, const cplx* G0, double* sc,
                              size_t scs) {
    const int tiles = (hm.N + 31) / 32;
    hipLaunchKernelGGL(k_hubbard_corr_prep, dim3(tiles * tiles, 1, lc.nb), dim3(256), 0, lc.st, hm, T, S, Gt, G0, sc, lc.cs, scs);
}

// TD = 0: g = G of the slice, the scratch of (T, S) = (G, G): <c^+_A c_B> = delta_AB - G(B, A).  Block: count, [HUB_EQ_CH][N].
// TD = 1: g = G(tau,0), the scratch of T = G(0,tau), no stencil: <c^+_A(tau) c_B(0)> = -G(0,tau)(B, A).  Row `row` of count[rows], [rows][HUB_TD_CH][N].
// TD = 2: the forms of TD = 1 and, from the scratch of (T, S) = (G(0,tau), G(tau,0)), the two bond channels.  Row `row` of count[rows], [rows][HUB_EQ_CH][N].
template<int TD>
__global__ __launch_bounds__(TDP_BINS * TDP_PARTS) void k_hubbard_corr(DevModel dm, const cplx* __restrict__ g, const double* __restrict__ sc,
                                                                       double* __restrict__ acc, int row, int rows, size_t cs, size_t scs, size_t acs) {
    constexpr int NCH = TD == 1 ? HUB_TD_CH : HUB_EQ_CH;
    __shared__ double red[NCH][TDP_PARTS][TDP_BINS];
    CHAIN(g);
    sc = chain_ptr(sc, scs); acc = chain_ptr(acc, acs);
    const int N = dm.N, L = dm.L;
    const size_t ng = (size_t)dm.ng, NN = (size_t)N * N;
    const double *tU = sc, *tD = sc + NN, *sS = sc + 2 * NN, *sD = sc + 3 * NN, *ob = sc + 4 * NN;
    const BinWalk bw(N, L);
    const double dl = (!TD && bw.d == 0) ? 1.0 : 0.0;                           // delta_AB: the pairs of displacement 0
    double w[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) w[ch] = 0.0;
    for (BinSite st = bw.first(N, L); st.B < N; bw.next(st, L)) {
        const size_t idx = (size_t)st.B * N + st.A;
        const double gu = g[(size_t)st.B * ng + st.A].x, gd = g[(size_t)(N + st.B) * ng + (N + st.A)].x;
        const double hu = dl - tU[idx], hd = dl - tD[idx];                      // <c^+_A c_B> per spin
        const double nuA = ob[st.A], ndA = ob[N + st.A], nuB = ob[2 * N + st.B], ndB = ob[3 * N + st.B];
        const double conn = hu * gu + hd * gd;
        w[0] += gu;
        w[1] += gd;
        w[2] += (nuA + ndA) * (nuB + ndB) + conn;
        w[3] += 0.25 * ((nuA - ndA) * (nuB - ndB) + conn);
        w[4] += 0.25 * (hu * gd + hd * gu);
        w[5] += gu * gd;
        if (TD != 1) {
            w[NCH - 2] += 0.25 * gu * sS[idx];
            w[NCH - 1] += 0.25 * gu * sD[idx];
        }
    }
    double* dst = TD ? acc + rows + (size_t)row * NCH * N : acc + 1;
    bw.reduce_add(w, red, NCH, dst, N, 1, TD ? acc + row : acc);
}
void launch_hubbard_eq_corr(const Launch& lc, const DevModel& hm, const cplx* G, const double* sc, size_t scs, double* acc, size_t acs) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    hipLaunchKernelGGL(k_hubbard_corr<0>, grid, block, 0, lc.st, hm, G, sc, acc, 0, 1, lc.cs, scs, acs);
}
void launch_hubbard_td_corr(const Launch& lc, const DevModel& hm, const cplx* GT0, const double* sc, size_t scs, double* acc, size_t acs,
                            int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    hipLaunchKernelGGL(k_hubbard_corr<1>, grid, block, 0, lc.st, hm, GT0, sc, acc, row, rows, lc.cs, scs, acs);
}

void launch_hubbard_td_fine_corr(const Launch& lc, const DevModel& hm, const cplx* GT0, const double* sc, size_t scs, double* acc, size_t acs,
                                 int row, int rows) {
    const dim3 grid((hm.N + TDP_BINS - 1) / TDP_BINS, 1, lc.nb), block(TDP_BINS * TDP_PARTS);
    hipLaunchKernelGGL(k_hubbard_corr<2>, grid, block, 0, lc.st, hm, GT0, sc, acc, row, rows, lc.cs, scs, acs);
}

// Matsubara transforms of the every-slice block count[m+1], [m+1][HUB_EQ_CH][N] (dqmc_hubbard_td_matsubara_host; definitions in dqmc_hip.h
// and DESIGN.md 24), with the contract and the structure of k_td_matsubara (kernels_measure.hip): one workgroup per (frequency tile,
// channel, chain); the weighted twiddles tw[f][k] = w_k (cos, sin)(omega_n tau_k) / count_k of the tile in LDS, the phase index reduced in
// integers -- 2 (n k mod m) for the bosonic channels 2 .. 7, (2n+1) k mod 2m for the fermionic channels 0, 1 -- and handed to sincospi;
// thread e walks the rows k = 0 .. m of column e with the 2 nf sums in registers and leaves A = sum_k w_k cos C, B = sum_k w_k sin C in
// LDS; there one complex separable L x L transform per frequency, F(A + i B) with e^{-i q d} (the lattice is periodic: the fermionic
// channels use the same spatial phases).  One writer per output element, sums in ascending k, y, x, no atomics; threads past the end
// store nothing.  bad[chain] = 1 if a row of the chain has a count < 1, written by workgroup (0, 0) of the chain alone.
__global__ __launch_bounds__(256) void k_hubbard_td_matsubara(const double* __restrict__ acc, double* __restrict__ out, double* __restrict__ bad,
                                                              TdmShape a, size_t cs) {
    CHAIN(acc);
    extern __shared__ double htm_sm[];
    const int tid = threadIdx.x, comp = blockIdx.y, rows = a.m + 1, m = a.m, L = a.L, W = a.W, WP = a.WP, R = a.rlen;
    const int f0 = blockIdx.x * a.ftile, nf = a.nfreq - f0 < a.ftile ? a.nfreq - f0 : a.ftile;
    const bool fermionic = comp < 2;
    double* tw = htm_sm;                                    // [ftile][rows] (w_k cos / count_k, w_k sin / count_k)
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
        int num = (-2 * kk * d) % (2 * L);                  // phase = pi num / L
        if (num < 0) num += 2 * L;
        double s, c;
        sincospi((double)num / (double)L, &s, &c);
        tx[2 * (kk * WP + d)] = c; tx[2 * (kk * WP + d) + 1] = s;
        ty[2 * (kk * WP + d)] = c; ty[2 * (kk * WP + d) + 1] = s;
    }
    anybad = __syncthreads_or(anybad);
    if (blockIdx.x == 0 && comp == 0 && tid == 0) bad[blockIdx.z] = anybad ? 1.0 : 0.0;
    // time step: column e of the channel, rows in ascending order
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
        const double sc = a.scale;
        tdm_dft2(a, tx, ty, T, zA, zA + R, 1, [&](int q, double re, double im) { o[2 * q] = sc * re; o[2 * q + 1] = sc * im; });
    }
}
bool launch_hubbard_td_matsubara(const Launch& lc, const DevModel& hm, const double* acc, int nfreq, double* out, double* bad) {
    const int L = hm.L, N = hm.N, m = hm.m;
    const size_t budget = 152 * 1024;
    int ftile = nfreq < TDM_FT ? nfreq : TDM_FT;
    while (ftile >= 1 && measure_td_matsubara_lds_doubles(ftile, m, L, L, N) * sizeof(double) > budget) --ftile;
    if (ftile < 1) return false;
    const size_t lds = measure_td_matsubara_lds_doubles(ftile, m, L, L, N) * sizeof(double);
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_hubbard_td_matsubara, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        (void)hipGetLastError();                            // the launch below then reports the problem
    TdmShape a{0, HUB_EQ_CH, nfreq, ftile, m, L, N, L, L | 1, N, HUB_EQ_CH * N, 0, 0, hm.dtau / (double)N, (size_t)HUB_EQ_CH * nfreq * N * 2};
    hipLaunchKernelGGL(k_hubbard_td_matsubara, dim3((nfreq + ftile - 1) / ftile, HUB_EQ_CH, lc.nb), dim3(256), lds, lc.st, acc, out, bad, a, lc.cs);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The parts of a Hubbard context in the measurement series (DQMC_SERIES_HUB_*, dqmc_hip.h).  They follow the contract of
// the series kernels in kernels_measure.hip: the blocks are only read, one writer per output element, a fixed summation order, no
// atomics, no element of a chain depends on another chain or on the number of chains.  The equal-time part needs no kernel of its
// own: ACC_HUB_EQ has the count, [nch][N] layout of k_series_eq_sample.
// ---------------------------------------------------------------------------------------------------------------------------------
// Part 14 from the block of k_hubbard_measure, a[0 .. 5 + N]: the eight scalars of DetHubbard::finishMeasurements with cnt = a[5] for the
// number of slices (occUp, occDn, occTotal, occDouble, localMoment, eKinetic, ePotential, eTotal), then zcorr[j] = a[6 + j] / cnt.
// One workgroup per chain: thread 0 writes the scalars and the flag bad[chain] = 1 if cnt < 1, the lanes write zcorr.
__global__ __launch_bounds__(64) void k_hubbard_series_scalars(const double* __restrict__ acc, size_t cs, double* __restrict__ sample, size_t S,
                                                               size_t off, double* __restrict__ bad, int N, double t, double U, double mu) {
    CHAIN(acc);
    double* out = sample + (size_t)blockIdx.z * S + off;
    const double cnt = acc[5];
    if (threadIdx.x == 0) {
        bad[blockIdx.z] = cnt >= 1.0 ? 0.0 : 1.0;
        const double inv = 1.0 / ((double)N * cnt);
        const double occUp = 1.0 - inv * acc[0], occDn = 1.0 - inv * acc[1], occTotal = occUp + occDn;
        const double occDouble = 1.0 + inv * (acc[4] - acc[0] - acc[1]);
        const double ePotential = U * occDouble;
        const double eKinetic = (t / ((double)N * cnt)) * (acc[2] + acc[3]) - mu * occTotal;
        out[0] = occUp; out[1] = occDn; out[2] = occTotal; out[3] = occDouble; out[4] = occTotal - 2 * occDouble;
        out[5] = eKinetic; out[6] = ePotential; out[7] = eKinetic + ePotential;
    }
    for (int j = threadIdx.x; j < N; j += 64) out[8 + j] = acc[6 + j] / cnt;
}
void launch_hubbard_series_scalars(const Launch& lc, const DevModel& hm, const double* slice, double t, double U, double mu, double* sample, size_t S,
                                   size_t off, double* bad) {
    hipLaunchKernelGGL(k_hubbard_series_scalars, dim3(1, 1, lc.nb), dim3(64), 0, lc.st, slice, lc.cs, sample, S, off, bad, hm.N, t, U, mu);
}
// Part 16 from the block count[rows], [rows][HUB_TD_CH][N], rows = n - 1: C_X(d, tau_j) = sum / (N count_j) into out[j][X][d], the layout of
// the block, and S_X(q, tau_j) = sum_d cos(q d) C_X(d, tau_j) into out[rows + j][X][q].  One workgroup per (channel X, row j, chain) stages
// its C in LDS like k_series_eq_sample -- (3 N + 2 L) doubles -- and runs the same cosine sum.  bad[chain] = 1 if any count_j < 1: one
// writer, thread 0 of the workgroup of channel 0 and row 0, which walks all the counts.
__global__ __launch_bounds__(256) void k_hubbard_series_td_sample(const double* __restrict__ acc, size_t cs, const double* __restrict__ trig,
                                                                  double* __restrict__ sample, size_t S, size_t off, double* __restrict__ bad, int L) {
    extern __shared__ double hts_sm[];
    CHAIN(acc);
    const int tid = threadIdx.x, ch = blockIdx.x, j = blockIdx.y, rows = gridDim.y, N = L * L;
    double* out = sample + (size_t)blockIdx.z * S + off;
    double* C = hts_sm;                                     // [N]
    double* Ac = C + N;                                     // [dy][qx]
    double* As = Ac + N;
    double* ct = As + N;                                    // [L]
    double* st = ct + L;
    if (ch == 0 && j == 0 && tid == 0) {
        double flag = 0.0;
        for (int r = 0; r < rows; ++r) if (!(acc[r] >= 1.0)) flag = 1.0;
        bad[blockIdx.z] = flag;
    }
    for (int i = tid; i < L; i += 256) { ct[i] = trig[i]; st[i] = trig[L + i]; }
    const size_t row = ((size_t)j * HUB_TD_CH + ch) * N;
    const double den = (double)N * acc[j];
    for (int d = tid; d < N; d += 256) {
        const double v = acc[rows + row + d] / den;
        C[d] = v;
        out[row + d] = v;
    }
    __syncthreads();
    series_cosine_sum(C, Ac, As, ct, st, out + (size_t)rows * HUB_TD_CH * N + row, L, tid);
}
bool launch_hubbard_series_td_sample(const Launch& lc, const DevModel& hm, const double* td, const double* trig, double* sample, size_t S, size_t off,
                                     double* bad) {
    const size_t lds = series_eq_sample_lds_bytes(hm.L);
    if (lds > 152 * 1024) return false;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_hubbard_series_td_sample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        (void)hipGetLastError();
    hipLaunchKernelGGL(k_hubbard_series_td_sample, dim3(HUB_TD_CH, hm.n - 1, lc.nb), dim3(256), lds, lc.st, td, lc.cs, trig, sample, S, off, bad, hm.L);
    return true;
}
