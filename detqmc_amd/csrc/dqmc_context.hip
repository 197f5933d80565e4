// C-ABI implementation (include/dqmc_hip.h): device context of one DQMC replica and the
// stabilised-sweep building blocks of DetModelGC (reference src/detmodel.h) on top of the kernels.
#include "dqmc_ctx.h"
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

void build_tournament(int nblk, std::vector<int>& out);   // kernels_svd.hip

thread_local std::string g_err;

// per-chain device memory: reserves a range of the arena layout; *p holds the offset (+256) until
// arena_commit turns it into chain 0's address.  p must stay where it is until then.
template<class T>
static int dalloc(dqmc_ctx* c, T** p, size_t count) {
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    *p = (T*)(uintptr_t)(c->arena_off + 256);
    c->fixups.push_back((void**)p);
    c->arena_off += bytes;
    return 0;
}
static int arena_commit(dqmc_ctx* c) {
    const size_t cs = c->arena_off;
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, cs * (size_t)c->nb));
    c->allocs.push_back(q);
    HIPCHK(hipMemsetAsync(q, 0, cs * (size_t)c->nb, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->arena = (char*)q;
    for (void** pp : c->fixups) *pp = c->arena + ((uintptr_t)*pp - 256);
    c->fixups.clear();
    c->lc = Launch{c->st, c->nb, cs};
    return 0;
}
extern "C" const char* dqmc_last_error(void) { return g_err.c_str(); }
static int set_slot_identity(dqmc_ctx* c, UdVSlot& sl);

// ---------------------------------------------------------------------------------------------
// model set-up on the host: plaquette tables (detsdwopdim.cpp:217-260, :1598-1684, :1788-1826)
// ---------------------------------------------------------------------------------------------
typedef std::complex<double> hc;

// Hermitian 4x4 eigen-decomposition by cyclic Jacobi (replaces arma::eig_sym of :1671)
static void herm4_exp(const hc H[4][4], double pref, hc out[4][4]) {
    hc A[4][4], Vv[4][4];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { A[i][j] = H[i][j]; Vv[i][j] = (i == j) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 4; ++p) for (int q = p + 1; q < 4; ++q) off += std::norm(A[p][q]);
        if (off < 1e-300) break;
        for (int p = 0; p < 4; ++p) for (int q = p + 1; q < 4; ++q) {
            double apq = std::abs(A[p][q]);
            if (apq < 1e-300) continue;
            hc ph = A[p][q] / apq;
            double app = A[p][p].real(), aqq = A[q][q].real();
            double zeta = (aqq - app) / (2.0 * apq);
            double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
            double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
            // J = [[cs, sn], [-sn conj(ph), cs conj(ph)]]:  A <- A J, V <- V J, then A <- J^H A
            for (int k = 0; k < 4; ++k) {
                hc akp = A[k][p], akq = A[k][q];
                A[k][p] = cs * akp - sn * std::conj(ph) * akq;
                A[k][q] = sn * akp + cs * std::conj(ph) * akq;
                hc vkp = Vv[k][p], vkq = Vv[k][q];
                Vv[k][p] = cs * vkp - sn * std::conj(ph) * vkq;
                Vv[k][q] = sn * vkp + cs * std::conj(ph) * vkq;
            }
            for (int k = 0; k < 4; ++k) {
                hc apk = A[p][k], aqk = A[q][k];
                A[p][k] = cs * apk - sn * ph * aqk;
                A[q][k] = sn * apk + cs * ph * aqk;
            }
        }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        hc acc = 0.0;
        for (int k = 0; k < 4; ++k) acc += Vv[i][k] * std::exp(pref * A[k][k].real()) * std::conj(Vv[j][k]);
        out[i][j] = acc;
    }
}

static void build_tables(const dqmc_params& p, std::vector<int>& psites, std::vector<hc>& pmats,
                         std::vector<double>& pabcd, std::vector<int>& neigh, bool all_half = false) {
    const int L = p.L, N = L * L, P = N / 4;
    neigh.assign(4 * N, 0);
    for (int site = 0; site < N; ++site) {
        int x = site % L, y = site / L;
        neigh[0 * N + site] = y * L + (x + 1) % L;
        neigh[1 * N + site] = y * L + (x - 1 + L) % L;
        neigh[2 * N + site] = ((y + 1) % L) * L + x;
        neigh[3 * N + site] = ((y - 1 + L) % L) * L + x;
    }
    psites.assign(2 * P * 4, 0);
    pmats.assign((size_t)2 * 2 * 2 * P * 16, hc(0.0));
    pabcd.assign((size_t)2 * 2 * 2 * P * 4, 0.0);
    const double hopHor[2] = {p.txhor, p.tyhor}, hopVer[2] = {p.txver, p.tyver};
    const bool apbc_x = (p.bc == DQMC_BC_APBC_X || p.bc == DQMC_BC_APBC_XY);
    const bool apbc_y = (p.bc == DQMC_BC_APBC_Y || p.bc == DQMC_BC_APBC_XY);
    const double zmag = p.weakZflux ? 1.0 / N : 0.0;    // zmag[XUP] = zmag[YDOWN] (:218-222, :1619-1620)
    const double pi = M_PI;
    for (int sub = 0; sub < 2; ++sub) {
        int pidx = 0;
        // plaquettes of a subgroup are disjoint, so their order is free: x runs fastest so that lanes working on
        // consecutive plaquettes touch LDS / memory 2 sites apart (the reference's y-fastest order would put them
        // 2 L sites = a multiple of the LDS bank period apart: 64-way bank conflicts in k_bmult_chain)
        for (int i2 = sub; i2 < L; i2 += 2)
            for (int i1 = sub; i1 < L; i1 += 2, ++pidx) {
                int i = i2 * L + i1, j = neigh[0 * N + i], k = neigh[2 * N + i], l = neigh[0 * N + k];
                const int corner[4] = {i, j, k, l};
                for (int q = 0; q < 4; ++q) psites[(sub * 4 + q) * P + pidx] = corner[q];
                const bool half = all_half || (sub == 1);
                for (int band = 0; band < 2; ++band)
                    for (int signIdx = 0; signIdx < 2; ++signIdx) {
                        const double sign = signIdx == 0 ? -1.0 : +1.0;
                        hc Mloc[16];
                        hc* M = Mloc;
                        const size_t tbl = (size_t)((band * 2 + signIdx) * 2 + sub);
                        if (!p.weakZflux) {
                            const double f = half ? 0.5 : 1.0;
                            double ch_hor = std::cosh(-f * p.dtau * hopHor[band]);
                            double sh_hor = sign * std::sinh(-f * p.dtau * hopHor[band]);
                            double ch_ver = std::cosh(-f * p.dtau * hopVer[band]);
                            double sh_ver = sign * std::sinh(-f * p.dtau * hopVer[band]);
                            if (apbc_x && i1 == L - 1) sh_hor *= -1;
                            if (apbc_y && i2 == L - 1) sh_ver *= -1;
                            double a = ch_hor * ch_ver, b = ch_ver * sh_hor, c = ch_hor * sh_ver, d = sh_hor * sh_ver;
                            const double rows[4][4] = {{a, b, c, d}, {b, a, d, c}, {c, d, a, b}, {d, c, b, a}};
                            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) M[r * 4 + q] = rows[r][q];
                            const double abcd[4] = {a, b, c, d};
                            for (int q = 0; q < 4; ++q) pabcd[(tbl * 4 + q) * P + pidx] = abcd[q];
                        } else {
                            double hh = hopHor[band], hv = hopVer[band];
                            if (apbc_x && i1 == L - 1) hh *= -1;
                            if (apbc_y && i2 == L - 1) hv *= -1;
                            int j1 = j % L, k2 = k / L;
                            hc ph_ij = std::exp(hc(0.0, -2.0 * pi * zmag * i2));
                            hc ph_kl = std::exp(hc(0.0, -2.0 * pi * zmag * k2));
                            hc ph_ik = 1.0, ph_jl = 1.0;
                            if (i2 == L - 1) {
                                ph_ik = std::exp(hc(0.0, +2.0 * pi * zmag * L * i1));
                                ph_jl = std::exp(hc(0.0, +2.0 * pi * zmag * L * j1));
                            }
                            hc H[4][4];
                            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) H[r][q] = 0.0;
                            H[0][1] = ph_ij * hh; H[0][2] = ph_ik * hv; H[1][3] = ph_jl * hv; H[2][3] = ph_kl * hh;
                            hc Hh[4][4];
                            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) Hh[r][q] = -(H[r][q] + std::conj(H[q][r]));
                            hc E[4][4];
                            herm4_exp(Hh, sign * (half ? 0.5 : 1.0) * p.dtau, E);
                            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) M[r * 4 + q] = E[r][q];
                        }
                        for (int e = 0; e < 16; ++e) pmats[(tbl * 16 + e) * P + pidx] = M[e];
                    }
            }
    }
}

// CB_NONE (checkerboard = false): dense hopping propagators.  setupPropK (detsdwopdim.cpp:1210-1285)
// builds K_band = -mu_band 1 - sum_<ij> t_ij (APBC signs, Peierls phases of zmag[XUP] = zmag[YDOWN]);
// computePropagator (detmodel.cpp:31-39) exponentiates it through eig_sym.  Here: cyclic Jacobi on
// the host (set-up only), out[signIdx] = blockdiag_b(e^{-+dtau K_band(b)}), n_g x n_g column-major.  As in
// computeBmatSDW (:1324-1474) every block b uses propK[b & 1], also the lower O(3) blocks.
static void herm_exp_dense(int n, std::vector<hc>& A, double pref_minus, double pref_plus,
                           std::vector<hc>& Eminus, std::vector<hc>& Eplus) {
    std::vector<hc> V((size_t)n * n, hc(0.0));            // row-major helpers: A[i*n+j]
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    double total = 0.0;
    for (auto& a : A) total += std::norm(a);
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) off += std::norm(A[(size_t)p * n + q]);
        if (off <= 1e-32 * total) break;
        for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) {
            double apq = std::abs(A[(size_t)p * n + q]);
            if (apq < 1e-300) continue;
            hc ph = A[(size_t)p * n + q] / apq;
            double app = A[(size_t)p * n + p].real(), aqq = A[(size_t)q * n + q].real();
            double zeta = (aqq - app) / (2.0 * apq);
            double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
            double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
            const hc cph = std::conj(ph);
            for (int k = 0; k < n; ++k) {                 // A <- A J, V <- V J
                hc akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                A[(size_t)k * n + p] = cs * akp - sn * cph * akq;
                A[(size_t)k * n + q] = sn * akp + cs * cph * akq;
                hc vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                V[(size_t)k * n + p] = cs * vkp - sn * cph * vkq;
                V[(size_t)k * n + q] = sn * vkp + cs * cph * vkq;
            }
            for (int k = 0; k < n; ++k) {                 // A <- J^H A
                hc apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                A[(size_t)p * n + k] = cs * apk - sn * ph * aqk;
                A[(size_t)q * n + k] = sn * apk + cs * ph * aqk;
            }
        }
    }
    Eminus.assign((size_t)n * n, hc(0.0)); Eplus.assign((size_t)n * n, hc(0.0));
    std::vector<double> em(n), ep(n);
    for (int k = 0; k < n; ++k) { double ev = A[(size_t)k * n + k].real(); em[k] = std::exp(pref_minus * ev); ep[k] = std::exp(pref_plus * ev); }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
        hc a = 0.0, b = 0.0;
        for (int k = 0; k < n; ++k) {
            hc vv = V[(size_t)i * n + k] * std::conj(V[(size_t)j * n + k]);
            a += vv * em[k]; b += vv * ep[k];
        }
        Eminus[(size_t)i * n + j] = a; Eplus[(size_t)i * n + j] = b;
    }
}

// Hopping matrix of one band's stored sector (setupPropK, detsdwopdim.cpp:1210-1285), row major K[row * N + col]: -mu on the diagonal,
// -t on the bonds with the APBC signs and the Peierls phases of zmag[XUP] / zmag[YDOWN]
static void build_hopping_K(const dqmc_params& p, const std::vector<int>& neigh, int band, std::vector<hc>& K) {
    const int L = p.L, N = L * L;
    const double hopHor[2] = {p.txhor, p.tyhor}, hopVer[2] = {p.txver, p.tyver}, mu[2] = {p.mux, p.muy};
    const bool apbc_x = (p.bc == DQMC_BC_APBC_X || p.bc == DQMC_BC_APBC_XY);
    const bool apbc_y = (p.bc == DQMC_BC_APBC_Y || p.bc == DQMC_BC_APBC_XY);
    const double zmag = p.weakZflux ? 1.0 / N : 0.0, pi = M_PI;
    K.assign((size_t)N * N, hc(0.0));
    for (int i = 0; i < N; ++i) K[(size_t)i * N + i] = -mu[band];
    for (int site = 0; site < N; ++site) {
        const int sx = site % L, sy = site / L;
        for (int dir = 0; dir < 4; ++dir) {           // XPLUS, XMINUS, YPLUS, YMINUS
            double hop = dir < 2 ? hopHor[band] : hopVer[band];
            if (apbc_x && ((sx == 0 && dir == 1) || (sx == L - 1 && dir == 0))) hop *= -1;
            if (apbc_y && ((sy == 0 && dir == 3) || (sy == L - 1 && dir == 2))) hop *= -1;
            hc phase = 1.0;
            if (dir == 0) phase = std::exp(hc(0.0, -2.0 * pi * zmag * sy));
            if (dir == 1) phase = std::exp(hc(0.0, +2.0 * pi * zmag * sy));
            if (dir == 2 && sy == L - 1) phase = std::exp(hc(0.0, +2.0 * pi * zmag * L * sx));
            if (dir == 3 && sy == 0) phase = std::exp(hc(0.0, -2.0 * pi * zmag * L * sx));
            K[(size_t)site * N + neigh[dir * N + site]] -= hop * phase;
        }
    }
}

static void build_dense_propK(const dqmc_params& p, const std::vector<int>& neigh, int MSF,
                              std::vector<hc>& out_minus, std::vector<hc>& out_plus, double tfac = 1.0) {
    const int L = p.L, N = L * L, ng = MSF * N;
    out_minus.assign((size_t)ng * ng, hc(0.0)); out_plus.assign((size_t)ng * ng, hc(0.0));
    for (int band = 0; band < 2; ++band) {
        std::vector<hc> K;
        build_hopping_K(p, neigh, band, K);
        std::vector<hc> Em, Ep;
        herm_exp_dense(N, K, -p.dtau * tfac, +p.dtau * tfac, Em, Ep);
        for (int b = band; b < MSF; b += 2)
            for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) {
                out_minus[(size_t)(b * N + j) * ng + (b * N + i)] = Em[(size_t)i * N + j];
                out_plus[(size_t)(b * N + j) * ng + (b * N + i)] = Ep[(size_t)i * N + j];
            }
    }
}

// Bond amplitudes of dqmc_measure_timedisplaced_current, bt[(mu * MSF + flavour) * N + site] = T_flavour(site) = K^flavour[site (+) mu, site]:
// read off the hopping matrices above.  Stored flavours XUP, YDOWN (, XDOWN, YUP for O(3), which has no flux: the same two bands again).
static void build_bond_table(const dqmc_params& p, const std::vector<int>& neigh, int MSF, std::vector<hc>& bt) {
    const int N = p.L * p.L;
    bt.assign((size_t)2 * MSF * N, hc(0.0));
    for (int band = 0; band < 2; ++band) {
        std::vector<hc> K;
        build_hopping_K(p, neigh, band, K);
        for (int mu = 0; mu < 2; ++mu)
            for (int site = 0; site < N; ++site) {
                const hc T = K[(size_t)neigh[(mu == 0 ? 0 : 2) * N + site] * N + site];
                for (int b = band; b < MSF; b += 2) bt[(size_t)(mu * MSF + b) * N + site] = T;
            }
    }
}

// Hubbard replica: blockdiag(P, P) and blockdiag(P^-1, P^-1), P = proptmat.
//   direct (checkerboard = false): tmat = -mu 1 - t sum_<ij>, P = e^{-dtau tmat} by diagonalisation (setupPropTmat_direct,
//     dethubbard.cpp:702-714 + computePropagator, detmodel.cpp:25-33), P^-1 = e^{+dtau tmat};
//   checkerboard (dos Santos 2003, setupPropTmat_checkerboard :717-770): the ordered product
//     (ch + sh kxa)(ch + sh kxb)(ch + sh kya)(ch + sh kyb), ch = cosh(dtau t), sh = sinh(dtau t), without a chemical
//     potential -- the reference writes the same product expanded into its 16 terms; P^-1 = reversed order, sh -> -sh.
// The reference inverts B numerically (arma::inv, dethubbard.h:318-337); the exact inverse agrees to rounding.
static void build_hubbard_propK(const dqmc_params& p, const std::vector<int>& neigh, std::vector<hc>& out_minus, std::vector<hc>& out_plus) {
    const int L = p.L, N = L * L, ng = 2 * N;
    const double t = p.txhor, mu = p.mux;
    std::vector<hc> Em, Ep;
    if (p.cb_none) {
        std::vector<hc> T((size_t)N * N, hc(0.0));
        for (int i = 0; i < N; ++i) T[(size_t)i * N + i] = -mu;
        for (int site = 0; site < N; ++site)
            for (int dir = 0; dir < 4; ++dir) T[(size_t)neigh[dir * N + site] * N + site] -= t;
        herm_exp_dense(N, T, -p.dtau, +p.dtau, Em, Ep);
    } else {
        const double ch = std::cosh(p.dtau * t), sh = std::sinh(p.dtau * t);
        auto bond_matrix = [&](int dirn, int parity, double shv) {          // ch 1 + shv k, k = bonds (a, a + dir) from sub-board `parity`
            std::vector<double> M((size_t)N * N, 0.0);
            for (int i = 0; i < N; ++i) M[(size_t)i * N + i] = ch;
            for (int y = 0; y < L; ++y)
                for (int x = 0; x < L; ++x) {
                    const int coord = dirn == 0 ? x : y;
                    if ((coord & 1) != parity) continue;
                    const int a = y * L + x, b = neigh[(dirn == 0 ? 0 : 2) * N + a];
                    M[(size_t)a * N + b] += shv; M[(size_t)b * N + a] += shv;
                }
            return M;
        };
        auto mul = [&](const std::vector<double>& A, const std::vector<double>& B) {
            std::vector<double> C((size_t)N * N, 0.0);
            for (int i = 0; i < N; ++i) for (int k = 0; k < N; ++k) { const double a = A[(size_t)i * N + k]; if (a != 0.0) for (int j = 0; j < N; ++j) C[(size_t)i * N + j] += a * B[(size_t)k * N + j]; }
            return C;
        };
        const std::vector<double> F = mul(mul(bond_matrix(0, 0, sh), bond_matrix(0, 1, sh)), mul(bond_matrix(1, 0, sh), bond_matrix(1, 1, sh)));
        const std::vector<double> Fi = mul(mul(bond_matrix(1, 1, -sh), bond_matrix(1, 0, -sh)), mul(bond_matrix(0, 1, -sh), bond_matrix(0, 0, -sh)));
        Em.assign((size_t)N * N, hc(0.0)); Ep.assign((size_t)N * N, hc(0.0));
        for (size_t i = 0; i < (size_t)N * N; ++i) { Em[i] = F[i]; Ep[i] = Fi[i]; }
    }
    out_minus.assign((size_t)ng * ng, hc(0.0)); out_plus.assign((size_t)ng * ng, hc(0.0));
    for (int b = 0; b < 2; ++b)
        for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) {
            out_minus[(size_t)(b * N + j) * ng + (b * N + i)] = Em[(size_t)i * N + j];
            out_plus[(size_t)(b * N + j) * ng + (b * N + i)] = Ep[(size_t)i * N + j];
        }
}

// ---------------------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------------------
// workspace of the QR-mode factorisations and of the scale-split inverse inside greenFromUdV (green_qr)
static int alloc_qr_work(dqmc_ctx* c) {
    const int ng = c->n_g, np = (ng + 15) / 16;
    const size_t n2 = (size_t)ng * ng;
    int rc;
#define A_(x) if ((rc = (x))) return rc;
    A_(dalloc(c, &c->qw.V, n2)); A_(dalloc(c, &c->qw.T, (size_t)np * 2 * 256));
    A_(dalloc(c, &c->qw.W, (size_t)16 * ng)); A_(dalloc(c, &c->qw.W2, (size_t)16 * ng)); A_(dalloc(c, &c->qw.Rneg, (size_t)32 * ng));
    if (ng > 1024) { c->qw.part_count = (size_t)ng * 64 * 8; A_(dalloc(c, &c->qw.part, c->qw.part_count)); }   // split-K scratch of the block Gram-Schmidt QR
    A_(dalloc(c, &c->qr_perm, (size_t)ng)); A_(dalloc(c, &c->lu_swaps, (size_t)LU_SWAP_INTS)); A_(dalloc(c, &c->lu_tneg, (size_t)ng * 32)); A_(dalloc(c, &c->qr_perm_inv, (size_t)ng)); A_(dalloc(c, &c->qr_dinv, (size_t)ng));
    A_(dalloc(c, &c->rmax_inv, (size_t)ng)); A_(dalloc(c, &c->rmin, (size_t)ng));
    A_(dalloc(c, &c->lmax_inv, (size_t)ng)); A_(dalloc(c, &c->lmin, (size_t)ng));
#undef A_
    return 0;
}

static int alloc_slot(dqmc_ctx* c, UdVSlot& sl) {
    size_t n2 = (size_t)c->n_g * c->n_g;
    int rc;
    if ((rc = dalloc(c, &sl.U, n2))) return rc;
    if ((rc = dalloc(c, &sl.d, (size_t)c->n_g))) return rc;
    if ((rc = dalloc(c, &sl.Vt, n2))) return rc;
    return 0;
}

extern "C" int dqmc_create(const dqmc_params* p, dqmc_ctx** out) { return dqmc_create_batch(p, 1, out); }
static int create_fill(dqmc_ctx* c, const dqmc_params* p);

extern "C" int dqmc_create_batch(const dqmc_params* p, int nchains, dqmc_ctx** out) {
    if (!p || !out) return fail(DQMC_EINVAL, "null argument");
    *out = nullptr;
    if (nchains < 1 || nchains > 1024) return fail(DQMC_EINVAL, "nchains must be in 1..1024");
    // parameter rules of ModelParamsDetSDW::check (detsdwparams.cpp:21-140) that concern the kernels
    if (p->opdim < 1 || p->opdim > 3) return fail(DQMC_EINVAL, "opdim must be 1, 2 or 3");
    if (p->L < 2 || (p->L % 2) != 0)
        return fail(DQMC_EINVAL, "Checker board decomposition only supported for even linear lattice sizes");
    if (p->weakZflux && p->opdim != 2) return fail(DQMC_EINVAL, "Magnetic field currently only supported for opdim=2");
    if (p->m < 2 || p->s < 1 || p->s >= p->m) return fail(DQMC_EINVAL, "need 0 < s < m");
    const int N = p->L * p->L, MSF = p->opdim == 3 ? 4 : 2;
    if (p->delaySteps < 1 || p->delaySteps > N) return fail(DQMC_EINVAL, "delaySteps must be in 1..N");
    if (MSF * p->delaySteps > DQMC_MAX_WDIM) return fail(DQMC_EINVAL, "MSF*delaySteps must be <= 64 on this build");
    if (p->bc < 0 || p->bc > 3) return fail(DQMC_EINVAL, "bc");
    if (p->tuning.decide_threads != 0 && p->tuning.decide_threads != 256 && p->tuning.decide_threads != 512)
        return fail(DQMC_EINVAL, "tuning.decide_threads must be 0, 256 or 512");
    {   // the field also carries DQMC_TUNING_NO_RNG_LOOKAHEAD
        const int path = p->tuning.bmult_path & ~DQMC_TUNING_NO_RNG_LOOKAHEAD;
        if (p->tuning.bmult_path < 0 || path > 2) return fail(DQMC_EINVAL, "tuning.bmult_path must be 0, 1 or 2");
    }
    if (p->stabilisation != DQMC_STAB_SVD && p->stabilisation != DQMC_STAB_QR) return fail(DQMC_EINVAL, "stabilisation");
    if (!(p->dtau > 0)) return fail(DQMC_EINVAL, "dtau");
    if (p->model != DQMC_MODEL_SDW && p->model != DQMC_MODEL_HUBBARD) return fail(DQMC_EINVAL, "model");
    if (p->model == DQMC_MODEL_HUBBARD) {
        if (p->opdim != 1 || p->weakZflux || p->bc != DQMC_BC_PBC || p->delaySteps != 1)
            return fail(DQMC_EINVAL, "Hubbard replica: opdim must be 1, delaySteps 1, bc pbc, no flux");   // dethubbardparams.cpp:41-43
        if (!(p->u >= 0)) return fail(DQMC_EINVAL, "Hubbard replica: U must be >= 0 (alpha = acosh(e^{dtau U / 2}))");
        if (p->cdwU != 0.0) return fail(DQMC_EINVAL, "Hubbard replica: cdwU must be 0");
    }
    const int ng = MSF * N;
    if (p->stabilisation == DQMC_STAB_SVD && ng > 2304) return fail(DQMC_EINVAL, "n_g > 2304 not supported by the Jacobi kernel instantiations");
    if (ng > 4096) return fail(DQMC_EINVAL, "n_g > 4096 not supported by the QR panel kernel instantiations");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DQMC_ENODEV, "no HIP device available");
    if (p->device < 0 || p->device >= ndev) return fail(DQMC_ENODEV, "device ordinal out of range");
    HIPCHK(hipSetDevice(p->device));

    dqmc_ctx* c = new dqmc_ctx();
    c->p = *p;
    c->nb = nchains;
    c->N = N; c->MSF = MSF; c->n_g = ng; c->m = p->m; c->s = p->s; c->D = p->delaySteps;
    c->n = (p->m + p->s - 1) / p->s;       // ceil(m/s), detmodel.h:518
    // every failure below leaves through ONE cleanup: the context, its stream and all device memory allocated so far
    const int rc = create_fill(c, p);
    if (rc != DQMC_OK) { dqmc_destroy(c); return rc; }
    *out = c;
    return DQMC_OK;
}

static int create_fill(dqmc_ctx* c, const dqmc_params* p) {
    const int N = c->N, MSF = c->MSF, ng = c->n_g;
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_win, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_flush, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_adv, hipEventDisableTiming));

    DevModel& hm = c->hm;
    memset(&hm, 0, sizeof(hm));
    hm.opdim = p->opdim; hm.MSF = MSF; hm.L = p->L; hm.N = N; hm.ng = ng; hm.m = p->m; hm.s = p->s; hm.n = c->n;
    hm.D = p->delaySteps; hm.P = N / 4; hm.phi2bosons = p->phi2bosons;
    // proposals per delayed-update block: twice the block depth (the step-size adaptation steers the acceptance to
    // accRatio = 0.5), never below it (dqmc_update_slice launches ceil(N / D) rounds); DQMC_PROPOSAL_BUDGET overrides, 0 = no limit.
    // Shallow blocks (woodbury / iterative: D = 1) gain nothing from it.
    hm.pbudget = p->delaySteps >= 8 ? 2 * p->delaySteps : 0;
    if (p->tuning.proposal_budget != 0) hm.pbudget = p->tuning.proposal_budget < 0 ? 0 : p->tuning.proposal_budget;
    if (hm.pbudget > 0 && hm.pbudget < p->delaySteps) hm.pbudget = p->delaySteps;
    hm.decide_nt = p->tuning.decide_threads;
    hm.bmult_path = p->tuning.bmult_path & ~DQMC_TUNING_NO_RNG_LOOKAHEAD;
#ifdef DQMC_DECIDE_TIMING
    hm.dbg = (getenv("DQMC_DECIDE_TIMING") && atoi(getenv("DQMC_DECIDE_TIMING"))) ? 8 : 0;   // phase timers of k_update_decide; never changes a result
#endif
    hm.dtau = p->dtau; hm.r = p->r; hm.c = p->c; hm.u = p->u; hm.lambda = p->lambda;
    hm.ov[0] = std::exp(p->dtau * p->mux); hm.ov[1] = std::exp(p->dtau * p->muy);
    hm.ovinv[0] = std::exp(-p->dtau * p->mux); hm.ovinv[1] = std::exp(-p->dtau * p->muy);

    std::vector<int> psites, neigh;
    std::vector<hc> pmats;
    std::vector<double> pabcd;
    build_tables(*p, psites, pmats, pabcd, neigh);
    std::vector<hc> pmats_h;
    std::vector<double> pabcd_h;
    { std::vector<int> ps2, nb2; build_tables(*p, ps2, pmats_h, pabcd_h, nb2, true); }
    int *d_psites, *d_neigh; cplx *d_pmats, *d_pmats_h; double *d_pabcd, *d_pabcd_h;
    int rc;
#define A_(x) if ((rc = (x))) return rc;
    A_(salloc(c, &d_psites, psites.size()));
    A_(salloc(c, &d_neigh, neigh.size()));
    A_(salloc(c, &d_pmats, pmats.size()));
    A_(salloc(c, &d_pabcd, pabcd.size()));
    HIPCHK(copy_sync(c, d_pabcd, pabcd.data(), pabcd.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(c, d_psites, psites.data(), psites.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(c, d_neigh, neigh.data(), neigh.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(c, d_pmats, pmats.data(), pmats.size() * sizeof(hc), hipMemcpyHostToDevice));
    A_(salloc(c, &d_pmats_h, pmats_h.size()));
    A_(salloc(c, &d_pabcd_h, pabcd_h.size()));
    HIPCHK(copy_sync(c, d_pmats_h, pmats_h.data(), pmats_h.size() * sizeof(hc), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(c, d_pabcd_h, pabcd_h.data(), pabcd_h.size() * sizeof(double), hipMemcpyHostToDevice));
    hm.psites = d_psites; hm.neigh = d_neigh; hm.pmats = d_pmats; hm.pabcd = d_pabcd; hm.pm_real = p->weakZflux ? 0 : 1;
    hm.pmats_h = d_pmats_h; hm.pabcd_h = d_pabcd_h;
    if (p->model == DQMC_MODEL_HUBBARD) {
        hm.hubbard = 1; hm.dense = 1;
        hm.ov[0] = hm.ov[1] = hm.ovinv[0] = hm.ovinv[1] = 1.0;
        const double alpha = std::acosh(std::exp(p->dtau * p->u * 0.5));              // dethubbard.cpp:55
        hm.hub_exp_alpha[0] = std::exp(alpha); hm.hub_exp_alpha[1] = std::exp(-alpha);
        c->hub_e_m2a = std::exp(-2.0 * alpha * 1.0); c->hub_e_p2a = std::exp(2.0 * alpha * 1.0);
        std::vector<hc> em, ep;
        build_hubbard_propK(*p, neigh, em, ep);
        const size_t nn = (size_t)ng * ng;
        A_(salloc(c, &c->propK[0], nn)); A_(salloc(c, &c->propK[1], nn)); A_(dalloc(c, &c->Tdense, nn));
        HIPCHK(copy_sync(c, c->propK[0], em.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
        HIPCHK(copy_sync(c, c->propK[1], ep.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
    } else if (p->cb_none) {
        hm.dense = 1;
        hm.ov[0] = hm.ov[1] = hm.ovinv[0] = hm.ovinv[1] = 1.0;     // mu is part of K in setupPropK
        std::vector<hc> em, ep;
        build_dense_propK(*p, neigh, MSF, em, ep);
        const size_t nn = (size_t)ng * ng;
        A_(salloc(c, &c->propK[0], nn)); A_(salloc(c, &c->propK[1], nn)); A_(dalloc(c, &c->Tdense, nn));
        HIPCHK(copy_sync(c, c->propK[0], em.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
        HIPCHK(copy_sync(c, c->propK[1], ep.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
        build_dense_propK(*p, neigh, MSF, em, ep, 0.5);           // propK_half, propK_half_inv (detsdwopdim.cpp:1282-1283)
        A_(salloc(c, &c->propKh[0], nn)); A_(salloc(c, &c->propKh[1], nn));
        HIPCHK(copy_sync(c, c->propKh[0], em.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
        HIPCHK(copy_sync(c, c->propKh[1], ep.data(), nn * sizeof(hc), hipMemcpyHostToDevice));
    }

    const size_t nphi = (size_t)(p->m + 1) * p->opdim * N, ncs = (size_t)(p->m + 1) * N;
    A_(dalloc(c, &c->phi, nphi)); A_(dalloc(c, &c->coshT, ncs)); A_(dalloc(c, &c->sinhT, ncs));
    A_(dalloc(c, &c->phi_bak, nphi)); A_(dalloc(c, &c->cosh_bak, ncs)); A_(dalloc(c, &c->sinh_bak, ncs));
    if (p->cdwU != 0.0) { A_(dalloc(c, &c->cdwl, ncs)); A_(dalloc(c, &c->cdwC, ncs)); A_(dalloc(c, &c->cdwS, ncs)); }

    const size_t n2 = (size_t)ng * ng;
    A_(dalloc(c, &c->G, n2)); A_(dalloc(c, &c->G_bak, n2));
    A_(dalloc(c, &c->sv, (size_t)ng)); A_(dalloc(c, &c->sv_bak, (size_t)ng));
    c->storage.resize(c->n + 1); c->storage_bak.resize(c->n + 1);
    for (int l = 0; l <= c->n; ++l) { A_(alloc_slot(c, c->storage[l])); A_(alloc_slot(c, c->storage_bak[l])); }
    A_(alloc_slot(c, c->spare)); A_(alloc_slot(c, c->tmpudv));
    A_(dalloc(c, &c->T1, n2)); A_(dalloc(c, &c->T2, n2)); A_(dalloc(c, &c->T3, n2)); A_(dalloc(c, &c->T4, n2));
    A_(dalloc(c, &c->sw.A, n2)); A_(dalloc(c, &c->sw.V, n2));
    A_(dalloc(c, &c->sw.norms, (size_t)ng)); A_(dalloc(c, &c->sw.rnorms, (size_t)ng)); A_(dalloc(c, &c->sw.flagT, 1)); A_(dalloc(c, &c->sw.rank, (size_t)ng));
    A_(salloc(c, &c->sw.flag, 1));        // residual of a Jacobi sweep: max over all chains
    HIPCHK(hipHostMalloc((void**)&c->sw.hflag, 2 * sizeof(unsigned long long), hipHostMallocMapped));
    c->sw.hflag[0] = 0; c->sw.hflag[1] = 0;
    HIPCHK(hipHostGetDevicePointer((void**)&c->sw.hslot_dev, c->sw.hflag, 0));
    A_(salloc(c, &c->sw.seqctr, 1));
    HIPCHK(hipMemsetAsync(c->sw.seqctr, 0, sizeof(unsigned long long), c->st));
    c->sw.host_seq = &c->jacobi_host_seq;
    c->sw.last_residual = &c->last_svd_residual;
    c->sw.sweep_graph = &c->jacobi_graph;
    {
        int bw = svd_block_cols(ng);
        int nblk = ng / bw;
        std::vector<int> rounds;
        build_tournament(nblk, rounds);
        int* d_rounds;
        A_(salloc(c, &d_rounds, rounds.size()));
        HIPCHK(copy_sync(c, d_rounds, rounds.data(), rounds.size() * sizeof(int), hipMemcpyHostToDevice));
        c->sw.rounds = d_rounds; c->sw.nrounds = nblk - 1; c->sw.nblk = nblk;
    }
    c->stab = p->stabilisation;
    // a sweep budget the Jacobi SVD cannot meet makes the "SVD failed" path (udv.h:77-88 in the reference) reachable
    if (p->tuning.max_jacobi_sweeps > 0) c->max_jacobi_sweeps = p->tuning.max_jacobi_sweeps;
    // n_g > 1024: block Gram-Schmidt + Cholesky-QR2 on the GEMM kernel instead of 144 tall Householder panels (kernels_qr.hip)
    c->qr_bgs = p->tuning.qr_variant == 2 || (p->tuning.qr_variant == 0 && ng > 1024);
    c->green_lu = ng <= 512 && p->tuning.green_variant != 1;
    if (c->stab == DQMC_STAB_QR) A_(alloc_qr_work(c));
    A_(alloc_slot(c, c->eye));
    const int WD = MSF * c->D;
    const int WD8 = (WD + 7) & ~7;          // X and GrT are zero padded to a multiple of 8 columns for the flush kernel
    A_(dalloc(c, &c->X, (size_t)ng * WD8)); A_(dalloc(c, &c->Gr, (size_t)WD8 * ng)); A_(dalloc(c, &c->W, (size_t)WD * WD));
    {   // Pipelined updates (see dqmc_update_slice) need a bounded proposal window (pbudget) small enough for a compact copy.
        // Measured on MI355X (round 3): at the headline size the decisions of block b + 1 do overlap the flush of block b (88 % of
        // their time), but the flush slows down next to them (165 -> 215 us), the window kernel and two cross-stream waits per block
        // add ~ 35 us, and the next gather still waits for the flush: no gain per sweep for one context (213 vs 216 sweeps/s), a loss
        // for four overlapping contexts (250 vs 285) and for a single chain (5.6 vs 6.2).  Where it pays: n_g = 2304 (config 5), where
        // the flush is three quarters of an HBM-bound block -- 8 chains in one context 1.29 -> 1.40 sweeps/s, in two contexts 1.47 ->
        // 1.56.  So automatic means n_g > 1024 with at least two chains; the decision is latched HERE, from the parameters alone
        // (callers that drive many contexts at once pass pipeline = -1, host/detsdw.cpp).
        const int want = p->tuning.pipeline;
        const bool on = want > 0 || (want == 0 && ng > 1024 && c->nb >= 2);
        if (on && p->model == DQMC_MODEL_SDW && hm.pbudget > 0 && MSF * hm.pbudget <= 512) {
            c->pipelined = true;
            c->pipe_P = hm.pbudget;
            // one spare column: the decision kernel's look-ahead never fetches past the window (kernels_update.hip), the spare column
            // keeps even a stray address inside this buffer
            A_(dalloc(c, &c->Gwin, (size_t)MSF * hm.pbudget * (MSF * hm.pbudget + 1)));
        }
    }
    if (p->rng_window_per_site < 0 || p->rng_window_per_site > 4096) return fail(DQMC_EINVAL, "rng_window_per_site");
    c->uni_cap = (size_t)(p->rng_window_per_site > 0 ? p->rng_window_per_site : (p->opdim + 1 + (p->cdwU != 0.0 ? 2 : 0))) * N * p->m + 64;     // one sweep's worst case (+ the cdwl pass)
    A_(dalloc(c, &c->uniforms, c->uni_cap));
    if (!(p->tuning.bmult_path & DQMC_TUNING_NO_RNG_LOOKAHEAD)) {       // the look-ahead's second window and tail (dqmc_advance_uniforms)
        A_(dalloc(c, &c->uniforms_next, c->uni_cap)); A_(dalloc(c, &c->uni_tail, c->uni_cap));
    }
    A_(dalloc(c, &c->us, 1));
    A_(dalloc(c, &c->scalar_out, 8));
    A_(salloc(c, &c->shift_buf, (size_t)c->nb * 3));
    auto acc_alloc = [c](int id, size_t count) { c->acc[id].n = count; return dalloc(c, &c->acc[id].p, count); };
    A_(acc_alloc(ACC_SLICE, measure_accum_doubles(N, p->L)));
    const bool hub_fine = p->model == DQMC_MODEL_HUBBARD && p->timedisplaced > 0 && (p->timedisplaced & DQMC_TD_HUB_EVERY_SLICE);
    const int td_level = p->timedisplaced & ~DQMC_TD_EVERY_SLICE & ~(hub_fine ? DQMC_TD_HUB_EVERY_SLICE : 0);
    if (p->timedisplaced < 0 || td_level > 2)
        return fail(DQMC_EINVAL, "timedisplaced must be 0, 1 or 2 (| DQMC_TD_EVERY_SLICE; DQMC_TD_HUB_EVERY_SLICE: Hubbard model only)");
    if ((p->timedisplaced & DQMC_TD_EVERY_SLICE) && !td_level) return fail(DQMC_EINVAL, "DQMC_TD_EVERY_SLICE needs timedisplaced >= 1");
    if (p->model == DQMC_MODEL_HUBBARD && (p->timedisplaced || p->td_particle_hole)) {
        // the one reservation of this model, behind every other buffer: the matrices of the time-displaced Green's functions with G(0),
        // the scratch of the correlators' prepare pass (ph_H: n_g^2 complex hold its 4 N^2 + 4 N doubles) and the block of
        // dqmc_hubbard_measure_timedisplaced; none of the SDW blocks
        if ((p->timedisplaced != 1 && p->timedisplaced != (1 | DQMC_TD_HUB_EVERY_SLICE)) || p->td_particle_hole != 1)
            return fail(DQMC_EINVAL, "Hubbard replica: timedisplaced = 1 (| DQMC_TD_HUB_EVERY_SLICE) with td_particle_hole = 1 is the only "
                                     "time-displaced reservation (every other value of the two fields: SDW model only)");
        if (hub_fine && c->n < 2) return fail(DQMC_EINVAL, "Hubbard replica: DQMC_TD_HUB_EVERY_SLICE needs s < m (n >= 2)");
        c->td_reserved = true;
        A_(dalloc(c, &c->GT0, n2)); A_(dalloc(c, &c->G0T, n2)); A_(dalloc(c, &c->td_W, n2));
        if (c->stab != DQMC_STAB_QR) { A_(alloc_qr_work(c)); A_(dalloc(c, &c->td_sv, (size_t)ng)); }
        A_(dalloc(c, &c->G00, n2)); A_(dalloc(c, &c->ph_H, n2));
        A_(acc_alloc(ACC_HUB_TD, hubbard_td_doubles(N, c->n)));
    } else if (td_level) {          // behind every other buffer: the layout of a context without them is unchanged
        if (p->model != DQMC_MODEL_SDW) return fail(DQMC_EINVAL, "timedisplaced: SDW model only");
        c->td_reserved = true;
        A_(dalloc(c, &c->GT0, n2)); A_(dalloc(c, &c->G0T, n2)); A_(dalloc(c, &c->td_W, n2));
        if (c->stab != DQMC_STAB_QR) { A_(alloc_qr_work(c)); A_(dalloc(c, &c->td_sv, (size_t)ng)); }
        A_(acc_alloc(ACC_TD, measure_td_doubles(p->L, c->n)));
        if (td_level == 2) A_(acc_alloc(ACC_TD_PAIR, measure_td_pair_doubles(N, c->n)));   // behind the block above: timedisplaced == 1 keeps its layout
    }
    const int ph_level = p->td_particle_hole & ~DQMC_TD_PH_BAND;
    const bool ph_band = p->td_particle_hole >= 0 && (p->td_particle_hole & DQMC_TD_PH_BAND);
    if (p->td_particle_hole < 0 || ph_level > 2) return fail(DQMC_EINVAL, "td_particle_hole must be 0, 1 or 2 (| DQMC_TD_PH_BAND)");
    if (ph_band && !ph_level) return fail(DQMC_EINVAL, "DQMC_TD_PH_BAND needs td_particle_hole >= 1");
    if (ph_level && p->model == DQMC_MODEL_SDW) {     // behind the blocks above: contexts without the flag are laid out as before
        if (!td_level) return fail(DQMC_EINVAL, "td_particle_hole needs timedisplaced >= 1");
        A_(dalloc(c, &c->G00, n2)); A_(dalloc(c, &c->ph_H, n2));
        A_(dalloc(c, &c->ph_ob, measure_td_ph_onebody_cplx(N)));
        A_(acc_alloc(ACC_TD_PH, measure_td_ph_doubles(N, c->n)));
    }
    if (ph_level == 2) {                    // behind the blocks above again: value 1 keeps its layout
        std::vector<hc> bt;
        build_bond_table(*p, neigh, MSF, bt);
        A_(salloc(c, &c->cur_bt, bt.size()));
        HIPCHK(copy_sync(c, c->cur_bt, bt.data(), bt.size() * sizeof(hc), hipMemcpyHostToDevice));
        A_(dalloc(c, &c->cur_ob, measure_td_current_onebody_cplx(N)));
        A_(acc_alloc(ACC_TD_CUR, measure_td_current_doubles(N, c->n)));
    }
    if (p->timedisplaced & DQMC_TD_EVERY_SLICE) {   // behind every block above: contexts without the flag are laid out as before
        c->td_fine = true;
        A_(dalloc(c, &c->fGT0, n2)); A_(dalloc(c, &c->fG0T, n2)); A_(dalloc(c, &c->fGTT, n2));
        const bool on[4] = {true, td_level == 2, ph_level >= 1, ph_level == 2};
        for (int ch = 0; ch < 4; ++ch)
            if (on[ch]) A_(acc_alloc(ACC_FINE0 + ch, (size_t)(p->m + 1) * (1 + measure_td_row_doubles(ch, N, p->L))));
    }
    if (ph_band) {                          // behind every buffer above: contexts without the flag are laid out as before
        A_(dalloc(c, &c->band_ob, measure_td_band_onebody_cplx(N)));
        A_(acc_alloc(ACC_TD_BAND, measure_td_band_doubles(N, c->n)));
        if (c->td_fine) A_(acc_alloc(ACC_FINE0 + 4, (size_t)(p->m + 1) * (1 + measure_td_row_doubles(4, N, p->L))));
    }
    if (hub_fine) {                         // behind every buffer above: a Hubbard context without the flag is laid out as before
        c->td_fine = true;
        A_(dalloc(c, &c->fGT0, n2)); A_(dalloc(c, &c->fG0T, n2)); A_(dalloc(c, &c->fGTT, n2));
        A_(acc_alloc(ACC_HUB_TD_FINE, hubbard_td_fine_doubles(N, p->m)));
    }
    A_(arena_commit(c));                    // from here on the per-chain pointers are real (chain 0) addresses, zero filled
#undef A_
    for (int id = 0; id < ACC_EQ; ++id) c->acc[id].stride = c->lc.cs;
    c->acc[ACC_HUB_TD].stride = c->lc.cs;
    c->acc[ACC_HUB_TD_FINE].stride = c->lc.cs;
    c->qw.err = &c->us->chol_fail;
    hm.phi = c->phi; hm.coshT = c->coshT; hm.sinhT = c->sinhT;
    if (p->cdwU != 0.0) {
        // cdwl_eta / cdwl_gamma (detsdwopdim.h:1209-1235), getCoshSinhTermCDWl (detsdwopdim.cpp:1138-1143)
        hm.cdw_on = 1; hm.cdwl = c->cdwl; hm.cdwC = c->cdwC; hm.cdwS = c->cdwS;
        const double eta[2] = {std::sqrt(2. * (3. - std::sqrt(6.))), std::sqrt(2. * (3. + std::sqrt(6.)))};
        for (int a = 0; a < 2; ++a) {
            const double arg = std::sqrt(p->dtau) * p->cdwU * eta[a];
            hm.cdw_cosh[a] = std::cosh(arg); hm.cdw_sinh[a] = std::sinh(arg);
        }
        hm.cdw_gamma[0] = 3. + std::sqrt(6.); hm.cdw_gamma[1] = 3. - std::sqrt(6.);
    }
    DevUpdateState hus;
    memset(&hus, 0, sizeof(hus));
    hus.pub.phiDelta = 0.5;                 // AdjustmentData::InitialPhiDelta (detsdwopdim.h:489)
    hus.pub.angleDelta = 0.0; hus.pub.scaleDelta = 0.1;                      // InitialAngleDelta, InitialScaleDelta (:490-491)
    hus.pub.curminAngleDelta = -1.0; hus.pub.curmaxAngleDelta = 1.0;         // Min / MaxAngleDelta (:494-495)
    hus.pub.curminScaleDelta = 0.0; hus.pub.curmaxScaleDelta = 1.0;          // Min / MaxScaleDelta (:492-493)
    hus.pub.targetAccRatio = p->accRatio;
    hus.slice_done = 1;
    hus.r = p->r;
    for (int b = 0; b < c->nb; ++b) HIPCHK(copy_sync(c, chainp(c, c->us, b), &hus, sizeof(hus), hipMemcpyHostToDevice));
    { int rc2 = set_slot_identity(c, c->eye); if (rc2) return rc2; }
    if (c->hm.cdw_on) {                      // l = +1 everywhere (setupConstantField, detsdwopdim.cpp:1116-1128) until the host sets the field
        std::vector<double> ones((size_t)(c->m + 1) * N, 1.0);
        for (int b = 0; b < c->nb; ++b) HIPCHK(copy_sync(c, chainp(c, c->cdwl, b), ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
        launch_cdw_terms(c->lc, c->hm);
    }
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}

void series_free(dqmc_ctx* c) {
    dqmc_ctx::Series& s = c->ser;
    for (double* q : {s.sample, s.openbin, s.bins, s.bad, s.trig, s.stat, s.var, s.binning, s.vertex}) if (q) (void)hipFree(q);
    if (s.srctab) (void)hipFree((void*)s.srctab);
    if (s.vertex_tab) (void)hipFree(s.vertex_tab);
    if (s.ph_tab) (void)hipFree(s.ph_tab);
    s = dqmc_ctx::Series{};
}

static void green_check_free(dqmc_ctx* c);                 // the buffers of dqmc_set_green_check (below, next to dqmc_advance)
extern "C" void dqmc_destroy(dqmc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (c->st) (void)hipStreamSynchronize(c->st);
    for (void* q : c->allocs) (void)hipFree(q);
    if (c->mats_out) (void)hipFree(c->mats_out);
    custom_free(c);
    custom_pair_free(c);
    green_matrix_free(c);
    green_check_free(c);
    series_free(c);
    if (c->jacobi_graph) (void)hipGraphExecDestroy(c->jacobi_graph);
    if (c->sw.hflag) (void)hipHostFree(c->sw.hflag);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev_win) (void)hipEventDestroy(c->ev_win);
    if (c->ev_flush) (void)hipEventDestroy(c->ev_flush);
    if (c->st_up) (void)hipStreamSynchronize(c->st_up);
    if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
    if (c->ev_adv) (void)hipEventDestroy(c->ev_adv);
    if (c->uni_pin) (void)hipHostFree(c->uni_pin);
    if (c->st_up && c->st_up != c->st2) (void)hipStreamDestroy(c->st_up);
    if (c->st2) (void)hipStreamDestroy(c->st2);
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

extern "C" int dqmc_synchronize(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" void* dqmc_stream(dqmc_ctx* c) { return c ? (void*)c->st : nullptr; }
extern "C" int dqmc_num_chains(dqmc_ctx* c) { return c ? c->nb : 0; }
extern "C" int dqmc_select_chain(dqmc_ctx* c, int chain) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (chain < 0 || chain >= c->nb) return fail(DQMC_EINVAL, "chain index out of range");
    c->sel = chain;
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// fields
// ---------------------------------------------------------------------------------------------
extern "C" int dqmc_set_fields_host(dqmc_ctx* c, const double* phi) {
    if (!c || !phi) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t nphi = (size_t)(c->m + 1) * c->p.opdim * c->N;
    HIPCHK(hipMemcpyAsync(selp(c, c->phi), phi, nphi * sizeof(double), hipMemcpyHostToDevice, c->st));
    { ProfScope ps(c, FAM_OTHER, 1); launch_cosh_sinh(c->lc, c->hm); }
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" int dqmc_get_fields_host(dqmc_ctx* c, double* phi, double* coshT, double* sinhT) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    const size_t nphi = (size_t)(c->m + 1) * c->p.opdim * c->N, ncs = (size_t)(c->m + 1) * c->N;
    HIPCHK(hipStreamSynchronize(c->st));
    if (phi) HIPCHK(copy_sync(c, phi, selp(c, c->phi), nphi * sizeof(double), hipMemcpyDeviceToHost));
    if (coshT) HIPCHK(copy_sync(c, coshT, selp(c, c->coshT), ncs * sizeof(double), hipMemcpyDeviceToHost));
    if (sinhT) HIPCHK(copy_sync(c, sinhT, selp(c, c->sinhT), ncs * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}

// the discrete field of the selected chain, l_i(tau_k) in {+-1, +-2}: cdwl[k * N + site], slice 0 unused (cdwU != 0 only)
extern "C" int dqmc_set_cdwl_host(dqmc_ctx* c, const int32_t* cdwl) {
    if (!c || !cdwl) return fail(DQMC_EINVAL, "null argument");
    if (!c->hm.cdw_on) return fail(DQMC_EINVAL, "dqmc_set_cdwl_host: the context was created with cdwU == 0");
    (void)hipSetDevice(c->p.device);
    const size_t ncs = (size_t)(c->m + 1) * c->N;
    std::vector<double> v(ncs);
    for (size_t i = 0; i < ncs; ++i) {
        const int32_t l = cdwl[i];
        if (i >= (size_t)c->N && l != 1 && l != -1 && l != 2 && l != -2) return fail(DQMC_EINVAL, "cdwl values must be +-1 or +-2");
        v[i] = (double)l;
    }
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, selp(c, c->cdwl), v.data(), ncs * sizeof(double), hipMemcpyHostToDevice));
    { ProfScope ps(c, FAM_OTHER, 1); launch_cdw_terms(c->lc, c->hm); }
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" int dqmc_get_cdwl_host(dqmc_ctx* c, int32_t* cdwl) {
    if (!c || !cdwl) return fail(DQMC_EINVAL, "null argument");
    if (!c->hm.cdw_on) return fail(DQMC_EINVAL, "dqmc_get_cdwl_host: the context was created with cdwU == 0");
    (void)hipSetDevice(c->p.device);
    const size_t ncs = (size_t)(c->m + 1) * c->N;
    std::vector<double> v(ncs);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, v.data(), selp(c, c->cdwl), ncs * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ncs; ++i) cdwl[i] = (int32_t)v[i];
    return DQMC_OK;
}

// all chains in one strided transfer each way: phi_all = nchains cubes of (m+1) * opdim * N doubles, back to back
extern "C" int dqmc_set_fields_all_host(dqmc_ctx* c, const double* phi_all) {
    if (!c || !phi_all) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t bytes = (size_t)(c->m + 1) * c->p.opdim * c->N * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(c->phi, c->lc.cs, phi_all, bytes, bytes, (size_t)c->nb, hipMemcpyHostToDevice, c->st));
    { ProfScope ps(c, FAM_OTHER, 1); launch_cosh_sinh(c->lc, c->hm); }
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" int dqmc_get_fields_all_host(dqmc_ctx* c, double* phi_all) {
    if (!c || !phi_all) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t bytes = (size_t)(c->m + 1) * c->p.opdim * c->N * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(phi_all, bytes, c->phi, c->lc.cs, bytes, (size_t)c->nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// device-side building blocks
// ---------------------------------------------------------------------------------------------
// C = op(A) op(B) with n_g x n_g operands; callers set the options (negate, accumulate, scales, sharedA / sharedB, ...) by name
GemmArgs gemm_square(dqmc_ctx* c, const cplx* A, int opA, const cplx* B, int opB, cplx* C) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = c->n_g; g.opA = opA; g.B = B; g.ldb = c->n_g; g.opB = opB; g.C = C; g.ldc = c->n_g;
    g.M = g.N = g.K = c->n_g; g.Kmul = 1;
    return g;
}
// every n_g^3 product of the model goes through here: flop accounting (a lower triangular op(B) takes half the multiply-adds) and timing
void run_gemm(dqmc_ctx* c, const GemmArgs& g) {
    c->gemm_flops += (g.b_lower ? 4.0 : 8.0) * (double)g.M * g.N * g.K * c->nb;
    ProfScope ps(c, FAM_GEMM, 1);
    launch_gemm(c->lc, g);
}

// chain order of checkerboard{Left,Right}MultiplyBmat[Inv] (detsdwopdim.cpp:2076-2090, 2172-2186,
// 2307-2324, 2406-2420)
// src != nullptr: out of place, A = (chain) src -- the first pass of the checkerboard kernel reads src instead of A, the copy in front
// of an in-place multiply never happens.  (An empty chain and the dense propagator copy.)
void bmult_dev(dqmc_ctx* c, int side, int inverse, int k2, int k1, cplx* A, const cplx* src) {
    const int count = k2 - k1;
    if (src && (count <= 0 || c->hm.dense)) { launch_copy(c->lc, src, A, (size_t)c->n_g * c->n_g); src = nullptr; }
    if (count <= 0) return;
    bool ascending = (side == DQMC_LEFT) ? !inverse : (bool)inverse;
    int kfirst = ascending ? k1 + 1 : k2, kstep = ascending ? 1 : -1;
    if (!c->hm.dense) {
        ProfScope ps(c, FAM_BMULT, 1);
        launch_bmult(c->lc, nullptr, c->hm, side, inverse, kfirst, kstep, count, A, c->n_g, 0, src);
        return;
    }
    // CB_NONE (sdw*MultiplyBmat[Inv] functors with CBM == CB_NONE, detsdwopdim.h:1305-1375): per slice
    // B_k = e^{-dtau V_k} propK, B_k^{-1} = propK^{-1} e^{+dtau V_k}; propK^{-+1} is one MFMA GEMM with the
    // block-diagonal dense matrix, e^{-+dtau V_k} the site-local mix of the chain kernel.  The reference
    // inverts the chain product numerically (arma::inv); the exact factor-wise inverse used here agrees
    // with it to rounding.
    const bool hop_first = ((side == DQMC_RIGHT) == (bool)inverse);   // left B, right B^-1
    const cplx* PK = c->propK[inverse ? 1 : 0];
    const size_t n2 = (size_t)c->n_g * c->n_g;
    for (int i = 0; i < count; ++i) {
        const int k = kfirst + i * kstep;
        auto hop = [&]() {
            GemmArgs g = (side == DQMC_LEFT) ? gemm_square(c, PK, 0, A, 0, c->Tdense) : gemm_square(c, A, 0, PK, 0, c->Tdense);
            g.sharedA = (side == DQMC_LEFT); g.sharedB = !g.sharedA;
            run_gemm(c, g);
            launch_copy(c->lc, c->Tdense, A, n2);
        };
        if (hop_first) hop();
        {
            ProfScope ps(c, FAM_BMULT, 1);
            if (c->hm.hubbard) launch_hubbard_vscale(c->lc, c->hm, side, inverse, k, A, c->n_g);     // diag(e^{+-alpha s_k}) per spin block
            else launch_bmult(c->lc, nullptr, c->hm, side, inverse, k, kstep, 1, A, c->n_g);
        }
        if (!hop_first) hop();
    }
}

// udvDecompose (udv.h:68-102) of diag(rowscale) M diag(colscale)
static void svd_prof_begin(void* u) {
    dqmc_ctx* c = (dqmc_ctx*)u;
    c->ev_open.push_back({FAM_ROUNDS, prof_event_pair(c, c->st)});
}
static void svd_prof_end(void* u, int launches) {
    dqmc_ctx* c = (dqmc_ctx*)u;
    (void)hipEventRecord(c->ev_pool[c->ev_open.back().second + 1], c->st);
    c->fam_launches[FAM_ROUNDS] += launches;
    c->fam_launches[FAM_JACOBI] += launches;
}
// QR mode: the FAM_ROUNDS slot times the k_qr_apply launches (the launch count of the family is kept by run_qr's caller)
static void qr_apply_prof_end(void* u, int launches) {
    dqmc_ctx* c = (dqmc_ctx*)u;
    (void)hipEventRecord(c->ev_pool[c->ev_open.back().second + 1], c->st);
    c->fam_launches[FAM_ROUNDS] += launches;
}
static int udv_dev(dqmc_ctx* c, const cplx* M, const double* colscale, const double* rowscale, UdVSlot out) {
    SvdProfHooks hooks{svd_prof_begin, svd_prof_end, c};
    int sweeps = run_svd(c->lc, c->n_g, M, c->n_g, colscale, rowscale, out.U, out.d, out.Vt, c->sw, c->max_jacobi_sweeps,
                         c->prof ? &hooks : nullptr);
    if (!c->prof && sweeps > 0) c->fam_launches[FAM_JACOBI] += (uint64_t)sweeps * c->sw.nrounds;
    if (sweeps == DQMC_ENOCONV) return fail(DQMC_ENOCONV, "SVD failed (Jacobi did not converge)");
    if (sweeps < 0) return fail(sweeps, std::string("SVD failed: ") + hipGetErrorString(hipGetLastError()));
    c->last_svd_sweeps = sweeps;
    c->svd_calls += 1; c->svd_sweeps_total += sweeps;
    if (sweeps > c->svd_sweeps_max) c->svd_sweeps_max = sweeps;
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// QR ("UDT") stabilisation mode.  Chain factors keep the reference's convention M = U diag(d) V_t^H:
//   R-type (chains built upwards, B(tau,0)):   Ms P = Q R   ->  U = Q (unitary), V_t = (D^-1 R P^T)^H
//   L-type (chains built downwards, B(beta,tau), row graded): the same on Ms^H with the roles swapped
//           ->  V_t = Q (unitary), U = (D^-1 R P^T)^H
// so in  G = [1 + U_r d_r V_r^H U_l d_l V_l^H]^-1 = V_l [U_r^H V_l + d_r (V_r^H U_l) d_l]^-1 U_r^H
// exactly the two factors that must be unitary (U_r, V_l) are (cf. detmodel.h:762-767).
// ---------------------------------------------------------------------------------------------
enum { KIND_R = 0, KIND_L = 1 };

// Did a Cholesky-QR panel of the factorisation just enqueued fail its pivot test in any chain (k_chol64 sets DevUpdateState::chol_fail)?
// Waits for the stream; clears the flags.
static int chol_failed(dqmc_ctx* c, int* failed) {
    c->err_host.assign((size_t)c->nb, 0);
    int* flag = &c->us->chol_fail;
    HIPCHK(hipMemcpy2DAsync(c->err_host.data(), sizeof(int), flag, c->lc.cs, sizeof(int), (size_t)c->nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    *failed = 0;
    for (int b = 0; b < c->nb; ++b) if (c->err_host[b]) *failed = 1;
    if (*failed) HIPCHK(hipMemset2DAsync(flag, c->lc.cs, 0, sizeof(int), (size_t)c->nb, c->st));
    return DQMC_OK;
}

// Pivoted QR of M' = diag(rs) M diag(cs) (of its adjoint if transpose), M' P = Q R: the columns are ranked by their norms (qr_perm = P)
// and R is left in sw.A.  qr_bgs (n > 1024): block Gram-Schmidt + Cholesky-QR2 on the GEMM kernel instead of 144 tall Householder panels
// (kernels_qr.hip); it holds on the graded B-chains of udt_dev and on the scale-split sum Z of green_qr (entries O(1)) alike.  A panel
// too ill conditioned for Cholesky-QR (pivot test in k_chol64) is not an error: the factorisation is redone right here with the
// unconditionally stable Householder panels, for all chains of the context (one stream synchronisation per factorisation, which at
// these sizes takes tens of milliseconds).
// Qdst: where an explicit Q goes.  form_q: the Householder panels form Q there as well; without it they leave Q in reflector form in
// the QR workspace (run_qr_apply_q), so a caller that can live with either learns from q_explicit which one it got.
struct QrOutcome { int launches; bool q_explicit; };
static int qr_factorise(dqmc_ctx* c, const cplx* M, const double* cs, const double* rs, int transpose, cplx* Qdst, bool form_q, QrOutcome* out) {
    const int n = c->n_g;
    launch_scaled_norms_rank(c->lc, M, n, cs, rs, transpose, n, c->sw.norms, c->qr_perm, c->sw.rnorms);
    launch_udt_init(c->lc, M, n, cs, rs, c->qr_perm, transpose, c->sw.A, n);
    int launches = 3;                                   // norms, ranks, init
    bool bgs = c->qr_bgs;
    if (bgs) {
        launches += run_qr_bgs(c->lc, n, c->sw.A, Qdst, c->qw);
        int failed = 0;
        { int rc = chol_failed(c, &failed); if (rc) return rc; }
        if (failed) {
            c->cholqr_fallbacks += 1;
            bgs = false;
            qr_reset_workspace(c->lc, n, c->qw);
            launch_udt_init(c->lc, M, n, cs, rs, c->qr_perm, transpose, c->sw.A, n);
            launches += 3;                              // two fills, init
        }
    }
    if (!bgs) launches += run_qr(c->lc, n, c->sw.A, form_q ? Qdst : nullptr, c->qw);
    c->qr_calls += 1;
    *out = QrOutcome{launches, bgs || form_q};
    return DQMC_OK;
}

// lazy != 0: the non-unitary factor T^H = (D^-1 R P^T)^H is not formed; R stays in sw.A, 1/d and the inverse permutation
// go to qr_dinv / qr_perm_inv for the triangular chaining product of decompose_chained
static int udt_dev(dqmc_ctx* c, const cplx* M, const double* colscale, const double* rowscale, int kind, UdVSlot out, int lazy = 0) {
    const int n = c->n_g;
    const int transpose = (kind == KIND_L);
    ProfScope ps(c, FAM_JACOBI, 0);
    cplx* Q = transpose ? out.Vt : out.U;
    cplx* Tt = transpose ? out.U : out.Vt;
    QrOutcome qr;
    { int rc = qr_factorise(c, M, colscale, rowscale, transpose, Q, true, &qr); if (rc) return rc; }
    launch_udt_diag(c->lc, c->sw.A, n, out.d);
    if (lazy) launch_udt_lazy(c->lc, out.d, c->qr_perm, n, c->qr_dinv, c->qr_perm_inv);
    else launch_udt_tmat(c->lc, c->sw.A, out.d, c->qr_perm, n, Tt);
    c->fam_launches[FAM_JACOBI] += qr.launches + 2;     // + diag, lazy / tmat
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// G, the time-displaced pair and G(0) of one boundary from one factorisation of the scale-split matrix
//   Z = Drmax^-1 (U_r^H V_l) Dlmax^-1 + Drmin (V_r^H U_l) Dlmin
// (the scales of the L-type and the R-type factorisation split into their parts > 1 and <= 1, so that Z has entries O(1)).  Each of
// the four matrices is a left bracket {V_l Dlmax^-1, U_l Dlmin} and a right bracket {Drmax^-1 U_r^H, Drmin V_r^H} around Z^-1
// (dqmc_hip.h; no unitarity of the graded factors is assumed):
//   G        =  [V_l Dlmax^-1] Z^-1 [Drmax^-1 U_r^H] =  A_max B_max
//   G(tau,0) =  [V_l Dlmax^-1] Z^-1 [Drmin V_r^H]    =  A_max B_min
//   G(0,tau) = -[U_l Dlmin]    Z^-1 [Drmax^-1 U_r^H] = -A_min B_max
//   1 - G(0) =  [U_l Dlmin]    Z^-1 [Drmin V_r^H]    =  A_min B_min        (G(0) of the boundary's own field configuration)
// where every half takes one factor of Z^-1 along: A = left_half(left bracket), B = right_half(right bracket).  So each matrix beyond
// G costs one more triangular solve or Q application and one GEMM.  Per route of the factorisation (ZFactors):
//   LU          P Z = L U, L \ U in T2 (n_g <= 512)   A = X U^-1      B = L^-1 P Y, kept as its adjoint (Y^H P^T) L^-H (two right-hand
//                                                                     triangular solves; the products take it with opB = 1)
//   reflectors  Z P = Q R, R in sw.A                  A = X P R^-1    B = Q^H Y, Q applied from the QR workspace and never formed
//   explicit Q  Z P = Q R, R in sw.A, Q in T4         A = X P R^-1    B = Q^H Y by GEMM, Y staged in a scratch matrix first
// (dqmc_tuning::green_variant = 1 keeps a QR route where LU would do; Q is explicit when block Gram-Schmidt made it.)
// Buffers:  A_max -> T3 and B_max -> T1: scratch of the chain step before, dead once that was decomposed.
//           B_min -> T4 on the LU route: T2 still holds L \ U, and no Q lives in T4.
//           B_min -> T2 on the QR routes: the factorisation worked on a copy of Z in sw.A (also when it fell back and copied it
//                    again), so T2 is free from there on, and T4 may hold Q.
//           A_min -> td_W, the only buffer of its own the pair has.  The explicit-Q route stages Y in sw.V for B_max (Jacobi
//                    workspace: idle in QR mode, done with in SVD mode) and in td_W for B_min -- so B_min comes before A_min.
// The helpers return the launches they made in the decomposition family; their GEMMs count themselves (run_gemm).
// ---------------------------------------------------------------------------------------------
enum ZRoute { Z_LU, Z_QR_REFLECTORS, Z_QR_EXPLICIT };
struct ZFactors {
    ZRoute route;
    const cplx* tri;        // the triangular factor(s): T2 = L \ U, or sw.A = R
    const cplx* Q;          // T4 on the explicit-Q route, else nullptr
    int adjoint;            // the right halves are stored as their adjoints: opB of every product A B
};
// factorises Z (in T2) and writes the log-det vector: |det Z| = prod |U_kk| = prod |R_kk|
static int factorise_z(dqmc_ctx* c, double* svout, ZFactors* z, int* launches) {
    const int n = c->n_g;
    ProfScope ps(c, FAM_JACOBI, 0);
    if (c->green_lu) {
        *launches = run_lu(c->lc, n, c->T2, c->qr_perm, c->lu_swaps, c->lu_tneg);      // T2 = L \ U, qr_perm = row permutation
        c->lu_calls += 1;
        *z = ZFactors{Z_LU, c->T2, nullptr, 1};
    } else {
        QrOutcome qr;
        { int rc = qr_factorise(c, c->T2, nullptr, nullptr, 0, c->T4, false, &qr); if (rc) return rc; }
        *launches = qr.launches;
        *z = ZFactors{qr.q_explicit ? Z_QR_EXPLICIT : Z_QR_REFLECTORS, c->sw.A, qr.q_explicit ? c->T4 : nullptr, 0};
    }
    launch_logdet_vector(c->lc, z->tri, c->rmax_inv, c->lmax_inv, n, svout);
    *launches += 1;
    return DQMC_OK;
}
// dst = (X diag(scale)) U^-1 (LU)  or  (X diag(scale)) P R^-1 (QR routes)
static int left_half(dqmc_ctx* c, const ZFactors& z, const cplx* X, const double* scale, cplx* dst) {
    ProfScope ps(c, FAM_JACOBI, 0);
    if (z.route == Z_LU) {
        // no column permutation: the solve reads X diag(scale) where it lies (first touch of dst), the scaled copy in front of it is gone
        const ColSrc src = {X, c->n_g, nullptr, scale};
        return run_trsm_right_upper(c->lc, c->n_g, z.tri, dst, c->qw, 0, 0, &src);
    }
    // QR routes: the scatter dst[:, perm[j]] = X[:, j] scale[j] stays a pass of its own (reading it in the solve needs the inverse permutation)
    launch_permute_scale_cols(c->lc, X, scale, c->qr_perm, c->n_g, dst);
    return 1 + run_trsm_right_upper(c->lc, c->n_g, z.tri, dst, c->qw);
}
// dst = [L^-1 P (diag(scale) Yh^H)]^H (LU)  or  Q^H (diag(scale) Yh^H) (QR routes); stage: scratch of the explicit-Q route
static int right_half(dqmc_ctx* c, const ZFactors& z, const cplx* Yh, const double* scale, cplx* dst, cplx* stage) {
    const int n = c->n_g;
    int launches = 1;
    {
        ProfScope ps(c, FAM_JACOBI, 0);
        if (z.route == Z_LU) {
            const ColSrc src = {Yh, n, c->qr_perm, scale};                                   // (Yh diag(scale)) P^T, read where it lies
            launches = run_trsm_right_upper(c->lc, n, z.tri, dst, c->qw, 1, 1, &src);        // dst <- ((Yh diag(scale)) P^T) L^-H
        } else if (z.route == Z_QR_REFLECTORS) {
            launch_udt_init(c->lc, Yh, n, scale, nullptr, nullptr, 1, dst, n);               // dst = diag(scale) Yh^H
            launches += run_qr_apply_q(c->lc, n, dst, c->qw, 1);                             // dst <- Q^H dst
        } else launch_udt_init(c->lc, Yh, n, scale, nullptr, nullptr, 1, stage, n);          // stage = diag(scale) Yh^H
    }
    if (z.route == Z_QR_EXPLICIT) run_gemm(c, gemm_square(c, z.Q, 1, stage, 0, dst));        // dst = Q^H stage
    return launches;
}

// Lp / Rp: the L-type / R-type factorisation (nullptr = identity).  Gout = nullptr: G itself is not formed (SVD mode builds only the
// time-displaced pair here); td: also G(tau,0), G(0,tau) and, with dqmc_params::td_particle_hole, G(0).
static int green_qr(dqmc_ctx* c, const UdVSlot* Lp, const UdVSlot* Rp, cplx* Gout, double* svout, bool td = false) {
    const UdVSlot& L = Lp ? *Lp : c->eye;
    const UdVSlot& R = Rp ? *Rp : c->eye;
    {
        ProfScope ps(c, FAM_OTHER, 2);
        launch_split_scales(c->lc, R.d, c->n_g, c->rmax_inv, c->rmin);
        launch_split_scales(c->lc, L.d, c->n_g, c->lmax_inv, c->lmin);
    }
    GemmArgs g = gemm_square(c, R.U, 1, L.Vt, 0, c->T2);
    g.rowscale = c->rmax_inv; g.colscale = c->lmax_inv;
    run_gemm(c, g);
    g = gemm_square(c, R.Vt, 1, L.U, 0, c->T2);
    g.rowscale = c->rmin; g.colscale = c->lmin; g.accumulate = 1;
    run_gemm(c, g);
    ZFactors z;
    int launches = 0;
    { int rc = factorise_z(c, svout, &z, &launches); if (rc) return rc; }
    launches += left_half(c, z, L.Vt, c->lmax_inv, c->T3);                                   // A_max
    launches += right_half(c, z, R.U, c->rmax_inv, c->T1, c->sw.V);                          // B_max
    if (Gout) run_gemm(c, gemm_square(c, c->T3, 0, c->T1, z.adjoint, Gout));
    if (td) {
        cplx* Bmin = z.route == Z_LU ? c->T4 : c->T2;
        launches += right_half(c, z, R.Vt, c->rmin, Bmin, c->td_W);
        launches += left_half(c, z, L.U, c->lmin, c->td_W);                                  // A_min
        run_gemm(c, gemm_square(c, c->T3, 0, Bmin, z.adjoint, c->GT0));
        g = gemm_square(c, c->td_W, 0, c->T1, z.adjoint, c->G0T);
        g.negate = 1;
        run_gemm(c, g);
        if (c->G00) {                                                                        // G(0) = 1 - A_min B_min (eye.d holds ones)
            g = gemm_square(c, c->td_W, 0, Bmin, z.adjoint, c->G00);
            g.negate = 1;
            run_gemm(c, g);
            ProfScope ps(c, FAM_OTHER, 1);
            launch_add_diag(c->lc, c->G00, c->eye.d, c->n_g);
        }
    }
    c->fam_launches[FAM_JACOBI] += launches;
    return DQMC_OK;
}

// mode dispatch --------------------------------------------------------------------------------
static int udv_dev(dqmc_ctx* c, const cplx* M, const double* colscale, const double* rowscale, UdVSlot out);
static int decompose(dqmc_ctx* c, const cplx* M, const double* colscale, const double* rowscale, int kind, UdVSlot out) {
    if (c->stab == DQMC_STAB_QR) return udt_dev(c, M, colscale, rowscale, kind, out);
    return udv_dev(c, M, colscale, rowscale, out);
}

// Decomposition of a chain step whose non-unitary factor is chained with the previous one (detmodel.h:987, :1143):
// out gets the unitary factor, the scales, and Aold * (new non-unitary factor).  QR mode: that factor is
// P R^H D^-1, so the product is a column gather of Aold times a LOWER TRIANGULAR matrix -- half the multiply-adds,
// and the factor itself is never written.
static int decompose_chained(dqmc_ctx* c, const cplx* M, const double* colscale, const double* rowscale, int kind, UdVSlot out,
                             const cplx* Aold) {
    cplx* dest = (kind == KIND_R) ? out.Vt : out.U;
    if (c->stab == DQMC_STAB_QR) {
        int rc = udt_dev(c, M, colscale, rowscale, kind, out, 1);
        if (rc) return rc;
        GemmArgs g = gemm_square(c, Aold, 0, c->sw.A, 1, dest);               // dest = Aold[:, P^-1] R^H D^-1
        g.a_kgather = c->qr_perm_inv; g.b_lower = 1; g.colscale = c->qr_dinv;
        run_gemm(c, g);
        return DQMC_OK;
    }
    UdVSlot t = out;
    if (kind == KIND_R) t.Vt = c->tmpudv.Vt; else t.U = c->tmpudv.U;
    int rc = decompose(c, M, colscale, rowscale, kind, t);
    if (rc) return rc;
    run_gemm(c, gemm_square(c, Aold, 0, (kind == KIND_R) ? c->tmpudv.Vt : c->tmpudv.U, 0, dest));
    return DQMC_OK;
}

// SVD mode: G = (Vl t.Vt) diag(1 / sv) (Ur t.U)^H from the SVD t of the matrix inside the inverse (t.d = sv)
static void green_from_svd(dqmc_ctx* c, const cplx* Vl, const cplx* Ur, const UdVSlot& t) {
    run_gemm(c, gemm_square(c, Vl, 0, t.Vt, 0, c->T3));                   // Vt_product
    run_gemm(c, gemm_square(c, Ur, 0, t.U, 0, c->T4));                    // U_product
    GemmArgs g = gemm_square(c, c->T3, 0, c->T4, 1, c->G);
    g.kscale = c->sv; g.kscale_invert = 1;
    run_gemm(c, g);
}
// greenFromUdV (detmodel.h:769-818)
// While the time-displaced functions are on, this is where they come from (every call is at an interior boundary).
static int green_from_udv(dqmc_ctx* c, const UdVSlot& L, const UdVSlot& R) {
    if (c->stab == DQMC_STAB_QR) return green_qr(c, &L, &R, c->G, c->sv, c->td_on);
    run_gemm(c, gemm_square(c, R.U, 1, L.Vt, 0, c->T2));                  // UtVt_rl = U_r^H V_t_l
    GemmArgs g = gemm_square(c, R.Vt, 1, L.U, 0, c->T2);                  // += diag(d_r) (V_t_r^H U_l) diag(d_l)
    g.rowscale = R.d; g.colscale = L.d; g.accumulate = 1;
    run_gemm(c, g);
    UdVSlot t = c->tmpudv; t.d = c->sv;
    int rc = udv_dev(c, c->T2, nullptr, nullptr, t);
    if (rc) return rc;
    green_from_svd(c, L.Vt, R.U, t);
    // SVD mode: G stays on the path above; the pair comes from the scale-split Z, built and factorised after G
    if (c->td_on) return green_qr(c, &L, &R, nullptr, c->td_sv, true);
    return DQMC_OK;
}
// greenFromEye_and_UdV (detmodel.h:823-860); kind tells whether the factorisation is R-type or L-type
static int green_from_eye(dqmc_ctx* c, const UdVSlot& R, int kind) {
    if (c->stab == DQMC_STAB_QR) return (kind == KIND_R) ? green_qr(c, nullptr, &R, c->G, c->sv) : green_qr(c, &R, nullptr, c->G, c->sv);
    run_gemm(c, gemm_square(c, R.U, 1, R.Vt, 0, c->T2));
    { ProfScope ps(c, FAM_OTHER, 1); launch_add_diag(c->lc, c->T2, R.d, c->n_g); }
    UdVSlot t = c->tmpudv; t.d = c->sv;
    int rc = udv_dev(c, c->T2, nullptr, nullptr, t);
    if (rc) return rc;
    green_from_svd(c, R.Vt, R.U, t);
    return DQMC_OK;
}

static int set_slot_identity(dqmc_ctx* c, UdVSlot& sl) {
    ProfScope ps(c, FAM_OTHER, 2);
    launch_set_identity(c->lc, sl.U, c->n_g);
    launch_set_identity(c->lc, sl.Vt, c->n_g);
    std::vector<double> ones(c->n_g, 1.0);
    for (int b = 0; b < c->nb; ++b)
        HIPCHK(hipMemcpyAsync(chainp(c, sl.d, b), ones.data(), c->n_g * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}

// setupUdVStorage_and_calculateGreen_skeleton (detmodel.h:680-713)
extern "C" int dqmc_udv_setup(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    HIPCHK(hipSetDevice(c->p.device));
    const int n = c->n, s = c->s, m = c->m, ng = c->n_g;
    int rc;
    if ((rc = set_slot_identity(c, c->storage[0]))) return rc;
    { ProfScope ps(c, FAM_OTHER, 1); launch_set_identity(c->lc, c->T1, ng); }
    bmult_dev(c, DQMC_LEFT, 0, s, 0, c->T1);
    if ((rc = decompose(c, c->T1, nullptr, nullptr, KIND_R, c->storage[1]))) return rc;
    for (int l = 1; l <= n - 1; ++l) {
        const int k_l = s * l, k_lp1 = (l < n - 1) ? s * (l + 1) : m;
        bmult_dev(c, DQMC_LEFT, 0, k_lp1, k_l, c->T1, c->storage[l].U);
        if ((rc = decompose_chained(c, c->T1, c->storage[l].d, nullptr, KIND_R, c->storage[l + 1], c->storage[l].Vt))) return rc;
    }
    if ((rc = green_from_eye(c, c->storage[n], KIND_R))) return rc;
    c->currentTimeslice = m;
    c->g_stale = false;
    return finish(c, "dqmc_udv_setup");
}

extern "C" int dqmc_reset_storage0(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    return set_slot_identity(c, c->storage[0]);
}

// ---------------------------------------------------------------------------------------------
// wrap-error diagnostics (dqmc_hip.h: dqmc_set_green_check; kernels_green_check.hip)
// ---------------------------------------------------------------------------------------------
static size_t green_check_doubles(const dqmc_ctx* c) { return (size_t)2 * (c->n + 1) * DQMC_GREEN_CHECK_FIELDS; }
static void green_check_free(dqmc_ctx* c) {
    for (void* q : {(void*)c->gc_keep, (void*)c->gc_part, (void*)c->gc_out, (void*)c->gc_table}) if (q) (void)hipFree(q);
    c->gc_keep = nullptr; c->gc_part = c->gc_out = c->gc_table = nullptr;
    c->gc_on = false;
}
extern "C" int dqmc_set_green_check(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if ((on != 0) == c->gc_on) return DQMC_OK;
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));                   // nothing enqueued still uses the buffers
    if (!on) { green_check_free(c); return DQMC_OK; }
    // the new buffers first: a failed allocation leaves the context as it was
    const size_t nb = (size_t)c->nb, n2 = (size_t)c->n_g * c->n_g, tab = green_check_doubles(c) * nb * sizeof(double);
    void *keep = nullptr, *part = nullptr, *out = nullptr, *table = nullptr;
    hipError_t e = hipMalloc(&keep, n2 * nb * sizeof(cplx));
    if (e == hipSuccess) e = hipMalloc(&part, green_diff_partial_doubles(c->n_g) * nb * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&out, 6 * nb * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&table, tab);
    if (e == hipSuccess) e = hipMemsetAsync(table, 0, tab, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) {
        for (void* q : {keep, part, out, table}) if (q) (void)hipFree(q);
        return fail(DQMC_EHIP, std::string("dqmc_set_green_check: ") + hipGetErrorString(e));
    }
    c->gc_keep = (cplx*)keep; c->gc_part = (double*)part; c->gc_out = (double*)out; c->gc_table = (double*)table;
    c->gc_on = true;
    return DQMC_OK;
}
extern "C" size_t dqmc_green_check_size(dqmc_ctx* c) { return c && c->gc_on ? green_check_doubles(c) : 0; }
extern "C" int dqmc_green_check_read_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (!c->gc_on) return fail(DQMC_EINVAL, "the wrap-error diagnostics are switched off (dqmc_set_green_check)");
    (void)hipSetDevice(c->p.device);
    HIPCHK(copy_sync(c, out, c->gc_table, green_check_doubles(c) * c->nb * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_green_check_reset(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->gc_on) return fail(DQMC_EINVAL, "the wrap-error diagnostics are switched off (dqmc_set_green_check)");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipMemsetAsync(c->gc_table, 0, green_check_doubles(c) * c->nb * sizeof(double), c->st));
    return finish(c, "dqmc_green_check_reset");
}
// the advance is about to rebuild G: keep the wrapped one
static void green_check_keep(dqmc_ctx* c) {
    ProfScope ps(c, FAM_OTHER, 1);
    const size_t n2 = (size_t)c->n_g * c->n_g;
    launch_green_keep(c->lc, c->G, c->gc_keep, n2 * sizeof(cplx), n2);
}
// ... and it has: one sample into row [dir][j]; stored: the factorisation the advance is about to put into storage[j]
static void green_check_sample(dqmc_ctx* c, int dir, int j, const UdVSlot& stored) {
    ProfScope ps(c, FAM_OTHER, 2);
    const size_t n2 = (size_t)c->n_g * c->n_g;
    const GreenCheckFold fold = {c->gc_table, green_check_doubles(c) * sizeof(double), (dir == DQMC_UP ? c->n + 1 : 0) + j, stored.d,
                                 c->stab == DQMC_STAB_SVD ? c->sv : nullptr};
    launch_green_diff(c->lc, c->gc_keep, n2 * sizeof(cplx), c->G, c->n_g, c->n_g, c->N, c->gc_part,
                      green_diff_partial_doubles(c->n_g) * sizeof(double), c->gc_out, 6 * sizeof(double), &fold);
}

// advanceDownGreen (detmodel.h:956-1017) / advanceUpGreen (detmodel.h:1109-1163)
extern "C" int dqmc_advance(dqmc_ctx* c, int dir, int l) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    HIPCHK(hipSetDevice(c->p.device));
    const int n = c->n, s = c->s, m = c->m, ng = c->n_g;
    int rc;
    if (dir == DQMC_DOWN) {
        if (l < 1 || l > n) return fail(DQMC_EINVAL, "advanceDown: l out of range");
        if (c->currentTimeslice != s * (l - 1)) return fail(DQMC_EINVAL, "advanceDown: currentTimeslice != s*(l-1)");
        const int k_l = (l < n) ? s * l : m, k_lm1 = s * (l - 1);
        const bool check = c->gc_on && !c->g_stale;      // the wrapped G exists: compare it with the rebuilt one
        if (check) green_check_keep(c);
        UdVSlot L = c->spare;
        if (l < n) {
            const UdVSlot& st = c->storage[l];
            { ProfScope ps(c, FAM_OTHER, 1); launch_conj_transpose(c->lc, st.Vt, c->T1, ng); }
            bmult_dev(c, DQMC_RIGHT, 0, k_l, k_lm1, c->T1);
            if ((rc = decompose_chained(c, c->T1, nullptr, st.d, KIND_L, L, st.U))) return rc;
        } else {
            { ProfScope ps(c, FAM_OTHER, 1); launch_set_identity(c->lc, c->T1, ng); }
            bmult_dev(c, DQMC_RIGHT, 0, k_l, k_lm1, c->T1);
            if ((rc = decompose(c, c->T1, nullptr, nullptr, KIND_L, L))) return rc;
        }
        if (l - 1 > 0) {
            rc = green_from_udv(c, L, c->storage[l - 1]);
            if (!rc && c->td_on) c->td_slice = s * (l - 1);
        } else rc = green_from_eye(c, L, KIND_L);
        if (rc) return rc;
        if (check) green_check_sample(c, dir, l - 1, L);
        std::swap(c->storage[l - 1], c->spare);          // storage[l-1] = UdV_L
        c->currentTimeslice = s * (l - 1);
        c->g_stale = false;
        return finish(c, "dqmc_advance");
    } else if (dir == DQMC_UP) {
        if (l < 0 || l > n - 1) return fail(DQMC_EINVAL, "advanceUp: l out of range");
        const int k_l = s * l, k_lp1 = (l < n - 1) ? s * (l + 1) : m;
        if (c->currentTimeslice != k_lp1) return fail(DQMC_EINVAL, "advanceUp: currentTimeslice != k_{l+1}");
        const bool check = c->gc_on && !c->g_stale;
        if (check) green_check_keep(c);
        const UdVSlot& st = c->storage[l];
        UdVSlot T = c->spare;
        bmult_dev(c, DQMC_LEFT, 0, k_lp1, k_l, c->T1, st.U);
        if ((rc = decompose_chained(c, c->T1, st.d, nullptr, KIND_R, T, st.Vt))) return rc;
        if (k_lp1 != m) {
            rc = green_from_udv(c, c->storage[l + 1], T);
            if (!rc && c->td_on) c->td_slice = k_lp1;
        } else rc = green_from_eye(c, T, KIND_R);
        if (rc) return rc;
        if (check) green_check_sample(c, dir, l + 1, T);
        std::swap(c->storage[l + 1], c->spare);
        c->currentTimeslice = k_lp1;
        c->g_stale = false;
        return finish(c, "dqmc_advance");
    }
    return fail(DQMC_EINVAL, "dir must be DQMC_UP or DQMC_DOWN");
}

// every entry that reads G refuses while dqmc_wrap_skip has left it stale

// wrapUpGreen / wrapDownGreen (detmodel.h:1236-1259, 1066-1095)
extern "C" int dqmc_wrap(dqmc_ctx* c, int dir, int k) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    G_FRESH(c, "wrap");
    if (c->currentTimeslice != k) return fail(DQMC_EINVAL, "wrap: currentTimeslice != k");
    if (dir == DQMC_UP) {
        if (k < 0 || k >= c->m) return fail(DQMC_EINVAL, "wrapUp: k out of range");
        bmult_dev(c, DQMC_RIGHT, 1, k + 1, k, c->G);
        bmult_dev(c, DQMC_LEFT, 0, k + 1, k, c->G);
        c->currentTimeslice = k + 1;
    } else if (dir == DQMC_DOWN) {
        if (k < 1 || k > c->m) return fail(DQMC_EINVAL, "wrapDown: k out of range");
        bmult_dev(c, DQMC_RIGHT, 0, k, k - 1, c->G);
        bmult_dev(c, DQMC_LEFT, 1, k, k - 1, c->G);
        c->currentTimeslice = k - 1;
    } else return fail(DQMC_EINVAL, "dir must be DQMC_UP or DQMC_DOWN");
    return finish(c, "dqmc_wrap");
}
// the checks and the bookkeeping of dqmc_wrap for a wrap whose G the following dqmc_advance overwrites: nothing is launched
extern "C" int dqmc_wrap_skip(dqmc_ctx* c, int dir, int k) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    G_FRESH(c, "wrap");
    if (c->currentTimeslice != k) return fail(DQMC_EINVAL, "wrap: currentTimeslice != k");
    if (dir == DQMC_UP) {
        if (k < 0 || k >= c->m) return fail(DQMC_EINVAL, "wrapUp: k out of range");
        c->currentTimeslice = k + 1;
    } else if (dir == DQMC_DOWN) {
        if (k < 1 || k > c->m) return fail(DQMC_EINVAL, "wrapDown: k out of range");
        c->currentTimeslice = k - 1;
    } else return fail(DQMC_EINVAL, "dir must be DQMC_UP or DQMC_DOWN");
    c->g_stale = true;
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// local updates
// ---------------------------------------------------------------------------------------------
extern "C" int dqmc_push_uniforms_host(dqmc_ctx* c, const double* u, size_t nvals) {
    if (!c || (!u && nvals)) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (nvals > c->uni_cap)
        return fail(DQMC_EINVAL, "more uniforms than the window holds (rng_window_per_site * N * m + 64; default per site: opdim + 1 [+ 2 with cdwU])");
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, selp(c, c->uniforms), u, nvals * sizeof(double), hipMemcpyHostToDevice));
    uint64_t vals[2] = {0, (uint64_t)nvals};
    HIPCHK(copy_sync(c, (char*)selp(c, c->us) + offsetof(DevUpdateState, pub) + offsetof(dqmc_update_state, rng_consumed), vals,
                     sizeof(vals), hipMemcpyHostToDevice));
    c->uni_n = c->nb == 1 ? nvals : 0;      // with more chains the windows may now differ in size: no look-ahead until all are pushed
    c->tail_staged = false;
    c->windows_pushed += 1;
    return DQMC_OK;
}

// all chains at once: u holds nchains windows of nvals uniforms each, back to back; ONE strided copy into the arena
extern "C" int dqmc_push_uniforms_all_host(dqmc_ctx* c, const double* u, size_t nvals) {
    if (!c || (!u && nvals)) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (nvals > c->uni_cap)
        return fail(DQMC_EINVAL, "more uniforms than the window holds (rng_window_per_site * N * m + 64; default per site: opdim + 1 [+ 2 with cdwU])");
    HIPCHK(hipMemcpy2DAsync(c->uniforms, c->lc.cs, u, nvals * sizeof(double), nvals * sizeof(double), (size_t)c->nb, hipMemcpyHostToDevice, c->st));
    std::vector<uint64_t> vals((size_t)2 * c->nb);
    for (int b = 0; b < c->nb; ++b) { vals[2 * b] = 0; vals[2 * b + 1] = (uint64_t)nvals; }
    HIPCHK(hipMemcpy2DAsync((char*)c->us + offsetof(DevUpdateState, pub) + offsetof(dqmc_update_state, rng_consumed), c->lc.cs, vals.data(),
                            2 * sizeof(uint64_t), 2 * sizeof(uint64_t), (size_t)c->nb, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->uni_n = nvals;
    c->tail_staged = false;
    c->windows_pushed += 1;
    return DQMC_OK;
}

// ---- look-ahead on the uniforms (include/dqmc_hip.h; schedule and ordering: DESIGN.md section 19) ----
// The staging buffer holds nb windows of uni_cap doubles and, behind them, the nb offsets the splice kernel reads straight from
// host memory.  The upload's stream is st2 where the update schedule leaves it idle, else a stream of its own.
static int lookahead_ready(dqmc_ctx* c) {
    if (!c->uniforms_next) return fail(DQMC_EINVAL, "the context was created without the look-ahead on the uniforms (DQMC_TUNING_NO_RNG_LOOKAHEAD)");
    if (c->uni_pin) return DQMC_OK;
    if (!c->st_up) {
        if (c->pipelined) HIPCHK(hipStreamCreateWithFlags(&c->st_up, hipStreamNonBlocking));
        else c->st_up = c->st2;
    }
    void* q = nullptr;
    HIPCHK(hipHostMalloc(&q, ((size_t)c->nb * c->uni_cap + (size_t)c->nb) * sizeof(double), hipHostMallocDefault));
    c->uni_pin = (double*)q;
    c->uni_off = (unsigned long long*)(c->uni_pin + (size_t)c->nb * c->uni_cap);
    return DQMC_OK;
}
extern "C" int dqmc_uniforms_staging_host(dqmc_ctx* c, double** buf, size_t* capacity) {
    if (!c || !buf) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (int rc = lookahead_ready(c)) return rc;
    if (c->tail_event_live) HIPCHK(hipEventSynchronize(c->ev_tail));       // an upload may still be reading the buffer
    *buf = c->uni_pin;
    if (capacity) *capacity = c->uni_cap;
    return DQMC_OK;
}
extern "C" int dqmc_stage_uniforms_tail_host(dqmc_ctx* c, const double* u, size_t nvals) {
    if (!c || !u) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (int rc = lookahead_ready(c)) return rc;
    if (nvals == 0 || nvals != c->uni_n) return fail(DQMC_EINVAL, "the tail must have the size of the current window of every chain");
    if (u != c->uni_pin) {
        if (c->tail_event_live) HIPCHK(hipEventSynchronize(c->ev_tail));
        memcpy(c->uni_pin, u, (size_t)c->nb * nvals * sizeof(double));
    }
    // the last splice read the tail buffer: the upload overwrites it only behind that kernel
    if (c->adv_event_live) HIPCHK(hipStreamWaitEvent(c->st_up, c->ev_adv, 0));
    HIPCHK(hipMemcpy2DAsync(c->uni_tail, c->lc.cs, c->uni_pin, nvals * sizeof(double), nvals * sizeof(double), (size_t)c->nb,
                            hipMemcpyHostToDevice, c->st_up));
    HIPCHK(hipEventRecord(c->ev_tail, c->st_up));
    c->tail_event_live = true;
    c->tail_staged = true;
    return DQMC_OK;
}
extern "C" int dqmc_advance_uniforms(dqmc_ctx* c, const uint64_t* offset) {
    if (!c || !offset) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (!c->uniforms_next) return fail(DQMC_EINVAL, "the context was created without the look-ahead on the uniforms (DQMC_TUNING_NO_RNG_LOOKAHEAD)");
    if (!c->tail_staged || c->uni_n == 0) return fail(DQMC_EINVAL, "dqmc_advance_uniforms: no tail is staged");
    for (int b = 0; b < c->nb; ++b)
        if (offset[b] > c->uni_n) return fail(DQMC_EINVAL, "dqmc_advance_uniforms: offset past the end of the window");
    if (c->adv_event_live) HIPCHK(hipEventSynchronize(c->ev_adv));         // the last splice may still be reading the offsets
    for (int b = 0; b < c->nb; ++b) c->uni_off[b] = offset[b];
    HIPCHK(hipStreamWaitEvent(c->st, c->ev_tail, 0));
    launch_advance_uniforms(c->lc, c->us, c->uniforms, c->uni_tail, c->uniforms_next, c->uni_off, c->uni_n);
    HIPCHK(hipEventRecord(c->ev_adv, c->st));
    c->adv_event_live = true;
    std::swap(c->uniforms, c->uniforms_next);
    c->tail_staged = false;
    c->windows_advanced += 1;
    return finish(c, "dqmc_advance_uniforms");
}
extern "C" int dqmc_get_uniform_window_host(dqmc_ctx* c, double* out, size_t nvals) {
    if (!c || (!out && nvals)) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (nvals > c->uni_cap) return fail(DQMC_EINVAL, "more uniforms than the window holds");
    HIPCHK(copy_sync(c, out, selp(c, c->uniforms), nvals * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// out[nchains]: the update state of every chain, one strided copy
extern "C" int dqmc_get_update_states_all_host(dqmc_ctx* c, dqmc_update_state* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipMemcpy2DAsync(out, sizeof(dqmc_update_state), &c->us->pub, c->lc.cs, sizeof(dqmc_update_state), (size_t)c->nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int b = 0; b < c->nb; ++b)
        if (out[b].error) return fail(out[b].error, "device ran out of pre-drawn uniforms");
    return DQMC_OK;
}

extern "C" int dqmc_update_slice(dqmc_ctx* c, int k, int thermalization) {
    return dqmc_update_slice_ex(c, k, thermalization, DQMC_PROPOSE_BOX, DQMC_ADAPT_BOX, 0, 1);
}

// skip_final: in the last pass over the slice a chain neither gathers nor flushes the block in which it finishes the slice
// (dqmc_update_slice_final; sequential schedule only).  The decisions, and with them everything but G, X and GrT, are untouched.
static int update_slice_run(dqmc_ctx* c, int k, int thermalization, int proposal, int adapt, int adapt_scale_variance, int repeat, bool skip_final) {
    if (k < 1 || k > c->m) return fail(DQMC_EINVAL, "updateInSlice: k out of range");
    if (c->currentTimeslice != k) return fail(DQMC_EINVAL, "updateInSlice: currentTimeslice != k");
    G_FRESH(c, "updateInSlice");
    if (proposal < DQMC_PROPOSE_BOX || proposal > DQMC_PROPOSE_ROTATE_AND_SCALE) return fail(DQMC_EINVAL, "updateInSlice: unknown proposal kind");
    if (proposal != DQMC_PROPOSE_BOX && (c->p.opdim != 3 || c->hm.hubbard))
        return fail(DQMC_EINVAL, "rotate / scale proposals are only supported for the O(3) model");      // detsdwopdim.cpp:3938, 4012, 4085
    if (adapt < DQMC_ADAPT_BOX || adapt > DQMC_ADAPT_SCALE) return fail(DQMC_EINVAL, "updateInSlice: unknown adaptation");
    if (repeat < 1) return fail(DQMC_EINVAL, "repeatUpdateInSlice must be >= 1");
    if (c->hm.hubbard && repeat != 1) return fail(DQMC_EINVAL, "Hubbard replica: repeat must be 1");
    const int adapt_what = adapt | (adapt_scale_variance ? 4 : 0);
    if (c->hm.hubbard) {            // DetHubbard::updateInSlice (dethubbard.cpp:141-172): the whole slice in one launch
        ProfScope ps(c, FAM_UPDATE, 1);
        launch_hubbard_slice(c->lc, c->hm, c->us, c->uniforms, c->G, k, c->hub_e_m2a, c->hub_e_p2a);
        return finish(c, "dqmc_update_slice");
    }
    const int rounds = (c->N + c->D - 1) / c->D;
    const int WD = c->MSF * c->D;
    // Pipelined form (latched at dqmc_create): decide(b + 1) needs G only inside its proposal window, so the window kernel hands it a
    // compact, already updated copy and the flush of block b over the whole of G runs on the second stream next to the decisions of
    // block b + 1; gather(b + 1) waits for it.  The first block of a pass reads G itself.  Profiling and DQMC_SYNC_CHECK keep the
    // schedule: the flush is timed / checked on the stream it runs on.
    const bool pipe = c->pipelined;
    Launch lc2 = c->lc; lc2.st = c->st2;
    auto pass = [&](int cdw_pass, int thermal, int reset_nd, bool skip) -> int {
        // skip: k_update_decide sets slice_done in the launch in which the chain's cursor reaches N and leaves block_j standing
        const int* done = skip ? &c->us->slice_done : nullptr;
        for (int r = 0; r < rounds; ++r) {
            {
                ProfScope ps(c, FAM_UPDATE, 1);
                launch_update_decide(c->lc, nullptr, c->hm, c->us, c->uniforms, c->G, c->W, k, r == 0, cdw_pass ? 0 : thermal, cdw_pass,
                                     c->Gwin, (pipe && r > 0) ? c->pipe_P : 0, proposal, adapt_what, reset_nd && r == 0);
            }
            if (pipe && r > 0) HIPCHK(hipStreamWaitEvent(c->st, c->ev_flush, 0));      // gather reads whole rows / columns of the flushed G
            {
                ProfScope ps(c, FAM_GATHER, 1);
                launch_update_gather(c->lc, c->hm, c->us, c->G, c->W, c->X, c->Gr, skip);
            }
            if (pipe) {
                { ProfScope ps(c, FAM_OTHER, 1); launch_update_window(c->lc, c->hm, c->us, c->G, c->X, c->Gr, c->Gwin, c->pipe_P); }
                HIPCHK(hipEventRecord(c->ev_win, c->st));
                HIPCHK(hipStreamWaitEvent(c->st2, c->ev_win, 0));
                {
                    ProfScope ps(c, FAM_FLUSH, 1, c->st2);
                    launch_flush(lc2, c->X, c->Gr, c->n_g, c->G, c->n_g, c->n_g, WD, &c->us->flush_k, 1);
                }
                HIPCHK(hipEventRecord(c->ev_flush, c->st2));
                c->blocks_pipelined += 1;
            } else {
                ProfScope ps(c, FAM_FLUSH, 1);
                launch_flush(c->lc, c->X, c->Gr, c->n_g, c->G, c->n_g, c->n_g, WD, &c->us->block_j, c->MSF, 0, done);
                c->blocks_sequential += 1;
            }
        }
        if (pipe) HIPCHK(hipStreamWaitEvent(c->st, c->ev_flush, 0));                     // whatever comes next on the main stream sees the flushed G
        return DQMC_OK;
    };
    // repeatUpdateInSlice passes over the slice (detsdwopdim.cpp:2438); the step-size adaptation sees the last one's acceptance ratio
    // (updateInSliceThermalization, :3294-3331); the Box-Muller stack of the scale proposals is reset once per updateInSlice (:2433)
    const bool skip = skip_final && !pipe;
    for (int rep = 0; rep < repeat; ++rep) {
        int rc = pass(0, (thermalization && rep == repeat - 1) ? 1 : 0, rep == 0, skip && rep == repeat - 1 && !c->hm.cdw_on);
        if (rc) return rc;
    }
    // cdwU != 0: the second pass over the slice updates the discrete field (detsdwopdim.cpp:2474-2485); its acceptance ratio is
    // discarded there and here (no step-width adaptation)
    if (c->hm.cdw_on) { int rc = pass(1, 0, 0, skip); if (rc) return rc; }
    return finish(c, "dqmc_update_slice");
}

extern "C" int dqmc_update_slice_ex(dqmc_ctx* c, int k, int thermalization, int proposal, int adapt, int adapt_scale_variance, int repeat) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    return update_slice_run(c, k, thermalization, proposal, adapt, adapt_scale_variance, repeat, false);
}

extern "C" int dqmc_update_slice_final(dqmc_ctx* c, int k, int thermalization, int proposal, int adapt, int adapt_scale_variance, int repeat,
                                       int then_wrap_dir) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    if (then_wrap_dir != 0 && then_wrap_dir != DQMC_DOWN) return fail(DQMC_EINVAL, "updateInSlice: then_wrap_dir must be 0 or DQMC_DOWN");
    const bool skip = !c->pipelined && !c->hm.hubbard;
    // k in 1 .. m and currentTimeslice == k (update_slice_run refuses anything else before it launches): wrapDown's own checks hold
    int rc = update_slice_run(c, k, thermalization, proposal, adapt, adapt_scale_variance, repeat, skip);
    if (rc) return rc;
    if (!skip) return then_wrap_dir == DQMC_DOWN ? dqmc_wrap(c, DQMC_DOWN, k) : DQMC_OK;
    if (then_wrap_dir == DQMC_DOWN) c->currentTimeslice = k - 1;
    c->g_stale = true;
    return DQMC_OK;
}

extern "C" int dqmc_get_schedule_info(dqmc_ctx* c, dqmc_schedule_info* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    memset(out, 0, sizeof(*out));
    out->pipelined = c->pipelined ? 1 : 0;
    out->proposal_budget = c->hm.pbudget;
    out->blocks_pipelined = c->blocks_pipelined;
    out->blocks_sequential = c->blocks_sequential;
    out->qr_block_gram_schmidt = (c->stab == DQMC_STAB_QR && c->qr_bgs) ? 1 : 0;
    out->green_lu = (c->stab == DQMC_STAB_QR && c->green_lu) ? 1 : 0;
    out->cholqr_fallbacks = c->cholqr_fallbacks;
    out->uniform_windows_advanced = c->windows_advanced;
    out->uniform_windows_pushed = c->windows_pushed;
    return DQMC_OK;
}

extern "C" int dqmc_get_update_state_host(dqmc_ctx* c, dqmc_update_state* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
#ifdef DQMC_DECIDE_TIMING
    if (c->hm.dbg & 8) {     // developer phase timers of the decision kernel
        DevUpdateState h;
        HIPCHK(copy_sync(c, &h, selp(c, c->us), sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "[decide cycles, chain %d, %llu launches]", c->sel, h.dbg_cycles[12]);
        for (int i = 0; i < 10; ++i) fprintf(stderr, " t%d=%llu", i, h.dbg_cycles[i]);
        fprintf(stderr, "\n");
    }
#endif
    HIPCHK(copy_sync(c, out, &selp(c, c->us)->pub, sizeof(*out), hipMemcpyDeviceToHost));
    if (out->error) return fail(out->error, "device ran out of pre-drawn uniforms");
    return DQMC_OK;
}
extern "C" int dqmc_set_update_state_host(dqmc_ctx* c, const dqmc_update_state* in) {
    if (!c || !in) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, &selp(c, c->us)->pub, in, sizeof(*in), hipMemcpyHostToDevice));
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// host-buffer entry points (tests, measurements, global moves)
// ---------------------------------------------------------------------------------------------
extern "C" int dqmc_bmult_host(dqmc_ctx* c, int side, int inverse, int k2, int k1, dqmc_cplx* A) {
    if (!c || !A) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (!(k2 > k1) || k2 > c->m || k1 < 0) return fail(DQMC_EINVAL, "need 0 <= k1 < k2 <= m");
    const size_t n2 = (size_t)c->n_g * c->n_g;
    for (int b = 0; b < c->nb; ++b)     // every chain gets the input; the selected chain's result is returned
        HIPCHK(hipMemcpyAsync(chainp(c, c->T1, b), A, n2 * sizeof(cplx), hipMemcpyHostToDevice, c->st));
    bmult_dev(c, side, inverse, k2, k1, c->T1);
    HIPCHK(hipMemcpyAsync(A, selp(c, c->T1), n2 * sizeof(cplx), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_bmult_host");
}
// out of place: source in T3, destination T1 filled with NaN bit patterns first (nothing of its old content may enter the result)
extern "C" int dqmc_bmult_src_host(dqmc_ctx* c, int side, int inverse, int k2, int k1, const dqmc_cplx* src, dqmc_cplx* out, dqmc_cplx* src_after) {
    if (!c || !src || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    if (!(k2 > k1) || k2 > c->m || k1 < 0) return fail(DQMC_EINVAL, "need 0 <= k1 < k2 <= m");
    const size_t n2 = (size_t)c->n_g * c->n_g;
    for (int b = 0; b < c->nb; ++b) {
        HIPCHK(hipMemcpyAsync(chainp(c, c->T3, b), src, n2 * sizeof(cplx), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(chainp(c, c->T1, b), 0xff, n2 * sizeof(cplx), c->st));
    }
    bmult_dev(c, side, inverse, k2, k1, c->T1, c->T3);
    HIPCHK(hipMemcpyAsync(out, selp(c, c->T1), n2 * sizeof(cplx), hipMemcpyDeviceToHost, c->st));
    if (src_after) HIPCHK(hipMemcpyAsync(src_after, selp(c, c->T3), n2 * sizeof(cplx), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_bmult_src_host");
}

extern "C" int dqmc_udv_decompose_host(dqmc_ctx* c, const dqmc_cplx* M, dqmc_cplx* U, double* d, dqmc_cplx* V_t,
                                       int* sweeps_used) {
    if (!c || !M || !U || !d || !V_t) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t n2 = (size_t)c->n_g * c->n_g;
    for (int b = 0; b < c->nb; ++b)
        HIPCHK(hipMemcpyAsync(chainp(c, c->T1, b), M, n2 * sizeof(cplx), hipMemcpyHostToDevice, c->st));
    int rc = decompose(c, c->T1, nullptr, nullptr, KIND_R, c->tmpudv);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, U, selp(c, c->tmpudv.U), n2 * sizeof(cplx), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, d, selp(c, c->tmpudv.d), c->n_g * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, V_t, selp(c, c->tmpudv.Vt), n2 * sizeof(cplx), hipMemcpyDeviceToHost));
    if (sweeps_used) *sweeps_used = c->last_svd_sweeps;
    return DQMC_OK;
}

// Test-facing: the stabilisation routines on caller-given operands, every chain its own (dqmc_hip.h).  They borrow buffers of the sweep
// (spare, tmpudv, storage[0], T1, T3, sv, G and the time-displaced matrices), so the context's own state is void afterwards:
static void stab_test_invalidate(dqmc_ctx* c) {
    c->g_stale = true;
    c->currentTimeslice = -1;                          // no dqmc_advance accepts this: only dqmc_udv_setup brings the context back
    c->td_slice = -1;
}
// per-chain upload / download of [nb][count] host arrays
template<class T>
static int stab_upload(dqmc_ctx* c, T* dev, const void* host, size_t count) {
    for (int b = 0; b < c->nb; ++b)
        HIPCHK(hipMemcpyAsync(chainp(c, dev, b), (const T*)host + (size_t)b * count, count * sizeof(T), hipMemcpyHostToDevice, c->st));
    return DQMC_OK;
}
template<class T>
static int stab_download(dqmc_ctx* c, void* host, const T* dev, size_t count) {
    if (!host) return DQMC_OK;
    for (int b = 0; b < c->nb; ++b)
        HIPCHK(hipMemcpyAsync((T*)host + (size_t)b * count, chainp(c, dev, b), count * sizeof(T), hipMemcpyDeviceToHost, c->st));
    return DQMC_OK;
}

extern "C" int dqmc_decompose_host(dqmc_ctx* c, const dqmc_cplx* M, const double* colscale, const double* rowscale, int kind,
                                   const dqmc_cplx* Aold, dqmc_cplx* U, double* d, dqmc_cplx* V_t, int* sweeps_used) {
    if (!c || !M || !U || !d || !V_t) return fail(DQMC_EINVAL, "null argument");
    if (kind != KIND_R && kind != KIND_L) return fail(DQMC_EINVAL, "kind must be 0 (R-type) or 1 (L-type)");
    (void)hipSetDevice(c->p.device);
    const size_t n2 = (size_t)c->n_g * c->n_g, ng = (size_t)c->n_g;
    stab_test_invalidate(c);
    int rc;
    // operands where no factorisation writes: M in T1 (as in the sweep), the scales in tmpudv.d and sv, the old factor in T3
    if ((rc = stab_upload(c, c->T1, M, n2))) return rc;
    if (colscale && (rc = stab_upload(c, c->tmpudv.d, colscale, ng))) return rc;
    if (rowscale && (rc = stab_upload(c, c->sv, rowscale, ng))) return rc;
    if (Aold && (rc = stab_upload(c, c->T3, Aold, n2))) return rc;
    const double* cs = colscale ? c->tmpudv.d : nullptr;
    const double* rs = rowscale ? c->sv : nullptr;
    c->last_svd_sweeps = 0;
    rc = Aold ? decompose_chained(c, c->T1, cs, rs, kind, c->spare, c->T3) : decompose(c, c->T1, cs, rs, kind, c->spare);
    if (rc) return rc;
    if ((rc = stab_download(c, U, c->spare.U, n2))) return rc;
    if ((rc = stab_download(c, d, c->spare.d, ng))) return rc;
    if ((rc = stab_download(c, V_t, c->spare.Vt, n2))) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    if (sweeps_used) *sweeps_used = c->last_svd_sweeps;
    return finish(c, "dqmc_decompose_host");
}

extern "C" int dqmc_green_from_factors_host(dqmc_ctx* c, const dqmc_cplx* U_l, const double* d_l, const dqmc_cplx* V_l,
                                            const dqmc_cplx* U_r, const double* d_r, const dqmc_cplx* V_r,
                                            dqmc_cplx* G, double* sv, dqmc_cplx* GT0, dqmc_cplx* G0T, dqmc_cplx* G00) {
    if (!c || !G || !sv) return fail(DQMC_EINVAL, "null argument");
    const bool hasL = U_l && d_l && V_l, hasR = U_r && d_r && V_r;
    if ((!hasL && (U_l || d_l || V_l)) || (!hasR && (U_r || d_r || V_r))) return fail(DQMC_EINVAL, "a slot is given whole or not at all");
    if (!hasL && !hasR) return fail(DQMC_EINVAL, "at least one slot is needed");
    const bool td = hasL && hasR && c->td_on;
    if ((GT0 || G0T) && !td) return fail(DQMC_EINVAL, "G(tau,0), G(0,tau): both slots and dqmc_set_timedisplaced(on) are needed");
    if (G00 && !(td && c->G00)) return fail(DQMC_EINVAL, "G(0): both slots, dqmc_set_timedisplaced(on) and dqmc_params::td_particle_hole are needed");
    (void)hipSetDevice(c->p.device);
    const size_t n2 = (size_t)c->n_g * c->n_g, ng = (size_t)c->n_g;
    stab_test_invalidate(c);
    int rc;
    // the slots where the sweep keeps them: no routine below writes spare or storage[0]
    const UdVSlot &L = c->spare, &R = c->storage[0];
    if (hasL) {
        if ((rc = stab_upload(c, L.U, U_l, n2)) || (rc = stab_upload(c, L.d, d_l, ng)) || (rc = stab_upload(c, L.Vt, V_l, n2))) return rc;
    }
    if (hasR) {
        if ((rc = stab_upload(c, R.U, U_r, n2)) || (rc = stab_upload(c, R.d, d_r, ng)) || (rc = stab_upload(c, R.Vt, V_r, n2))) return rc;
    }
    if (hasL && hasR) rc = green_from_udv(c, L, R);
    else rc = hasR ? green_from_eye(c, R, KIND_R) : green_from_eye(c, L, KIND_L);
    if (rc) return rc;
    if ((rc = stab_download(c, G, c->G, n2)) || (rc = stab_download(c, sv, c->sv, ng))) return rc;
    if (td && ((rc = stab_download(c, GT0, c->GT0, n2)) || (rc = stab_download(c, G0T, c->G0T, n2)))) return rc;
    if (td && c->G00 && (rc = stab_download(c, G00, c->G00, n2))) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_green_from_factors_host");
}

extern "C" int dqmc_gemm_host(dqmc_ctx* c, int opA, int opB, const dqmc_cplx* A, const dqmc_cplx* B, dqmc_cplx* C) {
    if (!c || !A || !B || !C) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t n2 = (size_t)c->n_g * c->n_g;
    for (int b = 0; b < c->nb; ++b) {
        HIPCHK(hipMemcpyAsync(chainp(c, c->T1, b), A, n2 * sizeof(cplx), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(chainp(c, c->T2, b), B, n2 * sizeof(cplx), hipMemcpyHostToDevice, c->st));
    }
    run_gemm(c, gemm_square(c, c->T1, opA, c->T2, opB, c->T3));
    HIPCHK(hipMemcpyAsync(C, selp(c, c->T3), n2 * sizeof(cplx), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_gemm_host");
}

extern "C" int dqmc_get_green_host(dqmc_ctx* c, dqmc_cplx* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    G_FRESH(c, "dqmc_get_green_host");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, out, selp(c, c->G), (size_t)c->n_g * c->n_g * sizeof(cplx), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_set_green_host(dqmc_ctx* c, const dqmc_cplx* in, int currentTimeslice) {
    if (!c || !in) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, selp(c, c->G), in, (size_t)c->n_g * c->n_g * sizeof(cplx), hipMemcpyHostToDevice));
    c->currentTimeslice = currentTimeslice;
    c->g_stale = false;
    return DQMC_OK;
}
extern "C" int dqmc_get_sv_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, out, selp(c, c->sv), c->n_g * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// green_inv_sv of every chain: out[nchains][n_g]
extern "C" int dqmc_get_sv_all_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    const size_t bytes = (size_t)c->n_g * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(out, bytes, c->sv, c->lc.cs, bytes, (size_t)c->nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" int dqmc_get_udv_host(dqmc_ctx* c, int l, dqmc_cplx* U, double* d, dqmc_cplx* V_t) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    if (l < 0 || l > c->n) return fail(DQMC_EINVAL, "l out of range");
    const size_t n2 = (size_t)c->n_g * c->n_g;
    HIPCHK(hipStreamSynchronize(c->st));
    if (U) HIPCHK(copy_sync(c, U, selp(c, c->storage[l].U), n2 * sizeof(cplx), hipMemcpyDeviceToHost));
    if (d) HIPCHK(copy_sync(c, d, selp(c, c->storage[l].d), c->n_g * sizeof(double), hipMemcpyDeviceToHost));
    if (V_t) HIPCHK(copy_sync(c, V_t, selp(c, c->storage[l].Vt), n2 * sizeof(cplx), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_current_timeslice(dqmc_ctx* c) { return c ? c->currentTimeslice : -1; }

// globalMoveStoreBackups / RestoreBackups (detsdwopdim.cpp:3886-3917).  Backup (all chains): the fields are
// copied, the matrices the move recomputes from scratch (G, sv, UdV storage) swap roles with their backup
// buffers -- the same swap for every chain, so the chains keep one arena layout.  Restore (the selected
// chain only: each chain accepts or rejects its own move): copies that chain's backup back.
static void swap_state(dqmc_ctx* c) {
    std::swap(c->G, c->G_bak);
    std::swap(c->sv, c->sv_bak);
    std::swap(c->storage, c->storage_bak);
}
extern "C" int dqmc_backup(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    G_FRESH(c, "dqmc_backup");
    (void)hipSetDevice(c->p.device);
    const size_t nphi = (size_t)(c->m + 1) * c->p.opdim * c->N, ncs = (size_t)(c->m + 1) * c->N;
    launch_copy_bytes(c->lc, c->phi, c->phi_bak, nphi * sizeof(double));
    launch_copy_bytes(c->lc, c->coshT, c->cosh_bak, ncs * sizeof(double));
    launch_copy_bytes(c->lc, c->sinhT, c->sinh_bak, ncs * sizeof(double));
    swap_state(c);
    return finish(c, "dqmc_backup");
}
extern "C" int dqmc_restore(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    const size_t nphi = (size_t)(c->m + 1) * c->p.opdim * c->N, ncs = (size_t)(c->m + 1) * c->N;
    const size_t n2b = (size_t)c->n_g * c->n_g * sizeof(cplx), nb1 = (size_t)c->n_g * sizeof(double);
#define CP_(dst, src, bytes) HIPCHK(hipMemcpyAsync(selp(c, dst), selp(c, src), bytes, hipMemcpyDeviceToDevice, c->st))
    CP_(c->phi, c->phi_bak, nphi * sizeof(double));
    CP_(c->coshT, c->cosh_bak, ncs * sizeof(double));
    CP_(c->sinhT, c->sinh_bak, ncs * sizeof(double));
    CP_(c->G, c->G_bak, n2b);
    CP_(c->sv, c->sv_bak, nb1);
    for (int l = 0; l <= c->n; ++l) {
        CP_(c->storage[l].U, c->storage_bak[l].U, n2b);
        CP_(c->storage[l].d, c->storage_bak[l].d, nb1);
        CP_(c->storage[l].Vt, c->storage_bak[l].Vt, n2b);
    }
#undef CP_
    c->currentTimeslice = c->m;
    c->g_stale = false;                  // backups are only ever taken of a fresh G
    return finish(c, "dqmc_restore");
}

extern "C" int dqmc_exchange_action_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    { ProfScope ps(c, FAM_OTHER, 1); launch_phi_sq_sum(c->lc, c->hm, c->scalar_out); }
    HIPCHK(hipStreamSynchronize(c->st));
    double v;
    HIPCHK(copy_sync(c, &v, selp(c, c->scalar_out), sizeof(double), hipMemcpyDeviceToHost));
    *out = 0.5 * c->p.dtau * v;
    return DQMC_OK;
}

// The same for ALL chains, left ON THE DEVICE: out_dev[b] = 1/2 dtau sum phi^2 of chain b, out_dev a caller-owned device array of
// nchains doubles (e.g. the send buffer of the replica-exchange all_gather over RCCL: no host hop).  Returns when the values are there.
extern "C" int dqmc_exchange_actions_device(dqmc_ctx* c, double* out_dev) {
    if (!c || !out_dev) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, out_dev) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(DQMC_EINVAL, "dqmc_exchange_actions_device: out_dev must be device memory");
    }
    {
        ProfScope ps(c, FAM_OTHER, 2);
        launch_phi_sq_sum(c->lc, c->hm, c->scalar_out);
        launch_gather_scalars(c->lc, c->scalar_out, 0.5 * c->p.dtau, out_dev);
    }
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_exchange_actions_device");
}

// phiAction of every chain (detsdwopdim.cpp:4242-4300), computed on the device from the resident field: out[nchains]
extern "C" int dqmc_phi_action_all_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    { ProfScope ps(c, FAM_OTHER, 1); launch_phi_action(c->lc, c->hm, c->us, c->scalar_out); }
    HIPCHK(hipMemcpy2DAsync(out, sizeof(double), c->scalar_out, c->lc.cs, sizeof(double), (size_t)c->nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return finish(c, "dqmc_phi_action_all_host");
}
// addGlobalRandomDisplacement for every chain: shifts[nchains][opdim]; also refreshes the cosh / sinh caches
extern "C" int dqmc_shift_fields_all_host(dqmc_ctx* c, const double* shifts) {
    if (!c || !shifts) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    HIPCHK(copy_sync(c, c->shift_buf, shifts, (size_t)c->nb * c->p.opdim * sizeof(double), hipMemcpyHostToDevice));
    { ProfScope ps(c, FAM_OTHER, 2); launch_phi_shift(c->lc, c->hm, c->shift_buf); launch_cosh_sinh(c->lc, c->hm); }
    return finish(c, "dqmc_shift_fields_all_host");
}

extern "C" int dqmc_set_exchange_parameter(dqmc_ctx* c, double r) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    if (c->sel == 0) { c->p.r = r; c->hm.r = r; }
    HIPCHK(hipStreamSynchronize(c->st));     // the decision kernel reads DevUpdateState::r of its chain
    HIPCHK(copy_sync(c, (char*)selp(c, c->us) + offsetof(DevUpdateState, r), &r, sizeof(double), hipMemcpyHostToDevice));
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
static void sub_prof_begin(void* u, int sub) {
    dqmc_ctx* c = (dqmc_ctx*)u;
    c->sub_open.push_back({sub, prof_event_pair(c, c->st)});
}
static void sub_prof_end(void* u, int sub, double flops, double bytes) {
    dqmc_ctx* c = (dqmc_ctx*)u;
    (void)hipEventRecord(c->ev_pool[c->sub_open.back().second + 1], c->st);
    c->sub_launches[sub] += 1; c->sub_flops[sub] += flops; c->sub_bytes[sub] += bytes;
}
void prof_collect(dqmc_ctx* c) {
    (void)hipStreamSynchronize(c->st);
    if (c->st2) (void)hipStreamSynchronize(c->st2);
    for (auto& o : c->ev_open) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[o.second], c->ev_pool[o.second + 1]) == hipSuccess)
            c->fam_ms[o.first] += ms;
    }
    for (auto& o : c->sub_open) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[o.second], c->ev_pool[o.second + 1]) == hipSuccess)
            c->sub_ms[o.first] += ms;
    }
    c->sub_open.clear();
    c->ev_open.clear();
    c->ev_used = 0;
}
extern "C" int dqmc_profile_enable(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    prof_collect(c);
    c->prof = on != 0;
    c->subprof = SubProf{sub_prof_begin, sub_prof_end, c};
    c->lc.sub = c->prof ? &c->subprof : nullptr;
    c->qr_apply_hooks = SvdProfHooks{svd_prof_begin, qr_apply_prof_end, c};
    c->qw.apply_hooks = c->prof ? &c->qr_apply_hooks : nullptr;
    for (int i = 0; i < FAM_COUNT; ++i) { c->fam_ms[i] = 0; c->fam_launches[i] = 0; }
    for (int i = 0; i < SUBFAM_COUNT; ++i) { c->sub_ms[i] = 0; c->sub_flops[i] = 0; c->sub_bytes[i] = 0; c->sub_launches[i] = 0; }
    c->svd_calls = 0; c->svd_sweeps_total = 0; c->svd_sweeps_max = 0; c->qr_calls = 0; c->lu_calls = 0; c->gemm_flops = 0.0;
    const unsigned long long zero[2] = {0, 0};
    for (int b = 0; b < c->nb; ++b)
        HIPCHK(copy_sync(c, (char*)chainp(c, c->us, b) + offsetof(DevUpdateState, blocks_nonempty), zero, sizeof(zero), hipMemcpyHostToDevice));
    return DQMC_OK;
}
extern "C" int dqmc_profile_read(dqmc_ctx* c, dqmc_profile* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    (void)hipSetDevice(c->p.device);
    prof_collect(c);
    memset(out, 0, sizeof(*out));
    for (int i = 0; i < 7; ++i) { out->ms[i] = c->fam_ms[i]; out->launches[i] = c->fam_launches[i]; }
    // SVD mode: the decomposition family is dominated by the rounds, which are timed batch-wise
    if (c->stab == DQMC_STAB_SVD) out->ms[DQMC_FAM_DECOMP] = c->fam_ms[FAM_ROUNDS];
    out->svd_calls = c->svd_calls; out->svd_sweeps_total = c->svd_sweeps_total; out->svd_sweeps_max = (uint64_t)c->svd_sweeps_max;
    out->qr_calls = c->qr_calls;
    out->lu_calls = c->lu_calls;
    out->gemm_flops = c->gemm_flops;
    out->decomp_round_ms = c->fam_ms[FAM_ROUNDS];
    out->decomp_rounds = c->fam_launches[FAM_ROUNDS];
    for (int b = 0; b < c->nb; ++b) {            // summed over the chains: independent of the selected chain
        unsigned long long v[2];
        HIPCHK(copy_sync(c, v, (char*)chainp(c, c->us, b) + offsetof(DevUpdateState, blocks_nonempty), sizeof(v), hipMemcpyDeviceToHost));
        out->blocks_nonempty += v[0];
        out->updates_accepted += v[1];
    }
    out->chains = (uint64_t)c->nb;
    for (int i = 0; i < SUBFAM_COUNT; ++i) {
        out->sub_ms[i] = c->sub_ms[i]; out->sub_launches[i] = c->sub_launches[i]; out->sub_flops[i] = c->sub_flops[i]; out->sub_bytes[i] = c->sub_bytes[i];
    }
    return DQMC_OK;
}
