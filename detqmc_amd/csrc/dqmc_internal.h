// Internal declarations shared by the HIP kernels and the C-ABI implementation.
// Not part of the public boundary (that is include/dqmc_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dqmc_hip.h"

#include <stdlib.h>
#include <float.h>
// Developer A/B switches of individual kernels (tile shapes, 3M vs 4M products, ...).  None changes a result.  They exist only in
// builds with -DDQMC_DEV_KNOBS (DQMC_BUILD_DEFINES=-DDQMC_DEV_KNOBS python -m detqmc_amd.build --force); the shipped library reads
// ONE environment variable, DQMC_SYNC_CHECK (debug mode, dqmc_ctx.h) -- everything else that selects an execution variant is
// a create-time parameter (dqmc_tuning, include/dqmc_hip.h).
static inline const char* dev_knob(const char* name) {
#ifdef DQMC_DEV_KNOBS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

typedef double2 cplx;   // .x = re, .y = im; same bytes as dqmc_cplx / std::complex<double>

#define DQMC_MAX_MSF 4
#define DQMC_MAX_WDIM 64          // MSF * delaySteps <= 64 (W lives in LDS in the decision kernel)
#define DQMC_DECIDE_WIDE_MAX_CHAINS 32   // contexts of at most this many chains launch k_update_decide with 512 threads (kernels_update.hip)

// ---- batched chains ---------------------------------------------------------------------------
// One context can run nb independent Markov chains (replicas) in lockstep.  Every per-chain device buffer of
// chain b lives at (address of chain 0's buffer) + b * cs: all chains share one arena layout.  Kernels are
// launched with gridDim.z = nb and shift their per-chain pointer arguments by blockIdx.z * cs; read-only
// tables (plaquette tables, neighbours, tournament schedule) are shared and never shifted.
// sub: optional timing hooks for launches that belong to a kernel family of their own INSIDE a larger scope (profiling only): the
// trailing updates of the LU factorisation on the flush kernel (sub-family 0) and the products inside factorisations / triangular
// solves on k_zgemm (sub-family 1) -- both fill the GPU and are priced against a roof, unlike the panel kernels around them
enum { SUBFAM_LU_UPDATE = 0, SUBFAM_FACT_GEMM = 1, SUBFAM_COUNT = 4 };
struct SubProf { void (*begin)(void* user, int sub); void (*end)(void* user, int sub, double flops, double bytes); void* user; };
struct Launch { hipStream_t st; int nb; size_t cs; const SubProf* sub = nullptr; };
template<class T> __device__ __forceinline__ T* chain_ptr(T* p, size_t cs) {
    return p ? (T*)((char*)p + (size_t)blockIdx.z * cs) : p;
}
#define CHAIN(p) p = chain_ptr(p, cs)
// streaming (nontemporal) access to a matrix element: for operands a kernel touches exactly once per launch, so that they do not
// evict the panels / tables the same kernel re-reads from the L2 (one global_load/store_dwordx4 with the nt bit)
__device__ __forceinline__ cplx nt_load(const cplx* p) {
    cplx t;
    t.x = __builtin_nontemporal_load(&p->x); t.y = __builtin_nontemporal_load(&p->y);
    return t;
}
__device__ __forceinline__ void nt_store(cplx* p, const cplx& v) {
    __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y);
}
// 1 / v = conj(v) / |v|^2.  When |v|^2 is not a normal number (|v| outside ~ [1.5e-154, 1.3e154]: it would be 0, subnormal or inf) v is
// first scaled by a power of two, s = v 2^-e with max(|re s|, |im s|) in [1, 2), and 1 / v = (conj(s) / |s|^2) 2^-e.  The scaled form
// rounds exactly like the direct one would without the range limit, and inputs with a normal |v|^2 take the direct form unchanged.
// v = 0, inf or NaN: the direct form (inf / NaN result).  Used by the triangular solve (k_trsm_block) and the LU pivots (k_lu_panel).
__device__ __forceinline__ cplx cplx_recip(cplx v) {
    const double dn = v.x * v.x + v.y * v.y;
    const double mx = fmax(fabs(v.x), fabs(v.y));
    if (!(dn >= DBL_MIN && dn <= DBL_MAX) && mx > 0.0 && mx <= DBL_MAX) {
        const int e = ilogb(mx);
        const double sx = ldexp(v.x, -e), sy = ldexp(v.y, -e), sn = sx * sx + sy * sy;
        return make_double2(ldexp(sx / sn, -e), ldexp(-sy / sn, -e));
    }
    return make_double2(v.x / dn, -v.y / dn);
}
// XCD-aware launch shape for the wide MFMA kernels: consecutive workgroup ids go round-robin over the 8 XCDs (each with
// its own L2), so with a 1-D grid and   xcd = id % 8,  chain = 8 * (id / 8 / tiles) + xcd,  tile = (id / 8) % tiles
// all tiles of one chain run on ONE XCD and share the operand panels in that L2 instead of fetching them 8 times.
// Used when the number of chains is a multiple of 8; otherwise grid.z = chain as everywhere else.
template<class T> __device__ __forceinline__ T* chain_ptr_i(T* p, size_t cs, int chain) {
    return p ? (T*)((char*)p + (size_t)chain * cs) : p;
}
__device__ __forceinline__ void xcd_chain_tile(int tiles, int nb, int& chain, int& tile) {
    if (gridDim.z == 1 && nb > 1) {
        const int id = blockIdx.x, xcd = id & 7, t = id >> 3;
        chain = (t / tiles) * 8 + xcd;
        tile = t % tiles;
    } else {
        chain = blockIdx.z;
        tile = blockIdx.x;
    }
}

// Everything a kernel needs to know about the model; lives in device memory, one per context.
struct DevModel {
    int opdim, MSF, L, N, ng, m, s, n, D, P;   // P = plaquettes per subgroup = N/4
    int phi2bosons;
    int decide_nt;     // threads per workgroup of k_update_decide: 0 automatic, 256, 512 (dqmc_tuning::decide_threads)
    int bmult_path;    // checkerboard B-multiply kernel: 0 automatic, 1 k_bmult_chain, 2 k_bmult_direct where it applies (dqmc_tuning::bmult_path)
    int pbudget;       // proposals per delayed-update block (0: no limit); a launch-balancing knob, the chain does not depend on it
    int dbg;           // bit 3: phase timers of k_update_decide; only ever set in builds with -DDQMC_DECIDE_TIMING (always 0 otherwise)
    int dense;         // CB_NONE: the hopping part is a dense GEMM done by the host loop, the chain kernel
                       // only applies e^{+-dtau V}; ov/ovinv are 1 (mu sits inside propK)
    double dtau, r, c, u, lambda;   // r: chain 0's value at create time only -- kernels read DevUpdateState::r
    double ov[2];      // e^{+dtau mu_band}   (detsdwopdim.cpp:2037-2038)
    double ovinv[2];   // e^{-dtau mu_band}   (detsdwopdim.cpp:2137-2138)
    // plaquette sites [sub][4][P] (sub 0: even corners, sub 1: odd corners; detsdwopdim.cpp:1776-1785).  All
    // plaquette tables are structure-of-arrays over the plaquette index: lanes work on consecutive plaquettes
    const int* psites;
    // 4x4 complex plaquette exponentials [band][signIdx][sub][16 (row-major entry)][P]; sub 1 holds the
    // half-step matrices, sub 0 the full-step ones (symmetric break-up, detsdwopdim.cpp:1846-1865);
    // signIdx 0: e^{-dtau K}, 1: e^{+dtau K}.  Used with a magnetic flux (complex Hermitian matrices).
    const cplx* pmats;
    // without flux the matrices are real with four distinct entries, rows (a b c d)(b a d c)(c d a b)(d c b a)
    // (cb_assaad_applyBondFactorsLeft, detsdwopdim.cpp:1688-1756): [band][signIdx][sub][4][P]
    const double* pabcd;
    int pm_real;
    // the same two tables with HALF steps for both subgroups (shiftGreenSymmetric, detsdwopdim.cpp:4507-4563)
    const cplx* pmats_h;
    const double* pabcd_h;
    // fields
    double* phi;       // [m+1][opdim][N]
    double* coshT;     // [m+1][N]
    double* sinhT;     // [m+1][N]
    // cdwU != 0 (cdw_on): the discrete four-valued field l_i(tau_k) in {+-1, +-2} (kept as doubles: it travels with the other per-site
    // scalars of a proposal) and its caches cosh / sinh(sqrt(dtau) cdwU eta(l)) (coshTermCDWl / sinhTermCDWl, detsdwopdim.cpp:1138-1163)
    int cdw_on;
    double* cdwl;      // [m+1][N]
    double* cdwC;      // [m+1][N]
    double* cdwS;      // [m+1][N]
    double cdw_cosh[2], cdw_sinh[2];   // |l| = 1, 2 (sinh for l > 0)
    double cdw_gamma[2];               // cdwl_gamma(|l|) (detsdwopdim.h:1209-1220)
    const int* neigh;  // [4][N]  XPLUS, XMINUS, YPLUS, YMINUS (neighbortable.h:34-36)
    // Hubbard replica (dqmc_params::model == DQMC_MODEL_HUBBARD): phi holds the Ising auxiliary field (+-1.0, opdim = 1),
    // the hopping part is the dense propagator (dense = 1), the site-diagonal part is e^{+-alpha s} (kernels_hubbard.hip)
    int hubbard;
    double hub_exp_alpha[2];   // e^{+alpha}, e^{-alpha}, cosh(alpha) = e^{dtau U / 2} (dethubbard.cpp:55)
};
__device__ __forceinline__ DevModel chain_model(DevModel dm, size_t cs) {
    dm.phi = chain_ptr(dm.phi, cs); dm.coshT = chain_ptr(dm.coshT, cs); dm.sinhT = chain_ptr(dm.sinhT, cs);
    if (dm.cdw_on) { dm.cdwl = chain_ptr(dm.cdwl, cs); dm.cdwC = chain_ptr(dm.cdwC, cs); dm.cdwS = chain_ptr(dm.cdwS, cs); }
    return dm;
}

struct DevUpdateState {
    dqmc_update_state pub;   // mirrored to the host on request
    int site_cursor;         // next site to be proposed in the current slice
    int acc_count;           // accepted proposals in the current slice
    int block_j;             // accepted updates in the block the last decision launch produced
    int slice_done;
    int flush_k;             // K = MSF j of the block whose flush is in flight (pipelined update: block_j already belongs to the next block)
    int nd_has;              // rotate / scale proposals: the Box-Muller stack of NormalDistribution holds a value (normaldistribution.h), ...
    double nd_cached;        // ... this one; reset at the top of every updateInSlice
    int chol_fail;           // set by k_chol64 when a Cholesky-QR panel fails its pivot test; read and cleared by the host after the factorisation
    double r;                // this chain's exchange parameter (differs between the chains of a batch)
    int block_sites[DQMC_MAX_WDIM];
    unsigned long long blocks_nonempty;  // delayed-update blocks that accepted at least one update (-> real flushes)
    unsigned long long updates_accepted; // accepted local updates (sum of the block ranks j); must follow blocks_nonempty
    unsigned long long dbg_cycles[16];   // developer phase timers of the decision kernel (-DDQMC_DECIDE_TIMING builds only)
};

// ---- launchers (implemented in the kernels_*.hip files) ---------------------------------------
// checkerboard chain: A <- prod B_k A etc. for k = kfirst, kfirst+kstep, ... (count slices)
void launch_bmult(const Launch& lc, const DevModel* dm, const DevModel& hm, int side, int inverse,
                  int kfirst, int kstep, int kcount, cplx* A, int lda, int shift = 0,    // shift: half-step hopping passes only
                  const cplx* Asrc = nullptr);   // Asrc: out of place -- the operands are read from Asrc (layout and lda of A), A is only written

// A matrix that is read where it lies instead of being copied first: column j of it is X[:, col] * scale[col] with col = idx ? idx[j] : j
// (idx == nullptr: the columns in place; scale == nullptr: 1).  k_gather_scale_cols and, with the identity, k_permute_scale_cols write
// exactly these values; a kernel that takes a ColSrc forms them with col_src_value, the same single multiply per component.
// X == nullptr: no source.  All three pointers are per-chain buffers.
struct ColSrc { const cplx* X; int ld; const int* idx; const double* scale; };
// the source of the columns from j0 on
static inline ColSrc col_src_from(const ColSrc& s, int j0) {
    ColSrc r = s;
    if (!r.X) return r;
    if (r.idx) r.idx += j0;
    else { r.X += (size_t)j0 * r.ld; if (r.scale) r.scale += j0; }
    return r;
}
#ifdef __HIPCC__
// v * s, never contracted into a neighbouring add: the value equals the one a copy kernel would have stored
__device__ __forceinline__ cplx col_src_value(cplx v, double s) {
#pragma clang fp contract(off)
    return make_double2(v.x * s, v.y * s);
}
#endif

// C = alpha-less complex GEMM on MFMA f64: C[MxN] (+)= op(A)[MxK] . diag(kscale) . op(B)[KxN]
struct GemmArgs {
    const cplx* A; int lda; int opA;      // op: 0 = N, 1 = conjugate transpose
    const cplx* B; int ldb; int opB;
    cplx* C; int ldc;
    int M, N, K;
    const int* Kdev;            // if non-null: K = min(K, *Kdev * Kmul) read on the device
    int Kmul;
    const double* kscale;       // optional scale of the contraction index
    int kscale_invert;          // use 1/kscale
    const double* rowscale;     // optional epilogue: acc *= rowscale[i] * colscale[j] (either may be null: factor 1)
    const double* colscale;
    int accumulate;             // C += instead of C =
    int negate;                 // the product enters with a minus sign (C -= A B with accumulate)
    int sharedA, sharedB;       // operand is one matrix for all chains (not shifted by the chain stride)
    const int* a_kgather;       // opA == 0 only: column k of op(A) is column a_kgather[k] of A
    int b_lower;                // op(B) is lower triangular (entries with k < j are zero): the k loop of a column tile starts at its first column
    // split-K (skinny products with a long contraction index, e.g. Q_prev^H A_j of the block Gram-Schmidt QR: few output tiles, K = n):
    // ksplit > 1 slices of K are computed by separate workgroups into part[slice][N][M] and summed in a fixed order by a second kernel
    int ksplit; cplx* part;
    size_t part_count;          // capacity of part in complex numbers (0: eight slices of M x N, the round-3 contract)
    int tag;                    // 1: a product inside a factorisation (LU trailing update, triangular solve) -- same code, its own kernel
                                // name (template argument), so that profiles keep it apart from the model's n_g^3 products
    ColSrc csrc;                // with accumulate: the old value of C(i, j) is column j of this source instead of what C holds (C is only
                                // written: the first touch of a destination that a scaled / gathered copy used to fill).  Not with split-K
};
void launch_gemm(const Launch& lc, const GemmArgs& a);
// the same with the kernel path named: -1 what launch_gemm does, 0 the generic kernel, 1 the whole-tile kernel where the arguments
// allow it (kernels_gemm.hip, gemm_full_path).  Returns the path that ran (0 / 1).  Both paths give bit-identical C.
int launch_gemm_path(const Launch& lc, const GemmArgs& a, int path);
// the kernel shape launch_gemm picks for these arguments and nb chains: tile 32 or 64, ksplit slices of K (1: no split-K; only with
// 32 x 32 tiles), xcd 1: the XCD-grouped 1-D grid (nb a multiple of 8), 0: grid.z = chain
struct GemmPlan { int tile, ksplit, xcd; };
GemmPlan gemm_plan(const GemmArgs& a, int nb);
// G += X GrT^T, K = min(Kmax, *Kdev * Kmul): the delayed-update flush as a register-only read-modify-write stream.  X and GrT are
// n x K8 (K8 = K rounded up to a multiple of 8, columns K .. K8 - 1 zero), both with leading dimension ld
void launch_flush(const Launch& lc, const cplx* X, const cplx* GrT, int ld, cplx* G, int ldc, int n, int Kmax,
                  const int* Kdev, int Kmul, int tag = 0,     // G (n x n) += X GrT^T, K = min(Kmax, *Kdev * Kmul) (Kdev may be null); tag 1: own kernel name
                  const int* skip = nullptr);                 // skip (per chain, may be null): nothing is done for a chain whose *skip != 0

// one-sided Jacobi SVD, M = U diag(d) V^H, d descending.  work: A (n*n), V (n*n), norms(n), rank(n),
// flag (int).  Host-driven sweep loop with one flag read-back per sweep.  Returns sweeps used or <0.
struct SvdWork {
    cplx* A; cplx* V; double* norms; double* rnorms; int* rank; int* flagT;
    unsigned long long* flag; double* last_residual;
    unsigned long long* hflag;       // mapped pinned host memory: [0] sequence number, [1] residual bits
    unsigned long long* hslot_dev;   // device alias of hflag
    unsigned long long* seqctr;      // device-side publish counter
    unsigned long long* host_seq;    // host-side expectation
    const int* rounds; int nrounds; int nblk;   // tournament table [nrounds][nblk/2][2]
    hipGraphExec_t* sweep_graph;                // lazily captured: memset + all rounds of one Jacobi sweep
};
// optional timing hooks around each batch of back-to-back round launches (one Jacobi sweep)
struct SvdProfHooks { void (*begin)(void* user); void (*end)(void* user, int launches); void* user; };
int run_svd(const Launch& lc, int n, const cplx* M, int ldm, const double* colscale, const double* rowscale,
            cplx* U, double* d, cplx* Vt, const SvdWork& w, int max_sweeps, const SvdProfHooks* hooks = nullptr);
int svd_block_cols(int n);      // columns per block used by the Jacobi kernel for this n

// local updates
// diagonal entries and off-diagonal scale of e^{sign dtau V} at one site: (0,0) = (2,2) = c0, (1,1) = (3,3) = c1, off-diagonal entries
// carry xs (evMatrix, detsdwopdim.cpp:3187-3229; cd / cmd of :2003-2006).  idx = k N + site.
__device__ __forceinline__ void cdw_site_terms(const DevModel& dm, size_t idx, double sign, double c, double& c0, double& c1, double& xs) {
    if (dm.cdw_on) {
        const double cC = dm.cdwC[idx], sC = dm.cdwS[idx];
        c0 = c * cC - sign * sC; c1 = c * cC + sign * sC; xs *= cC;
    } else { c0 = c; c1 = c; }
}
void launch_cdw_terms(const Launch& lc, const DevModel& hm);      // cdwC / cdwS from cdwl, all slices
// cdw_mode 0: phi proposals (with the cdw terms in e^{dtau V} when cdw_on); 1: the cdwl pass (proposeNewCDWl, :4173-4182)
void launch_update_decide(const Launch& lc, const DevModel* dm, const DevModel& hm, DevUpdateState* us,
                          const double* uniforms, const cplx* G, cplx* W, int k, int first, int thermal, int cdw_pass = 0,
                          const cplx* Gwin = nullptr, int winP = 0,       // winP > 0: G entries from the window copy (k_update_window)
                          int proposal = 0, int adapt_what = 0, int reset_nd = 0);   // proposal: DQMC_PROPOSE_*; adapt_what: 0 box, 1 rotate, 2 scale (+ 4: adaptScaleVariance)
void launch_update_window(const Launch& lc, const DevModel& hm, DevUpdateState* us, const cplx* G, const cplx* X, const cplx* GrT,
                          cplx* Gw, int P);
void launch_update_gather(const Launch& lc, const DevModel& hm, const DevUpdateState* us, const cplx* G,
                          const cplx* W, cplx* X, cplx* GrT, int skip_done = 0);     // skip_done: nothing for a chain whose slice_done is set
// nw = cur[off ..) followed by tail[0 .. off) per chain, `need` values; cursor of the window back to 0 (off: [nb], host-pinned)
void launch_advance_uniforms(const Launch& lc, DevUpdateState* us, const double* cur, const double* tail, double* nw,
                             const unsigned long long* off, size_t need);

// Hubbard replica (kernels_hubbard.hip)
void launch_hubbard_vscale(const Launch& lc, const DevModel& hm, int side, int inverse, int k, cplx* A, int lda);
void launch_hubbard_slice(const Launch& lc, const DevModel& hm, DevUpdateState* us, const double* uniforms, cplx* G, int k,
                          double e_m2a, double e_p2a);
void launch_hubbard_measure(const Launch& lc, const DevModel& hm, const cplx* G, double* acc);
// Correlators of the Hubbard replica (dqmc_hubbard_* in dqmc_hip.h).  Channels of the equal-time block count, [HUB_EQ_CH][N]: greenUp,
// greenDn, charge, spinZZ, spinXX, pairS, pairSx, pairD; of the time-displaced block count[n-1], [n-1][HUB_TD_CH][N]: the first six.
// launch_hubbard_corr_prep fills the scratch sc (hubbard_corr_scratch_doubles per chain) both walks read: the spin blocks of T transposed,
// with S != nullptr the two stencilled forms of its down block, and the occupations of the tau side (from Gt) and the 0 side (from G0).
// Equal time: (T, S, Gt, G0) = (G, G, G, G); time-displaced: (G(0,tau), nullptr, G(tau), G(0)), then the walk over G(tau,0).
// sc and acc may live outside the arena: chain b at (char*)sc + b * scs, (char*)acc + b * acs
#define HUB_EQ_CH 8
#define HUB_TD_CH 6
size_t hubbard_corr_scratch_doubles(int N);
size_t hubbard_eq_doubles(int N);
size_t hubbard_td_doubles(int N, int n);
void launch_hubbard_corr_prep(const Launch& lc, const DevModel& hm, const cplx* T, const cplx* S, const cplx* Gt, const cplx* G0, double* sc,
                              size_t scs);
void launch_hubbard_eq_corr(const Launch& lc, const DevModel& hm, const cplx* G, const double* sc, size_t scs, double* acc, size_t acs);
void launch_hubbard_td_corr(const Launch& lc, const DevModel& hm, const cplx* GT0, const double* sc, size_t scs, double* acc, size_t acs,
                            int row, int rows);
// Every-slice block of the Hubbard replica (DQMC_TD_HUB_EVERY_SLICE): count[m+1], [m+1][HUB_EQ_CH][N].  launch_hubbard_td_fine_corr is the
// walk over G(tau,0) with all eight channels; its scratch comes from launch_hubbard_corr_prep(T = G(0,tau), S = G(tau,0), G(tau), G(0)).
// launch_hubbard_td_matsubara: the transforms of that block (inside the arena), out[chain][HUB_EQ_CH][nfreq][N] (re, im), bad[chain] = 1 for
// a chain with a row that was never measured; out and bad are plain device arrays.  false, nothing launched: the lattice is too large for the LDS
size_t hubbard_td_fine_doubles(int N, int m);
void launch_hubbard_td_fine_corr(const Launch& lc, const DevModel& hm, const cplx* GT0, const double* sc, size_t scs, double* acc, size_t acs,
                                 int row, int rows);
bool launch_hubbard_td_matsubara(const Launch& lc, const DevModel& hm, const double* acc, int nfreq, double* out, double* bad);

// misc elementwise
void launch_cosh_sinh(const Launch& lc, const DevModel& hm);
void launch_set_identity(const Launch& lc, cplx* A, int n);
void launch_conj_transpose(const Launch& lc, const cplx* A, cplx* B, int n);
void launch_add_diag(const Launch& lc, cplx* A, const double* d, int n);
void launch_copy(const Launch& lc, const cplx* A, cplx* B, size_t count);
void launch_copy_bytes(const Launch& lc, const void* src, void* dst, size_t bytes);   // same buffer of every chain
void launch_phi_sq_sum(const Launch& lc, const DevModel& hm, double* out);
void launch_gather_scalars(const Launch& lc, const double* src, double factor, double* dst);      // dst[b] = factor * src of chain b (dst: plain device array)
void launch_phi_action(const Launch& lc, const DevModel& hm, const DevUpdateState* us, double* out);
void launch_phi_shift(const Launch& lc, const DevModel& hm, const double* shifts /* shared buffer [nchains][opdim] */);
// fermionic observables of one time slice accumulated from the shifted Green's function gs (kernels_measure.hip)
// acc layout (doubles): [0] sum Re gs, [1] Re tr gs, [2] occDiffSq sum, [3] slices, then pairPlus[N], pairMinus[N],
// SX[(2L-1)^2] (re, im), SY[(2L-1)^2] (re, im)
void launch_measure_accum(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc);
size_t measure_accum_doubles(int N, int L);
// time-displaced block: count[n-1], then per boundary j = 1 .. n-1 the S_X / S_Y bins of the shifted G(tau_j, 0) (dqmc_hip.h)
// (row, rows): the block holds count[rows], then row `row` at offset rows + row * stride -- (j - 1, n - 1) for the coarse blocks,
// (k, m + 1) for the every-slice blocks; the same for the three launchers below
void launch_measure_td(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, int row, int rows);
size_t measure_td_row_doubles(int channel, int N, int L);   // stride of a row: channel 0 bins, 1 pairing, 2 particle-hole, 3 current, 4 band (5: measure_custom_row_doubles)
// every-slice end rows: (G, G - 1) -> (a_t0, a_0t), (1 - G, -G) -> (b_t0, b_0t), G -> gtt; one elementwise pass, all chains
void launch_td_ends(const Launch& lc, const cplx* G, cplx* a_t0, cplx* a_0t, cplx* b_t0, cplx* b_0t, cplx* gtt, int ng);
size_t measure_td_doubles(int L, int n);
// Matsubara transforms of the every-slice block `acc` of `channel` (count[m+1], then the rows): out[chain][component][nfreq][N] (re, im),
// bad[chain] = 1 if a row of the chain was never measured; out and bad are plain device arrays (no chain stride).  false: the lattice
// is too large for the kernel's LDS, nothing was launched.  out_chain_stride (doubles) != 0: chain b's results at out + b * stride.
// Channels 5 and 6 (user-defined bilinears, pair operators): custom_count components per row, and the block lives outside the arena, chain b at
// (char*)acc + b * custom_chain_bytes
bool launch_td_matsubara(const Launch& lc, const DevModel& hm, const double* acc, int channel, int nfreq, int apbx, int apby,
                         double* out, double* bad, size_t out_chain_stride = 0, int custom_count = 0, size_t custom_chain_bytes = 0);
bool td_matsubara_fits(const DevModel& hm, int channel, int nfreq);     // what launch_td_matsubara would return, nothing launched
// measurement series (dqmc_series_*): sample / open / closed / bad are plain device arrays, chain b of an [nb][S] array at b * S
bool launch_series_eq_sample(const Launch& lc, const DevModel& hm, const double* eqacc, size_t eq_n, int nch, const double* trig, double* sample,
                             size_t S, size_t off, double* bad);     // nch channels of the block count, X[nch][N] -> C_X [nch][N], S_X [nch][N]
void launch_series_band_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, double* value, double* err);
void launch_series_custom_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, int count, int qx, int qy,
                                  double* value, double* err);      // value, err [nb][count]: R of every user-defined bilinear at Q = (qx, qy)
size_t series_eq_sample_lds_bytes(int L);
#ifdef __HIPCC__
// The separable cosine sum of the sample kernels (k_series_eq_sample, k_hubbard_series_td_sample): out[qy L + qx] = sum_d cos(q d) C(d) for
// C [N] in LDS, in the order of the host's finishFermionic -- over dx into (Ac, As)[dy][qx], then over dy -- with the phase index reduced
// mod L in integers and (ct, st) = cos / sin(2 pi j / L).  Called by all 256 threads of a workgroup after a barrier behind the writes
// of C, ct and st; Ac and As are N doubles of LDS scratch each.
__device__ __forceinline__ void series_cosine_sum(const double* C, double* Ac, double* As, const double* ct, const double* st, double* __restrict__ out,
                                                  int L, int tid) {
    const int N = L * L;
    for (int i = tid; i < N; i += 256) {
        const int dy = i / L, qx = i - dy * L;
        double sc = 0.0, ss = 0.0;
        for (int dx = 0; dx < L; ++dx) {
            const double v = C[dy * L + dx];
            const int j = (qx * dx) % L;
            sc += ct[j] * v; ss += st[j] * v;
        }
        Ac[i] = sc; As[i] = ss;
    }
    __syncthreads();
    for (int q = tid; q < N; q += 256) {
        const int qy = q / L, qx = q - qy * L;
        double sq = 0.0;
        for (int dy = 0; dy < L; ++dy) {
            const int j = (qy * dy) % L;
            sq += ct[j] * Ac[dy * L + qx] - st[j] * As[dy * L + qx];
        }
        out[q] = sq;
    }
}
#endif
// The Matsubara kernels (k_td_matsubara in kernels_measure.hip, k_hubbard_td_matsubara in kernels_hubbard.hip): a tile of at most TDM_FT
// frequencies per workgroup, the shape both are launched with, the LDS a tile needs (doubles) and the separable spatial transform.
#define TDM_FT 8
struct TdmShape { int channel, ncomp, nfreq, ftile, m, L, N, W, WP, rlen, stride, apbx, apby; double scale; size_t ocs; };   // ocs: chain stride of out (doubles)
size_t measure_td_matsubara_lds_doubles(int ftile, int m, int L, int W, int rlen);
#ifdef __HIPCC__
// T[ky][ix] = sum_iy ty[ky][iy] U[iy][ix], then emit(ky L + kx, sum_ix tx[kx][ix] T[ky][ix]); U = (ur, ui)[(iy W + ix) str]
template<class Emit>
__device__ __forceinline__ void tdm_dft2(const TdmShape& a, const double* tx, const double* ty, double* T, const double* ur, const double* ui,
                                         int str, Emit emit) {
    const int L = a.L, W = a.W, WP = a.WP;
    for (int i = threadIdx.x; i < L * W; i += 256) {
        const int ky = i / W, ix = i - ky * W;
        const double* t = ty + (size_t)2 * ky * WP;
        double re = 0.0, im = 0.0;
        for (int iy = 0; iy < W; ++iy) {
            const double c = t[2 * iy], s = t[2 * iy + 1], xr = ur[(size_t)(iy * W + ix) * str], xi = ui[(size_t)(iy * W + ix) * str];
            re += c * xr - s * xi;
            im += c * xi + s * xr;
        }
        T[2 * i] = re; T[2 * i + 1] = im;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < a.N; q += 256) {
        const int ky = q / L, kx = q - ky * L;
        const double* t = tx + (size_t)2 * kx * WP;
        const double* v = T + (size_t)2 * ky * W;
        double re = 0.0, im = 0.0;
        for (int ix = 0; ix < W; ++ix) {
            const double c = t[2 * ix], s = t[2 * ix + 1];
            re += c * v[2 * ix] - s * v[2 * ix + 1];
            im += c * v[2 * ix + 1] + s * v[2 * ix];
        }
        emit(q, re, im);
    }
    __syncthreads();                                        // T is free again
}
#endif
// the parts of a Hubbard context (DQMC_SERIES_HUB_*; kernels_hubbard.hip, the derived quantities in kernels_measure.hip).  slice / td: the
// blocks ACC_SLICE and ACC_HUB_TD inside the arena (chain stride lc.cs); t, U, mu: the parameters the eight scalars are formed with.
// launch_hubbard_series_td_sample returns false, with nothing launched, for a lattice beyond the sample kernels' LDS
void launch_hubbard_series_scalars(const Launch& lc, const DevModel& hm, const double* slice, double t, double U, double mu, double* sample, size_t S,
                                   size_t off, double* bad);
bool launch_hubbard_series_td_sample(const Launch& lc, const DevModel& hm, const double* td, const double* trig, double* sample, size_t S, size_t off,
                                     double* bad);
void launch_series_hubbard_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, size_t off, int qx, int qy,
                                   double* value, double* err);      // value, err [nb][19] (dqmc_series_hubbard_derived_host)
void launch_series_accum(const Launch& lc, const double* sample, double* open, double* closed, size_t n, int close, int bin_size);
void launch_series_accum_routed(const Launch& lc, const double* const* src, double* open, double* closed, size_t S, int close, int bin_size);
void launch_series_stats(const Launch& lc, const double* bins, size_t n, int B, double* mean, double* err);
void launch_series_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, int nfreq, long long off_eq,
                           long long off_cur, double* value, double* err);
// the order-parameter part (DQMC_SERIES_PHI): chi [nfreq][N] and five scalars from the field; trig = (cos, sin)(2 pi j / L) [2 L], ttab =
// (cos, sin)(2 pi j / m) [2 m].  series_phi_sample_fgroup: frequencies per workgroup, 0 if a single frequency does not fit the LDS
bool launch_series_phi_sample(const Launch& lc, const DevModel& hm, const double* trig, const double* ttab, int nfreq, double* sample,
                              size_t S, size_t off);
int series_phi_sample_fgroup(int L, int m, int nfreq);
hipError_t series_phi_sample_prepare();                     // the kernel's dynamic LDS limit, set by dqmc_series_begin on the series' device
void launch_series_phi_derived(const Launch& lc, const DevModel& hm, const double* bins, size_t S, int B, int nfreq, size_t off,
                               double* value, double* err);
// long runs: in-place merge of neighbouring closed bins (half = pairs to merge), Welford's update of (w, m2) [nb][S] with the sample rows
// (src == nullptr: the rows of `sample` in order; cnt = samples including this one), and the binning analysis err / tau [levels][n]
// (tau == nullptr: errors only; m2 is read only with tau)
void launch_series_rebin(const Launch& lc, double* bins, size_t n, int half);
void launch_series_welford(const Launch& lc, const double* sample, const double* const* src, double* w, double* m2, size_t S, long long cnt);
void launch_series_binning(const Launch& lc, const double* bins, const double* m2, size_t n, int B, int levels, int bin_size,
                           long long samples, double* err, double* tau);
// time-displaced pairing block: count[n-1], then per boundary j = 1 .. n-1 the sums over B of Re T+(B (+) d, B) [N] and Re T-(B (+) d, B) [N]
void launch_measure_td_pair(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, int row, int rows);
size_t measure_td_pair_doubles(int N, int n);
// time-displaced particle-hole block: count[n-1], then per boundary j = 1 .. n-1 the sums over B of Re W(B (+) d, B) for charge [N], spinZ [N], sdw [N].
// gs = shifted G(tau_j, 0), hs = (shifted G(0, tau_j))^H, ob = the one-body values [2][5][N] that launch_td_ph_onebody wrote from the
// shifted equal-time matrices (t = 0: G(tau_j), t = 1: G(0))
void launch_td_ph_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, int t);
void launch_measure_td_ph(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* ob, double* acc, int row, int rows);
size_t measure_td_ph_doubles(int N, int n);
size_t measure_td_ph_onebody_cplx(int N);
// equal-time two-particle block (dqmc_set_equal_time_correlators): count, then the sums over B of Re W(B (+) d, B) for charge [N], spinZ [N],
// sdw [N] and of Re T+-(B (+) d, B) for pairPlus [N], pairMinus [N], all from the one shifted matrix gs.  acc and the one-body scratch ob
// are plain device arrays outside the arena: chain b at acc + b * measure_eq_doubles(N) and ob + b * measure_eq_onebody_cplx(N)
void launch_measure_eq_corr(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, double* acc);
size_t measure_eq_doubles(int N);
size_t measure_eq_onebody_cplx(int N);
// time-displaced current-current block: count[n-1], then per boundary j = 1 .. n-1 the sums over B of Re W[j_mu(B (+) d), j_mu(B)] for mu = x [N]
// and mu = y [N], then sum_A Re o_tau[k_x(A)] and sum_A Re o_tau[k_y(A)].  bt = bond amplitudes [2][MSF][N] (shared by all chains),
// ob = the one-body values [2][4][N] (j_x, j_y, k_x, k_y) that launch_td_current_onebody wrote; gs, hs as for launch_measure_td_ph
void launch_td_current_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* bt, cplx* ob, int t);
void launch_measure_td_current(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* bt, const cplx* ob, double* acc, int row, int rows);
size_t measure_td_current_doubles(int N, int n);
size_t measure_td_current_onebody_cplx(int N);
size_t measure_td_current_bond_cplx(int N, int opdim);
// band-resolved charge blocks (DQMC_TD_PH_BAND, dqmc_set_equal_time_band): the sums over B of Re W(B (+) d, B) for bandDiff [N] and bandMix [N].
// Time-displaced: count[n-1], then the rows; gs, hs as for launch_measure_td_ph, ob = the one-body values [2][2][N] of launch_td_band_onebody.
// Equal-time: count, bandDiff[N], bandMix[N] from the one shifted matrix gs; acc and the scratch ob [3][N] are plain device arrays outside
// the arena, chain b at acc + b * measure_eq_band_doubles(N) and ob + b * measure_eq_band_onebody_cplx(N)
void launch_td_band_onebody(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, int t);
void launch_measure_td_band(const Launch& lc, const DevModel& hm, const cplx* gs, const cplx* hs, const cplx* ob, double* acc, int row, int rows);
size_t measure_td_band_doubles(int N, int n);
size_t measure_td_band_onebody_cplx(int N);
void launch_measure_eq_band(const Launch& lc, const DevModel& hm, const cplx* gs, cplx* ob, double* acc);
size_t measure_eq_band_doubles(int N);
size_t measure_eq_band_onebody_cplx(int N);
// user-defined bilinears (dqmc_set_custom_bilinears): count matrices M [count][4][4] (row-major, host memory: they travel as a kernel argument)
// with their non-zero masks (bit 4 a + b: M_ab != 0), every channel in one launch; a row holds the channels' sums over B of Re W(B (+) d, B),
// [count][N].  Time-displaced: count[rows], then the rows; gs, hs as for launch_measure_td_ph.  Equal-time: count, then one row; M2, mask2 =
// the squares of the matrices (the delta term).  acc and the scratch ob are plain device arrays outside the arena: chain b at acc + b * acs
// (equal-time: 1 + measure_custom_row_doubles) and ob + b * measure_*_custom_onebody_cplx
// Bond parts (dqmc_set_custom_bond_bilinears): with bond != nullptr the three entries launch the stencil kernels instead, for every set
// operator.  Device table tab (measure_custom_bond_table_cplx complex, shared by the chains): the five site blocks of every operator,
// V[count][5][4][4] = M0, Mx, Mx^H, My, My^H, then the link factors u[2][N] of the stored sector (x bonds, y bonds); mk[count][5] the
// non-zero masks of the blocks (device memory as well: the kernels index both by a loop variable); parts[c] bit k: block k of operator c
// is non-zero -- the launch argument that lets on-site-only operators skip the bond block pairs.
struct CustomBond { const cplx* tab; const unsigned* mk; unsigned parts[DQMC_CUSTOM_MAX]; };
size_t measure_custom_bond_table_cplx(int count, int N);
void launch_td_custom_onebody(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* gs, cplx* ob, int t,
                              const CustomBond* bond = nullptr);
void launch_measure_td_custom(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* gs, const cplx* hs,
                              const cplx* ob, double* acc, size_t acs, int row, int rows, const CustomBond* bond = nullptr);
void launch_measure_eq_custom(const Launch& lc, const DevModel& hm, int count, const cplx* M, const unsigned* mask, const cplx* M2, const unsigned* mask2,
                              const cplx* gs, cplx* ob, double* acc, const CustomBond* bond = nullptr);
// user-defined pair operators (dqmc_set_custom_pair_operators): row `row` of `rows` of a block count[rows], then rows [count][N], from ONE
// shifted matrix gs -- g~(tau,0) for the time-displaced blocks, g~ of the slice with (row, rows) = (0, 1) for the equal-time block.  Fa
// [count][4][4] = F0 - F0^T with its non-zero masks (host memory, a kernel argument) serves the on-site kernel; with pair != nullptr the
// stencil kernel runs instead, for every set operator.  Device table tab (measure_custom_pair_table_cplx complex, shared by the
// chains): V[count][3 blocks 0, x, y][3 forms F, conj F, F^H][4][4], then the link signs u[2][N]; mk[count][3][2] the non-zero masks of
// F and of F^H; parts[c] bit k: block k of operator c is non-zero.  acc lives outside the arena: chain b at acc + b * acs
struct CustomPair { const cplx* tab; const unsigned* mk; unsigned parts[DQMC_CUSTOM_MAX]; };
size_t measure_custom_pair_table_cplx(int count, int N);
void launch_measure_custom_pair(const Launch& lc, const DevModel& hm, int count, const cplx* Fa, const unsigned* mask, const cplx* gs, double* acc,
                                size_t acs, int row, int rows, const CustomPair* pair = nullptr);
// the averaged Green's function block (dqmc_set_green_matrix): row `row` of `rows` of a block count[rows], then rows [N][R][R] (re, im), from
// the shifted g~(tau,0); sample part 13 of the series from the every-slice block; bubble and vertex of the pair operators from the closed
// bins (pair: the stencil table of every set operator; pb: nb (B + 1)(m + 1) count doubles of scratch; value, err [nb][count][5 + m])
size_t measure_green_matrix_row_doubles(int opdim, int N);
void launch_measure_green_matrix(const Launch& lc, const DevModel& hm, const cplx* gs, double* acc, size_t acs, int row, int rows, int apbx, int apby);
void launch_series_green_sample(const Launch& lc, const DevModel& hm, const double* fine, size_t chain_bytes, double* sample, size_t S, size_t off,
                                double* bad);
size_t series_pair_bubble_lds_bytes(int opdim, int N);
bool launch_series_pair_vertex(const Launch& lc, const DevModel& hm, const double* bins, const double* mean, const double* trig, size_t S, int B,
                               int nfreq, size_t off_chi, size_t off_g, int count, const CustomPair& pair, int qx, int qy, int apbx, int apby,
                               double* pb, double* value, double* err);
// particle-hole bubble and vertex of the user-defined bilinears from the closed bins (parts 9 and 13): bond: the stencil table of every set
// operator; pb: nb (B + 1)(m + 1) count doubles of scratch; value, err [nb][count][6 + m]
size_t series_ph_bubble_lds_bytes(int opdim, int N);
bool launch_series_ph_vertex(const Launch& lc, const DevModel& hm, const double* bins, const double* mean, const double* trig, size_t S, int B,
                             int nfreq, size_t off_chi, size_t off_g, int count, const CustomBond& bond, int qx, int qy, int apbx, int apby,
                             double* pb, double* value, double* err);
// wrap-error diagnostics (kernels_green_check.hip; dqmc_set_green_check): the six results of dqmc_hip.h for the wrapped Gw against the
// fresh Gf, both n x n at leading dimension ld, in two launches.  Gf is a per-chain buffer at the chain stride; Gw, the partials
// (green_diff_partial_doubles(n) doubles per chain) and out (6 doubles per chain: maxAbs, argmax, maxSiteDiag, sumAbs, maxFresh,
// nonfinite) have strides of their own, in bytes (the context keeps them outside the arena).  fold != nullptr: the finalise step also
// forms the log scale spreads of d and, unless null, sv (n values each, per-chain buffers at the chain stride) and folds the sample
// into row `row` of every chain's table
struct GreenCheckFold { double* table; size_t table_stride; int row; const double* d; const double* sv; };
size_t green_diff_partial_doubles(int n);
void launch_green_keep(const Launch& lc, const cplx* G, cplx* keep, size_t keep_stride, size_t count);   // keep[chain] = G of the chain
void launch_green_diff(const Launch& lc, const cplx* Gw, size_t gw_stride, const cplx* Gf, int n, int ld, int N, double* part,
                       size_t part_stride, double* out, size_t out_stride, const GreenCheckFold* fold = nullptr);
size_t measure_custom_row_doubles(int count, int N);
size_t measure_td_custom_onebody_cplx(int count, int N);
size_t measure_eq_custom_onebody_cplx(int count, int N);

// ---- QR / UDT building blocks (kernels_qr.hip) ------------------------------------------------
struct SvdProfHooks;
struct QrWork { cplx* V; cplx* T; cplx* W; cplx* W2; cplx* Rneg; const SvdProfHooks* apply_hooks; cplx* part; size_t part_count; int* err; };   // part: split-K scratch (n > 1024); err: per-chain failure flag of the Cholesky-QR panels (DevUpdateState::chol_fail)   // hooks: optional timing of the k_qr_apply launches
int run_qr(const Launch& lc, int n, cplx* A, cplx* Q, const QrWork& w);                 // A -> R in place, Q explicit (Q == nullptr: reflectors only)
int run_qr_apply_q(const Launch& lc, int n, cplx* C, const QrWork& w, int trans);
// large n: QR by block Gram-Schmidt with reorthogonalisation + Cholesky-QR2 panels, all on the GEMM kernel (kernels_qr.hip); Q is always explicit
int run_qr_bgs(const Launch& lc, int n, cplx* A, cplx* Q, const QrWork& w);
void qr_reset_workspace(const Launch& lc, int n, const QrWork& w);      // zero w.V / w.T before Householder panels follow a block Gram-Schmidt run
int run_trsm_right_upper(const Launch& lc, int n, const cplx* R, cplx* C, const QrWork& w, int trans = 0, int unit = 0,     // C <- C R^-1 (trans: R = (stored lower triangle)^H; unit: unit diagonal)
                         const ColSrc* src = nullptr);   // src: C <- S R^-1 with the right-hand side S read from the column source (ld n, not C itself); C is only written
// (the diagonal reciprocals are scale-safe, cplx_recip: a diagonal entry outside ~ [1e-154, 1e154] is no special case)
#define LU_SWAP_INTS 128
// pivot search and multipliers are scale-safe: LU of 2^k A has the pivots and L of A and U scaled by 2^k, also where |a|^2 leaves
// the normal range; NaN entries are never chosen as pivots
int run_lu(const Launch& lc, int n, cplx* A, int* perm, int* swaps, cplx* tneg);    // tneg: scratch of n * 32 complex per chain                                 // P A = L U in place (n <= 512, else -1), kernels_lu.hip
void launch_gather_scale_cols(const Launch& lc, const cplx* X, const double* cs, const int* perm, int n, cplx* Y);   // Y[:, j] = X[:, perm[j]] cs[perm[j]]
void launch_udt_init(const Launch& lc, const cplx* M, int ldm, const double* cs, const double* rs, const int* perm,
                     int transpose, cplx* W, int n);
void launch_udt_diag(const Launch& lc, const cplx* R, int n, double* d);
void launch_udt_lazy(const Launch& lc, const double* d, const int* perm, int n, double* dinv, int* perm_inv);   // 1/d and the inverse permutation
void launch_udt_tmat(const Launch& lc, const cplx* R, const double* d, const int* perm, int n, cplx* Tt);
void launch_permute_scale_cols(const Launch& lc, const cplx* X, const double* cs, const int* perm, int n, cplx* Y);
void launch_split_scales(const Launch& lc, const double* d, int n, double* dmax_inv, double* dmin);
void launch_logdet_vector(const Launch& lc, const cplx* R, const double* a, const double* b, int n, double* sv);
// column norms / ranks shared with the SVD path (kernels_svd.hip)
void launch_scaled_norms_rank(const Launch& lc, const cplx* M, int ldm, const double* cs, const double* rs, int transpose,
                              int n, double* norms, int* rank, double* scratch_d);
