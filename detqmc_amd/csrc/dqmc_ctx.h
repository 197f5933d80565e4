// Private to the two units of the C-ABI implementation (dqmc_context.hip: context, sweep building blocks; dqmc_measure_api.hip: measurement and
// series entry points): the context itself and the helpers every entry point is written with.
#pragma once
#include "dqmc_internal.h"
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#define DQMC_PRIVATE __attribute__((visibility("hidden")))     // shared by the two units, not part of the library's interface

extern DQMC_PRIVATE thread_local std::string g_err;     // the one definition: dqmc_context.hip
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                       \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess)                                                                           \
            return fail(DQMC_EHIP, std::string(#x) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                                       std::to_string(__LINE__) + ")");                                  \
    } while (0)

// DQMC_SYNC_CHECK=1 (debug mode): every entry point that only enqueues work waits for its stream before it returns and
// every kernel family scope waits when it closes, so an asynchronous GPU fault is reported by the call -- and the kernel
// family -- that caused it.  Without it the enqueue-only entry points see a fault whenever the runtime notices it, i.e.
// possibly one or more calls later (the message says so).  Results are identical either way.
static bool sync_check_on() {
    static const bool on = getenv("DQMC_SYNC_CHECK") && atoi(getenv("DQMC_SYNC_CHECK")) != 0;
    return on;
}

struct UdVSlot { cplx* U; double* d; cplx* Vt; };

enum { FAM_BMULT = DQMC_FAM_BMULT, FAM_GEMM = DQMC_FAM_GEMM, FAM_JACOBI = DQMC_FAM_DECOMP, FAM_UPDATE = DQMC_FAM_DECIDE,
       FAM_OTHER = DQMC_FAM_OTHER, FAM_GATHER = DQMC_FAM_GATHER, FAM_FLUSH = DQMC_FAM_FLUSH, FAM_ROUNDS = 7, FAM_COUNT = DQMC_FAM_COUNT };

// The measurement accumulator blocks of a context, one table (dqmc_ctx::acc): the per-slice observables, the four coarse time-displaced
// channels, the four every-slice ones (channel ch at ACC_FINE0 + ch, as ACC_TD + ch for the coarse ones) and the equal-time correlators;
// channel 4 of both families and ACC_EQ_BAND are the band-resolved charge blocks (DQMC_TD_PH_BAND, dqmc_set_equal_time_band), channel 5
// and ACC_EQ_CUSTOM the blocks of the user-defined bilinears (dqmc_set_custom_bilinears), channel 6 and ACC_EQ_CUSTOM_PAIR those of the
// user-defined pair operators (dqmc_set_custom_pair_operators), channel 7 the averaged Green's function block (dqmc_set_green_matrix);
// ACC_HUB_EQ / ACC_HUB_TD the equal-time and time-displaced correlators of the Hubbard model (dqmc_hubbard_*), behind every SDW block,
// ACC_HUB_TD_FINE its every-slice block (DQMC_TD_HUB_EVERY_SLICE)
enum { TD_CHANNELS = 8 };
enum { ACC_SLICE, ACC_TD, ACC_TD_PAIR, ACC_TD_PH, ACC_TD_CUR, ACC_TD_BAND, ACC_TD_CUSTOM, ACC_TD_CUSTOM_PAIR, ACC_TD_GREEN_MATRIX, ACC_FINE0,
       ACC_EQ = ACC_FINE0 + TD_CHANNELS, ACC_EQ_BAND, ACC_EQ_CUSTOM, ACC_EQ_CUSTOM_PAIR, ACC_HUB_EQ, ACC_HUB_TD, ACC_HUB_TD_FINE, ACC_COUNT };
// n: doubles per chain, 0 while the context has no such block; chain b starts at (char*)p + b * stride (the arena's chain stride; the
// equal-time blocks and every block of the user-defined bilinears and pair operators live outside the arena as [chain][n]); missing: what a read of an absent
// block reports
struct AccBlock { double* p; size_t n, stride; const char* missing; };

struct dqmc_ctx {
    dqmc_params p;
    DevModel hm;
    hipStream_t st = nullptr;
    // pipelined local updates (dqmc_update_slice): the flush of block b runs on st2 while the decisions of block b + 1 run on st
    hipStream_t st2 = nullptr;
    hipEvent_t ev_win = nullptr, ev_flush = nullptr;
    cplx* Gwin = nullptr;          // (MSF pbudget)^2: the next block's proposal window of G (k_update_window)
    int pipe_P = 0;                // pbudget when the pipelined schedule is in effect, else 0
    bool pipelined = false;        // latched at dqmc_create (dqmc_tuning::pipeline, n_g, chains): nothing else decides the schedule
    uint64_t blocks_pipelined = 0, blocks_sequential = 0, cholqr_fallbacks = 0;
    bool qr_bgs = false, green_lu = false;       // latched at dqmc_create (dqmc_tuning::qr_variant / green_variant)
    std::vector<int> err_host;     // scratch of chol_failed()
    // batched chains: nb chains in lockstep; per-chain buffers of chain b = chain 0's + b * cs (one arena)
    Launch lc{nullptr, 1, 0};
    int nb = 1, sel = 0;                // sel: chain the host-buffer entry points talk to (dqmc_select_chain)
    char* arena = nullptr;
    size_t arena_off = 0;
    std::vector<void**> fixups;
    int n_g = 0, MSF = 0, N = 0, m = 0, s = 0, n = 0, D = 0;
    std::vector<void*> allocs;
    // fields + backups
    double *phi = nullptr, *coshT = nullptr, *sinhT = nullptr;
    double *cdwl = nullptr, *cdwC = nullptr, *cdwS = nullptr;      // cdwU != 0 only
    double *phi_bak = nullptr, *cosh_bak = nullptr, *sinh_bak = nullptr;
    // Green's function, singular values of G^-1
    cplx *G = nullptr, *G_bak = nullptr;
    double *sv = nullptr, *sv_bak = nullptr;
    std::vector<UdVSlot> storage, storage_bak;
    UdVSlot spare{}, tmpudv{};
    cplx *T1 = nullptr, *T2 = nullptr, *T3 = nullptr, *T4 = nullptr;
    cplx *propK[2] = {nullptr, nullptr}, *Tdense = nullptr;   // CB_NONE only: blockdiag e^{-+dtau K} (n_g x n_g), GEMM target
    cplx *propKh[2] = {nullptr, nullptr};                    // CB_NONE only: e^{-+dtau K / 2} (propK_half, propK_half_inv)
    AccBlock acc[ACC_COUNT] = {
        {nullptr, 0, 0, "the context has no measurement accumulators"},                       // every context has them
        {nullptr, 0, 0, "context created without dqmc_params::timedisplaced"},
        {nullptr, 0, 0, "context created without dqmc_params::timedisplaced == 2"},
        {nullptr, 0, 0, "context created without dqmc_params::td_particle_hole"},
        {nullptr, 0, 0, "context created without dqmc_params::td_particle_hole = 2"},
        {nullptr, 0, 0, "context created without DQMC_TD_PH_BAND"},
        {nullptr, 0, 0, "no user-defined bilinear is set (dqmc_set_custom_bilinears), or the context was created without dqmc_params::td_particle_hole"},
        {nullptr, 0, 0, "no user-defined pair operator is set (dqmc_set_custom_pair_operators), or the context was created without dqmc_params::timedisplaced"},
        {nullptr, 0, 0, "the averaged Green's function block is switched off (dqmc_set_green_matrix)"},
        {nullptr, 0, 0, "no every-slice block for this channel"}, {nullptr, 0, 0, "no every-slice block for this channel"},
        {nullptr, 0, 0, "no every-slice block for this channel"}, {nullptr, 0, 0, "no every-slice block for this channel"},
        {nullptr, 0, 0, "no every-slice block for this channel"}, {nullptr, 0, 0, "no every-slice block for this channel"},
        {nullptr, 0, 0, "no every-slice block for this channel"}, {nullptr, 0, 0, "no every-slice block for this channel"},
        {nullptr, 0, 0, "the equal-time correlators have never been enabled (dqmc_set_equal_time_correlators)"},
        {nullptr, 0, 0, "the equal-time band correlators have never been enabled (dqmc_set_equal_time_band)"},
        {nullptr, 0, 0, "no user-defined bilinear is set (dqmc_set_custom_bilinears)"},
        {nullptr, 0, 0, "no user-defined pair operator is set (dqmc_set_custom_pair_operators)"},
        {nullptr, 0, 0, "the Hubbard equal-time correlators have never been enabled (dqmc_hubbard_set_equal_time_correlators)"},
        {nullptr, 0, 0, "Hubbard context created without dqmc_params::timedisplaced = 1 and td_particle_hole = 1"},
        {nullptr, 0, 0, "Hubbard context created without DQMC_TD_HUB_EVERY_SLICE"}};
    // time-displaced Green's functions (dqmc_params::timedisplaced reserves them; dqmc_set_timedisplaced switches them on)
    bool td_reserved = false, td_on = false;
    int td_slice = -1;                                        // tau slice of the last pair GT0 / G0T (all chains), -1: none yet
    cplx *GT0 = nullptr, *G0T = nullptr, *td_W = nullptr;     // G(tau,0), G(0,tau), scratch of the extra solves
    double* td_sv = nullptr;                                  // SVD mode: log-det output of the LU / QR route (c->sv keeps the Jacobi values)
    // dqmc_params::td_particle_hole: G(0) of the boundary's own field configuration, (shifted G(0,tau))^H, one-body values
    cplx *G00 = nullptr, *ph_H = nullptr, *ph_ob = nullptr;
    // td_particle_hole == 2: bond amplitudes (shared by the chains) and one-body values of the current-current correlators
    cplx *cur_bt = nullptr, *cur_ob = nullptr;
    // DQMC_TD_PH_BAND: one-body values [2][2][N] of the band-resolved charge channels
    cplx *band_ob = nullptr;
    // DQMC_TD_EVERY_SLICE: work copies of G(tau_k,0), G(0,tau_k), G(tau_k) that the segment / ends entries propagate (the sweep's own G,
    // GT0, G0T, G00 are only read) and the slice they stand on; one fine accumulator block (m + 1 rows) per enabled channel: 0 G(k, tau)
    // bins, 1 pairing, 2 particle-hole, 3 current.  DQMC_TD_HUB_EVERY_SLICE: the same work copies and the one block ACC_HUB_TD_FINE
    bool td_fine = false;
    int fine_slice = -1;
    cplx *fGT0 = nullptr, *fG0T = nullptr, *fGTT = nullptr;
    double* mats_out = nullptr;                               // dqmc_measure_td_matsubara_host: results + one flag per chain, outside the arena,
    size_t mats_cap = 0;                                      // allocated on first use and grown on demand (doubles)
    // dqmc_set_equal_time_correlators: block [chain][1 + 5 N] and one-body scratch [chain][5 N], outside the arena, allocated by the first enable
    bool eq_on = false;
    cplx* eq_ob = nullptr;
    // dqmc_hubbard_set_equal_time_correlators: block ACC_HUB_EQ [chain][1 + 8 N] and the scratch of the prepare pass [chain][4 N^2 + 4 N], outside
    // the arena, allocated by the first enable.  The time-displaced block ACC_HUB_TD lives in the arena; its prepare pass writes into ph_H
    bool hub_eq_on = false;
    double* hub_eq_sc = nullptr;
    // dqmc_set_equal_time_band: block [chain][1 + 2 N] and one-body scratch [chain][3 N], outside the arena, allocated by the first enable
    bool eqb_on = false;
    cplx* eqb_ob = nullptr;
    // dqmc_set_custom_bilinears: the matrices [count][4][4], their squares (the equal-time delta term) and the non-zero masks of both, on the
    // host -- they travel to the kernels as a launch argument; the blocks ACC_TD_CUSTOM [chain][(n-1)(1 + count N)] and ACC_EQ_CUSTOM
    // [chain][1 + count N] and the one-body scratch of the two forms, outside the arena, allocated by the call and freed by the next one
    int cst_count = 0;
    cplx cst_M[DQMC_CUSTOM_MAX * 16] = {}, cst_M2[DQMC_CUSTOM_MAX * 16] = {};
    unsigned cst_mask[DQMC_CUSTOM_MAX] = {}, cst_mask2[DQMC_CUSTOM_MAX] = {};
    bool eqc_on = false;
    cplx *cst_td_ob = nullptr, *cst_eq_ob = nullptr;
    // dqmc_set_custom_bond_bilinears: the bond parts on the host (for the getter), and while at least one is non-zero (cst_bond_on) the
    // device table and masks the stencil kernels read (CustomBond in dqmc_internal.h), allocated and freed with the blocks above
    cplx cst_Mx[DQMC_CUSTOM_MAX * 16] = {}, cst_My[DQMC_CUSTOM_MAX * 16] = {};
    bool cst_bond_on = false;
    CustomBond cst_bond = {};
    // dqmc_set_custom_pair_operators: the operators (F0, Fx, Fy) [count][4][4] on the host (for the getter), Fa = F0 - F0^T with its
    // non-zero masks (the on-site kernel's launch argument), and while an operator has a bond part (cpr_bond_on) the device table of the
    // stencil kernel (CustomPair in dqmc_internal.h); the blocks ACC_TD_CUSTOM_PAIR [chain][(n-1)(1 + count N)], its every-slice twin
    // and ACC_EQ_CUSTOM_PAIR [chain][1 + count N], outside the arena, allocated by the call and freed by the next one.  Independent of
    // the user-defined bilinears above
    int cpr_count = 0;
    cplx cpr_F0[DQMC_CUSTOM_MAX * 16] = {}, cpr_Fx[DQMC_CUSTOM_MAX * 16] = {}, cpr_Fy[DQMC_CUSTOM_MAX * 16] = {}, cpr_Fa[DQMC_CUSTOM_MAX * 16] = {};
    unsigned cpr_mask[DQMC_CUSTOM_MAX] = {};
    bool eqp_on = false, cpr_bond_on = false;
    CustomPair cpr_bond = {};
    // dqmc_set_green_matrix: while on, the blocks ACC_TD_GREEN_MATRIX [chain][(n-1)(1 + 2 R^2 N)] and its every-slice twin (channel 7),
    // outside the arena, allocated by the switch-on and freed by the switch-off
    bool gm_on = false;
    // dqmc_series_*: the measurement series.  Device buffers outside the arena, allocated by dqmc_series_begin and freed by dqmc_series_end
    // or with the context: sample [nb][S], open bin [nb][S], closed bins [max_bins][nb][S], the per-part flags [SERIES_AUX_ROWS][nb], the cos /
    // sin table (2 pi j / L [2 L]; with the order-parameter part, index 6 of off / len, also 2 pi j / m [2 m] behind it) and the result buffer
    // of the statistics calls (mean, err [nb][S] each, then SERIES_AUX_ROWS rows [nb] for the derived calls: value, err [nb][6] each, or
    // [nb][19] each for a Hubbard context).  The counters live on the host.
    // srctab [nb]: the source rows of dqmc_series_accumulate, filled from srchost before every launch; formed: the sample buffer holds
    // the sample of a successful dqmc_series_form_sample that no dqmc_series_accumulate has consumed yet.
    enum { SERIES_AUX_ROWS = 38 };                            // 2 x 19: value and err of dqmc_series_hubbard_derived_host, the largest user
    struct Series {
        bool open = false, formed = false;
        int bin_size = 0, max_bins = 0, nfreq = 0, parts = 0, closed = 0, in_open = 0;
        int flags = 0;                                        // DQMC_SERIES_AUTO_REBIN | DQMC_SERIES_TRACK_VARIANCE (dqmc_series_configure)
        long long samples = 0, rebins = 0;                    // accumulates since begin / merges of neighbouring bins so far
        size_t S = 0, off[17] = {}, len[17] = {};              // index = bit number; 5 is never used; 14 .. 16: a Hubbard context's parts
        double *sample = nullptr, *openbin = nullptr, *bins = nullptr, *bad = nullptr, *trig = nullptr, *stat = nullptr;
        double *var = nullptr;                                // running mean w [nb][S], then m2 [nb][S]: allocated with TRACK_VARIANCE
        double *binning = nullptr;                            // result of dqmc_series_binning_host, err then tau [levels][nb][S] each,
        size_t binning_cap = 0;                               // allocated on first use and grown on demand (doubles)
        double *vertex = nullptr;                             // dqmc_series_pair_vertex_host: the per-row bubbles and the results;
        size_t vertex_cap = 0;                                // allocated on first use and grown on demand (doubles)
        void *vertex_tab = nullptr;                           // ... its operator table and masks while no operator has a bond part (else
        CustomPair vertex_pair = {};                          // the measurement kernels' table serves): built by the first call
        void *ph_tab = nullptr;                               // dqmc_series_ph_vertex_host (it shares the buffer `vertex`): the same for
        CustomBond ph_bond = {};                              // the bilinears while none has a bond part
        const double** srctab = nullptr;
        std::vector<const double*> srchost;
    } ser;
    SvdWork sw{};
    double hub_e_m2a = 1.0, hub_e_p2a = 1.0;  // Hubbard: exp(-+2 alpha) of weightRatioSingleFlip (dethubbard.cpp:866-867)
    int stab = 0;                       // DQMC_STAB_SVD / DQMC_STAB_QR
    QrWork qw{};
    int* qr_perm = nullptr;
    int* lu_swaps = nullptr;
    cplx* lu_tneg = nullptr;       // -U12^T of the current LU panel (n_g x 32), operand of the trailing update on k_flush
    uint64_t lu_calls = 0;         // gather lists of the LU panels (kernels_lu.hip)
    int* qr_perm_inv = nullptr;      // inverse of qr_perm and 1/d of the last lazy UDT (triangular chaining product)
    double* qr_dinv = nullptr;
    double *rmax_inv = nullptr, *rmin = nullptr, *lmax_inv = nullptr, *lmin = nullptr;
    UdVSlot eye{};
    uint64_t qr_calls = 0;
    int max_jacobi_sweeps = 80;
    int last_svd_sweeps = 0;
    double last_svd_residual = 0.0;
    hipGraphExec_t jacobi_graph = nullptr;
    unsigned long long jacobi_host_seq = 0;
    uint64_t svd_calls = 0, svd_sweeps_total = 0;
    int svd_sweeps_max = 0;
    // updates
    cplx *X = nullptr, *Gr = nullptr, *W = nullptr;
    double* uniforms = nullptr;
    size_t uni_cap = 0;
    // look-ahead on the uniforms (dqmc_stage_uniforms_tail_host / dqmc_advance_uniforms): the window the next advance writes (it then
    // changes places with `uniforms`), the draws behind the current window, the pinned staging buffer (room for [nb][uni_cap]) with the offsets
    // [nb] of the advance behind it (allocated on first use), and the events that order upload and splice kernel
    double *uniforms_next = nullptr, *uni_tail = nullptr, *uni_pin = nullptr;
    unsigned long long* uni_off = nullptr;
    size_t uni_n = 0;                   // size of the current window of every chain, 0: not known (a single chain was pushed)
    bool tail_staged = false, tail_event_live = false, adv_event_live = false;
    hipStream_t st_up = nullptr;        // the upload's stream: st2 unless the pipelined schedule uses that one
    hipEvent_t ev_tail = nullptr, ev_adv = nullptr;
    uint64_t windows_advanced = 0, windows_pushed = 0;
    DevUpdateState* us = nullptr;
    double* scalar_out = nullptr;
    double* shift_buf = nullptr;        // [nchains][opdim] displacements of a global shift move (shared buffer)
    int currentTimeslice = 0;
    bool g_stale = false;          // dqmc_wrap_skip moved currentTimeslice without computing G: nothing may read G until it is rebuilt
    // dqmc_set_green_check: while on, the wrapped G every advance keeps [chain][n_g^2], the compare kernel's partials and results and
    // the table [chain][2][n+1][DQMC_GREEN_CHECK_FIELDS], outside the arena, allocated by the switch-on and freed by the switch-off
    bool gc_on = false;
    cplx* gc_keep = nullptr;
    double *gc_part = nullptr, *gc_out = nullptr, *gc_table = nullptr;
    // profiling
    bool prof = false;
    int prof_depth = 0;                 // open ProfScopes (they nest)
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, int>> ev_open;   // (family, index of begin event); end = index+1
    size_t ev_used = 0;
    double fam_ms[FAM_COUNT] = {0};
    uint64_t fam_launches[FAM_COUNT] = {0};
    double gemm_flops = 0.0;
    SubProf subprof{};                  // hooks handed to the launchers through Launch::sub while profiling is on
    SvdProfHooks qr_apply_hooks{};      // and through QrWork::apply_hooks (timing of the k_qr_apply launches)
    std::vector<std::pair<int, int>> sub_open;      // (sub-family, begin event)
    double sub_ms[SUBFAM_COUNT] = {0}, sub_flops[SUBFAM_COUNT] = {0}, sub_bytes[SUBFAM_COUNT] = {0};
    uint64_t sub_launches[SUBFAM_COUNT] = {0};
    std::string fault;                  // DQMC_SYNC_CHECK: first kernel family whose work came back with an error
};
static const char* const kFamName[FAM_COUNT] = {"k_bmult_chain / site-local V", "k_zgemm (n_g^3 products)", "decomposition (QR / LU / Jacobi, triangular solves)",
                                                "k_update_decide / k_hubbard_slice", "small kernels (copies, scales, set-up)", "k_update_gather", "k_flush", "rounds"};
// end of an entry point that only enqueued work
static int finish(dqmc_ctx* c, const char* entry) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && sync_check_on()) e = hipStreamSynchronize(c->st);
    if (e == hipSuccess && sync_check_on() && c->pipelined) {      // the flushes of a pipelined update run on the second stream
        e = hipStreamSynchronize(c->st2);
        if (e != hipSuccess && c->fault.empty()) c->fault = std::string("k_flush (second stream) (") + hipGetErrorString(e) + ")";
    }
    if (e == hipSuccess && c->fault.empty()) return DQMC_OK;
    std::string msg = std::string(entry) + ": " + (e != hipSuccess ? hipGetErrorString(e) : "GPU fault");
    if (!c->fault.empty()) msg += " in " + c->fault;
    msg += sync_check_on() ? " [DQMC_SYNC_CHECK: raised by work this call enqueued]"
                           : " [asynchronous: may stem from an earlier call; rerun with DQMC_SYNC_CHECK=1 to name the call and kernel family]";
    return fail(DQMC_EHIP, msg);
}

// shared (chain independent) device memory
template<class T>
static int salloc(dqmc_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, count * sizeof(T)));
    c->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}
// the selected chain's copy of a per-chain buffer (host-buffer entry points)
template<class T> static T* selp(dqmc_ctx* c, T* p) { return (T*)((char*)p + (size_t)c->sel * c->lc.cs); }
template<class T> static T* chainp(dqmc_ctx* c, T* p, int b) { return (T*)((char*)p + (size_t)b * c->lc.cs); }
// Blocking copy on the context's OWN (non-blocking) stream.  Nothing in this library touches the legacy null stream: a
// null-stream copy would wait for -- and hold up -- every blocking stream of the process, i.e. serialise contexts that
// different host threads drive concurrently (one context per sub-batch of replicas, host/detsdw.cpp).
static hipError_t copy_sync(dqmc_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->st);
    return e != hipSuccess ? e : hipStreamSynchronize(c->st);
}

DQMC_PRIVATE void prof_collect(dqmc_ctx* c);                 // dqmc_context.hip
enum { PROF_EVENT_CAP = 8192 };     // events alive at most: beyond that the finished pairs are collected and reused
// A fresh (begin, end) pair of timing events: records the begin event on st and returns its index; the end event is index + 1
static int prof_event_pair(dqmc_ctx* c, hipStream_t st) {
    if (c->ev_used + 2 > c->ev_pool.size())
        for (int i = 0; i < 2; ++i) { hipEvent_t e; (void)hipEventCreate(&e); c->ev_pool.push_back(e); }
    const int idx = (int)c->ev_used;
    (void)hipEventRecord(c->ev_pool[idx], st);
    c->ev_used += 2;
    return idx;
}

struct ProfScope {
    dqmc_ctx* c; int fam; uint64_t launches; int idx = -1;     // idx: this scope's begin event (scopes may nest)
    hipStream_t st;                                            // the stream the scope's kernels are launched on (c->st, or c->st2 for a pipelined flush)
    ProfScope(dqmc_ctx* c_, int fam_, uint64_t launches_, hipStream_t st_ = nullptr) : c(c_), fam(fam_), launches(launches_), st(st_ ? st_ : c_->st) {
        c->fam_launches[fam] += launches;
        if (!c->prof) return;
        if (c->ev_used + 2 > PROF_EVENT_CAP && c->prof_depth == 0) prof_collect(c);   // not while an outer scope is open
        ++c->prof_depth;
        idx = prof_event_pair(c, st);
        c->ev_open.push_back({fam, idx});
    }
    ~ProfScope() {
        if (sync_check_on() && c->fault.empty()) {
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) c->fault = std::string(kFamName[fam]) + (st == c->st ? "" : " (second stream)") + " (" + hipGetErrorString(e) + ")";
        }
        if (idx < 0) return;
        (void)hipEventRecord(c->ev_pool[idx + 1], st);
        --c->prof_depth;
    }
};

#define G_FRESH(c, who) do { if ((c)->g_stale) return fail(DQMC_EINVAL, who ": G is stale after dqmc_wrap_skip (dqmc_advance, dqmc_udv_setup or dqmc_set_green_host rebuild it)"); } while (0)

// building blocks of dqmc_context.hip that the measurement entry points use
DQMC_PRIVATE GemmArgs gemm_square(dqmc_ctx* c, const cplx* A, int opA, const cplx* B, int opB, cplx* C);
DQMC_PRIVATE void run_gemm(dqmc_ctx* c, const GemmArgs& g);
DQMC_PRIVATE void bmult_dev(dqmc_ctx* c, int side, int inverse, int k2, int k1, cplx* A, const cplx* src = nullptr);
DQMC_PRIVATE void series_free(dqmc_ctx* c);
DQMC_PRIVATE void green_matrix_free(dqmc_ctx* c);           // dqmc_measure_api.hip: the blocks of dqmc_set_green_matrix
DQMC_PRIVATE void custom_pair_free(dqmc_ctx* c);            // dqmc_measure_api.hip: the blocks of dqmc_set_custom_pair_operators
DQMC_PRIVATE void custom_free(dqmc_ctx* c);                 // dqmc_measure_api.hip: the blocks of dqmc_set_custom_bilinears
