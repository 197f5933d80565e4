/*
 * dqmc_hip.h -- C ABI of the MI355X (gfx950) DQMC sweep kernels.
 *
 * This is the drop-in boundary for the reference's DetModelGC/DetSDW hot path
 * (crstnbr/detqmc).  The reference has NO runtime plugin boundary for this path: DetQMC<Model> is
 * a class template and DetModelGC::sweep_skeleton takes the B-multiply / update routines as
 * template callables (src/detqmc.h:58-59, src/detmodel.h:250-265).  Each entry point below
 * replaces one of those callables / member functions; the reference interface it replaces is
 * cited as file:line relative to /root/reference/src.  INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - complex fp64, interleaved (re, im) == std::complex<double> == arma::cx_double
 *   - matrices are n_g x n_g, COLUMN-major, leading dimension n_g, n_g = MSF*N,
 *     MSF = (opdim == 3 ? 4 : 2) (src/detsdwopdim.h:161), N = L*L, site = y*L + x
 *   - phi is laid out like the reference's arma::Cube phi(N, OPDIM, m+1): index
 *     site + N*(dim + OPDIM*k); slice k = 0 is unused (src/detsdwopdim.h:461-466)
 *   - every function returns 0 on success, a negative DQMC_E* code otherwise; nothing throws
 *     across the boundary; dqmc_last_error() gives the text
 *   - one dqmc_ctx == one replica, bound to one device and one HIP stream; not thread-safe;
 *     different contexts may be driven from different host threads
 *   - functions whose name ends in _host take/return caller-owned HOST buffers and synchronise;
 *     all others only enqueue work on the context's stream
 */
#ifndef DQMC_HIP_H_
#define DQMC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dqmc_ctx dqmc_ctx;

typedef struct dqmc_cplx { double re, im; } dqmc_cplx;

enum {
    DQMC_OK = 0,
    DQMC_EINVAL = -1,     /* bad argument / unsupported parameter (reference: ParameterWrong) */
    DQMC_EHIP = -2,       /* HIP runtime error */
    DQMC_ENOCONV = -3,    /* decomposition did not converge (reference: "SVD failed (std)", udv.h:77-88) */
    DQMC_ERNG = -4,       /* device ran out of pre-drawn uniforms */
    DQMC_ENODEV = -5      /* no usable GPU */
};

enum { DQMC_BC_PBC = 0, DQMC_BC_APBC_X = 1, DQMC_BC_APBC_Y = 2, DQMC_BC_APBC_XY = 3 };
enum { DQMC_LEFT = 0, DQMC_RIGHT = 1 };
enum { DQMC_UP = +1, DQMC_DOWN = -1 };
enum { DQMC_STAB_SVD = 0, DQMC_STAB_QR = 1 };
enum { DQMC_MODEL_SDW = 0, DQMC_MODEL_HUBBARD = 1 };
/* flag bit of dqmc_params::timedisplaced (the low bits keep their values 0 / 1 / 2): also reserve what the every-slice entries
 * dqmc_measure_timedisplaced_segment / _ends need */
enum { DQMC_TD_EVERY_SLICE = 0x100 };
/* flag bit of dqmc_params::timedisplaced, DQMC_MODEL_HUBBARD only: also reserve what the every-slice entries of the Hubbard model
 * dqmc_hubbard_measure_timedisplaced_segment / _ends need (three work matrices and one block of m + 1 rows, behind every other buffer) */
enum { DQMC_TD_HUB_EVERY_SLICE = 0x400 };
/* flag bit of dqmc_params::td_particle_hole (the low bits keep their values 0 / 1 / 2): also reserve what the band-resolved charge
 * channels bandDiff / bandMix need (dqmc_measure_timedisplaced_band below) */
enum { DQMC_TD_PH_BAND = 0x100 };

/* Execution choices that change NO result (the parity tests hold for every value); 0 = automatic everywhere.  They are
 * create-time parameters of a context: nothing about a context's launch schedule depends on the environment or on other
 * contexts of the process. */
typedef struct dqmc_tuning {
    int32_t pipeline;          /* delayed updates: the flush of block b on a second stream next to the decisions of block b + 1
                                  (which read a compact, already updated copy of their proposal window).  0: automatic (n_g > 1024
                                  and at least two chains), 1: on, -1: off.  dqmc_get_schedule_info tells what ran */
    int32_t qr_variant;        /* QR mode, chain factorisations: 0 automatic (Householder panels up to n_g = 1024, block
                                  Gram-Schmidt + Cholesky-QR2 above), 1: Householder, 2: block Gram-Schmidt */
    int32_t green_variant;     /* QR mode, inverse inside greenFromUdV: 0 automatic (LU with partial pivoting for n_g <= 512,
                                  QR above), 1: QR */
    int32_t max_jacobi_sweeps; /* SVD mode: sweep budget of the one-sided Jacobi SVD, 0 = 80; exhausting it is DQMC_ENOCONV
                                  ("SVD failed", udv.h:77-88) */
    int32_t proposal_budget;   /* proposals per delayed-update block: 0 automatic (2 delaySteps for delaySteps >= 8), -1 no
                                  limit, > 0 that many (at least delaySteps) */
    int32_t decide_threads;    /* threads per workgroup of the decision kernel: 0 automatic (512 for O(1) / O(2) contexts of at most 32
                                  chains, else 256), 256, 512 (O(3): always 256).  Launch shape only: the chain does not depend on it */
    int32_t bmult_path;        /* checkerboard B-multiply kernel: 0 automatic (the direct kernel for the launch kinds where it measured
                                  faster), 1: the staged kernel k_bmult_chain everywhere, 2: the direct kernel wherever it
                                  applies (checkerboard launches outside shift mode).  Both give the same bits.  Other values:
                                  DQMC_EINVAL.  (The field took the last reserved slot: the bytes of the struct are where they were.)
                                  The struct has no free slot left, so one more choice travels as a flag bit of this field:
                                  | DQMC_TUNING_NO_RNG_LOOKAHEAD: the context reserves no second window and no tail of pre-drawn
                                  uniforms, dqmc_stage_uniforms_tail_host / dqmc_advance_uniforms return DQMC_EINVAL */
} dqmc_tuning;
enum { DQMC_TUNING_NO_RNG_LOOKAHEAD = 0x100 };

/* ModelParamsDetSDW fields the kernels depend on (src/detsdwparams.h:24-120) */
typedef struct dqmc_params {
    int32_t opdim;        /* 1, 2 or 3 */
    int32_t L;            /* even */
    int32_t m;            /* time slices */
    int32_t s;            /* stabilisation interval, s < m */
    int32_t delaySteps;   /* D, 1..N, MSF*D <= 64 */
    int32_t bc;           /* DQMC_BC_* */
    int32_t weakZflux;    /* only with opdim == 2 */
    int32_t phi2bosons;
    int32_t device;       /* HIP device ordinal */
    int32_t stabilisation; /* DQMC_STAB_SVD (reference-exact UdV = SVD) or DQMC_STAB_QR (pre-pivoted Householder UDT) */
    int32_t cb_none;      /* 0: checkerboard break-up CB_ASSAAD_BERG (every shipped config); 1: checkerboard=false,
                             dense B_k = e^{-dtau V_k} e^{-dtau K} (computeBmatSDW, detsdwopdim.cpp:1309-1485) */
    int32_t model;        /* DQMC_MODEL_SDW (default) or DQMC_MODEL_HUBBARD: the reference's DetHubbard (src/dethubbard.{h,cpp}), both
                             spin sectors in one block-diagonal 2N x 2N matrix.  Hubbard reads: L, m, s, dtau, txhor = t, u = U,
                             mux = mu, cb_none = !checkerboard (propagator e^{-dtau T} by diagonalisation, or the checkerboard
                             product form of dethubbard.cpp:717-770), stabilisation, device; opdim must be 1 (the field is the
                             Ising auxiliary field, phi = +-1), delaySteps 1 */
    double dtau, r, c, u, lambda;
    double txhor, txver, tyhor, tyver;
    double mux, muy;
    double accRatio;      /* target acceptance for the box step adaptation */
    double cdwU;          /* != 0: the discrete field l_i(tau) in {+-1, +-2} next to phi (detsdwparams.h:61; evMatrix,
                             detsdwopdim.cpp:3187-3229); dqmc_update_slice then runs the cdwl pass behind the phi pass (:2474-2485) */
    int32_t rng_window_per_site;   /* capacity of the window of pre-drawn uniforms, per site and time slice of a sweep; 0 = what box proposals
                                      with repeatUpdateInSlice = 1 can consume at most (opdim + 1, + 2 with cdwU).  Callers that use
                                      dqmc_update_slice_ex with more passes or the rotate / scale proposals (whose Gaussian draws consume
                                      a variable number) size it: repeat x (opdim + 1) resp. repeat x 8 (+ 2 with cdwU) */
    int32_t timedisplaced; /* 1: reserve the per-chain buffers of the time-displaced Green's functions and their accumulator
                              block (SDW model only); dqmc_set_timedisplaced switches the computation on and off.  2: also the
                              accumulator block of dqmc_measure_timedisplaced_pair.  0: nothing is reserved, nothing changes.
                              1 | DQMC_TD_EVERY_SLICE, 2 | DQMC_TD_EVERY_SLICE: everything the low value reserves with the same layout,
                              launches and results, and behind every other buffer (those of td_particle_hole included) three work
                              matrices and one every-slice accumulator block per enabled channel (the struct has no free slot: the
                              option travels as a flag bit).  Any other value, any other bit: DQMC_EINVAL.  DQMC_MODEL_HUBBARD accepts
                              timedisplaced = 1 together with td_particle_hole = 1 and nothing else: the matrices of G(tau,0), G(0,tau),
                              G(0), one scratch matrix and the block of dqmc_hubbard_measure_timedisplaced, behind every other buffer;
                              1 | DQMC_TD_HUB_EVERY_SLICE with td_particle_hole = 1 (needs s < m, i.e. n >= 2): the same with the same
                              layout, launches and results, and behind it three work matrices and the every-slice block of
                              dqmc_hubbard_measure_timedisplaced_segment / _ends.  The SDW model refuses DQMC_TD_HUB_EVERY_SLICE, the
                              Hubbard model DQMC_TD_EVERY_SLICE */
    dqmc_tuning tuning;   /* all zero = automatic */
    int32_t td_particle_hole; /* 1 (needs timedisplaced >= 1, SDW model; DQMC_EINVAL otherwise): also reserve, behind every other buffer,
                                 the equal-time G(0) of the boundary's own field configuration, one matrix for a shifted copy, the
                                 per-site one-body values and the accumulator block of dqmc_measure_timedisplaced_ph.  0: nothing is
                                 reserved, nothing changes.  2: everything value 1 reserves with the same layout, launches and results,
                                 and behind it the bond-amplitude table, the per-site one-body values and the accumulator block of
                                 dqmc_measure_timedisplaced_current.  1 | DQMC_TD_PH_BAND, 2 | DQMC_TD_PH_BAND: everything the low value
                                 reserves with the same layout, launches and results, and behind every other buffer (the every-slice
                                 ones included) the one-body values and the accumulator block of dqmc_measure_timedisplaced_band, with
                                 DQMC_TD_EVERY_SLICE also an every-slice block for channel 4.  Any other value, any other bit, the flag
                                 on 0: DQMC_EINVAL.  (The field took the second reserved slot of dqmc_tuning: the bytes of the struct
                                 are where they were.) */
} dqmc_params;

/* AdjustmentData + slice bookkeeping that lives on the device between calls
 * (src/detsdwopdim.h:481-577, RunningAverage.h) */
typedef struct dqmc_update_state {
    double phiDelta;
    double targetAccRatio;
    double lastAccRatio;
    double ra_runningAverage;
    double ra_values[100];
    int32_t ra_samplesAdded;
    int32_t ra_head;
    uint64_t rng_consumed;   /* uniforms consumed from the pushed window */
    uint64_t rng_avail;      /* size of the pushed window */
    int32_t error;           /* DQMC_ERNG if the window ran dry */
    int32_t reserved;
    /* rotate / scale proposals of the O(3) model (spinProposalMethod != box): AdjustmentData::angleDelta (the minimal cos(theta) of a
     * rotation), scaleDelta (width of the Gaussian |phi|^3 update), the bisection bounds of their adaptation and the running
     * averages accRatioLocal_rotate_RA / _scale_RA (src/detsdwopdim.h:489-530, src/detsdwopdim.cpp:3299-3375) */
    double angleDelta, scaleDelta;
    double curminAngleDelta, curmaxAngleDelta, curminScaleDelta, curmaxScaleDelta;
    double rot_runningAverage;
    double rot_values[100];
    double scl_runningAverage;
    double scl_values[100];
    int32_t rot_samplesAdded, rot_head, scl_samplesAdded, scl_head;
} dqmc_update_state;

/* ---- lifetime ------------------------------------------------------------------------- */
/* replaces DetSDW ctor set-up of hopping constants / 4-site exponentials
 * (detsdwopdim.cpp:217-264, :1598-1684) */
int dqmc_create(const dqmc_params* p, dqmc_ctx** out);
/* Batched replicas: ONE context that advances `nchains` independent Markov chains (the replicas of a
 * parallel-tempering run, src/detqmcpt.h: one replica per MPI rank there) in lockstep -- every kernel launch
 * carries all chains (grid.z = chain), which is what fills the 256 CUs at the lattice sizes of interest.
 * All chains share the lattice/temperature parameters of *p; fields, RNG windows, update state and the
 * exchange parameter r are per chain.  The compute entry points (udv_setup, advance, wrap, update_slice,
 * backup) act on all chains; the host-buffer entry points (set/get fields, Green's function, singular
 * values, UdV, uniforms, update state, exchange parameter / action, restore) act on the chain chosen with
 * dqmc_select_chain (default 0).  dqmc_create == dqmc_create_batch with nchains = 1. */
int dqmc_create_batch(const dqmc_params* p, int nchains, dqmc_ctx** out);
int dqmc_select_chain(dqmc_ctx* ctx, int chain);
int dqmc_num_chains(dqmc_ctx* ctx);
void dqmc_destroy(dqmc_ctx* ctx);
const char* dqmc_last_error(void);
int dqmc_synchronize(dqmc_ctx* ctx);
/* raw stream handle (hipStream_t) for event timing by the harness */
void* dqmc_stream(dqmc_ctx* ctx);

/* ---- fields (a22) ---------------------------------------------------------------------- */
/* upload phi and recompute cosh/sinh caches: updateCoshSinhTermsPhi (detsdwopdim.cpp:1175-1181) */
int dqmc_set_fields_host(dqmc_ctx* ctx, const double* phi);
int dqmc_get_fields_host(dqmc_ctx* ctx, double* phi, double* coshTermPhi, double* sinhTermPhi);
/* cdwU != 0: the discrete field of the selected chain, cdwl[k * N + site] in {+-1, +-2} (slice 0 unused); set recomputes
 * coshTermCDWl / sinhTermCDWl (updateCoshSinhTermsCDWl, detsdwopdim.cpp:1183-1190).  After dqmc_create the field is +1
 * everywhere (setupConstantField, :1116-1128).  DQMC_EINVAL on a context created with cdwU == 0. */
int dqmc_set_cdwl_host(dqmc_ctx* ctx, const int32_t* cdwl);
int dqmc_get_cdwl_host(dqmc_ctx* ctx, int32_t* cdwl);
/* all chains of a batched context in ONE transfer: phi_all = nchains cubes of (m+1) * opdim * N doubles, back to back */
int dqmc_set_fields_all_host(dqmc_ctx* ctx, const double* phi_all);
int dqmc_get_fields_all_host(dqmc_ctx* ctx, double* phi_all);

/* ---- checkerboard B-multiplies (a10-a14) -------------------------------------------------- */
/* A <- B(k2,k1) A | B(k2,k1)^-1 A | A B(k2,k1) | A B(k2,k1)^-1 on a HOST matrix:
 * checkerboard{Left,Right}MultiplyBmat[Inv] (detsdwopdim.cpp:2076-2090, 2172-2186, 2307-2324,
 * 2406-2420), i.e. the four callables of sweep_skeleton (detmodel.h:256-260). */
int dqmc_bmult_host(dqmc_ctx* ctx, int side, int inverse, int k2, int k1, dqmc_cplx* A);
/* The same out of place, as the chain steps of dqmc_advance (DQMC_UP) and dqmc_udv_setup run it: out = B(k2,k1) src etc.; the device
 * kernel reads its operands from a source buffer and writes another.  src_after (may be NULL) receives the source buffer as it is
 * afterwards: unchanged. */
int dqmc_bmult_src_host(dqmc_ctx* ctx, int side, int inverse, int k2, int k1, const dqmc_cplx* src, dqmc_cplx* out, dqmc_cplx* src_after);

/* ---- UdV decomposition and dense products (a2, L1) ---------------------------------------- */
/* udvDecompose (udv.h:68-102): M = U diag(d) V_t^H, d descending */
int dqmc_udv_decompose_host(dqmc_ctx* ctx, const dqmc_cplx* M, dqmc_cplx* U, double* d, dqmc_cplx* V_t,
                            int* sweeps_used);
/* Test-facing: the chain factorisation exactly as dqmc_udv_setup / dqmc_advance call it, on caller-given operands, every chain its own.
 *   M [nchains][n_g^2], colscale / rowscale [nchains][n_g] (each may be NULL): the matrix factorised is M' = diag(rowscale) M diag(colscale)
 *   kind 0: R-type, M' = U d V_t^H with U unitary (QR mode: V_t = (D^-1 R P^T)^H);  kind 1: L-type, V_t unitary, the adjoint's factorisation
 *           (SVD mode: both factors are unitary for either kind, d descending)
 *   Aold [nchains][n_g^2] or NULL: with it the chained step runs (QR mode: the lazy triangular product) and the non-unitary factor
 *           returned (V_t for kind 0, U for kind 1) is Aold times the new one
 *   U, V_t [nchains][n_g^2], d [nchains][n_g]; sweeps_used (may be NULL): Jacobi sweeps in SVD mode, 0 in QR mode
 * dqmc_green_from_factors_host: greenFromUdV on an L-type slot (U_l, d_l, V_l) and an R-type slot (U_r, d_r, V_r), B_L = U_l d_l V_l^H,
 * B_R = U_r d_r V_r^H, layouts as above; a slot is three pointers or three NULLs.  Both slots: G = (1 + B_R B_L)^-1 and, while
 * dqmc_set_timedisplaced is on, G(tau,0) = G B_R, G(0,tau) = -B_L G and (dqmc_params::td_particle_hole) G(0) = 1 - B_L G B_R into GT0,
 * G0T, G00 [nchains][n_g^2] (each may be NULL; non-NULL where the context does not compute it: DQMC_EINVAL).  One slot NULL:
 * greenFromEye_and_UdV of the other with its kind, G alone.  Only U_r and V_l are taken as unitary.  sv [nchains][n_g]: what
 * dqmc_get_sv_host reports (QR mode: sum of log sv = log |det(1 + B_R B_L)|).
 * Both calls work in buffers of the sweep (UdV storage, G, the singular values): afterwards the context's G is stale and no advance is
 * accepted until the next dqmc_udv_setup.  No sweep calls them. */
int dqmc_decompose_host(dqmc_ctx* ctx, const dqmc_cplx* M, const double* colscale, const double* rowscale, int kind,
                        const dqmc_cplx* Aold, dqmc_cplx* U, double* d, dqmc_cplx* V_t, int* sweeps_used);
int dqmc_green_from_factors_host(dqmc_ctx* ctx, const dqmc_cplx* U_l, const double* d_l, const dqmc_cplx* V_l,
                                 const dqmc_cplx* U_r, const double* d_r, const dqmc_cplx* V_r,
                                 dqmc_cplx* G, double* sv, dqmc_cplx* GT0, dqmc_cplx* G0T, dqmc_cplx* G00);
/* C = op(A) op(B), op = identity (0) or conjugate transpose (1): the zgemm calls behind
 * detmodel.h:784-815 */
int dqmc_gemm_host(dqmc_ctx* ctx, int opA, int opB, const dqmc_cplx* A, const dqmc_cplx* B, dqmc_cplx* C);

/* ---- stabilised Green's function (a3-a8) ---------------------------------------------------- */
/* setupUdVStorage_and_calculateGreen_skeleton (detmodel.h:680-713): storage[0..n], G(beta) */
int dqmc_udv_setup(dqmc_ctx* ctx);
/* advanceUpGreen(l) / advanceDownGreen(l) incl. greenFromUdV / greenFromEye_and_UdV
 * (detmodel.h:1109-1163, 956-1017, 769-860) */
int dqmc_advance(dqmc_ctx* ctx, int dir, int l);
/* wrapUpGreen(k): G <- B_{k+1} G B_{k+1}^-1 ; wrapDownGreen(k): G <- B_k^-1 G B_k
 * (detmodel.h:1236-1259, 1066-1095) */
int dqmc_wrap(dqmc_ctx* ctx, int dir, int k);
/* A wrap whose result nobody reads: the checks of dqmc_wrap, currentTimeslice moves as there, nothing is launched and G is
 * marked stale.  For the last wrap of a segment of a down sweep, which the dqmc_advance that follows overwrites (it rebuilds G
 * from the UdV factors).  While G is stale every entry that reads G (update, wrap, measure, get / shift Green, backup, ...)
 * returns DQMC_EINVAL; dqmc_advance, dqmc_udv_setup and dqmc_set_green_host clear the mark. */
int dqmc_wrap_skip(dqmc_ctx* ctx, int dir, int k);
/* sweepUp resets storage[0] to the identity (detmodel.h:1293-1295) */
int dqmc_reset_storage0(dqmc_ctx* ctx);
/* Wrap-error diagnostics ("green check"): how far the Green's function carried by wraps and updates has drifted from the one rebuilt
 * from the UdV factors, at every stabilisation boundary -- the number that tells whether the interval s is adequate (the reference's
 * logGreenConsistency, detmodel.h:993-1010, 1129-1158, and logSV, detmodel.h:796-807).  Both models.  dqmc_set_green_check(ctx, on) is
 * run-time state, to be changed between entry calls: switching on allocates, outside the arena and cleared, one G-sized buffer per chain,
 * the partial results of the compare kernel and the table below (a failed allocation leaves the context as it was); switching off frees
 * them; a repeated call changes nothing.  With the switch off no buffer exists, no launch is added and every entry point behaves bit
 * for bit as without this section.
 * While on, a dqmc_advance that finds G fresh on entry (no dqmc_wrap_skip / dqmc_update_slice_final since it was last computed or set)
 * keeps a copy Gw of it, rebuilds G = Gf as always and then compares the two on the device, all chains in one stream-ordered pass
 * (no host synchronisation, no atomics, fixed summation order: the same matrices give the same bits):
 *   maxAbs      = max |Gw - Gf| over all entries, argmax = row + col n_g of the first entry (column-major order) that attains it,
 *                 0 for an all-zero difference
 *   maxSiteDiag = the same maximum over the entries with row mod N == col mod N (the reference's "block diagonals": what local
 *                 observables read)
 *   meanAbs     = sum |Gw - Gf| / n_g^2,   maxRel = maxAbs / max |Gf|
 *   nonfinite   = entries where either matrix is inf or NaN; such an entry enters maxAbs (and argmax) as +inf and stays out of
 *                 maxSiteDiag, meanAbs and max |Gf|, so a NaN is never hidden by a maximum
 * and folds them into row [dir][j] of every chain's table, dir = 0 for DQMC_DOWN, 1 for DQMC_UP, j = the storage index the advance
 * lands on (l - 1 for a down advance: 0 .. n-1; l + 1 for an up advance: 1 .. n).  An advance that finds G stale takes no sample and
 * moves no count; dqmc_udv_setup, dqmc_restore and dqmc_set_green_host never take one themselves (the advance that follows a
 * dqmc_set_green_host compares against the matrix that call set).
 * Table: per chain [2][n+1] rows of DQMC_GREEN_CHECK_FIELDS doubles, all zero after the switch-on and dqmc_green_check_reset:
 *   [0] count            samples folded into the row
 *   [1] lastMaxAbs       maxAbs of the latest sample
 *   [2] maxAbs           running maximum of maxAbs          [3] sumMaxAbs   sum of maxAbs (mean = / count)
 *   [4] maxSiteDiag      running maximum                    [5] sumMeanAbs  sum of meanAbs (mean = / count)
 *   [6] maxRel           running maximum                    [7] argmax      of the sample that set [2]
 *   [8] nonfinite        sum over the samples
 *   [9] logScaleSpread   running maximum of log(max d / min d) of the scales d of the factorisation the advance just stored in
 *                        storage[j] (both stabilisation modes)
 *   [10] logSvSpread     DQMC_STAB_SVD: running maximum of log(max sv) - log(min sv) of the singular values of G^-1 the rebuild found
 *                        (dqmc_get_sv_host; the reference's logSV).  DQMC_STAB_QR: 0 (the vector holds the log-det factors there)
 * The spreads are formed on the device in the finalise step of the compare.  dqmc_green_check_size: doubles per chain, 2 (n + 1)
 * DQMC_GREEN_CHECK_FIELDS, 0 while off.  dqmc_green_check_read_host: out[nchains][2][n+1][DQMC_GREEN_CHECK_FIELDS], all chains;
 * synchronises.  The readers and the reset return DQMC_EINVAL while the switch is off.  The table is per chain of this context: it is
 * not part of any saved state or of the measurement series, and dqmc_measure_reset leaves it alone. */
enum { DQMC_GREEN_CHECK_FIELDS = 11 };
int dqmc_set_green_check(dqmc_ctx* ctx, int on);
size_t dqmc_green_check_size(dqmc_ctx* ctx);
int dqmc_green_check_read_host(dqmc_ctx* ctx, double* out);
int dqmc_green_check_reset(dqmc_ctx* ctx);

/* ---- local updates (a17-a20) ---------------------------------------------------------------- */
/* replace the window of pre-drawn uniforms (0,1) the device consumes in stream order */
int dqmc_push_uniforms_host(dqmc_ctx* ctx, const double* u, size_t n);
/* the same for ALL chains of a batched context in one transfer: u = nchains windows of n uniforms each, back to back */
int dqmc_push_uniforms_all_host(dqmc_ctx* ctx, const double* u, size_t n);
/* Look-ahead on the stream of uniforms: while the device works through the window [p, p + n) of every chain, the host uploads the
 * n draws behind it and the next sweep starts from a window spliced on the device -- no transfer and no wait at its head.
 *   dqmc_uniforms_staging_host: the context's pinned staging buffer (nchains windows of `capacity` doubles are guaranteed to fit back
 *     to back for every n the context accepts); allocated by the first call.  It waits for an upload that still reads the buffer, so
 *     the caller may fill it when the call returns.
 *   dqmc_stage_uniforms_tail_host: u = nchains runs of n uniforms, back to back, chain b's being the stream positions
 *     [p_b + n, p_b + 2 n) behind its current window; n must be the size of the current window (the last dqmc_push_uniforms_all_host
 *     or dqmc_advance_uniforms).  u may be the staging buffer itself; otherwise it is copied there first.  The upload runs on a stream
 *     of its own, behind the last dqmc_advance_uniforms (event), and the call waits for nothing the main stream holds.
 *   dqmc_advance_uniforms: ONE launch on the main stream, behind the staged upload (event).  offset[b] in 0 .. n = how far chain b's
 *     stream has moved since its window began (what the device consumed plus what the host drew since); the new window of chain b is
 *     new[i] = i < n - offset[b] ? cur[offset[b] + i] : tail[i - (n - offset[b])], it takes the place of the current one, and
 *     rng_consumed = 0, rng_avail = n, error = 0.  The tail is used up: stage the next one before the next advance.
 * DQMC_EINVAL (nothing launched, nothing changed): no tail staged, an offset > n, n unlike the current window's size, or a context
 * created with DQMC_TUNING_NO_RNG_LOOKAHEAD.  dqmc_push_uniforms_*_host drop a staged tail.  dqmc_get_schedule_info counts both paths. */
int dqmc_uniforms_staging_host(dqmc_ctx* ctx, double** buf, size_t* capacity);
int dqmc_stage_uniforms_tail_host(dqmc_ctx* ctx, const double* u, size_t n);
int dqmc_advance_uniforms(dqmc_ctx* ctx, const uint64_t* offset /* [nchains] */);
/* the first n uniforms of the selected chain's current window (tests) */
int dqmc_get_uniform_window_host(dqmc_ctx* ctx, double* out, size_t n);
/* updateInSlice (detsdwopdim.cpp:2428-2489, delayed updates :3023-3175, box proposals :3922-3931,
 * deltaSPhi :4186-4239, get_delta_forsite :3179-3289); thermalization != 0 adds the step-size
 * adaptation of updateInSliceThermalization (:3294-3375) */
int dqmc_update_slice(dqmc_ctx* ctx, int k, int thermalization);
/* The same with the other proposal kinds and repeatUpdateInSlice (src/detsdwopdim.cpp:2438-2470): `proposal` = DQMC_PROPOSE_BOX
 * (proposeNewPhiBox), _ROTATE (proposeRotatedPhi, :3945-4002), _SCALE (proposeScaledPhi, :4016-4077), _ROTATE_AND_SCALE
 * (proposeRotatedScaledPhi, :4092-4170) -- the last three for opdim == 3 only, as in the reference; `repeat` passes over the slice
 * (each a full updateInSlice_delayed; lastAccRatio is the last pass's); with thermalization != 0 the running average and step
 * parameter named by `adapt` are updated once, from the last pass (updateInSliceThermalization, :3294-3375): DQMC_ADAPT_BOX (phiDelta),
 * _ROTATE (angleDelta), _SCALE (scaleDelta, only moved with adapt_scale_variance != 0).  Which kind a sweep uses (rotate_then_scale
 * alternates with performedSweeps, rotate_and_scale alternates the ADAPTED quantity every 100 sweeps) is the host layer's business. */
enum { DQMC_PROPOSE_BOX = 0, DQMC_PROPOSE_ROTATE = 1, DQMC_PROPOSE_SCALE = 2, DQMC_PROPOSE_ROTATE_AND_SCALE = 3 };
enum { DQMC_ADAPT_BOX = 0, DQMC_ADAPT_ROTATE = 1, DQMC_ADAPT_SCALE = 2 };
int dqmc_update_slice_ex(dqmc_ctx* ctx, int k, int thermalization, int proposal, int adapt, int adapt_scale_variance, int repeat);
/* The update of the LAST slice of a segment, whose G nobody reads: the dqmc_advance that follows rebuilds G from the UdV factors.  The
 * same decisions as dqmc_update_slice_ex (fields, update state, counters bit for bit), but in the last pass over the slice a chain does
 * not gather and flush the delayed-update block in which it finishes the slice.  G is marked stale as after dqmc_wrap_skip (every
 * entry that reads G returns DQMC_EINVAL until dqmc_advance, dqmc_udv_setup or dqmc_set_green_host rebuild it).  then_wrap_dir: 0, or
 * DQMC_DOWN to take the checks and the currentTimeslice bookkeeping of the down wrap of slice k along (dqmc_wrap_skip itself refuses a
 * stale G).  A refused call changes nothing.  Where the block cannot be skipped (pipelined schedule, Hubbard replica) this is
 * dqmc_update_slice_ex followed by dqmc_wrap for DQMC_DOWN, and G stays fresh. */
int dqmc_update_slice_final(dqmc_ctx* ctx, int k, int thermalization, int proposal, int adapt, int adapt_scale_variance, int repeat,
                            int then_wrap_dir);
/* Which schedule dqmc_update_slice runs for this context (latched at dqmc_create from dqmc_tuning::pipeline and the shape of the
 * context) and how many delayed-update blocks have gone through each since dqmc_create. */
typedef struct dqmc_schedule_info {
    int32_t pipelined;              /* 1: flush on the second stream next to the next block's decisions; 0: strictly sequential */
    int32_t proposal_budget;        /* proposals per block in effect (0: no limit) */
    uint64_t blocks_pipelined;      /* decide / gather / flush rounds launched in the pipelined form */
    uint64_t blocks_sequential;     /* ... in the sequential form */
    int32_t qr_block_gram_schmidt;  /* 1: chain factorisations by block Gram-Schmidt + CholQR2, 0: Householder panels */
    int32_t green_lu;               /* 1: inverse inside greenFromUdV by LU, 0: by QR */
    uint64_t cholqr_fallbacks;      /* factorisations in which a CholQR panel lost definiteness and was redone with Householder panels */
    uint64_t uniform_windows_advanced;  /* windows of uniforms spliced on the device (dqmc_advance_uniforms) ... */
    uint64_t uniform_windows_pushed;    /* ... and pushed whole from the host (dqmc_push_uniforms_host / _all_host) */
} dqmc_schedule_info;
int dqmc_get_schedule_info(dqmc_ctx* ctx, dqmc_schedule_info* out);
int dqmc_get_update_state_host(dqmc_ctx* ctx, dqmc_update_state* out);
int dqmc_get_update_states_all_host(dqmc_ctx* ctx, dqmc_update_state* out /* [nchains] */);
int dqmc_set_update_state_host(dqmc_ctx* ctx, const dqmc_update_state* in);

/* ---- state access ------------------------------------------------------------------------------ */
int dqmc_get_green_host(dqmc_ctx* ctx, dqmc_cplx* out);
int dqmc_set_green_host(dqmc_ctx* ctx, const dqmc_cplx* in, int currentTimeslice);
/* green_inv_sv (detmodel.h:466): singular values of G^-1 in SVD mode; in QR mode a positive vector with
 * the same log-sum (= log|det G^-1|), which is all the global moves use (detsdwopdim.cpp:3613-3620) */
int dqmc_get_sv_host(dqmc_ctx* ctx, double* out);
int dqmc_get_sv_all_host(dqmc_ctx* ctx, double* out /* [nchains][n_g] */);
int dqmc_get_udv_host(dqmc_ctx* ctx, int l, dqmc_cplx* U, double* d, dqmc_cplx* V_t);
int dqmc_current_timeslice(dqmc_ctx* ctx);

/* ---- global-move support (a21) ------------------------------------------------------------------ */
/* globalMoveStoreBackups / globalMoveRestoreBackups (detsdwopdim.cpp:3886-3917): swap G, sv,
 * UdV storage, copy fields */
int dqmc_backup(dqmc_ctx* ctx);
int dqmc_restore(dqmc_ctx* ctx);
/* global shift move on the device (attemptGlobalShiftMove, detsdwopdim.cpp:3565-3644): phiAction (:4242-4300) of every chain from
 * the resident field, out[nchains]; addGlobalRandomDisplacement (:3755-3763) of every chain, shifts[nchains][opdim] */
int dqmc_phi_action_all_host(dqmc_ctx* ctx, double* out);
int dqmc_shift_fields_all_host(dqmc_ctx* ctx, const double* shifts);
/* 1/2 dtau sum phi^2 (get_exchange_action_contribution, detsdwopdim.cpp:5205-5216) */
int dqmc_exchange_action_host(dqmc_ctx* ctx, double* out);
/* the same for every chain of the context, written to a caller-owned DEVICE array of nchains doubles (the send buffer of the
 * replica-exchange all_gather, src/detqmcpt.h:1003-1010, without a host hop); returns when the values are there */
int dqmc_exchange_actions_device(dqmc_ctx* ctx, double* out_dev);

/* ---- fermionic measurements --------------------------------------------------
 * shiftGreenSymmetric (src/detsdwopdim.cpp:4507-4612): e^{-dtau K/2} G e^{+dtau K/2} of the selected chain */
int dqmc_shift_green_symmetric_host(dqmc_ctx* ctx, dqmc_cplx* out);
/* initMeasurements / measure(k), G-dependent part (src/detsdwopdim.cpp:458-505, :545-899), all chains: the slice's
 * contributions are accumulated on the device.  Accumulator layout (doubles, dqmc_measure_accum_size of them):
 * [0] greenK0 sum, [1] greenLocal sum, [2] occDiffSq sum, [3] slices measured, pairPlus[N], pairMinus[N],
 * S_X[(2L-1)^2] and S_Y[(2L-1)^2] as (re, im): S_band(dx, dy) = sum over site pairs with r_i - r_j = (dx, dy) of
 * g_band,up(i,j) + g_band,down(i,j), bin index (dy + L-1) (2L-1) + (dx + L-1); the momentum-space occupation is
 * their Fourier sum (finishMeasurements does it on the host). */
int dqmc_measure_reset(dqmc_ctx* ctx);
int dqmc_measure_slice(dqmc_ctx* ctx);
size_t dqmc_measure_accum_size(dqmc_ctx* ctx);
int dqmc_measure_read_host(dqmc_ctx* ctx, double* out);
/* ---- equal-time charge, spin, SDW and pairing correlators (SDW model only) ----------
 * A switch of dqmc_measure_slice, not a create-time parameter.  While on, every dqmc_measure_slice also bins, from the same shifted
 * matrix g~ = e^{-dtau K/2} G(tau_k) e^{+dtau K/2} (no second shift), for every periodic site difference d = (dx, dy), bin dy L + dx,
 *   sum_B Re W_X(B (+) d, B),  X = charge, spinZ, sdw:  the W^M(A, B) of dqmc_measure_timedisplaced_ph with G(tau,0) -> g~ and
 *                              G(0,tau) -> g~ - 1 (both one-body factors from g~; the delta term enters the d = 0 bin analytically),
 *   sum_B Re T+-(B (+) d, B):  the T+- of dqmc_measure_timedisplaced_pair evaluated on g~,
 * and counts one sample.  All chains in one launch; one writer per accumulator, fixed summation order, bit-reproducible.
 * Block of one chain (doubles, dqmc_measure_eq_accum_size of them): count, charge[N], spinZ[N], sdw[N], pairPlus[N], pairMinus[N] --
 * raw sums, C_X(d) = sum / (count N).  The first enable allocates the block for all chains outside the per-chain arena (no existing
 * buffer moves); it is freed with the context and cleared by dqmc_measure_reset.  While off, dqmc_measure_slice launches what it always
 * did; the block of dqmc_measure_read_host is the same either way.  The Hubbard model returns DQMC_EINVAL. */
int dqmc_set_equal_time_correlators(dqmc_ctx* ctx, int on);
size_t dqmc_measure_eq_accum_size(dqmc_ctx* ctx);       /* 0 before the first enable, else 1 + 5 N */
int dqmc_measure_eq_read_host(dqmc_ctx* ctx, double* out);   /* selected chain; DQMC_EINVAL before the first enable */
/* The equal-time form of the band-resolved charge channels (bandDiff, bandMix: dqmc_measure_timedisplaced_band below): a second switch of
 * dqmc_measure_slice, independent of the one above, with a block of its own outside the arena that the first enable allocates:
 * count, bandDiff[N], bandMix[N] per chain (dqmc_measure_eq_band_accum_size = 1 + 2 N doubles), raw sums of Re W(B (+) d, B) with one
 * matrix g~ in both roles.  Both matrices have M^2 = 1, so the delta term is tr_4 g~(B; B) = 4 - o^charge(B), added to the d = 0 bin as for
 * the charge channel.  The transposed factor is read in place.  While off, and for every other block while on, nothing changes;
 * dqmc_measure_reset clears the block.  The Hubbard model returns DQMC_EINVAL. */
int dqmc_set_equal_time_band(dqmc_ctx* ctx, int on);
size_t dqmc_measure_eq_band_accum_size(dqmc_ctx* ctx);  /* 0 before the first enable, else 1 + 2 N */
int dqmc_measure_eq_band_read_host(dqmc_ctx* ctx, double* out);   /* selected chain; DQMC_EINVAL before the first enable */
/* ---- Hubbard model: equal-time and time-displaced correlators -----------------------
 * G_s(A, B) = <c_As c^+_Bs> is spin block s of the context's G (0 up, 1 down), real parts; sites A = y L + x; A = B (+) d periodic, bin
 * dy L + dx.  n_s = c^+_s c_s, n = n_up + n_dn, S^z = (n_up - n_dn) / 2; pair operators Delta_A = c_Aup c_Adn and
 * Delta^f_A = 1/2 sum_dl f_dl c_Aup c_(A+dl)dn over the four neighbours, f = +1 (extended s) or +1 on +-x, -1 on +-y (d wave).
 * Every block holds raw sums over B of X(B (+) d, B) per configuration and a sample counter: C_X(d) = sum / (count N).
 * Equal time -- a switch of dqmc_measure_slice: while on, every dqmc_measure_slice also bins, from the slice's own unshifted G,
 *   0 greenUp G_up(A,B)   1 greenDn G_dn(A,B)   2 charge <n_A n_B>   3 spinZZ <S^z_A S^z_B>   4 spinXX 1/4 <S^+_A S^-_B + S^-_A S^+_B>
 *   5 pairS <Delta_A Delta^+_B>   6 pairSx, 7 pairD <Delta^f_A Delta^f+_B>
 * with <c^+_As c_Bs> = delta_AB - G_s(B,A), <n_As n_Bs'> = <n_As><n_Bs'> + delta_ss' <c^+_As c_Bs> G_s(A,B),
 * <S^+_A S^-_B> = <c^+_Aup c_Bup> G_dn(A,B), <Delta_A Delta^+_B> = G_up(A,B) G_dn(A,B) and
 * <Delta^f_A Delta^f+_B> = 1/4 sum_{dl,dl'} f_dl f_dl' G_up(A,B) G_dn(A+dl, B+dl').  Block of one chain: count, then [8][N]
 * (dqmc_hubbard_eq_accum_size = 1 + 8 N doubles), allocated for all chains outside the arena by the first enable, freed with the
 * context, cleared by dqmc_measure_reset.  The block of dqmc_measure_read_host is the same either way.
 * Time-displaced -- context created with timedisplaced = 1 and td_particle_hole = 1 (the only values a Hubbard context accepts besides
 * 0, 0): dqmc_hubbard_measure_timedisplaced(ctx, j), right after the advance that ended on boundary j while dqmc_set_timedisplaced is
 * on, bins channels 0 .. 5 as <O_A(tau_j) O^+_B(0)> from G(tau,0), G(0,tau), G(tau), G(0) (conventions below): the equal-time forms with
 * G_s(A,B) -> G(tau,0)_s(A,B), <c^+_As c_Bs> -> -G(0,tau)_s(B,A), <n_As> from G(tau), <n_Bs> from G(0).  Block: count[n-1], then
 * [n-1][6][N].  All chains in one launch each; one writer per accumulator, fixed summation order, bit-reproducible.
 * DQMC_EINVAL: an SDW context; the time-displaced entries without the reservation or away from boundary j. */
int dqmc_hubbard_set_equal_time_correlators(dqmc_ctx* ctx, int on);
size_t dqmc_hubbard_eq_accum_size(dqmc_ctx* ctx);       /* 0 before the first enable */
int dqmc_hubbard_eq_read_host(dqmc_ctx* ctx, double* out);   /* selected chain */
int dqmc_hubbard_measure_timedisplaced(dqmc_ctx* ctx, int j);
size_t dqmc_hubbard_td_accum_size(dqmc_ctx* ctx);       /* 0 without the reservation */
int dqmc_hubbard_td_read_host(dqmc_ctx* ctx, double* out);   /* selected chain */
/* Every time slice, tau_k = k dtau, k = 0 .. m -- context created with timedisplaced = 1 | DQMC_TD_HUB_EVERY_SLICE and td_particle_hole = 1
 * (DESIGN.md 24).  The propagation identities, preconditions and slice bookkeeping are those of dqmc_measure_timedisplaced_segment / _ends
 * below (the same work copies, the same B-multiplies: G, the boundary pair and G(0) come out bit-identical):
 * dqmc_hubbard_measure_timedisplaced_segment(ctx, j) bins rows k = j s .. min((j+1) s, m) - 1 and, for j = 1, k = s-1 .. 1;
 * dqmc_hubbard_measure_timedisplaced_ends(ctx), at time slice 0 or m, rows 0 and m from G(0+,0) = G, G(0,0+) = G - 1, G(beta-,0) = 1 - G,
 * G(0,beta-) = -G with G(tau) = G(0) = G.  Block of one chain (dqmc_hubbard_td_fine_accum_size = (m+1)(1 + 8 N) doubles, 0 without the
 * reservation; inside the arena, cleared by dqmc_measure_reset): count[m+1], then [m+1][8][N] raw sums in the channel order of the
 * equal-time block.  Channels 0 .. 5: the forms of dqmc_hubbard_measure_timedisplaced (row j s has the bits of coarse row j); channels 6, 7:
 * <Delta^f_A(tau) Delta^f+_B(0)> = 1/4 G(tau,0)_up(A,B) sum_{dl,dl'} f_dl f_dl' G(tau,0)_dn(A+dl, B+dl').  Two launches per row, all chains;
 * one writer per accumulator, fixed summation order.
 * Matsubara transforms of the block, all chains and all eight channels in ONE launch (k_hubbard_td_matsubara): with C_X(d, tau_k) =
 * row k / (count_k N), w_0 = w_m = 1/2 (1 otherwise), n = 0 .. nfreq-1, q = (2 pi / L)(qx, qy), column qy L + qx,
 *   channels 2 .. 7 (bosonic, omega_n = 2 pi n / beta):        chi_X(q, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i q d} C_X(d, tau_k)
 *   channels 0, 1 (fermionic, omega_n = (2n+1) pi / beta):     G_s(k, i omega_n)   = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i k d} G_s(d, tau_k)
 * out: [chain][8][nfreq][N] complex as (re, im), dqmc_hubbard_td_matsubara_size doubles (0 for arguments the call rejects).  DQMC_EINVAL,
 * with nothing written to out: nfreq outside 1 .. m, a row of any chain with a sample count < 1, a lattice beyond the kernel's LDS.  Reads
 * the block only; two calls give identical bits.  Every entry: DQMC_EINVAL on an SDW context or without the reservation. */
int dqmc_hubbard_measure_timedisplaced_segment(dqmc_ctx* ctx, int j);
int dqmc_hubbard_measure_timedisplaced_ends(dqmc_ctx* ctx);
size_t dqmc_hubbard_td_fine_accum_size(dqmc_ctx* ctx);  /* 0 without the reservation */
int dqmc_hubbard_td_fine_read_host(dqmc_ctx* ctx, double* out);   /* selected chain */
int dqmc_hubbard_td_fine_counts_host(dqmc_ctx* ctx, double* out);   /* selected chain: the m + 1 sample counts alone, the block's prefix */
size_t dqmc_hubbard_td_matsubara_size(dqmc_ctx* ctx, int nfreq);
int dqmc_hubbard_td_matsubara_host(dqmc_ctx* ctx, int nfreq, double* out);
/* ---- time-displaced Green's functions ----------------------------------------------------------
 * At an interior stabilisation boundary tau_j = j s (j = 1 .. n-1) the advance holds B(tau,0) = U_r D_r V_r^H and
 * B(beta,tau) = U_l D_l V_l^H at once.  With the scales split into their parts > 1 and <= 1 and
 *   Z = Drmax^-1 (U_r^H V_l) Dlmax^-1 + Drmin (V_r^H U_l) Dlmin
 * (the matrix the QR mode inverts for G anyway):
 *   G(tau)   =  [V_l Dlmax^-1] Z^-1 [Drmax^-1 U_r^H]
 *   G(tau,0) =  [B(tau,0)^-1 + B(beta,tau)]^-1 =  [V_l Dlmax^-1] Z^-1 [Drmin V_r^H]
 *   G(0,tau) = -[B(tau,0) + B(beta,tau)^-1]^-1 = -[U_l Dlmin] Z^-1 [Drmax^-1 U_r^H]
 * Needs a context created with dqmc_params::timedisplaced != 0 (DQMC_EINVAL otherwise).  While switched on, every
 * dqmc_advance that ends on an interior boundary also fills G(tau,0) and G(0,tau) of all chains: QR mode reuses the
 * factorisation of Z (two more triangular solves or Q applications and two GEMMs); SVD mode leaves G on its own path and
 * builds and factorises the split Z after it.  Switched off, nothing is computed. */
int dqmc_set_timedisplaced(dqmc_ctx* ctx, int on);
/* the last pair computed, selected chain; *slice = the tau slice s j it belongs to.  DQMC_EINVAL if none was computed yet */
int dqmc_get_green_timedisplaced_host(dqmc_ctx* ctx, dqmc_cplx* g_t0, dqmc_cplx* g_0t, int* slice);
/* bins the last pair's e^{-dtau K/2} G(tau_j,0) e^{+dtau K/2} (all chains; the pair must belong to boundary j) into a block of its
 * own.  Layout (doubles, dqmc_measure_td_accum_size of them): count[n-1] (samples per boundary), then for j = 1 .. n-1 the bins
 * S_X[(2L-1)^2] and S_Y[(2L-1)^2] as (re, im), defined like those of dqmc_measure_slice (spin summed, bin index
 * (dy + L-1) (2L-1) + (dx + L-1)), at offset (n-1) + (j-1) 4 (2L-1)^2.  dqmc_measure_reset clears it as well. */
int dqmc_measure_timedisplaced(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_accum_size(dqmc_ctx* ctx);       /* 0 without the reservation */
int dqmc_measure_td_read_host(dqmc_ctx* ctx, double* out);
/* Time-displaced pairing correlators from the same shifted matrix gs = e^{-dtau K/2} G(tau_j,0) e^{+dtau K/2} (all chains; same
 * preconditions as dqmc_measure_timedisplaced, and a context created with dqmc_params::timedisplaced == 2).  With the band-spin
 * access rule of the equal-time measurement (detsdwopdim.cpp:594-612) and, for a site pair (A, B),
 *   P(b1,b2) = gs(A b1 dn; B b2 up) gs(A b1 up; B b2 dn) - gs(A b1 dn; B b2 dn) gs(A b1 up; B b2 up)        (:695-715)
 *   T+ = -4 [P(X,X) + P(X,Y) + P(Y,X) + P(Y,Y)],   T- = -4 [P(X,X) - P(X,Y) - P(Y,X) + P(Y,Y)]
 * the block of boundary j receives  sum_B Re T+-(B (+) d, B)  for every periodic site difference d = (dx, dy), bin dy L + dx (dividing
 * by N and by the count gives the translation average).  Layout (doubles, dqmc_measure_td_pair_accum_size of them): count[n-1], then for
 * j = 1 .. n-1 the T+ sums [N] followed by the T- sums [N], at offset (n-1) + (j-1) 2N.  A block of its own: the layout of the block of
 * dqmc_measure_timedisplaced does not depend on it.  dqmc_measure_reset clears it as well. */
int dqmc_measure_timedisplaced_pair(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_pair_accum_size(dqmc_ctx* ctx);  /* 0 without the reservation */
int dqmc_measure_td_pair_read_host(dqmc_ctx* ctx, double* out);
/* Time-displaced particle-hole correlators (charge, spin-z, SDW order parameter); context created with td_particle_hole = 1.
 * While the time-displaced functions are switched on, an advance that ends on an interior boundary then also forms the equal-time
 *   G(0) = 1 - B(beta,tau) G(tau) B(tau,0) = 1 - [U_l Dlmin] Z^-1 [Drmin V_r^H]
 * of the SAME (half-updated) field configuration, one GEMM from the left factor of G(0,tau) and the right factor of G(tau,0).
 * With g~ = e^{-dtau K/2} g e^{+dtau K/2} for all four matrices, G(tau,0)_ab = <c_a(tau) c_b^+(0)>, G(0,tau)_ab = -<c_b^+(tau) c_a(0)>,
 * the band-spin order XUP, YDOWN, XDOWN, YUP and a site bilinear O^M_i = sum_ab c^+_ia M_ab c_ib (M a Hermitian 4 x 4 matrix):
 *   o^M_t(A) = tr M - sum_ab M_ab g~(t)(A b; A a)                                                            (t = tau, 0)
 *   W^M(A,B) = o^M_tau(A) o^M_0(B) - sum_abcd M_ab M_cd g~(0,tau)(B d; A a) g~(tau,0)(A b; B c)
 * Channels: charge M = 1; spinZ M = diag(+1,-1,-1,+1) / 2; sdw = (1/OPDIM) sum_{a < OPDIM} W^{M_a} with the inter-band spin bilinears
 *   M_x: (0,1) = (1,0) = (2,3) = (3,2) = 1;   M_y: (0,1) = -i, (1,0) = +i, (2,3) = +i, (3,2) = -i;   M_z: (0,3) = (3,0) = 1, (1,2) = (2,1) = -1.
 * dqmc_measure_timedisplaced_ph(j) (all chains) adds sum_B Re W(B (+) d, B) for every periodic site difference d = (dx, dy), bin
 * dy L + dx, to the block of boundary j.  Preconditions: the last pair belongs to boundary j AND the context still stands on that
 * boundary (G is the G(tau_j) the advance produced: call it before the next wrap or update); DQMC_EINVAL otherwise.
 * Layout (doubles, dqmc_measure_td_ph_accum_size of them): count[n-1], then for j = 1 .. n-1 the charge sums [N], the spinZ sums [N]
 * and the sdw sums [N], at offset (n-1) + (j-1) 3N; dividing by N and by the count gives the translation average.
 * dqmc_measure_reset clears the block as well. */
int dqmc_measure_timedisplaced_ph(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_ph_accum_size(dqmc_ctx* ctx);    /* 0 without the reservation */
int dqmc_measure_td_ph_read_host(dqmc_ctx* ctx, double* out);
/* Time-displaced current-current correlators Lambda_xx, Lambda_yy and the bond kinetic energy; context created with td_particle_hole = 2.
 * Full index space: flavour N + site, flavour order XUP, YDOWN, XDOWN, YUP; engine matrices expanded by the access rule of the equal-time
 * measurement (OPDIM < 3: stored sector, its conjugate, zeros).  K^a is the hopping matrix of flavour a, the one the dense propagator
 * e^{-dtau K} is built from: band X for XUP / XDOWN, band Y for YDOWN / YUP, t*hor on x bonds, t*ver on y bonds, APBC sign on bonds that
 * cross the boundary, with flux the Peierls phase of the stored sector, complex conjugated for the flavours of the conjugate sector.
 * For a direction mu in {x, y}, a site i and i' = i (+) mu let T_a(i) = K^a[i', i], the coefficient of c^+_{i' a} c_{i a}:
 *   current              j_mu(i) = sum_a i [ T_a(i) c^+_{i' a} c_{i a} - conj T_a(i) c^+_{i a} c_{i' a} ]
 *   bond kinetic energy  k_mu(i) = sum_a   [ T_a(i) c^+_{i' a} c_{i a} + h.c. ]
 * and for a one-body operator O = sum_pq c^+_p M_pq c_q on the four shifted matrices g~ of a boundary (conventions as above)
 *   o_t[M]      = tr M - sum_pq M_pq g~_t(q, p)
 *   W[M_A, M_B] = o_tau[M_A] o_0[M_B] - sum_pqrs (M_A)_pq (M_B)_rs g~(0,tau)(s, p) g~(tau,0)(q, r).
 * dqmc_measure_timedisplaced_current(j) (all chains) adds to the block of boundary j, for every periodic site difference d = (dx, dy),
 * bin dy L + dx,  sum_B Re W[j_mu(B (+) d), j_mu(B)]  for mu = x and mu = y, and the two sums  sum_A Re o_tau[k_mu(A)]  (the diamagnetic
 * term, from g~(tau_j)).  Preconditions and DQMC_EINVAL behaviour of dqmc_measure_timedisplaced_ph; the call prepares its own shifted
 * matrices, leaves G and the other measurement blocks alone and works in either order with the other calls of the boundary.
 * Layout (doubles, dqmc_measure_td_current_accum_size of them): count[n-1], then for j = 1 .. n-1 the Lambda_xx sums [N], the Lambda_yy
 * sums [N], sum_A Re o_tau[k_x] and sum_A Re o_tau[k_y], at offset (n-1) + (j-1) (2N + 2); dividing by N and by the count gives the
 * translation averages.  The superfluid density
 *   rho_s = 1/4 [ Lambda_xx(q_x -> 0, q_y = 0, i omega = 0) - Lambda_xx(q_x = 0, q_y -> 0, i omega = 0) ]
 * needs the tau quadrature and the smallest non-zero q: with DQMC_TD_EVERY_SLICE, dqmc_measure_td_matsubara_host (below) forms
 * Lambda_mumu(q, i omega_n) on the device; a reader of the coarse block does it itself.  dqmc_measure_reset clears the block as well. */
int dqmc_measure_timedisplaced_current(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_current_accum_size(dqmc_ctx* ctx);   /* 0 without the reservation */
int dqmc_measure_td_current_read_host(dqmc_ctx* ctx, double* out);
/* Band-resolved charge correlators; context created with td_particle_hole = 1 | DQMC_TD_PH_BAND or 2 | DQMC_TD_PH_BAND.  The W^M(A,B) of
 * dqmc_measure_timedisplaced_ph, on the same four shifted matrices, for the two spin-singlet bilinears the channels above leave out:
 *   bandDiff  M_BAND = diag(+1, -1, +1, -1):  n_x - n_y.  q = 0: the B1g (nematic) susceptibility; q = (pi, pi): the d-wave charge-density
 *             wave sum_s (psi^+_xs psi_xs - psi^+_ys psi_ys), the particle-hole partner of pairMinus
 *   bandMix   M_MIX: (0,3) = (3,0) = (1,2) = (2,1) = +1:  sum_s (psi^+_xs psi_ys + h.c.), M_z of the sdw channel with the relative sign of
 *             the two spin species flipped: the charge partner of the SDW order parameter
 *   o^M_t(A) = tr M - sum_ab M_ab g~_t(A b; A a),   W^M(A,B) = o^M_tau(A) o^M_0(B) - sum_abcd M_ab M_cd g~(0,tau)(B d; A a) g~(tau,0)(A b; B c)
 * OPDIM < 3 (stored sector (XUP, YDOWN), its conjugate (XDOWN, YUP)): M_BAND is sector diagonal with the same signs in both sectors, so
 * its connected part is 4 x that of spinZ and o = -2 Re (g~_00 - g~_11) where spinZ has -i Im of the same number; M_MIX couples the two
 * sectors, o = 0 exactly and every connected term is a product of one element of each sector (kernels_measure.hip).
 * dqmc_measure_timedisplaced_band(j) (all chains) adds sum_B Re W(B (+) d, B) for every periodic site difference d = (dx, dy), bin
 * dy L + dx, to the block of boundary j.  Preconditions and DQMC_EINVAL behaviour of dqmc_measure_timedisplaced_ph; the call prepares its
 * own shifted matrices, leaves G and the other measurement blocks alone and works in either order with the other calls of the boundary.
 * Layout (doubles, dqmc_measure_td_band_accum_size of them): count[n-1], then for j = 1 .. n-1 the bandDiff sums [N] and the bandMix
 * sums [N], at offset (n-1) + (j-1) 2N; raw sums: dividing by N and by the count gives the translation average.  dqmc_measure_reset
 * clears the block as well. */
int dqmc_measure_timedisplaced_band(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_band_accum_size(dqmc_ctx* ctx);  /* 0 without the reservation */
int dqmc_measure_td_band_read_host(dqmc_ctx* ctx, double* out);
/* User-defined bilinears ("customBilinears"): the same W^M(A,B), and its equal-time form, for up to DQMC_CUSTOM_MAX Hermitian 4 x 4
 * matrices M in band-spin space (order XUP, YDOWN, XDOWN, YUP) that are set at run time -- any on-site particle-hole bilinear
 * O^M_i = sum_ab c^+_ia M_ab c_ib of the two-band model: one band's in-plane spin (XUP <-> XDOWN), n_x alone, ...  SDW model only.
 * dqmc_set_custom_bilinears(ctx, count, M): M[count][4][4] row-major, count = 0 .. DQMC_CUSTOM_MAX.  DQMC_EINVAL with nothing changed: a
 * count out of range, an entry that is not finite, M[a][b] != conj(M[b][a]) (compared exactly), a matrix that is all zero, a Hubbard
 * context.  On success the blocks of an earlier call are released and new, cleared ones allocated outside the arena: the equal-time block
 * 1 + count N; on a context created with td_particle_hole >= 1 the coarse block (n-1)(1 + count N); with DQMC_TD_EVERY_SLICE as well the fine
 * block (m+1)(1 + count N), every-slice channel 5, filled by dqmc_measure_timedisplaced_segment / _ends and transformed by
 * dqmc_measure_td_matsubara_host(5) into [count][nfreq][N] like the other channels.  count = 0 removes them (and switches
 * dqmc_set_equal_time_custom off; a replacement leaves the switch as it is).  The matrices travel to the kernels as a launch argument; OPDIM < 3 keeps only the
 * (XUP, YDOWN) sector of a Green's function, the (XDOWN, YUP) sector is its complex conjugate and the blocks between them vanish -- a
 * matrix that couples the two sectors is legal.  dqmc_get_custom_bilinears reads count and the matrices back (M may be NULL).
 * dqmc_measure_timedisplaced_custom(j) (all chains, every set matrix in one launch): preconditions, DQMC_EINVAL behaviour and independence
 * of dqmc_measure_timedisplaced_band.  Layout (doubles, dqmc_measure_td_custom_accum_size of them): count[n-1], then for j = 1 .. n-1
 * `count` rows of N raw sums sum_B Re W(B (+) d, B), bin dy L + dx, at offset (n-1) + (j-1) count N.
 * dqmc_set_equal_time_custom(on): a third switch of dqmc_measure_slice, independent of the other two (DQMC_EINVAL while no matrix is set):
 * one shifted matrix in every role, the delta term sum_bc (M^2)_cb g~(B b; B c) in the d = 0 bin (M^2 = 1 is not assumed).  Layout
 * (dqmc_measure_eq_custom_accum_size doubles): count, then `count` rows of N raw sums.  dqmc_measure_reset clears both blocks. */
#define DQMC_CUSTOM_MAX 4
int dqmc_set_custom_bilinears(dqmc_ctx* ctx, int count, const dqmc_cplx* M);
int dqmc_get_custom_bilinears(dqmc_ctx* ctx, int* count, dqmc_cplx* M);
int dqmc_measure_timedisplaced_custom(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_custom_accum_size(dqmc_ctx* ctx);  /* 0 without matrices or without td_particle_hole */
int dqmc_measure_td_custom_read_host(dqmc_ctx* ctx, double* out);
int dqmc_set_equal_time_custom(dqmc_ctx* ctx, int on);
size_t dqmc_measure_eq_custom_accum_size(dqmc_ctx* ctx);  /* 0 while no matrix is set */
int dqmc_measure_eq_custom_read_host(dqmc_ctx* ctx, double* out);
/* Bond (form-factor) parts of the user-defined bilinears.  Operator c is given by three 4 x 4 matrices: M0 (Hermitian, the on-site part as
 * above) and Mx, My (arbitrary complex) on the bonds A -> A (+) x and A -> A (+) y, the Hermitian conjugate added by the library:
 *   O_A = sum_ab c^+_{A a} M0_ab c_{A b} + sum_{mu = x, y} sum_ab [ u^ab_mu(A) Mmu_ab c^+_{A (+) mu, a} c_{A b} + h.c. ]
 * u is the unit-modulus link factor the hopping bond carries (antiperiodic sign times Peierls phase, built from bc and the flux): without
 * flux +-1 for every entry; with weakZflux entry (a, a) takes flavour a's link and a non-zero flavour-off-diagonal entry of Mx or My
 * has no covariant definition.  As a one-body matrix over (site, flavour) O_A has the blocks (A, A) = M0, (A (+) mu, A) = u Mmu,
 * (A, A (+) mu) = (u Mmu)^H, and the correlators are the definitions above with that matrix:
 *   o_t(A) = tr M0 - sum_ij (O_A)_ij g_t(j; i),    W(A, B) = o_tau(A) o_0(B) - sum_ijkl (O_A)_ij (O_B)_kl g0t(l; i) gt0(j; k),
 * equal-time with gt0 -> g~ and g0t -> g~ - 1, the delta wherever two stencil sites coincide.
 * dqmc_set_custom_bond_bilinears(ctx, count, M0, Mx, My): each array [count][4][4] row-major; Mx and My may be NULL (all zero).  It
 * replaces whatever an earlier call of either setter left, with the side effects of dqmc_set_custom_bilinears, and returns DQMC_EINVAL
 * with nothing changed for a count out of range, an entry that is not finite, an M0 that is not Hermitian, an operator whose three
 * parts are all zero (M0 = 0 with a bond part is legal), an off-diagonal bond entry under weakZflux, a series with a custom part open,
 * a Hubbard context.  While at least one operator has a bond part, dqmc_measure_timedisplaced_custom, the every-slice channel 5 and
 * dqmc_set_equal_time_custom run the stencil kernels for every set operator; blocks, sizes and layouts are the ones above.
 * dqmc_set_custom_bilinears clears every bond part; dqmc_get_custom_bilinears keeps returning count and the M0.
 * dqmc_get_custom_bond_bilinears reads all three back (each array may be NULL). */
int dqmc_set_custom_bond_bilinears(dqmc_ctx* ctx, int count, const dqmc_cplx* M0, const dqmc_cplx* Mx, const dqmc_cplx* My);
int dqmc_get_custom_bond_bilinears(dqmc_ctx* ctx, int* count, dqmc_cplx* M0, dqmc_cplx* Mx, dqmc_cplx* My);
/* User-defined pair operators ("customPair"): the pairing channel of the user-defined bilinears.  Operator c = 0 .. DQMC_CUSTOM_MAX - 1
 * is three complex 4 x 4 matrices (F0, Fx, Fy) in the band-spin order XUP, YDOWN, XDOWN, YUP:
 *   Delta_A = sum_ab F0_ab c_{A a} c_{A b} + sum_{mu = x, y} u_mu(A) sum_ab Fmu_ab c_{A (+) mu, a} c_{A b}
 * u_mu(A) = +-1 the antiperiodic sign of the bond A -> A (+) mu, so that Delta_A is translation-covariant under apbc-*.  Delta is not
 * Hermitian and no Hermitian conjugate is added.  Only the antisymmetric part of F0 contributes; any F0 is accepted.  With bonds
 * A -> A (+) x and A -> A (+) y only, a bond operator is bond-centred: its q = 0 sums equal those of the four-bond operator up to a
 * constant factor.  Measured is
 *   P_c(A, B; tau) = <Delta_A(tau) Delta_B^+(0)> = sum_ijkl D^A_ij conj(D^B_kl) [g(i; k) g(j; l) - g(i; l) g(j; k)],
 * g the shifted G(tau,0) over (flavour, site), D_A the dense coefficient matrix of Delta_A with the site blocks (A, A) = F0,
 * (A (+) mu, A) = u_mu Fmu.  A particle-conserving ensemble has no anomalous average: no disconnected term, and G(tau,0) alone is
 * needed.  At equal time the same expression on the shifted G of the slice (<c c c^+ c^+> has no delta term).  Binned as every other
 * correlator, C_c(d) = (1/N) sum_B Re P_c(B (+) d, B), bin dy L + dx, with NO factor 4: F0[XUP, XDOWN] = 1, F0[YUP, YDOWN] = +-1
 * gives pairPlus / pairMinus of dqmc_measure_timedisplaced_pair divided by 4.
 * dqmc_set_custom_pair_operators(ctx, count, F0, Fx, Fy): each array [count][4][4] row-major, Fx and Fy may be NULL (all zero), count = 0
 * removes the operators.  Run-time state like dqmc_set_custom_bilinears and independent of it: neither call touches the other's
 * operators or blocks.  The call allocates the blocks below outside the arena (a failed allocation leaves the context as it was); a
 * second call replaces the operators and clears the blocks; the equal-time switch outlives a replacement, not the removal.  With no
 * operator set no kernel of this section is launched and every other block, launch count and result keeps its bits.  DQMC_EINVAL
 * with nothing changed: count out of range, an entry that is not finite, an operator that vanishes identically (F0 - F0^T = 0 with Fx =
 * Fy = 0), a non-zero bond entry under weakZflux (the two fermions of a bond pair sit on different sites and carry flavour-dependent
 * Peierls phases; no gauge choice is made here -- on-site operators are allowed under flux, the formula applied as it stands like the
 * fixed channels), a Hubbard context, a series with a pair part open.  dqmc_get_custom_pair_operators reads count and the three
 * arrays back (each may be NULL).
 * dqmc_measure_timedisplaced_custom_pair(j) (all chains, every operator in one launch): preconditions of
 * dqmc_measure_timedisplaced_pair; needs only timedisplaced >= 1.  Layout (doubles, dqmc_measure_td_custom_pair_accum_size of them):
 * count[n-1], then for j = 1 .. n-1 `count` rows of N raw sums over B of Re P_c(B (+) d, B).  Every-slice channel 6 with
 * DQMC_TD_EVERY_SLICE (row stride count N).
 * dqmc_set_equal_time_custom_pair(on): a fourth switch of dqmc_measure_slice, independent of the other three (DQMC_EINVAL while no
 * operator is set).  Block (dqmc_measure_eq_custom_pair_accum_size doubles): count, then `count` rows of N raw sums.
 * dqmc_measure_reset clears all blocks. */
int dqmc_set_custom_pair_operators(dqmc_ctx* ctx, int count, const dqmc_cplx* F0, const dqmc_cplx* Fx, const dqmc_cplx* Fy);
int dqmc_get_custom_pair_operators(dqmc_ctx* ctx, int* count, dqmc_cplx* F0, dqmc_cplx* Fx, dqmc_cplx* Fy);
int dqmc_measure_timedisplaced_custom_pair(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_custom_pair_accum_size(dqmc_ctx* ctx);  /* 0 without operators or without timedisplaced */
int dqmc_measure_td_custom_pair_read_host(dqmc_ctx* ctx, double* out);
int dqmc_set_equal_time_custom_pair(dqmc_ctx* ctx, int on);
size_t dqmc_measure_eq_custom_pair_accum_size(dqmc_ctx* ctx);  /* 0 while no operator is set */
int dqmc_measure_eq_custom_pair_read_host(dqmc_ctx* ctx, double* out);
/* The averaged Green's function block ("greenMatrix"): what the pairing bubble Pbar, the Wick form on the ensemble-averaged <G(tau,0)>, is
 * built from (dqmc_series_pair_vertex_host below).  SDW model only.  dqmc_set_green_matrix(ctx, on) is run-time state like the operators
 * above; switching on allocates the blocks below, cleared, outside the arena (a failed allocation leaves the context as it was), switching
 * off releases them; a repeated call changes nothing.  While on, every place that measures a time-displaced row -- the coarse call
 * dqmc_measure_timedisplaced_green_matrix(j) (preconditions of dqmc_measure_timedisplaced_pair), dqmc_measure_timedisplaced_segment and
 * dqmc_measure_timedisplaced_ends -- adds, from the shifted g~ = e^{-dtau K/2} G(tau,0) e^{+dtau K/2} the pair kernels read,
 *   Gbar_rc(d; tau) += sum_B sigma(B, d) g~((B (+) d) r; B c),   d = (dx, dy) periodic, bin dy L + dx,
 * r, c over the stored flavour block (R = 2 for O(1) and O(2): the (XUP, YDOWN) sector; R = 4 for O(3)), sigma(B, d) = -1 for each
 * antiperiodic direction in which B + d wraps (bx + dx >= L, likewise in y), +1 otherwise.  With this sign the summand does not depend on
 * B in a translation-invariant ensemble (G(P + L e_mu, Q) = -G(P, Q) along an antiperiodic direction), and the full matrix is recovered as
 *   gbar(P r; Q c) = sigma(Q, P (-) Q) Gbar_rc(P (-) Q) / (N count);
 * for OPDIM < 3 the (XDOWN, YUP) sector is the complex conjugate of the stored one and the blocks between the sectors vanish, element by
 * element and therefore for averages too.  One launch per row over all chains, one writer per accumulator, fixed summation order, no
 * atomics: bits do not depend on how chains are batched.
 * Layout of the coarse block (doubles, dqmc_measure_td_green_matrix_accum_size of them, 0 while off): count[n-1], then for j = 1 .. n-1 a
 * row [N][R][R] of raw sums as (re, im), 2 R^2 N doubles.  Every-slice channel 7 with DQMC_TD_EVERY_SLICE: count[m+1], then rows k = 0 .. m
 * of the same form; dqmc_measure_td_fine_accum_size(ctx, 7) is 0 while the switch is off.  The channel has no Matsubara transform
 * (dqmc_measure_td_matsubara_size(ctx, 7, .) is 0, the call returns DQMC_EINVAL): channel 0 serves G(k, i omega_n).  dqmc_measure_reset
 * clears both blocks.  With the switch off no kernel of this section is launched and every other block, launch count and result keeps
 * its bits.  DQMC_EINVAL with nothing changed: a Hubbard context; switching on under weakZflux (<G> is invariant under magnetic
 * translations only; no gauge choice is made here) or on a context created without timedisplaced >= 1; switching off while a series
 * holds DQMC_SERIES_GREEN_MATRIX. */
int dqmc_set_green_matrix(dqmc_ctx* ctx, int on);
int dqmc_measure_timedisplaced_green_matrix(dqmc_ctx* ctx, int j);
size_t dqmc_measure_td_green_matrix_accum_size(dqmc_ctx* ctx);  /* 0 while the switch is off */
int dqmc_measure_td_green_matrix_read_host(dqmc_ctx* ctx, double* out);
/* G(0) of the last pair's field configuration, selected chain; *slice as for dqmc_get_green_timedisplaced_host.  DQMC_EINVAL without
 * td_particle_hole or if no pair was computed yet */
int dqmc_get_green0_timedisplaced_host(dqmc_ctx* ctx, dqmc_cplx* g00, int* slice);
/* Every time slice, tau_k = k dtau, k = 0 .. m (context created with timedisplaced | DQMC_TD_EVERY_SLICE; DQMC_EINVAL otherwise).
 * Inside ONE field configuration the functions of neighbouring slices follow from each other without a new factorisation:
 *   G(tau_{k+1},0) = B_{k+1} G(tau_k,0),   G(0,tau_{k+1}) = G(0,tau_k) B_{k+1}^-1,   G(tau_{k+1}) = B_{k+1} G(tau_k) B_{k+1}^-1,   G(0) unchanged
 *   G(tau_{k-1},0) = B_k^-1 G(tau_k,0),    G(0,tau_{k-1}) = G(0,tau_k) B_k,         G(tau_{k-1}) = B_k^-1 G(tau_k) B_k
 * and the end rows from the equal-time G(0) alone:
 *   G(0+,0) = G(0),  G(0,0+) = G(0) - 1,  G(beta-,0) = 1 - G(0),  G(0,beta-) = -G(0).
 * dqmc_measure_timedisplaced_segment(j) (all chains; preconditions of dqmc_measure_timedisplaced_ph: the last pair belongs to boundary j
 * and the context still stands on it) measures, with the fields as they are on the device at that moment, the slices
 * k = j s .. min((j+1) s, m) - 1 by upward propagation from the boundary's matrices and, for j = 1, also k = s-1 .. 1 by downward
 * propagation: at most s - 1 unstabilised steps, the distance of the equal-time wrap.  Calling it once at every boundary j = 1 .. n-1
 * hits every k in 1 .. m-1 exactly once, also when s does not divide m.  Propagation works on copies: G, the boundary pair and G(0)
 * come out bit-identical.  Per slice the four shifted matrices e^{-dtau K/2} g e^{+dtau K/2} are prepared once and handed to every
 * enabled channel kernel (the kernels, operands and summation order of dqmc_measure_timedisplaced, _pair, _ph and _current: row j s
 * equals row j of the coarse block bit for bit); the one-body values of G(0) are formed once per segment.
 * dqmc_measure_timedisplaced_ends() (all chains) measures rows 0 and m.  Precondition: the context stands at tau = 0 == beta
 * (current time slice 0 or m: the state after the closing advance of either sweep direction), so that G = G(0); DQMC_EINVAL
 * otherwise.  Both rows use G(tau) = G(0) = G.
 * Blocks: channel 0 = bins of dqmc_measure_timedisplaced, 1 = _pair, 2 = _ph, 3 = _current, 4 = _band (row stride 2N), 5 = _custom (row
 * stride count N, present while matrices are set), 6 = _custom_pair (row stride count N, present while pair operators are set), 7 = _green_matrix
 * (row stride 2 R^2 N, present while dqmc_set_green_matrix is on); a channel has a
 * block if its coarse block is reserved.  Layout (doubles, dqmc_measure_td_fine_accum_size of them, 0 without the block): count[m+1], then row k = 0 .. m
 * at offset (m+1) + k stride, stride and contents of a row as in the coarse block: 4 (2L-1)^2, 2N, 3N, 2N + 2.
 * dqmc_measure_reset clears them as well.  A Hubbard context returns DQMC_EINVAL from the segment, ends and Matsubara entries (its own:
 * dqmc_hubbard_measure_timedisplaced_segment / _ends, dqmc_hubbard_td_matsubara_host); with DQMC_TD_HUB_EVERY_SLICE the size / read pair
 * serves its one block as channel 0. */
int dqmc_measure_timedisplaced_segment(dqmc_ctx* ctx, int j);
int dqmc_measure_timedisplaced_ends(dqmc_ctx* ctx);
size_t dqmc_measure_td_fine_accum_size(dqmc_ctx* ctx, int channel);
int dqmc_measure_td_fine_read_host(dqmc_ctx* ctx, int channel, double* out);
/* Matsubara transforms of one every-slice block, all chains and all components of the block in ONE launch (kernels_measure.hip).
 * With C_X(d, tau_k) = row k of component X divided by N and by the row's sample count, the trapezoid weights w_0 = w_m = 1/2 (1 otherwise)
 * over the closed grid tau_k = k dtau, k = 0 .. m, and n = 0 .. nfreq-1 (1 <= nfreq <= m):
 *   channels 1, 2, 3, 4 (bosonic, omega_n = 2 pi n / beta):
 *     chi_X(q, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i q d} C_X(d, tau_k),  q = (2 pi / L)(qx, qy), column qy L + qx
 *   channel 0 (fermionic, omega_n = (2n+1) pi / beta), band X, Y:
 *     G_band(k, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} G_band(k, tau_k),  G_band(k, tau) = Re (Fourier sum over the bins) / 2N,
 *     column = the k-vector index of kOcc / greenKTau (k = -pi + (kk + 1/2 along antiperiodic directions) 2 pi / L); rows 0 and m as
 *     dqmc_measure_timedisplaced_ends wrote them.
 * out: [chain][component][nfreq][N] complex as (re, im), dqmc_measure_td_matsubara_size(ctx, channel, nfreq) doubles (0 for arguments
 * the call below rejects); component order = the block's order: X, Y / T+, T- / charge, spinZ, sdw / Lambda_xx, Lambda_yy (the two bond
 * kinetic sums of channel 3 are not transformed) / bandDiff, bandMix.  DQMC_EINVAL without the every-slice reservation, without that channel's block, for
 * nfreq outside 1 .. m, or if a row of any chain has a sample count < 1 (nothing is written to out then).  Reads the block only: G, the
 * pair, G(0) and every accumulator stay bit-identical; one writer per output element and a fixed summation order, so two calls give
 * identical bits.  The device result buffer lies outside the arena, is allocated on first use and freed with the context. */
size_t dqmc_measure_td_matsubara_size(dqmc_ctx* ctx, int channel, int nfreq);
int dqmc_measure_td_matsubara_host(dqmc_ctx* ctx, int channel, int nfreq, double* out);
/* ---- measurement series: bins over sweeps and jackknife errors on the device (the parts of a Hubbard context: below) ----------
 * One sample per measurement sweep, formed from the blocks above as they stand and accumulated into bins of bin_size sweeps; nothing is
 * copied per sweep.  All run-time calls: dqmc_params stays byte for byte.
 * parts (bit mask): bit 0 = the equal-time block (needs dqmc_measure_eq_accum_size != 0); bits 1 .. 4 = the Matsubara transform of
 * every-slice channel 0 .. 3 (each needs that channel's fine block and 1 <= nfreq <= m; nfreq is ignored without such a bit).
 * The sample of one chain has S doubles, the parts in mask order:
 *   bit 0:  C_X(d) [5][N] then S_X(q) [5][N], X = charge, spinZ, sdw, pairPlus, pairMinus:  C_X(d) = sum / (double(N) count) (one
 *           division), S_X(q) = sum_d cos(q d) C_X(d), column qy L + qx, the phase index reduced mod L in integers and the cos / sin of
 *           2 pi j / L taken from a table computed on the host
 *   bit 1 + channel:  what dqmc_measure_td_matsubara_host returns for (channel, nfreq), [component][nfreq][N] complex as (re, im) -- the
 *           same kernel, launched with the sample buffer as its target
 * dqmc_series_begin allocates, outside the arena, the sample [nb][S], the open bin [nb][S], the closed bins [max_bins][nb][S], the
 * per-part flags and the result buffer of the statistics calls.  DQMC_EINVAL: empty or unknown mask, a missing block, bin_size < 1,
 * max_bins < 2, a series already open, any of these parts on a Hubbard context, a lattice too large for the LDS of the Matsubara or sample kernel.
 * dqmc_series_layout: where part (= bit number 0 .. 4, 6: the order-parameter part, 7, 8: the band parts, 9 .. 13, 14 .. 16: the Hubbard parts, all below) sits inside S.
 * dqmc_series_add_sweep (all chains): forms the sample and adds it to the open bin, open += sample, in call order; the bin_size-th call
 * writes closed[k] = open / bin_size and clears the open bin.  DQMC_EINVAL with no bin changed: the equal-time count of any chain or a
 * fine row count of any chain and channel of the mask is < 1; max_bins bins are already closed (nothing is dropped silently, and there
 * is no re-binning unless DQMC_SERIES_AUTO_REBIN is set, below).  Reads the blocks only: G and every accumulator stay bit-identical.  dqmc_measure_reset does not touch the series.
 * The call synchronises (it reads the flags back, nb doubles per part).  It is dqmc_series_form_sample followed by
 * dqmc_series_accumulate(ctx, NULL):
 * A SLOT is a row of the series buffers (open bin, closed bins, statistics), indexed like a chain.  The two halves let a caller add the
 * sample of any chain of the device to any slot -- under replica exchange, the sample of the chain that holds control parameter s to slot s.
 * dqmc_series_form_sample (all chains): the sample of every chain from the blocks as they stand into the sample buffer, and the flags read
 * back.  The DQMC_EINVALs of dqmc_series_add_sweep: no series open, max_bins bins closed, a lattice too large for the LDS, a block without
 * a sample.  On success the context's sample is marked as formed; no counter moves and no bin is touched.  A second call forms the
 * sample again.
 * dqmc_series_sample_device: the device address of the sample buffer [nb][S] (chain b at *rows + b S) and S; valid from
 * dqmc_series_begin to dqmc_series_end.
 * dqmc_series_accumulate: src = host array of nb device pointers; slot s of this context does open[s] += src[s][0 .. S), and on the
 * bin_size-th call closed[k][s] = open[s] / bin_size with open[s] cleared -- the operations of dqmc_series_add_sweep, the same bits.
 * src == NULL: the context's own rows in order.  DQMC_EINVAL, with every bin and counter as it was and nothing launched: the context's
 * sample is not formed; an entry is null; an entry is not S doubles of device memory on the context's device (hipPointerGetAttributes
 * and the allocation's range: a wrong pointer is an error code, never a launch).  Clears the formed mark, moves the counters as
 * dqmc_series_add_sweep does and returns after the stream has finished, so every sample buffer it read may be rewritten afterwards.
 * Ordering rule: a context may read another context's sample rows only between that context's successful dqmc_series_form_sample and
 * its next dqmc_series_form_sample.  Both calls synchronise their own stream before they return; keeping to the rule across contexts
 * (and host threads) is the caller's job.  The readers below are indexed by slot.
 * dqmc_series_read_bins_host: closed bins first .. first + count - 1 of the selected chain, out[count][S] -- what a user persists.
 * dqmc_series_stats_host (all chains, mean and err [nb][S]): over the B closed bins x_b (DQMC_EINVAL for B < 2),
 *   mean = (1/B) sum_b x_b,   x_(b) = (B mean - x_b) / (B - 1),   err = sqrt((B - 1)/B sum_b (x_(b) - mean)^2).
 * dqmc_series_derived_host (all chains, value and err [nb][6]; entries whose part is not in the mask are NaN):
 *   0 .. 4:  R_X = 1 - 1/2 [S_X(Q + dx) + S_X(Q + dy)] / S_X(Q),  dx = (1,0), dy = (0,1) in units of 2 pi / L,  Q = (L/2, L/2) for
 *            charge, spinZ, sdw and (0,0) for pairPlus, pairMinus
 *   5:       rho_s = 1/8 Re [Lxx(1,0) - Lxx(0,1) + Lyy(0,1) - Lyy(1,0)] at frequency n = 0 of channel 3
 *   value = f(mean);  err = the jackknife over theta_(b) = f(x_(b)), about the mean of the theta_(b).
 * One writer per output element, fixed summation order (bins in index order), no atomics: bins and statistics do not depend on how
 * chains are batched, and two statistics calls give identical bits.  dqmc_series_end frees the buffers; dqmc_destroy does it too.
 * The order-parameter part, DQMC_SERIES_PHI = 64: bit 6 and part index 6 of dqmc_series_layout (bit 5 stays refused: with the band parts below the accepted
 * mask is 0x1df).  It needs no block -- the field phi(r, k), k = 1 .. m, always exists -- and no flag, so it may be the only part of a series; it
 * needs 1 <= nfreq <= m, and nfreq is stored in the state even when no Matsubara part is present.  It sits after all other parts and
 * holds nfreq N + 5 doubles:
 *   chi [nfreq][N], real, column qy L + qx.  With K = m N, q = 2 pi (qx, qy) / L, omega_n = 2 pi n / beta, n = 0 .. nfreq-1:
 *           A_d(n, q) = (1/K) sum_{k=1..m} sum_r phi_d(r, k) exp(i 2 pi n k / m - i 2 pi (qx x + qy y) / L),   chi(n, q) = sum_d |A_d(n, q)|^2
 *           (temporal sign +1, spatial sign -1, both normalisations inside A).  The physical susceptibility is beta N <chi(n, q)>.
 *           The temporal phases cos / sin(2 pi j / m), j = n k mod m reduced in integers, and the spatial ones come from host tables.
 *   scalars [5]:  |phibar| = sqrt(chi(0, 0));  |phibar|^2 = chi(0, 0), the bits of that chi element;  |phibar|^4 = (|phibar|^2)^2;
 *           the equal-time susceptibility (N/m) sum_k sum_d ((1/N) sum_r phi_d(r, k))^2;  associatedEnergy = sum phi^2 / (2 N m).
 * DQMC_EINVAL at dqmc_series_begin: nfreq outside 1 .. m, a lattice whose single-frequency tile exceeds the sample kernel's LDS.
 * dqmc_series_phi_derived_host (all chains, value and err [nb][6]; DQMC_EINVAL for B < 2 or a series without the part), the jackknife
 * of dqmc_series_derived_host, with beta = m dtau, chi0 = chi(0, (0,0)), chix = chi(0, column 1), chiy = chi(0, column L):
 *   0: Binder cumulant 1 - <|phibar|^4> / (3 <|phibar|^2>^2)      1: Binder ratio <|phibar|^4> / <|phibar|^2>^2
 *   2: beta N <|phibar|^2>                                        3: beta N (<|phibar|^2> - <|phibar|>^2)
 *   4: R_phi = 1 - 1/2 (chix + chiy) / chi0                       5: xi_phi = sqrt(chi0 / (1/2 (chix + chiy)) - 1) / (2 sin(pi / L)),
 *                                                                    NaN where the argument of the root is negative
 * The band parts: DQMC_SERIES_MATS_BAND = 128 (bit 7: the Matsubara transform of every-slice channel 4, [2][nfreq][N] complex) and
 * DQMC_SERIES_EQ_BAND = 256 (bit 8: the block of dqmc_set_equal_time_band as C_X(d) [2][N] then S_X(q) [2][N], X = bandDiff, bandMix, formed
 * like bit 0 with the same cosine table and integer phase reduction).  Parts sit in mask order: the two lie
 * behind the order-parameter part, and every mask without them keeps its S, its offsets and its bits.
 * dqmc_series_band_derived_host (all chains, value and err [nb][3]; DQMC_EINVAL for B < 2 or a series without bit 8), the jackknife of
 * dqmc_series_derived_host over R = 1 - 1/2 [S(Q + dx) + S(Q + dy)] / S(Q):
 *   0: bandDiff at Q = (L/2, L/2), the d-wave CDW     1: bandDiff at Q = (0, 0), the nematic     2: bandMix at Q = (L/2, L/2)
 * The parts of the user-defined bilinears (`count` matrices set by dqmc_set_custom_bilinears), behind all of the above so that every
 * older mask keeps its S, its offsets and its bits: DQMC_SERIES_MATS_CUSTOM = 512 (bit 9: the Matsubara transform of every-slice channel 5,
 * [count][nfreq][N] complex) and DQMC_SERIES_EQ_CUSTOM = 1024 (bit 10: the block of dqmc_set_equal_time_custom as C(d) [count][N] then
 * S(q) [count][N], formed like bit 8).  The accepted mask is 0x7df.  While a series with one of the two is open,
 * dqmc_set_custom_bilinears returns DQMC_EINVAL.  dqmc_series_custom_derived_host(qx, qy) (all chains, value and err [nb][count];
 * DQMC_EINVAL for B < 2, a series without bit 10, qx or qy outside 0 .. L-1): the same jackknife of R for every matrix at the caller's
 * Q = (qx, qy), in units of 2 pi / L.
 * The parts of the user-defined pair operators (dqmc_set_custom_pair_operators), behind all of the above again:
 * DQMC_SERIES_MATS_CUSTOM_PAIR = 2048 (bit 11: the Matsubara transform of every-slice channel 6, [count][nfreq][N] complex) and
 * DQMC_SERIES_EQ_CUSTOM_PAIR = 4096 (bit 12: the block of dqmc_set_equal_time_custom_pair as C(d) [count][N] then S(q) [count][N]).  Both
 * are refused (DQMC_EINVAL) while no pair operator is set; with them the accepted mask was 0x1fdf (0x3fdf with the part below).  While a series with one of the two is open,
 * dqmc_set_custom_pair_operators returns DQMC_EINVAL.  dqmc_series_custom_pair_derived_host(qx, qy): R of every pair operator at the
 * caller's Q by the routine of dqmc_series_custom_derived_host (value and err [nb][count]; DQMC_EINVAL for B < 2, a series without
 * bit 12, qx or qy outside 0 .. L-1).
 * The part of the averaged Green's function, DQMC_SERIES_GREEN_MATRIX = 8192 (bit 13, part index 13), behind all of the above: the
 * normalised every-slice block of dqmc_set_green_matrix, Gbar_rc(d, tau_k) / (double(N) count) (one division), [m+1][N][R][R] complex as
 * (re, im), formed by one launch.  It costs (m+1) 2 R^2 N doubles per chain and bin -- 0.8 MB at O(2), L = 16, m = 100 -- so max_bins is
 * sized accordingly.  Refused (DQMC_EINVAL) unless the switch is on and the context has DQMC_TD_EVERY_SLICE; the accepted mask is 0x3fdf.
 * Bins, re-binning, the running variance, routing, export and import treat it like every other part, through S alone.
 * dqmc_series_pair_vertex_host(qx, qy) (all slots, every pair operator c; value and err [nb][count][5 + m],
 * dqmc_series_pair_vertex_size doubles each, 0 where the call is refused): bubble and interaction vertex with jackknife errors.  For one
 * set of bin means x -- the mean, or a leave-one-out mean x_(b) = (B mean - x_b) / (B - 1) -- with gbar(tau_k) rebuilt from part 13 of x:
 *   Pbar_c(d, tau_k) = Re sum_ijkl D^d_ij conj(D^0_kl) [gbar(i; k) gbar(j; l) - gbar(i; l) gbar(j; k)]   (D of dqmc_set_custom_pair_operators
 *                      with its link signs; gbar is translation-covariant, so the site pair (B (+) d, B) is evaluated at B = 0)
 *   Pbar_c(Q, tau_k) = sum_d cos(Q d) Pbar_c(d, tau_k),   Pbar_c = dtau sum_k w_k Pbar_c(Q, tau_k),  w_0 = w_m = 1/2
 *   P_c = Re chi_c(Q, i omega_0) of part 11,   Gamma_c = 1 / P_c - 1 / Pbar_c,   Gamma Pbar_c = Pbar_c / P_c - 1.
 * Output per slot and operator: P, Pbar, Gamma, Gamma Pbar, then Pbar_c(Q, tau_k) for k = 0 .. m.  value = f(mean); err = the jackknife
 * over theta_(b) = f(x_(b)) about the mean of the theta_(b), as dqmc_series_derived_host; an entry with a vanishing denominator is NaN.
 * Gamma Pbar -> -1 marks the pairing instability; its sign says attractive or repulsive.  Two kernels: one workgroup per (slot, jackknife
 * index, row) stages the row in LDS and reduces over d in a fixed tree; the second sums over k and the bins in index order.  No atomics:
 * two calls give identical bits and a slot's result does not depend on batching.  DQMC_EINVAL: a series without bit 11 or bit 13, B < 2,
 * qx or qy outside 0 .. L-1, a lattice whose row does not fit the LDS (2 R^2 N doubles + 8 KiB > 152 KiB).
 * dqmc_series_ph_vertex_host(qx, qy) (all slots, every user-defined bilinear c = (M0, Mx, My) of dqmc_set_custom_bond_bilinears; value and
 * err [nb][count][6 + m], dqmc_series_ph_vertex_size doubles each, 0 where the call is refused): the particle-hole counterpart, from parts
 * 9 and 13.  No new part, flag or block: without the call nothing changes.  For one set of bin means x, with the five site blocks
 * V_k(A) = f_k(A) W_k of the bond section and
 *   gbar(0,tau_k)(P; Q) = -gbar(tau_{m-k},0)(P; Q),  k = 0 .. m     (cyclic invariance of the weight: exact in the ensemble average,
 *                      element by element and so for the stored sector too; the end rows obey it as measured and carry the delta term)
 *   chibar_c(d, tau_k) = -sum_(k, k') Re f_k(A) f_k'(B) tr(W_k gbar(tau_k,0)^(qr) W_k' gbar(0,tau_k)^(sp)),   (A, B) = (d, 0): the connected
 *                      Wick term of W(A, B) with gbar in the place of g~, site superscripts as in the bond section
 *   chibar_c(Q, tau_k) = sum_d cos(Q d) chibar_c(d, tau_k),   chibar_c = dtau sum_k w_k chibar_c(Q, tau_k),  w_0 = w_m = 1/2
 *   obar_c = tr M0 - sum_ij (O_0)_ij gbar(tau_0,0)(j; i)   (site 0, row 0),   D_c = beta Re(obar_c^2) sum_d cos(Q d)   (beta N Re obar_c^2
 *                      at Q = 0, else 0: the disconnected part that channel 5 carries)
 *   chi_c = Re chi_c(Q, i omega_0) of part 9 - D_c,   Gamma_c = 1 / chi_c - 1 / chibar_c,   Gamma chibar_c = chibar_c / chi_c - 1.
 * Output per slot and operator: chi, chibar, Gamma, Gamma chibar, D, then chibar_c(Q, tau_k) for k = 0 .. m.  Normalisation per site pair
 * as the Matsubara transform; on a free matrix chi_c = chibar_c to rounding at every Q.  value, err, NaN rule, kernel pair, fixed
 * summation order (no atomics, identical bits, independent of batching) as dqmc_series_pair_vertex_host; the bubble kernel stages rows
 * k and m - k.  DQMC_EINVAL with nothing touched: a series without bit 9 or bit 13, B < 2, qx or qy outside 0 .. L-1, no bilinear set, a
 * lattice whose two rows do not fit the LDS (4 R^2 N doubles + 8 KiB > 152 KiB). */
/* The parts of a Hubbard context, behind all of the above (every older mask keeps its S, its offsets and its bits).  A Hubbard context
 * accepts any non-empty subset of 0x1c000 and no other bit; an SDW context keeps its mask 0x3fdf and refuses the three; every refusal is
 * DQMC_EINVAL with nothing allocated.  nfreq is ignored on a Hubbard context and stored as 0.  Formed from the blocks as they stand:
 *   DQMC_SERIES_HUB_SCALARS = 16384 (bit 14, 8 + N doubles; needs nothing: the block of dqmc_measure_slice always exists): from
 *     a[0 .. 5 + N] of dqmc_measure_read_host with cnt = a[5] and K = N cnt: occUp = 1 - a[0] / K, occDn = 1 - a[1] / K, occTotal,
 *     occDouble = 1 + (a[4] - a[0] - a[1]) / K, localMoment = occTotal - 2 occDouble, eKinetic = txhor (a[2] + a[3]) / K - mux occTotal,
 *     ePotential = u occDouble, eTotal, in this order, then zcorr[j] = a[6 + j] / cnt.  The chain is flagged if cnt < 1.
 *   DQMC_SERIES_HUB_EQ = 32768 (bit 15, 16 N; needs dqmc_hubbard_eq_accum_size != 0): C_X(d) [8][N] then S_X(q) [8][N], X = greenUp,
 *     greenDn, charge, spinZZ, spinXX, pairS, pairSx, pairD, formed like bit 0 by the same kernel.
 *   DQMC_SERIES_HUB_TD = 65536 (bit 16, 12 (n-1) N; needs dqmc_hubbard_td_accum_size != 0 and n >= 2): C_X(d, tau_j) [n-1][6][N] =
 *     sum / (double(N) count_j) in the layout of the block, then S_X(q, tau_j) [n-1][6][N] by the cosine sum of bit 0 (same table, same
 *     integer phase reduction, same order); for greenUp, greenDn the second half is Re G_s(k = q, tau_j).  Flagged if any count_j < 1.
 * dqmc_series_hubbard_derived_host(qx, qy) (all chains, value and err [nb][19]; DQMC_EINVAL with nothing touched for a series without bit
 * 15, B < 2, qx or qy outside 0 .. L-1).  With Q = (qx, qy), Sbar_X = 1/2 [S_X(Q + dx) + S_X(Q + dy)], indices mod L:
 *   0 .. 7:   R_X = 1 - Sbar_X / S_X(Q) for the eight channels
 *   8 .. 15:  xi_X = sqrt(S_X(Q) / Sbar_X - 1) / (2 sin(pi / L))
 *   16 .. 18: S(Q), R and xi of the rotation-summed spin channel S_spin = S_spinZZ + 2 S_spinXX (= <S.S>), summed bin by bin
 * value = f(bin mean), err = the jackknife of dqmc_series_derived_host.  value is NaN where the root's argument of f(mean) is negative or
 * a denominator vanishes; err is NaN where that holds for the mean or for any leave-one-out set; no other entry is affected.
 * Everything else -- accumulate, routed accumulate, re-binning, running variance, statistics, binning analysis, export / import --
 * treats a sample as S doubles and serves these parts unchanged. */
enum { DQMC_SERIES_HUB_SCALARS = 16384, DQMC_SERIES_HUB_EQ = 32768, DQMC_SERIES_HUB_TD = 65536 };
int dqmc_series_hubbard_derived_host(dqmc_ctx* ctx, int qx, int qy, double* value, double* err);
enum { DQMC_SERIES_EQ = 1, DQMC_SERIES_MATS_G = 2, DQMC_SERIES_MATS_PAIR = 4, DQMC_SERIES_MATS_PH = 8, DQMC_SERIES_MATS_CURRENT = 16,
       DQMC_SERIES_PHI = 64, DQMC_SERIES_MATS_BAND = 128, DQMC_SERIES_EQ_BAND = 256, DQMC_SERIES_MATS_CUSTOM = 512, DQMC_SERIES_EQ_CUSTOM = 1024,
       DQMC_SERIES_MATS_CUSTOM_PAIR = 2048, DQMC_SERIES_EQ_CUSTOM_PAIR = 4096, DQMC_SERIES_GREEN_MATRIX = 8192 };
int dqmc_series_begin(dqmc_ctx* ctx, int bin_size, int max_bins, int nfreq, int parts);
int dqmc_series_layout(dqmc_ctx* ctx, int part, size_t* offset, size_t* length);
int dqmc_series_add_sweep(dqmc_ctx* ctx);
int dqmc_series_form_sample(dqmc_ctx* ctx);
int dqmc_series_sample_device(dqmc_ctx* ctx, const double** rows, size_t* S);
int dqmc_series_accumulate(dqmc_ctx* ctx, const double* const* src);
int dqmc_series_info(dqmc_ctx* ctx, int* bins_closed, int* sweeps_in_open_bin, size_t* sample_len);
int dqmc_series_read_bins_host(dqmc_ctx* ctx, int first, int count, double* out);
int dqmc_series_stats_host(dqmc_ctx* ctx, double* mean, double* err);
int dqmc_series_derived_host(dqmc_ctx* ctx, double* value, double* err);
int dqmc_series_phi_derived_host(dqmc_ctx* ctx, double* value, double* err);
int dqmc_series_band_derived_host(dqmc_ctx* ctx, double* value, double* err);
int dqmc_series_custom_derived_host(dqmc_ctx* ctx, int qx, int qy, double* value, double* err);
int dqmc_series_custom_pair_derived_host(dqmc_ctx* ctx, int qx, int qy, double* value, double* err);
size_t dqmc_series_pair_vertex_size(dqmc_ctx* ctx);
int dqmc_series_pair_vertex_host(dqmc_ctx* ctx, int qx, int qy, double* value, double* err);
size_t dqmc_series_ph_vertex_size(dqmc_ctx* ctx);
int dqmc_series_ph_vertex_host(dqmc_ctx* ctx, int qx, int qy, double* value, double* err);
int dqmc_series_end(dqmc_ctx* ctx);
/* ---- the series over a long run: re-binning, binning analysis with tau_int, export / import ------------
 * All of it is new surface: with none of these calls used, every call above keeps its bits, its error codes and its launches.
 * dqmc_series_configure: the options of the open series, allowed only while it is empty (no accumulate since dqmc_series_begin).
 *   DQMC_SERIES_AUTO_REBIN needs max_bins even and >= 4.  DQMC_EINVAL with nothing changed otherwise, and for unknown bits.  The options
 *   are no bits of `parts`: dqmc_series_begin refuses parts = 32.
 * dqmc_series_rebin: merges neighbouring closed bins in place, all slots: closed[k] = (closed[2k] + closed[2k+1]) * 0.5 for k < B/2 (two
 *   IEEE operations); bins_closed halves, bin_size doubles, rebins increments.  The open bin and sweeps_in_open_bin stay: the open bin
 *   now closes after the new bin_size samples.  DQMC_EINVAL with nothing changed: an odd number of closed bins; a bin_size that would
 *   rise above 2^30.  Zero closed bins: only bin_size doubles.
 * AUTO_REBIN: the dqmc_series_accumulate / dqmc_series_add_sweep whose close makes bins_closed == max_bins re-bins before it returns, so
 *   the series is never observed full (dqmc_series_form_sample is unchanged).  If bin_size cannot double, the series becomes full.
 * TRACK_VARIANCE: two more buffers [nb][S] per slot, a running mean w and m2, routed like the open bin.  Every accumulate raises
 *   `samples` to n and does d = x - w; w += d / n; m2 += d (x - w) (Welford) in a kernel of its own.  `samples` counts without the flag too.
 * dqmc_series_binning_host (all chains; err and tau [levels][nb][S]; tau may be NULL): levels in 1 .. 12.  Level l has B_l = bins_closed >> l
 *   merged bins y^l_k, y^0_k = closed bin k, y^l_k = (y^(l-1)_2k + y^(l-1)_(2k+1)) * 0.5 -- what l calls of dqmc_series_rebin would leave;
 *   closed bins beyond 2^l B_l are not used.  err_l = the err of dqmc_series_stats_host over y^l_0 .. y^l_(B_l - 1) in index order;
 *   tau_l = 1/2 err_l^2 (B_l 2^l bin_size) / sigma^2, sigma^2 = m2 / (samples - 1) over all samples of the slot, in sweeps; NaN where
 *   sigma^2 is not > 0.  DQMC_EINVAL: levels out of range, B_(levels-1) < 2, tau without TRACK_VARIANCE or with samples < 2.  The bins are
 *   only read (twice, whatever `levels` is); one writer per element, index order, no atomics: two calls give identical bits, and a
 *   chain's results do not depend on how chains are batched.
 * dqmc_series_export_host / _import_host: the closed bins [bins_closed][nb][S], the open bin [nb][S], then w and m2 [nb][S] each if the
 *   variance is tracked; len must be exactly that many doubles.  Import goes into an open series (dqmc_series_begin): nb, sample_len,
 *   parts and nfreq of the struct must match it, bins_closed < its max_bins, 0 <= sweeps_in_open_bin < bin_size, the flags valid for its
 *   max_bins (max_bins of the struct is not read).  It sets bin_size, flags, the counters, samples and rebins from the struct and clears
 *   the formed mark.  Every DQMC_EINVAL leaves the series as it was.  With dqmc_series_begin this is the restore path of a checkpoint. */
#define DQMC_SERIES_AUTO_REBIN     1
#define DQMC_SERIES_TRACK_VARIANCE 2
typedef struct { int bin_size, max_bins, nfreq, parts, flags, bins_closed, sweeps_in_open_bin, nb;
                 long long samples, rebins; size_t sample_len; } dqmc_series_state;
int dqmc_series_configure(dqmc_ctx* ctx, int flags);
int dqmc_series_get_state(dqmc_ctx* ctx, dqmc_series_state* state);
int dqmc_series_rebin(dqmc_ctx* ctx);
int dqmc_series_binning_host(dqmc_ctx* ctx, int levels, double* err, double* tau);
int dqmc_series_export_host(dqmc_ctx* ctx, double* out, size_t len);
int dqmc_series_import_host(dqmc_ctx* ctx, const dqmc_series_state* state, const double* in, size_t len);
/* for tests: the last propagated triple G(tau_k,0), G(0,tau_k), G(tau_k) of the selected chain and its slice k (after
 * dqmc_measure_timedisplaced_ends: the triple of row m) */
int dqmc_get_green_td_fine_host(dqmc_ctx* ctx, dqmc_cplx* g_t0, dqmc_cplx* g_0t, dqmc_cplx* g_tt, int* slice);

/* set_exchange_parameter_value (detsdwopdim.cpp:5195-5197): r only enters the bosonic action */
int dqmc_set_exchange_parameter(dqmc_ctx* ctx, double r);

/* ---- measurement helpers for bench.py -------------------------------------------------------- */
/* Device time per kernel family, measured with HIP events on the context's own stream while profiling is
 * switched on, plus launch counts and decomposition statistics. */
enum { DQMC_FAM_BMULT = 0, DQMC_FAM_GEMM = 1, DQMC_FAM_DECOMP = 2, DQMC_FAM_DECIDE = 3, DQMC_FAM_OTHER = 4,
       DQMC_FAM_GATHER = 5, DQMC_FAM_FLUSH = 6, DQMC_FAM_COUNT = 8 };
typedef struct dqmc_profile {
    double ms[8];              /* per family: bmult, gemm (fixed-size products), decomp (Jacobi rounds or QR),
                                  decide, other, gather, flush (G += X Gr), unused */
    uint64_t launches[8];
    uint64_t svd_calls, svd_sweeps_total, svd_sweeps_max, qr_calls;
    double gemm_flops;         /* 8 M N K summed over the launches of family gemm (4 M N K for the triangular chaining product) */
    double decomp_round_ms;    /* SVD mode: time inside batches of back-to-back Jacobi rounds only */
    uint64_t decomp_rounds;
    uint64_t blocks_nonempty;   /* delayed-update blocks that really flushed, summed over all chains, since dqmc_profile_enable */
    uint64_t chains;            /* chains every launch of this context carries */
    uint64_t updates_accepted;  /* accepted local updates, summed over all chains, since dqmc_profile_enable (flush flops = 8 n_g^2 MSF each) */
    uint64_t lu_calls;          /* QR mode: Green's functions whose inner inverse came from the LU factorisation (n_g <= 512); qr_calls then
                                   counts the chain factorisations (UDT) only */
    /* GPU-filling launches INSIDE the decomposition family, timed on their own (their time is also part of ms[DQMC_FAM_DECOMP]):
       [0] trailing updates of the LU factorisation (K = 32, on the flush kernel), [1] products inside factorisations and triangular
       solves (k_zgemm: the levels of the recursive solves, the block Gram-Schmidt QR); flops counted as 8 M N K, bytes as the
       operands read once and the result written (read-modify-written) once */
    double sub_ms[4];
    uint64_t sub_launches[4];
    double sub_flops[4];
    double sub_bytes[4];
} dqmc_profile;
int dqmc_profile_enable(dqmc_ctx* ctx, int on);
int dqmc_profile_read(dqmc_ctx* ctx, dqmc_profile* out);

#ifdef __cplusplus
}
#endif
#endif /* DQMC_HIP_H_ */
