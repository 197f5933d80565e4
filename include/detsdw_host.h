/*
 * detsdw_host.h -- C API of the C++ host layer that sits ABOVE the kernel ABI (dqmc_hip.h).
 *
 * The host layer (detqmc_amd/csrc/host/detsdw.{h,cpp}) is the build's DetSDW / DetModelGC
 * equivalent: it owns the RNG stream, the parameter checks and the control flow of
 * sweep_skeleton / sweepUp / sweepDown / globalMove (reference src/detmodel.h:1266-1478,
 * src/detsdwopdim.cpp:3461-3644, 4423-4502) and calls ONLY the C ABI of dqmc_hip.h.  This header
 * exposes that C++ class with the reference's method names so that harnesses written in C, or
 * Python through ctypes, can drive it; it mirrors the operator surface DetQMC<Model> /
 * DetQMCPT<Model> require of a replica (src/detqmc.h:58-156, src/detmodel.h:138-156,
 * src/detsdwopdim.h:116-153).
 */
#ifndef DETSDW_HOST_H_
#define DETSDW_HOST_H_

#include <stddef.h>
#include <stdint.h>
#include "dqmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct detsdw_replica detsdw_replica;

/* ModelParamsDetSDW (src/detsdwparams.h:24-120) + rngSeed/simindex of DetQMCParams
 * (src/detqmcparams.h) as far as the sweep path uses them.  Unsupported reference options
 * (turnoffFermions, overRelaxation, phiFixed) are rejected by detsdw_create with DQMC_EINVAL and a
 * message naming the option. */
typedef struct detsdw_params {
    int32_t opdim;
    int32_t L;
    int32_t m;                   /* give m > 0 OR beta > 0, not both (detmodelparams.h:97-110) */
    int32_t s;
    int32_t delaySteps;
    int32_t globalShift;
    int32_t globalUpdateInterval;
    int32_t weakZflux;
    int32_t phi2bosons;
    int32_t device;
    int32_t simindex;
    uint32_t rngSeed;
    int32_t has_mux_muy;         /* if 0: mux = muy = mu (detsdwopdim.cpp:75-79) */
    int32_t updateMethod;        /* 0 iterative, 1 woodbury, 2 delayed (all give the same chain; 0/1 run with D = 1) */
    char bc[16];                 /* "pbc", "apbc-x", "apbc-y", "apbc-xy" */
    double beta, dtau;
    double r, c, u, lambda;
    double txhor, txver, tyhor, tyver;
    double mu, mux, muy;
    double accRatio;
    double cdwU;                 /* != 0: discrete field l_i(tau) next to phi, updated in a second pass over each slice (detsdwopdim.cpp:2474-2485) */
    int32_t stabilisation;       /* 0 = SVD (as the reference), 1 = QR/UDT (same G to rounding, much faster) */
    int32_t cb_none;             /* 0 = checkerboard (default), 1 = checkerboard=false: dense B matrices (CB_NONE) */
    int32_t wolffClusterUpdate;       /* attemptWolffClusterUpdate every globalUpdateInterval sweeps (detsdwopdim.cpp:3488-3562) */
    int32_t wolffClusterShiftUpdate;  /* combined cluster + global shift (:3647-3751); excludes the two individual moves */
    int32_t repeatWolffPerSweep;      /* cluster flips per attempt, 0 is read as 1 */
    int32_t fermionMeasurements;      /* 1: sweep(takeMeasurements) also takes the G-dependent observables (the reference's
                                         default, i.e. turnoffFermionMeasurements = false); 0: bosonic observables only.
                                         | DETSDW_FM_EQ_CORRELATORS (equalTimeCorrelators; needs bit 0, ParameterWrong otherwise): a
                                         measurement sweep also bins the equal-time charge, spin-z, SDW and pairing correlators on
                                         every one of its m slices (DETSDW_OBS_CHARGECORR .. _PAIRMINUSSQ).  The struct has no free
                                         slot, so the option travels as a flag bit.
                                         | DETSDW_FM_EQ_BAND (bandCorrelators; needs DETSDW_FM_EQ_CORRELATORS, ParameterWrong otherwise):
                                         and the equal-time bandDiff / bandMix correlators (DETSDW_OBS_BANDDIFFCORR .. _BANDMIXSQ).
                                         Any other bit: ParameterWrong */
    int32_t spinProposalMethod;       /* 0 box (default), 1 rotate_then_scale, 2 rotate_and_scale -- the latter two for opdim == 3 only
                                         (src/detsdwparams.h:40-42, src/detsdwopdim.cpp:2447-2470) */
    int32_t adaptScaleVariance;       /* adapt scaleDelta during thermalization (src/detsdwparams.h:43) */
    int32_t repeatUpdateInSlice;      /* passes of local updates per time slice and sweep, 0 is read as 1 (src/detsdwparams.h:90) */
    int32_t timeDisplacedMeasurements; /* 1 (needs fermionMeasurements): a measurement sweep also takes G(k, tau_j) at the interior
                                         stabilisation boundaries tau_j = j s dtau, j = 1 .. n-1 (DETSDW_OBS_GREENKTAU_X / _Y); 2: and the
                                         time-displaced pairing correlators (DETSDW_OBS_PAIRPLUSTAU .. _PAIRMINUSTAU_Q0).
                                         | DETSDW_TD_EVERY_SLICE (timeDisplacedEverySlice; needs a level >= 1, ParameterWrong otherwise):
                                         every enabled time-displaced channel is also measured on every time slice tau_k = k dtau,
                                         k = 0 .. m (DETSDW_OBS_FINE).  The struct has no free slot and its bytes stay where they are,
                                         so the option travels as a flag bit, as in dqmc_params::timedisplaced.
                                         | DETSDW_TD_FINE_ON_DEVICE (timeDisplacedFineOnDevice; needs DETSDW_TD_EVERY_SLICE, ParameterWrong
                                         otherwise): the every-slice blocks are not copied to the host after a measurement sweep; the
                                         ...Fine observables raise ParameterWrong and detsdw_get_matsubara* are their readers */
    dqmc_tuning tuning;               /* result-neutral execution choices handed to every kernel context (dqmc_hip.h); all zero =
                                         automatic.  With pipeline = 0 the host layer switches the pipelined update on only for
                                         handles of at most two kernel contexts (more contexts overlap each other instead).
                                         bmult_path | DQMC_TUNING_NO_RNG_LOOKAHEAD (rngLookahead = -1): every sweep pushes its whole
                                         window of uniforms before it starts; otherwise the next window's draws are generated and
                                         uploaded while the device sweeps and the window is spliced on the device (same chain) */
    int32_t timeDisplacedParticleHole; /* 1 (needs timeDisplacedMeasurements >= 1): a measurement sweep also takes the time-displaced
                                         charge, spin-z and SDW order-parameter correlators (DETSDW_OBS_CHARGETAU .. _SDWTAU_Q0).  The
                                         field took the second reserved slot of dqmc_tuning: the bytes of the struct are where they were.
                                         2: also the current-current correlators and the bond kinetic energy (DETSDW_OBS_CURRENTXTAU ..
                                         _BONDKINETICY).
                                         | DETSDW_TD_PH_BAND (bandCorrelators; needs a value >= 1, ParameterWrong otherwise): and the
                                         band-resolved charge correlators bandDiff (n_x - n_y: nematic at q = 0, d-wave CDW at (pi, pi))
                                         and bandMix (dqmc_measure_timedisplaced_band; DETSDW_OBS_BANDDIFFTAU .. _BANDMIXTAU_Q0).
                                         Any other value, any other bit: ParameterWrong */
} detsdw_params;

typedef struct detsdw_info {
    int32_t opdim, L, N, MSF, n_g, m, s, n;
    int32_t performedSweeps;
    int32_t lastSweepDir;        /* +1 up, -1 down */
    int32_t acceptedGlobalShifts, attemptedGlobalShifts;
    int32_t currentTimeslice;
    int32_t reserved;
    int32_t acceptedWolffClusterUpdates, attemptedWolffClusterUpdates;
    int32_t acceptedWolffClusterShiftUpdates, attemptedWolffClusterShiftUpdates;
    double addedWolffClusterSize;
    double beta, dtau;
    double phiDelta, lastAccRatioLocal_phi;
    double r;                    /* exchange parameter */
    double angleDelta, scaleDelta;   /* rotate / scale proposals (AdjustmentData, src/detsdwopdim.h:510-512) */
    uint64_t rngDrawn;           /* uniforms consumed from the stream so far */
} detsdw_info;

/* control data swapped in replica exchange: UpdateStatistics + AdjustmentData
 * (src/detsdwopdim.cpp:5219-5247), fixed-size POD instead of a boost archive */
typedef struct detsdw_control_data {
    int32_t acceptedGlobalShifts, attemptedGlobalShifts;
    int32_t acceptedWolffClusterUpdates, attemptedWolffClusterUpdates;
    int32_t acceptedWolffClusterShiftUpdates, attemptedWolffClusterShiftUpdates;
    double addedWolffClusterSize;
    dqmc_update_state adjust;
} detsdw_control_data;

/* bosonic observables of a measurement sweep: initMeasurements / measure / finishMeasurements with
 * turnoffFermionMeasurements (src/detsdwopdim.cpp:441-456, :509-545, :903-921); valid after detsdw_sweep(r, 1).
 * With fermionMeasurements the G-dependent observables follow (:545-899): the scalars below fermionic_valid and the vectors of
 * detsdw_get_observable_vector. */
typedef struct detsdw_observables {
    double meanPhi[3];
    double normMeanPhi;
    double associatedEnergy;
    double phiRhoS_Gc, phiRhoS_Gs;      /* opdim == 2 only */
    int32_t valid;                      /* 1 after a sweep with takeMeasurements */
    int32_t fermionic_valid;            /* 1 if the fields below and the vectors of detsdw_get_observable_vector were taken */
    double greenK0, greenLocal;         /* src/detsdwopdim.cpp:565-588, :926-927 */
    double pairPlusMax, pairMinusMax;   /* :986-1002 */
    double occDiffSq;                   /* :866-897, :1013 */
} detsdw_observables;
enum { DETSDW_OBS_KOCCX = 0, DETSDW_OBS_KOCCY = 1, DETSDW_OBS_PAIRPLUS = 2, DETSDW_OBS_PAIRMINUS = 3,
       DETSDW_OBS_GREENKTAU_X = 4, DETSDW_OBS_GREENKTAU_Y = 5,
       DETSDW_OBS_PAIRPLUSTAU = 6, DETSDW_OBS_PAIRMINUSTAU = 7, DETSDW_OBS_PAIRPLUSTAU_Q0 = 8, DETSDW_OBS_PAIRMINUSTAU_Q0 = 9,
       DETSDW_OBS_CHARGETAU = 10, DETSDW_OBS_SPINZTAU = 11, DETSDW_OBS_SDWTAU = 12,
       DETSDW_OBS_CHARGETAU_Q0 = 13, DETSDW_OBS_SPINZTAU_Q0 = 14, DETSDW_OBS_SDWTAU_Q0 = 15,
       DETSDW_OBS_CURRENTXTAU = 16, DETSDW_OBS_CURRENTYTAU = 17, DETSDW_OBS_CURRENTXTAU_Q0 = 18, DETSDW_OBS_CURRENTYTAU_Q0 = 19,
       DETSDW_OBS_BONDKINETICX = 20, DETSDW_OBS_BONDKINETICY = 21,
       DETSDW_OBS_CHARGECORR = 22, DETSDW_OBS_SPINZCORR = 23, DETSDW_OBS_SDWCORR = 24, DETSDW_OBS_PAIRPLUSCORR = 25, DETSDW_OBS_PAIRMINUSCORR = 26,
       DETSDW_OBS_CHARGESQ = 27, DETSDW_OBS_SPINZSQ = 28, DETSDW_OBS_SDWSQ = 29, DETSDW_OBS_PAIRPLUSSQ = 30, DETSDW_OBS_PAIRMINUSSQ = 31,
       /* the order-parameter part of a measurement series only (detsdw_series_* below; detsdw_get_observable_vector refuses them) */
       DETSDW_OBS_PHICHI = 32, DETSDW_OBS_PHISCALARS = 33,
       /* bandCorrelators: the time-displaced ones have DETSDW_OBS_FINE twins and Matsubara transforms like chargeTau, the equal-time
          ones are read and enter a series like chargeCorr / chargeSq */
       DETSDW_OBS_BANDDIFFTAU = 34, DETSDW_OBS_BANDMIXTAU = 35, DETSDW_OBS_BANDDIFFTAU_Q0 = 36, DETSDW_OBS_BANDMIXTAU_Q0 = 37,
       DETSDW_OBS_BANDDIFFCORR = 38, DETSDW_OBS_BANDMIXCORR = 39, DETSDW_OBS_BANDDIFFSQ = 40, DETSDW_OBS_BANDMIXSQ = 41,
       /* user-defined bilinears (detsdw_set_custom_bilinears), matrix c = 0 .. 3 at BASE + c: custom{c}Tau and custom{c}TauQ0 with the rows,
          normalisation, DETSDW_OBS_FINE twins and Matsubara transforms of bandDiffTau; custom{c}Corr and custom{c}Sq with those of
          bandDiffCorr / bandDiffSq.  ParameterWrong for a c that is not set, or without the family the observable rides on */
       DETSDW_OBS_CUSTOMTAU = 42, DETSDW_OBS_CUSTOMTAU_Q0 = 46, DETSDW_OBS_CUSTOMCORR = 50, DETSDW_OBS_CUSTOMSQ = 54,
       /* user-defined pair operators (detsdw_set_custom_pair_operators), operator c = 0 .. 3 at BASE + c: customPair{c}Tau,
          customPair{c}TauQ0 (DETSDW_OBS_FINE twins, Matsubara transforms), customPair{c}Corr, customPair{c}Sq, like the custom{c} ones */
       DETSDW_OBS_CUSTOMPAIRTAU = 58, DETSDW_OBS_CUSTOMPAIRTAU_Q0 = 62, DETSDW_OBS_CUSTOMPAIRCORR = 66, DETSDW_OBS_CUSTOMPAIRSQ = 70,
       /* the averaged Green's function (detsdw_set_green_matrix): greenMatrixTau, rows x N x 4 x 4 complex as (re, im) -- per row and
          periodic site difference d the full 4 x 4 block Gbar_ab(d) / (N count), expanded from the stored sector for OPDIM < 3; rows
          j = 1 .. n-1, with DETSDW_OBS_FINE (greenMatrixTauFine) k = 0 .. m.  As a series observable: the stored block, [m+1][N][R][R] complex */
       DETSDW_OBS_GREENMATRIXTAU = 74 };
/* equalTimeCorrelators: flag bit of detsdw_params::fermionMeasurements */
enum { DETSDW_FM_EQ_CORRELATORS = 0x100 };
/* bandCorrelators: DETSDW_FM_EQ_BAND is a flag bit of detsdw_params::fermionMeasurements, DETSDW_TD_PH_BAND one of ::timeDisplacedParticleHole */
enum { DETSDW_FM_EQ_BAND = 0x200, DETSDW_TD_PH_BAND = 0x100 };
/* timeDisplacedEverySlice: flag bit of detsdw_params::timeDisplacedMeasurements */
enum { DETSDW_TD_EVERY_SLICE = 0x100 };
/* timeDisplacedFineOnDevice: flag bit of detsdw_params::timeDisplacedMeasurements; never reaches dqmc_params::timedisplaced */
enum { DETSDW_TD_FINE_ON_DEVICE = 0x200 };
/* which | DETSDW_OBS_FINE for which = DETSDW_OBS_GREENKTAU_X .. _BONDKINETICY and DETSDW_OBS_BANDDIFFTAU .. _BANDMIXTAU_Q0: the every-slice twin ("...Fine") of the observable, rows
 * k = 0 .. m instead of j = 1 .. n-1, columns unchanged; needs timeDisplacedEverySlice next to the option its coarse twin needs */
enum { DETSDW_OBS_FINE = 0x100 };    /* a bit of the observable index: unrelated to DETSDW_TD_EVERY_SLICE, a bit of a parameter */
/* What an observable index is, from the host layer's catalogue (detqmc_amd/csrc/host/obs_catalogue.h); needs no handle and no GPU.
 * family: where the values come from -- the per-slice accumulators (kOccX .. pairMinus), an equal-time block, a time-displaced block, or
 *   the order-parameter part of a series.  block: the channel 0 .. 7 of dqmc_measure_td_fine_read_host (time-displaced) or the equal-time
 *   block 0 .. 3 (fixed channels, band, custom bilinears, custom pair operators); component: the index inside the block.
 * kind: the shape -- SITE [N]; TAU [rows][N]; TAU_Q0 and ROW_SCALAR [rows]; CORR and SQ [N]; GREEN_MATRIX [rows][N][4][4] complex (as a
 *   series observable the stored [m+1][N][R][R] complex); PHI_CHI [nfreq][N]; PHI_SCALARS [5].  rows = n-1, or m+1 with DETSDW_OBS_FINE.
 * fine: `which` carried DETSDW_OBS_FINE.  has_fine_twin, has_matsubara (detsdw_get_matsubara takes the index); series_part, series_bit:
 *   the part index of dqmc_series_layout and the DQMC_SERIES_* bit of the part that holds it, both -1 where the series readers refuse
 *   the index.  An index with DETSDW_OBS_FINE has no Matsubara transform and no series part of its own.
 * DQMC_EINVAL: an unknown index, or DETSDW_OBS_FINE on an index without a twin. */
enum { DETSDW_OBS_FAMILY_SLICE = 0, DETSDW_OBS_FAMILY_EQ = 1, DETSDW_OBS_FAMILY_TD = 2, DETSDW_OBS_FAMILY_PHI = 3 };
enum { DETSDW_OBS_KIND_SITE = 0, DETSDW_OBS_KIND_TAU = 1, DETSDW_OBS_KIND_TAU_Q0 = 2, DETSDW_OBS_KIND_ROW_SCALAR = 3, DETSDW_OBS_KIND_CORR = 4,
       DETSDW_OBS_KIND_SQ = 5, DETSDW_OBS_KIND_GREEN_MATRIX = 6, DETSDW_OBS_KIND_PHI_CHI = 7, DETSDW_OBS_KIND_PHI_SCALARS = 8 };
typedef struct detsdw_observable_desc {
    int32_t family, block, component, kind;
    int32_t fine, has_fine_twin, has_matsubara;
    int32_t series_part, series_bit;
} detsdw_observable_desc;
int detsdw_describe_observable(int which, detsdw_observable_desc* out);

/* createReplica (src/detsdwopdim.cpp:49-84) + DetSDW ctor (:158-361): checks parameters, seeds the
 * RNG with (rngSeed, simindex + 1) (src/detqmc.h:181), draws the random field, builds UdV storage and
 * G(beta) */
int detsdw_create(const detsdw_params* p, detsdw_replica** out);
/* The replicas of one parallel-tempering ensemble held by ONE process / GPU (the reference holds one replica per
 * MPI rank, src/detqmcpt.h:300-420): p[0..nchains) may differ only in r, rngSeed and simindex.  All chains
 * sweep in lockstep (every kernel launch carries all of them); each follows exactly the Markov chain a
 * single replica created from p[b] would.  detsdw_sweep* act on all chains, every other call below on the
 * chain chosen with detsdw_select_chain (default 0). */
int detsdw_create_batch(const detsdw_params* p, int nchains, detsdw_replica** out);
/* The chains of a batch live in `sub_batches` kernel contexts (own HIP stream each) that a sweep drives concurrently, one
 * host thread per context: the contexts drift out of phase, so the latency-bound kernels of one overlap the streaming /
 * MFMA kernels of the others inside ONE process.  Results do not depend on the grouping (independent Markov chains).
 * sub_batches = 0 (what detsdw_create_batch passes): automatic, up to 4 contexts of at least 32 chains each; otherwise a
 * divisor of nchains. */
int detsdw_create_batch_ex(const detsdw_params* p, int nchains, int sub_batches, detsdw_replica** out);
int detsdw_num_sub_batches(detsdw_replica* r);
int detsdw_select_chain(detsdw_replica* r, int chain);
int detsdw_num_chains(detsdw_replica* r);
void detsdw_destroy(detsdw_replica* r);
const char* detsdw_last_error(void);

/* DetModel::sweep / sweepThermalization (src/detmodel.h:138-147, src/detsdwopdim.cpp:4423-4502) */
int detsdw_sweep(detsdw_replica* r, int takeMeasurements);
int detsdw_sweep_thermalization(detsdw_replica* r);

int detsdw_get_info(detsdw_replica* r, detsdw_info* out);
int detsdw_get_observables(detsdw_replica* r, detsdw_observables* out);
/* N-vectors of the last measurement sweep: kOccX, kOccY (site index = k-vector, :616-659, :937-941), pairPlus, pairMinus.
 * With timeDisplacedMeasurements: greenKTauX / greenKTauY, (n-1) x N (row j-1 = tau_j, column = k-vector as for kOcc):
 *   G_band(k, tau_j) = Re (1/2N) sum_spin sum_{a,b} e^{i k (r_a - r_b)} [e^{-dtau K/2} G(tau_j, 0) e^{+dtau K/2}]_{(a,band,spin),(b,band,spin)}
 * With timeDisplacedMeasurements == 2: pairPlusTau / pairMinusTau, (n-1) x N (row j-1 = tau_j, column = periodic site difference
 * d = (dx, dy), index dy L + dx):  C+-(d, tau_j) = (1/N) sum_B Re T+-(B (+) d, B), T+- the pairPlus / pairMinus expressions (:695-715)
 * on the same shifted G(tau_j, 0) (dqmc_measure_timedisplaced_pair); pairPlusTauQ0 / pairMinusTauQ0, n-1: their sums over d
 * With timeDisplacedParticleHole: chargeTau / spinZTau / sdwTau, (n-1) x N, same rows and columns:
 *   C(d, tau_j) = (1/N) sum_B Re W(B (+) d, B),  W the Wick contraction of <O_A(tau_j) O_B(0)> for the site bilinears of
 * dqmc_measure_timedisplaced_ph (dqmc_hip.h); chargeTauQ0 / spinZTauQ0 / sdwTauQ0, n-1: their sums over d
 * With timeDisplacedParticleHole == 2: currentXTau / currentYTau, (n-1) x N, same rows and columns:
 *   Lambda_mumu(d, tau_j) = (1/N) sum_B Re W[j_mu(B (+) d), j_mu(B)],  j_mu the bond current of dqmc_measure_timedisplaced_current;
 * currentXTauQ0 / currentYTauQ0, n-1: their sums over d; bondKineticX / bondKineticY, n-1: (1/N) sum_A Re <k_mu(A)> at tau_j, the
 * diamagnetic term.  The tau quadrature and the Fourier sum over d of the every-slice twins: detsdw_get_matsubara below
 * With DETSDW_FM_EQ_CORRELATORS (ParameterWrong without it; no DETSDW_OBS_FINE twins): chargeCorr / spinZCorr / sdwCorr / pairPlusCorr /
 * pairMinusCorr, N, column = periodic site difference dy L + dx:
 *   C_X(d) = (1 / (m N)) sum_{slices k = 1 .. m} sum_B Re W_X(B (+) d, B)   on g~ = e^{-dtau K/2} G(tau_k) e^{+dtau K/2} after the updates
 * of slice k (dqmc_set_equal_time_correlators, dqmc_hip.h: the Wick forms of the time-displaced channels with G(tau,0) -> g~,
 * G(0,tau) -> g~ - 1, and T+- on g~); chargeSq / spinZSq / sdwSq / pairPlusSq / pairMinusSq, N, column qy L + qx, q = 2 pi (qx, qy) / L:
 *   S_X(q) = sum_d cos(q d) C_X(d).   Values of ONE sweep; averages and error bars over sweeps: the measurement series below
 * With DETSDW_TD_PH_BAND: bandDiffTau / bandMixTau, (n-1) x N, and bandDiffTauQ0 / bandMixTauQ0, n-1, rows, columns and normalisation of
 * chargeTau, for the bilinears M_BAND / M_MIX of dqmc_measure_timedisplaced_band.  With DETSDW_FM_EQ_BAND: bandDiffCorr / bandMixCorr and
 * bandDiffSq / bandMixSq, N, defined like chargeCorr / chargeSq (dqmc_set_equal_time_band) */
int detsdw_get_observable_vector(detsdw_replica* r, int which, double* out);
/* With timeDisplacedEverySlice: the Matsubara transforms of the every-slice observable `which`, formed on the device from the blocks
 * of the last measurement sweep (dqmc_measure_td_matsubara_host, dqmc_hip.h), n = 0 .. nfreq-1, 1 <= nfreq <= m, trapezoid weights
 * w_0 = w_m = 1/2 over tau_k = k dtau.  which = DETSDW_OBS_PAIRPLUSTAU, _PAIRMINUSTAU, _CHARGETAU, _SPINZTAU, _SDWTAU, _CURRENTXTAU,
 * _CURRENTYTAU (no DETSDW_OBS_FINE bit), omega_n = 2 pi n / beta:
 *   chi(q, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} sum_d e^{-i q d} C(d, tau_k),   q = (2 pi / L)(qx, qy), column qy L + qx;
 * which = DETSDW_OBS_GREENKTAU_X / _Y, omega_n = (2n+1) pi / beta:
 *   G_band(k, i omega_n) = dtau sum_k w_k e^{i omega_n tau_k} G_band(k, tau_k),   column = k-vector as for kOcc.
 * detsdw_get_matsubara: the selected chain, out[nfreq][N] complex as (re, im); detsdw_get_matsubara_all: every chain in handle order,
 * out[nchains][nfreq][N], ONE device call per kernel context.  Valid after detsdw_sweep(r, 1) and until the next sweep of either
 * kind (DQMC_EINVAL otherwise); ParameterWrong if the option `which` needs, or timeDisplacedEverySlice, is off.  The superfluid density
 * follows from Lambda_xx, Lambda_yy at i omega = 0 and the smallest non-zero q:
 *   rho_s = 1/8 Re [ Lxx(qx=1, qy=0) - Lxx(qx=0, qy=1) + Lyy(qx=0, qy=1) - Lyy(qx=1, qy=0) ] */
int detsdw_get_matsubara(detsdw_replica* r, int which, int nfreq, double* out);
int detsdw_get_matsubara_all(detsdw_replica* r, int which, int nfreq, double* out);
/* Measurement series: bins over measurement sweeps and jackknife errors, kept on the device (dqmc_series_*, dqmc_hip.h).
 * detsdw_series_begin opens one series per kernel context.  Its parts follow from the handle's options: the equal-time part with
 * equalTimeCorrelators (and the equal-time band part with DETSDW_FM_EQ_BAND), one Matsubara part (nfreq frequencies, 1 <= nfreq <= m) per
 * enabled every-slice channel (bandDiffTau / bandMixTau with DETSDW_TD_PH_BAND included); nfreq is ignored
 * without timeDisplacedEverySlice; ParameterWrong if neither option is on -- unless flags holds DETSDW_SERIES_PHI, the third way to
 * open a series (the order-parameter part below, which needs no option).  While the series is open every detsdw_sweep(r, 1) ends
 * with one sample of every chain added to the series (after binSize of them a bin closes); thermalisation sweeps and detsdw_sweep(r, 0) add
 * nothing.  A measurement sweep on a full series (maxBins bins closed) fails with DQMC_EINVAL before it changes anything: read the
 * series out and end it, or let it re-bin itself (detsdw_series_configure below).
 * flags: DETSDW_SERIES_NO_HOST_COPY -- while the series is open a measurement sweep does not copy the equal-time block to the host
 * and forms no cosine sums there; DETSDW_OBS_CHARGECORR .. _PAIRMINUSSQ of detsdw_get_observable_vector then raise ParameterWrong
 * (as the ...Fine observables do with timeDisplacedFineOnDevice).
 * Readers (DQMC_EINVAL with fewer than two closed bins; definitions of mean, err and the derived quantities in dqmc_hip.h):
 *   detsdw_series_stats: the selected chain; which = DETSDW_OBS_CHARGECORR .. _PAIRMINUSSQ: mean[N], err[N]; which = one of the
 *     observables of detsdw_get_matsubara: mean[nfreq][N] complex as (re, im), err likewise with the errors of the real and the
 *     imaginary part separately.  detsdw_series_stats_all: every chain in handle order, [nchains] x the same; one device call per
 *     kernel context serves every `which` until the next bin closes.
 *   detsdw_series_derived_all: what = DETSDW_SERIES_R_CHARGE .. _R_PAIRMINUS (correlation ratios) or DETSDW_SERIES_RHO_S, value[nchains]
 *     and err[nchains]; ParameterWrong if the option the quantity needs is off.
 *   detsdw_series_read_bins: closed bins first .. first + count - 1 of `which`, selected chain: out[count] x (N, or [nfreq][N] complex).
 * The order-parameter part, flags & DETSDW_SERIES_PHI (the part DQMC_SERIES_PHI of dqmc_hip.h, formed on the device from the field
 * itself): chi_phi(q, i omega_n), n = 0 .. nfreq-1 (1 <= nfreq <= m), and the scalars |phibar|, |phibar|^2, |phibar|^4, the equal-time
 * susceptibility and associatedEnergy -- what the reference gets offline from its configuration stream.  It is added to whatever parts
 * the options provide, and a handle with no other part may open a series with it, also one with fermionMeasurements = 0 (then every
 * detsdw_sweep(r, 1) feeds the series, and no Green's function measurement is needed).  Without the flag nothing changes.
 *   which = DETSDW_OBS_PHICHI: [nfreq][N] real, column qy L + qx; DETSDW_OBS_PHISCALARS: [5], for detsdw_series_stats, _stats_all,
 *     _read_bins, _binning, _binning_all (ParameterWrong without the part).  The physical susceptibility is beta N <chi>.
 *   what = DETSDW_SERIES_BINDER_PHI (1 - <|phibar|^4> / (3 <|phibar|^2>^2)), _BINDER_RATIO_PHI (<|phibar|^4> / <|phibar|^2>^2), _CHI_PHI
 *     (beta N <|phibar|^2>), _CHI_PHI_CONNECTED (beta N (<|phibar|^2> - <|phibar|>^2)), _R_PHI (1 - (chi(0; 1,0) + chi(0; 0,1)) / (2 chi(0; 0,0)))
 *     and _XI_PHI (the second-moment correlation length, NaN where undefined) for detsdw_series_derived_all: dqmc_series_phi_derived_host;
 *     ParameterWrong without the part.  A series file with the part loads only into a series opened with the flag.
 * detsdw_save_state does not store the series, and detsdw_load_state leaves an open series alone (bins closed before the load stay,
 * the open bin keeps what it holds; neither stores the route): the series has a file of its own, detsdw_series_save / _load below.
 * Slots and the route: a SLOT is a row of the series buffers (open bin, closed bins, statistics), indexed like a chain; the index of
 * every reader above -- the selected chain, or the position in an ..._all result -- means the slot.  A measurement sweep adds the sample
 * of chain c to slot slotOfChain[c]; the route is the identity after detsdw_series_begin, which is a series per chain.  Under replica
 * exchange within the handle a chain's control parameter changes: keep the route equal to the chains' parameter indices
 * (detsdw_series_route after every exchange step) and row s is control parameter s, whichever chain measured it.
 *   detsdw_series_route: slotOfChain[nchains] over ALL chains of the handle, whatever chain is selected; ParameterWrong unless it is a
 *     permutation of 0 .. nchains-1, DQMC_EINVAL when no series is open.  It may be called between any two sweeps, in mid-bin too: the
 *     open bin of a slot then goes on with the samples of another chain.  detsdw_series_end resets it to the identity.
 *   detsdw_series_get_route: the stored route, out[nchains].
 * A measurement sweep runs in two phases: every kernel context sweeps and forms its sample (dqmc_series_form_sample); when all have
 * finished, every context accumulates its slots from the rows of whichever contexts hold the routed chains (dqmc_series_accumulate;
 * this is how the ordering rule of dqmc_hip.h is kept).  If a context fails in the first phase no context accumulates and every series
 * is as it was; the sweep itself has happened.  With the identity the bins are bit for bit those of a series without a route, for any
 * number of sub-batches.  The route changes no trajectory and no observable of a sweep.  Routing across handles (GPUs) is not provided. */
enum { DETSDW_SERIES_NO_HOST_COPY = 1, DETSDW_SERIES_PHI = 2 };
enum { DETSDW_SERIES_R_CHARGE = 0, DETSDW_SERIES_R_SPINZ = 1, DETSDW_SERIES_R_SDW = 2, DETSDW_SERIES_R_PAIRPLUS = 3,
       DETSDW_SERIES_R_PAIRMINUS = 4, DETSDW_SERIES_RHO_S = 5,
       DETSDW_SERIES_BINDER_PHI = 6, DETSDW_SERIES_BINDER_RATIO_PHI = 7, DETSDW_SERIES_CHI_PHI = 8, DETSDW_SERIES_CHI_PHI_CONNECTED = 9,
       DETSDW_SERIES_R_PHI = 10, DETSDW_SERIES_XI_PHI = 11,
       /* correlation ratios of the equal-time band part (dqmc_series_band_derived_host): bandDiff at (pi, pi), bandDiff at 0, bandMix at (pi, pi) */
       DETSDW_SERIES_R_DCDW = 12, DETSDW_SERIES_R_NEMATIC = 13, DETSDW_SERIES_R_BANDMIX = 14 };
int detsdw_series_begin(detsdw_replica* r, int binSize, int maxBins, int nfreq, int flags);
int detsdw_series_route(detsdw_replica* r, const int* slotOfChain);
int detsdw_series_get_route(detsdw_replica* r, int* out);
int detsdw_series_info(detsdw_replica* r, int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen);
int detsdw_series_stats(detsdw_replica* r, int which, double* mean, double* err);
int detsdw_series_stats_all(detsdw_replica* r, int which, double* mean, double* err);
int detsdw_series_derived_all(detsdw_replica* r, int what, double* value, double* err);
/* what = 0 R_dCDW, 1 R_nematic, 2 R_bandMix (the same numbers as DETSDW_SERIES_R_DCDW .. _R_BANDMIX of detsdw_series_derived_all):
 * value[nchains], err[nchains]; ParameterWrong without DETSDW_FM_EQ_BAND */
int detsdw_series_band_derived(detsdw_replica* r, int what, double* value, double* err);
/* User-defined bilinears: count = 0 .. 4 Hermitian 4 x 4 matrices M[count][4][4] (row-major, band-spin order XUP, YDOWN, XDOWN, YUP) handed to
 * dqmc_set_custom_bilinears of every sub-batch context; may be called between sweeps, a second call replaces the first.  ParameterWrong
 * unless equalTimeCorrelators or timeDisplacedParticleHole >= 1 is on; the kernel level's refusals (a matrix that is not Hermitian, not
 * finite or all zero; a series with a custom part open) come back as its error, and ParameterWrong while a series with
 * DETSDW_SERIES_NO_HOST_COPY is open (it has no part for matrices set after it began, and nothing else would read their equal-time block).
 * The Matsubara transforms of the other channels stay valid across the call.  Measurement sweeps then measure the matrices wherever
 * they measure bandDiff / bandMix: at the coarse boundaries and on every slice (with timeDisplacedParticleHole) and at equal time (with
 * equalTimeCorrelators); the observables are DETSDW_OBS_CUSTOMTAU .. above.  A series begun while matrices are set carries
 * DQMC_SERIES_MATS_CUSTOM / DQMC_SERIES_EQ_CUSTOM, routed like every other part; detsdw_series_stats* / _read_bins / _binning* take
 * custom{c}Tau, custom{c}Corr and custom{c}Sq; detsdw_series_save writes the count and the matrices behind everything else (files of
 * series without a custom part keep their bytes) and detsdw_series_load raises ParameterWrong if they differ from the ones that are set.
 * detsdw_series_custom_derived: value[nchains], err[nchains] of R = 1 - 1/2 [S(Q + dx) + S(Q + dy)] / S(Q) for matrix c at Q = (qx, qy). */
int detsdw_set_custom_bilinears(detsdw_replica* r, int count, const dqmc_cplx* M);
int detsdw_series_custom_derived(detsdw_replica* r, int c, int qx, int qy, double* value, double* err);
/* The same with nearest-neighbour bond parts (dqmc_set_custom_bond_bilinears: M0 Hermitian, Mx / My arbitrary or NULL, [count][4][4] each):
 * the contract of detsdw_set_custom_bilinears, the kernel level's further refusals (all three parts of an operator zero, an off-diagonal
 * bond entry under weakZflux) included.  Every observable, Matsubara transform and series part above serves the operators unchanged.
 * detsdw_series_save writes, only while a bond part is non-zero, one more block behind the matrices (int32 1, Mx[count], My[count]);
 * detsdw_series_load raises ParameterWrong if the bond parts of the file and of the handle differ, a missing block on either side
 * included.  detsdw_set_custom_bilinears clears the bond parts.  The getter returns count and the three parts (each may be NULL). */
int detsdw_set_custom_bond_bilinears(detsdw_replica* r, int count, const dqmc_cplx* M0, const dqmc_cplx* Mx, const dqmc_cplx* My);
int detsdw_get_custom_bond_bilinears(detsdw_replica* r, int* count, dqmc_cplx* M0, dqmc_cplx* Mx, dqmc_cplx* My);
/* User-defined pair operators (dqmc_set_custom_pair_operators in dqmc_hip.h: the definition, the Wick form, the refusals): F0, Fx, Fy
 * [count][4][4] each, Fx / Fy may be NULL, count = 0 removes them; independent of the custom bilinears.  Forwarded to every sub-batch
 * context, between sweeps; if a later context fails the earlier ones get their old operators back.  ParameterWrong unless
 * equalTimeCorrelators or timeDisplacedMeasurements is set, and while a series with DETSDW_SERIES_NO_HOST_COPY is open; the kernel
 * level's refusals come back as its error.  Measurement sweeps then fill customPair{c}Tau / TauQ0 (timeDisplacedMeasurements >= 1; with
 * timeDisplacedEverySlice also the DETSDW_OBS_FINE twins and detsdw_get_matsubara[_all]) and customPair{c}Corr / Sq
 * (equalTimeCorrelators): C(d) = (1/N) sum_B Re <Delta_(B + d) Delta_B^+>, no factor 4 (pairPlusTau = 4 x the row of pair_operator 's').
 * A series begun while operators are set carries DQMC_SERIES_MATS_CUSTOM_PAIR / DQMC_SERIES_EQ_CUSTOM_PAIR, routed like every other
 * part; the series readers take customPair{c}Tau, Corr and Sq; detsdw_series_save appends one block (count, F0, Fx, Fy, zero padded to
 * DQMC_CUSTOM_MAX) behind everything else only while such a part is open, and detsdw_series_load raises ParameterWrong on a mismatch
 * before anything is imported.  detsdw_series_custom_pair_derived: value[nchains], err[nchains] of R at Q = (qx, qy) for operator c. */
int detsdw_set_custom_pair_operators(detsdw_replica* r, int count, const dqmc_cplx* F0, const dqmc_cplx* Fx, const dqmc_cplx* Fy);
int detsdw_get_custom_pair_operators(detsdw_replica* r, int* count, dqmc_cplx* F0, dqmc_cplx* Fx, dqmc_cplx* Fy);
int detsdw_series_custom_pair_derived(detsdw_replica* r, int c, int qx, int qy, double* value, double* err);
/* The averaged Green's function and the pair vertex (dqmc_set_green_matrix, dqmc_series_pair_vertex_host in dqmc_hip.h: definitions, sign
 * convention, refusals).  detsdw_set_green_matrix(on): forwarded to every sub-batch context, between sweeps; ParameterWrong without
 * timeDisplacedMeasurements, the kernel level's refusals (weakZflux, an open series that holds the part) come back as its error.  While
 * on, measurement sweeps fill greenMatrixTau (and, with timeDisplacedEverySlice, its DETSDW_OBS_FINE twin), and a series begun with
 * timeDisplacedEverySlice carries DQMC_SERIES_GREEN_MATRIX -- no new flag of detsdw_series_begin -- routed, re-binned and saved like every
 * other part: (m+1) 2 R^2 N doubles per chain and bin (0.8 MB at O(2), L = 16, m = 100), so maxBins is sized accordingly.  The series file
 * records the part in the `parts` word of its header; detsdw_series_load raises ParameterWrong on a mismatch before anything is imported,
 * and a series without the part writes the bytes it wrote before.  The series readers take DETSDW_OBS_GREENMATRIXTAU.
 * detsdw_series_pair_vertex: value[nchains][5 + m], err[nchains][5 + m] for pair operator c at Q = (qx, qy): P, Pbar, Gamma, Gamma Pbar,
 * then Pbar_c(Q, tau_k), k = 0 .. m; needs pair operators and the switch set before the series began. */
int detsdw_set_green_matrix(detsdw_replica* r, int on);
int detsdw_series_pair_vertex(detsdw_replica* r, int c, int qx, int qy, double* value, double* err);
/* The particle-hole counterpart (dqmc_series_ph_vertex_host in dqmc_hip.h): value[nchains][6 + m], err[nchains][6 + m] for user-defined
 * bilinear c (detsdw_set_custom_bilinears / detsdw_set_custom_bond_bilinears) at Q = (qx, qy): chi, chibar, Gamma, Gamma chibar, D, then
 * chibar_c(Q, tau_k), k = 0 .. m, over all sub-batch contexts in handle order.  Needs the matrices and detsdw_set_green_matrix set before
 * the series began, timeDisplacedParticleHole and timeDisplacedEverySlice; no new part and no new flag. */
int detsdw_series_ph_vertex(detsdw_replica* r, int c, int qx, int qy, double* value, double* err);
/* Wrap-error diagnostics (dqmc_set_green_check in dqmc_hip.h: definitions, table layout).  detsdw_set_green_check(on): forwarded to every
 * sub-batch context, between sweeps.  While on, sweepDown and sweepUp take the plain path at segment ends in every sweep, measuring or
 * not -- dqmc_update_slice_ex followed by dqmc_wrap, never dqmc_update_slice_final or dqmc_wrap_skip -- so that every one of the n
 * advances of a sweep finds a wrapped G and takes a sample.  The shortcuts only leave out work nobody reads: fields, Green's functions,
 * random streams and observables keep their bits whether the switch is on or off.  What it costs: n un-skipped wraps and flushes per
 * sweep, a copy of G and the compare.  detsdw_get_green_check: out[nchains][2][n+1][DQMC_GREEN_CHECK_FIELDS], chain-major
 * over all sub-batch contexts in handle order; it and detsdw_reset_green_check raise ParameterWrong while the switch is off.
 * Not included: the table is per chain (per slot of the handle) -- it is not routed by control parameter under replica exchange -- and
 * it is no part of detsdw_save_state or of the measurement series. */
int detsdw_set_green_check(detsdw_replica* r, int on);
int detsdw_get_green_check(detsdw_replica* r, double* out);
int detsdw_reset_green_check(detsdw_replica* r);
int detsdw_series_read_bins(detsdw_replica* r, int which, int first, int count, double* out);
int detsdw_series_end(detsdw_replica* r);
/* The series over a long run (kernel calls and formulas: dqmc_hip.h).  All of it is new surface: without these calls nothing changes.
 *   detsdw_series_configure: flags = DQMC_SERIES_AUTO_REBIN | DQMC_SERIES_TRACK_VARIANCE, applied to every kernel context, only while
 *     the series is empty.  With AUTO_REBIN (maxBins even and >= 4) the sweep that closes bin maxBins merges neighbouring bins before it
 *     returns -- half as many bins of twice the size -- so a measurement sweep is never refused for a full series.  All contexts
 *     accumulate in the same sweeps, so they re-bin in the same sweep.
 *   detsdw_series_rebin: the same merge on request (DQMC_EINVAL for an odd number of closed bins).
 *   detsdw_series_get_state: the state all contexts share; nb = the chains of the handle.
 *   detsdw_series_binning / _binning_all: the binning analysis of the selected slot, err[levels] x the slice of detsdw_series_stats and
 *     tau likewise (tau may be NULL; it needs TRACK_VARIANCE), or of every slot in handle order, [nchains][levels] x the slice.  One
 *     device call per kernel context serves every `which` until the next sample or re-bin.
 *   detsdw_series_save / _load: the series file -- magic "DQMCSER1", int32 version, dqmc_series_state (nb = all chains), the route
 *     int32[nchains], then per SLOT in handle order the closed bins [bins_closed][S], the open bin [S] and, with TRACK_VARIANCE, w [S] and
 *     m2 [S].  It does not depend on sub_batches.  detsdw_series_load needs a series already open (detsdw_series_begin with the options of
 *     the run: NO_HOST_COPY is taken from that call, bin size, options, counters, bins and the route from the file).  The whole file is
 *     checked against every kernel context before any context imports; a mismatch (chains, parts, nfreq, more bins than maxBins holds,
 *     options not valid for maxBins, a truncated file) is ParameterWrong or DQMC_EINVAL and leaves the series and the route as they were.
 *     detsdw_save_state / detsdw_load_state and their file do not change: a checkpoint of a run with a series is the two files. */
int detsdw_series_configure(detsdw_replica* r, int flags);
int detsdw_series_rebin(detsdw_replica* r);
int detsdw_series_get_state(detsdw_replica* r, dqmc_series_state* out);
int detsdw_series_binning(detsdw_replica* r, int which, int levels, double* err, double* tau);
int detsdw_series_binning_all(detsdw_replica* r, int which, int levels, double* err, double* tau);
int detsdw_series_save(detsdw_replica* r, const char* path);
int detsdw_series_load(detsdw_replica* r, const char* path);
/* tau_j = j s dtau of the rows of greenKTauX / Y, j = 1 .. n-1: out[n-1] */
int detsdw_get_tau_grid(detsdw_replica* r, double* out);
/* With timeDisplacedEverySlice: tau_k = k dtau of the rows of the ...Fine observables, k = 0 .. m: out[m+1].  Interior rows k = 1 .. m-1
 * are measured in the half-updated field configuration of the stabilisation boundary whose segment they lie in (k < 2 s: boundary 1,
 * else boundary floor(k / s)), by at most s - 1 unstabilised propagation steps from that boundary's G(tau_j,0), G(0,tau_j), G(tau_j);
 * rows 0 and m in the field at the end of the sweep, from G(0) alone.  Row j s equals row j - 1 of the coarse observable bit for bit */
int detsdw_get_tau_grid_fine(detsdw_replica* r, double* out);
/* phi in the reference layout (N, OPDIM, m+1) column-major */
int detsdw_get_phi(detsdw_replica* r, double* phi);
int detsdw_set_phi(detsdw_replica* r, const double* phi);      /* also rebuilds UdV storage and G */
/* the discrete field cdwl(site, k) in the reference layout (N x (m+1) column-major, values +-1 / +-2, slice 0 unused);
 * set needs cdwU != 0 and rebuilds UdV storage and G */
int detsdw_get_cdwl(detsdw_replica* r, int32_t* cdwl);
int detsdw_set_cdwl(detsdw_replica* r, const int32_t* cdwl);
int detsdw_get_green(detsdw_replica* r, dqmc_cplx* g);
int detsdw_get_green_inv_sv(detsdw_replica* r, double* sv);
double detsdw_rng_rand01(detsdw_replica* r);                   /* draws from the replica's stream */
dqmc_ctx* detsdw_ctx(detsdw_replica* r);                       /* kernel context holding the selected chain */
dqmc_ctx* detsdw_ctx_of_chain(detsdw_replica* r, int chain, int* local_index);   /* ... and the chain's index inside it */

/* saveConfigurationStreamBinary (src/detsdwopdim.cpp:4991-5012): appends the current field configuration to
 * <directory>/configs-phi.binarystream in the reference's order (x outer, y, k = 1..m, component; raw fp64), the
 * format its evaluation tools (sdwcorr, deteval) read */
int detsdw_save_configuration_stream_binary(detsdw_replica* r, const char* directory);

/* Checkpoint / resume: field configurations, RNG stream positions, step-size adaptation state and update statistics of
 * every chain (what the reference keeps in simulation.state, src/detsdwopdim.h:1127-1148, src/rngwrapper.h:100-116; own
 * binary format).  detsdw_load_state needs a replica created with the same parameters; it rebuilds UdV storage and
 * G(beta) like the reference's resume does, i.e. the next sweep is a down sweep -- a checkpoint written after an even
 * number of sweeps continues exactly the uninterrupted Markov chain. */
int detsdw_save_state(detsdw_replica* r, const char* path);
int detsdw_load_state(detsdw_replica* r, const char* path);

/* replica-exchange surface (src/detsdwopdim.h:116-153, src/detsdwopdim.cpp:5185-5247) */
double detsdw_get_exchange_parameter_value(detsdw_replica* r);
int detsdw_set_exchange_parameter_value(detsdw_replica* r, double value);
const char* detsdw_get_exchange_parameter_name(detsdw_replica* r);
int detsdw_get_exchange_action_contribution(detsdw_replica* r, double* out);
/* all chains of the handle at once, on the device: out_dev[chain] (device array of detsdw_num_chains doubles) */
int detsdw_exchange_actions_device(detsdw_replica* r, double* out_dev);
int detsdw_get_control_data(detsdw_replica* r, detsdw_control_data* out);
int detsdw_set_control_data(detsdw_replica* r, const detsdw_control_data* in);
/* get_replica_exchange_probability<DetSDW> (src/detsdwopdim.cpp:5251-5264) */
double detsdw_replica_exchange_probability(double par1, double action1, double par2, double action2);

/* RNG restatement, exposed for host-only tests: first n draws of RngWrapper(seed, processIndex) */
int detsdw_rng_fill(uint32_t seed, uint32_t processIndex, double* out, size_t n);
/* The same stream driven through the replica's own RngStream by a script of nops steps, host only: op[i] = DETSDW_RNG_RAND01 (arg[i]
 * single draws), _PEEK (look at the next arg[i] draws without consuming them), _CONSUME (retire arg[i] draws a peek has shown) or
 * _ROUNDTRIP (serialize, then deserialize into a fresh stream that takes over).  Every draw the script sees is written to
 * out[its stream position]; *nout = one past the highest position written.  DQMC_EINVAL: a position beyond cap, a draw that differs
 * from what the same position showed before, a consume past what was peeked, an unknown op. */
enum { DETSDW_RNG_RAND01 = 0, DETSDW_RNG_PEEK = 1, DETSDW_RNG_CONSUME = 2, DETSDW_RNG_ROUNDTRIP = 3 };
int detsdw_rng_replay(uint32_t seed, uint32_t processIndex, const int32_t* op, const uint64_t* arg, size_t nops, double* out, size_t cap,
                      size_t* nout);

#ifdef __cplusplus
}
#endif
#endif /* DETSDW_HOST_H_ */
