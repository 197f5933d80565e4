/*
 * dethubbard_host.h -- C API of the Hubbard replica (BASELINE config 1): the build's DetHubbard
 * (reference src/dethubbard.{h,cpp}: DetModelGC<2, double, false>, discrete Hubbard-Stratonovich field, single
 * spin-flip updates with rank-1 Sherman-Morrison Green's-function updates) on top of the kernel ABI (dqmc_hip.h,
 * dqmc_params::model = DQMC_MODEL_HUBBARD).  Same layering as detsdw_host.h: the C++ host class
 * (detqmc_amd/csrc/host/dethubbard.{h,cpp}) owns the RNG stream and the control flow of sweep_skeleton / sweepUp /
 * sweepDown (src/detmodel.h:1266-1478) and calls ONLY the kernel ABI.
 */
#ifndef DETHUBBARD_HOST_H_
#define DETHUBBARD_HOST_H_

#include <stddef.h>
#include <stdint.h>
#include "dqmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dethubbard_replica dethubbard_replica;

/* ModelParams<DetHubbard> (src/dethubbardparams.h:28-50) + rngSeed / simindex of DetQMCParams */
typedef struct dethubbard_params {
    int32_t L;                   /* linear size; d = 2 (the only dimension this build supports) */
    int32_t d;
    int32_t m;                   /* give m > 0 OR beta > 0 (src/detmodelparams.h:97-110) */
    int32_t s;
    int32_t checkerboard;        /* 0: e^{-dtau T} by diagonalisation; 1: checkerboard product form (no chemical potential) */
    int32_t device;
    int32_t simindex;
    uint32_t rngSeed;
    int32_t stabilisation;       /* DQMC_STAB_SVD (as the reference) or DQMC_STAB_QR */
    int32_t measureFlags;        /* DETHUBBARD_MEASURE_* bits; 0: the eight scalars and zcorr only.  Any other bit, _TD_FINE without _TD: ParameterWrong */
    double beta, dtau;
    double t, U, mu;
} dethubbard_params;

/* dethubbard_params::measureFlags (the word was `reserved`: same offset and size, 0 = what it always meant).
 * _EQ: a measurement sweep also bins the equal-time correlators of dqmc_hubbard_set_equal_time_correlators on all m slices.
 * _TD: the kernel context is created with the time-displaced reservation, and a measurement sweep computes G(tau_j,0), G(0,tau_j),
 *      G(0) at every interior boundary j = 1 .. n-1 of its direction and bins dqmc_hubbard_measure_timedisplaced(j) there.
 * _TD_FINE (needs _TD, and s < m as given; ParameterWrong otherwise): the kernel context also gets the every-slice reservation
 *      (DQMC_TD_HUB_EVERY_SLICE), and a measurement sweep bins all eight channels on the grid tau_k = k dtau, k = 0 .. m: after
 *      dqmc_hubbard_measure_timedisplaced(j) the segment of boundary j, after the closing advance rows 0 and m.
 * None changes the Markov chain, the eight scalars, zcorr or the blocks of the other flags; thermalisation sweeps launch nothing new. */
enum { DETHUBBARD_MEASURE_EQ = 1, DETHUBBARD_MEASURE_TD = 2, DETHUBBARD_MEASURE_TD_FINE = 4 };

/* obsScalar of DetHubbard (src/dethubbard.cpp:85-93), valid after dethubbard_sweep(r, 1) */
typedef struct dethubbard_observables {
    double occUp, occDn, occTotal, occDouble, localMoment, eKinetic, ePotential, eTotal;
    int32_t valid, reserved;
} dethubbard_observables;

typedef struct dethubbard_info {
    int32_t L, N, m, s, n, performedSweeps, lastSweepDir, currentTimeslice;
    double beta, dtau, alpha, lastAccRatio;
    uint64_t rngDrawn;
} dethubbard_info;

/* createReplica (src/dethubbard.cpp:37-47) + ctor (:49-118): parameter checks, random auxiliary field, propagator,
 * UdV storage and G(beta).  nchains independent replicas (simindex, simindex + 1, ...) advance in lockstep. */
int dethubbard_create(const dethubbard_params* p, int nchains, dethubbard_replica** out);
void dethubbard_destroy(dethubbard_replica* r);
const char* dethubbard_last_error(void);
int dethubbard_select_chain(dethubbard_replica* r, int chain);
/* DetHubbard::sweep / sweepThermalization (src/dethubbard.cpp:921-945) */
int dethubbard_sweep(dethubbard_replica* r, int takeMeasurements);
int dethubbard_sweep_thermalization(dethubbard_replica* r);
int dethubbard_get_info(dethubbard_replica* r, dethubbard_info* out);
/* auxfield(N, m + 1) column-major as doubles +-1 (column 0 unused), gUp / gDn N x N column-major */
int dethubbard_get_auxfield(dethubbard_replica* r, double* out);
int dethubbard_get_green(dethubbard_replica* r, double* gUp, double* gDn);
int dethubbard_get_observables(dethubbard_replica* r, dethubbard_observables* out);
int dethubbard_get_zcorr(dethubbard_replica* r, double* out /* [N] */);
/* Normalised correlators C_X(d) = sum / (count N) of the last measurement sweep, selected chain, index dy L + dx (dqmc_hip.h: Hubbard
 * model).  Equal time: greenUp, greenDn, charge, spinZZ, spinXX, pairS, pairSx, pairD; time-displaced: the first six at tau_j = j s dtau,
 * j = 1 .. n-1.  DQMC_EINVAL without the flag, before a measurement sweep, and while a series with DETHUBBARD_SERIES_NO_HOST_COPY is
 * open (below).  Values of ONE sweep; averages and error bars over sweeps: the measurement series at the end of this header. */
int dethubbard_get_eq_correlators(dethubbard_replica* r, double* out /* [8][N] */);
int dethubbard_get_td_correlators(dethubbard_replica* r, double* out /* [n-1][6][N] */);
/* DETHUBBARD_MEASURE_TD_FINE: all eight channels on every time slice, C_X(d, tau_k) = sum / (count N), k = 0 .. m, selected chain; refused
 * like the two getters above.  dethubbard_get_matsubara / _all: chi_X(q, i omega_n) (channels 2 .. 7, omega_n = 2 pi n / beta) and
 * G_s(k, i omega_n) (channels 0, 1, omega_n = (2n+1) pi / beta) of dqmc_hubbard_td_matsubara_host, n = 0 .. nfreq-1, 1 <= nfreq <= m, complex
 * as (re, im), column qy L + qx; of the selected chain / of every chain.  They read the block on the device: valid after a measurement sweep
 * until the next sweep of either kind (DQMC_EINVAL outside that window), also while a series with DETHUBBARD_SERIES_NO_HOST_COPY is open. */
int dethubbard_get_td_fine_correlators(dethubbard_replica* r, double* out /* [m+1][8][N] */);
int dethubbard_get_matsubara(dethubbard_replica* r, int nfreq, double* out /* [8][nfreq][N] complex */);
int dethubbard_get_matsubara_all(dethubbard_replica* r, int nfreq, double* out /* [nchains][8][nfreq][N] complex */);
/* Checkpoint / resume (what DetQMC::saveState keeps for the replica: auxfield, src/dethubbard.h:352-358, plus the position of
 * the random stream); dethubbard_load_state needs a replica created with the same parameters and rebuilds UdV storage and G(beta)
 * like the reference's loadContents does (src/dethubbard.h:345-350) */
int dethubbard_save_state(dethubbard_replica* r, const char* path);
int dethubbard_load_state(dethubbard_replica* r, const char* path);
double dethubbard_rng_rand01(dethubbard_replica* r);
/* Wrap-error diagnostics (dqmc_set_green_check in dqmc_hip.h: definitions and table layout).  dethubbard_set_green_check(r, on): the
 * switch of the replica's kernel context, between sweeps; this replica's sweeps take no shortcut at segment ends, so every advance of a
 * sweep samples and the chain does not depend on the switch.  dethubbard_get_green_check: out[nchains][2][n+1][DQMC_GREEN_CHECK_FIELDS];
 * it and the reset return DQMC_EINVAL while the switch is off.  The table is per chain and is not part of dethubbard_save_state. */
int dethubbard_set_green_check(dethubbard_replica* r, int on);
int dethubbard_get_green_check(dethubbard_replica* r, double* out);
int dethubbard_reset_green_check(dethubbard_replica* r);
dqmc_ctx* dethubbard_ctx(dethubbard_replica* r);

/* Measurement series: bins over measurement sweeps and jackknife errors, kept on the device (dqmc_series_* with the DQMC_SERIES_HUB_*
 * parts, dqmc_hip.h).  The calls have the semantics of their detsdw_series_* namesakes (detsdw_host.h).
 * dethubbard_series_begin: the parts follow from the handle -- scalars and zcorr always, the equal-time part with DETHUBBARD_MEASURE_EQ,
 *   the time-displaced part with DETHUBBARD_MEASURE_TD and n >= 2.  flags: DETHUBBARD_SERIES_NO_HOST_COPY or 0; any other bit is
 *   ParameterWrong.  While the series is open every dethubbard_sweep(r, 1) ends with one sample of every chain added to the series;
 *   thermalisation sweeps and dethubbard_sweep(r, 0) add nothing.  A measurement sweep on a full series (maxBins bins closed, no
 *   automatic re-binning) fails with DQMC_EINVAL before it pushes uniforms or touches the field.  The Markov chain does not depend on
 *   the series or its flags.
 *   DETHUBBARD_SERIES_NO_HOST_COPY: while the series is open a measurement sweep does not read the equal-time and time-displaced blocks
 *   back; dethubbard_get_eq_correlators / _td_correlators fail with a message that names NO_HOST_COPY, and a block without a sample is
 *   reported by the series' own flags.  The scalars and zcorr of dethubbard_get_observables / _get_zcorr are still filled.
 * Readers take an observable index DETHUBBARD_OBS_*: SCALARS [8] (the order of dethubbard_observables), ZCORR [N], the eight C_X(d) [N]
 *   (DETHUBBARD_OBS_GREENUPCORR + X) and S_X(q) [N] (DETHUBBARD_OBS_GREENUPSQ + X, column qy L + qx) of the equal-time channels, the six
 *   C_X(d, tau_j) [n-1][N] (DETHUBBARD_OBS_GREENUPTAU + X) and S_X(q, tau_j) [n-1][N] (DETHUBBARD_OBS_GREENUPTAUSQ + X; for greenUp,
 *   greenDn: Re G_s(k, tau_j)).  An index whose part the series lacks is ParameterWrong.
 *   dethubbard_series_stats: mean and err of `which`, the selected chain; _stats_all: every chain, [nchains] x the same;
 *   _read_bins: closed bins first .. first + count - 1 of `which`, selected chain; _binning / _binning_all: err (and tau unless NULL;
 *   tau needs DQMC_SERIES_TRACK_VARIANCE) [levels] x the shape, _all: [nchains][levels] x the shape.
 *   dethubbard_series_derived_all: value[nchains][19], err[nchains][19] of dqmc_series_hubbard_derived_host at Q = (qx, qy).
 * dethubbard_series_configure / _rebin / _get_state: dqmc_series_configure / _rebin / _get_state of the kernel context.
 * dethubbard_series_save / _load: the series file of detsdw_series_save -- magic "DQMCSER1", int32 version, dqmc_series_state, the route
 *   [nchains] int32 (written as the identity: this replica has no routing), then per chain the closed bins [bins_closed][S], the open bin
 *   [S] and, if the variance is tracked, w [S] and m2 [S].  _load needs an open series with the same number of chains, parts and sample
 *   length; every refusal leaves the series as it was.  dethubbard_save_state / _load_state and their file do not change: a checkpoint
 *   of a run with a series is the two files.  dethubbard_destroy ends an open series. */
enum { DETHUBBARD_SERIES_NO_HOST_COPY = 1 };
enum { DETHUBBARD_OBS_SCALARS = 0, DETHUBBARD_OBS_ZCORR = 1, DETHUBBARD_OBS_GREENUPCORR = 2, DETHUBBARD_OBS_GREENUPSQ = 10,
       DETHUBBARD_OBS_GREENUPTAU = 18, DETHUBBARD_OBS_GREENUPTAUSQ = 24, DETHUBBARD_OBS_COUNT = 30 };
int dethubbard_series_begin(dethubbard_replica* r, int binSize, int maxBins, int flags);
int dethubbard_series_info(dethubbard_replica* r, int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen);
int dethubbard_series_stats(dethubbard_replica* r, int which, double* mean, double* err);
int dethubbard_series_stats_all(dethubbard_replica* r, int which, double* mean, double* err);
int dethubbard_series_read_bins(dethubbard_replica* r, int which, int first, int count, double* out);
int dethubbard_series_derived_all(dethubbard_replica* r, int qx, int qy, double* value, double* err);
int dethubbard_series_configure(dethubbard_replica* r, int flags);
int dethubbard_series_rebin(dethubbard_replica* r);
int dethubbard_series_get_state(dethubbard_replica* r, dqmc_series_state* out);
int dethubbard_series_binning(dethubbard_replica* r, int which, int levels, double* err, double* tau);
int dethubbard_series_binning_all(dethubbard_replica* r, int which, int levels, double* err, double* tau);
int dethubbard_series_save(dethubbard_replica* r, const char* path);
int dethubbard_series_load(dethubbard_replica* r, const char* path);
int dethubbard_series_end(dethubbard_replica* r);

#ifdef __cplusplus
}
#endif
#endif /* DETHUBBARD_HOST_H_ */
