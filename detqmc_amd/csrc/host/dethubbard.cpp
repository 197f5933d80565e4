// Host control flow of the Hubbard replica (see dethubbard.h).  Mirrors:
//   createReplica / updateTemperatureParameters / ModelParams<DetHubbard>::check   src/dethubbard.cpp:37-47, src/detmodelparams.h:68-122,
//                                                                                   src/dethubbardparams.cpp:21-55
//   DetHubbard ctor, setupRandomAuxfield                                            src/dethubbard.cpp:49-118, 690-700
//   sweep_skeleton / sweepDown / sweepUp (no global move in this model)             src/detmodel.h:1266-1478
//   initMeasurements / finishMeasurements                                           src/dethubbard.cpp:501-519, 637-649
// All numerics go through the C ABI in include/dqmc_hip.h.
#include "dethubbard.h"
#include <cmath>
#include <cstdio>
#include <cstring>

namespace detqmc {

void DetHubbard::check(int rc, const char* what) {
    if (rc != DQMC_OK) throw GeneralError(rc, std::string(what) + ": " + dqmc_last_error());
}

DetHubbard::DetHubbard(const dethubbard_params& in, int nchains) : p_(in) {
    if (nchains < 1) throw ParameterWrong("need at least one replica");
    // updateTemperatureParameters (detmodelparams.h:68-122)
    if (!(p_.dtau > 0)) throw ParameterWrong("Parameter dtau has incorrect value");
    if (p_.s <= 0) throw ParameterWrong("Parameter s has incorrect value");
    if (p_.beta > 0 && p_.m > 0) throw ParameterWrong("Only specify one of the parameters beta and m");
    if (!(p_.beta > 0) && p_.m <= 0) throw ParameterWrong("Specify either parameter m or beta");
    if (p_.m <= 0) p_.m = (int32_t)std::round(p_.beta / p_.dtau);
    p_.beta = p_.m * p_.dtau;
    if ((p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE) && p_.s >= p_.m)
        throw ParameterWrong("Parameter measureFlags: DETHUBBARD_MEASURE_TD_FINE needs s < m (at least one interior boundary)");
    while (p_.m <= p_.s) p_.s -= 1;
    if (p_.s < 1) throw ParameterWrong("Cannot choose parameter s obeying 0 < s < m");
    // ModelParams<DetHubbard>::check (dethubbardparams.cpp:21-55)
    if (p_.L <= 0) throw ParameterWrong("Parameter L has incorrect value");
    if (p_.d != 2) throw ParameterWrong("Hubbard replica: only d = 2 lattices are supported by this build");
    if (p_.checkerboard && p_.L % 2 != 0) throw ParameterWrong("Checker board decomposition only supported for even linear lattice sizes");
    if (p_.L % 2 != 0) throw ParameterWrong("this build needs an even linear lattice size");
    if (p_.measureFlags & ~(DETHUBBARD_MEASURE_EQ | DETHUBBARD_MEASURE_TD | DETHUBBARD_MEASURE_TD_FINE))
        throw ParameterWrong("Parameter measureFlags has an unknown bit set");
    if ((p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE) && !(p_.measureFlags & DETHUBBARD_MEASURE_TD))
        throw ParameterWrong("Parameter measureFlags: DETHUBBARD_MEASURE_TD_FINE needs DETHUBBARD_MEASURE_TD");
    N_ = p_.L * p_.L; m_ = p_.m; s_ = p_.s; n_ = (m_ + s_ - 1) / s_;
    alpha_ = std::acosh(std::exp(p_.dtau * p_.U * 0.5));

    dqmc_params kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.model = DQMC_MODEL_HUBBARD;
    kp.opdim = 1; kp.L = p_.L; kp.m = m_; kp.s = s_; kp.delaySteps = 1; kp.bc = DQMC_BC_PBC; kp.device = p_.device;
    kp.stabilisation = p_.stabilisation; kp.cb_none = p_.checkerboard ? 0 : 1;
    kp.dtau = p_.dtau; kp.txhor = p_.t; kp.u = p_.U; kp.mux = p_.mu; kp.muy = p_.mu; kp.accRatio = 0.5;
    kp.tuning.bmult_path = DQMC_TUNING_NO_RNG_LOOKAHEAD;     // this replica pushes every window whole (beginLocalUpdates)
    if (p_.measureFlags & DETHUBBARD_MEASURE_TD) { kp.timedisplaced = 1; kp.td_particle_hole = 1; }   // G(tau,0), G(0,tau), G(0) and the block
    if (p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE) kp.timedisplaced |= DQMC_TD_HUB_EVERY_SLICE;    // the work copies and the every-slice block
    check(dqmc_create_batch(&kp, nchains, &ctx_), "dqmc_create");
    try {
        std::vector<double> all((size_t)nchains * (m_ + 1) * N_, 0.0);
        for (int b = 0; b < nchains; ++b) {
            ch_.emplace_back(p_.rngSeed, (uint32_t)(p_.simindex + b));
            Chain& c = ch_.back();
            c.aux.assign((size_t)(m_ + 1) * N_, 0.0);
            for (int k = 1; k <= m_; ++k)                                    // setupRandomAuxfield (:690-700)
                for (int site = 0; site < N_; ++site) c.aux[(size_t)k * N_ + site] = (c.rng.rand01() <= 0.5) ? +1.0 : -1.0;
            // slice 0 is never used; +1 keeps the cosh/sinh helper kernel away from 0/0
            for (int site = 0; site < N_; ++site) c.aux[site] = 1.0;
            std::memcpy(&all[(size_t)b * (m_ + 1) * N_], c.aux.data(), c.aux.size() * sizeof(double));
        }
        check(dqmc_set_fields_all_host(ctx_, all.data()), "dqmc_set_fields_all_host");
        check(dqmc_udv_setup(ctx_), "setupUdVStorage_and_calculateGreen");
    } catch (...) {
        dqmc_destroy(ctx_);
        throw;
    }
}

DetHubbard::~DetHubbard() {
    if (seriesOpen_) (void)dqmc_series_end(ctx_);
    dqmc_destroy(ctx_);
}

void DetHubbard::updateInSlice(int k) {
    check(dqmc_update_slice(ctx_, k, 0), "updateInSlice");
    if (measuring_) check(dqmc_measure_slice(ctx_), "measure");     // updateInSliceAndMaybeMeasure (detmodel.h:1279-1285)
}

// an advance, and on the interior boundary it ends on the time-displaced correlators of that boundary (measurement sweeps with
// DETHUBBARD_MEASURE_TD: the context has just formed G(tau_j,0), G(0,tau_j) and G(0) next to G(tau_j))
void DetHubbard::advance(int dir, int l, int boundary, const char* what) {
    check(dqmc_advance(ctx_, dir, l), what);
    if (measuringTD_ && boundary) check(dqmc_hubbard_measure_timedisplaced(ctx_, boundary), "measureTimeDisplaced");
    if (measuringFine_ && boundary) check(dqmc_hubbard_measure_timedisplaced_segment(ctx_, boundary), "measureTimeDisplacedSegment");
    if (measuringFine_ && !boundary) check(dqmc_hubbard_measure_timedisplaced_ends(ctx_), "measureTimeDisplacedEnds");
}

void DetHubbard::sweepDown() {                                      // detmodel.h:1333-1399
    for (int k = m_; k >= (n_ - 1) * s_ + 1; --k) { updateInSlice(k); check(dqmc_wrap(ctx_, DQMC_DOWN, k), "wrapDownGreen"); }
    for (int l = n_ - 1; l >= 1; --l) {
        advance(DQMC_DOWN, l + 1, l, "advanceDownGreen");
        for (int k = l * s_; k >= (l - 1) * s_ + 1; --k) { updateInSlice(k); check(dqmc_wrap(ctx_, DQMC_DOWN, k), "wrapDownGreen"); }
    }
    advance(DQMC_DOWN, 1, 0, "advanceDownGreen");
}

void DetHubbard::sweepUp() {                                        // detmodel.h:1266-1325
    check(dqmc_reset_storage0(ctx_), "reset storage[0]");
    for (int l = 0; l <= n_ - 2; ++l) {
        for (int k = l * s_ + 1; k <= (l + 1) * s_; ++k) { check(dqmc_wrap(ctx_, DQMC_UP, k - 1), "wrapUpGreen"); updateInSlice(k); }
        advance(DQMC_UP, l, l + 1, "advanceUpGreen");
    }
    for (int k = (n_ - 1) * s_ + 1; k <= m_; ++k) { check(dqmc_wrap(ctx_, DQMC_UP, k - 1), "wrapUpGreen"); updateInSlice(k); }
    advance(DQMC_UP, n_ - 1, 0, "advanceUpGreen");
}

void DetHubbard::sweep_skeleton(bool takeMeasurements) {
    const size_t need = (size_t)2 * N_ * m_;                        // per proposal: one draw for the site, at most one for Metropolis
    const size_t nb = ch_.size();
    const bool feedSeries = takeMeasurements && seriesOpen_;
    if (feedSeries) {                  // nothing is dropped silently, and nothing has changed yet
        dqmc_series_state st;
        check(dqmc_series_get_state(ctx_, &st), "dqmc_series_get_state");
        if (st.bins_closed >= st.max_bins) throw GeneralError(DQMC_EINVAL, "the measurement series is full (maxBins bins are closed): read it out and end it");
    }
    window_.resize(need * nb);
    for (size_t b = 0; b < nb; ++b) std::memcpy(&window_[b * need], ch_[b].rng.peek(need), need * sizeof(double));
    check(dqmc_push_uniforms_all_host(ctx_, window_.data(), need), "dqmc_push_uniforms_all_host");
    if (takeMeasurements) check(dqmc_measure_reset(ctx_), "initMeasurements");
    measuring_ = takeMeasurements;
    // the correlators ride on measurement sweeps only: thermalisation sweeps launch nothing new and never form the time-displaced pair
    const bool eq = takeMeasurements && (p_.measureFlags & DETHUBBARD_MEASURE_EQ);
    measuringTD_ = takeMeasurements && (p_.measureFlags & DETHUBBARD_MEASURE_TD);
    measuringFine_ = takeMeasurements && (p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE);
    fineLive_ = false;
    if (eq) check(dqmc_hubbard_set_equal_time_correlators(ctx_, 1), "dqmc_hubbard_set_equal_time_correlators");
    if (measuringTD_) check(dqmc_set_timedisplaced(ctx_, 1), "dqmc_set_timedisplaced");
    auto off = [this, eq]() {
        if (eq) (void)dqmc_hubbard_set_equal_time_correlators(ctx_, 0);
        if (measuringTD_) (void)dqmc_set_timedisplaced(ctx_, 0);
        measuring_ = measuringTD_ = measuringFine_ = false;
    };
    try {
        if (lastSweepDir_ == Up) sweepDown(); else sweepUp();
    } catch (...) { off(); throw; }
    off();
    lastSweepDir_ = (lastSweepDir_ == Up) ? Down : Up;
    ++performedSweeps_;
    std::vector<dqmc_update_state> st(nb);
    check(dqmc_get_update_states_all_host(ctx_, st.data()), "dqmc_get_update_states_all_host");
    for (size_t b = 0; b < nb; ++b) {
        ch_[b].rng.consume((size_t)st[b].rng_consumed);
        ch_[b].lastAccRatio = st[b].lastAccRatio;
        if (takeMeasurements) finishMeasurements((int)b); else ch_[b].obs.valid = 0;
    }
    if (takeMeasurements) corrStale_ = seriesNoHostCopy();
    fineLive_ = takeMeasurements && (p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE);
    if (feedSeries) check(dqmc_series_add_sweep(ctx_), "dqmc_series_add_sweep");     // one sample of every chain, from the blocks on the device
}

void DetHubbard::sweep(bool takeMeasurements) { sweep_skeleton(takeMeasurements); }

// finishMeasurements (dethubbard.cpp:637-649) from the device accumulators (layout: kernels_hubbard.hip)
void DetHubbard::finishMeasurements(int b) {
    check(dqmc_select_chain(ctx_, b), "dqmc_select_chain");
    std::vector<double> acc(dqmc_measure_accum_size(ctx_));
    check(dqmc_measure_read_host(ctx_, acc.data()), "dqmc_measure_read_host");
    if ((int)acc[5] != m_) throw GeneralError(DQMC_EINVAL, "measurement sweep did not visit every time slice");
    const double N = N_, m = m_;
    dethubbard_observables& o = ch_[b].obs;
    o.valid = 0;
    o.occUp = 1.0 - (1.0 / (N * m)) * acc[0];
    o.occDn = 1.0 - (1.0 / (N * m)) * acc[1];
    o.occTotal = o.occUp + o.occDn;
    o.occDouble = 1.0 + (1.0 / (N * m)) * (acc[4] - acc[0] - acc[1]);
    o.localMoment = o.occTotal - 2 * o.occDouble;
    o.ePotential = p_.U * o.occDouble;
    o.eKinetic = (p_.t / (N * m)) * (acc[2] + acc[3]) - p_.mu * o.occTotal;
    o.eTotal = o.eKinetic + o.ePotential;
    ch_[b].zcorr.assign(N_, 0.0);
    for (int j = 0; j < N_; ++j) ch_[b].zcorr[j] = acc[6 + j] / m;
    const bool copy = !seriesNoHostCopy();                          // without it the series' own flags report a block without a sample
    if (copy && (p_.measureFlags & DETHUBBARD_MEASURE_EQ)) {        // count, [8][N] raw sums -> C(d) = sum / (count N)
        std::vector<double> blk(dqmc_hubbard_eq_accum_size(ctx_));
        check(dqmc_hubbard_eq_read_host(ctx_, blk.data()), "dqmc_hubbard_eq_read_host");
        if ((int)blk[0] != m_) throw GeneralError(DQMC_EINVAL, "measurement sweep did not bin the equal-time correlators on every time slice");
        ch_[b].eqCorr.assign(blk.size() - 1, 0.0);
        for (size_t i = 0; i + 1 < blk.size(); ++i) ch_[b].eqCorr[i] = blk[1 + i] / (m * N);
    }
    if (copy && (p_.measureFlags & DETHUBBARD_MEASURE_TD)) {        // count[n-1], [n-1][6][N]
        std::vector<double> blk(dqmc_hubbard_td_accum_size(ctx_));
        check(dqmc_hubbard_td_read_host(ctx_, blk.data()), "dqmc_hubbard_td_read_host");
        const size_t rows = (size_t)(n_ - 1), row = (blk.size() - rows) / (rows ? rows : 1);
        ch_[b].tdCorr.assign(rows * row, 0.0);
        for (size_t j = 0; j < rows; ++j) {
            if ((int)blk[j] != 1) throw GeneralError(DQMC_EINVAL, "measurement sweep did not take one time-displaced sample per interior boundary");
            for (size_t i = 0; i < row; ++i) ch_[b].tdCorr[j * row + i] = blk[rows + j * row + i] / N;
        }
    }
    if (p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE) {             // count[m+1], [m+1][8][N]; without the copy only the m + 1 counts are read
        const size_t rows = (size_t)m_ + 1, row = (size_t)8 * N_;
        std::vector<double> blk(copy ? dqmc_hubbard_td_fine_accum_size(ctx_) : rows);
        if (copy) check(dqmc_hubbard_td_fine_read_host(ctx_, blk.data()), "dqmc_hubbard_td_fine_read_host");
        else check(dqmc_hubbard_td_fine_counts_host(ctx_, blk.data()), "dqmc_hubbard_td_fine_counts_host");
        for (size_t k = 0; k < rows; ++k)
            if (blk[k] != 1.0) throw GeneralError(DQMC_EINVAL, "measurement sweep did not take one every-slice sample per time slice");
        if (copy) {
            ch_[b].tdFineCorr.assign(rows * row, 0.0);
            for (size_t i = 0; i < rows * row; ++i) ch_[b].tdFineCorr[i] = blk[rows + i] / N;
        }
    }
    o.valid = 1;                                                    // last: a sweep that threw above leaves no half-read observables behind
}

void DetHubbard::getEqCorrelators(double* out, int b) const {
    if (!(p_.measureFlags & DETHUBBARD_MEASURE_EQ)) throw GeneralError(DQMC_EINVAL, "the equal-time correlators need DETHUBBARD_MEASURE_EQ in measureFlags");
    if (seriesNoHostCopy())
        throw GeneralError(DQMC_EINVAL, "the correlators are not copied to the host while a series with DETHUBBARD_SERIES_NO_HOST_COPY is open: read the series");
    if (!ch_[b].obs.valid || corrStale_) throw GeneralError(DQMC_EINVAL, "no measurement has been taken");
    std::memcpy(out, ch_[b].eqCorr.data(), ch_[b].eqCorr.size() * sizeof(double));
}

void DetHubbard::getTdCorrelators(double* out, int b) const {
    if (!(p_.measureFlags & DETHUBBARD_MEASURE_TD)) throw GeneralError(DQMC_EINVAL, "the time-displaced correlators need DETHUBBARD_MEASURE_TD in measureFlags");
    if (seriesNoHostCopy())
        throw GeneralError(DQMC_EINVAL, "the correlators are not copied to the host while a series with DETHUBBARD_SERIES_NO_HOST_COPY is open: read the series");
    if (!ch_[b].obs.valid || corrStale_) throw GeneralError(DQMC_EINVAL, "no measurement has been taken");
    std::memcpy(out, ch_[b].tdCorr.data(), ch_[b].tdCorr.size() * sizeof(double));
}

void DetHubbard::getTdFineCorrelators(double* out, int b) const {
    if (!(p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE)) throw GeneralError(DQMC_EINVAL, "the every-slice correlators need DETHUBBARD_MEASURE_TD_FINE in measureFlags");
    if (seriesNoHostCopy())
        throw GeneralError(DQMC_EINVAL, "the correlators are not copied to the host while a series with DETHUBBARD_SERIES_NO_HOST_COPY is open: read the series");
    if (!ch_[b].obs.valid || corrStale_) throw GeneralError(DQMC_EINVAL, "no measurement has been taken");
    std::memcpy(out, ch_[b].tdFineCorr.data(), ch_[b].tdFineCorr.size() * sizeof(double));
}

void DetHubbard::getMatsubara(int nfreq, double* out, int b) {
    if (!(p_.measureFlags & DETHUBBARD_MEASURE_TD_FINE)) throw GeneralError(DQMC_EINVAL, "the Matsubara transforms need DETHUBBARD_MEASURE_TD_FINE in measureFlags");
    if (!fineLive_) throw GeneralError(DQMC_EINVAL, "the Matsubara transforms are valid after a measurement sweep, until the next sweep");
    const size_t all = dqmc_hubbard_td_matsubara_size(ctx_, nfreq);
    if (!all) throw GeneralError(DQMC_EINVAL, "nfreq must be in 1..m");
    if (b < 0) { check(dqmc_hubbard_td_matsubara_host(ctx_, nfreq, out), "dqmc_hubbard_td_matsubara_host"); return; }
    std::vector<double> buf(all);
    check(dqmc_hubbard_td_matsubara_host(ctx_, nfreq, buf.data()), "dqmc_hubbard_td_matsubara_host");
    const size_t per = all / ch_.size();
    std::memcpy(out, &buf[(size_t)b * per], per * sizeof(double));
}

void DetHubbard::getZcorr(double* out, int b) const {
    if (!ch_[b].obs.valid) throw GeneralError(DQMC_EINVAL, "no measurement has been taken");
    std::memcpy(out, ch_[b].zcorr.data(), ch_[b].zcorr.size() * sizeof(double));
}

void DetHubbard::getInfo(dethubbard_info& o, int b) {
    std::memset(&o, 0, sizeof(o));
    o.L = p_.L; o.N = N_; o.m = m_; o.s = s_; o.n = n_; o.performedSweeps = performedSweeps_; o.lastSweepDir = (int)lastSweepDir_;
    o.currentTimeslice = dqmc_current_timeslice(ctx_);
    o.beta = p_.beta; o.dtau = p_.dtau; o.alpha = alpha_; o.lastAccRatio = ch_[b].lastAccRatio; o.rngDrawn = ch_[b].rng.drawn();
}

void DetHubbard::getAuxfield(double* out, int b) {
    check(dqmc_select_chain(ctx_, b), "dqmc_select_chain");
    check(dqmc_get_fields_host(ctx_, ch_[b].aux.data(), nullptr, nullptr), "dqmc_get_fields_host");
    // device layout [m+1][N] == the reference's auxfield(N, m+1) column-major
    std::memcpy(out, ch_[b].aux.data(), ch_[b].aux.size() * sizeof(double));
}

void DetHubbard::getGreen(double* gUp, double* gDn, int b) {
    check(dqmc_select_chain(ctx_, b), "dqmc_select_chain");
    const int ng = 2 * N_;
    std::vector<dqmc_cplx> g((size_t)ng * ng);
    check(dqmc_get_green_host(ctx_, g.data()), "dqmc_get_green_host");
    for (int j = 0; j < N_; ++j)
        for (int i = 0; i < N_; ++i) {
            if (gUp) gUp[(size_t)j * N_ + i] = g[(size_t)j * ng + i].re;
            if (gDn) gDn[(size_t)j * N_ + i] = g[(size_t)(N_ + j) * ng + (N_ + i)].re;
        }
}

// ---- measurement series (include/dethubbard_host.h): one dqmc_series on the kernel context ----
void DetHubbard::seriesBegin(int binSize, int maxBins, int flags) {
    if (seriesOpen_) throw GeneralError(DQMC_EINVAL, "a measurement series is already open");
    if (flags & ~DETHUBBARD_SERIES_NO_HOST_COPY) throw ParameterWrong("unknown flag of dethubbard_series_begin");
    int parts = DQMC_SERIES_HUB_SCALARS;
    if (p_.measureFlags & DETHUBBARD_MEASURE_EQ) parts |= DQMC_SERIES_HUB_EQ;
    if ((p_.measureFlags & DETHUBBARD_MEASURE_TD) && n_ >= 2) parts |= DQMC_SERIES_HUB_TD;
    if ((parts & DQMC_SERIES_HUB_EQ) && !dqmc_hubbard_eq_accum_size(ctx_)) {     // the first enable allocates the block; measurement sweeps switch it on themselves
        check(dqmc_hubbard_set_equal_time_correlators(ctx_, 1), "dqmc_hubbard_set_equal_time_correlators");
        check(dqmc_hubbard_set_equal_time_correlators(ctx_, 0), "dqmc_hubbard_set_equal_time_correlators");
    }
    check(dqmc_series_begin(ctx_, binSize, maxBins, 0, parts), "dqmc_series_begin");
    seriesOpen_ = true; seriesParts_ = parts; seriesFlags_ = flags;
}
void DetHubbard::seriesEnd() {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    seriesOpen_ = false;
    check(dqmc_series_end(ctx_), "dqmc_series_end");
}
void DetHubbard::seriesInfo(int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    check(dqmc_series_info(ctx_, binsClosed, sweepsInOpenBin, sampleLen), "dqmc_series_info");
}
DetHubbard::SeriesSlice DetHubbard::seriesSlice(int which) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    if (which < 0 || which >= DETHUBBARD_OBS_COUNT) throw ParameterWrong("the measurement series does not hold this observable");
    const size_t N = (size_t)N_, rows = (size_t)(n_ > 1 ? n_ - 1 : 0);
    int part;
    SeriesSlice s{0, 1, 0, N};
    if (which == DETHUBBARD_OBS_SCALARS) { part = 14; s.len = 8; }
    else if (which == DETHUBBARD_OBS_ZCORR) { part = 14; s.off = 8; }
    else if (which < DETHUBBARD_OBS_GREENUPTAU) { part = 15; s.off = (size_t)(which - DETHUBBARD_OBS_GREENUPCORR) * N; }   // C_X [8][N], then S_X [8][N]
    else {                                                  // C_X [n-1][6][N], then S_X [n-1][6][N]: channel X of every row
        part = 16;
        const bool sq = which >= DETHUBBARD_OBS_GREENUPTAUSQ;
        const size_t X = (size_t)(which - (sq ? DETHUBBARD_OBS_GREENUPTAUSQ : DETHUBBARD_OBS_GREENUPTAU));
        s.off = (sq ? rows * 6 * N : 0) + X * N; s.rows = rows; s.stride = 6 * N;
    }
    if (!(seriesParts_ & (1 << part)))
        throw ParameterWrong(part == 15 ? "the series has no equal-time part: the handle needs DETHUBBARD_MEASURE_EQ"
                                        : "the series has no time-displaced part: the handle needs DETHUBBARD_MEASURE_TD and n >= 2");
    size_t off = 0, len = 0;
    check(dqmc_series_layout(ctx_, part, &off, &len), "dqmc_series_layout");
    s.off += off;
    return s;
}
void DetHubbard::seriesStats(int which, double* mean, double* err, int b) {
    const SeriesSlice s = seriesSlice(which);
    size_t S = 0;
    check(dqmc_series_info(ctx_, nullptr, nullptr, &S), "dqmc_series_info");
    std::vector<double> mu(ch_.size() * S), er(ch_.size() * S);
    check(dqmc_series_stats_host(ctx_, mu.data(), er.data()), "dqmc_series_stats_host");
    for (size_t j = 0; j < s.rows; ++j) {
        std::memcpy(mean + j * s.len, &mu[(size_t)b * S + s.off + j * s.stride], s.len * sizeof(double));
        std::memcpy(err + j * s.len, &er[(size_t)b * S + s.off + j * s.stride], s.len * sizeof(double));
    }
}
void DetHubbard::seriesStatsAll(int which, double* mean, double* err) {
    const SeriesSlice s = seriesSlice(which);
    size_t S = 0;
    check(dqmc_series_info(ctx_, nullptr, nullptr, &S), "dqmc_series_info");
    std::vector<double> mu(ch_.size() * S), er(ch_.size() * S);
    check(dqmc_series_stats_host(ctx_, mu.data(), er.data()), "dqmc_series_stats_host");
    const size_t per = s.rows * s.len;
    for (size_t b = 0; b < ch_.size(); ++b)
        for (size_t j = 0; j < s.rows; ++j) {
            std::memcpy(mean + b * per + j * s.len, &mu[b * S + s.off + j * s.stride], s.len * sizeof(double));
            std::memcpy(err + b * per + j * s.len, &er[b * S + s.off + j * s.stride], s.len * sizeof(double));
        }
}
void DetHubbard::seriesReadBins(int which, int first, int count, double* out, int b) {
    const SeriesSlice s = seriesSlice(which);
    if (count < 1) throw ParameterWrong("dethubbard_series_read_bins: count must be at least 1");
    size_t S = 0;
    check(dqmc_series_info(ctx_, nullptr, nullptr, &S), "dqmc_series_info");
    check(dqmc_select_chain(ctx_, b), "dqmc_select_chain");
    std::vector<double> buf((size_t)count * S);
    check(dqmc_series_read_bins_host(ctx_, first, count, buf.data()), "dqmc_series_read_bins_host");
    const size_t per = s.rows * s.len;
    for (size_t i = 0; i < (size_t)count; ++i)
        for (size_t j = 0; j < s.rows; ++j) std::memcpy(out + i * per + j * s.len, &buf[i * S + s.off + j * s.stride], s.len * sizeof(double));
}
void DetHubbard::seriesDerivedAll(int qx, int qy, double* value, double* err) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    if (!(seriesParts_ & DQMC_SERIES_HUB_EQ)) throw ParameterWrong("the derived quantities need the equal-time part: the handle needs DETHUBBARD_MEASURE_EQ");
    check(dqmc_series_hubbard_derived_host(ctx_, qx, qy, value, err), "dqmc_series_hubbard_derived_host");
}
void DetHubbard::seriesConfigure(int flags) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    check(dqmc_series_configure(ctx_, flags), "dqmc_series_configure");
}
void DetHubbard::seriesRebin() {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    check(dqmc_series_rebin(ctx_), "dqmc_series_rebin");
}
void DetHubbard::seriesGetState(dqmc_series_state& out) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open");
    check(dqmc_series_get_state(ctx_, &out), "dqmc_series_get_state");
}
void DetHubbard::seriesBinningAll(int which, int levels, double* err, double* tau) {
    const SeriesSlice s = seriesSlice(which);
    if (levels < 1 || levels > 12) throw ParameterWrong("dethubbard_series_binning: levels must be in 1..12");
    size_t S = 0;
    check(dqmc_series_info(ctx_, nullptr, nullptr, &S), "dqmc_series_info");
    const size_t nb = ch_.size(), per = s.rows * s.len;
    std::vector<double> e((size_t)levels * nb * S), t(tau ? e.size() : 0);
    check(dqmc_series_binning_host(ctx_, levels, e.data(), tau ? t.data() : nullptr), "dqmc_series_binning_host");
    for (size_t b = 0; b < nb; ++b)
        for (size_t l = 0; l < (size_t)levels; ++l)
            for (size_t j = 0; j < s.rows; ++j) {
                const size_t at = (l * nb + b) * S + s.off + j * s.stride, to = (b * levels + l) * per + j * s.len;
                std::memcpy(err + to, &e[at], s.len * sizeof(double));
                if (tau) std::memcpy(tau + to, &t[at], s.len * sizeof(double));
            }
}
void DetHubbard::seriesBinning(int which, int levels, double* err, double* tau, int b) {
    const SeriesSlice s = seriesSlice(which);
    if (levels < 1 || levels > 12) throw ParameterWrong("dethubbard_series_binning: levels must be in 1..12");
    const size_t len = (size_t)levels * s.rows * s.len, nb = ch_.size();
    std::vector<double> e(nb * len), t(tau ? nb * len : 0);
    seriesBinningAll(which, levels, e.data(), tau ? t.data() : nullptr);
    std::memcpy(err, &e[(size_t)b * len], len * sizeof(double));
    if (tau) std::memcpy(tau, &t[(size_t)b * len], len * sizeof(double));
}

// ---- checkpoint / resume ----
namespace {
const char kHubMagic[8] = {'D', 'Q', 'M', 'C', 'H', 'U', 'B', '1'};
struct HubFile { std::FILE* f; ~HubFile() { if (f) std::fclose(f); } };
void hwr(std::FILE* f, const void* p, size_t n) { if (std::fwrite(p, 1, n, f) != n) throw GeneralError(DQMC_EINVAL, "checkpoint: write error"); }
void hrd(std::FILE* f, void* p, size_t n) { if (std::fread(p, 1, n, f) != n) throw GeneralError(DQMC_EINVAL, "checkpoint: truncated file"); }
}  // namespace

void DetHubbard::saveState(const std::string& path) {
    HubFile hf{std::fopen(path.c_str(), "wb")};
    if (!hf.f) throw GeneralError(DQMC_EINVAL, "Could not open file " + path + " for writing");
    const int32_t hdr[6] = {(int32_t)ch_.size(), p_.L, m_, s_, performedSweeps_, (int32_t)lastSweepDir_};
    hwr(hf.f, kHubMagic, 8); hwr(hf.f, hdr, sizeof(hdr));
    for (int b = 0; b < (int)ch_.size(); ++b) {
        Chain& c = ch_[b];
        check(dqmc_select_chain(ctx_, b), "dqmc_select_chain");
        check(dqmc_get_fields_host(ctx_, c.aux.data(), nullptr, nullptr), "dqmc_get_fields_host");
        const std::vector<uint64_t> rng = c.rng.serialize();
        const uint64_t nr = rng.size(), na = c.aux.size();
        hwr(hf.f, &nr, 8); hwr(hf.f, rng.data(), nr * 8);
        hwr(hf.f, &na, 8); hwr(hf.f, c.aux.data(), na * 8);
    }
}

void DetHubbard::loadState(const std::string& path) {
    HubFile hf{std::fopen(path.c_str(), "rb")};
    if (!hf.f) throw GeneralError(DQMC_EINVAL, "Could not open file " + path + " for reading");
    char magic[8]; int32_t hdr[6];
    hrd(hf.f, magic, 8); hrd(hf.f, hdr, sizeof(hdr));
    if (std::memcmp(magic, kHubMagic, 8) != 0) throw GeneralError(DQMC_EINVAL, "checkpoint: not a detqmc_amd Hubbard state file");
    if (hdr[0] != (int32_t)ch_.size() || hdr[1] != p_.L || hdr[2] != m_ || hdr[3] != s_)
        throw GeneralError(DQMC_EINVAL, "checkpoint: written for a different replica set-up");
    std::vector<double> all(ch_.size() * (size_t)(m_ + 1) * N_);
    for (size_t b = 0; b < ch_.size(); ++b) {
        Chain& c = ch_[b];
        uint64_t nr = 0, na = 0;
        hrd(hf.f, &nr, 8);
        if (nr < DSFMT19937::state_words() + 3 || nr > (1u << 26)) throw GeneralError(DQMC_EINVAL, "checkpoint: bad RNG record");
        std::vector<uint64_t> rng(nr);
        hrd(hf.f, rng.data(), nr * 8);
        hrd(hf.f, &na, 8);
        if (na != c.aux.size()) throw GeneralError(DQMC_EINVAL, "checkpoint: field size mismatch");
        hrd(hf.f, c.aux.data(), na * 8);
        c.rng.deserialize(rng);
        std::memcpy(&all[b * c.aux.size()], c.aux.data(), na * 8);
    }
    check(dqmc_set_fields_all_host(ctx_, all.data()), "dqmc_set_fields_all_host");
    check(dqmc_udv_setup(ctx_), "setupUdVStorage_and_calculateGreen");       // dethubbard.h:345-350
    performedSweeps_ = hdr[4];
    lastSweepDir_ = Up;
    fineLive_ = false;                                              // the every-slice block is no longer that of the last sweep
}

// ---- the series file, in the format of detsdw_series_save: magic, version, dqmc_series_state, the route [nchains] int32 (the identity:
// this replica has no routing), then per chain the closed bins [bins_closed][S], the open bin [S] and, if the variance is tracked, w [S]
// and m2 [S]
namespace {
const char kSeriesMagic[8] = {'D', 'Q', 'M', 'C', 'S', 'E', 'R', '1'};
const int32_t kSeriesVersion = 1;
size_t seriesExtra(int flags) { return (flags & DQMC_SERIES_TRACK_VARIANCE) ? 3 : 1; }     // blocks [nb][S] of an export behind the closed bins
}  // namespace

void DetHubbard::seriesSave(const std::string& path) {
    dqmc_series_state st;
    seriesGetState(st);
    HubFile hf{std::fopen(path.c_str(), "wb")};
    if (!hf.f) throw GeneralError(DQMC_EINVAL, "Could not open file " + path + " for writing");
    hwr(hf.f, kSeriesMagic, 8); hwr(hf.f, &kSeriesVersion, sizeof(kSeriesVersion)); hwr(hf.f, &st, sizeof(st));
    std::vector<int32_t> route(ch_.size());
    for (size_t b = 0; b < route.size(); ++b) route[b] = (int32_t)b;
    hwr(hf.f, route.data(), route.size() * sizeof(int32_t));
    const size_t S = st.sample_len, B = (size_t)st.bins_closed, extra = seriesExtra(st.flags), n = ch_.size() * S;
    std::vector<double> buf((B + extra) * n), row((B + extra) * S);
    check(dqmc_series_export_host(ctx_, buf.data(), buf.size()), "dqmc_series_export_host");
    for (size_t b = 0; b < ch_.size(); ++b) {                // the export is [block][chain][S]: gather the chain's rows
        for (size_t k = 0; k < B + extra; ++k) std::memcpy(&row[k * S], &buf[k * n + b * S], S * sizeof(double));
        hwr(hf.f, row.data(), row.size() * sizeof(double));
    }
}

void DetHubbard::seriesLoad(const std::string& path) {
    if (!seriesOpen_) throw GeneralError(DQMC_EINVAL, "no measurement series is open: dethubbard_series_begin with the options of the run first");
    HubFile hf{std::fopen(path.c_str(), "rb")};
    if (!hf.f) throw GeneralError(DQMC_EINVAL, "Could not open file " + path + " for reading");
    char magic[8]; int32_t version = 0; dqmc_series_state st;
    hrd(hf.f, magic, 8); hrd(hf.f, &version, sizeof(version)); hrd(hf.f, &st, sizeof(st));
    if (std::memcmp(magic, kSeriesMagic, 8) != 0 || version != kSeriesVersion) throw GeneralError(DQMC_EINVAL, "series file: not a detqmc_amd series file of this version");
    const int nch = (int)ch_.size();
    if (st.nb != nch) throw ParameterWrong("series file: written for a different number of chains");
    // the whole file is read and checked before the kernel context imports
    dqmc_series_state own;
    check(dqmc_series_get_state(ctx_, &own), "dqmc_series_get_state");
    if (st.sample_len != own.sample_len || st.parts != own.parts || st.nfreq != own.nfreq)
        throw ParameterWrong("series file: parts or the sample length differ from the open series");
    if (st.bins_closed < 0 || st.bins_closed >= own.max_bins) throw ParameterWrong("series file: more closed bins than maxBins of the open series holds");
    if (st.bin_size < 1 || st.sweeps_in_open_bin < 0 || st.sweeps_in_open_bin >= st.bin_size || st.samples < 0 || st.rebins < 0)
        throw ParameterWrong("series file: bad counters");
    if ((st.flags & ~(DQMC_SERIES_AUTO_REBIN | DQMC_SERIES_TRACK_VARIANCE)) || ((st.flags & DQMC_SERIES_AUTO_REBIN) && (own.max_bins < 4 || own.max_bins % 2)))
        throw ParameterWrong("series file: its options are not valid for maxBins of the open series");
    std::vector<int32_t> route((size_t)nch);
    hrd(hf.f, route.data(), route.size() * sizeof(int32_t));
    for (int b = 0; b < nch; ++b)
        if (route[(size_t)b] != b) throw ParameterWrong("series file: a routed series (written under replica exchange) does not load into a Hubbard replica");
    const size_t S = st.sample_len, B = (size_t)st.bins_closed, extra = seriesExtra(st.flags), n = (size_t)nch * S;
    std::vector<double> slots((size_t)nch * (B + extra) * S);
    hrd(hf.f, slots.data(), slots.size() * sizeof(double));
    char more;
    if (std::fread(&more, 1, 1, hf.f) != 0) throw GeneralError(DQMC_EINVAL, "series file: longer than its header says");
    std::vector<double> buf((B + extra) * n);
    for (size_t b = 0; b < (size_t)nch; ++b)
        for (size_t k = 0; k < B + extra; ++k) std::memcpy(&buf[k * n + b * S], &slots[(b * (B + extra) + k) * S], S * sizeof(double));
    check(dqmc_series_import_host(ctx_, &st, buf.data(), buf.size()), "dqmc_series_import_host");
}

}  // namespace detqmc

// ---------------------------------------------------------------------------------------------
// C API (include/dethubbard_host.h)
// ---------------------------------------------------------------------------------------------
using detqmc::DetHubbard;
struct dethubbard_replica { DetHubbard* impl; int sel; };
static thread_local std::string g_hub_err;
#define HGUARD(...)                                                                                \
    if (!r) { g_hub_err = "null replica handle"; return DQMC_EINVAL; }                             \
    try { __VA_ARGS__; return DQMC_OK; }                                                           \
    catch (const detqmc::GeneralError& e) { g_hub_err = e.what(); return e.code; }                 \
    catch (const std::exception& e) { g_hub_err = e.what(); return DQMC_EINVAL; }

extern "C" const char* dethubbard_last_error(void) { return g_hub_err.c_str(); }
extern "C" int dethubbard_create(const dethubbard_params* p, int nchains, dethubbard_replica** out) {
    if (!p || !out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    *out = nullptr;
    try { DetHubbard* d = new DetHubbard(*p, nchains); *out = new dethubbard_replica{d, 0}; return DQMC_OK; }
    catch (const detqmc::GeneralError& e) { g_hub_err = e.what(); return e.code; }
    catch (const std::exception& e) { g_hub_err = e.what(); return DQMC_EINVAL; }
}
extern "C" void dethubbard_destroy(dethubbard_replica* r) { if (r) { delete r->impl; delete r; } }
extern "C" int dethubbard_select_chain(dethubbard_replica* r, int chain) {
    if (!r || chain < 0 || chain >= r->impl->numChains()) { g_hub_err = "chain index out of range"; return DQMC_EINVAL; }
    r->sel = chain;
    return DQMC_OK;
}
extern "C" int dethubbard_sweep(dethubbard_replica* r, int tm) { HGUARD(r->impl->sweep(tm != 0)) }
extern "C" int dethubbard_sweep_thermalization(dethubbard_replica* r) { HGUARD(r->impl->sweepThermalization()) }
extern "C" int dethubbard_get_info(dethubbard_replica* r, dethubbard_info* out) { HGUARD(r->impl->getInfo(*out, r->sel)) }
extern "C" int dethubbard_get_auxfield(dethubbard_replica* r, double* out) { HGUARD(r->impl->getAuxfield(out, r->sel)) }
extern "C" int dethubbard_get_green(dethubbard_replica* r, double* gUp, double* gDn) { HGUARD(r->impl->getGreen(gUp, gDn, r->sel)) }
extern "C" int dethubbard_get_observables(dethubbard_replica* r, dethubbard_observables* out) { HGUARD(r->impl->getObservables(*out, r->sel)) }
extern "C" int dethubbard_get_zcorr(dethubbard_replica* r, double* out) { HGUARD(r->impl->getZcorr(out, r->sel)) }
extern "C" int dethubbard_get_eq_correlators(dethubbard_replica* r, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getEqCorrelators(out, r->sel))
}
extern "C" int dethubbard_get_td_correlators(dethubbard_replica* r, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getTdCorrelators(out, r->sel))
}
extern "C" int dethubbard_get_td_fine_correlators(dethubbard_replica* r, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getTdFineCorrelators(out, r->sel))
}
extern "C" int dethubbard_get_matsubara(dethubbard_replica* r, int nfreq, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getMatsubara(nfreq, out, r->sel))
}
extern "C" int dethubbard_get_matsubara_all(dethubbard_replica* r, int nfreq, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getMatsubara(nfreq, out, -1))
}
extern "C" int dethubbard_save_state(dethubbard_replica* r, const char* path) {
    if (!path) { g_hub_err = "null path"; return DQMC_EINVAL; }
    HGUARD(r->impl->saveState(path))
}
extern "C" int dethubbard_load_state(dethubbard_replica* r, const char* path) {
    if (!path) { g_hub_err = "null path"; return DQMC_EINVAL; }
    HGUARD(r->impl->loadState(path))
}
extern "C" int dethubbard_set_green_check(dethubbard_replica* r, int on) { HGUARD(r->impl->setGreenCheck(on != 0)) }
extern "C" int dethubbard_get_green_check(dethubbard_replica* r, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->getGreenCheck(out))
}
extern "C" int dethubbard_reset_green_check(dethubbard_replica* r) { HGUARD(r->impl->resetGreenCheck()) }
extern "C" int dethubbard_series_begin(dethubbard_replica* r, int binSize, int maxBins, int flags) { HGUARD(r->impl->seriesBegin(binSize, maxBins, flags)) }
extern "C" int dethubbard_series_end(dethubbard_replica* r) { HGUARD(r->impl->seriesEnd()) }
extern "C" int dethubbard_series_info(dethubbard_replica* r, int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen) {
    HGUARD(r->impl->seriesInfo(binsClosed, sweepsInOpenBin, sampleLen))
}
extern "C" int dethubbard_series_stats(dethubbard_replica* r, int which, double* mean, double* err) {
    if (!mean || !err) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesStats(which, mean, err, r->sel))
}
extern "C" int dethubbard_series_stats_all(dethubbard_replica* r, int which, double* mean, double* err) {
    if (!mean || !err) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesStatsAll(which, mean, err))
}
extern "C" int dethubbard_series_read_bins(dethubbard_replica* r, int which, int first, int count, double* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesReadBins(which, first, count, out, r->sel))
}
extern "C" int dethubbard_series_derived_all(dethubbard_replica* r, int qx, int qy, double* value, double* err) {
    if (!value || !err) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesDerivedAll(qx, qy, value, err))
}
extern "C" int dethubbard_series_configure(dethubbard_replica* r, int flags) { HGUARD(r->impl->seriesConfigure(flags)) }
extern "C" int dethubbard_series_rebin(dethubbard_replica* r) { HGUARD(r->impl->seriesRebin()) }
extern "C" int dethubbard_series_get_state(dethubbard_replica* r, dqmc_series_state* out) {
    if (!out) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesGetState(*out))
}
extern "C" int dethubbard_series_binning(dethubbard_replica* r, int which, int levels, double* err, double* tau) {
    if (!err) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesBinning(which, levels, err, tau, r->sel))
}
extern "C" int dethubbard_series_binning_all(dethubbard_replica* r, int which, int levels, double* err, double* tau) {
    if (!err) { g_hub_err = "null argument"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesBinningAll(which, levels, err, tau))
}
extern "C" int dethubbard_series_save(dethubbard_replica* r, const char* path) {
    if (!path) { g_hub_err = "null path"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesSave(path))
}
extern "C" int dethubbard_series_load(dethubbard_replica* r, const char* path) {
    if (!path) { g_hub_err = "null path"; return DQMC_EINVAL; }
    HGUARD(r->impl->seriesLoad(path))
}
extern "C" double dethubbard_rng_rand01(dethubbard_replica* r) { return r ? r->impl->rand01(r->sel) : -1.0; }
extern "C" dqmc_ctx* dethubbard_ctx(dethubbard_replica* r) { return r ? r->impl->ctx() : nullptr; }
