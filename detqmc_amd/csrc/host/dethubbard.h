// Host-side Hubbard replica: the build's DetHubbard (reference src/dethubbard.{h,cpp}) -- pure control flow over the
// kernel ABI, like detsdw.h.  nb >= 1 independent replicas advance in lockstep through one kernel context.
#pragma once
#include <string>
#include <vector>
#include "../../../include/dethubbard_host.h"
#include "detsdw.h"             // GeneralError / ParameterWrong, RngStream

namespace detqmc {

class DetHubbard {
public:
    DetHubbard(const dethubbard_params& pars, int nchains);
    ~DetHubbard();
    DetHubbard(const DetHubbard&) = delete;
    DetHubbard& operator=(const DetHubbard&) = delete;

    int numChains() const { return (int)ch_.size(); }
    void sweep(bool takeMeasurements);
    void sweepThermalization() { sweep_skeleton(false); }
    void getInfo(dethubbard_info& out, int b);
    void getAuxfield(double* out, int b);
    void getGreen(double* gUp, double* gDn, int b);
    void getObservables(dethubbard_observables& out, int b) const { out = ch_[b].obs; }
    void getZcorr(double* out, int b) const;
    void getEqCorrelators(double* out, int b) const;       // [8][N], needs DETHUBBARD_MEASURE_EQ
    void getTdCorrelators(double* out, int b) const;       // [n-1][6][N], needs DETHUBBARD_MEASURE_TD
    void getTdFineCorrelators(double* out, int b) const;   // [m+1][8][N], needs DETHUBBARD_MEASURE_TD_FINE
    void getMatsubara(int nfreq, double* out, int b);      // [8][nfreq][N] complex, b < 0: every chain; from the block on the device
    void saveState(const std::string& path);
    void loadState(const std::string& path);
    double rand01(int b) { return ch_[b].rng.rand01(); }
    // wrap-error diagnostics of the kernel context (dqmc_set_green_check); out[nchains][2][n+1][DQMC_GREEN_CHECK_FIELDS]
    void setGreenCheck(bool on) { check(dqmc_set_green_check(ctx_, on ? 1 : 0), "dqmc_set_green_check"); }
    void getGreenCheck(double* out) { check(dqmc_green_check_read_host(ctx_, out), "dqmc_green_check_read_host"); }
    void resetGreenCheck() { check(dqmc_green_check_reset(ctx_), "dqmc_green_check_reset"); }
    dqmc_ctx* ctx() { return ctx_; }
    // measurement series (include/dethubbard_host.h): one dqmc_series on the kernel context with the parts the handle's measureFlags provide
    void seriesBegin(int binSize, int maxBins, int flags);
    void seriesEnd();
    void seriesInfo(int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen);
    void seriesStats(int which, double* mean, double* err, int b);
    void seriesStatsAll(int which, double* mean, double* err);
    void seriesReadBins(int which, int first, int count, double* out, int b);
    void seriesDerivedAll(int qx, int qy, double* value, double* err);
    void seriesConfigure(int flags);
    void seriesRebin();
    void seriesGetState(dqmc_series_state& out);
    void seriesBinning(int which, int levels, double* err, double* tau, int b);
    void seriesBinningAll(int which, int levels, double* err, double* tau);
    void seriesSave(const std::string& path);
    void seriesLoad(const std::string& path);

private:
    enum SweepDirection { Up = +1, Down = -1 };
    struct Chain {
        RngStream rng;
        std::vector<double> aux;               // host mirror of the auxiliary field [m+1][N], +-1.0
        double lastAccRatio = 0.0;
        dethubbard_observables obs{};
        std::vector<double> zcorr;
        std::vector<double> eqCorr, tdCorr, tdFineCorr;    // normalised C(d) of the last measurement sweep (measureFlags)
        Chain(uint32_t seed, uint32_t simindex) : rng(seed, simindex + 1u) {}      // detqmc.h:181
    };
    dethubbard_params p_;
    std::vector<Chain> ch_;
    std::vector<double> window_;
    int N_, m_, s_, n_;
    double alpha_;
    dqmc_ctx* ctx_ = nullptr;
    SweepDirection lastSweepDir_ = Up;
    int performedSweeps_ = 0;
    bool measuring_ = false;
    bool measuringTD_ = false;        // ... with G(tau_j, 0) and its correlators after every interior advance (DETHUBBARD_MEASURE_TD)
    bool measuringFine_ = false;      // ... and the every-slice rows of the boundary's segment and of the ends (DETHUBBARD_MEASURE_TD_FINE)
    bool fineLive_ = false;           // the every-slice block on the device is that of the last sweep, a measurement sweep

    // the open series: its parts (DQMC_SERIES_HUB_*) and the flags of seriesBegin; corrStale_: the last measurement sweep did not copy
    // the correlator blocks (DETHUBBARD_SERIES_NO_HOST_COPY), eqCorr / tdCorr of the chains are not its values
    bool seriesOpen_ = false, corrStale_ = false;
    int seriesParts_ = 0, seriesFlags_ = 0;
    // where observable `which` sits inside a sample: `rows` rows of `len` doubles, row j at off + j * stride
    struct SeriesSlice { size_t off, rows, stride, len; };
    SeriesSlice seriesSlice(int which);
    bool seriesNoHostCopy() const { return seriesOpen_ && (seriesFlags_ & DETHUBBARD_SERIES_NO_HOST_COPY); }

    static void check(int rc, const char* what);
    void sweep_skeleton(bool takeMeasurements);
    void sweepDown();
    void sweepUp();
    void updateInSlice(int k);
    void advance(int dir, int l, int boundary, const char* what);     // boundary: the interior boundary j the advance ends on, 0: none (the closing advance)
    void finishMeasurements(int b);
};

}  // namespace detqmc
