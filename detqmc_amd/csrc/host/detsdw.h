// Host-side replica: the build's equivalent of DetSDW<CB_ASSAAD_BERG, OPDIM> on top of
// DetModelGC<1, cpx> (reference src/detsdwopdim.{h,cpp}, src/detmodel.h).  Pure control flow: every
// numerical step is a call into the kernel ABI (include/dqmc_hip.h).  Method names follow the
// reference so the parity tests read like the reference's own call sites.
#pragma once
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../../include/detsdw_host.h"
#include "dsfmt19937.h"
#include "obs_catalogue.h"

namespace detqmc {

// src/exceptions.h:24-73
struct GeneralError : std::runtime_error {
    int code;
    GeneralError(int code_, const std::string& msg) : std::runtime_error(msg), code(code_) {}
};
struct ParameterWrong : GeneralError {
    explicit ParameterWrong(const std::string& msg) : GeneralError(DQMC_EINVAL, msg) {}
};

// One object drives nb >= 1 replicas ("chains") that share lattice, temperature and couplings and differ in
// RNG stream (rngSeed / simindex), field configuration and the exchange parameter r -- exactly the set of
// replicas of a DetQMCPT run (src/detqmcpt.h).  nb = 1 is the reference's single replica.
// Per-replica methods take the chain index b.
//
// The chains are held in S sub-batches ("groups"), each ONE kernel context (dqmc_create_batch: every launch carries
// all chains of the group, own HIP stream).  A sweep runs the groups concurrently, one host thread per group: the
// groups drift out of phase, so the latency-bound kernels of one (decision kernel, QR panel: one workgroup per chain)
// overlap the streaming / MFMA kernels of the others -- within one process what round 1 needed four worker
// processes for.  Chains are independent Markov chains, so the grouping changes no result (tests).
class DetSDW {
public:
    explicit DetSDW(const detsdw_params& pars) : DetSDW(&pars, 1) {}     // createReplica + ctor
    // sub_batches: 0 = automatic (up to 4 groups of at least 32 chains each), otherwise a divisor of nchains
    DetSDW(const detsdw_params* pars, int nchains, int sub_batches = 0);
    ~DetSDW();
    DetSDW(const DetSDW&) = delete;
    DetSDW& operator=(const DetSDW&) = delete;

    int numChains() const { return (int)ch_.size(); }
    void sweep(bool takeMeasurements);
    void sweepThermalization();

    // replica exchange surface
    double get_exchange_parameter_value(int b = 0) const { return ch_[b].pars.r; }
    void set_exchange_parameter_value(double r, int b = 0);
    const char* get_exchange_parameter_name() const { return "r"; }
    double get_exchange_action_contribution(int b = 0);
    void get_control_data(detsdw_control_data& out, int b = 0);
    void set_control_data(const detsdw_control_data& in, int b = 0);

    void getInfo(detsdw_info& out, int b = 0);
    void getObservables(detsdw_observables& out, int b = 0) const { out = ch_[b].obs; }
    void getObservableVector(int which, double* out, int b = 0) const;
    void getTauGrid(double* out) const;
    void getTauGridFine(double* out) const;        // k dtau, k = 0 .. m (timeDisplacedEverySlice)
    // chi(q, i omega_n) / G(k, i omega_n) of the every-slice observable `which`, n = 0 .. nfreq-1: out[nfreq][N] (re, im) of chain b, or
    // out[nchains][nfreq][N] of every chain in handle order; valid after a measurement sweep and until the next sweep
    void getMatsubara(int which, int nfreq, double* out, int b = 0);
    void getMatsubaraAll(int which, int nfreq, double* out);
    // measurement series (include/detsdw_host.h): one dqmc_series per kernel context, fed by every sweep(true) while it is open
    void seriesBegin(int binSize, int maxBins, int nfreq, int flags);
    void seriesEnd();
    void seriesRoute(const int* slotOfChain);      // permutation over all chains of the handle: the sample of chain c goes to slot slotOfChain[c]
    void seriesGetRoute(int* out) const;
    void seriesInfo(int* binsClosed, int* sweepsInOpenBin, size_t* sampleLen);
    void seriesStats(int which, double* mean, double* err, int b = 0);
    void seriesStatsAll(int which, double* mean, double* err);
    void seriesDerivedAll(int what, double* value, double* err);
    void seriesBandDerived(int at, double* value, double* err);
    void seriesCustomDerived(int c, int qx, int qy, double* value, double* err);
    // user-defined bilinears (include/detsdw_host.h): count Hermitian 4 x 4 matrices for every kernel context, between sweeps
    void setCustomBilinears(int count, const dqmc_cplx* M);
    void setCustomBondBilinears(int count, const dqmc_cplx* M0, const dqmc_cplx* Mx, const dqmc_cplx* My);
    void getCustomBondBilinears(int* count, dqmc_cplx* M0, dqmc_cplx* Mx, dqmc_cplx* My) const;
    // user-defined pair operators (include/detsdw_host.h): count operators (F0, Fx, Fy) for every kernel context, between sweeps
    void setCustomPairOperators(int count, const dqmc_cplx* F0, const dqmc_cplx* Fx, const dqmc_cplx* Fy);
    void getCustomPairOperators(int* count, dqmc_cplx* F0, dqmc_cplx* Fx, dqmc_cplx* Fy) const;
    void seriesCustomPairDerived(int c, int qx, int qy, double* value, double* err);
    // the averaged Green's function block of every kernel context, and the bubble / vertex of pair operator c from the series
    void setGreenMatrix(bool on);
    // wrap-error diagnostics of every kernel context (include/detsdw_host.h); out[nchains][2][n+1][DQMC_GREEN_CHECK_FIELDS], handle order
    void setGreenCheck(bool on);
    void getGreenCheck(double* out);
    void resetGreenCheck();
    void seriesPairVertex(int c, int qx, int qy, double* value, double* err);
    void seriesPhVertex(int c, int qx, int qy, double* value, double* err);      // ... of user-defined bilinear c
    void seriesReadBins(int which, int first, int count, double* out, int b = 0);
    // long runs: options, re-binning, binning analysis (err, tau [levels] x the slice of seriesStats; tau may be null), series file
    void seriesConfigure(int flags);
    void seriesRebin();
    void seriesGetState(dqmc_series_state& out);   // the state every kernel context shares, nb = all chains of the handle
    void seriesBinning(int which, int levels, double* err, double* tau, int b = 0);
    void seriesBinningAll(int which, int levels, double* err, double* tau);
    void seriesSave(const std::string& path);
    void seriesLoad(const std::string& path);
    void getPhi(double* phi, int b = 0);
    void setPhi(const double* phi, int b = 0);
    void getCdwl(int32_t* cdwl, int b = 0);
    void setCdwl(const int32_t* cdwl, int b = 0);
    void getGreen(dqmc_cplx* g, int b = 0);
    void getGreenInvSv(double* sv, int b = 0);
    void saveConfigurationStreamBinary(const std::string& directory, int b = 0);
    void saveState(const std::string& path);
    void loadState(const std::string& path);
    double rand01(int b = 0) { return ch_[b].rng.rand01(); }
    int numSubBatches() const { return (int)groups_.size(); }
    // kernel context that holds chain b and b's index inside it
    dqmc_ctx* ctx(int b = 0, int* local = nullptr) { if (local) *local = b - grp(b).first; return grp(b).ctx; }

private:
    enum SweepDirection { Up = +1, Down = -1 };
    // Storage of the observable vectors, addressed by what the catalogue returns for an index (obs_catalogue.h, DetSDW::stored)
    struct TdComp { std::vector<double> val, q0, scalar; };     // one component of a time-displaced channel: rows x N (channel 7: rows x N x 4 x 4
                                                                // complex), its row sums, and the channel's per-row scalar of that number
    struct TdObs { std::vector<TdComp> ch[kTdChannels]; };      // one row per tau of the family's grid
    struct EqComp { std::vector<double> corr, sq; };            // one component of an equal-time block: C(d) and S(q), N each
    struct Chain {
        detsdw_params pars;
        RngStream rng;
        std::vector<double> phi;               // host mirror, valid after syncPhiFromDevice(b)
        std::vector<int32_t> cdwl;             // discrete field l_i(tau_k), [k * N + site]; lives on the device when cdwU != 0 (getCdwl)
        int acceptedGlobalShifts = 0, attemptedGlobalShifts = 0;          // UpdateStatistics (detsdwopdim.h:285-311)
        int acceptedWolffClusterUpdates = 0, attemptedWolffClusterUpdates = 0;
        int acceptedWolffClusterShiftUpdates = 0, attemptedWolffClusterShiftUpdates = 0;
        double addedWolffClusterSize = 0.0;
        double phiDelta = 0.5, lastAccRatio = 0.0;
        double angleDelta = 0.0, scaleDelta = 0.1;          // AdjustmentData::InitialAngleDelta / InitialScaleDelta (detsdwopdim.h:490-491)
        detsdw_observables obs{};
        std::vector<double> slice[4];          // kOccX, kOccY, pairPlus, pairMinus
        std::vector<EqComp> eq[kEqBlocks];
        TdObs td, tdFine;                      // rows = interior boundaries j = 1 .. n-1 / time slices k = 0 .. m (timeDisplacedEverySlice)
        Chain(const detsdw_params& p) : pars(p), rng(p.rngSeed, (uint32_t)p.simindex + 1u) {   // detqmc.h:181
            for (const ObsRow& r : kObsRows) {             // every component the catalogue can name exists, empty until it is measured
                if (r.family == DETSDW_OBS_FAMILY_TD) { td.ch[r.block].resize(r.n); tdFine.ch[r.block].resize(r.n); }
                if (r.family == DETSDW_OBS_FAMILY_EQ) eq[r.block].resize(r.n);
            }
        }
    };
    std::vector<Chain> ch_;
    struct Group {                                 // one sub-batch = one kernel context, chains [first, first + count)
        dqmc_ctx* ctx = nullptr;
        int first = 0, count = 0;
        std::vector<double> window;                // uniforms of the coming sweep, all chains of the group (full push without look-ahead)
        std::vector<uint64_t> windowStart;         // per chain: rng.drawn() at which the window on the device begins
        bool tailStaged = false;                   // the draws behind those windows are on the device or on their way (stageLocalUpdates)
        std::vector<double> fields;                // host staging of all chains' fields (global moves)
        std::vector<double> mats[kTdChannels];     // Matsubara transforms of the group's chains per channel, [chain][component][nfreq][N] (re, im)
        int matsNfreq[kTdChannels] = {};           // ... and the nfreq they hold (0: none); cleared by every sweep
        std::vector<double> seriesMean, seriesErr; // dqmc_series_stats_host of the group's chains, [chain][S] each ...
        int seriesStatsBins = 0;                   // ... and the number of closed bins they were formed from (0: none)
        std::vector<double> seriesBinErr, seriesBinTau;   // dqmc_series_binning_host of the group's chains, [level][chain][S] each ...
        int seriesBinLevels = 0;                          // ... the levels they hold (0: none), whether tau was formed, and the samples
        bool seriesBinHasTau = false;                     // and rebins of the series they were formed from
        long long seriesBinSamples = 0, seriesBinRebins = 0;
    };
    std::vector<Group> groups_;
    int N_, MSF_, ng_, m_, s_, n_, opdim_;
    SweepDirection lastSweepDir_ = Up;
    int performedSweeps_ = 0;
    std::vector<dqmc_cplx> customM_;               // the matrices of setCustomBilinears, [count][4][4] (every kernel context holds the same)
    int customCount() const { return (int)customM_.size() / 16; }
    std::vector<dqmc_cplx> customMx_, customMy_;   // the bond parts of setCustomBondBilinears, [count][4][4] each; empty while none is non-zero
    bool customBond() const { return !customMx_.empty(); }
    void setCustomOperators(int count, const dqmc_cplx* M, const dqmc_cplx* Mx, const dqmc_cplx* My, bool bond);
    std::vector<dqmc_cplx> pairF_[3];              // F0, Fx, Fy of setCustomPairOperators, [DQMC_CUSTOM_MAX][4][4] each, zero padded
    int pairCount_ = 0;
    bool greenMatrix_ = false;                     // setGreenMatrix: every kernel context fills its averaged Green's function block
    bool greenCheck_ = false;                      // setGreenCheck: the sweeps take the plain path at segment ends, so that every advance finds a wrapped G
    int pairCount() const { return pairCount_; }
    bool customPairTd() const;                     // pair operators are set and the handle measures time-displaced
    bool customPairEq() const;                     // ... the equal-time correlators
    bool customTd() const;                         // matrices are set and the handle measures the particle-hole family
    bool customEq() const;                         // ... the equal-time correlators
    bool has(ObsNeeds needs) const;                // the option predicate of a catalogue row
    int live(const ObsRow& r) const { return r.count == ObsCount::Custom ? customCount() : r.count == ObsCount::Pair ? pairCount() : r.n; }
    const std::vector<double>& stored(const Chain& c, const ObsRow& r, int comp, bool fine) const;
    void dropStored(int tdChannel, int eqBlock);   // after the operators of a channel changed: its vectors are empty until the next measurement sweep

    Group& grp(int b) { return groups_[(size_t)b / (size_t)groups_[0].count]; }
    static void check(int rc, const char* what);
    dqmc_ctx* select(int b);                       // selects chain b in its context and returns that context
    static void normalise(detsdw_params& p, int& bcv);
    void setupRandomField(Chain& c);
    void setupUdVStorage_and_calculateGreen(Group& g);
    void forEachGroup(const std::function<void(Group&)>& fn);      // concurrently, one host thread per group
    void sweep_skeleton(Group& g, bool thermalization);
    void measureBosonic(Chain& c, bool descending);
    void finishFermionic(int b);
    bool measuring_ = false;          // measure(k) after the updates of slice k (updateInSliceAndMaybeMeasure)
    bool measuringTD_ = false;        // ... and G(tau_j, 0) after every interior advance (timeDisplacedMeasurements)
    bool tdBlocksValid_ = false;      // the device's time-displaced blocks are those of the last sweep, a measurement sweep
    struct { bool open = false; int binSize = 0, maxBins = 0, nfreq = 0, parts = 0, flags = 0; } series_;
    std::vector<int> seriesRoute_;    // slotOfChain, the identity unless detsdw_series_route has set another
    bool seriesNoHostCopy() const { return series_.open && (series_.flags & DETSDW_SERIES_NO_HOST_COPY); }
    void seriesSlice(int which, int& part, size_t& offset, size_t& length);   // where `which` sits inside its part
    void seriesStatsOf(Group& g);                                             // fills the group's cache
    void seriesBinningOf(Group& g, int levels, bool withTau);                 // the same for the binning analysis
    static void seriesDropCaches(Group& g) { g.seriesStatsBins = 0; g.seriesBinLevels = 0; }   // after a re-bin or a load: the keys repeat
    void invalidateMatsubara();
    const double* matsubara(Group& g, int which, int nfreq, int& ncomp, int& comp);
    void measureTimeDisplaced(Group& g, int j);
    void measureTimeDisplacedEnds(Group& g);
    void sweepDown(Group& g, bool thermalization);
    void sweepUp(Group& g, bool thermalization);
    // segmentEnd: the advance that follows rebuilds G (last slice of a segment).  Returns true when it took the wrap of a down sweep along
    bool updateInSlice(Group& g, int k, bool thermalization, bool segmentEnd = false, bool down = false);
    int uniformsPerSite() const;
public:
    void exchangeActionsDevice(double* out_dev);        // out_dev[chain], device memory
private:
    void beginLocalUpdates(Group& g);
    void stageLocalUpdates(Group& g);              // look-ahead: draws and uploads the next window's tail while the device sweeps
    bool lookahead_ = true;                        // detsdw_params::tuning without DQMC_TUNING_NO_RNG_LOOKAHEAD
    void endLocalUpdates(Group& g);
    void globalMove(Group& g);
    enum GlobalMoveKind { MoveShift, MoveWolff, MoveWolffShift };
    void attemptGlobalMove(Group& g, GlobalMoveKind kind);
    unsigned buildAndFlipCluster(Chain& c);
    void addGlobalRandomDisplacement(Chain& c);
    double phiAction(const Chain& c) const;
    void syncPhiFromDevice(int b);
    size_t phiIdx(int site, int dim, int k) const { return (size_t)site + (size_t)N_ * (dim + (size_t)opdim_ * k); }
};

}  // namespace detqmc
