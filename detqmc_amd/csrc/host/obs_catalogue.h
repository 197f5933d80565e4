// The observable catalogue of the SDW host replica: one row per contiguous range of DETSDW_OBS_* indices (include/detsdw_host.h).
// A row answers what every reader asks of an index -- where the values live (family, block, component, kind), whether the index has a
// DETSDW_OBS_FINE twin and a Matsubara transform, which option it needs and what is said without it, and which part of a measurement
// series holds it.  getObservableVector, matsubara, seriesSlice, seriesBegin and finishFermionic (detsdw.cpp) read it, and so does
// detsdw_describe_observable.  A new observable is a new row here, its DETSDW_OBS_* number, and its name in detqmc_amd/model.py.
// Plain C++: no HIP, no handle.
#pragma once
#include "../../../include/detsdw_host.h"

namespace detqmc {

// the time-displaced channels of dqmc_measure_td_fine_read_host and the equal-time blocks, as the storage is indexed
enum { kTdGreenK = 0, kTdPair = 1, kTdPh = 2, kTdCurrent = 3, kTdBand = 4, kTdCustom = 5, kTdCustomPair = 6, kTdGreenMatrix = 7, kTdChannels = 8 };
enum { kEqFixed = 0, kEqBand = 1, kEqCustom = 2, kEqCustomPair = 3, kEqBlocks = 4 };

// the option predicate a row needs (DetSDW::has)
enum class ObsNeeds { Nothing, TdLevel, TdLevel2, PhLevel, PhLevel2, TdBand, EqCorrelators, EqBand, CustomTd, CustomEq, CustomPairTd, CustomPairEq, GreenMatrix };
// how many of a row's components exist: all of them, customCount() or pairCount() (DetSDW::live)
enum class ObsCount { Fixed, Custom, Pair };

struct ObsRow {
    int first, n;            // the indices [first, first + n); component = index - first
    int family, block, kind; // DETSDW_OBS_FAMILY_*, channel (time-displaced) or block (equal-time), DETSDW_OBS_KIND_*
    ObsCount count;
    bool fineTwin, matsubara;
    ObsNeeds needs;
    const char* needsMsg;    // what getObservableVector says without `needs` ...
    const char* matsMsg;     // ... and what matsubara says
    const char* staleMsg;    // what getObservableVector says while the storage is empty (null: nothing, the vector is copied as it is)
    int seriesBit;           // DQMC_SERIES_* of the series part that holds the observable (0: none); the part index is the bit's position
};

namespace obs_text {
constexpr const char* kGreenK = "greenKTauX / greenKTauY need timeDisplacedMeasurements";
constexpr const char* kPair = "pairPlusTau / pairMinusTau need timeDisplacedMeasurements = 2";
constexpr const char* kPh = "chargeTau / spinZTau / sdwTau need timeDisplacedParticleHole";
constexpr const char* kCurrent = "currentXTau / currentYTau / bondKineticX / bondKineticY need timeDisplacedParticleHole = 2";
constexpr const char* kCurrentMats = "currentXTau / currentYTau need timeDisplacedParticleHole = 2";
constexpr const char* kEq = "the equal-time correlators and structure factors need equalTimeCorrelators (DETSDW_FM_EQ_CORRELATORS)";
constexpr const char* kBandTd = "bandDiffTau / bandMixTau need bandCorrelators with timeDisplacedParticleHole (DETSDW_TD_PH_BAND)";
constexpr const char* kBandEq = "bandDiffCorr / bandMixCorr / bandDiffSq / bandMixSq need bandCorrelators with equalTimeCorrelators (DETSDW_FM_EQ_BAND)";
constexpr const char* kCustomTd = "custom{c}Tau needs timeDisplacedParticleHole";
constexpr const char* kCustomTdMats = "custom{c}Tau needs a matrix set by detsdw_set_custom_bilinears and timeDisplacedParticleHole";
constexpr const char* kCustomEq = "custom{c}Corr / custom{c}Sq need equalTimeCorrelators";
constexpr const char* kCustomStale = "no measurement sweep has run since the user-defined bilinears were set";
constexpr const char* kPairTd = "customPair{c}Tau needs timeDisplacedMeasurements";
constexpr const char* kPairTdMats = "customPair{c}Tau needs an operator set by detsdw_set_custom_pair_operators and timeDisplacedMeasurements";
constexpr const char* kPairEq = "customPair{c}Corr / customPair{c}Sq need equalTimeCorrelators";
constexpr const char* kPairStale = "no measurement sweep has run since the user-defined pair operators were set";
constexpr const char* kGreenMatrix = "greenMatrixTau needs detsdw_set_green_matrix";
constexpr const char* kGreenMatrixStale = "no measurement sweep has run since the averaged Green's function was switched on";
}  // namespace obs_text

// in the order of the indices; the time-displaced channels and the equal-time blocks appear in ascending order, which is the order
// finishFermionic reads them in
static const ObsRow kObsRows[] = {
    // first, n, family, block, kind, count, fine twin, Matsubara, needs, texts (vector, Matsubara, stale), series bit
    {DETSDW_OBS_KOCCX, 4, DETSDW_OBS_FAMILY_SLICE, 0, DETSDW_OBS_KIND_SITE, ObsCount::Fixed, false, false, ObsNeeds::Nothing, nullptr, nullptr, nullptr, 0},
    {DETSDW_OBS_GREENKTAU_X, 2, DETSDW_OBS_FAMILY_TD, kTdGreenK, DETSDW_OBS_KIND_TAU, ObsCount::Fixed, true, true, ObsNeeds::TdLevel, obs_text::kGreenK, obs_text::kGreenK, nullptr, DQMC_SERIES_MATS_G},
    {DETSDW_OBS_PAIRPLUSTAU, 2, DETSDW_OBS_FAMILY_TD, kTdPair, DETSDW_OBS_KIND_TAU, ObsCount::Fixed, true, true, ObsNeeds::TdLevel2, obs_text::kPair, obs_text::kPair, nullptr, DQMC_SERIES_MATS_PAIR},
    {DETSDW_OBS_PAIRPLUSTAU_Q0, 2, DETSDW_OBS_FAMILY_TD, kTdPair, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Fixed, true, false, ObsNeeds::TdLevel2, obs_text::kPair, nullptr, nullptr, 0},
    {DETSDW_OBS_CHARGETAU, 3, DETSDW_OBS_FAMILY_TD, kTdPh, DETSDW_OBS_KIND_TAU, ObsCount::Fixed, true, true, ObsNeeds::PhLevel, obs_text::kPh, obs_text::kPh, nullptr, DQMC_SERIES_MATS_PH},
    {DETSDW_OBS_CHARGETAU_Q0, 3, DETSDW_OBS_FAMILY_TD, kTdPh, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Fixed, true, false, ObsNeeds::PhLevel, obs_text::kPh, nullptr, nullptr, 0},
    {DETSDW_OBS_CURRENTXTAU, 2, DETSDW_OBS_FAMILY_TD, kTdCurrent, DETSDW_OBS_KIND_TAU, ObsCount::Fixed, true, true, ObsNeeds::PhLevel2, obs_text::kCurrent, obs_text::kCurrentMats, nullptr, DQMC_SERIES_MATS_CURRENT},
    {DETSDW_OBS_CURRENTXTAU_Q0, 2, DETSDW_OBS_FAMILY_TD, kTdCurrent, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Fixed, true, false, ObsNeeds::PhLevel2, obs_text::kCurrent, nullptr, nullptr, 0},
    {DETSDW_OBS_BONDKINETICX, 2, DETSDW_OBS_FAMILY_TD, kTdCurrent, DETSDW_OBS_KIND_ROW_SCALAR, ObsCount::Fixed, true, false, ObsNeeds::PhLevel2, obs_text::kCurrent, nullptr, nullptr, 0},
    {DETSDW_OBS_CHARGECORR, 5, DETSDW_OBS_FAMILY_EQ, kEqFixed, DETSDW_OBS_KIND_CORR, ObsCount::Fixed, false, false, ObsNeeds::EqCorrelators, obs_text::kEq, nullptr, nullptr, DQMC_SERIES_EQ},
    {DETSDW_OBS_CHARGESQ, 5, DETSDW_OBS_FAMILY_EQ, kEqFixed, DETSDW_OBS_KIND_SQ, ObsCount::Fixed, false, false, ObsNeeds::EqCorrelators, obs_text::kEq, nullptr, nullptr, DQMC_SERIES_EQ},
    {DETSDW_OBS_PHICHI, 1, DETSDW_OBS_FAMILY_PHI, 0, DETSDW_OBS_KIND_PHI_CHI, ObsCount::Fixed, false, false, ObsNeeds::Nothing, nullptr, nullptr, nullptr, DQMC_SERIES_PHI},
    {DETSDW_OBS_PHISCALARS, 1, DETSDW_OBS_FAMILY_PHI, 0, DETSDW_OBS_KIND_PHI_SCALARS, ObsCount::Fixed, false, false, ObsNeeds::Nothing, nullptr, nullptr, nullptr, DQMC_SERIES_PHI},
    {DETSDW_OBS_BANDDIFFTAU, 2, DETSDW_OBS_FAMILY_TD, kTdBand, DETSDW_OBS_KIND_TAU, ObsCount::Fixed, true, true, ObsNeeds::TdBand, obs_text::kBandTd, obs_text::kBandTd, nullptr, DQMC_SERIES_MATS_BAND},
    {DETSDW_OBS_BANDDIFFTAU_Q0, 2, DETSDW_OBS_FAMILY_TD, kTdBand, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Fixed, true, false, ObsNeeds::TdBand, obs_text::kBandTd, nullptr, nullptr, 0},
    {DETSDW_OBS_BANDDIFFCORR, 2, DETSDW_OBS_FAMILY_EQ, kEqBand, DETSDW_OBS_KIND_CORR, ObsCount::Fixed, false, false, ObsNeeds::EqBand, obs_text::kBandEq, nullptr, nullptr, DQMC_SERIES_EQ_BAND},
    {DETSDW_OBS_BANDDIFFSQ, 2, DETSDW_OBS_FAMILY_EQ, kEqBand, DETSDW_OBS_KIND_SQ, ObsCount::Fixed, false, false, ObsNeeds::EqBand, obs_text::kBandEq, nullptr, nullptr, DQMC_SERIES_EQ_BAND},
    {DETSDW_OBS_CUSTOMTAU, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_TD, kTdCustom, DETSDW_OBS_KIND_TAU, ObsCount::Custom, true, true, ObsNeeds::CustomTd, obs_text::kCustomTd, obs_text::kCustomTdMats, obs_text::kCustomStale, DQMC_SERIES_MATS_CUSTOM},
    {DETSDW_OBS_CUSTOMTAU_Q0, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_TD, kTdCustom, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Custom, true, false, ObsNeeds::CustomTd, obs_text::kCustomTd, nullptr, obs_text::kCustomStale, 0},
    {DETSDW_OBS_CUSTOMCORR, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_EQ, kEqCustom, DETSDW_OBS_KIND_CORR, ObsCount::Custom, false, false, ObsNeeds::CustomEq, obs_text::kCustomEq, nullptr, obs_text::kCustomStale, DQMC_SERIES_EQ_CUSTOM},
    {DETSDW_OBS_CUSTOMSQ, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_EQ, kEqCustom, DETSDW_OBS_KIND_SQ, ObsCount::Custom, false, false, ObsNeeds::CustomEq, obs_text::kCustomEq, nullptr, obs_text::kCustomStale, DQMC_SERIES_EQ_CUSTOM},
    {DETSDW_OBS_CUSTOMPAIRTAU, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_TD, kTdCustomPair, DETSDW_OBS_KIND_TAU, ObsCount::Pair, true, true, ObsNeeds::CustomPairTd, obs_text::kPairTd, obs_text::kPairTdMats, obs_text::kPairStale, DQMC_SERIES_MATS_CUSTOM_PAIR},
    {DETSDW_OBS_CUSTOMPAIRTAU_Q0, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_TD, kTdCustomPair, DETSDW_OBS_KIND_TAU_Q0, ObsCount::Pair, true, false, ObsNeeds::CustomPairTd, obs_text::kPairTd, nullptr, obs_text::kPairStale, 0},
    {DETSDW_OBS_CUSTOMPAIRCORR, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_EQ, kEqCustomPair, DETSDW_OBS_KIND_CORR, ObsCount::Pair, false, false, ObsNeeds::CustomPairEq, obs_text::kPairEq, nullptr, obs_text::kPairStale, DQMC_SERIES_EQ_CUSTOM_PAIR},
    {DETSDW_OBS_CUSTOMPAIRSQ, DQMC_CUSTOM_MAX, DETSDW_OBS_FAMILY_EQ, kEqCustomPair, DETSDW_OBS_KIND_SQ, ObsCount::Pair, false, false, ObsNeeds::CustomPairEq, obs_text::kPairEq, nullptr, obs_text::kPairStale, DQMC_SERIES_EQ_CUSTOM_PAIR},
    {DETSDW_OBS_GREENMATRIXTAU, 1, DETSDW_OBS_FAMILY_TD, kTdGreenMatrix, DETSDW_OBS_KIND_GREEN_MATRIX, ObsCount::Fixed, true, false, ObsNeeds::GreenMatrix, obs_text::kGreenMatrix, nullptr, obs_text::kGreenMatrixStale, DQMC_SERIES_GREEN_MATRIX},
};

// an index of a custom / custom-pair row beyond the count that is set
inline const char* obs_not_set_text(ObsCount c) {
    return c == ObsCount::Pair ? "no user-defined pair operator with this index is set (detsdw_set_custom_pair_operators)"
                               : "no user-defined bilinear with this index is set (detsdw_set_custom_bilinears)";
}

// what seriesSlice says of a part the open series does not hold (or of a custom index beyond the count), by the part's bit
inline const char* obs_series_missing_text(int bit) {
    switch (bit) {
    case DQMC_SERIES_EQ: return "the equal-time part of the series needs equalTimeCorrelators";
    case DQMC_SERIES_EQ_BAND: return "the equal-time band part of the series needs bandCorrelators with equalTimeCorrelators";
    case DQMC_SERIES_EQ_CUSTOM: return "the series holds no equal-time part of this user-defined bilinear";
    case DQMC_SERIES_MATS_CUSTOM: return "the series holds no Matsubara part of this user-defined bilinear";
    case DQMC_SERIES_EQ_CUSTOM_PAIR: return "the series holds no equal-time part of this user-defined pair operator";
    case DQMC_SERIES_MATS_CUSTOM_PAIR: return "the series holds no Matsubara part of this user-defined pair operator";
    case DQMC_SERIES_GREEN_MATRIX: return "the series holds no averaged Green's function: detsdw_set_green_matrix before the series began, and timeDisplacedEverySlice";
    case DQMC_SERIES_PHI: return "the series has no order-parameter part: detsdw_series_begin with DETSDW_SERIES_PHI";
    default: return "the series has no Matsubara part for this observable: the option it needs, or timeDisplacedEverySlice, is off";
    }
}
// part index of dqmc_series_layout: the position of the part's bit (include/dqmc_hip.h)
inline int obs_series_part(int bit) {
    int part = 0;
    while (bit > 1) { bit >>= 1; ++part; }
    return part;
}

// the trailing per-row scalars of a time-displaced channel's block: the components of its ROW_SCALAR row (2 for the current channel)
inline int obs_row_scalars(int channel) {
    for (const ObsRow& r : kObsRows)
        if (r.family == DETSDW_OBS_FAMILY_TD && r.block == channel && r.kind == DETSDW_OBS_KIND_ROW_SCALAR) return r.n;
    return 0;
}

// index -> (row, component, fine); row is null for an unknown index and for the DETSDW_OBS_FINE bit on an index without a twin
struct ObsRef { const ObsRow* row; int comp; bool fine; };
inline ObsRef obs_lookup(int which) {
    const bool fine = (which & DETSDW_OBS_FINE) != 0;
    const int w = which & ~DETSDW_OBS_FINE;
    for (const ObsRow& r : kObsRows)
        if (w >= r.first && w < r.first + r.n) return {fine && !r.fineTwin ? nullptr : &r, w - r.first, fine};
    return {nullptr, 0, fine};
}

}  // namespace detqmc
