"""ctypes binding of the in-tree shared library (include/dqmc_hip.h + include/detsdw_host.h).

There is NO fallback: if libdetqmc_amd.so is missing or cannot be loaded this module raises, and
every compute entry point needs a GPU (dqmc_create returns DQMC_ENODEV without one).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libdetqmc_amd.so")


class DqmcError(RuntimeError):
    """Error code from the C ABI, carrying the library's message (reference: GeneralError)."""

    def __init__(self, code, msg):
        super().__init__(f"[dqmc {code}] {msg}")
        self.code = code


DQMC_TD_EVERY_SLICE = 0x100     # flag bit of dqmc_params.timedisplaced
DQMC_TD_HUB_EVERY_SLICE = 0x400  # flag bit of dqmc_params.timedisplaced, Hubbard model: the every-slice reservation
DETSDW_TD_EVERY_SLICE = 0x100   # flag bit of detsdw_params.timeDisplacedMeasurements
DETSDW_TD_FINE_ON_DEVICE = 0x200  # flag bit of detsdw_params.timeDisplacedMeasurements: the fine blocks stay on the device
DETSDW_OBS_FINE = 0x100         # flag bit of the observable index: the every-slice twin
DQMC_SERIES_AUTO_REBIN, DQMC_SERIES_TRACK_VARIANCE = 1, 2   # flags of dqmc_series_configure / detsdw_series_configure
DETSDW_SERIES_NO_HOST_COPY = 1    # flag of detsdw_series_begin: no equal-time block copy per measurement sweep while the series is open
DETSDW_SERIES_PHI = 2             # flag of detsdw_series_begin: the order-parameter part (chi_phi(q, i omega_n) and its scalars)
DETSDW_FM_EQ_CORRELATORS = 0x100  # flag bit of detsdw_params.fermionMeasurements: equal-time charge / spin / SDW / pairing correlators
DQMC_TD_PH_BAND = 0x100           # flag bit of dqmc_params.td_particle_hole: the band-resolved charge channels bandDiff / bandMix
DETSDW_TD_PH_BAND = 0x100         # flag bit of detsdw_params.timeDisplacedParticleHole: the same at the host level
DETSDW_FM_EQ_BAND = 0x200         # flag bit of detsdw_params.fermionMeasurements: equal-time bandDiff / bandMix correlators
DQMC_SERIES_MATS_BAND, DQMC_SERIES_EQ_BAND = 128, 256   # parts of dqmc_series_begin: Matsubara transform of channel 4, equal-time band block
DQMC_SERIES_MATS_CUSTOM, DQMC_SERIES_EQ_CUSTOM = 512, 1024   # ... Matsubara transform of channel 5, equal-time block of the custom bilinears
DQMC_SERIES_MATS_CUSTOM_PAIR, DQMC_SERIES_EQ_CUSTOM_PAIR = 2048, 4096   # ... Matsubara transform of channel 6, equal-time block of the custom pair operators
DQMC_SERIES_GREEN_MATRIX = 8192    # ... the normalised averaged Green's function of every slice (dqmc_set_green_matrix)
DQMC_SERIES_HUB_SCALARS, DQMC_SERIES_HUB_EQ, DQMC_SERIES_HUB_TD = 16384, 32768, 65536   # the parts of a Hubbard context (parts 14 .. 16)
DQMC_CUSTOM_MAX = 4               # matrices of dqmc_set_custom_bilinears at most
# detsdw_observable_desc: family and kind of an observable index (detsdw_describe_observable)
DETSDW_OBS_FAMILY_SLICE, DETSDW_OBS_FAMILY_EQ, DETSDW_OBS_FAMILY_TD, DETSDW_OBS_FAMILY_PHI = 0, 1, 2, 3
(DETSDW_OBS_KIND_SITE, DETSDW_OBS_KIND_TAU, DETSDW_OBS_KIND_TAU_Q0, DETSDW_OBS_KIND_ROW_SCALAR, DETSDW_OBS_KIND_CORR, DETSDW_OBS_KIND_SQ,
 DETSDW_OBS_KIND_GREEN_MATRIX, DETSDW_OBS_KIND_PHI_CHI, DETSDW_OBS_KIND_PHI_SCALARS) = range(9)


class dqmc_cplx(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


class dqmc_tuning(C.Structure):
    _fields_ = [("pipeline", C.c_int32), ("qr_variant", C.c_int32), ("green_variant", C.c_int32),
                ("max_jacobi_sweeps", C.c_int32), ("proposal_budget", C.c_int32), ("decide_threads", C.c_int32), ("bmult_path", C.c_int32)]


DQMC_TUNING_NO_RNG_LOOKAHEAD = 0x100      # flag bit of dqmc_tuning.bmult_path


class dqmc_schedule_info(C.Structure):
    _fields_ = [("pipelined", C.c_int32), ("proposal_budget", C.c_int32), ("blocks_pipelined", C.c_uint64),
                ("blocks_sequential", C.c_uint64), ("qr_block_gram_schmidt", C.c_int32), ("green_lu", C.c_int32),
                ("cholqr_fallbacks", C.c_uint64), ("uniform_windows_advanced", C.c_uint64), ("uniform_windows_pushed", C.c_uint64)]


class dqmc_params(C.Structure):
    _fields_ = [("opdim", C.c_int32), ("L", C.c_int32), ("m", C.c_int32), ("s", C.c_int32),
                ("delaySteps", C.c_int32), ("bc", C.c_int32), ("weakZflux", C.c_int32),
                ("phi2bosons", C.c_int32), ("device", C.c_int32), ("stabilisation", C.c_int32),
                ("cb_none", C.c_int32), ("model", C.c_int32),
                ("dtau", C.c_double), ("r", C.c_double), ("c", C.c_double), ("u", C.c_double),
                ("lambda_", C.c_double),
                ("txhor", C.c_double), ("txver", C.c_double), ("tyhor", C.c_double), ("tyver", C.c_double),
                ("mux", C.c_double), ("muy", C.c_double), ("accRatio", C.c_double), ("cdwU", C.c_double),
                ("rng_window_per_site", C.c_int32), ("timedisplaced", C.c_int32),
                ("tuning", dqmc_tuning), ("td_particle_hole", C.c_int32)]


class dqmc_update_state(C.Structure):
    _fields_ = [("phiDelta", C.c_double), ("targetAccRatio", C.c_double), ("lastAccRatio", C.c_double),
                ("ra_runningAverage", C.c_double), ("ra_values", C.c_double * 100),
                ("ra_samplesAdded", C.c_int32), ("ra_head", C.c_int32),
                ("rng_consumed", C.c_uint64), ("rng_avail", C.c_uint64),
                ("error", C.c_int32), ("reserved", C.c_int32),
                ("angleDelta", C.c_double), ("scaleDelta", C.c_double),
                ("curminAngleDelta", C.c_double), ("curmaxAngleDelta", C.c_double),
                ("curminScaleDelta", C.c_double), ("curmaxScaleDelta", C.c_double),
                ("rot_runningAverage", C.c_double), ("rot_values", C.c_double * 100),
                ("scl_runningAverage", C.c_double), ("scl_values", C.c_double * 100),
                ("rot_samplesAdded", C.c_int32), ("rot_head", C.c_int32), ("scl_samplesAdded", C.c_int32), ("scl_head", C.c_int32)]


class dqmc_series_state(C.Structure):
    _fields_ = [("bin_size", C.c_int), ("max_bins", C.c_int), ("nfreq", C.c_int), ("parts", C.c_int), ("flags", C.c_int),
                ("bins_closed", C.c_int), ("sweeps_in_open_bin", C.c_int), ("nb", C.c_int),
                ("samples", C.c_longlong), ("rebins", C.c_longlong), ("sample_len", C.c_size_t)]


class dqmc_profile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_uint64 * 8),
                ("svd_calls", C.c_uint64), ("svd_sweeps_total", C.c_uint64), ("svd_sweeps_max", C.c_uint64),
                ("qr_calls", C.c_uint64), ("gemm_flops", C.c_double), ("decomp_round_ms", C.c_double),
                ("decomp_rounds", C.c_uint64), ("blocks_nonempty", C.c_uint64), ("chains", C.c_uint64),
                ("updates_accepted", C.c_uint64), ("lu_calls", C.c_uint64),
                ("sub_ms", C.c_double * 4), ("sub_launches", C.c_uint64 * 4), ("sub_flops", C.c_double * 4), ("sub_bytes", C.c_double * 4)]


class detsdw_params(C.Structure):
    _fields_ = [("opdim", C.c_int32), ("L", C.c_int32), ("m", C.c_int32), ("s", C.c_int32),
                ("delaySteps", C.c_int32), ("globalShift", C.c_int32), ("globalUpdateInterval", C.c_int32),
                ("weakZflux", C.c_int32), ("phi2bosons", C.c_int32), ("device", C.c_int32),
                ("simindex", C.c_int32), ("rngSeed", C.c_uint32), ("has_mux_muy", C.c_int32),
                ("updateMethod", C.c_int32), ("bc", C.c_char * 16),
                ("beta", C.c_double), ("dtau", C.c_double),
                ("r", C.c_double), ("c", C.c_double), ("u", C.c_double), ("lambda_", C.c_double),
                ("txhor", C.c_double), ("txver", C.c_double), ("tyhor", C.c_double), ("tyver", C.c_double),
                ("mu", C.c_double), ("mux", C.c_double), ("muy", C.c_double),
                ("accRatio", C.c_double), ("cdwU", C.c_double),
                ("stabilisation", C.c_int32), ("cb_none", C.c_int32),
                ("wolffClusterUpdate", C.c_int32), ("wolffClusterShiftUpdate", C.c_int32),
                ("repeatWolffPerSweep", C.c_int32), ("fermionMeasurements", C.c_int32),
                ("spinProposalMethod", C.c_int32), ("adaptScaleVariance", C.c_int32), ("repeatUpdateInSlice", C.c_int32),
                ("timeDisplacedMeasurements", C.c_int32),
                ("tuning", dqmc_tuning), ("timeDisplacedParticleHole", C.c_int32)]


class detsdw_info(C.Structure):
    _fields_ = [("opdim", C.c_int32), ("L", C.c_int32), ("N", C.c_int32), ("MSF", C.c_int32),
                ("n_g", C.c_int32), ("m", C.c_int32), ("s", C.c_int32), ("n", C.c_int32),
                ("performedSweeps", C.c_int32), ("lastSweepDir", C.c_int32),
                ("acceptedGlobalShifts", C.c_int32), ("attemptedGlobalShifts", C.c_int32),
                ("currentTimeslice", C.c_int32), ("reserved", C.c_int32),
                ("acceptedWolffClusterUpdates", C.c_int32), ("attemptedWolffClusterUpdates", C.c_int32),
                ("acceptedWolffClusterShiftUpdates", C.c_int32), ("attemptedWolffClusterShiftUpdates", C.c_int32),
                ("addedWolffClusterSize", C.c_double),
                ("beta", C.c_double), ("dtau", C.c_double),
                ("phiDelta", C.c_double), ("lastAccRatioLocal_phi", C.c_double), ("r", C.c_double),
                ("angleDelta", C.c_double), ("scaleDelta", C.c_double),
                ("rngDrawn", C.c_uint64)]


class detsdw_observable_desc(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("family", "block", "component", "kind", "fine", "has_fine_twin", "has_matsubara",
                                          "series_part", "series_bit")]


class detsdw_observables(C.Structure):
    _fields_ = [("meanPhi", C.c_double * 3), ("normMeanPhi", C.c_double), ("associatedEnergy", C.c_double),
                ("phiRhoS_Gc", C.c_double), ("phiRhoS_Gs", C.c_double), ("valid", C.c_int32), ("fermionic_valid", C.c_int32),
                ("greenK0", C.c_double), ("greenLocal", C.c_double), ("pairPlusMax", C.c_double), ("pairMinusMax", C.c_double),
                ("occDiffSq", C.c_double)]


class detsdw_control_data(C.Structure):
    _fields_ = [("acceptedGlobalShifts", C.c_int32), ("attemptedGlobalShifts", C.c_int32),
                ("acceptedWolffClusterUpdates", C.c_int32), ("attemptedWolffClusterUpdates", C.c_int32),
                ("acceptedWolffClusterShiftUpdates", C.c_int32), ("attemptedWolffClusterShiftUpdates", C.c_int32),
                ("addedWolffClusterSize", C.c_double),
                ("adjust", dqmc_update_state)]


# every symbol include/*.h declares: (name, restype, argtypes)
_P = C.c_void_p
_DP = C.POINTER(C.c_double)
class dethubbard_params(C.Structure):
    _fields_ = [("L", C.c_int32), ("d", C.c_int32), ("m", C.c_int32), ("s", C.c_int32), ("checkerboard", C.c_int32),
                ("device", C.c_int32), ("simindex", C.c_int32), ("rngSeed", C.c_uint32), ("stabilisation", C.c_int32),
                ("measureFlags", C.c_int32), ("beta", C.c_double), ("dtau", C.c_double), ("t", C.c_double), ("U", C.c_double),
                ("mu", C.c_double)]


DETHUBBARD_MEASURE_EQ, DETHUBBARD_MEASURE_TD, DETHUBBARD_MEASURE_TD_FINE = 1, 2, 4      # dethubbard_params.measureFlags (include/dethubbard_host.h)
DETHUBBARD_SERIES_NO_HOST_COPY = 1                       # flag of dethubbard_series_begin
# observable indices of the dethubbard_series_* readers: the eight '...Corr' / '...Sq' and the six '...Tau' / '...TauSq' follow in channel order
(DETHUBBARD_OBS_SCALARS, DETHUBBARD_OBS_ZCORR, DETHUBBARD_OBS_GREENUPCORR, DETHUBBARD_OBS_GREENUPSQ, DETHUBBARD_OBS_GREENUPTAU,
 DETHUBBARD_OBS_GREENUPTAUSQ) = 0, 1, 2, 10, 18, 24


class dethubbard_observables(C.Structure):
    _fields_ = [("occUp", C.c_double), ("occDn", C.c_double), ("occTotal", C.c_double), ("occDouble", C.c_double),
                ("localMoment", C.c_double), ("eKinetic", C.c_double), ("ePotential", C.c_double), ("eTotal", C.c_double),
                ("valid", C.c_int32), ("reserved", C.c_int32)]


class dethubbard_info(C.Structure):
    _fields_ = [("L", C.c_int32), ("N", C.c_int32), ("m", C.c_int32), ("s", C.c_int32), ("n", C.c_int32),
                ("performedSweeps", C.c_int32), ("lastSweepDir", C.c_int32), ("currentTimeslice", C.c_int32),
                ("beta", C.c_double), ("dtau", C.c_double), ("alpha", C.c_double), ("lastAccRatio", C.c_double),
                ("rngDrawn", C.c_uint64)]


SYMBOLS = [
    ("dqmc_create", C.c_int, [C.POINTER(dqmc_params), C.POINTER(_P)]),
    ("dqmc_create_batch", C.c_int, [C.POINTER(dqmc_params), C.c_int, C.POINTER(_P)]),
    ("dqmc_select_chain", C.c_int, [_P, C.c_int]),
    ("dqmc_num_chains", C.c_int, [_P]),
    ("dqmc_destroy", None, [_P]),
    ("dqmc_last_error", C.c_char_p, []),
    ("dqmc_synchronize", C.c_int, [_P]),
    ("dqmc_stream", _P, [_P]),
    ("dqmc_set_fields_host", C.c_int, [_P, _DP]),
    ("dqmc_get_fields_host", C.c_int, [_P, _DP, _DP, _DP]),
    ("dqmc_set_cdwl_host", C.c_int, [_P, _P]),
    ("dqmc_get_cdwl_host", C.c_int, [_P, _P]),
    ("dqmc_set_fields_all_host", C.c_int, [_P, _DP]),
    ("dqmc_get_fields_all_host", C.c_int, [_P, _DP]),
    ("dqmc_bmult_host", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("dqmc_bmult_src_host", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("dqmc_udv_decompose_host", C.c_int, [_P, _P, _P, _DP, _P, C.POINTER(C.c_int)]),
    ("dqmc_decompose_host", C.c_int, [_P, _P, _DP, _DP, C.c_int, _P, _P, _DP, _P, C.POINTER(C.c_int)]),
    ("dqmc_green_from_factors_host", C.c_int, [_P, _P, _DP, _P, _P, _DP, _P, _P, _DP, _P, _P, _P]),
    ("dqmc_gemm_host", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    ("dqmc_udv_setup", C.c_int, [_P]),
    ("dqmc_advance", C.c_int, [_P, C.c_int, C.c_int]),
    ("dqmc_wrap", C.c_int, [_P, C.c_int, C.c_int]),
    ("dqmc_wrap_skip", C.c_int, [_P, C.c_int, C.c_int]),
    ("dqmc_reset_storage0", C.c_int, [_P]),
    ("dqmc_push_uniforms_host", C.c_int, [_P, _DP, C.c_size_t]),
    ("dqmc_push_uniforms_all_host", C.c_int, [_P, _DP, C.c_size_t]),
    ("dqmc_uniforms_staging_host", C.c_int, [_P, C.POINTER(_DP), C.POINTER(C.c_size_t)]),
    ("dqmc_stage_uniforms_tail_host", C.c_int, [_P, _DP, C.c_size_t]),
    ("dqmc_advance_uniforms", C.c_int, [_P, C.POINTER(C.c_uint64)]),
    ("dqmc_get_uniform_window_host", C.c_int, [_P, _DP, C.c_size_t]),
    ("dqmc_update_slice", C.c_int, [_P, C.c_int, C.c_int]),
    ("dqmc_update_slice_ex", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dqmc_update_slice_final", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dqmc_get_schedule_info", C.c_int, [_P, C.POINTER(dqmc_schedule_info)]),
    ("dqmc_get_update_states_all_host", C.c_int, [_P, C.POINTER(dqmc_update_state)]),
    ("dqmc_get_update_state_host", C.c_int, [_P, C.POINTER(dqmc_update_state)]),
    ("dqmc_set_update_state_host", C.c_int, [_P, C.POINTER(dqmc_update_state)]),
    ("dqmc_get_green_host", C.c_int, [_P, _P]),
    ("dqmc_set_green_host", C.c_int, [_P, _P, C.c_int]),
    ("dqmc_get_sv_host", C.c_int, [_P, _DP]),
    ("dqmc_get_sv_all_host", C.c_int, [_P, _DP]),
    ("dqmc_get_udv_host", C.c_int, [_P, C.c_int, _P, _DP, _P]),
    ("dqmc_current_timeslice", C.c_int, [_P]),
    ("dqmc_backup", C.c_int, [_P]),
    ("dqmc_restore", C.c_int, [_P]),
    ("dqmc_exchange_action_host", C.c_int, [_P, _DP]),
    ("dqmc_exchange_actions_device", C.c_int, [_P, _P]),
    ("dqmc_phi_action_all_host", C.c_int, [_P, _DP]),
    ("dqmc_shift_fields_all_host", C.c_int, [_P, _DP]),
    ("dqmc_set_exchange_parameter", C.c_int, [_P, C.c_double]),
    ("dqmc_shift_green_symmetric_host", C.c_int, [_P, _P]),
    ("dqmc_measure_reset", C.c_int, [_P]),
    ("dqmc_measure_slice", C.c_int, [_P]),
    ("dqmc_measure_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_equal_time_correlators", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_eq_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_eq_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_equal_time_band", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_eq_band_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_eq_band_read_host", C.c_int, [_P, _DP]),
    ("dqmc_hubbard_set_equal_time_correlators", C.c_int, [_P, C.c_int]),
    ("dqmc_hubbard_eq_accum_size", C.c_size_t, [_P]),
    ("dqmc_hubbard_eq_read_host", C.c_int, [_P, _DP]),
    ("dqmc_hubbard_measure_timedisplaced", C.c_int, [_P, C.c_int]),
    ("dqmc_hubbard_td_accum_size", C.c_size_t, [_P]),
    ("dqmc_hubbard_td_read_host", C.c_int, [_P, _DP]),
    ("dqmc_hubbard_measure_timedisplaced_segment", C.c_int, [_P, C.c_int]),
    ("dqmc_hubbard_measure_timedisplaced_ends", C.c_int, [_P]),
    ("dqmc_hubbard_td_fine_accum_size", C.c_size_t, [_P]),
    ("dqmc_hubbard_td_fine_read_host", C.c_int, [_P, _DP]),
    ("dqmc_hubbard_td_fine_counts_host", C.c_int, [_P, _DP]),
    ("dqmc_hubbard_td_matsubara_size", C.c_size_t, [_P, C.c_int]),
    ("dqmc_hubbard_td_matsubara_host", C.c_int, [_P, C.c_int, _DP]),
    ("dqmc_set_timedisplaced", C.c_int, [_P, C.c_int]),
    ("dqmc_get_green_timedisplaced_host", C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    ("dqmc_measure_timedisplaced", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_read_host", C.c_int, [_P, _DP]),
    ("dqmc_measure_timedisplaced_pair", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_pair_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_pair_read_host", C.c_int, [_P, _DP]),
    ("dqmc_measure_timedisplaced_ph", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_ph_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_ph_read_host", C.c_int, [_P, _DP]),
    ("dqmc_get_green0_timedisplaced_host", C.c_int, [_P, _P, C.POINTER(C.c_int)]),
    ("dqmc_measure_timedisplaced_current", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_current_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_current_read_host", C.c_int, [_P, _DP]),
    ("dqmc_measure_timedisplaced_band", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_band_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_band_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_custom_bilinears", C.c_int, [_P, C.c_int, _P]),
    ("dqmc_get_custom_bilinears", C.c_int, [_P, C.POINTER(C.c_int), _P]),
    ("dqmc_set_custom_bond_bilinears", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("dqmc_get_custom_bond_bilinears", C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P]),
    ("dqmc_measure_timedisplaced_custom", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_custom_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_custom_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_equal_time_custom", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_eq_custom_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_eq_custom_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_custom_pair_operators", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("dqmc_get_custom_pair_operators", C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P]),
    ("dqmc_measure_timedisplaced_custom_pair", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_custom_pair_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_custom_pair_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_equal_time_custom_pair", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_eq_custom_pair_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_eq_custom_pair_read_host", C.c_int, [_P, _DP]),
    ("dqmc_set_green_matrix", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_timedisplaced_green_matrix", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_td_green_matrix_accum_size", C.c_size_t, [_P]),
    ("dqmc_measure_td_green_matrix_read_host", C.c_int, [_P, _DP]),
    ("dqmc_measure_timedisplaced_segment", C.c_int, [_P, C.c_int]),
    ("dqmc_measure_timedisplaced_ends", C.c_int, [_P]),
    ("dqmc_measure_td_fine_accum_size", C.c_size_t, [_P, C.c_int]),
    ("dqmc_measure_td_fine_read_host", C.c_int, [_P, C.c_int, _DP]),
    ("dqmc_measure_td_matsubara_size", C.c_size_t, [_P, C.c_int, C.c_int]),
    ("dqmc_measure_td_matsubara_host", C.c_int, [_P, C.c_int, C.c_int, _DP]),
    ("dqmc_series_begin", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("dqmc_series_layout", C.c_int, [_P, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("dqmc_series_add_sweep", C.c_int, [_P]),
    ("dqmc_series_form_sample", C.c_int, [_P]),
    ("dqmc_series_sample_device", C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("dqmc_series_accumulate", C.c_int, [_P, C.POINTER(C.c_void_p)]),
    ("dqmc_series_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("dqmc_series_read_bins_host", C.c_int, [_P, C.c_int, C.c_int, _DP]),
    ("dqmc_series_stats_host", C.c_int, [_P, _DP, _DP]),
    ("dqmc_series_derived_host", C.c_int, [_P, _DP, _DP]),
    ("dqmc_series_phi_derived_host", C.c_int, [_P, _DP, _DP]),
    ("dqmc_series_band_derived_host", C.c_int, [_P, _DP, _DP]),
    ("dqmc_series_custom_derived_host", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dqmc_series_custom_pair_derived_host", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dqmc_series_pair_vertex_size", C.c_size_t, [_P]),
    ("dqmc_series_pair_vertex_host", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dqmc_series_ph_vertex_size", C.c_size_t, [_P]),
    ("dqmc_series_ph_vertex_host", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dqmc_series_hubbard_derived_host", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dqmc_series_end", C.c_int, [_P]),
    ("dqmc_series_configure", C.c_int, [_P, C.c_int]),
    ("dqmc_series_get_state", C.c_int, [_P, C.POINTER(dqmc_series_state)]),
    ("dqmc_series_rebin", C.c_int, [_P]),
    ("dqmc_series_binning_host", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("dqmc_series_export_host", C.c_int, [_P, _DP, C.c_size_t]),
    ("dqmc_series_import_host", C.c_int, [_P, C.POINTER(dqmc_series_state), _DP, C.c_size_t]),
    ("dqmc_get_green_td_fine_host", C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_int)]),
    ("dqmc_td_fine_propagate", C.c_int, [_P, C.c_int, C.c_int]),     # tests only: exported, not declared in include/dqmc_hip.h
    ("dqmc_set_green_check", C.c_int, [_P, C.c_int]),
    ("dqmc_green_check_size", C.c_size_t, [_P]),
    ("dqmc_green_check_read_host", C.c_int, [_P, _DP]),
    ("dqmc_green_check_reset", C.c_int, [_P]),
    ("dqmc_profile_enable", C.c_int, [_P, C.c_int]),
    ("dqmc_profile_read", C.c_int, [_P, C.POINTER(dqmc_profile)]),
    ("detsdw_create", C.c_int, [C.POINTER(detsdw_params), C.POINTER(_P)]),
    ("detsdw_create_batch", C.c_int, [C.POINTER(detsdw_params), C.c_int, C.POINTER(_P)]),
    ("detsdw_create_batch_ex", C.c_int, [C.POINTER(detsdw_params), C.c_int, C.c_int, C.POINTER(_P)]),
    ("detsdw_num_sub_batches", C.c_int, [_P]),
    ("detsdw_ctx_of_chain", _P, [_P, C.c_int, C.POINTER(C.c_int)]),
    ("detsdw_select_chain", C.c_int, [_P, C.c_int]),
    ("detsdw_num_chains", C.c_int, [_P]),
    ("detsdw_destroy", None, [_P]),
    ("detsdw_last_error", C.c_char_p, []),
    ("detsdw_sweep", C.c_int, [_P, C.c_int]),
    ("detsdw_sweep_thermalization", C.c_int, [_P]),
    ("detsdw_get_info", C.c_int, [_P, C.POINTER(detsdw_info)]),
    ("detsdw_get_observables", C.c_int, [_P, C.POINTER(detsdw_observables)]),
    ("detsdw_get_observable_vector", C.c_int, [_P, C.c_int, _DP]),
    ("detsdw_describe_observable", C.c_int, [C.c_int, C.POINTER(detsdw_observable_desc)]),
    ("detsdw_get_matsubara", C.c_int, [_P, C.c_int, C.c_int, _DP]),
    ("detsdw_get_matsubara_all", C.c_int, [_P, C.c_int, C.c_int, _DP]),
    ("detsdw_series_begin", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("detsdw_series_route", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("detsdw_series_get_route", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("detsdw_series_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("detsdw_series_stats", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("detsdw_series_stats_all", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("detsdw_series_derived_all", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("detsdw_series_band_derived", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("detsdw_set_custom_bilinears", C.c_int, [_P, C.c_int, _P]),
    ("detsdw_set_custom_bond_bilinears", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("detsdw_get_custom_bond_bilinears", C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P]),
    ("detsdw_series_custom_derived", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_set_custom_pair_operators", C.c_int, [_P, C.c_int, _P, _P, _P]),
    ("detsdw_get_custom_pair_operators", C.c_int, [_P, C.POINTER(C.c_int), _P, _P, _P]),
    ("detsdw_series_custom_pair_derived", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_set_green_matrix", C.c_int, [_P, C.c_int]),
    ("detsdw_series_pair_vertex", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_series_ph_vertex", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_set_green_check", C.c_int, [_P, C.c_int]),
    ("detsdw_get_green_check", C.c_int, [_P, _DP]),
    ("detsdw_reset_green_check", C.c_int, [_P]),
    ("detsdw_series_read_bins", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP]),
    ("detsdw_series_end", C.c_int, [_P]),
    ("detsdw_series_configure", C.c_int, [_P, C.c_int]),
    ("detsdw_series_rebin", C.c_int, [_P]),
    ("detsdw_series_get_state", C.c_int, [_P, C.POINTER(dqmc_series_state)]),
    ("detsdw_series_binning", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_series_binning_all", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("detsdw_series_save", C.c_int, [_P, C.c_char_p]),
    ("detsdw_series_load", C.c_int, [_P, C.c_char_p]),
    ("detsdw_get_tau_grid", C.c_int, [_P, _DP]),
    ("detsdw_get_tau_grid_fine", C.c_int, [_P, _DP]),
    ("detsdw_get_phi", C.c_int, [_P, _DP]),
    ("detsdw_set_phi", C.c_int, [_P, _DP]),
    ("detsdw_get_cdwl", C.c_int, [_P, _P]),
    ("detsdw_set_cdwl", C.c_int, [_P, _P]),
    ("detsdw_get_green", C.c_int, [_P, _P]),
    ("detsdw_get_green_inv_sv", C.c_int, [_P, _DP]),
    ("detsdw_save_configuration_stream_binary", C.c_int, [_P, C.c_char_p]),
    ("detsdw_save_state", C.c_int, [_P, C.c_char_p]),
    ("detsdw_load_state", C.c_int, [_P, C.c_char_p]),
    ("detsdw_rng_rand01", C.c_double, [_P]),
    ("detsdw_ctx", _P, [_P]),
    ("detsdw_get_exchange_parameter_value", C.c_double, [_P]),
    ("detsdw_set_exchange_parameter_value", C.c_int, [_P, C.c_double]),
    ("detsdw_get_exchange_parameter_name", C.c_char_p, [_P]),
    ("detsdw_get_exchange_action_contribution", C.c_int, [_P, _DP]),
    ("detsdw_exchange_actions_device", C.c_int, [_P, _P]),
    ("detsdw_get_control_data", C.c_int, [_P, C.POINTER(detsdw_control_data)]),
    ("detsdw_set_control_data", C.c_int, [_P, C.POINTER(detsdw_control_data)]),
    ("detsdw_replica_exchange_probability", C.c_double, [C.c_double] * 4),
    ("detsdw_rng_fill", C.c_int, [C.c_uint32, C.c_uint32, _DP, C.c_size_t]),
    ("detsdw_rng_replay", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_size_t, _DP, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    ("dethubbard_create", C.c_int, [C.POINTER(dethubbard_params), C.c_int, C.POINTER(_P)]),
    ("dethubbard_destroy", None, [_P]),
    ("dethubbard_last_error", C.c_char_p, []),
    ("dethubbard_select_chain", C.c_int, [_P, C.c_int]),
    ("dethubbard_sweep", C.c_int, [_P, C.c_int]),
    ("dethubbard_sweep_thermalization", C.c_int, [_P]),
    ("dethubbard_get_info", C.c_int, [_P, C.POINTER(dethubbard_info)]),
    ("dethubbard_get_auxfield", C.c_int, [_P, _DP]),
    ("dethubbard_get_green", C.c_int, [_P, _DP, _DP]),
    ("dethubbard_get_observables", C.c_int, [_P, C.POINTER(dethubbard_observables)]),
    ("dethubbard_get_zcorr", C.c_int, [_P, _DP]),
    ("dethubbard_get_eq_correlators", C.c_int, [_P, _DP]),
    ("dethubbard_get_td_correlators", C.c_int, [_P, _DP]),
    ("dethubbard_get_td_fine_correlators", C.c_int, [_P, _DP]),
    ("dethubbard_get_matsubara", C.c_int, [_P, C.c_int, _DP]),
    ("dethubbard_get_matsubara_all", C.c_int, [_P, C.c_int, _DP]),
    ("dethubbard_save_state", C.c_int, [_P, C.c_char_p]),
    ("dethubbard_load_state", C.c_int, [_P, C.c_char_p]),
    ("dethubbard_set_green_check", C.c_int, [_P, C.c_int]),
    ("dethubbard_get_green_check", C.c_int, [_P, _DP]),
    ("dethubbard_reset_green_check", C.c_int, [_P]),
    ("dethubbard_rng_rand01", C.c_double, [_P]),
    ("dethubbard_ctx", _P, [_P]),
    ("dethubbard_series_begin", C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    ("dethubbard_series_info", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("dethubbard_series_stats", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("dethubbard_series_stats_all", C.c_int, [_P, C.c_int, _DP, _DP]),
    ("dethubbard_series_read_bins", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _DP]),
    ("dethubbard_series_derived_all", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dethubbard_series_configure", C.c_int, [_P, C.c_int]),
    ("dethubbard_series_rebin", C.c_int, [_P]),
    ("dethubbard_series_get_state", C.c_int, [_P, C.POINTER(dqmc_series_state)]),
    ("dethubbard_series_binning", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dethubbard_series_binning_all", C.c_int, [_P, C.c_int, C.c_int, _DP, _DP]),
    ("dethubbard_series_save", C.c_int, [_P, C.c_char_p]),
    ("dethubbard_series_load", C.c_int, [_P, C.c_char_p]),
    ("dethubbard_series_end", C.c_int, [_P]),
]

_lib = None


def load():
    """Load the shared library; raises if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python -m detqmc_amd.build` "
                          "(there is no CPU fallback for the DQMC kernels)")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, host=False):
    if rc != 0:
        lib = load()
        msg = (lib.dethubbard_last_error() if host == "hubbard" else lib.detsdw_last_error() if host else lib.dqmc_last_error()) or b""
        raise DqmcError(rc, msg.decode("utf-8", "replace"))
