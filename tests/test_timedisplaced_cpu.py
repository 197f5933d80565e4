"""Host-side checks of the time-displaced measurement option (no GPU needed: parameters are checked before any device work)."""
import ctypes as C

import pytest


def test_option_needs_fermion_measurements():
    from detqmc_amd import DqmcError, SDWParams
    from detqmc_amd.model import DetSDW
    with pytest.raises(DqmcError, match="timeDisplacedMeasurements needs fermionMeasurements"):
        DetSDW(SDWParams(opdim=2, L=4, beta=2.0, s=5, timeDisplacedMeasurements=True, fermionMeasurements=False))


def test_struct_layout_unchanged():
    from detqmc_amd import _lib
    names = [f[0] for f in _lib.detsdw_params._fields_]
    assert names[names.index("repeatUpdateInSlice") + 1] == "timeDisplacedMeasurements"
    assert _lib.detsdw_params.timeDisplacedMeasurements.size == 4
    assert _lib.dqmc_params.timedisplaced.offset + 4 == _lib.dqmc_params.tuning.offset
    lib = _lib.load()
    for sym in ("dqmc_set_timedisplaced", "dqmc_get_green_timedisplaced_host", "dqmc_measure_timedisplaced",
                "dqmc_measure_td_accum_size", "dqmc_measure_td_read_host", "detsdw_get_tau_grid"):
        assert hasattr(lib, sym)
    assert lib.dqmc_measure_td_accum_size(None) == 0
    assert lib.detsdw_get_tau_grid(None, (C.c_double * 4)()) != 0
