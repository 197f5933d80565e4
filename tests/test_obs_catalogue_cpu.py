"""detsdw_describe_observable against what include/detsdw_host.h and include/dqmc_hip.h document of every observable index, and the names
of detqmc_amd.model against the descriptors.  The expectations are written out here, not derived from the catalogue.  Needs no GPU."""
import ctypes as C
import types

import pytest

from detqmc_amd import _lib, model

FINE = _lib.DETSDW_OBS_FINE
LAST = 74                                      # DETSDW_OBS_GREENMATRIXTAU
# DETSDW_OBS_FINE twins: GREENKTAU_X .. BONDKINETICY, the band tau names, custom / custom-pair Tau and TauQ0 (four slots each), GREENMATRIXTAU
FINE_TWINS = set(range(4, 22)) | set(range(34, 38)) | set(range(42, 50)) | set(range(58, 66)) | {74}
# index -> (part of dqmc_series_layout, DQMC_SERIES_* bit)
SERIES = {}
for _indices, _part in ((range(22, 32), 0), ((4, 5), 1), ((6, 7), 2), ((10, 11, 12), 3), ((16, 17), 4), ((32, 33), 6), ((34, 35), 7),
                        (range(38, 42), 8), (range(42, 46), 9), (range(50, 58), 10), (range(58, 62), 11), (range(66, 74), 12), ((74,), 13)):
    for _w in _indices:
        SERIES[_w] = (_part, 1 << _part)


@pytest.fixture(scope="module")
def describe():
    import detqmc_amd
    lib = detqmc_amd.load()

    def call(which):
        d = _lib.detsdw_observable_desc()
        return lib.detsdw_describe_observable(which, C.byref(d)), d
    return call


def test_known_indices_fine_twins_transforms_and_series_parts(describe):
    assert (_lib.DQMC_SERIES_MATS_BAND, _lib.DQMC_SERIES_EQ_BAND, _lib.DQMC_SERIES_MATS_CUSTOM, _lib.DQMC_SERIES_EQ_CUSTOM, _lib.DQMC_SERIES_MATS_CUSTOM_PAIR,
            _lib.DQMC_SERIES_EQ_CUSTOM_PAIR, _lib.DQMC_SERIES_GREEN_MATRIX) == (128, 256, 512, 1024, 2048, 4096, 8192)
    matsubara = set(model.MATSUBARA.values()) | set(range(42, 46)) | set(range(58, 62))
    for which in range(LAST + 1):                          # every index up to the last is documented, all four slots of the custom ranges
        rc, d = describe(which)
        assert rc == 0, which
        assert not d.fine
        assert bool(d.has_fine_twin) == (which in FINE_TWINS), which
        assert bool(d.has_matsubara) == (which in matsubara), which
        assert (d.series_part, d.series_bit) == SERIES.get(which, (-1, -1)), which
        rc, f = describe(which | FINE)
        assert (rc == 0) == (which in FINE_TWINS), which
        if rc == 0:                                        # the twin is the same observable on the other grid; no reader but the vector's takes it
            assert f.fine and f.has_fine_twin and not f.has_matsubara and (f.series_part, f.series_bit) == (-1, -1)
            assert (f.family, f.block, f.component, f.kind) == (d.family, d.block, d.component, d.kind)


def test_unknown_indices_are_refused(describe):
    import detqmc_amd
    for which in (-1, -2, -FINE, LAST + 1, LAST + 2, 77, 78, 255, (LAST + 1) | FINE, 2 * FINE, 4 | 2 * FINE):
        assert describe(which)[0] == -1, which
    assert b"unknown observable" in detqmc_amd.load().detsdw_last_error()


def test_components_blocks_and_kinds(describe):
    K = _lib
    TD, EQ = K.DETSDW_OBS_FAMILY_TD, K.DETSDW_OBS_FAMILY_EQ
    expect = {0: (K.DETSDW_OBS_FAMILY_SLICE, 0, 0, K.DETSDW_OBS_KIND_SITE), 3: (K.DETSDW_OBS_FAMILY_SLICE, 0, 3, K.DETSDW_OBS_KIND_SITE),
              5: (TD, 0, 1, K.DETSDW_OBS_KIND_TAU), 7: (TD, 1, 1, K.DETSDW_OBS_KIND_TAU), 9: (TD, 1, 1, K.DETSDW_OBS_KIND_TAU_Q0),
              12: (TD, 2, 2, K.DETSDW_OBS_KIND_TAU), 15: (TD, 2, 2, K.DETSDW_OBS_KIND_TAU_Q0), 17: (TD, 3, 1, K.DETSDW_OBS_KIND_TAU),
              19: (TD, 3, 1, K.DETSDW_OBS_KIND_TAU_Q0), 21: (TD, 3, 1, K.DETSDW_OBS_KIND_ROW_SCALAR), 26: (EQ, 0, 4, K.DETSDW_OBS_KIND_CORR),
              31: (EQ, 0, 4, K.DETSDW_OBS_KIND_SQ), 32: (K.DETSDW_OBS_FAMILY_PHI, 0, 0, K.DETSDW_OBS_KIND_PHI_CHI),
              33: (K.DETSDW_OBS_FAMILY_PHI, 0, 0, K.DETSDW_OBS_KIND_PHI_SCALARS), 35: (TD, 4, 1, K.DETSDW_OBS_KIND_TAU),
              37: (TD, 4, 1, K.DETSDW_OBS_KIND_TAU_Q0), 39: (EQ, 1, 1, K.DETSDW_OBS_KIND_CORR), 41: (EQ, 1, 1, K.DETSDW_OBS_KIND_SQ),
              45: (TD, 5, 3, K.DETSDW_OBS_KIND_TAU), 46: (TD, 5, 0, K.DETSDW_OBS_KIND_TAU_Q0), 53: (EQ, 2, 3, K.DETSDW_OBS_KIND_CORR),
              54: (EQ, 2, 0, K.DETSDW_OBS_KIND_SQ), 61: (TD, 6, 3, K.DETSDW_OBS_KIND_TAU), 65: (TD, 6, 3, K.DETSDW_OBS_KIND_TAU_Q0),
              66: (EQ, 3, 0, K.DETSDW_OBS_KIND_CORR), 73: (EQ, 3, 3, K.DETSDW_OBS_KIND_SQ), 74: (TD, 7, 0, K.DETSDW_OBS_KIND_GREEN_MATRIX)}
    for which, want in expect.items():
        d = describe(which)[1]
        assert (d.family, d.block, d.component, d.kind) == want, which


def test_python_names_resolve_to_the_documented_shapes():
    """every name of the table, every custom name and every 'Fine' twin: the shape observable_vector documents, from the descriptor's kind"""
    info = types.SimpleNamespace(N=16, m=12, n=3, opdim=2)
    names = [n for n in model.OBSERVABLES if n not in model.SERIES_PHI_OBS]
    names += [f"{p}{c}{k}" for p in ("custom", "customPair") for c in range(4) for k in ("Tau", "TauQ0", "Corr", "Sq")]
    assert len(set(model.OBSERVABLES.values())) == len(model.OBSERVABLES) == 43
    for name in names:
        which, d = model.observable_index(name)
        for fine in (False, True):
            rows = info.m + 1 if fine else info.n - 1
            want = ((rows, info.N, 4, 4) if name == "greenMatrixTau" else (rows, info.N) if name.endswith("Tau") or name.startswith("greenKTau")
                    else (rows,) if name.endswith("TauQ0") or name.startswith("bondKinetic") else (info.N,))
            if not fine:
                assert model.observable_shape(d, info) == (want, name == "greenMatrixTau"), name
            elif which in FINE_TWINS:
                wf, df = model.observable_index(name + "Fine")
                assert wf == which | FINE and model.observable_shape(df, info) == (want, name == "greenMatrixTau"), name
            else:
                with pytest.raises(KeyError):
                    model.observable_index(name + "Fine")
    # what the series readers return
    for name, want in (("chargeSq", ((16,), False)), ("custom3Corr", ((16,), False)), ("phiChi", ((3, 16), False)), ("phiScalars", ((5,), False)),
                       ("sdwTau", ((3, 16), True)), ("customPair0Tau", ((3, 16), True)), ("greenMatrixTau", ((13, 16, 2, 2), True))):
        assert model.observable_shape(model.observable_index(name)[1], info, nfreq=3, series=True) == want, name
    assert model.observable_shape(model.observable_index("greenMatrixTau")[1], types.SimpleNamespace(N=16, m=12, n=3, opdim=3), 3, True)[0] == (13, 16, 4, 4)
    for name in ("nothing", "custom4Tau", "customPair0", "chargeTauFineFine", "phiChiFine"):
        with pytest.raises(KeyError):
            model.observable_index(name)


def test_exported_views_keep_their_contents():
    assert model.MATSUBARA == {"greenKTauX": 4, "greenKTauY": 5, "pairPlusTau": 6, "pairMinusTau": 7, "chargeTau": 10, "spinZTau": 11, "sdwTau": 12,
                               "currentXTau": 16, "currentYTau": 17, "bandDiffTau": 34, "bandMixTau": 35}
    assert model.EQ_CORRELATORS == {"chargeCorr": 22, "spinZCorr": 23, "sdwCorr": 24, "pairPlusCorr": 25, "pairMinusCorr": 26,
                                    "chargeSq": 27, "spinZSq": 28, "sdwSq": 29, "pairPlusSq": 30, "pairMinusSq": 31}
    assert model.BAND_EQ_CORRELATORS == {"bandDiffCorr": 38, "bandMixCorr": 39, "bandDiffSq": 40, "bandMixSq": 41}
    assert model.CUSTOM_OBS_BASE == {"Tau": 42, "TauQ0": 46, "Corr": 50, "Sq": 54}
    assert model.CUSTOM_PAIR_OBS_BASE == {"Tau": 58, "TauQ0": 62, "Corr": 66, "Sq": 70}
    assert model.SERIES_PHI_OBS == {"phiChi": 32, "phiScalars": 33} and model.GREEN_MATRIX_OBS == 74
    assert model.custom_observable("custom2Sq") == ("Sq", 56) and model.custom_pair_observable("customPair1TauQ0") == ("TauQ0", 63)
    assert model.custom_observable("customPair1Tau") is None and model.custom_pair_observable("custom1Tau") is None
