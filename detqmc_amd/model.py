"""Thin Python mirrors of the two native layers.

  KernelContext  <-> dqmc_ctx (include/dqmc_hip.h): the kernel-level ABI, method names follow the
                     reference functions each call replaces (detmodel.h / detsdwopdim.cpp).
  DetSDW         <-> detqmc::DetSDW (C++ host layer, include/detsdw_host.h): the replica with the
                     reference's operator surface: sweep(), sweepThermalization(),
                     get/set_exchange_parameter_value(), get_exchange_action_contribution(), ...

numpy arrays cross the boundary in the reference's layouts: complex128 column-major n_g x n_g
matrices, phi as (N, OPDIM, m+1) column-major.
"""
import ctypes as C
import re
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, load

BC = {"pbc": 0, "apbc-x": 1, "apbc-y": 2, "apbc-xy": 3}
UPDATE_METHOD = {"iterative": 0, "woodbury": 1, "delayed": 2}
STABILISATION = {"svd": 0, "qr": 1}
LEFT, RIGHT = 0, 1
UP, DOWN = +1, -1


@dataclass
class SDWParams:
    """ModelParamsDetSDW (reference src/detsdwparams.h:24-120), defaults of the shipped examples."""
    opdim: int = 2
    L: int = 4
    beta: float = 0.0
    m: int = 0
    dtau: float = 0.1
    s: int = 10
    r: float = -1.0
    c: float = 3.0
    u: float = 1.0
    lambda_: float = 1.0
    txhor: float = -1.0
    txver: float = -0.5
    tyhor: float = 0.5
    tyver: float = 1.0
    mu: float = -0.5
    mux: float = None
    muy: float = None
    accRatio: float = 0.5
    delaySteps: int = 16
    updateMethod: str = "delayed"
    bc: str = "pbc"
    weakZflux: bool = False
    globalShift: bool = False
    wolffClusterUpdate: bool = False
    wolffClusterShiftUpdate: bool = False
    repeatWolffPerSweep: int = 1
    fermionMeasurements: bool = False    # sweep(True) also takes the G-dependent observables (reference default: on)
    equalTimeCorrelators: bool = False   # ... and the equal-time charge / spinZ / SDW / pairing correlators C(d) and S(q), all m slices (needs fermionMeasurements)
    timeDisplacedMeasurements: bool = False   # ... and G(k, tau_j) at the interior stabilisation boundaries (needs fermionMeasurements)
    timeDisplacedPairing: bool = False        # ... and the pairing correlators P+-(r, tau_j) (needs timeDisplacedMeasurements)
    timeDisplacedParticleHole: bool = False   # ... and the charge / spin-z / SDW correlators C(r, tau_j) (needs timeDisplacedMeasurements)
    timeDisplacedCurrent: bool = False        # ... and the current-current correlators Lambda_xx/yy(r, tau_j) (needs timeDisplacedParticleHole)
    timeDisplacedEverySlice: bool = False     # ... every enabled channel also on every slice tau_k = k dtau, k = 0 .. m: the '...Fine' observables (needs timeDisplacedMeasurements)
    bandCorrelators: bool = False             # ... and the band-resolved charge channels bandDiff (n_x - n_y: nematic / d-wave CDW) and bandMix, time-displaced with
                                              #     timeDisplacedParticleHole, equal-time with equalTimeCorrelators (needs at least one of the two)
    timeDisplacedFineOnDevice: bool = False   # ... whose blocks then stay on the device: no '...Fine' observables, matsubara() reads them (needs timeDisplacedEverySlice)
    globalUpdateInterval: int = 100
    phi2bosons: bool = False
    cdwU: float = 0.0
    rngSeed: int = 1020304050
    simindex: int = 0
    device: int = 0
    stabilisation: str = "svd"   # "svd": UdV = SVD like the reference; "qr": pre-pivoted Householder UDT
    checkerboard: bool = True    # False = CB_NONE: dense B_k = e^{-dtau V_k} e^{-dtau K} (reference option checkerboard=false)
    spinProposalMethod: str = "box"      # "box", "rotate_then_scale", "rotate_and_scale" (the latter two: opdim = 3 only)
    adaptScaleVariance: bool = False
    repeatUpdateInSlice: int = 1
    # result-neutral execution choices (dqmc_tuning, include/dqmc_hip.h); 0 = automatic
    pipeline: int = 0            # 1 / -1: pipelined delayed updates on / off
    qrVariant: int = 0           # 1: Householder panels, 2: block Gram-Schmidt + Cholesky-QR2
    greenVariant: int = 0        # 1: QR instead of LU inside greenFromUdV
    maxJacobiSweeps: int = 0     # SVD mode: sweep budget of the Jacobi SVD (0 = 80)
    proposalBudget: int = 0      # proposals per delayed-update block (-1: no limit)
    decideThreads: int = 0       # threads per workgroup of the decision kernel (0: automatic, 256, 512); launch shape only
    bmultPath: int = 0           # checkerboard B-multiply kernel (0: automatic, 1: staged, 2: direct wherever it applies); same bits
    rngLookahead: int = 0        # the next sweep's uniforms are drawn and uploaded while the device sweeps (0: automatic = on, -1: off)


# The observables of the SDW host replica: name -> DETSDW_OBS_* index (include/detsdw_host.h).  What an index is -- shape, 'Fine' twin,
# Matsubara transform, series part -- is not restated here: the library's catalogue says it (describe_observable).  The matrices and pair
# operators a user sets are named 'custom{c}...' / 'customPair{c}...' (custom_observable, custom_pair_observable below)
OBSERVABLES = {"kOccX": 0, "kOccY": 1, "pairPlus": 2, "pairMinus": 3, "greenKTauX": 4, "greenKTauY": 5,
               "pairPlusTau": 6, "pairMinusTau": 7, "pairPlusTauQ0": 8, "pairMinusTauQ0": 9,
               "chargeTau": 10, "spinZTau": 11, "sdwTau": 12, "chargeTauQ0": 13, "spinZTauQ0": 14, "sdwTauQ0": 15,
               "currentXTau": 16, "currentYTau": 17, "currentXTauQ0": 18, "currentYTauQ0": 19, "bondKineticX": 20, "bondKineticY": 21,
               "chargeCorr": 22, "spinZCorr": 23, "sdwCorr": 24, "pairPlusCorr": 25, "pairMinusCorr": 26,
               "chargeSq": 27, "spinZSq": 28, "sdwSq": 29, "pairPlusSq": 30, "pairMinusSq": 31, "phiChi": 32, "phiScalars": 33,
               "bandDiffTau": 34, "bandMixTau": 35, "bandDiffTauQ0": 36, "bandMixTauQ0": 37,
               "bandDiffCorr": 38, "bandMixCorr": 39, "bandDiffSq": 40, "bandMixSq": 41, "greenMatrixTau": 74}
# views of the table: the fixed names with a Matsubara transform (DetSDW.matsubara); the equal-time correlators and structure factors
# (SDWParams.equalTimeCorrelators) and those of the band-resolved charge channels (bandCorrelators); the order-parameter part of a series
# opened with phi=True (real, (nfreq, N) and (5,)); 'greenMatrixTau' (and its 'Fine' twin)
MATSUBARA = {n: OBSERVABLES[n] for n in "greenKTauX greenKTauY pairPlusTau pairMinusTau chargeTau spinZTau sdwTau currentXTau currentYTau bandDiffTau bandMixTau".split()}
EQ_CORRELATORS = {n: OBSERVABLES[n] for n in "chargeCorr spinZCorr sdwCorr pairPlusCorr pairMinusCorr chargeSq spinZSq sdwSq pairPlusSq pairMinusSq".split()}
BAND_EQ_CORRELATORS = {n: OBSERVABLES[n] for n in "bandDiffCorr bandMixCorr bandDiffSq bandMixSq".split()}
SERIES_PHI_OBS = {n: OBSERVABLES[n] for n in "phiChi phiScalars".split()}
GREEN_MATRIX_OBS = OBSERVABLES["greenMatrixTau"]


def structure_factor(c, L):
    """S(q) = sum_d cos(q . d) C(d) of an equal-time correlator C over the periodic site differences (last axis, index dy L + dx):
    last axis of the result = qy L + qx, q = 2 pi (qx, qy) / L.  The sum the '...Sq' observables are formed with, for averages of
    '...Corr' a user keeps; leading axes are kept.  It serves any C(d) in this layout, the Hubbard replica's included:
    structure_factor(hub.observable_vector("spinZZCorr"), L)[(L // 2) * L + L // 2] is the antiferromagnetic S(pi, pi),
    1 - structure_factor(hub.observable_vector("greenUpCorr"), L) is n_up(k)."""
    c = np.asarray(c, dtype=np.float64)
    L = int(L)
    x = np.arange(L * L) % L
    y = np.arange(L * L) // L
    ph = 2.0 * np.pi / L * (np.outer(x, x) + np.outer(y, y))      # [q, d]
    return c @ np.cos(ph).T


def superfluid_stiffness(chi_xx, chi_yy, L):
    """rho_s = 1/8 Re [Lxx(qx=1, qy=0; 0) - Lxx(qx=0, qy=1; 0) + Lyy(qx=0, qy=1; 0) - Lyy(qx=1, qy=0; 0)] from
    chi_xx = matsubara('currentXTau', nfreq), chi_yy = matsubara('currentYTau', nfreq) (last two axes: frequency, q = qy L + qx):
    rho_s = 1/4 [Lambda_xx(q_x -> 0, q_y = 0) - Lambda_xx(q_x = 0, q_y -> 0)] at i omega = 0 and the smallest non-zero q, averaged over
    the two directions.  Leading axes (chains) are kept."""
    xx, yy = np.asarray(chi_xx)[..., 0, :], np.asarray(chi_yy)[..., 0, :]
    return 0.125 * np.real(xx[..., 1] - xx[..., L] + yy[..., L] - yy[..., 1])


# derived quantities of a measurement series (DetSDWBatch.series_derived_all): name -> index of detsdw_series_derived_all
SERIES_DERIVED = {"R_charge": 0, "R_spinZ": 1, "R_sdw": 2, "R_pairPlus": 3, "R_pairMinus": 4, "rhoS": 5,
                  "binderPhi": 6, "binderRatioPhi": 7, "chiPhi": 8, "chiPhiConnected": 9, "R_phi": 10, "xiPhi": 11,
                  "R_dCDW": 12, "R_nematic": 13, "R_bandMix": 14}
# parts of a kernel-level series (KernelContext.series_begin): bit 0 the equal-time block, bits 1 .. 4 the Matsubara transform of channel 0 .. 3,
# bit 6 (part index 6 of series_layout) the order-parameter part: chi_phi [nfreq][N] and five scalars from the field itself
SERIES_EQ, SERIES_MATS_G, SERIES_MATS_PAIR, SERIES_MATS_PH, SERIES_MATS_CURRENT = 1, 2, 4, 8, 16
SERIES_PHI = 64
# bit 7: the Matsubara transform of channel 4 (bandDiff, bandMix), bit 8: the equal-time band block, C_X(d) [2][N] then S_X(q) [2][N]
SERIES_MATS_BAND, SERIES_EQ_BAND = 128, 256
# bit 9: the Matsubara transform of channel 5 (one component per matrix of set_custom_bilinears), bit 10: their equal-time block,
# C(d) [count][N] then S(q) [count][N]
SERIES_MATS_CUSTOM, SERIES_EQ_CUSTOM = 512, 1024
# observables of the custom bilinears (DetSDWBatch.set_custom_bilinears), matrix c = 0 .. 3: 'custom{c}Tau', 'custom{c}TauQ0' (with
# 'Fine' twins), 'custom{c}Corr', 'custom{c}Sq' -> index base + c of detsdw_get_observable_vector
CUSTOM_OBS_BASE = {"Tau": 42, "TauQ0": 46, "Corr": 50, "Sq": 54}


def custom_observable(name):
    """(kind, index) of a custom-bilinear observable name, kind in CUSTOM_OBS_BASE; None for any other name"""
    m = re.fullmatch(r"custom([0-3])(Tau|TauQ0|Corr|Sq)", name)
    return (m.group(2), CUSTOM_OBS_BASE[m.group(2)] + int(m.group(1))) if m else None


def custom_ratio(name):
    """matrix index c of the derived series quantity 'R_custom{c}'; None for any other name"""
    m = re.fullmatch(r"R_custom([0-3])", name)
    return int(m.group(1)) if m else None


# bit 11: the Matsubara transform of channel 6 (one component per operator of set_custom_pair_operators), bit 12: their equal-time
# block, C(d) [count][N] then S(q) [count][N]
SERIES_MATS_CUSTOM_PAIR, SERIES_EQ_CUSTOM_PAIR = 2048, 4096
# observables of the custom pair operators (DetSDWBatch.set_custom_pair_operators), operator c = 0 .. 3: 'customPair{c}Tau',
# 'customPair{c}TauQ0' (with 'Fine' twins), 'customPair{c}Corr', 'customPair{c}Sq' -> index base + c of detsdw_get_observable_vector
CUSTOM_PAIR_OBS_BASE = {"Tau": 58, "TauQ0": 62, "Corr": 66, "Sq": 70}


def custom_pair_observable(name):
    """(kind, index) of a custom-pair observable name, kind in CUSTOM_PAIR_OBS_BASE; None for any other name"""
    m = re.fullmatch(r"customPair([0-3])(Tau|TauQ0|Corr|Sq)", name)
    return (m.group(2), CUSTOM_PAIR_OBS_BASE[m.group(2)] + int(m.group(1))) if m else None


def custom_pair_ratio(name):
    """operator index c of the derived series quantity 'R_customPair{c}'; None for any other name"""
    m = re.fullmatch(r"R_customPair([0-3])", name)
    return int(m.group(1)) if m else None


# bit 13: the normalised averaged Green's function of every slice (set_green_matrix), [m+1][N][R][R] complex
SERIES_GREEN_MATRIX = 8192
# the parts of a Hubbard context (part indices 14 .. 16): scalars and zcorr, the equal-time and the time-displaced correlators
SERIES_HUB_SCALARS, SERIES_HUB_EQ, SERIES_HUB_TD = 16384, 32768, 65536
# derived series quantities of the pair vertex (DetSDWBatch.series_derived_all): name prefix -> entry of detsdw_series_pair_vertex
PAIR_VERTEX_QUANTITIES = {"vertexCustomPair": 0, "bubbleCustomPair": 1, "gammaCustomPair": 2, "gammaBubbleCustomPair": 3}


def pair_vertex_quantity(name):
    """(entry, operator index c) of 'vertexCustomPair{c}' (P), 'bubbleCustomPair{c}' (Pbar), 'gammaCustomPair{c}' (Gamma = 1/P - 1/Pbar) or
    'gammaBubbleCustomPair{c}' (Gamma Pbar = Pbar/P - 1); None for any other name"""
    m = re.fullmatch(r"(vertexCustomPair|bubbleCustomPair|gammaCustomPair|gammaBubbleCustomPair)([0-3])", name)
    return (PAIR_VERTEX_QUANTITIES[m.group(1)], int(m.group(2))) if m else None


# ... of the particle-hole vertex of the custom bilinears: name prefix -> entry of detsdw_series_ph_vertex
PH_VERTEX_QUANTITIES = {"vertexCustom": 0, "bubbleCustom": 1, "gammaCustom": 2, "gammaBubbleCustom": 3, "disconnectedCustom": 4}


def ph_vertex_quantity(name):
    """(entry, matrix index c) of 'vertexCustom{c}' (chi = Re chi(Q, i omega_0) - D), 'bubbleCustom{c}' (chibar), 'gammaCustom{c}'
    (Gamma = 1/chi - 1/chibar), 'gammaBubbleCustom{c}' (Gamma chibar = chibar/chi - 1) or 'disconnectedCustom{c}' (D); None for any other name"""
    m = re.fullmatch(r"(vertexCustom|bubbleCustom|gammaCustom|gammaBubbleCustom|disconnectedCustom)([0-3])", name)
    return (PH_VERTEX_QUANTITIES[m.group(1)], int(m.group(2))) if m else None


def observable_index(name):
    """(index, detsdw_observable_desc) of a name of OBSERVABLES, 'custom{c}...', 'customPair{c}...' or one of those + 'Fine' where the
    observable has an every-slice twin; KeyError otherwise.  The descriptor is the library's catalogue entry of the index: no GPU"""
    fine = name.endswith("Fine")
    base = name[:-4] if fine else name
    cw = custom_observable(base) or custom_pair_observable(base)
    which = (cw[1] if cw else OBSERVABLES[base]) | (_lib.DETSDW_OBS_FINE if fine else 0)
    d = _lib.detsdw_observable_desc()
    if load().detsdw_describe_observable(which, C.byref(d)) != 0:
        raise KeyError(name)
    return which, d


def observable_shape(d, info, nfreq=0, series=False):
    """(shape, complex?) of one chain's values from the descriptor's kind: what observable_vector returns or, with series, what the series
    readers return -- the Matsubara transform in place of the tau rows, the stored flavour block of the Green matrix.  info: N, m, n, opdim"""
    K, N, R = _lib, info.N, 4 if info.opdim == 3 else 2
    rows = info.m + 1 if d.fine else info.n - 1
    shape = {K.DETSDW_OBS_KIND_SITE: (N,), K.DETSDW_OBS_KIND_CORR: (N,), K.DETSDW_OBS_KIND_SQ: (N,), K.DETSDW_OBS_KIND_TAU_Q0: (rows,),
             K.DETSDW_OBS_KIND_ROW_SCALAR: (rows,), K.DETSDW_OBS_KIND_PHI_CHI: (int(nfreq), N), K.DETSDW_OBS_KIND_PHI_SCALARS: (5,),
             K.DETSDW_OBS_KIND_TAU: (int(nfreq) if series else rows, N),
             K.DETSDW_OBS_KIND_GREEN_MATRIX: (info.m + 1, N, R, R) if series else (rows, N, 4, 4)}[d.kind]
    return shape, d.kind == K.DETSDW_OBS_KIND_GREEN_MATRIX or (series and d.kind == K.DETSDW_OBS_KIND_TAU)


def _matsubara_index(name):
    """index of detsdw_get_matsubara for a name of MATSUBARA, 'custom{c}Tau' or 'customPair{c}Tau'; KeyError otherwise"""
    which, d = observable_index(name)
    if not d.has_matsubara:
        raise KeyError(name)
    return which


def phi_sample(phi, L, nfreq):
    """The order-parameter part of a series sample in numpy, from a field phi (m+1, N, opdim) with slices 1 .. m (slice 0 is not read):
    (chi, scalars) with chi (nfreq, N), column qy L + qx,
        A_d(n, q) = (1/(m N)) sum_{k=1..m} sum_r phi_d(r, k) exp(i 2 pi n k / m - i 2 pi (qx x + qy y) / L),   chi(n, q) = sum_d |A_d(n, q)|^2
    (the physical susceptibility is beta N <chi>), and scalars = (|phibar|, |phibar|^2, |phibar|^4, the equal-time susceptibility
    (N/m) sum_k sum_d ((1/N) sum_r phi_d(r, k))^2, associatedEnergy = sum phi^2 / (2 N m)) with |phibar|^2 = chi(0, 0)."""
    phi = np.asarray(phi, dtype=np.float64)
    L, nfreq = int(L), int(nfreq)
    m, N, opdim = phi.shape[0] - 1, phi.shape[1], phi.shape[2]
    if N != L * L or not 1 <= nfreq <= m:
        raise ValueError("phi_sample needs phi of shape (m+1, L L, opdim) and 1 <= nfreq <= m")
    f = phi[1:]                                             # [k-1][r][d]
    k = np.arange(1, m + 1)
    et = np.exp(2j * np.pi * np.outer(np.arange(nfreq), k) / m)            # [n][k]
    j = np.arange(L)
    es = np.exp(-2j * np.pi * np.outer(j, j) / L)                          # [q][x]
    t = np.einsum("nk,kyxd->nyxd", et, f.reshape(m, L, L, opdim))
    a = np.einsum("qy,px,nyxd->nqpd", es, es, t) / (m * N)                 # [n][qy][qx][d]
    chi = (np.abs(a) ** 2).sum(axis=3).reshape(nfreq, N)
    m2 = chi[0, 0]
    eqt = ((f.sum(axis=1) / N) ** 2).sum() * N / m
    return chi, np.array([np.sqrt(m2), m2, m2 * m2, eqt, (f ** 2).sum() / (2.0 * N * m)])


def jackknife(bins, f=None):
    """Jackknife over the leading axis of `bins` (B >= 2 bin means x_b), the formulas of dqmc_series_stats_host / _derived_host:
    mean = (1/B) sum_b x_b, x_(b) = (B mean - x_b) / (B - 1).  f=None: returns (mean, err) with
    err = sqrt((B - 1)/B sum_b (x_(b) - mean)^2), element by element.  With a function f of one bin-shaped array: returns
    (f(mean), err) with err = sqrt((B - 1)/B sum_b (theta_(b) - mean_b theta_(b))^2), theta_(b) = f(x_(b))."""
    x = np.asarray(bins, dtype=np.float64)
    B = x.shape[0]
    if B < 2:
        raise ValueError("the jackknife needs at least two bins")
    mean = x.sum(axis=0) / B
    loo = (B * mean - x) / (B - 1)
    if f is None:
        return mean, np.sqrt((B - 1) / B * ((loo - mean) ** 2).sum(axis=0))
    theta = np.array([f(v) for v in loo])
    return f(mean), np.sqrt((B - 1) / B * ((theta - theta.sum(axis=0) / B) ** 2).sum(axis=0))


def binning_analysis(bins, bin_size, variance=None):
    """Binning analysis over the leading axis of `bins` (B closed bin means of bin_size sweeps each), the formulas of
    dqmc_series_binning_host: level l holds B_l = B >> l merged bins, y^0 = bins, y^l_k = (y^(l-1)_2k + y^(l-1)_(2k+1)) * 0.5 (bins beyond
    2^l B_l are not used), for every level with B_l >= 2.  Returns err [levels] + bins.shape[1:], the jackknife error of every level,
    or with variance = sigma^2 of the single samples (m2 / (samples - 1)) the pair (err, tau) with the integrated autocorrelation time
    tau_l = 1/2 err_l^2 (B_l 2^l bin_size) / sigma^2 in sweeps, NaN where sigma^2 is not > 0."""
    y = np.asarray(bins, dtype=np.float64)
    if y.shape[0] < 2:
        raise ValueError("the binning analysis needs at least two bins")
    errs, taus = [], []
    if variance is not None:
        var = np.asarray(variance, dtype=np.float64)
        safe = np.where(var > 0, var, 1.0)
    level = 0
    while y.shape[0] >= 2:
        errs.append(jackknife(y)[1])
        if variance is not None:
            t = 0.5 * errs[-1] * errs[-1] * (float(y.shape[0]) * float(1 << level) * float(bin_size)) / safe
            taus.append(np.where(var > 0, t, np.nan))
        half = y.shape[0] // 2
        y = (y[0:2 * half:2] + y[1:2 * half:2]) * 0.5
        level += 1
    return np.array(errs) if variance is None else (np.array(errs), np.array(taus))


# wrap-error diagnostics (dqmc_set_green_check): the doubles of one table row, in order (include/dqmc_hip.h)
GREEN_CHECK_FIELDS = ("count", "lastMaxAbs", "maxAbs", "sumMaxAbs", "maxSiteDiag", "sumMeanAbs", "maxRel", "argmax", "nonfinite",
                      "logScaleSpread", "logSvSpread")


def green_check_decode(raw, ng):
    """The tables of dqmc_green_check_read_host / detsdw_get_green_check, raw (chains, 2, n+1, 11), as a dict of arrays of shape
    (chains, 2, n+1): axis 1 is the sweep direction (0 down, 1 up), axis 2 the storage index j the advance landed on (boundary
    tau = j s).  count; lastMaxAbs, maxAbs (running maximum), meanMaxAbs (mean over the samples) of max |G_wrapped - G_rebuilt|;
    maxSiteDiag, the maximum over the entries local observables read (row mod N == col mod N); meanAbs, the mean over the samples of the
    mean difference; maxRel = maxAbs / max |G_rebuilt|; argmax (..., 2) = (row, col) of the entry behind maxAbs; nonfinite, the entries
    that were inf or NaN (maxAbs is inf then); logScaleSpread = log(max d / min d) of the stored factorisation; logSvSpread = log of the
    condition number of G^-1 (SVD stabilisation; 0 with QR).  Means are 0 in rows without a sample"""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 4 or raw.shape[1] != 2 or raw.shape[3] != len(GREEN_CHECK_FIELDS):
        raise ValueError("green_check_decode: expected shape (chains, 2, n+1, %d), got %r" % (len(GREEN_CHECK_FIELDS), raw.shape))
    f = {name: raw[..., i] for i, name in enumerate(GREEN_CHECK_FIELDS)}
    count = f["count"].astype(np.int64)
    denom = np.maximum(count, 1)
    idx = f["argmax"].astype(np.int64)
    return {"count": count, "lastMaxAbs": f["lastMaxAbs"].copy(), "maxAbs": f["maxAbs"].copy(), "meanMaxAbs": f["sumMaxAbs"] / denom,
            "maxSiteDiag": f["maxSiteDiag"].copy(), "meanAbs": f["sumMeanAbs"] / denom, "maxRel": f["maxRel"].copy(),
            "argmax": np.stack([idx % ng, idx // ng], axis=-1), "nonfinite": f["nonfinite"].astype(np.int64),
            "logScaleSpread": f["logScaleSpread"].copy(), "logSvSpread": f["logSvSpread"].copy()}


def green_check_worst(decoded):
    """per chain (maxAbs, dir, boundary, row, col) of the largest maxAbs of green_check_decode's result (the first row in (dir, boundary)
    order on ties); dir 0: down sweep, 1: up sweep; a NaN-free inf (non-finite entries) wins"""
    out = []
    for mx, am in zip(decoded["maxAbs"], decoded["argmax"]):
        d, j = np.unravel_index(int(np.argmax(mx)), mx.shape)
        out.append((float(mx[d, j]), int(d), int(j), int(am[d, j, 0]), int(am[d, j, 1])))
    return out


class _GreenCheck:
    """set_green_check / green_check / green_check_worst / green_check_reset of a host-layer handle; the class names its three C entry
    points and the error channel in _gc_calls and answers _gc_shape() = (chains, n, n_g)"""

    def _gc_handle(self):
        return self.h

    def set_green_check(self, on=True):
        """wrap-error diagnostics: while on, every stabilisation boundary compares the Green's function carried by wraps and updates with
        the one rebuilt from the UdV factors, on the device (green_check()).  The sweeps then take no shortcut at segment ends -- n more
        wraps and flushes per sweep, a copy of G and the compare -- and the Markov chain keeps its bits.  Between sweeps"""
        check(getattr(self.lib, self._gc_calls[0])(self._gc_handle(), int(on)), host=self._gc_calls[3])

    def _green_check_raw(self):
        chains, n, _ = self._gc_shape()
        raw = np.zeros((chains, 2, n + 1, len(GREEN_CHECK_FIELDS)))
        check(getattr(self.lib, self._gc_calls[1])(self._gc_handle(), raw.ctypes.data_as(_lib._DP)), host=self._gc_calls[3])
        return raw

    def green_check(self):
        """dict of arrays (chains, 2, n+1) (see green_check_decode); raises while the switch is off"""
        return green_check_decode(self._green_check_raw(), self._gc_shape()[2])

    def green_check_worst(self):
        """per chain (maxAbs, dir, boundary, row, col) of the worst boundary so far (green_check_worst)"""
        return green_check_worst(self.green_check())

    def green_check_reset(self):
        """clears the tables; the switch stays on"""
        check(getattr(self.lib, self._gc_calls[2])(self._gc_handle()), host=self._gc_calls[3])


SPIN_PROPOSAL = {"box": 0, "rotate_then_scale": 1, "rotate_and_scale": 2}
PROPOSE = {"box": 0, "rotate": 1, "scale": 2, "rotate_and_scale": 3}
ADAPT = {"box": 0, "rotate": 1, "scale": 2}


def _tuning(pipeline=0, qrVariant=0, greenVariant=0, maxJacobiSweeps=0, proposalBudget=0, decideThreads=0, bmultPath=0, rngLookahead=0):
    if int(rngLookahead) not in (0, -1):
        raise ValueError("rngLookahead must be 0 (automatic: on) or -1 (off)")
    # dqmc_tuning has no free slot: the look-ahead switch travels as a flag bit of bmult_path (include/dqmc_hip.h)
    path = int(bmultPath) | (_lib.DQMC_TUNING_NO_RNG_LOOKAHEAD if int(rngLookahead) == -1 and 0 <= int(bmultPath) <= 2 else 0)
    return _lib.dqmc_tuning(pipeline=int(pipeline), qr_variant=int(qrVariant), green_variant=int(greenVariant),
                            max_jacobi_sweeps=int(maxJacobiSweeps), proposal_budget=int(proposalBudget),
                            decide_threads=int(decideThreads), bmult_path=path)


def _fmat(a):
    """complex128, column-major, owned."""
    return np.array(a, dtype=np.complex128, order="F", copy=True)


def _custom_matrices(mats):
    """the argument of set_custom_bilinears as one C-contiguous complex array (count, 4, 4); the library validates the entries"""
    return np.ascontiguousarray(np.asarray(list(mats), dtype=np.complex128).reshape(-1, 4, 4))


def _custom_bond_operators(ops):
    """the argument of set_custom_bond_bilinears, a list of (M0, Mx, My) with None for a zero matrix, as three C-contiguous complex
    arrays (count, 4, 4); the library validates the entries"""
    ops = [tuple(op) for op in ops]
    if any(len(op) != 3 for op in ops):
        raise ValueError("every operator is a tuple (M0, Mx, My); None stands for a zero matrix")
    zero = np.zeros((4, 4), dtype=np.complex128)
    return [_custom_matrices([zero if op[k] is None else op[k] for op in ops]) for k in range(3)]


def _get_custom_bond(call, handle, host):
    n = C.c_int(0)
    m = [np.zeros((_lib.DQMC_CUSTOM_MAX, 4, 4), dtype=np.complex128) for _ in range(3)]
    check(call(handle, C.byref(n), *[a.ctypes.data for a in m]), host=host)
    return [tuple(a[c].copy() for a in m) for c in range(n.value)]


def _bond_tuple(params, mu, factor):
    """(None, Mx, My) with factor * diag(-t) of the flavours' bands on the bond of direction mu (0 / 'x' or 1 / 'y')"""
    mu = {"x": 0, "y": 1}.get(mu, mu)
    if mu not in (0, 1):
        raise ValueError("mu must be 'x' or 'y' (0 or 1)")
    hop = ((params.txhor, params.tyhor), (params.txver, params.tyver))[mu]        # band x, band y
    M = factor * np.diag([-hop[0], -hop[1], -hop[0], -hop[1]]).astype(np.complex128)      # XUP, YDOWN, XDOWN, YUP
    return (None, M, None) if mu == 0 else (None, None, M)


def bond_current(params, mu):
    """the (M0, Mx, My) tuple of the current operator j_mu of measure_timedisplaced_current for set_custom_bond_bilinears:
    M_mu = diag(i T), T = -t of the flavour's band in direction mu; the link factor (boundary sign, Peierls phase) is supplied by the
    library.  params: anything with txhor, txver, tyhor, tyver (SDWParams, dqmc_params)"""
    return _bond_tuple(params, mu, 1j)


def bond_kinetic(params, mu):
    """the same for the bond kinetic energy k_mu: M_mu = diag(T)"""
    return _bond_tuple(params, mu, 1.0)


def pair_operator(kind):
    """the (F0, Fx, Fy) tuple of a common pairing channel for set_custom_pair_operators (band-spin order XUP, YDOWN, XDOWN, YUP).  With S
    the singlet matrix, S[XUP, XDOWN] = S[YUP, YDOWN] = 1, S[XDOWN, XUP] = S[YDOWN, YUP] = -1:
        's'       F0[XUP, XDOWN] = F0[YUP, YDOWN] = 1: the operator of pairPlus (4 C(d) = pairPlus)
        'd_band'  F0[XUP, XDOWN] = 1, F0[YUP, YDOWN] = -1: the operator of pairMinus
        's_ext'   Fx = Fy = S: extended s on the bonds
        'd_bond'  Fx = S, Fy = -S: bond d-wave
    The bond operators use the bonds A -> A + x and A -> A + y only, so they are bond-centred: their q = 0 sums equal those of the
    four-bond operator up to a constant factor."""
    XUP, YDOWN, XDOWN, YUP = 0, 1, 2, 3
    F = np.zeros((4, 4), dtype=np.complex128)
    if kind in ("s", "d_band"):
        F[XUP, XDOWN], F[YUP, YDOWN] = 1.0, 1.0 if kind == "s" else -1.0
        return (F, None, None)
    if kind in ("s_ext", "d_bond"):
        F[XUP, XDOWN] = F[YUP, YDOWN] = 1.0
        F[XDOWN, XUP] = F[YDOWN, YUP] = -1.0
        return (None, F, F.copy() if kind == "s_ext" else -F)
    raise ValueError("kind must be 's', 'd_band', 's_ext' or 'd_bond'")


def pair_bubble(gbar, ops, L, bc="pbc"):
    """The pairing bubble Pbar_c(d) of the pair operators `ops` (a list of (F0, Fx, Fy), see pair_operator) on an averaged Green's
    function: the numpy counterpart of the device's bubble kernel, for users who want another function of the series bins.
    gbar: complex (..., N, R, R), the normalised block of set_green_matrix, gbar[..., dy L + dx, r, c] = Gbar_rc(d) / (N count), R = 2 (the
    (XUP, YDOWN) sector of O(1) / O(2)) or 4; leading axes (bins, time slices) are carried along.  The full matrix is
    g(P r; Q c) = sigma(Q, P - Q) gbar_rc(P - Q), sigma = -1 for each antiperiodic direction of bc ('pbc', 'apbc-x', 'apbc-y', 'apbc-xy') in
    which Q + (P - Q) wraps; the (XDOWN, YUP) sector of R = 2 is the complex conjugate.  Returns the real array (..., count, N),
        Pbar_c(d) = Re sum_ijkl D^d_ij conj(D^0_kl) [g(i; k) g(j; l) - g(i; l) g(j; k)],
    D^A the dense operator with the site blocks (A, A) = F0, (A + mu, A) = u_mu(A) Fmu; g is translation-covariant, so the site pair
    (B + d, B) is taken at B = 0."""
    g = np.asarray(gbar, dtype=np.complex128)
    N, R = L * L, g.shape[-1]
    if bc not in ("pbc", "apbc-x", "apbc-y", "apbc-xy") or g.shape[-3:] != (N, R, R) or R not in (2, 4):
        raise ValueError("gbar must be (..., L L, R, R) with R = 2 or 4, bc one of 'pbc', 'apbc-x', 'apbc-y', 'apbc-xy'")
    apb = (bc in ("apbc-x", "apbc-xy"), bc in ("apbc-y", "apbc-xy"))
    if R == 2:
        full = np.zeros(g.shape[:-2] + (4, 4), dtype=np.complex128)
        full[..., :2, :2] = g
        full[..., 2:, 2:] = np.conj(g)
        g = full
    ax, ay = np.arange(N) % L, np.arange(N) // L
    zero = np.zeros((4, 4), dtype=np.complex128)

    def block(px, py, qx, qy):
        """g(P .; Q .) for the site arrays P and the one site Q: (..., N, 4, 4)"""
        dx, dy = (px - qx) % L, (py - qy) % L
        sg = np.where(apb[0] & (qx + dx >= L), -1.0, 1.0) * np.where(apb[1] & (qy + dy >= L), -1.0, 1.0)
        return sg[:, None, None] * g[..., dy * L + dx, :, :]

    # site blocks k = 0, x, y of the operator at A = d (all d at once) and at B = 0, with their link signs
    PA = [(ax, ay, np.ones(N)), ((ax + 1) % L, ay, np.where(apb[0] & (ax == L - 1), -1.0, 1.0)), (ax, (ay + 1) % L, np.where(apb[1] & (ay == L - 1), -1.0, 1.0))]
    QB = [(0, 0), (1 % L, 0), (0, 1 % L)]
    out = []
    for op in ops:
        F = [zero if m is None else np.asarray(m, dtype=np.complex128) for m in op]
        acc = np.zeros(g.shape[:-3] + (N,))
        for ka in range(3):
            if not F[ka].any():
                continue
            px, py, ua = PA[ka]
            for kb in range(3):
                if not F[kb].any():
                    continue
                qx, qy = QB[kb]
                direct = np.einsum("ab,cd,...ac,...bd->...", F[ka], np.conj(F[kb]), block(px, py, qx, qy), block(ax, ay, 0, 0), optimize=True)
                exchange = np.einsum("ab,cd,...ad,...bc->...", F[ka], np.conj(F[kb]), block(px, py, 0, 0), block(ax, ay, qx, qy), optimize=True)
                acc = acc + ua * (direct - exchange).real
        out.append(acc)
    return np.stack(out, axis=-2) if out else np.zeros(g.shape[:-3] + (0, N))


def _ph_full(gbar, L, bc, lead):
    """(full 4 x 4 blocks (..., N, 4, 4), antiperiodic flags) of a normalised block of set_green_matrix with at least `lead` leading axes"""
    g = np.asarray(gbar, dtype=np.complex128)
    N, R = L * L, g.shape[-1]
    if bc not in ("pbc", "apbc-x", "apbc-y", "apbc-xy") or g.ndim < 3 + lead or g.shape[-3:] != (N, R, R) or R not in (2, 4):
        raise ValueError("gbar must be (..., L L, R, R) with R = 2 or 4, bc one of 'pbc', 'apbc-x', 'apbc-y', 'apbc-xy'")
    if R == 2:
        full = np.zeros(g.shape[:-2] + (4, 4), dtype=np.complex128)
        full[..., :2, :2] = g
        full[..., 2:, 2:] = np.conj(g)
        g = full
    return g, (bc in ("apbc-x", "apbc-xy"), bc in ("apbc-y", "apbc-xy"))


def _ph_block(g, L, apb, P, Q):
    """g(P .; Q .) = sigma(Q, P - Q) g[..., P - Q, :, :] for site coordinate arrays P = (px, py), Q = (qx, qy) of one length: (..., n, 4, 4)"""
    dx, dy = (P[0] - Q[0]) % L, (P[1] - Q[1]) % L
    sg = np.where(apb[0] & (Q[0] + dx >= L), -1.0, 1.0) * np.where(apb[1] & (Q[1] + dy >= L), -1.0, 1.0)
    return sg[:, None, None] * g[..., dy * L + dx, :, :]


def _ph_stencil(op, L, apb, sx, sy):
    """the five site blocks V_k(S) = f_k(S) W_k of the operator (M0, Mx, My) at the sites S = (sx, sy) (arrays): a list of
    (W_k, p, q, f_k) with W = M0, Mx, Mx^H, My, My^H, p the site of c^+, q that of c, f_k = +-1 the link sign; zero blocks are left out"""
    zero = np.zeros((4, 4), dtype=np.complex128)
    M0, Mx, My = (zero if m is None else np.asarray(m, dtype=np.complex128) for m in op)
    S, Sx, Sy = (sx, sy), ((sx + 1) % L, sy), (sx, (sy + 1) % L)
    ux, uy = np.where(apb[0] & (sx == L - 1), -1.0, 1.0), np.where(apb[1] & (sy == L - 1), -1.0, 1.0)
    blocks = [(M0, S, S, np.ones(len(sx))), (Mx, Sx, S, ux), (Mx.conj().T, S, Sx, ux), (My, Sy, S, uy), (My.conj().T, S, Sy, uy)]
    return [b for b in blocks if b[0].any()]


def ph_bubble(gbar, ops, L, bc="pbc"):
    """The particle-hole bubble chibar_c(d, tau_k) of the bilinears `ops` (a list of (M0, Mx, My) as set_custom_bond_bilinears takes them; an
    on-site matrix M is (M, None, None)) on an averaged Green's function: the numpy counterpart of the device's bubble kernel.
    gbar: complex (..., m+1, N, R, R), all rows k = 0 .. m of the normalised block of set_green_matrix (see pair_bubble for the block, the
    sign sigma and the sectors); leading axes (bins) are carried along.  With gbar(0, tau_k) = -gbar(tau_{m-k}, 0) -- the cyclic invariance
    of the weight -- returns the real array (..., m+1, count, N),
        chibar_c(d, tau_k) = -sum_{k, k'} Re f_k(A) f_k'(B) tr(W_k gbar(tau_k,0)(A^q; B^r) W_k' gbar(0,tau_k)(B^s; A^p)),   (A, B) = (d, 0),
    the connected Wick term of <O_A(tau_k) O_B(0)> over the five site blocks V_k = f_k W_k of each operator (W = M0, Mx, Mx^H, My, My^H
    between the sites (p, q) = (A, A), (A + x, A), (A, A + x), (A + y, A), (A, A + y), f_k the link sign)."""
    g, apb = _ph_full(gbar, L, bc, 1)
    N = L * L
    gt = -np.flip(g, axis=-4)                               # gbar(0, tau_k)
    ax, ay = np.arange(N) % L, np.arange(N) // L
    zx = np.zeros(N, dtype=int)
    out = []
    for op in ops:
        acc = np.zeros(g.shape[:-3] + (N,))
        for WA, pA, qA, fA in _ph_stencil(op, L, apb, ax, ay):
            for WB, rB, sB, fB in _ph_stencil(op, L, apb, zx, zx):
                tr = np.einsum("ab,...bc,cd,...da->...", WA, _ph_block(g, L, apb, qA, rB), WB, _ph_block(gt, L, apb, sB, pA), optimize=True)
                acc = acc - fA * fB * tr.real
        out.append(acc)
    return np.stack(out, axis=-2) if out else np.zeros(g.shape[:-3] + (0, N))


def ph_one_body(gbar0, ops, L, bc="pbc"):
    """The one-body value obar_c = tr M0 - sum_ij (O_0)_ij gbar(tau_0,0)(j; i) of the bilinears `ops` at site 0 (it does not depend on the
    site for a translation-covariant matrix).  gbar0: complex (..., N, R, R), row 0 of the block ph_bubble takes.  Returns complex
    (..., count); the disconnected part of chi_c(Q = 0, i omega_0) is beta N Re(obar_c^2)."""
    g, apb = _ph_full(gbar0, L, bc, 0)
    z = np.zeros(1, dtype=int)
    out = []
    for op in ops:
        M0 = np.zeros((4, 4), dtype=np.complex128) if op[0] is None else np.asarray(op[0], dtype=np.complex128)
        acc = np.trace(M0) + np.zeros(g.shape[:-3], dtype=np.complex128)
        for W, p, q, f in _ph_stencil(op, L, apb, z, z):
            acc = acc - f[0] * np.einsum("ab,...ba->...", W, _ph_block(g, L, apb, q, p)[..., 0, :, :])
        out.append(acc)
    return np.stack(out, axis=-1) if out else np.zeros(g.shape[:-3] + (0,), dtype=np.complex128)


class KernelContext:
    """One dqmc_ctx.  Needs a GPU."""

    def __init__(self, opdim, L, m, s, dtau, delaySteps=16, bc="pbc", weakZflux=False, r=-1.0, c=3.0, u=1.0,
                 lambda_=1.0, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0, mux=-0.5, muy=-0.5,
                 accRatio=0.5, phi2bosons=False, device=0, stabilisation="svd", checkerboard=True, nchains=1, cdwU=0.0,
                 pipeline=0, qrVariant=0, greenVariant=0, maxJacobiSweeps=0, proposalBudget=0, rngWindowPerSite=0, decideThreads=0, bmultPath=0,
                 rngLookahead=0, timeDisplaced=False, tdParticleHole=False, tdCurrent=False, tdEverySlice=False, tdBand=False):
        self.lib = load()
        p = _lib.dqmc_params(opdim=opdim, L=L, m=m, s=s, delaySteps=delaySteps, bc=BC[bc],
                             weakZflux=int(weakZflux), phi2bosons=int(phi2bosons), device=device,
                             stabilisation=STABILISATION[stabilisation], cb_none=int(not checkerboard), dtau=dtau, r=r, c=c, u=u, lambda_=lambda_, txhor=txhor, txver=txver,
                             tyhor=tyhor, tyver=tyver, mux=mux, muy=muy, accRatio=accRatio, cdwU=cdwU, rng_window_per_site=int(rngWindowPerSite),
                             timedisplaced=int(timeDisplaced) | (_lib.DQMC_TD_EVERY_SLICE if tdEverySlice else 0), td_particle_hole=(2 if tdCurrent else int(tdParticleHole)) | (_lib.DQMC_TD_PH_BAND if tdBand else 0),
                             tuning=_tuning(pipeline, qrVariant, greenVariant, maxJacobiSweeps, proposalBudget, decideThreads, bmultPath, rngLookahead))
        h = C.c_void_p()
        check(self.lib.dqmc_create_batch(C.byref(p), nchains, C.byref(h)))
        self.h = h
        self.nchains = nchains
        self.opdim, self.L, self.m, self.s = opdim, L, m, s
        self.N = L * L
        self.MSF = 4 if opdim == 3 else 2
        self.ng = self.MSF * self.N
        self.n = -(-m // s)

    def close(self):
        if self.h:
            self.lib.dqmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shiftGreenSymmetric(self):
        g = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        check(self.lib.dqmc_shift_green_symmetric_host(self.h, g.ctypes.data))
        return g

    def set_timedisplaced(self, on=True):
        """while on, every advance that ends on an interior boundary also computes G(tau,0) and G(0,tau) (needs timeDisplaced=True
        at construction)"""
        check(self.lib.dqmc_set_timedisplaced(self.h, int(on)))

    def green_timedisplaced(self):
        """(slice, G(tau,0), G(0,tau)) of the last interior advance, selected chain"""
        gt0 = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        g0t = np.zeros_like(gt0)
        sl = C.c_int(-1)
        check(self.lib.dqmc_get_green_timedisplaced_host(self.h, gt0.ctypes.data, g0t.ctypes.data, C.byref(sl)))
        return sl.value, gt0, g0t

    def _read_block(self, size_fn, read_fn, *which):
        """one accumulator block of the selected chain through its (size, read) pair of entry points"""
        out = np.zeros(size_fn(self.h, *which))
        check(read_fn(self.h, *which, out.ctypes.data_as(_lib._DP)))
        return out

    def measure_reset(self):
        check(self.lib.dqmc_measure_reset(self.h))

    def measure_slice(self):
        """shiftGreenSymmetric of the current G and one sample added to every equal-time accumulator, all chains"""
        check(self.lib.dqmc_measure_slice(self.h))

    def measure_read(self):
        """the selected chain's accumulators: [greenK0, greenLocal, occDiffSq, count, pairPlus[N], pairMinus[N], S_X, S_Y]"""
        return self._read_block(self.lib.dqmc_measure_accum_size, self.lib.dqmc_measure_read_host)

    def set_equal_time_correlators(self, on=True):
        """while on, every measure_slice also bins the equal-time charge / spinZ / sdw / pairPlus / pairMinus sums of the same shifted
        matrix into a block of their own (SDW model only; the first enable allocates the block)"""
        check(self.lib.dqmc_set_equal_time_correlators(self.h, int(on)))

    def measure_eq_read(self):
        """the selected chain's equal-time block: [count, charge[N], spinZ[N], sdw[N], pairPlus[N], pairMinus[N]], raw sums over B of
        Re W(B (+) d, B), index dy L + dx; C(d) = sum / (count N)"""
        return self._read_block(self.lib.dqmc_measure_eq_accum_size, self.lib.dqmc_measure_eq_read_host)

    def set_equal_time_band(self, on=True):
        """while on, every measure_slice also bins the equal-time bandDiff / bandMix sums of the same shifted matrix into a block of their
        own (SDW model only; the first enable allocates the block; independent of set_equal_time_correlators)"""
        check(self.lib.dqmc_set_equal_time_band(self.h, int(on)))

    def measure_eq_band_read(self):
        """the selected chain's equal-time band block: [count, bandDiff[N], bandMix[N]], raw sums, index dy L + dx"""
        return self._read_block(self.lib.dqmc_measure_eq_band_accum_size, self.lib.dqmc_measure_eq_band_read_host)

    def hubbard_set_equal_time_correlators(self, on=True):
        """Hubbard model: while on, every measure_slice also bins the eight equal-time correlators of the slice's own G into a block of
        their own (the first enable allocates it)"""
        check(self.lib.dqmc_hubbard_set_equal_time_correlators(self.h, int(on)))

    def hubbard_eq_read(self):
        """the selected chain's block: [count, greenUp[N], greenDn[N], charge[N], spinZZ[N], spinXX[N], pairS[N], pairSx[N], pairD[N]],
        raw sums over B of X(B (+) d, B), index dy L + dx; C(d) = sum / (count N)"""
        return self._read_block(self.lib.dqmc_hubbard_eq_accum_size, self.lib.dqmc_hubbard_eq_read_host)

    def hubbard_measure_timedisplaced(self, j):
        """Hubbard model: the six time-displaced correlators of boundary j from G(tau,0), G(0,tau), G(tau), G(0) into their block (call it
        right after the advance that ended on boundary j, with set_timedisplaced on)"""
        check(self.lib.dqmc_hubbard_measure_timedisplaced(self.h, j))

    def hubbard_measure_timedisplaced_segment(self, j):
        """Hubbard model, context with DQMC_TD_HUB_EVERY_SLICE: all eight channels on every slice of boundary j's segment into the every-slice
        block, by propagation from the boundary's matrices (right after the advance that ended on boundary j)"""
        check(self.lib.dqmc_hubbard_measure_timedisplaced_segment(self.h, j))

    def hubbard_measure_timedisplaced_ends(self):
        """Hubbard model: rows 0 and m of the every-slice block from G = G(0) (the context must stand at time slice 0 or m)"""
        check(self.lib.dqmc_hubbard_measure_timedisplaced_ends(self.h))

    def hubbard_td_fine_read(self):
        """count[m+1], then [m+1][8][N] raw sums of the selected chain, the channel order of hubbard_eq_read"""
        return self._read_block(self.lib.dqmc_hubbard_td_fine_accum_size, self.lib.dqmc_hubbard_td_fine_read_host)

    def hubbard_td_matsubara(self, nfreq):
        """Matsubara transforms of the every-slice block, every chain and channel: complex (nchains, 8, nfreq, N); channels 0, 1 at the
        fermionic frequencies, 2 .. 7 at the bosonic ones"""
        out = np.zeros(self.lib.dqmc_hubbard_td_matsubara_size(self.h, nfreq))
        check(self.lib.dqmc_hubbard_td_matsubara_host(self.h, nfreq, out.ctypes.data_as(_lib._DP)))
        return out.view(np.complex128).reshape(self.nchains_total(), 8, nfreq, self.N)

    def hubbard_td_read(self):
        """count[n-1], then per boundary [greenUp, greenDn, charge, spinZZ, spinXX, pairS][N], raw sums"""
        return self._read_block(self.lib.dqmc_hubbard_td_accum_size, self.lib.dqmc_hubbard_td_read_host)

    def measure_timedisplaced(self, j):
        check(self.lib.dqmc_measure_timedisplaced(self.h, j))

    def measure_td_read(self):
        return self._read_block(self.lib.dqmc_measure_td_accum_size, self.lib.dqmc_measure_td_read_host)

    def measure_timedisplaced_pair(self, j):
        """pairing correlators of the last pair's shifted G(tau_j, 0) into their block (needs timeDisplaced=2 at construction)"""
        check(self.lib.dqmc_measure_timedisplaced_pair(self.h, j))

    def measure_td_pair_read(self):
        """count[n-1], then per boundary the N sums of Re T+ and the N sums of Re T- over the periodic site differences"""
        return self._read_block(self.lib.dqmc_measure_td_pair_accum_size, self.lib.dqmc_measure_td_pair_read_host)

    def green0_timedisplaced(self):
        """(slice, G(0)) of the last interior advance's own field configuration, selected chain (needs tdParticleHole=True)"""
        g00 = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        sl = C.c_int(-1)
        check(self.lib.dqmc_get_green0_timedisplaced_host(self.h, g00.ctypes.data, C.byref(sl)))
        return sl.value, g00

    def measure_timedisplaced_ph(self, j):
        """charge / spinZ / sdw correlators of boundary j from the four shifted Green's functions into their block (needs
        tdParticleHole=True at construction; call it right after the advance that ended on boundary j)"""
        check(self.lib.dqmc_measure_timedisplaced_ph(self.h, j))

    def measure_td_ph_read(self):
        """count[n-1], then per boundary the N sums of Re W over the periodic site differences for charge, spinZ and sdw"""
        return self._read_block(self.lib.dqmc_measure_td_ph_accum_size, self.lib.dqmc_measure_td_ph_read_host)

    def measure_timedisplaced_current(self, j):
        """current-current correlators and bond kinetic energy of boundary j into their block (needs tdCurrent=True at construction; call
        it right after the advance that ended on boundary j)"""
        check(self.lib.dqmc_measure_timedisplaced_current(self.h, j))

    def measure_td_current_read(self):
        """count[n-1], then per boundary the N sums of Re W[j_x, j_x], the N sums of Re W[j_y, j_y] over the periodic site differences and
        the two sums of Re o_tau[k_x], Re o_tau[k_y] over the sites"""
        return self._read_block(self.lib.dqmc_measure_td_current_accum_size, self.lib.dqmc_measure_td_current_read_host)

    def measure_timedisplaced_band(self, j):
        """bandDiff / bandMix correlators of boundary j from the four shifted Green's functions into their block (needs tdBand=True at
        construction; call it right after the advance that ended on boundary j)"""
        check(self.lib.dqmc_measure_timedisplaced_band(self.h, j))

    def measure_td_band_read(self):
        """count[n-1], then per boundary the N sums of Re W over the periodic site differences for bandDiff and bandMix"""
        return self._read_block(self.lib.dqmc_measure_td_band_accum_size, self.lib.dqmc_measure_td_band_read_host)

    def set_custom_bilinears(self, mats):
        """up to four Hermitian 4 x 4 matrices (band-spin order XUP, YDOWN, XDOWN, YUP) whose bilinears sum_ab c^+_a M_ab c_b are measured
        time-displaced (measure_timedisplaced_custom, needs tdParticleHole=True) and at equal time (set_equal_time_custom); an empty list
        removes them.  A second call replaces the matrices and clears their blocks"""
        m = _custom_matrices(mats)
        check(self.lib.dqmc_set_custom_bilinears(self.h, len(m), m.ctypes.data))

    def set_custom_bond_bilinears(self, ops):
        """up to four operators (M0, Mx, My): M0 Hermitian on the site, Mx / My arbitrary complex 4 x 4 on the bonds A -> A + x, A -> A + y
        (None: zero; the Hermitian conjugate and the bonds' link factors are added by the library), measured through the same entries and
        blocks as set_custom_bilinears, which they replace.  See bond_current / bond_kinetic"""
        m0, mx, my = _custom_bond_operators(ops)
        check(self.lib.dqmc_set_custom_bond_bilinears(self.h, len(m0), m0.ctypes.data, mx.ctypes.data, my.ctypes.data))

    def get_custom_bond_bilinears(self):
        """the operators that are set: a list of (M0, Mx, My), complex 4 x 4 each"""
        return _get_custom_bond(self.lib.dqmc_get_custom_bond_bilinears, self.h, False)

    def get_custom_bilinears(self):
        """the matrices that are set, complex (count, 4, 4)"""
        n = C.c_int(0)
        m = np.zeros((_lib.DQMC_CUSTOM_MAX, 4, 4), dtype=np.complex128)
        check(self.lib.dqmc_get_custom_bilinears(self.h, C.byref(n), m.ctypes.data))
        return m[:n.value].copy()

    def measure_timedisplaced_custom(self, j):
        """the correlators of every set matrix at boundary j, one launch, into their block (call it right after the advance that ended on
        boundary j)"""
        check(self.lib.dqmc_measure_timedisplaced_custom(self.h, j))

    def measure_td_custom_read(self):
        """count[n-1], then per boundary one row of N sums of Re W over the periodic site differences for every set matrix"""
        return self._read_block(self.lib.dqmc_measure_td_custom_accum_size, self.lib.dqmc_measure_td_custom_read_host)

    def set_equal_time_custom(self, on=True):
        """while on, every measure_slice also bins the equal-time sums of every set matrix into a block of their own (independent of the
        other two equal-time switches)"""
        check(self.lib.dqmc_set_equal_time_custom(self.h, int(on)))

    def measure_eq_custom_read(self):
        """the selected chain's equal-time block of the set matrices: [count, one row of N raw sums per matrix], index dy L + dx"""
        return self._read_block(self.lib.dqmc_measure_eq_custom_accum_size, self.lib.dqmc_measure_eq_custom_read_host)

    def set_custom_pair_operators(self, ops):
        """up to four pair operators (F0, Fx, Fy), complex 4 x 4 each, None for a zero matrix:
        Delta_A = sum_ab F0_ab c_(A a) c_(A b) + sum_mu u_mu(A) sum_ab Fmu_ab c_(A + mu, a) c_(A b); <Delta_A(tau) Delta_B^+(0)> is measured
        time-displaced (measure_timedisplaced_custom_pair, needs timeDisplaced >= 1) and at equal time (set_equal_time_custom_pair).  An
        empty list removes them; independent of set_custom_bilinears.  See pair_operator"""
        f0, fx, fy = _custom_bond_operators(ops)
        check(self.lib.dqmc_set_custom_pair_operators(self.h, len(f0), f0.ctypes.data, fx.ctypes.data, fy.ctypes.data))

    def get_custom_pair_operators(self):
        """the pair operators that are set: a list of (F0, Fx, Fy), complex 4 x 4 each"""
        return _get_custom_bond(self.lib.dqmc_get_custom_pair_operators, self.h, False)

    def measure_timedisplaced_custom_pair(self, j):
        """the pair correlators of every set operator at boundary j, one launch, into their block"""
        check(self.lib.dqmc_measure_timedisplaced_custom_pair(self.h, j))

    def measure_td_custom_pair_read(self):
        """count[n-1], then per boundary one row of N sums of Re P over the periodic site differences for every set pair operator"""
        return self._read_block(self.lib.dqmc_measure_td_custom_pair_accum_size, self.lib.dqmc_measure_td_custom_pair_read_host)

    def set_equal_time_custom_pair(self, on=True):
        """while on, every measure_slice also bins the equal-time sums of every set pair operator into a block of their own (independent
        of the other three equal-time switches)"""
        check(self.lib.dqmc_set_equal_time_custom_pair(self.h, int(on)))

    def measure_eq_custom_pair_read(self):
        """the selected chain's equal-time block of the set pair operators: [count, one row of N raw sums per operator], index dy L + dx"""
        return self._read_block(self.lib.dqmc_measure_eq_custom_pair_accum_size, self.lib.dqmc_measure_eq_custom_pair_read_host)

    def set_green_matrix(self, on=True):
        """while on, every time-displaced row also bins Gbar_rc(d) = sum_B sigma(B, d) g~((B + d) r; B c) of the shifted G(tau,0) into
        a block of its own (coarse rows by measure_timedisplaced_green_matrix, every-slice channel 7): the input of the pairing bubble
        (series_pair_vertex, pair_bubble).  Needs timeDisplaced >= 1; refused under weakZflux"""
        check(self.lib.dqmc_set_green_matrix(self.h, int(on)))

    def set_green_check(self, on=True):
        """wrap-error diagnostics: while on, every advance that finds G fresh keeps it and compares it with the rebuilt one on the device
        (all chains, no host synchronisation), one sample into row [dir][j] of green_check()"""
        check(self.lib.dqmc_set_green_check(self.h, int(on)))

    def green_check_raw(self):
        """the tables of all chains, (nchains, 2, n+1, 11) doubles (include/dqmc_hip.h); raises while the switch is off"""
        raw = np.zeros((self.lib.dqmc_num_chains(self.h), 2, self.n + 1, len(GREEN_CHECK_FIELDS)))
        if self.lib.dqmc_green_check_size(self.h) not in (0, raw[0].size):
            raise RuntimeError("dqmc_green_check_size disagrees with the table layout")
        check(self.lib.dqmc_green_check_read_host(self.h, raw.ctypes.data_as(_lib._DP)))
        return raw

    def green_check(self):
        return green_check_decode(self.green_check_raw(), self.ng)

    def green_check_reset(self):
        check(self.lib.dqmc_green_check_reset(self.h))

    def measure_timedisplaced_green_matrix(self, j):
        """the averaged Green's function block at boundary j, one launch"""
        check(self.lib.dqmc_measure_timedisplaced_green_matrix(self.h, j))

    def measure_td_green_matrix_read(self):
        """count[n-1], then per boundary one row [N][R][R] of raw sums as (re, im); bin dy L + dx"""
        return self._read_block(self.lib.dqmc_measure_td_green_matrix_accum_size, self.lib.dqmc_measure_td_green_matrix_read_host)

    def measure_timedisplaced_segment(self, j):
        """every slice of boundary j's segment into the fine blocks, by propagation from the boundary's matrices (needs tdEverySlice=True at
        construction; call it right after the advance that ended on boundary j)"""
        check(self.lib.dqmc_measure_timedisplaced_segment(self.h, j))

    def measure_timedisplaced_ends(self):
        """rows 0 and m of the fine blocks from G = G(0) (the context must stand at time slice 0 or m)"""
        check(self.lib.dqmc_measure_timedisplaced_ends(self.h))

    def measure_td_fine_read(self, channel):
        """fine block of channel 0 (G(k, tau) bins), 1 (pairing), 2 (particle-hole), 3 (current), 4 (band), 5 (custom bilinears), 6 (custom pair
        operators), 7 (the averaged Green's function): count[m+1], then rows k = 0 .. m"""
        return self._read_block(self.lib.dqmc_measure_td_fine_accum_size, self.lib.dqmc_measure_td_fine_read_host, channel)

    def measure_td_matsubara(self, channel, nfreq):
        """Matsubara transforms of the fine block of `channel`, every chain and component: complex (nchains, components, nfreq, N)"""
        out = np.zeros(self.lib.dqmc_measure_td_matsubara_size(self.h, channel, nfreq))
        check(self.lib.dqmc_measure_td_matsubara_host(self.h, channel, nfreq, out.ctypes.data_as(_lib._DP)))
        return out.view(np.complex128).reshape(self.nchains_total(), -1, nfreq, self.N)     # 3 components for channel 2, one per matrix for 5

    def series_begin(self, bin_size, max_bins, nfreq=0, parts=SERIES_EQ):
        """open the measurement series of this context: bins of bin_size samples, at most max_bins of them; parts = SERIES_EQ |
        SERIES_MATS_G | ... (the equal-time block must have been enabled, the Matsubara parts need their every-slice block) | SERIES_PHI
        (the order-parameter part: needs no block, 1 <= nfreq <= m; it may be the only part)"""
        check(self.lib.dqmc_series_begin(self.h, int(bin_size), int(max_bins), int(nfreq), int(parts)))

    def series_add_sweep(self):
        """one sample of every chain from the blocks as they stand, added to the open bin"""
        check(self.lib.dqmc_series_add_sweep(self.h))

    def series_form_sample(self):
        """the first half of series_add_sweep: the sample of every chain into the sample buffer; moves no counter, touches no bin"""
        check(self.lib.dqmc_series_form_sample(self.h))

    def series_sample_device(self):
        """(device address of the sample buffer [nchains][S], S): chain b at address + 8 b S; valid while the series is open"""
        rows, s = C.c_void_p(0), C.c_size_t(0)
        check(self.lib.dqmc_series_sample_device(self.h, C.byref(rows), C.byref(s)))
        return rows.value, s.value

    def series_accumulate(self, ptrs=None):
        """the second half: slot s adds the S doubles at device address ptrs[s] (one per chain of this context; rows of any context of the
        same device whose sample is formed) to its open bin; None: the context's own rows in order"""
        if ptrs is None:
            check(self.lib.dqmc_series_accumulate(self.h, None))
            return
        ptrs = [int(p) if p else None for p in ptrs]
        if len(ptrs) != self.nchains_total():
            raise ValueError("series_accumulate needs one pointer per chain of the context")
        check(self.lib.dqmc_series_accumulate(self.h, (C.c_void_p * len(ptrs))(*ptrs)))

    def series_info(self):
        """(bins closed, samples in the open bin, doubles per sample S)"""
        a, b, s = C.c_int(0), C.c_int(0), C.c_size_t(0)
        check(self.lib.dqmc_series_info(self.h, C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def series_layout(self, part):
        """(offset, length) of part 0 (equal-time: C_X(d) [5][N], S_X(q) [5][N]), 1 + channel (Matsubara, [component][nfreq][N] (re, im)), 6
        (order parameter; 14 .. 16: a Hubbard context's scalars + zcorr, C_X(d) / S_X(q) [8][N] each, C_X(d, tau_j) / S_X(q, tau_j) [n-1][6][N]
        each), 7 (Matsubara of the band channel), 8 (equal-time band: C_X(d) [2][N], S_X(q) [2][N]), 9 (Matsubara of the custom
        bilinears), 10 (their equal-time block: C(d) [count][N], S(q) [count][N]), 11 and 12 (the same two of the custom pair operators)"""
        off, ln = C.c_size_t(0), C.c_size_t(0)
        check(self.lib.dqmc_series_layout(self.h, int(part), C.byref(off), C.byref(ln)))
        return off.value, ln.value

    def series_bins(self, first=0, count=None):
        """closed bins first .. first + count - 1 (default: all from first) of the selected chain: (count, S)"""
        closed, _, S = self.series_info()
        count = closed - first if count is None else int(count)
        out = np.zeros((max(count, 0), S))
        check(self.lib.dqmc_series_read_bins_host(self.h, int(first), count, out.ctypes.data_as(_lib._DP)))
        return out

    def series_stats(self):
        """(mean, err) of every element over the closed bins, jackknife, all chains: (nchains, S) each"""
        S = self.series_info()[2]
        mean, err = np.zeros((self.nchains_total(), S)), np.zeros((self.nchains_total(), S))
        check(self.lib.dqmc_series_stats_host(self.h, mean.ctypes.data_as(_lib._DP), err.ctypes.data_as(_lib._DP)))
        return mean, err

    def series_derived(self):
        """(value, err), (nchains, 6) each: the correlation ratios R_charge, R_spinZ, R_sdw, R_pairPlus, R_pairMinus and rho_s; NaN where
        the part is not in the series"""
        v, e = np.zeros((self.nchains_total(), 6)), np.zeros((self.nchains_total(), 6))
        check(self.lib.dqmc_series_derived_host(self.h, v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_band_derived(self):
        """(value, err), (nchains, 3) each, of a series with SERIES_EQ_BAND: the jackknifed correlation ratios R_dCDW (bandDiff at (pi, pi)),
        R_nematic (bandDiff at q = 0) and R_bandMix (bandMix at (pi, pi))"""
        v, e = np.zeros((self.nchains_total(), 3)), np.zeros((self.nchains_total(), 3))
        check(self.lib.dqmc_series_band_derived_host(self.h, v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_custom_derived(self, Q=None):
        """(value, err), (nchains, count) each, of a series with SERIES_EQ_CUSTOM: the jackknifed correlation ratio
        R = 1 - [S(Q + dx) + S(Q + dy)] / (2 S(Q)) of every custom bilinear at Q = (qx, qy) in units of 2 pi / L, default (L/2, L/2)"""
        qx, qy = (self.L // 2, self.L // 2) if Q is None else Q
        count = len(self.get_custom_bilinears())
        v, e = np.zeros((self.nchains_total(), count)), np.zeros((self.nchains_total(), count))
        check(self.lib.dqmc_series_custom_derived_host(self.h, int(qx), int(qy), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_custom_pair_derived(self, Q=None):
        """series_custom_derived for the custom pair operators of a series with SERIES_EQ_CUSTOM_PAIR: (value, err), (nchains, count)"""
        qx, qy = (self.L // 2, self.L // 2) if Q is None else Q
        count = len(self.get_custom_pair_operators())
        v, e = np.zeros((self.nchains_total(), count)), np.zeros((self.nchains_total(), count))
        check(self.lib.dqmc_series_custom_pair_derived_host(self.h, int(qx), int(qy), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_pair_vertex(self, Q=(0, 0)):
        """bubble and vertex of every custom pair operator at Q = (qx, qy), of a series with SERIES_MATS_CUSTOM_PAIR | SERIES_GREEN_MATRIX:
        (value, err), (nchains, count, 5 + m) each -- P = Re chi(Q, i omega_0), Pbar, Gamma = 1/P - 1/Pbar, Gamma Pbar = Pbar/P - 1, then
        Pbar(Q, tau_k) for k = 0 .. m; jackknife over the closed bins"""
        n = self.lib.dqmc_series_pair_vertex_size(self.h)
        v, e = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        check(self.lib.dqmc_series_pair_vertex_host(self.h, int(Q[0]), int(Q[1]), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v.reshape(self.nchains_total(), -1, 5 + self.m), e.reshape(self.nchains_total(), -1, 5 + self.m)

    def series_ph_vertex(self, Q=(0, 0)):
        """particle-hole bubble and vertex of every custom bilinear at Q = (qx, qy), of a series with SERIES_MATS_CUSTOM |
        SERIES_GREEN_MATRIX: (value, err), (nchains, count, 6 + m) each -- chi = Re chi(Q, i omega_0) - D, chibar (the connected Wick term on
        the averaged Green's function, ph_bubble), Gamma = 1/chi - 1/chibar, Gamma chibar = chibar/chi - 1, D = beta Re(obar^2) sum_d cos(Q d),
        then chibar(Q, tau_k) for k = 0 .. m; jackknife over the closed bins"""
        n = self.lib.dqmc_series_ph_vertex_size(self.h)
        v, e = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        check(self.lib.dqmc_series_ph_vertex_host(self.h, int(Q[0]), int(Q[1]), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v.reshape(self.nchains_total(), -1, 6 + self.m), e.reshape(self.nchains_total(), -1, 6 + self.m)

    def series_hubbard_derived(self, Q):
        """(value, err), (nchains, 19) each, of a Hubbard context's series with SERIES_HUB_EQ at Q = (qx, qy) in units of 2 pi / L: R_X
        (entries 0 .. 7) and xi_X (8 .. 15) of greenUp, greenDn, charge, spinZZ, spinXX, pairS, pairSx, pairD, then S(Q), R and xi of
        the rotation-summed spin channel spinZZ + 2 spinXX; NaN where the quantity is undefined"""
        v, e = np.zeros((self.nchains_total(), 19)), np.zeros((self.nchains_total(), 19))
        check(self.lib.dqmc_series_hubbard_derived_host(self.h, int(Q[0]), int(Q[1]), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_phi_derived(self):
        """(value, err), (nchains, 6) each, of a series with SERIES_PHI: the jackknifed Binder cumulant and ratio of |phibar|, beta N
        <|phibar|^2>, its connected part, the correlation ratio R_phi and the second-moment correlation length xi_phi"""
        v, e = np.zeros((self.nchains_total(), 6)), np.zeros((self.nchains_total(), 6))
        check(self.lib.dqmc_series_phi_derived_host(self.h, v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)))
        return v, e

    def series_end(self):
        check(self.lib.dqmc_series_end(self.h))

    def series_configure(self, auto_rebin=False, track_variance=False):
        """options of the open, still empty series: auto_rebin merges neighbouring bins whenever max_bins (even, >= 4) bins are closed;
        track_variance keeps the running mean and m2 of the single samples per slot (for tau of series_binning)"""
        flags = (_lib.DQMC_SERIES_AUTO_REBIN if auto_rebin else 0) | (_lib.DQMC_SERIES_TRACK_VARIANCE if track_variance else 0)
        check(self.lib.dqmc_series_configure(self.h, flags))

    def series_state(self):
        """the dqmc_series_state of the open series: bin_size, max_bins, nfreq, parts, flags, bins_closed, sweeps_in_open_bin, nb, samples,
        rebins, sample_len"""
        st = _lib.dqmc_series_state()
        check(self.lib.dqmc_series_get_state(self.h, C.byref(st)))
        return st

    def series_rebin(self):
        """merge neighbouring closed bins in place: half as many bins of twice the size"""
        check(self.lib.dqmc_series_rebin(self.h))

    def series_binning(self, levels, tau=True):
        """binning analysis of every slot: (err, tau), (levels, nchains, S) each -- the jackknife error over the bins merged l times and the
        integrated autocorrelation time in sweeps it implies (needs track_variance); tau=False: err alone"""
        S = self.series_info()[2]
        shape = (max(int(levels), 0), self.nchains_total(), S)
        err = np.zeros(shape)
        if not tau:
            check(self.lib.dqmc_series_binning_host(self.h, int(levels), err.ctypes.data_as(_lib._DP), None))
            return err
        t = np.zeros(shape)
        check(self.lib.dqmc_series_binning_host(self.h, int(levels), err.ctypes.data_as(_lib._DP), t.ctypes.data_as(_lib._DP)))
        return err, t

    def _series_export_len(self, st):
        return (st.bins_closed + 1 + (2 if st.flags & _lib.DQMC_SERIES_TRACK_VARIANCE else 0)) * st.nb * st.sample_len

    def series_export(self):
        """(state, data): data = the closed bins [bins_closed][nchains][S], the open bin [nchains][S] and, with track_variance, w and m2
        [nchains][S] each, flat"""
        st = self.series_state()
        out = np.zeros(self._series_export_len(st))
        check(self.lib.dqmc_series_export_host(self.h, out.ctypes.data_as(_lib._DP), out.size))
        return st, out

    def series_import(self, state, data):
        """restore what series_export returned into the open series (series_begin with the same parts, nfreq and chains first)"""
        data = np.ascontiguousarray(data, dtype=np.float64)
        check(self.lib.dqmc_series_import_host(self.h, C.byref(state), data.ctypes.data_as(_lib._DP), data.size))

    def td_fine_propagate(self, j, k):
        """for tests: the work copies at slice k of boundary j's segment, by the steps of measure_timedisplaced_segment; measures nothing"""
        check(self.lib.dqmc_td_fine_propagate(self.h, j, k))

    def green_td_fine(self):
        """(slice k, G(tau_k,0), G(0,tau_k), G(tau_k)): the last propagated triple of the selected chain"""
        gt0 = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        g0t, gtt = np.zeros_like(gt0), np.zeros_like(gt0)
        sl = C.c_int(-1)
        check(self.lib.dqmc_get_green_td_fine_host(self.h, gt0.ctypes.data, g0t.ctypes.data, gtt.ctypes.data, C.byref(sl)))
        return sl.value, gt0, g0t, gtt

    def select_chain(self, b):
        """host-buffer calls (fields, G, sv, UdV, uniforms, update state, ...) refer to chain b from now on"""
        check(self.lib.dqmc_select_chain(self.h, b))

    # fields: phi given/returned as (m+1, N, OPDIM) [oracle layout]; the ABI uses (N, OPDIM, m+1) col-major
    def set_fields(self, phi_kNd):
        ref = np.asfortranarray(np.transpose(np.asarray(phi_kNd, dtype=np.float64), (1, 2, 0)))
        check(self.lib.dqmc_set_fields_host(self.h, ref.ctypes.data_as(_lib._DP)))

    # the discrete field of cdwU != 0: (m+1, N) int32, values +-1 / +-2 (slice 0 unused)
    def set_cdwl(self, cdwl_kN):
        a = np.ascontiguousarray(cdwl_kN, dtype=np.int32)
        assert a.shape == (self.m + 1, self.N)
        check(self.lib.dqmc_set_cdwl_host(self.h, a.ctypes.data))

    def get_cdwl(self):
        a = np.zeros((self.m + 1, self.N), dtype=np.int32)
        check(self.lib.dqmc_get_cdwl_host(self.h, a.ctypes.data))
        return a

    def get_fields(self):
        phi = np.zeros((self.N, self.opdim, self.m + 1), order="F")
        ch = np.zeros((self.N, self.m + 1), order="F")
        sh = np.zeros((self.N, self.m + 1), order="F")
        check(self.lib.dqmc_get_fields_host(self.h, phi.ctypes.data_as(_lib._DP), ch.ctypes.data_as(_lib._DP),
                                            sh.ctypes.data_as(_lib._DP)))
        return np.transpose(phi, (2, 0, 1)).copy(), ch.T.copy(), sh.T.copy()

    def bmult(self, side, inverse, k2, k1, A):
        a = _fmat(A)
        check(self.lib.dqmc_bmult_host(self.h, side, int(inverse), k2, k1, a.ctypes.data))
        return a

    def bmult_src(self, side, inverse, k2, k1, A):
        """dqmc_bmult_src_host: the same product out of place; returns (result, the source buffer as it is afterwards)"""
        a = _fmat(A)
        out, after = np.zeros_like(a), np.zeros_like(a)
        check(self.lib.dqmc_bmult_src_host(self.h, side, int(inverse), k2, k1, a.ctypes.data, out.ctypes.data, after.ctypes.data))
        return out, after

    def leftMultiplyBmat(self, A, k2, k1):
        return self.bmult(LEFT, 0, k2, k1, A)

    def leftMultiplyBmatInv(self, A, k2, k1):
        return self.bmult(LEFT, 1, k2, k1, A)

    def rightMultiplyBmat(self, A, k2, k1):
        return self.bmult(RIGHT, 0, k2, k1, A)

    def rightMultiplyBmatInv(self, A, k2, k1):
        return self.bmult(RIGHT, 1, k2, k1, A)

    def udvDecompose(self, M):
        a = _fmat(M)
        U = np.zeros_like(a)
        Vt = np.zeros_like(a)
        d = np.zeros(self.ng)
        sw = C.c_int(0)
        check(self.lib.dqmc_udv_decompose_host(self.h, a.ctypes.data, U.ctypes.data, d.ctypes.data_as(_lib._DP),
                                               Vt.ctypes.data, C.byref(sw)))
        return U, d, Vt, sw.value

    # per-chain operands of the two test-facing stabilisation calls: (nchains, n_g, n_g) <-> [chain] column-major, (nchains, n_g) scales
    def _chain_mats(self, a):
        if a is None:
            return None
        a = np.asarray(a, dtype=np.complex128).reshape(self.nchains_total(), self.ng, self.ng)
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))

    def _chain_vecs(self, a):
        if a is None:
            return None
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.nchains_total(), self.ng))

    def _chain_out(self):
        return np.zeros((self.nchains_total(), self.ng, self.ng), dtype=np.complex128)

    def decompose(self, M, colscale=None, rowscale=None, kind=0, Aold=None):
        """dqmc_decompose_host: the chain factorisation of diag(rowscale) M diag(colscale) as the sweep calls it, every chain its own
        operands, shapes (nchains, n_g, n_g) and (nchains, n_g); kind 0 R-type, 1 L-type; with Aold the chained step.  Returns
        (U, d, V_t, sweeps), M' = U diag(d) V_t^H.  The context's own G is void afterwards (setupUdVStorage_and_calculateGreen rebuilds it)"""
        m, a = self._chain_mats(M), self._chain_mats(Aold)
        cs, rs = self._chain_vecs(colscale), self._chain_vecs(rowscale)
        U, Vt, d = self._chain_out(), self._chain_out(), np.zeros((self.nchains_total(), self.ng))
        sw = C.c_int(0)
        dp = lambda v: None if v is None else v.ctypes.data_as(_lib._DP)
        check(self.lib.dqmc_decompose_host(self.h, m.ctypes.data, dp(cs), dp(rs), int(kind), None if a is None else a.ctypes.data,
                                           U.ctypes.data, dp(d), Vt.ctypes.data, C.byref(sw)))
        return np.transpose(U, (0, 2, 1)).copy(), d, np.transpose(Vt, (0, 2, 1)).copy(), sw.value

    def green_from_factors(self, L=None, R=None, td=False, g0=False):
        """dqmc_green_from_factors_host: greenFromUdV of the L-type slot L = (U_l, d_l, V_l) and the R-type slot R = (U_r, d_r, V_r), per
        chain; one of them None: greenFromEye_and_UdV of the other.  Returns a dict with 'G', 'sv' and, with td (set_timedisplaced on,
        both slots), 'GT0', 'G0T', with g0 (tdParticleHole) also 'G00'.  The context's own G is void afterwards"""
        slots = []
        for sl in (L, R):
            slots += [None, None, None] if sl is None else [self._chain_mats(sl[0]), self._chain_vecs(sl[1]), self._chain_mats(sl[2])]
        out = {"G": self._chain_out(), "sv": np.zeros((self.nchains_total(), self.ng))}
        if td:
            out["GT0"], out["G0T"] = self._chain_out(), self._chain_out()
        if g0:
            out["G00"] = self._chain_out()
        mp = lambda v: None if v is None else v.ctypes.data
        dp = lambda v: None if v is None else v.ctypes.data_as(_lib._DP)
        check(self.lib.dqmc_green_from_factors_host(self.h, mp(slots[0]), dp(slots[1]), mp(slots[2]), mp(slots[3]), dp(slots[4]), mp(slots[5]),
                                                    mp(out["G"]), dp(out["sv"]), mp(out.get("GT0")), mp(out.get("G0T")), mp(out.get("G00"))))
        return {k: (v if k == "sv" else np.transpose(v, (0, 2, 1)).copy()) for k, v in out.items()}

    def gemm(self, opA, opB, A, B):
        a, b = _fmat(A), _fmat(B)
        c = np.zeros_like(a)
        check(self.lib.dqmc_gemm_host(self.h, opA, opB, a.ctypes.data, b.ctypes.data, c.ctypes.data))
        return c

    def setupUdVStorage_and_calculateGreen(self):
        check(self.lib.dqmc_udv_setup(self.h))

    def advanceDownGreen(self, l):
        check(self.lib.dqmc_advance(self.h, DOWN, l))

    def advanceUpGreen(self, l):
        check(self.lib.dqmc_advance(self.h, UP, l))

    def wrapDownGreen(self, k):
        check(self.lib.dqmc_wrap(self.h, DOWN, k))

    def wrapUpGreen(self, k):
        check(self.lib.dqmc_wrap(self.h, UP, k))

    def wrapSkip(self, direction, k):
        """dqmc_wrap_skip: the bookkeeping of a wrap whose G the following advance overwrites; G is stale until then"""
        check(self.lib.dqmc_wrap_skip(self.h, direction, k))

    def reset_storage0(self):
        check(self.lib.dqmc_reset_storage0(self.h))

    def push_uniforms(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self.lib.dqmc_push_uniforms_host(self.h, u.ctypes.data_as(_lib._DP), u.size))

    def push_uniforms_all(self, u):
        """u[nchains][n]: every chain's window in one transfer"""
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self.lib.dqmc_push_uniforms_all_host(self.h, u.ctypes.data_as(_lib._DP), u.shape[1]))

    def stage_uniforms_tail(self, u):
        """u[nchains][n]: the n draws behind every chain's current window (dqmc_stage_uniforms_tail_host)"""
        u = np.ascontiguousarray(u, dtype=np.float64)
        check(self.lib.dqmc_stage_uniforms_tail_host(self.h, u.ctypes.data_as(_lib._DP), u.shape[1]))

    def advance_uniforms(self, offsets):
        """dqmc_advance_uniforms: the new window of chain b starts offsets[b] draws behind the start of its current one"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.size != self.nchains_total():
            raise ValueError("one offset per chain")
        check(self.lib.dqmc_advance_uniforms(self.h, off.ctypes.data_as(C.POINTER(C.c_uint64))))

    def uniform_window(self, n):
        """the first n uniforms of the selected chain's current window"""
        out = np.zeros(int(n))
        check(self.lib.dqmc_get_uniform_window_host(self.h, out.ctypes.data_as(_lib._DP), out.size))
        return out

    def update_states_all(self):
        st = (_lib.dqmc_update_state * self.nchains_total())()
        check(self.lib.dqmc_get_update_states_all_host(self.h, st))
        return list(st)

    def updateInSlice(self, k, thermalization=False, proposal="box", adapt="box", adaptScaleVariance=False, repeat=1):
        """updateInSlice / updateInSliceThermalization; proposal: box | rotate | scale | rotate_and_scale (the latter three: O(3))"""
        check(self.lib.dqmc_update_slice_ex(self.h, k, int(thermalization), PROPOSE[proposal], ADAPT[adapt], int(adaptScaleVariance), int(repeat)))

    def updateInSliceFinal(self, k, thermalization=False, proposal="box", adapt="box", adaptScaleVariance=False, repeat=1, thenWrap=0):
        """dqmc_update_slice_final: updateInSlice of the last slice of a segment -- the block in which a chain finishes the slice is
        not flushed, G is stale until the advance that follows; thenWrap: 0, or DOWN for the bookkeeping of wrapDownGreen(k) as well"""
        check(self.lib.dqmc_update_slice_final(self.h, k, int(thermalization), PROPOSE[proposal], ADAPT[adapt], int(adaptScaleVariance),
                                               int(repeat), int(thenWrap)))

    def update_state(self):
        st = _lib.dqmc_update_state()
        check(self.lib.dqmc_get_update_state_host(self.h, C.byref(st)))
        return st

    def set_update_state(self, st):
        check(self.lib.dqmc_set_update_state_host(self.h, C.byref(st)))

    @property
    def g(self):
        g = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        check(self.lib.dqmc_get_green_host(self.h, g.ctypes.data))
        return g

    def set_green(self, g, k):
        a = _fmat(g)
        check(self.lib.dqmc_set_green_host(self.h, a.ctypes.data, k))

    @property
    def g_inv_sv(self):
        sv = np.zeros(self.ng)
        check(self.lib.dqmc_get_sv_host(self.h, sv.ctypes.data_as(_lib._DP)))
        return sv

    def udv(self, l):
        U = np.zeros((self.ng, self.ng), dtype=np.complex128, order="F")
        Vt = np.zeros_like(U)
        d = np.zeros(self.ng)
        check(self.lib.dqmc_get_udv_host(self.h, l, U.ctypes.data, d.ctypes.data_as(_lib._DP), Vt.ctypes.data))
        return U, d, Vt

    @property
    def currentTimeslice(self):
        return self.lib.dqmc_current_timeslice(self.h)

    def backup(self):
        check(self.lib.dqmc_backup(self.h))

    def restore(self):
        check(self.lib.dqmc_restore(self.h))

    def exchange_action(self):
        v = C.c_double(0)
        check(self.lib.dqmc_exchange_action_host(self.h, C.byref(v)))
        return v.value

    def set_exchange_parameter(self, r):
        check(self.lib.dqmc_set_exchange_parameter(self.h, r))

    # one transfer / one launch for ALL chains of a batched context
    def phi_action_all(self):
        out = np.zeros(self.nchains_total())
        check(self.lib.dqmc_phi_action_all_host(self.h, out.ctypes.data_as(_lib._DP)))
        return out

    def shift_fields_all(self, shifts):
        a = np.ascontiguousarray(shifts, dtype=np.float64)
        check(self.lib.dqmc_shift_fields_all_host(self.h, a.ctypes.data_as(_lib._DP)))

    def get_fields_all(self):
        """(nchains, m+1, N, OPDIM)"""
        nb = self.nchains_total()
        a = np.zeros((nb, self.m + 1, self.opdim, self.N))
        check(self.lib.dqmc_get_fields_all_host(self.h, a.ctypes.data_as(_lib._DP)))
        return np.transpose(a, (0, 1, 3, 2)).copy()

    def sv_all(self):
        a = np.zeros((self.nchains_total(), self.ng))
        check(self.lib.dqmc_get_sv_all_host(self.h, a.ctypes.data_as(_lib._DP)))
        return a

    def nchains_total(self):
        return self.lib.dqmc_num_chains(self.h)

    def synchronize(self):
        check(self.lib.dqmc_synchronize(self.h))

    def schedule_info(self):
        """which execution variants this context latched at create time, and how many update blocks ran through each schedule"""
        si = _lib.dqmc_schedule_info()
        check(self.lib.dqmc_get_schedule_info(self.h, C.byref(si)))
        return si

    def profile_enable(self, on=True):
        check(self.lib.dqmc_profile_enable(self.h, int(on)))

    def profile_read(self):
        pr = _lib.dqmc_profile()
        check(self.lib.dqmc_profile_read(self.h, C.byref(pr)))
        names = ["bmult", "gemm", "decomp", "decide", "other", "gather", "flush"]
        out = {nm: (pr.ms[i], int(pr.launches[i])) for i, nm in enumerate(names)}
        out["jacobi"] = out["decomp"]
        out.update(svd_calls=int(pr.svd_calls), svd_sweeps_total=int(pr.svd_sweeps_total),
                   svd_sweeps_max=int(pr.svd_sweeps_max), qr_calls=int(pr.qr_calls), gemm_flops=pr.gemm_flops,
                   decomp_round_ms=pr.decomp_round_ms, decomp_rounds=int(pr.decomp_rounds),
                   blocks_nonempty=int(pr.blocks_nonempty), chains=int(pr.chains),
                   updates_accepted=int(pr.updates_accepted), lu_calls=int(pr.lu_calls),
                   sub={"lu_update": [pr.sub_ms[0], int(pr.sub_launches[0]), pr.sub_flops[0], pr.sub_bytes[0]],
                        "fact_gemm": [pr.sub_ms[1], int(pr.sub_launches[1]), pr.sub_flops[1], pr.sub_bytes[1]]})
        return out


class _CtxView(KernelContext):
    """Non-owning KernelContext over the dqmc_ctx of a DetSDW replica (profiling, state inspection)."""

    def __init__(self, lib, handle, info):
        self.lib, self.h = lib, C.c_void_p(handle)
        self.opdim, self.L, self.m, self.s = info.opdim, info.L, info.m, info.s
        self.N, self.MSF, self.ng, self.n = info.N, info.MSF, info.n_g, info.n

    def close(self):
        self.h = None


def _host_params(pars: SDWParams):
    if pars.timeDisplacedPairing and not pars.timeDisplacedMeasurements:
        raise ValueError("timeDisplacedPairing needs timeDisplacedMeasurements")
    if pars.timeDisplacedParticleHole and not pars.timeDisplacedMeasurements:
        raise ValueError("timeDisplacedParticleHole needs timeDisplacedMeasurements")
    if pars.equalTimeCorrelators and not pars.fermionMeasurements:
        raise ValueError("equalTimeCorrelators needs fermionMeasurements")
    if pars.timeDisplacedCurrent and not pars.timeDisplacedParticleHole:
        raise ValueError("timeDisplacedCurrent needs timeDisplacedParticleHole")
    if pars.bandCorrelators and not (pars.timeDisplacedParticleHole or pars.equalTimeCorrelators):
        raise ValueError("bandCorrelators needs timeDisplacedParticleHole or equalTimeCorrelators")
    band_td = bool(pars.bandCorrelators and pars.timeDisplacedParticleHole)
    band_eq = bool(pars.bandCorrelators and pars.equalTimeCorrelators)
    return _lib.detsdw_params(
        opdim=pars.opdim, L=pars.L, m=pars.m, s=pars.s, delaySteps=pars.delaySteps,
        globalShift=int(pars.globalShift), globalUpdateInterval=pars.globalUpdateInterval,
        weakZflux=int(pars.weakZflux), phi2bosons=int(pars.phi2bosons), device=pars.device,
        simindex=pars.simindex, rngSeed=pars.rngSeed,
        has_mux_muy=int(pars.mux is not None and pars.muy is not None),
        updateMethod=UPDATE_METHOD[pars.updateMethod], bc=pars.bc.encode(),
        beta=pars.beta, dtau=pars.dtau, r=pars.r, c=pars.c, u=pars.u, lambda_=pars.lambda_,
        txhor=pars.txhor, txver=pars.txver, tyhor=pars.tyhor, tyver=pars.tyver,
        mu=pars.mu, mux=pars.mux or 0.0, muy=pars.muy or 0.0, accRatio=pars.accRatio, cdwU=pars.cdwU,
        stabilisation=STABILISATION[pars.stabilisation], cb_none=int(not pars.checkerboard),
        wolffClusterUpdate=int(pars.wolffClusterUpdate), wolffClusterShiftUpdate=int(pars.wolffClusterShiftUpdate),
        repeatWolffPerSweep=int(pars.repeatWolffPerSweep), fermionMeasurements=int(bool(pars.fermionMeasurements)) | (_lib.DETSDW_FM_EQ_CORRELATORS if pars.equalTimeCorrelators else 0)
        | (_lib.DETSDW_FM_EQ_BAND if band_eq else 0),
        spinProposalMethod=SPIN_PROPOSAL[pars.spinProposalMethod], adaptScaleVariance=int(pars.adaptScaleVariance),
        repeatUpdateInSlice=int(pars.repeatUpdateInSlice), timeDisplacedMeasurements=(2 if pars.timeDisplacedPairing else int(bool(pars.timeDisplacedMeasurements)))
        | (_lib.DETSDW_TD_EVERY_SLICE if pars.timeDisplacedEverySlice else 0)      # without timeDisplacedMeasurements: ParameterWrong from the library
        | (_lib.DETSDW_TD_FINE_ON_DEVICE if pars.timeDisplacedFineOnDevice else 0),  # without timeDisplacedEverySlice: the same
        timeDisplacedParticleHole=(2 if pars.timeDisplacedCurrent else int(bool(pars.timeDisplacedParticleHole))) | (_lib.DETSDW_TD_PH_BAND if band_td else 0),
        tuning=_tuning(pars.pipeline, pars.qrVariant, pars.greenVariant, pars.maxJacobiSweeps, pars.proposalBudget, pars.decideThreads, pars.bmultPath, pars.rngLookahead))


class DetSDW(_GreenCheck):
    """The replica (C++ host layer): same method names as the reference's DetSDW / DetModel.

    Also serves as the view of ONE chain of a DetSDWBatch (`batch.chain(b)`): then it does not own the
    handle, `sweep*` are not available on it (the batch sweeps all chains in lockstep) and every call first
    selects its chain."""

    def __init__(self, pars: SDWParams = None, _batch=None, _chain=0):
        self.lib = load()
        self._chain = _chain
        self._batch = _batch
        if _batch is not None:
            self.h = _batch.h
            self.pars = _batch.pars_list[_chain]
            return
        p = _host_params(pars)
        h = C.c_void_p()
        check(self.lib.detsdw_create(C.byref(p), C.byref(h)), host=True)
        self.h = h
        self.pars = pars

    def _sel(self):
        if self._batch is not None:
            check(self.lib.detsdw_select_chain(self.h, self._chain), host=True)

    def close(self):
        if self._batch is not None:
            self.h = None
            return
        if self.h:
            self.lib.detsdw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _gc_calls = ("detsdw_set_green_check", "detsdw_get_green_check", "detsdw_reset_green_check", True)

    def _gc_handle(self):
        if self._batch is not None:
            raise RuntimeError("the wrap-error diagnostics belong to the whole batch: call them on the DetSDWBatch")
        return self.h

    def _gc_shape(self):
        i = self.info
        return 1, i.n, i.n_g

    def sweep(self, takeMeasurements=False):
        if self._batch is not None:
            raise RuntimeError("a chain of a batch cannot sweep on its own: call DetSDWBatch.sweep()")
        check(self.lib.detsdw_sweep(self.h, int(takeMeasurements)), host=True)

    def sweepThermalization(self):
        if self._batch is not None:
            raise RuntimeError("a chain of a batch cannot sweep on its own: call DetSDWBatch.sweepThermalization()")
        check(self.lib.detsdw_sweep_thermalization(self.h), host=True)

    @property
    def info(self):
        self._sel()
        i = _lib.detsdw_info()
        check(self.lib.detsdw_get_info(self.h, C.byref(i)), host=True)
        return i

    @property
    def observables(self):
        """bosonic observables of the last sweep(takeMeasurements=True) (reference: measure / finishMeasurements)"""
        self._sel()
        o = _lib.detsdw_observables()
        check(self.lib.detsdw_get_observables(self.h, C.byref(o)), host=True)
        return o

    def observable_vector(self, name):
        """'kOccX', 'kOccY', 'pairPlus', 'pairMinus' of the last sweep(True) with fermionMeasurements (length N); 'greenKTauX',
        'greenKTauY' with timeDisplacedMeasurements: shape (n-1, N), row j-1 = tau_j of tau_grid(); 'pairPlusTau', 'pairMinusTau'
        with timeDisplacedPairing: shape (n-1, N), column = periodic site difference dy L + dx; 'pairPlusTauQ0', 'pairMinusTauQ0':
        their sums over the site difference, length n-1; 'chargeTau', 'spinZTau', 'sdwTau' with timeDisplacedParticleHole: shape
        (n-1, N), same rows and columns; 'chargeTauQ0', 'spinZTauQ0', 'sdwTauQ0': their sums over the site difference; 'currentXTau',
        'currentYTau' with timeDisplacedCurrent: shape (n-1, N), same rows and columns; 'currentXTauQ0', 'currentYTauQ0': their sums over
        the site difference; 'bondKineticX', 'bondKineticY': the bond kinetic energy per site at tau_j, length n-1.  With
        timeDisplacedEverySlice every name from 'greenKTauX' on has a twin name + 'Fine' (e.g. 'chargeTauFine', 'pairPlusTauQ0Fine',
        'bondKineticXFine') with m+1 rows instead of n-1: row k = tau_k of tau_grid(fine=True), k = 0 .. m.  With equalTimeCorrelators:
        'chargeCorr', 'spinZCorr', 'sdwCorr', 'pairPlusCorr', 'pairMinusCorr' (length N, column = periodic site difference dy L + dx,
        averaged over the m slices of the sweep and over translations) and their structure factors 'chargeSq', 'spinZSq', 'sdwSq',
        'pairPlusSq', 'pairMinusSq' (length N, column qy L + qx, q = 2 pi (qx, qy) / L; structure_factor of the former).  With
        bandCorrelators: 'bandDiffTau', 'bandMixTau', 'bandDiffTauQ0', 'bandMixTauQ0' (and their 'Fine' twins) next to 'chargeTau', and
        'bandDiffCorr', 'bandMixCorr', 'bandDiffSq', 'bandMixSq' next to 'chargeCorr' / 'chargeSq'.  With matrices set by
        DetSDWBatch.set_custom_bilinears: 'custom{c}Tau', 'custom{c}TauQ0' (and their 'Fine' twins), 'custom{c}Corr', 'custom{c}Sq' for
        matrix c, shaped like the bandDiff names; with operators set by DetSDWBatch.set_custom_pair_operators the same four as
        'customPair{c}...' for pair operator c"""
        self._sel()
        which, d = observable_index(name)
        if d.family == _lib.DETSDW_OBS_FAMILY_PHI:            # the order-parameter part lives in a series only
            raise KeyError(name)
        shape, cplx = observable_shape(d, self.info)
        out = np.zeros(shape, dtype=np.complex128 if cplx else np.float64)
        check(self.lib.detsdw_get_observable_vector(self.h, which, out.ctypes.data_as(_lib._DP)), host=True)
        return out

    def matsubara(self, name, nfreq):
        """chi(q, i omega_n) of 'pairPlusTau', 'pairMinusTau', 'chargeTau', 'spinZTau', 'sdwTau', 'currentXTau', 'currentYTau' (column
        qy L + qx, q = 2 pi (qx, qy) / L) or G(k, i omega_n) of 'greenKTauX', 'greenKTauY' (column = k-vector as for kOcc), n = 0 ..
        nfreq-1: complex (nfreq, N), formed on the device from the every-slice blocks of the last sweep(True) by the trapezoid rule
        (needs timeDisplacedEverySlice; valid until the next sweep).  Frequencies: matsubara_frequencies()"""
        self._sel()
        out = np.zeros((int(nfreq), self.info.N), dtype=np.complex128)
        check(self.lib.detsdw_get_matsubara(self.h, _matsubara_index(name), int(nfreq), out.ctypes.data_as(_lib._DP)), host=True)
        return out

    def _series_shape(self, name):
        """(index of detsdw_series_stats, shape of one chain's values, complex?) of a series observable"""
        if self._batch is None:
            raise RuntimeError("a measurement series is opened on a batch: DetSDWBatch([pars]).series_begin()")
        which, d = observable_index(name)
        if d.series_part < 0:
            raise KeyError(name)
        return (which,) + observable_shape(d, self.info, self._batch._series_nfreq, series=True)

    def series_stats(self, name):
        """(mean, err) of this chain over the closed bins of the open series (DetSDWBatch.series_begin): name = an equal-time
        '...Corr' / '...Sq' observable, length N, or a name of matsubara(), complex (nfreq, N) with err = err(Re) + i err(Im)"""
        self._sel()
        which, shape, cplx = self._series_shape(name)
        mean, err = (np.zeros(shape, dtype=np.complex128 if cplx else np.float64) for _ in range(2))
        check(self.lib.detsdw_series_stats(self.h, which, mean.ctypes.data_as(_lib._DP), err.ctypes.data_as(_lib._DP)), host=True)
        return mean, err

    def series_bins(self, name, first=0, count=None):
        """the closed bin means first .. first + count - 1 (default: all from first) of this chain: (count,) + the shape of series_stats"""
        self._sel()
        which, shape, cplx = self._series_shape(name)
        if count is None:
            count = self._batch.series_info()[0] - first
        out = np.zeros((max(int(count), 0),) + shape, dtype=np.complex128 if cplx else np.float64)
        check(self.lib.detsdw_series_read_bins(self.h, which, int(first), int(count), out.ctypes.data_as(_lib._DP)), host=True)
        return out

    def series_binning(self, name, levels):
        """(err, tau) of this chain's slot, (levels,) + the shape of series_stats each: the binning analysis of the open series (needs
        track_variance); for complex observables the real and the imaginary part are analysed separately"""
        self._sel()
        which, shape, cplx = self._series_shape(name)
        err, tau = (np.zeros((max(int(levels), 0),) + shape, dtype=np.complex128 if cplx else np.float64) for _ in range(2))
        check(self.lib.detsdw_series_binning(self.h, which, int(levels), err.ctypes.data_as(_lib._DP), tau.ctypes.data_as(_lib._DP)), host=True)
        return err, tau

    def matsubara_frequencies(self, nfreq, fermionic=False):
        """omega_n, n = 0 .. nfreq-1: 2 pi n / beta, or (2n+1) pi / beta for the fermionic 'greenKTauX' / 'greenKTauY'"""
        n = np.arange(int(nfreq))
        return ((2 * n + 1) if fermionic else 2 * n) * np.pi / self.info.beta

    def tau_grid(self, fine=False):
        """tau_j = j s dtau, j = 1 .. n-1: the rows of greenKTauX / greenKTauY; fine=True (timeDisplacedEverySlice): tau_k = k dtau,
        k = 0 .. m, the rows of the '...Fine' observables"""
        if fine:
            out = np.zeros(self.info.m + 1)
            check(self.lib.detsdw_get_tau_grid_fine(self.h, out.ctypes.data_as(_lib._DP)), host=True)
            return out
        out = np.zeros(self.info.n - 1)
        check(self.lib.detsdw_get_tau_grid(self.h, out.ctypes.data_as(_lib._DP)), host=True)
        return out

    @property
    def phi(self):
        """(m+1, N, OPDIM) like the oracle; the ABI hands out the reference layout."""
        self._sel()
        i = self.info
        a = np.zeros((i.N, i.opdim, i.m + 1), order="F")
        check(self.lib.detsdw_get_phi(self.h, a.ctypes.data_as(_lib._DP)), host=True)
        return np.transpose(a, (2, 0, 1)).copy()

    @property
    def cdwl(self):
        """(m+1, N) int32: the discrete field l_i(tau_k) of cdwU != 0 (drawn at set-up whatever cdwU is; slice 0 unused)."""
        self._sel()
        i = self.info
        a = np.zeros((i.m + 1, i.N), dtype=np.int32)
        check(self.lib.detsdw_get_cdwl(self.h, a.ctypes.data), host=True)
        return a

    def set_cdwl(self, cdwl_kN):
        self._sel()
        a = np.ascontiguousarray(cdwl_kN, dtype=np.int32)
        check(self.lib.detsdw_set_cdwl(self.h, a.ctypes.data), host=True)

    def set_phi(self, phi_kNd):
        self._sel()
        ref = np.asfortranarray(np.transpose(np.asarray(phi_kNd, dtype=np.float64), (1, 2, 0)))
        check(self.lib.detsdw_set_phi(self.h, ref.ctypes.data_as(_lib._DP)), host=True)

    @property
    def g(self):
        self._sel()
        n = self.info.n_g
        g = np.zeros((n, n), dtype=np.complex128, order="F")
        check(self.lib.detsdw_get_green(self.h, g.ctypes.data), host=True)
        return g

    @property
    def g_inv_sv(self):
        self._sel()
        sv = np.zeros(self.info.n_g)
        check(self.lib.detsdw_get_green_inv_sv(self.h, sv.ctypes.data_as(_lib._DP)), host=True)
        return sv

    def save_state(self, path):
        """checkpoint of the whole replica object (all chains if this is a view of a batch)"""
        check(self.lib.detsdw_save_state(self.h, str(path).encode()), host=True)

    def load_state(self, path):
        check(self.lib.detsdw_load_state(self.h, str(path).encode()), host=True)

    def saveConfigurationStreamBinary(self, directory="."):
        """appends to <directory>/configs-phi.binarystream (reference format, src/detsdwopdim.cpp:4991-5012)"""
        self._sel()
        check(self.lib.detsdw_save_configuration_stream_binary(self.h, str(directory).encode()), host=True)

    def rand01(self):
        self._sel()
        return self.lib.detsdw_rng_rand01(self.h)

    @property
    def kernel_context(self):
        """the kernel context that holds this chain (a batch may spread its chains over several), this chain selected"""
        local = C.c_int(0)
        kc = _CtxView(self.lib, self.lib.detsdw_ctx_of_chain(self.h, self._chain, C.byref(local)), self.info)
        check(self.lib.dqmc_select_chain(kc.h, local.value))
        return kc

    # replica exchange surface (reference src/detsdwopdim.h:116-153)
    def get_exchange_parameter_value(self):
        self._sel()
        return self.lib.detsdw_get_exchange_parameter_value(self.h)

    def set_exchange_parameter_value(self, v):
        self._sel()
        check(self.lib.detsdw_set_exchange_parameter_value(self.h, v), host=True)

    def get_exchange_parameter_name(self):
        return self.lib.detsdw_get_exchange_parameter_name(self.h).decode()

    def get_exchange_action_contribution(self):
        self._sel()
        v = C.c_double(0)
        check(self.lib.detsdw_get_exchange_action_contribution(self.h, C.byref(v)), host=True)
        return v.value

    def get_control_data(self):
        self._sel()
        cd = _lib.detsdw_control_data()
        check(self.lib.detsdw_get_control_data(self.h, C.byref(cd)), host=True)
        return cd

    def set_control_data(self, cd):
        self._sel()
        check(self.lib.detsdw_set_control_data(self.h, C.byref(cd)), host=True)


class DetSDWBatch(_GreenCheck):
    """The replicas of one parallel-tempering ensemble on ONE GPU, swept in lockstep by one kernel context
    (detsdw_create_batch): every launch carries all chains, which is what fills the chip.  The parameter sets
    may differ only in r, rngSeed and simindex; chain b follows exactly the Markov chain of DetSDW(pars[b])."""

    def __init__(self, pars_list, sub_batches=0):
        """sub_batches: kernel contexts the chains are spread over and swept concurrently (one host thread each);
        0 = automatic (up to 4 contexts of at least 32 chains), 1 = one context / one launch sequence for all chains"""
        self.lib = load()
        self.pars_list = list(pars_list)
        arr = (_lib.detsdw_params * len(self.pars_list))(*[_host_params(p) for p in self.pars_list])
        h = C.c_void_p()
        check(self.lib.detsdw_create_batch_ex(arr, len(self.pars_list), int(sub_batches), C.byref(h)), host=True)
        self.h = h
        self.sub_batches = self.lib.detsdw_num_sub_batches(h)
        self._series_nfreq = 0
        self._series_open = False
        self.chains = [DetSDW(_batch=self, _chain=b) for b in range(len(self.pars_list))]

    def __len__(self):
        return len(self.chains)

    # the tables are per chain (per slot of the handle): not routed by control parameter, not part of save_state or of the series
    _gc_calls = ("detsdw_set_green_check", "detsdw_get_green_check", "detsdw_reset_green_check", True)

    def _gc_shape(self):
        i = self.chains[0].info
        return len(self.chains), i.n, i.n_g

    def chain(self, b):
        return self.chains[b]

    def sweep(self, takeMeasurements=False):
        check(self.lib.detsdw_sweep(self.h, int(takeMeasurements)), host=True)

    def sweepThermalization(self):
        check(self.lib.detsdw_sweep_thermalization(self.h), host=True)

    def save_state(self, path):
        check(self.lib.detsdw_save_state(self.h, str(path).encode()), host=True)

    def load_state(self, path):
        check(self.lib.detsdw_load_state(self.h, str(path).encode()), host=True)

    def set_custom_bilinears(self, mats):
        """up to four Hermitian 4 x 4 matrices M (band-spin order XUP, YDOWN, XDOWN, YUP): from the next sweep(True) on the correlators of
        sum_ab c^+_a M_ab c_b are measured like bandDiff -- 'custom{c}Tau' ... with timeDisplacedParticleHole, 'custom{c}Corr' / 'custom{c}Sq'
        with equalTimeCorrelators (one of the two is needed).  Between sweeps; a second call replaces the matrices, [] removes them"""
        m = _custom_matrices(mats)
        check(self.lib.detsdw_set_custom_bilinears(self.h, len(m), m.ctypes.data), host=True)

    def set_custom_bond_bilinears(self, ops):
        """set_custom_bilinears with nearest-neighbour bond parts: a list of up to four (M0, Mx, My), None for a zero matrix (see
        KernelContext.set_custom_bond_bilinears, bond_current, bond_kinetic).  Every 'custom{c}...' observable, Matsubara transform and
        series quantity serves the operators unchanged"""
        m0, mx, my = _custom_bond_operators(ops)
        check(self.lib.detsdw_set_custom_bond_bilinears(self.h, len(m0), m0.ctypes.data, mx.ctypes.data, my.ctypes.data), host=True)

    def get_custom_bond_bilinears(self):
        """the operators that are set: a list of (M0, Mx, My), complex 4 x 4 each"""
        return _get_custom_bond(self.lib.detsdw_get_custom_bond_bilinears, self.h, True)

    def set_custom_pair_operators(self, ops):
        """up to four pair operators (F0, Fx, Fy), None for a zero matrix (see KernelContext.set_custom_pair_operators, pair_operator): from
        the next sweep(True) on <Delta_A(tau) Delta_B^+(0)> is measured -- 'customPair{c}Tau' / 'customPair{c}TauQ0' (and their 'Fine' twins)
        with timeDisplacedMeasurements, 'customPair{c}Corr' / 'customPair{c}Sq' with equalTimeCorrelators (one of the two is needed).  Between
        sweeps; a second call replaces the operators, [] removes them; independent of set_custom_bilinears"""
        f0, fx, fy = _custom_bond_operators(ops)
        check(self.lib.detsdw_set_custom_pair_operators(self.h, len(f0), f0.ctypes.data, fx.ctypes.data, fy.ctypes.data), host=True)

    def get_custom_pair_operators(self):
        """the pair operators that are set: a list of (F0, Fx, Fy), complex 4 x 4 each"""
        return _get_custom_bond(self.lib.detsdw_get_custom_pair_operators, self.h, True)

    def set_green_matrix(self, on=True):
        """from the next sweep(True) on every time-displaced row also bins the averaged Green's function
        Gbar_rc(d; tau) = sum_B sigma(B, d) g~((B + d) r; B c) (see KernelContext.set_green_matrix): 'greenMatrixTau' (and 'greenMatrixTauFine'),
        complex (rows, N, 4, 4), and, in a series opened afterwards with timeDisplacedEverySlice, the part behind
        series_stats_all('greenMatrixTau') and the pair vertex (series_derived_all('gammaBubbleCustomPair{c}', Q=(0, 0)), series_pair_bubble_all).
        The part costs (m+1) 2 R^2 N doubles per chain and bin: size maxBins accordingly.  Needs timeDisplacedMeasurements; between sweeps"""
        check(self.lib.detsdw_set_green_matrix(self.h, int(on)), host=True)

    def _series_pair_vertex(self, c, Q):
        m = self.chains[0].info.m
        if Q is None:
            raise ValueError("the pair vertex needs Q = (qx, qy) in units of 2 pi / L: (0, 0) for uniform pairing")
        qx, qy = Q
        v, e = np.zeros((len(self.chains), 5 + m)), np.zeros((len(self.chains), 5 + m))
        check(self.lib.detsdw_series_pair_vertex(self.h, int(c), int(qx), int(qy), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)), host=True)
        return v, e

    def series_pair_bubble_all(self, c, Q):
        """(value, err), (nchains, m+1) each: the bubble Pbar_c(Q, tau_k) of pair operator c on the averaged Green's function of the series,
        Q = (qx, qy) in units of 2 pi / L ((0, 0): uniform pairing), jackknife over the closed bins"""
        v, e = self._series_pair_vertex(c, Q)
        return v[:, 4:].copy(), e[:, 4:].copy()

    def _series_ph_vertex(self, c, Q):
        m = self.chains[0].info.m
        if Q is None:
            raise ValueError("the particle-hole vertex needs Q = (qx, qy) in units of 2 pi / L: (L/2, L/2) for the SDW channel, (0, 0) for nematic ones")
        qx, qy = Q
        v, e = np.zeros((len(self.chains), 6 + m)), np.zeros((len(self.chains), 6 + m))
        check(self.lib.detsdw_series_ph_vertex(self.h, int(c), int(qx), int(qy), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)), host=True)
        return v, e

    def series_ph_bubble_all(self, c, Q):
        """(value, err), (nchains, m+1) each: the particle-hole bubble chibar_c(Q, tau_k) of custom bilinear c on the averaged Green's function
        of the series (set_green_matrix and the matrices set before it began), Q = (qx, qy) in units of 2 pi / L, jackknife over the closed
        bins"""
        v, e = self._series_ph_vertex(c, Q)
        return v[:, 5:].copy(), e[:, 5:].copy()

    def matsubara_all(self, name, nfreq):
        """DetSDW.matsubara of every chain: complex (nchains, nfreq, N), one device call per sub-batch"""
        out = np.zeros((len(self.chains), int(nfreq), self.chains[0].info.N), dtype=np.complex128)
        check(self.lib.detsdw_get_matsubara_all(self.h, _matsubara_index(name), int(nfreq), out.ctypes.data_as(_lib._DP)), host=True)
        return out

    def series_begin(self, binSize, maxBins, nfreq=0, host_copy=True, auto_rebin=False, track_variance=False, phi=False):
        """open a measurement series on the device: from now on every sweep(True) adds one sample per chain -- the equal-time C(d),
        S(q) with equalTimeCorrelators, the Matsubara transforms at nfreq frequencies of every enabled channel with
        timeDisplacedEverySlice -- to bins of binSize sweeps, at most maxBins of them.  host_copy=False: measurement sweeps no longer
        copy the equal-time block to the host ('...Corr' / '...Sq' of observable_vector raise while the series is open).
        auto_rebin: whenever maxBins (even, >= 4) bins are closed, neighbouring bins are merged -- the run never outlives the series;
        track_variance: keep the variance of the single samples, which series_binning_all needs for tau;
        phi: add the order-parameter part, formed on the device from the field -- 'phiChi' (nfreq, N), chi_phi(q, i omega_n) with the
        physical susceptibility beta N <chi>, and 'phiScalars' (|phibar|, |phibar|^2, |phibar|^4, equal-time susceptibility,
        associatedEnergy), with 'binderPhi', 'binderRatioPhi', 'chiPhi', 'chiPhiConnected', 'R_phi', 'xiPhi' of series_derived_all.  Needs
        1 <= nfreq <= m and no other option: a batch without fermionMeasurements may open such a series"""
        flags = (0 if host_copy else _lib.DETSDW_SERIES_NO_HOST_COPY) | (_lib.DETSDW_SERIES_PHI if phi else 0)
        check(self.lib.detsdw_series_begin(self.h, int(binSize), int(maxBins), int(nfreq), flags), host=True)
        self._series_nfreq = int(nfreq)
        self._series_open = True
        if auto_rebin or track_variance:
            opts = (_lib.DQMC_SERIES_AUTO_REBIN if auto_rebin else 0) | (_lib.DQMC_SERIES_TRACK_VARIANCE if track_variance else 0)
            try:
                check(self.lib.detsdw_series_configure(self.h, opts), host=True)
            except _lib.DqmcError:
                self.lib.detsdw_series_end(self.h)         # refused options: no half-configured series stays open
                self._series_open = False
                raise

    def series_state(self):
        """the dqmc_series_state all kernel contexts share (nb = the chains of the batch)"""
        st = _lib.dqmc_series_state()
        check(self.lib.detsdw_series_get_state(self.h, C.byref(st)), host=True)
        return st

    def series_rebin(self):
        """merge neighbouring closed bins of every slot: half as many bins of twice the size"""
        check(self.lib.detsdw_series_rebin(self.h), host=True)

    def series_binning_all(self, name, levels):
        """DetSDW.series_binning of every slot: (err, tau), (nchains, levels) + the per-chain shape each; one device call per sub-batch"""
        which, shape, cplx = self.chains[0]._series_shape(name)
        err, tau = (np.zeros((len(self.chains), max(int(levels), 0)) + shape, dtype=np.complex128 if cplx else np.float64) for _ in range(2))
        check(self.lib.detsdw_series_binning_all(self.h, which, int(levels), err.ctypes.data_as(_lib._DP), tau.ctypes.data_as(_lib._DP)), host=True)
        return err, tau

    def series_save(self, path):
        """the whole series -- bins, open bin, counters, variance, route -- to a file of its own, next to save_state"""
        check(self.lib.detsdw_series_save(self.h, str(path).encode()), host=True)

    def series_load(self, path):
        """restore a series_save file into the open series (series_begin with the options of the run first); restores the route too"""
        check(self.lib.detsdw_series_load(self.h, str(path).encode()), host=True)

    def series_is_open(self):
        return self._series_open

    def series_route(self, slots=None):
        """slots = a permutation of range(len(self)): from now on the sample of chain c goes to series slot slots[c] (a slot is what the
        series readers index; under replica exchange keep slots = the chains' control parameter indices and row s is parameter s).
        May change between any two sweeps; series_end resets it to the identity.  No argument: returns the current route"""
        n = len(self.chains)
        if slots is None:
            out = (C.c_int * n)()
            check(self.lib.detsdw_series_get_route(self.h, out), host=True)
            return list(out)
        slots = [int(s) for s in slots]
        if len(slots) != n:
            raise ValueError("series_route needs one slot per chain of the batch")
        check(self.lib.detsdw_series_route(self.h, (C.c_int * n)(*slots)), host=True)

    def series_info(self):
        """(bins closed, sweeps in the open bin, doubles per sample)"""
        a, b, s = C.c_int(0), C.c_int(0), C.c_size_t(0)
        check(self.lib.detsdw_series_info(self.h, C.byref(a), C.byref(b), C.byref(s)), host=True)
        return a.value, b.value, s.value

    def series_stats_all(self, name):
        """DetSDW.series_stats of every chain: (mean, err), (nchains,) + the per-chain shape each; one device call per sub-batch"""
        which, shape, cplx = self.chains[0]._series_shape(name)
        mean, err = (np.zeros((len(self.chains),) + shape, dtype=np.complex128 if cplx else np.float64) for _ in range(2))
        check(self.lib.detsdw_series_stats_all(self.h, which, mean.ctypes.data_as(_lib._DP), err.ctypes.data_as(_lib._DP)), host=True)
        return mean, err

    def series_derived_all(self, name, Q=None):
        """(value, err) per chain of a jackknifed derived quantity: the correlation ratios 'R_charge', 'R_spinZ', 'R_sdw',
        'R_pairPlus', 'R_pairMinus' (equalTimeCorrelators) or 'rhoS' (timeDisplacedCurrent with timeDisplacedEverySlice);
        'R_custom{c}' / 'R_customPair{c}': the correlation ratio of custom bilinear / pair operator c at Q = (qx, qy) in units of
        2 pi / L, default (L/2, L/2); with set_green_matrix and pair operators set before the series began, at a Q that must be given
        ((0, 0) for uniform pairing; ValueError without it: the default of the R_ names would be the wrong one here):
        'vertexCustomPair{c}' (P = Re chi(Q, i omega_0)), 'bubbleCustomPair{c}' (Pbar, the same contraction on the averaged Green's function),
        'gammaCustomPair{c}' (Gamma = 1/P - 1/Pbar) and 'gammaBubbleCustomPair{c}' (Gamma Pbar = Pbar/P - 1; -> -1 at the instability);
        the same for custom bilinear c (particle-hole channels, Q must be given as well): 'vertexCustom{c}' (chi = Re chi(Q, i omega_0) - D),
        'bubbleCustom{c}' (chibar), 'gammaCustom{c}', 'gammaBubbleCustom{c}' and 'disconnectedCustom{c}' (D = beta Re(obar^2) sum_d cos(Q d))"""
        pv = pair_vertex_quantity(name)
        if pv is not None:
            v, e = self._series_pair_vertex(pv[1], Q)
            return v[:, pv[0]].copy(), e[:, pv[0]].copy()
        pv = ph_vertex_quantity(name)
        if pv is not None:
            v, e = self._series_ph_vertex(pv[1], Q)
            return v[:, pv[0]].copy(), e[:, pv[0]].copy()
        v, e = np.zeros(len(self.chains)), np.zeros(len(self.chains))
        c = custom_ratio(name)
        if c is not None:
            L = self.chains[0].info.L
            qx, qy = (L // 2, L // 2) if Q is None else Q
            check(self.lib.detsdw_series_custom_derived(self.h, c, int(qx), int(qy), v.ctypes.data_as(_lib._DP),
                                                        e.ctypes.data_as(_lib._DP)), host=True)
            return v, e
        c = custom_pair_ratio(name)
        if c is not None:                                   # 'R_customPair{c}': the same for pair operator c
            L = self.chains[0].info.L
            qx, qy = (L // 2, L // 2) if Q is None else Q
            check(self.lib.detsdw_series_custom_pair_derived(self.h, c, int(qx), int(qy), v.ctypes.data_as(_lib._DP),
                                                             e.ctypes.data_as(_lib._DP)), host=True)
            return v, e
        if Q is not None:
            raise ValueError("Q belongs to 'R_custom{c}'")
        check(self.lib.detsdw_series_derived_all(self.h, SERIES_DERIVED[name], v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)), host=True)
        return v, e

    def series_end(self):
        check(self.lib.detsdw_series_end(self.h), host=True)
        self._series_open = False

    def exchange_actions_device(self, device_ptr):
        """get_exchange_action_contribution of EVERY chain written to device memory (len(self) doubles at device_ptr, e.g.
        torch_tensor.data_ptr()): the send buffer of the replica-exchange all_gather, no host hop"""
        check(self.lib.detsdw_exchange_actions_device(self.h, C.c_void_p(int(device_ptr))), host=True)

    @property
    def kernel_context(self):
        """the kernel context of chain 0 (the only one unless the batch has several sub-batches)"""
        return self.chains[0].kernel_context

    def kernel_contexts(self):
        """one view per sub-batch"""
        per = len(self.chains) // self.sub_batches
        return [self.chains[g * per].kernel_context for g in range(self.sub_batches)]

    def close(self):
        if self.h:
            for c in self.chains:
                c.h = None
            self.lib.detsdw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class HubbardParams:
    """ModelParams<DetHubbard> (reference src/dethubbardparams.h:28-50)"""
    L: int = 4
    d: int = 2
    beta: float = 0.0
    m: int = 0
    dtau: float = 0.1
    s: int = 10
    t: float = 1.0
    U: float = 4.0
    mu: float = 0.0
    checkerboard: bool = False
    rngSeed: int = 1020304050
    simindex: int = 0
    device: int = 0
    stabilisation: str = "svd"
    equalTimeCorrelators: bool = False        # measurement sweeps also bin the '...Corr' observables on every time slice
    timeDisplacedCorrelators: bool = False    # ... and the '...Tau' observables at the interior boundaries tau_j = j s dtau
    timeDisplacedEverySlice: bool = False     # ... and the '...TauFine' observables on every time slice tau_k = k dtau, k = 0 .. m (needs the line above)


# DetHubbard.observable_vector: row of the equal-time block (N,) / of every boundary's rows of the time-displaced block (n-1, N)
HUBBARD_EQ_CORRELATORS = {"greenUpCorr": 0, "greenDnCorr": 1, "chargeCorr": 2, "spinZZCorr": 3, "spinXXCorr": 4, "pairSCorr": 5,
                          "pairSxCorr": 6, "pairDCorr": 7}
HUBBARD_TD_CORRELATORS = {"greenUpTau": 0, "greenDnTau": 1, "chargeTau": 2, "spinZZTau": 3, "spinXXTau": 4, "pairSTau": 5}
# '...TauFine': all eight channels on every time slice (m+1, N); their Matsubara transforms go by the '...Tau' name
HUBBARD_TD_FINE_CORRELATORS = {n[:-4] + "TauFine": x for n, x in HUBBARD_EQ_CORRELATORS.items()}
HUBBARD_MATSUBARA = {n[:-4] + "Tau": x for n, x in HUBBARD_EQ_CORRELATORS.items()}
HUBBARD_SCALARS = ("occUp", "occDn", "occTotal", "occDouble", "localMoment", "eKinetic", "ePotential", "eTotal")
# DetHubbard.series_*: name -> observable index of dethubbard_series_* ('...Sq' = S_X(q) of '...Corr', '...TauSq' of '...Tau')
HUBBARD_SERIES_OBS = {"scalars": _lib.DETHUBBARD_OBS_SCALARS, "zcorr": _lib.DETHUBBARD_OBS_ZCORR}
for _n, _x in HUBBARD_EQ_CORRELATORS.items():
    HUBBARD_SERIES_OBS[_n] = _lib.DETHUBBARD_OBS_GREENUPCORR + _x
    HUBBARD_SERIES_OBS[_n[:-4] + "Sq"] = _lib.DETHUBBARD_OBS_GREENUPSQ + _x
for _n, _x in HUBBARD_TD_CORRELATORS.items():
    HUBBARD_SERIES_OBS[_n] = _lib.DETHUBBARD_OBS_GREENUPTAU + _x
    HUBBARD_SERIES_OBS[_n + "Sq"] = _lib.DETHUBBARD_OBS_GREENUPTAUSQ + _x
# DetHubbard.series_derived_all: name -> entry of dqmc_series_hubbard_derived_host; the channels whose default Q is (L/2, L/2)
HUBBARD_SERIES_DERIVED = {"S_spin": 16, "R_spin": 17, "xi_spin": 18}
for _n, _x in HUBBARD_EQ_CORRELATORS.items():
    HUBBARD_SERIES_DERIVED["R_" + _n[:-4]] = _x
    HUBBARD_SERIES_DERIVED["xi_" + _n[:-4]] = 8 + _x
HUBBARD_Q_PI_PI = ("charge", "spinZZ", "spinXX", "spin")


def _hubbard_host_params(pars: HubbardParams):
    """the dethubbard_params that DetHubbard hands to dethubbard_create"""
    flags = ((_lib.DETHUBBARD_MEASURE_EQ if pars.equalTimeCorrelators else 0) | (_lib.DETHUBBARD_MEASURE_TD if pars.timeDisplacedCorrelators else 0)
             | (_lib.DETHUBBARD_MEASURE_TD_FINE if pars.timeDisplacedEverySlice else 0))
    return _lib.dethubbard_params(L=pars.L, d=pars.d, m=pars.m, s=pars.s, checkerboard=int(pars.checkerboard), device=pars.device,
                                  simindex=pars.simindex, rngSeed=pars.rngSeed, stabilisation=STABILISATION[pars.stabilisation],
                                  measureFlags=flags, beta=pars.beta, dtau=pars.dtau, t=pars.t, U=pars.U, mu=pars.mu)


class DetHubbard(_GreenCheck):
    """The Hubbard replica of BASELINE config 1 (C++ host layer detqmc_amd/csrc/host/dethubbard.cpp): the reference's
    DetHubbard (src/dethubbard.{h,cpp}) with both spin sectors in one block-diagonal Green's function on the GPU.
    nchains > 1: independent replicas (simindex, simindex + 1, ...) in lockstep; `select(b)` picks the one the getters
    talk to."""

    def __init__(self, pars: HubbardParams, nchains=1):
        self.lib = load()
        self.pars = pars
        p = _hubbard_host_params(pars)
        h = C.c_void_p()
        check(self.lib.dethubbard_create(C.byref(p), nchains, C.byref(h)), host="hubbard")
        self.h = h
        self.nchains = nchains

    def close(self):
        if self.h:
            self.lib.dethubbard_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def select(self, b):
        check(self.lib.dethubbard_select_chain(self.h, b), host="hubbard")

    _gc_calls = ("dethubbard_set_green_check", "dethubbard_get_green_check", "dethubbard_reset_green_check", "hubbard")

    def _gc_shape(self):
        i = self.info
        return self.nchains, i.n, 2 * i.N

    def sweep(self, takeMeasurements=False):
        check(self.lib.dethubbard_sweep(self.h, int(takeMeasurements)), host="hubbard")

    def sweepThermalization(self):
        check(self.lib.dethubbard_sweep_thermalization(self.h), host="hubbard")

    @property
    def info(self):
        i = _lib.dethubbard_info()
        check(self.lib.dethubbard_get_info(self.h, C.byref(i)), host="hubbard")
        return i

    @property
    def auxfield(self):
        """(N, m+1) like the reference's MatInt auxfield, as +-1.0 (column 0 unused)"""
        i = self.info
        a = np.zeros((i.N, i.m + 1), order="F")
        check(self.lib.dethubbard_get_auxfield(self.h, a.ctypes.data_as(_lib._DP)), host="hubbard")
        return a

    @property
    def green(self):
        """(gUp, gDn), N x N each"""
        n = self.info.N
        gu, gd = np.zeros((n, n), order="F"), np.zeros((n, n), order="F")
        check(self.lib.dethubbard_get_green(self.h, gu.ctypes.data_as(_lib._DP), gd.ctypes.data_as(_lib._DP)), host="hubbard")
        return gu, gd

    @property
    def observables(self):
        o = _lib.dethubbard_observables()
        check(self.lib.dethubbard_get_observables(self.h, C.byref(o)), host="hubbard")
        return o

    @property
    def zcorr(self):
        out = np.zeros(self.info.N)
        check(self.lib.dethubbard_get_zcorr(self.h, out.ctypes.data_as(_lib._DP)), host="hubbard")
        return out

    def observable_vector(self, name):
        """C(d) of the last measurement sweep, selected chain, index dy L + dx over the periodic site differences.
        HubbardParams.equalTimeCorrelators: 'greenUpCorr', 'greenDnCorr', 'chargeCorr', 'spinZZCorr', 'spinXXCorr', 'pairSCorr', 'pairSxCorr',
        'pairDCorr', shape (N,), averaged over the m time slices.  HubbardParams.timeDisplacedCorrelators: 'greenUpTau', 'greenDnTau',
        'chargeTau', 'spinZZTau', 'spinXXTau', 'pairSTau', shape (n-1, N), rows = tau_grid().  structure_factor(c, L) turns either into
        S(q) (e.g. the antiferromagnetic S(pi, pi) from 'spinZZCorr', n(k) from 'greenUpCorr').  HubbardParams.timeDisplacedEverySlice:
        'greenUpTauFine', 'greenDnTauFine', 'chargeTauFine', 'spinZZTauFine', 'spinXXTauFine', 'pairSTauFine', 'pairSxTauFine', 'pairDTauFine',
        shape (m+1, N), rows = tau_grid(fine=True)."""
        i = self.info
        if name in HUBBARD_EQ_CORRELATORS:
            out = np.zeros((8, i.N))
            check(self.lib.dethubbard_get_eq_correlators(self.h, out.ctypes.data_as(_lib._DP)), host="hubbard")
            return out[HUBBARD_EQ_CORRELATORS[name]].copy()
        if name in HUBBARD_TD_CORRELATORS:
            out = np.zeros((i.n - 1, 6, i.N))
            check(self.lib.dethubbard_get_td_correlators(self.h, out.ctypes.data_as(_lib._DP)), host="hubbard")
            return out[:, HUBBARD_TD_CORRELATORS[name], :].copy()
        if name in HUBBARD_TD_FINE_CORRELATORS:
            out = np.zeros((i.m + 1, 8, i.N))
            check(self.lib.dethubbard_get_td_fine_correlators(self.h, out.ctypes.data_as(_lib._DP)), host="hubbard")
            return out[:, HUBBARD_TD_FINE_CORRELATORS[name], :].copy()
        raise KeyError(name)

    def tau_grid(self, fine=False):
        """tau_j = j s dtau, j = 1 .. n-1: the rows of the '...Tau' observables; fine=True: tau_k = k dtau, k = 0 .. m, the rows of '...TauFine'"""
        i = self.info
        if fine:
            return np.arange(i.m + 1) * i.dtau
        return np.arange(1, i.n) * (i.s * i.dtau)

    def matsubara(self, name, nfreq):
        """Matsubara transform of the every-slice rows of the last measurement sweep, selected chain, complex (nfreq, N), column qy L + qx
        (HubbardParams.timeDisplacedEverySlice; trapezoid rule over tau_grid(fine=True)).  'chargeTau', 'spinZZTau', 'spinXXTau', 'pairSTau',
        'pairSxTau', 'pairDTau': chi_X(q, i omega_n) at the bosonic frequencies -- the spin susceptibility chi_s(pi, pi; 0) is
        matsubara('spinZZTau', 1)[0, (L // 2) * L + L // 2], the pair susceptibilities P_s, P_d(q = 0; 0) are column 0 of 'pairSxTau' /
        'pairDTau'; 'greenUpTau', 'greenDnTau': G_s(k, i omega_n) at the fermionic ones.  Valid until the next sweep of either kind"""
        at = HUBBARD_MATSUBARA[name]
        out = np.zeros((8, int(nfreq), self.info.N), dtype=np.complex128)
        check(self.lib.dethubbard_get_matsubara(self.h, int(nfreq), out.ctypes.data_as(_lib._DP)), host="hubbard")
        return out[at].copy()

    def matsubara_all(self, name, nfreq):
        """matsubara of every chain, complex (nchains, nfreq, N); one device call"""
        at = HUBBARD_MATSUBARA[name]
        out = np.zeros((self.nchains, 8, int(nfreq), self.info.N), dtype=np.complex128)
        check(self.lib.dethubbard_get_matsubara_all(self.h, int(nfreq), out.ctypes.data_as(_lib._DP)), host="hubbard")
        return out[:, at].copy()

    def matsubara_frequencies(self, nfreq, fermionic=False):
        """omega_n, n = 0 .. nfreq-1: 2 pi n / beta, or (2n+1) pi / beta with fermionic=True"""
        n = np.arange(int(nfreq))
        return (2 * n + 1) * np.pi / self.info.beta if fermionic else 2 * n * np.pi / self.info.beta

    def rand01(self):
        return self.lib.dethubbard_rng_rand01(self.h)

    def save_state(self, path):
        check(self.lib.dethubbard_save_state(self.h, str(path).encode()), host="hubbard")

    # ---- measurement series: bins over measurement sweeps and jackknife errors on the device ----
    def series_begin(self, binSize, maxBins, host_copy=True, auto_rebin=False, track_variance=False):
        """open a measurement series on the device: from now on every sweep(True) adds one sample per chain -- 'scalars' (the eight of
        `observables`, in that order) and 'zcorr' always, the '...Corr' vectors and their structure factors '...Sq' with
        equalTimeCorrelators, the '...Tau' rows and '...TauSq' ('greenUpTauSq' = Re G_up(k, tau_j)) with timeDisplacedCorrelators -- to bins
        of binSize sweeps, at most maxBins of them.  host_copy=False: measurement sweeps no longer copy the correlator blocks to the host
        (the '...Corr' / '...Tau' names of observable_vector raise while the series is open; observables and zcorr stay).
        auto_rebin: whenever maxBins (even, >= 4) bins are closed, neighbouring bins are merged; track_variance: keep the variance of
        the single samples, which series_binning_all needs for tau"""
        flags = 0 if host_copy else _lib.DETHUBBARD_SERIES_NO_HOST_COPY
        check(self.lib.dethubbard_series_begin(self.h, int(binSize), int(maxBins), flags), host="hubbard")
        self._series_open = True
        if auto_rebin or track_variance:
            opts = (_lib.DQMC_SERIES_AUTO_REBIN if auto_rebin else 0) | (_lib.DQMC_SERIES_TRACK_VARIANCE if track_variance else 0)
            try:
                check(self.lib.dethubbard_series_configure(self.h, opts), host="hubbard")
            except _lib.DqmcError:
                self.lib.dethubbard_series_end(self.h)     # refused options: no half-configured series stays open
                self._series_open = False
                raise

    def series_is_open(self):
        return getattr(self, "_series_open", False)

    def series_info(self):
        """(bins closed, sweeps in the open bin, doubles per sample)"""
        a, b, s = C.c_int(0), C.c_int(0), C.c_size_t(0)
        check(self.lib.dethubbard_series_info(self.h, C.byref(a), C.byref(b), C.byref(s)), host="hubbard")
        return a.value, b.value, s.value

    def _series_shape(self, name):
        """(observable index, per-chain shape) of a series name"""
        if name not in HUBBARD_SERIES_OBS:
            raise KeyError(name)
        i = self.info
        if name == "scalars":
            return HUBBARD_SERIES_OBS[name], (8,)
        if name.endswith("Tau") or name.endswith("TauSq"):
            return HUBBARD_SERIES_OBS[name], (max(i.n - 1, 0), i.N)
        return HUBBARD_SERIES_OBS[name], (i.N,)

    def series_stats(self, name):
        """(mean, err) of a series observable over the closed bins, jackknife, selected chain"""
        which, shape = self._series_shape(name)
        mean, err = np.zeros(shape), np.zeros(shape)
        check(self.lib.dethubbard_series_stats(self.h, which, mean.ctypes.data_as(_lib._DP), err.ctypes.data_as(_lib._DP)), host="hubbard")
        return mean, err

    def series_stats_all(self, name):
        """series_stats of every chain: (mean, err), (nchains,) + the per-chain shape each; one device call"""
        which, shape = self._series_shape(name)
        mean, err = np.zeros((self.nchains,) + shape), np.zeros((self.nchains,) + shape)
        check(self.lib.dethubbard_series_stats_all(self.h, which, mean.ctypes.data_as(_lib._DP), err.ctypes.data_as(_lib._DP)), host="hubbard")
        return mean, err

    def series_bins(self, name, first=0, count=None):
        """closed bins first .. first + count - 1 (default: all from first) of a series observable, selected chain: (count,) + shape"""
        which, shape = self._series_shape(name)
        count = self.series_info()[0] - first if count is None else int(count)
        out = np.zeros((max(count, 0),) + shape)
        check(self.lib.dethubbard_series_read_bins(self.h, which, int(first), count, out.ctypes.data_as(_lib._DP)), host="hubbard")
        return out

    def series_derived_all(self, name, Q=None):
        """(value, err) per chain of a jackknifed derived quantity of the equal-time structure factors at Q = (qx, qy) in units of
        2 pi / L: 'R_<channel>' = 1 - Sbar / S(Q) with Sbar = [S(Q + dx) + S(Q + dy)] / 2, 'xi_<channel>' = sqrt(S(Q) / Sbar - 1) /
        (2 sin(pi / L)) for channel in greenUp, greenDn, charge, spinZZ, spinXX, pairS, pairSx, pairD, and 'S_spin', 'R_spin', 'xi_spin'
        of the rotation-summed spin channel spinZZ + 2 spinXX.  Default Q: (L/2, L/2) for charge, spinZZ, spinXX and spin, (0, 0) for the
        Green and pairing channels.  NaN where the root's argument is negative or a denominator vanishes"""
        at = HUBBARD_SERIES_DERIVED[name]
        if Q is None:
            L = self.info.L
            Q = (L // 2, L // 2) if name.split("_", 1)[1] in HUBBARD_Q_PI_PI else (0, 0)
        v, e = np.zeros((self.nchains, 19)), np.zeros((self.nchains, 19))
        check(self.lib.dethubbard_series_derived_all(self.h, int(Q[0]), int(Q[1]), v.ctypes.data_as(_lib._DP), e.ctypes.data_as(_lib._DP)), host="hubbard")
        return v[:, at].copy(), e[:, at].copy()

    def series_binning_all(self, name, levels):
        """binning analysis of every chain: (err, tau), (nchains, levels) + the per-chain shape each -- the jackknife error over the bins
        merged l times and the integrated autocorrelation time in sweeps it implies; tau is None without track_variance"""
        which, shape = self._series_shape(name)
        full = (self.nchains, max(int(levels), 0)) + shape
        err = np.zeros(full)
        tau = np.zeros(full) if self.series_state().flags & _lib.DQMC_SERIES_TRACK_VARIANCE else None
        check(self.lib.dethubbard_series_binning_all(self.h, which, int(levels), err.ctypes.data_as(_lib._DP),
                                                     tau.ctypes.data_as(_lib._DP) if tau is not None else None), host="hubbard")
        return err, tau

    def series_rebin(self):
        """merge neighbouring closed bins of every chain: half as many bins of twice the size"""
        check(self.lib.dethubbard_series_rebin(self.h), host="hubbard")

    def series_state(self):
        """the dqmc_series_state of the open series"""
        st = _lib.dqmc_series_state()
        check(self.lib.dethubbard_series_get_state(self.h, C.byref(st)), host="hubbard")
        return st

    def series_save(self, path):
        """the whole series -- bins, open bin, counters, variance -- to a file of its own, next to save_state"""
        check(self.lib.dethubbard_series_save(self.h, str(path).encode()), host="hubbard")

    def series_load(self, path):
        """restore a series_save file into the open series (series_begin with the options of the run first)"""
        check(self.lib.dethubbard_series_load(self.h, str(path).encode()), host="hubbard")

    def series_end(self):
        check(self.lib.dethubbard_series_end(self.h), host="hubbard")
        self._series_open = False

    def load_state(self, path):
        check(self.lib.dethubbard_load_state(self.h, str(path).encode()), host="hubbard")
