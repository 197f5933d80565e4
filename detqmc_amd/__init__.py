"""detqmc_amd -- MI355X-native DQMC sweep engine (hot path of crstnbr/detqmc).

Python only binds the C ABI (include/dqmc_hip.h) and the C++ host layer (include/detsdw_host.h)
for tests and the benchmark harness; the product is the shared library.
"""
from ._lib import DqmcError, load, LIB_PATH  # noqa: F401
from .model import HUBBARD_SERIES_DERIVED, HUBBARD_SERIES_OBS, DetHubbard, DetSDW, DetSDWBatch, HubbardParams, KernelContext, SDWParams, binning_analysis, bond_current, bond_kinetic, green_check_decode, green_check_worst, jackknife, pair_bubble, pair_operator, ph_bubble, ph_one_body, phi_sample, structure_factor, superfluid_stiffness  # noqa: F401
