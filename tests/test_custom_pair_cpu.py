"""User-defined pair operators, the part that needs no GPU: the Wick form of tests/custom_pair_reference.py against exact
diagonalisation, the link to the fixed channels pairPlus / pairMinus, the antisymmetry of F0, inputs on which the GPU comparison cannot
pass with a dropped conjugate, and the entry points in the built library and the Python layer.  Every test prints its figures before it
asserts."""
import ctypes as C

import numpy as np
import pytest

import custom_pair_reference as cp

# (opdim, L, checkerboard, bc, flux): KERNEL_CASES of tests/test_gpu_band_correlators.py, the cases of the GPU kernel test (m = 20, s = 5)
GPU_CASES = [(1, 4, True, "pbc", False), (2, 4, True, "pbc", False), (3, 4, True, "pbc", False), (2, 4, True, "apbc-xy", False),
             (2, 4, False, "pbc", False), (3, 4, False, "pbc", False), (2, 4, True, "pbc", True), (2, 6, True, "pbc", False),
             (3, 6, True, "pbc", False)]


def _inputs(opdim, L=4, m=20, s=5, tau=10, bc="pbc", flux=False, checkerboard=True):
    """an oracle and its shifted (G(tau), G(tau,0)) at tau: fields uniform(-1, 1) with the seed of the GPU kernel test"""
    from td_ph_reference import four_greens
    from td_reference import Chain, make_oracle, shift_symmetric
    phi = np.random.default_rng(300 * opdim + L + m).uniform(-1.0, 1.0, (m + 1, L * L, opdim))
    phi[0] = 0.0
    ora = make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, bc=bc, checkerboard=checkerboard, weakZflux=flux, delaySteps=4)
    return ora, [shift_symmetric(ora, g) for g in four_greens(Chain(ora), tau)[:2]]


@pytest.mark.parametrize("nfac,cut", [(4, 2), (5, 1), (6, 4)])
def test_wick_form_against_exact_diagonalisation(nfac, cut):
    """8 modes, 256-dimensional Fock space, U = prod_k exp(-c^+ h_k c); dense random complex D_A != D_B:
    <Delta_A(tau) Delta_B^+(0)> = Tr[U_n .. U_(cut+1) Delta_A U_cut .. U_1 Delta_B^+] / Tr[U] against the Wick form on G(tau,0), and
    Tr[U Delta_A Delta_B^+] / Tr[U] against the same form on G(0).  Bound 1e-11, the bound of the existing ED tests."""
    from td_ph_reference import greens_from_b
    from test_td_particle_hole_cpu import _exp_herm, _fock_operators
    nm = 8
    rng = np.random.default_rng(700 * nfac + cut)
    c = _fock_operators(nm)
    cd = [x.conj().T for x in c]
    hs = []
    for _ in range(nfac):
        h = rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm))
        h = 0.5 * (h + h.conj().T)
        hs.append(h / np.linalg.norm(h, 2))
    Us = [_exp_herm(sum(h[a, b] * cd[a] @ c[b] for a in range(nm) for b in range(nm))) for h in hs]
    Bs = [_exp_herm(h) for h in hs]

    def prod(fs, lo, hi, dim):
        out = np.eye(dim, dtype=complex)
        for k in range(lo, hi):
            out = fs[k] @ out
        return out

    Ur, Ul = prod(Us, 0, cut, 2 ** nm), prod(Us, cut, nfac, 2 ** nm)
    _, gt0, _, g00 = greens_from_b(prod(Bs, 0, cut, nm), prod(Bs, cut, nfac, nm))
    Z = np.trace(Ul @ Ur)
    DA, DB = [rng.normal(size=(nm, nm)) + 1j * rng.normal(size=(nm, nm)) for _ in range(2)]
    dA = sum(DA[i, j] * c[i] @ c[j] for i in range(nm) for j in range(nm))
    dBh = sum(DB[i, j] * c[i] @ c[j] for i in range(nm) for j in range(nm)).conj().T
    e_td = abs(np.trace(Ul @ dA @ Ur @ dBh) / Z - cp.pair_wick_all(gt0, DA[None], DB[None])[0, 0])
    e_eq = abs(np.trace(Ul @ Ur @ dA @ dBh) / Z - cp.pair_wick_all(g00, DA[None], DB[None])[0, 0])
    print(f"{nfac} factors, cut {cut}: |ED - Wick| time-displaced {e_td:.2e}, equal-time {e_eq:.2e}")
    assert e_td < 1e-11 and e_eq < 1e-11


@pytest.mark.parametrize("opdim", [1, 2, 3])
def test_fixed_channels(opdim):
    """4 P(A, B) of the operators 's' and 'd_band' is T+-(A, B) of tests/td_pair_reference.py, every site pair: 1e-13"""
    from detqmc_amd import pair_operator
    from td_pair_reference import pair_terms
    from td_ph_reference import expand
    ora, (gtt, gt0) = _inputs(opdim)
    u = cp.link_signs(ora.L)
    for gs in (gt0, gtt):
        plus, minus = pair_terms(ora, gs)
        g = expand(ora, gs)
        for kind, ref in (("s", plus), ("d_band", minus)):
            P = cp.pair_wick_all(g, cp.dense_pair_operators(pair_operator(kind), u, ora.L))
            e = np.abs(4.0 * P - ref).max()
            print(f"O({opdim}) {kind}: max |4 P - T| = {e:.2e}, max |T| = {np.abs(ref).max():.3f}")
            assert np.abs(ref).max() > 1e-3 and e < 1e-13
    assert np.array_equal(cp.P_S[0], pair_operator("s")[0]) and np.array_equal(cp.P_DBAND[0], pair_operator("d_band")[0])
    S = pair_operator("s_ext")[1]
    assert np.array_equal(S, -S.T) and np.array_equal(pair_operator("s_ext")[2], S) and np.array_equal(pair_operator("d_bond")[2], -S)
    assert pair_operator("s_ext")[0] is None and np.array_equal(pair_operator("d_bond")[1], S) and np.array_equal(S, cp._singlet())
    with pytest.raises(ValueError):
        pair_operator("p")


@pytest.mark.parametrize("opdim", [2, 3])
def test_only_the_antisymmetric_part_of_f0_contributes(opdim):
    """adding a symmetric matrix to F0 changes nothing (1e-13 of the largest |P|), and an F0 with zero antisymmetric part gives exactly
    zero"""
    from td_ph_reference import expand
    ora, (_, gt0) = _inputs(opdim)
    g, u = expand(ora, gt0), cp.link_signs(ora.L)
    F0, Fx, Fy = cp.P_RAND
    sym = cp.P_SYM_BOND[0]
    assert np.array_equal(sym, sym.T)
    base = cp.pair_wick_all(g, cp.dense_pair_operators((F0, Fx, Fy), u, ora.L))
    more = cp.pair_wick_all(g, cp.dense_pair_operators((F0 + sym, Fx, Fy), u, ora.L))
    anti = cp.pair_wick_all(g, cp.dense_pair_operators((0.5 * (F0 - F0.T), Fx, Fy), u, ora.L))
    zero = cp.pair_wick_all(g, cp.dense_pair_operators((sym, None, None), u, ora.L))
    e = max(np.abs(more - base).max(), np.abs(anti - base).max()) / np.abs(base).max()
    print(f"O({opdim}): symmetrised F0 moves P by {e:.2e} of max |P| = {np.abs(base).max():.3f}; symmetric F0 alone: max |P| = {np.abs(zero).max():.1e}")
    assert e < 1e-13 and not zero.any()


@pytest.mark.parametrize("opdim,L,checkerboard,bc,flux", [c for c in GPU_CASES if c[0] == 2])
def test_a_dropped_conjugate_cannot_pass(opdim, L, checkerboard, bc, flux):
    """on the GPU kernel test's inputs the dense operator's C(d), time-displaced and equal-time, changes by more than 1e-3 of its
    largest entry when the conjugation of the second sector is dropped from the reference's expand: a kernel that puts the conjugate
    in the wrong place cannot pass at 1e-10.  O(2) only: O(3) stores the full matrix (no sector rule) and the O(1) matrices are real
    (the conjugate is the identity there, so there is nothing to drop).  Every reference row is also far above the 1e-6 floor the GPU test asserts.
    Measured: the change is between 1.7e-3 (L = 6, time-displaced) and 2.7e-2 (flux, equal-time) of the largest entry over the five
    cases, seven orders of magnitude above the GPU test's bound."""
    ora, gs = _inputs(opdim, L=L, bc=bc, flux=flux, checkerboard=checkerboard)
    ops = cp.pair_ops(flux)
    u = cp.link_signs(ora.L, bc)
    for name, g in zip(("equal-time", "time-displaced"), gs):
        ref = cp.pair_correlators(ora, ops, g)
        bad = cp.pair_correlators_full(ops[:1], u, L, cp.expand_unconjugated(ora, g))[0]
        change = np.abs(bad - ref[0]).max() / np.abs(ref[0]).max()
        print(f"O({opdim}) L={L} {bc} cb={checkerboard} flux={flux} {name}: dropped conjugate moves C(d) by {change:.3e} of max |C|; "
              f"max |C| {['%.3f' % np.abs(r).max() for r in ref]}")
        assert change > 1e-3
        assert min(np.abs(r).max() for r in ref) > 1e-6


def test_library_and_python_layer_carry_the_entry_points():
    """the new symbols are exported and bound, NULL handles are refused, no struct changed its size, the constants have their values,
    and the names parse"""
    import detqmc_amd
    from detqmc_amd import DetSDWBatch, KernelContext, _lib, model
    lib = _lib.load()
    bound = {s[0] for s in _lib.SYMBOLS}
    for sym in ("dqmc_set_custom_pair_operators", "dqmc_get_custom_pair_operators", "dqmc_measure_timedisplaced_custom_pair",
                "dqmc_measure_td_custom_pair_accum_size", "dqmc_measure_td_custom_pair_read_host", "dqmc_set_equal_time_custom_pair",
                "dqmc_measure_eq_custom_pair_accum_size", "dqmc_measure_eq_custom_pair_read_host", "dqmc_series_custom_pair_derived_host",
                "detsdw_set_custom_pair_operators", "detsdw_get_custom_pair_operators", "detsdw_series_custom_pair_derived"):
        assert hasattr(lib, sym) and sym in bound, sym
    f = np.ascontiguousarray(cp.P_RAND[0])
    n = C.c_int(5)
    out = np.zeros(4)
    dp = out.ctypes.data_as(_lib._DP)
    assert lib.dqmc_set_custom_pair_operators(None, 1, f.ctypes.data, None, None) == -1
    assert lib.dqmc_get_custom_pair_operators(None, C.byref(n), None, None, None) == -1 and n.value == 5
    assert lib.dqmc_measure_timedisplaced_custom_pair(None, 1) == -1 and lib.dqmc_set_equal_time_custom_pair(None, 1) == -1
    assert lib.dqmc_measure_td_custom_pair_accum_size(None) == 0 and lib.dqmc_measure_eq_custom_pair_accum_size(None) == 0
    assert lib.dqmc_measure_td_custom_pair_read_host(None, dp) == -1 and lib.dqmc_measure_eq_custom_pair_read_host(None, dp) == -1
    assert lib.dqmc_series_custom_pair_derived_host(None, 0, 0, dp, dp) == -1 and not out.any()
    assert lib.detsdw_set_custom_pair_operators(None, 1, f.ctypes.data, None, None) == -1
    assert lib.detsdw_get_custom_pair_operators(None, C.byref(n), None, None, None) == -1 and n.value == 5
    assert lib.detsdw_series_custom_pair_derived(None, 0, 0, 0, dp, dp) == -1
    assert C.sizeof(_lib.dqmc_params) == 192 and C.sizeof(_lib.detsdw_params) == 264 and C.sizeof(_lib.dqmc_series_state) == 56
    assert (_lib.DQMC_SERIES_MATS_CUSTOM_PAIR, _lib.DQMC_SERIES_EQ_CUSTOM_PAIR) == (2048, 4096) == (model.SERIES_MATS_CUSTOM_PAIR, model.SERIES_EQ_CUSTOM_PAIR)
    assert (_lib.DQMC_SERIES_MATS_CUSTOM, _lib.DQMC_SERIES_EQ_CUSTOM, _lib.DQMC_CUSTOM_MAX) == (512, 1024, 4)
    assert model.CUSTOM_PAIR_OBS_BASE == {"Tau": 58, "TauQ0": 62, "Corr": 66, "Sq": 70}
    for cls in (KernelContext, DetSDWBatch):
        for name in ("set_custom_pair_operators", "get_custom_pair_operators"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(detqmc_amd.pair_operator)
    # the names
    for c in range(4):
        for kind, base in model.CUSTOM_PAIR_OBS_BASE.items():
            assert model.custom_pair_observable(f"customPair{c}{kind}") == (kind, base + c)
            assert model.custom_observable(f"customPair{c}{kind}") is None
        assert model.custom_pair_ratio(f"R_customPair{c}") == c and model.custom_ratio(f"R_customPair{c}") is None
    for bad in ("custom0Tau", "customPair4Tau", "customPairTau", "customPair0", "customPair0tau", "customPair0TauFine", "customPair-1Sq",
                "customPair0CorrX", "xcustomPair0Corr", "pairPlusTau", "customPair00Sq", ""):
        assert model.custom_pair_observable(bad) is None, bad
    for bad in ("R_custom0", "R_customPair4", "R_customPair", "customPair0", "R_pairPlus"):
        assert model.custom_pair_ratio(bad) is None, bad
    assert model.custom_observable("custom0Tau") == ("Tau", 42)
