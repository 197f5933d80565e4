"""Matsubara transforms chi(q, i omega_n), G(k, i omega_n) of the every-slice blocks on the device (dqmc_measure_td_matsubara_host,
DetSDW.matsubara): against the numpy restatement applied to the same sweep's '...Fine' vectors, call behaviour, timeDisplacedFineOnDevice
and the error paths.

Tolerance of the comparisons: 1e-10 (max-norm relative error over the whole (nfreq, N) array), the project's parity tolerance -- both
sides sum the same <= (m+1) (2L-1)^2 terms of order one in fp64, in a different order.  Every comparison prints its figure first."""
import dataclasses
import hashlib

import numpy as np
import pytest

import td_matsubara_reference as tm
from conftest import relerr

pytestmark = pytest.mark.gpu

ALL = list(tm.FERMIONIC) + list(tm.BOSONIC)
COARSE = ["greenKTauX", "greenKTauY", "pairPlusTau", "pairMinusTau", "pairPlusTauQ0", "pairMinusTauQ0", "chargeTau", "spinZTau",
          "sdwTau", "chargeTauQ0", "spinZTauQ0", "sdwTauQ0", "currentXTau", "currentYTau", "currentXTauQ0", "currentYTauQ0",
          "bondKineticX", "bondKineticY"]

# name -> (parameters, chains, sub-batches, names).  o2: s does not divide m, two kernel contexts, two frequency tiles (m > 8);
# o1: N = 36 (no multiple of a wave), antiperiodic in x, one tile; o3: no current block; o2L8: the bins of channel 0 (2 * 15^2 = 450
# doubles per band) need two passes of the 256 threads
CASES = {
    "o2": (dict(opdim=2, L=4, beta=1.0, s=3), 4, 2, ALL),
    "o1": (dict(opdim=1, L=6, beta=0.7, s=2, bc="apbc-x"), 3, 1, ALL),
    "o3": (dict(opdim=3, L=4, beta=1.0, s=3, timeDisplacedCurrent=False), 2, 1, ALL[:7]),
    "o2L8": (dict(opdim=2, L=8, beta=0.4, s=2), 1, 1, ALL),
}


def _batch(case, **over):
    from detqmc_amd import DetSDWBatch, SDWParams
    kw, chains, subs, _ = CASES[case]
    kw = dict(dict(dtau=0.1, delaySteps=4, updateMethod="delayed", stabilisation="qr", fermionMeasurements=True,
                   timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True, timeDisplacedCurrent=True,
                   timeDisplacedEverySlice=True, rngSeed=4711), **kw)
    kw.update(over)
    p = SDWParams(**kw)
    return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.2 * i) for i in range(chains)], sub_batches=subs)


def _run(batch):
    batch.sweepThermalization()
    batch.sweepThermalization()
    batch.sweep(True)


def _sha(batch):
    h = hashlib.sha256()
    for b in range(len(batch)):
        h.update(np.ascontiguousarray(batch.chain(b).phi).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def o2_results():
    """case o2 on the default path: per chain the transforms of every name at nfreq = m and the coarse vectors"""
    batch = _batch("o2")
    try:
        _run(batch)
        m = batch.chain(0).info.m
        return dict(m=m, mats=[{nm: batch.chain(b).matsubara(nm, m) for nm in ALL} for b in range(len(batch))],
                    coarse=[{nm: batch.chain(b).observable_vector(nm) for nm in COARSE} for b in range(len(batch))], sha=_sha(batch))
    finally:
        batch.close()


# ---- 1.-3. against numpy on the same sweep's Fine vectors ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_matches_numpy_on_the_fine_vectors(case):
    kw, chains, subs, names = CASES[case]
    batch = _batch(case)
    try:
        assert batch.sub_batches == subs
        _run(batch)
        info = batch.chain(0).info
        m, L, N = info.m, info.L, info.N
        assert m == round(kw["beta"] / 0.1)
        worst = {}
        for b in range(chains):
            rep = batch.chain(b)
            for nm in names:
                fine = rep.observable_vector(nm + "Fine")
                ref = tm.transform(nm, fine, L, 0.1, m)
                dev = rep.matsubara(nm, m)
                assert dev.shape == (m, N) and dev.dtype == np.complex128
                assert np.abs(ref).max() > 1e-6                      # not a comparison of zeros
                worst[nm] = max(worst.get(nm, 0.0), relerr(dev, ref))
        print(f"case {case}: largest relative error per observable over {chains} chains:",
              ", ".join(f"{nm} {e:.1e}" for nm, e in worst.items()), "(bound 1e-10)")
        assert max(worst.values()) <= 1e-10
        rep = batch.chain(0)
        assert np.allclose(rep.matsubara_frequencies(3), 2 * np.pi * np.arange(3) / info.beta, rtol=1e-15)
        assert np.allclose(rep.matsubara_frequencies(3, fermionic=True), (2 * np.arange(3) + 1) * np.pi / info.beta, rtol=1e-15)
        if "currentXTau" in names:
            from detqmc_amd import superfluid_stiffness
            rho = superfluid_stiffness(batch.matsubara_all("currentXTau", 1), batch.matsubara_all("currentYTau", 1), L)
            lx = tm.bosonic(rep.observable_vector("currentXTauFine"), L, 0.1, 1)[0]
            ly = tm.bosonic(rep.observable_vector("currentYTauFine"), L, 0.1, 1)[0]
            want = 0.125 * (lx[1] - lx[L] + ly[L] - ly[1]).real
            print(f"case {case}: rho_s of chain 0 from the device {rho[0]:.12e}, from numpy {want:.12e}")
            assert rho.shape == (chains,) and abs(rho[0] - want) <= 1e-10 * max(np.abs(lx).max(), np.abs(ly).max())
    finally:
        batch.close()


# ---- 4. call behaviour ---------------------------------------------------------------------------------------------------------------
def test_call_behaviour(o2_results):
    batch, twin = _batch("o2"), _batch("o2")
    try:
        _run(batch)
        _run(twin)
        chains, m = len(batch), o2_results["m"]
        before = [dict(fine={nm: batch.chain(b).observable_vector(nm + "Fine") for nm in COARSE},
                       coarse={nm: batch.chain(b).observable_vector(nm) for nm in COARSE}, g=batch.chain(b).g) for b in range(chains)]
        kcs = batch.kernel_contexts()
        per = chains // len(kcs)

        def fine_blocks():
            # the accumulator blocks of every chain of every context (the read refers to the context's selected chain, and the host
            # layer's calls below move that selection)
            out = []
            for kc in kcs:
                for b in range(per):
                    kc.select_chain(b)
                    out.append([kc.measure_td_fine_read(ch) for ch in range(4)])
            return out

        blocks = fine_blocks()
        for nm in ALL:
            every = batch.matsubara_all(nm, m)
            assert every.shape == (chains, m, 16)
            for b in range(chains):
                one = batch.chain(b).matsubara(nm, m)
                assert np.array_equal(one, o2_results["mats"][b][nm]), (nm, b)       # another batch object, the same bits
                assert np.array_equal(every[b], one), (nm, b)                        # chains in handle order across sub-batches
                assert np.array_equal(batch.chain(b).matsubara(nm, m), one)          # a second call
                assert np.array_equal(batch.chain(b).matsubara(nm, 1)[0], one[0])    # nfreq = 1 is row 0
            assert np.array_equal(batch.matsubara_all(nm, m), every)
        # the kernel itself, twice: identical bits (one writer per element, fixed order), and what the host layer handed out
        for g, kc in enumerate(kcs):
            for ch, names in enumerate((ALL[0:2], ALL[2:4], ALL[4:7], ALL[7:9])):
                first, second = kc.measure_td_matsubara(ch, m), kc.measure_td_matsubara(ch, m)
                assert first.shape == (per, len(names), m, 16)
                assert np.array_equal(first, second), (g, ch)
                assert np.array_equal(kc.measure_td_matsubara(ch, 3), first[:, :, :3]), (g, ch)
                for comp, nm in enumerate(names):
                    for b in range(per):
                        assert np.array_equal(first[b, comp], o2_results["mats"][g * per + b][nm]), (g, nm, b)
        # nothing else moved
        assert len(blocks) == chains
        for was, now in zip(blocks, fine_blocks()):
            for ch in range(4):
                assert np.array_equal(now[ch], was[ch]), ch
        for b in range(chains):
            rep = batch.chain(b)
            for nm in COARSE:
                assert np.array_equal(rep.observable_vector(nm + "Fine"), before[b]["fine"][nm]), nm
                assert np.array_equal(rep.observable_vector(nm), before[b]["coarse"][nm]), nm
            assert np.array_equal(rep.g, before[b]["g"])
        assert _sha(batch) == _sha(twin) == o2_results["sha"]
        for _ in range(2):
            batch.sweep(True)
            twin.sweep(True)
        assert _sha(batch) == _sha(twin) != o2_results["sha"]
        for b in range(chains):
            assert np.array_equal(batch.chain(b).g, twin.chain(b).g)
    finally:
        batch.close()
        twin.close()


# ---- 5. timeDisplacedFineOnDevice ------------------------------------------------------------------------------------------------------
def test_fine_on_device(o2_results):
    from detqmc_amd import DqmcError
    batch = _batch("o2", timeDisplacedFineOnDevice=True)
    try:
        _run(batch)
        m = o2_results["m"]
        assert _sha(batch) == o2_results["sha"]
        for nm in ALL:
            every = batch.matsubara_all(nm, m)
            for b in range(len(batch)):
                assert np.array_equal(every[b], o2_results["mats"][b][nm]), (nm, b)
        for b in range(len(batch)):
            rep = batch.chain(b)
            for nm in COARSE:
                assert np.array_equal(rep.observable_vector(nm), o2_results["coarse"][b][nm]), nm
            for nm in ("greenKTauXFine", "pairPlusTauFine", "sdwTauQ0Fine", "currentYTauFine", "bondKineticXFine"):
                with pytest.raises(DqmcError) as e:
                    rep.observable_vector(nm)
                assert e.value.code == -1 and "timeDisplacedFineOnDevice" in str(e.value)
            assert len(rep.tau_grid(fine=True)) == m + 1
    finally:
        batch.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors():
    from detqmc_amd import DetSDW, DqmcError, SDWParams
    base = dict(opdim=2, L=4, beta=1.0, dtau=0.1, s=3, delaySteps=4, stabilisation="qr", fermionMeasurements=True,
                timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True, timeDisplacedEverySlice=True)

    def refused(rep, nm, nfreq, frag=None):
        with pytest.raises(DqmcError) as e:
            rep.matsubara(nm, nfreq)
        assert e.value.code == -1
        if frag:
            assert frag in str(e.value), str(e.value)

    rep = DetSDW(SDWParams(**base))
    try:
        refused(rep, "chargeTau", 3, "measurement sweep")            # before any measurement sweep
        rep.sweep(True)
        assert rep.matsubara("chargeTau", 3).shape == (3, 16)
        assert rep.matsubara("chargeTau", 10).shape == (10, 16)
        refused(rep, "chargeTau", 0, "nfreq")
        refused(rep, "chargeTau", 11, "nfreq")
        refused(rep, "currentXTau", 3, "timeDisplacedParticleHole = 2")     # a channel that is not enabled
        with pytest.raises(KeyError):
            rep.matsubara("bondKineticX", 3)                         # no transform of this observable
        kc = rep.kernel_context
        for ch, nfreq in ((3, 3), (4, 3), (-1, 3), (2, 0), (2, 11)):
            with pytest.raises(DqmcError) as e:
                kc.measure_td_matsubara(ch, nfreq)
            assert e.value.code == -1
            assert kc.lib.dqmc_measure_td_matsubara_size(kc.h, ch, nfreq) == 0
        rep.sweepThermalization()
        refused(rep, "chargeTau", 3, "measurement sweep")            # after a thermalisation sweep
        rep.sweep(True)
        rep.matsubara("chargeTau", 3)
        rep.sweep(False)
        refused(rep, "chargeTau", 3, "measurement sweep")
    finally:
        rep.close()
    rep = DetSDW(SDWParams(**dict(base, timeDisplacedEverySlice=False)))
    try:
        rep.sweep(True)
        refused(rep, "chargeTau", 3, "timeDisplacedEverySlice")      # no every-slice option
        with pytest.raises(DqmcError) as e:
            rep.kernel_context.measure_td_matsubara(2, 3)
        assert e.value.code == -1
    finally:
        rep.close()
    with pytest.raises(DqmcError) as e:                              # the flag without every-slice
        DetSDW(SDWParams(**dict(base, timeDisplacedEverySlice=False, timeDisplacedFineOnDevice=True)))
    assert e.value.code == -1 and "timeDisplacedFineOnDevice" in str(e.value)
    # a block with a row that was never measured: an error, not a zero
    from detqmc_amd import KernelContext
    ctx = KernelContext(2, 4, 10, 3, 0.1, delaySteps=4, stabilisation="qr", timeDisplaced=2, tdEverySlice=True)
    try:
        import td_fine_reference as tf
        ctx.set_fields(tf.random_phi(2, 16, 10, 5))
        ctx.setupUdVStorage_and_calculateGreen()
        ctx.measure_reset()
        ctx.measure_timedisplaced_ends()                             # rows 0 and m only
        with pytest.raises(DqmcError) as e:
            ctx.measure_td_matsubara(1, 2)
        assert e.value.code == -1 and "no sample" in str(e.value)
    finally:
        ctx.close()
