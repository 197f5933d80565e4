"""Wall time of a measurement sweep with the every-slice blocks finished on the host against the same sweep with
timeDisplacedFineOnDevice plus the Matsubara transforms of all nine observables, and the device time of the transform kernel alone.

    python scripts/time_td_finish.py [--L 8] [--beta 4.0] [--chains 32] [--nfreq 8] [--warmup 3] [--sweeps 5]

(a) default path: sweep(True) copies every fine block of every chain to the host and forms the '...Fine' observables there.
(b) timeDisplacedFineOnDevice: sweep(True) skips that; matsubara_all of the nine names at nfreq frequencies follows (four kernel
    launches and four device-to-host copies per kernel context).
The two batches run the same Markov chains (same seeds); their sweeps alternate, so both see the same machine.  Times are host clocks
around calls that end in a device synchronise; the kernel time is the HIP-event time of family 'other' across the transform calls
(nothing else is launched between the two readings).  Needs a GPU."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ["greenKTauX", "greenKTauY", "pairPlusTau", "pairMinusTau", "chargeTau", "spinZTau", "sdwTau", "currentXTau", "currentYTau"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--beta", type=float, default=4.0)
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    from detqmc_amd import DetSDWBatch, SDWParams

    def batch(on_device):
        p = SDWParams(opdim=2, L=a.L, beta=a.beta, dtau=0.1, s=10, stabilisation="qr", fermionMeasurements=True,
                      timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True, timeDisplacedCurrent=True,
                      timeDisplacedEverySlice=True, timeDisplacedFineOnDevice=on_device)
        return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.01 * i) for i in range(a.chains)])

    host, dev = batch(False), batch(True)

    def sweep_host():
        t = time.perf_counter()
        host.sweep(True)
        return time.perf_counter() - t

    def sweep_dev():
        t = time.perf_counter()
        dev.sweep(True)
        t1 = time.perf_counter()
        out = [dev.matsubara_all(nm, a.nfreq) for nm in NAMES]
        return time.perf_counter() - t, time.perf_counter() - t1, out

    for _ in range(a.warmup):
        sweep_host()
        sweep_dev()
    ta, tb, tm = [], [], []
    for _ in range(a.sweeps):
        ta.append(sweep_host())
        whole, mats, out = sweep_dev()
        tb.append(whole)
        tm.append(mats)
    # same chains, same transforms: the host path's Fine vectors through numpy would give these to rounding (tests); here only a sanity check
    assert all(np.isfinite(o).all() for o in out)
    assert np.array_equal(host.chain(0).phi, dev.chain(0).phi)
    # the kernel alone: HIP events of the four launches per context
    dev.sweep(True)
    kcs = dev.kernel_contexts()
    for kc in kcs:
        kc.profile_enable(True)
    before = [kc.profile_read()["other"] for kc in kcs]
    for nm in NAMES:
        dev.matsubara_all(nm, a.nfreq)
    after = [kc.profile_read()["other"] for kc in kcs]
    kernel_ms = sum(x[0] - y[0] for x, y in zip(after, before))
    launches = sum(x[1] - y[1] for x, y in zip(after, before))
    for kc in kcs:
        kc.profile_enable(False)
    ma, mb = statistics.median(ta), statistics.median(tb)
    info = host.chain(0).info
    print(f"L = {a.L}, beta = {a.beta} (m = {info.m}), {a.chains} chains in {host.sub_batches} context(s), nfreq = {a.nfreq}; "
          f"median of {a.sweeps} after {a.warmup} warm-up sweeps")
    print(f"(a) sweep(True), fine blocks finished on the host:            {1e3 * ma:9.2f} ms   (min {1e3 * min(ta):.2f}, max {1e3 * max(ta):.2f})")
    print(f"(b) sweep(True) with timeDisplacedFineOnDevice + 9 transforms: {1e3 * mb:9.2f} ms   (min {1e3 * min(tb):.2f}, max {1e3 * max(tb):.2f}); "
          f"of which the nine matsubara_all calls {1e3 * statistics.median(tm):.2f} ms")
    print(f"(b) / (a) = {mb / ma:.3f}")
    print(f"transform kernel alone (HIP events): {kernel_ms:.3f} ms for {launches} launches")
    host.close()
    dev.close()


if __name__ == "__main__":
    main()
