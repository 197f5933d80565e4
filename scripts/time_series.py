"""Wall time of a measurement sweep with the equal-time correlators in three modes, and the device time of the series kernels.

    python scripts/time_series.py [--opdim 2] [--L 8] [--beta 4.0] [--chains 32] [--warmup 3] [--sweeps 5] [--repeat 20]

(a) sweep(True) with equalTimeCorrelators, no series: finishFermionic reads the [1 + 5 N] block of every chain and forms the cosine
    sums on the host (what scripts/time_eq_correlators.py calls (b)).
(b) the same with a measurement series open (DetSDWBatch.series_begin): every context also runs dqmc_series_add_sweep after its sweep --
    k_series_eq_sample, one read of the per-chain flags, k_series_accum.
(c) the series with host_copy=False: no equal-time block read and no host cosine sums; the main block of every chain is still read.
The three batches run the same Markov chains (same seeds); their sweeps alternate, so all see the same machine.  Times are host clocks
around calls that end in a device synchronise; median of `sweeps` after `warmup`.  Kernel times: HIP-event time of family 'other'
across `repeat` series_add_sweep calls on one context (sample + accumulate, the flag read between them is not inside an event pair)
and across `repeat` series_stats / series_derived calls over 8 closed bins.  Needs a GPU."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opdim", type=int, default=2)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--beta", type=float, default=4.0)
    ap.add_argument("--chains", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from detqmc_amd import DetSDWBatch, SDWParams

    def batch():
        p = SDWParams(opdim=a.opdim, L=a.L, beta=a.beta, dtau=0.1, s=10, stabilisation="qr", fermionMeasurements=True, equalTimeCorrelators=True)
        return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.01 * i) for i in range(a.chains)])

    plain, ser, nocopy = batch(), batch(), batch()
    total = a.warmup + a.sweeps
    ser.series_begin(1, total + 1)
    nocopy.series_begin(1, total + 1, host_copy=False)

    def sweep(b):
        t = time.perf_counter()
        b.sweep(True)
        return time.perf_counter() - t

    times = {0: [], 1: [], 2: []}
    for it in range(total):
        for i, b in enumerate((plain, ser, nocopy)):
            t = sweep(b)
            if it >= a.warmup:
                times[i].append(t)
    assert np.array_equal(plain.chain(0).phi, ser.chain(0).phi) and np.array_equal(plain.chain(0).phi, nocopy.chain(0).phi)
    assert ser.series_info()[:2] == (total, 0)
    m1, e1 = ser.series_stats_all("sdwSq")
    m2, e2 = nocopy.series_stats_all("sdwSq")
    assert np.array_equal(m1, m2) and np.array_equal(e1, e2) and np.isfinite(e1).all()
    ser.series_end()
    # the kernels alone, on one context: the blocks of the last sweep are still there
    kc = ser.kernel_contexts()[0]
    nb = kc.nchains_total()

    def other_ms(fn, repeat):
        fn()                                     # warm
        kc.profile_enable(True)
        before = kc.profile_read()["other"][0]
        for _ in range(repeat):
            fn()
        ms = (kc.profile_read()["other"][0] - before) / repeat
        kc.profile_enable(False)
        return ms

    kc.series_begin(10 ** 6, 2, 0, 1)
    add_ms = other_ms(kc.series_add_sweep, a.repeat)
    kc.series_end()
    kc.series_begin(1, 8, 0, 1)
    for _ in range(8):
        kc.series_add_sweep()
    stats_ms = other_ms(kc.series_stats, a.repeat)
    derived_ms = other_ms(kc.series_derived, a.repeat)
    kc.series_end()
    info = plain.chain(0).info
    med = [statistics.median(times[i]) for i in range(3)]
    print(f"O({a.opdim}), L = {a.L}, beta = {a.beta} (m = {info.m}), {a.chains} chains in {plain.sub_batches} context(s); "
          f"median of {a.sweeps} after {a.warmup} warm-up sweeps")
    for i, label in enumerate(("(a) sweep(True), equalTimeCorrelators, no series:", "(b) with a series:", "(c) with a series, host_copy=False:")):
        print(f"{label:52s} {1e3 * med[i]:9.2f} ms   (min {1e3 * min(times[i]):.2f}, max {1e3 * max(times[i]):.2f})")
    print(f"(b) / (a) = {med[1] / med[0]:.3f}   (c) / (a) = {med[2] / med[0]:.3f}")
    print(f"one context of {nb} chains, HIP events, mean of {a.repeat}: k_series_eq_sample + k_series_accum {1e3 * add_ms:.1f} us; "
          f"k_series_stats over 8 bins {1e3 * stats_ms:.1f} us; k_series_derived {1e3 * derived_ms:.1f} us")
    for b in (plain, ser, nocopy):
        b.close()


if __name__ == "__main__":
    main()
