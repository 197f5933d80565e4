"""Wall time of a measurement sweep with and without the equal-time correlators (equalTimeCorrelators), and the device time of one
k_measure_eq_corr launch next to its streaming bound.

    python scripts/time_eq_correlators.py [--opdim 2] [--L 8] [--beta 4.0] [--chains 32] [--warmup 3] [--sweeps 5] [--repeat 20]

(a) sweep(True) with fermionMeasurements only.
(b) sweep(True) with equalTimeCorrelators: every dqmc_measure_slice also launches k_eq_onebody + k_measure_eq_corr on the shifted
    matrix it already has, and finishFermionic reads the [1 + 5 N] block of every chain.
The two batches run the same Markov chains (same seeds); their sweeps alternate, so both see the same machine.  Times are host clocks
around calls that end in a device synchronise.  The kernel time is the HIP-event time of family 'other' across `repeat`
dqmc_measure_slice calls with the switch on minus the same with the switch off (the difference is the pair k_eq_onebody +
k_measure_eq_corr; the one-body kernel touches 16 N of the n_g^2 elements).  Algorithmic bytes of one launch: nb * 2 * 16 * n_g^2 (the
matrix read in both orientations), priced at the 6.3 TB/s DESIGN.md section 4 quotes as achievable.  Needs a GPU."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12


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

    def batch(eq):
        p = SDWParams(opdim=a.opdim, L=a.L, beta=a.beta, dtau=0.1, s=10, stabilisation="qr", fermionMeasurements=True, equalTimeCorrelators=eq)
        return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.01 * i) for i in range(a.chains)])

    off, on = batch(False), batch(True)

    def sweep(b):
        t = time.perf_counter()
        b.sweep(True)
        return time.perf_counter() - t

    for _ in range(a.warmup):
        sweep(off)
        sweep(on)
    ta, tb = [], []
    for _ in range(a.sweeps):
        ta.append(sweep(off))
        tb.append(sweep(on))
    assert np.array_equal(off.chain(0).phi, on.chain(0).phi)
    assert np.isfinite(on.chain(0).observable_vector("sdwSq")).all()
    # the kernel alone: HIP events of family 'other' across measure_slice calls, switch on minus switch off (the accumulators of the
    # last sweep are overwritten: nothing reads them after this)
    kcs = on.kernel_contexts()
    ms = {}
    for flag in (False, True):
        total = 0.0
        for kc in kcs:
            kc.set_equal_time_correlators(flag)
            kc.measure_slice()                   # warm
            kc.profile_enable(True)
            before = kc.profile_read()["other"][0]
            for _ in range(a.repeat):
                kc.measure_slice()
            total += kc.profile_read()["other"][0] - before
            kc.profile_enable(False)
            kc.set_equal_time_correlators(False)
        ms[flag] = total / (a.repeat * len(kcs))
    info = off.chain(0).info
    nb = a.chains // len(kcs)
    nbytes = nb * 2 * 16 * info.n_g ** 2
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f"O({a.opdim}), L = {a.L}, beta = {a.beta} (m = {info.m}), {a.chains} chains in {off.sub_batches} context(s); "
          f"median of {a.sweeps} after {a.warmup} warm-up sweeps")
    print(f"(a) sweep(True), fermionMeasurements only:      {1e3 * ma:9.2f} ms   (min {1e3 * min(ta):.2f}, max {1e3 * max(ta):.2f})")
    print(f"(b) sweep(True) with equalTimeCorrelators:      {1e3 * mb:9.2f} ms   (min {1e3 * min(tb):.2f}, max {1e3 * max(tb):.2f})")
    print(f"(b) / (a) = {mb / ma:.3f}")
    print(f"k_eq_onebody + k_measure_eq_corr, one launch of {nb} chains (HIP events, mean of {a.repeat}): {1e3 * (ms[True] - ms[False]):.1f} us; "
          f"algorithmic bytes {nbytes / 1e6:.2f} MB = {1e6 * nbytes / HBM_BYTES_PER_S:.1f} us at {HBM_BYTES_PER_S / 1e12:.1f} TB/s")
    off.close()
    on.close()


if __name__ == "__main__":
    main()
