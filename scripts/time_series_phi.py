"""Device time of the order-parameter sample kernel and wall time of a measurement sweep with and without the order-parameter part.

    python scripts/time_series_phi.py [--opdim 2] [--L 16] [--beta 10.0] [--chains 128] [--nfreq 4] [--warmup 2] [--sweeps 5] [--repeat 20]

(a) sweep(True) with fermionMeasurements, no series.
(b) the same with a series that holds the order-parameter part alone (DetSDWBatch.series_begin(phi=True)): every context also runs
    k_series_phi_sample and k_series_accum after its sweep -- one launch more for the sample, no host copy.
The two batches run the same Markov chains (same seeds); their sweeps alternate, so both see the same machine.  Times are host clocks
around calls that end in a device synchronise; median of `sweeps` after `warmup`.  Kernel time: HIP-event time of family 'other' across
`repeat` series_form_sample calls on one context of a series with this part alone -- k_series_phi_sample is the only launch inside the
event pair -- next to the bytes of phi one pass reads (the scalars' second pass over the field, served from the L2, is counted apart).
Needs a GPU."""
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
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--beta", type=float, default=10.0)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--nfreq", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from detqmc_amd import DetSDWBatch, SDWParams, phi_sample

    def batch():
        p = SDWParams(opdim=a.opdim, L=a.L, beta=a.beta, dtau=0.1, s=10, stabilisation="qr", fermionMeasurements=True)
        return DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.01 * i) for i in range(a.chains)])

    plain, ser = batch(), batch()
    total = a.warmup + a.sweeps
    ser.series_begin(1, total + 1, nfreq=a.nfreq, phi=True)

    def sweep(b):
        t = time.perf_counter()
        b.sweep(True)
        return time.perf_counter() - t

    times = {0: [], 1: []}
    for it in range(total):
        for i, b in enumerate((plain, ser)):
            t = sweep(b)
            if it >= a.warmup:
                times[i].append(t)
    assert np.array_equal(plain.chain(0).phi, ser.chain(0).phi)
    assert ser.series_info()[:2] == (total, 0)
    chi, sc = phi_sample(ser.chain(0).phi, a.L, a.nfreq)
    got = ser.chain(0).series_bins("phiChi", total - 1, 1)[0]
    assert np.abs(got - chi).max() <= 1e-10 * np.abs(chi).max()
    ser.series_end()
    kc = ser.kernel_contexts()[0]
    nb = kc.nchains_total()
    kc.series_begin(1, 2, a.nfreq, 64)
    kc.series_form_sample()                      # warm
    kc.profile_enable(True)
    before = kc.profile_read()["other"][0]
    for _ in range(a.repeat):
        kc.series_form_sample()
    ms = (kc.profile_read()["other"][0] - before) / a.repeat
    kc.profile_enable(False)
    kc.series_end()
    info = plain.chain(0).info
    field = nb * info.m * a.opdim * info.N * 8
    med = [statistics.median(times[i]) for i in range(2)]
    print(f"O({a.opdim}), L = {a.L}, beta = {a.beta} (m = {info.m}), {a.chains} chains in {plain.sub_batches} context(s), nfreq = {a.nfreq}; "
          f"median of {a.sweeps} after {a.warmup} warm-up sweeps")
    for i, label in enumerate(("(a) sweep(True), no series:", "(b) with a series, phi=True:")):
        print(f"{label:36s} {1e3 * med[i]:9.2f} ms   (min {1e3 * min(times[i]):.2f}, max {1e3 * max(times[i]):.2f})")
    print(f"(b) / (a) = {med[1] / med[0]:.4f}")
    print(f"one context of {nb} chains, HIP events, mean of {a.repeat}: k_series_phi_sample {1e3 * ms:.1f} us; one pass over phi reads "
          f"{field / 1e6:.2f} MB ({field / nb / 1e6:.3f} MB per chain): {field / (1e-3 * ms) / 1e9:.1f} GB/s of first-pass reads")
    for b in (plain, ser):
        b.close()


if __name__ == "__main__":
    main()
