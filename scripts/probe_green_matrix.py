"""What the averaged Green's function block costs per measurement sweep, and what one vertex call costs.

    python scripts/probe_green_matrix.py [--chains 128] [--sweeps 3] [--bins 20] [--shapes headline,o3]

The method of scripts/probe_custom_pair.py: one process, one job.  Per shape -- the headline's lattice (O(2), L = 16, beta = 10, s = 10,
delaySteps = 16 in one context) and O(3), L = 8, beta = 10 -- with timeDisplacedEverySlice on and two pair operators set, ONE batch of
`chains` chains in one kernel context measures with set_green_matrix off and on: `sweeps` measurement sweeps each after one that is not
timed, wall clock around sweep(True).  Then, with the switch on, a series of `bins` bins of one sweep is filled and
series_derived_all("gammaBubbleCustomPair0") -- one call of the two vertex kernels over all slots, operators and jackknife indices -- is
timed three times.  Prints every time, the medians and the ratio on / off."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from detqmc_amd import DetSDWBatch, SDWParams, pair_operator  # noqa: E402

SHAPES = {"headline": dict(opdim=2, L=16, beta=10.0, s=10), "o3": dict(opdim=3, L=8, beta=10.0, s=10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--shapes", default="headline,o3")
    args = ap.parse_args()
    for name in args.shapes.split(","):
        p = SDWParams(dtau=0.1, delaySteps=16, stabilisation="qr", fermionMeasurements=True, timeDisplacedMeasurements=True,
                      timeDisplacedEverySlice=True, timeDisplacedFineOnDevice=True, rngSeed=99, **SHAPES[name])
        batch = DetSDWBatch([dataclasses.replace(p, simindex=i) for i in range(args.chains)], sub_batches=1)
        try:
            batch.sweepThermalization()
            batch.set_custom_pair_operators([pair_operator("s"), pair_operator("d_bond")])
            med = {}
            for label, on in (("off", False), ("on", True)):
                batch.set_green_matrix(on)
                batch.sweep(True)
                times = []
                for _ in range(args.sweeps):
                    t0 = time.perf_counter()
                    batch.sweep(True)
                    times.append(time.perf_counter() - t0)
                med[label] = statistics.median(times)
                print(f"{name} chains={args.chains} green_matrix {label:3s}: " + " ".join(f"{t:.4f}" for t in times) + f"  median {med[label]:.4f} s",
                      flush=True)
            print(f"{name}: on / off = {med['on'] / med['off']:.3f}", flush=True)
            batch.series_begin(1, args.bins + 2, nfreq=1)
            for _ in range(args.bins):
                batch.sweep(True)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                value, err = batch.series_derived_all("gammaBubbleCustomPair0", Q=(0, 0))
                times.append(time.perf_counter() - t0)
            print(f"{name} chains={args.chains} vertex call at {batch.series_info()[0]} bins: " + " ".join(f"{t:.4f}" for t in times)
                  + f"  median {statistics.median(times):.4f} s; Gamma Pbar of slot 0: {value[0]:.4f} +- {err[0]:.1e}", flush=True)
            batch.series_end()
        finally:
            batch.close()


if __name__ == "__main__":
    main()
