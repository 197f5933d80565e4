"""What one particle-hole vertex call costs.

    python scripts/probe_ph_vertex.py [--chains 128] [--bins 20]

The method of scripts/probe_green_matrix.py: one process, one job, the headline's lattice (O(2), L = 16, beta = 10, s = 10, delaySteps = 16)
with timeDisplacedParticleHole and timeDisplacedEverySlice on, ONE batch of `chains` chains in one kernel context.  Two bilinears are set,
the on-site spin-z matrix and the d-density-wave bond operator, set_green_matrix is on, a series of `bins` bins of one sweep is filled, and
series_derived_all("gammaBubbleCustom0", Q = (L/2, L/2)) -- one call of the two kernels over all slots, both operators and all jackknife
indices -- is timed three times; then the same with the on-site matrix alone (the table the first call builds, one block pair of 25)."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from detqmc_amd import DetSDWBatch, SDWParams  # noqa: E402

SPINZ = (0.5 * np.diag([1.0, -1.0, -1.0, 1.0]).astype(complex), None, None)
DDW = (None, 1j * np.eye(4), -1j * np.eye(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--bins", type=int, default=20)
    args = ap.parse_args()
    L = 16
    p = SDWParams(opdim=2, L=L, beta=10.0, s=10, dtau=0.1, delaySteps=16, stabilisation="qr", fermionMeasurements=True, timeDisplacedMeasurements=True,
                  timeDisplacedParticleHole=True, timeDisplacedEverySlice=True, timeDisplacedFineOnDevice=True, rngSeed=99)
    batch = DetSDWBatch([dataclasses.replace(p, simindex=i) for i in range(args.chains)], sub_batches=1)
    try:
        batch.sweepThermalization()
        batch.set_green_matrix(True)
        for label, ops in (("spin-z + ddw bond", [SPINZ, DDW]), ("spin-z alone", [SPINZ])):
            batch.set_custom_bond_bilinears(ops)
            batch.series_begin(1, args.bins + 2, nfreq=1)
            for _ in range(args.bins):
                batch.sweep(True)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                value, err = batch.series_derived_all("gammaBubbleCustom0", Q=(L // 2, L // 2))
                times.append(time.perf_counter() - t0)
            print(f"headline chains={args.chains} {label}: ph vertex call at {batch.series_info()[0]} bins: " + " ".join(f"{t:.4f}" for t in times)
                  + f"  median {statistics.median(times):.4f} s; Gamma chibar of slot 0: {value[0]:.4f} +- {err[0]:.1e}", flush=True)
            batch.series_end()
    finally:
        batch.close()


if __name__ == "__main__":
    main()
