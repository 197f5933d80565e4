"""What the bond parts of the user-defined bilinears cost per measurement sweep.

    python scripts/probe_custom_bonds.py [--chains 128] [--sweeps 3] [--shapes headline,o3]

One process, one job.  Per shape -- the headline's lattice (O(2), L = 16, beta = 10, s = 10; with delaySteps = 16 in one context, where
bench.py runs delayed(32) in four: the update path, which these ratios of measurement sweeps do not compare) and O(3), L = 8,
beta = 10 -- and with
timeDisplacedEverySlice off and on, ONE batch of `chains` chains in one kernel context measures, in turn,

    none      no custom operator
    site4     four on-site operators: the existing kernels, the yardstick
    bond1     four operators of which one carries bonds: the stencil kernels, three operators in block pair (0, 0) alone
    bond4     four operators that all carry bonds

`sweeps` measurement sweeps each after one that is not timed, wall clock around sweep(True) (which ends with the copies of the blocks to
the host, so the device is idle when it returns).  Prints every time, the medians and the ratios against `none` and `site4`."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from detqmc_amd import DetSDWBatch, SDWParams, bond_current, bond_kinetic  # noqa: E402

SHAPES = {"headline": dict(opdim=2, L=16, beta=10.0, s=10), "o3": dict(opdim=3, L=8, beta=10.0, s=10)}


def operators(p):
    rng = np.random.default_rng(7)

    def rand():
        return rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))

    herm = [0.5 * (a + a.conj().T) for a in (rand() for _ in range(4))]
    site4 = [(m, None, None) for m in herm]
    ddw = (None, 1j * np.eye(4), -1j * np.eye(4))
    return {"none": [], "site4": site4, "bond1": site4[:3] + [(herm[3], rand(), rand())],
            "bond4": [(herm[0], rand(), rand()), bond_kinetic(p, "x"), bond_current(p, "y"), ddw]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--shapes", default="headline,o3")
    args = ap.parse_args()
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        for every in (False, True):
            p = SDWParams(dtau=0.1, delaySteps=16, stabilisation="qr", fermionMeasurements=True, equalTimeCorrelators=True,
                          timeDisplacedMeasurements=True, timeDisplacedParticleHole=True, timeDisplacedEverySlice=every,
                          timeDisplacedFineOnDevice=every, rngSeed=99, **shape)
            batch = DetSDWBatch([dataclasses.replace(p, simindex=i) for i in range(args.chains)], sub_batches=1)
            try:
                batch.sweepThermalization()
                med = {}
                for label, ops in operators(p).items():
                    batch.set_custom_bond_bilinears(ops)
                    batch.sweep(True)
                    times = []
                    for _ in range(args.sweeps):
                        t0 = time.perf_counter()
                        batch.sweep(True)
                        times.append(time.perf_counter() - t0)
                    med[label] = statistics.median(times)
                    print(f"{name} every_slice={int(every)} chains={args.chains} {label:6s}: " + " ".join(f"{t:.4f}" for t in times)
                          + f"  median {med[label]:.4f} s", flush=True)
                print(f"{name} every_slice={int(every)}: against none: site4 {med['site4'] / med['none']:.3f}, bond1 {med['bond1'] / med['none']:.3f}, "
                      f"bond4 {med['bond4'] / med['none']:.3f}; custom part against site4's: bond1 "
                      f"{(med['bond1'] - med['none']) / (med['site4'] - med['none']):.2f} x, bond4 "
                      f"{(med['bond4'] - med['none']) / (med['site4'] - med['none']):.2f} x", flush=True)
            finally:
                batch.close()


if __name__ == "__main__":
    main()
