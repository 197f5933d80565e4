"""What the user-defined pair operators cost per measurement sweep.

    python scripts/probe_custom_pair.py [--chains 128] [--sweeps 3] [--shapes headline,o3]

The method of scripts/probe_custom_bonds.py: one process, one job.  Per shape -- the headline's lattice (O(2), L = 16, beta = 10, s = 10,
delaySteps = 16 in one context) and O(3), L = 8, beta = 10 -- and with timeDisplacedEverySlice off and on, ONE batch of `chains` chains
in one kernel context measures, in turn,

    none      no pair operator
    site1     one on-site operator ('s'): the on-site kernel
    site4     four on-site operators
    bond1     four operators of which one carries bonds: the stencil kernel, three operators in block pair (0, 0) alone
    bond4     four operators that all carry bonds

`sweeps` measurement sweeps each after one that is not timed, wall clock around sweep(True).  Prints every time, the medians and the
ratios against `none`."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from detqmc_amd import DetSDWBatch, SDWParams, pair_operator  # noqa: E402

SHAPES = {"headline": dict(opdim=2, L=16, beta=10.0, s=10), "o3": dict(opdim=3, L=8, beta=10.0, s=10)}


def operators():
    rng = np.random.default_rng(11)

    def rand():
        return rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))

    site4 = [pair_operator("s"), pair_operator("d_band"), (rand(), None, None), (rand(), None, None)]
    return {"none": [], "site1": site4[:1], "site4": site4, "bond1": site4[:3] + [(rand(), rand(), rand())],
            "bond4": [pair_operator("s_ext"), pair_operator("d_bond"), (rand(), rand(), rand()), (None, rand(), None)]}


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
                          timeDisplacedMeasurements=True, timeDisplacedEverySlice=every, timeDisplacedFineOnDevice=every, rngSeed=99, **shape)
            batch = DetSDWBatch([dataclasses.replace(p, simindex=i) for i in range(args.chains)], sub_batches=1)
            try:
                batch.sweepThermalization()
                med = {}
                for label, ops in operators().items():
                    batch.set_custom_pair_operators(ops)
                    batch.sweep(True)
                    times = []
                    for _ in range(args.sweeps):
                        t0 = time.perf_counter()
                        batch.sweep(True)
                        times.append(time.perf_counter() - t0)
                    med[label] = statistics.median(times)
                    print(f"{name} every_slice={int(every)} chains={args.chains} {label:6s}: " + " ".join(f"{t:.4f}" for t in times)
                          + f"  median {med[label]:.4f} s", flush=True)
                print(f"{name} every_slice={int(every)}: against none: " + ", ".join(f"{k} {med[k] / med['none']:.3f}" for k in med if k != "none"),
                      flush=True)
            finally:
                batch.close()


if __name__ == "__main__":
    main()
