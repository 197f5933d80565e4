"""What the wrap-error diagnostics (set_green_check) cost per sweep at the headline shape, and what they report there.

    python scripts/probe_green_check.py [--chains 512] [--sub-batches 4] [--sweeps 10] [--rounds 3]

One process, one job: the benchmark's workload (SDW O(2), L = 16, beta = 10, dtau = 0.1, s = 10, delaySteps = 32, QR stabilisation,
`chains` chains in `sub-batches` kernel contexts) thermalises a few sweeps, then `rounds` times: `sweeps` sweepThermalization() with the
switch off, the same with it on, wall clock around each group (an even number of sweeps, so both groups hold as many down as up
sweeps).  Prints every rate, the medians, the ratio on / off, and the worst boundary the table saw."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from detqmc_amd import DetSDWBatch, SDWParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--sub-batches", type=int, default=4)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.sweeps % 2:
        ap.error("--sweeps must be even")
    p = SDWParams(opdim=2, L=16, beta=10.0, dtau=0.1, s=10, delaySteps=32, stabilisation="qr", rngSeed=1020304050)
    batch = DetSDWBatch([dataclasses.replace(p, simindex=i) for i in range(args.chains)], sub_batches=args.sub_batches)
    try:
        for _ in range(4):
            batch.sweepThermalization()
        rate = {False: [], True: []}
        for r in range(args.rounds):
            for on in (False, True):
                batch.set_green_check(on)
                batch.sweepThermalization()
                batch.sweepThermalization()
                t0 = time.perf_counter()
                for _ in range(args.sweeps):
                    batch.sweepThermalization()
                dt = time.perf_counter() - t0
                rate[on].append(args.chains * args.sweeps / dt)
                print(f"round {r} green_check {'on ' if on else 'off'}: {rate[on][-1]:.1f} sweeps/s", flush=True)
        off, on = statistics.median(rate[False]), statistics.median(rate[True])
        print(f"median off {off:.1f} sweeps/s, on {on:.1f} sweeps/s, on / off = {on / off:.4f} (time per sweep x {off / on:.4f})", flush=True)
        worst = batch.green_check_worst()
        b = max(range(len(worst)), key=lambda i: worst[i][0])
        t = batch.green_check()
        print(f"worst boundary of {args.chains} chains: chain {b}, maxAbs {worst[b][0]:.3e} at dir {worst[b][1]} boundary {worst[b][2]} "
              f"entry ({worst[b][3]}, {worst[b][4]}); median over chains of the per-chain maximum {statistics.median(w[0] for w in worst):.3e}; "
              f"largest maxRel {t['maxRel'].max():.3e}, largest logScaleSpread {t['logScaleSpread'].max():.1f}, "
              f"non-finite entries {int(t['nonfinite'].sum())}", flush=True)
    finally:
        batch.close()


if __name__ == "__main__":
    main()
