"""Time of one DetSDWBatch.series_binning_all call, and of k_series_binning alone, on a series filled with synthetic bins.

    python scripts/time_series_binning.py [--L 16] [--beta 2.0] [--chains 128] [--maxbins 100] [--nfreq 4] [--levels 5] [--repeat 5]

The series is opened with every part (equal-time correlators and the Matsubara transforms of all four every-slice channels); maxbins - 2
bins per slot go in through series_import, so no sweep runs and beta only sizes the blocks.  A call is timed with the host clock; the
level count alternates between `levels` and `levels` + 1 so that no call is served from the host layer's cache.  The kernel time is the
HIP-event time of family 'other' on one kernel context.  Needs a GPU."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--maxbins", type=int, default=100)
    ap.add_argument("--nfreq", type=int, default=4)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    from detqmc_amd import DetSDWBatch, SDWParams

    p = SDWParams(opdim=2, L=a.L, beta=a.beta, dtau=0.1, s=10, stabilisation="qr", fermionMeasurements=True, equalTimeCorrelators=True,
                  timeDisplacedMeasurements=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True, timeDisplacedCurrent=True,
                  timeDisplacedEverySlice=True)
    batch = DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.01 * i) for i in range(a.chains)])
    batch.series_begin(1, a.maxbins, a.nfreq, host_copy=False, track_variance=True)
    B = a.maxbins - 2
    rng = np.random.default_rng(0)
    for kc in batch.kernel_contexts():
        st = kc.series_state()
        n = st.nb * st.sample_len
        st.bins_closed, st.samples = B, B
        data = np.concatenate([1.0 + 0.1 * rng.standard_normal(B * n), np.zeros(n), np.ones(n), np.full(n, 0.01 * (B - 1))])
        kc.series_import(st, data)
    st = batch.series_state()
    gib = st.bins_closed * st.nb * st.sample_len * 8 / 2.0 ** 30
    wall = []
    for i in range(a.repeat + 1):
        t = time.perf_counter()
        err, tau = batch.series_binning_all("sdwSq", a.levels + i % 2)
        if i:
            wall.append(time.perf_counter() - t)
    assert np.isfinite(err).all() and np.isfinite(tau).all()
    kc = batch.kernel_contexts()[0]
    kc.profile_enable(True)
    before = kc.profile_read()["other"][0]
    for _ in range(a.repeat):
        kc.series_binning(a.levels)
    kern = (kc.profile_read()["other"][0] - before) / a.repeat
    kc.profile_enable(False)
    per_ctx = gib / batch.sub_batches
    print(f"L = {a.L}, {a.chains} chains in {batch.sub_batches} context(s), {B} closed bins of S = {st.sample_len} doubles per slot "
          f"({gib:.2f} GiB of bins), {a.levels} / {a.levels + 1} levels")
    print(f"series_binning_all, all contexts, results copied to the host: median {1e3 * statistics.median(wall):.1f} ms "
          f"(min {1e3 * min(wall):.1f}, max {1e3 * max(wall):.1f}) of {a.repeat} calls")
    print(f"k_series_binning on one context ({per_ctx:.2f} GiB of bins read twice): {kern:.2f} ms, {2 * per_ctx * 2 ** 30 / (kern * 1e-3) / 1e12:.2f} TB/s")
    batch.close()


if __name__ == "__main__":
    main()
