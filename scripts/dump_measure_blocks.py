"""Everything the measurement entry points produce, for a bit-for-bit comparison of two builds of the library.

    python scripts/dump_measure_blocks.py OUT.npz            # on each build, same machine
    python scripts/dump_measure_blocks.py --compare A.npz B.npz

Per case a fixed-seed DetSDWBatch of 2 chains in one context: one thermalisation sweep, then two measurement sweeps (one per sweep
direction; the blocks are cleared at the start of each, so they are read after each).  Written per sweep and chain: every accumulator
block through KernelContext.measure_*_read, the equal-time block and the four measure_td_matsubara(ch, nfreq=3); after both sweeps the
bins of a series (bin size 1, every part the case has) and the launches per kernel family over the two measurement sweeps.  --compare
wants every array np.array_equal (the same kernels get the same operands in the same order: no tolerance) and names what differs.
Needs a GPU."""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ALL = dict(fermionMeasurements=True, equalTimeCorrelators=True, timeDisplacedMeasurements=True, timeDisplacedPairing=True,
           timeDisplacedParticleHole=True, timeDisplacedCurrent=True, timeDisplacedEverySlice=True)
CASES = {"o2_qr": dict(opdim=2, beta=2.0, stabilisation="qr"),
         "o3_qr": dict(opdim=3, beta=2.0, stabilisation="qr"),
         "o2_svd_m22": dict(opdim=2, beta=2.2, stabilisation="svd"),            # ragged last segment, the j == 1 downward leg
         "o2_qr_dense": dict(opdim=2, beta=2.0, stabilisation="qr", checkerboard=False),
         "o2_qr_coarse": dict(opdim=2, beta=2.0, stabilisation="qr", timeDisplacedEverySlice=False)}
FAMILIES = ["bmult", "gemm", "decomp", "decide", "other", "gather", "flush"]


def dump(path):
    from detqmc_amd import DetSDWBatch, SDWParams
    out = {}
    for case, kw in CASES.items():
        p = SDWParams(**{**ALL, **dict(L=4, dtau=0.1, s=5, delaySteps=4, rngSeed=4711), **kw})
        b = DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.25 * i) for i in range(2)], sub_batches=1)
        kc = b.kernel_context
        b.sweepThermalization()
        b.series_begin(1, 4, nfreq=3, phi=True)
        before = kc.profile_read()
        for sweep in range(2):
            b.sweep(True)
            reads = dict(slice=kc.measure_read, eq=kc.measure_eq_read, td=kc.measure_td_read, pair=kc.measure_td_pair_read,
                         ph=kc.measure_td_ph_read, current=kc.measure_td_current_read)
            if p.timeDisplacedEverySlice:
                reads.update({f"fine{ch}": (lambda ch=ch: kc.measure_td_fine_read(ch)) for ch in range(4)})
                for ch in range(4):
                    out[f"{case}/sweep{sweep}/matsubara{ch}"] = kc.measure_td_matsubara(ch, 3)
            for chain in range(2):
                kc.select_chain(chain)
                for name, read in reads.items():
                    out[f"{case}/sweep{sweep}/chain{chain}/{name}"] = read()
        after = kc.profile_read()
        out[f"{case}/launches"] = np.array([after[f][1] - before[f][1] for f in FAMILIES])
        for chain in range(2):
            kc.select_chain(chain)
            out[f"{case}/chain{chain}/series_bins"] = kc.series_bins()
        assert out[f"{case}/chain0/series_bins"].shape[0] == 2
        b.series_end()
        b.close()
    np.savez(path, **out)
    print(f"{len(out)} arrays of {len(CASES)} cases -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k], equal_nan=True)]
    for case in CASES:
        n = sum(k.startswith(case + "/") for k in A.files)
        print(f"{case}: {n} arrays, launches {dict(zip(FAMILIES, A[case + '/launches'].tolist()))}: "
              + ("identical" if not any(k.startswith(case + "/") for k in bad) else "DIFFERENT"))
    for k in bad:
        print("differs:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else dump(sys.argv[1]))
