"""Everything the host replica returns for every observable index, written to one .npz: the record two commits are compared with.

    python scripts/dump_observables.py --out a.npz            # on each commit
    python scripts/dump_observables.py --compare a.npz b.npz   # anywhere: entries, arrays, errors, differences (exit code 1 on any)

Five small batches (L = 4, m = 12, s = 4, apbc-x, four chains in two sub-batches, one thermalisation and two measurement sweeps): every
measurement option on with opdim = 3 and with opdim = 1, the same with timeDisplacedFineOnDevice, the same with a series opened with
host_copy=False, and one with fermionMeasurements and timeDisplacedMeasurements only.  For every index 0 .. 77, with and without
DETSDW_OBS_FINE, on chains 0 and 3: detsdw_get_observable_vector, detsdw_get_matsubara (nfreq = 3), detsdw_series_stats and
detsdw_series_read_bins through the raw C bindings.  An entry is the returned array, or 'rc|detsdw_last_error()' of a refused call.
The shape of a result is not known here (that is part of what is compared): every call writes into a buffer of sentinels, and what it
wrote, up to the last changed element, is the entry.  Needs a GPU."""
import argparse
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SENTINEL = -7.25e300
BUF = 1 << 15          # doubles; the largest result, two bins of greenMatrixTau, is 2 x 13 x 16 x 32


def configurations():
    from detqmc_amd import SDWParams, bond_kinetic, pair_operator
    base = dict(L=4, m=12, s=4, dtau=0.1, delaySteps=4, bc="apbc-x", stabilisation="qr", fermionMeasurements=True, timeDisplacedMeasurements=True)
    full = dict(base, equalTimeCorrelators=True, bandCorrelators=True, timeDisplacedPairing=True, timeDisplacedParticleHole=True,
                timeDisplacedCurrent=True, timeDisplacedEverySlice=True)
    spin_z = np.diag([1.0, -1.0, -1.0, 1.0])

    def everything(batch, p):
        batch.set_custom_bond_bilinears([(spin_z, None, None), bond_kinetic(p, "x")])
        batch.set_custom_pair_operators([pair_operator("s"), pair_operator("d_bond")])
        batch.set_green_matrix(True)

    return [("full3", dict(full, opdim=3), everything, dict(host_copy=True)),
            ("full1", dict(full, opdim=1), everything, dict(host_copy=True)),
            ("minimal", dict(base, opdim=3), None, None),
            ("fineOnDevice", dict(full, opdim=3, timeDisplacedFineOnDevice=True), everything, dict(host_copy=True)),
            ("noHostCopy", dict(full, opdim=3), everything, dict(host_copy=False))], SDWParams


def dump(out_path):
    import ctypes as C
    from detqmc_amd import DetSDWBatch, _lib
    configs, SDWParams = configurations()
    entries = {}
    buf, buf2 = np.empty(BUF), np.empty(BUF)
    dp = lambda a: a.ctypes.data_as(_lib._DP)

    def record(key, rc, lib, *arrays):
        if rc != 0:
            entries[key] = np.array("%d|%s" % (rc, (lib.detsdw_last_error() or b"").decode()))
            return
        for tag, a in zip(("", ".err"), arrays):
            changed = np.nonzero(a != SENTINEL)[0]
            entries[key + tag] = a[:changed[-1] + 1].copy() if changed.size else np.zeros(0)

    for name, kw, setup, series in configs:
        p = SDWParams(**kw)
        batch = DetSDWBatch([dataclasses.replace(p, simindex=i, r=-1.0 + 0.05 * i) for i in range(4)], sub_batches=2)
        lib, h = batch.lib, batch.h
        if setup:
            setup(batch, p)
        if series:
            batch.series_begin(1, 8, nfreq=3, phi=True, **series)
        batch.sweepThermalization()
        batch.sweep(True)
        batch.sweep(True)
        for chain in (0, 3):
            assert lib.detsdw_select_chain(h, chain) == 0
            for base in range(78):
                for which in (base, base | _lib.DETSDW_OBS_FINE):
                    key = "%s/c%d/w%d" % (name, chain, which)
                    buf.fill(SENTINEL)
                    record(key + "/vector", lib.detsdw_get_observable_vector(h, which, dp(buf)), lib, buf)
                    buf.fill(SENTINEL)
                    record(key + "/matsubara", lib.detsdw_get_matsubara(h, which, 3, dp(buf)), lib, buf)
                    buf.fill(SENTINEL)
                    buf2.fill(SENTINEL)
                    record(key + "/stats", lib.detsdw_series_stats(h, which, dp(buf), dp(buf2)), lib, buf, buf2)
                    buf.fill(SENTINEL)
                    record(key + "/bins", lib.detsdw_series_read_bins(h, which, 0, 2, dp(buf)), lib, buf)
        batch.close()
        print("%s: %d entries so far" % (name, len(entries)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **entries)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    keys = sorted(set(a.files) | set(b.files))
    arrays = errors = 0
    diffs = []
    for k in keys:
        if k not in a.files or k not in b.files:
            diffs.append(k + ": in one file only")
            continue
        x, y = a[k], b[k]
        if x.dtype.kind == "U" or y.dtype.kind == "U":
            errors += 1
            same = x.dtype.kind == y.dtype.kind and str(x) == str(y)
        else:
            arrays += 1
            same = np.array_equal(x, y)
        if not same:
            diffs.append(k)
    print("entries compared: %d\narrays: %d\nerrors: %d\ndifferences: %d" % (len(keys), arrays, errors, len(diffs)))
    for k in diffs[:40]:
        print("  differs:", k)
    return 1 if diffs else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out)
