"""What the Hubbard replica's every-slice tau grid costs per measurement sweep.

    python scripts/time_hubbard_td_fine.py [OUT.log]

The configuration of DESIGN.md 21's table: L = 8, beta = 4, dtau = 0.1, s = 10, U = 4, 32 chains, QR.  Three settings in one process,
alternating sweep by sweep: measureFlags 3 (equal-time and boundary rows), 7 (and every slice), 7 followed by matsubara_all of all eight
names at nfreq = 8.  Per setting: 2 warm-up sweeps, then the median wall time of 5 sweep(True); then one profiled sweep per handle for
the launches and event-timer milliseconds per kernel family, the split of the time flag 7 adds between the propagation (the GEMM and
B-multiply families: bmult_dev of the three work copies) and the measurement launches (the `other` family), and the event-timer time of
the k_hubbard_td_matsubara launch alone.  Needs a GPU."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = ["bmult", "gemm", "decomp", "decide", "other", "gather", "flush"]
NAMES = ["greenUpTau", "greenDnTau", "chargeTau", "spinZZTau", "spinXXTau", "pairSTau", "pairSxTau", "pairDTau"]


def main(path):
    from detqmc_amd import DetHubbard, HubbardParams
    from detqmc_amd.model import _CtxView
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def make(fine):
        return DetHubbard(HubbardParams(L=8, beta=4.0, dtau=0.1, s=10, U=4.0, stabilisation="qr", equalTimeCorrelators=True,
                                        timeDisplacedCorrelators=True, timeDisplacedEverySlice=fine), nchains=32)

    def ctx(rep):
        inf = rep.info

        class _I:
            opdim, L, m, s, N, MSF, n_g, n = 1, inf.L, inf.m, inf.s, inf.N, 2, 2 * inf.N, inf.n
        return _CtxView(rep.lib, rep.lib.dethubbard_ctx(rep.h), _I)

    reps = {"flags 3": make(False), "flags 7": make(True), "flags 7 + matsubara_all": make(True)}
    ctxs = {k: ctx(r) for k, r in reps.items()}

    def one(key):
        rep = reps[key]
        ctxs[key].synchronize()
        t0 = time.perf_counter()
        rep.sweep(True)
        if key.endswith("matsubara_all"):
            for nm in NAMES:
                rep.matsubara_all(nm, 8)
        ctxs[key].synchronize()
        return time.perf_counter() - t0

    times = {k: [] for k in reps}
    for it in range(7):
        for key in reps:
            t = one(key)
            if it >= 2:
                times[key].append(t)
    med = {}
    for key, ts in times.items():
        med[key] = statistics.median(ts)
        say(f"{key}: sweep(True) times (s) {[f'{t:.5f}' for t in ts]} median {med[key]:.5f}")
    say(f"ratio flags 7 / flags 3: {med['flags 7'] / med['flags 3']:.4f}; with matsubara_all of eight names at nfreq = 8: "
        f"{med['flags 7 + matsubara_all'] / med['flags 3']:.4f}")
    prof = {}
    for key in ("flags 3", "flags 7"):
        c = ctxs[key]
        c.profile_enable(True)
        reps[key].sweep(True)
        prof[key] = c.profile_read()
        c.profile_enable(False)
        say(f"{key}: profiled sweep, ms (launches): " + ", ".join(f"{f} {prof[key][f][0]:.3f} ({prof[key][f][1]})" for f in FAMILIES[:5]))
    add = {f: prof["flags 7"][f][0] - prof["flags 3"][f][0] for f in FAMILIES}
    prop, meas, total = add["bmult"] + add["gemm"], add["other"], sum(add.values())
    say(f"added by flag 7, event-timer ms: propagation (gemm {add['gemm']:.3f} + bmult {add['bmult']:.3f}) = {prop:.3f}, measurement launches "
        f"(other) = {meas:.3f}, all families = {total:.3f}; propagation share {prop / total:.3f}")
    say(f"added launches: " + ", ".join(f"{f} {prof['flags 7'][f][1] - prof['flags 3'][f][1]}" for f in FAMILIES[:5]))
    c = ctxs["flags 7"]
    ts = []
    for _ in range(5):
        c.profile_enable(True)
        c.hubbard_td_matsubara(8)
        pr = c.profile_read()
        c.profile_enable(False)
        assert pr["other"][1] == 1 and sum(pr[f][1] for f in FAMILIES) == 1
        ts.append(pr["other"][0])
    say(f"k_hubbard_td_matsubara alone (32 chains, 8 channels, nfreq = 8), event-timer ms: {[f'{t:.4f}' for t in ts]} median {statistics.median(ts):.4f}")
    for r in reps.values():
        r.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
