"""Shared numpy side of the every-slice time-displaced tests: the cases, the slice coverage rule, the propagation identities applied
with the oracle's B matrices, and e_ref, the error of that float64 propagation against direct inverses."""
import functools

import numpy as np

from conftest import relerr
from td_reference import Chain, make_oracle

# name: (opdim, L, m, s, oracle / context options)
CASES = {
    "a1": (1, 4, 20, 5, {}),
    "a2": (2, 4, 20, 5, {}),
    "a3": (3, 4, 20, 5, {}),
    "b": (2, 4, 22, 5, {}),                              # s does not divide m: short last segment
    "c": (2, 4, 20, 5, dict(bc="apbc-xy")),
    "d": (2, 4, 20, 5, dict(weakZflux=True)),            # complex tables
    "e": (2, 4, 20, 5, dict(checkerboard=False)),        # dense B
    "f2": (2, 6, 20, 5, {}),                             # N = 36 is no multiple of a wave
    "f3": (3, 6, 20, 5, {}),
    "g": (2, 16, 10, 5, {}),                             # n_g = 512: the LU route, one boundary
    "h": (2, 4, 20, 5, dict(stabilisation="svd")),
}
# e_ref is taken over these: every case but h, which is a2 on the CPU (the stabilisation mode belongs to the device)
CPU_CASES = ("a1", "a2", "a3", "b", "c", "d", "e", "f2", "f3", "g")


def random_phi(opdim, N, m, seed):
    phi = np.random.default_rng(seed).uniform(-1.0, 1.0, (m + 1, N, opdim))
    phi[0] = 0.0
    return phi


def case_oracle(name):
    opdim, L, m, s, opt = CASES[name]
    opt = {k: v for k, v in opt.items() if k != "stabilisation"}
    phi = random_phi(opdim, L * L, m, 1000 + sum(map(ord, name)))
    return phi, make_oracle(phi, opdim=opdim, L=L, beta=m * 0.1, dtau=0.1, s=s, delaySteps=4, **opt)


def segment_slices(j, m, s):
    """(slices reached upward from boundary j, in order; slices reached downward, in order): the rule of
    dqmc_measure_timedisplaced_segment"""
    up = list(range(j * s, min((j + 1) * s, m)))
    down = list(range(s - 1, 0, -1)) if j == 1 else []
    return up, down


def coverage(m, s):
    """every slice the sweep measures, with multiplicity: the ends entry gives 0 and m, the segments the rest"""
    n = -(-m // s)
    hit = [0, m]
    for j in range(1, n):
        up, down = segment_slices(j, m, s)
        hit += up + down
    return sorted(hit)


def step(Bk, triple, k, direction):
    """(G(t,0), G(0,t), G(t)) from slice k to k + 1 (direction +1) or k - 1 (direction -1) with the single-slice matrices Bk"""
    gt0, g0t, gtt = triple
    inv = np.linalg.inv
    if direction > 0:
        B = Bk[k + 1]
        return B @ gt0, g0t @ inv(B), B @ gtt @ inv(B)
    B = Bk[k]
    return inv(B) @ gt0, g0t @ B, inv(B) @ gtt @ B


def propagate(Bk, triple, k0, k):
    q = k0
    while q < k:
        triple = step(Bk, triple, q, +1)
        q += 1
    while q > k:
        triple = step(Bk, triple, q, -1)
        q -= 1
    return triple


def triple_err(got, ref):
    return max(relerr(a, b) for a, b in zip(got, ref))


def propagation_error(chain, m, s):
    """largest relative error, over all slices of all segments, of the numpy propagation from Chain.greens(tau_j) against
    Chain.greens(k)"""
    n = -(-m // s)
    worst = 0.0
    for j in range(1, n):
        gtt, gt0, g0t = chain.greens(j * s)
        up, down = segment_slices(j, m, s)
        for k in up + down:
            d_tt, d_t0, d_0t = chain.greens(k)
            worst = max(worst, triple_err(propagate(chain.Bk, (gt0, g0t, gtt), j * s, k), (d_t0, d_0t, d_tt)))
    return worst


@functools.lru_cache(maxsize=None)
def case_chain(name):
    """(phi, oracle, Chain) of a case, built once per process and left unchanged"""
    phi, ora = case_oracle(name)
    return phi, ora, Chain(ora)


@functools.lru_cache(maxsize=None)
def case_e_ref(name):
    _, _, m, s, _ = CASES[name]
    return propagation_error(case_chain(name)[2], m, s)


@functools.lru_cache(maxsize=None)
def e_ref():
    """the largest case_e_ref over CPU_CASES"""
    return max(case_e_ref(nm) for nm in CPU_CASES)


def td_bins(ora, gs):
    """S_X, S_Y bins of dqmc_measure_timedisplaced from a shifted engine matrix, in the block's layout [band][bin][re, im]"""
    L, N = ora.L, ora.N

    def blk(bs):
        if ora.OPDIM == 3 or bs < 2:
            return gs[N * bs:N * (bs + 1), N * bs:N * (bs + 1)]
        return np.conj(gs[N * (bs - 2):N * (bs - 1), N * (bs - 2):N * (bs - 1)])

    W = 2 * L - 1
    x, y = np.arange(N) % L, np.arange(N) // L
    bin_ = ((y[:, None] - y[None, :] + L - 1) * W + (x[:, None] - x[None, :] + L - 1)).ravel()
    out = np.zeros((2, W * W), dtype=complex)
    for band, S in ((0, blk(0) + blk(2)), (1, blk(3) + blk(1))):
        np.add.at(out[band], bin_, S.ravel())
    return np.ascontiguousarray(out).view(np.float64).ravel()
