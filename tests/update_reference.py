"""Extended-precision reference of one updateInSlice call (the delayed-update slice of kernels_update.hip).  Plain numpy in long
double (x87 80-bit: 64-bit significand), no GPU.

It restates updateInSlice as the reference program defines it (oracle/detsdw_oracle.py:687-853 cites the lines): sites 0 .. N-1 in
order and, after every accepted proposal, an IMMEDIATE rank-MSF update of the whole of G,
    S = G[c,c],   M' = 1 + (1 - S) delta,   G <- G + G[:,c] delta M'^-1 (G[c,:] - E_c).
No delay blocks, no W: deliberately not the kernel's sub-matrix formulation.  The MSF x MSF inverse and determinant come from a
hand-written long-double Gauss-Jordan (numpy.linalg has no long double).

Proposals are formed in fp64, operation for operation as the device (and the reference program) does -- box: span = high - low,
t = span u, r = low + t, phi + r; rotate / scale: the oracle's own formulas and its NormalDistribution stack, called as they stand;
proposeNewCDWl from one uniform with the null-proposal rule prob = 1 the oracle and the kernel share.  Everything behind the
proposal is long double: Delta S with and without phi2bosons, cosh and sinh / |phi|, the cdw terms, delta, det, prob.

The uniform stream comes from a SUPPLIER, not from an array: rand01() for the proposals, accept(prob) for the acceptance test
(requested only when prob <= 1, as the reference program draws it).  RegimeSupplier forms the acceptance uniform from the
reference's own prob -- accept: prob / 2, reject: (1 + prob) / 2 -- so every decision sits far from its threshold, and records the
stream it handed out: that array is what a test pushes to the device.  The one comparison a supplier cannot steer, prob > 1, is
asserted to be far from its threshold for every proposal (|prob - 1| > 1e-6 max(1, prob)): a condition on the inputs, checked here
alone; a case that violates it gets another seed.

tests/test_update_reference_cpu.py pins this file to the committed goldens, to the fp64 oracle and to a one-shot Woodbury route."""
import math

import numpy as np

from detsdw_oracle import DetSDWOracle, NormalDistribution
from model_reference import CLD, LD, U, abs1, make_lattice  # noqa: F401  (re-exported for the tests)

assert np.finfo(np.longdouble).nmant >= 63, \
    "tests/update_reference.py needs an extended-precision long double (>= 64-bit significand); this platform's has %d bits" \
    % (np.finfo(np.longdouble).nmant + 1)
ULD = float(np.finfo(np.longdouble).eps) / 2          # unit roundoff of long double

PROPOSALS = ("box", "rotate", "scale", "rotate_and_scale")


# ------------------------------------------------------------------------------------------------------------------------------
# suppliers of the uniform stream
# ------------------------------------------------------------------------------------------------------------------------------
class RngSupplier:
    """every uniform straight from an object with rand01() (dsfmt_oracle.RngWrapper: a fixture's own stream)"""

    def __init__(self, rng):
        self.rng = rng
        self.values = []

    def begin_proposal(self, pass_index, site):
        pass

    def rand01(self):
        v = self.rng.rand01()
        self.values.append(v)
        return v

    def accept(self, prob, null=False):
        return self.rand01()

    def free_accept(self):
        pass

    @property
    def stream(self):
        return np.array(self.values, dtype=np.float64)


class RegimeSupplier:
    """proposal uniforms from a seeded numpy generator; the acceptance uniform from the reference's own prob according to the regime
    ("all": accept, "none": reject, "alternate": accept, reject, accept, ... -- a proposal with prob > 1 is accepted whatever the
    regime says and then counts as the accept of the alternation).  inject = {(pass_index, site): [values]}: handed out, in order, by
    the first rand01() calls from that proposal on (the rejected Box-Muller pairs of the direct-load row)."""

    def __init__(self, seed, regime, inject=None):
        assert regime in ("all", "none", "alternate")
        self.gen = np.random.default_rng(seed)
        self.regime = regime
        self.next_accept = True
        self.values = []
        self.inject = dict(inject or {})
        self.queue = []

    def begin_proposal(self, pass_index, site):
        self.queue += list(self.inject.pop((pass_index, site), []))

    def rand01(self):
        if self.queue:
            v = float(self.queue.pop(0))
        else:
            v = 0.0
            while not 0.0 < v < 1.0:
                v = float(self.gen.random())
        self.values.append(v)
        return v

    def accept(self, prob, null=False):
        """the uniform of an acceptance test with probability prob <= 1"""
        if null or not prob > 0.0:         # nothing to decide: a null cdwl proposal changes nothing, prob <= 0 cannot be accepted
            v = 0.5
        else:
            if self.regime == "all":
                want = True
            elif self.regime == "none":
                want = False
            else:
                want = self.next_accept
                self.next_accept = not want
            v = float(prob / 2 if want else (1 + prob) / 2)
            assert 0.0 < v < 1.0 and (v < prob) == want
        self.values.append(v)
        return v

    def free_accept(self):
        if self.regime == "alternate":
            self.next_accept = False

    @property
    def stream(self):
        return np.array(self.values, dtype=np.float64)


class ReplayRng:
    """rand01() out of a recorded stream: drives the fp64 oracle through the decisions the reference took"""

    def __init__(self, stream):
        self.stream = np.asarray(stream, dtype=np.float64)
        self.count = 0

    def rand01(self):
        v = float(self.stream[self.count])
        self.count += 1
        return v

    def randRange(self, low, high):
        return low + (high - low) * self.rand01()


# ------------------------------------------------------------------------------------------------------------------------------
# small dense algebra in long double
# ------------------------------------------------------------------------------------------------------------------------------
def gauss_jordan(A):
    """(A^-1, det A) of a small complex matrix in long double: Gauss-Jordan with partial pivoting"""
    n = A.shape[0]
    M = np.array(A, dtype=CLD)
    Inv = np.eye(n, dtype=CLD)
    det = CLD(1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
            Inv[[c, piv]] = Inv[[piv, c]]
            det = -det
        pv = M[c, c]
        det = det * pv
        M[c] = M[c] / pv
        Inv[c] = Inv[c] / pv
        for r in range(n):
            if r != c:
                f = M[r, c]
                M[r] = M[r] - f * M[c]
                Inv[r] = Inv[r] - f * Inv[c]
    return Inv, det


class _Proposer:
    """the oracle's fp64 rotate / scale proposal formulas, called as they stand on this object's phi, rng and step sizes"""
    _rotated = DetSDWOracle._rotated
    proposeRotatedPhi = DetSDWOracle.proposeRotatedPhi
    proposeScaledPhi = DetSDWOracle.proposeScaledPhi
    proposeRotatedScaledPhi = DetSDWOracle.proposeRotatedScaledPhi


class SliceResult:
    pass


def block_structure(accepted, N, D, budget):
    """accepted updates per decision launch, as the device forms its blocks (k_update_decide): a launch ends after min(D, sites
    left) accepted updates, after `budget` proposals (0: no limit) or at the last site"""
    budget = budget if budget > 0 else N
    blocks = []
    site = 0
    while site < N:
        dnow = min(D, N - site)
        j = it = 0
        while j < dnow and site < N and it < budget:
            j += int(bool(accepted[site]))
            site += 1
            it += 1
        blocks.append(j)
    return blocks


def default_budget(D, proposal_budget=0):
    """the proposals-per-block rule of dqmc_tuning::proposal_budget (include/dqmc_hip.h): 0 automatic (2 D for D >= 8, else no
    limit), -1 no limit, > 0 that many but at least D; returns 0 for "no limit" """
    b = 2 * D if D >= 8 else 0
    if proposal_budget != 0:
        b = 0 if proposal_budget < 0 else proposal_budget
    if 0 < b < D:
        b = D
    return b


class UpdateReference:
    def __init__(self, lat):
        """lat: model_reference.make_lattice(...) (the oracle's lattice and parameter tables, no Green's function)"""
        self.lat = lat
        self.p = lat.pars
        self.N, self.L, self.m, self.MSF, self.ng, self.OPDIM = lat.N, lat.L, lat.m, lat.MSF, lat.ng, lat.OPDIM
        self.dtau = lat.dtau

    # ------------------------------------------------------------------ pieces, all long double
    def cosh_sinh(self, phivec):
        ph = np.asarray(phivec, dtype=LD)
        nrm = np.sqrt(np.sum(ph * ph))
        a = LD(self.p.lambda_) * LD(self.dtau) * nrm
        return np.cosh(a), np.sinh(a) / nrm

    @staticmethod
    def cdw_eta(l):
        s6 = np.sqrt(LD(6))
        e = np.sqrt(2 * (3 - s6)) if abs(l) == 1 else np.sqrt(2 * (3 + s6)) if abs(l) == 2 else LD(0)
        return e if l > 0 else -e

    @staticmethod
    def cdw_gamma(l):
        s6 = np.sqrt(LD(6))
        return 3 + s6 if abs(l) == 1 else 3 - s6

    def cdw_cosh_sinh(self, l):
        arg = np.sqrt(LD(self.dtau)) * LD(self.p.cdwU) * self.cdw_eta(int(l))
        return np.cosh(arg), np.sinh(arg)

    def ev_matrix(self, sign, phivec, l):
        """e^{sign dtau V} at one site (detsdwopdim.cpp:3188-3229) from the field values themselves"""
        M = self.MSF
        ph = np.asarray(phivec, dtype=LD)
        c, x = self.cosh_sinh(ph)
        cC, sC = (self.cdw_cosh_sinh(l) if self.p.cdwU else (LD(1), LD(0)))
        ev = np.zeros((M, M), dtype=CLD)
        p0 = ph[0]
        p1 = ph[1] if self.OPDIM > 1 else LD(0)
        ev[0, 0] = c * cC - sign * sC
        ev[1, 1] = c * cC + sign * sC
        x = x * cC
        ev[0, 1] = sign * (p0 - 1j * p1) * x
        ev[1, 0] = sign * (p0 + 1j * p1) * x
        if self.OPDIM == 3:
            p2 = ph[2]
            ev[2, 2], ev[3, 3] = ev[0, 0], ev[1, 1]
            ev[0, 3] = ev[3, 0] = sign * p2 * x
            ev[2, 1] = ev[1, 2] = -sign * p2 * x
            ev[3, 2] = ev[0, 1]
            ev[2, 3] = ev[1, 0]
        return ev

    def delta_s_phi(self, phi, k, site, newphi, r):
        """deltaSPhi (detsdwopdim.cpp:4186-4239)"""
        p = self.p
        dtau, c, u, r = LD(self.dtau), LD(p.c), LD(p.u), LD(r)
        old = np.asarray(phi[k, site], dtype=LD)
        new = np.asarray(newphi, dtype=LD)
        diff = new - old
        oldSq, newSq = np.sum(old * old), np.sum(new * new)
        sqd = newSq - oldSq
        if p.phi2bosons:
            return dtau * LD(0.5) * r * sqd
        pow4 = newSq * newSq - oldSq * oldSq
        kE = k - 1 if k > 1 else self.m
        kL = k + 1 if k < self.m else 1
        tn = np.asarray(phi[kL, site], dtype=LD) + np.asarray(phi[kE, site], dtype=LD)
        sn = np.zeros(self.OPDIM, dtype=LD)
        for d in range(4):
            sn = sn + np.asarray(phi[k, self.lat.neigh[d, site]], dtype=LD)
        d1 = (1 / (c * c * dtau)) * (sqd - np.sum(tn * diff))
        d2 = LD(0.5) * dtau * (4 * sqd - 2 * np.sum(sn * diff))
        d3 = dtau * (LD(0.5) * r * sqd + LD(0.25) * u * pow4)
        return d1 + d2 + d3

    # ------------------------------------------------------------------ the slice
    def update_slice(self, k, phi, G, supplier, cdwl=None, proposal="box", repeat=1, phiDelta=0.5, angleDelta=0.0, scaleDelta=0.1,
                     r=None, D=None, budget=0, keep_updates=False):
        """one updateInSlice(k): `repeat` passes of phi proposals and, with cdwU != 0, the cdwl pass (its acceptance ratio is
        discarded).  phi: (m+1, N, OPDIM) float64; G: the equal-time Green's function of slice k (any complex dtype); cdwl: (m+1, N)
        integers; r: the chain's exchange parameter (default: the lattice's); D, budget: the device's delay depth and proposals per
        block (0: no limit), used for the operation count c_slice alone."""
        assert proposal in PROPOSALS and (proposal == "box" or self.OPDIM == 3)
        N, MSF, ng = self.N, self.MSF, self.ng
        r = self.p.r if r is None else r
        D = self.p.delaySteps if D is None else D
        phi = np.array(phi, dtype=np.float64)
        cdwl = np.ones((self.m + 1, N), dtype=np.int32) if cdwl is None else np.array(cdwl, dtype=np.int32)
        G = np.array(G, dtype=CLD)
        comp = abs1(G)
        eye = np.eye(MSF, dtype=CLD)
        res = SliceResult()
        res.decisions = []            # per pass: list of N flags, 1 = a change of the state was accepted
        res.dropped = 0               # scale proposals with new_r3 <= 0
        res.null_proposals = 0
        res.free_accepts = 0          # accepted with prob > 1: no uniform drawn
        res.max_draws = 0             # most uniforms one proposal drew (without its acceptance test)
        res.dets = []
        res.sites = []                # per accepted update: (pass index, site)
        res.deltas = []
        res.updates = []              # keep_updates: (idx, abs1(G[:,c] delta), abs1(M'^-1 (G[c,:] - E)))
        res.min_margin = math.inf     # min over the proposals of |prob - 1| / max(1, prob)
        prop = _Proposer()
        prop.phi = phi
        prop.rng = supplier
        prop.angleDelta, prop.scaleDelta = angleDelta, scaleDelta
        prop.normal_distribution = NormalDistribution(supplier)          # reset at the top of updateInSlice (:2433-2435)
        passes = [proposal] * repeat + (["cdwl"] if self.p.cdwU else [])
        accratio = 0.0
        c_slice = 0
        for ipass, what in enumerate(passes):
            flags = [0] * N
            for site in range(N):
                supplier.begin_proposal(ipass, site)
                drawn0 = len(supplier.values)
                new_l = old_l = int(cdwl[k, site])
                newphi = phi[k, site].copy()
                null = False
                if what == "box":
                    for d in range(self.OPDIM):
                        low, high = -phiDelta, phiDelta
                        span = high - low
                        t = span * supplier.rand01()
                        rr = low + t
                        newphi[d] = phi[k, site, d] + rr
                elif what == "cdwl":
                    new_l = DetSDWOracle.cdwl_from_uniform(supplier.rand01())
                    null = new_l == old_l
                    res.null_proposals += int(null)
                else:
                    newphi, valid = (prop.proposeRotatedPhi if what == "rotate" else prop.proposeScaledPhi if what == "scale"
                                     else prop.proposeRotatedScaledPhi)(site, k)
                    if not valid:                       # changed == NONE: rejected at once, no acceptance draw
                        res.dropped += 1
                        res.max_draws = max(res.max_draws, len(supplier.values) - drawn0)
                        continue
                res.max_draws = max(res.max_draws, len(supplier.values) - drawn0)
                idx = site + N * np.arange(MSF)
                if null:
                    prob = LD(1)
                    delta = np.zeros((MSF, MSF), dtype=CLD)
                else:
                    probS = LD(1) if what == "cdwl" else np.exp(-self.delta_s_phi(phi, k, site, newphi, r))
                    delta = self.ev_matrix(-1, newphi, new_l) @ self.ev_matrix(+1, phi[k, site], old_l) - eye
                    S = G[np.ix_(idx, idx)]
                    Mp = eye + (eye - S) @ delta
                    Minv, det = gauss_jordan(Mp)
                    probF = det.real if self.OPDIM == 3 else det.real * det.real + det.imag * det.imag
                    prob = probS * probF * (self.cdw_gamma(new_l) / self.cdw_gamma(old_l))
                    margin = float(abs(prob - 1) / max(LD(1), prob))
                    res.min_margin = min(res.min_margin, margin)
                    assert margin > 1e-6, "proposal at site %d of pass %d has prob = %.17g, too close to 1: use another seed" \
                        % (site, ipass, float(prob))
                if prob > 1:
                    accept = True
                    supplier.free_accept()
                    res.free_accepts += 1
                else:
                    accept = supplier.accept(float(prob), null=null) < prob
                if not accept or null:
                    continue
                flags[site] = 1
                phi[k, site] = newphi
                cdwl[k, site] = new_l
                R = G[idx, :].copy()
                R[np.arange(MSF), idx] -= 1
                C = G[:, idx] @ delta
                Y = Minv @ R
                G = G + C @ Y
                Ca, Ya = abs1(C), abs1(Y)
                comp = comp + Ca @ Ya
                res.dets.append(det)
                res.sites.append((ipass, site))
                res.deltas.append(delta)
                if keep_updates:
                    res.updates.append((idx, Ca, Ya))
            if what != "cdwl":
                accratio = sum(flags) / N
            res.decisions.append(flags)
            c_slice += sum(4 * (MSF * j + 2) for j in block_structure(flags, N, D, budget))
        res.phi = phi
        res.phi_k = phi[k]
        res.cdwl_k = cdwl[k]
        ch = np.zeros(N, dtype=LD)
        sh = np.zeros(N, dtype=LD)
        cC = np.ones(N, dtype=LD)
        sC = np.zeros(N, dtype=LD)
        for site in range(N):
            ch[site], sh[site] = self.cosh_sinh(phi[k, site])
            if self.p.cdwU:
                cC[site], sC[site] = self.cdw_cosh_sinh(cdwl[k, site])
        res.cosh_k, res.sinh_k, res.cdwC_k, res.cdwS_k = ch, sh, cC, sC
        res.G = G
        res.comp = comp
        res.c_slice = c_slice
        res.accepted = [sum(f) for f in res.decisions]
        res.accRatio = accratio
        res.stream = supplier.stream
        res.consumed = len(res.stream)
        return res


def oracle_twin(lat, k, phi, G, stream, cdwl=None, proposal="box", repeat=1, phiDelta=0.5, angleDelta=0.0, scaleDelta=0.1, r=None, D=None):
    """the fp64 oracle (DetSDWOracle.updateInSlice_delayed, delay depth D) driven by a recorded stream from the same input; returns
    the oracle object (phi, cdwl, g, lastAccRatioLocal_phi) and the number of uniforms it consumed"""
    import copy
    import dataclasses
    o = copy.copy(lat)
    kw = {}
    if r is not None:
        kw["r"] = r
    if D is not None:
        kw["delaySteps"] = D
    o.pars = dataclasses.replace(lat.pars, **kw)
    N, m = o.N, o.m
    o.phi = np.array(phi, dtype=np.float64)
    o.cdwl = np.ones((m + 1, N), dtype=np.int32) if cdwl is None else np.array(cdwl, dtype=np.int32)
    o.coshTermPhi = np.zeros((m + 1, N))
    o.sinhTermPhi = np.zeros((m + 1, N))
    o.coshTermCDWl = np.ones((m + 1, N))
    o.sinhTermCDWl = np.zeros((m + 1, N))
    o.updateCoshSinhTermsPhi()
    if o.pars.cdwU:
        o.updateCoshSinhTermsCDWl()
    o.g = np.array(G, dtype=np.complex128)
    o.rng = ReplayRng(stream)
    o.phiDelta, o.angleDelta, o.scaleDelta = phiDelta, angleDelta, scaleDelta
    o.normal_distribution = NormalDistribution(o.rng)
    o.lastAccRatioLocal_phi = 0.0
    for _ in range(repeat):
        o.lastAccRatioLocal_phi = o.updateInSlice_delayed(k, "phi" if proposal == "box" else proposal)
    if o.pars.cdwU:
        o.updateInSlice_delayed(k, "cdwl")
    return o, o.rng.count


def e64_spread(g64, G_ld, bs=16):
    """blockwise (bs x bs, max) error of an fp64 result against the long-double one, spread over its block: float64 (ng, ng)"""
    err = np.abs(np.asarray(g64).astype(CLD) - G_ld).astype(np.float64)
    n0, n1 = err.shape
    p0, p1 = (-n0) % bs, (-n1) % bs
    e = np.pad(err, ((0, p0), (0, p1)))
    B = e.reshape(e.shape[0] // bs, bs, e.shape[1] // bs, bs).max(axis=(1, 3))
    return np.repeat(np.repeat(B, bs, axis=0), bs, axis=1)[:n0, :n1]


def green_bound(res, g64):
    """the elementwise bound of the device's G: c_slice u comp + 8 e64 + u |G_ld| (tests/test_gpu_update_slice.py composes it)"""
    return res.c_slice * U * res.comp + 8.0 * e64_spread(g64, res.G) + U * np.abs(res.G).astype(np.float64)


def one_shot_woodbury(G_in, sites, deltas, N, MSF):
    """G' = G + G[:,I] Delta_I (1 + (1 - G[I,I]) Delta_I)^-1 (G[I,:] - E_I) over ALL accepted sites I of a pass at once (block-diagonal
    Delta_I of the per-site delta), solved with the same long-double elimination; returns (G', det(1 + (1 - G[I,I]) Delta_I))"""
    G = np.array(G_in, dtype=CLD)
    if not sites:
        return G, CLD(1)
    I = np.concatenate([s + N * np.arange(MSF) for s in sites])
    K = len(I)
    Dl = np.zeros((K, K), dtype=CLD)
    for a, d in enumerate(deltas):
        Dl[a * MSF:(a + 1) * MSF, a * MSF:(a + 1) * MSF] = d
    M = np.eye(K, dtype=CLD) + (np.eye(K, dtype=CLD) - G[np.ix_(I, I)]) @ Dl
    Minv, det = gauss_jordan(M)
    R = G[I, :].copy()
    R[np.arange(K), I] -= 1
    return G + (G[:, I] @ Dl) @ (Minv @ R), det


# ------------------------------------------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_update_slice.py (here so that tests/test_update_reference_cpu.py checks every row's regime cap
# without a GPU).  m = 4, s = 2, dtau = 0.1, the field amplitude and the band parameters of test_gpu_model_kernels.BASE.
# ------------------------------------------------------------------------------------------------------------------------------
M_SLICES, S_SLICES, DTAU = 4, 2, 0.1
BASE = dict(mux=-0.3, muy=0.7, txhor=-1.0, txver=-0.5, tyhor=0.5, tyver=1.0)
WIDTH = {"all": 1.0, "alternate": 4.0, "none": 6.0}        # box half-width phiDelta per regime (set through set_update_state)
ROT = dict(angleDelta=0.5, scaleDelta=0.1)
SPARE_BOX, SPARE_WINDOW = 4, 36      # spare uniforms behind the stream: a box proposal checks for opdim + 1 values, a rotate / scale
#                                      proposal for two windows of 16 (k_update_decide) -- the last proposal needs them to be there


def case_params(case):
    kw = dict(opdim=case["opdim"], L=case["L"], dtau=DTAU, delaySteps=case["D"], lambda_=1.0, bc="pbc", weakZflux=False,
              checkerboard=True, cdwU=0.0, phi2bosons=False, **BASE)
    kw.update(case["model"])
    return kw


def case_lattice(case):
    return make_lattice(beta=M_SLICES * DTAU, s=S_SLICES, **case_params(case))


def case_fields(case, chain):
    """random field of chain `chain`: uniform in [-1.2, 1.2], the discrete field uniform in {+-1, +-2}"""
    opdim, L = case["opdim"], case["L"]
    rng = np.random.default_rng(case["seed"] * 1000 + chain)
    phi = rng.uniform(-1.2, 1.2, (M_SLICES + 1, L * L, opdim))
    phi[0] = 0.0
    cdwl = rng.choice([-2, -1, 1, 2], (M_SLICES + 1, L * L)).astype(np.int32)
    return phi, cdwl


def case_supplier(case, chain):
    return RegimeSupplier(case["seed"] * 7919 + 13 * chain + 1, case["regimes"][chain], inject=case["inject"])


def case_step(case, chain):
    """(phiDelta, angleDelta, scaleDelta, r) of chain `chain`"""
    return (WIDTH[case["regimes"][chain]], case["angleDelta"], case["scaleDelta"], case["r0"] - 0.25 * chain)


def case_reference(case, chain, phi, cdwl, G):
    """the long-double slice of one chain from the Green's function G of slice case["k"]"""
    lat = case_lattice(case)
    pd, ad, sd, r = case_step(case, chain)
    ref = UpdateReference(lat)
    res = ref.update_slice(case["k"], phi, G, case_supplier(case, chain), cdwl=cdwl if lat.pars.cdwU else None, proposal=case["proposal"],
                           repeat=case["repeat"], phiDelta=pd, angleDelta=ad, scaleDelta=sd, r=r, D=case["D"],
                           budget=default_budget(case["D"], case["proposalBudget"]))
    return lat, res


def case_twin(case, chain, lat, phi, cdwl, G, stream):
    pd, ad, sd, r = case_step(case, chain)
    return oracle_twin(lat, case["k"], phi, G, stream, cdwl=cdwl if lat.pars.cdwU else None, proposal=case["proposal"],
                       repeat=case["repeat"], phiDelta=pd, angleDelta=ad, scaleDelta=sd, r=r, D=case["D"])


def _row(group, opdim, L, D, regimes, tag="", **kw):
    regimes = (regimes,) if isinstance(regimes, str) else tuple(regimes)
    case = dict(group=group, opdim=opdim, L=L, D=D, regimes=regimes, k=M_SLICES, proposal="box", repeat=1, model={}, decideThreads=0,
                proposalBudget=0, pipeline=0, nchains=len(regimes), inject=None, expect_dropped=False, expect_direct=False, r0=-1.0, **ROT)
    case.update(kw)
    rg = regimes[0] if len(set(regimes)) == 1 else "mixed"
    case["id"] = "-".join(x for x in (group, f"o{opdim}", f"L{L}", f"D{D}", rg, tag) if x)
    return case


# Rows whose default seed (101 + row number) misses the row's own precondition -- the regime cap, a null cdwl proposal, a dropped
# proposal, |prob - 1| > 1e-6 -- take the first seed of 101 + row number + 1000 j that meets it.  Conditions on the inputs, found and
# checked with the long-double reference alone (tests/test_update_reference_cpu.py), never with the device.
SEEDS = {
    "o1o3-o1-L4-D16-none": 1129,
    "cdw-o2-L4-D16-alternate": 1184,
    "rotscale-o3-L4-D3-alternate-rotate-x1": 4189,
    "rotscale-o3-L4-D3-alternate-rotate-x2": 8190,
    "rotscale-o3-L4-D3-alternate-scale-x1": 3193,
    "rotscale-o3-L4-D3-alternate-scale-x2": 17194,
    "rotscale-o3-L4-D3-all-rotate_and_scale-x2": 1196,
    "rotscale-o3-L4-D3-alternate-rotate_and_scale-x1": 1197,
    "rotscale-o3-L4-D3-alternate-rotate_and_scale-x2": 2198,
    "rotscale-o3-L4-D16-alternate-rotate-x1": 3201,
    "rotscale-o3-L4-D16-alternate-rotate-x2": 3202,
    "rotscale-o3-L4-D16-all-scale-x1": 2203,
    "rotscale-o3-L4-D16-alternate-scale-x1": 1205,
    "rotscale-o3-L4-D16-alternate-scale-x2": 2206,
    "rotscale-o3-L4-D16-alternate-rotate_and_scale-x1": 2209,
    "rotscale-o3-L4-D16-alternate-rotate_and_scale-x2": 1210,
    "rotscale-o3-L4-D3-alternate-scale-direct": 1211,
}


def _table():
    rows = []
    R3 = ("all", "none", "alternate")
    # regimes x depth, box proposals, O(2): D = 32 at N = 36 has a 4-site tail block, D = 5 and 7 odd nI, D = 8 under "none"
    # budget-ended empty launches, L = 8 with D = 32 two full rounds of MSF D = 64 under "all"
    for L, Ds in ((6, (1, 2, 5, 7, 8, 31, 32)), (8, (32,))):
        for D in Ds:
            rows += [_row("depth", 2, L, D, rg) for rg in R3]
    for opdim, L, Ds in ((1, 4, (1, 16)), (3, 4, (1, 3, 16)), (3, 6, (16,))):
        for D in Ds:
            rows += [_row("o1o3", opdim, L, D, rg) for rg in R3]
    for opdim in (1, 2):
        for D in (5, 32):
            rows += [_row("shape", opdim, 6, D, "alternate", tag=f"nt{nt}", decideThreads=nt) for nt in (256, 512)]
    for b in (-1, 8, 16, 17):
        rows += [_row("budget", 2, 6, 8, rg, tag=f"b{b}", proposalBudget=b) for rg in ("alternate", "none")]
    for opdim, L, D in ((2, 6, 8), (2, 8, 32), (3, 6, 16)):
        for rg in ("all", "alternate"):
            rows += [_row("pipeline", opdim, L, D, (rg,) * nb, tag=f"nb{nb}", pipeline=1) for nb in (1, 2)]
    rows.append(_row("pipeline", 2, 6, 8, "alternate", tag="bD", pipeline=1, proposalBudget=8))
    for opdim in (2, 3):
        rows += [_row("slices", opdim, 4, 4, "alternate", tag=f"k{k}", k=k) for k in (1, 3)]
    # phi2bosons: Delta S is the r term alone -- with r = -1 nearly every proposal has prob > 1 and "alternate" cannot be met; r = 8
    rows += [_row("options", opdim, 4, 5, "alternate", tag="phi2bosons", model=dict(phi2bosons=True), r0=8.0) for opdim in (2, 3)]
    rows += [_row("options", 2, 4, 5, "alternate", tag=t, model=mo) for t, mo in
             (("apbcxy", dict(bc="apbc-xy")), ("flux", dict(weakZflux=True)), ("dense", dict(checkerboard=False)))]
    for opdim in (1, 2, 3):
        rows += [_row("cdw", opdim, 4, D, "alternate", model=dict(cdwU=0.7)) for D in (3, 16)]
    for D in (3, 16):
        for prop in ("rotate", "scale", "rotate_and_scale"):
            for rg in ("all", "alternate"):
                rows += [_row("rotscale", 3, 4, D, rg, tag=f"{prop}-x{rep}", proposal=prop, repeat=rep) for rep in (1, 2)]
    # nine rejected Box-Muller pairs in front of the proposal at site 8: it consumes more than the prefetched window of 16 uniforms
    rows.append(_row("rotscale", 3, 4, 3, "alternate", tag="scale-direct", proposal="scale", inject={(0, 8): [0.99] * 18},
                     expect_direct=True))
    # a wide Gaussian: some proposals come out with new_r3 <= 0 and are dropped without an acceptance draw
    rows.append(_row("rotscale", 3, 4, 3, "alternate", tag="scale-dropped", proposal="scale", scaleDelta=1.0, expect_dropped=True))
    rows.append(_row("batch", 2, 6, 8, ("all", "none", "alternate")))
    rows.append(_row("batch", 2, 4, 16, [R3[b % 3] for b in range(33)], tag="nb33"))
    rows.append(_row("batch", 2, 4, 16, [R3[b % 3] for b in range(8)], tag="nb8"))
    for i, c in enumerate(rows):
        c["seed"] = SEEDS.get(c["id"], 101 + i)
    for c in rows:                      # the two launch shapes of a pair run the same input: their fields are compared bit for bit
        if c["id"].endswith("-nt512"):
            c["seed"] = next(o["seed"] for o in rows if o["id"] == c["id"].replace("-nt512", "-nt256"))
    assert len({c["id"] for c in rows}) == len(rows)
    return rows


CASES = _table()


def regime_cap_ok(regime, accepted, N):
    """"all": every proposal accepted; "none": at most N / 8; "alternate": within N / 8 of N / 2"""
    if regime == "all":
        return accepted == N
    if regime == "none":
        return accepted <= N / 8
    return abs(accepted - N / 2) <= N / 8
