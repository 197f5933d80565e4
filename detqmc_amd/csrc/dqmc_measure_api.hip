// C-ABI implementation (include/dqmc_hip.h), second unit: the measurement entry points -- per-slice and equal-time accumulators, the
// time-displaced channels at the boundaries and on every slice, their Matsubara transforms -- and the measurement series.
#include "dqmc_ctx.h"
#include <cmath>
#include <cstddef>
#include <cstring>

// ---------------------------------------------------------------------------------------------
// fermionic measurements: shiftGreenSymmetric + per-slice accumulation on the device
// ---------------------------------------------------------------------------------------------
// T1 <- e^{-dtau K/2} G e^{+dtau K/2} (detsdwopdim.cpp:4507-4612); src: G (default) or another matrix of the same shape
static void shift_green_dev(dqmc_ctx* c, const cplx* src = nullptr) {
    const size_t n2 = (size_t)c->n_g * c->n_g;
    launch_copy(c->lc, src ? src : c->G, c->T1, n2);
    if (!c->hm.dense) {
        ProfScope ps(c, FAM_BMULT, 2);
        launch_bmult(c->lc, nullptr, c->hm, DQMC_RIGHT, 1, 0, 1, 1, c->T1, c->n_g, /*shift=*/1);   // right: +sinh half steps
        launch_bmult(c->lc, nullptr, c->hm, DQMC_LEFT, 0, 0, 1, 1, c->T1, c->n_g, /*shift=*/1);    // left:  -sinh half steps
    } else {
        GemmArgs g = gemm_square(c, c->T1, 0, c->propKh[1], 0, c->Tdense);
        g.sharedB = 1;
        run_gemm(c, g);
        g = gemm_square(c, c->propKh[0], 0, c->Tdense, 0, c->T1);
        g.sharedA = 1;
        run_gemm(c, g);
    }
}
extern "C" int dqmc_shift_green_symmetric_host(dqmc_ctx* c, dqmc_cplx* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "shiftGreenSymmetric belongs to the SDW model");
    G_FRESH(c, "dqmc_shift_green_symmetric_host");
    (void)hipSetDevice(c->p.device);
    shift_green_dev(c);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(c, out, selp(c, c->T1), (size_t)c->n_g * c->n_g * sizeof(cplx), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// zero fill of every block the context has, by the block's own stride: the blocks outside the arena are [chain][n], contiguous, and take
// one call; a block inside the arena takes one call per chain
static int acc_reset_all(dqmc_ctx* c) {
    for (int id = 0; id < ACC_COUNT; ++id) {
        const AccBlock& a = c->acc[id];
        if (!a.n) continue;
        if (a.stride == a.n * sizeof(double)) { HIPCHK(hipMemsetAsync(a.p, 0, a.n * (size_t)c->nb * sizeof(double), c->st)); continue; }
        for (int b = 0; b < c->nb; ++b) HIPCHK(hipMemsetAsync((char*)a.p + (size_t)b * a.stride, 0, a.n * sizeof(double), c->st));
    }
    return DQMC_OK;
}
// the selected chain's copy of block id, after everything enqueued so far
static int acc_read(dqmc_ctx* c, int id, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    const AccBlock& a = c->acc[id];
    if (!a.n) return fail(DQMC_EINVAL, a.missing);
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, out, (const char*)a.p + (size_t)c->sel * a.stride, a.n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
static size_t acc_size(dqmc_ctx* c, int id) { return c ? c->acc[id].n : 0; }
extern "C" int dqmc_measure_reset(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    (void)hipSetDevice(c->p.device);
    return acc_reset_all(c);
}
extern "C" int dqmc_measure_slice(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    G_FRESH(c, "dqmc_measure_slice");
    (void)hipSetDevice(c->p.device);
    if (c->hm.hubbard) {            // DetHubbard::measure (dethubbard.cpp:521-545): accumulator layout in kernels_hubbard.hip
        { ProfScope ps(c, FAM_OTHER, 1); launch_hubbard_measure(c->lc, c->hm, c->G, c->acc[ACC_SLICE].p); }
        if (c->hub_eq_on) {         // the same unshifted G: prepare pass (transposes, bond stencils, occupations), then the walk
            ProfScope ps(c, FAM_OTHER, 2);
            const AccBlock& a = c->acc[ACC_HUB_EQ];
            const size_t scs = hubbard_corr_scratch_doubles(c->N) * sizeof(double);
            launch_hubbard_corr_prep(c->lc, c->hm, c->G, c->G, c->G, c->G, c->hub_eq_sc, scs);
            launch_hubbard_eq_corr(c->lc, c->hm, c->G, c->hub_eq_sc, scs, a.p, a.stride);
        }
        return finish(c, "dqmc_measure_slice");
    }
    shift_green_dev(c);
    { ProfScope ps(c, FAM_OTHER, 1); launch_measure_accum(c->lc, c->hm, c->T1, c->acc[ACC_SLICE].p); }
    if (c->eq_on) { ProfScope ps(c, FAM_OTHER, 2); launch_measure_eq_corr(c->lc, c->hm, c->T1, c->eq_ob, c->acc[ACC_EQ].p); }   // same T1, no second shift
    if (c->eqb_on) { ProfScope ps(c, FAM_OTHER, 2); launch_measure_eq_band(c->lc, c->hm, c->T1, c->eqb_ob, c->acc[ACC_EQ_BAND].p); }
    if (c->eqc_on) {
        ProfScope ps(c, FAM_OTHER, 2);
        launch_measure_eq_custom(c->lc, c->hm, c->cst_count, c->cst_M, c->cst_mask, c->cst_M2, c->cst_mask2, c->T1, c->cst_eq_ob, c->acc[ACC_EQ_CUSTOM].p,
                                 c->cst_bond_on ? &c->cst_bond : nullptr);
    }
    if (c->eqp_on) {                                        // the same contraction as the time-displaced rows, on the slice's own T1
        ProfScope ps(c, FAM_OTHER, 1);
        const AccBlock& a = c->acc[ACC_EQ_CUSTOM_PAIR];
        launch_measure_custom_pair(c->lc, c->hm, c->cpr_count, c->cpr_Fa, c->cpr_mask, c->T1, a.p, a.stride / sizeof(double), 0, 1,
                                   c->cpr_bond_on ? &c->cpr_bond : nullptr);
    }
    return finish(c, "dqmc_measure_slice");
}
extern "C" size_t dqmc_measure_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_SLICE); }
extern "C" int dqmc_measure_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_SLICE, out); }
// equal-time charge / spin / SDW / pairing correlators (dqmc_hip.h): a switch of dqmc_measure_slice with a block of its own
extern "C" int dqmc_set_equal_time_correlators(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the equal-time correlators belong to the SDW model");
    AccBlock& eq = c->acc[ACC_EQ];
    if (on && !eq.n) {
        (void)hipSetDevice(c->p.device);
        const size_t n = measure_eq_doubles(c->N);
        if (const int rc = salloc(c, &eq.p, n * (size_t)c->nb)) return rc;
        if (const int rc = salloc(c, &c->eq_ob, measure_eq_onebody_cplx(c->N) * (size_t)c->nb)) return rc;
        HIPCHK(hipMemsetAsync(eq.p, 0, n * (size_t)c->nb * sizeof(double), c->st));
        HIPCHK(hipMemsetAsync(c->eq_ob, 0, measure_eq_onebody_cplx(c->N) * (size_t)c->nb * sizeof(cplx), c->st));
        eq.n = n; eq.stride = n * sizeof(double);
    }
    c->eq_on = on != 0;
    return DQMC_OK;
}
extern "C" size_t dqmc_measure_eq_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_EQ); }
extern "C" int dqmc_measure_eq_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_EQ, out); }
// Hubbard replica (dqmc_hip.h): equal-time correlators, a switch of dqmc_measure_slice with a block of its own outside the arena ...
extern "C" int dqmc_hubbard_set_equal_time_correlators(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_hubbard_set_equal_time_correlators belongs to the Hubbard model");
    AccBlock& eq = c->acc[ACC_HUB_EQ];
    if (on && !eq.n) {
        (void)hipSetDevice(c->p.device);
        const size_t n = hubbard_eq_doubles(c->N), nsc = hubbard_corr_scratch_doubles(c->N);
        if (const int rc = salloc(c, &eq.p, n * (size_t)c->nb)) return rc;
        if (const int rc = salloc(c, &c->hub_eq_sc, nsc * (size_t)c->nb)) return rc;
        HIPCHK(hipMemsetAsync(eq.p, 0, n * (size_t)c->nb * sizeof(double), c->st));
        HIPCHK(hipMemsetAsync(c->hub_eq_sc, 0, nsc * (size_t)c->nb * sizeof(double), c->st));
        eq.n = n; eq.stride = n * sizeof(double);
    }
    c->hub_eq_on = on != 0;
    return DQMC_OK;
}
extern "C" size_t dqmc_hubbard_eq_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_HUB_EQ); }
extern "C" int dqmc_hubbard_eq_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_HUB_EQ, out); }
// equal-time bandDiff / bandMix correlators (dqmc_hip.h): a second, independent switch of dqmc_measure_slice with a block of its own
extern "C" int dqmc_set_equal_time_band(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the equal-time band correlators belong to the SDW model");
    AccBlock& eq = c->acc[ACC_EQ_BAND];
    if (on && !eq.n) {
        (void)hipSetDevice(c->p.device);
        const size_t n = measure_eq_band_doubles(c->N), nob = measure_eq_band_onebody_cplx(c->N);
        if (const int rc = salloc(c, &eq.p, n * (size_t)c->nb)) return rc;
        if (const int rc = salloc(c, &c->eqb_ob, nob * (size_t)c->nb)) return rc;
        HIPCHK(hipMemsetAsync(eq.p, 0, n * (size_t)c->nb * sizeof(double), c->st));
        HIPCHK(hipMemsetAsync(c->eqb_ob, 0, nob * (size_t)c->nb * sizeof(cplx), c->st));
        eq.n = n; eq.stride = n * sizeof(double);
    }
    c->eqb_on = on != 0;
    return DQMC_OK;
}
extern "C" size_t dqmc_measure_eq_band_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_EQ_BAND); }
extern "C" int dqmc_measure_eq_band_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_EQ_BAND, out); }
// user-defined bilinears (dqmc_hip.h): the matrices stay on the host, the blocks and the one-body scratch live outside the arena
void custom_free(dqmc_ctx* c) {
    for (void* q : {(void*)c->acc[ACC_TD_CUSTOM].p, (void*)c->acc[ACC_FINE0 + 5].p, (void*)c->acc[ACC_EQ_CUSTOM].p, (void*)c->cst_td_ob, (void*)c->cst_eq_ob,
                    (void*)c->cst_bond.tab, (void*)c->cst_bond.mk})
        if (q) (void)hipFree(q);
    c->acc[ACC_TD_CUSTOM].p = c->acc[ACC_FINE0 + 5].p = c->acc[ACC_EQ_CUSTOM].p = nullptr;
    c->acc[ACC_TD_CUSTOM].n = c->acc[ACC_FINE0 + 5].n = c->acc[ACC_EQ_CUSTOM].n = 0;
    c->cst_td_ob = c->cst_eq_ob = nullptr;
    c->cst_bond = CustomBond{};
    c->cst_bond_on = false;
    c->cst_count = 0;
    c->eqc_on = false;
}
// Link factor of the bond site -> site (+) mu in the stored sector: the antiperiodic sign times the Peierls phase, what build_hopping_K
// (dqmc_context.hip) puts on K[site (+) mu, site] with the amplitude left out
static cplx custom_link(const dqmc_params& p, int mu, int site) {
    const int L = p.L, N = L * L, sx = site % L, sy = site / L;
    const bool apbc_x = (p.bc == DQMC_BC_APBC_X || p.bc == DQMC_BC_APBC_XY), apbc_y = (p.bc == DQMC_BC_APBC_Y || p.bc == DQMC_BC_APBC_XY);
    const double zmag = p.weakZflux ? 1.0 / N : 0.0;
    double sign = 1.0, arg = 0.0;
    if (mu == 0) {
        if (apbc_x && sx == L - 1) sign = -1.0;
        arg = 2.0 * M_PI * zmag * sy;
    } else {
        if (apbc_y && sy == L - 1) sign = -1.0;
        if (sy == L - 1) arg = -2.0 * M_PI * zmag * L * sx;
    }
    if (!p.weakZflux) return make_double2(sign, 0.0);
    return make_double2(sign * std::cos(arg), sign * std::sin(arg));
}
// the device table of the stencil kernels on the host (CustomBond in dqmc_internal.h): blocks M0, Mx, Mx^H, My, My^H of every operator,
// then the link factors; mk the non-zero masks of the blocks, bond.parts the blocks an operator has
static void custom_bond_table(const dqmc_ctx* c, int count, const dqmc_cplx* M, const dqmc_cplx* Mx, const dqmc_cplx* My, std::vector<cplx>& tab,
                              std::vector<unsigned>& mk, CustomBond& bond) {
    tab.assign(measure_custom_bond_table_cplx(count, c->N), make_double2(0.0, 0.0));
    mk.assign((size_t)count * 5, 0u);
    for (int ch = 0; ch < count; ++ch) {
        cplx* v = tab.data() + (size_t)ch * 80;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const dqmc_cplx zero{0.0, 0.0};
                const dqmc_cplx m0 = M[16 * ch + 4 * a + b];
                const dqmc_cplx x = Mx ? Mx[16 * ch + 4 * a + b] : zero, xt = Mx ? Mx[16 * ch + 4 * b + a] : zero;
                const dqmc_cplx y = My ? My[16 * ch + 4 * a + b] : zero, yt = My ? My[16 * ch + 4 * b + a] : zero;
                v[4 * a + b] = make_double2(m0.re, m0.im);
                v[16 + 4 * a + b] = make_double2(x.re, x.im);
                v[32 + 4 * a + b] = make_double2(xt.re, -xt.im);
                v[48 + 4 * a + b] = make_double2(y.re, y.im);
                v[64 + 4 * a + b] = make_double2(yt.re, -yt.im);
            }
        for (int k = 0; k < 5; ++k) {
            unsigned bits = 0;
            for (int e = 0; e < 16; ++e)
                if (v[16 * k + e].x != 0.0 || v[16 * k + e].y != 0.0) bits |= 1u << e;
            mk[(size_t)ch * 5 + k] = bits;
            if (bits) bond.parts[ch] |= 1u << k;
        }
    }
    cplx* lk = tab.data() + (size_t)count * 80;
    for (int mu = 0; mu < 2; ++mu)
        for (int site = 0; site < c->N; ++site) lk[(size_t)mu * c->N + site] = custom_link(c->p, mu, site);
}
// Both setters.  M0 [count][4][4] Hermitian, Mx / My arbitrary or nullptr (all zero); `who` names the entry in the messages.
static int custom_set(dqmc_ctx* c, int count, const dqmc_cplx* M, const dqmc_cplx* Mx, const dqmc_cplx* My, const std::string& who) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined bilinears belong to the SDW model");
    if (count < 0 || count > DQMC_CUSTOM_MAX) return fail(DQMC_EINVAL, who + ": count must be in 0 .. DQMC_CUSTOM_MAX");
    if (count && !M) return fail(DQMC_EINVAL, "null argument");
    if (c->ser.open && (c->ser.parts & (DQMC_SERIES_MATS_CUSTOM | DQMC_SERIES_EQ_CUSTOM)))
        return fail(DQMC_EINVAL, who + ": a measurement series with a part of the user-defined bilinears is open");
    bool bonds = false;
    for (int ch = 0; ch < count; ++ch) {
        const dqmc_cplx* m = M + 16 * ch;
        bool any = false;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const dqmc_cplx v = m[4 * a + b], w = m[4 * b + a];
                if (!std::isfinite(v.re) || !std::isfinite(v.im)) return fail(DQMC_EINVAL, who + ": an entry is not finite");
                if (v.re != w.re || v.im != -w.im) return fail(DQMC_EINVAL, who + ": a matrix is not Hermitian");
                any = any || v.re != 0.0 || v.im != 0.0;
            }
        for (const dqmc_cplx* bm : {Mx, My})
            for (int k = 0; bm && k < 16; ++k) {
                const dqmc_cplx v = bm[16 * ch + k];
                if (!std::isfinite(v.re) || !std::isfinite(v.im)) return fail(DQMC_EINVAL, who + ": an entry is not finite");
                if (v.re == 0.0 && v.im == 0.0) continue;
                if (c->p.weakZflux && k / 4 != k % 4)
                    return fail(DQMC_EINVAL, who + ": with weakZflux a bond part with a flavour-off-diagonal entry has no covariant definition");
                any = bonds = true;
            }
        if (!any) return fail(DQMC_EINVAL, who + ": a matrix is all zero");
    }
    (void)hipSetDevice(c->p.device);
    // the new buffers first: a failed allocation leaves the context as it was
    const size_t nb = (size_t)c->nb, row = measure_custom_row_doubles(count, c->N);
    const size_t n_eq = count ? 1 + row : 0, n_td = count && c->G00 ? (size_t)(c->n - 1) * (1 + row) : 0;
    const size_t n_fine = n_td && c->td_fine ? (size_t)(c->m + 1) * (1 + row) : 0;
    const size_t ob_eq = count ? measure_eq_custom_onebody_cplx(count, c->N) : 0, ob_td = n_td ? measure_td_custom_onebody_cplx(count, c->N) : 0;
    // the device table of the stencil kernels: blocks M0, Mx, Mx^H, My, My^H of every operator, then the link factors
    std::vector<cplx> tab;
    std::vector<unsigned> mk;
    CustomBond bond{};
    if (bonds) custom_bond_table(c, count, M, Mx, My, tab, mk, bond);
    double *eq = nullptr, *td = nullptr, *fine = nullptr;
    cplx *oe = nullptr, *ot = nullptr, *dtab = nullptr;
    unsigned* dmk = nullptr;
    hipError_t e = hipSuccess;
    if (n_eq) e = hipMalloc((void**)&eq, n_eq * nb * sizeof(double));
    if (e == hipSuccess && ob_eq) e = hipMalloc((void**)&oe, ob_eq * nb * sizeof(cplx));
    if (e == hipSuccess && n_td) e = hipMalloc((void**)&td, n_td * nb * sizeof(double));
    if (e == hipSuccess && ob_td) e = hipMalloc((void**)&ot, ob_td * nb * sizeof(cplx));
    if (e == hipSuccess && n_fine) e = hipMalloc((void**)&fine, n_fine * nb * sizeof(double));
    if (e == hipSuccess && bonds) e = hipMalloc((void**)&dtab, tab.size() * sizeof(cplx));
    if (e == hipSuccess && bonds) e = hipMalloc((void**)&dmk, mk.size() * sizeof(unsigned));
    if (e == hipSuccess && n_fine) e = hipMemsetAsync(fine, 0, n_fine * nb * sizeof(double), c->st);
    if (e == hipSuccess && n_eq) e = hipMemsetAsync(eq, 0, n_eq * nb * sizeof(double), c->st);
    if (e == hipSuccess && ob_eq) e = hipMemsetAsync(oe, 0, ob_eq * nb * sizeof(cplx), c->st);
    if (e == hipSuccess && n_td) e = hipMemsetAsync(td, 0, n_td * nb * sizeof(double), c->st);
    if (e == hipSuccess && ob_td) e = hipMemsetAsync(ot, 0, ob_td * nb * sizeof(cplx), c->st);
    if (e == hipSuccess && bonds) e = hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(cplx), hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && bonds) e = hipMemcpyAsync(dmk, mk.data(), mk.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);  // also: nothing enqueued still uses the blocks released below
    if (e != hipSuccess) {
        for (void* q : {(void*)eq, (void*)oe, (void*)td, (void*)ot, (void*)fine, (void*)dtab, (void*)dmk}) if (q) (void)hipFree(q);
        return fail(DQMC_EHIP, who + ": " + hipGetErrorString(e));
    }
    const bool eq_switch = c->eqc_on && count > 0;          // the switch outlives a replacement, not the removal
    custom_free(c);
    c->eqc_on = eq_switch;
    c->acc[ACC_EQ_CUSTOM].p = eq; c->acc[ACC_EQ_CUSTOM].n = n_eq; c->acc[ACC_EQ_CUSTOM].stride = n_eq * sizeof(double);
    c->acc[ACC_TD_CUSTOM].p = td; c->acc[ACC_TD_CUSTOM].n = n_td; c->acc[ACC_TD_CUSTOM].stride = n_td * sizeof(double);
    c->acc[ACC_FINE0 + 5].p = fine; c->acc[ACC_FINE0 + 5].n = n_fine; c->acc[ACC_FINE0 + 5].stride = n_fine * sizeof(double);
    c->cst_eq_ob = oe; c->cst_td_ob = ot;
    c->cst_count = count;
    bond.tab = dtab; bond.mk = dmk;
    c->cst_bond = bond;
    c->cst_bond_on = bonds;
    for (int k = 0; k < 16 * DQMC_CUSTOM_MAX; ++k) {
        const bool in = k < 16 * count;
        c->cst_Mx[k] = in && Mx ? make_double2(Mx[k].re, Mx[k].im) : make_double2(0.0, 0.0);
        c->cst_My[k] = in && My ? make_double2(My[k].re, My[k].im) : make_double2(0.0, 0.0);
    }
    for (int ch = 0; ch < count; ++ch) {
        cplx* m = c->cst_M + 16 * ch;
        cplx* m2 = c->cst_M2 + 16 * ch;
        for (int k = 0; k < 16; ++k) m[k] = make_double2(M[16 * ch + k].re, M[16 * ch + k].im);
        c->cst_mask[ch] = c->cst_mask2[ch] = 0;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                cplx v = make_double2(0.0, 0.0);
                for (int k = 0; k < 4; ++k) {
                    v.x += m[4 * a + k].x * m[4 * k + b].x - m[4 * a + k].y * m[4 * k + b].y;
                    v.y += m[4 * a + k].x * m[4 * k + b].y + m[4 * a + k].y * m[4 * k + b].x;
                }
                m2[4 * a + b] = v;
                if (m[4 * a + b].x != 0.0 || m[4 * a + b].y != 0.0) c->cst_mask[ch] |= 1u << (4 * a + b);
                if (v.x != 0.0 || v.y != 0.0) c->cst_mask2[ch] |= 1u << (4 * a + b);
            }
    }
    return DQMC_OK;
}
extern "C" int dqmc_set_custom_bilinears(dqmc_ctx* c, int count, const dqmc_cplx* M) {
    return custom_set(c, count, M, nullptr, nullptr, "dqmc_set_custom_bilinears");
}
extern "C" int dqmc_set_custom_bond_bilinears(dqmc_ctx* c, int count, const dqmc_cplx* M0, const dqmc_cplx* Mx, const dqmc_cplx* My) {
    return custom_set(c, count, M0, Mx, My, "dqmc_set_custom_bond_bilinears");
}
extern "C" int dqmc_get_custom_bond_bilinears(dqmc_ctx* c, int* count, dqmc_cplx* M0, dqmc_cplx* Mx, dqmc_cplx* My) {
    if (!c || !count) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined bilinears belong to the SDW model");
    *count = c->cst_count;
    for (int k = 0; k < 16 * c->cst_count; ++k) {
        if (M0) { M0[k].re = c->cst_M[k].x; M0[k].im = c->cst_M[k].y; }
        if (Mx) { Mx[k].re = c->cst_Mx[k].x; Mx[k].im = c->cst_Mx[k].y; }
        if (My) { My[k].re = c->cst_My[k].x; My[k].im = c->cst_My[k].y; }
    }
    return DQMC_OK;
}
extern "C" int dqmc_get_custom_bilinears(dqmc_ctx* c, int* count, dqmc_cplx* M) {
    if (!c || !count) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined bilinears belong to the SDW model");
    *count = c->cst_count;
    for (int k = 0; M && k < 16 * c->cst_count; ++k) { M[k].re = c->cst_M[k].x; M[k].im = c->cst_M[k].y; }
    return DQMC_OK;
}
extern "C" int dqmc_set_equal_time_custom(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined bilinears belong to the SDW model");
    if (on && !c->cst_count) return fail(DQMC_EINVAL, c->acc[ACC_EQ_CUSTOM].missing);
    c->eqc_on = on != 0;
    return DQMC_OK;
}
extern "C" size_t dqmc_measure_eq_custom_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_EQ_CUSTOM); }
extern "C" int dqmc_measure_eq_custom_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_EQ_CUSTOM, out); }
// user-defined pair operators (dqmc_hip.h): run-time state like the bilinears above and independent of them
void custom_pair_free(dqmc_ctx* c) {
    for (void* q : {(void*)c->acc[ACC_TD_CUSTOM_PAIR].p, (void*)c->acc[ACC_FINE0 + 6].p, (void*)c->acc[ACC_EQ_CUSTOM_PAIR].p, (void*)c->cpr_bond.tab,
                    (void*)c->cpr_bond.mk})
        if (q) (void)hipFree(q);
    c->acc[ACC_TD_CUSTOM_PAIR].p = c->acc[ACC_FINE0 + 6].p = c->acc[ACC_EQ_CUSTOM_PAIR].p = nullptr;
    c->acc[ACC_TD_CUSTOM_PAIR].n = c->acc[ACC_FINE0 + 6].n = c->acc[ACC_EQ_CUSTOM_PAIR].n = 0;
    c->cpr_bond = CustomPair{};
    c->cpr_bond_on = false;
    c->cpr_count = 0;
    c->eqp_on = false;
}
// the device table of the stencil kernel on the host (CustomPair in dqmc_internal.h): per operator and block 0, x, y the forms F, conj F,
// F^H, then the link signs; mk the non-zero masks, pair.parts the blocks an operator has
static void custom_pair_table(const dqmc_ctx* c, int count, const dqmc_cplx* F0, const dqmc_cplx* Fx, const dqmc_cplx* Fy, std::vector<cplx>& tab,
                              std::vector<unsigned>& mk, CustomPair& pair) {
    tab.assign(measure_custom_pair_table_cplx(count, c->N), make_double2(0.0, 0.0));
    mk.assign((size_t)count * 6, 0u);
    const dqmc_cplx zero{0.0, 0.0};
    for (int ch = 0; ch < count; ++ch)
        for (int k = 0; k < 3; ++k) {
            const dqmc_cplx* src = k == 0 ? F0 : k == 1 ? Fx : Fy;
            cplx* v = tab.data() + ((size_t)ch * 3 + k) * 48;
            unsigned bits = 0, bits_h = 0;
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) {
                    const dqmc_cplx f = src ? src[16 * ch + 4 * a + b] : zero, ft = src ? src[16 * ch + 4 * b + a] : zero;
                    v[4 * a + b] = make_double2(f.re, f.im);
                    v[16 + 4 * a + b] = make_double2(f.re, -f.im);
                    v[32 + 4 * a + b] = make_double2(ft.re, -ft.im);
                    if (f.re != 0.0 || f.im != 0.0) bits |= 1u << (4 * a + b);
                    if (ft.re != 0.0 || ft.im != 0.0) bits_h |= 1u << (4 * a + b);
                }
            mk[((size_t)ch * 3 + k) * 2] = bits; mk[((size_t)ch * 3 + k) * 2 + 1] = bits_h;
            if (bits) pair.parts[ch] |= 1u << k;
        }
    cplx* lk = tab.data() + (size_t)count * 144;
    for (int mu = 0; mu < 2; ++mu)
        for (int site = 0; site < c->N; ++site) lk[(size_t)mu * c->N + site] = custom_link(c->p, mu, site);     // no flux here: +-1
}
extern "C" int dqmc_set_custom_pair_operators(dqmc_ctx* c, int count, const dqmc_cplx* F0, const dqmc_cplx* Fx, const dqmc_cplx* Fy) {
    const std::string who = "dqmc_set_custom_pair_operators";
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined pair operators belong to the SDW model");
    if (count < 0 || count > DQMC_CUSTOM_MAX) return fail(DQMC_EINVAL, who + ": count must be in 0 .. DQMC_CUSTOM_MAX");
    if (count && !F0) return fail(DQMC_EINVAL, "null argument");
    if (c->ser.open && (c->ser.parts & (DQMC_SERIES_MATS_CUSTOM_PAIR | DQMC_SERIES_EQ_CUSTOM_PAIR)))
        return fail(DQMC_EINVAL, who + ": a measurement series with a part of the user-defined pair operators is open");
    bool bonds = false;
    for (int ch = 0; ch < count; ++ch) {
        bool any = false;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const dqmc_cplx v = F0[16 * ch + 4 * a + b], w = F0[16 * ch + 4 * b + a];
                if (!std::isfinite(v.re) || !std::isfinite(v.im)) return fail(DQMC_EINVAL, who + ": an entry is not finite");
                any = any || v.re != w.re || v.im != w.im;  // the antisymmetric part alone contributes
            }
        for (const dqmc_cplx* bm : {Fx, Fy})
            for (int k = 0; bm && k < 16; ++k) {
                const dqmc_cplx v = bm[16 * ch + k];
                if (!std::isfinite(v.re) || !std::isfinite(v.im)) return fail(DQMC_EINVAL, who + ": an entry is not finite");
                if (v.re == 0.0 && v.im == 0.0) continue;
                if (c->p.weakZflux)
                    return fail(DQMC_EINVAL, who + ": with weakZflux the two fermions of a bond pair carry flavour-dependent Peierls phases: a bond "
                                "part has no gauge-covariant definition under the flux");
                any = bonds = true;
            }
        if (!any) return fail(DQMC_EINVAL, who + ": an operator vanishes identically (F0 - F0^T = 0 and no bond part)");
    }
    (void)hipSetDevice(c->p.device);
    // the new buffers first: a failed allocation leaves the context as it was
    const size_t nb = (size_t)c->nb, row = measure_custom_row_doubles(count, c->N);
    const size_t n_eq = count ? 1 + row : 0, n_td = count && c->td_reserved ? (size_t)(c->n - 1) * (1 + row) : 0;
    const size_t n_fine = n_td && c->td_fine ? (size_t)(c->m + 1) * (1 + row) : 0;
    std::vector<cplx> tab;
    std::vector<unsigned> mk;
    CustomPair pair{};
    if (bonds) custom_pair_table(c, count, F0, Fx, Fy, tab, mk, pair);
    double *eq = nullptr, *td = nullptr, *fine = nullptr;
    cplx* dtab = nullptr;
    unsigned* dmk = nullptr;
    hipError_t e = hipSuccess;
    if (n_eq) e = hipMalloc((void**)&eq, n_eq * nb * sizeof(double));
    if (e == hipSuccess && n_td) e = hipMalloc((void**)&td, n_td * nb * sizeof(double));
    if (e == hipSuccess && n_fine) e = hipMalloc((void**)&fine, n_fine * nb * sizeof(double));
    if (e == hipSuccess && bonds) e = hipMalloc((void**)&dtab, tab.size() * sizeof(cplx));
    if (e == hipSuccess && bonds) e = hipMalloc((void**)&dmk, mk.size() * sizeof(unsigned));
    if (e == hipSuccess && n_eq) e = hipMemsetAsync(eq, 0, n_eq * nb * sizeof(double), c->st);
    if (e == hipSuccess && n_td) e = hipMemsetAsync(td, 0, n_td * nb * sizeof(double), c->st);
    if (e == hipSuccess && n_fine) e = hipMemsetAsync(fine, 0, n_fine * nb * sizeof(double), c->st);
    if (e == hipSuccess && bonds) e = hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(cplx), hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess && bonds) e = hipMemcpyAsync(dmk, mk.data(), mk.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);  // also: nothing enqueued still uses the blocks released below
    if (e != hipSuccess) {
        for (void* q : {(void*)eq, (void*)td, (void*)fine, (void*)dtab, (void*)dmk}) if (q) (void)hipFree(q);
        return fail(DQMC_EHIP, who + ": " + hipGetErrorString(e));
    }
    const bool eq_switch = c->eqp_on && count > 0;          // the switch outlives a replacement, not the removal
    custom_pair_free(c);
    c->eqp_on = eq_switch;
    c->acc[ACC_EQ_CUSTOM_PAIR].p = eq; c->acc[ACC_EQ_CUSTOM_PAIR].n = n_eq; c->acc[ACC_EQ_CUSTOM_PAIR].stride = n_eq * sizeof(double);
    c->acc[ACC_TD_CUSTOM_PAIR].p = td; c->acc[ACC_TD_CUSTOM_PAIR].n = n_td; c->acc[ACC_TD_CUSTOM_PAIR].stride = n_td * sizeof(double);
    c->acc[ACC_FINE0 + 6].p = fine; c->acc[ACC_FINE0 + 6].n = n_fine; c->acc[ACC_FINE0 + 6].stride = n_fine * sizeof(double);
    c->cpr_count = count;
    pair.tab = dtab; pair.mk = dmk;
    c->cpr_bond = pair;
    c->cpr_bond_on = bonds;
    for (int k = 0; k < 16 * DQMC_CUSTOM_MAX; ++k) {
        const bool in = k < 16 * count;
        c->cpr_F0[k] = in ? make_double2(F0[k].re, F0[k].im) : make_double2(0.0, 0.0);
        c->cpr_Fx[k] = in && Fx ? make_double2(Fx[k].re, Fx[k].im) : make_double2(0.0, 0.0);
        c->cpr_Fy[k] = in && Fy ? make_double2(Fy[k].re, Fy[k].im) : make_double2(0.0, 0.0);
    }
    for (int ch = 0; ch < DQMC_CUSTOM_MAX; ++ch) {
        c->cpr_mask[ch] = 0;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const cplx f = c->cpr_F0[16 * ch + 4 * a + b], ft = c->cpr_F0[16 * ch + 4 * b + a];
                const cplx v = make_double2(f.x - ft.x, f.y - ft.y);
                c->cpr_Fa[16 * ch + 4 * a + b] = v;
                if (v.x != 0.0 || v.y != 0.0) c->cpr_mask[ch] |= 1u << (4 * a + b);
            }
    }
    return DQMC_OK;
}
extern "C" int dqmc_get_custom_pair_operators(dqmc_ctx* c, int* count, dqmc_cplx* F0, dqmc_cplx* Fx, dqmc_cplx* Fy) {
    if (!c || !count) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined pair operators belong to the SDW model");
    *count = c->cpr_count;
    for (int k = 0; k < 16 * c->cpr_count; ++k) {
        if (F0) { F0[k].re = c->cpr_F0[k].x; F0[k].im = c->cpr_F0[k].y; }
        if (Fx) { Fx[k].re = c->cpr_Fx[k].x; Fx[k].im = c->cpr_Fx[k].y; }
        if (Fy) { Fy[k].re = c->cpr_Fy[k].x; Fy[k].im = c->cpr_Fy[k].y; }
    }
    return DQMC_OK;
}
extern "C" int dqmc_set_equal_time_custom_pair(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the user-defined pair operators belong to the SDW model");
    if (on && !c->cpr_count) return fail(DQMC_EINVAL, c->acc[ACC_EQ_CUSTOM_PAIR].missing);
    c->eqp_on = on != 0;
    return DQMC_OK;
}
extern "C" size_t dqmc_measure_eq_custom_pair_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_EQ_CUSTOM_PAIR); }
extern "C" int dqmc_measure_eq_custom_pair_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_EQ_CUSTOM_PAIR, out); }
// the averaged Green's function block (dqmc_hip.h): run-time state like the operators above
void green_matrix_free(dqmc_ctx* c) {
    for (AccBlock* a : {&c->acc[ACC_TD_GREEN_MATRIX], &c->acc[ACC_FINE0 + 7]}) {
        if (a->p) (void)hipFree(a->p);
        a->p = nullptr; a->n = 0;
    }
    c->gm_on = false;
}
extern "C" int dqmc_set_green_matrix(dqmc_ctx* c, int on) {
    const std::string who = "dqmc_set_green_matrix";
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "the averaged Green's function block belongs to the SDW model");
    if (!on) {
        if (c->ser.open && (c->ser.parts & DQMC_SERIES_GREEN_MATRIX))
            return fail(DQMC_EINVAL, who + ": a measurement series with the part of the averaged Green's function is open");
        if (!c->gm_on) return DQMC_OK;
        (void)hipSetDevice(c->p.device);
        HIPCHK(hipStreamSynchronize(c->st));               // nothing enqueued still uses the blocks
        green_matrix_free(c);
        return DQMC_OK;
    }
    if (c->p.weakZflux)
        return fail(DQMC_EINVAL, who + ": with weakZflux <G> is invariant under magnetic translations only: the block has no gauge-independent "
                    "definition under the flux");
    if (!c->td_reserved) return fail(DQMC_EINVAL, who + ": needs a context created with dqmc_params::timedisplaced >= 1");
    if (c->gm_on) return DQMC_OK;
    (void)hipSetDevice(c->p.device);
    // the new buffers first: a failed allocation leaves the context as it was
    const size_t nb = (size_t)c->nb, row = measure_green_matrix_row_doubles(c->p.opdim, c->N);
    const size_t n_td = (size_t)(c->n - 1) * (1 + row), n_fine = c->td_fine ? (size_t)(c->m + 1) * (1 + row) : 0;
    double *td = nullptr, *fine = nullptr;
    hipError_t e = hipMalloc((void**)&td, n_td * nb * sizeof(double));
    if (e == hipSuccess && n_fine) e = hipMalloc((void**)&fine, n_fine * nb * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(td, 0, n_td * nb * sizeof(double), c->st);
    if (e == hipSuccess && n_fine) e = hipMemsetAsync(fine, 0, n_fine * nb * sizeof(double), c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) {
        for (void* q : {(void*)td, (void*)fine}) if (q) (void)hipFree(q);
        return fail(DQMC_EHIP, who + ": " + hipGetErrorString(e));
    }
    AccBlock &a = c->acc[ACC_TD_GREEN_MATRIX], &f = c->acc[ACC_FINE0 + 7];
    a.p = td; a.n = n_td; a.stride = n_td * sizeof(double);
    f.p = fine; f.n = n_fine; f.stride = n_fine * sizeof(double);
    c->gm_on = true;
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// time-displaced Green's functions (dqmc_hip.h; computed inside green_from_udv while td_on)
// ---------------------------------------------------------------------------------------------
extern "C" int dqmc_set_timedisplaced(dqmc_ctx* c, int on) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (on && !c->td_reserved) return fail(DQMC_EINVAL, "time-displaced Green's functions need a context created with dqmc_params::timedisplaced != 0");
    c->td_on = on != 0;
    return DQMC_OK;
}
extern "C" int dqmc_get_green_timedisplaced_host(dqmc_ctx* c, dqmc_cplx* g_t0, dqmc_cplx* g_0t, int* slice) {
    if (!c || !g_t0 || !g_0t || !slice) return fail(DQMC_EINVAL, "null argument");
    if (!c->td_reserved || c->td_slice < 0) return fail(DQMC_EINVAL, "no time-displaced Green's function has been computed");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipGetLastError());
    const size_t bytes = (size_t)c->n_g * c->n_g * sizeof(cplx);
    HIPCHK(copy_sync(c, g_t0, selp(c, c->GT0), bytes, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, g_0t, selp(c, c->G0T), bytes, hipMemcpyDeviceToHost));
    *slice = c->td_slice;
    return DQMC_OK;
}
// ---- the channel kernels: coarse boundaries and every time slice (DQMC_TD_EVERY_SLICE) ---------------------------------------------
enum { CH_G = 1, CH_PAIR = 2, CH_PH = 4, CH_CUR = 8, CH_BAND = 16, CH_CUSTOM = 32, CH_CUSTOM_PAIR = 64, CH_GREEN_MATRIX = 128,
       CH_TWO_BODY = CH_PH | CH_CUR | CH_BAND | CH_CUSTOM };     // bit ch of a channel mask; the pair channels and the averaged Green's
                                                                 // function need the shifted gt0 alone
static bool ser_apbx(const dqmc_ctx* c) { return c->p.bc == DQMC_BC_APBC_X || c->p.bc == DQMC_BC_APBC_XY; }
static bool ser_apby(const dqmc_ctx* c) { return c->p.bc == DQMC_BC_APBC_Y || c->p.bc == DQMC_BC_APBC_XY; }
// One-body values of an equal-time matrix for the masked particle-hole / current / band kernels (t = 0: tau side, 1: 0 side): one shift of g,
// then each masked table.  g == nullptr: T1 still holds the shifted matrix of the call before.
static void td_onebody(dqmc_ctx* c, unsigned mask, const cplx* g, int t) {
    if (!(mask & CH_TWO_BODY)) return;
    if (g) shift_green_dev(c, g);
    if (mask & CH_PH) { ProfScope ps(c, FAM_OTHER, 1); launch_td_ph_onebody(c->lc, c->hm, c->T1, c->ph_ob, t); }
    if (mask & CH_CUR) { ProfScope ps(c, FAM_OTHER, 1); launch_td_current_onebody(c->lc, c->hm, c->T1, c->cur_bt, c->cur_ob, t); }
    if (mask & CH_BAND) { ProfScope ps(c, FAM_OTHER, 1); launch_td_band_onebody(c->lc, c->hm, c->T1, c->band_ob, t); }
    if (mask & CH_CUSTOM) {
        ProfScope ps(c, FAM_OTHER, 1);
        launch_td_custom_onebody(c->lc, c->hm, c->cst_count, c->cst_M, c->cst_mask, c->T1, c->cst_td_ob, t,
                                 c->cst_bond_on ? &c->cst_bond : nullptr);
    }
}
// The one place that launches the channel kernels: row `row` of `rows` of the masked channels' blocks (channel ch: acc[first + ch]) from
// (gt0, g0t, gtt, g00) = (G(tau,0), G(0,tau), G(tau), G(0)).  Every shifted matrix is prepared once and handed to all masked kernels:
// shifted gtt / g00 -> one-body values of the tau / 0 side (nullptr: already there), (shifted g0t)^H -> ph_H, shifted gt0 -> T1.  Only the
// particle-hole, current and band channels need the first three.  T1 is scratch of many other calls, so nothing is carried between calls.
static void td_row(dqmc_ctx* c, unsigned mask, int first, int row, int rows, const cplx* gt0, const cplx* g0t, const cplx* gtt, const cplx* g00) {
    if (gtt) td_onebody(c, mask, gtt, 0);
    if (g00) td_onebody(c, mask, g00, 1);
    if (mask & CH_TWO_BODY) {
        shift_green_dev(c, g0t);
        { ProfScope ps(c, FAM_OTHER, 1); launch_conj_transpose(c->lc, c->T1, c->ph_H, c->n_g); }
    }
    shift_green_dev(c, gt0);
    if (mask & CH_G) { ProfScope ps(c, FAM_OTHER, 1); launch_measure_td(c->lc, c->hm, c->T1, c->acc[first].p, row, rows); }
    if (mask & CH_PAIR) { ProfScope ps(c, FAM_OTHER, 1); launch_measure_td_pair(c->lc, c->hm, c->T1, c->acc[first + 1].p, row, rows); }
    if (mask & CH_PH) { ProfScope ps(c, FAM_OTHER, 1); launch_measure_td_ph(c->lc, c->hm, c->T1, c->ph_H, c->ph_ob, c->acc[first + 2].p, row, rows); }
    if (mask & CH_CUR) {
        ProfScope ps(c, FAM_OTHER, 1);
        launch_measure_td_current(c->lc, c->hm, c->T1, c->ph_H, c->cur_bt, c->cur_ob, c->acc[first + 3].p, row, rows);
    }
    if (mask & CH_BAND) { ProfScope ps(c, FAM_OTHER, 1); launch_measure_td_band(c->lc, c->hm, c->T1, c->ph_H, c->band_ob, c->acc[first + 4].p, row, rows); }
    if (mask & CH_CUSTOM) {
        ProfScope ps(c, FAM_OTHER, 1);
        const AccBlock& a = c->acc[first + 5];
        launch_measure_td_custom(c->lc, c->hm, c->cst_count, c->cst_M, c->cst_mask, c->T1, c->ph_H, c->cst_td_ob, a.p, a.stride / sizeof(double), row, rows,
                                 c->cst_bond_on ? &c->cst_bond : nullptr);
    }
    if (mask & CH_CUSTOM_PAIR) {
        ProfScope ps(c, FAM_OTHER, 1);
        const AccBlock& a = c->acc[first + 6];
        launch_measure_custom_pair(c->lc, c->hm, c->cpr_count, c->cpr_Fa, c->cpr_mask, c->T1, a.p, a.stride / sizeof(double), row, rows,
                                   c->cpr_bond_on ? &c->cpr_bond : nullptr);
    }
    if (mask & CH_GREEN_MATRIX) {
        ProfScope ps(c, FAM_OTHER, 1);
        const AccBlock& a = c->acc[first + 7];
        launch_measure_green_matrix(c->lc, c->hm, c->T1, a.p, a.stride / sizeof(double), row, rows, ser_apbx(c), ser_apby(c));
    }
}
// what every entry that works at boundary j asks for; need_current_G: the entry also reads G, which must still be G(tau_j)
static int td_boundary_ok(dqmc_ctx* c, int j, bool need_current_G) {
    if (j < 1 || j > c->n - 1) return fail(DQMC_EINVAL, "boundary index j must be in 1..n-1");
    if (c->td_slice != c->s * j) return fail(DQMC_EINVAL, "the last time-displaced pair does not belong to boundary j");
    if (!need_current_G) return DQMC_OK;
    if (c->currentTimeslice != c->s * j) return fail(DQMC_EINVAL, "the context has left boundary j: G is no longer G(tau_j)");
    G_FRESH(c, "time-displaced measurement");
    return DQMC_OK;
}
// Row j - 1 of n - 1 of one coarse block, channel ch: G(k, tau) bins, pairing (neither reads G), particle-hole, current, band (all three
// of the boundary the context stands on).  Each call prepares its shifted matrices itself, so the five stand on their own in any order.
static int td_coarse(dqmc_ctx* c, int ch, int j, const char* entry) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, std::string(entry) + " belongs to the SDW model (Hubbard: dqmc_hubbard_measure_timedisplaced)");
    if (!c->acc[ACC_TD + ch].n) return fail(DQMC_EINVAL, c->acc[ACC_TD + ch].missing);
    if (const int rc = td_boundary_ok(c, j, ((1u << ch) & CH_TWO_BODY) != 0)) return rc;
    (void)hipSetDevice(c->p.device);
    td_row(c, 1u << ch, ACC_TD, j - 1, c->n - 1, c->GT0, c->G0T, c->G, c->G00);
    return finish(c, entry);
}
extern "C" int dqmc_measure_timedisplaced(dqmc_ctx* c, int j) { return td_coarse(c, 0, j, "dqmc_measure_timedisplaced"); }
extern "C" int dqmc_measure_timedisplaced_pair(dqmc_ctx* c, int j) { return td_coarse(c, 1, j, "dqmc_measure_timedisplaced_pair"); }
extern "C" int dqmc_measure_timedisplaced_ph(dqmc_ctx* c, int j) { return td_coarse(c, 2, j, "dqmc_measure_timedisplaced_ph"); }
extern "C" int dqmc_measure_timedisplaced_current(dqmc_ctx* c, int j) { return td_coarse(c, 3, j, "dqmc_measure_timedisplaced_current"); }
extern "C" int dqmc_measure_timedisplaced_band(dqmc_ctx* c, int j) { return td_coarse(c, 4, j, "dqmc_measure_timedisplaced_band"); }
extern "C" int dqmc_measure_timedisplaced_custom(dqmc_ctx* c, int j) { return td_coarse(c, 5, j, "dqmc_measure_timedisplaced_custom"); }
extern "C" int dqmc_measure_timedisplaced_custom_pair(dqmc_ctx* c, int j) { return td_coarse(c, 6, j, "dqmc_measure_timedisplaced_custom_pair"); }
extern "C" int dqmc_measure_timedisplaced_green_matrix(dqmc_ctx* c, int j) { return td_coarse(c, 7, j, "dqmc_measure_timedisplaced_green_matrix"); }
// ... and the time-displaced ones: row j - 1 of the block, from the four matrices of the boundary the context stands on, unshifted
extern "C" int dqmc_hubbard_measure_timedisplaced(dqmc_ctx* c, int j) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_hubbard_measure_timedisplaced belongs to the Hubbard model");
    const AccBlock& a = c->acc[ACC_HUB_TD];
    if (!a.n) return fail(DQMC_EINVAL, a.missing);
    if (const int rc = td_boundary_ok(c, j, true)) return rc;
    (void)hipSetDevice(c->p.device);
    ProfScope ps(c, FAM_OTHER, 2);
    double* sc = (double*)c->ph_H;
    launch_hubbard_corr_prep(c->lc, c->hm, c->G0T, nullptr, c->G, c->G00, sc, c->lc.cs);
    launch_hubbard_td_corr(c->lc, c->hm, c->GT0, sc, c->lc.cs, a.p, a.stride, j - 1, c->n - 1);
    return finish(c, "dqmc_hubbard_measure_timedisplaced");
}
extern "C" size_t dqmc_hubbard_td_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_HUB_TD); }
extern "C" int dqmc_hubbard_td_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_HUB_TD, out); }
extern "C" size_t dqmc_measure_td_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD); }
extern "C" int dqmc_measure_td_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD, out); }
extern "C" size_t dqmc_measure_td_pair_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_PAIR); }
extern "C" int dqmc_measure_td_pair_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_PAIR, out); }
extern "C" size_t dqmc_measure_td_ph_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_PH); }
extern "C" int dqmc_measure_td_ph_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_PH, out); }
extern "C" size_t dqmc_measure_td_current_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_CUR); }
extern "C" int dqmc_measure_td_current_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_CUR, out); }
extern "C" size_t dqmc_measure_td_band_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_BAND); }
extern "C" int dqmc_measure_td_band_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_BAND, out); }
extern "C" size_t dqmc_measure_td_custom_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_CUSTOM); }
extern "C" int dqmc_measure_td_custom_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_CUSTOM, out); }
extern "C" size_t dqmc_measure_td_custom_pair_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_CUSTOM_PAIR); }
extern "C" int dqmc_measure_td_custom_pair_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_CUSTOM_PAIR, out); }
extern "C" size_t dqmc_measure_td_green_matrix_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_TD_GREEN_MATRIX); }
extern "C" int dqmc_measure_td_green_matrix_read_host(dqmc_ctx* c, double* out) { return acc_read(c, ACC_TD_GREEN_MATRIX, out); }
extern "C" int dqmc_get_green0_timedisplaced_host(dqmc_ctx* c, dqmc_cplx* g00, int* slice) {
    if (!c || !g00 || !slice) return fail(DQMC_EINVAL, "null argument");
    if (!c->G00) return fail(DQMC_EINVAL, "context created without dqmc_params::td_particle_hole");
    if (c->td_slice < 0) return fail(DQMC_EINVAL, "no time-displaced Green's function has been computed");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(c, g00, selp(c, c->G00), (size_t)c->n_g * c->n_g * sizeof(cplx), hipMemcpyDeviceToHost));
    *slice = c->td_slice;
    return DQMC_OK;
}

// ---- every time slice (DQMC_TD_EVERY_SLICE) ----------------------------------------------------------------------------------
static size_t td_fine_n(const dqmc_ctx* c, int channel) { return channel >= 0 && channel < TD_CHANNELS ? c->acc[ACC_FINE0 + channel].n : 0; }
static unsigned td_fine_mask(const dqmc_ctx* c) {
    unsigned mask = 0;
    for (int ch = 0; ch < TD_CHANNELS; ++ch) if (td_fine_n(c, ch)) mask |= 1u << ch;
    return mask;
}
// the work copies from slice k to k + 1 (dir > 0) or to k - 1 (dir < 0), fields as they are on the device now:
//   up:   G(t,0) <- B_{k+1} G(t,0),   G(0,t) <- G(0,t) B_{k+1}^-1,   G(t) <- B_{k+1} G(t) B_{k+1}^-1
//   down: G(t,0) <- B_k^-1 G(t,0),    G(0,t) <- G(0,t) B_k,          G(t) <- B_k^-1 G(t) B_k
static void td_fine_step(dqmc_ctx* c, int k, int dir) {
    if (dir > 0) {
        bmult_dev(c, DQMC_LEFT, 0, k + 1, k, c->fGT0);
        bmult_dev(c, DQMC_RIGHT, 1, k + 1, k, c->fG0T);
        bmult_dev(c, DQMC_RIGHT, 1, k + 1, k, c->fGTT);
        bmult_dev(c, DQMC_LEFT, 0, k + 1, k, c->fGTT);
    } else {
        bmult_dev(c, DQMC_LEFT, 1, k, k - 1, c->fGT0);
        bmult_dev(c, DQMC_RIGHT, 0, k, k - 1, c->fG0T);
        bmult_dev(c, DQMC_RIGHT, 0, k, k - 1, c->fGTT);
        bmult_dev(c, DQMC_LEFT, 1, k, k - 1, c->fGTT);
    }
    c->fine_slice = k + (dir > 0 ? 1 : -1);
}
static void td_fine_load_boundary(dqmc_ctx* c) {
    const size_t n2 = (size_t)c->n_g * c->n_g;
    ProfScope ps(c, FAM_OTHER, 3);
    launch_copy(c->lc, c->GT0, c->fGT0, n2);
    launch_copy(c->lc, c->G0T, c->fG0T, n2);
    launch_copy(c->lc, c->G, c->fGTT, n2);
    c->fine_slice = c->td_slice;
}
extern "C" int dqmc_measure_timedisplaced_segment(dqmc_ctx* c, int j) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_measure_timedisplaced_segment belongs to the SDW model (Hubbard: dqmc_hubbard_measure_timedisplaced_segment)");
    if (!c->td_fine) return fail(DQMC_EINVAL, "context created without DQMC_TD_EVERY_SLICE");
    if (const int rc = td_boundary_ok(c, j, true)) return rc;
    (void)hipSetDevice(c->p.device);
    const int s = c->s, k0 = s * j, k1 = (s * (j + 1) < c->m ? s * (j + 1) : c->m) - 1;
    const unsigned mask = td_fine_mask(c);
    const int rows = c->m + 1;
    td_onebody(c, mask, c->G00, 1);           // G(0) does not move with tau: once per segment
    td_fine_load_boundary(c);
    for (int k = k0; k <= k1; ++k) {
        td_row(c, mask, ACC_FINE0, k, rows, c->fGT0, c->fG0T, c->fGTT, nullptr);
        if (k < k1) td_fine_step(c, k, +1);
    }
    if (j == 1 && s > 1) {                    // the slices below the first boundary have no boundary of their own
        td_fine_load_boundary(c);
        for (int k = s; k >= 2; --k) {
            td_fine_step(c, k, -1);
            td_row(c, mask, ACC_FINE0, k - 1, rows, c->fGT0, c->fG0T, c->fGTT, nullptr);
        }
    }
    return finish(c, "dqmc_measure_timedisplaced_segment");
}
// For the tests only, exported but not part of include/dqmc_hip.h: the work copies at slice k of boundary j's segment, by the steps
// dqmc_measure_timedisplaced_segment takes (its preconditions; DQMC_EINVAL for a k outside the segment); nothing is measured
extern "C" int dqmc_td_fine_propagate(dqmc_ctx* c, int j, int k) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->td_fine) return fail(DQMC_EINVAL, "context created without DQMC_TD_EVERY_SLICE (Hubbard: DQMC_TD_HUB_EVERY_SLICE)");
    if (const int rc = td_boundary_ok(c, j, true)) return rc;
    const int s = c->s, k0 = s * j, k1 = (s * (j + 1) < c->m ? s * (j + 1) : c->m) - 1;
    if (k > k1 || k < (j == 1 ? 1 : k0)) return fail(DQMC_EINVAL, "slice k does not belong to the segment of boundary j");
    (void)hipSetDevice(c->p.device);
    td_fine_load_boundary(c);
    for (int q = k0; q < k; ++q) td_fine_step(c, q, +1);
    for (int q = k0; q > k; --q) td_fine_step(c, q, -1);
    return finish(c, "dqmc_td_fine_propagate");
}
extern "C" int dqmc_measure_timedisplaced_ends(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_measure_timedisplaced_ends belongs to the SDW model (Hubbard: dqmc_hubbard_measure_timedisplaced_ends)");
    if (!c->td_fine) return fail(DQMC_EINVAL, "context created without DQMC_TD_EVERY_SLICE");
    if (c->currentTimeslice != 0 && c->currentTimeslice != c->m)
        return fail(DQMC_EINVAL, "the context does not stand at tau = 0 (beta): G is not G(0)");
    G_FRESH(c, "dqmc_measure_timedisplaced_ends");
    (void)hipSetDevice(c->p.device);
    // row m from the work copies (they are what dqmc_get_green_td_fine_host reports afterwards), row 0 from T2 / T3: scratch of the
    // Green's function routines, idle here (the shifts use T1 and, with the dense B, Tdense only)
    { ProfScope ps(c, FAM_OTHER, 1); launch_td_ends(c->lc, c->G, c->T2, c->T3, c->fGT0, c->fG0T, c->fGTT, c->n_g); }
    c->fine_slice = c->m;
    const unsigned mask = td_fine_mask(c);
    td_onebody(c, mask, c->G, 0);             // G(tau) = G(0) = G for both rows and both sides: ONE shift of G
    td_onebody(c, mask, nullptr, 1);
    td_row(c, mask, ACC_FINE0, 0, c->m + 1, c->T2, c->T3, nullptr, nullptr);
    td_row(c, mask, ACC_FINE0, c->m, c->m + 1, c->fGT0, c->fG0T, nullptr, nullptr);
    return finish(c, "dqmc_measure_timedisplaced_ends");
}
// a Hubbard context has one every-slice block: it answers as channel 0
extern "C" size_t dqmc_measure_td_fine_accum_size(dqmc_ctx* c, int channel) {
    if (c && c->hm.hubbard) return channel == 0 ? acc_size(c, ACC_HUB_TD_FINE) : 0;
    return c ? td_fine_n(c, channel) : 0;
}
extern "C" int dqmc_measure_td_fine_read_host(dqmc_ctx* c, int channel, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) {
        if (channel != 0) return fail(DQMC_EINVAL, "a Hubbard context has one every-slice block, channel 0 (dqmc_hubbard_td_fine_read_host)");
        return acc_read(c, ACC_HUB_TD_FINE, out);
    }
    if (!td_fine_n(c, channel)) return fail(DQMC_EINVAL, c->acc[ACC_FINE0].missing);
    return acc_read(c, ACC_FINE0 + channel, out);
}
// ---- every time slice, Hubbard model (DQMC_TD_HUB_EVERY_SLICE): the work copies and steps above, the model's own contraction ----
// row k of m + 1 from the displaced matrices (gt0, g0t), G(tau) = gtt and G(0) = g00: prepare pass with the stencil source, then the walk
static void hubbard_fine_row(dqmc_ctx* c, int k, const cplx* gt0, const cplx* g0t, const cplx* gtt, const cplx* g00) {
    ProfScope ps(c, FAM_OTHER, 2);
    const AccBlock& a = c->acc[ACC_HUB_TD_FINE];
    double* sc = (double*)c->ph_H;
    launch_hubbard_corr_prep(c->lc, c->hm, g0t, gt0, gtt, g00, sc, c->lc.cs);
    launch_hubbard_td_fine_corr(c->lc, c->hm, gt0, sc, c->lc.cs, a.p, a.stride, k, c->m + 1);
}
static int hubbard_fine_ok(dqmc_ctx* c, const char* entry) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->hm.hubbard) return fail(DQMC_EINVAL, std::string(entry) + " belongs to the Hubbard model");
    if (!c->acc[ACC_HUB_TD_FINE].n) return fail(DQMC_EINVAL, c->acc[ACC_HUB_TD_FINE].missing);
    return DQMC_OK;
}
extern "C" int dqmc_hubbard_measure_timedisplaced_segment(dqmc_ctx* c, int j) {
    if (const int rc = hubbard_fine_ok(c, "dqmc_hubbard_measure_timedisplaced_segment")) return rc;
    if (const int rc = td_boundary_ok(c, j, true)) return rc;
    (void)hipSetDevice(c->p.device);
    const int s = c->s, k0 = s * j, k1 = (s * (j + 1) < c->m ? s * (j + 1) : c->m) - 1;
    td_fine_load_boundary(c);
    for (int k = k0; k <= k1; ++k) {
        hubbard_fine_row(c, k, c->fGT0, c->fG0T, c->fGTT, c->G00);
        if (k < k1) td_fine_step(c, k, +1);
    }
    if (j == 1 && s > 1) {                    // the slices below the first boundary have no boundary of their own
        td_fine_load_boundary(c);
        for (int k = s; k >= 2; --k) {
            td_fine_step(c, k, -1);
            hubbard_fine_row(c, k - 1, c->fGT0, c->fG0T, c->fGTT, c->G00);
        }
    }
    return finish(c, "dqmc_hubbard_measure_timedisplaced_segment");
}
extern "C" int dqmc_hubbard_measure_timedisplaced_ends(dqmc_ctx* c) {
    if (const int rc = hubbard_fine_ok(c, "dqmc_hubbard_measure_timedisplaced_ends")) return rc;
    if (c->currentTimeslice != 0 && c->currentTimeslice != c->m)
        return fail(DQMC_EINVAL, "the context does not stand at tau = 0 (beta): G is not G(0)");
    G_FRESH(c, "dqmc_hubbard_measure_timedisplaced_ends");
    (void)hipSetDevice(c->p.device);
    // staged as dqmc_measure_timedisplaced_ends does: row m in the work copies, row 0 in T2 / T3 (idle here)
    { ProfScope ps(c, FAM_OTHER, 1); launch_td_ends(c->lc, c->G, c->T2, c->T3, c->fGT0, c->fG0T, c->fGTT, c->n_g); }
    c->fine_slice = c->m;
    hubbard_fine_row(c, 0, c->T2, c->T3, c->G, c->G);       // G(tau) = G(0) = G for both rows and both sides
    hubbard_fine_row(c, c->m, c->fGT0, c->fG0T, c->G, c->G);
    return finish(c, "dqmc_hubbard_measure_timedisplaced_ends");
}
extern "C" size_t dqmc_hubbard_td_fine_accum_size(dqmc_ctx* c) { return acc_size(c, ACC_HUB_TD_FINE); }
extern "C" int dqmc_hubbard_td_fine_read_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (!c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_hubbard_td_fine_read_host belongs to the Hubbard model");
    return acc_read(c, ACC_HUB_TD_FINE, out);
}
extern "C" int dqmc_hubbard_td_fine_counts_host(dqmc_ctx* c, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (const int rc = hubbard_fine_ok(c, "dqmc_hubbard_td_fine_counts_host")) return rc;
    const AccBlock& a = c->acc[ACC_HUB_TD_FINE];
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(copy_sync(c, out, (const char*)a.p + (size_t)c->sel * a.stride, (size_t)(c->m + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" size_t dqmc_hubbard_td_matsubara_size(dqmc_ctx* c, int nfreq) {
    if (!c || !c->hm.hubbard || !c->acc[ACC_HUB_TD_FINE].n || nfreq < 1 || nfreq > c->m) return 0;
    return (size_t)c->nb * HUB_EQ_CH * nfreq * c->N * 2;
}
extern "C" int dqmc_hubbard_td_matsubara_host(dqmc_ctx* c, int nfreq, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (const int rc = hubbard_fine_ok(c, "dqmc_hubbard_td_matsubara_host")) return rc;
    if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "nfreq must be in 1..m");
    (void)hipSetDevice(c->p.device);
    const size_t n_out = dqmc_hubbard_td_matsubara_size(c, nfreq), need = n_out + (size_t)c->nb;
    if (need > c->mats_cap) {
        HIPCHK(hipStreamSynchronize(c->st));
        if (c->mats_out) { (void)hipFree(c->mats_out); c->mats_out = nullptr; c->mats_cap = 0; }
        HIPCHK(hipMalloc((void**)&c->mats_out, need * sizeof(double)));
        c->mats_cap = need;
    }
    bool launched;
    {
        ProfScope ps(c, FAM_OTHER, 1);
        launched = launch_hubbard_td_matsubara(c->lc, c->hm, c->acc[ACC_HUB_TD_FINE].p, nfreq, c->mats_out, c->mats_out + n_out);
    }
    if (!launched) return fail(DQMC_EINVAL, "dqmc_hubbard_td_matsubara_host: the lattice is too large for the kernel's LDS");
    { const int rc = finish(c, "dqmc_hubbard_td_matsubara_host"); if (rc != DQMC_OK) return rc; }
    std::vector<double> bad((size_t)c->nb);
    HIPCHK(copy_sync(c, bad.data(), c->mats_out + n_out, bad.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (double b : bad) if (b != 0.0) return fail(DQMC_EINVAL, "an every-slice row has no sample: the measurement sweep did not visit every time slice");
    HIPCHK(copy_sync(c, out, c->mats_out, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
static int td_ncomp(const dqmc_ctx* c, int channel) { return channel == 6 ? c->cpr_count : channel == 5 ? c->cst_count : channel == 2 ? 3 : 2; }
// the Matsubara launch of one every-slice block; channels 5 and 6 bring their component count and their own chain stride
static bool mats_launch(dqmc_ctx* c, int ch, int nfreq, double* out, double* bad, size_t out_chain_stride) {
    const AccBlock& a = c->acc[ACC_FINE0 + ch];
    return launch_td_matsubara(c->lc, c->hm, a.p, ch, nfreq, ser_apbx(c), ser_apby(c), out, bad, out_chain_stride, td_ncomp(c, ch), a.stride);
}
extern "C" size_t dqmc_measure_td_matsubara_size(dqmc_ctx* c, int channel, int nfreq) {
    if (!c || channel == 7 || !td_fine_n(c, channel) || nfreq < 1 || nfreq > c->m) return 0;      // channel 7: channel 0 serves G(k, i omega_n)
    return (size_t)c->nb * td_ncomp(c, channel) * nfreq * c->N * 2;
}
extern "C" int dqmc_measure_td_matsubara_host(dqmc_ctx* c, int channel, int nfreq, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    if (c->hm.hubbard) return fail(DQMC_EINVAL, "dqmc_measure_td_matsubara_host belongs to the SDW model (Hubbard: dqmc_hubbard_td_matsubara_host)");
    if (!c->td_fine) return fail(DQMC_EINVAL, "context created without DQMC_TD_EVERY_SLICE");
    if (!td_fine_n(c, channel)) return fail(DQMC_EINVAL, c->acc[ACC_FINE0].missing);
    if (channel == 7) return fail(DQMC_EINVAL, "dqmc_measure_td_matsubara_host: the averaged Green's function block has no transform (channel 0 serves G(k, i omega_n))");
    if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "nfreq must be in 1..m");
    (void)hipSetDevice(c->p.device);
    const size_t n_out = dqmc_measure_td_matsubara_size(c, channel, nfreq), need = n_out + (size_t)c->nb;
    if (need > c->mats_cap) {
        HIPCHK(hipStreamSynchronize(c->st));
        if (c->mats_out) { (void)hipFree(c->mats_out); c->mats_out = nullptr; c->mats_cap = 0; }
        HIPCHK(hipMalloc((void**)&c->mats_out, need * sizeof(double)));
        c->mats_cap = need;
    }
    bool launched;
    {
        ProfScope ps(c, FAM_OTHER, 1);
        launched = mats_launch(c, channel, nfreq, c->mats_out, c->mats_out + n_out, 0);
    }
    if (!launched) return fail(DQMC_EINVAL, "dqmc_measure_td_matsubara_host: the lattice is too large for the kernel's LDS");
    { const int rc = finish(c, "dqmc_measure_td_matsubara_host"); if (rc != DQMC_OK) return rc; }
    std::vector<double> bad((size_t)c->nb);
    HIPCHK(copy_sync(c, bad.data(), c->mats_out + n_out, bad.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (double b : bad) if (b != 0.0) return fail(DQMC_EINVAL, "an every-slice row has no sample: the measurement sweep did not visit every time slice");
    HIPCHK(copy_sync(c, out, c->mats_out, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}

// ---------------------------------------------------------------------------------------------
// measurement series (dqmc_hip.h; kernels in kernels_measure.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dqmc_series_begin(dqmc_ctx* c, int bin_size, int max_bins, int nfreq, int parts) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (c->ser.open) return fail(DQMC_EINVAL, "a measurement series is already open (dqmc_series_end)");
    const int hub_mask = DQMC_SERIES_HUB_SCALARS | DQMC_SERIES_HUB_EQ | DQMC_SERIES_HUB_TD;
    if (c->hm.hubbard && (parts <= 0 || (parts & ~hub_mask)))
        return fail(DQMC_EINVAL, "dqmc_series_begin: on a Hubbard context parts must be a non-empty mask of bits 14 .. 16 (the other parts belong to the SDW model)");
    if (!c->hm.hubbard && (parts <= 0 || (parts & ~0x3fdf))) return fail(DQMC_EINVAL, "dqmc_series_begin: parts must be a non-empty mask of bits 0 .. 4 and 6 .. 13");
    if (bin_size < 1) return fail(DQMC_EINVAL, "dqmc_series_begin: bin_size must be at least 1");
    if (max_bins < 2) return fail(DQMC_EINVAL, "dqmc_series_begin: max_bins must be at least 2");
    if ((parts & DQMC_SERIES_HUB_EQ) && !c->acc[ACC_HUB_EQ].n)
        return fail(DQMC_EINVAL, "dqmc_series_begin: the Hubbard equal-time block has never been enabled (dqmc_hubbard_set_equal_time_correlators)");
    if ((parts & DQMC_SERIES_HUB_TD) && (!c->acc[ACC_HUB_TD].n || c->n < 2))
        return fail(DQMC_EINVAL, "dqmc_series_begin: no time-displaced block (a Hubbard context created with timedisplaced = 1, td_particle_hole = 1 and n >= 2)");
    if ((parts & (DQMC_SERIES_HUB_EQ | DQMC_SERIES_HUB_TD)) && series_eq_sample_lds_bytes(c->hm.L) > 152 * 1024)
        return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the sample kernels' LDS");
    if ((parts & 1) && !c->acc[ACC_EQ].n) return fail(DQMC_EINVAL, "dqmc_series_begin: the equal-time block has never been enabled (dqmc_set_equal_time_correlators)");
    if ((parts & DQMC_SERIES_EQ_BAND) && !c->acc[ACC_EQ_BAND].n) return fail(DQMC_EINVAL, "dqmc_series_begin: the equal-time band block has never been enabled (dqmc_set_equal_time_band)");
    if ((parts & DQMC_SERIES_EQ_CUSTOM) && !c->acc[ACC_EQ_CUSTOM].n) return fail(DQMC_EINVAL, "dqmc_series_begin: no user-defined bilinear is set (dqmc_set_custom_bilinears)");
    if ((parts & (DQMC_SERIES_MATS_CUSTOM_PAIR | DQMC_SERIES_EQ_CUSTOM_PAIR)) && !c->cpr_count)
        return fail(DQMC_EINVAL, "dqmc_series_begin: no user-defined pair operator is set (dqmc_set_custom_pair_operators): the part's block is missing");
    if ((parts & DQMC_SERIES_GREEN_MATRIX) && (!c->gm_on || !td_fine_n(c, 7)))
        return fail(DQMC_EINVAL, "dqmc_series_begin: the averaged Green's function has no every-slice block (dqmc_set_green_matrix, DQMC_TD_EVERY_SLICE)");
    if ((parts & (1 | DQMC_SERIES_EQ_BAND | DQMC_SERIES_EQ_CUSTOM | DQMC_SERIES_EQ_CUSTOM_PAIR)) && series_eq_sample_lds_bytes(c->hm.L) > 152 * 1024)
        return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the equal-time sample kernel's LDS");
    dqmc_ctx::Series s;
    const size_t N = (size_t)c->N;
    if (parts & 1) { s.off[0] = 0; s.len[0] = 10 * N; s.S = 10 * N; }
    for (int ch = 0; ch < 4; ++ch) {
        if (!(parts & (2 << ch))) continue;
        if (!c->td_fine || !td_fine_n(c, ch)) return fail(DQMC_EINVAL, "dqmc_series_begin: no every-slice block for a channel of the mask");
        if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "dqmc_series_begin: nfreq must be in 1..m");
        if (!td_matsubara_fits(c->hm, ch, nfreq)) return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the Matsubara kernel's LDS");
        s.off[1 + ch] = s.S; s.len[1 + ch] = (size_t)(ch == 2 ? 3 : 2) * nfreq * N * 2; s.S += s.len[1 + ch];
    }
    if (parts & DQMC_SERIES_PHI) {                          // the field always exists: no block to ask for
        if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "dqmc_series_begin: nfreq must be in 1..m");
        if (series_phi_sample_fgroup(c->hm.L, c->m, nfreq) < 1)
            return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the order-parameter sample kernel's LDS");
        s.off[6] = s.S; s.len[6] = (size_t)nfreq * N + 5; s.S += s.len[6];
    }
    if (parts & DQMC_SERIES_MATS_BAND) {                    // the new parts lie behind every part that existed before them
        if (!c->td_fine || !td_fine_n(c, 4)) return fail(DQMC_EINVAL, "dqmc_series_begin: no every-slice block for a channel of the mask");
        if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "dqmc_series_begin: nfreq must be in 1..m");
        if (!td_matsubara_fits(c->hm, 4, nfreq)) return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the Matsubara kernel's LDS");
        s.off[7] = s.S; s.len[7] = (size_t)2 * nfreq * N * 2; s.S += s.len[7];
    }
    if (parts & DQMC_SERIES_EQ_BAND) { s.off[8] = s.S; s.len[8] = 4 * N; s.S += s.len[8]; }
    if (parts & DQMC_SERIES_MATS_CUSTOM) {                  // the parts of the user-defined bilinears: behind everything else again
        if (!c->td_fine || !td_fine_n(c, 5)) return fail(DQMC_EINVAL, "dqmc_series_begin: no every-slice block for a channel of the mask");
        if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "dqmc_series_begin: nfreq must be in 1..m");
        if (!td_matsubara_fits(c->hm, 5, nfreq)) return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the Matsubara kernel's LDS");
        s.off[9] = s.S; s.len[9] = (size_t)c->cst_count * nfreq * N * 2; s.S += s.len[9];
    }
    if (parts & DQMC_SERIES_EQ_CUSTOM) { s.off[10] = s.S; s.len[10] = (size_t)2 * c->cst_count * N; s.S += s.len[10]; }
    if (parts & DQMC_SERIES_MATS_CUSTOM_PAIR) {             // the parts of the user-defined pair operators: behind everything else again
        if (!c->td_fine || !td_fine_n(c, 6)) return fail(DQMC_EINVAL, "dqmc_series_begin: no every-slice block for a channel of the mask");
        if (nfreq < 1 || nfreq > c->m) return fail(DQMC_EINVAL, "dqmc_series_begin: nfreq must be in 1..m");
        if (!td_matsubara_fits(c->hm, 6, nfreq)) return fail(DQMC_EINVAL, "dqmc_series_begin: the lattice is too large for the Matsubara kernel's LDS");
        s.off[11] = s.S; s.len[11] = (size_t)c->cpr_count * nfreq * N * 2; s.S += s.len[11];
    }
    if (parts & DQMC_SERIES_EQ_CUSTOM_PAIR) { s.off[12] = s.S; s.len[12] = (size_t)2 * c->cpr_count * N; s.S += s.len[12]; }
    if (parts & DQMC_SERIES_GREEN_MATRIX) {                 // the averaged Green's function: behind all older parts
        s.off[13] = s.S; s.len[13] = (size_t)(c->m + 1) * measure_green_matrix_row_doubles(c->p.opdim, c->N); s.S += s.len[13];
    }
    // the parts of a Hubbard context, behind every SDW bit: scalars and zcorr, C_X(d) / S_X(q) [8][N] each, C_X(d, tau_j) / S_X(q, tau_j) [n-1][6][N] each
    if (parts & DQMC_SERIES_HUB_SCALARS) { s.off[14] = s.S; s.len[14] = 8 + N; s.S += s.len[14]; }
    if (parts & DQMC_SERIES_HUB_EQ) { s.off[15] = s.S; s.len[15] = (size_t)2 * HUB_EQ_CH * N; s.S += s.len[15]; }
    if (parts & DQMC_SERIES_HUB_TD) { s.off[16] = s.S; s.len[16] = (size_t)2 * HUB_TD_CH * (c->n - 1) * N; s.S += s.len[16]; }
    s.bin_size = bin_size; s.max_bins = max_bins; s.parts = parts;
    s.nfreq = (parts & (0x1e | DQMC_SERIES_PHI | DQMC_SERIES_MATS_BAND | DQMC_SERIES_MATS_CUSTOM | DQMC_SERIES_MATS_CUSTOM_PAIR)) ? nfreq : 0;
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, L = (size_t)c->hm.L;
    c->ser = s;                                             // from here on series_free releases what was allocated
    dqmc_ctx::Series& r = c->ser;
    hipError_t e = (parts & DQMC_SERIES_PHI) ? series_phi_sample_prepare() : hipSuccess;   // an attribute failure is an error here, not at launch
    if (e == hipSuccess) e = hipMalloc((void**)&r.sample, n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r.openbin, n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r.bins, (size_t)max_bins * n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r.bad, (size_t)dqmc_ctx::SERIES_AUX_ROWS * c->nb * sizeof(double));
    const size_t mt = (parts & DQMC_SERIES_PHI) ? (size_t)c->m : 0;     // the temporal table of the order-parameter part
    if (e == hipSuccess) e = hipMalloc((void**)&r.trig, 2 * (L + mt) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r.stat, (2 * n + (size_t)dqmc_ctx::SERIES_AUX_ROWS * c->nb) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&r.srctab, (size_t)c->nb * sizeof(const double*));
    if (e == hipSuccess) e = hipMemsetAsync(r.sample, 0, n * sizeof(double), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(r.openbin, 0, n * sizeof(double), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(r.bins, 0, (size_t)max_bins * n * sizeof(double), c->st);
    if (e == hipSuccess) e = hipMemsetAsync(r.bad, 0, (size_t)dqmc_ctx::SERIES_AUX_ROWS * c->nb * sizeof(double), c->st);
    if (e == hipSuccess) {
        // cos / sin(2 pi j / L) as finishFermionic of the host layer forms them: the device's structure factors use the same values
        std::vector<double> trig(2 * (L + mt));
        for (size_t j = 0; j < L; ++j) { trig[j] = std::cos(2.0 * M_PI * double(j) / double(L)); trig[L + j] = std::sin(2.0 * M_PI * double(j) / double(L)); }
        for (size_t j = 0; j < mt; ++j) { trig[2 * L + j] = std::cos(2.0 * M_PI * double(j) / double(mt)); trig[2 * L + mt + j] = std::sin(2.0 * M_PI * double(j) / double(mt)); }
        e = copy_sync(c, r.trig, trig.data(), trig.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { series_free(c); return fail(DQMC_EHIP, std::string("dqmc_series_begin: ") + hipGetErrorString(e)); }
    r.open = true;
    return DQMC_OK;
}
extern "C" int dqmc_series_end(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->ser.open) return fail(DQMC_EINVAL, "no measurement series is open");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    series_free(c);
    return DQMC_OK;
}
extern "C" int dqmc_series_layout(dqmc_ctx* c, int part, size_t* offset, size_t* length) {
    if (!c || !offset || !length) return fail(DQMC_EINVAL, "null argument");
    if (!c->ser.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (part < 0 || part > 16 || !(c->ser.parts & (1 << part))) return fail(DQMC_EINVAL, "dqmc_series_layout: the part is not in the series");
    *offset = c->ser.off[part]; *length = c->ser.len[part];
    return DQMC_OK;
}
extern "C" int dqmc_series_info(dqmc_ctx* c, int* bins_closed, int* sweeps_in_open_bin, size_t* sample_len) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    if (!c->ser.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (bins_closed) *bins_closed = c->ser.closed;
    if (sweeps_in_open_bin) *sweeps_in_open_bin = c->ser.in_open;
    if (sample_len) *sample_len = c->ser.S;
    return DQMC_OK;
}
// The first half of dqmc_series_add_sweep: the sample of all chains from the blocks as they stand, and the flags read back.  `entry`
// names the public call in the messages.
static int series_form_sample(dqmc_ctx* c, const char* entry) {
    dqmc_ctx::Series& s = c->ser;
    const std::string who(entry);
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (s.closed >= s.max_bins) return fail(DQMC_EINVAL, who + ": the series is full (max_bins bins are closed)");
    (void)hipSetDevice(c->p.device);
    s.formed = false;                                       // the sample buffer is rewritten from here on
    // the flags of the parts behind each other, [part][chain]
    int nparts = 0;
    {
        ProfScope ps(c, FAM_OTHER, 0);
        if (s.parts & 1) {
            if (!launch_series_eq_sample(c->lc, c->hm, c->acc[ACC_EQ].p, c->acc[ACC_EQ].n, 5, s.trig, s.sample, s.S, s.off[0], s.bad))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the equal-time sample kernel's LDS");
            ++nparts;
        }
        for (int ch = 0; ch < 4; ++ch)
            if (s.parts & (2 << ch)) {
                if (!launch_td_matsubara(c->lc, c->hm, c->acc[ACC_FINE0 + ch].p, ch, s.nfreq, ser_apbx(c), ser_apby(c), s.sample + s.off[1 + ch],
                                         s.bad + (size_t)nparts * c->nb, s.S))
                    return fail(DQMC_EINVAL, who + ": the lattice is too large for the Matsubara kernel's LDS");
                ++nparts;
            }
        if (s.parts & DQMC_SERIES_MATS_BAND) {
            if (!launch_td_matsubara(c->lc, c->hm, c->acc[ACC_FINE0 + 4].p, 4, s.nfreq, ser_apbx(c), ser_apby(c), s.sample + s.off[7],
                                     s.bad + (size_t)nparts * c->nb, s.S))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the Matsubara kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_EQ_BAND) {
            if (!launch_series_eq_sample(c->lc, c->hm, c->acc[ACC_EQ_BAND].p, c->acc[ACC_EQ_BAND].n, 2, s.trig, s.sample, s.S, s.off[8],
                                         s.bad + (size_t)nparts * c->nb))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the equal-time sample kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_MATS_CUSTOM) {
            if (!mats_launch(c, 5, s.nfreq, s.sample + s.off[9], s.bad + (size_t)nparts * c->nb, s.S))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the Matsubara kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_EQ_CUSTOM) {
            if (!launch_series_eq_sample(c->lc, c->hm, c->acc[ACC_EQ_CUSTOM].p, c->acc[ACC_EQ_CUSTOM].n, c->cst_count, s.trig, s.sample, s.S, s.off[10],
                                         s.bad + (size_t)nparts * c->nb))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the equal-time sample kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_MATS_CUSTOM_PAIR) {
            if (!mats_launch(c, 6, s.nfreq, s.sample + s.off[11], s.bad + (size_t)nparts * c->nb, s.S))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the Matsubara kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_EQ_CUSTOM_PAIR) {
            const AccBlock& a = c->acc[ACC_EQ_CUSTOM_PAIR];
            if (!launch_series_eq_sample(c->lc, c->hm, a.p, a.n, c->cpr_count, s.trig, s.sample, s.S, s.off[12], s.bad + (size_t)nparts * c->nb))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the equal-time sample kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_GREEN_MATRIX) {
            const AccBlock& a = c->acc[ACC_FINE0 + 7];
            launch_series_green_sample(c->lc, c->hm, a.p, a.stride, s.sample, s.S, s.off[13], s.bad + (size_t)nparts * c->nb);
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_HUB_SCALARS) {
            launch_hubbard_series_scalars(c->lc, c->hm, c->acc[ACC_SLICE].p, c->p.txhor, c->p.u, c->p.mux, s.sample, s.S, s.off[14],
                                          s.bad + (size_t)nparts * c->nb);
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_HUB_EQ) {                 // the block has the count, [nch][N] layout of the SDW equal-time blocks
            const AccBlock& a = c->acc[ACC_HUB_EQ];
            if (!launch_series_eq_sample(c->lc, c->hm, a.p, a.n, HUB_EQ_CH, s.trig, s.sample, s.S, s.off[15], s.bad + (size_t)nparts * c->nb))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the equal-time sample kernel's LDS");
            ++nparts;
        }
        if (s.parts & DQMC_SERIES_HUB_TD) {
            if (!launch_hubbard_series_td_sample(c->lc, c->hm, c->acc[ACC_HUB_TD].p, s.trig, s.sample, s.S, s.off[16], s.bad + (size_t)nparts * c->nb))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the time-displaced sample kernel's LDS");
            ++nparts;
        }
        c->fam_launches[FAM_OTHER] += (uint64_t)nparts;
        if (s.parts & DQMC_SERIES_PHI) {                    // after the other parts; no flag row: the field always exists
            if (!launch_series_phi_sample(c->lc, c->hm, s.trig, s.trig + 2 * (size_t)c->hm.L, s.nfreq, s.sample, s.S, s.off[6]))
                return fail(DQMC_EINVAL, who + ": the lattice is too large for the order-parameter sample kernel's LDS");
            ++c->fam_launches[FAM_OTHER];
        }
    }
    { const int rc = finish(c, entry); if (rc != DQMC_OK) return rc; }
    std::vector<double> bad((size_t)nparts * c->nb);
    if (nparts) HIPCHK(copy_sync(c, bad.data(), s.bad, bad.size() * sizeof(double), hipMemcpyDeviceToHost));
    else HIPCHK(hipStreamSynchronize(c->st));               // the order-parameter part alone: no flags, the call still synchronises
    for (double b : bad)
        if (b != 0.0) return fail(DQMC_EINVAL, who + ": a block of the series has no sample (equal-time count or an every-slice row count < 1)");
    s.formed = true;
    return DQMC_OK;
}
// true if [p, p + bytes) is device memory of `device`; a host address, an address the runtime does not know and a range that leaves its
// allocation are all false, and no error stays pending
static bool series_device_range(const void* p, size_t bytes, int device) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (attr.type != hipMemoryTypeDevice || attr.device != device) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uintptr_t lo = (uintptr_t)base, at = (uintptr_t)p;
    return at >= lo && bytes <= size && at - lo <= size - bytes;
}
// closed[k] = (closed[2k] + closed[2k+1]) * 0.5 for all slots; the caller has checked an even number of closed bins and the bin size
constexpr int SERIES_MAX_BIN_SIZE = 1 << 29;                // the largest bin_size that can still double: the result stays within 2^30
static int series_rebin(dqmc_ctx* c, const char* entry) {
    dqmc_ctx::Series& s = c->ser;
    if (s.closed > 0) {
        { ProfScope ps(c, FAM_OTHER, 1); launch_series_rebin(c->lc, s.bins, (size_t)c->nb * s.S, s.closed / 2); }
        { const int rc = finish(c, entry); if (rc != DQMC_OK) return rc; }
        HIPCHK(hipStreamSynchronize(c->st));
    }
    s.closed /= 2; s.bin_size *= 2; ++s.rebins;
    return DQMC_OK;
}
// The second half: open[s] += src[s][0 .. S) for every slot s of this context, src == nullptr: the context's own rows in order
static int series_accumulate(dqmc_ctx* c, const double* const* src, const char* entry) {
    dqmc_ctx::Series& s = c->ser;
    const std::string who(entry);
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!s.formed) return fail(DQMC_EINVAL, who + ": the context's sample is not formed (dqmc_series_form_sample)");
    if (s.closed >= s.max_bins) return fail(DQMC_EINVAL, who + ": the series is full (max_bins bins are closed)");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S;
    const int close = s.in_open + 1 == s.bin_size;
    if (!src) {
        ProfScope ps(c, FAM_OTHER, 1);
        launch_series_accum(c->lc, s.sample, s.openbin, s.bins + (size_t)s.closed * n, n, close, s.bin_size);
    } else {
        for (int b = 0; b < c->nb; ++b) {
            if (!src[b]) return fail(DQMC_EINVAL, who + ": a source row is null");
            if (((uintptr_t)src[b] & (sizeof(double) - 1)) || !series_device_range(src[b], s.S * sizeof(double), c->p.device))
                return fail(DQMC_EINVAL, who + ": a source row is not S doubles of device memory on the context's device");
        }
        s.srchost.assign(src, src + c->nb);                 // stays alive until the stream has taken the copy
        HIPCHK(hipMemcpyAsync((void*)s.srctab, s.srchost.data(), (size_t)c->nb * sizeof(const double*), hipMemcpyHostToDevice, c->st));
        ProfScope ps(c, FAM_OTHER, 1);
        launch_series_accum_routed(c->lc, s.srctab, s.openbin, s.bins + (size_t)s.closed * n, s.S, close, s.bin_size);
    }
    if (s.flags & DQMC_SERIES_TRACK_VARIANCE) {             // the same rows once more, into the running mean and m2 of the slot
        ProfScope ps(c, FAM_OTHER, 1);
        launch_series_welford(c->lc, s.sample, src ? s.srctab : nullptr, s.var, s.var + n, s.S, s.samples + 1);
    }
    s.formed = false;
    { const int rc = finish(c, entry); if (rc != DQMC_OK) return rc; }
    HIPCHK(hipStreamSynchronize(c->st));                    // the rows may belong to another context: they are free again on return
    ++s.samples;
    if (close) { ++s.closed; s.in_open = 0; } else ++s.in_open;
    // auto re-binning: the close that fills the series merges neighbouring bins before the call returns, so the series is never
    // observed full; if bin_size cannot double any more the series becomes full as it does without the flag
    if (close && (s.flags & DQMC_SERIES_AUTO_REBIN) && s.closed == s.max_bins && s.bin_size <= SERIES_MAX_BIN_SIZE) return series_rebin(c, entry);
    return DQMC_OK;
}
extern "C" int dqmc_series_form_sample(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    return series_form_sample(c, "dqmc_series_form_sample");
}
extern "C" int dqmc_series_sample_device(dqmc_ctx* c, const double** rows, size_t* S) {
    if (!c || !rows || !S) return fail(DQMC_EINVAL, "null argument");
    if (!c->ser.open) return fail(DQMC_EINVAL, "no measurement series is open");
    *rows = c->ser.sample; *S = c->ser.S;
    return DQMC_OK;
}
extern "C" int dqmc_series_accumulate(dqmc_ctx* c, const double* const* src) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    return series_accumulate(c, src, "dqmc_series_accumulate");
}
extern "C" int dqmc_series_add_sweep(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    const int rc = series_form_sample(c, "dqmc_series_add_sweep");
    return rc != DQMC_OK ? rc : series_accumulate(c, nullptr, "dqmc_series_add_sweep");
}
extern "C" int dqmc_series_read_bins_host(dqmc_ctx* c, int first, int count, double* out) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (first < 0 || count < 1 || first > s.closed || count > s.closed - first) return fail(DQMC_EINVAL, "dqmc_series_read_bins_host: bins outside the closed range");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S;
    HIPCHK(hipMemcpy2DAsync(out, s.S * sizeof(double), s.bins + (size_t)first * n + (size_t)c->sel * s.S, n * sizeof(double),
                            s.S * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return DQMC_OK;
}
extern "C" int dqmc_series_stats_host(dqmc_ctx* c, double* mean, double* err) {
    if (!c || !mean || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (s.closed < 2) return fail(DQMC_EINVAL, "dqmc_series_stats_host: the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S;
    { ProfScope ps(c, FAM_OTHER, 1); launch_series_stats(c->lc, s.bins, n, s.closed, s.stat, s.stat + n); }
    { const int rc = finish(c, "dqmc_series_stats_host"); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, mean, s.stat, n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, s.stat + n, n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_series_derived_host(dqmc_ctx* c, double* value, double* err) {
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (s.closed < 2) return fail(DQMC_EINVAL, "dqmc_series_derived_host: the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, nd = (size_t)6 * c->nb;
    double* dv = s.stat + 2 * n;
    {
        ProfScope ps(c, FAM_OTHER, 1);
        launch_series_derived(c->lc, c->hm, s.bins, s.S, s.closed, s.nfreq, (s.parts & 1) ? (long long)s.off[0] : -1,
                              (s.parts & 16) ? (long long)s.off[4] : -1, dv, dv + nd);
    }
    { const int rc = finish(c, "dqmc_series_derived_host"); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, dv + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_series_band_derived_host(dqmc_ctx* c, double* value, double* err) {
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & DQMC_SERIES_EQ_BAND)) return fail(DQMC_EINVAL, "dqmc_series_band_derived_host: the series has no equal-time band part");
    if (s.closed < 2) return fail(DQMC_EINVAL, "dqmc_series_band_derived_host: the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, nd = (size_t)3 * c->nb;
    double* dv = s.stat + 2 * n;                            // the result rows of dqmc_series_derived_host: the calls are synchronous
    { ProfScope ps(c, FAM_OTHER, 1); launch_series_band_derived(c->lc, c->hm, s.bins, s.S, s.closed, s.off[8], dv, dv + nd); }
    { const int rc = finish(c, "dqmc_series_band_derived_host"); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, dv + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// R of every operator of an equal-time part [count][N] C(d), [count][N] S(q) at series part `bit`: the user-defined bilinears and pair operators
static int series_ratio_derived(dqmc_ctx* c, int part, int bit, int count, int qx, int qy, double* value, double* err, const std::string& who,
                                const char* what) {
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & part)) return fail(DQMC_EINVAL, who + ": the series has no equal-time part of the user-defined " + what);
    if (qx < 0 || qx >= c->hm.L || qy < 0 || qy >= c->hm.L) return fail(DQMC_EINVAL, who + ": qx and qy must be in 0 .. L-1");
    if (s.closed < 2) return fail(DQMC_EINVAL, who + ": the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, nd = (size_t)count * c->nb;
    double* dv = s.stat + 2 * n;                            // the result rows of dqmc_series_derived_host: the calls are synchronous
    { ProfScope ps(c, FAM_OTHER, 1); launch_series_custom_derived(c->lc, c->hm, s.bins, s.S, s.closed, s.off[bit], count, qx, qy, dv, dv + nd); }
    { const int rc = finish(c, who.c_str()); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, dv + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_series_custom_derived_host(dqmc_ctx* c, int qx, int qy, double* value, double* err) {
    return series_ratio_derived(c, DQMC_SERIES_EQ_CUSTOM, 10, c ? c->cst_count : 0, qx, qy, value, err, "dqmc_series_custom_derived_host", "bilinears");
}
extern "C" int dqmc_series_custom_pair_derived_host(dqmc_ctx* c, int qx, int qy, double* value, double* err) {
    return series_ratio_derived(c, DQMC_SERIES_EQ_CUSTOM_PAIR, 12, c ? c->cpr_count : 0, qx, qy, value, err, "dqmc_series_custom_pair_derived_host",
                                "pair operators");
}
// R, xi of the eight equal-time channels of a Hubbard series and S, R, xi of the rotation-summed spin channel at Q = (qx, qy)
extern "C" int dqmc_series_hubbard_derived_host(dqmc_ctx* c, int qx, int qy, double* value, double* err) {
    const std::string who = "dqmc_series_hubbard_derived_host";
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & DQMC_SERIES_HUB_EQ)) return fail(DQMC_EINVAL, who + ": the series has no equal-time part of the Hubbard model (DQMC_SERIES_HUB_EQ)");
    if (qx < 0 || qx >= c->hm.L || qy < 0 || qy >= c->hm.L) return fail(DQMC_EINVAL, who + ": qx and qy must be in 0 .. L-1");
    if (s.closed < 2) return fail(DQMC_EINVAL, who + ": the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, nd = (size_t)19 * c->nb;
    double* dv = s.stat + 2 * n;                            // the result rows behind the statistics (SERIES_AUX_ROWS of them): the calls are synchronous
    { ProfScope ps(c, FAM_OTHER, 1); launch_series_hubbard_derived(c->lc, c->hm, s.bins, s.S, s.closed, s.off[15], qx, qy, dv, dv + nd); }
    { const int rc = finish(c, who.c_str()); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, dv + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// Bubble and vertex of every pair operator at Q = (qx, qy) (dqmc_hip.h): the bin means, then the two kernels of launch_series_pair_vertex.
// The scratch buffer s.vertex holds the bubbles pb [nb][B + 1][m + 1][count], then value and err [nb][count][5 + m] each
extern "C" size_t dqmc_series_pair_vertex_size(dqmc_ctx* c) {
    if (!c || !c->ser.open || (c->ser.parts & (DQMC_SERIES_MATS_CUSTOM_PAIR | DQMC_SERIES_GREEN_MATRIX)) != (DQMC_SERIES_MATS_CUSTOM_PAIR | DQMC_SERIES_GREEN_MATRIX))
        return 0;
    return (size_t)c->nb * c->cpr_count * (5 + c->m);
}
extern "C" int dqmc_series_pair_vertex_host(dqmc_ctx* c, int qx, int qy, double* value, double* err) {
    const std::string who = "dqmc_series_pair_vertex_host";
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & DQMC_SERIES_MATS_CUSTOM_PAIR) || !(s.parts & DQMC_SERIES_GREEN_MATRIX) || s.nfreq < 1)
        return fail(DQMC_EINVAL, who + ": the series needs the Matsubara part of the pair operators (bit 11) and the averaged Green's function (bit 13)");
    if (qx < 0 || qx >= c->hm.L || qy < 0 || qy >= c->hm.L) return fail(DQMC_EINVAL, who + ": qx and qy must be in 0 .. L-1");
    if (s.closed < 2) return fail(DQMC_EINVAL, who + ": the jackknife needs at least two closed bins");
    if (series_pair_bubble_lds_bytes(c->p.opdim, c->N) > 152 * 1024) return fail(DQMC_EINVAL, who + ": the lattice is too large for the bubble kernel's LDS");
    (void)hipSetDevice(c->p.device);
    const int count = c->cpr_count, B = s.closed;
    // the operator table: the measurement kernels' own while an operator has a bond part; otherwise built once per series (the
    // operators cannot change while a series holds bit 11) and kept in an allocation of its own, the table and then its masks
    if (!c->cpr_bond_on && !s.vertex_tab) {
        std::vector<dqmc_cplx> F[3];
        const cplx* src[3] = {c->cpr_F0, c->cpr_Fx, c->cpr_Fy};
        for (int k = 0; k < 3; ++k)
            for (int e = 0; e < 16 * count; ++e) F[k].push_back(dqmc_cplx{src[k][e].x, src[k][e].y});
        std::vector<cplx> tab;
        std::vector<unsigned> mk;
        CustomPair pair{};
        custom_pair_table(c, count, F[0].data(), F[1].data(), F[2].data(), tab, mk, pair);
        HIPCHK(hipMalloc((void**)&s.vertex_tab, tab.size() * sizeof(cplx) + mk.size() * sizeof(unsigned)));
        pair.tab = (const cplx*)s.vertex_tab; pair.mk = (const unsigned*)((const cplx*)s.vertex_tab + tab.size());
        hipError_t e = copy_sync(c, s.vertex_tab, tab.data(), tab.size() * sizeof(cplx), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = copy_sync(c, (void*)pair.mk, mk.data(), mk.size() * sizeof(unsigned), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(s.vertex_tab); s.vertex_tab = nullptr; HIPCHK(e); }
        s.vertex_pair = pair;
    }
    const CustomPair& pair = c->cpr_bond_on ? c->cpr_bond : s.vertex_pair;
    const size_t n = (size_t)c->nb * s.S, n_pb = (size_t)c->nb * (B + 1) * (c->m + 1) * count, n_out = dqmc_series_pair_vertex_size(c);
    const size_t need = n_pb + 2 * n_out;
    if (need > s.vertex_cap) {
        HIPCHK(hipStreamSynchronize(c->st));
        if (s.vertex) { (void)hipFree(s.vertex); s.vertex = nullptr; s.vertex_cap = 0; }
        HIPCHK(hipMalloc((void**)&s.vertex, need * sizeof(double)));
        s.vertex_cap = need;
    }
    double *pb = s.vertex, *dv = pb + n_pb, *de = dv + n_out;
    bool launched;
    {
        ProfScope ps(c, FAM_OTHER, 3);
        launch_series_stats(c->lc, s.bins, n, B, s.stat, s.stat + n);
        launched = launch_series_pair_vertex(c->lc, c->hm, s.bins, s.stat, s.trig, s.S, B, s.nfreq, s.off[11], s.off[13], count, pair, qx, qy,
                                             ser_apbx(c), ser_apby(c), pb, dv, de);
    }
    if (!launched) return fail(DQMC_EINVAL, who + ": the lattice is too large for the bubble kernel's LDS");
    { const int rc = finish(c, who.c_str()); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, n_out * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, de, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
// Particle-hole bubble and vertex of every user-defined bilinear at Q = (qx, qy) (dqmc_hip.h): the bin means, then the two kernels of
// launch_series_ph_vertex.  s.vertex holds the bubbles pb [nb][B + 1][m + 1][count], then value and err [nb][count][6 + m] each
static bool series_ph_vertex_ok(const dqmc_ctx* c) {
    return c && c->ser.open && (c->ser.parts & DQMC_SERIES_MATS_CUSTOM) && (c->ser.parts & DQMC_SERIES_GREEN_MATRIX) && c->cst_count > 0;
}
extern "C" size_t dqmc_series_ph_vertex_size(dqmc_ctx* c) {
    if (!series_ph_vertex_ok(c)) return 0;
    return (size_t)c->nb * c->cst_count * (6 + c->m);
}
extern "C" int dqmc_series_ph_vertex_host(dqmc_ctx* c, int qx, int qy, double* value, double* err) {
    const std::string who = "dqmc_series_ph_vertex_host";
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & DQMC_SERIES_MATS_CUSTOM) || !(s.parts & DQMC_SERIES_GREEN_MATRIX) || s.nfreq < 1)
        return fail(DQMC_EINVAL, who + ": the series needs the Matsubara part of the user-defined bilinears (bit 9) and the averaged Green's function (bit 13)");
    if (!c->cst_count) return fail(DQMC_EINVAL, who + ": no user-defined bilinear is set (dqmc_set_custom_bilinears)");
    if (qx < 0 || qx >= c->hm.L || qy < 0 || qy >= c->hm.L) return fail(DQMC_EINVAL, who + ": qx and qy must be in 0 .. L-1");
    if (s.closed < 2) return fail(DQMC_EINVAL, who + ": the jackknife needs at least two closed bins");
    if (series_ph_bubble_lds_bytes(c->p.opdim, c->N) > 152 * 1024) return fail(DQMC_EINVAL, who + ": the lattice is too large for the bubble kernel's LDS");
    (void)hipSetDevice(c->p.device);
    const int count = c->cst_count, B = s.closed;
    // the operator table: the measurement kernels' own while an operator has a bond part; otherwise built once per series (the
    // operators cannot change while a series holds bit 9) and kept in an allocation of its own, the table and then its masks
    if (!c->cst_bond_on && !s.ph_tab) {
        std::vector<dqmc_cplx> M0;
        for (int e = 0; e < 16 * count; ++e) M0.push_back(dqmc_cplx{c->cst_M[e].x, c->cst_M[e].y});
        std::vector<cplx> tab;
        std::vector<unsigned> mk;
        CustomBond bond{};
        custom_bond_table(c, count, M0.data(), nullptr, nullptr, tab, mk, bond);
        HIPCHK(hipMalloc((void**)&s.ph_tab, tab.size() * sizeof(cplx) + mk.size() * sizeof(unsigned)));
        bond.tab = (const cplx*)s.ph_tab; bond.mk = (const unsigned*)((const cplx*)s.ph_tab + tab.size());
        hipError_t e = copy_sync(c, s.ph_tab, tab.data(), tab.size() * sizeof(cplx), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = copy_sync(c, (void*)bond.mk, mk.data(), mk.size() * sizeof(unsigned), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(s.ph_tab); s.ph_tab = nullptr; HIPCHK(e); }
        s.ph_bond = bond;
    }
    const CustomBond& bond = c->cst_bond_on ? c->cst_bond : s.ph_bond;
    const size_t n = (size_t)c->nb * s.S, n_pb = (size_t)c->nb * (B + 1) * (c->m + 1) * count, n_out = dqmc_series_ph_vertex_size(c);
    const size_t need = n_pb + 2 * n_out;
    if (need > s.vertex_cap) {
        HIPCHK(hipStreamSynchronize(c->st));
        if (s.vertex) { (void)hipFree(s.vertex); s.vertex = nullptr; s.vertex_cap = 0; }
        HIPCHK(hipMalloc((void**)&s.vertex, need * sizeof(double)));
        s.vertex_cap = need;
    }
    double *pb = s.vertex, *dv = pb + n_pb, *de = dv + n_out;
    bool launched;
    {
        ProfScope ps(c, FAM_OTHER, 3);
        launch_series_stats(c->lc, s.bins, n, B, s.stat, s.stat + n);
        launched = launch_series_ph_vertex(c->lc, c->hm, s.bins, s.stat, s.trig, s.S, B, s.nfreq, s.off[9], s.off[13], count, bond, qx, qy,
                                           ser_apbx(c), ser_apby(c), pb, dv, de);
    }
    if (!launched) return fail(DQMC_EINVAL, who + ": the lattice is too large for the bubble kernel's LDS");
    { const int rc = finish(c, who.c_str()); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, n_out * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, de, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_series_phi_derived_host(dqmc_ctx* c, double* value, double* err) {
    if (!c || !value || !err) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (!(s.parts & DQMC_SERIES_PHI)) return fail(DQMC_EINVAL, "dqmc_series_phi_derived_host: the series has no order-parameter part");
    if (s.closed < 2) return fail(DQMC_EINVAL, "dqmc_series_phi_derived_host: the jackknife needs at least two closed bins");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, nd = (size_t)6 * c->nb;
    double* dv = s.stat + 2 * n;                            // the result rows of dqmc_series_derived_host: the calls are synchronous
    { ProfScope ps(c, FAM_OTHER, 1); launch_series_phi_derived(c->lc, c->hm, s.bins, s.S, s.closed, s.nfreq, s.off[6], dv, dv + nd); }
    { const int rc = finish(c, "dqmc_series_phi_derived_host"); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, value, dv, nd * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, err, dv + nd, nd * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}

// ---- long runs: options, re-binning, binning analysis, export / import (dqmc_hip.h) ----
static bool series_flags_valid(int flags, int max_bins) {
    if (flags & ~(DQMC_SERIES_AUTO_REBIN | DQMC_SERIES_TRACK_VARIANCE)) return false;
    return !(flags & DQMC_SERIES_AUTO_REBIN) || (max_bins >= 4 && max_bins % 2 == 0);
}
// w and m2 [nb][S], zeroed; kept until the series ends once they exist
static hipError_t series_alloc_variance(dqmc_ctx* c) {
    dqmc_ctx::Series& s = c->ser;
    const size_t bytes = 2 * (size_t)c->nb * s.S * sizeof(double);
    if (!s.var) {
        const hipError_t e = hipMalloc((void**)&s.var, bytes);
        if (e != hipSuccess) { s.var = nullptr; return e; }
    }
    return hipMemsetAsync(s.var, 0, bytes, c->st);
}
extern "C" int dqmc_series_configure(dqmc_ctx* c, int flags) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (s.samples || s.closed || s.in_open) return fail(DQMC_EINVAL, "dqmc_series_configure: the series is not empty any more");
    if (!series_flags_valid(flags, s.max_bins))
        return fail(DQMC_EINVAL, "dqmc_series_configure: unknown flag, or DQMC_SERIES_AUTO_REBIN with max_bins odd or below 4");
    (void)hipSetDevice(c->p.device);
    if (flags & DQMC_SERIES_TRACK_VARIANCE) {
        HIPCHK(series_alloc_variance(c));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    s.flags = flags;
    return DQMC_OK;
}
static void series_fill_state(const dqmc_ctx* c, dqmc_series_state* st) {
    const dqmc_ctx::Series& s = c->ser;
    std::memset(st, 0, sizeof(*st));
    st->bin_size = s.bin_size; st->max_bins = s.max_bins; st->nfreq = s.nfreq; st->parts = s.parts; st->flags = s.flags;
    st->bins_closed = s.closed; st->sweeps_in_open_bin = s.in_open; st->nb = c->nb;
    st->samples = s.samples; st->rebins = s.rebins; st->sample_len = s.S;
}
extern "C" int dqmc_series_get_state(dqmc_ctx* c, dqmc_series_state* st) {
    if (!c || !st) return fail(DQMC_EINVAL, "null argument");
    if (!c->ser.open) return fail(DQMC_EINVAL, "no measurement series is open");
    series_fill_state(c, st);
    return DQMC_OK;
}
extern "C" int dqmc_series_rebin(dqmc_ctx* c) {
    if (!c) return fail(DQMC_EINVAL, "null ctx");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (s.closed % 2) return fail(DQMC_EINVAL, "dqmc_series_rebin: the number of closed bins is odd");
    if (s.bin_size > SERIES_MAX_BIN_SIZE) return fail(DQMC_EINVAL, "dqmc_series_rebin: bin_size cannot double any more");
    (void)hipSetDevice(c->p.device);
    return series_rebin(c, "dqmc_series_rebin");
}
extern "C" int dqmc_series_binning_host(dqmc_ctx* c, int levels, double* err, double* tau) {
    if (!c || !err) return fail(DQMC_EINVAL, "null argument");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (levels < 1 || levels > 12) return fail(DQMC_EINVAL, "dqmc_series_binning_host: levels must be in 1..12");
    if ((s.closed >> (levels - 1)) < 2) return fail(DQMC_EINVAL, "dqmc_series_binning_host: the top level needs at least two merged bins");
    if (tau && !(s.flags & DQMC_SERIES_TRACK_VARIANCE)) return fail(DQMC_EINVAL, "dqmc_series_binning_host: tau needs DQMC_SERIES_TRACK_VARIANCE");
    if (tau && s.samples < 2) return fail(DQMC_EINVAL, "dqmc_series_binning_host: tau needs at least two samples");
    (void)hipSetDevice(c->p.device);
    const size_t n = (size_t)c->nb * s.S, need = 2 * (size_t)levels * n;
    if (need > s.binning_cap) {
        HIPCHK(hipStreamSynchronize(c->st));
        if (s.binning) { (void)hipFree(s.binning); s.binning = nullptr; s.binning_cap = 0; }
        HIPCHK(hipMalloc((void**)&s.binning, need * sizeof(double)));
        s.binning_cap = need;
    }
    double* derr = s.binning;
    double* dtau = tau ? s.binning + (size_t)levels * n : nullptr;
    {
        ProfScope ps(c, FAM_OTHER, 1);
        launch_series_binning(c->lc, s.bins, tau ? s.var + n : nullptr, n, s.closed, levels, s.bin_size, s.samples, derr, dtau);
    }
    { const int rc = finish(c, "dqmc_series_binning_host"); if (rc != DQMC_OK) return rc; }
    HIPCHK(copy_sync(c, err, derr, (size_t)levels * n * sizeof(double), hipMemcpyDeviceToHost));
    if (tau) HIPCHK(copy_sync(c, tau, dtau, (size_t)levels * n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
static size_t series_export_len(size_t n, int closed, int flags) {
    return ((size_t)closed + 1 + ((flags & DQMC_SERIES_TRACK_VARIANCE) ? 2 : 0)) * n;
}
extern "C" int dqmc_series_export_host(dqmc_ctx* c, double* out, size_t len) {
    if (!c || !out) return fail(DQMC_EINVAL, "null argument");
    const dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    const size_t n = (size_t)c->nb * s.S;
    if (len != series_export_len(n, s.closed, s.flags)) return fail(DQMC_EINVAL, "dqmc_series_export_host: len is not the size of the series");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    const size_t nc = (size_t)s.closed * n;
    if (nc) HIPCHK(copy_sync(c, out, s.bins, nc * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, out + nc, s.openbin, n * sizeof(double), hipMemcpyDeviceToHost));
    if (s.flags & DQMC_SERIES_TRACK_VARIANCE) HIPCHK(copy_sync(c, out + nc + n, s.var, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    return DQMC_OK;
}
extern "C" int dqmc_series_import_host(dqmc_ctx* c, const dqmc_series_state* st, const double* in, size_t len) {
    if (!c || !st || !in) return fail(DQMC_EINVAL, "null argument");
    dqmc_ctx::Series& s = c->ser;
    if (!s.open) return fail(DQMC_EINVAL, "no measurement series is open");
    if (st->nb != c->nb || st->sample_len != s.S || st->parts != s.parts || st->nfreq != s.nfreq)
        return fail(DQMC_EINVAL, "dqmc_series_import_host: chains, sample length, parts or nfreq differ from the open series");
    if (st->bins_closed < 0 || st->bins_closed >= s.max_bins) return fail(DQMC_EINVAL, "dqmc_series_import_host: bins_closed must be below max_bins of the open series");
    if (st->bin_size < 1 || st->sweeps_in_open_bin < 0 || st->sweeps_in_open_bin >= st->bin_size)
        return fail(DQMC_EINVAL, "dqmc_series_import_host: sweeps_in_open_bin must be below bin_size");
    if (!series_flags_valid(st->flags, s.max_bins)) return fail(DQMC_EINVAL, "dqmc_series_import_host: the flags are not valid for max_bins of the open series");
    if (st->samples < 0 || st->rebins < 0) return fail(DQMC_EINVAL, "dqmc_series_import_host: negative counter");
    const size_t n = (size_t)c->nb * s.S;
    if (len != series_export_len(n, st->bins_closed, st->flags)) return fail(DQMC_EINVAL, "dqmc_series_import_host: len is not the size of the series");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    if ((st->flags & DQMC_SERIES_TRACK_VARIANCE) && !s.var) HIPCHK(series_alloc_variance(c));   // nothing of the series has changed yet
    const size_t nc = (size_t)st->bins_closed * n;
    if (nc) HIPCHK(copy_sync(c, s.bins, in, nc * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(c, s.openbin, in + nc, n * sizeof(double), hipMemcpyHostToDevice));
    if (st->flags & DQMC_SERIES_TRACK_VARIANCE) HIPCHK(copy_sync(c, s.var, in + nc + n, 2 * n * sizeof(double), hipMemcpyHostToDevice));
    s.bin_size = st->bin_size; s.flags = st->flags; s.closed = st->bins_closed; s.in_open = st->sweeps_in_open_bin;
    s.samples = st->samples; s.rebins = st->rebins; s.formed = false;
    return DQMC_OK;
}

extern "C" int dqmc_get_green_td_fine_host(dqmc_ctx* c, dqmc_cplx* g_t0, dqmc_cplx* g_0t, dqmc_cplx* g_tt, int* slice) {
    if (!c || !g_t0 || !g_0t || !g_tt || !slice) return fail(DQMC_EINVAL, "null argument");
    if (!c->td_fine || c->fine_slice < 0) return fail(DQMC_EINVAL, "no every-slice Green's function has been propagated");
    (void)hipSetDevice(c->p.device);
    HIPCHK(hipStreamSynchronize(c->st));
    HIPCHK(hipGetLastError());
    const size_t bytes = (size_t)c->n_g * c->n_g * sizeof(cplx);
    HIPCHK(copy_sync(c, g_t0, selp(c, c->fGT0), bytes, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, g_0t, selp(c, c->fG0T), bytes, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(c, g_tt, selp(c, c->fGTT), bytes, hipMemcpyDeviceToHost));
    *slice = c->fine_slice;
    return DQMC_OK;
}
