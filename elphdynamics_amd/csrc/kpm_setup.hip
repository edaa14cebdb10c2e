// kpm_setup.hip — the KPM preconditioner's entry points: elph_kpm_create, setup!(P) for every resident chain, its injected forms,
// elph_kpm_apply.  Host orchestration only: the planning is kpm_host.cpp's (pure), the kernels are kpm_dev.hip's and kernels.hip's.

#include <cmath>
#include <cstdlib>

#include "elph_internal.h"

void elph_kpm_free(elph_handle_s *h) {
    KpmState &K = h->kpm;
    void *ptrs[] = {K.d_Ebar, K.d_cbar, K.d_sbar, K.d_lp_cbar, K.d_lp_sbar, K.d_sq_cbar, K.d_sq_sbar, K.d_order, K.d_coff, K.d_wsched,
                    K.d_desc, K.d_fold, K.d_lam, K.d_coeff, K.d_start};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    K = KpmState();
}

extern "C" int elph_kpm_create(elph_handle h, int n, double buf, double c1, double c2) {
    CHECK_H(h);
    if (n < 1 || !(buf >= 0.0)) { elph_set_error("bad KPM parameters"); return ELPH_E_ARG; }
    // KPMExpansion ctor, KPMPreconditioners.jl:101-146: λ_lo = 0, λ_hi = 2, order 1 everywhere (one per chain, made on demand)
    elph_kpm_free(h);
    h->kpm.par = {n, buf, c1, c2};
    h->kpm.ssh = h->kind == ELPH_MODEL_SSH; h->kpm.created = true;
    return ELPH_OK;
}

// (re)size the per-chain host state and the device buffers for nch chains
static int kpm_reserve(elph_handle_s *h, int nch) {
    KpmState &K = h->kpm;
    const int Lo2 = (int)((h->L + 1) / 2);
    // a different number of configurations: every expansion starts from the constructor state again
    if (K.nch() != nch) K.chains.assign((size_t)nch, KpmChain(Lo2));
    K.h_Ebar.resize((size_t)nch * h->N);
    if (nch > K.tab_cap) {
        RC(dev_alloc(&K.d_Ebar, (size_t)nch * h->N));
        RC(dev_alloc(&K.d_order, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_coff, (size_t)nch * (Lo2 + 1)));
        RC(dev_alloc(&K.d_wsched, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_desc, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_fold, (size_t)nch * Lo2 * 2));
        RC(dev_alloc(&K.d_lam, (size_t)nch * 2));
        if (K.d_start) { HIPCHK(hipFree(K.d_start)); K.d_start = nullptr; }      // (made again for nch chains on its next use)
        K.tab_cap = nch;
    }
    const int hch = K.hop_per_chain() ? nch : 1;      // averaged hopping: one set per chain (SSH chains) or shared
    if (hch > K.hop_cap) {
        RC(dev_alloc(&K.d_cbar, (size_t)hch * h->nb));
        RC(dev_alloc(&K.d_sbar, (size_t)hch * h->nb));
        if (h->fast_capable) {
            RC(dev_alloc(&K.d_lp_cbar, (size_t)hch * h->lp_ne * ELPH_WAVE));
            RC(dev_alloc(&K.d_lp_sbar, (size_t)hch * h->lp_ne * ELPH_WAVE));
        }
        if (h->shape.sq_L() > 0) {
            RC(dev_alloc(&K.d_sq_cbar, (size_t)hch * 4 * h->N));
            RC(dev_alloc(&K.d_sq_sbar, (size_t)hch * 4 * h->N));
        }
        K.hop_cap = hch;
    }
    return ELPH_OK;
}

// Where update_A! takes its averaged inputs: the handle's own model, or the caller's — the full-lattice handle of a sharded HMC update holds
// no field of its own, so every rank contributes its own rows and the sum is injected (hmc.hip): Ē (Holstein) or c̄ / s̄ (bond phonons).
struct KpmSource { const double *Ebar = nullptr, *cbar = nullptr, *sbar = nullptr; };

// update_A! (KPMPreconditioners.jl:332-349 Holstein; :355-381 SSH) and the device images of the averaged hopping
static int kpm_update_A(elph_handle_s *h, const KpmSource &src) {
    KpmState &K = h->kpm;
    const int nch = K.nch();
    const size_t N = (size_t)h->N, nb = (size_t)h->nb;
    if (h->kind == ELPH_MODEL_HOLSTEIN) {
        // (Ē stays on the device: the Arnoldi kernel and the apply read it there)
        if (src.Ebar) HIPCHK(hipMemcpy(K.d_Ebar, src.Ebar, sizeof(double) * N, hipMemcpyHostToDevice));
        else RC(elph_launch_ebar(h, nch));
        K.h_cbar = h->h_c; K.h_sbar = h->h_s;
    } else {
        // Ebar = exp(dtau mu), held per chain (equal unless the chemical potential is tuned per chain)
        HIPCHK(hipMemcpyAsync(K.d_Ebar, h->d_E, sizeof(double) * nch * N, hipMemcpyDeviceToDevice, h->stream));
        if (src.cbar) { K.h_cbar.assign(src.cbar, src.cbar + nb); K.h_sbar.assign(src.sbar, src.sbar + nb); }
        K.h_cbar.resize(nch * nb); K.h_sbar.resize(nch * nb);
        if (nb > 0 && src.cbar) {
            HIPCHK(hipMemcpyAsync(K.d_cbar, K.h_cbar.data(), sizeof(double) * nch * nb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(K.d_sbar, K.h_sbar.data(), sizeof(double) * nch * nb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        } else if (nb > 0) {   // tau-means of cosht, sinht from the device tables (they may have been produced there)
            RC(elph_launch_cs_bar(h, K.d_cbar, K.d_sbar, nch));
            HIPCHK(hipMemcpyAsync(K.h_cbar.data(), K.d_cbar, sizeof(double) * nch * nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(K.h_sbar.data(), K.d_sbar, sizeof(double) * nch * nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    // Holstein: c̄ = cosh(Δτ t), s̄ = sinh(Δτ t) never change after elph_create — upload their three device images once
    if (h->kind == ELPH_MODEL_HOLSTEIN && K.hop_uploaded) return ELPH_OK;
    const int hch = K.hop_per_chain() ? nch : 1;
    if (nb > 0 && h->kind == ELPH_MODEL_HOLSTEIN) {
        HIPCHK(hipMemcpy(K.d_cbar, K.h_cbar.data(), sizeof(double) * nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_sbar, K.h_sbar.data(), sizeof(double) * nb, hipMemcpyHostToDevice));
    }
    if (h->fast_capable) {
        const size_t per = (size_t)h->lp_ne * ELPH_WAVE;
        std::vector<double> lc((size_t)hch * per), ls((size_t)hch * per);
        for (int c = 0; c < hch; ++c) {
            elph_lp_pack(h, K.h_cbar.data() + c * nb, lc.data() + c * per, 1.0);
            elph_lp_pack(h, K.h_sbar.data() + c * nb, ls.data() + c * per, 0.0);
        }
        HIPCHK(hipMemcpy(K.d_lp_cbar, lc.data(), sizeof(double) * lc.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_lp_sbar, ls.data(), sizeof(double) * ls.size(), hipMemcpyHostToDevice));
    }
    if (h->shape.sq_L() > 0) {
        const size_t per = 4 * N;
        std::vector<double> qc((size_t)hch * per), qs((size_t)hch * per);
        bool uni = true;
        for (int c = 0; c < hch; ++c) {
            double *q0 = qc.data() + c * per, *q1 = qs.data() + c * per;
            for (size_t k = 0; k < per; ++k) { q0[k] = K.h_cbar[c * nb + h->shape.bond[k]]; q1[k] = K.h_sbar[c * nb + h->shape.bond[k]]; }
            for (size_t k = 1; k < per; ++k) uni = uni && q0[k] == q0[0] && q1[k] == q1[0];       // uniform within the chain
        }
        K.sq_chain_uniform = uni;
        HIPCHK(hipMemcpy(K.d_sq_cbar, qc.data(), sizeof(double) * qc.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_sq_sbar, qs.data(), sizeof(double) * qs.size(), hipMemcpyHostToDevice));
    }
    K.hop_uniform = nb > 0 && !K.hop_per_chain();      // (read by the honeycomb and patch-layout forms only)
    for (size_t k = 1; k < nb && K.hop_uniform; ++k) K.hop_uniform = K.h_cbar[k] == K.h_cbar[0] && K.h_sbar[k] == K.h_sbar[0];
    K.hop_uploaded = true;
    return ELPH_OK;
}

// The Arnoldi bounds of every chain the caller does not skip, on the device (kpm_dev.hip: all chains in one launch; eb[2c] = e_min and
// eb[2c+1] = e_max).  ELPH_E_UNSUPPORTED where the kernel refuses the shape: eb is untouched and the caller takes the host path.
static int kpm_bounds_device(elph_handle_s *h, const double *b_max, const double *b_min, const std::vector<char> &skip, std::vector<double> &eb) {
    KpmState &K = h->kpm;
    const int N = (int)h->N, nch = K.nch();
    const size_t nst = (size_t)2 * nch * N;
    if (!K.d_start) RC(dev_alloc(&K.d_start, (size_t)K.tab_cap * (2 * N + 2)));
    HIPCHK(hipMemcpyAsync(K.d_start, b_max, sizeof(double) * (size_t)nch * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(K.d_start + (size_t)nch * N, b_min, sizeof(double) * (size_t)nch * N, hipMemcpyHostToDevice, h->stream));
    RC(elph_kpm_bounds_dev(h, nch, K.d_start, K.d_start + nst));
    std::vector<double> dev((size_t)2 * nch);
    HIPCHK(hipMemcpyAsync(dev.data(), K.d_start + nst, sizeof(double) * 2 * (size_t)nch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nch; ++c)
        if (!skip[(size_t)c]) { eb[2 * (size_t)c] = dev[2 * (size_t)c]; eb[2 * (size_t)c + 1] = dev[2 * (size_t)c + 1]; }
    return ELPH_OK;
}

// The same on the host (kpm_host.cpp), chain by chain: needs Ē (and the averaged hoppings) on the host
static int kpm_bounds_host(elph_handle_s *h, const double *b_max, const double *b_min, const std::vector<char> &skip, std::vector<double> &eb) {
    KpmState &K = h->kpm;
    const int N = (int)h->N, nch = K.nch();
    HIPCHK(hipMemcpy(K.h_Ebar.data(), K.d_Ebar, sizeof(double) * (size_t)nch * N, hipMemcpyDeviceToHost));
    for (int c = 0; c < nch; ++c)
        if (!skip[(size_t)c]) (void)elph_kpm_arnoldi(h, c, b_max + (size_t)c * N, b_min + (size_t)c * N, &eb[2 * (size_t)c], &eb[2 * (size_t)c + 1]);
    return ELPH_OK;
}

// Whether setup!(P) asks the device for its bounds: three chains and more on a lattice of one wave, or as ELPH_KPM_HOST / ELPH_KPM_DEVICE pin it
// (one or two chains: the host's scalar Arnoldi + LAPACK-style QR, 0.1 ms per chain, beats a kernel whose one wave spends
//  ~0.25 ms on the same sequential work; from three chains on all of them run side by side on the device)
static bool kpm_bounds_on_device(const elph_handle_s *h) {
    const char *eh = getenv("ELPH_KPM_HOST"), *ed = getenv("ELPH_KPM_DEVICE");     // read per call: tests pin one path
    const bool host_only = eh && eh[0] == '1', dev_always = ed && ed[0] == '1';
    return !host_only && h->N <= 512 && (h->kpm.nch() >= 3 || dev_always);
}

// The Arnoldi bounds of the chains not skipped, on the device when the caller asks for it and the kernel takes the shape, else on the host;
// *ran_on_device says which
static int kpm_bounds_arnoldi(elph_handle_s *h, bool device, const double *b_max, const double *b_min, const std::vector<char> &skip,
                              std::vector<double> &eb, int *ran_on_device) {
    if (ran_on_device) *ran_on_device = 0;
    if (device) {
        const int rcd = kpm_bounds_device(h, b_max, b_min, skip, eb);
        if (rcd == ELPH_OK && ran_on_device) *ran_on_device = 1;
        if (rcd != ELPH_E_UNSUPPORTED) return rcd;
    }
    return kpm_bounds_host(h, b_max, b_min, skip, eb);
}

// The eigenvalue bounds of every chain (:272-273), eb[2c] = e_min and eb[2c+1] = e_max: injected, or the Arnoldi process with the caller's
// start vectors — on the device for all chains at once (kpm_dev.hip: one wavefront per chain and per operator, Ritz values by a
// wave-parallel Hessenberg QR), on the host for lattices beyond one wave
static int kpm_bounds(elph_handle_s *h, const double *b_max, const double *b_min, const double *e_min, const double *e_max,
                      std::vector<double> &eb) {
    const int nch = h->kpm.nch();
    std::vector<char> injected((size_t)nch, 0);
    eb.assign((size_t)2 * nch, NAN);
    bool need_arnoldi = false;
    for (int c = 0; c < nch; ++c) {
        injected[(size_t)c] = e_min && e_max && std::isfinite(e_min[c]) && std::isfinite(e_max[c]);
        if (injected[(size_t)c]) { eb[2 * (size_t)c] = e_min[c]; eb[2 * (size_t)c + 1] = e_max[c]; } else need_arnoldi = true;
    }
    if (!need_arnoldi) return ELPH_OK;
    if (!(b_max && b_min)) { elph_set_error("Arnoldi start vectors required when bounds are not injected"); return ELPH_E_ARG; }
    return kpm_bounds_arnoldi(h, kpm_bounds_on_device(h), b_max, b_min, injected, eb, nullptr);
}

// the device copies of the tables
static int kpm_upload(elph_handle_s *h) {
    KpmState &K = h->kpm;
    const KpmTables &T = K.tab;
    const size_t ncoeff = T.coeff.size() / 2;
    if (ncoeff > K.coeff_cap) {
        RC(dev_alloc(&K.d_coeff, ncoeff));
        K.coeff_cap = ncoeff;
    }
    HIPCHK(hipMemcpy(K.d_coeff, T.coeff.data(), ncoeff * sizeof(double2), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_order, T.order.data(), sizeof(int) * T.order.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_coff, T.coff.data(), sizeof(int) * T.coff.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_wsched, T.wsched.data(), sizeof(int) * T.wsched.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_desc, T.desc.data(), sizeof(KpmDesc) * T.desc.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_fold, T.fold.data(), sizeof(double) * T.fold.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_lam, T.lam.data(), sizeof(double) * T.lam.size(), hipMemcpyHostToDevice));
    return ELPH_OK;
}

// setup!(P) for every chain resident in the handle (h->nchains of them).  All arrays are per chain.
static int kpm_setup_core(elph_handle_s *h, const KpmSource &src, const double *b_max, const double *b_min, const double *e_min,
                          const double *e_max, int *active, double *lam_lo, double *lam_hi) {
    KpmState &K = h->kpm;
    if (!K.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    if (!src.Ebar) RC(need_model(h));      // (an injected Ē is all the expansion needs: that handle never multiplies by M)
    HIPCHK(hipStreamSynchronize(h->stream));
    RC(kpm_reserve(h, h->nchains));
    RC(kpm_update_A(h, src));
    std::vector<double> eb;
    RC(kpm_bounds(h, b_max, b_min, e_min, e_max, eb));
    if (elph_kpm_plan(K, (int)h->L, eb.data())) RC(kpm_upload(h));
    K.ready = true;
    for (int c = 0; c < K.nch(); ++c) {
        if (active) active[c] = K.chains[(size_t)c].active;
        if (lam_lo) lam_lo[c] = K.chains[(size_t)c].lam_lo;
        if (lam_hi) lam_hi[c] = K.chains[(size_t)c].lam_hi;
    }
    return ELPH_OK;
}

// elph_bench.h: the bounds as kpm_bounds' two branches compute them, with nothing of setup!(P) after them
extern "C" int elph_bench_kpm_bounds(elph_handle h, int where, const double *b_max, const double *b_min, double *e_out, int *ran_on_device) {
    CHECK_H(h);
    KpmState &K = h->kpm;
    if (!K.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    if (!b_max || !b_min || !e_out || where < 0 || where > 2) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(need_model(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    RC(kpm_reserve(h, h->nchains));
    RC(kpm_update_A(h, KpmSource()));
    const std::vector<char> none((size_t)K.nch(), 0);
    std::vector<double> eb((size_t)2 * K.nch(), NAN);
    RC(kpm_bounds_arnoldi(h, where == 1 || (where == 2 && kpm_bounds_on_device(h)), b_max, b_min, none, eb, ran_on_device));
    std::copy(eb.begin(), eb.end(), e_out);
    return ELPH_OK;
}

// setup!(P) of a Holstein handle whose τ-averaged exp(−ΔτV) comes from OUTSIDE (KpmSource).  One chain.
int elph_i_kpm_setup_ebar(elph_handle_s *h, const double *Ebar_host, const double *b_max, const double *b_min) {
    if (h->kind != ELPH_MODEL_HOLSTEIN || !h->kpm.created) { elph_set_error("Ē injection: a Holstein handle with elph_kpm_create done"); return ELPH_E_STATE; }
    set_nchains(h, 1);
    return kpm_setup_core(h, KpmSource{Ebar_host, nullptr, nullptr}, b_max, b_min, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// setup!(P) of a bond-phonon handle whose τ-averaged hopping tables come from OUTSIDE (KpmSource); exp(Δτμ) is the handle's own
// (elph_update_model_ssh once; μ does not move).  One chain.
int elph_i_kpm_setup_csbar(elph_handle_s *h, const double *cbar_host, const double *sbar_host, const double *b_max, const double *b_min) {
    if (h->kind != ELPH_MODEL_SSH || !h->kpm.created || !h->have_E) {
        elph_set_error("c̄ / s̄ injection: a bond-phonon handle with elph_kpm_create and one elph_update_model_ssh done");
        return ELPH_E_STATE;
    }
    set_nchains(h, 1);
    return kpm_setup_core(h, KpmSource{nullptr, cbar_host, sbar_host}, b_max, b_min, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int elph_kpm_setup(elph_handle h, const double *b_max, const double *b_min, double e_min, double e_max,
                              int *active, double *lam_lo, double *lam_hi) {
    CHECK_H(h);
    if (h->nchains != 1) { elph_set_error("%d phonon configurations are resident: use elph_kpm_setup_chains", h->nchains); return ELPH_E_STATE; }
    return kpm_setup_core(h, KpmSource(), b_max, b_min, &e_min, &e_max, active, lam_lo, lam_hi);
}

extern "C" int elph_kpm_setup_chains(elph_handle h, const double *b_max, const double *b_min, const double *e_min,
                                     const double *e_max, int *active, double *lam_lo, double *lam_hi) {
    CHECK_H(h);
    return kpm_setup_core(h, KpmSource(), b_max, b_min, e_min, e_max, active, lam_lo, lam_hi);
}

extern "C" int elph_kpm_orders(elph_handle h, int64_t *orders, int64_t *total) {
    CHECK_H(h);
    if (!h->kpm.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    const int Lo2 = (int)((h->L + 1) / 2);
    int64_t tot = 0;
    for (int w = 0; w < Lo2; ++w) {
        const int o = h->kpm.chains.empty() ? 1 : h->kpm.chains[0].order[w];
        if (orders) orders[w] = o;
        tot += o;
    }
    if (total) *total = tot;
    return ELPH_OK;
}

extern "C" int elph_kpm_apply_dev(elph_handle h, double *z_dev, const double *r_dev) {
    CHECK_H(h);
    if (!h->kpm.ready) { elph_set_error("elph_kpm_setup has not been called"); return ELPH_E_STATE; }
    if (!z_dev || !r_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_launch_r2s(h, h->work.r, r_dev, 1));
    RC(elph_launch_kpm_apply(h, h->work.zp, h->work.r, 1, 0));
    RC(elph_launch_s2r(h, z_dev, h->work.zp, 1));
    return ELPH_OK;
}

extern "C" int elph_kpm_apply(elph_handle h, double *z, const double *r) {
    CHECK_H(h);
    if (!z || !r) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t bytes = (size_t)h->ndim * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, r, bytes, hipMemcpyHostToDevice, h->stream));
    RC(elph_kpm_apply_dev(h, h->work.stage_out, h->work.stage_in));
    HIPCHK(hipMemcpyAsync(z, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}
