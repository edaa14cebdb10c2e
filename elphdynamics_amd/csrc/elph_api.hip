// elph_api.hip — what every caller of libelphgpu.so (include/elph_gpu.h) needs first: errors and the build record, the handle's life cycle,
// the solve workspace, the update_model! and mul! families, the tau-transform entry points.  (The solves: cg_solve.hip; forces and muldMdx!:
// force.hip; the preconditioner: kpm_setup.hip; the measurement hooks: bench_hooks.hip; the device-free half of elph_create: lattice_shape.cpp.)
// Host orchestration only: argument checks and layout staging.  All arithmetic on lattice vectors happens in kernels.hip.
// There is NO CPU fallback: without a gfx950 device every compute entry point fails.

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "elph_internal.h"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------

static thread_local char g_err[512] = "";

void elph_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int elph_launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { elph_set_error("launch %s failed: %s", what, hipGetErrorString(e)); return ELPH_E_HIP; }
    return ELPH_OK;
}

extern "C" const char *elph_last_error(void) { return g_err; }
extern "C" int elph_abi_version(void) { return ELPH_ABI_VERSION; }
// the build record: written by elphdynamics_amd/build.py into a translation unit of its own at every link
extern "C" const char elph_build_info_text[];
extern "C" const char *elph_build_info(void) { return elph_build_info_text; }

extern "C" int elph_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the number of phonon configurations resident in the handle; the KPM expansion is per chain, so a change invalidates it
void set_nchains(elph_handle_s *h, int n) {
    if (h->nchains != n) { h->nchains = n; h->kpm.ready = false; }
}

int need_model(elph_handle_s *h) {
    if (!h->have_E) { elph_set_error("update_model has not been called on this handle"); return ELPH_E_STATE; }
    return ELPH_OK;
}

// the device half of the lane program (cg_fast.hip) that elph_i_host_handle planned
static int build_lane_program(elph_handle_s *h) {
    const int NE = h->lp_ne;
    RC(dev_alloc(&h->d_lp_ij, (size_t)NE * ELPH_WAVE));
    HIPCHK(hipMemcpy(h->d_lp_ij, h->h_lp_ij.data(), sizeof(unsigned) * NE * ELPH_WAVE, hipMemcpyHostToDevice));
    const size_t ntau = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1;
    RC(dev_alloc(&h->d_lp_c, ntau * NE * ELPH_WAVE));
    RC(dev_alloc(&h->d_lp_s, ntau * NE * ELPH_WAVE));
    if (h->shape.sq_L() > 0) {
        RC(dev_alloc(&h->d_sq_bond, (size_t)4 * h->N));
        HIPCHK(hipMemcpy(h->d_sq_bond, h->shape.bond.data(), sizeof(int) * 4 * h->N, hipMemcpyHostToDevice));
    }
    if (h->shape.kind == LatticeShape::SQUARE && h->shape.patch()) {      // the site -> bond map of the colouring: hopping disorder in the patch layout (pgrid.hip)
        RC(dev_alloc(&h->d_pg_bond, (size_t)4 * h->N));
        HIPCHK(hipMemcpy(h->d_pg_bond, h->shape.bond.data(), sizeof(int) * 4 * h->N, hipMemcpyHostToDevice));
    }
    return ELPH_OK;
}

// uploads the lane-program copy of the per-bond cosh/sinh tables (h_c/h_s)
static int upload_lp_cs(elph_handle_s *h) {
    if (!h->fast) return ELPH_OK;
    const int NE = h->lp_ne;
    const size_t ntau = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1, per = (size_t)NE * ELPH_WAVE;
    if (h->h_c.size() < ntau * (size_t)h->nb) return ELPH_OK;   // SSH before the first update_model
    std::vector<double> c(ntau * per), s(ntau * per);
    for (size_t t = 0; t < ntau; ++t) {
        elph_lp_pack(h, h->h_c.data() + t * (size_t)h->nb, c.data() + t * per, 1.0);
        elph_lp_pack(h, h->h_s.data() + t * (size_t)h->nb, s.data() + t * per, 0.0);
    }
    HIPCHK(hipMemcpy(h->d_lp_c, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lp_s, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// life cycle
// ------------------------------------------------------------------------------------------

int elph_work_reserve(elph_handle_s *h, int nrhs) {
    SolveWork &W = h->work;
    if (nrhs <= W.cap_rhs) return ELPH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t Lo2 = (size_t)(h->L + 1) / 2, Lh = (size_t)h->L / 2 + 1, c = (size_t)nrhs;
    W.ndim = (size_t)h->ndim; W.nnu = Lo2 * (size_t)h->N; W.nrz = (size_t)h->L * (size_t)h->npl;
    for (double **v : {&W.stage_in, &W.stage_out, &W.b, &W.x, &W.r, &W.z, &W.zp, &W.tmp}) RC(dev_alloc(v, c * W.ndim));
    RC(dev_alloc(&W.p, 2 * c * W.ndim));
    RC(dev_alloc(&W.phi, 2 * W.ndim));
    RC(dev_alloc(&W.xfield, W.ndim));
    RC(dev_alloc(&W.sums, 4 * c * W.nrz));
    RC(dev_alloc(&W.state, 2 * c));
    RC(dev_alloc(&W.scal, 4 * c));
    RC(dev_alloc(&W.alpha, c));
    RC(dev_alloc(&W.nu, c * std::max(std::max(Lo2, Lh) * (size_t)h->N, W.ndim)));      // (the plain transforms' Lh frequencies fit too)
    if (W.h_state) HIPCHK(hipHostFree(W.h_state));
    if (W.h_scal) HIPCHK(hipHostFree(W.h_scal));
    HIPCHK(hipHostMalloc((void **)&W.h_state, 2 * c * sizeof(CgState), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&W.h_scal, 4 * c * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(W.sums, 0, 4 * c * W.nrz * sizeof(double), h->stream));
    W.cap_rhs = nrhs;
    return ELPH_OK;
}

void elph_work_release(elph_handle_s *h) {
    SolveWork &W = h->work;
    void *ptrs[] = {W.stage_in, W.stage_out, W.b, W.x, W.r, W.z, W.zp, W.tmp, W.p, W.nu, W.sums, W.state, W.alpha, W.scal, W.hist, W.phi, W.xfield};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (W.h_state) (void)hipHostFree(W.h_state);
    if (W.h_scal) (void)hipHostFree(W.h_scal);
    W = SolveWork();
}

// elements of a staged transfer; refuses one the staging buffers do not hold
static int staged_size(elph_handle_s *h, int nvec, int ncols, size_t *n) {
    *n = (size_t)nvec * (size_t)(ncols ? ncols : h->N) * (size_t)h->L;
    const size_t held = (size_t)h->work.cap_rhs * h->work.ndim;
    if (*n > held) { elph_set_error("staging %zu doubles, the staging buffers hold %zu", *n, held); return ELPH_E_STATE; }
    return ELPH_OK;
}

int elph_stage_in(elph_handle_s *h, double *dstS, const double *hostR, int nvec, int ncols) {
    size_t n = 0;
    RC(staged_size(h, nvec, ncols, &n));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, hostR, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return elph_launch_r2s(h, dstS, h->work.stage_in, nvec, ncols);
}

int elph_stage_out(elph_handle_s *h, double *hostR, const double *srcS, int nvec, int ncols) {
    size_t n = 0;
    RC(staged_size(h, nvec, ncols, &n));
    RC(elph_launch_s2r(h, h->work.stage_out, srcS, nvec, ncols));
    HIPCHK(hipMemcpyAsync(hostR, h->work.stage_out, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return ELPH_OK;
}

int elph_retry_in_slot0(elph_handle_s *h, int r, const std::function<int()> &solve_and_flag, double *x, double *b) {
    SolveWork W = h->work;
    if (x) W.x = x;
    if (b) W.b = b;
    const size_t bytes = W.ndim * sizeof(double);
    if (r != 0) {
        HIPCHK(hipMemcpyAsync(W.stage_out, W.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.stage_in, W.b, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.x, W.x + r * W.ndim, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.b, W.b + r * W.ndim, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    if (h->nchains > 1) h->solo_chain = r % h->nchains;   // slot 0 must keep rhs r's fermion matrix
    const int rc = solve_and_flag();
    h->solo_chain = -1;
    RC(rc);
    if (r != 0) {
        HIPCHK(hipMemcpyAsync(W.x + r * W.ndim, W.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.x, W.stage_out, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.b, W.stage_in, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return ELPH_OK;
}

void elph_fold_pair(int nch, const int64_t *it2, const int *fl2, int64_t *iters, int *flag) {
    for (int c = 0; c < nch; ++c) {
        int64_t tot = it2[c];
        int fl = fl2[c];
        if (fl == 0) { tot += it2[nch + c]; fl = fl2[nch + c]; }      // a failed first solve suppresses the second (:880)
        if (fl == 0) tot = (tot + 1) / 2;                             // cld(iters, 2)  (:907-909)
        iters[c] = tot;
        flag[c] = fl;
    }
}

void elph_fold_pair_stages(int nch, const int64_t *it4, const int *fl4, int64_t *iters, int *flag, int *zero_minus) {
    const size_t n2 = 2 * (size_t)nch;                                   // it4, fl4: [stage][sign][chain]
    std::vector<int64_t> it2(n2);
    std::vector<int> fl2(n2);
    for (size_t r = 0; r < n2; ++r) {
        it2[r] = it4[r] + it4[n2 + r];                                   // iters += iters′ of the second stage (:863, :871)
        fl2[r] = std::max(fl4[r], fl4[n2 + r]);                          // flag = max(flag, flag′) (:864, :872)
    }
    elph_fold_pair(nch, it2.data(), fl2.data(), iters, flag);
    if (zero_minus) for (int c = 0; c < nch; ++c) zero_minus[c] = fl2[c] != 0;
}

extern "C" int elph_create(elph_handle *out, int kind, int64_t nsites, int64_t ltau, int64_t nbonds,
                           const int64_t *neighbor_table, const double *cosht, const double *sinht, int device) {
    if (!out) { elph_set_error("out is null"); return ELPH_E_ARG; }
    *out = nullptr;
    if (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) { elph_set_error("bad model kind %d", kind); return ELPH_E_ARG; }
    if (nsites < 1 || ltau < 1 || nbonds < 0) { elph_set_error("bad sizes N=%lld L=%lld nb=%lld", (long long)nsites, (long long)ltau, (long long)nbonds); return ELPH_E_ARG; }
    if (nsites > (int64_t)ELPH_MAX_SITES) {
        elph_set_error("nsites=%lld exceeds the %d sites a one-workgroup-per-slice kernel supports", (long long)nsites, ELPH_MAX_SITES);
        return ELPH_E_UNSUPPORTED;
    }
    if (nsites * ltau > (int64_t)1 << 30) { elph_set_error("ndim too large"); return ELPH_E_UNSUPPORTED; }
    // (beyond 1024 slices the tau-transforms run as dft_big.hip's two-step form, whose launches carry the slice index in gridDim.y)
    if (ltau > 65535) { elph_set_error("ltau=%lld: the time axis is limited to 65535 slices (launch geometry of the long-axis transform)", (long long)ltau); return ELPH_E_UNSUPPORTED; }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { elph_set_error("no HIP device visible"); return ELPH_E_NOGPU; }
    if (device < 0 || device >= ndev) { elph_set_error("device %d not in 0..%d", device, ndev - 1); return ELPH_E_ARG; }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        elph_set_error("device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return ELPH_E_NOGPU;
    }

    elph_handle_s *h = new elph_handle_s();
    elph_i_host_handle(h, kind, nsites, ltau, nbonds, neighbor_table, cosht, sinht);
    h->device = device;
    h->maxiter = h->ndim;   // ConjugateGradient ctor default (IterativeSolvers.jl:49-51)

    int rc = ELPH_OK;
    auto fail = [&](int code) { elph_destroy(h); return code; };
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { elph_set_error("stream create failed"); return fail(ELPH_E_HIP); }
    h->own_stream = true;
    if ((rc = dev_alloc(&h->d_bi, (size_t)nbonds))) return fail(rc);
    if ((rc = dev_alloc(&h->d_bj, (size_t)nbonds))) return fail(rc);
    if ((rc = dev_alloc(&h->d_coloff, h->h_coloff.size()))) return fail(rc);
    const size_t ncs = (kind == ELPH_MODEL_SSH) ? (size_t)ltau * (size_t)nbonds : (size_t)nbonds;
    if ((rc = dev_alloc(&h->d_c, ncs))) return fail(rc);
    if ((rc = dev_alloc(&h->d_s, ncs))) return fail(rc);
    const size_t nE = (kind == ELPH_MODEL_SSH) ? (size_t)nsites : (size_t)h->ndim;
    if ((rc = dev_alloc(&h->d_E, nE))) return fail(rc);
    h->E_cap = (int64_t)nE;
    if ((rc = dev_alloc(&h->d_lam, 3 * (size_t)nsites))) return fail(rc);
    if (nbonds > 0) {
        if (hipMemcpy(h->d_bi, h->h_bi.data(), sizeof(int) * nbonds, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_bj, h->h_bj.data(), sizeof(int) * nbonds, hipMemcpyHostToDevice) != hipSuccess) {
            elph_set_error("table upload failed");
            return fail(ELPH_E_HIP);
        }
    }
    if (hipMemcpy(h->d_coloff, h->h_coloff.data(), sizeof(int) * h->h_coloff.size(), hipMemcpyHostToDevice) != hipSuccess) {
        elph_set_error("table upload failed");
        return fail(ELPH_E_HIP);
    }
    if (kind == ELPH_MODEL_HOLSTEIN && nbonds > 0) {
        if (hipMemcpy(h->d_c, cosht, sizeof(double) * nbonds, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_s, sinht, sizeof(double) * nbonds, hipMemcpyHostToDevice) != hipSuccess) {
            elph_set_error("cosh/sinh upload failed");
            return fail(ELPH_E_HIP);
        }
    }
    if ((rc = elph_dft_build_tables(h))) return fail(rc);
    if ((rc = build_lane_program(h))) return fail(rc);
    if ((rc = upload_lp_cs(h))) return fail(rc);
    if ((rc = elph_work_reserve(h, 1))) return fail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { elph_set_error("sync failed"); return fail(ELPH_E_HIP); }
    *out = h;
    return ELPH_OK;
}

extern "C" int elph_destroy(elph_handle h) {
    if (!h) return ELPH_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    elph_i_slabs_free(h);                             // (the slab handles of a large lattice: each is destroyed through here again)
    elph_shard_free(h);
    elph_hmc_free(h);
    elph_greens_free(h);
    elph_msolve_free(h);
    elph_dft_free(h);
    elph_kpm_free(h);
    elph_work_release(h);
    void *ptrs[] = {h->d_bi, h->d_bj, h->d_coloff, h->d_c, h->d_s, h->d_E, h->d_lam, h->d_ssh_x, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_bar,
                    h->d_ssh_cb, h->d_ssh_slot, h->d_diag, h->d_lp_ij, h->d_lp_c, h->d_lp_s, h->d_sq_bond, h->d_pg_bond, h->res.d_res, h->d_mu_ch};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    for (int k = 1; k < ELPH_SPLIT_PARTS; ++k)
        if (h->split_stream[k]) (void)hipStreamDestroy(h->split_stream[k]);
    if (h->split_ev) (void)hipEventDestroy(h->split_ev);
    delete h;
    return ELPH_OK;
}

extern "C" int elph_set_stream(elph_handle h, void *hip_stream) {
    CHECK_H(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hip_stream) {
        if (h->own_stream) { HIPCHK(hipStreamDestroy(h->stream)); h->own_stream = false; }
        h->stream = (hipStream_t)hip_stream;
    } else if (!h->own_stream) {
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return ELPH_OK;
}

extern "C" int elph_synchronize(elph_handle h) {
    CHECK_H(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// update_model!
// ------------------------------------------------------------------------------------------

// the site parameters of a Holstein model -> d_lam = [lambda | lambda2 | mu] (mu may be null: muldMdx! does not read it), stream-ordered
int elph_i_holstein_upload_params(elph_handle_s *h, const double *lambda, const double *lambda2, const double *mu) {
    const size_t N = (size_t)h->N;
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (mu) HIPCHK(hipMemcpyAsync(h->d_lam + 2 * N, mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return ELPH_OK;
}

// reference: (Ltau x Nbonds) column-major = [bond][tau]; device: tau-major [tau][bond]
void elph_bt_to_tb(double *tb, const double *bt, size_t L, size_t nb) {
    for (size_t n = 0; n < nb; ++n)
        for (size_t t = 0; t < L; ++t) tb[t * nb + n] = bt[n * L + t];
}
void elph_tb_to_bt(double *bt, const double *tb, size_t L, size_t nb) {
    for (size_t n = 0; n < nb; ++n)
        for (size_t t = 0; t < L; ++t) bt[n * L + t] = tb[t * nb + n];
}

// idle lane-program slots: the identity bond (cosh, sinh) = (1, 0) on every slice of the first nch chains' tables (blocking copies: the
// handle's stream does not wait for the null stream, so nothing is left in flight there)
static int lp_identity_fill(elph_handle_s *h, size_t nch) {
    const size_t n = nch * (size_t)h->L * (size_t)h->lp_ne * ELPH_WAVE;
    std::vector<double> one(n, 1.0), zero(n, 0.0);
    HIPCHK(hipMemcpy(h->d_lp_c, one.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lp_s, zero.data(), n * sizeof(double), hipMemcpyHostToDevice));
    return ELPH_OK;
}

extern "C" int elph_update_model_holstein(elph_handle h, const double *x, const double *lambda, const double *lambda2,
                                          const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!x || !lambda || !lambda2 || !mu) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_i_holstein_upload_params(h, lambda, lambda2, mu));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, x, (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    set_nchains(h, 1);   // expansions were per chain
    RC(elph_launch_expV(h, h->work.stage_in, dtau));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    return ELPH_OK;
}

// several independent phonon configurations (chains) resident at once: right-hand side r of a batched solve
// uses chain r % nchains.  X: nchains * ndim (reference layout, chain-major).
extern "C" int elph_update_model_holstein_chains(elph_handle h, int nchains, const double *X, const double *lambda,
                                                 const double *lambda2, const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (nchains < 1 || !X || !lambda || !lambda2 || !mu) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const size_t nd = (size_t)h->ndim;
    RC(elph_i_reserve_chains(h, nchains));
    RC(elph_i_holstein_upload_params(h, lambda, lambda2, mu));
    // all configurations in one transfer (the staging buffer holds cap_rhs vectors), one exp kernel per chain, one sync
    RC(elph_work_reserve(h, nchains));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, X, (size_t)nchains * nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int c = 0; c < nchains; ++c) RC(elph_launch_expV(h, h->work.stage_in + (size_t)c * nd, dtau, c));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    h->kpm.ready = false;   // the preconditioner belongs to ONE configuration
    return ELPH_OK;
}

extern "C" int elph_set_expV(elph_handle h, const double *expnDtauV) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!expnDtauV) { elph_set_error("null argument"); return ELPH_E_ARG; }
    HIPCHK(hipMemcpyAsync(h->work.stage_in, expnDtauV, (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    set_nchains(h, 1);   // expansions were per chain
    RC(elph_launch_r2s(h, h->d_E, h->work.stage_in, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    return ELPH_OK;
}

extern "C" int elph_update_model_ssh(elph_handle h, const double *cosht, const double *sinht, const double *expDtauMu) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (!expDtauMu || (h->nb > 0 && (!cosht || !sinht))) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t L = (size_t)h->L, nb = (size_t)h->nb;
    h->h_c.resize(L * nb); h->h_s.resize(L * nb);
    elph_bt_to_tb(h->h_c.data(), cosht, L, nb);
    elph_bt_to_tb(h->h_s.data(), sinht, L, nb);
    if (nb > 0) {
        HIPCHK(hipMemcpy(h->d_c, h->h_c.data(), L * nb * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_s, h->h_s.data(), L * nb * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(h->d_E, expDtauMu, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice));
    RC(upload_lp_cs(h));
    h->mu_per_chain = false;
    set_nchains(h, 1);      // host tables describe ONE configuration
    h->cs_host_stale = false;
    h->have_E = true;
    return ELPH_OK;
}

// update_model!(ssh) computed ON THE DEVICE from the phonon fields (SSHModels.jl:510-562): no cosh/sinh on the host, no
// (Ltau x Nbonds) tables over PCIe.
//   x          double[nph * ltau]   ssh.x, field = (phonon-1) Ltau + tau
//   cb_index   int64[nph]           1-based checkerboard position of each phonon's bond = checkerboard_perm[phonon_to_bond[p]]
//   t_ph, alpha, alpha2  double[nph] bare hopping of that bond (ssh.t[bond]) and the couplings
//   t_bare_cb  double[nbonds]       bare hopping of EVERY bond in checkerboard order (bonds without a phonon keep it)
//   mu         double[nsites]
// A bond is driven by at most one field per tau (equivalent fields carry equal x, :548-558).
// per-phonon tables, bare hoppings, lane-program slot map and mu of an SSH handle -> device (d_ssh_*, d_lam)
int elph_i_ssh_upload_params(elph_handle_s *h, int64_t nph, const int64_t *cb_index, const double *t_ph, const double *alpha,
                             const double *alpha2, const double *t_bare_cb, const double *mu) {
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (nph < 0 || !mu || (h->nb > 0 && !t_bare_cb) || (nph > 0 && (!cb_index || !t_ph || !alpha || !alpha2))) {
        elph_set_error("null argument");
        return ELPH_E_ARG;
    }
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, np = (size_t)nph;
    std::vector<int> cb0(np);
    for (size_t p = 0; p < np; ++p) {
        if (cb_index[p] < 1 || cb_index[p] > (int64_t)nb) { elph_set_error("cb_index[%zu] = %lld outside 1..%zu", p, (long long)cb_index[p], nb); return ELPH_E_ARG; }
        cb0[p] = (int)(cb_index[p] - 1);
    }
    if (!h->d_ssh_slot) {     // once: lane-program slot of each checkerboard bond (the layout of elph_lp_pack)
        std::vector<int> slot(std::max<size_t>(nb, 1), -1);
        if (h->fast_capable) {
            const int PP = (h->npl + 1) / 2;
            for (int col = 0; col < h->ncol && col < h->lp_mc; ++col)
                for (int n = h->h_coloff[col]; n < h->h_coloff[col + 1]; ++n) {
                    const int k = n - h->h_coloff[col];
                    slot[(size_t)n] = (col * PP + k / ELPH_WAVE) * ELPH_WAVE + (k % ELPH_WAVE);
                }
            RC(lp_identity_fill(h, 1));
        }
        RC(dev_alloc(&h->d_ssh_slot, slot.size()));
        HIPCHK(hipMemcpy(h->d_ssh_slot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
        RC(dev_alloc(&h->d_ssh_tbare, std::max<size_t>(nb, 1)));
    }
    if ((int64_t)np > h->ssh_nph_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        RC(dev_alloc(&h->d_ssh_x, std::max<size_t>((size_t)h->ssh_chain_cap * np * L, 1)));
        RC(dev_alloc(&h->d_ssh_par, std::max<size_t>(3 * np, 1)));
        RC(dev_alloc(&h->d_ssh_cb, std::max<size_t>(np, 1)));
        h->ssh_nph_cap = (int64_t)np;
    }
    if (np > 0) {
        HIPCHK(hipMemcpyAsync(h->d_ssh_par, t_ph, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_par + np, alpha, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_par + 2 * np, alpha2, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_cb, cb0.data(), np * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    if (nb > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_tbare, t_bare_cb, nb * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam, mu, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // cb0 / the caller's arrays may go away
    h->ssh_nph = (int)np;
    return ELPH_OK;
}

extern "C" int elph_update_model_ssh_fields(elph_handle h, const double *x, int64_t nph, const int64_t *cb_index, const double *t_ph,
                                            const double *alpha, const double *alpha2, const double *t_bare_cb, const double *mu,
                                            double dtau) {
    CHECK_H(h);
    if (nph > 0 && !x) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_i_ssh_upload_params(h, nph, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu));
    h->mu_per_chain = false;
    set_nchains(h, 1);
    const size_t np = (size_t)nph;
    if (np > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_x, x, np * (size_t)h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_ssh_update(h, h->d_ssh_x, (int)np, h->d_ssh_cb, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_slot, dtau));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ssh_dtau = dtau;
    h->cs_host_stale = true;
    h->have_E = true;
    return ELPH_OK;
}

// Several independent phonon configurations (chains) of one SSH deck in one handle: X[nchains][nph*ltau]; in a batched call
// right-hand side r then uses the hopping tables of chain r % nchains (exp(dtau mu) and the couplings are the deck's, shared).
extern "C" int elph_update_model_ssh_fields_chains(elph_handle h, int nchains, const double *X, int64_t nph, const int64_t *cb_index,
                                                   const double *t_ph, const double *alpha, const double *alpha2,
                                                   const double *t_bare_cb, const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (nchains < 1 || (nph > 0 && !X)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_i_reserve_chains(h, nchains));
    RC(elph_i_ssh_upload_params(h, nph, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu));
    const size_t np = (size_t)nph;
    if (np > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_x, X, (size_t)nchains * np * (size_t)h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_ssh_update(h, h->d_ssh_x, (int)np, h->d_ssh_cb, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_slot, dtau, 0, nchains));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ssh_dtau = dtau;
    h->cs_host_stale = true;
    h->have_E = true;
    h->kpm.ready = false;
    return ELPH_OK;
}

// model.cosht / model.sinht as the reference stores them, (Ltau x Nbonds) column-major = [bond][tau] — for callers that
// reach into those fields (KPMPreconditioners.jl:362-378) after a device-side update
extern "C" int elph_get_cosh_sinh(elph_handle h, double *cosht, double *sinht) {
    CHECK_H(h);
    if (!cosht || !sinht) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t L = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1, nb = (size_t)h->nb;
    std::vector<double> c(L * nb), s(L * nb);
    if (nb > 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(c.data(), h->d_c, c.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(s.data(), h->d_s, s.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    elph_tb_to_bt(cosht, c.data(), L, nb);
    elph_tb_to_bt(sinht, s.data(), L, nb);
    return ELPH_OK;
}

// SSH: one set of hopping tables (tau-major cosh/sinh + their lane-program copies) and one field buffer per chain
static int ssh_reserve_chains(elph_handle_s *h, int nchains) {
    if (nchains <= h->ssh_chain_cap) return ELPH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, per = (size_t)h->lp_ne * ELPH_WAVE, nc = (size_t)nchains;
    RC(dev_alloc(&h->d_c, nc * L * nb));
    RC(dev_alloc(&h->d_s, nc * L * nb));
    if (h->fast_capable) {
        RC(dev_alloc(&h->d_lp_c, nc * L * per));
        RC(dev_alloc(&h->d_lp_s, nc * L * per));
        RC(lp_identity_fill(h, nc));
    }
    if (h->ssh_nph_cap > 0) RC(dev_alloc(&h->d_ssh_x, nc * (size_t)h->ssh_nph_cap * L));
    RC(dev_alloc(&h->d_E, nc * (size_t)h->N));          // exp(dtau mu) per chain
    h->E_cap = (int64_t)(nc * (size_t)h->N);
    h->ssh_chain_cap = nchains;
    h->have_E = false;          // the tables are empty until the next update_model!
    h->cs_host_stale = true;
    return ELPH_OK;
}

int elph_i_reserve_chains(elph_handle_s *h, int nchains) {
    if (nchains < 1) { elph_set_error("nchains < 1"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->kind == ELPH_MODEL_SSH) {
        RC(ssh_reserve_chains(h, nchains));
        set_nchains(h, nchains);
        return ELPH_OK;
    }
    const int64_t need = (int64_t)nchains * h->ndim;
    if (need > h->E_cap) {
        RC(dev_alloc(&h->d_E, (size_t)need));
        h->E_cap = need;
        h->have_E = false;
    }
    set_nchains(h, nchains);
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// mul! family
// ------------------------------------------------------------------------------------------

static int mul_dev(elph_handle_s *h, int which, double *y_dev, const double *v_dev) {
    RC(need_model(h));
    if (!y_dev || !v_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_launch_r2s(h, h->work.b, v_dev, 1));
    if (which == 3) {                                    // M Mᵀ v (Models.jl:229-238): two launches, not on the CG path
        RC(elph_launch_mul(h, 1, h->work.tmp, h->work.b, 1));
        RC(elph_launch_mul(h, 0, h->work.x, h->work.tmp, 1));
    } else {
        RC(elph_launch_mul(h, which, h->work.x, h->work.b, 1));
    }
    RC(elph_launch_s2r(h, y_dev, h->work.x, 1));
    return ELPH_OK;
}

static int mul_host(elph_handle_s *h, int which, double *y, const double *v) {
    if (!y || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t bytes = (size_t)h->ndim * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, v, bytes, hipMemcpyHostToDevice, h->stream));
    RC(mul_dev(h, which, h->work.stage_out, h->work.stage_in));
    HIPCHK(hipMemcpyAsync(y, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_mulM(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 0, y, v); }
extern "C" int elph_mulMT(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 1, y, v); }
extern "C" int elph_mulMTM(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 2, y, v); }
extern "C" int elph_mulMMT(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 3, y, v); }
extern "C" int elph_mulM_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 0, y, v); }
extern "C" int elph_mulMT_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 1, y, v); }
extern "C" int elph_mulMTM_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 2, y, v); }

// the defaults of the handle's solves (model.solver; the driver is cg_solve.hip)
extern "C" int elph_solver_set(elph_handle h, double tol, int64_t maxiter, double kappa_max) {
    CHECK_H(h);
    if (!(tol > 0.0) || maxiter < 0 || !(kappa_max > 0.0)) { elph_set_error("bad solver parameters"); return ELPH_E_ARG; }
    h->tol = tol;
    h->maxiter = (maxiter < 1) ? h->ndim : maxiter;   // IterativeSolvers.jl:49-51
    h->kmax = kappa_max;
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// Fourier acceleration / twisted FFT
// ------------------------------------------------------------------------------------------

extern "C" int elph_fourier_accelerate(elph_handle h, double *vout, const double *vin, const double *diag, double power,
                                       int64_t nph) {
    CHECK_H(h);
    if (!vout || !vin || !diag || nph < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const int64_t L = h->L, n = nph * L;
    // scratch: 3 real vectors of n + complex half spectrum; grown on demand (nph may exceed nsites for SSH)
    const int64_t need = 3 * n + 2 * (L / 2 + 1) * nph;
    if (need > h->diag_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        RC(dev_alloc(&h->d_diag, (size_t)need));
        h->diag_cap = need;
    }
    double *dR = h->d_diag, *aS = h->d_diag + n, *bS = h->d_diag + 2 * n;
    double2 *u = reinterpret_cast<double2 *>(h->d_diag + 3 * n);
    // stage (layout R -> S for "nph" columns), transform with the handle's tables, stage back
    HIPCHK(hipMemcpyAsync(dR, diag, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, bS, dR, 1, (int)nph));          // bS = diag in layout S  (diag[k][s])
    HIPCHK(hipMemcpyAsync(dR, vin, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, aS, dR, 1, (int)nph));          // aS = v in layout S
    RC(elph_dft_accel(h, dR, aS, bS, power, (int)nph, u, 1));   // dR = result in layout S
    RC(elph_launch_s2r(h, aS, dR, 1, (int)nph));          // aS = result in layout R
    HIPCHK(hipMemcpyAsync(vout, aS, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_tau_to_omega(elph_handle h, double *nu_complex, const double *v) {
    CHECK_H(h);
    if (!nu_complex || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t nd = (size_t)h->ndim;
    RC(elph_work_reserve(h, 2));   // complex scratch = 2 real vectors
    RC(elph_stage_in(h, h->work.b, v, 1));
    double2 *fullS = reinterpret_cast<double2 *>(h->work.p);           // [L][N] complex
    RC(elph_launch_tau_to_omega(h, fullS, h->work.b));
    // complex layout S -> complex layout R: transpose re and im planes separately via a strided copy
    // (API convenience path; the solver itself never leaves layout S)
    std::vector<double> tmp(2 * nd);
    HIPCHK(hipMemcpyAsync(tmp.data(), fullS, 2 * nd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->N, L = (size_t)h->L;
    for (size_t k = 0; k < L; ++k)
        for (size_t s = 0; s < N; ++s) {
            nu_complex[2 * (s * L + k)] = tmp[2 * (k * N + s)];
            nu_complex[2 * (s * L + k) + 1] = tmp[2 * (k * N + s) + 1];
        }
    return ELPH_OK;
}

extern "C" int elph_omega_to_tau(elph_handle h, double *v, const double *nu_complex) {
    CHECK_H(h);
    if (!nu_complex || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t nd = (size_t)h->ndim, N = (size_t)h->N, L = (size_t)h->L;
    RC(elph_work_reserve(h, 2));
    std::vector<double> tmp(2 * nd);
    for (size_t k = 0; k < L; ++k)
        for (size_t s = 0; s < N; ++s) {
            tmp[2 * (k * N + s)] = nu_complex[2 * (s * L + k)];
            tmp[2 * (k * N + s) + 1] = nu_complex[2 * (s * L + k) + 1];
        }
    double2 *fullS = reinterpret_cast<double2 *>(h->work.p);
    HIPCHK(hipMemcpy(fullS, tmp.data(), 2 * nd * sizeof(double), hipMemcpyHostToDevice));
    RC(elph_launch_omega_to_tau(h, h->work.x, fullS));
    RC(elph_stage_out(h, v, h->work.x, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}
