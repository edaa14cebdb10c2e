// bench_hooks.hip — the measurement hooks of elph_bench.h: the timed units bench.py measures, the probes of what a handle (or a bond table
// without a device) would launch, elph_wg_status.  (elph_bench_lattice_shape is lattice_shape.cpp's, elph_bench_kpm_bounds kpm_setup.hip's.)

#include "elph_internal.h"

static int bench_launch_unit(elph_handle_s *h, int what, int nrhs) {
    switch (what) {
        case 0: return elph_launch_mul(h, 2, h->work.z, h->work.b, nrhs);
        case 1: return elph_launch_cg_iteration(h, nrhs, 0);
        case 2: return elph_launch_kpm_apply(h, h->work.zp, h->work.b, nrhs, 0);
        case 3: return elph_launch_cg_iteration(h, nrhs, 1);
        case 11: return ELPH_E_ARG;      // (two half-batches on two streams: elph_bench_run drives both handles itself)
        case 4: return elph_launch_cg_kernel(h, nrhs, 0);
        case 5: return elph_launch_cg_kernel(h, nrhs, 1);
        default: {
            // 6, 7, 8: the three kernels of the KPM apply as the preconditioned iteration (case 3) launches them, one at a time
            return elph_launch_kpm_apply(h, h->work.zp, h->work.r, nrhs, h->plan.xr_in_fwd ? 2 : 1, 1 << (what - 6));
        }
    }
}

extern "C" int elph_bench_prepare(elph_handle h, int what, int nrhs, const double *B) {
    CHECK_H(h);
    RC(need_model(h));
    if (nrhs < 1 || what < 0 || what > 12) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if ((what == 2 || what == 3 || what == 10 || what == 11 || (what >= 6 && what <= 8)) && !h->kpm.ready) { elph_set_error("KPM not set up"); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, nrhs));
    if (B) {
        RC(elph_stage_in(h, h->work.b, B, nrhs));
    }
    // fixed-count CG: tol = 0 never converges, kmax = inf, x0 = 0
    CgParams P;
    P.tol = 0.0; P.kmax = INFINITY; P.maxiter = (long long)1 << 40; P.use_prec = (what == 3 || what == 10 || what == 11 || (what >= 6 && what <= 8)); P.record_hist = 0; P.hist_stride = 0;
    h->cur_params = P;
    HIPCHK(hipMemsetAsync(h->work.x, 0, (size_t)nrhs * (size_t)h->ndim * sizeof(double), h->stream));
    h->x_zero = false;
    RC(elph_launch_cg_init(h, nrhs, P.use_prec, true));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->x_zero = true;      // (x is zero: the elph_bench_run(9 | 10) that follows consumes the hint as run_cg does)
    return ELPH_OK;
}

extern "C" int elph_bench_get_x(elph_handle h, int nrhs, double *X) {
    CHECK_H(h);
    if (nrhs < 1 || nrhs > h->work.cap_rhs || !X) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_bench_info(elph_handle h, int nrhs, int *slices_per_wave) {
    CHECK_H(h);
    if (nrhs < 1 || !slices_per_wave) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *slices_per_wave = h->plan.T;      // (of the batch elph_bench_prepare planned)
    return ELPH_OK;
}

// Health of the workgroup-resident kernels on this handle: *cooling_down = solves left on the streaming iteration after a team timed
// out (0: the resident kernel is in use), *fallbacks = how many launches were given up and re-solved by the streaming iteration.
extern "C" int elph_wg_status(elph_handle h, int *cooling_down, int64_t *fallbacks) {
    CHECK_H(h);
    if (cooling_down) *cooling_down = h->res.cooldown;
    if (fallbacks) *fallbacks = h->res.fallbacks;
    return ELPH_OK;
}

extern "C" int elph_bench_wg_info(elph_handle h, int nrhs, int *usable, int *T, int *W, int *G) {
    CHECK_H(h);
    if (!usable || nrhs < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    int t = 0, w = 0, g = 0;
    *usable = (!h->res.cooling() && elph_wg_usable(h, &t, &w, &g, nrhs)) ? 1 : 0;
    if (T) *T = t;
    if (W) *W = w;
    if (G) *G = g;
    return ELPH_OK;
}

extern "C" int elph_bench_px_info(elph_handle h, int *fused) {
    CHECK_H(h);
    if (!fused) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *fused = h->plan.px ? (h->plan.ap == CgPlan::AP_SQ16 ? 2 : 1) : 0;      // 2: with the register-exchange k_cg_ap of the 16 x 16 lattice (cg_sq16.hip)
    return ELPH_OK;
}

extern "C" int elph_bench_pg_info(elph_handle h, int *kind, int *px, int *py, int *nw, int *tables) {
    CHECK_H(h);
    if (kind) *kind = h->shape.patch_kind();
    if (px) *px = h->shape.PX;
    if (py) *py = h->shape.PY;
    if (nw) *nw = std::max(h->shape.NW, 1);
    if (tables) *tables = (h->shape.patch() && h->kind == ELPH_MODEL_HOLSTEIN && !h->shape.hop_uniform && elph_pg_disorder_ok(h)) ? 1 : 0;
    return ELPH_OK;
}

// the time-axis chunking of the patch mat-vec kernels (pgrid.hip: elph_pg_chunks): from the rule's own inputs without a device, and as this handle
// would launch nvec vectors now (pg_launch_shape's re-shaping and the pin ELPH_PG_T included)
extern "C" int elph_bench_pg_chunks(int kernel, int px, int py, int nw, int honeycomb, int64_t nvec, int64_t ltau, int *out) {
    if (!out || kernel < PG_K_MUL || kernel > PG_K_CG_AP_PX || px < 1 || py < 1 || nw < 1 || nvec < 1 || ltau < 1 || ltau > INT32_MAX) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    const PgChunks ck = elph_pg_chunks(kernel, px, py, nw, honeycomb != 0, (long long)nvec, (int)ltau);
    out[0] = ck.T; out[1] = ck.nch; out[2] = ck.last;
    return ELPH_OK;
}
extern "C" int elph_bench_pg_chunk_info(elph_handle h, int kernel, int nvec, int *out) {
    CHECK_H(h);
    if (!out || kernel < PG_K_MUL || kernel > PG_K_CG_AP_PX || nvec < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (!h->shape.patch()) { elph_set_error("this handle has no patch layout"); return ELPH_E_UNSUPPORTED; }
    elph_pg_chunk_probe(h, kernel, nvec, out);
    return ELPH_OK;
}

// the plan of the resident CG launch that elph_create's handle would make for this bond table and time axis, on a host-only handle (no
// device): the slots of _lib.WG_PLAN_SLOTS
extern "C" int elph_bench_wg_plan(int kind, int64_t nsites, int64_t ltau, int64_t nbonds, const int64_t *neighbor_table, const double *cosht,
                                  const double *sinht, int nrhs, int world, int *out) {
    if (!out || (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) || nsites < 1 || nsites > ELPH_MAX_SITES || ltau < 1 || nbonds < 0 || nrhs < 1 || world < 0) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    elph_handle_s h;
    elph_i_host_handle(&h, kind, nsites, ltau, nbonds, neighbor_table, cosht, sinht);
    elph_i_wg_plan_probe(&h, nrhs, world, out);
    return ELPH_OK;
}

// the plan of one tau-axis transform (dft_mfma.hip: elph_plan_dft) at Ltau = ltau without a device, and on a handle's own h->dft.shape: the
// slots of _lib.DFT_PLAN_SLOTS
extern "C" int elph_bench_dft_plan(int64_t ltau, int which, int inverse, int N, int nvec, int nrz_slots, int *out) {
    if (!out || ltau < 1 || (which != DFT_TWISTED && which != DFT_PLAIN) || N < 1 || nvec < 1 || nrz_slots < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    elph_i_dft_plan_probe(dft_shape(ltau), which, inverse != 0, N, nvec, nrz_slots, out);
    return ELPH_OK;
}
extern "C" int elph_bench_dft_info(elph_handle h, int which, int inverse, int N, int nvec, int nrz_slots, int *out) {
    CHECK_H(h);
    if (!out || (which != DFT_TWISTED && which != DFT_PLAIN) || N < 1 || nvec < 1 || nrz_slots < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    elph_i_dft_plan_probe(h->dft.shape, which, inverse != 0, N, nvec, nrz_slots, out);
    return ELPH_OK;
}

// The time of `body` between two events on the handle's stream: e0 after the stream has drained and before body's first launch, e1 after
// its last (or after the join of the parts of a batch).  `name` leads the text of a HIP error, which goes before body's own.
template <class Body>
static int timed(elph_handle_s *h, const char *name, const Body &body, double *ms_total) {
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    int rc = ELPH_OK;
    hipError_t er = hipStreamSynchronize(h->stream);
    if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
    if (er == hipSuccess) rc = body();
    if (er == hipSuccess) er = hipEventRecord(e1, h->stream);
    if (er == hipSuccess) er = hipEventSynchronize(e1);
    float ms = 0.f;
    if (er == hipSuccess) er = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (er != hipSuccess) { elph_set_error("%s: %s", name, hipGetErrorString(er)); return ELPH_E_HIP; }
    if (rc) return rc;
    *ms_total = (double)ms;
    return ELPH_OK;
}

extern "C" int elph_bench_run(elph_handle h, int what, int nrhs, int reps, int use_graph, double *ms_total) {
    CHECK_H(h);
    if (nrhs < 1 || nrhs > h->work.cap_rhs || reps < 1 || !ms_total || what < 0 || what > 12) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (use_graph) { elph_set_error("elph_bench_run: captured-graph replay is not supported (use_graph must be 0)"); return ELPH_E_UNSUPPORTED; }
    if (what == 12) {        // `reps` un-preconditioned iterations of every right-hand side in the slab form of a large lattice (slabs.hip): sum of the launches' event times
        if (!elph_i_slabs_usable(h, nrhs)) { elph_set_error("the slab form does not apply to this handle / batch"); return ELPH_E_UNSUPPORTED; }
        bool ran = false;
        std::vector<int64_t> its((size_t)nrhs);
        RC(elph_i_slabs_solve(h, nrhs, h->cur_params, reps, its.data(), &ran, ms_total));
        if (!ran) { elph_set_error("the slab form gave up (time-out)"); return ELPH_E_HIP; }
        return ELPH_OK;
    }
    if (what == 9 || what == 10) {        // `reps` iterations of the whole batch in one launch of the workgroup-resident kernel (10: the preconditioned one)
        bool ran = false, aborted = false;
        const bool x0_zero = h->x_zero;      // (x is known to be zero only right after elph_bench_prepare)
        h->x_zero = false;
        CgBufs B = elph_make_bufs(h, nrhs);
        B.params = h->cur_params;
        double ms = 0.0;
        RC(timed(h, "bench (workgroup-resident)", [&]() -> int {
            RC(elph_wg_cooldown_step(h));
            RC((what == 9) ? elph_wg_cg(h, B, nrhs, reps, x0_zero, nullptr, &ran) : elph_pcg_wg(h, B, nrhs, reps, nullptr, &ran));
            if (!ran) { elph_set_error("the workgroup-resident kernel does not apply to this handle"); return ELPH_E_UNSUPPORTED; }
            return ELPH_OK;
        }, &ms));
        RC(elph_wg_aborted(h, &aborted));
        if (aborted) { elph_wg_timed_out(h); return ELPH_E_HIP; }
        *ms_total = ms;
        return ELPH_OK;
    }
    if (what == 11) {        // `reps` preconditioned iterations of the batch as two half-batches on two streams (run_cg's form from 192 right-hand sides)
        if (!split_legal(h, nrhs, 1, false)) { elph_set_error("the two-stream form does not apply to this batch"); return ELPH_E_UNSUPPORTED; }
        std::shared_ptr<void> parts;      // (outlives the timing: its end drains the other streams)
        return timed(h, "bench (two streams)", [&]() -> int { return elph_i_split_iterations(h, nrhs, reps, &parts); }, ms_total);
    }
    return timed(h, "elph_bench_run", [&]() -> int {
        for (int r = 0; r < reps; ++r) RC(bench_launch_unit(h, what, nrhs));
        return ELPH_OK;
    }, ms_total);
}
