// cg_solve.hip — the CG driver (the resident forms where they apply, else the streaming iteration in chunks, as one part or as the parts
// of a preconditioned batch), the ldiv! flag logic (Models.jl:74-186), the entry points elph_ldiv* and elph_cg_solve.  Host orchestration only.

#include <cstdlib>

#include "elph_internal.h"

// ------------------------------------------------------------------------------------------
// A large KPM-preconditioned batch as TWO half-batches on two streams.  One iteration is four dependent kernels (k_cg_ap, forward
// transform + residual update, Chebyshev recursion, inverse transform + p/x-update), each ending in a drain of the whole chip before the
// next may start, the Chebyshev one latency-bound and the transforms quantised in rounds of waves (288 right-hand sides: 2.25 rounds).
// Two independent halves, each with its own chain of kernels, fill one another's tails and run the latency-bound kernel of one under
// the HBM-bound kernels of the other.  The second half is a VIEW of the handle: a copy whose per-right-hand-side device arrays start at
// right-hand side n/2 and whose stream is the second stream — every launcher reads buffers and stream from the handle it is given, so
// nothing else changes, and each right-hand side sees exactly the arithmetic of the single-stream form (same kernels, same partial-sum
// layout per right-hand side).  Needs the p/x-fused iteration (the unfused one ping-pongs p between two slots whose distance depends on
// the batch size) and halves that hold whole groups of chains.  ELPH_SPLIT_STREAMS=0 off, =1 wherever legal; default from 192 right-hand sides.
// ------------------------------------------------------------------------------------------
__global__ void k_spin_us(long long ticks, long long *sink) {      // wall_clock64: 100 MHz
    const long long t0 = wall_clock64();
    long long t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (sink) *sink = t;
}

// do kernels on `a` and `b` run at the same time?  (two 40-us spins: together ~40 us, one after the other ~80)
static int streams_overlap(hipStream_t a, hipStream_t b, bool *yes) {
    hipEvent_t e0 = nullptr, e1 = nullptr, eb = nullptr;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
    float best = 1e9f;
    hipError_t er = hipSuccess;
    for (int rep = 0; rep < 3 && er == hipSuccess; ++rep) {
        er = hipStreamSynchronize(a);
        if (er == hipSuccess) er = hipStreamSynchronize(b);
        if (er == hipSuccess) er = hipEventRecord(e0, a);
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(1), 0, a, 4000LL, (long long *)nullptr);
            hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(1), 0, b, 4000LL, (long long *)nullptr);
            er = hipEventRecord(eb, b);
        }
        if (er == hipSuccess) er = hipStreamWaitEvent(a, eb, 0);
        if (er == hipSuccess) er = hipEventRecord(e1, a);
        if (er == hipSuccess) er = hipEventSynchronize(e1);
        float ms = 0.f;
        if (er == hipSuccess) er = hipEventElapsedTime(&ms, e0, e1);
        if (er == hipSuccess && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(eb);
    if (er != hipSuccess) { elph_set_error("stream pairing probe: %s", hipGetErrorString(er)); return ELPH_E_HIP; }
    *yes = best < 0.062f;      // (40 us each: < 62 us = they overlapped)
    return ELPH_OK;
}

static int make_overlapping_stream(elph_handle_s *h, hipStream_t *out) {
    std::vector<hipStream_t> aside;
    hipStream_t chosen = nullptr;
    int rc = ELPH_OK;
    for (int attempt = 0; attempt < 8 && !chosen && rc == ELPH_OK; ++attempt) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { elph_set_error("hipStreamCreate failed"); rc = ELPH_E_HIP; break; }
        bool ok = true;
        rc = streams_overlap(h->stream, s, &ok);
        if (rc == ELPH_OK && (ok || attempt == 7)) chosen = s;      // (eight in a row on the main stream's queue: take it, the form still works)
        else aside.push_back(s);
    }
    for (hipStream_t s : aside) (void)hipStreamDestroy(s);
    if (rc) { if (chosen) (void)hipStreamDestroy(chosen); return rc; }
    *out = chosen;
    return ELPH_OK;
}

// The parts of a solve's chunk loop: `ways` parts of n1 right-hand sides each, part 0 the handle itself on its own stream — one part (the
// default: a one-stream solve) or ELPH_SPLIT_PARTS of a preconditioned batch on streams of their own (split_begin)
struct SplitRun {
    bool on = false, ok = false;
    int ways = 1, n1 = 0;
    elph_handle_s *main = nullptr, *view[ELPH_SPLIT_PARTS] = {};
    CgPlan before;                                        // the whole batch's plan (split_begin replaces it with the parts')
    SplitRun(elph_handle_s *h, int nrhs) : n1(nrhs), main(h) { view[0] = h; }
    // A solve that leaves through an error return must not leave kernels of the other streams in flight behind it (they write work.x, work.p, work.r,
    // work.state of their parts while the caller's next step — ldiv's zero-fill, a retry, a new solve — runs on the main stream), nor the handle
    // believing in a plan that never ran to its end.
    ~SplitRun() {
        for (int k = 1; k < ways; ++k)
            if (view[k]) {
                if (on) (void)hipStreamSynchronize(view[k]->stream);
                delete view[k];
            }
        if (ways > 1 && !ok) main->plan = before;      // (split_begin changed it; also when it failed before its streams ran)
    }
};

bool split_legal(elph_handle_s *h, int nrhs, int use_prec, bool hist) {
    const int ways = ELPH_SPLIT_PARTS;
    if (!use_prec || hist || nrhs < 2 * ways || (nrhs % ways) || h->solo_chain >= 0 || h->dot_hi > 0) return false;
    const int n1 = nrhs / ways;
    if (n1 % std::max(1, h->nchains) || n1 % std::max(1, h->kpm.nch())) return false;
    return elph_plan_cg(h, n1, true, nrhs).px;      // (the parts choose their slices per wave for the whole batch in flight)
}

static bool split_wanted(elph_handle_s *h, int nrhs, int use_prec, bool hist) {
    const char *e = getenv("ELPH_SPLIT_STREAMS");
    if (e && e[0] == '0') return false;
    if (!split_legal(h, nrhs, use_prec, hist)) return false;
    // (config C, 128 right-hand sides: 130 us either way, profiles/r05/px_chunk_T.log; five sites per lane — the honeycomb lattice of config D,
    //  whose fused kernel stays at two waves per SIMD — gains from 64 on: D 128: 131 -> 116 us, 256: 262 -> 230, profiles/r05/px_fused_five_sites_per_lane.log;
    //  honeycomb 16 x 16 cells, eight sites per lane: 64 right-hand sides 64 -> 55 us, 256: 159 -> 145; D at 64: 89 -> 87)
    // (hopping disorder on 4 x 4 patches: the table variants of the patch kernels hold 40 KB of LDS per wavefront — two half-batches side by side lose to one
    //  stream: 32 x 32 at 96 right-hand sides 763 against 732 us, 28 x 28 695 against 663; profiles/r06/hopping_disorder_patch_kernels_with_tables.log)
    if (!(e && e[0] == '1') && h->shape.PX * h->shape.PY >= 16 && !h->kpm.hop_uniform && elph_pg_disorder_ok(h)) return false;
    return (e && e[0] == '1') || nrhs >= (h->npl >= 5 ? 64 : 192);
}

// after elph_launch_cg_init(h, nrhs, 1, …) on the main stream
static int split_begin(elph_handle_s *h, int nrhs, SplitRun &S) {
    S.ways = ELPH_SPLIT_PARTS;
    S.n1 = nrhs / S.ways;
    S.before = h->plan;
    // The parts must run on DIFFERENT hardware queues.  HIP maps its streams onto a few hardware queues per process (four by default,
    // GPU_MAX_HW_QUEUES) by a rule of its own: in a process that holds several handles a part's stream can share the queue of the handle's main
    // stream — the parts then run one after the other, slower than one stream (round 6: the second handle of a process, 32 x 32 at 72 right-hand
    // sides: 437 us instead of 353; a stream priority of its own did not change the mapping).  So the pairing is MEASURED once per stream: a spin
    // kernel on each of the two streams at the same time — two that overlap finish in the time of one; a candidate that does not is set aside
    // (kept alive until the choice is made, so that the next candidate does not inherit its queue) and the next one is tried.
    for (int k = 1; k < S.ways; ++k)
        if (!h->split_stream[k]) RC(make_overlapping_stream(h, &h->split_stream[k]));
    if (!h->split_ev) HIPCHK(hipEventCreateWithFlags(&h->split_ev, hipEventDisableTiming));
    h->plan = elph_plan_cg(h, S.n1, true, nrhs);          // (split_legal: the parts run p/x-fused whatever the whole batch would have run)
    HIPCHK(hipEventRecord(h->split_ev, h->stream));       // the start state (x0, r0, p0, rho0 of every right-hand side) is on the main stream
    for (int k = 1; k < S.ways; ++k) {
        elph_handle_s *v = S.view[k] = new elph_handle_s(*h);
        v->work = h->work.part((size_t)k * (size_t)S.n1);
        v->stream = h->split_stream[k];
        HIPCHK(hipStreamWaitEvent(v->stream, h->split_ev, 0));
    }
    S.on = true;
    return ELPH_OK;
}

// one iteration of every part, each on its stream
static int split_iteration(SplitRun &S, int use_prec) {
    for (int k = 0; k < S.ways; ++k) RC(elph_launch_cg_iteration(S.view[k], S.n1, use_prec));
    return ELPH_OK;
}

// the main stream continues only after the other parts have finished
static int split_join(SplitRun &S) {
    elph_handle_s *h = S.main;
    for (int k = 1; k < S.ways; ++k) {
        HIPCHK(hipEventRecord(h->split_ev, S.view[k]->stream));
        HIPCHK(hipStreamWaitEvent(h->stream, h->split_ev, 0));
    }
    return ELPH_OK;
}

// elph_bench_run's two-stream form (bench_hooks.hip): `reps` preconditioned iterations of a batch that split_legal accepts, as parts, joined
// on the main stream.  *run keeps the parts until the caller lets go of it — after it has timed the join; SplitRun's end drains their streams.
int elph_i_split_iterations(elph_handle_s *h, int nrhs, int reps, std::shared_ptr<void> *run) {
    auto S = std::make_shared<SplitRun>(h, nrhs);
    *run = S;
    int rc = split_begin(h, nrhs, *S);
    for (int r = 0; r < reps && rc == ELPH_OK; ++r) rc = split_iteration(*S, 1);
    if (rc == ELPH_OK) rc = split_join(*S);
    if (S->on) h->ap_count = S->view[S->ways - 1]->ap_count;
    S->ok = (rc == ELPH_OK);
    return rc;
}

// The CG states of every part come back to the host (each on its stream, then all drained): iters[r] = the iteration count of every
// right-hand side whose newer state copy is terminal; *all_done: every one is
static int read_states(const SplitRun &S, int64_t *iters, bool *all_done) {
    for (int k = 0; k < S.ways; ++k)
        HIPCHK(hipMemcpyAsync(S.view[k]->work.h_state, S.view[k]->work.state, sizeof(CgState) * 2 * (size_t)S.n1, hipMemcpyDeviceToHost, S.view[k]->stream));
    for (int k = 0; k < S.ways; ++k) HIPCHK(hipStreamSynchronize(S.view[k]->stream));
    *all_done = true;
    for (int r = 0; r < S.ways * S.n1; ++r) {
        const CgState &a = S.main->work.h_state[2 * r], &b = S.main->work.h_state[2 * r + 1];
        const CgState &s = (b.seq > a.seq) ? b : a;
        if (!s.done) *all_done = false;
        else iters[r] = s.iters;
    }
    return ELPH_OK;
}

// the eps histories of a finished solve (host, nrhs x (maxiter + 1); nullptr: none recorded)
static int read_hist(elph_handle_s *h, int nrhs, int64_t maxiter, double *eps_hist) {
    if (!eps_hist) return ELPH_OK;
    HIPCHK(hipMemcpyAsync(eps_hist, h->work.hist, sizeof(double) * (size_t)nrhs * (size_t)(maxiter + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// Which resident form would this solve take, ignoring the cool-down (except that a handle that cools down does not BUILD its slabs just to
// be counted) — in the order they are tried: the whole un-preconditioned solve in
// one launch with the Krylov vectors in registers (cg_wg.hip: k_cg_wg); on a lattice beyond one wave's slice the same kernel on slabs of
// rows of the lattice, all on this device, one launch per right-hand side (slabs.hip; x0 = 0 only — the slab kernel starts from it:
// ldiv!'s zero-fill); the whole PRECONDITIONED solve in one launch for one to eight right-hand sides on the 16 x 16 square lattice
// (pcg_wg.hip: k_pcg_wg).  `after`: the forms up to that one have declined.  The shape only — elph_wg_cg's cost rule is its own.
enum ResidentForm { RES_NONE, RES_CG_WG, RES_SLABS, RES_PCG_WG };
static ResidentForm resident_form(elph_handle_s *h, int nrhs, int use_prec, bool x0_zero, int64_t maxiter, ResidentForm after = RES_NONE) {
    if (maxiter < 1) return RES_NONE;
    if (use_prec) return (after < RES_PCG_WG && elph_pcg_wg_usable(h, nrhs)) ? RES_PCG_WG : RES_NONE;
    if (after < RES_CG_WG && h->fast && elph_wg_usable(h, nullptr, nullptr, nullptr, nrhs)) return RES_CG_WG;
    // (cooling down: only slabs that exist already count — it has them, or the form is not its own)
    if (after < RES_SLABS && x0_zero && (h->slabs || !h->res.cooling()) && elph_i_slabs_usable(h, nrhs)) return RES_SLABS;
    return RES_NONE;
}

// One attempt of k_cg_wg / k_pcg_wg (use_prec) at the solve elph_launch_cg_init has set up.  The launcher parks the caller's initial guess
// in x0_save — scratch its kind of solve does not use — once it has decided to launch.  *solved: the states are terminal, iters filled.
// Otherwise the streaming iteration can start: nothing was launched (the form declined), or a team gave up (x, r of the right-hand sides
// that had finished were overwritten) and every right-hand side is back at the caller's initial guess, re-initialised.
static int resident_attempt(elph_handle_s *h, const SplitRun &S, int nrhs, int use_prec, const CgParams &P, bool x0_zero, double *x0_save,
                            int64_t *iters, bool *solved) {
    *solved = false;
    bool ran = false, all_done = false, aborted = false;
    CgBufs B = elph_make_bufs(h, nrhs);
    B.params = P;
    RC(use_prec ? elph_pcg_wg(h, B, nrhs, 0, x0_save, &ran) : elph_wg_cg(h, B, nrhs, 0, x0_zero, x0_save, &ran));
    if (!ran) return ELPH_OK;
    RC(read_states(S, iters, &all_done));
    RC(elph_wg_aborted(h, &aborted));
    if (!aborted) {
        if (!all_done) {
            elph_set_error(use_prec ? "resident preconditioned CG ended without a terminal state (internal error)"
                                    : "workgroup-resident CG ended without a terminal state (internal error)");
            return ELPH_E_STATE;
        }
        *solved = true;
        return ELPH_OK;
    }
    elph_wg_timed_out(h);
    HIPCHK(hipMemcpyAsync(h->work.x, x0_save, (size_t)nrhs * (size_t)h->ndim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return elph_launch_cg_init(h, nrhs, use_prec);
}

// Runs CG on work.b / work.x (layout S) for nrhs right-hand sides.  Returns per-rhs iteration counts.
static int run_cg(elph_handle_s *h, int nrhs, int use_prec, double tol, int64_t maxiter, double kmax, int64_t *iters,
                  double *eps_hist /* host, optional, nrhs*(maxiter+1) */) {
    const bool x0_zero = h->x_zero;        // the hint belongs to THIS solve: consumed before anything can return
    h->x_zero = false;
    if (use_prec && !h->kpm.ready) { elph_set_error("preconditioned solve requested before elph_kpm_setup"); return ELPH_E_STATE; }
    CgParams P;
    P.tol = tol; P.kmax = kmax; P.maxiter = maxiter; P.use_prec = use_prec;
    P.record_hist = eps_hist ? 1 : 0;
    P.hist_stride = maxiter + 1;
    if (eps_hist) {
        const int64_t need = (int64_t)nrhs * (maxiter + 1);
        if (need > h->work.hist_cap) {
            HIPCHK(hipStreamSynchronize(h->stream));
            RC(dev_alloc(&h->work.hist, (size_t)need));
            h->work.hist_cap = need;
        }
    }
    h->cur_params = P;
    // one solve of the cool-down after a resident kernel timed out — counted only for solves that WOULD have taken a resident kernel (any
    // form, either kind of solve): a stream of large streaming batches in between does not bring the retry forward, and a solve that
    // never launches a resident kernel does not clear the abort word
    if (h->res.cooling() && resident_form(h, nrhs, use_prec, x0_zero, maxiter) != RES_NONE) RC(elph_wg_cooldown_step(h));
    RC(elph_launch_cg_init(h, nrhs, use_prec, x0_zero));      // (x0 = 0: A x0 = 0 without the mat-vec)
    SplitRun S(h, nrhs);

    // the resident forms, each where it applies; one that declines leaves the solve to the next, a time-out to the streaming iteration
    for (ResidentForm f = RES_NONE; !h->res.cooling() && (f = resident_form(h, nrhs, use_prec, x0_zero, maxiter, f)) != RES_NONE;) {
        bool solved = false;
        if (f == RES_SLABS) {
            RC(elph_i_slabs_solve(h, nrhs, P, 0, iters, &solved, nullptr));
            if (!solved) RC(elph_launch_cg_init(h, nrhs, use_prec, true));      // (x is zero again: elph_i_slabs_solve)
        } else {
            RC(resident_attempt(h, S, nrhs, use_prec, P, x0_zero, use_prec ? h->work.tmp : h->work.zp, iters, &solved));
        }
        if (solved) return read_hist(h, nrhs, maxiter, eps_hist);
    }

    // the streaming iteration, ELPH_CG_CHUNK iterations of every part between two reads of the states
    if (split_wanted(h, nrhs, use_prec, eps_hist != nullptr)) RC(split_begin(h, nrhs, S));
    const int64_t max_chunks = (maxiter + 1 + ELPH_CG_CHUNK - 1) / ELPH_CG_CHUNK + 1;
    bool all_done = false;
    for (int64_t c = 0; c < max_chunks && !all_done; ++c) {
        for (int it = 0; it < ELPH_CG_CHUNK; ++it) RC(split_iteration(S, use_prec));
        RC(read_states(S, iters, &all_done));
    }
    h->ap_count = S.view[S.ways - 1]->ap_count;
    S.ok = all_done;
    if (!all_done) {
        elph_set_error(S.ways > 1 ? "CG chunk loop (two streams) ended without a terminal state (internal error)" : "CG chunk loop ended without a terminal state (internal error)");
        return ELPH_E_STATE;
    }
    return read_hist(h, nrhs, maxiter, eps_hist);
}

// residual + flag logic of ldiv! for rhs already solved into work.x; zeroes x where flag > 0
static int residual_and_flags(elph_handle_s *h, int nrhs, const int64_t *iters, int64_t cmp_maxiter, double *resid, int *flag) {
    RC(elph_launch_residual(h, nrhs));
    HIPCHK(hipMemcpyAsync(h->work.h_scal, h->work.scal, sizeof(double) * (size_t)nrhs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int r = 0; r < nrhs; ++r) {
        resid[r] = h->work.h_scal[r];
        if (resid[r] > sqrt(h->tol)) {           // Models.jl:100,157 (NaN compares false, as in the reference)
            flag[r] = (iters[r] == cmp_maxiter) ? 1 : 2;
            RC(elph_launch_zero(h, h->work.x + (size_t)r * (size_t)h->ndim, h->ndim));   // fill!(x,0)
        } else {
            flag[r] = 0;
        }
    }
    return ELPH_OK;
}

// ldiv! on device-resident layout-S work.b/work.x
int elph_i_ldiv_core(elph_handle_s *h, int nrhs, int use_prec, int64_t maxiter, int64_t *iters, double *resid, int *flag) {
    RC(need_model(h));
    if (maxiter == 0) maxiter = h->maxiter;                                  // Models.jl:78-80,143-145
    RC(run_cg(h, nrhs, use_prec ? 1 : 0, h->tol, maxiter, h->kmax, iters, nullptr));
    // the flag of a preconditioned solve compares maxiter (Models.jl:103), that of a plain one solver.maxiter (Models.jl:160)
    RC(residual_and_flags(h, nrhs, iters, use_prec ? maxiter : h->maxiter, resid, flag));
    if (!use_prec) return ELPH_OK;
    // failed right-hand sides: retry without preconditioner, 10x maxiter, from x = 0 (Models.jl:129-133)
    for (int r = 0; r < nrhs; ++r) {
        if (flag[r] == 0) continue;
        int64_t it1 = 0; double rs1 = 0; int fl1 = 0;
        RC(elph_retry_in_slot0(h, r, [&]() -> int {
            RC(run_cg(h, 1, 0, h->tol, 10 * maxiter, h->kmax, &it1, nullptr));
            return residual_and_flags(h, 1, &it1, h->maxiter, &rs1, &fl1);
        }));
        iters[r] = it1; resid[r] = rs1; flag[r] = fl1;
    }
    return ELPH_OK;
}

static int stage_in_dev(elph_handle_s *h, int nrhs, const double *X_dev, const double *B_dev) {
    RC(elph_work_reserve(h, nrhs));
    RC(elph_launch_r2s(h, h->work.b, B_dev, nrhs));
    RC(elph_launch_r2s(h, h->work.x, X_dev, nrhs));
    h->x_zero = false;                              // (a caller's initial guess)
    return ELPH_OK;
}

// Is the caller's initial guess all zeros?  Looked at only where it decides something: a lattice beyond one wave's slice whose
// un-preconditioned solve of one or two right-hand sides the slab form (slabs.hip; it starts from x = 0) could take.  Stops at the first
// non-zero; a zero guess costs one pass over the vector on the host (1.3 MB at 32 x 32 sites, 160 slices) — against a solve of milliseconds.
static bool x0_is_zero(elph_handle_s *h, int nrhs, int use_prec, const double *X) {
    if (use_prec || h->have_E == false) return false;
    if (!elph_i_slabs_usable(h, nrhs)) return false;      // (also while cooling down: the hint still lets run_cg count the solve)
    const size_t n = (size_t)nrhs * (size_t)h->ndim;
    for (size_t i = 0; i < n; ++i) if (X[i] != 0.0) return false;
    return true;
}

// The caller's initial guess (host, reference layout) into work.x.  fill!(x, 0) of the callers (HMC.jl:854, GreensFunctions.jl:334) seen
// on the host becomes a memset and the x = 0 hint: the slab form may take the solve.
static int stage_x0(elph_handle_s *h, int nrhs, int use_prec, const double *X) {
    if (x0_is_zero(h, nrhs, use_prec, X)) {
        HIPCHK(hipMemsetAsync(h->work.x, 0, (size_t)nrhs * (size_t)h->ndim * sizeof(double), h->stream));
        h->x_zero = true;
    } else {
        RC(elph_stage_in(h, h->work.x, X, nrhs));
        h->x_zero = false;                          // (a caller's initial guess)
    }
    return ELPH_OK;
}

extern "C" int elph_ldiv_batched_dev(elph_handle h, int nrhs, double *X_dev, const double *B_dev, int use_prec,
                                     int64_t maxiter, int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    if (nrhs < 1 || !X_dev || !B_dev || !iters || !residual_error || !flag || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(stage_in_dev(h, nrhs, X_dev, B_dev));
    RC(elph_i_ldiv_core(h, nrhs, use_prec, maxiter, iters, residual_error, flag));
    RC(elph_launch_s2r(h, X_dev, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_ldiv_dev(elph_handle h, double *x_dev, const double *b_dev, int use_prec, int64_t maxiter,
                             int64_t *iters, double *residual_error, int *flag) {
    return elph_ldiv_batched_dev(h, 1, x_dev, b_dev, use_prec, maxiter, iters, residual_error, flag);
}

extern "C" int elph_ldiv_batched(elph_handle h, int nrhs, double *X, const double *B, int use_prec, int64_t maxiter,
                                 int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    if (nrhs < 1 || !X || !B || !iters || !residual_error || !flag || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_work_reserve(h, nrhs));
    RC(elph_stage_in(h, h->work.b, B, nrhs));
    RC(stage_x0(h, nrhs, use_prec, X));
    RC(elph_i_ldiv_core(h, nrhs, use_prec, maxiter, iters, residual_error, flag));
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_ldiv(elph_handle h, double *x, const double *b, int use_prec, int64_t maxiter, int64_t *iters,
                         double *residual_error, int *flag) {
    return elph_ldiv_batched(h, 1, x, b, use_prec, maxiter, iters, residual_error, flag);
}

extern "C" int elph_cg_solve(elph_handle h, double *x, const double *b, double tol, int64_t maxiter, double kappa_max,
                             int use_precond, int64_t *iters, double *eps_hist) {
    CHECK_H(h);
    RC(need_model(h));
    if (!x || !b || !iters || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (maxiter == 0) maxiter = h->maxiter;       // iszero() defaults, IterativeSolvers.jl:160-173
    if (tol == 0.0) tol = h->tol;
    if (kappa_max == 0.0) kappa_max = h->kmax;
    RC(elph_stage_in(h, h->work.b, b, 1));
    RC(stage_x0(h, 1, use_precond, x));
    RC(run_cg(h, 1, use_precond ? 1 : 0, tol, maxiter, kappa_max, iters, eps_hist));
    RC(elph_stage_out(h, x, h->work.x, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// (internal: shard.hip) Sites [site_lo, site_hi) (0-based) enter the inner products of the streaming CG (p.z, r.r, b.b); the other
// sites of the handle's lattice are ghost sites of a spatial shard: they take part in the mat-vec, their values come from the
// neighbouring ranks.  A restricted range runs the generic kernel family.  (0, nsites) restores the default.
int elph_i_set_dot_range(elph_handle_s *h, int64_t site_lo, int64_t site_hi) {
    if (site_lo < 0 || site_hi > h->N || site_lo >= site_hi) { elph_set_error("bad site range [%lld, %lld)", (long long)site_lo, (long long)site_hi); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool all = (site_lo == 0 && site_hi == h->N);
    h->dot_lo = all ? 0 : (int)site_lo;
    h->dot_hi = all ? 0 : (int)site_hi;
    h->fast = all ? h->fast_capable : false;
    return ELPH_OK;
}
