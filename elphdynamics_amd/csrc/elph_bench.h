// elph_bench.h — PRIVATE measurement hooks of libelphgpu (bench.py, tools/): exported by the library, NOT part of the drop-in ABI
// (include/elph_gpu.h).  Nothing a caller of the operator API needs; signatures may change between rounds.
#pragma once
#include "../../include/elph_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement of one hot-path unit with inputs resident in HBM (no host traffic in the timed region).
 * what: 0 = MᵀM apply, 1 = one un-preconditioned CG iteration of the two-kernel (streaming) form (k_cg_ap + k_cg_xr, stop
 *       test disabled), 2 = KPM apply, 3 = one preconditioned CG iteration, 4 = k_cg_ap alone, 5 = k_cg_xr alone,
 *       6 / 7 / 8 = the forward transform / Chebyshev recursion / inverse transform of the KPM apply alone (as the
 *       preconditioned iteration launches them), 9 = `reps` un-preconditioned CG iterations of every right-hand side in ONE
 *       launch of the workgroup-resident kernel (cg_wg.hip: the form elph_ldiv/elph_cg_solve use when elph_bench_wg_info
 *       says it applies; needs a fresh elph_bench_prepare before every run), 10 = `reps` KPM-PRECONDITIONED iterations in one
 *       launch of the resident preconditioned kernel (pcg_wg.hip: what elph_ldiv with a preconditioner runs for 1..8 right-hand
 *       sides on the 16 x 16 square lattice; ELPH_E_UNSUPPORTED elsewhere; fresh elph_bench_prepare(…, 10, …) before every run), 11 = `reps` preconditioned iterations
 *       of the batch as TWO half-batches on two streams (the form elph_ldiv_batched runs from 192 right-hand sides; prepare with what = 3;
 *       ELPH_E_UNSUPPORTED where the halves are not whole groups of chains or the p/x-fused iteration does not apply),
 *       12 = `reps` un-preconditioned iterations of every right-hand side in the SLAB form of a lattice beyond 320 sites (slabs.hip: the resident
 *       kernel on slabs of rows, all on this device, one launch per right-hand side; prepare with what = 1; *ms_total = sum of the launches).
 * elph_bench_prepare: loads nrhs right-hand sides (B: host, reference layout, nrhs*ndim; NULL keeps what the
 *   last solve left on the device), zeroes x, seeds the CG state with tol = 0 (never converges).
 * elph_bench_run: launches `reps` units back-to-back on the handle's stream, brackets them with HIP events recorded on that
 *   stream, synchronises, and returns the event time in ms (total, not per rep).  use_graph must be 0: the replay of
 *   captured graphs was removed, and any other value returns ELPH_E_UNSUPPORTED (the parameter stays for the ABI). */
int elph_bench_prepare(elph_handle h, int what, int nrhs, const double *B);
int elph_bench_run(elph_handle h, int what, int nrhs, int reps, int use_graph, double *ms_total);
/* The solution block x the last elph_bench_run left on the device (nrhs right-hand sides, reference layout, nrhs*ndim doubles) copied to X:
 * what a solve of the batch hands its caller.  The two-kernel forms apply x += alpha p one iteration late (in the next k_cg_ap). */
int elph_bench_get_x(elph_handle h, int nrhs, double *X);
/* Which k_cg_ap variant a batch of nrhs uses: *slices_per_wave = 1 (k_cg_ap_fast / generic) or T (k_cg_ap_chunk<T>). */
int elph_bench_info(elph_handle h, int nrhs, int *slices_per_wave);
/* Whether un-preconditioned solves of a batch of nrhs right-hand sides run as the workgroup-resident kernel (*usable = 1) and
 * its shape: T tau-slices per wavefront, W wavefronts per workgroup, G workgroups per right-hand side. */
int elph_bench_wg_info(elph_handle h, int nrhs, int *usable, int *T, int *W, int *G);

/* Whether the LAST preconditioned solve / elph_bench_prepare ran its iteration p/x-fused (*fused = 1: x += alpha p and p = P^-1 r + beta p
 * in the epilogue of the inverse tau-transform, k_cg_ap_chunk<PX> reading the ready p; kernels.hip: px_plan). */
int elph_bench_px_info(elph_handle h, int *fused);

/* The patch layout of this handle (pgrid.hip), if any: *kind 0 none, 1 square, 2 honeycomb, 3 triangular, 4 simple cubic (2 x 2 x 2 sites per thread, reported as
 * PX = PY = 2); the patch shape and the wavefronts per time slice; *tables = 1 when the hopping is disordered and the mat-vec / Chebyshev kernels take the patch layout with a (cosh, sinh) table in LDS. */
int elph_bench_pg_info(elph_handle h, int *kind, int *px, int *py, int *nw, int *tables);

/* The time-axis chunking of one launch of the patch mat-vec kernels (pgrid.hip: elph_pg_chunks, the one rule both launchers call).  kernel: 0 k_mul_pg,
 * 1 k_cg_ap_pg, 2 k_cg_ap_pg<PX> (the p/x-fused iteration).  A workgroup walks T consecutive time slices of one vector; out = T, the chunks per vector,
 * the slices of the last chunk.  ELPH_PG_T=n pins T for both kernels (read per call, clamped to [1, ltau]; unset or not a whole number: the rule).
 * elph_bench_pg_chunks: from the rule's own inputs — the launch shape (px, py, nw, honeycomb or not), the vectors of the launch, ltau; out[3]; needs no
 * device.  elph_bench_pg_chunk_info: what this handle would launch for nvec vectors now, out[7] = the launch shape px, py, nw (which a large fused batch
 * re-shapes, ELPH_PG_2X2_FROM), T, chunks, last, and whether the handle's mat-vecs and streaming CG iteration take these kernels at all (0: a lane
 * program, ELPH_NO_PG=1 or hopping disorder without a table variant keep them out); ELPH_E_UNSUPPORTED on a handle without a patch layout. */
int elph_bench_pg_chunks(int kernel, int px, int py, int nw, int honeycomb, int64_t nvec, int64_t ltau, int *out);
int elph_bench_pg_chunk_info(elph_handle h, int kernel, int nvec, int *out);

/* What elph_create would recognise in this bond table (same table arguments; needs no device): out[16] = the small square lattice's LX, LY and its
 * DPP size (1: 8 x 8, 2: 16 x 16, else 0); the honeycomb lattice's LX, LY (cells) and whether it is 12 x 12; the patch layout's kind (0 none,
 * 1 square, 2 honeycomb, 3 triangular, 4 simple cubic: side L of the L x L x L box, PX = PY = 2 for its 2 x 2 x 2 patches), side, PX, PY and wavefronts per slice (1 without one); the GRID layout's lanes GX, GY; the honeycomb grid
 * form's registers per lane (2, 4, 8; 0); whether the model's hopping is one (cosh, sinh); the site -> bond map uploaded (0 none, 1 small square,
 * 2 patch).  Reads ELPH_PG_MW as elph_create does. */
int elph_bench_lattice_shape(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht, const double *sinht,
                             int *out);

/* The plan of the workgroup-resident CG launch (cg_wg.hip: WgPlan) that a handle created from this bond table at Ltau = ltau makes for nrhs
 * right-hand sides (needs no device; reads the ELPH_*WG* switches as a solve does).  world = 0: the un-sharded solve; world > 0: one rank of a
 * sharded solve over that many ranks (the table is the rank's slab).  out[9] = usable; the form (0 lane program, 1 16 x 16 DPP, 2 12 x 12
 * honeycomb DPP, 4 8 x 8 DPP, 5 GRID, 6 HGRID, 7 triangular GRID); the kernel's sites per lane; T, W, G; bytes of dynamic LDS; whether the cost
 * rule takes the resident kernel; whether the launch table holds the plan's kernel. */
int elph_bench_wg_plan(int kind, int64_t nsites, int64_t ltau, int64_t nbonds, const int64_t *neighbor_table, const double *cosht,
                       const double *sinht, int nrhs, int world, int *out);

/* The plan of one tau-axis transform (dft_mfma.hip: elph_plan_dft) of nvec vectors of N columns on a time axis of ltau slices (needs no device;
 * reads ELPH_DFT_MFMA, ELPH_DFT_R2, ELPH_FUSE_XR, ELPH_FUSE_PX and ELPH_DFT_BIG_BLOCKED as a transform does).  which: 0 twisted, 1 plain;
 * nrz_slots: the r.z partial slots offered by an inverse that has to deliver them, else 0.  out[10] = the form (0 scalar tables, 1 one tile per
 * wave, 2 direct matrix-core, 3 / 4 even/odd split in registers / with its W panel in LDS, 5 / 6 / 7 long axis: one row per wave / blocked /
 * direct); the reduction tiles and row groups of its table; bytes of dynamic LDS; the r.z slots it fills; whether the residual update, the
 * p/x-update and the order-1 fold may ride on it; whether nrz_slots is too few (the transform returns ELPH_E_STATE); the form
 * fourier_accelerate runs this direction in (plain: the matrix cores only when both directions take them; twisted: the form itself).
 * elph_bench_dft_info: the same from the record a handle made at elph_create. */
int elph_bench_dft_plan(int64_t ltau, int which, int inverse, int N, int nvec, int nrz_slots, int *out);
int elph_bench_dft_info(elph_handle h, int which, int inverse, int N, int nvec, int nrz_slots, int *out);

/* What setup!(P) plans for nch chains at Ltau = ltau over nsteps successive steps of bounds (kpm_host.cpp: elph_kpm_plan; needs no device).
 * e_bounds: [nsteps][nch][2] (e_min, e_max); uploaded[s] = 1 when step s uploads the tables.  After the last step: active[nch]; lam[nch][4] =
 * lam_lo, lam_hi and the uploaded (lam_avg, lam_mag); the tables order, wsched [nch][Lo2] and coff [nch][Lo2+1]; c0 [nch][Lo2][2] the leading
 * coefficient of each schedule entry; fold [nch][Lo2][2]; the coefficients (complex interleaved) into coeff, which holds coeff_cap doubles.
 * *ncoeff = the doubles they take (ELPH_E_ARG when coeff is given and too small).  Any output may be NULL. */
int elph_bench_kpm_plan(int64_t ltau, double buf, double c1, double c2, int nch, int nsteps, const double *e_bounds, int *uploaded,
                        int *active, double *lam, int *order, int *coff, int *wsched, double *c0, double *fold, double *coeff,
                        int64_t coeff_cap, int64_t *ncoeff);

/* The Hessenberg QR iteration of the Arnoldi bounds alone: out[k] = the largest real part of the eigenvalues of the k-th of nmat upper-Hessenberg
 * matrices A ([nmat][n x n], column-major, host memory), +inf where the iteration did not converge.  where = 0: the host's elph_hess_eigvals
 * (kpm_host.cpp; h may be NULL, needs no device); where = 1: the device's hess_max_real (kpm_dev.hip) as k_kpm_bounds calls it, one wavefront per
 * matrix, the matrix in LDS — ELPH_E_UNSUPPORTED beyond n = 64. */
int elph_bench_hess_max_real(elph_handle h, int where, int nmat, int n, const double *A, double *out);
/* The raw Arnoldi bounds of every resident chain, e_out[nch][2] = (e_min, e_max), as setup!(P) computes them before it plans (no margin, no
 * acceptance window, no retention): where = 0 the host branch (kpm_host.cpp), 1 the device kernel (kpm_dev.hip) with the host as its fallback where
 * the kernel refuses the shape, 2 whichever setup!(P) itself would take (chain count, ELPH_KPM_HOST / ELPH_KPM_DEVICE).  *ran_on_device = 1 when
 * the device kernel produced them.  b_max, b_min: [nch][N] start vectors.  Needs elph_kpm_create and a model update, like elph_kpm_setup_chains;
 * leaves the planned expansions alone. */
int elph_bench_kpm_bounds(elph_handle h, int where, const double *b_max, const double *b_min, double *e_out, int *ran_on_device);

/* Whether an un-preconditioned solve of nrhs right-hand sides FROM x = 0 on this handle runs in the slab form (slabs.hip: lattices beyond
 * 320 sites as slabs of rows on the same device, the resident kernel per slab, one launch) and its shape. */
int elph_bench_slabs_info(elph_handle h, int nrhs, int *usable, int *slabs, int *sites_per_slab, int *own_sites);

/* The estimator's noise generator alone (greens_noise.hip): fills a device buffer of the hook's own with nvec vectors of ndim standard normals of
 * batch `seed`, `reps` times back to back between two HIP events; *ms_total = the event time.  mapping: 0 = Box-Muller pair k on thread k (the
 * mapping of the HMC state's generator), 1 = site fastest across the lanes (even Ltau; ELPH_E_UNSUPPORTED otherwise), -1 = what the estimator's
 * device-drawn update launches.  out (may be NULL): elements [out_first, out_first + out_count) of the buffer as it lies on the device, layout S
 * [vec][tau][site].  Needs no estimator. */
int elph_bench_greens_noise(elph_handle h, int mapping, int64_t nvec, uint64_t seed, int reps, double *ms_total, int64_t out_first,
                            int64_t out_count, double *out);

/* The two-stage pair solve of a BiCGStab / GMRES handle alone (msolve.hip: elph_i_msolve_pair) on the nrhs right-hand sides the last force or
 * action evaluation left on the device (work.b: Λϕ± of every chain; nrhs at most what that evaluation solved), with the handle's tolerance:
 * zero_start = 1 as the callers run it (the first mat-vec of every stage skipped on the promise of a zero guess), 0 with that mat-vec on the
 * zeroed guess — the same bits.  *ms_total = the host's time over `reps` pair solves, synchronised before and after; iters: [2 stages][nrhs]
 * of the last one (may be NULL). */
int elph_bench_msolve_pair(elph_handle h, int nrhs, int use_precond, int zero_start, int reps, double *ms_total, int64_t *iters);

/* The launch shape of the one-sided KPM apply and of the BiCGStab / GMRES vector kernels on this handle (needs no set-up): out[5] = the threads per
 * workgroup of k_kpm_cheb_side, its sites per thread NPL (the template argument), whether the bond program rides in LDS (lds_tables), whether
 * elph_kpm_apply_side and a preconditioned elph_msolve refuse the lattice (NPL beyond 6), and the threads per workgroup of the solver kernels
 * (msolve.hip: ms_block, 64 per wave). */
int elph_bench_kpm_side_info(elph_handle h, int *out);

/* the sharded solve (shard.hip): exactly `iters` iterations (no stop test); *ms = HIP-event time of this rank's launch.  b_slab may
 * be NULL (keeps the right-hand side of the previous call).  Needs elph_shard_prepare + barrier like a solve. */
int elph_shard_iterate(elph_handle h, const double *b_slab, int64_t iters, double *ms);

#ifdef __cplusplus
}
#endif
