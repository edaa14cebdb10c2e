// currcorr.hip — CurrentCurrent of the Holstein model accumulated on the device, for one configuration or for EVERY chain resident in
// the handle at once (DESIGN.md "CurrentCurrent of the Holstein model"):
//   measure_CurrentCurrent!(holstein)   Measurements.jl:1790-2098     the bodies of currcorr_dev.h, shared with the SSH unit
//   translational_average!              Utilities.jl:49-60
// The reference is mirrored as it executes.  Read term by term the method builds the eight fields A0 .. A7 per bond definition of the
// SSH method (:2100-2384; formulas, notation and the four δ terms in ssh_bondcorr.hip's header), the same eight translation averages
// with the same signs and operand order — the fourth term subtracted (:1929), the sixth averaging the n″ field against the n′ field
// (:1956-1962), the b == c δ term reading M⁻¹r₁[:, b] (:2050) — and the same τ = β slice (:2083-2093).  It differs in the hopping that
// weights every factor: t = reshaped(model.t, (L₁, L₂, L₃, n_def)) (:1835), static, in definition order (bond = cell + N_cells (n − 1):
// assign_t! appends, initialize_model! never permutes it), applied inside `for τ in Lₜ` (:1868-1871 and after every other product, the
// δ terms' :2014-2017 included) — a loop over the NUMBER Lₜ, which visits the last time slice alone.  So the weight of definition n is 1
// on slices 1 .. Lτ − 1 and t[cell, n] on slice Lτ, in every field and δ term: the policy CcLastSlice of currcorr_dev.h.  With t = 1
// everywhere this is the physical correlation; otherwise it is what the reference computes, and what this unit computes.
// The b == c displacement l = r″ is reduced mod L, as in the SSH units (unreduced the reference's index throws).
//
// The method reads the vectors R and M⁻¹R and nothing setup! makes, so this unit reads ElphGreensView::R / X in place (as
// density_moments.hip and snapshots.hip do) and never runs the estimator's pipeline: the estimator's own tables are not touched.  The
// weights depend on neither the field nor the chain: one table [n_def N_cells], uploaded at create.
//
// Layouts are ssh_bondcorr.hip's.  Vector v (0-based) of chain c is row v nchains + c of the estimator, so the v-th vectors of all
// chains are one block [chain][ndim]; nchains = 1 is the single configuration.  Every buffer carries the chain between the definition
// (or listed pair) and the time axis:
//   f  [NCC][ndef][chain][L][nc]     nu [NCC][ndef][chain][Lh][nc]     Y [pair][chain][Lh][nc]     B [pair][chain][L][nc]
//   part [pair][chain][L][NDELTA]    dl [pair][chain][NDELTA]
// and the accumulator is ONE allocation [chain][CurrentCurrent], a chain's block laid out as elph_ssh_bond_fetch's CurrentCurrent.  The
// folds of one accumulate add into a second such block, zeroed first, which one last kernel adds to the accumulator (k_cur_add): what
// an accumulate adds does not depend on what the accumulator held, so the same accumulate twice is exactly twice the first.  The
// chain is the last grid axis of every kernel, so the launches of one accumulate depend on the vectors per chain and on the request,
// not on the number of chains.  Reductions as in ssh_bondcorr.hip: a thread walks its cells in index order, the lanes of a wave fold by
// halves, the waves are added in index order through LDS, one partial per time slice, the slices added in slice order; everything else
// is one thread's sum in index order.  No floating-point atomics.  A workgroup reads one chain's vectors only, so chain c's bits depend
// on chain c's vectors alone and equal those of a single-configuration handle holding them.  State: the handle's slot `current`.

#include <vector>

#include "currcorr_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int NWAVE = MEAS_NWAVE;
const CorrWords WORDS = {"Holstein CurrentCurrent", "bond", "with no pair of bonds"};
const char *const NAMES[1] = {"CurrentCurrent"};
constexpr long long GRID_YZ_MAX = 65535;

struct CurrentState {
    int nchains = 1;
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, ndef = 0;
    CorrPlan<1> cr;                 // ONE chain's plan; cr.acc: [chain][CurrentCurrent]; cr.req is bound to chain 0 of `call`
    double *call = nullptr;         // [chain][CurrentCurrent] the sum over the pairs of vectors of the accumulate in progress
    int *defs = nullptr;            // [ndef][DEFW]
    double *t0 = nullptr;           // [ndef nc] model.t, bond = cell + nc n
    double *f = nullptr;            // [NCC][ndef][chain][L][nc] the fields of one pair of vectors
    double2 *nu = nullptr;          // [NCC][ndef][chain][Lh][nc] their half spectra, then their cell-axis DFTs in place
    double2 *Y = nullptr;           // [np][chain][Lh][nc] per-frequency correlations of the listed pairs
    double *B = nullptr;            // [np][chain][L][nc]
    double *part = nullptr;         // [np][chain][L][NDELTA] one partial per time slice
    double *dl = nullptr;           // [np][chain][NDELTA] the δ terms of one pair of vectors, signed and normalised
};

CurrentState *cur_of(elph_handle_s *h) { return (CurrentState *)h->current; }

int need_state(elph_handle_s *h) { return corr_need(h->current, "elph_current_create"); }

// ---- the kernels: the bodies of currcorr_dev.h under the last-slice weight, the chain the last grid axis; per: L nc, slice: Lh nc

// One thread per (cell, τ, definition) of chain blockIdx.y.  v: chain 0's vectors, chain c's c L N further on.
__global__ void __launch_bounds__(TPB) k_cur_fields(double *__restrict__ f, ElphGreensPair v, const int *__restrict__ defs,
                                                    const double *__restrict__ t0, int N, int L, int ns, int L1, int L2, int L3, int ndef,
                                                    int nchains) {
    const size_t ch = blockIdx.y, o = ch * L * N, per = (size_t)L * (L1 * L2 * L3);
    cc_fields_at(f + ch * per, v.X1 + o, v.X2 + o, v.R1 + o, v.R2 + o, defs, CcLastSlice{t0, L}, N, L, ns, L1, L2, L3, ndef,
                 (long long)blockIdx.x * TPB + threadIdx.x, (size_t)nchains * per);
}

// One workgroup per (frequency, listed pair, chain).  LDS: 2 buffers of nc complex.
__global__ void __launch_bounds__(TPB) k_cur_correlate(double2 *__restrict__ Y, const double2 *__restrict__ nu, CcReq rq, int Lh, int ndef, int L1,
                                                       int L2, int L3, const double2 *__restrict__ tw, double norm, int nchains) {
    extern __shared__ double2 lds[];
    const int nc = L1 * L2 * L3;
    const size_t ch = blockIdx.z, slice = (size_t)Lh * nc;
    cc_correlate_slice(Y + (((size_t)blockIdx.y * nchains + ch) * Lh + blockIdx.x) * nc, nu + ch * slice, rq, blockIdx.y, blockIdx.x, ndef, L1, L2, L3, tw,
                       norm, (size_t)nchains * slice, lds);
}

// One workgroup per (time slice, listed pair, chain).  X1, R1: vector 1 of chain 0's pair.
__global__ void __launch_bounds__(TPB) k_cur_delta(double *__restrict__ part, CcReq rq, const double *__restrict__ X1, const double *__restrict__ R1,
                                                   const int *__restrict__ defs, const double *__restrict__ t0, int N, int L, int ns, int L1, int L2,
                                                   int L3, int nchains) {
    __shared__ double red[NWAVE];
    const size_t ch = blockIdx.z, o = ch * L * N;
    cc_delta_slice(part + ((size_t)blockIdx.y * nchains + ch) * L * NDELTA, rq, blockIdx.y, blockIdx.x, X1 + o, R1 + o, defs, CcLastSlice{t0, L}, N, ns,
                   L1, L2, L3, red);
}

// One thread per (δ term, chain, listed pair): dl and part are [pair][chain] blocks, np nchains of them.
__global__ void __launch_bounds__(TPB) k_cur_delta_finish(double *__restrict__ dl, const double *__restrict__ part, int np, int nchains, int L, int nc) {
    cc_delta_finish_at(dl, part, np * nchains, L, nc, blockIdx.x * TPB + threadIdx.x);
}

// One thread per (τ, cell, listed pair) of chain blockIdx.z.  block: doubles of a chain's accumulator.
__global__ void __launch_bounds__(TPB) k_cur_fold(CcReq rq, const double *__restrict__ B, const double *__restrict__ dl, const int *__restrict__ defs,
                                                  int L, int L1, int L2, int L3, int nchains, size_t block) {
    const size_t ch = blockIdx.z, per = (size_t)L * (L1 * L2 * L3);
    cc_fold_at(rq, (long long)blockIdx.x * TPB + threadIdx.x, B + ch * per, dl + ch * NDELTA, defs, L, L1, L2, L3, (size_t)nchains * per,
               (size_t)nchains * NDELTA, ch * block);
}

// acc += call, one thread per element of [chain][CurrentCurrent]: an accumulate adds ITS total once, so what it adds does not depend
// on what the accumulator held, and the same accumulate twice is exactly twice the first.
__global__ void __launch_bounds__(TPB) k_cur_add(double *__restrict__ acc, const double *__restrict__ call, size_t n) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) acc[i] += call[i];
}

// CurrentCurrent of one pair of vectors v of every chain into the call's sum
int accumulate_pair(elph_handle_s *h, CurrentState *m, const ElphGreensView &g, const ElphGreensPair &v) {
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = m->ns, nc = m->nc, ndef = m->ndef, np = m->cr.req.np[0], nch = m->nchains;
    const size_t shm = bc_lds_bytes(nc);
    const long long nfld = (long long)L * nc * ndef;
    const double norm = 1.0 / ((double)L * (double)nc * (double)nc);   // 1/(L Nc)² in all: the other 1/L is in the inverse τ table
    hipLaunchKernelGGL(k_cur_fields, dim3((unsigned)((nfld + TPB - 1) / TPB), (unsigned)nch), dim3(TPB), 0, h->stream, m->f, v, m->defs, m->t0, N, L, ns,
                       m->L1, m->L2, m->L3, ndef, nch);
    RC(elph_launch_check("k_cur_fields"));
    RC(elph_dft_fwd_plain(h, m->nu, m->f, nc, NCC * ndef * nch));
    hipLaunchKernelGGL(k_bc_spatial_fwd, dim3((unsigned)Lh, (unsigned)(NCC * ndef * nch)), dim3(TPB), shm, h->stream, m->nu, Lh, m->L1, m->L2, m->L3,
                       g.tw);
    RC(elph_launch_check("k_bc_spatial_fwd(Holstein CurrentCurrent)"));
    hipLaunchKernelGGL(k_cur_correlate, dim3((unsigned)Lh, (unsigned)np, (unsigned)nch), dim3(TPB), shm, h->stream, m->Y, m->nu, m->cr.req, Lh, ndef,
                       m->L1, m->L2, m->L3, g.tw, norm, nch);
    RC(elph_launch_check("k_cur_correlate"));
    RC(elph_dft_inv_plain(h, m->B, m->Y, nc, np * nch));
    hipLaunchKernelGGL(k_cur_delta, dim3((unsigned)L, (unsigned)np, (unsigned)nch), dim3(TPB), 0, h->stream, m->part, m->cr.req, v.X1, v.R1, m->defs,
                       m->t0, N, L, ns, m->L1, m->L2, m->L3, nch);
    RC(elph_launch_check("k_cur_delta"));
    hipLaunchKernelGGL(k_cur_delta_finish, dim3((unsigned)(((long long)np * nch * NDELTA + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->dl, m->part, np,
                       nch, L, nc);
    RC(elph_launch_check("k_cur_delta_finish"));
    hipLaunchKernelGGL(k_cur_fold, dim3((unsigned)((m->cr.fold_max + TPB - 1) / TPB), 1, (unsigned)nch), dim3(TPB), 0, h->stream, m->cr.req, m->B, m->dl,
                       m->defs, L, m->L1, m->L2, m->L3, nch, m->cr.total);
    return elph_launch_check("k_cur_fold");
}

// Everything one accumulate queues on the handle's stream; the caller synchronises, whatever this returns.
int accumulate_launches(elph_handle_s *h, CurrentState *m, const ElphGreensView &g) {
    const int nch = m->nchains, nvc = g.nv / nch;
    const size_t blk = (size_t)nch * (size_t)h->ndim;                  // the v-th vectors of all chains
    const size_t n = (size_t)nch * m->cr.total;
    HIPCHK(hipMemsetAsync(m->call, 0, std::max<size_t>(n, 1) * sizeof(double), h->stream));
    for (int i = 0; i < nvc - 1; ++i)
        for (int j = i + 1; j < nvc; ++j) {                            // pairs of a chain's vectors; every launch serves all chains
            const ElphGreensPair v = {g.X + i * blk, g.X + j * blk, g.R + i * blk, g.R + j * blk};
            RC(accumulate_pair(h, m, g, v));
        }
    hipLaunchKernelGGL(k_cur_add, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, m->cr.acc, m->call, n);
    return elph_launch_check("k_cur_add");
}

}  // namespace

void elph_current_free(elph_handle_s *h) {
    CurrentState *m = cur_of(h);
    if (!m) return;
    corr_free({m->cr.pairs, m->cr.acc, m->call, m->defs, m->t0, m->f, m->nu, m->Y, m->B, m->part, m->dl});
    delete m;
    h->current = nullptr;
}

extern "C" int elph_current_create(elph_handle h, int nchains, int n_def, const int *o1, const int *o2, const int *v, int64_t Nbonds,
                                   const double *t, int measure, int time_dependent, int npairs, const int *pairs) {
    CHECK_H(h);
    elph_current_free(h);
    RC(corr_refuse_model(h, WORDS.prefix, ELPH_MODEL_HOLSTEIN));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle", WORDS.prefix, nchains, h->nchains);
        return ELPH_E_ARG;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    RC(bc_check(WORDS, g, n_def, o1, o2, v, &measure, &time_dependent, &npairs));
    std::vector<int> defs;
    RC(bc_defs_table(defs, WORDS, g, n_def, o1, o2, v));
    const int L = (int)h->L, Lh = L / 2 + 1, nc = g.nc;
    CorrPlan<1> plan;                                  // request bookkeeping before anything is allocated
    RC(corr_plan(plan, WORDS, NAMES, &measure, &time_dependent, &npairs, pairs, n_def, L, nc, 0));
    if (Nbonds < 0 || Nbonds != h->nb || !t) {
        elph_set_error("%s: %lld bonds (the handle has %lld), or a null hopping array", WORDS.prefix, (long long)Nbonds, (long long)h->nb);
        return ELPH_E_ARG;
    }
    RC(cc_check_bond_count(WORDS.prefix, n_def, nc, Nbonds));
    // the chain multiplies the slices of the cell-axis DFT (grid y) and the right-hand sides of the tau-DFTs (grid z)
    const int np = plan.req.np[0];
    if ((long long)NCC * n_def * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %d fields x %d bond definitions x %d chains = %lld slices exceed the grid's %lld", WORDS.prefix, NCC, n_def, nchains,
                       (long long)NCC * n_def * nchains, GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    if ((long long)np * nchains > GRID_YZ_MAX) {
        elph_set_error("%s: %d listed pairs x %d chains = %lld transforms exceed the grid's %lld", WORDS.prefix, np, nchains, (long long)np * nchains,
                       GRID_YZ_MAX);
        return ELPH_E_UNSUPPORTED;
    }
    CurrentState *m = new CurrentState;
    h->current = m;
    m->nchains = nchains; m->ns = g.ns; m->L1 = g.L1; m->L2 = g.L2; m->L3 = g.L3; m->nc = nc; m->ndef = n_def;
    m->cr = plan;
    CorrFirstError ok;
    if (np) {
        const size_t nch = (size_t)nchains, nb = (size_t)n_def * nc, nf = nch * NCC * n_def, nP = nch * np;
        const bool allocated = ok(corr_alloc(&m->cr.pairs, m->cr.prs.size())) && ok(corr_alloc(&m->cr.acc, nch * m->cr.total)) &&
            ok(corr_alloc(&m->call, nch * m->cr.total)) && ok(corr_alloc(&m->defs, defs.size())) && ok(corr_alloc(&m->t0, nb)) && ok(corr_alloc(&m->f, nf * L * nc)) &&
            ok(corr_alloc(&m->nu, nf * Lh * nc)) && ok(corr_alloc(&m->Y, nP * Lh * nc)) && ok(corr_alloc(&m->B, nP * L * nc)) &&
            ok(corr_alloc(&m->part, nP * L * NDELTA)) && ok(corr_alloc(&m->dl, nP * NDELTA));
        if (allocated && ok(corr_up(m->defs, defs.data(), defs.size() * sizeof(int))) && ok(corr_up(m->t0, t, nb * sizeof(double))))
            ok(corr_upload(m->cr, WORDS.prefix));      // the pairs; zeroes chain 0's block
        m->cr.req.acc[0] = m->call;                    // the fold adds into the call's sum
        if (ok.rc == ELPH_OK && hipMemset(m->cr.acc, 0, std::max<size_t>(nch * m->cr.total, 1) * sizeof(double)) != hipSuccess) {
            elph_set_error("%s: hipMemset failed", WORDS.prefix);
            ok(ELPH_E_HIP);
        }
        if (ok.rc == ELPH_OK && ok(bc_allow_lds(k_bc_spatial_fwd, WORDS, nc))) ok(bc_allow_lds(k_cur_correlate, WORDS, nc));
    }
    if (ok.rc != ELPH_OK) elph_current_free(h);
    return ok.rc;
}

extern "C" int elph_current_accumulate(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    CurrentState *m = cur_of(h);
    const int nch = m->nchains;
    if (h->nchains != nch) {
        elph_set_error("%s: created for %d chains, %d are resident in this handle now", WORDS.prefix, nch, h->nchains);
        return ELPH_E_STATE;
    }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (g.nv % nch) {
        elph_set_error("%s: the estimator's %d vectors are not a multiple of the %d resident chains", WORDS.prefix, g.nv, nch);
        return ELPH_E_STATE;
    }
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    if (!m->cr.req.np[0]) return ELPH_OK;
    const int rc = accumulate_launches(h, m, g);
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc == ELPH_OK && e != hipSuccess) { elph_set_error("%s: hipStreamSynchronize -> %s", WORDS.prefix, hipGetErrorString(e)); return ELPH_E_HIP; }
    return rc;
}

extern "C" int elph_current_fetch(elph_handle h, int chain, double *CurrentCurrent) {
    CHECK_H(h);
    RC(need_state(h));
    const CurrentState *m = cur_of(h);
    if (chain < 0 || chain >= m->nchains) { elph_set_error("%s: chain %d outside 0..%d", WORDS.prefix, chain, m->nchains - 1); return ELPH_E_ARG; }
    if (!m->cr.req.np[0]) return ELPH_OK;
    CorrPlan<1> one = m->cr;                           // the chain's block, laid out as the plan says
    one.acc = m->cr.acc + (size_t)chain * m->cr.total;
    std::vector<double> host;
    double *outs[1] = {CurrentCurrent};
    return corr_fetch(h, one, host, outs);
}

extern "C" int elph_current_reset(elph_handle h) {
    CHECK_H(h);
    RC(need_state(h));
    const CurrentState *m = cur_of(h);
    if (m->cr.req.np[0]) HIPCHK(hipMemsetAsync(m->cr.acc, 0, std::max<size_t>((size_t)m->nchains * m->cr.total, 1) * sizeof(double), h->stream));
    return ELPH_OK;
}
