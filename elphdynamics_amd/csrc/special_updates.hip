// special_updates.hip — the special updates (SpecialUpdates.jl:97-366) on the device-resident field of the HMC state (hmc_dev.h), two routes:
//   elph_hmc_special_move[_chains]    one proposed move per chain, columns and random numbers from the caller, decided on the host;
//   elph_hmc_special_update_chains    special_update! itself: nmoves moves of every chain in one call — the sites / bonds / phonon pairs drawn on
//                                     the device from the handle's generator, decided there, nothing but the small per-move results comes back.
// Both move all chains in one launch of k_sp_colop.  The two decisions stay apart: tests/test_gpu_special_updates.py checks one with the other.

#include <cstring>
#include "hmc_dev.h"

using namespace hmc;

namespace {

// pick(u, n) = min(floor(u n), n − 1): u01 can round to 1.0
__device__ __forceinline__ int sp_pick(double u, int n) {
    const int k = (int)floor(u * (double)n);
    return k < n - 1 ? k : n - 1;
}

// the draw of a reflection (:113: one phonon column) or of a Holstein swap (:248-258: the two sites of one bond): chain c uses uniform 2c
__global__ void __launch_bounds__(TPB) k_sp_draw(int *__restrict__ ci, int *__restrict__ cj, uint64_t seed, int nch, int kind, int nf,
                                                 int nb, const int *__restrict__ bi, const int *__restrict__ bj) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= nch) return;
    const double u0 = u01(seed, 2 * (uint64_t)c);
    if (kind == 0) {
        const int i = sp_pick(u0, nf);
        ci[c] = i; cj[c] = i;
    } else {
        const int b = sp_pick(u0, nb);
        ci[c] = bi[b]; cj[c] = bj[b];
    }
}

// the draw of an SSH swap (:324-328), first half: i = pick(u0, Nph) of chain blockIdx.y, and for every column q whether its world line is
// NOT ≈ that of i (Julia's isapprox: ‖xᵢ − x_q‖ ≤ √eps max(‖xᵢ‖, ‖x_q‖)).  A lane owns a column and walks τ: the loads of a slice are
// contiguous over the lanes, xᵢ(τ) is one address for the whole workgroup, every sum runs in the order of τ
__global__ void __launch_bounds__(TPB) k_sp_differs(int *__restrict__ differs, const double *__restrict__ x, uint64_t seed, int nf, int L) {
    const int c = blockIdx.y, q = blockIdx.x * TPB + threadIdx.x;
    if (q >= nf) return;
    const int i = sp_pick(u01(seed, 2 * (uint64_t)c), nf);
    const double *xc = x + (size_t)c * (size_t)nf * (size_t)L;
    double ni = 0.0, nq = 0.0, d = 0.0;
    for (int t = 0; t < L; ++t) {
        const double a = xc[(size_t)t * nf + i], b = xc[(size_t)t * nf + q];
        ni += a * a;
        nq += b * b;
        d += (a - b) * (a - b);
    }
    differs[(size_t)c * nf + q] = !(sqrt(d) <= 1.4901161193847656e-08 * fmax(sqrt(ni), sqrt(nq)));
}

// second half, one workgroup per chain: D = the flagged columns in increasing order, j = D[pick(u1, |D|)], j = i when D is empty (every
// world line ≈ xᵢ: the move is the identity).  A thread counts a contiguous segment of columns; the prefix over the threads is exact
__global__ void __launch_bounds__(TPB) k_sp_select(int *__restrict__ ci, int *__restrict__ cj, const int *__restrict__ differs, uint64_t seed,
                                                   int nf) {
    __shared__ int cnt[TPB];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int *f = differs + (size_t)c * nf;
    const int seg = (nf + TPB - 1) / TPB;
    const int lo = min(tid * seg, nf), hi = min(lo + seg, nf);
    int own = 0;
    for (int q = lo; q < hi; ++q) own += f[q];
    cnt[tid] = own;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < TPB; ++k) {
        const int v = cnt[k];
        total += v;
        if (k < tid) before += v;
    }
    const int i = sp_pick(u01(seed, 2 * (uint64_t)c), nf);
    if (tid == 0) {
        ci[c] = i;
        if (total == 0) cj[c] = i;
    }
    if (total == 0) return;
    const int r = sp_pick(u01(seed, 2 * (uint64_t)c + 1), total);
    if (r < before || r >= before + own) return;
    int k = before;
    for (int q = lo; q < hi; ++q) {
        if (!f[q]) continue;
        if (k == r) { cj[c] = q; return; }
        ++k;
    }
}

// The move of every chain in one launch (blockIdx.y = chain): reflect column ci[c] (kind 0) or swap columns ci[c], cj[c] (kind 1) of the
// tau-major field x[c][t][column]; mask: only the chains whose entry is non-zero (the undo of the rejected ones), NULL: all.  Both moves
// are involutions
__global__ void __launch_bounds__(TPB) k_sp_colop(double *__restrict__ x, int nf, int L, int kind, const int *__restrict__ ci,
                                                  const int *__restrict__ cj, const int *__restrict__ mask) {
    const int c = blockIdx.y, t = blockIdx.x * TPB + threadIdx.x;
    if (t >= L || (mask && !mask[c])) return;
    double *row = x + ((size_t)c * (size_t)L + (size_t)t) * (size_t)nf;
    const int i = ci[c], j = cj[c];
    if (kind == 0) row[i] = -row[i];
    else if (i != j) { const double a = row[i]; row[i] = row[j]; row[j] = a; }
}

// The Metropolis test of one move, a thread per chain.  part: [6][nch][L] per-slice partials of R₊², R₋², Λϕ₊·O⁻¹Λϕ₊, Λϕ₋·O⁻¹Λϕ₋,
// S_b/Δτ before and S_b/Δτ after, each summed here in the order of the slices (the order sum_rows adds them in on the host);
// u = uniform c of batch seed_u.  Writes the undo mask and the move's row of the outputs
__global__ void __launch_bounds__(ELPH_WAVE) k_sp_accept(const double *__restrict__ part, int nch, int L, double dtau, uint64_t seed_u,
                                                         const int *__restrict__ flag, const int *__restrict__ ci, const int *__restrict__ cj,
                                                         int *__restrict__ undo, int *__restrict__ acc, long long *__restrict__ out_i,
                                                         long long *__restrict__ out_j, double *__restrict__ out_S0, double *__restrict__ out_S1) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * ELPH_WAVE + threadIdx.x;
    if (c >= nch) return;
    double s[6];
    for (int k = 0; k < 6; ++k) {
        const double *p = part + ((size_t)k * nch + c) * (size_t)L;
        double a = 0.0;
        for (int q = 0; q < L; ++q) a += p[q];
        s[k] = a;
    }
    const double sb0 = dtau * s[4], sb1 = dtau * s[5];
    const double S0 = s[0] / 2 + s[1] / 2 + sb0, S1 = s[2] / 2 + s[3] / 2 + sb1;
    const double e = exp(-(S1 - S0)), P = (1.0 < e) ? 1.0 : e;
    const int a = (u01(seed_u, (uint64_t)c) < P && flag[c] == 0) ? 1 : 0;
    acc[c] = a;
    undo[c] = !a;
    out_i[c] = ci[c];
    out_j[c] = cj[c];
    out_S0[c] = S0;
    out_S1[c] = S1;
}

// the device scratch of the special updates, carved from one allocation that only grows
struct SpScratch {
    double *part;                          // [6][nch][L]
    int *differs;                          // [nch][nf] (SSH swap)
    int *ci, *cj, *undo, *flag;            // [nch]
    int *acc;                              // [nmoves][nch]
    long long *out_i, *out_j;              // [nmoves][nch]
    double *S0, *S1;                       // [nmoves][nch]
};

int special_scratch(HmcState *st, int L, size_t nmoves, bool ssh_swap, SpScratch *S) {
    const size_t nch = (size_t)st->nch, rows = nmoves * nch;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_part = take(6 * nch * (size_t)L * sizeof(double)), o_dif = take(ssh_swap ? nch * (size_t)st->nf * sizeof(int) : 0);
    const size_t o_ci = take(nch * sizeof(int)), o_cj = take(nch * sizeof(int)), o_undo = take(nch * sizeof(int)), o_flag = take(nch * sizeof(int));
    const size_t o_acc = take(rows * sizeof(int)), o_i = take(rows * sizeof(long long)), o_j = take(rows * sizeof(long long));
    const size_t o_S0 = take(rows * sizeof(double)), o_S1 = take(rows * sizeof(double));
    if (off > st->sp_cap) {
        if (st->sp_buf) { HIPCHK(hipFree(st->sp_buf)); st->sp_buf = nullptr; st->sp_cap = 0; }
        HIPCHK(hipMalloc(&st->sp_buf, off));
        st->sp_cap = off;
    }
    char *b = static_cast<char *>(st->sp_buf);
    S->part = reinterpret_cast<double *>(b + o_part);
    S->differs = reinterpret_cast<int *>(b + o_dif);
    S->ci = reinterpret_cast<int *>(b + o_ci); S->cj = reinterpret_cast<int *>(b + o_cj);
    S->undo = reinterpret_cast<int *>(b + o_undo); S->flag = reinterpret_cast<int *>(b + o_flag);
    S->acc = reinterpret_cast<int *>(b + o_acc);
    S->out_i = reinterpret_cast<long long *>(b + o_i); S->out_j = reinterpret_cast<long long *>(b + o_j);
    S->S0 = reinterpret_cast<double *>(b + o_S0); S->S1 = reinterpret_cast<double *>(b + o_S1);
    return ELPH_OK;
}

// the move (or, with a mask, its undo) of the chains on the columns in S, and update_model! after it
int move_chains(elph_handle_s *h, HmcState *st, const SpScratch &S, int kind, const int *mask) {
    hipLaunchKernelGGL(k_sp_colop, dim3(nblk(h->L), (unsigned)st->nch), dim3(TPB), 0, h->stream, st->x, st->nf, (int)h->L, kind,
                       (const int *)S.ci, (const int *)S.cj, mask);
    RC(chk("k_sp_colop"));
    return update_model(h, st);
}

int refuse_shared(const HmcState *st) {
    if (!st->shared) return ELPH_OK;
    elph_set_error("special moves on shared fields: the reference's swap leaves the fields unequal and then stops in update_model!");
    return ELPH_E_UNSUPPORTED;
}

}  // namespace

// The body of the loops of special_update! (SpecialUpdates.jl:103-136 reflection, :205-275 swap) for every chain of an HMC state:
//   S₀ = refresh_ϕ!(hmc, model, sample_R = true) — Rp, Rm are the fresh R± (HMC.jl:665-692), S₀ = (R₊² + R₋²)/2 + S_b;
//   the move (kind 0: x_col(τ) → −x_col(τ) on column col_i; kind 1: columns col_i, col_j exchange their world lines; 0-based
//   phonon columns = sites for Holstein), update_model!, calc_O⁻¹Λϕ!(…, 2.0), S₁ = calc_S;
//   accepted iff u < min(1, e^{−(S₁−S₀)}) and flag == 0, otherwise the move is undone and update_model! runs again.
// kpm_randn: b_max, b_min [2][nchains][nsites] of the one setup!(P) (NULL without preconditioner).  The choice of sites / bonds
// (sample!(model.rng, …)) stays with the caller.  out: accepted, S₀, S₁, iterations, flag, [nchains] each.
extern "C" int elph_hmc_special_move_chains(elph_handle h, int kind, const int64_t *col_i, const int64_t *col_j, const double *Rp,
                                            const double *Rm, int use_precond, const double *kpm_randn, const double *u_accept,
                                            int *accepted, double *S0_out, double *S1_out, int64_t *iters_out, int *flag_out) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st, true));
    const int nch = st->nch;
    if (!accepted || !col_i || kind < 0 || kind > 1 || (kind == 1 && !col_j)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    for (int c = 0; c < nch; ++c)
        if (col_i[c] < 0 || col_i[c] >= st->nf || (kind == 1 && (col_j[c] < 0 || col_j[c] >= st->nf))) {
            elph_set_error("chain %d: column outside 0..%d", c, st->nf - 1);
            return ELPH_E_ARG;
        }
    RC(refuse_shared(st));
    RC(need_randoms(st, Rp && Rm && u_accept && (!use_precond || kpm_randn), "Rp, Rm, u_accept (kpm_randn with a preconditioner)"));
    if (use_precond && !h->kpm.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, 2 * nch));
    RC(elph_i_reserve_chains(h, nch));
    SpScratch S;
    RC(special_scratch(st, (int)h->L, 1, false, &S));
    const size_t nd = (size_t)h->ndim;
    std::vector<int> ci((size_t)nch), cj((size_t)nch), undo((size_t)nch, 0), flag((size_t)nch, 0);      // ci, cj, undo are uploaded: alive until the stream has drained
    for (int c = 0; c < nch; ++c) { ci[(size_t)c] = (int)col_i[c]; cj[(size_t)c] = (int)(kind == 1 ? col_j[c] : col_i[c]); }
    HIPCHK(hipMemcpyAsync(S.ci, ci.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(S.cj, cj.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice, h->stream));
    RC(update_model(h, st));
    RC(refresh_phi(h, st, Rp, Rm));
    std::vector<double> kpm_own, u_own;
    if (use_precond) RC(given_or_drawn(st, &kpm_randn, kpm_own, 2 * (size_t)nch * (size_t)h->N, true));
    RC(given_or_drawn(st, &u_accept, u_own, (size_t)nch, false));
    std::vector<double> rr((size_t)2 * nch), sf((size_t)2 * nch), sb0((size_t)nch), sb1((size_t)nch);
    RC(dots_host(h, st, st->R2, st->R2, (long long)nd, 2 * nch, rr.data()));
    RC(calc_Sb(h, st, sb0.data()));
    RC(move_chains(h, st, S, kind, nullptr));
    int64_t kpm_calls = 0;
    std::vector<int64_t> iters((size_t)nch, 0);
    RC(calc_OinvLphi(h, st, use_precond, 2.0, kpm_randn, &kpm_calls, iters.data(), flag.data()));
    RC(dots_host(h, st, h->work.b, h->work.x, (long long)nd, 2 * nch, sf.data()));
    RC(calc_Sb(h, st, sb1.data()));
    bool any_undo = false;
    for (int c = 0; c < nch; ++c) {
        const double S0 = rr[(size_t)c] / 2 + rr[(size_t)nch + c] / 2 + sb0[(size_t)c];
        const double S1 = sf[(size_t)c] / 2 + sf[(size_t)nch + c] / 2 + sb1[(size_t)c];
        const double e = exp(-(S1 - S0)), P = (1.0 < e) ? 1.0 : e;
        const int acc = (u_accept[c] < P && flag[(size_t)c] == 0) ? 1 : 0;
        accepted[c] = acc;
        undo[(size_t)c] = !acc;
        any_undo = any_undo || !acc;
        if (S0_out) S0_out[c] = S0;
        if (S1_out) S1_out[c] = S1;
        if (iters_out) iters_out[c] = iters[(size_t)c];
        if (flag_out) flag_out[c] = flag[(size_t)c];
    }
    if (any_undo) {
        HIPCHK(hipMemcpyAsync(S.undo, undo.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice, h->stream));
        RC(move_chains(h, st, S, kind, S.undo));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// the single chain of an HMC state created with elph_hmc_create / elph_hmc_create_ssh; u_accept < 0: drawn
extern "C" int elph_hmc_special_move(elph_handle h, int kind, int64_t col_i, int64_t col_j, const double *Rp, const double *Rm,
                                     int use_precond, const double *kpm_randn, double u_accept, int *accepted, double *S0_out,
                                     double *S1_out, int64_t *iters_out, int *flag_out) {
    CHECK_H(h);
    HmcState *st = state_of(h);
    if (!st || st->nch != 1) { elph_set_error("elph_hmc_create / elph_hmc_create_ssh (single chain) has not been called"); return ELPH_E_STATE; }
    return elph_hmc_special_move_chains(h, kind, &col_i, &col_j, Rp, Rm, use_precond, kpm_randn, u_accept >= 0.0 ? &u_accept : nullptr,
                                        accepted, S0_out, S1_out, iters_out, flag_out);
}

// special_update!(model, hmc, ru / su, P) (SpecialUpdates.jl:97-366) for every chain of the HMC state: nmoves times the body of
// elph_hmc_special_move_chains with the columns drawn here.
// Draw (chain c: u0, u1 = uniforms 2c, 2c + 1 of the batch): reflection — column pick(u0, nf) (:113); Holstein swap — the two sites of
// bond pick(u0, nbonds) of the handle's table (:248-258); SSH swap — i = pick(u0, Nph), j = D[pick(u1, |D|)] with D the columns whose
// world line is not ≈ xᵢ, j = i when there is none (:324-328, the reference's while loop without the loop).
// Launches and copies per move do not depend on the chain count; the outputs ([nmoves][nch]) are copied back once at the end.
extern "C" int elph_hmc_special_update_chains(elph_handle h, int kind, int64_t nmoves, int use_precond, int *accepted, int64_t *col_i,
                                              int64_t *col_j, double *S0_out, double *S1_out, int64_t *iters_out, int *flag_out) {
    CHECK_H(h);
    if (h->shard || h->is_slab) { elph_set_error("elph_hmc_special_update_chains: special moves on a sharded lattice are not supported"); return ELPH_E_UNSUPPORTED; }
    HmcState *st;
    RC(state_ready(h, &st));
    const int nch = st->nch, L = (int)h->L;
    if (!accepted || kind < 0 || kind > 1 || nmoves < 1 || nmoves > (int64_t)(1 << 28) / nch) { elph_set_error("bad argument (kind 0 / 1, nmoves >= 1)"); return ELPH_E_ARG; }
    RC(refuse_shared(st));
    if (!st->rng_on) { elph_set_error("elph_hmc_special_update_chains draws its moves on the device: elph_hmc_set_rng has not been called"); return ELPH_E_STATE; }
    RC(state_ready(h, &st, true));
    const bool ssh_swap = st->ssh && kind == 1;
    if (kind == 1 && !st->ssh && h->nb < 1) { elph_set_error("a Holstein swap needs a bond"); return ELPH_E_ARG; }
    if (use_precond && !h->kpm.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, 2 * nch));
    RC(elph_i_reserve_chains(h, nch));
    SpScratch S;
    RC(special_scratch(st, L, (size_t)nmoves, ssh_swap, &S));
    const size_t nd = (size_t)h->ndim, rows = (size_t)nmoves * (size_t)nch;
    double *const p_rr = S.part, *const p_sf = S.part + 2 * (size_t)nch * L, *const p_sb0 = S.part + 4 * (size_t)nch * L, *const p_sb1 = S.part + 5 * (size_t)nch * L;
    std::vector<int64_t> iters(rows, 0);
    std::vector<int> flag(rows, 0);          // lives until the stream has drained: every move uploads its row
    std::vector<double> kpm_own;
    RC(update_model(h, st));
    for (int64_t mv = 0; mv < nmoves; ++mv) {
        const size_t row = (size_t)mv * (size_t)nch;
        // the draw
        const uint64_t seed_d = next_batch_seed(st);
        if (ssh_swap) {
            hipLaunchKernelGGL(k_sp_differs, dim3(nblk(st->nf), (unsigned)nch), dim3(TPB), 0, h->stream, S.differs, (const double *)st->x, seed_d, st->nf, L);
            RC(chk("k_sp_differs"));
            hipLaunchKernelGGL(k_sp_select, dim3((unsigned)nch), dim3(TPB), 0, h->stream, S.ci, S.cj, (const int *)S.differs, seed_d, st->nf);
            RC(chk("k_sp_select"));
        } else {
            hipLaunchKernelGGL(k_sp_draw, dim3(nblk(nch)), dim3(TPB), 0, h->stream, S.ci, S.cj, seed_d, nch, kind, st->nf, (int)h->nb,
                               (const int *)h->d_bi, (const int *)h->d_bj);
            RC(chk("k_sp_draw"));
        }
        // refresh_ϕ!(…, sample_R = true) for every chain, the start vectors of the set-up, the batch of the Metropolis numbers
        RC(refresh_phi(h, st, nullptr, nullptr));
        const double *kpm = nullptr;
        if (use_precond) RC(given_or_drawn(st, &kpm, kpm_own, 2 * (size_t)nch * (size_t)h->N, true));
        const uint64_t seed_u = next_batch_seed(st);
        RC(dot_parts(h, st, p_rr, st->R2, st->R2, (long long)nd, 2 * nch));
        RC(sb_parts(h, st, p_sb0));
        // the move, the action after it
        RC(move_chains(h, st, S, kind, nullptr));
        int64_t kpm_calls = 0;
        RC(calc_OinvLphi(h, st, use_precond, 2.0, kpm, &kpm_calls, iters.data() + row, flag.data() + row));
        HIPCHK(hipMemcpyAsync(S.flag, flag.data() + row, (size_t)nch * sizeof(int), hipMemcpyHostToDevice, h->stream));
        RC(dot_parts(h, st, p_sf, h->work.b, h->work.x, (long long)nd, 2 * nch));
        RC(sb_parts(h, st, p_sb1));
        // the Metropolis test and the undo of the rejected chains
        hipLaunchKernelGGL(k_sp_accept, dim3((unsigned)((nch + ELPH_WAVE - 1) / ELPH_WAVE)), dim3(ELPH_WAVE), 0, h->stream, (const double *)S.part, nch, L,
                           st->dtau, seed_u, (const int *)S.flag, (const int *)S.ci, (const int *)S.cj, S.undo, S.acc + row, S.out_i + row, S.out_j + row,
                           S.S0 + row, S.S1 + row);
        RC(chk("k_sp_accept"));
        RC(move_chains(h, st, S, kind, S.undo));
    }
    HIPCHK(hipMemcpyAsync(accepted, S.acc, rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (col_i) HIPCHK(hipMemcpyAsync(col_i, S.out_i, rows * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (col_j) HIPCHK(hipMemcpyAsync(col_j, S.out_j, rows * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (S0_out) HIPCHK(hipMemcpyAsync(S0_out, S.S0, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (S1_out) HIPCHK(hipMemcpyAsync(S1_out, S.S1, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (iters_out) memcpy(iters_out, iters.data(), rows * sizeof(int64_t));
    if (flag_out) memcpy(flag_out, flag.data(), rows * sizeof(int));
    return ELPH_OK;
}
