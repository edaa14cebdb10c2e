// hmc.hip — one HMC update of the Holstein model as a device-resident trajectory:
//   update!(model, hmc, fa, P)  ->  standard_update! (Nb = 1) / multitimestep_update! (Nb > 1),   HMC.jl:313-638
//   refresh_v!, refresh_ϕ!                                                                         HMC.jl:648-692
//   calc_H / calc_K / calc_S / calc_Sf                                                             HMC.jl:697-784
//   calc_Sb, calc_dSbdx!                                                                           PhononAction.jl:11-66,114-187
// x, v, ϕ±, Λϕ±, O⁻¹Λϕ±, dS/dx live on the device (layout S) for the whole trajectory and between trajectories; the host
// drives the leapfrog loop (every step ends in the CG stop test anyway), and only scalars (partial sums of S, K, the
// solver status) come back.  The random numbers the reference draws from model.rng are inputs of the call.
// No CPU fallback: every arithmetic step on lattice vectors is a kernel below or one of the solver's kernels.
// Here: the state and its setters, the trajectory, and the steps it shares with langevin.hip and special_updates.hip (hmc_dev.h).

#include "hmc_dev.h"

using namespace hmc;

namespace {

// The build's counter-based generator (sm64, u01: rng_dev.h).
// nvec vectors of ncols*L standard normals, written in layout S ([vec][tau][col]); the batch is numbered in the reference
// layout ([vec][col][tau]) so that it equals synth.randn(seed, nvec*ncols*L) handed over by the host
__global__ void __launch_bounds__(TPB) k_randn_S(double *__restrict__ dst, uint64_t seed, long long n, int ncols, int L) {
    const long long k = (long long)blockIdx.x * TPB + threadIdx.x;        // pair index
    const long long m = (n + 1) / 2;
    if (k >= m) return;
    const double r = sqrt(-2.0 * log(u01(seed, (uint64_t)k)));
    double sn, cs;
    sincos(6.283185307179586476925 * u01(seed, (uint64_t)(m + k)), &sn, &cs);
    const long long per = (long long)ncols * L;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long long i = 2 * k + e;
        if (i >= n) break;
        const long long vec = i / per, w = i - vec * per;
        const int col = (int)(w / L), t = (int)(w - (long long)col * L);
        dst[vec * per + (long long)t * ncols + col] = r * (e ? sn : cs);
    }
}

// E(τ,s) = exp(-Δτ (λ x + λ₂ x² - μ)), x already in layout S  (update_model!, HolsteinModels.jl:526-549)
__global__ void __launch_bounds__(TPB) k_hmc_expV(double *__restrict__ E, const double *__restrict__ x,
                                                  const double *__restrict__ lam3, int N, long long n, double dtau,
                                                  const double *__restrict__ mu_ch, long long ndim) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int s = (int)(i % N);
    const double xi = x[i];
    const double mu = mu_ch ? mu_ch[(i / ndim) * N + s] : lam3[2 * N + s];      // per chain when the tuner runs per chain
    E[i] = exp(-dtau * (lam3[s] * xi + lam3[N + s] * (xi * xi) + -mu));
}

// v = α v + sqrt(1-α²) y   (refresh_v!, HMC.jl:656)
__global__ void __launch_bounds__(TPB) k_hmc_refresh_v(double *__restrict__ v, const double *__restrict__ y, double alpha,
                                                       long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) v[i] = alpha * v[i] + sqrt(1.0 - alpha * alpha) * y[i];
}

// v = v - cv Q;  x = x + cx v  (cx = 0: velocity half step only)   (HMC.jl:392-395,421)
__global__ void __launch_bounds__(TPB) k_hmc_leap(double *__restrict__ v, double *__restrict__ x, const double *__restrict__ Q,
                                                  double cv, double cx, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double vn = v[i] - cv * Q[i];
    v[i] = vn;
    if (cx != 0.0) x[i] = x[i] + cx * vn;
}

// v = -v0  (rejected update, HMC.jl:453)
__global__ void __launch_bounds__(TPB) k_hmc_neg(double *__restrict__ v, const double *__restrict__ v0, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) v[i] = -v0[i];
}

// ϕ = Λ⁻¹ (MᵀR):  ϕ(τ) = -(1/Λ(τ)) u(τ-1),  ϕ(0) = +(1/Λ(0)) u(L-1)   (mulΛ⁻¹!, HMC.jl:978-995; Λ: :921-941)
__global__ void __launch_bounds__(TPB) k_hmc_phi(double *__restrict__ phi, const double *__restrict__ u,
                                                 const double *__restrict__ x, const double *__restrict__ lam3, int N, int L,
                                                 double dtau, int nch) {
    // i runs over [chain][ndim]; blockIdx.y = sign; u, phi are [sign][chain][ndim]
    const long long nd = (long long)N * L, n = nd * nch, i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const long long base = (i / nd) * nd;
    const int s = (int)(i % N), t = (int)((i % nd) / N);
    const int tm1 = (t == 0) ? L - 1 : t - 1;
    const double sg = (t == 0) ? 1.0 : -1.0;
    const double xi = x[i];
    const double Lam = exp(-dtau * (lam3[s] * xi + lam3[N + s] * (xi * xi)) / 2);
    const size_t o = (size_t)blockIdx.y * (size_t)n;
    phi[o + i] = sg * (1.0 / Lam) * u[o + (size_t)base + (size_t)tm1 * N + s];
}

// dS/dx (+)= dSb/dx   (calc_dSbdx!, PhononAction.jl:114-187, no dispersive modes)
__global__ void __launch_bounds__(TPB) k_hmc_dsb(double *__restrict__ dS, const double *__restrict__ x,
                                                 const double *__restrict__ par, int N, int L, double dtau, int accumulate,
                                                 int nch, const double *__restrict__ lam_shift = nullptr) {
    const long long nd = (long long)N * L, n = nd * nch, i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)((i / nd) * nd);
    const int s = (int)(i % N), t = (int)((i % nd) / N);
    const int tp1 = (t == L - 1) ? 0 : t + 1, tm1 = (t == 0) ? L - 1 : t - 1;
    const double w = par[s], w4 = par[N + s];
    const double xt = x[i];
    double d = accumulate ? dS[i] : 0.0;
    d += (dtau * w * w) * xt;
    d += (dtau * 4 * w4) * xt * xt * xt;
    d -= (x[base + (size_t)tp1 * N + s] + x[base + (size_t)tm1 * N + s] - 2.0 * xt) / dtau;
    if (lam_shift) d -= dtau * lam_shift[s];         // calc_dSbdx!(…, shifted = true): the particle-hole shifted action (Langevin)
    dS[i] = d;
}

__device__ __forceinline__ double blk_sum(double v, double *sc) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6, nw = TPB >> 6;
    if ((threadIdx.x & 63) == 0) sc[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < nw; ++k) t += sc[k];
    __syncthreads();
    return t;
}

// per-slice partial of Sb/Δτ   (calc_Sb, PhononAction.jl:11-66)
__global__ void __launch_bounds__(TPB) k_hmc_sb_part(double *__restrict__ part, const double *__restrict__ x,
                                                     const double *__restrict__ par, int N, int L, double dtau,
                                                     const double *__restrict__ wcol, int col_lo = 0, int col_hi = 1 << 30) {
    __shared__ double sc[8];
    const int t = blockIdx.x, tm1 = (t == 0) ? L - 1 : t - 1;
    x += (size_t)blockIdx.y * (size_t)N * L;                   // blockIdx.y = chain
    part += (size_t)blockIdx.y * L;
    double acc = 0.0;
    for (int s = threadIdx.x; s < N; s += TPB) {
        if (s < col_lo || s >= col_hi) continue;               // a sharded lattice: this rank's own columns only
        if (wcol && wcol[s] == 0.0) continue;                  // only primary phonons count (PhononAction.jl:83)
        const double xt = x[(size_t)t * N + s], xm = x[(size_t)tm1 * N + s], w = par[s], w4 = par[N + s];
        acc += w * w * (xt * xt) / 2 + w4 * (xt * xt * xt * xt);
        acc += (xt - xm) * (xt - xm) / (dtau * dtau) / 2;
    }
    acc = blk_sum(acc, sc);
    if (threadIdx.x == 0) part[t] = acc;
}

// partial dot products of vector blockIdx.y (n elements each): part[y][b] = sum over block b's range of a·b
__global__ void __launch_bounds__(TPB) k_hmc_dot_part(double *__restrict__ part, const double *__restrict__ a,
                                                      const double *__restrict__ b, long long n, long long per_block,
                                                      int ncols = 0, int col_lo = 0, int col_hi = 0) {
    __shared__ double sc[8];
    a += (size_t)blockIdx.y * (size_t)n; b += (size_t)blockIdx.y * (size_t)n;
    part += (size_t)blockIdx.y * gridDim.x;
    const long long lo = (long long)blockIdx.x * per_block, hi = (lo + per_block < n) ? lo + per_block : n;
    double acc = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += TPB) {
        if (ncols > 0) { const int c = (int)(i % ncols); if (c < col_lo || c >= col_hi) continue; }      // (sharded: own columns of [tau][col])
        acc += a[i] * b[i];
    }
    acc = blk_sum(acc, sc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// Shared fields (layout S: index = tau*nf + column).  k_alias_sum: every member of a class gets the class sum (muldMdx!,
// SSHModels.jl:820-826); k_alias_copy: every column takes its primary's value (randn!, :568-575); k_mask_cols: v *= wcol.
__global__ void __launch_bounds__(TPB) k_alias_sum(double *__restrict__ F, const int *__restrict__ prim, const int *__restrict__ next,
                                                   int nf, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int col = (int)(i % nf);
    if (prim[col] != col || next[col] < 0) return;
    const long long base = i - col;
    double sum = F[i];
    for (int c = next[col]; c >= 0; c = next[c]) sum += F[base + c];
    F[i] = sum;
    for (int c = next[col]; c >= 0; c = next[c]) F[base + c] = sum;
}
__global__ void __launch_bounds__(TPB) k_alias_copy(double *__restrict__ F, const int *__restrict__ prim, int nf, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int col = (int)(i % nf);
    if (prim[col] != col) F[i] = F[i - col + prim[col]];       // primaries are never written: no race
}
__global__ void __launch_bounds__(TPB) k_mask_cols(double *__restrict__ F, const double *__restrict__ wcol, int nf, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) F[i] *= wcol[i % nf];
}

// a sharded lattice (shard.hip: elph_shard_set_collectives): sums count this rank's own columns and are added over the ranks
bool sharded(const elph_handle_s *h) { return h->shard != nullptr && elph_i_shard_active(h); }

// rows x per_row partials back from the device, each row added in slice order
int read_sums(elph_handle_s *h, const double *part, int rows, int per_row, double *out) {
    std::vector<double> p((size_t)rows * per_row);
    HIPCHK(hipMemcpyAsync(p.data(), part, sizeof(double) * p.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    sum_rows(p.data(), rows, per_row, out);
    return ELPH_OK;
}

}  // namespace

namespace hmc {

int chk(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { elph_set_error("%s: %s", what, hipGetErrorString(e)); return ELPH_E_HIP; }
    return ELPH_OK;
}

int state_ready(elph_handle_s *h, HmcState **st, bool with_field) {
    *st = state_of(h);
    if (!*st) { elph_set_error("elph_hmc_create / elph_langevin_create[_ssh][_chains] has not been called"); return ELPH_E_STATE; }
    if (with_field && !(*st)->have_state) { elph_set_error("elph_hmc_set_state(x) has not been called"); return ELPH_E_STATE; }
    return ELPH_OK;
}

int dot_parts(elph_handle_s *h, HmcState *st, double *part, const double *a, const double *b, long long n, int count, bool site_vectors) {
    const int nb = (int)h->L;
    int ncols = 0, clo = 0, chi = 0;
    // a shard: site vectors count the own rows; field vectors of the Holstein model are site vectors; bond-phonon fields were masked by the caller
    if (sharded(h) && (site_vectors || !st->wown)) { ncols = (int)(n / h->L); elph_i_shard_own_range(h, &clo, &chi); }
    hipLaunchKernelGGL(k_hmc_dot_part, dim3((unsigned)nb, (unsigned)count), dim3(TPB), 0, h->stream, part, a, b, n, (n + nb - 1) / nb, ncols, clo, chi);
    return chk("k_hmc_dot_part");
}

int sb_parts(elph_handle_s *h, HmcState *st, double *part) {
    int clo = 0, chi = 1 << 30;
    if (sharded(h) && !st->wown) elph_i_shard_own_range(h, &clo, &chi);
    const double *w = st->wown ? st->wown : (st->shared ? st->wcol : nullptr);      // (bond phonons on a shard: the owned columns)
    hipLaunchKernelGGL(k_hmc_sb_part, dim3((unsigned)h->L, (unsigned)st->nch), dim3(TPB), 0, h->stream, part, st->x, st->par, st->nf, (int)h->L,
                       st->dtau, w, clo, chi);
    return chk("k_hmc_sb_part");
}

int dots_host(elph_handle_s *h, HmcState *st, const double *a, const double *b, long long n, int count, double *out, bool site_vectors) {
    RC(dot_parts(h, st, st->part, a, b, n, count, site_vectors));
    RC(read_sums(h, st->part, count, (int)h->L, out));
    return sharded(h) ? elph_i_shard_allreduce(h, out, count) : ELPH_OK;
}

int calc_Sb(elph_handle_s *h, HmcState *st, double *out) {
    RC(sb_parts(h, st, st->part));
    RC(read_sums(h, st->part, st->nch, (int)h->L, out));
    for (int c = 0; c < st->nch; ++c) out[c] = st->dtau * out[c];
    return sharded(h) ? elph_i_shard_allreduce(h, out, st->nch) : ELPH_OK;
}

int alias_sum(elph_handle_s *h, HmcState *st, double *F) {
    if (!st->shared) return ELPH_OK;
    const long long n = (long long)st->nf * h->L * st->nch;
    hipLaunchKernelGGL(k_alias_sum, dim3(nblk(n)), dim3(TPB), 0, h->stream, F, (const int *)st->prim, (const int *)st->next, st->nf, n);
    return chk("k_alias_sum");
}

int add_dsb(elph_handle_s *h, HmcState *st, double *dS, int accumulate, const double *lam_shift) {
    const long long n = (long long)st->nf * h->L * st->nch;
    hipLaunchKernelGGL(k_hmc_dsb, dim3(nblk(n)), dim3(TPB), 0, h->stream, dS, (const double *)st->x, (const double *)st->par, st->nf, (int)h->L,
                       st->dtau, accumulate, st->nch, lam_shift);
    return chk("k_hmc_dsb");
}

int update_model(elph_handle_s *h, HmcState *st) {
    if (st->ssh) {      // SSHModels.jl:510-562 from the device-resident fields (tau-major)
        RC(elph_launch_ssh_update(h, st->x, st->nf, h->d_ssh_cb, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_slot, st->dtau, 1, st->nch));
        h->ssh_dtau = st->dtau;
        h->cs_host_stale = true;
        h->have_E = true;
        return ELPH_OK;
    }
    const long long n = (long long)h->ndim * st->nch;
    hipLaunchKernelGGL(k_hmc_expV, dim3(nblk(n)), dim3(TPB), 0, h->stream, h->d_E, st->x, h->d_lam, (int)h->N, n, st->dtau,
                       (const double *)((h->mu_per_chain && st->nch <= h->mu_ch_cap) ? h->d_mu_ch : nullptr), (long long)h->ndim);
    h->have_E = true;
    return chk("k_hmc_expV");
}

// calc_O⁻¹Λϕ!(hmc, model, P, power)  (HMC.jl:820-915) for every chain: setup!(P) per chain, Λϕ±, all 2·nch solves as one
// batch (right-hand side v·nch + c belongs to chain c), per chain iters = cld(total, 2) and flag.  CG on MᵀM, or — the handle's solver
// kind — the two-stage pair solve of BiCGStab / GMRES on Mᵀ and M (msolve.hip)
int calc_OinvLphi(elph_handle_s *h, HmcState *st, int use_precond, double power, const double *kpm_randn, int64_t *kpm_calls,
                  int64_t *iters, int *flag) {
    const size_t nd = (size_t)h->ndim;
    const int nch = st->nch;
    int use = 0;
    if (h->solver_kind != ELPH_SOLVER_CG) RC(elph_i_msolve_ready(h));      // (before the sharded routes below, which are CG's)
    if (use_precond && sharded(h)) {
        // a sharded lattice: the expansion lives on the full-lattice handle (elph_shard_set_full_lattice), set up identically on every rank from
        // the SAME start vectors (kpm_randn holds vectors of the whole lattice) and the Ē summed over the ranks' own rows
        elph_handle_s *hf = elph_i_shard_full(h);
        const size_t NG = (size_t)hf->N;
        const double *bmax = kpm_randn + (size_t)(2 * *kpm_calls) * NG, *bmin = bmax + NG;
        ++*kpm_calls;
        if (st->ssh) {
            // bond phonons: the τ-means of cosh / sinh of every bond of the lattice, from the owners' slabs (update_A!, KPMPreconditioners.jl:355-381);
            // Λ ≡ 1 (HMC.jl:943-946,970-973): the right-hand sides are ϕ± themselves
            std::vector<double> cs;
            int64_t nbg = 0;
            RC(elph_i_shard_global_csbar(h, cs, &nbg));
            if (nbg != hf->nb) { elph_set_error("the full-lattice handle has %lld bonds, elph_shard_set_bonds named %lld", (long long)hf->nb, (long long)nbg); return ELPH_E_ARG; }
            RC(elph_i_kpm_setup_csbar(hf, cs.data(), cs.data() + nbg, bmax, bmin));
            HIPCHK(hipMemcpyAsync(h->work.b, st->phi, 2 * (size_t)nch * nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        } else {
            std::vector<double> Eg;
            RC(elph_i_shard_global_ebar(h, Eg));
            RC(elph_i_kpm_setup_ebar(hf, Eg.data(), bmax, bmin));
            RC(elph_launch_lambda_rhs(h, h->work.b, st->phi, st->x, st->dtau, nch));
        }
        HIPCHK(hipMemsetAsync(h->work.x, 0, 2 * (size_t)nch * nd * sizeof(double), h->stream));
        h->x_zero = false;
        return elph_i_shard_solve_pair(h, hf, 1, power, iters, flag);
    }
    if (use_precond) {
        // start vectors of this set-up call: [b_max | b_min][chain][N]
        const double *bmax = kpm_randn + (size_t)(2 * *kpm_calls) * (size_t)nch * (size_t)h->N, *bmin = bmax + (size_t)nch * h->N;
        ++*kpm_calls;
        RC(elph_kpm_setup_chains(h, bmax, bmin, nullptr, nullptr, nullptr, nullptr, nullptr));
        use = 1;                      // an inactive preconditioner is the identity inside the preconditioned recurrence
    }
    if (st->ssh)        // Λ ≡ 1 (HMC.jl:943-946,970-973): the right-hand sides are ϕ± themselves
        HIPCHK(hipMemcpyAsync(h->work.b, st->phi, 2 * (size_t)nch * nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else
        RC(elph_launch_lambda_rhs(h, h->work.b, st->phi, st->x, st->dtau, nch));
    HIPCHK(hipMemsetAsync(h->work.x, 0, 2 * (size_t)nch * nd * sizeof(double), h->stream));
    h->x_zero = true;
    if (sharded(h)) {      // one lattice over several ranks: the two solves one after the other through the sharded kernel (shard.hip)
        h->x_zero = false;
        return elph_i_shard_solve_pair(h, nullptr, 0, power, iters, flag);
    }
    if (h->solver_kind != ELPH_SOLVER_CG) {      // the mul_by_M branch (:859-873, :888-902): Mᵀ y = Λϕ±, then M x = y, y in work.z
        h->x_zero = false;
        std::vector<int64_t> it4((size_t)4 * nch, 0);
        std::vector<int> fl4((size_t)4 * nch, 0), zm((size_t)nch, 0);
        {
            TolPower scope(h, power);
            RC(elph_i_msolve_pair(h, 2 * nch, use, h->work.x, h->work.z, h->work.b, it4.data(), fl4.data()));
        }
        elph_fold_pair_stages(nch, it4.data(), fl4.data(), iters, flag, zm.data());
        for (int c = 0; c < nch; ++c)
            if (zm[c]) RC(elph_launch_zero(h, h->work.x + (size_t)(nch + c) * nd, (int64_t)nd));
        return ELPH_OK;
    }
    std::vector<int64_t> it2((size_t)2 * nch, 0);
    std::vector<double> res2((size_t)2 * nch);
    std::vector<int> fl2((size_t)2 * nch, 0);
    {
        TolPower scope(h, power);
        RC(elph_i_ldiv_core(h, 2 * nch, use, 0, it2.data(), res2.data(), fl2.data()));
    }
    elph_fold_pair(nch, it2.data(), fl2.data(), iters, flag);
    return ELPH_OK;
}

int fa(elph_handle_s *h, HmcState *st, double *out, const double *in, double power) {
    return elph_launch_fft_accel(h, out, in, st->faM, power, st->nf, st->nch);
}

int randn_vectors(elph_handle_s *h, HmcState *st, double *dstS, const double *host, int nvec, int ncols) {
    if (host) return elph_stage_in(h, dstS, host, nvec, ncols);
    RC(need_randoms(st, false, "random inputs"));
    const int nc = ncols > 0 ? ncols : (int)h->N;
    const long long n = (long long)nvec * nc * h->L;
    hipLaunchKernelGGL(k_randn_S, dim3(nblk((n + 1) / 2)), dim3(TPB), 0, h->stream, dstS, next_batch_seed(st), n, nc, (int)h->L);
    RC(chk("k_randn_S"));
    if (ncols > 0 && st->shared) {      // randn!(v, ssh): v = v[primary_field]  (SSHModels.jl:568-575)
        hipLaunchKernelGGL(k_alias_copy, dim3(nblk(n)), dim3(TPB), 0, h->stream, dstS, (const int *)st->prim, nc, n);
        RC(chk("k_alias_copy"));
    }
    return ELPH_OK;
}

int refresh_phi(elph_handle_s *h, HmcState *st, const double *Rp, const double *Rm) {
    const size_t nd = (size_t)h->ndim;
    const int nch = st->nch;                 // R2, ϕ: [sign][chain][ndim]
    RC(randn_vectors(h, st, st->R2, Rp, nch));
    RC(randn_vectors(h, st, st->R2 + (size_t)nch * nd, Rm, nch));
    RC(elph_launch_mul(h, 1, h->work.b, st->R2, 2 * nch));
    if (st->ssh)        // Λ⁻¹ ≡ 1: ϕ± = MᵀR±
        HIPCHK(hipMemcpyAsync(st->phi, h->work.b, 2 * (size_t)nch * nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else {
        hipLaunchKernelGGL(k_hmc_phi, dim3(nblk((long long)nd * nch), 2), dim3(TPB), 0, h->stream, st->phi, (const double *)h->work.b,
                           (const double *)st->x, (const double *)h->d_lam, (int)h->N, (int)h->L, st->dtau, nch);
        RC(chk("k_hmc_phi"));
    }
    return ELPH_OK;
}

}  // namespace hmc

namespace {

// calc_H (HMC.jl:697-705) per chain: S = Sf + Sb (:745-756,768-784), K = v·(M v)/2 (:711-719)
int calc_H(elph_handle_s *h, HmcState *st, double *H, double *S, double *K) {
    const int nch = st->nch;
    std::vector<double> sf((size_t)2 * nch), sb((size_t)nch), k((size_t)nch);
    RC(dots_host(h, st, h->work.b, h->work.x, (long long)h->ndim, 2 * nch, sf.data()));
    RC(calc_Sb(h, st, sb.data()));
    RC(fa(h, st, st->y, st->v, 1.0));
    if (st->shared || st->wown) {       // calc_K of the SSH model counts primary fields only (HMC.jl:720-738); on a shard: the owned columns
        const long long nn = (long long)st->nf * h->L * nch;
        hipLaunchKernelGGL(k_mask_cols, dim3(nblk(nn)), dim3(TPB), 0, h->stream, st->y, (const double *)(st->wown ? st->wown : st->wcol), st->nf, nn);
        RC(chk("k_mask_cols"));
    }
    RC(dots_host(h, st, st->v, st->y, (long long)st->nf * h->L, nch, k.data(), false));
    for (int c = 0; c < nch; ++c) {
        S[c] = (sf[(size_t)c] + sf[(size_t)nch + c]) / 2 + sb[(size_t)c];
        K[c] = k[(size_t)c] / 2;
        H[c] = S[c] + K[c];
    }
    return ELPH_OK;
}

// dS/dx = dSf/dx [+ dSb/dx]; Q = M^-1 dS/dx in place  (HMC.jl:379-384)
int force(elph_handle_s *h, HmcState *st, bool with_Sb) {
    if (st->ssh) {      // dSf/dx = -dMdx(M X₊, X₊) - dMdx(M X₋, X₋)  (HMC.jl:797-808; muldΛdx! is a no-op)
        RC(elph_launch_force_ssh(h, h->work.p, h->work.x, nullptr, st->nch));        // bond brackets q[chain][tau][bond] (work.p is free here)
        RC(elph_launch_ssh_scatter(h, st->dS, h->work.p, st->x, h->d_ssh_par, h->d_ssh_cb, st->nf, st->dtau, 1, -1.0, st->nch));
        RC(alias_sum(h, st, st->dS));
    } else {
        RC(elph_launch_force_holstein(h, st->dS, h->work.x, st->phi, st->x, st->dtau, st->nch));
    }
    // a sharded lattice: the fermion force is exact on the own rows (the MᵀM closure); the ghost rows — which the leapfrog moves along with
    // the own ones, so that the next update_model! sees the whole slab — take it from their owners.  The boson force and the Fourier
    // acceleration below are pointwise in the site index.
    if (sharded(h) && st->ssh) RC(elph_i_shard_ghost_sync_cols(h, st->dS, 1, st->nf, st->gcol.data(), st->ngcol, st->wown_host.data()));
    else if (sharded(h)) RC(elph_i_shard_ghost_sync(h, st->dS, 1));
    if (with_Sb) RC(add_dsb(h, st, st->dS, 1));
    return fa(h, st, st->dS, st->dS, -1.0);
}

// Q = M^-1 dSb/dx, the inner force of multitimestep_update!  (HMC.jl:528-532)
int boson_force(elph_handle_s *h, HmcState *st) {
    RC(add_dsb(h, st, st->dS, 0));
    return fa(h, st, st->dS, st->dS, -1.0);
}

int leap(elph_handle_s *h, HmcState *st, double cv, double cx) {
    const long long n = (long long)st->nf * h->L * st->nch;
    hipLaunchKernelGGL(k_hmc_leap, dim3(nblk(n)), dim3(TPB), 0, h->stream, st->v, st->x, st->dS, cv, cx, n);
    return chk("k_hmc_leap");
}

// Every device allocation of the state, in one list: hmc_create_core makes those with a size, the others are made on first use (0);
// elph_hmc_free frees them all
struct DevAlloc { void **p; size_t bytes; };
std::vector<DevAlloc> device_allocations(const elph_handle_s *h, HmcState *st) {
    const size_t nd = (size_t)h->ndim * sizeof(double), nfd = (size_t)st->nf * (size_t)h->L * sizeof(double), nc = (size_t)st->nch;
    return {{(void **)&st->x, nc * nfd}, {(void **)&st->v, nc * nfd}, {(void **)&st->x0, nc * nfd}, {(void **)&st->v0, nc * nfd},
            {(void **)&st->dS, nc * nfd}, {(void **)&st->y, nc * nfd}, {(void **)&st->faM, nfd}, {(void **)&st->R2, 2 * nc * nd},
            {(void **)&st->phi, 2 * nc * nd}, {(void **)&st->par, 2 * (size_t)st->nf * sizeof(double)}, {(void **)&st->part, 2 * nc * (size_t)h->L * sizeof(double)},
            {(void **)&st->prim, 0}, {(void **)&st->next, 0}, {(void **)&st->wcol, 0}, {(void **)&st->wown, 0}, {&st->sp_buf, 0}};
}

}  // namespace

void elph_hmc_free(elph_handle_s *h) {
    HmcState *st = state_of(h);
    if (!st) return;
    for (const DevAlloc &a : device_allocations(h, st)) if (*a.p) (void)hipFree(*a.p);
    delete st;
    h->hmc = nullptr;
}

static int hmc_create_core(elph_handle_s *h, int nchains, int nf, bool ssh, const double *omega, const double *omega4, double dtau,
                           const double *fa_mass) {
    // staging / scratch must hold the field vectors too (SSH: Nph columns may exceed the number of sites)
    const int per_field = (int)(((int64_t)nf + h->N - 1) / h->N);
    RC(elph_work_reserve(h, std::max(2 * nchains, 2 * per_field + 1)));
    elph_hmc_free(h);
    HmcState *st = new HmcState();
    h->hmc = st;
    st->nch = nchains; st->nf = nf; st->ssh = ssh;
    h->mu_per_chain = false;                 // a new dynamics state starts from the deck's one chemical potential
    const size_t nfd = (size_t)nf * (size_t)h->L, nc = (size_t)nchains;
    for (const DevAlloc &a : device_allocations(h, st)) if (a.bytes) HIPCHK(hipMalloc(a.p, a.bytes));
    st->dtau = dtau;
    HIPCHK(hipMemcpyAsync(st->par, omega, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->par + nf, omega4, (size_t)nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_stage_in(h, st->faM, fa_mass, 1, nf));
    HIPCHK(hipMemsetAsync(st->v, 0, nc * nfd * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(st->x, 0, nc * nfd * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_hmc_create_chains(elph_handle h, int nchains, const double *omega, const double *omega4, const double *lambda,
                                      const double *lambda2, const double *mu, double dtau, const double *fa_mass) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("elph_hmc_create[_chains]: Holstein handles (SSH: elph_hmc_create_ssh)"); return ELPH_E_UNSUPPORTED; }
    if (nchains < 1 || !omega || !omega4 || !lambda || !lambda2 || !mu || !fa_mass || !(dtau > 0.0)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_work_reserve(h, 2 * nchains));
    RC(elph_i_reserve_chains(h, nchains));
    const size_t N = (size_t)h->N;
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + 2 * N, mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return hmc_create_core(h, nchains, (int)h->N, false, omega, omega4, dtau, fa_mass);
}

extern "C" int elph_hmc_create(elph_handle h, const double *omega, const double *omega4, const double *lambda,
                               const double *lambda2, const double *mu, double dtau, const double *fa_mass) {
    return elph_hmc_create_chains(h, 1, omega, omega4, lambda, lambda2, mu, dtau, fa_mass);
}

// HybridMonteCarlo for an SSH model (bond phonons): omega, omega4 per phonon (double[nph]), fa_mass double[nph * ltau]; the
// remaining arguments are those of elph_update_model_ssh_fields (couplings, checkerboard positions, bare hoppings, mu).
extern "C" int elph_hmc_create_ssh_chains(elph_handle h, int nchains, int64_t nph, const double *omega, const double *omega4,
                                          const int64_t *cb_index, const double *t_ph, const double *alpha, const double *alpha2,
                                          const double *t_bare_cb, const double *mu, double dtau, const double *fa_mass) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("elph_hmc_create_ssh: SSH handles only"); return ELPH_E_UNSUPPORTED; }
    if (nchains < 1 || nph < 1 || !omega || !omega4 || !fa_mass || !(dtau > 0.0)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_i_ssh_bracket_capacity(h, 2 * nchains, nchains));
    RC(elph_i_reserve_chains(h, nchains));
    RC(elph_i_ssh_upload_params(h, nph, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu));
    return hmc_create_core(h, nchains, (int)nph, true, omega, omega4, dtau, fa_mass);
}

extern "C" int elph_hmc_create_ssh(elph_handle h, int64_t nph, const double *omega, const double *omega4, const int64_t *cb_index,
                                   const double *t_ph, const double *alpha, const double *alpha2, const double *t_bare_cb,
                                   const double *mu, double dtau, const double *fa_mass) {
    return elph_hmc_create_ssh_chains(h, 1, nph, omega, omega4, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu, dtau, fa_mass);
}

// x, v: double[nchains * ndim] (chain-major, reference layout inside a chain); NULL = leave
extern "C" int elph_hmc_set_state(elph_handle h, const double *x, const double *v) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (x && st->shared) {      // update_model! refuses fields that differ from their primary (SSHModels.jl:549-559; isapprox)
        const size_t L = (size_t)h->L;
        for (int ch = 0; ch < st->nch; ++ch)
        for (int c = 0; c < st->nf; ++c) {
            const int pc = st->prim_host[(size_t)c];
            if (pc == c) continue;
            const size_t co = (size_t)ch * (size_t)st->nf * L;
            for (size_t t = 0; t < L; ++t) {
                const double a = x[co + (size_t)c * L + t], b = x[co + (size_t)pc * L + t];
                if (!(fabs(a - b) <= 1.4901161193847656e-08 * fmax(fabs(a), fabs(b)))) {
                    elph_set_error("(x[%zu]=%g) != (x[%zu]=%g): fields that share a primary field must be equal", (size_t)c * L + t + 1, a,
                                   (size_t)pc * L + t + 1, b);
                    return ELPH_E_ARG;
                }
            }
        }
    }
    if (x) {
        RC(elph_stage_in(h, st->x, x, st->nch, st->nf));
        HIPCHK(hipStreamSynchronize(h->stream));
        st->have_state = true;
    }
    if (v) {
        RC(elph_stage_in(h, st->v, v, st->nch, st->nf));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ELPH_OK;
}

extern "C" int elph_hmc_get_state(elph_handle h, double *x, double *v) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (x) {
        RC(elph_stage_out(h, x, st->x, st->nch, st->nf));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (v) {
        RC(elph_stage_out(h, v, st->v, st->nch, st->nf));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ELPH_OK;
}

// model.μ changed (the chemical-potential tuner, MuFinder.jl:68-107: μ += Δμ on every site): refresh the device copy and the model
extern "C" int elph_hmc_set_mu(elph_handle h, const double *mu) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (!mu) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t N = (size_t)h->N;
    h->mu_per_chain = false;
    HIPCHK(hipMemcpyAsync(h->d_lam + (st->ssh ? 0 : 2 * N), mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (st->have_state) {
        RC(update_model(h, st));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ELPH_OK;
}

// the tuner with chains in lockstep: every chain its own chemical potential, mu[nchains][nsites]
extern "C" int elph_hmc_set_mu_chains(elph_handle h, const double *mu) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (!mu) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t N = (size_t)h->N, nch = (size_t)st->nch;
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((int)nch > h->mu_ch_cap) {
        if (h->d_mu_ch) { HIPCHK(hipFree(h->d_mu_ch)); h->d_mu_ch = nullptr; }
        HIPCHK(hipMalloc((void **)&h->d_mu_ch, nch * N * sizeof(double)));
        h->mu_ch_cap = (int)nch;
    }
    HIPCHK(hipMemcpy(h->d_mu_ch, mu, nch * N * sizeof(double), hipMemcpyHostToDevice));
    h->mu_per_chain = true;
    if (st->have_state) {
        RC(update_model(h, st));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ELPH_OK;
}

extern "C" int elph_hmc_set_shared_fields(elph_handle h, const int64_t *primary_column) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (!st->ssh) { elph_set_error("elph_hmc_create_ssh / elph_langevin_create_ssh has not been called"); return ELPH_E_STATE; }
    if (!primary_column) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const int nf = st->nf;
    std::vector<int> prim((size_t)nf), next((size_t)nf, -1), last((size_t)nf);
    std::vector<double> w((size_t)nf);
    bool any = false;
    for (int c = 0; c < nf; ++c) {
        const int64_t p = primary_column[c];
        if (p < 0 || p > c || primary_column[p] != p) {
            elph_set_error("primary_column[%d] = %lld: a primary is an earlier (or the same) column that is its own primary", c, (long long)p);
            return ELPH_E_ARG;
        }
        prim[(size_t)c] = (int)p;
        last[(size_t)c] = c;
        w[(size_t)c] = (p == c) ? 1.0 : 0.0;
        if (p != c) {       // append to the class list of p, in column order
            next[(size_t)last[(size_t)p]] = c;
            last[(size_t)p] = c;
            any = true;
        }
    }
    if (!st->prim) {
        HIPCHK(hipMalloc((void **)&st->prim, (size_t)nf * sizeof(int)));
        HIPCHK(hipMalloc((void **)&st->next, (size_t)nf * sizeof(int)));
        HIPCHK(hipMalloc((void **)&st->wcol, (size_t)nf * sizeof(double)));
    }
    HIPCHK(hipMemcpy(st->prim, prim.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(st->next, next.data(), (size_t)nf * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(st->wcol, w.data(), (size_t)nf * sizeof(double), hipMemcpyHostToDevice));
    st->prim_host = prim;
    st->shared = any;
    return ELPH_OK;
}

// Bond phonons on a sharded lattice: the slab's phonon columns (the phonons of its bonds, ghost bonds included) in the numbering of the whole
// lattice, and which of them this rank owns (the bond's first site lies in the own rows: every phonon has exactly one owner).  Call after
// elph_hmc_create_ssh on the slab handle.  Sums over fields (S_b, K) then count owned columns and are added over the ranks; the fermion
// force — exact on the owner, where the bond bracket is — reaches the other holders of a column through the host all-reduce.
extern "C" int elph_shard_hmc_set_columns(elph_handle h, const int64_t *global_column, int64_t n_global_columns, const double *own_weight) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    if (!st->ssh) { elph_set_error("elph_hmc_create_ssh has not been called"); return ELPH_E_STATE; }
    if (!h->shard) { elph_set_error("elph_shard_create has not been called"); return ELPH_E_STATE; }
    if (!global_column || !own_weight || n_global_columns < st->nf) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    st->gcol.assign((size_t)st->nf, 0);
    st->wown_host.assign((size_t)st->nf, 0.0);
    for (int c = 0; c < st->nf; ++c) {
        if (global_column[c] < 0 || global_column[c] >= n_global_columns || !(own_weight[c] == 0.0 || own_weight[c] == 1.0)) {
            elph_set_error("column %d: global column %lld of %lld, weight %g", c, (long long)global_column[c], (long long)n_global_columns, own_weight[c]);
            return ELPH_E_ARG;
        }
        st->gcol[(size_t)c] = (int)global_column[c];
        st->wown_host[(size_t)c] = own_weight[c];
    }
    st->ngcol = (int)n_global_columns;
    if (!st->wown) HIPCHK(hipMalloc((void **)&st->wown, (size_t)st->nf * sizeof(double)));
    HIPCHK(hipMemcpy(st->wown, st->wown_host.data(), (size_t)st->nf * sizeof(double), hipMemcpyHostToDevice));
    return ELPH_OK;
}

extern "C" int elph_hmc_set_rng(elph_handle h, uint64_t seed) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st));
    st->rng_on = true;
    st->rng_seed = seed;
    st->rng_batches = 0;
    return ELPH_OK;
}

extern "C" int elph_hmc_rng_batches(elph_handle h, uint64_t *batches) {
    CHECK_H(h);
    HmcState *st = state_of(h);
    if (!st || !batches) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *batches = st->rng_batches;
    return ELPH_OK;
}

// One HMC update of every chain, in lockstep: the leapfrog schedule is common, each chain has its own field, momenta,
// pseudofermions, energies, Metropolis test and failure flag.  A chain whose solve fails (flag > 0, HMC.jl:405-408) is
// dead for this update: its field is put back to x0 at once (so that its remaining — ignored — solves stay cheap) and
// it is rejected at the end.
extern "C" int elph_hmc_update_chains(elph_handle h, double dt, int64_t nt, int nb, double alpha, int use_precond, const double *R,
                                      const double *Rp, const double *Rm, const double *kpm_randn, const double *u_accept,
                                      int *accepted, double *iters_per_solve, double *energies, int *flag_out) {
    CHECK_H(h);
    HmcState *st;
    RC(state_ready(h, &st, true));
    if (!accepted || nt < 0 || nb < 1 || !(alpha >= 0.0 && alpha < 1.0) || !(dt > 0.0)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(need_randoms(st, R && Rp && Rm && u_accept && (!use_precond || kpm_randn), "R, Rp, Rm, u_accept (and kpm_randn with a preconditioner)"));
    if (use_precond && !h->kpm.created && !sharded(h)) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    const int nch = st->nch;
    if (sharded(h)) {
        // one lattice over several ranks: the trajectory runs on the slab (own + ghost rows); the random vectors must be the slab's part
        // of the GLOBAL vectors (ghost entries included) and the uniform of the Metropolis test the same number on every rank
        const bool prec_ok = !use_precond || (elph_i_shard_full(h) && elph_i_shard_full(h)->kpm.created && kpm_randn && (!st->ssh || elph_i_shard_has_bonds(h)));
        if ((st->ssh && (!st->wown || st->shared)) || nch != 1 || !prec_ok || st->rng_on || !R || !Rp || !Rm || !u_accept) {
            elph_set_error("HMC on a sharded lattice: one chain, with R, Rp, Rm and u_accept given (the slab's part of the global vectors); bond "
                           "phonons after elph_shard_hmc_set_columns, without shared fields; a preconditioner needs elph_shard_set_full_lattice with "
                           "elph_kpm_create done, kpm_randn = start vectors of the WHOLE lattice and — bond phonons — elph_shard_set_bonds");
            return ELPH_E_UNSUPPORTED;
        }
    }
    RC(elph_work_reserve(h, 2 * nch));
    RC(elph_i_reserve_chains(h, nch));
    const size_t nfd = (size_t)st->nf * (size_t)h->L, cbytes = nfd * sizeof(double), bytes = (size_t)nch * cbytes;
    const long long n = (long long)nfd * nch;
    const double dtp = dt / (double)nb;
    int64_t kpm_calls = 0;
    std::vector<int64_t> iters((size_t)nch, 0), itrs((size_t)nch, 0);
    std::vector<int> flag((size_t)nch, 0), dead((size_t)nch, 0);
    std::vector<double> H0((size_t)nch, 0.0), H1((size_t)nch, 0.0), S((size_t)nch, 0.0), K((size_t)nch, 0.0), P((size_t)nch, 0.0);
    auto bury = [&]() -> int {              // chains that just failed: remember the flag, restore their field
        for (int c = 0; c < nch; ++c)
            if (flag[(size_t)c] > 0 && !dead[(size_t)c]) {
                dead[(size_t)c] = flag[(size_t)c];
                HIPCHK(hipMemcpyAsync(st->x + (size_t)c * nfd, st->x0 + (size_t)c * nfd, cbytes, hipMemcpyDeviceToDevice, h->stream));
            }
        return ELPH_OK;
    };
    auto all_dead = [&]() { for (int c = 0; c < nch; ++c) if (!dead[(size_t)c]) return false; return true; };

    RC(update_model(h, st));
    // refresh_v!  (HMC.jl:648-659)
    RC(randn_vectors(h, st, st->y, R, nch, st->nf));
    RC(fa(h, st, st->y, st->y, -0.5));
    hipLaunchKernelGGL(k_hmc_refresh_v, dim3(nblk(n)), dim3(TPB), 0, h->stream, st->v, st->y, alpha, n);
    RC(chk("k_hmc_refresh_v"));
    HIPCHK(hipMemcpyAsync(st->x0, st->x, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->v0, st->v, bytes, hipMemcpyDeviceToDevice, h->stream));
    RC(refresh_phi(h, st, Rp, Rm));
    std::vector<double> kpm_own, u_own;
    if (use_precond) RC(given_or_drawn(st, &kpm_randn, kpm_own, (size_t)(nt + 2) * 2 * (size_t)nch * (size_t)h->N, true));
    RC(given_or_drawn(st, &u_accept, u_own, (size_t)nch, false));
    // a sharded lattice: MᵀR± is exact on the own rows only (its ghost rows would need R beyond the slab); ϕ± of the ghost rows from their owners
    if (sharded(h)) RC(elph_i_shard_ghost_sync(h, st->phi, 2));

    RC(calc_OinvLphi(h, st, use_precond, 2.0, kpm_randn, &kpm_calls, itrs.data(), flag.data()));
    // standard_update! :373 counts these iterations;  multitimestep_update! :507 has "iters += iters": not counted
    if (nb == 1) for (int c = 0; c < nch; ++c) iters[(size_t)c] = itrs[(size_t)c];
    RC(bury());
    if (!all_dead()) {
        RC(calc_H(h, st, H0.data(), S.data(), K.data()));
        RC(force(h, st, nb == 1));
        for (int64_t t = 1; t <= nt; ++t) {
            if (nb == 1) {
                RC(leap(h, st, dt / 2, dt));                                   // :392-395
            } else {
                RC(leap(h, st, dt / 2, 0.0));                                  // :525
                RC(boson_force(h, st));                                        // :528-532
                for (int tp = 1; tp <= nb; ++tp) {                             // :535-552
                    RC(leap(h, st, dtp / 2, dtp));
                    RC(boson_force(h, st));
                    RC(leap(h, st, dtp / 2, 0.0));
                }
            }
            for (int c = 0; c < nch; ++c)       // a dead chain idles at its old field
                if (dead[(size_t)c])
                    HIPCHK(hipMemcpyAsync(st->x + (size_t)c * nfd, st->x0 + (size_t)c * nfd, cbytes, hipMemcpyDeviceToDevice, h->stream));
            RC(update_model(h, st));
            RC(calc_OinvLphi(h, st, use_precond, 1.0, kpm_randn, &kpm_calls, itrs.data(), flag.data()));
            for (int c = 0; c < nch; ++c) if (!dead[(size_t)c]) iters[(size_t)c] += itrs[(size_t)c];
            RC(bury());
            if (all_dead()) break;                                             // :405-408
            RC(force(h, st, nb == 1));
            RC(leap(h, st, dt / 2, 0.0));                                      // :418
        }
    }
    if (!all_dead()) {
        RC(calc_OinvLphi(h, st, use_precond, 2.0, kpm_randn, &kpm_calls, itrs.data(), flag.data()));
        for (int c = 0; c < nch; ++c) if (!dead[(size_t)c]) iters[(size_t)c] += itrs[(size_t)c];
        RC(bury());
        if (!all_dead()) {
            RC(calc_H(h, st, H1.data(), S.data(), K.data()));
            for (int c = 0; c < nch; ++c) {
                if (dead[(size_t)c]) continue;
                const double e = exp(-(H1[(size_t)c] - H0[(size_t)c]));
                P[(size_t)c] = (1.0 < e) ? 1.0 : e;                            // min(1, exp(-ΔH)); NaN -> NaN -> reject, like Julia
            }
        }
    }
    bool any_reject = false;
    for (int c = 0; c < nch; ++c) {
        const int acc = (!dead[(size_t)c] && u_accept[c] < P[(size_t)c]) ? 1 : 0;      // :441
        accepted[c] = acc;
        if (!acc) {
            any_reject = true;
            HIPCHK(hipMemcpyAsync(st->x + (size_t)c * nfd, st->x0 + (size_t)c * nfd, cbytes, hipMemcpyDeviceToDevice, h->stream));
            hipLaunchKernelGGL(k_hmc_neg, dim3(nblk((long long)nfd)), dim3(TPB), 0, h->stream, st->v + (size_t)c * nfd,
                               st->v0 + (size_t)c * nfd, (long long)nfd);
            RC(chk("k_hmc_neg"));
        }
    }
    if (any_reject) RC(update_model(h, st));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nch; ++c) {
        if (iters_per_solve) iters_per_solve[c] = (double)((iters[(size_t)c] + (nt + 2) - 1) / (nt + 2));   // T1(cld(iters, Nt+2))
        if (energies) {
            double *e = energies + 5 * (size_t)c;
            e[0] = H0[(size_t)c]; e[1] = H1[(size_t)c]; e[2] = S[(size_t)c]; e[3] = K[(size_t)c]; e[4] = P[(size_t)c];
        }
        if (flag_out) flag_out[c] = dead[(size_t)c];
    }
    return ELPH_OK;
}

extern "C" int elph_hmc_update(elph_handle h, double dt, int64_t nt, int nb, double alpha, int use_precond, const double *R,
                               const double *Rp, const double *Rm, const double *kpm_randn, double u_accept, int *accepted,
                               double *iters_per_solve, double *energies, int *flag_out) {
    CHECK_H(h);
    HmcState *st = state_of(h);
    if (st && st->nch != 1) { elph_set_error("%d chains: use elph_hmc_update_chains", st->nch); return ELPH_E_STATE; }
    return elph_hmc_update_chains(h, dt, nt, nb, alpha, use_precond, R, Rp, Rm, kpm_randn, u_accept >= 0.0 ? &u_accept : nullptr, accepted, iters_per_solve,
                                  energies, flag_out);
}
