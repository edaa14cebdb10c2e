// greens.hip — stochastic Green's-function estimator on the device:
//   update!(estimator, model, P)      GreensFunctions.jl:201-234   n_v solves M⁻¹r = (MᵀM)⁻¹ Mᵀ r as ONE batched CG
//   setup!(estimator, n₁, n₂)         GreensFunctions.jl:239-288   the four translation-averaged products
//   convolve!, antiperiodic_copy!, periodic_product!               :351-440
//
// The reference doubles the time axis to 2L (antiperiodic copy [a, -a] or periodic copy [a·c, a·c]), runs 4-D FFTs
// (FFTW) of size 2L x L1 x L2 x L3 per orbital, multiplies fft(a)[ω,k]·fft(b)[-ω,-k]/V and transforms back: a circular
// cross-correlation  ab[Δ] = (1/V) Σ_x a~[x+Δ] b~[x].  Here the doubling is never materialised:
//   * an antiperiodic 2L-sequence has only odd frequencies and they are twice the L-point *twisted* spectrum
//     (TimeFreqFFTs.jl:55-73 — the transform the KPM preconditioner already owns); a periodic one only even
//     frequencies = twice the plain L-point spectrum; both inputs are real, so half spectra suffice and
//     fft(b)[-ω,-k] = conj fft(b)[ω,k];
//   * R and M⁻¹R sit in layout S (slice-major) after the solve, which is the layout the τ-DFT kernels of dft.hip read
//     with coalesced rows; the spatial transform of one frequency slice (N complex numbers) fits in LDS, so
//     forward spatial DFT of a and b, the orbital outer product, and the inverse spatial DFT are ONE kernel
//     (k_gr_spatial, one workgroup per (product, frequency, chain));
//   * the result is real; the second half of the 2L axis is ∓ the first.  Output arrays keep the reference's shape
//     Complex[2L, n_s, n_s, L1, L2, L3] (imaginary parts are exact zeros) so measure_GΔ0 & co. index them unchanged.
// Spatial extents are the lattice's (8…32): direct DFTs with host-built twiddles, exact index reduction.
//
// There is ONE pipeline, over an ElphGreensChainScratch: one pair of vectors of every chain the scratch serves, the chain a grid axis.
// The estimator's own scratch serves one chain (nchains = 1: row n of R is vector n) and alone carries the doubled complex copies; a
// measurement unit of resident chains brings scratch of its own, so that the estimator's tables are not touched.

#include <cmath>
#include <vector>

#include "cell_dft_dev.h"
#include "elph_internal.h"
#include "rng_dev.h"

namespace {

constexpr int TPB = 256;
static_assert(TPB == CELL_DFT_TPB, "dft_cells walks the workgroup of k_gr_spatial");

struct GreensState {
    int ns = 1, L1 = 1, L2 = 1, L3 = 1, nc = 1, nv = 2;
    bool have_vectors = false;
    bool rng_on = false;                   // the estimator's own generator (elph_greens_set_rng)
    uint64_t rng_seed = 0, rng_batches = 0;
    double *R = nullptr, *X = nullptr;     // [nv][ndim] layout S: noise vectors and M⁻¹R
    ElphGreensChainScratch own{};          // the pipeline's buffers for one chain (layouts: elph_internal.h), with own.out [4][2L*ns*N]
    double2 *tw = nullptr;                 // [L1 + L2 + L3] exp(-2πi j/Lx)
};

GreensState *gs_of(elph_handle_s *h) { return (GreensState *)h->greens; }

// The eight fields of setup! (GreensFunctions.jl:261-284), pointwise, layout S:
//   0: (M⁻¹r₁ + M⁻¹r₂)/√2   1: (r₁ + r₂)/√2            — antiperiodic pair (G[Δ,0])
//   2: M⁻¹r₁·M⁻¹r₂          3: r₁·r₂                   — G[Δ,0]·G[Δ,0]
//   4: M⁻¹r₂·r₂             5: M⁻¹r₁·r₁                — G[Δ,Δ]·G[0,0]
//   6: M⁻¹r₁·r₂             7: M⁻¹r₂·r₁                — G[Δ,0]·G[0,Δ]
__global__ void __launch_bounds__(TPB) k_gr_fields(double *__restrict__ f, const double *__restrict__ x1,
                                                   const double *__restrict__ x2, const double *__restrict__ r1,
                                                   const double *__restrict__ r2, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double a1 = x1[i], a2 = x2[i], b1 = r1[i], b2 = r2[i];
    const double sq2 = sqrt(2.0);
    f[i] = (a1 + a2) / sq2;
    f[n + i] = (b1 + b2) / sq2;
    f[2 * n + i] = a1 * a2;
    f[3 * n + i] = b1 * b2;
    f[4 * n + i] = a2 * b2;
    f[5 * n + i] = a1 * b1;
    f[6 * n + i] = a1 * b2;
    f[7 * n + i] = a2 * b1;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// The work of one workgroup on one frequency slice: spatial DFT of the two spectra a, b (N complex numbers each), outer product over
// orbitals with fft(b)[-ω,-k] = conj fft(b)[ω,k], inverse spatial DFT into y[s2 + ns*(s1 + ns*cell)].
// LDS: 3 buffers of N complex + 2 of nc complex.
__device__ __forceinline__ void gr_spatial_slice(double2 *__restrict__ y, const double2 *__restrict__ a, const double2 *__restrict__ b,
                                                 double2 *lds, int N, int ns, int L1, int L2, int L3, const double2 *__restrict__ tw,
                                                 double norm) {
    const int nc = L1 * L2 * L3;
    double2 *A = lds, *B = lds + N, *T = lds + 2 * N, *P = lds + 3 * N, *Q = P + nc;
    for (int e = threadIdx.x; e < N; e += TPB) A[e] = a[e];
    __syncthreads();
    double2 *Af = dft_cells<false>(A, T, ns, L1, L2, L3, tw);
    double2 *free1 = (Af == A) ? T : A;
    for (int e = threadIdx.x; e < N; e += TPB) B[e] = b[e];
    __syncthreads();
    double2 *Bf = dft_cells<false>(B, free1, ns, L1, L2, L3, tw);
    for (int s1 = 0; s1 < ns; ++s1) {
        for (int s2 = 0; s2 < ns; ++s2) {
            for (int q = threadIdx.x; q < nc; q += TPB) {
                const double2 av = Af[q * ns + s2], bv = Bf[q * ns + s1];
                P[q] = make_double2((av.x * bv.x + av.y * bv.y) * norm, (av.y * bv.x - av.x * bv.y) * norm);   // a·conj(b)
            }
            __syncthreads();
            double2 *Pf = dft_cells<true>(P, Q, 1, L1, L2, L3, tw);
            for (int q = threadIdx.x; q < nc; q += TPB) y[s2 + ns * (s1 + ns * q)] = Pf[q];
            __syncthreads();
        }
    }
}

// One workgroup per (frequency k, product c, chain).  The spectra of a field are [chain][K][N], the two fields of a product lie
// field_stride apart (nchains K N for a pair of spectra, 0 for an autocorrelation) and products conv_stride_in apart;
// Y[c][chain][k][s2 + ns*(s1 + ns*cell)].
__global__ void __launch_bounds__(TPB) k_gr_spatial(double2 *__restrict__ Y, const double2 *__restrict__ nuA, long long field_stride, int K, int N,
                                                    int ns, int L1, int L2, int L3, const double2 *__restrict__ tw, double norm,
                                                    long long conv_stride_in, long long conv_stride_out) {
    extern __shared__ double2 lds[];
    const int k = blockIdx.x, c = blockIdx.y, chain = blockIdx.z;
    const double2 *a = nuA + (size_t)c * conv_stride_in + ((size_t)chain * K + k) * N;
    gr_spatial_slice(Y + (size_t)c * conv_stride_out + ((size_t)chain * K + k) * ns * N, a, a + field_stride, lds, N, ns, L1, L2, L3, tw, norm);
}

// C[c][t][col] (real, Δτ < L) -> out[c][τ + 2L*col] complex for τ < 2L; the second half is sgn(c) times the first.
// 32x32 tile transpose through LDS: coalesced reads along col, coalesced writes along τ.
__global__ void __launch_bounds__(TPB) k_gr_out(double2 *__restrict__ out, const double *__restrict__ C, int L, int ncol) {
    __shared__ double tile[32][33];
    const int c = blockIdx.z;
    const double sgn = (c == 0) ? -1.0 : 1.0;
    const int col0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const double *Cc = C + (size_t)c * L * ncol;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, col = col0 + tx;
        tile[r][tx] = (t < L && col < ncol) ? Cc[(size_t)t * ncol + col] : 0.0;
    }
    __syncthreads();
    double2 *o = out + (size_t)c * 2 * L * ncol;
    for (int r = ty; r < 32; r += 8) {
        const int col = col0 + r, t = t0 + tx;
        if (t < L && col < ncol) {
            const double v = tile[tx][r];
            o[(size_t)col * 2 * L + t] = make_double2(v, 0.0);
            o[(size_t)col * 2 * L + L + t] = make_double2(sgn * v, 0.0);
        }
    }
}

template <class T>
int gr_alloc(T **p, size_t n) {
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
    HIPCHK(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return ELPH_OK;
}

size_t spatial_lds_bytes(const elph_handle_s *h, const GreensState *g) { return (3 * (size_t)h->N + 2 * (size_t)g->nc) * sizeof(double2); }

}  // namespace

void elph_greens_free(elph_handle_s *h) {
    elph_meas_free(h);                     // the measurement accumulators are shaped by the estimator
    elph_meas_chains_free(h);
    elph_bond_free(h);
    elph_bond_chains_free(h);
    elph_i_ssh_meas_free(h);
    elph_ssh_meas_chains_free(h);
    elph_ssh_bond_free(h);
    elph_ssh_bond_chains_free(h);
    elph_density_moments_free(h);
    elph_snapshots_free(h);
    elph_current_free(h);
    GreensState *g = gs_of(h);
    if (!g) return;
    void *ptrs[] = {g->R, g->X, g->tw};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    elph_i_greens_chain_scratch_free(&g->own);
    delete g;
    h->greens = nullptr;
}

extern "C" int elph_greens_create(elph_handle h, int norbits, int L1, int L2, int L3, int nv) {
    CHECK_H(h);
    if (norbits < 1 || L1 < 1 || L2 < 1 || L3 < 1 || (int64_t)norbits * L1 * L2 * L3 != h->N) {
        elph_set_error("norbits*L1*L2*L3 = %lld does not match nsites = %lld", (long long)norbits * L1 * L2 * L3, (long long)h->N);
        return ELPH_E_ARG;
    }
    elph_greens_free(h);
    GreensState *g = new GreensState();
    h->greens = g;
    g->ns = norbits; g->L1 = L1; g->L2 = L2; g->L3 = L3; g->nc = L1 * L2 * L3;
    g->nv = std::max(2, nv);                                           // GreensFunctions.jl:167
    if (spatial_lds_bytes(h, g) > 160 * 1024) {
        elph_set_error("Green's-function estimator: a frequency slice of %lld sites does not fit in 160 KB of LDS", (long long)h->N);
        elph_greens_free(h);
        return ELPH_E_UNSUPPORTED;
    }
    const size_t nd = (size_t)h->ndim, N = (size_t)h->N, L = (size_t)h->L;
    RC(gr_alloc(&g->R, (size_t)g->nv * nd));
    RC(gr_alloc(&g->X, (size_t)g->nv * nd));
    RC(elph_i_greens_chain_scratch_alloc(h, 1, &g->own));
    RC(gr_alloc(&g->own.out, 4 * 2 * L * (size_t)g->ns * N));
    std::vector<double2> tw((size_t)L1 + L2 + L3);
    size_t o = 0;
    for (int len : {L1, L2, L3}) {
        for (int j = 0; j < len; ++j) {
            const double a = 2.0 * M_PI * (double)j / (double)len;
            tw[o + j] = make_double2(cos(a), -sin(a));
        }
        o += (size_t)len;
    }
    RC(gr_alloc(&g->tw, tw.size()));
    HIPCHK(hipMemcpy(g->tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
    HIPCHK(hipFuncSetAttribute((const void *)k_gr_spatial, hipFuncAttributeMaxDynamicSharedMemorySize, (int)spatial_lds_bytes(h, g)));
    return ELPH_OK;
}

static int need_greens(elph_handle_s *h) {
    if (!h->greens) { elph_set_error("elph_greens_create has not been called"); return ELPH_E_STATE; }
    return ELPH_OK;
}

extern "C" int elph_greens_nv(elph_handle h, int *nv) {
    CHECK_H(h);
    RC(need_greens(h));
    if (nv) *nv = gs_of(h)->nv;
    return ELPH_OK;
}

// several chains resident: right-hand side r of the batch belongs to chain r % nchains, so vector v of chain c is row
// v * nchains + c of R — the estimator must then hold a multiple of nchains vectors
static int check_chain_count(const elph_handle_s *h, int nv) {
    if (h->nchains != 1 && nv % h->nchains) {
        elph_set_error("%d chains are resident: the estimator needs a multiple of that many vectors (it has %d)", h->nchains, nv);
        return ELPH_E_ARG;
    }
    return ELPH_OK;
}

// update! after its randn!: the noise vectors are in g->R (layout S).  Mᵀr, zero start, the batched solve, M⁻¹R into g->X; one synchronisation.
// A BiCGStab / GMRES handle solves M x = r₁ itself (the mul_by_M branch, :216-221): no Mᵀr, R is the right-hand side where it lies and the
// solution is written where it stays.
static int solve_from_R(elph_handle_s *h, GreensState *g, int use_precond, int64_t *iters, double *residual_error, int *flag) {
    const int nv = g->nv;
    const size_t nd = (size_t)h->ndim;
    if (h->solver_kind != ELPH_SOLVER_CG) {
        std::vector<int64_t> it((size_t)nv);
        std::vector<double> res((size_t)nv);
        std::vector<int> fl((size_t)nv);
        RC(elph_launch_zero(h, g->X, (int64_t)nv * h->ndim));              // fill!(M⁻¹r₁, 0)  :213
        h->x_zero = true;
        RC(elph_i_mldiv_core(h, 0, nv, use_precond ? 1 : 0, 0, g->X, g->R, it.data(), res.data(), fl.data()));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int i = 0; i < nv; ++i) {
            if (iters) iters[i] = it[i];
            if (residual_error) residual_error[i] = res[i];
            if (flag) flag[i] = fl[i];
        }
        g->have_vectors = true;
        return ELPH_OK;
    }
    RC(elph_launch_mul(h, 1, h->work.b, g->R, nv));                       // Mᵀr₁ (model.v″, :223-224)
    RC(elph_launch_zero(h, h->work.x, (int64_t)nv * h->ndim));            // fill!(M⁻¹r₁, 0)  :213
    h->x_zero = false;                                                 // (this path does not use the x = 0 hint, and takes nobody else's)
    std::vector<int64_t> it((size_t)nv);
    std::vector<double> res((size_t)nv);
    std::vector<int> fl((size_t)nv);
    RC(elph_i_ldiv_core(h, nv, use_precond ? 1 : 0, 0, it.data(), res.data(), fl.data()));
    HIPCHK(hipMemcpyAsync(g->X, h->work.x, (size_t)nv * nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < nv; ++i) {
        if (iters) iters[i] = it[i];
        if (residual_error) residual_error[i] = res[i];
        if (flag) flag[i] = fl[i];
    }
    g->have_vectors = true;
    return ELPH_OK;
}

// update!(estimator, model, P): the caller supplies the n_v noise vectors (the reference draws them from model.rng, :212)
extern "C" int elph_greens_update(elph_handle h, const double *R, int use_precond, int64_t *iters, double *residual_error,
                                  int *flag) {
    CHECK_H(h);
    RC(need_greens(h));
    if (!R) { elph_set_error("R is null"); return ELPH_E_ARG; }
    GreensState *g = gs_of(h);
    const int nv = g->nv;
    RC(check_chain_count(h, nv));
    RC(elph_work_reserve(h, nv));
    RC(elph_stage_in(h, g->R, R, nv));
    return solve_from_R(h, g, use_precond, iters, residual_error, flag);
}

// The estimator's own generator (independent of the HMC state's, elph_hmc_set_rng): batch b, counted since this call, is seeded with output b
// of SplitMix64(seed).  A new elph_greens_create starts without one.
extern "C" int elph_greens_set_rng(elph_handle h, uint64_t seed) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    g->rng_on = true;
    g->rng_seed = seed;
    g->rng_batches = 0;
    return ELPH_OK;
}

extern "C" int elph_greens_rng_batches(elph_handle h, uint64_t *batches) {
    CHECK_H(h);
    RC(need_greens(h));
    if (!batches) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *batches = gs_of(h)->rng_batches;
    return ELPH_OK;
}

// update!(estimator, model, P) with its randn!(R) on the device: one batch of n_v * ndim normals straight into g->R (greens_noise.hip), no
// vector crosses the bus in either direction
extern "C" int elph_greens_update_rng(elph_handle h, int use_precond, int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    if (!g->rng_on) { elph_set_error("the estimator has no generator: call elph_greens_set_rng first"); return ELPH_E_STATE; }
    const int nv = g->nv;
    RC(check_chain_count(h, nv));
    RC(elph_work_reserve(h, nv));
    RC(elph_i_greens_randn(h, g->R, sm64(g->rng_seed, ++g->rng_batches), nv));
    return solve_from_R(h, g, use_precond, iters, residual_error, flag);
}

// estimator.R / estimator.M⁻¹R as host arrays (n_v vectors of length ndim, reference layout); either may be NULL
extern "C" int elph_greens_set_vectors(elph_handle h, const double *R, const double *MinvR) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    RC(elph_work_reserve(h, g->nv));
    if (R) {
        RC(elph_stage_in(h, g->R, R, g->nv));
    }
    if (MinvR) {
        RC(elph_stage_in(h, g->X, MinvR, g->nv));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (R && MinvR) g->have_vectors = true;
    return ELPH_OK;
}

extern "C" int elph_greens_get_vectors(elph_handle h, double *R, double *MinvR) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    if (!g->have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    if (R) {
        RC(elph_stage_out(h, R, g->R, g->nv));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (MinvR) {
        RC(elph_stage_out(h, MinvR, g->X, g->nv));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return ELPH_OK;
}

// What measure.hip and bondcorr.hip read of the estimator (device pointers stay owned by it).
int elph_i_greens_view(elph_handle_s *h, ElphGreensView *v) {
    RC(need_greens(h));
    const GreensState *g = gs_of(h);
    v->ns = g->ns; v->L1 = g->L1; v->L2 = g->L2; v->L3 = g->L3; v->nc = g->nc; v->nv = g->nv;
    v->have_vectors = g->have_vectors;
    v->C = g->own.C; v->tw = g->tw;
    v->R = g->R; v->X = g->X;
    return ELPH_OK;
}

const ElphGreensChainScratch *elph_i_greens_own_scratch(elph_handle_s *h) { return h->greens ? &gs_of(h)->own : nullptr; }

// The scratch of the two pipelines below for nchains chains, sized by the estimator's shape (sizes: elph_internal.h); out stays null.
int elph_i_greens_chain_scratch_alloc(elph_handle_s *h, int nchains, ElphGreensChainScratch *S) {
    RC(need_greens(h));
    const GreensState *g = gs_of(h);
    const size_t nch = (size_t)nchains, nd = (size_t)h->ndim, N = (size_t)h->N, L = (size_t)h->L, Lo2 = (L + 1) / 2, Lh = L / 2 + 1, ncol = (size_t)g->ns * N;
    S->nchains = nchains;
    int rc = gr_alloc(&S->f, 8 * nch * nd);
    if (rc == ELPH_OK) rc = gr_alloc(&S->nuA, 2 * nch * Lo2 * N);
    if (rc == ELPH_OK) rc = gr_alloc(&S->nuP, 6 * nch * Lh * N);
    if (rc == ELPH_OK) rc = gr_alloc(&S->Y, 4 * nch * Lh * ncol);
    if (rc == ELPH_OK) rc = gr_alloc(&S->C, 4 * nch * L * ncol);
    if (rc != ELPH_OK) elph_i_greens_chain_scratch_free(S);
    return rc;
}

void elph_i_greens_chain_scratch_free(ElphGreensChainScratch *S) {
    void *ptrs[] = {S->f, S->nuA, S->nuP, S->Y, S->C, S->out};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    S->f = S->C = nullptr;
    S->nuA = S->nuP = S->Y = S->out = nullptr;
}

// The device part of setup!(estimator, n₁, n₂) for one pair of vectors of EVERY chain of S in one pass: v1, v2 count a chain's vectors
// (1-based, up to n_v = nv / nchains), vector v of chain c is row (v - 1) nchains + c of R and M⁻¹R, so the inputs of all chains are one
// contiguous block and every transform runs with its batch multiplied by nchains.  The result is the four real correlations
// S.C[table][chain][Δτ < L][s₂ + n_s (s₁ + n_s cell)] and, with `expand` (S.out: the estimator's own scratch), their doubled complex copies
// in the reference's shape; p: chain 0's vectors.  Stream-ordered: no copy to the host, no synchronisation.
static int setup_pair(elph_handle_s *h, const ElphGreensChainScratch &S, int v1, int v2, ElphGreensPair *p, bool expand) {
    GreensState *g = gs_of(h);
    const int nch = S.nchains;
    const int N = (int)h->N, L = (int)h->L, Lo2 = (L + 1) / 2, Lh = L / 2 + 1, ns = g->ns, ncol = ns * N;
    const size_t nd = (size_t)h->ndim, blk = (size_t)nch * nd;
    const long long n = (long long)blk;
    p->X1 = g->X + (size_t)(v1 - 1) * blk; p->X2 = g->X + (size_t)(v2 - 1) * blk;
    p->R1 = g->R + (size_t)(v1 - 1) * blk; p->R2 = g->R + (size_t)(v2 - 1) * blk;
    hipLaunchKernelGGL(k_gr_fields, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, S.f, p->X1, p->X2, p->R1, p->R2, n);
    RC(elph_launch_check("k_gr_fields"));
    RC(elph_dft_fwd_twisted(h, S.nuA, S.f, N, 2 * nch, nullptr));
    RC(elph_dft_fwd_plain(h, S.nuP, S.f + 2 * blk, N, 6 * nch));
    // total normalisation 1/(L·Nc)² (see header): 1/L comes from the inverse τ tables, the rest here
    const double norm = 1.0 / ((double)L * (double)g->nc * (double)g->nc);
    const size_t shm = spatial_lds_bytes(h, g);
    const long long ytab = (long long)nch * Lh * ncol;                 // one table's spectra; the twisted one fills nch Lo2 ncol of it
    hipLaunchKernelGGL(k_gr_spatial, dim3((unsigned)Lo2, 1, (unsigned)nch), dim3(TPB), shm, h->stream, S.Y, S.nuA, (long long)nch * Lo2 * N, Lo2, N, ns,
                       g->L1, g->L2, g->L3, g->tw, norm, 0LL, 0LL);
    RC(elph_launch_check("k_gr_spatial(twisted)"));
    hipLaunchKernelGGL(k_gr_spatial, dim3((unsigned)Lh, 3, (unsigned)nch), dim3(TPB), shm, h->stream, S.Y + ytab, S.nuP, (long long)nch * Lh * N, Lh,
                       N, ns, g->L1, g->L2, g->L3, g->tw, norm, 2LL * nch * Lh * N, ytab);
    RC(elph_launch_check("k_gr_spatial(plain)"));
    const size_t ctab = (size_t)nch * L * ncol;
    RC(elph_dft_inv_twisted(h, S.C, S.Y, ncol, nch, nullptr, nullptr, nullptr, 0));
    // the plain inverse walks [rhs][Lh][ncol] spectra and writes [rhs][L][ncol]
    RC(elph_dft_inv_plain(h, S.C + ctab, S.Y + ytab, ncol, 3 * nch));
    if (expand) {
        hipLaunchKernelGGL(k_gr_out, dim3((unsigned)((ncol + 31) / 32), (unsigned)((L + 31) / 32), 4), dim3(TPB), 0, h->stream, S.out, S.C, L, ncol);
        RC(elph_launch_check("k_gr_out"));
    }
    return ELPH_OK;
}

// One step of a measurement's loop over the pairs v1 < v2 of a chain's vectors (make_measurements!, Measurements.jl:550-560) in the scratch
// S.  In the estimator's own scratch the doubled complex copies are refreshed for the last pair (elph_greens_dev_arrays); in scratch a
// measurement unit owns, the estimator's scratch and tables are not touched.
int elph_i_greens_setup_chains_dev(elph_handle_s *h, const ElphGreensChainScratch &S, int v1, int v2, ElphGreensPair *p) {
    RC(need_greens(h));
    const GreensState *g = gs_of(h);
    const int nch = S.nchains;
    if (!g->have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    if (nch < 1 || g->nv % nch) { elph_set_error("the estimator's %d vectors are not a multiple of %d chains", g->nv, nch); return ELPH_E_STATE; }
    const int nvc = g->nv / nch;
    if (v1 < 1 || v1 > nvc || v2 < 1 || v2 > nvc) { elph_set_error("v1=%d, v2=%d outside 1..%d", v1, v2, nvc); return ELPH_E_ARG; }
    return setup_pair(h, S, v1, v2, p, S.out && v1 == nvc - 1);
}

// translational_average! (Utilities.jl:49-60) of a real field periodic in τ with itself, every orbital pair at once, for the nchains fields
// vS[chain][ndim] (layout S) — the plain-spectrum branch of setup! with both spectra that of v:
//   outS[chain][Δτ][a + n_s (b + n_s Δcell)] = 1/(L Nc) Σ_{τ, cell} v[τ + Δτ][a, cell + Δcell] · v[τ][b, cell]
// Uses S.nuP and S.Y: call it before, not between, elph_i_greens_setup_chains_dev and what reads S.C.
int elph_i_greens_autocorr_chains_dev(elph_handle_s *h, const ElphGreensChainScratch &S, double *outS, const double *vS) {
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    const int N = (int)h->N, L = (int)h->L, Lh = L / 2 + 1, ns = g->ns, ncol = ns * N, nch = S.nchains;
    RC(elph_dft_fwd_plain(h, S.nuP, vS, N, nch));
    const double norm = 1.0 / ((double)L * (double)g->nc * (double)g->nc);
    hipLaunchKernelGGL(k_gr_spatial, dim3((unsigned)Lh, 1, (unsigned)nch), dim3(TPB), spatial_lds_bytes(h, g), h->stream, S.Y, S.nuP, 0LL, Lh, N, ns,
                       g->L1, g->L2, g->L3, g->tw, norm, 0LL, 0LL);
    RC(elph_launch_check("k_gr_spatial(autocorrelation)"));
    RC(elph_dft_inv_plain(h, outS, S.Y, ncol, nch));
    return ELPH_OK;
}

// setup!(estimator, n₁, n₂) — n₁, n₂ 1-based.  Each output (NULL = not copied back) is Complex[2L, n_s, n_s, L1, L2, L3],
// interleaved re/im, first index fastest.  The arrays also stay on the device (elph_greens_dev_arrays).
extern "C" int elph_greens_setup(elph_handle h, int n1, int n2, double *GD0, double *GD0_GD0, double *GDD_G00, double *GD0_G0D) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    if (!g->have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    if (n1 < 1 || n1 > g->nv || n2 < 1 || n2 > g->nv) { elph_set_error("n1=%d, n2=%d outside 1..%d", n1, n2, g->nv); return ELPH_E_ARG; }
    ElphGreensPair p;
    RC(setup_pair(h, g->own, n1, n2, &p, true));
    const size_t cnt = 2 * (size_t)h->L * (size_t)g->ns * (size_t)h->N;   // complex numbers per array
    // order of the device arrays: 0 GΔ0, 1 GΔ0·GΔ0, 2 GΔΔ·G00, 3 GΔ0·G0Δ (fields 0/1, 2/3, 4/5, 6/7)
    double *outs[4] = {GD0, GD0_GD0, GDD_G00, GD0_G0D};
    for (int c = 0; c < 4; ++c)
        if (outs[c]) HIPCHK(hipMemcpyAsync(outs[c], g->own.out + (size_t)c * cnt, cnt * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// Device-resident results of the last elph_greens_setup: arrays[c] (c = 0..3 as above), `count` complex numbers each.
extern "C" int elph_greens_dev_arrays(elph_handle h, void **arrays, int64_t *count) {
    CHECK_H(h);
    RC(need_greens(h));
    GreensState *g = gs_of(h);
    const size_t cnt = 2 * (size_t)h->L * (size_t)g->ns * (size_t)h->N;
    if (arrays) for (int c = 0; c < 4; ++c) arrays[c] = (void *)(g->own.out + (size_t)c * cnt);
    if (count) *count = (int64_t)cnt;
    return ELPH_OK;
}
