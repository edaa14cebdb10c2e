// msolve.hip — BiCGStab and GMRES(restart) on M x = b or Mᵀ x = b (gfx950), the solvers behind `mul_by_M = true` models
// (IterativeSolvers.jl:354-417, :464-570; HolsteinModels.jl:286-298), with the one-sided KPM preconditioners
// (LeftRightKPMPreconditioner, KPMPreconditioners.jl:494-600) and ldiv!'s residual / flag / retry logic (Models.jl:74-186).
//
// Both solvers are batched over nrhs right-hand sides on layout-S vectors; right-hand side r uses the matrix and the expansion of chain
// r % nchains.  ONE workgroup owns one right-hand side in every kernel of this file: it sweeps the vectors with a fixed element-to-thread
// map, sums every inner product in a fixed order (wave butterfly, then the waves in order — repeated solves are bit-identical), finishes
// the solver scalars itself and keeps them in a per-right-hand-side record on the device (MsRec).  No reduction has a launch of its own,
// no scalar crosses the bus; the host reads the records once per MS_CHUNK iterations.  A finished right-hand side is skipped by every
// kernel of this file and by the Chebyshev kernel of the preconditioner (the existing mat-vec and transform kernels have no skip: they run
// on its idle vectors), so its x does not change.
//
// The right-hand sides advance in lockstep (each follows exactly the single-vector recurrences and stop rule): every running right-hand
// side is at the same iteration, and for GMRES at the same Arnoldi column, so the host drives the cycle structure and the device decides
// only who has stopped.
//
// BiCGStab, per iteration: [Left/Right apply] mat-vec k_bi_s [Left/Right apply] mat-vec k_bi_xr — two launches of its own.
//   k_bi_s    α = ρ / r̃·v, s = r - α v, |s|/|b| < tol: x += α p̂ and stop (the half-step exit)
//   k_bi_xr   ω = t·s / t·t, x += α p̂ + ω ŝ, r = s - ω t, the stop tests, and the head of the next iteration: ρ = r̃·r, β, p = r + β (p - ω v)
// Breakdown (ρ = 0, ω = 0) ends the loop and the solve returns maxiter, as the reference does.
//
// GMRES(restart), per Arnoldi step: mat-vec [Left/Right apply] k_gm_arnoldi — one launch of its own: the modified Gram-Schmidt sweep in the
// reference's order (pass k applies w -= H[k-1,i] v_{k-1} and accumulates v_k·w: one pass per k), the norm and v_{i+1}, the stored and the
// new plane rotation, the stop test, and on convergence update!.  Per cycle: k_gm_update (back-substitution by one lane, x += V y),
// mat-vec, k_gm_resid, [apply], k_gm_start.  The Krylov basis V is [restart + 1][capacity][ndim] — column-major over the batch, so that
// column i of every right-hand side is one contiguous batch for the mat-vec; it is allocated on the first GMRES solve and freed with the
// handle: (restart + 1) ndim doubles per right-hand side, 6.9 MB at 16 x 16 sites, 160 slices and restart 20.
//
// The reference as it executes: GMRES runs whole cycles; iter < maxiter (the call's) is tested between cycles only, inside a cycle only the
// tolerance and iter == solver.maxiter end it.  ONE deliberate difference: a cycle cut at iter == solver.maxiter after i < restart steps
// updates x with the i columns it built; the reference back-substitutes over all `restart` columns there (:538), reading columns this
// cycle never wrote (zero in the first cycle: 0/0).  Whenever solver.maxiter is a multiple of restart the two coincide.
//
// The callers of the solve (estimator, HMC force and action, Langevin force, special updates) reach these solvers through the handle's
// solver kind (elph_solver_set_kind) and two internals on device-resident vectors, wherever the caller has them (MsVecs): elph_i_mldiv_core,
// ldiv! of that kind, and elph_i_msolve_pair, the two-stage O⁻¹ b = M⁻¹ M⁻ᵀ b of calc_O⁻¹Λϕ! (HMC.jl:851-903).  ldiv!'s verdict on a batch is one
// kernel (k_ms_verdict: residual, flag, x zeroed), and a caller's promise that x = 0 (h->x_zero) starts either solver from r = b without the
// mat-vec on the zero batch (k_bi_init<true>, k_gm_resid<true>) — the same bits.

#include <chrono>
#include <cmath>

#include "elph_internal.h"

#define MS_CHUNK 4          // iterations (Arnoldi steps) between two reads of the records by the host
#define MS_NVEC 12          // work vectors per right-hand side

namespace {

struct MsRec {              // one right-hand side
    double normb, rho, alpha, omega, eps;
    long long it;           // BiCGStab: the iteration in progress
    long long iters;        // what solve! returns (valid once done)
    int done;               // 0 running, 1 tolerance, 2 breakdown, 3 out of iterations
    int pad;
};

struct MsVerdict { double resid; int flag, pad; };      // ldiv!'s residual_error and flag of one right-hand side

struct MsolveState {
    int cap = 0;                   // right-hand sides the buffers hold
    double *vec = nullptr;         // [MS_NVEC][cap][ndim]
    MsRec *rec = nullptr, *h_rec = nullptr;      // [cap]; pinned
    int *done = nullptr;           // [cap] mirror of rec.done for the preconditioner's kernel
    MsVerdict *verd = nullptr, *h_verd = nullptr;      // [cap] k_ms_verdict's output; pinned
    double *V = nullptr;           // GMRES: [restart + 1][cap][ndim]
    double *gm = nullptr;          // GMRES: per right-hand side H [(R+1) R] column-major | s | cs | sn | y, each R + 1
    int V_restart = 0, V_cap = 0;
};

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, ELPH_WAVE);
    return v;
}

// the sum over the workgroup in EVERY thread, the same bits in each: wave butterfly, then the waves in order.  sc: 16 doubles of LDS
__device__ __forceinline__ double ms_block_sum(double v, double *sc) {
    v = ms_wave_sum(v);
    const int nw = blockDim.x / ELPH_WAVE;
    __syncthreads();
    if ((threadIdx.x & (ELPH_WAVE - 1)) == 0) sc[threadIdx.x / ELPH_WAVE] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += sc[w];
    return t;
}

// ------------------------------------------------------------------------------------------ BiCGStab (IterativeSolvers.jl:354-417)

struct BiBufs { double *x, *r, *rt, *p, *ph, *s, *sh, *v, *t; const double *b; MsRec *rec; int *done; long long nd; };

// r = b - A x0 (A x0 in B.t), r̃ = r, and the head of iteration 1: ρ = r̃·r, β = 0, p = r.  ZERO: x0 = 0 by the caller's promise — r = b
// without the mat-vec (A 0 is exactly 0 and b - 0 = b: the same bits), B.t is not read
template <bool ZERO>
__global__ void __launch_bounds__(1024) k_bi_init(BiBufs B, long long maxiter) {
    __shared__ double sc[32];
    const int rhs = blockIdx.x;
    const size_t o = (size_t)rhs * (size_t)B.nd;
    double bb = 0.0, rr = 0.0;
    for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) {
        const double bv = B.b[o + i], rv = ZERO ? bv : bv - B.t[o + i];
        B.r[o + i] = rv; B.rt[o + i] = rv; B.p[o + i] = rv; B.v[o + i] = 0.0;
        bb += bv * bv; rr += rv * rv;
    }
    bb = ms_block_sum(bb, sc);
    rr = ms_block_sum(rr, sc + 16);
    if (threadIdx.x == 0) {
        MsRec R;
        R.normb = sqrt(bb); R.rho = rr; R.alpha = 0.0; R.omega = 1.0; R.eps = sqrt(rr) / R.normb;
        R.it = 1; R.iters = maxiter; R.done = (rr == 0.0) ? 2 : 0; R.pad = 0;      // ρ = 0: break, return maxiter (:388-390, :416)
        B.rec[rhs] = R;
        B.done[rhs] = R.done;
    }
}

// v = A p̂ is in:  α = ρ / r̃·v, s = r - α v, ϵ = |s| / |b| < tol: x += α p̂, return i  (:395-401)
__global__ void __launch_bounds__(1024) k_bi_s(BiBufs B, double tol) {
    __shared__ double sc[16];
    const int rhs = blockIdx.x;
    MsRec R = B.rec[rhs];
    if (R.done) return;
    const size_t o = (size_t)rhs * (size_t)B.nd;
    double rtv = 0.0;
    for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) rtv += B.rt[o + i] * B.v[o + i];
    rtv = ms_block_sum(rtv, sc);
    const double alpha = R.rho / rtv;
    double ss = 0.0;
    for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) {
        const double sv = B.r[o + i] - alpha * B.v[o + i];
        B.s[o + i] = sv;
        ss += sv * sv;
    }
    ss = ms_block_sum(ss, sc);
    const double eps = sqrt(ss) / R.normb;
    const bool stop = eps < tol;
    if (stop)
        for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) B.x[o + i] += alpha * B.ph[o + i];
    if (threadIdx.x == 0) {
        R.alpha = alpha; R.eps = eps;
        if (stop) { R.done = 1; R.iters = R.it; B.done[rhs] = 1; }
        B.rec[rhs] = R;
    }
}

// t = A ŝ is in:  ω = t·s / t·t, x += α p̂ + ω ŝ, r = s - ω t, the stop tests (:404-413); then the head of the next iteration (:386-392)
__global__ void __launch_bounds__(1024) k_bi_xr(BiBufs B, double tol, long long maxiter) {
    __shared__ double sc[32];
    const int rhs = blockIdx.x;
    MsRec R = B.rec[rhs];
    if (R.done) return;
    const size_t o = (size_t)rhs * (size_t)B.nd;
    double ts = 0.0, tt = 0.0;
    for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) {
        const double tv = B.t[o + i];
        ts += tv * B.s[o + i]; tt += tv * tv;
    }
    ts = ms_block_sum(ts, sc);
    tt = ms_block_sum(tt, sc + 16);
    const double omega = ts / tt, alpha = R.alpha;
    double rr = 0.0, rtr = 0.0;
    for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) {
        B.x[o + i] += alpha * B.ph[o + i] + omega * B.sh[o + i];
        const double rv = B.s[o + i] - omega * B.t[o + i];
        B.r[o + i] = rv;
        rr += rv * rv; rtr += B.rt[o + i] * rv;
    }
    rr = ms_block_sum(rr, sc);
    rtr = ms_block_sum(rtr, sc + 16);
    const double eps = sqrt(rr) / R.normb;
    int done = 0;
    long long iters = maxiter;
    if (eps < tol) { done = 1; iters = R.it; }
    else if (omega == 0.0) done = 2;
    else if (R.it >= maxiter) done = 3;
    else if (rtr == 0.0) done = 2;
    if (!done) {
        const double beta = (rtr / R.rho) * (alpha / omega);
        for (long long i = threadIdx.x; i < B.nd; i += blockDim.x) B.p[o + i] = B.r[o + i] + beta * (B.p[o + i] - omega * B.v[o + i]);
    }
    if (threadIdx.x == 0) {
        R.omega = omega; R.eps = eps;
        if (done) { R.done = done; R.iters = iters; B.done[rhs] = done; }
        else { R.rho = rtr; R.it += 1; }
        B.rec[rhs] = R;
    }
}

// ------------------------------------------------------------------------------------------ GMRES (IterativeSolvers.jl:464-584)

struct GmBufs {
    double *x, *V, *w, *r, *gm;
    const double *b, *pb;          // pb: b with the preconditioner applied (b itself without one)
    MsRec *rec; int *done;
    long long nd, vstride;         // vstride: cap * ndim, the distance between two columns of V
    int R;                         // restart
};
__device__ __forceinline__ double *gm_H(const GmBufs &G, int rhs) { return G.gm + (size_t)rhs * ((size_t)(G.R + 1) * (G.R + 4)); }

// update!(x, k, H, s, y, V) (:552-570) for the workgroup's right-hand side; y: R + 1 doubles of LDS
__device__ __forceinline__ void gm_update(const GmBufs &G, int rhs, int k, double *y) {
    const int R1 = G.R + 1;
    const double *H = gm_H(G, rhs), *s = H + (size_t)R1 * G.R;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < R1; ++i) y[i] = s[i];
        for (int i = k - 1; i >= 0; --i) {
            y[i] /= H[i + (size_t)R1 * i];
            for (int j = i - 1; j >= 0; --j) y[j] -= H[j + (size_t)R1 * i] * y[i];
        }
    }
    __syncthreads();
    const size_t o = (size_t)rhs * (size_t)G.nd;
    for (long long i = threadIdx.x; i < G.nd; i += blockDim.x) {
        double xv = G.x[o + i];
        for (int j = 0; j < k; ++j) xv += y[j] * G.V[(size_t)j * G.vstride + o + i];
        G.x[o + i] = xv;
    }
}

// r = b - A x (A x in G.w) for the running right-hand sides (:493-494, :539-540).  ZERO (the first residual only): x = 0 by the caller's
// promise — r = b without the mat-vec, G.w is not read
template <bool ZERO>
__global__ void __launch_bounds__(1024) k_gm_resid(GmBufs G, int first) {
    const int rhs = blockIdx.x;
    if (!first && G.rec[rhs].done) return;
    const size_t o = (size_t)rhs * (size_t)G.nd;
    for (long long i = threadIdx.x; i < G.nd; i += blockDim.x) G.r[o + i] = ZERO ? G.b[o + i] : G.b[o + i] - G.w[o + i];
}

// r = P⁻¹ (b - A x) is in (first: and pb = P⁻¹ b: normb, :485-490):  β = |r|, ϵ = β / normb < tol: return iter; iter >= maxiter: return iter
// (the while test, :507); else a new cycle: V[:,1] = r / β, s = (β, 0, ...)  (:508-510)
__global__ void __launch_bounds__(1024) k_gm_start(GmBufs G, int first, long long iter, long long maxiter, double tol) {
    __shared__ double sc[32];
    const int rhs = blockIdx.x;
    MsRec R;
    if (first) { R.normb = 1.0; R.rho = R.alpha = R.omega = R.eps = 0.0; R.it = 0; R.iters = 0; R.done = 0; R.pad = 0; }
    else R = G.rec[rhs];
    if (R.done) return;
    const size_t o = (size_t)rhs * (size_t)G.nd;
    if (first) {
        double bb = 0.0;
        for (long long i = threadIdx.x; i < G.nd; i += blockDim.x) { const double v = G.pb[o + i]; bb += v * v; }
        bb = ms_block_sum(bb, sc + 16);
        R.normb = sqrt(bb);
        if (R.normb == 0.0) R.normb = 1.0;
    }
    double rr = 0.0;
    for (long long i = threadIdx.x; i < G.nd; i += blockDim.x) { const double v = G.r[o + i]; rr += v * v; }
    rr = ms_block_sum(rr, sc);
    const double beta = sqrt(rr);
    R.eps = beta / R.normb;
    R.it = iter;
    if (R.eps < tol) { R.done = 1; R.iters = iter; }
    else if (iter >= maxiter) { R.done = 3; R.iters = iter; }
    else {
        for (long long i = threadIdx.x; i < G.nd; i += blockDim.x) G.V[o + i] = G.r[o + i] / beta;
        double *s = gm_H(G, rhs) + (size_t)(G.R + 1) * G.R;
        for (int i = threadIdx.x; i <= G.R; i += blockDim.x) s[i] = (i == 0) ? beta : 0.0;
    }
    if (threadIdx.x == 0) { G.rec[rhs] = R; G.done[rhs] = R.done; }
}

// Arnoldi step i (0-based) of the cycle, w = P⁻¹ A v_i is in (:516-533)
__global__ void __launch_bounds__(1024) k_gm_arnoldi(GmBufs G, int i, long long iter, double tol) {
    extern __shared__ double y[];          // R + 1
    __shared__ double sc[16];
    const int rhs = blockIdx.x;
    if (G.rec[rhs].done) return;
    const double normb = G.rec[rhs].normb;
    const int R1 = G.R + 1;
    const size_t o = (size_t)rhs * (size_t)G.nd;
    double *H = gm_H(G, rhs), *Hi = H + (size_t)R1 * i, *s = H + (size_t)R1 * G.R, *cs = s + R1, *sn = cs + R1;
    double *w = G.w + o;
    // modified Gram-Schmidt: pass k applies the previous projection and accumulates v_k·w; the last pass accumulates |w|²
    double hprev = 0.0;
    for (int k = 0; k <= i + 1; ++k) {
        const double *vk = G.V + (size_t)k * G.vstride + o, *vp = G.V + (size_t)(k > 0 ? k - 1 : 0) * G.vstride + o;
        double acc = 0.0;
        for (long long e = threadIdx.x; e < G.nd; e += blockDim.x) {
            double wv = w[e];
            if (k > 0) { wv -= hprev * vp[e]; w[e] = wv; }
            acc += (k <= i) ? vk[e] * wv : wv * wv;
        }
        acc = ms_block_sum(acc, sc);
        hprev = (k <= i) ? acc : sqrt(acc);
        if (threadIdx.x == 0) Hi[k] = hprev;
    }
    {
        double *vn = G.V + (size_t)(i + 1) * G.vstride + o;
        for (long long e = threadIdx.x; e < G.nd; e += blockDim.x) vn[e] = w[e] / hprev;
    }
    __syncthreads();                       // Hi[] of thread 0 is read below by thread 0 only; the barrier orders the V writes before gm_update
    double eps = 0.0;
    if (threadIdx.x == 0) {
        for (int k = 0; k < i; ++k) {      // the stored rotations (:523-525)
            const double a = Hi[k], b = Hi[k + 1];
            Hi[k] = cs[k] * a + sn[k] * b;
            Hi[k + 1] = -sn[k] * a + cs[k] * b;
        }
        // cos, sin of angle(dx + i dy) (:579-584) as (dx, dy) / |(dx, dy)|, scaled by the larger component; angle(0) = 0
        const double dx = Hi[i], dy = Hi[i + 1], big = fmax(fabs(dx), fabs(dy));
        const double ux = (big == 0.0) ? 1.0 : dx / big, uy = (big == 0.0) ? 0.0 : dy / big, hyp = sqrt(ux * ux + uy * uy);
        const double c = ux / hyp, sv = uy / hyp;
        cs[i] = c; sn[i] = sv;
        Hi[i] = c * dx + sv * dy;
        Hi[i + 1] = -sv * dx + c * dy;
        const double a = s[i], b = s[i + 1];
        s[i] = c * a + sv * b;
        s[i + 1] = -sv * a + c * b;
        eps = fabs(s[i + 1]) / normb;
        sc[0] = eps;
    }
    __syncthreads();
    eps = sc[0];
    if (eps < tol) gm_update(G, rhs, i + 1, y);
    if (threadIdx.x == 0) {
        MsRec *rec = G.rec + rhs;
        rec->eps = eps; rec->it = iter;
        if (eps < tol) { rec->done = 1; rec->iters = iter; G.done[rhs] = 1; }
    }
}

// the end of a cycle: update!(x, k, ...) for the running right-hand sides (:538; k: the columns this cycle built)
__global__ void __launch_bounds__(1024) k_gm_update(GmBufs G, int k) {
    extern __shared__ double y[];
    const int rhs = blockIdx.x;
    if (G.rec[rhs].done) return;
    gm_update(G, rhs, k, y);
}

// ------------------------------------------------------------------------------------------ the true residual of ldiv! (Models.jl:93-97)

// The verdict of ldiv! on the whole batch (Models.jl:93-126, :150-183): residual_error = |A x - b| / |b| (A x in ax); above sqrt(tol)
// (NaN compares false, as in the reference) the flag is 1 — out of iterations: the record's iters == cmp_maxiter — or 2, and x is zeroed
// (fill!(x, 0)); else 0.  out[rhs] = {residual_error, flag}
__global__ void __launch_bounds__(1024) k_ms_verdict(MsVerdict *__restrict__ out, double *__restrict__ x, const double *__restrict__ ax,
                                                     const double *__restrict__ b, const MsRec *__restrict__ rec, long long nd,
                                                     double sqrt_tol, long long cmp_maxiter) {
    __shared__ double sc[32];
    const int rhs = blockIdx.x;
    const size_t o = (size_t)rhs * (size_t)nd;
    double a = 0.0, c = 0.0;
    for (long long i = threadIdx.x; i < nd; i += blockDim.x) {
        const double bv = b[o + i], d = ax[o + i] - bv;
        a += d * d; c += bv * bv;
    }
    a = ms_block_sum(a, sc);
    c = ms_block_sum(c, sc + 16);
    const double resid = sqrt(a) / sqrt(c);
    const bool flagged = resid > sqrt_tol;
    if (flagged)
        for (long long i = threadIdx.x; i < nd; i += blockDim.x) x[o + i] = 0.0;
    if (threadIdx.x == 0) {
        MsVerdict v;
        v.resid = resid; v.flag = flagged ? ((rec[rhs].iters == cmp_maxiter) ? 1 : 2) : 0; v.pad = 0;
        out[rhs] = v;
    }
}

// ------------------------------------------------------------------------------------------ host

MsolveState *ms_state(elph_handle_s *h) { return static_cast<MsolveState *>(h->msolve); }

template <class T>
int ms_alloc(T **p, size_t n) {
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
    HIPCHK(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return ELPH_OK;
}

int ms_reserve(elph_handle_s *h, int nrhs, int restart /* 0: BiCGStab */) {
    if (!h->msolve) h->msolve = new MsolveState();
    MsolveState *S = ms_state(h);
    RC(elph_work_reserve(h, nrhs));
    const size_t nd = (size_t)h->ndim;
    if (nrhs > S->cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        RC(ms_alloc(&S->vec, (size_t)MS_NVEC * nrhs * nd));
        RC(ms_alloc(&S->rec, (size_t)nrhs));
        RC(ms_alloc(&S->done, (size_t)nrhs));
        RC(ms_alloc(&S->verd, (size_t)nrhs));
        if (S->h_rec) HIPCHK(hipHostFree(S->h_rec));
        if (S->h_verd) HIPCHK(hipHostFree(S->h_verd));
        S->h_rec = nullptr; S->h_verd = nullptr;
        HIPCHK(hipHostMalloc((void **)&S->h_rec, (size_t)nrhs * sizeof(MsRec), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&S->h_verd, (size_t)nrhs * sizeof(MsVerdict), hipHostMallocDefault));
        S->cap = nrhs;
    }
    if (restart > 0 && (restart > S->V_restart || S->cap > S->V_cap)) {
        HIPCHK(hipStreamSynchronize(h->stream));
        const int R = std::max(restart, S->V_restart);
        RC(ms_alloc(&S->V, (size_t)(R + 1) * S->cap * nd));
        RC(ms_alloc(&S->gm, (size_t)S->cap * (size_t)(R + 1) * (R + 4)));
        S->V_restart = R; S->V_cap = S->cap;
    }
    return ELPH_OK;
}

double *ms_vec(elph_handle_s *h, int k) { MsolveState *S = ms_state(h); return S->vec + (size_t)k * S->cap * (size_t)h->ndim; }

int ms_block(const elph_handle_s *h) {        // threads of a workgroup: a wave per 256 elements, 1 ... 16 waves
    const long long waves = (h->ndim + 255) / 256;
    return ELPH_WAVE * (int)std::min<long long>(16, std::max<long long>(1, waves));
}

// the records to the host; *all_done, and iters[] of the finished ones
int ms_read(elph_handle_s *h, int nrhs, int64_t *iters, bool *all_done) {
    MsolveState *S = ms_state(h);
    HIPCHK(hipMemcpyAsync(S->h_rec, S->rec, (size_t)nrhs * sizeof(MsRec), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *all_done = true;
    for (int r = 0; r < nrhs; ++r) {
        if (!S->h_rec[r].done) *all_done = false;
        else iters[r] = (int64_t)S->h_rec[r].iters;
    }
    return ELPH_OK;
}

int ms_apply(elph_handle_s *h, double *z, const double *r, int nrhs, int transposed) {
    return elph_launch_kpm_apply_side(h, z, r, nrhs, transposed, ms_state(h)->done);
}

// where a solve has its right-hand sides and its solutions ([nrhs][ndim], layout S), and whether x is zero by the caller's promise
struct MsVecs { double *x; const double *b; bool x_zero; };

// solve!(x, A, b, bicgstab[, P])
int run_bicgstab(elph_handle_s *h, MsVecs U, int transposed, int nrhs, int use_prec, double tol, int64_t maxiter, int64_t *iters) {
    RC(ms_reserve(h, nrhs, 0));
    MsolveState *S = ms_state(h);
    BiBufs B;
    B.x = U.x; B.b = U.b; B.rec = S->rec; B.done = S->done; B.nd = h->ndim;
    B.r = ms_vec(h, 0); B.rt = ms_vec(h, 1); B.p = ms_vec(h, 2); B.s = ms_vec(h, 3); B.v = ms_vec(h, 4); B.t = ms_vec(h, 5);
    B.ph = use_prec ? ms_vec(h, 6) : B.p;
    B.sh = use_prec ? ms_vec(h, 7) : B.s;
    const int which = transposed ? 1 : 0, bs = ms_block(h);
    if (!U.x_zero) RC(elph_launch_mul(h, which, B.t, B.x, nrhs));
    hipLaunchKernelGGL(U.x_zero ? k_bi_init<true> : k_bi_init<false>, dim3((unsigned)nrhs), dim3((unsigned)bs), 0, h->stream, B,
                       (long long)maxiter);
    RC(elph_launch_check("k_bi_init"));
    bool all_done = false;
    for (int64_t i = 0; i < maxiter && !all_done; ++i) {
        if (use_prec) RC(ms_apply(h, B.ph, B.p, nrhs, transposed));
        RC(elph_launch_mul(h, which, B.v, B.ph, nrhs));
        hipLaunchKernelGGL(k_bi_s, dim3((unsigned)nrhs), dim3((unsigned)bs), 0, h->stream, B, tol);
        if (use_prec) RC(ms_apply(h, B.sh, B.s, nrhs, transposed));
        RC(elph_launch_mul(h, which, B.t, B.sh, nrhs));
        hipLaunchKernelGGL(k_bi_xr, dim3((unsigned)nrhs), dim3((unsigned)bs), 0, h->stream, B, tol, (long long)maxiter);
        RC(elph_launch_check("k_bi_xr"));
        if ((i + 1) % MS_CHUNK == 0 || i + 1 == maxiter) RC(ms_read(h, nrhs, iters, &all_done));
    }
    if (!all_done) { elph_set_error("BiCGStab ended without a terminal state (internal error)"); return ELPH_E_STATE; }
    return ELPH_OK;
}

// solve!(x, A, b, gmres[, M])
int run_gmres(elph_handle_s *h, MsVecs U, int transposed, int nrhs, int use_prec, double tol, int64_t maxiter, int64_t solver_maxiter, int restart,
              int64_t *iters) {
    RC(ms_reserve(h, nrhs, restart));
    MsolveState *S = ms_state(h);
    GmBufs G;
    G.x = U.x; G.b = U.b; G.V = S->V; G.gm = S->gm; G.rec = S->rec; G.done = S->done;
    G.nd = h->ndim; G.vstride = (long long)S->cap * h->ndim; G.R = restart;
    double *w_raw = ms_vec(h, 8), *r_raw = ms_vec(h, 9);
    G.w = use_prec ? ms_vec(h, 10) : w_raw;
    G.r = r_raw;
    G.pb = use_prec ? ms_vec(h, 11) : U.b;
    const int which = transposed ? 1 : 0, bs = ms_block(h);
    const size_t shm = (size_t)(restart + 1) * sizeof(double);
    const dim3 grid((unsigned)nrhs), block((unsigned)bs);
    HIPCHK(hipMemsetAsync(S->done, 0, (size_t)nrhs * sizeof(int), h->stream));
    if (use_prec) RC(ms_apply(h, ms_vec(h, 11), U.b, nrhs, transposed));

    // r = P⁻¹ (b - A x), then the tests between two cycles and the start of the next one
    auto residual_and_start = [&](int first, int64_t iter) -> int {
        double *ax = use_prec ? ms_vec(h, 10) : w_raw;
        GmBufs Gr = G; Gr.w = ax;
        const bool zero = first && U.x_zero;
        if (!zero) RC(elph_launch_mul(h, which, ax, G.x, nrhs));
        hipLaunchKernelGGL(zero ? k_gm_resid<true> : k_gm_resid<false>, grid, block, 0, h->stream, Gr, first);
        if (use_prec) RC(ms_apply(h, r_raw, r_raw, nrhs, transposed));
        hipLaunchKernelGGL(k_gm_start, grid, block, 0, h->stream, G, first, (long long)iter, (long long)maxiter, tol);
        return elph_launch_check("k_gm_start");
    };

    int64_t iter = 0;
    bool all_done = false;
    RC(residual_and_start(1, 0));
    RC(ms_read(h, nrhs, iters, &all_done));
    while (!all_done) {
        int cols = 0;
        for (int i = 0; i < restart && !all_done; ++i) {
            ++iter;
            RC(elph_launch_mul(h, which, w_raw, G.V + (size_t)i * (size_t)G.vstride, nrhs));
            if (use_prec) RC(ms_apply(h, G.w, w_raw, nrhs, transposed));
            hipLaunchKernelGGL(k_gm_arnoldi, grid, block, shm, h->stream, G, i, (long long)iter, tol);
            RC(elph_launch_check("k_gm_arnoldi"));
            cols = i + 1;
            if (iter == solver_maxiter) break;                                   // (:534)
            if (cols % MS_CHUNK == 0 && cols < restart) RC(ms_read(h, nrhs, iters, &all_done));
        }
        if (all_done) break;
        hipLaunchKernelGGL(k_gm_update, grid, block, shm, h->stream, G, cols);
        RC(residual_and_start(0, iter));
        RC(ms_read(h, nrhs, iters, &all_done));
    }
    return ELPH_OK;
}

int need_ready(elph_handle_s *h, int solver, int transposed, int nrhs, int use_prec, int restart) {
    (void)transposed;
    if (!h->have_E) { elph_set_error("update_model has not been called on this handle"); return ELPH_E_STATE; }
    const char *name = solver == ELPH_SOLVER_GMRES ? "GMRES" : "BiCGStab";
    if (h->shard || h->is_slab) { elph_set_error("%s does not run on a sharded or slab handle", name); return ELPH_E_STATE; }
    if (h->dot_hi > 0) { elph_set_error("%s does not run with a restricted inner-product range", name); return ELPH_E_STATE; }
    if (solver != ELPH_SOLVER_BICGSTAB && solver != ELPH_SOLVER_GMRES) { elph_set_error("solver: 1 BiCGStab, 2 GMRES"); return ELPH_E_ARG; }
    if (nrhs < 1) { elph_set_error("nrhs < 1"); return ELPH_E_ARG; }
    if (solver == ELPH_SOLVER_GMRES && (restart < 1 || restart > 1024)) { elph_set_error("GMRES restart outside 1 ... 1024"); return ELPH_E_ARG; }
    if (use_prec && !h->kpm.ready) { elph_set_error("preconditioned solve requested before elph_kpm_setup"); return ELPH_E_STATE; }
    return ELPH_OK;
}

int ms_solve(elph_handle_s *h, MsVecs U, int solver, int transposed, int nrhs, int use_prec, double tol, int64_t maxiter,
             int64_t solver_maxiter, int restart, int64_t *iters) {
    h->x_zero = false;                       // (a promise belongs to one solve: the callers hand it on in U)
    if (solver == ELPH_SOLVER_BICGSTAB) return run_bicgstab(h, U, transposed, nrhs, use_prec, tol, maxiter, iters);
    return run_gmres(h, U, transposed, nrhs, use_prec, tol, maxiter, solver_maxiter, restart, iters);
}

// residual_error and flag of ldiv! for the solve the records belong to; x zeroed where the flag is positive: one launch, one read
int ms_residual_and_flags(elph_handle_s *h, MsVecs U, int transposed, int nrhs, int64_t cmp_maxiter, double *resid, int *flag) {
    MsolveState *S = ms_state(h);
    double *ax = ms_vec(h, 8);
    RC(elph_launch_mul(h, transposed ? 1 : 0, ax, U.x, nrhs));
    hipLaunchKernelGGL(k_ms_verdict, dim3((unsigned)nrhs), dim3((unsigned)ms_block(h)), 0, h->stream, S->verd, U.x, (const double *)ax, U.b,
                       (const MsRec *)S->rec, (long long)h->ndim, sqrt(h->tol), (long long)cmp_maxiter);
    RC(elph_launch_check("k_ms_verdict"));
    HIPCHK(hipMemcpyAsync(S->h_verd, S->verd, sizeof(MsVerdict) * (size_t)nrhs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int r = 0; r < nrhs; ++r) { resid[r] = S->h_verd[r].resid; flag[r] = S->h_verd[r].flag; }
    return ELPH_OK;
}

// ldiv! of U.b into U.x
int ms_ldiv(elph_handle_s *h, MsVecs U, int solver, int transposed, int nrhs, int use_prec, int64_t maxiter, int restart, int64_t *iters,
            double *resid, int *flag) {
    if (maxiter == 0) maxiter = h->maxiter;                                                       // Models.jl:78-80, :143-145
    RC(ms_solve(h, U, solver, transposed, nrhs, use_prec, h->tol, maxiter, h->maxiter, restart, iters));
    RC(ms_residual_and_flags(h, U, transposed, nrhs, use_prec ? maxiter : h->maxiter, resid, flag));      // :103 maxiter, :160 solver.maxiter
    if (!use_prec) return ELPH_OK;
    // flagged right-hand sides: again without the preconditioner, from x = 0 (zeroed above), 10 x maxiter (:129-133), one at a time in slot 0
    const MsVecs U0 = {U.x, U.b, true};
    for (int r = 0; r < nrhs; ++r) {
        if (flag[r] == 0) continue;
        int64_t it1 = 0; double rs1 = 0; int fl1 = 0;
        RC(elph_retry_in_slot0(h, r, [&]() -> int {
            RC(ms_solve(h, U0, solver, transposed, 1, 0, h->tol, 10 * maxiter, h->maxiter, restart, &it1));
            return ms_residual_and_flags(h, U0, transposed, 1, h->maxiter, &rs1, &fl1);
        }, U.x, const_cast<double *>(U.b)));
        iters[r] = it1; resid[r] = rs1; flag[r] = fl1;
    }
    return ELPH_OK;
}

int default_restart(const elph_handle_s *h, int restart) { return restart < 0 ? (int)std::min<int64_t>(20, h->ndim) : restart; }      // :448-450

}  // namespace

void elph_msolve_free(elph_handle_s *h) {
    MsolveState *S = ms_state(h);
    if (!S) return;
    void *ptrs[] = {S->vec, S->rec, S->done, S->verd, S->V, S->gm};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (S->h_rec) (void)hipHostFree(S->h_rec);
    if (S->h_verd) (void)hipHostFree(S->h_verd);
    delete S;
    h->msolve = nullptr;
}

int elph_i_mldiv_core(elph_handle_s *h, int transposed, int nrhs, int use_prec, int64_t maxiter, double *x, const double *b, int64_t *iters,
                      double *resid, int *flag) {
    const bool x_zero = h->x_zero;           // the promise belongs to THIS solve: consumed before anything can return
    h->x_zero = false;
    const int solver = h->solver_kind, restart = solver == ELPH_SOLVER_GMRES ? h->solver_restart : 0;
    RC(need_ready(h, solver, transposed, nrhs, use_prec, restart));
    RC(ms_reserve(h, nrhs, restart));
    const MsVecs U = {x, b, x_zero};
    return ms_ldiv(h, U, solver, transposed ? 1 : 0, nrhs, use_prec ? 1 : 0, maxiter, restart, iters, resid, flag);
}

int elph_i_msolve_ready(elph_handle_s *h) { return need_ready(h, h->solver_kind, 0, 1, 0, h->solver_restart); }

// promise: hand the stages the zero-guess promise (the callers); false: they compute A·0 (elph_bench_msolve_pair's comparison)
static int msolve_pair(elph_handle_s *h, int nrhs, int use_prec, double *x, double *y, const double *b, int64_t *iters2, int *flag2,
                       bool promise) {
    const size_t bytes = (size_t)nrhs * (size_t)h->ndim * sizeof(double);
    std::vector<double> res((size_t)nrhs);
    HIPCHK(hipMemsetAsync(y, 0, bytes, h->stream));                // fill!(M⁻ᵀΛϕ, 0)  (HMC.jl:862)
    h->x_zero = promise;
    RC(elph_i_mldiv_core(h, 1, nrhs, use_prec, 0, y, b, iters2, res.data(), flag2));
    HIPCHK(hipMemsetAsync(x, 0, bytes, h->stream));                // fill!(O⁻¹Λϕ, 0)  (:869)
    h->x_zero = promise;
    return elph_i_mldiv_core(h, 0, nrhs, use_prec, 0, x, y, iters2 + nrhs, res.data(), flag2 + nrhs);
}

int elph_i_msolve_pair(elph_handle_s *h, int nrhs, int use_prec, double *x, double *y, const double *b, int64_t *iters2, int *flag2) {
    return msolve_pair(h, nrhs, use_prec, x, y, b, iters2, flag2, true);
}

extern "C" int elph_bench_msolve_pair(elph_handle h, int nrhs, int use_precond, int zero_start, int reps, double *ms_total, int64_t *iters) {
    CHECK_H(h);
    if (nrhs < 1 || reps < 1 || !ms_total) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (h->solver_kind == ELPH_SOLVER_CG) { elph_set_error("the handle's solver is CG: elph_solver_set_kind first"); return ELPH_E_STATE; }
    if (nrhs > h->work.cap_rhs) { elph_set_error("%d right-hand sides asked for, the last evaluation left %d", nrhs, h->work.cap_rhs); return ELPH_E_ARG; }
    std::vector<int64_t> it2((size_t)2 * nrhs, 0);
    std::vector<int> fl2((size_t)2 * nrhs, 0);
    HIPCHK(hipStreamSynchronize(h->stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r)
        RC(msolve_pair(h, nrhs, use_precond ? 1 : 0, h->work.x, h->work.z, h->work.b, it2.data(), fl2.data(), zero_start != 0));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (iters) std::copy(it2.begin(), it2.end(), iters);
    return ELPH_OK;
}

extern "C" int elph_bench_kpm_side_info(elph_handle h, int *out) {
    CHECK_H(h);
    if (!out) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const KpmSlabShape sh = elph_kpm_slab_shape(h);
    out[0] = sh.cbs; out[1] = sh.npl; out[2] = sh.lds_tables;
    out[3] = sh.npl > ELPH_SIDE_NPL_MAX ? 1 : 0;
    out[4] = ms_block(h);
    return ELPH_OK;
}

extern "C" int elph_solver_set_kind(elph_handle h, int solver, int restart) {
    CHECK_H(h);
    if (solver != ELPH_SOLVER_CG && solver != ELPH_SOLVER_BICGSTAB && solver != ELPH_SOLVER_GMRES) {
        elph_set_error("solver: 0 CG, 1 BiCGStab, 2 GMRES");
        return ELPH_E_ARG;
    }
    if (solver == ELPH_SOLVER_GMRES) {
        restart = default_restart(h, restart);
        if (restart < 1 || restart > 1024) { elph_set_error("GMRES restart outside 1 ... 1024"); return ELPH_E_ARG; }
        h->solver_restart = restart;
    }
    h->solver_kind = solver;
    return ELPH_OK;
}

extern "C" int elph_kpm_apply_side(elph_handle h, int nvec, double *vout, const double *vin, int transposed) {
    CHECK_H(h);
    if (!vout || !vin || nvec < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (!h->kpm.ready) { elph_set_error("elph_kpm_setup has not been called"); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, nvec));
    RC(elph_stage_in(h, h->work.r, vin, nvec));
    RC(elph_launch_kpm_apply_side(h, h->work.zp, h->work.r, nvec, transposed ? 1 : 0, nullptr));
    RC(elph_stage_out(h, vout, h->work.zp, nvec));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_msolve(elph_handle h, int solver, int transposed, int nrhs, double *X, const double *B, int use_precond, double tol,
                           int64_t maxiter, int64_t solver_maxiter, int restart, int64_t *iters) {
    CHECK_H(h);
    if (!X || !B || !iters || maxiter < 0 || solver_maxiter < 0 || tol < 0.0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    restart = default_restart(h, restart);
    RC(need_ready(h, solver, transposed, nrhs, use_precond, restart));
    if (tol == 0.0) tol = h->tol;                                  // iszero() defaults, IterativeSolvers.jl:376-382, :476-482
    if (solver_maxiter == 0) solver_maxiter = h->maxiter;
    if (maxiter == 0) maxiter = solver_maxiter;
    RC(ms_reserve(h, nrhs, solver == ELPH_SOLVER_GMRES ? restart : 0));
    RC(elph_stage_in(h, h->work.b, B, nrhs));
    RC(elph_stage_in(h, h->work.x, X, nrhs));
    const MsVecs U = {h->work.x, h->work.b, false};                // (the caller's guess is taken as given)
    RC(ms_solve(h, U, solver, transposed ? 1 : 0, nrhs, use_precond ? 1 : 0, tol, maxiter, solver_maxiter, restart, iters));
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_mldiv(elph_handle h, int solver, int transposed, int nrhs, double *X, const double *B, int use_precond, int64_t maxiter,
                          int restart, int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    if (!X || !B || !iters || !residual_error || !flag || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    restart = default_restart(h, restart);
    RC(need_ready(h, solver, transposed, nrhs, use_precond, restart));
    RC(ms_reserve(h, nrhs, solver == ELPH_SOLVER_GMRES ? restart : 0));
    RC(elph_stage_in(h, h->work.b, B, nrhs));
    RC(elph_stage_in(h, h->work.x, X, nrhs));
    const MsVecs U = {h->work.x, h->work.b, false};                // (the caller's guess is taken as given)
    RC(ms_ldiv(h, U, solver, transposed ? 1 : 0, nrhs, use_precond ? 1 : 0, maxiter, restart, iters, residual_error, flag));
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}
