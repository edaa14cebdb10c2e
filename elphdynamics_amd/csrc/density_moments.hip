// density_moments.hip — ⟨N⟩ and ⟨N²⟩ of every chain resident in the handle from the estimator's vectors alone: the two numbers the
// chemical-potential tuner takes after every update (update_μ!, MuFinder.jl:77-97; measure_density and measure_N², Measurements.jl:1283-1312).
//
// The reference reaches them through setup!(estimator, p, q) for every pair p < q of the n_v vectors, four 4-D convolutions per pair, of
// which measure_N² reads one table at Δτ = 0, summed over every displacement and both orbitals.  That sum factorises slice by slice:
//   C_pq(τ) = Σ_site (M⁻¹r_p)[site, τ] · r_q[site, τ]                            an n_v x n_v matrix per time slice
//   T_p = (1/L) Σ_τ C_pp(τ)        N_p = 2 (N − T_p)        S_pq = Σ_τ C_pq(τ) C_qp(τ)
//   N_pq = (N_p + N_q) / 2          N²_pq = N_p N_q + T_p + T_q − (2/L) S_pq      averaged over the binomial(n_v, 2) pairs
// so one pass over R and M⁻¹R serves: no convolution, and nothing of the model, the lattice family or the field enters.
//
// Two kernels, stream-ordered.  k_dm_slice, one wavefront per (τ, chain): C(τ) of the chain into part[chain][τ][p][q]; a lane walks the
// sites of the slice a wavefront apart (each row's slice is N contiguous doubles: coalesced) and holds a TILE x TILE block of C in
// registers, the rows tiled when n_v > TILE, so registers depend on neither N nor n_v and no LDS is used.  The cost of a slice is the
// cross-lane sums, six steps per entry of C whatever N is, not the n_v² products per site: one wavefront per slice sums each entry once
// (four wavefronts sharing a slice each summed all of them: 0.65 ms a call instead of 0.29 ms for 64 chains at 16 x 16, L = 160, n_v = 10,
// tools/time_mu_tuner.py).  k_dm_finish, one workgroup per chain: the slices' partials added in slice order, then the pairs in the reference's order by
// one thread.  The rule of the measurement units' reductions holds: one fixed order, no atomics, the same inputs give the same bits; a
// workgroup reads one chain's rows only.
//
// Layout: vector v (0-based) of chain c is row v nchains + c of R and M⁻¹R (greens.hip), each row [τ][site] (layout S).

#include <vector>

#include "elph_internal.h"
#include "meas_dev.h"

namespace {

constexpr int TPB = MEAS_TPB;
constexpr int TILE = 5;             // rows of M⁻¹R x rows of R a wavefront holds at once: the decks' n_v = 10 is two tiles a side

struct DensityMomentsState {
    double *buf = nullptr;          // [nchains][L][n_v²] the slices' partials, then [nchains][n_v² + n_v] S and the traces, then [nchains][2] (N, N²)
    size_t cap = 0;                 // doubles of buf
};

DensityMomentsState *dm_of(elph_handle_s *h) { return (DensityMomentsState *)h->density_moments; }

// part[chain][tau][p][q] = Σ_site X[p nch + chain][tau][site] · R[q nch + chain][tau][site]
__global__ void __launch_bounds__(ELPH_WAVE) k_dm_slice(double *__restrict__ part, const double *__restrict__ X, const double *__restrict__ R, int N,
                                                        int L, int nch, int nv) {
    const int tau = blockIdx.x, ch = blockIdx.y, lane = threadIdx.x;
    const size_t nd = (size_t)L * N, vstride = (size_t)nch * nd, base = (size_t)ch * nd + (size_t)tau * N;
    double *out = part + ((size_t)ch * L + tau) * nv * nv;
    for (int p0 = 0; p0 < nv; p0 += TILE)
        for (int q0 = 0; q0 < nv; q0 += TILE) {
            const int np = min(TILE, nv - p0), nq = min(TILE, nv - q0);
            double acc[TILE][TILE];
#pragma unroll
            for (int i = 0; i < TILE; ++i)
#pragma unroll
                for (int j = 0; j < TILE; ++j) acc[i][j] = 0.0;
            for (int s = lane; s < N; s += ELPH_WAVE) {            // the site axis in chunks of a wavefront
                double x[TILE], r[TILE];
#pragma unroll
                for (int i = 0; i < TILE; ++i) x[i] = (i < np) ? X[base + (size_t)(p0 + i) * vstride + s] : 0.0;
#pragma unroll
                for (int j = 0; j < TILE; ++j) r[j] = (j < nq) ? R[base + (size_t)(q0 + j) * vstride + s] : 0.0;
#pragma unroll
                for (int i = 0; i < TILE; ++i)
#pragma unroll
                    for (int j = 0; j < TILE; ++j) acc[i][j] += x[i] * r[j];
            }
            // the wavefront's tree of block_sum (meas_dev.h) for every entry of the tile
#pragma unroll
            for (int i = 0; i < TILE; ++i)
#pragma unroll
                for (int j = 0; j < TILE; ++j) {
                    if (i < np && j < nq) {                         // the same in every lane
                        double v = acc[i][j];
                        for (int off = ELPH_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, ELPH_WAVE);
                        if (lane == 0) out[(size_t)(p0 + i) * nv + (q0 + j)] = v;
                    }
                }
        }
}

// One workgroup per chain.  fin: [nchains][n_v² + n_v] (S, then the traces Σ_τ C_pp), out: [nchains][2] (N, N²)
__global__ void __launch_bounds__(TPB) k_dm_finish(double *__restrict__ out, double *__restrict__ fin, const double *__restrict__ part, int N, int L,
                                                   int nv) {
    const size_t ch = blockIdx.x, n2 = (size_t)nv * nv;
    const double *C = part + ch * L * n2;
    double *S = fin + ch * (n2 + nv), *Tr = S + n2;
    for (size_t e = threadIdx.x; e < n2; e += TPB) {
        const size_t p = e / nv, q = e % nv, et = q * nv + p;
        double s = 0.0, t = 0.0;
        for (int tau = 0; tau < L; ++tau) {                         // slice order
            const double c = C[(size_t)tau * n2 + e];
            s += c * C[(size_t)tau * n2 + et];
            t += c;
        }
        S[e] = s;
        if (p == q) Tr[p] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double Nd = (double)N, Ld = (double)L;
    double sumN = 0.0, sumN2 = 0.0;
    for (int p = 0; p < nv - 1; ++p)                                // the pairs in the reference's order (MuFinder.jl:81-93)
        for (int q = p + 1; q < nv; ++q) {
            const double Tp = Tr[p] / Ld, Tq = Tr[q] / Ld;
            const double Np = 2 * (Nd - Tp), Nq = 2 * (Nd - Tq);
            sumN += (Np + Nq) / 2;
            sumN2 += Np * Nq + Tp + Tq - (2.0 / Ld) * S[(size_t)p * nv + q];
        }
    const double npairs = 0.5 * (double)nv * (double)(nv - 1);
    out[2 * ch] = sumN / npairs;
    out[2 * ch + 1] = sumN2 / npairs;
}

}  // namespace

void elph_density_moments_free(elph_handle_s *h) {
    DensityMomentsState *d = dm_of(h);
    if (!d) return;
    if (d->buf) (void)hipFree(d->buf);
    delete d;
    h->density_moments = nullptr;
}

extern "C" int elph_density_moments(elph_handle h, int nchains, double *N, double *Nsqr) {
    CHECK_H(h);
    if (h->shard || h->is_slab) { elph_set_error("density moments: sharded and slab handles are not supported"); return ELPH_E_UNSUPPORTED; }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("density moments: asked for %d chains, %d are resident in this handle", nchains, h->nchains);
        return ELPH_E_ARG;
    }
    if (!N || !Nsqr) { elph_set_error("density moments: a null output array"); return ELPH_E_ARG; }
    if (g.nv % nchains) {
        elph_set_error("density moments: the estimator's %d vectors are not a multiple of the %d resident chains", g.nv, nchains);
        return ELPH_E_STATE;
    }
    const int nv = g.nv / nchains;
    if (nv < 2) { elph_set_error("density moments: %d vector per chain, a pair needs two", nv); return ELPH_E_STATE; }
    if (!g.have_vectors) { elph_set_error("no vectors yet: call elph_greens_update or elph_greens_set_vectors"); return ELPH_E_STATE; }
    const size_t nch = (size_t)nchains, L = (size_t)h->L, n2 = (size_t)nv * nv;
    const size_t npart = nch * L * n2, nfin = nch * (n2 + nv), need = npart + nfin + 2 * nch;
    DensityMomentsState *d = dm_of(h);
    if (!d) h->density_moments = d = new DensityMomentsState;
    if (need > d->cap) {                                            // first use, or the shape grew
        HIPCHK(hipStreamSynchronize(h->stream));
        if (d->buf) { HIPCHK(hipFree(d->buf)); d->buf = nullptr; d->cap = 0; }
        HIPCHK(hipMalloc((void **)&d->buf, need * sizeof(double)));
        d->cap = need;
    }
    double *part = d->buf, *fin = part + npart, *out = fin + nfin;
    hipLaunchKernelGGL(k_dm_slice, dim3((unsigned)L, (unsigned)nch), dim3(ELPH_WAVE), 0, h->stream, part, g.X, g.R, (int)h->N, (int)L, nchains, nv);
    RC(elph_launch_check("k_dm_slice"));
    hipLaunchKernelGGL(k_dm_finish, dim3((unsigned)nch), dim3(TPB), 0, h->stream, out, fin, part, (int)h->N, (int)L, nv);
    RC(elph_launch_check("k_dm_finish"));
    std::vector<double> host(2 * nch);
    HIPCHK(hipMemcpyAsync(host.data(), out, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t c = 0; c < nch; ++c) { N[c] = host[2 * c]; Nsqr[c] = host[2 * c + 1]; }
    return ELPH_OK;
}
