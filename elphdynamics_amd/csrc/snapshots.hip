// snapshots.hip — the density and double-occupancy snapshots of every chain resident in the handle from the estimator's vectors alone:
// the per-site profiles make_snapshot_measurements! writes after every measurement (take_density_snapshot! and
// take_double_occupancy_snapshot!, Measurements.jl:1351-1435).
//
// With R and M⁻¹R viewed as (L, N, n_v) and d_n(τ, i) = 1 − M⁻¹R[τ, i, n] · R[τ, i, n] the reference sums
//   density[i]          = Σ_τ Σ_{n = 1..n_v} 2 d_n                         / (n_v L)
//   double_occupancy[i] = Σ_τ Σ_{n = 1..n_v − 1} Σ_{m = 2..n_v} d_n d_m    / (binomial(n_v, 2) L)
// The ranges of the second are the reference's (:1416-1417): beyond n_v = 2 they hold n = m terms and both orders of some pairs.  Per
// (τ, i) the double sum is a product, (S − d_{n_v}) · (S − d_1) with S = Σ_n d_n, so one stream over n that keeps S, d_1 and d_{n_v}
// serves both profiles: registers depend on neither n_v nor N, no LDS, and nothing of the model, the lattice family or the field enters.
//
// Two kernels, stream-ordered.  k_snap_part, one thread per site, grid (site blocks, τ segments, chain): a thread walks the SEG slices
// of its segment side by side and, inside, the chain's n_v rows, and adds S and (S − d_last)(S − d_first) of the slices in slice order
// into part[chain][segment][2][N].  Adjacent lanes read adjacent doubles of a slice: coalesced.  The τ axis is cut because one chain at
// 16 x 16 is 256 threads, which alone cannot hide the latency of their loads.  SEG is a constant: the cut of the τ axis depends on L
// alone, never on nchains or n_v, so a chain's bits do not depend on its neighbours and equal a single configuration's.  k_snap_finish,
// one thread per (chain, site): the segments' partials added in segment order, then divided by the reference's V, n_v L and binomial(n_v, 2) L.  The rule
// of the measurement units' reductions holds: one fixed order, no atomics, the same inputs give the same bits; a thread reads one
// chain's rows only.
//
// Layout: vector v (0-based) of chain c is row v nchains + c of R and M⁻¹R (greens.hip), each row [τ][site] (layout S).

#include "elph_internal.h"

namespace {

constexpr int SEG = 4;              // slices of one τ segment, walked side by side by a thread: 2 SEG independent loads per vector

struct SnapshotsState {
    double *buf = nullptr;          // [nchains][nseg][2][N] the segments' partials, then [2][nchains][N] the two profiles
    size_t cap = 0;                 // doubles of buf
};

SnapshotsState *snap_of(elph_handle_s *h) { return (SnapshotsState *)h->snapshots; }

// part[chain][seg][0][site] = Σ_{τ in seg} S(τ, site),  part[chain][seg][1][site] = Σ_{τ in seg} (S − d_last)(S − d_first)
__global__ void __launch_bounds__(ELPH_WAVE) k_snap_part(double *__restrict__ part, const double *__restrict__ X, const double *__restrict__ R, int N,
                                                         int L, int nch, int nv) {
    const int site = blockIdx.x * ELPH_WAVE + threadIdx.x, seg = blockIdx.y, ch = blockIdx.z, tau0 = seg * SEG;
    if (site >= N) return;
    const size_t nd = (size_t)L * N, vstride = (size_t)nch * nd, base = (size_t)ch * nd + (size_t)tau0 * N + site;
    double S[SEG], dfirst[SEG], dlast[SEG];
#pragma unroll
    for (int t = 0; t < SEG; ++t) S[t] = dfirst[t] = dlast[t] = 0.0;
    for (int n = 0; n < nv; ++n) {
        const size_t row = base + (size_t)n * vstride;
        double x[SEG], r[SEG];
#pragma unroll
        for (int t = 0; t < SEG; ++t) {                             // tau0 + t < L is the same in every lane of the grid's row
            const bool in = tau0 + t < L;
            x[t] = in ? X[row + (size_t)t * N] : 0.0;
            r[t] = in ? R[row + (size_t)t * N] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < SEG; ++t) {
            const double d = 1.0 - x[t] * r[t];
            if (n == 0) dfirst[t] = d;
            dlast[t] = d;
            S[t] += d;
        }
    }
    double dens = 0.0, docc = 0.0;
#pragma unroll
    for (int t = 0; t < SEG; ++t)                                   // slice order
        if (tau0 + t < L) {
            dens += S[t];
            docc += (S[t] - dlast[t]) * (S[t] - dfirst[t]);
        }
    double *out = part + ((size_t)ch * gridDim.y + seg) * 2 * N;
    out[site] = dens;
    out[(size_t)N + site] = docc;
}

// out[0][chain][site] the density profile, out[1][chain][site] the double occupancy, normalised
__global__ void __launch_bounds__(ELPH_WAVE) k_snap_finish(double *__restrict__ out, const double *__restrict__ part, int N, int nseg, int nch,
                                                           double V1, double V2) {
    const int site = blockIdx.x * ELPH_WAVE + threadIdx.x, ch = blockIdx.y;
    if (site >= N) return;
    const double *p = part + (size_t)ch * nseg * 2 * N + site;
    double dens = 0.0, docc = 0.0;
    for (int s = 0; s < nseg; ++s) {                                // segment order
        dens += p[(size_t)s * 2 * N];
        docc += p[((size_t)s * 2 + 1) * N];
    }
    out[(size_t)ch * N + site] = 2.0 * dens / V1;                 // Σ 2 d_n, then the reference's val / V
    out[((size_t)nch + ch) * N + site] = docc / V2;
}

}  // namespace

void elph_snapshots_free(elph_handle_s *h) {
    SnapshotsState *d = snap_of(h);
    if (!d) return;
    if (d->buf) (void)hipFree(d->buf);
    delete d;
    h->snapshots = nullptr;
}

extern "C" int elph_snapshots(elph_handle h, int nchains, double *density, double *double_occ) {
    CHECK_H(h);
    if (h->shard || h->is_slab) { elph_set_error("snapshots: sharded and slab handles are not supported"); return ELPH_E_UNSUPPORTED; }
    ElphGreensView g;
    RC(elph_i_greens_view(h, &g));
    if (nchains < 1 || nchains != h->nchains) {
        elph_set_error("snapshots: asked for %d chains, %d are resident in this handle", nchains, h->nchains);
        return ELPH_E_ARG;
    }
    if (!density && !double_occ) { elph_set_error("snapshots: both output arrays are null, one of the 2 is needed"); return ELPH_E_ARG; }
    if (g.nv % nchains) {
        elph_set_error("snapshots: the estimator's %d vectors are not a multiple of the %d resident chains", g.nv, nchains);
        return ELPH_E_STATE;
    }
    const int nv = g.nv / nchains;
    if (nv < 2) { elph_set_error("snapshots: %d vector per chain, binomial(n_v, 2) needs two", nv); return ELPH_E_STATE; }
    if (!g.have_vectors) {
        elph_set_error("snapshots: the estimator's %d vectors hold no vectors yet: call elph_greens_update or elph_greens_set_vectors", g.nv);
        return ELPH_E_STATE;
    }
    const size_t nch = (size_t)nchains, N = (size_t)h->N, L = (size_t)h->L, nseg = (L + SEG - 1) / SEG;
    const size_t npart = nch * nseg * 2 * N, nout = 2 * nch * N, need = npart + nout;
    SnapshotsState *d = snap_of(h);
    if (!d) h->snapshots = d = new SnapshotsState;
    if (need > d->cap) {                                            // first use, or the shape grew
        HIPCHK(hipStreamSynchronize(h->stream));
        if (d->buf) { HIPCHK(hipFree(d->buf)); d->buf = nullptr; d->cap = 0; }
        HIPCHK(hipMalloc((void **)&d->buf, need * sizeof(double)));
        d->cap = need;
    }
    double *part = d->buf, *out = part + npart;
    const unsigned nblk = (unsigned)((N + ELPH_WAVE - 1) / ELPH_WAVE);
    hipLaunchKernelGGL(k_snap_part, dim3(nblk, (unsigned)nseg, (unsigned)nch), dim3(ELPH_WAVE), 0, h->stream, part, g.X, g.R, (int)N, (int)L,
                       nchains, nv);
    RC(elph_launch_check("k_snap_part"));
    const double V1 = (double)nv * (double)L, V2 = 0.5 * (double)nv * (double)(nv - 1) * (double)L;
    hipLaunchKernelGGL(k_snap_finish, dim3(nblk, (unsigned)nch), dim3(ELPH_WAVE), 0, h->stream, out, part, (int)N, (int)nseg, nchains, V1, V2);
    RC(elph_launch_check("k_snap_finish"));
    if (density) HIPCHK(hipMemcpyAsync(density, out, nch * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (double_occ) HIPCHK(hipMemcpyAsync(double_occ, out + nch * N, nch * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}
