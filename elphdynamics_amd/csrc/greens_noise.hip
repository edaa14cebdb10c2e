// greens_noise.hip — the Green's-function estimator's noise vectors drawn on the device (elph_greens_update_rng, greens.hip):
//   randn!(R) of update!(estimator, model, P)      GreensFunctions.jl:212
// One batch of nvec * ndim standard normals of the build's generator (rng_dev.h), numbered in the layout the host array would have had
// ([vec][site][τ], τ fastest) and written straight into layout S ([vec][τ][site]): the batch equals
// synth.randn(batch seed, nvec * ndim).reshape(nvec, ndim) handed over through elph_greens_update.
//
// Box-Muller makes elements (2k, 2k+1) from one (r, θ).  Two mappings of pairs to threads:
//   * pair-indexed (k_gr_randn_pair): thread k owns pair k, as k_randn_S of hmc.hip does.  Any shape; neighbouring lanes store 2 N doubles
//     apart, one 8-byte store per cache line and instruction.
//   * site-fastest (k_gr_randn_site): for even L a pair is time slices (2j, 2j+1) of one site, so a thread that owns (vec, j, site) with the
//     site fastest across the lanes stores its cosine at [vec][2j][site] and its sine at [vec][2j+1][site]: both stores are contiguous over
//     the lanes.  Odd L makes pairs straddle sites and takes the pair-indexed kernel.
// The two write the same bits.  All element indices are 64-bit: nvec * ndim exceeds 2^31 well within device memory.

#include <climits>

#include "elph_internal.h"
#include "rng_dev.h"

namespace {

constexpr int TPB = 256;

// (r cos θ, r sin θ) of pair k of a batch of m pairs
__device__ __forceinline__ void box_muller(uint64_t seed, long long m, long long k, double *c, double *s) {
    const double r = sqrt(-2.0 * log(u01(seed, (uint64_t)k)));
    double sn, cs;
    sincos(6.283185307179586476925 * u01(seed, (uint64_t)(m + k)), &sn, &cs);
    *c = r * cs;
    *s = r * sn;
}

// n normals as vectors of N * L; thread k owns elements 2k and 2k + 1 of the reference numbering (the last pair of an odd n has no sine)
__global__ void __launch_bounds__(TPB) k_gr_randn_pair(double *__restrict__ dst, uint64_t seed, long long n, int N, int L) {
    const long long k = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long m = (n + 1) / 2;
    if (k >= m) return;
    double v[2];
    box_muller(seed, m, k, &v[0], &v[1]);
    const long long per = (long long)N * L;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long long i = 2 * k + e;
        if (i >= n) break;
        const long long vec = i / per, w = i - vec * per;
        const int site = (int)(w / L), t = (int)(w - (long long)site * L);
        dst[vec * per + (long long)t * N + site] = v[e];
    }
}

// even L: blockIdx.x walks q = j N + site of one vector (hq = N L / 2 pairs, below 2^31), blockIdx.y strides over the vectors
__global__ void __launch_bounds__(TPB) k_gr_randn_site(double *__restrict__ dst, uint64_t seed, long long nvec, int N, int L) {
    const unsigned hq = (unsigned)(((long long)N * L) / 2);
    const unsigned q = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (q >= hq) return;
    const unsigned j = q / (unsigned)N, site = q - j * (unsigned)N;
    const long long per = (long long)N * L, half = L / 2, m = nvec * (long long)hq;
    for (long long vec = blockIdx.y; vec < nvec; vec += gridDim.y) {
        const long long k = (vec * N + site) * half + j;
        double c, s;
        box_muller(seed, m, k, &c, &s);
        double *o = dst + vec * per + 2ll * j * N + site;
        o[0] = c;
        o[N] = s;
    }
}

bool site_mapping_applies(const elph_handle_s *h) { return h->L % 2 == 0 && (long long)h->N * h->L / 2 <= (long long)INT_MAX; }

}  // namespace

// nvec vectors of ndim normals of batch `seed` into dstS (layout S).  mapping: 0 pair-indexed, 1 site-fastest (ELPH_E_UNSUPPORTED where it does
// not apply), anything else = the one the estimator ships: site-fastest where it applies.  Stream-ordered, no synchronisation.
int elph_i_greens_randn(elph_handle_s *h, double *dstS, uint64_t seed, int64_t nvec, int mapping) {
    if (nvec < 1) return ELPH_OK;
    const bool site_ok = site_mapping_applies(h);
    if (mapping == 1 && !site_ok) { elph_set_error("the site-fastest mapping needs an even Ltau (it is %lld)", (long long)h->L); return ELPH_E_UNSUPPORTED; }
    const int N = (int)h->N, L = (int)h->L;
    if (mapping == 0 || !site_ok) {
        const long long n = (long long)nvec * h->ndim, m = (n + 1) / 2;
        hipLaunchKernelGGL(k_gr_randn_pair, dim3((unsigned)((m + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, dstS, seed, n, N, L);
        return elph_launch_check("k_gr_randn_pair");
    }
    const long long hq = (long long)h->ndim / 2;
    hipLaunchKernelGGL(k_gr_randn_site, dim3((unsigned)((hq + TPB - 1) / TPB), (unsigned)std::min<int64_t>(nvec, 65535)), dim3(TPB), 0, h->stream,
                       dstS, seed, (long long)nvec, N, L);
    return elph_launch_check("k_gr_randn_site");
}

extern "C" int elph_bench_greens_noise(elph_handle h, int mapping, int64_t nvec, uint64_t seed, int reps, double *ms_total, int64_t out_first,
                                       int64_t out_count, double *out) {
    CHECK_H(h);
    const int64_t n = nvec * h->ndim;
    if (nvec < 1 || reps < 1 || (out && (out_first < 0 || out_count < 0 || out_first > n - out_count))) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, (size_t)n * sizeof(double)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t er = hipEventCreate(&e0);
    if (er == hipSuccess) er = hipEventCreate(&e1);
    if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
    int rc = ELPH_OK;
    for (int r = 0; r < reps && er == hipSuccess && rc == ELPH_OK; ++r) rc = elph_i_greens_randn(h, buf, seed, nvec, mapping);
    if (er == hipSuccess && rc == ELPH_OK) er = hipEventRecord(e1, h->stream);
    if (er == hipSuccess && rc == ELPH_OK) er = hipEventSynchronize(e1);
    float ms = 0.f;
    if (er == hipSuccess && rc == ELPH_OK) er = hipEventElapsedTime(&ms, e0, e1);
    if (er == hipSuccess && rc == ELPH_OK && out && out_count > 0) er = hipMemcpy(out, buf + out_first, (size_t)out_count * sizeof(double), hipMemcpyDeviceToHost);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    if (rc) return rc;
    if (er != hipSuccess) { elph_set_error("elph_bench_greens_noise: %s", hipGetErrorString(er)); return ELPH_E_HIP; }
    if (ms_total) *ms_total = (double)ms;
    return ELPH_OK;
}
