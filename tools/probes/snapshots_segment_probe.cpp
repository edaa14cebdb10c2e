// Probe: the partial-sum kernel of csrc/snapshots.hip alone, timed with device events, over the choices it fixes: slices per tau segment
// (SEG), threads per workgroup (TPB) and the unrolling of the loop over a chain's vectors (UNR).  Config C (16 x 16, L = 160), n_v = 10,
// 64 / 16 / 2 chains, zero-filled vectors (the arithmetic does not depend on the values); medians of 10 launches after 2.  The bytes are
// the 2 n_v nchains N L doubles every variant reads once (419 MB at 64 chains: beyond the Infinity Cache).  The body is k_snap_part's.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip tools/probes/snapshots_segment_probe.cpp -o /tmp/snapshots_segment_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); return 1; } } while (0)
template <int SEG, int TPB, int UNR>
__global__ void __launch_bounds__(TPB) k_part(double *__restrict__ part, const double *__restrict__ X, const double *__restrict__ R, int N, int L, int nch, int nv) {
    const int site = blockIdx.x * TPB + threadIdx.x, seg = blockIdx.y, ch = blockIdx.z, tau0 = seg * SEG;
    if (site >= N) return;
    const size_t nd = (size_t)L * N, vstride = (size_t)nch * nd, base = (size_t)ch * nd + (size_t)tau0 * N + site;
    double S[SEG], dfirst[SEG], dlast[SEG];
#pragma unroll
    for (int t = 0; t < SEG; ++t) S[t] = dfirst[t] = dlast[t] = 0.0;
#pragma unroll UNR
    for (int n = 0; n < nv; ++n) {
        const size_t row = base + (size_t)n * vstride;
        double x[SEG], r[SEG];
#pragma unroll
        for (int t = 0; t < SEG; ++t) {
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
    for (int t = 0; t < SEG; ++t)
        if (tau0 + t < L) { dens += S[t]; docc += (S[t] - dlast[t]) * (S[t] - dfirst[t]); }
    double *out = part + ((size_t)ch * gridDim.y + seg) * 2 * N;
    out[site] = dens;
    out[(size_t)N + site] = docc;
}
template <int SEG, int TPB, int UNR>
int run(const char *name, double *part, const double *X, const double *R, int N, int L, int nch, int nv, hipStream_t st) {
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> ms;
    const int nseg = (L + SEG - 1) / SEG;
    for (int rep = 0; rep < 12; ++rep) {
        CK(hipEventRecord(a, st));
        hipLaunchKernelGGL((k_part<SEG, TPB, UNR>), dim3((N + TPB - 1) / TPB, nseg, nch), dim3(TPB), 0, st, part, X, R, N, L, nch, nv);
        CK(hipGetLastError());
        CK(hipEventRecord(b, st));
        CK(hipEventSynchronize(b));
        float t; CK(hipEventElapsedTime(&t, a, b));
        if (rep >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double bytes = 2.0 * nv * nch * (double)N * L * 8;
    printf("%-22s nch %2d: median %.4f ms  min %.4f ms  %.2f TB/s at the median\n", name, nch, ms[ms.size() / 2], ms[0], bytes / (ms[ms.size() / 2] * 1e-3) / 1e12);
    return 0;
}
int main() {
    const int N = 256, L = 160, nv = 10, maxch = 64;
    const size_t nvec = (size_t)nv * maxch * N * L;
    double *X, *R, *part;
    CK(hipMalloc((void **)&X, nvec * 8)); CK(hipMalloc((void **)&R, nvec * 8));
    CK(hipMalloc((void **)&part, (size_t)maxch * L * 2 * N * 8));      // nseg <= L
    CK(hipMemset(X, 0, nvec * 8)); CK(hipMemset(R, 0, nvec * 8));
    hipStream_t st; CK(hipStreamCreate(&st));
    for (int nch : {64, 16, 2}) {
#define RUN(S, T, U) if (run<S, T, U>("SEG" #S " TPB" #T " UNR" #U, part, X, R, N, L, nch, nv, st)) return 1
        RUN(4, 64, 1); RUN(4, 64, 2); RUN(4, 256, 1); RUN(8, 64, 1); RUN(8, 64, 2); RUN(2, 64, 1); RUN(2, 64, 4); RUN(1, 64, 8); RUN(8, 256, 1); RUN(4, 128, 2);
    }
    CK(hipDeviceSynchronize());
    printf("done\n");
    return 0;
}
