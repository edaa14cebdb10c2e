// cell_dft_dev.h — direct DFTs over the (up to) three cell axes of an array held in LDS, shared by the Green's-function estimator
// (greens.hip) and the bond correlations (bondcorr_dev.h).  Spatial extents are the lattice's (8…32): host-built twiddles
// tw[L1 + L2 + L3] = exp(-2πi j/Lx), exact index reduction.  Workgroups of CELL_DFT_TPB threads.
#pragma once

#include <hip/hip_runtime.h>

constexpr int CELL_DFT_TPB = 256;

// dst[e] = Σ_j src[e with axis index j] · w^(a·j), a = axis index of e; w = tw (forward) or conj tw (inverse)
template <bool INV>
__device__ void dft_axis(double2 *dst, const double2 *src, int total, int stride, int len, const double2 *__restrict__ tw) {
    for (int e = threadIdx.x; e < total; e += CELL_DFT_TPB) {
        const int a = (e / stride) % len;
        const int base = e - a * stride;
        double2 acc = make_double2(0.0, 0.0);
        int m = 0;                                  // (a*j) mod len, exact
        for (int j = 0; j < len; ++j) {
            double2 w = tw[m];
            if (INV) w.y = -w.y;
            const double2 v = src[base + j * stride];
            acc.x += v.x * w.x - v.y * w.y;
            acc.y += v.x * w.y + v.y * w.x;
            m += a;
            if (m >= len) m -= len;
        }
        dst[e] = acc;
    }
    __syncthreads();
}

// DFT over the (up to) three cell axes of `total` = unit*L1*L2*L3 complex numbers held in LDS buffer a (scratch b);
// returns the buffer that holds the result.  unit = n_s when the orbital index is interleaved, 1 for cell arrays.
template <bool INV>
__device__ double2 *dft_cells(double2 *a, double2 *b, int unit, int L1, int L2, int L3, const double2 *__restrict__ tw) {
    const int total = unit * L1 * L2 * L3;
    if (L1 > 1) { dft_axis<INV>(b, a, total, unit, L1, tw); double2 *t = a; a = b; b = t; }
    if (L2 > 1) { dft_axis<INV>(b, a, total, unit * L1, L2, tw + L1); double2 *t = a; a = b; b = t; }
    if (L3 > 1) { dft_axis<INV>(b, a, total, unit * L1 * L2, L3, tw + L1 + L2); double2 *t = a; a = b; b = t; }
    return a;
}
