// meas_dev.h — the device code the measurement units share (measure.hip: Holstein, ssh_measure.hip and ssh_bondcorr.hip: bond phonons):
// the workgroup sum in its one fixed order, the modulated hopping of a bond phonon, and the folds of the estimator's four real tables into Greens, DenDen, SpinSpin and PairGreens
// (Measurements.jl:1469-1596), which do not depend on the model.  Layouts: header of measure.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "elph_internal.h"

constexpr int MEAS_TPB = 256;
constexpr int MEAS_NWAVE = MEAS_TPB / ELPH_WAVE;
enum { MEAS_GREENS = 0, MEAS_DENDEN = 1, MEAS_SPINSPIN = 2, MEAS_PAIRGREENS = 3 };

// Sum over the workgroup in a fixed order; the result is valid on thread 0.  red: MEAS_NWAVE doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int off = ELPH_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, ELPH_WAVE);
    __syncthreads();                                   // the previous call's readers are done with red
    if ((threadIdx.x & (ELPH_WAVE - 1)) == 0) red[threadIdx.x / ELPH_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < MEAS_NWAVE; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ int sign_of(double v) { return (v > 0.0) - (v < 0.0); }          // Julia's sign: sign(0) = 0

// the modulated hopping t' = t - (alpha x + sign(x) alpha2 x^2) of a bond phonon (SSHModels.jl:531-533)
__device__ __forceinline__ double t_modulated(double t, double alpha, double alpha2, double x) {
    return t - (alpha * x + sign_of(x) * alpha2 * (x * x));
}

// measure_<which>(l = cell, o1, o2, tau) of one pair of vectors (o1, o2 0-based, tau <= L).  C: the estimator's four real tables
// C[c][tau < L][s2 + n_s (s1 + n_s cell)] of this pair.  tstride: doubles between two of the four tables, nchains L n_s N in the
// pipeline's [table][chain][L][n_s N] (measure.hip, ssh_measure.hip).
__device__ __forceinline__ double meas_fold(int which, const double *__restrict__ C, int N, int L, int ns, int L1, int L2, int L3, int tau,
                                            int cell, int o1, int o2, size_t tstride) {
    const size_t ncol = (size_t)ns * N, tab = tstride;
    const bool beta = (tau == L);
    double v;
    if (which == MEAS_SPINSPIN) {
        if (beta) {                                    // <s(i+r, beta) s(i, 0)> = <s(i-r, 0) s(i, 0)>, orbitals swapped
            tau = 0;
            const int l1 = cell % L1, l2 = (cell / L1) % L2, l3 = cell / (L1 * L2);
            cell = ((L1 - l1) % L1) + L1 * (((L2 - l2) % L2) + L2 * ((L3 - l3) % L3));
            const int s = o1; o1 = o2; o2 = s;
        }
        const size_t e = (size_t)tau * ncol + o2 + ns * (o1 + ns * cell);
        v = -2 * C[3 * tab + e];
        if (cell == 0 && o1 == o2 && tau == 0) v += 2 * C[e];
    } else {
        const int tm = beta ? 0 : tau;                 // tau % L
        const size_t e = (size_t)tm * ncol + o2 + ns * (o1 + ns * cell);
        const bool diag = (cell == 0 && o1 == o2);
        if (which == MEAS_GREENS) {
            v = C[e];
            if (beta) v = (diag ? 1.0 : 0.0) - v;      // G_r(beta) = delta_r - G_r(0)
        } else if (which == MEAS_DENDEN) {
            const double G00 = C[o1 + ns * o1], Grr = C[o2 + ns * o2];      // tau = 0, r = 0 diagonal entries
            double h = -C[3 * tab + e];
            if (diag && tm == 0) h += C[e];
            v = 4.0 * (1.0 - Grr - G00 + C[2 * tab + e] + 0.5 * h);
        } else {                                       // MEAS_PAIRGREENS
            v = C[tab + e];
            if (beta && diag) v = v + 1.0 - 2 * C[o1 + ns * o1];            // P_r(beta) = P_r(0) + delta_r (1 - 2 G_0(0))
        }
    }
    return v;
}
