// meas_holstein_dev.h — what one workgroup does in each kernel of the Holstein measurements (measure.hip: the chain is a grid axis, and a
// kernel there only says where a workgroup finds its chain's block).  Every function takes ONE configuration's pointers.  Layouts and the
// rule of the reductions: header of measure.hip.
#pragma once

#include "corr_req.h"
#include "meas_dev.h"

constexpr int MS_NCORR = 5;
constexpr int MS_PHONONGREENS = 4;    // 0..3: the folds of meas_dev.h
constexpr int MS_NONSITE = 9;         // density, double_occ, x, x2, x4, phonon_pe, phonon_ke, elph_energy, mu
constexpr int MS_NXONLY = 6;          // x, x2, x4, phonon_pe, phonon_ke, mu: functions of the field alone

// The field-only on-site terms (Measurements.jl:955-970) of time slice t: part[t][o * MS_NXONLY + k].  red: MEAS_NWAVE doubles of LDS.
__device__ __forceinline__ void ms_x_slice(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ om,
                                           const double *__restrict__ om4, const double *__restrict__ mu, int N, int L, int ns, int nc, double dtau,
                                           int t, double *red) {
    const int tn = (t + 1 == L) ? 0 : t + 1;
    const double *xt = x + (size_t)t * N, *xn = x + (size_t)tn * N;
    for (int o = 0; o < ns; ++o) {
        double a[MS_NXONLY] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int c = threadIdx.x; c < nc; c += MEAS_TPB) {
            const int i = c * ns + o;
            const double xi = xt[i], dx = xn[i] - xi, x2 = xi * xi, x4 = x2 * x2;
            a[0] += xi;
            a[1] += x2;
            a[2] += x4;
            a[3] += om[i] * om[i] * x2 / 2 + om4[i] * x4;
            a[4] += 0.5 / dtau - dx * dx / (dtau * dtau) / 2;
            a[5] += mu[i];
        }
        for (int k = 0; k < MS_NXONLY; ++k) {
            const double s = block_sum(a[k], red);
            if (threadIdx.x == 0) part[(size_t)t * MS_NXONLY * ns + o * MS_NXONLY + k] = s;
        }
    }
}

// xs[k][o] = (sum of the slices' partials in slice order) / (Nc L)
__device__ __forceinline__ void ms_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ns, double norm) {
    const int nq = MS_NXONLY * ns;
    for (int q = threadIdx.x; q < nq; q += MEAS_TPB) {
        double s = 0.0;
        for (int t = 0; t < L; ++t) s += part[(size_t)t * nq + q];
        const int o = q / MS_NXONLY, k = q % MS_NXONLY;
        xs[k * ns + o] = s / norm;
    }
}

// The terms of one pair of vectors that need the estimate (Measurements.jl:949-962, :1056-1064, :1287-1288), time slice t.
// part[t][q]: q = 3 o + {density, double_occ, elph_energy}; 3 n_s + {dot(M^-1 r1, r1), dot(M^-1 r2, r2)}; 3 n_s + 2 + bond definition.
__device__ __forceinline__ void ms_pair_slice(double *__restrict__ part, const double *__restrict__ X1, const double *__restrict__ X2,
                                              const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ x,
                                              const double *__restrict__ lam, const int *__restrict__ bs, const double *__restrict__ bt, int N,
                                              int ns, int nc, int ndef, long long nbonds, int t, double *red) {
    const int nq = 3 * ns + 2 + ndef;
    const size_t o0 = (size_t)t * N;
    const double *a1 = X1 + o0, *a2 = X2 + o0, *b1 = R1 + o0, *b2 = R2 + o0, *xt = x + o0;
    double *out = part + (size_t)t * nq;
    double d1 = 0.0, d2 = 0.0;
    for (int o = 0; o < ns; ++o) {
        double den = 0.0, docc = 0.0, eph = 0.0, g1s = 0.0, g2s = 0.0;
        for (int c = threadIdx.x; c < nc; c += MEAS_TPB) {
            const int i = c * ns + o;
            const double G1 = a1[i] * b1[i], G2 = a2[i] * b2[i];
            den += (1.0 - G1) + (1.0 - G2);
            docc += (1.0 - G1) * (1.0 - G2);
            eph += lam[i] * xt[i] * (2.0 - G1 - G2);
            g1s += G1;
            g2s += G2;
        }
        double s = block_sum(den, red);
        if (threadIdx.x == 0) out[3 * o] = s;
        s = block_sum(docc, red);
        if (threadIdx.x == 0) out[3 * o + 1] = s;
        s = block_sum(eph, red);
        if (threadIdx.x == 0) out[3 * o + 2] = s;
        d1 += block_sum(g1s, red);                     // thread 0: orbitals in index order
        d2 += block_sum(g2s, red);
    }
    if (threadIdx.x == 0) { out[3 * ns] = d1; out[3 * ns + 1] = d2; }
    for (int d = 0; d < ndef; ++d) {
        double ke = 0.0;
        for (int c = threadIdx.x; c < nc; c += MEAS_TPB) {
            const long long b = (long long)d * nc + c;
            const int s1 = bs[b], s2 = bs[nbonds + b];
            // -t h, h = -(G1 + G2 + G3 + G4)
            ke += bt[b] * (a1[s1] * b1[s2] + a1[s2] * b1[s1] + a2[s1] * b2[s2] + a2[s2] * b2[s1]);
        }
        const double s = block_sum(ke, red);
        if (threadIdx.x == 0) out[3 * ns + 2 + d] = s;
    }
}

// One workgroup: the slices' partials in slice order, the tau = 0 slice of G[D,0] G[0,D] (C3) for Nsqr, then every scalar accumulator of
// this pair.  acc: [density, Nsqr, mu | MS_NONSITE x n_s | ndef].  tot: [nq] + MEAS_NWAVE doubles of LDS.
__device__ __forceinline__ void ms_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                          const double *__restrict__ C3, int N, int L, int ns, int nc, int ndef, double mu_mean, double *tot) {
    const int nq = 3 * ns + 2 + ndef, ncol = ns * N;
    double *red = tot + nq;
    for (int q = threadIdx.x; q < nq; q += MEAS_TPB) {
        double s = 0.0;
        for (int t = 0; t < L; ++t) s += part[(size_t)t * nq + q];
        tot[q] = s;
    }
    double g = 0.0;
    for (int i = threadIdx.x; i < ncol; i += MEAS_TPB) g += C3[i];
    const double sumG = block_sum(g, red);             // (its barriers also publish tot)
    const double norm = (double)nc * (double)L;
    if (threadIdx.x == 0) {
        const double Nd = (double)N;
        const double Tr1 = tot[3 * ns] / L, Tr2 = tot[3 * ns + 1] / L;
        const double N1 = 2 * (Nd - Tr1), N2 = 2 * (Nd - Tr2);
        acc[0] += (N1 + N2) / (2 * Nd);
        acc[1] += N1 * N2 + Tr1 + Tr2 - 2 * (Nd / ns) * sumG;
        acc[2] += mu_mean;
    }
    double *on = acc + 3;
    for (int o = threadIdx.x; o < ns; o += MEAS_TPB) {
        on[0 * ns + o] += tot[3 * o] / norm;
        on[1 * ns + o] += tot[3 * o + 1] / norm;
        on[2 * ns + o] += xs[0 * ns + o];
        on[3 * ns + o] += xs[1 * ns + o];
        on[4 * ns + o] += xs[2 * ns + o];
        on[5 * ns + o] += xs[3 * ns + o];
        on[6 * ns + o] += xs[4 * ns + o];
        on[7 * ns + o] += tot[3 * o + 2] / norm;
        on[8 * ns + o] += xs[5 * ns + o];
    }
    for (int d = threadIdx.x; d < ndef; d += MEAS_TPB) acc[3 + MS_NONSITE * ns + d] += tot[3 * ns + 2 + d] / norm;
}

// Element idx = (tau, cell, listed pair) of correlation `which` (Measurements.jl:1469-1650).  C: the estimator's four real tables of this
// pair, tstride apart; ph: the field's translation average, this configuration's at ph_off (ph may be null when
// PhononGreens is not measured: it is only indexed then); acc_off: where this configuration's accumulators start.
__device__ __forceinline__ void ms_fold(const CorrReq<MS_NCORR> &rq, int which, long long idx, const double *__restrict__ C,
                                        const double *__restrict__ ph, int N, int L, int ns, int L1, int L2, int L3, size_t tstride,
                                        size_t acc_off, size_t ph_off) {
    const int np = rq.np[which], L0 = rq.L0[which], nc = L1 * L2 * L3;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc);
    const int p = (int)(idx / ((long long)L0 * nc));
    const int o1 = rq.pairs[which][2 * p], o2 = rq.pairs[which][2 * p + 1];
    double v;
    if (which == MS_PHONONGREENS)                      // x1x2[D] = 1/(L Nc) sum x_o1[. + D] x_o2[.]; slice L is slice 0
        v = ph[ph_off + (size_t)(tau == L ? 0 : tau) * ns * N + o1 + ns * (o2 + ns * cell)];
    else
        v = meas_fold(which, C, N, L, ns, L1, L2, L3, tau, cell, o1, o2, tstride);
    rq.acc[which][acc_off + idx] += v;
}
