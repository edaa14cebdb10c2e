// meas_ssh_dev.h — what one workgroup does in each kernel of the bond-phonon (SSH) measurements (ssh_measure.hip: the chain is a grid
// axis, and a kernel there only says where a workgroup finds its chain's block).  Every function takes ONE configuration's pointers.
// Layouts and the rule of the reductions: header of ssh_measure.hip.
#pragma once

#include "cell_dft_dev.h"
#include "corr_req.h"
#include "meas_dev.h"

constexpr int SM_NCORR = 5;
constexpr int SM_PHONONGREENS = 4;    // 0..3: the folds of meas_dev.h
constexpr int SM_NONSITE = 3;         // density, double_occ, mu
constexpr int SM_NINTER = 8;          // x, x2, x4, phonon_pe, phonon_ke, elph_energy, el_ke, sign_switch
constexpr int SM_NXONLY = 6;          // x, x2, x4, phonon_pe, phonon_ke, sign_switch: functions of the field alone
constexpr int SM_NBPAR = 4;           // per bond: t, omega, alpha, alpha2 (zeros on a bare bond)
static_assert(MEAS_TPB == CELL_DFT_TPB, "dft_cells walks the workgroup of sm_ph");

// LDS of sm_ph: 4 buffers of nc complex
inline size_t sm_ph_lds_bytes(int nc) { return 4 * (size_t)nc * sizeof(double2); }

// The field-only terms (Measurements.jl:1127-1147) of time slice t: part[t][d * SM_NXONLY + k].  red: MEAS_NWAVE doubles of LDS.
__device__ __forceinline__ void sm_x_slice(double *__restrict__ part, const double *__restrict__ x, const double *__restrict__ bpar,
                                           const int *__restrict__ bph, const int *__restrict__ doff, const int *__restrict__ dlist, int Nph,
                                           int L, int ndef, long long nbonds, double dtau, int t, double *red) {
    const int tn = (t + 1 == L) ? 0 : t + 1;
    const double *xt = x + (size_t)t * Nph, *xn = x + (size_t)tn * Nph;
    const double *bt = bpar, *om = bpar + nbonds, *al = bpar + 2 * nbonds, *al2 = bpar + 3 * nbonds;
    for (int d = 0; d < ndef; ++d) {
        double a[SM_NXONLY] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = doff[d] + threadIdx.x; j < doff[d + 1]; j += MEAS_TPB) {
            const int b = dlist[j], ph = bph[b];
            if (ph < 0) continue;
            const double xi = xt[ph], dx = xn[ph] - xi, x2 = xi * xi;
            a[0] += xi;
            a[1] += x2;
            a[2] += x2 * x2;
            a[3] += om[b] * om[b] * x2 / 2;
            a[4] += 0.5 / dtau - dx * dx / (dtau * dtau) / 2;
            a[5] += (sign_of(bt[b]) != sign_of(t_modulated(bt[b], al[b], al2[b], xi))) ? 1.0 : 0.0;
        }
        for (int k = 0; k < SM_NXONLY; ++k) {
            const double s = block_sum(a[k], red);
            if (threadIdx.x == 0) part[(size_t)t * SM_NXONLY * ndef + d * SM_NXONLY + k] = s;
        }
    }
}

// xs[k][d] = (sum of the slices' partials in slice order) / V
__device__ __forceinline__ void sm_x_finish(double *__restrict__ xs, const double *__restrict__ part, int L, int ndef, double V) {
    const int nq = SM_NXONLY * ndef;
    for (int q = threadIdx.x; q < nq; q += MEAS_TPB) {
        double s = 0.0;
        for (int t = 0; t < L; ++t) s += part[(size_t)t * nq + q];
        const int d = q / SM_NXONLY, k = q % SM_NXONLY;
        xs[k * ndef + d] = s / V;
    }
}

// The terms of one pair of vectors that need the estimate (:1011-1016, :1121-1150, :1287-1288), time slice t.
// part[t][q]: q = 2 o + {density, double_occ}; 2 n_s + {dot(M^-1 r1, r1), dot(M^-1 r2, r2)}; 2 n_s + 2 + 2 d + {el_ke, elph_energy}.
__device__ __forceinline__ void sm_pair_slice(double *__restrict__ part, const double *__restrict__ X1, const double *__restrict__ X2,
                                              const double *__restrict__ R1, const double *__restrict__ R2, const double *__restrict__ x,
                                              const int *__restrict__ bs, const double *__restrict__ bpar, const int *__restrict__ bph,
                                              const int *__restrict__ doff, const int *__restrict__ dlist, int N, int Nph, int ns, int nc,
                                              int ndef, long long nbonds, int t, double *red) {
    const int nq = 2 * ns + 2 + 2 * ndef;
    const size_t o0 = (size_t)t * N;
    const double *a1 = X1 + o0, *a2 = X2 + o0, *b1 = R1 + o0, *b2 = R2 + o0, *xt = x + (size_t)t * Nph;
    const double *bt = bpar, *al = bpar + 2 * nbonds, *al2 = bpar + 3 * nbonds;
    double *out = part + (size_t)t * nq;
    double d1 = 0.0, d2 = 0.0;
    for (int o = 0; o < ns; ++o) {
        double den = 0.0, docc = 0.0, g1s = 0.0, g2s = 0.0;
        for (int c = threadIdx.x; c < nc; c += MEAS_TPB) {
            const int i = c * ns + o;
            const double G1 = a1[i] * b1[i], G2 = a2[i] * b2[i];
            den += (1.0 - G1) + (1.0 - G2);
            docc += (1.0 - G1) * (1.0 - G2);
            g1s += G1;
            g2s += G2;
        }
        double s = block_sum(den, red);
        if (threadIdx.x == 0) out[2 * o] = s;
        s = block_sum(docc, red);
        if (threadIdx.x == 0) out[2 * o + 1] = s;
        d1 += block_sum(g1s, red);                     // thread 0: orbitals in index order
        d2 += block_sum(g2s, red);
    }
    if (threadIdx.x == 0) { out[2 * ns] = d1; out[2 * ns + 1] = d2; }
    for (int d = 0; d < ndef; ++d) {
        double ke = 0.0, eph = 0.0;
        for (int j = doff[d] + threadIdx.x; j < doff[d + 1]; j += MEAS_TPB) {
            const int b = dlist[j], ph = bph[b];
            const int s1 = bs[b], s2 = bs[nbonds + b];
            // h = -(G1 + G2 + G3 + G4)
            const double mh = a1[s1] * b1[s2] + a1[s2] * b1[s1] + a2[s1] * b2[s2] + a2[s2] * b2[s1];
            double tp = bt[b];
            if (ph >= 0) {
                const double xi = xt[ph];
                tp = t_modulated(tp, al[b], al2[b], xi);
                eph -= al[b] * mh * xi;                // alpha h x
            }
            ke += tp * mh;                             // -t' h
        }
        double s = block_sum(ke, red);
        if (threadIdx.x == 0) out[2 * ns + 2 + 2 * d] = s;
        s = block_sum(eph, red);
        if (threadIdx.x == 0) out[2 * ns + 2 + 2 * d + 1] = s;
    }
}

// One workgroup: the slices' partials in slice order, the tau = 0 slice of G[D,0] G[0,D] (C3) for Nsqr, then every scalar accumulator of
// this pair.  acc: [density, Nsqr, mu | SM_NONSITE x n_s | SM_NINTER x ndef].  tot: [nq] + MEAS_NWAVE doubles of LDS.
__device__ __forceinline__ void sm_finish(double *__restrict__ acc, const double *__restrict__ part, const double *__restrict__ xs,
                                          const double *__restrict__ muo, const double *__restrict__ C3, int N, int L, int ns, int nc, int ndef,
                                          double mu_mean, double V, double *tot) {
    const int nq = 2 * ns + 2 + 2 * ndef, ncol = ns * N;
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
        const double Tr1 = tot[2 * ns] / L, Tr2 = tot[2 * ns + 1] / L;
        const double N1 = 2 * (Nd - Tr1), N2 = 2 * (Nd - Tr2);
        acc[0] += (N1 + N2) / (2 * Nd);
        acc[1] += N1 * N2 + Tr1 + Tr2 - 2 * (Nd / ns) * sumG;
        acc[2] += mu_mean;
    }
    double *on = acc + 3;
    for (int o = threadIdx.x; o < ns; o += MEAS_TPB) {
        on[0 * ns + o] += tot[2 * o] / norm;
        on[1 * ns + o] += tot[2 * o + 1] / norm;
        on[2 * ns + o] += muo[o];
    }
    double *in = acc + 3 + SM_NONSITE * ns;
    for (int d = threadIdx.x; d < ndef; d += MEAS_TPB) {
        for (int k = 0; k < 5; ++k) in[k * ndef + d] += xs[k * ndef + d];
        in[5 * ndef + d] += tot[2 * ns + 2 + 2 * d + 1] / V;
        in[6 * ndef + d] += tot[2 * ns + 2 + 2 * d] / V;
        in[7 * ndef + d] += xs[5 * ndef + d];
    }
}

// One workgroup, one frequency and one listed pair (t1, t2) of phonon types: the cell-axis DFTs of the two types' spectra, their product
// with fft(g)[-w,-k] = conj fft(g)[w,k], the inverse cell-axis DFT.  nuk: this frequency's row of the field's half spectra, [Nph];
// y: [nc] of the pair at this frequency; lds: 4 buffers of nc complex.
__device__ __forceinline__ void sm_ph(double2 *__restrict__ y, const double2 *__restrict__ nuk, int t1, int t2, int L1, int L2, int L3,
                                      const double2 *__restrict__ tw, double norm, double2 *lds) {
    const int nc = L1 * L2 * L3;
    const double2 *f = nuk + (size_t)t2 * nc, *g = nuk + (size_t)t1 * nc;
    double2 *A = lds, *TA = lds + nc, *B = lds + 2 * nc, *TB = lds + 3 * nc;
    for (int q = threadIdx.x; q < nc; q += MEAS_TPB) { A[q] = f[q]; B[q] = g[q]; }
    __syncthreads();
    const double2 *Af = dft_cells<false>(A, TA, 1, L1, L2, L3, tw);
    const double2 *Bf = dft_cells<false>(B, TB, 1, L1, L2, L3, tw);
    double2 *P = (Af == A) ? TA : A, *Q = (Bf == B) ? TB : B;
    for (int q = threadIdx.x; q < nc; q += MEAS_TPB) {
        const double2 a = Af[q], b = Bf[q];            // a·conj(b)
        P[q] = make_double2((a.x * b.x + a.y * b.y) * norm, (a.y * b.x - a.x * b.y) * norm);
    }
    __syncthreads();
    const double2 *Pf = dft_cells<true>(P, Q, 1, L1, L2, L3, tw);
    for (int q = threadIdx.x; q < nc; q += MEAS_TPB) y[q] = Pf[q];
}

// Element idx = (tau, cell, listed pair) of correlation `which`.  C: the estimator's four real tables of this pair of vectors, tstride
// apart; B: this configuration's translation averages of the listed phonon-type pairs, [nP][L][nc] (only indexed when
// PhononGreens is measured); slice L is slice 0; acc_off: where this configuration's accumulators start.
__device__ __forceinline__ void sm_fold(const CorrReq<SM_NCORR> &rq, int which, long long idx, const double *__restrict__ C,
                                        const double *__restrict__ B, int N, int L, int ns, int L1, int L2, int L3, size_t tstride,
                                        size_t acc_off) {
    const int np = rq.np[which], L0 = rq.L0[which], nc = L1 * L2 * L3;
    if (idx >= (long long)L0 * nc * np) return;
    const int tau = (int)(idx % L0), cell = (int)((idx / L0) % nc);
    const int p = (int)(idx / ((long long)L0 * nc));
    double v;
    if (which == SM_PHONONGREENS)
        v = B[((size_t)p * L + (tau == L ? 0 : tau)) * nc + cell];
    else
        v = meas_fold(which, C, N, L, ns, L1, L2, L3, tau, cell, rq.pairs[which][2 * p], rq.pairs[which][2 * p + 1], tstride);
    rq.acc[which][acc_off + idx] += v;
}

// acc += cur, one thread per element
__device__ __forceinline__ void sm_add(double *__restrict__ acc, const double *__restrict__ cur, long long n) {
    const long long i = (long long)blockIdx.x * MEAS_TPB + threadIdx.x;
    if (i < n) acc[i] += cur[i];
}
