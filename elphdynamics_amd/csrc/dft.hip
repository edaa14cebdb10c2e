// dft.hip — tau-axis transforms for the KPM preconditioner and Fourier acceleration.
//
// Reference: TimeFreqFFTs.jl:55-73 (tau_to_omega!: FFT of Theta.*v), :112-130 (omega_to_tau!),
// FourierAcceleration.jl:91-143 (fourier_accelerate!).  FFTW conventions: forward unnormalised
// exp(-2 pi i k t/L), inverse scaled 1/L.
//
// L_tau is 40..160 on every deck and all site columns are independent, so each transform is a direct
// real DFT over the half spectrum (real input => Hermitian symmetry; the twisted spectrum obeys
// nu[L-1-k] = conj nu[k], exactly the half the KPM loop visits, KPMPreconditioners.jl:449-467):
//   * lane = site: every global access is a coalesced 512-B (f64) / 1-KB (complex) row of layout S;
//   * twiddles come from host-built tables with the reduction index contiguous, Tk[k][t] / Tt[t][k],
//     so a wave reads them with wide *scalar* loads (the address depends only on block and loop index);
//     the inverse tables carry the Hermitian weight and the 1/L, so the inner loop is 2 FMA per term;
//   * the reduction axis is walked in register chunks with the next chunk's loads issued before the
//     current chunk's FMAs (two named buffers), so a wave pays ~L/TC memory round trips, not L.
// O(L^2) per column is deliberate at these lengths (13 MFLOP at config C); tables are O(L^2) bytes.

#include <cstdlib>

#include "elph_internal.h"

#define WAVE ELPH_WAVE

__device__ __forceinline__ double dft_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// `state` (optional) points at the CURRENT copy of the CG state (the host adds the launch parity)
__device__ __forceinline__ bool dft_done(const CgState *state, int rhs) {
    if (!state) return false;
    return __hip_atomic_load(&state[2 * rhs].done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// out[k][s] = f(k,s) * sum_t Tk[k][t] * v[t][s]      k in [0,K), real v
//   PLAIN: f = symmetrised diag^power (fourier_accelerate!), else f = 1
template <int KPT, int TC, bool PLAIN>
__global__ void __launch_bounds__(WAVE) k_dft_fwd_tab(double2 *__restrict__ out, const double *__restrict__ v,
                                                      const double2 *__restrict__ Tk, int N, int L, int K, int Lp,
                                                      const CgState *state, const double *__restrict__ diag, double power) {
    // Tk rows are zero-padded to Lp = roundup(L, 2*TC): the tail needs no predicate (clamped loads * 0)
    const int rhs = blockIdx.z;
    if (dft_done(state, rhs)) return;
    const int s = blockIdx.x * WAVE + threadIdx.x;
    const bool ok = s < N;
    const int sc = ok ? s : N - 1;
    const int k0 = blockIdx.y * KPT;
    const double *vv = v + (size_t)rhs * N * L;
    const double2 *tw[KPT];
    double2 acc[KPT];
#pragma unroll
    for (int kk = 0; kk < KPT; ++kk) {
        const int k = (k0 + kk < K) ? k0 + kk : K - 1;
        tw[kk] = Tk + (size_t)k * Lp;
        acc[kk] = make_double2(0.0, 0.0);
    }
    double xa[TC], xb[TC];
    auto load = [&](double (&x)[TC], int t0) {
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            const int t = (t0 + j < L) ? t0 + j : L - 1;
            x[j] = vv[(size_t)t * N + sc];
        }
    };
    auto comp = [&](const double (&x)[TC], int t0) {
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                const double2 w = tw[kk][t0 + j];
                acc[kk].x += x[j] * w.x;
                acc[kk].y += x[j] * w.y;
            }
        }
    };
    load(xa, 0);
    for (int t0 = 0; t0 < Lp; t0 += 2 * TC) {
        load(xb, t0 + TC);
        comp(xa, t0);
        load(xa, t0 + 2 * TC);
        comp(xb, t0 + TC);
    }
    if (ok) {
#pragma unroll
        for (int kk = 0; kk < KPT; ++kk) {
            const int k = k0 + kk;
            if (k < K) {
                double2 r = acc[kk];
                if (PLAIN && diag) {
                    // Re iFFT(D .* FFT(v)) of a real v only sees the symmetric part of D: (D[k] + D[L-k])/2
                    const int km = (k == 0) ? 0 : L - k;
                    const double f = 0.5 * (pow(diag[(size_t)k * N + s], power) + pow(diag[(size_t)km * N + s], power));
                    r.x *= f;
                    r.y *= f;
                }
                out[((size_t)rhs * K + k) * N + s] = r;
            }
        }
    }
}

// out[t][s] = sum_{k<K} Re( Tt[t][k] * nu[k][s] )   (weights and 1/L folded into Tt); optional fused partial r.out
template <int TPT, int KC>
__global__ void __launch_bounds__(WAVE) k_dft_inv_tab(double *__restrict__ out, const double2 *__restrict__ nu,
                                                      const double2 *__restrict__ Tt, int N, int L, int K, int Kp,
                                                      const CgState *state, const double *__restrict__ rvec,
                                                      double *__restrict__ rz_part, int nrz) {
    // Tt rows are zero-padded to Kp = roundup(K, 2*KC)
    const int rhs = blockIdx.z;
    if (dft_done(state, rhs)) return;
    const int s = blockIdx.x * WAVE + threadIdx.x;
    const bool ok = s < N;
    const int sc = ok ? s : N - 1;
    const int t0 = blockIdx.y * TPT;
    const double2 *nn = nu + (size_t)rhs * K * N;
    const double2 *tw[TPT];
    double acc[TPT];
#pragma unroll
    for (int tt = 0; tt < TPT; ++tt) {
        const int t = (t0 + tt < L) ? t0 + tt : L - 1;
        tw[tt] = Tt + (size_t)t * Kp;
        acc[tt] = 0.0;
    }
    double2 xa[KC], xb[KC];
    auto load = [&](double2 (&x)[KC], int kb) {
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int k = (kb + j < K) ? kb + j : K - 1;
            x[j] = nn[(size_t)k * N + sc];
        }
    };
    auto comp = [&](const double2 (&x)[KC], int kb) {
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const double2 w = tw[tt][kb + j];
                acc[tt] += w.x * x[j].x - w.y * x[j].y;
            }
        }
    };
    load(xa, 0);
    for (int kb = 0; kb < Kp; kb += 2 * KC) {
        load(xb, kb + KC);
        comp(xa, kb);
        load(xa, kb + 2 * KC);
        comp(xb, kb + KC);
    }
    double dot = 0.0;
#pragma unroll
    for (int tt = 0; tt < TPT; ++tt) {
        const int t = t0 + tt;
        if (ok && t < L) {
            const size_t i = (size_t)rhs * N * L + (size_t)t * N + s;
            out[i] = acc[tt];
            if (rz_part) dot += rvec[i] * acc[tt];
        }
    }
    if (rz_part) {
        dot = dft_wave_sum(dot);
        if (threadIdx.x == 0) {
            // own slot, plus this block's share of the slots no block of this grid owns (the reducers read all nrz)
            const int G = (int)(gridDim.x * gridDim.y), b = (int)(blockIdx.y * gridDim.x + blockIdx.x);
            double *slots = rz_part + (size_t)rhs * nrz;
            slots[b] = dot;
            for (int q = G + b; q < nrz; q += G) slots[q] = 0.0;
        }
    }
}

// u[rhs][k][s] *= (D[k][s]^p + D[L-k][s]^p)/2  — the symmetrised diagonal of fourier_accelerate! between the two GEMM-form
// transforms of a batch (the scalar forward kernel applies it in its epilogue)
__global__ void __launch_bounds__(256) k_dft_diag(double2 *__restrict__ u, const double *__restrict__ diag, double power, int N,
                                                  int L, int K, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int s = (int)(i % N), k = (int)((i / N) % K);
    const int km = (k == 0) ? 0 : L - k;
    const double f = 0.5 * (pow(diag[(size_t)k * N + s], power) + pow(diag[(size_t)km * N + s], power));
    double2 v = u[i];
    v.x *= f; v.y *= f;
    u[i] = v;
}

// Single-solve shapes (2 outputs per wave: many waves for the latency-bound case).  These kernels are bound by the
// scalar twiddle stream (106 SGPRs hold < 30 twiddles); a wider shape (8 outputs per wave) was measured ~15 % SLOWER in
// a batch, so batches go to the matrix-core GEMM form in dft_mfma.hip instead.
constexpr int DFT_KPT = 2, DFT_TC = 40, DFT_TPT = ELPH_DFT_TPT, DFT_KC = 20;
static int dft_pad(int n, int m) { return ((n + m - 1) / m) * m; }

static DftPlan plan(const elph_handle_s *h, int which, bool inverse, int N, int nvec, int nrz_slots) {
    return elph_plan_dft(h->dft.shape, dft_switches(), which, inverse, N, nvec, nrz_slots);
}
static int half(int which, int L) { return which == DFT_TWISTED ? (L + 1) / 2 : L / 2 + 1; }      // frequencies of the half spectrum

// nu[rhs][k][s] = FFT_t((twisted ? Theta : 1) .* v)[k], k < half; diag (plain, scalar form only): fourier_accelerate!'s diagonal in the epilogue
static int dft_fwd(elph_handle_s *h, const DftPlan &p, int which, double2 *nu, const double *vS, int N, int nrhs, const CgState *st,
                   const double *diag = nullptr, double power = 0.0) {
    const int L = (int)h->L, K = half(which, L);
    const dim3 grid((unsigned)((N + WAVE - 1) / WAVE), (unsigned)((K + DFT_KPT - 1) / DFT_KPT), (unsigned)nrhs);
    switch (p.form) {
    case DFT_SCALAR:
        if (which == DFT_TWISTED)
            hipLaunchKernelGGL((k_dft_fwd_tab<DFT_KPT, DFT_TC, false>), grid, dim3(WAVE), 0, h->stream, nu, vS, h->dft.Tk, N, L, K,
                               dft_pad(L, 2 * DFT_TC), st, (const double *)nullptr, 0.0);
        else
            hipLaunchKernelGGL((k_dft_fwd_tab<DFT_KPT, DFT_TC, true>), grid, dim3(WAVE), 0, h->stream, nu, vS, h->dft.Pk, N, L, K,
                               dft_pad(L, 2 * DFT_TC), st, diag, power);
        return elph_launch_check(which == DFT_TWISTED ? "k_dft_fwd_tab(twisted)" : "k_dft_fwd_tab(plain)");
    case DFT_BIG_ROW: case DFT_BIG_BLOCKED: case DFT_BIG_DIRECT:      // (finished right-hand sides are transformed too)
        return elph_dft_big_fwd(h, p.form, which == DFT_TWISTED, nu, vS, N, nrhs);
    default:
        return elph_dft_mfma_run(h, p, which, false, reinterpret_cast<double *>(nu), vS, N, nrhs, st, nullptr, nullptr, 0);
    }
}

// out = Re((twisted ? conj(Theta) : 1) .* iFFT(nu)) from the half spectrum (Hermitian weights and 1/L in the tables); rz_part (optional)
// receives partial r.out sums
static int dft_inv(elph_handle_s *h, const DftPlan &p, int which, double *outS, const double2 *nu, int N, int nrhs, const CgState *st,
                   const double *rvec, double *rz_part, int nrz) {
    const int L = (int)h->L, K = half(which, L);
    if (p.short_slots) {
        const bool big = p.form >= DFT_BIG_ROW, r2 = p.form == DFT_SPLIT_REG || p.form == DFT_SPLIT_LDS;
        elph_set_error("%s: %d partial slots needed, %d available", big ? "dft_big" : r2 ? "dft_mfma_r2" : "dft_mfma", p.slots, nrz);
        return ELPH_E_STATE;
    }
    switch (p.form) {
    case DFT_SCALAR:
        // r.z partial slots: (blockIdx.y * gridDim.x + blockIdx.x) < ceil(L/TPT)*nst <= L*npl = nrz; the kernel clears the rest
        hipLaunchKernelGGL((k_dft_inv_tab<DFT_TPT, DFT_KC>), dim3((unsigned)((N + WAVE - 1) / WAVE), (unsigned)((L + DFT_TPT - 1) / DFT_TPT), (unsigned)nrhs),
                           dim3(WAVE), 0, h->stream, outS, nu, which == DFT_TWISTED ? h->dft.Tt : h->dft.Pt, N, L, K, dft_pad(K, 2 * DFT_KC), st, rvec,
                           rz_part, nrz);
        return elph_launch_check(which == DFT_TWISTED ? "k_dft_inv_tab(twisted)" : "k_dft_inv_tab(plain)");
    case DFT_BIG_ROW: case DFT_BIG_BLOCKED: case DFT_BIG_DIRECT:
        return elph_dft_big_inv(h, p.form, which == DFT_TWISTED, outS, nu, N, nrhs, rvec, rz_part, nrz);
    default:
        return elph_dft_mfma_run(h, p, which, true, outS, reinterpret_cast<const double *>(nu), N, nrhs, st, rvec, rz_part, nrz);
    }
}

// the twisted pair (TimeFreqFFTs.jl: tau_to_omega!, omega_to_tau!): half spectrum k < ceil(L/2)
int elph_dft_fwd_twisted(elph_handle_s *h, double2 *nu, const double *vS, int N, int nrhs, const CgState *st) {
    return dft_fwd(h, plan(h, DFT_TWISTED, false, N, nrhs, 0), DFT_TWISTED, nu, vS, N, nrhs, st);
}
int elph_dft_inv_twisted(elph_handle_s *h, double *outS, const double2 *nu, int N, int nrhs, const CgState *st,
                         const double *rvec, double *rz_part, int nrz) {
    return dft_inv(h, plan(h, DFT_TWISTED, true, N, nrhs, rz_part ? nrz : 0), DFT_TWISTED, outS, nu, N, nrhs, st, rvec, rz_part, nrz);
}
// the plain (untwisted) pair: half spectrum k <= L/2
int elph_dft_fwd_plain(elph_handle_s *h, double2 *nu, const double *vS, int N, int nrhs) {
    return dft_fwd(h, plan(h, DFT_PLAIN, false, N, nrhs, 0), DFT_PLAIN, nu, vS, N, nrhs, nullptr);
}
int elph_dft_inv_plain(elph_handle_s *h, double *outS, const double2 *nu, int N, int nrhs) {
    return dft_inv(h, plan(h, DFT_PLAIN, true, N, nrhs, 0), DFT_PLAIN, outS, nu, N, nrhs, nullptr, nullptr, nullptr, 0);
}

// out = Re iFFT( diag^power .* FFT(in) ), N columns, nvec vectors sharing one diagonal
int elph_dft_accel(elph_handle_s *h, double *outS, const double *inS, const double *diagS, double power, int N, double2 *u, int nvec) {
    DftPlan pf = plan(h, DFT_PLAIN, false, N, nvec, 0), pi = plan(h, DFT_PLAIN, true, N, nvec, 0);
    elph_dft_pair(pf, pi);
    const bool in_epilogue = pf.form == DFT_SCALAR;      // the scalar forward kernel applies the diagonal itself
    RC(dft_fwd(h, pf, DFT_PLAIN, u, inS, N, nvec, nullptr, in_epilogue ? diagS : nullptr, power));
    if (!in_epilogue) {
        const int L = (int)h->L, Lh = L / 2 + 1;
        const long long total = (long long)nvec * Lh * N;
        hipLaunchKernelGGL(k_dft_diag, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, u, diagS, power, N, L, Lh, total);
        RC(elph_launch_check("k_dft_diag"));
    }
    return dft_inv(h, pi, DFT_PLAIN, outS, u, N, nvec, nullptr, nullptr, nullptr, 0);
}

int elph_dft_upload(void **dev, const void *src, size_t bytes) {
    HIPCHK(hipMalloc(dev, bytes));
    HIPCHK(hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice));
    return ELPH_OK;
}

void elph_dft_free(elph_handle_s *h) {
    DftState &D = h->dft;
    void *ptrs[] = {D.theta, D.Tk, D.Tt, D.Pk, D.Pt, D.W[0][0], D.W[0][1], D.W[1][0], D.W[1][1], D.W_r2[0], D.W_r2[1], D.r2_tw,
                    D.big_W1, D.big_W2, D.big_TW, D.big_a, D.big_b};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    D = DftState{};
}

// host: h->dft — the shape of the time axis and the tables of the forms it offers, with exact index reduction
int elph_dft_build_tables(elph_handle_s *h) {
    DftState &D = h->dft;
    D.shape = dft_shape(h->L);
    {
        std::vector<double2> theta((size_t)2 * h->L);
        for (size_t m = 0; m < theta.size(); ++m) {
            const double a = M_PI * (double)m / (double)h->L;
            theta[m] = make_double2(cos(a), -sin(a));
        }
        RC(elph_dft_upload((void **)&D.theta, theta.data(), theta.size() * sizeof(double2)));
    }
    if (D.shape.big()) return elph_dft_big_build_tables(h);
    const int L = (int)h->L, Lo2 = (L + 1) / 2, Lh = L / 2 + 1;
    const int Lp = dft_pad(L, 2 * DFT_TC), Kp2 = dft_pad(Lo2, 2 * DFT_KC), Kph = dft_pad(Lh, 2 * DFT_KC);
    const double2 zero = make_double2(0.0, 0.0);
    std::vector<double2> Tk((size_t)Lo2 * Lp, zero), Tt((size_t)L * Kp2, zero), Pk((size_t)Lh * Lp, zero), Pt((size_t)L * Kph, zero);
    const double invL = 1.0 / (double)L;
    for (int k = 0; k < Lo2; ++k) {
        // odd L: the middle frequency k = (L-1)/2 is its own mirror image (weight 1)
        const double wgt = ((L & 1) && k == Lo2 - 1) ? 1.0 : 2.0;
        for (int t = 0; t < L; ++t) {
            const long long m = ((long long)(2 * k + 1) * t) % (2LL * L);
            const double a = M_PI * (double)m / (double)L;
            Tk[(size_t)k * Lp + t] = make_double2(cos(a), -sin(a));                            // exp(-i a)
            Tt[(size_t)t * Kp2 + k] = make_double2(wgt * invL * cos(a), wgt * invL * sin(a));  // wgt/L exp(+i a)
        }
    }
    for (int k = 0; k < Lh; ++k) {
        const double wgt = (k == 0 || 2 * k == L) ? 1.0 : 2.0;
        for (int t = 0; t < L; ++t) {
            const long long m = ((long long)k * t) % L;
            const double a = 2.0 * M_PI * (double)m / (double)L;
            Pk[(size_t)k * Lp + t] = make_double2(cos(a), -sin(a));
            Pt[(size_t)t * Kph + k] = make_double2(wgt * invL * cos(a), wgt * invL * sin(a));
        }
    }
    struct { double2 **d; std::vector<double2> *v; } tabs[] = {{&D.Tk, &Tk}, {&D.Tt, &Tt}, {&D.Pk, &Pk}, {&D.Pt, &Pt}};
    for (auto &tb : tabs) RC(elph_dft_upload((void **)tb.d, tb.v->data(), tb.v->size() * sizeof(double2)));
    return elph_dft_mfma_build_tables(h);
}
