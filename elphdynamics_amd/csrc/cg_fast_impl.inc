// cg_fast_impl.inc — the lane-program kernels and their launchers for ONE sites-per-lane count ELPH_LP_NPL and one lane-program width
// ELPH_LP_MC (colours a lane keeps in registers: 4 for square / honeycomb / chain lattices, 6 for triangular), inside namespace LPNS.
// Compiled by cg_fast_npl.hip; what does not depend on the count is in cg_fast_shared.inc.  See cg_fast.hip.

namespace LPNS {

template <int NPL>
struct LaneProg {
    static constexpr int PP = (NPL + 1) / 2;     // passes per colour: ceil(N/2 / 64)
    static constexpr int NE = ELPH_LP_MC * PP;
    unsigned ij[NE];
};

template <int NPL>
__device__ __forceinline__ void lp_load_ij(unsigned (&ij)[ELPH_LP_MC * ((NPL + 1) / 2)], const ModelDev &m) {
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
#pragma unroll
    for (int e = 0; e < NE; ++e) ij[e] = m.lp_ij[e * WAVE + threadIdx.x];
}

template <int NPL>
__device__ __forceinline__ void lp_load_cs(double (&c)[ELPH_LP_MC * ((NPL + 1) / 2)], double (&s)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                           const double *lc, const double *ls) {
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        c[e] = lc[e * WAVE + threadIdx.x];
        s[e] = ls[e * WAVE + threadIdx.x];
    }
}

// one checkerboard sweep with register-resident bonds (Checkerboard.jl:57-83 / :149-175).
// Straight-line code: idle lanes of a ragged colour address two private padding slots of the slab with
// (c,s) = (1,0), so there is no per-lane predicate and the compiler batches all LDS reads of a colour.
template <int NPL, int NBUF, bool REVERSE>
__device__ __forceinline__ void lp_sweep(double *buf0, double *buf1, const unsigned (&ij)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                         const double (&c0)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&s0)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                         const double (&c1)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&s1)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                         int ncol) {
    constexpr int PP = (NPL + 1) / 2;
#pragma unroll
    for (int cc = 0; cc < ELPH_LP_MC; ++cc) {
        const int col = REVERSE ? ELPH_LP_MC - 1 - cc : cc;
        if (col < ncol) {
            double a0[PP], a1[PP], b0[PP], b1[PP];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const unsigned w = ij[col * PP + pp];
                const int i = w & 0xFFFF, j = w >> 16;
                a0[pp] = buf0[i]; a1[pp] = buf0[j];
                if (NBUF == 2) { b0[pp] = buf1[i]; b1[pp] = buf1[j]; }
            }
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const int e = col * PP + pp;
                const unsigned w = ij[e];
                const int i = w & 0xFFFF, j = w >> 16;
                buf0[i] = c0[e] * a0[pp] + s0[e] * a1[pp];
                buf0[j] = c0[e] * a1[pp] + s0[e] * a0[pp];
                if (NBUF == 2) {
                    buf1[i] = c1[e] * b0[pp] + s1[e] * b1[pp];
                    buf1[j] = c1[e] * b1[pp] + s1[e] * b0[pp];
                }
            }
            WAVE_LDS_ORDER();
        }
    }
}

// LDS slab of one tau-slice: NPL*64 site slots + 2 private padding slots per lane (idle lane-program entries)
template <int NPL>
__host__ __device__ constexpr int slab_len() { return NPL * WAVE + 2 * WAVE; }

// ------------------------------------------------------------------------------------------
// y = M v | M^T v | M^T M v   (same maths as k_mul in kernels.hip)
// All global loads are unconditional (site index clamped to N-1 for the lanes past a ragged N); LDS
// accesses need no predicate (slab padded to NPL*64); only global stores are guarded.
// ------------------------------------------------------------------------------------------

template <int NPL, int WHICH, bool SSH>
__global__ void __launch_bounds__(WAVE) k_mul_fast(double *__restrict__ y, const double *__restrict__ v, ModelDev m) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
    double *bufA = lds, *bufB = lds + slab_len<NPL>();
    const int N = m.N, L = m.L;
    int t, vecid;
    if (!xcd_map(L, t, vecid)) return;
    const int tm1 = (t == 0) ? L - 1 : t - 1;
    const int tp1 = (t == L - 1) ? 0 : t + 1;
    const size_t vec = (size_t)vecid * (size_t)N * (size_t)L;
    const double *vv = v + vec;
    double *yy = y + vec;
    const double sg0 = (t == 0) ? -1.0 : 1.0, sg1 = (tp1 == 0) ? -1.0 : 1.0;
    const double *Ech = m.E + (size_t)(vecid % m.nchains) * m.E_chain_stride;
    const double *E0 = Ech + (size_t)t * m.E_tau_stride, *E1 = Ech + (size_t)tp1 * m.E_tau_stride;

    unsigned ij[NE];
    double c0[NE], s0[NE], c1[NE], s1[NE];
    lp_load_ij<NPL>(ij, m);
    if (SSH) {
        ssh_chain_select(m, vecid);
        lp_load_cs<NPL>(c0, s0, m.lp_c + (size_t)t * m.lp_tau_stride, m.lp_s + (size_t)t * m.lp_tau_stride);
        lp_load_cs<NPL>(c1, s1, m.lp_c + (size_t)tp1 * m.lp_tau_stride, m.lp_s + (size_t)tp1 * m.lp_tau_stride);
    } else {
        lp_load_cs<NPL>(c0, s0, m.lp_c, m.lp_s);
    }
    double vm[NPL], v0[NPL], vp[NPL], e0[NPL], e1[NPL], w0[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const int sc = (s < N) ? s : N - 1;
        v0[q] = vv[(size_t)t * N + sc];
        if (WHICH != 1) { vm[q] = vv[(size_t)tm1 * N + sc]; e0[q] = E0[sc]; }
        if (WHICH != 0) { vp[q] = vv[(size_t)tp1 * N + sc]; e1[q] = E1[sc]; }
    }
    if (WHICH == 0) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) bufA[threadIdx.x + q * WAVE] = e0[q] * vm[q];
        WAVE_LDS_ORDER();
        lp_sweep<NPL, 1, false>(bufA, nullptr, ij, c0, s0, c0, s0, m.ncol);
#pragma unroll
        for (int q = 0; q < NPL; ++q) { const int s = threadIdx.x + q * WAVE; if (s < N) yy[(size_t)t * N + s] = v0[q] - sg0 * bufA[s]; }
    } else if (WHICH == 1) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) bufA[threadIdx.x + q * WAVE] = vp[q];
        WAVE_LDS_ORDER();
        if (SSH) lp_sweep<NPL, 1, true>(bufA, nullptr, ij, c1, s1, c1, s1, m.ncol);
        else lp_sweep<NPL, 1, true>(bufA, nullptr, ij, c0, s0, c0, s0, m.ncol);
#pragma unroll
        for (int q = 0; q < NPL; ++q) { const int s = threadIdx.x + q * WAVE; if (s < N) yy[(size_t)t * N + s] = v0[q] - sg1 * e1[q] * bufA[s]; }
    } else {
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            bufA[s] = e0[q] * vm[q];
            bufB[s] = e1[q] * v0[q];
        }
        WAVE_LDS_ORDER();
        if (SSH) lp_sweep<NPL, 2, false>(bufA, bufB, ij, c0, s0, c1, s1, m.ncol);
        else lp_sweep<NPL, 2, false>(bufA, bufB, ij, c0, s0, c0, s0, m.ncol);
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            w0[q] = v0[q] - sg0 * bufA[s];
            bufB[s] = vp[q] - sg1 * bufB[s];
        }
        WAVE_LDS_ORDER();
        if (SSH) lp_sweep<NPL, 1, true>(bufB, nullptr, ij, c1, s1, c1, s1, m.ncol);
        else lp_sweep<NPL, 1, true>(bufB, nullptr, ij, c0, s0, c0, s0, m.ncol);
#pragma unroll
        for (int q = 0; q < NPL; ++q) { const int s = threadIdx.x + q * WAVE; if (s < N) yy[(size_t)t * N + s] = w0[q] - sg1 * e1[q] * bufB[s]; }
    }
}

// ------------------------------------------------------------------------------------------
// CG kernels (IterativeSolvers.jl:153-314); see kernels.hip for the protocol between them.
// ------------------------------------------------------------------------------------------

#define IS_LEADER (t == 0)
template <int NPL, bool SSH>
__global__ void __launch_bounds__(WAVE) k_cg_ap_fast(CgBufs B, ModelDev m, int parity) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
    double *bufA = lds, *bufB = lds + slab_len<NPL>();
    const int N = m.N, L = m.L;
    int t, rhs;
    if (!xcd_map(L, t, rhs)) return;
    const size_t ndim = (size_t)N * L;
    const int tm1 = (t == 0) ? L - 1 : t - 1;
    const int tp1 = (t == L - 1) ? 0 : t + 1;

    // ---- every global load of the kernel, none depending on another ---------------------------
    CgState *st2 = B.state + 2 * rhs;
    const CgState S = ld_state(st2 + parity);        // this launch's copy; the other one is written below
    const CgParams P = B.params;
    const double *src = (P.use_prec ? B.zp : B.r) + (size_t)rhs * ndim;
    const double *pold = B.p + ((size_t)parity * B.nrhs + rhs) * ndim;
    double *pnew = B.p + ((size_t)(parity ^ 1) * B.nrhs + rhs) * ndim;
    double *z = B.z + (size_t)rhs * ndim;
    const double *Ech = m.E + (size_t)(rhs % m.nchains) * m.E_chain_stride;
    const double *E0 = Ech + (size_t)t * m.E_tau_stride, *E1 = Ech + (size_t)tp1 * m.E_tau_stride;

    double *x = B.x + (size_t)rhs * ndim;
    const double alpha_prev = B.alpha[rhs];          // step length of the previous iteration (unused when seq == 0)
    double sm[NPL], s0v[NPL], sp[NPL], qm[NPL], q0[NPL], qp[NPL], e0[NPL], e1[NPL], xv[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const int sc = (s < N) ? s : N - 1;
        const size_t im = (size_t)tm1 * N + sc, i0 = (size_t)t * N + sc, ip = (size_t)tp1 * N + sc;
        sm[q] = src[im]; s0v[q] = src[i0]; sp[q] = src[ip];
        qm[q] = pold[im]; q0[q] = pold[i0]; qp[q] = pold[ip];
        e0[q] = E0[sc]; e1[q] = E1[sc];
        xv[q] = x[i0];
    }
    unsigned ij[NE];
    double c0[NE], s0[NE], c1[NE], s1[NE];
    lp_load_ij<NPL>(ij, m);
    if (SSH) {
        ssh_chain_select(m, rhs);
        lp_load_cs<NPL>(c0, s0, m.lp_c + (size_t)t * m.lp_tau_stride, m.lp_s + (size_t)t * m.lp_tau_stride);
        lp_load_cs<NPL>(c1, s1, m.lp_c + (size_t)tp1 * m.lp_tau_stride, m.lp_s + (size_t)tp1 * m.lp_tau_stride);
    } else {
        lp_load_cs<NPL>(c0, s0, m.lp_c, m.lp_s);
    }
    const double rr = reduce_partials2(B.rr + (size_t)rhs * L, L);
    const double rz = P.use_prec ? reduce_partials2(B.rz + (size_t)rhs * B.nrz, B.nrz) : rr;

    // ---- scalar control (identical in every wave of this rhs) ----------------------------------
    CgState *Sout = st2 + (parity ^ 1);
    if (S.done) {                                     // keep both copies terminal: later launches alternate between them
        if (IS_LEADER && threadIdx.x == 0) *Sout = S;
        return;
    }
    const long long seq = S.seq;
    const bool first = (seq == 0);
    double beta = 0.0, rho = S.rho, kmin = S.kmin, eps = S.eps;
    if (!first) {
        // x += alpha p of the iteration whose stop test follows (IterativeSolvers.jl:205/282), with the p this launch reads anyway
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            if (s < N) x[(size_t)t * N + s] = xv[q] + alpha_prev * q0[q];
        }
        const int done = cg_stop_test(P, S, rr, seq, eps, kmin);
        if (t == 0 && threadIdx.x == 0 && P.record_hist) B.hist[(size_t)rhs * P.hist_stride + seq] = eps;
        if (done) {
            if (t == 0 && threadIdx.x == 0) {
                CgState o = S;
                o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = done;
                *Sout = o;
            }
            return;
        }
        beta = rz / S.rho;
        rho = rz;
    }

    // ---- p = (z|r) + beta p on slices t-1, t, t+1; stage E.*p into LDS ---------------------------
    double p0[NPL], pp[NPL], w0[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const double pm = first ? qm[q] : sm[q] + beta * qm[q];
        p0[q] = first ? q0[q] : s0v[q] + beta * q0[q];
        pp[q] = first ? qp[q] : sp[q] + beta * qp[q];
        bufA[s] = e0[q] * pm;
        bufB[s] = e1[q] * p0[q];
        if (s < N) pnew[(size_t)t * N + s] = p0[q];
    }
    WAVE_LDS_ORDER();
    const double sg0 = (t == 0) ? -1.0 : 1.0, sg1 = (tp1 == 0) ? -1.0 : 1.0;
    if (SSH) lp_sweep<NPL, 2, false>(bufA, bufB, ij, c0, s0, c1, s1, m.ncol);
    else lp_sweep<NPL, 2, false>(bufA, bufB, ij, c0, s0, c0, s0, m.ncol);
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        w0[q] = p0[q] - sg0 * bufA[s];
        bufB[s] = pp[q] - sg1 * bufB[s];
    }
    WAVE_LDS_ORDER();
    if (SSH) lp_sweep<NPL, 1, true>(bufB, nullptr, ij, c1, s1, c1, s1, m.ncol);
    else lp_sweep<NPL, 1, true>(bufB, nullptr, ij, c0, s0, c0, s0, m.ncol);
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const double zz = w0[q] - sg1 * e1[q] * bufB[s];
        if (s < N) {
            z[(size_t)t * N + s] = zz;
            acc += p0[q] * zz;
        }
    }
    acc = wave_sum2(acc);
    if (threadIdx.x == 0) {
        B.pap[(size_t)rhs * B.npap + t] = acc;
        if (t == 0) {
            CgState o = S;
            o.rho = rho; o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = 0;
            *Sout = o;
        }
    }
}

#undef IS_LEADER
#define IS_LEADER (ch == 0)
// combined pass: forward sweep on bufA (slice tau+1) and reverse sweep on bufB (w(tau)) in the same 4 stages
template <int NPL>
__device__ __forceinline__ void lp_sweep_fr(double *bufA, double *bufB, const unsigned (&ij)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                            const double (&cA)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&sA)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                            const double (&cB)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&sB)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                            int ncol, bool doA) {
    constexpr int PP = (NPL + 1) / 2;
#pragma unroll
    for (int cc = 0; cc < ELPH_LP_MC; ++cc) {
        const int colA = cc, colB = ELPH_LP_MC - 1 - cc;
        const bool onA = doA && (colA < ncol), onB = (colB < ncol);
        if (onA || onB) {
            double a0[PP], a1[PP], b0[PP], b1[PP];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                if (onA) { const unsigned w = ij[colA * PP + pp]; a0[pp] = bufA[w & 0xFFFF]; a1[pp] = bufA[w >> 16]; }
                if (onB) { const unsigned w = ij[colB * PP + pp]; b0[pp] = bufB[w & 0xFFFF]; b1[pp] = bufB[w >> 16]; }
            }
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                if (onA) {
                    const int e = colA * PP + pp; const unsigned w = ij[e];
                    bufA[w & 0xFFFF] = cA[e] * a0[pp] + sA[e] * a1[pp];
                    bufA[w >> 16] = cA[e] * a1[pp] + sA[e] * a0[pp];
                }
                if (onB) {
                    const int e = colB * PP + pp; const unsigned w = ij[e];
                    bufB[w & 0xFFFF] = cB[e] * b0[pp] + sB[e] * b1[pp];
                    bufB[w >> 16] = cB[e] * b1[pp] + sB[e] * b0[pp];
                }
            }
            WAVE_LDS_ORDER();
        }
    }
}

// Batched-throughput variant of k_cg_ap_fast: one wave owns T consecutive tau-slices of one right-hand side.
//   w(t) = p(t) - sg(t) CB_t [E(t) .* p(t-1)]            needs T+1 forward sweeps  (t = t0 .. t0+T)
//   z(t) = w(t) - sg(t+1) E(t+1) .* CB_{t+1}^T w(t+1)    needs T   reverse sweeps
// The reverse sweep of w(t0+j) and the forward sweep of slice t0+j+1 run in the SAME four colour stages
// (independent LDS slabs), so a slice costs 4 stages instead of 8 and ~3 slice loads instead of 8; the next
// slice's loads are issued one stage ahead.  Results are bit-identical to the T=1 kernel (same operations per
// element, same order), only the p.z partial sums are grouped per chunk instead of per slice.
// (chunk_block_map — which (right-hand side, chunk) a block works on: cg_fast_common.h, shared with cg_sq16.hip)

// PX (preconditioned batches, Holstein): the search direction arrives READY in B.p (slot 0) — the inverse tau-transform of the previous
// iteration formed p = P^-1 r + beta p and applied x += alpha p in its epilogue (dft_mfma.hip: PxFuse) — so this kernel reads p (own
// slices + two halo slices) and exp(-dtau V), writes z and the p.z partials, and keeps the scalar state machine (stop test, rho)
// exactly as without PX: 2.6 vectors of traffic instead of 6.7.
template <int NPL, int T, bool SSH, bool PX>
__device__ __forceinline__ void cg_ap_chunk_body(const CgBufs &B, ModelDev &m, int parity_order) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
    double *bufA = lds, *bufB = lds + slab_len<NPL>();
    const int N = m.N, L = m.L;
    const int nch = L / T;
    const int parity = parity_order & 1;
    int rhs, ch;
    chunk_block_map((int)blockIdx.x, B.nrhs, nch, m.nchains > 0 ? m.nchains : 1, parity_order >> 1, rhs, ch);
    const int t0 = ch * T;
    const size_t ndim = (size_t)N * L;
    auto wrap = [L](int t) { return (t < 0) ? t + L : ((t >= L) ? t - L : t); };

    CgState *st2 = B.state + 2 * rhs;
    const CgState S = ld_state(st2 + parity);        // this launch's copy; the other one is written below
    const CgParams P = B.params;
    const double *src = PX ? B.p + (size_t)rhs * ndim : (P.use_prec ? B.zp : B.r) + (size_t)rhs * ndim;
    const double *pold = B.p + ((size_t)(PX ? 0 : parity) * B.nrhs + rhs) * ndim;
    double *pnew = B.p + ((size_t)(parity ^ 1) * B.nrhs + rhs) * ndim;
    double *z = B.z + (size_t)rhs * ndim;
    double *x = B.x + (size_t)rhs * ndim;
    const double alpha_prev = B.alpha[rhs];          // step length of the previous iteration (unused when seq == 0)

    int sc[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) { const int s = threadIdx.x + q * WAVE; sc[q] = (s < N) ? s : N - 1; }
    auto load_sq = [&](int t, double (&sv)[NPL], double (&qv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) { const size_t i = (size_t)t * N + sc[q]; sv[q] = src[i]; qv[q] = PX ? 0.0 : pold[i]; }
    };
    auto load_e = [&](int t, double (&ev)[NPL]) {
        const double *Et = m.E + (size_t)(rhs % m.nchains) * m.E_chain_stride + (size_t)t * m.E_tau_stride;
#pragma unroll
        for (int q = 0; q < NPL; ++q) ev[q] = Et[sc[q]];
    };
    auto load_x = [&](int t, double (&xv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) xv[q] = x[(size_t)t * N + sc[q]];
    };
    // x(t) += alpha_prev p_old(t) for an OWN slice (t0 <= t < t0+T), with the p_old values this launch has in registers
    auto update_x = [&](int t, const double (&xv)[NPL], const double (&qv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            if (s < N) x[(size_t)t * N + s] = xv[q] + alpha_prev * qv[q];
        }
    };

    // ---- prologue loads (independent of everything) ----------------------------------------------
    double Sm[NPL], Qm[NPL], S0[NPL], Q0[NPL], S1[NPL], Q1[NPL], E0[NPL], E1[NPL], X0[NPL], X1[NPL];
    load_sq(wrap(t0 - 1), Sm, Qm);
    load_sq(t0, S0, Q0);
    load_sq(wrap(t0 + 1), S1, Q1);
    load_e(t0, E0);
    load_e(wrap(t0 + 1), E1);
    if (!PX) {
        load_x(t0, X0);
        if (T > 1) load_x(t0 + 1, X1);               // t0 + 1 <= L - 1 whenever T > 1 (T divides L)
    }
    unsigned ij[NE];
    double cA[NE], sA[NE], cB[NE], sB[NE];
    lp_load_ij<NPL>(ij, m);
    if (SSH) {
        ssh_chain_select(m, rhs);
        lp_load_cs<NPL>(cA, sA, m.lp_c + (size_t)t0 * m.lp_tau_stride, m.lp_s + (size_t)t0 * m.lp_tau_stride);
        lp_load_cs<NPL>(cB, sB, m.lp_c + (size_t)wrap(t0 + 1) * m.lp_tau_stride, m.lp_s + (size_t)wrap(t0 + 1) * m.lp_tau_stride);
    } else {
        lp_load_cs<NPL>(cA, sA, m.lp_c, m.lp_s);
    }
    const double rr = reduce_partials2(B.rr + (size_t)rhs * L, L);
    const double rz = P.use_prec ? reduce_partials2(B.rz + (size_t)rhs * B.nrz, B.nrz) : rr;

    // ---- scalar control (identical in every wave of this rhs; same code as k_cg_ap_fast) -----------
    CgState *Sout = st2 + (parity ^ 1);
    if (S.done) {                                     // keep both copies terminal: later launches alternate between them
        if (IS_LEADER && threadIdx.x == 0) *Sout = S;
        return;
    }
    const long long seq = S.seq;
    const bool first = (seq == 0);
    double beta = 0.0, rho = S.rho, kmin = S.kmin, eps = S.eps;
    if (!first) {
        const int done = cg_stop_test(P, S, rr, seq, eps, kmin);
        if (ch == 0 && threadIdx.x == 0 && P.record_hist) B.hist[(size_t)rhs * P.hist_stride + seq] = eps;
        if (done) {
            // the solve ends here: apply the pending x += alpha p of the last iteration to all own slices, then leave
            // (PX: the inverse transform has applied it already)
            if (!PX) {
                update_x(t0, X0, Q0);
                if (T > 1) update_x(t0 + 1, X1, Q1);
                for (int j = 2; j < T; ++j) {
                    double xv[NPL], qv[NPL];
#pragma unroll
                    for (int q = 0; q < NPL; ++q) { const size_t i = (size_t)(t0 + j) * N + sc[q]; xv[q] = x[i]; qv[q] = pold[i]; }
                    update_x(t0 + j, xv, qv);
                }
            }
            if (ch == 0 && threadIdx.x == 0) {
                CgState o = S;
                o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = done;
                *Sout = o;
            }
            return;
        }
        if (!PX) {
            update_x(t0, X0, Q0);
            if (T > 1) update_x(t0 + 1, X1, Q1);
        }
        beta = rz / S.rho;
        rho = rz;
    }
    auto pval = [&](double sv, double qv) { return PX ? sv : (first ? qv : sv + beta * qv); };
    auto sgn = [](int t) { return (t == 0) ? -1.0 : 1.0; };

    // ---- prologue: w(t0), w(t0+1) by one two-slab forward sweep --------------------------------------
    double pprev[NPL], pcur[NPL], wprev[NPL], wcur[NPL], Ecur[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const double pm = pval(Sm[q], Qm[q]);
        pprev[q] = pval(S0[q], Q0[q]);
        pcur[q] = pval(S1[q], Q1[q]);
        bufA[s] = E0[q] * pm;
        bufB[s] = E1[q] * pprev[q];
        Ecur[q] = E1[q];
        if (!PX && s < N) pnew[(size_t)t0 * N + s] = pprev[q];
    }
    WAVE_LDS_ORDER();
    if (SSH) lp_sweep<NPL, 2, false>(bufA, bufB, ij, cA, sA, cB, sB, m.ncol);
    else lp_sweep<NPL, 2, false>(bufA, bufB, ij, cA, sA, cA, sA, m.ncol);
    {
        const double sga = sgn(t0), sgb = sgn(wrap(t0 + 1));
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            wprev[q] = pprev[q] - sga * bufA[s];
            wcur[q] = pcur[q] - sgb * bufB[s];
        }
    }
    WAVE_LDS_ORDER();

    // ---- pipelined stages: reverse sweep of w(t0+j)  ||  forward sweep of slice t0+j+1 ---------------
    double acc = 0.0;
    // Slices t0+2 … t0+T stream through a register ring PF stages deep: a stage (four colour sweeps) lasts ~0.3 us, an HBM
    // round trip under load several times that, and at ~1.25 waves per SIMD nothing else hides it — the registers are free.
    // (the SSH variant also keeps two sets of per-slice hopping tables: a ring of depth 1 keeps it under 256 registers, i.e. at two
    //  waves per SIMD, which matters more than the second slice in flight — 1280 waves do not fit 1024 SIMDs in one round)
    constexpr int PF = (SSH || NPL >= 5 || (ELPH_LP_MC == 6 && NPL >= 4)) ? 1 : ((T >= 4) ? 2 : 1);   // (more sites per lane / six-colour lane programs: the same register argument)
    static_assert(T <= 20, "chunk length");
    double Sr[PF][NPL], Qr[PF][NPL], Er[PF][NPL], Xr[PF][NPL];
#pragma unroll
    for (int k = 0; k < PF; ++k)
        if (k + 2 <= T) {
            load_sq(wrap(t0 + 2 + k), Sr[k], Qr[k]);
            load_e(wrap(t0 + 2 + k), Er[k]);
            if (!PX && k + 2 < T) load_x(t0 + 2 + k, Xr[k]);   // own slices only (the last ring slice, t0+T, is halo)
        }
#pragma unroll
    for (int j = 1; j <= T; ++j) {
        const int tj = wrap(t0 + j);              // slice whose w is reverse-swept now
        const int tn = wrap(t0 + j + 1);          // slice forward-swept now (if j < T)
        const bool more = (j < T);
        double (&Sn)[NPL] = Sr[(j - 1) % PF];     // slice tn in the ring (compile-time slot: the loop is unrolled)
        double (&Qn)[NPL] = Qr[(j - 1) % PF];
        double (&En)[NPL] = Er[(j - 1) % PF];
        double (&Xn)[NPL] = Xr[(j - 1) % PF];
        if (SSH) {
            // B-side tables: slice tj — the A-side tables of the previous stage (stage 1: already in cB from the opening sweep),
            // handed over in registers (the loop is unrolled: a rename, not a copy); A-side: slice tn, the only table load per stage
            if (j > 1) {
#pragma unroll
                for (int e = 0; e < NE; ++e) { cB[e] = cA[e]; sB[e] = sA[e]; }
            }
            if (more) lp_load_cs<NPL>(cA, sA, m.lp_c + (size_t)tn * m.lp_tau_stride, m.lp_s + (size_t)tn * m.lp_tau_stride);
        }
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            bufB[s] = wcur[q];
            if (more) bufA[s] = En[q] * pcur[q];          // E(tn) .* p(tj)
        }
        WAVE_LDS_ORDER();
        if (SSH) lp_sweep_fr<NPL>(bufA, bufB, ij, cA, sA, cB, sB, m.ncol, more);
        else lp_sweep_fr<NPL>(bufA, bufB, ij, cA, sA, cA, sA, m.ncol, more);
        const double sgj = sgn(tj), sgnn = sgn(tn);
        double pnext[NPL], wnext[NPL];
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            const double zz = wprev[q] - sgj * Ecur[q] * bufB[s];        // z(t0+j-1)
            if (s < N) {
                z[(size_t)wrap(t0 + j - 1) * N + s] = zz;
                acc += pprev[q] * zz;
            }
            if (more) {
                pnext[q] = pval(Sn[q], Qn[q]);                           // p(tn)
                wnext[q] = pnext[q] - sgnn * bufA[s];                    // w(tn)
                if (!PX && s < N) pnew[(size_t)tj * N + s] = pcur[q];
            }
        }
        if (!PX && !first && j + 1 < T) update_x(t0 + j + 1, Xn, Qn);    // tn = t0+j+1 is an own slice
        WAVE_LDS_ORDER();
        if (more) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                wprev[q] = wcur[q]; wcur[q] = wnext[q];
                pprev[q] = pcur[q]; pcur[q] = pnext[q];
                Ecur[q] = En[q];
            }
            if (j + 1 + PF <= T) {                                        // refill this slot
                load_sq(wrap(t0 + j + 1 + PF), Sn, Qn);
                load_e(wrap(t0 + j + 1 + PF), En);
                if (!PX && j + 1 + PF < T) load_x(t0 + j + 1 + PF, Xn);
            }
        }
    }
    acc = wave_sum2(acc);
    if (threadIdx.x == 0) {
        B.pap[(size_t)rhs * B.npap + ch] = acc;
        if (ch == 0) {
            CgState o = S;
            o.rho = rho; o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = 0;
            *Sout = o;
        }
    }
}

template <int NPL, int T, bool SSH>
__global__ void __launch_bounds__(WAVE) k_cg_ap_chunk(CgBufs B, ModelDev m, int parity_order) {
    cg_ap_chunk_body<NPL, T, SSH, false>(B, m, parity_order);
}
// the p/x-fused form needs a third fewer registers: compiled for three waves per SIMD (288 right-hand sides x 10 chunks of 16 slices are
// 2880 waves — one round of the chip's 3072 slots at three per SIMD, one and a half at two)
template <int NPL, int T>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(3, 3))) k_cg_ap_chunk_px(CgBufs B, ModelDev m, int parity_order) {
    cg_ap_chunk_body<NPL, T, false, true>(B, m, parity_order);
}
// five and more sites per lane (the honeycomb lattice of config D: 288 sites) do not fit three waves per SIMD — the capped kernel spills
// 200-600 bytes per lane and the fused iteration LOSES to the unfused one (D, 256 right-hand sides: 310 against 249 us,
// profiles/r05/px_fused_five_sites_per_lane.log): two waves per SIMD for them
template <int NPL, int T>
__global__ void __launch_bounds__(WAVE) k_cg_ap_chunk_px2(CgBufs B, ModelDev m, int parity_order) {
    cg_ap_chunk_body<NPL, T, false, true>(B, m, parity_order);
}
// bond phonons (two sets of per-slice hopping tables in registers): two waves per SIMD, like the unfused form — but without the six
// vectors of p-/x-update traffic
template <int NPL, int T>
__global__ void __launch_bounds__(WAVE) k_cg_ap_chunk_px_ssh(CgBufs B, ModelDev m, int parity_order) {
    cg_ap_chunk_body<NPL, T, true, true>(B, m, parity_order);
}

// The same kernel with the chunk length as a RUN-TIME number and a ragged last chunk (Tmax slices per wave, the last wave of a
// right-hand side takes what is left): the slice loop is rolled (two statically indexed stages of the register ring per trip), so any
// chunk length costs the same ~10 KB of code (the unrolled form: 61 KB at 20 slices, past the instruction cache at 32) and the host
// can cut the time axis so that the waves of a batch fill the chip's wave slots in ONE round — 288 right-hand sides x 8 chunks of 20 are
// 2304 waves for 2048 slots (two rounds, the second an eighth full: 141 us); 7 chunks of 23,...,22 are 2016 (one round).
// Same operations per element in the same order as the unrolled kernel; the p.z partial sums are grouped per chunk.
template <int NPL, bool SSH>
__global__ void __launch_bounds__(WAVE) k_cg_ap_chunk_rt(CgBufs B, ModelDev m, int parity, int Tmax) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
    double *bufA = lds, *bufB = lds + slab_len<NPL>();
    const int N = m.N, L = m.L;
    const int nch = (L + Tmax - 1) / Tmax;
    const int rhs = blockIdx.x / nch, ch = blockIdx.x - rhs * nch;
    const int t0 = ch * Tmax;
    const int T = (L - t0 < Tmax) ? L - t0 : Tmax;                 // slices of this wave (>= 2: the host's choice of Tmax)
    const size_t ndim = (size_t)N * L;
    auto wrap = [L](int t) { return (t < 0) ? t + L : ((t >= L) ? t - L : t); };

    CgState *st2 = B.state + 2 * rhs;
    const CgState S = ld_state(st2 + parity);        // this launch's copy; the other one is written below
    const CgParams P = B.params;
    const double *src = (P.use_prec ? B.zp : B.r) + (size_t)rhs * ndim;
    const double *pold = B.p + ((size_t)parity * B.nrhs + rhs) * ndim;
    double *pnew = B.p + ((size_t)(parity ^ 1) * B.nrhs + rhs) * ndim;
    double *z = B.z + (size_t)rhs * ndim;
    double *x = B.x + (size_t)rhs * ndim;
    const double alpha_prev = B.alpha[rhs];          // step length of the previous iteration (unused when seq == 0)

    int sc[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) { const int s = threadIdx.x + q * WAVE; sc[q] = (s < N) ? s : N - 1; }
    auto load_sq = [&](int t, double (&sv)[NPL], double (&qv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) { const size_t i = (size_t)t * N + sc[q]; sv[q] = src[i]; qv[q] = pold[i]; }
    };
    auto load_e = [&](int t, double (&ev)[NPL]) {
        const double *Et = m.E + (size_t)(rhs % m.nchains) * m.E_chain_stride + (size_t)t * m.E_tau_stride;
#pragma unroll
        for (int q = 0; q < NPL; ++q) ev[q] = Et[sc[q]];
    };
    auto load_x = [&](int t, double (&xv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) xv[q] = x[(size_t)t * N + sc[q]];
    };
    // x(t) += alpha_prev p_old(t) for an OWN slice (t0 <= t < t0+T), with the p_old values this launch has in registers
    auto update_x = [&](int t, const double (&xv)[NPL], const double (&qv)[NPL]) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            if (s < N) x[(size_t)t * N + s] = xv[q] + alpha_prev * qv[q];
        }
    };

    // ---- prologue loads (independent of everything) ----------------------------------------------
    double Sm[NPL], Qm[NPL], S0[NPL], Q0[NPL], S1[NPL], Q1[NPL], E0[NPL], E1[NPL], X0[NPL], X1[NPL];
    load_sq(wrap(t0 - 1), Sm, Qm);
    load_sq(t0, S0, Q0);
    load_sq(wrap(t0 + 1), S1, Q1);
    load_e(t0, E0);
    load_e(wrap(t0 + 1), E1);
    load_x(t0, X0);
    load_x(t0 + 1, X1);                              // (T >= 2)
    unsigned ij[NE];
    double cA[NE], sA[NE], cB[NE], sB[NE];
    lp_load_ij<NPL>(ij, m);
    if (SSH) {
        ssh_chain_select(m, rhs);
        lp_load_cs<NPL>(cA, sA, m.lp_c + (size_t)t0 * m.lp_tau_stride, m.lp_s + (size_t)t0 * m.lp_tau_stride);
        lp_load_cs<NPL>(cB, sB, m.lp_c + (size_t)wrap(t0 + 1) * m.lp_tau_stride, m.lp_s + (size_t)wrap(t0 + 1) * m.lp_tau_stride);
    } else {
        lp_load_cs<NPL>(cA, sA, m.lp_c, m.lp_s);
    }
    const double rr = reduce_partials2(B.rr + (size_t)rhs * L, L);
    const double rz = P.use_prec ? reduce_partials2(B.rz + (size_t)rhs * B.nrz, B.nrz) : rr;

    // ---- scalar control (identical in every wave of this rhs; same code as k_cg_ap_fast) -----------
    CgState *Sout = st2 + (parity ^ 1);
    if (S.done) {                                     // keep both copies terminal: later launches alternate between them
        if (IS_LEADER && threadIdx.x == 0) *Sout = S;
        return;
    }
    const long long seq = S.seq;
    const bool first = (seq == 0);
    double beta = 0.0, rho = S.rho, kmin = S.kmin, eps = S.eps;
    if (!first) {
        const int done = cg_stop_test(P, S, rr, seq, eps, kmin);
        if (ch == 0 && threadIdx.x == 0 && P.record_hist) B.hist[(size_t)rhs * P.hist_stride + seq] = eps;
        if (done) {
            // the solve ends here: apply the pending x += alpha p of the last iteration to all own slices, then leave
            update_x(t0, X0, Q0);
            update_x(t0 + 1, X1, Q1);
            for (int j = 2; j < T; ++j) {
                double xv[NPL], qv[NPL];
#pragma unroll
                for (int q = 0; q < NPL; ++q) { const size_t i = (size_t)(t0 + j) * N + sc[q]; xv[q] = x[i]; qv[q] = pold[i]; }
                update_x(t0 + j, xv, qv);
            }
            if (ch == 0 && threadIdx.x == 0) {
                CgState o = S;
                o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = done;
                *Sout = o;
            }
            return;
        }
        update_x(t0, X0, Q0);
        update_x(t0 + 1, X1, Q1);
        beta = rz / S.rho;
        rho = rz;
    }
    auto pval = [&](double sv, double qv) { return first ? qv : sv + beta * qv; };
    auto sgn = [](int t) { return (t == 0) ? -1.0 : 1.0; };

    // ---- prologue: w(t0), w(t0+1) by one two-slab forward sweep --------------------------------------
    double pprev[NPL], pcur[NPL], wprev[NPL], wcur[NPL], Ecur[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const double pm = pval(Sm[q], Qm[q]);
        pprev[q] = pval(S0[q], Q0[q]);
        pcur[q] = pval(S1[q], Q1[q]);
        bufA[s] = E0[q] * pm;
        bufB[s] = E1[q] * pprev[q];
        Ecur[q] = E1[q];
        if (s < N) pnew[(size_t)t0 * N + s] = pprev[q];
    }
    WAVE_LDS_ORDER();
    if (SSH) lp_sweep<NPL, 2, false>(bufA, bufB, ij, cA, sA, cB, sB, m.ncol);
    else lp_sweep<NPL, 2, false>(bufA, bufB, ij, cA, sA, cA, sA, m.ncol);
    {
        const double sga = sgn(t0), sgb = sgn(wrap(t0 + 1));
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            wprev[q] = pprev[q] - sga * bufA[s];
            wcur[q] = pcur[q] - sgb * bufB[s];
        }
    }
    WAVE_LDS_ORDER();

    // ---- pipelined stages: reverse sweep of w(t0+j)  ||  forward sweep of slice t0+j+1 ---------------
    double acc = 0.0;
    // Slices t0+2 … t0+T stream through a register ring PF stages deep: a stage (four colour sweeps) lasts ~0.3 us, an HBM
    // round trip under load several times that, and at ~1.25 waves per SIMD nothing else hides it — the registers are free.
    // (the SSH variant also keeps two sets of per-slice hopping tables: a ring of depth 1 keeps it under 256 registers, i.e. at two
    //  waves per SIMD, which matters more than the second slice in flight — 1280 waves do not fit 1024 SIMDs in one round)
    constexpr int PF = (SSH || NPL >= 5 || (ELPH_LP_MC == 6 && NPL >= 4)) ? 1 : 2;   // (more sites per lane / six-colour lane programs: the same register argument)
    double Sr[PF][NPL], Qr[PF][NPL], Er[PF][NPL], Xr[PF][NPL];
#pragma unroll
    for (int k = 0; k < PF; ++k)
        if (k + 2 <= T) {
            load_sq(wrap(t0 + 2 + k), Sr[k], Qr[k]);
            load_e(wrap(t0 + 2 + k), Er[k]);
            if (k + 2 < T) load_x(t0 + 2 + k, Xr[k]);          // own slices only (the last ring slice, t0+T, is halo)
        }
#pragma unroll 1
    for (int j0 = 1; j0 <= T; j0 += PF) {
#pragma unroll
    for (int kk = 0; kk < PF; ++kk) {
        const int j = j0 + kk;
        if (j > T) break;
        const int tj = wrap(t0 + j);              // slice whose w is reverse-swept now
        const int tn = wrap(t0 + j + 1);          // slice forward-swept now (if j < T)
        const bool more = (j < T);
        double (&Sn)[NPL] = Sr[kk];               // slice tn in the ring (compile-time slot: stage j0 + kk uses slot kk)
        double (&Qn)[NPL] = Qr[kk];
        double (&En)[NPL] = Er[kk];
        double (&Xn)[NPL] = Xr[kk];
        if (SSH) {
            // B-side tables: slice tj — the A-side tables of the previous stage (stage 1: already in cB from the opening sweep),
            // handed over in registers (the loop is unrolled: a rename, not a copy); A-side: slice tn, the only table load per stage
            if (j > 1) {
#pragma unroll
                for (int e = 0; e < NE; ++e) { cB[e] = cA[e]; sB[e] = sA[e]; }
            }
            if (more) lp_load_cs<NPL>(cA, sA, m.lp_c + (size_t)tn * m.lp_tau_stride, m.lp_s + (size_t)tn * m.lp_tau_stride);
        }
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            bufB[s] = wcur[q];
            if (more) bufA[s] = En[q] * pcur[q];          // E(tn) .* p(tj)
        }
        WAVE_LDS_ORDER();
        if (SSH) lp_sweep_fr<NPL>(bufA, bufB, ij, cA, sA, cB, sB, m.ncol, more);
        else lp_sweep_fr<NPL>(bufA, bufB, ij, cA, sA, cA, sA, m.ncol, more);
        const double sgj = sgn(tj), sgnn = sgn(tn);
        double pnext[NPL], wnext[NPL];
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = threadIdx.x + q * WAVE;
            const double zz = wprev[q] - sgj * Ecur[q] * bufB[s];        // z(t0+j-1)
            if (s < N) {
                z[(size_t)wrap(t0 + j - 1) * N + s] = zz;
                acc += pprev[q] * zz;
            }
            if (more) {
                pnext[q] = pval(Sn[q], Qn[q]);                           // p(tn)
                wnext[q] = pnext[q] - sgnn * bufA[s];                    // w(tn)
                if (s < N) pnew[(size_t)tj * N + s] = pcur[q];
            }
        }
        if (!first && j + 1 < T) update_x(t0 + j + 1, Xn, Qn);           // tn = t0+j+1 is an own slice
        WAVE_LDS_ORDER();
        if (more) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                wprev[q] = wcur[q]; wcur[q] = wnext[q];
                pprev[q] = pcur[q]; pcur[q] = pnext[q];
                Ecur[q] = En[q];
            }
            if (j + 1 + PF <= T) {                                        // refill this slot
                load_sq(wrap(t0 + j + 1 + PF), Sn, Qn);
                load_e(wrap(t0 + j + 1 + PF), En);
                if (j + 1 + PF < T) load_x(t0 + j + 1 + PF, Xn);
            }
        }
    }
    }
    acc = wave_sum2(acc);
    if (threadIdx.x == 0) {
        B.pap[(size_t)rhs * B.npap + ch] = acc;
        if (ch == 0) {
            CgState o = S;
            o.rho = rho; o.kmin = kmin; o.eps = eps; o.seq = seq + 1; o.iters = seq; o.done = 0;
            *Sout = o;
        }
    }
}

#undef IS_LEADER
template <int NPL>
__global__ void __launch_bounds__(WAVE) k_cg_xr_fast(CgBufs B, int N, int L, int parity) {
    // r -= alpha z and the partial r.r.  x += alpha p is NOT done here: the next k_cg_ap reads this p anyway (as its p_old),
    // so it applies the update there and this kernel moves 24 B per element instead of 48 (alpha travels in B.alpha).
    int t, rhs;
    if (!xcd_map(L, t, rhs)) return;
    const size_t ndim = (size_t)N * L;
    const CgState S = ld_state(B.state + 2 * rhs + parity);   // written by the k_cg_ap launch just before
    const double *z = B.z + (size_t)rhs * ndim;
    double *r = B.r + (size_t)rhs * ndim;
    double rv[NPL], zv[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        const size_t i = (size_t)t * N + ((s < N) ? s : N - 1);
        rv[q] = r[i]; zv[q] = z[i];
    }
    const double pap = reduce_partials2(B.pap + (size_t)rhs * B.npap, B.npap);
    if (S.done) return;
    const double alpha = S.rho / pap;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = threadIdx.x + q * WAVE;
        if (s < N) {
            const size_t i = (size_t)t * N + s;
            const double rn = rv[q] - alpha * zv[q];
            r[i] = rn;
            acc += rn * rn;
        }
    }
    acc = wave_sum2(acc);
    if (threadIdx.x == 0) {
        B.rr[(size_t)rhs * L + t] = acc;
        if (t == 0) B.alpha[rhs] = alpha;
    }
}

// ------------------------------------------------------------------------------------------
// KPM Chebyshev recursion, re/im-split variant.
// A' is real, so the real and the imaginary part of u_n obey the SAME real three-term recursion and never
// mix; only the coefficient sums do.  One 128-thread workgroup per frequency block: wave 0 carries Re u,
// wave 1 carries Im u, each in its own LDS slab (half the LDS bytes and half the instructions per wave of the
// complex kernel), each accumulating P = sum cx_n u_n and Q = sum cy_n u_n; the halves are combined
// through LDS once per series:
//     conj coefficients (first series):  Re = P_re + Q_im,  Im = P_im - Q_re
//     plain coefficients (second):       Re = P_re - Q_im,  Im = P_im + Q_re
// LDS addresses of a lane's bonds are precomputed pointers (no per-access address arithmetic).
// ------------------------------------------------------------------------------------------

template <int NPL, bool REVERSE>
__device__ __forceinline__ void lp_sweep_ptr(double *const (&pi)[ELPH_LP_MC * ((NPL + 1) / 2)], double *const (&pj)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                             const double (&c)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&s)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                             int ncol) {
    constexpr int PP = (NPL + 1) / 2;
#pragma unroll
    for (int cc = 0; cc < ELPH_LP_MC; ++cc) {
        const int col = REVERSE ? ELPH_LP_MC - 1 - cc : cc;
        if (col < ncol) {
            double a0[PP], a1[PP];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) { a0[pp] = *pi[col * PP + pp]; a1[pp] = *pj[col * PP + pp]; }
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const int e = col * PP + pp;
                *pi[e] = c[e] * a0[pp] + s[e] * a1[pp];
                *pj[e] = c[e] * a1[pp] + s[e] * a0[pp];
            }
            WAVE_LDS_ORDER();
        }
    }
}

template <int NPL, bool TRANSPOSED>
__device__ __forceinline__ void kpm_series_ri(double (&P)[NPL], double (&Q)[NPL], const double (&vin)[NPL], double *slab,
                                              const double (&eb)[NPL], const double2 *c, int order, double a, double b,
                                              double *const (&pi)[ELPH_LP_MC * ((NPL + 1) / 2)], double *const (&pj)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                              const double (&cb)[ELPH_LP_MC * ((NPL + 1) / 2)], const double (&sb)[ELPH_LP_MC * ((NPL + 1) / 2)],
                                              int ncol) {
    double um1[NPL], un[NPL];
    const int lane = threadIdx.x & (WAVE - 1);
    {
        const double2 c0 = c[0];
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            P[q] = c0.x * vin[q];
            Q[q] = c0.y * vin[q];
            un[q] = vin[q];
            um1[q] = 0.0;
        }
    }
    for (int n = 2; n <= order; ++n) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) slab[lane + q * WAVE] = TRANSPOSED ? un[q] : eb[q] * un[q];
        WAVE_LDS_ORDER();
        lp_sweep_ptr<NPL, TRANSPOSED>(pi, pj, cb, sb, ncol);
        const double2 cn = c[n - 1];
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            double av = slab[lane + q * WAVE];
            if (TRANSPOSED) av *= eb[q];
            double up = a * av - b * un[q];                    // A' u_n   (mulA'!, :685-693)
            if (n > 2) up = 2.0 * up - um1[q];                 // u_{n+1} = 2 A' u_n - u_{n-1}
            um1[q] = un[q];
            un[q] = up;
            P[q] += cn.x * up;
            Q[q] += cn.y * up;
        }
        WAVE_LDS_ORDER();
    }
}

template <int NPL>
// rz_part != nullptr (round 6): the r.(P^-1 r) partial sums in frequency space, slot 2 blockIdx.y + wave (the contract of kpm_cheb_sq_body,
// cg_fast_shared.inc) — the p/x-fused iteration for lane-program lattices without a register-exchange recursion (square L = 22, hopping
// disorder on honeycomb lattices, ...)
__global__ void __launch_bounds__(2 * WAVE) k_kpm_cheb_ri(double2 *__restrict__ nu, KpmDev K, ModelDev m, int Lo2,
                                                          const CgState *state, double *__restrict__ rz_part, int nrz,
                                                          const double *__restrict__ rr_part) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NE = ELPH_LP_MC * ((NPL + 1) / 2);
    constexpr int SL = slab_len<NPL>();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
    double *slab = lds + wv * SL;                 // this wave's component slab
    double *xch = lds + 2 * SL;                   // exchange area [2][NPL*64]
    const int rhs = blockIdx.x;   // x = right-hand side, y = frequency in longest-first order: ALL long recursions are dispatched first
    if (state && ld_state(state + 2 * rhs).done) return;   // `state` points at the current copy (host adds the parity)
    const KpmChainView V = kpm_chain_view(K, rhs, m.N);
    const int w = V.wsched[blockIdx.y];
    const int N = m.N;
    const int order = V.order[w];
    const double2 *c = K.coeff + V.coff[w];
    double *u = reinterpret_cast<double *>(nu + ((size_t)rhs * Lo2 + w) * N);    // interleaved re,im
    double *pi[NE], *pj[NE];
    double cb[NE], sb[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const unsigned ij = m.lp_ij[e * WAVE + lane];
        pi[e] = slab + (ij & 0xFFFF);
        pj[e] = slab + (ij >> 16);
        cb[e] = V.lp_cbar[e * WAVE + lane];
        sb[e] = V.lp_sbar[e * WAVE + lane];
    }
    double vin[NPL], eb[NPL], P[NPL], Q[NPL], mid[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = lane + q * WAVE;
        const int sc = (s < N) ? s : N - 1;
        vin[q] = u[2 * sc + wv];
        eb[q] = V.Ebar[sc];
    }
    const double a = V.a, b = V.b;
    // ---- first series: M^-T[w,w], conjugated coefficients (KPMPreconditioners.jl:621-648)
    kpm_series_ri<NPL, true>(P, Q, vin, slab, eb, c, order, a, b, pi, pj, cb, sb, m.ncol);
#pragma unroll
    for (int q = 0; q < NPL; ++q) xch[wv * NPL * WAVE + lane + q * WAVE] = Q[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const double Qo = xch[(wv ^ 1) * NPL * WAVE + lane + q * WAVE];
        mid[q] = (wv == 0) ? P[q] + Qo : P[q] - Qo;
    }
    __syncthreads();
    // ---- second series: M^-1[w,w] (:650-677)
    kpm_series_ri<NPL, false>(P, Q, mid, slab, eb, c, order, a, b, pi, pj, cb, sb, m.ncol);
#pragma unroll
    for (int q = 0; q < NPL; ++q) xch[wv * NPL * WAVE + lane + q * WAVE] = Q[q];
    __syncthreads();
    double dot = 0.0;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = lane + q * WAVE;
        const double Qo = xch[(wv ^ 1) * NPL * WAVE + lane + q * WAVE];
        const double res = (wv == 0) ? P[q] - Qo : P[q] + Qo;
        if (s < N) { u[2 * s + wv] = res; dot += vin[q] * res; }
    }
    if (rz_part) {
        dot = wave_sum2(dot);
        if (lane == 0) {
            const int Ltau = m.L, bid = 2 * (int)blockIdx.y + wv, nb = 2 * (int)gridDim.y;
            const double wgt = ((Ltau & 1) && w == Lo2 - 1) ? 1.0 : 2.0;
            double *slots = rz_part + (size_t)rhs * nrz;
            slots[bid] = V.active ? wgt * dot / (double)Ltau : (bid < Ltau ? rr_part[(size_t)rhs * Ltau + bid] : 0.0);
            for (int qq = nb + bid; qq < nrz; qq += nb) slots[qq] = 0.0;
        }
    }
}


// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------

// One translation unit per sites-per-lane count (ELPH_LP_NPL = 1 … 8, build.py compiles cg_fast_npl.hip eight times per lane-program
// width): the kernels of THIS count only are instantiated here, and the launchers carry the count in their names (LPFN); the dispatch
// on h->npl lives in cg_fast_shared.inc.  (One unit with all eight counts was 340 kernels and 5 min 42 s of single-thread compile.)
#define DISPATCH_NPL_F(npl, CALL)                                                                                      \
    {                                                                                                                  \
        if ((npl) != ELPH_LP_NPL) { elph_set_error("lane-program launcher for %d sites per lane called with %d", ELPH_LP_NPL, (int)(npl)); return ELPH_E_STATE; } \
        constexpr int NPL = ELPH_LP_NPL;                                                                               \
        CALL;                                                                                                          \
    }
#define LP_CAT2(a, b) a##b
#define LP_CAT(a, b) LP_CAT2(a, b)
#define LPFN(name) LP_CAT(name##_n, ELPH_LP_NPL)

static unsigned xcd_grid(const elph_handle_s *h, int nvec) { return 8u * (unsigned)((h->L + 7) / 8) * (unsigned)nvec; }

int LPFN(elph_fast_mul)(elph_handle_s *h, int which, double *yS, const double *vS, int nvec) {
    ModelDev m = elph_model_dev(h);
    const size_t shm = 2 * (size_t)(h->npl * WAVE + 2 * WAVE) * sizeof(double);
    const dim3 grid(xcd_grid(h, nvec));
    const bool ssh = (h->kind == ELPH_MODEL_SSH);
    DISPATCH_NPL_F(h->npl, {
        if (ssh) {
            if (which == 0) hipLaunchKernelGGL((k_mul_fast<NPL, 0, true>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
            else if (which == 1) hipLaunchKernelGGL((k_mul_fast<NPL, 1, true>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
            else hipLaunchKernelGGL((k_mul_fast<NPL, 2, true>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
        } else {
            if (which == 0) hipLaunchKernelGGL((k_mul_fast<NPL, 0, false>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
            else if (which == 1) hipLaunchKernelGGL((k_mul_fast<NPL, 1, false>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
            else hipLaunchKernelGGL((k_mul_fast<NPL, 2, false>), grid, dim3(WAVE), shm, h->stream, yS, vS, m);
        }
    });
    return elph_launch_check("k_mul_fast");
}

int LPFN(elph_fast_cg_ap)(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool px) {
    ModelDev m = elph_model_dev(h);
    const size_t shm = 2 * (size_t)(h->npl * WAVE + 2 * WAVE) * sizeof(double);
    const bool ssh = (h->kind == ELPH_MODEL_SSH);
    const int T = (B.npap == (int)h->L) ? 1 : (int)((h->L + B.npap - 1) / B.npap);
    if (T > 1) {
        const dim3 grid((unsigned)(nrhs * B.npap));
        const bool templ = (h->L % T == 0) && (T == 20 || T == 16 || T == 10 || T == 8 || T == 5 || T == 4 || T == 2);
        if (px && (!templ || (ssh && ELPH_LP_MC != 4))) { elph_set_error("k_cg_ap_chunk: the p/x-fused iteration was planned for a shape it does not exist in"); return ELPH_E_STATE; }
        if (!templ) {
            DISPATCH_NPL_F(h->npl, {
                if (ssh) hipLaunchKernelGGL((k_cg_ap_chunk_rt<NPL, true>), grid, dim3(WAVE), shm, h->stream, B, m, parity, T);
                else hipLaunchKernelGGL((k_cg_ap_chunk_rt<NPL, false>), grid, dim3(WAVE), shm, h->stream, B, m, parity, T);
            });
            return elph_launch_check("k_cg_ap_chunk_rt");
        }
        // (blocks in the XCD-aware order of chunk_block_map; solo_chain: the model shows ONE chain to the kernels)
        const int po = parity | ((h->solo_chain < 0) ? 2 : 0);
#if ELPH_LP_MC == 4      // (the p/x-fused form is planned for four-colour lane programs only: no six-colour instantiations)
#define CHUNK_PX_BRANCH(TT) else if (px) { if constexpr (NPL >= 5) hipLaunchKernelGGL((k_cg_ap_chunk_px2<NPL, TT>), grid, dim3(WAVE), shm, h->stream, B, m, po); \
                                          else hipLaunchKernelGGL((k_cg_ap_chunk_px<NPL, TT>), grid, dim3(WAVE), shm, h->stream, B, m, po); }
#define CHUNK_PX_SSH_BRANCH(TT) if (ssh && px) hipLaunchKernelGGL((k_cg_ap_chunk_px_ssh<NPL, TT>), grid, dim3(WAVE), shm, h->stream, B, m, po); else
#else
#define CHUNK_PX_BRANCH(TT) else if (px) { elph_set_error("p/x-fused iteration: four-colour lane programs only"); return ELPH_E_STATE; }
#define CHUNK_PX_SSH_BRANCH(TT)
#endif
#define LAUNCH_CHUNK(TT)                                                                                           \
        DISPATCH_NPL_F(h->npl, {                                                                                       \
            CHUNK_PX_SSH_BRANCH(TT)                                                                                    \
            if (ssh) hipLaunchKernelGGL((k_cg_ap_chunk<NPL, TT, true>), grid, dim3(WAVE), shm, h->stream, B, m, po);  \
            CHUNK_PX_BRANCH(TT)                                                                                        \
            else hipLaunchKernelGGL((k_cg_ap_chunk<NPL, TT, false>), grid, dim3(WAVE), shm, h->stream, B, m, po);     \
        })
        if (T == 20) { LAUNCH_CHUNK(20); }
        else if (T == 16) { LAUNCH_CHUNK(16); }
        else if (T == 10) { LAUNCH_CHUNK(10); }
        else if (T == 8) { LAUNCH_CHUNK(8); }
        else if (T == 5) { LAUNCH_CHUNK(5); }
        else if (T == 4) { LAUNCH_CHUNK(4); }
        else if (T == 2) { LAUNCH_CHUNK(2); }
        else { elph_set_error("k_cg_ap_chunk: no instantiation for %d slices per wave", T); return ELPH_E_UNSUPPORTED; }
#undef LAUNCH_CHUNK
#undef CHUNK_PX_BRANCH
#undef CHUNK_PX_SSH_BRANCH
        return elph_launch_check("k_cg_ap_chunk");
    }
    if (px) { elph_set_error("k_cg_ap_fast: the p/x-fused iteration exists in the chunked kernel only"); return ELPH_E_STATE; }
    const dim3 grid(xcd_grid(h, nrhs));
    DISPATCH_NPL_F(h->npl, {
        if (ssh) hipLaunchKernelGGL((k_cg_ap_fast<NPL, true>), grid, dim3(WAVE), shm, h->stream, B, m, parity);
        else hipLaunchKernelGGL((k_cg_ap_fast<NPL, false>), grid, dim3(WAVE), shm, h->stream, B, m, parity);
    });
    return elph_launch_check("k_cg_ap_fast");
}

int LPFN(elph_fast_cg_xr)(elph_handle_s *h, const CgBufs &B, int nrhs, int parity) {
    const dim3 grid(xcd_grid(h, nrhs));
    DISPATCH_NPL_F(h->npl, {
        hipLaunchKernelGGL((k_cg_xr_fast<NPL>), grid, dim3(WAVE), 0, h->stream, B, (int)h->N, (int)h->L, parity);
    });
    return elph_launch_check("k_cg_xr_fast");
}


// the Chebyshev recursion through the LDS slab (the Re / Im two-wave form): what elph_fast_kpm_cheb falls to when no
// register-exchange layout serves the lattice
int LPFN(elph_fast_kpm_cheb_lds)(elph_handle_s *h, int nrhs, const CgState *st, double *rz_part, int nrz, const double *rr_part) {
    KpmDev K = elph_kpm_dev(h);
    ModelDev m = elph_model_dev(h);
    const int Lo2 = (int)((h->L + 1) / 2);
    const size_t shm = (size_t)(2 * (h->npl * WAVE + 2 * WAVE) + 2 * h->npl * WAVE) * sizeof(double);
    DISPATCH_NPL_F(h->npl, {
        hipLaunchKernelGGL((k_kpm_cheb_ri<NPL>), dim3((unsigned)nrhs, (unsigned)Lo2), dim3(2 * WAVE), shm, h->stream, h->work.nu, K, m,
                           Lo2, st, rz_part, nrz, rr_part);
    });
    return elph_launch_check("k_kpm_cheb_ri");
}

#undef DISPATCH_NPL_F
#undef LPFN
#undef LP_CAT
#undef LP_CAT2

}  // namespace LPNS
