// cg_fast_shared.inc — what the lane-program family needs once per lane-program width ELPH_LP_MC, whatever the sites-per-lane count:
// the register-exchange Chebyshev kernels (4 colours only), the slices-per-wave rules, and the dispatch of every launcher on h->npl
// into the per-count translation units (cg_fast_npl.hip x 8, cg_fast_impl.inc).  Included by cg_fast.hip (4) and cg_fast6.hip (6).

namespace LPNS {

#if ELPH_LP_MC == 4   // register-exchange kernel of the 4-colour square lattice: one instantiation is enough
// ------------------------------------------------------------------------------------------
// KPM Chebyshev recursion for the even-L square lattice (L = 8, 16): checkerboard exchange in REGISTERS.
// The greedy colouring of the reference yields [x-even | x-odd | y-even | y-odd] (SURVEY.md Appendix A; the
// host verifies the bond table against exactly that pattern before enabling this kernel).  Each lane owns a
// P x P patch of sites (P = L/8; lanes form an 8 x 8 grid of patches):
//   * x-even / y-even bonds of a 2x2 patch connect two of the lane's own registers  -> no data movement,
//   * x-odd / y-odd bonds connect to the neighbouring patch                          -> one wave shuffle per value,
// so a checkerboard apply is 2 shuffle rounds + FMAs, with no LDS slab, no LDS round trip per colour.
// Same re/im split as k_kpm_cheb_ri (wave 0 = Re, wave 1 = Im, one LDS exchange per series).
// ------------------------------------------------------------------------------------------

// (SqLane, sq_cb_apply, sq16_cb_apply, kpm_series_sq: kpm_sq_dev.h — shared with the resident preconditioned solver, pcg_wg.hip)
using kpmsq::SqLane;
using kpmsq::kpm_series_sq;

// HC: the honeycomb lattice of 12 x 12 cells in the quad layout of kpm_sq_dev.h (six sites per lane, 48 lanes; uniform hopping) — the
// same kernel around another checkerboard (P is ignored)
// GRID: any other even-L square lattice up to 16 x 16 in the GRID layout of cg_fast_common.h (2 x 2 patches on a G x G grid of lanes, crossings
// by ds_bpermute; uniform hopping; P = 2 for the register count, ROWS and HC off)
// HGN > 0: any other honeycomb lattice in the HGRID layout (HGN = 2, 4 or 8 registers per lane: 1, 2 or 4 cells; uniform hopping)
template <int P, bool UNI, bool ROWS, bool HC, bool GRID = false, int HGN = 0>
__device__ __forceinline__ void kpm_cheb_sq_body(double2 *__restrict__ nu, KpmDev K, const double *__restrict__ sqc,
                                                 const double *__restrict__ sqs, int N, int Lo2,
                                                 const CgState *state, double *__restrict__ rz_part, int nrz, int Ltau,
                                                 const double *__restrict__ rr_part, int fold_nct) {
    constexpr int NS = (HGN > 0) ? HGN : (HC ? 6 : P * P), LS = 8 * P;
    static_assert(HGN == 0 || (UNI && !ROWS && !HC && !GRID), "honeycomb grid recursion: uniform hopping");
    static_assert(!HC || (UNI && !ROWS), "honeycomb recursion: uniform hopping");
    static_assert(!GRID || (P == 2 && UNI && !ROWS && !HC), "grid recursion: 2 x 2 patches, uniform hopping");
    int GG = 1;
    if (GRID) { while (4 * GG * GG < N) ++GG; }         // G = L / 2
    __shared__ double xch[2][NS * WAVE];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
    // x = right-hand side, y = frequency in longest-first order: ALL long recursions are dispatched first; a block takes the
    // frequencies y, y + gridDim.y, ... of that order (a long recursion and ever shorter ones: the tables stay in registers)
    const int rhs = blockIdx.x;
    if (state && ld_state(state + 2 * rhs).done) return;
    const KpmChainView V = kpm_chain_view(K, rhs, N);
    if (K.sq_stride && K.nchains > 1) { const size_t o = (size_t)(rhs % K.nchains) * (size_t)K.sq_stride; sqc += o; sqs += o; }   // SSH chains
    // A series of order 1 is its leading coefficient: z_w = c0 (conj(c0) r_w) — no checkerboard apply, no tables.  That is most
    // frequencies (config C: 47 of 80; order_w ~ 1/phi_w), so those blocks take this exit before any set-up: each thread does the
    // arithmetic of the general path (products first, then the sums — the same roundings) on the complex values of its sites.
    // (what this block has to do comes from ONE packed descriptor — frequency, order, coefficient offset, leading coefficient:
    //  these blocks are latency-bound, four dependent scalar loads in front of the first data load were most of their life)
    const KpmDesc D0 = V.desc[blockIdx.y < (unsigned)Lo2 ? blockIdx.y : 0];
    if (V.active && D0.order == 1 && fold_nct > 0) {
        // FOLD: the forward transform has written this frequency already scaled by |c0|^2 and added its share of r.z (slots
        // [2 Lo2, 2 Lo2 + fold_nct)): this block only keeps the slot bookkeeping — its own slot is zero, the slots beyond are cleared
        if (rz_part && lane == 0) {
            const int G = 2 * Lo2, bid = 2 * (int)blockIdx.y + wv;
            double *slots = rz_part + (size_t)rhs * nrz;
            slots[bid] = 0.0;
            const int nb = 2 * (int)gridDim.y;
            for (int qq = nb + bid; qq < nrz; qq += nb) if (qq < G || qq >= G + fold_nct) slots[qq] = 0.0;
        }
        return;
    }
    if (gridDim.y == (unsigned)Lo2 && V.active && D0.order == 1) {
        const int w = D0.w;
        const double2 c0 = make_double2(D0.c0x, D0.c0y);
        double2 *uc = nu + ((size_t)rhs * Lo2 + w) * N;
        double dot = 0.0;
        for (int i = threadIdx.x; i < N; i += 2 * WAVE) {
            const double2 v = uc[i];
            const double mr = __dadd_rn(__dmul_rn(c0.x, v.x), __dmul_rn(c0.y, v.y)), mi = __dsub_rn(__dmul_rn(c0.x, v.y), __dmul_rn(c0.y, v.x));
            const double rr_ = __dsub_rn(__dmul_rn(c0.x, mr), __dmul_rn(c0.y, mi)), ri = __dadd_rn(__dmul_rn(c0.x, mi), __dmul_rn(c0.y, mr));
            uc[i] = make_double2(rr_, ri);
            dot += v.x * rr_ + v.y * ri;
        }
        if (rz_part) {
            dot = wave_sum2(dot);
            if (lane == 0) {
                const double wgt = ((Ltau & 1) && w == Lo2 - 1) ? 1.0 : 2.0;
                const int G = 2 * Lo2, bid = 2 * (int)blockIdx.y + wv;
                double *slots = rz_part + (size_t)rhs * nrz;
                slots[bid] = wgt * dot / (double)Ltau;
                const int nb = 2 * (int)gridDim.y;          // (with the fold the grid holds only the frequencies some chain still recurses on)
                for (int qq = nb + bid; qq < nrz; qq += nb) if (qq < G || qq >= G + fold_nct) slots[qq] = 0.0;
            }
        }
        return;
    }
    const int pa = lane & 7, pb = lane >> 3;
    int HL = 1;
    if (HGN > 0) { while (2 * HL * HL < N) ++HL; }      // cells per side
    constexpr int HNP = (HGN > 0) ? HGN : 2;            // (a valid instantiation of the helpers when the form is off)
    const bool act = (HGN > 0) ? lane < (HL / HgDim<HNP>::PX) * (HL / HgDim<HNP>::PY) : GRID ? lane < GG * GG : (!HC || lane < 48);      // (honeycomb: 48 lanes hold the lattice, the rest shadow lanes 0..15 and store nothing; grid: G x G lanes)
    kpmsq::HcLane TH;
    TH.up = (lane < 48) ? (lane + 4) % 48 : lane; TH.dn = (lane < 48) ? (lane + 44) % 48 : lane; TH.th = 0.0;
    SqLane<P> T;
    T.xp = ((pa + 1) & 7) + 8 * pb; T.xm = ((pa + 7) & 7) + 8 * pb;
    T.yp = pa + 8 * ((pb + 1) & 7); T.ym = pa + 8 * ((pb + 7) & 7);
    T.xe = (pa ^ 1) + 8 * pb; T.ye = pa + 8 * (pb ^ 1);
    if (P == 1) {   // odd colours pair (odd, odd+1): an odd coordinate looks up, an even one looks down
        if (!(pa & 1)) T.xp = T.xm;
        if (!(pb & 1)) T.yp = T.ym;
    }
    static_assert(!ROWS || P == 2, "row layout: the 16 x 16 lattice");
    if (ROWS) { T.yp = sq_patch_ycross(lane); T.ym = T.yp; }
    int site[NS];
    double eb[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int dx = q % P, dy = q / P;
        site[q] = (HGN > 0) ? hgrid_site<HNP>(lane, q, HL) : GRID ? grid_site(lane, q, GG) : HC ? kpmsq::hc12q_site(lane, q) : (ROWS ? sq_patch_site(lane, q) : (pa * P + dx) + LS * (pb * P + dy));
        eb[q] = V.Ebar[site[q]];
        if (!UNI) {
#pragma unroll
            for (int col = 0; col < 4; ++col) {
                T.c[col][q] = sqc[(size_t)col * N + site[q]];
                T.s[col][q] = sqs[(size_t)col * N + site[q]];
            }
        }
    }
    if (UNI) { T.cu = sqc[0]; T.su = sqs[0]; }
    double a = V.a;
    const double b = V.b;
    if (ROWS && UNI) {       // factored colours (sq16_cb_apply): th in T.su, c^4 into the scale of A'
        const double cc = T.cu * T.cu;
        T.su = T.su / T.cu; T.cu = cc * cc;
        a *= T.cu;
    }
    if (HC) { TH.th = T.su / T.cu; a *= T.cu * T.cu * T.cu; }      // three colours: c^3
    GridCtx TG;
    if constexpr (GRID) { TG = grid_ctx(lane, GG, T.cu, T.su); a *= TG.k4; }
    HgCtx THG;
    if constexpr (HGN > 0) { THG = hgrid_ctx<HNP>(lane, HL, T.cu, T.su); a *= THG.k3; }
    // (measured: the kernel ends with the longest recursion — order ~60 at frequency 0 against 1-3 for most — and that chain is
    //  latency-bound on its own; raising its wave priority changes nothing, for one right-hand side or for 128)
    for (int wy = blockIdx.y; wy < Lo2; wy += (fold_nct > 0 ? Lo2 : (int)gridDim.y)) {      // (the fold: one frequency per block, the rest is the transform's)
        const KpmDesc D = (wy == (int)blockIdx.y) ? D0 : V.desc[wy];
        const int w = D.w;
        const int order = D.order;
        const double2 *c = K.coeff + D.coff;
        double *u = reinterpret_cast<double *>(nu + ((size_t)rhs * Lo2 + w) * N);
        double vin[NS], Pa[NS], Qa[NS], mid[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) vin[q] = u[2 * site[q] + wv];
        if constexpr (HGN > 0) kpmsq::kpm_series_hgrid<NS, true>(Pa, Qa, vin, eb, c, order, a, b, THG);
        else if constexpr (GRID) kpmsq::kpm_series_grid<true>(Pa, Qa, vin, eb, c, order, a, b, TG);
        else if constexpr (HC) kpmsq::kpm_series_hc<true>(Pa, Qa, vin, eb, c, order, a, b, TH);
        else kpm_series_sq<P, true, UNI, ROWS>(Pa, Qa, vin, eb, c, order, a, b, T);
#pragma unroll
        for (int q = 0; q < NS; ++q) xch[wv][q * WAVE + lane] = Qa[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const double Qo = xch[wv ^ 1][q * WAVE + lane];
            mid[q] = (wv == 0) ? Pa[q] + Qo : Pa[q] - Qo;
        }
        __syncthreads();
        if constexpr (HGN > 0) kpmsq::kpm_series_hgrid<NS, false>(Pa, Qa, mid, eb, c, order, a, b, THG);
        else if constexpr (GRID) kpmsq::kpm_series_grid<false>(Pa, Qa, mid, eb, c, order, a, b, TG);
        else if constexpr (HC) kpmsq::kpm_series_hc<false>(Pa, Qa, mid, eb, c, order, a, b, TH);
        else kpm_series_sq<P, false, UNI, ROWS>(Pa, Qa, mid, eb, c, order, a, b, T);
#pragma unroll
        for (int q = 0; q < NS; ++q) xch[wv][q * WAVE + lane] = Qa[q];
        __syncthreads();
        double dot = 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const double Qo = xch[wv ^ 1][q * WAVE + lane];
            const double res = (wv == 0) ? Pa[q] - Qo : Pa[q] + Qo;
            if (act) { u[2 * site[q] + wv] = res; dot += vin[q] * res; }
        }
        __syncthreads();                  // (xch is rewritten by the next frequency)
        // r.(P^-1 r) in frequency space (Parseval for the twisted transform: a.b = (1/L) sum_k conj(a_k) b_k; this wave holds the
        // real or the imaginary parts of one frequency, whose mirror L-1-k contributes the same): the inverse transform then
        // needs no second pass over r for the fused r.z of the CG
        if (rz_part) {
            dot = wave_sum2(dot);
            if (lane == 0) {
                const double wgt = ((Ltau & 1) && w == Lo2 - 1) ? 1.0 : 2.0;
                const int G = 2 * Lo2, bid = 2 * wy + wv;
                double *slots = rz_part + (size_t)rhs * nrz;
                // identity preconditioner (this chain's expansion is inactive): r.z IS r.r — hand over the r.r partial sums of the
                // residual update slot by slot, so that the iteration is bit-identical to the un-preconditioned one
                slots[bid] = V.active ? wgt * dot / (double)Ltau : (bid < Ltau ? rr_part[(size_t)rhs * Ltau + bid] : 0.0);
                const int nb = (gridDim.y == (unsigned)Lo2 || fold_nct > 0) ? 2 * (int)gridDim.y : G;
                for (int qq = nb + bid; qq < nrz; qq += nb) if (qq < G || qq >= G + fold_nct) slots[qq] = 0.0;
            }
        }
    }
}

#endif

// ---- the per-count launchers (cg_fast_impl.inc, one translation unit each) and the dispatch on h->npl -----------------------------
#define LP_DECL(K)                                                                                             \
    int elph_fast_mul_n##K(elph_handle_s *h, int which, double *yS, const double *vS, int nvec);               \
    int elph_fast_cg_ap_n##K(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool px);                \
    int elph_fast_cg_xr_n##K(elph_handle_s *h, const CgBufs &B, int nrhs, int parity);                         \
    int elph_fast_kpm_cheb_lds_n##K(elph_handle_s *h, int nrhs, const CgState *st, double *rz_part, int nrz, const double *rr_part);
LP_DECL(1) LP_DECL(2) LP_DECL(3) LP_DECL(4) LP_DECL(5) LP_DECL(6) LP_DECL(7) LP_DECL(8)
#undef LP_DECL
#define LP_SWITCH(fn, ...)                                  \
    switch (h->npl) {                                       \
        case 1: return fn##_n1(__VA_ARGS__);                \
        case 2: return fn##_n2(__VA_ARGS__);                \
        case 3: return fn##_n3(__VA_ARGS__);                \
        case 4: return fn##_n4(__VA_ARGS__);                \
        case 5: return fn##_n5(__VA_ARGS__);                \
        case 6: return fn##_n6(__VA_ARGS__);                \
        case 7: return fn##_n7(__VA_ARGS__);                \
        case 8: return fn##_n8(__VA_ARGS__);                \
        default: elph_set_error("lane program: %d sites per lane (1 ... 8 exist)", (int)h->npl); return ELPH_E_STATE; \
    }
int elph_fast_mul(elph_handle_s *h, int which, double *yS, const double *vS, int nvec) { LP_SWITCH(elph_fast_mul, h, which, yS, vS, nvec) }
int elph_fast_cg_ap(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool px) { LP_SWITCH(elph_fast_cg_ap, h, B, nrhs, parity, px) }
int elph_fast_cg_xr(elph_handle_s *h, const CgBufs &B, int nrhs, int parity) { LP_SWITCH(elph_fast_cg_xr, h, B, nrhs, parity) }
static int kpm_cheb_lds_npl(elph_handle_s *h, int nrhs, const CgState *st, double *rz_part, int nrz, const double *rr_part) { LP_SWITCH(elph_fast_kpm_cheb_lds, h, nrhs, st, rz_part, nrz, rr_part) }
#undef LP_SWITCH

// slices per wave for the batched kernel: the largest T in {20,16,10,8,5,4,2} dividing L that still leaves >= 1024 waves.  (A RAGGED cut
// of the time axis that runs a batch in one round of the chip measured slower — the rolled kernel k_cg_ap_chunk_rt is ~15 % slower per
// slice than the unrolled one, profiles/r03/time_kpm_ragged_chunks.log — and was removed; the run-time kernel serves ELPH_CHUNK_T.)
static int choose_T_template(const elph_handle_s *h, int nrhs) {
    if (!h->fast || h->force_T == 1) return 1;
    // slices per wave must divide Ltau; 10 and 5 serve the time axes that are multiples of 10 but not of 8 (Ltau = 30, 50, 70, 90 …),
    // which would otherwise fall to T = 2 and read every slice of r and p twice
    const int cand[7] = {20, 16, 10, 8, 5, 4, 2};
    for (int T : cand) {
        if (h->force_T > 1 && T != h->force_T) continue;
        // 16 slices per wave halve the tau-halo re-reads once more, but only pay while the grid stays near one wave per
        // SIMD (measured at config C: 128 rhs = 1280 waves: 52.8 -> 48.9 us; 64 rhs (640 waves) and 256 rhs (2560) lose 3-5 %).
        // 20 slices per wave (time axes that are multiples of 20) go one step further wherever they still leave one wave per
        // SIMD: 128 rhs = exactly 1024 waves 48.9 -> 46.8 us, 256 rhs = 2048 waves 99.2 -> 92.2 us; below 1024 waves they lose
        // (64 rhs: 27.5 -> 33.6 us), which the >= 1024 test below excludes.  32 slices per wave are 4x slower (the unrolled
        // slice loop no longer fits the instruction cache).
        // (round 3, 288 right-hand sides of config C: 20 slices per wave are 2304 waves for the chip's 2048 slots at two per SIMD — a
        //  second, nearly empty round — and lose to 16 slices per wave: CG iteration 165.8 vs 153.7 us, preconditioned 326.8 vs 311.4,
        //  profiles/r03/time_chunkT_288.log; so 20 is skipped while its grid overshoots one round by less than a quarter, and 16
        //  keeps its exclusion only where it was measured to lose, from 2560 waves of its own)
        const int64_t waves = (int64_t)nrhs * (h->L / T);
        if (T == 20 && h->force_T != 20 && h->L % 16 == 0 && waves > 2048 && waves <= 2560) continue;
        if (T == 16 && h->force_T != 16 && waves >= 2048 && !((int64_t)nrhs * (h->L / 20) > 2048 && (int64_t)nrhs * (h->L / 20) <= 2560 && h->L % 20 == 0)) continue;
        if (h->L % T) continue;
        if (h->force_T > 1 || (int64_t)nrhs * (h->L / T) >= 1024) return T;
    }
    return 1;
}

int elph_choose_T(const elph_handle_s *h, int nrhs);
// Slices per wave of the p/x-fused kernel (k_cg_ap_chunk_px, three waves per SIMD = 3072 wave slots): the largest template length
// whose grid still fills most of one round (>= 2560 waves) — measured at config C (tools/time_px_chunk_T.py, profiles/r05/
// px_chunk_T.log): 288 right-hand sides 16 slices per wave (2880 waves: iteration 289 us; 20: 293, 8: 297), 128 right-hand sides 8 (2560
// waves: 131 us; 20 = 1024 waves: 142).  nrhs = the right-hand sides IN FLIGHT (both halves of a two-stream batch).
int elph_choose_T_px(const elph_handle_s *h, int nrhs, bool two_streams) {
    if (!h->fast || h->force_T == 1) return 1;
    const int cand[7] = {20, 16, 10, 8, 5, 4, 2};
    // (forced lengths; bond phonons: the fused kernel keeps two sets of hopping tables in registers and stays at two waves per SIMD — the
    //  unfused kernel's rule holds: config E, 128 right-hand sides 142 us with 20 slices per wave, 148 with 8; 256: 269 either way)
    if (h->force_T > 1 || h->kind == ELPH_MODEL_SSH) return LPNS::elph_choose_T(h, nrhs);
    if (h->npl >= 5) {
        // five and more sites per lane (k_cg_ap_chunk_px2, two waves per SIMD; config D): the unfused kernel's rule, capped at 10 slices per wave — the
        // kernel alone is fastest at 20, the ITERATION is not (D, two streams: 192 right-hand sides 174 -> 161 us, 256: 229 -> 213, 288: 253 -> 239;
        // one stream 208 -> 195, 265 -> 254, 283 -> 273; profiles/r05/px_fused_five_sites_per_lane.log)
        const int T0 = LPNS::elph_choose_T(h, nrhs);
        if (T0 <= 10) return T0;
        const int capped[5] = {10, 8, 5, 4, 2};
        for (int T : capped) if (h->L % T == 0) return T;
        return T0;
    }
    // two half-batches on two streams (nrhs: both halves counted): the other half's kernels fill what a shorter grid leaves idle, so
    // the longest chunks whose grid is 1536 ... 2048 waves win — 256 right-hand sides 20 slices per wave 230 us against 243 with 16, 192:
    // 182 against 185 with 10; 288 (2304 waves at 20) stays with the one-stream rule: 16 slices per wave 259 us against 262
    if (two_streams)
        for (int T : cand) {
            if (h->L % T) continue;
            const int64_t w = (int64_t)nrhs * (h->L / T);
            if (w >= 1536 && w <= 2048) return T;
        }
    for (int T : cand) {
        if (h->L % T) continue;
        if ((int64_t)nrhs * (h->L / T) >= 2560) return T;
    }
    return LPNS::elph_choose_T(h, nrhs);
}

int elph_choose_T(const elph_handle_s *h, int nrhs) {
    if (h->fast && h->force_T > 1 && h->force_T < h->L) {      // ELPH_CHUNK_T: any length (not a template size: the run-time kernel)
        const int F = h->force_T;
        const bool templ = (h->L % F == 0) && (F == 20 || F == 16 || F == 10 || F == 8 || F == 5 || F == 4 || F == 2);
        if (!templ) {
            int64_t T = F;
            while (T < h->L && h->L - ((h->L + T - 1) / T - 1) * T < 2) ++T;
            return (int)T;
        }
    }
    return choose_T_template(h, nrhs);
}


#if ELPH_LP_MC == 4
template <int P, bool UNI, bool ROWS = false, bool HC = false, bool GRID = false, int HGN = 0>
__global__ void __launch_bounds__(2 * WAVE) k_kpm_cheb_sq(double2 *__restrict__ nu, KpmDev K, const double *__restrict__ sqc,
                                                          const double *__restrict__ sqs, int N, int Lo2,
                                                          const CgState *state, double *__restrict__ rz_part, int nrz, int Ltau,
                                                          const double *__restrict__ rr_part, int fold_nct) {
    kpm_cheb_sq_body<P, UNI, ROWS, HC, GRID, HGN>(nu, K, sqc, sqs, N, Lo2, state, rz_part, nrz, Ltau, rr_part, fold_nct);
}
// the same for FOUR waves per SIMD (128 registers): the uniform-hopping recursion of the 16 x 16 lattice needs 132 as the compiler
// allots them — one wave per SIMD less for four registers; a batch is thousands of latency-bound chains, every wave in flight counts
template <int P, bool UNI, bool ROWS = false, bool HC = false>
__global__ void __launch_bounds__(2 * WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_kpm_cheb_sq_w4(double2 *__restrict__ nu, KpmDev K, const double *__restrict__ sqc, const double *__restrict__ sqs, int N, int Lo2,
                 const CgState *state, double *__restrict__ rz_part, int nrz, int Ltau, const double *__restrict__ rr_part, int fold_nct) {
    kpm_cheb_sq_body<P, UNI, ROWS, HC>(nu, K, sqc, sqs, N, Lo2, state, rz_part, nrz, Ltau, rr_part, fold_nct);
}

#endif

// rz_part != nullptr: the caller wants the r.z partial sums of the CG from this kernel (frequency space; every form below delivers them,
// the LDS recursion where the caller's slots hold the 2 Lo2 partials of a launch: elph_plan_cg plans rz_freq by that rule).  reg: the
// register-exchange recursion where this lattice has one (elph_reg_cheb_form), else the Re / Im recursion through the LDS slab
int elph_fast_kpm_cheb(elph_handle_s *h, int nrhs, const CgState *st, bool reg, double *rz_part, int nrz, const double *rr_part, int fold_nct) {
    KpmDev K = elph_kpm_dev(h);
    const int Lo2 = (int)((h->L + 1) / 2);
#if ELPH_LP_MC == 4
    // with the fold only the frequencies that some chain still recurses on get a block (the schedule is longest first)
    const unsigned gy = (unsigned)(fold_nct > 0 ? h->kpm.tab.recurse : Lo2);
    int hgn = 0;
    const int form = reg ? elph_reg_cheb_form(h, &hgn) : REG_NONE;
    if (form == REG_SQ) {
        // one frequency per block (the kernel loops over y, y + gridDim.y, ...: 2, 4 or 8 frequencies per block were measured — no
        // faster at 1 right-hand side or at 128: block dispatch is not what the kernel waits for)
#define SQ_LAUNCH(PV, UV, ...) hipLaunchKernelGGL((k_kpm_cheb_sq<PV, UV, ##__VA_ARGS__>), dim3((unsigned)nrhs, gy), dim3(2 * WAVE), 0, h->stream, \
                                             h->work.nu, K, h->kpm.d_sq_cbar, h->kpm.d_sq_sbar, (int)h->N, Lo2, st, rz_part, nrz, (int)h->L, rr_part, fold_nct)
        const int P = h->shape.dpp();
        if (P == 2 && h->kpm.sq_chain_uniform && nrhs >= 16) {
            hipLaunchKernelGGL((k_kpm_cheb_sq_w4<2, true, true>), dim3((unsigned)nrhs, gy), dim3(2 * WAVE), 0, h->stream,
                               h->work.nu, K, h->kpm.d_sq_cbar, h->kpm.d_sq_sbar, (int)h->N, Lo2, st, rz_part, nrz, (int)h->L, rr_part, fold_nct);
        } else if (P == 2) { if (h->kpm.sq_chain_uniform) SQ_LAUNCH(2, true, true); else SQ_LAUNCH(2, false, true); }
        else        { if (h->kpm.sq_chain_uniform) SQ_LAUNCH(1, true); else SQ_LAUNCH(1, false); }
#undef SQ_LAUNCH
        return elph_launch_check("k_kpm_cheb_sq");
    }
    if (form == REG_SQ_GRID) {
        hipLaunchKernelGGL((k_kpm_cheb_sq<2, true, false, false, true>), dim3((unsigned)nrhs, gy), dim3(2 * WAVE), 0, h->stream,
                           h->work.nu, K, h->kpm.d_sq_cbar, h->kpm.d_sq_sbar, (int)h->N, Lo2, st, rz_part, nrz, (int)h->L, rr_part, fold_nct);
        return elph_launch_check("k_kpm_cheb_sq(grid)");
    }
    if (form == REG_HC_GRID) {
#define HG_LAUNCH(NV) hipLaunchKernelGGL((k_kpm_cheb_sq<2, true, false, false, false, NV>), dim3((unsigned)nrhs, gy), dim3(2 * WAVE), 0, h->stream, \
                                         h->work.nu, K, h->kpm.d_cbar, h->kpm.d_sbar, (int)h->N, Lo2, st, rz_part, nrz, (int)h->L, rr_part, fold_nct)
        if (hgn == 2) HG_LAUNCH(2); else if (hgn == 4) HG_LAUNCH(4); else HG_LAUNCH(8);
#undef HG_LAUNCH
        return elph_launch_check("k_kpm_cheb_sq(honeycomb grid)");
    }
    if (form == REG_HC12) {
        hipLaunchKernelGGL((k_kpm_cheb_sq<2, true, false, true>), dim3((unsigned)nrhs, gy), dim3(2 * WAVE), 0, h->stream,
                           h->work.nu, K, h->kpm.d_cbar, h->kpm.d_sbar, (int)h->N, Lo2, st, rz_part, nrz, (int)h->L, rr_part, fold_nct);
        return elph_launch_check("k_kpm_cheb_sq(honeycomb)");
    }
#else
    (void)reg;
#endif
    // the Re / Im recursion through the LDS slab delivers r.z too (round 6), where the caller's slots hold the 2 Lo2 partials of a launch
    const bool lds_rz = rz_part != nullptr && 2 * Lo2 <= nrz;
    return kpm_cheb_lds_npl(h, nrhs, st, lds_rz ? rz_part : nullptr, nrz, rr_part);
}

}  // namespace LPNS
