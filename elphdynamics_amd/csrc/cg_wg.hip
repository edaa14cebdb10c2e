// cg_wg.hip — workgroup-resident conjugate gradient: the whole un-preconditioned solve of M^T M x = b
// (IterativeSolvers.jl:239-314) in ONE launch, Krylov vectors in registers, for lattices with a 4-colour lane program.
//
// Why: the two-kernel iteration (cg_fast_impl.inc) streams r, p, x, z through HBM/L2 every iteration — HBM-bound in a large
// batch (0.6-0.7 of the 8 TB/s peak), launch-bound for the reference's real call shape (1-2 right-hand sides: 8 us per
// iteration for 0.6 us of work).  Here a right-hand side belongs to a TEAM of G workgroups of W wavefronts; a wavefront owns
// T consecutive tau-slices for the whole solve and keeps p (own slices + one halo slice each side) and exp(-dtau V) in registers,
// x and r in its LDS (or registers, by shape).  Nothing of the Krylov vectors goes back to memory between iterations: an
// iteration costs two checkerboard-sweep passes (in registers — the DPP forms of cg_wg_dev.h — or in the wave's private LDS
// slabs) plus ONE MEETING of the team: every workgroup publishes FOUR sums — p.z, r.z, z.z and the r.r of the current residual —
// and the boundary slices of z; alpha = r.r / p.z, r'.r' = r.r - 2 alpha r.z + alpha^2 z.z gives beta and the stop test without a
// second reduction, and the neighbouring workgroup's boundary slice of r' is its r minus alpha times its z (see the loop).
// A meeting is hierarchical: wave partials -> LDS -> s_barrier (inside the workgroup), then — only if the team has more
// than one workgroup — one 64-byte record per workgroup through L2: eight 8-byte {tag = iteration, half of an f64} granules
// written by ONE sc1 store each and polled with sc1 loads until all tags carry the iteration number
// (cdna_hip_programming.md, Guideline 16, form R2: the data is the flag; no fence).  The boundary slices of z travel as granules
// of the same kind.  Every wave of a team reduces the same records in the same order, so alpha, beta and the stop decision are
// bit-identical across the team and from run to run.  (A sharded solve, SHARD, meets on two levels: the workgroups of a rank, then
// the ranks through their mailboxes.)
//
// Behind the meeting (un-sharded solves, FUSED in the kernel): everything that decides — alpha, r'.r', the stop test, beta — follows from
// the four sums, so it is made FIRST; then ONE pass over the own slices makes r' = r - alpha z (stored to LDS for the neighbouring waves),
// x += alpha p and p = r' + beta p from the r' it still holds in a register; then the barrier that releases the neighbours' r', and the
// two halo slices of p.  The square-lattice DPP forms add their four sums per batch of reverse sweeps.  Every fma keeps its operands and
// every sum its order: the bits of a solve are those of the order this replaces (update, barrier, stop test, p-update from LDS), which
// the sharded solves and the one-slice shapes keep (one slice per wave: measured 1.3 % slower with the pass than without).
// (Built, measured and left out: the forward sweeps of the slabs 1 .. T — they read the wave's own slices of p only — BEFORE that barrier,
// the loop rotated by them.  4-slice shape 1.0 % over the old order against 2.2 % without the rotation, 2 slices 0.3 against 2.4 %, one
// slice 4 % slower: profiles/wg_fused_tail/.)
//
// Placement: team members are blocks with equal blockIdx % 8 (they share an XCD and its L2 under the observed round-robin
// placement — speed only, never correctness).  The grid may hold more teams than the chip can keep resident: blocks are
// dispatched in index order, a team's members have neighbouring indices, so at most the eight teams at the dispatch
// frontier wait (spinning) for members that start when another team has finished its solve.  Every spin is bounded by a
// wall-clock limit; a wave that gives up raises `abort`, all others leave within 64 polls, and the host falls back to the
// two-kernel iteration.

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "cg_fast_common.h"

#include "cg_wg_dev.h"
#include "pgrid_dev.h"

namespace wg {

#ifdef ELPH_WG_ARRIVE
__device__ unsigned long long g_wg_arrive[4096 * 4];
// (tools/diag_wg_timeline.py) per workgroup: wall clock at the top of its first iteration, at the end of its first iteration, when it saw
// `done`, and after its last stores — what a launch of few iterations spends outside them
__device__ unsigned long long g_wg_timeline[4096 * 4];
#define TL(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_wg_timeline[blockIdx.x * 4 + (k)] = (unsigned long long)wall_clock64(); } while (0)
#else
#define TL(k) do { } while (0)
#endif

// SQ: the DPP form for the 16 x 16 square lattice in the reference's colouring (NPL = 4, no LDS slabs; Holstein: uniform hopping in
// two scalars, disordered hopping in per-site registers; SSH: a table set per time slice, SqSsh); otherwise the lane-program form
//     FORM 0: lane program, 1: the square-lattice DPP form (SQ), 2: the honeycomb DPP form (HC: 12 x 12 cells, six sites per lane of
//     which a quarter are mirror lanes, uniform hopping; cg_wg_dev.h), 4: the 8 x 8 DPP form, 5: the GRID form — any other even-L
//     square lattice up to 16 x 16 (cg_fast_common.h: 2 x 2 patches on a G x G grid of lanes, crossings by ds_bpermute), 6: the HGRID
//     form — any other honeycomb lattice up to 16 x 16 cells (1, 2 or 4 cells per lane on a grid of lanes; m.hc_L cells per side)
// SHARD: this launch is one rank's part of a solve over several GPUs (T = 1, lane-program form)
// X0Z: the initial guess is known to be zero (the library zeroed it for this solve): x0 is not read
// RANKS (with SHARD): SEVERAL RANKS OF ONE SHARDED SOLVE IN ONE LAUNCH (the slabs of a lattice beyond one wave's slice on ONE GPU,
// slabs.hip): rank q's G workgroups are the blocks q G .. q G + G - 1 and every rank's launch arguments — its slab's buffers, tables,
// control block, mailboxes — come from memory (R.ranks).  The ranks wait for each other, so they must all be resident: one grid
// guarantees what P streams do not (streams share the process's few hardware queues, and a queue runs its launches one after the other).
struct WgRankArgs { CgBufs B; ModelDev m; WgCtl R; ShardCtl Sh; };

// The forms of the kernel (its template parameter FORM stays an int: the numbers are part of the kernels' names).
enum Form { LANE = 0, SQ16 = 1, HC12 = 2, S8 = 4, GRID = 5, HGRID = 6, TGRID = 7 };

// Where the loop-invariant and the update-only vectors of a (form, sites per lane, slices per wave) live, and the dynamic LDS that follows
// from it — ONE statement for the kernel (which carves its pointers from it) and for the host (which sizes every launch from `total`).
struct WgPlace {
    int SL, LSL, HSL, NSLAB;      // doubles per lane-program slab | lanes per register and doubles per slice in LDS | LDS slabs per wave
    bool S_LDS, E_LDS, X_REG, E_SHARED, X_GLB, PH_LDS;
};
__host__ __device__ __forceinline__ constexpr WgPlace wg_place(int FORM, int NPL, int T, bool SSH) {
    const bool SQ = FORM == SQ16, HC = FORM == HC12, GR = FORM == GRID || FORM == TGRID;
    WgPlace P{};
    // slices in LDS: LSL lanes per register, HSL doubles per slice.  Honeycomb form: the 48 REAL lanes only — a mirror lane READS the
    // slot of the lane it mirrors (lr) and writes nothing (lwok): its r, exp(-dtau V) and halo values are the real lane's by
    // construction, and a quarter of the LDS is not spent on copies (what lets 3 slices per wave fit)
    P.SL = NPL * WAVE + 2 * WAVE; P.LSL = HC ? 48 : WAVE; P.HSL = NPL * P.LSL;
    P.NSLAB = FORM != LANE ? 0 : T + 1;            // (the other forms exchange registers)
    // 4 slices per wave (DPP form, throughput shape): exp(-dtau V) moves to LDS (read twice per iteration; 40 registers) and x stays in
    // registers instead (LDS is full); otherwise E in registers (0.35 us per iteration faster at 2 slices per wave), x and r in LDS
    // bond phonons, DPP form, 2 slices per wave: the table set of slice t0 in LDS (24 doubles per lane), x in registers
    P.S_LDS = SQ && SSH && T == 2;
    // honeycomb DPP form, 2 slices per wave: exp(-dtau V) in LDS too (six sites per lane: 36 registers)
    P.E_LDS = ((SQ || GR) && T >= 4) || (HC && T >= 2);
    P.X_REG = ((SQ || GR) && T >= 4) || P.S_LDS || (HC && T >= 3);
    // (honeycomb: neighbouring waves SHARE the slice of exp(-dtau V) between them — [W T + 1] slices per workgroup instead of W (T + 1);
    //  both write the same values to it)
    P.E_SHARED = HC;
    // honeycomb, 3 slices per wave: x lives in MEMORY (it is touched once per iteration, x += alpha p): its slices are loaded behind the
    // sums — the meeting that follows hides the round trip — and stored back by the update; between two updates no register holds it
    P.X_GLB = HC && T >= 3;
    // honeycomb, 3 slices per wave: the two HALO slices of p wait in LDS between the p-update that makes them and the mat-vec that
    // consumes them (24 registers that would otherwise sit through both sweeps)
    P.PH_LDS = HC && T >= 3;
    return P;
}
// The regions of the dynamic LDS, in doubles, each as the step from the region the kernel reaches it from:
//   [W][NSLAB][SL] slabs | r [W][T][HSL] | x [W][T][HSL] (unless X_REG) | exp(-dtau V) (E_LDS) or the SSH table set (S_LDS) |
//   partials and totals [48] | rhalo [2][HSL] | zhalo [2][HSL] | the halo slices of p [W][2][HSL] (PH_LDS)
struct WgLayout { size_t r, x_r, e_r, part_e, rhalo_part, zhalo_rhalo, ph_zhalo, total; };
__host__ __device__ __forceinline__ constexpr WgLayout wg_layout(int FORM, int NPL, int T, bool SSH, int W) {
    const WgPlace P = wg_place(FORM, NPL, T, SSH);
    WgLayout Y{};
    Y.r = (size_t)W * P.NSLAB * P.SL;
    Y.x_r = (size_t)W * T * P.HSL;
    Y.e_r = (size_t)(P.X_REG ? 1 : 2) * W * T * P.HSL;
    Y.part_e = P.E_LDS ? (P.E_SHARED ? ((size_t)W * T + 1) * P.HSL : (size_t)W * (T + 1) * P.HSL) : (P.S_LDS ? (size_t)W * SQ_TABS * WAVE : 0);
    Y.rhalo_part = 48;
    Y.zhalo_rhalo = 2 * P.HSL;
    Y.ph_zhalo = 2 * P.HSL;
    Y.total = Y.r + Y.e_r + Y.part_e + Y.rhalo_part + Y.zhalo_rhalo + Y.ph_zhalo + (P.PH_LDS ? (size_t)W * 2 * P.HSL : 0);
    return Y;
}
template <int NPL, int T, bool SSH, bool UNI, int FORM, bool SHARD, bool X0Z = false, bool RANKS = false>
__global__ void __launch_bounds__(512) k_cg_wg(CgBufs B, ModelDev m, WgCtl R, ShardCtl Sh) {
    static_assert(!RANKS || SHARD, "several ranks per launch: sharded solves only");
    unsigned bid = 0;
    if constexpr (RANKS) {
        const WgRankArgs *__restrict__ A = static_cast<const WgRankArgs *>(R.ranks);
        const unsigned rk = blockIdx.x / (unsigned)R.G;
        bid = blockIdx.x - rk * (unsigned)R.G;
        B = A[rk].B; m = A[rk].m; Sh = A[rk].Sh; R = A[rk].R;
    }
    constexpr bool SQ = FORM == Form::SQ16, HC = FORM == Form::HC12, S8 = FORM == Form::S8, TG = FORM == Form::TGRID, GR = FORM == Form::GRID || TG, HG = FORM == Form::HGRID, REGX = FORM != Form::LANE;      // REGX: the checkerboard exchanges registers, no LDS slabs
    // (FORM 7, TG: an even-L TRIANGULAR lattice up to 16 x 16 in the GRID layout — the same 2 x 2 patches, the two diagonal colours of
    //  pgrid::Tri<2, 2> added to the sweep, c^6 where the square lattice takes c^4)
    static_assert(!TG || !SHARD, "triangular grid form: no shards");
    static_assert(!HG || ((NPL == 2 || NPL == 4 || NPL == 8) && UNI && !SSH && T <= 2), "honeycomb grid form: 1, 2 or 4 cells per lane, uniform hopping, at most two slices per wave");
    static_assert(!GR || (NPL == 4 && UNI && !SSH && T <= 4), "grid form (even-L square lattices, 2 x 2 patches on a G x G lane grid): uniform hopping, at most four slices per wave");
    static_assert(!S8 || (NPL == 1 && UNI && !SSH && !SHARD), "8 x 8 DPP form: one site per lane, uniform hopping");
    static_assert(!SHARD || (T == 1 && (FORM == Form::LANE || FORM == Form::GRID || FORM == Form::HGRID)), "sharded solves: one slice per wave; lane-program, GRID or HGRID form (the slab closed into a ring)");
    static_assert(!HC || (NPL == HC_NPL && UNI && !SSH && T <= 3), "honeycomb DPP form: six sites per lane, uniform hopping");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    static_assert(!SQ || NPL == 4, "DPP form: the 16 x 16 square lattice, four sites per lane");
    static_assert(!(SQ && SSH) || (!UNI && T <= 2), "DPP form with bond phonons: a table set per slice, at most two slices per wave");
    static_assert(!SQ || UNI || T <= 2, "DPP form with per-site hopping: 32 registers of (cosh, sinh) leave room for two slices");
    constexpr int NE = MC * ((NPL + 1) / 2);
    // where the vectors live and how the LDS is cut: wg_place / wg_layout above, the host's statement too
    constexpr WgPlace PL = wg_place(FORM, NPL, T, SSH);
    constexpr int HS = NPL * WAVE, SL = PL.SL, LSL = PL.LSL, HSL = PL.HSL, NSLAB = PL.NSLAB;
    static_assert(SL == slab_len<NPL>(), "the slab of the lane-program sweeps");
    constexpr bool S_LDS = PL.S_LDS, E_LDS = PL.E_LDS, X_REG = PL.X_REG, E_SHARED = PL.E_SHARED, X_GLB = PL.X_GLB, PH_LDS = PL.PH_LDS;
    constexpr int NT = SSH ? T + 1 : 1;                // hopping-table sets (SSH: one per slice t0 .. t0+T)
    constexpr int NEJ = SSH ? 1 : T + 1;               // exp(-dtau V) slices (SSH: exp(dtau mu), per site only)
    constexpr int NSREG = (SQ && SSH) ? (S_LDS ? T : T + 1) : 1;
    const int W = R.W, G = R.G;
    // (a shard: ONE right-hand side, its G workgroups are the whole grid, spread over the XCDs — several ranks on one GPU, the test
    //  box, would otherwise pile their teams onto the XCD where every dispatch starts: 2 x 20 workgroups do not fit its 32 CUs)
    const int xcd = SHARD ? 0 : (blockIdx.x & 7), idx = SHARD ? (RANKS ? bid : blockIdx.x) : (blockIdx.x >> 3);
    const int tq = idx / G, g = idx - tq * G;
    // ONE solve per workgroup and an oversubscribed grid (teams at the dispatch frontier wait for members that start when another team
    // ends — blocks are dispatched in index order; the wall-clock bound, the fallback and the cool-down of elph_wg_cg are the guard).
    // Persistent teams that loop over right-hand sides measured 4 % slower (profiles/r03/wg_persistent_teams.log) and were removed.
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
    const int rhs = tq * 8 + xcd;
#ifdef ELPH_WG_ARRIVE
    // diagnostic build (tools/diag_wg_arrive.py): where and when every workgroup of the grid started — XCC_ID and the hardware id of its
    // CU, the wall clock — to see which members a team that timed out was waiting for
#ifndef ELPH_WG_ARRIVE_NOSTART
    if (threadIdx.x == 0 && blockIdx.x < 4096) {
        g_wg_arrive[blockIdx.x * 4 + 0] = 1ull + (unsigned long long)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20);      // XCC_ID[3:0]
        g_wg_arrive[blockIdx.x * 4 + 1] = (unsigned long long)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);            // HW_ID
        g_wg_arrive[blockIdx.x * 4 + 2] = (unsigned long long)wall_clock64();
    }
#endif
#endif
    if (rhs >= B.nrhs) return;
    const int N = m.N, L = m.L;
    const int t0 = (g * W + wv) * T;
    const int lr = HC ? 12 * (hc_src_lane(lane) >> 4) + (hc_src_lane(lane) & 15) - 2 : lane;      // LDS slot this lane reads (and, if lwok, writes)
    const int GGX = GR ? m.grid_GX : 0, GGY = GR ? m.grid_GY : 0;      // grid form: GX x GY lanes hold the lattice, the rest idle
    const int HLX = HG ? m.hc_LX : 0, HLY = HG ? m.hc_LY : 0;         // honeycomb grid form: (LX / PX) x (LY / PY) lanes
    const bool lwok = HC ? hc_real(lane) : (GR ? lane < GGX * GGY : (HG ? lane < (HLX / HgDim<NPL>::PX) * (HLY / HgDim<NPL>::PY) : true));
    const size_t ndim = (size_t)N * L;
    const WgLayout LY = wg_layout(FORM, NPL, T, SSH, W);
    double *slab = lds + (size_t)wv * NSLAB * SL;
    double *rall = lds + LY.r;                         // [W][T][HS]: r of every wave's slices — neighbours read their halo slices here
    double *rl = rall + (size_t)wv * T * HSL;
    double *xl = rall + LY.x_r + (size_t)wv * T * HSL; // [W][T][HSL]: this wave's slices of x (unless X_REG)
    double *eall = rall + LY.e_r;                      // [W][T+1][HSL]: exp(-dtau V) of slices t0 .. t0+T (E_LDS)
    double *el = eall + (size_t)wv * (E_SHARED ? T : T + 1) * HSL;
    double *partA = eall + LY.part_e, *partB = partA + 8, *bc = partA + 16;   // bc: p.z total, r.r total, 0.0 = a poller gave up
    // single-meeting form: part[4][8] wave partials of p.z, r.z, z.z, r.r | tot[8]: the four totals, [4] the direct r.r of the fallback
    // meeting, [5] 0.0 = a poller gave up | partF[8] | rhalo[2][HS]: the boundary slices of r of the two neighbouring workgroups (kept in
    // LDS rather than in registers: the 4-slice shape has none to spare)
    double *part = partA, *tot = partA + 32, *partF = partA + 40, *rhalo = partA + LY.rhalo_part, *zhalo = rhalo + LY.zhalo_rhalo;
    double *phl = zhalo + LY.ph_zhalo + (size_t)wv * 2 * HSL;         // [W][2][HSL]: the halo slices of p (PH_LDS)
#define PHALO(k, q) phl[((k) ? 1 : 0) * HSL + lr + (q) * LSL]   // zhalo[2][HS]: their boundary slices of z
    auto wrap = [L](int t) { return (t < 0) ? t + L : ((t >= L) ? t - L : t); };
    auto sgn = [](int t) { return (t == 0) ? -1.0 : 1.0; };
    const CgParams P = B.params;
    CgState *st2 = B.state + 2 * rhs;
    const CgState S = ld_state(st2);
    if (!SHARD && (S.done || S.seq != 0)) return;      // fresh solves only (the host guarantees it); a shard seeds its state below

    // site of register q of this lane: lane + 64 q (layout S order), or the column segments of the DPP form
    int sc[NPL], ss[NPL];
    bool live[NPL], own[NPL];                          // own: the site enters the inner products (a shard counts its own rows only)
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int s = SQ ? sq_patch_site(lane, q) : (HC ? hc_site(lane, q) : (S8 ? s8_site(lane) : (GR ? grid_site(lane, q, GGX, GGY) : (HG ? hgrid_site<NPL>(lane, q, HLX, HLY) : lane + q * WAVE))));
        live[q] = (GR || HG) ? lwok : (REGX || s < N);            // (DPP forms: every register of every lane holds a site — no selects in the sums)
        own[q] = SHARD ? (live[q] && s >= Sh.own_lo && s < Sh.own_hi) : (HC ? hc_real(lane) : live[q]);     // (honeycomb: mirror lanes carry copies)
        sc[q] = live[q] ? s : N - 1;
        ss[q] = live[q] ? s : N;                          // (a shard asks where a site sits among own and ghost rows: an idle register sits nowhere)
    }
    double *xg = B.x + (size_t)rhs * ndim, *rg = B.r + (size_t)rhs * ndim;
    const double *Ech = m.E + (size_t)(rhs % m.nchains) * m.E_chain_stride;

    // x and r live in this wave's LDS (lane-linear, conflict-free): both are only touched by the two vector updates, never by the
    // mat-vec — no register across the mat-vec, no vector-memory traffic inside the loop that a meeting's poll would wait behind,
    // and the neighbouring waves read their halo slices of r straight from here
    double zw[T + 1][NPL], p[T + 2][NPL], E[E_LDS ? 1 : NEJ][NPL], xr[X_REG ? T : 1][NPL];
    // (x0 = 0 known to the library: a compile-time variant, X0Z, does not read it — 12 us less per launch of 288 right-hand sides.  As a
    //  RUN-TIME choice, and likewise reading the own slices of r0 once for r and p0 = r0, it changes the register assignment of the
    //  LOOP — 256 registers, none to spare at 4 slices per wave — and costs it 8-20 %: 5.6-6.4 against 5.2 us per iteration at 48
    //  right-hand sides (profiles/r03/wg_load_variants.log).)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            if (lwok) rl[j * HSL + lr + q * LSL] = rg[(size_t)(t0 + j) * N + sc[q]];
            if (X_GLB) {}      // (x0 is where it is: the caller's initial guess in memory)
            else if (X_REG) xr[X_REG ? j : 0][q] = X0Z ? 0.0 : xg[(size_t)(t0 + j) * N + sc[q]];
            else if (lwok) xl[j * HSL + lr + q * LSL] = X0Z ? 0.0 : xg[(size_t)(t0 + j) * N + sc[q]];
        }
#pragma unroll
    for (int j = 0; j < T + 2; ++j)
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            p[j][q] = rg[(size_t)wrap(t0 + j - 1) * N + sc[q]];      // p0 = r0 (:272): one vector less to read
            if (PH_LDS && (j == 0 || j == T + 1) && lwok) PHALO(j, q) = p[j][q];
        }
#pragma unroll
    for (int j = 0; j < NEJ; ++j)
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const double ev = Ech[(size_t)wrap(t0 + j) * m.E_tau_stride + sc[q]];
            if (E_LDS) { if (lwok) el[j * HSL + lr + q * LSL] = ev; }
            else E[E_LDS ? 0 : j][q] = ev;
        }
    unsigned ij[NE];
    Tab<NE, UNI> tab[NT];
    SqCtx<UNI> X;
    SqSsh<NSREG, S_LDS> XS;
    HcCtx XH;
    S8Ctx X8;
    GridCtx XG;
    HgCtx XHG;
    pgrid::Ctx XT;
    if constexpr (GR) {
        XG = grid_ctx(lane, GGX, GGY, m.c_uni, m.s_uni);
        if constexpr (TG) { XT = pgrid::Tri<2, 2>::make_ctx(lane, 2 * GGX, m.c_uni, m.s_uni); XG.k4 = XT.ks; }      // (k4 carries c^6 here)
    } else if constexpr (HG) {
        XHG = hgrid_ctx<NPL>(lane, HLX, HLY, m.c_uni, m.s_uni);
    } else if constexpr (S8) {
        X8.th = m.s_uni / m.c_uni; X8.k4 = (m.c_uni * m.c_uni) * (m.c_uni * m.c_uni);
        X8.yx = sq_patch_ycross(lane); X8.xodd = (lane >> 1) & 1;
    } else if constexpr (HC) {
        XH.th = m.s_uni / m.c_uni; XH.k3 = m.c_uni * m.c_uni * m.c_uni;
        XH.up = (lane + 16) & (WAVE - 1); XH.dn = (lane + 48) & (WAVE - 1);
    } else if constexpr (SQ && SSH) {
        // table set j = the hopping of slice t0 + j, gathered from the per-(tau, bond) tables through the site -> bond map of each colour
        ssh_chain_select(m, rhs);
        XS.yx = sq_patch_ycross(lane);
        XS.l0 = eall + (size_t)wv * SQ_TABS * WAVE + lane;
#pragma unroll
        for (int j = 0; j <= T; ++j) {
            const double *cj = m.c + (size_t)wrap(t0 + j) * m.cs_tau_stride, *sj = m.s + (size_t)wrap(t0 + j) * m.cs_tau_stride;
            SqTabS tb;
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                const int b0 = m.sq_bond[0 * N + sc[2 * pr]], b2 = m.sq_bond[2 * N + sc[pr]];
                tb.ci[0][pr] = cj[b0]; tb.si[0][pr] = sj[b0];
                tb.ci[1][pr] = cj[b2]; tb.si[1][pr] = sj[b2];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b1 = m.sq_bond[1 * N + sc[k]], b3 = m.sq_bond[3 * N + sc[k]];
                tb.cx[0][k] = cj[b1]; tb.sx[0][k] = sj[b1];
                tb.cx[1][k] = cj[b3]; tb.sx[1][k] = sj[b3];
            }
            if (S_LDS && j == 0) {
                double *d = eall + (size_t)wv * SQ_TABS * WAVE + lane;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    d[(0 + pr) * WAVE] = tb.ci[0][pr]; d[(2 + pr) * WAVE] = tb.si[0][pr];
                    d[(4 + pr) * WAVE] = tb.ci[1][pr]; d[(6 + pr) * WAVE] = tb.si[1][pr];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    d[(8 + k) * WAVE] = tb.cx[0][k]; d[(12 + k) * WAVE] = tb.sx[0][k];
                    d[(16 + k) * WAVE] = tb.cx[1][k]; d[(20 + k) * WAVE] = tb.sx[1][k];
                }
            } else {
                XS.t[S_LDS ? (j > 0 ? j - 1 : 0) : (j < NSREG ? j : 0)] = tb;
            }
        }
    } else if constexpr (SQ) {
        X.yx = sq_patch_ycross(lane);
        if constexpr (UNI) {
            X.c[0][0] = m.c_uni; X.s[0][0] = m.s_uni / m.c_uni; X.k4 = (m.c_uni * m.c_uni) * (m.c_uni * m.c_uni);
        } else {
            X.k4 = 1.0;
#pragma unroll
            for (int col = 0; col < 4; ++col)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int bd = m.sq_bond[col * N + sc[k]];
                    X.c[UNI ? 0 : col][UNI ? 0 : k] = m.c[bd];
                    X.s[UNI ? 0 : col][UNI ? 0 : k] = m.s[bd];
                }
        }
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) ij[e] = m.lp_ij[e * WAVE + lane];
        if (SSH) {
            ssh_chain_select(m, rhs);
#pragma unroll
            for (int j = 0; j < NT; ++j)
                load_tab<NE, UNI>(tab[j], m.lp_c + (size_t)wrap(t0 + j) * m.lp_tau_stride, m.lp_s + (size_t)wrap(t0 + j) * m.lp_tau_stride, lane, m);
        } else {
            load_tab<NE, UNI>(tab[0], m.lp_c, m.lp_s, lane, m);
        }
    }
#define EXPV(j, q) (E_LDS ? el[(j) * HSL + lr + (q) * LSL] : E[(SSH || E_LDS) ? 0 : (j)][q])

    // records and boundary granules exist TWICE, by the parity of the iteration: a workgroup that has met for iteration k goes on and
    // publishes its record of k + 1 one mat-vec later — into the OTHER set, so that a member that is late reading the records of k
    // (its polling wave held up: two workgroups sharing a CU, a time-sliced GPU) still finds them; nobody can reach k + 2 before that
    // member has published k + 1, i.e. finished reading k.  (With a single set such a member waited for tags that had already moved on —
    // the time-out of the experimental 4-wave shape, tools/diag_wg_arrive.py.)
    constexpr size_t SLOTS_RHS = SLOTS_PER_RHS;
    u64 *const slots0 = R.slots + (size_t)rhs * 2 * SLOTS_RHS;
    u64 *const bnd0 = R.bnd + (size_t)rhs * 2 * G * 2 * HS * 2;     // [parity][G][first | last slice][HS][2 granules]
    const int gm = (g == 0) ? G - 1 : g - 1, gp = (g == G - 1) ? 0 : g + 1;
    double rho = S.rho, kmin = S.kmin, eps = S.eps;
    double eps0 = S.eps0, normb = S.normb;

    // (ordered before their first readers by the barriers that follow.  bc — the seed meeting of a shard — shares its three words with
    //  part[16..18], the z.z partials of waves 0..2: in an un-sharded solve it must NOT be touched here — nothing orders this store of wave 0 before the first iteration's part[] stores of a wave that finished its
    //  set-up sooner, and a late 1.0 in place of wave 2's z.z partial costs that solve its first beta: one iteration more, about one
    //  first solve in three of a fresh handle with the slow set-up of the bond-phonon DPP form)
    if (threadIdx.x == 0) { tot[5] = 1.0; if (SHARD) bc[2] = 1.0; }
    // the boundary waves of a workgroup keep the neighbouring workgroup's boundary slice of r (p0 = r0: it sits in the halo of p)
    if (G > 1) {
        if (wv == 0) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) if (lwok) rhalo[lr + q * LSL] = p[0][q];
        }
        if (wv == W - 1) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) if (lwok) rhalo[HSL + lr + q * LSL] = p[T + 1][q];
        }
    }
    // ghost sites of this lane: where their values arrive in the own mailbox (nullptr: not a ghost site), slice t0
    const u64 *gaddr[NPL];
    if constexpr (SHARD) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int s = ss[q];
            gaddr[q] = (s < Sh.own_lo) ? sh_ghost(Sh.mail[Sh.rank], 0, L, Sh.cap_ghost, t0, s)
                     : (s >= Sh.own_hi && s < N) ? sh_ghost(Sh.mail[Sh.rank], 1, L, Sh.cap_ghost, t0, s - Sh.own_hi) : nullptr;
        }
        // x0 = 0, r0 = p0 = b (the host put b into r and p): |b|^2 over the own sites of all ranks seeds the state
        // (IterativeSolvers.jl:259-274 with x = 0: eps0 = 1, rho0 = |b|^2)
        double a0 = 0.0;
#pragma unroll
        for (int q = 0; q < NPL; ++q) if (own[q]) a0 += p[1][q] * p[1][q];
        a0 = wave_sum_dpp(a0);
        if (lane == 0) partA[wv] = a0;
        wg_barrier();
        if (wv == 0) {
            const double mine = wg_sum(partA, W, lane);
            sh_publish<RANKS>(Sh, 0, g, G, mine, 1u, lane);
            const u64 *none[NPL];
#pragma unroll
            for (int q = 0; q < NPL; ++q) none[q] = nullptr;
            double tot = 0.0, dummy[NPL];
            const bool ok = sh_poll<NPL, RANKS>(Sh, true, 0, G, none, 1u, lane, R, tot, dummy);
            if (lane == 0) { bc[0] = tot; if (!ok) bc[2] = 0.0; }
        }
        wg_barrier();
        if (bc[2] == 0.0) return;
        const double bb = bc[0];
        normb = sqrt(bb); eps0 = 1.0; eps = 1.0; rho = bb; kmin = 0.0;
        wg_barrier();                                   // bc[0] is rewritten by the first meeting of the loop
    }
    // screens of the stop test (see there)
    double rr_far = (P.tol * normb) * (P.tol * normb) * 1.000001, y_num = 4.0 * (eps0 * normb) * (eps0 * normb);
    double it_kappa = 0.17 * sqrt(P.kmax);
    // FUSED (un-sharded solves of two and more slices per wave): the tail of an iteration decides first — alpha, r'.r', the stop test and beta follow from the
    // meeting's four sums alone — and then makes ONE pass over the own slices: r' = r - alpha z (to LDS for the neighbours), x += alpha p and
    // p = r' + beta p from the r' it holds in a register.  (The order it replaces — update, barrier, stop test, p-update — read every
    // r' back from LDS behind the barrier.)
    // One slice per wave keeps the old order (config C, 2 right-hand sides: 3.40 us per iteration against 3.44 with the pass).
    // BSUM (the square-lattice DPP forms): the four sums are added behind each batch of reverse sweeps.
    constexpr bool FUSED = !SHARD && T >= 2, BSUM = SQ;
    // RPOLL (the 16 x 16 uniform form at 4 slices per wave): the pass's sixteen reads of the own slices of r go out in the meeting's poll
    // window, into registers the reverse batches have left free — nothing writes a wave's own r between the first barrier of the
    // iteration and the pass (the neighbours only read it, the wave itself writes it in the pass), the `lgkmcnt(0)` of the barrier
    // behind the poll retires them while every wave waits for L2 anyway, and the pass starts its fma the moment beta exists and issues
    // only its sixteen stores.  Left alone the eight waves queued 16 reads + 16 writes each at the CU's LDS with the vector ALU idle.
    constexpr bool RPOLL = SQ && !SSH && UNI && T == 4 && !SHARD;
    // (alpha, beta and the screens of the stop test carry the same bits in every lane: FUSED keeps them in scalar registers — the pass holds
    //  alpha AND beta, and the 4-slice shape has no vector register to spare)
    auto uni = [](double v) __attribute__((always_inline)) {
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    };
    if constexpr (FUSED) { rr_far = uni(rr_far); y_num = uni(y_num); it_kappa = uni(it_kappa); normb = uni(normb); eps0 = uni(eps0); }
    // RPOLL, teams of two and more: the boundary wave W-1 issues in front of its SIMD's other wave for the whole solve.  The parent's
    // phase stamps show wave W-1 reaching the barrier in front of the meeting last; the supposed reason is that it is the younger wave
    // of its SIMD (the arbitration's loser) AND issues the sixteen granule stores of z with their addresses and selects, while wave 0
    // does the same stores as the older wave.  What was measured is in DESIGN.md section 3 and profiles/wg_boundary_waves.  ONE
    // s_setprio, under a condition read as a scalar: the instruction ignores EXEC, under a lane predicate every wave would raise
    // itself.  (Raised at the top of the mat-vec and dropped behind the first barrier instead, so that a polling wave never outranks
    // its partner: 0.7 % SLOWER than no priority at all.)
    if constexpr (RPOLL) {
        if (G > 1 && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == W - 1) __builtin_amdgcn_s_setprio(1);
    }
    STAMP_DECL;
    for (long long seq = 0;; ++seq) {
        const unsigned epoch = R.epoch0 + (unsigned)seq + (SHARD ? 2u : 1u);
        const unsigned par = epoch & 1u;
        u64 *const slotsA = slots0 + (size_t)par * SLOTS_RHS, *const slotsB = slotsA + SLOTS_A;
        u64 *const bnd = bnd0 + (size_t)par * G * 2 * HS * 2;
        const size_t ghp = SHARD ? (size_t)par * 2 * L * Sh.cap_ghost * 2 : 0;      // (a shard: the ghost rows of z in the mailboxes, by parity too)
        STAMP(9);
        if (seq == 0) TL(0);
        if (seq == 1) TL(1);
        // ---- z = M^T M p on the own slices:  w(t) = p(t) - sg(t) CB_t [E(t) p(t-1)]  for t = t0 .. t0+T  (T+1 forward sweeps at once),
        //      z(t) = w(t) - sg(t+1) E(t+1) CB_{t+1}^T w(t+1)  for t = t0 .. t0+T-1  (T reverse sweeps at once)
        // (w and z share registers: z(t0+j) overwrites w(t0+j) once the reverse sweep of w(t0+j+1) has been taken)
        double (&w)[T + 1][NPL] = zw;
        double b_pz = 0.0, b_rz = 0.0, b_zz = 0.0, b_rr = 0.0;   // BSUM: the four sums of the meeting (see there), summed behind the reverse batches
        if constexpr (S8) {
#pragma unroll
            for (int k = 0; k <= T; ++k) w[k][0] = EXPV(k, 0) * p[k][0];
            s8_sweepN<T + 1, false>(w, X8);
#pragma unroll
            for (int k = 0; k <= T; ++k) w[k][0] = p[k + 1][0] - sgn(wrap(t0 + k)) * X8.k4 * w[k][0];
            double gq[T][1];
#pragma unroll
            for (int i = 0; i < T; ++i) gq[i][0] = w[i + 1][0];
            s8_sweepN<T, true>(gq, X8);
#pragma unroll
            for (int i = 0; i < T; ++i) w[i][0] = w[i][0] - sgn(wrap(t0 + i + 1)) * X8.k4 * (EXPV(i + 1, 0) * gq[i][0]);      // z(t0+i)
        } else if constexpr (HC) {
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[k][q] = EXPV(k, q) * ((PH_LDS && k == 0) ? PHALO(0, q) : p[k][q]);
            hc_sweepN<T + 1, false>(w, XH);
#pragma unroll
            for (int k = 0; k <= T; ++k) {
                const double sg = sgn(wrap(t0 + k)) * XH.k3;
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[k][q] = ((PH_LDS && k == T) ? PHALO(1, q) : p[k + 1][q]) - sg * w[k][q];
            }
            // reverse sweeps of the slabs J0 .. J0 + NB - 1 at once (both compile-time: a run-time index into w would put it on the stack)
            auto rev = [&](auto nb, auto j0c) __attribute__((always_inline)) {
                constexpr int NB = decltype(nb)::value, j0 = decltype(j0c)::value;
                double gq[NB][NPL];
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) gq[i][q] = w[j0 + i + 1][q];
                hc_sweepN<NB, true>(gq, XH);
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const double sg = sgn(wrap(t0 + j0 + i + 1)) * XH.k3;
#pragma unroll
                    for (int q = 0; q < NPL; ++q) w[j0 + i][q] = w[j0 + i][q] - sg * (EXPV(j0 + i + 1, q) * gq[i][q]);     // z(t0+j0+i)
                }
            };
            using std::integral_constant;
            if constexpr (T == 3) { rev(integral_constant<int, 2>(), integral_constant<int, 0>()); rev(integral_constant<int, 1>(), integral_constant<int, 2>()); }
            else rev(integral_constant<int, T>(), integral_constant<int, 0>());
        } else if constexpr (HG) {
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[k][q] = EXPV(k, q) * p[k][q];
            hgrid_sweepN<NPL, T + 1, false>(w, XHG);
#pragma unroll
            for (int k = 0; k <= T; ++k) {
                const double sg = sgn(wrap(t0 + k)) * XHG.k3;
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[k][q] = p[k + 1][q] - sg * w[k][q];
            }
            double gq[T][NPL];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int q = 0; q < NPL; ++q) gq[i][q] = w[i + 1][q];
            hgrid_sweepN<NPL, T, true>(gq, XHG);
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const double sg = sgn(wrap(t0 + i + 1)) * XHG.k3;
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[i][q] = w[i][q] - sg * (EXPV(i + 1, q) * gq[i][q]);      // z(t0+i)
            }
        } else if constexpr (GR) {
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = EXPV(k, q) * p[k][q];
            if constexpr (TG) {
#pragma unroll
                for (int k = 0; k <= T; ++k) pgrid::Tri<2, 2>::apply<false>(w[k], XT);
            } else grid_sweepN<T + 1, false, (T >= 4) ? 1 : 2>(w, XG);
#pragma unroll
            for (int k = 0; k <= T; ++k) {
                const double sg = sgn(wrap(t0 + k)) * XG.k4;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = p[k + 1][q] - sg * w[k][q];
            }
            constexpr int RBG = (T >= 4) ? 2 : T;            // reverse sweeps per batch (4 slices per wave: two batches, as in the DPP form)
#pragma unroll
            for (int j0 = 0; j0 < T; j0 += RBG) {
                double gq[RBG][4];
#pragma unroll
                for (int i = 0; i < RBG; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) gq[i][q] = w[j0 + i + 1][q];
                if constexpr (TG) {
#pragma unroll
                    for (int i = 0; i < RBG; ++i) pgrid::Tri<2, 2>::apply<true>(gq[i], XT);
                } else grid_sweepN<RBG, true, (T >= 4) ? 1 : 2>(gq, XG);
#pragma unroll
                for (int i = 0; i < RBG; ++i) {
                    const double sg = sgn(wrap(t0 + j0 + i + 1)) * XG.k4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) w[j0 + i][q] = w[j0 + i][q] - sg * (EXPV(j0 + i + 1, q) * gq[i][q]);      // z(t0+j0+i)
                }
            }
        } else if constexpr (SQ && !SSH && UNI && T == 4) {
            // 4 slices per wave: the arithmetic of the branch below in another interleaving.  The y-odd colour's crossing (ds_bpermute; the
            // eight waves of the workgroup queue at the CU's one LDS crossbar) is ISSUED for a pair of slabs and APPLIED only after work that
            // does not need it (cg_wg_dev.h: sq_cross_issue / sq_cross_apply), and the slices of exp(-dtau V) and of r that a reverse
            // batch reads from LDS are all requested at once, one colour before they are used — LDS operations return in order, so a
            // read behind a crossing waits for the crossing and a read that is waited for at once exposes its whole latency.  Every fma
            // keeps its operands and every sum its (slice, register) order: the same bits.  The colours stay colour-major over the slabs:
            // a slab-PAIR-major forward sweep (colours 0 .. 2 of the next pair under a pair's crossing, 52 vector instructions of cover
            // instead of 12 .. 26) measured 3 % SLOWER than the parent — consecutive colours of one pair depend on each other, colours of
            // different pairs do not (profiles/wg_sweep_order).
            // The forward prologue's ten reads of exp(-dtau V) go out together, into the registers of w (z was consumed by the fused pass:
            // they are free), in a scheduling region of their own, and the products retire them with counted waits — the compiler, no
            // register to spare, had serialised them (read, wait, two products, read, ...: eight waits with 0 .. 4 vector instructions of
            // cover at the very top of every wave's chain).  The same v_mul_f64 on the same operands.
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = EXPV(k, q);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = w[k][q] * p[k][q];
            auto fwd_tail = [&](auto kc) __attribute__((always_inline)) {              // w(t0+k) from the swept slab k
                constexpr int k = decltype(kc)::value;
                const double sg = sgn(wrap(t0 + k)) * X.k4;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = p[k + 1][q] - sg * w[k][q];
            };
            using std::integral_constant;
            using SX = SqCtx<UNI>;
            double c0[2], c1[2], d0[2], d1[2], e0[1], e1[1];
            // forward sweeps (y-odd is the last colour): the crossing of slabs 0, 1 under the y-even colour of slabs 2 .. 4, that of slabs
            // 2, 3 under the epilogue of slabs 0, 1, that of slab 4 under the epilogue of slabs 2, 3 — and between those two the crossing
            // of the FIRST reverse batch (y-odd is its first colour; w(t0+1), w(t0+2) are final by then)
            sq_pairs<T + 1, 0, 0, SX>(w, X); sq_pairs<T + 1, 0, 1, SX>(w, X);
            sq_colour<2, 2, 0, SX>(&w[0], X);
            sq_cross_issue<2, SX>(&w[0], X, c0, c1);
            sq_colour<2, 2, 2, SX>(&w[2], X); sq_colour<1, 2, 4, SX>(&w[4], X);
            sq_cross_apply<2, 0, SX>(&w[0], X, c0, c1);
            sq_cross_issue<2, SX>(&w[2], X, c0, c1);
            fwd_tail(integral_constant<int, 0>()); fwd_tail(integral_constant<int, 1>());
            __builtin_amdgcn_sched_barrier(0);
            sq_cross_apply<2, 2, SX>(&w[2], X, c0, c1);
            sq_cross_issue<1, SX>(&w[4], X, e0, e1);
            fwd_tail(integral_constant<int, 2>());
            __builtin_amdgcn_sched_barrier(0);
            sq_cross_issue<2, SX>(&w[1], X, d0, d1);
            fwd_tail(integral_constant<int, 3>());
            __builtin_amdgcn_sched_barrier(0);
            sq_cross_apply<1, 4, SX>(&w[4], X, e0, e1);
            fwd_tail(integral_constant<int, 4>());
            __builtin_amdgcn_sched_barrier(0);
            // a reverse batch of two slabs whose crossing (x0, x1) is in flight: z(t0+j0+i) and the batch's share of the four sums, in the
            // order of the branch below.  exp(-dtau V) is requested before the x-odd colour; r before the NEXT batch's crossing is issued,
            // into the registers the swept slabs leave free — that crossing then has the 32 fma of the sums to itself.
            auto rev_batch = [&](auto j0c, const double (&x0)[2], const double (&x1)[2], auto next_crossing) __attribute__((always_inline)) {
                constexpr int j0 = decltype(j0c)::value;
                double gq[2][4], ev[2][4], rv[2][4];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) gq[i][q] = w[j0 + i + 1][q];
                sq_cross_apply<2, 0, SX>(gq, X, x0, x1);
                sq_colour<2, 2, 0, SX>(gq, X);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) ev[i][q] = EXPV(j0 + i + 1, q);
                __builtin_amdgcn_sched_barrier(0);
                sq_colour<2, 1, 0, SX>(gq, X);
                sq_colour<2, 0, 0, SX>(gq, X);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const double sg = sgn(wrap(t0 + j0 + i + 1)) * X.k4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) w[j0 + i][q] = w[j0 + i][q] - sg * (ev[i][q] * gq[i][q]);    // z(t0+j0+i)
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) rv[i][q] = rl[(j0 + i) * HSL + lr + q * LSL];
                __builtin_amdgcn_sched_barrier(0);
                next_crossing();
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        b_pz += p[j0 + i + 1][q] * w[j0 + i][q];
                        b_rz += rv[i][q] * w[j0 + i][q];
                        b_zz += w[j0 + i][q] * w[j0 + i][q];
                        b_rr += rv[i][q] * rv[i][q];
                    }
                __builtin_amdgcn_sched_barrier(0);
            };
            rev_batch(integral_constant<int, 0>(), d0, d1, [&]() __attribute__((always_inline)) { sq_cross_issue<2, SX>(&w[3], X, c0, c1); });
            rev_batch(integral_constant<int, 2>(), c0, c1, []() {});
        } else if constexpr (SQ) {
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = EXPV(k, q) * p[k][q];
            if constexpr (SSH) sq_sweepS<T + 1, false, 0>(w, XS);
            else sq_sweepN<T + 1, false, UNI>(w, X);
#pragma unroll
            for (int k = 0; k <= T; ++k) {
                const double sg = UNI ? sgn(wrap(t0 + k)) * X.k4 : sgn(wrap(t0 + k));
#pragma unroll
                for (int q = 0; q < 4; ++q) w[k][q] = p[k + 1][q] - sg * w[k][q];
            }
            constexpr int RB = (T >= 4) ? 2 : T;             // reverse sweeps per batch (4 slices per wave: two batches, 16 registers less)
#pragma unroll
            for (int j0 = 0; j0 < T; j0 += RB) {
                double gq[RB][4];
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) gq[i][q] = w[j0 + i + 1][q];
                if constexpr (SSH) sq_sweepS<RB, true, 1>(gq, XS);          // (RB = T: one batch, the sets of t0+1 ..)
                else sq_sweepN<RB, true, UNI>(gq, X);
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const double sg = UNI ? sgn(wrap(t0 + j0 + i + 1)) * X.k4 : sgn(wrap(t0 + j0 + i + 1));
#pragma unroll
                    for (int q = 0; q < 4; ++q) w[j0 + i][q] = w[j0 + i][q] - sg * (EXPV(j0 + i + 1, q) * gq[i][q]);    // z(t0+j0+i)
                }
                // the four sums over the slices of this batch, in the (j, q) order of the single loop of the other forms: with two batches
                // the first batch's share overlaps the cross-lane latency of the second batch's sweeps
                if constexpr (BSUM) {
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (own[q]) {
                            const double rv = rl[(j0 + i) * HSL + lr + q * LSL];
                            b_pz += p[j0 + i + 1][q] * w[j0 + i][q];
                            b_rz += rv * w[j0 + i][q];
                            b_zz += w[j0 + i][q] * w[j0 + i][q];
                            b_rr += rv * rv;
                        }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k <= T; ++k)
#pragma unroll
                for (int q = 0; q < NPL; ++q) slab[k * SL + lane + q * WAVE] = EXPV(k, q) * p[k][q];
            WAVE_LDS_ORDER();
            sweepN<NPL, T + 1, false, UNI, NT, SSH ? 1 : 0, 0>(slab, ij, tab, m.ncol);
#pragma unroll
            for (int k = 0; k <= T; ++k) {
                const double sg = sgn(wrap(t0 + k));
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[k][q] = p[k + 1][q] - sg * slab[k * SL + lane + q * WAVE];
            }
            WAVE_LDS_ORDER();
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) slab[j * SL + lane + q * WAVE] = w[j + 1][q];
            WAVE_LDS_ORDER();
            sweepN<NPL, T, true, UNI, NT, SSH ? 1 : 0, SSH ? 1 : 0>(slab, ij, tab, m.ncol);
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const double sg = sgn(wrap(t0 + j + 1));
#pragma unroll
                for (int q = 0; q < NPL; ++q) w[j][q] = w[j][q] - sg * EXPV(j + 1, q) * slab[j * SL + lane + q * WAVE];       // z(t0+j)
            }
            WAVE_LDS_ORDER();
        }
        double (&z)[T + 1][NPL] = zw;                         // rows 0 .. T-1
        // (honeycomb, 3 slices per wave: the addresses of the boundary granules are made afresh every iteration from a laundered lane
        //  number — kept across the loop they are 2 registers each, 24 of them, in a kernel that has none to spare)
        int lane_b = lane;
        if constexpr (HC && T >= 3) asm volatile("" : "+v"(lane_b));
        double rr;                                            // r.r of the NEW residual
        double alpha_f = 0.0;                                 // FUSED: alpha, for the pass behind the stop test
        double rt[RPOLL ? T : 1][NPL];                        // RPOLL: the own slices of r, read in the poll window for the pass
        // (RPOLL INVARIANT: the pass stores the interior slices 1 .. T-2 of rl late — behind the barrier that follows it and the halo
        //  reads, and not at all on the `done` exit.  No other wave, and no exit path, reads the interior slices of rl under RPOLL: their
        //  only readers are this wave's own reads in the next mat-vec and poll window, in order behind its own stores.  A new reader
        //  of rl on an exit path — as SHARD has for rg — would get stale interior slices.)
        {   // ================= the single-meeting iteration ==================================================================
        // The two meetings of the textbook iteration (p.z -> alpha; then r.r of the new residual and its boundary slices -> beta, halo
        // of p) fold into ONE: every workgroup publishes FOUR sums — p.z, r.z, z.z and the r.r of the current residual — and the
        // boundary slices of z.  With them every wave has  alpha = r.r / p.z  and, by the algebraic identity of r' = r - alpha z,
        //     r'.r' = r.r - 2 alpha r.z + alpha^2 z.z
        // so beta and the stop test need no second reduction, and the neighbour's boundary slice of r' is its r (kept here) minus
        // alpha times its z (just received).  The direct r.r enters every iteration afresh (summed from the actual vector when it is
        // made, published one meeting later): the identity is applied for ONE step only, its rounding error (a few ulp of r.r) never
        // accumulates.  When the step shrinks the residual so much that the identity cancels (r'.r' < r.r / 1000: never in the
        // hundreds of iterations of these matrices, but possible on a nearly diagonal one) the direct sum is taken in a second,
        // single-sum meeting — the same branch in every wave of the team, since all hold the same bits.
        double s_pz = b_pz, s_rz = b_rz, s_zz = b_zz, s_rr = b_rr;
        if constexpr (!BSUM) {                                // (BSUM: summed behind the reverse batches)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int q = 0; q < NPL; ++q)
                if (own[q]) {
                    const double rv = rl[j * HSL + lr + q * LSL];
                    s_pz += p[j + 1][q] * z[j][q];
                    s_rz += rv * z[j][q];
                    s_zz += z[j][q] * z[j][q];
                    s_rr += rv * rv;
                }
        }
        {
            const double k4 = wave_sum4(s_pz, s_rz, s_zz, s_rr, lane);
            if (lane < 4) part[lane * 8 + wv] = k4;
        }
        if constexpr (X_GLB) {
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) xr[X_REG ? j : 0][q] = xg[(size_t)(t0 + j) * N + sc[q]];
        }
        if constexpr (SHARD) {
            // the rows of z my rank neighbours hold as ghosts: straight into their mailboxes (device-initiated stores over xGMI),
            // self-tagged — with alpha from the meeting the neighbour makes its ghost rows of the new residual itself
            const int prev = (Sh.rank + Sh.P - 1) % Sh.P, next = (Sh.rank + 1) % Sh.P;
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const int s = ss[q];
                const u64 bits = (u64)__double_as_longlong(z[0][q]), tag = (u64)epoch << 32;
                if (s >= Sh.own_lo && s < Sh.own_lo + Sh.n_to_prev) {              // bottom rows -> previous rank's ghosts above its own rows
                    u64 *d = sh_ghost(Sh.mail[prev], 1, L, Sh.cap_ghost, t0, s - Sh.own_lo) + ghp;
                    st_mail<RANKS>(d, tag | (bits & 0xFFFFFFFFull)); st_mail<RANKS>(d + 1, tag | (bits >> 32));
                }
                if (s >= Sh.own_hi - Sh.n_to_next && s < Sh.own_hi) {              // top rows -> next rank's ghosts below its own rows
                    u64 *d = sh_ghost(Sh.mail[next], 0, L, Sh.cap_ghost, t0, s - (Sh.own_hi - Sh.n_to_next)) + ghp;
                    st_mail<RANKS>(d, tag | (bits & 0xFFFFFFFFull)); st_mail<RANKS>(d + 1, tag | (bits >> 32));
                }
            }
        }
        if (G > 1) {                                          // boundary slices of z for the neighbouring workgroups (self-tagged granules)
            if (wv == 0) {
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    st_f64_gran(bnd + (((size_t)g * 2 + 0) * HS + lane_b + q * WAVE) * 2, z[0][q], epoch);
                    if constexpr (HC && T >= 3) __builtin_amdgcn_sched_barrier(0);      // (one value's granules and address at a time)
                }
            }
            if (wv == W - 1) {
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    st_f64_gran(bnd + (((size_t)g * 2 + 1) * HS + lane_b + q * WAVE) * 2, z[T - 1][q], epoch);
                    if constexpr (HC && T >= 3) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        STAMP(0);
        wg_barrier();
        STAMP(2);
        double pap, rz, zz, rr0;
        double gz[NPL];                                       // a shard: z of this wave's slice on the ghost rows (from the rank neighbours)
        if constexpr (SHARD) {
            // Two-level meeting.  Every workgroup publishes its four sums to the workgroups of its rank (device memory); workgroup 0
            // of the rank adds them and stores the RANK's record into every rank's mailbox; every workgroup then adds the P rank
            // records in rank order — one local hop and one hop between GPUs per iteration (round 2: two meetings of P G records
            // each).  Meanwhile every wave takes the ghost rows of z of its slice from the own mailbox, the two boundary waves also
            // the neighbouring workgroup's boundary slice of z (own rows from that workgroup, ghost rows from the mailbox).
            const int rw = (W >= 3) ? 1 : 0;
            u64 *rankrec = Sh.mail[Sh.rank] + (size_t)SH_MAXREC * 2 + (size_t)par * 8 * REC4;      // [parity][P <= 8][8 granules] (the area of round 2's second meeting)
            bool ok = true;
            if (wv == rw) publish_rec4(slotsA, g, sum_part4(part, W, lane), epoch, lane);
            {   // ghost rows of the own slice (+ the halo slice of a boundary wave)
                const bool bw = G > 1 && (wv == 0 || wv == W - 1);
                const int th = (wv == 0) ? wrap(t0 - 1) : wrap(t0 + T);
                const u64 *bh = bw ? ((wv == 0) ? bnd + (((size_t)gm * 2 + 1) * HS) * 2 : bnd + (((size_t)gp * 2 + 0) * HS) * 2) : nullptr;
                const u64 *ga2[NPL];
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    const int s = ss[q];
                    ga2[q] = !bw ? nullptr
                           : (s < Sh.own_lo) ? sh_ghost(Sh.mail[Sh.rank], 0, L, Sh.cap_ghost, th, s) + ghp
                           : (s >= Sh.own_hi && s < N) ? sh_ghost(Sh.mail[Sh.rank], 1, L, Sh.cap_ghost, th, s - Sh.own_hi) + ghp : nullptr;
                }
                u64 a0[NPL], a1[NPL], h0[NPL], h1[NPL], c0[NPL], c1[NPL];
                long long t_start = 0;
                for (int spin = 0;; ++spin) {
                    bool good = true;
#pragma unroll
                    for (int q = 0; q < NPL; ++q) {
                        if (gaddr[q]) { a0[q] = ld_mail<RANKS>(gaddr[q] + ghp); a1[q] = ld_mail<RANKS>(gaddr[q] + ghp + 1); }
                        if (bh) { h0[q] = ld_gran(bh + 2 * (lane + q * WAVE)); h1[q] = ld_gran(bh + 2 * (lane + q * WAVE) + 1); }
                        if (ga2[q]) { c0[q] = ld_mail<RANKS>(ga2[q]); c1[q] = ld_mail<RANKS>(ga2[q] + 1); }
                    }
#pragma unroll
                    for (int q = 0; q < NPL; ++q) {
                        if (gaddr[q]) good = good && (unsigned)(a0[q] >> 32) == epoch && (unsigned)(a1[q] >> 32) == epoch;
                        if (bh) good = good && (unsigned)(h0[q] >> 32) == epoch && (unsigned)(h1[q] >> 32) == epoch;
                        if (ga2[q]) good = good && (unsigned)(c0[q] >> 32) == epoch && (unsigned)(c1[q] >> 32) == epoch;
                    }
                    if (__all(good)) break;
                    if (poll_bail<NPL>(spin, t_start, lane, R)) { ok = false; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    gz[q] = gaddr[q] ? __hiloint2double((int)(unsigned)a1[q], (int)(unsigned)a0[q]) : 0.0;
                    if (bw) {
                        const double hv = ga2[q] ? __hiloint2double((int)(unsigned)c1[q], (int)(unsigned)c0[q])
                                                 : __hiloint2double((int)(unsigned)h1[q], (int)(unsigned)h0[q]);
                        zhalo[((wv == 0) ? 0 : HSL) + lr + q * LSL] = hv;
                    }
                }
            }
            if (wv == rw) {
                if (g == 0) {       // the rank's record: the local records in workgroup order, then to every rank's mailbox
                    double d0, d1, t4 = 0.0;
                    if (G <= 8) { u64 v[1] = {0}; ok = poll_rec4<1>(slotsA, G, nullptr, nullptr, epoch, lane, R, v, d0, d1) && ok; t4 = sum_rec4<1>(v, G, lane); }
                    else        { u64 v[4] = {0, 0, 0, 0}; ok = poll_rec4<4>(slotsA, G, nullptr, nullptr, epoch, lane, R, v, d0, d1) && ok; t4 = sum_rec4<4>(v, G, lane); }
                    const double mine = __shfl(t4, lane & 6, WAVE);            // lane l: the total of value (l & 7) >> 1
                    if (lane < 8 * Sh.P) {
                        const u64 bits = (u64)__double_as_longlong(mine);
                        st_mail<RANKS>(Sh.mail[lane >> 3] + (size_t)SH_MAXREC * 2 + (size_t)par * 8 * REC4 + (size_t)Sh.rank * REC4 + (lane & 7),
                               ((u64)epoch << 32) | ((lane & 1) ? (bits >> 32) : (bits & 0xFFFFFFFFull)));
                    }
                }
                u64 v[1] = {0};
                long long t_start = 0;
                for (int spin = 0;; ++spin) {
                    bool good = true;
                    if (lane < REC4 * Sh.P) { v[0] = ld_mail<RANKS>(rankrec + lane); good = (unsigned)(v[0] >> 32) == epoch; }
                    if (__all(good)) break;
                    if (poll_bail<1>(spin, t_start, lane, R)) { ok = false; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                const double t4 = sum_rec4<1>(v, Sh.P, lane);                  // ranks in rank order: the same bits on every rank
                if (lane < 8 && !(lane & 1)) tot[lane >> 1] = t4;
            }
            if (!ok && lane == 0) tot[5] = 0.0;
            wg_barrier();
            if (tot[5] == 0.0) return;
            pap = tot[0]; rz = tot[1]; zz = tot[2]; rr0 = tot[3];
        } else if (G == 1) {
            const double t4 = sum_part4(part, W, lane);
            if constexpr (RPOLL) {                            // (a team of one has no poll window: behind the read of the partials, never in front)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) rt[RPOLL ? j : 0][q] = rl[j * HSL + lr + q * LSL];
                __builtin_amdgcn_sched_barrier(0);
            }
            pap = readlane_f64(t4, 0); rz = readlane_f64(t4, 8); zz = readlane_f64(t4, 16); rr0 = readlane_f64(t4, 24);
        } else {
            // Every wave fetches its share of the two boundary slices of z (2 NPL segments of 64 values, segment s -> wave s % W, two
            // at a time) into LDS; one of them also trades the team's records.
            constexpr int NSEG = 2 * NPL;
            const int rw = (W > NSEG) ? NSEG : ((W >= 3) ? 1 : 0);        // (a wave without a segment if there is one)
            bool ok = true;
            double t4 = 0.0;
            if (wv == rw) publish_rec4(slotsA, g, sum_part4(part, W, lane), epoch, lane);
            if constexpr (RPOLL) {                            // (behind the record's publication, in front of the polls)
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) rt[RPOLL ? j : 0][q] = rl[j * HSL + lr + q * LSL];
            }
            for (int s0 = wv; s0 < NSEG || (s0 == wv && wv == rw); s0 += 2 * W) {
                const int s1 = s0 + W;
                const u64 *b0 = nullptr, *b1 = nullptr;
                if (s0 < NSEG) b0 = bnd + ((((s0 < NPL) ? (size_t)gm * 2 + 1 : (size_t)gp * 2 + 0) * HS) + lane_b + (size_t)(s0 % NPL) * WAVE) * 2;
                if (s1 < NSEG) b1 = bnd + ((((s1 < NPL) ? (size_t)gm * 2 + 1 : (size_t)gp * 2 + 0) * HS) + lane_b + (size_t)(s1 % NPL) * WAVE) * 2;
                const bool recs = (wv == rw && s0 == wv);
                double z0 = 0.0, z1 = 0.0;
                if (G <= 8) {
                    u64 v[1] = {0};
                    ok = poll_rec4<1>(recs ? slotsA : nullptr, G, b0, b1, epoch, lane, R, v, z0, z1) && ok;
                    if (recs) t4 = sum_rec4<1>(v, G, lane);
                } else {
                    u64 v[4] = {0, 0, 0, 0};
                    ok = poll_rec4<4>(recs ? slotsA : nullptr, G, b0, b1, epoch, lane, R, v, z0, z1) && ok;
                    if (recs) t4 = sum_rec4<4>(v, G, lane);
                }
                if (b0 && lwok) zhalo[(size_t)s0 * LSL + lr] = z0;        // (segment s = side * NPL + q lives at [side][q * LSL + slot])
                if (b1 && lwok) zhalo[(size_t)s1 * LSL + lr] = z1;
                if (!ok) break;
            }
            if (wv == rw && lane < 8 && !(lane & 1)) tot[lane >> 1] = t4;
            if (!ok && lane == 0) tot[5] = 0.0;
#ifdef ELPH_WG_ARRIVE
            if (!ok && lane == 0 && blockIdx.x < 4096) g_wg_arrive[blockIdx.x * 4 + 3] = ((unsigned long long)(seq + 1) << 8) | (1ull << wv);   // iteration and wave of a poll that gave up
#endif
            wg_barrier();
            if (tot[5] == 0.0) return;
            pap = tot[0]; rz = tot[1]; zz = tot[2]; rr0 = tot[3];
        }
        STAMP(1);
        rho = rr0;                                            // r.r of the residual this iteration started from, summed from the vector
        const double alpha = FUSED ? uni(rr0 / pap) : rr0 / pap;
        if constexpr (FUSED) alpha_f = alpha;                 // :278-279 (rho = r.r)
        rr = rr0 + alpha * (alpha * zz - 2.0 * rz);
        // ---- x += alpha p, r -= alpha z (own slices) ----------------------------------------------------------------------------
        if constexpr (!FUSED) {
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const double zq = (SHARD && gaddr[q]) ? gz[q] : z[j][q];                           // (a shard's ghost rows: the owner's z)
                const double rn = rl[j * HSL + lr + q * LSL] - alpha * zq;                          // :285
                if (lwok) rl[j * HSL + lr + q * LSL] = rn;
                if (X_GLB) { if (lwok) xg[(size_t)(t0 + j) * N + sc[q]] = xr[X_REG ? j : 0][q] + alpha * p[j + 1][q]; }
                else if (X_REG) xr[X_REG ? j : 0][q] += alpha * p[j + 1][q];                       // :282
                else if (lwok) xl[j * HSL + lr + q * LSL] += alpha * p[j + 1][q];
            }
        if (G > 1 && (wv == 0 || wv == W - 1)) {              // the neighbouring workgroup's boundary slice of the new residual
            double *rh = rhalo + ((wv == 0) ? 0 : HSL);
            const double *zh = zhalo + ((wv == 0) ? 0 : HSL);
#pragma unroll
            for (int q = 0; q < NPL; ++q) if (lwok) rh[lr + q * LSL] = rh[lr + q * LSL] - alpha * zh[lr + q * LSL];
        }
        STAMP(3);
        }
        // FUSED: the same update waits for the stop test and beta (below) and takes the p-update along (WITHP: p = r' + beta p from the r'
        // just made; never in the honeycomb DPP form — a mirror lane's z is not the real lane's, its p is made from the real lane's r' in
        // LDS).  When the identity cancels — the scalars at hand tell — the direct sum and the second meeting come first, as in the sharded
        // solves, and the sum takes r' as the pass will make it (below); the pass itself stays ONE piece of straight-line code after the
        // stop test: with the update on two paths that join again, x sat in two register sets at once and the 4-slice shape spilled
        if (!(rr > 1e-3 * rr0)) {
            // the identity cancels: take r'.r' from the vector itself (second meeting of this iteration; every wave of the team is here)
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q)
                    if (own[q]) {
                        // (FUSED: r' is not in LDS yet — the same fma makes the same bits here as in the pass that will store them)
                        const double rn = RPOLL ? rt[RPOLL ? j : 0][q] - alpha * z[j][q] : (FUSED ? rl[j * HSL + lr + q * LSL] - alpha * z[j][q] : rl[j * HSL + lr + q * LSL]);
                        a += rn * rn;
                    }
            a = wave_sum_dpp(a);
            // (RPOLL holds r in registers from the poll window on: this rare branch makes its slot's address afresh, from the wave number read
            //  as a scalar — kept in a vector register across the loop it was the one register too many, 8 bytes of scratch)
            if (lane == 0) partF[RPOLL ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : wv] = a;
            wg_barrier();
            if constexpr (SHARD) {
                if (wv == 0) {
                    sh_publish<RANKS>(Sh, 0, g, G, wg_sum(partF, W, lane), epoch, lane);
                    const u64 *none[NPL];
#pragma unroll
                    for (int q = 0; q < NPL; ++q) none[q] = nullptr;
                    double t = 0.0, dummy[NPL];
                    const bool ok = sh_poll<NPL, RANKS>(Sh, true, 0, G, none, epoch, lane, R, t, dummy);
                    if (lane == 0) { tot[4] = t; if (!ok) tot[5] = 0.0; }
                }
                wg_barrier();
                if (tot[5] == 0.0) return;
                rr = tot[4];
            } else if (G == 1) {
                rr = wg_sum(partF, W, lane);
            } else {
                if (wv == 0) {
                    const double mine = wg_sum(partF, W, lane);
                    if (lane < 2) {
                        const u64 bits = (u64)__double_as_longlong(mine);
                        st_gran(slotsB + 2 * g + lane, ((u64)epoch << 32) | (lane ? (bits >> 32) : (bits & 0xFFFFFFFFull)));
                    }
                    u64 v = 0;
                    const bool ok = poll_records(slotsB, G, epoch, lane, R, v);
                    const int half = (int)(unsigned)v;
                    double t = 0.0;
                    for (int k = 0; k < G; ++k)
                        t += __hiloint2double(__builtin_amdgcn_readlane(half, 2 * k + 1), __builtin_amdgcn_readlane(half, 2 * k));
                    if (lane == 0) { tot[4] = t; if (!ok) tot[5] = 0.0; }
                }
                wg_barrier();
                if (tot[5] == 0.0) return;
                rr = tot[4];
            }
        }
        if constexpr (!FUSED) {
            wg_barrier();                                     // the new residual of every wave is in LDS: the neighbours' halo slices
            STAMP(4);
        }
        }
        STAMP(5);
        STAMP(6);
        // ---- stop test of iteration it = seq + 1 (IterativeSolvers.jl:286-295) ---------------------------------------------
        // eps = |r|/|b| < tol, kappa_min = max_j (2j / ln(2 eps0/eps_j))^2 > kappa_max, j = maxiter — a square root, two divisions and
        // a logarithm in f64 (~150 instructions in EVERY wave: half a mat-vec of this kernel).  Two comparisons screen them out
        // while no decision is near:  r.r well above (tol |b|)^2 rules out the first;  (2 eps0/eps)^2 = y outside [1/2, 2] means
        // |ln(2 eps0/eps)| > 0.34, which rules out the second while 2j < 0.34 sqrt(kappa_max).  Near a decision, on the last
        // iteration and with a residual history the exact arithmetic of the reference runs (eps, and kappa_min of THAT iteration:
        // an iteration stops on kappa only through its own term, the earlier ones did not stop).
        // (fixed_iters — measurement — takes the tolerance screen as passed: a solve would have stopped there; its iterations
        // cost what the iterations of a running solve cost.)
        const long long it = seq + 1;
        const bool fixed = R.fixed_iters > 0;
        int done = 0;
        const bool screened = !P.record_hist && it < (fixed ? R.fixed_iters : P.maxiter) && (fixed || rr > rr_far) &&
                              (rr + rr <= y_num || rr >= y_num + y_num) && (double)it < it_kappa;
        if (!screened) {
            eps = sqrt(rr) / normb;
            const double qq = 2.0 * (double)it / log(2.0 * eps0 / eps);
            const double val = qq * qq;
            kmin = (val > kmin) ? val : kmin;
            if (eps < P.tol) done = 1;
            else if (kmin > P.kmax) done = 2;
            else if (it >= P.maxiter) done = 3;
            if (fixed) done = (it >= R.fixed_iters) ? 3 : 0;
            if (g == 0 && wv == 0 && lane == 0 && P.record_hist) B.hist[(size_t)rhs * P.hist_stride + it] = eps;
        }
        STAMP(7);
        if constexpr (FUSED) {
            // the fused pass.  beta is made, and p is updated, whether or not this was the last iteration: past `done` nothing reads p
            // (x takes alpha p of the OLD p inside the pass), and a select per value would cost more than the update.  rho = rr0 here.
            // (RPOLL: only the two boundary slices of r' are stored here, in front of the barrier — they are all the neighbouring waves read;
            //  slices 1 .. T-2 are read by the wave itself, in the next mat-vec, and are stored behind the barrier and the halo reads, from
            //  the registers of rt.  No `lwok`: every lane of this form holds sites.)
            const double beta = uni(rr / rho);
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    const double rn = (RPOLL ? rt[RPOLL ? j : 0][q] : rl[j * HSL + lr + q * LSL]) - alpha_f * z[j][q];     // :285
                    if constexpr (RPOLL) { rt[RPOLL ? j : 0][q] = rn; if (j == 0 || j == T - 1) rl[j * HSL + lr + q * LSL] = rn; }
                    else if (lwok) rl[j * HSL + lr + q * LSL] = rn;
                    if (X_GLB) { if (lwok) xg[(size_t)(t0 + j) * N + sc[q]] = xr[X_REG ? j : 0][q] + alpha_f * p[j + 1][q]; }
                    else if (X_REG) xr[X_REG ? j : 0][q] += alpha_f * p[j + 1][q];                   // :282
                    else if (lwok) xl[j * HSL + lr + q * LSL] += alpha_f * p[j + 1][q];
                    if constexpr (!HC) p[j + 1][q] = rn + beta * p[j + 1][q];
                }
            if constexpr (HC) {
                // from the real lane's r' in LDS: a wave reads what it wrote itself, no barrier — but the COMPILER must not hand a mirror
                // lane, which stored nothing, the r it read from that slot before the real lane's store
                WAVE_LDS_ORDER();
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) p[j + 1][q] = rl[j * HSL + lr + q * LSL] + beta * p[j + 1][q];
            }
            if (G > 1 && (wv == 0 || wv == W - 1)) {          // the neighbouring workgroup's boundary slice of the new residual
                double *rh = rhalo + ((wv == 0) ? 0 : HSL);
                const double *zh = zhalo + ((wv == 0) ? 0 : HSL);
                if constexpr (SQ && !SSH && UNI && T == 4) {
                    // (4 slices per wave: the four reads at once and the results written in one group — left alone it is two serialised
                    //  read-wait-fma-write groups, the stores to rh are in the way of the reads behind them, while the other six waves
                    //  already wait at the barrier below.  No `lwok`: every lane of this form holds sites.)
                    double rhv[NPL], zhv[NPL];
#pragma unroll
                    for (int q = 0; q < NPL; ++q) { rhv[q] = rh[lr + q * LSL]; zhv[q] = zh[lr + q * LSL]; }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < NPL; ++q) rh[lr + q * LSL] = rhv[q] - alpha_f * zhv[q];
                } else {
#pragma unroll
                    for (int q = 0; q < NPL; ++q) if (lwok) rh[lr + q * LSL] = rh[lr + q * LSL] - alpha_f * zh[lr + q * LSL];
                }
            }
            STAMP(3);
        }
        if (done) {
            STAMP_OUT(it);
            TL(2);
            // (the store addresses are made here, from a laundered lane number: computed before the loop they sit in 2 registers per
            //  value for the whole solve — in a kernel that has none to spare: 10 -> 2 spilled registers at 4 slices per wave)
            int lane2 = lane;
            asm volatile("" : "+v"(lane2));
            // (FUSED: the first slice likewise, from the wave number read afresh as a scalar — one base address per slice would otherwise sit in
            //  vector registers for the whole solve; and the state record is read again below rather than kept)
            const int t0s = FUSED ? (g * W + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * T : t0;
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) {
                    const int s2 = SQ ? sq_patch_site(lane2, q) : (HC ? hc_site(lane2, q) : (S8 ? s8_site(lane2) : (GR ? grid_site(lane2, q, GGX, GGY) : (HG ? hgrid_site<NPL>(lane2, q, HLX, HLY) : lane2 + q * WAVE))));
                    if (HC ? hc_real(lane2) : (GR ? lane2 < GGX * GGY : (HG ? lane2 < (HLX / HgDim<NPL>::PX) * (HLY / HgDim<NPL>::PY) : (SQ || s2 < N)))) {
                        // (the residual stays on the chip: ldiv! judges a solution by its TRUE residual, Models.jl:150-160; a shard's
                        //  caller may want it)
                        if (SHARD) rg[(size_t)(t0 + j) * N + s2] = rl[j * HSL + lr + q * LSL];
                        if (!X_GLB) xg[(size_t)(t0s + j) * N + s2] = X_REG ? xr[X_REG ? j : 0][q] : xl[j * HSL + lr + q * LSL];
                    }
                }
            if (g == 0 && wv == 0 && lane == 0) {
                CgState o = FUSED ? ld_state(st2) : S;
                o.rho = rho; o.kmin = kmin; o.eps = eps; o.seq = it + 1; o.iters = it; o.done = done;
                st2[0] = o;
                st2[1] = o;
            }
            TL(3);
            return;
        }
        const double beta = rr / rho;
        rho = rr;
        if constexpr (FUSED) {
            wg_barrier();                                     // the new residual of every wave is in LDS: the neighbours' halo slices
            STAMP(4);
        }
        // ---- next direction on the two halo slices, and (sharded solves) on the own slices (p = r + beta p is pointwise) ----
        {
            const bool lx = (G > 1 && wv == 0), rx = (G > 1 && wv == W - 1);
            const double *sl = rall + ((size_t)((wv > 0) ? wv - 1 : W - 1) * T + (T - 1)) * HSL;    // last slice of the wave below
            const double *sr = rall + ((size_t)((wv < W - 1) ? wv + 1 : 0) * T + 0) * HSL;         // first slice of the wave above
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const double hl = lx ? rhalo[lr + q * LSL] : sl[lr + q * LSL];
                const double hr = rx ? rhalo[HSL + lr + q * LSL] : sr[lr + q * LSL];
                if constexpr (PH_LDS) {
                    const double n0 = hl + beta * PHALO(0, q), n1 = hr + beta * PHALO(1, q);
                    if (lwok) { PHALO(0, q) = n0; PHALO(1, q) = n1; }
                } else {
                    p[0][q] = hl + beta * p[0][q];
                    p[T + 1][q] = hr + beta * p[T + 1][q];
                }
            }
            if constexpr (RPOLL) {                            // the interior slices of r' (see the pass): behind the halo reads
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 1; j < T - 1; ++j)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) rl[j * HSL + lr + q * LSL] = rt[RPOLL ? j : 0][q];
            }
        }
        if constexpr (!FUSED) {
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int q = 0; q < NPL; ++q) p[j + 1][q] = rl[j * HSL + lr + q * LSL] + beta * p[j + 1][q];
        }
        STAMP(8);
    }
#undef EXPV
#undef PHALO
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

// ONE RECORD PER LAUNCH: which form, which team shape, how much LDS, resident or streaming — made once, by a pure function (plan_wg; a
// shard's: plan_shard) of what the handle knows (WgFacts) and what the caller and the environment ask (WgKnobs).  elph_wg_cg,
// elph_wg_usable, the sharded launches and the device-free probe elph_i_wg_plan_probe all read the same record; launch() maps it to
// the one instantiation of k_cg_wg that runs it.
struct WgFacts {
    int kind = 0, L = 0, npl = 0, lp_mc = 0;     // npl: ceil(N / 64), the lane program's sites per lane
    long long ndim = 0;
    bool fast = false, fast_capable = false, uniform = false;      // uniform: Holstein, one (cosh, sinh) on every bond (LatticeShape::hop_uniform)
    const LatticeShape *shape = nullptr;
    int dot_hi = 0, solo_chain = -1;
};
static WgFacts wg_facts(const elph_handle_s *h) {
    WgFacts F;
    F.kind = h->kind; F.L = (int)h->L; F.npl = h->npl; F.lp_mc = h->lp_mc; F.ndim = (long long)h->ndim;
    F.fast = h->fast; F.fast_capable = h->fast_capable; F.uniform = h->shape.hop_uniform; F.shape = &h->shape;
    F.dot_hi = h->dot_hi; F.solo_chain = h->solo_chain;
    return F;
}

// the batch, the measurement mode and the switches of DESIGN.md §9 — read once per plan, and per call: the tests switch them
struct WgKnobs {
    int nrhs = 1;
    long long fixed_iters = 0;     // > 0: a measurement of this kernel — no cost rule
    bool no_wg = false;            // ELPH_NO_WG=1: the streaming iteration
    bool no_dpp = false;           // ELPH_WG_NO_DPP=1: none of the register-exchange forms, the lane-program form instead
    bool always = false;           // ELPH_WG_ALWAYS=1: no cost rule
    int force_T = 0;               // ELPH_WG_T: the slices per wave (0: the rule of pick_shape)
    int wmax = 8;                  // ELPH_WG_W (experiments): cap on the waves per workgroup
};
static WgKnobs wg_knobs(int nrhs, long long fixed_iters) {
    auto on = [](const char *e) { return e && e[0] == '1'; };
    WgKnobs K;
    K.nrhs = nrhs; K.fixed_iters = fixed_iters;
    K.no_wg = on(getenv("ELPH_NO_WG")); K.no_dpp = on(getenv("ELPH_WG_NO_DPP")); K.always = on(getenv("ELPH_WG_ALWAYS"));
    const char *et = getenv("ELPH_WG_T"), *ew = getenv("ELPH_WG_W");
    K.force_T = et ? atoi(et) : 0;
    K.wmax = ew ? std::max(1, atoi(ew)) : 8;
    return K;
}

struct WgPlan {
    bool usable = false;           // a resident form and shape exist for this handle and batch
    Form form = LANE;
    int npl = 0, T = 0, W = 0, G = 0;      // npl: sites per lane of the KERNEL (honeycomb DPP form: 6; grid form: 4; honeycomb grid form: 2, 4, 8)
    bool ssh = false, uniform = false;
    size_t shm = 0;                // bytes of dynamic LDS: wg_layout's total
    int per_round = 0;             // right-hand sides one round of the grid holds: one team per G CUs of an XCD
    double resident_us = 0.0, streaming_us = 0.0;      // per iteration: one round of this plan | the two-kernel iteration of the whole batch
    bool resident = false;         // usable, and the cost rule (or a measurement, or ELPH_WG_ALWAYS) takes it
};

// Which form a lattice takes.  for_shard: the slab of a sharded solve, its rows closed into a ring by the caller — a periodic rectangle.
//  SQ16   the 16 x 16 square lattice in the reference's colouring (elph_recognise_lattice), Holstein or SSH
//  HC12   Holstein with uniform hopping on 12 x 12 honeycomb cells
//  S8     Holstein with uniform hopping on the 8 x 8 square lattice
//  TGRID  Holstein with uniform hopping on an even-L triangular lattice of at most 16 x 16 sites (the recognised shape has a grid of
//         lanes): the GRID layout with the two diagonal colours (pgrid::Tri<2, 2>)
//  GRID   Holstein with uniform hopping on a periodic LX x LY square lattice whose 2 x 2 patches fit the lanes of a wave
//         (LatticeShape::small_square).  An ordinary solve takes it for the sizes WITHOUT a DPP form of their own (not 16 x 16, not 8 x 8);
//         a sharded solve for every size — the DPP forms know no shards
//  HGRID  Holstein with uniform hopping on a periodic honeycomb lattice whose cells fit a grid of lanes (LatticeShape::hgrid_regs: 2, 4 or
//         8 registers per lane = 1, 2 x 1 or 2 x 2 cells; 12 x 12 has a DPP form of its own — which knows no shards)
//  LANE   everything else with a 4-colour lane program
// *npl: the kernel's sites per lane.
static Form pick_form(const WgFacts &F, const WgKnobs &K, bool for_shard, int *npl) {
    const LatticeShape &S = *F.shape;
    const bool hol_uni = F.kind == ELPH_MODEL_HOLSTEIN && F.uniform && !K.no_dpp;
    const bool grid = hol_uni && S.small_square() && S.GX * S.GY >= 1 && S.GX * S.GY <= 64;
    Form f = LANE;
    if (for_shard) {
        // (measured, profiles/r04/shard_ring_grid_forms_ab.log: the GRID form pays from three sites per lane of the lane program — a
        //  slab of up to 128 sites is two LDS values per lane and colour, cheaper than four registers on half the lanes: config C over 4 / 8
        //  ranks 5.3 / 6.0 us in the lane program against 6.5 / 7.2; the HGRID form with 8 registers per lane spills in the shard's
        //  kernel: config D on one rank 16.6 against 9.6 us)
        if (grid && F.npl >= 3) f = GRID;
        else if (hol_uni && S.hgrid_regs() > 0 && S.hgrid_regs() != 8) f = HGRID;
    } else {
        if (S.dpp() == 2 && !K.no_dpp) f = SQ16;
        else if (hol_uni && S.hc12()) f = HC12;
        else if (hol_uni && S.dpp() == 1) f = S8;
        else if (hol_uni && S.kind == LatticeShape::TRIANGULAR && S.GX > 0) f = TGRID;
        else if (grid && S.dpp() == 0) f = GRID;
        else if (hol_uni && S.hgrid_regs() > 0) f = HGRID;
    }
    *npl = f == HC12 ? HC_NPL : ((f == GRID || f == TGRID) ? 4 : (f == HGRID ? S.hgrid_regs() : F.npl));
    return f;
}

static int largest_divisor_le8(int n, int cap = 8) { for (int w = std::min(cap, n); w >= 1; --w) if (n % w == 0) return w; return 1; }

// T slices per wave: what the register file takes at two waves per SIMD — lane-program form 2 for site phonons with <= 4 sites
// per lane, else 1; DPP form 2 (config C: 5.8 us per iteration, 24 right-hand sides fill the chip), or 4 for batches that the
// 2-slice shape cannot hold in one round (6.8 us per iteration, but 48 right-hand sides per round: 14 vs 7.3 M mat-vecs/s);
// W = the largest divisor of Ltau / T that is <= 8 waves; G = workgroups per right-hand side (<= 32: the 2G record granules of
// a meeting are polled by one wave instruction).  Fills form, npl, T, W, G, shm of *out.
static bool pick_shape(const WgFacts &F, const WgKnobs &K, WgPlan *out) {
    const int L = F.L, forceT = K.force_T, nrhs = K.nrhs;
    int npl = 0;
    const Form form = pick_form(F, K, false, &npl);
    const bool ssh = F.kind == ELPH_MODEL_SSH, sq = form == SQ16, hc = form == HC12, s8 = form == S8, gr = form == GRID || form == TGRID, hg = form == HGRID;
    const bool lane = !sq && !hc && !gr && !hg;            // (the lane-program form and, where the rules below do not name it, the 8 x 8 DPP form)
    if (F.lp_mc != 4 && form != TGRID) return false;       // (a six-colour lattice has no lane-program form here: only the triangular grid form)
    if (lane && F.npl > 5) return false;                   // (the lane-program form carries at most 320 sites; plan_wg lets larger honeycomb lattices through for the grid form only)
    auto take = [&](int T, int W, int G) {
        const size_t shm = wg_layout(form, npl, T, ssh, W).total * sizeof(double);
        if (shm > 160 * 1024) return false;
        out->form = form; out->npl = npl; out->T = T; out->W = W; out->G = G; out->shm = shm;
        return true;
    };
    // one site per lane (the 8 x 8 lattice: config B): the whole time axis fits ONE workgroup — up to 8 waves of 4, 5 or 8 slices — and
    // a team of one needs no records, no boundary granules, no polls: its meeting is an LDS reduction and a barrier, and a round holds
    // 256 right-hand sides.  Its iteration is longer (config B: 6.3 us at 5 slices per wave against 3.5 at 2 with teams of four), so it
    // is the shape of batches beyond one round of 2 slices per wave (B: 64): 256 right-hand sides 14.0 -> 6.4 us = 36 -> 80 M mat-vecs/s
    bool big_batch = true;
    if (!forceT && L % 2 == 0) {
        const int G2 = (L / 2) / largest_divisor_le8(L / 2);
        big_batch = G2 <= 32 && nrhs > 8 * (32 / G2);
    }
    // (the 8 x 8 DPP form: the team of one is the fastest shape at every batch size — 2.04 us per iteration for one right-hand side, 2.3 us
    //  for 256 = 222 M mat-vecs/s — its sweeps are a few dozen register moves)
    if (!ssh && lane && F.npl == 1 && (big_batch || s8)) {
        const int one[3] = {4, 5, 8};
        for (int T : one) {
            if ((forceT && T != forceT) || L % T || L / T > 8 || L / T < 2) continue;
            if (take(T, L / T, 1)) return true;
        }
    }
    const int cand[4] = {4, 3, 2, 1};
    for (int T : cand) {
        if (forceT && T != forceT) continue;
        if (T == 3) {
            // honeycomb form only: 48 right-hand sides per round instead of 24 at 2 slices per wave, but 8.6 us per iteration against 5.7
            // (the kernel still spills 42 registers: six sites per lane x three slices is more than the register file and the LDS hold
            // next to each other, even with x in memory) — taken when the rounds it saves outweigh that: 25-48 and everything from 73
            // right-hand sides on
            if (!hc || L % 3 || L % 2) continue;
            if (forceT != 3) {
                const int G2 = (L / 2) / largest_divisor_le8(L / 2), G3 = (L / 3) / largest_divisor_le8(L / 3);
                if (G2 > 32 || G3 > 32) continue;
                const int r2 = 8 * (32 / G2), r3 = 8 * (32 / G3);
                if (nrhs <= r2 || 8.6 * ((nrhs + r3 - 1) / r3) >= 5.7 * ((nrhs + r2 - 1) / r2)) continue;
            }
        }
        if (T == 4) {
            if (!(sq || gr) || !F.uniform || ssh) continue;
            if (forceT != 4) {                           // only when 2 slices per wave would need a second round: 8 XCDs x (32 CUs / G2) teams
                if (L % 2) continue;
                const int G2 = (L / 2) / largest_divisor_le8(L / 2);
                if (G2 > 32 || nrhs <= 8 * (32 / G2)) continue;
            }
        }
        if (gr && T == 3) continue;
        if (hg && T > 2) continue;
        if (T == 2 && !lane && forceT != 2) {
            // DPP form: a batch that one round of 1 slice per wave holds (config C: up to 8 right-hand sides, one team of 20 workgroups per
            // XCD) runs that shape — with ONE meeting per iteration the shorter mat-vec wins over the larger team: 3.47 against 4.00 us
            // per iteration for one right-hand side (round 2, two meetings: the other way round)
            const int G1 = L / largest_divisor_le8(L);
            if (G1 <= 32 && L / G1 >= 2 && nrhs <= 8 * (32 / G1)) continue;
        }
        if (T == 2 && lane && ((ssh && F.npl > 4) || F.npl > 5 || (!ssh && F.npl >= 4 && !F.uniform))) continue;
        if (T == 2 && lane && (F.npl == 5 || ssh) && forceT != 2) {
            // 5 sites per lane (honeycomb L = 12) and bond phonons (three table sets per wave: 41 registers spill): 2 slices per wave are
            // slower per iteration (D: 10.0 vs 9.3 us; E: 12.9 vs 9.5 us) but hold more right-hand sides per round (D: 24 instead
            // of 16; E: 24 instead of 8) — taken once a batch exceeds the round of 1 slice per wave
            const int G1 = L / largest_divisor_le8(L);
            if (G1 <= 32 && nrhs <= 8 * (32 / G1)) continue;
        }
        if (L % T) continue;
        const int Wt = L / T, W = largest_divisor_le8(Wt, K.wmax), G = Wt / W;
        if (G > 32) continue;
        if (G > 1 && W < 2) continue;                    // (a wave polls at most ONE neighbouring workgroup's boundary slice)
        if (take(T, W, G)) return true;
    }
    return false;
}

// ---- the cost model behind the choice of form: ONE table, every entry with the measurement it was fitted to -----------------------
// us per iteration of ONE round of the resident kernel (a round holds 8 x floor(32 / G) right-hand sides: one team per G CUs of an XCD)
//     t = a + g * G + s * T * (sites per lane / 4 where the form scales with them)
// and of the two-kernel streaming iteration (HBM-bound, linear in the batch).  Fitted on MI355X.  The rule only has to order the two
// forms: a 20 % error in an entry moves a crossover by a few right-hand sides.
struct WgCost { Form form; bool ssh; double a, g, s; const char *measured; };
static const WgCost wg_cost_table[] = {
    {LANE,  false, 2.00, 0.12, 0.50, "profiles/r02/time_forms.log: configs B, C, D, E at 1-2 slices per wave; x sites per lane; + 3.9 for SSH at 2 slices, 0.85 T per slice from 4"},
    {SQ16,  false, 2.66, 0.01, 0.62, "profiles/r03/time_forms.log: 3.5 / 4.0 / 5.2 us at 1 / 2 / 4 slices per wave"},
    {SQ16,  true,  2.50, 0.00, 1.30, "profiles/r03/time_forms_E_ssh_dpp.log: 3.8 / 5.1 us at 1 / 2 slices"},
    {HC12,  false, 2.10, 0.00, 1.70, "profiles/r03/time_forms_D_honeycomb_dpp.log: 3.8 / 5.5 us at 1 / 2 slices; 8.6 us at 3 (time_forms_D_three_slices_per_wave.log)"},
    {S8,    false, 2.30, 0.00, 0.00, "profiles/r03/time_wg_B_8x8_dpp_form.log: team of one, 2.04-2.3 us whatever the batch"},
    {GRID,  false, 2.90, 0.01, 1.35, "profiles/r04/grid_form_even_L_square_lattices.log: L = 12: 4.3 / 5.6 / 10.0 us at 1 / 2 / 4 slices; L = 14, 10: 3.6-4.0 at 1"},
    {TGRID, false, 3.20, 0.00, 2.20, "profiles/r04/tgrid_triangular_resident.log: L = 16: 4.9 / 6.7 / 12.4 us at 1 / 2 / 4 slices per wave (4: 69 doubles spilled)"},
    {HGRID, false, 2.30, 0.01, 1.10, "profiles/r04/hgrid_form_honeycomb_lattices.log: L = 6: 2.5 us (2 registers per lane), L = 10: 3.3-3.8 (4), L = 16: 4.5-5.8 (8); x sites per lane / 4"},
};
static const double wg_streaming_cost[3] = {10.0, 0.56, 0.02};   // us: launch floor + nrhs x (0.56 x Ndim / 40960 [x 1.1 for SSH] + 0.02) — profiles/r03/time_forms.log (C: 37 us at 64, 128 at 256)

// the entry of a form; bond phonons take the form's SSH entry where it has one (the lane program prices them by a term of its own)
static const WgCost &wg_cost(Form form, bool ssh) {
    const WgCost *hol = nullptr;
    for (const WgCost &c : wg_cost_table) {
        if (c.form == form && c.ssh == ssh) return c;
        if (c.form == form && !c.ssh) hol = &c;
    }
    return hol ? *hol : wg_cost_table[0];
}
static double resident_iteration_us(const WgFacts &F, const WgPlan &P) {
    const WgCost &c = wg_cost(P.form, P.ssh);
    switch (P.form) {
        case S8: return c.a;
        case HC12: return (P.T == 3) ? 8.6 : c.a + c.s * P.T;
        case SQ16: return P.ssh ? c.a + c.s * P.T : c.a + c.g * P.G + c.s * P.T;
        case HGRID: return c.a + c.g * P.G + c.s * P.T * (P.npl / 4.0);
        case GRID: case TGRID: return c.a + c.g * P.G + c.s * P.T;
        case LANE: break;
    }
    return c.a + c.g * P.G + (P.T >= 4 ? 0.85 : c.s) * P.T * F.npl + ((P.ssh && P.T == 2) ? 3.9 : 0.0);
}
static double streaming_iteration_us(const WgFacts &F, int nrhs) {
    return wg_streaming_cost[0] + nrhs * (wg_streaming_cost[1] * (double)F.ndim / 40960.0 * (F.kind == ELPH_MODEL_SSH ? 1.1 : 1.0) + wg_streaming_cost[2]);
}

// The plan of an un-sharded solve.  Which form is faster for THIS batch is a deterministic rule (never a timing at run time — which form
// runs decides the last bits of a solution) from ONE table of measured constants, wg_cost_table above.
static WgPlan plan_wg(const WgFacts &F, const WgKnobs &K) {
    WgPlan P;
    P.ssh = F.kind == ELPH_MODEL_SSH; P.uniform = F.uniform;
    const LatticeShape &S = *F.shape;
    const bool hol = F.kind == ELPH_MODEL_HOLSTEIN;
    const bool tri_grid = hol && S.kind == LatticeShape::TRIANGULAR && S.GX > 0;      // (a six-colour lattice, but its resident form needs no lane program)
    // (npl > 5: the lane-program form's limit — 320 sites; the honeycomb grid form carries up to 512 in one wave)
    if (K.no_wg || !F.fast || (F.lp_mc != 4 && !tri_grid) || (F.npl > 5 && !(S.honeycomb() && !S.hc12() && hol)) || F.dot_hi != 0 || F.solo_chain >= 0) return P;
    if (!pick_shape(F, K, &P)) return P;
    P.usable = true;
    P.per_round = 8 * std::max(1, 32 / P.G);
    P.resident_us = resident_iteration_us(F, P);
    P.streaming_us = streaming_iteration_us(F, K.nrhs);
    const double rounds = (double)((K.nrhs + P.per_round - 1) / P.per_round);
    P.resident = K.fixed_iters > 0 || K.always || !(rounds * P.resident_us > P.streaming_us);
    return P;
}

// One rank's plan of a solve over `world` ranks: one slice per wave on every rank (slab sizes differ between ranks; the team shape must
// not: elph_shard_shape).  A slab whose rows the caller closed into a ring (a periodic rectangle in the reference's colouring: sharded.py,
// ring=True) runs a register-exchange form — the own rows of z = M^T M p do not see the ring bond (it lies beyond the ghost rows'
// dependency closure).  A sharded solve has no streaming iteration to compare with: its plan is resident.
static int plan_shard(const WgFacts &F, const WgKnobs &K, int world, WgPlan *out) {
    WgPlan P;
    P.ssh = F.kind == ELPH_MODEL_SSH; P.uniform = F.uniform;
    P.form = pick_form(F, K, true, &P.npl);
    if (P.form == LANE && (!F.fast_capable || F.lp_mc != 4 || F.npl > 5)) {
        elph_set_error("sharded solve: the slab needs a 4-colour lane program and <= 320 sites (N = %lld)", F.ndim / std::max(F.L, 1));
        return ELPH_E_UNSUPPORTED;
    }
    RC(elph_shard_shape(F.L, world, &P.W, &P.G, nullptr, nullptr));
    P.T = 1;
    P.shm = wg_layout(P.form, P.npl, P.T, P.ssh, P.W).total * sizeof(double);
    P.per_round = 1;
    P.usable = P.resident = true;
    *out = P;
    return ELPH_OK;
}

// ---- the launch table: every instantiation of k_cg_wg, named once ------------------------------------------------------------------
// PLAIN: an un-sharded solve; SHARD: one rank of a solve over several GPUs; RANKS: several ranks of a sharded solve in one launch
enum Variant { PLAIN, SHARD, RANKS };
typedef void (*WgKernel)(CgBufs, ModelDev, WgCtl, ShardCtl);
struct WgEntry { Variant v; int form, npl, T; bool ssh, uni, x0z; WgKernel fn; };
#define K(V, FORM, NPL, T, SSH, UNI, X0Z) {V, FORM, NPL, T, SSH, UNI, X0Z, k_cg_wg<NPL, T, SSH, UNI, FORM, (V) != PLAIN, X0Z, (V) == RANKS>}
#define K_UNI(V, FORM, NPL, T) K(V, FORM, NPL, T, false, true, false), K(V, FORM, NPL, T, false, false, false)      // Holstein: uniform | per-bond hopping
#define K_SSH(V, FORM, NPL, T) K(V, FORM, NPL, T, true, false, false)
#define K_HOL(V, FORM, NPL, T) K(V, FORM, NPL, T, false, true, false)                                                // the forms of uniform hopping
static const WgEntry wg_kernels[] = {
    // lane program: 1 or 2 slices per wave up to five sites per lane (bond phonons: 2 slices up to four) ...
    K_UNI(PLAIN, LANE, 1, 1), K_UNI(PLAIN, LANE, 2, 1), K_UNI(PLAIN, LANE, 3, 1), K_UNI(PLAIN, LANE, 4, 1), K_UNI(PLAIN, LANE, 5, 1),
    K_UNI(PLAIN, LANE, 1, 2), K_UNI(PLAIN, LANE, 2, 2), K_UNI(PLAIN, LANE, 3, 2), K_UNI(PLAIN, LANE, 4, 2), K_UNI(PLAIN, LANE, 5, 2),
    K_SSH(PLAIN, LANE, 1, 1), K_SSH(PLAIN, LANE, 2, 1), K_SSH(PLAIN, LANE, 3, 1), K_SSH(PLAIN, LANE, 4, 1), K_SSH(PLAIN, LANE, 5, 1),
    K_SSH(PLAIN, LANE, 1, 2), K_SSH(PLAIN, LANE, 2, 2), K_SSH(PLAIN, LANE, 3, 2), K_SSH(PLAIN, LANE, 4, 2),
    // ... and one site per lane in a team of one: 4, 5 or 8 slices per wave
    K_UNI(PLAIN, LANE, 1, 4), K_UNI(PLAIN, LANE, 1, 5), K_UNI(PLAIN, LANE, 1, 8),
    // 16 x 16 DPP form: uniform hopping up to 4 slices per wave (with the variant that does not read x0 = 0), per-site hopping and bond phonons up to 2
    K_UNI(PLAIN, SQ16, 4, 1), K_UNI(PLAIN, SQ16, 4, 2), K_HOL(PLAIN, SQ16, 4, 4), K(PLAIN, SQ16, 4, 4, false, true, true),
    K_SSH(PLAIN, SQ16, 4, 1), K_SSH(PLAIN, SQ16, 4, 2),
    K_HOL(PLAIN, HC12, HC_NPL, 1), K_HOL(PLAIN, HC12, HC_NPL, 2), K_HOL(PLAIN, HC12, HC_NPL, 3),
    K_HOL(PLAIN, S8, 1, 1), K_HOL(PLAIN, S8, 1, 2), K_HOL(PLAIN, S8, 1, 4), K_HOL(PLAIN, S8, 1, 5), K_HOL(PLAIN, S8, 1, 8),
    K_HOL(PLAIN, GRID, 4, 1), K_HOL(PLAIN, GRID, 4, 2), K_HOL(PLAIN, GRID, 4, 4),
    K_HOL(PLAIN, TGRID, 4, 1), K_HOL(PLAIN, TGRID, 4, 2), K_HOL(PLAIN, TGRID, 4, 4),
    K_HOL(PLAIN, HGRID, 2, 1), K_HOL(PLAIN, HGRID, 4, 1), K_HOL(PLAIN, HGRID, 8, 1), K_HOL(PLAIN, HGRID, 2, 2), K_HOL(PLAIN, HGRID, 4, 2), K_HOL(PLAIN, HGRID, 8, 2),
    // one rank of a sharded solve: one slice per wave; the slab in the lane program, or — closed into a ring — in the GRID or HGRID form
    K_UNI(SHARD, LANE, 1, 1), K_UNI(SHARD, LANE, 2, 1), K_UNI(SHARD, LANE, 3, 1), K_UNI(SHARD, LANE, 4, 1), K_UNI(SHARD, LANE, 5, 1),
    K_SSH(SHARD, LANE, 1, 1), K_SSH(SHARD, LANE, 2, 1), K_SSH(SHARD, LANE, 3, 1), K_SSH(SHARD, LANE, 4, 1), K_SSH(SHARD, LANE, 5, 1),
    K_HOL(SHARD, GRID, 4, 1), K_HOL(SHARD, HGRID, 2, 1), K_HOL(SHARD, HGRID, 4, 1), K_HOL(SHARD, HGRID, 8, 1),
    // the ranks of one device in one launch: site phonons, lane program or GRID form
    K_UNI(RANKS, LANE, 1, 1), K_UNI(RANKS, LANE, 2, 1), K_UNI(RANKS, LANE, 3, 1), K_UNI(RANKS, LANE, 4, 1), K_UNI(RANKS, LANE, 5, 1),
    K_HOL(RANKS, GRID, 4, 1),
};
#undef K_HOL
#undef K_SSH
#undef K_UNI
#undef K

// (x0_zero is a licence, not a demand: a plan without a kernel that skips reading x0 runs the one that reads it)
static const WgEntry *find_kernel(const WgPlan &P, Variant v, bool x0_zero) {
    const WgEntry *reads_x0 = nullptr;
    for (const WgEntry &k : wg_kernels) {
        if (k.v != v || k.form != P.form || k.npl != P.npl || k.T != P.T || k.ssh != P.ssh || k.uni != P.uniform) continue;
        if (k.x0z == x0_zero) return &k;
        if (!k.x0z) reads_x0 = &k;
    }
    return reads_x0;
}

static int launch(const WgPlan &P, Variant v, bool x0_zero, dim3 grid, hipStream_t stream, const CgBufs &B, const ModelDev &m, const WgCtl &R,
                  const ShardCtl &Sh = ShardCtl()) {
    static const char *const vname[] = {"", " (shard)", " (ranks)"};
    const WgEntry *k = find_kernel(P, v, x0_zero);
    if (!k) {
        elph_set_error("k_cg_wg%s: no kernel for form %d with %d sites per lane, %d slices per wave, ssh %d, uniform %d", vname[v], (int)P.form, P.npl, P.T, (int)P.ssh, (int)P.uniform);
        return ELPH_E_STATE;
    }
    hipError_t e = hipFuncSetAttribute((const void *)k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.shm);
    if (e == hipSuccess) { hipLaunchKernelGGL(k->fn, grid, dim3(P.W * WAVE), P.shm, stream, B, m, R, Sh); e = hipGetLastError(); }
    if (e != hipSuccess) { elph_set_error("launch k_cg_wg%s failed: %s", vname[v], hipGetErrorString(e)); return ELPH_E_HIP; }
    return ELPH_OK;
}

}  // namespace wg

// Whether the workgroup-resident kernel can run this handle's un-preconditioned solves (and with which shape).
// How many workgroups of the resident kernels may a launch count on being resident AT ONCE on this handle's device?  Their teams spin on
// one another's records: a workgroup that is not resident is waited for until the time-out.  One workgroup per CU (the kernels run at 256
// registers x 8 waves, or need most of the LDS), a sixteenth of the CUs left to whatever else the device runs: 240 on a whole MI355X
// (256 CUs), proportionally fewer on a partitioned or CU-masked device (CPX: 32 CUs -> 30).  Queried once per device.
int elph_i_resident_wg_limit(const elph_handle_s *h) {
    static std::atomic<int> cache[64];      // (0: not asked yet; two threads that ask at once store the same answer)
    const int d = (h && h->device >= 0 && h->device < 64) ? h->device : 0;
    int lim = cache[d].load(std::memory_order_relaxed);
    if (lim <= 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || cus <= 0) cus = 256;
        lim = std::max(1, cus - cus / 16);
        cache[d].store(lim, std::memory_order_relaxed);
    }
    return lim;
}

// a view of the plan: does a resident form exist for this handle and batch, and with which team shape (not: does the cost rule take it)
bool elph_wg_usable(const elph_handle_s *h, int *T, int *W, int *G, int nrhs) {
    const wg::WgPlan P = wg::plan_wg(wg::wg_facts(h), wg::wg_knobs(nrhs, 0));
    if (!P.usable) return false;
    if (T) *T = P.T;
    if (W) *W = P.W;
    if (G) *G = P.G;
    return true;
}

// The plan of a handle that need not own a device (elph_bench_wg_plan): world = 0 the un-sharded solve of nrhs right-hand sides, world > 0
// one rank of a solve over that many.  out[9]: usable, form, sites per lane, T, W, G, bytes of LDS, resident, whether the launch table
// holds the plan's kernel.
void elph_i_wg_plan_probe(const elph_handle_s *h, int nrhs, int world, int *out) {
    const wg::WgFacts F = wg::wg_facts(h);
    const wg::WgKnobs K = wg::wg_knobs(nrhs, 0);
    wg::WgPlan P;
    if (world > 0) { if (wg::plan_shard(F, K, world, &P) != ELPH_OK) P = wg::WgPlan(); }
    else P = wg::plan_wg(F, K);
    const bool has = P.usable && wg::find_kernel(P, world > 0 ? wg::SHARD : wg::PLAIN, false) != nullptr;
    const int v[9] = {P.usable, (int)P.form, P.npl, P.T, P.W, P.G, (int)P.shm, P.resident, has};
    std::copy(v, v + 9, out);
}

// The operational knobs of every resident kernel (cg_wg.hip, pcg_wg.hip, slabs.hip, shard.hip), read per call:
// ELPH_WG_TIMEOUT_MS, the wait bound of a team (dflt: the caller's default when it is not set) ...
long long elph_wg_timeout_ms(long long dflt) {
    const char *e = getenv("ELPH_WG_TIMEOUT_MS");
    return e ? atoll(e) : dflt;
}
// ... ELPH_WG_COOLDOWN, the solves that run streaming after a time-out (default 16) ...
int elph_wg_cooldown() {
    const char *e = getenv("ELPH_WG_COOLDOWN");
    return e ? std::max(1, atoi(e)) : 16;
}
// ... and the tests' ELPH_SLABS_TEST_TIMEOUT: its first character, 0 when it is not set
char elph_slabs_test_timeout() {
    const char *e = getenv("ELPH_SLABS_TEST_TIMEOUT");
    return e ? e[0] : 0;
}

// A team timed out on an earlier solve (the GPU was shared with something that held its CUs): the handle runs the streaming iteration
// for the next ELPH_WG_COOLDOWN solves (default 16), then tries the resident kernels again with a cleared abort word.  One step per
// solve that WOULD have taken a resident kernel — called by both of them (elph_wg_cg, elph_pcg_wg), so a handle that only ever runs
// preconditioned solves recovers too.
int elph_wg_cooldown_step(elph_handle_s *h) {
    ResidentState &S = h->res;
    if (!S.cooling() || --S.cooldown > 0) return ELPH_OK;
    if (S.d_res && S.abort_off) HIPCHK(hipMemsetAsync(static_cast<char *>(S.d_res) + S.abort_off, 0, sizeof(int), h->stream));
    return ELPH_OK;
}

// after the stream has drained: did a team give up?  Reads the abort word and nothing else — what a time-out means is the caller's.
int elph_wg_aborted(const elph_handle_s *h, bool *aborted) {
    *aborted = false;
    const ResidentState &S = h->res;
    if (!S.d_res || S.abort_off == 0) return ELPH_OK;
    int ab = 0;
    HIPCHK(hipMemcpy(&ab, static_cast<const char *>(S.d_res) + S.abort_off, sizeof(int), hipMemcpyDeviceToHost));
    *aborted = ab != 0;
    return ELPH_OK;
}

// A resident launch of this handle timed out and its solve goes to the streaming iteration: the ONLY writer of that record.
void elph_wg_timed_out(elph_handle_s *h) {
    ResidentState &S = h->res;
    S.cooldown = elph_wg_cooldown();
    ++S.fallbacks;
    elph_set_error("workgroup-resident CG timed out waiting for its team (T=%d W=%d G=%d); falling back to the two-kernel iteration", S.T, S.W, S.G);
}

// The control block of one resident launch (elph_internal.h: ResidentState).  Tags: a range of (iterations + 2) values per launch; the
// block is zeroed only when it is (re)allocated or the 32-bit range wraps — or for every launch that numbers from 0 (WG_TAGS_RESTART).
// The abort word sits at the END of the allocation (its place must not move with the batch size).
int elph_wg_ctl(elph_handle_s *h, size_t n_rec, size_t n_extra, unsigned long long span, long long timeout_ms, WgTags tags, wg::WgCtl *R) {
    ResidentState &S = h->res;
    const size_t need = (n_rec + n_extra) * sizeof(wg::u64) + 64;
    bool zero = tags == WG_TAGS_RESTART || (unsigned long long)S.next_tag + span >= 0xFFFFFFFFull;
    if (need > S.cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (S.d_res) HIPCHK(hipFree(S.d_res));
        S.d_res = nullptr;
        S.cap = 0;
        HIPCHK(hipMalloc(&S.d_res, need));
        S.cap = need;
        zero = true;
    }
    if (zero) { HIPCHK(hipMemsetAsync(S.d_res, 0, S.cap, h->stream)); S.next_tag = 0; }
    S.abort_off = S.cap - 64;
    *R = wg::WgCtl{};
    R->slots = static_cast<wg::u64 *>(S.d_res);
    R->bnd = nullptr;
    R->abort = reinterpret_cast<int *>(static_cast<char *>(S.d_res) + S.abort_off);
    R->epoch0 = S.next_tag;
    if (tags == WG_TAGS_RUNNING) S.next_tag += (unsigned)span;
    R->timeout_ticks = timeout_ms * 100000LL;      // wall_clock64 runs at 100 MHz
    return ELPH_OK;
}

// Runs the whole un-preconditioned CG for rhs [0, nrhs) after elph_launch_cg_init (fixed_iters > 0: exactly that many
// iterations without stop test — measurement).  *ran = false: not applicable, nothing was launched.
// A team that timed out shows in the abort word (elph_wg_aborted): the caller restores x0_save, re-initialises and runs the two-kernel path.
int elph_wg_cg(elph_handle_s *h, const CgBufs &B, int nrhs, long long fixed_iters, bool x0_zero, double *x0_save, bool *ran) {
    *ran = false;
    if (B.params.use_prec) return ELPH_OK;
    if (h->res.cooling()) return ELPH_OK;               // (after a time-out: elph_wg_cooldown_step, run_cg)
    const wg::WgPlan P = wg::plan_wg(wg::wg_facts(h), wg::wg_knobs(nrhs, fixed_iters));
    if (!P.resident) return ELPH_OK;
    const ModelDev m = elph_model_dev(h);
    const size_t HS = (size_t)P.npl * WAVE;
    const size_t n_slots = 2 * (size_t)nrhs * wg::SLOTS_PER_RHS, n_bnd = (P.G > 1) ? 2 * (size_t)nrhs * P.G * 2 * HS * 2 : 0;      // (x 2: by the parity of the iteration)
    // (2 s: a team at the dispatch frontier of an oversubscribed grid waits for whole solves of the resident ones — tens of ms for a
    //  batch of hundreds of right-hand sides; a measurement launch of thousands of fixed iterations gets its own duration on top)
    wg::WgCtl R;
    RC(elph_wg_ctl(h, n_slots, n_bnd, elph_wg_tag_span(B.params, fixed_iters), elph_wg_timeout_ms(2000) + (fixed_iters > 0 ? fixed_iters / 10 : 0),
                   WG_TAGS_RUNNING, &R));
    R.bnd = R.slots + n_slots;
    R.G = P.G; R.W = P.W;
    R.fixed_iters = fixed_iters;
    R.x0_zero = x0_zero ? 1 : 0;           // (x0 = 0 known: the 4-slice DPP shape has an instantiation that does not read it)
    if (x0_save)                // the caller's initial guess survives for the fallback (run_cg: in work.zp, unused by an un-preconditioned solve)
        HIPCHK(hipMemcpyAsync(x0_save, h->work.x, (size_t)nrhs * (size_t)h->ndim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    const dim3 grid((unsigned)(8 * ((nrhs + 7) / 8) * P.G));       // one solve per workgroup: every right-hand side has its team in the grid
    RC(wg::launch(P, wg::PLAIN, x0_zero, grid, h->stream, B, m, R));
    h->res.launched(P.T, P.W, P.G);
    *ran = true;
    return ELPH_OK;
}

#ifdef ELPH_WG_ARRIVE
extern "C" int elph_debug_wg_arrive(unsigned long long *out, int n_blocks, int clear) {
    if (clear) { static unsigned long long z[4096 * 4]; return hipMemcpyToSymbol(HIP_SYMBOL(wg::g_wg_arrive), z, sizeof(z)) == hipSuccess ? 0 : -1; }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(wg::g_wg_arrive), (size_t)n_blocks * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef ELPH_WG_ARRIVE
extern "C" int elph_debug_wg_timeline(unsigned long long *out, int n_blocks) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(wg::g_wg_timeline), (size_t)n_blocks * 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef ELPH_WG_STAMPS
extern "C" int elph_debug_wg_stamps(unsigned long long *out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(wg::g_wg_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

// One rank's launch of a solve over several GPUs (shard.hip holds the mailbox and calls this).  x0 = 0, b in B.r and B.p.
// one rank's launch arguments of a sharded solve: the plan of its slab (wg::plan_shard), control block (zeroed), tags
static int shard_rank_setup(elph_handle_s *h, long long fixed_iters, const ElphShardCtl &Sh, ModelDev &m, wg::WgPlan &P, wg::WgCtl &R) {
    m = elph_model_dev(h);
    RC(wg::plan_shard(wg::wg_facts(h), wg::wg_knobs(1, fixed_iters), Sh.P, &P));
    const size_t HS = (size_t)P.npl * WAVE;
    const size_t n_slots = 2 * wg::SLOTS_PER_RHS, n_bnd = (P.G > 1) ? 2 * (size_t)P.G * 2 * HS * 2 : 0;
    // (the records of a sharded solve live in the ranks' mailboxes, one numbering for all: this rank's block — the boundary granules of
    //  its workgroups — is zeroed and its tags restart at 2 with every launch.  A sharded solve has NO streaming fallback behind it — a
    //  time-out is a failed solve — and its ranks start with whatever skew the host's barrier, first-launch code loading and time-slicing
    //  leave: the long bound, elph_shard_timeout_ms)
    RC(elph_wg_ctl(h, n_slots, n_bnd, 0, elph_shard_timeout_ms(), WG_TAGS_RESTART, &R));
    R.bnd = R.slots + n_slots;
    R.G = P.G; R.W = P.W;
    R.fixed_iters = fixed_iters;
    return ELPH_OK;
}

int elph_wg_cg_shard(elph_handle_s *h, const CgBufs &B, long long fixed_iters, const ElphShardCtl &Sh, int *G_out) {
    ModelDev m;
    wg::WgPlan P;
    wg::WgCtl R;
    RC(shard_rank_setup(h, fixed_iters, Sh, m, P, R));
    const dim3 grid((unsigned)P.G);                        // one right-hand side: its G workgroups, round-robin over the XCDs
    RC(wg::launch(P, wg::SHARD, false, grid, h->stream, B, m, R, Sh));
    h->res.launched(P.T, P.W, P.G);
    if (G_out) *G_out = P.G;
    return ELPH_OK;
}

// ALL RANKS OF A SHARDED SOLVE WHOSE SLABS LIVE ON ONE DEVICE, IN ONE LAUNCH (slabs.hip): the same kernel, rank q's workgroups = blocks
// q G .. q G + G - 1, launch arguments from d_args (device memory, P x elph_wg_rank_args_bytes()).  Every slab must take the lane-program
// or the GRID form with the same sites per lane and the same team shape; all P G workgroups must be resident at once (they wait for each other).
size_t elph_wg_rank_args_bytes() { return sizeof(wg::WgRankArgs); }

int elph_wg_cg_ranks(elph_handle_s *const *hs, int P, const CgBufs *Bs, long long fixed_iters, const ElphShardCtl *ctls, void *h_args,
                     void *d_args, hipStream_t stream, long long timeout_ms, int *G_out) {
    if (P < 1 || P > 2 * ELPH_SHARD_MAXRANKS) { elph_set_error("bad rank count %d", P); return ELPH_E_ARG; }      // (up to two sets of slabs)
    wg::WgRankArgs *A = static_cast<wg::WgRankArgs *>(h_args);          // (pinned, owned by the caller: the copy below is asynchronous)
    wg::WgPlan P0;
    for (int q = 0; q < P; ++q) {
        if (hs[q]->stream != stream) { elph_set_error("slab %d runs on another stream", q); return ELPH_E_STATE; }
        wg::WgPlan Pq;
        RC(shard_rank_setup(hs[q], fixed_iters, ctls[q], A[(size_t)q].m, Pq, A[(size_t)q].R));
        if (Pq.form == wg::HGRID || hs[q]->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("slabs on one device: lane-program or GRID form, site phonons"); return ELPH_E_UNSUPPORTED; }
        if (q == 0) P0 = Pq;
        else if (Pq.npl != P0.npl || Pq.W != P0.W || Pq.G != P0.G || Pq.shm != P0.shm || Pq.form != P0.form) { elph_set_error("slabs on one device: slab %d has another shape", q); return ELPH_E_UNSUPPORTED; }
        P0.uniform = P0.uniform && Pq.uniform;      // (one kernel for all slabs: uniform hopping only if every slab has it)
        if (timeout_ms > 0) A[(size_t)q].R.timeout_ticks = timeout_ms * 100000LL;      // (slabs of one device: a streaming fallback exists, the short bound)
        A[(size_t)q].B = Bs[q];
        A[(size_t)q].Sh = ctls[q];
    }
    if ((long long)P * P0.G > elph_i_resident_wg_limit(hs[0])) { elph_set_error("slabs on one device: %d x %d workgroups cannot all be resident", P, P0.G); return ELPH_E_UNSUPPORTED; }
    HIPCHK(hipMemcpyAsync(d_args, A, (size_t)P * sizeof(wg::WgRankArgs), hipMemcpyHostToDevice, stream));
    wg::WgCtl R0 = A[0].R;
    R0.ranks = d_args;
    // (tests, ELPH_SLABS_TEST_TIMEOUT=2: the last rank's workgroups are NOT launched — the others wait for them until their bound and give up)
    const int drop = (elph_slabs_test_timeout() == '2') ? 1 : 0;
    const dim3 grid((unsigned)((P - drop) * P0.G));
    RC(wg::launch(P0, wg::RANKS, false, grid, stream, Bs[0], A[0].m, R0, ctls[0]));
    for (int q = 0; q < P; ++q) hs[q]->res.launched(1, P0.W, P0.G);
    if (G_out) *G_out = P0.G;
    return ELPH_OK;
}
