// elph_internal.h — internal declarations of libelphgpu (gfx950 only).
//
// Device-side data layout ("layout S", slice-major): a lattice vector is stored as
//     v_S[tau * N + site]
// i.e. one imaginary-time slice (all N sites) is contiguous.  The reference / C-ABI layout
// ("layout R", Utilities.jl:12-15) is v_R[site * L + tau].  Host and `_dev` entry points
// convert with a tiled transpose kernel; everything between (CG vectors, expV, KPM scratch)
// stays in layout S, so that
//   * one wavefront owns one tau-slice: its loads/stores are contiguous 8*N bytes,
//   * the checkerboard sweep (couples sites at fixed tau) runs in that wave's LDS with no
//     cross-wave synchronisation,
//   * the tau-FFT output nu[omega][site] is already the omega-major layout the per-omega
//     Chebyshev recursion of the KPM preconditioner wants (no transposes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <math.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/elph_gpu.h"
#include "elph_bench.h"

#define ELPH_WAVE 64
#define ELPH_MAX_NPL 8          // sites per thread
#define ELPH_MAX_SITES 8192      // generic kernels: workgroups of up to 1024 threads x 8 sites
#define ELPH_CG_CHUNK 16        // CG iterations between two reads of the CG states by the host (even: ping-pong parity)

void elph_set_error(const char *fmt, ...);
int elph_launch_check(const char *what);      // elph_api.hip: hipGetLastError after a launch, "launch <what> failed: ..." into the error text

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            elph_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return ELPH_E_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define RC(call)                \
    do {                        \
        int _rc = (call);       \
        if (_rc) return _rc;    \
    } while (0)

#define CHECK_H(h)                                                    \
    do {                                                              \
        if (!(h)) { elph_set_error("null handle"); return ELPH_E_ARG; } \
        HIPCHK(hipSetDevice((h)->device));                            \
    } while (0)

// Model description handed to kernels by value.
struct ModelDev {
    int N, L, nb, ncol;
    int cs_tau_stride;   // 0 (Holstein: c,s per bond) or nb (SSH: c,s per (tau,bond))
    int E_tau_stride;    // N (Holstein: E per (tau,site)) or 0 (SSH: E per site)
    int nchains;         // independent phonon configurations resident in E (right-hand side r uses chain r % nchains)
    long long E_chain_stride;   // ndim (Holstein) between chains; unused when nchains == 1
    const int *bi;       // [nb] 0-based first site of bond, checkerboard order
    const int *bj;       // [nb]
    const int *coloff;   // [ncol+1] colour boundaries into the bond list
    const double *c;     // cosh table
    const double *s;     // sinh table
    const double *E;     // exp(-dtau V) (Holstein, layout S) or exp(dtau mu) (SSH)
    // "lane program" (cg_fast.hip): bonds re-packed [colour][pass][lane], PP = ceil(npl/2) passes per colour,
    // NE = MC*PP entries (MC = 4 or 6 colours); idle slots point at the lane's padding pair.  Only valid when ncol <= 6.
    const unsigned *lp_ij;   // [NE][64]  i | j << 16
    const double *lp_c;      // [1 or L][NE][64]
    const double *lp_s;
    int lp_tau_stride;       // 0 (Holstein) or NE*64 (SSH)
    // SSH with several resident phonon configurations: one set of hopping tables per chain (0: shared tables)
    long long cs_chain_stride, lp_chain_stride;
    // every bond carries the same (cosh, sinh) (Holstein without hopping disorder): kernels may keep them in two scalars
    int uniform;
    double c_uni, s_uni;
    // 16 x 16 square lattice in the reference's colouring: the bond that covers site i in colour col ([4][N]; nullptr otherwise)
    const int *sq_bond;
    // a periodic square lattice of (2 grid_GX) x (2 grid_GY) sites in that colouring (square: GX = GY = L / 2; the slab of a sharded solve:
    // 16 x rows): the lane grid of the GRID layout (cg_fast_common.h); 0 otherwise
    int grid_GX, grid_GY;
    // a periodic honeycomb lattice of hc_LX x hc_LY two-site cells in the reference's colouring (LatticeShape); 0 otherwise
    int hc_LX, hc_LY;
};
#ifdef __HIPCC__
// the hopping tables of the chain right-hand side `rhs` belongs to (SSH chains; no-op otherwise)
__device__ __forceinline__ void ssh_chain_select(ModelDev &m, int rhs) {
    if (m.cs_chain_stride) {
        const long long c = rhs % m.nchains;
        m.c += c * m.cs_chain_stride; m.s += c * m.cs_chain_stride;
        m.lp_c += c * m.lp_chain_stride; m.lp_s += c * m.lp_chain_stride;
    }
}
#endif

// internal only (never crosses the C ABI): a resident launch gave up at its time-out — the caller owns the fallback.  Distinct from ELPH_E_HIP so
// that a real device error (event, copy, launch) is never mistaken for a time-out and hidden behind the streaming fallback.
#define ELPH_I_ABORTED (-100)
int elph_i_resident_wg_limit(const elph_handle_s *h);      // cg_wg.hip: workgroups of a resident kernel that can be co-resident on the handle's device

// Solver parameters travel BY VALUE in the kernel arguments (never through a small H2D copy + scalar load).
#define ELPH_SPLIT_PARTS 2    // parts of a preconditioned batch on streams of their own (cg_solve.hip: SplitRun)

struct CgParams {
    double tol, kmax;
    long long maxiter;
    int use_prec;
    int record_hist;
    long long hist_stride;
};

// Buffers of the CG iteration kernels (all layout S).
struct CgState;
struct CgBufs {
    double *x, *r, *z, *zp;     // [nrhs][ndim]; zp = P^-1 r (preconditioned only)
    double *p;                  // [2][nrhs][ndim] ping-pong by (seq & 1)
    double *pap, *rr, *rz;      // partial sums [nrhs][npart]
    double *alpha;              // [nrhs] step length of the last k_cg_xr (fast family: x += alpha p is applied by the NEXT k_cg_ap)
    CgState *state;             // [nrhs][2]
    CgParams params;
    double *hist;               // optional eps history
    int dot_lo, dot_hi;         // sites [dot_lo, dot_hi) enter the inner products (whole slice unless a spatial shard)
    int nrz;                    // number of r.z partials per rhs
    int npap;                   // number of p.z partials per rhs (L, or L/T for the chunked kernel)
    int nrhs;
};

// CG state of one right-hand side; two copies, the newer one has the larger seq.
struct CgState {
    double rho;       // r.z (or r.r) belonging to the current search direction
    double kmin;      // running lower bound of the condition number (IterativeSolvers.jl:289)
    double eps0;      // |r0|/|b|
    double normb;     // |b|
    double eps;       // last evaluated |r|/|b|
    long long seq;    // number of k_cg_ap launches that advanced this state
    long long iters;  // completed CG iterations
    int done;         // 0 running, 1 eps<tol, 2 kmin>kmax, 3 maxiter reached
    int pad;
};


// The kernels one CG iteration launches, chosen once per solve by elph_plan_cg (kernels.hip) and only read by the launchers (host only).
struct CgPlan {
    enum Ap { AP_LANE, AP_SQ16, AP_PG, AP_GEN };      // k_cg_ap: lane program, its register form (cg_sq16.hip), patch form (pgrid.hip), generic
    enum Cheb { CH_LANE, CH_PG, CH_GEN };             // Chebyshev recursion: lane family (elph_fast_kpm_cheb), patch form, generic k_kpm_cheb
    int nrhs = 0, in_flight = 0;   // right-hand sides of this stream / on all streams (the parts of a split batch: every part)
    bool px = false;               // preconditioned and p/x-fused (x += alpha p, p = P^-1 r + beta p in the inverse transform's epilogue)
    bool xr_in_fwd = false;        // a preconditioned iteration folds its residual update into the forward transform (kpm apply cg_mode 2)
    bool reg_cheb = false;         // the lane family's register-exchange Chebyshev recursion runs (elph_reg_cheb_form; not under ELPH_NO_SQ=1)
    bool rz_freq = false;          // inside CG the Chebyshev kernel delivers the r.z partials in frequency space
    bool fold = false;             // cg_mode 2: the order-1 frequencies are finished by the forward transform (dft_mfma.hip: XrFuse)
    Ap ap = AP_LANE;
    Cheb cheb = CH_LANE;
    int T = 1;                     // slices per wave of k_cg_ap: npap = ceil(L / T) p.Ap partials per right-hand side
};


// one frequency block of a chain's schedule, packed so that a Chebyshev block learns what it has to do from ONE 32-byte load
// (frequency, order, offset of its coefficients, leading coefficient) instead of a chain of four dependent ones
struct KpmDesc { int w, order, coff, pad; double c0x, c0y; };

struct KpmDev {
    int active;
    int Lo2;
    int nchains;              // one expansion per phonon configuration (chain); right-hand side r uses chain r % nchains
    double lam_avg, lam_mag;  // chain 0 by value (the single-chain kernels never wait for a load of them)
    const double *lam;        // [nchains][2] lam_avg, lam_mag
    const double *Ebar;       // [nchains][N]
    const double *cbar;       // [nb]
    const double *sbar;       // [nb]
    const int *order;         // [nchains][Lo2]
    const int *coff;          // [nchains][Lo2+1] offsets into coeff (absolute: a chain's base is included)
    const double2 *coeff;     // [sum over chains of sum order]
    const int *wsched;        // [nchains][Lo2] omega indices sorted by decreasing order (longest first)
    const KpmDesc *desc;      // [nchains][Lo2] the same schedule, packed (entry y: frequency wsched[y])
    const double *lp_cbar;    // lane-program copies of cbar/sbar [NE][64]
    const double *lp_sbar;
    // SSH chains: every chain has its own tau-averaged hopping (cbar, sbar) — strides between chains, 0 when shared (Holstein)
    long long hop_stride, lp_hop_stride, sq_stride;
};

// One chain's view of the expansion (device side).
struct KpmChainView {
    const int *order, *coff, *wsched;
    const KpmDesc *desc;
    const double *Ebar;
    double a, b;              // 1/lam_mag, lam_avg/lam_mag
    const double *cbar, *sbar, *lp_cbar, *lp_sbar;    // this chain's averaged hopping tables
    bool active;              // false: this chain's preconditioner is the identity (order 1, coefficient 1 everywhere)
};
#ifdef __HIPCC__
__device__ __forceinline__ KpmChainView kpm_chain_view(const KpmDev &K, int rhs, int N) {
    KpmChainView V;
    if (K.nchains > 1) {
        const int c = rhs % K.nchains;
        V.order = K.order + (size_t)c * K.Lo2;
        V.coff = K.coff + (size_t)c * (K.Lo2 + 1);
        V.wsched = K.wsched + (size_t)c * K.Lo2;
        V.desc = K.desc + (size_t)c * K.Lo2;
        V.Ebar = K.Ebar + (size_t)c * N;
        const double avg = K.lam[2 * c], mag = K.lam[2 * c + 1];
        V.a = 1.0 / mag;
        V.b = avg / mag;
        V.active = mag > 0.0;                                  // the host uploads a negative magnitude for an inactive chain
        V.cbar = K.cbar + c * K.hop_stride; V.sbar = K.sbar + c * K.hop_stride;
        V.lp_cbar = K.lp_cbar + c * K.lp_hop_stride; V.lp_sbar = K.lp_sbar + c * K.lp_hop_stride;
    } else {
        V.cbar = K.cbar; V.sbar = K.sbar; V.lp_cbar = K.lp_cbar; V.lp_sbar = K.lp_sbar;
        V.order = K.order; V.coff = K.coff; V.wsched = K.wsched; V.desc = K.desc; V.Ebar = K.Ebar;
        V.a = 1.0 / K.lam_mag;
        V.b = K.lam_avg / K.lam_mag;
        V.active = K.active != 0;
    }
    return V;
}
#endif

// The lattice a handle's bond table holds, recognised once at elph_create by elph_recognise_lattice (lattice_shape.cpp) in the reference's colouring
// (host only).  Derived facts are accessors, not fields.
struct LatticeShape {
    enum Kind { NONE, SQUARE, HONEYCOMB, TRIANGULAR, CUBIC };     // (the values are the patch kinds of pgrid.hip)
    Kind kind = NONE;
    int LX = 0, LY = 0;            // periodic LX x LY sites (square, triangular) or two-site cells (honeycomb); cubic: LX x LY x LZ sites
    int LZ = 0;                    // simple cubic only (0: a two-dimensional lattice)
    int PX = 0, PY = 0, NW = 0;    // patch layout (pgrid_dev.h): PX x PY sites / cells per lane (cubic: 2 x 2 x 2 sites) on NW wavefronts per slice; 0: none
    int GX = 0, GY = 0;            // GRID layout (cg_fast_common.h): a GX x GY grid of lanes holding 2 x 2 patches; 0: none
    std::vector<int> bond;         // square lattices: [4][N] the bond that covers site i in colour col
    bool hop_uniform = false;      // Holstein, and every bond of the model's table carries (hop_c, hop_s)
    double hop_c = 1.0, hop_s = 0.0;

    bool patch() const { return PX > 0; }
    int patch_kind() const { return patch() ? (int)kind : 0; }
    // a square lattice without patches: up to 16 x 16 sites, or a rectangle of at most 64 patches (a sharded solve's ring-closed slab)
    bool small_square() const { return kind == SQUARE && !patch(); }
    int sq_L() const { return small_square() && LX == LY ? LX : 0; }                        // ... when it is square
    int dpp() const { return sq_L() == 8 ? 1 : sq_L() == 16 ? 2 : 0; }                      // 1: the 8 x 8, 2: the 16 x 16 DPP forms
    bool honeycomb() const { return kind == HONEYCOMB; }
    int cubic_L() const { return kind == CUBIC && LX == LY && LY == LZ ? LZ : 0; }            // the side of a simple-cubic lattice in the patch layout
    int hc_L() const { return honeycomb() && LX == LY ? LX : 0; }
    bool hc12() const { return hc_L() == 12; }                                                // the honeycomb DPP / quad forms
    // the honeycomb grid form: registers per lane (2, 4 or 8: 1, 2 x 1 or 2 x 2 cells) when the cells fit 64 lanes, else 0
    int hgrid_regs() const {
        if (!honeycomb()) return 0;
        if (LX * LY <= 64) return 2;
        if (LX % 2 == 0 && (LX / 2) * LY <= 64) return 4;
        if (LX % 2 == 0 && LY % 2 == 0 && (LX / 2) * (LY / 2) <= 64) return 8;
        return 0;
    }
};

// The KPM preconditioner of a handle (host only): elph_kpm_create's parameters, one expansion per chain, the averaged inputs and the
// flattened tables, each with its device images.  kpm_setup_core (kpm_setup.hip) fills it; the planning is pure (kpm_host.cpp).
struct KpmParams { int n = 20; double buf = 0.05, c1 = 1.0, c2 = 1.0; };

// one chain's expansion (KPMExpansion, KPMPreconditioners.jl:101-146); the constructor state is order 1 and c₀ = 1 everywhere
struct KpmChain {
    double lam_lo = 0.0, lam_hi = 2.0;
    int active = 1;
    bool fresh = true;                     // never uploaded
    std::vector<int> order;                // [Lo2]; coeff: complex interleaved, sum of order
    std::vector<double> coeff;
    explicit KpmChain(int Lo2 = 0) : order((size_t)Lo2, 1), coeff(2 * (size_t)Lo2, 0.0) { for (int w = 0; w < Lo2; ++w) coeff[2 * (size_t)w] = 1.0; }
};

// the device tables of every chain's expansion, flattened (elph_kpm_tables)
struct KpmTables {
    std::vector<int> order, coff, wsched;  // [nch][Lo2], [nch][Lo2+1] (absolute offsets into coeff), [nch][Lo2] frequencies longest first
    std::vector<KpmDesc> desc;             // [nch][Lo2] the same schedule, packed
    std::vector<double> fold;              // [nch][Lo2][2] order-1 fold of the forward transform: {scale, r.z weight} (dft_mfma.hip: XrFuse)
    std::vector<double> lam;               // [nch][2] lam_avg, lam_mag (< 0: the identity expansion)
    std::vector<double> coeff;             // complex interleaved, all chains
    int recurse = 1;                       // frequency blocks that some chain still recurses on (order >= 2, or an identity expansion)
};

struct KpmState {
    KpmParams par;
    bool created = false, ready = false, ssh = false;      // ssh: bond phonons, every chain has its own averaged hopping
    std::vector<KpmChain> chains;          // one per resident configuration
    // averaged inputs (update_A!) and their device images
    std::vector<double> h_Ebar, h_cbar, h_sbar;     // h_Ebar: [nch][N]; h_cbar, h_sbar: [nb], or [nch][nb] when hop_per_chain()
    double *d_Ebar = nullptr, *d_cbar = nullptr, *d_sbar = nullptr;    // [nch][N]; [hop chains][nb]
    double *d_lp_cbar = nullptr, *d_lp_sbar = nullptr;    // lane-program copies [hop chains][NE][64] (fast_capable)
    double *d_sq_cbar = nullptr, *d_sq_sbar = nullptr;    // [hop chains][4][N] through shape.bond (shape.sq_L() > 0)
    int hop_cap = 0;                       // chains the hopping images are allocated for
    bool hop_uploaded = false;             // Holstein: c̄, s̄ (= cosh, sinh of the fixed hoppings) are on the device already
    bool sq_chain_uniform = false;         // small square lattices: the averaged hopping is one (cbar, sbar) WITHIN each chain (SSH chains may
                                           // differ from one another): the register Chebyshev kernels keep them in scalars
    bool hop_uniform = false;              // the averaged hopping is one (cbar, sbar) for every bond, shared by all chains
    // the flattened tables and their device copies
    KpmTables tab;
    int *d_order = nullptr, *d_coff = nullptr, *d_wsched = nullptr;
    KpmDesc *d_desc = nullptr;
    double *d_fold = nullptr, *d_lam = nullptr;
    double2 *d_coeff = nullptr;
    int tab_cap = 0;                       // chains d_Ebar, the tables and d_start are allocated for
    size_t coeff_cap = 0;                  // coefficients d_coeff holds
    double *d_start = nullptr;             // Arnoldi start vectors [2][nch][N] + the bounds [nch][2] coming back (kpm_dev.hip); made on first use
    int nch() const { return (int)chains.size(); }
    bool hop_per_chain() const { return ssh && nch() > 1; }
    bool any_active() const { for (const auto &C : chains) if (C.active) return true; return chains.empty(); }
    bool all_active() const { for (const auto &C : chains) if (!C.active) return false; return true; }
    double lam_avg(int c) const { return tab.lam.empty() ? 1.0 : tab.lam[2 * (size_t)c]; }
    double lam_mag(int c) const { return tab.lam.empty() ? 1.0 : tab.lam[2 * (size_t)c + 1]; }
};

// The host state of the resident solvers — k_cg_wg in its plain, sharded and slab launches (cg_wg.hip), k_pcg_wg (pcg_wg.hip).  They share
// ONE control block per handle, one tag numbering, one abort word and one time-out / cool-down / fallback protocol:
//   block   [meeting records | extra words: k_cg_wg's boundary granules or k_pcg_wg's flags | ... | abort word in the last 64 bytes]
//           laid out, grown, zeroed and numbered by elph_wg_ctl alone;
//   shape   of the last launch, for the time-out message: launched();
//   health  elph_wg_timed_out is the only writer of a time-out, elph_wg_cooldown_step the only one that counts it down and clears it.
struct ResidentState {
    void *d_res = nullptr;                 // the control block (freed by elph_destroy)
    size_t cap = 0;                        // its bytes
    unsigned next_tag = 0;                 // next free tag of the meeting records (WgCtl::epoch0 of the next launch)
    size_t abort_off = 0;                  // byte offset of the abort word in d_res (0: nothing launched yet)
    int T = 0, W = 0, G = 0;               // shape of the last resident launch (0: none yet)
    int cooldown = 0;                      // solves left on the streaming iteration after a time-out, then the resident kernels are tried again
    long long fallbacks = 0;               // how many launches timed out (elph_wg_status)
    bool cooling() const { return cooldown > 0; }
    void launched(int t, int w, int g) { T = t; W = w; G = g; }
};

// The tau-axis transforms (dft.hip, dft_mfma.hip, dft_big.hip).  What a time axis offers is derived once (dft_shape), the switches are read
// once per plan (dft_switches), one pure planner chooses the form of a transform (elph_plan_dft); the launchers read the plan and decide
// nothing.  The device-free probe elph_bench_dft_plan holds the planner to tests/golden/dft_plan.json.
enum DftKind { DFT_TWISTED = 0, DFT_PLAIN = 1 };
// SCALAR: scalar-twiddle tables (dft.hip); matrix cores (dft_mfma.hip): ONE_TILE one 16 x 16 output tile per wave (k_dft_mfma_1), DIRECT the
// (2K x L) GEMM (k_dft_mfma), SPLIT_REG / SPLIT_LDS the even/odd split of the twisted transform with its data in registers (k_dft_mfma_r2) / its
// W panel in LDS (k_dft_mfma_r2s); long axes (dft_big.hip): BIG_ROW one output row per wave, BIG_BLOCKED k_big_s1 / k_big_s2, BIG_DIRECT a prime
enum DftForm { DFT_SCALAR, DFT_ONE_TILE, DFT_DIRECT, DFT_SPLIT_REG, DFT_SPLIT_LDS, DFT_BIG_ROW, DFT_BIG_BLOCKED, DFT_BIG_DIRECT };
struct DftTab { int nt = 0, groups = 0; };     // reduction tiles (a template size; 0: no such table), row groups of 5 row tiles
struct DftShape {
    int L = 0;
    int L1 = 0, L2 = 0;        // the long-axis split L = L1 * L2 (0: not a long axis; L2 == 1: the direct long transform)
    DftTab mf[2][2];           // the direct matrix-core tables [twisted / plain][forward / inverse]
    DftTab r2[2];              // the even/odd split of the twisted transform [forward / inverse]: even L >= 8
    bool big() const { return L1 > 0; }
};
// ELPH_DFT_MFMA (-1 unset), ELPH_DFT_R2, ELPH_FUSE_XR, ELPH_FUSE_PX, ELPH_DFT_BIG_BLOCKED (-1 unset)
struct DftSwitches { int mfma = -1; bool r2 = true, fuse_xr = true, fuse_px = true; int big_blocked = -1; };
struct DftPlan {
    DftForm form = DFT_SCALAR;
    int nt = 0, groups = 0;    // of the table the form reads (matrix-core forms)
    int lds = 0;               // dynamic LDS bytes: the W panel of DFT_SPLIT_LDS
    int slots = 0;             // r.z partial slots the form fills (0: no r.z asked for)
    bool short_slots = false;  // the inverse has to deliver r.z and the caller offers fewer slots than the form fills: ELPH_E_STATE
    // what the preconditioned CG iteration may fuse into this transform (elph_plan_cg): the residual update and the order-1 fold into the
    // forward twisted transform, the p/x-update into the inverse one
    bool xr = false, px = false, fold = false;
};
struct DftState {
    DftShape shape;
    double2 *theta = nullptr;                    // [2L] exp(-i pi t / L)
    double2 *Tk = nullptr, *Tt = nullptr;        // scalar twisted tables [Lo2][L] / [L][Lo2]
    double2 *Pk = nullptr, *Pt = nullptr;        // scalar plain tables   [Lh][L]  / [L][Lh]
    double *W[2][2] = {}, *W_r2[2] = {};         // matrix-core tables in A-tile order, as shape.mf / shape.r2
    double *r2_tw = nullptr;                     // [L/2] (cos, -sin) of pi (2k+1) / L
    double2 *big_W1 = nullptr, *big_W2 = nullptr, *big_TW = nullptr;      // long axis: the two sub-transforms and the L roots of unity
    double2 *big_a = nullptr, *big_b = nullptr;  // ... two complex work vectors of big_cap elements, grown with the batch (dft_big.hip)
    size_t big_cap = 0;
};

// The workspace of a solve (host only; all device vectors in layout S): everything sized by the number of right-hand sides the handle has
// room for.  elph_work_reserve (elph_api.hip) is its only allocator, elph_work_release its only freer, part() the only code that knows which
// arrays are per right-hand side and how far each advances.
struct SolveWork {
    int cap_rhs = 0;                       // right-hand sides there is room for
    size_t ndim = 0, nnu = 0, nrz = 0;     // elements per right-hand side: of a vector, of nu (ceil(L/2) N), of one partial-sum array (L npl)
    double *stage_in = nullptr, *stage_out = nullptr;      // layout R staging [cap_rhs][ndim] (elph_stage_in, elph_stage_out)
    double *b = nullptr, *x = nullptr, *r = nullptr, *z = nullptr, *zp = nullptr;      // [cap_rhs][ndim]
    double *tmp = nullptr;                 // [cap_rhs][ndim] scratch (v''')
    double *p = nullptr;                   // [2][cap_rhs][ndim] ping-pong by parity
    double2 *nu = nullptr;                 // [cap_rhs][>= nnu] complex (half spectrum, omega-major)
    double *sums = nullptr;                // partial sums: the four arrays pap, rr, rz, bb of [cap_rhs][nrz]
    CgState *state = nullptr, *h_state = nullptr;          // [cap_rhs][2], device and pinned
    double *alpha = nullptr;               // [cap_rhs] CG step length handed from k_cg_xr to the next k_cg_ap
    double *scal = nullptr, *h_scal = nullptr;             // [4 cap_rhs] small scalar scratch (residual norms), device and pinned
    double *hist = nullptr;                // hist_cap doubles: the eps histories of a solve that records them (run_cg grows it)
    int64_t hist_cap = 0;
    double *phi = nullptr, *xfield = nullptr;              // force assembly: phi+- [2][ndim], x in layout S [ndim]

    size_t part_stride() const { return (size_t)cap_rhs * nrz; }      // between two of the partial-sum arrays
    double *pap() const { return sums; }
    double *rr() const { return sums + part_stride(); }
    double *rz() const { return sums + 2 * part_stride(); }
    double *bb() const { return sums + 3 * part_stride(); }
    // The view of the right-hand sides from r0 on (the second stream's part of a split batch).  cap_rhs stays the whole record's: it is the
    // distance of the partial-sum arrays, which are indexed [rhs][<= nrz], so one offset serves all four.  p is [2][cap_rhs][ndim]: slot 1 of
    // one part would overlap slot 0 of the next, so a view is only good for an iteration that reads and writes slot 0 alone, the p/x-fused
    // one (cg_solve.hip: split_legal demands it).  What is not per right-hand side (staging, scal, hist, phi, xfield) is shared.
    SolveWork part(size_t r0) const {
        SolveWork v = *this;
        v.b += r0 * ndim; v.x += r0 * ndim; v.r += r0 * ndim; v.z += r0 * ndim; v.zp += r0 * ndim; v.tmp += r0 * ndim; v.p += r0 * ndim;
        v.nu += r0 * nnu;
        v.state += 2 * r0; v.h_state += 2 * r0; v.alpha += r0;
        v.sums += r0 * nrz;
        return v;
    }
};

struct elph_handle_s {
    int kind = 0, device = 0;
    int64_t N = 0, L = 0, nb = 0, ndim = 0;
    int npl = 0;               // ceil(N/64)
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // model
    int ncol = 0;
    std::vector<int> h_bi, h_bj, h_coloff;
    std::vector<double> h_c, h_s;          // Holstein: [nb]; SSH: tau-major [L][nb]
    int *d_bi = nullptr, *d_bj = nullptr, *d_coloff = nullptr;
    double *d_c = nullptr, *d_s = nullptr, *d_E = nullptr;
    bool have_E = false;
    int nchains = 1;                       // Holstein: independent chains sharing one handle / one batch
    int64_t E_cap = 0;                     // doubles allocated for d_E
    int dot_lo = 0, dot_hi = 0;            // sites counted in the CG inner products (elph_set_dot_range); hi = 0: all
    bool fast_capable = false;             // lane-program kernels possible for this bond table (fast may be switched off)
    int solo_chain = -1;                   // >= 0: kernels see only this chain (single re-solve of one RHS of a chains batch)
    double *d_lam = nullptr;               // [3N] lambda, lambda2, mu staging
    hipStream_t split_stream[ELPH_SPLIT_PARTS] = {};      // streams 1 … ways-1 + event of the split form of a preconditioned batch (cg_solve.hip: SplitRun; [0] unused: the handle's own stream)
    hipEvent_t split_ev = nullptr;
    CgPlan plan;                           // the kernels of the current solve's CG iteration (kernels.hip: elph_plan_cg)
    // SSH update_model! on the device (elph_update_model_ssh_fields): staging of x, per-phonon tables, slot map
    double *d_ssh_x = nullptr, *d_ssh_par = nullptr, *d_ssh_tbare = nullptr, *d_ssh_bar = nullptr;
    int *d_ssh_cb = nullptr, *d_ssh_slot = nullptr;
    int64_t ssh_nph_cap = 0;
    double *d_mu_ch = nullptr;             // [mu_ch_cap][N] chemical potential per chain (the tuner with chains in lockstep)
    int mu_ch_cap = 0;
    bool mu_per_chain = false;
    int ssh_chain_cap = 1;                 // SSH: chains whose hopping tables (d_c, d_s, d_lp_c, d_lp_s) and fields (d_ssh_x) are allocated
    int ssh_nph = -1;                      // fields of the last device-side update_model!
    double ssh_dtau = 0.0;
    bool cs_host_stale = false;            // SSH: d_c/d_s were produced on the device; h_c/h_s are not current
    // lane program (fast path, ncol <= 4)
    bool fast = false;
    int lp_mc = 4;                         // colours of the lane program the kernels were compiled for: 4 (lp4) or 6 (lp6)
    int lp_ne = 0;
    std::vector<unsigned> h_lp_ij;
    unsigned *d_lp_ij = nullptr;
    double *d_lp_c = nullptr, *d_lp_s = nullptr;
    LatticeShape shape;                    // the lattice of the bond table (elph_create: elph_recognise_lattice)
    int *d_pg_bond = nullptr;                            // [4][N] shape.bond of a square lattice in the patch layout: hopping disorder there
    int *d_sq_bond = nullptr;                            // [4][N] shape.bond of a small square lattice (shape.sq_L() > 0)
    void *shard = nullptr;                 // ShardState (shard.hip), owned
    void *slabs = nullptr;                 // SlabSet (slabs.hip), owned: slab handles of this lattice on the same device
    bool slabs_tried = false;              // the slab decomposition was attempted (slabs == nullptr: it does not apply)
    bool is_slab = false;                  // this handle IS a slab of another handle (never decomposed again)
    void *hmc = nullptr;                   // HmcState (hmc_dev.h; hmc.hip, langevin.hip, special_updates.hip), owned by hmc.hip
    void *greens = nullptr;                // GreensState (greens.hip), owned
    // the measurement families, two slots each, owned and freed with greens: the single-configuration entry points' state (nchains = 1,
    // the estimator's own scratch) and the _chains entry points' (every resident chain, scratch of its own) — the same type, side by side
    void *meas = nullptr, *meas_chains = nullptr;                  // MeasState (measure.hip)
    void *bond = nullptr, *bond_chains = nullptr;                  // HolsteinBondState (bondcorr.hip)
    void *ssh_meas = nullptr, *ssh_meas_chains = nullptr;          // SshMeasState (ssh_measure.hip)
    void *ssh_bond = nullptr, *ssh_bond_chains = nullptr;          // SshBondState (ssh_bondcorr.hip)
    void *density_moments = nullptr;       // DensityMomentsState (density_moments.hip), owned; freed with greens
    void *snapshots = nullptr;             // SnapshotsState (snapshots.hip), owned; freed with greens
    void *current = nullptr;               // CurrentState (currcorr.hip), owned; freed with greens
    void *msolve = nullptr;                // MsolveState (msolve.hip), owned: the work vectors of BiCGStab and GMRES, GMRES's Krylov basis
    ResidentState res;                     // the resident solvers' control block, last launch shape and health (cg_wg.hip)
    // x = 0 hint: set by the library right after it zeroes work.x for a solve it is about to start (fill!(x, 0) of the callers, HMC.jl:854;
    // elph_bench_prepare).  run_cg — and elph_bench_run(9 | 10) — read AND clear it first thing (an early error return cannot leave it
    // behind for the next solve) and hand it on as an argument: to elph_launch_cg_init (A x0 = 0 needs no mat-vec) and to elph_wg_cg
    // (the resident kernel does not read x0 either)
    bool x_zero = false;
    long long ap_count = 0;                // k_cg_ap launches since the last cg_init (ping-pong parity)
    int force_T = 0;                       // ELPH_CHUNK_T: 0 auto, 1 never chunk, n > 1 force n slices per wave (template sizes 2/4/5/8/10/16/20 dividing Ltau: the unrolled kernel; any other: k_cg_ap_chunk_rt, ragged last chunk)

    // solver defaults (model.solver)
    double tol = 1e-4, kmax = 1e12;
    int64_t maxiter = 0;
    int solver_kind = ELPH_SOLVER_CG;      // what the callers of the solve run (elph_solver_set_kind); restart: GMRES only
    int solver_restart = 20;

    SolveWork work;                        // the workspace of every solve (elph_work_reserve)
    CgParams cur_params;                   // parameters of the solve in progress (copied into every launch)

    KpmState kpm;                          // the KPM preconditioner (elph_kpm_create, kpm_setup_core)

    DftState dft;                          // the tau-axis transforms: shape, tables, work buffers (elph_dft_build_tables)
    double *d_diag = nullptr;              // fourier-acceleration diagonal staging
    int64_t diag_cap = 0;
};

// ---- launchers implemented in kernels.hip -------------------------------------------------
ModelDev elph_model_dev(const elph_handle_s *h);
KpmDev elph_kpm_dev(const elph_handle_s *h);

// ---- lattice_shape.cpp: the host half of elph_create (no device) ---------------------------------------------------------------------------
int check_bond_table(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht, const double *sinht);
// sizes, coloured bond table, Holstein hopping table, the lane program's plan and the recognised lattice, from elph_create's (checked) arguments
void elph_i_host_handle(elph_handle_s *h, int kind, int64_t nsites, int64_t ltau, int64_t nbonds, const int64_t *neighbor_table,
                        const double *cosht, const double *sinht);

// ---- cg_solve.hip: the CG driver ------------------------------------------------------------------------------------------------------------
// ldiv! on device-resident layout-S work.b / work.x (also hmc.hip, langevin.hip, special_updates.hip, force.hip)
int elph_i_ldiv_core(elph_handle_s *h, int nrhs, int use_prec, int64_t maxiter, int64_t *iters, double *resid, int *flag);
bool split_legal(elph_handle_s *h, int nrhs, int use_prec, bool hist);      // may this batch run as parts on streams of their own?
// `reps` preconditioned iterations of such a batch as parts, joined on the main stream; *run keeps the parts alive (bench_hooks.hip)
int elph_i_split_iterations(elph_handle_s *h, int nrhs, int reps, std::shared_ptr<void> *run);

// ---- elph_api.hip: helpers of every host unit ------------------------------------------------------------------------------------------------
// (re)allocates n elements (at least one) of device memory at *p
template <class T>
int dev_alloc(T **p, size_t n) {
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
    if (n == 0) n = 1;
    HIPCHK(hipMalloc((void **)p, n * sizeof(T)));
    return ELPH_OK;
}
int need_model(elph_handle_s *h);                  // ELPH_E_STATE before the first update_model!
void set_nchains(elph_handle_s *h, int n);         // the resident configurations; a change invalidates the KPM expansion
// lambda, lambda2 and (unless null) mu of a Holstein model into d_lam, stream-ordered
int elph_i_holstein_upload_params(elph_handle_s *h, const double *lambda, const double *lambda2, const double *mu);
// the reference's (Ltau x Nbonds) column-major tables, bt[bond][tau], <-> the device's tau-major tb[tau][bond]
void elph_bt_to_tb(double *tb, const double *bt, size_t L, size_t nb);
void elph_tb_to_bt(double *bt, const double *tb, size_t L, size_t nb);
// the solve workspace and the idioms built on it (elph_api.hip)
int elph_work_reserve(elph_handle_s *h, int nrhs);      // room for nrhs right-hand sides in h->work (grows only; drains the stream when it does)
void elph_work_release(elph_handle_s *h);
// nvec host vectors in the reference layout <-> device vectors in layout S through the staging buffers, stream-ordered, no synchronisation;
// ncols = 0: site vectors (ndim), otherwise field vectors of that many columns.  ELPH_E_STATE when the staging buffer is too small.
int elph_stage_in(elph_handle_s *h, double *dstS, const double *hostR, int nvec, int ncols = 0);
int elph_stage_out(elph_handle_s *h, double *hostR, const double *srcS, int nvec, int ncols = 0);
// Right-hand side r of a batch once more, alone, in slot 0 (the retry of a flagged right-hand side, Models.jl:129-133): slot 0 of x and b
// is parked in the staging buffers, r moves in, the kernels see r's chain only (solo_chain, when the handle holds several), solve_and_flag
// runs, the result moves back to r and slot 0 is restored.
// x, b: the batch's vectors when they are not work.x / work.b (msolve.hip's callers; solve_and_flag then works on slot 0 of these).
int elph_retry_in_slot0(elph_handle_s *h, int r, const std::function<int()> &solve_and_flag, double *x = nullptr, double *b = nullptr);
// the solver tolerance at tol^power for the length of a scope: the two solves of calc_O⁻¹Λϕ! (HMC.jl:827-828, restored as at :912)
struct TolPower {
    elph_handle_s *h;
    double tol0;
    TolPower(elph_handle_s *hh, double power) : h(hh), tol0(hh->tol) { h->tol = pow(tol0, power); }
    ~TolPower() { h->tol = tol0; }
    TolPower(const TolPower &) = delete;
    TolPower &operator=(const TolPower &) = delete;
};
// what calc_O⁻¹Λϕ! returns for each of nch chains from the (iters, flag) of its + and − solve, it2 / fl2: [2][nch]: a failed first solve
// suppresses the second (HMC.jl:880), two good ones report cld(total, 2) (:907-909)
void elph_fold_pair(int nch, const int64_t *it2, const int *fl2, int64_t *iters, int *flag);
// The fermion force of one configuration (update_model! + calc_O⁻¹Λϕ! + calc_dSfdx!); the entry points of force.hip and shard.hip check
// their arguments and supply the pair solve: right-hand sides in work.b[0..1], solutions into work.x[0..1], (iters, flag) as above.
typedef std::function<int(int64_t *iters, int *flag)> ElphPairSolve;
// Holstein: the force is accumulated into the rows [own_lo, own_hi) of dSfdx (the whole lattice: 0, N)
int elph_i_force_holstein(elph_handle_s *h, const double *x, const double *lambda, const double *lambda2, const double *mu, double dtau,
                          const double *phi_plus, const double *phi_minus, double *dSfdx, double *Xp_out, double *Xm_out, int64_t *iters,
                          int *flag, int own_lo, int own_hi, const ElphPairSolve &solve_pair);
// SSH: the bond brackets q_out[n Ltau + tau]
int elph_i_force_ssh(elph_handle_s *h, const double *rhs_plus, const double *rhs_minus, double *q_out, double *Xp_out, double *Xm_out,
                     int64_t *iters, int *flag, const ElphPairSolve &solve_pair);
int elph_i_ssh_bracket_capacity(elph_handle_s *h, int nrhs, int nch);     // nrhs vectors + the SSH bond brackets of nch chains
int elph_i_set_dot_range(elph_handle_s *h, int64_t site_lo, int64_t site_hi);   // inner products over [lo, hi) only (a shard's own sites)
int elph_i_reserve_chains(elph_handle_s *h, int nchains);   // d_E for nchains configurations, h->nchains = nchains
void elph_hmc_free(elph_handle_s *h);
void elph_shard_free(elph_handle_s *h);
// sharded callers (shard.hip): hooks for hmc.hip
bool elph_i_shard_active(const elph_handle_s *h);                           // a shard with its collectives set (or a single rank)
void elph_i_shard_own_range(const elph_handle_s *h, int *lo, int *hi);      // own sites [lo, hi) of the slab
int elph_i_shard_allreduce(elph_handle_s *h, double *buf, int n);
int elph_i_shard_ghost_sync(elph_handle_s *h, double *vecS, int nvec);
int elph_i_shard_ghost_sync_cols(elph_handle_s *h, double *vecS, int nvec, int ncols, const int *gcol, int ngcol, const double *own);
int elph_i_shard_ldiv_dev(elph_handle_s *h, elph_handle_s *hfull, int use_prec, int64_t maxiter, int64_t *iters, double *resid, int *flag);
int elph_i_kpm_setup_ebar(elph_handle_s *h, const double *Ebar_host, const double *b_max, const double *b_min);      // kpm_setup.hip
elph_handle_s *elph_i_shard_full(const elph_handle_s *h);                  // the full-lattice handle registered with elph_shard_set_full_lattice (or nullptr)
int elph_i_shard_global_ebar(elph_handle_s *h, std::vector<double> &Ebar_global);      // Ē of the whole lattice from every rank's own rows
bool elph_i_shard_has_bonds(const elph_handle_s *h);                                    // elph_shard_set_bonds has been called for this slab's bonds
int elph_i_shard_global_csbar(elph_handle_s *h, std::vector<double> &cs, int64_t *n_bonds);   // [c̄ | s̄] of every bond of the lattice from the owners' tables
int elph_i_kpm_setup_csbar(elph_handle_s *h, const double *cbar_host, const double *sbar_host, const double *b_max, const double *b_min);      // kpm_setup.hip
int elph_i_shard_solve_pair(elph_handle_s *h, elph_handle_s *hfull, int use_prec, double tol_power, int64_t *iters, int *flag);
void elph_greens_free(elph_handle_s *h);
void elph_meas_free(elph_handle_s *h);                                      // measure.hip: the slot meas
void elph_meas_chains_free(elph_handle_s *h);                               //              the slot meas_chains
void elph_bond_free(elph_handle_s *h);                                      // bondcorr.hip: bond
void elph_bond_chains_free(elph_handle_s *h);                               //               bond_chains
void elph_i_ssh_meas_free(elph_handle_s *h);                                // ssh_measure.hip: ssh_meas (elph_ssh_meas_free is its public form)
void elph_ssh_meas_chains_free(elph_handle_s *h);                           //                  ssh_meas_chains
void elph_ssh_bond_free(elph_handle_s *h);                                  // ssh_bondcorr.hip: ssh_bond
void elph_ssh_bond_chains_free(elph_handle_s *h);                           //                   ssh_bond_chains
void elph_density_moments_free(elph_handle_s *h);                           // density_moments.hip
void elph_snapshots_free(elph_handle_s *h);                                 // snapshots.hip
void elph_current_free(elph_handle_s *h);                                   // currcorr.hip
// greens.hip internals used by the measurement units
struct ElphGreensView {
    int ns, L1, L2, L3, nc, nv;
    bool have_vectors;
    const double *C;           // [4][L][ns*N] the real correlations of the last pair set up in the estimator's own scratch
    const double *R, *X;       // [nv][ndim] layout S: the noise vectors and M⁻¹R (density_moments.hip, snapshots.hip and currcorr.hip read them in place)
    const double2 *tw;         // [L1 + L2 + L3] exp(-2πi j/Lx), the twiddles of the cell-axis DFTs
};
int elph_i_greens_view(elph_handle_s *h, ElphGreensView *v);
struct ElphGreensPair { const double *X1, *X2, *R1, *R2; };                // a pair's vectors x = M⁻¹r, r
// The buffers of the estimator's pipeline (setup!, and the autocorrelation of a field) for one pair of vectors of nchains chains at once;
// sizes in elements, with Lo2 = ceil(L/2), Lh = L/2 + 1, ncol = n_s N.  The estimator owns one for nchains = 1 — what elph_greens_setup
// and the single-configuration measurement entry points run in; the _chains entry points allocate their own, so that they leave the
// estimator's tables alone.
struct ElphGreensChainScratch {
    int nchains;
    double *f;                 // [8][nchains][ndim] the input fields
    double2 *nuA, *nuP;        // [2][nchains][Lo2][N] twisted, [6][nchains][Lh][N] plain half spectra
    double2 *Y;                // [4][nchains][Lh][ncol] per-frequency spatial correlations
    double *C;                 // [4][nchains][L][ncol] the real tables: table-major, a chain's tables lie nchains L ncol apart
    double2 *out;              // the estimator's own scratch: [4][2L ncol] the doubled complex copies (elph_greens_dev_arrays); null otherwise
};
// the five buffers sized by the estimator's shape for nchains chains (S zero-initialised; on failure what was allocated is freed) / freed
int elph_i_greens_chain_scratch_alloc(elph_handle_s *h, int nchains, ElphGreensChainScratch *S);
void elph_i_greens_chain_scratch_free(ElphGreensChainScratch *S);
const ElphGreensChainScratch *elph_i_greens_own_scratch(elph_handle_s *h);      // the estimator's (null before elph_greens_create)
// one step of the loop over pairs v1 < v2 of a chain's vectors: the four tables of the pair into S.C; in the estimator's own scratch the
// doubled complex copies are refreshed for the last pair.  p: chain 0's vectors; chain c's lie c ndim further.  No synchronisation.
int elph_i_greens_setup_chains_dev(elph_handle_s *h, const ElphGreensChainScratch &S, int v1, int v2, ElphGreensPair *p);
int elph_i_greens_autocorr_chains_dev(elph_handle_s *h, const ElphGreensChainScratch &S, double *outS, const double *vS);
// greens_noise.hip: nvec vectors of ndim standard normals of batch `seed` (rng_dev.h), numbered in the reference layout, into dstS (layout S).
// mapping of Box-Muller pairs to threads: 0 pair-indexed, 1 site-fastest (even Ltau only), -1 the one the estimator ships.  Stream-ordered.
int elph_i_greens_randn(elph_handle_s *h, double *dstS, uint64_t seed, int64_t nvec, int mapping = -1);
int elph_launch_r2s(elph_handle_s *h, double *dstS, const double *srcR, int nvec, int ncols = 0);
int elph_launch_s2r(elph_handle_s *h, double *dstR, const double *srcS, int nvec, int ncols = 0);
int elph_launch_expV(elph_handle_s *h, const double *xR, double dtau, int chain = 0);
int elph_launch_ssh_update(elph_handle_s *h, const double *x_dev, int nph, const int *cb0_dev, const double *par_dev,
                           const double *tbare_dev, const int *slot_dev, double dtau, int x_tau_major = 0, int nch = 1);
int elph_launch_cs_bar(elph_handle_s *h, double *cbar_dev, double *sbar_dev, int nch = 1);
int elph_launch_ssh_scatter(elph_handle_s *h, double *F_dev, const double *q_dev, const double *x_dev, const double *par_dev,
                            const int *cb0_dev, int nph, double dtau, int tau_major = 0, double scale = 1.0, int nch = 1);
int elph_i_ssh_upload_params(elph_handle_s *h, int64_t nph, const int64_t *cb_index, const double *t_ph, const double *alpha,
                             const double *alpha2, const double *t_bare_cb, const double *mu);
int elph_launch_mul(elph_handle_s *h, int which /*0 M, 1 MT, 2 MTM*/, double *yS, const double *vS, int nvec);
int elph_launch_cg_init(elph_handle_s *h, int nrhs, int use_prec, bool x_zero = false);   // x_zero: work.x was zeroed by the library for THIS solve
int elph_launch_cg_iteration(elph_handle_s *h, int nrhs, int use_prec);
int elph_launch_cg_kernel(elph_handle_s *h, int nrhs, int which /*0 = k_cg_ap, 1 = k_cg_xr*/);
int elph_launch_residual(elph_handle_s *h, int nrhs);
int elph_launch_cg_init_only(elph_handle_s *h, int nrhs);
int elph_launch_cg_state0_only(elph_handle_s *h, int nrhs);
int elph_launch_cg_init_prec_only(elph_handle_s *h, int nrhs);
int elph_launch_kpm_apply(elph_handle_s *h, double *zS, const double *rS, int nrhs, int cg_mode, int parts = 7);
// one side of the expansion (kernels.hip: k_kpm_cheb_side): transposed 0 Left ~ M⁻¹, 1 Right ~ M⁻ᵀ; done: [nrhs] skip flags or nullptr
int elph_launch_kpm_apply_side(elph_handle_s *h, double *zS, const double *rS, int nrhs, int transposed, const int *done);
// The launch shape of the LDS-slab Chebyshev kernels (k_kpm_cheb, k_kpm_cheb_side), a pure function of the handle: cbs threads per workgroup,
// npl = ceil(N / cbs) sites per thread, shm bytes of slab, tab bytes of bond program, which rides in LDS next to the slab when lds_tables = 1.
// The one-sided kernel is instantiated for npl <= ELPH_SIDE_NPL_MAX.
struct KpmSlabShape { int cbs, npl, lds_tables; size_t shm, tab; };
constexpr int ELPH_SIDE_NPL_MAX = 6;
KpmSlabShape elph_kpm_slab_shape(const elph_handle_s *h);
void elph_msolve_free(elph_handle_s *h);                                    // msolve.hip
// msolve.hip internals used by hmc.hip, langevin.hip, greens.hip and force.hip: the handle's solver kind (BiCGStab or GMRES, never CG) on
// device-resident layout-S vectors.  Both consume the h->x_zero promise of their caller (x was zeroed by the library for THIS solve).
// ldiv!(x, model, b[, P]; maxiter) for A = M (transposed 0) or Mᵀ (1), use_prec: the Left / the Right side of the expansion
int elph_i_mldiv_core(elph_handle_s *h, int transposed, int nrhs, int use_prec, int64_t maxiter, double *x, const double *b, int64_t *iters,
                      double *resid, int *flag);
int elph_i_msolve_ready(elph_handle_s *h);      // ELPH_E_STATE, naming the solver, where the handle's BiCGStab / GMRES cannot run (sharded, slab, restricted range)
// O⁻¹ b as the reference's mul_by_M branch of calc_O⁻¹Λϕ! runs it (HMC.jl:851-903): Mᵀ y = b from y = 0 with the Right side, then M x = y
// from x = 0 with the Left side, y read where the first stage left it; b is not written.  iters2, flag2: [2 stages][nrhs]
int elph_i_msolve_pair(elph_handle_s *h, int nrhs, int use_prec, double *x, double *y, const double *b, int64_t *iters2, int *flag2);
// what calc_O⁻¹Λϕ! returns for each of nch chains from the stages of such a pair solve of the 2 nch right-hand sides, it4 / fl4:
// [2 stages][2 signs][nch]: iters± = it₁± + it₂±, flag± = max(flag₁±, flag₂±) (:863-876), then as elph_fold_pair; zero_minus[c] (may be
// null): ϕ₋ of chain c was suppressed and its output has to be zero
void elph_fold_pair_stages(int nch, const int64_t *it4, const int *fl4, int64_t *iters, int *flag, int *zero_minus);
int elph_launch_ebar(elph_handle_s *h, int nch = 1);
int elph_launch_fft_accel(elph_handle_s *h, double *outS, const double *inS, const double *diagS, double power, int64_t ncol,
                          int nvec = 1);
int elph_launch_tau_to_omega(elph_handle_s *h, double2 *nuS, const double *vS);
int elph_launch_omega_to_tau(elph_handle_s *h, double *vS, const double2 *nuS);
int elph_launch_zero(elph_handle_s *h, double *p, int64_t n);
int elph_launch_lambda_rhs(elph_handle_s *h, double *bS, const double *phiS, const double *xS, double dtau, int nch = 1);
int elph_launch_force_ssh(elph_handle_s *h, double *q, const double *XS, const double *US = nullptr, int nch = 1);
int elph_launch_dmdx_holstein(elph_handle_s *h, double *FS, const double *uS, const double *vS, const double *xS, double dtau,
                              double scale, int nch = 1);
int elph_launch_force_holstein(elph_handle_s *h, double *FS, const double *XS, const double *phiS, const double *xS, double dtau,
                               int nch = 1);

// ---- fast path (cg_fast.hip) ----------------------------------------------------------------
int elph_fast_mul(elph_handle_s *h, int which, double *yS, const double *vS, int nvec);
int elph_fast_cg_ap(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool fused = false);      // fused: the p/x-fused iteration (reads the ready p)
int elph_fast_cg_xr(elph_handle_s *h, const CgBufs &B, int nrhs, int parity);
// cg_sq16.hip: the p/x-fused k_cg_ap of the 16 x 16 square lattice with the checkerboard in registers (no LDS slabs)
bool elph_sq16_ap_usable(const elph_handle_s *h, int T);      // the shape; ELPH_SQ16_AP is elph_plan_cg's
int elph_sq16_cg_ap_px(elph_handle_s *h, const CgBufs &B, int nrhs, int parity);
// ---- one solve over several GPUs (cg_wg.hip, shard.hip): by-value description of this rank's shard for the resident kernel
#define ELPH_SHARD_MAXREC 256      // records of a meeting: ranks x workgroups per rank (8 x 20 at Ltau = 160; polled as 8 x 64 granules)
#define ELPH_SHARD_MAXRANKS 8
struct ElphShardCtl {
    int rank = 0, P = 1;
    int own_lo = 0, own_hi = 0;       // own sites [own_lo, own_hi) of the slab lattice; [0, own_lo) and [own_hi, N) are ghosts
    int n_to_prev = 0, n_to_next = 0; // own sites (from the bottom / from the top) that the previous / next rank holds as ghosts
    int cap_ghost = 0;                // capacity (sites) of a ghost region of the mailbox, the same on all ranks
    unsigned long long *mail[ELPH_SHARD_MAXRANKS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
extern "C" int elph_shard_shape(int64_t ltau, int world, int *waves, int *groups, int *records, int *max_records);   // shard.hip
int elph_wg_cg_shard(elph_handle_s *h, const CgBufs &B, long long fixed_iters, const ElphShardCtl &Sh, int *G_out);
// all ranks of a sharded solve whose slabs live on ONE device in one launch (cg_wg.hip; h_args pinned, d_args device: P x elph_wg_rank_args_bytes())
size_t elph_wg_rank_args_bytes();
int elph_wg_cg_ranks(elph_handle_s *const *hs, int P, const CgBufs *Bs, long long fixed_iters, const ElphShardCtl *ctls, void *h_args,
                     void *d_args, hipStream_t stream, long long timeout_ms, int *G_out);
int elph_i_shard_run_ranks(elph_handle_s *const *hs, int P, int nsets, void *h_args, void *d_args, double tol, int64_t maxiter, double kmax,
                           long long fixed_iters, long long timeout_ms, CgState *state_out, double *ms_out, double *const *hist_dev = nullptr,
                           long long hist_stride = 0);      // shard.hip
int elph_i_shard_create_local(elph_handle_s *h, int rank, int world, int64_t own_lo, int64_t own_n, int64_t n_to_prev, int64_t n_to_next,
                              int64_t cap_ghost, void *key_out);      // shard.hip: elph_shard_create for slabs that all live on one device (mailbox = ordinary device memory, not exported)
// ---- slabs.hip: the resident un-preconditioned solve of a lattice BEYOND one wave's slice (N > 320) as slabs of rows on the same device
bool elph_i_slabs_usable(elph_handle_s *h, int nrhs);      // builds the slabs on first use
int elph_i_slabs_solve(elph_handle_s *h, int nrhs, const CgParams &P, long long fixed_iters, int64_t *iters, bool *ran, double *ms_out);      // (P.record_hist: the eps histories go to h->work.hist)
void elph_i_slabs_free(elph_handle_s *h);

// ---- workgroup-resident CG (cg_wg.hip): the whole un-preconditioned solve in one launch
bool elph_wg_usable(const elph_handle_s *h, int *T, int *W, int *G, int nrhs = 1);
// the launch plan of a handle that need not own a device, as elph_bench_wg_plan reports it (world > 0: one rank of a sharded solve)
void elph_i_wg_plan_probe(const elph_handle_s *h, int nrhs, int world, int *out);
// x0_zero: the library zeroed work.x for this solve; x0_save: where the initial guess goes once the launch is decided, for the caller's
// fallback after a time-out (nullptr: not kept — a measurement launch)
int elph_wg_cg(elph_handle_s *h, const CgBufs &B, int nrhs, long long fixed_iters, bool x0_zero, double *x0_save, bool *ran);
// the resident solvers' control block for one launch (ResidentState): room for n_rec record words + n_extra words behind them + the abort
// word, zeroed when it grows or the 32-bit tags would wrap; *R comes back with slots, abort, epoch0 (a range of `span` tags of its own)
// and timeout_ticks filled, bnd = nullptr, everything else 0.  WG_TAGS_RESTART (a sharded launch: its records live in the ranks'
// mailboxes under one numbering for all) zeroes the block every time and numbers from 0 — no span.
namespace wg { struct WgCtl; }
enum WgTags { WG_TAGS_RUNNING, WG_TAGS_RESTART };
int elph_wg_ctl(elph_handle_s *h, size_t n_rec, size_t n_extra, unsigned long long span, long long timeout_ms, WgTags tags, wg::WgCtl *R);
// tags of one launch: one per iteration + 2
inline unsigned long long elph_wg_tag_span(const CgParams &P, long long fixed_iters) {
    return (unsigned long long)std::min<long long>(fixed_iters > 0 ? fixed_iters : P.maxiter, 1LL << 30) + 2;
}
int elph_wg_aborted(const elph_handle_s *h, bool *aborted); // after the stream has drained: was the abort word raised?  (reads only)
void elph_wg_timed_out(elph_handle_s *h);                   // THE record of a time-out: cool-down, fallback count, message
bool elph_pg_cheb_usable(const elph_handle_s *h);
bool elph_pg_disorder_ok(const elph_handle_s *h);      // hopping disorder on this handle's patch shape (pgrid.hip)                       // pgrid.hip
int elph_pg_kpm_cheb(elph_handle_s *h, int nrhs, const CgState *st, double *rz_part = nullptr, int nrz = 0, const double *rr_part = nullptr);
bool elph_pg_ap_usable(const elph_handle_s *h);
bool elph_pg_mw();                                          // ELPH_PG_MW: patch shapes of several wavefronts per slice allowed (pgrid.hip)
bool elph_pg_mul_usable(const elph_handle_s *h);
int elph_pg_mul(elph_handle_s *h, const ModelDev &m, int which, double *yS, const double *vS, int nvec);
// the time-axis chunking of one k_mul_pg / k_cg_ap_pg launch (pgrid.hip): T slices per workgroup, nch chunks per vector, the last of `last` slices
struct PgChunks { int T, nch, last; };
enum { PG_K_MUL = 0, PG_K_CG_AP = 1, PG_K_CG_AP_PX = 2 };
PgChunks elph_pg_chunks(int kernel, int px, int py, int nw, bool honeycomb, long long nvec, int L);      // pure but for the pin ELPH_PG_T
void elph_pg_chunk_probe(const elph_handle_s *h, int kernel, int nvec, int *out);                         // out[7] = px, py, nw, T, nch, last, taken
int elph_pg_cg_ap(elph_handle_s *h, const CgBufs &B, const ModelDev &m, int nrhs, int parity, bool fused = false);      // fused: the p/x-fused iteration (reads the ready p)
int elph_wg_cooldown_step(elph_handle_s *h);                // one solve of the cool-down after a time-out (both resident kernels call it)
long long elph_shard_timeout_ms();                          // wait bound of the sharded solves (shard.hip)
long long elph_wg_timeout_ms(long long dflt);               // ELPH_WG_TIMEOUT_MS, dflt when unset (cg_wg.hip)
int elph_wg_cooldown();                                     // ELPH_WG_COOLDOWN (cg_wg.hip)
char elph_slabs_test_timeout();                             // first character of ELPH_SLABS_TEST_TIMEOUT, 0 when unset (cg_wg.hip)
// ---- workgroup-resident KPM-preconditioned CG (pcg_wg.hip): the whole preconditioned solve of 1..8 right-hand sides in one launch
bool elph_pcg_wg_usable(const elph_handle_s *h, int nrhs);
int elph_pcg_wg(elph_handle_s *h, const CgBufs &B, int nrhs, long long fixed_iters, double *x0_save, bool *ran);      // x0_save: as elph_wg_cg's
CgBufs elph_make_bufs(elph_handle_s *h, int nrhs);
// reg: the plan's reg_cheb (the register-exchange recursion where elph_reg_cheb_form has one); rz_part: the r.z partials in frequency space
int elph_fast_kpm_cheb(elph_handle_s *h, int nrhs, const CgState *st, bool reg, double *rz_part = nullptr, int nrz = 0,
                       const double *rr_part = nullptr, int fold_nct = 0);
enum RegCheb { REG_NONE, REG_SQ, REG_SQ_GRID, REG_HC_GRID, REG_HC12 };
int elph_reg_cheb_form(const elph_handle_s *h, int *hgn = nullptr);      // cg_fast.hip: the lane family's register-exchange recursion of this lattice
int elph_choose_T(const elph_handle_s *h, int nrhs);
int elph_choose_T_px(const elph_handle_s *h, int nrhs, bool two_streams);      // the p/x-fused kernel's own rule (three waves per SIMD); nrhs in flight
CgPlan elph_plan_cg(const elph_handle_s *h, int nrhs, bool prec, int in_flight);      // kernels.hip: mutates nothing
// packs per-bond values (order of h_bi/h_bj) into the lane-program layout [NE][64] (idle slots = fill)
void elph_lp_pack(const elph_handle_s *h, const double *per_bond, double *out, double fill);

// ---- tau-axis transforms (dft.hip; the planner and the matrix-core forms in dft_mfma.hip, long axes in dft_big.hip) ------------------------
constexpr int ELPH_DFT_TPT = 2;                             // time slices per wave of the scalar inverse (its r.z slots: ceil(L / TPT) per site tile)
DftShape dft_shape(int64_t L);                              // pure: no HIP calls
DftSwitches dft_switches();                                 // the one reader of the five switches; called per plan
// which: DftKind; nrz_slots: the r.z partial slots offered by an inverse that has to deliver them, else 0
DftPlan elph_plan_dft(const DftShape &S, const DftSwitches &sw, int which, bool inverse, int N, int nvec, int nrz_slots);
DftPlan elph_dft_split_plan(const DftShape &S, bool inverse);      // the even/odd split's form and table alone (the fused launches below)
void elph_dft_pair(DftPlan &fwd, DftPlan &inv);             // fourier_accelerate's plain pair: the matrix cores only when both directions take them
void elph_i_dft_plan_probe(const DftShape &S, int which, bool inverse, int N, int nvec, int nrz_slots, int *out);      // _lib.DFT_PLAN_SLOTS
int elph_dft_build_tables(elph_handle_s *h);                // h->dft: with elph_dft_free the only allocator / freer of its tables
void elph_dft_free(elph_handle_s *h);
int elph_dft_upload(void **dev, const void *src, size_t bytes);
int elph_dft_fwd_twisted(elph_handle_s *h, double2 *nu, const double *vS, int N, int nrhs, const CgState *st);
int elph_dft_inv_twisted(elph_handle_s *h, double *outS, const double2 *nu, int N, int nrhs, const CgState *st,
                         const double *rvec, double *rz_part, int nrz);
int elph_dft_fwd_plain(elph_handle_s *h, double2 *nu, const double *vS, int N, int nrhs);
int elph_dft_inv_plain(elph_handle_s *h, double *outS, const double2 *nu, int N, int nrhs);
int elph_dft_accel(elph_handle_s *h, double *outS, const double *inS, const double *diagS, double power, int N, double2 *u,
                   int nvec = 1);
// the launches of a plan's form: DFT_ONE_TILE, DFT_DIRECT, DFT_SPLIT_* (dft_mfma.hip) and DFT_BIG_* (dft_big.hip)
int elph_dft_mfma_run(elph_handle_s *h, const DftPlan &p, int which, bool inverse, double *out, const double *in, int N, int nrhs,
                      const CgState *st, const double *rvec, double *rz_part, int nrz);
int elph_dft_mfma_build_tables(elph_handle_s *h);
int elph_dft_mfma_fwd_xr(elph_handle_s *h, double2 *nu, double *rS, const double *zS, const double *pap, int npap, double *rr,
                         double *alpha, int N, int nrhs, const CgState *st, const double *fold = nullptr, int fold_nch = 1,
                         double *frz = nullptr, int fnrz = 0, int fslot0 = 0);
int elph_dft_mfma_inv_px(elph_handle_s *h, const double2 *nu, int N, int nrhs, const CgState *st, double *pS, double *xS,
                         const double *alpha, const double *rz, int nrz);
int elph_dft_big_build_tables(elph_handle_s *h);
int elph_dft_big_fwd(elph_handle_s *h, DftForm form, bool twisted, double2 *nu, const double *vS, int N, int nvec);
int elph_dft_big_inv(elph_handle_s *h, DftForm form, bool twisted, double *outS, const double2 *nu, int N, int nvec, const double *rvec,
                     double *rz_part, int nrz);

// ---- host-side KPM setup (kpm_host.cpp) ---------------------------------------------------
void elph_kpm_coefficients(double *c_z, int order, double lam_lo, double lam_hi, double phi);
// one chain for its bounds: acceptance window, hysteresis, orders and coefficients; true when the chain's tables change (moved, turned on
// or off, or never uploaded)
bool elph_kpm_plan_chain(const KpmParams &p, int L, double e_min, double e_max, KpmChain &C);
KpmTables elph_kpm_tables(int L, const std::vector<KpmChain> &chains);
// every chain of K for its bounds eb[nch][2] (e_min, e_max); rebuilds K.tab when a chain changed or K is not ready, and says so (the
// caller then uploads the tables)
bool elph_kpm_plan(KpmState &K, int L, const double *eb);
void elph_kpm_free(elph_handle_s *h);      // kpm_setup.hip: the device buffers of h->kpm; h->kpm back to its initial state
int elph_kpm_arnoldi(const elph_handle_s *h, int chain, const double *b_max, const double *b_min, double *e_min,
                     double *e_max);
int elph_hess_eigvals(std::vector<double> &a, int n, std::vector<double> &wr, std::vector<double> &wi);
int elph_kpm_bounds_dev(elph_handle_s *h, int nch, const double *d_bstart, double *d_eout);
int elph_hess_max_real_dev(elph_handle_s *h, int nmat, int n, const double *A, double *out);      // kpm_dev.hip: the device QR iteration alone
