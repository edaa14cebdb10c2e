// elph_api.hip — extern "C" entry points of libelphgpu.so (include/elph_gpu.h).
// Host orchestration only: argument checks, layout staging, the CG chunk loop and the ldiv!
// flag logic (Models.jl:74-186).  All arithmetic on lattice vectors happens in kernels.hip.
// There is NO CPU fallback: without a gfx950 device every compute entry point fails.

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <numeric>


#include "elph_internal.h"
#include "pgrid_dev.h"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------

static thread_local char g_err[512] = "";

void elph_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int elph_launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { elph_set_error("launch %s failed: %s", what, hipGetErrorString(e)); return ELPH_E_HIP; }
    return ELPH_OK;
}

extern "C" const char *elph_last_error(void) { return g_err; }
extern "C" int elph_abi_version(void) { return ELPH_ABI_VERSION; }
// the build record: written by elphdynamics_amd/build.py into a translation unit of its own at every link
extern "C" const char elph_build_info_text[];
extern "C" const char *elph_build_info(void) { return elph_build_info_text; }

extern "C" int elph_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

template <class T>
static int dev_alloc(T **p, size_t n) {
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; }
    if (n == 0) n = 1;
    HIPCHK(hipMalloc((void **)p, n * sizeof(T)));
    return ELPH_OK;
}

// the number of phonon configurations resident in the handle; the KPM expansion is per chain, so a change invalidates it
static void set_nchains(elph_handle_s *h, int n) {
    if (h->nchains != n) { h->nchains = n; h->kpm.ready = false; }
}

// ------------------------------------------------------------------------------------------
// lane program (cg_fast.hip): bonds re-packed [colour][pass][lane]
// ------------------------------------------------------------------------------------------

void elph_lp_pack(const elph_handle_s *h, const double *per_bond, double *out, double fill) {
    const int PP = (h->npl + 1) / 2, NE = h->lp_mc * PP;
    for (int i = 0; i < NE * ELPH_WAVE; ++i) out[i] = fill;
    for (int col = 0; col < h->ncol && col < h->lp_mc; ++col) {
        const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
        for (int n = b0; n < b1; ++n) {
            const int k = n - b0;
            out[(col * PP + k / ELPH_WAVE) * ELPH_WAVE + (k % ELPH_WAVE)] = per_bond[n];
        }
    }
}

static LatticeShape elph_recognise_lattice(const elph_handle_s *h);

// the host half: colours per program, the (i, j) words of every lane, whether the lane-program kernels apply, the recognised lattice
static void plan_lane_program(elph_handle_s *h) {
    h->lp_mc = (h->ncol <= 4) ? 4 : 6;      // kernels exist for 4-colour (square, honeycomb, chain) and 6-colour (triangular) programs
    const int PP = (h->npl + 1) / 2, NE = h->lp_mc * PP;
    h->lp_ne = NE;
    const char *ct = getenv("ELPH_CHUNK_T");
    h->force_T = ct ? atoi(ct) : 0;
    const char *nf = getenv("ELPH_NO_FAST");
    h->fast = (h->ncol <= 6) && (h->npl <= ELPH_MAX_NPL) && !(nf && nf[0] == '1');
    // idle slots (ragged colours / fewer than 4 colours): each lane owns two padding slots of the LDS slab,
    // paired with (cosh, sinh) = (1, 0) by elph_lp_pack => a no-op bond, no predicate in the kernels
    h->h_lp_ij.resize((size_t)NE * ELPH_WAVE);
    for (int e = 0; e < NE; ++e)
        for (int l = 0; l < ELPH_WAVE; ++l) {
            const unsigned i = (unsigned)(h->npl * ELPH_WAVE + 2 * l);
            h->h_lp_ij[(size_t)e * ELPH_WAVE + l] = i | ((i + 1) << 16);
        }
    if (h->fast) {
        for (int col = 0; col < h->ncol; ++col) {
            const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
            if (b1 - b0 > PP * ELPH_WAVE) { h->fast = false; break; }
            for (int n = b0; n < b1; ++n) {
                const int k = n - b0;
                h->h_lp_ij[(size_t)(col * PP + k / ELPH_WAVE) * ELPH_WAVE + (k % ELPH_WAVE)] =
                    (unsigned)h->h_bi[n] | ((unsigned)h->h_bj[n] << 16);
            }
        }
    }
    h->fast_capable = h->fast;
    h->shape = elph_recognise_lattice(h);
}

static int build_lane_program(elph_handle_s *h) {
    plan_lane_program(h);
    const int NE = h->lp_ne;
    RC(dev_alloc(&h->d_lp_ij, (size_t)NE * ELPH_WAVE));
    HIPCHK(hipMemcpy(h->d_lp_ij, h->h_lp_ij.data(), sizeof(unsigned) * NE * ELPH_WAVE, hipMemcpyHostToDevice));
    const size_t ntau = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1;
    RC(dev_alloc(&h->d_lp_c, ntau * NE * ELPH_WAVE));
    RC(dev_alloc(&h->d_lp_s, ntau * NE * ELPH_WAVE));
    if (h->shape.sq_L() > 0) {
        RC(dev_alloc(&h->d_sq_bond, (size_t)4 * h->N));
        HIPCHK(hipMemcpy(h->d_sq_bond, h->shape.bond.data(), sizeof(int) * 4 * h->N, hipMemcpyHostToDevice));
    }
    if (h->shape.kind == LatticeShape::SQUARE && h->shape.patch()) {      // the site -> bond map of the colouring: hopping disorder in the patch layout (pgrid.hip)
        RC(dev_alloc(&h->d_pg_bond, (size_t)4 * h->N));
        HIPCHK(hipMemcpy(h->d_pg_bond, h->shape.bond.data(), sizeof(int) * 4 * h->N, hipMemcpyHostToDevice));
    }
    return ELPH_OK;
}

// Lattice recognition: the colouring elph_create found is matched against the reference's colourings of periodic square, honeycomb and triangular
// lattices.  Any deviation (other lattice, other bond order) leaves the shape NONE, and the LDS kernels are used.

// square LX x LY (site = x + LX y), colours [x-even | x-odd | y-even | y-odd]; fills bond ([4][N] the bond covering site i in colour col)
static bool match_square(const elph_handle_s *h, int LX, int LY, std::vector<int> &bond) {
    bond.assign((size_t)4 * h->N, -1);
    for (int col = 0; col < 4; ++col) {
        const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
        if (b1 - b0 != h->N / 2) return false;
        for (int n = b0; n < b1; ++n) {
            const int i = h->h_bi[n], j = h->h_bj[n];
            const int xi = i % LX, yi = i / LX, xj = j % LX, yj = j / LX;
            bool ok = false;
            // expected partner of site (x,y): col 0: x^1 ; col 1: x odd -> x+1, even -> x-1 ; cols 2,3 the same along y
            auto partner = [](int x, int colpar, int L) { return colpar == 0 ? (x ^ 1) : ((x & 1) ? (x + 1) % L : (x + L - 1) % L); };
            if (col < 2) ok = (yi == yj) && (partner(xi, col, LX) == xj) && (partner(xj, col, LX) == xi);
            else ok = (xi == xj) && (partner(yi, col - 2, LY) == yj) && (partner(yj, col - 2, LY) == yi);
            if (!ok) return false;
            bond[(size_t)col * h->N + i] = n;
            bond[(size_t)col * h->N + j] = n;
        }
    }
    for (int v : bond) if (v < 0) return false;
    return true;
}

// honeycomb of LX x LY two-site cells (site = 2 (x + LX y) + orbital), colours [A-B of a cell | B(x,y)-A(x+1,y) | B(x,y)-A(x,y+1)] (the bond
// definitions of examples/holstein_hmc_honeycomb.toml through Checkerboard.jl:471-515)
static bool match_honeycomb(const elph_handle_s *h, int LX, int LY) {
    std::vector<char> seen((size_t)3 * h->N, 0);
    for (int col = 0; col < 3; ++col) {
        const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
        if (b1 - b0 != LX * LY) return false;
        for (int n = b0; n < b1; ++n) {
            int i = h->h_bi[n], j = h->h_bj[n];
            if (i & 1) std::swap(i, j);                      // i: the A site (orbital 0), j: the B site
            if ((i & 1) != 0 || (j & 1) != 1) return false;
            const int ca = i >> 1, cb = j >> 1, xa = ca % LX, ya = ca / LX, xb = cb % LX, yb = cb / LX;
            bool ok = false;
            if (col == 0) ok = (ca == cb);
            else if (col == 1) ok = (ya == yb) && (xa == (xb + 1) % LX);
            else ok = (xa == xb) && (ya == (yb + 1) % LY);
            if (!ok || seen[(size_t)col * h->N + i] || seen[(size_t)col * h->N + j]) return false;
            seen[(size_t)col * h->N + i] = seen[(size_t)col * h->N + j] = 1;
        }
    }
    return true;
}

// even-L triangular (site = x + L y; bonds (1,0), (0,1), (1,-1): examples/holstein_hmc_triangular.toml), colours [x-even | x-odd | y-even |
// diagonal from even y | y-odd | diagonal from odd y], the diagonal of (x, y) ending at (x - 1, y + 1)
static bool match_triangular(const elph_handle_s *h, int L) {
    auto partner = [L](int col, int x, int y, int *px_, int *py_) {
        const int xp = (x + 1) % L, xm = (x + L - 1) % L, yp = (y + 1) % L, ym = (y + L - 1) % L;
        switch (col) {
            case 0: *px_ = x ^ 1; *py_ = y; break;
            case 1: *px_ = (x & 1) ? xp : xm; *py_ = y; break;
            case 2: *px_ = x; *py_ = y ^ 1; break;
            case 3: if (!(y & 1)) { *px_ = xm; *py_ = yp; } else { *px_ = xp; *py_ = ym; } break;
            case 4: *px_ = x; *py_ = (y & 1) ? yp : ym; break;
            default: if (y & 1) { *px_ = xm; *py_ = yp; } else { *px_ = xp; *py_ = ym; } break;
        }
    };
    std::vector<char> seen((size_t)6 * h->N, 0);
    for (int col = 0; col < 6; ++col) {
        const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
        if (b1 - b0 != h->N / 2) return false;
        for (int n = b0; n < b1; ++n) {
            const int i = h->h_bi[n], j = h->h_bj[n];
            int qx, qy;
            partner(col, i % L, i / L, &qx, &qy);
            if (qx + L * qy != j) return false;
            partner(col, j % L, j / L, &qx, &qy);
            if (qx + L * qy != i) return false;
            if (seen[(size_t)col * h->N + i] || seen[(size_t)col * h->N + j]) return false;
            seen[(size_t)col * h->N + i] = seen[(size_t)col * h->N + j] = 1;
        }
    }
    return true;
}

// simple cubic L x L x L (site = x + L (y + L z); bonds (1,0,0), (0,1,0), (0,0,1)), colours [x-even | x-odd | y-even | y-odd | z-even | z-odd]: what
// the greedy colouring gives even extents of at least 4 (an odd extent mixes the directions inside the colours and fails here)
static bool match_cubic(const elph_handle_s *h, int L) {
    auto partner = [L](int col, int i) {
        int r[3] = {i % L, (i / L) % L, i / (L * L)};
        int &a = r[col >> 1];
        a = (col & 1) ? ((a & 1) ? (a + 1) % L : (a + L - 1) % L) : (a ^ 1);
        return r[0] + L * (r[1] + L * r[2]);
    };
    std::vector<char> seen((size_t)6 * h->N, 0);
    for (int col = 0; col < 6; ++col) {
        const int b0 = h->h_coloff[col], b1 = h->h_coloff[col + 1];
        if (b1 - b0 != h->N / 2) return false;
        for (int n = b0; n < b1; ++n) {
            const int i = h->h_bi[n], j = h->h_bj[n];
            if (partner(col, i) != j || partner(col, j) != i) return false;
            if (seen[(size_t)col * h->N + i] || seen[(size_t)col * h->N + j]) return false;
            seen[(size_t)col * h->N + i] = seen[(size_t)col * h->N + j] = 1;
        }
    }
    return true;
}

// The shape of a handle's lattice from its coloured bond table, its model kind and its hopping table (h_bi, h_bj, h_coloff, kind, h_c, h_s);
// reads nothing else of the handle and changes nothing.  ELPH_PG_MW=0 (pgrid.hip: elph_pg_mw) keeps the patch shapes to one wavefront per slice.
static LatticeShape elph_recognise_lattice(const elph_handle_s *h) {
    LatticeShape s;
    const bool hol = h->kind == ELPH_MODEL_HOLSTEIN;
    if (hol && h->nb > 0) {      // the model's own hopping table: Holstein tables never change after elph_create
        bool uni = true;
        for (int64_t n = 1; n < h->nb && uni; ++n) uni = (h->h_c[(size_t)n] == h->h_c[0] && h->h_s[(size_t)n] == h->h_s[0]);
        if (uni) { s.hop_uniform = true; s.hop_c = h->h_c[0]; s.hop_s = h->h_s[0]; }
    }
    const int64_t N = h->N;
    if (h->ncol == 4 && h->nb == 2 * N && N >= 16) {
        // the square up to 16 x 16 first, then every even LX x LY with LX LY = N whose 2 x 2 patches fit the 64 lanes of a wave (the slab of a
        // sharded solve: its rows closed into a ring): the register-exchange forms (GRID layout; DPP layouts of their own for 8 x 8, 16 x 16)
        std::vector<std::pair<int, int>> cand;
        for (int l = 4; l <= 16; l += 2) if ((int64_t)l * l == N) cand.push_back({l, l});
        for (int lx = 4; lx <= 32; lx += 2)
            if (N % lx == 0) { const int ly = (int)(N / lx); if (ly >= 4 && ly % 2 == 0 && lx != ly && (lx / 2) * (ly / 2) <= 64) cand.push_back({lx, ly}); }
        for (auto &c : cand)
            if (match_square(h, c.first, c.second, s.bond)) {
                s.kind = LatticeShape::SQUARE; s.LX = c.first; s.LY = c.second; s.GX = c.first / 2; s.GY = c.second / 2;
                return s;
            }
        // a larger square lattice: PX x PY patches per lane (pgrid_dev.h) — the Chebyshev recursion of the preconditioner in registers
        int l = 18;
        while (l <= 64 && (int64_t)l * l != N) l += 2;
        int px = 0, py = 0, nw = 1;
        // no patch that fits one wavefront: several wavefronts per slice, the patch edges through LDS (ELPH_PG_MW=0: the generic kernels, A/B)
        if (l <= 64 && (pgrid::pick_patch(l, &px, &py) || (elph_pg_mw() && pgrid::pick_patch_mw(l, &px, &py, &nw)))) {
            // hopping disorder on 28 x 28 / 32 x 32: 2 x 2 patches on four wavefronts instead of 4 x 4 on one — 12 table entries per thread instead of 40
            // (measured, profiles/r06/hopping_disorder_patch_kernels_with_tables.log); ELPH_PG_MW=0 keeps the one-wavefront shape
            // (... and 30 x 30, whose 2 x 10 patches have no table variant: 15 x 15 threads on four wavefronts)
            if (hol && !s.hop_uniform && nw == 1 && ((px == 4 && py == 4) || (px == 2 && py == 10)) && elph_pg_mw()) { px = 2; py = 2; nw = ((l / 2) * (l / 2) + 63) / 64; }
            if (match_square(h, l, l, s.bond)) {
                s.kind = LatticeShape::SQUARE; s.LX = s.LY = l; s.PX = px; s.PY = py; s.NW = nw;
                return s;
            }
        }
        s.bond.clear();
    } else if (h->ncol == 3 && !(N & 1) && h->nb == 3 * (N / 2) && N >= 8) {
        // honeycomb: square first, then rectangles (12 x 12 has the DPP / quad forms; beyond 16 x 16 cells, PX x PY cells per lane)
        const int cells = (int)(N / 2);
        std::vector<std::pair<int, int>> cand;
        for (int l = 2; l <= 64; ++l) if (l * l == cells) cand.push_back({l, l});
        for (int lx = 2; lx <= 32; ++lx)
            if (cells % lx == 0) { const int ly = cells / lx; if (ly >= 2 && lx != ly) cand.push_back({lx, ly}); }
        for (auto &c : cand) {
            if (!match_honeycomb(h, c.first, c.second)) continue;
            s.kind = LatticeShape::HONEYCOMB; s.LX = c.first; s.LY = c.second;
            int px = 0, py = 0, nw = 1;
            if (c.first == c.second && c.first > 16 &&
                (pgrid::pick_hpatch(c.first, &px, &py) || (elph_pg_mw() && pgrid::pick_hpatch_mw(c.first, &px, &py, &nw)))) {
                s.PX = px; s.PY = py; s.NW = nw;
            }
            return s;
        }
    } else if (h->ncol == 6 && h->nb == 3 * N && N >= 16) {
        // triangular: the patch-layout kernels (pgrid::Tri); up to 16 x 16 also the GRID layout of the resident CG (cg_wg.hip: FORM 7)
        int L = 0;
        for (int l = 4; l <= 64; l += 2) if ((int64_t)l * l == N) L = l;
        int px = 0, py = 0;
        if (L && pgrid::pick_tpatch(L, &px, &py) && match_triangular(h, L)) {
            s.kind = LatticeShape::TRIANGULAR; s.LX = s.LY = L; s.PX = px; s.PY = py; s.NW = 1;
            if (L <= 16) s.GX = s.GY = L / 2;
            return s;
        }
        // simple cubic, Holstein with one (cosh, sinh) for every bond: 2 x 2 x 2 sites per thread (pgrid::Cu); hopping disorder, bond phonons and
        // every other box keep the kernels of an unrecognised lattice
        int Lc = 0, nw = 1;
        for (int l = 6; l <= 12; l += 2) if ((int64_t)l * l * l == N) Lc = l;
        if (Lc && hol && s.hop_uniform && pgrid::pick_cpatch(Lc, &nw) && (nw == 1 || elph_pg_mw()) && match_cubic(h, Lc)) {
            s.kind = LatticeShape::CUBIC; s.LX = s.LY = s.LZ = Lc; s.PX = s.PY = 2; s.NW = nw;
        }
    }
    return s;
}

// uploads the lane-program copy of the per-bond cosh/sinh tables (h_c/h_s)
static int upload_lp_cs(elph_handle_s *h) {
    if (!h->fast) return ELPH_OK;
    const int NE = h->lp_ne;
    const size_t ntau = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1, per = (size_t)NE * ELPH_WAVE;
    if (h->h_c.size() < ntau * (size_t)h->nb) return ELPH_OK;   // SSH before the first update_model
    std::vector<double> c(ntau * per), s(ntau * per);
    for (size_t t = 0; t < ntau; ++t) {
        elph_lp_pack(h, h->h_c.data() + t * (size_t)h->nb, c.data() + t * per, 1.0);
        elph_lp_pack(h, h->h_s.data() + t * (size_t)h->nb, s.data() + t * per, 0.0);
    }
    HIPCHK(hipMemcpy(h->d_lp_c, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_lp_s, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// life cycle
// ------------------------------------------------------------------------------------------

int elph_work_reserve(elph_handle_s *h, int nrhs) {
    SolveWork &W = h->work;
    if (nrhs <= W.cap_rhs) return ELPH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t Lo2 = (size_t)(h->L + 1) / 2, Lh = (size_t)h->L / 2 + 1, c = (size_t)nrhs;
    W.ndim = (size_t)h->ndim; W.nnu = Lo2 * (size_t)h->N; W.nrz = (size_t)h->L * (size_t)h->npl;
    for (double **v : {&W.stage_in, &W.stage_out, &W.b, &W.x, &W.r, &W.z, &W.zp, &W.tmp}) RC(dev_alloc(v, c * W.ndim));
    RC(dev_alloc(&W.p, 2 * c * W.ndim));
    RC(dev_alloc(&W.phi, 2 * W.ndim));
    RC(dev_alloc(&W.xfield, W.ndim));
    RC(dev_alloc(&W.sums, 4 * c * W.nrz));
    RC(dev_alloc(&W.state, 2 * c));
    RC(dev_alloc(&W.scal, 4 * c));
    RC(dev_alloc(&W.alpha, c));
    RC(dev_alloc(&W.nu, c * std::max(std::max(Lo2, Lh) * (size_t)h->N, W.ndim)));      // (the plain transforms' Lh frequencies fit too)
    if (W.h_state) HIPCHK(hipHostFree(W.h_state));
    if (W.h_scal) HIPCHK(hipHostFree(W.h_scal));
    HIPCHK(hipHostMalloc((void **)&W.h_state, 2 * c * sizeof(CgState), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&W.h_scal, 4 * c * sizeof(double), hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(W.sums, 0, 4 * c * W.nrz * sizeof(double), h->stream));
    W.cap_rhs = nrhs;
    return ELPH_OK;
}

void elph_work_release(elph_handle_s *h) {
    SolveWork &W = h->work;
    void *ptrs[] = {W.stage_in, W.stage_out, W.b, W.x, W.r, W.z, W.zp, W.tmp, W.p, W.nu, W.sums, W.state, W.alpha, W.scal, W.hist, W.phi, W.xfield};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (W.h_state) (void)hipHostFree(W.h_state);
    if (W.h_scal) (void)hipHostFree(W.h_scal);
    W = SolveWork();
}

// elements of a staged transfer; refuses one the staging buffers do not hold
static int staged_size(elph_handle_s *h, int nvec, int ncols, size_t *n) {
    *n = (size_t)nvec * (size_t)(ncols ? ncols : h->N) * (size_t)h->L;
    const size_t held = (size_t)h->work.cap_rhs * h->work.ndim;
    if (*n > held) { elph_set_error("staging %zu doubles, the staging buffers hold %zu", *n, held); return ELPH_E_STATE; }
    return ELPH_OK;
}

int elph_stage_in(elph_handle_s *h, double *dstS, const double *hostR, int nvec, int ncols) {
    size_t n = 0;
    RC(staged_size(h, nvec, ncols, &n));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, hostR, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return elph_launch_r2s(h, dstS, h->work.stage_in, nvec, ncols);
}

int elph_stage_out(elph_handle_s *h, double *hostR, const double *srcS, int nvec, int ncols) {
    size_t n = 0;
    RC(staged_size(h, nvec, ncols, &n));
    RC(elph_launch_s2r(h, h->work.stage_out, srcS, nvec, ncols));
    HIPCHK(hipMemcpyAsync(hostR, h->work.stage_out, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return ELPH_OK;
}

int elph_retry_in_slot0(elph_handle_s *h, int r, const std::function<int()> &solve_and_flag, double *x, double *b) {
    SolveWork W = h->work;
    if (x) W.x = x;
    if (b) W.b = b;
    const size_t bytes = W.ndim * sizeof(double);
    if (r != 0) {
        HIPCHK(hipMemcpyAsync(W.stage_out, W.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.stage_in, W.b, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.x, W.x + r * W.ndim, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.b, W.b + r * W.ndim, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    if (h->nchains > 1) h->solo_chain = r % h->nchains;   // slot 0 must keep rhs r's fermion matrix
    const int rc = solve_and_flag();
    h->solo_chain = -1;
    RC(rc);
    if (r != 0) {
        HIPCHK(hipMemcpyAsync(W.x + r * W.ndim, W.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.x, W.stage_out, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(W.b, W.stage_in, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return ELPH_OK;
}

void elph_fold_pair(int nch, const int64_t *it2, const int *fl2, int64_t *iters, int *flag) {
    for (int c = 0; c < nch; ++c) {
        int64_t tot = it2[c];
        int fl = fl2[c];
        if (fl == 0) { tot += it2[nch + c]; fl = fl2[nch + c]; }      // a failed first solve suppresses the second (:880)
        if (fl == 0) tot = (tot + 1) / 2;                             // cld(iters, 2)  (:907-909)
        iters[c] = tot;
        flag[c] = fl;
    }
}

void elph_fold_pair_stages(int nch, const int64_t *it4, const int *fl4, int64_t *iters, int *flag, int *zero_minus) {
    const size_t n2 = 2 * (size_t)nch;                                   // it4, fl4: [stage][sign][chain]
    std::vector<int64_t> it2(n2);
    std::vector<int> fl2(n2);
    for (size_t r = 0; r < n2; ++r) {
        it2[r] = it4[r] + it4[n2 + r];                                   // iters += iters′ of the second stage (:863, :871)
        fl2[r] = std::max(fl4[r], fl4[n2 + r]);                          // flag = max(flag, flag′) (:864, :872)
    }
    elph_fold_pair(nch, it2.data(), fl2.data(), iters, flag);
    if (zero_minus) for (int c = 0; c < nch; ++c) zero_minus[c] = fl2[c] != 0;
}

// the bond-table arguments of elph_create (and of the recognition probe)
static int check_bond_table(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht, const double *sinht) {
    if (nbonds > 0 && !neighbor_table) { elph_set_error("neighbor_table is null"); return ELPH_E_ARG; }
    if (kind == ELPH_MODEL_HOLSTEIN && nbonds > 0 && (!cosht || !sinht)) { elph_set_error("cosht/sinht null"); return ELPH_E_ARG; }
    for (int64_t n = 0; n < nbonds; ++n) {
        const int64_t i = neighbor_table[2 * n], j = neighbor_table[2 * n + 1];
        if (i < 1 || i > nsites || j < 1 || j > nsites || i == j) {
            elph_set_error("neighbor_table[:,%lld] = (%lld,%lld) out of range 1..%lld", (long long)n + 1, (long long)i, (long long)j, (long long)nsites);
            return ELPH_E_ARG;
        }
    }
    return ELPH_OK;
}

// bond tables, 0-based; colours = maximal runs of site-disjoint bonds (reproduces the groups of checkerboard_groups!,
// Checkerboard.jl:471-515, for any table in checkerboard order, and stays correct — only slower — for an arbitrary bond order).
// Host only: h->N and h->nb are set, the table has been range-checked.
static void colour_bonds(elph_handle_s *h, const int64_t *neighbor_table) {
    h->h_bi.resize(h->nb); h->h_bj.resize(h->nb);
    h->h_coloff.assign(1, 0);
    std::vector<char> used(h->N, 0);
    for (int64_t n = 0; n < h->nb; ++n) {
        const int i = (int)(neighbor_table[2 * n] - 1), j = (int)(neighbor_table[2 * n + 1] - 1);
        if (used[i] || used[j]) {
            h->h_coloff.push_back((int)n);
            std::fill(used.begin(), used.end(), 0);
        }
        used[i] = used[j] = 1;
        h->h_bi[n] = i; h->h_bj[n] = j;
    }
    if (h->nb > 0) h->h_coloff.push_back((int)h->nb);
    h->ncol = (int)h->h_coloff.size() - 1;
}

extern "C" int elph_create(elph_handle *out, int kind, int64_t nsites, int64_t ltau, int64_t nbonds,
                           const int64_t *neighbor_table, const double *cosht, const double *sinht, int device) {
    if (!out) { elph_set_error("out is null"); return ELPH_E_ARG; }
    *out = nullptr;
    if (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) { elph_set_error("bad model kind %d", kind); return ELPH_E_ARG; }
    if (nsites < 1 || ltau < 1 || nbonds < 0) { elph_set_error("bad sizes N=%lld L=%lld nb=%lld", (long long)nsites, (long long)ltau, (long long)nbonds); return ELPH_E_ARG; }
    if (nsites > (int64_t)ELPH_MAX_SITES) {
        elph_set_error("nsites=%lld exceeds the %d sites a one-workgroup-per-slice kernel supports", (long long)nsites, ELPH_MAX_SITES);
        return ELPH_E_UNSUPPORTED;
    }
    if (nsites * ltau > (int64_t)1 << 30) { elph_set_error("ndim too large"); return ELPH_E_UNSUPPORTED; }
    // (beyond 1024 slices the tau-transforms run as dft_big.hip's two-step form, whose launches carry the slice index in gridDim.y)
    if (ltau > 65535) { elph_set_error("ltau=%lld: the time axis is limited to 65535 slices (launch geometry of the long-axis transform)", (long long)ltau); return ELPH_E_UNSUPPORTED; }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { elph_set_error("no HIP device visible"); return ELPH_E_NOGPU; }
    if (device < 0 || device >= ndev) { elph_set_error("device %d not in 0..%d", device, ndev - 1); return ELPH_E_ARG; }
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        elph_set_error("device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return ELPH_E_NOGPU;
    }

    elph_handle_s *h = new elph_handle_s();
    h->kind = kind; h->device = device;
    h->N = nsites; h->L = ltau; h->nb = nbonds; h->ndim = nsites * ltau;
    h->npl = (int)((nsites + ELPH_WAVE - 1) / ELPH_WAVE);
    h->maxiter = h->ndim;   // ConjugateGradient ctor default (IterativeSolvers.jl:49-51)

    colour_bonds(h, neighbor_table);

    int rc = ELPH_OK;
    auto fail = [&](int code) { elph_destroy(h); return code; };
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { elph_set_error("stream create failed"); return fail(ELPH_E_HIP); }
    h->own_stream = true;
    if ((rc = dev_alloc(&h->d_bi, (size_t)nbonds))) return fail(rc);
    if ((rc = dev_alloc(&h->d_bj, (size_t)nbonds))) return fail(rc);
    if ((rc = dev_alloc(&h->d_coloff, h->h_coloff.size()))) return fail(rc);
    const size_t ncs = (kind == ELPH_MODEL_SSH) ? (size_t)ltau * (size_t)nbonds : (size_t)nbonds;
    if ((rc = dev_alloc(&h->d_c, ncs))) return fail(rc);
    if ((rc = dev_alloc(&h->d_s, ncs))) return fail(rc);
    const size_t nE = (kind == ELPH_MODEL_SSH) ? (size_t)nsites : (size_t)h->ndim;
    if ((rc = dev_alloc(&h->d_E, nE))) return fail(rc);
    h->E_cap = (int64_t)nE;
    if ((rc = dev_alloc(&h->d_lam, 3 * (size_t)nsites))) return fail(rc);
    if (nbonds > 0) {
        if (hipMemcpy(h->d_bi, h->h_bi.data(), sizeof(int) * nbonds, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_bj, h->h_bj.data(), sizeof(int) * nbonds, hipMemcpyHostToDevice) != hipSuccess) {
            elph_set_error("table upload failed");
            return fail(ELPH_E_HIP);
        }
    }
    if (hipMemcpy(h->d_coloff, h->h_coloff.data(), sizeof(int) * h->h_coloff.size(), hipMemcpyHostToDevice) != hipSuccess) {
        elph_set_error("table upload failed");
        return fail(ELPH_E_HIP);
    }
    if (kind == ELPH_MODEL_HOLSTEIN && nbonds > 0) {
        h->h_c.assign(cosht, cosht + nbonds);
        h->h_s.assign(sinht, sinht + nbonds);
        if (hipMemcpy(h->d_c, cosht, sizeof(double) * nbonds, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_s, sinht, sizeof(double) * nbonds, hipMemcpyHostToDevice) != hipSuccess) {
            elph_set_error("cosh/sinh upload failed");
            return fail(ELPH_E_HIP);
        }
    }
    if ((rc = elph_dft_build_tables(h))) return fail(rc);
    if ((rc = build_lane_program(h))) return fail(rc);
    if ((rc = upload_lp_cs(h))) return fail(rc);
    if ((rc = elph_work_reserve(h, 1))) return fail(rc);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { elph_set_error("sync failed"); return fail(ELPH_E_HIP); }
    *out = h;
    return ELPH_OK;
}

extern "C" int elph_destroy(elph_handle h) {
    if (!h) return ELPH_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    elph_i_slabs_free(h);                             // (the slab handles of a large lattice: each is destroyed through here again)
    elph_shard_free(h);
    elph_hmc_free(h);
    elph_greens_free(h);
    elph_msolve_free(h);
    elph_dft_free(h);
    elph_kpm_free(h);
    elph_work_release(h);
    void *ptrs[] = {h->d_bi, h->d_bj, h->d_coloff, h->d_c, h->d_s, h->d_E, h->d_lam, h->d_ssh_x, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_bar,
                    h->d_ssh_cb, h->d_ssh_slot, h->d_diag, h->d_lp_ij, h->d_lp_c, h->d_lp_s, h->d_sq_bond, h->d_pg_bond, h->res.d_res, h->d_mu_ch};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    for (int k = 1; k < ELPH_SPLIT_PARTS; ++k)
        if (h->split_stream[k]) (void)hipStreamDestroy(h->split_stream[k]);
    if (h->split_ev) (void)hipEventDestroy(h->split_ev);
    delete h;
    return ELPH_OK;
}

extern "C" int elph_set_stream(elph_handle h, void *hip_stream) {
    CHECK_H(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hip_stream) {
        if (h->own_stream) { HIPCHK(hipStreamDestroy(h->stream)); h->own_stream = false; }
        h->stream = (hipStream_t)hip_stream;
    } else if (!h->own_stream) {
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return ELPH_OK;
}

extern "C" int elph_synchronize(elph_handle h) {
    CHECK_H(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// update_model!
// ------------------------------------------------------------------------------------------

extern "C" int elph_update_model_holstein(elph_handle h, const double *x, const double *lambda, const double *lambda2,
                                          const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!x || !lambda || !lambda2 || !mu) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t N = (size_t)h->N;
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + 2 * N, mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, x, (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    set_nchains(h, 1);   // expansions were per chain
    RC(elph_launch_expV(h, h->work.stage_in, dtau));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    return ELPH_OK;
}

// several independent phonon configurations (chains) resident at once: right-hand side r of a batched solve
// uses chain r % nchains.  X: nchains * ndim (reference layout, chain-major).
extern "C" int elph_update_model_holstein_chains(elph_handle h, int nchains, const double *X, const double *lambda,
                                                 const double *lambda2, const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (nchains < 1 || !X || !lambda || !lambda2 || !mu) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const size_t N = (size_t)h->N, nd = (size_t)h->ndim;
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((int64_t)nchains * (int64_t)nd > h->E_cap) {
        RC(dev_alloc(&h->d_E, (size_t)nchains * nd));
        h->E_cap = (int64_t)nchains * (int64_t)nd;
    }
    h->nchains = nchains;
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + 2 * N, mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // all configurations in one transfer (the staging buffer holds cap_rhs vectors), one exp kernel per chain, one sync
    RC(elph_work_reserve(h, nchains));
    HIPCHK(hipMemcpyAsync(h->work.stage_in, X, (size_t)nchains * nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int c = 0; c < nchains; ++c) RC(elph_launch_expV(h, h->work.stage_in + (size_t)c * nd, dtau, c));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    h->kpm.ready = false;   // the preconditioner belongs to ONE configuration
    return ELPH_OK;
}

extern "C" int elph_set_expV(elph_handle h, const double *expnDtauV) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!expnDtauV) { elph_set_error("null argument"); return ELPH_E_ARG; }
    HIPCHK(hipMemcpyAsync(h->work.stage_in, expnDtauV, (size_t)h->ndim * sizeof(double), hipMemcpyHostToDevice, h->stream));
    set_nchains(h, 1);   // expansions were per chain
    RC(elph_launch_r2s(h, h->d_E, h->work.stage_in, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_E = true;
    return ELPH_OK;
}

extern "C" int elph_update_model_ssh(elph_handle h, const double *cosht, const double *sinht, const double *expDtauMu) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (!expDtauMu || (h->nb > 0 && (!cosht || !sinht))) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t L = (size_t)h->L, nb = (size_t)h->nb;
    // reference: (Ltau x Nbonds) column-major = [bond][tau]; device: tau-major [tau][bond]
    h->h_c.resize(L * nb); h->h_s.resize(L * nb);
    for (size_t n = 0; n < nb; ++n)
        for (size_t t = 0; t < L; ++t) {
            h->h_c[t * nb + n] = cosht[n * L + t];
            h->h_s[t * nb + n] = sinht[n * L + t];
        }
    if (nb > 0) {
        HIPCHK(hipMemcpy(h->d_c, h->h_c.data(), L * nb * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_s, h->h_s.data(), L * nb * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(h->d_E, expDtauMu, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice));
    RC(upload_lp_cs(h));
    h->mu_per_chain = false;
    set_nchains(h, 1);      // host tables describe ONE configuration
    h->cs_host_stale = false;
    h->have_E = true;
    return ELPH_OK;
}

// update_model!(ssh) computed ON THE DEVICE from the phonon fields (SSHModels.jl:510-562): no cosh/sinh on the host, no
// (Ltau x Nbonds) tables over PCIe.
//   x          double[nph * ltau]   ssh.x, field = (phonon-1) Ltau + tau
//   cb_index   int64[nph]           1-based checkerboard position of each phonon's bond = checkerboard_perm[phonon_to_bond[p]]
//   t_ph, alpha, alpha2  double[nph] bare hopping of that bond (ssh.t[bond]) and the couplings
//   t_bare_cb  double[nbonds]       bare hopping of EVERY bond in checkerboard order (bonds without a phonon keep it)
//   mu         double[nsites]
// A bond is driven by at most one field per tau (equivalent fields carry equal x, :548-558).
// per-phonon tables, bare hoppings, lane-program slot map and mu of an SSH handle -> device (d_ssh_*, d_lam)
int elph_i_ssh_upload_params(elph_handle_s *h, int64_t nph, const int64_t *cb_index, const double *t_ph, const double *alpha,
                             const double *alpha2, const double *t_bare_cb, const double *mu) {
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (nph < 0 || !mu || (h->nb > 0 && !t_bare_cb) || (nph > 0 && (!cb_index || !t_ph || !alpha || !alpha2))) {
        elph_set_error("null argument");
        return ELPH_E_ARG;
    }
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, np = (size_t)nph;
    std::vector<int> cb0(np);
    for (size_t p = 0; p < np; ++p) {
        if (cb_index[p] < 1 || cb_index[p] > (int64_t)nb) { elph_set_error("cb_index[%zu] = %lld outside 1..%zu", p, (long long)cb_index[p], nb); return ELPH_E_ARG; }
        cb0[p] = (int)(cb_index[p] - 1);
    }
    if (!h->d_ssh_slot) {     // once: lane-program slot of each checkerboard bond (the layout of elph_lp_pack)
        std::vector<int> slot(std::max<size_t>(nb, 1), -1);
        if (h->fast_capable) {
            const int PP = (h->npl + 1) / 2;
            for (int col = 0; col < h->ncol && col < h->lp_mc; ++col)
                for (int n = h->h_coloff[col]; n < h->h_coloff[col + 1]; ++n) {
                    const int k = n - h->h_coloff[col];
                    slot[(size_t)n] = (col * PP + k / ELPH_WAVE) * ELPH_WAVE + (k % ELPH_WAVE);
                }
            // idle lane-program slots: the identity bond (cosh, sinh) = (1, 0) on every slice
            const size_t per = (size_t)h->lp_ne * ELPH_WAVE;
            std::vector<double> one(L * per, 1.0), zero(L * per, 0.0);
            HIPCHK(hipMemcpy(h->d_lp_c, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(h->d_lp_s, zero.data(), zero.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        RC(dev_alloc(&h->d_ssh_slot, slot.size()));
        HIPCHK(hipMemcpy(h->d_ssh_slot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
        RC(dev_alloc(&h->d_ssh_tbare, std::max<size_t>(nb, 1)));
    }
    if ((int64_t)np > h->ssh_nph_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        RC(dev_alloc(&h->d_ssh_x, std::max<size_t>((size_t)h->ssh_chain_cap * np * L, 1)));
        RC(dev_alloc(&h->d_ssh_par, std::max<size_t>(3 * np, 1)));
        RC(dev_alloc(&h->d_ssh_cb, std::max<size_t>(np, 1)));
        h->ssh_nph_cap = (int64_t)np;
    }
    if (np > 0) {
        HIPCHK(hipMemcpyAsync(h->d_ssh_par, t_ph, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_par + np, alpha, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_par + 2 * np, alpha2, np * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ssh_cb, cb0.data(), np * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    if (nb > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_tbare, t_bare_cb, nb * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam, mu, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // cb0 / the caller's arrays may go away
    h->ssh_nph = (int)np;
    return ELPH_OK;
}

extern "C" int elph_update_model_ssh_fields(elph_handle h, const double *x, int64_t nph, const int64_t *cb_index, const double *t_ph,
                                            const double *alpha, const double *alpha2, const double *t_bare_cb, const double *mu,
                                            double dtau) {
    CHECK_H(h);
    if (nph > 0 && !x) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_i_ssh_upload_params(h, nph, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu));
    h->mu_per_chain = false;
    set_nchains(h, 1);
    const size_t np = (size_t)nph;
    if (np > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_x, x, np * (size_t)h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_ssh_update(h, h->d_ssh_x, (int)np, h->d_ssh_cb, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_slot, dtau));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ssh_dtau = dtau;
    h->cs_host_stale = true;
    h->have_E = true;
    return ELPH_OK;
}

// Several independent phonon configurations (chains) of one SSH deck in one handle: X[nchains][nph*ltau]; in a batched call
// right-hand side r then uses the hopping tables of chain r % nchains (exp(dtau mu) and the couplings are the deck's, shared).
extern "C" int elph_update_model_ssh_fields_chains(elph_handle h, int nchains, const double *X, int64_t nph, const int64_t *cb_index,
                                                   const double *t_ph, const double *alpha, const double *alpha2,
                                                   const double *t_bare_cb, const double *mu, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    if (nchains < 1 || (nph > 0 && !X)) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_i_reserve_chains(h, nchains));
    RC(elph_i_ssh_upload_params(h, nph, cb_index, t_ph, alpha, alpha2, t_bare_cb, mu));
    const size_t np = (size_t)nph;
    if (np > 0) HIPCHK(hipMemcpyAsync(h->d_ssh_x, X, (size_t)nchains * np * (size_t)h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_ssh_update(h, h->d_ssh_x, (int)np, h->d_ssh_cb, h->d_ssh_par, h->d_ssh_tbare, h->d_ssh_slot, dtau, 0, nchains));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ssh_dtau = dtau;
    h->cs_host_stale = true;
    h->have_E = true;
    h->kpm.ready = false;
    return ELPH_OK;
}

// model.cosht / model.sinht as the reference stores them, (Ltau x Nbonds) column-major = [bond][tau] — for callers that
// reach into those fields (KPMPreconditioners.jl:362-378) after a device-side update
extern "C" int elph_get_cosh_sinh(elph_handle h, double *cosht, double *sinht) {
    CHECK_H(h);
    if (!cosht || !sinht) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t L = (h->kind == ELPH_MODEL_SSH) ? (size_t)h->L : 1, nb = (size_t)h->nb;
    std::vector<double> c(L * nb), s(L * nb);
    if (nb > 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(c.data(), h->d_c, c.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(s.data(), h->d_s, s.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (size_t n = 0; n < nb; ++n)
        for (size_t t = 0; t < L; ++t) { cosht[n * L + t] = c[t * nb + n]; sinht[n * L + t] = s[t * nb + n]; }
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// mul! family
// ------------------------------------------------------------------------------------------

static int need_model(elph_handle_s *h) {
    if (!h->have_E) { elph_set_error("update_model has not been called on this handle"); return ELPH_E_STATE; }
    return ELPH_OK;
}

static int mul_dev(elph_handle_s *h, int which, double *y_dev, const double *v_dev) {
    RC(need_model(h));
    if (!y_dev || !v_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_launch_r2s(h, h->work.b, v_dev, 1));
    if (which == 3) {                                    // M Mᵀ v (Models.jl:229-238): two launches, not on the CG path
        RC(elph_launch_mul(h, 1, h->work.tmp, h->work.b, 1));
        RC(elph_launch_mul(h, 0, h->work.x, h->work.tmp, 1));
    } else {
        RC(elph_launch_mul(h, which, h->work.x, h->work.b, 1));
    }
    RC(elph_launch_s2r(h, y_dev, h->work.x, 1));
    return ELPH_OK;
}

static int mul_host(elph_handle_s *h, int which, double *y, const double *v) {
    if (!y || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t bytes = (size_t)h->ndim * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, v, bytes, hipMemcpyHostToDevice, h->stream));
    RC(mul_dev(h, which, h->work.stage_out, h->work.stage_in));
    HIPCHK(hipMemcpyAsync(y, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_mulM(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 0, y, v); }
extern "C" int elph_mulMT(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 1, y, v); }
extern "C" int elph_mulMTM(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 2, y, v); }
extern "C" int elph_mulMMT(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_host(h, 3, y, v); }
extern "C" int elph_mulM_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 0, y, v); }
extern "C" int elph_mulMT_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 1, y, v); }
extern "C" int elph_mulMTM_dev(elph_handle h, double *y, const double *v) { CHECK_H(h); return mul_dev(h, 2, y, v); }

// ------------------------------------------------------------------------------------------
// CG driver
// ------------------------------------------------------------------------------------------

extern "C" int elph_solver_set(elph_handle h, double tol, int64_t maxiter, double kappa_max) {
    CHECK_H(h);
    if (!(tol > 0.0) || maxiter < 0 || !(kappa_max > 0.0)) { elph_set_error("bad solver parameters"); return ELPH_E_ARG; }
    h->tol = tol;
    h->maxiter = (maxiter < 1) ? h->ndim : maxiter;   // IterativeSolvers.jl:49-51
    h->kmax = kappa_max;
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// A large KPM-preconditioned batch as TWO half-batches on two streams.  One iteration is four dependent kernels (k_cg_ap, forward
// transform + residual update, Chebyshev recursion, inverse transform + p/x-update), each ending in a drain of the whole chip before the
// next may start, the Chebyshev one latency-bound and the transforms quantised in rounds of waves (288 right-hand sides: 2.25 rounds).
// Two independent halves, each with its own chain of kernels, fill one another's tails and run the latency-bound kernel of one under
// the HBM-bound kernels of the other.  The second half is a VIEW of the handle: a copy whose per-right-hand-side device arrays start at
// right-hand side n/2 and whose stream is the second stream — every launcher reads buffers and stream from the handle it is given, so
// nothing else changes, and each right-hand side sees exactly the arithmetic of the single-stream form (same kernels, same partial-sum
// layout per right-hand side).  Needs the p/x-fused iteration (the unfused one ping-pongs p between two slots whose distance depends on
// the batch size) and halves that hold whole groups of chains.  ELPH_SPLIT_STREAMS=0 off, =1 wherever legal; default from 192 right-hand sides.
// ------------------------------------------------------------------------------------------
__global__ void k_spin_us(long long ticks, long long *sink) {      // wall_clock64: 100 MHz
    const long long t0 = wall_clock64();
    long long t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (sink) *sink = t;
}

// do kernels on `a` and `b` run at the same time?  (two 40-us spins: together ~40 us, one after the other ~80)
static int streams_overlap(hipStream_t a, hipStream_t b, bool *yes) {
    hipEvent_t e0 = nullptr, e1 = nullptr, eb = nullptr;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
    float best = 1e9f;
    hipError_t er = hipSuccess;
    for (int rep = 0; rep < 3 && er == hipSuccess; ++rep) {
        er = hipStreamSynchronize(a);
        if (er == hipSuccess) er = hipStreamSynchronize(b);
        if (er == hipSuccess) er = hipEventRecord(e0, a);
        if (er == hipSuccess) {
            hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(1), 0, a, 4000LL, (long long *)nullptr);
            hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(1), 0, b, 4000LL, (long long *)nullptr);
            er = hipEventRecord(eb, b);
        }
        if (er == hipSuccess) er = hipStreamWaitEvent(a, eb, 0);
        if (er == hipSuccess) er = hipEventRecord(e1, a);
        if (er == hipSuccess) er = hipEventSynchronize(e1);
        float ms = 0.f;
        if (er == hipSuccess) er = hipEventElapsedTime(&ms, e0, e1);
        if (er == hipSuccess && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(eb);
    if (er != hipSuccess) { elph_set_error("stream pairing probe: %s", hipGetErrorString(er)); return ELPH_E_HIP; }
    *yes = best < 0.062f;      // (40 us each: < 62 us = they overlapped)
    return ELPH_OK;
}

static int make_overlapping_stream(elph_handle_s *h, hipStream_t *out) {
    std::vector<hipStream_t> aside;
    hipStream_t chosen = nullptr;
    int rc = ELPH_OK;
    for (int attempt = 0; attempt < 8 && !chosen && rc == ELPH_OK; ++attempt) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { elph_set_error("hipStreamCreate failed"); rc = ELPH_E_HIP; break; }
        bool ok = true;
        rc = streams_overlap(h->stream, s, &ok);
        if (rc == ELPH_OK && (ok || attempt == 7)) chosen = s;      // (eight in a row on the main stream's queue: take it, the form still works)
        else aside.push_back(s);
    }
    for (hipStream_t s : aside) (void)hipStreamDestroy(s);
    if (rc) { if (chosen) (void)hipStreamDestroy(chosen); return rc; }
    *out = chosen;
    return ELPH_OK;
}

// The parts of a solve's chunk loop: `ways` parts of n1 right-hand sides each, part 0 the handle itself on its own stream — one part (the
// default: a one-stream solve) or ELPH_SPLIT_PARTS of a preconditioned batch on streams of their own (split_begin)
struct SplitRun {
    bool on = false, ok = false;
    int ways = 1, n1 = 0;
    elph_handle_s *main = nullptr, *view[ELPH_SPLIT_PARTS] = {};
    CgPlan before;                                        // the whole batch's plan (split_begin replaces it with the parts')
    SplitRun(elph_handle_s *h, int nrhs) : n1(nrhs), main(h) { view[0] = h; }
    // A solve that leaves through an error return must not leave kernels of the other streams in flight behind it (they write work.x, work.p, work.r,
    // work.state of their parts while the caller's next step — ldiv's zero-fill, a retry, a new solve — runs on the main stream), nor the handle
    // believing in a plan that never ran to its end.
    ~SplitRun() {
        for (int k = 1; k < ways; ++k)
            if (view[k]) {
                if (on) (void)hipStreamSynchronize(view[k]->stream);
                delete view[k];
            }
        if (ways > 1 && !ok) main->plan = before;      // (split_begin changed it; also when it failed before its streams ran)
    }
};

static bool split_legal(elph_handle_s *h, int nrhs, int use_prec, bool hist) {
    const int ways = ELPH_SPLIT_PARTS;
    if (!use_prec || hist || nrhs < 2 * ways || (nrhs % ways) || h->solo_chain >= 0 || h->dot_hi > 0) return false;
    const int n1 = nrhs / ways;
    if (n1 % std::max(1, h->nchains) || n1 % std::max(1, h->kpm.nch())) return false;
    return elph_plan_cg(h, n1, true, nrhs).px;      // (the parts choose their slices per wave for the whole batch in flight)
}

static bool split_wanted(elph_handle_s *h, int nrhs, int use_prec, bool hist) {
    const char *e = getenv("ELPH_SPLIT_STREAMS");
    if (e && e[0] == '0') return false;
    if (!split_legal(h, nrhs, use_prec, hist)) return false;
    // (config C, 128 right-hand sides: 130 us either way, profiles/r05/px_chunk_T.log; five sites per lane — the honeycomb lattice of config D,
    //  whose fused kernel stays at two waves per SIMD — gains from 64 on: D 128: 131 -> 116 us, 256: 262 -> 230, profiles/r05/px_fused_five_sites_per_lane.log;
    //  honeycomb 16 x 16 cells, eight sites per lane: 64 right-hand sides 64 -> 55 us, 256: 159 -> 145; D at 64: 89 -> 87)
    // (hopping disorder on 4 x 4 patches: the table variants of the patch kernels hold 40 KB of LDS per wavefront — two half-batches side by side lose to one
    //  stream: 32 x 32 at 96 right-hand sides 763 against 732 us, 28 x 28 695 against 663; profiles/r06/hopping_disorder_patch_kernels_with_tables.log)
    if (!(e && e[0] == '1') && h->shape.PX * h->shape.PY >= 16 && !h->kpm.hop_uniform && elph_pg_disorder_ok(h)) return false;
    return (e && e[0] == '1') || nrhs >= (h->npl >= 5 ? 64 : 192);
}

// after elph_launch_cg_init(h, nrhs, 1, …) on the main stream
static int split_begin(elph_handle_s *h, int nrhs, SplitRun &S) {
    S.ways = ELPH_SPLIT_PARTS;
    S.n1 = nrhs / S.ways;
    S.before = h->plan;
    // The parts must run on DIFFERENT hardware queues.  HIP maps its streams onto a few hardware queues per process (four by default,
    // GPU_MAX_HW_QUEUES) by a rule of its own: in a process that holds several handles a part's stream can share the queue of the handle's main
    // stream — the parts then run one after the other, slower than one stream (round 6: the second handle of a process, 32 x 32 at 72 right-hand
    // sides: 437 us instead of 353; a stream priority of its own did not change the mapping).  So the pairing is MEASURED once per stream: a spin
    // kernel on each of the two streams at the same time — two that overlap finish in the time of one; a candidate that does not is set aside
    // (kept alive until the choice is made, so that the next candidate does not inherit its queue) and the next one is tried.
    for (int k = 1; k < S.ways; ++k)
        if (!h->split_stream[k]) RC(make_overlapping_stream(h, &h->split_stream[k]));
    if (!h->split_ev) HIPCHK(hipEventCreateWithFlags(&h->split_ev, hipEventDisableTiming));
    h->plan = elph_plan_cg(h, S.n1, true, nrhs);          // (split_legal: the parts run p/x-fused whatever the whole batch would have run)
    HIPCHK(hipEventRecord(h->split_ev, h->stream));       // the start state (x0, r0, p0, rho0 of every right-hand side) is on the main stream
    for (int k = 1; k < S.ways; ++k) {
        elph_handle_s *v = S.view[k] = new elph_handle_s(*h);
        v->work = h->work.part((size_t)k * (size_t)S.n1);
        v->stream = h->split_stream[k];
        HIPCHK(hipStreamWaitEvent(v->stream, h->split_ev, 0));
    }
    S.on = true;
    return ELPH_OK;
}

// one iteration of every part, each on its stream
static int split_iteration(SplitRun &S, int use_prec) {
    for (int k = 0; k < S.ways; ++k) RC(elph_launch_cg_iteration(S.view[k], S.n1, use_prec));
    return ELPH_OK;
}

// the main stream continues only after the other parts have finished
static int split_join(SplitRun &S) {
    elph_handle_s *h = S.main;
    for (int k = 1; k < S.ways; ++k) {
        HIPCHK(hipEventRecord(h->split_ev, S.view[k]->stream));
        HIPCHK(hipStreamWaitEvent(h->stream, h->split_ev, 0));
    }
    return ELPH_OK;
}

// The CG states of every part come back to the host (each on its stream, then all drained): iters[r] = the iteration count of every
// right-hand side whose newer state copy is terminal; *all_done: every one is
static int read_states(const SplitRun &S, int64_t *iters, bool *all_done) {
    for (int k = 0; k < S.ways; ++k)
        HIPCHK(hipMemcpyAsync(S.view[k]->work.h_state, S.view[k]->work.state, sizeof(CgState) * 2 * (size_t)S.n1, hipMemcpyDeviceToHost, S.view[k]->stream));
    for (int k = 0; k < S.ways; ++k) HIPCHK(hipStreamSynchronize(S.view[k]->stream));
    *all_done = true;
    for (int r = 0; r < S.ways * S.n1; ++r) {
        const CgState &a = S.main->work.h_state[2 * r], &b = S.main->work.h_state[2 * r + 1];
        const CgState &s = (b.seq > a.seq) ? b : a;
        if (!s.done) *all_done = false;
        else iters[r] = s.iters;
    }
    return ELPH_OK;
}

// the eps histories of a finished solve (host, nrhs x (maxiter + 1); nullptr: none recorded)
static int read_hist(elph_handle_s *h, int nrhs, int64_t maxiter, double *eps_hist) {
    if (!eps_hist) return ELPH_OK;
    HIPCHK(hipMemcpyAsync(eps_hist, h->work.hist, sizeof(double) * (size_t)nrhs * (size_t)(maxiter + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// Which resident form would this solve take, ignoring the cool-down (except that a handle that cools down does not BUILD its slabs just to
// be counted) — in the order they are tried: the whole un-preconditioned solve in
// one launch with the Krylov vectors in registers (cg_wg.hip: k_cg_wg); on a lattice beyond one wave's slice the same kernel on slabs of
// rows of the lattice, all on this device, one launch per right-hand side (slabs.hip; x0 = 0 only — the slab kernel starts from it:
// ldiv!'s zero-fill); the whole PRECONDITIONED solve in one launch for one to eight right-hand sides on the 16 x 16 square lattice
// (pcg_wg.hip: k_pcg_wg).  `after`: the forms up to that one have declined.  The shape only — elph_wg_cg's cost rule is its own.
enum ResidentForm { RES_NONE, RES_CG_WG, RES_SLABS, RES_PCG_WG };
static ResidentForm resident_form(elph_handle_s *h, int nrhs, int use_prec, bool x0_zero, int64_t maxiter, ResidentForm after = RES_NONE) {
    if (maxiter < 1) return RES_NONE;
    if (use_prec) return (after < RES_PCG_WG && elph_pcg_wg_usable(h, nrhs)) ? RES_PCG_WG : RES_NONE;
    if (after < RES_CG_WG && h->fast && elph_wg_usable(h, nullptr, nullptr, nullptr, nrhs)) return RES_CG_WG;
    // (cooling down: only slabs that exist already count — it has them, or the form is not its own)
    if (after < RES_SLABS && x0_zero && (h->slabs || !h->res.cooling()) && elph_i_slabs_usable(h, nrhs)) return RES_SLABS;
    return RES_NONE;
}

// One attempt of k_cg_wg / k_pcg_wg (use_prec) at the solve elph_launch_cg_init has set up.  The launcher parks the caller's initial guess
// in x0_save — scratch its kind of solve does not use — once it has decided to launch.  *solved: the states are terminal, iters filled.
// Otherwise the streaming iteration can start: nothing was launched (the form declined), or a team gave up (x, r of the right-hand sides
// that had finished were overwritten) and every right-hand side is back at the caller's initial guess, re-initialised.
static int resident_attempt(elph_handle_s *h, const SplitRun &S, int nrhs, int use_prec, const CgParams &P, bool x0_zero, double *x0_save,
                            int64_t *iters, bool *solved) {
    *solved = false;
    bool ran = false, all_done = false, aborted = false;
    CgBufs B = elph_make_bufs(h, nrhs);
    B.params = P;
    RC(use_prec ? elph_pcg_wg(h, B, nrhs, 0, x0_save, &ran) : elph_wg_cg(h, B, nrhs, 0, x0_zero, x0_save, &ran));
    if (!ran) return ELPH_OK;
    RC(read_states(S, iters, &all_done));
    RC(elph_wg_aborted(h, &aborted));
    if (!aborted) {
        if (!all_done) {
            elph_set_error(use_prec ? "resident preconditioned CG ended without a terminal state (internal error)"
                                    : "workgroup-resident CG ended without a terminal state (internal error)");
            return ELPH_E_STATE;
        }
        *solved = true;
        return ELPH_OK;
    }
    elph_wg_timed_out(h);
    HIPCHK(hipMemcpyAsync(h->work.x, x0_save, (size_t)nrhs * (size_t)h->ndim * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return elph_launch_cg_init(h, nrhs, use_prec);
}

// Runs CG on work.b / work.x (layout S) for nrhs right-hand sides.  Returns per-rhs iteration counts.
static int run_cg(elph_handle_s *h, int nrhs, int use_prec, double tol, int64_t maxiter, double kmax, int64_t *iters,
                  double *eps_hist /* host, optional, nrhs*(maxiter+1) */) {
    const bool x0_zero = h->x_zero;        // the hint belongs to THIS solve: consumed before anything can return
    h->x_zero = false;
    if (use_prec && !h->kpm.ready) { elph_set_error("preconditioned solve requested before elph_kpm_setup"); return ELPH_E_STATE; }
    CgParams P;
    P.tol = tol; P.kmax = kmax; P.maxiter = maxiter; P.use_prec = use_prec;
    P.record_hist = eps_hist ? 1 : 0;
    P.hist_stride = maxiter + 1;
    if (eps_hist) {
        const int64_t need = (int64_t)nrhs * (maxiter + 1);
        if (need > h->work.hist_cap) {
            HIPCHK(hipStreamSynchronize(h->stream));
            RC(dev_alloc(&h->work.hist, (size_t)need));
            h->work.hist_cap = need;
        }
    }
    h->cur_params = P;
    // one solve of the cool-down after a resident kernel timed out — counted only for solves that WOULD have taken a resident kernel (any
    // form, either kind of solve): a stream of large streaming batches in between does not bring the retry forward, and a solve that
    // never launches a resident kernel does not clear the abort word
    if (h->res.cooling() && resident_form(h, nrhs, use_prec, x0_zero, maxiter) != RES_NONE) RC(elph_wg_cooldown_step(h));
    RC(elph_launch_cg_init(h, nrhs, use_prec, x0_zero));      // (x0 = 0: A x0 = 0 without the mat-vec)
    SplitRun S(h, nrhs);

    // the resident forms, each where it applies; one that declines leaves the solve to the next, a time-out to the streaming iteration
    for (ResidentForm f = RES_NONE; !h->res.cooling() && (f = resident_form(h, nrhs, use_prec, x0_zero, maxiter, f)) != RES_NONE;) {
        bool solved = false;
        if (f == RES_SLABS) {
            RC(elph_i_slabs_solve(h, nrhs, P, 0, iters, &solved, nullptr));
            if (!solved) RC(elph_launch_cg_init(h, nrhs, use_prec, true));      // (x is zero again: elph_i_slabs_solve)
        } else {
            RC(resident_attempt(h, S, nrhs, use_prec, P, x0_zero, use_prec ? h->work.tmp : h->work.zp, iters, &solved));
        }
        if (solved) return read_hist(h, nrhs, maxiter, eps_hist);
    }

    // the streaming iteration, ELPH_CG_CHUNK iterations of every part between two reads of the states
    if (split_wanted(h, nrhs, use_prec, eps_hist != nullptr)) RC(split_begin(h, nrhs, S));
    const int64_t max_chunks = (maxiter + 1 + ELPH_CG_CHUNK - 1) / ELPH_CG_CHUNK + 1;
    bool all_done = false;
    for (int64_t c = 0; c < max_chunks && !all_done; ++c) {
        for (int it = 0; it < ELPH_CG_CHUNK; ++it) RC(split_iteration(S, use_prec));
        RC(read_states(S, iters, &all_done));
    }
    h->ap_count = S.view[S.ways - 1]->ap_count;
    S.ok = all_done;
    if (!all_done) {
        elph_set_error(S.ways > 1 ? "CG chunk loop (two streams) ended without a terminal state (internal error)" : "CG chunk loop ended without a terminal state (internal error)");
        return ELPH_E_STATE;
    }
    return read_hist(h, nrhs, maxiter, eps_hist);
}

// residual + flag logic of ldiv! for rhs already solved into work.x; zeroes x where flag > 0
static int residual_and_flags(elph_handle_s *h, int nrhs, const int64_t *iters, int64_t cmp_maxiter, double *resid, int *flag) {
    RC(elph_launch_residual(h, nrhs));
    HIPCHK(hipMemcpyAsync(h->work.h_scal, h->work.scal, sizeof(double) * (size_t)nrhs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int r = 0; r < nrhs; ++r) {
        resid[r] = h->work.h_scal[r];
        if (resid[r] > sqrt(h->tol)) {           // Models.jl:100,157 (NaN compares false, as in the reference)
            flag[r] = (iters[r] == cmp_maxiter) ? 1 : 2;
            RC(elph_launch_zero(h, h->work.x + (size_t)r * (size_t)h->ndim, h->ndim));   // fill!(x,0)
        } else {
            flag[r] = 0;
        }
    }
    return ELPH_OK;
}

// ldiv! on device-resident layout-S work.b/work.x
static int ldiv_core(elph_handle_s *h, int nrhs, int use_prec, int64_t maxiter, int64_t *iters, double *resid, int *flag) {
    RC(need_model(h));
    if (maxiter == 0) maxiter = h->maxiter;                                  // Models.jl:78-80,143-145
    if (!use_prec) {
        RC(run_cg(h, nrhs, 0, h->tol, maxiter, h->kmax, iters, nullptr));
        RC(residual_and_flags(h, nrhs, iters, h->maxiter, resid, flag));     // Models.jl:160 compares solver.maxiter
        return ELPH_OK;
    }
    RC(run_cg(h, nrhs, 1, h->tol, maxiter, h->kmax, iters, nullptr));
    RC(residual_and_flags(h, nrhs, iters, maxiter, resid, flag));            // Models.jl:103 compares maxiter
    // failed right-hand sides: retry without preconditioner, 10x maxiter, from x = 0 (Models.jl:129-133)
    for (int r = 0; r < nrhs; ++r) {
        if (flag[r] == 0) continue;
        int64_t it1 = 0; double rs1 = 0; int fl1 = 0;
        RC(elph_retry_in_slot0(h, r, [&]() -> int {
            RC(run_cg(h, 1, 0, h->tol, 10 * maxiter, h->kmax, &it1, nullptr));
            return residual_and_flags(h, 1, &it1, h->maxiter, &rs1, &fl1);
        }));
        iters[r] = it1; resid[r] = rs1; flag[r] = fl1;
    }
    return ELPH_OK;
}

int elph_i_ldiv_core(elph_handle_s *h, int nrhs, int use_prec, int64_t maxiter, int64_t *iters, double *resid, int *flag) {
    return ldiv_core(h, nrhs, use_prec, maxiter, iters, resid, flag);
}

// Room for nrhs vectors and for the bond brackets q[chain][tau][bond] of nch chains (SSH force).  The brackets go to work.p (two vectors per
// right-hand side) and their scatter onto the phonon fields to work.tmp (one), so a lattice with more than two bonds per site (triangular,
// cubic) needs more than the two right-hand sides of the solves: ceil(nb/N) vectors per chain hold both.
int elph_i_ssh_bracket_capacity(elph_handle_s *h, int nrhs, int nch) {
    const int per_site = (int)((h->nb + h->N - 1) / h->N);
    return elph_work_reserve(h, std::max(nrhs, nch * per_site));
}
// SSH: one set of hopping tables (tau-major cosh/sinh + their lane-program copies) and one field buffer per chain
static int ssh_reserve_chains(elph_handle_s *h, int nchains) {
    if (nchains <= h->ssh_chain_cap) return ELPH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, per = (size_t)h->lp_ne * ELPH_WAVE, nc = (size_t)nchains;
    RC(dev_alloc(&h->d_c, nc * L * nb));
    RC(dev_alloc(&h->d_s, nc * L * nb));
    if (h->fast_capable) {
        RC(dev_alloc(&h->d_lp_c, nc * L * per));
        RC(dev_alloc(&h->d_lp_s, nc * L * per));
        // idle lane-program slots: the identity bond (cosh, sinh) = (1, 0) on every slice of every chain
        std::vector<double> one(nc * L * per, 1.0);
        HIPCHK(hipMemcpy(h->d_lp_c, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(h->d_lp_s, 0, one.size() * sizeof(double)));
    }
    if (h->ssh_nph_cap > 0) RC(dev_alloc(&h->d_ssh_x, nc * (size_t)h->ssh_nph_cap * L));
    RC(dev_alloc(&h->d_E, nc * (size_t)h->N));          // exp(dtau mu) per chain
    h->E_cap = (int64_t)(nc * (size_t)h->N);
    h->ssh_chain_cap = nchains;
    h->have_E = false;          // the tables are empty until the next update_model!
    h->cs_host_stale = true;
    return ELPH_OK;
}

int elph_i_reserve_chains(elph_handle_s *h, int nchains) {
    if (nchains < 1) { elph_set_error("nchains < 1"); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->kind == ELPH_MODEL_SSH) {
        RC(ssh_reserve_chains(h, nchains));
        set_nchains(h, nchains);
        return ELPH_OK;
    }
    const int64_t need = (int64_t)nchains * h->ndim;
    if (need > h->E_cap) {
        RC(dev_alloc(&h->d_E, (size_t)need));
        h->E_cap = need;
        h->have_E = false;
    }
    set_nchains(h, nchains);
    return ELPH_OK;
}

static int stage_in_dev(elph_handle_s *h, int nrhs, const double *X_dev, const double *B_dev) {
    RC(elph_work_reserve(h, nrhs));
    RC(elph_launch_r2s(h, h->work.b, B_dev, nrhs));
    RC(elph_launch_r2s(h, h->work.x, X_dev, nrhs));
    h->x_zero = false;                              // (a caller's initial guess)
    return ELPH_OK;
}

// Is the caller's initial guess all zeros?  Looked at only where it decides something: a lattice beyond one wave's slice whose
// un-preconditioned solve of one or two right-hand sides the slab form (slabs.hip; it starts from x = 0) could take.  Stops at the first
// non-zero; a zero guess costs one pass over the vector on the host (1.3 MB at 32 x 32 sites, 160 slices) — against a solve of milliseconds.
static bool x0_is_zero(elph_handle_s *h, int nrhs, int use_prec, const double *X) {
    if (use_prec || h->have_E == false) return false;
    if (!elph_i_slabs_usable(h, nrhs)) return false;      // (also while cooling down: the hint still lets run_cg count the solve)
    const size_t n = (size_t)nrhs * (size_t)h->ndim;
    for (size_t i = 0; i < n; ++i) if (X[i] != 0.0) return false;
    return true;
}

extern "C" int elph_ldiv_batched_dev(elph_handle h, int nrhs, double *X_dev, const double *B_dev, int use_prec,
                                     int64_t maxiter, int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    if (nrhs < 1 || !X_dev || !B_dev || !iters || !residual_error || !flag || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(stage_in_dev(h, nrhs, X_dev, B_dev));
    RC(ldiv_core(h, nrhs, use_prec, maxiter, iters, residual_error, flag));
    RC(elph_launch_s2r(h, X_dev, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_ldiv_dev(elph_handle h, double *x_dev, const double *b_dev, int use_prec, int64_t maxiter,
                             int64_t *iters, double *residual_error, int *flag) {
    return elph_ldiv_batched_dev(h, 1, x_dev, b_dev, use_prec, maxiter, iters, residual_error, flag);
}

extern "C" int elph_ldiv_batched(elph_handle h, int nrhs, double *X, const double *B, int use_prec, int64_t maxiter,
                                 int64_t *iters, double *residual_error, int *flag) {
    CHECK_H(h);
    if (nrhs < 1 || !X || !B || !iters || !residual_error || !flag || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_work_reserve(h, nrhs));
    const size_t bytes = (size_t)nrhs * (size_t)h->ndim * sizeof(double);
    RC(elph_stage_in(h, h->work.b, B, nrhs));
    if (x0_is_zero(h, nrhs, use_prec, X)) {          // fill!(x, 0) of the callers (HMC.jl:854, GreensFunctions.jl:334): seen on the host, the slab form may take the solve
        HIPCHK(hipMemsetAsync(h->work.x, 0, bytes, h->stream));
        h->x_zero = true;
    } else {
        RC(elph_stage_in(h, h->work.x, X, nrhs));
        h->x_zero = false;                          // (a caller's initial guess)
    }
    RC(ldiv_core(h, nrhs, use_prec, maxiter, iters, residual_error, flag));
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_ldiv(elph_handle h, double *x, const double *b, int use_prec, int64_t maxiter, int64_t *iters,
                         double *residual_error, int *flag) {
    return elph_ldiv_batched(h, 1, x, b, use_prec, maxiter, iters, residual_error, flag);
}

extern "C" int elph_cg_solve(elph_handle h, double *x, const double *b, double tol, int64_t maxiter, double kappa_max,
                             int use_precond, int64_t *iters, double *eps_hist) {
    CHECK_H(h);
    RC(need_model(h));
    if (!x || !b || !iters || maxiter < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (maxiter == 0) maxiter = h->maxiter;       // iszero() defaults, IterativeSolvers.jl:160-173
    if (tol == 0.0) tol = h->tol;
    if (kappa_max == 0.0) kappa_max = h->kmax;
    const size_t bytes = (size_t)h->ndim * sizeof(double);
    RC(elph_stage_in(h, h->work.b, b, 1));
    if (x0_is_zero(h, 1, use_precond, x)) {
        HIPCHK(hipMemsetAsync(h->work.x, 0, bytes, h->stream));
        h->x_zero = true;
    } else {
        RC(elph_stage_in(h, h->work.x, x, 1));
        h->x_zero = false;                          // (a caller's initial guess)
    }
    RC(run_cg(h, 1, use_precond ? 1 : 0, tol, maxiter, kappa_max, iters, eps_hist));
    RC(elph_stage_out(h, x, h->work.x, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// (internal: shard.hip) Sites [site_lo, site_hi) (0-based) enter the inner products of the streaming CG (p.z, r.r, b.b); the other
// sites of the handle's lattice are ghost sites of a spatial shard: they take part in the mat-vec, their values come from the
// neighbouring ranks.  A restricted range runs the generic kernel family.  (0, nsites) restores the default.
int elph_i_set_dot_range(elph_handle_s *h, int64_t site_lo, int64_t site_hi) {
    if (site_lo < 0 || site_hi > h->N || site_lo >= site_hi) { elph_set_error("bad site range [%lld, %lld)", (long long)site_lo, (long long)site_hi); return ELPH_E_ARG; }
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool all = (site_lo == 0 && site_hi == h->N);
    h->dot_lo = all ? 0 : (int)site_lo;
    h->dot_hi = all ? 0 : (int)site_hi;
    h->fast = all ? h->fast_capable : false;
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// fermion force: update_model! + calc_O⁻¹Λϕ! + calc_dSfdx! with x, phi± , X± resident
// ------------------------------------------------------------------------------------------

int elph_i_force_holstein(elph_handle_s *h, const double *x, const double *lambda, const double *lambda2, const double *mu, double dtau,
                          const double *phi_plus, const double *phi_minus, double *dSfdx, double *Xp_out, double *Xm_out, int64_t *iters,
                          int *flag, int own_lo, int own_hi, const ElphPairSolve &solve_pair) {
    RC(elph_work_reserve(h, 2));
    const SolveWork &W = h->work;
    const size_t nd = (size_t)h->ndim, N = (size_t)h->N, L = (size_t)h->L;
    // update_model! (HolsteinModels.jl:526-549) and x in layout S
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + 2 * N, mu, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(W.stage_in, x, nd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_expV(h, W.stage_in, dtau));
    RC(elph_launch_r2s(h, W.xfield, W.stage_in, 1));
    h->have_E = true;
    // phi± -> layout S; b± = Λ phi± (HMC.jl:840-842)
    RC(elph_stage_in(h, W.phi, phi_plus, 1));
    RC(elph_stage_in(h, W.phi + nd, phi_minus, 1));
    RC(elph_launch_lambda_rhs(h, W.b, W.phi, W.xfield, dtau));
    RC(solve_pair(iters, flag));
    // dSf/dx (HMC.jl:790-814)
    RC(elph_launch_force_holstein(h, W.tmp, W.x, W.phi, W.xfield, dtau));
    std::vector<double> F(nd);
    RC(elph_stage_out(h, F.data(), W.tmp, 1));
    if (Xp_out) RC(elph_stage_out(h, Xp_out, W.x, 1));
    if (Xm_out) RC(elph_stage_out(h, Xm_out, W.x + nd, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = (size_t)own_lo * L; i < (size_t)own_hi * L; ++i) dSfdx[i] += F[i];      // "@. dSfdx += ..." accumulates (:803-811)
    return ELPH_OK;
}

// the two solves of calc_O⁻¹Λϕ! as one batch from x = 0 (fill!(O⁻¹Λϕ, 0), HMC.jl:854,883) at tol^power
static ElphPairSolve batch_pair(elph_handle_s *h, int use_precond, double tol_power) {
    return [=](int64_t *iters, int *flag) -> int {
        const size_t nd = (size_t)h->ndim;
        if (h->solver_kind != ELPH_SOLVER_CG) {      // the mul_by_M branch (HMC.jl:859-873, :888-902): Mᵀ y = Λϕ±, then M x = y, y in work.z
            int64_t it4[4] = {0, 0, 0, 0};
            int fl4[4] = {0, 0, 0, 0}, zero_minus = 0;
            {
                TolPower scope(h, tol_power);
                RC(elph_i_msolve_pair(h, 2, use_precond ? 1 : 0, h->work.x, h->work.z, h->work.b, it4, fl4));
            }
            elph_fold_pair_stages(1, it4, fl4, iters, flag, &zero_minus);
            if (zero_minus) RC(elph_launch_zero(h, h->work.x + nd, (int64_t)nd));
            return ELPH_OK;
        }
        HIPCHK(hipMemsetAsync(h->work.x, 0, 2 * nd * sizeof(double), h->stream));
        h->x_zero = true;
        int64_t it2[2] = {0, 0};
        double res2[2];
        int fl2[2] = {0, 0};
        {
            TolPower scope(h, tol_power);
            RC(ldiv_core(h, 2, use_precond, 0, it2, res2, fl2));
        }
        elph_fold_pair(1, it2, fl2, iters, flag);
        if (fl2[0]) RC(elph_launch_zero(h, h->work.x + nd, (int64_t)nd));
        return ELPH_OK;
    };
}

extern "C" int elph_fermion_force_holstein(elph_handle h, const double *x, const double *lambda, const double *lambda2,
                                           const double *mu, double dtau, const double *phi_plus, const double *phi_minus,
                                           int use_precond, double tol_power, double *dSfdx, double *Xp_out, double *Xm_out,
                                           int64_t *iters, int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    if (!x || !lambda || !lambda2 || !mu || !phi_plus || !phi_minus || !dSfdx || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    set_nchains(h, 1);   // expansions were per chain
    return elph_i_force_holstein(h, x, lambda, lambda2, mu, dtau, phi_plus, phi_minus, dSfdx, Xp_out, Xm_out, iters, flag, 0, (int)h->N,
                                 batch_pair(h, use_precond, tol_power));
}

// the two solves of calc_O⁻¹Λϕ! for an SSH handle (Λ = identity) + the bond brackets q[tau][n] left in h->work.p
static int ssh_force_core(elph_handle_s *h, const double *rhs_plus, const double *rhs_minus, int64_t *iters, int *flag,
                          const ElphPairSolve &solve_pair) {
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));
    RC(elph_stage_in(h, h->work.b, rhs_plus, 1));
    RC(elph_stage_in(h, h->work.b + h->ndim, rhs_minus, 1));
    RC(solve_pair(iters, flag));
    return elph_launch_force_ssh(h, h->work.p, h->work.x);     // work.p: scratch, free once the solves are done
}

static int ssh_solutions_out(elph_handle_s *h, double *Xp_out, double *Xm_out) {
    if (Xp_out) RC(elph_stage_out(h, Xp_out, h->work.x, 1));
    if (Xm_out) RC(elph_stage_out(h, Xm_out, h->work.x + h->ndim, 1));
    return ELPH_OK;
}

int elph_i_force_ssh(elph_handle_s *h, const double *rhs_plus, const double *rhs_minus, double *q_out, double *Xp_out, double *Xm_out,
                     int64_t *iters, int *flag, const ElphPairSolve &solve_pair) {
    RC(ssh_force_core(h, rhs_plus, rhs_minus, iters, flag, solve_pair));
    // q[tau][n] on the device (tau-major) -> q_out[n*L + tau] (tau fastest, like the reference's (Ltau x Nbonds) arrays)
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, nq = L * nb;
    std::vector<double> qt(nq);
    if (nq) HIPCHK(hipMemcpyAsync(qt.data(), h->work.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RC(ssh_solutions_out(h, Xp_out, Xm_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t t = 0; t < L; ++t)
        for (size_t n = 0; n < nb; ++n) q_out[n * L + t] = qt[t * nb + n];
    return ELPH_OK;
}

extern "C" int elph_fermion_force_ssh(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                      double tol_power, double *q_out, double *Xp_out, double *Xm_out, int64_t *iters,
                                      int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!rhs_plus || !rhs_minus || !q_out || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    return elph_i_force_ssh(h, rhs_plus, rhs_minus, q_out, Xp_out, Xm_out, iters, flag, batch_pair(h, use_precond, tol_power));
}

// The same with the scatter onto the phonon fields done on the device (SSHModels.jl:797-823 with one field per bond):
//   dSdx[(p-1) Ltau + tau] -= sg(tau) dtau (alpha_p + 2 alpha2_p x) q[tau][bond(p)],   sg(1) = -1   (HMC.jl:803,808)
// for the fields, couplings and checkerboard positions given to the last elph_update_model_ssh_fields call.
extern "C" int elph_fermion_force_ssh_fields(elph_handle h, const double *rhs_plus, const double *rhs_minus, int use_precond,
                                             double tol_power, double *dSdx, double *Xp_out, double *Xm_out, int64_t *iters,
                                             int *flag) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!rhs_plus || !rhs_minus || !dSdx || !iters || !flag) { elph_set_error("null argument"); return ELPH_E_ARG; }
    if (!h->cs_host_stale || h->ssh_nph < 0) { elph_set_error("elph_update_model_ssh_fields has not been called for the current field"); return ELPH_E_STATE; }
    RC(ssh_force_core(h, rhs_plus, rhs_minus, iters, flag, batch_pair(h, use_precond, tol_power)));
    const size_t nf = (size_t)h->ssh_nph * (size_t)h->L;
    double *dF = h->work.tmp;                                   // cap*ndim doubles
    if (nf > (size_t)h->work.cap_rhs * (size_t)h->ndim) { elph_set_error("more phonon fields than scratch"); return ELPH_E_UNSUPPORTED; }
    RC(elph_launch_ssh_scatter(h, dF, h->work.p, h->d_ssh_x, h->d_ssh_par, h->d_ssh_cb, h->ssh_nph, h->ssh_dtau));
    std::vector<double> F(nf);
    if (nf) HIPCHK(hipMemcpyAsync(F.data(), dF, nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RC(ssh_solutions_out(h, Xp_out, Xm_out));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < nf; ++i) dSdx[i] -= F[i];         // the reference accumulates into hmc.dSdx (HMC.jl:808)
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// muldMdx!(dMdx, u, model, v): ⟨∂M/∂x⟩ = uᵀ(∂M/∂x)v per field, for caller-given u and v — the operator calc_dSfdx! (HMC.jl:799,804)
// and LangevinDynamics.calc_dSfdx! (:378) call; HolsteinModels.jl:691-755, SSHModels.jl:707-829
// ------------------------------------------------------------------------------------------

// u, v, x, dMdx: device pointers, reference layout; lambda, lambda2: host double[nsites]
extern "C" int elph_muldMdx_holstein_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev, const double *x_dev,
                                         const double *lambda, const double *lambda2, double dtau) {
    CHECK_H(h);
    if (h->kind != ELPH_MODEL_HOLSTEIN) { elph_set_error("not a Holstein handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!dMdx_dev || !u_dev || !v_dev || !x_dev || !lambda || !lambda2) { elph_set_error("null argument"); return ELPH_E_ARG; }
    if (h->nchains != 1) { elph_set_error("muldMdx! acts on one phonon configuration; the handle holds %d chains", h->nchains); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, 2));
    const size_t nd = (size_t)h->ndim, N = (size_t)h->N;
    HIPCHK(hipMemcpyAsync(h->d_lam, lambda, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_lam + N, lambda2, N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, h->work.xfield, x_dev, 1));
    RC(elph_launch_r2s(h, h->work.b, u_dev, 1));
    RC(elph_launch_r2s(h, h->work.b + nd, v_dev, 1));
    RC(elph_launch_dmdx_holstein(h, h->work.tmp, h->work.b, h->work.b + nd, h->work.xfield, dtau, 1.0));
    RC(elph_launch_s2r(h, dMdx_dev, h->work.tmp, 1));
    HIPCHK(hipStreamSynchronize(h->stream));           // lambda / lambda2 are the caller's host arrays
    return ELPH_OK;
}

extern "C" int elph_muldMdx_holstein(elph_handle h, double *dMdx, const double *u, const double *v, const double *x,
                                     const double *lambda, const double *lambda2, double dtau) {
    CHECK_H(h);
    if (!dMdx || !u || !v || !x) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_work_reserve(h, 3));                         // stage_in: u, v, x
    const size_t nd = (size_t)h->ndim, bytes = nd * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, u, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + nd, v, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + 2 * nd, x, bytes, hipMemcpyHostToDevice, h->stream));
    RC(elph_muldMdx_holstein_dev(h, h->work.stage_out, h->work.stage_in, h->work.stage_in + nd, h->work.stage_in + 2 * nd, lambda, lambda2, dtau));
    HIPCHK(hipMemcpyAsync(dMdx, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// the bond brackets q[tau][n] of muldMdx!(·, u, ssh, v) left in h->work.p (u, v: device, reference layout)
static int ssh_dmdx_core(elph_handle_s *h, const double *u_dev, const double *v_dev) {
    if (h->kind != ELPH_MODEL_SSH) { elph_set_error("not an SSH handle"); return ELPH_E_ARG; }
    RC(need_model(h));
    if (!u_dev || !v_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    if (h->nchains != 1) { elph_set_error("muldMdx! acts on one phonon configuration; the handle holds %d chains", h->nchains); return ELPH_E_STATE; }
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));          // no-op when u_dev, v_dev are the handle's own staging (ssh_dmdx_stage)
    const size_t nd = (size_t)h->ndim;
    RC(elph_launch_r2s(h, h->work.b, u_dev, 1));
    RC(elph_launch_r2s(h, h->work.b + nd, v_dev, 1));
    return elph_launch_force_ssh(h, h->work.p, h->work.b + nd, h->work.b, 1);      // b0 = e^{Δτμ} v(τ−1), c0 = CBᵀ u
}

static int ssh_dmdx_stage(elph_handle_s *h, const double *u, const double *v) {
    if (!u || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_i_ssh_bracket_capacity(h, 2, 1));
    const size_t nd = (size_t)h->ndim, bytes = nd * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, u, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->work.stage_in + nd, v, bytes, hipMemcpyHostToDevice, h->stream));
    return ssh_dmdx_core(h, h->work.stage_in, h->work.stage_in + nd);
}

extern "C" int elph_muldMdx_ssh(elph_handle h, double *q_out, const double *u, const double *v) {
    CHECK_H(h);
    if (!q_out) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_stage(h, u, v));
    const size_t L = (size_t)h->L, nb = (size_t)h->nb, nq = L * nb;
    std::vector<double> qt(nq);
    if (nq) HIPCHK(hipMemcpyAsync(qt.data(), h->work.p, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t t = 0; t < L; ++t)
        for (size_t n = 0; n < nb; ++n) q_out[n * L + t] = qt[t * nb + n];
    return ELPH_OK;
}

static int ssh_dmdx_fields(elph_handle_s *h, double **dF, size_t *nf) {
    if (!h->cs_host_stale || h->ssh_nph < 0) { elph_set_error("elph_update_model_ssh_fields has not been called for the current field"); return ELPH_E_STATE; }
    *nf = (size_t)h->ssh_nph * (size_t)h->L;
    *dF = h->work.tmp;
    if (*nf > (size_t)h->work.cap_rhs * (size_t)h->ndim) { elph_set_error("more phonon fields than scratch"); return ELPH_E_UNSUPPORTED; }
    return elph_launch_ssh_scatter(h, *dF, h->work.p, h->d_ssh_x, h->d_ssh_par, h->d_ssh_cb, h->ssh_nph, h->ssh_dtau);
}

extern "C" int elph_muldMdx_ssh_fields(elph_handle h, double *dMdx, const double *u, const double *v) {
    CHECK_H(h);
    if (!dMdx) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_stage(h, u, v));
    double *dF = nullptr; size_t nf = 0;
    RC(ssh_dmdx_fields(h, &dF, &nf));
    if (nf) HIPCHK(hipMemcpyAsync(dMdx, dF, nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_muldMdx_ssh_fields_dev(elph_handle h, double *dMdx_dev, const double *u_dev, const double *v_dev) {
    CHECK_H(h);
    if (!dMdx_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(ssh_dmdx_core(h, u_dev, v_dev));
    double *dF = nullptr; size_t nf = 0;
    RC(ssh_dmdx_fields(h, &dF, &nf));
    if (nf) HIPCHK(hipMemcpyAsync(dMdx_dev, dF, nf * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// KPM preconditioner
// ------------------------------------------------------------------------------------------

void elph_kpm_free(elph_handle_s *h) {
    KpmState &K = h->kpm;
    void *ptrs[] = {K.d_Ebar, K.d_cbar, K.d_sbar, K.d_lp_cbar, K.d_lp_sbar, K.d_sq_cbar, K.d_sq_sbar, K.d_order, K.d_coff, K.d_wsched,
                    K.d_desc, K.d_fold, K.d_lam, K.d_coeff, K.d_start};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    K = KpmState();
}

extern "C" int elph_kpm_create(elph_handle h, int n, double buf, double c1, double c2) {
    CHECK_H(h);
    if (n < 1 || !(buf >= 0.0)) { elph_set_error("bad KPM parameters"); return ELPH_E_ARG; }
    // KPMExpansion ctor, KPMPreconditioners.jl:101-146: λ_lo = 0, λ_hi = 2, order 1 everywhere (one per chain, made on demand)
    elph_kpm_free(h);
    h->kpm.par = {n, buf, c1, c2};
    h->kpm.ssh = h->kind == ELPH_MODEL_SSH; h->kpm.created = true;
    return ELPH_OK;
}

// (re)size the per-chain host state and the device buffers for nch chains
static int kpm_reserve(elph_handle_s *h, int nch) {
    KpmState &K = h->kpm;
    const int Lo2 = (int)((h->L + 1) / 2);
    // a different number of configurations: every expansion starts from the constructor state again
    if (K.nch() != nch) K.chains.assign((size_t)nch, KpmChain(Lo2));
    K.h_Ebar.resize((size_t)nch * h->N);
    if (nch > K.tab_cap) {
        RC(dev_alloc(&K.d_Ebar, (size_t)nch * h->N));
        RC(dev_alloc(&K.d_order, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_coff, (size_t)nch * (Lo2 + 1)));
        RC(dev_alloc(&K.d_wsched, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_desc, (size_t)nch * Lo2));
        RC(dev_alloc(&K.d_fold, (size_t)nch * Lo2 * 2));
        RC(dev_alloc(&K.d_lam, (size_t)nch * 2));
        if (K.d_start) { HIPCHK(hipFree(K.d_start)); K.d_start = nullptr; }      // (made again for nch chains on its next use)
        K.tab_cap = nch;
    }
    const int hch = K.hop_per_chain() ? nch : 1;      // averaged hopping: one set per chain (SSH chains) or shared
    if (hch > K.hop_cap) {
        RC(dev_alloc(&K.d_cbar, (size_t)hch * h->nb));
        RC(dev_alloc(&K.d_sbar, (size_t)hch * h->nb));
        if (h->fast_capable) {
            RC(dev_alloc(&K.d_lp_cbar, (size_t)hch * h->lp_ne * ELPH_WAVE));
            RC(dev_alloc(&K.d_lp_sbar, (size_t)hch * h->lp_ne * ELPH_WAVE));
        }
        if (h->shape.sq_L() > 0) {
            RC(dev_alloc(&K.d_sq_cbar, (size_t)hch * 4 * h->N));
            RC(dev_alloc(&K.d_sq_sbar, (size_t)hch * 4 * h->N));
        }
        K.hop_cap = hch;
    }
    return ELPH_OK;
}

// Where update_A! takes its averaged inputs: the handle's own model, or the caller's — the full-lattice handle of a sharded HMC update holds
// no field of its own, so every rank contributes its own rows and the sum is injected (hmc.hip): Ē (Holstein) or c̄ / s̄ (bond phonons).
struct KpmSource { const double *Ebar = nullptr, *cbar = nullptr, *sbar = nullptr; };

// update_A! (KPMPreconditioners.jl:332-349 Holstein; :355-381 SSH) and the device images of the averaged hopping
static int kpm_update_A(elph_handle_s *h, const KpmSource &src) {
    KpmState &K = h->kpm;
    const int nch = K.nch();
    const size_t N = (size_t)h->N, nb = (size_t)h->nb;
    if (h->kind == ELPH_MODEL_HOLSTEIN) {
        // (Ē stays on the device: the Arnoldi kernel and the apply read it there)
        if (src.Ebar) HIPCHK(hipMemcpy(K.d_Ebar, src.Ebar, sizeof(double) * N, hipMemcpyHostToDevice));
        else RC(elph_launch_ebar(h, nch));
        K.h_cbar = h->h_c; K.h_sbar = h->h_s;
    } else {
        // Ebar = exp(dtau mu), held per chain (equal unless the chemical potential is tuned per chain)
        HIPCHK(hipMemcpyAsync(K.d_Ebar, h->d_E, sizeof(double) * nch * N, hipMemcpyDeviceToDevice, h->stream));
        if (src.cbar) { K.h_cbar.assign(src.cbar, src.cbar + nb); K.h_sbar.assign(src.sbar, src.sbar + nb); }
        K.h_cbar.resize(nch * nb); K.h_sbar.resize(nch * nb);
        if (nb > 0 && src.cbar) {
            HIPCHK(hipMemcpyAsync(K.d_cbar, K.h_cbar.data(), sizeof(double) * nch * nb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(K.d_sbar, K.h_sbar.data(), sizeof(double) * nch * nb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        } else if (nb > 0) {   // tau-means of cosht, sinht from the device tables (they may have been produced there)
            RC(elph_launch_cs_bar(h, K.d_cbar, K.d_sbar, nch));
            HIPCHK(hipMemcpyAsync(K.h_cbar.data(), K.d_cbar, sizeof(double) * nch * nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(K.h_sbar.data(), K.d_sbar, sizeof(double) * nch * nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
        }
    }
    // Holstein: c̄ = cosh(Δτ t), s̄ = sinh(Δτ t) never change after elph_create — upload their three device images once
    if (h->kind == ELPH_MODEL_HOLSTEIN && K.hop_uploaded) return ELPH_OK;
    const int hch = K.hop_per_chain() ? nch : 1;
    if (nb > 0 && h->kind == ELPH_MODEL_HOLSTEIN) {
        HIPCHK(hipMemcpy(K.d_cbar, K.h_cbar.data(), sizeof(double) * nb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_sbar, K.h_sbar.data(), sizeof(double) * nb, hipMemcpyHostToDevice));
    }
    if (h->fast_capable) {
        const size_t per = (size_t)h->lp_ne * ELPH_WAVE;
        std::vector<double> lc((size_t)hch * per), ls((size_t)hch * per);
        for (int c = 0; c < hch; ++c) {
            elph_lp_pack(h, K.h_cbar.data() + c * nb, lc.data() + c * per, 1.0);
            elph_lp_pack(h, K.h_sbar.data() + c * nb, ls.data() + c * per, 0.0);
        }
        HIPCHK(hipMemcpy(K.d_lp_cbar, lc.data(), sizeof(double) * lc.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_lp_sbar, ls.data(), sizeof(double) * ls.size(), hipMemcpyHostToDevice));
    }
    if (h->shape.sq_L() > 0) {
        const size_t per = 4 * N;
        std::vector<double> qc((size_t)hch * per), qs((size_t)hch * per);
        bool uni = true;
        for (int c = 0; c < hch; ++c) {
            double *q0 = qc.data() + c * per, *q1 = qs.data() + c * per;
            for (size_t k = 0; k < per; ++k) { q0[k] = K.h_cbar[c * nb + h->shape.bond[k]]; q1[k] = K.h_sbar[c * nb + h->shape.bond[k]]; }
            for (size_t k = 1; k < per; ++k) uni = uni && q0[k] == q0[0] && q1[k] == q1[0];       // uniform within the chain
        }
        K.sq_chain_uniform = uni;
        HIPCHK(hipMemcpy(K.d_sq_cbar, qc.data(), sizeof(double) * qc.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(K.d_sq_sbar, qs.data(), sizeof(double) * qs.size(), hipMemcpyHostToDevice));
    }
    K.hop_uniform = nb > 0 && !K.hop_per_chain();      // (read by the honeycomb and patch-layout forms only)
    for (size_t k = 1; k < nb && K.hop_uniform; ++k) K.hop_uniform = K.h_cbar[k] == K.h_cbar[0] && K.h_sbar[k] == K.h_sbar[0];
    K.hop_uploaded = true;
    return ELPH_OK;
}

// The Arnoldi bounds of every chain the caller does not skip, on the device (kpm_dev.hip: all chains in one launch; eb[2c] = e_min and
// eb[2c+1] = e_max).  ELPH_E_UNSUPPORTED where the kernel refuses the shape: eb is untouched and the caller takes the host path.
static int kpm_bounds_device(elph_handle_s *h, const double *b_max, const double *b_min, const std::vector<char> &skip, std::vector<double> &eb) {
    KpmState &K = h->kpm;
    const int N = (int)h->N, nch = K.nch();
    const size_t nst = (size_t)2 * nch * N;
    if (!K.d_start) RC(dev_alloc(&K.d_start, (size_t)K.tab_cap * (2 * N + 2)));
    HIPCHK(hipMemcpyAsync(K.d_start, b_max, sizeof(double) * (size_t)nch * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(K.d_start + (size_t)nch * N, b_min, sizeof(double) * (size_t)nch * N, hipMemcpyHostToDevice, h->stream));
    RC(elph_kpm_bounds_dev(h, nch, K.d_start, K.d_start + nst));
    std::vector<double> dev((size_t)2 * nch);
    HIPCHK(hipMemcpyAsync(dev.data(), K.d_start + nst, sizeof(double) * 2 * (size_t)nch, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < nch; ++c)
        if (!skip[(size_t)c]) { eb[2 * (size_t)c] = dev[2 * (size_t)c]; eb[2 * (size_t)c + 1] = dev[2 * (size_t)c + 1]; }
    return ELPH_OK;
}

// The same on the host (kpm_host.cpp), chain by chain: needs Ē (and the averaged hoppings) on the host
static int kpm_bounds_host(elph_handle_s *h, const double *b_max, const double *b_min, const std::vector<char> &skip, std::vector<double> &eb) {
    KpmState &K = h->kpm;
    const int N = (int)h->N, nch = K.nch();
    HIPCHK(hipMemcpy(K.h_Ebar.data(), K.d_Ebar, sizeof(double) * (size_t)nch * N, hipMemcpyDeviceToHost));
    for (int c = 0; c < nch; ++c)
        if (!skip[(size_t)c]) (void)elph_kpm_arnoldi(h, c, b_max + (size_t)c * N, b_min + (size_t)c * N, &eb[2 * (size_t)c], &eb[2 * (size_t)c + 1]);
    return ELPH_OK;
}

// Whether setup!(P) asks the device for its bounds: three chains and more on a lattice of one wave, or as ELPH_KPM_HOST / ELPH_KPM_DEVICE pin it
// (one or two chains: the host's scalar Arnoldi + LAPACK-style QR, 0.1 ms per chain, beats a kernel whose one wave spends
//  ~0.25 ms on the same sequential work; from three chains on all of them run side by side on the device)
static bool kpm_bounds_on_device(const elph_handle_s *h) {
    const char *eh = getenv("ELPH_KPM_HOST"), *ed = getenv("ELPH_KPM_DEVICE");     // read per call: tests pin one path
    const bool host_only = eh && eh[0] == '1', dev_always = ed && ed[0] == '1';
    return !host_only && h->N <= 512 && (h->kpm.nch() >= 3 || dev_always);
}

// The Arnoldi bounds of the chains not skipped, on the device when the caller asks for it and the kernel takes the shape, else on the host;
// *ran_on_device says which
static int kpm_bounds_arnoldi(elph_handle_s *h, bool device, const double *b_max, const double *b_min, const std::vector<char> &skip,
                              std::vector<double> &eb, int *ran_on_device) {
    if (ran_on_device) *ran_on_device = 0;
    if (device) {
        const int rcd = kpm_bounds_device(h, b_max, b_min, skip, eb);
        if (rcd == ELPH_OK && ran_on_device) *ran_on_device = 1;
        if (rcd != ELPH_E_UNSUPPORTED) return rcd;
    }
    return kpm_bounds_host(h, b_max, b_min, skip, eb);
}

// The eigenvalue bounds of every chain (:272-273), eb[2c] = e_min and eb[2c+1] = e_max: injected, or the Arnoldi process with the caller's
// start vectors — on the device for all chains at once (kpm_dev.hip: one wavefront per chain and per operator, Ritz values by a
// wave-parallel Hessenberg QR), on the host for lattices beyond one wave
static int kpm_bounds(elph_handle_s *h, const double *b_max, const double *b_min, const double *e_min, const double *e_max,
                      std::vector<double> &eb) {
    const int nch = h->kpm.nch();
    std::vector<char> injected((size_t)nch, 0);
    eb.assign((size_t)2 * nch, NAN);
    bool need_arnoldi = false;
    for (int c = 0; c < nch; ++c) {
        injected[(size_t)c] = e_min && e_max && std::isfinite(e_min[c]) && std::isfinite(e_max[c]);
        if (injected[(size_t)c]) { eb[2 * (size_t)c] = e_min[c]; eb[2 * (size_t)c + 1] = e_max[c]; } else need_arnoldi = true;
    }
    if (!need_arnoldi) return ELPH_OK;
    if (!(b_max && b_min)) { elph_set_error("Arnoldi start vectors required when bounds are not injected"); return ELPH_E_ARG; }
    return kpm_bounds_arnoldi(h, kpm_bounds_on_device(h), b_max, b_min, injected, eb, nullptr);
}

// the device copies of the tables
static int kpm_upload(elph_handle_s *h) {
    KpmState &K = h->kpm;
    const KpmTables &T = K.tab;
    const size_t ncoeff = T.coeff.size() / 2;
    if (ncoeff > K.coeff_cap) {
        RC(dev_alloc(&K.d_coeff, ncoeff));
        K.coeff_cap = ncoeff;
    }
    HIPCHK(hipMemcpy(K.d_coeff, T.coeff.data(), ncoeff * sizeof(double2), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_order, T.order.data(), sizeof(int) * T.order.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_coff, T.coff.data(), sizeof(int) * T.coff.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_wsched, T.wsched.data(), sizeof(int) * T.wsched.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_desc, T.desc.data(), sizeof(KpmDesc) * T.desc.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_fold, T.fold.data(), sizeof(double) * T.fold.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(K.d_lam, T.lam.data(), sizeof(double) * T.lam.size(), hipMemcpyHostToDevice));
    return ELPH_OK;
}

// setup!(P) for every chain resident in the handle (h->nchains of them).  All arrays are per chain.
static int kpm_setup_core(elph_handle_s *h, const KpmSource &src, const double *b_max, const double *b_min, const double *e_min,
                          const double *e_max, int *active, double *lam_lo, double *lam_hi) {
    KpmState &K = h->kpm;
    if (!K.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    if (!src.Ebar) RC(need_model(h));      // (an injected Ē is all the expansion needs: that handle never multiplies by M)
    HIPCHK(hipStreamSynchronize(h->stream));
    RC(kpm_reserve(h, h->nchains));
    RC(kpm_update_A(h, src));
    std::vector<double> eb;
    RC(kpm_bounds(h, b_max, b_min, e_min, e_max, eb));
    if (elph_kpm_plan(K, (int)h->L, eb.data())) RC(kpm_upload(h));
    K.ready = true;
    for (int c = 0; c < K.nch(); ++c) {
        if (active) active[c] = K.chains[(size_t)c].active;
        if (lam_lo) lam_lo[c] = K.chains[(size_t)c].lam_lo;
        if (lam_hi) lam_hi[c] = K.chains[(size_t)c].lam_hi;
    }
    return ELPH_OK;
}

// elph_bench.h: the bounds as kpm_bounds' two branches compute them, with nothing of setup!(P) after them
extern "C" int elph_bench_kpm_bounds(elph_handle h, int where, const double *b_max, const double *b_min, double *e_out, int *ran_on_device) {
    CHECK_H(h);
    KpmState &K = h->kpm;
    if (!K.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    if (!b_max || !b_min || !e_out || where < 0 || where > 2) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(need_model(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    RC(kpm_reserve(h, h->nchains));
    RC(kpm_update_A(h, KpmSource()));
    const std::vector<char> none((size_t)K.nch(), 0);
    std::vector<double> eb((size_t)2 * K.nch(), NAN);
    RC(kpm_bounds_arnoldi(h, where == 1 || (where == 2 && kpm_bounds_on_device(h)), b_max, b_min, none, eb, ran_on_device));
    std::copy(eb.begin(), eb.end(), e_out);
    return ELPH_OK;
}

// setup!(P) of a Holstein handle whose τ-averaged exp(−ΔτV) comes from OUTSIDE (KpmSource).  One chain.
int elph_i_kpm_setup_ebar(elph_handle_s *h, const double *Ebar_host, const double *b_max, const double *b_min) {
    if (h->kind != ELPH_MODEL_HOLSTEIN || !h->kpm.created) { elph_set_error("Ē injection: a Holstein handle with elph_kpm_create done"); return ELPH_E_STATE; }
    set_nchains(h, 1);
    return kpm_setup_core(h, KpmSource{Ebar_host, nullptr, nullptr}, b_max, b_min, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// setup!(P) of a bond-phonon handle whose τ-averaged hopping tables come from OUTSIDE (KpmSource); exp(Δτμ) is the handle's own
// (elph_update_model_ssh once; μ does not move).  One chain.
int elph_i_kpm_setup_csbar(elph_handle_s *h, const double *cbar_host, const double *sbar_host, const double *b_max, const double *b_min) {
    if (h->kind != ELPH_MODEL_SSH || !h->kpm.created || !h->have_E) {
        elph_set_error("c̄ / s̄ injection: a bond-phonon handle with elph_kpm_create and one elph_update_model_ssh done");
        return ELPH_E_STATE;
    }
    set_nchains(h, 1);
    return kpm_setup_core(h, KpmSource{nullptr, cbar_host, sbar_host}, b_max, b_min, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int elph_kpm_setup(elph_handle h, const double *b_max, const double *b_min, double e_min, double e_max,
                              int *active, double *lam_lo, double *lam_hi) {
    CHECK_H(h);
    if (h->nchains != 1) { elph_set_error("%d phonon configurations are resident: use elph_kpm_setup_chains", h->nchains); return ELPH_E_STATE; }
    return kpm_setup_core(h, KpmSource(), b_max, b_min, &e_min, &e_max, active, lam_lo, lam_hi);
}

extern "C" int elph_kpm_setup_chains(elph_handle h, const double *b_max, const double *b_min, const double *e_min,
                                     const double *e_max, int *active, double *lam_lo, double *lam_hi) {
    CHECK_H(h);
    return kpm_setup_core(h, KpmSource(), b_max, b_min, e_min, e_max, active, lam_lo, lam_hi);
}

extern "C" int elph_kpm_orders(elph_handle h, int64_t *orders, int64_t *total) {
    CHECK_H(h);
    if (!h->kpm.created) { elph_set_error("elph_kpm_create has not been called"); return ELPH_E_STATE; }
    const int Lo2 = (int)((h->L + 1) / 2);
    int64_t tot = 0;
    for (int w = 0; w < Lo2; ++w) {
        const int o = h->kpm.chains.empty() ? 1 : h->kpm.chains[0].order[w];
        if (orders) orders[w] = o;
        tot += o;
    }
    if (total) *total = tot;
    return ELPH_OK;
}

extern "C" int elph_kpm_apply_dev(elph_handle h, double *z_dev, const double *r_dev) {
    CHECK_H(h);
    if (!h->kpm.ready) { elph_set_error("elph_kpm_setup has not been called"); return ELPH_E_STATE; }
    if (!z_dev || !r_dev) { elph_set_error("null argument"); return ELPH_E_ARG; }
    RC(elph_launch_r2s(h, h->work.r, r_dev, 1));
    RC(elph_launch_kpm_apply(h, h->work.zp, h->work.r, 1, 0));
    RC(elph_launch_s2r(h, z_dev, h->work.zp, 1));
    return ELPH_OK;
}

extern "C" int elph_kpm_apply(elph_handle h, double *z, const double *r) {
    CHECK_H(h);
    if (!z || !r) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t bytes = (size_t)h->ndim * sizeof(double);
    HIPCHK(hipMemcpyAsync(h->work.stage_in, r, bytes, hipMemcpyHostToDevice, h->stream));
    RC(elph_kpm_apply_dev(h, h->work.stage_out, h->work.stage_in));
    HIPCHK(hipMemcpyAsync(z, h->work.stage_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// Fourier acceleration / twisted FFT
// ------------------------------------------------------------------------------------------

extern "C" int elph_fourier_accelerate(elph_handle h, double *vout, const double *vin, const double *diag, double power,
                                       int64_t nph) {
    CHECK_H(h);
    if (!vout || !vin || !diag || nph < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    const int64_t L = h->L, n = nph * L;
    // scratch: 3 real vectors of n + complex half spectrum; grown on demand (nph may exceed nsites for SSH)
    const int64_t need = 3 * n + 2 * (L / 2 + 1) * nph;
    if (need > h->diag_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        RC(dev_alloc(&h->d_diag, (size_t)need));
        h->diag_cap = need;
    }
    double *dR = h->d_diag, *aS = h->d_diag + n, *bS = h->d_diag + 2 * n;
    double2 *u = reinterpret_cast<double2 *>(h->d_diag + 3 * n);
    // stage (layout R -> S for "nph" columns), transform with the handle's tables, stage back
    HIPCHK(hipMemcpyAsync(dR, diag, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, bS, dR, 1, (int)nph));          // bS = diag in layout S  (diag[k][s])
    HIPCHK(hipMemcpyAsync(dR, vin, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    RC(elph_launch_r2s(h, aS, dR, 1, (int)nph));          // aS = v in layout S
    RC(elph_dft_accel(h, dR, aS, bS, power, (int)nph, u, 1));   // dR = result in layout S
    RC(elph_launch_s2r(h, aS, dR, 1, (int)nph));          // aS = result in layout R
    HIPCHK(hipMemcpyAsync(vout, aS, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_tau_to_omega(elph_handle h, double *nu_complex, const double *v) {
    CHECK_H(h);
    if (!nu_complex || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t nd = (size_t)h->ndim;
    RC(elph_work_reserve(h, 2));   // complex scratch = 2 real vectors
    RC(elph_stage_in(h, h->work.b, v, 1));
    double2 *fullS = reinterpret_cast<double2 *>(h->work.p);           // [L][N] complex
    RC(elph_launch_tau_to_omega(h, fullS, h->work.b));
    // complex layout S -> complex layout R: transpose re and im planes separately via a strided copy
    // (API convenience path; the solver itself never leaves layout S)
    std::vector<double> tmp(2 * nd);
    HIPCHK(hipMemcpyAsync(tmp.data(), fullS, 2 * nd * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->N, L = (size_t)h->L;
    for (size_t k = 0; k < L; ++k)
        for (size_t s = 0; s < N; ++s) {
            nu_complex[2 * (s * L + k)] = tmp[2 * (k * N + s)];
            nu_complex[2 * (s * L + k) + 1] = tmp[2 * (k * N + s) + 1];
        }
    return ELPH_OK;
}

extern "C" int elph_omega_to_tau(elph_handle h, double *v, const double *nu_complex) {
    CHECK_H(h);
    if (!nu_complex || !v) { elph_set_error("null argument"); return ELPH_E_ARG; }
    const size_t nd = (size_t)h->ndim, N = (size_t)h->N, L = (size_t)h->L;
    RC(elph_work_reserve(h, 2));
    std::vector<double> tmp(2 * nd);
    for (size_t k = 0; k < L; ++k)
        for (size_t s = 0; s < N; ++s) {
            tmp[2 * (k * N + s)] = nu_complex[2 * (s * L + k)];
            tmp[2 * (k * N + s) + 1] = nu_complex[2 * (s * L + k) + 1];
        }
    double2 *fullS = reinterpret_cast<double2 *>(h->work.p);
    HIPCHK(hipMemcpy(fullS, tmp.data(), 2 * nd * sizeof(double), hipMemcpyHostToDevice));
    RC(elph_launch_omega_to_tau(h, h->work.x, fullS));
    RC(elph_stage_out(h, v, h->work.x, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

// ------------------------------------------------------------------------------------------
// measurement hooks (bench.py)
// ------------------------------------------------------------------------------------------

static int bench_launch_unit(elph_handle_s *h, int what, int nrhs) {
    switch (what) {
        case 0: return elph_launch_mul(h, 2, h->work.z, h->work.b, nrhs);
        case 1: return elph_launch_cg_iteration(h, nrhs, 0);
        case 2: return elph_launch_kpm_apply(h, h->work.zp, h->work.b, nrhs, 0);
        case 3: return elph_launch_cg_iteration(h, nrhs, 1);
        case 11: return ELPH_E_ARG;      // (two half-batches on two streams: elph_bench_run drives both handles itself)
        case 4: return elph_launch_cg_kernel(h, nrhs, 0);
        case 5: return elph_launch_cg_kernel(h, nrhs, 1);
        default: {
            // 6, 7, 8: the three kernels of the KPM apply as the preconditioned iteration (case 3) launches them, one at a time
            return elph_launch_kpm_apply(h, h->work.zp, h->work.r, nrhs, h->plan.xr_in_fwd ? 2 : 1, 1 << (what - 6));
        }
    }
}

extern "C" int elph_bench_prepare(elph_handle h, int what, int nrhs, const double *B) {
    CHECK_H(h);
    RC(need_model(h));
    if (nrhs < 1 || what < 0 || what > 12) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if ((what == 2 || what == 3 || what == 10 || what == 11 || (what >= 6 && what <= 8)) && !h->kpm.ready) { elph_set_error("KPM not set up"); return ELPH_E_STATE; }
    RC(elph_work_reserve(h, nrhs));
    if (B) {
        RC(elph_stage_in(h, h->work.b, B, nrhs));
    }
    // fixed-count CG: tol = 0 never converges, kmax = inf, x0 = 0
    CgParams P;
    P.tol = 0.0; P.kmax = INFINITY; P.maxiter = (long long)1 << 40; P.use_prec = (what == 3 || what == 10 || what == 11 || (what >= 6 && what <= 8)); P.record_hist = 0; P.hist_stride = 0;
    h->cur_params = P;
    HIPCHK(hipMemsetAsync(h->work.x, 0, (size_t)nrhs * (size_t)h->ndim * sizeof(double), h->stream));
    h->x_zero = false;
    RC(elph_launch_cg_init(h, nrhs, P.use_prec, true));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->x_zero = true;      // (x is zero: the elph_bench_run(9 | 10) that follows consumes the hint as run_cg does)
    return ELPH_OK;
}

extern "C" int elph_bench_get_x(elph_handle h, int nrhs, double *X) {
    CHECK_H(h);
    if (nrhs < 1 || nrhs > h->work.cap_rhs || !X) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    RC(elph_stage_out(h, X, h->work.x, nrhs));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ELPH_OK;
}

extern "C" int elph_bench_info(elph_handle h, int nrhs, int *slices_per_wave) {
    CHECK_H(h);
    if (nrhs < 1 || !slices_per_wave) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *slices_per_wave = h->plan.T;      // (of the batch elph_bench_prepare planned)
    return ELPH_OK;
}

// Health of the workgroup-resident kernels on this handle: *cooling_down = solves left on the streaming iteration after a team timed
// out (0: the resident kernel is in use), *fallbacks = how many launches were given up and re-solved by the streaming iteration.
extern "C" int elph_wg_status(elph_handle h, int *cooling_down, int64_t *fallbacks) {
    CHECK_H(h);
    if (cooling_down) *cooling_down = h->res.cooldown;
    if (fallbacks) *fallbacks = h->res.fallbacks;
    return ELPH_OK;
}

extern "C" int elph_bench_wg_info(elph_handle h, int nrhs, int *usable, int *T, int *W, int *G) {
    CHECK_H(h);
    if (!usable || nrhs < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    int t = 0, w = 0, g = 0;
    *usable = (!h->res.cooling() && elph_wg_usable(h, &t, &w, &g, nrhs)) ? 1 : 0;
    if (T) *T = t;
    if (W) *W = w;
    if (G) *G = g;
    return ELPH_OK;
}

extern "C" int elph_bench_px_info(elph_handle h, int *fused) {
    CHECK_H(h);
    if (!fused) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    *fused = h->plan.px ? (h->plan.ap == CgPlan::AP_SQ16 ? 2 : 1) : 0;      // 2: with the register-exchange k_cg_ap of the 16 x 16 lattice (cg_sq16.hip)
    return ELPH_OK;
}

extern "C" int elph_bench_pg_info(elph_handle h, int *kind, int *px, int *py, int *nw, int *tables) {
    CHECK_H(h);
    if (kind) *kind = h->shape.patch_kind();
    if (px) *px = h->shape.PX;
    if (py) *py = h->shape.PY;
    if (nw) *nw = std::max(h->shape.NW, 1);
    if (tables) *tables = (h->shape.patch() && h->kind == ELPH_MODEL_HOLSTEIN && !h->shape.hop_uniform && elph_pg_disorder_ok(h)) ? 1 : 0;
    return ELPH_OK;
}

// the time-axis chunking of the patch mat-vec kernels (pgrid.hip: elph_pg_chunks): from the rule's own inputs without a device, and as this handle
// would launch nvec vectors now (pg_launch_shape's re-shaping and the pin ELPH_PG_T included)
extern "C" int elph_bench_pg_chunks(int kernel, int px, int py, int nw, int honeycomb, int64_t nvec, int64_t ltau, int *out) {
    if (!out || kernel < PG_K_MUL || kernel > PG_K_CG_AP_PX || px < 1 || py < 1 || nw < 1 || nvec < 1 || ltau < 1 || ltau > INT32_MAX) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    const PgChunks ck = elph_pg_chunks(kernel, px, py, nw, honeycomb != 0, (long long)nvec, (int)ltau);
    out[0] = ck.T; out[1] = ck.nch; out[2] = ck.last;
    return ELPH_OK;
}
extern "C" int elph_bench_pg_chunk_info(elph_handle h, int kernel, int nvec, int *out) {
    CHECK_H(h);
    if (!out || kernel < PG_K_MUL || kernel > PG_K_CG_AP_PX || nvec < 1) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (!h->shape.patch()) { elph_set_error("this handle has no patch layout"); return ELPH_E_UNSUPPORTED; }
    elph_pg_chunk_probe(h, kernel, nvec, out);
    return ELPH_OK;
}

// what elph_create recognises in a bond table, on a host-only handle (no device): the slots of _lib.LATTICE_SHAPE_SLOTS
extern "C" int elph_bench_lattice_shape(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht,
                                        const double *sinht, int *out) {
    if (!out || (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) || nsites < 1 || nsites > ELPH_MAX_SITES || nbonds < 0) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    elph_handle_s h;
    h.kind = kind; h.N = nsites; h.nb = nbonds;
    colour_bonds(&h, neighbor_table);
    if (kind == ELPH_MODEL_HOLSTEIN) { h.h_c.assign(cosht, cosht + nbonds); h.h_s.assign(sinht, sinht + nbonds); }
    const LatticeShape sh = elph_recognise_lattice(&h);
    const bool sq = sh.small_square(), hc = sh.honeycomb();
    const int v[] = {sq ? sh.LX : 0, sq ? sh.LY : 0, sh.dpp(), hc ? sh.LX : 0, hc ? sh.LY : 0, sh.hc12(), sh.patch_kind(), sh.patch() ? sh.LX : 0, sh.PX, sh.PY,
                     std::max(sh.NW, 1), sh.GX, sh.GY, sh.hgrid_regs(), sh.hop_uniform, sh.sq_L() > 0 ? 1 : sh.patch_kind() == LatticeShape::SQUARE ? 2 : 0};
    std::copy(std::begin(v), std::end(v), out);
    return ELPH_OK;
}

// the plan of the resident CG launch that elph_create's handle would make for this bond table and time axis, on a host-only handle (no
// device): the slots of _lib.WG_PLAN_SLOTS
extern "C" int elph_bench_wg_plan(int kind, int64_t nsites, int64_t ltau, int64_t nbonds, const int64_t *neighbor_table, const double *cosht,
                                  const double *sinht, int nrhs, int world, int *out) {
    if (!out || (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) || nsites < 1 || nsites > ELPH_MAX_SITES || ltau < 1 || nbonds < 0 || nrhs < 1 || world < 0) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    elph_handle_s h;
    h.kind = kind; h.N = nsites; h.L = ltau; h.nb = nbonds; h.ndim = nsites * ltau;
    h.npl = (int)((nsites + ELPH_WAVE - 1) / ELPH_WAVE);
    colour_bonds(&h, neighbor_table);
    if (kind == ELPH_MODEL_HOLSTEIN) { h.h_c.assign(cosht, cosht + nbonds); h.h_s.assign(sinht, sinht + nbonds); }
    plan_lane_program(&h);
    elph_i_wg_plan_probe(&h, nrhs, world, out);
    return ELPH_OK;
}

// the plan of one tau-axis transform (dft_mfma.hip: elph_plan_dft) at Ltau = ltau without a device, and on a handle's own h->dft.shape: the
// slots of _lib.DFT_PLAN_SLOTS
extern "C" int elph_bench_dft_plan(int64_t ltau, int which, int inverse, int N, int nvec, int nrz_slots, int *out) {
    if (!out || ltau < 1 || (which != DFT_TWISTED && which != DFT_PLAIN) || N < 1 || nvec < 1 || nrz_slots < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    elph_i_dft_plan_probe(dft_shape(ltau), which, inverse != 0, N, nvec, nrz_slots, out);
    return ELPH_OK;
}
extern "C" int elph_bench_dft_info(elph_handle h, int which, int inverse, int N, int nvec, int nrz_slots, int *out) {
    CHECK_H(h);
    if (!out || (which != DFT_TWISTED && which != DFT_PLAIN) || N < 1 || nvec < 1 || nrz_slots < 0) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    elph_i_dft_plan_probe(h->dft.shape, which, inverse != 0, N, nvec, nrz_slots, out);
    return ELPH_OK;
}

extern "C" int elph_bench_run(elph_handle h, int what, int nrhs, int reps, int use_graph, double *ms_total) {
    CHECK_H(h);
    if (nrhs < 1 || nrhs > h->work.cap_rhs || reps < 1 || !ms_total || what < 0 || what > 12) { elph_set_error("bad argument"); return ELPH_E_ARG; }
    if (use_graph) { elph_set_error("elph_bench_run: captured-graph replay is not supported (use_graph must be 0)"); return ELPH_E_UNSUPPORTED; }
    if (what == 12) {        // `reps` un-preconditioned iterations of every right-hand side in the slab form of a large lattice (slabs.hip): sum of the launches' event times
        if (!elph_i_slabs_usable(h, nrhs)) { elph_set_error("the slab form does not apply to this handle / batch"); return ELPH_E_UNSUPPORTED; }
        bool ran = false;
        std::vector<int64_t> its((size_t)nrhs);
        RC(elph_i_slabs_solve(h, nrhs, h->cur_params, reps, its.data(), &ran, ms_total));
        if (!ran) { elph_set_error("the slab form gave up (time-out)"); return ELPH_E_HIP; }
        return ELPH_OK;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    int rc = ELPH_OK;
    if (what == 9 || what == 10) {        // `reps` iterations of the whole batch in one launch of the workgroup-resident kernel (10: the preconditioned one)
        bool ran = false, aborted = false;
        const bool x0_zero = h->x_zero;      // (x is known to be zero only right after elph_bench_prepare)
        h->x_zero = false;
        CgBufs B = elph_make_bufs(h, nrhs);
        B.params = h->cur_params;
        hipError_t er = hipStreamSynchronize(h->stream);
        if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
        if (er == hipSuccess) {
            rc = elph_wg_cooldown_step(h);
            if (rc == ELPH_OK) rc = (what == 9) ? elph_wg_cg(h, B, nrhs, reps, x0_zero, nullptr, &ran) : elph_pcg_wg(h, B, nrhs, reps, nullptr, &ran);
            if (rc == ELPH_OK && !ran) { elph_set_error("the workgroup-resident kernel does not apply to this handle"); rc = ELPH_E_UNSUPPORTED; }
        }
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventRecord(e1, h->stream);
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventSynchronize(e1);
        float ms = 0.f;
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (er != hipSuccess) { elph_set_error("bench (workgroup-resident): %s", hipGetErrorString(er)); return ELPH_E_HIP; }
        if (rc) return rc;
        RC(elph_wg_aborted(h, &aborted));
        if (aborted) { elph_wg_timed_out(h); return ELPH_E_HIP; }
        *ms_total = (double)ms;
        return ELPH_OK;
    }
    if (what == 11) {        // `reps` preconditioned iterations of the batch as two half-batches on two streams (run_cg's form from 192 right-hand sides)
        if (!split_legal(h, nrhs, 1, false)) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); elph_set_error("the two-stream form does not apply to this batch"); return ELPH_E_UNSUPPORTED; }
        SplitRun S(h, nrhs);
        hipError_t er = hipStreamSynchronize(h->stream);
        if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
        if (er == hipSuccess) rc = split_begin(h, nrhs, S);
        for (int r = 0; r < reps && rc == ELPH_OK && er == hipSuccess; ++r) rc = split_iteration(S, 1);
        if (rc == ELPH_OK && er == hipSuccess) rc = split_join(S);
        if (S.on) h->ap_count = S.view[S.ways - 1]->ap_count;
        S.ok = (rc == ELPH_OK && er == hipSuccess);
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventRecord(e1, h->stream);
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventSynchronize(e1);
        float ms = 0.f;
        if (er == hipSuccess && rc == ELPH_OK) er = hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (er != hipSuccess) { elph_set_error("bench (two streams): %s", hipGetErrorString(er)); return ELPH_E_HIP; }
        if (rc) return rc;
        *ms_total = (double)ms;
        return ELPH_OK;
    }
    if (rc == ELPH_OK) {
        hipError_t er = hipStreamSynchronize(h->stream);
        if (er == hipSuccess) er = hipEventRecord(e0, h->stream);
        if (er == hipSuccess) {
            for (int r = 0; r < reps && rc == ELPH_OK; ++r) rc = bench_launch_unit(h, what, nrhs);
        }
        if (er == hipSuccess) er = hipEventRecord(e1, h->stream);
        if (er == hipSuccess) er = hipEventSynchronize(e1);
        float ms = 0.f;
        if (er == hipSuccess) er = hipEventElapsedTime(&ms, e0, e1);
        if (er != hipSuccess) { elph_set_error("elph_bench_run: %s", hipGetErrorString(er)); rc = ELPH_E_HIP; }
        else *ms_total = (double)ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}
