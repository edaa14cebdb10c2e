// lattice_shape.cpp — the host half of elph_create: check and colouring of the bond table, the lane program's plan, the recognition of the
// lattice, the handle without a device built from them.  Host only: no kernel, no HIP call; of other units it asks elph_set_error and elph_pg_mw.

#include <cstdlib>

#include "elph_internal.h"
#include "pgrid_dev.h"

// the bond-table arguments of elph_create (and of the device-free probes)
int check_bond_table(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht, const double *sinht) {
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

// Everything of a handle that needs no device, from the arguments of elph_create (checked: sizes, check_bond_table).  elph_create goes on to
// the device from here; the device-free probes (elph_bench_lattice_shape, elph_bench_wg_plan) read their answer off it.
void elph_i_host_handle(elph_handle_s *h, int kind, int64_t nsites, int64_t ltau, int64_t nbonds, const int64_t *neighbor_table,
                        const double *cosht, const double *sinht) {
    h->kind = kind; h->N = nsites; h->L = ltau; h->nb = nbonds; h->ndim = nsites * ltau;
    h->npl = (int)((nsites + ELPH_WAVE - 1) / ELPH_WAVE);
    colour_bonds(h, neighbor_table);
    if (kind == ELPH_MODEL_HOLSTEIN && nbonds > 0) { h->h_c.assign(cosht, cosht + nbonds); h->h_s.assign(sinht, sinht + nbonds); }
    plan_lane_program(h);
}

// what elph_create recognises in a bond table, on a host-only handle (no device): the slots of _lib.LATTICE_SHAPE_SLOTS
extern "C" int elph_bench_lattice_shape(int kind, int64_t nsites, int64_t nbonds, const int64_t *neighbor_table, const double *cosht,
                                        const double *sinht, int *out) {
    if (!out || (kind != ELPH_MODEL_HOLSTEIN && kind != ELPH_MODEL_SSH) || nsites < 1 || nsites > ELPH_MAX_SITES || nbonds < 0) {
        elph_set_error("bad argument"); return ELPH_E_ARG;
    }
    RC(check_bond_table(kind, nsites, nbonds, neighbor_table, cosht, sinht));
    elph_handle_s h;
    elph_i_host_handle(&h, kind, nsites, 1, nbonds, neighbor_table, cosht, sinht);      // (the shape does not depend on the time axis)
    const LatticeShape &sh = h.shape;
    const bool sq = sh.small_square(), hc = sh.honeycomb();
    const int v[] = {sq ? sh.LX : 0, sq ? sh.LY : 0, sh.dpp(), hc ? sh.LX : 0, hc ? sh.LY : 0, sh.hc12(), sh.patch_kind(), sh.patch() ? sh.LX : 0, sh.PX, sh.PY,
                     std::max(sh.NW, 1), sh.GX, sh.GY, sh.hgrid_regs(), sh.hop_uniform, sh.sq_L() > 0 ? 1 : sh.patch_kind() == LatticeShape::SQUARE ? 2 : 0};
    std::copy(std::begin(v), std::end(v), out);
    return ELPH_OK;
}
