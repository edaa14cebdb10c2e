// cg_fast.hip — latency-tuned gfx950 kernels for lattices whose checkerboard has <= 6 colours
// (every even-L square, honeycomb and triangular lattice of the reference's example decks).
// The kernels live in cg_fast_impl.inc, compiled per lane-program width — 4 colours (namespace lp4) and 6 (lp6) — and per sites-per-lane
// count (cg_fast_npl.hip, 8 translation units each; this file holds what is common to the counts: cg_fast_shared.inc) —
// the colour count is a compile-time loop bound (bonds live in registers, the fused forward/reverse sweep pairs colour
// cc with colour MC-1-cc), so a 4-colour lattice does not pay for the two stages only triangular lattices need.
//
// What differs from the generic kernels in kernels.hip (same arithmetic, same results):
//   * "lane program": the bond list is re-packed on the host per colour into [colour][pass][lane]
//     so that every lane keeps ITS bonds (site pair + cosh + sinh) in registers for the whole kernel;
//     a checkerboard colour is then  LDS read -> 4 FMAs -> LDS write -> wave barrier  with no
//     dependent global load inside the sweep (the generic kernel pays one L2 round trip per colour);
//   * every global load of the kernel (state, partial sums, vectors, exp(-dtau V), lane program)
//     is independent of every other and issued up front: one memory round trip per kernel;
//   * the p ping-pong index is a launch constant (launch parity) instead of device state;
//   * XCD-aware 1-D grid: workgroups with equal (blockIdx.x % 8) share an XCD/L2, so they are given
//     consecutive tau-slices — the tau+-1 halo re-reads of the fused MtM then hit the same L2.
//
// Reference semantics: see kernels.hip / SURVEY.md Appendix A.

#include "cg_fast_common.h"
#include "kpm_sq_dev.h"

#define ELPH_LP_MC 4
#define LPNS lp4
#include "cg_fast_shared.inc"
#undef ELPH_LP_MC
#undef LPNS

// the 6-colour instantiation lives in cg_fast6.hip
namespace lp6 {
int elph_fast_mul(elph_handle_s *h, int which, double *yS, const double *vS, int nvec);
int elph_fast_cg_ap(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool px);
int elph_fast_cg_xr(elph_handle_s *h, const CgBufs &B, int nrhs, int parity);
int elph_fast_kpm_cheb(elph_handle_s *h, int nrhs, const CgState *st, bool reg, double *rz_part, int nrz, const double *rr_part, int fold_nct);
}  // namespace lp6
// ---- dispatch on the handle's lane-program width ------------------------------------------------------------
int elph_fast_mul(elph_handle_s *h, int which, double *yS, const double *vS, int nvec) {
    return h->lp_mc == 4 ? lp4::elph_fast_mul(h, which, yS, vS, nvec) : lp6::elph_fast_mul(h, which, yS, vS, nvec);
}
int elph_choose_T(const elph_handle_s *h, int nrhs) { return lp4::elph_choose_T(h, nrhs); }
int elph_choose_T_px(const elph_handle_s *h, int nrhs, bool two_streams) { return lp4::elph_choose_T_px(h, nrhs, two_streams); }
int elph_fast_cg_ap(elph_handle_s *h, const CgBufs &B, int nrhs, int parity, bool px) {
    return h->lp_mc == 4 ? lp4::elph_fast_cg_ap(h, B, nrhs, parity, px) : lp6::elph_fast_cg_ap(h, B, nrhs, parity, px);
}
int elph_fast_cg_xr(elph_handle_s *h, const CgBufs &B, int nrhs, int parity) {
    return h->lp_mc == 4 ? lp4::elph_fast_cg_xr(h, B, nrhs, parity) : lp6::elph_fast_cg_xr(h, B, nrhs, parity);
}
int elph_fast_kpm_cheb(elph_handle_s *h, int nrhs, const CgState *st, bool reg, double *rz_part, int nrz, const double *rr_part, int fold_nct) {
    return h->lp_mc == 4 ? lp4::elph_fast_kpm_cheb(h, nrhs, st, reg, rz_part, nrz, rr_part, fold_nct)
                         : lp6::elph_fast_kpm_cheb(h, nrhs, st, reg, rz_part, nrz, rr_part, fold_nct);
}

// The register-exchange Chebyshev recursion of the lane family for this lattice (the four-colour kernels of elph_fast_kpm_cheb; the forms
// that can deliver r.z in frequency space), in the order the dispatch tries them; *hgn: cells per lane of the honeycomb grid form
int elph_reg_cheb_form(const elph_handle_s *h, int *hgn) {
    const bool hol = h->kind == ELPH_MODEL_HOLSTEIN;
    const LatticeShape &s = h->shape;
    if (s.dpp() > 0) return REG_SQ;
    // any other even-L square lattice (L = 4, 6, 10, 12, 14) with one (cosh, sinh) for every bond: the GRID layout
    if (s.sq_L() > 0 && h->kpm.sq_chain_uniform && hol) return REG_SQ_GRID;
    if (s.hc_L() > 0 && !s.hc12() && h->kpm.hop_uniform && hol && s.hgrid_regs()) {
        // any other square honeycomb lattice whose cells fit a grid of lanes, one (cosh, sinh) for every bond: the HGRID layout
        if (hgn) *hgn = s.hgrid_regs();
        return REG_HC_GRID;
    }
    // the honeycomb lattice of 12 x 12 cells with one (cosh, sinh) for every bond: the quad layout
    if (s.hc12() && h->kpm.hop_uniform && hol) return REG_HC12;
    return REG_NONE;
}

