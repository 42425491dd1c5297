// suhmo_hier.hip -- AMR hierarchies whose levels are UNIONS OF BOXES (suhmo_hier_int.h): the operator methods of a level, the merged
// launches over several levels, the AMR V-cycle and the composite residual, create / destroy, the options and the C-ABI.
//
// Cycle = suhmo_amr.hip's, arithmetic = oracle/amrm.c, bit for bit.
#include "suhmo_hier_int.h"
#include <string>

int suhmo_grad_cc(suhmo_level *L, int depth, hipStream_t st);          // suhmo_bcoef.hip
int suhmo_apply_and_residual_rects(suhmo_level *L, int depth, const int4 *d_rects, int n, int maxw, int maxh, hipStream_t st);   // suhmo_ops.hip
int suhmo_grad_cc_list(suhmo_level *L, int depth, const int2 *d_cells, int n, hipStream_t st);

using namespace hier;
namespace {
inline const suhmo_phys_t &phys_of(suhmo_hier *H, int l) { return H->lev[l].box[0]->ph; }
inline bool has_alpha(suhmo_hier *H, int l) { return H->lev[l].box[0]->d[0].v.alpha != 0.0; }
int hier_gsrb(suhmo_hier *H, int l, int sweeps, suhmo_stream_t s, bool may_swap = false)
{
    SUHMO_TIME("AMRNonLinearPoissonOp::relaxNF");
    if (l == 0) { H->phi_shadow_fresh = false; H->phi_ver[0]++; H->base_full_ver++; return suhmo_level_gsrb(base_of(H), 0, sweeps, s); }
    int rc;
    suhmo_multi m;
    if ((rc = multi_of(H, l, HST(s), m))) return rc;
    HLev &Vf = H->lev[l];
    if (sweeps > 0 && H->fused_relax && Vf.halo_ok && !Vf.part) {
        // two sweeps per launch: a box's workgroup relaxes the box and, redundantly, the 4 cells around it that belong to its neighbours,
        // reading their canvases directly -- no exchange between the colour passes, a quarter of the launches (suhmo_gsrb.hip:k_gsrb_box_m)
        if ((rc = ensure_field(H, l, SUHMO_F_PHI2)) || (rc = multi_of(H, l, HST(s), m))) return rc;
        if (Vf.self_wrap < 0) {                            // a box that is its own periodic neighbour: its physical ghost is another tile's cell
            Vf.self_wrap = 0;
            for (suhmo_level *L : Vf.box) { const DV &v = L->d[0].v; if ((v.per[0] && !v.cfx[0]) || (v.per[1] && !v.ext[0])) Vf.self_wrap = 1; }
        }
        const int bcg = H->merged_launches && !Vf.self_wrap;             // the closing ghost fill (:757-759) rides in the relaxation launches
        int src = SUHMO_F_PHI, dst = SUHMO_F_PHI2;
        const int per = H->box_sweeps;                      // sweeps per launch: 4 (the whole smoothing of num_smooth = 4) or 2
        for (int done = 0; done < sweeps; done += per) {
            const int npass = 2 * std::min(per, sweeps - done);
            if ((rc = suhmo_multi_gsrb_box(m, phys_of(H, l), has_alpha(H, l), Vf.halo.d, Vf.hbase.d, src, dst, npass, bcg, HST(s)))) return rc;
            std::swap(src, dst);
            H->phi_ver[l]++; H->n_fused_relax++;
        }
        if (src != SUHMO_F_PHI) {                          // an odd number of launches: the result is on the second canvas
            if (may_swap && Vf.d_fp_alt) {                 // (inside a V-cycle: that canvas becomes the head; vcycle_amr puts things back)
                swap_head(H, l);
                if (!bcg && (rc = multi_of(H, l, HST(s), m))) return rc;   // the closing fill below writes the ring of the new head
            } else if ((rc = launch_copy(m.on(), SUHMO_F_PHI, SUHMO_F_PHI2, HST(s)))) return rc;
        }
        return bcg ? 0 : launch_fill_ghosts(m.on(), SUHMO_F_PHI, 1, HST(s));                                  // :757-759
    }
    // exchange() before every colour pass (:692, :751): once here (unless the side ghosts are current), then every pass pushes
    // its new side cells into the ghost cells they feed
    if (sweeps > 0 && (rc = hier_ff(H, l, SUHMO_F_PHI, -1, false, HST(s)))) return rc;
    // owner computes: a pass relaxes this rank's boxes, the side cells of the colour it advanced travel to the ranks whose boxes lie across
    // those sides, and the exchange launch copies them into the ghost cells: the reference's own pattern, exchange() + pass (:692, :751)
    HLev &V = H->lev[l];
    const bool push = H->push_ghosts && !V.part;
    for (int it = 0; it < sweeps; it++)
        for (int pass = 0; pass < 2; pass++) {
            if ((rc = launch_colour_pass(m.on(), has_alpha(H, l), pass, 0, 0, push ? m.push : nullptr, m.pbase, HST(s)))) return rc;
            H->phi_ver[l]++;
            if (!push && (rc = hier_ff(H, l, SUHMO_F_PHI, -1, false, HST(s), V.part ? pass : -1))) return rc;
        }
    if (sweeps > 0 && (rc = launch_fill_ghosts(m.on(), SUHMO_F_PHI, 1, HST(s)))) return rc;                        // :757-759
    if (sweeps > 0 && push) H->ff_seen[l] = H->phi_ver[l];          // every pass pushed its side cells: the ghosts are current
    return 0;
}
int hier_level_residual(suhmo_hier *H, int l, suhmo_stream_t s)   // residualI: RES
{
    if (l == 0) return suhmo_level_residual(base_of(H), 0, s);
    int rc;
    suhmo_multi m;
    if ((rc = hier_ff(H, l, SUHMO_F_PHI, -1, false, HST(s))) || (rc = multi_of(H, l, HST(s), m))) return rc;
    return launch_apply_boxes(m.on(), has_alpha(H, l), 1, HST(s));            // (owner computes: m = this rank's boxes)
}
int hier_axby(suhmo_hier *H, int l, int dst, int x, int y, double a, double b, suhmo_stream_t s)
{
    if (l == 0) return suhmo_level_axby(base_of(H), 0, dst, x, y, a, b, s);
    int rc;
    suhmo_multi m;
    if ((rc = ensure_field(H, l, dst)) || (rc = ensure_field(H, l, x)) || (rc = ensure_field(H, l, y)) || (rc = multi_of(H, l, HST(s), m))) return rc;
    return launch_axby(m.on(), dst, x, y, a, b, HST(s));
}
int hier_copy(suhmo_hier *H, int l, int dst, int src, suhmo_stream_t s)
{
    int rc;
    if ((rc = ensure_field(H, l, dst)) || (rc = ensure_field(H, l, src))) return rc;
    if (dst == SUHMO_F_PHI) { for (suhmo_level *L : H->lev[l].box) L->d[0].phi_fresh = 0; H->phi_ver[l]++; }
    if (dst == SUHMO_F_PHI && l == 0) H->phi_shadow_fresh = false;
    if (dst == SUHMO_F_MASK) for (suhmo_level *L : H->lev[l].box) suhmo_mask_written(L);
    if (dst == SUHMO_F_ZB) for (suhmo_level *L : H->lev[l].box) suhmo_zb_written(L);
    if (l == 0) H->base_full_ver++;
    if (l == 0) {
        suhmo_level *L = base_of(H);
        HIPCHK(hipMemcpyAsync(L->d[0].fp.f[dst], L->d[0].fp.f[src], L->d[0].elems * sizeof(double), hipMemcpyDeviceToDevice, HST(s)));
        return 0;
    }
    suhmo_multi m;
    if ((rc = multi_of(H, l, HST(s), m))) return rc;
    return launch_copy(m.on(), dst, src, HST(s));
}
// head of level l: its coarse-fine ghosts from level l-1
int cf_phi(suhmo_hier *H, int l, suhmo_stream_t s)
{
    if (l == 0) return 0;
    if (H->cf_seen[l][0] == H->phi_ver[l] && H->cf_seen[l][1] == H->phi_ver[l - 1]) return 0;       // the ghosts are current
    if (H->merged_launches && !H->lev[l].part && H->ff_seen[l] != H->phi_ver[l]) {
        // the side ghosts between the boxes are stale as well (whoever reads the head next asks for them): both in one launch
        int rc = hier_cf_ff(H, l, SUHMO_F_PHI, SUHMO_F_PHI, -1, -1, false, HST(s));
        if (!rc) { H->cf_seen[l][0] = H->phi_ver[l]; H->cf_seen[l][1] = H->phi_ver[l - 1]; H->ff_seen[l] = H->phi_ver[l]; }
        return rc;
    }
    int rc = hier_cf(H, l, SUHMO_F_PHI, SUHMO_F_PHI, HST(s));
    if (!rc) { H->cf_seen[l][0] = H->phi_ver[l]; H->cf_seen[l][1] = H->phi_ver[l - 1]; }
    return rc;
}

// ---- several levels per launch (option merged_launches; this process holds every box and the whole of level 0)
inline bool levels_mergeable(const suhmo_hier *H) { return H->merged_launches && !H->part && !dist_base(H) && H->nlev <= SUHMO_LVMAX + 1; }
// the boxes of the levels lhi, lhi - 1, .. llo (>= 1) as one launch's table; mode_top for lhi, mode_rest for the others
int levels_boxes(suhmo_hier *H, int llo, int lhi, int mode_top, int mode_rest, suhmo_stream_t s, suhmo_lvboxes &lv)
{
    memset(&lv, 0, sizeof(lv));
    int rc;
    for (int l = lhi; l >= std::max(1, llo); l--) {
        suhmo_multi m;
        if ((rc = multi_of(H, l, HST(s), m))) return rc;
        const int q = lv.n++;
        lv.dv[q] = m.dv; lv.fp[q] = m.fp; lv.nbox[q] = m.nbox; lv.mode[q] = l == lhi ? mode_top : mode_rest;
        lv.maxnx = std::max(lv.maxnx, m.maxnx); lv.maxny = std::max(lv.maxny, m.maxny);
    }
    return 0;
}
// L(phi) and the residual of level 0 inside a composite residual: as it is (left behind by the cycle's last launch), on the rectangles the
// average from level 1 changed, or over the whole level
int base_apply_residual(suhmo_hier *H, bool whole_level_follows, suhmo_stream_t s)
{
    int rc;
    HLev &V1 = H->lev[1];
    if (!whole_level_follows && H->base_fused_ver == H->base_full_ver)
        { rc = 0; H->n_fused_residual++; }                                // L(phi) and rhs - L(phi) of the head as it is: written by the cycle's last launch
    else if (H->incremental && whole_level_follows && H->base_res_seen == H->base_full_ver)
        { rc = suhmo_apply_and_residual_rects(base_of(H), 0, V1.dirty0.d, (int)V1.dirty0.n, V1.dirty_w, V1.dirty_h, HST(s)); H->n_incr_residual++; }   // only what the average changed
    else rc = suhmo_apply_and_residual(base_of(H), 0, HST(s));
    H->base_res_seen = whole_level_follows ? 0 : H->base_full_ver;       // (the solve loop's evaluation is the one the next cycle can build on)
    return rc;
}
// RES of the levels llo .. lhi: level lhi's own residual (residualI), the composite residual with the reflux from the level above on the others
// (what hier_level_residual(lhi) and composite_residual(lhi), .., composite_residual(llo + 1) leave) in ONE launch per kind: ghosts, operator on
// the levels of boxes, [level 0], refluxes.  Nothing of one level's part reads what another's writes (ghosts from valid cells; L(phi) from the
// level's own head; a reflux adds fluxes of two heads to L(phi) of its coarse cells).
int levels_residual(suhmo_hier *H, int lhi, int llo, bool whole_level_follows, suhmo_stream_t s, bool average_down = false)
{
    int rc;
    if ((rc = ghosts_levels(H, llo, lhi, s))) return rc;
    for (int l = std::max(1, llo); l < lhi; l++) if ((rc = ensure_field(H, l, SUHMO_F_LPHI))) return rc;
    suhmo_lvboxes lv;
    if ((rc = levels_boxes(H, llo, lhi, 1, 3, s, lv)) || (rc = suhmo_levels_apply(lv, phys_of(H, lhi), has_alpha(H, lhi), HST(s)))) return rc;
    if (llo == 0 && (rc = base_apply_residual(H, whole_level_follows, s))) return rc;
    return reflux_levels(H, lhi, llo, average_down, s);
}

// cell-centred gradient of level l (compGradientCC) with its domain-side ghosts
int hier_grad_cc(suhmo_hier *H, int l, suhmo_stream_t s)
{
    if (l == 0) return suhmo_grad_cc(base_of(H), 0, HST(s));
    int rc;
    suhmo_multi m;
    if ((rc = hier_ff(H, l, SUHMO_F_PHI, -1, false, HST(s)))) return rc;              // UpdateOperator :47
    if ((rc = ensure_field(H, l, SUHMO_F_GRADX)) || (rc = ensure_field(H, l, SUHMO_F_GRADY)) || (rc = ensure_field(H, l, SUHMO_F_RE)) || (rc = multi_of(H, l, HST(s), m))) return rc;
    return suhmo_multi_grad_cc(m, HST(s));
}
// UpdateOperator of level l >= 1 with its coarser level (src/VCAMRNonLinearPoissonOp.cpp:34-64, src/AmrHydro.cpp:1415-1539)
int hier_update_operator(suhmo_hier *H, int l, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::UpdateOperator(AMR)");
    int rc;
    if (l - 1 >= 1 && levels_mergeable(H)) {
        // the gradients of this level and of the coarser one: their ghosts in one launch, the two gradients in one launch
        suhmo_lvboxes lv;
        if ((rc = ghosts_levels(H, l - 1, l, s))) return rc;
        for (int q = l - 1; q <= l; q++) for (int f : {SUHMO_F_GRADX, SUHMO_F_GRADY, SUHMO_F_RE}) if ((rc = ensure_field(H, q, f))) return rc;
        if ((rc = levels_boxes(H, l - 1, l, 0, 0, s, lv)) || (rc = suhmo_levels_grad_cc(lv, phys_of(H, l).use_mask_gradients, HST(s)))) return rc;
        if ((rc = hier_cf_ff(H, l, SUHMO_F_GRADX, SUHMO_F_GRADX, SUHMO_F_GRADY, SUHMO_F_GRADY, true, HST(s)))) return rc;
        suhmo_multi m;
        if ((rc = multi_of(H, l, HST(s), m))) return rc;
        faces_made(H, l);
        return suhmo_multi_re_bcoef(m, HST(s));
    }
    if ((rc = cf_phi(H, l - 1, s))) return rc;                    // the coarser level's own coarse-fine ghosts (its gradient reads them)
    if ((rc = hier_grad_cc(H, l, s))) return rc;
    // the coarse gradient is read by the coarse-fine interpolation below and by nothing else: on level 0 only the cells those
    // stencils touch are evaluated (a pass over the whole level otherwise, 86 us at 4096^2)
    if (l - 1 == 0 && H->incremental) { rc = suhmo_grad_cc_list(base_of(H), 0, H->lev[1].gcells.d, (int)H->lev[1].gcells.n, HST(s)); H->n_sparse_grad++; }
    else rc = hier_grad_cc(H, l - 1, s);
    if (rc) return rc;
    if (H->merged_launches && !H->lev[l].part) {
        if ((rc = hier_cf_ff(H, l, SUHMO_F_GRADX, SUHMO_F_GRADX, SUHMO_F_GRADY, SUHMO_F_GRADY, true, HST(s)))) return rc;
    } else {
        if ((rc = hier_cf(H, l, SUHMO_F_GRADX, SUHMO_F_GRADX, HST(s), SUHMO_F_GRADY, SUHMO_F_GRADY))) return rc;
        if ((rc = hier_ff(H, l, SUHMO_F_GRADX, SUHMO_F_GRADY, true, HST(s)))) return rc;  // lvlgradH.exchange() src/AmrHydro.cpp:1490
    }
    suhmo_multi m;
    if ((rc = multi_of(H, l, HST(s), m))) return rc;
    faces_made(H, l);
    return suhmo_multi_re_bcoef(m, HST(s));
}
// RES of level l-1 = rhs - [applyOpI(phi) + reflux from level l]; LPHI of level l-1 keeps the plain L(phi)
// whole_level_follows: called from inside a V-cycle (what follows turns RES of level l-1 into a FAS right-hand side); false: the
// residual evaluation of the solve loop
int composite_residual(suhmo_hier *H, int l, suhmo_stream_t s, bool whole_level_follows = true)
{
    int rc;
    // one pass writes LPHI and rhs - LPHI; the cells next to the coarse-fine faces then get rhs - (LPHI + flux mismatch): the
    // values of copy, reflux, axby(RES, RHS, -1, 1) over the whole level, without two of its three passes
    if ((rc = cf_phi(H, l - 1, s))) return rc;
    if (l - 1 == 0) rc = base_apply_residual(H, whole_level_follows, s);
    else {
        suhmo_multi m;
        if ((rc = hier_ff(H, l - 1, SUHMO_F_PHI, -1, false, HST(s))) || (rc = ensure_field(H, l - 1, SUHMO_F_LPHI)) || (rc = multi_of(H, l - 1, HST(s), m))) return rc;
        rc = launch_apply_boxes(m.on(), has_alpha(H, l - 1), 3, HST(s));
    }
    if (rc) return rc;
    if ((rc = cf_phi(H, l, s))) return rc;
    return hier_reflux(H, l, SUHMO_F_RES, HST(s), 1);
}
int vcycle_amr(suhmo_hier *H, int l, const suhmo_solver_params_t *sp, suhmo_stream_t s)
{
    if (l == 0) { H->phi_shadow_fresh = false; H->phi_ver[0]++; H->base_full_ver++; return suhmo_level_vcycle(base_of(H), sp, s); }
    int rc;
    if ((rc = cf_phi(H, l, s))) return rc;
    if (sp->bcoeff_otf && (rc = hier_update_operator(H, l, s))) return rc;
    if ((rc = hier_gsrb(H, l, sp->num_smooth, s, true))) return rc;                           // relaxNF
    if ((rc = hier_avg(H, l, SUHMO_F_PHI, SUHMO_F_PHI, 0, 0.0, HST(s)))) return rc;           // AMRRestrictS(skip_res)
    if (levels_mergeable(H)) { if ((rc = levels_residual(H, l, l - 1, true, s, true))) return rc; }      // (the average of the residual rides in the reflux launch)
    else {
        if ((rc = cf_phi(H, l, s))) return rc;
        if ((rc = hier_level_residual(H, l, s))) return rc;
        if ((rc = composite_residual(H, l, s))) return rc;
        if ((rc = hier_avg(H, l, SUHMO_F_RES, SUHMO_F_RES, 0, 0.0, HST(s)))) return rc;
    }
    // the right-hand side of level l-1 is set aside while its FAS problem runs: two canvases trade places on level 0 (its
    // pointers travel by value), a copy on a level of boxes (their pointers sit in a device table)
    SwapGuard rhs_aside;                                   // (trades back on every way out of this scope)
    if (l - 1 == 0) {
        rhs_aside.arm(&base_of(H)->d[0].fp.f[SUHMO_F_RHS], &base_of(H)->d[0].fp.f[SUHMO_F_RHS0]);
        if ((rc = hier_axby(H, 0, SUHMO_F_RHS, SUHMO_F_RES, SUHMO_F_LPHI, 1.0, 1.0, s))) return rc;
        if (dist_base(H) && (rc = suhmo_level_exchange(base_of(H), 0, SUHMO_F_RHS, s))) return rc;      // rank strips: rhs halo rows (relaxed redundantly)
        // the head of level 0 before its FAS problem: level 1 reads the correction of level 0 only through the windows of its boxes,
        // so only those cells are kept (and only their differences formed)
        if ((rc = hier_window_save(H, l, SUHMO_F_PHI, HST(s)))) return rc;
    } else {
        // a level of boxes: its right-hand side set aside, the FAS right-hand side formed, a copy of its head kept -- one launch
        // (copy RHS0 <- RHS, axby RHS <- RES + LPHI, copy PHIOLD <- PHI: the same expressions on the same operands)
        suhmo_multi mc;
        for (int f : {SUHMO_F_RHS0, SUHMO_F_PHIOLD, SUHMO_F_LPHI}) if ((rc = ensure_field(H, l - 1, f))) return rc;
        if ((rc = multi_of(H, l - 1, HST(s), mc)) || (rc = launch_fas_enter(mc.on(), HST(s)))) return rc;
    }
    if (l - 1 == 0) {
        // level 0's own V-cycle runs against the FAS right-hand side; its last launch is asked to leave L(phi) and TRUE rhs - L(phi) behind
        // (the true right-hand side waits on the second canvas): what the solve loop's residual evaluation computes next
        suhmo_level *B = base_of(H);
        B->resout_req = 3; B->resout_rhs = B->d[0].fp.f[SUHMO_F_RHS0]; B->resout_done = 0;
        rc = vcycle_amr(H, 0, sp, s);
        if (!rc && B->resout_done) H->base_fused_ver = H->base_full_ver;
        B->resout_req = 0; B->resout_rhs = nullptr; B->resout_done = 0;
        if (rc) return rc;
    } else if ((rc = vcycle_amr(H, l - 1, sp, s))) return rc;
    if (l - 1 == 0) { rhs_aside.back(); rc = hier_prolong2(H, l, SUHMO_F_PHI, HST(s), true); }                // AMRProlongS_2 of phi - phi_saved
    else {                                                                                    // RHS <- RHS0, CORR <- PHI - PHIOLD: one launch
        if ((rc = ensure_field(H, l - 1, SUHMO_F_CORR))) return rc;
        if (H->merged_launches) rc = hier_prolong2(H, l, SUHMO_F_PHI, HST(s), false, true);      // leaving and prolongation in one launch
        else {
            suhmo_multi mc;
            if ((rc = multi_of(H, l - 1, HST(s), mc)) || (rc = launch_fas_leave(mc.on(), HST(s)))) return rc;
            rc = hier_prolong2(H, l, SUHMO_F_CORR, HST(s));
        }
    }
    if (rc) return rc;
    if ((rc = cf_phi(H, l, s))) return rc;
    if ((rc = hier_gsrb(H, l, sp->num_smooth, s, true))) return rc;
    if (H->lev[l].swapped) {                               // (an odd number of odd relaxations: the head goes back to its own canvas by a copy after all)
        suhmo_multi m;
        if ((rc = multi_of(H, l, HST(s), m)) || (rc = launch_copy(m.on(), SUHMO_F_PHI2, SUHMO_F_PHI, HST(s)))) return rc;
        swap_head(H, l);
    }
    return 0;
}
// every C-ABI entry: the caller may have loaded new data
int check_hier(suhmo_hier *H)
{
    ARG(H && H->nlev >= 1);
    // a V-cycle that failed half way may have left a level with the canvases of its head trading places (swap_head): the head goes back to its
    // own canvas before anything else looks at the level
    for (int l = 1; l < H->nlev; l++)
        if (H->lev[l].swapped) {
            suhmo_multi m;
            int rc;
            HIPCHK(hipSetDevice(H->device));
            HIPCHK(hipDeviceSynchronize());
            if ((rc = multi_of(H, l, nullptr, m)) || (rc = launch_copy(m.on(), SUHMO_F_PHI2, SUHMO_F_PHI, nullptr))) return rc;
            HIPCHK(hipDeviceSynchronize());
            swap_head(H, l);
        }
    suhmo_hier_invalidate_(H);
    return 0;
}
}  // namespace

// ------------------------------------------------------------------ C-ABI
extern "C" int suhmo_hier_destroy(suhmo_hier_t *H)
{
    if (!H) return 0;
    (void)hipSetDevice(H->device);
    (void)hipDeviceSynchronize();
    if (H->gap) { (void)suhmo_hier_destroy(H->gap); H->gap = nullptr; }
    for (int f = 0; f < SUHMO_F_COUNT; f++) if (H->shadow.f[f]) (void)hipFree(H->shadow.f[f]);
    H->need.release(); H->need_c.release(); H->need_rl.release(); H->cover_full.release();
    if (H->cover_whole) (void)hipFree(H->cover_whole);
    if (H->red_all) (void)hipFree(H->red_all);
    if (H->xs) (void)hipFree(H->xs);
    if (H->xr) (void)hipFree(H->xr);
    if (H->snap_buf) (void)hipFree(H->snap_buf);
    suhmo_hier_flatten_release_(H);
    suhmo_hier_compare_release_(H);
    suhmo_hier_balance_release_(H);
    for (int l = 0; l < 8; l++) {
        HLev &V = H->lev[l];
        V.snap_cells[0].release(); V.snap_cells[1].release();
        for (suhmo_level *L : V.box) if (!(l == 0 && H->base_borrowed)) (void)suhmo_level_destroy(L);
        V.ff_side.release(); V.ff_all.release(); V.push.release(); V.pbase.release(); V.cf.release(); V.pwl.release(); V.avg.release(); V.wing.release();
            V.wstart.release(); V.halo.release(); V.hbase.release();
        V.targets.release(); V.faces.release(); V.dirty0.release(); V.gcells.release();
        if (V.winbuf) (void)hipFree(V.winbuf);
        if (V.winold) (void)hipFree(V.winold);
        if (V.d_win) (void)hipFree(V.d_win);
        if (V.d_wing_box) (void)hipFree(V.d_wing_box);
        if (V.d_fp) (void)hipFree(V.d_fp);
        if (V.d_fp_alt) (void)hipFree(V.d_fp_alt);
        if (V.d_dv) (void)hipFree(V.d_dv);
        if (V.d_red) (void)hipFree(V.d_red);
        for (Sync *S : {&V.sy_side[0], &V.sy_side[1], &V.sy_sides, &V.sy_all, &V.sy_cread, &V.sy_win, &V.sy_fface}) S->release();
        V.avg_cov.release(); V.avg_put.release(); V.avg_get.release();
    }
    for (suhmo_tagmap *&m : H->tags) { suhmo_tagmap_release(m); m = nullptr; }
    if (H->ps) (void)hipFree(H->ps);
    if (H->pr) (void)hipFree(H->pr);
    delete H;
    return 0;
}

extern "C" int suhmo_hier_create(suhmo_hier_t **out, const suhmo_level_desc_t *base, int nlev, const int *nbox, const int *boxes)
{
    return suhmo_hier_create_opts(out, base, nlev, nbox, boxes, nullptr);
}
// ---- the options: one entry each -- key, member, default, the form a value takes, whether only the creation string may set it, what a
// change resets.  suhmo_hier_create_opts, suhmo_hier_set_option and suhmo_hier_get_option walk this table; a gap hierarchy is created with
// its parent's current values
static long flag(long v) { return v != 0; }
static long two_or_four(long v) { return v >= 4 ? 4 : 2; }
static long at_least_one(long v) { return std::max(1L, v); }
static void stale_residual(suhmo_hier *H) { H->base_res_seen = 0; }
static void stale_ghosts(suhmo_hier *H) { for (unsigned long &v : H->ff_seen) v = 0; }
// (incremental_residual = 0: every composite residual / coarse gradient over the whole of level 0, A/B runs and tests; shadow = 1: an uncut
// level 0 read through the shadow path all the same, tests; the others: the members of suhmo_hier)
struct HierOpt { const char *key; long suhmo_hier::*m; long dflt; long (*form)(long); bool creation_only; void (*reset)(suhmo_hier *); };
static const HierOpt hier_opts[] = {
    {"push_ghosts",          &suhmo_hier::push_ghosts,     1,      flag,         false, stale_ghosts},
    {"incremental_residual", &suhmo_hier::incremental,     1,      flag,         false, stale_residual},
    {"fused_prolong",        &suhmo_hier::fused_prolong,   1,      flag,         false, nullptr},
    {"merged_launches",      &suhmo_hier::merged_launches, 1,      flag,         false, nullptr},
    {"box_sweeps",           &suhmo_hier::box_sweeps,      4,      two_or_four,  false, nullptr},
    {"fused_relax",          &suhmo_hier::fused_relax,     1,      flag,         false, nullptr},
    {"shadow",               &suhmo_hier::shadowed,        0,      flag,         true,  nullptr},
    {"partition_min_cells",  &suhmo_hier::part_min_cells,  350000, at_least_one, true,  nullptr},
    {"track_old_volume",     &suhmo_hier::track_old_volume, 0,     flag,         false, nullptr},
};
static const HierOpt *find_opt(const char *key, size_t n)
{
    for (const HierOpt &o : hier_opts) if (strlen(o.key) == n && !strncmp(o.key, key, n)) return &o;
    return nullptr;
}
// "key=value,key=value" -> the options of H, the defaults for the keys it does not name
static int parse_opts(suhmo_hier *H, const char *opts)
{
    for (const HierOpt &o : hier_opts) H->*o.m = o.dflt;
    for (const char *p = opts ? opts : ""; *p;) {
        while (*p == ',' || *p == ' ') p++;
        if (!*p) break;
        const char *e = p + strcspn(p, ",=");
        const HierOpt *o = *e == '=' ? find_opt(p, e - p) : nullptr;
        if (!o) { suhmo_set_error("unknown hierarchy option '%.*s' in \"%s\"", (int)(e - p), p, opts); return -1; }
        H->*o->m = o->form(atol(e + 1));
        p = e + strcspn(e, ",");
    }
    return 0;
}
extern "C" int suhmo_hier_create_opts(suhmo_hier_t **out, const suhmo_level_desc_t *base, int nlev, const int *nbox, const int *boxes, const char *options)
{
    return suhmo_hier_create_on_(out, base, nullptr, nlev, nbox, boxes, options);
}
std::string suhmo_hier_options_(const suhmo_hier *H)
{
    std::string opts;
    for (const HierOpt &o : hier_opts) opts += std::string(o.key) + "=" + std::to_string(H->*o.m) + ",";
    return opts;
}
int suhmo_hier_check_(suhmo_hier *H) { return check_hier(H); }
int suhmo_hier_create_on_(suhmo_hier **out, const suhmo_level_desc_t *base, suhmo_level *adopt, int nlev, const int *nbox, const int *boxes, const char *options)
{
    ARG(out && base && nlev >= 1 && nlev <= 8);
    ARG(nlev == 1 || (nbox && boxes));
    ARG(base->i0 == 0 && (base->nx_global == 0 || base->nx_global == base->nx));
    const bool cut = !(base->j0 == 0 && base->ny == base->ny_global);
    if (cut && (base->ny_global % base->ny || base->j0 % base->ny)) { suhmo_set_error("hier: level 0 must be cut into EQUAL rank strips"); return -1; }
    suhmo_hier *H = new suhmo_hier();
    if (parse_opts(H, options)) { delete H; return -1; }
    if (cut) { H->world = base->ny_global / base->ny; H->rank = base->j0 / base->ny; H->shadowed = 1; }
    H->nlev = nlev; H->device = base->device; H->bc = base->bc; H->base_desc = *base; H->base_desc.boxes = nullptr; H->base_desc.nbox = 0;
    suhmo_level *B = adopt;
    H->base_borrowed = adopt != nullptr;
    int rc = adopt ? 0 : suhmo_level_create(&B, base);
    if (rc) { delete H; return rc; }
    B->zb_off = 1;                          // (a hierarchy's base keeps loading its bed elevation: suhmo_common.h)
    H->lev[0].l = 0; H->lev[0].nxd = base->nx; H->lev[0].nyd = base->ny_global; H->lev[0].box.push_back(B);
    H->vglob = B->d[0].v;
    if (H->shadowed) {
        DV &g = H->vglob;
        g.ny = g.nyg; g.j0 = 0; g.rows = g.ny + 2 * g.gy;
        g.ext[0] = g.ext[1] = g.rk[0] = g.rk[1] = 0;
    }
    {   // owner computes: the levels >= 1 are dealt to the ranks -- all of them or none -- when the largest holds at least partition_min_cells
        // cells per rank (per AMR cycle a level's ~26 passes shrink by (1 - 1/W) x 14 us per million cells each and ~28
        // collectives of ~30 us + 8 B x W x the packed cells / the link rate are added: even at ~2.6 M cells per level on 8 ranks)
        long most = 0;
        const int *qq = boxes;
        for (int l = 1; l < nlev; l++) {
            long cells = 0;
            for (int k = 0; k < nbox[l]; k++, qq += 4) cells += (long)(qq[2] - qq[0] + 1) * (qq[3] - qq[1] + 1);
            most = std::max(most, cells);
        }
        H->part = H->world > 1 && nlev > 1 && most >= H->part_min_cells * H->world;
    }
    const int *q = boxes;
    for (int l = 1; l < nlev; l++) {
        HLev &V = H->lev[l];
        V.l = l; V.nxd = H->lev[l - 1].nxd * 2; V.nyd = H->lev[l - 1].nyd * 2;
        if (nbox[l] < 1) { suhmo_set_error("hier: level %d has no box", l); suhmo_hier_destroy(H); return -1; }
        V.b4.assign(q, q + 4 * (size_t)nbox[l]);
        q += 4 * (size_t)nbox[l];
        for (int k = 0; k < nbox[l]; k++) {
            const int *b = &V.b4[4 * k];
            if ((b[0] & 1) || (b[1] & 1) || !(b[2] & 1) || !(b[3] & 1) || b[0] < 0 || b[1] < 0 || b[2] >= V.nxd || b[3] >= V.nyd || b[2] < b[0] || b[3] < b[1]) {
                suhmo_set_error("hier: box %d of level %d is not a coarse-aligned box of the refined domain", k, l); suhmo_hier_destroy(H); return -1; }
        }
        V.index.build(V.b4, V.nxd, V.nyd);
        for (int k = 0; k < nbox[l]; k++) {                  // disjoint: no two boxes that share a bucket intersect
            const int *b = &V.b4[4 * k];
            for (int by = b[1] / V.index.bs; by <= b[3] / V.index.bs; by++)
                for (int bx = b[0] / V.index.bs; bx <= b[2] / V.index.bs; bx++) {
                    const size_t qb = (size_t)by * V.index.nbx + bx;
                    for (int p = V.index.start[qb]; p < V.index.start[qb + 1]; p++) {
                        const int o = V.index.items[p];
                        const int *ob = &V.b4[4 * o];
                        if (o != k && std::max(b[0], ob[0]) <= std::min(b[2], ob[2]) && std::max(b[1], ob[1]) <= std::min(b[3], ob[3])) {
                            suhmo_set_error("hier: boxes of level %d overlap", l); suhmo_hier_destroy(H); return -1; }
                    }
                }
        }
        for (int k = 0; k < nbox[l]; k++) {
            const int *b = &V.b4[4 * k];
            suhmo_level_desc_t d = *base;
            d.nx = b[2] - b[0] + 1; d.ny = b[3] - b[1] + 1;
            d.i0 = b[0]; d.nx_global = V.nxd; d.j0 = b[1]; d.ny_global = V.nyd;
            d.dx = base->dx / (double)(1 << l); d.dy = base->dy / (double)(1 << l);
            d.nbox = 0; d.boxes = nullptr; d.max_box = std::max(d.nx, d.ny);
            d.halo_rows = 1; d.patch_j0 = 0; d.patch_ny = 0;
            suhmo_level *L = nullptr;
            rc = suhmo_level_create_(&L, &d, H->part);           // (owner computes: geometry first, storage once the plans say which boxes this rank holds)
            if (rc) { suhmo_hier_destroy(H); return rc; }
            L->gsrb_variant = 0; L->gsrb_tile = 0;               // in-place colour passes: the canvases of a box never move
            V.box.push_back(L);
        }
    }
    static const int need[] = {SUHMO_F_LPHI, SUHMO_F_GRADX, SUHMO_F_GRADY, SUHMO_F_RE, SUHMO_F_RHS0, SUHMO_F_PHIOLD, SUHMO_F_CORR};
    for (int l = 1; l < nlev; l++) if ((rc = part_setup(H, l))) { suhmo_hier_destroy(H); return rc; }
    for (int l = 1; l < nlev; l++) if ((rc = build_plans(H, l))) { suhmo_hier_destroy(H); return rc; }
    for (int l = 1; l < nlev && H->part; l++) {              // storage for the boxes this rank owns or mirrors; every other box stays a stub
        HLev &V = H->lev[l];
        for (size_t k = 0; k < V.box.size(); k++)
            if (V.held[k]) { V.held_boxes++; if ((rc = suhmo_level_materialize_(V.box[k]))) { suhmo_hier_destroy(H); return rc; } }
    }
    for (int l = 0; l < nlev; l++) for (int f : need) if ((rc = ensure_field(H, l, f))) { suhmo_hier_destroy(H); return rc; }
    for (int l = 1; l < nlev; l++) if ((rc = refresh_tables(H, l, nullptr))) { suhmo_hier_destroy(H); return rc; }
    // SUHMO_F_COVER: 1 under a finer level, 0 elsewhere
    for (int l = 0; l < nlev; l++) for (suhmo_level *L : H->lev[l].box) if (!L->stub && (rc = suhmo_level_set_value(L, 0, SUHMO_F_COVER, 0.0, nullptr))) { suhmo_hier_destroy(H); return rc; }
    for (int l = 1; l < nlev; l++) if ((rc = hier_avg(H, l, SUHMO_F_COVER, SUHMO_F_COVER, 1, 1.0, nullptr))) { suhmo_hier_destroy(H); return rc; }
    if (H->shadowed && nlev > 1 && (rc = cover_whole_base(H))) { suhmo_hier_destroy(H); return rc; }
    HIPCHK(hipDeviceSynchronize());
    *out = H;
    return 0;
}
// for the time step (suhmo_step.hip)
void suhmo_hier_invalidate_(suhmo_hier *H)
{
    H->phi_shadow_fresh = false;
    for (int l = 0; l < 8; l++) H->phi_ver[l]++;
    H->base_full_ver++;
    if (H->gap) suhmo_hier_invalidate_(H->gap);
}
// MAX over the ranks of a value every rank computed on the boxes it owns (through the all-reduce of the base strip)
int suhmo_hier_allreduce_max_(suhmo_hier *H, double *v)
{
    suhmo_level *B = H->lev[0].box[0];
    if (H->world <= 1) return 0;
    if (!B->ar) { suhmo_set_error("hier: the levels are partitioned over the ranks and level 0 has no all-reduce hook"); return -1; }
    return B->ar(B->user, v);
}
int suhmo_hier_allgather_(suhmo_hier *H, const double *send, long count, double *recv, hipStream_t st)
{
    if (!H->ag) { suhmo_set_error("hier: no all-gather is attached (suhmo_hier_attach_rccl / suhmo_hier_set_allgather)"); return -1; }
    H->part_gathers++;
    return H->ag(H->ag_user, send, count, recv, (suhmo_stream_t)st);
}
int suhmo_hier_gap_(suhmo_hier *H, const suhmo_model_params_t *mp, double dt, suhmo_hier **gap)
{
    if (H->gap && H->gap_dt != dt) {                       // a new time step size: beta = dt diffFactor of every operator; boxes, plans and tables stay
        for (int l = 0; l < H->nlev; l++)
            for (suhmo_level *L : H->gap->lev[l].box) { int rc = suhmo_level_set_alpha_beta(L, 1.0, dt * mp->diffFactor); if (rc) return rc; }
        HIPCHK(hipDeviceSynchronize());
        for (int l = 1; l < H->nlev; l++) {                // the device copies of the boxes' views carry beta: uploaded again at the next use
            HLev &V = H->gap->lev[l];
            if (V.d_dv) { (void)hipFree(V.d_dv); V.d_dv = nullptr; }
            if (V.d_red) { (void)hipFree(V.d_red); V.d_red = nullptr; }
            V.h_fp.clear();
        }
        H->gap->vglob.beta = H->gap->lev[0].box[0]->d[0].v.beta;
        H->gap_dt = dt;
    }
    if (!H->gap) {
        suhmo_level_desc_t d = H->base_desc;
        const suhmo_level *B = H->lev[0].box[0];
        d.boxes = B->boxes.data(); d.nbox = (int)(B->boxes.size() / 4);
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { d.bc.type[a][b] = 1; d.bc.value[a][b] = 0.0; }
        d.phys.use_NL = 0; d.alpha = 1.0; d.beta = dt * mp->diffFactor;
        std::vector<int> nbox(H->nlev, 0), flat;
        for (int l = 1; l < H->nlev; l++) { nbox[l] = (int)H->lev[l].box.size(); flat.insert(flat.end(), H->lev[l].b4.begin(), H->lev[l].b4.end()); }
        const std::string opts = suhmo_hier_options_(H);   // the parent's options as they are now
        int rc = suhmo_hier_create_opts(&H->gap, &d, H->nlev, nbox.data(), flat.data(), opts.c_str()); if (rc) return rc;
        H->gap_dt = dt;
        H->gap->ag = H->ag; H->gap->ag_user = H->ag_user;                                  // same strips, same ranks
        { suhmo_level *G0 = H->gap->lev[0].box[0]; suhmo_level_share_transport(G0, B);
          G0->ag = B->ag; G0->ag_user = B->ag_user; G0->agg_min_cells = B->agg_min_cells; if ((rc = suhmo_agg_setup(G0))) return rc; }
        for (int l = 0; l < H->nlev; l++)
            for (suhmo_level *L : H->gap->lev[l].box) if (!L->stub && (rc = suhmo_level_set_value(L, 0, SUHMO_F_ACOEF, 1.0, nullptr))) return rc;   // aCoeff_GH :1820-1828
    }
    {   // the bottom solver of the head solve's hierarchy
        const suhmo_level *B = base_of(H);
        suhmo_level *G0 = H->gap->lev[0].box[0];
        if (G0->bottom_solver != B->bottom_solver || G0->bottom_one_launch_max_cells != B->bottom_one_launch_max_cells) {
            int rc = suhmo_bottom_configure(G0, B->bottom_solver, B->bottom_one_launch_max_cells); if (rc) return rc;
        }
    }
    *gap = H->gap;
    return 0;
}

extern "C" int suhmo_hier_set_option(suhmo_hier_t *H, const char *key, long value)
{
    ARG(H && key);
    if (!strcmp(key, "bottom_solver") || !strcmp(key, "bottom_one_launch_max_cells")) {   // the bottom of every V-cycle is level 0's
        int rc = suhmo_level_set_option(base_of(H), key, value);
        if (rc == 0 && H->gap) rc = suhmo_hier_set_option(H->gap, key, value);
        return rc;
    }
    // suhmo_flatten.hip.  flatten_release (any value): the finest array and the scratch of suhmo_hier_flatten go back to the device now instead of
    // with the hierarchy; the next flatten allocates again.  flatten_fail_slot (tests; -1: off): see scratch() there.  Neither is inherited
    if (!strcmp(key, "flatten_release")) { HIPCHK(hipSetDevice(H->device)); HIPCHK(hipDeviceSynchronize()); suhmo_hier_flatten_release_(H); return 0; }
    if (!strcmp(key, "flatten_fail_slot")) { H->flat_fail_slot = value; return 0; }
    const HierOpt *o = find_opt(key, strlen(key));
    if (!o) { suhmo_set_error("unknown hierarchy option '%s'", key); return -1; }
    if (o->creation_only) { suhmo_set_error("hierarchy option '%s' is set when the hierarchy is created (suhmo_hier_create_opts)", key); return -1; }
    H->*o->m = o->form(value);
    if (o->reset) o->reset(H);
    return H->gap ? suhmo_hier_set_option(H->gap, key, value) : 0;
}
extern "C" int suhmo_hier_get_option(const suhmo_hier_t *H, const char *key, long *value)
{
    ARG(H && key && value);
    if (const HierOpt *o = find_opt(key, strlen(key))) { *value = H->*o->m; return 0; }
    if (!strncmp(key, "bottom_", 7)) {                    // bottom_solver, bottom_one_launch_max_cells, the bottom counters (with the gap solve's)
        int rc = suhmo_level_get_option(base_of(const_cast<suhmo_hier *>(H)), key, value);
        long g = 0;
        if (rc == 0 && H->gap && (!strcmp(key, "bottom_solver_iterations") || !strncmp(key, "bottom_solves_", 14))
            && (rc = suhmo_hier_get_option(H->gap, key, &g)) == 0) *value += g;
        return rc;
    }
    if (!strcmp(key, "ibc_launches")) { *value = H->n_ibc_launches; return 0; }
    if (!strcmp(key, "fused_relax_launches")) { *value = H->n_fused_relax + (H->gap ? H->gap->n_fused_relax : 0); return 0; }
    if (!strcmp(key, "gap_num_boxes")) {                  // boxes of the levels >= 1 of the gap-height hierarchy of the implicit step; -1: there is none (yet)
        *value = -1;
        if (H->gap) { *value = 0; for (int l = 1; l < H->gap->nlev; l++) *value += (long)H->gap->lev[l].box.size(); }
        return 0;
    }
    if (!strcmp(key, "recharge_launches")) { *value = H->n_recharge_launches; return 0; }
    if (!strcmp(key, "moulin_source_calls")) { *value = H->n_moulin_calls; return 0; }
    if (!strcmp(key, "run_readbacks")) { *value = H->n_run_readbacks; return 0; }
    if (!strcmp(key, "snapshot_launches")) { *value = H->n_snap_launches; return 0; }
    if (!strcmp(key, "snapshot_copies")) { *value = H->n_snap_copies; return 0; }
    if (!strcmp(key, "flatten_launches")) { *value = H->n_flat_launches; return 0; }
    if (!strcmp(key, "flatten_copies")) { *value = H->n_flat_copies; return 0; }
    if (!strcmp(key, "flatten_fail_slot")) { *value = H->flat_fail_slot; return 0; }
    if (!strcmp(key, "flatten_device_bytes")) {           // the finest array and the scratch of every level, level 0's included
        long c = (long)H->flat_cap * 8;
        for (int l = 0; l < H->nlev; l++) c += (long)H->lev[l].flat_slab.size() * (long)H->lev[l].flat_elems * 8;
        *value = c; return 0;
    }
    if (!strcmp(key, "compare_launches")) { *value = H->n_cmp_launches; return 0; }
    if (!strcmp(key, "compare_copies")) { *value = H->n_cmp_copies; return 0; }
    if (!strcmp(key, "compare_device_bytes")) { *value = (long)H->cmp_cap * 8; return 0; }
    if (!strcmp(key, "balance_launches")) { *value = H->n_bal_launches; return 0; }
    if (!strcmp(key, "balance_copies")) { *value = H->n_bal_copies; return 0; }
    if (!strcmp(key, "balance_device_bytes")) { *value = (long)H->bal_cap * 8; return 0; }
    if (!strcmp(key, "budget_launches")) { *value = H->n_wb_launches; return 0; }
    if (!strcmp(key, "budget_copies")) { *value = H->n_wb_copies; return 0; }
    if (!strcmp(key, "budget_device_bytes")) { *value = (long)(H->wb_cap + H->vol_cap) * 8; return 0; }
    if (!strcmp(key, "run_plots")) { *value = H->n_run_plots; return 0; }
    if (!strcmp(key, "run_checkpoints")) { *value = H->n_run_checkpoints; return 0; }
    if (!strcmp(key, "incremental_residual_passes")) { *value = H->n_incr_residual; return 0; }
    if (!strcmp(key, "residuals_left_by_relax")) { *value = H->n_fused_residual; return 0; }
    if (!strcmp(key, "sparse_gradient_passes")) { *value = H->n_sparse_grad; return 0; }
    if (!strcmp(key, "partition_gathers")) { *value = H->part_gathers + (H->gap ? H->gap->part_gathers : 0); return 0; }
    if (!strncmp(key, "partitioned_level_", 18) || !strncmp(key, "own_boxes_level_", 16)) {      // e.g. own_boxes_level_2: boxes of level 2 this rank relaxes
        const bool own = key[0] == 'o';
        const int l = atoi(key + (own ? 16 : 18));
        if (l < 0 || l >= H->nlev) { suhmo_set_error("no level %d", l); return -1; }
        const HLev &V = H->lev[l];
        *value = own ? V.n_owned() : (V.part ? 1 : 0);
        return 0;
    }
    if (!strcmp(key, "partition_bytes")) { *value = H->part_bytes + (H->gap ? H->gap->part_bytes : 0); return 0; }     // bytes this rank contributed to the partition's collectives
    {   // per level l >= 1: <key>_level_<l>
        static const char *keys[] = {"ghost_exchange_bytes_level_", "held_boxes_level_", "owned_cells_level_", "canvas_bytes_level_", "ghost_exchange_bound_bytes_level_"};
        for (int q = 0; q < 5; q++) {
            const size_t n = strlen(keys[q]);
            if (strncmp(key, keys[q], n)) continue;
            const int l = atoi(key + n);
            if (l < 1 || l >= H->nlev) { suhmo_set_error("no level %d", l); return -1; }
            const HLev &V = H->lev[l];
            if (q == 0) *value = H->side_bytes[l];                                   // what this rank sends per colour-pass exchange (the larger colour)
            else if (q == 1) *value = V.part ? V.held_boxes : (long)V.box.size();
            else if (q == 2) { long c = 0; if (V.part) c = V.owned_cells; else for (size_t k = 0; k < V.box.size(); k++) { const int *b = &V.b4[4 * k];
                c += (long)(b[2] - b[0] + 1) * (b[3] - b[1] + 1); } *value = c; }
            else if (q == 3) { long c = 0; for (suhmo_level *L : V.box) for (int f = 0; f < SUHMO_F_COUNT; f++) if (L->d[0].fp.f[f]) c += (long)L->d[0].elems * 8;
                               c += (long)V.flat_slab.size() * (long)V.flat_elems * 8; *value = c; }     // (with the scratch of suhmo_hier_flatten)
            // 4 sides x 8 B of the owned boxes
            else { long c = 0; for (int k = V.part ? V.b0 : 0; k < (V.part ? V.b0 + V.nown : 0); k++) { const int *b = &V.b4[4 * k];
                c += 8L * 2 * ((b[2] - b[0] + 1) + (b[3] - b[1] + 1)); } *value = c; }
            return 0;
        }
    }
    suhmo_set_error("unknown hierarchy option '%s'", key);
    return -1;
}
extern "C" int suhmo_hier_set_allgather(suhmo_hier_t *H, suhmo_hier_allgather_fn fn, void *user)
{
    ARG(H);
    H->ag = fn; H->ag_user = user;
    if (H->gap) { H->gap->ag = fn; H->gap->ag_user = user; }
    return 0;
}
int suhmo_rccl_allgather_hook(void *user, const double *send, long count, double *recv, suhmo_stream_t s);   // suhmo_rccl.hip; user = the level's Strip
extern "C" int suhmo_hier_attach_rccl(suhmo_hier_t *H)
{
    ARG(H);
    suhmo_level *B = base_of(H);
    if (!B->rccl) { suhmo_set_error("hier: attach the base strip first (suhmo_level_attach_rccl on suhmo_hier_box(H, 0, 0))"); return -1; }
    return suhmo_hier_set_allgather(H, suhmo_rccl_allgather_hook, B->rccl);
}
extern "C" long suhmo_hier_gathers(const suhmo_hier_t *H) { return H ? H->gathers + (H->gap ? H->gap->gathers : 0) : -1; }
extern "C" int suhmo_hier_num_levels(const suhmo_hier_t *H) { return H ? H->nlev : -1; }
extern "C" int suhmo_hier_num_boxes(const suhmo_hier_t *H, int l) { return (H && l >= 0 && l < H->nlev) ? (int)H->lev[l].box.size() : -1; }
extern "C" int suhmo_hier_get_boxes(const suhmo_hier_t *H, int l, int *boxes)
{
    ARG(H && l >= 1 && l < H->nlev && boxes);
    std::copy(H->lev[l].b4.begin(), H->lev[l].b4.end(), boxes);
    return 0;
}
extern "C" suhmo_level_t *suhmo_hier_box(suhmo_hier_t *H, int l, int k)
{
    if (!H || l < 0 || l >= H->nlev || k < 0 || k >= (int)H->lev[l].box.size()) return nullptr;
    return H->lev[l].box[k];
}
// which rank holds box k of level l: -1 = every rank (a replicated level, level 0's strip); `held`: this rank keeps storage for it (its own
// box, or a mirror of a neighbour's whose cells its plans read) -- a box that is neither is a stub: suhmo_level_set_field etc. refuse it
extern "C" int suhmo_hier_box_owner(const suhmo_hier_t *H, int l, int k, int *held)
{
    if (!H || l < 0 || l >= H->nlev || k < 0 || k >= (int)H->lev[l].box.size()) return -2;
    const HLev &V = H->lev[l];
    if (held) *held = V.part ? (int)V.held[k] : 1;
    return V.part ? V.owner[k] : -1;
}
extern "C" int suhmo_hier_exchange(suhmo_hier_t *H, int l, int field, int corners, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 0 && l < H->nlev && field >= 0 && field < SUHMO_F_COUNT);
    HIPCHK(hipSetDevice(H->device));
    if (field == SUHMO_F_MASK) for (suhmo_level *L : H->lev[l].box) suhmo_mask_written(L);      // (ghost cells of the mask are rewritten)
    if (field == SUHMO_F_ZB) for (suhmo_level *L : H->lev[l].box) suhmo_zb_written(L);
    return hier_ff(H, l, field, -1, corners != 0, HST(s));
}
extern "C" int suhmo_hier_cf_interp(suhmo_hier_t *H, int l, int field_f, int field_c, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 1 && l < H->nlev && field_f >= 0 && field_f < SUHMO_F_COUNT && field_c >= 0 && field_c < SUHMO_F_COUNT);
    HIPCHK(hipSetDevice(H->device));
    return hier_cf(H, l, field_f, field_c, HST(s));
}
extern "C" int suhmo_hier_pwl_fill(suhmo_hier_t *H, int l, int field_f, int field_c, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 1 && l < H->nlev && field_f >= 0 && field_f < SUHMO_F_COUNT && field_c >= 0 && field_c < SUHMO_F_COUNT);
    HIPCHK(hipSetDevice(H->device));
    return hier_pwl(H, l, field_f, field_c, HST(s));
}
extern "C" int suhmo_hier_average(suhmo_hier_t *H, int l, int field_f, int field_c, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 1 && l < H->nlev && field_f >= 0 && field_f < SUHMO_F_COUNT && field_c >= 0 && field_c < SUHMO_F_COUNT);
    HIPCHK(hipSetDevice(H->device));
    return hier_avg(H, l, field_f, field_c, 0, 0.0, HST(s));
}
extern "C" int suhmo_hier_gsrb(suhmo_hier_t *H, int l, int sweeps, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 0 && l < H->nlev && sweeps >= 0);
    HIPCHK(hipSetDevice(H->device));
    return hier_gsrb(H, l, sweeps, s);
}
extern "C" int suhmo_hier_update_operator(suhmo_hier_t *H, int l, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    ARG(l >= 0 && l < H->nlev);
    HIPCHK(hipSetDevice(H->device));
    if (l == 0) return suhmo_level_update_operator(base_of(H), 0, s);
    return hier_update_operator(H, l, s);
}
// composite residual of the hierarchy (RES of every level, covered cells zeroed) and its max norm (AMRNorm :1222-1264)
// the composite residual of all levels and its max norm over the cells no finer level covers (AMRResidual + AMRNorm)
static int hier_residual_(suhmo_hier *H, double *norm, suhmo_stream_t s)
{
    SUHMO_TIME("AMRNonLinearPoissonOp::AMRResidual");
    int rc;
    const int top = H->nlev - 1;
    if (levels_mergeable(H)) {
        // every level's ghosts, operator and reflux in one launch per kind; the covered cells are zeroed by the pass that takes the first stage
        // of the max norm; ONE launch over all partial maxima and one read-back (a maximum is the same in any order)
        if ((rc = levels_residual(H, top, 0, false, s))) return rc;
        if (!H->red_all) {
            size_t nb = 0;
            for (int l = 1; l <= top; l++) nb += H->lev[l].box.size();
            HIPCHK(hipMalloc(&H->red_all, (64 * nb + 16) * sizeof(double)));
        }
        const double *lists[2];
        int np[2];
        suhmo_lvboxes lv;
        // level 0: a large one is not read a second time for its cover -- its covered rectangles are zeroed by their list (one small launch), then the
        // plain first stage; a small one zeroes as it reduces, like the levels of boxes
        const bool large = base_of(H)->d[0].elems > (1 << 20);
        if (large && (rc = hier_avg(H, 1, SUHMO_F_RES, SUHMO_F_RES, 1, 0.0, HST(s)))) return rc;
        if ((rc = suhmo_level_norm_max_partials(base_of(H), SUHMO_F_RES, !large, &lists[0], &np[0], HST(s)))) return rc;
        if ((rc = levels_boxes(H, 1, top, 0, 1, s, lv)) || (rc = suhmo_levels_norm_max_cover_partials(lv, SUHMO_F_RES, H->red_all, &np[1], HST(s)))) return rc;
        lists[1] = H->red_all;
        return norm ? suhmo_norm_max_of_lists(base_of(H), lists, np, 2, norm, HST(s)) : 0;
    }
    if ((rc = cf_phi(H, top, s))) return rc;
    if ((rc = hier_level_residual(H, top, s))) return rc;                                  // AMRResidualNF on the finest level
    for (int l = top; l >= 1; l--) if ((rc = composite_residual(H, l, s, false))) return rc;
    for (int l = top; l >= 1; l--) if ((rc = hier_avg(H, l, SUHMO_F_RES, SUHMO_F_RES, 1, 0.0, HST(s)))) return rc;
    if (norm && H->merged_launches && !H->part && !dist_base(H)) {
        // one process holds everything: the first stages of every level's max norm, then ONE launch over their partial maxima and one read-back
        // (a maximum is the same in any order) instead of a reduction and a read-back per level
        const double *lists[8];
        int np[8];
        if ((rc = suhmo_level_norm_max_partials(base_of(H), SUHMO_F_RES, false, &lists[0], &np[0], HST(s)))) return rc;
        for (int l = 1; l <= top; l++) {
            suhmo_multi mv;
            if ((rc = multi_of(H, l, HST(s), mv)) || (rc = suhmo_multi_norm_max_partials(mv, SUHMO_F_RES, &lists[l], &np[l], HST(s)))) return rc;
        }
        return suhmo_norm_max_of_lists(base_of(H), lists, np, top + 1, norm, HST(s));
    }
    if (norm) {
        double m = 0.0;
        if ((rc = suhmo_level_norm(base_of(H), 0, SUHMO_F_RES, 0, &m, s))) return rc;
        double mp = 0.0;
        for (int l = 1; l <= top; l++) {
            double a = 0.0;
            const double *list;
            int n;
            suhmo_multi mv;
            if ((rc = multi_of(H, l, HST(s), mv))) return rc;
            if (mv.nbox <= 0) continue;                                 // a rank that owns no box of the level
            if ((rc = suhmo_multi_norm_max_partials(mv, SUHMO_F_RES, &list, &n, HST(s))) || (rc = suhmo_norm_max_of_lists(base_of(H), &list, &n, 1, &a, HST(s)))) return rc;
            if (a > mp) mp = a;
        }
        if (H->part && (rc = suhmo_hier_allreduce_max_(H, &mp))) return rc;     // owner computes: every rank saw its own boxes only
        if (mp > m) m = mp;
        *norm = m;
    }
    return 0;
}
extern "C" int suhmo_hier_residual(suhmo_hier_t *H, double *norm, suhmo_stream_t s)
{
    int rc = check_hier(H); if (rc) return rc;
    HIPCHK(hipSetDevice(H->device));
    return hier_residual_(H, norm, s);
}
extern "C" int suhmo_hier_vcycle(suhmo_hier_t *H, const suhmo_solver_params_t *sp, suhmo_stream_t s)
{
    SUHMO_TIME("AMRFASMultiGrid::VCycle(AMR)");
    int rc = check_hier(H); if (rc) return rc;
    ARG(sp);
    HIPCHK(hipSetDevice(H->device));
    return vcycle_amr(H, H->nlev - 1, sp, s);
}
extern "C" int suhmo_hier_solve(suhmo_hier_t *H, const suhmo_solver_params_t *sp, int *iters, double *hist, suhmo_stream_t s)
{
    SUHMO_TIME("AMRFASMultiGrid::solve(AMR)");
    ARG(sp);
    int rc;
    if (H && H->nlev == 1) return suhmo_level_solve(base_of(H), sp, iters, hist, s);
    // one invalidation at the entry (the caller may have loaded data); inside the loop every writer keeps the version counters, so
    // ghosts interpolated for the residual serve the cycle that follows, and the residual of level 0 is re-evaluated only where the
    // average from level 1 changed its head
    if ((rc = check_hier(H))) return rc;
    HIPCHK(hipSetDevice(H->device));
    rc = suhmo_solve_no_init(sp, iters, hist, [&](double *rnorm) { return hier_residual_(H, rnorm, s); },
                             [&] { SUHMO_TIME("AMRFASMultiGrid::VCycle(AMR)"); return vcycle_amr(H, H->nlev - 1, sp, s); });
    if (rc) return rc;
    // the domain sides of every ring as the solve's last residual evaluation leaves them in the oracle: the inhomogeneous boundary
    // condition (as suhmo_level_solve); the residual kernels evaluate it on the fly over the relaxation's homogeneous fill
    if ((rc = suhmo_level_fill_ghosts(base_of(H), 0, SUHMO_F_PHI, 0, s))) return rc;
    for (int l = 1; l < H->nlev; l++) {
        suhmo_multi m;
        if ((rc = multi_of(H, l, HST(s), m)) || (rc = launch_fill_ghosts(m.on(), SUHMO_F_PHI, 0, HST(s)))) return rc;
    }
    return 0;
}
