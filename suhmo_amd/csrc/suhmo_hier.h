// suhmo_hier.h -- every box of a level of a hierarchy of box unions as one launch target (OnBoxes, suhmo_target.h), and the launchers of
// suhmo_gsrb.hip / suhmo_ops.hip that cross translation units (the hierarchy itself: suhmo_hier_int.h)
#pragma once
#include "suhmo_target.h"
// every box of a level in ONE launch (blockIdx.z = box): device tables of the boxes' views and field pointers
constexpr int SUHMO_BOX_HALO = 8;    // cells around a box the plan `halo` of a level covers (k_gsrb_box_m advances through up to that many: 4 sweeps per launch)
struct suhmo_multi { const DV *dv; const FP *fp; int nbox, maxnx, maxny; double *red; /* reduction scratch, 64 nbox + 16 doubles */
                     int merged; /* hierarchy option merged_launches: gradient + its ghosts, Re + bCoef in one launch each */
                     const void *push; const int *pbase; /* fine-fine ghost cells a side cell feeds (int2 {box, offset}), first entry of every box */
                     suhmo_phys_t ph; /* the level's physics constants */
                     OnBoxes on() const { return OnBoxes{dv, fp, ph, nbox, maxnx, maxny}; } };
// suhmo_gsrb.hip: one colour pass over the rows [-lo, ny - 1 + hi] of a target; push / pbase (boxes only, or NULL): suhmo_multi's
template <class T> int launch_colour_pass(const T &t, bool has_alpha, int pass, int lo, int hi, const void *push, const int *pbase, hipStream_t st);
// suhmo_gsrb.hip: 2 sweeps per launch (bc_ghosts: + the closing homogeneous ghost fill)
int suhmo_multi_gsrb_box(const suhmo_multi &m, const suhmo_phys_t &ph, bool has_alpha, const void *halo, const int *hbase, int fsrc, int fdst, int npass,
    int bc_ghosts, hipStream_t st);
// suhmo_ops.hip: one launcher per operation, over any target it is launched over
template <class T> int launch_fill_ghosts(const T &t, int field, int homog, hipStream_t st);
template <class T> int launch_axby(const T &t, int fd, int fx, int fy, double a, double b, hipStream_t st);
template <class T> int launch_restrict(const T &f, const T &c, bool also_phi, bool has_alpha, hipStream_t st);      // RES (and PHI) of the coarse depth
template <class T> int launch_prolong(const T &f, const T &c, int lo, int hi, int lo_c, int hi_c, hipStream_t st);   // CORR_c, phi += P(CORR_c); halo rows covered
int launch_apply_boxes(const OnBoxes &t, bool has_alpha, int mode, hipStream_t st);                                   // mode 0: LPHI, 1: RES, 3: both
int suhmo_apply_and_residual(suhmo_level *L, int depth, hipStream_t st);                                                  // LPHI and RES = rhs - LPHI in one pass
int launch_fas_enter(const OnBoxes &t, hipStream_t st);   // RHS0 <- RHS, RHS <- RES + LPHI, PHIOLD <- PHI in one launch
int launch_fas_leave(const OnBoxes &t, hipStream_t st);   // RHS <- RHS0, CORR <- PHI - PHIOLD in one launch
int launch_copy(const OnBoxes &t, int fd, int fs, hipStream_t st);                                                        // valid cells + ghost ring
int launch_copy_between(const OnBoxes &dst, const OnBoxes &src, const int *fd, const int *fs, int n, hipStream_t st);   // same boxes, two hierarchies
int launch_extrap_ghosts(const OnBoxes &t, int field, hipStream_t st);                 // suhmo_step.hip: ExtrapGhostCells of a cell field
// suhmo_bcoef.hip
template <class T> int launch_grad_cc(const T &t, hipStream_t st);         // cell-centred gradient and its ghosts
template <class T> int launch_re(const T &t, hipStream_t st);              // COMPUTERE on the ghosted box
template <class T> int launch_bcoef_faces(const T &t, hipStream_t st);
template <class T> int launch_coef_ghosts(const T &t, int field, hipStream_t st);      // CopyGhostCells
template <class T> int launch_bcoef_fused(const T &t, bool wide, unsigned *flag, unsigned epoch, hipStream_t st, unsigned *small = nullptr, bool unmasked = false);   // UpdateOperator, the fused WFlx_level kernel
int suhmo_multi_grad_cc(const suhmo_multi &m, hipStream_t st);      // launch_grad_cc, or one launch when m.merged
int suhmo_multi_re_bcoef(const suhmo_multi &m, hipStream_t st);     // launch_re + launch_bcoef_faces, or one launch when m.merged
// max |field| over valid cells in pieces, for one read-back over a whole hierarchy: first stages (the partial maxima of level 0 -- cover: field <- 0
// where SUHMO_F_COVER is set, on the way -- and of a level of boxes, where they always lie), then one second stage over all lists (suhmo_reduce.h)
int suhmo_level_norm_max_partials(suhmo_level *L, int field, bool cover, const double **partials, int *np, hipStream_t st);
int suhmo_multi_norm_max_partials(const suhmo_multi &m, int field, const double **partials, int *np, hipStream_t st);
int suhmo_norm_max_of_lists(suhmo_level *slot, const double *const *partials, const int *np, int cnt, double *out, hipStream_t st);
// SEVERAL levels of boxes in one launch (blockIdx.z runs over the boxes of the listed levels, one after the other): by value, indexed with
// constants only (an unrolled search), so that the tables stay in scalar registers
constexpr int SUHMO_LVMAX = 7;
struct suhmo_lvboxes { const DV *dv[SUHMO_LVMAX]; const FP *fp[SUHMO_LVMAX]; int nbox[SUHMO_LVMAX], mode[SUHMO_LVMAX]; int n, maxnx, maxny; };
int suhmo_levels_apply(const suhmo_lvboxes &lv, const suhmo_phys_t &ph, bool has_alpha, hipStream_t st);   // mode[q]: 1 RES = rhs - L(phi), 3: LPHI as well (launch_apply_boxes)
// field <- 0 where SUHMO_F_COVER is set (mode[q] != 0), and the first stage of max |field| over the rest, of the listed levels; one partial per workgroup
int suhmo_levels_norm_max_cover_partials(const suhmo_lvboxes &lv, int field, double *partial, int *np, hipStream_t st);
int suhmo_levels_grad_cc(const suhmo_lvboxes &lv, int hasMask, hipStream_t st);                              // suhmo_multi_grad_cc (merged form) of several levels
