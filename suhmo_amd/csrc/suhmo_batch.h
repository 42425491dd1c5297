// suhmo_batch.h -- an ensemble of whole levels on one grid as one launch target (suhmo_batch.hip: tables, control flow; the batched
// __global__ wrappers live next to the device bodies they share with the solo kernels, in suhmo_gsrb.hip / suhmo_ops.hip / suhmo_bcoef.hip).
//
// A batched launch has gridDim.z = number of ACTIVE members; blockIdx.z picks, through the active list (a by-value kernel argument: no
// launch and no synchronisation to maintain it), a row of the per-depth device tables DV[n] / FP[n] / suhmo_phys_t[n].  The tile relaxation
// writes out of place and trades the two head canvases of a depth; members that leave the active list stop trading, so which canvas holds a
// member's head is a bit per member (`alt`) that travels with the table: the tables themselves are written once.
#pragma once
#include "suhmo_common.h"

constexpr int SUHMO_BATCH_MAX = 64;      // members of a batch (one bit each in BatchTab::alt)
struct BatchSel { int n; unsigned char m[SUHMO_BATCH_MAX]; };       // active list: blockIdx.z -> member
// one multigrid depth of every member.  fp[k].f[SUHMO_F_PHI] / f[SUHMO_F_PHI2]: the two head canvases of member k as they lay when the
// table was written; bit k of alt: they have traded places since (a whole level has no other use for SUHMO_F_PHI2)
struct BatchTab { const DV *dv; const FP *fp; const suhmo_phys_t *ph; unsigned long long alt; };

__device__ __forceinline__ int batch_member(const BatchSel &s) { return s.m[blockIdx.z]; }
__device__ __forceinline__ FP batch_fp(const BatchTab &t, int k)
{
    FP fp = t.fp[k];
    if ((t.alt >> k) & 1) { double *a = fp.f[SUHMO_F_PHI]; fp.f[SUHMO_F_PHI] = fp.f[SUHMO_F_PHI2]; fp.f[SUHMO_F_PHI2] = a; }
    return fp;
}

// ---- launchers; `v`: the view of any member at that depth (the members share the grid), has_alpha: the shared alpha != 0
// suhmo_gsrb.hip: S sweeps (x chunks) of the tile kernel, PHI -> PHI2 (the caller flips alt of the active members afterwards); coarse != NULL
// with prolong: phi += P(phi_c - phi_c,old) while loading; frhs: rhs = res + L(phi), LPHI, PHIOLD formed while loading
int suhmo_batch_gsrb_tile(const BatchTab &t, const BatchTab *coarse, const DV *vc, const BatchSel &sel, const DV &v, int S, int T, int chunks, bool frhs, bool prolong,
                          bool has_alpha, int order, hipStream_t st);
bool suhmo_batch_tile_ok(const DV &v);                    // the tile kernel can relax this depth (else colour passes)
int suhmo_batch_single_tile(const DV &v);                 // the depth is ONE tile of this edge (all its sweeps in one launch), or 0
int suhmo_batch_colour_pass(const BatchTab &t, const BatchSel &sel, const DV &v, int pass, bool has_alpha, hipStream_t st);
// suhmo_ops.hip
int suhmo_batch_fill_ghosts(const BatchTab &t, const BatchSel &sel, const DV &v, int field, int homog, hipStream_t st);
int suhmo_batch_restrict_both(const BatchTab &f, const BatchTab &c, const BatchSel &sel, const DV &vc, bool has_alpha, hipStream_t st);
int suhmo_batch_fas_coarse_rhs(const BatchTab &t, const BatchSel &sel, const DV &v, bool has_alpha, hipStream_t st);
int suhmo_batch_prolong(const BatchTab &f, const BatchTab &c, const BatchSel &sel, const DV &vf, const DV &vc, hipStream_t st);   // CORR_c, phi += P(CORR_c)
// RES = rhs - L(phi) of depth 0 and max |RES| of every active member: two launches, slot[k] <- the norm of member k, then the sequence number
// (partial: device scratch of n * workgroups doubles; slot / flag: device addresses of pinned host memory)
int suhmo_batch_residual_norm(const BatchTab &t, const BatchSel &sel, const DV &v, bool has_alpha, double *partial, double *slot,
                              unsigned long long *flag, unsigned long long seq, hipStream_t st);
size_t suhmo_batch_residual_partials(const DV &v);        // workgroups (= partial maxima) per member of that launch
// suhmo_bcoef.hip: UpdateOperator of depth 0 (the fused WFlx_level kernel) and AverageOperator of one coarse depth (ratio r)
int suhmo_batch_update_operator(const BatchTab &t, const BatchSel &sel, const DV &v, hipStream_t st);
int suhmo_batch_average_operator(const BatchTab &f, const BatchTab &c, const BatchSel &sel, const DV &vc, int r, hipStream_t st);
int suhmo_batch_avg_table(suhmo_level *const *mem, int n, void **dev);      // the members' coefficient / face canvases of all depths: rows written once
// AverageOperator of every depth > 0 (tabs[dep]: the tables of every depth) in one pass where the grid allows; *launches: how many it took
int suhmo_batch_average_operator_all(const BatchTab *tabs, const void *avg, const BatchSel &sel, const suhmo_level *L0, int nd, hipStream_t st, int *launches);
int suhmo_batch_build_mg_coefficients(const BatchTab &t0, const void *avg, const BatchSel &sel, const suhmo_level *L0, hipStream_t st, int *launches);
int suhmo_batch_copy_ghosts(const BatchTab &t, const BatchSel &sel, const DV &v, int field, hipStream_t st);      // exchange + CopyGhostCells
int suhmo_batch_grad_re(const BatchTab &t, const BatchSel &sel, const DV &v, hipStream_t st);                     // three launches
int suhmo_batch_bcoef_faces(const BatchTab &t, const BatchSel &sel, const DV &v, hipStream_t st);
int suhmo_batch_copy_canvas(const BatchTab &t, const BatchSel &sel, int fd, int fs, size_t elems, hipStream_t st);   // suhmo_ops.hip: a whole canvas, ghosts included

// ---- the time step (suhmo_step.hip: timestep_fas over the layout Batch, whose hooks use what follows from suhmo_batch.hip)
struct suhmo_batch;
struct BatchStep {                      // what a phase of the step launches over: the tables of depth 0, the members it serves, device rows of mp[n]
    BatchTab t; BatchSel sel; const DV *v; size_t elems; const suhmo_model_params_t *mp;
    double *partial, *slot; unsigned long long *flag, seq;     // reductions: scratch (2 x workgroups per member), pinned slots (2 per member), sequence number
};
int suhmo_batch_size_(const suhmo_batch *B);
bool suhmo_batch_step_select(suhmo_batch *B, const char *still);             // the members of the next phase: still[k] != 0, or everybody when none is
BatchStep suhmo_batch_step(suhmo_batch *B, bool reduction = false);         // (reduction: a new sequence number)
BatchSel suhmo_batch_step_subset(const suhmo_batch *B, const suhmo_model_params_t *mp_host, bool (*pick)(const suhmo_model_params_t &));
void suhmo_batch_count(suhmo_batch *B, int launches);
int suhmo_batch_step_mg_coefficients(suhmo_batch *B, hipStream_t st);
int suhmo_batch_step_solve(suhmo_batch *B, const suhmo_solver_params_t *sp, int *iters, hipStream_t st);   // SolveForHead_nl of the phase's members; iters[n]
int suhmo_batch_step_read(suhmo_batch *B, hipStream_t st, double *a, double *b);                          // the pinned slots of the phase's members -> a[k], b[k]
int suhmo_batch_step_begin(suhmo_batch *B, const suhmo_model_params_t *mp, hipStream_t st);   // tables against the handles, mp[n] on the device
// SolveForGap_nl of the members `sel` (all with use_impl_diff) on the gap batch, sp = gap_solver_params; mp: host rows of ALL members
int suhmo_batch_step_solve_gap(suhmo_batch *B, const BatchSel &sel, const suhmo_model_params_t *mp, double dt, const suhmo_solver_params_t *sp, hipStream_t st);
// suhmo_step.hip: b, RES, DCX, DCY of the members -> PHI, RHS, BX, BY of their gap handles (whole canvases) in one launch; and PHI of the gap
// handles -> b in one, cells without ice keeping their b where the member's freeze_icefree_gap is set (mpt: device rows of mp[n])
int suhmo_batch_gap_load(const BatchTab &h, const BatchTab &g, const BatchSel &sel, size_t elems, hipStream_t st);
int suhmo_batch_gap_store(const BatchTab &h, const BatchTab &g, const BatchSel &sel, const suhmo_model_params_t *mpt, size_t elems, hipStream_t st);
int suhmo_batch_timestep_run(suhmo_batch *B, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles, hipStream_t st);
