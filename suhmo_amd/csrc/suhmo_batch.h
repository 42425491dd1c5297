// suhmo_batch.h -- an ensemble of whole levels on one grid (suhmo_batch.hip: tables, control flow).  The members of a depth are the launch
// target OnMembers of suhmo_target.h; the kernels are the ones every other target launches, next to their device bodies.
#pragma once
#include "suhmo_hier.h"      // the launchers every target shares

// ---- launchers that only an ensemble has (the shared ones: suhmo_hier.h); has_alpha: the shared alpha != 0
// suhmo_gsrb.hip: S sweeps (x chunks) of the tile kernel, PHI -> PHI2 (the caller flips alt of the active members afterwards); coarse != NULL
// with prolong: phi += P(phi_c - phi_c,old) while loading; frhs: rhs = res + L(phi), LPHI, PHIOLD formed while loading
int suhmo_batch_gsrb_tile(const BatchTab &t, const BatchTab *coarse, const DV *vc, const BatchSel &sel, const DV &v, int S, int T, int chunks, bool frhs, bool prolong,
                          bool has_alpha, int order, hipStream_t st);
bool suhmo_batch_tile_ok(const DV &v);                    // the tile kernel can relax this depth (else colour passes)
// suhmo_bottom.hip: RelaxSolver::solve of the members' bottom depth, one workgroup per active member in ONE launch; ctr[k]: the device
// counters of member k (iterations, solves).  The depth must fit the LDS (suhmo_bottom_fits)
int suhmo_batch_relax_solve(const OnMembers &t, bool has_alpha, unsigned long long *const *ctr, hipStream_t st);
// suhmo_ops.hip
int launch_fas_coarse_rhs(const OnMembers &t, bool has_alpha, hipStream_t st);
// RES = rhs - L(phi) of depth 0 and max |RES| of every active member: two launches, slot[k] <- the norm of member k, then the sequence number
// (partial: device scratch of n * workgroups doubles; slot / flag: device addresses of pinned host memory)
int launch_residual_norm_members(const OnMembers &t, bool has_alpha, double *partial, double *slot, unsigned long long *flag, unsigned long long seq, hipStream_t st);
size_t suhmo_batch_residual_partials(const OnMembers &t);        // workgroups (= partial maxima) per member of that launch
int launch_copy_canvas(const OnMembers &t, int fd, int fs, size_t elems, hipStream_t st);   // a whole canvas, ghosts included
// suhmo_bcoef.hip
int suhmo_batch_avg_table(suhmo_level *const *mem, int n, void **dev);      // the members' coefficient / face canvases of all depths: rows written once
// AverageOperator of every depth > 0 (t[dep]: the members at every depth) in one pass where the grid allows; *launches: how many it took
int suhmo_batch_average_operator_all(const OnMembers *t, const void *avg, int nd, hipStream_t st, int *launches);
int suhmo_batch_build_mg_coefficients(const OnMembers &t0, const void *avg, const suhmo_level *L0, hipStream_t st, int *launches);

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
void suhmo_batch_step_faces_made(suhmo_batch *B);                           // the phase's members are about to have their face coefficients formed (suhmo_faces_made)
int suhmo_batch_step_mg_coefficients(suhmo_batch *B, hipStream_t st);
int suhmo_batch_step_solve(suhmo_batch *B, const suhmo_solver_params_t *sp, int *iters, hipStream_t st);   // SolveForHead_nl of the phase's members; iters[n]
int suhmo_batch_step_read(suhmo_batch *B, hipStream_t st, double *a, double *b);                          // the pinned slots of the phase's members -> a[k], b[k]
// tables against the handles, mp[n] on the device; serve[n] (NULL: everybody): the members this step is for
int suhmo_batch_step_begin(suhmo_batch *B, const suhmo_model_params_t *mp, hipStream_t st, const char *serve = nullptr);
// SolveForGap_nl of the members `sel` (all with use_impl_diff) on the gap batch, sp = gap_solver_params; mp: host rows of ALL members
int suhmo_batch_step_solve_gap(suhmo_batch *B, const BatchSel &sel, const suhmo_model_params_t *mp, double dt, const suhmo_solver_params_t *sp, hipStream_t st);
// suhmo_step.hip: b, RES, DCX, DCY of the members -> PHI, RHS, BX, BY of their gap handles (whole canvases) in one launch; and PHI of the gap
// handles -> b in one, cells without ice keeping their b where the member's freeze_icefree_gap is set (mpt: device rows of mp[n])
int suhmo_batch_gap_load(const OnMembers &h, const OnMembers &g, size_t elems, hipStream_t st);
int suhmo_batch_gap_store(const OnMembers &h, const OnMembers &g, size_t elems, hipStream_t st);      // h.mp: the members' device rows
// active[n] (NULL: everybody): the members the step is for (suhmo_batch_run; the others are in none of its launches, 0 iterations)
int suhmo_batch_timestep_run(suhmo_batch *B, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles, hipStream_t st,
                             const int *active = nullptr);

// ---- forcing and diagnostics of the members in one launch each: the device bodies of the per-level calls over OnMembers
// suhmo_forcing.hip
// COMPUTE_TIMEVARYINGRECHARGE of the members `t` serves: SUHMO_F_MSRC from the resident SUHMO_F_ZS, temperature and background input per member
int launch_time_varying_recharge(const OnMembers &t, const PerMember &TK, const PerMember &background, hipStream_t st);
// one moulin list on one view, what the three moulin kernels work on: a level, box or patch passes it by value, an ensemble keeps a device row per member
struct MoulinJob {
    DV v; int n, nblk;                 // the cells the Gaussians are sampled on; moulins; 16 x 16 tiles of v (= partial sums per moulin)
    const double *mo, *flux;           // {x, y, sigma} and the flux of every moulin
    double *integ, *partial;           // n integrals; nblk x n tile sums
    double tf; double *out;            // time factor; the source term (a canvas of v)
};
// the lists of the members in `sel` (rows[k]: member k's, on the device; nmax: the longest of them): three launches.  tf != NULL: the time
// factors of this launch, by value, instead of the rows' (a run writes the rows once and changes the factor every step)
int suhmo_batch_moulin_launch(const MoulinJob *rows, const BatchSel &sel, int nx, int ny, int nmax, hipStream_t st, const PerMember *tf = nullptr);
// suhmo_postproc.hip
// column sums of the SHMIP tables (suhmo_level_postproc_partial), out[k][8][nx] for every member k `t` serves; t.mp: the members' device rows
int launch_postproc_columns(const OnMembers &t, double *out, hipStream_t st);
// suhmo_postproc_temporal of those column sums on the device: out[k][6] for every member k `t` serves (one row of a run's series)
int launch_postproc_temporal_row(const OnMembers &t, const double *cols, double *out, hipStream_t st);
// suhmo_balance.hip
// the mass balance of the members `t` serves: one first stage into partial (suhmo_balance_member_doubles() per member of the batch), one final launch
// into out[k][SUHMO_MB_COUNT] for every member k served; suhmo_balance_check_member_: what member k must hold (rc -1, nothing launched)
size_t suhmo_balance_member_doubles();
int suhmo_balance_check_member_(const suhmo_level *L, int k);
int launch_mass_balance(const OnMembers &t, double *partial, double *out, hipStream_t st);
// the water budget of the members `t` serves (t.mp: the members' device rows): one first stage into partial (suhmo_budget_member_doubles() per member
// of the batch), one final launch into out[k][SUHMO_WB_COUNT] -- a DEVICE address -- for every member k served.  vol: the volume partials tracked
// steps kept (npo per member, launch_member_volumes; NULL: none), have: bit k = member k has some; VOLUME_OLD of the others is a quiet NaN
size_t suhmo_budget_member_doubles();
size_t suhmo_volume_member_doubles();
int suhmo_budget_check_member_(const suhmo_level *L, const suhmo_model_params_t *mp, int k, const char *who, bool faces, bool source);
int launch_member_volumes(const OnMembers &t, double *vol, int *np, hipStream_t st);
int launch_water_budget(const OnMembers &t, double *partial, const double *vol, int npo, unsigned long long have, double *out, hipStream_t st);
// suhmo_batch.hip: option track_old_volume is on, and then the first stage above for the members the step serves (suhmo_step.hip calls it behind
// suhmo_batch_step_begin)
int suhmo_batch_step_track_volume(suhmo_batch *B, hipStream_t st);
