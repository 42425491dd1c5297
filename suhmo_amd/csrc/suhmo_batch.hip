// suhmo_batch.hip -- an ensemble of N independent whole levels on ONE grid, stepped through one launch sequence.
//
// The reference's SHMIP suites are parameter sweeps on a 320 x 64 level (exec/A_SHMIP ... exec/F_SHMIP): 80 waves of tile work per
// member, on a part with 1024 SIMDs, and every launch costs its fixed few microseconds whatever its size.  A batch runs the FAS V-cycle of
// suhmo_fas.hip (operator methods src/VCAMRNonLinearPoissonOp.cpp:32-460, src/AMRNonLinearPoissonOp.cpp:707-886) and
// the solveNoInit loop with every kernel launched ONCE for all members that still have work (gridDim.z = active members, suhmo_batch.h),
// and one read-back per cycle that carries all their residual norms.  Each member sees exactly the sequence of operations it would see
// alone: the device bodies are the solo kernels', the stopping rule is SolveNoInit (suhmo_common.h) per member, and a member that has
// stopped is simply no longer in the active list of the launches that follow.
//
// Members are ordinary level handles owned by the batch (suhmo_batch_member): fields, BC values and physics constants are loaded and read
// through the suhmo_level_* entry points.  Tables are compared with the handles at the start of every batch call and written again only
// when a pointer, a view or a constant has changed.
//
// The implicit gap-height solve of the time step (option implicit_gap; SolveForGap_nl, src/AmrHydro.cpp:593-662, :3376-3455) runs on a second
// batch the first one owns: N handles with the linear operator of gap_level_prepare (suhmo_step.hip), their own tables, the same cycle and
// solve loop.  Its beta = dt x diffFactor is the member's own (the kernels read it from the member's row).
#include "suhmo_batch.h"
#include "suhmo_relax_plan.h"
#include "suhmo_ibc.h"
#include <algorithm>
#include <new>

struct suhmo_batch {
    int n, ndepth, device;
    bool has_alpha;
    std::vector<suhmo_level *> mem;
    DV *d_dv[SUHMO_MAXDEPTH];
    FP *d_fp[SUHMO_MAXDEPTH];
    suhmo_phys_t *d_ph;
    std::vector<DV> h_dv[SUHMO_MAXDEPTH];                   // what the device tables hold
    std::vector<FP> h_fp[SUHMO_MAXDEPTH];
    std::vector<suhmo_phys_t> h_ph;
    unsigned long long alt[SUHMO_MAXDEPTH];                 // bit k: the head canvases of member k have traded places since the table was written
    bool written;
    double *partial; size_t np;                             // partial maxima of the reductions: np workgroups per member, up to two values each
    double *hslot, *hslot_dev;                              // pinned: n values + the sequence number at [SUHMO_BATCH_MAX]
    unsigned long long hseq;
    int tile_order;
    long launches, readbacks, member_cycles;
    void *d_avg;                                            // the members' coefficient / face canvases of all depths (suhmo_bcoef.hip)
    suhmo_model_params_t *d_mp; std::vector<suhmo_model_params_t> h_mp;   // the time step: mp[n] on the device, rewritten when it changed
    BatchSel phase;                                         // the time step: the members the current phase serves
    BatchSel everyone;                                      // ... and the members the step is for (all of them, or the active ones of a run)
    bool beta_per_member;                                   // a gap batch: beta belongs to the member (alpha and everything that shapes a launch stay shared)
    int implicit_gap;                                       // option: members with use_impl_diff are stepped (default 0: refused)
    suhmo_batch *gap;                                       // the gap batch, created by the first step that needs it; its counters add to this one's
    std::vector<double> gap_beta;                           // beta its handle of member k holds
    // creation option bottom_solver (suhmo_batch_create_opts): RelaxSolver after the bottom relaxes of every cycle, one workgroup per member in one
    // launch (suhmo_bottom.hip).  Every member handle holds the same value; d_ctr[k]: the device counters of member k (its bottom_ctr)
    int bottom_solver; long bottom_max_cells;
    unsigned long long **d_ctr;
    // forcing and diagnostics of all members (suhmo_batch_moulin_source, suhmo_batch_postproc_*): scratch that grows on demand and goes with the batch
    double *d_moulin; size_t moulin_cap;                    // the members' rows (MoulinJob), their moulin tables, integrals and tile sums
    std::vector<double> h_moulin, h_integ;                  // what is sent to / read from it
    double *d_cols, *h_cols; size_t cols_cap;               // column sums [n][8][nx] on the device and in pinned host memory
    double *d_series, *h_series; size_t series_cap;         // the finished rows of a run [rows][n][6] (suhmo_batch_run), the same way
    double *d_bal, *h_bal;                                  // suhmo_batch_mass_balance: the members' partials and, behind them, their seven sums [n][7]; the sums in pinned memory
    // "WATER BUDGET": option track_old_volume; the volume partials the tracked steps kept (vol_np per member; bit k of vol_have: member k has some);
    // the members' partials of a budget and, behind them, their ten values [n][10], those in pinned memory too; the rows of a run's series
    int track_old_volume, vol_np;
    double *d_vol; unsigned long long vol_have;
    double *d_wb, *h_wb;
    double *d_wbs, *h_wbs; size_t wbs_cap;
};
constexpr int SLOT_FLAG = 2 * SUHMO_BATCH_MAX;             // pinned slot: two values per member, then the sequence number

static const DV &view(const suhmo_batch *B, int dep) { return B->mem[0]->d[dep].v; }
static BatchTab tab(const suhmo_batch *B, int dep) { return BatchTab{B->d_dv[dep], B->d_fp[dep], B->d_ph, B->alt[dep]}; }
static OnMembers on(const suhmo_batch *B, int dep, const BatchSel &sel) { return on_members(tab(B, dep), sel, view(B, dep)); }   // the members `sel` at a depth, as a launch target

// the device tables against the member handles: rows are rewritten when something other than the trade of the two head canvases changed
static int batch_sync(suhmo_batch *B, hipStream_t st)
{
    bool dirty = !B->written;
    for (int dep = 0; dep < B->ndepth; dep++) {
        unsigned long long alt = 0;
        for (int k = 0; k < B->n; k++) {
            Depth &D = B->mem[k]->d[dep];
            FP row = D.fp;
            row.f[SUHMO_F_PHI2] = D.phi_alt;
            FP &m = B->h_fp[dep][k];
            FP traded = m;
            std::swap(traded.f[SUHMO_F_PHI], traded.f[SUHMO_F_PHI2]);
            if (!memcmp(&row, &m, sizeof(FP))) { }
            else if (!memcmp(&row, &traded, sizeof(FP))) alt |= 1ull << k;
            else { m = row; dirty = true; }
            if (memcmp(&D.v, &B->h_dv[dep][k], sizeof(DV))) { B->h_dv[dep][k] = D.v; dirty = true; }
            // launch geometry and kernel variant are decided once for all members: what decides them must be shared (the BC VALUES are not)
            const DV &v0 = B->mem[0]->d[dep].v;
            if (memcmp(D.v.bct, v0.bct, sizeof(v0.bct)) || memcmp(D.v.per, v0.per, sizeof(v0.per)) || D.v.alpha != v0.alpha || (D.v.beta != v0.beta && !B->beta_per_member)) {
                suhmo_set_error("batch: member %d differs from member 0 in BC types, periodicity or alpha / beta: these are shared by all members", k);
                B->written = false;                          // (rows compared so far may be ahead of the device: the next call writes all)
                return -1;
            }
        }
        B->alt[dep] = alt;
    }
    for (int k = 0; k < B->n; k++)
        if (memcmp(&B->mem[k]->ph, &B->h_ph[k], sizeof(suhmo_phys_t))) { B->h_ph[k] = B->mem[k]->ph; dirty = true; }
    if (!dirty) return 0;
    HIPCHK(hipStreamSynchronize(st));                        // (no launch in flight reads the rows about to change)
    for (int dep = 0; dep < B->ndepth; dep++) {
        HIPCHK(hipMemcpy(B->d_dv[dep], B->h_dv[dep].data(), B->n * sizeof(DV), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(B->d_fp[dep], B->h_fp[dep].data(), B->n * sizeof(FP), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(B->d_ph, B->h_ph.data(), B->n * sizeof(suhmo_phys_t), hipMemcpyHostToDevice));
    B->written = true;
    return 0;
}
// the active members' head canvases of a depth have traded places (an out-of-place relaxation launch)
static void traded(suhmo_batch *B, int dep, const BatchSel &sel)
{
    for (int z = 0; z < sel.n; z++) {
        Depth &D = B->mem[sel.m[z]]->d[dep];
        std::swap(D.fp.f[SUHMO_F_PHI], D.phi_alt);
        B->alt[dep] ^= 1ull << sel.m[z];
    }
    suhmo_fp_changed();
}
static int batch_readback(suhmo_batch *B, hipStream_t st)
{
    B->readbacks++;
    volatile unsigned long long *flag = (volatile unsigned long long *)(B->hslot + SLOT_FLAG);
    for (long spin = 0; spin < 400000000L; spin++) {
        if (__atomic_load_n((unsigned long long *)flag, __ATOMIC_ACQUIRE) == B->hseq) return 0;
        if ((spin & 0xfff) == 0xfff && hipStreamQuery(st) != hipErrorNotReady) break;        // finished, or failed: the synchronisation below reports it
    }
    HIPCHK(hipStreamSynchronize(st));
    if (__atomic_load_n((unsigned long long *)flag, __ATOMIC_ACQUIRE) == B->hseq) return 0;
    suhmo_set_error("batch: the reduction's values did not arrive in the pinned slot");
    return -2;
}
// (suhmo_readback's mechanism -- a sequence number behind the values in pinned memory, polled -- with a slot per member: that one is tied to a
// level's two-value slot and its strip reductions)
// residualI of depth 0 of the active members and their max norms: hslot[k]
static int batch_residual_norms(suhmo_batch *B, const BatchSel &sel, hipStream_t st)
{
    int rc = launch_residual_norm_members(on(B, 0, sel), B->has_alpha, B->partial, B->hslot_dev,
                                          (unsigned long long *)(B->hslot_dev + SLOT_FLAG), ++B->hseq, st);
    if (rc) return rc;
    B->launches += 2;
    return batch_readback(B, st);
}

// relax() of the cycle (suhmo_fas.hip): tile launches of 4 / 2 / 1 sweeps where the grid allows (a depth that is one tile: all its sweeps in
// one launch), colour passes elsewhere; the relax that ends the cycle fills the ring with the homogeneous boundary condition
static int batch_relax(suhmo_batch *B, int dep, int sweeps, const BatchSel &sel, hipStream_t st, bool observable, bool frhs, bool prolong)
{
    const DV &v = view(B, dep);
    int rc;
    if (suhmo_batch_tile_ok(v)) {
        for (int it = 0; it < sweeps;) {
            const TileStep s = plan_tile_step(sweeps - it, 4, plan_single_tile(0, v.nx, v.ny), 16);
            const BatchTab c = prolong ? tab(B, dep + 1) : tab(B, dep);
            if ((rc = suhmo_batch_gsrb_tile(tab(B, dep), prolong ? &c : nullptr, prolong ? &view(B, dep + 1) : nullptr, sel, v, s.S, s.T, s.chunks,
                                            frhs, prolong, B->has_alpha, B->tile_order, st))) return rc;
            traded(B, dep, sel);
            B->launches++;
            frhs = prolong = false;
            it += s.S * s.chunks;
        }
    } else {
        if (frhs || prolong) { suhmo_set_error("internal: batch: a fused right-hand side / prolongation on a depth of colour passes"); return -4; }
        for (int p = 0; p < 2 * sweeps; p++) {
            if ((rc = launch_colour_pass(on(B, dep, sel), B->has_alpha, p & 1, 0, 0, nullptr, nullptr, st))) return rc;
            B->launches++;
        }
    }
    if (sweeps > 0 && observable) {
        if ((rc = launch_fill_ghosts(on(B, dep, sel), SUHMO_F_PHI, 1, st))) return rc;
        B->launches++;
    }
    return 0;
}
// the bottom depth `dep` of a batch with bottom_solver = 1 runs in the one launch (the only path a batch has): 0, or -5 and a message
static int batch_bottom_fits(const suhmo_batch *B, int dep)
{
    const DV &v = view(B, dep);
    const long cells = (long)v.nx * v.ny;
    if (cells <= 16384 && cells <= B->bottom_max_cells) return 0;
    suhmo_set_error("batch: bottom_solver = 1 with a bottom depth of %d x %d = %ld cells: a batch runs RelaxSolver in one launch only, on at most %ld cells "
                    "(16384, and bottom_one_launch_max_cells)", v.nx, v.ny, cells, std::min(16384L, B->bottom_max_cells));
    return -5;
}
// fas_cycle of suhmo_fas.hip for whole levels (no rank strips), `frhs`: this depth's first relaxation forms its FAS right-hand side
static int batch_fas_cycle(suhmo_batch *B, int dep, const suhmo_solver_params_t *sp, int nd, const BatchSel &sel, hipStream_t st, bool frhs)
{
    int rc;
    const int S = sp->num_smooth;
    if (dep == nd - 1) {
        if (!B->bottom_solver) return batch_relax(B, dep, sp->num_bottom, sel, st, dep == 0, frhs, false);   // bottom relaxes
        // bottom relaxes, then RelaxSolver of every active member in one launch; its loop ends on a residual evaluation, whose ghost fill is
        // the inhomogeneous one: that is what a depth-0 bottom leaves in the ghost ring
        if ((rc = batch_relax(B, dep, sp->num_bottom, sel, st, false, frhs, false))) return rc;
        if ((rc = suhmo_batch_relax_solve(on(B, dep, sel), B->has_alpha, B->d_ctr, st))) return rc;
        B->launches++;
        if (dep != 0) return 0;
        if ((rc = launch_fill_ghosts(on(B, 0, sel), SUHMO_F_PHI, 0, st))) return rc;
        B->launches++;
        return 0;
    }
    if ((rc = batch_relax(B, dep, S, sel, st, false, frhs, false))) return rc;                        // pre-smooth
    if ((rc = launch_restrict(on(B, dep, sel), on(B, dep + 1, sel), true, B->has_alpha, st))) return rc;   // RES, PHI of dep + 1
    B->launches++;
    const int next_sweeps = dep + 1 == nd - 1 ? sp->num_bottom : S;
    const bool rhs_in_relax = next_sweeps >= 1 && suhmo_batch_tile_ok(view(B, dep + 1));
    if (!rhs_in_relax) {                                                                                // PHIOLD = R phi, rhs_c = res_c + L_c(R phi)
        if ((rc = launch_fas_coarse_rhs(on(B, dep + 1, sel), B->has_alpha, st))) return rc;
        B->launches++;
    }
    if ((rc = batch_fas_cycle(B, dep + 1, sp, nd, sel, st, rhs_in_relax))) return rc;
    const bool prolong_in_relax = S >= 1 && suhmo_batch_tile_ok(view(B, dep));
    if (!prolong_in_relax) {                                                                            // corr = phi_c - phi_c,old; phi += P(corr)
        if ((rc = launch_prolong(on(B, dep, sel), on(B, dep + 1, sel), 0, 0, 0, 0, st))) return rc;
        B->launches += 2;
    }
    return batch_relax(B, dep, S, sel, st, dep == 0, false, prolong_in_relax);                          // post-smooth
}
static int batch_vcycle(suhmo_batch *B, const suhmo_solver_params_t *sp, const BatchSel &sel, hipStream_t st)
{
    int rc, nd = B->ndepth;
    if (sel.n <= 0) return 0;
    if (sp->max_depth >= 0 && sp->max_depth + 1 < nd) nd = sp->max_depth + 1;
    if (B->bottom_solver && (rc = batch_bottom_fits(B, nd - 1))) return rc;                             // (max_depth moves the bottom)
    if (sp->bcoeff_otf) {                                                                               // UpdateOperator, AverageOperator on every depth > 0
        if ((rc = launch_bcoef_fused(on(B, 0, sel), false, nullptr, 0u, st))) return rc;
        for (int z = 0; z < sel.n; z++) suhmo_faces_made(B->mem[sel.m[z]]);
        B->launches++;
        OnMembers tabs[SUHMO_MAXDEPTH];
        for (int dep = 0; dep < nd; dep++) tabs[dep] = on(B, dep, sel);
        int nl = 0;
        if ((rc = suhmo_batch_average_operator_all(tabs, B->d_avg, nd, st, &nl))) return rc;
        B->launches += nl;
    }
    if ((rc = batch_fas_cycle(B, 0, sp, nd, sel, st, false))) return rc;
    B->member_cycles += sel.n;
    return 0;
}
static BatchSel all_members(const suhmo_batch *B)
{
    BatchSel sel; memset(&sel, 0, sizeof(sel));
    sel.n = B->n;
    for (int k = 0; k < B->n; k++) sel.m[k] = (unsigned char)k;
    return sel;
}
// the members whose flag in active[n] is not 0 (NULL: all)
static BatchSel flagged_members(const suhmo_batch *B, const int *active)
{
    BatchSel sel = all_members(B);
    if (active) { sel.n = 0; for (int k = 0; k < B->n; k++) if (active[k]) sel.m[sel.n++] = (unsigned char)k; }
    return sel;
}
static int batch_enter(suhmo_batch *B, hipStream_t st)
{
    HIPCHK(hipSetDevice(B->device));
    for (int k = 0; k < B->n; k++)
        if (B->mem[k]->bottom_solver != B->bottom_solver) {
            suhmo_set_error("batch: bottom_solver = %d on member %d, %d on the batch: the option is fixed when the batch is created (suhmo_batch_create_opts) and "
                            "shared by all members", B->mem[k]->bottom_solver, k, B->bottom_solver);
            return -5;
        }
    return batch_sync(B, st);
}

extern "C" int suhmo_batch_destroy(suhmo_batch_t *B)
{
    if (!B) return 0;
    (void)hipSetDevice(B->device);
    (void)hipDeviceSynchronize();
    for (suhmo_level *L : B->mem) if (L) { L->batch_owned = 0; (void)suhmo_level_destroy(L); }
    for (int dep = 0; dep < SUHMO_MAXDEPTH; dep++) { if (B->d_dv[dep]) (void)hipFree(B->d_dv[dep]); if (B->d_fp[dep]) (void)hipFree(B->d_fp[dep]); }
    if (B->d_ph) (void)hipFree(B->d_ph);
    if (B->partial) (void)hipFree(B->partial);
    if (B->d_avg) (void)hipFree(B->d_avg);
    if (B->d_mp) (void)hipFree(B->d_mp);
    if (B->d_ctr) (void)hipFree(B->d_ctr);
    if (B->d_moulin) (void)hipFree(B->d_moulin);
    if (B->d_cols) (void)hipFree(B->d_cols);
    if (B->h_cols) (void)hipHostFree(B->h_cols);
    if (B->d_series) (void)hipFree(B->d_series);
    if (B->h_series) (void)hipHostFree(B->h_series);
    if (B->d_bal) (void)hipFree(B->d_bal);
    if (B->h_bal) (void)hipHostFree(B->h_bal);
    if (B->d_vol) (void)hipFree(B->d_vol);
    if (B->d_wb) (void)hipFree(B->d_wb);
    if (B->h_wb) (void)hipHostFree(B->h_wb);
    if (B->d_wbs) (void)hipFree(B->d_wbs);
    if (B->h_wbs) (void)hipHostFree(B->h_wbs);
    if (B->hslot) (void)hipHostFree(B->hslot);
    if (B->gap) (void)suhmo_batch_destroy(B->gap);
    delete B;
    return 0;
}
static int batch_create(suhmo_batch **out, const suhmo_level_desc_t *desc, int n_members, bool beta_per_member, int bottom_solver)
{
    *out = nullptr;
    if (n_members < 1 || n_members > SUHMO_BATCH_MAX) { suhmo_set_error("batch: n_members = %d, must be 1 .. %d", n_members, SUHMO_BATCH_MAX); return -1; }
    if (desc->j0 != 0 || desc->ny_global != desc->ny || desc->i0 != 0 || desc->nx_global != 0 || desc->patch_ny != 0 || desc->patch_j0 != 0) {
        suhmo_set_error("batch: members are whole levels (a rank strip or an AMR patch descriptor is refused: j0 / ny_global / i0 / nx_global / patch_*)");
        return -5;
    }
    if (desc->nx < 4 || desc->ny < 4) { suhmo_set_error("batch: members of at least 4 x 4 cells (the fused UpdateOperator kernel)"); return -5; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); suhmo_set_error("no HIP device: the product path has no CPU fallback"); return -3; }
    suhmo_batch *B = new (std::nothrow) suhmo_batch();
    if (!B) { suhmo_set_error("out of memory"); return -2; }
    B->n = n_members; B->device = desc->device; B->has_alpha = desc->alpha != 0.0; B->tile_order = 0;
    B->beta_per_member = beta_per_member; B->implicit_gap = 0; B->gap = nullptr;
    B->bottom_solver = bottom_solver; B->bottom_max_cells = 0; B->d_ctr = nullptr;
    auto fail = [&](int rc) { (void)suhmo_batch_destroy(B); return rc; };
    for (int k = 0; k < n_members; k++) {
        suhmo_level *L = nullptr;
        int rc = suhmo_level_create(&L, desc);
        if (rc) return fail(rc);                              // (no device: rc -3 with suhmo_level_create's message)
        L->batch_owned = 1; L->zb_off = 1;                    // (an ensemble's launches load every member's bed elevation)
        B->mem.push_back(L);
        if (k == 0) {                                         // (a bottom the one launch cannot take: refused before the other members are allocated)
            B->ndepth = L->ndepth; B->bottom_max_cells = L->bottom_one_launch_max_cells;
            if (bottom_solver && batch_bottom_fits(B, B->ndepth - 1)) return fail(-5);
        }
    }
    if (hipSetDevice(B->device) != hipSuccess) { suhmo_set_error("batch: hipSetDevice failed"); return fail(-2); }
    if (bottom_solver) {                                      // the members take the option (and their counters) as a level does; the rows of d_ctr never change
        std::vector<unsigned long long *> ctr;
        for (suhmo_level *L : B->mem) {
            int rc = suhmo_bottom_configure(L, 1, B->bottom_max_cells); if (rc) return fail(rc);
            ctr.push_back(L->bottom_ctr);
        }
        if (hipMalloc(&B->d_ctr, n_members * sizeof(unsigned long long *)) != hipSuccess
            || hipMemcpy(B->d_ctr, ctr.data(), n_members * sizeof(unsigned long long *), hipMemcpyHostToDevice) != hipSuccess) {
            suhmo_set_error("batch: hipMalloc failed"); return fail(-2);
        }
    }
    for (suhmo_level *L : B->mem)
        for (int dep = 0; dep < B->ndepth; dep++) {
            Depth &D = L->d[dep];
            for (int f : {SUHMO_F_LPHI, SUHMO_F_PHIOLD, SUHMO_F_CORR, SUHMO_F_RES})
                if (!suhmo_field(L, dep, f)) { suhmo_set_error("batch: field allocation failed"); return fail(-2); }
            if (!D.phi_alt) {
                if (hipMalloc(&D.phi_alt, D.elems * sizeof(double)) != hipSuccess || hipMemset(D.phi_alt, 0, D.elems * sizeof(double)) != hipSuccess) {
                    suhmo_set_error("batch: hipMalloc failed"); return fail(-2);
                }
            }
        }
    for (int dep = 0; dep < B->ndepth; dep++) {
        B->h_dv[dep].resize(n_members); B->h_fp[dep].resize(n_members);
        memset(B->h_dv[dep].data(), 0, n_members * sizeof(DV)); memset(B->h_fp[dep].data(), 0, n_members * sizeof(FP));
        if (hipMalloc(&B->d_dv[dep], n_members * sizeof(DV)) != hipSuccess || hipMalloc(&B->d_fp[dep], n_members * sizeof(FP)) != hipSuccess) {
            suhmo_set_error("batch: hipMalloc failed"); return fail(-2);
        }
    }
    B->h_ph.resize(n_members);
    memset(B->h_ph.data(), 0, n_members * sizeof(suhmo_phys_t));
    B->np = suhmo_batch_residual_partials(on_members(BatchTab{}, BatchSel{}, view(B, 0)));
    if (hipMalloc(&B->d_ph, n_members * sizeof(suhmo_phys_t)) != hipSuccess || hipMalloc(&B->partial, 2 * n_members * B->np * sizeof(double)) != hipSuccess
        || hipHostMalloc(&B->hslot, (SLOT_FLAG + 8) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess
        || hipHostGetDevicePointer((void **)&B->hslot_dev, B->hslot, 0) != hipSuccess) {
        suhmo_set_error("batch: allocation of the tables / the pinned slot failed"); return fail(-2);
    }
    memset(B->hslot, 0, (SLOT_FLAG + 8) * sizeof(double));
    B->h_mp.resize(n_members);
    memset(B->h_mp.data(), 0xff, n_members * sizeof(suhmo_model_params_t));
    if (hipMalloc(&B->d_mp, n_members * sizeof(suhmo_model_params_t)) != hipSuccess) { suhmo_set_error("batch: hipMalloc failed"); return fail(-2); }
    { int rc = suhmo_batch_avg_table(B->mem.data(), n_members, &B->d_avg); if (rc) return fail(rc); }
    B->phase = B->everyone = all_members(B);
    *out = B;
    return 0;
}
// "key=value,key=value": the creation options (bottom_solver), the defaults for the keys it does not name
extern "C" int suhmo_batch_create_opts(suhmo_batch_t **out, const suhmo_level_desc_t *desc, int n_members, const char *options)
{
    ARG(out && desc);
    int bottom_solver = 0;
    for (const char *p = options ? options : ""; *p;) {
        while (*p == ',' || *p == ' ') p++;
        if (!*p) break;
        const char *e = p + strcspn(p, ",=");
        if (*e != '=' || e - p != 13 || strncmp(p, "bottom_solver", 13)) { suhmo_set_error("unknown batch option '%.*s' in \"%s\"", (int)(e - p), p, options); return -1; }
        const long v = atol(e + 1);
        if (v != 0 && v != 1) { suhmo_set_error("batch: bottom_solver: 0 (bottom relaxes only) or 1 (RelaxSolver)"); return -1; }
        bottom_solver = (int)v;
        p = e + strcspn(e, ",");
    }
    return batch_create(out, desc, n_members, false, bottom_solver);
}
extern "C" int suhmo_batch_create(suhmo_batch_t **out, const suhmo_level_desc_t *desc, int n_members) { return suhmo_batch_create_opts(out, desc, n_members, nullptr); }
extern "C" int suhmo_batch_size(const suhmo_batch_t *B) { return B ? B->n : 0; }
extern "C" suhmo_level_t *suhmo_batch_member(suhmo_batch_t *B, int k)
{
    if (!B || k < 0 || k >= B->n) { suhmo_set_error("batch: no member %d", k); return nullptr; }
    return B->mem[k];
}

extern "C" int suhmo_batch_set_phys(suhmo_batch_t *B, int k, const suhmo_phys_t *phys)
{
    ARG(B && phys && k >= 0 && k < B->n);
    suhmo_level *L = B->mem[k];
    L->ph = *phys; L->desc.phys = *phys;
    suhmo_level_drop_graphs(L);                               // (captured launches of the member's own V-cycles carry the constants by value)
    return 0;
}

extern "C" int suhmo_batch_vcycle(suhmo_batch_t *B, const suhmo_solver_params_t *sp, const int *active, suhmo_stream_t s)
{
    SUHMO_TIME("AMRFASMultiGrid::VCycle");
    ARG(B && sp);
    int rc = batch_enter(B, (hipStream_t)s); if (rc) return rc;
    const BatchSel sel = flagged_members(B, active);
    return batch_vcycle(B, sp, sel, (hipStream_t)s);          // (no member selected: nothing to do)
}
// the AMRMultiGrid::solve loop of the members in `first`, each with its own stopping rule; iters / residual: arrays over ALL members
static int batch_solve(suhmo_batch *B, const suhmo_solver_params_t *sp, const BatchSel &first, int *iters, double *residual, hipStream_t st)
{
    int rc;
    if (first.n <= 0) return 0;
    std::vector<SolveNoInit> state(B->n);
    std::vector<char> in(B->n, 0);
    if ((rc = batch_residual_norms(B, first, st))) return rc;
    for (int z = 0; z < first.n; z++) { in[first.m[z]] = 1; state[first.m[z]].start(B->hslot[first.m[z]]); }
    for (;;) {
        BatchSel sel; memset(&sel, 0, sizeof(sel));
        for (int k = 0; k < B->n; k++) if (in[k] && state[k].go(sp)) sel.m[sel.n++] = (unsigned char)k;
        if (!sel.n) break;
        if ((rc = batch_vcycle(B, sp, sel, st)) || (rc = batch_residual_norms(B, sel, st))) return rc;
        for (int z = 0; z < sel.n; z++) state[sel.m[z]].cycled(B->hslot[sel.m[z]]);
    }
    for (int k = 0; k < B->n; k++) if (in[k]) { if (iters) iters[k] = state[k].iter; if (residual) residual[k] = state[k].rnorm; }
    // the ring as the solve of a level leaves it (suhmo_level_solve): the inhomogeneous fill of the final residual evaluation
    if ((rc = launch_fill_ghosts(on(B, 0, first), SUHMO_F_PHI, 0, st))) return rc;
    B->launches++;
    return 0;
}
extern "C" int suhmo_batch_solve(suhmo_batch_t *B, const suhmo_solver_params_t *sp, int *iters, double *residual, suhmo_stream_t s)
{
    SUHMO_TIME("AMRFASMultiGrid::solve");
    ARG(B && sp);
    int rc = batch_enter(B, (hipStream_t)s); if (rc) return rc;
    return batch_solve(B, sp, all_members(B), iters, residual, (hipStream_t)s);
}

// ---- the time step: timestep_fas over the layout Batch (suhmo_step.hip), whose hooks reach the batch through these
int suhmo_batch_size_(const suhmo_batch *B) { return B->n; }
void suhmo_batch_step_faces_made(suhmo_batch *B) { for (int z = 0; z < B->phase.n; z++) suhmo_faces_made(B->mem[B->phase.m[z]]); }
void suhmo_batch_count(suhmo_batch *B, int launches) { B->launches += launches; }
bool suhmo_batch_step_select(suhmo_batch *B, const char *still)
{
    BatchSel sel; memset(&sel, 0, sizeof(sel));
    for (int k = 0; k < B->n; k++) if (still[k]) sel.m[sel.n++] = (unsigned char)k;
    B->phase = sel.n ? sel : B->everyone;
    return sel.n > 0;
}
BatchStep suhmo_batch_step(suhmo_batch *B, bool reduction)
{
    if (reduction) ++B->hseq;
    return BatchStep{tab(B, 0), B->phase, &view(B, 0), B->mem[0]->d[0].elems, B->d_mp, B->partial, B->hslot_dev,
                     (unsigned long long *)(B->hslot_dev + SLOT_FLAG), B->hseq};
}
BatchSel suhmo_batch_step_subset(const suhmo_batch *B, const suhmo_model_params_t *mp_host, bool (*pick)(const suhmo_model_params_t &))
{
    BatchSel sel; memset(&sel, 0, sizeof(sel));
    for (int z = 0; z < B->phase.n; z++) if (pick(mp_host[B->phase.m[z]])) sel.m[sel.n++] = B->phase.m[z];
    return sel;
}
int suhmo_batch_step_mg_coefficients(suhmo_batch *B, hipStream_t st)
{
    int nl = 0;
    int rc = suhmo_batch_build_mg_coefficients(on(B, 0, B->phase), B->d_avg, B->mem[0], st, &nl);
    B->launches += nl;
    for (suhmo_level *L : B->mem) L->coarse_mask_ok = 1;
    return rc;
}
int suhmo_batch_step_solve(suhmo_batch *B, const suhmo_solver_params_t *sp, int *iters, hipStream_t st) { return batch_solve(B, sp, B->phase, iters, nullptr, st); }
int suhmo_batch_step_read(suhmo_batch *B, hipStream_t st, double *a, double *b)
{
    int rc = batch_readback(B, st); if (rc) return rc;
    for (int z = 0; z < B->phase.n; z++) { const int k = B->phase.m[z]; a[k] = B->hslot[2 * k]; b[k] = B->hslot[2 * k + 1]; }
    return 0;
}
// ---- SolveForGap_nl of a batch: solve_gap_implicit (suhmo_step.hip) of every member in `sel`, one launch sequence
// the gap batch with beta = dt diffFactor of every member in its handles.  Created once: the descriptor of gap_level_prepare, aCoef = 1 on
// depth 0 and MGnewOp's cell averages of every coarse depth (aCoef = 1 there too; they never change, so they are not built again per step)
static int gap_batch_prepare(suhmo_batch *B, const suhmo_model_params_t *mp, double dt, hipStream_t st)
{
    int rc;
    const bool fresh = !B->gap;
    if (fresh) {
        suhmo_level *L0 = B->mem[0];
        suhmo_level_desc_t d = L0->desc;
        d.boxes = L0->boxes.data(); d.nbox = (int)(L0->boxes.size() / 4);
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { d.bc.type[a][b] = 1; d.bc.value[a][b] = 0.0; }
        d.phys.use_NL = 0; d.alpha = 1.0; d.beta = dt * mp[0].diffFactor;
        suhmo_batch *G = nullptr;
        if ((rc = batch_create(&G, &d, B->n, true, B->bottom_solver))) return rc;                      // (the same bottom solver: gap_level_prepare)
        B->gap = G;
        B->gap_beta.assign(B->n, d.beta);
        for (suhmo_level *L : G->mem)
            if ((rc = suhmo_level_set_value(L, 0, SUHMO_F_ACOEF, 1.0, (suhmo_stream_t)st))) return rc;      // aCoeff_GH :1820-1828
    }
    suhmo_batch *G = B->gap;
    for (int k = 0; k < B->n; k++) {                        // a new dt or diffFactor: only beta changes (the tables follow in batch_sync)
        const double beta = dt * mp[k].diffFactor;
        if (beta == B->gap_beta[k]) continue;
        if ((rc = suhmo_level_set_alpha_beta(G->mem[k], 1.0, beta))) return rc;
        B->gap_beta[k] = beta;
    }
    G->tile_order = B->tile_order;
    if ((rc = batch_enter(G, st)) || !fresh) return rc;
    int nl = 0;
    rc = suhmo_batch_build_mg_coefficients(on(G, 0, all_members(G)), G->d_avg, G->mem[0], st, &nl);
    G->launches += nl;
    return rc;
}
int suhmo_batch_step_solve_gap(suhmo_batch *B, const BatchSel &sel, const suhmo_model_params_t *mp, double dt, const suhmo_solver_params_t *sp, hipStream_t st)
{
    int rc, nl = 0;
    if (sel.n <= 0) return 0;
    if (sp->bcoeff_otf) { suhmo_set_error("internal: batch: the gap-height solve keeps its coefficients (bcoeff_otf = 0)"); return -4; }
    if ((rc = gap_batch_prepare(B, mp, dt, st))) return rc;
    suhmo_batch *G = B->gap;
    const size_t elems = B->mem[0]->d[0].elems;
    if (G->mem[0]->d[0].elems != elems) { suhmo_set_error("internal: batch: gap level geometry"); return -4; }
    if ((rc = suhmo_batch_gap_load(on(B, 0, sel), on(G, 0, sel), elems, st))) return rc;                   // initial guess = b :3382-3385, RHS, D on the faces
    G->launches++;
    OnMembers tabs[SUHMO_MAXDEPTH];
    for (int dep = 0; dep < G->ndepth; dep++) tabs[dep] = on(G, dep, sel);
    if ((rc = suhmo_batch_average_operator_all(tabs, G->d_avg, G->ndepth, st, &nl))) return rc;     // coarse D = average of the fine faces
    G->launches += nl;
    if ((rc = batch_solve(G, sp, sel, nullptr, nullptr, st))) return rc;
    if ((rc = suhmo_batch_gap_store(on_members(tab(B, 0), sel, view(B, 0), B->d_mp), on(G, 0, sel), elems, st))) return rc;         // (tab(G, 0) after the solve: the canvases have traded)
    G->launches++;
    return 0;
}
// mp[n] on the device: rewritten when a row changed
static int batch_mp_sync(suhmo_batch *B, const suhmo_model_params_t *mp, hipStream_t st)
{
    if (!memcmp(B->h_mp.data(), mp, B->n * sizeof(suhmo_model_params_t))) return 0;
    HIPCHK(hipStreamSynchronize(st));                        // (no launch in flight reads the rows about to change)
    memcpy(B->h_mp.data(), mp, B->n * sizeof(suhmo_model_params_t));
    HIPCHK(hipMemcpy(B->d_mp, B->h_mp.data(), B->n * sizeof(suhmo_model_params_t), hipMemcpyHostToDevice));
    return 0;
}
// the step's entry: tables against the handles (the step's fields have just been allocated), mp[n] on the device, everybody in the first phase
int suhmo_batch_step_begin(suhmo_batch *B, const suhmo_model_params_t *mp, hipStream_t st, const char *serve)
{
    int rc = batch_enter(B, st); if (rc) return rc;
    if ((rc = batch_mp_sync(B, mp, st))) return rc;
    B->everyone = all_members(B);
    if (serve) { B->everyone.n = 0; for (int k = 0; k < B->n; k++) if (serve[k]) B->everyone.m[B->everyone.n++] = (unsigned char)k; }
    B->phase = B->everyone;
    return 0;
}
// "WATER BUDGET", option track_old_volume: the volume the step starts from, of the members it serves; the others keep what they had
int suhmo_batch_step_track_volume(suhmo_batch *B, hipStream_t st)
{
    if (!B->track_old_volume || B->everyone.n <= 0) return 0;
    for (int z = 0; z < B->everyone.n; z++) {
        const FP &fp = B->mem[B->everyone.m[z]]->d[0].fp;
        if (!fp.f[SUHMO_F_MASK] || !fp.f[SUHMO_F_B]) { suhmo_set_error("batch: track_old_volume: member %d holds no ice mask or no gap height", (int)B->everyone.m[z]); return -1; }
    }
    if (!B->d_vol && hipMalloc(&B->d_vol, B->n * suhmo_volume_member_doubles() * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError(); B->d_vol = nullptr; suhmo_set_error("batch: the volume partials cannot be allocated"); return -2;
    }
    int np = 0, rc = launch_member_volumes(on(B, 0, B->everyone), B->d_vol, &np, st);
    if (rc) return rc;
    B->launches++;
    B->vol_np = np;
    for (int z = 0; z < B->everyone.n; z++) B->vol_have |= 1ull << B->everyone.m[z];
    return 0;
}
extern "C" int suhmo_batch_timestep(suhmo_batch_t *B, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles,
                                    suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::timeStepFAS");
    ARG(B && mp);
    for (int k = 0; k < B->n && !B->implicit_gap; k++)
        if (mp[k].use_impl_diff) {
            suhmo_set_error("batch: use_impl_diff = 1 (member %d): the implicit gap-height solve of a batch is not built (into a step, unless batch option implicit_gap is set to 1)", k);
            return -5;
        }
    HIPCHK(hipSetDevice(B->device));
    return suhmo_batch_timestep_run(B, mp, dt, cur_step, picard_iters, vcycles, (hipStream_t)s);
}

// ---- forcing and diagnostics of all members: what suhmo_level_time_varying_recharge, suhmo_level_moulin_source and suhmo_level_postproc_* do on
// a member handle, for the members whose flag in active[n] is not 0, in the launches of ONE member.  Everything is checked on every such member
// before anything is launched; the source field is allocated like a member's first per-level call does, and the tables follow (batch_enter)
static int batch_source_fields(suhmo_batch *B, const BatchSel &sel, hipStream_t st)
{
    HIPCHK(hipSetDevice(B->device));
    for (int z = 0; z < sel.n; z++)
        if (!suhmo_field(B->mem[sel.m[z]], 0, SUHMO_F_MSRC)) { suhmo_set_error("batch: field allocation failed (member %d)", sel.m[z]); return -2; }
    return batch_enter(B, st);
}
extern "C" int suhmo_batch_time_varying_recharge(suhmo_batch_t *B, const double *T_K, const double *background, const int *active, suhmo_stream_t s)
{
    ARG(B && T_K && background);
    hipStream_t st = (hipStream_t)s;
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    for (int z = 0; z < sel.n; z++)
        if (!B->mem[sel.m[z]]->d[0].fp.f[SUHMO_F_ZS]) {
            suhmo_set_error("batch: time-varying recharge: load the ice surface height (SUHMO_F_ZS) of member %d first", sel.m[z]);
            return -1;
        }
    int rc = batch_source_fields(B, sel, st); if (rc) return rc;
    PerMember tk, bg;
    memset(&tk, 0, sizeof(tk)); memset(&bg, 0, sizeof(bg));
    for (int k = 0; k < B->n; k++) { tk.x[k] = T_K[k]; bg.x[k] = background[k]; }
    if ((rc = launch_time_varying_recharge(on(B, 0, sel), tk, bg, st))) return rc;
    B->launches++;
    return 0;
}
// suhmo_level_ibc_init of the flagged members in one launch (+ the two CopyGhostCells launches): include/suhmo_hip.h, "INITIAL CONDITIONS".  The
// members' parameter rows live on the device for the length of the call
extern "C" int suhmo_batch_ibc_init(suhmo_batch_t *B, const suhmo_ibc_t *ibcs, const int *active, suhmo_stream_t s)
{
    if (!B) { suhmo_set_error("suhmo_batch_ibc_init: no batch"); return -1; }
    if (!ibcs) { suhmo_set_error("suhmo_batch_ibc_init: no suhmo_ibc_t given"); return -1; }
    hipStream_t st = (hipStream_t)s;
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    int rc;
    for (int z = 0; z < sel.n; z++) {
        if ((rc = suhmo_ibc_check_(&ibcs[sel.m[z]], "suhmo_batch_ibc_init"))) return rc;
        if (ibcs[sel.m[z]].kind != ibcs[sel.m[0]].kind) {
            suhmo_set_error("suhmo_batch_ibc_init: member %d has kind %d, member %d kind %d: the members of one call share the kind", sel.m[z], ibcs[sel.m[z]].kind,
                            sel.m[0], ibcs[sel.m[0]].kind);
            return -1;
        }
    }
    HIPCHK(hipSetDevice(B->device));
    static const int fields[] = {SUHMO_F_ZB, SUHMO_F_ZS, SUHMO_F_PI, SUHMO_F_B, SUHMO_F_PW, SUHMO_F_PHI, SUHMO_F_MR, SUHMO_F_ACOEF, SUHMO_F_MASK};
    for (int z = 0; z < sel.n; z++)
        for (int f : fields)
            if (!suhmo_field(B->mem[sel.m[z]], 0, f)) { suhmo_set_error("batch: field allocation failed (member %d)", sel.m[z]); return -2; }
    if ((rc = batch_enter(B, st))) return rc;
    std::vector<IbcRow> rows(B->n);
    for (int z = 0; z < sel.n; z++) rows[sel.m[z]] = ibc_row(ibcs[sel.m[z]]);
    IbcRow *d_rows = nullptr;
    HIPCHK(hipMalloc(&d_rows, rows.size() * sizeof(IbcRow)));
    hipError_t e = hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(IbcRow), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        int launched = 0;
        rc = launch_ibc_init(on(B, 0, sel), d_rows, st, &launched);
        B->launches += launched;
        e = hipStreamSynchronize(st);                        // (the rows are read by the launch in flight)
    }
    (void)hipFree(d_rows);
    if (e != hipSuccess) { suhmo_set_error("suhmo_batch_ibc_init: %s", hipGetErrorString(e)); return -2; }
    for (int z = 0; z < sel.n && !rc; z++) {
        suhmo_level *L = B->mem[sel.m[z]];
        L->d[0].phi_fresh = 0; suhmo_mask_written(L); suhmo_zb_written(L);
    }
    return rc;
}
// member k's moulins are entries off[k] .. off[k] + n_moulins[k] - 1 of the concatenated arrays, off[k] = the entries of the members before it
// (a member without a flag may give 0, or a list that is skipped).  The checks of every flagged member; *nmax: the longest list
static int batch_moulin_check(const suhmo_batch *B, const BatchSel &sel, const int *n_moulins, const double *sigma, size_t *off, int *nmax)
{
    off[0] = 0;
    for (int k = 0; k < B->n; k++) off[k + 1] = off[k] + (n_moulins[k] > 0 ? (size_t)n_moulins[k] : 0);
    *nmax = 0;
    for (int z = 0; z < sel.n; z++) {
        const int k = sel.m[z];
        if (n_moulins[k] < 1) { suhmo_set_error("batch: moulin source: n_moulins = %d on member %d (at least 1)", n_moulins[k], k); return -1; }
        for (int m = 0; m < n_moulins[k]; m++)
            if (!(sigma[off[k] + m] > 0.0)) { suhmo_set_error("batch: moulin source: sigma <= 0 (member %d, its moulin %d)", k, m); return -1; }
        *nmax = std::max(*nmax, n_moulins[k]);
    }
    return 0;
}
// the lists and a row (MoulinJob) per flagged member into the batch's scratch, enqueued on st; time_factor NULL: 0 in the rows (a run passes the
// factor with every launch).  *integ_d: where the integrals of all lists will be
static int batch_moulin_upload(suhmo_batch *B, const BatchSel &sel, const int *n_moulins, const double *positions, const double *sigma, const double *flux,
                               const double *time_factor, const size_t *off, hipStream_t st, double **integ_out)
{
    const size_t N = off[B->n];
    const DV &v = view(B, 0);
    const size_t nblk = (size_t)((v.nx + 15) / 16) * ((v.ny + 15) / 16);
    // the device scratch: rows[n] | {x, y, sigma} x n_k, flux x n_k of every member (4 N) | integrals (N) | tile sums (nblk x N)
    static_assert(sizeof(MoulinJob) % sizeof(double) == 0, "rows and tables share one array of doubles");
    const size_t rowd = sizeof(MoulinJob) / sizeof(double), head = B->n * rowd, need = head + (5 + nblk) * N;
    if (need > B->moulin_cap) {
        HIPCHK(hipStreamSynchronize(st));
        if (B->d_moulin) (void)hipFree(B->d_moulin);
        B->d_moulin = nullptr; B->moulin_cap = 0;
        HIPCHK(hipMalloc(&B->d_moulin, need * sizeof(double)));
        B->moulin_cap = need;
    }
    double *tab_d = B->d_moulin + head, *integ_d = tab_d + 4 * N, *partial_d = integ_d + N;
    B->h_moulin.assign(head + 4 * N, 0.0);
    double *tab_h = B->h_moulin.data() + head;
    for (int z = 0; z < sel.n; z++) {
        const int k = sel.m[z], n = n_moulins[k];
        const size_t o = off[k];
        for (int m = 0; m < n; m++) {
            tab_h[4 * o + 3 * m] = positions[2 * (o + m)]; tab_h[4 * o + 3 * m + 1] = positions[2 * (o + m) + 1]; tab_h[4 * o + 3 * m + 2] = sigma[o + m];
            tab_h[4 * o + 3 * (size_t)n + m] = flux[o + m];
        }
        const Depth &D = B->mem[k]->d[0];
        const MoulinJob job{D.v, n, (int)nblk, tab_d + 4 * o, tab_d + 4 * o + 3 * (size_t)n, integ_d + o, partial_d + nblk * o, time_factor ? time_factor[k] : 0.0,
                            D.fp.f[SUHMO_F_MSRC]};
        memcpy(B->h_moulin.data() + k * rowd, &job, sizeof(job));
    }
    *integ_out = integ_d;
    const hipError_t e = hipMemcpyAsync(B->d_moulin, B->h_moulin.data(), B->h_moulin.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { suhmo_set_error("batch: moulin source: %s", hipGetErrorString(e)); return -2; }
    return 0;
}
extern "C" int suhmo_batch_moulin_source(suhmo_batch_t *B, const int *n_moulins, const double *positions, const double *sigma, const double *flux,
                                         const double *time_factor, double *integrals, const int *active, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::Calc_moulin_source_term_distributed");
    ARG(B && n_moulins && positions && sigma && flux && time_factor);
    hipStream_t st = (hipStream_t)s;
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    size_t off[SUHMO_BATCH_MAX + 1];
    int nmax = 0;
    int rc = batch_moulin_check(B, sel, n_moulins, sigma, off, &nmax); if (rc) return rc;
    const size_t N = off[B->n];
    if ((rc = batch_source_fields(B, sel, st))) return rc;
    const DV &v = view(B, 0);
    double *integ_d = nullptr;
    if ((rc = batch_moulin_upload(B, sel, n_moulins, positions, sigma, flux, time_factor, off, st, &integ_d))) return rc;
    if ((rc = suhmo_batch_moulin_launch((const MoulinJob *)B->d_moulin, sel, v.nx, v.ny, nmax, st))) return rc;
    B->launches += 3;
    hipError_t e = hipSuccess;
    if (integrals) { B->h_integ.resize(N); e = hipMemcpyAsync(B->h_integ.data(), integ_d, N * sizeof(double), hipMemcpyDeviceToHost, st); }
    if (e == hipSuccess) e = hipStreamSynchronize(st);       // (the one synchronisation: the integrals have arrived, the host table may be written again)
    if (e != hipSuccess) { suhmo_set_error("batch: moulin source: %s", hipGetErrorString(e)); return -2; }
    if (integrals)
        for (int z = 0; z < sel.n; z++) { const int k = sel.m[z]; memcpy(integrals + off[k], B->h_integ.data() + off[k], n_moulins[k] * sizeof(double)); }
    return 0;
}
// column sums of the flagged members in B->d_cols[k][8][nx]: the checks, then one launch
static int batch_column_launch(suhmo_batch *B, const suhmo_model_params_t *mp, const BatchSel &sel, hipStream_t st)
{
    for (int z = 0; z < sel.n; z++) {
        const int k = sel.m[z];
        const Depth &D = B->mem[k]->d[0];
        for (int f : {SUHMO_F_QWX, SUHMO_F_CD, SUHMO_F_MR, SUHMO_F_PW}) if (!D.fp.f[f]) { suhmo_set_error("batch: no time step has run on member %d", k); return -1; }
        if (mp[k].use_moulin_source && !D.fp.f[SUHMO_F_MSRC]) { suhmo_set_error("batch: use_moulin_source without a moulin source term (SUHMO_F_MSRC) on member %d", k); return -1; }
    }
    int rc = batch_enter(B, st); if (rc) return rc;
    if ((rc = batch_mp_sync(B, mp, st))) return rc;
    const DV &v = view(B, 0);
    const size_t per = 8 * (size_t)v.nx, need = B->n * per;
    if (need > B->cols_cap) {
        HIPCHK(hipStreamSynchronize(st));
        if (B->d_cols) (void)hipFree(B->d_cols);
        if (B->h_cols) (void)hipHostFree(B->h_cols);
        B->d_cols = B->h_cols = nullptr; B->cols_cap = 0;
        HIPCHK(hipMalloc(&B->d_cols, need * sizeof(double)));
        HIPCHK(hipHostMalloc(&B->h_cols, need * sizeof(double), hipHostMallocDefault));
        B->cols_cap = need;
    }
    if ((rc = launch_postproc_columns(on_members(tab(B, 0), sel, v, B->d_mp), B->d_cols, st))) return rc;
    B->launches++;
    return 0;
}
// ... and in B->h_cols[k][8][nx]: one copy, one synchronisation
static int batch_column_sums(suhmo_batch *B, const suhmo_model_params_t *mp, const BatchSel &sel, hipStream_t st)
{
    int rc = batch_column_launch(B, mp, sel, st); if (rc) return rc;
    const size_t per = 8 * (size_t)view(B, 0).nx;
    const int k0 = sel.m[0], k1 = sel.m[sel.n - 1];           // (the list ascends: the rows from the first to the last flagged member)
    HIPCHK(hipMemcpyAsync(B->h_cols + k0 * per, B->d_cols + k0 * per, (k1 - k0 + 1) * per * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    B->readbacks++;
    return 0;
}
// what: 0 the sums [n][8][nx], 1 suhmo_postproc_temporal of them [n][6], 2 suhmo_postproc_finish [n][nx][8]; rows of members without a flag stay
static int batch_postproc(suhmo_batch *B, const suhmo_model_params_t *mp, double *out, const int *active, suhmo_stream_t s, int what)
{
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    int rc = batch_column_sums(B, mp, sel, (hipStream_t)s); if (rc) return rc;
    const DV &v = view(B, 0);
    const size_t per = 8 * (size_t)v.nx;
    for (int z = 0; z < sel.n; z++) {
        const int k = sel.m[z];
        const double *sums = B->h_cols + k * per;
        if (what == 0) memcpy(out + k * per, sums, per * sizeof(double));
        else if ((rc = what == 1 ? suhmo_postproc_temporal(sums, v.nx, v.dx, out + 6 * (size_t)k) : suhmo_postproc_finish(sums, v.nx, v.dx, out + k * per))) return rc;
    }
    return 0;
}
extern "C" int suhmo_batch_postproc_partial(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *sums, const int *active, suhmo_stream_t s)
{
    ARG(B && mp && sums);
    return batch_postproc(B, mp, sums, active, s, 0);
}
extern "C" int suhmo_batch_postproc_temporal(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *out, const int *active, suhmo_stream_t s)
{
    ARG(B && mp && out);
    return batch_postproc(B, mp, out, active, s, 1);
}
extern "C" int suhmo_batch_postproc_table(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *table, const int *active, suhmo_stream_t s)
{
    ARG(B && mp && table);
    return batch_postproc(B, mp, table, active, s, 2);
}

// ---- the mass balance of the flagged members (include/suhmo_hip.h, "MASS BALANCE"; suhmo_balance.hip): one first stage, one final launch, one
// read-back; the rows of members without a flag stay the caller's.  Read-only
extern "C" int suhmo_batch_mass_balance(suhmo_batch_t *B, double *out, const int *active, suhmo_stream_t s)
{
    ARG(B && out);
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    int rc;
    for (int z = 0; z < sel.n; z++) if ((rc = suhmo_balance_check_member_(B->mem[sel.m[z]], sel.m[z]))) return rc;
    hipStream_t st = (hipStream_t)s;
    if ((rc = batch_enter(B, st))) return rc;
    const size_t per = suhmo_balance_member_doubles(), nres = (size_t)SUHMO_MB_COUNT * B->n;
    if (!B->d_bal) {
        if (hipMalloc(&B->d_bal, (B->n * per + nres) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); B->d_bal = nullptr; suhmo_set_error("batch: the partial buffer of the mass balance cannot be allocated"); return -2; }
        if (hipHostMalloc(&B->h_bal, nres * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); (void)hipFree(B->d_bal); B->d_bal = B->h_bal = nullptr;
            suhmo_set_error("batch: the pinned rows of the mass balance cannot be allocated"); return -2;
        }
    }
    double *res = B->d_bal + B->n * per;
    if ((rc = launch_mass_balance(on(B, 0, sel), B->d_bal, res, st))) return rc;
    B->launches += 2;
    const int k0 = sel.m[0], k1 = sel.m[sel.n - 1];           // (the list ascends: the rows from the first to the last flagged member)
    HIPCHK(hipMemcpyAsync(B->h_bal + SUHMO_MB_COUNT * k0, res + SUHMO_MB_COUNT * k0, (size_t)(k1 - k0 + 1) * SUHMO_MB_COUNT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    B->readbacks++;
    for (int z = 0; z < sel.n; z++) memcpy(out + SUHMO_MB_COUNT * (size_t)sel.m[z], B->h_bal + SUHMO_MB_COUNT * (size_t)sel.m[z], SUHMO_MB_COUNT * sizeof(double));
    return 0;
}

// ---- the water budget of the flagged members (include/suhmo_hip.h, "WATER BUDGET"; suhmo_balance.hip): as the mass balance, with mp[n] on the
// device for the members' ramp, distributed input, water density and source switch.  Read-only
static int batch_budget_check(const suhmo_batch *B, const suhmo_model_params_t *mp, const BatchSel &sel, const char *who, bool faces, bool source)
{
    int rc;
    for (int z = 0; z < sel.n; z++) if ((rc = suhmo_budget_check_member_(B->mem[sel.m[z]], &mp[sel.m[z]], sel.m[z], who, faces, source))) return rc;
    return 0;
}
static int batch_budget_buffers(suhmo_batch *B)
{
    if (B->d_wb) return 0;
    const size_t per = suhmo_budget_member_doubles(), nres = (size_t)SUHMO_WB_COUNT * B->n;
    if (hipMalloc(&B->d_wb, (B->n * per + nres) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); B->d_wb = nullptr; suhmo_set_error("batch: the partial buffer of the water budget cannot be allocated"); return -2; }
    if (hipHostMalloc(&B->h_wb, nres * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(B->d_wb); B->d_wb = B->h_wb = nullptr;
        suhmo_set_error("batch: the pinned rows of the water budget cannot be allocated"); return -2;
    }
    return 0;
}
// the first stage and the final launch; out: a DEVICE address, [n][SUHMO_WB_COUNT]
static int batch_budget_launch(suhmo_batch *B, const suhmo_model_params_t *mp, const BatchSel &sel, double *out, hipStream_t st)
{
    int rc = batch_enter(B, st); if (rc) return rc;
    if ((rc = batch_mp_sync(B, mp, st))) return rc;
    if ((rc = launch_water_budget(on_members(tab(B, 0), sel, view(B, 0), B->d_mp), B->d_wb, B->d_vol, B->vol_np, B->vol_have, out, st))) return rc;
    B->launches += 2;
    return 0;
}
extern "C" int suhmo_batch_water_budget(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *out, const int *active, suhmo_stream_t s)
{
    ARG(B && mp && out);
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    int rc;
    if ((rc = batch_budget_check(B, mp, sel, "suhmo_batch_water_budget", true, true))) return rc;
    hipStream_t st = (hipStream_t)s;
    HIPCHK(hipSetDevice(B->device));
    if ((rc = batch_budget_buffers(B))) return rc;
    double *res = B->d_wb + B->n * suhmo_budget_member_doubles();
    if ((rc = batch_budget_launch(B, mp, sel, res, st))) return rc;
    const int k0 = sel.m[0], k1 = sel.m[sel.n - 1];           // (the list ascends: the rows from the first to the last flagged member)
    HIPCHK(hipMemcpyAsync(B->h_wb + SUHMO_WB_COUNT * k0, res + SUHMO_WB_COUNT * k0, (size_t)(k1 - k0 + 1) * SUHMO_WB_COUNT * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    B->readbacks++;
    for (int z = 0; z < sel.n; z++) memcpy(out + SUHMO_WB_COUNT * (size_t)sel.m[z], B->h_wb + SUHMO_WB_COUNT * (size_t)sel.m[z], SUHMO_WB_COUNT * sizeof(double));
    return 0;
}

// ---- the run: AmrHydro::run (src/AmrHydro.cpp:1283-1365) of the flagged members in one call.  Per step the forcing launches from the
// schedule's values, suhmo_batch_timestep_run, and on a diagnostic step the column sums and the row finished on the device
// (d_postproc_temporal_row) into B->d_series[row][n][6]; one copy and one synchronisation after the last step
static int batch_run_series_out(suhmo_batch *B, const BatchSel &sel, int rows, double *out, hipStream_t st)
{
    if (rows <= 0) return 0;
    const size_t per = 6 * (size_t)B->n;
    HIPCHK(hipMemcpyAsync(B->h_series, B->d_series, rows * per * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    B->readbacks++;
    for (int r = 0; r < rows; r++)                           // (the entries of members without a flag stay the caller's)
        for (int z = 0; z < sel.n; z++) memcpy(out + r * per + 6 * (size_t)sel.m[z], B->h_series + r * per + 6 * (size_t)sel.m[z], 6 * sizeof(double));
    return 0;
}
// the budget rows of a run [rows][n][10] (B->d_wbs): one copy, one synchronisation; the entries of members without a flag stay the caller's
static int batch_run_budget_out(suhmo_batch *B, const BatchSel &sel, int rows, double *out, hipStream_t st)
{
    if (rows <= 0) return 0;
    const size_t per = (size_t)SUHMO_WB_COUNT * B->n;
    HIPCHK(hipMemcpyAsync(B->h_wbs, B->d_wbs, rows * per * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    B->readbacks++;
    for (int r = 0; r < rows; r++)
        for (int z = 0; z < sel.n; z++)
            memcpy(out + r * per + SUHMO_WB_COUNT * (size_t)sel.m[z], B->h_wbs + r * per + SUHMO_WB_COUNT * (size_t)sel.m[z], SUHMO_WB_COUNT * sizeof(double));
    return 0;
}
extern "C" int suhmo_batch_run(suhmo_batch_t *B, const suhmo_model_params_t *mp, const suhmo_batch_schedule_t *sch, const int *active,
                               suhmo_batch_run_result_t *res, suhmo_stream_t s)
{
    return suhmo_batch_run_bud(B, mp, sch, active, nullptr, res, s);
}
// bud != NULL: "WATER BUDGET", the series inside the runs -- a budget row of every flagged member after the steps that end one, finished on the
// device into B->d_wbs; those steps run with track_old_volume = 1, the others with the caller's setting, which every way out restores
extern "C" int suhmo_batch_run_bud(suhmo_batch_t *B, const suhmo_model_params_t *mp, const suhmo_batch_schedule_t *sch, const int *active,
                                   suhmo_run_budget_t *bud, suhmo_batch_run_result_t *res, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::run");
    ARG(B && mp && sch && res);
    hipStream_t st = (hipStream_t)s;
    res->steps_done = 0; res->n_rows = 0;
    if (bud) bud->n_rows = 0;
    if (sch->n_steps < 1) { suhmo_set_error("batch: run: n_steps = %d (at least 1)", sch->n_steps); return -1; }
    if (!(sch->dt > 0.0) || sch->first_cur_step < 1 || sch->diag_every < 0) { suhmo_set_error("batch: run: dt > 0, first_cur_step >= 1 and diag_every >= 0"); return -1; }
    if (sch->n_members != B->n) { suhmo_set_error("batch: run: the schedule is laid out for %d members, the batch has %d", sch->n_members, B->n); return -1; }
    const bool recharge = sch->T_K || sch->background, moulins = sch->n_moulins || sch->positions || sch->sigma || sch->flux || sch->moulin_factor;
    if (recharge && !(sch->T_K && sch->background)) { suhmo_set_error("batch: run: a temperature schedule needs T_K and background"); return -1; }
    if (moulins && !(sch->n_moulins && sch->positions && sch->sigma && sch->flux && sch->moulin_factor)) {
        suhmo_set_error("batch: run: a moulin schedule needs n_moulins, positions, sigma, flux and moulin_factor"); return -1;
    }
    if (recharge && moulins) { suhmo_set_error("batch: run: a temperature schedule and a moulin schedule write the same source term (SUHMO_F_MSRC): give one"); return -1; }
    const int n = B->n, total_rows = sch->diag_every ? sch->n_steps / sch->diag_every : 0;
    if (total_rows > 0 && !res->rows) { suhmo_set_error("batch: run: %d rows and no array for them", total_rows); return -1; }
    if (bud && bud->every < 1) { suhmo_set_error("batch: run: a budget row every %d steps (at least 1)", bud->every); return -1; }
    if (bud && !bud->rows) { suhmo_set_error("batch: run: a budget series and no array for its rows"); return -1; }
    const int total_wb = bud ? sch->n_steps / bud->every : 0;
    const BatchSel sel = flagged_members(B, active);
    if (!sel.n) return 0;
    // ---- every flagged member, before anything is launched
    size_t off[SUHMO_BATCH_MAX + 1];
    int nmax = 0, rc;
    for (int z = 0; z < sel.n; z++) {
        const int k = sel.m[z];
        const Depth &D = B->mem[k]->d[0];
        if (recharge && !D.fp.f[SUHMO_F_ZS]) { suhmo_set_error("batch: run: time-varying recharge: load the ice surface height (SUHMO_F_ZS) of member %d first", k); return -1; }
        if (mp[k].use_impl_diff && !B->implicit_gap) { suhmo_set_error("batch: run: use_impl_diff = 1 (member %d) without batch option implicit_gap", k); return -5; }
        if (mp[k].use_impl_diff && mp[k].diffFactor == 0.0) { suhmo_set_error("batch: run: use_ImplDiff with diffFactor = 0 (member %d)", k); return -1; }
        if (mp[k].use_moulin_source && !recharge && !moulins && !D.fp.f[SUHMO_F_MSRC]) {
            suhmo_set_error("batch: run: use_moulin_source without a source term or a schedule that writes one (member %d)", k); return -1;
        }
    }
    if (moulins && (rc = batch_moulin_check(B, sel, sch->n_moulins, sch->sigma, off, &nmax))) return rc;
    // (the face coefficients and the melt rate are the first step's to form; the source term is the rule above)
    if (bud && (rc = batch_budget_check(B, mp, sel, "batch: run: budget", false, false))) return rc;
    HIPCHK(hipSetDevice(B->device));
    if ((rc = (recharge || moulins) ? batch_source_fields(B, sel, st) : batch_enter(B, st))) return rc;      // (bottom_solver of the handles: rc -5)
    // ---- what the run needs on the device: the lists once, the series
    const DV &v = view(B, 0);
    if (moulins) {
        double *integ_d = nullptr;
        if ((rc = batch_moulin_upload(B, sel, sch->n_moulins, sch->positions, sch->sigma, sch->flux, nullptr, off, st, &integ_d))) return rc;
        HIPCHK(hipStreamSynchronize(st));                    // (the host table may be written again)
    }
    const size_t per = 6 * (size_t)n;
    if (total_rows * per > B->series_cap) {
        HIPCHK(hipStreamSynchronize(st));
        if (B->d_series) (void)hipFree(B->d_series);
        if (B->h_series) (void)hipHostFree(B->h_series);
        B->d_series = B->h_series = nullptr; B->series_cap = 0;
        HIPCHK(hipMalloc(&B->d_series, total_rows * per * sizeof(double)));
        HIPCHK(hipHostMalloc(&B->h_series, total_rows * per * sizeof(double), hipHostMallocDefault));
        B->series_cap = total_rows * per;
    }
    const size_t wper = (size_t)SUHMO_WB_COUNT * n;
    if (total_wb > 0) {
        if ((rc = batch_budget_buffers(B))) return rc;
        if (total_wb * wper > B->wbs_cap) {
            HIPCHK(hipStreamSynchronize(st));
            if (B->d_wbs) (void)hipFree(B->d_wbs);
            if (B->h_wbs) (void)hipHostFree(B->h_wbs);
            B->d_wbs = B->h_wbs = nullptr; B->wbs_cap = 0;
            HIPCHK(hipMalloc(&B->d_wbs, total_wb * wper * sizeof(double)));
            HIPCHK(hipHostMalloc(&B->h_wbs, total_wb * wper * sizeof(double), hipHostMallocDefault));
            B->wbs_cap = total_wb * wper;
        }
    }
    std::vector<suhmo_model_params_t> mps(mp, mp + n);
    const int track = B->track_old_volume;
    int rows = 0, wrows = 0;
    rc = 0;
    for (int k = 0; k < sch->n_steps && !rc; k++) {
        PerMember a, b;
        if (recharge) {
            memset(&a, 0, sizeof(a)); memset(&b, 0, sizeof(b));
            for (int m = 0; m < n; m++) { a.x[m] = sch->T_K[(size_t)k * n + m]; b.x[m] = sch->background[(size_t)k * n + m]; }
            if ((rc = launch_time_varying_recharge(on(B, 0, sel), a, b, st))) break;
            B->launches++;
        }
        if (moulins) {
            memset(&a, 0, sizeof(a));
            for (int m = 0; m < n; m++) a.x[m] = sch->moulin_factor[(size_t)k * n + m];
            if ((rc = suhmo_batch_moulin_launch((const MoulinJob *)B->d_moulin, sel, v.nx, v.ny, nmax, st, &a))) break;
            B->launches += 3;
        }
        if (sch->ramp) for (int m = 0; m < n; m++) mps[m].ramp = sch->ramp[k];
        const bool brow = total_wb > 0 && (k + 1) % bud->every == 0;
        if (brow) B->track_old_volume = 1;
        rc = suhmo_batch_timestep_run(B, mps.data(), sch->dt, sch->first_cur_step + k, res->picard_iters ? res->picard_iters + (size_t)k * n : nullptr,
                                      res->vcycles ? res->vcycles + (size_t)k * n : nullptr, st, active);
        B->track_old_volume = track;
        if (rc) break;
        res->steps_done = k + 1;
        if (sch->diag_every && (k + 1) % sch->diag_every == 0) {
            if ((rc = batch_column_launch(B, mps.data(), sel, st))) break;
            if ((rc = launch_postproc_temporal_row(on(B, 0, sel), B->d_cols, B->d_series + rows * per, st))) break;
            B->launches++;
            rows++;
        }
        if (brow) {
            if ((rc = batch_budget_launch(B, mps.data(), sel, B->d_wbs + wrows * wper, st))) break;
            wrows++;
        }
    }
    res->n_rows = rows;
    const std::string msg = rc ? suhmo_last_error() : "";
    int rc2 = batch_run_series_out(B, sel, rows, res->rows, st);
    if (bud) {
        const int rc3 = batch_run_budget_out(B, sel, wrows, bud->rows, st);
        if (!rc3) bud->n_rows = wrows;
        rc2 = rc2 ? rc2 : rc3;
    }
    if (rc && !rc2) suhmo_set_error("%s", msg.c_str());
    return rc ? rc : rc2;
}

extern "C" int suhmo_batch_set_option(suhmo_batch_t *B, const char *key, long value)
{
    ARG(B && key);
    if (!strcmp(key, "tile_order")) { ARG(value >= 0 && value <= 2); B->tile_order = (int)value; return 0; }
    if (!strcmp(key, "bottom_solver")) {
        if (value == B->bottom_solver) return 0;
        suhmo_set_error("batch: bottom_solver = %ld on a batch created with %d: the option is fixed at creation (suhmo_batch_create_opts)", value, B->bottom_solver);
        return -5;
    }
    if (!strcmp(key, "implicit_gap")) { ARG(value == 0 || value == 1); B->implicit_gap = (int)value; return 0; }
    if (!strcmp(key, "track_old_volume")) { ARG(value == 0 || value == 1); B->track_old_volume = (int)value; return 0; }
    if (!strcmp(key, "batch_launches") || !strcmp(key, "batch_readbacks") || !strcmp(key, "batch_member_cycles") || !strcmp(key, "batch_gap_member_cycles")
        || !strcmp(key, "bottom_solver_iterations") || !strcmp(key, "bottom_solves_one_launch")) { suhmo_set_error("batch: option %s is read-only", key); return -1; }
    suhmo_set_error("batch: unknown option %s", key);
    return -1;
}
extern "C" int suhmo_batch_get_option(const suhmo_batch_t *B, const char *key, long *value)
{
    ARG(B && key && value);
    if (!strcmp(key, "tile_order")) *value = B->tile_order;
    else if (!strcmp(key, "bottom_solver")) *value = B->bottom_solver;
    else if (!strcmp(key, "bottom_solver_iterations") || !strcmp(key, "bottom_solves_one_launch")) {      // summed over the members, the gap batch's included
        const int which = strcmp(key, "bottom_solver_iterations") ? 1 : 0;
        *value = 0;
        for (const suhmo_batch *b : {B, (const suhmo_batch *)B->gap})
            if (b) for (const suhmo_level *L : b->mem) *value += suhmo_bottom_counter(L, which);
    }
    else if (!strcmp(key, "implicit_gap")) *value = B->implicit_gap;
    else if (!strcmp(key, "track_old_volume")) *value = B->track_old_volume;
    else if (!strcmp(key, "batch_launches")) *value = B->launches + (B->gap ? B->gap->launches : 0);
    else if (!strcmp(key, "batch_readbacks")) *value = B->readbacks + (B->gap ? B->gap->readbacks : 0);
    else if (!strcmp(key, "batch_member_cycles")) *value = B->member_cycles;
    else if (!strcmp(key, "batch_gap_member_cycles")) *value = B->gap ? B->gap->member_cycles : 0;
    else { suhmo_set_error("batch: unknown option %s", key); return -1; }
    return 0;
}
