// suhmo_hier_int.h -- what the units of a hierarchy share.  AMR hierarchies whose levels are UNIONS OF BOXES, the way the reference grids them
// (BRMeshRefine with fill_ratio < 1 and block_factor 2: several abutting and disjoint boxes per level,
// src/AmrHydro.cpp:4176-4604, exec/AMR_multiMoulins/run_C_3lev/input.hydro:37,64-83).
//
// Level 0 is one level handle (the domain, with its multigrid depths: every fast kernel of suhmo_gsrb.hip runs there).
// A level l >= 1 is a list of rectangles, each an ordinary level handle created as a patch of the refined domain
// (desc.i0 / nx_global / j0 / ny_global): a rectangle keeps its own ghost ring in its canvas, exactly as a Chombo box
// keeps its own ghost cells -- at a re-entrant corner of the union the same index is the x-ghost of one box and the
// y-ghost of another, with different interpolated values.  What ties the rectangles together is compiled ONCE, when
// the hierarchy is created, into index plans that live in HBM; every inter-box / inter-level step is then one kernel
// launch over a plan, whatever the number of boxes:
//   ff      ghost cell <- the cell of the box of the same level that holds it (Copier::exchange,
//           src/VCAMRNonLinearPoissonOp.cpp:912-913; sides, and corners for the fields exchanged with the default copier)
//   cf      coarse-fine ghost cell <- QuadCFInterp from level l-1, the tangential stencil chosen on the host from the
//           coverage of the coarse cells ([Chombo] QuadCFStencil; oracle/amrm.c:cf_interp states the same rule)
//   pwl     ghost cell (corners included) <- PiecewiseLinearFillPatch from level l-1
//   avg     rectangles (fine box x coarse box) for FORT_AVERAGE / zeroing covered cells
//   win     per fine box the coarse correction over coarsen(box) grown by one cell, gathered from the boxes of level
//           l-1 (the copyTo of AMRProlongS_2, src/AMRNonLinearPoissonOp.cpp:1156), then PROLONG_2_NL
//   reflux  per coarse cell next to coarse-fine faces: its faces in the order (fine box, direction, side)
// Field pointers of levels >= 1 are held in a device table per level (the boxes relax with in-place colour passes, so
// the pointers never move); the base level's pointers travel as a kernel argument (its phi canvases ping-pong).
//
// Cycle = suhmo_amr.hip's, arithmetic = oracle/amrm.c, bit for bit.  [Chombo] pieces are
// restated from upstream Chombo 3.2 (fork not vendored): unpinned against the reference.
#pragma once
#include "suhmo_hier.h"
#include <algorithm>
#define HST(s) ((hipStream_t)(s))

namespace hier {
struct Ref { int b, off; };                          // cell of a level: box index, canvas offset
struct CopyEnt { Ref d, s; };
struct CfEnt { Ref f; int step; int kind; int xsign; Ref c[3]; };
// kind: 0 centred (c = cm, c0, cp)   1 forward 2nd order (c0, cp, cpp)   2 forward 1st order (c0, cp)
//       3 backward 2nd order (c0, cm, cmm)   4 backward 1st order (c0, cm)   5 no tangential derivative (c0)
struct PwlEnt { Ref f; Ref c[9]; int par; int sx, sy; };   // c[4] = the coarse cell; b = -1: outside the domain; par: bit0 gi&1, bit1 gj&1
                                                           // sx, sy: slope stencil 0 central, 1 one-sided hi (no lo neighbour), 2 one-sided lo
struct RectEnt { int fb, cb, foff, coff, w, h; };          // average: w x h coarse cells
struct WinEnt { int cb, coff, woff, w, h; };               // window gather: w x h coarse cells into the window buffer
struct Face { int dir, side; int fb, foff; Ref hi, lo, bq; };
struct Target { Ref t; int first, count; };
struct Win { int i0, j0, nx, ny; size_t base; };           // coarse window of a fine box: origin (level l-1 indices), size, offset in the level's buffer

template <class T> struct DevVec {
    T *d = nullptr; size_t n = 0;
    int upload(const std::vector<T> &h)
    {
        n = h.size();
        if (!n) return 0;
        if (hipMalloc(&d, n * sizeof(T)) != hipSuccess) return -2;
        if (hipMemcpy(d, h.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return -2;
        return 0;
    }
    void release() { if (d) (void)hipFree(d); d = nullptr; n = 0; }
};

// spatial index of a level's boxes (bucket grid), for the point and rectangle queries of the plan builder
struct BoxIndex {
    int nxd = 0, nyd = 0, bs = 32, nbx = 0, nby = 0;
    std::vector<int> start, items;
    const std::vector<int> *b4 = nullptr;
    void build(const std::vector<int> &boxes, int nx, int ny);    // suhmo_hier_plan.hip
    int find(int i, int j) const            // box holding cell (i,j) (inside the domain), -1 = none
    {
        size_t q = (size_t)(j / bs) * nbx + i / bs;
        for (int p = start[q]; p < start[q + 1]; p++) {
            const int *b = &(*b4)[4 * items[p]];
            if (i >= b[0] && i <= b[2] && j >= b[1] && j <= b[3]) return items[p];
        }
        return -1;
    }
};

// ---- levels dealt to the ranks (owner computes).  A cell that a plan executed on one rank reads from a box another rank owns travels
// as ONE packed value: the owner packs the cells somebody needs (send, in a fixed order), one all-gather moves every rank's segment,
// the reader scatters what it needs into its MIRROR of the owner's box (recv: mirror cell, owner rank, position in that segment).
// Mirrors exist only for boxes some plan of this rank reads; every other foreign box is a stub without storage.
struct SyncRecv { Ref d; int rank, pos; };
struct Sync {
    DevVec<Ref> send; DevVec<SyncRecv> recv; long stride = 0;         // stride: longest segment over the ranks (0: nothing travels, no collective)
    void release() { send.release(); recv.release(); stride = 0; }
};
struct Xf { int owner, b, off, reader; };                             // plan building: cell (b, off) of `owner` is read on `reader`
struct PutEnt { int cb, coff, rank, pos, w, h; };                     // w x h averaged cells arriving in `rank`'s segment at pos -> box cb at coff
struct HLev {
    int l = 0, nxd = 0, nyd = 0;
    std::vector<suhmo_level *> box;
    std::vector<int> b4;
    BoxIndex index;
    // plans (device)
    DevVec<CopyEnt> ff_side, ff_all;                 // ff_all = sides, then corners (the default copier's exchange in one launch)
    DevVec<int2> push; DevVec<int> pbase;            // ff_side seen from the source cell (the colour passes push, suhmo_gsrb.hip)
    DevVec<int2> halo; DevVec<int> hbase; bool halo_ok = false;   // per box the cells of its 4-cell surroundings (box, canvas offset; -1: no cell of the level): two sweeps per launch
    DevVec<CfEnt> cf;
    DevVec<PwlEnt> pwl;
    DevVec<RectEnt> avg; int avg_w = 0, avg_h = 0;
    DevVec<WinEnt> wing; int wing_w = 0, wing_h = 0; DevVec<int> wstart; int win_max = 0;   // wstart[k] .. wstart[k + 1]: the pieces of box k's window
    DevVec<Target> targets; DevVec<Face> faces;
    // level 1 only, in the cells of this rank's part of level 0: the rectangles whose L(phi) / residual change when level 1's head is
    // averaged down (coarsen(box) grown by one cell, periodic images included), and the cells its gradient interpolation reads
    DevVec<int4> dirty0; int dirty_w = 0, dirty_h = 0; DevVec<int2> gcells;
    std::vector<Win> win; double *winbuf = nullptr, *winold = nullptr; size_t winelems = 0; Win *d_win = nullptr; int *d_wing_box = nullptr;
    // field pointer / view tables of the boxes
    std::vector<FP> h_fp; FP *d_fp = nullptr; DV *d_dv = nullptr;
    // the same table with the two canvases of the head trading places: a relaxation of an odd number of launches inside a V-cycle leaves its
    // result on the second canvas and makes THAT the head (swap_head) instead of copying it back; the post-smoothing undoes it
    std::vector<FP> h_fp_alt; FP *d_fp_alt = nullptr; bool swapped = false;
    unsigned long tab_epoch = 0;                                  // suhmo_fp_epoch() the tables were last compared at
    unsigned long long ensured = 0;                               // fields every box is known to have
    int self_wrap = -1;                                            // some box of the level is its own periodic neighbour (-1: not looked at yet)
    double *d_red = nullptr; int maxnx = 0, maxny = 0;            // reduction scratch (64 nbox + 16 doubles), largest box
    // ---- owner computes (rank strips, creation option partition_min_cells): boxes own[r] .. own[r+1] belong to rank r (LoadBalance,
    // src/AmrHydro.cpp:4283, 4929).  EVERY pass over the level runs on the owner's boxes only; plans are executed by the owner of the cell
    // they write; what they read of other ranks' boxes travels as packed cells (Sync), what they write into them (averages) as packed
    // rectangles (avg_put / avg_get).  The ghost exchange before a colour pass (Copier::exchange, src/VCAMRNonLinearPoissonOp.cpp:692,
    // 912-913) moves the side cells of ONE colour of the boxes that have a neighbour on another rank and nothing else.
    bool part = false;
    std::vector<int> own, owner;                     // owner[k]
    std::vector<char> held;                          // this rank keeps storage for box k (its own, or a mirror some plan here reads)
    int b0 = 0, nown = 0;                            // this rank's boxes: b0 .. b0 + nown
    int first_owned() const { return part ? b0 : 0; }                 // the boxes this rank computes (a replicated level: all of them)
    int n_owned() const { return part ? nown : (int)box.size(); }
    Sync sy_side[2], sy_sides, sy_all;               // cells of THIS level: sources of fine-fine side ghosts by colour / both colours / sides + corners
    Sync sy_cread, sy_win;                           // cells of level l-1 (>= 1) the stencils / the correction windows of this level's plans read here
    Sync sy_fface;                                   // cells of THIS level the reflux into level l-1 reads on the owners of the coarse cells
    DevVec<RectEnt> avg_cov; int cov_w = 0, cov_h = 0;       // covered rectangles by the owner of the COARSE cells (zeroing / marking them)
    DevVec<RectEnt> avg_put; DevVec<PutEnt> avg_get; long put_stride = 0, put_mine = 0; int put_w = 0, put_h = 0, get_w = 0, get_h = 0;
    long owned_cells = 0, held_boxes = 0;
    DevVec<long> snap_cells[2];                      // suhmo_snap.hip: per box the cells of the boxes before it, each grown by 0 / 1 ghost cells (built on first use)
    // suhmo_flatten.hip: the level's private scratch -- per component slot ONE allocation that holds a canvas of every box (flat_elems doubles),
    // and the boxes' pointers into them as a table, slot q in f[q] (on the host; for the levels >= 1 on the device too).  Allocated on first use
    std::vector<double *> flat_slab; size_t flat_elems = 0; std::vector<FP> flat_h; FP *flat_fp = nullptr;
};
}  // namespace hier

struct suhmo_hier {
    int nlev = 0, device = 0;
    hier::HLev lev[8];
    suhmo_bc_t bc;
    suhmo_level_desc_t base_desc;
    suhmo_hier *gap = nullptr; double gap_dt = 0.0;        // implicit gap-height operator of the time step, owned
    bool base_borrowed = false;                            // level 0's handle belongs to another hierarchy (suhmo_hier_regrid, while the new one is built /
                                                           // once the old one has handed its base level over): suhmo_hier_destroy leaves it alone
    // ---- level 0 cut into rank strips (one process per GPU): a rank holds its own rows of level 0 and ALL boxes of the finer
    // levels.  What level 1 reads of level 0 (coarse-fine stencils, linear fill, correction windows, reflux) comes from a
    // SHADOW: canvases with the geometry of the whole level 0, kept current only at the cells the plans read (`need`, sorted
    // by row, so the cells a rank owns are one segment); one all-gather refreshes a field (or several) before a plan runs.
    // What level 1 writes into level 0 (averages, reflux) is clipped to the rank's own rows when the plans are built.
    int rank = 0, world = 1;
    DV vglob;                                              // level 0 as one canvas (= the base view when it is not cut)
    FP shadow{};                                           // COMPACT: only the rows of level 0 that hold a cell some plan reads (shadow_rows of them, pitch
    size_t shadow_elems = 0; int shadow_rows = 0;          // vglob.P; a plan's offset = compact row * P + column); fields allocated on first use
    double *cover_whole = nullptr;                         // SUHMO_F_COVER of the WHOLE level 0 (geometry only; the moulin integrals run over all of it)
    hier::DevVec<int> need, need_c; hier::DevVec<int2> need_rl;        // offsets in vglob (what the owner packs) / in the compact shadow; (owner rank, position in its segment)
    std::vector<int> seg;                                  // need[seg[r] .. seg[r+1]) are rows of rank r
    long cnt_max = 0;                                      // longest segment: every rank contributes cnt_max doubles per field
    double *xs = nullptr, *xr = nullptr; size_t xcap = 0;  // staging of the all-gather
    suhmo_hier_allgather_fn ag = nullptr; void *ag_user = nullptr;
    long gathers = 0;
    // coarse-fine ghosts of the head of level l are current while neither level l's nor level l-1's head has been written since they
    // were interpolated: phi_ver[l] counts the writes, cf_seen[l] = the two versions the ghosts were made from
    unsigned long phi_ver[8] = {1, 1, 1, 1, 1, 1, 1, 1}, cf_seen[8][2] = {}, ff_seen[8] = {};    // ff_seen: likewise the fine-fine side ghosts
    bool phi_shadow_fresh = false;                         // the shadow's head is current: nothing has written level 0's head since its refresh
    // LPHI and RES = rhs - LPHI of level 0 were evaluated over the whole level (the composite residual of the solve loop) and, since
    // then, level 0's head has changed only where level 1 was averaged down: the next composite residual re-evaluates only the
    // rectangles lev[1].dirty0.  base_full_ver counts every other write to level 0 (head, right-hand side, coefficients: all of them
    // pass through the level-0 V-cycle or an entry point of the C-ABI)
    unsigned long base_full_ver = 1, base_res_seen = 0;
    // ... or were left behind by the launch that ended level 0's own V-cycle (suhmo_gsrb.hip, residual output): the solve loop's residual
    // evaluation then needs no pass over level 0 at all
    unsigned long base_fused_ver = 0;
    // ---- the options (their table, defaults and what a change resets: hier_opts in suhmo_hier.hip)
    long push_ghosts;                                      // push_ghosts = 0: an exchange launch before every colour pass instead
    long fused_relax;                                      // two sweeps per launch on levels of boxes (0: a launch per colour pass)
    long box_sweeps;                                       // sweeps per launch of k_gsrb_box_m (4 or 2)
    long merged_launches;                                  // both kinds of ghost cell in one launch, one norm read-back per hierarchy, ... (0: a launch each)
    long fused_prolong;                                    // AMRProlongS_2 of a box in one workgroup (0: gather, BC, prolongation as three launches)
    long incremental;                                      // incremental_residual
    long shadowed;                                         // creation option shadow = 1, or world > 1 (tests: the whole path on one rank)
    long part_min_cells;                                   // creation option partition_min_cells: when the largest level >= 1 holds at least this many cells
                                                           // PER RANK, the levels >= 1 are dealt to the ranks (below it a pass is shorter than the messages it needs)
    bool part = false;                                     // ... they are
    long n_fused_relax = 0;                                // launches of two sweeps or more on levels of boxes (read-only option fused_relax_launches)
    long part_gathers = 0, part_bytes = 0;                 // collectives of the partition; bytes THIS rank contributed to them
    long side_bytes[8] = {};                               // bytes this rank contributes to ONE colour-pass ghost exchange of level l (the larger colour)
    double *ps = nullptr, *pr = nullptr; size_t pcap = 0;  // staging of those collectives (pcap doubles per rank)
    // read-only counters (suhmo_hier_get_option): composite residuals of level 0 evaluated on the dirty rectangles only / not at all (left
    // behind by the launch that ended level 0's V-cycle), coarse gradients evaluated on the cell list only
    long n_incr_residual = 0, n_fused_residual = 0, n_sparse_grad = 0;
    // launches of suhmo_hier_time_varying_recharge (one per level), calls of suhmo_hier_moulin_source, copies of a run's series to the host
    // (read-only options recharge_launches, moulin_source_calls, run_readbacks; a run carries them across its regrids)
    long n_recharge_launches = 0, n_moulin_calls = 0, n_run_readbacks = 0;
    // suhmo_snap.hip: device staging of a snapshot (the largest level's packed size so far; allocated on first use), its launches and copies
    // (read-only options snapshot_launches, snapshot_copies); plots and checkpoints the last run handed to its callback (run_plots, run_checkpoints)
    double *snap_buf = nullptr; size_t snap_cap = 0;
    long n_snap_launches = 0, n_snap_copies = 0, n_run_plots = 0, n_run_checkpoints = 0;
    // suhmo_flatten.hip: the finest array on the device (the largest so far; allocated on first use), the launches and copies of the flattens
    // (read-only options flatten_launches, flatten_copies)
    double *flat_buf = nullptr; size_t flat_cap = 0;
    long n_flat_launches = 0, n_flat_copies = 0;
    // suhmo_compare.hip: the partials of every first stage of a comparison and, behind them, what its final stage leaves (allocated on first use;
    // cmp_cap doubles), its launches and copies (read-only options compare_launches, compare_copies, compare_device_bytes)
    double *cmp_buf = nullptr; size_t cmp_cap = 0;
    long n_cmp_launches = 0, n_cmp_copies = 0;
    // suhmo_balance.hip: the partials of every first stage of a mass balance and, behind them, the seven sums per level (allocated on first use;
    // bal_cap doubles), its launches and copies (read-only options balance_launches, balance_copies, balance_device_bytes)
    double *bal_buf = nullptr; size_t bal_cap = 0;
    long n_bal_launches = 0, n_bal_copies = 0;
    // "WATER BUDGET" (suhmo_balance.hip).  track_old_volume: option (hier_opts): suhmo_hier_timestep begins with k_volume of every level into
    // vol_buf -- level l's partials at vol_off[l], vol_n[l] of them (0: no tracked step has run on this handle); wb_buf: the partials of every
    // first stage of a budget and, behind them, ten values per level (wb_cap doubles).  Allocated on first use.  Read-only options
    // budget_launches, budget_copies (a run carries them across its regrids), budget_device_bytes
    long track_old_volume;
    double *vol_buf = nullptr, *wb_buf = nullptr; size_t vol_cap = 0, wb_cap = 0;
    size_t vol_off[8] = {}; int vol_n[8] = {};
    long n_wb_launches = 0, n_wb_copies = 0;
    // suhmo_ibc.hip, "INITIAL CONDITIONS": the IBC suhmo_hier_set_ibc left on the handle (suhmo_hier_regrid reloads every new level with it and hands it
    // to the new handle) and the launches of the IBC bodies so far (read-only option ibc_launches; a regrid carries it over)
    bool has_ibc = false; suhmo_ibc_t ibc{};
    long n_ibc_launches = 0;
    long flat_fail_slot = -1;                              // option flatten_fail_slot (tests): the allocation of this scratch slot on the finest level fails
    double *red_all = nullptr;                             // partial maxima of a norm over all levels of boxes (64 per box + 16)
    struct suhmo_tagmap *tags[8] = {};                     // tag maps of suhmo_hier_tag_cells, one per level (suhmo_tags.hip), owned
    hier::DevVec<hier::RectEnt> cover_full;                            // coarsen(boxes of level 1) in the shadow: COVER of the whole level 0
};

namespace hier {
inline bool wrap_cell(const suhmo_hier *H, const HLev &V, int &i, int &j)
{
    if (H->bc.periodic[0]) { if (i < 0) i += V.nxd; else if (i >= V.nxd) i -= V.nxd; }
    if (H->bc.periodic[1]) { if (j < 0) j += V.nyd; else if (j >= V.nyd) j -= V.nyd; }
    return i >= 0 && i < V.nxd && j >= 0 && j < V.nyd;
}
inline int owner_of(const suhmo_hier *H, const HLev &V, int i, int j)
{
    if (!wrap_cell(H, V, i, j)) return -1;
    if (V.l == 0) return 0;
    return V.index.find(i, j);
}
// canvas reference of the cell (i,j) (level indices, wrapped into the domain) in the box that holds it; b = -1 if none
inline Ref cell_ref(const suhmo_hier *H, const HLev &V, int i, int j)
{
    Ref r{-1, 0};
    if (!wrap_cell(H, V, i, j)) return r;
    int o = V.l == 0 ? 0 : V.index.find(i, j);
    if (o < 0) return r;
    const DV &v = V.l == 0 ? H->vglob : V.box[o]->d[0].v;
    r.b = o; r.off = cidx(v, i - v.i0, j - v.j0);
    return r;
}
inline bool dist_base(const suhmo_hier *H) { return H->shadowed; }
inline suhmo_level *base_of(suhmo_hier *H) { return H->lev[0].box[0]; }
inline void faces_made(suhmo_hier *H, int l) { for (suhmo_level *L : H->lev[l].box) suhmo_faces_made(L); }      // the level's face coefficients are about to be formed
inline Ref local_ref(const HLev &V, int k, int il, int jl) { return Ref{k, cidx(V.box[k]->d[0].v, il, jl)}; }

// ---- suhmo_hier_plan.hip: the plans of level l, compiled once at creation (after part_setup has dealt the boxes to the ranks)
int part_setup(suhmo_hier *H, int l);
int build_plans(suhmo_hier *H, int l);

// ---- suhmo_hier_fill.hip: device tables, plan launches
// device table of the boxes' field pointers (levels >= 1).  The boxes relax in place, so a pointer changes only when a
// field is allocated for the first time: then the table is uploaded again (rare; synchronous).
int refresh_tables_upload(suhmo_hier *H, int l, hipStream_t st);
inline int refresh_tables(suhmo_hier *H, int l, hipStream_t st)
{
    if (l == 0) return 0;
    const HLev &V = H->lev[l];
    // (63 boxes x 32 pointers compared before every launch was a third of the host's time per launch: no field pointer anywhere has
    //  changed since the last comparison -> the tables are current)
    if (V.d_fp && V.d_dv && V.h_fp.size() == V.box.size() && V.tab_epoch == suhmo_fp_epoch()) return 0;
    return refresh_tables_upload(H, l, st);
}
void swap_head(suhmo_hier *H, int l);
inline int ensure_field(suhmo_hier *H, int l, int field)
{
    HLev &V = H->lev[l];
    if (V.ensured >> field & 1ull) return 0;
    for (size_t k = 0; k < V.box.size(); k++) {
        if (V.part && !V.held[k]) continue;                            // a box other ranks hold: no storage here
        if (!suhmo_field(V.box[k], 0, field)) { suhmo_set_error("field allocation failed"); return -2; }
    }
    V.ensured |= 1ull << field;
    return 0;
}
// all boxes of level l >= 1 as one launch target
inline int multi_of(suhmo_hier *H, int l, hipStream_t st, suhmo_multi &m)
{
    int rc = refresh_tables(H, l, st); if (rc) return rc;
    HLev &V = H->lev[l];
    m.dv = V.d_dv; m.fp = V.d_fp; m.nbox = (int)V.box.size(); m.maxnx = V.maxnx; m.maxny = V.maxny; m.red = V.d_red;
    m.push = V.push.d; m.pbase = V.pbase.d; m.merged = H->merged_launches; m.ph = V.box[0]->ph;
    if (V.part) { m.dv += V.b0; m.fp += V.b0; m.nbox = V.nown; m.push = nullptr; m.pbase = nullptr; }   // owner computes: the tables from this rank's first box
    return 0;
}
// level l as the target of one launcher: f(on_level(base, 0)) for level 0, f(all boxes of level l) for l >= 1 (f: a generic lambda)
template <class F> inline int on_hier_level(suhmo_hier *H, int l, hipStream_t st, F &&f)
{
    if (l == 0) return f(on_level(base_of(H), 0));
    suhmo_multi m;
    int rc = multi_of(H, l, st, m);
    return rc ? rc : f(m.on());
}
// the launchers of the plans (what each does: at its definition)
int hier_ff(suhmo_hier *H, int l, int f0, int f1, bool corners, hipStream_t st, int colour = -1);
int hier_cf(suhmo_hier *H, int l, int ff, int fc, hipStream_t st, int ff1 = -1, int fc1 = -1);
int hier_cf_ff(suhmo_hier *H, int l, int ff, int fc, int ff1, int fc1, bool corners, hipStream_t st);
int hier_pwl(suhmo_hier *H, int l, int ff, int fc, hipStream_t st);
int hier_ff_on(suhmo_hier *H, int l, const FP *tab, int f0, int f1, bool corners, hipStream_t st);
int hier_pwl_on(suhmo_hier *H, int l, const FP *ftab, int ff, const FP *ctab, const FP &cbase, int use_base, int fc, hipStream_t st);
int hier_avg(suhmo_hier *H, int l, int ff, int fc, int mode, double val, hipStream_t st);
int hier_window_save(suhmo_hier *H, int l, int field_c, hipStream_t st);
int hier_prolong2(suhmo_hier *H, int l, int field_c, hipStream_t st, bool minus_saved = false, bool leave_below = false);
int hier_reflux(suhmo_hier *H, int l, int field_c, hipStream_t st, int residual = 0);
int ghosts_levels(suhmo_hier *H, int llo, int lhi, suhmo_stream_t s);
int reflux_levels(suhmo_hier *H, int lhi, int llo, bool average_down, suhmo_stream_t s);
int cover_whole_base(suhmo_hier *H);
}  // namespace hier

// ---- suhmo_hier.hip: what the time step (suhmo_step.hip) needs besides the plans
void suhmo_hier_invalidate_(suhmo_hier *H);                                         // an entry point outside suhmo_hier.hip: the caller may have loaded new data
// MAX over the ranks of a value each computed on its own boxes; the all-gather of the hierarchy (device buffers, `count` doubles per rank)
int suhmo_hier_allreduce_max_(suhmo_hier *H, double *v);
int suhmo_hier_allgather_(suhmo_hier *H, const double *send, long count, double *recv, hipStream_t st);
// the hierarchy of SolveForGap_nl: the same boxes, alpha = 1, beta = dt diffFactor, Neumann-0 sides, no nonlinear term
int suhmo_hier_gap_(suhmo_hier *H, const suhmo_model_params_t *mp, double dt, suhmo_hier **gap);
// ---- suhmo_hier.hip: what the regrid (suhmo_regrid.hip) needs of the creation path
// suhmo_hier_create_opts around an EXISTING base level handle (adopt != NULL: borrowed until the caller settles who owns it, base_borrowed)
int suhmo_hier_create_on_(suhmo_hier **out, const suhmo_level_desc_t *base, suhmo_level *adopt, int nlev, const int *nbox, const int *boxes, const char *options);
std::string suhmo_hier_options_(const suhmo_hier *H);                               // the options as they are now, "key=value,..."
int suhmo_hier_check_(suhmo_hier *H);                                               // what every C-ABI entry of a hierarchy does first
// ---- what the run of a hierarchy (suhmo_run.hip) needs of the time step, the forcing and the diagnostics
int suhmo_step_check_args_(const suhmo_model_params_t *mp, double dt, int cur_step);   // suhmo_step.hip
// suhmo_forcing.hip
int suhmo_hier_recharge_check_(suhmo_hier *H, const char *who);                      // rank strips: -5; a box without SUHMO_F_ZS: -1, naming it
int suhmo_hier_recharge_launch_(suhmo_hier *H, double T_K, double background_input, hipStream_t st);      // one launch per level
// suhmo_postproc.hip
int suhmo_level_postproc_row_check_(suhmo_level *L, const suhmo_model_params_t *mp, bool forcing_writes_source);
int suhmo_level_postproc_row_launch_(suhmo_level *L, const suhmo_model_params_t *mp, double *cols, double *out6, hipStream_t st);
// ---- what suhmo_step.hip and suhmo_forcing.hip share: the cells of a region that do not count (a finer level covers them), and the check
// of nested levels (suhmo_amr.hip)
struct Excl { int i0, j0, i1, j1; };       // local cells [i0, i1) x [j0, j1)
int suhmo_amr_check_hierarchy(suhmo_level_t **lv, int nlev);
// ---- suhmo_snap.hip: what the run needs of the snapshot -- its refusals, and the offsets (level_offset [nlev + 1], box_offset, either may be NULL) -> doubles in all
int suhmo_hier_snapshot_check_(const suhmo_hier *H, const char *who, int ncomp, const suhmo_snap_comp_t *comps, int ghost);
long suhmo_hier_snapshot_sizes_(const suhmo_hier *H, int ncomp, int ghost, long *level_offset, long *box_offset);
// ---- suhmo_flatten.hip: its scratch and finest array go with the hierarchy
void suhmo_hier_flatten_release_(suhmo_hier *H);
// ... and what suhmo_compare.hip needs of it: the component list checked (who: the entry point the message names), the refusals that depend on
// max_level, and the device part of a flatten -- steps (i) to (iii), the finest array left in H->flat_buf, nothing copied
struct FlatComps { int n; int kind[SUHMO_FLAT_MAX_COMPS], f1[SUHMO_FLAT_MAX_COMPS], f2[SUHMO_FLAT_MAX_COMPS]; };
int suhmo_flat_comps_(const char *who, int ncomp, const suhmo_flat_comp_t *comps, FlatComps &c);
int suhmo_hier_flatten_check_(const suhmo_hier *H, int max_level);
int suhmo_hier_flatten_device_(suhmo_hier *H, int max_level, const FlatComps &c, hipStream_t st);
// ---- suhmo_compare.hip: its partial buffer goes with the hierarchy
void suhmo_hier_compare_release_(suhmo_hier *H);
// ---- suhmo_balance.hip: likewise (the buffers of the mass balance and of the water budget)
void suhmo_hier_balance_release_(suhmo_hier *H);
// ---- suhmo_balance.hip, "WATER BUDGET": what the time steps (suhmo_step.hip) and the run (suhmo_run.hip) need of it
int suhmo_level_track_volume_(suhmo_level *L, hipStream_t st);                      // k_volume of a level into L->vol_buf (rank strips: -5)
int suhmo_hier_track_volume_(suhmo_hier *H, hipStream_t st);                        // ... of every level of H into H->vol_buf: nlev launches
// what suhmo_hier_water_budget refuses (faces: the face coefficients and SUHMO_F_MR are asked for too -- a run leaves them to its first step;
// source: use_moulin_source needs SUHMO_F_MSRC on every box now)
int suhmo_hier_budget_check_(const suhmo_hier *H, const suhmo_model_params_t *mp, const char *who, bool faces, bool source);
// the nlev first stages and the final launch: ten doubles per level to the DEVICE address out; nothing copied, nothing synchronised
int suhmo_hier_budget_launch_(suhmo_hier *H, const suhmo_model_params_t *mp, double *out, hipStream_t st);
