// suhmo_common.h -- internal types shared by the HIP translation units of libsuhmo_hip.so.
// gfx950 (MI355X) only; compiled with -ffp-contract=off so that every kernel reproduces
// the reference's Fortran expression association bit for bit ("Parity").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <string>
#include <vector>
#include "../../include/suhmo_hip.h"

#define SUHMO_XOFF 16      // column of cell i = 0 in a canvas row (128-byte aligned)
#define SUHMO_MAXDEPTH 16

// Level canvas geometry + boundary description of one multigrid depth, passed by value to
// kernels.  Canvas element of cell/face (i,j): (j + gy) * P + XOFF + i.  Every field of a
// depth (cell-centred, x-faces, y-faces) uses the same canvas shape.
struct DV {
    int nx, ny;        // cells of this strip at this depth
    int P;             // pitch in doubles (multiple of 16)
    int gy;            // ghost rows below / above
    int rows;          // ny + 2*gy
    int j0, nyg;       // global row of local j = 0; rows of the whole level (colour parity, faces)
    double dx, dy;     // cell size
    double rdx, rdy;   // one/(dx*dx), one/(dy*dy)   (src/VCAMRNonLinearPoissonOpF.ChF:110)
    double fdx, fdy;   // one/dx, one/dy             (util/GradientF.ChF:57)
    double alpha, beta;
    int bct[2][2];     // [dir][side] 0 Dirichlet, 1 Neumann
    double two_v[2][2];// 2.0*value               (DiriBC order 1: 2*value - near)
    double neu[2][2];  // (sign*dx)*value         (NeumBC: near + sign*dx*value)
    int per[2];        // periodic
    int ext[2];        // y side is a rank boundary or a coarse-fine side: ghost rows hold data
    int i0, nxg;       // AMR patch: global column of local i = 0, columns of the whole (refined) domain
    int cfx[2];        // x side is a coarse-fine side: ghost columns hold interpolated data
    int rk[2];         // y side is a RANK boundary (halo rows exchanged with a neighbour); ext && !rk = coarse-fine side
};

struct FP { double *f[SUHMO_F_COUNT]; };

__host__ __device__ __forceinline__ int cidx(const DV &v, int i, int j)
{
    return (j + v.gy) * v.P + SUHMO_XOFF + i;
}

// ---- neighbour values of phi with the physical BC / periodic wrap applied on the fly ----
// mixBCValues (src/AmrHydro.cpp:248-309): ghost = 2*value - near (Dirichlet, order 1) or
// near + sign*dx*value (Neumann); the ghost depends only on the adjacent interior cell, so
// it is recomputed from registers instead of being stored between colour passes.
__device__ __forceinline__ double phiW(const DV &v, const double *__restrict__ p, int idx, int i, double c, bool homog)
{
    if (i > 0 || v.cfx[0]) return p[idx - 1];
    if (v.per[0]) return p[idx + v.nx - 1];
    if (v.bct[0][0] == 0) return (homog ? 0.0 : v.two_v[0][0]) - c;
    return homog ? c : c + v.neu[0][0];
}
__device__ __forceinline__ double phiE(const DV &v, const double *__restrict__ p, int idx, int i, double c, bool homog)
{
    if (i < v.nx - 1 || v.cfx[1]) return p[idx + 1];
    if (v.per[0]) return p[idx - (v.nx - 1)];
    if (v.bct[0][1] == 0) return (homog ? 0.0 : v.two_v[0][1]) - c;
    return homog ? c : c + v.neu[0][1];
}
__device__ __forceinline__ double phiS(const DV &v, const double *__restrict__ p, int idx, int j, double c, bool homog)
{
    if (j > 0 || v.ext[0]) return p[idx - v.P];
    if (v.per[1]) return p[idx + (v.ny - 1) * v.P];
    if (v.bct[1][0] == 0) return (homog ? 0.0 : v.two_v[1][0]) - c;
    return homog ? c : c + v.neu[1][0];
}
__device__ __forceinline__ double phiN(const DV &v, const double *__restrict__ p, int idx, int j, double c, bool homog)
{
    if (j < v.ny - 1 || v.ext[1]) return p[idx + v.P];
    if (v.per[1]) return p[idx - (v.ny - 1) * v.P];
    if (v.bct[1][1] == 0) return (homog ? 0.0 : v.two_v[1][1]) - c;
    return homog ? c : c + v.neu[1][1];
}

// COMPUTENONLINEARTERMS, src/AmrHydroF.ChF:38-65
__device__ __forceinline__ void nl_terms(const suhmo_phys_t &ph, double phi, double B, double Pi,
                                         double zb, double mask, double &nl, double &dnl)
{
    if (!ph.use_NL || mask < 0.0) { nl = 0.0; dnl = 0.0; return; }
    double N = Pi - ph.rho_w_g * (phi - zb);
    nl = -ph.A * B * N * N * N;
    dnl = 3.0 * ph.A * B * 1000.0 * ph.grav * N * N;
    if (ph.cutOffbr > B) {
        nl = nl * (1.0 - (ph.cutOffbr - B) / ph.cutOffbr);
        dnl = dnl * B / ph.cutOffbr;
    }
    if (ph.maxOffbr < B) {
        nl = nl * (1.0 - (ph.maxOffbr - B) / ph.maxOffbr);
        dnl = dnl * B / ph.maxOffbr;
    }
}

// L(phi) at one cell, src/VCAMRNonLinearPoissonOpF.ChF:130-152 / 257-279.  `aterm` is
// alpha*aCoef(i,j) (or alpha alone when alpha == 0 and aCoef is not read).
__device__ __forceinline__ double lofphi_cell(const DV &v, double aterm, double c, double e, double w,
                                              double n, double s, double bxE, double bxW, double byN,
                                              double byS, double nl)
{
    return aterm * c
           - v.beta * (bxE * (e - c) * v.rdx - bxW * (c - w) * v.rdx
                       + byN * (n - c) * v.rdy - byS * (c - s) * v.rdy)
           + nl;
}

// lambda, resetLambda + SUMFACESNL (src/VCAMRNonLinearPoissonOp.cpp:517-528, ...OpF.ChF:591-598)
__device__ __forceinline__ double lambda_cell(const DV &v, double aterm, double bxE, double bxW,
                                              double byN, double byS)
{
    double lam = aterm;
    lam = lam + v.rdx * v.beta * (bxE + bxW);
    lam = lam + v.rdy * v.beta * (byN + byS);
    return lam;
}

// WFlx_level's arithmetic on values, shared by every kernel that forms face coefficients (suhmo_bcoef.hip: the four-kernel path and
// k_bcoef_fused; suhmo_gsrb.hip: the relaxation launch that forms depth 0's faces itself).
// Cell-centred gradient = EdgeToCell(NEWMACGRAD) (util/GradientF.ChF:57-70); z*: the face gradient is masked out (use_mask_gradients)
__device__ __forceinline__ void gradcc_from(const DV &v, double c, double w, double e, double s, double n, bool zW, bool zE, bool zS,
                                            bool zN, double &gx, double &gy)
{
    double gW = v.fdx * (c - w), gE = v.fdx * (e - c), gS = v.fdy * (c - s), gN = v.fdy * (n - c);
    if (zW) gW = 0.0;
    if (zE) gE = 0.0;
    if (zS) gS = 0.0;
    if (zN) gN = 0.0;
    gx = 0.5 * (gW + gE);
    gy = 0.5 * (gS + gN);
}
// COMPUTERE (src/AmrHydroF.ChF:92-109) in two steps: the norm of the gradient, then Re from it and the gap height
__device__ __forceinline__ double grad_norm(double gx, double gy) { return sqrt(gx * gx + gy * gy); }
__device__ __forceinline__ double re_from(const suhmo_phys_t &ph, double sg, double B)
{
    double discr = 1.0 + 4.0 * ph.omega * (B * B * B * ph.grav * sg) / (12.0 * ph.nu * ph.nu);
    return (-1.0 + sqrt(discr)) / (2.0 * ph.omega);
}
// CellToEdge(Re), CellToEdge(B), setup_iceMask_EC, COMPUTEBCOEFF (src/AmrHydro.cpp:1512-1537, src/HydroIBC.cpp:139-184,
// src/AmrHydroF.ChF:212-228): the face between cell c and the cell m below / left of it
__device__ __forceinline__ double bcoef_face(const suhmo_phys_t &ph, double Rc, double Rm, double Bc, double Bm,
                                             double mc, double mm, bool dom_edge)
{
    double Ref = 0.5 * (Rc + Rm), Bf = 0.5 * (Bc + Bm);
    double mec;
    if (fabs(mc - mm) < 1e-10) mec = (mc > 0.0) ? 1.0 : -1.0; else mec = 0.0;
    if (dom_edge) mec = 0.0;
    double num_q = -(Bf * Bf * Bf * ph.grav);
    double denom_q = 12.0 * ph.nu * (1.0 + ph.omega * Ref);
    if (mec < 0.0 && ph.cutOffB > 0) return 0.0;
    return num_q / denom_q;
}

struct Depth {
    DV v;
    FP fp;
    size_t elems;      // doubles per canvas
    int nbox;
    int prolong_pending; // the next fused relax adds P(phi_c - phi_c,old) while loading phi (FAS prolongIncrement)
    int rhs_pending;     // the next tile relax forms the FAS right-hand side rhs = res + L(phi) while loading (and PHIOLD, LPHI)
    int bcoef_pending;   // depth 0: the next streaming relax forms the face coefficients from phi as loaded (UpdateOperator) and stores them
    double *phi_alt;   // second phi canvas: the fused GSRB kernel writes out of place (ping-pong)
    int phi_fresh;     // strips: halo rows of phi (each rank-boundary side) that hold the neighbour's CURRENT values
    int zb_state;      // what is known about the depth's bed elevation (suhmo_level::zb_known): SUHMO_ZB_UNKNOWN / _UNIFORM / _VARYING
    double zb_value;   // _UNIFORM: the value of every cell
};

struct VGraph {                 // a V-cycle captured for one set of solver parameters and one state of the phi ping-pong (suhmo_fas.hip)
    int key[4]; hipGraphExec_t exec;
    double *p0[SUHMO_MAXDEPTH], *a0[SUHMO_MAXDEPTH];     // PHI / second canvas of every depth when the cycle starts ...
    double *p1[SUHMO_MAXDEPTH], *a1[SUHMO_MAXDEPTH];     // ... and when it ends (an odd number of out-of-place launches on a depth swaps them)
    double *rhs;                                         // right-hand-side canvas of depth 0 the cycle was captured with
    int rout_req, rout_done, rout_np; const double *rout_rhs;     // the residual its last launch was asked to leave behind (resout_req, resout_rhs) and did
    int bcoef_in_relax; long n_bcoef_in_relax;                    // captured with the option (part of the key); its launches that form depth 0's faces
    int mask_clean; long n_bcoef_unmasked, n_relax_unmasked;      // captured with the ice mask known clean (part of the key); its launches that leave the mask out
    // captured with these depths' bed known uniform (bit d; part of the key, and with any bit set the count of writes to the bed too: the
    // launches carry the VALUE); its launches per depth that take the bed as a scalar
    unsigned zb_uniform, zb_version; long n_relax_zb[SUHMO_MAXDEPTH];
    int yface_ring; long n_relax_yring[SUHMO_MAXDEPTH];           // captured with this yface_ring (part of the key); its launches per depth with one ring of y-faces
    int has_scan;                                                 // its (masked) k_bcoef_fused also writes the scan word: a launch of it can carry a scan of the mask
};
struct ProfEv { hipEvent_t a, b; long cells; int restricts; };   // restricts: 1 the launch also did the restriction (RST), 2 it also formed the face coefficients (BCF: neither read counts it)

struct suhmo_level {
    int ndepth;
    int batch_owned;            // a member of a batch (suhmo_batch.hip): suhmo_level_destroy refuses it
    int stub;                   // geometry only: no canvas, no scratch (a box of a partitioned AMR level held by other ranks; suhmo_hier_plan.hip)
    Depth d[SUHMO_MAXDEPTH];
    suhmo_level_desc_t desc;
    std::vector<int> boxes;     // nbox x 4, global indices, depth 0
    suhmo_phys_t ph;
    int device;
    double *scratch;            // reduction scratch (device)
    double *hscratch;           // pinned host scratch
    double *hscratch_dev;       // its device address: the last kernel of a reduction writes the result and a sequence number there
    unsigned long long hseq;    // and the host polls for the number instead of synchronising the stream (env SUHMO_POLL_READBACK, default 1)
    int poll_readback;
    size_t scratch_elems;
    suhmo_exchange_fn ex;
    suhmo_allreduce_max_fn ar;
    suhmo_allreduce_fn ar2;                            // n values, MAX or SUM, on the host (suhmo_level_set_reduce_hook)
    int (*ard)(void *user, double *dev_values, int n, int op, suhmo_stream_t s);   // the same in place on DEVICE values, enqueued on s (native transport)
    void *user;
    int (*ex_begin)(void *user);                       // optional: open / close a batch of exchanges that
    int (*ex_end)(void *user, suhmo_level *L, suhmo_stream_t s);   // travel as ONE message group (native transport)
    long graph_max_cells;        // V-cycles of levels up to this size are replayed as HIP graphs (env SUHMO_GRAPH_MAX_CELLS, 0 = off)
    std::vector<VGraph> vgraphs; int vgraph_seen[4]; hipStream_t gstream;
    long vgraph_replays;         // V-cycles that ran as a launch of a captured graph (read-only option vcycle_graph_replays)
    suhmo_level *gap; double gap_dt;   // implicit gap-height operator of the time step (suhmo_step.hip), owned
    void *rccl;                 // native transport state (suhmo_rccl.hip), owned by the level
    int faces_deferred;         // rank strips: UpdateOperator left the halo rows of the depth-0 faces to the message that carries the coarse depths' (suhmo_average_operator_all)
    void *ipc; int ipc_owner;   // peer-direct halo transport (suhmo_ipc.hip): arena and neighbours' mappings; a gap-height handle borrows its level's
    // agglomeration of the coarse depths of a rank strip (suhmo_agg.hip): from depth agg_depth on (0 = none) the cycle runs on `agg`, a
    // handle of the WHOLE level at that depth held by every rank; all-gather transport ag (suhmo_level_set_allgather / attach_rccl)
    long agg_min_cells;         // depths whose strip holds fewer cells are agglomerated (env SUHMO_AGG_MIN_CELLS, default 100000: at 4096^2 cells per strip the two deepest of six depths; 0 = off)
    int agg_depth, agg_world, agg_rank;
    suhmo_level *agg;
    int agg_static_stale;       // A was (re)created after the last coefficient build: its B / Pi / zb / mask / aCoef / faces are gathered before the cycle enters it
    suhmo_allgather_fn ag; void *ag_user;
    double *agg_send, *agg_recv; size_t agg_cap; long agg_gathers;
    // the solve loops ask the cycle to leave the residual of its final phi behind (suhmo_gsrb.hip, RM = 2): resout_req bit 0 RES, bit 1 LPHI
    // too; resout_rhs: the right-hand side it is about (NULL: the level's); resout_armed: set by the cycle around its last relax of depth 0;
    // resout_done: the launch did it (else the caller runs its own pass); read-only option residual_in_relax_launches counts them
    int resout_req, resout_armed, resout_done; const double *resout_rhs; long resout_count;
    int resout_np;              // resout_req bit 2: the launch also left that many partial maxima of |RES| in scratch + 2 (k_norm_final's input)
    // UpdateOperator of the V-cycle inside the first pre-smoothing launch of depth 0 (suhmo_gsrb.hip, BCF; option bcoef_in_relax, default 1);
    // bcoef_nd: the depths AverageOperator refreshes right behind that launch; read-only option bcoef_in_relax_launches counts them
    int bcoef_in_relax, bcoef_nd; long bcoef_in_relax_count;
    // AverageOperator behind that launch on a side stream, beside the next launch of depth 0, which reads none of its output (option avg_overlap,
    // default 1; suhmo_gsrb_can_overlap_avg); avg_fork: this cycle may fork (vcycle_body); avg_flying: the coarse faces are in flight on
    // astream -- suhmo_avg_join makes a stream wait for them; read-only option avg_overlap_launches counts the forks
    int avg_overlap, avg_fork, avg_flying; long avg_overlap_count;
    hipStream_t astream; hipEvent_t aev[2];
    long frhs_stream, frhs_tile;   // launches that formed a coarse depth's FAS right-hand side themselves (streaming / tile kernel); read-only options
    // what the relaxation scheduler did on a rank strip (suhmo_launch_gsrb, suhmo_prolong_with_halo); read-only options strip_*
    long strip_tile, strip_tile_rst, strip_tile_shallow, strip_colour, strip_stream, strip_stream_rst, strip_prolong_unfused;
    int prof_on;
    std::vector<ProfEv> prof;
    int gsrb_variant;           // kernel selection (see suhmo_gsrb.hip); env SUHMO_GSRB_VARIANT
    long fused_min_cells;       // auto mode: use the fused kernel from this many cells (env SUHMO_FUSED_MIN_CELLS)
    int bcoef_fused;            // single-kernel WFlx_level (env SUHMO_BCOEF_FUSED, default 1)
    int bcoef_tile_x;           // its tile width: 62 (64 x 4 threads) or 126 (128 x 2 threads); env SUHMO_BCOEF_TILE_X
    int fused_nt;               // threads per workgroup of the fused kernel: 256 or 64 (env SUHMO_FUSED_NT)
    int fused_restrict;         // the last pre-smoothing launch also restricts (env SUHMO_FUSED_RESTRICT, default 1)
    int fused_hc;               // rows per chunk of the fused kernel (0 = auto); env SUHMO_FUSED_HC
    int fas_rhs_fused;          // coarse FAS right-hand side rhs = res + L(R phi), the copy of R phi and L(phi) in ONE pass (k_apply<., 2>) instead of
                                // copy + applyOp + axby (env SUHMO_FAS_RHS_FUSED, default 1)
    int strips_rhs_local;       // rank strips: R phi and RES travel together, the coarse right-hand side of the halo rows is computed locally
                                // (env SUHMO_STRIPS_RHS_LOCAL, default 1)
    int skip_mask;              // the streaming relaxation skips the ice-mask array in a V-cycle whose UpdateOperator found no negative cell
                                // (env SUHMO_SKIP_MASK, default 1)
    int mask_reported;          // the last suhmo_level_update_operator(depth 0) made that report
    int coarse_mask_ok;         // the ice masks of the depths > 0 are MGnewOp's averages of depth 0's current one (suhmo_build_mg_coefficients; any
                                // write to the field clears it): the report about depth 0 then covers them (an average of non-negative cells)
    unsigned mask_epoch, maskflag_epoch;   // number of the last k_bcoef_fused call on depth 0; the call whose report is current (0: none)
    // what is known about the ice mask ACROSS cycles (option mask_known, default 1; 0: only the per-cycle report above).  The mask is caller
    // data: it changes through the entry points that write SUHMO_F_MASK (suhmo_mask_written) and, on a rank strip, through the halo rows an
    // exchange brings (suhmo_mask_halo_written); between two writes what one scan found stays true.  CLEAN: every value k_bcoef_fused can
    // read at depth 0 -- the level's cells, the stored ghost ring on the Re range, a strip's halo rows with their ghost columns -- is >= 1e-6,
    // so `mask < 0`, `mask < 1e-6` and bcoef_face's early return are all constant there (and on the coarse depths while coarse_mask_ok
    // holds: averages of such values, Neumann / periodic ghosts); DIRTY: the scan met a smaller value.  The first k_bcoef_fused after a write
    // scans (widened report into a second device word), a 4-byte copy into pinned memory and an event follow it on the stream, and later
    // launches ask the event (hipEventQuery: never a wait); until the answer is there everything runs as without the option.
    int mask_known, mask_state;            // SUHMO_MASK_UNKNOWN / _CLEAN / _DIRTY
    unsigned mask_version, mask_scan_version;   // writes so far; the one the scan in flight (mask_scan_pending) looked at
    int mask_scan_pending, mask_capturing;      // (mask_capturing: inside a graph capture -- the masked kernels get the scan word, the host-side clear / copy / event stay outside)
    int mask_scan_captured;                     // ... and such a kernel was captured (VGraph::has_scan)
    int mask_view;                              // the caller holds a writable device pointer to the mask (suhmo_level_field_view): nothing about it is ever known
    int mask_scan_errors;                       // event queries that failed for good (not "not ready"): after three the level stops scanning
    unsigned *mask_host; hipEvent_t mask_ev;    // pinned word the scan's answer arrives in (0: nothing below 1e-6), the event behind the copy
    long mask_scans, bcoef_unmasked, relax_unmasked;   // read-only options mask_scans, bcoef_unmasked_launches, relax_unmasked_launches
    // what is known about the BED ELEVATION across cycles (option zb_known, default 1; 0: nothing is scanned, every launch loads the array).
    // zb is caller data like the mask: it changes through the entry points that write SUHMO_F_ZB on any depth (suhmo_zb_written) and through
    // MGnewOp's averages (suhmo_build_mg_coefficients); between two writes what one scan found stays true.  UNIFORM: the level's own cells of
    // the depth -- all a streaming launch of a whole level reads -- hold ONE bit pattern (compared as 64-bit integers: -0.0 is not +0.0, a NaN
    // equals itself), kept in Depth::zb_value; VARYING: they do not.  Every depth is scanned on its own (an average (c + c + c + c) / 4 is c
    // for many values, not for all).  The first V-cycle after a write launches the scan (k_zb_scan, one launch per depth), a copy of the
    // answers into pinned memory and an event follow on the stream, later cycles ask the event (hipEventQuery: never a wait); until the answer
    // is there everything runs as without the option.  zb_off: nothing is ever known -- the caller holds a writable pointer
    // (suhmo_level_field_view), or the level serves a hierarchy, an ensemble or the agglomerated depths of a rank strip.
    int zb_known, zb_off;
    unsigned zb_version, zb_scan_version;       // writes so far; the one the scan in flight (zb_scan_pending) looked at
    int zb_scan_pending, zb_scan_errors;        // (errors: event queries that failed for good; after three the level stops scanning)
    unsigned long long *zb_dev, *zb_host;       // per depth two words, [2 d] differing cells seen, [2 d + 1] the first cell's bits: on the device, in pinned memory
    hipEvent_t zb_ev;
    long zb_scans, relax_zb_uniform[SUHMO_MAXDEPTH];   // read-only options zb_scans, relax_zb_uniform_launches (+ _d<depth>)
    int yface_ring;             // 1 (default): the plain two-sweep streaming launch with the bed as a scalar keeps one ring of y-faces and three waves
                                // per SIMD (not on y-periodic levels); 0: two rings, two waves, the chunk heights of those (env SUHMO_YFACE_RING;
                                // same bits)
    long relax_yring[SUHMO_MAXDEPTH];                  // read-only options relax_yring_launches (+ _d<depth>)
    int overlap_halo;           // rank strips, streaming kernel: the halo exchange travels on a second stream while the chunks that do not
                                // read halo rows relax; the two end chunks follow (env SUHMO_OVERLAP_HALO; 1 = default: with the native, stream-ordered
                                // RCCL transport only; 2 = with any hook, the caller vouches that it orders against the stream it is given; 0 = off)
    hipStream_t xstream; hipEvent_t xev[2]; long overlapped;   // ... its stream and events; launches that overlapped so far
    int tile_strips;            // tile kernel on rank strips (env SUHMO_TILE_STRIPS, default 1)
    int tile_chunks;            // a level that is one tile relaxes all its sweeps in one launch (env SUHMO_TILE_CHUNKS, default 1)
    int resid_in_relax;         // the solve loops' residual evaluation rides on the launch that ends the V-cycle (streaming kernel at depth 0; default 1)
    int fas_rhs_in_relax;       // coarse FAS right-hand side formed by the first relax of the depth: bit 0 in the tile kernel, bit 1 in the streaming kernel (env SUHMO_FAS_RHS_IN_RELAX, default 3)
    long tile_max_cells;        // auto mode: levels below this many cells relax on the tile kernel (env SUHMO_TILE_MAX_CELLS)
    int tile_restrict;          // the tile kernel's last pre-smoothing launch also restricts: 0 never (a separate kernel restricts: faster on one GPU and
                                // on a rank strip alike, profiles/r02_h_tile_restrict_ab.txt), 1 always, 2 on rank strips only (env SUHMO_TILE_RESTRICT, default 0)
    int tile_order;             // workgroup -> tile map of the tile kernel: 0 as launched, 1 a contiguous run of tiles per XCD, 2 the same in panels of 8 tile rows (env SUHMO_TILE_ORDER)
    // bottom solver (suhmo_bottom.hip): 1 = Chombo's RelaxSolver after the bottom relaxes of every cycle (option bottom_solver, default 0);
    // bottoms of up to bottom_one_launch_max_cells cells that fit the LDS run it in one launch (option / env SUHMO_BOTTOM_ONE_LAUNCH_MAX_CELLS,
    // 0 = always the host loop); bottom_ctr: device counters (iterations, one-launch solves); the host loop counts on the host
    int bottom_solver; long bottom_one_launch_max_cells;
    unsigned long long *bottom_ctr; long bottom_host_iters, bottom_host_solves;
    int gsrb_tile, tile_t, tile_s;      // cache-resident depths: S sweeps per launch on LDS tiles (env SUHMO_GSRB_TILE, default 1); tile edge 16 / 32
                                // (env SUHMO_TILE_T, 0 = by size)
    struct suhmo_tagmap *tags;  // tag map of suhmo_level_tag_cells (suhmo_tags.hip), owned; NULL until the first call
    int faces_made;             // depth 0's face coefficients have been formed (UpdateOperator in any of its forms, the time step) or loaded by the
                                // caller at least once: what the mass balance (suhmo_balance.hip) asks before it reads them (suhmo_faces_made)
    double *bal_buf;            // suhmo_level_mass_balance: the partials of its first stage and, behind them, its seven sums; allocated on first use
    // "WATER BUDGET" (suhmo_balance.hip).  track_old_volume: option, 1 = suhmo_level_timestep begins with k_volume into vol_buf (vol_np partials;
    // 0: no tracked step has run); wb_buf: the partials of suhmo_level_water_budget and, behind them, its ten values.  Allocated on first use
    int track_old_volume, vol_np;
    double *vol_buf, *wb_buf;
};
static inline void suhmo_faces_made(suhmo_level *L) { L->faces_made = 1; }

enum { SUHMO_MASK_UNKNOWN = 0, SUHMO_MASK_CLEAN = 1, SUHMO_MASK_DIRTY = 2 };
// a write to the ice mask of the level's cells or ghost ring: the coarse masks are no longer its averages, no report about it holds
static inline void suhmo_mask_written(suhmo_level *L)
{
    L->coarse_mask_ok = 0; L->maskflag_epoch = 0;
    L->mask_version++; L->mask_state = SUHMO_MASK_UNKNOWN;
}
// a write to the halo rows of a rank strip's mask only (the neighbours' cells): the strip's own averages stand, what a scan found does not
static inline void suhmo_mask_halo_written(suhmo_level *L) { L->mask_version++; L->mask_state = SUHMO_MASK_UNKNOWN; }
enum { SUHMO_ZB_UNKNOWN = 0, SUHMO_ZB_UNIFORM = 1, SUHMO_ZB_VARYING = 2 };
// a write to the bed elevation of any depth (cells, ghost ring or halo rows): nothing about it holds any more
static inline void suhmo_zb_written(suhmo_level *L)
{
    L->zb_version++;
    for (int d = 0; d < SUHMO_MAXDEPTH; d++) L->d[d].zb_state = SUHMO_ZB_UNKNOWN;
}
// the streaming relaxation of `depth` may take the bed as a scalar (whole levels: no rank strip, no AMR patch)
static inline bool suhmo_zb_uniform(const suhmo_level *L, int depth)
{
    return L->zb_known && !L->zb_off && L->d[depth].zb_state == SUHMO_ZB_UNIFORM && !L->ex && L->desc.nx_global == 0;
}
void suhmo_zb_poll(suhmo_level *L);                       // suhmo_level.hip: takes the answer of a scan up if it has arrived
int suhmo_zb_scan_if_due(suhmo_level *L, hipStream_t st); // suhmo_level.hip: launches the scan when nothing is known and none is in flight
bool suhmo_gsrb_streams(const suhmo_level *L, int depth); // suhmo_gsrb.hip: the depth's relaxation runs on the streaming kernel
int suhmo_gsrb_stream_wg_per_cu(const char *which, long *value);   // suhmo_gsrb.hip: read-only options stream_wg_per_cu_<which>; 1: no such name
bool suhmo_mask_would_scan(const suhmo_level *L);   // suhmo_bcoef.hip: the next UpdateOperator of depth 0 scans the mask
// the two device words behind the reductions' scratch (its last double): [0] the per-cycle report "a negative cell" (= the epoch), [1] the scan
// "a value below 1e-6"; the scan's answer arrives in the pinned scratch at double SUHMO_HSCRATCH_MASK (the reductions use [0, 16))
#define SUHMO_HSCRATCH_DOUBLES 64
#define SUHMO_HSCRATCH_MASK 60
#define SUHMO_HSCRATCH_ZB 16       // 2 x SUHMO_MAXDEPTH words: the answers of a scan of the bed elevation
static inline unsigned *suhmo_mask_report_word(const suhmo_level *L) { return (unsigned *)(L->scratch + L->scratch_elems - 1); }
static inline unsigned *suhmo_mask_scan_word(const suhmo_level *L) { return suhmo_mask_report_word(L) + 1; }
int suhmo_mask_scan_begin(suhmo_level *L, hipStream_t st);   // suhmo_bcoef.hip: clears the scan word on st ...
int suhmo_mask_scan_end(suhmo_level *L, hipStream_t st);     // ... and, behind the kernels that set it, the copy to pinned memory and the event
void suhmo_mask_poll(suhmo_level *L);      // suhmo_bcoef.hip: takes the answer of a scan up if it has arrived
// the relaxation of `depth` may leave the mask out altogether (levels and rank strips, not AMR patches; the coarse depths while their masks
// are depth 0's averages)
static inline bool suhmo_mask_clean(const suhmo_level *L, int depth)
{
    return L->mask_known && !L->mask_view && L->mask_state == SUHMO_MASK_CLEAN && (depth == 0 || L->coarse_mask_ok) && L->desc.nx_global == 0;
}
void suhmo_set_error(const char *fmt, ...);
void suhmo_tagmap_release(struct suhmo_tagmap *m);   // suhmo_tags.hip (NULL: nothing)
// Named scoped timers with the reference's CH_TIME labels (src/VCAMRNonLinearPoissonOp.cpp:40,69,103,277,390,660; report =
// CH_TIMER_REPORT, exec/A_SHMIP/Suhmo.cpp:136).  Off by default (one relaxed load per scope); suhmo_timers_enable(1): host wall
// time per scope, (2): the device is synchronised at both ends, so the time includes the kernels the scope launched.
struct SuhmoTimer { const char *name; double t0; int mode; explicit SuhmoTimer(const char *n); ~SuhmoTimer(); };
#define SUHMO_TIME(label) SuhmoTimer suhmo_tm_(label)
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    suhmo_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return -2; } } while (0)
#define ARG(cond) do { if (!(cond)) { suhmo_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, #cond); return -1; } } while (0)

double *suhmo_field(suhmo_level *L, int depth, int field);   // lazily allocates
int suhmo_level_create_(suhmo_level_t **out, const suhmo_level_desc_t *desc, bool stub);   // suhmo_level.hip
// dst uses src's transport hooks (exchange, reductions, peer-direct arena): a gap-height handle and the level it solves for
void suhmo_level_share_transport(suhmo_level *dst, const suhmo_level *src);   // suhmo_level.hip
int suhmo_level_materialize_(suhmo_level *L);
// Two canvases of a level trade places while its FAS problem runs (the level's own right-hand side is set aside): whatever way the
// scope is left -- an exchange or all-gather hook failing in between included -- they trade back, so a caller that catches the
// error still holds the problem it posed
// every change of a field POINTER of any level (a field allocated on first use, phi canvases trading places) advances this count: tables of
// pointers kept elsewhere (suhmo_hier_fill.hip: the boxes of a level as one launch target) are compared again only after it moved
void suhmo_fp_changed();
unsigned long suhmo_fp_epoch();
struct SwapGuard {
    double **a, **b; bool armed;
    SwapGuard() : a(nullptr), b(nullptr), armed(false) {}
    void arm(double **a_, double **b_) { a = a_; b = b_; std::swap(*a, *b); armed = true; suhmo_fp_changed(); }
    void back() { if (armed) { std::swap(*a, *b); armed = false; suhmo_fp_changed(); } }
    ~SwapGuard() { back(); }
};
int suhmo_average_operator_all(suhmo_level *L, int nd, hipStream_t st);      // suhmo_bcoef.hip
int suhmo_restrict_both(suhmo_level *L, int depth, hipStream_t st);                 // suhmo_ops.hip
bool suhmo_gsrb_can_fuse_prolong(suhmo_level *L, int depth, int sweeps);           // suhmo_gsrb.hip
int suhmo_level_residual_and_norm(suhmo_level *L, double *out, hipStream_t st);                   // suhmo_ops.hip
int suhmo_level_norm_from_partials(suhmo_level *L, int np, double *out, hipStream_t st);   // suhmo_ops.hip
bool suhmo_gsrb_can_fuse_rhs(suhmo_level *L, int depth, int sweeps, bool rhs_local = false);               // suhmo_gsrb.hip
bool suhmo_gsrb_can_fuse_bcoef(suhmo_level *L, int sweeps);   // suhmo_gsrb.hip: the first of `sweeps` pre-smoothing sweeps of depth 0 can form the faces
bool suhmo_gsrb_can_overlap_avg(const suhmo_level *L);        // suhmo_gsrb.hip: ... and AverageOperator behind it may run on the level's side stream
int suhmo_avg_join(suhmo_level *L, hipStream_t st);           // suhmo_gsrb.hip: st waits for the coarse faces if they are in flight there (else nothing)
void suhmo_avg_release(suhmo_level *L);                       // suhmo_gsrb.hip: the side stream and its events
int suhmo_launch_gsrb(suhmo_level *L, int depth, int sweeps, int tail, hipStream_t st, int *restricted = nullptr);   // suhmo_gsrb.hip; tail = halo
                                                    // rows worth keeping valid at exit; restricted: see there
void suhmo_level_drop_graphs(suhmo_level *L);                                     // suhmo_fas.hip
int suhmo_ensure_phi_halo(suhmo_level *L, int depth, int need, hipStream_t st);      // suhmo_ops.hip
int suhmo_fas_coarse_rhs(suhmo_level *L, int depth, hipStream_t st, int hcomp = 0);  // suhmo_ops.hip; hcomp: halo rows that get rhs computed too
// Result of a reduction whose last kernel was launched with suhmo_host_slot(L): 8 bytes back on the host.
struct HostSlot { double *val; unsigned long long *flag; unsigned long long seq; };
HostSlot suhmo_host_slot(suhmo_level *L);                                           // suhmo_ops.hip; call right before the launch
int suhmo_readback(suhmo_level *L, hipStream_t st, double *out, double *out2 = nullptr);   // after the launch; out2: a second value (scratch[1] / val[1])
// n = 1 or 2 values a reduction's last kernel left in L->scratch[0..n-1] (launched with suhmo_reduce_slot(L)): combined over the ranks of a
// strip partition (op 0 MAX, 1 SUM) and brought to the host.  On a strip with the native transport the all-reduce runs on the device, on
// the kernels' stream, and a publishing kernel follows; with host hooks the local values are read back first.
HostSlot suhmo_reduce_slot(suhmo_level *L);                                         // = suhmo_host_slot, or an empty slot when the values still travel
int suhmo_reduce_finish(suhmo_level *L, hipStream_t st, int n, int op, double *out, double *out2 = nullptr);
__device__ __forceinline__ void suhmo_publish(const HostSlot &h, double v)
{
    if (!h.val) return;
    h.val[0] = v;
    __hip_atomic_store(h.flag, h.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int suhmo_build_mg_coefficients(suhmo_level *L, bool with_faces, hipStream_t st);   // suhmo_bcoef.hip
// suhmo_agg.hip: agglomeration of the coarse multigrid depths of a rank strip
void suhmo_ipc_release(suhmo_level *L);   // suhmo_ipc.hip
int suhmo_ipc_batch(suhmo_level *L, int open, hipStream_t st);
int suhmo_agg_setup(suhmo_level *L);
void suhmo_agg_release(suhmo_level *L);
int suhmo_agg_gather_static(suhmo_level *L, bool with_faces, hipStream_t st);
int suhmo_agg_gather_faces(suhmo_level *L, int nd, hipStream_t st);
int suhmo_agg_gather_state(suhmo_level *L, hipStream_t st);
int suhmo_agg_scatter(suhmo_level *L, hipStream_t st);
int suhmo_exchange_list(suhmo_level *L, int depth, const int *fields, int n, hipStream_t st);   // LevelData::exchange across rank boundaries
// suhmo_bottom.hip: the bottom solver of the FAS cycle
bool suhmo_bottom_one_launch(const suhmo_level *L, int dep);
int suhmo_bottom_configure(suhmo_level *L, int solver, long one_launch_max_cells);
long suhmo_bottom_counter(const suhmo_level *L, int which);
int suhmo_bottom_solve(suhmo_level *L, int dep, int tail, hipStream_t st);
static inline int suhmo_halo_rows(const DV &v) { return v.gy < v.ny ? v.gy : v.ny; }
// AMRMultiGrid::solveNoInit's stopping rule as the state of ONE solve: the solve loop of a level layout below keeps one, a batch of levels
// (suhmo_batch.hip) one per member, so that members stop at their own cycle.
struct SolveNoInit {
    double rnorm, initial_rnorm, norm_last;
    int iter;
    void start(double r) { rnorm = r; initial_rnorm = r; norm_last = 2.0 * r; iter = 0; }
    bool go(const suhmo_solver_params_t *sp) const
    {
        const bool goNorm = rnorm > sp->norm_thresh, goRedu = rnorm > sp->eps * initial_rnorm, goIter = iter < sp->max_iter;
        const bool goHang = iter < sp->imin || rnorm < (1.0 - sp->hang) * norm_last, goMin = iter < sp->iter_min;
        return goMin || (goIter && goRedu && goHang && goNorm);
    }
    void cycled(double r) { norm_last = rnorm; rnorm = r; iter++; }       // one V-cycle later the residual norm is r
};
// The loop for every level layout: `residual(&norm)` evaluates the residual and its norm, `cycle()` runs one V-cycle; hist[0..*iters]
// receive the norms.  What differs between layouts (a cycle that leaves its residual behind, the closing fill of the rings) stays with
// the callables and the caller.
template <class Residual, class Cycle>
int suhmo_solve_no_init(const suhmo_solver_params_t *sp, int *iters, double *hist, Residual residual, Cycle cycle)
{
    int rc;
    double rnorm = 0.0;
    if ((rc = residual(&rnorm))) return rc;
    SolveNoInit s;
    s.start(rnorm);
    if (hist) hist[0] = rnorm;
    while (s.go(sp)) {
        if ((rc = cycle()) || (rc = residual(&rnorm))) return rc;
        s.cycled(rnorm);
        if (hist) hist[s.iter] = rnorm;
    }
    if (iters) *iters = s.iter;
    return 0;
}
