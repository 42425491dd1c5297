/*
 * suhmo_hip.h -- C-ABI of the MI355X-native hydraulic-head solve (libsuhmo_hip.so).
 *
 * Drop-in boundary for ONE hot path of EnnaDelfen/SUHMO: the per-timestep nonlinear
 * variable-coefficient Poisson (FAS multigrid) solve for hydraulic head,
 *   VCAMRNonLinearPoissonOp + AMRNonLinearPoissonOp + the AmrHydro callbacks they invoke.
 * Plain C: opaque handle, pointers and sizes, int return codes (0 = ok, <0 = error, text
 * via suhmo_last_error()), no exceptions, caller-provided HIP stream (NULL = default
 * stream).  All data fp64.  Citations are file:line in the SUHMO checkout.
 *
 * The reference calls its Fortran kernels once per box (<= 64x64 cells).  This ABI is
 * level-batched: one call works on a whole AMR level / multigrid depth that lives in HBM
 * as a "level canvas" (see DESIGN.md): the level's boxes (Chombo DisjointBoxLayout) are
 * registered once, box data (FArrayBox::dataPtr) is scattered into / gathered from the
 * canvas with suhmo_level_put_box / get_box, and every operator method of the reference
 * has one entry point below.
 *
 * Array conventions: "global" arrays are row-major [j][i] (i fastest) = Fortran a(i,j);
 * a box fab is Fortran order a(lo0:hi0, lo1:hi1) exactly as Chombo's CHF_FRA passes it.
 */
#ifndef SUHMO_HIP_H
#define SUHMO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct suhmo_level suhmo_level_t;
typedef void *suhmo_stream_t; /* hipStream_t */

/* physics constants reaching the kernels: suhmo_params.cpp:51-74; the literals 1000.0*9.8
 * and 9.8 are hard-coded in src/AmrHydroF.ChF:45-52,103,217 */
typedef struct suhmo_phys {
    double A, omega, nu, cutOffbr, maxOffbr;
    double rho_w_g; /* 9800.0 */
    double grav;    /* 9.8    */
    int cutOffB;            /* solver.cut_solve_outside_domain (src/AmrHydro.cpp:872) */
    int use_NL;             /* solver.use_NL (:877) */
    int use_mask_gradients; /* solver.use_mask_for_gradients (:873) */
} suhmo_phys_t;

/* bc.lo_bc/hi_bc (0 Dirichlet, 1 Neumann), x.lo_dirich_val ..., AmrHydro.is_periodic
 * (src/AmrHydro.cpp:99-155, mixBCValues :248-309); index [dir][side] */
typedef struct suhmo_bc {
    int    type[2][2];
    double value[2][2];
    int    periodic[2];
} suhmo_bc_t;

/* AMRMultiGrid::setSolverParameters as called at src/AmrHydro.cpp:737-762 */
typedef struct suhmo_solver_params {
    int    num_smooth, num_bottom, max_iter, iter_min, imin;
    double eps, hang, norm_thresh;
    int    bcoeff_otf;  /* solver.bcoeff_otf: UpdateOperator/AverageOperator each V-cycle */
    int    max_depth;   /* -1: as deep as MGnewOp's rule allows */
} suhmo_solver_params_t;

/* one level (or, multi-GPU, this rank's strip of rows of it) */
typedef struct suhmo_level_desc {
    int nx, ny;          /* cells of the strip held by this process */
    int j0, ny_global;   /* first global row of the strip, rows of the whole level */
    double dx, dy;
    int nbox;            /* boxes of the DisjointBoxLayout that lie in this strip */
    const int *boxes;    /* nbox x {lo0, lo1, hi0, hi1}, global cell indices; may be NULL:
                            then the strip is split into max_box x max_box boxes */
    int max_box;         /* AmrHydro.max_box_size (used when boxes == NULL), e.g. 64 */
    double alpha, beta;  /* 0, -1 at src/AmrHydro.cpp:713-714 */
    suhmo_bc_t bc;
    suhmo_phys_t phys;
    int device;          /* HIP device ordinal */
    int halo_rows;       /* ghost rows kept on the strip's y sides (>= 1) */
    int i0, nx_global;   /* AMR patch: first global column held and columns of the whole (refined) domain;
                            0, 0 = the level spans the domain in x.  A side of the rectangle that is not on the
                            domain boundary (and not a rank boundary) is a COARSE-FINE side: its ghost cells hold
                            data (suhmo_amr2_cf_interp) instead of the physical boundary condition */
    int patch_j0, patch_ny; /* AMR patch cut into rank strips: rows of the WHOLE patch (0, 0 = this handle holds all of it);
                            a y side of the strip that lies inside that range is a rank boundary (exchanged halo rows),
                            the ends of the range are coarse-fine sides */
} suhmo_level_desc_t;

/* field ids (same numbering as the test oracle) */
enum {
    SUHMO_F_PHI = 0, SUHMO_F_RHS, SUHMO_F_ACOEF, SUHMO_F_B, SUHMO_F_PI, SUHMO_F_ZB,
    SUHMO_F_MASK, SUHMO_F_BX, SUHMO_F_BY, SUHMO_F_LAMBDA, SUHMO_F_RES, SUHMO_F_LPHI,
    SUHMO_F_NL, SUHMO_F_DNL, SUHMO_F_PHIOLD, SUHMO_F_CORR, SUHMO_F_GRADX, SUHMO_F_GRADY,
    SUHMO_F_RE,
    /* fields of the caller of the solve (suhmo_level_timestep): melt rate, water pressure, water
     * flux on x / y faces, lagged head, channelisation degree */
    SUHMO_F_MR, SUHMO_F_PW, SUHMO_F_QWX, SUHMO_F_QWY, SUHMO_F_HLAG, SUHMO_F_CD,
    SUHMO_F_RHS0,        /* AMR: the base level's own rhs while it carries the FAS rhs */
    SUHMO_F_MSRC,        /* moulin source term, m/s (suhmo_level_moulin_source) */
    SUHMO_F_DCX, SUHMO_F_DCY, SUHMO_F_DTERM,   /* diffusion coefficient of the gap height on x / y faces, div(D grad b) */
    SUHMO_F_ZS,          /* ice surface height (m_iceheight), input of suhmo_level_time_varying_recharge */
    SUHMO_F_COVER,       /* hierarchies of box unions: 1 where a finer level covers the cell, else 0 (norms, Picard test, moulin integrals) */
    SUHMO_F_PHI2,        /* hierarchies of box unions: second canvas of the head (the several-sweeps-per-launch relaxation writes out of place) */
    SUHMO_F_COUNT
};

const char *suhmo_last_error(void);
int suhmo_device_count(void);

/* VCAMRNonLinearPoissonOpFactory::define + MGnewOp/AMRnewOp
 * (src/VCAMRNonLinearPoissonOp.cpp:877-953, 1016-1286): allocates the level canvas for
 * depth 0 and every multigrid depth allowed by coarsenable(2^d * s_maxCoarse) (:1053). */
int suhmo_level_create(suhmo_level_t **out, const suhmo_level_desc_t *desc);
int suhmo_level_destroy(suhmo_level_t *L);
int suhmo_level_num_depths(const suhmo_level_t *L);
/* Kernel selection of a level (defaults are chosen by level size and shape; the SUHMO_<KEY> environment variables read when
 * the level is created override them for A/B runs): key = gsrb_variant (-1 auto, 0 colour passes / tiles, 1, 2 = sweeps per
 * streaming pass), gsrb_tile, tile_t (0, 16, 32), tile_s, tile_max_cells, tile_chunks, tile_strips, fused_min_cells, fused_hc,
 * fused_nt (64, 256), fused_restrict, fas_rhs_in_relax, strips_rhs_local, bcoef_fused, graph_max_cells, poll_readback, overlap_halo,
 * agg_min_cells, fas_rhs_fused, resid_in_relax (1: the residual the solve loops evaluate after every V-cycle is left behind by the cycle's
 * last launch where the streaming kernel runs depth 0; 0: always a pass of its own).  Read-only counters: overlapped_launches, agg_gathers,
 * rhs_in_streaming_launches, rhs_in_tile_launches, residual_in_relax_launches, vcycle_graph_replays (V-cycles that ran
 * as a launch of a captured graph); on rank strips, what the relaxation scheduler did: strip_tile_launches, strip_tile_restricting_launches,
 * strip_tile_shallow_halo_fallbacks (the halo held fewer current rows than a tile launch needs: colour passes), strip_colour_passes,
 * strip_streaming_launches, strip_streaming_restricting_launches, strip_unfused_prolongations.
 * mask_known (default 1): what UpdateOperator finds out about the ice mask is kept until the mask is written again.  Contract: the mask
 * of a level changes only through this library -- every entry point that writes a field the caller names (set_field, put_box, axby,
 * set_value, divergence, fill_ghosts, unpack_rows, the exchanges (suhmo_hier_exchange included), suhmo_amr2_average / _set_covered / _reflux / _finer_operator_changed, suhmo_hier_average
 * and the hierarchy's copies) notices when that field is SUHMO_F_MASK.  suhmo_level_field_view of SUHMO_F_MASK hands out a writable pointer the
 * library cannot watch: from then on that level keeps nothing about its mask (as with mask_known = 0).  The first fused UpdateOperator of depth 0
 * after a write scans for values below 1e-6 among everything it loads (cells, ghost ring, a strip's halo rows); the answer comes back
 * through an asynchronous 4-byte copy and an event that later calls only query.  While it says "none", whole levels run the instantiations of
 * the fused WFlx_level kernel and of the streaming relaxation that leave the mask out (no load, no register, no test); the results are the
 * same bits.  0: the per-cycle report of skip_mask only.  Ensembles and box unions always read the mask.  Read-only: mask_scans,
 * bcoef_unmasked_launches, relax_unmasked_launches (launches of graph replays included), mask_state (0 unknown, 1 clean, 2 dirty).
 * zb_known (default 1): what a scan finds out about the bed elevation is kept until SUHMO_F_ZB is written again, under the same contract as
 * the mask's (the entry points above notice that field too, on any depth; suhmo_level_build_mg_coefficients rewrites the coarse depths';
 * suhmo_level_field_view of SUHMO_F_ZB ends the bookkeeping of that level for good).  The first V-cycle after a write scans every depth's
 * cells, bit pattern against bit pattern (-0.0 is not +0.0); the answers come back through an asynchronous copy and an event that later
 * cycles only query.  While a depth's bed is ONE pattern, the streaming relaxation of a whole level with a clean mask and alpha = 0 takes
 * it as a scalar and loads no zb (same operand, same bits); a varying bed, rank strips, AMR patches, hierarchies, ensembles: the array is
 * loaded as before.  0: nothing is scanned.  Read-only: zb_scans, zb_state (depth 0; zb_state_d<depth>: 0 unknown, 1 uniform, 2 varying),
 * relax_zb_uniform_launches (all depths; relax_zb_uniform_launches_d<depth>; launches of graph replays included).
 * yface_ring (default 1, env SUHMO_YFACE_RING): of those launches the plain one -- it absorbs nothing but a prolongation -- keeps one ring of
 * y-faces (the north face of a row is the south face of the next), which leaves it three waves per SIMD, and cuts its chunks for its own
 * occupancy; not on levels that are periodic in y, where face 0 and face ny are two stored rows.  0: two rings, two waves, the chunks of
 * those.  Same bits either way.  Read-only: relax_yring_launches (all depths; relax_yring_launches_d<depth>; graph replays included);
 * stream_wg_per_cu_<plain | yring | rst | rout | frhs | bcf>: the workgroups per CU the occupancy query answers for that launch of the
 * clean-mask, uniform-bed cycle (12 for yring, 8 for the others on MI355X).
 * bcoef_in_relax (default 1): while the mask of a whole level (no rank strip, no AMR patch) is known clean, alpha = 0, depth 0 relaxes on the
 * streaming kernel and the pre-smoothing has at least three sweeps, the V-cycle's UpdateOperator is not a pass of its own: the first
 * pre-smoothing launch of depth 0 forms the face coefficients from the head as it loads it and stores them (same bits), AverageOperator
 * follows that launch.  0, or any of the conditions not met: the fused WFlx_level kernel as before.  Read-only: bcoef_in_relax_launches
 * (graph replays included; such a launch also counts as a bcoef_unmasked_launch and a relax_unmasked_launch).
 * avg_overlap (default 1, env SUHMO_AVG_OVERLAP): in such a cycle, when it runs as plain launches (not as a captured graph or the eager first
 * use of a level whose cycles are captured, not while profiling), AverageOperator runs on a side stream of the level beside the next depth-0
 * launch, which reads none of the coarse faces; the cycle's stream waits for it before its first read of a coarse face and before the call
 * returns, so the caller sees one stream as before.  0: on the cycle's stream.  Same bits either way.  Read-only: avg_overlap_launches.
 * Not a kernel-selection knob (it changes the bits): bottom_solver (default 0: the cycle's bottom is its numBottom relaxes; 1: followed by
 * Chombo's RelaxSolver as the reference configures it, src/AmrHydro.cpp:623,628,726,733-735 -- up to 40 rounds of relax(2), ended by an l2
 * residual below 1e-6 x its first value or reduced by less than 10 %).  It reaches the level's agglomerated copy and its gap-height operator;
 * suhmo_hier_set_option forwards it to level 0 of a hierarchy and to its gap-height hierarchy.  bottom_one_launch_max_cells (default 16384,
 * env SUHMO_BOTTOM_ONE_LAUNCH_MAX_CELLS; 0 = never): whole-level bottoms of up to this many cells (at most 128 x 128) run the loop in one
 * launch, larger ones, rank strips and AMR patches as a host loop of launches with an 8-byte read-back per iteration (their V-cycles are
 * then not replayed as graphs).  Read-only counters: bottom_solver_iterations, bottom_solves_one_launch, bottom_solves_host_loop.
 * On rank strips every rank must make the same choices (suhmo_level_attach_rccl checks). */
int suhmo_level_set_option(suhmo_level_t *L, const char *key, long value);
int suhmo_level_get_option(const suhmo_level_t *L, const char *key, long *value);
int suhmo_level_synchronize(suhmo_level_t *L, suhmo_stream_t s);

/* LevelData<FArrayBox> / LevelData<FluxBox> traffic, box by box (DataIterator order =
 * index into desc.boxes).  `fab` is a host pointer to Fortran-order data over
 * [flo0:fhi0] x [flo1:fhi1] (the FArrayBox box of that grid at this depth, ghosts
 * included; for face fields the face-centred box).  put copies the VALID cells (faces) of
 * box `ibox` and, if with_domain_ghosts != 0, those ghost cells of the fab that lie outside
 * the problem domain (caller-owned data for B / iceMask); interior ghost cells are never
 * copied (they duplicate a neighbour's valid cells).  get fills valid cells plus all ghost
 * cells of the fab from the canvas (= what exchange + BC would have produced).
 * Caller-owned ghost data across a PERIODIC side (B, Pi, zb, iceMask, however they are set: put_box, set_field, a box of a
 * hierarchy) must be the periodic image of the valid cells, bit for bit, as the reference's exchange leaves it.  A periodic
 * level has one face on the wrap: the library keeps the coefficient of face 0 == face nx (ny) once, computed from the ghost
 * on one side, and a reflux or a flux across the wrap reads it.  Ghost data that is periodic only up to rounding gives two
 * values for that face, and results that differ from the reference's in the last bits. */
int suhmo_level_put_box(suhmo_level_t *L, int depth, int field, int ibox, const double *fab,
                        int flo0, int flo1, int fhi0, int fhi1, int with_domain_ghosts,
                        suhmo_stream_t s);
int suhmo_level_get_box(suhmo_level_t *L, int depth, int field, int ibox, double *fab,
                        int flo0, int flo1, int fhi0, int fhi1, suhmo_stream_t s);
/* whole-strip variants: cell fields ny x nx (ghosted: (ny+2) x (nx+2)); BX ny x (nx+1);
 * BY (ny+1) x nx.  `on_device` != 0: src/dst is a device pointer. */
int suhmo_level_set_field(suhmo_level_t *L, int depth, int field, const double *src,
                          int ghosted, int on_device, suhmo_stream_t s);
int suhmo_level_get_field(suhmo_level_t *L, int depth, int field, double *dst,
                          int ghosted, int on_device, suhmo_stream_t s);
/* raw device view of a field canvas (for zero-copy callers): base pointer, pitch in
 * doubles, offset of cell (0,0) */
int suhmo_level_field_view(suhmo_level_t *L, int depth, int field, double **base,
                           long *pitch, long *origin);

/* --- operator methods; each replaces the named reference method for a whole level --- */
/* AMRNonLinearPoissonOp::relax -> VCAMRNonLinearPoissonOp::levelGSRB x sweeps
 * (src/AMRNonLinearPoissonOp.cpp:707-750, src/VCAMRNonLinearPoissonOp.cpp:654-760), kernel
 * GSRBHELMHOLTZVCNL2D (src/VCAMRNonLinearPoissonOpF.ChF:46-168) with COMPUTENONLINEARTERMS
 * (src/AmrHydroF.ChF:23-68), SUMFACESNL (:574-601) and mixBCValues fused in. */
int suhmo_level_gsrb(suhmo_level_t *L, int depth, int sweeps, suhmo_stream_t s);
/* applyOpI / applyOpNoBoundary (src/VCAMRNonLinearPoissonOp.cpp:273-345), VCNLCOMPUTEOP2D */
int suhmo_level_apply_op(suhmo_level_t *L, int depth, int homogeneous, suhmo_stream_t s);
/* residualI (:98-167), VCNLCOMPUTERES2D */
int suhmo_level_residual(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* restrictResidual (:384-460), RESTRICTRESVCNL2D: RES[depth+1] */
int suhmo_level_restrict_residual(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* restrictR (:347-372), RESTRICTVCNL: PHI[depth+1] */
int suhmo_level_restrict_r(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* prolongIncrement (src/AMRNonLinearPoissonOp.cpp:856-886), PROLONGNL:
 * PHI[depth] += P(CORR[depth+1]) */
int suhmo_level_prolong_increment(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* AMRProlongS_2's kernel PROLONG_2_NL (src/AMRNonLinearPoissonOpF.ChF:646-709):
 * PHI[depth] += bilinear(CORR[depth+1], ghosted) */
int suhmo_level_prolong_bilinear(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* UpdateOperator (src/VCAMRNonLinearPoissonOp.cpp:34-64) = AmrHydro::WFlx_level
 * (src/AmrHydro.cpp:1415-1539): NEWMACGRAD, EdgeToCell, ExtrapGhostCells, COMPUTERE,
 * CellToEdge, setup_iceMask_EC, COMPUTEBCOEFF -> BX, BY of `depth` */
int suhmo_level_update_operator(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* AverageOperator (:66-95): BX,BY[depth] <- CoarseAverageFace(BX,BY[0], 2^depth) */
int suhmo_level_average_operator(suhmo_level_t *L, int depth, suhmo_stream_t s);
/* MGnewOp coefficient coarsening (:1096-1173) for every depth > 0 */
int suhmo_level_build_mg_coefficients(suhmo_level_t *L, suhmo_stream_t s);
/* stand-alone pieces for parity of a2 / a9 / a16 / a19 / a10 */
int suhmo_level_nonlinear(suhmo_level_t *L, int depth, suhmo_stream_t s);     /* NL, DNL */
int suhmo_level_compute_lambda(suhmo_level_t *L, int depth, suhmo_stream_t s);/* LAMBDA  */
int suhmo_level_fill_ghosts(suhmo_level_t *L, int depth, int field, int homogeneous,
                            suhmo_stream_t s);   /* exchange (periodic wrap) + mixBCValues */
/* DIVERGENCE (util/DivergenceF.ChF:23-57): dst_field += d(BX)/dx + d(BY)/dy */
int suhmo_level_divergence(suhmo_level_t *L, int depth, int dst_field, suhmo_stream_t s);
/* getFlux (src/VCAMRNonLinearPoissonOp.cpp:792-841) on all faces of direction dir into
 * device/host array `flux` shaped like BX/BY */
int suhmo_level_get_flux(suhmo_level_t *L, int depth, int dir, int ref, double *flux_host,
                         suhmo_stream_t s);
/* norm over valid cells (AMRNonLinearPoissonOp::norm, :660-666): ord 0 max-abs, 2 l2 */
int suhmo_level_norm(suhmo_level_t *L, int depth, int field, int ord, double *out,
                     suhmo_stream_t s);
/* dotProduct (src/AMRNonLinearPoissonOp.cpp:519-551): sum over the valid cells of x * y (device reduction; over all ranks of a strip
 * partition through the reduce hook; the summation order differs from the reference's box-by-box sum: 1e-12 relative) */
int suhmo_level_dot(suhmo_level_t *L, int depth, int x, int y, double *out, suhmo_stream_t s);
/* LevelDataOps vector ops (:629-688): dst = a*x + b*y ; dst += scale*x ; set value */
int suhmo_level_axby(suhmo_level_t *L, int depth, int dst, int x, int y, double a, double b,
                     suhmo_stream_t s);
int suhmo_level_set_value(suhmo_level_t *L, int depth, int field, double v, suhmo_stream_t s);

/* one FAS V-cycle on PHI/RHS of depth 0, and the AMRMultiGrid::solve loop
 * (src/AmrHydro.cpp:766).  hist (length max_iter+1, may be NULL) gets residual norms. */
int suhmo_level_vcycle(suhmo_level_t *L, const suhmo_solver_params_t *sp, suhmo_stream_t s);
int suhmo_level_solve(suhmo_level_t *L, const suhmo_solver_params_t *sp, int *iters,
                      double *hist, suhmo_stream_t s);

/* ---- the caller of the solve ("next rows" of the hot path): one AmrHydro::timeStepFAS
 * (src/AmrHydro.cpp:2254-3460) for a single level with distributed water input and the explicit
 * gap-height update: Picard loop { lagged Re / Qw / melt rate -> RHS_h (:2920-3079) ->
 * SolveForHead_nl (:3119) -> convergence test (:3169-3228) } then CalcRHS_gapHeightFAS (:2069-2171)
 * + forward Euler (:3394-3408).  PHI holds the head, B the gap height (both updated in place).
 * On a rank strip (desc.j0 / ny_global, hooks attached) every rank calls it with the same arguments: the halo rows of
 * b, mR, grad h and RHS_h travel through the exchange hook where the reference calls exchange(), the Picard test is
 * MAX all-reduced, and the result equals the single-process one bit for bit. */
typedef struct suhmo_model_params {
    double rho_i, rho_w, gravity;      /* suhmo_params.cpp:51-53 */
    double G, L, ct, cw;               /* suhmo.GeoFlux, LatHeat, ct, cw */
    double ub0, ub1;                   /* suhmo.SlidingVelocity */
    double br, lr;                     /* suhmo.br, suhmo.lr */
    double diffFactor;                 /* suhmo.diffFactor: weight of div(D grad b) in both equations (:3071, :2145) */
    double distributed_input;          /* suhmo.distributed_input */
    double eps_picard;                 /* solver.eps_PicardIte */
    int basal_friction, use_mask_rhs_b;
    int use_moulin_source;             /* suhmo.n_moulins > 0: RHS_h += MSRC * ramp + distributed_input (:3060-3066) */
    double ramp;                       /* suhmo.ramp factor of this step (:2448-2467); 1 when off */
    int use_impl_diff;                 /* solver.use_ImplDiff: gap height by the implicit VC Helmholtz solve (:593-662) */
    /* Run-state settings (0, 0 = the committed source).  The reference's committed result tables (exec/{A,B,E,F}_SHMIP/.../
     * results/postproc.dat) were written by a code state that differs from the committed source in these two places -- read off the
     * tables themselves, DESIGN.md section 4 -- so a run that is to be diffed against those tables sets them:
     *   head_melt_off       1: RHS_h without the melt term mR (1/rho_w - 1/rho_i) (src/AmrHydro.cpp:3046-3048; the term is
     *                       multiplied by 0.0, as the test oracle's knob does)
     *   freeze_icefree_gap  1: the gap height of cells without ice (iceMask < 0) is left as it is by the implicit gap-height
     *                       solve (SolveForGap_nl, :593-662, :3425-3455; CalcRHS_gapHeightFAS :2069-2171 with use_mask_rhs_b already
     *                       keeps it in the explicit update)
     * The third setting of suite F, the surface elevation in the field the lapse rate reads (src/ValleyIBC.cpp:299 ends with the
     * ice thickness), is data: load SUHMO_F_ZS with whichever field the run is to use. */
    int head_melt_off, freeze_icefree_gap;
} suhmo_model_params_t;
/* cur_step = AmrHydro::m_cur_step after its increment (1 for the first step): selects the solver
 * parameters and the Picard stopping rule.  picard_iters / vcycles: totals of this step. */
int suhmo_level_timestep(suhmo_level_t *L, const suhmo_model_params_t *mp, double dt, int cur_step,
                         int *picard_iters, int *vcycles, suhmo_stream_t s);

/* Moulin source term of one level (Calc_moulin_integral + Calc_moulin_source_term_distributed,
 * src/AmrHydro.cpp:1866-2066): n Gaussians (positions x0,y0,x1,y1,..., sigma, flux in m3/s; HOST arrays) sampled
 * with the reference's 3 x 3 Gauss-Legendre rule per cell, each normalised by its integral over the level;
 * time_factor = max(1 - runoff sin(2 pi (t - t_restart) / 86400), 0).  Result in SUHMO_F_MSRC (m/s);
 * integrals (m2, n values) are returned when the pointer is not NULL.  exp() is the device library's: results
 * agree with the CPU restatement to ~1e-14 relative, not bitwise.  On a rank strip every rank integrates over the
 * whole level itself (the integrand is analytic), in the single-process order: no communication, same bits. */
int suhmo_level_moulin_source(suhmo_level_t *L, int n_moulins, const double *positions, const double *sigma,
                              const double *flux, double time_factor, double *integrals, suhmo_stream_t s);

/* Time-varying distributed recharge (suhmo.time_varying_input, suites D / F of SHMIP; COMPUTE_TIMEVARYINGRECHARGE,
 * src/AmrHydroF.ChF:346-373, caller src/AmrHydro.cpp:2849-2861): MSRC = max(ddf (T_K + zs dT/dz), 0) + background with
 * ddf = 0.01/86400, dT/dz = -0.0075, zs = SUHMO_F_ZS, T_K = -16 cos(2 pi (t - t_restart)/year) - 5 + deltaT computed by the
 * caller.  Use with model.use_moulin_source = 1, ramp = 1, distributed_input = 0 (RHS_h takes MSRC as its source term). */
int suhmo_level_time_varying_recharge(suhmo_level_t *L, double T_K, double background_input, suhmo_stream_t s);

/* SHMIP cross-section table of the current state (AmrHydro::timeStepFAS post-processing, src/AmrHydro.cpp:3647-4102;
 * columns of the results/postproc.dat files under exec/A_SHMIP, exec/B_SHMIP, ...): for every cell column i the row
 *   x [km], ice-covered width, discharge, channelised part, distributed part (through x-face i, weighted with the
 *   channelisation degree on the face), recharge by the external input and by melt upstream of the column (cumulative
 *   from the upper end), mean effective pressure [MPa].
 * table: HOST array nx x 8, row-major.  Uses QWX, CD, MR, PW, PI, MASK (and MSRC with use_moulin_source) as the last
 * suhmo_level_timestep left them. */
int suhmo_level_postproc_table(suhmo_level_t *L, const suhmo_model_params_t *mp, double *table, suhmo_stream_t s);
/* the same in two steps for a level cut into rank strips: column sums over this strip's rows (HOST array 8 x nx: width,
 * Q, Q channelised, Q distributed, external recharge, melt recharge, sum and count of Pi - Pw), which the host adds over
 * the ranks (the reference: MPI_Allreduce, src/AmrHydro.cpp:3818-4013), and the table from the added sums */
int suhmo_level_postproc_partial(suhmo_level_t *L, const suhmo_model_params_t *mp, double *sums, suhmo_stream_t s);
int suhmo_postproc_finish(const double *sums, int nx, double dx, double *table);
/* the temporal post-processing (AmrHydro.post_proc_shmip_temporal, src/AmrHydro.cpp:3778-3810, 4040-4053; the rows of
 * exec/F_SHMIP/F<k>/results/postproc.dat) from the same column sums: out[6] = mean effective pressure [Pa] over the ice-covered
 * cells, over the bands 600 m < x < 900 m, 3000 m < x < 3300 m, 5100 m < x < 5400 m (cell centres; NaN for an empty band), the recharge
 * upstream of column 1 (external + melt) and the discharge through x-face 1.  suhmo_level_postproc_temporal: a whole level. */
int suhmo_postproc_temporal(const double *sums, int nx, double dx, double *out);
int suhmo_level_postproc_temporal(suhmo_level_t *L, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s);
/* the same six values finished on the device (the body a run of an ensemble writes its rows with, suhmo_batch_run): the column sums stay there,
 * 48 bytes come back.  The bits of suhmo_level_postproc_temporal: one thread per value, the host function's operations in its column order. */
int suhmo_level_postproc_temporal_device(suhmo_level_t *L, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s);

/* setAlphaAndBeta (src/VCAMRNonLinearPoissonOp.cpp:462-469) and setBC (src/AMRNonLinearPoissonOp.cpp:1275-1278) of the
 * operator, for every multigrid depth of the level; setBC keeps the periodicity the level was created with */
int suhmo_level_set_alpha_beta(suhmo_level_t *L, double alpha, double beta);
int suhmo_level_set_bc(suhmo_level_t *L, const suhmo_bc_t *bc);

/* multi-GPU strips: pack the `rows` owned rows next to side (0 = y-lo, 1 = y-hi) of a
 * field into a contiguous device buffer (rows x (nx+1) doubles) / unpack a neighbour's rows
 * into the ghost rows of that side.  The transport (RCCL send/recv) belongs to the host. */
int suhmo_level_pack_rows(suhmo_level_t *L, int depth, int field, int side, int rows,
                          double *dev_buf, suhmo_stream_t s);
int suhmo_level_unpack_rows(suhmo_level_t *L, int depth, int field, int side, int rows,
                            const double *dev_buf, suhmo_stream_t s);
/* hook called by the V-cycle driver wherever the reference calls LevelData::exchange on a
 * field whose strip ghost rows must come from another rank; NULL = single process. */
typedef int (*suhmo_exchange_fn)(void *user, suhmo_level_t *L, int depth, const int *fields,
                                 int nfields, suhmo_stream_t s);   /* several fields = one message per neighbour */
typedef int (*suhmo_allreduce_max_fn)(void *user, double *value);
int suhmo_level_set_hooks(suhmo_level_t *L, suhmo_exchange_fn ex, suhmo_allreduce_max_fn ar,
                          void *user);
/* general reduction over the ranks of a strip partition: n values in place, op 0 = MAX, 1 = SUM (what the reference does with
 * MPI_Allreduce inside norm(), dotProduct() and computeMax, src/AMRNonLinearPoissonOp.cpp:660-666, 1222-1264; src/AmrHydro.cpp:3169-3185).
 * Optional: with only the MAX hook of suhmo_level_set_hooks, suhmo_level_norm(ord 2) and suhmo_level_dot on a strip return -5.
 * `user` is the pointer given to suhmo_level_set_hooks.  suhmo_level_attach_rccl installs a device-resident equivalent
 * (ncclAllReduce on the kernels' stream, the result read back through pinned memory: no stream synchronisation). */
typedef int (*suhmo_allreduce_fn)(void *user, double *values, int n, int op);
int suhmo_level_set_reduce_hook(suhmo_level_t *L, suhmo_allreduce_fn fn);
/* all-gather of `count` doubles per rank (device buffers; recv holds world x count, rank-major, ranks in ascending j0), enqueued on /
 * ordered with s.  With it attached, the multigrid depths whose strip holds fewer than `agg_min_cells` cells (option, default 100000;
 * SURVEY.md 8e) are AGGLOMERATED: every rank runs them redundantly on a copy of the whole level, fed by two all-gathers per V-cycle,
 * instead of exchanging halo rows per relaxation (suhmo_amd/csrc/suhmo_agg.hip).  suhmo_level_attach_rccl installs ncclAllGather.
 * suhmo_level_agglomerated_depth: first agglomerated depth, 0 = none. */
typedef int (*suhmo_allgather_fn)(void *user, const double *send, long count, double *recv, suhmo_stream_t s);
int suhmo_level_set_allgather(suhmo_level_t *L, suhmo_allgather_fn fn, void *user);
int suhmo_level_agglomerated_depth(const suhmo_level_t *L);
/* LevelData::exchange of one field across the strip's rank boundaries (calls the hook; a
 * no-op for a single-process level).  Used by the host after it loads coefficient fields. */
int suhmo_level_exchange(suhmo_level_t *L, int depth, int field, suhmo_stream_t s);
/* rows of ghost data kept per y side / 1 if the side is a rank boundary */
int suhmo_level_halo_info(const suhmo_level_t *L, int depth, int *halo_rows, int *ext_lo, int *ext_hi,
                          int *nx, int *ny);
/* rank strips, read-only: the halo rows of phi (counted from the strip's edge, each rank-boundary side) that hold the neighbour's
 * current values according to the scheduler's bookkeeping; 0 .. min(halo_rows, ny); -1 on bad arguments */
int suhmo_level_phi_halo_fresh(const suhmo_level_t *L, int depth);

/* Native transport for those hooks: RCCL send/recv + 1-element MAX all-reduce enqueued on the caller's
 * stream (suhmo_amd/csrc/suhmo_rccl.hip); stands where the reference has MPI under LevelData::exchange
 * (src/VCAMRNonLinearPoissonOp.cpp:692) and under norm() (src/AMRNonLinearPoissonOp.cpp:1222-1264).
 *   suhmo_rccl_load       dlopen librccl (path NULL/"" = "librccl.so"); no link-time dependency
 *   suhmo_rccl_unique_id  128-byte ncclUniqueId, made on one rank, distributed by the host (MPI_Bcast, ...)
 *   suhmo_level_attach_rccl  COLLECTIVE: ranks 0..world-1 own the strips in ascending j0; installs the hooks
 *   suhmo_level_rccl_exchanges  messages sent so far by this level (diagnostics) */
int suhmo_rccl_load(const char *librccl_path);
int suhmo_rccl_unique_id(void *id128);
int suhmo_level_attach_rccl(suhmo_level_t *L, const void *id128, int rank, int world, int periodic_y,
                            suhmo_stream_t s);
int suhmo_level_detach_rccl(suhmo_level_t *L);
long suhmo_level_rccl_exchanges(const suhmo_level_t *L);
int suhmo_level_rccl_comm_count(const suhmo_level_t *L);   /* ranks the level's communicator reports (ncclCommCount); -1: not attached */
/* ---- peer-direct halo transport (suhmo_amd/csrc/suhmo_ipc.hip; SUHMO_TRANSPORT=ipc in suhmo_amd.multigpu): a rank's exchange kernel stores its
 * edge rows straight into the neighbour's receive slots -- device memory of the neighbouring GPU mapped with hipIpcOpenMemHandle, peer
 * stores over xGMI -- and publishes a sequence number there; the same launch polls the neighbour's number locally, copies its own slots
 * into the halo rows and acknowledges (one launch per message, a flag pair per workgroup, no grid-wide step).  What the
 * reference does with MPI point-to-point inside LevelData::exchange (src/VCAMRNonLinearPoissonOp.cpp:692, 912-913) without a
 * communication kernel in between.  Two steps, both per rank: suhmo_level_ipc_export lays out and allocates the rank's arena and fills
 * `blob128` (128 bytes: the IPC handle, the process id, the address); the host carries the blobs to the neighbours (MPI_Sendrecv /
 * torch.distributed all_gather); suhmo_level_attach_ipc maps the arenas of rank - 1 and rank + 1 (periodic_y: the ends are neighbours;
 * NULL where there is none; ranks that are threads of one process, or a rank that is its own neighbour, need no mapping) and routes the
 * level's halo exchanges through them.  Reductions and all-gathers keep the transport the level is attached to (suhmo_level_attach_rccl,
 * suhmo_level_set_hooks): attach that first.  Every wait on a neighbour is bounded (about 3 s): the next exchange then fails with rc -7.
 * Destroy or detach a level only after something that synchronises the ranks has followed its last exchange (a norm, a barrier): a neighbour's
 * last acknowledgement is a store into this rank's arena. */
int suhmo_level_ipc_export(suhmo_level_t *L, void *blob128);
int suhmo_level_attach_ipc(suhmo_level_t *L, int rank, int world, int periodic_y, const void *blob_lo, const void *blob_hi);
long suhmo_level_ipc_exchanges(const suhmo_level_t *L);   /* halo messages sent so far; -1: not attached */
int suhmo_level_detach_ipc(suhmo_level_t *L);               /* back to the transport the level had before suhmo_level_attach_ipc; the arena is unmapped and freed */

/* ---- two AMR levels: base level `coarse` (spans the domain) + one patch `fine` refined by 2, created with
 * desc.i0 / nx_global / j0 / ny_global = its place in the refined domain (coarse-aligned), dx = coarse dx / 2.
 * Method names of the reference in brackets (src/AMRNonLinearPoissonOp.cpp, src/VCAMRNonLinearPoissonOp.cpp).
 *   suhmo_amr2_cf_interp    fine coarse-fine ghosts of field_f <- QuadCFInterp(coarse field_c)  [m_interpWithCoarser.coarseFineInterp :701,:933]
 *   suhmo_amr2_average      coarse field_c under the patch <- average of fine field_f           [AMRRestrictS :1027-1069]
 *   suhmo_amr2_fine_update_operator   bCoef of the fine level from head + coarse head          [UpdateOperator :34-64, WFlx_level :1455-1488]
 *   suhmo_amr2_residual     RES on both levels (coarse: with reflux, covered cells zeroed), composite max norm
 *                           [AMRResidual/AMRResidualNF :889-939, reflux :555-652, AMRNorm :1222-1264]
 *   suhmo_amr2_vcycle / suhmo_amr2_solve   AMR FAS cycle (relaxNF, AMRRestrictS, base-level V-cycle, AMRProlongS_2
 *                           :1143-1206) and the solveNoInit loop on the composite norm */
int suhmo_amr2_cf_interp(suhmo_level_t *coarse, suhmo_level_t *fine, int field_f, int field_c, suhmo_stream_t s);
int suhmo_amr2_average(suhmo_level_t *coarse, suhmo_level_t *fine, int field_f, int field_c, suhmo_stream_t s);
int suhmo_amr2_prolong2(suhmo_level_t *coarse, suhmo_level_t *fine, int field_c, suhmo_stream_t s);      /* AMRProlongS_2 :1143-1206 */
int suhmo_amr2_set_covered(suhmo_level_t *coarse, suhmo_level_t *fine, int field_c, double value, suhmo_stream_t s); /* AMRNorm :1241-1258 */
int suhmo_amr2_fine_update_operator(suhmo_level_t *coarse, suhmo_level_t *fine, suhmo_stream_t s);
/* pieces of the AMRLevelOp interface the FAS cycle of the fork does not use itself:
 *   suhmo_amr2_reflux       coarse field_c (holding L(phi) of the coarse level) += flux mismatch on the coarse-fine faces,
 *                           after coarseFineInterp of the fine head               [reflux, src/VCAMRNonLinearPoissonOp.cpp:555-652]
 *   suhmo_amr2_prolong_pc   fine PHI += coarse field_c, piecewise constant         [AMRProlong / AMRProlongS :1073-1140]
 *   suhmo_amr2_finer_operator_changed   coarse aCoef, B, Pi, zb, iceMask, bCoef under the patch <- averages of the fine
 *                           level's                                                [finerOperatorChanged :1356-1439]
 *   suhmo_amr2_pwl_fill     fine ghost ring of field_f <- PiecewiseLinearFillPatch(coarse field_c): limited linear
 *                           interpolation, the time loop's coarse-fine ghosts of b, mR, Re [src/AmrHydro.cpp:2373-2380, 2499-2507, 2711-2719] */
int suhmo_amr2_pwl_fill(suhmo_level_t *coarse, suhmo_level_t *fine, int field_f, int field_c, suhmo_stream_t s);
int suhmo_amr2_reflux(suhmo_level_t *coarse, suhmo_level_t *fine, int field_c, suhmo_stream_t s);
int suhmo_amr2_prolong_pc(suhmo_level_t *coarse, suhmo_level_t *fine, int field_c, suhmo_stream_t s);
int suhmo_amr2_finer_operator_changed(suhmo_level_t *coarse, suhmo_level_t *fine, suhmo_stream_t s);
int suhmo_amr2_residual(suhmo_level_t *coarse, suhmo_level_t *fine, double *norm, suhmo_stream_t s);
int suhmo_amr2_vcycle(suhmo_level_t *coarse, suhmo_level_t *fine, const suhmo_solver_params_t *sp, suhmo_stream_t s);
int suhmo_amr2_solve(suhmo_level_t *coarse, suhmo_level_t *fine, const suhmo_solver_params_t *sp, int *iters,
                     double *resid_hist, suhmo_stream_t s);

/* N nested levels: levels[0] = base level, levels[l] = one patch refined by 2 and properly nested (2 cells) in
 * level l-1 (cfg4 / cfg5 hierarchies); the suhmo_amr2_* calls are the nlev = 2 case.  A coarser level that is itself
 * a patch gets its own coarse-fine ghosts interpolated before its operator or gradient is evaluated. */
int suhmo_amr_residual(suhmo_level_t **levels, int nlev, double *norm, suhmo_stream_t s);
int suhmo_amr_vcycle(suhmo_level_t **levels, int nlev, const suhmo_solver_params_t *sp, suhmo_stream_t s);
int suhmo_amr_solve(suhmo_level_t **levels, int nlev, const suhmo_solver_params_t *sp, int *iters,
                    double *resid_hist, suhmo_stream_t s);
/* suhmo_level_timestep on the hierarchy (AmrHydro::timeStepFAS with m_finest_level > 0): per level the same phases,
 * PiecewiseLinearFillPatch of the coarse-fine ghosts of b, mR, Re, QuadCFInterp of h and of its cell-centred gradient,
 * SolveForHead_nl over all levels, CoarseAverage of h (:3138-3141), Picard test over the cells no finer level covers.
 * Gap height: forward Euler level by level, or (use_impl_diff) SolveForGap_nl over the hierarchy.  PHI / B of every level
 * updated in place. */
int suhmo_amr_timestep(suhmo_level_t **levels, int nlev, const suhmo_model_params_t *mp, double dt, int cur_step,
                       int *picard_iters, int *vcycles, suhmo_stream_t s);
/* suhmo_level_moulin_source on the hierarchy (Calc_moulin_integral over all levels, src/AmrHydro.cpp:1866-2019: cells under
 * a finer level do not count; :2819-2826: they get the average of the finer level's source term).  MSRC of every level
 * this process holds.  patch_boxes: 4 (nlev - 1) ints, box (lo0, lo1, hi0, hi1) of level l+1 in the cells of level l;
 * NULL = take the geometry from the handles (every level whole on this process).  On rank strips every rank integrates
 * all levels itself from patch_boxes: no communication, the single-process bits. */
int suhmo_amr_moulin_source(suhmo_level_t **levels, int nlev, const int *patch_boxes, int n_moulins, const double *positions,
                            const double *sigma, const double *flux, double time_factor, double *integrals, suhmo_stream_t s);

/* ---- hierarchies whose levels are UNIONS OF BOXES, as the reference grids them (BRMeshRefine: several abutting and
 * disjoint boxes per level, src/AmrHydro.cpp:4176-4604; exec/AMR_multiMoulins/run_C_3lev/input.hydro:37,64-83).
 * Level 0 = the domain (desc `base`, one level handle with its multigrid depths); level l >= 1 = nbox[l] disjoint,
 * coarse-aligned boxes (lo0, lo1, hi0, hi1 in the index space of level l, one after the other in `boxes`, level 1
 * first; nbox[0] is ignored) refined by 2, whose union is properly nested in level l-1: coarsen(box) grown by 2 cells lies
 * in the union of level l-1 or outside the domain.  Every box is a level handle of its own (suhmo_hier_box: load and read
 * its fields with suhmo_level_set_field / get_field, ghosted = with the box's own ghost ring) keeping ITS OWN ghost cells,
 * as a Chombo box does; ghost cells are fine-fine (another box of the level holds the cell: suhmo_hier_exchange =
 * Copier::exchange, src/VCAMRNonLinearPoissonOp.cpp:912-913), coarse-fine (suhmo_hier_cf_interp = QuadCFInterp with the
 * tangential stencil restricted to coarse cells the level does not cover, suhmo_hier_pwl_fill = PiecewiseLinearFillPatch)
 * or domain ghosts (physical BC).  The cycle is suhmo_amr_vcycle's; with one box per level the
 * results equal suhmo_amr_*'s bit for bit.
 * ONE PROCESS PER GPU: `base` may describe a rank's STRIP of level 0 (j0 / ny / ny_global as for suhmo_level_create, equal
 * strips, rank = j0 / ny; halo_rows as the strip needs them).  Level 0 -- where the cells are -- is then partitioned as a
 * single level is (halo rows over suhmo_level_attach_rccl / suhmo_level_set_hooks on suhmo_hier_box(H, 0, 0)); the boxes of
 * the levels >= 1 are held and relaxed by EVERY rank while they are small (a few per cent of the cells of the configurations
 * the reference ships, exec/AMR_multiMoulins/run_C_3lev) and dealt to the ranks, storage and work, from partition_min_cells on (below).  Level 1 reads level 0 through
 * an all-gather of exactly the coarse cells its stencils touch (suhmo_hier_attach_rccl, or suhmo_hier_set_allgather for a
 * host transport) and writes only this rank's rows.  Results are the single-process bits. */
typedef struct suhmo_hier suhmo_hier_t;
int suhmo_hier_create(suhmo_hier_t **out, const suhmo_level_desc_t *base, int nlev, const int *nbox, const int *boxes);
/* the same with options, "key=value,key=value" (NULL = defaults): shadow = 1 routes level 1's reads of an UNCUT level 0 through the
 * pack / all-gather / unpack path of rank strips (tests of that path on one rank); push_ghosts = 0: an exchange launch before every
 * colour pass instead of side cells pushed by the pass; incremental_residual = 0: every composite residual and coarse gradient of
 * a cycle over the whole of level 0 (default 1: inside suhmo_hier_solve the residual evaluated for the stopping rule serves the next
 * cycle except in the cells the average from level 1 changed, and level 0's gradient is evaluated only where level 1's coarse-fine
 * interpolation reads it -- the same bits, two passes over level 0 less per cycle).  fused_relax = 0: a launch per colour pass on the levels
 * of boxes (default 1: up to four sweeps per launch, a box's 16 x 16 tiles advancing the 8 cells around them from the neighbours' canvases;
 * box_sweeps = 2: two sweeps per launch on 4 cells; read-only counter fused_relax_launches); fused_prolong = 0: AMRProlongS_2 as three
 * launches (default: one workgroup per box); merged_launches = 0: a launch for either kind of ghost cell, for the gradient and its ghosts, for Re
 * and bCoef, per level for ghosts / operator / reflux / norm, a read-back per level's norm, the closing ghost fill and the leaving of a FAS problem on
 * their own (default 1: one launch each, several levels per launch where nothing orders them -- the same bits).  These can also be changed later
 * (suhmo_hier_set_option; the gap-height hierarchy of suhmo_hier_timestep is created with the current values and follows every change).
 * An unknown key is refused; shadow and partition_min_cells are fixed at creation.
 * partition_min_cells = n (rank strips; default 350000): when the largest level >= 1 holds at least n cells PER RANK the levels >= 1 are dealt to the ranks, the boxes
 * of a level in the order given cut into runs of about equal cell counts (the reference: LoadBalance(procIDs, grids),
 * src/AmrHydro.cpp:4283, 4929).  OWNER COMPUTES: every pass over such a level runs on the owner's boxes only and only they (plus mirrors
 * of the neighbours' boxes a plan of this rank reads) have storage here -- every other box is a stub (suhmo_hier_box_owner);
 * what a plan reads of another rank's box travels as packed cells in one all-gather: before a colour pass the side cells of the colour
 * just advanced, one cell deep, of the boxes that have a neighbour on another rank (the reference's Copier: exchange() before every
 * colour pass, src/VCAMRNonLinearPoissonOp.cpp:692, 912-913), the coarse cells of coarse-fine stencils and correction windows, the
 * fine cells next to coarse-fine faces for the flux register; averages onto coarse cells another rank holds travel as packed
 * rectangles.  Below the threshold a pass over the levels is shorter than the messages, so every rank relaxes all boxes.  The same
 * bits either way.  Read-only through suhmo_hier_get_option: partitioned_level_<l> (0 / 1), own_boxes_level_<l>, held_boxes_level_<l>
 * (own + mirrors), owned_cells_level_<l>, canvas_bytes_level_<l> (bytes of the level's canvases on this rank),
 * gap_num_boxes (boxes of the levels >= 1 of the gap-height hierarchy of the implicit time step, which is made on the hierarchy's own boxes by the
 * first implicit step; -1 while there is none),
 * ghost_exchange_bytes_level_<l> (what this rank sends per colour-pass exchange) and ghost_exchange_bound_bytes_level_<l> (4 sides x 8 B
 * of its boxes), partition_gathers, partition_bytes (collectives of the partition so far / bytes this rank put into them). */
int suhmo_hier_create_opts(suhmo_hier_t **out, const suhmo_level_desc_t *base, int nlev, const int *nbox, const int *boxes, const char *options);
int suhmo_hier_set_option(suhmo_hier_t *H, const char *key, long value);
int suhmo_hier_get_option(const suhmo_hier_t *H, const char *key, long *value);
/* all-gather of `count` doubles per rank (device buffers; recv holds world x count, rank-major), enqueued on / ordered with s */
typedef suhmo_allgather_fn suhmo_hier_allgather_fn;
int suhmo_hier_set_allgather(suhmo_hier_t *H, suhmo_hier_allgather_fn fn, void *user);
int suhmo_hier_attach_rccl(suhmo_hier_t *H);    /* after suhmo_level_attach_rccl on the base strip: ncclAllGather on its communicator */
long suhmo_hier_gathers(const suhmo_hier_t *H); /* all-gathers issued so far */
int suhmo_hier_destroy(suhmo_hier_t *H);
int suhmo_hier_num_levels(const suhmo_hier_t *H);
int suhmo_hier_num_boxes(const suhmo_hier_t *H, int level);
suhmo_level_t *suhmo_hier_box(suhmo_hier_t *H, int level, int box);   /* level 0, box 0 = the base level */
/* the boxes of level `level` >= 1 as the hierarchy was created with them: 4 x suhmo_hier_num_boxes(H, level) ints (lo0, lo1, hi0, hi1) -- what a
 * caller needs of a handle it did not create itself (the one a regrid inside suhmo_hier_run leaves) */
int suhmo_hier_get_boxes(const suhmo_hier_t *H, int level, int *boxes);
/* the rank that owns box `box` of a level dealt to the ranks (partition_min_cells), -1: every rank holds it (a replicated level, level 0's
 * strip), -2: no such box; *held (may be NULL): this rank keeps storage for it -- its own box or a mirror; load and read a box where it is
 * owned (a mirror's cells are overwritten by its owner's; a box that is not held refuses field access with rc -7) */
int suhmo_hier_box_owner(const suhmo_hier_t *H, int level, int box, int *held);
int suhmo_hier_exchange(suhmo_hier_t *H, int level, int field, int corners, suhmo_stream_t s);
int suhmo_hier_cf_interp(suhmo_hier_t *H, int level, int field_f, int field_c, suhmo_stream_t s);   /* from level - 1 */
int suhmo_hier_pwl_fill(suhmo_hier_t *H, int level, int field_f, int field_c, suhmo_stream_t s);
int suhmo_hier_average(suhmo_hier_t *H, int level, int field_f, int field_c, suhmo_stream_t s);     /* into level - 1 [AMRRestrictS :1027-1069] */
int suhmo_hier_gsrb(suhmo_hier_t *H, int level, int sweeps, suhmo_stream_t s);                      /* relax of one level */
int suhmo_hier_update_operator(suhmo_hier_t *H, int level, suhmo_stream_t s);
int suhmo_hier_residual(suhmo_hier_t *H, double *norm, suhmo_stream_t s);
int suhmo_hier_vcycle(suhmo_hier_t *H, const suhmo_solver_params_t *sp, suhmo_stream_t s);
int suhmo_hier_solve(suhmo_hier_t *H, const suhmo_solver_params_t *sp, int *iters, double *resid_hist, suhmo_stream_t s);
/* suhmo_amr_timestep / suhmo_amr_moulin_source on a hierarchy of box unions (AmrHydro::timeStepFAS with m_finest_level > 0,
 * Calc_moulin_integral over all levels): the phases of suhmo_level_timestep on every box, exchange() between the boxes of a
 * level after every ghost fill, PiecewiseLinearFillPatch / QuadCFInterp from the level below, SolveForHead_nl = suhmo_hier_solve,
 * gap height by forward Euler or (use_impl_diff) SolveForGap_nl over a second hierarchy of the same boxes. */
int suhmo_hier_timestep(suhmo_hier_t *H, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles,
                        suhmo_stream_t s);
int suhmo_hier_moulin_source(suhmo_hier_t *H, int n_moulins, const double *positions, const double *sigma, const double *flux,
                             double time_factor, double *integrals, suhmo_stream_t s);

/* ---- GRID GENERATION: from tagged cells to the box lists suhmo_hier_create takes (suhmo_amd/csrc/suhmo_tags.hip).  The
 * reference grids every AMR run this way: AmrHydro::initGrids (src/AmrHydro.cpp:4835-4955) and regrid (:4227-4511) tag cells by a threshold on a
 * field (tagCellsLevel, :4539-4604) and hand the tags to BRMeshRefine with fill_ratio, block_factor, nestingRadius and max_box_size.
 *
 * TAGGING (device).  suhmo_hier_tag_cells accumulates into the tag map of level `level` (0 .. nlev - 1) of a hierarchy, suhmo_level_tag_cells
 * into that of a single level handle (level 0, the first pass of initGrids).  A VALID cell of any box of the level is tagged when
 * vmin < value && value < vmax -- both strict, so a NaN tags nothing; ghost cells are never read; cells under a finer level are tagged like
 * the others.  field: any SUHMO_F_* the level holds (the reference's tag variables: meltingRate = SUHMO_F_MR, GapHeight = SUHMO_F_B,
 * Pi = SUHMO_F_PI, Qx = SUHMO_F_QWX; a face field is read at the low face of the cell; a field the level does not hold yet is allocated, zero, as on any first use).  A tag grows
 * to the square of `grow` cells around it (Chebyshev, IntVectSet::grow, tags_grow), then further by grow_x - grow / grow_y - grow in a
 * direction whose value exceeds grow (tags_grow_dir), and is clipped to the level's domain box in BOTH directions.  DEVIATION from the
 * reference's `&= ProblemDomain`: no periodic wrap -- a grown tag that leaves a periodic side is dropped, not carried to the other side (the
 * nesting margins of suhmo_grids_generate do wrap).  Several calls form the union (a_tags |= local_tags); suhmo_hier_clear_tags /
 * suhmo_level_clear_tags empty the map (level < 0: every level's).
 * The map is kept at `granularity` g >= 1 cells of the level per entry, row-major [nby][nbx] with nbx = ceil(nx / g), nby = ceil(ny / g): an entry is
 * 1 when any grown tag lies in it, whichever box (or none) holds its cells.  g = block_factor / 2 is the size, in this level's cells, of one
 * block of the level to be generated.  A map in use keeps its granularity: another g before a clear is rc -1.
 * MEMORY: ONE BYTE PER ENTRY on the device, allocated on first use, owned by the handle and freed with it: 2 x 2^l x nx0 x ny0 / g^2 bytes
 * for level l.  The reference's run_C_3lev (256 x 256 base, block_factor 2, so g = 1) costs 64 KiB + 256 KiB (+ 1 MiB with a third refined
 * level); cfg5 at the 4096 x 4096 north-star base with three refined levels costs 256 MiB for its finest tag level (level 2: 16384 x 16384
 * entries at g = 1), 64 MiB and 16 MiB for the two below.  The kernels store the byte 1 with plain vector stores (every writer of an entry stores
 * the same value).  suhmo_*_get_tags copies a map out: host may be NULL (sizes only); a level without a map reports 0 x 0.
 * Rank strips: rc -5 (a strip's map would be a part of the level's; not built).
 *
 * BOX GENERATION (host; needs no device).  suhmo_grids_generate turns tag maps into box lists by Berger-Rigoutsos clustering.  Chombo's
 * BRMeshRefine is in the un-vendored fork: the algorithm below is restated from Berger & Rigoutsos (1991), UNPINNED against the reference
 * (SURVEY.md Appendix E).  tags[l], l = 0 .. ntag - 1: the map of level l at granularity block_factor / 2, of
 * (nx0 << l) / g x (ny0 << l) / g entries (g must divide nx0 and ny0).  block_factor: a power of two >= 2; max_box_size: a positive
 * multiple of block_factor; fill_ratio in (0, 1]; nesting_radius below 2 is RAISED TO 2, the margin suhmo_hier_create demands.
 * Top-down, as BRMeshRefine::regrid with base level 0: for l = ntag - 1 down to 0, tags[l] first receives every entry touched by
 * coarsen(grow(coarsen(box), nesting_radius)) of each box already generated on level l + 2 (inner coarsen: to cells of level l + 1, outer: to
 * level l; a cell that leaves a periodic side wraps, one that leaves a non-periodic side is dropped), then level l + 1 is generated from it --
 * every tagged entry is covered by a box, so the proper-nesting rule of suhmo_hier_create holds by construction.  Levels above the first
 * level without tags are dropped.  Per level, in block units on the bounding rectangle of the tags, make(R): shrink R to the bounding box of
 * its tags (none: return); emit R when tagged / area >= fill_ratio and both sides <= max_box_size / block_factor; else split by the first
 * rule that applies to the signatures Sx (column sums), Sy (row sums) -- (a) a hole S = 0, per direction the one nearest the centre (tie: lower
 * index), the longer side's first (tie: x), else the other's: [lo, i-1] + [i+1, hi]; (b) an inflection, D[i] = S[i-1] - 2 S[i] + S[i+1] for
 * lo < i < hi, between i and i+1 where D[i] D[i+1] < 0 with strength |D[i] - D[i+1]|, per direction the strongest (ties: nearest the centre, then
 * lower index), of the two the stronger (ties: longer side, then x): [lo, i] + [i+1, hi]; (c) bisect the longer side (tie: x) into floor(len/2)
 * and the rest -- and recurse on the lower part first.  Boxes come in emission order: deterministic.  A box (I0, J0, I1, J1) in blocks is
 * (I0 b, J0 b, (I1+1) b - 1, (J1+1) b - 1) in cells of level l + 1.
 * Output as suhmo_hier_create takes it: *nlev_out = levels including level 0, nbox[0 .. *nlev_out - 1] (nbox[0] = 0; the array must hold ntag + 1
 * ints), boxes = (lo0, lo1, hi0, hi1) one after the other, level 1 first.  rc -1: a bad parameter, ntag < 1 or > 7; rc -4: boxes_cap (in
 * boxes) too small -- nbox[] and *nlev_out are still set and the message names the needed count, so a second call can succeed.
 *
 * THE REST OF tagCells (src/AmrHydro.cpp:4514-4536): subset boxes and per-variable level ranges.
 * suhmo_hier_restrict_tags(H, level, nboxes, boxes, s) is `levelTags &= tagSubset` (:4530-4533, AmrHydro.tagSubsetBoxesFile): every entry of the
 * level's tag map that lies in none of the boxes (lo0, lo1, hi0, hi1 in cells of that level, HOST array; they may overlap and may reach beyond
 * the domain) is cleared -- entry (a, b) of a map at granularity g lies in a box when lo0 <= a g <= hi0 and lo1 <= b g <= hi1.  One launch: one
 * thread per entry, the box list in device memory (owned by the map), plain byte stores of 0.  nboxes == 0: a no-op, rc 0 (the reference skips
 * an empty subset); a level without a map: rc 0, nothing to do; a box with lo > hi, or whose lo or hi + 1 is not a multiple of g (an entry must
 * lie wholly inside or wholly outside): rc -1 and nothing is cleared; rank strips: rc -5.  Tagging after a restrict accumulates again.
 * suhmo_tag_subsets_nest (host; no device) builds the per-level subsets the way the reference does when it reads the file (:1097-1108): input
 * nbox[l] boxes per level l = 0 .. nlev - 1, one after the other in `boxes`; for l = 1, 2, ... in this order, with C = the NESTED subset of level
 * l - 1, every box (lo0, lo1, hi0, hi1) -> (2 lo0, 2 lo1, 2 hi0 + 1, 2 hi1 + 1): C empty: level l keeps its own; else level l's own empty: it becomes C;
 * else it becomes the non-empty pairwise intersections own[a] x C[c], a outer, c inner (none: the subset is empty and constrains nothing).
 * Output like the input; rc -4 when boxes_cap (in boxes) is too small, nbox_out set and the needed count in the message.
 * A tag variable m has a level range (AmrHydro.tagging_mins / tagging_caps): it tags the levels max(min_level, 0) .. min(cap_level, max_level - 1,
 * finest level) (:4521-4527), and the subset of a level is applied after each variable's tagging of it, on the accumulated map (suhmo_tag_spec_t
 * and suhmo_hier_run below; HipHierModel.tag_and_regrid is the same loop over these calls).
 *
 * BOTH.  suhmo_hier_generate_grids copies out the tag maps of the levels 0, 1, ... of H that have one (up to the first without; their
 * granularity must be block_factor / 2: rc -1; no map on level 0: rc -1) and calls the generator with the hierarchy's base size and
 * periodicity.  *same (may be NULL) = 1 when the generated hierarchy has H's number of levels and every level holds the same SET of boxes, in
 * any order (gridsSame, :4278-4296).  A hierarchy on rank strips: rc -5.  No fields move here: suhmo_hier_regrid (below) carries a state to
 * the new grids; initGrids loads the initial state instead. */
typedef struct suhmo_grid_params { double fill_ratio; int block_factor, max_box_size, nesting_radius; } suhmo_grid_params_t;
int suhmo_hier_tag_cells(suhmo_hier_t *H, int level, int field, double vmin, double vmax, int grow, int grow_x, int grow_y, int granularity,
                         suhmo_stream_t s);
int suhmo_hier_clear_tags(suhmo_hier_t *H, int level);
int suhmo_hier_get_tags(suhmo_hier_t *H, int level, unsigned char *host, int *nbx, int *nby);
int suhmo_level_tag_cells(suhmo_level_t *L, int field, double vmin, double vmax, int grow, int grow_x, int grow_y, int granularity,
                          suhmo_stream_t s);
int suhmo_level_clear_tags(suhmo_level_t *L);
int suhmo_level_get_tags(suhmo_level_t *L, unsigned char *host, int *nbx, int *nby);
int suhmo_grids_generate(int nx0, int ny0, const int periodic[2], const suhmo_grid_params_t *p, int ntag, const unsigned char *const *tags,
                         int *nlev_out, int *nbox, int *boxes, int boxes_cap);
int suhmo_hier_generate_grids(suhmo_hier_t *H, const suhmo_grid_params_t *p, int *nlev_out, int *nbox, int *boxes, int boxes_cap, int *same);
int suhmo_hier_restrict_tags(suhmo_hier_t *H, int level, int nboxes, const int *boxes, suhmo_stream_t s);
int suhmo_tag_subsets_nest(int nlev, const int *nbox, const int *boxes, int *nbox_out, int *boxes_out, int boxes_cap);

/* ---- REGRID: FIELD TRANSFER (suhmo_amd/csrc/suhmo_regrid.hip; tests/regrid_ref.py is the numpy twin of this text).
 * The third step of AmrHydro::regrid (src/AmrHydro.cpp:4227-4511) after tagging and clustering: destructiveRegrid (:4176-4223) for refinement
 * ratio 2.  Level 0 is the domain and never changes (m_regrid_lbase = 0, the only value the reference ships): its fields are carried over
 * unchanged.  Per level l = 1 .. new finest, ASCENDING, so that level l reads the NEW level l - 1 with all its steps done, and per field:
 *  a. INTERPOLATE every valid cell of every new box of level l from level l - 1 -- FineInterp::interpToFine with m_boundary_limit_type = 3,
 *     limitTangentialOnly.  For the coarse cell (I, J) under the fine cells (2I + p, 2J + q), p, q in {0, 1}, c(a, b) the coarse value at
 *     (I + a, J + b), c0 = c(0, 0):
 *       neighbours  (I + a, J + b) EXISTS if it lies in the coarse domain after the wrap through a periodic side; proper nesting makes every
 *                   existing neighbour a valid cell of level l - 1.
 *       slopes      s[d] as oracle/amr_step_m.c:or_pwl_fill and k_pwl compute them: central 0.5 * (c(+1) - c(-1)) when both neighbours in
 *                   direction d exist, c(+1) - c0 when the low one does not, c0 - c(-1) when the high one does not (neither: 0).
 *       limiter     FORT_INTERPLIMIT, or_pwl_fill's arithmetic: smax, smin over the existing cells of the 3 x 3 block (c0 included);
 *                   deltasum = 0.5 * (|s0| + |s1|); where deltasum > 0: etamax = (smax - c0) / deltasum, etamin = (c0 - smin) / deltasum,
 *                   eta = max(min(min(etamin, etamax), 1), 0).
 *       where       a cell with all eight neighbours: both slopes times eta.  A cell that lacks a neighbour in the directions N != {} (next to
 *                   a non-periodic domain side): eta on the slopes of the directions NOT in N only; the one-sided normal slopes stay as
 *                   computed (at a domain corner, N = both: nothing is limited).  eta itself is the value above, normal slope included in
 *                   deltasum: a tangential slope larger than half the normal range is still cut.
 *       value       v = c0; v = v + s0 * (p ? 0.25 : -0.25); v = v + s1 * (q ? 0.25 : -0.25) -- this order, separate statements, no
 *                   contraction, as k_pwl is written.
 *     [Chombo] FineInterp.cpp is in the un-vendored fork.  Away from the domain sides the arithmetic is exactly or_pwl_fill's, which the test
 *     oracle pins; the BOUNDARY CLAUSE ("where", and one-sided slopes that escape the limiter) is restated from the documented meaning of
 *     limitTangentialOnly and is UNPINNED against the reference, as BRMeshRefine is.
 *  b. COARSE-FINE GHOST CELLS of the new boxes: PiecewiseLinearFillPatch from the new level l - 1 (suhmo_hier_pwl_fill: corners included, no
 *     periodic images in its stencil, both slopes limited).
 *  c. COPY: every valid cell of a new box that is a valid cell of some old box of level l gets the old value, bit for bit
 *     (a_oldData->copyTo(*newData)); the copy wins over (a).  Only old VALID cells are read, never an old ghost cell.  A level the old
 *     hierarchy does not have contributes nothing; a level the new one does not have is dropped (:4462-4467).
 *  d. EXCHANGE between the new boxes, corners included (suhmo_hier_exchange).
 *  e. DOMAIN GHOST CELLS across a non-periodic side, side cells only, by the rule the reference's regrid applies to the field and with the
 *     launches of the time step: CopyGhostCells (ghost = the cell next to it) for SUHMO_F_ZB and SUHMO_F_MASK (:4419, :4436) and for
 *     SUHMO_F_B (the time step's own ghost fill of b); ExtrapGhostCells (ghost = 2 x the cell next to it - the one behind) for SUHMO_F_PI,
 *     SUHMO_F_ZS, SUHMO_F_MR, SUHMO_F_PW (:4379-4383, :4420-4421); the head's are the solver's business and every other field's are left as
 *     created (0).  Ghost cells diagonal to a domain corner are written by nobody.
 *
 * suhmo_hier_regrid(H, nlev, nbox, boxes, nfields, fields, out, s): nlev / nbox / boxes exactly as suhmo_hier_create takes them, so the output of
 * suhmo_hier_generate_grids passes straight in.  fields: nfields (<= 16) ids of cell-centred fields (a face field, SUHMO_F_COVER or
 * SUHMO_F_PHI2: rc -1); NULL = the reference's list (:4363-4376) restricted to what is held as arrays here: PHI, B, PI, ZB, MASK, MR, PW, ZS.
 * A field a level does not hold yet is allocated, zero, as on any first use.  Every other field of the levels >= 1 starts as in a freshly
 * created hierarchy (the reference allocates m_old_head, m_Re, m_qw, the moulin source term and the gradients anew); the next
 * suhmo_hier_moulin_source / suhmo_hier_timestep recomputes them.  The new hierarchy gets the base descriptor, the options and the all-gather
 * callback of the old one.
 * OWNERSHIP: *out ADOPTS the base level handle of H -- level 0 with its multigrid depths is neither copied nor re-created, and
 * suhmo_hier_box(*out, 0, 0) is the handle suhmo_hier_box(H, 0, 0) was -- and H IS CONSUMED: destroyed on success (its boxes, plans, tag
 * maps and the gap-height hierarchy of its time step go with it; the base level forgets what it knew about its ice mask and drops its
 * captured V-cycles).  When the call fails *out = NULL and H is untouched and usable; lists suhmo_hier_create refuses (bad nesting,
 * misaligned or overlapping boxes, ...) give suhmo_hier_create's return code and message.  A hierarchy on rank strips, with levels dealt
 * to the ranks or created with shadow = 1: rc -5.  The call synchronises the device.
 * MEMORY of the plans, per level and only for the duration of the call: 32 B per pair (new box, box of level l - 1) that intersect + 24 B
 * per pair (old box, new box) that intersect.  Not built: m_regrid_lbase > 0, refinement ratios other than 2, rank strips. */
int suhmo_hier_regrid(suhmo_hier_t *H, int nlev, const int *nbox, const int *boxes, int nfields, const int *fields, suhmo_hier_t **out,
                      suhmo_stream_t s);

/* ---- THE RUN OF A HIERARCHY (suhmo_amd/csrc/suhmo_run.hip, suhmo_forcing.hip, suhmo_postproc.hip): what AmrHydro::run (src/AmrHydro.cpp:1283-1365)
 * does around timeStepFAS, for a hierarchy of box unions.
 * suhmo_hier_time_varying_recharge   suhmo_level_time_varying_recharge on every box (timeStepFAS evaluates COMPUTE_TIMEVARYINGRECHARGE level by
 *     level, :2846-2863): SUHMO_F_MSRC of every box, ghost ring included, bit for bit what the level call on that box's handle writes.  ONE launch
 *     for level 0 and ONE per refined level (read-only option recharge_launches counts them), never one per box.  No averaging down and no
 *     coarse-fine fill: the reference does neither for this source (:2854-2863, unlike the moulins', :2818-2839).  Checked before anything is
 *     launched: a box that does not hold SUHMO_F_ZS: rc -1, the message names level and box; a hierarchy on rank strips or with levels dealt to
 *     the ranks: rc -5.
 * suhmo_hier_postproc_temporal   the daily row: the reference evaluates it on level 0 ("POST PROC -- 1 LEVEL", :3643-3700) --
 *     suhmo_level_postproc_temporal_device on suhmo_hier_box(H, 0, 0), its bits and its refusals; rank strips: rc -5.
 * suhmo_hier_run   the time loop in one call.  For step k = 0 .. n_steps - 1 with c = first_cur_step + k (cur_step of suhmo_hier_timestep):
 *   1. REGRID when regrid_interval > 0, c - 1 != 0 and (c - 1) % regrid_interval == 0 (:1317; c - 1 is m_cur_step before its increment), except at
 *      k = 0 when skip_first_regrid is set (the reference's m_cur_step != m_restart_step).  suhmo_hier_clear_tags(-1); for every tag variable m, in
 *      order, for l = max(min_level, 0) .. min(cap_level, max_level - 1, finest level): suhmo_hier_tag_cells(l, field, vmin, vmax, grow, grow_x,
 *      grow_y, grid.block_factor / 2), then, when subset_nbox[l] > 0, suhmo_hier_restrict_tags(l) with the boxes of that level (subset_boxes: level
 *      0's first; the caller has nested them, suhmo_tag_subsets_nest); suhmo_hier_generate_grids; when *same is 0, suhmo_hier_regrid with
 *      n_fields / fields (NULL: its default list).  After such a grid-changing regrid *H is the new handle and reload(user, *H, index of the regrid
 *      in the log, c) is called -- the place of initializeBed / initializePi / setup_iceMask (:4387-4437): it loads through the ordinary per-box
 *      calls.  When *same is 1 the handle and every view stay.
 *   2. FORCING.  With T_K: the recharge launches above with T_K[k], background[k], every step.  With moulins: suhmo_hier_moulin_source with the
 *      factor f[k] = moulin_factor[k] (NULL: 1.0), but only when k = 0, or a grid-changing regrid happened in this step's (1), or the bits of f[k]
 *      differ from those of f[k - 1] -- the reference's m_regrid rule (:2802) plus a factor that can change.  Both kinds at once: rc -1.
 *   3. suhmo_hier_timestep with *mp, ramp = ramp[k] when ramp is given, dt, cur_step = c.
 *   4. When diag_every > 0 and (k + 1) % diag_every == 0: the column sums of level 0 and the row of suhmo_hier_postproc_temporal finished ON THE
 *      DEVICE into a series [rows][6]: no copy and no synchronisation per row.
 * After the last step the series comes back in ONE copy (read-only option run_readbacks counts it; moulin_source_calls counts (2)'s calls; a run
 * carries the three counters of this section over its regrids).  Every field of every box, every count and every row is bit for bit what the
 * same sequence of the public calls gives.  The schedule carries VALUES, all HOST arrays.
 * res: steps_done, n_rows; picard_iters / vcycles [n_steps] (may be NULL); rows [n_steps / diag_every][6] (may be NULL when there are none);
 * moulin_steps [n_steps] (may be NULL): 1 where (2) formed the moulin source; n_regrids = regrids done, the first regrids_cap of them logged in
 * regrids (may be NULL): cur_step = c, same, nlev and nbox[l] of the generated lists (nbox[0] = 0); n_moved = those of them with same = 0, i.e. how
 * often *H became a new handle.  A regrid whose lists suhmo_hier_create refuses is neither logged nor counted: the hierarchy is the old one.
 * THE SURFACE HEIGHT ACROSS A REGRID: with T_K the new boxes must hold SUHMO_F_ZS before the next recharge launch.  They do when `fields` is NULL
 * or lists SUHMO_F_ZS (the transfer brings it), or when `reload` loads it on EVERY new box; after a grid-changing regrid and its `reload` every
 * box is checked again, and a box without it ends the run there with rc -1 (the message names level and box), nothing launched on the new
 * hierarchy, steps_done = the steps completed and *H the new handle.
 * A failing step, a list suhmo_hier_create refuses, or a reload that returns non-zero ends the run with that call's rc (reload: rc -1, its value
 * in the message): steps_done = the steps completed, the rows so far copied out, and *H a usable hierarchy -- the old one when the regrid
 * failed, the new one otherwise.  Checked before anything is launched, rc -1 (rank strips, levels dealt to the ranks: -5) and a message:
 * n_steps < 1, dt <= 0, first_cur_step < 1, diag_every < 0; T_K without background or the reverse; an incomplete set of moulin arrays (n_moulins
 * >= 1 with positions, sigma > 0, flux; or none of them), both kinds of forcing; regrid_interval < 0, regrid_interval > 0 without tags, with
 * max_level outside 1 .. 8, with grid parameters suhmo_grids_generate refuses (its rc), with a bad tag field or reach, with a subset box not
 * aligned to block_factor / 2; SUHMO_F_ZS missing where T_K is given; use_moulin_source without any forcing and without a source term on
 * some box; use_impl_diff with diffFactor = 0; rows without an array for them, or a level 0 suhmo_hier_postproc_temporal refuses.
 * Eager launches as in suhmo_batch_run; no graph capture.  Not built: rank strips. */
typedef struct suhmo_tag_spec { int field; double vmin, vmax; int grow, grow_x, grow_y; int min_level, cap_level; } suhmo_tag_spec_t;
typedef int (*suhmo_hier_reload_fn)(void *user, suhmo_hier_t *Hnew, int regrid_index, int cur_step);
typedef struct suhmo_hier_schedule {
    int n_steps; double dt; int first_cur_step;
    const double *T_K, *background;            /* [n_steps] each, or both NULL */
    int n_moulins; const double *positions, *sigma, *flux;   /* once for the run, or n_moulins = 0 and all NULL */
    const double *moulin_factor;               /* [n_steps] or NULL (= 1.0) */
    const double *ramp;                        /* [n_steps] or NULL */
    int diag_every;                            /* 0: no rows */
    int regrid_interval, skip_first_regrid, max_level;       /* regrid_interval 0: never regrid; max_level: AmrHydro.max_level, levels above 0 at most */
    int n_tags; const suhmo_tag_spec_t *tags; suhmo_grid_params_t grid;
    const int *subset_nbox, *subset_boxes;     /* per level 0 .. max_level - 1, or both NULL */
    int n_fields; const int *fields;           /* as suhmo_hier_regrid */
    suhmo_hier_reload_fn reload; void *user;   /* or NULL */
} suhmo_hier_schedule_t;
typedef struct suhmo_hier_regrid_log { int cur_step, same, nlev; int nbox[8]; } suhmo_hier_regrid_log_t;
typedef struct suhmo_hier_run_result {
    int steps_done, n_rows;
    int *picard_iters, *vcycles;               /* [n_steps], may be NULL */
    double *rows;                              /* [n_steps / diag_every][6] */
    int *moulin_steps;                         /* [n_steps], may be NULL */
    int n_regrids, regrids_cap;
    suhmo_hier_regrid_log_t *regrids;          /* [regrids_cap], may be NULL */
    int n_moved;                               /* regrids that moved the hierarchy onto other boxes (*H changed n_moved times) */
} suhmo_hier_run_result_t;
int suhmo_hier_time_varying_recharge(suhmo_hier_t *H, double T_K, double background_input, suhmo_stream_t s);
int suhmo_hier_postproc_temporal(suhmo_hier_t *H, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s);
int suhmo_hier_run(suhmo_hier_t **H, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, suhmo_hier_run_result_t *res,
                   suhmo_stream_t s);

/* ---- SNAPSHOT (suhmo_amd/csrc/suhmo_snap.hip; DESIGN.md section 5, "Output of a run"; tests/snapshot_ref.py is the numpy twin of this text): a list of
 * fields of a whole hierarchy gathered on the device into the order Chombo writes a LevelData to disk -- what AmrHydro::writePlotFile and
 * writeCheckpointFile (src/AmrHydro.cpp:5474-5667, 5670-5842) hand to HDF5 -- with ONE launch and ONE copy per level, whatever the number of boxes.
 * LAYOUT.  Per level the boxes come in the hierarchy's order; level 0 is the single box (0, 0, nx0 - 1, ny0 - 1).  Box k grown by `ghost` (0 or 1)
 * is ncomp x (ny_k + 2 ghost) x (nx_k + 2 ghost) doubles ordered [comp][j][i], i fastest; boxes follow one another and levels follow one another.
 * A level's slice is exactly the "data:datatype=0" dataset of a Chombo LevelData with ncomp components.  box_offset holds, per level, the nbox + 1
 * prefix sums in doubles (the "data:offsets=0" dataset; total boxes + nlev entries in all, level 0's two first); level_offset[l] is where level l
 * starts in host_dst and level_offset[nlev] the doubles in all.  host_dst == NULL fills the offsets only: nothing is launched and the device is
 * not touched.
 * COMPONENTS (at most SUHMO_SNAP_MAX_COMPS), each {kind, field, value}:
 *   SUHMO_SNAP_FIELD         a cell-centred SUHMO_F_*: bit for bit what suhmo_level_get_field with ghosted = 1 returns for that box, ghost ring included
 *                            (its interior for ghost = 0) -- the head wherever the relaxation left it, on either of its two canvases.  A field the box does
 *                            not hold is written as 0.0; nothing is allocated: a snapshot does not change what a box holds.
 *   SUHMO_SNAP_FACE_TO_CELL  a face field (QWX, QWY, BX, BY, DCX, DCY) averaged to cells as EdgeToCell does, 0.5 * (lo + hi), in VALID cells; ghost cells are
 *                            0.0.  This is m_qw of src/AmrHydro.cpp:3281-3287 before its ghost fills.  DEVIATION: the reference fills the ghost cells of
 *                            Qw_x / Qw_y before it plots them (:3290-3300); here they stay 0.0.
 *   SUHMO_SNAP_CONST         `value` everywhere.
 * One body and one kernel template over the launch target: level 0 (and suhmo_level_snapshot: a single level handle, whole, as the one box) as a
 * level, every refined level as one launch over its boxes, blockIdx.z = box.  The component list travels by value; the per-box offsets are a device
 * table the hierarchy owns.  Thread (i, j) loops over the components: loads and stores are contiguous in i.  Plain vector stores.  Each level goes
 * into a device staging buffer and from there in one hipMemcpyAsync into host_dst; one stream synchronisation ends the call.  Read-only options
 * snapshot_launches and snapshot_copies count them (nlev each per snapshot); a run carries them over its regrids.
 * MEMORY.  The staging is the largest level's packed size over the snapshots so far, allocated on first use, owned by the hierarchy and freed with
 * it.  13 components with ghost 1 cost 6.9 MB for a 256 x 256 base and 1.75 GB for the 4096 x 4096 base (level 0's packed size; a refined level
 * whose boxes hold more cells than level 0 costs what they hold).  A caller who cannot afford that snapshots fewer components per call.  suhmo_level_snapshot allocates its
 * staging for the call.  The per-box offset tables: 8 B per box and ghost width.
 * REFUSED before anything is launched, host_dst untouched.  rc -1: ncomp outside 1 .. 16, ghost other than 0 or 1, an unknown kind, a field id out
 * of range, a face field as SUHMO_SNAP_FIELD or a cell field as SUHMO_SNAP_FACE_TO_CELL, SUHMO_F_COVER / SUHMO_F_PHI2 named directly.  rc -5: a rank
 * strip, levels dealt to the ranks, a hierarchy created with shadow = 1. */
enum { SUHMO_SNAP_FIELD = 0, SUHMO_SNAP_FACE_TO_CELL = 1, SUHMO_SNAP_CONST = 2 };
#define SUHMO_SNAP_MAX_COMPS 16
typedef struct suhmo_snap_comp { int kind, field; double value; } suhmo_snap_comp_t;
int suhmo_hier_snapshot(suhmo_hier_t *H, int ncomp, const suhmo_snap_comp_t *comps, int ghost, long *level_offset /* [nlev + 1] */,
                        long *box_offset /* [total boxes + nlev] */, double *host_dst, suhmo_stream_t s);
int suhmo_level_snapshot(suhmo_level_t *L, int ncomp, const suhmo_snap_comp_t *comps, int ghost, long *ndoubles, double *host_dst, suhmo_stream_t s);

/* ---- FLATTEN (suhmo_amd/csrc/suhmo_flatten.hip; DESIGN.md section 5, "Comparison of runs"; tests/flatten_ref.py is the numpy twin of this text): a
 * hierarchy interpolated onto ONE uniform grid at the resolution of level max_level -- AmrHydro::interpFinest (src/AmrHydro.cpp:4623-4829, called
 * at :3648-3650 with post_proc_comparisons), the composite writePltPP (:5298-5389) writes so that an AMR run is compared cell by cell with the
 * uniform run and with other AMR depths.
 * COMPONENTS (at most SUHMO_FLAT_MAX_COMPS), each {kind, field, field2}:
 *   SUHMO_FLAT_FIELD   a cell-centred SUHMO_F_* (the head wherever the relaxation left it, on either of its two canvases).
 *   SUHMO_FLAT_DIFF    field - field2, formed in the cells of each level BEFORE the interpolation: the reference interpolates N = Pi - Pw, not Pi
 *                      and Pw, and the limiter is not linear.  The reference's two plotted components are {FIELD, B} and {DIFF, PI, PW}.
 *   A field a box does not hold counts as 0.0 there; nothing is allocated for it (the snapshot's rule).
 * OUTPUT.  ncomp x nyF x nxF doubles ordered [comp][j][i], nxF = nx0 << max_level, nyF = ny0 << max_level: exactly one box with ghost 0 in the
 * layout suhmo_plt_write_level takes for a level.  dims = {nxF, nyF}; host_dst == NULL fills dims only: nothing is launched and the device is not
 * touched.  All offsets are long (32768 x 32768 cells times 16 components is beyond an int).
 * ARITHMETIC.  Levels l = 0 .. finest level in ASCENDING order, a finer level overwriting what a coarser one wrote (copyTo, :4769-4771).  With
 * r = 2^(max_level - l), every valid cell (I, J) of level l with value c0 gives its r x r children (r I + p, r J + q), p, q = 0 .. r - 1:
 *       v = c0; v = v + s0 * dx_p; v = v + s1 * dy_q        with dx_p = -0.5 + (p + 0.5) / r, dy_q = -0.5 + (q + 0.5) / r
 * -- this order, separate statements, multiply and add NOT contracted (for r >= 4 the offsets are no longer powers of two).  This is
 * FineInterp::interpToFine with the whole ratio in ONE shot (:4692-4697, :4761-4765), not an iteration of ratio 2.  s0, s1 and the limiter are
 * rule (a) of "REGRID: FIELD TRANSFER" above statement by statement: central or one-sided slopes, smax / smin over the existing cells of the
 * 3 x 3 block, eta, and limitTangentialOnly next to a non-periodic domain side.  r = 1 is a copy.
 * NEIGHBOURS of a cell of level l: across a non-periodic domain side the neighbour does not exist; in another box of the level, or across a
 * periodic side, it is that box's VALID value; inside the domain but held by no box of the level (l >= 1: the EDGE CLAUSE) it is the
 * PiecewiseLinearFillPatch value of the same component from level l - 1 -- rule (b) of the regrid (tests/regrid_ref.py: pwl_cell), computed from
 * the component as evaluated on level l - 1, not from the flattened array.  DEVIATION, [Chombo], UNPINNED: by our reading of upstream Chombo 3.2
 * the reference reads there ghost cells of FineInterp's coarsened copy that nothing has set.
 * READ-ONLY.  The components are evaluated into private scratch canvases (one per component and box, with the box's canvas geometry; allocated on
 * first use, owned by the hierarchy, freed with it; canvas_bytes_level_<l> counts them); the scratch rings are filled by the plans of the regrid's
 * steps (b) and (d) over those canvases.  No field and no ghost ring a time step, a snapshot or a checkpoint reads is written, and the fields' own
 * ghost rings are not inputs.  The finest array lives on the device (ncomp x nyF x nxF doubles, the largest so far, owned by the hierarchy).
 * MEMORY.  Scratch and finest array stay until the hierarchy is destroyed (a regrid makes a new one) or until suhmo_hier_set_option(H,
 * "flatten_release", 1) gives both back at once; the next flatten allocates again.  Read-only option flatten_device_bytes: what they hold now, level
 * 0's scratch included.  A scratch allocation that fails part way gives back what the call took of that level, so that every level's device table
 * lists exactly the slots that exist; option flatten_fail_slot (tests; -1 = off) makes the allocation of that slot on the finest level fail.
 * LAUNCHES per call, on one stream, with nlev levels: nlev (evaluation) + per level l >= 1 [ncomp if the level has coarse-fine ghost cells] +
 * [ceil(ncomp / 2) if it has fine-fine ghost cells, periodic images included] + nlev (interpolation); then ONE hipMemcpyAsync into host_dst and one
 * synchronisation.  Read-only options flatten_launches and flatten_copies count them (they belong to the handle: a regrid starts them at 0).
 * REFUSED before anything is launched, host_dst untouched.  rc -1: ncomp outside 1 .. 16, an unknown kind, a field id out of range, a face field,
 * SUHMO_F_COVER / SUHMO_F_PHI2, max_level below the finest level, max_level so large that nxF or nyF leaves int.  rc -2: the finest array (or the
 * scratch) cannot be allocated; the hierarchy stays usable.  rc -5: a rank strip, levels dealt to the ranks, a hierarchy created with shadow = 1.
 * Not built: the reference's third quantity tau (:4678; std::pow, whose bits on the device are not the host's), flattening inside suhmo_hier_run_out. */
enum { SUHMO_FLAT_FIELD = 0, SUHMO_FLAT_DIFF = 1 };
#define SUHMO_FLAT_MAX_COMPS 16
typedef struct suhmo_flat_comp { int kind, field, field2; } suhmo_flat_comp_t;
int suhmo_hier_flatten(suhmo_hier_t *H, int max_level, int ncomp, const suhmo_flat_comp_t *comps, long dims[2] /* nxF, nyF */, double *host_dst,
                       suhmo_stream_t s);

/* ---- COMPARE (suhmo_amd/csrc/suhmo_compare.hip; DESIGN.md section 5, "Comparison of runs"; tests/compare_ref.py is the numpy twin of this text, of
 * suhmo_compare.h and of suhmo_reduce.h): the composite error of a hierarchy against a finer SINGLE-LEVEL run, reduced on the device to three doubles
 * per component -- L1, L2 and max.  It is the number the reference's convergence tables hold, which CONV_ANA/scripts/launch_comparaison*.py produce
 * with ChomboCompare in two ways: on the levels of the plot file, the exact solution averaged down to each level and covered cells left out
 * (SUHMO_CMP_COMPOSITE), and on the plotCustom composites, cell by cell on the same finest grid (SUHMO_CMP_FINEST).
 * INPUTS.  `exact` is a plain whole level on the hierarchy's device whose valid cells are exactly (nx0 << exact_level) x (ny0 << exact_level),
 * exact_level >= the finest level of H.  comps is the list suhmo_hier_flatten takes: FIELD or DIFF is evaluated on BOTH sides from the same field
 * ids, a DIFF per cell on each side before anything else.  A field a box of H does not hold counts as 0.0 (the flatten's rule); a field `exact`
 * does not hold is refused.
 * COMPOSITE.  For level l, r = 2^(exact_level - l) and w_l = dx_l * dy_l (formed on the host).  For every valid cell of every box whose
 * SUHMO_F_COVER is 0 (a covered cell contributes nothing and the exact cells under it are not read), with c its component:
 *       avg   the exact component over the r x r block under the cell: within a row of the block the r values are added as a PAIRWISE TREE OF
 *             NEIGHBOURS, (x0 + x1) + (x2 + x3), ...; the r row sums are added in ascending row order, starting from the first row's sum; the
 *             result times 1.0 / (r r), which is exact.  r = 1: the value as it is.
 *       e = c - avg;   terms  |e| * w_l,  (e * e) * w_l,  |e|          -- products rounded before the sums, nothing contracted
 * The order of the block is layout-independent and lets a group of r lanes form a row sum with __shfl_xor butterflies from coalesced loads.
 * The three terms are reduced as sum, sum, max in the order of suhmo_reduce.h and nothing else: a first stage per level -- level 0 under CAP_LEVEL;
 * a level of boxes under CAP_BOX with ONE grid for all its boxes, that of the level's largest box extents (max nx, max ny over the boxes), every
 * box leaving that many partials (a workgroup without cells leaves 0.0, 0.0, 0.0) -- the partials one list per level, boxes ascending; the second
 * stage over the lists in ascending level order.  norms[q] = {sum1, sqrt(sum2), max}; the max is exact.  level_terms[l][q] = {sum1, sum2, max}
 * of level l's own second stage (the same rule over that list alone), without the square root.
 * FINEST.  The device part of suhmo_hier_flatten at max_level = exact_level -- its steps (i) to (iii), the same scratch, the same finest array,
 * the same launches (flatten_launches counts them) -- then ONE first stage under CAP_LEVEL over the nyF x nxF array: e = flat - x, the terms as
 * above with w = dx * dy of the exact level.  Nothing but the result is copied: flatten_copies does not move.  level_terms must be NULL.
 * READ-ONLY, like the flatten.  LAUNCHES: COMPOSITE nlev first stages (every component in the one launch of its level) + one final stage; FINEST
 * one first stage + one final stage beside the flatten's.  ONE copy of 3 ncomp doubles (with level_terms: 3 ncomp (1 + nlev)) and ONE
 * synchronisation.  Read-only options compare_launches and compare_copies count them.  The partial buffer belongs to the hierarchy: allocated on
 * first use (compare_device_bytes: what it holds), freed with it; a regrid makes a new handle, which allocates its own.
 * REFUSED before anything is launched, norms untouched.  rc -1: the component checks of the flatten; an unknown mode; level_terms in FINEST;
 * exact NULL; exact_level below the finest level, or so large that the finest grid leaves int; exact's extents other than those above;
 * COMPOSITE with r > 64 on level 0 (exact_level > 6); a field exact does not hold.  rc -2: an allocation fails (the partial buffer; in FINEST
 * the flatten's finest array or scratch); the hierarchy stays usable.  rc -5: H on rank strips, with levels dealt to the ranks or created with
 * shadow = 1; exact a rank strip; exact on another device.
 * Not built: a hierarchy as the exact side, tau, rank strips, comparing inside suhmo_hier_run_out. */
enum { SUHMO_CMP_COMPOSITE = 0, SUHMO_CMP_FINEST = 1 };
int suhmo_hier_compare(suhmo_hier_t *H, suhmo_level_t *exact, int exact_level, int mode, int ncomp, const suhmo_flat_comp_t *comps,
                       double *norms /* [ncomp][3]: L1, L2, max */, double *level_terms /* NULL or [nlev][ncomp][3]: sum1, sum2, max */,
                       suhmo_stream_t s);

/* ---- OUTPUT INSIDE THE RUN (suhmo_amd/csrc/suhmo_run.hip): suhmo_hier_run_out is suhmo_hier_run with the plot files and checkpoints AmrHydro::run
 * writes (src/AmrHydro.cpp:1311-1336, 1343-1358); suhmo_hier_run is the same call with out = NULL.  With b = c - 1, the reference's m_cur_step before
 * step c:
 *   1. PLOT when plot_interval > 0 and b % plot_interval == 0 (:1311) -- b = 0 included: the initial state;
 *   2. the REGRID of suhmo_hier_run's rule 1 (:1317);
 *   3. CHECKPOINT when check_interval > 0, b % check_interval == 0 and b != restart_step (:1327; m_restart_step is 0 in a fresh run, :806);
 *   4. the forcing, the step and the row, as suhmo_hier_run does them.
 * After the last step (:1343-1358), unless no_final is set (a run that another run continues): a plot with cur_step = the last c when plot_interval
 * >= 0 and a checkpoint when check_interval >= 0, each once.  So at a b where all three fall together the plot shows the OLD boxes and the
 * checkpoint the NEW ones.  An interval of -1 switches that kind of output off altogether, 0 leaves only the final file.
 * Each event is one snapshot (ghost 1) of the component list of its kind into a pinned host buffer the run owns, then
 * write(user, *H, kind, cur_step, ncomp, level_offset, box_offset, data) with the current handle (its boxes: suhmo_hier_get_boxes); cur_step is the
 * reference's m_cur_step in the file name, b before a step and the last c after the run.  The pointers are valid during the call only.  The library
 * links no HDF5: writing is the callback's business (suhmo_amd.plotfile, suhmo_amd.checkpoint).  A callback that returns non-zero ends the run with
 * rc -1, its value in the message: steps_done is exact, the rows so far are copied out and *H is usable.  Checked before the first launch, rc -1: an
 * interval below -1; an interval >= 0 without a component list or without a callback; a list the snapshot would refuse (its rc).
 * The plots and checkpoints the last run handed to its callback: read-only options run_plots and run_checkpoints. */
typedef int (*suhmo_hier_output_fn)(void *user, suhmo_hier_t *H, int kind /* 0 plot, 1 checkpoint */, int cur_step /* m_cur_step of the file name */,
                                    int ncomp, const long *level_offset, const long *box_offset, const double *data);
typedef struct suhmo_hier_output {
    int plot_interval, check_interval, restart_step, no_final;
    int n_plot; const suhmo_snap_comp_t *plot;
    int n_check; const suhmo_snap_comp_t *check;
    suhmo_hier_output_fn write; void *user;
} suhmo_hier_output_t;
int suhmo_hier_run_out(suhmo_hier_t **H, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, const suhmo_hier_output_t *out,
                       suhmo_hier_run_result_t *res, suhmo_stream_t s);

/* ---- an ENSEMBLE of N independent models on the same grid, stepped together (suhmo_amd/csrc/suhmo_batch.hip): the
 * reference's SHMIP suites are parameter sweeps on one 320 x 64 level (exec/A_SHMIP ... exec/F_SHMIP), far too small to occupy the device.  Every
 * kernel launch of a batch call serves all members that still have work and ONE read-back per V-cycle carries all their residual norms; each
 * member's results are bit for bit those of running it alone.
 *   suhmo_batch_create    n_members (1 .. 64) whole levels from one descriptor: nx, ny, dx, dy, max_box (hence the depth count), alpha / beta, BC types
 *                         and periodicity are shared (a batch call on members that differ in them fails with rc -1); a descriptor of a rank strip or an AMR patch is refused (rc -5), n_members out of range rc -1,
 *                         no device rc -3
 *   suhmo_batch_create_opts   the same with creation options "key=value,...": bottom_solver=1 -- every V-cycle of the batch (and of the gap batch of
 *                         implicit_gap) ends with Chombo's RelaxSolver after its numBottom relaxes, as level option bottom_solver = 1 does on a member run
 *                         alone, bit for bit: ONE more launch per cycle whatever n_members, one workgroup per active member, each with its own loop
 *                         and break test.  The option changes the results and needs allocations, so it is fixed for the life of the batch.  Only the
 *                         one-launch path exists: a bottom depth of more than 16384 cells (or bottom_one_launch_max_cells) is refused with rc -5 and a
 *                         message naming its size, here and by a call whose max_depth makes such a depth the bottom.  NULL or "": suhmo_batch_create.
 *                         An unknown key or a value other than 0 / 1: rc -1.
 *   suhmo_batch_member    member k as an ordinary level handle, owned by the batch (suhmo_level_destroy on it fails with rc -1): its fields, BC
 *                         VALUES (suhmo_level_set_bc with the shared types) and physics constants are per member, loaded and read through
 *                         suhmo_level_put_box / get_box / set_field / get_field / set_bc / norm / ...
 *   suhmo_batch_set_phys  the physics constants of member k (a level has them from its descriptor only; members are created from one)
 *   suhmo_batch_vcycle    one FAS V-cycle (suhmo_level_vcycle) of the members whose flag in active[n] is not 0 (NULL = all; none: a no-op, rc 0)
 *   suhmo_batch_solve     the AMRMultiGrid::solve loop (suhmo_level_solve) with the stopping rule applied per member: a member that stops leaves
 *                         the launches that follow.  iters[n], residual[n] (may be NULL): cycles and final residual max norm of every member.
 *                         Read-backs: one for the initial norms + one per cycle of the member that runs longest.
 *   suhmo_batch_timestep  suhmo_level_timestep of every member, in lock-step by phase: [I] gap-height ghosts and MG coefficients of all members, [II] Picard
 *                         iterations of the members still iterating (lagged chain, RHS_h, the solve above over exactly those members, ONE read-back
 *                         of all their Picard maxima, the test per member), [III] chain, melt rate, forward-Euler gap update and ghosts of all.
 *                         mp[n]: the model parameters of every member (use_moulin_source, distributed_input, ramp, diffFactor, head_melt_off, eps_picard, ...);
 *                         dt and cur_step are shared.  picard_iters[n], vcycles[n] (may be NULL).  use_impl_diff = 1 on any member: rc -5 unless
 *                         option implicit_gap is 1.  With it, [III] is per member: forward-Euler members as above, the others through
 *                         SolveForGap_nl on a second batch of linear operators the batch owns (created by the first step that needs it; alpha = 1,
 *                         beta = dt x diffFactor of the member, Neumann-0 sides): one launch loads b, the right-hand side and D of all of them, one
 *                         averages D to the coarse depths, the solve above runs with the gap solve's parameters, one launch stores the solution
 *                         (freeze_icefree_gap per member), one fills the ghosts of b.  A batch may mix both kinds; use_impl_diff with diffFactor = 0
 *                         on a member: rc -1.  Moulin sources / recharge: suhmo_level_moulin_source / suhmo_level_time_varying_recharge on the
 *                         member handle, one member at a time, or the calls below for all members at once.
 *   Forcing and diagnostics of all members whose flag in active[n] is not 0 (NULL = all; none: a no-op, rc 0), each with the launches of ONE
 *   member and bit for bit what the per-level call on the member handle gives; a member without a flag keeps its source term and its rows of
 *   the output.  Every flagged member is checked before anything is launched (rc -1 and a message naming the member); a NULL array other than
 *   active (and integrals): rc -1.
 *   suhmo_batch_time_varying_recharge   suhmo_level_time_varying_recharge with T_K[n] and background[n]: SUHMO_F_MSRC of every member from its
 *                         SUHMO_F_ZS, which stays on the device (load it once through the member handle; a member without it: rc -1).  One launch.
 *   suhmo_batch_moulin_source   suhmo_level_moulin_source with a list per member: n_moulins[n], and positions (2 per moulin), sigma, flux and
 *                         integrals (may be NULL) concatenated, member 0 first -- member k's entries follow those of the members before it (a
 *                         member without a flag may give 0, or entries that are skipped); time_factor[n].  n_moulins < 1 or a sigma <= 0 on a
 *                         flagged member: rc -1.  Three launches and one synchronisation; the scratch belongs to the batch.
 *   suhmo_batch_postproc_partial / _temporal / _table   suhmo_level_postproc_partial / _temporal / _table of every member with mp[n]: sums
 *                         [n][8][nx], out [n][6], table [n][nx][8].  One launch and one read-back for all members.  No time step run yet on a
 *                         member, or use_moulin_source without a source term: rc -1.
 *   suhmo_batch_run       the time loop (AmrHydro::run, src/AmrHydro.cpp:1283-1365) of the members whose flag in active[n] is not 0 (NULL = all; none: a
 *                         no-op, rc 0) in ONE call: per step k = 0 .. n_steps - 1 the forcing launches the schedule asks for, the step
 *                         suhmo_batch_timestep runs (mp[n] with the schedule's ramp; cur_step = first_cur_step + k; members without a flag are in none
 *                         of its launches) and, when (k + 1) % diag_every == 0, the column sums and one more launch that finishes the row of
 *                         suhmo_batch_postproc_temporal ON THE DEVICE into a series [rows][n][6] -- no copy and no synchronisation per row.  After the
 *                         last step the series comes back in one copy: the diagnostics of a run are ONE read-back in batch_readbacks whatever the
 *                         number of rows.  Every member's fields, counts and rows are bit for bit what the per-call loop gives (recharge or moulin
 *                         call, suhmo_batch_timestep, suhmo_batch_postproc_temporal).  The schedule carries VALUES, all host arrays (the caller
 *                         evaluates the cos / sin of the temperature and the time factor, so they are its bits): see suhmo_batch_schedule_t.
 *                         res: steps_done; picard_iters / vcycles [n_steps][n] (may be NULL; 0 for a member without a flag); rows [n_rows][n][6]
 *                         (n_rows = n_steps / diag_every; the entries of members without a flag keep what the caller put there; may be NULL when
 *                         diag_every = 0).  A step that fails ends the run: its rc, steps_done = the steps completed, the rows written so far
 *                         copied out.  Checked on every flagged member before anything is launched, rc -1 / -5 and a message naming the member:
 *                         SUHMO_F_ZS where a temperature schedule is given, sigma > 0 and non-empty moulin lists, use_moulin_source without a
 *                         source, use_impl_diff against option implicit_gap, bottom_solver of the handles; n_steps < 1, dt <= 0, first_cur_step < 1,
 *                         diag_every < 0, n_members other than the batch's, T_K without background (or the reverse), an incomplete set of moulin
 *                         arrays, both kinds of forcing at once (they write the same source term): rc -1.
 *   suhmo_batch_set_option / get_option   tile_order (0 .. 2, as the level's); bottom_solver: get reports the creation value, set returns 0 for
 *                         that value and rc -5 for the other one (fixed at creation: suhmo_batch_create_opts); implicit_gap (0 / 1, default 0: see
 *                         suhmo_batch_timestep).  Read-only counters: batch_launches, batch_readbacks (both include the gap solves and the calls above),
 *                         batch_member_cycles (V-cycles of head solves summed over the members that ran them), batch_gap_member_cycles (the same for
 *                         the gap solves), bottom_solver_iterations and bottom_solves_one_launch (RelaxSolver's iterations and solves summed over
 *                         the members, the gap solves included; the same keys on a member handle: that member alone).  An unknown key: rc -1.
 *                         Every batch call first checks that bottom_solver of every member handle is the batch's: a member set to the other value
 *                         through suhmo_level_set_option makes the call fail with rc -5 before anything is launched.
 * A batch relaxes every depth with the tile kernel (colour passes where the grid rules it out); eager launches only, no graph capture.
 * Not built: rank strips, AMR patches and hierarchies as members, graph capture of a step or a run, a host-loop RelaxSolver for bottoms the one launch cannot take. */
typedef struct suhmo_batch suhmo_batch_t;
int suhmo_batch_create(suhmo_batch_t **out, const suhmo_level_desc_t *desc, int n_members);
int suhmo_batch_create_opts(suhmo_batch_t **out, const suhmo_level_desc_t *desc, int n_members, const char *options);
int suhmo_batch_destroy(suhmo_batch_t *B);
int suhmo_batch_size(const suhmo_batch_t *B);
suhmo_level_t *suhmo_batch_member(suhmo_batch_t *B, int k);
int suhmo_batch_set_phys(suhmo_batch_t *B, int k, const suhmo_phys_t *phys);
int suhmo_batch_vcycle(suhmo_batch_t *B, const suhmo_solver_params_t *sp, const int *active, suhmo_stream_t s);
int suhmo_batch_solve(suhmo_batch_t *B, const suhmo_solver_params_t *sp, int *iters, double *residual, suhmo_stream_t s);
int suhmo_batch_timestep(suhmo_batch_t *B, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles, suhmo_stream_t s);
int suhmo_batch_time_varying_recharge(suhmo_batch_t *B, const double *T_K, const double *background, const int *active, suhmo_stream_t s);
int suhmo_batch_moulin_source(suhmo_batch_t *B, const int *n_moulins, const double *positions, const double *sigma, const double *flux,
                              const double *time_factor, double *integrals, const int *active, suhmo_stream_t s);
int suhmo_batch_postproc_partial(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *sums, const int *active, suhmo_stream_t s);
int suhmo_batch_postproc_temporal(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *out, const int *active, suhmo_stream_t s);
int suhmo_batch_postproc_table(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *table, const int *active, suhmo_stream_t s);
typedef struct suhmo_batch_schedule {
    int n_steps;
    double dt;
    int first_cur_step;             /* cur_step of the first step (1 for a fresh batch; a second run continues with the first's + its n_steps) */
    int n_members;                  /* the member count the arrays below are laid out for: must be the batch's */
    const double *T_K, *background; /* [n_steps][n] each, or both NULL: one suhmo_batch_time_varying_recharge launch per step */
    const int *n_moulins;           /* [n]; positions, sigma, flux: the members' lists concatenated, as suhmo_batch_moulin_source takes them, given */
    const double *positions, *sigma, *flux;   /* once for the run; or all NULL */
    const double *moulin_factor;    /* [n_steps][n]: the time factor of every step (three launches per step) */
    const double *ramp;             /* [n_steps], or NULL: written into every member's mp.ramp for that step */
    int diag_every;                 /* 0: no rows; else a row after step k when (k + 1) % diag_every == 0 */
} suhmo_batch_schedule_t;
typedef struct suhmo_batch_run_result {
    int steps_done, n_rows;
    int *picard_iters, *vcycles;    /* [n_steps][n], may be NULL */
    double *rows;                   /* [n_steps / diag_every][n][6] */
} suhmo_batch_run_result_t;
int suhmo_batch_run(suhmo_batch_t *B, const suhmo_model_params_t *mp, const suhmo_batch_schedule_t *sch, const int *active,
                    suhmo_batch_run_result_t *res, suhmo_stream_t s);
int suhmo_batch_set_option(suhmo_batch_t *B, const char *key, long value);
int suhmo_batch_get_option(const suhmo_batch_t *B, const char *key, long *value);

/* ---- MASS BALANCE (suhmo_amd/csrc/suhmo_balance.hip; DESIGN.md section 5, "Mass balance"; tests/massbalance_ref.py is the numpy twin of this text,
 * of suhmo_balance.h and of suhmo_reduce.h): AmrHydro::check_fluxes (src/AmrHydro.cpp:440-590), the third part of the post_proc block that ends
 * every timeStepFAS (:3643-3652), reduced on the device to seven doubles per level: the discharge through the four domain sides, the discharge
 * through the ice margin (the "fake EB" faces) and the ice-bearing domain sides, the water volume.
 * A FACE.  The x-face between cell lo = (i - 1, j) and cell hi = (i, j) of a box, I = i0 + i its global face column, nxg the columns of the
 * level's domain; the arithmetic is the reference's, statement by statement, nothing contracted:
 *       area = dy;   gradphi = (phihi - philo) * (-1.0) / dx   (a division, as the reference has it);   flux = -K * gradphi
 *       K            SUHMO_F_BX at that face; the high domain face I = nxg lies in the canvas column right of the last cell
 *       phihi/philo  the head beside the face as phiE / phiW return it with homog = false: the neighbour inside the box, the STORED ghost on a
 *                    box or coarse-fine side, the wrap on a periodic side, the mixBCValues ghost on a physical side -- what the reference's
 *                    m_head holds in its ghost cells after the last solve of the Picard loop (:3157-3164)
 *       mhi/mlo      SUHMO_F_MASK of the two cells, read from the canvas as stored, ghost cells included
 *       mec          as bcoef_face forms it: +-1 where |mhi - mlo| < 1e-10, otherwise 0, and 0 on both domain faces (HydroIBC.cpp:139-184)
 *   where fabs(mec) < 1e-10, with d = mhi - mlo:   d > 0: DIR_X += flux*area;   d < 0: DIR_X -= flux*area;   d == 0 and mhi > 0: += at I == 0,
 *   -= at I == nxg.  Independently: LO_X += flux*area at I == 0, HI_X += flux*area at I == nxg.  The y direction is the same rule with j0, nyg,
 *   area = dx, SUHMO_F_BY and phiN / phiS.  The reference asks no question about periodicity here: a periodic side counts like any other.
 * A CELL.  Where mask > 0: VOLUME += B * dx * dy, multiplied left to right.  m_old_gapheight is not kept on the device: the call reports the volume
 * of the state it is given; the reference's Bold is the same call before the step (tools/mass_balance.py does that).
 * BOXES.  The reference walks all faces of every box, so a face on a side two boxes share is counted by BOTH -- its LO / HI never (such a face is
 * no domain face), its DIR where it is a margin face.  Restated as it is.  Every level is summed whole, covered cells included.
 * ORDER.  That of suhmo_reduce.h and nothing else.  First stage: the walk over the valid cells; the thread of cell (i, j) folds, in this order,
 * its low x-face, its high x-face if i == nx - 1, its low y-face, its high y-face if j == ny - 1, its volume term; each of the seven values has its
 * own accumulator, started at 0.0; the block tree; seven doubles per workgroup.  The grid: CAP_LEVEL for a level or a member of an ensemble; for a
 * level of boxes CAP_BOX on the level's largest box extents, ONE grid for all its boxes, boxes ascending.  Second stage per level / member: thread
 * t takes the partials t, t + 256, ..., then the tree -- so a member's bits are those of the same model run alone, and level 0 of a hierarchy's
 * those of the same level alone.
 * LAUNCHES AND COPIES.  suhmo_level_mass_balance: two launches, one copy of 7 doubles, one synchronisation.  suhmo_hier_mass_balance: nlev first
 * stages + ONE final launch (a workgroup per level), one copy of 7 nlev doubles, one synchronisation; read-only options balance_launches and
 * balance_copies count them, balance_device_bytes is what the partial buffer holds (the hierarchy's: allocated on first use, freed with it; a
 * regrid makes a new handle, which allocates its own).  suhmo_batch_mass_balance: one first stage over the flagged members, ONE final launch (a
 * workgroup per flagged member), one read-back (batch_launches += 2, batch_readbacks += 1); entries of members without a flag keep the caller's.
 * READ-ONLY: nothing a step, a snapshot or a checkpoint reads is written.
 * REFUSED before anything is launched, out untouched, a step afterwards unaffected.  rc -1: a NULL argument; a level (a box, a member) whose face
 * coefficients have never been formed or loaded (no solve, no step, no UpdateOperator has run on it -- after a regrid: on its new boxes).  rc -5: a
 * rank strip; a hierarchy on rank strips, with levels dealt to the ranks or created with shadow = 1; a nested-patch handle (nx_global > 0) passed
 * to the level call.
 * Not built: rank strips, nested patches (suhmo_amr_*), a composite balance with covered cells left out.  Bold kept on the device and the series
 * inside suhmo_hier_run / suhmo_batch_run: "WATER BUDGET" below. */
enum { SUHMO_MB_LO_X = 0, SUHMO_MB_HI_X, SUHMO_MB_LO_Y, SUHMO_MB_HI_Y, SUHMO_MB_DIR_X, SUHMO_MB_DIR_Y, SUHMO_MB_VOLUME, SUHMO_MB_COUNT };
int suhmo_level_mass_balance(suhmo_level_t *L, double out[SUHMO_MB_COUNT], suhmo_stream_t s);
int suhmo_hier_mass_balance(suhmo_hier_t *H, double *out /* [nlev][SUHMO_MB_COUNT] */, suhmo_stream_t s);
int suhmo_batch_mass_balance(suhmo_batch_t *B, double *out /* [n][SUHMO_MB_COUNT] */, const int *active, suhmo_stream_t s);

/* ---- WATER BUDGET (suhmo_amd/csrc/suhmo_balance.hip, suhmo_run.hip, suhmo_batch.hip; DESIGN.md section 5, "Water budget"; tests/budget_ref.py is
 * the numpy twin): the conservation record the reference prints after every step of a run with AmrHydro.post_proc = true -- check_fluxes with
 * B/Bold (src/AmrHydro.cpp:440-590) and the line "Time(months) VOL_waterTot rechargeTOT ramp" (:4036-4038) -- as TEN doubles per level or member:
 *   0 .. 6        the seven values of "MASS BALANCE": the same rule, the same order, the same bits (mb_fold of suhmo_balance.h is stated once)
 *   VOLUME_OLD    the reference's BtotOld: sum of B dx dy over the cells with mask > 0 of the gap height the last TRACKED step started from.  The
 *                 device updates b in place, so the sum is measured at the entry of the step, before anything writes b (after the regrid, reload
 *                 and forcing of a run's step: the reference copies m_old_gapheight at the top of timeStepFAS).  First stage k_volume (mask and B
 *                 only, 16 B per cell) on the grid, walk and tree of k_balance; the partials stay on the device, nothing is copied or
 *                 synchronised; the final stage of a budget finishes them with the second-stage walk.  So the value is bit for bit the VOLUME of
 *                 the mass-balance call made immediately before that step.  A quiet NaN where no tracked step has run on that level or member:
 *                 option off, no step yet, a member the tracked steps left out from the start, EVERY level of the new handle after a regrid.
 *   RECH_EXT      the two parts of rechargeTOT (:3766-3773), per cell with ice = mask > 0 as d_postproc_columns forms them:
 *   RECH_MELT         src = use_moulin_source ? MSRC * ramp + distributed_input : (ice ? distributed_input : 0.0)
 *                     ice:  ext += src * dy * dx;   melt += (MR / rho_w) * dy * dx
 *                 folded AFTER the volume term of the same cell, each with its own accumulator started at 0.0, reduced in the order of
 *                 suhmo_reduce.h like the other values.  This is NOT the per-column order of the SHMIP table (suhmo_level_postproc_partial sums
 *                 a column's rows first): the two agree to rounding only.  The reference forms the line on level 0; here every level has its own.
 * mp supplies ramp, distributed_input, rho_w and use_moulin_source (an ensemble: each member's own row of mp[n]).
 * OPTION track_old_volume (suhmo_level_set_option, suhmo_hier_set_option, suhmo_batch_set_option; 0 or 1, default 0: every launch sequence and
 * counter of a step is what it was).  With 1, suhmo_level_timestep, suhmo_hier_timestep and suhmo_batch_timestep begin -- after their refusals --
 * with the k_volume first stage into a buffer the handle owns (allocated on first use, freed with it): one launch for a level, one per level of a
 * hierarchy (never one per box), one for the members the step serves; members it does not serve keep what they had.  suhmo_hier_regrid carries
 * the option to the new handle as it carries the others; the kept volume does not carry over.  Refused with rc -5 on rank strips.
 * LAUNCHES AND COPIES of the stand-alone calls, as the mass-balance calls: suhmo_level_water_budget: two launches, one copy of 10 doubles, one
 * synchronisation.  suhmo_hier_water_budget: nlev first stages (k_budget: head, mask, B, BX, BY, MR, MSRC; nine values per workgroup) + ONE final
 * launch (a workgroup per level: the nine sums, VOLUME_OLD from the kept partials, ten doubles), one copy, one synchronisation.
 * suhmo_batch_water_budget: one first stage, one final launch (a workgroup per flagged member), one read-back (batch_launches += 2,
 * batch_readbacks += 1); rows of members without a flag keep the caller's.  Read-only options of a hierarchy: budget_launches (the k_volume
 * launches of tracked steps, the first stages and final launches of budgets), budget_copies, budget_device_bytes (the partial buffers the handle
 * holds); a run carries the first two across its regrids.  An ensemble counts in batch_launches and batch_readbacks.  READ-ONLY calls.
 * REFUSED before anything is launched, out untouched, a step afterwards unaffected: everything the mass-balance calls refuse, with their codes;
 * rc -1: mp is NULL; SUHMO_F_MR is missing (no time step has run); use_moulin_source without SUHMO_F_MSRC (the message names the level and box,
 * or the member).
 * THE SERIES INSIDE THE RUNS.  suhmo_hier_run_bud and suhmo_batch_run_bud with bud = NULL ARE suhmo_hier_run_out and suhmo_batch_run (which
 * are thin wrappers of them).  With bud: a row after step k when (k + 1) % every == 0.  The run sets track_old_volume = 1 for exactly the steps
 * that end in a row (the other steps run with the caller's setting) and puts the caller's setting back on every way out.  After such a step --
 * and after the daily row if both fall together -- the first stages and the final stage, which writes straight into a device series the run
 * owns: no copy and no synchronisation per row; after the last step the series comes back in ONE copy (budget_copies += 1; an ensemble:
 * batch_readbacks += 1).  The series belongs to the run and survives a regrid's change of handle; the partial buffers belong to the handle.
 * Entries of levels the hierarchy does not have at that row, and of members without a flag, keep the caller's values.  A failing step, regrid,
 * reload or output callback ends the run as it does without a budget; the rows finished so far are copied out and n_rows is exact.
 * Refused before the first launch, rc -1: every < 1; rows NULL; nlev NULL for a hierarchy; lev_cap too small; what the stand-alone call refuses of
 * the starting state, except the face coefficients and SUHMO_F_MR, which the first step forms; use_moulin_source with no forcing of the run to
 * write the source and no source on some box (the run's own rule).  rc -5: rank strips, levels dealt to the ranks, shadow = 1.
 * Not built: rank strips; nested patches (suhmo_amr_*); a composite budget with covered cells left out (the reference gives no rule for a face
 * between a covered and an uncovered cell); the band-discharge lines of post_proc_shmip_temporal (:4055-4078; the reference's own dump_PP.py
 * does not read them). */
enum { SUHMO_WB_LO_X = 0, SUHMO_WB_HI_X, SUHMO_WB_LO_Y, SUHMO_WB_HI_Y, SUHMO_WB_DIR_X, SUHMO_WB_DIR_Y, SUHMO_WB_VOLUME,
       SUHMO_WB_VOLUME_OLD, SUHMO_WB_RECH_EXT, SUHMO_WB_RECH_MELT, SUHMO_WB_COUNT };
int suhmo_level_water_budget(suhmo_level_t *L, const suhmo_model_params_t *mp, double out[SUHMO_WB_COUNT], suhmo_stream_t s);
int suhmo_hier_water_budget(suhmo_hier_t *H, const suhmo_model_params_t *mp, double *out /* [nlev][SUHMO_WB_COUNT] */, suhmo_stream_t s);
int suhmo_batch_water_budget(suhmo_batch_t *B, const suhmo_model_params_t *mp, double *out /* [n][SUHMO_WB_COUNT] */, const int *active, suhmo_stream_t s);
typedef struct suhmo_run_budget {
    int every;        /* a row after step k when (k + 1) % every == 0; > 0 */
    int lev_cap;      /* hierarchy: levels a row has room for (>= min(max_level + 1, 8) when the run regrids, >= nlev otherwise); ensemble: ignored */
    double *rows;     /* hierarchy [n_steps / every][lev_cap][SUHMO_WB_COUNT]; ensemble [n_steps / every][n][SUHMO_WB_COUNT] */
    int *nlev;        /* hierarchy [n_steps / every]: levels the hierarchy had at that row; ensemble: may be NULL */
    int n_rows;       /* out */
} suhmo_run_budget_t;
int suhmo_hier_run_bud(suhmo_hier_t **H, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, const suhmo_hier_output_t *out,
                       suhmo_run_budget_t *bud, suhmo_hier_run_result_t *res, suhmo_stream_t s);
int suhmo_batch_run_bud(suhmo_batch_t *B, const suhmo_model_params_t *mp, const suhmo_batch_schedule_t *sch, const int *active,
                        suhmo_run_budget_t *bud, suhmo_batch_run_result_t *res, suhmo_stream_t s);

/* ---- INITIAL CONDITIONS (suhmo_amd/csrc/suhmo_ibc.hip, suhmo_ibc.h; tests/ibc_ref.py is the numpy twin of this text): the
 * reference's four IBC classes, selected by problem_type in exec/<case>/Suhmo.cpp, evaluated on the device -- the first state of a model
 * (initializeData + setup_iceMask, AmrHydro::initData :5100-5147) and what AmrHydro::regrid evaluates anew on every new level
 * (initializeBed, the 10-argument initializePi, setup_iceMask with the ghost fills around them, :4387-4437).
 *   SUHMO_IBC_BASIC   HydroIBC          SUHMO_IBC_SQRT   SqrtIBC (SHMIP A, B, F)
 *   SUHMO_IBC_VALLEY  ValleyIBC (E)     SUHMO_IBC_DINO   MountainIBC (AMR_multiMoulins)
 * suhmo_ibc_t holds the kind, the suhmo_params values the formulas read (slope = m_slope, ice_height = m_H, gap_init = m_gapInit, rho_i, rho_w,
 * gravity, G, L) and ValleyIBC's gamma.  Fact = 1 / (rho_w * gravity) below.
 * CELLS.  Every body runs over the box WITH its ghost ring, i = -1 .. nx, j = -1 .. ny, cell (i, j) of a box whose first cell is (i0, j0) of its
 * level: gi = i0 + i, gj = j0 + j; a (gi, gj) that lies beyond a PERIODIC side of the level's domain is first wrapped into it (so every
 * written field holds the periodic image there, what Chombo's exchange leaves); x = (gi + 0.5) * dx, y = (gj + 0.5) * dy, and y = (gj + 0.5) * dy
 * - 750 for the valley.  Every expression is evaluated left to right as written, one rounding per operation, no contraction; max(a, b) and
 * min(a, b) are std::max / std::min, a < b ? b : a and b < a ? b : a: a NaN in a (sqrt's ghost cells left of x = -ice_height) comes back.
 * CONSTANTS formed once on the host with the C library and passed by value: P = pow(2.0e10, 0.25); H6 = 100 * pow(6200, 0.25) + 6000 / 60 - P + 1;
 * cos and sin of a * 3.14159 / 180 for the dino's angles a = 35, 90, 60, 2.  On the device run only sqrt (correctly rounded), the valley's
 * pow(x + 200, 0.25) and the dino's exp: those two kinds are NOT bit for bit the host's where they enter.
 * INITIAL STATE (initializeData), per kind -- zb = SUHMO_F_ZB, zs = SUHMO_F_ZS (m_iceheight), Pi = SUHMO_F_PI, b = SUHMO_F_B, Pw = SUHMO_F_PW, h = SUHMO_F_PHI:
 *   basic   zb = slope * x; b = gap_init; zs = ice_height; Pi = rho_i * gravity * zs; Pw = Pi * 0.5; h = Pw * Fact + zb.
 *   sqrt    zb = slope * x; zs = max(6 * (sqrt(x + ice_height) - sqrt(ice_height)) + 1, 0); Pi = max(rho_i * gravity * zs, 0);
 *           b = 1e-16 where Pi < 2, else gap_init; Pw = 101325; h = Pw * Fact + zb.
 *   valley  S = 100 * pow(x + 200, 0.25) + x / 60 - P + 1; f(g) = (H6 - 6000 * g) * x * x / (6000 * 6000) + g * x; fx = f(gamma), fb = f(0.05);
 *           gy = 0.5e-6 * |y * y * y|; hx = (-4.5 * x / 6000 + 5) * (S - fx) / (S - fb + 1e-16); zb = fx + gy * hx;
 *           Pi = rho_i * gravity * max(S - zb, 0); b = 1e-16 where Pi < 1e-10, else gap_init; zs = max(S - zb, 0) (the CORRECTED ice height);
 *           Pw = Pi * 0.5; h = Pw * Fact + zb, then 0 where h < 0 (resetCovered).
 *   dino    t = 1.5e-3 * x + -1.5e-3 * y + 100; zs = 2 * (t + 100); finger(a, x0, y0, A, sg, sigma): xb = x - x0, yb = y - y0, xt = xb * cos + yb * sin,
 *           yt = -xb * sin + yb * cos, Ag = A * exp(-0.5 / (sg * sg) * yt * yt), value Ag * exp(-0.5 / (sigma * sigma) * xt * xt); the four fingers
 *           (35, 1e5, 0, 250, 5e4, sigma = 12000 - 3000 * min(1 - (50000 - yt) / 50000, 1)), (90, 85000, 0, 250, 3e4, 1e4), (60, 55000, 0, 100, 2e4, 5000),
 *           (2, 1e5, 2e4, 300, 35000, 6000); zb = max(max(t, 0) + f2 + f3 + f4 + f5, 0) -- WITHOUT the reference's bed noise (an unseeded
 *           std::default_random_engine drawn in box order, :174, :270: not reproducible); Pi = rho_i * gravity * max(zs, 0); b = 1e-16 where
 *           Pi == 0, else gap_init; Pw = Pi * 0.5; h = Pw * Fact + zb, then 0 where h < 0.
 *   all     SUHMO_F_MR = G / L; SUHMO_F_ACOEF = 0; SUHMO_F_MASK = 1 where Pi > 0, else -1 (setup_iceMask).  Re, qw ("dummy stuff -- will be erased
 *           right away"), the sliding speed and the bump fields (scalars of the model here) are not written; the AGU_test_case branches are not built.
 * RELOAD BODY (initializeBed + initializePi), what each class writes there and nothing else:
 *   basic, sqrt   zb = slope * x.        valley   zs = S (UNcorrected), zb, Pi as above.
 *   dino          zs, Pi as above, b = 1e-16 where Pi == 0 (else b stays); its bed is what the transfer brought.
 * MASK BODY (setup_iceMask): SUHMO_F_MASK = 1 where the stored Pi > 0, else -1, ghost ring included.
 * One __global__ template per body over the launch targets (a level, the boxes of a level, the members of an ensemble); 64 x 4 threads over
 * (nx + 2) x (ny + 2); plain vector stores.
 *
 * suhmo_level_ibc_init(L, ibc, s)    the initial state and the mask of one whole level in ONE launch, then CopyGhostCells (ghost = the cell next to it,
 *     side cells only) of SUHMO_F_ZB and SUHMO_F_MASK across the non-periodic domain sides (initData, :5133-5147).  A whole level is one created with
 *     j0 = 0, ny = ny_global and nx_global = 0 (or i0 = 0, nx_global = nx, as a hierarchy's base may be written).  A rank strip, a patch of a
 *     nested hierarchy (suhmo_amr_*) or a box of a hierarchy -- anything else: rc -5.
 * suhmo_hier_ibc_init(H, ibc, s)     the same on every level: one launch for level 0 and one per refined level (read-only option ibc_launches counts
 *     the launches of the bodies), CopyGhostCells of ZB and MASK on every level; then for l = 1, 2, ... in order the MASK of level l:
 *     PiecewiseLinearFillPatch of its coarse-fine ghost cells from level l - 1 (suhmo_hier_pwl_fill), exchange with corners (suhmo_hier_exchange),
 *     CopyGhostCells.  rc -5: rank strips, levels dealt to the ranks, shadow = 1.
 * suhmo_batch_ibc_init(B, ibcs, active, s)   suhmo_level_ibc_init on every member whose flag in active[n] is not 0 (NULL: all) in ONE launch + the two
 *     ghost launches; ibcs[n_members], a device row per member: the kinds of the active members must be equal (rc -1), every other value is the member's.
 *     The rows are uploaded for the call and freed at its end: the call SYNCHRONISES the stream (an initialisation call; batch_launches grows by the
 *     launches made, 3).
 * suhmo_hier_set_ibc(H, ibc)         keeps *ibc on the handle (NULL: none); suhmo_hier_regrid hands it to the new handle with the options.
 * suhmo_hier_ibc_reload(H, level, s) level >= 1, :4387-4437: (1) the reload body on every box of the level, one launch; (2) for each field it wrote among
 *     ZB, PI, ZS, in this order: suhmo_hier_pwl_fill from level - 1, suhmo_hier_exchange with corners, then CopyGhostCells (ZB) or
 *     ExtrapGhostCells (PI, ZS; ghost = 2 x the cell next to it - the one behind); (3) the mask body, one launch; (4) pwl fill, exchange,
 *     CopyGhostCells of MASK.  A field the body did not write keeps what the transfer left (the dino's b is written inside valid and ghost cells
 *     alike and gets no fill).  Needs suhmo_hier_set_ibc; ibc_launches grows by 2.
 * suhmo_hier_regrid with an IBC on H: after steps a - e of the new level l, suhmo_hier_ibc_reload(new handle, l) -- INSIDE the ascending loop, so that
 *     level l + 1 interpolates from the reloaded level l, as the reference's loop does.  Without an IBC nothing changes.
 * suhmo_hier_run with an IBC on *H: `reload` may be NULL; one that is given still runs, after the device reload.  For THE SURFACE HEIGHT ACROSS A
 *     REGRID valley and dino bring SUHMO_F_ZS to every new box, basic and sqrt do not.
 * Every call counts as a write of the fields it touches, as suhmo_level_set_field does: what the level knows about its ice mask and bed, the halo
 * state of its head, and the hierarchy's ghost / residual bookkeeping start over.
 * Checked before anything is launched, rc -1 and a message: a NULL handle or struct, an unknown kind, gap_init <= 0, a level outside
 * 1 .. nlev - 1 for the reload, a reload without an IBC on the handle.
 * Not built: the bed noise, AGU_test_case, an IBC that reads files, bump fields as arrays, rank strips. */
enum { SUHMO_IBC_BASIC = 0, SUHMO_IBC_SQRT = 1, SUHMO_IBC_VALLEY = 2, SUHMO_IBC_DINO = 3 };
typedef struct suhmo_ibc {
    int kind;
    double slope, ice_height, gap_init, rho_i, rho_w, gravity, G, L;
    double gamma;      /* valley */
} suhmo_ibc_t;
int suhmo_level_ibc_init(suhmo_level_t *L, const suhmo_ibc_t *ibc, suhmo_stream_t s);
int suhmo_hier_ibc_init(suhmo_hier_t *H, const suhmo_ibc_t *ibc, suhmo_stream_t s);
int suhmo_batch_ibc_init(suhmo_batch_t *B, const suhmo_ibc_t *ibcs, const int *active, suhmo_stream_t s);
int suhmo_hier_set_ibc(suhmo_hier_t *H, const suhmo_ibc_t *ibc);
int suhmo_hier_ibc_reload(suhmo_hier_t *H, int level, suhmo_stream_t s);

/* Named timers with the reference's CH_TIME labels (src/VCAMRNonLinearPoissonOp.cpp:40,69,103,277,390,660; CH_TIMER_REPORT at
 * exec/A_SHMIP/Suhmo.cpp:136).  mode 0 off (default; env SUHMO_TIMERS), 1 host wall time per scope, 2 with the device synchronised at
 * both ends of a scope (the time of the kernels it launched; serialises, for profiling only).  suhmo_timers_report writes
 * "label calls total[s] mean[us]" lines, most expensive first, and returns the bytes the full report needs. */
int suhmo_timers_enable(int mode);
int suhmo_timers_reset(void);
long suhmo_timers_report(char *buf, long size);

/* timing helper: average device time (ms) of the depth-0 GSRB sweep kernel launches since the last reset, measured with
 * HIP events on the launch stream.  suhmo_level_profile_read: the plain K-sweep launches (k_gsrb_fused<K, ., ., false>);
 * suhmo_level_profile_read_restricting: the launches that end a pre-smoothing and also restrict (k_gsrb_fused<K, ., ., true>:
 * K sweeps + RESTRICTRESVCNL2D + RESTRICTVCNL in one pass) */
int suhmo_level_profile_reset(suhmo_level_t *L);
int suhmo_level_profile_enable(suhmo_level_t *L, int on);
int suhmo_level_profile_read(suhmo_level_t *L, suhmo_stream_t s, double *gsrb_ms_total,
                             long *gsrb_launches, long *gsrb_cells);
int suhmo_level_profile_read_restricting(suhmo_level_t *L, suhmo_stream_t s, double *ms_total, long *launches, long *cells);

#ifdef __cplusplus
}
#endif
#endif
