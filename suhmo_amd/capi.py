"""ctypes binding of libsuhmo_hip.so (the C-ABI declared in include/suhmo_hip.h).

There is NO fallback: if the HIP library is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("SUHMO_LIB") or os.path.join(CSRC, "libsuhmo_hip.so")     # SUHMO_LIB: another build of the same library (A/B runs)
_LIB = None


class SuhmoError(RuntimeError):
    pass


class Phys(C.Structure):
    _fields_ = [("A", C.c_double), ("omega", C.c_double), ("nu", C.c_double),
                ("cutOffbr", C.c_double), ("maxOffbr", C.c_double),
                ("rho_w_g", C.c_double), ("grav", C.c_double),
                ("cutOffB", C.c_int), ("use_NL", C.c_int), ("use_mask_gradients", C.c_int)]


class BC(C.Structure):
    _fields_ = [("type", (C.c_int * 2) * 2), ("value", (C.c_double * 2) * 2), ("periodic", C.c_int * 2)]


class SolverParams(C.Structure):
    _fields_ = [("num_smooth", C.c_int), ("num_bottom", C.c_int), ("max_iter", C.c_int),
                ("iter_min", C.c_int), ("imin", C.c_int), ("eps", C.c_double), ("hang", C.c_double),
                ("norm_thresh", C.c_double), ("bcoeff_otf", C.c_int), ("max_depth", C.c_int)]


class ModelParams(C.Structure):
    _fields_ = [("rho_i", C.c_double), ("rho_w", C.c_double), ("gravity", C.c_double), ("G", C.c_double),
                ("L", C.c_double), ("ct", C.c_double), ("cw", C.c_double), ("ub0", C.c_double), ("ub1", C.c_double),
                ("br", C.c_double), ("lr", C.c_double), ("diffFactor", C.c_double),
                ("distributed_input", C.c_double), ("eps_picard", C.c_double),
                ("basal_friction", C.c_int), ("use_mask_rhs_b", C.c_int), ("use_moulin_source", C.c_int),
                ("ramp", C.c_double), ("use_impl_diff", C.c_int),
                ("head_melt_off", C.c_int), ("freeze_icefree_gap", C.c_int)]


class LevelDesc(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("j0", C.c_int), ("ny_global", C.c_int),
                ("dx", C.c_double), ("dy", C.c_double), ("nbox", C.c_int), ("boxes", C.POINTER(C.c_int)),
                ("max_box", C.c_int), ("alpha", C.c_double), ("beta", C.c_double),
                ("bc", BC), ("phys", Phys), ("device", C.c_int), ("halo_rows", C.c_int),
                ("i0", C.c_int), ("nx_global", C.c_int), ("patch_j0", C.c_int), ("patch_ny", C.c_int)]


class BatchSchedule(C.Structure):
    """suhmo_batch_schedule_t: the values a run of an ensemble is driven by (suhmo_batch_run), all host arrays"""
    _fields_ = [("n_steps", C.c_int), ("dt", C.c_double), ("first_cur_step", C.c_int), ("n_members", C.c_int),
                ("T_K", C.POINTER(C.c_double)), ("background", C.POINTER(C.c_double)),
                ("n_moulins", C.POINTER(C.c_int)), ("positions", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double)),
                ("flux", C.POINTER(C.c_double)), ("moulin_factor", C.POINTER(C.c_double)), ("ramp", C.POINTER(C.c_double)),
                ("diag_every", C.c_int)]


class BatchRunResult(C.Structure):
    _fields_ = [("steps_done", C.c_int), ("n_rows", C.c_int), ("picard_iters", C.POINTER(C.c_int)), ("vcycles", C.POINTER(C.c_int)),
                ("rows", C.POINTER(C.c_double))]


class RunBudget(C.Structure):
    """suhmo_run_budget_t: the water budget series of suhmo_hier_run_bud / suhmo_batch_run_bud (include/suhmo_hip.h, "WATER BUDGET")"""
    _fields_ = [("every", C.c_int), ("lev_cap", C.c_int), ("rows", C.POINTER(C.c_double)), ("nlev", C.POINTER(C.c_int)), ("n_rows", C.c_int)]


class GridParams(C.Structure):
    """suhmo_grid_params_t: what the reference hands to BRMeshRefine"""
    _fields_ = [("fill_ratio", C.c_double), ("block_factor", C.c_int), ("max_box_size", C.c_int), ("nesting_radius", C.c_int)]


class TagSpec(C.Structure):
    """suhmo_tag_spec_t: a tag variable of a run's regrids, with the levels it tags"""
    _fields_ = [("field", C.c_int), ("vmin", C.c_double), ("vmax", C.c_double), ("grow", C.c_int), ("grow_x", C.c_int), ("grow_y", C.c_int),
                ("min_level", C.c_int), ("cap_level", C.c_int)]


IBC_BASIC, IBC_SQRT, IBC_VALLEY, IBC_DINO = 0, 1, 2, 3          # SUHMO_IBC_*: the reference's problem_type basic / sqrt / valley / dino
IBC_KINDS = dict(basic=IBC_BASIC, sqrt=IBC_SQRT, valley=IBC_VALLEY, dino=IBC_DINO)


class Ibc(C.Structure):
    """suhmo_ibc_t: an IBC class of the reference and the values its formulas read (include/suhmo_hip.h, "INITIAL CONDITIONS")"""
    _fields_ = [("kind", C.c_int), ("slope", C.c_double), ("ice_height", C.c_double), ("gap_init", C.c_double), ("rho_i", C.c_double),
                ("rho_w", C.c_double), ("gravity", C.c_double), ("G", C.c_double), ("L", C.c_double), ("gamma", C.c_double)]


RELOAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int)      # user, the new hierarchy, index of the regrid, cur_step


class HierSchedule(C.Structure):
    """suhmo_hier_schedule_t: the values a run of a hierarchy is driven by (suhmo_hier_run), all host arrays"""
    _fields_ = [("n_steps", C.c_int), ("dt", C.c_double), ("first_cur_step", C.c_int),
                ("T_K", C.POINTER(C.c_double)), ("background", C.POINTER(C.c_double)),
                ("n_moulins", C.c_int), ("positions", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double)), ("flux", C.POINTER(C.c_double)),
                ("moulin_factor", C.POINTER(C.c_double)), ("ramp", C.POINTER(C.c_double)), ("diag_every", C.c_int),
                ("regrid_interval", C.c_int), ("skip_first_regrid", C.c_int), ("max_level", C.c_int),
                ("n_tags", C.c_int), ("tags", C.POINTER(TagSpec)), ("grid", GridParams),
                ("subset_nbox", C.POINTER(C.c_int)), ("subset_boxes", C.POINTER(C.c_int)),
                ("n_fields", C.c_int), ("fields", C.POINTER(C.c_int)), ("reload", RELOAD_FN), ("user", C.c_void_p)]


class HierRegridLog(C.Structure):
    _fields_ = [("cur_step", C.c_int), ("same", C.c_int), ("nlev", C.c_int), ("nbox", C.c_int * 8)]


class HierRunResult(C.Structure):
    _fields_ = [("steps_done", C.c_int), ("n_rows", C.c_int), ("picard_iters", C.POINTER(C.c_int)), ("vcycles", C.POINTER(C.c_int)),
                ("rows", C.POINTER(C.c_double)), ("moulin_steps", C.POINTER(C.c_int)), ("n_regrids", C.c_int), ("regrids_cap", C.c_int),
                ("regrids", C.POINTER(HierRegridLog)), ("n_moved", C.c_int)]


class SnapComp(C.Structure):
    """suhmo_snap_comp_t: one component of a snapshot"""
    _fields_ = [("kind", C.c_int), ("field", C.c_int), ("value", C.c_double)]


SNAP_FIELD, SNAP_FACE_TO_CELL, SNAP_CONST = 0, 1, 2
SNAP_MAX_COMPS = 16
# user, the hierarchy, kind (0 plot, 1 checkpoint), cur_step, ncomp, level_offset, box_offset, data
OUTPUT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_double))


class HierOutput(C.Structure):
    """suhmo_hier_output_t: the plot files and checkpoints of a run (suhmo_hier_run_out)"""
    _fields_ = [("plot_interval", C.c_int), ("check_interval", C.c_int), ("restart_step", C.c_int), ("no_final", C.c_int),
                ("n_plot", C.c_int), ("plot", C.POINTER(SnapComp)), ("n_check", C.c_int), ("check", C.POINTER(SnapComp)),
                ("write", OUTPUT_FN), ("user", C.c_void_p)]


def snap_comps(comps):
    """[(kind, field, value) or (kind, field) or SnapComp] -> a C array of suhmo_snap_comp_t"""
    arr = (SnapComp * max(len(comps), 1))()
    for q, c in enumerate(comps):
        arr[q] = c if isinstance(c, SnapComp) else SnapComp(int(c[0]), int(c[1]), float(c[2]) if len(c) > 2 else 0.0)
    return arr


class FlatComp(C.Structure):
    """suhmo_flat_comp_t: one component of a flatten (FLAT_FIELD: field; FLAT_DIFF: field - field2, formed before the interpolation)"""
    _fields_ = [("kind", C.c_int), ("field", C.c_int), ("field2", C.c_int)]


FLAT_FIELD, FLAT_DIFF = 0, 1
FLAT_MAX_COMPS = 16
CMP_COMPOSITE, CMP_FINEST = 0, 1             # the modes of suhmo_hier_compare


def flat_comps(comps):
    """[(kind, field) or (kind, field, field2) or FlatComp] -> a C array of suhmo_flat_comp_t"""
    arr = (FlatComp * max(len(comps), 1))()
    for q, c in enumerate(comps):
        arr[q] = c if isinstance(c, FlatComp) else FlatComp(int(c[0]), int(c[1]), int(c[2]) if len(c) > 2 else 0)
    return arr


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int)      # values, n, op (0 MAX, 1 SUM)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p)

# every symbol include/suhmo_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "suhmo_last_error", "suhmo_device_count", "suhmo_level_create", "suhmo_level_destroy",
    "suhmo_level_num_depths", "suhmo_level_synchronize", "suhmo_level_put_box", "suhmo_level_get_box",
    "suhmo_level_set_field", "suhmo_level_get_field", "suhmo_level_field_view", "suhmo_level_gsrb",
    "suhmo_level_apply_op", "suhmo_level_residual", "suhmo_level_restrict_residual",
    "suhmo_level_restrict_r", "suhmo_level_prolong_increment", "suhmo_level_prolong_bilinear",
    "suhmo_level_update_operator", "suhmo_level_average_operator", "suhmo_level_build_mg_coefficients",
    "suhmo_level_nonlinear", "suhmo_level_compute_lambda", "suhmo_level_fill_ghosts",
    "suhmo_level_divergence", "suhmo_level_get_flux", "suhmo_level_norm", "suhmo_level_axby",
    "suhmo_level_set_value", "suhmo_level_vcycle", "suhmo_level_solve", "suhmo_level_pack_rows",
    "suhmo_level_unpack_rows", "suhmo_level_set_hooks", "suhmo_level_exchange", "suhmo_level_halo_info", "suhmo_level_phi_halo_fresh", "suhmo_level_profile_reset",
    "suhmo_level_profile_enable", "suhmo_level_profile_read", "suhmo_level_profile_read_restricting", "suhmo_level_timestep",
    "suhmo_rccl_load", "suhmo_rccl_unique_id", "suhmo_level_attach_rccl", "suhmo_level_detach_rccl",
    "suhmo_level_rccl_exchanges", "suhmo_level_rccl_comm_count", "suhmo_level_ipc_export", "suhmo_level_attach_ipc", "suhmo_level_ipc_exchanges", "suhmo_level_detach_ipc",
    "suhmo_amr2_cf_interp", "suhmo_amr2_average", "suhmo_amr2_fine_update_operator", "suhmo_amr2_residual",
    "suhmo_amr2_vcycle", "suhmo_amr2_solve", "suhmo_level_moulin_source", "suhmo_amr2_prolong2", "suhmo_amr2_set_covered",
    "suhmo_amr_residual", "suhmo_amr_vcycle", "suhmo_amr_solve", "suhmo_level_postproc_table", "suhmo_level_postproc_partial", "suhmo_postproc_finish", "suhmo_postproc_temporal", "suhmo_level_postproc_temporal",
    "suhmo_level_set_alpha_beta", "suhmo_level_set_bc", "suhmo_amr2_reflux", "suhmo_amr2_pwl_fill", "suhmo_amr_timestep", "suhmo_level_time_varying_recharge", "suhmo_amr_moulin_source", "suhmo_amr2_prolong_pc", "suhmo_amr2_finer_operator_changed",
    "suhmo_hier_create", "suhmo_hier_destroy", "suhmo_hier_num_levels", "suhmo_hier_num_boxes", "suhmo_hier_box", "suhmo_hier_box_owner", "suhmo_hier_exchange",
    "suhmo_hier_cf_interp", "suhmo_hier_pwl_fill", "suhmo_hier_average", "suhmo_hier_gsrb", "suhmo_hier_update_operator",
    "suhmo_hier_residual", "suhmo_hier_vcycle", "suhmo_hier_solve", "suhmo_hier_timestep", "suhmo_hier_moulin_source",
    "suhmo_hier_set_allgather", "suhmo_hier_attach_rccl", "suhmo_hier_gathers", "suhmo_level_set_option", "suhmo_level_get_option", "suhmo_timers_enable", "suhmo_timers_reset", "suhmo_timers_report",
    "suhmo_level_set_reduce_hook", "suhmo_level_dot", "suhmo_level_set_allgather", "suhmo_level_agglomerated_depth",
    "suhmo_hier_create_opts", "suhmo_hier_set_option", "suhmo_hier_get_option",
    "suhmo_batch_create", "suhmo_batch_destroy", "suhmo_batch_size", "suhmo_batch_member", "suhmo_batch_set_phys", "suhmo_batch_vcycle", "suhmo_batch_solve", "suhmo_batch_timestep",
    "suhmo_batch_set_option", "suhmo_batch_get_option", "suhmo_batch_create_opts",
    "suhmo_batch_time_varying_recharge", "suhmo_batch_moulin_source", "suhmo_batch_postproc_partial", "suhmo_batch_postproc_temporal", "suhmo_batch_postproc_table",
    "suhmo_batch_run", "suhmo_level_postproc_temporal_device",
    "suhmo_hier_tag_cells", "suhmo_hier_clear_tags", "suhmo_hier_get_tags", "suhmo_level_tag_cells", "suhmo_level_clear_tags", "suhmo_level_get_tags",
    "suhmo_grids_generate", "suhmo_hier_generate_grids", "suhmo_hier_regrid",
    "suhmo_hier_restrict_tags", "suhmo_tag_subsets_nest", "suhmo_hier_get_boxes",
    "suhmo_hier_time_varying_recharge", "suhmo_hier_postproc_temporal", "suhmo_hier_run",
    "suhmo_hier_snapshot", "suhmo_level_snapshot", "suhmo_hier_run_out", "suhmo_hier_flatten",
    "suhmo_hier_compare",
    "suhmo_level_mass_balance", "suhmo_hier_mass_balance", "suhmo_batch_mass_balance",
    "suhmo_level_water_budget", "suhmo_hier_water_budget", "suhmo_batch_water_budget", "suhmo_hier_run_bud", "suhmo_batch_run_bud",
    "suhmo_level_ibc_init", "suhmo_hier_ibc_init", "suhmo_batch_ibc_init", "suhmo_hier_set_ibc", "suhmo_hier_ibc_reload",
]
# the seven values of a mass balance in the order of the enum SUHMO_MB_* (include/suhmo_hip.h, "MASS BALANCE")
MB_NAMES = ("lo_x", "hi_x", "lo_y", "hi_y", "dir_x", "dir_y", "volume")
# the ten values of a water budget in the order of the enum SUHMO_WB_* ("WATER BUDGET"): those seven, the volume the last tracked step started
# from (NaN: none), the two parts of rechargeTOT
WB_NAMES = MB_NAMES + ("volume_old", "recharge_ext", "recharge_melt")


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU).  With SUHMO_LIB set the library in use is
    somebody else's build: nothing is compiled (the in-tree file would not be the one lib() loads)."""
    if os.environ.get("SUHMO_LIB"):
        if not os.path.exists(LIB_PATH):
            raise SuhmoError("SUHMO_LIB = %s does not exist" % LIB_PATH)
        return LIB_PATH
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "suhmo_hip.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", CSRC, "-B", "libsuhmo_hip.so"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SuhmoError("libsuhmo_hip.so not built (%s); run __graft_entry__.build(). "
                         "There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    dp, vp, ci = C.POINTER(C.c_double), C.c_void_p, C.c_int
    L.suhmo_last_error.restype = C.c_char_p
    L.suhmo_level_create.argtypes = [C.POINTER(vp), C.POINTER(LevelDesc)]
    L.suhmo_level_destroy.argtypes = [vp]
    L.suhmo_level_num_depths.argtypes = [vp]
    L.suhmo_level_synchronize.argtypes = [vp, vp]
    L.suhmo_level_put_box.argtypes = [vp, ci, ci, ci, dp, ci, ci, ci, ci, ci, vp]
    L.suhmo_level_get_box.argtypes = [vp, ci, ci, ci, dp, ci, ci, ci, ci, vp]
    L.suhmo_level_set_field.argtypes = [vp, ci, ci, vp, ci, ci, vp]
    L.suhmo_level_get_field.argtypes = [vp, ci, ci, vp, ci, ci, vp]
    L.suhmo_level_field_view.argtypes = [vp, ci, ci, C.POINTER(vp), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.suhmo_level_gsrb.argtypes = [vp, ci, ci, vp]
    L.suhmo_level_apply_op.argtypes = [vp, ci, ci, vp]
    for n in ("residual", "restrict_residual", "restrict_r", "prolong_increment", "prolong_bilinear",
              "update_operator", "average_operator", "nonlinear", "compute_lambda"):
        getattr(L, "suhmo_level_" + n).argtypes = [vp, ci, vp]
    L.suhmo_level_build_mg_coefficients.argtypes = [vp, vp]
    L.suhmo_level_fill_ghosts.argtypes = [vp, ci, ci, ci, vp]
    L.suhmo_level_divergence.argtypes = [vp, ci, ci, vp]
    L.suhmo_level_get_flux.argtypes = [vp, ci, ci, ci, dp, vp]
    L.suhmo_level_norm.argtypes = [vp, ci, ci, ci, dp, vp]
    L.suhmo_level_axby.argtypes = [vp, ci, ci, ci, ci, C.c_double, C.c_double, vp]
    L.suhmo_level_set_value.argtypes = [vp, ci, ci, C.c_double, vp]
    L.suhmo_level_vcycle.argtypes = [vp, C.POINTER(SolverParams), vp]
    L.suhmo_level_solve.argtypes = [vp, C.POINTER(SolverParams), C.POINTER(ci), dp, vp]
    L.suhmo_level_pack_rows.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    L.suhmo_level_unpack_rows.argtypes = [vp, ci, ci, ci, ci, vp, vp]
    L.suhmo_level_set_hooks.argtypes = [vp, EXCHANGE_FN, ALLREDUCE_FN, vp]
    L.suhmo_level_set_reduce_hook.argtypes = [vp, REDUCE_FN]
    L.suhmo_level_set_allgather.argtypes = [vp, ALLGATHER_FN, vp]
    L.suhmo_level_agglomerated_depth.argtypes = [vp]
    L.suhmo_level_dot.argtypes = [vp, ci, ci, ci, dp, vp]
    L.suhmo_level_exchange.argtypes = [vp, ci, ci, vp]
    L.suhmo_level_halo_info.argtypes = [vp, ci] + [C.POINTER(ci)] * 5
    L.suhmo_level_phi_halo_fresh.argtypes = [vp, ci]
    L.suhmo_level_timestep.argtypes = [vp, C.POINTER(ModelParams), C.c_double, ci, C.POINTER(ci), C.POINTER(ci), vp]
    L.suhmo_rccl_load.argtypes = [C.c_char_p]
    L.suhmo_rccl_unique_id.argtypes = [vp]
    L.suhmo_level_attach_rccl.argtypes = [vp, vp, ci, ci, ci, vp]
    L.suhmo_level_detach_rccl.argtypes = [vp]
    L.suhmo_level_rccl_exchanges.argtypes = [vp]
    L.suhmo_level_rccl_exchanges.restype = C.c_long
    L.suhmo_level_ipc_export.argtypes = [vp, vp]
    L.suhmo_level_attach_ipc.argtypes = [vp, ci, ci, ci, vp, vp]
    L.suhmo_level_ipc_exchanges.argtypes = [vp]
    L.suhmo_level_detach_ipc.argtypes = [vp]
    L.suhmo_level_ipc_exchanges.restype = C.c_long
    L.suhmo_level_moulin_source.argtypes = [vp, ci, dp, dp, dp, C.c_double, dp, vp]
    L.suhmo_level_postproc_table.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_level_postproc_partial.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_postproc_finish.argtypes = [dp, C.c_int, C.c_double, dp]
    L.suhmo_postproc_temporal.argtypes = [dp, C.c_int, C.c_double, dp]
    L.suhmo_level_postproc_temporal.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_level_set_alpha_beta.argtypes = [vp, C.c_double, C.c_double]
    L.suhmo_level_set_bc.argtypes = [vp, C.POINTER(BC)]
    L.suhmo_amr2_reflux.argtypes = [vp, vp, C.c_int, vp]
    L.suhmo_amr2_pwl_fill.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.suhmo_level_time_varying_recharge.argtypes = [vp, C.c_double, C.c_double, vp]
    L.suhmo_amr_moulin_source.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int), C.c_int, dp, dp, dp, C.c_double, dp, vp]
    L.suhmo_amr_timestep.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(ModelParams), C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    L.suhmo_amr2_prolong_pc.argtypes = [vp, vp, C.c_int, vp]
    L.suhmo_amr2_finer_operator_changed.argtypes = [vp, vp, vp]
    L.suhmo_amr_residual.argtypes = [C.POINTER(vp), ci, dp, vp]
    L.suhmo_amr_vcycle.argtypes = [C.POINTER(vp), ci, C.POINTER(SolverParams), vp]
    L.suhmo_amr_solve.argtypes = [C.POINTER(vp), ci, C.POINTER(SolverParams), C.POINTER(ci), dp, vp]
    L.suhmo_amr2_prolong2.argtypes = [vp, vp, ci, vp]
    L.suhmo_amr2_set_covered.argtypes = [vp, vp, ci, C.c_double, vp]
    L.suhmo_amr2_cf_interp.argtypes = [vp, vp, ci, ci, vp]
    L.suhmo_amr2_average.argtypes = [vp, vp, ci, ci, vp]
    L.suhmo_amr2_fine_update_operator.argtypes = [vp, vp, vp]
    L.suhmo_amr2_residual.argtypes = [vp, vp, dp, vp]
    L.suhmo_amr2_vcycle.argtypes = [vp, vp, C.POINTER(SolverParams), vp]
    L.suhmo_amr2_solve.argtypes = [vp, vp, C.POINTER(SolverParams), C.POINTER(ci), dp, vp]
    ip = C.POINTER(ci)
    L.suhmo_hier_create.argtypes = [C.POINTER(vp), C.POINTER(LevelDesc), ci, ip, ip]
    L.suhmo_hier_create_opts.argtypes = [C.POINTER(vp), C.POINTER(LevelDesc), ci, ip, ip, C.c_char_p]
    L.suhmo_hier_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.suhmo_hier_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_long)]
    L.suhmo_hier_destroy.argtypes = [vp]
    L.suhmo_hier_num_levels.argtypes = [vp]
    L.suhmo_hier_num_boxes.argtypes = [vp, ci]
    L.suhmo_hier_box.argtypes = [vp, ci, ci]
    L.suhmo_hier_box.restype = vp
    L.suhmo_hier_box_owner.argtypes = [vp, ci, ci, ip]
    L.suhmo_hier_exchange.argtypes = [vp, ci, ci, ci, vp]
    L.suhmo_hier_cf_interp.argtypes = [vp, ci, ci, ci, vp]
    L.suhmo_hier_pwl_fill.argtypes = [vp, ci, ci, ci, vp]
    L.suhmo_hier_average.argtypes = [vp, ci, ci, ci, vp]
    L.suhmo_hier_gsrb.argtypes = [vp, ci, ci, vp]
    L.suhmo_hier_update_operator.argtypes = [vp, ci, vp]
    L.suhmo_hier_residual.argtypes = [vp, dp, vp]
    L.suhmo_hier_vcycle.argtypes = [vp, C.POINTER(SolverParams), vp]
    L.suhmo_hier_solve.argtypes = [vp, C.POINTER(SolverParams), ip, dp, vp]
    L.suhmo_hier_timestep.argtypes = [vp, C.POINTER(ModelParams), C.c_double, ci, ip, ip, vp]
    L.suhmo_hier_moulin_source.argtypes = [vp, ci, dp, dp, dp, C.c_double, dp, vp]
    L.suhmo_hier_set_allgather.argtypes = [vp, ALLGATHER_FN, vp]
    L.suhmo_hier_attach_rccl.argtypes = [vp]
    L.suhmo_hier_gathers.argtypes = [vp]
    L.suhmo_hier_gathers.restype = C.c_long
    L.suhmo_timers_enable.argtypes = [ci]
    L.suhmo_timers_report.argtypes = [C.c_char_p, C.c_long]
    L.suhmo_timers_report.restype = C.c_long
    L.suhmo_level_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.suhmo_level_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_long)]
    L.suhmo_batch_create.argtypes = [C.POINTER(vp), C.POINTER(LevelDesc), ci]
    L.suhmo_batch_create_opts.argtypes = [C.POINTER(vp), C.POINTER(LevelDesc), ci, C.c_char_p]
    L.suhmo_batch_destroy.argtypes = [vp]
    L.suhmo_batch_size.argtypes = [vp]
    L.suhmo_batch_member.argtypes = [vp, ci]
    L.suhmo_batch_member.restype = vp
    L.suhmo_batch_set_phys.argtypes = [vp, ci, C.POINTER(Phys)]
    L.suhmo_batch_vcycle.argtypes = [vp, C.POINTER(SolverParams), ip, vp]
    L.suhmo_batch_solve.argtypes = [vp, C.POINTER(SolverParams), ip, dp, vp]
    L.suhmo_batch_timestep.argtypes = [vp, C.POINTER(ModelParams), C.c_double, ci, ip, ip, vp]
    L.suhmo_batch_time_varying_recharge.argtypes = [vp, dp, dp, ip, vp]
    L.suhmo_batch_moulin_source.argtypes = [vp, ip, dp, dp, dp, dp, dp, ip, vp]
    for fn in (L.suhmo_batch_postproc_partial, L.suhmo_batch_postproc_temporal, L.suhmo_batch_postproc_table):
        fn.argtypes = [vp, C.POINTER(ModelParams), dp, ip, vp]
    L.suhmo_batch_run.argtypes = [vp, C.POINTER(ModelParams), C.POINTER(BatchSchedule), ip, C.POINTER(BatchRunResult), vp]
    L.suhmo_level_postproc_temporal_device.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_batch_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.suhmo_batch_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_long)]
    L.suhmo_level_profile_reset.argtypes = [vp]
    L.suhmo_level_profile_enable.argtypes = [vp, ci]
    L.suhmo_level_profile_read.argtypes = [vp, vp, dp, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.suhmo_level_profile_read_restricting.argtypes = [vp, vp, dp, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    ucp = C.POINTER(C.c_ubyte)
    L.suhmo_hier_tag_cells.argtypes = [vp, ci, ci, C.c_double, C.c_double, ci, ci, ci, ci, vp]
    L.suhmo_hier_clear_tags.argtypes = [vp, ci]
    L.suhmo_hier_get_tags.argtypes = [vp, ci, ucp, ip, ip]
    L.suhmo_level_tag_cells.argtypes = [vp, ci, C.c_double, C.c_double, ci, ci, ci, ci, vp]
    L.suhmo_level_clear_tags.argtypes = [vp]
    L.suhmo_level_get_tags.argtypes = [vp, ucp, ip, ip]
    L.suhmo_grids_generate.argtypes = [ci, ci, ip, C.POINTER(GridParams), ci, C.POINTER(ucp), ip, ip, ip, ci]
    L.suhmo_hier_generate_grids.argtypes = [vp, C.POINTER(GridParams), ip, ip, ip, ci, ip]
    L.suhmo_hier_regrid.argtypes = [vp, ci, ip, ip, ci, ip, C.POINTER(vp), vp]
    L.suhmo_hier_restrict_tags.argtypes = [vp, ci, ci, ip, vp]
    L.suhmo_tag_subsets_nest.argtypes = [ci, ip, ip, ip, ip, ci]
    L.suhmo_hier_get_boxes.argtypes = [vp, ci, ip]
    L.suhmo_hier_time_varying_recharge.argtypes = [vp, C.c_double, C.c_double, vp]
    L.suhmo_hier_postproc_temporal.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_hier_run.argtypes = [C.POINTER(vp), C.POINTER(ModelParams), C.POINTER(HierSchedule), C.POINTER(HierRunResult), vp]
    lp = C.POINTER(C.c_long)
    L.suhmo_hier_snapshot.argtypes = [vp, ci, C.POINTER(SnapComp), ci, lp, lp, dp, vp]
    L.suhmo_level_snapshot.argtypes = [vp, ci, C.POINTER(SnapComp), ci, lp, dp, vp]
    L.suhmo_hier_run_out.argtypes = [C.POINTER(vp), C.POINTER(ModelParams), C.POINTER(HierSchedule), C.POINTER(HierOutput), C.POINTER(HierRunResult), vp]
    L.suhmo_hier_flatten.argtypes = [vp, ci, ci, C.POINTER(FlatComp), lp, dp, vp]
    L.suhmo_hier_compare.argtypes = [vp, vp, ci, ci, ci, C.POINTER(FlatComp), dp, dp, vp]
    L.suhmo_level_mass_balance.argtypes = [vp, dp, vp]
    L.suhmo_hier_mass_balance.argtypes = [vp, dp, vp]
    L.suhmo_batch_mass_balance.argtypes = [vp, dp, ip, vp]
    L.suhmo_level_water_budget.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_hier_water_budget.argtypes = [vp, C.POINTER(ModelParams), dp, vp]
    L.suhmo_batch_water_budget.argtypes = [vp, C.POINTER(ModelParams), dp, ip, vp]
    L.suhmo_hier_run_bud.argtypes = [C.POINTER(vp), C.POINTER(ModelParams), C.POINTER(HierSchedule), C.POINTER(HierOutput), C.POINTER(RunBudget),
                                     C.POINTER(HierRunResult), vp]
    L.suhmo_batch_run_bud.argtypes = [vp, C.POINTER(ModelParams), C.POINTER(BatchSchedule), ip, C.POINTER(RunBudget), C.POINTER(BatchRunResult), vp]
    L.suhmo_level_ibc_init.argtypes = [vp, C.POINTER(Ibc), vp]
    L.suhmo_hier_ibc_init.argtypes = [vp, C.POINTER(Ibc), vp]
    L.suhmo_batch_ibc_init.argtypes = [vp, C.POINTER(Ibc), ip, vp]
    L.suhmo_hier_set_ibc.argtypes = [vp, C.POINTER(Ibc)]
    L.suhmo_hier_ibc_reload.argtypes = [vp, ci, vp]
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        raise SuhmoError("libsuhmo_hip: rc=%d: %s" % (rc, lib().suhmo_last_error().decode()))


def timers_report():
    """CH_TIMER_REPORT: the named timers as text (enable with lib().suhmo_timers_enable(1 | 2) or SUHMO_TIMERS)"""
    n = lib().suhmo_timers_report(None, 0)
    buf = C.create_string_buffer(n)
    lib().suhmo_timers_report(buf, n)
    return buf.value.decode()
