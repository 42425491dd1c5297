// suhmo_run.hip -- AmrHydro::run (src/AmrHydro.cpp:1283-1365) for a hierarchy of box unions in one call: per step the regrid the reference
// does before it (:1317; tagCells :4514-4536, suhmo_hier_generate_grids, suhmo_hier_regrid), the forcing timeStepFAS evaluates first (seasonal
// recharge :2846-2863, or the moulin source when m_regrid asks for it, :2802), suhmo_hier_timestep, and the daily row of level 0 finished on the
// device into a series that comes back in one copy.  The C-ABI and the order: include/suhmo_hip.h, "THE RUN OF A HIERARCHY".  Nothing here
// computes: every step is one of the public calls (or the launches of one), so the results are the per-call loop's bit for bit.  Eager
// launches, no graph capture, as suhmo_batch_run.  suhmo_hier_run_out adds the plot files and checkpoints AmrHydro::run writes (:1311-1336, :1343-1358):
// a snapshot (suhmo_snap.hip) handed to the caller's callback, include/suhmo_hip.h, "OUTPUT INSIDE THE RUN".  suhmo_hier_run_bud adds the water
// budget series ("WATER BUDGET" there): rows of ten doubles per level finished on the device into a series the run owns, one copy at the end.
#include "suhmo_hier_int.h"
#include <cstring>
#include <vector>

using namespace hier;

namespace {
bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }
// (c - 1) is the reference's m_cur_step before its increment
bool regrid_due(const suhmo_hier_schedule_t *sch, int k)
{
    const int before = sch->first_cur_step + k - 1;
    if (sch->regrid_interval <= 0 || before == 0 || before % sch->regrid_interval) return false;
    return !(k == 0 && sch->skip_first_regrid);
}
// the subset of level l: its boxes follow those of the levels below in subset_boxes
const int *subset_of(const suhmo_hier_schedule_t *sch, int l)
{
    const int *q = sch->subset_boxes;
    for (int m = 0; m < l; m++) q += 4 * (size_t)sch->subset_nbox[m];
    return q;
}
// the body of AmrHydro::regrid on *Hp before the step with cur_step c.  *changed: the hierarchy moved onto other boxes (*Hp is the new handle)
int run_regrid(suhmo_hier **Hp, const suhmo_hier_schedule_t *sch, int c, suhmo_hier_run_result_t *res, bool *changed, suhmo_stream_t s)
{
    suhmo_hier *H = *Hp;
    const int g = sch->grid.block_factor / 2;
    int rc;
    *changed = false;
    if ((rc = suhmo_hier_clear_tags(H, -1))) return rc;
    for (int m = 0; m < sch->n_tags; m++) {
        const suhmo_tag_spec_t &t = sch->tags[m];
        const int top = std::min(t.cap_level, std::min(sch->max_level - 1, H->nlev - 1)), lo = std::max(t.min_level, 0);
        for (int l = lo; l <= top; l++) {
            if ((rc = suhmo_hier_tag_cells(H, l, t.field, t.vmin, t.vmax, t.grow, t.grow_x, t.grow_y, g, s))) return rc;
            if (sch->subset_nbox && sch->subset_nbox[l] > 0 && (rc = suhmo_hier_restrict_tags(H, l, sch->subset_nbox[l], subset_of(sch, l), s))) return rc;
        }
    }
    int nlev = 0, nbox[9] = {}, same = 0;
    std::vector<int> boxes(4 * 256);
    rc = suhmo_hier_generate_grids(H, &sch->grid, &nlev, nbox, boxes.data(), (int)(boxes.size() / 4), &same);
    if (rc == -4) {
        long total = 0;
        for (int l = 1; l < nlev; l++) total += nbox[l];
        boxes.assign(4 * (size_t)total, 0);
        rc = suhmo_hier_generate_grids(H, &sch->grid, &nlev, nbox, boxes.data(), (int)total, &same);
    }
    if (rc) return rc;
    // a regrid is logged and counted once it is done: for lists suhmo_hier_create refuses there is no entry, and the hierarchy is the old one
    const int idx = res->n_regrids;
    auto log = [&]() {
        if (res->regrids && idx < res->regrids_cap) {
            suhmo_hier_regrid_log_t &e = res->regrids[idx];
            e.cur_step = c; e.same = same; e.nlev = nlev;
            for (int l = 0; l < 8; l++) e.nbox[l] = l < nlev ? nbox[l] : 0;
        }
        res->n_regrids = idx + 1;
    };
    if (same) { log(); return 0; }
    const long carried[7] = {H->n_recharge_launches, H->n_moulin_calls, H->n_run_readbacks, H->n_snap_launches, H->n_snap_copies, H->n_wb_launches, H->n_wb_copies};
    suhmo_hier *N = nullptr;
    if ((rc = suhmo_hier_regrid(H, nlev, nbox, boxes.data(), sch->n_fields, sch->fields, &N, s))) return rc;      // (H is untouched and usable)
    N->n_recharge_launches = carried[0]; N->n_moulin_calls = carried[1]; N->n_run_readbacks = carried[2];
    N->n_snap_launches = carried[3]; N->n_snap_copies = carried[4];
    N->n_wb_launches = carried[5]; N->n_wb_copies = carried[6];
    *Hp = N;
    *changed = true;
    log();
    res->n_moved++;
    if (sch->reload) {
        const int r = sch->reload(sch->user, N, idx, c);
        if (r) { suhmo_set_error("suhmo_hier_run: reload returned %d after regrid %d (before the step with cur_step %d)", r, idx, c); return -1; }
    }
    // the seasonal recharge reads SUHMO_F_ZS of every box: the new boxes hold it only when the transfer's field list or `reload` brought it
    if ((sch->T_K || sch->background) && (rc = suhmo_hier_recharge_check_(N, "suhmo_hier_run: after a regrid"))) return rc;
    return 0;
}
// the plot files and checkpoints of a run: one snapshot per event into a pinned buffer the run owns, then the caller's callback
struct Output {
    const suhmo_hier_output_t *o;
    double *pinned = nullptr; size_t cap = 0;
    std::vector<long> lo, bo;
    long n[2] = {0, 0};
    explicit Output(const suhmo_hier_output_t *out) : o(out) {}
    ~Output() { if (pinned) (void)hipHostFree(pinned); }
    bool plot_before(int b) const { return o && o->plot_interval > 0 && b % o->plot_interval == 0; }                                        // :1311
    bool check_before(int b) const { return o && o->check_interval > 0 && b % o->check_interval == 0 && b != o->restart_step; }             // :1327
    // kind 0 plot, 1 checkpoint; cur_step: m_cur_step of the file name
    int emit(suhmo_hier *H, int kind, int cur_step, suhmo_stream_t s)
    {
        const int ncomp = kind ? o->n_check : o->n_plot;
        const suhmo_snap_comp_t *comps = kind ? o->check : o->plot;
        size_t nbox = 0;
        for (int l = 0; l < H->nlev; l++) nbox += H->lev[l].box.size();
        lo.assign(H->nlev + 1, 0); bo.assign(nbox + H->nlev, 0);
        const size_t need = (size_t)suhmo_hier_snapshot_sizes_(H, ncomp, 1, nullptr, nullptr);
        if (need > cap) {
            if (pinned) { HIPCHK(hipHostFree(pinned)); pinned = nullptr; cap = 0; }
            HIPCHK(hipHostMalloc(&pinned, need * sizeof(double), hipHostMallocDefault));
            cap = need;
        }
        int rc = suhmo_hier_snapshot(H, ncomp, comps, 1, lo.data(), bo.data(), pinned, s);
        if (rc) return rc;
        const int r = o->write(o->user, H, kind, cur_step, ncomp, lo.data(), bo.data(), pinned);
        if (r) {
            suhmo_set_error("suhmo_hier_run: write returned %d for the %s with cur_step %d", r, kind ? "checkpoint" : "plot", cur_step);
            return -1;
        }
        n[kind]++;
        return 0;
    }
};
}  // namespace

extern "C" int suhmo_hier_run(suhmo_hier_t **Hp, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, suhmo_hier_run_result_t *res,
                              suhmo_stream_t s)
{
    return suhmo_hier_run_out(Hp, mp, sch, nullptr, res, s);
}

extern "C" int suhmo_hier_run_out(suhmo_hier_t **Hp, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, const suhmo_hier_output_t *out,
                                  suhmo_hier_run_result_t *res, suhmo_stream_t s)
{
    return suhmo_hier_run_bud(Hp, mp, sch, out, nullptr, res, s);
}

// bud != NULL: a budget row of every level after the steps that end one.  Those steps run with track_old_volume = 1 (the volume is measured
// inside the step: behind its regrid, reload and forcing), the others with the caller's setting, which is put back right behind the step -- so
// every way out leaves it.  A regrid hands the setting to the new handle with the other options; the series stays with the run
extern "C" int suhmo_hier_run_bud(suhmo_hier_t **Hp, const suhmo_model_params_t *mp, const suhmo_hier_schedule_t *sch, const suhmo_hier_output_t *out,
                                  suhmo_run_budget_t *bud, suhmo_hier_run_result_t *res, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::run");
    ARG(Hp && *Hp && mp && sch && res);
    suhmo_hier *H = *Hp;
    hipStream_t st = HST(s);
    res->steps_done = 0; res->n_rows = 0; res->n_regrids = 0; res->n_moved = 0;
    if (bud) bud->n_rows = 0;
    int rc;
    // ---- everything that can be refused, before anything is launched
    if (sch->n_steps < 1) { suhmo_set_error("suhmo_hier_run: n_steps = %d (at least 1)", sch->n_steps); return -1; }
    if (!(sch->dt > 0.0) || sch->first_cur_step < 1 || sch->diag_every < 0) { suhmo_set_error("suhmo_hier_run: dt > 0, first_cur_step >= 1 and diag_every >= 0"); return -1; }
    if (H->world > 1 || H->part) { suhmo_set_error("suhmo_hier_run: a hierarchy on rank strips (or with levels dealt to the ranks) is not built"); return -5; }
    const bool recharge = sch->T_K || sch->background;
    const bool moulins = sch->n_moulins != 0 || sch->positions || sch->sigma || sch->flux || sch->moulin_factor;
    if (recharge && !(sch->T_K && sch->background)) { suhmo_set_error("suhmo_hier_run: a temperature schedule needs T_K and background"); return -1; }
    if (moulins && !(sch->n_moulins > 0 && sch->positions && sch->sigma && sch->flux)) {
        suhmo_set_error("suhmo_hier_run: a moulin schedule needs n_moulins >= 1, positions, sigma and flux"); return -1;
    }
    if (recharge && moulins) { suhmo_set_error("suhmo_hier_run: a temperature schedule and a moulin schedule write the same source term (SUHMO_F_MSRC): give one"); return -1; }
    if (moulins) for (int m = 0; m < sch->n_moulins; m++) if (!(sch->sigma[m] > 0.0)) { suhmo_set_error("suhmo_hier_run: sigma of moulin %d is not positive", m); return -1; }
    if (sch->regrid_interval < 0) { suhmo_set_error("suhmo_hier_run: regrid_interval = %d", sch->regrid_interval); return -1; }
    const suhmo_level *B = base_of(H);
    if (sch->regrid_interval > 0) {
        if (sch->n_tags < 1 || !sch->tags) { suhmo_set_error("suhmo_hier_run: regrid_interval = %d without tag variables", sch->regrid_interval); return -1; }
        if (sch->max_level < 1 || sch->max_level > 8) { suhmo_set_error("suhmo_hier_run: max_level = %d (1 .. 8)", sch->max_level); return -1; }
        if (sch->fields ? (sch->n_fields < 0 || sch->n_fields > 16) : false) { suhmo_set_error("suhmo_hier_run: n_fields = %d (at most 16)", sch->n_fields); return -1; }
        {   // the grid parameters, as suhmo_grids_generate judges them (a map without tags: nothing is generated)
            const DV &v = B->d[0].v;
            std::vector<unsigned char> none((size_t)v.nxg * v.nyg, 0);
            const unsigned char *ptr = none.data();
            int nl = 0, nb[2] = {};
            if ((rc = suhmo_grids_generate(v.nxg, v.nyg, H->bc.periodic, &sch->grid, 1, &ptr, &nl, nb, nullptr, 0))) return rc;
        }
        const int g = sch->grid.block_factor / 2;
        for (int m = 0; m < sch->n_tags; m++) {
            const suhmo_tag_spec_t &t = sch->tags[m];
            if (t.field < 0 || t.field >= SUHMO_F_COUNT || t.grow < 0 || t.grow_x < 0 || t.grow_y < 0) { suhmo_set_error("suhmo_hier_run: tag variable %d: field %d, grow %d / %d / %d", m, t.field, t.grow, t.grow_x, t.grow_y); return -1; }
        }
        if ((sch->subset_nbox == nullptr) != (sch->subset_boxes == nullptr)) { suhmo_set_error("suhmo_hier_run: tag subsets need subset_nbox and subset_boxes"); return -1; }
        if (sch->subset_nbox) {
            const int *q = sch->subset_boxes;
            for (int l = 0; l < sch->max_level; l++) {
                if (sch->subset_nbox[l] < 0) { suhmo_set_error("suhmo_hier_run: subset_nbox[%d] = %d", l, sch->subset_nbox[l]); return -1; }
                for (int k = 0; k < sch->subset_nbox[l]; k++, q += 4)
                    if (q[0] > q[2] || q[1] > q[3] || q[0] % g || q[1] % g || (q[2] + 1) % g || (q[3] + 1) % g) {
                        suhmo_set_error("suhmo_hier_run: subset box %d of level %d (%d, %d, %d, %d) is empty or not aligned to block_factor / 2 = %d", k, l, q[0], q[1], q[2], q[3], g);
                        return -1;
                    }
            }
        }
    }
    if (out) {
        if (out->plot_interval < -1 || out->check_interval < -1) { suhmo_set_error("suhmo_hier_run: plot_interval = %d, check_interval = %d (-1: off)", out->plot_interval, out->check_interval); return -1; }
        const bool plots = out->plot_interval >= 0, checks = out->check_interval >= 0;
        if ((plots || checks) && !out->write) { suhmo_set_error("suhmo_hier_run: output without a callback to write it"); return -1; }
        if ((plots && (out->n_plot < 1 || !out->plot)) || (checks && (out->n_check < 1 || !out->check))) { suhmo_set_error("suhmo_hier_run: output without a component list"); return -1; }
        if (plots && (rc = suhmo_hier_snapshot_check_(H, "suhmo_hier_run: plot components", out->n_plot, out->plot, 1))) return rc;
        if (checks && (rc = suhmo_hier_snapshot_check_(H, "suhmo_hier_run: checkpoint components", out->n_check, out->check, 1))) return rc;
    }
    if (recharge && (rc = suhmo_hier_recharge_check_(H, "suhmo_hier_run"))) return rc;
    if (mp->use_moulin_source && !recharge && !moulins)
        for (int l = 0; l < H->nlev; l++)
            for (size_t k = 0; k < H->lev[l].box.size(); k++)
                if (!H->lev[l].box[k]->d[0].fp.f[SUHMO_F_MSRC]) {
                    suhmo_set_error("suhmo_hier_run: use_moulin_source without a source term (level %d, box %d) or a schedule that writes one", l, (int)k); return -1;
                }
    if ((rc = suhmo_step_check_args_(mp, sch->dt, sch->first_cur_step))) return rc;
    const int total_rows = sch->diag_every ? sch->n_steps / sch->diag_every : 0;
    if (total_rows > 0 && !res->rows) { suhmo_set_error("suhmo_hier_run: %d rows and no array for them", total_rows); return -1; }
    if (total_rows > 0 && (rc = suhmo_level_postproc_row_check_(base_of(H), mp, recharge || moulins))) return rc;
    if (bud) {
        if (bud->every < 1) { suhmo_set_error("suhmo_hier_run: a budget row every %d steps (at least 1)", bud->every); return -1; }
        if (!bud->rows || !bud->nlev) { suhmo_set_error("suhmo_hier_run: a budget series needs the arrays rows and nlev"); return -1; }
        const int need = sch->regrid_interval > 0 ? std::max(std::min(sch->max_level + 1, 8), H->nlev) : H->nlev;     // (at most 8 levels: suhmo_hier_create)
        if (bud->lev_cap < need) { suhmo_set_error("suhmo_hier_run: budget rows with room for %d levels, the run can have %d", bud->lev_cap, need); return -1; }
        // (the face coefficients and the melt rate are the first step's to form; the source term is the rule above)
        if ((rc = suhmo_hier_budget_check_(H, mp, "suhmo_hier_run: budget", false, false))) return rc;
    }
    if ((rc = suhmo_hier_check_(H))) return rc;
    HIPCHK(hipSetDevice(H->device));
    // ---- the budget series [rows][lev_cap][10] on the device for the length of the run, and where its one copy lands
    const int total_wb = bud ? sch->n_steps / bud->every : 0;
    const size_t wper = bud ? (size_t)SUHMO_WB_COUNT * bud->lev_cap : 0;
    double *wseries = nullptr;
    if (total_wb > 0) HIPCHK(hipMalloc(&wseries, total_wb * wper * sizeof(double)));
    const long track = H->track_old_volume;
    int wrows = 0;
    // ---- the series [rows][6] and the column sums of one row, on the device for the length of the run
    const size_t ncol = 8 * (size_t)B->d[0].v.nx;
    double *series = nullptr;
    if (total_rows > 0 && hipMalloc(&series, (6 * (size_t)total_rows + ncol) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        if (wseries) (void)hipFree(wseries);
        suhmo_set_error("suhmo_hier_run: the series (%zu doubles) cannot be allocated", 6 * (size_t)total_rows + ncol); return -2;
    }
    double *cols = series ? series + 6 * (size_t)total_rows : nullptr;
    int rows = 0;
    rc = 0;
    Output output(out && (out->plot_interval >= 0 || out->check_interval >= 0) ? out : nullptr);
    for (int k = 0; k < sch->n_steps; k++) {
        const int c = sch->first_cur_step + k;
        bool changed = false;
        // 0. plot file: the state before the regrid
        if (output.plot_before(c - 1) && (rc = output.emit(H, 0, c - 1, s))) break;
        // 1. regrid
        if (regrid_due(sch, k)) {
            rc = run_regrid(Hp, sch, c, res, &changed, s);
            H = *Hp;
            if (rc) break;
        }
        // 1b. checkpoint: on the boxes the regrid left
        if (output.check_before(c - 1) && (rc = output.emit(H, 1, c - 1, s))) break;
        // 2. forcing
        if (recharge && (rc = suhmo_hier_recharge_launch_(H, sch->T_K[k], sch->background[k], st))) break;
        const double factor = sch->moulin_factor ? sch->moulin_factor[k] : 1.0;
        const bool form = moulins && (k == 0 || changed || !same_bits(factor, sch->moulin_factor ? sch->moulin_factor[k - 1] : 1.0));
        if (res->moulin_steps) res->moulin_steps[k] = form;
        if (form && (rc = suhmo_hier_moulin_source(H, sch->n_moulins, sch->positions, sch->sigma, sch->flux, factor, nullptr, s))) break;
        // 3. time step
        suhmo_model_params_t mpk = *mp;
        if (sch->ramp) mpk.ramp = sch->ramp[k];
        int pi = 0, nv = 0;
        const bool brow = total_wb > 0 && (k + 1) % bud->every == 0;
        if (brow) H->track_old_volume = 1;
        rc = suhmo_hier_timestep(H, &mpk, sch->dt, c, &pi, &nv, s);
        H->track_old_volume = track;
        if (rc) break;
        if (res->picard_iters) res->picard_iters[k] = pi;
        if (res->vcycles) res->vcycles[k] = nv;
        res->steps_done = k + 1;
        // 4. diagnostic row
        if (sch->diag_every && (k + 1) % sch->diag_every == 0) {
            if ((rc = suhmo_level_postproc_row_launch_(base_of(H), &mpk, cols, series + 6 * (size_t)rows, st))) break;
            rows++;
        }
        // 5. budget row: the levels the hierarchy has now
        if (brow) {
            if ((rc = suhmo_hier_budget_launch_(H, &mpk, wseries + wrows * wper, st))) break;
            bud->nlev[wrows++] = H->nlev;
        }
    }
    // the files after the last step (:1343-1358)
    if (!rc && output.o && !out->no_final) {
        const int last = sch->first_cur_step + sch->n_steps - 1;
        if (out->plot_interval >= 0) rc = output.emit(H, 0, last, s);
        if (!rc && out->check_interval >= 0) rc = output.emit(H, 1, last, s);
    }
    H->n_run_plots = output.n[0]; H->n_run_checkpoints = output.n[1];
    res->n_rows = rows;
    int rc2 = 0;
    if (rows > 0) {
        const std::string msg = rc ? suhmo_last_error() : "";
        hipError_t e = hipMemcpyAsync(res->rows, series, 6 * (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        H->n_run_readbacks++;
        if (e != hipSuccess) { suhmo_set_error("suhmo_hier_run: copy of the series: %s", hipGetErrorString(e)); rc2 = -2; }
        else if (rc) suhmo_set_error("%s", msg.c_str());
    } else if (series) (void)hipStreamSynchronize(st);
    if (series) (void)hipFree(series);
    // the budget rows finished so far: one copy, then the levels each row has (the other entries keep the caller's values)
    if (wrows > 0) {
        const std::string msg = rc ? suhmo_last_error() : "";
        std::vector<double> h(wrows * wper);
        hipError_t e = hipMemcpyAsync(h.data(), wseries, h.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        H->n_wb_copies++;
        if (e != hipSuccess) { suhmo_set_error("suhmo_hier_run: copy of the budget series: %s", hipGetErrorString(e)); rc2 = rc2 ? rc2 : -2; }
        else {
            for (int r = 0; r < wrows; r++) memcpy(bud->rows + r * wper, h.data() + r * wper, (size_t)SUHMO_WB_COUNT * bud->nlev[r] * sizeof(double));
            bud->n_rows = wrows;
            if (rc) suhmo_set_error("%s", msg.c_str());
        }
    } else if (wseries) (void)hipStreamSynchronize(st);
    if (wseries) (void)hipFree(wseries);
    return rc ? rc : rc2;
}
