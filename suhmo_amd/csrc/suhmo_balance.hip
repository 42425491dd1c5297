// suhmo_balance.hip -- the mass balance of a level, of every level of a hierarchy, of the members of an ensemble, reduced on the device:
// AmrHydro::check_fluxes (src/AmrHydro.cpp:440-590), the third part of the post_proc block that ends every timeStepFAS (:3643-3652) -- the
// discharge through the four domain sides, through the ice margin and the ice-bearing domain sides, and the water volume.  The rule and the
// refusals: include/suhmo_hip.h, "MASS BALANCE"; the per-face and per-cell arithmetic: suhmo_balance.h; the order of the sums: suhmo_reduce.h;
// tests/massbalance_ref.py is the numpy twin of all three.  Read-only.
// The water budget ("WATER BUDGET" there; tests/budget_ref.py) is the same walk with two more arrays and two more sums: k_budget (head, mask, B, BX,
// BY, MR, MSRC: nine values per workgroup), k_volume (mask and B: the volume alone, left on the device by a tracked time step before it writes b)
// and k_budget_final (a workgroup per level / flagged member: the nine sums, VOLUME_OLD from the kept volume partials, ten doubles to an address
// the caller names -- a buffer that is copied once, or a row of a run's series).
//
// Per call, on one stream:
//   k_balance        the first stage of suhmo_reduce.h over the cells of a level (CAP_LEVEL), of the boxes of a level (CAP_BOX on the largest box
//                    extents, one grid for all boxes) or of the flagged members of an ensemble (CAP_LEVEL): seven values per workgroup
//   k_balance_final  ONE launch: the second stage per level of a hierarchy / per flagged member, a workgroup each (thread t takes the partials
//                    t, t + 256, ..., then the tree); one hipMemcpyAsync of what it leaves, one synchronisation
// k_balance walks as every first stage does: a wave owns 64 consecutive cells of a row, so each of its loads of head, mask, B, BX and BY at the
// cell is 64 consecutive doubles.  The west values are the same lines one double to the left; the south row is the row the wave below in the
// workgroup (or the workgroup below) loads as its own: both come from cache, HBM is read once, 5 arrays x 8 B per cell.  The east and north
// values are loaded by the last column and the last row alone.  Plain vector loads and stores, no atomics, no LDS beyond block_tree's.
#include "suhmo_hier_int.h"
#include "suhmo_level_int.h"
#include "suhmo_batch.h"
#include "suhmo_reduce.h"
#include "suhmo_balance.h"

using namespace hier;

namespace {
using Red = RedSum7;
constexpr int NV = SUHMO_MB_COUNT;
static_assert(Red::NV == SUHMO_MB_COUNT, "one accumulator per value of the mass balance");
constexpr size_t LEVEL_PARTIALS = (size_t)CAP_LEVEL.x * CAP_LEVEL.y;

// the workgroup's seven values: partial + 7 * (its place in the list of its level / among the members' lists)
template <class T> __global__ __launch_bounds__(256) void k_balance(T t, double *__restrict__ partial)
{
    const DV &v = t.view();
    const FP &fp = t.fields();
    const double *__restrict__ head = fp.f[SUHMO_F_PHI], *__restrict__ mask = fp.f[SUHMO_F_MASK], *__restrict__ B = fp.f[SUHMO_F_B];
    const double *__restrict__ bx = fp.f[SUHMO_F_BX], *__restrict__ by = fp.f[SUHMO_F_BY];
    // (a wave of BLK2D is one row of the walk: j as a scalar makes the row's tests -- first row, last row, the sides in y -- scalar branches and
    //  the row's address scalar arithmetic, which halves the scalar registers the tests kept as lane masks)
    reduce_cells<Red>(v, partial + NV * (t.slot((size_t)gridDim.x * gridDim.y) + plane_block()),
                      [&](int i, int j, double (&a)[NV]) { mb_fold(v, head, mask, B, bx, by, i, __builtin_amdgcn_readfirstlane(j), a); });
}

// the water budget's first stage: k_balance's walk and fold, then the cell's two recharge terms; nine values per workgroup.  t.model(): ramp,
// distributed_input, rho_w, use_moulin_source (a member's own row; by value for a level or the boxes of a level)
using RedW = RedSum9;
constexpr int NW = WB_P_COUNT;
static_assert(RedW::NV == WB_P_COUNT && SUHMO_WB_COUNT == WB_P_COUNT + 1 && SUHMO_WB_VOLUME_OLD == SUHMO_MB_COUNT, "seven values, VOLUME_OLD, the two recharge sums");
template <class T> __global__ __launch_bounds__(256) void k_budget(T t, double *__restrict__ partial)
{
    const DV &v = t.view();
    const FP &fp = t.fields();
    const suhmo_model_params_t &mp = t.model();
    const double *__restrict__ head = fp.f[SUHMO_F_PHI], *__restrict__ mask = fp.f[SUHMO_F_MASK], *__restrict__ B = fp.f[SUHMO_F_B];
    const double *__restrict__ bx = fp.f[SUHMO_F_BX], *__restrict__ by = fp.f[SUHMO_F_BY], *__restrict__ mr = fp.f[SUHMO_F_MR];
    const double *__restrict__ ms = mp.use_moulin_source ? fp.f[SUHMO_F_MSRC] : nullptr;
    const double ramp = mp.ramp, din = mp.distributed_input, rho_w = mp.rho_w;
    reduce_cells<RedW>(v, partial + NW * (t.slot((size_t)gridDim.x * gridDim.y) + plane_block()),
                       [&](int i, int j, double (&a)[NW]) { wb_fold(v, head, mask, B, bx, by, mr, ms, ramp, din, rho_w, i, __builtin_amdgcn_readfirstlane(j), a); });
}
// the volume alone (mb_cell, the term k_balance folds last): ONE value per workgroup, on k_balance's grid, so that what the second stage makes of
// these partials is bit for bit the VOLUME of a mass balance of the same state
template <class T> __global__ __launch_bounds__(256) void k_volume(T t, double *__restrict__ partial)
{
    const DV &v = t.view();
    const FP &fp = t.fields();
    const double *__restrict__ mask = fp.f[SUHMO_F_MASK], *__restrict__ B = fp.f[SUHMO_F_B];
    reduce_cells<RedSum>(v, partial + t.slot((size_t)gridDim.x * gridDim.y) + plane_block(), [&](int i, int j, double (&a)[1]) {
        const int idx = cidx(v, i, __builtin_amdgcn_readfirstlane(j));
        mb_cell(mask[idx], B[idx], v.dx, v.dy, a[0]);
    });
}

// the second stage of suhmo_reduce.h (k_norm_final's walk over ONE list): thread t takes the partials t, t + 256, ... of the list, then the tree
template <class R> __device__ __forceinline__ void second_stage(const double *__restrict__ p, int n, int tid, double (&a)[R::NV])
{
#pragma unroll
    for (int q = 0; q < R::NV; q++) a[q] = R::init(q);
    for (int e = tid; e < n; e += 256) {
#pragma unroll
        for (int q = 0; q < R::NV; q++) a[q] = red_op<R>(q, a[q], p[R::NV * e + q]);
    }
    block_tree<R>(tid, a);
}
// ... for workgroup b: list b of pl -> out[b] (the levels of a hierarchy), or, where sel.n > 0, the np partials of member sel.m[b] behind
// pl.p[0] -> out[that member]
struct BalLists { PartialLists pl; BatchSel sel; int np; };
__global__ __launch_bounds__(256) void k_balance_final(BalLists bl, double *__restrict__ out)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    const double *__restrict__ p = bl.pl.p[0];
    int n = bl.np, k = b;
    if (bl.sel.n > 0) { k = bl.sel.m[b]; p += (size_t)NV * bl.np * k; }
    else {
#pragma unroll
        for (int l = 0; l < RED_LISTS; l++) if (l == b) { p = bl.pl.p[l]; n = bl.pl.n[l]; }     // (constants only: the table stays in scalar registers)
    }
    double a[NV];
    second_stage<Red>(p, n, tid, a);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < NV; q++) out[(size_t)NV * k + q] = a[q];
    }
}
// the same for a budget: the nine sums of list b / member sel.m[b], and VOLUME_OLD from the kept volume partials -- `old`, laid out like pl with one
// value per partial (a member's npo = old.n[0] partials behind old.p[0]); a level with old.n <= 0, a member without its bit in `have`: a quiet NaN
struct BudLists { PartialLists pl, old; BatchSel sel; int np; unsigned long long have; };
__global__ __launch_bounds__(256) void k_budget_final(BudLists bl, double *__restrict__ out)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    const double *__restrict__ p = bl.pl.p[0], *__restrict__ po = bl.old.p[0];
    int n = bl.np, no = bl.old.n[0], k = b;
    if (bl.sel.n > 0) {
        k = bl.sel.m[b];
        p += (size_t)NW * bl.np * k;
        po += (size_t)(no > 0 ? no : 0) * k;
        if (!((bl.have >> k) & 1ull)) no = 0;
    } else {
#pragma unroll
        for (int l = 0; l < RED_LISTS; l++) if (l == b) { p = bl.pl.p[l]; n = bl.pl.n[l]; po = bl.old.p[l]; no = bl.old.n[l]; }
    }
    double a[NW], o[1];
    second_stage<RedW>(p, n, tid, a);
    second_stage<RedSum>(po, no, tid, o);
    if (tid == 0) {
        double *__restrict__ row = out + (size_t)SUHMO_WB_COUNT * k;
#pragma unroll
        for (int q = 0; q < SUHMO_MB_COUNT; q++) row[q] = a[q];
        row[SUHMO_WB_VOLUME_OLD] = no > 0 ? o[0] : __longlong_as_double(0x7ff8000000000000ll);
        row[SUHMO_WB_RECH_EXT] = a[WB_P_EXT];
        row[SUHMO_WB_RECH_MELT] = a[WB_P_MELT];
    }
}
int launch_budget_final(const BudLists &bl, int groups, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_budget_final, dim3(groups), dim3(256), 0, st, bl, out);
    HIPCHK(hipGetLastError());
    return 0;
}
int launch_balance_final(const BalLists &bl, int groups, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_balance_final, dim3(groups), dim3(256), 0, st, bl, out);
    HIPCHK(hipGetLastError());
    return 0;
}

// what a level, a box or a member must hold before the call reads it; what: how the message names it ("the level", "box 3 of level 1", "member 2")
int check_state(const suhmo_level *L, const char *who, const std::string &what)
{
    const FP &fp = L->d[0].fp;
    for (int f : {SUHMO_F_PHI, SUHMO_F_MASK, SUHMO_F_B, SUHMO_F_BX, SUHMO_F_BY})
        if (!fp.f[f]) { suhmo_set_error("%s: %s does not hold field %d", who, what.c_str(), f); return -1; }
    if (!L->faces_made) {
        suhmo_set_error("%s: %s has no face coefficients yet: no solve, step or UpdateOperator has run on it", who, what.c_str()); return -1;
    }
    return 0;
}
// partials a hierarchy can leave: level 0 under CAP_LEVEL, 64 per box
size_t partial_cap(const suhmo_hier *H)
{
    size_t n = LEVEL_PARTIALS;
    for (int l = 1; l < H->nlev; l++) n += 64 * H->lev[l].box.size();
    return n;
}
}  // namespace

void suhmo_hier_balance_release_(suhmo_hier *H)
{
    if (H->bal_buf) (void)hipFree(H->bal_buf);
    H->bal_buf = nullptr; H->bal_cap = 0;
    if (H->wb_buf) (void)hipFree(H->wb_buf);
    if (H->vol_buf) (void)hipFree(H->vol_buf);
    H->wb_buf = H->vol_buf = nullptr; H->wb_cap = H->vol_cap = 0;
    for (int &n : H->vol_n) n = 0;
}

extern "C" int suhmo_level_mass_balance(suhmo_level_t *L, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("check_fluxes");
    const char *who = "suhmo_level_mass_balance";
    ARG(L && out);
    if (L->stub || L->desc.nx_global > 0) { suhmo_set_error("%s: a box of a hierarchy or a nested patch: not built (suhmo_hier_mass_balance takes a hierarchy)", who); return -5; }
    const DV &v = L->d[0].v;
    if (on_strip(L) || v.ext[0] || v.ext[1]) { suhmo_set_error("%s: a rank strip: not built", who); return -5; }
    int rc;
    if ((rc = check_state(L, who, "the level"))) return rc;
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = HST(s);
    if (!L->bal_buf && hipMalloc(&L->bal_buf, NV * (LEVEL_PARTIALS + 1) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        L->bal_buf = nullptr;
        suhmo_set_error("%s: the partial buffer cannot be allocated", who); return -2;
    }
    int np = 0;
    if ((rc = launch_partials(k_balance<OnLevel>, on_level(L, 0), CAP_LEVEL, L->bal_buf, &np, st))) return rc;
    BalLists bl{};
    bl.pl = one_list(L->bal_buf, np);
    double *res = L->bal_buf + NV * LEVEL_PARTIALS;
    if ((rc = launch_balance_final(bl, 1, res, st))) return rc;
    double h[NV];
    HIPCHK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, h, sizeof(h));
    return 0;
}

extern "C" int suhmo_hier_mass_balance(suhmo_hier_t *H, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("check_fluxes");
    const char *who = "suhmo_hier_mass_balance";
    ARG(H && out);
    ARG(H->nlev >= 1);
    if (H->world > 1 || H->part || H->shadowed) {
        suhmo_set_error("%s: a hierarchy on rank strips, with levels dealt to the ranks or created with shadow = 1 is not built", who); return -5;
    }
    const int nlev = H->nlev;
    int rc;
    for (int l = 0; l < nlev; l++)
        for (size_t k = 0; k < H->lev[l].box.size(); k++) {
            if (H->lev[l].box[k]->stub) { suhmo_set_error("%s: box %zu of level %d is held by another rank: not built", who, k, l); return -5; }
            if ((rc = check_state(H->lev[l].box[k], who, "box " + std::to_string(k) + " of level " + std::to_string(l)))) return rc;
        }
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(H->device));
    const size_t cap = partial_cap(H);
    if (!H->bal_buf) {
        const size_t n = NV * (cap + RED_LISTS);
        if (hipMalloc(&H->bal_buf, n * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            H->bal_buf = nullptr;
            suhmo_set_error("%s: the partial buffer (%zu doubles) cannot be allocated", who, n); return -2;
        }
        H->bal_cap = n;
    }
    BalLists bl{};
    size_t off = 0;
    for (int l = 0; l < nlev; l++) {
        double *partial = H->bal_buf + NV * off;
        int np = 0;
        rc = on_hier_level(H, l, st, [&](const auto &t) {
            int per = 0;
            const int r = launch_partials(k_balance<std::decay_t<decltype(t)>>, t, l == 0 ? CAP_LEVEL : CAP_BOX, partial, &per, st);
            np = per * t.count();
            return r;
        });
        if (rc) return rc;
        H->n_bal_launches++;
        bl.pl.p[l] = partial; bl.pl.n[l] = np; off += (size_t)np;
    }
    bl.pl.cnt = nlev;
    double *res = H->bal_buf + NV * cap;
    if ((rc = launch_balance_final(bl, nlev, res, st))) return rc;
    H->n_bal_launches++;
    double h[NV * RED_LISTS];
    HIPCHK(hipMemcpyAsync(h, res, (size_t)NV * nlev * sizeof(double), hipMemcpyDeviceToHost, st));
    H->n_bal_copies++;
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, h, (size_t)NV * nlev * sizeof(double));
    return 0;
}

// the flagged members of an ensemble (suhmo_batch.hip: suhmo_batch_mass_balance, which owns the buffers): one first stage, np partials per member
// behind partial (room for CAP_LEVEL's), then one final launch into out[member][7]
size_t suhmo_balance_member_doubles() { return NV * LEVEL_PARTIALS; }
int suhmo_balance_check_member_(const suhmo_level *L, int k) { return check_state(L, "suhmo_batch_mass_balance", "member " + std::to_string(k)); }
int launch_mass_balance(const OnMembers &t, double *partial, double *out, hipStream_t st)
{
    int np = 0, rc = launch_partials(k_balance<OnMembers>, t, CAP_LEVEL, partial, &np, st);
    if (rc) return rc;
    BalLists bl{};
    bl.pl = one_list(partial, np);
    bl.sel = t.sel; bl.np = np;
    return launch_balance_final(bl, t.sel.n, out, st);
}

// ------------------------------------------------------------------ the water budget (include/suhmo_hip.h, "WATER BUDGET")
namespace {
int dev_alloc(double **p, size_t n, const char *who, const char *what)
{
    if (*p) return 0;
    if (hipMalloc(p, n * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        suhmo_set_error("%s: %s (%zu doubles) cannot be allocated", who, what, n); return -2;
    }
    return 0;
}
// what a budget reads of a level, a box or a member.  faces: the face coefficients and SUHMO_F_MR must be there (a run leaves both to its first
// step and asks for the fields a caller loads only); source: with use_moulin_source, SUHMO_F_MSRC must be there now
int check_budget(const suhmo_level *L, const suhmo_model_params_t *mp, const char *who, const std::string &what, bool faces, bool source)
{
    const FP &fp = L->d[0].fp;
    int rc;
    if (faces) {
        if ((rc = check_state(L, who, what))) return rc;
        if (!fp.f[SUHMO_F_MR]) { suhmo_set_error("%s: %s does not hold the melt rate (SUHMO_F_MR): no time step has run on it", who, what.c_str()); return -1; }
    } else
        for (int f : {SUHMO_F_PHI, SUHMO_F_MASK, SUHMO_F_B})
            if (!fp.f[f]) { suhmo_set_error("%s: %s does not hold field %d", who, what.c_str(), f); return -1; }
    if (source && mp->use_moulin_source && !fp.f[SUHMO_F_MSRC]) {
        suhmo_set_error("%s: use_moulin_source without a source term (SUHMO_F_MSRC) on %s", who, what.c_str()); return -1;
    }
    return 0;
}
int refuse_level(const suhmo_level *L, const char *who)
{
    if (L->stub || L->desc.nx_global > 0) { suhmo_set_error("%s: a box of a hierarchy or a nested patch: not built (a hierarchy has its own call)", who); return -5; }
    const DV &v = L->d[0].v;
    if (on_strip(L) || v.ext[0] || v.ext[1]) { suhmo_set_error("%s: a rank strip: not built", who); return -5; }
    return 0;
}
int refuse_hier(const suhmo_hier *H, const char *who)
{
    if (H->world > 1 || H->part || H->shadowed) {
        suhmo_set_error("%s: a hierarchy on rank strips, with levels dealt to the ranks or created with shadow = 1 is not built", who); return -5;
    }
    for (int l = 0; l < H->nlev; l++)
        for (size_t k = 0; k < H->lev[l].box.size(); k++)
            if (H->lev[l].box[k]->stub) { suhmo_set_error("%s: box %zu of level %d is held by another rank: not built", who, k, l); return -5; }
    return 0;
}
}  // namespace

// ---- the volume a tracked step starts from: the first stage alone, its partials kept by the handle
int suhmo_level_track_volume_(suhmo_level *L, hipStream_t st)
{
    const char *who = "suhmo_level_timestep (track_old_volume)";
    int rc;
    if ((rc = refuse_level(L, who))) return rc;
    const FP &fp = L->d[0].fp;
    if (!fp.f[SUHMO_F_MASK] || !fp.f[SUHMO_F_B]) { suhmo_set_error("%s: the level holds no ice mask or no gap height", who); return -1; }
    if ((rc = dev_alloc(&L->vol_buf, LEVEL_PARTIALS, who, "the volume partials"))) return rc;
    int np = 0;
    if ((rc = launch_partials(k_volume<OnLevel>, on_level(L, 0), CAP_LEVEL, L->vol_buf, &np, st))) return rc;
    L->vol_np = np;
    return 0;
}
int suhmo_hier_track_volume_(suhmo_hier *H, hipStream_t st)
{
    const char *who = "suhmo_hier_timestep (track_old_volume)";
    int rc;
    if ((rc = refuse_hier(H, who))) return rc;
    for (int l = 0; l < H->nlev; l++)
        for (size_t k = 0; k < H->lev[l].box.size(); k++) {
            const FP &fp = H->lev[l].box[k]->d[0].fp;
            if (!fp.f[SUHMO_F_MASK] || !fp.f[SUHMO_F_B]) { suhmo_set_error("%s: box %zu of level %d holds no ice mask or no gap height", who, k, l); return -1; }
        }
    const size_t cap = partial_cap(H);
    if ((rc = dev_alloc(&H->vol_buf, cap, who, "the volume partials"))) return rc;
    H->vol_cap = cap;
    size_t off = 0;
    for (int l = 0; l < H->nlev; l++) {
        double *partial = H->vol_buf + off;
        int np = 0;
        rc = on_hier_level(H, l, st, [&](const auto &t) {
            int per = 0;
            const int r = launch_partials(k_volume<std::decay_t<decltype(t)>>, t, l == 0 ? CAP_LEVEL : CAP_BOX, partial, &per, st);
            np = per * t.count();
            return r;
        });
        if (rc) return rc;
        H->n_wb_launches++;
        H->vol_off[l] = off; H->vol_n[l] = np; off += (size_t)np;
    }
    return 0;
}

// ---- a level
extern "C" int suhmo_level_water_budget(suhmo_level_t *L, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("check_fluxes");
    const char *who = "suhmo_level_water_budget";
    ARG(L && mp && out);
    int rc;
    if ((rc = refuse_level(L, who))) return rc;
    if ((rc = check_budget(L, mp, who, "the level", true, true))) return rc;
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = HST(s);
    if ((rc = dev_alloc(&L->wb_buf, NW * LEVEL_PARTIALS + SUHMO_WB_COUNT, who, "the partial buffer"))) return rc;
    int np = 0;
    const auto t = stepping(on_level(L, 0), *mp);
    if ((rc = launch_partials(k_budget<std::decay_t<decltype(t)>>, t, CAP_LEVEL, L->wb_buf, &np, st))) return rc;
    BudLists bl{};
    bl.pl = one_list(L->wb_buf, np);
    bl.old = one_list(L->vol_buf, L->vol_buf ? L->vol_np : 0);
    double *res = L->wb_buf + NW * LEVEL_PARTIALS;
    if ((rc = launch_budget_final(bl, 1, res, st))) return rc;
    double h[SUHMO_WB_COUNT];
    HIPCHK(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, h, sizeof(h));
    return 0;
}

// ---- a hierarchy
int suhmo_hier_budget_check_(const suhmo_hier *H, const suhmo_model_params_t *mp, const char *who, bool faces, bool source)
{
    int rc;
    if ((rc = refuse_hier(H, who))) return rc;
    for (int l = 0; l < H->nlev; l++)
        for (size_t k = 0; k < H->lev[l].box.size(); k++)
            if ((rc = check_budget(H->lev[l].box[k], mp, who, "box " + std::to_string(k) + " of level " + std::to_string(l), faces, source))) return rc;
    return 0;
}
int suhmo_hier_budget_launch_(suhmo_hier *H, const suhmo_model_params_t *mp, double *out, hipStream_t st)
{
    const char *who = "suhmo_hier_water_budget";
    const size_t cap = partial_cap(H);
    int rc;
    if ((rc = dev_alloc(&H->wb_buf, NW * cap + SUHMO_WB_COUNT * RED_LISTS, who, "the partial buffer"))) return rc;
    H->wb_cap = NW * cap + SUHMO_WB_COUNT * RED_LISTS;
    BudLists bl{};
    size_t off = 0;
    for (int l = 0; l < H->nlev; l++) {
        double *partial = H->wb_buf + NW * off;
        int np = 0;
        rc = on_hier_level(H, l, st, [&](const auto &t) {
            int per = 0;
            const auto ts = stepping(t, *mp);
            const int r = launch_partials(k_budget<std::decay_t<decltype(ts)>>, ts, l == 0 ? CAP_LEVEL : CAP_BOX, partial, &per, st);
            np = per * t.count();
            return r;
        });
        if (rc) return rc;
        H->n_wb_launches++;
        bl.pl.p[l] = partial; bl.pl.n[l] = np; off += (size_t)np;
        bl.old.p[l] = H->vol_buf ? H->vol_buf + H->vol_off[l] : nullptr; bl.old.n[l] = H->vol_buf ? H->vol_n[l] : 0;
    }
    bl.pl.cnt = bl.old.cnt = H->nlev;
    if ((rc = launch_budget_final(bl, H->nlev, out, st))) return rc;
    H->n_wb_launches++;
    return 0;
}
extern "C" int suhmo_hier_water_budget(suhmo_hier_t *H, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("check_fluxes");
    const char *who = "suhmo_hier_water_budget";
    ARG(H && mp && out);
    ARG(H->nlev >= 1);
    int rc;
    if ((rc = suhmo_hier_budget_check_(H, mp, who, true, true))) return rc;
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(H->device));
    const size_t cap = partial_cap(H);
    if ((rc = dev_alloc(&H->wb_buf, NW * cap + SUHMO_WB_COUNT * RED_LISTS, who, "the partial buffer"))) return rc;
    double *res = H->wb_buf + NW * cap;
    if ((rc = suhmo_hier_budget_launch_(H, mp, res, st))) return rc;
    double h[SUHMO_WB_COUNT * RED_LISTS];
    HIPCHK(hipMemcpyAsync(h, res, (size_t)SUHMO_WB_COUNT * H->nlev * sizeof(double), hipMemcpyDeviceToHost, st));
    H->n_wb_copies++;
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, h, (size_t)SUHMO_WB_COUNT * H->nlev * sizeof(double));
    return 0;
}

// ---- the flagged members of an ensemble (suhmo_batch.hip owns the buffers and the bits "member k has a kept volume")
size_t suhmo_budget_member_doubles() { return NW * LEVEL_PARTIALS; }
size_t suhmo_volume_member_doubles() { return LEVEL_PARTIALS; }
int suhmo_budget_check_member_(const suhmo_level *L, const suhmo_model_params_t *mp, int k, const char *who, bool faces, bool source)
{
    return check_budget(L, mp, who, "member " + std::to_string(k), faces, source);
}
int launch_member_volumes(const OnMembers &t, double *vol, int *np, hipStream_t st) { return launch_partials(k_volume<OnMembers>, t, CAP_LEVEL, vol, np, st); }
int launch_water_budget(const OnMembers &t, double *partial, const double *vol, int npo, unsigned long long have, double *out, hipStream_t st)
{
    int np = 0, rc = launch_partials(k_budget<OnMembers>, t, CAP_LEVEL, partial, &np, st);
    if (rc) return rc;
    BudLists bl{};
    bl.pl = one_list(partial, np);
    bl.old = one_list(vol, vol ? npo : 0);
    bl.sel = t.sel; bl.np = np; bl.have = vol ? have : 0ull;
    return launch_budget_final(bl, t.sel.n, out, st);
}
