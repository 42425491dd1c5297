// suhmo_ibc.hip -- the reference's IBC classes on the device: the first state of a level, a hierarchy or an ensemble (initializeData +
// setup_iceMask, AmrHydro::initData, src/AmrHydro.cpp:5100-5147) and what AmrHydro::regrid evaluates anew on a new level (initializeBed,
// initializePi, setup_iceMask and the ghost fills around them, :4387-4437).  The rule is stated in include/suhmo_hip.h, "INITIAL CONDITIONS";
// tests/ibc_ref.py is its numpy twin; the per-cell functions are suhmo_ibc.h.  Three bodies, each ONE __global__ template over the launch
// target (suhmo_target.h) with the extent GHOSTED: thread (i, j) is cell (i - 1, j - 1) of the box with its ghost ring.  The ghost fills are
// the launches the time step and the regrid use (CopyGhostCells, ExtrapGhostCells, the pwl and exchange plans of a hierarchy).
#include "suhmo_hier_int.h"
#include "suhmo_level_int.h"
#include "suhmo_ibc.h"

using namespace hier;
int suhmo_copy_ghosts(suhmo_level *L, int depth, int field, hipStream_t st);      // suhmo_bcoef.hip: CopyGhostCells of a level

namespace {
// initializeData + setup_iceMask
template <class T, class R> __global__ __launch_bounds__(256) void k_ibc_init(T t, R rows)
{
    const DV &v = t.view();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    const IbcRow &r = row_of(t, rows);
    const FP fp = t.fields();
    const IbcCell c = ibc_initial_cell(r, v, i, j);
    const int idx = cidx(v, i, j);
    fp.f[SUHMO_F_ZB][idx] = c.zb;
    fp.f[SUHMO_F_ZS][idx] = c.zs;
    fp.f[SUHMO_F_PI][idx] = c.Pi;
    fp.f[SUHMO_F_B][idx] = c.b;
    fp.f[SUHMO_F_PW][idx] = c.Pw;
    fp.f[SUHMO_F_PHI][idx] = c.h;
    fp.f[SUHMO_F_MR][idx] = r.p.G / r.p.L;
    fp.f[SUHMO_F_ACOEF][idx] = 0.0;
    fp.f[SUHMO_F_MASK][idx] = ibc_mask_of(c.Pi);
}
// initializeBed + initializePi
template <class T, class R> __global__ __launch_bounds__(256) void k_ibc_reload(T t, R rows)
{
    const DV &v = t.view();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    ibc_reload_cell(row_of(t, rows), v, t.fields(), i, j, cidx(v, i, j));
}
// setup_iceMask
template <class T> __global__ __launch_bounds__(256) void k_ibc_mask(T t)
{
    const DV &v = t.view();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    const FP fp = t.fields();
    const int idx = cidx(v, i, j);
    fp.f[SUHMO_F_MASK][idx] = ibc_mask_of(fp.f[SUHMO_F_PI][idx]);
}
template __global__ void k_ibc_init<OnLevel, IbcRow>(OnLevel, IbcRow);
template __global__ void k_ibc_init<OnBoxes, IbcRow>(OnBoxes, IbcRow);
template __global__ void k_ibc_init<OnMembers, const IbcRow *>(OnMembers, const IbcRow *);
template __global__ void k_ibc_reload<OnLevel, IbcRow>(OnLevel, IbcRow);
template __global__ void k_ibc_reload<OnBoxes, IbcRow>(OnBoxes, IbcRow);
template __global__ void k_ibc_reload<OnMembers, const IbcRow *>(OnMembers, const IbcRow *);
template __global__ void k_ibc_mask<OnLevel>(OnLevel);
template __global__ void k_ibc_mask<OnBoxes>(OnBoxes);
template __global__ void k_ibc_mask<OnMembers>(OnMembers);

const int init_fields[] = {SUHMO_F_ZB, SUHMO_F_ZS, SUHMO_F_PI, SUHMO_F_B, SUHMO_F_PW, SUHMO_F_PHI, SUHMO_F_MR, SUHMO_F_ACOEF, SUHMO_F_MASK};
// what suhmo_level_set_field of the written fields does to a level's bookkeeping
void level_written(suhmo_level *L, bool head)
{
    if (head) phi_changed(L, 0);
    suhmo_mask_written(L);
    suhmo_zb_written(L);
}
int level_fields(suhmo_level *L, const int *f, int n)
{
    for (int q = 0; q < n; q++) if (!suhmo_field(L, 0, f[q])) { suhmo_set_error("ibc: field allocation failed"); return -2; }
    return 0;
}
bool whole_level(const suhmo_level *L)
{
    const DV &v = L->d[0].v;
    // (nx_global == nx with i0 == 0 describes the whole width too: suhmo_hier_create takes a base written that way)
    const bool whole_x = L->desc.nx_global == 0 || (L->desc.i0 == 0 && L->desc.nx_global == L->desc.nx);
    return !L->stub && !on_strip(L) && !v.ext[0] && !v.ext[1] && whole_x;
}
// the body and CopyGhostCells of ZB and MASK on level l of a hierarchy
int hier_level_init(suhmo_hier *H, int l, const IbcRow &row, hipStream_t st)
{
    int rc;
    for (int f : init_fields) if ((rc = ensure_field(H, l, f))) return rc;
    if (l == 0) {
        suhmo_level *B = base_of(H);
        if ((rc = launch_over(k_ibc_init<OnLevel, IbcRow>, on_level(B, 0), GHOSTED, st, row)) || (rc = suhmo_copy_ghosts(B, 0, SUHMO_F_ZB, st))
            || (rc = suhmo_copy_ghosts(B, 0, SUHMO_F_MASK, st))) return rc;
    } else {
        suhmo_multi m;
        if ((rc = multi_of(H, l, st, m)) || (rc = launch_over(k_ibc_init<OnBoxes, IbcRow>, m.on(), GHOSTED, st, row))
            || (rc = launch_coef_ghosts(m.on(), SUHMO_F_ZB, st)) || (rc = launch_coef_ghosts(m.on(), SUHMO_F_MASK, st))) return rc;
    }
    H->n_ibc_launches++;
    for (suhmo_level *L : H->lev[l].box) level_written(L, true);
    return 0;
}
// pwl fill from level l - 1, exchange with corners, then the domain-ghost rule of the field
int hier_field_ghosts(suhmo_hier *H, int l, int f, hipStream_t st)
{
    int rc;
    if ((rc = hier_pwl(H, l, f, f, st)) || (rc = hier_ff(H, l, f, -1, true, st))) return rc;
    suhmo_multi m;
    if ((rc = multi_of(H, l, st, m))) return rc;
    return f == SUHMO_F_ZB || f == SUHMO_F_MASK ? launch_coef_ghosts(m.on(), f, st) : launch_extrap_ghosts(m.on(), f, st);
}
int hier_refused(const suhmo_hier *H, const char *who)
{
    if (H->world > 1 || H->part || H->shadowed) {
        suhmo_set_error("%s: a hierarchy on rank strips, with levels dealt to the ranks or read through the shadow of level 0 is not built", who);
        return -5;
    }
    return 0;
}
}  // namespace

int suhmo_ibc_check_(const suhmo_ibc_t *ibc, const char *who)
{
    if (!ibc) { suhmo_set_error("%s: no suhmo_ibc_t given", who); return -1; }
    if (ibc->kind < SUHMO_IBC_BASIC || ibc->kind > SUHMO_IBC_DINO) { suhmo_set_error("%s: unknown kind %d (SUHMO_IBC_BASIC .. SUHMO_IBC_DINO)", who, ibc->kind); return -1; }
    if (!(ibc->gap_init > 0.0)) { suhmo_set_error("%s: gap_init = %g (must be positive)", who, ibc->gap_init); return -1; }
    return 0;
}
int launch_ibc_init(const OnMembers &t, const IbcRow *rows, hipStream_t st, int *launched)
{
    int rc;
    *launched = 0;
    if ((rc = launch_over(k_ibc_init<OnMembers, const IbcRow *>, t, GHOSTED, st, rows))) return rc;
    ++*launched;
    if ((rc = launch_coef_ghosts(t, SUHMO_F_ZB, st))) return rc;
    ++*launched;
    if ((rc = launch_coef_ghosts(t, SUHMO_F_MASK, st))) return rc;
    ++*launched;
    return 0;
}

extern "C" int suhmo_level_ibc_init(suhmo_level_t *L, const suhmo_ibc_t *ibc, suhmo_stream_t s)
{
    if (!L) { suhmo_set_error("suhmo_level_ibc_init: no level"); return -1; }
    int rc = suhmo_ibc_check_(ibc, "suhmo_level_ibc_init"); if (rc) return rc;
    if (!whole_level(L)) { suhmo_set_error("suhmo_level_ibc_init: a rank strip, a patch of a nested hierarchy or a box of a hierarchy: not built (a hierarchy: suhmo_hier_ibc_init)"); return -5; }
    HIPCHK(hipSetDevice(L->device));
    if ((rc = level_fields(L, init_fields, (int)(sizeof(init_fields) / sizeof(int))))) return rc;
    hipStream_t st = (hipStream_t)s;
    const OnLevel t = on_level(L, 0);
    if ((rc = launch_over(k_ibc_init<OnLevel, IbcRow>, t, GHOSTED, st, ibc_row(*ibc)))) return rc;
    level_written(L, true);
    if ((rc = suhmo_copy_ghosts(L, 0, SUHMO_F_ZB, st)) || (rc = suhmo_copy_ghosts(L, 0, SUHMO_F_MASK, st))) return rc;
    return 0;
}

extern "C" int suhmo_hier_ibc_init(suhmo_hier_t *H, const suhmo_ibc_t *ibc, suhmo_stream_t s)
{
    if (!H) { suhmo_set_error("suhmo_hier_ibc_init: no hierarchy"); return -1; }
    int rc = suhmo_ibc_check_(ibc, "suhmo_hier_ibc_init"); if (rc) return rc;
    if ((rc = hier_refused(H, "suhmo_hier_ibc_init")) || (rc = suhmo_hier_check_(H))) return rc;
    HIPCHK(hipSetDevice(H->device));
    hipStream_t st = HST(s);
    const IbcRow row = ibc_row(*ibc);
    for (int l = 0; l < H->nlev; l++) if ((rc = hier_level_init(H, l, row, st))) return rc;
    for (int l = 1; l < H->nlev; l++) if ((rc = hier_field_ghosts(H, l, SUHMO_F_MASK, st))) return rc;
    suhmo_hier_invalidate_(H);
    return 0;
}

extern "C" int suhmo_hier_set_ibc(suhmo_hier_t *H, const suhmo_ibc_t *ibc)
{
    if (!H) { suhmo_set_error("suhmo_hier_set_ibc: no hierarchy"); return -1; }
    if (!ibc) { H->has_ibc = false; return 0; }
    int rc = suhmo_ibc_check_(ibc, "suhmo_hier_set_ibc"); if (rc) return rc;
    H->ibc = *ibc; H->has_ibc = true;
    return 0;
}

int suhmo_hier_ibc_reload_(suhmo_hier *H, int l, hipStream_t st)
{
    int rc;
    const int kind = H->ibc.kind;
    static const int order[] = {SUHMO_F_ZB, SUHMO_F_PI, SUHMO_F_ZS};
    for (int f : order) if (ibc_reload_writes(kind, f) && ((rc = ensure_field(H, l, f)) || (rc = ensure_field(H, l - 1, f)))) return rc;
    if ((rc = ensure_field(H, l, SUHMO_F_PI)) || (rc = ensure_field(H, l, SUHMO_F_MASK)) || (rc = ensure_field(H, l - 1, SUHMO_F_MASK))) return rc;
    if (kind == SUHMO_IBC_DINO && (rc = ensure_field(H, l, SUHMO_F_B))) return rc;
    suhmo_multi m;
    // (1) the bed / Pi body
    if ((rc = multi_of(H, l, st, m)) || (rc = launch_over(k_ibc_reload<OnBoxes, IbcRow>, m.on(), GHOSTED, st, ibc_row(H->ibc)))) return rc;
    H->n_ibc_launches++;
    // (2) the ghost cells of what it wrote
    for (int f : order) if (ibc_reload_writes(kind, f) && (rc = hier_field_ghosts(H, l, f, st))) return rc;
    // (3) setup_iceMask, (4) its ghost cells
    if ((rc = multi_of(H, l, st, m)) || (rc = launch_over(k_ibc_mask<OnBoxes>, m.on(), GHOSTED, st))) return rc;
    H->n_ibc_launches++;
    if ((rc = hier_field_ghosts(H, l, SUHMO_F_MASK, st))) return rc;
    for (suhmo_level *L : H->lev[l].box) level_written(L, false);
    return 0;
}
extern "C" int suhmo_hier_ibc_reload(suhmo_hier_t *H, int level, suhmo_stream_t s)
{
    if (!H) { suhmo_set_error("suhmo_hier_ibc_reload: no hierarchy"); return -1; }
    if (!H->has_ibc) { suhmo_set_error("suhmo_hier_ibc_reload: no IBC on the handle (suhmo_hier_set_ibc)"); return -1; }
    if (level < 1 || level >= H->nlev) { suhmo_set_error("suhmo_hier_ibc_reload: level %d (1 .. %d: level 0 is never reloaded)", level, H->nlev - 1); return -1; }
    int rc;
    if ((rc = hier_refused(H, "suhmo_hier_ibc_reload")) || (rc = suhmo_hier_check_(H))) return rc;
    HIPCHK(hipSetDevice(H->device));
    if ((rc = suhmo_hier_ibc_reload_(H, level, HST(s)))) return rc;
    suhmo_hier_invalidate_(H);
    return 0;
}
