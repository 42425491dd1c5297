// suhmo_balance.hip -- the mass balance of a level, of every level of a hierarchy, of the members of an ensemble, reduced on the device:
// AmrHydro::check_fluxes (src/AmrHydro.cpp:440-590), the third part of the post_proc block that ends every timeStepFAS (:3643-3652) -- the
// discharge through the four domain sides, through the ice margin and the ice-bearing domain sides, and the water volume.  The rule and the
// refusals: include/suhmo_hip.h, "MASS BALANCE"; the per-face and per-cell arithmetic: suhmo_balance.h; the order of the sums: suhmo_reduce.h;
// tests/massbalance_ref.py is the numpy twin of all three.  Read-only.
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

// the second stage of suhmo_reduce.h (k_norm_final's walk over ONE list) for workgroup b: list b of pl -> out[b] (the levels of a hierarchy), or,
// where sel.n > 0, the np partials of member sel.m[b] behind pl.p[0] -> out[that member]
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
#pragma unroll
    for (int q = 0; q < NV; q++) a[q] = Red::init(q);
    for (int e = tid; e < n; e += 256) {
#pragma unroll
        for (int q = 0; q < NV; q++) a[q] = red_op<Red>(q, a[q], p[NV * e + q]);
    }
    block_tree<Red>(tid, a);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < NV; q++) out[(size_t)NV * k + q] = a[q];
    }
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
