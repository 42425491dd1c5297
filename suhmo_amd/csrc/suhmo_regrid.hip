// suhmo_regrid.hip -- the third step of AmrHydro::regrid (src/AmrHydro.cpp:4227-4511): a hierarchy's fields moved onto regenerated box lists
// (destructiveRegrid, :4176-4223) without leaving HBM.  The rule is stated in include/suhmo_hip.h, "REGRID: FIELD TRANSFER"; tests/regrid_ref.py
// is its numpy twin.
//
// Per new level l = 1, 2, ..., ascending (level l reads the NEW level l-1, all its steps done), for every listed field:
//   (a) k_regrid_interp   every valid cell of every new box <- FineInterp::interpToFine of level l-1, over the plan "new box x coarse box"
//   (b) hier_pwl          coarse-fine ghost cells <- PiecewiseLinearFillPatch of level l-1
//   (c) k_regrid_copy     valid cells an old box of level l holds <- the old values, over the plan "old box x new box" (after (a): the copy wins)
//   (d) hier_ff           exchange between the new boxes, corners included
//   (e) domain ghost cells across a non-periodic side: CopyGhostCells / ExtrapGhostCells, the launches the time step uses
// With an IBC on the old handle (suhmo_hier_set_ibc) the level is then reloaded -- initializeBed / initializePi / setup_iceMask and their ghost fills,
// suhmo_ibc.hip -- before level l + 1 reads it (:4387-4437 sit inside the reference's loop over the levels).
// The two plans are lists of RECTANGLES (a few dozen bytes per pair of boxes that intersect), built on the host from the two box lists, uploaded, used
// once and freed.  A coarse neighbour that sits in another box of level l-1 or across a periodic side is read from the coarse box's own ghost
// ring, which step (d) of level l-1 has just made current with corners; level 0 is one canvas, where the wrapped neighbour is addressed directly.
#include "suhmo_hier_int.h"
#include "suhmo_transfer.h"
#include "suhmo_ibc.h"

using namespace hier;
namespace {
constexpr int RG_MAXF = 16;                                // fields per launch
struct RgFields { int n; int f[RG_MAXF]; };
// w x h coarse cells (I0 + I, J0 + J) of coarse box cb at canvas offset coff -> the 2w x 2h fine cells of new box fb at foff
struct RgInterp { int fb, cb, foff, coff, w, h, I0, J0; };
// w x h fine cells of old box sb at soff -> new box db at doff
struct RgCopy { int db, sb, doff, soff, w, h; };

// FineInterp::interpToFine, ratio 2 (suhmo_transfer.h: limited_slopes with tangential_only, child_value).  One thread = one coarse cell and its
// four children.
__global__ __launch_bounds__(256) void k_regrid_interp(const RgInterp *__restrict__ e, const FP *__restrict__ ftab, const DV *__restrict__ fdv,
                                                       const FP *__restrict__ ctab, const DV *__restrict__ cdv, FP cbase, DV cbdv, int use_base,
                                                       int nxd, int nyd, int perx, int pery, RgFields fl)
{
    const RgInterp q = e[blockIdx.z];
    const int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= q.w || J >= q.h) return;
    const int Ig = q.I0 + I, Jg = q.J0 + J;
    const int Pc = use_base ? cbdv.P : cdv[q.cb].P, Pf = fdv[q.fb].P;
    // which neighbours exist: inside the coarse domain after the wrap through a periodic side
    const bool xl = perx || Ig - 1 >= 0, xh = perx || Ig + 1 <= nxd - 1, yl = pery || Jg - 1 >= 0, yh = pery || Jg + 1 <= nyd - 1;
    // where they are: one cell away in the box's canvas (its ghost ring holds the cells of other boxes and periodic images); on level 0 the
    // wrapped cell itself
    int ox[3] = {-1, 0, 1}, oy[3] = {-Pc, 0, Pc};
    if (use_base) {
        if (Ig - 1 < 0) ox[0] = nxd - 1;
        if (Ig + 1 > nxd - 1) ox[2] = -(nxd - 1);
        if (Jg - 1 < 0) oy[0] = (nyd - 1) * Pc;
        if (Jg + 1 > nyd - 1) oy[2] = -(nyd - 1) * Pc;
    }
    const bool ex[3] = {xl, true, xh}, ey[3] = {yl, true, yh};
    const int c = q.coff + J * Pc + I, f0 = q.foff + 2 * J * Pf + 2 * I;
    for (int t = 0; t < fl.n; t++) {
        const double *__restrict__ C = use_base ? cbase.f[fl.f[t]] : ctab[q.cb].f[fl.f[t]];
        double nb[3][3], s0, s1;
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int a = 0; a < 3; a++) nb[b][a] = (ex[a] && ey[b]) ? C[c + oy[b] + ox[a]] : 0.0;
        limited_slopes(nb, xl, xh, yl, yh, true, s0, s1);
        const double c0 = nb[1][1];
        double *__restrict__ F = ftab[q.fb].f[fl.f[t]];
        // fine cells (2I + p, 2J + q), a row per store (canvas offsets of even fine columns are even: 16-byte aligned)
        *reinterpret_cast<double2 *>(F + f0) = make_double2(child_value(c0, s0, s1, -0.25, -0.25), child_value(c0, s0, s1, 0.25, -0.25));
        *reinterpret_cast<double2 *>(F + f0 + Pf) = make_double2(child_value(c0, s0, s1, -0.25, 0.25), child_value(c0, s0, s1, 0.25, 0.25));
    }
}
// a_oldData->copyTo(*newData): valid cells only
__global__ __launch_bounds__(256) void k_regrid_copy(const RgCopy *__restrict__ e, const FP *__restrict__ dtab, const DV *__restrict__ ddv,
                                                     const FP *__restrict__ stab, const DV *__restrict__ sdv, RgFields fl)
{
    const RgCopy q = e[blockIdx.z];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= q.w || j >= q.h) return;
    const int d = q.doff + j * ddv[q.db].P + i, s = q.soff + j * sdv[q.sb].P + i;
    for (int t = 0; t < fl.n; t++) dtab[q.db].f[fl.f[t]][d] = stab[q.sb].f[fl.f[t]][s];
}

// the boxes of level V that intersect the rectangle (i0, j0) .. (i1, j1), each once: emit(box, a0, c0, a1, c1)
template <class E> void intersecting(const HLev &V, int i0, int j0, int i1, int j1, E &&emit)
{
    const BoxIndex &X = V.index;
    for (int by = j0 / X.bs; by <= j1 / X.bs; by++)
        for (int bx = i0 / X.bs; bx <= i1 / X.bs; bx++) {
            const size_t q = (size_t)by * X.nbx + bx;
            for (int p = X.start[q]; p < X.start[q + 1]; p++) {
                const int o = X.items[p];
                const int *b = &V.b4[4 * o];
                const int a0 = std::max(i0, b[0]), a1 = std::min(i1, b[2]), c0 = std::max(j0, b[1]), c1 = std::min(j1, b[3]);
                if (a0 > a1 || c0 > c1) continue;
                if (a0 / X.bs != bx || c0 / X.bs != by) continue;            // only from the bucket that holds the corner of the intersection
                emit(o, a0, c0, a1, c1);
            }
        }
}
// the reference's list (src/AmrHydro.cpp:4363-4376) restricted to what is held as arrays here
const int default_fields[] = {SUHMO_F_PHI, SUHMO_F_B, SUHMO_F_PI, SUHMO_F_ZB, SUHMO_F_MASK, SUHMO_F_MR, SUHMO_F_PW, SUHMO_F_ZS};
bool cell_field(int f)
{
    switch (f) {
    case SUHMO_F_BX: case SUHMO_F_BY: case SUHMO_F_QWX: case SUHMO_F_QWY: case SUHMO_F_DCX: case SUHMO_F_DCY: case SUHMO_F_COVER: case SUHMO_F_PHI2: return false;
    default: return f >= 0 && f < SUHMO_F_COUNT;
    }
}

// the fields of level l of N from level l-1 of N and level l of O
int transfer_level(suhmo_hier *O, suhmo_hier *N, int l, const RgFields &fl, hipStream_t st)
{
    int rc;
    HLev &F = N->lev[l], &C = N->lev[l - 1];
    for (int t = 0; t < fl.n; t++) {
        if ((rc = ensure_field(N, l, fl.f[t]))) return rc;
        if (l - 1 == 0) { if (!suhmo_field(base_of(N), 0, fl.f[t])) { suhmo_set_error("field allocation failed"); return -2; } }
        else if ((rc = ensure_field(N, l - 1, fl.f[t]))) return rc;
        if (l < O->nlev && (rc = ensure_field(O, l, fl.f[t]))) return rc;
    }
    // ---- the two plans
    std::vector<RgInterp> pi; std::vector<RgCopy> pc;
    int iw = 0, ih = 0, cw = 0, ch = 0;
    for (int k = 0; k < (int)F.box.size(); k++) {
        const int *b = &F.b4[4 * k];
        const DV &v = F.box[k]->d[0].v;
        auto piece = [&](int o, int a0, int c0, int a1, int c1) {
            const DV &vc = C.box[o]->d[0].v;
            pi.push_back(RgInterp{k, o, cidx(v, 2 * a0 - b[0], 2 * c0 - b[1]), cidx(vc, a0 - vc.i0, c0 - vc.j0), a1 - a0 + 1, c1 - c0 + 1, a0, c0});
            iw = std::max(iw, a1 - a0 + 1); ih = std::max(ih, c1 - c0 + 1);
        };
        if (C.l == 0) piece(0, b[0] / 2, b[1] / 2, b[2] / 2, b[3] / 2);
        else intersecting(C, b[0] / 2, b[1] / 2, b[2] / 2, b[3] / 2, piece);
        if (l < O->nlev)
            intersecting(O->lev[l], b[0], b[1], b[2], b[3], [&](int o, int a0, int c0, int a1, int c1) {
                const DV &vo = O->lev[l].box[o]->d[0].v;
                pc.push_back(RgCopy{k, o, cidx(v, a0 - b[0], c0 - b[1]), cidx(vo, a0 - vo.i0, c0 - vo.j0), a1 - a0 + 1, c1 - c0 + 1});
                cw = std::max(cw, a1 - a0 + 1); ch = std::max(ch, c1 - c0 + 1);
            });
    }
    {   // (proper nesting, which suhmo_hier_create has checked, makes the pieces cover every new box)
        long cells = 0, want = 0;
        for (const RgInterp &q : pi) cells += (long)q.w * q.h;
        for (size_t k = 0; k < F.box.size(); k++) { const int *b = &F.b4[4 * k]; want += (long)(b[2] / 2 - b[0] / 2 + 1) * (b[3] / 2 - b[1] / 2 + 1); }
        if (cells != want) { suhmo_set_error("regrid: internal: the interpolation pieces of level %d do not cover its boxes", l); return -4; }
    }
    DevVec<RgInterp> di; DevVec<RgCopy> dc;
    if (di.upload(pi) || dc.upload(pc)) { di.release(); dc.release(); suhmo_set_error("regrid: plan upload failed"); return -2; }
    auto run = [&]() -> int {
        int rc;
        // (a)
        if ((rc = refresh_tables(N, l, st)) || (rc = refresh_tables(N, l - 1, st))) return rc;
        const suhmo_level *B = base_of(N);
        const bool ub = l - 1 == 0;
        hipLaunchKernelGGL(k_regrid_interp, dim3((iw + 63) / 64, (ih + 3) / 4, (unsigned)di.n), dim3(64, 4), 0, st, di.d, F.d_fp, F.d_dv,
                           ub ? nullptr : C.d_fp, ub ? nullptr : C.d_dv, ub ? B->d[0].fp : FP{}, ub ? B->d[0].v : DV{}, ub ? 1 : 0,
                           C.nxd, C.nyd, (int)N->bc.periodic[0], (int)N->bc.periodic[1], fl);
        HIPCHK(hipGetLastError());
        // (b)
        for (int t = 0; t < fl.n; t++) if ((rc = hier_pwl(N, l, fl.f[t], fl.f[t], st))) return rc;
        // (c)
        if (dc.n) {
            if ((rc = refresh_tables(O, l, st)) || (rc = refresh_tables(N, l, st))) return rc;
            hipLaunchKernelGGL(k_regrid_copy, dim3((cw + 63) / 64, (ch + 3) / 4, (unsigned)dc.n), dim3(64, 4), 0, st, dc.d, F.d_fp, F.d_dv,
                               O->lev[l].d_fp, O->lev[l].d_dv, fl);
            HIPCHK(hipGetLastError());
        }
        // (d)
        for (int t = 0; t < fl.n; t += 2) if ((rc = hier_ff(N, l, fl.f[t], t + 1 < fl.n ? fl.f[t + 1] : -1, true, st))) return rc;
        // (e) what the reference's regrid does to the field (src/AmrHydro.cpp:4379-4383, 4419-4421, 4436); B: the time step's own ghost fill
        suhmo_multi m;
        if ((rc = multi_of(N, l, st, m))) return rc;
        for (int t = 0; t < fl.n; t++) {
            const int f = fl.f[t];
            if (f == SUHMO_F_ZB || f == SUHMO_F_MASK || f == SUHMO_F_B) rc = launch_coef_ghosts(m.on(), f, st);
            else if (f == SUHMO_F_PI || f == SUHMO_F_ZS || f == SUHMO_F_MR || f == SUHMO_F_PW) rc = launch_extrap_ghosts(m.on(), f, st);
            if (rc) return rc;
            if (f == SUHMO_F_MASK) for (suhmo_level *L : F.box) suhmo_mask_written(L);
            if (f == SUHMO_F_ZB) for (suhmo_level *L : F.box) suhmo_zb_written(L);
        }
        return 0;
    };
    rc = run();
    // the plans are read by launches in flight: they go once the stream has drained
    if (hipStreamSynchronize(st) != hipSuccess && !rc) { suhmo_set_error("regrid: the transfer launches of level %d failed", l); rc = -2; }
    di.release(); dc.release();
    return rc;
}
}  // namespace

extern "C" int suhmo_hier_regrid(suhmo_hier_t *O, int nlev, const int *nbox, const int *boxes, int nfields, const int *fields, suhmo_hier_t **out,
                                 suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::regrid(field transfer)");
    if (out) *out = nullptr;
    ARG(O && out && nlev >= 1 && nlev <= 8 && (fields == nullptr || (nfields >= 0 && nfields <= RG_MAXF)));
    if (O->world > 1 || O->part || O->shadowed) { suhmo_set_error("regrid: a hierarchy on rank strips (or read through the shadow of level 0) is not built"); return -5; }
    RgFields fl{};
    if (!fields) { fl.n = (int)(sizeof(default_fields) / sizeof(int)); for (int t = 0; t < fl.n; t++) fl.f[t] = default_fields[t]; }
    else
        for (int t = 0; t < nfields; t++) {
            if (!cell_field(fields[t])) { suhmo_set_error("regrid: field %d is not a cell field that can be transferred", fields[t]); return -1; }
            bool seen = false;
            for (int u = 0; u < fl.n; u++) seen = seen || fl.f[u] == fields[t];
            if (!seen) fl.f[fl.n++] = fields[t];
        }
    int rc = suhmo_hier_check_(O); if (rc) return rc;
    HIPCHK(hipSetDevice(O->device));
    HIPCHK(hipStreamSynchronize(HST(s)));
    suhmo_level *B = base_of(O);
    suhmo_hier *N = nullptr;
    const std::string opts = suhmo_hier_options_(O);
    {   SUHMO_TIME("regrid: hierarchy creation (boxes, plans, tables)");
        rc = suhmo_hier_create_on_(&N, &O->base_desc, B, nlev, nbox, boxes, opts.c_str()); }
    if (!rc) {
        SUHMO_TIME("regrid: transfer plans and launches");
        N->ag = O->ag; N->ag_user = O->ag_user;
        N->has_ibc = O->has_ibc; N->ibc = O->ibc; N->n_ibc_launches = O->n_ibc_launches;
        for (int l = 1; l < N->nlev && !rc; l++) {
            if (fl.n) rc = transfer_level(O, N, l, fl, HST(s));
            // initializeBed / initializePi / setup_iceMask of the new level (src/AmrHydro.cpp:4387-4437), before level l + 1 interpolates from it
            if (!rc && N->has_ibc) rc = suhmo_hier_ibc_reload_(N, l, HST(s));
        }
    }
    if (rc) {
        // the old hierarchy stays as it was.  The one thing creation writes into the base level is SUHMO_F_COVER (geometry): marked again for the old boxes
        if (N) (void)suhmo_hier_destroy(N);
        std::string msg = suhmo_last_error();
        if (suhmo_level_set_value(B, 0, SUHMO_F_COVER, 0.0, nullptr) == 0 && O->nlev > 1) (void)hier_avg(O, 1, SUHMO_F_COVER, SUHMO_F_COVER, 1, 1.0, nullptr);
        (void)hipDeviceSynchronize();
        suhmo_set_error("%s", msg.c_str());
        return rc;
    }
    // the base level changes hands: nothing the old hierarchy knew about it survives -- its gap-height hierarchy, tag maps, plans and tables go
    // with it, the base level forgets what it knew about its ice mask and its captured V-cycles
    suhmo_mask_written(B); suhmo_zb_written(B);
    suhmo_level_drop_graphs(B);
    B->resout_req = 0; B->resout_rhs = nullptr; B->resout_done = 0;
    N->base_borrowed = false;
    O->base_borrowed = true;
    {   SUHMO_TIME("regrid: old hierarchy destroyed");
        (void)suhmo_hier_destroy(O); }
    suhmo_hier_invalidate_(N);
    *out = N;
    return 0;
}
