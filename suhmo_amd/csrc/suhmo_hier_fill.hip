// suhmo_hier_fill.hip -- the plans of a hierarchy of box unions executed (suhmo_hier_int.h): their kernels and launchers, the device tables,
// the shadow of a level 0 cut into rank strips, the exchange of packed cells between the owners of a partitioned level's boxes
#include "suhmo_hier_int.h"
#include "suhmo_transfer.h"

using namespace hier;
namespace {
// ------------------------------------------------------------------ kernels over the plans
__device__ __forceinline__ double *fptr(const FP *tab, const FP &base, int use_base, int b, int field)
{
    return use_base ? base.f[field] : tab[b].f[field];
}
__device__ __forceinline__ void d_ff(const CopyEnt &c, const FP *__restrict__ tab, int f0, int f1)
{
    tab[c.d.b].f[f0][c.d.off] = tab[c.s.b].f[f0][c.s.off];
    if (f1 >= 0) tab[c.d.b].f[f1][c.d.off] = tab[c.s.b].f[f1][c.s.off];
}
__global__ void k_ff(const CopyEnt *__restrict__ e, int n, const FP *__restrict__ tab, int f0, int f1)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    d_ff(e[t], tab, f0, f1);
}
// QuadCFInterp (suhmo_transfer.h: cf_tangential, cf_ghost): q.kind is cf_tangential's, q.c[] its stencil cells in its order
__device__ __forceinline__ void d_cf(const CfEnt &q, const FP *__restrict__ ftab, int ff0, const FP *__restrict__ ctab, const FP &cbase,
                                     int use_base, int fc0, int ff1, int fc1)
{
    const double xt = q.xsign ? 0.25 : -0.25;
    const bool two = q.kind != CF_NONE, three = q.kind == CF_CENTRED || q.kind == CF_HI2 || q.kind == CF_LO2;   // cells the stencil has
  for (int pass = 0; pass < (ff1 >= 0 ? 2 : 1); pass++) {          // one or two fields over the same stencils (the two gradient components)
    const int ff = pass ? ff1 : ff0, fc = pass ? fc1 : fc0;
#define CVAL(m) fptr(ctab, cbase, use_base, q.c[m].b, fc)[q.c[m].off]
    const double a = CVAL(0), b = two ? CVAL(1) : 0.0, c = three ? CVAL(2) : 0.0;
#undef CVAL
    double d1, d2;
    const double c0 = cf_tangential(q.kind, a, b, c, d1, d2);
    double *f = ftab[q.f.b].f[ff];
    f[q.f.off] = cf_ghost(c0, d1, d2, xt, f[q.f.off + q.step], f[q.f.off + 2 * q.step]);
  }
}
__global__ void k_cf(const CfEnt *__restrict__ e, int n, const FP *__restrict__ ftab, int ff0, const FP *__restrict__ ctab, FP cbase,
                     int use_base, int fc0, int ff1, int fc1)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    d_cf(e[t], ftab, ff0, ctab, cbase, use_base, fc0, ff1, fc1);
}
// both kinds of ghost cell of one or two fields of a level in ONE launch: the coarse-fine ghosts are interpolated from the level below and two
// VALID cells of their own box, the fine-fine ghosts are copies of VALID cells of the neighbouring boxes -- neither reads what the other
// writes (workgroups [0, nbcf): the cf plan, the rest: the ff plan)
__global__ void k_cf_ff(const CfEnt *__restrict__ ce, int ncf, int nbcf, const CopyEnt *__restrict__ fe, int nff, const FP *__restrict__ ftab, int ff0,
                        const FP *__restrict__ ctab, FP cbase, int use_base, int fc0, int ff1, int fc1)
{
    if ((int)blockIdx.x < nbcf) {
        int t = blockIdx.x * blockDim.x + threadIdx.x;
        if (t < ncf) d_cf(ce[t], ftab, ff0, ctab, cbase, use_base, fc0, ff1, fc1);
    } else {
        int t = (blockIdx.x - nbcf) * blockDim.x + threadIdx.x;
        if (t < nff) d_ff(fe[t], ftab, ff0, ff1);
    }
}
// ... of the head of SEVERAL levels (their ghosts depend on valid cells only, of the level itself and of the one below: no order among them).
// By value, indexed with constants only (unrolled search), so that the tables stay in scalar registers.
struct LvGhosts { const CfEnt *cf[SUHMO_LVMAX]; const CopyEnt *ff[SUHMO_LVMAX]; const FP *ftab[SUHMO_LVMAX], *ctab[SUHMO_LVMAX];
                  int ncf[SUHMO_LVMAX], nbcf[SUHMO_LVMAX], nff[SUHMO_LVMAX], nb[SUHMO_LVMAX], use_base[SUHMO_LVMAX]; int n; };
__global__ void k_cf_ff_lv(LvGhosts lv, FP cbase, int field)
{
    int b = blockIdx.x, q = -1;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t < lv.n && q < 0) { if (b < lv.nb[t]) q = t; else b -= lv.nb[t]; }
    if (q < 0) return;
    const CfEnt *ce = nullptr; const CopyEnt *fe = nullptr; const FP *ftab = nullptr, *ctab = nullptr; int ncf = 0, nbcf = 0, nff = 0, use_base = 0;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t == q) { ce = lv.cf[t]; fe = lv.ff[t]; ftab = lv.ftab[t]; ctab = lv.ctab[t]; ncf = lv.ncf[t]; nbcf = lv.nbcf[t]; nff = lv.nff[t]; use_base = lv.use_base[t]; }
    if (b < nbcf) {
        int t = b * blockDim.x + threadIdx.x;
        if (t < ncf) d_cf(ce[t], ftab, field, ctab, cbase, use_base, field, -1, -1);
    } else {
        int t = (b - nbcf) * blockDim.x + threadIdx.x;
        if (t < nff) d_ff(fe[t], ftab, field, -1);
    }
}
// PiecewiseLinearFillPatch (suhmo_transfer.h: limited_slopes, child_value).  A neighbour the plan marks b < 0 lies outside the domain; q.sx / q.sy
// say the same of the middle row and column (0: both neighbours, 1: none below, 2: none above)
__global__ void k_pwl(const PwlEnt *__restrict__ e, int n, const FP *__restrict__ ftab, int ff, const FP *__restrict__ ctab, FP cbase,
                      int use_base, int fc)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    PwlEnt q = e[t];
#define CVAL(m) fptr(ctab, cbase, use_base, q.c[m].b, fc)[q.c[m].off]
    double nb[3][3], s0, s1;
#pragma unroll
    for (int m = 0; m < 9; m++) nb[m / 3][m % 3] = q.c[m].b < 0 ? 0.0 : CVAL(m);
#undef CVAL
    limited_slopes(nb, q.sx != 1, q.sx != 2, q.sy != 1, q.sy != 2, false, s0, s1);
    ftab[q.f.b].f[ff][q.f.off] = child_value(nb[1][1], s0, s1, (q.par & 1) ? 0.25 : -0.25, (q.par & 2) ? 0.25 : -0.25);
}
// FORT_AVERAGE (mode 0; suhmo_transfer.h: avg4) / covered cells <- val (mode 1)
__device__ __forceinline__ void d_avg(const RectEnt &q, int I, int J, const FP *__restrict__ ftab, const DV *__restrict__ fdv, int ff,
                                      const FP *__restrict__ ctab, const DV *__restrict__ cdv, const FP &cbase, const DV &cbdv, int use_base, int fc, int mode, double val)
{
    if (I >= q.w || J >= q.h) return;
    const int Pc = use_base ? cbdv.P : cdv[q.cb].P;
    double *c = fptr(ctab, cbase, use_base, q.cb, fc);
    if (mode == 1) { c[q.coff + J * Pc + I] = val; return; }
    const int Pf = fdv[q.fb].P;
    const double *f = ftab[q.fb].f[ff];
    int b = q.foff + 2 * J * Pf + 2 * I;
    c[q.coff + J * Pc + I] = avg4(f[b], f[b + 1], f[b + Pf], f[b + Pf + 1]);
}
__global__ void k_avg(const RectEnt *__restrict__ e, const FP *__restrict__ ftab, const DV *__restrict__ fdv, int ff,
                      const FP *__restrict__ ctab, const DV *__restrict__ cdv, FP cbase, DV cbdv, int use_base, int fc, int mode, double val)
{
    d_avg(e[blockIdx.z], blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * blockDim.y + threadIdx.y, ftab, fdv, ff, ctab, cdv, cbase, cbdv, use_base, fc, mode, val);
}
// owner computes: the same averages into this rank's segment of an all-gather (q.coff = position, pitch = q.w) ...
__global__ void k_avg_put(const RectEnt *__restrict__ e, const FP *__restrict__ ftab, const DV *__restrict__ fdv, int ff, double *__restrict__ buf)
{
    RectEnt q = e[blockIdx.z];
    int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= q.w || J >= q.h) return;
    const int Pf = fdv[q.fb].P;
    const double *f = ftab[q.fb].f[ff];
    int b = q.foff + 2 * J * Pf + 2 * I;
    buf[q.coff + (long)J * q.w + I] = avg4(f[b], f[b + 1], f[b + Pf], f[b + Pf + 1]);
}
// ... and the holder of the coarse cells takes its rectangles out of the writers' segments
__global__ void k_put_unpack(const PutEnt *__restrict__ e, const FP *__restrict__ ctab, const DV *__restrict__ cdv, FP cbase, DV cbdv, int use_base, int fc,
                             const double *__restrict__ buf, long stride)
{
    PutEnt q = e[blockIdx.z];
    int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= q.w || J >= q.h) return;
    const int Pc = use_base ? cbdv.P : cdv[q.cb].P;
    double *c = fptr(ctab, cbase, use_base, q.cb, fc);
    c[q.coff + J * Pc + I] = buf[(long)q.rank * stride + q.pos + (long)J * q.w + I];
}
// old != NULL: the window gets c - old (the correction phi - phi_saved, as axby(phi, saved, 1, -1) states it), old being an earlier
// gather of the same cells
__global__ void k_win_gather(const WinEnt *__restrict__ e, double *__restrict__ wbuf, const FP *__restrict__ ctab, const DV *__restrict__ cdv,
                             FP cbase, DV cbdv, int use_base, int fc, const Win *__restrict__ wins, const int *__restrict__ went_box,
                             const double *__restrict__ old = nullptr)
{
    WinEnt q = e[blockIdx.z];
    int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= q.w || J >= q.h) return;
    const int Pc = use_base ? cbdv.P : cdv[q.cb].P;
    const double *c = fptr(ctab, cbase, use_base, q.cb, fc);
    const Win w = wins[went_box[blockIdx.z]];
    const size_t o = w.base + q.woff + (size_t)J * w.nx + I;
    const double cv = c[q.coff + J * Pc + I];
    wbuf[o] = old ? 1.0 * cv + -1.0 * old[o] : cv;
}
// physical BC of the coarse level on the window of every fine box (suhmo_transfer.h: bc_ghost), along the
// coarsened box's own extent only: the corner cells beyond it are never written (value 0)
__global__ void k_win_bc(const Win *__restrict__ wins, int nwin, double *__restrict__ wbuf, DV cv /* a view of level l-1: BC data, domain size */)
{
    int k = blockIdx.y;
    if (k >= nwin) return;
    const Win w = wins[k];
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int inx = w.nx - 2, iny = w.ny - 2;             // the coarsened box itself
    double *p = wbuf + w.base;
    int dir, side, tt;
    if (t < 2 * iny) { dir = 0; side = t / iny; tt = t % iny; }
    else { t -= 2 * iny; if (t >= 2 * inx) return; dir = 1; side = t / inx; tt = t % inx; }
    if (cv.per[dir]) return;
    const int ndom = dir == 0 ? cv.nxg : cv.nyg;
    const int g = dir == 0 ? (side ? w.i0 + w.nx - 1 : w.i0) : (side ? w.j0 + w.ny - 1 : w.j0);   // global index of the ghost layer
    if (g >= 0 && g <= ndom - 1) return;
    const int il = dir == 0 ? (side ? w.nx - 1 : 0) : tt + 1, jl = dir == 0 ? tt + 1 : (side ? w.ny - 1 : 0);
    const int in_ = dir == 0 ? (side ? w.nx - 2 : 1) : il, jn_ = dir == 0 ? jl : (side ? w.ny - 2 : 1);
    p[(size_t)jl * w.nx + il] = bc_ghost(cv.bct[dir][side], cv.two_v[dir][side], cv.neu[dir][side], p[(size_t)jn_ * w.nx + in_]);
}
// PROLONG_2_NL (suhmo_transfer.h: prolong2_nl) of every box of a level from its window
__global__ void k_prolong2_win(const Win *__restrict__ wins, const double *__restrict__ wbuf, const FP *__restrict__ ftab, const DV *__restrict__ fdv)
{
    const int k = blockIdx.z;
    const DV v = fdv[k];
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    const Win w = wins[k];
    const double *c = wbuf + w.base;
    int gi = i + v.i0, gj = j + v.j0;
    int ic = gi / 2, jc = gj / 2, o1 = 2 * (gi % 2) - 1, o2 = 2 * (gj % 2) - 1;
    int cc = (jc - w.j0) * w.nx + (ic - w.i0);
    double *phi = ftab[k].f[SUHMO_F_PHI];
    int idx = cidx(v, i, j);
    phi[idx] = prolong2_nl(phi[idx], c[cc], c[cc + o1], c[cc + o2 * w.nx], c[cc + o1 + o2 * w.nx]);
}
// AMRProlongS_2 of one box per workgroup: the three steps above (gather of the coarse correction into the box's window, physical BC on the
// window, PROLONG_2_NL) with the window in LDS instead of three launches over a buffer in HBM; the same expressions on the same operands.
// wstart[k] .. wstart[k + 1]: the gather pieces of box k.  old != NULL: the window gets c - old (see k_win_gather)
// fc_minus >= 0: the coarse field is 1 fc + (-1) fc_minus formed on the fly (the correction PHI - PHIOLD of a level of boxes leaving its FAS problem),
// and the workgroups from nk on ARE that leaving (k_fas_leave's RHS <- RHS0, CORR <- PHI - PHIOLD on the coarse level's boxes: they write
// neither PHI nor PHIOLD): one launch instead of two
__global__ __launch_bounds__(256) void k_prolong2_fused(const WinEnt *__restrict__ e, const int *__restrict__ wstart, const Win *__restrict__ wins, int k0,
                                                        const FP *__restrict__ ctab, const DV *__restrict__ cdv, FP cbase, DV cbdv, int use_base, int fc,
                                                        const double *__restrict__ old, const FP *__restrict__ ftab, const DV *__restrict__ fdv,
                                                        int fc_minus, int nk, int cgx, int cgy)
{
    extern __shared__ double win[];
    if (fc_minus >= 0 && (int)blockIdx.x >= nk) {
        const int b = blockIdx.x - nk, bx = b % cgx, by = (b / cgx) % cgy, bz = b / (cgx * cgy);
        const DV &v = cdv[bz];
        const FP &f = ctab[bz];
        const int i = bx * 64 + (int)(threadIdx.x & 63) - 1, j = by * 4 + (int)(threadIdx.x >> 6) - 1;
        if (i > v.nx || j > v.ny) return;
        const int idx = cidx(v, i, j);
        f.f[SUHMO_F_RHS][idx] = f.f[SUHMO_F_RHS0][idx];
        if (i >= 0 && i < v.nx && j >= 0 && j < v.ny) f.f[SUHMO_F_CORR][idx] = 1.0 * f.f[SUHMO_F_PHI][idx] + -1.0 * f.f[SUHMO_F_PHIOLD][idx];
        return;
    }
    const int k = k0 + blockIdx.x, tid = threadIdx.x;
    const Win w = wins[k];
    const int nw = w.nx * w.ny;
    for (int t = tid; t < nw; t += 256) win[t] = 0.0;                       // (cells no piece and no BC writes: the corners, value 0)
    __syncthreads();
    for (int p = wstart[k]; p < wstart[k + 1]; p++) {
        const WinEnt q = e[p];
        const int Pc = use_base ? cbdv.P : cdv[q.cb].P;
        const double *c = fptr(ctab, cbase, use_base, q.cb, fc);
        const double *cm = fc_minus >= 0 ? fptr(ctab, cbase, use_base, q.cb, fc_minus) : nullptr;
        for (int t = tid; t < q.w * q.h; t += 256) {
            const int J = t / q.w, I = t - J * q.w;
            const int o = q.woff + J * w.nx + I;
            double cv = c[q.coff + J * Pc + I];
            if (cm) cv = 1.0 * cv + -1.0 * cm[q.coff + J * Pc + I];
            win[o] = old ? 1.0 * cv + -1.0 * old[w.base + o] : cv;
        }
    }
    __syncthreads();
    {   // k_win_bc
        const int inx = w.nx - 2, iny = w.ny - 2;
        for (int t0 = tid; t0 < 2 * iny + 2 * inx; t0 += 256) {
            int t = t0, dir, side, tt;
            if (t < 2 * iny) { dir = 0; side = t / iny; tt = t % iny; }
            else { t -= 2 * iny; dir = 1; side = t / inx; tt = t % inx; }
            if (cbdv.per[dir]) continue;
            const int ndom = dir == 0 ? cbdv.nxg : cbdv.nyg;
            const int g = dir == 0 ? (side ? w.i0 + w.nx - 1 : w.i0) : (side ? w.j0 + w.ny - 1 : w.j0);
            if (g >= 0 && g <= ndom - 1) continue;
            const int il = dir == 0 ? (side ? w.nx - 1 : 0) : tt + 1, jl = dir == 0 ? tt + 1 : (side ? w.ny - 1 : 0);
            const int in_ = dir == 0 ? (side ? w.nx - 2 : 1) : il, jn_ = dir == 0 ? jl : (side ? w.ny - 2 : 1);
            win[jl * w.nx + il] = bc_ghost(cbdv.bct[dir][side], cbdv.two_v[dir][side], cbdv.neu[dir][side], win[jn_ * w.nx + in_]);
        }
    }
    __syncthreads();
    {   // k_prolong2_win
        const DV v = fdv[k];
        double *phi = ftab[k].f[SUHMO_F_PHI];
        for (int t = tid; t < v.nx * v.ny; t += 256) {
            const int j = t / v.nx, i = t - j * v.nx;
            const int gi = i + v.i0, gj = j + v.j0;
            const int ic = gi / 2, jc = gj / 2, o1 = 2 * (gi % 2) - 1, o2 = 2 * (gj % 2) - 1;
            const int cc = (jc - w.j0) * w.nx + (ic - w.i0);
            const int idx = cidx(v, i, j);
            phi[idx] = prolong2_nl(phi[idx], win[cc], win[cc + o1], win[cc + o2 * w.nx], win[cc + o1 + o2 * w.nx]);
        }
    }
}
// LevelFluxRegister (suhmo_transfer.h: reflux_*): one thread per coarse cell next to coarse-fine faces
__device__ __forceinline__ void d_reflux(const Target &T, const Face *__restrict__ faces, const FP *__restrict__ ftab, const DV *__restrict__ fdv,
                                         const FP *__restrict__ ctab, const FP &cbase, const FP &cdst, int use_base, int field_c, double dxc, double dyc, double beta, int residual)
{
    // cdst: the level itself; cbase: where its cells are read (the shadow of a cut level 0).  residual: the register is added to
    // LPHI's value and field_c <- rhs - that (the axby of the composite residual, for the cells the reflux reaches)
    double *lof = fptr(ctab, cdst, use_base, T.t.b, field_c);
    const double rscale = 1.0 / (dxc * dyc);
    double acc = residual ? fptr(ctab, cdst, use_base, T.t.b, SUHMO_F_LPHI)[T.t.off] : lof[T.t.off];
    for (int m = 0; m < T.count; m++) {
        Face f = faces[T.first + m];
        const double dxd = f.dir == 0 ? dxc : dyc, tsize = f.dir == 0 ? dyc : dxc;
        const double cs = beta * 1 / dxd, fs = beta * 2 / dxd;
        const double sign = f.side == 0 ? 1.0 : -1.0;
        double phihi = fptr(ctab, cbase, use_base, f.hi.b, SUHMO_F_PHI)[f.hi.off], philo = fptr(ctab, cbase, use_base, f.lo.b, SUHMO_F_PHI)[f.lo.off];
        double bc_ = fptr(ctab, cbase, use_base, f.bq.b, f.dir == 0 ? SUHMO_F_BX : SUHMO_F_BY)[f.bq.off];
        double reg = reflux_coarse(tsize, bc_, phihi, philo, cs);
        const double *phif = ftab[f.fb].f[SUHMO_F_PHI], *bf = ftab[f.fb].f[f.dir == 0 ? SUHMO_F_BX : SUHMO_F_BY];
        const int Pf = fdv[f.fb].P;
        for (int k = 0; k < 2; k++) {
            int idx = f.foff + (f.dir == 0 ? k * Pf : k);
            double ph_hi = phif[idx], ph_lo = f.dir == 0 ? phif[idx - 1] : phif[idx - Pf];
            reg = reflux_add_fine(reg, tsize, bf[idx], ph_hi, ph_lo, fs);
        }
        acc = reflux_apply(acc, sign, rscale, reg);
    }
    lof[T.t.off] = residual ? reflux_residual(acc, fptr(ctab, cdst, use_base, T.t.b, SUHMO_F_RHS)[T.t.off]) : acc;
}
__global__ void k_reflux(const Target *__restrict__ tg, int n, const Face *__restrict__ faces, const FP *__restrict__ ftab, const DV *__restrict__ fdv,
                         const FP *__restrict__ ctab, FP cbase, FP cdst, int use_base, int field_c, double dxc, double dyc, double beta, int residual)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    d_reflux(tg[t], faces, ftab, fdv, ctab, cbase, cdst, use_base, field_c, dxc, dyc, beta, residual);
}
// the refluxes of SEVERAL levels (level l's adds to cells of level l-1 from fluxes of levels l and l-1: no order among them)
struct LvReflux { const Target *tg[SUHMO_LVMAX]; const Face *faces[SUHMO_LVMAX]; const FP *ftab[SUHMO_LVMAX], *ctab[SUHMO_LVMAX]; const DV *fdv[SUHMO_LVMAX];
                  int ntg[SUHMO_LVMAX], nb[SUHMO_LVMAX], use_base[SUHMO_LVMAX]; double dxc[SUHMO_LVMAX], dyc[SUHMO_LVMAX], beta[SUHMO_LVMAX]; int n; };
// ... and, in the workgroups from nb0 on, ONE level's FORT_AVERAGE of the same field onto the cells it covers (the step that follows the reflux in a
// V-cycle's down-leg: it reads the fine residual and writes COVERED coarse cells, the reflux writes uncovered ones next to the coarse-fine faces)
struct AvgPart { const RectEnt *e; const FP *ftab, *ctab; const DV *fdv, *cdv; int use_base, n, gx, gy, nb0; };
__global__ void k_reflux_lv(LvReflux lv, FP cbase, FP cdst, int field_c, int residual, AvgPart av, DV cbdv)
{
    if (av.n > 0 && (int)blockIdx.x >= av.nb0) {
        const int b = blockIdx.x - av.nb0, bx = b % av.gx, by = (b / av.gx) % av.gy, bz = b / (av.gx * av.gy);
        d_avg(av.e[bz], bx * 64 + (int)(threadIdx.x & 63), by * 4 + (int)(threadIdx.x >> 6), av.ftab, av.fdv, field_c, av.ctab, av.cdv, cdst, cbdv, av.use_base, field_c, 0, 0.0);
        return;
    }
    int b = blockIdx.x, q = -1;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t < lv.n && q < 0) { if (b < lv.nb[t]) q = t; else b -= lv.nb[t]; }
    if (q < 0) return;
    const Target *tg = nullptr; const Face *faces = nullptr; const FP *ftab = nullptr, *ctab = nullptr; const DV *fdv = nullptr;
    int ntg = 0, use_base = 0; double dxc = 0.0, dyc = 0.0, beta = 0.0;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t == q) { tg = lv.tg[t]; faces = lv.faces[t]; ftab = lv.ftab[t]; ctab = lv.ctab[t]; fdv = lv.fdv[t]; ntg = lv.ntg[t]; use_base = lv.use_base[t];
                      dxc = lv.dxc[t]; dyc = lv.dyc[t]; beta = lv.beta[t]; }
    const int t = b * blockDim.x + threadIdx.x;
    if (t < ntg) d_reflux(tg[t], faces, ftab, fdv, ctab, cbase, cdst, use_base, field_c, dxc, dyc, beta, residual);
}

// ---- shadow of a level 0 cut into rank strips
constexpr int XF = 4;                                    // fields per all-gather
struct FList { const double *src[XF]; double *dst[XF]; int n; };
__global__ void k_need_pack(const int *__restrict__ need, int first, int n, int shift, FList fl, double *__restrict__ buf, long stride)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int off = need[first + t] - shift;             // the cell in this rank's strip canvas (same pitch, same ghost rows)
    for (int f = 0; f < fl.n; f++) buf[f * stride + t] = fl.src[f][off];
}
__global__ void k_need_unpack(const int *__restrict__ need /* offsets in the compact shadow */, const int2 *__restrict__ rl, int n, FList fl, const double *__restrict__ buf, long stride)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int2 q = rl[t];
    const int off = need[t];
    for (int f = 0; f < fl.n; f++) fl.dst[f][off] = buf[((long)q.x * fl.n + f) * stride + q.y];
}

// ---- owner computes: packed cells from their owners to the mirrors of the ranks that read them
struct FIdx { int f[XF]; int n; };
__global__ void k_sync_pack(const Ref *__restrict__ e, int n, const FP *__restrict__ tab, FIdx fl, double *__restrict__ buf, long stride)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const Ref q = e[t];
    for (int f = 0; f < fl.n; f++) buf[f * stride + t] = tab[q.b].f[fl.f[f]][q.off];
}
__global__ void k_sync_unpack(const SyncRecv *__restrict__ e, int n, const FP *__restrict__ tab, FIdx fl, const double *__restrict__ buf, long stride)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const SyncRecv q = e[t];
    for (int f = 0; f < fl.n; f++) tab[q.d.b].f[fl.f[f]][q.d.off] = buf[((long)q.rank * fl.n + f) * stride + q.pos];
}
}  // namespace

namespace hier {
static inline dim3 g1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

int refresh_tables_upload(suhmo_hier *H, int l, hipStream_t st)      // (refresh_tables found them out of date)
{
    HLev &V = H->lev[l];
    const size_t nb = V.box.size();
    V.tab_epoch = suhmo_fp_epoch();
    bool dirty = V.d_fp == nullptr;
    if (V.h_fp.size() != nb) { V.h_fp.assign(nb, FP{}); dirty = true; }
    for (size_t k = 0; k < nb; k++)
        if (memcmp(&V.h_fp[k], &V.box[k]->d[0].fp, sizeof(FP))) { V.h_fp[k] = V.box[k]->d[0].fp; dirty = true; }
    if (!dirty) return 0;
    HIPCHK(hipStreamSynchronize(st));
    if (!V.d_fp) { HIPCHK(hipMalloc(&V.d_fp, nb * sizeof(FP))); HIPCHK(hipMalloc(&V.d_fp_alt, nb * sizeof(FP))); }
    HIPCHK(hipMemcpy(V.d_fp, V.h_fp.data(), nb * sizeof(FP), hipMemcpyHostToDevice));
    V.h_fp_alt = V.h_fp;
    for (FP &f : V.h_fp_alt) std::swap(f.f[SUHMO_F_PHI], f.f[SUHMO_F_PHI2]);
    HIPCHK(hipMemcpy(V.d_fp_alt, V.h_fp_alt.data(), nb * sizeof(FP), hipMemcpyHostToDevice));
    if (!V.d_dv) {
        std::vector<DV> dv(nb);
        for (size_t k = 0; k < nb; k++) dv[k] = V.box[k]->d[0].v;
        HIPCHK(hipMalloc(&V.d_dv, nb * sizeof(DV)));
        HIPCHK(hipMemcpy(V.d_dv, dv.data(), nb * sizeof(DV), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&V.d_red, (64 * nb + 16) * sizeof(double)));
        for (size_t k = 0; k < nb; k++) { V.maxnx = std::max(V.maxnx, dv[k].nx); V.maxny = std::max(V.maxny, dv[k].ny); }
    }
    return 0;
}
// the two canvases of the head of a level of boxes trade places: in the boxes' handles and by switching to the table that lists them the other way
// round (no copy, nothing uploaded; requires SUHMO_F_PHI2 on every box and current tables)
void swap_head(suhmo_hier *H, int l)
{
    HLev &V = H->lev[l];
    for (suhmo_level *L : V.box) std::swap(L->d[0].fp.f[SUHMO_F_PHI], L->d[0].fp.f[SUHMO_F_PHI2]);
    std::swap(V.d_fp, V.d_fp_alt);
    V.h_fp.swap(V.h_fp_alt);
    V.swapped = !V.swapped;
}

static double *shadow_field(suhmo_hier *H, int field)
{
    if (!H->shadow.f[field]) {
        double *p = nullptr;
        if (hipMalloc(&p, H->shadow_elems * sizeof(double)) != hipSuccess) return nullptr;
        (void)hipMemset(p, 0, H->shadow_elems * sizeof(double));
        H->shadow.f[field] = p;
    }
    return H->shadow.f[field];
}
// the shadow's copies of `fields` of level 0 <- the owners' current values (collective over the ranks of level 0)
static int refresh_base(suhmo_hier *H, const int *fields, int nf, hipStream_t st)
{
    if (!dist_base(H) || H->nlev < 2) return 0;
    // the head is read by several plans in a row (coarse-fine interpolation before every operator of level 1) while level 0 rests:
    // one all-gather serves them.  Whatever writes level 0's head clears the flag (the average from level 1, its own V-cycle, a
    // copy into it) and so does every entry point of the C-ABI (the caller may have loaded new data)
    if (nf == 1 && fields[0] == SUHMO_F_PHI && H->phi_shadow_fresh) return 0;
    SUHMO_TIME("hier: all-gather of the coarse cells level 1 reads");
    if (!H->ag) { suhmo_set_error("hier: level 0 is a rank strip and no all-gather is attached (suhmo_hier_attach_rccl / suhmo_hier_set_allgather)"); return -1; }
    ARG(nf >= 1 && nf <= XF);
    suhmo_level *B = base_of(H);
    FList fl;
    fl.n = nf;
    for (int f = 0; f < nf; f++) {
        fl.src[f] = suhmo_field(B, 0, fields[f]); fl.dst[f] = shadow_field(H, fields[f]);
        if (!fl.src[f] || !fl.dst[f]) { suhmo_set_error("field allocation failed"); return -2; }
    }
    const long stride = H->cnt_max, count = stride * nf;
    const size_t cap = (size_t)stride * XF;
    if (!H->xs) {
        HIPCHK(hipMalloc(&H->xs, std::max<size_t>(1, cap) * sizeof(double)));
        HIPCHK(hipMalloc(&H->xr, std::max<size_t>(1, cap * H->world) * sizeof(double)));
        HIPCHK(hipMemset(H->xs, 0, std::max<size_t>(1, cap) * sizeof(double)));
    }
    const int first = H->seg[H->rank], mine = H->seg[H->rank + 1] - first;
    const DV &sv = B->d[0].v;
    if (mine) hipLaunchKernelGGL(k_need_pack, g1(mine), dim3(256), 0, st, H->need.d, first, mine, sv.j0 * sv.P, fl, H->xs, stride);
    HIPCHK(hipGetLastError());
    int rc = H->ag(H->ag_user, H->xs, count, H->xr, (suhmo_stream_t)st);
    if (rc) return rc;
    H->gathers++;
    if (H->need.n) hipLaunchKernelGGL(k_need_unpack, g1(H->need.n), dim3(256), 0, st, H->need_c.d, H->need_rl.d, (int)H->need.n, fl, H->xr, stride);
    HIPCHK(hipGetLastError());
    for (int f = 0; f < nf; f++) if (fields[f] == SUHMO_F_PHI) H->phi_shadow_fresh = true;
    return 0;
}
static inline int refresh_base1(suhmo_hier *H, int field, hipStream_t st) { return refresh_base(H, &field, 1, st); }

static int part_staging(suhmo_hier *H, size_t doubles, hipStream_t st)
{
    if (doubles <= H->pcap) return 0;
    if (H->ps) { HIPCHK(hipStreamSynchronize(st)); (void)hipFree(H->ps); (void)hipFree(H->pr); H->ps = H->pr = nullptr; }
    H->pcap = doubles + doubles / 4 + 64;
    HIPCHK(hipMalloc(&H->ps, H->pcap * sizeof(double)));
    HIPCHK(hipMalloc(&H->pr, H->pcap * H->world * sizeof(double)));
    HIPCHK(hipMemsetAsync(H->ps, 0, H->pcap * sizeof(double), st));
    return 0;
}
// fields of level lt (the level whose cells S lists) from their owners into this rank's mirrors; collective over the ranks (skipped by all
// of them alike when nothing of this kind travels anywhere)
static int sync_run(suhmo_hier *H, int lt, Sync &S, const int *fields, int nf, hipStream_t st)
{
    if (S.stride == 0) return 0;
    SUHMO_TIME("hier: exchange of packed cells between the owners of a level's boxes");
    if (!H->ag) { suhmo_set_error("hier: level %d is partitioned over the ranks and no all-gather is attached (suhmo_hier_attach_rccl / suhmo_hier_set_allgather)", lt); return -1; }
    ARG(nf >= 1 && nf <= XF);
    int rc;
    FIdx fl; fl.n = nf;
    for (int f = 0; f < nf; f++) { fl.f[f] = fields[f]; if ((rc = ensure_field(H, lt, fields[f]))) return rc; }
    if ((rc = refresh_tables(H, lt, st)) || (rc = part_staging(H, (size_t)nf * S.stride, st))) return rc;
    HLev &V = H->lev[lt];
    if (S.send.n) hipLaunchKernelGGL(k_sync_pack, g1(S.send.n), dim3(256), 0, st, S.send.d, (int)S.send.n, V.d_fp, fl, H->ps, S.stride);
    HIPCHK(hipGetLastError());
    if ((rc = H->ag(H->ag_user, H->ps, (long)nf * S.stride, H->pr, (suhmo_stream_t)st))) return rc;
    H->part_gathers++; H->part_bytes += 8L * nf * (long)S.send.n;
    if (S.recv.n) hipLaunchKernelGGL(k_sync_unpack, g1(S.recv.n), dim3(256), 0, st, S.recv.d, (int)S.recv.n, V.d_fp, fl, H->pr, S.stride);
    HIPCHK(hipGetLastError());
    return 0;
}
static inline int sync1(suhmo_hier *H, int lt, Sync &S, int field, hipStream_t st) { return sync_run(H, lt, S, &field, 1, st); }

// coarse-side arguments of a kernel that reads / writes level l-1.  base / bdv: where the cells of level 0 are READ (the shadow
// of a cut level 0); dst / ddv: where they are written (the level, or this rank's strip of it)
struct CoarseArgs { const FP *tab; const DV *dv; FP base; DV bdv; FP dst; DV ddv; int use_base; };
static int coarse_args(suhmo_hier *H, int lc, hipStream_t st, CoarseArgs &a)
{
    memset(&a, 0, sizeof(a));
    if (lc == 0) {
        a.dst = base_of(H)->d[0].fp; a.ddv = base_of(H)->d[0].v; a.use_base = 1;
        if (dist_base(H)) { a.base = H->shadow; a.bdv = H->vglob; } else { a.base = a.dst; a.bdv = a.ddv; }
        return 0;
    }
    int rc = refresh_tables(H, lc, st); if (rc) return rc;
    a.tab = H->lev[lc].d_fp; a.dv = H->lev[lc].d_dv; a.bdv = H->lev[lc].box[0]->d[0].v;
    return 0;
}

// Copier::exchange of one or two cell fields of level l
// colour >= 0 (owner computes, after a colour pass of the head): only the side cells of that colour have changed and travel
int hier_ff(suhmo_hier *H, int l, int f0, int f1, bool corners, hipStream_t st, int colour)
{
    if (l == 0) return 0;                                   // the base canvas: a neighbour's cell IS the ghost
    HLev &V = H->lev[l];
    int rc;
    if ((rc = ensure_field(H, l, f0)) || (f1 >= 0 && (rc = ensure_field(H, l, f1))) || (rc = refresh_tables(H, l, st))) return rc;
    const bool head_sides = f0 == SUHMO_F_PHI && f1 < 0 && !corners;
    if (head_sides && H->ff_seen[l] == H->phi_ver[l]) return 0;              // the side ghosts of the head are current
    if (head_sides) H->ff_seen[l] = H->phi_ver[l];
    if (V.part) {                                           // the source cells other ranks own -> their mirrors here, then the copies below
        const int fl[2] = {f0, f1};
        Sync &S = corners ? V.sy_all : (colour >= 0 ? V.sy_side[colour & 1] : V.sy_sides);
        if ((rc = sync_run(H, l, S, fl, f1 >= 0 ? 2 : 1, st))) return rc;
    }
    // (a corner ghost's source is a valid cell, never a ghost: sides and corners do not depend on each other)
    return hier_ff_on(H, l, V.d_fp, f0, f1, corners, st);
}
// the launch of hier_ff / hier_pwl over tables the caller holds: canvases with the geometry of the boxes' own, numbered as the caller likes
// (suhmo_flatten.hip: its private scratch).  Levels held whole by this process
int hier_ff_on(suhmo_hier *H, int l, const FP *tab, int f0, int f1, bool corners, hipStream_t st)
{
    HLev &V = H->lev[l];
    const DevVec<CopyEnt> &list = corners ? V.ff_all : V.ff_side;
    if (list.n) hipLaunchKernelGGL(k_ff, g1(list.n), dim3(256), 0, st, list.d, (int)list.n, tab, f0, f1);
    HIPCHK(hipGetLastError());
    return 0;
}
int hier_pwl_on(suhmo_hier *H, int l, const FP *ftab, int ff, const FP *ctab, const FP &cbase, int use_base, int fc, hipStream_t st)
{
    HLev &V = H->lev[l];
    if (V.pwl.n) hipLaunchKernelGGL(k_pwl, g1(V.pwl.n), dim3(256), 0, st, V.pwl.d, (int)V.pwl.n, ftab, ff, ctab, cbase, use_base, fc);
    HIPCHK(hipGetLastError());
    return 0;
}
// QuadCFInterp: coarse-fine ghosts of field ff of level l <- field fc of level l-1
int hier_cf(suhmo_hier *H, int l, int ff, int fc, hipStream_t st, int ff1, int fc1)
{
    SUHMO_TIME("QuadCFInterp::coarseFineInterp");
    if (l == 0) return 0;
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l, ff)) || (rc = ensure_field(H, l - 1, fc)) || (rc = refresh_tables(H, l, st))) return rc;
    if (ff1 >= 0 && ((rc = ensure_field(H, l, ff1)) || (rc = ensure_field(H, l - 1, fc1)) || (rc = refresh_tables(H, l, st)))) return rc;
    { const int fl[2] = {fc, fc1};
      if (l == 1) rc = refresh_base(H, fl, ff1 >= 0 ? 2 : 1, st); else rc = V.part ? sync_run(H, l - 1, V.sy_cread, fl, ff1 >= 0 ? 2 : 1, st) : 0;
      if (rc) return rc; }
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    if (V.cf.n) hipLaunchKernelGGL(k_cf, g1(V.cf.n), dim3(256), 0, st, V.cf.d, (int)V.cf.n, V.d_fp, ff, ca.tab, ca.base, ca.use_base, fc, ff1, fc1);
    HIPCHK(hipGetLastError());
    return 0;
}
// hier_cf + hier_ff of the same field(s) in one launch (levels held whole by this process)
int hier_cf_ff(suhmo_hier *H, int l, int ff, int fc, int ff1, int fc1, bool corners, hipStream_t st)
{
    SUHMO_TIME("QuadCFInterp::coarseFineInterp + exchange");
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l, ff)) || (rc = ensure_field(H, l - 1, fc)) || (rc = refresh_tables(H, l, st))) return rc;
    if (ff1 >= 0 && ((rc = ensure_field(H, l, ff1)) || (rc = ensure_field(H, l - 1, fc1)) || (rc = refresh_tables(H, l, st)))) return rc;
    { const int fl[2] = {fc, fc1};
      if (l == 1 && (rc = refresh_base(H, fl, ff1 >= 0 ? 2 : 1, st))) return rc; }
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    const DevVec<CopyEnt> &list = corners ? V.ff_all : V.ff_side;
    const int nbcf = (int)g1(V.cf.n).x, nbff = (int)g1(list.n).x;
    if (nbcf + nbff > 0)
        hipLaunchKernelGGL(k_cf_ff, dim3(nbcf + nbff), dim3(256), 0, st, V.cf.d, (int)V.cf.n, nbcf, list.d, (int)list.n, V.d_fp, ff, ca.tab, ca.base, ca.use_base, fc, ff1, fc1);
    HIPCHK(hipGetLastError());
    return 0;
}
int hier_pwl(suhmo_hier *H, int l, int ff, int fc, hipStream_t st)
{
    if (l == 0) return 0;
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l, ff)) || (rc = ensure_field(H, l - 1, fc)) || (rc = refresh_tables(H, l, st))) return rc;
    if (l == 1 && (rc = refresh_base1(H, fc, st))) return rc;
    if (l > 1 && V.part && (rc = sync1(H, l - 1, V.sy_cread, fc, st))) return rc;
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    return hier_pwl_on(H, l, V.d_fp, ff, ca.tab, ca.base, ca.use_base, fc, st);
}
// FORT_AVERAGE of field ff of level l into the covered cells of field fc of level l-1 (mode 0) / covered cells <- val (mode 1)
int hier_avg(suhmo_hier *H, int l, int ff, int fc, int mode, double val, hipStream_t st)
{
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l, ff)) || (rc = ensure_field(H, l - 1, fc)) || (rc = refresh_tables(H, l, st)) || (rc = coarse_args(H, l - 1, st, ca))) return rc;
    if (fc == SUHMO_F_PHI) { for (suhmo_level *L : H->lev[l - 1].box) L->d[0].phi_fresh = 0; H->phi_ver[l - 1]++; }
    if (fc == SUHMO_F_PHI && l == 1) H->phi_shadow_fresh = false;
    if (fc == SUHMO_F_ZB) for (suhmo_level *L : H->lev[l - 1].box) suhmo_zb_written(L);
    if (fc == SUHMO_F_MASK) for (suhmo_level *L : H->lev[l - 1].box) suhmo_mask_written(L);      // (level 0 is a whole level: it may know its mask clean)
    if (mode == 1) {                                        // geometry only: every holder of coarse cells marks / zeroes its own
        if (V.avg_cov.n) {
            dim3 grd((V.cov_w + 63) / 64, (V.cov_h + 3) / 4, (unsigned)V.avg_cov.n);
            hipLaunchKernelGGL(k_avg, grd, dim3(64, 4), 0, st, V.avg_cov.d, V.d_fp, V.d_dv, ff, ca.tab, ca.dv, ca.dst, ca.ddv, ca.use_base, fc, mode, val);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (V.avg.n) {
        dim3 grd((V.avg_w + 63) / 64, (V.avg_h + 3) / 4, (unsigned)V.avg.n);
        hipLaunchKernelGGL(k_avg, grd, dim3(64, 4), 0, st, V.avg.d, V.d_fp, V.d_dv, ff, ca.tab, ca.dv, ca.dst, ca.ddv, ca.use_base, fc, mode, val);
    }
    HIPCHK(hipGetLastError());
    if (V.part && V.put_stride) {
        // owner computes: averages of this rank's fine boxes over coarse cells another rank holds travel in this rank's segment of one
        // all-gather; the holder of the coarse cells takes its rectangles from there (FORT_AVERAGE's sum, the same bits)
        SUHMO_TIME("hier: averages onto coarse cells other ranks hold");
        if (!H->ag) { suhmo_set_error("hier: level %d is partitioned over the ranks and no all-gather is attached", l); return -1; }
        if ((rc = part_staging(H, (size_t)V.put_stride, st))) return rc;
        if (V.avg_put.n) {
            dim3 grd((V.put_w + 63) / 64, (V.put_h + 3) / 4, (unsigned)V.avg_put.n);
            hipLaunchKernelGGL(k_avg_put, grd, dim3(64, 4), 0, st, V.avg_put.d, V.d_fp, V.d_dv, ff, H->ps);
        }
        HIPCHK(hipGetLastError());
        if ((rc = H->ag(H->ag_user, H->ps, V.put_stride, H->pr, (suhmo_stream_t)st))) return rc;
        H->part_gathers++;
        H->part_bytes += 8L * V.put_mine;
        if (V.avg_get.n) {
            dim3 grd((V.get_w + 63) / 64, (V.get_h + 3) / 4, (unsigned)V.avg_get.n);
            hipLaunchKernelGGL(k_put_unpack, grd, dim3(64, 4), 0, st, V.avg_get.d, ca.tab, ca.dv, ca.dst, ca.ddv, ca.use_base, fc, H->pr, V.put_stride);
        }
        HIPCHK(hipGetLastError());
    }
    return 0;
}
// AMRProlongS_2 (:1143-1206): PHI of level l += PROLONG_2_NL(field_c of level l-1), the coarse field gathered per box with
// its physical-BC ghosts (inhomogeneous in FAS mode)
// minus_saved: the coarse field is field_c minus what hier_window_save kept of it (the correction of a FAS cycle: only the
// windows of it are ever formed)
int hier_window_save(suhmo_hier *H, int l, int field_c, hipStream_t st)
{
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l - 1, field_c)) || (rc = refresh_tables(H, l, st))) return rc;
    if (l == 1 && (rc = refresh_base1(H, field_c, st))) return rc;
    if (l > 1 && V.part && (rc = sync1(H, l - 1, V.sy_win, field_c, st))) return rc;
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    if (!V.winold) {
        HIPCHK(hipMalloc(&V.winold, std::max<size_t>(1, V.winelems) * sizeof(double)));
        HIPCHK(hipMemsetAsync(V.winold, 0, std::max<size_t>(1, V.winelems) * sizeof(double), st));
    }
    if (V.wing.n) {
        dim3 grd((V.wing_w + 63) / 64, (V.wing_h + 3) / 4, (unsigned)V.wing.n);
        hipLaunchKernelGGL(k_win_gather, grd, dim3(64, 4), 0, st, V.wing.d, V.winold, ca.tab, ca.dv, ca.base, ca.bdv, ca.use_base, field_c, V.d_win, V.d_wing_box);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// leave_below (l - 1 >= 1): the level below leaves its FAS problem in the same launch, field_c = PHI minus PHIOLD formed on the fly
int hier_prolong2(suhmo_hier *H, int l, int field_c, hipStream_t st, bool minus_saved, bool leave_below)
{
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if (leave_below && !(H->fused_prolong && V.win_max <= 6144 && !V.part && !H->lev[l - 1].part && l - 1 >= 1)) {     // two launches after all
        suhmo_multi mc;
        if ((rc = multi_of(H, l - 1, st, mc)) || (rc = launch_fas_leave(mc.on(), st))) return rc;
        return hier_prolong2(H, l, SUHMO_F_CORR, st);
    }
    if ((rc = ensure_field(H, l - 1, field_c)) || (rc = refresh_tables(H, l, st))) return rc;
    if (l == 1 && (rc = refresh_base1(H, field_c, st))) return rc;
    if (l > 1 && V.part && (rc = sync1(H, l - 1, V.sy_win, field_c, st))) return rc;
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    for (suhmo_level *L : V.box) L->d[0].phi_fresh = 0;
    H->phi_ver[l]++;
    const int k0 = V.first_owned(), nk = V.n_owned();                 // (owner computes: the windows of this rank's boxes)
    if (nk <= 0) return 0;
    if (leave_below) {
        suhmo_multi mc;
        if ((rc = multi_of(H, l - 1, st, mc))) return rc;
        const int cgx = (mc.maxnx + 2 + 63) / 64, cgy = (mc.maxny + 2 + 3) / 4;
        hipLaunchKernelGGL(k_prolong2_fused, dim3(nk + cgx * cgy * mc.nbox), dim3(256), (size_t)V.win_max * sizeof(double), st, V.wing.d, V.wstart.d, V.d_win, k0,
                           ca.tab, ca.dv, ca.base, ca.bdv, ca.use_base, (int)SUHMO_F_PHI, (const double *)nullptr, V.d_fp, V.d_dv, (int)SUHMO_F_PHIOLD, nk, cgx, cgy);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (H->fused_prolong && V.win_max <= 6144) {                       // gather + BC + PROLONG_2_NL of a box in one workgroup, the window in LDS
        hipLaunchKernelGGL(k_prolong2_fused, dim3(nk), dim3(256), (size_t)V.win_max * sizeof(double), st, V.wing.d, V.wstart.d, V.d_win, k0,
                           ca.tab, ca.dv, ca.base, ca.bdv, ca.use_base, field_c, minus_saved ? V.winold : nullptr, V.d_fp, V.d_dv, -1, nk, 1, 1);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (V.wing.n) {
        dim3 grd((V.wing_w + 63) / 64, (V.wing_h + 3) / 4, (unsigned)V.wing.n);
        hipLaunchKernelGGL(k_win_gather, grd, dim3(64, 4), 0, st, V.wing.d, V.winbuf, ca.tab, ca.dv, ca.base, ca.bdv, ca.use_base, field_c, V.d_win, V.d_wing_box,
                           minus_saved ? V.winold : nullptr);
    }
    int maxp = 0, maxx = 0, maxy = 0;
    for (const Win &w : V.win) maxp = std::max(maxp, 2 * (w.nx - 2) + 2 * (w.ny - 2));
    for (suhmo_level *L : V.box) { maxx = std::max(maxx, L->d[0].v.nx); maxy = std::max(maxy, L->d[0].v.ny); }
    hipLaunchKernelGGL(k_win_bc, dim3((maxp + 255) / 256, nk), dim3(256), 0, st, V.d_win + k0, nk, V.winbuf, ca.bdv);
    hipLaunchKernelGGL(k_prolong2_win, dim3((maxx + 63) / 64, (maxy + 3) / 4, nk), dim3(64, 4), 0, st, V.d_win + k0, V.winbuf, V.d_fp + k0, V.d_dv + k0);
    HIPCHK(hipGetLastError());
    return 0;
}
// reflux (src/VCAMRNonLinearPoissonOp.cpp:555-652): field_c of level l-1 (holding L(phi)) += the flux mismatch on the
// coarse-fine faces of level l
int hier_reflux(suhmo_hier *H, int l, int field_c, hipStream_t st, int residual)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::reflux");
    HLev &V = H->lev[l];
    int rc;
    CoarseArgs ca;
    if ((rc = ensure_field(H, l - 1, field_c)) || (rc = refresh_tables(H, l, st))) return rc;
    if (field_c == SUHMO_F_ZB) for (suhmo_level *L : H->lev[l - 1].box) suhmo_zb_written(L);
    if (field_c == SUHMO_F_MASK) for (suhmo_level *L : H->lev[l - 1].box) suhmo_mask_written(L);
    { const int fl[3] = {SUHMO_F_PHI, SUHMO_F_BX, SUHMO_F_BY};
      if (l == 1) { if ((rc = refresh_base(H, fl, 3, st))) return rc; }
      else if (V.part && (rc = sync_run(H, l - 1, V.sy_cread, fl, 3, st))) return rc;
      // owner computes: the register is added up where the coarse cell lives; the fine cells and faces next to the coarse-fine faces come along
      if (V.part && (rc = sync_run(H, l, V.sy_fface, fl, 3, st))) return rc; }
    if ((rc = coarse_args(H, l - 1, st, ca))) return rc;
    const DV &vc = H->lev[l - 1].box[0]->d[0].v;
    if (V.targets.n)
        hipLaunchKernelGGL(k_reflux, g1(V.targets.n), dim3(256), 0, st, V.targets.d, (int)V.targets.n, V.faces.d, V.d_fp, V.d_dv, ca.tab, ca.base, ca.dst,
                           ca.use_base, field_c, vc.dx, vc.dy, vc.beta, residual);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- several levels per launch (option merged_launches; this process holds every box and the whole of level 0)
// coarse-fine and fine-fine side ghosts of the head of the levels llo .. lhi (>= 1) that are stale: ONE launch
int ghosts_levels(suhmo_hier *H, int llo, int lhi, suhmo_stream_t s)
{
    LvGhosts g;
    memset(&g, 0, sizeof(g));
    int rc, nb = 0;
    for (int l = std::max(1, llo); l <= lhi; l++) {
        HLev &V = H->lev[l];
        const bool cf_ok = H->cf_seen[l][0] == H->phi_ver[l] && H->cf_seen[l][1] == H->phi_ver[l - 1], ff_ok = H->ff_seen[l] == H->phi_ver[l];
        if (cf_ok && ff_ok) continue;
        if ((rc = ensure_field(H, l, SUHMO_F_PHI)) || (rc = ensure_field(H, l - 1, SUHMO_F_PHI)) || (rc = refresh_tables(H, l, HST(s)))) return rc;
        if (l - 1 >= 1 && (rc = refresh_tables(H, l - 1, HST(s)))) return rc;
        const int q = g.n++;
        g.cf[q] = V.cf.d; g.ncf[q] = (int)V.cf.n; g.nbcf[q] = (int)g1(V.cf.n).x;
        g.ff[q] = V.ff_side.d; g.nff[q] = (int)V.ff_side.n;
        g.nb[q] = g.nbcf[q] + (int)g1(V.ff_side.n).x;
        g.ftab[q] = V.d_fp; g.ctab[q] = l - 1 >= 1 ? H->lev[l - 1].d_fp : nullptr; g.use_base[q] = l - 1 == 0;
        nb += g.nb[q];
        H->cf_seen[l][0] = H->phi_ver[l]; H->cf_seen[l][1] = H->phi_ver[l - 1]; H->ff_seen[l] = H->phi_ver[l];
    }
    if (nb > 0) {
        SUHMO_TIME("QuadCFInterp::coarseFineInterp + exchange");
        hipLaunchKernelGGL(k_cf_ff_lv, dim3(nb), dim3(256), 0, HST(s), g, base_of(H)->d[0].fp, (int)SUHMO_F_PHI);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// the refluxes of the levels lhi .. llo + 1 into RES of the level below each (the residual form of hier_reflux) in ONE launch; average_down:
// AMRRestrictS of the residual of level lhi rides along (hier_avg(H, lhi, RES, RES, 0))
int reflux_levels(suhmo_hier *H, int lhi, int llo, bool average_down, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::reflux");
    int rc;
    LvReflux r;
    memset(&r, 0, sizeof(r));
    int nb = 0;
    for (int l = lhi; l > llo; l--) {
        HLev &V = H->lev[l];
        if (!V.targets.n) continue;
        if ((rc = refresh_tables(H, l, HST(s))) || (l - 1 >= 1 && (rc = refresh_tables(H, l - 1, HST(s))))) return rc;
        const DV &vc = H->lev[l - 1].box[0]->d[0].v;
        const int q = r.n++;
        r.tg[q] = V.targets.d; r.ntg[q] = (int)V.targets.n; r.nb[q] = (int)g1(V.targets.n).x; r.faces[q] = V.faces.d;
        r.ftab[q] = V.d_fp; r.fdv[q] = V.d_dv; r.ctab[q] = l - 1 >= 1 ? H->lev[l - 1].d_fp : nullptr; r.use_base[q] = l - 1 == 0;
        r.dxc[q] = vc.dx; r.dyc[q] = vc.dy; r.beta[q] = vc.beta;
        nb += r.nb[q];
    }
    AvgPart av;
    memset(&av, 0, sizeof(av));
    if (average_down) {
        HLev &V = H->lev[lhi];
        CoarseArgs ca;
        if ((rc = refresh_tables(H, lhi, HST(s))) || (rc = coarse_args(H, lhi - 1, HST(s), ca))) return rc;
        av.e = V.avg.d; av.n = (int)V.avg.n; av.ftab = V.d_fp; av.fdv = V.d_dv; av.ctab = ca.tab; av.cdv = ca.dv; av.use_base = ca.use_base;
        av.gx = (V.avg_w + 63) / 64; av.gy = (V.avg_h + 3) / 4; av.nb0 = nb;
        nb += av.gx * av.gy * av.n;
    }
    if (nb > 0) hipLaunchKernelGGL(k_reflux_lv, dim3(nb), dim3(256), 0, HST(s), r, base_of(H)->d[0].fp, base_of(H)->d[0].fp, (int)SUHMO_F_RES, 1, av, base_of(H)->d[0].v);
    HIPCHK(hipGetLastError());
    return 0;
}

// COVER of the whole level 0 (geometry only): the moulin integrals run over all of it
int cover_whole_base(suhmo_hier *H)
{
    const size_t welems = (size_t)H->vglob.P * (size_t)(H->vglob.rows + 1);
    if (hipMalloc(&H->cover_whole, welems * sizeof(double)) != hipSuccess) { suhmo_set_error("field allocation failed"); return -2; }
    HIPCHK(hipMemset(H->cover_whole, 0, welems * sizeof(double)));
    FP whole{}; whole.f[SUHMO_F_COVER] = H->cover_whole;
    HLev &V = H->lev[1];
    if (H->cover_full.n) {
        int w = 0, h = 0;
        std::vector<RectEnt> tmp(H->cover_full.n);
        HIPCHK(hipMemcpy(tmp.data(), H->cover_full.d, tmp.size() * sizeof(RectEnt), hipMemcpyDeviceToHost));
        for (auto &e : tmp) { w = std::max(w, e.w); h = std::max(h, e.h); }
        dim3 grd((w + 63) / 64, (h + 3) / 4, (unsigned)H->cover_full.n);
        hipLaunchKernelGGL(k_avg, grd, dim3(64, 4), 0, nullptr, H->cover_full.d, V.d_fp, V.d_dv, (int)SUHMO_F_COVER, (const FP *)nullptr, (const DV *)nullptr,
                           whole, H->vglob, 1, (int)SUHMO_F_COVER, 1, 1.0);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
}  // namespace hier
