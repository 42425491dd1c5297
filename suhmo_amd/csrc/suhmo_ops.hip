// suhmo_ops.hip -- the level's operator kernels: ghost fill, applyOp / residual, restriction, prolongation, vector operations and norms, and the
// same for every box of a multi-box AMR level in one launch.  (Split off suhmo_level.hip in round 4; reference citations: file:line in the SUHMO checkout.)
#include "suhmo_hier.h"
#include "suhmo_level_int.h"
#include "suhmo_batch.h"
#include "suhmo_transfer.h"
#include "suhmo_reduce.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>
// ------------------------------------------------------------------ kernels

// exchange (periodic wrap) + mixBCValues into the stored ghost ring of a cell field
// (src/AmrHydro.cpp:248-309).  One thread per perimeter cell.
__device__ __forceinline__ void d_fill_ghosts(const DV &v, double *__restrict__ p, int homog)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * v.ny) {                       // x sides
        int side = t / v.ny, j = t % v.ny;
        if (v.cfx[side]) return;              // coarse-fine side: ghost columns hold interpolated data
        int i = side ? v.nx - 1 : 0;
        int idx = cidx(v, i, j);
        double c = p[idx];
        if (side) p[idx + 1] = phiE(v, p, idx, i, c, homog); else p[idx - 1] = phiW(v, p, idx, i, c, homog);
        return;
    }
    t -= 2 * v.ny;
    if (t < 2 * v.nx) {                       // y sides
        int side = t / v.nx, i = t % v.nx;
        if (v.ext[side]) return;              // rank boundary: ghost rows hold exchanged data
        int j = side ? v.ny - 1 : 0;
        int idx = cidx(v, i, j);
        double c = p[idx];
        if (side) p[idx + v.P] = phiN(v, p, idx, j, c, homog); else p[idx - v.P] = phiS(v, p, idx, j, c, homog);
    }
}
template <class T> __global__ void k_fill_ghosts(T t, int field, int homog) { d_fill_ghosts(t.view(), t.field(field), homog); }
template <class T> int launch_fill_ghosts(const T &t, int field, int homog, hipStream_t st) { return launch_over(k_fill_ghosts<T>, t, PERIMETER, st, field, homog); }
template int launch_fill_ghosts(const OnBoxes &, int, int, hipStream_t);
template int launch_fill_ghosts(const OnMembers &, int, int, hipStream_t);

extern "C" int suhmo_level_fill_ghosts(suhmo_level_t *L, int depth, int field, int homogeneous, suhmo_stream_t s)
{
    CHECK_DF(L, depth, field); ARG(!is_face(field));
    HIPCHK(hipSetDevice(L->device));
    if (!suhmo_field(L, depth, field)) return -2;
    if (field == SUHMO_F_ZB) suhmo_zb_written(L);
    if (field == SUHMO_F_MASK) suhmo_mask_written(L);      // (the stored ghost ring is part of what the gradient's mask tests read)
    return launch_fill_ghosts(on_level(L, depth), field, homogeneous, (hipStream_t)s);
}

// VCNLCOMPUTEOP2D / VCNLCOMPUTERES2D with BC, NL fused.  MODE 0: LPHI = L(phi); 1: RES = rhs - L(phi);
// 2: the FAS right-hand side of a coarse depth in one pass: LPHI = L(phi), RHS = axby(RES, LPHI, 1, 1), PHIOLD = phi
// 3: LPHI = L(phi) and RES = axby(LPHI, RHS, -1, 1) in one pass (the composite residual of an AMR level, suhmo_hier.hip)
// (returns what it stored in RES, MODE 1 / 3; 0 for a thread outside the level)
template <bool HAS_ALPHA, int MODE>
__device__ __forceinline__ double d_apply_at(const DV &v, const FP &fp, suhmo_phys_t ph, int homog, int halo, int hcomp, int i, int j)
{
    if (i >= v.nx || j >= v.ny + halo) return 0.0;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    int idx = cidx(v, i, j);
    if (MODE == 2 && (j < 0 || j >= v.ny)) {
        // rank strip: the first hcomp halo rows beyond a rank boundary get the neighbour's right-hand side computed here (its phi
        // and RES were exchanged together), which saves the exchange of RHS; the rows further out only copy phi
        const bool comp = (j < 0 && v.rk[0] && j >= -hcomp) || (j >= v.ny && v.rk[1] && j < v.ny + hcomp);
        if (!comp) { fp.f[SUHMO_F_PHIOLD][idx] = phi[idx]; return 0.0; }
    }
    double c = phi[idx];
    double e = phiE(v, phi, idx, i, c, homog), w = phiW(v, phi, idx, i, c, homog);
    double n = phiN(v, phi, idx, j, c, homog), s = phiS(v, phi, idx, j, c, homog);
    double bxW = fp.f[SUHMO_F_BX][idx], bxE = fp.f[SUHMO_F_BX][idx + 1];
    double byS = fp.f[SUHMO_F_BY][idx], byN = fp.f[SUHMO_F_BY][idx + v.P];
    double nl, dnl;
    nl_terms(ph, c, fp.f[SUHMO_F_B][idx], fp.f[SUHMO_F_PI][idx], fp.f[SUHMO_F_ZB][idx], fp.f[SUHMO_F_MASK][idx], nl, dnl);
    double aterm = HAS_ALPHA ? v.alpha * fp.f[SUHMO_F_ACOEF][idx] : v.alpha;
    double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, byN, byS, nl);
    double res = 0.0;
    if (MODE == 0) fp.f[SUHMO_F_LPHI][idx] = lofphi;
    else if (MODE == 1) fp.f[SUHMO_F_RES][idx] = res = fp.f[SUHMO_F_RHS][idx] - lofphi;
    else if (MODE == 3) { fp.f[SUHMO_F_LPHI][idx] = lofphi; fp.f[SUHMO_F_RES][idx] = res = -1.0 * lofphi + 1.0 * fp.f[SUHMO_F_RHS][idx]; }
    else {
        fp.f[SUHMO_F_LPHI][idx] = lofphi;
        fp.f[SUHMO_F_RHS][idx] = 1.0 * fp.f[SUHMO_F_RES][idx] + 1.0 * lofphi;
        fp.f[SUHMO_F_PHIOLD][idx] = c;
    }
    return res;
}
template <bool HAS_ALPHA, int MODE>
__device__ __forceinline__ void d_apply(const DV &v, const FP &fp, suhmo_phys_t ph, int homog, int halo, int hcomp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - halo;     // MODE 2 on a rank strip: the halo rows only copy phi
    d_apply_at<HAS_ALPHA, MODE>(v, fp, ph, homog, halo, hcomp, i, j);
}
template <class T, bool HAS_ALPHA, int MODE>
__global__ __launch_bounds__(256) void k_apply(T t, int homog, int halo, int hcomp)
{
    d_apply<HAS_ALPHA, MODE>(t.view(), t.fields(), t.phys(), homog, halo, hcomp);
}
// the operator over the cells of a target and `halo` rows beyond both y sides (MODE 2 on a rank strip)
template <int MODE, class T> static int launch_apply(const T &t, bool has_alpha, int homog, hipStream_t st, int halo = 0, int hcomp = 0)
{
    const dim3 grd = grid2d(t.nx(), t.ny() + 2 * halo);
    if (has_alpha) return launch_grid(k_apply<T, true, MODE>, t, grd, BLK2D, st, homog, halo, hcomp);
    return launch_grid(k_apply<T, false, MODE>, t, grd, BLK2D, st, homog, halo, hcomp);
}
// RES = rhs - L(phi) and, in the same pass, the first stage of its max norm (one partial per workgroup, as k_norm_partial leaves them for
// k_norm_final): the solve loop's residual evaluation on levels whose cycle's last launch cannot leave it behind (the tile-kernel sizes)
template <bool HAS_ALPHA>
__device__ __forceinline__ void d_residual_norm(const DV &v, const FP &fp, const suhmo_phys_t &ph, double *__restrict__ partial)
{
    __shared__ double sm[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    const double r = wave_max(fabs(d_apply_at<HAS_ALPHA, 1>(v, fp, ph, 0, 0, 0, i, j)));
    if (threadIdx.x == 0) sm[threadIdx.y] = r;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
// (a member of an ensemble: its partial maxima at partial + member * workgroups, in the order of a level's own launch)
template <class T, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void k_residual_norm(T t, double *__restrict__ partial)
{
    d_residual_norm<HAS_ALPHA>(t.view(), t.fields(), t.phys(), partial + t.slot((size_t)gridDim.x * gridDim.y));
}
template <class T> static int launch_residual_norm(const T &t, bool has_alpha, double *partial, hipStream_t st)
{
    if (has_alpha) return launch_over(k_residual_norm<T, true>, t, CELLS, st, partial);
    return launch_over(k_residual_norm<T, false>, t, CELLS, st, partial);
}
// LPHI and RES = rhs - LPHI on a list of rectangles (x = first column, y = first row, z = columns, w = rows) of the level: the part of
// a composite residual that has changed since the whole level was evaluated (suhmo_hier.hip); overlapping rectangles write the same values
template <bool HAS_ALPHA>
__global__ __launch_bounds__(256) void k_apply_rects(DV v, FP fp, suhmo_phys_t ph, const int4 *__restrict__ rects)
{
    const int4 r = rects[blockIdx.z];
    const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y * blockDim.y + threadIdx.y;
    if (a >= r.z || b >= r.w) return;
    d_apply_at<HAS_ALPHA, 3>(v, fp, ph, 0, 0, 0, r.x + a, r.y + b);
}

// the box of blockIdx.z among the boxes of several levels: its level's slot q (unrolled: constant indices only), its index in that level
__device__ __forceinline__ bool lv_find(const suhmo_lvboxes &lv, int &q, int &k)
{
    int z = blockIdx.z;
    q = -1; k = 0;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t < lv.n && q < 0) { if (z < lv.nbox[t]) { q = t; k = z; } else z -= lv.nbox[t]; }
    return q >= 0;
}
#define LV_PICK(lv, q, member, out) do { _Pragma("unroll") for (int t_ = 0; t_ < SUHMO_LVMAX; t_++) if (t_ == (q)) (out) = (lv).member[t_]; } while (0)
template <bool HAS_ALPHA>
__global__ __launch_bounds__(256) void k_apply_lv(suhmo_lvboxes lv, suhmo_phys_t ph)
{
    int q, k;
    if (!lv_find(lv, q, k)) return;
    const DV *dv = nullptr; const FP *fp = nullptr; int mode = 1;
    LV_PICK(lv, q, dv, dv); LV_PICK(lv, q, fp, fp); LV_PICK(lv, q, mode, mode);
    if (mode == 1) d_apply<HAS_ALPHA, 1>(dv[k], fp[k], ph, 0, 0, 0);
    else d_apply<HAS_ALPHA, 3>(dv[k], fp[k], ph, 0, 0, 0);
}
int suhmo_levels_apply(const suhmo_lvboxes &lv, const suhmo_phys_t &ph, bool has_alpha, hipStream_t st)
{
    int nz = 0;
    for (int q = 0; q < lv.n; q++) nz += lv.nbox[q];
    if (nz <= 0) return 0;
    const dim3 grd((lv.maxnx + 63) / 64, (lv.maxny + 3) / 4, nz);
    if (has_alpha) hipLaunchKernelGGL(k_apply_lv<true>, grd, BLK2D, 0, st, lv, ph);
    else hipLaunchKernelGGL(k_apply_lv<false>, grd, BLK2D, 0, st, lv, ph);
    HIPCHK(hipGetLastError());
    return 0;
}

int suhmo_exchange_fields(suhmo_level *L, int depth, std::initializer_list<int> fields, hipStream_t st)
{
    const DV &v = L->d[depth].v;
    if (!(L->ex && (v.ext[0] || v.ext[1]))) return 0;
    for (int f : fields) if (!suhmo_field(L, depth, f)) return -2;
    int rc = L->ex(L->user, L, depth, fields.begin(), (int)fields.size(), (suhmo_stream_t)st);
    if (!rc) for (int f : fields) if (f == SUHMO_F_PHI) L->d[depth].phi_fresh = suhmo_halo_rows(v);
    for (int f : fields) if (f == SUHMO_F_MASK) suhmo_mask_halo_written(L);
    for (int f : fields) if (f == SUHMO_F_ZB) suhmo_zb_written(L);
    return rc;
}
int suhmo_exchange_list(suhmo_level *L, int depth, const int *fields, int n, hipStream_t st)    // for suhmo_step.hip
{
    const DV &v = L->d[depth].v;
    if (!(L->ex && (v.ext[0] || v.ext[1]))) return 0;
    for (int k = 0; k < n; k++) if (!suhmo_field(L, depth, fields[k])) return -2;
    int rc = L->ex(L->user, L, depth, fields, n, (suhmo_stream_t)st);
    if (!rc) for (int k = 0; k < n; k++) if (fields[k] == SUHMO_F_PHI) L->d[depth].phi_fresh = suhmo_halo_rows(v);
    for (int k = 0; k < n; k++) if (fields[k] == SUHMO_F_MASK) suhmo_mask_halo_written(L);
    for (int k = 0; k < n; k++) if (fields[k] == SUHMO_F_ZB) suhmo_zb_written(L);
    return rc;
}
// strips: make sure `need` halo rows of phi hold the neighbours' current values.  Every kernel that
// changes phi lowers Depth::phi_fresh (a colour pass that also advances the halo rows redundantly loses
// one row, a K-sweep fused launch 2K), so an exchange happens only when the stencil about to run would
// reach stale rows -- LevelData::exchange of the reference (src/VCAMRNonLinearPoissonOp.cpp:47,124,304,405,692)
int suhmo_ensure_phi_halo(suhmo_level *L, int depth, int need, hipStream_t st)
{
    Depth &D = L->d[depth];
    if (!(L->ex && (D.v.ext[0] || D.v.ext[1]))) return 0;
    if (D.phi_fresh >= need) return 0;
    return suhmo_exchange_fields(L, depth, {SUHMO_F_PHI}, st);
}

extern "C" int suhmo_level_apply_op(suhmo_level_t *L, int depth, int homogeneous, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::applyOpI");
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_LPHI)) return -2;
    int rc = suhmo_ensure_phi_halo(L, depth, 1, (hipStream_t)s); if (rc) return rc;
    return launch_apply<0>(on_level(L, depth), D.v.alpha != 0.0, homogeneous, (hipStream_t)s);
}

// applyOpI (inhomogeneous) and the residual of it in one pass: LPHI = L(phi), RES = rhs - L(phi)
int suhmo_apply_and_residual(suhmo_level *L, int depth, hipStream_t st)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::applyOpI");
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_LPHI) || !suhmo_field(L, depth, SUHMO_F_RES)) return -2;
    int rc = suhmo_ensure_phi_halo(L, depth, 1, st); if (rc) return rc;
    return launch_apply<3>(on_level(L, depth), D.v.alpha != 0.0, 0, st);
}

int suhmo_apply_and_residual_rects(suhmo_level *L, int depth, const int4 *d_rects, int n, int maxw, int maxh, hipStream_t st)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::applyOpI");
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_LPHI) || !suhmo_field(L, depth, SUHMO_F_RES)) return -2;
    int rc = suhmo_ensure_phi_halo(L, depth, 1, st); if (rc) return rc;
    if (!n) return 0;
    dim3 grd((maxw + 63) / 64, (maxh + 3) / 4, n);
    if (D.v.alpha != 0.0) hipLaunchKernelGGL((k_apply_rects<true>), grd, BLK2D, 0, st, D.v, D.fp, L->ph, d_rects);
    else hipLaunchKernelGGL((k_apply_rects<false>), grd, BLK2D, 0, st, D.v, D.fp, L->ph, d_rects);
    HIPCHK(hipGetLastError());
    return 0;
}

// FAS cycle, coarse depth after the restriction: rhs_c = res_c + L_c(R phi) and the copy of R phi the prolongation
// subtracts (on a rank strip with its exchanged halo rows), one pass instead of applyOp + axby + a device copy
int suhmo_fas_coarse_rhs(suhmo_level *L, int depth, hipStream_t st, int hcomp)
{
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_LPHI) || !suhmo_field(L, depth, SUHMO_F_PHIOLD)) return -2;
    const int halo = (D.v.ext[0] || D.v.ext[1]) ? D.v.gy : 0;
    return launch_apply<2>(on_level(L, depth), D.v.alpha != 0.0, 0, st, halo, hcomp);
}

extern "C" int suhmo_level_residual(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::residualI");
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    int rc = suhmo_ensure_phi_halo(L, depth, 1, (hipStream_t)s); if (rc) return rc;
    return launch_apply<1>(on_level(L, depth), D.v.alpha != 0.0, 0, (hipStream_t)s);
}

// COMPUTENONLINEARTERMS / lambda as stand-alone kernels (parity of a2, a9)
__global__ void k_nonlinear(DV v, FP fp, suhmo_phys_t ph)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int idx = cidx(v, i, j);
    double nl, dnl;
    nl_terms(ph, fp.f[SUHMO_F_PHI][idx], fp.f[SUHMO_F_B][idx], fp.f[SUHMO_F_PI][idx], fp.f[SUHMO_F_ZB][idx], fp.f[SUHMO_F_MASK][idx], nl, dnl);
    fp.f[SUHMO_F_NL][idx] = nl; fp.f[SUHMO_F_DNL][idx] = dnl;
}
__global__ void k_lambda(DV v, FP fp)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int idx = cidx(v, i, j);
    double aterm = fp.f[SUHMO_F_ACOEF][idx] * v.alpha;
    fp.f[SUHMO_F_LAMBDA][idx] = lambda_cell(v, aterm, fp.f[SUHMO_F_BX][idx + 1], fp.f[SUHMO_F_BX][idx],
                                            fp.f[SUHMO_F_BY][idx + v.P], fp.f[SUHMO_F_BY][idx]);
}
extern "C" int suhmo_level_nonlinear(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_NL) || !suhmo_field(L, depth, SUHMO_F_DNL)) return -2;
    hipLaunchKernelGGL(k_nonlinear, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp, L->ph);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int suhmo_level_compute_lambda(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_LAMBDA)) return -2;
    hipLaunchKernelGGL(k_lambda, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int suhmo_level_gsrb(suhmo_level_t *L, int depth, int sweeps, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::levelGSRB");
    ARG(L); ARG(depth >= 0 && depth < L->ndepth); ARG(sweeps >= 0);
    HIPCHK(hipSetDevice(L->device));
    int rc = suhmo_launch_gsrb(L, depth, sweeps, 0, (hipStream_t)s);
    if (rc) return rc;
    // levelGSRB leaves the ghosts with the HOMOGENEOUS BC applied (:757-759)
    if (sweeps > 0) return suhmo_level_fill_ghosts(L, depth, SUHMO_F_PHI, 1, s);
    return 0;
}

// RESTRICTRESVCNL2D (src/VCAMRNonLinearPoissonOpF.ChF:516-558) fused with BC + NL: one thread
// per coarse cell; the four fine contributions are accumulated in the reference's loop order
// (2I,2J), (2I+1,2J), (2I,2J+1), (2I+1,2J+1) onto a zero-initialised coarse value.
template <bool HAS_ALPHA>
__device__ __forceinline__ void d_restrict_residual(const DV &v, const FP &fp, const DV &vc, double *__restrict__ resC, double *__restrict__ phiC, const suhmo_phys_t &ph)
{
    int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= vc.nx || J >= vc.ny) return;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    // the thread's 2 x 2 fine cells start at an even column: every row is read as 16-byte pairs (canvas column
    // SUHMO_XOFF + 2I is 16-byte aligned), the W / E neighbours of the pair as single values
    const int i0 = 2 * I, j0 = 2 * J, base = cidx(v, i0, j0);
    auto ld2 = [&](const double *__restrict__ p, int idx) { return *reinterpret_cast<const double2 *>(p + idx); };
    double2 pc[2], pS, pN;
    pc[0] = ld2(phi, base); pc[1] = ld2(phi, base + v.P);
    // south of row j0 / north of row j0 + 1 (physical BC evaluated from the adjacent interior value)
    if (j0 > 0 || v.ext[0]) pS = ld2(phi, base - v.P);
    else if (v.per[1]) pS = ld2(phi, base + (v.ny - 1) * v.P);
    else { pS.x = phiS(v, phi, base, j0, pc[0].x, false); pS.y = phiS(v, phi, base + 1, j0, pc[0].y, false); }
    if (j0 + 1 < v.ny - 1 || v.ext[1]) pN = ld2(phi, base + 2 * v.P);
    else if (v.per[1]) pN = ld2(phi, base + v.P - (v.ny - 1) * v.P);
    else { pN.x = phiN(v, phi, base + v.P, j0 + 1, pc[1].x, false); pN.y = phiN(v, phi, base + v.P + 1, j0 + 1, pc[1].y, false); }
    double acc = 0.0, accp = 0.0;      // accp: RESTRICTVCNL of phi (restrictR), same visiting order
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int j = j0 + b, idx = base + b * v.P;
        const double2 cc = pc[b];
        const double w0 = phiW(v, phi, idx, i0, cc.x, false), e1 = phiE(v, phi, idx + 1, i0 + 1, cc.y, false);
        const double2 sS = b == 0 ? pS : pc[0], nN = b == 0 ? pc[1] : pN;
        const double2 bx01 = ld2(fp.f[SUHMO_F_BX], idx); const double bx2 = fp.f[SUHMO_F_BX][idx + 2];
        const double2 byS = ld2(fp.f[SUHMO_F_BY], idx), byN = ld2(fp.f[SUHMO_F_BY], idx + v.P);
        const double2 B2 = ld2(fp.f[SUHMO_F_B], idx), Pi2 = ld2(fp.f[SUHMO_F_PI], idx), zb2 = ld2(fp.f[SUHMO_F_ZB], idx), mk2 = ld2(fp.f[SUHMO_F_MASK], idx);
        const double2 rhs2 = ld2(fp.f[SUHMO_F_RHS], idx);
        double2 a2 = make_double2(0.0, 0.0);
        if (HAS_ALPHA) a2 = ld2(fp.f[SUHMO_F_ACOEF], idx);
        (void)j;
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const double c = a ? cc.y : cc.x, w = a ? cc.x : w0, e = a ? e1 : cc.y;
            const double n = a ? nN.y : nN.x, s_ = a ? sS.y : sS.x;
            const double bxW = a ? bx01.y : bx01.x, bxE = a ? bx2 : bx01.y;
            double nl, dnl;
            nl_terms(ph, c, a ? B2.y : B2.x, a ? Pi2.y : Pi2.x, a ? zb2.y : zb2.x, a ? mk2.y : mk2.x, nl, dnl);
            double aterm = HAS_ALPHA ? v.alpha * (a ? a2.y : a2.x) : v.alpha;
            double lofphi = lofphi_cell(v, aterm, c, e, w, n, s_, bxE, bxW, a ? byN.y : byN.x, a ? byS.y : byS.x, nl);
            acc = acc + ((a ? rhs2.y : rhs2.x) - lofphi) / 4.0;
            accp = accp + c / 4.0;
        }
    }
    resC[cidx(vc, I, J)] = acc;
    if (phiC) phiC[cidx(vc, I, J)] = accp;
}
template <class T, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void k_restrict_residual(T c, T f, int also_phi)      // RES (and PHI) of the coarse depth c
{
    const FP &fc = c.fields();
    d_restrict_residual<HAS_ALPHA>(f.view(), f.fields(), c.view(), fc.f[SUHMO_F_RES], also_phi ? fc.f[SUHMO_F_PHI] : nullptr, f.phys());
}
template <class T> int launch_restrict(const T &f, const T &c, bool also_phi, bool has_alpha, hipStream_t st)
{
    if (has_alpha) return launch_over(k_restrict_residual<T, true>, c, CELLS, st, f, (int)also_phi);
    return launch_over(k_restrict_residual<T, false>, c, CELLS, st, f, (int)also_phi);
}
template int launch_restrict(const OnMembers &, const OnMembers &, bool, bool, hipStream_t);

static int restrict_residual_impl(suhmo_level *L, int depth, bool also_phi, hipStream_t st)
{
    int rc = suhmo_ensure_phi_halo(L, depth, 1, st); if (rc) return rc;
    if (also_phi) phi_changed(L, depth + 1);
    return launch_restrict(on_level(L, depth), on_level(L, depth + 1), also_phi, L->d[depth].v.alpha != 0.0, st);
}
extern "C" int suhmo_level_restrict_residual(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::restrictResidual");
    ARG(L); ARG(depth >= 0 && depth + 1 < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    return restrict_residual_impl(L, depth, false, (hipStream_t)s);
}
// restrictResidual + restrictR of the FAS cycle in one pass over the fine level
int suhmo_restrict_both(suhmo_level *L, int depth, hipStream_t st) { return restrict_residual_impl(L, depth, true, st); }

// RESTRICTVCNL (src/VCAMRNonLinearPoissonOpF.ChF:432-446)
__global__ void k_restrict_r(DV v, const double *__restrict__ f, DV vc, double *__restrict__ c)
{
    int I = blockIdx.x * blockDim.x + threadIdx.x, J = blockIdx.y * blockDim.y + threadIdx.y;
    if (I >= vc.nx || J >= vc.ny) return;
    int idx = cidx(v, 2 * I, 2 * J);
    double acc = 0.0;
    acc = acc + f[idx] / 4.0;
    acc = acc + f[idx + 1] / 4.0;
    acc = acc + f[idx + v.P] / 4.0;
    acc = acc + f[idx + v.P + 1] / 4.0;
    c[cidx(vc, I, J)] = acc;
}
extern "C" int suhmo_level_restrict_r(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    ARG(L); ARG(depth >= 0 && depth + 1 < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth], &C = L->d[depth + 1];
    phi_changed(L, depth + 1);
    hipLaunchKernelGGL(k_restrict_r, grid2d(C.v.nx, C.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp.f[SUHMO_F_PHI], C.v, C.fp.f[SUHMO_F_PHI]);
    HIPCHK(hipGetLastError());
    return 0;
}

// PROLONGNL (src/AMRNonLinearPoissonOpF.ChF:617-628), m = 2
__global__ void k_prolong(DV v, double *__restrict__ phi, DV vc, const double *__restrict__ c)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int idx = cidx(v, i, j);
    phi[idx] = phi[idx] + c[cidx(vc, i / 2, j / 2)];
}
extern "C" int suhmo_level_prolong_increment(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    SUHMO_TIME("AMRNonLinearPoissonOp::prolongIncrement");
    ARG(L); ARG(depth >= 0 && depth + 1 < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth], &C = L->d[depth + 1];
    phi_changed(L, depth);
    hipLaunchKernelGGL(k_prolong, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp.f[SUHMO_F_PHI], C.v, C.fp.f[SUHMO_F_CORR]);
    HIPCHK(hipGetLastError());
    return 0;
}

// FAS correction of the cycle: CORR_c = 1*phi_c + (-1)*phi_c,old (LevelDataOps::axby), phi += P(CORR_c) (PROLONGNL).
// On rank strips both kernels also cover the halo rows that are valid on BOTH depths (fine: phi_fresh rows, coarse:
// phi_fresh rows of phi_c; PHIOLD was copied after the exchange), so the post-smoothing can start without an exchange.
__device__ __forceinline__ void d_axby_rows(const DV &v, double *__restrict__ dst, const double *__restrict__ x, const double *__restrict__ y, double a, double b, int jlo, int jhi)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = jlo + (int)(blockIdx.y * blockDim.y + threadIdx.y);
    if (i >= v.nx || j > jhi) return;
    int idx = cidx(v, i, j);
    dst[idx] = a * x[idx] + b * y[idx];
}
__device__ __forceinline__ void d_prolong_rows(const DV &v, double *__restrict__ phi, const DV &vc, const double *__restrict__ c, int jlo, int jhi)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = jlo + (int)(blockIdx.y * blockDim.y + threadIdx.y);
    if (i >= v.nx || j > jhi) return;
    int idx = cidx(v, i, j);
    phi[idx] = phi[idx] + c[cidx(vc, i / 2, j >> 1)];          // j >> 1: floor, halo rows have j < 0
}
// rows [-lo, ny - 1 + hi] of the target (lo, hi: halo rows below / above)
template <class T> __global__ void k_axby_rows(T t, int fd, int fx, int fy, double a, double b, int lo, int hi)
{
    const DV v = t.view();
    d_axby_rows(v, t.field(fd), t.field(fx), t.field(fy), a, b, -lo, v.ny - 1 + hi);
}
template <class T> __global__ void k_prolong_rows(T f, T c, int lo, int hi)
{
    const DV v = f.view();
    d_prolong_rows(v, f.fields().f[SUHMO_F_PHI], c.view(), c.fields().f[SUHMO_F_CORR], -lo, v.ny - 1 + hi);
}
// CORR_c = phi_c - phi_c,old over lo_c / hi_c halo rows, phi += P(CORR_c) over lo / hi
template <class T> int launch_prolong(const T &f, const T &c, int lo, int hi, int lo_c, int hi_c, hipStream_t st)
{
    int rc = launch_grid(k_axby_rows<T>, c, grid2d(c.nx(), c.ny() + lo_c + hi_c), BLK2D, st, (int)SUHMO_F_CORR, (int)SUHMO_F_PHI, (int)SUHMO_F_PHIOLD, 1.0, -1.0, lo_c, hi_c);
    return rc ? rc : launch_grid(k_prolong_rows<T>, f, grid2d(f.nx(), f.ny() + lo + hi), BLK2D, st, c, lo, hi);
}
template int launch_prolong(const OnMembers &, const OnMembers &, int, int, int, int, hipStream_t);
int suhmo_prolong_with_halo(suhmo_level *L, int depth, hipStream_t st)
{
    Depth &D = L->d[depth], &C = L->d[depth + 1];
    const bool ext = L->ex && (D.v.ext[0] || D.v.ext[1]);
    int R = 0;                                              // fine halo rows that stay valid through the prolongation
    if (ext) { R = D.phi_fresh < 2 * C.phi_fresh ? D.phi_fresh : 2 * C.phi_fresh; R &= ~1; }
    const int Rc = R / 2;
    const int jlo = D.v.ext[0] ? -R : 0, jhi = D.v.ny - 1 + (D.v.ext[1] ? R : 0);
    const int cjlo = C.v.ext[0] ? -Rc : 0, cjhi = C.v.ny - 1 + (C.v.ext[1] ? Rc : 0);
    if (!suhmo_field(L, depth + 1, SUHMO_F_CORR)) return -2;
    int rc = launch_prolong(on_level(L, depth), on_level(L, depth + 1), -jlo, jhi - (D.v.ny - 1), -cjlo, cjhi - (C.v.ny - 1), st);
    if (rc) return rc;
    D.phi_fresh = R;
    if (ext) L->strip_prolong_unfused++;
    return 0;
}

// PROLONG_2_NL (suhmo_transfer.h: prolong2_nl), coarse data read with its stored ghosts
__global__ void k_prolong2(DV v, double *__restrict__ phi, DV vc, const double *__restrict__ c)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int ic = i / 2, jc = j / 2, o1 = 2 * (i % 2) - 1, o2 = 2 * (j % 2) - 1;
    int idx = cidx(v, i, j), cc = cidx(vc, ic, jc);
    phi[idx] = prolong2_nl(phi[idx], c[cc], c[cc + o1], c[cc + o2 * vc.P], c[cc + o1 + o2 * vc.P]);
}
extern "C" int suhmo_level_prolong_bilinear(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    ARG(L); ARG(depth >= 0 && depth + 1 < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth], &C = L->d[depth + 1];
    phi_changed(L, depth);
    hipLaunchKernelGGL(k_prolong2, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp.f[SUHMO_F_PHI], C.v, C.fp.f[SUHMO_F_CORR]);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ small operators
// DIVERGENCE (util/DivergenceF.ChF:38-54), called for dir 0 then dir 1
__global__ void k_divergence(DV v, const double *__restrict__ ux, const double *__restrict__ uy, double *__restrict__ div)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int idx = cidx(v, i, j);
    double d = div[idx];
    d = d + v.fdx * (ux[idx + 1] - ux[idx]);
    d = d + v.fdy * (uy[idx + v.P] - uy[idx]);
    div[idx] = d;
}
extern "C" int suhmo_level_divergence(suhmo_level_t *L, int depth, int dst_field, suhmo_stream_t s)
{
    CHECK_DF(L, depth, dst_field); ARG(!is_face(dst_field));
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    double *dst = suhmo_field(L, depth, dst_field);
    if (dst_field == SUHMO_F_MASK) suhmo_mask_written(L);
    if (dst_field == SUHMO_F_ZB) suhmo_zb_written(L);
    hipLaunchKernelGGL(k_divergence, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, D.fp.f[SUHMO_F_BX], D.fp.f[SUHMO_F_BY], dst);
    HIPCHK(hipGetLastError());
    return 0;
}

// getFlux (src/VCAMRNonLinearPoissonOp.cpp:820-840): F = -b * ((phi_hi - phi_lo) * (beta*ref/dx))
__global__ void k_getflux(DV v, FP fp, int dir, double scale, double *__restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    int nxf = dir == 0 ? v.nx + 1 : v.nx, nyf = dir == 0 ? v.ny : v.ny + 1;
    if (i >= nxf || j >= nyf) return;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    int idx = cidx(v, i, j);
    double phihi = phi[idx], philo = dir == 0 ? phi[idx - 1] : phi[idx - v.P];   // stored ghosts
    double gradphi = (phihi - philo) * scale;
    out[(size_t)j * nxf + i] = -fp.f[dir == 0 ? SUHMO_F_BX : SUHMO_F_BY][idx] * gradphi;
}
extern "C" int suhmo_level_get_flux(suhmo_level_t *L, int depth, int dir, int ref, double *flux_host, suhmo_stream_t s)
{
    ARG(L); ARG(depth >= 0 && depth < L->ndepth); ARG(dir == 0 || dir == 1); ARG(flux_host);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    Depth &D = L->d[depth];
    int rc = suhmo_level_fill_ghosts(L, depth, SUHMO_F_PHI, 0, s); if (rc) return rc;
    int nxf = dir == 0 ? D.v.nx + 1 : D.v.nx, nyf = dir == 0 ? D.v.ny : D.v.ny + 1;
    double *tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, (size_t)nxf * nyf * 8));
    double scale = D.v.beta * ref / (dir == 0 ? D.v.dx : D.v.dy);
    hipLaunchKernelGGL(k_getflux, grid2d(nxf, nyf), BLK2D, 0, st, D.v, D.fp, dir, scale, tmp);
    HIPCHK(hipMemcpyAsync(flux_host, tmp, (size_t)nxf * nyf * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipFree(tmp));
    return 0;
}

// LevelDataOps::axby / setVal on valid cells
__device__ __forceinline__ void d_axby(const DV &v, double *__restrict__ dst, const double *__restrict__ x, const double *__restrict__ y, double a, double b)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    int idx = cidx(v, i, j);
    dst[idx] = a * x[idx] + b * y[idx];
}
template <class T> __global__ void k_axby(T t, int fd, int fx, int fy, double a, double b)
{
    d_axby(t.view(), t.field(fd), t.field(fx), t.field(fy), a, b);
}
template <class T> int launch_axby(const T &t, int fd, int fx, int fy, double a, double b, hipStream_t st) { return launch_over(k_axby<T>, t, CELLS, st, fd, fx, fy, a, b); }
template int launch_axby(const OnBoxes &, int, int, int, double, double, hipStream_t);
__global__ void k_setval(DV v, double *__restrict__ dst, double val)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    dst[cidx(v, i, j)] = val;
}
extern "C" int suhmo_level_axby(suhmo_level_t *L, int depth, int dst, int x, int y, double a, double b, suhmo_stream_t s)
{
    CHECK_DF(L, depth, dst); CHECK_DF(L, depth, x); CHECK_DF(L, depth, y);
    HIPCHK(hipSetDevice(L->device));
    if (!suhmo_field(L, depth, dst) || !suhmo_field(L, depth, x) || !suhmo_field(L, depth, y)) return -2;
    if (dst == SUHMO_F_PHI) phi_changed(L, depth);
    if (dst == SUHMO_F_ZB) suhmo_zb_written(L);
    if (dst == SUHMO_F_MASK) suhmo_mask_written(L);      // (the reports about the ice mask end with any write to it)
    return launch_axby(on_level(L, depth), dst, x, y, a, b, (hipStream_t)s);
}
extern "C" int suhmo_level_set_value(suhmo_level_t *L, int depth, int field, double val, suhmo_stream_t s)
{
    CHECK_DF(L, depth, field);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[depth];
    if (field == SUHMO_F_PHI) phi_changed(L, depth);
    if (field == SUHMO_F_MASK) suhmo_mask_written(L);
    if (field == SUHMO_F_ZB) suhmo_zb_written(L);
    hipLaunchKernelGGL(k_setval, grid2d(D.v.nx, D.v.ny), BLK2D, 0, (hipStream_t)s, D.v, suhmo_field(L, depth, field), val);
    HIPCHK(hipGetLastError());
    return 0;
}

// norms and the dot product over valid cells: the first stages of suhmo_reduce.h (the order of a sum: there), one partial per workgroup.
// max |x| of a field, the composite norm's covered cells zeroed on the way where `cover` is given (AMRNorm zeroes them,
// src/AMRNonLinearPoissonOp.cpp:1241-1258)
__device__ __forceinline__ void d_norm_max(const DV &v, double *__restrict__ x, const double *__restrict__ cover, double *__restrict__ out)
{
    reduce_cells<RedMax>(v, out, [&](int i, int j, double (&a)[1]) {
        const int idx = cidx(v, i, j);
        if (cover && cover[idx] != 0.0) x[idx] = 0.0; else a[0] = fmax(a[0], fabs(x[idx]));
    });
}
// (a level, the boxes of a level: a level's own workgroups per box, its partial maxima one after the other)
template <class T, bool COVER> __global__ __launch_bounds__(256) void k_norm_partial(T t, double *__restrict__ partial, int field)
{
    d_norm_max(t.view(), t.field(field), COVER ? t.field(SUHMO_F_COVER) : nullptr, partial + t.slot((size_t)gridDim.x * gridDim.y) + plane_block());
}
__global__ __launch_bounds__(256) void k_norm2_partial(OnLevel t, double *__restrict__ partial, int field)
{
    const DV &v = t.view();
    const double *__restrict__ x = t.field(field);
    reduce_cells<RedSum>(v, partial + plane_block(), [&](int i, int j, double (&a)[1]) { const double val = x[cidx(v, i, j)]; a[0] += val * val; });
}
__global__ __launch_bounds__(256) void k_dot_partial(OnLevel t, double *__restrict__ partial, int fx, int fy)
{
    const DV &v = t.view();
    const double *__restrict__ x = t.field(fx), *__restrict__ y = t.field(fy);
    reduce_cells<RedSum>(v, partial + plane_block(), [&](int i, int j, double (&a)[1]) { const int idx = cidx(v, i, j); a[0] += x[idx] * y[idx]; });
}
// The 8-byte result of a reduction.  Synchronising the stream costs ~17 us of idle GPU per read-back on this platform (the copy
// kernel, the interrupt, the wake-up); instead the reduction's last kernel stores the value and then, with a system-scope release,
// a sequence number into pinned coherent host memory, and the host spins on the number.  In-order stream: when the number is
// there, everything enqueued before is done.  A kernel that never publishes (a fault) ends in the stream synchronisation below,
// which reports it.
HostSlot suhmo_host_slot(suhmo_level *L)
{
    HostSlot h{nullptr, nullptr, 0};
    if (L->poll_readback) { h.val = L->hscratch_dev; h.flag = (unsigned long long *)(L->hscratch_dev + 8); h.seq = ++L->hseq; }
    return h;
}
int suhmo_readback(suhmo_level *L, hipStream_t st, double *out, double *out2)
{
    if (L->poll_readback) {
        HIPCHK(hipGetLastError());
        volatile unsigned long long *flag = (volatile unsigned long long *)(L->hscratch + 8);
        for (long spin = 0; spin < 400000000L; spin++) {
            if (__atomic_load_n((unsigned long long *)flag, __ATOMIC_ACQUIRE) == L->hseq) { *out = L->hscratch[0]; if (out2) *out2 = L->hscratch[1]; return 0; }
            if ((spin & 0xffff) == 0xffff && hipStreamQuery(st) == hipSuccess) break;     // finished without us seeing the store: read below
        }
        HIPCHK(hipStreamSynchronize(st));
        if (__atomic_load_n((unsigned long long *)flag, __ATOMIC_ACQUIRE) == L->hseq) { *out = L->hscratch[0]; if (out2) *out2 = L->hscratch[1]; return 0; }
        // not published (mapping not coherent on this system): fall back for good
        L->poll_readback = 0;
    }
    HIPCHK(hipMemcpyAsync(L->hscratch, L->scratch, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = L->hscratch[0];
    if (out2) *out2 = L->hscratch[1];
    return 0;
}
__global__ void k_publish2(const double *__restrict__ v, HostSlot hs)
{
    if (hs.val) hs.val[1] = v[1];
    suhmo_publish(hs, v[0]);
}
HostSlot suhmo_reduce_slot(suhmo_level *L)
{
    if (on_strip(L) && L->ard) return HostSlot{nullptr, nullptr, 0};       // published after the device all-reduce
    return suhmo_host_slot(L);
}
int suhmo_reduce_finish(suhmo_level *L, hipStream_t st, int n, int op, double *out, double *out2)
{
    ARG(n == 1 || n == 2);
    double v[2] = {0.0, 0.0};
    int rc;
    if (on_strip(L) && L->ard) {
        if ((rc = L->ard(L->user, L->scratch, n, op, (suhmo_stream_t)st))) return rc;
        hipLaunchKernelGGL(k_publish2, dim3(1), dim3(1), 0, st, L->scratch, suhmo_host_slot(L));
        HIPCHK(hipGetLastError());
        if ((rc = suhmo_readback(L, st, &v[0], &v[1]))) return rc;
    } else {
        if ((rc = suhmo_readback(L, st, &v[0], &v[1]))) return rc;
        if (on_strip(L) && (L->ar || L->ar2)) {
            if (L->ar2) { if ((rc = L->ar2(L->user, v, n, op))) return rc; }
            else if (op == 0) { for (int k = 0; k < n; k++) if ((rc = L->ar(L->user, &v[k]))) return rc; }
            else { suhmo_set_error("a SUM over the ranks of a strip needs suhmo_level_set_reduce_hook or the native transport (the hook of suhmo_level_set_hooks reduces MAX only)"); return -5; }
        }
    }
    *out = v[0];
    if (out2) *out2 = v[1];
    return 0;
}
extern "C" int suhmo_level_dot(suhmo_level_t *L, int depth, int x, int y, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("AMRNonLinearPoissonOp::dotProduct");
    CHECK_DF(L, depth, x); CHECK_DF(L, depth, y); ARG(out);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    if (!suhmo_field(L, depth, x) || !suhmo_field(L, depth, y)) { suhmo_set_error("field allocation failed"); return -2; }
    int rc = launch_reduction<RedSum>(k_dot_partial, on_level(L, depth), CAP_LEVEL, L->scratch + 2, L->scratch, suhmo_reduce_slot(L), st, x, y);
    return rc ? rc : suhmo_reduce_finish(L, st, 1, 1, out);
}
extern "C" int suhmo_level_norm(suhmo_level_t *L, int depth, int field, int ord, double *out, suhmo_stream_t s)
{
    SUHMO_TIME("AMRNonLinearPoissonOp::norm");
    CHECK_DF(L, depth, field); ARG(out); ARG(ord == 0 || ord == 2);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    if (!suhmo_field(L, depth, field)) { suhmo_set_error("field allocation failed"); return -2; }
    const OnLevel t = on_level(L, depth);
    int rc = ord == 0 ? launch_reduction<RedMax>(k_norm_partial<OnLevel, false>, t, CAP_LEVEL, L->scratch + 2, L->scratch, suhmo_reduce_slot(L), st, field)
                      : launch_reduction<RedSum>(k_norm2_partial, t, CAP_LEVEL, L->scratch + 2, L->scratch, suhmo_reduce_slot(L), st, field);
    if (rc) return rc;
    double r = 0.0;
    // the reference's norm() reduces over the ranks (src/AMRNonLinearPoissonOp.cpp:1222-1264): MAX for the max norm, SUM of the squares for l2
    if ((rc = suhmo_reduce_finish(L, st, 1, ord == 0 ? 0 : 1, &r))) return rc;
    if (ord == 2) r = sqrt(r);
    *out = r;
    return 0;
}

// residualI of depth 0 and the max norm of the result in two launches instead of three (levels of up to scratch-many workgroups)
int suhmo_level_residual_and_norm(suhmo_level *L, double *out, hipStream_t st)
{
    Depth &D = L->d[0];
    const dim3 grd = grid2d(D.v.nx, D.v.ny);
    const size_t np = (size_t)grd.x * grd.y;
    int rc;
    if (np + 4 >= L->scratch_elems) {
        if ((rc = suhmo_level_residual(L, 0, (suhmo_stream_t)st))) return rc;
        return suhmo_level_norm(L, 0, SUHMO_F_RES, 0, out, (suhmo_stream_t)st);
    }
    if ((rc = suhmo_ensure_phi_halo(L, 0, 1, st))) return rc;
    if ((rc = launch_residual_norm(on_level(L, 0), D.v.alpha != 0.0, L->scratch + 2, st))) return rc;
    return suhmo_level_norm_from_partials(L, (int)np, out, st);
}
// max norm of RES at depth 0 from the partial maxima the cycle's last launch left behind (suhmo_gsrb.hip, residual output): the second
// stage of suhmo_level_norm alone
int suhmo_level_norm_from_partials(suhmo_level *L, int np, double *out, hipStream_t st)
{
    double r = 0.0;
    int rc = launch_final<RedMax>(one_list(L->scratch + 2, np), L->scratch, suhmo_reduce_slot(L), st);
    if (rc || (rc = suhmo_reduce_finish(L, st, 1, 0, &r))) return rc;
    *out = r;
    return 0;
}

// ------------------------------------------------------------------ every box of a multi-box AMR level in one launch
__global__ void k_copy(OnBoxes t, int fd, int fs)
{
    const DV &v = t.view();
    const FP &f = t.fields();
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    int idx = cidx(v, i, j);
    f.f[fd][idx] = f.f[fs][idx];
}
// A level of boxes entering / leaving its FAS problem in an AMR V-cycle (suhmo_hier.hip:vcycle_amr), one launch each instead of three / two:
//   enter: RHS0 <- RHS (copy, ghost ring included), RHS <- 1 RES + 1 LPHI (axby, valid cells), PHIOLD <- PHI (copy)
//   leave: RHS <- RHS0 (copy), CORR <- 1 PHI + (-1) PHIOLD (axby)               -- the expressions of k_copy / k_axby on the same operands
__global__ void k_fas_enter(OnBoxes t)
{
    const DV &v = t.view();
    const FP &f = t.fields();
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    int idx = cidx(v, i, j);
    f.f[SUHMO_F_RHS0][idx] = f.f[SUHMO_F_RHS][idx];
    f.f[SUHMO_F_PHIOLD][idx] = f.f[SUHMO_F_PHI][idx];
    if (i >= 0 && i < v.nx && j >= 0 && j < v.ny) f.f[SUHMO_F_RHS][idx] = 1.0 * f.f[SUHMO_F_RES][idx] + 1.0 * f.f[SUHMO_F_LPHI][idx];
}
__global__ void k_fas_leave(OnBoxes t)
{
    const DV &v = t.view();
    const FP &f = t.fields();
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    int idx = cidx(v, i, j);
    f.f[SUHMO_F_RHS][idx] = f.f[SUHMO_F_RHS0][idx];
    if (i >= 0 && i < v.nx && j >= 0 && j < v.ny) f.f[SUHMO_F_CORR][idx] = 1.0 * f.f[SUHMO_F_PHI][idx] + -1.0 * f.f[SUHMO_F_PHIOLD][idx];
}
// fields of the boxes of one hierarchy <- fields of the same boxes of another (the implicit gap-height operator's copy of a level)
struct CopyPairs { int n, fd[4], fs[4]; };
__global__ void k_copy_between(OnBoxes src, OnBoxes dst, CopyPairs cp)
{
    const DV &v = src.view();
    const FP &fs = src.fields(), &fd = dst.fields();
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    int idx = cidx(v, i, j);
    for (int q = 0; q < cp.n; q++) fd.f[cp.fd[q]][idx] = fs.f[cp.fs[q]][idx];
}
// mode 0: LPHI, 1: RES, 3: both
int launch_apply_boxes(const OnBoxes &t, bool has_alpha, int mode, hipStream_t st)
{
    return mode == 0 ? launch_apply<0>(t, has_alpha, 0, st) : mode == 1 ? launch_apply<1>(t, has_alpha, 0, st) : launch_apply<3>(t, has_alpha, 0, st);
}
int launch_copy(const OnBoxes &t, int fd, int fs, hipStream_t st) { return launch_over(k_copy, t, GHOSTED, st, fd, fs); }
int launch_fas_enter(const OnBoxes &t, hipStream_t st) { return launch_over(k_fas_enter, t, GHOSTED, st); }
int launch_fas_leave(const OnBoxes &t, hipStream_t st) { return launch_over(k_fas_leave, t, GHOSTED, st); }
int launch_copy_between(const OnBoxes &dst, const OnBoxes &src, const int *fd, const int *fs, int n, hipStream_t st)
{
    if (n < 1 || n > 4 || dst.nbox != src.nbox) { suhmo_set_error("internal: copy between hierarchies"); return -4; }
    CopyPairs cp;
    cp.n = n;
    for (int q = 0; q < n; q++) { cp.fd[q] = fd[q]; cp.fs[q] = fs[q]; }
    return launch_over(k_copy_between, src, GHOSTED, st, dst, cp);
}
// AMRNorm over a hierarchy in ONE read-back: the first stages of level 0 (suhmo_level_norm_max_partials) and of every level of boxes
// (suhmo_multi_norm_max_partials) leave their partial maxima where they always do; one second stage takes the maximum of all the lists
// (a maximum does not care about the order) and publishes it
// (cover: the covered cells of the level are zeroed on the way, SUHMO_F_COVER)
int suhmo_level_norm_max_partials(suhmo_level *L, int field, bool cover, const double **partials, int *np, hipStream_t st)
{
    if (!suhmo_field(L, 0, field) || (cover && !suhmo_field(L, 0, SUHMO_F_COVER))) { suhmo_set_error("field allocation failed"); return -2; }
    *partials = L->scratch + 2;
    return launch_partials(cover ? k_norm_partial<OnLevel, true> : k_norm_partial<OnLevel, false>, on_level(L, 0), CAP_LEVEL, L->scratch + 2, np, st, field);
}
int suhmo_multi_norm_max_partials(const suhmo_multi &m, int field, const double **partials, int *np, hipStream_t st)
{
    *partials = m.red;
    int rc = launch_partials(k_norm_partial<OnBoxes, false>, m.on(), CAP_BOX, m.red, np, st, field);
    *np *= std::max(m.nbox, 0);
    return rc;
}
int suhmo_norm_max_of_lists(suhmo_level *slot, const double *const *partials, const int *np, int cnt, double *out, hipStream_t st)
{
    if (cnt > RED_LISTS) { suhmo_set_error("internal: norm over more lists than levels"); return -4; }
    PartialLists pl;
    pl.cnt = cnt;
    for (int q = 0; q < cnt; q++) { pl.p[q] = partials[q]; pl.n[q] = np[q]; }
    int rc = launch_final<RedMax>(pl, slot->scratch, suhmo_host_slot(slot), st);
    return rc ? rc : suhmo_readback(slot, st, out);
}
// several levels of boxes: lv.mode[q] != 0: the level has cells under a finer one (every level but the finest), they are zeroed on the way
__global__ __launch_bounds__(256) void k_norm_max_cover_lv(suhmo_lvboxes lv, int field, double *__restrict__ partial)
{
    int q, k;
    const int slot = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (!lv_find(lv, q, k)) { if (threadIdx.x == 0 && threadIdx.y == 0) partial[slot] = 0.0; return; }
    const DV *dv = nullptr; const FP *fp = nullptr; int covered = 0;
    LV_PICK(lv, q, dv, dv); LV_PICK(lv, q, fp, fp); LV_PICK(lv, q, mode, covered);
    d_norm_max(dv[k], fp[k].f[field], covered ? fp[k].f[SUHMO_F_COVER] : nullptr, partial + slot);
}
int suhmo_levels_norm_max_cover_partials(const suhmo_lvboxes &lv, int field, double *partial, int *np, hipStream_t st)
{
    int nz = 0;
    for (int q = 0; q < lv.n; q++) nz += lv.nbox[q];
    *np = 0;
    if (nz <= 0) return 0;
    dim3 grd = reduce_grid(lv.maxnx, lv.maxny, CAP_BOX);
    grd.z = nz;
    hipLaunchKernelGGL(k_norm_max_cover_lv, grd, BLK2D, 0, st, lv, field, partial);
    HIPCHK(hipGetLastError());
    *np = (int)(grd.x * grd.y * grd.z);
    return 0;
}


// ------------------------------------------------------------------ every active member of a batch of whole levels in one launch (suhmo_batch.hip)
int launch_fas_coarse_rhs(const OnMembers &t, bool has_alpha, hipStream_t st) { return launch_apply<2>(t, has_alpha, 0, st); }
size_t suhmo_batch_residual_partials(const OnMembers &t) { const dim3 g = grid2d(t.nx(), t.ny()); return (size_t)g.x * g.y; }
int launch_residual_norm_members(const OnMembers &t, bool has_alpha, double *partial, double *slot, unsigned long long *flag, unsigned long long seq, hipStream_t st)
{
    if (t.count() <= 0) return 0;
    int rc = launch_residual_norm(t, has_alpha, partial, st); if (rc) return rc;
    hipLaunchKernelGGL(k_norm_final_members<RedMax>, dim3(1), dim3(256), 0, st, t.sel, partial, (int)suhmo_batch_residual_partials(t), slot, flag, seq);
    HIPCHK(hipGetLastError());
    return 0;
}
__global__ void k_copy_canvas(OnMembers t, int fd, int fs, size_t elems)
{
    const double *__restrict__ src = t.field(fs);
    double *__restrict__ dst = t.field(fd);
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < elems; q += (size_t)gridDim.x * blockDim.x) dst[q] = src[q];
}
int launch_copy_canvas(const OnMembers &t, int fd, int fs, size_t elems, hipStream_t st)
{
    return launch_grid(k_copy_canvas, t, dim3((unsigned)std::min<size_t>((elems + 255) / 256, 256)), dim3(256), st, fd, fs, elems);
}
