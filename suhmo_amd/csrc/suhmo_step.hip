// suhmo_step.hip -- the caller of the head solve, device resident: one AmrHydro::timeStepFAS
// (src/AmrHydro.cpp:2254-3460) on one level (suhmo_level_timestep) or on an AMR hierarchy (suhmo_amr_timestep), each whole
// or cut into rank strips: distributed, time-varying or moulin water input, with or without the diffusive term
// (suhmo.diffFactor), explicit or implicit (solver.use_ImplDiff) gap-height update.  "Next rows" of SURVEY.md 8(f).
//
//   [II]  Picard loop (:2477-3235): ghosts of h and b -> grad h (compute_grad_head :1610-1674) ->
//         Re (evaluate_Re_quadratic :1711-1778) -> Qw on faces (evaluate_Qw_ec :1677-1709, COMPUTEQW)
//         -> Qw.grad(h), Qw.grad(zb) (COMPUTESCAPROD + EdgeToCell :2954-2979) -> melt rate
//         (Calc_meltingRate :2174-2252) -> RHS_h (:3031-3078) -> SolveForHead_nl -> Picard test
//   [III] the same chain with the new head, CalcRHS_gapHeightFAS (:2069-2171), forward Euler (:3406)
// Head = PHI, gap height = B: both stay in HBM across Picard iterations and timesteps; per step
// the host sees two scalars per Picard iteration (max head, max relative change).
// On a rank strip (suhmo_level_desc.j0 / ny_global) the same step runs on every rank: wherever the reference exchanges
// a field (b, mR, grad h, RHS halos for the redundant halo-row relaxation) the strip's exchange hook is called, the
// Picard test is MAX all-reduced; the moulin integrals are evaluated redundantly over the whole domain (analytic
// integrand, no data), so the result does not depend on the partition bit for bit.
#include "suhmo_hier_int.h"
#include "suhmo_batch.h"
#include "suhmo_reduce.h"
#include <cmath>

using namespace hier;

// Qw on x- and y-faces: B_ec, Re_ec by CellToEdge (half*(cell + lower cell)), grad h by NEWMACGRAD
// with the physical BC applied on the fly, COMPUTEQW (src/AmrHydroF.ChF:137-150)
__device__ __forceinline__ double face_grad(const DV &v, const double *__restrict__ phi, const double *__restrict__ mk,
                                            int i, int j, int dir, int hasMask)
{
    // face (i,j) of direction dir lies between cell (i,j) and (i-1,j) / (i,j-1)
    double hi, lo;
    if (dir == 0) {
        if (i < v.nx) { int idx = cidx(v, i, j); hi = phi[idx]; lo = phiW(v, phi, idx, i, hi, false); }
        else { int idx = cidx(v, v.nx - 1, j); lo = phi[idx]; hi = phiE(v, phi, idx, v.nx - 1, lo, false); }
    } else {
        if (j < v.ny) { int idx = cidx(v, i, j); hi = phi[idx]; lo = phiS(v, phi, idx, j, hi, false); }
        else { int idx = cidx(v, i, v.ny - 1); lo = phi[idx]; hi = phiN(v, phi, idx, v.ny - 1, lo, false); }
    }
    double g = (dir == 0 ? v.fdx : v.fdy) * (hi - lo);
    if (hasMask) {
        int idx = cidx(v, i, j), idm = dir == 0 ? idx - 1 : idx - v.P;
        if (mk[idx] < 1e-6 || mk[idm] < 1e-6) g = 0.0;
    }
    return g;
}
// gradient of the bed on a face: plain stored ghosts (zb is caller data over the ghosted level)
__device__ __forceinline__ double face_grad_zb(const DV &v, const double *__restrict__ zb, const double *__restrict__ mk,
                                               int i, int j, int dir, int hasMask)
{
    int idx = cidx(v, i, j), idm = dir == 0 ? idx - 1 : idx - v.P;
    double g = (dir == 0 ? v.fdx : v.fdy) * (zb[idx] - zb[idm]);
    if (hasMask && (mk[idx] < 1e-6 || mk[idm] < 1e-6)) g = 0.0;
    return g;
}

__device__ __forceinline__ void d_qw_faces(const DV &v, const FP &fp, suhmo_phys_t ph)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i > v.nx || j > v.ny) return;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI], *__restrict__ B = fp.f[SUHMO_F_B], *__restrict__ Re = fp.f[SUHMO_F_RE];
    const double *__restrict__ mk = fp.f[SUHMO_F_MASK];
    int idx = cidx(v, i, j);
    if (j < v.ny) {
        double b = 0.5 * (B[idx] + B[idx - 1]), re = 0.5 * (Re[idx] + Re[idx - 1]);
        double g = face_grad(v, phi, mk, i, j, 0, ph.use_mask_gradients);
        double num_q = -(b * b * b * ph.grav * g);
        double denom_q = 12.0 * ph.nu * (1.0 + ph.omega * re);
        fp.f[SUHMO_F_QWX][idx] = num_q / denom_q;
    }
    if (i < v.nx) {
        double b = 0.5 * (B[idx] + B[idx - v.P]), re = 0.5 * (Re[idx] + Re[idx - v.P]);
        double g = face_grad(v, phi, mk, i, j, 1, ph.use_mask_gradients);
        double num_q = -(b * b * b * ph.grav * g);
        double denom_q = 12.0 * ph.nu * (1.0 + ph.omega * re);
        fp.f[SUHMO_F_QWY][idx] = num_q / denom_q;
    }
}
template <class T> __global__ __launch_bounds__(256) void k_qw_faces(T t) { d_qw_faces(t.view(), t.fields(), t.phys()); }
template <class T> static int launch_qw_faces(const T &t, hipStream_t st) { return launch_over(k_qw_faces<T>, t, FACES, st); }

// MODE 0: melt rate + RHS_h (Picard iteration).  MODE 1: melt rate + gap-height RHS + forward Euler.
template <int MODE>
__device__ __forceinline__ void d_melt(const DV &v, const FP &fp, suhmo_phys_t ph, suhmo_model_params_t mp, double dt)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI], *__restrict__ zb = fp.f[SUHMO_F_ZB], *__restrict__ mk = fp.f[SUHMO_F_MASK];
    const double *__restrict__ qx = fp.f[SUHMO_F_QWX], *__restrict__ qy = fp.f[SUHMO_F_QWY];
    const int idx = cidx(v, i, j), hm = ph.use_mask_gradients;
    // COMPUTESCAPROD on the four faces of the cell, EdgeToCell
    double t1w = qx[idx] * face_grad(v, phi, mk, i, j, 0, hm), t1e = qx[idx + 1] * face_grad(v, phi, mk, i + 1, j, 0, hm);
    double t1s = qy[idx] * face_grad(v, phi, mk, i, j, 1, hm), t1n = qy[idx + v.P] * face_grad(v, phi, mk, i, j + 1, 1, hm);
    double t2w = qx[idx] * face_grad_zb(v, zb, mk, i, j, 0, hm), t2e = qx[idx + 1] * face_grad_zb(v, zb, mk, i + 1, j, 0, hm);
    double t2s = qy[idx] * face_grad_zb(v, zb, mk, i, j, 1, hm), t2n = qy[idx + v.P] * face_grad_zb(v, zb, mk, i, j + 1, 1, hm);
    double t0 = 0.5 * (t1w + t1e), t1 = 0.5 * (t1s + t1n), u0 = 0.5 * (t2w + t2e), u1 = 0.5 * (t2s + t2n);
    // Calc_meltingRate (src/AmrHydro.cpp:2210-2244)
    const double h = phi[idx], b = fp.f[SUHMO_F_B][idx], Pi = fp.f[SUHMO_F_PI][idx], im = mk[idx];
    double Pw = mp.gravity * mp.rho_w * (h - zb[idx]);
    double sca_prod = 0.0;
    if (mp.basal_friction) sca_prod = 20. * 20. * mp.ub0 * fabs(Pi - Pw) * mp.ub0;
    double abs_QPw = t0 + t1 - (u0 + u1);
    if ((abs_QPw < 0) && (b < 1e-6)) abs_QPw = 0.0;
    double m = mp.G + sca_prod - mp.rho_w * mp.gravity * (t0 + t1) + mp.ct * mp.cw * mp.rho_w * mp.rho_w * mp.gravity * abs_QPw;
    m = m / mp.L;
    m = fmax(m, 0.0);
    if (im < 0.0) m = 0.0;
    fp.f[SUHMO_F_MR][idx] = m;
    fp.f[SUHMO_F_PW][idx] = Pw;
    const double ub_norm = sqrt(mp.ub0 * mp.ub0 + mp.ub1 * mp.ub1);
    if (MODE == 0) {                                           // RHS_h, :3044-3077
        double rho_coef = (1.0 / mp.rho_w - 1.0 / mp.rho_i);
        if (mp.head_melt_off) rho_coef *= 0.0;                 // run-state setting of the reference's committed tables (suhmo_hip.h)
        double r = m * rho_coef;
        if (b < mp.br) r -= ub_norm * (mp.br - b) / mp.lr;
        if (mp.use_moulin_source) r += fp.f[SUHMO_F_MSRC][idx] * mp.ramp + mp.distributed_input;   // :3060-3066
        else r += (im > 0.0) ? mp.distributed_input : 0.0;     // distributed input where there is ice, :2871-2875
        if (mp.diffFactor != 0.0) r -= mp.diffFactor * fp.f[SUHMO_F_DTERM][idx];     // :3071
        if (im < 0.0) r = 0.0;
        fp.f[SUHMO_F_RHS][idx] = r;
    } else {                                                   // CalcRHS_gapHeightFAS :2113-2168 + forward Euler :3406
        double RHS = m * (1.0 / mp.rho_i), RHS_A = RHS, RHS_B = 0.0, cd = 0.0;
        if ((im < 0.0) && mp.use_mask_rhs_b) { RHS = 0.0; if (mp.use_impl_diff) RHS = b; }
        else {
            if (b < mp.br) { RHS += ub_norm * (mp.br - b) / mp.lr; RHS_B = ub_norm * (mp.br - b) / mp.lr; }
            double PimPw = Pi - Pw, AbsPimPw = fabs(PimPw);
            if (ph.cutOffbr > b) RHS -= ph.A * (AbsPimPw * AbsPimPw) * PimPw * b * (1.0 - (ph.cutOffbr - b) / ph.cutOffbr);
            else if (ph.maxOffbr < b) RHS -= ph.A * (AbsPimPw * AbsPimPw) * PimPw * b * (1.0 - (ph.maxOffbr - b) / ph.maxOffbr);
            else RHS -= ph.A * (AbsPimPw * AbsPimPw) * PimPw * b;
            if (!mp.use_impl_diff && mp.diffFactor != 0.0) RHS += mp.diffFactor * fp.f[SUHMO_F_DTERM][idx];   // :2145,:2152,:2159
            cd = RHS_A / (RHS_A + RHS_B);
            if (mp.use_impl_diff) RHS = b + dt * RHS;          // :2165
        }
        fp.f[SUHMO_F_CD][idx] = cd;
        if (mp.use_impl_diff) fp.f[SUHMO_F_RES][idx] = RHS;    // right-hand side of the implicit solve (RES is free here)
        else fp.f[SUHMO_F_B][idx] = RHS * dt + b;              // old b == b: the gap height is untouched during [II]
    }
}
// (an ensemble: every member's own physics constants and model parameters)
template <class T, int MODE> __global__ __launch_bounds__(256) void k_melt(T t, double dt) { d_melt<MODE>(t.view(), t.fields(), t.phys(), t.model(), dt); }
template <class T> static int launch_melt(const T &t, int final_, double dt, hipStream_t st)
{
    return final_ ? launch_over(k_melt<T, 1>, t, CELLS, st, dt) : launch_over(k_melt<T, 0>, t, CELLS, st, dt);
}

// run-state setting freeze_icefree_gap (suhmo_hip.h): cells without ice keep their gap height through SolveForGap_nl -- the solved
// value of such a cell is replaced by the old one before the solution is copied back (valid cells; the ghosts are refilled afterwards)
__device__ __forceinline__ void d_keep_icefree_cell(const double *mk, const double *bold, double *sol, size_t idx)
{
    if (mk[idx] < 0.0) sol[idx] = bold[idx];
}
__device__ __forceinline__ void d_keep_icefree(const DV &v, const double *__restrict__ mk, const double *__restrict__ bold, double *__restrict__ sol)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    d_keep_icefree_cell(mk, bold, sol, cidx(v, i, j));
}
template <class T> __global__ __launch_bounds__(256) void k_keep_icefree(T h, T g)     // h: the level, g: its gap handle
{
    const FP &fh = h.fields();
    d_keep_icefree(h.view(), fh.f[SUHMO_F_MASK], fh.f[SUHMO_F_B], g.fields().f[SUHMO_F_PHI]);
}
template <class T> static int launch_keep_icefree(const T &h, const T &g, hipStream_t st) { return launch_over(k_keep_icefree<T>, h, CELLS, st, g); }
// SolveForGap_nl of a batch (suhmo_batch.hip): h = the members' tables of depth 0, g = those of their gap handles.  What
// gap_level_prepare copies canvas by canvas (b -> PHI the initial guess, RES -> RHS, DCX -> BX, DCY -> BY; ghosts included), for every
// implicit member in one launch; a canvas is an even number of doubles (the pitch is a multiple of 16)
__global__ __launch_bounds__(256) void k_gap_load(OnMembers h, OnMembers g, size_t elems2)
{
    const FP s = h.fields(), d = g.fields();
    const double2 *__restrict__ b = (const double2 *)s.f[SUHMO_F_B], *__restrict__ res = (const double2 *)s.f[SUHMO_F_RES];
    const double2 *__restrict__ dcx = (const double2 *)s.f[SUHMO_F_DCX], *__restrict__ dcy = (const double2 *)s.f[SUHMO_F_DCY];
    double2 *__restrict__ phi = (double2 *)d.f[SUHMO_F_PHI], *__restrict__ rhs = (double2 *)d.f[SUHMO_F_RHS];
    double2 *__restrict__ bx = (double2 *)d.f[SUHMO_F_BX], *__restrict__ by = (double2 *)d.f[SUHMO_F_BY];
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < elems2; q += (size_t)gridDim.x * blockDim.x) {
        const double2 v0 = b[q], v1 = res[q], v2 = dcx[q], v3 = dcy[q];
        phi[q] = v0; rhs[q] = v1; bx[q] = v2; by[q] = v3;
    }
}
// ... and the way back: keep_icefree where the member's freeze_icefree_gap asks for it (valid cells), then the whole canvas into b
__global__ __launch_bounds__(256) void k_gap_store(OnMembers h, OnMembers g, size_t elems)
{
    const DV &v = h.view();
    const FP fh = h.fields();
    const double *mk = fh.f[SUHMO_F_MASK];
    double *b = fh.f[SUHMO_F_B], *sol = g.fields().f[SUHMO_F_PHI];
    const bool freeze = h.model().freeze_icefree_gap != 0;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < elems; q += (size_t)gridDim.x * blockDim.x) {
        if (freeze) {
            const int i = (int)(q % v.P) - SUHMO_XOFF, j = (int)(q / v.P) - v.gy;
            if (i >= 0 && i < v.nx && j >= 0 && j < v.ny) d_keep_icefree_cell(mk, b, sol, q);
        }
        b[q] = sol[q];
    }
}
int suhmo_batch_gap_load(const OnMembers &h, const OnMembers &g, size_t elems, hipStream_t st)
{
    if (elems & 1) { suhmo_set_error("internal: batch: a canvas of an odd number of doubles"); return -4; }
    return launch_grid(k_gap_load, h, dim3((unsigned)std::min<size_t>((elems / 2 + 255) / 256, 256)), dim3(256), st, g, elems / 2);
}
int suhmo_batch_gap_store(const OnMembers &h, const OnMembers &g, size_t elems, hipStream_t st)
{
    return launch_grid(k_gap_store, h, dim3((unsigned)std::min<size_t>((elems + 255) / 256, 256)), dim3(256), st, g, elems);
}
static int keep_icefree(suhmo_level *L, suhmo_level *G, hipStream_t st) { return launch_keep_icefree(on_level(L, 0), on_level(G, 0), st); }

// Picard convergence test, :3169-3185
static int exchange1(suhmo_level *L, int f, hipStream_t st) { return suhmo_exchange_list(L, 0, &f, 1, st); }
// Both numbers of the Picard test in one pass and one read-back: max h and max |h_lagged - h|.  The reference's
// max |(h_lagged - h) / maxHead| is the second divided by |maxHead| afterwards: a correctly rounded division by a fixed
// divisor is monotone and sign-symmetric, so the maximum of the quotients is the quotient of the maximum, bit for bit.
// First stage (RedMax2 of suhmo_reduce.h): pairs of partial maxima, one per workgroup.
// (the boxes of a level, the members of an ensemble: a level's own workgroups per box / member, its partial maxima one after the other)
template <class T> __global__ __launch_bounds__(256) void k_picard2_partial(T t, double *__restrict__ partial, Excl ex, int use_cover)
{
    const DV &v = t.view();
    const FP &fp = t.fields();
    const double *__restrict__ h = fp.f[SUHMO_F_PHI], *__restrict__ hl = fp.f[SUHMO_F_HLAG];
    const double *__restrict__ cover = use_cover ? fp.f[SUHMO_F_COVER] : nullptr;     // hierarchy of box unions
    reduce_cells<RedMax2>(v, partial + 2 * (t.slot((size_t)gridDim.x * gridDim.y) + plane_block()), [&](int i, int j, double (&a)[2]) {
        if (i >= ex.i0 && i < ex.i1 && j >= ex.j0 && j < ex.j1) return;
        const int idx = cidx(v, i, j);
        if (cover && cover[idx] != 0.0) return;
        a[0] = fmax(a[0], h[idx]);
        a[1] = fmax(a[1], fabs(hl[idx] - h[idx]));
    });
}
// max h and max |hl - h| over the level's cells (local to the rank)
// over_ranks: the maxima over all ranks of the level's strip partition (computeMax; one MAX all-reduce of both values)
static int picard_maxima(suhmo_level *L, double *maxh, double *maxd, hipStream_t st, Excl ex = Excl{0, 0, 0, 0}, bool covered = false, bool over_ranks = false)
{
    int rc = launch_reduction<RedMax2>(k_picard2_partial<OnLevel>, on_level(L, 0), CAP_LEVEL, L->scratch + 2, L->scratch,
                                       over_ranks ? suhmo_reduce_slot(L) : suhmo_host_slot(L), st, ex, (int)covered);
    if (rc) return rc;
    if (over_ranks) return suhmo_reduce_finish(L, st, 2, 0, maxh, maxd);
    return suhmo_readback(L, st, maxh, maxd);
}
static inline double picard_quotient(double maxd, double maxHead) { return maxd == 0.0 ? 0.0 : maxd / fabs(maxHead); }

// grad h (cell centred, ghosted) and Re on the ghosted level: reuses the WFlx_level kernels of
// suhmo_bcoef.hip (identical arithmetic: NEWMACGRAD + EdgeToCell + ExtrapGhostCells + COMPUTERE)
int suhmo_grad_re(suhmo_level *L, int depth, hipStream_t st);      // suhmo_bcoef.hip
int suhmo_grad_cc(suhmo_level *L, int depth, hipStream_t st);
int suhmo_copy_ghosts(suhmo_level *L, int depth, int field, hipStream_t st);

static int lagged_chain(suhmo_level *L, hipStream_t st)
{
    int rc = suhmo_grad_re(L, 0, st); if (rc) return rc;
    return launch_qw_faces(on_level(L, 0), st);
}

// ---- diffusion of the gap height (suhmo.diffFactor != 0)
// ghosts of the melt rate: exchange + ExtrapGhostCells (:2513,:2526); only the edges are read (CellToEdge)
__device__ __forceinline__ void d_extrap_ghosts(const DV &v, double *__restrict__ g)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * v.ny) {
        int side = t / v.ny, j = t % v.ny;
        if (v.cfx[side]) return;                             // coarse-fine side: interpolated
        if (side == 0) { int idx = cidx(v, 0, j); g[idx - 1] = v.per[0] ? g[idx + v.nx - 1] : 2.0 * g[idx] - g[idx + 1]; }
        else { int idx = cidx(v, v.nx - 1, j); g[idx + 1] = v.per[0] ? g[idx - (v.nx - 1)] : 2.0 * g[idx] - g[idx - 1]; }
        return;
    }
    t -= 2 * v.ny;
    if (t < 2 * v.nx) {
        int side = t / v.nx, i = t % v.nx;
        if (v.ext[side]) return;                             // rank boundary: exchanged; coarse-fine side: interpolated
        if (side == 0) { int idx = cidx(v, i, 0); g[idx - v.P] = v.per[1] ? g[idx + (v.ny - 1) * v.P] : 2.0 * g[idx] - g[idx + v.P]; }
        else { int idx = cidx(v, i, v.ny - 1); g[idx + v.P] = v.per[1] ? g[idx - (v.ny - 1) * v.P] : 2.0 * g[idx] - g[idx - v.P]; }
    }
}
template <class T> __global__ void k_extrap_ghosts(T t, int field) { d_extrap_ghosts(t.view(), t.field(field)); }
// ... of any cell field of every box of a level (the regrid's field transfer, suhmo_regrid.hip)
int launch_extrap_ghosts(const OnBoxes &t, int field, hipStream_t st) { return launch_over(k_extrap_ghosts<OnBoxes>, t, PERIMETER, st, field); }
// dCoeff: CellToEdge(mR), CellToEdge(b), setup_iceMask_EC, COMPUTEDCOEFF (src/AmrHydro.cpp:1831-1862, ...F.ChF:241-265)
__device__ __forceinline__ void d_dcoef_faces(const DV &v, const FP &fp, suhmo_phys_t ph, double rho_i)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i > v.nx || j > v.ny) return;
    const double *__restrict__ B = fp.f[SUHMO_F_B], *__restrict__ mR = fp.f[SUHMO_F_MR], *__restrict__ mk = fp.f[SUHMO_F_MASK];
    int idx = cidx(v, i, j);
    for (int dir = 0; dir < 2; dir++) {
        if ((dir == 0 && j >= v.ny) || (dir == 1 && i >= v.nx)) continue;
        int im = dir == 0 ? idx - 1 : idx - v.P;
        double m = mk[idx], mm1 = mk[im], mec;
        if (fabs(m - mm1) < 1e-10) mec = (m > 0.0) ? 1.0 : -1.0; else mec = 0.0;
        int f = dir == 0 ? i + v.i0 : j + v.j0, fhi = dir == 0 ? v.nxg : v.nyg;   // domain faces (global index on a strip / patch)
        if (f == 0 || f == fhi) mec = 0.0;
        double bec = 0.5 * (B[idx] + B[im]), mrec = 0.5 * (mR[idx] + mR[im]), d;
        if (mec < 0.0 && ph.cutOffB > 0) d = 0.0; else d = fmax(bec * mrec / rho_i, 5.0e-6);
        fp.f[dir == 0 ? SUHMO_F_DCX : SUHMO_F_DCY][idx] = d;
    }
}
template <class T> __global__ __launch_bounds__(256) void k_dcoef_faces(T t) { d_dcoef_faces(t.view(), t.fields(), t.phys(), t.model().rho_i); }
// COMPUTEDIFTERM2D (src/AmrHydroF.ChF:289-343) of the gap height with its copied ghosts
__device__ __forceinline__ void d_difterm(const DV &v, FP fp)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    const double *__restrict__ B = fp.f[SUHMO_F_B], *__restrict__ dx_ = fp.f[SUHMO_F_DCX], *__restrict__ dy_ = fp.f[SUHMO_F_DCY];
    int idx = cidx(v, i, j);
    const double dxinv0 = 1.0 / (v.dx * v.dx), dxinv1 = 1.0 / (v.dy * v.dy);
    fp.f[SUHMO_F_DTERM][idx] =
        (dx_[idx + 1] * (B[idx + 1] - B[idx]) * dxinv0 - dx_[idx] * (B[idx] - B[idx - 1]) * dxinv0
         + dy_[idx + v.P] * (B[idx + v.P] - B[idx]) * dxinv1 - dy_[idx] * (B[idx] - B[idx - v.P]) * dxinv1);
}
template <class T> __global__ __launch_bounds__(256) void k_difterm(T t) { d_difterm(t.view(), t.fields()); }
// the lagged diffusion terms of a target: ghosts of the melt rate, dCoeff on the faces, the term itself (the fields exist)
template <class T> static int launch_diffusion_terms(const T &t, hipStream_t st)
{
    int rc;
    if ((rc = launch_over(k_extrap_ghosts<T>, t, PERIMETER, st, (int)SUHMO_F_MR)) || (rc = launch_over(k_dcoef_faces<T>, t, FACES, st))) return rc;
    return launch_over(k_difterm<T>, t, CELLS, st);
}
static int diffusion_terms(suhmo_level *L, const suhmo_model_params_t *mp, hipStream_t st)
{
    for (int f : {SUHMO_F_DCX, SUHMO_F_DCY, SUHMO_F_DTERM}) if (!suhmo_field(L, 0, f)) { suhmo_set_error("field allocation failed"); return -2; }
    int rc = exchange1(L, SUHMO_F_MR, st); if (rc) return rc;          // levelmR.exchange() :2513
    return launch_diffusion_terms(stepping(on_level(L, 0), *mp), st);
}
// the lagged diffusion terms (diffusion), then the melt rate with RHS_h (final_ = 0) or with the gap-height update (1) of one level
static int level_melt(suhmo_level *L, const suhmo_model_params_t *mp, double dt, int final_, bool diffusion, hipStream_t st)
{
    int rc;
    if (diffusion && (rc = diffusion_terms(L, mp, st))) return rc;
    return launch_melt(stepping(on_level(L, 0), *mp), final_, dt, st);
}
// SolveForGap_nl (src/AmrHydro.cpp:593-662): (1 - dt diffFactor div(D grad)) b = RES on a second level handle with the
// linear operator (alpha = 1, aCoef = 1, beta = dt diffFactor, bCoef = D, no nonlinear term), FixedNeumBCFill = Neumann 0.
// [Chombo] VCAMRPoissonOp2 / AMRMultiGrid are not in the reference's tree: the cycle is the FAS cycle of suhmo_fas.hip,
// which for a linear operator converges to the same solution (oracle/time_loop.c:solve_gap_implicit does the same).
// this step's data of a level handle -> its gap handle G (canvases of one size), and the halo rows of G on a rank strip
static int gap_load(suhmo_level *L, suhmo_level *G, hipStream_t st)
{
    Depth &D = L->d[0], &GD = G->d[0];
    const size_t bytes = D.elems * sizeof(double);
    HIPCHK(hipMemcpyAsync(GD.fp.f[SUHMO_F_PHI], D.fp.f[SUHMO_F_B], bytes, hipMemcpyDeviceToDevice, st));      // initial guess = b :3382-3385
    HIPCHK(hipMemcpyAsync(GD.fp.f[SUHMO_F_RHS], D.fp.f[SUHMO_F_RES], bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(GD.fp.f[SUHMO_F_BX], D.fp.f[SUHMO_F_DCX], bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(GD.fp.f[SUHMO_F_BY], D.fp.f[SUHMO_F_DCY], bytes, hipMemcpyDeviceToDevice, st));
    GD.phi_fresh = 0;
    static const int halo_fields[] = {SUHMO_F_RHS, SUHMO_F_ACOEF, SUHMO_F_BX, SUHMO_F_BY};
    return suhmo_exchange_list(G, 0, halo_fields, 4, st);
}
// the second handle of a level (created on first use / when dt changes) loaded with this step's data
static int gap_level_prepare(suhmo_level *L, const suhmo_model_params_t *mp, double dt, hipStream_t st)
{
    Depth &D = L->d[0];
    if (L->gap && L->gap_dt != dt) {                       // a new time step size: only beta = dt diffFactor changes
        int rc = suhmo_level_set_alpha_beta(L->gap, 1.0, dt * mp->diffFactor); if (rc) return rc;
        L->gap_dt = dt;
    }
    if (!L->gap) {
        suhmo_level_desc_t d = L->desc;
        d.boxes = L->boxes.data(); d.nbox = (int)(L->boxes.size() / 4);
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) { d.bc.type[a][b] = 1; d.bc.value[a][b] = 0.0; }
        d.phys.use_NL = 0; d.alpha = 1.0; d.beta = dt * mp->diffFactor;
        int rc = suhmo_level_create(&L->gap, &d); if (rc) return rc;
        L->gap_dt = dt;
        if ((rc = suhmo_level_set_value(L->gap, 0, SUHMO_F_ACOEF, 1.0, (suhmo_stream_t)st))) return rc;       // aCoeff_GH :1820-1828
    }
    suhmo_level *G = L->gap;
    if (G->bottom_solver != L->bottom_solver || G->bottom_one_launch_max_cells != L->bottom_one_launch_max_cells) {   // the same bottom solver
        int rc = suhmo_bottom_configure(G, L->bottom_solver, L->bottom_one_launch_max_cells); if (rc) return rc;
    }
    suhmo_level_share_transport(G, L);
    if (G->ag != L->ag || G->ag_user != L->ag_user || G->agg_min_cells != L->agg_min_cells) {                // ... and the same agglomeration
        G->ag = L->ag; G->ag_user = L->ag_user; G->agg_min_cells = L->agg_min_cells;
        int rca = suhmo_agg_setup(G); if (rca) return rca;
    }       // same strip, same neighbours
    if (G->d[0].elems != D.elems) { suhmo_set_error("internal: gap level geometry"); return -4; }
    return gap_load(L, G, st);
}
static void gap_solver_params(suhmo_solver_params_t &sp, int cur_step)
{
    sp.num_smooth = 2; sp.num_bottom = 4; sp.max_iter = 100; sp.iter_min = 2; sp.imin = cur_step < 50 ? 10 : 5;
    sp.eps = 1.0e-7; sp.hang = 1.0e-6; sp.norm_thresh = 1.0e-7; sp.bcoeff_otf = 0; sp.max_depth = -1;
}
// SolveForHead_nl, :737-762
static void head_solver_params(suhmo_solver_params_t &sp, int cur_step)
{
    sp.num_smooth = 4; sp.num_bottom = 16; sp.max_iter = 100; sp.iter_min = 2; sp.imin = 5;
    sp.eps = 1.0e-7; sp.hang = 0.01; sp.norm_thresh = 1.0e-7; sp.bcoeff_otf = 1; sp.max_depth = -1;
    if (cur_step < 50) { sp.num_bottom = 10; sp.eps = 1.0e-10; sp.hang = 0.0001; sp.imin = 20; }
}
// ghosts of b of level l of nested levels (one level: lv = &L, l = 0): PiecewiseLinearFillPatch on coarse-fine sides (from the coarser
// level's current b, whose halo rows were exchanged just before), copies on domain sides (:3419-3420 / :3451-3452), halo rows on rank boundaries
static int amr_gap_ghosts(suhmo_level_t **lv, int l, hipStream_t st)
{
    int rc;
    if (!lv[l]) return 0;
    if (l > 0 && (rc = suhmo_amr2_pwl_fill(lv[l - 1], lv[l], SUHMO_F_B, SUHMO_F_B, (suhmo_stream_t)st))) return rc;
    if ((rc = suhmo_copy_ghosts(lv[l], 0, SUHMO_F_B, st))) return rc;
    return exchange1(lv[l], SUHMO_F_B, st);
}
// the solution back into level l: cells without ice keep their b if asked, PHI of the gap handle G -> b, the ghosts of b
static int gap_store(suhmo_level_t **lv, int l, suhmo_level *G, const suhmo_model_params_t *mp, hipStream_t st)
{
    int rc;
    Depth &D = lv[l]->d[0];
    if (mp->freeze_icefree_gap && (rc = keep_icefree(lv[l], G, st))) return rc;
    HIPCHK(hipMemcpyAsync(D.fp.f[SUHMO_F_B], G->d[0].fp.f[SUHMO_F_PHI], D.elems * sizeof(double), hipMemcpyDeviceToDevice, st));
    return amr_gap_ghosts(lv, l, st);
}
static int solve_gap_implicit(suhmo_level *L, const suhmo_model_params_t *mp, double dt, int cur_step, hipStream_t st)
{
    int rc = gap_level_prepare(L, mp, dt, st); if (rc) return rc;
    suhmo_level *G = L->gap;
    rc = suhmo_level_build_mg_coefficients(G, (suhmo_stream_t)st); if (rc) return rc;    // coarse D = average of the fine faces
    suhmo_solver_params_t sp;
    gap_solver_params(sp, cur_step);
    if ((rc = suhmo_level_solve(G, &sp, nullptr, nullptr, (suhmo_stream_t)st))) return rc;
    return gap_store(&L, 0, G, mp, st);
}

// ------------------------------------------------------------------ AmrHydro::timeStepFAS, once for every level layout
// the checks every time step starts with, and the fields of every level its phases write
static const int step_fields[] = {SUHMO_F_MR, SUHMO_F_PW, SUHMO_F_QWX, SUHMO_F_QWY, SUHMO_F_HLAG, SUHMO_F_CD, SUHMO_F_GRADX, SUHMO_F_GRADY, SUHMO_F_RE};
static int alloc_step_fields(suhmo_level *L)
{
    for (int f : step_fields) if (!suhmo_field(L, 0, f)) { suhmo_set_error("field allocation failed"); return -2; }
    return 0;
}
static bool lacks_source(const suhmo_level *L, const suhmo_model_params_t *mp) { return mp->use_moulin_source && !L->d[0].fp.f[SUHMO_F_MSRC]; }
// a rank strip (of a whole level: rk = ext) exchanges halo rows and reduces the Picard test through the hooks
static bool strip_without_hooks(const suhmo_level *L) { const DV &v = L->d[0].v; return (v.rk[0] || v.rk[1]) && !(L->ex && L->ar); }
static int check_step_args(const suhmo_model_params_t *mp, double dt, int cur_step)
{
    ARG(mp); ARG(dt > 0 && cur_step >= 1);
    if (mp->use_impl_diff && mp->diffFactor == 0.0) { suhmo_set_error("use_ImplDiff with diffFactor = 0"); return -1; }
    return 0;
}
int suhmo_step_check_args_(const suhmo_model_params_t *mp, double dt, int cur_step) { return check_step_args(mp, dt, cur_step); }
// the Picard test after iteration ite_idx (:3169-3195), given max h and max |h_lagged - h| over the cells no finer level covers
static int picard_test(double maxHead, double maxd, int ite_idx, int cur_step, const suhmo_model_params_t *mp, bool &converged)
{
    const double res = picard_quotient(maxd, maxHead);
    if (ite_idx > 100) { suhmo_set_error("does not converge (Picard iterations > 100)"); return -6; }   // :3190-3195
    if (cur_step < 2) converged = res < 0.05 && ite_idx > 2;
    else if (cur_step < 50) converged = res < 0.05;
    else converged = res < mp->eps_picard;
    return 0;
}
// The skeleton over a level layout Y (OneLevel, Nested, BoxUnions below).  Y has `nlev`, `base` (level 0's handle, the one the head
// solve's multigrid depths hang off) and `st`; its hooks gap_ghosts(l), chain(l) and melt_final(l) act on level l, the others on every
// level in the layout's own launch order.  What [III] does with the gap height depends on use_impl_diff: explicit_gap_ghosts and
// implicit_gap_solve decide it from mp of the one model, or per member (the overloads for Batch below).
// A layout may hold several independent MEMBERS on one grid (`nmem`; the three layouts of one model have 1; a batch: suhmo_batch.hip): the
// hooks then act on the members of the current phase, mp, the solve's cycle counts and the Picard maxima are arrays over the members, and
// `select(still)` tells the layout which members the next Picard iteration serves (returns false when none is left: the phases after
// the loop serve everybody again).  Every member sees the sequence of one model.
template <class Y> static int mg_coefficients(Y &y) { return suhmo_build_mg_coefficients(y.base, false, y.st); }
template <class Y> static int explicit_gap_ghosts(Y &y, int l, const suhmo_model_params_t *mp) { return mp->use_impl_diff ? 0 : y.gap_ghosts(l); }
template <class Y> static int implicit_gap_solve(Y &y, const suhmo_model_params_t *mp, double dt, int cur_step) { return mp->use_impl_diff ? y.solve_gap(mp, dt, cur_step) : 0; }
template <class Y>
static int timestep_fas(Y &y, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles, const char *serve = nullptr)
{
    int rc;
    // [I] ghosts of b (exchange + CopyGhostCells, :2385,:2429); ghosts of h are evaluated on the fly.  MGnewOp coarsening of B
    // (+ static Pi, zb, mask, aCoef): once per step, b does not change in [II]
    for (int l = 0; l < y.nlev; l++) if ((rc = y.gap_ghosts(l))) return rc;
    if ((rc = mg_coefficients(y))) return rc;                                     // bCoef: re-averaged by every V-cycle (bcoeff_otf)
    suhmo_solver_params_t sp;
    head_solver_params(sp, cur_step);
    const int n = y.nmem;
    int ite[SUHMO_BATCH_MAX], nv[SUHMO_BATCH_MAX], it[SUHMO_BATCH_MAX];
    char still[SUHMO_BATCH_MAX];
    double maxHead[SUHMO_BATCH_MAX], maxd[SUHMO_BATCH_MAX];
    for (int k = 0; k < n; k++) { ite[k] = nv[k] = 0; still[k] = serve ? serve[k] : 1; }    // (serve: the members of a layout the step is for)
    for (int ite_idx = 0; y.select(still); ite_idx++) {                           // [II]
        if ((rc = y.lag_head())) return rc;                                       // h_lagged = h, coarse-fine ghosts of b and mR
        for (int l = 0; l < y.nlev; l++) if ((rc = y.chain(l))) return rc;       // grad h, Re, Qw
        if ((rc = y.head_rhs(mp, dt))) return rc;                                 // bCoef, melt rate, RHS_h
        for (int k = 0; k < n; k++) { it[k] = 0; maxHead[k] = maxd[k] = 0.0; }
        if ((rc = y.solve_head(sp, it))) return rc;                               // SolveForHead_nl, CoarseAverage of h
        if ((rc = y.picard_maxima(maxHead, maxd))) return rc;
        for (int k = 0; k < n; k++) {
            if (!still[k]) continue;
            bool converged = false;
            nv[k] += it[k];
            if ((rc = picard_test(maxHead[k], maxd[k], ite_idx, cur_step, &mp[k], converged))) return rc;
            ite[k] = ite_idx + 1;
            if (converged) still[k] = 0;
        }
    }
    // [III] level by level: the coarse gap height is already updated when the fine ghost cells are filled
    for (int l = 0; l < y.nlev; l++) {
        if ((rc = y.chain(l)) || (rc = y.melt_final(l, mp, dt))) return rc;
        if ((rc = explicit_gap_ghosts(y, l, mp))) return rc;                      // (implicit: b stays, RES = b + dt RHS)
    }
    if ((rc = implicit_gap_solve(y, mp, dt, cur_step))) return rc;                // SolveForGap_nl :3425-3455, then the ghosts of b
    for (int k = 0; k < n; k++) { if (picard_iters) picard_iters[k] = ite[k]; if (vcycles) vcycles[k] = nv[k]; }
    return 0;
}

// ------------------------------------------------------------------ the time step on one level
struct OneLevel {
    suhmo_level *base;
    hipStream_t st;
    int nlev = 1;
    int nmem = 1;
    bool select(const char *still) { return still[0] != 0; }
    int gap_ghosts(int) { return amr_gap_ghosts(&base, 0, st); }
    int lag_head()
    {
        Depth &D = base->d[0];
        HIPCHK(hipMemcpyAsync(D.fp.f[SUHMO_F_HLAG], D.fp.f[SUHMO_F_PHI], D.elems * sizeof(double), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    int chain(int) { return lagged_chain(base, st); }
    int head_rhs(const suhmo_model_params_t *mp, double dt)
    {
        int rc;
        if ((rc = launch_bcoef_faces(on_level(base, 0), st))) return rc;                          // aCoeff_bCoeff :3087-3102
        suhmo_faces_made(base);
        if ((rc = level_melt(base, mp, dt, 0, mp->diffFactor != 0.0, st))) return rc;   // lagged melt rate :2548-2551, :2982-2992
        return exchange1(base, SUHMO_F_RHS, st);                                        // rank strips relax their halo rows redundantly
    }
    int solve_head(const suhmo_solver_params_t &sp, int *it) { return suhmo_level_solve(base, &sp, it, nullptr, st); }
    int picard_maxima(double *maxh, double *maxd)                                       // computeMax over all ranks
    {
        return ::picard_maxima(base, maxh, maxd, st, Excl{0, 0, 0, 0}, false, true);
    }
    int melt_final(int, const suhmo_model_params_t *mp, double dt) { return level_melt(base, mp, dt, 1, false, st); }
    int solve_gap(const suhmo_model_params_t *mp, double dt, int cur_step) { return solve_gap_implicit(base, mp, dt, cur_step, st); }
};

extern "C" int suhmo_level_timestep(suhmo_level_t *L, const suhmo_model_params_t *mp, double dt, int cur_step,
                                    int *picard_iters, int *vcycles, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::timeStepFAS");
    ARG(L);
    int rc = check_step_args(mp, dt, cur_step); if (rc) return rc;
    Depth &D = L->d[0];
    if (L->desc.nx_global > 0 || (D.v.ext[0] && !D.v.rk[0]) || (D.v.ext[1] && !D.v.rk[1])) { suhmo_set_error("timestep on an AMR patch is not built yet"); return -5; }
    if (strip_without_hooks(L)) { suhmo_set_error("timestep on a rank strip needs the exchange hooks (suhmo_level_attach_rccl / suhmo_level_set_hooks)"); return -1; }
    HIPCHK(hipSetDevice(L->device));
    if (lacks_source(L, mp)) { suhmo_set_error("use_moulin_source without suhmo_level_moulin_source"); return -1; }
    if ((rc = alloc_step_fields(L))) return rc;
    if (L->track_old_volume && (rc = suhmo_level_track_volume_(L, (hipStream_t)s))) return rc;     // "WATER BUDGET": the volume the step starts from
    OneLevel y{L, (hipStream_t)s};
    return timestep_fas(y, mp, dt, cur_step, picard_iters, vcycles);
}

// ------------------------------------------------------------------ the time step on a batch of levels on one grid (suhmo_batch.hip)
// OneLevel's hooks with every launch serving the members of the current phase (BatchStep): a whole level has no exchange, the chain is
// suhmo_grad_re + Qw, the Picard maxima of all members come back in one read-back.  The diffusion terms run over the members whose
// diffFactor is not 0, as level_melt decides for one model.
static bool has_diffusion(const suhmo_model_params_t &m) { return m.diffFactor != 0.0; }
static bool is_implicit(const suhmo_model_params_t &m) { return m.use_impl_diff != 0; }
static bool is_explicit(const suhmo_model_params_t &m) { return m.use_impl_diff == 0; }
struct Batch {
    suhmo_batch *B;
    hipStream_t st;
    int nlev = 1;
    int nmem;
    bool select(const char *still) { return suhmo_batch_step_select(B, still); }
    int gap_ghosts(const BatchSel &sel)
    {
        if (sel.n <= 0) return 0;
        const BatchStep p = suhmo_batch_step(B);
        suhmo_batch_count(B, 1);
        return launch_coef_ghosts(on_members(p.t, sel, *p.v), SUHMO_F_B, st);
    }
    int gap_ghosts(int) { return gap_ghosts(suhmo_batch_step(B).sel); }
    int lag_head()
    {
        const BatchStep p = suhmo_batch_step(B);
        suhmo_batch_count(B, 1);
        return launch_copy_canvas(on_members(p.t, p.sel, *p.v), SUHMO_F_HLAG, SUHMO_F_PHI, p.elems, st);
    }
    int chain(int)
    {
        const BatchStep p = suhmo_batch_step(B);
        const OnMembers t = on_members(p.t, p.sel, *p.v);
        int rc;
        if ((rc = launch_grad_cc(t, st)) || (rc = launch_re(t, st))) return rc;
        suhmo_batch_count(B, 4);
        return launch_qw_faces(t, st);
    }
    int melt(const suhmo_model_params_t *mp, double dt, int final_, bool diffusion)
    {
        const BatchStep p = suhmo_batch_step(B);
        int rc;
        if (diffusion) {
            const BatchSel d = suhmo_batch_step_subset(B, mp, has_diffusion);
            if (d.n > 0) {
                if ((rc = launch_diffusion_terms(on_members(p.t, d, *p.v, p.mp), st))) return rc;
                suhmo_batch_count(B, 3);
            }
        }
        suhmo_batch_count(B, 1);
        return launch_melt(on_members(p.t, p.sel, *p.v, p.mp), final_, dt, st);
    }
    int head_rhs(const suhmo_model_params_t *mp, double dt)
    {
        const BatchStep p = suhmo_batch_step(B);
        int rc = launch_bcoef_faces(on_members(p.t, p.sel, *p.v), st); if (rc) return rc;      // aCoeff_bCoeff :3087-3102
        suhmo_batch_step_faces_made(B);
        suhmo_batch_count(B, 1);
        return melt(mp, dt, 0, true);                                                    // lagged melt rate :2548-2551, :2982-2992
    }
    int solve_head(const suhmo_solver_params_t &sp, int *it) { return suhmo_batch_step_solve(B, &sp, it, st); }
    int picard_maxima(double *maxh, double *maxd)
    {
        const BatchStep p = suhmo_batch_step(B, true);
        int np, rc = launch_partials(k_picard2_partial<OnMembers>, on_members(p.t, p.sel, *p.v), CAP_LEVEL, p.partial, &np, st, Excl{0, 0, 0, 0}, 0);   // (the workgroups of picard_maxima, per member)
        if (rc) return rc;
        hipLaunchKernelGGL(k_norm_final_members<RedMax2>, dim3(1), dim3(256), 0, st, p.sel, p.partial, np, p.slot, p.flag, p.seq);
        HIPCHK(hipGetLastError());
        suhmo_batch_count(B, 2);
        return suhmo_batch_step_read(B, st, maxh, maxd);
    }
    int melt_final(int, const suhmo_model_params_t *mp, double dt) { return melt(mp, dt, 1, false); }
    // SolveForGap_nl of the members `sel` (solve_gap_implicit of each, one launch sequence), then the ghosts of their b
    int solve_gap(const BatchSel &sel, const suhmo_model_params_t *mp, double dt, int cur_step)
    {
        suhmo_solver_params_t sp;
        gap_solver_params(sp, cur_step);
        int rc = suhmo_batch_step_solve_gap(B, sel, mp, dt, &sp, st);
        return rc ? rc : gap_ghosts(sel);
    }
};
static int mg_coefficients(Batch &y) { return suhmo_batch_step_mg_coefficients(y.B, y.st); }
// [III] per member: forward Euler members get the ghosts of their new b, the others go through the gap batch
static int explicit_gap_ghosts(Batch &y, int, const suhmo_model_params_t *mp) { return y.gap_ghosts(suhmo_batch_step_subset(y.B, mp, is_explicit)); }
static int implicit_gap_solve(Batch &y, const suhmo_model_params_t *mp, double dt, int cur_step)
{
    const BatchSel sel = suhmo_batch_step_subset(y.B, mp, is_implicit);
    return sel.n > 0 ? y.solve_gap(sel, mp, dt, cur_step) : 0;
}
// active (NULL: everybody): the members the step is for; the others are in none of its launches and report 0 iterations
int suhmo_batch_timestep_run(suhmo_batch *B, const suhmo_model_params_t *mp, double dt, int cur_step, int *picard_iters, int *vcycles, hipStream_t st,
                             const int *active)
{
    int rc = 0;
    char serve[SUHMO_BATCH_MAX];
    for (int k = 0; k < suhmo_batch_size_(B); k++) serve[k] = !active || active[k];
    for (int k = 0; k < suhmo_batch_size_(B) && !rc; k++) rc = check_step_args(&mp[k], dt, cur_step);
    if (rc) return rc;
    for (int k = 0; k < suhmo_batch_size_(B); k++) {
        if (!serve[k]) continue;
        suhmo_level *L = suhmo_batch_member(B, k);
        if (lacks_source(L, &mp[k])) { suhmo_set_error("use_moulin_source without suhmo_level_moulin_source (member %d)", k); return -1; }
        if ((rc = alloc_step_fields(L))) return rc;
        if (mp[k].diffFactor != 0.0) for (int f : {SUHMO_F_DCX, SUHMO_F_DCY, SUHMO_F_DTERM}) if (!suhmo_field(L, 0, f)) { suhmo_set_error("field allocation failed"); return -2; }
    }
    if ((rc = suhmo_batch_step_begin(B, mp, st, active ? serve : nullptr))) return rc;
    if ((rc = suhmo_batch_step_track_volume(B, st))) return rc;                                     // "WATER BUDGET": option track_old_volume
    Batch y{B, st, 1, suhmo_batch_size_(B)};
    return timestep_fas(y, mp, dt, cur_step, picard_iters, vcycles, active ? serve : nullptr);
}


// ------------------------------------------------------------------ the time step on an AMR hierarchy
// oracle/amr_step_m.c: every level runs the phases above on its own rectangle; in between PiecewiseLinearFillPatch of the
// coarse-fine ghosts of b, mR, Re (:2373-2380, :2499-2507, :2711-2719), QuadCFInterp of h (inside compGradientMAC) and of
// the cell-centred gradient (:1650-1656), SolveForHead_nl over all levels, CoarseAverage of h (:3138-3141) and the
// Picard test over the cells no finer level covers (:3169-3185); the gap height by forward Euler level by level, or by
// SolveForGap_nl over a second hierarchy of handles (alpha = 1, beta = dt diffFactor, bCoef = D, as solve_gap_implicit).
// Rank strips: a rank holds of every level the rows of its own slab (lv[l] = NULL where the patch does not reach it);
// it still mirrors, on level l-1, the halo demand level l puts there, so that all ranks of a level's communicator issue
// the same sequence of exchanges (as the AMR cycle does, suhmo_amr.hip).
static int amr_chain(suhmo_level_t **lv, int l, hipStream_t st)
{
    suhmo_level *L = lv[l], *C = l > 0 ? lv[l - 1] : nullptr;
    suhmo_stream_t s = (suhmo_stream_t)st;
    int rc;
    if (!L) return C ? suhmo_ensure_phi_halo(C, 0, 1, st) : 0;
    if (C && (rc = suhmo_amr2_cf_interp(C, L, SUHMO_F_PHI, SUHMO_F_PHI, s))) return rc;
    if ((rc = suhmo_grad_cc(L, 0, st))) return rc;
    if (C) {
        if ((rc = suhmo_amr2_cf_interp(C, L, SUHMO_F_GRADX, SUHMO_F_GRADX, s))) return rc;
        if ((rc = suhmo_amr2_cf_interp(C, L, SUHMO_F_GRADY, SUHMO_F_GRADY, s))) return rc;
    }
    if ((rc = launch_re(on_level(L, 0), st))) return rc;
    if (C && (rc = suhmo_amr2_pwl_fill(C, L, SUHMO_F_RE, SUHMO_F_RE, s))) return rc;
    return launch_qw_faces(on_level(L, 0), st);
}
static Excl covered_by(suhmo_level_t **lv, int nlev, int l)
{
    if (l >= nlev - 1 || !lv[l + 1]) return Excl{0, 0, 0, 0};
    const DV &vf = lv[l + 1]->d[0].v, &v = lv[l]->d[0].v;
    return Excl{vf.i0 / 2 - v.i0, vf.j0 / 2 - v.j0, (vf.i0 + vf.nx) / 2 - v.i0, (vf.j0 + vf.ny) / 2 - v.j0};
}

struct Nested {
    suhmo_level_t **lv;
    int nlev;
    bool strips;
    suhmo_level *base;
    hipStream_t st;
    int nmem = 1;
    bool select(const char *still) { return still[0] != 0; }
    int gap_ghosts(int l) { return amr_gap_ghosts(lv, l, st); }
    int lag_head()
    {
        int rc;
        for (int l = 0; l < nlev; l++) {
            if (!lv[l]) continue;
            Depth &D = lv[l]->d[0];
            if ((rc = exchange1(lv[l], SUHMO_F_MR, st))) return rc;                    // levelmR.exchange() :2513 (and the stencil of the fill below)
            if (l > 0 && (rc = suhmo_amr2_pwl_fill(lv[l - 1], lv[l], SUHMO_F_MR, SUHMO_F_MR, (suhmo_stream_t)st))) return rc;
            if ((rc = amr_gap_ghosts(lv, l, st))) return rc;
            HIPCHK(hipMemcpyAsync(D.fp.f[SUHMO_F_HLAG], D.fp.f[SUHMO_F_PHI], D.elems * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        return 0;
    }
    int chain(int l) { return amr_chain(lv, l, st); }
    int head_rhs(const suhmo_model_params_t *mp, double dt)
    {
        int rc;
        for (int l = 0; l < nlev; l++) {
            if (!lv[l]) continue;
            if ((rc = launch_bcoef_faces(on_level(lv[l], 0), st))) return rc;                      // aCoeff_bCoeff :3087-3102
            suhmo_faces_made(lv[l]);
            if ((rc = level_melt(lv[l], mp, dt, 0, mp->diffFactor != 0.0, st))) return rc;
            if ((rc = exchange1(lv[l], SUHMO_F_RHS, st))) return rc;                   // halo rows relaxed redundantly
        }
        return 0;
    }
    int solve_head(const suhmo_solver_params_t &sp, int *it)
    {
        suhmo_stream_t s = (suhmo_stream_t)st;
        int rc = nlev == 1 ? suhmo_level_solve(lv[0], &sp, it, nullptr, s) : suhmo_amr_solve(lv, nlev, &sp, it, nullptr, s);
        if (rc) return rc;
        for (int l = nlev - 1; l > 0; l--) {                                            // CoarseAverage :3138-3141
            if (lv[l]) { if ((rc = suhmo_amr2_average(lv[l - 1], lv[l], SUHMO_F_PHI, SUHMO_F_PHI, s))) return rc; }
            else if (lv[l - 1]) lv[l - 1]->d[0].phi_fresh = 0;                          // changed on the ranks that hold level l
        }
        for (int l = 0; l + 1 < nlev; l++)      // the rings of the averaged heads, as the oracle refills them (exchange + BC, every level)
            if (lv[l] && (rc = suhmo_level_fill_ghosts(lv[l], 0, SUHMO_F_PHI, 0, s))) return rc;
        return 0;
    }
    int picard_maxima(double *maxHead, double *maxd)
    {
        int rc;
        *maxHead = -1.0e300; *maxd = 0.0;
        for (int l = 0; l < nlev; l++) {
            if (!lv[l]) continue;
            double m = 0.0, d = 0.0;
            if ((rc = ::picard_maxima(lv[l], &m, &d, st, covered_by(lv, nlev, l)))) return rc;
            *maxHead = std::max(*maxHead, m); *maxd = std::max(*maxd, d);
        }
        if (strips && lv[0]->ar) {                                  // computeMax over all ranks (level 0 reaches every rank)
            if ((rc = lv[0]->ar(lv[0]->user, maxHead))) return rc;
            if ((rc = lv[0]->ar(lv[0]->user, maxd))) return rc;
        }
        return 0;
    }
    int melt_final(int l, const suhmo_model_params_t *mp, double dt) { return lv[l] ? level_melt(lv[l], mp, dt, 1, false, st) : 0; }
    int solve_gap(const suhmo_model_params_t *mp, double dt, int cur_step)     // over a second hierarchy of handles
    {
        int rc;
        suhmo_stream_t s = (suhmo_stream_t)st;
        suhmo_level_t *gaps[8];
        for (int l = 0; l < nlev; l++) {
            gaps[l] = nullptr;
            if (!lv[l]) continue;
            if ((rc = gap_level_prepare(lv[l], mp, dt, st))) return rc;
            gaps[l] = lv[l]->gap;
        }
        if ((rc = suhmo_level_build_mg_coefficients(gaps[0], s))) return rc;
        suhmo_solver_params_t spg;
        gap_solver_params(spg, cur_step);
        if (nlev == 1) rc = suhmo_level_solve(gaps[0], &spg, nullptr, nullptr, s);
        else rc = suhmo_amr_solve(gaps, nlev, &spg, nullptr, nullptr, s);
        if (rc) return rc;
        for (int l = 0; l < nlev; l++) if (lv[l] && (rc = gap_store(lv, l, gaps[l], mp, st))) return rc;
        return 0;
    }
};

extern "C" int suhmo_amr_timestep(suhmo_level_t **lv, int nlev, const suhmo_model_params_t *mp, double dt, int cur_step,
                                  int *picard_iters, int *vcycles, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::timeStepFAS");
    ARG(lv && nlev >= 1 && nlev <= 8 && lv[0]);
    int rc = check_step_args(mp, dt, cur_step); if (rc) return rc;
    if ((rc = suhmo_amr_check_hierarchy(lv, nlev))) return rc;
    bool strips = false;
    for (int l = 0; l < nlev; l++) {
        if (!lv[l]) { strips = true; continue; }
        const DV &v = lv[l]->d[0].v;
        if (v.rk[0] || v.rk[1]) strips = true;
        if (strip_without_hooks(lv[l])) { suhmo_set_error("time step on rank strips needs the exchange hooks on every level"); return -1; }
        if (lacks_source(lv[l], mp)) { suhmo_set_error("use_moulin_source without a moulin source term (SUHMO_F_MSRC)"); return -1; }
    }
    HIPCHK(hipSetDevice(lv[0]->device));
    for (int l = 0; l < nlev; l++) if (lv[l] && (rc = alloc_step_fields(lv[l]))) return rc;
    Nested y{lv, nlev, strips, lv[0], (hipStream_t)s};
    return timestep_fas(y, mp, dt, cur_step, picard_iters, vcycles);
}

// ------------------------------------------------------------------ the time step on a hierarchy of box unions
// oracle/amr_step_m.c: suhmo_amr_timestep with every level's rectangle replaced by its boxes; after every fill of data ghosts
// the reference's exchange() is the fine-fine copy between the boxes of the level (suhmo_hier.hip).  Every phase of a level
// >= 1 is ONE launch over all its boxes (blockIdx.z = box, device tables of views and field pointers).
// One launcher on a whole level goes through on_hier_level (suhmo_hier_int.h); where level 0 does something different in kind (an exchange
// with the neighbouring strips, a whole-canvas copy), the branch on l == 0 is written out.
namespace {
int hier_chain(suhmo_hier *H, int l, hipStream_t st)
{
    int rc;
    suhmo_multi m;
    if ((rc = hier_cf(H, l, SUHMO_F_PHI, SUHMO_F_PHI, st))) return rc;                  // inside compGradientMAC
    if ((rc = hier_ff(H, l, SUHMO_F_PHI, -1, false, st))) return rc;
    if (l == 0) rc = suhmo_grad_cc(base_of(H), 0, st);                                  // (rank strips: with the halo rows of h)
    else if (!(rc = multi_of(H, l, st, m))) rc = suhmo_multi_grad_cc(m, st);
    if (rc) return rc;
    if ((rc = hier_cf(H, l, SUHMO_F_GRADX, SUHMO_F_GRADX, st, SUHMO_F_GRADY, SUHMO_F_GRADY))) return rc;   // :1650-1659
    if ((rc = hier_ff(H, l, SUHMO_F_GRADX, SUHMO_F_GRADY, true, st))) return rc;
    if ((rc = on_hier_level(H, l, st, [&](const auto &t) { return launch_re(t, st); }))) return rc;
    if ((rc = hier_pwl(H, l, SUHMO_F_RE, SUHMO_F_RE, st))) return rc;                   // :2711-2721
    if ((rc = hier_ff(H, l, SUHMO_F_RE, -1, true, st))) return rc;
    return on_hier_level(H, l, st, [&](const auto &t) { return launch_qw_faces(t, st); });
}
// ghosts of b of level l: PiecewiseLinearFillPatch on coarse-fine cells, exchange between the boxes, copies on domain sides
int hier_gap_ghosts(suhmo_hier *H, int l, hipStream_t st)
{
    int rc;
    if (l == 0) { suhmo_level *base = base_of(H); return amr_gap_ghosts(&base, 0, st); }      // (rank strips: with the halo rows)
    if ((rc = hier_pwl(H, l, SUHMO_F_B, SUHMO_F_B, st))) return rc;
    if ((rc = hier_ff(H, l, SUHMO_F_B, -1, true, st))) return rc;
    suhmo_multi m;
    if ((rc = multi_of(H, l, st, m))) return rc;
    return launch_coef_ghosts(m.on(), SUHMO_F_B, st);
}
// lagged diffusion terms (diffusion_terms of one level) and RHS_h / the gap-height right-hand side of a whole level
int hier_melt(suhmo_hier *H, int l, const suhmo_model_params_t *mp, double dt, int final_, bool diffusion, hipStream_t st)
{
    int rc;
    if (l == 0) return level_melt(base_of(H), mp, dt, final_, diffusion, st);       // (rank strips: with the halo rows of mR)
    if (diffusion) for (int f : {SUHMO_F_DCX, SUHMO_F_DCY, SUHMO_F_DTERM}) if ((rc = ensure_field(H, l, f))) return rc;
    suhmo_multi m;
    if ((rc = multi_of(H, l, st, m))) return rc;                             // the tables after the allocation
    if (m.nbox <= 0) return 0;                                               // owner computes: none of this level's boxes is this rank's
    if (diffusion && (rc = launch_diffusion_terms(stepping(m.on(), *mp), st))) return rc;
    return launch_melt(stepping(m.on(), *mp), final_, dt, st);
}
// max h and max |h_lagged - h| over the cells of level l no finer level covers
int hier_picard_maxima(suhmo_hier *H, int l, bool covered, double *maxh, double *maxd, hipStream_t st)
{
    int rc;
    suhmo_level *slot = base_of(H);
    if (l == 0) {
        suhmo_level *L = slot;
        if ((rc = picard_maxima(L, maxh, maxd, st, Excl{0, 0, 0, 0}, covered))) return rc;
        if (L->ar && (L->d[0].v.rk[0] || L->d[0].v.rk[1])) {                     // computeMax over the ranks of level 0
            if ((rc = L->ar(L->user, maxh))) return rc;
            if ((rc = L->ar(L->user, maxd))) return rc;
        }
        return 0;
    }
    suhmo_multi m;
    if ((rc = multi_of(H, l, st, m))) return rc;
    *maxh = -1.0e300; *maxd = 0.0;
    if (m.nbox > 0) {
        if ((rc = launch_reduction<RedMax2>(k_picard2_partial<OnBoxes>, m.on(), CAP_BOX_PAIRS, m.red, slot->scratch, suhmo_host_slot(slot), st, Excl{0, 0, 0, 0}, (int)covered))) return rc;
        if ((rc = suhmo_readback(slot, st, maxh, maxd))) return rc;
    }
    if (H->part) {                                            // owner computes: computeMax over the ranks
        if ((rc = suhmo_hier_allreduce_max_(H, maxh)) || (rc = suhmo_hier_allreduce_max_(H, maxd))) return rc;
    }
    return 0;
}
struct BoxUnions {
    suhmo_hier *H;
    int nlev;
    suhmo_level *base;
    hipStream_t st;
    int nmem = 1;
    bool select(const char *still) { return still[0] != 0; }
    int gap_ghosts(int l) { return hier_gap_ghosts(H, l, st); }
    int lag_head()
    {
        int rc;
        for (int l = 0; l < nlev; l++) {
            if ((rc = hier_gap_ghosts(H, l, st))) return rc;
            if (l == 0 && (rc = exchange1(base, SUHMO_F_MR, st))) return rc;                    // rank strips: levelmR.exchange() :2513
            if ((rc = hier_pwl(H, l, SUHMO_F_MR, SUHMO_F_MR, st))) return rc;
            if ((rc = hier_ff(H, l, SUHMO_F_MR, -1, true, st))) return rc;               // levelmR.exchange() :2513
            if (l == 0) { Depth &D = base->d[0];
                HIPCHK(hipMemcpyAsync(D.fp.f[SUHMO_F_HLAG], D.fp.f[SUHMO_F_PHI], D.elems * sizeof(double), hipMemcpyDeviceToDevice, st)); }
            else { suhmo_multi m; if ((rc = multi_of(H, l, st, m)) || (rc = launch_copy(m.on(), SUHMO_F_HLAG, SUHMO_F_PHI, st))) return rc; }
        }
        return 0;
    }
    int chain(int l) { return hier_chain(H, l, st); }
    int head_rhs(const suhmo_model_params_t *mp, double dt)
    {
        int rc;
        for (int l = 0; l < nlev; l++)                                                          // aCoeff_bCoeff :3087-3102
            if ((rc = on_hier_level(H, l, st, [&](const auto &t) { return launch_bcoef_faces(t, st); }))) return rc;
        for (int l = 0; l < nlev; l++) faces_made(H, l);
        for (int l = 0; l < nlev; l++) if ((rc = hier_melt(H, l, mp, dt, 0, mp->diffFactor != 0.0, st))) return rc;
        return exchange1(base, SUHMO_F_RHS, st);                                                // rank strips: halo rows relaxed redundantly
    }
    int solve_head(const suhmo_solver_params_t &sp, int *it)
    {
        int rc;
        if ((rc = suhmo_hier_solve(H, &sp, it, nullptr, (suhmo_stream_t)st))) return rc;
        for (int l = nlev - 1; l > 0; l--) if ((rc = hier_avg(H, l, SUHMO_F_PHI, SUHMO_F_PHI, 0, 0.0, st))) return rc;   // CoarseAverage :3138-3141
        for (int l = 0; l + 1 < nlev; l++) {    // the averaged heads' rings as the oracle refills them: BC of every box, level 0's periodic sides
            if (l == 0) { if ((rc = suhmo_level_fill_ghosts(base, 0, SUHMO_F_PHI, 0, (suhmo_stream_t)st))) return rc; continue; }
            suhmo_multi m;
            if ((rc = multi_of(H, l, st, m)) || (rc = launch_fill_ghosts(m.on(), SUHMO_F_PHI, 0, st))) return rc;
        }
        return 0;
    }
    int picard_maxima(double *maxHead, double *maxd)
    {
        int rc;
        *maxHead = -1.0e300; *maxd = 0.0;
        for (int l = 0; l < nlev; l++) {
            double m = 0.0, d = 0.0;
            if ((rc = hier_picard_maxima(H, l, l < nlev - 1, &m, &d, st))) return rc;
            *maxHead = std::max(*maxHead, m); *maxd = std::max(*maxd, d);
        }
        return 0;
    }
    int melt_final(int l, const suhmo_model_params_t *mp, double dt) { return hier_melt(H, l, mp, dt, 1, false, st); }
    int solve_gap(const suhmo_model_params_t *mp, double dt, int cur_step)     // over the gap-height hierarchy
    {
        int rc;
        suhmo_hier *G = nullptr;
        if ((rc = suhmo_hier_gap_(H, mp, dt, &G))) return rc;
        suhmo_level *gbase = base_of(G);
        if (gbase->d[0].elems != base->d[0].elems) { suhmo_set_error("internal: gap hierarchy geometry"); return -4; }
        if ((rc = gap_load(base, gbase, st))) return rc;               // level 0: one handle, as gap_level_prepare loads it
        for (int l = 1; l < nlev; l++) {                               // all boxes of a level: one launch
            static const int fd[4] = {SUHMO_F_PHI, SUHMO_F_RHS, SUHMO_F_BX, SUHMO_F_BY}, fs[4] = {SUHMO_F_B, SUHMO_F_RES, SUHMO_F_DCX, SUHMO_F_DCY};
            for (int f : fs) if ((rc = ensure_field(H, l, f))) return rc;
            for (int f : fd) if ((rc = ensure_field(G, l, f))) return rc;
            suhmo_multi mh, mg;
            if ((rc = multi_of(H, l, st, mh)) || (rc = multi_of(G, l, st, mg))) return rc;
            if ((rc = launch_copy_between(mg.on(), mh.on(), fd, fs, 4, st))) return rc;                                         // initial guess = b :3382-3385
            for (suhmo_level *L : G->lev[l].box) L->d[0].phi_fresh = 0;
        }
        if ((rc = suhmo_level_build_mg_coefficients(gbase, (suhmo_stream_t)st))) return rc;
        suhmo_solver_params_t spg;
        gap_solver_params(spg, cur_step);
        if ((rc = suhmo_hier_solve(G, &spg, nullptr, nullptr, (suhmo_stream_t)st))) return rc;
        if ((rc = gap_store(&base, 0, gbase, mp, st))) return rc;
        for (int l = 1; l < nlev; l++) {
            static const int fd[1] = {SUHMO_F_B}, fs[1] = {SUHMO_F_PHI};
            suhmo_multi mh, mg;
            if ((rc = multi_of(H, l, st, mh)) || (rc = multi_of(G, l, st, mg))) return rc;
            if (mp->freeze_icefree_gap && (rc = launch_keep_icefree(mh.on(), mg.on(), st))) return rc;
            if ((rc = launch_copy_between(mh.on(), mg.on(), fd, fs, 1, st))) return rc;
            if ((rc = hier_gap_ghosts(H, l, st))) return rc;
        }
        return 0;
    }
};
}  // namespace

extern "C" int suhmo_hier_timestep(suhmo_hier_t *H, const suhmo_model_params_t *mp, double dt, int cur_step,
                                   int *picard_iters, int *vcycles, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::timeStepFAS");
    ARG(H);
    int rc = check_step_args(mp, dt, cur_step); if (rc) return rc;
    const int nlev = H->nlev;
    HIPCHK(hipSetDevice(H->device));
    suhmo_hier_invalidate_(H);
    for (int l = 0; l < nlev; l++) {
        for (int f : step_fields) if ((rc = ensure_field(H, l, f))) return rc;
        if (mp->use_moulin_source) {
            const int k0 = H->lev[l].first_owned(), nk = H->lev[l].n_owned();
            for (int k = k0; k < k0 + nk; k++)
                if (lacks_source(H->lev[l].box[k], mp)) { suhmo_set_error("use_moulin_source without a moulin source term (suhmo_hier_moulin_source)"); return -1; }
        }
    }
    suhmo_level *base = base_of(H);
    if (strip_without_hooks(base)) { suhmo_set_error("time step on rank strips needs the exchange hooks on level 0"); return -1; }
    if (H->track_old_volume && (rc = suhmo_hier_track_volume_(H, (hipStream_t)s))) return rc;       // "WATER BUDGET": the volume the step starts from
    BoxUnions y{H, nlev, base, (hipStream_t)s};
    return timestep_fas(y, mp, dt, cur_step, picard_iters, vcycles);
}
