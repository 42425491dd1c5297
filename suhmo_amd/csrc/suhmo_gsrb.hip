// suhmo_gsrb.hip -- nonlinear variable-coefficient Gauss-Seidel red-black relaxation.
//
// Replaces VCAMRNonLinearPoissonOp::levelGSRB (src/VCAMRNonLinearPoissonOp.cpp:654-760):
//   per colour pass: exchange -> mixBCValues -> NonLinear_level -> GSRBHELMHOLTZVCNL2D
// The physical BC is evaluated on the fly, the nonlinear term and its derivative
// (COMPUTENONLINEARTERMS, src/AmrHydroF.ChF:23-68) and the relaxation coefficient lambda
// (SUMFACESNL, ...OpF.ChF:574-601) are recomputed in registers, so per sweep only phi, rhs,
// bx, by, B, Pi, zb, mask stream through HBM (72 B per cell per sweep).
// Colour rule: cell (i,j) is updated in pass p iff (i + j_global + p) is even
// (src/VCAMRNonLinearPoissonOpF.ChF:121-129).  GSRB is colour-Jacobi, so the result does not
// depend on the box decomposition: the kernels work on the whole level canvas.
//
// Two kernels:
//   k_gsrb_pass_simple   one launch per colour pass, one thread per active cell (small /
//                        odd-sized depths; also the structural reference for the fused one)
//   k_gsrb_fused<K>      K full sweeps (2K colour passes) in ONE pass over HBM: each
//                        workgroup owns a column strip x row chunk and marches down the rows
//                        with a (2K+3)-row ring of phi in LDS; row r-m is advanced from
//                        half-sweep m-1 to m while row r+1 is being prefetched, and row r-2K
//                        (all 2K half-sweeps done) is streamed out.  Halos of 2K cells are
//                        recomputed redundantly, output goes to a second phi buffer (ping-
//                        pong) so no workgroup ever reads a neighbour's updated cell.
#include "suhmo_hier.h"
#include "suhmo_batch.h"
#include "suhmo_relax_plan.h"
#include <type_traits>

// ---- variant 0: one thread per active-colour cell ----
// PUSH (boxes of a multi-box level): a cell on the side of its box also stores its new value into the ghost cell of the box
// across that side (push[pbase + side cell] = {box, canvas offset}, box < 0: none), so the next colour pass needs no
// Copier::exchange launch in between: a ghost cell of colour c is read only by the pass of the other colour.
template <bool HAS_ALPHA>
__device__ __forceinline__ void d_gsrb_pass_simple(const DV &v, const FP &fp, suhmo_phys_t ph, int pass, int jlo, int jhi,
                                                   const FP *__restrict__ ft = nullptr, const int2 *__restrict__ push = nullptr)
{
    // rows [jlo, jhi]: the strip's own rows plus, on rank boundaries, the halo rows that are
    // still fresh enough to be advanced redundantly (one exchange then feeds several passes)
    int j = jlo + (int)(blockIdx.y * blockDim.y + threadIdx.y);
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > jhi) return;
    int i = 2 * t + ((j + v.j0 + pass) & 1);
    if (i >= v.nx) return;
    double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    int idx = cidx(v, i, j);
    double c = phi[idx];
    double e = phiE(v, phi, idx, i, c, false), w = phiW(v, phi, idx, i, c, false);
    double n = phiN(v, phi, idx, j, c, false), s = phiS(v, phi, idx, j, c, false);
    double bxW = fp.f[SUHMO_F_BX][idx], bxE = fp.f[SUHMO_F_BX][idx + 1];
    double byS = fp.f[SUHMO_F_BY][idx], byN = fp.f[SUHMO_F_BY][idx + v.P];
    double nl, dnl;
    nl_terms(ph, c, fp.f[SUHMO_F_B][idx], fp.f[SUHMO_F_PI][idx], fp.f[SUHMO_F_ZB][idx],
             fp.f[SUHMO_F_MASK][idx], nl, dnl);
    double aterm = HAS_ALPHA ? v.alpha * fp.f[SUHMO_F_ACOEF][idx] : v.alpha;
    double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, byN, byS, nl);
    double lam = lambda_cell(v, aterm, bxE, bxW, byN, byS);
    double denom = 1.0e-16 + lam + dnl;                      // ...OpF.ChF:154
    const double pnew = c + (fp.f[SUHMO_F_RHS][idx] - lofphi) / denom; // :156
    phi[idx] = pnew;
    if (push) {                                               // sides in the order W, E (ny cells each), S, N (nx cells each)
        if (i == 0) { int2 q = push[j]; if (q.x >= 0) ft[q.x].f[SUHMO_F_PHI][q.y] = pnew; }
        if (i == v.nx - 1) { int2 q = push[v.ny + j]; if (q.x >= 0) ft[q.x].f[SUHMO_F_PHI][q.y] = pnew; }
        if (j == 0) { int2 q = push[2 * v.ny + i]; if (q.x >= 0) ft[q.x].f[SUHMO_F_PHI][q.y] = pnew; }
        if (j == v.ny - 1) { int2 q = push[2 * v.ny + v.nx + i]; if (q.x >= 0) ft[q.x].f[SUHMO_F_PHI][q.y] = pnew; }
    }
}
// rows [-lo, ny - 1 + hi] of a target.  push / pbase: the boxes' push tables (a target without a pointer table pushes nowhere)
template <class T, bool HAS_ALPHA>
__global__ __launch_bounds__(256) void k_gsrb_pass_simple(T t, int pass, int lo, int hi, const int2 *__restrict__ push, const int *__restrict__ pbase)
{
    const DV &v = t.view();
    const FP *ft = t.table();
    d_gsrb_pass_simple<HAS_ALPHA>(v, t.fields(), t.phys(), pass, -lo, v.ny - 1 + hi, ft, ft && push ? push + pbase[blockIdx.z] : nullptr);
}
template <class T> int launch_colour_pass(const T &t, bool has_alpha, int pass, int lo, int hi, const void *push, const int *pbase, hipStream_t st)
{
    const dim3 grd = grid2d((t.nx() + 1) / 2, t.ny() + lo + hi);
    if (has_alpha) return launch_grid(k_gsrb_pass_simple<T, true>, t, grd, BLK2D, st, pass, lo, hi, (const int2 *)push, pbase);
    return launch_grid(k_gsrb_pass_simple<T, false>, t, grd, BLK2D, st, pass, lo, hi, (const int2 *)push, pbase);
}
template int launch_colour_pass(const OnBoxes &, bool, int, int, int, const void *, const int *, hipStream_t);
template int launch_colour_pass(const OnMembers &, bool, int, int, int, const void *, const int *, hipStream_t);

static int launch_simple(suhmo_level *L, int depth, int pass, int ext_rows, hipStream_t st)
{
    const DV &v = L->d[depth].v;
    return launch_colour_pass(on_level(L, depth), v.alpha != 0.0, pass, v.rk[0] ? ext_rows : 0, v.rk[1] ? ext_rows : 0, nullptr, nullptr, st);
}

// one colour pass of one box of a multi-box AMR level (suhmo_hier.hip): in place, the ghost ring holds exchanged /
// interpolated data
int suhmo_gsrb_colour_pass(suhmo_level *L, int depth, int pass, hipStream_t st)
{
    int rc = launch_simple(L, depth, pass, 0, st); if (rc) return rc;
    L->d[depth].phi_fresh = 0;
    return 0;
}

// ---- levels that are UNIONS OF BOXES: several sweeps per launch (relaxNF, src/AMRNonLinearPoissonOp.cpp:690-750; levelGSRB :654-760).
// A workgroup owns a tile of a box and loads it with a halo of G = 4 or 8 cells -- the cells of the neighbouring boxes, taken from THEIR canvases (plan
// `halo`: for every position of the extended box the box that holds the cell and its canvas offset, or none) -- into LDS, advances the halo
// cells redundantly (pass m keeps what lies within 3 - m cells of the box current) and after 2 sweeps = 4 colour passes writes the box to the
// second canvas of the head.  What a cell reads beyond the cells of the level is what its OWN box's ghost ring says: the stored coarse-fine
// ghost (interpolated before the relaxation, constant during it) or the physical boundary condition of its side, evaluated with that box's
// view -- at a re-entrant corner of the union a position is the x-ghost of one box and the y-ghost of another, and each reader gets its own.
// Every update is d_gsrb_pass_simple's expression on the same operands in the same order, so the result is the colour passes' with an
// exchange before each, bit for bit; a launch reads canvases no workgroup of the launch writes (PHI -> PHI2, then PHI2 -> PHI).
// G: the halo the launch advances through = the sweeps it can do (G = 4: two sweeps; G = 8: FOUR sweeps -- a whole pre- or post-smoothing of the
// reference's num_smooth = 4 -- in one launch: the eight passes cost less than two launches' fixed parts).  T: the tile edge at most (a box is cut
// into ceil(n / T) tiles of equal width per direction).  Threads keep S positions of EACH colour of the tile's image.  What runs is T = 16, S = 1
// (320 / 512 threads): many small workgroups.  Measured and not kept: T = 32, S = 2 (48 x 48 image on 576 threads, 168 VGPRs) -- a 28 x 28 box as
// four tiles with their halos is 3600 positions and as one tile 1936, but cfg5's ~200 boxes per level do not fill 256 CUs with one workgroup each
// and a wave with two updates per pass has twice the dependent chain: 20.5 against 16.8 ms per step; on one box of 1024 x 256 cells 3.22 against
// 3.32 ms per step, within the box-to-box noise (`profiles/r04_w_box_tile_ab.txt`).  The plan `halo` is laid out for SUHMO_BOX_HALO = 8 cells around every box.
template <int G, int T, int S> struct BoxGeom { static constexpr int LW = T + 2 * G, NT = (((LW * LW / 2 + S - 1) / S + 63) / 64) * 64; };
template <bool HAS_ALPHA, int G, int T, int S>
__global__ __launch_bounds__((BoxGeom<G, T, S>::NT)) __attribute__((amdgpu_waves_per_eu(1, 3))) void k_gsrb_box_m(const DV *__restrict__ vt,
    const FP *__restrict__ ft, const int2 *__restrict__ halo, const int *__restrict__ hbase,
                                                                     suhmo_phys_t ph, int fsrc, int fdst, int npass, int bcg)
{
    constexpr int BOXG = G, BOXNT = BoxGeom<G, T, S>::NT, HG = SUHMO_BOX_HALO;
    constexpr int LWmax = T + 2 * BOXG;
    __shared__ double pl[LWmax * LWmax];
    __shared__ int own[LWmax * LWmax];
    const int k = blockIdx.y, tid = threadIdx.x;
    const DV &v = vt[k];                                               // (uniform: scalar loads, not a copy per lane)
    const int tiles_x = (v.nx + T - 1) / T, tiles_y = (v.ny + T - 1) / T;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int tj = blockIdx.x / tiles_x, ti = blockIdx.x - tj * tiles_x;
    const int twb = (v.nx + tiles_x - 1) / tiles_x, thb = (v.ny + tiles_y - 1) / tiles_y;      // tiles of equal size (the last one may be smaller)
    const int x0 = ti * twb, y0 = tj * thb;                            // the tile's first cell in the box = its halo's first position in the extended box
    const int tw = min(twb, v.nx - x0), th = min(thb, v.ny - y0);
    if (tw <= 0 || th <= 0) return;
    const int LW = tw + 2 * BOXG, LH = th + 2 * BOXG, EW = v.nx + 2 * HG, HW = (LW + 1) / 2;
    const int2 *__restrict__ hk = halo + hbase[k];
    const FP &fk = ft[k];
    // A thread keeps S positions of each colour of the tile's image through all passes (slot [s][c]: (i + j) & 1 == c, global indices; the colour
    // of a position follows from where the image lies, a periodic image keeps its parity), with everything about it that does not change: the
    // cell's box and offset, its coefficients, how far from the tile it lies.  A pass runs the slots of its colour: no lane idles for its colour.
    // One load phase of three dependent steps: the plan entry -> the box's view and field pointers (its own box: none) -> head and coefficients.
    const int par0 = (v.i0 + x0 - BOXG + v.j0 + y0 - BOXG) & 1;          // colour of the image's position (0, 0)
    int cq[S][2], cb[S][2], co[S][2], cd[S][2];    // position in the image (-1: none), box (-1: not advanced), canvas offset, distance from the tile
    double c_rhs[S][2], c_bxW[S][2], c_bxE[S][2], c_byS[S][2], c_byN[S][2], c_B[S][2], c_Pi[S][2], c_zb[S][2], c_mk[S][2], c_at[S][2];
    int2 hq[S][2];
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            cq[s][c] = -1; hq[s][c] = int2{-1, 0};
            const int p = tid + s * BOXNT;
            if (p < LH * HW) {
                const int lj = p / HW, li = 2 * (p - lj * HW) + ((lj + par0 + c) & 1);
                if (li < LW) { cq[s][c] = lj * LW + li; hq[s][c] = hk[(y0 + lj + HG - BOXG) * EW + x0 + li + HG - BOXG]; }
            }
        }
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int q = cq[s][c];
            cb[s][c] = -1; co[s][c] = 0; cd[s][c] = 0;
            c_rhs[s][c] = c_bxW[s][c] = c_bxE[s][c] = c_byS[s][c] = c_byN[s][c] = c_B[s][c] = c_Pi[s][c] = c_zb[s][c] = c_mk[s][c] = c_at[s][c] = 0.0;
            if (q < 0) continue;
            const int b = hq[s][c].x, off = hq[s][c].y;
            own[q] = b;
            if (b < 0) { pl[q] = 0.0; continue; }
            const int lj = q / LW, li = q - lj * LW;
            const int dx = li < BOXG ? BOXG - li : (li >= BOXG + tw ? li - (BOXG + tw - 1) : 0), dy = lj < BOXG ? BOXG - lj : (lj >= BOXG + th ? lj - (BOXG + th - 1) : 0);
            const int d = max(dx, dy);
            const FP &fb = b == k ? fk : ft[b];
            if (d >= BOXG) { pl[q] = fb.f[fsrc][off]; continue; }        // (the outermost ring is only read)
            const int Pb = b == k ? v.P : vt[b].P;
            cb[s][c] = b; co[s][c] = off; cd[s][c] = d;
            pl[q] = fb.f[fsrc][off];
            c_rhs[s][c] = fb.f[SUHMO_F_RHS][off];
            c_bxW[s][c] = fb.f[SUHMO_F_BX][off]; c_bxE[s][c] = fb.f[SUHMO_F_BX][off + 1];
            c_byS[s][c] = fb.f[SUHMO_F_BY][off]; c_byN[s][c] = fb.f[SUHMO_F_BY][off + Pb];
            c_B[s][c] = fb.f[SUHMO_F_B][off]; c_Pi[s][c] = fb.f[SUHMO_F_PI][off]; c_zb[s][c] = fb.f[SUHMO_F_ZB][off]; c_mk[s][c] = fb.f[SUHMO_F_MASK][off];
            c_at[s][c] = HAS_ALPHA ? v.alpha * fb.f[SUHMO_F_ACOEF][off] : v.alpha;      // (alpha, beta, the cell sizes and the BC data are the level's: every box's view has them)
        }
    __syncthreads();
    // What a cell reads beyond the cells of the level does not change during the launch: its own box's stored ghost (coarse-fine: interpolated before
    // the relaxation) or a physical boundary condition of its own value.  Worked out ONCE per position -- the box's view, the cell's indices, the ghost
    // value: global loads and an index computation that used to sit in every pass of every wave with a cell next to the level's edge -- as a kind per
    // direction (2 bits each: 0 a cell of the level, read from LDS; 1 the constant g; 2 g - c, Dirichlet: g = 2 x value; 3 c + g, Neumann: g = +-dx x
    // value: phiW / phiE / phiS / phiN's expressions) and the four g.
    int nk[S][2];
    double hW[S][2], hE[S][2], hS[S][2], hN[S][2];
#pragma unroll
    for (int s = 0; s < S; s++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            nk[s][c] = 0; hW[s][c] = hE[s][c] = hS[s][c] = hN[s][c] = 0.0;
            const int q = cq[s][c], b = cb[s][c];
            if (b < 0) continue;
            const bool oW = own[q - 1] < 0, oE = own[q + 1] < 0, oS = own[q - LW] < 0, oN = own[q + LW] < 0;
            if (!(oW || oE || oS || oN)) continue;
            const DV &vb = b == k ? v : vt[b];
            const double *__restrict__ psrc = (b == k ? fk : ft[b]).f[fsrc];
            const int off = co[s][c];
            // (a neighbour that is not a cell of the level lies outside the cell's own box: i == 0 / nx - 1 / j == 0 / ny - 1 there; a box that is its own
            //  periodic neighbour has its images in the plan as cells of the level)
            if (oW) { if (vb.cfx[0]) { nk[s][c] |= 1; hW[s][c] = psrc[off - 1]; } else if (vb.bct[0][0] == 0) { nk[s][c] |= 2; hW[s][c] = vb.two_v[0][0];
                } else { nk[s][c] |= 3; hW[s][c] = vb.neu[0][0]; } }
            if (oE) { if (vb.cfx[1]) { nk[s][c] |= 1 << 2; hE[s][c] = psrc[off + 1]; } else if (vb.bct[0][1] == 0) { nk[s][c] |= 2 << 2; hE[s][c] = vb.two_v[0][1];
                } else { nk[s][c] |= 3 << 2; hE[s][c] = vb.neu[0][1]; } }
            if (oS) { if (vb.ext[0]) { nk[s][c] |= 1 << 4; hS[s][c] = psrc[off - vb.P]; } else if (vb.bct[1][0] == 0) { nk[s][c] |= 2 << 4;
                hS[s][c] = vb.two_v[1][0]; } else { nk[s][c] |= 3 << 4; hS[s][c] = vb.neu[1][0]; } }
            if (oN) { if (vb.ext[1]) { nk[s][c] |= 1 << 6; hN[s][c] = psrc[off + vb.P]; } else if (vb.bct[1][1] == 0) { nk[s][c] |= 2 << 6;
                hN[s][c] = vb.two_v[1][1]; } else { nk[s][c] |= 3 << 6; hN[s][c] = vb.neu[1][1]; } }
        }
    auto outside = [](int kind, double g, double c) { return kind == 1 ? g : (kind == 2 ? g - c : c + g); };
    // one update: d_gsrb_pass_simple's expression.  Called with CONSTANT slot indices from either branch of the (uniform) colour test below: a
    // `u ? x[1] : x[0]` on the slot arrays is turned into a variably indexed load by the optimiser, which keeps all of them in scratch
    auto update = [&](int q, int kinds, double g_w, double g_e, double g_s, double g_n, double rhs, double bxW, double bxE, double byS, double byN, double B,
        double Pi, double zb, double mk, double at) {
        const double c = pl[q];
        // a neighbour that is a cell of the level: its current value; else what the cell's own box holds there (coarse-fine ghost / physical BC)
        double w, e, sv, n;
        if (kinds == 0) { w = pl[q - 1]; e = pl[q + 1]; sv = pl[q - LW]; n = pl[q + LW]; }
        else {
            w = (kinds & 3) ? outside(kinds & 3, g_w, c) : pl[q - 1];
            e = ((kinds >> 2) & 3) ? outside((kinds >> 2) & 3, g_e, c) : pl[q + 1];
            sv = ((kinds >> 4) & 3) ? outside((kinds >> 4) & 3, g_s, c) : pl[q - LW];
            n = ((kinds >> 6) & 3) ? outside((kinds >> 6) & 3, g_n, c) : pl[q + LW];
        }
        double nl, dnl;
        nl_terms(ph, c, B, Pi, zb, mk, nl, dnl);
        const double lofphi = lofphi_cell(v, at, c, e, w, n, sv, bxE, bxW, byN, byS, nl);
        const double lam = lambda_cell(v, at, bxE, bxW, byN, byS);
        const double denom = 1.0e-16 + lam + dnl;                      // ...OpF.ChF:154
        pl[q] = c + (rhs - lofphi) / denom;                            // :156 (a cell of one colour reads cells of the other only: in place)
    };
    for (int m = 0; m < npass; m++) {
        const int reach = npass - 1 - m;                               // the pass advances the cells of colour m & 1 within `reach` of the tile
        if ((m & 1) == 0) {
#pragma unroll
            for (int s = 0; s < S; s++)
                if (cb[s][0] >= 0 && cd[s][0] <= reach)
                    update(cq[s][0], nk[s][0], hW[s][0], hE[s][0], hS[s][0], hN[s][0], c_rhs[s][0], c_bxW[s][0], c_bxE[s][0], c_byS[s][0], c_byN[s][0], c_B[s][0],
                        c_Pi[s][0], c_zb[s][0], c_mk[s][0], c_at[s][0]);
        } else {
#pragma unroll
            for (int s = 0; s < S; s++)
                if (cb[s][1] >= 0 && cd[s][1] <= reach)
                    update(cq[s][1], nk[s][1], hW[s][1], hE[s][1], hS[s][1], hN[s][1], c_rhs[s][1], c_bxW[s][1], c_bxE[s][1], c_byS[s][1], c_byN[s][1], c_B[s][1],
                        c_Pi[s][1], c_zb[s][1], c_mk[s][1], c_at[s][1]);
        }
        __syncthreads();
    }
    // the tile to the second canvas; the box's ghost ring goes along unchanged (first tile): the coarse-fine ghosts stay what they are, the
    // fine-fine ones are not read by this kernel and are refreshed by the next exchange
    const double *__restrict__ psrc = fk.f[fsrc];
    double *__restrict__ pdst = fk.f[fdst];
    // bcg: the ghost cells beyond the box's PHYSICAL sides get the homogeneous boundary condition of the final values as well (levelGSRB's closing
    // fill, src/AMRNonLinearPoissonOp.cpp:757-759; d_fill_ghosts' expression on the same operand) instead of a launch of their own; the caller sets
    // it only when no box of the level is its own periodic neighbour (that ghost would be another tile's cell)
    const bool gW = bcg && !v.cfx[0] && !v.per[0], gE = bcg && !v.cfx[1] && !v.per[0], gS = bcg && !v.ext[0] && !v.per[1], gN = bcg && !v.ext[1] && !v.per[1];
    for (int q = tid; q < tw * th; q += BOXNT) {
        const int jj = q / tw, ii = q - jj * tw, gi = x0 + ii, gj = y0 + jj, idx = cidx(v, gi, gj);
        const double c = pl[(BOXG + jj) * LW + BOXG + ii];
        pdst[idx] = c;
        if (gW && gi == 0) pdst[idx - 1] = phiW(v, pdst, idx, gi, c, true);
        if (gE && gi == v.nx - 1) pdst[idx + 1] = phiE(v, pdst, idx, gi, c, true);
        if (gS && gj == 0) pdst[idx - v.P] = phiS(v, pdst, idx, gj, c, true);
        if (gN && gj == v.ny - 1) pdst[idx + v.P] = phiN(v, pdst, idx, gj, c, true);
    }
    if (blockIdx.x == 0)
        for (int q = tid; q < 2 * (v.nx + 2) + 2 * v.ny; q += BOXNT) {
            int ii, jj;
            bool filled;                                                // (a side cell the loop above writes)
            if (q < v.nx + 2) { ii = q - 1; jj = -1; filled = gS && ii >= 0 && ii < v.nx; }
            else if (q < 2 * (v.nx + 2)) { ii = q - (v.nx + 2) - 1; jj = v.ny; filled = gN && ii >= 0 && ii < v.nx; }
            else if (q < 2 * (v.nx + 2) + v.ny) { ii = -1; jj = q - 2 * (v.nx + 2); filled = gW; }
            else { ii = v.nx; jj = q - 2 * (v.nx + 2) - v.ny; filled = gE; }
            if (filled) continue;
            const int idx = cidx(v, ii, jj);
            pdst[idx] = psrc[idx];
        }
}
// `npass` colour passes (up to 8 = 4 sweeps) of every box of the level in one launch, fsrc -> fdst
template <int G, int T, int S>
static void launch_box(const suhmo_multi &m, const suhmo_phys_t &ph, bool has_alpha, const void *halo, const int *hbase, int fsrc, int fdst, int npass, int bc_ghosts, hipStream_t st)
{
    const dim3 grd(((m.maxnx + T - 1) / T) * ((m.maxny + T - 1) / T), m.nbox);
    if (has_alpha) hipLaunchKernelGGL((k_gsrb_box_m<true, G, T, S>), grd, dim3(BoxGeom<G, T, S>::NT), 0, st, m.dv, m.fp, (const int2 *)halo, hbase, ph, fsrc, fdst, npass, bc_ghosts);
    else hipLaunchKernelGGL((k_gsrb_box_m<false, G, T, S>), grd, dim3(BoxGeom<G, T, S>::NT), 0, st, m.dv, m.fp, (const int2 *)halo, hbase, ph, fsrc, fdst, npass, bc_ghosts);
}
int suhmo_multi_gsrb_box(const suhmo_multi &m, const suhmo_phys_t &ph, bool has_alpha, const void *halo, const int *hbase, int fsrc, int fdst, int npass, int bc_ghosts, hipStream_t st)
{
    if (m.nbox <= 0) return 0;
    if (npass < 1 || npass > 2 * SUHMO_BOX_HALO) { suhmo_set_error("internal: %d colour passes in one box launch", npass); return -4; }
    if (npass > 4) launch_box<8, 16, 1>(m, ph, has_alpha, halo, hbase, fsrc, fdst, npass, bc_ghosts, st);
    else launch_box<4, 16, 1>(m, ph, has_alpha, halo, hbase, fsrc, fdst, npass, bc_ghosts, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- variant 1: K sweeps fused, streaming over rows ----
struct FusedGeom {
    int W;        // owned columns per strip (even)
    int Hc;       // owned rows per chunk
    int nstrips, nchunks, ntiles;
    int ylo, yhi; // rows that exist for loading / computing (strip-local j, inclusive)
    int jbeg, jend; // rows written: [jbeg, jend) = the strip's rows plus, on rank boundaries, the halo rows that
                    // stay valid after this launch (advanced redundantly so the next launch needs no exchange)
    int wrap_y;   // rows outside [0, ny) are periodic images (single-rank periodic y)
    const unsigned *negflag; unsigned mask_epoch;   // *negflag == mask_epoch: the ice mask has a negative cell (k_bcoef_fused of this V-cycle); NULL: read the mask
    int nchl, chunk0, chunk1, edges;   // chunks of THIS launch: nchl of them starting at chunk0, or (edges) all but [chunk0, chunk1) --
                               // a rank strip relaxes its inner chunks while the halo rows travel, the end chunks afterwards
    // FAS prolongIncrement fused into the load of phi (PROLONGNL, AMRNonLinearPoissonOpF.ChF:619-627):
    // phi(i,j) += phi_c(i/2,j/2) - phi_c_old(i/2,j/2)
    const double *pc, *pco; int Pc, gyc;
    // RST: restrictResidual + restrictR fused into the launch that finishes the pre-smoothing: coarse RES / PHI canvases
    double *rres, *rphi; int rP, rgy;
    // FRHS: the first relaxation of a coarse FAS depth forms the depth's right-hand side rhs = res + L(R phi) itself (k_apply<., 2>'s
    // expressions on the rows as they are loaded) and stores it, L(phi) and the copy of R phi the prolongation subtracts later
    const double *fres; double *frhs, *flphi, *fphiold;
    // RM = 2: the launch that ends the cycle's post-smoothing leaves the residual of the final phi behind (the solve loop's residual
    // evaluation, k_apply<., 1> / <., 3>): RES = rtrue - L(phi), optionally L(phi) too; rtrue = the right-hand side the CALLER's residual is
    // about (inside an AMR cycle the level relaxes against its FAS right-hand side while the true one waits on the second canvas)
    const double *ortrue; double *ores, *olphi;
    double *onorm;      // ... and the chunk's max |RES| (one partial per strip x chunk: k_norm_partial's job, for k_norm_final); NULL: not asked for
    double zb_uniform;  // ZBU: the bed elevation of every cell of the depth (suhmo_common.h, "what is known about the bed")
};

// Cold uniform data of k_gsrb_fused<.., BCF>: what only a workgroup at a side of the level reads (the boundary types and values, the level's
// last row).  Carried through the row loop as kernel arguments by value it costs scalar registers the loop does not have: the launch that
// forms the faces is bound by its waves' instruction streams, and 62 spilled scalars were read back from vector lanes in every step.  So that
// instantiation reads them from the kernel-argument segment where they are used, inside the rare branch.  FusedArgs is the argument list as it
// lies there (every member is 8-byte aligned, as every argument is); the empty asm keeps the compiler from knowing the pointer, so the loads
// stay in the branch instead of moving in front of the loop.  The other instantiations gain nothing from it (measured) and
// keep the arguments by value.
struct FusedArgs { DV v; FP fp; const double *pin; double *pout; suhmo_phys_t ph; FusedGeom g; };
typedef const __attribute__((address_space(4))) FusedArgs *ColdArgs;
__device__ __forceinline__ ColdArgs cold_args()
{
    ColdArgs k = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return k;
}
// mixBCValues on the fly for one side (phiW / phiE / phiS / phiN, suhmo_common.h): the same expression on the same operands
struct SideBC { int t; double two_v, neu; };
template <bool COLD> __device__ __forceinline__ SideBC side_bc(const DV &v, const int d, const int s)
{
    SideBC b;
    if constexpr (COLD) { const ColdArgs k = cold_args(); b.t = k->v.bct[d][s]; b.two_v = k->v.two_v[d][s]; b.neu = k->v.neu[d][s]; }
    else { b.t = v.bct[d][s]; b.two_v = v.two_v[d][s]; b.neu = v.neu[d][s]; }
    return b;
}
__device__ __forceinline__ double bc_ghost(const SideBC &b, double c) { return (b.t == 0) ? b.two_v - c : c + b.neu; }

// MASKED = false: the level's ice mask is known clean (suhmo_common.h): the ring carries no mask, nothing loads, moves or tests it
template <bool MASKED> struct RowMask { double mask[2]; };
template <> struct RowMask<false> {};
// ZBU = true: the depth's bed elevation is known to be one value (suhmo_common.h): the ring carries no zb, nothing loads or moves it, and
// COMPUTENONLINEARTERMS gets the value itself (FusedGeom::zb_uniform: the same operand, so the same bits)
template <bool ZBU> struct RowZb { double zb[2]; };
template <> struct RowZb<true> {};
// YR = true: one ring of y-faces.  byN of row j IS byS of row j+1 (the same canvas row of by) wherever y is not periodic within the launch, so
// a row carries its north face only and a half-sweep takes the south face from the row below it in the ring: one load and two registers per
// row less (what the third wave per SIMD of the plain launch needs)
template <bool YR> struct RowByS { double byS[2]; };
template <> struct RowByS<true> {};
template <bool MASKED, bool ZBU = false, bool YR = false>
struct RowCoef : RowMask<MASKED>, RowZb<ZBU>, RowByS<YR> {          // per-thread coefficients of its column pair in one row
    double rhs[2], B[2], Pi[2], a[2], byN[2];
    double bx0, bx1, bx2;
};
template <bool MASKED, bool ZBU, bool YR> __device__ __forceinline__ double row_mask(const RowCoef<MASKED, ZBU, YR> &q, int a)
{
    if constexpr (MASKED) return q.mask[a]; else return 1.0;
}
template <bool MASKED, bool ZBU, bool YR> __device__ __forceinline__ double row_zb(const RowCoef<MASKED, ZBU, YR> &q, int a, const FusedGeom &g)
{
    if constexpr (ZBU) return g.zb_uniform; else return q.zb[a];
}
#define CP2(d, s, f) d.f[0] = s.f[0]; d.f[1] = s.f[1]
template <bool HAS_ALPHA, bool MASKED, bool ZBU, bool YR>
__device__ __forceinline__ void copy_coef(RowCoef<MASKED, ZBU, YR> &d, const RowCoef<MASKED, ZBU, YR> &s)
{
    CP2(d, s, rhs); CP2(d, s, B); CP2(d, s, Pi);
    if constexpr (!ZBU) { CP2(d, s, zb); }
    if constexpr (MASKED) { CP2(d, s, mask); }
    if (HAS_ALPHA) { CP2(d, s, a); }
    if constexpr (!YR) { CP2(d, s, byS); }
    CP2(d, s, byN);
    d.bx0 = s.bx0; d.bx1 = s.bx1; d.bx2 = s.bx2;
}

// RST = true: the launch also restricts.  Once row j-1, j, j+1 are final (all 2K half-sweeps), the residual rhs - L(phi) of
// row j is evaluated from the ring with the same expressions as k_restrict_residual and accumulated, in the reference's
// visiting order, into the coarse cell of the thread's column pair (RESTRICTRESVCNL2D + RESTRICTVCNL, VCAMR...OpF.ChF:480-561,
// 419-449): the separate pass over phi and the 8 coefficient arrays (75 B/cell) disappears.  Costs: one more ring row, one
// more coefficient row, one more final row above and below the chunk and two more halo columns per side.
// BCF = true: the launch is also the V-cycle's UpdateOperator of depth 0 (WFlx_level, suhmo_bcoef.hip): it loads no bx and no by but forms
// them from phi AS LOADED and stores them.  The half-sweeps run one step later, so that rows r, r-1, r-2 of the ring are still as loaded in
// step r: step r forms the cell-centred gradient of row r-1 (gx from the LDS row, gy from the lane's own column in rows r and r-2), its Re,
// the y-faces between rows r-2 and r-1 (byN of the row whose first half-sweep follows in the same step, byS of the next: computed once) and,
// after the step's first barrier -- Re goes through an LDS row so that a lane can read Re of the cells left and right of its pair, whose B it
// loaded with the row -- the row's x-faces.  Every value is gradcc_from / grad_norm / re_from / bcoef_face of k_bcoef_fused<.., MASKED = false>
// on the same operands: the ghost cells beyond a physical side get the gradient 2 g1 - g2 (k_grad_ghosts; in x both belong to the boundary
// lane's pair, in y the previous row's gradient waits in LDS) and the stored ghost B, the ghost cells of a periodic side the gradient
// of their image and the stored ghost B.  Costs: the geometry of the restricting launch (one more ring row and coefficient row, two more
// halo columns per side) and one more row of phi above and below a chunk; rhs, Pi and zb, which only the half-sweeps read, are loaded one
// step later than B (registers: 247, two waves per SIMD).  Every workgroup forms the faces of its halo cells itself, so no
// workgroup reads bx or by during the launch; owners store, the domain's last face column / row goes with the last strip / chunk.
template <int K, bool HAS_ALPHA, int NT, int RM = 0, bool FRHS = false, bool MASKED = true, bool BCF = false, bool ZBU = false, bool YR = false>
__global__ __launch_bounds__(NT) void k_gsrb_fused(DV v, FP fp, const double *__restrict__ pin,
                                                   double *__restrict__ pout, suhmo_phys_t ph, FusedGeom g)
{
    // RM: what the launch does with the final rows besides storing them: 0 nothing, 1 restricts (RST), 2 stores their residual (ROUT)
    constexpr bool ROUT = RM == 2, RR = RM != 0;
    static_assert(!(FRHS && (RR || HAS_ALPHA)), "the right-hand side is formed in the plain launch of an alpha = 0 operator");
    static_assert(!BCF || (K == 2 && NT == 64 && RM == 0 && !FRHS && !HAS_ALPHA && !MASKED), "the faces are formed in the plain two-sweep launch of a clean-mask alpha = 0 operator");
    static_assert(!ZBU || (K == 2 && NT == 64 && !HAS_ALPHA && !MASKED), "the bed as a scalar: the two-sweep launches of a clean-mask alpha = 0 operator");
    static_assert(!YR || (ZBU && RM == 0 && !FRHS && !BCF), "one ring of y-faces: the plain two-sweep launch with the bed as a scalar");
    constexpr bool WIDE = RR || BCF;           // one more ring row and coefficient row, two more halo columns per side
    constexpr int DL = BCF ? 1 : 0;            // steps the half-sweeps (and the output) lag behind
    constexpr int LW = 2 * NT, R = 2 * K + 3 + (WIDE ? 1 : 0);
    constexpr int HX = 2 * K + (WIDE ? 2 : 0), EY = RR ? 1 : 0;
    __shared__ double lds[R * LW];
    __shared__ double rre[BCF ? LW : 1], rsg[BCF ? LW : 1];      // BCF: Re and |grad| of the row whose faces are being formed
    __shared__ double2 gpv[BCF ? 2 * NT : 1];                    // BCF: every lane's gradient of the row below (read at the level's y sides only: not worth registers)

    // XCD-aware tile order: blocks are dealt round-robin over the 8 XCDs; give every XCD a
    // contiguous range of tiles (adjacent chunks of one strip share 2K halo rows in its L2).
    int b = blockIdx.x, q = g.ntiles / 8, rem = g.ntiles % 8, xcd = b % 8;
    int tile = xcd * q + (xcd < rem ? xcd : rem) + b / 8;
    int strip = tile / g.nchl, chunk = tile % g.nchl;
    chunk = g.edges ? (chunk < g.chunk0 ? chunk : g.chunk1 + (chunk - g.chunk0)) : g.chunk0 + chunk;

    const int t = threadIdx.x;
    const int c0 = strip * g.W;
    const int xl = 2 * t;                      // position of the pair's first cell in an LDS row
    const int i0 = c0 - HX + xl;               // its global column (even)
    const bool in_row = xl < g.W + 2 * HX;
    int im = i0;
    if (v.per[0]) { if (im < 0) im += v.nx; else if (im >= v.nx) im -= v.nx; }
    const bool cval = in_row && im >= 0 && im < v.nx;                 // pair lies in the domain
    const int cend = (c0 + g.W < v.nx) ? c0 + g.W : v.nx;
    const bool own = cval && i0 >= c0 && i0 < cend;

    const int jA = g.jbeg + chunk * g.Hc;
    const int jB = (jA + g.Hc < g.jend) ? jA + g.Hc : g.jend;
    const int jmin = (jA - EY - 2 * K > g.ylo) ? jA - EY - 2 * K : g.ylo;
    const int jmax = (jB - 1 + EY + 2 * K < g.yhi) ? jB - 1 + EY + 2 * K : g.yhi;

    const double *__restrict__ f_rhs = fp.f[SUHMO_F_RHS], *__restrict__ f_B = fp.f[SUHMO_F_B];
    const double *__restrict__ f_Pi = fp.f[SUHMO_F_PI], *__restrict__ f_zb = fp.f[SUHMO_F_ZB];
    const double *__restrict__ f_mask = fp.f[SUHMO_F_MASK], *__restrict__ f_a = fp.f[SUHMO_F_ACOEF];
    const double *__restrict__ f_bx = fp.f[SUHMO_F_BX], *__restrict__ f_by = fp.f[SUHMO_F_BY];
    // BCF (a whole level: no stored halo rows): phi is loaded one row further than the rows that are advanced, where the level has one
    const int jminP = BCF ? ((g.wrap_y || jmin > 0) ? jmin - 1 : jmin) : jmin;
    const int jmaxP = BCF ? ((g.wrap_y || jmax < v.ny - 1) ? jmax + 1 : jmax) : jmax;

    auto wrapj = [&](int j) { if (g.wrap_y) { if (j < 0) j += v.ny; else if (j >= v.ny) j -= v.ny; } return j; };
    auto ld2 = [&](const double *__restrict__ p, int idx) { return *reinterpret_cast<const double2 *>(p + idx); };

    // coefficient ring as NAMED variables (an indexed array ends up in scratch memory):
    // cf0 = row r (being prefetched), cfM = row r-M
    RowCoef<MASKED, ZBU, YR> cf0, cf1, cf2, cf3, cf4, cf5;
    double ys5[2] = {0.0, 0.0};            // YR: the north face of row r-5, the south face of the oldest row that is still advanced
    double racc = 0.0, raccp = 0.0;        // RST: the coarse cell's sums after its first fine row
    double nmax = 0.0;                     // ROUT: max |RES| over this thread's cells of the chunk
    // physical-BC sides this tile can touch (uniform): skip the per-lane boundary tests elsewhere
    const bool xbc = !v.per[0] && (c0 - HX <= 0 || c0 + g.W + HX >= v.nx);
    const bool ybc = !v.per[1] && (jmin <= 0 || jmax >= v.ny - 1);
    double2 pnext = make_double2(0.0, 0.0);
    double2 pprev = make_double2(0.0, 0.0);    // FRHS: this thread's pair of the row below the one whose L(phi) is formed, as loaded
    // BCF: B of the cells left and right of the pair in rows r and r-1 (the stored ghost cell at a side of the level); Re of row r-1 and of
    // the row below it, that row's gradient; |grad| of the ghost cell beyond a physical x side
    double bw0 = 0.0, be0 = 0.0, bw1 = 0.0, be1 = 0.0, rn0 = 0.0, rn1 = 0.0, rep0 = 0.0, rep1 = 0.0, sgG = 0.0;
    const bool xedge = c0 - HX <= 0 || c0 + g.W + HX >= v.nx;      // (uniform) the strip holds a lane next to a side of the level, or its image
    // the mask array is 8 of the 80 bytes a cell costs per launch and only its sign is used: when this V-cycle's UpdateOperator saw
    // no negative cell the loads are skipped (uniform); MASKED = false: the host knows already, the word is not read either
    bool usemask = false;
    if constexpr (MASKED) usemask = !g.negflag || *g.negflag == g.mask_epoch;

    int sr = 0;                            // LDS ring slot of row r
    // slot of an earlier row: sr - m, m <= R -- a compare instead of a division by 7 (the kernel issues nearly as many scalar as vector
    // instructions: 290.7 against 294.7 us per launch, profiles/r03_i_ring_index_ab.txt; keeping the seven offsets in rotating scalars
    // instead: fewer instructions, more spilled scalars, the same time)
    auto ring = [](int x) { return x < 0 ? x + R : x; };
    for (int r = jminP - 1; r <= jB - 1 + 2 * K + EY + DL; r++) {
        // ---- 1. prefetch: phi of row r+1, coefficients of row r (both first used in step r+1)
        bool lphi = cval && (r + 1 >= jminP) && (r + 1 <= jmaxP);
        if (lphi) {
            const int jr = wrapj(r + 1);
            pnext = ld2(pin, cidx(v, im, jr));
            if (!BCF && g.pc) {            // (never on the launch that forms the faces: launch_fused refuses it)
                const int ic = ((jr >> 1) + g.gyc) * g.Pc + SUHMO_XOFF + (im >> 1);
                const double corr = 1.0 * g.pc[ic] + (-1.0) * g.pco[ic];      // axby(1, -1), then PROLONGNL
                pnext.x = pnext.x + corr; pnext.y = pnext.y + corr;
            }
        }
        bool lcf = cval && (r >= jmin) && (r <= jmax);
        if (lcf) {
            int idx = cidx(v, im, wrapj(r));
#define LD2(dst, p, ix) { double2 t_ = ld2(p, ix); dst[0] = t_.x; dst[1] = t_.y; }
            if constexpr (!BCF) { LD2(cf0.rhs, (FRHS ? g.fres : f_rhs), idx); LD2(cf0.Pi, f_Pi, idx); if constexpr (!ZBU) { LD2(cf0.zb, f_zb, idx); } }
            LD2(cf0.B, f_B, idx);
            if constexpr (MASKED) { if (usemask) { LD2(cf0.mask, f_mask, idx); } else { cf0.mask[0] = 1.0; cf0.mask[1] = 1.0; } }
            if (HAS_ALPHA) LD2(cf0.a, f_a, idx);
            if constexpr (BCF) { bw0 = f_B[idx - 1]; be0 = f_B[idx + 2]; }      // (the stored ghost cell at a side of the level)
            else {
                if constexpr (!YR) { LD2(cf0.byS, f_by, idx); }
                LD2(cf0.byN, f_by, idx + v.P);
                double2 bxp = ld2(f_bx, idx);
                cf0.bx0 = bxp.x; cf0.bx1 = bxp.y; cf0.bx2 = f_bx[idx + 2];
            }
        }
        if constexpr (YR) {
            // the chunk's first row has no loaded row below it: its south face, as that row's north face, one step early (launch_fused keeps
            // y-periodic levels off this instantiation: no canvas row is an image of another here, this one is row jmin of by)
            if (cval && r == jmin - 1) { LD2(cf0.byN, f_by, cidx(v, im, r) + v.P); }
        }
        if constexpr (BCF) {
            // what only the half-sweeps read comes a step later, with the row that is one step from its first half-sweep (registers)
            if (cval && (r - 1 >= jmin) && (r - 1 <= jmax)) {
                const int idx = cidx(v, im, wrapj(r - 1));
                LD2(cf1.rhs, f_rhs, idx); LD2(cf1.Pi, f_Pi, idx); if constexpr (!ZBU) { LD2(cf1.zb, f_zb, idx); }
            }
        }
        __syncthreads();                   // row r (written at the end of step r-1) is visible

        // ---- 1b. FRHS: rows r-2 (this thread's own pair, kept in pprev), r-1 and r are still as loaded: L(phi) of row r-1, its
        // right-hand side (used by the half-sweeps below: cf1 IS row r-1), and the three stores of k_apply<., 2> for the chunk's rows
        if constexpr (FRHS) {
            const int jf = r - 1;
            if (cval && jf >= jmin && jf <= jmax) {
                const int s0 = ring(sr - 1), sN = sr;
                const double *row = lds + s0 * LW;
                double lo[2], cc[2];
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int x = xl + a, i = im + a;
                    double c = row[x];
                    double w = row[(a == 0 && xl == 0) ? 0 : x - 1], e = row[(a == 1 && xl == LW - 2) ? LW - 1 : x + 1];
                    double n = lds[sN * LW + x], s = a ? pprev.y : pprev.x;
                    if (xbc) {
                        if (i == 0) w = (v.bct[0][0] == 0) ? v.two_v[0][0] - c : c + v.neu[0][0];
                        if (i == v.nx - 1) e = (v.bct[0][1] == 0) ? v.two_v[0][1] - c : c + v.neu[0][1];
                    }
                    if (ybc) {
                        if (jf == 0 && !v.ext[0]) s = (v.bct[1][0] == 0) ? v.two_v[1][0] - c : c + v.neu[1][0];
                        if (jf == v.ny - 1 && !v.ext[1]) n = (v.bct[1][1] == 0) ? v.two_v[1][1] - c : c + v.neu[1][1];
                    }
                    double nl, dnl;
                    nl_terms(ph, c, cf1.B[a], cf1.Pi[a], row_zb(cf1, a, g), row_mask(cf1, a), nl, dnl);
                    const double bxW = a ? cf1.bx1 : cf1.bx0, bxE = a ? cf1.bx2 : cf1.bx1;
                    lo[a] = lofphi_cell(v, v.alpha, c, e, w, n, s, bxE, bxW, cf1.byN[a], cf1.byS[a], nl);
                    cc[a] = c;
                }
                cf1.rhs[0] = 1.0 * cf1.rhs[0] + 1.0 * lo[0]; cf1.rhs[1] = 1.0 * cf1.rhs[1] + 1.0 * lo[1];
                // rank strip: the end chunks also keep what they formed in the halo rows they only read (the later launches of the depth
                // advance halo rows too and the prolongation corrects them): the right-hand side wherever both row neighbours were loaded,
                // R phi in every loaded row -- the rows k_apply<., 2> serves with hcomp = halo - 1
                const bool lo_end = v.ext[0] && chunk == 0, hi_end = v.ext[1] && chunk == g.nchunks - 1;
                const int jP0 = lo_end ? jmin : jA, jP1 = hi_end ? jmax + 1 : jB;
                const int jR0 = lo_end ? jmin + 1 : jA, jR1 = hi_end ? jmax : jB;
                if (own && jf >= jP0 && jf < jP1) {
                    const int idx = cidx(v, i0, jf);
                    if (jf >= jR0 && jf < jR1) {
                        *reinterpret_cast<double2 *>(g.flphi + idx) = make_double2(lo[0], lo[1]);
                        *reinterpret_cast<double2 *>(g.frhs + idx) = make_double2(cf1.rhs[0], cf1.rhs[1]);
                    }
                    *reinterpret_cast<double2 *>(g.fphiold + idx) = make_double2(cc[0], cc[1]);
                }
                pprev = make_double2(cc[0], cc[1]);            // row r-1 as loaded: the south neighbours of row r in the next step
            }
            __syncthreads();                                   // the half-sweep below overwrites cells of row r-1 that the neighbours read above
        }

        // ---- 2. advance row r-m from half-sweep m-1 to m, m = 1..2K
        // One half-sweep of row r-m.  The colour offset `a` (which cell of the pair is updated)
        // depends only on the row, so it is WAVE-UNIFORM: branch on it once (scalar branch) and
        // address the pair's coefficients statically instead of selecting per lane.
        auto advance_a = [&](const int m, const RowCoef<MASKED, ZBU, YR> &q, const double (&byS)[2], auto a_tag) {
            constexpr int a = decltype(a_tag)::value;
            const int j = r - m - DL;
            const int x = xl + a, i = im + a;
            const int s0 = ring(sr - m - DL), sN = ring(sr - m - DL + 1), sS = ring(sr - m - DL - 1);
            const double *row = lds + s0 * LW;
            double c = row[x];
            double w = row[(a == 0 && xl == 0) ? 0 : x - 1], e = row[(a == 1 && xl == LW - 2) ? LW - 1 : x + 1];
            double n = lds[sN * LW + x], s = lds[sS * LW + x];
            if (xbc) {                                         // mixBCValues on the fly (strip touches a BC side)
                const SideBC bW = side_bc<BCF>(v, 0, 0), bE = side_bc<BCF>(v, 0, 1);
                if (i == 0) w = bc_ghost(bW, c);
                if (i == v.nx - 1) e = bc_ghost(bE, c);
            }
            if (ybc) {                                         // (BCF: a whole level, no stored halo rows)
                if (j == 0 && (BCF || !v.ext[0])) s = bc_ghost(side_bc<BCF>(v, 1, 0), c);
                if (j == v.ny - 1 && (BCF || !v.ext[1])) n = bc_ghost(side_bc<BCF>(v, 1, 1), c);
            }
            double nl, dnl;
            nl_terms(ph, c, q.B[a], q.Pi[a], row_zb(q, a, g), row_mask(q, a), nl, dnl);
            const double bxW = a ? q.bx1 : q.bx0, bxE = a ? q.bx2 : q.bx1;
            double aterm = HAS_ALPHA ? v.alpha * q.a[a] : v.alpha;
            double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, q.byN[a], byS[a], nl);
            double lam = lambda_cell(v, aterm, bxE, bxW, q.byN[a], byS[a]);
            double denom = 1.0e-16 + lam + dnl;
            lds[s0 * LW + x] = c + (q.rhs[a] - lofphi) / denom;
        };
        // byS: the row's south faces -- its own, or (YR) the north faces of the row below it in the ring
        auto advance_s = [&](const int m, const RowCoef<MASKED, ZBU, YR> &q, const double (&byS)[2]) {
            const int j = r - m - DL;
            if (j >= jmin && j <= jmax) {                      // uniform
                const int a = (j + v.j0 + ((m - 1) & 1)) & 1;  // uniform: colour offset of this row
                if (a) { if (cval) advance_a(m, q, byS, std::integral_constant<int, 1>()); }
                else   { if (cval) advance_a(m, q, byS, std::integral_constant<int, 0>()); }
            }
        };
        auto advance = [&](const int m, const RowCoef<MASKED, ZBU, YR> &q, const RowCoef<MASKED, ZBU, YR> &below) {
            if constexpr (YR) advance_s(m, q, below.byN); else advance_s(m, q, q.byS);
        };
        if constexpr (BCF) {
            // ---- 1c / 2. the faces of row r-1 (cf1), around the half-sweeps of rows r-2 .. r-5 (cf2 .. cf5)
            const int j1 = r - 1;
            const bool faces = j1 >= jmin && j1 <= jmax;       // uniform
            double *__restrict__ o_bx = fp.f[SUHMO_F_BX], *__restrict__ o_by = fp.f[SUHMO_F_BY];
            if (faces && cval) {
                const double *row = lds + ring(sr - 1) * LW, *rowN = lds + sr * LW, *rowS = lds + ring(sr - 2) * LW;
                const double ca = row[xl], cb = row[xl + 1];
                double w = row[xl == 0 ? 0 : xl - 1], e = row[xl == LW - 2 ? LW - 1 : xl + 2];
                double na = rowN[xl], nb = rowN[xl + 1], sa = rowS[xl], sb = rowS[xl + 1];      // (the lane's own cells: row r-2 is advanced below)
                if (xbc) {                                     // phiW / phiE (.., false)
                    const SideBC bW = side_bc<true>(v, 0, 0), bE = side_bc<true>(v, 0, 1);
                    if (im == 0) w = bc_ghost(bW, ca);
                    if (im + 1 == v.nx - 1) e = bc_ghost(bE, cb);
                }
                if (ybc) {                                     // phiS / phiN (.., false)
                    if (j1 == 0) { const SideBC bS = side_bc<true>(v, 1, 0); sa = bc_ghost(bS, ca); sb = bc_ghost(bS, cb); }
                    if (j1 == v.ny - 1) { const SideBC bN = side_bc<true>(v, 1, 1); na = bc_ghost(bN, ca); nb = bc_ghost(bN, cb); }
                }
                double gx0, gy0, gx1, gy1;
                gradcc_from(v, ca, w, cb, sa, na, false, false, false, false, gx0, gy0);
                gradcc_from(v, cb, ca, e, sb, nb, false, false, false, false, gx1, gy1);
                const double sg0 = grad_norm(gx0, gy0), sg1 = grad_norm(gx1, gy1);
                rn0 = re_from(ph, sg0, cf1.B[0]); rn1 = re_from(ph, sg1, cf1.B[1]);
                *reinterpret_cast<double2 *>(rre + xl) = make_double2(rn0, rn1);
                if (xedge) {
                    // the cell beyond a side of the level in x: periodic -- the gradient of its image, read from the neighbour lane below;
                    // physical -- 2 g1 - g2 of the two cells next to the side, both this lane's
                    if (v.per[0]) *reinterpret_cast<double2 *>(rsg + xl) = make_double2(sg0, sg1);
                    else if (im == 0) sgG = grad_norm(2.0 * gx0 - gx1, 2.0 * gy0 - gy1);
                    else if (im == v.nx - 2) sgG = grad_norm(2.0 * gx1 - gx0, 2.0 * gy1 - gy0);
                }
                cf1.byN[0] = 0.0; cf1.byN[1] = 0.0;            // (set in the next step, or below at the level's top row)
                if (j1 > jmin) {                               // Re of the row below was formed in the previous step
                    cf1.byS[0] = bcoef_face(ph, rn0, rep0, cf1.B[0], cf2.B[0], 1.0, 1.0, false);
                    cf1.byS[1] = bcoef_face(ph, rn1, rep1, cf1.B[1], cf2.B[1], 1.0, 1.0, false);
                    cf2.byN[0] = cf1.byS[0]; cf2.byN[1] = cf1.byS[1];
                    double gxp0 = 0.0, gxp1 = 0.0, gyp0 = 0.0, gyp1 = 0.0;
                    if ((g.wrap_y && (j1 == 0 || j1 == v.ny)) || (ybc && (j1 == 1 || j1 == v.ny - 1))) {
                        const double2 px = gpv[t], py = gpv[NT + t];
                        gxp0 = px.x; gxp1 = px.y; gyp0 = py.x; gyp1 = py.y;
                    }
                    if (g.wrap_y && (j1 == 0 || j1 == v.ny)) {
                        // periodic seam: face 0 has the stored ghost row -1 below it, face ny the stored ghost row ny above it, each with the
                        // gradient of its image
                        const double2 bS = ld2(f_B, cidx(v, im, -1)), bN = ld2(f_B, cidx(v, im, v.ny));
                        const double sp0 = grad_norm(gxp0, gyp0), sp1 = grad_norm(gxp1, gyp1);
                        cf1.byS[0] = bcoef_face(ph, rn0, re_from(ph, sp0, bS.x), cf1.B[0], bS.x, 1.0, 1.0, false);
                        cf1.byS[1] = bcoef_face(ph, rn1, re_from(ph, sp1, bS.y), cf1.B[1], bS.y, 1.0, 1.0, false);
                        cf2.byN[0] = bcoef_face(ph, re_from(ph, sg0, bN.x), rep0, bN.x, cf2.B[0], 1.0, 1.0, false);
                        cf2.byN[1] = bcoef_face(ph, re_from(ph, sg1, bN.y), rep1, bN.y, cf2.B[1], 1.0, 1.0, false);
                        if (own && j1 == v.ny && jB == cold_args()->g.jend) *reinterpret_cast<double2 *>(o_by + cidx(v, i0, v.ny)) = make_double2(cf2.byN[0], cf2.byN[1]);
                    }
                    if (ybc && j1 == 1) {
                        // physical bottom: face 0 of row 0 (cf2), the ghost row's gradient 2 g(0) - g(1) and its stored B
                        const double2 bS = ld2(f_B, cidx(v, im, -1));
                        const double rg0 = re_from(ph, grad_norm(2.0 * gxp0 - gx0, 2.0 * gyp0 - gy0), bS.x);
                        const double rg1 = re_from(ph, grad_norm(2.0 * gxp1 - gx1, 2.0 * gyp1 - gy1), bS.y);
                        cf2.byS[0] = bcoef_face(ph, rep0, rg0, cf2.B[0], bS.x, 1.0, 1.0, false);
                        cf2.byS[1] = bcoef_face(ph, rep1, rg1, cf2.B[1], bS.y, 1.0, 1.0, false);
                        if (own && jA <= 0) *reinterpret_cast<double2 *>(o_by + cidx(v, i0, 0)) = make_double2(cf2.byS[0], cf2.byS[1]);
                    }
                    if (ybc && j1 == v.ny - 1) {
                        // physical top: face ny, the ghost row's gradient 2 g(ny-1) - g(ny-2) and its stored B
                        const double2 bN = ld2(f_B, cidx(v, im, v.ny));
                        const double rg0 = re_from(ph, grad_norm(2.0 * gx0 - gxp0, 2.0 * gy0 - gyp0), bN.x);
                        const double rg1 = re_from(ph, grad_norm(2.0 * gx1 - gxp1, 2.0 * gy1 - gyp1), bN.y);
                        cf1.byN[0] = bcoef_face(ph, rg0, rn0, bN.x, cf1.B[0], 1.0, 1.0, false);
                        cf1.byN[1] = bcoef_face(ph, rg1, rn1, bN.y, cf1.B[1], 1.0, 1.0, false);
                        if (own && jB == cold_args()->g.jend) *reinterpret_cast<double2 *>(o_by + cidx(v, i0, v.ny)) = make_double2(cf1.byN[0], cf1.byN[1]);
                    }
                    if (own && j1 >= jA && j1 < jB) *reinterpret_cast<double2 *>(o_by + cidx(v, i0, j1)) = make_double2(cf1.byS[0], cf1.byS[1]);
                } else { cf1.byS[0] = 0.0; cf1.byS[1] = 0.0; }      // (the chunk's first loaded row: at the level's bottom set one step later, else never valid)
                gpv[t] = make_double2(gx0, gx1); gpv[NT + t] = make_double2(gy0, gy1);
            }
            advance(1, cf2, cf3);
            __syncthreads();                   // (also: Re of row r-1 is visible)
            if (faces && cval) {
                double reW = rre[xl == 0 ? 0 : xl - 1], reE = rre[xl == LW - 2 ? LW - 1 : xl + 2];
                if (xedge) {
                    if (im == 0) reW = re_from(ph, v.per[0] ? rsg[xl == 0 ? 0 : xl - 1] : sgG, bw1);
                    if (im == v.nx - 2) reE = re_from(ph, v.per[0] ? rsg[xl == LW - 2 ? LW - 1 : xl + 2] : sgG, be1);
                }
                cf1.bx0 = bcoef_face(ph, rn0, reW, cf1.B[0], bw1, 1.0, 1.0, false);
                cf1.bx1 = bcoef_face(ph, rn1, rn0, cf1.B[1], cf1.B[0], 1.0, 1.0, false);
                cf1.bx2 = bcoef_face(ph, reE, rn1, be1, cf1.B[1], 1.0, 1.0, false);
                if (own && j1 >= jA && j1 < jB) {
                    const int idx = cidx(v, i0, j1);
                    *reinterpret_cast<double2 *>(o_bx + idx) = make_double2(cf1.bx0, cf1.bx1);
                    if (i0 == v.nx - 2) o_bx[idx + 2] = cf1.bx2;      // the level's last face column
                }
                rep0 = rn0; rep1 = rn1;
            }
            advance(2, cf3, cf4);
            __syncthreads();
            advance(3, cf4, cf5);
            __syncthreads();
            advance(4, cf5, cf5);              // (never YR: the row's own south faces)
        } else {
        advance(1, cf1, cf2);
        __syncthreads();
        advance(2, cf2, cf3);
        if constexpr (K >= 2) {
            __syncthreads();
            advance(3, cf3, cf4);
            __syncthreads();
            if constexpr (YR) advance_s(4, cf4, ys5); else advance(4, cf4, cf4);
        }
        }

        // ---- 2b. RST: rows r-2K-2 .. r-2K are final: residual of row r-2K-1, restricted
        if constexpr (RR) {
            const int jr = r - 2 * K - 1;
            if (own && jr >= jA && jr < jB && jr >= 0 && jr < v.ny) {    // (rank strips: halo rows are advanced, not restricted)
                const RowCoef<MASKED, ZBU, YR> &q = (K >= 2) ? cf5 : cf3;
                const int s0 = ring(sr - (2 * K + 1)), sN = ring(sr - 2 * K), sS = ring(sr - (2 * K + 2));
                const double *row = lds + s0 * LW;
                double acc = (jr & 1) ? racc : 0.0, accp = (jr & 1) ? raccp : 0.0;
                double lo2[2] = {0.0, 0.0};
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int x = xl + a, i = im + a;
                    double c = row[x], w = row[x - 1], e = row[x + 1];       // own pairs never sit on the edge of the LDS row (HX >= 2)
                    double n = lds[sN * LW + x], s = lds[sS * LW + x];
                    if (xbc) {
                        if (i == 0) w = (v.bct[0][0] == 0) ? v.two_v[0][0] - c : c + v.neu[0][0];
                        if (i == v.nx - 1) e = (v.bct[0][1] == 0) ? v.two_v[0][1] - c : c + v.neu[0][1];
                    }
                    if (ybc) {
                        if (jr == 0 && !v.ext[0]) s = (v.bct[1][0] == 0) ? v.two_v[1][0] - c : c + v.neu[1][0];
                        if (jr == v.ny - 1 && !v.ext[1]) n = (v.bct[1][1] == 0) ? v.two_v[1][1] - c : c + v.neu[1][1];
                    }
                    double nl, dnl;
                    nl_terms(ph, c, q.B[a], q.Pi[a], row_zb(q, a, g), row_mask(q, a), nl, dnl);
                    const double bxW = a ? q.bx1 : q.bx0, bxE = a ? q.bx2 : q.bx1;
                    double aterm = HAS_ALPHA ? v.alpha * q.a[a] : v.alpha;
                    double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, q.byN[a], q.byS[a], nl);
                    if constexpr (ROUT) lo2[a] = lofphi;
                    else {
                        acc = acc + (q.rhs[a] - lofphi) / 4.0;
                        accp = accp + c / 4.0;
                    }
                }
                if constexpr (ROUT) {
                    const int idx = cidx(v, i0, jr);
                    const double2 rt = *reinterpret_cast<const double2 *>(g.ortrue + idx);
                    const double r0 = -1.0 * lo2[0] + 1.0 * rt.x, r1 = -1.0 * lo2[1] + 1.0 * rt.y;
                    *reinterpret_cast<double2 *>(g.ores + idx) = make_double2(r0, r1);
                    if (g.olphi) *reinterpret_cast<double2 *>(g.olphi + idx) = make_double2(lo2[0], lo2[1]);
                    nmax = fmax(nmax, fmax(fabs(r0), fabs(r1)));
                } else if (jr & 1) {
                    const int ic = ((jr >> 1) + g.rgy) * g.rP + SUHMO_XOFF + (i0 >> 1);
                    g.rres[ic] = acc; g.rphi[ic] = accp;
                } else { racc = acc; raccp = accp; }
            }
        }
        // ---- 3. row r-2K has all 2K half-sweeps: stream it out (own pair, written by this thread)
        {
            const int jo = r - 2 * K - DL;
            if (own && jo >= jA && jo < jB) {
                const int so = ring(sr - 2 * K - DL);
                double2 o = make_double2(lds[so * LW + xl], lds[so * LW + xl + 1]);
                *reinterpret_cast<double2 *>(pout + cidx(v, i0, jo)) = o;
            }
        }
        // ---- 4. row r+1 enters the ring (its slot held row r-2K-2: no longer read), rotate
        sr = sr + 1 == R ? 0 : sr + 1;
        if (in_row) { lds[sr * LW + xl] = pnext.x; lds[sr * LW + xl + 1] = pnext.y; }
        if constexpr (WIDE && K >= 2) copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf5, cf4);
        if constexpr (YR) { ys5[0] = cf4.byN[0]; ys5[1] = cf4.byN[1]; }
        if constexpr (K >= 2) { copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf4, cf3); copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf3, cf2); }
        else if constexpr (RR) copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf3, cf2);
        copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf2, cf1);
        if constexpr (BCF) { CP2(cf1, cf0, B); bw1 = bw0; be1 = be0; }      // (its faces are formed in the next step, the rest is loaded then)
        else copy_coef<HAS_ALPHA, MASKED, ZBU, YR>(cf1, cf0);
    }
    if constexpr (ROUT) {
        if (g.onorm) {                         // (uniform) the chunk's max norm: a maximum, so the order of the lanes does not matter
            static_assert(!ROUT || NT == 64, "one wave per workgroup");
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nmax = fmax(nmax, __shfl_xor(nmax, o));
            if (t == 0) g.onorm[strip * g.nchunks + chunk] = nmax;
        }
    }
}

static bool fused_ok(const suhmo_level *L, const Depth &D, int K)
{
    const DV &v = D.v;
    if (v.nx % 2 || v.nx < 64 || v.ny < 4 * K + 4) return false;
    if (v.cfx[0] || v.cfx[1] || L->desc.nx_global > 0) return false;   // AMR patch: colour-pass kernel (stored coarse-fine ghosts)
    if ((v.ext[0] || v.ext[1]) && (v.gy < 2 * K || v.ny < 2 * K)) return false;   // halo rows must be real data
    if (v.per[1] && !(v.ext[0] || v.ext[1]) && v.ny < 4 * K) return false;
    return true;
}

// ---- the next launch of a level's relaxation, decided once (relax_step below); the launchers execute it, suhmo_gsrb_can_fuse_* ask it
enum { STEP_COLOUR = 0, STEP_TILE, STEP_STREAM };
enum { ABSORB_PROLONG = 1, ABSORB_RHS = 2, ABSORB_BCOEF = 4 };   // what waits for the depth's next launch: Depth::prolong_ / rhs_ / bcoef_pending
struct RelaxStep {
    int path;                    // STEP_COLOUR: one sweep as two colour passes; STEP_TILE: k_gsrb_tile; STEP_STREAM: k_gsrb_fused
    int done;                    // sweeps the launch does: 1, S x chunks, K
    int S, T, chunks;            // tile
    int K, NT;                   // streaming
    bool masked;                 // streaming: the ice mask is not known clean (or alpha != 0): the instantiation that reads it
    bool zbu;                    // streaming: the depth's bed elevation is known to be one value: the instantiation that takes it as a scalar
    bool yring;                  // streaming: the plain launch of those with one ring of y-faces (three waves per SIMD; not where y is periodic)
    // what the launch absorbs: it restricts; it leaves the residual of the final phi behind; it forms the FAS right-hand side; it forms depth
    // 0's faces; it adds the prolonged correction while loading
    bool rst, rout, frhs, bcf, prolong;
    int need, adv;               // rank strip: halo rows that must be current; halo rows the launch advances redundantly (current afterwards)
    bool shallow;                // colour passes because the halo is shallower than the tile launch needs
    int absorbs() const { return (prolong ? ABSORB_PROLONG : 0) | (frhs ? ABSORB_RHS : 0) | (bcf ? ABSORB_BCOEF : 0); }
    int RM() const { return rout ? 2 : rst ? 1 : 0; }
};

// the instantiations of k_gsrb_fused, by what they do.  wg_per_cu, slots: workgroups a CU / the chip holds at once, each instantiation's own
// answer of the occupancy query (asked at its first launch): the chunks of a launch are cut for the kernel that runs them
typedef void (*FusedFn)(DV, FP, const double *, double *, suhmo_phys_t, FusedGeom);
struct FusedKernel { int key; FusedFn fn; int slots, wg_per_cu; };
constexpr int fused_key(int K, bool alpha, int NT, int RM, bool frhs, bool masked, bool bcf, bool zbu = false, bool yring = false)
{
    return K | RM << 4 | alpha << 8 | frhs << 9 | masked << 10 | bcf << 11 | NT << 12 | zbu << 24 | yring << 25;       // (K, RM < 16; NT < 4096)
}
#define FK(K, A, NT, RM, F, M, B) {fused_key(K, A, NT, RM, F, M, B), k_gsrb_fused<K, A, NT, RM, F, M, B>, 0, 0}
// the launches of the clean-mask alpha = 0 cycle at K = 2, NT = 64 with the bed as a scalar (ZBU); YR: the plain one with one ring of y-faces
#define FK_ZBU(RM, F, B, YR) {fused_key(2, false, 64, RM, F, false, B, true, YR), k_gsrb_fused<2, false, 64, RM, F, false, B, true, YR>, 0, 0}
#define FK_PLAIN(K, NT, RM) FK(K, false, NT, RM, false, true, false), FK(K, false, NT, RM, false, false, false)
static FusedKernel fused_kernels[] = {
    FK_PLAIN(2, 64, 0), FK_PLAIN(2, 64, 1), FK_PLAIN(2, 64, 2), FK_PLAIN(1, 64, 0), FK_PLAIN(2, 256, 0), FK_PLAIN(1, 256, 0),
    FK(1, true, 64, 0, false, true, false), FK(2, true, 64, 0, false, true, false), FK(1, true, 256, 0, false, true, false), FK(2, true, 256, 0, false, true, false),
    FK(2, false, 64, 0, true, true, false), FK(2, false, 64, 0, true, false, false), FK(2, false, 64, 0, false, false, true),
    FK_ZBU(0, false, false, false), FK_ZBU(1, false, false, false), FK_ZBU(2, false, false, false), FK_ZBU(0, true, false, false), FK_ZBU(0, false, true, false),
    FK_ZBU(0, false, false, true),
};
#undef FK_ZBU
#undef FK_PLAIN
#undef FK
static FusedKernel *fused_kernel(int K, bool alpha, int NT, int RM, bool frhs, bool masked, bool bcf, bool zbu, bool yring = false)
{
    const int key = fused_key(K, alpha, NT, RM, frhs, masked, bcf, zbu, yring);
    for (FusedKernel &k : fused_kernels) if (k.key == key) return &k;
    return nullptr;
}
// the occupancy of an instantiation, asked once
static int fused_occupancy(FusedKernel *k, int NT)
{
    if (k->slots) return 0;
    int nb = 0, ncu = 0, dev = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k->fn, NT, 0));
    k->wg_per_cu = nb > 0 ? nb : 1;
    k->slots = k->wg_per_cu * (ncu > 0 ? ncu : 256);
    return 0;
}
// read-only options stream_wg_per_cu_<which> (suhmo_level.hip): workgroups per CU of the two-sweep one-wave launches of the clean-mask
// alpha = 0 cycle with the bed as a scalar -- plain, yring, rst, rout, frhs, bcf.  1: no such name
int suhmo_gsrb_stream_wg_per_cu(const char *which, long *value)
{
    static const struct { const char *name; int RM; bool frhs, bcf, yring; } tab[] = {
        {"plain", 0, false, false, false}, {"yring", 0, false, false, true}, {"rst", 1, false, false, false}, {"rout", 2, false, false, false},
        {"frhs", 0, true, false, false}, {"bcf", 0, false, true, false}};
    for (const auto &e : tab) {
        if (strcmp(which, e.name)) continue;
        FusedKernel *k = fused_kernel(2, false, 64, e.RM, e.frhs, false, e.bcf, true, e.yring);
        if (!k) { suhmo_set_error("internal: no streaming kernel '%s'", which); return -4; }
        int rc = fused_occupancy(k, 64); if (rc) return rc;
        *value = k->wg_per_cu;
        return 0;
    }
    return 1;
}

// part 0: the whole level.  Rank strips with the exchange in flight: part 1 = the chunks that read no halo row (returns 1 and
// launches nothing when the geometry has none), part 2 = the first and the last chunk, then the canvases trade places.
static int launch_fused(suhmo_level *L, int depth, const RelaxStep &s, hipStream_t st, int part = 0)
{
    const int K = s.K, NT = s.NT, RM = s.RM(), ext_rows = s.adv;
    const bool RST = RM == 1, RR = RM != 0, unmasked = !s.masked;
    Depth &D = L->d[depth];
    const DV &v = D.v;
    // the one check that relax_step handed over a launch that exists: alpha with no variant, the variants whole (no part) and one at a time
    FusedKernel *k = fused_kernel(K, v.alpha != 0.0, NT, RM, s.frhs, s.masked, s.bcf, s.zbu, s.yring);
    if (!k || (part && (s.frhs || s.bcf)) || (s.bcf && s.prolong)) { suhmo_set_error("internal: a streaming relaxation step without a kernel"); return -4; }
    if (!D.phi_alt) {
        HIPCHK(hipMalloc(&D.phi_alt, D.elems * sizeof(double)));
        HIPCHK(hipMemsetAsync(D.phi_alt, 0, D.elems * sizeof(double), st));
    }
    FusedGeom g;
    // (a launch that also forms depth 0's faces has the restricting launch's strips: two more halo columns per side)
    const int HX = 2 * K + ((RR || s.bcf) ? 2 : 0);
    const int EY = RR ? 1 : 0;
    const int maxW = 2 * NT - 2 * HX;
    g.nstrips = (v.nx + maxW - 1) / maxW;
    g.W = 2 * ((v.nx + 2 * g.nstrips - 1) / (2 * g.nstrips));
    g.nstrips = (v.nx + g.W - 1) / g.W;
    // rows per chunk: all tiles resident in ONE round (tiles <= workgroup slots of the chip;
    // a partial second round costs a full one), but never shorter than 16K rows so that the
    // 4K-row pipeline fill stays small; measured on MI355X: profiles/r01_b_hc_sweep.log
    {
        { int rc = fused_occupancy(k, NT); if (rc) return rc; }   // of the kernel that is launched: the plain one with one ring of y-faces holds 12 per CU, the others 8
        g.jbeg = v.ext[0] ? -ext_rows : 0;
        g.jend = v.ny + (v.ext[1] ? ext_rows : 0);
        const int nrows = g.jend - g.jbeg;
        // The launch with one ring of y-faces (12 workgroups per CU) is cut for 15/16 of its slots and may go down to 6K rows: a round filled
        // to the last slot is slower than one that leaves a few free, and its shorter chunks still pay (MI355X, us per launch, the parent's
        // launch 266.1 at 71 rows and 80.6 at 19, profiles/r27_yface_ring_hc_sweep.txt):
        //   4096^2, 35 strips: 47 rows (two rounds) 314.9, 48 (3010 of 3072 slots) 268.7, 49 247.1, 50 252.9, 51 251.7, 52 248.6, 55 254.2, 60 257.4, 71 258.4
        //   2048^2, 18 strips: 12 rows (two rounds) 94.0, 13 74.4, 15 78.5, 16 82.0, 19 82.9
        // 15/16 of 3072 slots: 50 rows and 13 rows.
        const int slots = s.yring ? k->slots - k->slots / 16 : k->slots, floorK = s.yring ? 6 : 8;
        int nch = slots / g.nstrips;
        if (nch < 1) nch = 1;
        g.Hc = (nrows + nch - 1) / nch;
        // (not shorter than 8K rows: the 4K-row pipeline fill.  The one-round height itself is the optimum where it is allowed: 2048^2,
        //  19 rows: 45.1 us per sweep, 24 rows 51.4, 32 rows -- two rounds, the old lower bound -- 60.3, profiles/r03_stream2048.txt)
        if (g.Hc < floorK * K) g.Hc = floorK * K;
        // cache-resident depths (about 1 M cells) are latency-bound: many short chunks beat few long ones
        // (profiles/r01_k_sweep_small_hc.log: 1024^2, K = 2: 22.3 us per sweep at 6 rows vs 28.1 for the colour passes)
        if ((long)v.nx * v.ny < 2000000L) g.Hc = 6;
        if (L->fused_hc > 0) g.Hc = L->fused_hc;          // explicit: no lower clamp (tools/sweep_small_hc.sh)
        if (RST) g.Hc += g.Hc & 1;                        // a coarse cell's two fine rows stay in one chunk
        if (g.Hc > nrows) g.Hc = nrows;
        g.nchunks = (nrows + g.Hc - 1) / g.Hc;
    }
    g.nchl = g.nchunks; g.chunk0 = 0; g.chunk1 = g.nchunks; g.edges = 0;
    if (part) {
        // inner chunks [c0, c1): their rows and the 2K (+1) rows either side that they read are the strip's own (a side that is a
        // physical boundary has no halo rows to wait for)
        int c0 = 0, c1 = g.nchunks;
        if (v.ext[0]) while (c0 < g.nchunks && g.jbeg + c0 * g.Hc - 2 * K - EY < 0) c0++;
        if (v.ext[1]) while (c1 > c0 && std::min(g.jbeg + c1 * g.Hc, g.jend) - 1 + 2 * K + EY > v.ny - 1) c1--;
        const bool ok = c1 > c0 && c1 - c0 < g.nchunks;
        if (!ok) { if (part == 1) return 1; }
        else if (part == 1) { g.chunk0 = c0; g.chunk1 = c1; g.nchl = c1 - c0; }
        else { g.edges = 1; g.chunk0 = c0; g.chunk1 = c1; g.nchl = g.nchunks - (c1 - c0); }
    }
    g.ntiles = g.nstrips * g.nchl;
    bool selfper = v.per[1] && !(v.ext[0] || v.ext[1]);
    g.wrap_y = selfper;
    g.ylo = v.ext[0] ? g.jbeg - 2 * K - EY : (selfper ? -2 * K - EY : 0);
    g.yhi = v.ext[1] ? g.jend - 1 + 2 * K + EY : (selfper ? v.ny - 1 + 2 * K + EY : v.ny - 1);
    const double *pin = D.fp.f[SUHMO_F_PHI];
    g.pc = g.pco = nullptr; g.Pc = g.gyc = 0;
    if (s.prolong) {
        Depth &C = L->d[depth + 1];
        g.pc = C.fp.f[SUHMO_F_PHI]; g.pco = C.fp.f[SUHMO_F_PHIOLD]; g.Pc = C.v.P; g.gyc = C.v.gy;
        if (part != 1) D.prolong_pending = 0;
    }
    g.negflag = nullptr; g.mask_epoch = 0;
    // (the report is about depth 0's mask and, on a rank strip, the stored halo rows of every depth; the coarse masks are averages of
    //  depth 0's, MGnewOp: none of them is negative either -- as long as nobody has written one since, coarse_mask_ok)
    if (!unmasked && L->skip_mask && L->maskflag_epoch && L->maskflag_epoch == L->mask_epoch && (depth == 0 || L->coarse_mask_ok)
        && (L->desc.nx_global == 0)) {
        g.negflag = suhmo_mask_report_word(L); g.mask_epoch = L->mask_epoch;
    }
    g.rres = g.rphi = nullptr; g.rP = g.rgy = 0;
    if (RST) {
        Depth &C = L->d[depth + 1];
        g.rres = C.fp.f[SUHMO_F_RES]; g.rphi = C.fp.f[SUHMO_F_PHI]; g.rP = C.v.P; g.rgy = C.v.gy;
        C.phi_fresh = 0;
    }
    g.zb_uniform = s.zbu ? D.zb_value : 0.0;
    g.fres = nullptr; g.frhs = g.flphi = g.fphiold = nullptr;
    g.ortrue = nullptr; g.ores = g.olphi = nullptr; g.onorm = nullptr;
    if (RM == 2) {
        g.ortrue = L->resout_rhs ? L->resout_rhs : D.fp.f[SUHMO_F_RHS];
        g.ores = D.fp.f[SUHMO_F_RES];
        if (L->resout_req & 2) { g.olphi = suhmo_field(L, depth, SUHMO_F_LPHI); if (!g.olphi) return -2; }
        if ((L->resout_req & 4) && (size_t)g.nstrips * g.nchunks + 4 < L->scratch_elems) { g.onorm = L->scratch + 2; L->resout_np = g.nstrips * g.nchunks; }
        else L->resout_np = 0;
    }
    if (s.frhs) {
        g.fres = D.fp.f[SUHMO_F_RES]; g.frhs = D.fp.f[SUHMO_F_RHS]; g.flphi = suhmo_field(L, depth, SUHMO_F_LPHI); g.fphiold = suhmo_field(L, depth, SUHMO_F_PHIOLD);
        if (!g.flphi || !g.fphiold) return -2;
        D.rhs_pending = 0; L->frhs_stream++;
    }
    if (s.bcf) { D.bcoef_pending = 0; L->bcoef_in_relax_count++; suhmo_faces_made(L); L->bcoef_unmasked++; }   // (it is the cycle's unmasked UpdateOperator too)
    hipLaunchKernelGGL(k->fn, dim3(g.ntiles), dim3(NT), 0, st, v, D.fp, pin, D.phi_alt, L->ph, g);
    if (unmasked) L->relax_unmasked++;
    if (s.zbu) L->relax_zb_uniform[depth]++;
    if (s.yring) L->relax_yring[depth]++;
    if (part != 1) { std::swap(D.fp.f[SUHMO_F_PHI], D.phi_alt); suhmo_fp_changed(); }
    return 0;
}

// ---- variant 3: S sweeps of a T x T tile in LDS (cache-resident depths) ----
// Depths of up to about a million cells are latency-bound: a colour pass is one launch of ~5 us whatever its size (the
// dependent launch, the first touch of data the previous kernel wrote on another XCD), so a smoothing of 4 sweeps costs 8 of
// them.  Here a workgroup loads its tile plus a halo of 2S cells into LDS, keeps the coefficients of its cells in registers
// and runs all 2S colour passes between barriers; pass p is valid one cell further in from the halo's edge than pass p-1
// (sides that are physical boundaries do not shrink: the boundary condition is evaluated on the fly there), so after 2S
// passes exactly the tile is current.  Every update is the expression of k_gsrb_pass_simple on the same operands: the result
// is bitwise the same, the halo work is redundant.  Output goes to the second phi canvas (neighbour tiles read the old one).
struct TileGeom {
    int ntx, nty;
    const double *pc, *pco; int Pc, gyc;     // prolongIncrement fused into the load (as in FusedGeom)
    double *rres, *rphi; int rP, rgy;        // RST: coarse RES / PHI canvases
    int frhs;                                // first relaxation of a coarse FAS depth: rhs = res + L(phi) is formed here
    int jbeg, jend;                          // rows written: the level's, plus on a rank strip the halo rows that stay current for the next launch
    int chunks;                              // level = one tile: this many times S sweeps in the launch (halo images refreshed in LDS)
    int order;                               // workgroup -> tile: 0 as launched, 1 / 2 XCD-aware (see k_gsrb_tile)
};
// (the timing probes that switch parts of the tile kernel off -- wrong results on purpose -- live in a copy of this file:
//  tools/probes/suhmo_gsrb_tile_probe.hip, built by tools/probes/tile_probe.sh; nothing of them is in the product kernel)
// (of the ice mask COMPUTENONLINEARTERMS uses the sign only: mneg bit 0 / 1 = the first / second cell of the pair is without ice)
struct PairCoef { double rhs0, rhs1, B0, B1, Pi0, Pi1, zb0, zb1, a0, a1, byS0, byS1, byN0, byN1, bx0, bx1, bx2; int mneg; };

// RST = true: the launch also restricts (as k_gsrb_fused<.., RST>): one more ring of final values around the tile (two columns,
// pairs stay aligned), the residual quarters of the tile's cells go through LDS and one thread per coarse cell adds the four in
// the reference's visiting order (RESTRICTRESVCNL2D + RESTRICTVCNL).  The 32-wide tile is 28 rows high then: the same number
// of column pairs per thread, hence the same registers, as without the restriction.
template <int T, bool RST> struct TileShape { static constexpr int TX = T, TY = (RST && T == 32) ? 28 : T; };
// Threads per workgroup: 256 (5 column pairs per thread at T = 32, S = 4: 2 waves per SIMD).  Measured and dropped (profiles/r03_tile_*):
// 384 threads (3 pairs per thread, 161-168 VGPRs, 3 waves per SIMD on paper) -- the six waves of a workgroup land 2 + 2 + 1 + 1 on the
// four SIMDs, a second workgroup no longer fits beside the first, and the 2048^2 launch takes 266 us instead of 203.
template <int S, int T, bool RST> struct TileThreads { static constexpr int NT = 256; };
// (the body, shared by the solo kernel and the batched one below: blockIdx.x = tile)
// (no MASKED parameter here, unlike k_gsrb_fused: tried on the plain alpha = 0 launches -- the mask is one load per pair kept as two sign
// bits, the registers stay at the cap and the launches take what they took)
template <int S, int T, bool HAS_ALPHA, bool RST = false, bool CHUNKED = false>
__device__ __forceinline__ void d_gsrb_tile(const DV &v, const FP &fp, const double *__restrict__ pin, double *__restrict__ pout,
                                            const suhmo_phys_t &ph, const TileGeom &g)
{
    constexpr int TX = TileShape<T, RST>::TX, TY = TileShape<T, RST>::TY;
    constexpr int HX = 2 * S + (RST ? 2 : 0), HY = 2 * S + (RST ? 1 : 0);
    constexpr int LX = TX + 2 * HX, LY = TY + 2 * HY, NP = LX / 2, NPAIR = NP * LY;
    constexpr int NT = TileThreads<S, T, RST>::NT, NK = (NPAIR + NT - 1) / NT;
    // (a margin of one row + two cells either side: the straight-line pass below also evaluates the cells on the region's edge, whose
    // results are dropped, and reads one cell beyond them)
    constexpr int PAD = LX + 2;
    __shared__ double lds_raw[LY * LX + 2 * PAD];
    double *const lds = lds_raw + PAD;
    __shared__ double lq[RST ? TY * TX : 1];                  // RST: (rhs - L(phi)) / 4 of the tile's cells
    // Workgroups are dealt round-robin over the 8 XCDs, each with its own L2: every XCD takes a contiguous run of the tile list, so
    // that the tiles in flight on it are neighbours and the halo cells they share (2.25 x the tile's own at S = 4) are read from HBM
    // once.  order 2 lists the tiles in panels of 8 tile rows, column by column: the 64 tiles an XCD holds at a time form a square.
    int tl = blockIdx.x;
    if (g.order) {
        const int nt = g.ntx * g.nty, q8 = nt / 8, rem = nt % 8, xcd = tl % 8;
        tl = xcd * q8 + (xcd < rem ? xcd : rem) + tl / 8;
    }
    int tx = tl % g.ntx, ty = tl / g.ntx;
    if (g.order == 2) {
        const int pan = tl / (8 * g.ntx), r = tl - pan * 8 * g.ntx, hp = (g.nty - 8 * pan < 8) ? g.nty - 8 * pan : 8;
        tx = r / hp; ty = 8 * pan + r % hp;
    }
    const int tj0 = g.jbeg + ty * TY;                         // first row the tile writes
    const int gx0 = tx * TX - HX, gy0 = tj0 - HY;             // domain cell of LDS cell (0, 0)
    const int t = threadIdx.x;
    // thread -> column pairs: the pairs of a WAVE lie in rows of one parity (waves 0, 2: even rows of the region; 1, 3: odd rows), so
    // which cell of its pairs a colour pass advances is the same for the whole wave: a scalar branch picks one of two straight-line
    // bodies with the pair's coefficients addressed statically, instead of per-lane selects
    const int par = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 1;
    const int u0 = ((t >> 7) << 6) | (t & 63);                 // this thread among the NT / 2 of its parity
    auto pair_pos = [&](const int k, int &ly, int &lx) -> bool {
        const int u = u0 + (NT / 2) * k, r = u / NP;
        ly = 2 * r + par; lx = 2 * (u - r * NP);
        return ly < LY;
    };
    // (measured and dropped, profiles/r03_tile_probe.txt: the rows of a parity taken tile rows first, then the halo rows from the tile
    //  outwards, so that the later slots of a thread hold halo rows only and the straight-line passes skip a slot as a whole once none of
    //  its rows is advanced any more -- 34 slot-passes instead of 40, bitwise, and the launch takes the same 203 us)
    static_assert(LY % 2 == 0, "rows of the region come in pairs of parities");
    // a coarse-fine side takes precedence over the domain's periodicity (the patch does not wrap onto itself)
    const bool perx = v.per[0] && !v.cfx[0] && !v.cfx[1], pery = v.per[1] && !v.ext[0] && !v.ext[1];
    // sides of the LDS region that reach a physical boundary: nothing beyond them feeds the tile
    // (a coarse-fine side of an AMR patch: once the stored ghost column / row is in the region)
    const bool openW = !perx && gx0 <= (v.cfx[0] ? -1 : 0), openE = !perx && gx0 + LX - 1 >= v.nx - 1 + (v.cfx[1] ? 1 : 0);
    const bool openS = !pery && !v.rk[0] && gy0 <= (v.ext[0] ? -1 : 0), openN = !pery && !v.rk[1] && gy0 + LY - 1 >= v.ny - 1 + (v.ext[1] ? 1 : 0);
    auto wrap = [](int i, int n) { i %= n; return i < 0 ? i + n : i; };
    auto ld2 = [&](const double *__restrict__ p, int idx) { return *reinterpret_cast<const double2 *>(p + idx); };

    // coefficients of the thread's pairs as NAMED variables (an array ends up in scratch memory)
    PairCoef cf0, cf1, cf2, cf3, cf4;
    bool lv0, lv1, lv2, lv3, lv4;                             // the pair lies in the domain (or is a periodic image of one that does)
    static_assert(NK <= 5 && TX * TY / 4 <= NT, "tile too large for the workgroup");
#define TILE_EACH(F) { F(0, cf0, lv0); if constexpr (NK > 1) F(1, cf1, lv1); if constexpr (NK > 2) F(2, cf2, lv2); \
                       if constexpr (NK > 3) F(3, cf3, lv3); if constexpr (NK > 4) F(4, cf4, lv4); }
    bool special = false;                                     // a pair of this thread has a cell without ice or in a cut-off range of the gap height
    // most tiles of a large level: the whole region lies in the level's own cells (uniform) -- the index logic of the general case
    // (validity of every pair, periodic images, stored ghosts, halo rows) is 250 instructions per pair, 19 % of the launch at 2048^2
    const bool inner = gx0 >= 0 && gx0 + LX <= v.nx && gy0 >= 0 && gy0 + LY <= v.ny;
    // the coefficients of a pair in the domain (and the FAS correction added to its phi, PROLONGNL)
    auto ldcoef = [&](PairCoef &c, double2 &p2, const int idx, const int i, const int j) {
        if (g.pc) {
            const int ic = ((j >> 1) + g.gyc) * g.Pc + SUHMO_XOFF + (i >> 1);
            const double corr = 1.0 * g.pc[ic] + (-1.0) * g.pco[ic];      // axby(1, -1), then PROLONGNL
            p2.x = p2.x + corr; p2.y = p2.y + corr;
        }
        double2 d;
        d = ld2(g.frhs ? fp.f[SUHMO_F_RES] : fp.f[SUHMO_F_RHS], idx); c.rhs0 = d.x; c.rhs1 = d.y;
        d = ld2(fp.f[SUHMO_F_B], idx); c.B0 = d.x; c.B1 = d.y;
        d = ld2(fp.f[SUHMO_F_PI], idx); c.Pi0 = d.x; c.Pi1 = d.y;
        d = ld2(fp.f[SUHMO_F_ZB], idx); c.zb0 = d.x; c.zb1 = d.y;
        d = ld2(fp.f[SUHMO_F_MASK], idx); c.mneg = (d.x < 0.0 ? 1 : 0) | (d.y < 0.0 ? 2 : 0);
        if (HAS_ALPHA) { d = ld2(fp.f[SUHMO_F_ACOEF], idx); c.a0 = d.x; c.a1 = d.y; }
        d = ld2(fp.f[SUHMO_F_BY], idx); c.byS0 = d.x; c.byS1 = d.y;
        d = ld2(fp.f[SUHMO_F_BY], idx + v.P); c.byN0 = d.x; c.byN1 = d.y;
        d = ld2(fp.f[SUHMO_F_BX], idx); c.bx0 = d.x; c.bx1 = d.y; c.bx2 = fp.f[SUHMO_F_BX][idx + 2];
        special = special || c.mneg != 0 || ph.cutOffbr > c.B0 || ph.cutOffbr > c.B1 || ph.maxOffbr < c.B0 || ph.maxOffbr < c.B1;
    };
    auto load = [&](const int k, PairCoef &c, bool &live) {
        live = false;
        int ly, lx;
        if (pair_pos(k, ly, lx)) {
            int i = gx0 + lx, j = gy0 + ly;
            if (inner) {                                      // the region lies in the level's own cells: no test, no wrap, no ghost
                live = true;
                const int idx = cidx(v, i, j);
                double2 p2 = ld2(pin, idx);
                ldcoef(c, p2, idx, i, j);
                lds[ly * LX + lx] = p2.x; lds[ly * LX + lx + 1] = p2.y;
                return;
            }
            // (rank boundary of a strip: the rows beyond are the neighbour's cells, held in the canvas' halo rows with their
            //  coefficients; they are advanced redundantly like periodic images, without the wrap)
            // (only the halo rows the written rows depend on: the canvas ends at gy)
            const bool inx = perx || (i >= 0 && i < v.nx), iny = pery || (j >= 0 && j < v.ny) || (j < 0 && v.rk[0] && j >= g.jbeg - HY) || (j >= v.ny && v.rk[1]
                && j < g.jend + HY);
            // AMR patch: the ghost column / row beyond a coarse-fine side holds interpolated data: loaded, never advanced
            const bool exi = inx || (i == -2 && v.cfx[0]) || (i == v.nx && v.cfx[1]);
            const bool exj = iny || (j == -1 && v.ext[0] && !v.rk[0]) || (j == v.ny && v.ext[1] && !v.rk[1]);
            double2 p2 = make_double2(0.0, 0.0);
            if (exi && exj) {
                live = inx && iny;
                if (perx) i = wrap(i, v.nx);
                if (pery) j = wrap(j, v.ny);
                const int idx = cidx(v, i, j);
                p2 = ld2(pin, idx);
            }
            if (live) ldcoef(c, p2, cidx(v, i, j), i, j);
            lds[ly * LX + lx] = p2.x; lds[ly * LX + lx + 1] = p2.y;
        }
    };
    TILE_EACH(load);
    // Straight-line passes (below) when nothing in the region needs a case distinction: no physical-boundary, coarse-fine or
    // stored-ghost side in reach, every cell under ice and outside the cut-off ranges of COMPUTENONLINEARTERMS (workgroup-uniform)
    // (only in the instantiation that relaxes the large depths: with aCoef, the restriction or the chunk loop on top the second loop
    //  body costs the kernel its second wave per SIMD)
    constexpr bool PLAIN_OK = !HAS_ALPHA && !RST && !CHUNKED;
    const bool plain = PLAIN_OK && !__syncthreads_or(special ? 1 : 0) && ph.use_NL && !openW && !openE && !openS && !openN
                       && !v.cfx[0] && !v.cfx[1] && !(v.ext[0] && !v.rk[0]) && !(v.ext[1] && !v.rk[1]);
    if constexpr (!PLAIN_OK) __syncthreads();

    // The FAS right-hand side of a coarse depth, rhs = res + L(R phi) (applyOpMg + axby of the cycle, k_apply<., 2>), formed
    // from the restricted phi just loaded, for every cell the passes will advance; the tile's own cells also store it, L(phi)
    // and the copy of R phi the prolongation subtracts later.
    if (g.frhs) {
        const int ylo = openS ? 0 : 1, yhi = openN ? LY - 1 : LY - 2;
        auto mkrhs = [&](const int k, PairCoef &q_, const bool live) {
            int ly, lx;
            if (pair_pos(k, ly, lx) && live) {
                const int i = gx0 + lx, j = gy0 + ly;
                if (ly >= ylo && ly <= yhi) {
                    const double *row = lds + ly * LX;
                    double lo[2], cc[2];
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        const int x = lx + a, ii = i + a;
                        double c = row[x];
                        double w = row[x > 0 ? x - 1 : 0], e = row[x < LX - 1 ? x + 1 : LX - 1];
                        double s_ = lds[(ly > 0 ? ly - 1 : 0) * LX + x], n = lds[(ly < LY - 1 ? ly + 1 : LY - 1) * LX + x];
                        if (!perx) {
                            if (ii == 0 && !v.cfx[0]) w = (v.bct[0][0] == 0) ? v.two_v[0][0] - c : c + v.neu[0][0];
                            if (ii == v.nx - 1 && !v.cfx[1]) e = (v.bct[0][1] == 0) ? v.two_v[0][1] - c : c + v.neu[0][1];
                        }
                        if (!pery) {
                            if (j == 0 && !v.ext[0]) s_ = (v.bct[1][0] == 0) ? v.two_v[1][0] - c : c + v.neu[1][0];
                            if (j == v.ny - 1 && !v.ext[1]) n = (v.bct[1][1] == 0) ? v.two_v[1][1] - c : c + v.neu[1][1];
                        }
                        double nl, dnl;
                        nl_terms(ph, c, a ? q_.B1 : q_.B0, a ? q_.Pi1 : q_.Pi0, a ? q_.zb1 : q_.zb0, (q_.mneg >> a) & 1 ? -1.0 : 1.0, nl, dnl);
                        const double bxW = a ? q_.bx1 : q_.bx0, bxE = a ? q_.bx2 : q_.bx1;
                        double aterm = HAS_ALPHA ? v.alpha * (a ? q_.a1 : q_.a0) : v.alpha;
                        lo[a] = lofphi_cell(v, aterm, c, e, w, n, s_, bxE, bxW, a ? q_.byN1 : q_.byN0, a ? q_.byS1 : q_.byS0, nl);
                        cc[a] = c;
                    }
                    // (a cell on the region's edge, which no pass advances, gets a value nobody reads)
                    q_.rhs0 = 1.0 * q_.rhs0 + 1.0 * lo[0]; q_.rhs1 = 1.0 * q_.rhs1 + 1.0 * lo[1];
                    if (lx >= HX && lx < HX + TX && ly >= HY && ly < HY + TY && i < v.nx && j < g.jend) {
                        const int idx = cidx(v, i, j);
                        *reinterpret_cast<double2 *>(fp.f[SUHMO_F_LPHI] + idx) = make_double2(lo[0], lo[1]);
                        *reinterpret_cast<double2 *>(fp.f[SUHMO_F_RHS] + idx) = make_double2(q_.rhs0, q_.rhs1);
                        *reinterpret_cast<double2 *>(fp.f[SUHMO_F_PHIOLD] + idx) = make_double2(cc[0], cc[1]);
                    }
                }
            }
        };
        TILE_EACH(mkrhs);
        // (the passes below only write phi in LDS, which mkrhs only read: but a pass may overwrite a cell a slower wave still has
        // to read for its L(phi))
        __syncthreads();
    }

    // CHUNKED (its own instantiation: the outer loop costs the large tiles their second workgroup per CU): a level that is one
    // tile can go on after 2S passes, what the halo lacks then are only the periodic images of its own cells
#pragma unroll 1
    for (int chunk = 0; chunk < (CHUNKED ? g.chunks : 1); chunk++) {
    if (CHUNKED && chunk > 0 && (perx || pery)) {
        auto refresh = [&](const int k, const PairCoef &, const bool live) {
            int ly, lx;
            if (pair_pos(k, ly, lx) && live) {
                const int i = gx0 + lx, j = gy0 + ly;
                if (i < 0 || i >= v.nx || j < 0 || j >= v.ny) {
                    const int src = ((pery ? wrap(j, v.ny) : j) - gy0) * LX + ((perx ? wrap(i, v.nx) : i) - gx0);
                    const double a0 = lds[src], a1 = lds[src + 1];      // cells of the domain: nobody writes them here
                    lds[ly * LX + lx] = a0; lds[ly * LX + lx + 1] = a1;
                }
            }
        };
        TILE_EACH(refresh);
        __syncthreads();
    }
    if constexpr (PLAIN_OK) { if (plain) {
        // ---- the passes as straight-line code: every pair of the thread is evaluated (edge cells and idle slots too: their results
        // land in the margin), all LDS reads of a pass come before its writes (a pass reads the other colour and its own
        // centres only), nothing branches per lane: five independent updates the scheduler can interleave.  The expressions are
        // those of the general pass with the case distinctions that cannot occur here taken out: the same bits.
#pragma unroll 1
        for (int p = 0; p < 2 * S; p++) {
            const int lo = p + 1, xhi = LX - 2 - p, yhi = LY - 2 - p;
            const int a_pass = (gy0 + par + v.j0 + p) & 1;    // scalar: the pairs of this wave share their rows' parity
            // (the coefficients are loop-invariant: keep the compiler from hoisting products of them out of the pass loop into
            //  registers that do not exist)
#define TOUCH(c) asm volatile("" : "+v"(c.rhs0), "+v"(c.rhs1), "+v"(c.B0), "+v"(c.B1), "+v"(c.Pi0), "+v"(c.Pi1), "+v"(c.zb0), "+v"(c.zb1), \
                              "+v"(c.byS0), "+v"(c.byS1), "+v"(c.byN0), "+v"(c.byN1), "+v"(c.bx0), "+v"(c.bx1), "+v"(c.bx2))
            TOUCH(cf0); if constexpr (NK > 1) TOUCH(cf1); if constexpr (NK > 2) TOUCH(cf2); if constexpr (NK > 3) TOUCH(cf3); if constexpr (NK > 4) TOUCH(cf4);
#undef TOUCH
            double nv0 = 0.0, nv1 = 0.0, nv2 = 0.0, nv3 = 0.0, nv4 = 0.0;
            int ad0 = -1, ad1 = -1, ad2 = -1, ad3 = -1, ad4 = -1;
            auto upd = [&](const int k, const PairCoef &q_, auto a_tag, double &nv, int &ad) {
                constexpr int A = decltype(a_tag)::value;
                int ly, lx;
                const bool ok = pair_pos(k, ly, lx);
                if (!ok) { ly = par; lx = 0; }                // idle slot: any valid pair for the reads, a cell of the margin for the write
                const int x = lx + A;
                const double *row = lds + ly * LX;
                double2 pr; double wl, er, s, n;
                pr = *reinterpret_cast<const double2 *>(row + lx); wl = row[lx - 1]; er = row[lx + 2]; s = row[x - LX]; n = row[x + LX];
                const double c = A ? pr.y : pr.x;
                const double w = A ? pr.x : wl, e = A ? er : pr.y;
                const double B = A ? q_.B1 : q_.B0;
                const double N = (A ? q_.Pi1 : q_.Pi0) - ph.rho_w_g * (c - (A ? q_.zb1 : q_.zb0));      // nl_terms, no case applies
                const double nl = -ph.A * B * N * N * N;
                const double dnl = 3.0 * ph.A * B * 1000.0 * ph.grav * N * N;
                const double bxW = A ? q_.bx1 : q_.bx0, bxE = A ? q_.bx2 : q_.bx1;
                const double byN = A ? q_.byN1 : q_.byN0, byS = A ? q_.byS1 : q_.byS0;
                const double aterm = HAS_ALPHA ? v.alpha * (A ? q_.a1 : q_.a0) : v.alpha;
                const double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, byN, byS, nl);
                const double lam = lambda_cell(v, aterm, bxE, bxW, byN, byS);
                const double denom = 1.0e-16 + lam + dnl;
                const double cnew = c + ((A ? q_.rhs1 : q_.rhs0) - lofphi) / denom;
                // (the result of a cell outside this pass's region goes to a cell of the margin: an unconditional store, so that the
                //  compiler cannot sink the evaluation into a branch per pair, which would serialise the five updates again)
                const bool in = ok && x >= lo && x <= xhi && ly >= lo && ly <= yhi;
                nv = cnew;
                ad = in ? ly * LX + x : -1;
            };
            if (a_pass) {
                using A1 = std::integral_constant<int, 1>;
                upd(0, cf0, A1(), nv0, ad0); if constexpr (NK > 1) upd(1, cf1, A1(), nv1, ad1); if constexpr (NK > 2) upd(2, cf2, A1(), nv2, ad2);
                if constexpr (NK > 3) upd(3, cf3, A1(), nv3, ad3); if constexpr (NK > 4) upd(4, cf4, A1(), nv4, ad4);
            } else {
                using A0 = std::integral_constant<int, 0>;
                upd(0, cf0, A0(), nv0, ad0); if constexpr (NK > 1) upd(1, cf1, A0(), nv1, ad1); if constexpr (NK > 2) upd(2, cf2, A0(), nv2, ad2);
                if constexpr (NK > 3) upd(3, cf3, A0(), nv3, ad3); if constexpr (NK > 4) upd(4, cf4, A0(), nv4, ad4);
            }
            lds[ad0] = nv0; if constexpr (NK > 1) lds[ad1] = nv1; if constexpr (NK > 2) lds[ad2] = nv2;
            if constexpr (NK > 3) lds[ad3] = nv3; if constexpr (NK > 4) lds[ad4] = nv4;
            __syncthreads();
        }
    } }
    if (!(PLAIN_OK && plain))
#pragma unroll 1
    for (int p = 0; p < 2 * S; p++) {
        const int xlo = openW ? 0 : p + 1, xhi = openE ? LX - 1 : LX - 2 - p;
        const int ylo = openS ? 0 : p + 1, yhi = openN ? LY - 1 : LY - 2 - p;
        auto relax = [&](const int k, const PairCoef &q_, const bool live) {
            int ly, lx;
            if (pair_pos(k, ly, lx) && live) {
                const int j = gy0 + ly;
                const int a = (j + v.j0 + p) & 1;             // which cell of the pair has this pass's colour
                const int x = lx + a, i = gx0 + x;
                if (x >= xlo && x <= xhi && ly >= ylo && ly <= yhi) {
                    const double *row = lds + ly * LX;
                    double c = row[x];
                    double w = row[x > 0 ? x - 1 : 0], e = row[x < LX - 1 ? x + 1 : LX - 1];
                    double s = lds[(ly > 0 ? ly - 1 : 0) * LX + x], n = lds[(ly < LY - 1 ? ly + 1 : LY - 1) * LX + x];
                    if (!perx) {                          // mixBCValues on the fly
                        if (i == 0 && !v.cfx[0]) w = (v.bct[0][0] == 0) ? v.two_v[0][0] - c : c + v.neu[0][0];
                        if (i == v.nx - 1 && !v.cfx[1]) e = (v.bct[0][1] == 0) ? v.two_v[0][1] - c : c + v.neu[0][1];
                    }
                    if (!pery) {
                        if (j == 0 && !v.ext[0]) s = (v.bct[1][0] == 0) ? v.two_v[1][0] - c : c + v.neu[1][0];
                        if (j == v.ny - 1 && !v.ext[1]) n = (v.bct[1][1] == 0) ? v.two_v[1][1] - c : c + v.neu[1][1];
                    }
                    double nl, dnl;
                    nl_terms(ph, c, a ? q_.B1 : q_.B0, a ? q_.Pi1 : q_.Pi0, a ? q_.zb1 : q_.zb0, (q_.mneg >> a) & 1 ? -1.0 : 1.0, nl, dnl);
                    const double bxW = a ? q_.bx1 : q_.bx0, bxE = a ? q_.bx2 : q_.bx1;
                    const double byN = a ? q_.byN1 : q_.byN0, byS = a ? q_.byS1 : q_.byS0;
                    double aterm = HAS_ALPHA ? v.alpha * (a ? q_.a1 : q_.a0) : v.alpha;
                    double lofphi = lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, byN, byS, nl);
                    double lam = lambda_cell(v, aterm, bxE, bxW, byN, byS);
                    double denom = 1.0e-16 + lam + dnl;
                    lds[ly * LX + x] = c + ((a ? q_.rhs1 : q_.rhs0) - lofphi) / denom;
                }
            }
        };
        TILE_EACH(relax);
        __syncthreads();
    }
    }

    const int oi1 = (tx * TX + TX < v.nx) ? tx * TX + TX : v.nx, oj1 = (tj0 + TY < g.jend) ? tj0 + TY : g.jend;
    const int wi0 = tx * TX - ((tx == 0 && v.cfx[0]) ? 1 : 0), wi1 = oi1 + ((oi1 == v.nx && v.cfx[1]) ? 1 : 0);
    const int wj0 = tj0 - ((ty == 0 && v.ext[0] && !v.rk[0]) ? 1 : 0), wj1 = oj1 + ((oj1 == v.ny && v.ext[1] && !v.rk[1]) ? 1 : 0);
    auto store = [&](const int k, const PairCoef &q_, const bool) {
        int ly, lx;
        if (pair_pos(k, ly, lx)) {
            const int i = gx0 + lx, j = gy0 + ly;
            if (inner && !RST) {                              // (the tile itself lies in the level too)
                if (lx >= HX && lx < HX + TX && ly >= HY && ly < HY + TY)
                    *reinterpret_cast<double2 *>(pout + cidx(v, i, j)) = make_double2(lds[ly * LX + lx], lds[ly * LX + lx + 1]);
                return;
            }
            // cells this tile writes: its own and, next to a coarse-fine side, the stored ghosts (the other canvas has to
            // carry them too)
            if (j >= wj0 && j < wj1) {
                const bool m0 = i >= wi0 && i < wi1, m1 = i + 1 >= wi0 && i + 1 < wi1;
                if (m0 && m1) *reinterpret_cast<double2 *>(pout + cidx(v, i, j)) = make_double2(lds[ly * LX + lx], lds[ly * LX + lx + 1]);
                else if (m0) pout[cidx(v, i, j)] = lds[ly * LX + lx];
                else if (m1) pout[cidx(v, i + 1, j)] = lds[ly * LX + lx + 1];
            }
            if (lx >= HX && lx < HX + TX && ly >= HY && ly < HY + TY && i < v.nx && j >= 0 && j < v.ny) {   // (halo rows: advanced, not restricted)
                if constexpr (RST) {
                    const double *row = lds + ly * LX;
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        const int x = lx + a, ii = i + a;
                        double c = row[x], w = row[x - 1], e = row[x + 1];          // the tile never touches the edge of the LDS region
                        double s_ = lds[(ly - 1) * LX + x], n = lds[(ly + 1) * LX + x];
                        if (!perx) {
                            if (ii == 0 && !v.cfx[0]) w = (v.bct[0][0] == 0) ? v.two_v[0][0] - c : c + v.neu[0][0];
                            if (ii == v.nx - 1 && !v.cfx[1]) e = (v.bct[0][1] == 0) ? v.two_v[0][1] - c : c + v.neu[0][1];
                        }
                        if (!pery) {
                            if (j == 0 && !v.ext[0]) s_ = (v.bct[1][0] == 0) ? v.two_v[1][0] - c : c + v.neu[1][0];
                            if (j == v.ny - 1 && !v.ext[1]) n = (v.bct[1][1] == 0) ? v.two_v[1][1] - c : c + v.neu[1][1];
                        }
                        double nl, dnl;
                        nl_terms(ph, c, a ? q_.B1 : q_.B0, a ? q_.Pi1 : q_.Pi0, a ? q_.zb1 : q_.zb0, (q_.mneg >> a) & 1 ? -1.0 : 1.0, nl, dnl);
                        const double bxW = a ? q_.bx1 : q_.bx0, bxE = a ? q_.bx2 : q_.bx1;
                        double aterm = HAS_ALPHA ? v.alpha * (a ? q_.a1 : q_.a0) : v.alpha;
                        double lofphi = lofphi_cell(v, aterm, c, e, w, n, s_, bxE, bxW, a ? q_.byN1 : q_.byN0, a ? q_.byS1 : q_.byS0, nl);
                        lq[(ly - HY) * TX + (lx - HX) + a] = ((a ? q_.rhs1 : q_.rhs0) - lofphi) / 4.0;
                    }
                }
            }
        }
    };
    TILE_EACH(store);
#undef TILE_EACH
    if constexpr (RST) {
        __syncthreads();
        if (t < TX * TY / 4) {
            const int cx = t % (TX / 2), cy = t / (TX / 2);
            const int i = tx * TX + 2 * cx, j = tj0 + 2 * cy;
            if (i < v.nx && j >= 0 && j < v.ny) {
                const double *q0 = lq + (2 * cy) * TX + 2 * cx, *p0 = lds + (HY + 2 * cy) * LX + HX + 2 * cx;
                double acc = 0.0, accp = 0.0;
                acc = acc + q0[0]; accp = accp + p0[0] / 4.0;
                acc = acc + q0[1]; accp = accp + p0[1] / 4.0;
                acc = acc + q0[TX]; accp = accp + p0[LX] / 4.0;
                acc = acc + q0[TX + 1]; accp = accp + p0[LX + 1] / 4.0;
                const int ic = ((j >> 1) + g.rgy) * g.rP + SUHMO_XOFF + (i >> 1);
                g.rres[ic] = acc; g.rphi[ic] = accp;
            }
        }
    }
}
#define TILE_KERNEL_ATTRS(S, T, RST) __launch_bounds__((TileThreads<S, T, RST>::NT)) __attribute__((amdgpu_waves_per_eu((TileThreads<S, T, RST>::NT == 384 ? 3 : 2))))
template <int S, int T, bool HAS_ALPHA, bool RST = false, bool CHUNKED = false>
__global__ TILE_KERNEL_ATTRS(S, T, RST) void k_gsrb_tile(DV v, FP fp, const double *__restrict__ pin, double *__restrict__ pout, suhmo_phys_t ph, TileGeom g)
{
    d_gsrb_tile<S, T, HAS_ALPHA, RST, CHUNKED>(v, fp, pin, pout, ph, g);
}
// every active member of a batch in one launch (blockIdx.z, through the active list: suhmo_batch.h): the member's row of the tables, its
// head canvases as `alt` says they lie, the coarse canvases of the fused prolongation from the coarse depth's row
template <int S, int T, bool HAS_ALPHA, bool CHUNKED>
__global__ TILE_KERNEL_ATTRS(S, T, false) void k_gsrb_tile_b(BatchTab t, BatchTab c, BatchSel sel, TileGeom g, int prolong)
{
    const int k = batch_member(sel);
    const DV v = t.dv[k];
    const FP fp = batch_fp(t, k);
    const suhmo_phys_t ph = t.ph[k];
    if (prolong) { const FP fc = batch_fp(c, k); g.pc = fc.f[SUHMO_F_PHI]; g.pco = fc.f[SUHMO_F_PHIOLD]; }
    d_gsrb_tile<S, T, HAS_ALPHA, false, CHUNKED>(v, fp, fp.f[SUHMO_F_PHI], fp.f[SUHMO_F_PHI2], ph, g);
}
static bool tile_ok(const suhmo_level *L, const Depth &D)
{
    const DV &v = D.v;
    if (!L->gsrb_tile || !suhmo_batch_tile_ok(v)) return false;
    if ((v.rk[0] || v.rk[1]) && (!L->ex || !L->tile_strips || L->desc.nx_global > 0 || v.gy < 10 || v.ny < 10)) return false;   // rank strips: 2S + 1
                                                              // valid halo rows per launch (AMR patch strips: colour passes)
    return true;
}
// what the tile kernel asks of the grid itself (a batch, whole levels only, asks nothing else)
bool suhmo_batch_tile_ok(const DV &v)
{
    if (v.nx & 1) return false;                               // column pairs
    if (v.per[1] && (v.ny & 1)) return false;                 // colour of a periodic image = colour of the cell
    if ((v.per[0] && v.cfx[0] != v.cfx[1]) || (v.per[1] && v.ext[0] != v.ext[1])) return false;   // patch on one side of a periodic domain
    return true;
}

// the instantiations of k_gsrb_tile (chunked: S = 4 only), each with what the host needs for its grid
typedef void (*TileFn)(DV, FP, const double *, double *, suhmo_phys_t, TileGeom);
struct TileKernel { int key; TileFn fn; int NT, TX, TY; };
constexpr int tile_key(int S, int T, bool alpha, bool rst, bool chunked) { return S | alpha << 4 | rst << 5 | chunked << 6 | T << 8; }   // (S < 16)
#define TK(S, T, A, R, C) {tile_key(S, T, A, R, C), k_gsrb_tile<S, T, A, R, C>, TileThreads<S, T, R>::NT, TileShape<T, R>::TX, TileShape<T, R>::TY}
#define TK_ST(S, T, C) TK(S, T, false, false, C), TK(S, T, true, false, C), TK(S, T, false, true, C), TK(S, T, true, true, C)
static const TileKernel tile_kernels[] = {
    TK_ST(4, 16, false), TK_ST(4, 32, false), TK_ST(2, 16, false), TK_ST(2, 32, false), TK_ST(1, 16, false), TK_ST(1, 32, false),
    TK_ST(4, 16, true), TK_ST(4, 32, true),
};
#undef TK_ST
#undef TK
static const TileKernel *tile_kernel(int S, int T, bool alpha, bool rst, bool chunked)
{
    const int key = tile_key(S, T, alpha, rst, chunked);
    for (const TileKernel &k : tile_kernels) if (k.key == key) return &k;
    return nullptr;
}
static int launch_tile(suhmo_level *L, int depth, const RelaxStep &s, hipStream_t st)
{
    Depth &D = L->d[depth];
    const DV &v = D.v;
    const TileKernel *k = tile_kernel(s.S, s.T, v.alpha != 0.0, s.rst, s.chunks > 1);
    if (!k) { suhmo_set_error("internal: a tile relaxation step without a kernel"); return -4; }
    if (!D.phi_alt) {
        HIPCHK(hipMalloc(&D.phi_alt, D.elems * sizeof(double)));
        HIPCHK(hipMemsetAsync(D.phi_alt, 0, D.elems * sizeof(double), st));
    }
    TileGeom g;
    g.jbeg = v.rk[0] ? -s.adv : 0; g.jend = v.ny + (v.rk[1] ? s.adv : 0);
    g.ntx = (v.nx + k->TX - 1) / k->TX; g.nty = (g.jend - g.jbeg + k->TY - 1) / k->TY;
    g.pc = g.pco = nullptr; g.Pc = g.gyc = 0;
    g.rres = g.rphi = nullptr; g.rP = g.rgy = 0;
    if (s.rst) {
        Depth &C = L->d[depth + 1];
        g.rres = C.fp.f[SUHMO_F_RES]; g.rphi = C.fp.f[SUHMO_F_PHI]; g.rP = C.v.P; g.rgy = C.v.gy;
        C.phi_fresh = 0;
    }
    if (s.prolong) {
        Depth &C = L->d[depth + 1];
        g.pc = C.fp.f[SUHMO_F_PHI]; g.pco = C.fp.f[SUHMO_F_PHIOLD]; g.Pc = C.v.P; g.gyc = C.v.gy;
        D.prolong_pending = 0;
    }
    g.chunks = s.chunks;
    g.order = L->tile_order;
    g.frhs = 0;
    if (s.frhs) {
        if (!suhmo_field(L, depth, SUHMO_F_LPHI) || !suhmo_field(L, depth, SUHMO_F_PHIOLD)) return -2;
        g.frhs = 1; D.rhs_pending = 0; L->frhs_tile++;
    }
    hipLaunchKernelGGL(k->fn, dim3(g.ntx * g.nty), dim3(k->NT), 0, st, v, D.fp, (const double *)D.fp.f[SUHMO_F_PHI], D.phi_alt, L->ph, g);
    { std::swap(D.fp.f[SUHMO_F_PHI], D.phi_alt); suhmo_fp_changed(); }
    return 0;
}

// sweeps per launch of the streaming kernel, 0 = not the streaming kernel; tile: tile_ok(L, D)
static int pick_K(const suhmo_level *L, const Depth &D, bool tile, int remaining)
{
    int variant = L->gsrb_variant;       // -1 auto, 0 simple, 1 fused K=1, 2 fused K=2
    if (variant < 0) {
        // the streaming kernel pays ~(Hc + 4K) serial row steps per workgroup: below ~2M cells
        // (cache-resident depths) two plain colour-pass launches are faster
        // (profiles/r01_c_vcycle_trace.txt)
        const long cells = (long)D.v.nx * D.v.ny;
        variant = (cells >= (long)L->fused_min_cells) ? 2 : 0;
        // whole levels of up to a few million cells: 4 sweeps per launch on LDS tiles beat 2 per streaming pass
        // (profiles/r01_s_tile_vs_streaming.txt: 2048^2 47.5 vs 56.8 us per sweep, 4096^2 175 vs 146)
        if (tile && cells < L->tile_max_cells) variant = 0;
    }
    if (variant >= 2 && remaining >= 2 && fused_ok(L, D, 2)) return 2;
    if (variant >= 1 && fused_ok(L, D, 1)) return 1;
    return 0;
}
// rank strips: halo rows that are valid on the fine depth AND (halved) on the coarse one stay valid when the
// correction is added while loading
static int prolong_halo_rows(const suhmo_level *L, int depth)
{
    const Depth &D = L->d[depth], &C = L->d[depth + 1];
    int R = D.phi_fresh < 2 * C.phi_fresh ? D.phi_fresh : 2 * C.phi_fresh;
    return R & ~1;
}
static int pending(const Depth &D)
{
    return (D.prolong_pending ? ABSORB_PROLONG : 0) | (D.rhs_pending ? ABSORB_RHS : 0) | (D.bcoef_pending ? ABSORB_BCOEF : 0);
}
// the depth has halo rows that a transport keeps current
static bool has_halo(const suhmo_level *L, const DV &v) { return L->ex && (v.ext[0] || v.ext[1]); }

// THE schedule: the next launch of a relaxation of `depth` with `left` sweeps to go.  restricts: the caller restricts right after these sweeps;
// absorb: what waits for the launch (ABSORB_*); tail: halo rows worth keeping current for the next reader.  Rank strips: F = halo rows of phi
// that hold current neighbour values (Depth::phi_fresh).  A colour pass needs 1, an S- or K-sweep launch 2S or 2K, one more when it restricts
// or evaluates the residual (one exchange instead of the one the separate pass would ask for); each launch also advances, redundantly, as
// many of the remaining halo rows as the work still to come can use, so one exchange of halo_rows rows feeds up to halo_rows colour passes.
// settled: F is all there will be (exchanged already, or no exchange can help): a tile launch it does not feed gives way to colour passes,
// a launch one row short does not restrict and leaves no residual behind; !settled: the step says what it needs and the caller exchanges.
// No side effects: it reads the level and answers.
static RelaxStep relax_step(const suhmo_level *L, int depth, int left, int tail, bool restricts, int F, bool settled, int absorb)
{
    const Depth &D = L->d[depth];
    const DV &v = D.v;
    const bool ext = has_halo(L, v), stored = v.ext[0] || v.ext[1];
    const long cells = (long)v.nx * v.ny;
    // a coarse cell's two fine rows are this depth's own
    const bool can_restrict = restricts && L->fused_restrict && depth + 1 < L->ndepth && !(v.ny & 1) && !(v.j0 & 1);
    const bool tile = tile_ok(L, D);
    const int K = pick_K(L, D, tile, left);
    RelaxStep s{};
    if (K == 0 && tile) {
        const TileStep t = plan_tile_step(left, L->tile_s, L->tile_chunks && !ext ? plan_single_tile(L->tile_t, v.nx, v.ny) : 0, plan_tile_edge(L->tile_t, cells));
        s.rst = can_restrict && (L->tile_restrict == 1 || (L->tile_restrict == 2 && ext)) && t.S * t.chunks == left;
        // rank strip: the tile's halo rows beyond the strip are the neighbour's cells; they are advanced redundantly and stale afterwards
        s.need = ext ? 2 * t.S + (s.rst ? 1 : 0) : 0;
        if (!(settled && F < s.need)) {
            s.path = STEP_TILE; s.S = t.S; s.chunks = t.chunks; s.T = t.T; s.done = t.S * t.chunks;
            s.frhs = absorb & ABSORB_RHS; s.prolong = absorb & ABSORB_PROLONG;
            s.adv = ext ? plan_halo_advance(F, s.need, 2 * (left - t.S) + tail, v.gy - s.need, true) : 0;
            return s;
        }
        s = RelaxStep{}; s.shallow = true;
    }
    if (K == 0) { s.path = STEP_COLOUR; s.done = 1; s.need = ext ? 1 : 0; return s; }      // (each of its two passes asks for its row and advances its own)
    s.path = STEP_STREAM; s.K = s.done = K; s.NT = plan_stream_threads(L->fused_nt, cells);
    // the ice mask is known clean (suhmo_common.h): the instantiation without it (alpha = 0 operators: the head solve)
    s.masked = !(suhmo_mask_clean(L, depth) && v.alpha == 0.0);
    s.prolong = absorb & ABSORB_PROLONG;
    // the variants exist for the two-sweep launch of one-wave workgroups with alpha = 0 (with aCoef the extra coefficient row no longer fits
    // 2 waves per SIMD); restricting and the residual belong to the launch that ends the sweeps, not on AMR patches
    const bool variants = K == 2 && s.NT == 64 && v.alpha == 0.0, last = K == left;
    // the bed is known to be one value (suhmo_common.h): every variant of the clean-mask cycle of a whole level has an instantiation without it
    s.zbu = variants && !s.masked && !stored && suhmo_zb_uniform(L, depth);
    s.rst = can_restrict && variants && last && (!stored || (ext && L->desc.nx_global == 0 && v.gy >= 5));
    // the launch that ends the cycle (armed by the cycle for its last relax of depth 0) also leaves the residual of the final phi behind (same
    // needs as the restricting launch: one more final row and column around a chunk)
    s.rout = L->resout_armed && depth == 0 && !restricts && variants && last && (!stored || ext) && L->desc.nx_global == 0 && !(absorb & ABSORB_RHS);
    if (ext && settled && F < 2 * K + 1) s.rst = s.rout = false;      // (the solve loop then evaluates the residual in its own pass)
    s.need = ext ? 2 * K + (s.rst || s.rout ? 1 : 0) : 0;
    const bool plain = variants && !s.rst && !s.rout;
    s.frhs = (absorb & ABSORB_RHS) && plain;
    // depth 0 of a whole level -- no rank strip, no AMR patch -- with a mask known clean, and nothing else to absorb
    s.bcf = absorb == ABSORB_BCOEF && plain && depth == 0 && !stored && !s.masked;
    // the plain launch with the bed as a scalar that absorbs nothing but a prolongation: one ring of y-faces.  Not where y is periodic: face 0
    // and face ny are two canvas rows of by there, whose bits may differ (a ghost row of B that is not the periodic image)
    s.yring = L->yface_ring && s.zbu && plain && !s.frhs && !s.bcf && !v.per[1];
    // (the launch that forms the right-hand side loads, and keeps, all halo rows)
    s.adv = ext ? plan_halo_advance(F, s.need, (absorb & ABSORB_RHS) ? F : 2 * (left - K) + tail, v.gy - s.need, s.rst) : 0;
    return s;
}

// a two-sweep relaxation of the depth runs on the streaming kernel (what the scan of the bed elevation asks, suhmo_level.hip)
bool suhmo_gsrb_streams(const suhmo_level *L, int depth) { return relax_step(L, depth, 2, 0, false, 0, false, 0).path == STEP_STREAM; }

// ---- what suhmo_fas.hip asks before it leaves a pass to the first launch of a relaxation: would that launch absorb it?
// the first relaxation of a coarse FAS depth can form its right-hand side itself
bool suhmo_gsrb_can_fuse_rhs(suhmo_level *L, int depth, int sweeps, bool rhs_local)
{
    const Depth &D = L->d[depth];
    if (sweeps < 1 || !L->fas_rhs_in_relax) return false;
    const RelaxStep s = relax_step(L, depth, sweeps, 0, false, 0, false, ABSORB_RHS);
    if (!s.frhs) return false;
    const bool strip = D.v.rk[0] || D.v.rk[1];
    // tile launch: not on rank strips, where k_apply<., 2> also copies the halo rows of R phi
    if (s.path == STEP_TILE) return !strip && (L->fas_rhs_in_relax & 1);
    // streaming launch: not with fewer than four sweeps (with only two to do that launch is the one that restricts)
    if (!(L->fas_rhs_in_relax & 2) || sweeps < 4) return false;
    if (!(D.v.ext[0] || D.v.ext[1])) return true;
    // rank strip: R phi and RES have just arrived in all halo rows (the caller's rhs_local exchange); the launch then loads all of them
    return strip && L->ex && rhs_local && L->desc.nx_global == 0 && D.phi_fresh >= D.v.gy && D.v.gy >= 2 * s.K + 1 && D.v.ny >= D.v.gy;
}
// the first pre-smoothing launch of depth 0 can be the cycle's UpdateOperator as well (k_gsrb_fused<.., BCF>)
bool suhmo_gsrb_can_fuse_bcoef(suhmo_level *L, int sweeps)
{
    if (!L->bcoef_in_relax || L->ex) return false;            // (hooks: the faces' halo rows travel with the coarse depths', suhmo_fas.hip)
    const RelaxStep s = relax_step(L, 0, sweeps, 0, false, 0, false, ABSORB_BCOEF | pending(L->d[0]));
    return s.bcf && sweeps >= 3;         // the smoothing goes on after it (the launch that ends one restricts or leaves the residual behind)
}
// AverageOperator behind that launch may leave the cycle's stream: the next launch of depth 0 (two sweeps and the restriction) reads none of the
// coarse faces, so the two can share the GPU -- k_average_faces_all<OnLevel, ..> fits beside two resident waves of that launch per SIMD.
// suhmo_gsrb_can_fuse_bcoef has excluded rank strips, agglomerated levels and exchange hooks; not inside a capture (a captured graph keeps
// one branch) and not while profiling (the event pairs keep timing one launch each)
bool suhmo_gsrb_can_overlap_avg(const suhmo_level *L)
{
    return L->avg_overlap && !L->mask_capturing && !L->prof_on && !L->ex && !L->agg && !L->ex_begin && !L->ex_end && !L->ipc;
}
// the fork: an event behind the launch that stored depth 0's faces, the averages behind it on the level's side stream, an event behind them
// (enqueued before the launch they run beside: enqueued after it the cycle takes the same time, profiles/r21_avg_overlap_bench_parent_new_alternation.txt)
static int avg_fork(suhmo_level *L, hipStream_t st)
{
    if (!L->astream) {
        HIPCHK(hipStreamCreateWithFlags(&L->astream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&L->aev[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&L->aev[1], hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(L->aev[0], st));
    HIPCHK(hipStreamWaitEvent(L->astream, L->aev[0], 0));
    int rc = suhmo_average_operator_all(L, L->bcoef_nd, L->astream); if (rc) return rc;
    HIPCHK(hipEventRecord(L->aev[1], L->astream));
    L->avg_flying = 1; L->avg_overlap_count++;
    return 0;
}
// ... and the join, before anything on st that reads a coarse face or hands the level back to the caller
int suhmo_avg_join(suhmo_level *L, hipStream_t st)
{
    if (!L->avg_flying) return 0;
    L->avg_flying = 0;
    HIPCHK(hipStreamWaitEvent(st, L->aev[1], 0));
    return 0;
}
void suhmo_avg_release(suhmo_level *L)
{
    if (!L->astream) return;
    (void)hipStreamDestroy(L->astream); (void)hipEventDestroy(L->aev[0]); (void)hipEventDestroy(L->aev[1]);
    L->astream = nullptr; L->aev[0] = L->aev[1] = nullptr; L->avg_flying = 0;
}
// the first post-smoothing launch can add the prolonged correction while loading
bool suhmo_gsrb_can_fuse_prolong(suhmo_level *L, int depth, int sweeps)
{
    const Depth &D = L->d[depth];
    if (sweeps < 1 || depth + 1 >= L->ndepth) return false;
    const RelaxStep s = relax_step(L, depth, sweeps, 0, false, 0, false, ABSORB_PROLONG);
    if (!s.prolong) return false;                                         // colour passes
    const bool stored = D.v.ext[0] || D.v.ext[1];
    if (s.path == STEP_STREAM && stored && !L->ex) return false;          // stored ghost rows without a transport (AMR patch)
    // the halo rows the launch reads carry the correction on both depths (the tile launch is asked about rank sides only: the stored rows
    // of a coarse-fine side are interpolated, not exchanged, and suhmo_launch_gsrb checks them)
    const bool halo = s.path == STEP_TILE ? (D.v.rk[0] || D.v.rk[1]) : stored;
    return !halo || prolong_halo_rows(L, depth) >= s.need;                // else: un-fused prolongation, then an exchange
}

// the executor of relax_step.  restricted != NULL: the caller restricts right after these sweeps (pre-smoothing of the FAS cycle);
// *restricted = 1 if the last launch did it (coarse RES and PHI written), 0 if the caller still has to
int suhmo_launch_gsrb(suhmo_level *L, int depth, int sweeps, int tail, hipStream_t st, int *restricted)
{
    Depth &D = L->d[depth];
    const bool ext = has_halo(L, D.v);
    if (restricted) *restricted = 0;
    // (the first launch adds the correction while loading: only the halo rows current on BOTH depths may be read)
    int F = !ext ? 0 : D.prolong_pending ? prolong_halo_rows(L, depth) : D.phi_fresh;
    if (depth > 0) { int rc = suhmo_avg_join(L, st); if (rc) return rc; }   // the coarse faces, should they still be in flight on the side stream
    for (int it = 0; it < sweeps;) {
        const int left = sweeps - it, absorb = pending(D);
        // (no exchange can deepen the halo under a pending correction: the neighbour's phi lacks it as well)
        const bool settled = !ext || D.prolong_pending;
        RelaxStep s = relax_step(L, depth, left, tail, restricted != nullptr, F, settled, absorb);
        bool flying = false;                                               // the exchange is in flight on the second stream
        if (!settled && s.path != STEP_COLOUR && F < s.need) {
            // only the native transport is stream-ordered (its pack / send / recv / unpack are enqueued on the stream the hook is
            // given); a host transport (torch.distributed, gloo, threads) orders against other streams or the whole device:
            // overlap_halo = 1 overlaps with the native transport only, 2 = the caller vouches for its hook
            flying = s.path == STEP_STREAM && (L->overlap_halo == 2 || (L->overlap_halo && (L->rccl || L->ipc))) && D.v.ny >= 6 * s.need;
            if (flying) {
                if (!L->xstream) {
                    HIPCHK(hipStreamCreateWithFlags(&L->xstream, hipStreamNonBlocking));
                    HIPCHK(hipEventCreateWithFlags(&L->xev[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&L->xev[1], hipEventDisableTiming));
                }
                HIPCHK(hipEventRecord(L->xev[0], st));                     // the rows that travel are final
                HIPCHK(hipStreamWaitEvent(L->xstream, L->xev[0], 0));
            }
            int rc = suhmo_ensure_phi_halo(L, depth, s.need, flying ? L->xstream : st); if (rc) return rc;
            if (flying) HIPCHK(hipEventRecord(L->xev[1], L->xstream));
            F = D.phi_fresh;
            s = relax_step(L, depth, left, tail, restricted != nullptr, F, true, absorb);
        }
        // the one check that the step takes up everything that waits for it and has the halo it reads
        if (s.absorbs() != absorb || (ext && s.path != STEP_COLOUR && F < s.need)) {
            suhmo_set_error("internal: a relaxation launch that takes %d of what is pending (%d) or reads %d halo rows of %d", s.absorbs(), absorb, s.need, F);
            return -4;
        }
        if (s.shallow) L->strip_tile_shallow++;
        ProfEv pe{};
        const bool prof = L->prof_on && depth == 0;
        if (prof) {
            HIPCHK(hipEventCreate(&pe.a)); HIPCHK(hipEventCreate(&pe.b));
            HIPCHK(hipEventRecord(pe.a, st));
        }
        int rc = 0;
        if (s.path == STEP_TILE) {
            rc = launch_tile(L, depth, s, st);
            if (!rc && ext) { L->strip_tile++; if (s.rst) L->strip_tile_rst++; }
        } else if (s.path == STEP_COLOUR) {
            for (int pass = 0; pass < 2; pass++) {
                if (ext && F < 1) {
                    if ((rc = suhmo_ensure_phi_halo(L, depth, 1, st))) return rc;
                    F = D.phi_fresh;
                }
                // halo rows the work after this pass can use (AMR patch strips: the coarse-fine ghost columns of halo rows are not exchanged -> none)
                const int E = ext ? plan_halo_advance(F, 1, 2 * left - (pass + 1) + tail, L->desc.nx_global > 0 ? 0 : D.v.gy - 1, false) : 0;
                if ((rc = launch_simple(L, depth, pass, E, st))) return rc;
                if (ext) { F = E; D.phi_fresh = F; L->strip_colour++; }
            }
        } else {
            if (flying) {
                rc = launch_fused(L, depth, s, st, 1);                     // the chunks that read no halo row: now
                if (rc < 0) return rc;
                HIPCHK(hipStreamWaitEvent(st, L->xev[1], 0));              // the halo rows have arrived
                if (rc == 1) rc = launch_fused(L, depth, s, st, 0); else { rc = launch_fused(L, depth, s, st, 2); L->overlapped++; }
            } else rc = launch_fused(L, depth, s, st);
            if (!rc && ext) { L->strip_stream++; if (s.rst) L->strip_stream_rst++; }
        }
        if (rc) return rc;
        if (s.rst) *restricted = 1;
        if (s.rout) { L->resout_done = 1; L->resout_count++; }
        if (ext && s.path != STEP_COLOUR) { F = s.adv; D.phi_fresh = F; }
        if (prof) {
            HIPCHK(hipEventRecord(pe.b, st));
            pe.cells = (long)D.v.nx * D.v.ny * s.done;
            pe.restricts = s.bcf ? 2 : s.rst ? 1 : 0;
            L->prof.push_back(pe);
        }
        // AverageOperator reads the faces that launch has just stored: right behind it, on the side stream where the cycle allows (avg_fork)
        if (s.bcf) { rc = L->avg_fork ? avg_fork(L, st) : suhmo_average_operator_all(L, L->bcoef_nd, st); if (rc) return rc; }
        it += s.done;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ a batch of whole levels (suhmo_batch.hip): every active member in one launch
// the instantiations of k_gsrb_tile_b (chunked: S = 4 only)
typedef void (*TileBFn)(BatchTab, BatchTab, BatchSel, TileGeom, int);
struct TileBKernel { int key; TileBFn fn; int NT; };
#define TB(S, T, A, C) {tile_key(S, T, A, false, C), k_gsrb_tile_b<S, T, A, C>, TileThreads<S, T, false>::NT}
#define TB_ST(S, T, C) TB(S, T, false, C), TB(S, T, true, C)
static const TileBKernel tile_b_kernels[] = {
    TB_ST(4, 16, false), TB_ST(4, 32, false), TB_ST(2, 16, false), TB_ST(2, 32, false), TB_ST(1, 16, false), TB_ST(1, 32, false),
    TB_ST(4, 16, true), TB_ST(4, 32, true),
};
#undef TB_ST
#undef TB
static const TileBKernel *tile_b_kernel(int S, int T, bool alpha, bool chunked)
{
    const int key = tile_key(S, T, alpha, false, chunked);
    for (const TileBKernel &k : tile_b_kernels) if (k.key == key) return &k;
    return nullptr;
}
// T = 16 for depths of several tiles (the small levels a batch is for), 16 or 32 for a depth that is one tile (chunks > 1: S = 4)
int suhmo_batch_gsrb_tile(const BatchTab &t, const BatchTab *coarse, const DV *vc, const BatchSel &sel, const DV &v, int S, int T, int chunks, bool frhs, bool prolong,
                          bool has_alpha, int order, hipStream_t st)
{
    if (sel.n <= 0) return 0;
    TileGeom g;
    g.jbeg = 0; g.jend = v.ny;
    g.ntx = (v.nx + T - 1) / T; g.nty = (v.ny + T - 1) / T;
    g.pc = g.pco = nullptr; g.Pc = g.gyc = 0;
    g.rres = g.rphi = nullptr; g.rP = g.rgy = 0;
    const TileBKernel *k = tile_b_kernel(S, T, has_alpha, chunks > 1);
    if (!k || (chunks > 1 && g.ntx * g.nty != 1)) { suhmo_set_error("internal: a tile relaxation step of a batch without a kernel"); return -4; }
    if (prolong) {
        if (!coarse || !vc) { suhmo_set_error("internal: fused prolongation without the coarse tables"); return -4; }
        g.Pc = vc->P; g.gyc = vc->gy;                         // (the canvases themselves: the member's coarse row, in the kernel)
    }
    g.chunks = chunks; g.order = order; g.frhs = frhs ? 1 : 0;
    hipLaunchKernelGGL(k->fn, dim3(g.ntx * g.nty, 1, sel.n), dim3(k->NT), 0, st, t, coarse ? *coarse : t, sel, g, (int)prolong);
    HIPCHK(hipGetLastError());
    return 0;
}
