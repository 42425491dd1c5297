// suhmo_bcoef.hip -- UpdateOperator (WFlx_level: gradient, Re, bCoef on faces; the fused single-kernel form), AverageOperator and MGnewOp's
// coefficient coarsening.  (Split off suhmo_level.hip in round 4; reference citations: file:line in the SUHMO checkout.)
#include "suhmo_hier.h"
#include "suhmo_level_int.h"
#include "suhmo_batch.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>
// ------------------------------------------------------------------ bCoef update (WFlx_level)
// step 1: cell-centred gradient = EdgeToCell(NEWMACGRAD) (util/Gradient.cpp:96-127, :623;
// util/GradientF.ChF:57-70)
__device__ __forceinline__ void d_gradcc_val(const DV &v, const FP &fp, int hasMask, int i, int j, double &gx, double &gy)
{
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    int idx = cidx(v, i, j);
    double c = phi[idx];
    double e = phiE(v, phi, idx, i, c, false), w = phiW(v, phi, idx, i, c, false);
    double n = phiN(v, phi, idx, j, c, false), s = phiS(v, phi, idx, j, c, false);
    bool zW = false, zE = false, zS = false, zN = false;
    if (hasMask) {
        const double *__restrict__ m = fp.f[SUHMO_F_MASK];
        bool mc = m[idx] < 1e-6;
        zW = mc || m[idx - 1] < 1e-6;
        zE = mc || m[idx + 1] < 1e-6;
        zS = mc || m[idx - v.P] < 1e-6;
        zN = mc || m[idx + v.P] < 1e-6;
    }
    gradcc_from(v, c, w, e, s, n, zW, zE, zS, zN, gx, gy);
}
__device__ __forceinline__ void d_gradcc_at(const DV &v, const FP &fp, int hasMask, int i, int j)
{
    if (i >= v.nx || j >= v.ny) return;
    double gx, gy;
    d_gradcc_val(v, fp, hasMask, i, j, gx, gy);
    const int idx = cidx(v, i, j);
    fp.f[SUHMO_F_GRADX][idx] = gx;
    fp.f[SUHMO_F_GRADY][idx] = gy;
}
__device__ __forceinline__ void d_gradcc(const DV &v, const FP &fp, int hasMask)
{
    d_gradcc_at(v, fp, hasMask, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * blockDim.y + threadIdx.y);
}
template <class T> __global__ __launch_bounds__(256) void k_gradcc(T t) { d_gradcc(t.view(), t.fields(), t.phys().use_mask_gradients); }
// the same at a list of cells (x = i, y = j): the coarse cells a finer level's coarse-fine interpolation of the gradient reads
__global__ __launch_bounds__(256) void k_gradcc_list(DV v, FP fp, int hasMask, const int2 *__restrict__ cells, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    d_gradcc_at(v, fp, hasMask, cells[t].x, cells[t].y);
}
// step 2: ghosts of the gradient: exchange (periodic wrap) + ExtrapGhostCells
// (src/AmrHydro.cpp:1490-1491, util/ExtrapGhostCells.cpp:94-180, util/ExtrapBCF.ChF:21-29)
__device__ __forceinline__ void d_grad_ghosts(const DV &v, double *__restrict__ gx, double *__restrict__ gy)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    double *g2[2] = {gx, gy};
    if (t < 2 * v.ny) {
        int side = t / v.ny, j = t % v.ny;
        if (v.cfx[side]) return;
        for (int c = 0; c < 2; c++) {
            double *g = g2[c];
            if (side == 0) { int idx = cidx(v, 0, j); g[idx - 1] = v.per[0] ? g[idx + v.nx - 1] : 2.0 * g[idx] - g[idx + 1]; }
            else { int idx = cidx(v, v.nx - 1, j); g[idx + 1] = v.per[0] ? g[idx - (v.nx - 1)] : 2.0 * g[idx] - g[idx - 1]; }
        }
        return;
    }
    t -= 2 * v.ny;
    if (t < 2 * v.nx) {
        int side = t / v.nx, i = t % v.nx;
        if (v.ext[side]) return;
        for (int c = 0; c < 2; c++) {
            double *g = g2[c];
            if (side == 0) { int idx = cidx(v, i, 0); g[idx - v.P] = v.per[1] ? g[idx + (v.ny - 1) * v.P] : 2.0 * g[idx] - g[idx + v.P]; }
            else { int idx = cidx(v, i, v.ny - 1); g[idx + v.P] = v.per[1] ? g[idx - (v.ny - 1) * v.P] : 2.0 * g[idx] - g[idx - v.P]; }
        }
    }
}
template <class T> __global__ void k_grad_ghosts(T t)
{
    const FP &fp = t.fields();
    d_grad_ghosts(t.view(), fp.f[SUHMO_F_GRADX], fp.f[SUHMO_F_GRADY]);
}
// steps 1 + 2 of every box of a level in ONE launch: the thread of a cell on a physical side of its box also writes the ghost cell beyond it,
// from the gradient of the neighbour the extrapolation (or the periodic wrap) reads, evaluated a second time: d_grad_ghosts' expressions on the
// same values (boxes of AMR levels are at least two cells wide: block_factor 2)
__device__ __forceinline__ void d_gradcc_ghosts(const DV &v, const FP &fp, int hasMask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    double gx, gy, ox, oy;
    d_gradcc_val(v, fp, hasMask, i, j, gx, gy);
    const int idx = cidx(v, i, j);
    double *__restrict__ GX = fp.f[SUHMO_F_GRADX], *__restrict__ GY = fp.f[SUHMO_F_GRADY];
    GX[idx] = gx; GY[idx] = gy;
    if (i == 0 && !v.cfx[0]) {
        d_gradcc_val(v, fp, hasMask, v.per[0] ? v.nx - 1 : 1, j, ox, oy);
        GX[idx - 1] = v.per[0] ? ox : 2.0 * gx - ox; GY[idx - 1] = v.per[0] ? oy : 2.0 * gy - oy;
    }
    if (i == v.nx - 1 && !v.cfx[1]) {
        d_gradcc_val(v, fp, hasMask, v.per[0] ? 0 : v.nx - 2, j, ox, oy);
        GX[idx + 1] = v.per[0] ? ox : 2.0 * gx - ox; GY[idx + 1] = v.per[0] ? oy : 2.0 * gy - oy;
    }
    if (j == 0 && !v.ext[0]) {
        d_gradcc_val(v, fp, hasMask, i, v.per[1] ? v.ny - 1 : 1, ox, oy);
        GX[idx - v.P] = v.per[1] ? ox : 2.0 * gx - ox; GY[idx - v.P] = v.per[1] ? oy : 2.0 * gy - oy;
    }
    if (j == v.ny - 1 && !v.ext[1]) {
        d_gradcc_val(v, fp, hasMask, i, v.per[1] ? 0 : v.ny - 2, ox, oy);
        GX[idx + v.P] = v.per[1] ? ox : 2.0 * gx - ox; GY[idx + v.P] = v.per[1] ? oy : 2.0 * gy - oy;
    }
}
__global__ __launch_bounds__(256) void k_gradcc_ghosts(OnBoxes t) { d_gradcc_ghosts(t.view(), t.fields(), t.phys().use_mask_gradients); }
// ... of SEVERAL levels (UpdateOperator of an AMR level evaluates the gradient of its own and of the coarser level)
__global__ __launch_bounds__(256) void k_gradcc_ghosts_lv(suhmo_lvboxes lv, int hasMask)
{
    int z = blockIdx.z, q = -1;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++)
        if (t < lv.n && q < 0) { if (z < lv.nbox[t]) q = t; else z -= lv.nbox[t]; }
    if (q < 0) return;
    const DV *dv = nullptr; const FP *fp = nullptr;
#pragma unroll
    for (int t = 0; t < SUHMO_LVMAX; t++) if (t == q) { dv = lv.dv[t]; fp = lv.fp[t]; }
    d_gradcc_ghosts(dv[z], fp[z], hasMask);
}
// step 3: COMPUTERE on the ghosted box (src/AmrHydro.cpp:1495-1505, src/AmrHydroF.ChF:92-109)
__device__ __forceinline__ double d_re_val(const FP &fp, const suhmo_phys_t &ph, int idx)
{
    double gx = fp.f[SUHMO_F_GRADX][idx], gy = fp.f[SUHMO_F_GRADY][idx], B = fp.f[SUHMO_F_B][idx];
    return re_from(ph, grad_norm(gx, gy), B);
}
__device__ __forceinline__ void d_re(const DV &v, const FP &fp, suhmo_phys_t ph)
{
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    bool xo = (i < 0 || i >= v.nx), yo = (j < 0 || j >= v.ny);
    if (xo && yo) return;                                      // corner ghosts are never read
    int idx = cidx(v, i, j);
    fp.f[SUHMO_F_RE][idx] = d_re_val(fp, ph, idx);
}
template <class T> __global__ __launch_bounds__(256) void k_re(T t) { d_re(t.view(), t.fields(), t.phys()); }
// step 4: CellToEdge(Re), CellToEdge(B), setup_iceMask_EC, COMPUTEBCOEFF: bcoef_face (suhmo_common.h)
__device__ __forceinline__ void d_bcoef_faces(const DV &v, const FP &fp, suhmo_phys_t ph)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i > v.nx || j > v.ny) return;
    int idx = cidx(v, i, j);
    const double *__restrict__ Re = fp.f[SUHMO_F_RE], *__restrict__ B = fp.f[SUHMO_F_B], *__restrict__ m = fp.f[SUHMO_F_MASK];
    if (j < v.ny)   // x-face (i,j) between cells (i-1,j) and (i,j)
        fp.f[SUHMO_F_BX][idx] = bcoef_face(ph, Re[idx], Re[idx - 1], B[idx], B[idx - 1], m[idx], m[idx - 1], i + v.i0 == 0 || i + v.i0 == v.nxg);
    if (i < v.nx) { // y-face (i,j) between cells (i,j-1) and (i,j)
        int jg = j + v.j0;
        fp.f[SUHMO_F_BY][idx] = bcoef_face(ph, Re[idx], Re[idx - v.P], B[idx], B[idx - v.P], m[idx], m[idx - v.P], jg == 0 || jg == v.nyg);
    }
}
template <class T> __global__ __launch_bounds__(256) void k_bcoef_faces(T t) { d_bcoef_faces(t.view(), t.fields(), t.phys()); }
// steps 3 + 4 of every box of a level in ONE launch: the thread of a position of the ghosted box stores Re there (d_re) and the two faces on
// its low sides (d_bcoef_faces), with the Re of the two cells across those faces evaluated a second time from the same gradient and gap height
__global__ __launch_bounds__(256) void k_re_bcoef(OnBoxes t)
{
    const DV &v = t.view();
    const FP &fp = t.fields();
    const suhmo_phys_t &ph = t.phys();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
    if (i > v.nx || j > v.ny) return;
    const bool xo = (i < 0 || i >= v.nx), yo = (j < 0 || j >= v.ny);
    if (xo && yo) return;                                      // corner ghosts are never read
    const int idx = cidx(v, i, j);
    const double Rc = d_re_val(fp, ph, idx);
    fp.f[SUHMO_F_RE][idx] = Rc;
    if (i < 0 || j < 0) return;                                // (faces (i, j), 0 <= i <= nx, 0 <= j <= ny)
    const double *__restrict__ B = fp.f[SUHMO_F_B], *__restrict__ m = fp.f[SUHMO_F_MASK];
    if (j < v.ny)
        fp.f[SUHMO_F_BX][idx] = bcoef_face(ph, Rc, d_re_val(fp, ph, idx - 1), B[idx], B[idx - 1], m[idx], m[idx - 1], i + v.i0 == 0 || i + v.i0 == v.nxg);
    if (i < v.nx) {
        const int jg = j + v.j0;
        fp.f[SUHMO_F_BY][idx] = bcoef_face(ph, Rc, d_re_val(fp, ph, idx - v.P), B[idx], B[idx - v.P], m[idx], m[idx - v.P], jg == 0 || jg == v.nyg);
    }
}

// ---- fused WFlx_level: one kernel = steps 1-4 above on a tile staged in LDS.
// A block of 64 x 4 threads owns BT_X x BT_Y = 62 x 14 cells (26 KB of LDS, 6 blocks per CU: 0.26 ms at 4096^2 vs
// 0.29 ms with 30 rows).  phi tile (halo 2) and
// the B / mask tiles (halo 1) are loaded up front (one exposure to HBM latency); then
// cell-centred gradient on the Re range (halo 1: one lane per column, NK rows per
// thread, in registers) -> ghost gradients by linear extrapolation (periodic images and
// exchanged halo rows are ordinary cells) -> Re (LDS, aliasing the dead phi tile) -> the
// tile's W and S faces (+ the domain's E / N faces in the last tile column / row).
// Every value comes from the same expressions as the four-kernel path (bitwise equal); halo
// cells are recomputed instead of stored, so HBM sees phi, B, mask once and bx, by once.
// Tile shapes: 62 x 14 on 64 x 4 threads, or 126 x 14 on 128 x 2 threads (BT_X + 2 lanes per row; level option bcoef_tile_x): the wider tile's
// rows are 1040 instead of 528 bytes, so the 128-byte lines its unaligned ends drag in weigh half as much.
// INTERIOR: the tile and its two-cell halo lie inside the level -- no boundary condition, no wrap, no missing cell: the
// same expressions without the case distinctions (most tiles; uniform per workgroup)
// MASKED = false (the host knows the level's mask clean, suhmo_common.h: every value this kernel could read is >= 1e-6): no mask load, no
// mask tile (18 instead of 26 KB of LDS), no mask test in the gradient, no report; bcoef_face sees two equal positive cells, so its early
// return folds away.  The same expressions in the same order otherwise.
template <bool INTERIOR, int BT_X, int BT_Y, bool MASKED>
__device__ __forceinline__ void bcoef_tile(const DV &v, const FP &fp, const suhmo_phys_t &ph, int hasMask_, double *sphi, double *sB, double *sM,
                                           unsigned *negflag, unsigned epoch, unsigned *smallflag)
{
    const int hasMask = MASKED ? hasMask_ : 0;
    constexpr int PW = BT_X + 4, PH = BT_Y + 4;     // phi tile: cells [i0-2, i0+BT_X+1] x [j0-2, j0+BT_Y+1]
    constexpr int RW = BT_X + 2, RH = BT_Y + 2;     // Re tile:  cells [i0-1, i0+BT_X]   x [j0-1, j0+BT_Y]
    constexpr int TX = BT_X + 2, TY = 256 / TX;     // threads of the workgroup: TX lanes along a row, TY rows at a time
    constexpr int NK = RH / TY;
    static_assert(TX * TY == 256 && RH % TY == 0, "tile shape");
    double *sre = sphi;                              // phi is dead once the gradients exist
    const int i0 = blockIdx.x * BT_X, j0 = blockIdx.y * BT_Y;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const double *__restrict__ phi = fp.f[SUHMO_F_PHI], *__restrict__ Bf = fp.f[SUHMO_F_B], *__restrict__ mk = fp.f[SUHMO_F_MASK];
    double *__restrict__ bxo = fp.f[SUHMO_F_BX], *__restrict__ byo = fp.f[SUHMO_F_BY];
    const bool halo_lo = v.ext[0], halo_hi = v.ext[1], selfper_y = v.per[1] && !halo_lo && !halo_hi;
    // a cell "exists" (has its own phi) inside the domain, as a periodic image, or in an exchanged halo row.  Images: one period to either side
    // (wrapx / wrapy wrap once); on a level narrower than the tile the positions further out are never used and must not be loaded
    auto xin = [&](int i) { return INTERIOR || (i >= 0 && i < v.nx) || (v.per[0] && i >= -v.nx && i < 2 * v.nx); };
    auto yin = [&](int j) { return INTERIOR || (j >= 0 && j < v.ny) || (selfper_y && j >= -v.ny && j < 2 * v.ny) || (j < 0 && halo_lo && j >= -v.gy) || (j >= v.ny && halo_hi && j < v.ny + v.gy); };
    auto wrapx = [&](int i) { return (!INTERIOR && v.per[0]) ? (i < 0 ? i + v.nx : (i >= v.nx ? i - v.nx : i)) : i; };
    auto wrapy = [&](int j) { return (!INTERIOR && selfper_y) ? (j < 0 ? j + v.ny : (j >= v.ny ? j - v.ny : j)) : j; };

    // ---- phi tile.  Cells that do not exist get the physical-BC ghost of their interior
    // neighbour (only the first ghost layer is used: face gradient of the boundary cell).
    for (int lj = ty; lj < PH; lj += TY) {
        const int j = j0 - 2 + lj;
        const bool yi = yin(j);
        for (int li = tx; li < PW; li += TX) {
            const int i = i0 - 2 + li;
            const bool xi = xin(i);
            double val = 0.0;
            if (xi && yi) val = phi[cidx(v, wrapx(i), wrapy(j))];
            else if (yi && (i == -1 || i == v.nx)) {
                int ic = i < 0 ? 0 : v.nx - 1, idx = cidx(v, ic, wrapy(j));
                double c = phi[idx];
                val = i < 0 ? phiW(v, phi, idx, ic, c, false) : phiE(v, phi, idx, ic, c, false);
            } else if (xi && (j == -1 || j == v.ny)) {
                int jc = j < 0 ? 0 : v.ny - 1, idx = cidx(v, wrapx(i), jc);
                double c = phi[idx];
                val = j < 0 ? phiS(v, phi, idx, jc, c, false) : phiN(v, phi, idx, jc, c, false);
            }
            sphi[lj * PW + li] = val;
        }
    }
    // ---- B and mask on the Re range (stored ghosts included: caller data, src/AmrHydro.cpp:686-701)
    const int i = i0 - 1 + tx;
    const bool xi = xin(i);
    double Br[NK];
    bool hasB[NK];
    bool neg = false, small = false;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int lj = ty + TY * k, j = j0 - 1 + lj;
        hasB[k] = INTERIOR || (i >= -1 && i <= v.nx && j >= -v.gy && j <= v.ny + v.gy - 1 && !((i < 0 || i >= v.nx) && (j < 0 || j >= v.ny)));
        double b = 0.0, m = 0.0;
        if (hasB[k]) { int idx = cidx(v, i, j); b = Bf[idx]; if (MASKED) m = mk[idx]; }
        if (MASKED) {
            neg = neg || (m < 0.0 && i >= 0 && i < v.nx && j >= 0 && j < v.ny);      // (no branch here: the loads of the unrolled rows stay batched)
            small = small || (hasB[k] && m < 1e-6 && j >= -1 && j <= v.ny);      // (rows beyond a physical side's ghost row are loaded, never used)
        }
        Br[k] = b;
        sB[lj * RW + tx] = b;
        if (MASKED) sM[lj * RW + tx] = m;
    }
    // this pass sees the ice mask of every cell of the level anyway: it leaves word whether any is negative, so that the relaxation
    // launches of the same V-cycle may skip reading the array (suhmo_gsrb.hip; COMPUTENONLINEARTERMS only asks mask < 0) ...
    if (MASKED && negflag && neg) *negflag = epoch;
    // ... and, when the host asks (the first launch after a write to the mask), whether anything it loaded -- ghost ring included: the
    // gradient's mask tests read no other cells -- is below the 1e-6 of those tests: if not, later launches leave the mask out
    if (MASKED && smallflag && small) *smallflag = 1u;
    __syncthreads();
    // cell-centred gradient of the cell at phi-tile position p (k_gradcc); (gi, gj) = its indices
    auto gradcc = [&](int p, int gi, int gj, double &gx, double &gy) {
        double c = sphi[p], w = sphi[p - 1], e = sphi[p + 1], s = sphi[p - PW], n = sphi[p + PW];
        bool zW = false, zE = false, zS = false, zN = false;
        if (hasMask) {
            int idx = cidx(v, wrapx(gi), wrapy(gj));
            bool mc = mk[idx] < 1e-6;
            zW = mc || mk[idx - 1] < 1e-6;
            zE = mc || mk[idx + 1] < 1e-6;
            zS = mc || mk[idx - v.P] < 1e-6;
            zN = mc || mk[idx + v.P] < 1e-6;
        }
        gradcc_from(v, c, w, e, s, n, zW, zE, zS, zN, gx, gy);
    };
    double rer[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int lj = ty + TY * k, j = j0 - 1 + lj;
        const bool yi = yin(j);
        const int p = (lj + 1) * PW + (tx + 1);
        double gx = 0.0, gy = 0.0;
        if (xi && yi) {
            gradcc(p, i, j, gx, gy);
        } else if (xi != yi) {
            // first ghost layer on a non-periodic domain side: linear extrapolation of the two
            // interior neighbours' gradients (k_grad_ghosts, util/ExtrapBCF.ChF:21-29)
            int d = 0, di = 0, dj = 0;
            if (!xi && (i == -1 || i == v.nx)) { di = i < 0 ? 1 : -1; d = di; }
            else if (!yi && (j == -1 || j == v.ny)) { dj = j < 0 ? 1 : -1; d = dj * PW; }
            if (d != 0) {
                double g1x, g1y, g2x, g2y;
                gradcc(p + d, i + di, j + dj, g1x, g1y);
                gradcc(p + 2 * d, i + 2 * di, j + 2 * dj, g2x, g2y);
                gx = 2.0 * g1x - g2x; gy = 2.0 * g1y - g2y;
            }
        }
        // Re on the (ghosted) range (k_re)
        double re = 0.0;
        if (hasB[k]) {
            re = re_from(ph, grad_norm(gx, gy), Br[k]);
        }
        rer[k] = re;
    }
    __syncthreads();                                 // every lane is done reading the phi tile
#pragma unroll
    for (int k = 0; k < NK; k++) sre[(ty + TY * k) * RW + tx] = rer[k];
    __syncthreads();
    // ---- faces (k_bcoef_faces): lane tx >= 1 owns cell column i (its W and S faces); the last tile
    // column / row also owns the domain's E / N faces
    const int nxt = (!INTERIOR && i0 + BT_X >= v.nx) ? v.nx - i0 + 1 : BT_X, nyt = (!INTERIOR && j0 + BT_Y >= v.ny) ? v.ny - j0 + 1 : BT_Y;
    const int fx = tx - 1;                           // face column index inside the tile
    if (fx >= 0 && fx < nxt) {
        for (int fy = ty; fy < nyt; fy += TY) {
            const int j = j0 + fy, idx = cidx(v, i, j), r = (fy + 1) * RW + tx;
            if (INTERIOR || j < v.ny)
                bxo[idx] = bcoef_face(ph, sre[r], sre[r - 1], sB[r], sB[r - 1], MASKED ? sM[r] : 1.0, MASKED ? sM[r - 1] : 1.0, !INTERIOR && (i == 0 || i == v.nx));
            if (INTERIOR || i < v.nx) {
                int jg = j + v.j0;
                byo[idx] = bcoef_face(ph, sre[r], sre[r - RW], sB[r], sB[r - RW], MASKED ? sM[r] : 1.0, MASKED ? sM[r - RW] : 1.0, !INTERIOR && (jg == 0 || jg == v.nyg));
            }
        }
    }
}
// rank strip: the relaxation also reads the ice mask of its halo rows (the neighbours' cells, on every depth that streams); k_bcoef_fused
// reports on the strip's own cells, this one on the stored halo rows of the depths [0, nd)
struct MaskHalo { const double *m[SUHMO_MAXDEPTH]; int nx[SUHMO_MAXDEPTH], ny[SUHMO_MAXDEPTH], P[SUHMO_MAXDEPTH], gy[SUHMO_MAXDEPTH]; int nd, lo, hi; };
// (smallflag: the scan, bcoef_tile.  At depth 0 it asks what k_bcoef_fused's gradient asks, `< 1e-6`, of the two halo rows that reads and of the two
// ghost columns of the FIRST halo row of either side -- the only halo row whose Re enters a face, so the only one whose end cells' gradient
// tests them; they are caller data, set with the ghosted field.  The deeper halo rows and the coarse depths only the relaxation reads: `< 0`)
__global__ __launch_bounds__(256) void k_mask_halo_report(MaskHalo h, unsigned *negflag, unsigned epoch, unsigned *smallflag)
{
    const int d = blockIdx.z, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= h.nd || i >= h.nx[d]) return;
    const int g = h.gy[d];
    bool neg = false, small = false;
    for (int r = blockIdx.y; r < 2 * g; r += gridDim.y) {
        const bool top = r >= g;
        if (top ? !h.hi : !h.lo) continue;
        const int j = top ? h.ny[d] + (r - g) : -1 - r;
        const double *__restrict__ row = h.m[d] + (long)(j + g) * h.P[d] + SUHMO_XOFF;
        const double m = row[i];
        neg = neg || m < 0.0;
        const int dist = top ? r - g : r;      // 0: the halo row next to the strip
        small = small || ((d == 0 && dist < 2) ? m < 1e-6 : m < 0.0);
        if (smallflag && d == 0 && i == 0 && (j == -1 || j == h.ny[d])) small = small || row[-1] < 1e-6 || row[h.nx[d]] < 1e-6;
    }
    if (negflag && neg) *negflag = epoch;
    if (smallflag && small) *smallflag = 1u;
}
template <int BT_X, int BT_Y, bool MASKED>
__device__ __forceinline__ void d_bcoef_fused(const DV &v, const FP &fp, const suhmo_phys_t &ph, int hasMask, unsigned *negflag, unsigned epoch, unsigned *smallflag)
{
    __shared__ double sphi[(BT_X + 4) * (BT_Y + 4)], sB[(BT_X + 2) * (BT_Y + 2)], sM[MASKED ? (BT_X + 2) * (BT_Y + 2) : 1];
    const int i0 = blockIdx.x * BT_X, j0 = blockIdx.y * BT_Y;
    const bool interior = i0 - 2 >= 0 && i0 + BT_X + 1 <= v.nx - 1 && j0 - 2 >= 0 && j0 + BT_Y + 1 <= v.ny - 1;
    if (interior) bcoef_tile<true, BT_X, BT_Y, MASKED>(v, fp, ph, hasMask, sphi, sB, sM, negflag, epoch, smallflag);
    else bcoef_tile<false, BT_X, BT_Y, MASKED>(v, fp, ph, hasMask, sphi, sB, sM, negflag, epoch, smallflag);
}
template <class T, int BT_X, int BT_Y, bool MASKED = true>
__global__ __launch_bounds__(256) void k_bcoef_fused(T t, unsigned *negflag, unsigned epoch, unsigned *smallflag)
{
    const suhmo_phys_t ph = t.phys();
    if (std::is_same<T, OnMembers>::value) { negflag = nullptr; epoch = 0u; smallflag = nullptr; }      // an ensemble's relaxation always reads the ice mask: nobody takes a report
    d_bcoef_fused<BT_X, BT_Y, MASKED>(t.view(), t.fields(), ph, ph.use_mask_gradients, negflag, epoch, smallflag);
}
// tiles of 62 x 14 cells on 64 x 4 threads; wide (an A/B option of large single levels): 126 x 14 on 128 x 2.  flag: the report on the ice
// mask, or NULL (an ensemble: its relaxation always reads the mask).  The last tile column / row also owns the E / N faces
// small: the word of the scan for values below 1e-6, or NULL; unmasked (whole levels whose mask is known clean): the instantiation without the mask
template <class T> int launch_bcoef_fused(const T &t, bool wide, unsigned *flag, unsigned epoch, hipStream_t st, unsigned *small, bool unmasked)
{
    if constexpr (std::is_same<T, OnLevel>::value) {
        const dim3 gw((t.nx() + 125) / 126, (t.ny() + 13) / 14), gn((t.nx() + 61) / 62, (t.ny() + 13) / 14);
        unsigned *const none = nullptr;
        if (unmasked && wide) return launch_grid(k_bcoef_fused<T, 126, 14, false>, t, gw, dim3(128, 2), st, none, 0u, none);
        if (unmasked) return launch_grid(k_bcoef_fused<T, 62, 14, false>, t, gn, dim3(64, 4), st, none, 0u, none);
        if (wide) return launch_grid(k_bcoef_fused<T, 126, 14>, t, gw, dim3(128, 2), st, flag, epoch, small);
    }
    return launch_grid(k_bcoef_fused<T, 62, 14>, t, dim3((t.nx() + 61) / 62, (t.ny() + 13) / 14), dim3(64, 4), st, flag, epoch, small);
}
template int launch_bcoef_fused(const OnMembers &, bool, unsigned *, unsigned, hipStream_t, unsigned *, bool);
// the answer of a scan, if it has arrived (an event query: never a wait); a scan of a mask that has been written since is forgotten
void suhmo_mask_poll(suhmo_level *L)
{
    if (!L->mask_scan_pending) return;
    const hipError_t e = hipEventQuery(L->mask_ev);
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return; }
    L->mask_scan_pending = 0;
    // a query that fails for good (the event was recorded into a stream some caller is capturing, say): that scan has no answer; the state
    // stays unknown and a later cycle scans again, three times at the most
    if (e != hipSuccess) { (void)hipGetLastError(); L->mask_scan_errors++; return; }
    if (L->mask_scan_version == L->mask_version) L->mask_state = *(volatile unsigned *)L->mask_host ? SUHMO_MASK_DIRTY : SUHMO_MASK_CLEAN;
}
int suhmo_mask_scan_begin(suhmo_level *L, hipStream_t st)
{
    if (!L->mask_ev) HIPCHK(hipEventCreateWithFlags(&L->mask_ev, hipEventDisableTiming));
    HIPCHK(hipMemsetAsync(suhmo_mask_scan_word(L), 0, sizeof(unsigned), st));
    return 0;
}
int suhmo_mask_scan_end(suhmo_level *L, hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(L->mask_host, suhmo_mask_scan_word(L), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(L->mask_ev, st));
    L->mask_scan_pending = 1; L->mask_scan_version = L->mask_version; L->mask_scans++;
    return 0;
}
template <class T> int launch_re(const T &t, hipStream_t st) { return launch_over(k_re<T>, t, GHOSTED, st); }      // COMPUTERE on the ghosted box
template <class T> int launch_bcoef_faces(const T &t, hipStream_t st) { return launch_over(k_bcoef_faces<T>, t, FACES, st); }
template <class T> int launch_grad_cc(const T &t, hipStream_t st)      // the gradient and its ghosts (a level exchanges in between: suhmo_grad_cc)
{
    int rc = launch_over(k_gradcc<T>, t, CELLS, st);
    return rc ? rc : launch_over(k_grad_ghosts<T>, t, PERIMETER, st);
}
template int launch_re(const OnLevel &, hipStream_t);
template int launch_re(const OnBoxes &, hipStream_t);
template int launch_re(const OnMembers &, hipStream_t);
template int launch_bcoef_faces(const OnLevel &, hipStream_t);
template int launch_bcoef_faces(const OnBoxes &, hipStream_t);
template int launch_bcoef_faces(const OnMembers &, hipStream_t);
template int launch_grad_cc(const OnMembers &, hipStream_t);

// fused single-kernel path: needs >= 3 cells per direction (extrapolation sources inside every
// edge tile) and, on rank boundaries, 2 exchanged phi rows for the halo-row gradient
static bool bcoef_is_fused(const suhmo_level *L, int depth)
{
    const Depth &D = L->d[depth];
    return L->bcoef_fused && D.v.nx >= 4 && D.v.ny >= 4 && (!(D.v.ext[0] || D.v.ext[1]) || (D.v.gy >= 2 && D.v.ny >= 2))
           && L->desc.nx_global == 0;      // AMR patches: un-fused kernels (coarse-fine ghosts are stored data)
}
// the next UpdateOperator of depth 0 would scan the ice mask (suhmo_common.h)
bool suhmo_mask_would_scan(const suhmo_level *L)
{
    return L->mask_known && !L->mask_view && L->mask_scan_errors < 3 && L->mask_state == SUHMO_MASK_UNKNOWN && !L->mask_scan_pending && L->mask_host
           && !L->mask_capturing && bcoef_is_fused(L, 0);
}
extern "C" int suhmo_level_update_operator(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::UpdateOperator");
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    Depth &D = L->d[depth];
    const bool fused = bcoef_is_fused(L, depth);
    int rc = suhmo_ensure_phi_halo(L, depth, fused ? 2 : 1, st); if (rc) return rc;
    if (fused) {
        const bool wide = L->bcoef_tile_x == 126 && D.v.nx >= 256;
        // depth 0 of a whole level: the kernel also reports (device word = this call's number) whether the ice mask has a negative cell
        // (the V-cycle that called takes the report up, suhmo_fas.hip: it holds until that cycle ends, not across calls of this entry point)
        unsigned *flag = nullptr;
        if (depth == 0) { L->maskflag_epoch = 0; L->mask_reported = 0; }
        // what is known about the mask across calls (suhmo_common.h): clean -> the kernel without it; unknown, nothing in flight, not inside a
        // graph capture -> this launch scans: a second word (the other half of the report's double) is cleared, set by any workgroup that
        // loads a value below 1e-6, copied to pinned memory behind the launch; an event marks the copy
        if (depth == 0 && !L->mask_capturing) suhmo_mask_poll(L);
        const bool unmasked = depth == 0 && suhmo_mask_clean(L, 0);
        unsigned *small = nullptr;
        const bool scan = depth == 0 && suhmo_mask_would_scan(L);
        if (scan) { small = suhmo_mask_scan_word(L); if ((rc = suhmo_mask_scan_begin(L, st))) return rc; }
        // inside a graph capture the masked kernels get the word too: the launch of the graph can then carry a scan, with the clear, the
        // copy and the event around it (suhmo_fas.hip)
        if (depth == 0 && L->mask_capturing && L->mask_known && !L->mask_view && !unmasked && L->mask_host) { small = suhmo_mask_scan_word(L); L->mask_scan_captured = 1; }
        if (depth == 0 && L->skip_mask && !unmasked) {
            flag = suhmo_mask_report_word(L);
            if (++L->mask_epoch == 0) L->mask_epoch = 1;
            L->mask_reported = 1;
        }
        if ((rc = launch_bcoef_fused(on_level(L, depth), wide, flag, L->mask_epoch, st, small, unmasked))) return rc;
        if (unmasked) L->bcoef_unmasked++;
        if ((flag || small) && (D.v.ext[0] || D.v.ext[1])) {
            MaskHalo h;
            h.nd = 0; h.lo = D.v.ext[0]; h.hi = D.v.ext[1];
            const int last = L->coarse_mask_ok ? (L->agg ? L->agg_depth : L->ndepth) : 1;      // (agglomerated depths keep no halo rows)
            int gmax = 1;
            for (int k = 0; k < last && k < SUHMO_MAXDEPTH; k++) {
                const Depth &Dk = L->d[k];
                h.m[k] = Dk.fp.f[SUHMO_F_MASK]; h.nx[k] = Dk.v.nx; h.ny[k] = Dk.v.ny; h.P[k] = Dk.v.P; h.gy[k] = Dk.v.gy;
                if (Dk.v.gy > gmax) gmax = Dk.v.gy;
                h.nd = k + 1;
            }
            hipLaunchKernelGGL(k_mask_halo_report, dim3((D.v.nx + 255) / 256, 2 * gmax, h.nd), dim3(256), 0, st, h, flag, L->mask_epoch, small);
        }
        if (scan && (rc = suhmo_mask_scan_end(L, st))) return rc;
    } else {
        if (depth == 0) { L->maskflag_epoch = 0; L->mask_reported = 0; }
        if (!suhmo_field(L, depth, SUHMO_F_GRADX) || !suhmo_field(L, depth, SUHMO_F_GRADY) || !suhmo_field(L, depth, SUHMO_F_RE)) return -2;
        const OnLevel t = on_level(L, depth);
        if ((rc = launch_over(k_gradcc<OnLevel>, t, CELLS, st))) return rc;
        rc = suhmo_exchange_fields(L, depth, {SUHMO_F_GRADX, SUHMO_F_GRADY}, st); if (rc) return rc;
        if ((rc = launch_over(k_grad_ghosts<OnLevel>, t, PERIMETER, st)) || (rc = launch_re(t, st)) || (rc = launch_bcoef_faces(t, st))) return rc;
    }
    HIPCHK(hipGetLastError());
    if (depth == 0) suhmo_faces_made(L);
    // strips: the fused relaxation recomputes halo rows, so it needs the coefficients there too (faces_deferred: the V-cycle sends them
    // with the coarse depths' faces, one message for all depths: suhmo_average_operator_all)
    if (depth == 0 && L->faces_deferred) return 0;
    rc = suhmo_exchange_fields(L, depth, {SUHMO_F_BX, SUHMO_F_BY}, st); if (rc) return rc;
    return 0;
}

// pieces of the un-fused WFlx_level for the AMR fine level (suhmo_amr.hip): cell-centred gradient with its
// domain-side ghosts; then (after the coarse-fine ghosts were interpolated) Re and bCoef
int suhmo_grad_cc(suhmo_level *L, int depth, hipStream_t st)
{
    if (!suhmo_field(L, depth, SUHMO_F_GRADX) || !suhmo_field(L, depth, SUHMO_F_GRADY) || !suhmo_field(L, depth, SUHMO_F_RE)) return -2;
    int rc = suhmo_ensure_phi_halo(L, depth, 1, st); if (rc) return rc;
    if ((rc = launch_over(k_gradcc<OnLevel>, on_level(L, depth), CELLS, st))) return rc;
    rc = suhmo_exchange_fields(L, depth, {SUHMO_F_GRADX, SUHMO_F_GRADY}, st); if (rc) return rc;    // lvlgradH.exchange() :1490
    return launch_over(k_grad_ghosts<OnLevel>, on_level(L, depth), PERIMETER, st);
}
// GRADX / GRADY at the listed cells only (device list of (i, j)); nothing else of the two fields is touched
int suhmo_grad_cc_list(suhmo_level *L, int depth, const int2 *d_cells, int n, hipStream_t st)
{
    Depth &D = L->d[depth];
    if (!suhmo_field(L, depth, SUHMO_F_GRADX) || !suhmo_field(L, depth, SUHMO_F_GRADY) || !suhmo_field(L, depth, SUHMO_F_RE)) return -2;
    int rc = suhmo_ensure_phi_halo(L, depth, 1, st); if (rc) return rc;
    if (n) hipLaunchKernelGGL(k_gradcc_list, dim3((n + 255) / 256), dim3(256), 0, st, D.v, D.fp, L->ph.use_mask_gradients, d_cells, n);
    HIPCHK(hipGetLastError());
    return 0;
}
int suhmo_re_bcoef_unfused(suhmo_level *L, int depth, hipStream_t st)
{
    int rc = launch_re(on_level(L, depth), st);
    if (depth == 0) suhmo_faces_made(L);
    return rc ? rc : launch_bcoef_faces(on_level(L, depth), st);
}
// grad h (cell centred, extrapolated ghosts) and Re on the ghosted level, for the time step
// (suhmo_step.hip): the un-fused steps 1-3 above
int suhmo_grad_re(suhmo_level *L, int depth, hipStream_t st)
{
    int rc = suhmo_grad_cc(L, depth, st);                           // rank strips: phi halo row + exchange of the gradient
    return rc ? rc : launch_re(on_level(L, depth), st);
}

// AverageOperator: CoarseAverageFace(bCoef[0] -> bCoef[depth], ratio r = 2^depth), sequential
// sum of the r collinear fine faces divided by r  (src/VCAMRNonLinearPoissonOp.cpp:66-95)
__device__ __forceinline__ void d_average_faces(const DV &vf, const double *__restrict__ bxf, const double *__restrict__ byf,
                                                const DV &vc, double *__restrict__ bxc, double *__restrict__ byc, int r)
{
    int ic = blockIdx.x * blockDim.x + threadIdx.x, jc = blockIdx.y * blockDim.y + threadIdx.y;
    if (ic > vc.nx || jc > vc.ny) return;
    if (jc < vc.ny) {
        double sm = 0.0;
        int base = cidx(vf, ic * r, jc * r);
        for (int k = 0; k < r; k++) sm = sm + bxf[base + k * vf.P];
        bxc[cidx(vc, ic, jc)] = sm / (double)r;
    }
    if (ic < vc.nx) {
        double sm = 0.0;
        int base = cidx(vf, ic * r, jc * r);
        for (int k = 0; k < r; k++) sm = sm + byf[base + k];
        byc[cidx(vc, ic, jc)] = sm / (double)r;
    }
}
template <class T> __global__ void k_average_faces(T c, T f, int r)      // (faces: no second canvas)
{
    const FP &ff = f.fields(), &fc = c.fields();
    d_average_faces(f.view(), ff.f[SUHMO_F_BX], ff.f[SUHMO_F_BY], c.view(), fc.f[SUHMO_F_BX], fc.f[SUHMO_F_BY], r);
}
// All depths of AverageOperator in ONE pass over the depth-0 faces (the V-cycle refreshes every
// depth right after UpdateOperator).  The reference's arithmetic is a sequential sum of the
// r = 2^d collinear fine faces divided by r; the running sum of the first r/2 faces of a group IS
// the (unscaled) depth d-1 sum, so one walk over 2^(nd-1) faces yields every depth bit for bit.
struct AvgOut { double *bx[SUHMO_MAXDEPTH], *by[SUHMO_MAXDEPTH]; int P[SUHMO_MAXDEPTH]; int gy[SUHMO_MAXDEPTH]; };
#define AVG_ALL_MAXDEPTH 7     // depths one pass serves (avg_faces_one_pass): a block of 2^(nd-1) rows per thread of the x-face walker
// x-faces: thread = (even fine column i, block of R = 2^(nd-1) rows); walks the rows.  U: loads a thread keeps in flight (8; 4 on a level,
// whose launch has to fit beside another kernel's waves: suhmo_average_operator_all) -- the sums and their order do not depend on it
template <int U>
__device__ __forceinline__ void d_average_faces_x_all(const DV &vf, const double *__restrict__ bxf, const AvgOut &o, int nd, int bix, int biy, int tx, int ty)
{
    const int R = 1 << (nd - 1);
    int ih = bix * 64 + tx;                              // i = 2 * ih
    int jb = biy * 4 + ty;
    int i = 2 * ih;
    if (i > vf.nx || jb * R >= vf.ny) return;
    double sum[AVG_ALL_MAXDEPTH];
    const int base = cidx(vf, i, jb * R);
    auto take = [&](int k, double f) {
#pragma unroll
        for (int d = 1; d < AVG_ALL_MAXDEPTH; d++) {     // (unrolled: one running sum per depth the pass can have, not per depth a level can)
            if (d >= nd) break;
            const int r = 1 << d;
            if ((i & (r - 1)) != 0) break;               // column not on depth d's face grid (nor deeper)
            sum[d] = ((k & (r - 1)) == 0) ? 0.0 + f : sum[d] + f;
            if ((k & (r - 1)) == r - 1)
                o.bx[d][((jb * R + k) / r + o.gy[d]) * o.P[d] + SUHMO_XOFF + i / r] = sum[d] / (double)r;
        }
    };
    if (R >= 8) {
        for (int k0 = 0; k0 < R; k0 += U) {              // U independent loads in flight, then the (sequential) sums
            double fu[U];
#pragma unroll
            for (int u = 0; u < U; u++) fu[u] = bxf[base + (k0 + u) * vf.P];
#pragma unroll
            for (int u = 0; u < U; u++) take(k0 + u, fu[u]);
        }
    } else {
        for (int k = 0; k < R; k++) take(k, bxf[base + k * vf.P]);
    }
}
// y-faces: one wave walks 64 consecutive columns of YR even fine rows (their loads in flight together); lane l = column
template <int YR>
__device__ __forceinline__ void d_average_faces_y_all(const DV &vf, const double *__restrict__ byf, const AvgOut &o, int nd, int bix, int biy, int tid)
{
    const int lane = tid & 63;
    const int i = bix * 64 + lane;
    const int jb = 2 * YR * (biy * 4 + (tid >> 6));
    if (jb > vf.ny) return;                               // whole wave leaves together
    double fr[YR];
#pragma unroll
    for (int q = 0; q < YR; q++) {
        const int j = jb + 2 * q;
        fr[q] = (i < vf.nx && j <= vf.ny) ? byf[cidx(vf, i, j)] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < YR; q++) {
        const int j = jb + 2 * q;
        if (j > vf.ny) break;                            // uniform
        const double f = fr[q];
        double run = 0.0 + f;                             // depth-0 "sum" of a single face
        for (int d = 1; d < nd; d++) {
            const int r = 1 << d;
            if ((j & (r - 1)) != 0) break;                // row not on depth d's face grid
            // sequential continuation: (((run + f[l + r/2]) + f[l + r/2 + 1]) + ... + f[l + r - 1])
            double acc = run;
            for (int k = r / 2; k < r; k++) acc = acc + __shfl(f, (lane + k) & 63);
            run = acc;                                    // valid on lanes with (lane % r) == 0
            if ((lane & (r - 1)) == 0 && i < vf.nx)
                o.by[d][(j / r + o.gy[d]) * o.P[d] + SUHMO_XOFF + i / r] = run / (double)r;
        }
    }
}

// both directions in ONE launch of 256-thread workgroups: the first gxx * gxy of them are the x-face walkers (64 x 4 threads), the rest the
// y-face walkers (four waves): nothing of one reads what the other writes
template <int U>
__device__ __forceinline__ void d_average_faces_all(const DV &vf, const double *__restrict__ bxf, const double *__restrict__ byf, const AvgOut &o, int nd, int gxx, int gxy, int gyx)
{
    const int b = blockIdx.x, nbx = gxx * gxy;
    if (b < nbx) d_average_faces_x_all<U>(vf, bxf, o, nd, b % gxx, b / gxx, threadIdx.x & 63, threadIdx.x >> 6);
    else d_average_faces_y_all<U>(vf, byf, o, nd, (b - nbx) % gyx, (b - nbx) / gyx, threadIdx.x);
}
// the pointers of all depths beside the target (`A`): by value for a level, a device row per member of an ensemble (row_of)
struct AvgAll;
struct BatchAvg;
__device__ __forceinline__ const AvgOut &avg_out(const AvgOut &o) { return o; }
__device__ __forceinline__ const AvgOut &avg_out(const BatchAvg &b);
__device__ __forceinline__ const AvgAll &avg_all(const AvgAll &a) { return a; }
__device__ __forceinline__ const AvgAll &avg_all(const BatchAvg &b);
template <class T, class A, int U>
__global__ __launch_bounds__(256) void k_average_faces_all(T t, A av, int nd, int gxx, int gxy, int gyx)
{
    const FP &fp = t.fields();
    d_average_faces_all<U>(t.view(), fp.f[SUHMO_F_BX], fp.f[SUHMO_F_BY], avg_out(row_of(t, av)), nd, gxx, gxy, gyx);
}

template <class T> int launch_average_faces(const T &f, const T &c, int r, hipStream_t st) { return launch_over(k_average_faces<T>, c, FACES, st, f, r); }
extern "C" int suhmo_level_average_operator(suhmo_level_t *L, int depth, suhmo_stream_t s)
{
    SUHMO_TIME("VCAMRNonLinearPoissonOp::AverageOperator");
    ARG(L); ARG(depth >= 0 && depth < L->ndepth);
    if (depth == 0) return 0;
    HIPCHK(hipSetDevice(L->device));
    int rc = launch_average_faces(on_level(L, 0), on_level(L, depth), 1 << depth, (hipStream_t)s);
    return rc ? rc : suhmo_exchange_fields(L, depth, {SUHMO_F_BX, SUHMO_F_BY}, (hipStream_t)s);
}

static void fill_avg_out(const suhmo_level *L, int nd, AvgOut &o)
{
    for (int d = 0; d < nd; d++) { o.bx[d] = L->d[d].fp.f[SUHMO_F_BX]; o.by[d] = L->d[d].fp.f[SUHMO_F_BY]; o.P[d] = L->d[d].v.P; o.gy[d] = L->d[d].v.gy; }
}
#define AVG_U_BATCH 8     // loads in flight per thread of k_average_faces_all: an ensemble's launch ...
#define AVG_U_LEVEL 4     // ... and a level's, which at 36 VGPRs fits the 48 that two waves of the restricting relaxation leave on a SIMD
static void avg_faces_grids(const DV &v, int nd, int U, dim3 &gx, dim3 &gy)      // workgroups of the x-face and of the y-face walkers
{
    const int R = 1 << (nd - 1);
    gx = dim3((v.nx / 2 + 1 + 63) / 64, (v.ny / R + 3) / 4);
    gy = dim3((v.nx + 63) / 64, ((v.ny / 2 + 1 + U - 1) / U + 3) / 4);
}
static bool avg_faces_one_pass(const DV &v, int nd) { return !(nd > AVG_ALL_MAXDEPTH || v.nx % (1 << (nd - 1)) || v.ny % (1 << (nd - 1))); }
int suhmo_average_operator_all(suhmo_level *L, int nd, hipStream_t st)
{
    Depth &F = L->d[0];
    const bool d0 = L->faces_deferred != 0;          // the halo rows of the depth-0 faces are still to travel
    L->faces_deferred = 0;
    if (nd < 2) return d0 ? suhmo_exchange_fields(L, 0, {SUHMO_F_BX, SUHMO_F_BY}, st) : 0;
    if (!avg_faces_one_pass(F.v, nd)) {     // generic fallback
        if (d0) { int rc = suhmo_exchange_fields(L, 0, {SUHMO_F_BX, SUHMO_F_BY}, st); if (rc) return rc; }
        for (int k = 1; k < nd; k++) { int rc = suhmo_level_average_operator(L, k, (suhmo_stream_t)st); if (rc) return rc; }
        return suhmo_agg_gather_faces(L, nd, st);
    }
    AvgOut o;
    fill_avg_out(L, nd, o);
    dim3 gx, gy;
    avg_faces_grids(F.v, nd, AVG_U_LEVEL, gx, gy);
    { int rc = launch_grid(k_average_faces_all<OnLevel, AvgOut, AVG_U_LEVEL>, on_level(L, 0), dim3(gx.x * gx.y + gy.x * gy.y), dim3(256), st, o, nd, (int)gx.x, (int)gx.y, (int)gy.x); if (rc) return rc; }
    // strips: the coarse face coefficients of all depths travel as one message group when the transport can batch
    if (L->ipc) { int rc = suhmo_ipc_batch(L, 1, st); if (rc) return rc; }
    else if (L->ex_begin && L->ex) { int rc = L->ex_begin(L->user); if (rc) return rc; }
    for (int k = d0 ? 0 : 1; k < nd && !(L->agg && k >= L->agg_depth); k++) {
        int rc = suhmo_exchange_fields(L, k, {SUHMO_F_BX, SUHMO_F_BY}, st); if (rc) return rc;
    }
    if (L->ipc) { int rc = suhmo_ipc_batch(L, 0, st); if (rc) return rc; }
    else if (L->ex_end && L->ex) { int rc = L->ex_end(L->user, L, (suhmo_stream_t)st); if (rc) return rc; }
    return suhmo_agg_gather_faces(L, nd, st);       // agglomerated depths: every rank's rows of the coarse faces -> the whole-level copy
}

// MGnewOp coefficient coarsening: CoarseAverage (arithmetic) of aCoef, B, Pi, zb, iceMask from
// depth 0 with ratio r: sequential sum (ii fastest) * 1/r^2 (src/VCAMRNonLinearPoissonOp.cpp:1116-1138)
// The five coefficient fields of every coarse depth in ONE launch (blockIdx.z = (depth - 1) * 5 + field): each depth averages
// depth 0 directly, so they are independent.  The sum of a coarse cell is one sequential chain of r*r additions whatever the
// kernel does, so at the deep depths (few coarse cells, r = 16, 32) the time is the chain plus the latency of its loads: a row
// of the block is fetched as r/2 independent 16-byte loads, then added in order.
struct AvgDepth { int nx, ny, P, gy; int boff, nbx; double *c[5]; };   // boff: first workgroup of the depth, nbx: its workgroups per row of tiles
struct AvgAll { const double *f[5]; AvgDepth d[SUHMO_MAXDEPTH - 1]; };
template <int R>
__device__ __forceinline__ double average_block(const double *__restrict__ f, int base, int P, int r_)
{
    const int r = R ? R : r_;
    double sm = 0.0;
    if constexpr (R >= 2) {
        for (int jj = 0; jj < R; jj++) {
            double2 row[R / 2];
#pragma unroll
            for (int k = 0; k < R / 2; k++) row[k] = *reinterpret_cast<const double2 *>(f + base + jj * P + 2 * k);   // ic * r is even
#pragma unroll
            for (int k = 0; k < R / 2; k++) { sm = sm + row[k].x; sm = sm + row[k].y; }
        }
    } else {
        for (int jj = 0; jj < r; jj++)
            for (int ii = 0; ii < r; ii++) sm = sm + f[base + jj * P + ii];
    }
    return sm * (1.0 / (double)(r * r));
}
__device__ __forceinline__ void d_average_cells_all(const DV &vf, const AvgAll &a, int nd)
{
    // workgroups are numbered depth by depth (a grid sized for the largest depth would dispatch mostly empty ones)
    int dep = 1;
    while (dep + 1 < nd && (int)blockIdx.x >= a.d[dep].boff) dep++;
    const AvgDepth &C = a.d[dep - 1];
    const int local = blockIdx.x - C.boff, q = local % 5, tile = local / 5;
    const int ic = (tile % C.nbx) * blockDim.x + threadIdx.x, jc = (tile / C.nbx) * blockDim.y + threadIdx.y;
    if (ic >= C.nx || jc >= C.ny) return;
    const double *__restrict__ f = a.f[q];
    const int r = 1 << dep, base = cidx(vf, ic * r, jc * r);
    double m;
    switch (r) {
    case 2: m = average_block<2>(f, base, vf.P, r); break;
    case 4: m = average_block<4>(f, base, vf.P, r); break;
    case 8: m = average_block<8>(f, base, vf.P, r); break;
    case 16: m = average_block<16>(f, base, vf.P, r); break;
    case 32: m = average_block<32>(f, base, vf.P, r); break;
    default: m = average_block<0>(f, base, vf.P, r); break;
    }
    C.c[q][(jc + C.gy) * C.P + SUHMO_XOFF + ic] = m;
}
template <class T, class A> __global__ __launch_bounds__(256) void k_average_cells_all(T t, A av, int nd) { d_average_cells_all(t.view(), avg_all(row_of(t, av)), nd); }
// ghosts of coarse B / Pi / zb / mask: periodic wrap or Neumann copy (NeumBCForB :1309-1341)
__device__ __forceinline__ void d_coef_ghosts(const DV &v, double *__restrict__ p)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * v.ny) {
        int side = t / v.ny, j = t % v.ny;
        if (v.cfx[side]) return;
        if (side == 0) { int idx = cidx(v, 0, j); p[idx - 1] = v.per[0] ? p[idx + v.nx - 1] : p[idx]; }
        else { int idx = cidx(v, v.nx - 1, j); p[idx + 1] = v.per[0] ? p[idx - (v.nx - 1)] : p[idx]; }
        return;
    }
    t -= 2 * v.ny;
    if (t < 2 * v.nx) {
        int side = t / v.nx, i = t % v.nx;
        if (v.ext[side]) return;
        if (side == 0) { int idx = cidx(v, i, 0); p[idx - v.P] = v.per[1] ? p[idx + (v.ny - 1) * v.P] : p[idx]; }
        else { int idx = cidx(v, i, v.ny - 1); p[idx + v.P] = v.per[1] ? p[idx - (v.ny - 1) * v.P] : p[idx]; }
    }
}
template <class T> __global__ void k_coef_ghosts(T t, int field) { d_coef_ghosts(t.view(), t.field(field)); }
__device__ __forceinline__ void d_coef_ghosts_all(const DV &v0, const AvgAll &a)        // B, Pi, zb, mask of every coarse depth (blockIdx.y = (depth - 1) * 4 + field - 1)
{
    const AvgDepth &C = a.d[blockIdx.y / 4];
    double *__restrict__ p = C.c[1 + blockIdx.y % 4];
    const int nx = C.nx, ny = C.ny, P = C.P;
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * ny) {
        int side = t / ny, j = t % ny;
        if (v0.cfx[side]) return;
        if (side == 0) { int idx = (j + C.gy) * P + SUHMO_XOFF; p[idx - 1] = v0.per[0] ? p[idx + nx - 1] : p[idx]; }
        else { int idx = (j + C.gy) * P + SUHMO_XOFF + nx - 1; p[idx + 1] = v0.per[0] ? p[idx - (nx - 1)] : p[idx]; }
        return;
    }
    t -= 2 * ny;
    if (t < 2 * nx) {
        int side = t / nx, i = t % nx;
        if (v0.ext[side]) return;
        if (side == 0) { int idx = C.gy * P + SUHMO_XOFF + i; p[idx - P] = v0.per[1] ? p[idx + (ny - 1) * P] : p[idx]; }
        else { int idx = (ny - 1 + C.gy) * P + SUHMO_XOFF + i; p[idx + P] = v0.per[1] ? p[idx - (ny - 1) * P] : p[idx]; }
    }
}
template <class T, class A> __global__ void k_coef_ghosts_all(T t, A av) { d_coef_ghosts_all(t.view(), avg_all(row_of(t, av))); }
// an ensemble: the member's pointers of all depths are a row of a device table written once
struct BatchAvg { AvgAll a; AvgOut o; };
__device__ __forceinline__ const AvgOut &avg_out(const BatchAvg &b) { return b.o; }
__device__ __forceinline__ const AvgAll &avg_all(const BatchAvg &b) { return b.a; }
typedef const BatchAvg *__restrict__ BatchAvgRows;      // (written once: a kernel's stores never change them)
template <class T> int launch_coef_ghosts(const T &t, int field, hipStream_t st) { return launch_over(k_coef_ghosts<T>, t, PERIMETER, st, field); }
template int launch_coef_ghosts(const OnBoxes &, int, hipStream_t);
template int launch_coef_ghosts(const OnMembers &, int, hipStream_t);
// exchange + CopyGhostCells of a cell field (util/ExtrapGhostCells.cpp:182-269)
int suhmo_copy_ghosts(suhmo_level *L, int depth, int field, hipStream_t st)
{
    if (!suhmo_field(L, depth, field)) return -2;
    return launch_coef_ghosts(on_level(L, depth), field, st);
}
static int fill_avg_all(const suhmo_level *L, AvgAll &a)      // returns the workgroups of k_average_cells_all
{
    static const int fields[5] = {SUHMO_F_ACOEF, SUHMO_F_B, SUHMO_F_PI, SUHMO_F_ZB, SUHMO_F_MASK};
    int nblocks = 0;
    for (int q = 0; q < 5; q++) a.f[q] = L->d[0].fp.f[fields[q]];
    for (int dep = 1; dep < L->ndepth; dep++) {
        const Depth &C = L->d[dep];
        AvgDepth &o = a.d[dep - 1];
        o.nx = C.v.nx; o.ny = C.v.ny; o.P = C.v.P; o.gy = C.v.gy;
        for (int q = 0; q < 5; q++) o.c[q] = C.fp.f[fields[q]];
        o.boff = nblocks; o.nbx = (C.v.nx + 63) / 64;
        nblocks += 5 * o.nbx * ((C.v.ny + 3) / 4);
    }
    return nblocks;
}
// MGnewOp's coefficient averages of every depth > 0 and their ghosts: two launches (v1: the view of depth 1, the largest ring)
template <class T, class A> static int launch_average_cells_all(const T &t, A av, int nblocks, const DV &v1, int nd, hipStream_t st)
{
    int rc = launch_grid(k_average_cells_all<T, A>, t, dim3(nblocks), BLK2D, st, av, nd);
    return rc ? rc : launch_grid(k_coef_ghosts_all<T, A>, t, dim3((2 * v1.ny + 2 * v1.nx + 255) / 256, 4 * (nd - 1)), dim3(256), st, av);
}
// with_faces = false: the caller's cycle re-averages bCoef itself (bcoeff_otf: UpdateOperator + AverageOperator every V-cycle)
int suhmo_build_mg_coefficients(suhmo_level *L, bool with_faces, hipStream_t st)
{
    const int nd = L->ndepth;
    if (nd > 1) {
        AvgAll a;
        const int nblocks = fill_avg_all(L, a);
        int rc = launch_average_cells_all(on_level(L, 0), a, nblocks, L->d[1].v, nd, st); if (rc) return rc;
    }
    for (int dep = 1; dep < nd; dep++) {
        int rc;
        if (with_faces && (rc = suhmo_level_average_operator(L, dep, (suhmo_stream_t)st))) return rc;
        if (L->agg && dep >= L->agg_depth) continue;                  // agglomerated depths: no halo rows, the whole rows travel below
        rc = suhmo_exchange_fields(L, dep, {SUHMO_F_ACOEF, SUHMO_F_B, SUHMO_F_PI, SUHMO_F_ZB, SUHMO_F_MASK}, st); if (rc) return rc;
    }
    // a rank strip's scan looked at the halo rows of the depths whose masks were depth 0's averages at the time: if the coarse ones only
    // become so now, it looks again
    if (!L->coarse_mask_ok && (L->d[0].v.ext[0] || L->d[0].v.ext[1])) suhmo_mask_halo_written(L);
    L->coarse_mask_ok = 1;
    if (nd > 1) suhmo_zb_written(L);        // (the coarse depths' bed elevations are new averages: each is scanned on its own, suhmo_common.h)
    return suhmo_agg_gather_static(L, with_faces, st);
}
extern "C" int suhmo_level_build_mg_coefficients(suhmo_level_t *L, suhmo_stream_t s)
{
    ARG(L);
    HIPCHK(hipSetDevice(L->device));
    return suhmo_build_mg_coefficients(L, true, (hipStream_t)s);
}

// ---- every box of a multi-box AMR level in one launch
int suhmo_multi_grad_cc(const suhmo_multi &m, hipStream_t st)
{
    return m.merged ? launch_over(k_gradcc_ghosts, m.on(), CELLS, st) : launch_grad_cc(m.on(), st);
}

int suhmo_levels_grad_cc(const suhmo_lvboxes &lv, int hasMask, hipStream_t st)
{
    int nz = 0;
    for (int q = 0; q < lv.n; q++) nz += lv.nbox[q];
    if (nz <= 0) return 0;
    hipLaunchKernelGGL(k_gradcc_ghosts_lv, dim3((lv.maxnx + 63) / 64, (lv.maxny + 3) / 4, nz), BLK2D, 0, st, lv, hasMask);
    HIPCHK(hipGetLastError());
    return 0;
}

int suhmo_multi_re_bcoef(const suhmo_multi &m, hipStream_t st)
{
    const OnBoxes t = m.on();
    if (m.merged) return launch_over(k_re_bcoef, t, GHOSTED, st);
    int rc = launch_re(t, st);
    return rc ? rc : launch_bcoef_faces(t, st);
}

// ------------------------------------------------------------------ an ensemble (suhmo_batch.hip)
// the members' pointers of all depths (coefficient and face canvases: they never trade places): n rows, written once
int suhmo_batch_avg_table(suhmo_level *const *mem, int n, void **dev)
{
    std::vector<BatchAvg> h(n);
    for (int k = 0; k < n; k++) { memset(&h[k], 0, sizeof(BatchAvg)); fill_avg_all(mem[k], h[k].a); fill_avg_out(mem[k], mem[k]->ndepth, h[k].o); }
    if (!*dev) HIPCHK(hipMalloc(dev, n * sizeof(BatchAvg)));
    HIPCHK(hipMemcpy(*dev, h.data(), n * sizeof(BatchAvg), hipMemcpyHostToDevice));
    return 0;
}
// AverageOperator of every depth > 0 in one pass over the depth-0 faces where the grid allows (*launches: how many it took); t[dep]: the
// members at every depth
int suhmo_batch_average_operator_all(const OnMembers *t, const void *avg, int nd, hipStream_t st, int *launches)
{
    *launches = 0;
    if (t[0].count() <= 0 || nd < 2) return 0;
    DV v{};
    v.nx = t[0].nx(); v.ny = t[0].ny();
    if (!avg_faces_one_pass(v, nd)) {
        for (int dep = 1; dep < nd; dep++) {
            int rc = launch_average_faces(t[0], t[dep], 1 << dep, st); if (rc) return rc;
            ++*launches;
        }
        return 0;
    }
    dim3 gx, gy;
    avg_faces_grids(v, nd, AVG_U_BATCH, gx, gy);
    *launches = 1;
    return launch_grid(k_average_faces_all<OnMembers, BatchAvgRows, AVG_U_BATCH>, t[0], dim3(gx.x * gx.y + gy.x * gy.y), dim3(256), st, (const BatchAvg *)avg, nd, (int)gx.x, (int)gx.y, (int)gy.x);
}
// MGnewOp's coefficient averages of every depth > 0 and their ghosts (suhmo_build_mg_coefficients without the faces): two launches
int suhmo_batch_build_mg_coefficients(const OnMembers &t0, const void *avg, const suhmo_level *L0, hipStream_t st, int *launches)
{
    *launches = 0;
    const int nd = L0->ndepth;
    if (t0.count() <= 0 || nd < 2) return 0;
    AvgAll a;
    const int nblocks = fill_avg_all(L0, a);                 // (the geometry: the members share it)
    *launches = 2;
    return launch_average_cells_all(t0, (BatchAvgRows)avg, nblocks, L0->d[1].v, nd, st);
}
