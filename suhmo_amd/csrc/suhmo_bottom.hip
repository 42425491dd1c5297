// suhmo_bottom.hip -- the bottom solver of the FAS V-cycle: Chombo's RelaxSolver, as the reference configures it for every head
// solve (src/AmrHydro.cpp:726,733-735) and the implicit gap solve (:623,628).  The fork's three-argument preCond
// (src/VCAMRNonLinearPoissonOp.cpp:233-271) makes each of its iterations relax(phi, rhs, 2):
//
//     residual(dep); norm = l2(RES); first = norm
//     for it in 0 .. 39 while norm > 1e-20:
//         gsrb(dep, 2); residual(dep); old = norm; norm = l2(RES)
//         if norm < 1e-6 * first or norm > old * (1.0 - 0.1): break
//
// Opt-in, level option bottom_solver = 1 (default 0: the cycle stops after its numBottom relaxes, as before).  Two paths:
//   k_relax_solve   the whole loop in ONE launch of one workgroup: phi of the bottom depth lives in LDS for the whole solve, the
//                   coefficients are read through L2, the l2 norm is a fixed-order reduction in LDS, the break test runs on the device.
//                   Whole-level depths of up to 128 x 128 cells (and up to bottom_one_launch_max_cells).  A fixed launch: the V-cycle
//                   stays capturable as a graph.  One __global__ template over the launch target (suhmo_target.h): OnLevel is that one
//                   workgroup; OnMembers (an ensemble created with bottom_solver=1, suhmo_batch.hip) is one workgroup per ACTIVE member in
//                   one launch, each with its own loop, break test and counters -- a member's iteration count and bits are those of the
//                   same level run alone, and no workgroup waits for another.  The LDS stays the static 128 KiB: a workgroup then has a CU
//                   to itself, and an ensemble has at most 64 members for the part's 256 CUs, so sizing it to the depth would buy no
//                   concurrency the launch lacks (nothing measured).
//   host loop      everything else (larger bottoms, rank strips whose bottom is not agglomerated, AMR patches): the same loop from
//                   the existing launches (suhmo_launch_gsrb, suhmo_level_residual, suhmo_level_norm) and one 8-byte read-back per
//                   iteration.  A level whose bottom takes it is not replayed as a graph (suhmo_fas.hip).
// Every update and every residual is the expression of k_gsrb_pass_simple / k_apply<., 1> on the same operands: the same bits.  Only
// the order of the l2 sum differs from the oracle's serial one (the tests' tolerance for l2 norms; only a near-tie at a break test
// could show it).
#include "suhmo_batch.h"
#include <cmath>

#define SUHMO_BOTTOM_NT 1024
#define SUHMO_BOTTOM_LDS_CELLS 16384      // 128 x 128 doubles: 128 KiB of the CU's 160

// phi of the neighbour in LDS (interior cells only, row-major nx x ny), the boundary condition evaluated from the adjacent
// interior value as phiW / phiE / phiS / phiN do it (homog = false; whole level: no stored ghost, no coarse-fine side)
__device__ __forceinline__ double lds_w(const DV &v, const double *p, int k, int i, double c)
{
    if (i > 0) return p[k - 1];
    if (v.per[0]) return p[k + v.nx - 1];
    if (v.bct[0][0] == 0) return v.two_v[0][0] - c;
    return c + v.neu[0][0];
}
__device__ __forceinline__ double lds_e(const DV &v, const double *p, int k, int i, double c)
{
    if (i < v.nx - 1) return p[k + 1];
    if (v.per[0]) return p[k - (v.nx - 1)];
    if (v.bct[0][1] == 0) return v.two_v[0][1] - c;
    return c + v.neu[0][1];
}
__device__ __forceinline__ double lds_s(const DV &v, const double *p, int k, int j, double c)
{
    if (j > 0) return p[k - v.nx];
    if (v.per[1]) return p[k + (v.ny - 1) * v.nx];
    if (v.bct[1][0] == 0) return v.two_v[1][0] - c;
    return c + v.neu[1][0];
}
__device__ __forceinline__ double lds_n(const DV &v, const double *p, int k, int j, double c)
{
    if (j < v.ny - 1) return p[k + v.nx];
    if (v.per[1]) return p[k - (v.ny - 1) * v.nx];
    if (v.bct[1][1] == 0) return v.two_v[1][1] - c;
    return c + v.neu[1][1];
}

// L(phi) of cell (i, j) from LDS; dnl and lambda for the relaxation when asked
template <bool HAS_ALPHA>
__device__ __forceinline__ double lds_lofphi(const DV &v, const FP &fp, const suhmo_phys_t &ph, const double *p, int i, int j, int idx,
                                             double &lam, double &dnl)
{
    const int k = j * v.nx + i;
    const double c = p[k];
    const double e = lds_e(v, p, k, i, c), w = lds_w(v, p, k, i, c);
    const double n = lds_n(v, p, k, j, c), s = lds_s(v, p, k, j, c);
    const double bxW = fp.f[SUHMO_F_BX][idx], bxE = fp.f[SUHMO_F_BX][idx + 1];
    const double byS = fp.f[SUHMO_F_BY][idx], byN = fp.f[SUHMO_F_BY][idx + v.P];
    double nl;
    nl_terms(ph, c, fp.f[SUHMO_F_B][idx], fp.f[SUHMO_F_PI][idx], fp.f[SUHMO_F_ZB][idx], fp.f[SUHMO_F_MASK][idx], nl, dnl);
    const double aterm = HAS_ALPHA ? v.alpha * fp.f[SUHMO_F_ACOEF][idx] : v.alpha;
    lam = lambda_cell(v, aterm, bxE, bxW, byN, byS);
    return lofphi_cell(v, aterm, c, e, w, n, s, bxE, bxW, byN, byS, nl);
}

// RES = rhs - L(phi) of every cell (stored), and the l2 norm of it: per thread in cell order, per wave by a fixed butterfly,
// over the waves in wave order (the same sum on every launch)
template <bool HAS_ALPHA>
__device__ double lds_residual_l2(const DV &v, const FP &fp, const suhmo_phys_t &ph, const double *p, double *wsum)
{
    const int ncell = v.nx * v.ny;
    double acc = 0.0;
    for (int k = threadIdx.x; k < ncell; k += SUHMO_BOTTOM_NT) {
        const int j = k / v.nx, i = k - j * v.nx, idx = cidx(v, i, j);
        double lam, dnl;
        const double lofphi = lds_lofphi<HAS_ALPHA>(v, fp, ph, p, i, j, idx, lam, dnl);
        const double res = fp.f[SUHMO_F_RHS][idx] - lofphi;
        fp.f[SUHMO_F_RES][idx] = res;
        acc += res * res;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < SUHMO_BOTTOM_NT / 64; w++) r += wsum[w];
    __syncthreads();                                   // (wsum is written again by the next call)
    return sqrt(r);
}

// RelaxSolver::solve of ONE whole depth by the workgroup that runs it: the loop state (norm, first, it) lives in that workgroup's registers,
// phi and the wave sums in its LDS, and nothing is synchronised beyond the workgroup.  ctr: iterations, solves of that depth's level
template <bool HAS_ALPHA>
__device__ __forceinline__ void d_relax_solve(const DV &v, const FP &fp, const suhmo_phys_t &ph, unsigned long long *__restrict__ ctr)
{
    __shared__ double p[SUHMO_BOTTOM_LDS_CELLS];
    __shared__ double wsum[SUHMO_BOTTOM_NT / 64];
    const int ncell = v.nx * v.ny, half = (v.nx + 1) / 2;
    double *__restrict__ phi = fp.f[SUHMO_F_PHI];
    for (int k = threadIdx.x; k < ncell; k += SUHMO_BOTTOM_NT) { const int j = k / v.nx, i = k - j * v.nx; p[k] = phi[cidx(v, i, j)]; }
    __syncthreads();
    double norm = lds_residual_l2<HAS_ALPHA>(v, fp, ph, p, wsum);
    const double first = norm;
    int it = 0;
    for (; it < 40 && norm > 1.0e-20; ) {
        for (int pass = 0; pass < 4; pass++) {                                 // two sweeps: red, black, red, black
            for (int q = threadIdx.x; q < v.ny * half; q += SUHMO_BOTTOM_NT) {
                const int j = q / half, i = 2 * (q - j * half) + ((j + v.j0 + pass) & 1);
                if (i >= v.nx) continue;
                const int idx = cidx(v, i, j);
                double lam, dnl;
                const double c = p[j * v.nx + i];
                const double lofphi = lds_lofphi<HAS_ALPHA>(v, fp, ph, p, i, j, idx, lam, dnl);
                const double denom = 1.0e-16 + lam + dnl;                      // ...OpF.ChF:154
                p[j * v.nx + i] = c + (fp.f[SUHMO_F_RHS][idx] - lofphi) / denom;   // :156
            }
            __syncthreads();
        }
        const double old = norm;
        norm = lds_residual_l2<HAS_ALPHA>(v, fp, ph, p, wsum);
        it++;
        if (norm < 1.0e-6 * first || norm > old * (1.0 - 0.1)) break;
    }
    for (int k = threadIdx.x; k < ncell; k += SUHMO_BOTTOM_NT) { const int j = k / v.nx, i = k - j * v.nx; phi[cidx(v, i, j)] = p[k]; }
    if (threadIdx.x == 0) { atomicAdd(ctr, (unsigned long long)it); atomicAdd(ctr + 1, 1ull); }
}
// one workgroup per launch target: the depth of a level (OnLevel), or the bottom depth of every ACTIVE member of an ensemble (OnMembers:
// blockIdx.z -> member; its view, constants and counters are copied from the member's rows once, fields() hands out the head canvas the
// relaxation before has left current).  Members stop after their own iteration counts; none waits for another.
// C: the counters of the level (unsigned long long *), or a device row of them per member
template <class T, bool HAS_ALPHA, class C>
__global__ __launch_bounds__(SUHMO_BOTTOM_NT) void k_relax_solve(T t, C counters)
{
    const DV v = t.view();
    const FP fp = t.fields();
    const suhmo_phys_t ph = t.phys();
    d_relax_solve<HAS_ALPHA>(v, fp, ph, row_of(t, counters));
}
template <class T, class C> static int launch_relax_solve(const T &t, bool has_alpha, C counters, hipStream_t st)
{
    if ((long)t.nx() * t.ny() > SUHMO_BOTTOM_LDS_CELLS) { suhmo_set_error("internal: RelaxSolver in one launch on %d x %d cells: more than the LDS holds", t.nx(), t.ny()); return -4; }
    if (has_alpha) return launch_grid(k_relax_solve<T, true, C>, t, dim3(1), dim3(SUHMO_BOTTOM_NT), st, counters);
    return launch_grid(k_relax_solve<T, false, C>, t, dim3(1), dim3(SUHMO_BOTTOM_NT), st, counters);
}
// an ensemble: one launch for the members `t` at their bottom depth; ctr[k]: the device counters of member k (iterations, solves)
int suhmo_batch_relax_solve(const OnMembers &t, bool has_alpha, unsigned long long *const *ctr, hipStream_t st) { return launch_relax_solve(t, has_alpha, ctr, st); }

// the bottom depth `dep` of L takes the one-launch path
bool suhmo_bottom_one_launch(const suhmo_level *L, int dep)
{
    const DV &v = L->d[dep].v;
    const long cells = (long)v.nx * v.ny;
    return cells <= SUHMO_BOTTOM_LDS_CELLS && cells <= L->bottom_one_launch_max_cells && !v.ext[0] && !v.ext[1] && !v.cfx[0] && !v.cfx[1]
           && L->desc.nx_global == 0 && L->bottom_ctr;
}

// option values of the bottom solver (suhmo_level_set_option, and the sub-levels that run this level's cycles: L->agg, L->gap)
int suhmo_bottom_configure(suhmo_level *L, int solver, long one_launch_max_cells)
{
    if (solver && !L->bottom_ctr && !L->stub) {
        HIPCHK(hipSetDevice(L->device));
        HIPCHK(hipMalloc(&L->bottom_ctr, 2 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(L->bottom_ctr, 0, 2 * sizeof(unsigned long long)));
    }
    if (L->bottom_solver != solver || L->bottom_one_launch_max_cells != one_launch_max_cells) {
        L->bottom_solver = solver; L->bottom_one_launch_max_cells = one_launch_max_cells;
        suhmo_level_drop_graphs(L);
    }
    if (L->agg) { int rc = suhmo_bottom_configure(L->agg, solver, one_launch_max_cells); if (rc) return rc; }
    if (L->gap) { int rc = suhmo_bottom_configure(L->gap, solver, one_launch_max_cells); if (rc) return rc; }
    return 0;
}

// read-only counters of the level, its agglomerated copy and its gap-height operator: 0 iterations, 1 one-launch solves, 2 host-loop solves
long suhmo_bottom_counter(const suhmo_level *L, int which)
{
    long r = 0;
    if (which == 0) r += L->bottom_host_iters;
    if (which == 2) r += L->bottom_host_solves;
    if (which < 2 && L->bottom_ctr) {
        unsigned long long h[2] = {0, 0};
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, L->bottom_ctr, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) r += (long)h[which];
    }
    if (L->agg) r += suhmo_bottom_counter(L->agg, which);
    if (L->gap) r += suhmo_bottom_counter(L->gap, which);
    return r;
}

// RelaxSolver::solve on the bottom depth (after its numBottom relaxes); tail: halo rows of phi worth keeping valid (rank strips)
int suhmo_bottom_solve(suhmo_level *L, int dep, int tail, hipStream_t st)
{
    SUHMO_TIME("RelaxSolver::solve");
    Depth &D = L->d[dep];
    if (suhmo_bottom_one_launch(L, dep)) {
        int rc1 = launch_relax_solve(on_level(L, dep), D.v.alpha != 0.0, L->bottom_ctr, st); if (rc1) return rc1;
        D.phi_fresh = 0;
        return 0;
    }
    int rc;
    double norm = 0.0;
    if ((rc = suhmo_level_residual(L, dep, st))) return rc;
    if ((rc = suhmo_level_norm(L, dep, SUHMO_F_RES, 2, &norm, st))) return rc;
    const double first = norm;
    int it = 0;
    for (; it < 40 && norm > 1.0e-20; ) {
        if ((rc = suhmo_launch_gsrb(L, dep, 2, tail, st))) return rc;
        if ((rc = suhmo_level_residual(L, dep, st))) return rc;
        const double old = norm;
        if ((rc = suhmo_level_norm(L, dep, SUHMO_F_RES, 2, &norm, st))) return rc;
        it++;
        if (norm < 1.0e-6 * first || norm > old * (1.0 - 0.1)) break;
    }
    L->bottom_host_iters += it;
    L->bottom_host_solves++;
    return 0;
}
