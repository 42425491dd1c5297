// suhmo_compare.hip -- the composite error of a hierarchy against a finer single-level run, reduced on the device: the L1, L2 and max norms the
// reference's convergence tables hold (CONV_ANA/scripts/launch_comparaison*.py: ChomboCompare on the levels of a plot file, and on the plotCustom
// composites).  The rule, the modes and the refusals: include/suhmo_hip.h, "COMPARE"; the per-cell arithmetic: suhmo_compare.h; the order of the
// sums: suhmo_reduce.h; tests/compare_ref.py is the numpy twin of all three.  Read-only.
//
// Per call, on one stream:
//   COMPOSITE   k_cmp_level    one launch per level, every component in it: the first stage of suhmo_reduce.h over the level's cells (CAP_LEVEL for
//                              level 0, CAP_BOX per box), 3 values per workgroup and component
//   FINEST      the device part of suhmo_hier_flatten, then k_cmp_finest: one first stage (CAP_LEVEL) over the finest array
//   both        k_cmp_final    one launch: the second stage per component over all lists (and, for level_terms, over each list alone);
//                              one hipMemcpyAsync of its 3 doubles per component (and list), one synchronisation
// k_cmp_level is FINE-CENTRIC where r = 2^(exact_level - l) >= 2: a wave owns 64 cells of a level row (the walk of suhmo_reduce.h: wave = ty) and
// streams the 64 r exact cells under them row by row, 64 consecutive doubles per load instruction; groups of r lanes add their values with
// butterflies (group_sum: the pairwise tree of suhmo_compare.h), one __shfl hands each row sum to the lane that owns the level cell, and that
// lane adds the r rows in ascending order.  A wave whose 64 cells are all covered (or beyond the box) reads nothing, and no lane reads under a
// covered cell (its load goes to a cell that counts, its value is 0.0).  Plain vector loads and stores, no atomics, no LDS beyond block_tree's.
#include "suhmo_hier_int.h"
#include "suhmo_level_int.h"
#include "suhmo_reduce.h"
#include "suhmo_compare.h"
#include <climits>
#include <cmath>

using namespace hier;

namespace {
using Red = RedSumSumMax;

// ---- the pairwise tree of neighbours over groups of R lanes, every lane of a group left with the group's sum: the butterfly x = x + (the sum of
// the other half), halves of 1, 2, 4, ... lanes.  After the step of o lanes every lane of a 2 o group holds the same bits (addition commutes), so
// ANY lane of the other half serves as the partner: lane ^ 1 and lane ^ 2 are quad permutes, the mirror of a half row (lane 7 - k of 8) and of a
// row (lane 15 - k of 16) lie in the other half -- four DPP moves instead of LDS-pipe permutes; lane ^ 16 is a swizzle, lane ^ 32 a __shfl_xor
template <int CTRL> __device__ __forceinline__ double dpp_f64(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double swizzle_xor16(double x)
{
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401f);     // bit mode: and 0x1f, or 0, xor 0x10
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401f);
    return __hiloint2double(hi, lo);
}
template <int R> __device__ __forceinline__ double group_sum(double x)
{
    if constexpr (R > 1) x = x + dpp_f64<0xb1>(x);           // quad_perm [1, 0, 3, 2]
    if constexpr (R > 2) x = x + dpp_f64<0x4e>(x);           // quad_perm [2, 3, 0, 1]
    if constexpr (R > 4) x = x + dpp_f64<0x141>(x);          // row_half_mirror
    if constexpr (R > 8) x = x + dpp_f64<0x140>(x);          // row_mirror
    if constexpr (R > 16) x = x + swizzle_xor16(x);
    if constexpr (R > 32) x = x + __shfl_xor(x, 32);
    return x;
}

// the workgroup's three values of component q: partial + q * comp_stride + 3 * (its place in the level's list).  The components are taken in
// turn (three values times sixteen components do not fit one block_tree), with the barrier d_moulin_partial puts between its rounds
template <class T, int SH> __global__ __launch_bounds__(256) void k_cmp_level(T t, double *__restrict__ partial, FlatComps c, DV xv, FP xfp, double w, long comp_stride)
{
    constexpr int R = 1 << SH;
    const DV &v = t.view();
    const FP &fp = t.fields();
    const int lane = threadIdx.x, tid = threadIdx.y * 64 + lane;
    const double *__restrict__ cover = fp.f[SUHMO_F_COVER];
    double *__restrict__ out = partial + 3 * (t.slot((size_t)gridDim.x * gridDim.y) + plane_block());
    const int src = (lane << SH) & 63, mine = (lane << SH) >> 6;         // the pass and the lane in which this lane's row sum appears
    for (int q = 0; q < c.n; q++) {
        const bool diff = c.kind[q] == SUHMO_FLAT_DIFF;
        const double *__restrict__ ca = fp.f[c.f1[q]], *__restrict__ cb = fp.f[c.f2[q]];
        const double *__restrict__ xa = xfp.f[c.f1[q]], *__restrict__ xb = xfp.f[c.f2[q]];
        double a[Red::NV] = {0.0, 0.0, 0.0};
        // for_valid_cells, a wave at a time: j and ib are the same in every lane of a wave
        for (int j = blockIdx.y * 4 + threadIdx.y; j < v.ny; j += gridDim.y * 4)
            for (int ib = blockIdx.x * 64; ib < v.nx; ib += gridDim.x * 64) {
                const int i = ib + lane;
                const bool live = i < v.nx && !(cover && cover[cidx(v, i, j)] != 0.0);
                const unsigned long long lm = __ballot(live);
                if (!lm) continue;
                double avg = 0.0;
                if constexpr (SH == 0) {
                    if (live) avg = cmp_value(diff, xa, xb, cidx(xv, v.i0 + i, v.j0 + j));
                } else {
                    // batches of U loads of 64 consecutive doubles each; the loads of the next batch are issued before the butterflies of this
                    // one (a level of 256 x 256 cells gives every SIMD ONE wave: nothing else hides the latency).  A lane whose level cell
                    // does not count loads the first exact cell under the wave's first cell that does (in bounds, under no covered cell)
                    // and takes 0.0
                    constexpr int U = R <= 16 ? R : 8, NB = R / U, NT = R * NB;
                    const int fi0 = (v.i0 + ib) << SH, fj0 = (v.j0 + j) << SH, safe = (__ffsll((long long)lm) - 1) << SH;
                    // bit k: the level cell over this lane's exact cell in pass k counts.  What depends on it and on `mine` below is
                    // integer arithmetic on purpose: as tests they are the same in every batch, and the compiler keeps a lane mask in a
                    // pair of scalar registers for each of them across the loop (64 and more, spilled).  The sum of a group whose cell does
                    // not count is never used (its lanes form no other group's sum): its values need no zeroing
                    unsigned long long okbits = 0;
#pragma unroll 1
                    for (int k = 0; k < R; k++) okbits |= ((lm >> ((k * 64 + lane) >> SH)) & 1ull) << k;
                    // (cmp_value without its tests: the host has made sure that `exact` holds both fields, and DIFF is decided once per
                    //  component -- a test inside the batch would end the compiler's count of the loads in flight at every branch)
                    auto block = [&](auto DIFF) {
                    auto load = [&](int t, double (&x)[U]) {
                        const int fr = t / NB, k0 = (t % NB) * U;
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            const int fl = (k0 + u) * 64 + lane;       // the exact cell of this lane within the 64 R of the row
                            const int idx = cidx(xv, fi0 + safe + (int)((okbits >> (k0 + u)) & 1ull) * (fl - safe), fj0 + fr);
                            x[u] = xa[idx];
                            if constexpr (decltype(DIFF)::value) x[u] = x[u] - xb[idx];
                        }
                    };
                    long long rs = 0;                        // the bits of this lane's row sum
                    auto fold_batch = [&](int t, const double (&x)[U]) {
                        const int k0 = (t % NB) * U;
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            const long long g = __double_as_longlong(__shfl(group_sum<R>(x[u]), src));
                            const long long keep = (long long)((((k0 + u) ^ mine) - 1) >> 31);     // -1 where k0 + u == mine, else 0
                            rs = (g & keep) | (rs & ~keep);
                        }
                        if (t % NB == NB - 1) avg = t / NB == 0 ? __longlong_as_double(rs) : avg + __longlong_as_double(rs);       // a row of the block is complete
                    };
                    double xe[U], xo[U];                     // two sets of registers trading places (NT is even): no copy waits for a load
                    load(0, xe);
#pragma unroll 1
                    for (int t = 0; t < NT; t += 2) {
                        load(t + 1, xo);
                        fold_batch(t, xe);
                        if (t + 2 < NT) load(t + 2, xe);
                        fold_batch(t + 1, xo);
                    }
                    };
                    if (diff) block(std::true_type{}); else block(std::false_type{});
                    avg = avg * (1.0 / (double)(R * R));
                }
                if (live) cmp_fold(cmp_value(diff, ca, cb, cidx(v, i, j)), avg, w, a);
            }
        block_tree<Red>(tid, a);
        if (tid == 0) {
#pragma unroll
            for (int m = 0; m < Red::NV; m++) out[q * comp_stride + m] = a[m];
        }
        __syncthreads();
    }
}

// the first stage over the finest array of a flatten (flat: [comp][j][i], nx x ny of xv each): e = flat - x
__global__ __launch_bounds__(256) void k_cmp_finest(DV xv, FP xfp, FlatComps c, const double *__restrict__ flat, long plane, double w,
                                                    double *__restrict__ partial, long comp_stride)
{
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    double *__restrict__ out = partial + 3 * plane_block();
    for (int q = 0; q < c.n; q++) {
        const bool diff = c.kind[q] == SUHMO_FLAT_DIFF;
        const double *__restrict__ xa = xfp.f[c.f1[q]], *__restrict__ xb = xfp.f[c.f2[q]];
        const double *__restrict__ fq = flat + q * plane;
        double a[Red::NV] = {0.0, 0.0, 0.0};
        for_valid_cells(xv, [&](int i, int j) { cmp_fold(fq[(long)j * xv.nx + i], cmp_value(diff, xa, xb, cidx(xv, i, j)), w, a); });
        block_tree<Red>(tid, a);
        if (tid == 0) {
#pragma unroll
            for (int m = 0; m < Red::NV; m++) out[q * comp_stride + m] = a[m];
        }
        __syncthreads();
    }
}

// the second stage of suhmo_reduce.h (k_norm_final's walk) for component blockIdx.x over all lists (blockIdx.y = 0) or over list blockIdx.y - 1
// alone: out[blockIdx.y][component][3]
__global__ __launch_bounds__(256) void k_cmp_final(PartialLists pl, long comp_stride, double *__restrict__ out)
{
    const int tid = threadIdx.x, q = blockIdx.x, only = (int)blockIdx.y - 1;
    double a[Red::NV] = {0.0, 0.0, 0.0};
    for (int l = 0; l < pl.cnt; l++) {
        if (only >= 0 && l != only) continue;
        const double *__restrict__ p = pl.p[l] + q * comp_stride;
        for (int k = tid; k < pl.n[l]; k += 256) {
#pragma unroll
            for (int m = 0; m < Red::NV; m++) a[m] = red_op<Red>(m, a[m], p[Red::NV * k + m]);
        }
    }
    block_tree<Red>(tid, a);
    if (tid == 0) {
#pragma unroll
        for (int m = 0; m < Red::NV; m++) out[((size_t)blockIdx.y * gridDim.x + q) * Red::NV + m] = a[m];
    }
}

template <class T> int launch_cmp_level(const T &t, GridCap cap, int sh, hipStream_t st, double *partial, const FlatComps &c, const DV &xv, const FP &xfp,
                                        double w, long comp_stride, int *np)
{
    const dim3 grd = reduce_grid(t.nx(), t.ny(), cap);
    *np = (int)(grd.x * grd.y) * t.count();
    switch (sh) {
    case 0: return launch_grid(k_cmp_level<T, 0>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    case 1: return launch_grid(k_cmp_level<T, 1>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    case 2: return launch_grid(k_cmp_level<T, 2>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    case 3: return launch_grid(k_cmp_level<T, 3>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    case 4: return launch_grid(k_cmp_level<T, 4>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    case 5: return launch_grid(k_cmp_level<T, 5>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    default: return launch_grid(k_cmp_level<T, 6>, t, grd, BLK2D, st, partial, c, xv, xfp, w, comp_stride);
    }
}

// partials a hierarchy can leave in one list set: level 0 (or the finest array) under CAP_LEVEL, 64 per box
size_t partial_cap(const suhmo_hier *H)
{
    size_t n = (size_t)CAP_LEVEL.x * CAP_LEVEL.y;
    for (int l = 1; l < H->nlev; l++) n += 64 * H->lev[l].box.size();
    return n;
}
constexpr size_t OUT_DOUBLES = (size_t)(1 + RED_LISTS) * SUHMO_FLAT_MAX_COMPS * Red::NV;
}  // namespace

void suhmo_hier_compare_release_(suhmo_hier *H)
{
    if (H->cmp_buf) (void)hipFree(H->cmp_buf);
    H->cmp_buf = nullptr; H->cmp_cap = 0;
}

extern "C" int suhmo_hier_compare(suhmo_hier_t *H, suhmo_level_t *exact, int exact_level, int mode, int ncomp, const suhmo_flat_comp_t *comps,
                                  double *norms, double *level_terms, suhmo_stream_t s)
{
    SUHMO_TIME("suhmo_hier_compare");
    const char *who = "suhmo_hier_compare";
    ARG(H && H->nlev >= 1 && norms);
    FlatComps c;
    int rc;
    if ((rc = suhmo_flat_comps_(who, ncomp, comps, c))) return rc;
    if (mode != SUHMO_CMP_COMPOSITE && mode != SUHMO_CMP_FINEST) { suhmo_set_error("%s: mode %d", who, mode); return -1; }
    if (mode == SUHMO_CMP_FINEST && level_terms) { suhmo_set_error("%s: level_terms belong to SUHMO_CMP_COMPOSITE", who); return -1; }
    if (!exact) { suhmo_set_error("%s: no exact level", who); return -1; }
    const int top = H->nlev - 1, nlev = H->nlev;
    if (exact_level < top) { suhmo_set_error("%s: exact_level = %d is below the finest level %d", who, exact_level, top); return -1; }
    if ((rc = suhmo_hier_flatten_check_(H, exact_level))) return rc;         // the finest grid within int; rc -5 for the layouts that are not built
    const suhmo_level_desc_t &xd = exact->desc;
    if (exact->stub || on_strip(exact) || xd.j0 != 0 || (xd.ny_global && xd.ny_global != xd.ny)) {
        suhmo_set_error("%s: the exact level is a rank strip: not built", who); return -5;
    }
    if (exact->device != H->device) { suhmo_set_error("%s: the exact level is on device %d, the hierarchy on device %d: not built", who, exact->device, H->device); return -5; }
    const DV &xv = exact->d[0].v;
    const long nxF = (long)H->lev[0].nxd << exact_level, nyF = (long)H->lev[0].nyd << exact_level;
    if (xv.nx != nxF || xv.ny != nyF || xv.i0 != 0 || xv.j0 != 0 || exact->d[0].elems > (size_t)INT_MAX) {
        suhmo_set_error("%s: the exact level holds %d x %d cells, level %d of the hierarchy's domain %ld x %ld", who, xv.nx, xv.ny, exact_level, nxF, nyF); return -1;
    }
    if (mode == SUHMO_CMP_COMPOSITE && exact_level > 6) { suhmo_set_error("%s: r = 2^%d on level 0 (64 at most)", who, exact_level); return -1; }
    const FP &xfp = exact->d[0].fp;
    for (int q = 0; q < ncomp; q++)
        for (int f : {c.f1[q], c.f2[q]})
            if (!xfp.f[f]) { suhmo_set_error("%s: component %d: the exact level does not hold field %d", who, q, f); return -1; }
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(H->device));
    const size_t cap = partial_cap(H);
    if (!H->cmp_buf) {
        const size_t n = (size_t)SUHMO_FLAT_MAX_COMPS * Red::NV * cap + OUT_DOUBLES;
        if (hipMalloc(&H->cmp_buf, n * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            H->cmp_buf = nullptr;
            suhmo_set_error("%s: the partial buffer (%zu doubles) cannot be allocated", who, n); return -2;
        }
        H->cmp_cap = n;
    }
    const long comp_stride = (long)(Red::NV * cap);
    double *const out = H->cmp_buf + (size_t)SUHMO_FLAT_MAX_COMPS * Red::NV * cap;
    PartialLists pl{};
    if (mode == SUHMO_CMP_COMPOSITE) {
        size_t off = 0;
        for (int l = 0; l < nlev; l++) {
            const DV &v0 = H->lev[l].box[0]->d[0].v;
            const double w = v0.dx * v0.dy;
            double *partial = H->cmp_buf + Red::NV * off;
            int np = 0;
            rc = on_hier_level(H, l, st, [&](const auto &t) {
                return launch_cmp_level(t, l == 0 ? CAP_LEVEL : CAP_BOX, exact_level - l, st, partial, c, xv, xfp, w, comp_stride, &np); });
            if (rc) return rc;
            H->n_cmp_launches++;
            pl.p[l] = partial; pl.n[l] = np; off += (size_t)np;
        }
        pl.cnt = nlev;
    } else {
        if ((rc = suhmo_hier_flatten_device_(H, exact_level, c, st))) return rc;
        const dim3 grd = reduce_grid(xv.nx, xv.ny, CAP_LEVEL);
        hipLaunchKernelGGL(k_cmp_finest, grd, BLK2D, 0, st, xv, xfp, c, (const double *)H->flat_buf, nxF * nyF, xv.dx * xv.dy, H->cmp_buf, comp_stride);
        HIPCHK(hipGetLastError());
        H->n_cmp_launches++;
        pl = one_list(H->cmp_buf, (int)(grd.x * grd.y));
    }
    const int nrow = level_terms ? 1 + nlev : 1;
    hipLaunchKernelGGL(k_cmp_final, dim3(ncomp, nrow), dim3(256), 0, st, pl, comp_stride, out);
    HIPCHK(hipGetLastError());
    H->n_cmp_launches++;
    double res[OUT_DOUBLES];
    HIPCHK(hipMemcpyAsync(res, out, (size_t)nrow * ncomp * Red::NV * sizeof(double), hipMemcpyDeviceToHost, st));
    H->n_cmp_copies++;
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 0; q < ncomp; q++) { norms[3 * q] = res[3 * q]; norms[3 * q + 1] = sqrt(res[3 * q + 1]); norms[3 * q + 2] = res[3 * q + 2]; }
    if (level_terms) memcpy(level_terms, res + Red::NV * ncomp, (size_t)nlev * ncomp * Red::NV * sizeof(double));
    return 0;
}
