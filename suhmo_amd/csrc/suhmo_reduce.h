// suhmo_reduce.h -- the device reductions, each piece stated once: the walk over a view's valid cells, the block tree, the second stage
// and the grid of a first stage.  Every reduction is two-stage and deterministic: a first stage leaves one partial per workgroup, a second
// stage of one workgroup combines the partials and publishes.  The ORDER of the additions is part of the project's contract (norm(., 2),
// dot and the moulin integrals are the same bits on every rank and for every layout); it is what this file says and nothing else:
//
//   first stage   workgroups BLK2D (64 x 4), at most cap.x x cap.y of them (reduce_grid).  Thread (tx, ty) of workgroup (bx, by) takes the
//                 rows j = by * 4 + ty, + gridDim.y * 4, ... and in each the columns i = bx * 64 + tx, + gridDim.x * 64, ... and adds
//                 its terms in that order, starting from the reduction's init; then the block tree; partial[by * gridDim.x + bx]
//   block tree    sm[tid] = acc, tid = ty * blockDim.x + tx; for s = 128, 64, ..., 1: sm[tid] = op(sm[tid], sm[tid + s]) for tid < s
//   second stage  256 threads; thread t takes the partials t, t + 256, ... of each list in turn, starting from init; then the block tree
//
// op is the reduction's own; one whose values combine differently (RedSumSumMax: sum, sum, max) is asked with the value's number (red_op).
// A sum differs from the serial CPU sum by rounding only; a maximum is exact in any order.  tests/reduce_ref.py restates this order in
// numpy (two_stage_sum, block_tree) and tests/test_gpu_reductions.py holds the device to it bit for bit: change one, change the other.
#pragma once
#include "suhmo_target.h"
#include <algorithm>
#include <type_traits>

// ---- a reduction: NV values per cell that travel together, where they start and how two of them combine
struct RedMax { static constexpr int NV = 1;            // max |x|: the terms are >= 0
    static __device__ __forceinline__ double init(int) { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); } };
struct RedSum { static constexpr int NV = 1;
    static __device__ __forceinline__ double init(int) { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return a + b; } };
struct RedMax2 { static constexpr int NV = 2;           // the Picard test's pair: max h (any sign) and max |h_lagged - h|
    static __device__ __forceinline__ double init(int q) { return q == 0 ? -1.0e300 : 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); } };
// a reduction whose values do not all combine the same way says so (PER_VALUE) and takes the value's number: sum |e| w, sum e e w, max |e| of
// suhmo_compare.hip.  red_op is what the tree and the second stage call: q is a constant after unrolling, so a reduction with ONE op compiles to
// the code it always had
struct RedSumSumMax { static constexpr int NV = 3; static constexpr bool PER_VALUE = true;      // the terms are >= 0
    static __device__ __forceinline__ double init(int) { return 0.0; }
    static __device__ __forceinline__ double op(int q, double a, double b) { return q == 2 ? fmax(a, b) : a + b; } };
struct RedSum7 { static constexpr int NV = 7;           // the seven sums of the mass balance (suhmo_balance.hip), terms of any sign
    static __device__ __forceinline__ double init(int) { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return a + b; } };
struct RedSum9 { static constexpr int NV = 9;           // those seven and the two recharge sums of the water budget (suhmo_balance.hip)
    static __device__ __forceinline__ double init(int) { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return a + b; } };
template <class R, class = void> struct red_per_value : std::false_type {};
template <class R> struct red_per_value<R, std::void_t<decltype(R::PER_VALUE)>> : std::true_type {};
template <class R> __device__ __forceinline__ double red_op(int q, double a, double b)
{
    if constexpr (red_per_value<R>::value) return R::op(q, a, b);
    else return R::op(a, b);
}

// ---- the walk: f(i, j) for the valid cells of `v` this thread takes, j outer, i inner (what else a body skips -- an exclusion rectangle,
// covered cells -- is the body's business)
template <class F> __device__ __forceinline__ void for_valid_cells(const DV &v, F f)
{
    for (int j = blockIdx.y * blockDim.y + threadIdx.y; j < v.ny; j += gridDim.y * blockDim.y)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < v.nx; i += gridDim.x * blockDim.x) f(i, j);
}
// ---- the block tree over the 256 threads of a workgroup: a[] of every thread in, the result in a[] of thread 0 (tid == 0).  A caller
// that comes back for another round (d_moulin_partial, once per moulin) puts a barrier between its use of the result and the next call.
template <class R> __device__ __forceinline__ void block_tree(int tid, double (&a)[R::NV])
{
    __shared__ double sm[R::NV][256];
#pragma unroll
    for (int q = 0; q < R::NV; q++) sm[q][tid] = a[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < R::NV; q++) sm[q][tid] = red_op<R>(q, sm[q][tid], sm[q][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < R::NV; q++) a[q] = sm[q][0];
    }
}
// ---- a first stage: term(i, j, a) folds one cell into the thread's values a[NV]; the workgroup's result goes to out[0 .. NV - 1]
__device__ __forceinline__ int plane_block() { return blockIdx.y * gridDim.x + blockIdx.x; }       // the workgroup's partial within its box / member
template <class R, class F> __device__ __forceinline__ void reduce_cells(const DV &v, double *__restrict__ out, F term)
{
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    double a[R::NV];
#pragma unroll
    for (int q = 0; q < R::NV; q++) a[q] = R::init(q);
    for_valid_cells(v, [&](int i, int j) { term(i, j, a); });
    block_tree<R>(tid, a);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < R::NV; q++) out[q] = a[q];
    }
}
// ---- the second stage over a small table of lists of partials (NV doubles each; one list: a table of one row): out[0 .. NV - 1] and the
// pinned slot of the host (a second value in hs.val[1])
constexpr int RED_LISTS = 8;                         // levels of a hierarchy at most (suhmo_hier_create)
struct PartialLists { const double *p[RED_LISTS]; int n[RED_LISTS]; int cnt; };
static inline PartialLists one_list(const double *p, int n) { PartialLists pl{}; pl.p[0] = p; pl.n[0] = n; pl.cnt = 1; return pl; }
template <class R> __global__ __launch_bounds__(256) void k_norm_final(PartialLists pl, double *__restrict__ out, HostSlot hs)
{
    const int tid = threadIdx.x;
    double a[R::NV];
#pragma unroll
    for (int q = 0; q < R::NV; q++) a[q] = R::init(q);
    for (int l = 0; l < pl.cnt; l++)
        for (int k = tid; k < pl.n[l]; k += 256) {
#pragma unroll
            for (int q = 0; q < R::NV; q++) a[q] = red_op<R>(q, a[q], pl.p[l][R::NV * k + q]);
        }
    block_tree<R>(tid, a);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < R::NV; q++) out[q] = a[q];
        if (R::NV == 2 && hs.val) hs.val[1] = a[R::NV - 1];
        suhmo_publish(hs, a[0]);
    }
}
// ---- the second stage of the members of an ensemble (maxima only: exact in any order): a wave per member over its np partials, every value
// stored into the pinned slots of its member, then ONE sequence number for all of them
__device__ __forceinline__ double wave_max(double r)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r = fmax(r, __shfl_xor(r, o));
    return r;
}
template <class R> __global__ __launch_bounds__(256) void k_norm_final_members(BatchSel sel, const double *__restrict__ partial, int np, double *__restrict__ slot,
                                                                         unsigned long long *flag, unsigned long long seq)
{
    const int lane = threadIdx.x & 63;
    for (int z = threadIdx.x >> 6; z < sel.n; z += 4) {
        const int k = sel.m[z];
        double a[R::NV];
#pragma unroll
        for (int q = 0; q < R::NV; q++) a[q] = R::init(q);
        for (int p = lane; p < np; p += 64) {
#pragma unroll
            for (int q = 0; q < R::NV; q++) a[q] = fmax(a[q], partial[((size_t)k * np + p) * R::NV + q]);
        }
#pragma unroll
        for (int q = 0; q < R::NV; q++) a[q] = wave_max(a[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < R::NV; q++) slot[R::NV * k + q] = a[q];
        }
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- host side.  The grid of a first stage: the workgroups an extent asks for, under a cap
struct GridCap { int x, y; };
constexpr GridCap CAP_LEVEL{32, 128};                // a level, a member of an ensemble: up to 4096 partials (L->scratch + 2)
constexpr GridCap CAP_BOX{4, 16};                    // a box: up to 64 partials (suhmo_multi::red, suhmo_hier::red_all: 64 per box)
constexpr GridCap CAP_BOX_PAIRS{4, 8};               // a box, two values per workgroup: the same 64 doubles
static inline dim3 reduce_grid(int nx, int ny, GridCap cap) { return dim3(std::min((nx + 63) / 64, cap.x), std::min((ny + 3) / 4, cap.y)); }
// first stage over the cells of a target; *np: the partials it leaves PER box / member (those of box / member z from partial + slot(*np))
template <class T, class... P, class... A>
static int launch_partials(void (*first)(T, double *, P...), const T &t, GridCap cap, double *partial, int *np, hipStream_t st, A... a)
{
    const dim3 grd = reduce_grid(t.nx(), t.ny(), cap);
    *np = (int)(grd.x * grd.y);
    return launch_grid(first, t, grd, BLK2D, st, partial, a...);
}
template <class R> static int launch_final(const PartialLists &pl, double *out, HostSlot hs, hipStream_t st)
{
    hipLaunchKernelGGL(k_norm_final<R>, dim3(1), dim3(256), 0, st, pl, out, hs);
    HIPCHK(hipGetLastError());
    return 0;
}
// both stages of a level or of the boxes of a level (t.count() > 0): the caller reads `out` back (suhmo_readback / suhmo_reduce_finish)
template <class R, class T, class... P, class... A>
static int launch_reduction(void (*first)(T, double *, P...), const T &t, GridCap cap, double *partial, double *out, HostSlot hs, hipStream_t st, A... a)
{
    int np, rc = launch_partials(first, t, cap, partial, &np, st, a...);
    return rc ? rc : launch_final<R>(one_list(partial, np * t.count()), out, hs, st);
}
