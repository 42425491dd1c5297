// suhmo_target.h -- what a kernel is launched over.  A device body (d_*) works on one view DV, one set of field pointers FP and the
// physics constants; a launch target says where a workgroup finds them and what blockIdx.z means.  Every body has ONE __global__
// template over the target type, instantiated for the targets that are launched; launch_over() below is the one place that turns a
// target and an extent into a grid.  Targets are plain values passed to kernels by value (a captured graph keeps what they held).
//
//   OnLevel    one level / depth:       its view, pointers and constants themselves             blockIdx.z unused
//   OnBoxes    the boxes of a level:    device tables of views and pointers (suhmo_multi)      blockIdx.z = box
//   OnMembers  members of an ensemble:  device tables of every member + the active list        blockIdx.z -> active member
//
// Device side: view(), fields() (field(f): one of them by number), phys(), model() (time step) and slot(n) (where a body that leaves n partials per launch of one
// level puts those of this box / member).  Host side: count() = gridDim.z (0: nothing to launch) and nx() / ny(), the extent.
// A new target is one more struct with these members; the kernels it launches gain an instantiation, nothing else changes.
#pragma once
#include "suhmo_common.h"

#define BLK2D dim3(64, 4)

struct OnLevel {
    DV v; FP fp; suhmo_phys_t ph;
    __device__ __forceinline__ const DV &view() const { return v; }
    __device__ __forceinline__ const FP &fields() const { return fp; }
    __device__ __forceinline__ double *field(int f) const { return fp.f[f]; }
    __device__ __forceinline__ const FP *table() const { return nullptr; }                // (no neighbours to write to)
    __device__ __forceinline__ const suhmo_phys_t &phys() const { return ph; }
    __device__ __forceinline__ size_t slot(size_t) const { return 0; }
    int count() const { return 1; }
    int nx() const { return v.nx; }
    int ny() const { return v.ny; }
};
static inline OnLevel on_level(const suhmo_level *L, int depth) { return OnLevel{L->d[depth].v, L->d[depth].fp, L->ph}; }

struct OnBoxes {
    const DV *dv; const FP *fp; suhmo_phys_t ph; int nbox, maxnx, maxny;
    __device__ __forceinline__ const DV &view() const { return dv[blockIdx.z]; }
    __device__ __forceinline__ const FP &fields() const { return fp[blockIdx.z]; }
    __device__ __forceinline__ double *field(int f) const { return fp[blockIdx.z].f[f]; }
    __device__ __forceinline__ const FP *table() const { return fp; }                     // every box's pointers: a colour pass pushes into its neighbours' ghosts
    __device__ __forceinline__ const suhmo_phys_t &phys() const { return ph; }
    __device__ __forceinline__ size_t slot(size_t n) const { return blockIdx.z * n; }
    int count() const { return nbox; }               // 0: a rank that owns no box of the level
    int nx() const { return maxnx; }
    int ny() const { return maxny; }
};

// ---- an ensemble.  A launch has gridDim.z = number of ACTIVE members; blockIdx.z picks, through the active list (a by-value kernel
// argument: no launch and no synchronisation to maintain it), a row of the per-depth device tables DV[n] / FP[n] / suhmo_phys_t[n].
// The tile relaxation writes out of place and trades the two head canvases of a depth; members that leave the active list stop
// trading, so which canvas holds a member's head is a bit per member (`alt`) that travels with the table: the tables themselves are
// written once, and fields() is the only way to a member's pointers.
constexpr int SUHMO_BATCH_MAX = 64;      // members of a batch (one bit each in BatchTab::alt)
struct BatchSel { int n; unsigned char m[SUHMO_BATCH_MAX]; };       // active list: blockIdx.z -> member
// one multigrid depth of every member.  fp[k].f[SUHMO_F_PHI] / f[SUHMO_F_PHI2]: the two head canvases of member k as they lay when the
// table was written; bit k of alt: they have traded places since (a whole level has no other use for SUHMO_F_PHI2)
struct BatchTab { const DV *dv; const FP *fp; const suhmo_phys_t *ph; unsigned long long alt; };
__device__ __forceinline__ int batch_member(const BatchSel &s) { return s.m[blockIdx.z]; }
__device__ __forceinline__ FP batch_fp(const BatchTab &t, int k)
{
    FP fp = t.fp[k];
    if ((t.alt >> k) & 1) { double *a = fp.f[SUHMO_F_PHI]; fp.f[SUHMO_F_PHI] = fp.f[SUHMO_F_PHI2]; fp.f[SUHMO_F_PHI2] = a; }
    return fp;
}
struct OnMembers {
    BatchTab t; BatchSel sel; const suhmo_model_params_t *mp; int nx_, ny_;      // mp: device rows of mp[n] (time step), or NULL
    __device__ __forceinline__ int member() const { return batch_member(sel); }
    __device__ __forceinline__ const DV &view() const { return t.dv[member()]; }
    __device__ __forceinline__ FP fields() const { return batch_fp(t, member()); }
    __device__ __forceinline__ double *field(int f) const      // fields().f[f] for a field number known only at run time: the swap on the number
    {
        const int k = member();
        if (((t.alt >> k) & 1) && (f == SUHMO_F_PHI || f == SUHMO_F_PHI2)) f = f == SUHMO_F_PHI ? SUHMO_F_PHI2 : SUHMO_F_PHI;
        return t.fp[k].f[f];
    }
    __device__ __forceinline__ const FP *table() const { return nullptr; }
    __device__ __forceinline__ const suhmo_phys_t &phys() const { return t.ph[member()]; }
    __device__ __forceinline__ const suhmo_model_params_t &model() const { return mp[member()]; }
    __device__ __forceinline__ size_t slot(size_t n) const { return member() * n; }
    int count() const { return sel.n; }
    int nx() const { return nx_; }
    int ny() const { return ny_; }
};
// `v`: the view of any member at that depth (the members share the grid)
static inline OnMembers on_members(const BatchTab &t, const BatchSel &sel, const DV &v, const suhmo_model_params_t *mp = nullptr)
{
    return OnMembers{t, sel, mp, v.nx, v.ny};
}
// a level or the boxes of a level in a time-step kernel: the one set of model parameters by value
template <class T> struct Stepping : T {
    suhmo_model_params_t mp;
    __device__ __forceinline__ const suhmo_model_params_t &model() const { return mp; }
};
template <class T> static inline Stepping<T> stepping(const T &t, const suhmo_model_params_t &mp) { return Stepping<T>{t, mp}; }
// a table a kernel needs beside the target's own: by value for a level, a device row per member of an ensemble
template <class M> __device__ __forceinline__ const M &row_of(const OnLevel &, const M &m) { return m; }
template <class M> __device__ __forceinline__ const M &row_of(const OnBoxes &, const M &m) { return m; }           // (one table for every box of the level)
template <class M> __device__ __forceinline__ const M &row_of(const OnMembers &t, const M *m) { return m[t.member()]; }
// a number a kernel needs per launch: itself for a level, one per member of an ensemble -- like BatchSel a kernel argument by value (512 B: no
// copy and no synchronisation maintains it)
struct PerMember { double x[SUHMO_BATCH_MAX]; };
__device__ __forceinline__ double value_of(const OnLevel &, double x) { return x; }
__device__ __forceinline__ double value_of(const OnBoxes &, double x) { return x; }       // (one value for every box of the level)
__device__ __forceinline__ double value_of(const OnMembers &t, const PerMember &p) { return p.x[t.member()]; }

// ---- the grid of a launch: what the threads of a target's x-y plane stand for
enum Extent { CELLS, FACES /* cells + 1 */, GHOSTED /* the box with its ghost ring: cells + 2 */, PERIMETER /* 2 nx + 2 ny, 256 threads */ };
// grid (gx, gy, count()) of workgroups `blk`: launches, reports a launch error, returns 0 for an empty target
template <class T, class... P, class... A>
static int launch_grid(void (*kernel)(T, P...), const T &t, dim3 grd, dim3 blk, hipStream_t st, A... a)
{
    if (t.count() <= 0) return 0;
    grd.z = t.count();
    hipLaunchKernelGGL(kernel, grd, blk, 0, st, t, a...);
    HIPCHK(hipGetLastError());
    return 0;
}
static inline dim3 grid2d(int nx, int ny) { return dim3((nx + 63) / 64, (ny + 3) / 4); }      // workgroups BLK2D over nx x ny threads
template <class T, class... P, class... A>
static int launch_over(void (*kernel)(T, P...), const T &t, Extent e, hipStream_t st, A... a)
{
    if (e == PERIMETER) return launch_grid(kernel, t, dim3((2 * t.nx() + 2 * t.ny() + 255) / 256), dim3(256), st, a...);
    const int g = e == CELLS ? 0 : e == FACES ? 1 : 2;
    return launch_grid(kernel, t, grid2d(t.nx() + g, t.ny() + g), BLK2D, st, a...);
}
