// suhmo_compare.h -- the per-cell rule of "COMPARE" (include/suhmo_hip.h), stated ONCE as arithmetic on values and canvases: what a component is
// on either side, the average of the exact solution over the r x r block under a level cell, the three terms a cell contributes.  The ORDER of
// the additions is part of the rule (tests/compare_ref.py restates it in numpy: change one, change the other):
//   component    FIELD: a[idx];  DIFF: a[idx] - b[idx], formed per cell on each side before anything else; a field that is not held counts as 0.0
//   row sum      the r values of a row of the block as a pairwise tree of neighbours: (x0 + x1) + (x2 + x3), ... (r a power of two, <= 64)
//   block        the r row sums in ascending row order, starting from the first row's sum; times 1.0 / (r r) (exact); r = 1: the value as it is
//   terms        e = c - avg;  a0 += |e| w;  a1 += (e e) w;  a2 = max(a2, |e|)        -- products rounded before the sums, nothing contracted
// A covered cell (SUHMO_F_COVER != 0) contributes nothing and its block is not read.
// The kernels of suhmo_compare.hip call cmp_value and cmp_fold for every cell; where r >= 2 they form the row sums with __shfl_xor butterflies over
// groups of r lanes (lane k of a group after the step o = 1, 2, ...: its own sum + that of lane k ^ o -- the same tree, addition being
// commutative) and add the rows as cmp_block_average does.  cmp_cell is the whole rule for one level cell in serial form.
//
// Plain C++ once __device__ and __forceinline__ are defined away and DV / cidx exist (tests/host_cpp/compare_emu.cpp).
#pragma once
#include <math.h>

__device__ __forceinline__ double cmp_value(bool diff, const double *__restrict__ a, const double *__restrict__ b, long idx)
{
    double x = a ? a[idx] : 0.0;
    if (diff) x = x - (b ? b[idx] : 0.0);
    return x;
}
// x[0 .. r - 1] -> their sum as the pairwise tree of neighbours (x is used up)
__device__ __forceinline__ double cmp_row_tree(double *x, int r)
{
    for (int s = 1; s < r; s <<= 1)
        for (int k = 0; k < r; k += 2 * s) x[k] = x[k] + x[k + s];
    return x[0];
}
// the exact side under the level cell whose block starts at the exact cell (fi0, fj0): xv its view, xa / xb the component's fields there
__device__ __forceinline__ double cmp_block_average(const DV &xv, bool diff, const double *__restrict__ xa, const double *__restrict__ xb, int fi0, int fj0, int r)
{
    if (r == 1) return cmp_value(diff, xa, xb, cidx(xv, fi0, fj0));
    double acc = 0.0;
    for (int q = 0; q < r; q++) {
        double x[64];
        for (int p = 0; p < r; p++) x[p] = cmp_value(diff, xa, xb, cidx(xv, fi0 + p, fj0 + q));
        const double s = cmp_row_tree(x, r);
        acc = q == 0 ? s : acc + s;
    }
    return acc * (1.0 / (double)(r * r));
}
__device__ __forceinline__ void cmp_fold(double c, double avg, double w, double (&a)[3])
{
    const double e = c - avg, ae = fabs(e);
    a[0] = a[0] + ae * w;
    a[1] = a[1] + (e * e) * w;
    a[2] = fmax(a[2], ae);
}
// cell (i, j) of the box with view v (its component: ca / cb, its covered cells: cover or NULL) against the exact level, r = 1 << sh
__device__ __forceinline__ void cmp_cell(const DV &v, int i, int j, bool diff, const double *__restrict__ ca, const double *__restrict__ cb,
                                         const double *__restrict__ cover, const DV &xv, const double *__restrict__ xa, const double *__restrict__ xb,
                                         int sh, double w, double (&a)[3])
{
    const int idx = cidx(v, i, j);
    if (cover && cover[idx] != 0.0) return;                  // before its block is read
    cmp_fold(cmp_value(diff, ca, cb, idx), cmp_block_average(xv, diff, xa, xb, (v.i0 + i) << sh, (v.j0 + j) << sh, 1 << sh), w, a);
}
