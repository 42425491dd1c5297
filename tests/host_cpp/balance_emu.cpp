// balance_emu.cpp -- the per-face and per-cell rule of "MASS BALANCE" (suhmo_amd/csrc/suhmo_balance.h: mb_fold and what it calls) run on the HOST over
// whole levels of boxes, compiled as plain C++ with -ffp-contract=off and the address and undefined-behaviour sanitizers
// (tests/test_massbalance_cpu.py).  The canvases are heap blocks of exactly the library's size, so an access outside one is reported; whatever the
// rule must not read (the head's ghost cells on a physical or wrapped side, corners, B's ring, the canvas beyond the ring) is poisoned by the caller.
// The sums are taken in the order of suhmo_amd/csrc/suhmo_reduce.h, restated here as loops (the walk, the block tree, the second stage), so that
// the output is compared bit for bit with tests/massbalance_ref.py.  CPU only; needs no device.
//   balance_emu IN OUT     IN: 1 int (nlev); per level: 3 ints (nbox capx capy); per box 19 ints (nx ny P gy i0 j0 nxg nyg per[2] cfx[2] ext[2]
//                          bct[2][2] elems), 10 doubles (dx dy two_v[2][2] neu[2][2]) and 5 canvases (head mask B bx by)
//                          OUT: nlev x 7 doubles
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define SUHMO_XOFF 16
enum { SUHMO_MB_LO_X = 0, SUHMO_MB_HI_X, SUHMO_MB_LO_Y, SUHMO_MB_HI_Y, SUHMO_MB_DIR_X, SUHMO_MB_DIR_Y, SUHMO_MB_VOLUME, SUHMO_MB_COUNT };
// the members of the library's view (suhmo_common.h: DV) the rule reads, and its four neighbour functions, word for word
struct DV { int nx, ny, P, gy, i0, j0, nxg, nyg, per[2], cfx[2], ext[2], bct[2][2]; double dx, dy, two_v[2][2], neu[2][2]; };
static inline int cidx(const DV &v, int i, int j) { return (j + v.gy) * v.P + SUHMO_XOFF + i; }
#define __device__
#define __forceinline__ inline
#define __restrict__
__device__ __forceinline__ double phiW(const DV &v, const double *__restrict__ p, int idx, int i, double c, bool homog)
{
    if (i > 0 || v.cfx[0]) return p[idx - 1];
    if (v.per[0]) return p[idx + v.nx - 1];
    if (v.bct[0][0] == 0) return (homog ? 0.0 : v.two_v[0][0]) - c;
    return homog ? c : c + v.neu[0][0];
}
__device__ __forceinline__ double phiE(const DV &v, const double *__restrict__ p, int idx, int i, double c, bool homog)
{
    if (i < v.nx - 1 || v.cfx[1]) return p[idx + 1];
    if (v.per[0]) return p[idx - (v.nx - 1)];
    if (v.bct[0][1] == 0) return (homog ? 0.0 : v.two_v[0][1]) - c;
    return homog ? c : c + v.neu[0][1];
}
__device__ __forceinline__ double phiS(const DV &v, const double *__restrict__ p, int idx, int j, double c, bool homog)
{
    if (j > 0 || v.ext[0]) return p[idx - v.P];
    if (v.per[1]) return p[idx + (v.ny - 1) * v.P];
    if (v.bct[1][0] == 0) return (homog ? 0.0 : v.two_v[1][0]) - c;
    return homog ? c : c + v.neu[1][0];
}
__device__ __forceinline__ double phiN(const DV &v, const double *__restrict__ p, int idx, int j, double c, bool homog)
{
    if (j < v.ny - 1 || v.ext[1]) return p[idx + v.P];
    if (v.per[1]) return p[idx - (v.ny - 1) * v.P];
    if (v.bct[1][1] == 0) return (homog ? 0.0 : v.two_v[1][1]) - c;
    return homog ? c : c + v.neu[1][1];
}
#include "../../suhmo_amd/csrc/suhmo_balance.h"

constexpr int NV = SUHMO_MB_COUNT;
static void block_tree(double (*sm)[NV])                    // sm[256][NV] -> sm[0]
{
    for (int s = 128; s > 0; s >>= 1)
        for (int tid = 0; tid < s; tid++)
            for (int q = 0; q < NV; q++) sm[tid][q] = sm[tid][q] + sm[tid + s][q];
}
static void second_stage(const std::vector<double> &p, double *out)
{
    static double a[256][NV];
    for (int t = 0; t < 256; t++) for (int q = 0; q < NV; q++) a[t][q] = 0.0;
    for (int t = 0; t < 256; t++)
        for (size_t k = t; k < p.size() / NV; k += 256)
            for (int q = 0; q < NV; q++) a[t][q] = a[t][q] + p[NV * k + q];
    block_tree(a);
    for (int q = 0; q < NV; q++) out[q] = a[0][q];
}
struct Box { DV v; std::vector<double> c[5]; };
static bool rd(FILE *f, void *p, size_t sz, size_t n) { return fread(p, sz, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int nlev; if (!rd(f, &nlev, 4, 1)) return 2;
    std::vector<double> out((size_t)NV * nlev);
    for (int l = 0; l < nlev; l++) {
        int h[3]; if (!rd(f, h, 4, 3)) return 2;
        std::vector<Box> box(h[0]);
        int mx = 0, my = 0;
        for (Box &B : box) {
            int q[19]; double d[10];
            if (!rd(f, q, 4, 19) || !rd(f, d, 8, 10)) return 2;
            DV &v = B.v;
            v.nx = q[0]; v.ny = q[1]; v.P = q[2]; v.gy = q[3]; v.i0 = q[4]; v.j0 = q[5]; v.nxg = q[6]; v.nyg = q[7];
            for (int k = 0; k < 2; k++) { v.per[k] = q[8 + k]; v.cfx[k] = q[10 + k]; v.ext[k] = q[12 + k]; }
            for (int k = 0; k < 4; k++) { v.bct[k / 2][k % 2] = q[14 + k]; v.two_v[k / 2][k % 2] = d[2 + k]; v.neu[k / 2][k % 2] = d[6 + k]; }
            v.dx = d[0]; v.dy = d[1];
            for (std::vector<double> &c : B.c) { c.resize(q[18]); if (!rd(f, c.data(), 8, c.size())) return 2; }
            mx = std::max(mx, v.nx); my = std::max(my, v.ny);
        }
        const int gx = std::min((mx + 63) / 64, h[1]), gy = std::min((my + 3) / 4, h[2]);
        std::vector<double> list;
        for (const Box &B : box)
            for (int by = 0; by < gy; by++) for (int bx = 0; bx < gx; bx++) {
                static double sm[256][NV];
                for (int ty = 0; ty < 4; ty++) for (int tx = 0; tx < 64; tx++) {
                    double a[NV] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    for (int j = by * 4 + ty; j < B.v.ny; j += gy * 4)
                        for (int i = bx * 64 + tx; i < B.v.nx; i += gx * 64)
                            mb_fold(B.v, B.c[0].data(), B.c[1].data(), B.c[2].data(), B.c[3].data(), B.c[4].data(), i, j, a);
                    for (int q = 0; q < NV; q++) sm[ty * 64 + tx][q] = a[q];
                }
                block_tree(sm);
                for (int q = 0; q < NV; q++) list.push_back(sm[0][q]);
            }
        second_stage(list, &out[(size_t)NV * l]);
    }
    fclose(f);
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), 8, out.size(), g) != out.size()) return 2;
    fclose(g);
    return 0;
}
