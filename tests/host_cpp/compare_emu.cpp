// compare_emu.cpp -- the per-cell rule of "COMPARE" (suhmo_amd/csrc/suhmo_compare.h: cmp_cell and what it calls) run on the HOST over whole
// hierarchies, compiled as plain C++ with -ffp-contract=off and the address and undefined-behaviour sanitizers (tests/test_compare_cpu.py).  The
// canvases are heap blocks of exactly the library's size, so an access outside one is reported; the sums are taken in the order of
// suhmo_amd/csrc/suhmo_reduce.h, restated here as loops (the walk, the block tree, the second stage), so that the output is compared bit for bit
// with tests/compare_ref.py.  CPU only; needs no device.
//   compare_emu IN OUT     IN: 3 ints (nlev exact_level diff); the exact level: 5 ints (nx ny P gy elems) and 1 + diff canvases; per level: 1 int
//                          (nbox), 1 double (w), per box 7 ints (nx ny i0 j0 P gy elems) and 2 + diff canvases (a, [b], cover)
//                          OUT: 3 doubles (L1, L2, max), then nlev x 3 (each level's own sum1, sum2, max)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define SUHMO_XOFF 16
struct DV { int nx, ny, P, gy, i0, j0; };
static inline int cidx(const DV &v, int i, int j) { return (j + v.gy) * v.P + SUHMO_XOFF + i; }
#define __device__
#define __forceinline__ inline
#define __restrict__
#include "../../suhmo_amd/csrc/suhmo_compare.h"

static double op(int q, double a, double b) { return q == 2 ? std::fmax(a, b) : a + b; }
static void block_tree(double (*sm)[3])                     // sm[256][3] -> sm[0]
{
    for (int s = 128; s > 0; s >>= 1)
        for (int tid = 0; tid < s; tid++)
            for (int q = 0; q < 3; q++) sm[tid][q] = op(q, sm[tid][q], sm[tid + s][q]);
}
static void second_stage(const std::vector<const std::vector<double> *> &lists, double *out)
{
    static double a[256][3];
    for (int t = 0; t < 256; t++) for (int q = 0; q < 3; q++) a[t][q] = 0.0;
    for (const std::vector<double> *p : lists)
        for (int t = 0; t < 256; t++)
            for (size_t k = t; k < p->size() / 3; k += 256)
                for (int q = 0; q < 3; q++) a[t][q] = op(q, a[t][q], (*p)[3 * k + q]);
    block_tree(a);
    for (int q = 0; q < 3; q++) out[q] = a[0][q];
}
struct Box { DV v; std::vector<double> a, b, cover; };
static bool rd(FILE *f, void *p, size_t sz, size_t n) { return fread(p, sz, n, f) == n; }
static bool canvas(FILE *f, std::vector<double> &c, int elems) { c.resize(elems); return rd(f, c.data(), 8, elems); }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[3]; if (!rd(f, h, 4, 3)) return 2;
    const int nlev = h[0], el = h[1]; const bool diff = h[2] != 0;
    int x[5]; if (!rd(f, x, 4, 5)) return 2;
    DV xv{x[0], x[1], x[2], x[3], 0, 0};
    std::vector<double> xa, xb;
    if (!canvas(f, xa, x[4]) || (diff && !canvas(f, xb, x[4]))) return 2;
    std::vector<std::vector<double>> lists(nlev);
    std::vector<double> out(3 + 3 * nlev);
    for (int l = 0; l < nlev; l++) {
        int nb; double w;
        if (!rd(f, &nb, 4, 1) || !rd(f, &w, 8, 1)) return 2;
        std::vector<Box> box(nb);
        int mx = 0, my = 0;
        for (Box &B : box) {
            int q[7]; if (!rd(f, q, 4, 7)) return 2;
            B.v = DV{q[0], q[1], q[4], q[5], q[2], q[3]};
            if (!canvas(f, B.a, q[6]) || (diff && !canvas(f, B.b, q[6])) || !canvas(f, B.cover, q[6])) return 2;
            mx = std::max(mx, B.v.nx); my = std::max(my, B.v.ny);
        }
        const int capx = l == 0 ? 32 : 4, capy = l == 0 ? 128 : 16;                // CAP_LEVEL, CAP_BOX
        const int gx = std::min((mx + 63) / 64, capx), gy = std::min((my + 3) / 4, capy);
        for (const Box &B : box)
            for (int by = 0; by < gy; by++) for (int bx = 0; bx < gx; bx++) {
                static double sm[256][3];
                for (int ty = 0; ty < 4; ty++) for (int tx = 0; tx < 64; tx++) {
                    double a[3] = {0.0, 0.0, 0.0};
                    for (int j = by * 4 + ty; j < B.v.ny; j += gy * 4)
                        for (int i = bx * 64 + tx; i < B.v.nx; i += gx * 64)
                            cmp_cell(B.v, i, j, diff, B.a.data(), diff ? B.b.data() : nullptr, B.cover.data(), xv, xa.data(), diff ? xb.data() : nullptr, el - l, w, a);
                    for (int q = 0; q < 3; q++) sm[ty * 64 + tx][q] = a[q];
                }
                block_tree(sm);
                for (int q = 0; q < 3; q++) lists[l].push_back(sm[0][q]);
            }
        second_stage({&lists[l]}, &out[3 + 3 * l]);
    }
    std::vector<const std::vector<double> *> all;
    for (const std::vector<double> &p : lists) all.push_back(&p);
    second_stage(all, out.data());
    out[1] = std::sqrt(out[1]);
    fclose(f);
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), 8, out.size(), g) != out.size()) return 2;
    fclose(g);
    return 0;
}
