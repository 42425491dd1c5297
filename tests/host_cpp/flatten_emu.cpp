// flatten_emu.cpp -- k_flat_interp (suhmo_amd/csrc/suhmo_flatten.hip) run on the HOST: the kernel's text, cut out of the .hip file by
// tests/test_flatten_cpu.py into FLATTEN_KERNEL_INC, compiled as plain C++ (blockIdx / threadIdx are variables, the launch is a loop over the
// grid) with -ffp-contract=off and the address and undefined-behaviour sanitizers.  The canvases are heap blocks of exactly the library's size,
// so an access outside one is reported.  CPU only; needs no device.
//   flatten_emu IN OUT CAP     IN: 7 ints (nx0 ny0 perx pery nlev max_level ncomp), per level nbox, per box 7 ints (nx ny i0 j0 P gy elems) and
//                              ncomp canvases of elems doubles; OUT: ncomp x nyF x nxF doubles; CAP: the cap on the workgroups of a launch
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#define SUHMO_XOFF 16
#define SUHMO_F_COUNT 33
struct DV { int nx, ny, P, gy, rows, j0, nyg; double dx, dy, rdx, rdy, fdx, fdy, alpha, beta; int bct[2][2]; double two_v[2][2], neu[2][2]; int per[2], ext[2], i0, nxg, cfx[2], rk[2]; };
struct FP { double *f[SUHMO_F_COUNT]; };
static inline int cidx(const DV &v, int i, int j) { return (j + v.gy) * v.P + SUHMO_XOFF + i; }
struct d3 { unsigned x, y, z; };
static d3 blockIdx, blockDim, threadIdx, gridDim;
struct double2 { double x, y; };
static inline double2 make_double2(double a, double b) { return double2{a, b}; }
#define __global__
#define __launch_bounds__(x)
#define __device__
#define __forceinline__ inline
#include "../../suhmo_amd/csrc/suhmo_transfer.h"         // the rule the kernel calls: limited_slopes, child_value
#include FLATTEN_KERNEL_INC
// input file: ints: nxd0 nyd0 perx pery nlev max_level ncomp; per level: nbox; per box: nx ny i0 j0 P gy elems then ncomp canvases
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int h[7]; if (fread(h, 4, 7, f) != 7) return 2;
    int nx0 = h[0], ny0 = h[1], perx = h[2], pery = h[3], nlev = h[4], ml = h[5], nc = h[6];
    long nxF = (long)nx0 << ml, nyF = (long)ny0 << ml, plane = nxF * nyF;
    std::vector<double> out(nc * plane, NAN);
    for (int l = 0; l < nlev; l++) {
        int nb; if (fread(&nb, 4, 1, f) != 1) return 2;
        std::vector<DV> dv(nb); std::vector<FP> fp(nb); std::vector<std::vector<double>> store;
        int mx = 0, my = 0;
        for (int k = 0; k < nb; k++) {
            int q[7]; if (fread(q, 4, 7, f) != 7) return 2;
            DV v{}; v.nx = q[0]; v.ny = q[1]; v.i0 = q[2]; v.j0 = q[3]; v.P = q[4]; v.gy = q[5];
            dv[k] = v; mx = std::max(mx, v.nx); my = std::max(my, v.ny);
            for (int t = 0; t < nc; t++) { store.emplace_back(q[6]); if (fread(store.back().data(), 8, q[6], f) != (size_t)q[6]) return 2; }
        }
        { size_t s = 0; for (int k = 0; k < nb; k++) for (int t = 0; t < nc; t++) fp[k].f[t] = store[s++].data(); }
        int sh = ml - l; bool ub = l == 0;
        long tx = sh ? ((long)mx << sh) / 2 : mx, ty = (long)my << sh;
        unsigned gx = (unsigned)((tx + 63) / 64);
        long gy_all = (ty + 3) / 4, gy_cap = std::max(1L, (long)atoi(argv[3]) / ((long)gx * nb));
        gridDim = d3{gx, (unsigned)std::min(gy_all, std::min(gy_cap, 65535L)), (unsigned)nb}; blockDim = d3{64, 4, 1};
        for (unsigned bz = 0; bz < gridDim.z; bz++) for (unsigned by = 0; by < gridDim.y; by++) for (unsigned bx = 0; bx < gridDim.x; bx++)
            for (unsigned ty_ = 0; ty_ < 4; ty_++) for (unsigned tx_ = 0; tx_ < 64; tx_++) {
                blockIdx = d3{bx, by, bz}; threadIdx = d3{tx_, ty_, 0};
                if (sh) k_flat_interp<false>(ub ? nullptr : dv.data(), ub ? nullptr : fp.data(), ub ? dv[0] : DV{}, ub ? fp[0] : FP{}, ub, sh, nx0 << l, ny0 << l, perx, pery, nc, nxF, plane, out.data());
                else k_flat_interp<true>(ub ? nullptr : dv.data(), ub ? nullptr : fp.data(), ub ? dv[0] : DV{}, ub ? fp[0] : FP{}, ub, sh, nx0 << l, ny0 << l, perx, pery, nc, nxF, plane, out.data());
            }
    }
    FILE *g = fopen(argv[2], "wb"); fwrite(out.data(), 8, out.size(), g); fclose(g);
    return 0;
}
