// suhmo_ibc.h -- the reference's initial-condition classes (HydroIBC, SqrtIBC, ValleyIBC, MountainIBC) per cell: the parameter row a launch
// carries and the device functions of one cell.  The formulas, their association and what is left out: include/suhmo_hip.h, "INITIAL
// CONDITIONS"; the launches and the C-ABI: suhmo_ibc.hip.  Every function is one statement per operation of the reference's lines
// (src/HydroIBC.cpp:230-271, src/SqrtIBC.cpp:219-282, src/ValleyIBC.cpp:130-150, 236-336, src/MountainSetupIBC.cpp:89-108, 151-320); the
// library is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include "suhmo_target.h"

// what a launch carries: the caller's values and the constants that do not depend on the cell, formed on the HOST (the C library's bits)
struct IbcRow {
    suhmo_ibc_t p;
    double fact;             // 1 / (rho_w * gravity)
    double sqrt_h;           // sqrt: sqrt(ice_height)
    double pow2e10, h6000;   // valley: pow(2.0e10, 0.25); the surface at x = 6000
    double ca[4], sa[4];     // dino: cos / sin of the four angles
};
static inline IbcRow ibc_row(const suhmo_ibc_t &p)
{
    IbcRow r{};
    r.p = p;
    r.fact = 1. / (p.rho_w * p.gravity);
    r.sqrt_h = std::sqrt(p.ice_height);
    r.pow2e10 = std::pow(2.0e10, 0.25);
    r.h6000 = 100.0 * std::pow(6000. + 200.0, 0.25) + 6000. / 60.0 - r.pow2e10 + 1.0;
    const double angle[4] = {35.0, 90.0, 60.0, 2.0};
    for (int q = 0; q < 4; q++) { r.ca[q] = std::cos(angle[q] * 3.14159 / 180.0); r.sa[q] = std::sin(angle[q] * 3.14159 / 180.0); }
    return r;
}

struct IbcCell { double zb, zs, Pi, b, Pw, h; };
// std::max / std::min as the reference calls them: a NaN in the FIRST argument comes back (sqrt of a ghost cell left of x = -ice_height), where
// fmax / fmin would drop it
__device__ __forceinline__ double ibc_max(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ double ibc_min(double a, double b) { return b < a ? b : a; }

// position of cell (i, j) of the view, i = -1 .. nx, j = -1 .. ny: a cell beyond a periodic side of the level's domain is its image inside
__device__ __forceinline__ void ibc_position(const DV &v, int i, int j, double &x, double &y)
{
    int gi = v.i0 + i, gj = v.j0 + j;
    if (v.per[0]) { if (gi < 0) gi += v.nxg; else if (gi >= v.nxg) gi -= v.nxg; }
    if (v.per[1]) { if (gj < 0) gj += v.nyg; else if (gj >= v.nyg) gj -= v.nyg; }
    x = (gi + 0.5) * v.dx;
    y = (gj + 0.5) * v.dy;
}

// ---- valley: surface, bed and overburden pressure (both ValleyIBC bodies share these lines)
__device__ __forceinline__ void ibc_valley_geometry(const IbcRow &r, double x, double y, double &surf, double &zb, double &Pi)
{
    surf = 100.0 * pow(x + 200.0, 0.25) + x / 60.0 - r.pow2e10 + 1.0;
    const double gamma_b = 0.05;
    const double fx = (r.h6000 - 6000. * r.p.gamma) * x * x / (6000.0 * 6000.0) + r.p.gamma * x;
    const double fx_gb = (r.h6000 - 6000. * gamma_b) * x * x / (6000.0 * 6000.0) + gamma_b * x;
    const double gy = 0.5e-6 * fabs(y * y * y);
    const double hx = (-4.5 * x / 6000. + 5.0) * (surf - fx) / (surf - fx_gb + 1.0e-16);
    zb = fx + gy * hx;
    Pi = r.p.rho_i * r.p.gravity * ibc_max(surf - zb, 0.0);
}
// ---- dino: one Gaussian finger of the bed
__device__ __forceinline__ double ibc_finger(double ca, double sa, double x_bd, double y_bd, double a_max, double s_gauss, int tapered, double sigma)
{
    const double x_tilt = x_bd * ca + y_bd * sa;
    const double y_tilt = -x_bd * sa + y_bd * ca;
    const double a_gauss = a_max * exp(-0.5 / (s_gauss * s_gauss) * y_tilt * y_tilt);
    if (tapered) sigma = 12000.0 - 3000.0 * ibc_min(1.0 - (50000.0 - y_tilt) / 50000.0, 1.0);
    return a_gauss * exp(-0.5 / (sigma * sigma) * x_tilt * x_tilt);
}
__device__ __forceinline__ double ibc_dino_tilt(double x, double y) { return 1.5e-3 * x + -1.5e-3 * y + 100.0; }

// initializeData of one cell
__device__ __forceinline__ IbcCell ibc_initial_cell(const IbcRow &r, const DV &v, int i, int j)
{
    const suhmo_ibc_t &p = r.p;
    double x, y;
    ibc_position(v, i, j, x, y);
    IbcCell c;
    switch (p.kind) {
    case SUHMO_IBC_BASIC:
        c.zb = p.slope * x;
        c.b = p.gap_init;
        c.zs = p.ice_height;
        c.Pi = p.rho_i * p.gravity * c.zs;
        c.Pw = c.Pi * 0.5;
        c.h = c.Pw * r.fact + c.zb;
        break;
    case SUHMO_IBC_SQRT:
        c.zb = p.slope * x;
        c.zs = ibc_max(6.0 * (sqrt(x + p.ice_height) - r.sqrt_h) + 1.0, 0.0);
        c.Pi = ibc_max(p.rho_i * p.gravity * c.zs, 0.0);
        c.b = c.Pi < 2.0 ? 1.0e-16 : p.gap_init;
        c.Pw = 101325;
        c.h = c.Pw * r.fact + c.zb;
        break;
    case SUHMO_IBC_VALLEY: {
        double surf;
        ibc_valley_geometry(r, x, y - 750.0, surf, c.zb, c.Pi);
        c.b = c.Pi < 1.0e-10 ? 1.0e-16 : p.gap_init;
        c.zs = ibc_max(surf - c.zb, 0.0);
        c.Pw = c.Pi * 0.5;
        c.h = c.Pw * r.fact + c.zb;
        if (c.h < 0.0) c.h = 0.0;
        break;
    }
    default: {      // SUHMO_IBC_DINO
        const double tilt = ibc_dino_tilt(x, y);
        const double step_1 = ibc_max(tilt, 0.0);
        c.zs = 2.0 * (tilt + 100.0);
        const double step_2 = ibc_finger(r.ca[0], r.sa[0], x - 100000.00, y - 0.0, 250.0, 50000.0, 1, 0.0);
        const double step_3 = ibc_finger(r.ca[1], r.sa[1], x - 85000.00, y - 0.0, 250.0, 30000.0, 0, 10000.0);
        const double step_4 = ibc_finger(r.ca[2], r.sa[2], x - 55000.00, y - 0.0, 100.0, 20000.0, 0, 5000.0);
        const double step_5 = ibc_finger(r.ca[3], r.sa[3], x - 100000.00, y - 20000.0, 300.0, 35000.0, 0, 6000.0);
        c.zb = step_1 + step_2 + step_3 + step_4 + step_5;
        c.zb = ibc_max(c.zb, 0.0);                          // (the reference adds its unseeded noise inside this max)
        c.Pi = p.rho_i * p.gravity * ibc_max(c.zs, 0.0);
        c.b = c.Pi == 0.0 ? 1.0e-16 : p.gap_init;
        c.Pw = c.Pi * 0.5;
        c.h = c.Pw * r.fact + c.zb;
        if (c.h < 0.0) c.h = 0.0;
        break;
    }
    }
    return c;
}
__device__ __forceinline__ double ibc_mask_of(double Pi) { return Pi > 0.0 ? 1.0 : -1.0; }

// which of ZB, PI, ZS the reload body of a kind writes (host and device)
__host__ __device__ __forceinline__ bool ibc_reload_writes(int kind, int field)
{
    switch (kind) {
    case SUHMO_IBC_BASIC: case SUHMO_IBC_SQRT: return field == SUHMO_F_ZB;
    case SUHMO_IBC_VALLEY: return field == SUHMO_F_ZB || field == SUHMO_F_PI || field == SUHMO_F_ZS;
    default: return field == SUHMO_F_PI || field == SUHMO_F_ZS;
    }
}
// initializeBed + initializePi of one cell at canvas offset idx
__device__ __forceinline__ void ibc_reload_cell(const IbcRow &r, const DV &v, const FP &fp, int i, int j, int idx)
{
    const suhmo_ibc_t &p = r.p;
    double x, y;
    ibc_position(v, i, j, x, y);
    switch (p.kind) {
    case SUHMO_IBC_BASIC: case SUHMO_IBC_SQRT:
        fp.f[SUHMO_F_ZB][idx] = p.slope * x;
        break;
    case SUHMO_IBC_VALLEY: {
        double surf, zb, Pi;
        ibc_valley_geometry(r, x, y - 750.0, surf, zb, Pi);
        fp.f[SUHMO_F_ZS][idx] = surf;
        fp.f[SUHMO_F_ZB][idx] = zb;
        fp.f[SUHMO_F_PI][idx] = Pi;
        break;
    }
    default: {
        const double step_1 = ibc_dino_tilt(x, y) + 100.0;
        const double zs = 2.0 * step_1;
        const double Pi = p.rho_i * p.gravity * ibc_max(zs, 0.0);
        fp.f[SUHMO_F_ZS][idx] = zs;
        fp.f[SUHMO_F_PI][idx] = Pi;
        if (Pi == 0.0) fp.f[SUHMO_F_B][idx] = 1.0e-16;
        break;
    }
    }
}

// ---- suhmo_ibc.hip: the launches the other units need
int suhmo_ibc_check_(const suhmo_ibc_t *ibc, const char *who);                       // rc -1 and a message: NULL, an unknown kind, gap_init <= 0
int launch_ibc_init(const OnMembers &t, const IbcRow *rows, hipStream_t st, int *launched);   // rows: a DEVICE row per member of the batch; *launched: launches made
struct suhmo_hier;
int suhmo_hier_ibc_reload_(suhmo_hier *H, int level, hipStream_t st);                // suhmo_hier_ibc_reload without the entry checks (the regrid's loop)
