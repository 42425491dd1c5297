// suhmo_balance.h -- the per-face and per-cell rule of "MASS BALANCE" (include/suhmo_hip.h), stated ONCE as arithmetic on values and canvases:
// AmrHydro::check_fluxes (src/AmrHydro.cpp:440-590) statement by statement.  Division by the spacing as the reference has it (not a product
// with fdx), nothing contracted (-ffp-contract=off), every value its own accumulator.  tests/massbalance_ref.py restates it in numpy: change one,
// change the other.
//   face     gradphi = (phihi - philo) * (-1.0) / h;  flux = -K * gradphi;  t = flux * area                                     (:497-498)
//            mec as bcoef_face forms it: +-1 where |mhi - mlo| < 1e-10, else 0, and 0 on both domain faces        (HydroIBC.cpp:139-184)
//            where |mec| < 1e-10, with d = mhi - mlo:  d > 0: dir += t;  d < 0: dir -= t;  d == 0 and mhi > 0: += on the low domain
//            face, -= on the high one                                                                                               (:503-517)
//            independently: lo += t on the low domain face, hi += t on the high one -- periodic or not                              (:522-526)
//   cell     mask > 0: vol += B * dx * dy, multiplied left to right                                                                  (:534-535)
//   fold     what the thread of cell (i, j) adds, in this order: its low x-face; its high x-face if i == nx - 1; its low y-face; its high
//            y-face if j == ny - 1; its volume term.  So every face of a box is folded exactly once BY THAT BOX: a face on a side two boxes
//            share is folded by both, as the reference's walk over thisFluxes_dir.box() of every box does.
// The head beside a face is what phiW / phiE / phiS / phiN (suhmo_common.h) return with homog = false: the neighbour inside the box, the stored
// ghost on a box or coarse-fine side, the wrap on a periodic side, the mixBCValues ghost on a physical side (the reference fills m_head's ghost
// cells with exactly that after the last solve of the Picard loop, :3157-3164).  The mask is read from the canvas as stored, ghost cells included.
// K of the high domain face lies in the canvas column right of (row above) the last cell.
//
// Plain C++ once __device__ and __forceinline__ are defined away and DV, cidx, phiW, phiE, phiS, phiN and the SUHMO_MB_* numbers exist
// (tests/host_cpp/balance_emu.cpp).
#pragma once
#include <math.h>

// one face: h the spacing across it, area the length along it, at_lo / at_hi: it is the low / high face of the DOMAIN in its direction
__device__ __forceinline__ void mb_face(double phihi, double philo, double K, double mhi, double mlo, double h, double area, bool at_lo, bool at_hi,
                                        double &lo, double &hi, double &dir)
{
    const double gradphi = (phihi - philo) * (-1.0) / h;
    const double flux = -K * gradphi;
    const double t = flux * area;
    const double d = mhi - mlo;
    double mec = fabs(d) < 1e-10 ? ((mhi > 0.0) ? 1.0 : -1.0) : 0.0;
    mec = (at_lo || at_hi) ? 0.0 : mec;
    // the reference's chain of ifs (:503-517) as two tests, so that a face costs selects and no branch: `up` where it adds, `down` where it subtracts
    const bool on = fabs(mec) < 1.0e-10, pos = d > 0.0, neg = !pos && d < 0.0, edge = !pos && !neg && mhi > 0.0;
    const bool up = on && (pos || (edge && at_lo)), down = on && (neg || (edge && !at_lo && at_hi));
    dir = up ? dir + t : (down ? dir - t : dir);
    lo = at_lo ? lo + t : lo;
    hi = (!at_lo && at_hi) ? hi + t : hi;
}
__device__ __forceinline__ void mb_cell(double mask, double B, double dx, double dy, double &vol)
{
    vol = mask > 0.0 ? vol + B * dx * dy : vol;
}
// cell (i, j) of the box with view v: head, mask, B, bx, by its canvases; a[0 .. SUHMO_MB_COUNT - 1] the thread's seven values (N > SUHMO_MB_COUNT:
// the water budget's accumulators, whose first seven are these)
template <int N> __device__ __forceinline__ void mb_fold(const DV &v, const double *__restrict__ head, const double *__restrict__ mask, const double *__restrict__ B,
                                                         const double *__restrict__ bx, const double *__restrict__ by, int i, int j, double (&a)[N])
{
    static_assert(N >= SUHMO_MB_COUNT, "the seven values of the mass balance come first");
    const int idx = cidx(v, i, j);
    const int I = v.i0 + i, J = v.j0 + j;
    const double c = head[idx], m = mask[idx];
    mb_face(c, phiW(v, head, idx, i, c, false), bx[idx], m, mask[idx - 1], v.dx, v.dy, I == 0, I == v.nxg,
            a[SUHMO_MB_LO_X], a[SUHMO_MB_HI_X], a[SUHMO_MB_DIR_X]);
    if (i == v.nx - 1)
        mb_face(phiE(v, head, idx, i, c, false), c, bx[idx + 1], mask[idx + 1], m, v.dx, v.dy, I + 1 == 0, I + 1 == v.nxg,
                a[SUHMO_MB_LO_X], a[SUHMO_MB_HI_X], a[SUHMO_MB_DIR_X]);
    mb_face(c, phiS(v, head, idx, j, c, false), by[idx], m, mask[idx - v.P], v.dy, v.dx, J == 0, J == v.nyg,
            a[SUHMO_MB_LO_Y], a[SUHMO_MB_HI_Y], a[SUHMO_MB_DIR_Y]);
    if (j == v.ny - 1)
        mb_face(phiN(v, head, idx, j, c, false), c, by[idx + v.P], mask[idx + v.P], m, v.dy, v.dx, J + 1 == 0, J + 1 == v.nyg,
                a[SUHMO_MB_LO_Y], a[SUHMO_MB_HI_Y], a[SUHMO_MB_DIR_Y]);
    mb_cell(m, B[idx], v.dx, v.dy, a[SUHMO_MB_VOLUME]);
}

// ---- "WATER BUDGET" (include/suhmo_hip.h): what a first stage of the budget leaves per workgroup -- the seven values above, then the two parts of
// the reference's rechargeTOT (src/AmrHydro.cpp:3766-3773) as d_postproc_columns (suhmo_postproc.hip) forms them per cell, statement by statement
enum { WB_P_EXT = SUHMO_MB_COUNT, WB_P_MELT, WB_P_COUNT };
// ms: SUHMO_F_MSRC where the model has a moulin source (use_moulin_source), else NULL; mr: SUHMO_F_MR
__device__ __forceinline__ void wb_cell(double mask, const double *__restrict__ ms, const double *__restrict__ mr, int idx, double ramp, double distributed_input,
                                        double rho_w, double dx, double dy, double &ext, double &melt)
{
    const bool ice = mask > 0.0;
    const double src = ms ? ms[idx] * ramp + distributed_input : (ice ? distributed_input : 0.0);
    ext = ice ? ext + src * dy * dx : ext;
    melt = ice ? melt + (mr[idx] / rho_w) * dy * dx : melt;
}
// mb_fold of the cell, then its two recharge terms: after the volume term, each into its own accumulator
__device__ __forceinline__ void wb_fold(const DV &v, const double *__restrict__ head, const double *__restrict__ mask, const double *__restrict__ B,
                                        const double *__restrict__ bx, const double *__restrict__ by, const double *__restrict__ mr, const double *__restrict__ ms,
                                        double ramp, double distributed_input, double rho_w, int i, int j, double (&a)[WB_P_COUNT])
{
    mb_fold(v, head, mask, B, bx, by, i, j, a);
    const int idx = cidx(v, i, j);
    wb_cell(mask[idx], ms, mr, idx, ramp, distributed_input, rho_w, v.dx, v.dy, a[WB_P_EXT], a[WB_P_MELT]);
}
