// suhmo_transfer.h -- the rules that move data between AMR levels, each stated ONCE as arithmetic on values: no view, no field table, no pointer
// into a canvas or into LDS, no HIP type.  Every kernel that applies a rule loads its operands, calls the function and stores the result; the
// indexing, the plan decoding and the decision which neighbours exist stay with the kernel.  The oracle states the same arithmetic with the
// same association of operands (oracle/amrm.c, oracle/amr_step_m.c); parity is bitwise, so the ORDER of the operations below is part of the rule.
//
// Restated from upstream Chombo's documented semantics because the fork is not vendored (UNPINNED): QuadCFInterp,
// PiecewiseLinearFillPatch / FineInterp, FORT_AVERAGE, CoarseAverageFace, LevelFluxRegister.  From the reference's own source: PROLONG_2_NL and
// the ghosted coarse copy of AMRProlongS_2.
//
// Plain C++ once __device__ and __forceinline__ are defined away (tests/host_cpp/transfer_rules.cpp, tests/host_cpp/flatten_emu.cpp).
#pragma once
#include <math.h>

// ---- [Chombo] QuadCFInterp::coarseFineInterp, ratio 2 (oracle/amrm.c:cf_interp): a tangential quadratic on the coarse level through the coarse
// cell c0 under the ghost cell, then a normal quadratic through that value and the two fine cells inside.
// The tangential stencil by which coarse neighbours exist (next to a non-periodic domain side, or where the level below ends): a, b, c are the
// stencil's cells in the order of the table; returns c0, sets the first and second difference
//   kind            a    b     c
//   CF_CENTRED      c-1  c0    c+1
//   CF_HI2          c0   c+1   c+2      one-sided, 2nd order
//   CF_HI1          c0   c+1   -        one-sided, 1st order (no c+2)
//   CF_LO2          c0   c-1   c-2
//   CF_LO1          c0   c-1   -
//   CF_NONE         c0   -     -
enum { CF_CENTRED = 0, CF_HI2 = 1, CF_HI1 = 2, CF_LO2 = 3, CF_LO1 = 4, CF_NONE = 5 };
__device__ __forceinline__ double cf_tangential(int kind, double a, double b, double c, double &d1, double &d2)
{
    d1 = 0.0; d2 = 0.0;
    if (kind == CF_CENTRED) { d1 = 0.5 * (c - a); d2 = c - 2.0 * b + a; return b; }
    if (kind == CF_HI2) { d1 = 0.5 * (-3.0 * a + 4.0 * b - c); d2 = a - 2.0 * b + c; }
    else if (kind == CF_HI1) d1 = b - a;
    else if (kind == CF_LO2) { d1 = 0.5 * (3.0 * a - 4.0 * b + c); d2 = a - 2.0 * b + c; }
    else if (kind == CF_LO1) d1 = a - b;
    return a;
}
// ghost = 8/15 phistar + 2/3 near - 1/5 far; xt = +-1/4: the tangential offset of the fine cell centre in coarse cells; nearv, farv: the first
// and second fine cell inside
__device__ __forceinline__ double cf_ghost(double c0, double d1, double d2, double xt, double nearv, double farv)
{
    const double c_s = 8.0 / 15.0, c_b = 2.0 / 3.0, c_a = -0.2;
    double phistar = c0 + xt * d1 + (0.5 * xt * xt) * d2;
    return c_s * phistar + c_b * nearv + c_a * farv;
}

// ---- [Chombo] PiecewiseLinearFillPatch::fillInterp (oracle/amr_step_m.c:or_pwl_fill) and FineInterp::interpToFine with m_boundary_limit_type =
// limitTangentialOnly (include/suhmo_hip.h, "REGRID: FIELD TRANSFER" rule (a); tests/regrid_ref.py:limited_slopes is the numpy twin).
// nb[b][a]: the 3 x 3 coarse block (b: y, a: x, nb[1][1] the cell); xl, xh, yl, yh: the neighbour below / above in x / y exists (a corner exists
// where both its row and its column do; what nb holds for a missing cell is not read).  Slopes: central, one-sided where one neighbour is
// missing, 0 where both are; FORT_INTERPLIMIT: eta from the extrema of the existing cells of the block, i fastest.
// tangential_only: FineInterp -- a one-sided slope (normal to a domain side) stays as computed; false: the fill -- both slopes always limited
__device__ __forceinline__ void limited_slopes(const double nb[3][3], bool xl, bool xh, bool yl, bool yh, bool tangential_only, double &s0, double &s1)
{
    const double c0 = nb[1][1];
    const bool ex[3] = {xl, true, xh}, ey[3] = {yl, true, yh};
    s0 = 0.0; s1 = 0.0;
    if (xl && xh) s0 = 0.5 * (nb[1][2] - nb[1][0]); else if (xh) s0 = nb[1][2] - c0; else if (xl) s0 = c0 - nb[1][0];
    if (yl && yh) s1 = 0.5 * (nb[2][1] - nb[0][1]); else if (yh) s1 = nb[2][1] - c0; else if (yl) s1 = c0 - nb[0][1];
    double smax = c0, smin = c0;
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(ex[a] && ey[b])) continue;
            const double v = nb[b][a];
            smax = fmax(smax, v); smin = fmin(smin, v);
        }
    const double deltasum = 0.5 * (fabs(s0) + fabs(s1));
    if (deltasum > 0.0) {
        const double etamax = (smax - c0) / deltasum, etamin = (c0 - smin) / deltasum;
        const double eta = fmax(fmin(fmin(etamin, etamax), 1.0), 0.0);
        if (!tangential_only || (xl && xh)) s0 = eta * s0;
        if (!tangential_only || (yl && yh)) s1 = eta * s1;
    }
}
// coarse value + slope x offset of the child's centre in coarse cells (+-1/4 at ratio 2; -1/2 + (p + 1/2) / r at ratio r): x first, then y
__device__ __forceinline__ double child_value(double c0, double s0, double s1, double ox, double oy)
{
    double v = c0;
    v = v + s0 * ox;
    v = v + s1 * oy;
    return v;
}

// ---- [Chombo] FORT_AVERAGE: covered coarse cell = (sum of its 4 fine cells, i fastest: (0,0) (1,0) (0,1) (1,1)) * 1/4
__device__ __forceinline__ double avg4(double a, double b, double c, double d)
{
    double s = 0.0;
    s = s + a; s = s + b; s = s + c; s = s + d;
    return s * 0.25;
}
// [Chombo] CoarseAverageFace with the AMR ratio (VCAMRNonLinearPoissonOp::finerOperatorChanged :1356-1439): coarse face = (sum of its 2 fine faces) / 2
__device__ __forceinline__ double avg2(double a, double b)
{
    double sm = 0.0;
    sm = sm + a; sm = sm + b;
    return sm / 2.0;
}

// ---- PROLONG_2_NL (src/AMRNonLinearPoissonOpF.ChF:660-705): p: the fine value; c: its coarse cell; cx, cy: the coarse neighbour on the fine
// cell's side in x / in y; cd: the diagonal one.  9/16, 3/16, 3/16, 1/16
__device__ __forceinline__ double prolong2_nl(double p, double c, double cx, double cy, double cd)
{
    const double den = 1.0 / 16.0, fx1 = 3.0 * den, fx2 = 9.0 * den, f0 = 1.0 * den;
    p = p + fx2 * c + f0 * cd;
    p = p + fx1 * (cx + cy);
    return p;
}
// physical BC of the coarse level on a ghost cell of the prolongation's coarse copy (m_bc on a_temp, AMRProlongS_2 :1160-1166): Dirichlet
// (bct == 0, two_v = 2 x the boundary value) or Neumann (neu = the gradient x the spacing, outward); nearv: the first cell inside
__device__ __forceinline__ double bc_ghost(int bct, double two_v, double neu, double nearv)
{
    return bct == 0 ? two_v - nearv : nearv + neu;
}

// ---- [Chombo] LevelFluxRegister (oracle/amrm.c:reflux): on a coarse-fine face the coarse flux is replaced by the average of the two fine
// fluxes; L(phi) of the coarse cell outside the fine level += sign * reg / (dx dy).  Fluxes as VCAMRNonLinearPoissonOp::getFlux (:792-841):
// F = -bCoef * ((phi_hi - phi_lo) * beta * ratio / dx); tsize: the face's length; cs = beta / dx, fs = 2 beta / dx of the coarse level.
// The register after the coarse flux (incrementCoarse, scale -1) ...
__device__ __forceinline__ double reflux_coarse(double tsize, double bc, double phihi, double philo, double cs)
{
    double Fc = -bc * ((phihi - philo) * cs);
    return -(tsize * Fc);
}
// ... and after one of the two fine fluxes (incrementFine, scale 1/2)
__device__ __forceinline__ double reflux_add_fine(double reg, double tsize, double bf, double ph_hi, double ph_lo, double fs)
{
    double Ff = -bf * ((ph_hi - ph_lo) * fs);
    return reg + (tsize * Ff) * 0.5;
}
// the cell's value with one face's register added: sign = +1 on the low side of the fine level, -1 on the high side; rscale = 1 / (dx dy)
__device__ __forceinline__ double reflux_apply(double acc, double sign, double rscale, double reg)
{
    return acc + sign * rscale * reg;
}
// the residual form: acc is L(phi) with every register added; the cell gets rhs - that, what copy -> reflux -> axby(-1, 1) leaves there
__device__ __forceinline__ double reflux_residual(double acc, double rhs)
{
    return -1.0 * acc + 1.0 * rhs;
}
