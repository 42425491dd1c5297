// suhmo_postproc.hip -- the diagnostics of a level after a time step (suhmo_step.hip): the SHMIP cross-section table ("POST PROC -- 1 LEVEL",
// src/AmrHydro.cpp:3643-3810) as column sums on the device, and from them the table, the "Time(h - d)" lines of the temporal post-processing
// (:4040-4053) on the host or -- one row of a run's series, suhmo_run.hip / suhmo_batch.hip -- on the device.
#include "suhmo_hier_int.h"
#include "suhmo_batch.h"
#include <cmath>

using namespace hier;

// ------------------------------------------------------------------ SHMIP cross-section table
// one thread per cell column, rows summed in ascending j (the order of the reference's BoxIterator per column)
__device__ __forceinline__ void d_postproc_columns(const DV &v, const FP &fp, const suhmo_model_params_t &mp, double *__restrict__ out /* 8 x nx */)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.nx) return;
    const double *__restrict__ qx = fp.f[SUHMO_F_QWX], *__restrict__ cd = fp.f[SUHMO_F_CD], *__restrict__ mR = fp.f[SUHMO_F_MR];
    const double *__restrict__ Pw = fp.f[SUHMO_F_PW], *__restrict__ Pi = fp.f[SUHMO_F_PI], *__restrict__ mk = fp.f[SUHMO_F_MASK];
    const double *__restrict__ ms = mp.use_moulin_source ? fp.f[SUHMO_F_MSRC] : nullptr;
    double qt = 0.0, qc = 0.0, qd = 0.0, ext = 0.0, mr = 0.0, yl = 0.0, avp = 0.0, cnt = 0.0;
    for (int j = 0; j < v.ny; j++) {
        int idx = cidx(v, i, j);
        double cdec = 0.5 * (cd[idx] + cd[idx - 1]);                     // CellToEdge(chanDegree), :3696-3697
        double q = qx[idx] * v.dy;
        qt += q; qc += q * cdec; qd += q * (1.0 - cdec);                 // :3734-3738
        bool ice = mk[idx] > 0.0;
        double src = ms ? ms[idx] * mp.ramp + mp.distributed_input : (ice ? mp.distributed_input : 0.0);
        if (ice) { ext += src * v.dy * v.dx; mr += (mR[idx] / mp.rho_w) * v.dy * v.dx; yl += v.dy; }    // :3766-3775
        if (ice && Pi[idx] > 0.0) { avp += Pi[idx] - Pw[idx]; cnt += 1.0; }                             // :3778-3783
    }
    out[0 * v.nx + i] = yl; out[1 * v.nx + i] = qt; out[2 * v.nx + i] = qc; out[3 * v.nx + i] = qd;
    out[4 * v.nx + i] = ext; out[5 * v.nx + i] = mr; out[6 * v.nx + i] = avp; out[7 * v.nx + i] = cnt;
}
// out: 8 x nx of a level; of an ensemble [n][8][nx], the rows of the members the launch serves
template <class T> __global__ void k_postproc_columns(T t, double *__restrict__ out)
{
    d_postproc_columns(t.view(), t.fields(), t.model(), out + t.slot(8 * (size_t)t.view().nx));
}
template <class T> static int launch_postproc_columns_(const T &t, double *out, hipStream_t st)
{
    return launch_grid(k_postproc_columns<T>, t, dim3((t.nx() + 63) / 64), dim3(64), st, out);
}
int launch_postproc_columns(const OnMembers &t, double *out, hipStream_t st) { return launch_postproc_columns_(t, out, st); }
// ---- what the entry points below refuse, each check once, in the order every one of them reports
static int refuse_patch(const suhmo_level *L)
{
    if (L->desc.nx_global > 0) { suhmo_set_error("post-processing table on an AMR patch is not built"); return -5; }
    return 0;
}
static int refuse_no_source(const suhmo_level *L, const suhmo_model_params_t *mp)
{
    if (mp->use_moulin_source && !L->d[0].fp.f[SUHMO_F_MSRC]) { suhmo_set_error("use_moulin_source without suhmo_level_moulin_source"); return -1; }
    return 0;
}
// the fields the column sums read: what a time step leaves, and the source term where the model has one
static int check_fields(const suhmo_level *L, const suhmo_model_params_t *mp)
{
    for (int f : {SUHMO_F_QWX, SUHMO_F_CD, SUHMO_F_MR, SUHMO_F_PW}) if (!L->d[0].fp.f[f]) { suhmo_set_error("no time step has run on this level"); return -1; }
    return refuse_no_source(L, mp);
}
// the daily row is that of a whole level (the strips of a level add their column sums on the host) of two columns or more
static int check_row_geometry(const suhmo_level *L)
{
    const DV &v = L->d[0].v;
    int rc = refuse_patch(L); if (rc) return rc;
    if (v.ext[0] || v.ext[1]) { suhmo_set_error("rank strip: add the strips' suhmo_level_postproc_partial sums, then suhmo_postproc_temporal"); return -5; }
    if (v.nx < 2) { suhmo_set_error("temporal post-processing needs at least two columns"); return -1; }
    return 0;
}
// column sums over the rows of this level / strip: 8 x nx = width, Q, Q channelised, Q distributed, external recharge,
// melt recharge, sum of (Pi - Pw), count of its terms
extern "C" int suhmo_level_postproc_partial(suhmo_level_t *L, const suhmo_model_params_t *mp, double *sums, suhmo_stream_t s)
{
    ARG(L && mp && sums);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    int rc;
    if ((rc = refuse_patch(L)) || (rc = check_fields(L, mp))) return rc;
    const int nx = L->d[0].v.nx;
    double *dev = nullptr;
    HIPCHK(hipMalloc(&dev, 8 * (size_t)nx * sizeof(double)));
    rc = launch_postproc_columns_(stepping(on_level(L, 0), *mp), dev, st);
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(sums, dev, 8 * (size_t)nx * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) { suhmo_set_error("postproc table: %s", hipGetErrorString(e)); return -2; }
    return 0;
}
// the table from column sums (of the whole level: on rank strips the host adds the strips' sums first)
extern "C" int suhmo_postproc_finish(const double *sums, int nx, double dx, double *table)
{
    ARG(sums && table && nx > 0);
    const double *h = sums;
    double cext = 0.0, cmr = 0.0;
    for (int i = nx - 1; i >= 0; i--) {                    // recharge upstream of the column: cumulative from the upper end
        cext += h[4 * (size_t)nx + i]; cmr += h[5 * (size_t)nx + i];
        double *row = table + 8 * (size_t)i;
        row[0] = (i + 0.5) * dx / 1.0e3; row[1] = h[0 * (size_t)nx + i];
        row[2] = -h[1 * (size_t)nx + i]; row[3] = -h[2 * (size_t)nx + i]; row[4] = -h[3 * (size_t)nx + i];
        row[5] = cext; row[6] = cmr; row[7] = h[6 * (size_t)nx + i] / fmax(h[7 * (size_t)nx + i], 1.0) / 1.0e6;
    }
    return 0;
}
// the "Time(h - d)" lines of the temporal post-processing (src/AmrHydro.cpp:3778-3810, 4040-4053) from the column sums
extern "C" int suhmo_postproc_temporal(const double *sums, int nx, double dx, double *out)
{
    ARG(sums && out && nx > 1);
    const double *h = sums;
    const double lo[3] = {600.0, 3000.0, 5100.0}, hi[3] = {900.0, 3300.0, 5400.0};
    double tot = 0.0, cnt = 0.0, bs[3] = {0.0, 0.0, 0.0}, bc[3] = {0.0, 0.0, 0.0}, rech = 0.0;
    for (int i = 0; i < nx; i++) {
        const double x = (i + 0.5) * dx;
        tot += h[6 * (size_t)nx + i]; cnt += h[7 * (size_t)nx + i];
        for (int b = 0; b < 3; b++) if (x > lo[b] && x < hi[b]) { bs[b] += h[6 * (size_t)nx + i]; bc[b] += h[7 * (size_t)nx + i]; }
        if (i >= 1) rech += h[4 * (size_t)nx + i] + h[5 * (size_t)nx + i];
    }
    out[0] = tot / cnt;
    for (int b = 0; b < 3; b++) out[1 + b] = bs[b] / bc[b];
    out[4] = rech;
    out[5] = -h[1 * (size_t)nx + 1];
    return 0;
}
extern "C" int suhmo_level_postproc_temporal(suhmo_level_t *L, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s)
{
    ARG(L && mp && out);
    Depth &D = L->d[0];
    if (D.v.ext[0] || D.v.ext[1]) { suhmo_set_error("rank strip: add the strips' suhmo_level_postproc_partial sums, then suhmo_postproc_temporal"); return -5; }
    std::vector<double> h(8 * (size_t)D.v.nx);
    int rc = suhmo_level_postproc_partial(L, mp, h.data(), s); if (rc) return rc;
    return suhmo_postproc_temporal(h.data(), D.v.nx, D.v.dx, out);
}
// suhmo_postproc_temporal on the device: the six values from column sums that never leave it (a run keeps finished rows, 6 doubles per member,
// instead of 8 nx).  One thread per value, each the host function's loop over the columns in ascending order with its operations -- no tree, so
// the bits are the host's (0 / 0 of an empty band: NaN on both sides)
__device__ __forceinline__ void d_postproc_temporal_row(const DV &v, const double *__restrict__ h /* 8 x nx */, double *__restrict__ out /* 6 */)
{
    const int q = threadIdx.x;
    if (q >= 6) return;
    const size_t nx = v.nx;
    if (q == 0) {
        double tot = 0.0, cnt = 0.0;
        for (size_t i = 0; i < nx; i++) { tot += h[6 * nx + i]; cnt += h[7 * nx + i]; }
        out[0] = tot / cnt;
    } else if (q <= 3) {
        const double lo = q == 1 ? 600.0 : q == 2 ? 3000.0 : 5100.0, hi = q == 1 ? 900.0 : q == 2 ? 3300.0 : 5400.0;
        double bs = 0.0, bc = 0.0;
        for (size_t i = 0; i < nx; i++) {
            const double x = ((int)i + 0.5) * v.dx;
            if (x > lo && x < hi) { bs += h[6 * nx + i]; bc += h[7 * nx + i]; }
        }
        out[q] = bs / bc;
    } else if (q == 4) {
        double rech = 0.0;
        for (size_t i = 1; i < nx; i++) rech += h[4 * nx + i] + h[5 * nx + i];
        out[4] = rech;
    } else out[5] = -h[1 * nx + 1];
}
// cols: 8 x nx of a level, [n][8][nx] of an ensemble; out: 6 values, of an ensemble [n][6] (one row of a series): the entries of the members served
template <class T> __global__ void k_postproc_temporal_row(T t, const double *__restrict__ cols, double *__restrict__ out)
{
    d_postproc_temporal_row(t.view(), cols + t.slot(8 * (size_t)t.view().nx), out + t.slot(6));
}
template <class T> static int launch_postproc_temporal_row_(const T &t, const double *cols, double *out, hipStream_t st)
{
    return launch_grid(k_postproc_temporal_row<T>, t, dim3(1), dim3(64), st, cols, out);
}
int launch_postproc_temporal_row(const OnMembers &t, const double *cols, double *out, hipStream_t st) { return launch_postproc_temporal_row_(t, cols, out, st); }
// the two launches of a row into device memory the caller owns (cols: 8 nx doubles, out6: 6), everything checked
static int launch_row(suhmo_level *L, const suhmo_model_params_t *mp, double *cols, double *out6, hipStream_t st)
{
    int rc = launch_postproc_columns_(stepping(on_level(L, 0), *mp), cols, st);
    return rc ? rc : launch_postproc_temporal_row_(on_level(L, 0), cols, out6, st);
}
// the row of one level for the host: the row's checks, its launches into a block of this call, the six values copied out
extern "C" int suhmo_level_postproc_temporal_device(suhmo_level_t *L, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s)
{
    ARG(L && mp && out);
    HIPCHK(hipSetDevice(L->device));
    hipStream_t st = (hipStream_t)s;
    int rc;
    if ((rc = check_row_geometry(L)) || (rc = check_fields(L, mp))) return rc;
    const size_t ncol = 8 * (size_t)L->d[0].v.nx;
    double *dev = nullptr;
    HIPCHK(hipMalloc(&dev, (ncol + 6) * sizeof(double)));
    rc = launch_row(L, mp, dev, dev + ncol, st);
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(out, dev + ncol, 6 * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) { suhmo_set_error("postproc temporal: %s", hipGetErrorString(e)); return -2; }
    return 0;
}
// the same for a run of a hierarchy (suhmo_run.hip), which writes the rows of its series with no copy and no synchronisation per row: what
// can be refused before the first step (the source term only where no forcing of the run writes it), and per row the fields and the launches
int suhmo_level_postproc_row_check_(suhmo_level *L, const suhmo_model_params_t *mp, bool forcing_writes_source)
{
    int rc = check_row_geometry(L);
    return rc || forcing_writes_source ? rc : refuse_no_source(L, mp);
}
int suhmo_level_postproc_row_launch_(suhmo_level *L, const suhmo_model_params_t *mp, double *cols, double *out6, hipStream_t st)
{
    int rc = check_fields(L, mp);
    return rc ? rc : launch_row(L, mp, cols, out6, st);
}
// the daily row of a hierarchy: the reference evaluates it on level 0 ("POST PROC -- 1 LEVEL", src/AmrHydro.cpp:3643-3700); the finer
// levels enter through what the time step averaged down
extern "C" int suhmo_hier_postproc_temporal(suhmo_hier_t *H, const suhmo_model_params_t *mp, double *out, suhmo_stream_t s)
{
    ARG(H && mp && out);
    if (H->world > 1) { suhmo_set_error("suhmo_hier_postproc_temporal: a hierarchy on rank strips: add the strips' suhmo_level_postproc_partial sums"); return -5; }
    return suhmo_level_postproc_temporal_device(base_of(H), mp, out, s);
}
extern "C" int suhmo_level_postproc_table(suhmo_level_t *L, const suhmo_model_params_t *mp, double *table, suhmo_stream_t s)
{
    ARG(L && mp && table);
    Depth &D = L->d[0];
    if (D.v.ext[0] || D.v.ext[1]) { suhmo_set_error("rank strip: add the strips' suhmo_level_postproc_partial sums, then suhmo_postproc_finish"); return -5; }
    std::vector<double> h(8 * (size_t)D.v.nx);
    int rc = suhmo_level_postproc_partial(L, mp, h.data(), s); if (rc) return rc;
    return suhmo_postproc_finish(h.data(), D.v.nx, D.v.dx, table);
}
