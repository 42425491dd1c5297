// suhmo_forcing.hip -- the water input of a time step (suhmo_step.hip), written into SUHMO_F_MSRC: the moulin source term of a level, of
// nested patches, of a hierarchy of box unions and of the members of an ensemble, and the time-varying (seasonal) recharge.
#include "suhmo_hier_int.h"
#include "suhmo_batch.h"
#include "suhmo_reduce.h"
#include <cmath>

using namespace hier;

// ------------------------------------------------------------------ moulin source term
// Calc_moulin_integral / Calc_moulin_source_term_distributed (src/AmrHydro.cpp:1866-2066).  The n x N array of the
// reference (one component per moulin) is never stored: pass 1 integrates every Gaussian (per-tile partial sums in a
// fixed order, then one block per moulin), pass 2 re-evaluates and normalises.  A Gaussian whose argument exceeds
// 760 underflows to exactly 0 in the reference too, so tiles / cells that far away are skipped without changing a bit.
namespace {
__device__ __forceinline__ double moulin_cell(double xc, double yc, double dx, double dy, double mx, double my, double sg, bool &zero)
{
    const double l[3] = {-0.77459666924 / 2.0, 0.0, 0.77459666924 / 2.0};
    const double v[3] = {0.5555555555, 0.8888888888, 0.5555555555};
    const double k = -1.0 / (2.0 * sg * sg), prefac = 1.0 / (sg * sqrt(2.0 * 3.14));
    double ex[3], ey[3];
    for (int q = 0; q < 3; q++) { ex[q] = (xc + l[q]) * dx - mx; ey[q] = (yc + l[q]) * dy - my; }
    double ax = fmin(fabs(ex[0]), fabs(ex[2])), ay = fmin(fabs(ey[0]), fabs(ey[2]));
    if (ex[0] * ex[2] < 0.0) ax = 0.0;
    if (ey[0] * ey[2] < 0.0) ay = 0.0;
    zero = -k * (ax * ax + ay * ay) > 760.0;
    if (zero) return 0.0;
    double MS[9];
    for (int b = 0; b < 3; b++)
        for (int a = 0; a < 3; a++) { double rad = ex[a] * ex[a] + ey[b] * ey[b]; MS[3 * b + a] = prefac * exp(k * rad); }
    return v[0] * v[0] * MS[0] + v[1] * v[0] * MS[1] + v[2] * v[0] * MS[2]
         + v[0] * v[1] * MS[3] + v[1] * v[1] * MS[4] + v[2] * v[1] * MS[5]
         + v[0] * v[2] * MS[6] + v[1] * v[2] * MS[7] + v[2] * v[2] * MS[8];
}
// the three device bodies work on one MoulinJob (suhmo_batch.h): one moulin list on one view.  They are launched over a level, a box or a patch
// (OneMoulinList: the job by value) or over the members of an ensemble (MemberMoulinLists: a device row per member, blockIdx.z -> member)
struct OneMoulinList {
    MoulinJob j;
    __device__ __forceinline__ const MoulinJob &job() const { return j; }
    __device__ __forceinline__ double time_factor() const { return j.tf; }
};
struct MemberMoulinLists {
    const MoulinJob *rows; BatchSel sel;
    __device__ __forceinline__ const MoulinJob &job() const { return rows[batch_member(sel)]; }
    __device__ __forceinline__ double time_factor() const { return job().tf; }
};
// the same rows under the time factors of one step of a run (suhmo_batch_run): by value with the launch, the rows are written once
struct StepMoulinLists : MemberMoulinLists {
    PerMember tf;
    __device__ __forceinline__ double time_factor() const { return tf.x[batch_member(sel)]; }
};
__device__ __forceinline__ void d_moulin_partial(const DV &v, int n, const double *__restrict__ mo, double *__restrict__ partial, const Excl &ex,
                                                 const double *__restrict__ cover)
{
    const int tid = threadIdx.y * 16 + threadIdx.x;
    const int i = blockIdx.x * 16 + threadIdx.x, j = blockIdx.y * 16 + threadIdx.y;
    bool in = i < v.nx && j < v.ny && !(i >= ex.i0 && i < ex.i1 && j >= ex.j0 && j < ex.j1);   // covered by a finer level: 0
    if (in && cover && cover[cidx(v, i, j)] != 0.0) in = false;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const double tx0 = (v.i0 + blockIdx.x * 16) * v.dx, tx1 = (v.i0 + blockIdx.x * 16 + 16) * v.dx;      // the tile in physical coordinates (a patch / box
    const double ty0 = (v.j0 + blockIdx.y * 16) * v.dy, ty1 = (v.j0 + blockIdx.y * 16 + 16) * v.dy;      // starts at (i0, j0) of its level)
    for (int m = 0; m < n; m++) {
        const double mx = mo[3 * m], my = mo[3 * m + 1], sg = mo[3 * m + 2];
        double ddx = mx < tx0 ? tx0 - mx : (mx > tx1 ? mx - tx1 : 0.0), ddy = my < ty0 ? ty0 - my : (my > ty1 ? my - ty1 : 0.0);
        if ((ddx * ddx + ddy * ddy) / (2.0 * sg * sg) > 760.0) { if (tid == 0) partial[(size_t)blk * n + m] = 0.0; continue; }   // uniform
        bool z;
        double val[1] = {in ? moulin_cell(i + 0.5 + v.i0, j + 0.5 + v.j0, v.dx, v.dy, mx, my, sg, z) * v.dx * v.dy : 0.0};
        block_tree<RedSum>(tid, val);                     // one term per thread: the tree alone
        if (tid == 0) partial[(size_t)blk * n + m] = val[0];
        __syncthreads();
    }
}
// one workgroup per moulin (blockIdx.x; the lists of an ensemble differ in length: a workgroup past the end of its member's list has nothing to do)
__device__ __forceinline__ void d_moulin_final(const double *__restrict__ partial, int nblk, int n, double *__restrict__ integ)
{
    const int m = blockIdx.x, tid = threadIdx.x;
    if (m >= n) return;                                                                                  // uniform
    double acc[1] = {0.0};
    for (int b = tid; b < nblk; b += 256) acc[0] = acc[0] + partial[(size_t)b * n + m];      // (the second stage's stride over a list laid out per tile)
    block_tree<RedSum>(tid, acc);
    if (tid == 0) integ[m] = acc[0];
}
__device__ __forceinline__ void d_moulin_src(const DV &v, int n, const double *__restrict__ mo, const double *__restrict__ flux,
                                             const double *__restrict__ integ, double tf, double *__restrict__ out, const Excl &ex,
                                             const double *__restrict__ cover)
{
    const int i = blockIdx.x * 16 + threadIdx.x, j = blockIdx.y * 16 + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    if ((i >= ex.i0 && i < ex.i1 && j >= ex.j0 && j < ex.j1) || (cover && cover[cidx(v, i, j)] != 0.0)) { out[cidx(v, i, j)] = 0.0; return; }   // filled by the average of the finer level
    double sum = 0.0;
    for (int m = 0; m < n; m++) {
        bool z;
        double val = moulin_cell(i + 0.5 + v.i0, j + 0.5 + v.j0, v.dx, v.dy, mo[3 * m], mo[3 * m + 1], mo[3 * m + 2], z);
        if (!z) sum += val * tf / integ[m] * flux[m];
    }
    out[cidx(v, i, j)] = sum;
}
template <class J> __global__ __launch_bounds__(256) void k_moulin_partial(J t, Excl ex, const double *__restrict__ cover)
{
    const MoulinJob &j = t.job();
    d_moulin_partial(j.v, j.n, j.mo, j.partial, ex, cover);
}
template <class J> __global__ void k_moulin_final(J t)
{
    const MoulinJob &j = t.job();
    d_moulin_final(j.partial, j.nblk, j.n, j.integ);
}
template <class J> __global__ __launch_bounds__(256) void k_moulin_src(J t, Excl ex, const double *__restrict__ cover)
{
    const MoulinJob &j = t.job();
    d_moulin_src(j.v, j.n, j.mo, j.flux, j.integ, t.time_factor(), j.out, ex, cover);
}
// the launchers: 16 x 16 tiles of the job's view (grd), one workgroup per moulin for the integrals; gz = 1, or the active members
template <class J> void launch_moulin_partial(const J &t, dim3 grd, hipStream_t st, Excl ex, const double *cover = nullptr)
{
    hipLaunchKernelGGL(k_moulin_partial<J>, grd, dim3(16, 16), 0, st, t, ex, cover);
}
template <class J> void launch_moulin_final(const J &t, int nmax, int gz, hipStream_t st) { hipLaunchKernelGGL(k_moulin_final<J>, dim3(nmax, 1, gz), dim3(256), 0, st, t); }
template <class J> void launch_moulin_src(const J &t, dim3 grd, hipStream_t st, Excl ex, const double *cover = nullptr)
{
    hipLaunchKernelGGL(k_moulin_src<J>, grd, dim3(16, 16), 0, st, t, ex, cover);
}
// ---- one moulin pass.  The three entry points below are the same computation over their REGIONS, a region being the cells of one launch: a
// whole level, a patch rectangle less the rectangle of the next level (Excl), a box less the cells a finer level covers (SUHMO_F_COVER).
// Integrate every region, add the regions' integrals, write the source term of every region with the total.  The pass owns the ONE device
// block of a call (positions and sigma, fluxes, integrals, the tile sums of the largest region) and frees it on every way out.  The first
// HIP error sticks: the steps after it do nothing, finish() reports it.
dim3 tiles_of(const DV &v) { return dim3((v.nx + 15) / 16, (v.ny + 15) / 16); }
size_t ntiles(const DV &v) { return (size_t)((v.nx + 15) / 16) * ((v.ny + 15) / 16); }
DV whole_level(DV v) { v.ny = v.nyg; v.j0 = 0; return v; }     // of a rank strip: all rows of its level
struct MoulinPass {
    const int n; const double tf; const hipStream_t st;
    std::vector<double> h;                   // {x, y, sigma} of every moulin, then the fluxes
    double *dev = nullptr, *mo = nullptr, *fl = nullptr, *integ = nullptr, *partial = nullptr;
    hipError_t e = hipSuccess;
    MoulinPass(int n_, double time_factor, suhmo_stream_t s) : n(n_), tf(time_factor), st((hipStream_t)s), h(4 * (size_t)n_) {}
    ~MoulinPass() { (void)hipFree(dev); }
    int pack(const double *positions, const double *sigma, const double *flux)
    {
        for (int m = 0; m < n; m++) {
            ARG(sigma[m] > 0.0);
            h[3 * m] = positions[2 * m]; h[3 * m + 1] = positions[2 * m + 1]; h[3 * m + 2] = sigma[m]; h[3 * (size_t)n + m] = flux[m];
        }
        return 0;
    }
    int upload(size_t maxblk)                // maxblk: the 16 x 16 tiles of the largest region
    {
        HIPCHK(hipMalloc(&dev, (5 * (size_t)n + maxblk * n) * sizeof(double)));
        mo = dev; fl = dev + 3 * (size_t)n; integ = dev + 4 * (size_t)n; partial = dev + 5 * (size_t)n;
        e = hipMemcpyAsync(dev, h.data(), 4 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, st);
        return 0;
    }
    // the integrals of every Gaussian over one region -> integ, on the device (only the geometry of v is read)
    void integrate(const DV &v, Excl ex = Excl{0, 0, 0, 0}, const double *cover = nullptr)
    {
        if (e != hipSuccess) return;
        const OneMoulinList region{MoulinJob{v, n, (int)ntiles(v), mo, nullptr, integ, partial, 0.0, nullptr}};    // (the integration reads no flux, tf, out)
        launch_moulin_partial(region, tiles_of(v), st, ex, cover);
        launch_moulin_final(region, n, 1, st);
        e = hipGetLastError();
    }
    void read(double *dst) { if (e == hipSuccess) e = hipMemcpyAsync(dst, integ, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st); }   // integ -> dst[n]
    bool wait() { if (e == hipSuccess) e = hipStreamSynchronize(st); return e == hipSuccess; }
    void set_total(const double *total) { if (e == hipSuccess) e = hipMemcpyAsync(integ, total, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st); }
    // the source term of one region from integ as it stands: the integrals of the one region of a level, or the total
    void source(const DV &v, double *out, Excl ex = Excl{0, 0, 0, 0}, const double *cover = nullptr)
    {
        if (e != hipSuccess) return;
        launch_moulin_src(OneMoulinList{MoulinJob{v, n, 0, mo, fl, integ, nullptr, tf, out}}, tiles_of(v), st, ex, cover);      // (... the source pass no tile sums)
        e = hipGetLastError();
    }
    int finish()
    {
        wait();
        (void)hipFree(dev); dev = nullptr;
        if (e != hipSuccess) { suhmo_set_error("moulin source: %s", hipGetErrorString(e)); return -2; }
        return 0;
    }
};
}  // namespace
// the lists of the active members of an ensemble (rows[k]: member k's, on the device; nmax: the longest list): three launches whatever their number
// (tf != NULL: the time factors of this launch instead of the rows')
int suhmo_batch_moulin_launch(const MoulinJob *rows, const BatchSel &sel, int nx, int ny, int nmax, hipStream_t st, const PerMember *tf)
{
    if (sel.n <= 0) return 0;
    const MemberMoulinLists t{rows, sel};
    const dim3 grd((nx + 15) / 16, (ny + 15) / 16, sel.n);
    launch_moulin_partial(t, grd, st, Excl{0, 0, 0, 0});
    launch_moulin_final(t, nmax, sel.n, st);
    if (tf) launch_moulin_src(StepMoulinLists{{rows, sel}, *tf}, grd, st, Excl{0, 0, 0, 0});
    else launch_moulin_src(t, grd, st, Excl{0, 0, 0, 0});
    HIPCHK(hipGetLastError());
    return 0;
}

// one level, one region: the integrals never leave the device between the two passes, the call synchronises once.  A rank strip integrates
// over the whole level on every rank (geometry only), in the single-level order, and writes its own rows
extern "C" int suhmo_level_moulin_source(suhmo_level_t *L, int n, const double *positions, const double *sigma,
                                         const double *flux, double time_factor, double *integrals, suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::Calc_moulin_source_term_distributed");
    ARG(L && n >= 1 && positions && sigma && flux);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[0];
    if (L->desc.nx_global > 0) { suhmo_set_error("moulin source on an AMR patch is not built yet (the integral spans all levels)"); return -5; }
    double *out = suhmo_field(L, 0, SUHMO_F_MSRC);
    if (!out) { suhmo_set_error("field allocation failed"); return -2; }
    MoulinPass p(n, time_factor, s);
    int rc = p.pack(positions, sigma, flux); if (rc) return rc;
    if ((rc = p.upload(ntiles(whole_level(D.v))))) return rc;
    p.integrate(whole_level(D.v));
    p.source(D.v, out);
    if (integrals) p.read(integrals);
    return p.finish();
}

// Calc_moulin_integral + Calc_moulin_source_term_distributed on the hierarchy (:1866-2066, :2797-2837): every level samples
// the Gaussians at its own resolution, cells under a finer level do not count in the integrals (finest level first, :1891)
// and receive the average of the finer level's source term afterwards (CoarseAverage :2819-2826).
extern "C" int suhmo_amr_moulin_source(suhmo_level_t **lv, int nlev, const int *patch_boxes, int n, const double *positions,
                                       const double *sigma, const double *flux, double time_factor, double *integrals, suhmo_stream_t s)
{
    ARG(lv && nlev >= 1 && nlev <= 8 && lv[0] && n >= 1 && positions && sigma && flux);
    int rc = suhmo_amr_check_hierarchy(lv, nlev); if (rc) return rc;
    // every level's WHOLE rectangle (only the geometry is read): from the boxes (rank strips: a rank may hold a part of a level or none of
    // it, and integrates all of them itself -- analytic integrand, single-process order, no communication) or the handles
    const DV &b = lv[0]->d[0].v;
    auto rect = [&](int nx, int ny, int i0, int j0, double dx, double dy) { DV v = b; v.nx = nx; v.ny = ny; v.i0 = i0; v.j0 = j0; v.dx = dx; v.dy = dy; return v; };
    DV geo[8];
    geo[0] = rect(b.nx, b.nyg, 0, 0, b.dx, b.dy);
    for (int l = 1; l < nlev; l++) {
        if (patch_boxes) {
            const int *q = patch_boxes + 4 * (l - 1);
            ARG(q[2] >= q[0] && q[3] >= q[1]);
            geo[l] = rect(2 * (q[2] - q[0] + 1), 2 * (q[3] - q[1] + 1), 2 * q[0], 2 * q[1], geo[l - 1].dx / 2.0, geo[l - 1].dy / 2.0);
            if (lv[l]) { const DV &v = lv[l]->d[0].v; const bool part = v.rk[0] || v.rk[1];            // a rank strip holds some of the rows, a whole patch all of them
                if (v.nx != geo[l].nx || v.i0 != geo[l].i0 || v.j0 < geo[l].j0 || v.j0 + v.ny > geo[l].j0 + geo[l].ny
                    || (!part && (v.j0 != geo[l].j0 || v.ny != geo[l].ny))) { suhmo_set_error("moulin source: level %d does not match patch_boxes", l); return -1; } }
        } else {
            if (!lv[l] || lv[l]->d[0].v.rk[0] || lv[l]->d[0].v.rk[1]) { suhmo_set_error("moulin source on rank strips needs patch_boxes"); return -1; }
            const DV &v = lv[l]->d[0].v;
            geo[l] = rect(v.nx, v.ny, v.i0, v.j0, v.dx, v.dy);
        }
    }
    auto excl_of = [&](int l, const DV &v) {                          // the box of level l+1 in cells of level l, relative to v's first cell
        if (l >= nlev - 1) return Excl{0, 0, 0, 0};
        const DV &f = geo[l + 1];
        return Excl{f.i0 / 2 - v.i0, f.j0 / 2 - v.j0, (f.i0 + f.nx) / 2 - v.i0, (f.j0 + f.ny) / 2 - v.j0};
    };
    for (int l = 0; l < nlev; l++) if (lv[l] && !suhmo_field(lv[l], 0, SUHMO_F_MSRC)) { suhmo_set_error("field allocation failed"); return -2; }
    HIPCHK(hipSetDevice(lv[0]->device));
    MoulinPass p(n, time_factor, s);
    if ((rc = p.pack(positions, sigma, flux))) return rc;
    size_t maxblk = 0;
    for (int l = 0; l < nlev; l++) maxblk = std::max(maxblk, ntiles(geo[l]));
    if ((rc = p.upload(maxblk))) return rc;
    std::vector<double> total((size_t)n, 0.0), part((size_t)n);
    for (int l = nlev - 1; l >= 0; l--) {                             // finest first (:1891)
        p.integrate(geo[l], excl_of(l, geo[l]));
        p.read(part.data());
        if (!p.wait()) break;
        for (int m = 0; m < n; m++) total[m] += part[m];
    }
    p.set_total(total.data());
    for (int l = 0; l < nlev; l++) if (lv[l]) p.source(lv[l]->d[0].v, lv[l]->d[0].fp.f[SUHMO_F_MSRC], excl_of(l, lv[l]->d[0].v));
    if ((rc = p.finish())) return rc;
    for (int l = nlev - 1; l > 0; l--) if (lv[l] && (rc = suhmo_amr2_average(lv[l - 1], lv[l], SUHMO_F_MSRC, SUHMO_F_MSRC, s))) return rc;
    if (integrals) for (int m = 0; m < n; m++) integrals[m] = total[m];
    return 0;
}

// suhmo_amr_moulin_source on a hierarchy of box unions (oracle/amr_step_m.c:or_amrm_model_moulin_source): finest level first,
// box after box; cells under a finer level (SUHMO_F_COVER) do not count and get the finer level's average afterwards
extern "C" int suhmo_hier_moulin_source(suhmo_hier_t *H, int n, const double *positions, const double *sigma, const double *flux,
                                        double time_factor, double *integrals, suhmo_stream_t s)
{
    ARG(H && n >= 1 && positions && sigma && flux);
    const int nlev = H->nlev;
    HIPCHK(hipSetDevice(H->device));
    int rc;
    MoulinPass p(n, time_factor, s);
    if ((rc = p.pack(positions, sigma, flux))) return rc;
    H->n_moulin_calls++;
    // owner computes (levels >= 1 dealt to the ranks): a rank integrates and fills the boxes it owns; the per-box integrals of all ranks are
    // gathered and added up in the single-process order (finest level first, box after box), so every rank gets the same bits
    size_t maxblk = 0;
    std::vector<size_t> first(nlev + 1, 0);                            // level l's first box in that order, counted from level 0
    for (int l = 0; l < nlev; l++) {
        const HLev &V = H->lev[l];
        first[l + 1] = first[l] + V.box.size();
        for (int k = 0; k < (int)V.box.size(); k++) {
            const bool owned = k >= V.first_owned() && k < V.first_owned() + V.n_owned();
            if (owned && !suhmo_field(V.box[k], 0, SUHMO_F_MSRC)) { suhmo_set_error("field allocation failed"); return -2; }
            maxblk = std::max(maxblk, ntiles(l == 0 ? whole_level(V.box[k]->d[0].v) : V.box[k]->d[0].v));
        }
    }
    if ((rc = p.upload(maxblk))) return rc;
    const size_t nbt = first[nlev];
    const double *whole_cover = dist_base(H) ? H->cover_whole : nullptr;   // level 0 cut into rank strips: every rank integrates all of it (geometry only)
    std::vector<double> perbox(nbt * (size_t)n, 0.0), total((size_t)n, 0.0);   // the integrals over every box (this rank's; the others' after the gather)
    // every box this rank owns, level l, with the cells of it a finer level covers
    auto owned_boxes = [&](int l, auto &&visit) {
        const HLev &V = H->lev[l];
        for (int k = V.first_owned(); k < V.first_owned() + V.n_owned(); k++) visit(k, V.box[k], l < nlev - 1 ? V.box[k]->d[0].fp.f[SUHMO_F_COVER] : nullptr);
    };
    for (int l = nlev - 1; l >= 0; l--)
        owned_boxes(l, [&](int k, suhmo_level *L, const double *cover) {
            const DV &v = L->d[0].v;
            const bool cutbase = l == 0 && (v.rk[0] || v.rk[1]);
            p.integrate(cutbase ? whole_level(v) : v, Excl{0, 0, 0, 0}, cutbase && l < nlev - 1 ? whole_cover : cover);
            p.read(&perbox[(first[l] + k) * (size_t)n]);
            p.wait();
        });
    if (p.e == hipSuccess && H->part) {                                // every rank's integrals over its boxes -> every rank
        hipError_t &e = p.e;
        const hipStream_t st = p.st;
        const int world = H->world;
        const size_t cnt = nbt * (size_t)n;
        double *gs = nullptr, *gr = nullptr;
        std::vector<double> all(cnt * world);
        e = hipMalloc(&gs, cnt * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(&gr, cnt * world * sizeof(double));
        if (e == hipSuccess) e = hipMemcpyAsync(gs, perbox.data(), cnt * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && (rc = suhmo_hier_allgather_(H, gs, (long)cnt, gr, st))) { (void)hipFree(gs); (void)hipFree(gr); return rc; }
        if (e == hipSuccess) e = hipMemcpyAsync(all.data(), gr, cnt * world * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (gs) (void)hipFree(gs);
        if (gr) (void)hipFree(gr);
        if (e == hipSuccess)
            for (int l = 1; l < nlev; l++)
                for (size_t k = 0; k < first[l + 1] - first[l]; k++) {
                    const int o = suhmo_hier_box_owner(H, l, (int)k, nullptr);
                    if (o >= 0) for (int m = 0; m < n; m++) perbox[(first[l] + k) * (size_t)n + m] = all[(size_t)o * cnt + (first[l] + k) * (size_t)n + m];
                }
    }
    for (int l = nlev - 1; l >= 0; l--)                                // finest first (:1891), box after box
        for (size_t k = first[l]; k < first[l + 1]; k++)
            for (int m = 0; m < n; m++) total[m] += perbox[k * (size_t)n + m];
    p.set_total(total.data());
    for (int l = 0; l < nlev; l++)
        owned_boxes(l, [&](int, suhmo_level *L, const double *cover) { p.source(L->d[0].v, L->d[0].fp.f[SUHMO_F_MSRC], Excl{0, 0, 0, 0}, cover); });
    if ((rc = p.finish())) return rc;
    for (int l = nlev - 1; l > 0; l--) if ((rc = hier_avg(H, l, SUHMO_F_MSRC, SUHMO_F_MSRC, 0, 0.0, p.st))) return rc;
    if (integrals) for (int m = 0; m < n; m++) integrals[m] = total[m];
    return 0;
}

// COMPUTE_TIMEVARYINGRECHARGE (src/AmrHydroF.ChF:346-373) on the ghosted box of the source term
__device__ __forceinline__ void d_time_varying_recharge(const DV &v, const double *__restrict__ zs, double *__restrict__ out, double TK, double background)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x - 1, j = blockIdx.y * blockDim.y + threadIdx.y - 1;
    if (i > v.nx || j > v.ny) return;
    const double ddf = 0.01 / 86400., dT_dZ = -0.0075;
    int idx = cidx(v, i, j);
    out[idx] = fmax(ddf * (TK + zs[idx] * dT_dZ), 0.0) + background;
}
// V: the temperature and the background input -- a double each for a level, PerMember for an ensemble
template <class T, class V> __global__ void k_time_varying_recharge(T t, V TK, V background)
{
    d_time_varying_recharge(t.view(), t.field(SUHMO_F_ZS), t.field(SUHMO_F_MSRC), value_of(t, TK), value_of(t, background));
}
template <class T, class V> static int launch_time_varying_recharge_(const T &t, const V &TK, const V &background, hipStream_t st)
{
    return launch_over(k_time_varying_recharge<T, V>, t, GHOSTED, st, TK, background);
}
int launch_time_varying_recharge(const OnMembers &t, const PerMember &TK, const PerMember &background, hipStream_t st)
{
    return launch_time_varying_recharge_(t, TK, background, st);
}
extern "C" int suhmo_level_time_varying_recharge(suhmo_level_t *L, double T_K, double background_input, suhmo_stream_t s)
{
    ARG(L);
    HIPCHK(hipSetDevice(L->device));
    Depth &D = L->d[0];
    if (!D.fp.f[SUHMO_F_ZS]) { suhmo_set_error("time-varying recharge: load the ice surface height (SUHMO_F_ZS) first"); return -1; }
    double *out = suhmo_field(L, 0, SUHMO_F_MSRC);
    if (!out) { suhmo_set_error("field allocation failed"); return -2; }
    return launch_time_varying_recharge_(on_level(L, 0), T_K, background_input, (hipStream_t)s);
}
// the same on every box of a hierarchy of box unions (timeStepFAS evaluates it level by level, :2846-2863, with no averaging down and no
// coarse-fine fill): level 0 as a level, every refined level as ONE launch over its boxes.  Everything is checked before the first launch
int suhmo_hier_recharge_check_(suhmo_hier *H, const char *who)
{
    if (H->world > 1 || H->part) { suhmo_set_error("%s: a hierarchy on rank strips (or with levels dealt to the ranks) is not built", who); return -5; }
    for (int l = 0; l < H->nlev; l++)
        for (size_t k = 0; k < H->lev[l].box.size(); k++)
            if (!H->lev[l].box[k]->d[0].fp.f[SUHMO_F_ZS]) {
                suhmo_set_error("%s: time-varying recharge: load the ice surface height (SUHMO_F_ZS) of level %d, box %d first", who, l, (int)k);
                return -1;
            }
    return 0;
}
int suhmo_hier_recharge_launch_(suhmo_hier *H, double T_K, double background_input, hipStream_t st)
{
    int rc;
    for (int l = 0; l < H->nlev; l++) if ((rc = ensure_field(H, l, SUHMO_F_MSRC))) return rc;
    for (int l = 0; l < H->nlev; l++) {
        if ((rc = on_hier_level(H, l, st, [&](const auto &t) { return launch_time_varying_recharge_(t, T_K, background_input, st); }))) return rc;
        H->n_recharge_launches++;
    }
    return 0;
}
extern "C" int suhmo_hier_time_varying_recharge(suhmo_hier_t *H, double T_K, double background_input, suhmo_stream_t s)
{
    ARG(H);
    int rc = suhmo_hier_recharge_check_(H, "suhmo_hier_time_varying_recharge"); if (rc) return rc;
    if ((rc = suhmo_hier_check_(H))) return rc;
    HIPCHK(hipSetDevice(H->device));
    return suhmo_hier_recharge_launch_(H, T_K, background_input, (hipStream_t)s);
}
