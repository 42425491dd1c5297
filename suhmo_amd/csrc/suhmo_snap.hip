// suhmo_snap.hip -- a list of fields of a whole hierarchy (or of one level) gathered into Chombo's on-disk fab order: what writePlotFile and
// writeCheckpointFile (src/AmrHydro.cpp:5474-5667, 5670-5842) hand to HDF5.  One launch and one copy per level, whatever the number of boxes.
// The layout, the components and the refusals: include/suhmo_hip.h, "SNAPSHOT".  Read-only: no field is allocated, no ghost cell filled.
#include "suhmo_hier_int.h"
#include "suhmo_level_int.h"

using namespace hier;

namespace {
// the component list of a launch, by value (as BatchSel: nothing to upload, nothing to synchronise)
struct SnapComps { int n; int kind[SUHMO_SNAP_MAX_COMPS], field[SUHMO_SNAP_MAX_COMPS]; double value[SUHMO_SNAP_MAX_COMPS]; };

// thread (i, j) of the box grown by g writes its cell of every component: dst is the box's fab [comp][j][i], i fastest
__device__ __forceinline__ void d_pack_fields(const DV &v, const FP &fp, const SnapComps &c, int g, double *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x - g, j = blockIdx.y * blockDim.y + threadIdx.y - g;
    if (i >= v.nx + g || j >= v.ny + g) return;
    const int w = v.nx + 2 * g;
    const size_t plane = (size_t)w * (size_t)(v.ny + 2 * g);
    const size_t o = (size_t)(j + g) * w + (size_t)(i + g);
    const int idx = cidx(v, i, j);
    const bool valid = i >= 0 && i < v.nx && j >= 0 && j < v.ny;
    for (int q = 0; q < c.n; q++) {
        double x = 0.0;
        const double *__restrict__ p = c.kind[q] == SUHMO_SNAP_CONST ? nullptr : fp.f[c.field[q]];
        if (c.kind[q] == SUHMO_SNAP_CONST) x = c.value[q];
        else if (!p) x = 0.0;                                                            // a field the box does not hold
        else if (c.kind[q] == SUHMO_SNAP_FIELD) x = p[idx];
        else if (valid) {                                                                // EdgeToCell: the faces on either side of the cell
            const bool xf = c.field[q] == SUHMO_F_BX || c.field[q] == SUHMO_F_QWX || c.field[q] == SUHMO_F_DCX;
            x = 0.5 * (p[idx] + p[idx + (xf ? 1 : v.P)]);
        }
        dst[q * plane + o] = x;
    }
}
// cells: per box the cells of the boxes before it (each grown by g), or NULL for a single level; a box's fab starts at ncomp times that
template <class T> __global__ void k_pack_fields(T t, SnapComps c, int g, const long *__restrict__ cells, double *__restrict__ dst)
{
    d_pack_fields(t.view(), t.fields(), c, g, dst + (cells ? (size_t)cells[t.slot(1)] * (size_t)c.n : 0));
}
template <class T> int launch_pack(const T &t, const SnapComps &c, int g, const long *cells, double *dst, hipStream_t st)
{
    return launch_over(k_pack_fields<T>, t, g ? GHOSTED : CELLS, st, c, g, cells, dst);
}

int snap_comps(const char *who, int ncomp, const suhmo_snap_comp_t *comps, int ghost, SnapComps &c)
{
    if (ncomp < 1 || ncomp > SUHMO_SNAP_MAX_COMPS || !comps) { suhmo_set_error("%s: %d components (1 .. %d)", who, ncomp, SUHMO_SNAP_MAX_COMPS); return -1; }
    if (ghost != 0 && ghost != 1) { suhmo_set_error("%s: ghost = %d (0 or 1)", who, ghost); return -1; }
    c.n = ncomp;
    for (int q = 0; q < SUHMO_SNAP_MAX_COMPS; q++) { c.kind[q] = SUHMO_SNAP_CONST; c.field[q] = 0; c.value[q] = 0.0; }
    for (int q = 0; q < ncomp; q++) {
        const int k = comps[q].kind, f = comps[q].field;
        if (k != SUHMO_SNAP_FIELD && k != SUHMO_SNAP_FACE_TO_CELL && k != SUHMO_SNAP_CONST) { suhmo_set_error("%s: component %d: kind %d", who, q, k); return -1; }
        c.kind[q] = k;
        if (k == SUHMO_SNAP_CONST) { c.value[q] = comps[q].value; continue; }
        if (f < 0 || f >= SUHMO_F_COUNT) { suhmo_set_error("%s: component %d: no field %d", who, q, f); return -1; }
        if (f == SUHMO_F_COVER || f == SUHMO_F_PHI2) { suhmo_set_error("%s: component %d: field %d is the library's own (SUHMO_F_COVER / SUHMO_F_PHI2)", who, q, f); return -1; }
        if ((k == SUHMO_SNAP_FIELD) == is_face(f)) {
            suhmo_set_error("%s: component %d: field %d is %s (a face field is read as SUHMO_SNAP_FACE_TO_CELL, a cell field as SUHMO_SNAP_FIELD)", who, q, f,
                            is_face(f) ? "a face field" : "cell-centred");
            return -1;
        }
        c.field[q] = f;
    }
    return 0;
}
long grown(int nx, int ny, int g) { return (long)(nx + 2 * g) * (long)(ny + 2 * g); }
int snap_refuse_layout(const suhmo_hier *H, const char *who)
{
    if (H->world > 1 || H->part || H->shadowed) {
        suhmo_set_error("%s: a hierarchy on rank strips, with levels dealt to the ranks or created with shadow = 1 is not built", who); return -5;
    }
    return 0;
}
// the device staging of a hierarchy: at least `need` doubles
int staging(suhmo_hier *H, size_t need)
{
    if (H->snap_cap >= need) return 0;
    if (H->snap_buf) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(H->snap_buf)); H->snap_buf = nullptr; H->snap_cap = 0; }
    HIPCHK(hipMalloc(&H->snap_buf, need * sizeof(double)));
    H->snap_cap = need;
    return 0;
}
// per box of level l >= 1 the cells of the boxes before it, each grown by g: built once per ghost width
int cell_table(suhmo_hier *H, int l, int g)
{
    HLev &V = H->lev[l];
    if (V.snap_cells[g].d) return 0;
    std::vector<long> h(V.box.size());
    long sum = 0;
    for (size_t k = 0; k < V.box.size(); k++) { h[k] = sum; const DV &v = V.box[k]->d[0].v; sum += grown(v.nx, v.ny, g); }
    return V.snap_cells[g].upload(h);
}
}  // namespace

int suhmo_hier_snapshot_check_(const suhmo_hier *H, const char *who, int ncomp, const suhmo_snap_comp_t *comps, int ghost)
{
    SnapComps c;
    int rc = snap_comps(who, ncomp, comps, ghost, c);
    return rc ? rc : snap_refuse_layout(H, who);
}
long suhmo_hier_snapshot_sizes_(const suhmo_hier *H, int ncomp, int ghost, long *level_offset, long *box_offset)
{
    long total = 0, *bo = box_offset;
    for (int l = 0; l < H->nlev; l++) {
        if (level_offset) level_offset[l] = total;
        long sum = 0;
        for (suhmo_level *L : H->lev[l].box) {
            if (bo) *bo++ = sum;
            sum += ncomp * grown(L->d[0].v.nx, L->d[0].v.ny, ghost);
        }
        if (bo) *bo++ = sum;
        total += sum;
    }
    if (level_offset) level_offset[H->nlev] = total;
    return total;
}

extern "C" int suhmo_hier_snapshot(suhmo_hier_t *H, int ncomp, const suhmo_snap_comp_t *comps, int ghost, long *level_offset, long *box_offset,
                                   double *host_dst, suhmo_stream_t s)
{
    ARG(H && H->nlev >= 1 && level_offset && box_offset);
    SnapComps c;
    int rc;
    if ((rc = snap_comps("suhmo_hier_snapshot", ncomp, comps, ghost, c)) || (rc = snap_refuse_layout(H, "suhmo_hier_snapshot"))) return rc;
    suhmo_hier_snapshot_sizes_(H, ncomp, ghost, level_offset, box_offset);
    if (!host_dst) return 0;
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(H->device));
    size_t largest = 0;
    for (int l = 0; l < H->nlev; l++) largest = std::max(largest, (size_t)(level_offset[l + 1] - level_offset[l]));
    if ((rc = staging(H, largest))) return rc;
    for (int l = 1; l < H->nlev; l++) if ((rc = cell_table(H, l, ghost))) { suhmo_set_error("suhmo_hier_snapshot: the offset table of level %d", l); return rc; }
    for (int l = 0; l < H->nlev; l++) {
        if (l == 0) rc = launch_pack(on_level(base_of(H), 0), c, ghost, nullptr, H->snap_buf, st);
        else {
            suhmo_multi m;
            if ((rc = multi_of(H, l, st, m))) return rc;
            rc = launch_pack(m.on(), c, ghost, H->lev[l].snap_cells[ghost].d, H->snap_buf, st);
        }
        if (rc) return rc;
        H->n_snap_launches++;
        HIPCHK(hipMemcpyAsync(host_dst + level_offset[l], H->snap_buf, (size_t)(level_offset[l + 1] - level_offset[l]) * sizeof(double), hipMemcpyDeviceToHost, st));
        H->n_snap_copies++;
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// one level: the single box (0, 0, nx - 1, ny - 1).  The staging lives for the call
extern "C" int suhmo_level_snapshot(suhmo_level_t *L, int ncomp, const suhmo_snap_comp_t *comps, int ghost, long *ndoubles, double *host_dst, suhmo_stream_t s)
{
    ARG(L && ndoubles);
    SnapComps c;
    int rc = snap_comps("suhmo_level_snapshot", ncomp, comps, ghost, c); if (rc) return rc;
    if (L->stub || on_strip(L)) {
        suhmo_set_error("suhmo_level_snapshot: a rank strip (or a box another rank holds) is not built"); return -5;
    }
    const DV &v = L->d[0].v;
    *ndoubles = ncomp * grown(v.nx, v.ny, ghost);
    if (!host_dst) return 0;
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(L->device));
    double *buf = nullptr;
    HIPCHK(hipMalloc(&buf, (size_t)*ndoubles * sizeof(double)));
    rc = launch_pack(on_level(L, 0), c, ghost, nullptr, buf, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(host_dst, buf, (size_t)*ndoubles * sizeof(double), hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (e != hipSuccess) { suhmo_set_error("suhmo_level_snapshot: %s", hipGetErrorString(e)); return -2; }
    return rc;
}
