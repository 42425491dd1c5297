// suhmo_flatten.hip -- a hierarchy interpolated onto the uniform grid of its finest resolution: AmrHydro::interpFinest (src/AmrHydro.cpp:4623-4829), the
// composite that writePltPP (:5298-5389) hands to HDF5.  The rule, the components and the refusals: include/suhmo_hip.h, "FLATTEN";
// tests/flatten_ref.py is its numpy twin.  Read-only: the components are evaluated into PRIVATE scratch canvases with the geometry of the boxes'
// own; no field and no ghost ring of the hierarchy is written, and the fields' own ghost rings are not read.
//
// Per call, on one stream:
//   (i)   k_flat_eval     one launch per level: every component in the valid cells of every box -> the level's scratch
//   (ii)  hier_pwl_on / hier_ff_on   per level l >= 1, ascending: the scratch ring <- PiecewiseLinearFillPatch of level l-1's scratch, then the
//                         exchange between the boxes with corners -- the plans and launches of the regrid, over the scratch tables
//   (iii) k_flat_interp   one launch per level, ascending (a finer level overwrites): the level's valid cells times 2^(max_level - l) in each
//                         direction into the finest array on the device
//   (iv)  one hipMemcpyAsync into host_dst, one synchronisation
// (i) to (iii) are suhmo_hier_flatten_device_, which suhmo_compare.hip calls too (its FINEST mode reduces the finest array where it lies); (iv) is
// suhmo_hier_flatten's own
#include "suhmo_hier_int.h"
#include "suhmo_level_int.h"
#include "suhmo_transfer.h"
#include <climits>

using namespace hier;

namespace {
__device__ __forceinline__ const FP &scratch_of(const OnLevel &, const FP &base, const FP *) { return base; }
__device__ __forceinline__ const FP &scratch_of(const OnBoxes &, const FP &, const FP *tab) { return tab[blockIdx.z]; }

// (i) thread (i, j) of the box writes its cell of every component into scratch canvas q.  A field the box does not hold counts as 0.0
template <class T> __global__ void k_flat_eval(T t, FlatComps c, FP sbase, const FP *__restrict__ stab)
{
    const DV &v = t.view();
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    const FP &fp = t.fields();
    const FP &sp = scratch_of(t, sbase, stab);
    const int idx = cidx(v, i, j);
    for (int q = 0; q < c.n; q++) {
        const double *__restrict__ a = fp.f[c.f1[q]];
        double x = a ? a[idx] : 0.0;
        if (c.kind[q] == SUHMO_FLAT_DIFF) {                  // formed BEFORE the interpolation: the limiter is not linear
            const double *__restrict__ b = fp.f[c.f2[q]];
            x = x - (b ? b[idx] : 0.0);
        }
        sp.f[q][idx] = x;
    }
}

// (iii) FineInterp::interpToFine with the whole ratio r = 2^sh in one shot: rule (a) of the regrid (suhmo_transfer.h: limited_slopes with
// tangential_only, child_value), with the child offsets -0.5 + (p + 0.5) / r.  OUTPUT-centric: a thread owns two neighbouring
// cells of a finest row (they share their coarse cell, r being even) and stores them as one double2, consecutive lanes consecutive addresses; it
// recomputes the slopes and eta from the 3 x 3 coarse block, which r / 2 lanes of the row and r rows share through the caches.  COPY: r = 1, one
// cell per thread.  Rows beyond the grid are taken in further passes (gridDim.y is capped).
// Level 0 (use_base) is one canvas: the neighbour across a periodic side is addressed with the wrap.  A refined level reads its scratch ring,
// which (ii) has filled: another box's valid cell, a periodic image, or the linear fill from the level below (the edge clause).
template <bool COPY> __global__ __launch_bounds__(256) void k_flat_interp(const DV *__restrict__ dvtab, const FP *__restrict__ stab, DV bdv, FP sbase,
                                                                         int use_base, int sh, int nxd, int nyd, int perx, int pery, int ncomp,
                                                                         long nxF, long plane, double *__restrict__ out)
{
    const DV &v = use_base ? bdv : dvtab[blockIdx.z];
    const FP &sp = use_base ? sbase : stab[blockIdx.z];
    const long fl = ((long)blockIdx.x * blockDim.x + threadIdx.x) * (COPY ? 1 : 2);
    const int nxf = v.nx << sh, nyf = v.ny << sh;
    if (fl >= nxf) return;
    const int fi = (int)fl;
    const int I = fi >> sh, p = fi & ((1 << sh) - 1), Ig = v.i0 + I, P = v.P;
    const bool xl = perx || Ig - 1 >= 0, xh = perx || Ig + 1 <= nxd - 1;
    int ox[3] = {-1, 0, 1};
    if (use_base) {
        if (Ig - 1 < 0) ox[0] = nxd - 1;
        if (Ig + 1 > nxd - 1) ox[2] = -(nxd - 1);
    }
    const double rr = (double)(1 << sh);
    const double dx0 = -0.5 + ((double)p + 0.5) / rr, dx1 = -0.5 + ((double)(p + 1) + 0.5) / rr;
    for (int fj = blockIdx.y * blockDim.y + threadIdx.y; fj < nyf; fj += gridDim.y * blockDim.y) {
        const int J = fj >> sh, q = fj & ((1 << sh) - 1), Jg = v.j0 + J;
        const long o = (((long)v.j0 << sh) + fj) * nxF + ((long)v.i0 << sh) + fi;
        const int c = cidx(v, I, J);
        if (COPY) {
            for (int t = 0; t < ncomp; t++) out[t * plane + o] = sp.f[t][c];
            continue;
        }
        const bool yl = pery || Jg - 1 >= 0, yh = pery || Jg + 1 <= nyd - 1;
        int oy[3] = {-P, 0, P};
        if (use_base) {
            if (Jg - 1 < 0) oy[0] = (nyd - 1) * P;
            if (Jg + 1 > nyd - 1) oy[2] = -(nyd - 1) * P;
        }
        const bool ex[3] = {xl, true, xh}, ey[3] = {yl, true, yh};
        const double dy = -0.5 + ((double)q + 0.5) / rr;
        for (int t = 0; t < ncomp; t++) {
            const double *__restrict__ C = sp.f[t];
            double nb[3][3], s0, s1;
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int a = 0; a < 3; a++) nb[b][a] = (ex[a] && ey[b]) ? C[c + oy[b] + ox[a]] : 0.0;
            limited_slopes(nb, xl, xh, yl, yh, true, s0, s1);
            // (the finest column of an even fi is even and so are nxF and the plane: 16-byte aligned)
            *reinterpret_cast<double2 *>(out + t * plane + o) = make_double2(child_value(nb[1][1], s0, s1, dx0, dy), child_value(nb[1][1], s0, s1, dx1, dy));
        }
    }
}

int flat_comps(int ncomp, const suhmo_flat_comp_t *comps, FlatComps &c, const char *who)
{
    if (ncomp < 1 || ncomp > SUHMO_FLAT_MAX_COMPS || !comps) { suhmo_set_error("%s: %d components (1 .. %d)", who, ncomp, SUHMO_FLAT_MAX_COMPS); return -1; }
    memset(&c, 0, sizeof(c));
    c.n = ncomp;
    for (int q = 0; q < ncomp; q++) {
        const int k = comps[q].kind;
        if (k != SUHMO_FLAT_FIELD && k != SUHMO_FLAT_DIFF) { suhmo_set_error("%s: component %d: kind %d", who, q, k); return -1; }
        const int f[2] = {comps[q].field, comps[q].field2};
        for (int m = 0; m < (k == SUHMO_FLAT_DIFF ? 2 : 1); m++) {
            if (f[m] < 0 || f[m] >= SUHMO_F_COUNT) { suhmo_set_error("%s: component %d: no field %d", who, q, f[m]); return -1; }
            if (f[m] == SUHMO_F_COVER || f[m] == SUHMO_F_PHI2) { suhmo_set_error("%s: component %d: field %d is the library's own (SUHMO_F_COVER / SUHMO_F_PHI2)", who, q, f[m]); return -1; }
            if (is_face(f[m])) { suhmo_set_error("%s: component %d: field %d is a face field", who, q, f[m]); return -1; }
        }
        c.kind[q] = k; c.f1[q] = f[0]; c.f2[q] = k == SUHMO_FLAT_DIFF ? f[1] : f[0];
    }
    return 0;
}

// the scratch of level l: at least n component slots.  On return the level's device table lists exactly the slots of flat_slab: a call that
// cannot get all it needs gives back what it took (rc -2) and leaves slabs, host table and device table as it found them
int scratch(suhmo_hier *H, int l, int n, hipStream_t st)
{
    HLev &V = H->lev[l];
    const size_t had = V.flat_slab.size();
    if ((int)had >= n) return 0;
    const size_t nb = V.box.size();
    std::vector<size_t> off(nb);
    size_t elems = 0;
    for (size_t k = 0; k < nb; k++) { off[k] = elems; elems += V.box[k]->d[0].elems; }
    V.flat_elems = elems;
    if (V.flat_h.size() != nb) V.flat_h.assign(nb, FP{});
    auto give_back = [&]() {
        while (V.flat_slab.size() > had) {
            (void)hipFree(V.flat_slab.back());
            V.flat_slab.pop_back();
            for (size_t k = 0; k < nb; k++) V.flat_h[k].f[V.flat_slab.size()] = nullptr;
        }
        (void)hipGetLastError();
        suhmo_set_error("suhmo_hier_flatten: the scratch of level %d cannot be allocated (%zu bytes per component)", l, elems * sizeof(double));
        return -2;
    };
    while ((int)V.flat_slab.size() < n) {
        const int q = (int)V.flat_slab.size();
        double *p = nullptr;
        // (flatten_fail_slot: the test switch that makes the allocation of that slot on the finest level fail)
        if ((q == H->flat_fail_slot && l == H->nlev - 1) || hipMalloc(&p, elems * sizeof(double)) != hipSuccess) return give_back();
        // on the call's stream, ahead of the launch that writes the valid cells (the ring of level 0 is never read; the others' is filled by (ii))
        if (hipMemsetAsync(p, 0, elems * sizeof(double), st) != hipSuccess) { (void)hipFree(p); return give_back(); }
        for (size_t k = 0; k < nb; k++) V.flat_h[k].f[q] = p + off[k];
        V.flat_slab.push_back(p);
    }
    if (l >= 1) {                                            // (every earlier call has ended with a synchronisation: nothing reads the table)
        if (hipStreamSynchronize(st) != hipSuccess || (!V.flat_fp && hipMalloc(&V.flat_fp, nb * sizeof(FP)) != hipSuccess)
            || hipMemcpy(V.flat_fp, V.flat_h.data(), nb * sizeof(FP), hipMemcpyHostToDevice) != hipSuccess) {
            const int rc = give_back();                      // (the table, if there is one, still lists the slots that stay: rewritten for good measure)
            if (V.flat_fp) (void)hipMemcpy(V.flat_fp, V.flat_h.data(), nb * sizeof(FP), hipMemcpyHostToDevice);
            return rc;
        }
    }
    return 0;
}
}  // namespace

void suhmo_hier_flatten_release_(suhmo_hier *H)
{
    if (H->flat_buf) (void)hipFree(H->flat_buf);
    H->flat_buf = nullptr; H->flat_cap = 0;
    for (int l = 0; l < 8; l++) {
        HLev &V = H->lev[l];
        for (double *p : V.flat_slab) (void)hipFree(p);
        V.flat_slab.clear(); V.flat_h.clear(); V.flat_elems = 0;
        if (V.flat_fp) (void)hipFree(V.flat_fp);
        V.flat_fp = nullptr;
    }
}

int suhmo_flat_comps_(const char *who, int ncomp, const suhmo_flat_comp_t *comps, FlatComps &c) { return flat_comps(ncomp, comps, c, who); }

// the refusals that depend on max_level and on how the hierarchy is laid out, in the order of the header
int suhmo_hier_flatten_check_(const suhmo_hier *H, int max_level)
{
    const int top = H->nlev - 1;
    const int nx0 = H->lev[0].nxd, ny0 = H->lev[0].nyd;
    if (max_level < top) { suhmo_set_error("suhmo_hier_flatten: max_level = %d is below the finest level %d", max_level, top); return -1; }
    if (max_level > 30 || ((long)nx0 << max_level) > INT_MAX || ((long)ny0 << max_level) > INT_MAX) {
        suhmo_set_error("suhmo_hier_flatten: max_level = %d: the finest grid of a %d x %d base leaves int", max_level, nx0, ny0); return -1;
    }
    if (H->world > 1 || H->part || H->shadowed) {
        suhmo_set_error("suhmo_hier_flatten: a hierarchy on rank strips, with levels dealt to the ranks or created with shadow = 1 is not built"); return -5;
    }
    return 0;
}

// the device part of a flatten, steps (i) to (iii): the components of `c` on the uniform grid of max_level in H->flat_buf, [comp][j][i].  The
// caller has checked (suhmo_flat_comps_, suhmo_hier_flatten_check_) and set the device; nothing is copied and nothing synchronised at the end
int suhmo_hier_flatten_device_(suhmo_hier *H, int max_level, const FlatComps &c, hipStream_t st)
{
    int rc;
    const int ncomp = c.n, top = H->nlev - 1;
    const int nx0 = H->lev[0].nxd, ny0 = H->lev[0].nyd;
    const long nxF = (long)nx0 << max_level, nyF = (long)ny0 << max_level, plane = nxF * nyF;
    const size_t need = (size_t)ncomp * (size_t)plane;       // (< 2^4 x 2^62: no overflow; bytes may overflow, hence the first test)
    if (H->flat_cap < need) {
        if (H->flat_buf) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(H->flat_buf); H->flat_buf = nullptr; H->flat_cap = 0; }
        if (need > ((size_t)1 << 56) || hipMalloc(&H->flat_buf, need * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            H->flat_buf = nullptr;
            suhmo_set_error("suhmo_hier_flatten: the finest array (%d x %ld x %ld doubles) cannot be allocated", ncomp, nyF, nxF);
            return -2;
        }
        H->flat_cap = need;
    }
    for (int l = 0; l <= top; l++) if ((rc = scratch(H, l, ncomp, st))) return rc;
    suhmo_level *B = base_of(H);
  { SUHMO_TIME("interpFinest: evaluation, ghost fills, interpolation");        // (timer mode 2: the time of the kernels)
    // (i)
    for (int l = 0; l <= top; l++) {
        if (l == 0) rc = launch_over(k_flat_eval<OnLevel>, on_level(B, 0), CELLS, st, c, H->lev[0].flat_h[0], (const FP *)nullptr);
        else {
            suhmo_multi m;
            if ((rc = multi_of(H, l, st, m))) return rc;
            rc = launch_over(k_flat_eval<OnBoxes>, m.on(), CELLS, st, c, FP{}, (const FP *)H->lev[l].flat_fp);
        }
        if (rc) return rc;
        H->n_flat_launches++;
    }
    // (ii)
    for (int l = 1; l <= top; l++) {
        HLev &V = H->lev[l], &C = H->lev[l - 1];
        const bool ub = l - 1 == 0;
        for (int q = 0; q < ncomp; q++) {
            if ((rc = hier_pwl_on(H, l, V.flat_fp, q, ub ? nullptr : C.flat_fp, ub ? C.flat_h[0] : FP{}, ub ? 1 : 0, q, st))) return rc;
            if (V.pwl.n) H->n_flat_launches++;
        }
        for (int q = 0; q < ncomp; q += 2) {
            if ((rc = hier_ff_on(H, l, V.flat_fp, q, q + 1 < ncomp ? q + 1 : -1, true, st))) return rc;
            if (V.ff_all.n) H->n_flat_launches++;
        }
    }
    // (iii)
    for (int l = 0; l <= top; l++) {
        HLev &V = H->lev[l];
        const int sh = max_level - l;
        const bool ub = l == 0;
        const int mx = ub ? nx0 : V.maxnx, my = ub ? ny0 : V.maxny, nb = (int)V.box.size();
        const long tx = sh ? ((long)mx << sh) / 2 : mx, ty = (long)my << sh;
        const unsigned gx = (unsigned)((tx + 63) / 64);
        // (a memory-bound launch: some thousand workgroups, the rows beyond them in further passes of the same threads)
        const long gy_all = (ty + 3) / 4, gy_cap = std::max(1L, 8192L / ((long)gx * nb));
        const dim3 grd(gx, (unsigned)std::min(gy_all, std::min(gy_cap, 65535L)), (unsigned)nb), blk(64, 4);
        auto k = sh ? k_flat_interp<false> : k_flat_interp<true>;
        hipLaunchKernelGGL(k, grd, blk, 0, st, ub ? nullptr : V.d_dv, ub ? nullptr : V.flat_fp, ub ? B->d[0].v : DV{}, ub ? V.flat_h[0] : FP{}, ub ? 1 : 0, sh,
                           V.nxd, V.nyd, (int)H->bc.periodic[0], (int)H->bc.periodic[1], ncomp, nxF, plane, H->flat_buf);
        HIPCHK(hipGetLastError());
        H->n_flat_launches++;
    }
  }
    return 0;
}

extern "C" int suhmo_hier_flatten(suhmo_hier_t *H, int max_level, int ncomp, const suhmo_flat_comp_t *comps, long dims[2], double *host_dst,
                                  suhmo_stream_t s)
{
    SUHMO_TIME("AmrHydro::interpFinest");
    ARG(H && H->nlev >= 1 && dims);
    FlatComps c;
    int rc;
    if ((rc = flat_comps(ncomp, comps, c, "suhmo_hier_flatten")) || (rc = suhmo_hier_flatten_check_(H, max_level))) return rc;
    const long nxF = (long)H->lev[0].nxd << max_level, nyF = (long)H->lev[0].nyd << max_level;
    dims[0] = nxF; dims[1] = nyF;
    if (!host_dst) return 0;
    hipStream_t st = HST(s);
    HIPCHK(hipSetDevice(H->device));
    if ((rc = suhmo_hier_flatten_device_(H, max_level, c, st))) return rc;
    const size_t need = (size_t)ncomp * (size_t)(nxF * nyF);
  { SUHMO_TIME("interpFinest: copy to the host");
    // (iv)
    HIPCHK(hipMemcpyAsync(host_dst, H->flat_buf, need * sizeof(double), hipMemcpyDeviceToHost, st));
    H->n_flat_copies++;
    HIPCHK(hipStreamSynchronize(st));
  }
    return 0;
}
