// suhmo_plt.cpp -- Chombo-HDF5 plot files of the hydrology state (include/suhmo_plt.h: the layout).  Host code, HDF5 C library.
#include "../../include/suhmo_plt.h"
#include "suhmo_h5.h"

using namespace h5;

// src/AmrHydro.cpp:5484-5511
extern "C" const char *const suhmo_plt_component_names[SUHMO_PLT_NCOMP] = {
    "head", "gapHeight", "bedelevation", "overburdenPress", "Pw", "Qw_x", "Qw_y", "Re", "meltRate", "GradHead_x", "GradHead_y", "iceHeight", "iceMask"};

extern "C" const char *suhmo_plt_last_error(void) { return h5::err; }

struct suhmo_plt {
    hid_t file = -1;
    bool writing = false;
    hid_t box_t = -1, iv_t = -1, rv_t = -1;
    int nlev = 0, ncomp = 0;
    double time = 0.0, dt = 0.0;
    std::vector<int> nbox;                // per level, once written / read
    std::vector<long> ndoubles;
};

namespace {
hid_t open_level(const suhmo_plt *h, int level)
{
    hid_t g = H5Gopen2(h->file, level_name(level).c_str(), H5P_DEFAULT);
    if (g < 0) fail("plot file does not contain %s", level_name(level).c_str());
    return g;
}
long long extent(hid_t d)
{
    hid_t sp = H5Dget_space(d);
    long long n = sp >= 0 ? (long long)H5Sget_simple_extent_npoints(sp) : -1;
    if (sp >= 0) H5Sclose(sp);
    return n;
}
int write_1d(hid_t g, const char *name, hid_t type, hsize_t n, const void *data)
{
    hid_t sp = H5Screate_simple(1, &n, nullptr);
    hid_t d = H5Dcreate2(g, name, type, sp, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT);
    int rc = 0;
    if (d < 0 || H5Dwrite(d, type, H5S_ALL, H5S_ALL, H5P_DEFAULT, data) < 0) rc = fail("cannot write %s", name);
    if (d >= 0) H5Dclose(d);
    H5Sclose(sp);
    return rc;
}
}  // namespace

extern "C" int suhmo_plt_create(suhmo_plt_t **out, const char *path, int num_levels, int ncomp, const char *const *names, double time, double dt)
{
    if (!out || !path || num_levels < 1 || ncomp < 1 || !names) return fail("bad argument");
    for (int c = 0; c < ncomp; c++) if (!names[c]) return fail("component %d has no name", c);
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    suhmo_plt *h = new suhmo_plt();
    h->writing = true; h->nlev = num_levels; h->ncomp = ncomp; h->time = time; h->dt = dt;
    h->nbox.assign(num_levels, -1); h->ndoubles.assign(num_levels, 0);
    h->file = H5Fcreate(path, H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT);
    if (h->file < 0) { delete h; return fail("cannot create %s", path); }
    h->box_t = make_box_type(); h->iv_t = make_iv_type(); h->rv_t = make_rv_type();
    hid_t g = H5Gcreate2(h->file, "Chombo_global", H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT);
    int sd = 2; double tr = 0.0;
    int rc = put_attr(g, "SpaceDim", H5T_NATIVE_INT, &sd) | put_attr(g, "testReal", H5T_NATIVE_DOUBLE, &tr);
    H5Gclose(g);
    hid_t root = H5Gopen2(h->file, "/", H5P_DEFAULT);
    rc |= put_str(root, "filetype", "VanillaAMRFileType") | put_attr(root, "num_levels", H5T_NATIVE_INT, &num_levels)
        | put_attr(root, "num_components", H5T_NATIVE_INT, &ncomp);
    for (int c = 0; c < ncomp && !rc; c++) {
        char key[32]; snprintf(key, sizeof(key), "component_%d", c);
        rc |= put_str(root, key, names[c]);
    }
    H5Gclose(root);
    if (rc) { suhmo_plt_close(h); return -1; }
    *out = h;
    return 0;
}

extern "C" int suhmo_plt_write_level(suhmo_plt_t *h, int level, double dx, double dy, const int domain[4], int nbox, const int *boxes, int ghost,
                                     const long *offsets, const double *data)
{
    if (!h || !h->writing || level < 0 || level >= h->nlev || !domain || nbox < 1 || !boxes || ghost < 0 || !offsets || !data) return fail("bad argument");
    if (h->nbox[level] >= 0) return fail("level %d is written already", level);
    if (offsets[0] != 0) return fail("level %d: the offsets do not start at 0", level);
    for (int k = 0; k < nbox; k++)
        if (offsets[k + 1] - offsets[k] != h->ncomp * box_pts(&boxes[4 * k], ghost))
            return fail("level %d: box %d holds %ld doubles, %d components on the box grown by %d need %ld", level, k, offsets[k + 1] - offsets[k], h->ncomp, ghost,
                        h->ncomp * box_pts(&boxes[4 * k], ghost));
    hid_t g = H5Gcreate2(h->file, level_name(level).c_str(), H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT);
    if (g < 0) return fail("cannot create group %s", level_name(level).c_str());
    const int r = level < h->nlev - 1 ? 2 : 1;
    RV2 vdx{dx, dy}; IV2 vr{r, r};
    const double dtl = h->dt / (double)(1L << level);
    Box2 dom{domain[0], domain[1], domain[2], domain[3]};
    int rc = put_attr(g, "vec_dx", h->rv_t, &vdx) | put_attr(g, "vec_ref_ratio", h->iv_t, &vr);
    if (dx == dy) rc |= put_attr(g, "dx", H5T_NATIVE_DOUBLE, &dx);
    rc |= put_attr(g, "ref_ratio", H5T_NATIVE_INT, &r);                  // (the two directions of the ratio always agree here)
    rc |= put_attr(g, "dt", H5T_NATIVE_DOUBLE, &dtl) | put_attr(g, "time", H5T_NATIVE_DOUBLE, &h->time) | put_attr(g, "prob_domain", h->box_t, &dom);
    if (!rc) {
        std::vector<Box2> bx(nbox);
        for (int k = 0; k < nbox; k++) bx[k] = Box2{boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3]};
        std::vector<int> procs(nbox, 0);
        std::vector<long long> off(offsets, offsets + nbox + 1);
        rc = write_1d(g, "boxes", h->box_t, (hsize_t)nbox, bx.data()) | write_1d(g, "Processors", H5T_NATIVE_INT, (hsize_t)nbox, procs.data())
           | write_1d(g, "data:datatype=0", H5T_NATIVE_DOUBLE, (hsize_t)offsets[nbox], data)
           | write_1d(g, "data:offsets=0", H5T_NATIVE_LLONG, (hsize_t)nbox + 1, off.data());
    }
    if (!rc) {
        hid_t a = H5Gcreate2(g, "data_attributes", H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT);
        IV2 gv{ghost, ghost};
        rc = put_attr(a, "comps", H5T_NATIVE_INT, &h->ncomp) | put_attr(a, "ghost", h->iv_t, &gv) | put_attr(a, "outputGhost", h->iv_t, &gv)
           | put_str(a, "objectType", "FArrayBox");
        H5Gclose(a);
    }
    H5Gclose(g);
    if (!rc) { h->nbox[level] = nbox; h->ndoubles[level] = offsets[nbox]; }
    return rc ? -1 : 0;
}

extern "C" int suhmo_plt_close(suhmo_plt_t *h)
{
    if (!h) return 0;
    if (h->box_t >= 0) H5Tclose(h->box_t);
    if (h->iv_t >= 0) H5Tclose(h->iv_t);
    if (h->rv_t >= 0) H5Tclose(h->rv_t);
    if (h->file >= 0) H5Fclose(h->file);
    delete h;
    return 0;
}

extern "C" int suhmo_plt_open(suhmo_plt_t **out, const char *path, int *num_levels, int *ncomp)
{
    if (!out || !path) return fail("bad argument");
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    suhmo_plt *h = new suhmo_plt();
    h->file = H5Fopen(path, H5F_ACC_RDONLY, H5P_DEFAULT);
    if (h->file < 0) { delete h; return fail("cannot open %s", path); }
    h->box_t = make_box_type(); h->iv_t = make_iv_type(); h->rv_t = make_rv_type();
    hid_t root = H5Gopen2(h->file, "/", H5P_DEFAULT);
    std::string type;
    int rc = get_str(root, "filetype", type) | get_attr(root, "num_levels", H5T_NATIVE_INT, &h->nlev) | get_attr(root, "num_components", H5T_NATIVE_INT, &h->ncomp);
    H5Gclose(root);
    if (!rc && type != "VanillaAMRFileType") rc = fail("%s: filetype is \"%s\", not a plot file", path, type.c_str());
    if (!rc && (h->nlev < 1 || h->ncomp < 1)) rc = fail("%s: %d levels, %d components", path, h->nlev, h->ncomp);
    if (rc) { suhmo_plt_close(h); return -1; }
    h->nbox.assign(h->nlev, -1); h->ndoubles.assign(h->nlev, 0);
    if (num_levels) *num_levels = h->nlev;
    if (ncomp) *ncomp = h->ncomp;
    *out = h;
    return 0;
}

extern "C" int suhmo_plt_read_name(suhmo_plt_t *h, int comp, char *buf, int size)
{
    if (!h || h->writing || comp < 0 || comp >= h->ncomp || !buf || size < 1) return fail("bad argument");
    char key[32]; snprintf(key, sizeof(key), "component_%d", comp);
    hid_t root = H5Gopen2(h->file, "/", H5P_DEFAULT);
    std::string name;
    int rc = get_str(root, key, name);
    H5Gclose(root);
    if (rc) return -1;
    if ((int)name.size() >= size) return fail("%s has %d characters, room for %d", key, (int)name.size(), size - 1);
    memcpy(buf, name.c_str(), name.size() + 1);
    return 0;
}

extern "C" int suhmo_plt_read_level(suhmo_plt_t *h, int level, double *vec_dx, int *vec_ref_ratio, double *dx, int *ref_ratio, double *dt, double *time,
                                    int domain[4], int *nbox, int *boxes, int max_boxes, int *ghost, long *ndoubles)
{
    if (!h || h->writing || level < 0 || level >= h->nlev) return fail("bad argument");
    hid_t g = open_level(h, level);
    if (g < 0) return -1;
    int rc = 0;
    if (vec_dx) { RV2 v{0, 0}; rc |= get_attr(g, "vec_dx", h->rv_t, &v); vec_dx[0] = v.x; vec_dx[1] = v.y; }
    if (vec_ref_ratio) { IV2 v{0, 0}; rc |= get_attr(g, "vec_ref_ratio", h->iv_t, &v); vec_ref_ratio[0] = v.intvecti; vec_ref_ratio[1] = v.intvectj; }
    if (dx) { *dx = 0.0; if (H5Aexists(g, "dx") > 0) rc |= get_attr(g, "dx", H5T_NATIVE_DOUBLE, dx); }
    if (ref_ratio) { *ref_ratio = 0; if (H5Aexists(g, "ref_ratio") > 0) rc |= get_attr(g, "ref_ratio", H5T_NATIVE_INT, ref_ratio); }
    if (dt) rc |= get_attr(g, "dt", H5T_NATIVE_DOUBLE, dt);
    if (time) rc |= get_attr(g, "time", H5T_NATIVE_DOUBLE, time);
    if (domain) { Box2 d{0, 0, 0, 0}; rc |= get_attr(g, "prob_domain", h->box_t, &d); domain[0] = d.lo_i; domain[1] = d.lo_j; domain[2] = d.hi_i; domain[3] = d.hi_j; }
    std::vector<Box2> bx;
    if (!rc) {
        hid_t d = H5Dopen2(g, "boxes", H5P_DEFAULT);
        if (d < 0) rc = fail("level %d has no boxes", level);
        else {
            const long long n = extent(d);
            if (n < 1) rc = fail("level %d has no boxes", level);
            else { bx.resize((size_t)n); if (H5Dread(d, h->box_t, H5S_ALL, H5S_ALL, H5P_DEFAULT, bx.data()) < 0) rc = fail("cannot read the boxes of level %d", level); }
            H5Dclose(d);
        }
    }
    int gw = 0;
    if (!rc) {
        hid_t a = H5Gopen2(g, "data_attributes", H5P_DEFAULT);
        if (a < 0) rc = fail("level %d has no data_attributes", level);
        else {
            IV2 gv{0, 0}; int comps = 0;
            rc = get_attr(a, "outputGhost", h->iv_t, &gv) | get_attr(a, "comps", H5T_NATIVE_INT, &comps);
            H5Gclose(a);
            gw = gv.intvecti;
            if (!rc && (comps != h->ncomp || gv.intvectj != gw || gw < 0)) rc = fail("level %d: %d components (the file: %d), ghost (%d, %d)", level, comps, h->ncomp, gv.intvecti, gv.intvectj);
        }
    }
    if (!rc) {
        long total = 0;
        for (const Box2 &b : bx) { const int q[4] = {b.lo_i, b.lo_j, b.hi_i, b.hi_j}; total += h->ncomp * box_pts(q, gw); }
        h->nbox[level] = (int)bx.size(); h->ndoubles[level] = total;
        if (nbox) *nbox = (int)bx.size();
        if (ghost) *ghost = gw;
        if (ndoubles) *ndoubles = total;
        if (boxes) {
            if ((int)bx.size() > max_boxes) rc = fail("level %d has %d boxes, room for %d", level, (int)bx.size(), max_boxes);
            else for (size_t k = 0; k < bx.size(); k++) { boxes[4 * k] = bx[k].lo_i; boxes[4 * k + 1] = bx[k].lo_j; boxes[4 * k + 2] = bx[k].hi_i; boxes[4 * k + 3] = bx[k].hi_j; }
        }
    }
    H5Gclose(g);
    return rc ? -1 : 0;
}

extern "C" int suhmo_plt_read_data(suhmo_plt_t *h, int level, long *offsets, double *data)
{
    if (!h || h->writing || level < 0 || level >= h->nlev || !offsets || !data) return fail("bad argument");
    if (h->nbox[level] < 0) return fail("read the level first (suhmo_plt_read_level)");
    hid_t g = open_level(h, level);
    if (g < 0) return -1;
    const int nb = h->nbox[level];
    int rc = 0;
    // the extents are checked against what the box list implies before anything is read into the caller's buffers
    std::vector<long long> off((size_t)nb + 1, 0);
    {
        hid_t d = H5Dopen2(g, "data:offsets=0", H5P_DEFAULT);
        if (d < 0) rc = fail("level %d has no data", level);
        else if (extent(d) != (long long)nb + 1) rc = fail("level %d: the offsets hold %lld entries, the level has %d boxes", level, extent(d), nb);
        else if (H5Dread(d, H5T_NATIVE_LLONG, H5S_ALL, H5S_ALL, H5P_DEFAULT, off.data()) < 0) rc = fail("cannot read the offsets of level %d", level);
        if (d >= 0) H5Dclose(d);
    }
    if (!rc && (off[0] != 0 || off[nb] != h->ndoubles[level])) rc = fail("level %d: the offsets run from %lld to %lld, the boxes need 0 to %ld", level, off[0], off[nb], h->ndoubles[level]);
    if (!rc) {
        hid_t d = H5Dopen2(g, "data:datatype=0", H5P_DEFAULT);
        if (d < 0) rc = fail("level %d has no data", level);
        else if (extent(d) != h->ndoubles[level]) rc = fail("level %d: the data set holds %lld values, the boxes need %ld", level, extent(d), h->ndoubles[level]);
        else if (H5Dread(d, H5T_NATIVE_DOUBLE, H5S_ALL, H5S_ALL, H5P_DEFAULT, data) < 0) rc = fail("cannot read the data of level %d", level);
        if (d >= 0) H5Dclose(d);
    }
    if (!rc) for (int k = 0; k <= nb; k++) offsets[k] = (long)off[k];
    H5Gclose(g);
    return rc ? -1 : 0;
}
