// suhmo_h5.h -- what the two writers of libsuhmo_chk.so share (suhmo_chk.cpp: checkpoints, suhmo_plt.cpp: plot files): the error text, Chombo's
// compound types for boxes and vectors, scalar attributes.  Host code, HDF5 C library.
#pragma once
#include <hdf5.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace h5 {
inline thread_local char err[512] = "";
inline int fail(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof(err), fmt, ap); va_end(ap);
    return -1;
}
struct Box2 { int lo_i, lo_j, hi_i, hi_j; };
struct IV2 { int intvecti, intvectj; };
struct RV2 { double x, y; };
inline hid_t make_box_type()
{
    hid_t t = H5Tcreate(H5T_COMPOUND, sizeof(Box2));
    H5Tinsert(t, "lo_i", HOFFSET(Box2, lo_i), H5T_NATIVE_INT); H5Tinsert(t, "lo_j", HOFFSET(Box2, lo_j), H5T_NATIVE_INT);
    H5Tinsert(t, "hi_i", HOFFSET(Box2, hi_i), H5T_NATIVE_INT); H5Tinsert(t, "hi_j", HOFFSET(Box2, hi_j), H5T_NATIVE_INT);
    return t;
}
inline hid_t make_iv_type()
{
    hid_t t = H5Tcreate(H5T_COMPOUND, sizeof(IV2));
    H5Tinsert(t, "intvecti", HOFFSET(IV2, intvecti), H5T_NATIVE_INT); H5Tinsert(t, "intvectj", HOFFSET(IV2, intvectj), H5T_NATIVE_INT);
    return t;
}
inline hid_t make_rv_type()
{
    hid_t t = H5Tcreate(H5T_COMPOUND, sizeof(RV2));
    H5Tinsert(t, "x", HOFFSET(RV2, x), H5T_NATIVE_DOUBLE); H5Tinsert(t, "y", HOFFSET(RV2, y), H5T_NATIVE_DOUBLE);
    return t;
}
inline int put_attr(hid_t loc, const char *name, hid_t type, const void *val)
{
    hid_t sp = H5Screate(H5S_SCALAR);
    hid_t a = H5Acreate2(loc, name, type, sp, H5P_DEFAULT, H5P_DEFAULT);
    herr_t e = a >= 0 ? H5Awrite(a, type, val) : -1;
    if (a >= 0) H5Aclose(a);
    H5Sclose(sp);
    return e < 0 ? fail("cannot write attribute %s", name) : 0;
}
inline int put_str(hid_t loc, const char *name, const char *val)
{
    hid_t t = H5Tcopy(H5T_C_S1);
    H5Tset_size(t, strlen(val) > 0 ? strlen(val) : 1);
    int rc = put_attr(loc, name, t, val);
    H5Tclose(t);
    return rc;
}
inline int get_attr(hid_t loc, const char *name, hid_t type, void *val)
{
    if (H5Aexists(loc, name) <= 0) return fail("attribute %s missing", name);
    hid_t a = H5Aopen(loc, name, H5P_DEFAULT);
    herr_t e = a >= 0 ? H5Aread(a, type, val) : -1;
    if (a >= 0) H5Aclose(a);
    return e < 0 ? fail("cannot read attribute %s", name) : 0;
}
// a fixed-length string attribute (as put_str writes it) -> val, NUL-terminated
inline int get_str(hid_t loc, const char *name, std::string &val)
{
    if (H5Aexists(loc, name) <= 0) return fail("attribute %s missing", name);
    hid_t a = H5Aopen(loc, name, H5P_DEFAULT);
    if (a < 0) return fail("cannot read attribute %s", name);
    hid_t t = H5Aget_type(a);
    const size_t n = H5Tget_size(t);
    std::vector<char> buf(n + 1, 0);
    herr_t e = H5Tget_class(t) == H5T_STRING && !H5Tis_variable_str(t) ? H5Aread(a, t, buf.data()) : -1;
    H5Tclose(t); H5Aclose(a);
    if (e < 0) return fail("cannot read attribute %s", name);
    val = buf.data();
    return 0;
}
inline std::string level_name(int l) { char b[32]; snprintf(b, sizeof(b), "level_%d", l); return b; }
inline long box_pts(const int *b, int g) { return (long)(b[2] - b[0] + 1 + 2 * g) * (long)(b[3] - b[1] + 1 + 2 * g); }
}  // namespace h5
