/*
 * suhmo_plt.h -- C-ABI of the plot file writer / reader (libsuhmo_chk.so, host side, HDF5 C library).
 *
 * Replaces AmrHydro::writePlotFile (src/AmrHydro.cpp:5474-5667), which hands thirteen components per level to Chombo's
 * WriteAnisotropicAMRHierarchyHDF5.  A level's data arrive here as ONE multi-component block in Chombo's on-disk order -- a level slice of
 * suhmo_hier_snapshot (include/suhmo_hip.h, "SNAPSHOT") with its offsets -- and are written as they are: no per-box and no per-component copy.
 *
 * LAYOUT, restated from Chombo 3.2's lib/src/AMRIO/AMRIO.cpp and lib/src/BoxTools/CH_HDF5.cpp.  The fork is not vendored and the reference ships
 * no plot file: UNPINNED, like the checkpoint's (include/suhmo_chk.h); the round trip is what the tests hold it to.
 *
 *   where                      name               type                              value
 *   /                          filetype           string                            "VanillaAMRFileType"
 *   /                          num_levels         int
 *   /                          num_components     int
 *   /                          component_<n>      string                            n = 0 .. num_components - 1, unpadded
 *   /Chombo_global             SpaceDim, testReal int, double                       2, 0.0 (as the checkpoint writes them)
 *   /level_<l>                 vec_dx             compound {x, y} double
 *   /level_<l>                 vec_ref_ratio      compound {intvecti, intvectj} int (2, 2); (1, 1) on the finest level
 *   /level_<l>                 dx, ref_ratio      double, int                       only when the two directions agree
 *   /level_<l>                 dt                 double                            the file's dt / 2^l (the reference passes dt = 1.)
 *   /level_<l>                 time               double
 *   /level_<l>                 prob_domain        compound {lo_i, lo_j, hi_i, hi_j} int
 *   /level_<l>/boxes           dataset            compound box, one per box
 *   /level_<l>/Processors      dataset            int, one per box                  0
 *   /level_<l>/data:datatype=0 dataset            double                            box after box, each [comp][j][i] over the box grown by ghost
 *   /level_<l>/data:offsets=0  dataset            long long, nbox + 1               prefix sums of the boxes' sizes, in doubles
 *   /level_<l>/data_attributes comps              int                               num_components
 *   /level_<l>/data_attributes ghost, outputGhost compound {intvecti, intvectj} int (ghost, ghost); the reference plots with (1, 1)
 *   /level_<l>/data_attributes objectType         string                            "FArrayBox"
 *
 * The thirteen components of the reference, in its order (:5484-5511): head, gapHeight, bedelevation, overburdenPress, Pw, Qw_x, Qw_y, Re,
 * meltRate, GradHead_x, GradHead_y, iceHeight, iceMask (suhmo_plt_component_names).
 *
 * Plain C, host pointers, int return codes (0 ok), text via suhmo_plt_last_error.
 */
#ifndef SUHMO_PLT_H
#define SUHMO_PLT_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct suhmo_plt suhmo_plt_t;

#define SUHMO_PLT_NCOMP 13
extern const char *const suhmo_plt_component_names[SUHMO_PLT_NCOMP];

const char *suhmo_plt_last_error(void);

/* ---- writing: the levels 0 .. num_levels - 1, in order */
int suhmo_plt_create(suhmo_plt_t **out, const char *path, int num_levels, int ncomp, const char *const *names, double time, double dt);
/* boxes: nbox x {lo0, lo1, hi0, hi1}; offsets: nbox + 1 prefix sums in doubles, offsets[k + 1] - offsets[k] = ncomp x box k grown by ghost;
 * data: offsets[nbox] doubles */
int suhmo_plt_write_level(suhmo_plt_t *h, int level, double dx, double dy, const int domain[4], int nbox, const int *boxes, int ghost,
                          const long *offsets, const double *data);
int suhmo_plt_close(suhmo_plt_t *h);

/* ---- reading */
int suhmo_plt_open(suhmo_plt_t **out, const char *path, int *num_levels, int *ncomp);
int suhmo_plt_read_name(suhmo_plt_t *h, int comp, char *buf, int size);
/* every pointer may be NULL.  vec_dx[2], vec_ref_ratio[2]; *dx = 0.0 / *ref_ratio = 0 where the file has no scalar attribute; boxes == NULL:
 * only the count; *ndoubles: the length of the level's data */
int suhmo_plt_read_level(suhmo_plt_t *h, int level, double *vec_dx, int *vec_ref_ratio, double *dx, int *ref_ratio, double *dt, double *time,
                         int domain[4], int *nbox, int *boxes, int max_boxes, int *ghost, long *ndoubles);
/* offsets: nbox + 1, data: *ndoubles of suhmo_plt_read_level, which must have been called for that level */
int suhmo_plt_read_data(suhmo_plt_t *h, int level, long *offsets, double *data);

#ifdef __cplusplus
}
#endif
#endif
