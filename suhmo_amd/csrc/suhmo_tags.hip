// suhmo_tags.hip -- grid generation: cell tagging on the device (tagCellsLevel, src/AmrHydro.cpp:4539-4604) and, on the host, the step from tag
// maps to the box lists suhmo_hier_create takes (what the reference leaves to BRMeshRefine, src/AmrHydro.cpp:4227-4511, 4835-4955).  The C-ABI,
// the semantics and the clustering rules: include/suhmo_hip.h, "GRID GENERATION".  [Chombo] BRMeshRefine lives in the un-vendored fork: the
// clustering is Berger & Rigoutsos (1991) as the header writes it down, unpinned against the reference.
//
// The tagging kernel is one body over the launch targets of suhmo_target.h (a level: OnLevel, the boxes of a level of a hierarchy: OnBoxes):
// one thread per valid cell; a cell inside (vmin, vmax) stores the byte 1 into the entries of the level's map its grown rectangle touches.
// Every writer of an entry stores the same value, so there is nothing to order: plain byte stores.  Nothing else launches these kernels.
#include "suhmo_hier_int.h"
#include <array>

struct suhmo_tagmap {
    unsigned char *d = nullptr;      // device, [nby][nbx]
    int nbx = 0, nby = 0, g = 0;     // g = 0: empty (allocated or not), takes the granularity of the next call
    size_t cap = 0;
    int *sub = nullptr; int sub_cap = 0;   // device, the box list of the last suhmo_hier_restrict_tags (4 ints per box)
};
void suhmo_tagmap_release(suhmo_tagmap *m)
{
    if (!m) return;
    if (m->d) (void)hipFree(m->d);
    if (m->sub) (void)hipFree(m->sub);
    delete m;
}

namespace {
// gx, gy: reach of a tag in cells (max(grow, grow_dir)); nxd, nyd: the level's domain; the cell (i, j) of the view is cell (i0 + i, j0 + j) of it
template <class T>
__global__ __launch_bounds__(256) void k_tag_cells(T t, int field, double vmin, double vmax, int gx, int gy, int g, int nxd, int nyd, int nbx,
                                                   unsigned char *__restrict__ map)
{
    const DV &v = t.view();
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (i >= v.nx || j >= v.ny) return;
    const double x = t.field(field)[cidx(v, i, j)];
    if (!(vmin < x && x < vmax)) return;                       // both strict: a NaN tags nothing
    const int I = v.i0 + i, J = v.j0 + j;
    const int a0 = max(I - gx, 0) / g, a1 = min(I + gx, nxd - 1) / g;      // clipped to the domain box: no periodic wrap
    const int b0 = max(J - gy, 0) / g, b1 = min(J + gy, nyd - 1) / g;
    for (int b = b0; b <= b1; b++)
        for (int a = a0; a <= a1; a++) map[(size_t)b * nbx + a] = 1;
}

// levelTags &= tagSubset (src/AmrHydro.cpp:4530-4533): one thread per entry of the map; an entry whose first cell lies in none of the boxes
// (lo0, lo1, hi0, hi1, aligned to g: the entry then lies wholly outside all of them) is cleared with a plain byte store
__global__ __launch_bounds__(256) void k_restrict_tags(unsigned char *__restrict__ map, int nbx, int nby, int g, const int *__restrict__ boxes, int nboxes)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nbx * nby) return;
    const int I = (int)(e % nbx) * g, J = (int)(e / nbx) * g;
    for (int k = 0; k < nboxes; k++)
        if (I >= boxes[4 * k] && I <= boxes[4 * k + 2] && J >= boxes[4 * k + 1] && J <= boxes[4 * k + 3]) return;
    map[e] = 0;
}

int tag_args(int field, int grow, int grow_x, int grow_y, int granularity)
{
    ARG(field >= 0 && field < SUHMO_F_COUNT);
    ARG(grow >= 0 && grow_x >= 0 && grow_y >= 0 && granularity >= 1);
    return 0;
}
// the map of a level of nxd x nyd cells at granularity g, ready to be written (allocated and zeroed on first use and after a clear)
int tagmap_prepare(suhmo_tagmap *&m, int nxd, int nyd, int g, hipStream_t st)
{
    if (!m) m = new suhmo_tagmap();
    if (m->g && m->g != g) { suhmo_set_error("tags: the level's map is kept at granularity %d; clear it before tagging at %d", m->g, g); return -1; }
    if (m->g) return 0;
    const int nbx = (nxd + g - 1) / g, nby = (nyd + g - 1) / g;
    const size_t n = (size_t)nbx * nby;
    if (n > m->cap) {
        if (m->d) (void)hipFree(m->d);
        m->d = nullptr; m->cap = 0;
        HIPCHK(hipMalloc(&m->d, n));
        m->cap = n;
    }
    HIPCHK(hipMemsetAsync(m->d, 0, n, st));
    m->nbx = nbx; m->nby = nby; m->g = g;
    return 0;
}
int tagmap_get(suhmo_tagmap *m, int device, unsigned char *host, int *nbx, int *nby)
{
    const bool has = m && m->g;
    if (nbx) *nbx = has ? m->nbx : 0;
    if (nby) *nby = has ? m->nby : 0;
    if (!has || !host) return 0;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());                              // the tagging launches of any stream
    HIPCHK(hipMemcpy(host, m->d, (size_t)m->nbx * m->nby, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ box generation (host)
struct Gen {
    const unsigned char *T; int NX;        // tag map in blocks, row-major
    double fill; int M;                    // fill_ratio, max_box_size / block_factor
    std::vector<int> out;                  // emitted rectangles (I0, J0, I1, J1), in order
    std::vector<int> sx, sy;

    bool tag(int i, int j) const { return T[(size_t)j * NX + i] != 0; }
    // a hole of S[0 .. n) nearest the centre (ties: the lower index); -1: none
    static int hole(const std::vector<int> &S, int n)
    {
        int best = -1, bd = 0;
        for (int k = 0; k < n; k++) {
            if (S[k]) continue;
            const int d = std::abs(2 * k - (n - 1));
            if (best < 0 || d < bd) { best = k; bd = d; }
        }
        return best;
    }
    // the strongest inflection of S[0 .. n): the cut lies between k and k + 1; ties: nearest the centre, then the lower index; -1: none
    static int inflection(const std::vector<int> &S, int n, long &strength)
    {
        int best = -1, bd = 0;
        strength = 0;
        auto D = [&](int k) { return (long)S[k - 1] - 2L * S[k] + S[k + 1]; };
        for (int k = 1; k + 2 < n; k++) {
            const long a = D(k), b = D(k + 1);
            if (!((a < 0 && b > 0) || (a > 0 && b < 0))) continue;
            const long s = std::labs(a - b);
            const int d = std::abs(2 * k + 1 - (n - 1));
            if (best < 0 || s > strength || (s == strength && d < bd)) { best = k; strength = s; bd = d; }
        }
        return best;
    }
    void make(int i0, int j0, int i1, int j1)
    {
        // 1. the bounding box of the tags inside
        int a0 = i1 + 1, a1 = i0 - 1, b0 = j1 + 1, b1 = j0 - 1;
        long n = 0;
        for (int j = j0; j <= j1; j++)
            for (int i = i0; i <= i1; i++)
                if (tag(i, j)) { n++; a0 = std::min(a0, i); a1 = std::max(a1, i); b0 = std::min(b0, j); b1 = std::max(b1, j); }
        if (!n) return;
        i0 = a0; i1 = a1; j0 = b0; j1 = b1;
        const int w = i1 - i0 + 1, h = j1 - j0 + 1;
        // 2. efficient and small enough
        if ((double)n / (double)((long)w * h) >= fill && w <= M && h <= M) { out.insert(out.end(), {i0, j0, i1, j1}); return; }
        // 3. signatures
        sx.assign(w, 0); sy.assign(h, 0);
        for (int j = j0; j <= j1; j++)
            for (int i = i0; i <= i1; i++)
                if (tag(i, j)) { sx[i - i0]++; sy[j - j0]++; }
        const bool xfirst = w >= h;                       // the longer side, a tie goes to x
        int dir = -1, lo_end = 0, hi_begin = 0;            // split direction: [lo, lo_end] + [hi_begin, hi] (offsets from the rectangle's corner)
        {   // (a) hole
            const int hx = hole(sx, w), hy = hole(sy, h);
            if (hx >= 0 && (xfirst || hy < 0)) { dir = 0; lo_end = hx - 1; hi_begin = hx + 1; }
            else if (hy >= 0) { dir = 1; lo_end = hy - 1; hi_begin = hy + 1; }
        }
        if (dir < 0) {   // (b) inflection
            long stx = 0, sty = 0;
            const int kx = inflection(sx, w, stx), ky = inflection(sy, h, sty);
            if (kx >= 0 && (ky < 0 || stx > sty || (stx == sty && xfirst))) { dir = 0; lo_end = kx; hi_begin = kx + 1; }
            else if (ky >= 0) { dir = 1; lo_end = ky; hi_begin = ky + 1; }
        }
        if (dir < 0) {   // (c) bisect
            dir = xfirst ? 0 : 1;
            lo_end = (dir == 0 ? w : h) / 2 - 1; hi_begin = lo_end + 1;
        }
        // 4. the lower part first
        if (dir == 0) { make(i0, j0, i0 + lo_end, j1); make(i0 + hi_begin, j0, i1, j1); }
        else { make(i0, j0, i1, j0 + lo_end); make(i0, j0 + hi_begin, i1, j1); }
    }
};

// the entries of a level of n cells (granularity g, two levels below the boxes) that the cells lo .. hi of the level in between touch: wrapped
// into a periodic side, dropped beyond a non-periodic one
void nesting_entries(int lo, int hi, int n_mid, bool periodic, int g, std::vector<int> &e)
{
    e.clear();
    for (int c = lo; c <= hi; c++) {
        int w = c;
        if (w < 0 || w >= n_mid) {
            if (!periodic) continue;
            w = ((w % n_mid) + n_mid) % n_mid;
        }
        const int q = (w >> 1) / g;
        if (std::find(e.begin(), e.end(), q) == e.end()) e.push_back(q);
    }
}
}  // namespace

extern "C" int suhmo_grids_generate(int nx0, int ny0, const int periodic[2], const suhmo_grid_params_t *p, int ntag, const unsigned char *const *tags,
                                    int *nlev_out, int *nbox, int *boxes, int boxes_cap)
{
    ARG(p && periodic && nlev_out && nbox && tags);
    ARG(nx0 >= 1 && ny0 >= 1 && ntag >= 1 && ntag <= 7 && boxes_cap >= 0 && (boxes || boxes_cap == 0));
    const int b = p->block_factor;
    if (b < 2 || (b & (b - 1))) { suhmo_set_error("grids: block_factor %d is not a power of two >= 2", b); return -1; }
    if (p->max_box_size < b || p->max_box_size % b) { suhmo_set_error("grids: max_box_size %d is not a positive multiple of block_factor %d", p->max_box_size, b); return -1; }
    if (!(p->fill_ratio > 0.0 && p->fill_ratio <= 1.0)) { suhmo_set_error("grids: fill_ratio %g is not in (0, 1]", p->fill_ratio); return -1; }
    const int g = b / 2, nest = std::max(p->nesting_radius, 2);      // suhmo_hier_create demands 2
    if (nx0 % g || ny0 % g) { suhmo_set_error("grids: block_factor / 2 = %d does not divide the base level %d x %d", g, nx0, ny0); return -1; }
    if ((long)nx0 << ntag > (1L << 30) || (long)ny0 << ntag > (1L << 30)) { suhmo_set_error("grids: level %d of a %d x %d base is too large", ntag, nx0, ny0); return -1; }
    for (int l = 0; l < ntag; l++) ARG(tags[l]);
    // levels above the first level without tags are dropped
    int top = 0;
    for (; top < ntag; top++) {
        const size_t n = (size_t)((nx0 << top) / g) * ((ny0 << top) / g);
        if (!std::any_of(tags[top], tags[top] + n, [](unsigned char c) { return c != 0; })) break;
    }
    std::vector<std::vector<int>> lev(top + 2);          // lev[l]: boxes of level l, 4 ints each, in cells of level l
    std::vector<unsigned char> T;
    std::vector<int> ex, ey;
    for (int l = top - 1; l >= 0; l--) {
        const int NX = (nx0 << l) / g, NY = (ny0 << l) / g;
        T.assign(tags[l], tags[l] + (size_t)NX * NY);
        for (unsigned char &c : T) c = c != 0;
        const std::vector<int> &up = lev[l + 2];
        for (size_t k = 0; k < up.size(); k += 4) {       // proper nesting of the level above the one generated here
            nesting_entries((up[k] >> 1) - nest, (up[k + 2] >> 1) + nest, nx0 << (l + 1), periodic[0] != 0, g, ex);
            nesting_entries((up[k + 1] >> 1) - nest, (up[k + 3] >> 1) + nest, ny0 << (l + 1), periodic[1] != 0, g, ey);
            for (int J : ey) for (int I : ex) T[(size_t)J * NX + I] = 1;
        }
        Gen G{T.data(), NX, p->fill_ratio, p->max_box_size / b, {}, {}, {}};
        G.make(0, 0, NX - 1, NY - 1);
        std::vector<int> &o = lev[l + 1];
        for (size_t k = 0; k < G.out.size(); k += 4)
            o.insert(o.end(), {G.out[k] * b, G.out[k + 1] * b, (G.out[k + 2] + 1) * b - 1, (G.out[k + 3] + 1) * b - 1});
    }
    *nlev_out = top + 1;
    long total = 0;
    nbox[0] = 0;
    for (int l = 1; l <= top; l++) { nbox[l] = (int)(lev[l].size() / 4); total += nbox[l]; }
    for (int l = top + 1; l <= ntag; l++) nbox[l] = 0;
    if (total > boxes_cap) { suhmo_set_error("grids: %ld boxes generated, boxes_cap is %d: call again with room for %ld", total, boxes_cap, total); return -4; }
    int *q = boxes;
    for (int l = 1; l <= top; l++) q = std::copy(lev[l].begin(), lev[l].end(), q);
    return 0;
}

// ------------------------------------------------------------------ tagging (C-ABI)
extern "C" int suhmo_level_tag_cells(suhmo_level_t *L, int field, double vmin, double vmax, int grow, int grow_x, int grow_y, int granularity,
                                     suhmo_stream_t s)
{
    ARG(L && !L->stub);
    int rc = tag_args(field, grow, grow_x, grow_y, granularity);
    if (rc) return rc;
    const DV &v = L->d[0].v;
    if (v.rk[0] || v.rk[1] || (L->desc.nx_global == 0 && (v.j0 != 0 || v.ny != v.nyg))) { suhmo_set_error("tags: rank strips are not built"); return -5; }
    HIPCHK(hipSetDevice(L->device));
    if (!suhmo_field(L, 0, field)) { suhmo_set_error("field allocation failed"); return -2; }
    if ((rc = tagmap_prepare(L->tags, v.nxg, v.nyg, granularity, HST(s)))) return rc;
    return launch_over(k_tag_cells<OnLevel>, on_level(L, 0), CELLS, HST(s), field, vmin, vmax, std::max(grow, grow_x), std::max(grow, grow_y), granularity,
                       v.nxg, v.nyg, L->tags->nbx, L->tags->d);
}
extern "C" int suhmo_level_clear_tags(suhmo_level_t *L)
{
    ARG(L);
    if (L->tags) L->tags->g = 0;
    return 0;
}
extern "C" int suhmo_level_get_tags(suhmo_level_t *L, unsigned char *host, int *nbx, int *nby)
{
    ARG(L);
    return tagmap_get(L->tags, L->device, host, nbx, nby);
}

extern "C" int suhmo_hier_tag_cells(suhmo_hier_t *H, int level, int field, double vmin, double vmax, int grow, int grow_x, int grow_y, int granularity,
                                    suhmo_stream_t s)
{
    ARG(H && level >= 0 && level < H->nlev);
    int rc = tag_args(field, grow, grow_x, grow_y, granularity);
    if (rc) return rc;
    if (H->world > 1) { suhmo_set_error("tags: a hierarchy on rank strips is not built"); return -5; }
    HIPCHK(hipSetDevice(H->device));
    hier::HLev &V = H->lev[level];
    if ((rc = hier::ensure_field(H, level, field))) return rc;
    if ((rc = tagmap_prepare(H->tags[level], V.nxd, V.nyd, granularity, HST(s)))) return rc;
    suhmo_tagmap *m = H->tags[level];
    const int gx = std::max(grow, grow_x), gy = std::max(grow, grow_y);
    if (level == 0)
        return launch_over(k_tag_cells<OnLevel>, on_level(hier::base_of(H), 0), CELLS, HST(s), field, vmin, vmax, gx, gy, granularity, V.nxd, V.nyd, m->nbx, m->d);
    suhmo_multi mu;
    if ((rc = hier::multi_of(H, level, HST(s), mu))) return rc;
    return launch_over(k_tag_cells<OnBoxes>, mu.on(), CELLS, HST(s), field, vmin, vmax, gx, gy, granularity, V.nxd, V.nyd, m->nbx, m->d);
}
extern "C" int suhmo_hier_clear_tags(suhmo_hier_t *H, int level)
{
    ARG(H && level < H->nlev);
    for (int l = 0; l < H->nlev; l++)
        if ((level < 0 || l == level) && H->tags[l]) H->tags[l]->g = 0;
    return 0;
}
extern "C" int suhmo_hier_get_tags(suhmo_hier_t *H, int level, unsigned char *host, int *nbx, int *nby)
{
    ARG(H && level >= 0 && level < H->nlev);
    return tagmap_get(H->tags[level], H->device, host, nbx, nby);
}

extern "C" int suhmo_hier_restrict_tags(suhmo_hier_t *H, int level, int nboxes, const int *boxes, suhmo_stream_t s)
{
    ARG(H && level >= 0 && level < H->nlev && nboxes >= 0 && (boxes || nboxes == 0));
    if (H->world > 1) { suhmo_set_error("tags: a hierarchy on rank strips is not built"); return -5; }
    if (nboxes == 0) return 0;                                   // the reference skips an empty subset
    suhmo_tagmap *m = H->tags[level];
    if (!m || !m->g) return 0;                                   // no map: nothing to restrict
    for (int k = 0; k < nboxes; k++) {
        const int *b = boxes + 4 * (size_t)k;
        if (b[0] > b[2] || b[1] > b[3]) { suhmo_set_error("tags: subset box %d of level %d is empty (%d, %d, %d, %d)", k, level, b[0], b[1], b[2], b[3]); return -1; }
        if (b[0] % m->g || b[1] % m->g || (b[2] + 1) % m->g || (b[3] + 1) % m->g) {
            suhmo_set_error("tags: subset box %d of level %d (%d, %d, %d, %d) is not aligned to the map's granularity %d: an entry must lie wholly inside or outside",
                            k, level, b[0], b[1], b[2], b[3], m->g);
            return -1;
        }
    }
    HIPCHK(hipSetDevice(H->device));
    if (nboxes > m->sub_cap) {
        if (m->sub) (void)hipFree(m->sub);                        // (hipFree waits for the launches that read the old list)
        m->sub = nullptr; m->sub_cap = 0;
        HIPCHK(hipMalloc(&m->sub, 4 * (size_t)nboxes * sizeof(int)));
        m->sub_cap = nboxes;
    }
    HIPCHK(hipMemcpyAsync(m->sub, boxes, 4 * (size_t)nboxes * sizeof(int), hipMemcpyHostToDevice, HST(s)));
    HIPCHK(hipStreamSynchronize(HST(s)));                        // the caller's list is pageable memory and may be written again on return; once per
                                                                 // tag variable and level of a regrid, not on the path of a step
    const size_t n = (size_t)m->nbx * m->nby;
    hipLaunchKernelGGL(k_restrict_tags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, HST(s), m->d, m->nbx, m->nby, m->g, m->sub, nboxes);
    HIPCHK(hipGetLastError());
    return 0;
}

// the per-level subsets as the reference nests them when it reads tagSubsetBoxesFile (src/AmrHydro.cpp:1097-1108), host only: for l >= 1 the
// NESTED subset of level l - 1 refined by 2, when it is not empty, replaces an empty subset of level l and is intersected with a non-empty one
extern "C" int suhmo_tag_subsets_nest(int nlev, const int *nbox, const int *boxes, int *nbox_out, int *boxes_out, int boxes_cap)
{
    ARG(nlev >= 1 && nlev <= 8 && nbox && nbox_out && boxes_cap >= 0 && (boxes_out || boxes_cap == 0));
    std::vector<std::vector<int>> sub(nlev);
    const int *q = boxes;
    for (int l = 0; l < nlev; l++) {
        ARG(nbox[l] >= 0 && (boxes || nbox[l] == 0));
        for (int k = 0; k < nbox[l]; k++, q += 4) {
            ARG(q[0] <= q[2] && q[1] <= q[3]);
            sub[l].insert(sub[l].end(), q, q + 4);
        }
        if (l == 0 || sub[l - 1].empty()) continue;
        std::vector<int> crse;
        for (size_t k = 0; k < sub[l - 1].size(); k += 4) {
            const int *c = &sub[l - 1][k];
            crse.insert(crse.end(), {2 * c[0], 2 * c[1], 2 * c[2] + 1, 2 * c[3] + 1});
        }
        if (sub[l].empty()) { sub[l] = crse; continue; }
        std::vector<int> both;
        for (size_t a = 0; a < sub[l].size(); a += 4)
            for (size_t c = 0; c < crse.size(); c += 4) {
                const int lo0 = std::max(sub[l][a], crse[c]), lo1 = std::max(sub[l][a + 1], crse[c + 1]);
                const int hi0 = std::min(sub[l][a + 2], crse[c + 2]), hi1 = std::min(sub[l][a + 3], crse[c + 3]);
                if (lo0 <= hi0 && lo1 <= hi1) both.insert(both.end(), {lo0, lo1, hi0, hi1});
            }
        sub[l] = both;
    }
    long total = 0;
    for (int l = 0; l < nlev; l++) { nbox_out[l] = (int)(sub[l].size() / 4); total += nbox_out[l]; }
    if (total > boxes_cap) { suhmo_set_error("tag subsets: %ld boxes after nesting, boxes_cap is %d: call again with room for %ld", total, boxes_cap, total); return -4; }
    int *o = boxes_out;
    for (int l = 0; l < nlev; l++) o = std::copy(sub[l].begin(), sub[l].end(), o);
    return 0;
}

extern "C" int suhmo_hier_generate_grids(suhmo_hier_t *H, const suhmo_grid_params_t *p, int *nlev_out, int *nbox, int *boxes, int boxes_cap, int *same)
{
    ARG(H && p && nlev_out && nbox);
    if (H->world > 1) { suhmo_set_error("grids: a hierarchy on rank strips is not built"); return -5; }
    std::vector<std::vector<unsigned char>> maps;
    for (int l = 0; l < H->nlev && l < 7; l++) {
        const suhmo_tagmap *m = H->tags[l];
        if (!m || !m->g) break;
        if (m->g * 2 != p->block_factor) { suhmo_set_error("grids: the tag map of level %d is kept at granularity %d, block_factor / 2 is %d", l, m->g, p->block_factor / 2); return -1; }
        maps.emplace_back((size_t)m->nbx * m->nby);
        int rc = tagmap_get(H->tags[l], H->device, maps.back().data(), nullptr, nullptr);
        if (rc) return rc;
    }
    if (maps.empty()) { suhmo_set_error("grids: level 0 has no tag map"); return -1; }
    std::vector<const unsigned char *> ptr;
    for (const auto &m : maps) ptr.push_back(m.data());
    const hier::HLev &B = H->lev[0];
    int rc = suhmo_grids_generate(B.nxd, B.nyd, H->bc.periodic, p, (int)ptr.size(), ptr.data(), nlev_out, nbox, boxes, boxes_cap);
    if (rc) return rc;
    if (same) {      // gridsSame (src/AmrHydro.cpp:4278-4296): the same set of boxes on every level
        bool eq = *nlev_out == H->nlev;
        const int *q = boxes;
        for (int l = 1; eq && l < H->nlev; l++) {
            const std::vector<int> &b4 = H->lev[l].b4;
            eq = (size_t)nbox[l] * 4 == b4.size();
            if (eq) {
                auto sorted = [](const int *a, size_t nb) {
                    std::vector<std::array<int, 4>> v(nb);
                    for (size_t k = 0; k < nb; k++) v[k] = {a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]};
                    std::sort(v.begin(), v.end());
                    return v;
                };
                eq = sorted(q, nbox[l]) == sorted(b4.data(), nbox[l]);
            }
            q += 4 * (size_t)nbox[l];
        }
        *same = eq;
    }
    return 0;
}
