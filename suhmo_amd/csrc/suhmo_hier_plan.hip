// suhmo_hier_plan.hip -- the plan compiler of a hierarchy of box unions (suhmo_hier_int.h): what ties the boxes of a level to each
// other and to the level below, compiled on the host ONCE when the hierarchy is created, and the levels dealt to the ranks.  No kernels.
#include "suhmo_hier_int.h"
#include <map>

namespace hier {
void BoxIndex::build(const std::vector<int> &boxes, int nx, int ny)
{
    b4 = &boxes; nxd = nx; nyd = ny; nbx = (nx + bs - 1) / bs; nby = (ny + bs - 1) / bs;
    std::vector<int> cnt((size_t)nbx * nby + 1, 0);
    const int nb = (int)boxes.size() / 4;
    for (int pass = 0; pass < 2; pass++) {
        for (int k = 0; k < nb; k++) {
            const int *b = &boxes[4 * k];
            for (int by = b[1] / bs; by <= b[3] / bs; by++)
                for (int bx = b[0] / bs; bx <= b[2] / bs; bx++) {
                    size_t q = (size_t)by * nbx + bx;
                    if (pass == 0) cnt[q + 1]++; else items[start[q] + cnt[q]++] = k;
                }
        }
        if (pass == 0) {
            start.assign(cnt.size(), 0);
            for (size_t q = 1; q < cnt.size(); q++) start[q] = start[q - 1] + cnt[q];
            items.resize(start.back());
            std::fill(cnt.begin(), cnt.end(), 0);
        }
    }
}

// LoadBalance(procIDs, grids) (src/AmrHydro.cpp:4283, 4929): here the boxes in the order given, cut into `world` runs of about equal cell
// counts (a box goes to the rank its middle cell falls to): deterministic, contiguous, the same on every rank.  Called BEFORE the plans are
// built: every plan entry is kept by the rank that executes it
int part_setup(suhmo_hier *H, int l)
{
    HLev &V = H->lev[l];
    const int nb = (int)V.box.size(), W = H->world;
    V.part = H->part;
    if (!V.part) return 0;
    long total = 0;
    for (int k = 0; k < nb; k++) { const int *b = &V.b4[4 * k]; total += (long)(b[2] - b[0] + 1) * (b[3] - b[1] + 1); }
    V.owner.assign(nb, 0);
    long before = 0;
    int prev = 0;
    for (int k = 0; k < nb; k++) {
        const int *b = &V.b4[4 * k];
        const long c = (long)(b[2] - b[0] + 1) * (b[3] - b[1] + 1);
        const int r = std::max(prev, std::min(W - 1, (int)(((before + c / 2) * W) / total)));
        V.owner[k] = prev = r;
        if (r == H->rank) V.owned_cells += c;
        before += c;
    }
    V.own.assign(W + 1, nb);
    for (int r = 0; r < W; r++) V.own[r] = (int)(std::lower_bound(V.owner.begin(), V.owner.end(), r) - V.owner.begin());
    V.b0 = V.own[H->rank]; V.nown = V.own[H->rank + 1] - V.b0;
    V.held.assign(nb, 0);
    for (int k = V.b0; k < V.b0 + V.nown; k++) V.held[k] = 1;
    return 0;
}

// ------------------------------------------------------------------ plan building (host)
// transfers (owner, cell, reader) of one kind -> this rank's part of the exchange: the cells it packs (what anybody reads of its boxes, sorted:
// position = rank in that order), the cells it unpacks into its mirrors of V's boxes (marked as held), the longest segment
static int make_sync(suhmo_hier *H, HLev &V, std::vector<Xf> &x, Sync &S)
{
    const int me = H->rank;
    auto key = [](const Xf &a, const Xf &b) { return a.owner != b.owner ? a.owner < b.owner : a.b != b.b ? a.b < b.b : a.off != b.off ? a.off < b.off : a.reader < b.reader; };
    std::sort(x.begin(), x.end(), key);
    x.erase(std::unique(x.begin(), x.end(), [](const Xf &a, const Xf &b) { return a.owner == b.owner && a.b == b.b && a.off == b.off && a.reader == b.reader; }), x.end());
    std::vector<Ref> send; std::vector<SyncRecv> recv;
    std::vector<long> cnt(H->world, 0);
    for (size_t t = 0; t < x.size();) {                     // one cell of one owner, its readers
        size_t u = t;
        bool mine = false;
        while (u < x.size() && x[u].owner == x[t].owner && x[u].b == x[t].b && x[u].off == x[t].off) { mine = mine || x[u].reader == me; u++; }
        const int pos = (int)cnt[x[t].owner]++;
        if (x[t].owner == me) send.push_back(Ref{x[t].b, x[t].off});
        else if (mine) { recv.push_back(SyncRecv{Ref{x[t].b, x[t].off}, x[t].owner, pos}); V.held[x[t].b] = 1; }
        t = u;
    }
    S.stride = *std::max_element(cnt.begin(), cnt.end());
    return S.send.upload(send) | S.recv.upload(recv);
}
int build_plans(suhmo_hier *H, int l)
{
    HLev &F = H->lev[l], &C = H->lev[l - 1];
    const int nb = (int)F.box.size();
    std::vector<CopyEnt> ffs, ffc;
    std::vector<CfEnt> cf;
    std::vector<PwlEnt> pwl;
    std::vector<RectEnt> avg;
    std::vector<WinEnt> wing; std::vector<int> wing_box;
    F.win.resize(nb);
    size_t wtot = 0;
    // level 0 cut into rank strips: its cells are read through the shadow (offsets in H->vglob, collected in `needv`) and
    // written in the rank's own rows only
    const bool cut = C.l == 0 && dist_base(H);
    const DV sv = C.l == 0 ? base_of(H)->d[0].v : DV{};
    std::vector<int> needv;
    std::vector<int4> dirty0; std::vector<std::pair<int, int>> gcell;        // (level l == 1)
    std::vector<RectEnt> cover_full;
    auto note = [&](const Ref &r) { if (cut && r.b >= 0) needv.push_back(r.off); };
    // owner computes: who executes what.  ownF / ownC: the rank that holds box k of this level / box o of level l-1 (a replicated level:
    // every rank, i.e. "me"); a cell of a cut level 0 belongs to the strip its row lies in, and is READ through the shadow
    const bool P = F.part;
    const int me = H->rank;
    auto ownF = [&](int k) { return P ? F.owner[k] : me; };
    auto ownC = [&](int o) { return (P && C.l >= 1) ? C.owner[o] : me; };
    std::vector<Xf> x_side[2], x_all, x_cread, x_win, x_fface;
    std::vector<RectEnt> avg_cov, avg_put; std::vector<PutEnt> avg_get;
    std::vector<long> putpos(H->world, 0);
    auto good_cell = [&](int I, int J) -> bool {          // coarse cell (I,J) of level l-1 good for tangential stencils?
        if (!wrap_cell(H, C, I, J)) return false;
        return F.index.find(2 * I, 2 * J) < 0;
    };
    for (int k = 0; k < nb; k++) {
        const int *b = &F.b4[4 * k];
        const DV &v = F.box[k]->d[0].v;
        // ---- ghost ring: fine-fine copies, coarse-fine interpolation entries, linear fill entries
        for (int j = b[1] - 1; j <= b[3] + 1; j++)
            for (int i = b[0] - 1; i <= b[2] + 1; i++) {
                const bool gx = i < b[0] || i > b[2], gy = j < b[1] || j > b[3];
                if (!gx && !gy) continue;
                int iw = i, jw = j;
                if (!wrap_cell(H, F, iw, jw)) continue;                       // domain ghost
                const Ref mine = local_ref(F, k, i - b[0], j - b[1]);
                const int o = F.index.find(iw, jw);
                if (o >= 0) {
                    const DV &vo = F.box[o]->d[0].v;
                    CopyEnt e{mine, Ref{o, cidx(vo, iw - vo.i0, jw - vo.j0)}};
                    if (P && F.owner[o] != F.owner[k]) {                      // the source cell travels to the owner of the ghost
                        const Xf x{F.owner[o], e.s.b, e.s.off, F.owner[k]};
                        x_all.push_back(x);
                        if (!(gx && gy)) x_side[(iw + jw) & 1].push_back(x);
                    }
                    if (ownF(k) == me) (gx && gy ? ffc : ffs).push_back(e);
                    continue;
                }
                // coarse-fine cell
                {
                    PwlEnt p;
                    p.f = mine; p.par = (iw & 1) | ((jw & 1) << 1);
                    const int I = iw >> 1, J = jw >> 1;
                    for (int jj = -1; jj <= 1; jj++)
                        for (int ii = -1; ii <= 1; ii++) {
                            int In = I + ii, Jn = J + jj;
                            Ref r{-1, 0};
                            if (In >= 0 && In <= C.nxd - 1 && Jn >= 0 && Jn <= C.nyd - 1) {     // as or_pwl_fill: no periodic images
                                r = cell_ref(H, C, In, Jn);
                                if (r.b < 0) { suhmo_set_error("hier: level %d is not properly nested in level %d (linear fill stencil)", l, l - 1); return -1; }
                            }
                            p.c[(jj + 1) * 3 + (ii + 1)] = r;
                            note(r);
                            if (P && C.l >= 1 && r.b >= 0 && C.owner[r.b] != F.owner[k]) x_cread.push_back(Xf{C.owner[r.b], r.b, r.off, F.owner[k]});
                        }
                    p.sx = (I - 1 >= 0 && I + 1 <= C.nxd - 1) ? 0 : (I - 1 < 0 ? 1 : 2);
                    p.sy = (J - 1 >= 0 && J + 1 <= C.nyd - 1) ? 0 : (J - 1 < 0 ? 1 : 2);
                    if (ownF(k) == me) pwl.push_back(p);
                }
                if (gx && gy) continue;                                       // QuadCFInterp: sides only
                const int dir = gx ? 0 : 1, side = gx ? (i < b[0] ? 0 : 1) : (j < b[1] ? 0 : 1);
                const int g = dir == 0 ? i : j, t = dir == 0 ? j : i;
                CfEnt e;
                e.f = mine; e.step = (side == 0 ? 1 : -1) * (dir == 0 ? 1 : v.P);
                e.xsign = t & 1;
                const int icn = g >> 1, ict = t >> 1;
                auto good = [&](int o_) { return dir == 0 ? good_cell(icn, ict + o_) : good_cell(ict + o_, icn); };
                auto cref = [&](int o_) { return dir == 0 ? cell_ref(H, C, icn, ict + o_) : cell_ref(H, C, ict + o_, icn); };
                const bool lo = good(-1), hi = good(1);
                int need[3] = {0, 0, 0}, nneed = 1;
                if (lo && hi) { e.kind = 0; need[0] = -1; need[1] = 0; need[2] = 1; nneed = 3; }
                else if (hi) { if (good(2)) { e.kind = 1; need[1] = 1; need[2] = 2; nneed = 3; } else { e.kind = 2; need[1] = 1; nneed = 2; } }
                else if (lo) { if (good(-2)) { e.kind = 3; need[1] = -1; need[2] = -2; nneed = 3; } else { e.kind = 4; need[1] = -1; nneed = 2; } }
                else e.kind = 5;
                for (int m = 0; m < 3; m++) {
                    e.c[m] = m < nneed ? cref(need[m]) : Ref{0, 0};
                    if (m < nneed && e.c[m].b < 0) { suhmo_set_error("hier: level %d is not properly nested in level %d (coarse-fine stencil)", l, l - 1); return -1; }
                    if (m < nneed) note(e.c[m]);
                    if (m < nneed && P && C.l >= 1 && C.owner[e.c[m].b] != F.owner[k]) x_cread.push_back(Xf{C.owner[e.c[m].b], e.c[m].b, e.c[m].off, F.owner[k]});
                    if (m < nneed && C.l == 0) {                              // the coarse cell, wrapped into the domain (as cell_ref did)
                        int I = dir == 0 ? icn : ict + need[m], J = dir == 0 ? ict + need[m] : icn;
                        (void)wrap_cell(H, C, I, J);
                        gcell.push_back(std::make_pair(J, I));
                    }
                }
                if (ownF(k) == me) cf.push_back(e);
            }
        // ---- average / covered rectangles: coarsen(box) split over the boxes of level l-1
        const int ci0 = b[0] / 2, cj0 = b[1] / 2, ci1 = b[2] / 2, cj1 = b[3] / 2;
        auto split = [&](int I0, int J0, int I1, int J1, auto &&emit) -> int {     // region inside the domain
            if (C.l == 0) { emit(0, I0, J0, I1, J1); return 0; }
            long cells = 0;
            for (int by = J0 / C.index.bs; by <= J1 / C.index.bs; by++)
                for (int bx = I0 / C.index.bs; bx <= I1 / C.index.bs; bx++) {
                    size_t q = (size_t)by * C.index.nbx + bx;
                    for (int p = C.index.start[q]; p < C.index.start[q + 1]; p++) {
                        const int o = C.index.items[p];
                        const int *cb = &C.b4[4 * o];
                        // each box once: only from the bucket that holds the corner of the intersection
                        int a0 = std::max(I0, cb[0]), a1 = std::min(I1, cb[2]), c0 = std::max(J0, cb[1]), c1 = std::min(J1, cb[3]);
                        if (a0 > a1 || c0 > c1) continue;
                        if (a0 / C.index.bs != bx || c0 / C.index.bs != by) continue;
                        emit(o, a0, c0, a1, c1);
                        cells += (long)(a1 - a0 + 1) * (c1 - c0 + 1);
                    }
                }
            if (cells != (long)(I1 - I0 + 1) * (J1 - J0 + 1)) { suhmo_set_error("hier: level %d is not nested in level %d", l, l - 1); return -1; }
            return 0;
        };
        int rc = split(ci0, cj0, ci1, cj1, [&](int o, int a0, int c0, int a1, int c1) {
            if (cut) cover_full.push_back(RectEnt{k, 0, 0, cidx(H->vglob, a0, c0), a1 - a0 + 1, c1 - c0 + 1});
            const DV &vc = C.box[o]->d[0].v;
            // the piece by the rank that holds its coarse cells: a strip of a cut level 0 (its rows), the owner of coarse box o, or everybody
            const int r0 = (C.l == 0 && cut) ? c0 / sv.ny : 0, r1 = (C.l == 0 && cut) ? c1 / sv.ny : 0;
            for (int r = r0; r <= r1; r++) {
                int d0 = c0, d1 = c1, dest = ownC(o);
                if (C.l == 0 && cut) { d0 = std::max(c0, r * sv.ny); d1 = std::min(c1, r * sv.ny + sv.ny - 1); dest = r; }
                if (d0 > d1) continue;
                const int w = a1 - a0 + 1, h = d1 - d0 + 1, writer = ownF(k);
                const int foff = cidx(v, 2 * a0 - b[0], 2 * d0 - b[1]), coff = cidx(vc, a0 - vc.i0, d0 - vc.j0);
                if (dest == me) avg_cov.push_back(RectEnt{k, o, foff, coff, w, h});
                if (!P) { if (dest == me) avg.push_back(RectEnt{k, o, foff, coff, w, h}); continue; }      // a replicated level: every rank averages into what it holds
                if (writer == dest) { if (writer == me) avg.push_back(RectEnt{k, o, foff, coff, w, h}); continue; }
                // the owner of the fine box averages into its segment of an all-gather, the holder of the coarse cells takes them from there
                if (writer == me) avg_put.push_back(RectEnt{k, 0, foff, (int)putpos[writer], w, h});
                if (dest == me) avg_get.push_back(PutEnt{o, coff, writer, (int)putpos[writer], w, h});
                putpos[writer] += (long)w * h;
            }
        });
        if (rc) return rc;
        // ---- window: coarsen(box) grown by one cell, gathered from level l-1 (periodic images included)
        Win &w = F.win[k];
        w.i0 = ci0 - 1; w.j0 = cj0 - 1; w.nx = ci1 - ci0 + 3; w.ny = cj1 - cj0 + 3; w.base = wtot;
        if (ownF(k) == me) wtot += (size_t)w.nx * w.ny;                      // (only the windows of this rank's boxes exist)
        for (int sy = -1; sy <= 1; sy++)
            for (int sx = -1; sx <= 1; sx++) {
                if ((sx && !H->bc.periodic[0]) || (sy && !H->bc.periodic[1])) continue;
                // window cells [w.i0 .. ] that are images (shifted by sx nxd, sy nyd) of domain cells
                int I0 = std::max(w.i0, sx * C.nxd), I1 = std::min(w.i0 + w.nx - 1, sx * C.nxd + C.nxd - 1);
                int J0 = std::max(w.j0, sy * C.nyd), J1 = std::min(w.j0 + w.ny - 1, sy * C.nyd + C.nyd - 1);
                if (I0 > I1 || J0 > J1) continue;
                rc = split(I0 - sx * C.nxd, J0 - sy * C.nyd, I1 - sx * C.nxd, J1 - sy * C.nyd, [&](int o, int a0, int c0, int a1, int c1) {
                    const DV &vc = C.l == 0 ? H->vglob : C.box[o]->d[0].v;
                    if (C.l == 0) {                                           // the part of this window piece in this rank's rows
                        const int d0 = std::max(c0, sv.j0), d1 = std::min(c1, sv.j0 + sv.ny - 1);
                        if (d0 <= d1) dirty0.push_back(int4{a0, d0 - sv.j0, a1 - a0 + 1, d1 - d0 + 1});
                    }
                    if (cut) for (int J = c0; J <= c1; J++) for (int I = a0; I <= a1; I++) needv.push_back(cidx(vc, I, J));
                    if (P && C.l >= 1 && C.owner[o] != F.owner[k])
                        for (int J = c0; J <= c1; J++) for (int I = a0; I <= a1; I++) x_win.push_back(Xf{C.owner[o], o, cidx(vc, I - vc.i0, J - vc.j0), F.owner[k]});
                    if (ownF(k) != me) return;
                    wing.push_back(WinEnt{o, cidx(vc, a0 - vc.i0, c0 - vc.j0), (c0 + sy * C.nyd - w.j0) * w.nx + (a0 + sx * C.nxd - w.i0), a1 - a0 + 1, c1 - c0 + 1});
                    wing_box.push_back(k);
                });
                if (rc) return rc;
            }
    }
    // ---- reflux: faces grouped by the coarse cell they feed, in the order (fine box, direction, side)
    std::map<std::pair<int, int>, std::vector<Face>> by_target;
    std::vector<std::pair<int, int>> order;
    for (int k = 0; k < nb; k++) {
        const int *b = &F.b4[4 * k];
        const DV &v = F.box[k]->d[0].v;
        const int ci0 = b[0] / 2, cj0 = b[1] / 2, ci1 = b[2] / 2, cj1 = b[3] / 2;
        for (int dir = 0; dir < 2; dir++) {
            const int ndomc = dir == 0 ? C.nxd : C.nyd;
            for (int side = 0; side < 2; side++) {
                const int Fc = dir == 0 ? (side == 0 ? ci0 : ci1 + 1) : (side == 0 ? cj0 : cj1 + 1);
                const int outside = side == 0 ? Fc - 1 : Fc;
                if ((outside < 0 || outside > ndomc - 1) && !H->bc.periodic[dir]) continue;
                const int tlo = dir == 0 ? cj0 : ci0, thi = dir == 0 ? cj1 : ci1;
                for (int T = tlo; T <= thi; T++) {
                    const int oi = dir == 0 ? outside : T, oj = dir == 0 ? T : outside;
                    if (owner_of(H, F, 2 * oi, 2 * oj) >= 0) continue;                 // fine-fine side
                    Face f;
                    f.dir = dir; f.side = side; f.fb = k;
                    f.foff = dir == 0 ? cidx(v, 2 * Fc - b[0], 2 * T - b[1]) : cidx(v, 2 * T - b[0], 2 * Fc - b[1]);
                    f.hi = dir == 0 ? cell_ref(H, C, Fc, T) : cell_ref(H, C, T, Fc);
                    f.lo = dir == 0 ? cell_ref(H, C, Fc - 1, T) : cell_ref(H, C, T, Fc - 1);
                    if (f.hi.b < 0 || f.lo.b < 0) { suhmo_set_error("hier: level %d is not properly nested in level %d (reflux)", l, l - 1); return -1; }
                    note(f.hi); note(f.lo);
                    f.bq = f.hi;                                                       // the face is the low face of its high-side cell
                    Ref t = side == 0 ? f.lo : f.hi;
                    auto key = std::make_pair(t.b, t.off);
                    if (!by_target.count(key)) order.push_back(key);
                    by_target[key].push_back(f);
                }
            }
        }
    }
    std::vector<Target> targets; std::vector<Face> faces;
    for (auto &key : order) {
        auto &fv = by_target[key];
        Ref t{key.first, key.second};
        // the register of a coarse cell is added up by the rank that holds the cell: a strip of a cut level 0 (the cell of the shadow -> the
        // same cell of that strip), the owner of its box, or everybody
        int exec = me;
        if (cut) {
            const int J = t.off / H->vglob.P - H->vglob.gy, I = t.off % H->vglob.P - SUHMO_XOFF;
            exec = J / sv.ny;
            if (exec == me) t.off = cidx(sv, I, J - sv.j0);
        } else if (C.l >= 1) exec = ownC(t.b);
        if (P)
            for (const Face &f : fv) {
                if (F.owner[f.fb] != exec) {                            // the fine cells and faces the register reads (k_reflux)
                    const int Pf = F.box[f.fb]->d[0].v.P;
                    for (int kk = 0; kk < 2; kk++) {
                        const int idx = f.foff + (f.dir == 0 ? kk * Pf : kk);
                        x_fface.push_back(Xf{F.owner[f.fb], f.fb, idx, exec});
                        x_fface.push_back(Xf{F.owner[f.fb], f.fb, f.dir == 0 ? idx - 1 : idx - Pf, exec});
                    }
                }
                if (C.l >= 1) for (const Ref &r : {f.hi, f.lo}) if (C.owner[r.b] != exec) x_cread.push_back(Xf{C.owner[r.b], r.b, r.off, exec});
            }
        if (exec != me) continue;
        targets.push_back(Target{t, (int)faces.size(), (int)fv.size()});
        faces.insert(faces.end(), fv.begin(), fv.end());
    }
    if (cut) {
        std::sort(needv.begin(), needv.end());
        needv.erase(std::unique(needv.begin(), needv.end()), needv.end());
        const int N = (int)needv.size();
        // the shadow keeps only the rows that hold a needed cell, in ascending order (rows next to each other stay next to each other: the
        // window rectangles, whose every cell is needed, remain rectangles): every offset into level 0 the plans carry is mapped over
        const int Pg = H->vglob.P, gyg = H->vglob.gy;
        std::vector<int> rowc(H->vglob.nyg, -1);
        for (int t = 0; t < N; t++) rowc[needv[t] / Pg - gyg] = 0;
        int nrow = 0;
        for (int J = 0; J < H->vglob.nyg; J++) if (rowc[J] == 0) rowc[J] = nrow++;
        auto remap = [&](int off) { return rowc[off / Pg - gyg] * Pg + off % Pg; };
        for (CfEnt &e : cf) { const int nn = e.kind == 0 || e.kind == 1 || e.kind == 3 ? 3 : (e.kind == 5 ? 1 : 2); for (int m = 0; m < nn; m++) e.c[m].off = remap(e.c[m].off); }
        for (PwlEnt &q : pwl) for (int m = 0; m < 9; m++) if (q.c[m].b >= 0) q.c[m].off = remap(q.c[m].off);
        for (WinEnt &w : wing) w.coff = remap(w.coff);
        for (Face &f : faces) { f.hi.off = remap(f.hi.off); f.lo.off = remap(f.lo.off); f.bq.off = remap(f.bq.off); }
        std::vector<int> needc(N);
        for (int t = 0; t < N; t++) needc[t] = remap(needv[t]);
        H->shadow_rows = nrow; H->shadow_elems = (size_t)Pg * (size_t)(nrow + 1);
        if (H->need_c.upload(needc)) { suhmo_set_error("hier: plan upload failed"); return -2; }
        std::vector<int2> rl(N);
        H->seg.assign(H->world + 1, 0);
        for (int t = 0; t < N; t++) {
            const int J = needv[t] / H->vglob.P - H->vglob.gy;
            const int r = J / sv.ny;
            H->seg[r + 1]++;
            rl[t].x = r;
        }
        for (int r = 0; r < H->world; r++) { H->cnt_max = std::max<long>(H->cnt_max, H->seg[r + 1]); H->seg[r + 1] += H->seg[r]; }
        for (int t = 0; t < N; t++) rl[t].y = t - H->seg[rl[t].x];
        if (H->need.upload(needv) || H->need_rl.upload(rl) || H->cover_full.upload(cover_full)) { suhmo_set_error("hier: plan upload failed"); return -2; }
    }
    int rc = 0;
    if (!P) {   // the side copies by source cell: per box W, E (ny entries each), S, N (nx each)
        std::vector<int> pbase(nb);
        size_t tot = 0;
        for (int k = 0; k < nb; k++) { const DV &v = F.box[k]->d[0].v; pbase[k] = (int)tot; tot += 2 * (size_t)(v.nx + v.ny); }
        std::vector<int2> push(tot, int2{-1, 0});
        for (const CopyEnt &e : ffs) {
            const DV &vo = F.box[e.s.b]->d[0].v, &vk = F.box[e.d.b]->d[0].v;
            const int js = e.s.off / vo.P - vo.gy, is = e.s.off % vo.P - SUHMO_XOFF;      // the source cell in its box
            const int jd = e.d.off / vk.P - vk.gy, id = e.d.off % vk.P - SUHMO_XOFF;      // the ghost cell in its box
            int slot;
            if (id < 0) slot = vo.ny + js;                  // a W ghost is fed by a cell on the E side of its box
            else if (id >= vk.nx) slot = js;
            else if (jd < 0) slot = 2 * vo.ny + vo.nx + is; // an S ghost by a cell on the N side
            else slot = 2 * vo.ny + is;
            const bool ok = (id < 0 ? is == vo.nx - 1 : id >= vk.nx ? is == 0 : jd < 0 ? js == vo.ny - 1 : js == 0);
            int2 &q = push[pbase[e.s.b] + slot];
            if (!ok || q.x >= 0) { suhmo_set_error("hier: internal: fine-fine copy without a unique source side cell"); return -4; }
            q = int2{e.d.b, e.d.off};
        }
        rc |= F.push.upload(push); rc |= F.pbase.upload(pbase);
    }
    if (!P) {   // several sweeps per launch (suhmo_gsrb.hip:k_gsrb_box_m): for every position of a box grown by 8 cells the box that holds the cell
        constexpr int G = SUHMO_BOX_HALO;
        size_t tot = 0;
        std::vector<int> hb(nb);
        bool fits = true;
        for (int k = 0; k < nb; k++) { const DV &v = F.box[k]->d[0].v; hb[k] = (int)tot; tot += (size_t)(v.nx + 2 * G) * (v.ny + 2 * G);
                                       fits = fits && v.nx >= 2 && v.ny >= 2; }
        if (fits && tot < (1u << 30)) {
            std::vector<int2> hv(tot);
            for (int k = 0; k < nb; k++) {
                const int *b = &F.b4[4 * k];
                const DV &v = F.box[k]->d[0].v;
                const int EW = v.nx + 2 * G;
                for (int ej = 0; ej < v.ny + 2 * G; ej++)
                    for (int ei = 0; ei < EW; ei++) {
                        int iw = b[0] - G + ei, jw = b[1] - G + ej;
                        int2 h = int2{-1, 0};
                        if (wrap_cell(H, F, iw, jw)) {
                            const int o = F.index.find(iw, jw);
                            if (o >= 0) { const DV &vo = F.box[o]->d[0].v; h = int2{o, cidx(vo, iw - vo.i0, jw - vo.j0)}; }
                        }
                        hv[hb[k] + (size_t)ej * EW + ei] = h;
                    }
            }
            rc |= F.halo.upload(hv); rc |= F.hbase.upload(hb);
            F.halo_ok = true;
        }
    }
    rc |= F.ff_side.upload(ffs);
    { std::vector<CopyEnt> all(ffs); all.insert(all.end(), ffc.begin(), ffc.end()); rc |= F.ff_all.upload(all); } rc |= F.cf.upload(cf); rc |= F.pwl.upload(pwl);
    rc |= F.avg.upload(avg); rc |= F.wing.upload(wing); rc |= F.targets.upload(targets); rc |= F.faces.upload(faces);
    rc |= F.avg_cov.upload(avg_cov);
    for (auto &e : avg_cov) { F.cov_w = std::max(F.cov_w, e.w); F.cov_h = std::max(F.cov_h, e.h); }
    if (P) {
        rc |= F.avg_put.upload(avg_put); rc |= F.avg_get.upload(avg_get);
        F.put_stride = *std::max_element(putpos.begin(), putpos.end());
        for (auto &e : avg_put) { F.put_w = std::max(F.put_w, e.w); F.put_h = std::max(F.put_h, e.h); F.put_mine += (long)e.w * e.h; }
        for (auto &e : avg_get) { F.get_w = std::max(F.get_w, e.w); F.get_h = std::max(F.get_h, e.h); }
        std::vector<Xf> x_sides(x_side[0]); x_sides.insert(x_sides.end(), x_side[1].begin(), x_side[1].end());
        rc |= make_sync(H, F, x_side[0], F.sy_side[0]); rc |= make_sync(H, F, x_side[1], F.sy_side[1]); rc |= make_sync(H, F, x_sides, F.sy_sides);
        rc |= make_sync(H, F, x_all, F.sy_all); rc |= make_sync(H, F, x_fface, F.sy_fface);
        if (C.l >= 1) { rc |= make_sync(H, C, x_cread, F.sy_cread); rc |= make_sync(H, C, x_win, F.sy_win); }
        H->side_bytes[l] = 8 * (long)std::max(F.sy_side[0].send.n, F.sy_side[1].send.n);
    }
    if (C.l == 0) {
        std::sort(gcell.begin(), gcell.end());
        gcell.erase(std::unique(gcell.begin(), gcell.end()), gcell.end());
        std::vector<int2> gc;
        for (auto &q : gcell) if (q.first >= sv.j0 && q.first < sv.j0 + sv.ny) gc.push_back(int2{q.second, q.first - sv.j0});   // own rows, local (i, j)
        rc |= F.gcells.upload(gc); rc |= F.dirty0.upload(dirty0);
        F.dirty_w = F.dirty_h = 0;
        for (auto &r : dirty0) { F.dirty_w = std::max(F.dirty_w, r.z); F.dirty_h = std::max(F.dirty_h, r.w); }
    }
    if (rc) { suhmo_set_error("hier: plan upload failed"); return -2; }
    F.avg_w = F.avg_h = F.wing_w = F.wing_h = 0;
    for (auto &e : avg) { F.avg_w = std::max(F.avg_w, e.w); F.avg_h = std::max(F.avg_h, e.h); }
    for (auto &e : wing) { F.wing_w = std::max(F.wing_w, e.w); F.wing_h = std::max(F.wing_h, e.h); }
    {   // the pieces of a box's window are consecutive (the boxes were visited in order)
        std::vector<int> ws(nb + 1, 0);
        for (int b : wing_box) ws[b + 1]++;
        for (int k = 0; k < nb; k++) ws[k + 1] += ws[k];
        for (size_t t = 1; t < wing_box.size(); t++) if (wing_box[t] < wing_box[t - 1]) { suhmo_set_error("hier: internal: window pieces out of order"); return -4; }
        if (F.wstart.upload(ws)) { suhmo_set_error("hier: plan upload failed"); return -2; }
        for (const Win &w : F.win) F.win_max = std::max(F.win_max, w.nx * w.ny);
    }
    F.winelems = wtot;
    if (hipMalloc(&F.winbuf, std::max<size_t>(1, wtot) * sizeof(double)) != hipSuccess) { suhmo_set_error("hier: window allocation failed"); return -2; }
    (void)hipMemset(F.winbuf, 0, std::max<size_t>(1, wtot) * sizeof(double));
    if (hipMalloc(&F.d_win, std::max<size_t>(1, F.win.size()) * sizeof(Win)) != hipSuccess) return -2;
    if (hipMalloc(&F.d_wing_box, std::max<size_t>(1, wing_box.size()) * sizeof(int)) != hipSuccess) return -2;
    if (hipMemcpy(F.d_win, F.win.data(), F.win.size() * sizeof(Win), hipMemcpyHostToDevice) != hipSuccess) return -2;
    if (!wing_box.empty() && hipMemcpy(F.d_wing_box, wing_box.data(), wing_box.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return -2;
    return 0;
}
}  // namespace hier
