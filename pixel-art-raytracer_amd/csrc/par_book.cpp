// par_book.cpp — the host's scene bookkeeping (par_book.h).
#include "par_book.h"
#include "par_internal.h"

using S = par_book_state;

// The cull and range math of alt:202-240 for one AABB. `items`: the render work items it can cause: its sprite
// rectangle (ex wide, ey + ez tall, alt:310-317) is cut by the screen columns it reaches into that many pieces, each
// visited in whole 64-pixel chunks: sum of ceil(area_i / 64) <= floor(area / 64) + pieces. (A column switches to
// visiting its whole tile only when that takes fewer chunks.)
static par_footprint footprint_of(const par_book& b, const par_aabb& a) {
    const int W = b.W, H = b.H, L = b.L, B = b.B;
    par_footprint f;
    const int minx = a.px, miny = a.py, minz = a.pz;
    const int maxx = minx + a.ex, maxy = miny + a.ey, maxz = minz + a.ez;
    if ((maxx < 0) || (minx >= W) || (maxy < 0 - maxz) || (miny >= H - minz + B) || (maxz < -a.ez - B) ||
        (minz > L + B)) {
        return f;
    }
    const int x0 = std::max(0, minx / B), y0 = std::max(0, (H - maxy - maxz) / B), z0 = std::max(0, minz / B);
    const int x1 = std::min(b.gx, (maxx + B - 1) / B), y1 = std::min(b.gy, (H - miny - minz + B - 1) / B);
    const int z1 = std::min(b.gz, (maxz + B - 1) / B);
    if (x1 <= x0 || y1 <= y0 || z1 <= z0) return f;
    f.x0 = (int16_t)x0; f.x1 = (int16_t)x1; f.y0 = (int16_t)y0; f.y1 = (int16_t)y1;
    f.nz = z1 - z0;
    f.items = (int32_t)((int)a.ex * ((int)a.ey + (int)a.ez) / 64 + f.cols());
    f.px = a.px; f.ex = a.ex;
    f.row0 = H - ((int)a.py + a.ey + a.pz + a.ez);
    f.rh = (int)a.ey + (int)a.ez;
    return f;
}

// What an entity of these extents can cause at most, wherever it stands: an interval of length d meets at most
// ceil(d / B) + 1 bins of width B (alt:222-240), its sprite rectangle is ex x (ey + ez) pixels (alt:310-317).
static par_bound bound_of(const par_book& b, const par_aabb& a) {
    const int64_t nx = std::min<int64_t>(b.gx, ((int)a.ex + b.B - 1) / b.B + 1);
    const int64_t ny = std::min<int64_t>(b.gy, ((int)a.ey + (int)a.ez + b.B - 1) / b.B + 1);
    const int64_t nz = std::min<int64_t>(b.gz, ((int)a.ez + b.B - 1) / b.B + 1);
    return par_bound{nx * ny * nz, nx * ny, (int64_t)a.ex * ((int)a.ey + (int)a.ez) / 64 + nx * ny};
}

// Adds (sign = +1) or removes (-1) a footprint in both per-column histograms. A column whose pairs exceed PAR_COL_NB
// (<= PAR_COL_ENT) may overflow its record; while there is none, no column can, and the frame needs no launch for the
// overflow list.
void par_book::col_hist(const par_footprint& f, int sign) {
    constexpr int kSure = PAR_COL_NB < PAR_COL_ENT ? PAR_COL_NB : PAR_COL_ENT;
    for (int x = f.x0; x < f.x1; x++) {
        const int cx0 = x * B, tw = std::min(B, W - cx0);
        const int w = std::min(f.px + f.ex, cx0 + tw) - std::max((int)f.px, cx0);
        for (int y = f.y0; y < f.y1; y++) {
            int32_t& n = colpairs[(size_t)x * gy + y];
            const bool was = n > kSure;
            n += sign * f.nz;
            cols_over += (int)(n > kSure) - (int)was;
            const int ry0 = y * B, th = std::min(B, H - ry0);
            const int h = std::min(f.row0 + f.rh, ry0 + th) - std::max(f.row0, ry0);
            if (w > 0 && h > 0) {
                const int tile_chunks = (tw * th + 63) / 64;
                int32_t& k = colchunks[(size_t)x * gy + y];
                const bool could = k >= tile_chunks;
                k += sign * ((w * h + 63) / 64);
                cols_tileable += (int)(k >= tile_chunks) - (int)could;
            }
        }
    }
}

// Both per-column histograms from the footprints: then everything is current.
void par_book::rebuild_hist() {
    colpairs.assign((size_t)gx * gy, 0);
    colchunks.assign((size_t)gx * gy, 0);
    cols_over = cols_tileable = 0;
    for (const par_footprint& f : fp) col_hist(f, +1);
    state = S::CURRENT;
}

void par_book::refresh(par_book_state lag) {
    if (state <= lag) return;
    exact = par_bound{0, 0, 0};
    for (size_t i = 0; i < aabbs.size(); i++) {
        fp[i] = footprint_of(*this, aabbs[i]);
        exact += fp[i].bound();
    }
    rebuild_hist();
}

const par_book_plan& par_book::plan(par_change kind, const par_aabb* a, int first, int n) {
    refresh(kind == par_change::UPDATE ? S::CURRENT : kind == par_change::STAGE ? S::HIST_BEHIND : S::EXTENTS_ONLY);
    par_book_plan& p = plan_;
    const bool whole = kind == par_change::SET;
    p.kind = kind; p.aabbs = a; p.first = first; p.n = n;
    par_bound ex = whole ? par_bound{0, 0, 0} : exact, et = whole ? par_bound{0, 0, 0} : extent;
    const par_aabb* old = whole ? nullptr : aabbs.data() + first;
    if (kind != par_change::ASYNC) {
        p.fp.resize((size_t)n);
        par_footprint* out = p.fp.data();
        for (int i = 0; i < n; i++) {
            const par_footprint f = footprint_of(*this, a[i]);
            out[i] = f;
            ex += f.bound();
            if (old) ex -= fp[(size_t)(first + i)].bound();
        }
    }
    for (int i = 0; i < n; i++) {  // (extents rarely change)
        if (old && old[i].ex == a[i].ex && old[i].ey == a[i].ey && old[i].ez == a[i].ez) continue;
        et += bound_of(*this, a[i]);
        if (old) et -= bound_of(*this, old[i]);
    }
    p.exact = ex; p.extent = et;
    if (kind == par_change::ASYNC) ex = et;  // (need: the extents alone)
    p.need = par_bound{std::max(ex.pairs, et.pairs), std::max(ex.cols, et.cols), std::max(ex.items, et.items)};
    return p;
}

// [first, first + count) into the set: merged with every range it overlaps or touches, put in its place, and, should
// that make one range too many, the two neighbours with the smallest gap between them joined (the gap's indices
// then count as rewritten: more is cleared, never less).
void par_dirty_set::add(int first, int count) {
    if (count <= 0) return;
    int32_t a = first, b = first + count;
    int m = 0;
    for (int i = 0; i < n; i++) {
        if (hi[i] < a || lo[i] > b) {
            lo[m] = lo[i];
            hi[m++] = hi[i];
        } else {
            a = std::min(a, lo[i]);
            b = std::max(b, hi[i]);
        }
    }
    int at = m;
    for (; at > 0 && lo[at - 1] > a; at--) {
        lo[at] = lo[at - 1];
        hi[at] = hi[at - 1];
    }
    lo[at] = a;
    hi[at] = b;
    n = m + 1;
    if (n <= MAX) return;
    int best = 0;
    for (int i = 1; i + 1 < n; i++) {
        if (lo[i + 1] - hi[i] < lo[best + 1] - hi[best]) best = i;
    }
    hi[best] = hi[best + 1];
    for (int i = best + 1; i + 1 < n; i++) {
        lo[i] = lo[i + 1];
        hi[i] = hi[i + 1];
    }
    n--;
}

void par_book::commit() {
    par_book_plan& p = plan_;
    if (p.kind == par_change::SET) dirty.mark_all();  // (the count and the sprite ids may have changed too)
    else dirty.add(p.first, p.n);
    if (p.kind != par_change::ASYNC) exact = p.exact;
    extent = p.extent;
    if (p.kind == par_change::SET) {
        aabbs.assign(p.aabbs, p.aabbs + p.n);
        fp.swap(p.fp);
        return rebuild_hist();
    }
    std::copy(p.aabbs, p.aabbs + p.n, aabbs.begin() + p.first);
    if (p.kind == par_change::UPDATE) {
        for (int i = 0; i < p.n; i++) {
            col_hist(fp[(size_t)(p.first + i)], -1);
            col_hist(p.fp[(size_t)i], +1);
        }
    }
    if (p.kind != par_change::ASYNC) std::copy(p.fp.begin(), p.fp.begin() + p.n, fp.begin() + p.first);
    state = std::max(state, p.kind == par_change::UPDATE  ? S::CURRENT
                            : p.kind == par_change::STAGE ? S::HIST_BEHIND : S::EXTENTS_ONLY);
}

const par_bound& par_book::capture() {
    refresh(S::CURRENT);
    // Head-room for moving primitives: pair counts of later frames are only bounded by the pool. Wherever the
    // entities move, each reaches at most cols_max screen columns (cull and ranges of alt:212-240).
    const int64_t pairs = exact.pairs * 2 + 4096;
    const int64_t cols_max = (int64_t)((PAR_SPRITE_W + B - 1) / B + 1) * ((PAR_SPRITE_H + B - 1) / B + 1);
    const int64_t items = (int64_t)aabbs.size() * ((int64_t)PAR_SPRITE_W * PAR_SPRITE_H / 64 + cols_max);
    return graph = par_bound{pairs, pairs, std::min(items, max_items())};
}

// One shard of the render work-item list holds the items of the columns whose index is congruent to it: at most
// every item of the frame, and at most its share of the occupied columns (<= `cols`), each visited as a whole tile.
int64_t par_book::items_per_shard(int64_t items, int64_t cols) const {
    cols = std::min<int64_t>(cols, (int64_t)gx * gy);
    return std::min(items, (cols / PAR_ITEM_SHARDS + 1) * tile_chunks());
}
