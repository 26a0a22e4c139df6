// par_book.h — the host's scene bookkeeping: the entities' AABBs, the bins each reaches, the per-column histograms
// and the totals a frame's launches are sized and chosen by. Plain host C++ (no HIP calls); par_context keeps one.
// Its state, each lagging more than the one before:
//   CURRENT       everything is up to date.
//   HIST_BEHIND   footprints and exact totals are current, the per-column histograms are not (a captured graph does
//                 not read them, and keeping them costs a moving scene more host time per frame than the rest).
//   EXTENTS_ONLY  only the AABBs and the extent totals are current (no cull and range arithmetic per frame).
// The contract:
//   par_set_entities[_ref_layout]  -> CURRENT
//   par_update_aabbs (and the async call when it falls back to it) -> CURRENT (full refresh first)
//   par_update_aabbs_async         -> EXTENTS_ONLY
//   par_graph_capture[_lights]     -> CURRENT
//   par_graph_stage[_lights]       -> HIST_BEHIND; from EXTENTS_ONLY a full refresh first. A refused stage may leave
//                                     the state refreshed, but changes nothing else.
//   par_graph_launch               from EXTENTS_ONLY: CURRENT (full refresh); otherwise unchanged
// A scene change goes plan -> the caller checks capacity, grows pools by plan.need and copies to the device -> commit.
// A call refused or failed before its commit leaves the book as it was, but for a refresh.
#ifndef PAR_BOOK_H
#define PAR_BOOK_H

#include <stdint.h>
#include <algorithm>
#include <vector>

#include "par_raytracer.h"

// (entity, bin) pairs (alt:243-267), occupied screen columns and render work items (64-pixel chunks).
struct par_bound {
    int64_t pairs, cols, items;
    par_bound& operator+=(const par_bound& b) { pairs += b.pairs; cols += b.cols; items += b.items; return *this; }
    par_bound& operator-=(const par_bound& b) { pairs -= b.pairs; cols -= b.cols; items -= b.items; return *this; }
};

// The bins one entity is inserted into (cull and ranges of alt:202-240): bin columns [x0, x1) x [y0, y1), nz bins
// deep; empty when x1 <= x0. Everything the host sizes launches and lists with follows from it.
struct par_footprint {
    int16_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    int32_t nz = 0;
    int32_t items = 0;  // render work items (64-pixel chunks) the entity can cause, see footprint_of (par_book.cpp)
    int16_t px = 0, ex = 0;     // its sprite rectangle on screen (alt:310-317): columns [px, px + ex),
    int32_t row0 = 0, rh = 0;   // rows [row0, row0 + rh) = H - (py + ey + pz + ez) .. H - (py + pz)
    int32_t cols() const { return (x1 - x0) * (y1 - y0); }
    par_bound bound() const { return par_bound{(int64_t)cols() * nz, cols(), items}; }
};

enum class par_book_state : uint8_t { CURRENT, HIST_BEHIND, EXTENTS_ONLY };

// The whole scene (SET), or entities [first, first + n) by a blocking update, a graph stage or an async update.
enum class par_change : uint8_t { SET, UPDATE, STAGE, ASYNC };

struct par_book_plan {
    par_change kind = par_change::SET;
    const par_aabb* aabbs = nullptr; int first = 0, n = 0;  // the caller's, for entities [first, first + n)
    par_bound exact{}, extent{};      // the totals after the change (exact: not for ASYNC)
    par_bound need{};                 // what pools and lists must hold: the larger of the two, per component
    std::vector<par_footprint> fp;    // the new footprints (not for ASYNC); reused from call to call
};

// The entities rewritten since the context's last enqueued frame (what a kept frame, PAR_RENDER_KEPT_OUTPUTS, clears
// by): at most MAX disjoint index ranges [lo, hi), ascending, no two touching. One more is merged with whatever it
// touches; past MAX the two ranges with the smallest gap between them become one, so an index once added stays in the
// set until clear(). An update that rewrites the values it found still counts.
struct par_dirty_set {
    static constexpr int MAX = 4;
    static constexpr int32_t END = INT32_MAX;  // mark_all(): every index an entity can have, whatever the count becomes
    int n = 0;
    int32_t lo[MAX + 1] = {}, hi[MAX + 1] = {};
    void add(int first, int count);
    void mark_all() { n = 1; lo[0] = 0; hi[0] = END; }
    void clear() { n = 0; }
    bool empty() const { return n == 0; }
    bool all() const { return n == 1 && lo[0] == 0 && hi[0] == END; }
    bool has(int e) const {
        for (int i = 0; i < n; i++) {
            if (e >= lo[i] && e < hi[i]) return true;
        }
        return false;
    }
};

struct par_book {
    int W = 0, H = 0, L = 0, B = 0, gx = 0, gy = 0, gz = 0;
    par_book_state state = par_book_state::CURRENT;
    std::vector<par_aabb> aabbs;
    std::vector<par_footprint> fp;
    par_bound exact{};   // from the footprints: >= the frame's pairs, occupied columns and work items
    par_bound extent{};  // from the EXTENTS alone (bound_of): what pools and lists are sized by
    par_bound graph{};   // what a captured graph's launches are sized by (capture), for later frames too
    std::vector<int32_t> colpairs;   // (entity, bin) pairs per screen column (>= its occupied bins, >= its entries)
    int64_t cols_over = 0;           // columns with more pairs than a column record is sure to hold
    // 64-pixel chunks of the entities' sprite rectangles per screen column (what the column kernel adds up, over the
    // visible entries only, to choose between visiting a column entry by entry and as a whole tile), and the columns
    // where that reaches the tile's own chunks: only those can be visited as tiles
    std::vector<int32_t> colchunks;
    int64_t cols_tileable = 0;
    par_dirty_set dirty;  // fed by commit(); the context marks what does not come through the book and clears it per frame
    par_book_plan plan_;

    void init(const par_params& p, int x, int y, int z) {
        W = p.width; H = p.height; L = p.length; B = p.bin_size; gx = x; gy = y; gz = z;
    }
    // UPDATE refreshes to CURRENT first, STAGE out of EXTENTS_ONLY; commit applies the last plan.
    const par_book_plan& plan(par_change kind, const par_aabb* a, int first, int n);
    void commit();
    void refresh(par_book_state lag);  // a full refresh when the state lags more than `lag`
    const par_bound& capture();        // CURRENT, and `graph` for a graph captured now
    void col_hist(const par_footprint& f, int sign);
    void rebuild_hist();

    // What a frame reads. A captured graph's frames are sized by `graph`, others by the extents in EXTENTS_ONLY. The
    // launch shape (dense, chunks) reads cols_tileable and exact.items even where they lag behind the scene (the
    // former in HIST_BEHIND and EXTENTS_ONLY, the latter in EXTENTS_ONLY); what the launches hold never does.
    par_bound frame_bounds(bool graph_mode) const {
        return graph_mode ? graph : state == par_book_state::EXTENTS_ONLY ? extent : exact;
    }
    bool may_overflow() const { return cols_over > 0 || state != par_book_state::CURRENT; }
    bool dense() const { return cols_tileable >= std::max<int64_t>(16, (int64_t)gx * gy / 64); }
    // (no more than every column as a whole tile: the entities of a crowded small view overlap many times over)
    int64_t chunks() const { return std::min(exact.items, max_items()); }
    int64_t tile_chunks() const { return ((int64_t)B * B + 63) / 64; }
    int64_t max_items() const { return (int64_t)gx * gy * tile_chunks(); }  // every column visited as a whole tile
    int64_t items_per_shard(int64_t items, int64_t cols) const;
};

#endif
