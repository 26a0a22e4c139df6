// book_check.cpp — drives the host's scene bookkeeping (csrc/par_book.cpp) through seeded random sequences of the scene
// changes of its contract (par_book.h) and checks the book after every step against one built from scratch over the
// same AABBs. Host code only: tests/test_book_cpu.py builds and runs it without a GPU.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "par_book.h"

using S = par_book_state;

static int failures = 0, checks = 0;

#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        checks++;                                                                          \
        if (!(cond) && failures++ < 20) {                                                  \
            std::printf("FAIL line %d: %s; ", __LINE__, #cond);                            \
            std::printf(__VA_ARGS__);                                                      \
            std::printf("\n");                                                             \
        }                                                                                  \
    } while (0)

static bool eq(const par_bound& a, const par_bound& b) {
    return a.pairs == b.pairs && a.cols == b.cols && a.items == b.items;
}
static bool ge(const par_bound& a, const par_bound& b) {
    return a.pairs >= b.pairs && a.cols >= b.cols && a.items >= b.items;
}
static bool eq(const par_footprint& a, const par_footprint& b) {
    return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.nz == b.nz && a.items == b.items &&
           a.px == b.px && a.ex == b.ex && a.row0 == b.row0 && a.rh == b.rh;
}
static bool eq(const std::vector<par_footprint>& a, const std::vector<par_footprint>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        if (!eq(a[i], b[i])) return false;
    }
    return true;
}
static bool same_aabbs(const std::vector<par_aabb>& a, const std::vector<par_aabb>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(par_aabb)) == 0);
}
// Everything the book keeps but the plan.
static bool same_book(const par_book& a, const par_book& b) {
    return a.state == b.state && same_aabbs(a.aabbs, b.aabbs) && eq(a.fp, b.fp) && eq(a.exact, b.exact) &&
           eq(a.extent, b.extent) && eq(a.graph, b.graph) && a.colpairs == b.colpairs && a.colchunks == b.colchunks &&
           a.cols_over == b.cols_over && a.cols_tileable == b.cols_tileable;
}

struct view {
    int W, H, L, B;
};

struct driver {
    view v;
    std::mt19937 rng;
    par_book book;
    std::vector<par_aabb> mirror;  // what the book's AABBs must be
    S expect = S::CURRENT;
    int step = 0;

    int uni(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); }

    void init_book(par_book* b) const {
        par_params p{};
        p.width = v.W; p.height = v.H; p.length = v.L; p.bin_size = v.B;
        b->init(p, (v.W + v.B - 1) / v.B, (v.H + v.B - 1) / v.B, (v.L + v.B - 1) / v.B);
    }
    // Any extent the sprite takes, anywhere in and around the view (also wholly outside it).
    par_aabb random_aabb() {
        par_aabb a{};
        a.ex = (int16_t)uni(0, 20);
        a.ey = (int16_t)uni(0, 40);
        a.ez = (int16_t)uni(0, 40 - a.ey);
        a.px = (int16_t)uni(-80, v.W + 60);
        a.py = (int16_t)uni(-80, v.H + 60);
        a.pz = (int16_t)uni(-120, v.L + 100);
        return a;
    }
    // Mostly small steps (in and out of the view at its borders), some jumps, some new extents.
    par_aabb moved(par_aabb a) {
        const int k = uni(0, 9);
        if (k == 0) return random_aabb();
        const int d = k < 7 ? 5 : v.B;
        a.px = (int16_t)std::min(v.W + 200, std::max(-200, a.px + uni(-d, d)));
        a.py = (int16_t)std::min(v.H + 200, std::max(-200, a.py + uni(-d, d)));
        a.pz = (int16_t)std::min(v.L + 200, std::max(-200, a.pz + uni(-d, d)));
        if (k == 9) {
            a.ex = (int16_t)uni(0, 20);
            a.ey = (int16_t)uni(0, 40);
            a.ez = (int16_t)uni(0, 40 - a.ey);
        }
        return a;
    }

    void check(const char* what) {
        par_book scratch;  // the same AABBs, from scratch
        init_book(&scratch);
        scratch.plan(par_change::SET, mirror.data(), 0, (int)mirror.size());
        scratch.commit();
        const par_book& b = book;
        CHECK(b.state == expect, "%s step %d: state %d, expected %d", what, step, (int)b.state, (int)expect);
        CHECK(same_aabbs(b.aabbs, mirror), "%s step %d", what, step);
        CHECK(eq(b.extent, scratch.extent), "%s step %d: extent pairs %lld, from scratch %lld", what, step,
              (long long)b.extent.pairs, (long long)scratch.extent.pairs);
        if (b.state != S::EXTENTS_ONLY) {  // footprints and exact totals are current
            CHECK(eq(b.fp, scratch.fp), "%s step %d", what, step);
            CHECK(eq(b.exact, scratch.exact), "%s step %d: exact pairs %lld, from scratch %lld", what, step,
                  (long long)b.exact.pairs, (long long)scratch.exact.pairs);
        }
        if (b.state == S::CURRENT) {
            CHECK(b.colpairs == scratch.colpairs && b.cols_over == scratch.cols_over, "%s step %d", what, step);
            CHECK(b.colchunks == scratch.colchunks && b.cols_tileable == scratch.cols_tileable, "%s step %d", what, step);
            CHECK(ge(b.extent, b.exact), "%s step %d: extent below exact", what, step);
        }
        CHECK(eq(b.frame_bounds(false), b.state == S::EXTENTS_ONLY ? b.extent : b.exact), "%s step %d", what, step);
        CHECK(eq(b.frame_bounds(true), b.graph), "%s step %d", what, step);
        CHECK(b.may_overflow() == (b.cols_over > 0 || b.state != S::CURRENT), "%s step %d", what, step);
    }

    // A plan's totals and what pools must hold (before its commit).
    void check_plan(const par_book_plan& p, bool exact) {
        std::vector<par_aabb> after = mirror;
        if (p.kind == par_change::SET) after.assign(p.aabbs, p.aabbs + p.n);
        else std::copy(p.aabbs, p.aabbs + p.n, after.begin() + p.first);
        par_book scratch;
        init_book(&scratch);
        scratch.plan(par_change::SET, after.data(), 0, (int)after.size());
        scratch.commit();
        CHECK(eq(p.extent, scratch.extent), "plan step %d", step);
        if (exact) CHECK(eq(p.exact, scratch.exact), "plan step %d", step);
        const par_bound& e = exact ? p.exact : p.extent;
        CHECK(eq(p.need, par_bound{std::max(e.pairs, p.extent.pairs), std::max(e.cols, p.extent.cols),
                                   std::max(e.items, p.extent.items)}), "plan step %d", step);
    }

    void run(int steps) {
        init_book(&book);
        std::vector<par_aabb> a;
        for (step = 0; step < steps; step++) {
            const int n_all = (int)mirror.size();
            const int op = step == 0 ? 0 : uni(0, 99);
            if (op < 4) {  // par_set_entities
                a.resize((size_t)uni(0, 400));
                for (par_aabb& x : a) x = random_aabb();
                par_book before = book;
                check_plan(book.plan(par_change::SET, a.data(), 0, (int)a.size()), true);
                CHECK(same_book(book, before), "set plan, step %d", step);
                book.commit();
                mirror = a;
                expect = S::CURRENT;
                check("set");
                continue;
            }
            const int first = uni(0, n_all), n = uni(0, std::min(n_all - first, uni(0, 1) ? 8 : n_all));
            a.resize((size_t)n);
            for (int i = 0; i < n; i++) a[(size_t)i] = moved(mirror[(size_t)(first + i)]);
            if (op >= 80 && op < 88) {  // par_graph_launch
                book.refresh(S::HIST_BEHIND);
                if (expect == S::EXTENTS_ONLY) expect = S::CURRENT;
                check("launch");
                continue;
            }
            if (op >= 88 && op < 94) {  // par_graph_capture
                const par_bound& g = book.capture();
                expect = S::CURRENT;
                CHECK(g.pairs == book.exact.pairs * 2 + 4096 && g.cols == g.pairs && g.items <= book.max_items() &&
                      &g == &book.graph, "capture step %d", step);
                check("capture");
                continue;
            }
            // par_update_aabbs (also the async call's fall-back), par_update_aabbs_async, par_graph_stage, or (op >= 94)
            // any of them refused or failed after its plan: no commit
            const par_change kind = op < 24 || (op >= 94 && op % 3 == 0) ? par_change::UPDATE
                                    : op < 56 || (op >= 94 && op % 3 == 1) ? par_change::ASYNC : par_change::STAGE;
            const char* what = kind == par_change::UPDATE ? "update" : kind == par_change::ASYNC ? "async" : "stage";
            // the plan changes nothing but for the refresh it starts with (none for ASYNC)
            par_book before = book;
            if (kind == par_change::UPDATE) before.refresh(S::CURRENT);
            if (kind == par_change::STAGE) before.refresh(S::HIST_BEHIND);
            check_plan(book.plan(kind, a.data(), first, n), kind != par_change::ASYNC);
            CHECK(same_book(book, before), "%s plan, step %d", what, step);
            if (kind == par_change::UPDATE || (kind == par_change::STAGE && expect == S::EXTENTS_ONLY)) {
                expect = S::CURRENT;
            }
            if (op >= 94) {
                check("refused");
                continue;
            }
            expect = kind == par_change::UPDATE ? S::CURRENT : kind == par_change::ASYNC ? S::EXTENTS_ONLY
                                                                                          : S::HIST_BEHIND;
            book.commit();
            std::copy(a.begin(), a.end(), mirror.begin() + first);
            check(what);
        }
    }
};

int main() {
    const view views[] = {{480, 320, 320, 40}, {256, 256, 256, 8}, {1000, 700, 500, 32}, {97, 61, 83, 16},
                          {640, 400, 400, 160}, {333, 517, 129, 20}};
    unsigned seed = 20261016;
    for (const view& v : views) {
        for (int run = 0; run < 3; run++) {
            driver d{v, std::mt19937(seed++), par_book{}, {}, S::CURRENT, 0};
            d.run(400);
        }
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
