// dirty_check.cpp — drives the set of rewritten entity ranges (par_dirty_set, csrc/par_book.h) that a kept frame clears
// by: seeded random sequences of range updates against a plain bitmap of the indices added, and the book's commit()
// feeding it. Host code only; prints "<n> checks, <m> failures".
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "par_book.h"

static int checks = 0, failures = 0;

static void check(bool ok, const char* what, int a = 0, int b = 0) {
    checks++;
    if (ok) return;
    failures++;
    if (failures <= 20) std::printf("FAIL %s (%d, %d)\n", what, a, b);
}

// The invariants of the representation: at most MAX ranges, each non-empty, ascending, no two touching.
static void check_shape(const par_dirty_set& s) {
    check(s.n >= 0 && s.n <= par_dirty_set::MAX, "count within MAX", s.n);
    for (int i = 0; i < s.n; i++) {
        check(s.lo[i] < s.hi[i], "a range is not empty", s.lo[i], s.hi[i]);
        if (i) check(s.hi[i - 1] < s.lo[i], "ranges ascend and do not touch", s.hi[i - 1], s.lo[i]);
    }
}

static void random_sequences() {
    std::mt19937 rng(20240607u);
    const int N = 400;
    for (int round = 0; round < 300; round++) {
        par_dirty_set s;
        std::vector<char> added((size_t)N, 0);
        check(s.empty() && !s.all(), "a new set is empty");
        const int steps = 1 + (int)(rng() % 12);
        for (int k = 0; k < steps; k++) {
            const int first = (int)(rng() % N);
            const int count = (int)(rng() % 4 == 0 ? rng() % 40 : rng() % 3);  // (0 too: it adds nothing)
            const int n = std::min(count, N - first);
            const par_dirty_set before = s;
            s.add(first, n);
            for (int i = 0; i < n; i++) added[(size_t)(first + i)] = 1;
            check_shape(s);
            if (n == 0) check(s.n == before.n, "an empty update adds nothing");
            int exact = 0, in_set = 0;
            for (int e = 0; e < N; e++) {
                if (added[(size_t)e]) check(s.has(e), "merging never loses an index", e, k);
                exact += added[(size_t)e];
                in_set += s.has(e) ? 1 : 0;
            }
            // up to MAX separate runs are held exactly: nothing is merged before it has to be
            int runs = 0;
            for (int e = 0; e < N; e++) runs += added[(size_t)e] && (e == 0 || !added[(size_t)(e - 1)]);
            if (runs <= par_dirty_set::MAX && k < par_dirty_set::MAX) check(in_set == exact, "few runs are held exactly", in_set, exact);
            check(!s.has(-1) && !s.has(N), "nothing outside what was added");
        }
        s.clear();
        check(s.empty() && !s.has(0), "empty after clear()");
    }
}

static void closest_pair_is_merged() {
    par_dirty_set s;
    s.add(0, 1);
    s.add(100, 1);
    s.add(200, 1);
    s.add(300, 1);
    check(s.n == 4, "four single entities, four ranges", s.n);
    s.add(110, 1);  // a fifth: 100 and 110 are the closest pair
    check(s.n == 4 && s.lo[1] == 100 && s.hi[1] == 111, "the closest two become one", s.lo[1], s.hi[1]);
    check(s.has(105) && !s.has(50) && !s.has(150), "only the gap between them is taken in");
    s.add(1, 99);  // touches [0, 1) and [100, 111)
    check(s.n == 3 && s.lo[0] == 0 && s.hi[0] == 111, "a range that touches two joins them", s.n, s.hi[0]);
}

static void everything() {
    par_dirty_set s;
    s.add(5, 3);
    s.add(50, 2);
    s.mark_all();
    check(s.all() && s.n == 1, "everything is one range");
    s.add(7, 100);
    s.add(100000, 5);
    check(s.all() && s.n == 1, "everything absorbs all ranges", s.n);
    check(s.has(0) && s.has(1 << 30), "every index is in it");
    s.clear();
    check(s.empty() && !s.all(), "and it ends with the frame");
}

// The book feeds the set: an update of [first, first + n) adds that range whatever its kind, with the values it found
// too; par_set_entities marks everything. The context empties the set when it enqueues a frame (clear()).
static void book_feeds_the_set() {
    par_params p{};
    p.width = 488; p.height = 328; p.length = 320; p.bin_size = 40;
    const int gx = (p.width + 39) / 40, gy = (p.height + 39) / 40, gz = (p.length + 39) / 40;
    par_book book;
    book.init(p, gx, gy, gz);
    std::vector<par_aabb> a(20);  // (zeroed)
    for (int i = 0; i < 20; i++) {
        par_aabb& b = a[(size_t)i];
        b.px = (int16_t)(i * 20); b.py = 40; b.pz = 40;
        b.ex = 20; b.ey = 20; b.ez = 20;
    }
    book.plan(par_change::SET, a.data(), 0, 20);
    book.commit();
    check(book.dirty.all(), "par_set_entities marks everything");
    book.dirty.clear();  // a frame
    const par_change kinds[3] = {par_change::UPDATE, par_change::ASYNC, par_change::STAGE};
    for (int k = 0; k < 3; k++) {
        book.plan(kinds[k], a.data() + 3, 3, 2);  // identical values
        book.commit();
        check(book.dirty.n == 1 && book.dirty.lo[0] == 3 && book.dirty.hi[0] == 5, "an update adds its range", k, book.dirty.n);
        check(!book.dirty.has(2) && book.dirty.has(3) && book.dirty.has(4) && !book.dirty.has(5), "and no more", k);
        book.dirty.clear();
        check(book.dirty.empty(), "empty after a frame", k);
    }
    book.plan(par_change::UPDATE, a.data() + 10, 10, 1);
    check(book.dirty.empty(), "a plan that is not committed adds nothing");
    book.commit();
    book.plan(par_change::SET, a.data(), 0, 5);  // fewer entities: the nodes of 5..19 are still on the device
    book.commit();
    check(book.dirty.all() && book.dirty.has(19), "a smaller scene still covers the entities it dropped");
}

int main() {
    random_sequences();
    closest_pair_is_merged();
    everything();
    book_feeds_the_set();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
