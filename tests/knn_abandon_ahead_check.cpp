// knn_abandon_ahead_check.cpp -- stand-alone check of the predictor of the abandon checkpoint's head prefetch (knn_plan.h:
// knn_ahead_initial, knn_ahead_next, knn_ahead_speculate, knn_ahead_walk, knn_abandon_ahead, knn_ahead_counter), driven by
// tests/test_knn_abandon_ahead_plan.py.  No GPU, no HIP: it includes the planner header alone -- the kernel reads the same text.
//
// A chunk of tiles with a given outcome sequence (L leave, S stay, U untested) is walked through the shared predictor; the heads used,
// the heads wasted and the exposed DMA barriers ("bubbles") are compared with expectations written out by hand:
//   * every tile leaves;  every tile stays;  strict alternation, beginning either way;
//   * a stay at the first tile;  a stay at the last tile;
//   * untested tiles in between (they neither consult nor update the prediction);
//   * a one-tile chunk (never speculates);
//   * the same sequences with the option off: nothing used, nothing wasted, one bubble per leaving tile that has a next tile.
// Then which launches prefetch, and where their counters live.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../include/radad_hip.h"
#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static AheadCounts walk(const char* seq, bool on = true) {
    std::vector<int> o;
    for (const char* c = seq; *c; ++c) o.push_back(*c == 'L' ? KNN_AHEAD_LEAVE : *c == 'S' ? KNN_AHEAD_STAY : KNN_AHEAD_UNTESTED);
    return knn_ahead_walk(o.data(), (int)o.size(), on);
}
static void expect(const char* seq, bool on, int64_t used, int64_t wasted, int64_t bubbles) {
    const AheadCounts c = walk(seq, on);
    printf("walk %s %d %lld %lld %lld\n", seq, on ? 1 : 0, (long long)c.used, (long long)c.wasted, (long long)c.bubbles);
    CHECK(c.used == used && c.wasted == wasted && c.bubbles == bubbles, "%s (option %d): used %lld wasted %lld bubbles %lld, expected %lld %lld %lld", seq,
          on ? 1 : 0, (long long)c.used, (long long)c.wasted, (long long)c.bubbles, (long long)used, (long long)wasted, (long long)bubbles);
}

int main() {
    // ---- the rule itself
    CHECK(knn_ahead_initial(), "the open gate is evidence: the first tested tile is predicted to leave");
    CHECK(knn_ahead_next(true, true) && knn_ahead_next(false, true) && !knn_ahead_next(true, false) && !knn_ahead_next(false, false), "the last tested tile decides");
    CHECK(knn_ahead_speculate(true, true) && !knn_ahead_speculate(true, false) && !knn_ahead_speculate(false, true) && !knn_ahead_speculate(false, false),
          "a head is fetched for a predicted leave that has a next tile");
    // ---- walks, option on: (used, wasted, bubbles)
    expect("LLLLL", true, 4, 0, 0);          // the last tile has no next one: nothing to fetch, nothing to wait for
    expect("SSSSS", true, 0, 1, 1);          // the first is mis-predicted, then the prediction is "stays"
    expect("LSLSL", true, 1, 2, 3);          // L used | S wasted (bubble) | L not predicted (bubble) | S wasted (bubble) | L last: "the last
                                             // tested tile left" is wrong every time under strict alternation
    expect("SLSLS", true, 0, 2, 4);          // S wasted | L bubble | S wasted | L bubble | S last: no next tile, no head
    expect("LSLSLS", true, 1, 2, 4);         // as LSLSL, then | L (5th) not predicted, has a next: bubble | S last
    expect("SLLLL", true, 2, 1, 2);          // S wasted | L bubble (prediction was "stays") | L used | L used | L last
    expect("LLLLS", true, 4, 0, 0);          // the last tile never speculates: a stay there wastes nothing
    expect("LULUL", true, 2, 0, 0);          // the untested tiles run the plain pattern; the tested ones around them: used, used, last
    expect("SUULL", true, 0, 1, 2);          // S wasted | U U: the prediction stays "stays" | L bubble | L last
    expect("LUSUL", true, 1, 1, 1);          // L used | S wasted | L last
    expect("UUUUU", true, 0, 0, 0);
    expect("L", true, 0, 0, 0);              // a one-tile chunk
    expect("S", true, 0, 0, 0);
    expect("U", true, 0, 0, 0);
    expect("", true, 0, 0, 0);
    // ---- option off: today's pattern
    expect("LLLLL", false, 0, 0, 4);
    expect("SSSSS", false, 0, 0, 0);
    expect("LSLSL", false, 0, 0, 2);
    expect("LULUL", false, 0, 0, 2);
    expect("L", false, 0, 0, 0);
    // ---- every sequence of up to 9 tiles: a head is fetched only by a tested tile that has a next one; with the option off every leaving
    // tile that has a next one pays the bubble; with it on each of them either used a head or paid the bubble, never both
    for (int len = 0; len <= 9; ++len) {
        int64_t total = 1;
        for (int i = 0; i < len; ++i) total *= 3;
        for (int64_t code = 0; code < total; ++code) {
            char seq[16];
            int64_t c = code;
            int tested_with_next = 0, leaves_with_next = 0;
            for (int i = 0; i < len; ++i, c /= 3) {
                seq[i] = "LSU"[c % 3];
                if (seq[i] != 'U' && i + 1 < len) ++tested_with_next;
                if (seq[i] == 'L' && i + 1 < len) ++leaves_with_next;
            }
            seq[len] = 0;
            const AheadCounts on = walk(seq, true), off = walk(seq, false);
            CHECK(on.used + on.wasted <= tested_with_next, "%s", seq);
            CHECK(off.used == 0 && off.wasted == 0 && off.bubbles == leaves_with_next, "%s", seq);
            CHECK(on.used + (on.bubbles - on.wasted) == leaves_with_next, "%s: every leaving tile with a next one either used a head or paid the bubble", seq);
        }
    }
    // ---- which launches prefetch
    CHECK(knn_abandon_ahead(1, 1, false, 0) && knn_abandon_ahead(1, 2, false, KNN_DEAL_SETS - 1), "an abandoning launch that is not dealt");
    CHECK(!knn_abandon_ahead(0, 1, false, 0), "the option off");
    CHECK(!knn_abandon_ahead(1, 0, false, 0), "a launch that does not abandon (RADAD_KNN_OPT_ABANDON 0, the sample, a K split)");
    CHECK(!knn_abandon_ahead(1, 1, true, 0), "a dealt launch keeps its two barriers");
    CHECK(!knn_abandon_ahead(1, 1, false, KNN_DEAL_SETS) && !knn_abandon_ahead(1, 1, false, -1), "a launch without a counter set");
    // ---- the counters: inside the launch's own set, clear of the deferral's
    std::set<int> seen;
    for (int s = 0; s < KNN_DEAL_SETS; ++s) {
        const int a = knn_ahead_counter(s);
        CHECK(a >= knn_deal_counter(s, 0, 0) && a + 1 < knn_deal_counter(s, 0, 0) + KNN_DEAL_SLOTS * KNN_DEAL_MAX_QTILES && a + 1 < KNN_DEAL_COUNTERS, "set %d", s);
        CHECK(seen.insert(a).second && seen.insert(a + 1).second, "set %d", s);
        CHECK(seen.insert(knn_defer_tasks_counter(s)).second, "set %d: the deferral's task counter", s);
        for (int qt = 0; qt < KNN_DEFER_MAX_QTILES; ++qt) CHECK(seen.insert(knn_defer_counter(s, qt)).second, "set %d: list counter %d", s, qt);
    }
    printf("define %d\n", RADAD_KNN_OPT_ABANDON_AHEAD);
    if (failures) { printf("knn_abandon_ahead_check: %d FAILED\n", failures); return 1; }
    printf("knn_abandon_ahead_check: ok\n");
    return 0;
}
