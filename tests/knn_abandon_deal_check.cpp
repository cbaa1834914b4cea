// knn_abandon_deal_check.cpp -- stand-alone check of the host side of the abandoning scan's ticket deal (knn_plan.h: knn_abandon_deal,
// knn_deal_ticket, knn_deal_granules, knn_deal_counter), driven by tests/test_knn_abandon_deal_plan.py.  No GPU, no HIP: it includes
// the planner header alone -- the kernel converts its tickets with the same text.
//
//   * the mapping: for 1 ... 5000 row tiles and every granule the planner can return, every ticket of every slot enumerated -- each row
//     tile covered exactly once, no ticket past the launch, a used-up slot stays used up, and any 40 consecutive tiles touch all eight
//     slots (a store filled cluster by cluster spreads over every XCD slot);
//   * the decision: dealt exactly when the launch abandons, has <= 8 query tiles, is one of the search's first KNN_DEAL_SETS launches,
//     the option is on and a resident workgroup would draw at least two granules -- for 1 ... 8 query tiles and 64, 104, 256 and 304 CUs;
//   * the counter sets: disjoint, inside KNN_DEAL_COUNTERS.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                        \
    do {                                                                                        \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    std::vector<int> granules;
    for (int g = KNN_DEAL_GRANULE; g >= 1; g /= 2) granules.push_back(g);
    CHECK(!granules.empty() && (KNN_DEAL_GRANULE & (KNN_DEAL_GRANULE - 1)) == 0 && KNN_DEAL_GRANULE * KNN_DEAL_SLOTS <= 40,
          "the largest granule: a power of two, 8 of them within 40 tiles: %d", KNN_DEAL_GRANULE);
    if (KNN_DEAL_GRANULE < 4) granules.push_back(4);            // (the mapping itself holds for every granule that was measured)

    // ---- the mapping
    std::vector<int> cover, slot_of;
    for (int g : granules) {
        for (int tiles = 1; tiles <= 5000; ++tiles) {
            cover.assign(tiles, 0);
            slot_of.assign(tiles, -1);
            int64_t tickets = 0;
            for (int slot = 0; slot < KNN_DEAL_SLOTS; ++slot) {
                int64_t t = 0;
                for (;; ++t) {
                    const DealRange r = knn_deal_ticket(slot, t, tiles, g);
                    if (r.tiles == 0) break;
                    CHECK(r.tiles >= 1 && r.tiles <= g && r.tile0 >= 0 && r.tile0 % g == 0 && r.tile0 + r.tiles <= tiles,
                          "g %d tiles %d slot %d ticket %lld: [%d, +%d)", g, tiles, slot, (long long)t, r.tile0, r.tiles);
                    CHECK(r.tiles == g || r.tile0 + r.tiles == tiles, "only the launch's last granule is short: g %d tiles %d", g, tiles);
                    for (int i = r.tile0; i < r.tile0 + r.tiles && i < tiles; ++i) { ++cover[i]; slot_of[i] = slot; }
                }
                // used up stays used up: the draws a workgroup makes after the end, and the two a late workgroup starts with
                for (int64_t u = t; u < t + 4; ++u) CHECK(knn_deal_ticket(slot, u, tiles, g).tiles == 0, "g %d tiles %d slot %d ticket %lld", g, tiles, slot, (long long)u);
                CHECK(knn_deal_ticket(slot, -1, tiles, g).tiles == 0, "a negative ticket");
                tickets += t;
            }
            CHECK(tickets == knn_deal_granules(tiles, g), "g %d tiles %d: %lld tickets", g, tiles, (long long)tickets);
            int bad = 0;
            for (int i = 0; i < tiles; ++i) bad += cover[i] != 1;
            CHECK(bad == 0, "g %d tiles %d: %d tiles not covered exactly once", g, tiles, bad);
            // any 40 consecutive tiles touch all eight slots
            if (tiles >= 40 && (tiles % 97 == 0 || tiles <= 200 || tiles == 5000)) {
                for (int a = 0; a + 40 <= tiles; ++a) {
                    unsigned seen = 0;
                    for (int i = a; i < a + 40; ++i) seen |= 1u << slot_of[i];
                    if (seen != 0xffu) { CHECK(seen == 0xffu, "g %d tiles %d: tiles %d..%d touch slots %#x", g, tiles, a, a + 39, seen); break; }
                }
            }
        }
        printf("mapping g%d ok\n", g);
    }

    // ---- the decision
    int dealt_lines = 0;
    for (int cus : {64, 104, 256, 304})
        for (int qt = 1; qt <= 10; ++qt)
            for (int tiles = 1; tiles <= 5000; ++tiles) {
                int gq, gs; int64_t gc;
                knn_geometry_wide((int64_t)tiles * KW_M, (int64_t)qt * KW_N, &gq, &gs, &gc);
                DealFacts f;
                f.ab_ck = 1; f.row_tiles = tiles; f.n_qtiles = gq; f.n_splits = gs; f.cus = cus;
                const DealPlan d = knn_abandon_deal(f);
                if (qt > 8) { CHECK(!d.dealt, "more than 8 query tiles: cus %d qt %d tiles %d", cus, qt, tiles); continue; }
                // the rule, restated: the largest granule of KNN_DEAL_GRANULE, /2, ... 1 at which the smallest slot's share gives every
                // resident workgroup of a (slot, query tile) two granules
                const int resident = std::min(gs / 8, std::max(1, cus / (8 * gq)));
                int want = 0;
                for (int g = KNN_DEAL_GRANULE; g >= 1 && !want; g /= 2)
                    if (((tiles + g - 1) / g) / 8 >= 2 * resident) want = g;
                CHECK(d.dealt == (want > 0) && d.granule == want, "cus %d qt %d tiles %d: dealt %d granule %d, expected %d", cus, qt, tiles, (int)d.dealt, d.granule, want);
                if (d.dealt) {
                    CHECK(d.workgroups == gq * gs && d.resident == resident, "the grid stays the plan's: %d against %d x %d", d.workgroups, gq, gs);
                    // fewer than two granules per resident workgroup at the next larger granule, or there is none
                    CHECK(d.granule == KNN_DEAL_GRANULE || knn_deal_granules(tiles, 2 * d.granule) / 8 < 2 * resident, "the largest granule that qualifies");
                    ++dealt_lines;
                }
                for (int variant = 0; variant < 5; ++variant) {          // ... and never otherwise
                    DealFacts o = f;
                    if (variant == 0) o.opt_deal = 0;
                    if (variant == 1) o.ab_ck = 0;                       // the launch does not qualify for the abandon (knn_abandon_launch)
                    if (variant == 2) o.launch = KNN_DEAL_SETS;          // no counter set left
                    if (variant == 3) o.n_qtiles = 9;
                    if (variant == 4) o.cus = 0;
                    CHECK(!knn_abandon_deal(o).dealt, "variant %d dealt: cus %d qt %d tiles %d", variant, cus, qt, tiles);
                }
                if (tiles == 512 || tiles == 3395 || tiles == 1025 || tiles == 79 || tiles == 547)
                    printf("decision c%d_q%d_t%d %d %d %d\n", cus, qt, tiles, (int)d.dealt, d.granule, d.resident);
            }
    CHECK(dealt_lines > 0, "nothing was dealt");
    {
        // what knn_abandon_launch refuses is never dealt: the launch site hands its result in as ab_ck
        AbandonFacts a;
        a.floors = true; a.terms_current = true; a.dim = 512;
        DealFacts f;
        f.row_tiles = 3395; f.n_qtiles = 4; f.n_splits = 128; f.cus = 256;
        f.ab_ck = knn_abandon_launch(a);
        CHECK(f.ab_ck == 1 && knn_abandon_deal(f).dealt, "the benchmark's second launch");
        f.row_tiles = 512;
        CHECK(knn_abandon_deal(f).dealt, "the benchmark's first launch");
        for (int variant = 0; variant < 4; ++variant) {
            AbandonFacts b = a;
            if (variant == 0) b.ksplit = 2;
            if (variant == 1) b.sample = true;
            if (variant == 2) b.rsc = 1;
            if (variant == 3) b.per_call_bias = true;
            f.ab_ck = knn_abandon_launch(b);
            CHECK(f.ab_ck == 0 && !knn_abandon_deal(f).dealt, "variant %d", variant);
        }
        // the 20 000-row stores of the existing tests: 79 tiles
        f.ab_ck = 1; f.row_tiles = 79;
        for (int qt : {1, 2}) {
            int gq, gs; int64_t gc;
            knn_geometry_wide(20000, (int64_t)qt * KW_N, &gq, &gs, &gc);
            f.n_qtiles = gq; f.n_splits = gs;
            CHECK(!knn_abandon_deal(f).dealt, "20 000 rows, %d query tiles", qt);
        }
    }

    // ---- the counter sets
    {
        std::vector<int> seen(KNN_DEAL_COUNTERS, 0);
        for (int set = 0; set < KNN_DEAL_SETS; ++set)
            for (int slot = 0; slot < KNN_DEAL_SLOTS; ++slot)
                for (int qt = 0; qt < KNN_DEAL_MAX_QTILES; ++qt) {
                    const int c = knn_deal_counter(set, slot, qt);
                    CHECK(c >= 0 && c < KNN_DEAL_COUNTERS, "counter %d", c);
                    if (c >= 0 && c < KNN_DEAL_COUNTERS) ++seen[c];
                    // what the kernel adds to its launch's base (knn_hi.inc)
                    CHECK(c == knn_deal_counter(set, 0, 0) + slot * KNN_DEAL_MAX_QTILES + qt, "the kernel's index");
                }
        int bad = 0;
        for (int c : seen) bad += c != 1;
        CHECK(bad == 0, "%d counters shared or unused", bad);
    }
    static_assert(RADAD_KNN_OPT_ABANDON_DEAL == 7, "the option");
    if (failures) { printf("knn_abandon_deal_check: %d FAILED\n", failures); return 1; }
    printf("knn_abandon_deal_check: ok\n");
    return 0;
}
