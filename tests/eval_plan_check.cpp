// eval_plan_check.cpp -- the host-only plan of radad_eval_metrics (csrc/eval_plan.h) without a GPU: n = 1, every tile and merge
// pass boundary - 1 / 0 / + 1, the cap and past it; grids, pass counts, launch counts, a workspace whose sub-arrays do not
// overlap, hold what the kernels index and start on 16-byte boundaries; and the merge kernel's index arithmetic
// (eval_merge_split plus the merge-path search and the serial merge, restated here on the host) sorting real keys through
// every pass.  Prints one "case" line per plan and "eval_plan_check: ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eval_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            ++failures;                                                      \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);    \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
        }                                                                    \
    } while (0)

static void check_plan(int64_t n, int groups) {
    const EvalPlan p = eval_plan(n, groups);
    CHECK(p.ok, "n %lld", (long long)n);
    if (!p.ok) return;
    std::printf("case n%lld_g%d %d %d %d %d %d %zu %zu %zu %zu %zu %zu\n", (long long)n, groups, p.tiles, p.merge_passes, p.sorted_buf,
                p.sorts, p.launches, p.off_buf[0], p.off_buf[1], p.off_cnt, p.off_best, p.off_idx, p.total);
    CHECK((int64_t)p.tiles * EVAL_TILE >= n && (int64_t)(p.tiles - 1) * EVAL_TILE < n, "tiles %d for n %lld", p.tiles, (long long)n);
    // one run is left behind the last pass, two or more in front of it
    CHECK(eval_pass_runs(n, p.merge_passes) == 1, "n %lld: %lld runs left", (long long)n, (long long)eval_pass_runs(n, p.merge_passes));
    if (p.merge_passes > 0) CHECK(eval_pass_runs(n, p.merge_passes - 1) >= 2, "n %lld: a pass too many", (long long)n);
    CHECK(p.sorted_buf == (p.merge_passes & 1) && p.sorts == 1 + (groups != 0), "n %lld", (long long)n);
    CHECK(p.launches == (6 + p.merge_passes) + (groups ? 8 + p.merge_passes : 0), "n %lld launches %d", (long long)n, p.launches);
    CHECK(eval_pass_run(p.merge_passes > 0 ? p.merge_passes - 1 : 0) <= (int64_t)1 << 30, "a run's length fits an int");
    // the workspace: head, then five arrays in order, none overlapping, each 16-byte (256-byte) aligned and large enough
    const size_t off[6] = {0, p.off_buf[0], p.off_buf[1], p.off_cnt, p.off_best, p.off_idx};
    const size_t need[6] = {EVAL_WS_HEAD, (size_t)n * 8, (size_t)n * 8, (size_t)(n + 1) * 8, (size_t)n * 8, (size_t)n * 4};
    for (int i = 0; i < 6; ++i) {
        CHECK(off[i] % 16 == 0 && off[i] % 256 == 0, "array %d at %zu", i, off[i]);
        const size_t end = i + 1 < 6 ? off[i + 1] : p.total;
        CHECK(off[i] + need[i] <= end, "array %d: %zu + %zu > %zu", i, off[i], need[i], end);
    }
    CHECK(p.total % 256 == 0, "total %zu", p.total);
    // the tile totals live in the key buffer the sort left free: one uint64 per tile
    CHECK((size_t)p.tiles * 8 <= need[1], "tile totals %d > %zu bytes", p.tiles, need[1]);
    // every thread of every merge pass: its pair lies inside [0, n), its diagonal inside the pair
    if (n <= 3 * EVAL_TILE * 8) {
        for (int pass = 0; pass < p.merge_passes; ++pass) {
            const int run = (int)eval_pass_run(pass);
            for (int64_t o = 0; o < (int64_t)p.tiles * EVAL_TILE; o += EVAL_ITEMS) {
                if (o >= n) continue;
                const EvalMergeSplit m = eval_merge_split((int)o, (int)n, run);
                CHECK(m.p0 >= 0 && m.p0 % (2 * run) == 0 && m.nA >= 1 && m.nA <= run && m.nB >= 0 && m.nB <= run && m.p0 + m.nA + m.nB <= n &&
                          m.d >= 0 && m.d < m.nA + m.nB,
                      "n %lld pass %d o %lld: p0 %d nA %d nB %d d %d", (long long)n, pass, (long long)o, m.p0, m.nA, m.nB, m.d);
                CHECK(m.p0 + m.nA + m.nB == n || m.nA + m.nB == 2 * run, "n %lld pass %d: a short pair that is not the last", (long long)n, pass);
            }
        }
    }
}

// k_eval_merge's body for one thread, on the host
static void merge_thread(const std::vector<uint64_t>& src, std::vector<uint64_t>& dst, int o, int n, int run) {
    const EvalMergeSplit m = eval_merge_split(o, n, run);
    const uint64_t* A = src.data() + m.p0;
    const uint64_t* B = A + m.nA;
    int lo = std::max(0, m.d - m.nB), hi = std::min(m.d, m.nA);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        CHECK(mid >= 0 && mid < m.nA && m.d - 1 - mid >= 0 && m.d - 1 - mid < m.nB, "search out of range");
        if (A[mid] <= B[m.d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int a = lo, b = m.d - lo;
    const int cnt = std::min(EVAL_ITEMS, m.nA + m.nB - m.d);
    for (int i = 0; i < cnt; ++i) {
        CHECK(a < m.nA || b < m.nB, "both runs exhausted");
        if (b >= m.nB || (a < m.nA && A[a] <= B[b])) dst[o + i] = A[a++]; else dst[o + i] = B[b++];
    }
}

static void check_sort(int n, unsigned seed, int distinct) {
    const EvalPlan p = eval_plan(n, 0);
    std::vector<uint64_t> keys(n), buf[2];
    uint64_t s = seed * 2654435761u + 1;
    for (int i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        keys[i] = distinct ? (s >> 33) % (uint64_t)distinct : s >> 20;
    }
    buf[0] = keys;
    buf[1].assign(n, 0);
    for (int t = 0; t < p.tiles; ++t)       // the tile sort
        std::sort(buf[0].begin() + (size_t)t * EVAL_TILE, buf[0].begin() + std::min<size_t>(n, (size_t)(t + 1) * EVAL_TILE));
    for (int pass = 0; pass < p.merge_passes; ++pass)
        for (int o = 0; o < n; o += EVAL_ITEMS) merge_thread(buf[pass & 1], buf[(pass + 1) & 1], o, n, (int)eval_pass_run(pass));
    std::sort(keys.begin(), keys.end());
    CHECK(buf[p.sorted_buf] == keys, "n %d seed %u distinct %d: the passes do not sort", n, seed, distinct);
}

int main() {
    CHECK(!eval_plan(0, 0).ok && !eval_plan(-5, 1).ok && !eval_plan(EVAL_MAX_N + 1, 0).ok, "out-of-range n must be refused");
    std::vector<int64_t> ns = {1, 2, 3, EVAL_ITEMS - 1, EVAL_ITEMS, EVAL_ITEMS + 1, 63, 64, 65, EVAL_THREADS - 1, EVAL_THREADS, EVAL_THREADS + 1, 70001};
    for (int pass = 0; (EVAL_TILE << pass) <= EVAL_MAX_N; ++pass)
        for (int d = -1; d <= 1; ++d) {
            const int64_t n = ((int64_t)EVAL_TILE << pass) + d;
            if (n <= EVAL_MAX_N) ns.push_back(n);
        }
    ns.push_back(3 * EVAL_TILE - 1); ns.push_back(3 * EVAL_TILE); ns.push_back(3 * EVAL_TILE + 1);
    ns.push_back(EVAL_MAX_N - 1);
    for (int64_t n : ns)
        for (int g = 0; g < 2; ++g) check_plan(n, g);
    // pass counts by hand: 1 tile -> 0, 2 -> 1, 3..4 -> 2, 35 tiles (70 001) -> 6, the cap -> 13
    CHECK(eval_plan(EVAL_TILE, 0).merge_passes == 0 && eval_plan(EVAL_TILE + 1, 0).merge_passes == 1 &&
              eval_plan(2 * EVAL_TILE + 1, 0).merge_passes == 2 && eval_plan(70001, 1).merge_passes == 6 &&
              eval_plan(EVAL_MAX_N, 1).merge_passes == 13 && eval_plan(EVAL_MAX_N, 1).tiles == 8192,
          "hand-computed pass counts");
    CHECK(eval_plan(70001, 1).launches == 12 + 14 && eval_plan(1, 0).launches == 6, "hand-computed launch counts");
    // the cap's workspace by hand: head, 4 arrays of 2^24 x 8 bytes (one with an extra element, rounded up to 256), 2^24 x 4
    CHECK(eval_plan(EVAL_MAX_N, 1).total == 256 + 4 * ((size_t)1 << 27) + 256 + ((size_t)1 << 26), "the cap's workspace");
    for (int n : {1, 2, 7, 8, 9, EVAL_TILE - 1, EVAL_TILE, EVAL_TILE + 1, 2 * EVAL_TILE, 2 * EVAL_TILE + 1, 3 * EVAL_TILE + 5, 4 * EVAL_TILE - 1,
                  5 * EVAL_TILE + 1, 70001})
        for (int distinct : {0, 1, 5}) check_sort(n, (unsigned)n, distinct);
    std::printf(failures ? "eval_plan_check: %d FAILED\n" : "eval_plan_check: ok\n", failures);
    return failures ? 1 : 0;
}
