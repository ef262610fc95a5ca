// Drives the restart scheduler of the coordinate-descent batch (cnmf_amd/csrc/batch_sched.h) without a device
// (tests/test_host_batch_sched.py compiles this with the address and undefined-behaviour sanitizers and runs it).
//
//   batch_sched_main check                                   hand-written expectations + invariants on seeded synthetic jobs
//   batch_sched_main replay KC MODE LAG PART LEN k1,k2,...   one job, every restart LEN iterations long: prints the schedule statistics
//
// The fake device: a restart installed when it == t0 shows active == 0 in snapshot si iff si - t0 + 1 >= len[restart]; the
// host inspects snapshot it - 1 - lag; a retired slot keeps its descriptor (restart id, active = 0) until it is reused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../cnmf_amd/csrc/batch_sched.h"

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)
#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: REQUIRE failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Scheme { bool use3, usec, use2h, part; };
static Scheme scheme_of_mode(int mode, bool part) { return Scheme{mode != 0, mode == 3 || mode == 4, mode == 4 || mode == 5, part}; }

struct Result {
    int64_t outer, column, restart, restart_col, tail_its, tail_live, n_defrag;
    int n_narrow, n_rebalance;
};

// the loop of run_batch (refill -> iterate -> inspect -> compact) against the fake device, with the invariants checked at every step
static Result drive(const std::vector<int32_t>& ks, const std::vector<int>& len, int KC, int lag, Scheme f, const double* hint = nullptr)
{
    const int n = (int)ks.size();
    BatchSched sc(n, ks.data(), KC, hint, false);
    const int KC0 = sc.KC0;
    std::vector<int> hm((size_t)3 * KC0), installed(n, 0), retired(n, 0);
    std::vector<int64_t> t0(n, -1);
    struct Snap { int active, restart; };
    std::vector<int> dev_restart(KC0, -1);                       // the device's slot table: the restart a slot was last given
    std::vector<Snap> ring((size_t)SCHED_RING * KC0, Snap{0, -1});
    Result res{};
    int64_t kc_sum = 0;
    int last_KC = KC;

    auto invariants = [&]() {
        std::vector<std::pair<int, int>> live;
        for (int s = 0; s < KC0; ++s) {
            if (s >= sc.nslots) REQUIRE(sc.hs[s].state == 0);
            if (sc.hs[s].state) live.push_back({sc.hs[s].off, sc.hs[s].k});
        }
        std::sort(live.begin(), live.end());
        int end = 0, cols = 0;
        for (auto& iv : live) { REQUIRE(iv.first >= end); end = iv.first + iv.second; cols += iv.second; }
        REQUIRE(end <= sc.KC);
        REQUIRE(cols == sc.live_columns());
        REQUIRE((int)live.size() == sc.n_active);
        REQUIRE(sc.nslots <= KC0);
        REQUIRE(sc.KC <= last_KC);
        last_KC = sc.KC;
        REQUIRE(sc.column_iters == kc_sum);
        if (sc.n_pending > 0) {                                   // the allocator's free list and the live slots tile [0, KC)
            int fr = 0;
            for (auto& iv : sc.cols.free_) fr += iv.second;
            REQUIRE(fr + cols == sc.KC);
        }
    };

    while (true) {
        sc.begin_refill();
        while (true) {
            Placement p;
            while (sc.next_placement(&p)) {
                REQUIRE(p.slot >= 0 && p.slot < KC0 && p.restart >= 0 && p.restart < n);
                REQUIRE(p.k == ks[p.restart] && p.off >= 0 && p.off + p.k <= sc.KC);
                ++installed[p.restart]; t0[p.restart] = sc.it;
                dev_restart[p.slot] = p.restart;
                invariants();
            }
            if (!sc.defrag_due()) break;
            const RepackPlan pl = sc.plan_repack(sc.KC, false, hm.data());
            sc.defragmented();
            REQUIRE(pl.pos == sc.live_columns());
            // after a defragmentation the free columns form one interval at the right
            REQUIRE(sc.cols.free_.size() <= 1);
            if (!sc.cols.free_.empty())
                REQUIRE(sc.cols.free_[0].first == pl.pos && sc.cols.free_[0].first + sc.cols.free_[0].second == sc.KC);
            invariants();
        }
        if (sc.finished()) break;
        // iterate: the device publishes the state of every slot into the ring entry of this iteration
        for (int s = 0; s < sc.nslots; ++s) {
            const int r = dev_restart[s];
            ring[(size_t)(sc.it % SCHED_RING) * KC0 + s] = Snap{r >= 0 && sc.it - t0[r] + 1 >= len[r] ? 0 : 1, r};
        }
        kc_sum += sc.KC;
        sc.end_iteration();
        REQUIRE(sc.it < 10000000);                                // the job terminates
        // inspect
        const int64_t si = sc.it - 1 - lag;
        if (si >= 0) {
            const Snap* sp = &ring[(size_t)(si % SCHED_RING) * KC0];
            for (int s = 0; s < sc.snap_nslots[si % SCHED_RING]; ++s)
                if (sc.retirable(s, si, sp[s].active, sp[s].restart)) {
                    const int r = sc.hs[s].restart;
                    REQUIRE(si >= t0[r]);                         // never retired on a snapshot older than its installation
                    REQUIRE(si - t0[r] + 1 >= len[r]);
                    ++retired[r];
                    sc.retire(s, len[r]);
                    invariants();
                }
            sc.resort_pending();
        }
        // compact
        if (sc.in_tail()) {
            const TailPlan t = sc.tail_plan(f.use3, f.usec, f.use2h, f.part);
            if (t.rebalance) { sc.plan_repack(sc.KC, true, hm.data()); sc.rebalanced(); ++res.n_rebalance; invariants(); }
            if (t.width < sc.KC) {
                sc.plan_repack(t.width, t.stay3 && f.use2h && f.part, hm.data());
                sc.narrowed(t.width);
                if (!t.stay3) f.use3 = f.usec = f.use2h = false;
                ++res.n_narrow;
                invariants();
            }
        }
    }
    for (int r = 0; r < n; ++r) REQUIRE(installed[r] == 1 && retired[r] == 1);      // exactly once each
    invariants();
    res.outer = sc.it; res.column = sc.column_iters; res.restart = sc.restart_iters; res.restart_col = sc.restart_col_iters;
    res.tail_its = sc.tail_its; res.tail_live = sc.tail_live; res.n_defrag = sc.n_defrag;
    return res;
}

// ---- hand-written expectations: literals derived on paper from the rules, not from a run
static void check_initial_order()
{
    const int32_t ks[6] = {5, 5, 9, 13, 9, 5};
    BatchSched a(6, ks, 64, nullptr, false);
    CHECK((a.order == std::vector<int>{3, 2, 0, 4, 1, 5}));      // rounds over the distinct ranks, largest first
    std::vector<double> hint(SCHED_KMAX + 1, 0.0);
    hint[5] = 100; hint[9] = 30;                                  // rank 13 was never seen: it counts as longest
    BatchSched h(6, ks, 64, hint.data(), false);
    CHECK((h.order == std::vector<int>{3, 0, 1, 5, 2, 4}));
}

static void check_col_alloc()
{
    using V = std::vector<std::pair<int, int>>;
    ColAlloc c(100);
    CHECK(c.alloc(30) == 0);
    CHECK(c.alloc(50) == 30);
    CHECK(c.alloc(30) == -1);                                     // 20 columns left
    CHECK(c.alloc(20) == 80);
    CHECK(c.free_.empty());
    c.release(30, 50);
    CHECK(c.alloc(10) == 30);                                     // first fit: the hole, at its left end
    CHECK((c.free_ == V{{40, 40}}));
    c.release(0, 30);
    CHECK((c.free_ == V{{0, 30}, {40, 40}}));
    CHECK(c.alloc(35) == 40);                                     // the first interval is too small
    CHECK((c.free_ == V{{0, 30}, {75, 5}}));
    c.release(30, 10);                                            // joins its left neighbour only
    CHECK((c.free_ == V{{0, 40}, {75, 5}}));
    c.release(40, 35);                                            // joins both neighbours
    CHECK((c.free_ == V{{0, 80}}));
    c.release(80, 20);
    CHECK((c.free_ == V{{0, 100}}));
}

static void set_live(BatchSched& sc, const std::vector<int>& offs, const std::vector<int>& ranks)
{
    for (size_t s = 0; s < offs.size(); ++s) {
        sc.hs[s].state = 1; sc.hs[s].restart = (int)s; sc.hs[s].off = offs[s]; sc.hs[s].k = ranks[s];
    }
    sc.nslots = sc.n_active = (int)offs.size();
}

static void expect_map(const int* hm, int width, const std::vector<std::pair<int, std::pair<int, int>>>& runs)
{
    std::vector<int> want(width, -1);                             // (first new column, (first old column, length)), else -1
    for (auto& r : runs) for (int c = 0; c < r.second.second; ++c) want[r.first + c] = r.second.first + c;
    for (int c = 0; c < width; ++c) CHECK(hm[c] == want[c]);
}

static void check_repack_plans()
{
    {   // left: three live slots at offsets {40, 0, 100} with ranks {8, 16, 4}, width 128
        BatchSched sc(0, nullptr, 128, nullptr, false);
        set_live(sc, {40, 0, 100}, {8, 16, 4});
        std::vector<int> hm(3 * 128, -7);
        const RepackPlan pl = sc.plan_repack(128, false, hm.data());
        CHECK(pl.nmove == 2 && pl.pos == 28);
        expect_map(hm.data(), 128, {{0, {0, 16}}, {16, {40, 8}}, {24, {100, 4}}});
        CHECK(hm[128] == 0 && hm[256] == 16 && hm[129] == 2 && hm[257] == 24);      // slot 1 stays where it is
        CHECK(sc.hs[0].off == 16 && sc.hs[1].off == 0 && sc.hs[2].off == 24);
    }
    {   // balanced: width 512 = two groups; ranks {60, 50, 40, 30, 20, 10} -> fills 60+30+20 = 110 and 50+40+10 = 100
        BatchSched sc(0, nullptr, 1024, nullptr, false);
        set_live(sc, {0, 60, 110, 150, 180, 200}, {60, 50, 40, 30, 20, 10});
        std::vector<int> hm(3 * 1024, -7);
        const RepackPlan pl = sc.plan_repack(512, true, hm.data());
        CHECK(pl.nmove == 5 && pl.pos == 0);
        expect_map(hm.data(), 512, {{0, {0, 60}}, {60, {150, 30}}, {90, {180, 20}}, {256, {60, 50}}, {306, {110, 40}}, {346, {200, 10}}});
        const int ids[5] = {1, 2, 3, 4, 5}, offs[5] = {256, 306, 60, 90, 346};
        for (int i = 0; i < 5; ++i) CHECK(hm[1024 + i] == ids[i] && hm[2048 + i] == offs[i]);
        const int now[6] = {0, 256, 306, 60, 90, 346};
        for (int s = 0; s < 6; ++s) CHECK(sc.hs[s].off == now[s]);
    }
    {   // balanced, but the third restart fits no group any more (200 + 100 > 256 twice): the left plan
        BatchSched sc(0, nullptr, 1024, nullptr, false);
        set_live(sc, {0, 300, 600}, {200, 200, 100});
        std::vector<int> hm(3 * 1024, -7);
        const RepackPlan pl = sc.plan_repack(512, true, hm.data());
        CHECK(pl.nmove == 2 && pl.pos == 500);
        expect_map(hm.data(), 512, {{0, {0, 200}}, {200, {300, 200}}, {400, {600, 100}}});
        CHECK(hm[1024] == 1 && hm[2048] == 200 && hm[1025] == 2 && hm[2049] == 400);
    }
}

static void check_tail_widths()
{
    const int live[9] = {1, 32, 33, 64, 65, 200, 256, 257, 600};
    const int f32w[9] = {32, 32, 64, 64, 128, 256, 256, 512, 768};           // powers of two up to 256, then steps of 256
    const int g3w[9] = {32, 32, 64, 64, 256, 256, 256, 512, 768};            // bf16 planes of a general matrix: stays above 64
    const int cw[9] = {32, 32, 256, 256, 256, 256, 256, 512, 768};           // count path: leaves the matrix pipe for 32 columns only
    for (int i = 0; i < 9; ++i) {
        BatchSched sc(0, nullptr, 1024, nullptr, false);
        set_live(sc, {0}, {live[i]});
        sc.n_pending = 0;
        CHECK(sc.in_tail());
        TailPlan t = sc.tail_plan(false, false, false, false);
        CHECK(t.width == f32w[i] && !t.stay3 && !t.rebalance);
        t = sc.tail_plan(true, false, false, false);
        CHECK(t.width == g3w[i] && t.stay3 == (live[i] > 64) && !t.rebalance);
        t = sc.tail_plan(true, true, true, false);
        CHECK(t.width == cw[i] && t.stay3 == (live[i] > 32) && !t.rebalance);
    }
}

// ---- seeded synthetic jobs
static uint64_t g_lcg = 0;
static uint32_t lcg() { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_lcg >> 33); }
static std::vector<int> lengths(size_t n) { std::vector<int> l(n); for (auto& v : l) v = 35 + (int)(lcg() % 966); return l; }

static void check_synthetic_jobs()
{
    g_lcg = 2024;
    std::vector<int32_t> ks(150);
    for (auto& k : ks) k = 5 + (int32_t)(lcg() % 9);
    const std::vector<int> len = lengths(ks.size());
    for (int part = 0; part < 2; ++part)
        for (int lag = 1; lag <= 4; lag += 3) {
            const Result r = drive(ks, len, 1024, lag, scheme_of_mode(4, part != 0));
            CHECK(r.n_defrag >= 1);
            CHECK(r.n_narrow >= 1);
        }
    const Result g = drive(ks, len, 1024, 2, scheme_of_mode(2, false));
    CHECK(g.n_narrow >= 1);
    std::vector<double> hint(SCHED_KMAX + 1, 0.0);
    for (int k = 5; k <= 12; ++k) hint[k] = 1000.0 / k;
    drive(ks, len, 1024, 2, scheme_of_mode(4, false), hint.data());
    drive(std::vector<int32_t>(40, 9), lengths(40), 128, 2, scheme_of_mode(0, false));
    drive({3, 16, 33, 65, 128}, lengths(5), 256, 2, scheme_of_mode(0, false));
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "check")) {
        check_initial_order();
        check_col_alloc();
        check_repack_plans();
        check_tail_widths();
        check_synthetic_jobs();
        if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
        printf("ok\n");
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "replay")) {
        const int KC = atoi(argv[2]), mode = atoi(argv[3]), lag = atoi(argv[4]), part = atoi(argv[5]), L = atoi(argv[6]);
        std::vector<int32_t> ks;
        for (char* tok = strtok(argv[7], ","); tok; tok = strtok(nullptr, ",")) ks.push_back(atoi(tok));
        const Result r = drive(ks, std::vector<int>(ks.size(), L), KC, lag, scheme_of_mode(mode, part != 0));
        printf("{\"outer_iterations\": %lld, \"column_iterations\": %lld, \"restart_iterations\": %lld, \"tail_iterations\": %lld, "
               "\"tail_live_columns\": %lld}\n", (long long)r.outer, (long long)r.column, (long long)r.restart,
               (long long)r.tail_its, (long long)r.tail_live);
        return 0;
    }
    fprintf(stderr, "usage: %s check | replay KC MODE LAG PART LEN k1,k2,...\n", argv[0]);
    return 2;
}
