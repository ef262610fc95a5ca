// The restart scheduler of the coordinate-descent batch (run_batch, batch_host.hip.h), without a device: the queue order,
// the column allocator, refill placement, retirement bookkeeping, the re-packing plans and the tail width rule.  Plain
// C++ over the standard library only, so a CPU program can drive it (tests/host/batch_sched_main.cpp); batch_host.hip.h
// does the copies and launches that go with every decision made here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

constexpr int SCHED_KMAX = 128;     // = KMAX (kernels_sweep.hip.h) and RING (runtime.hip.h): batch_host.hip.h asserts both
constexpr int SCHED_RING = 8;

// simple first-fit interval allocator over the packed component columns
struct ColAlloc {
    std::vector<std::pair<int, int>> free_;   // (begin, length), sorted by begin
    explicit ColAlloc(int n) { free_.push_back({0, n}); }
    int alloc(int k) {
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].second >= k) {
                int b = free_[i].first;
                free_[i].first += k; free_[i].second -= k;
                if (free_[i].second == 0) free_.erase(free_.begin() + i);
                return b;
            }
        return -1;
    }
    void release(int b, int k) {
        auto it = std::lower_bound(free_.begin(), free_.end(), std::make_pair(b, 0));
        it = free_.insert(it, {b, k});
        if (it + 1 != free_.end() && it->first + it->second == (it + 1)->first) {
            it->second += (it + 1)->second; free_.erase(it + 1);
        }
        if (it != free_.begin() && (it - 1)->first + (it - 1)->second == it->first) {
            (it - 1)->second += it->second; free_.erase(it);
        }
    }
};

struct HostSlot { int state = 0; int restart = -1; int off = 0; int k = 0; int64_t installed_at = 0; };

struct Placement { int restart, slot, off, k; };          // refill: restart `restart` goes into slot `slot` at columns off .. off + k
struct RepackPlan { int nmove, pos; };                    // re-packing: slots that moved, first column behind the live ones (0: balanced)
struct TailPlan { int width; bool stay3, rebalance; };    // tail: the width to run at, still on the matrix pipe, same-width re-pack due

struct BatchSched {
    const int n;
    const int32_t* const kk;             // rank of every restart
    const int KC0;                       // packed columns the call started with (slot indices stay below it)
    int KC;                              // ... and runs at now (the tail narrows it)
    const double* const hint;            // caller's mean iterations per rank [SCHED_KMAX + 1], or NULL
    const bool dbg;

    // Queue order.  Restarts are independent, so the order they run in is free; what it decides is the TAIL of the
    // call: once the queue is dry the columns of finished restarts stay empty, and the call ends when the LONGEST
    // restart still in flight converges (iterations per restart span 35 ... 1000 and depend mostly on the rank: ranks
    // far from the data's own need the most).  Hence longest-expected-first:
    //   * start: the ranks interleaved (round-robin over the distinct ranks, largest first inside a round), so every
    //     rank is sampled within the first fill of the packed columns;
    //   * as restarts retire, the mean iteration count per rank is learned and the pending queue is re-sorted by it,
    //     descending (LPT) -- the short restarts are kept for the end, where they fill the columns the long ones free.
    // The caller's iteration hints (cnmf_set_iteration_hints: mean iterations per rank, e.g. what an earlier call on this
    // matrix learned) order the queue from the start.  Explicit only: the order decides the packed columns a restart
    // occupies and with them the last bits of its float32 result (tests/test_gpu_determinism.py).
    std::vector<int> order;
    size_t next = 0;                     // first queue position that may still be pending
    int n_pending;
    std::vector<int64_t> k_iters, k_done;        // learned per rank: sum of n_iter, restarts retired
    int last_resort_done = 0;

    ColAlloc cols;
    std::vector<HostSlot> hs;
    int nslots = 0;                      // highest used slot index + 1
    int n_active = 0, n_done = 0;
    int64_t it = 0;                      // batch iterations enqueued so far
    int snap_nslots[SCHED_RING] = {0};   // nslots of the iteration whose snapshot sits in a ring entry
    int64_t last_tail_repack = -1000, last_defrag = -8, n_defrag = 0;
    // what cnmf_batch_stats reports of the schedule
    int64_t restart_iters = 0, column_iters = 0, restart_col_iters = 0, tail_its = 0, tail_live = 0;
    int64_t dbg_it[65] = {0}, dbg_live[65] = {0};        // by KC / 32 (up to 2048 packed columns)
    // the refill pass in progress
    int attempt = 0, failed_k = 1 << 30; // failed_k: smallest rank that did not fit in this pass
    size_t pi = 0;

    double prior_of(int k) const { return hint ? hint[k] : 0.0; }

    BatchSched(int n_, const int32_t* kk_, int KC_, const double* hint_, bool dbg_)
        : n(n_), kk(kk_), KC0(KC_), KC(KC_), hint(hint_), dbg(dbg_), order(n_), n_pending(n_),
          k_iters(SCHED_KMAX + 1, 0), k_done(SCHED_KMAX + 1, 0), cols(KC_), hs(KC_)
    {
        std::vector<std::vector<int>> by_k(SCHED_KMAX + 1);
        for (int r = 0; r < n; ++r) by_k[kk[r]].push_back(r);
        size_t pos = 0;
        for (size_t j = 0; pos < (size_t)n; ++j)
            for (int k = SCHED_KMAX; k >= 1; --k)
                if (j < by_k[k].size()) order[pos++] = by_k[k][j];
        if (hint)                  // ranks never seen count as longest (sampled first), the others by their learned mean
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
                const double ea = prior_of(kk[a]) > 0 ? prior_of(kk[a]) : 1e30, eb = prior_of(kk[b]) > 0 ? prior_of(kk[b]) : 1e30;
                return ea > eb;
            });
    }

    int live_columns() const { int c = 0; for (int s = 0; s < nslots; ++s) if (hs[s].state) c += hs[s].k; return c; }
    // bit t: the 32 packed columns 32 t .. 32 t + 31 hold a live restart; *fullest: most live tiles in one 256-column group
    unsigned long long live_tiles(int* fullest) const {
        unsigned long long m = 0ull;
        for (int s = 0; s < nslots; ++s)
            if (hs[s].state)
                for (int t = hs[s].off / 32; t <= (hs[s].off + hs[s].k - 1) / 32 && t < 64; ++t) m |= 1ull << t;
        *fullest = 0;
        for (int g = 0; g < KC / 256; ++g) *fullest = std::max(*fullest, __builtin_popcountll((m >> (8 * g)) & 0xffull));
        return m;
    }
    bool finished() const { return n_active == 0 && n_pending == 0; }

    // ---- refill: begin_refill(), then next_placement() until it says no; if defrag_due(), the caller re-packs the live
    // slots to the left (plan_repack(KC, false, ...) and the device moves), calls defragmented() and places again.
    // Pending restarts are sorted by descending rank; a hole too small for the head of the queue is filled with the
    // largest pending rank that fits (restarts are independent, so the order they run in is free) -> the packed columns
    // stay full in the main phase (letting a hole wait for the head of the queue instead was measured and not adopted:
    // DESIGN.md section 8).
    void begin_refill() { attempt = 0; failed_k = 1 << 30; pi = next; }
    bool next_placement(Placement* p) {
        for (; pi < order.size() && n_pending > 0; ++pi) {
            const int r = order[pi];
            if (r < 0) { if (pi == next) ++next; continue; }      // already taken
            const int k = kk[r];
            if (k >= failed_k) continue;
            const int off = cols.alloc(k);
            if (off < 0) { failed_k = k; continue; }
            order[pi] = -1; --n_pending;
            if (pi == next) ++next;
            int s = 0;
            while (s < KC0 && hs[s].state != 0) ++s;
            hs[s].state = 1; hs[s].restart = r; hs[s].off = off; hs[s].k = k; hs[s].installed_at = it;
            nslots = std::max(nslots, s + 1);
            ++n_active;
            ++pi;
            *p = Placement{r, s, off, k};
            return true;
        }
        return false;
    }
    // Defragmentation: a pending restart did not fit although enough columns are free in total (holes left by retired
    // slots of other ranks).  Repacking costs about one iteration and buys a restart that runs for hundreds -- at most
    // once every 8 iterations.
    bool defrag_due() const {
        return attempt == 0 && n_pending > 0 && failed_k < (1 << 30) && it - last_defrag >= 8 && KC - live_columns() >= failed_k;
    }
    void rebuild_cols() {                 // the live slots lie packed from column 0: everything behind them is free
        cols = ColAlloc(KC);
        for (int s = 0; s < nslots; ++s) if (hs[s].state) cols.alloc(hs[s].k);
    }
    void defragmented() {
        rebuild_cols();
        last_defrag = it; ++n_defrag;
        attempt = 1; failed_k = 1 << 30; pi = next;        // place again into the contiguous free tail
    }

    // ---- one iteration was enqueued for every slot in flight
    void end_iteration() {
        snap_nslots[it % SCHED_RING] = nslots;
        column_iters += KC;
        if (n_pending == 0) { ++tail_its; tail_live += live_columns(); }
        if (dbg) { dbg_it[KC / 32] += 1; dbg_live[KC / 32] += live_columns(); }
        ++it;
    }

    // ---- retirement: slot s, as snapshot si shows it (its `active` flag and restart id), has finished
    bool retirable(int s, int64_t si, int snap_active, int snap_restart) const {
        return hs[s].state == 1 && hs[s].installed_at <= si && snap_active == 0 && snap_restart == hs[s].restart;
    }
    void retire(int s, int iter) {
        HostSlot& h = hs[s];
        restart_iters += iter;
        restart_col_iters += (int64_t)iter * h.k;
        k_iters[h.k] += iter; k_done[h.k] += 1;
        if (n_pending > 0) cols.release(h.off, h.k);       // (after the queue ran dry nothing is allocated any more)
        h.state = 0; h.restart = -1;
        --n_active; ++n_done;
    }
    // longest-expected-first: re-sort what is still pending by the mean iteration count learned per rank (ranks
    // without a finished restart yet count as longest: they are sampled first), every 8 retirements
    void resort_pending() {
        if (!(n_pending > 1 && n_done - last_resort_done >= 8)) return;
        last_resort_done = n_done;
        std::vector<int> rest;
        rest.reserve(n_pending);
        for (size_t q = next; q < order.size(); ++q) if (order[q] >= 0) rest.push_back(order[q]);
        // expected iterations of a rank: mean over the restarts that have STARTED -- the finished ones with their count,
        // the ones in flight with their age (a lower bound).  Counting only the finished ones is biased low while it
        // matters most: of a rank whose restarts take 300 or 1000 iterations the 300s retire first.  An earlier call's
        // mean (prior) enters as four pseudo-observations.
        std::vector<double> fly_age(SCHED_KMAX + 1, 0.0); std::vector<int> fly_n(SCHED_KMAX + 1, 0);
        for (int s2 = 0; s2 < nslots; ++s2)
            if (hs[s2].state) { fly_age[hs[s2].k] += (double)(it - hs[s2].installed_at); fly_n[hs[s2].k] += 1; }
        auto expect = [&](int r) {
            const int k = kk[r];
            double num = (double)k_iters[k] + fly_age[k], den = (double)k_done[k] + fly_n[k];
            if (prior_of(k) > 0) { num += 4.0 * prior_of(k); den += 4.0; }
            return den > 0 ? num / den : 1e30;
        };
        if (dbg && n_done % 64 < 8) {
            fprintf(stderr, "[cnmf] it %lld done %d pending %d expected per rank:", (long long)it, n_done, n_pending);
            for (int k = 1; k <= SCHED_KMAX; ++k)
                if (k_done[k] + fly_n[k] > 0)
                    fprintf(stderr, " k%d=%.0f(%lld done, %d fly)", k, ((double)k_iters[k] + fly_age[k]) / ((double)k_done[k] + fly_n[k]),
                            (long long)k_done[k], fly_n[k]);
            fprintf(stderr, "\n");
        }
        std::stable_sort(rest.begin(), rest.end(), [&](int a, int b) {
            const double ea = expect(a), eb = expect(b);
            return ea != eb ? ea > eb : kk[a] > kk[b];
        });
        order.resize(next);
        order.insert(order.end(), rest.begin(), rest.end());
    }

    // ---- re-packing plan: the live slots move to the left end of the packed columns (ascending offset order) and
    // everything from the first free column up to `width` is zeroed.  hm = [column map | moved slot ids | their new
    // offsets], KC0 ints each: row c of the re-packed factors is old row hm[c], or zero for -1.  The slots' `off` is updated.
    // balanced (the tail of a wide batch only: nothing will be installed any more): the live restarts are dealt to the
    // 256-column component groups so that every group holds about the same number of live 32-column tiles -- the GEMM
    // workgroups of ALL groups then skip the same share of their MFMAs (a pass lasts as long as its slowest workgroup);
    // a restart that fits no group any more falls back to the left plan.
    RepackPlan plan_repack(int width, bool balanced, int* hm) {
        std::vector<int> idx;
        for (int s = 0; s < nslots; ++s) if (hs[s].state) idx.push_back(s);
        std::sort(idx.begin(), idx.end(), [&](int a, int b) { return hs[a].off < hs[b].off; });
        int pos = 0, nmove = 0;
        const int ngroups = width / 256;
        if (balanced && ngroups > 1) {
            for (int c = 0; c < width; ++c) hm[c] = -1;
            std::vector<int> fill(ngroups, 0), byk(idx);
            std::stable_sort(byk.begin(), byk.end(), [&](int a, int b) { return hs[a].k > hs[b].k; });
            bool ok = true;
            std::vector<int> newoff(nslots, -1);
            for (int s : byk) {
                int g = -1;
                for (int q = 0; q < ngroups; ++q) if (fill[q] + hs[s].k <= 256 && (g < 0 || fill[q] < fill[g])) g = q;
                if (g < 0) { ok = false; break; }
                newoff[s] = g * 256 + fill[g]; fill[g] += hs[s].k;
            }
            if (ok) {
                for (int s : idx) {
                    HostSlot& h = hs[s];
                    for (int c = 0; c < h.k; ++c) hm[newoff[s] + c] = h.off + c;
                    if (h.off != newoff[s]) { hm[KC0 + nmove] = s; hm[2 * KC0 + nmove] = newoff[s]; ++nmove; h.off = newoff[s]; }
                }
                return RepackPlan{nmove, 0};                              // (there are zero rows inside [0, width) now)
            }
        }
        for (int s : idx) {
            HostSlot& h = hs[s];
            for (int c = 0; c < h.k; ++c) hm[pos + c] = h.off + c;
            if (h.off != pos) { hm[KC0 + nmove] = s; hm[2 * KC0 + nmove] = pos; ++nmove; h.off = pos; }
            pos += h.k;
        }
        for (int c = pos; c < width; ++c) hm[c] = -1;                    // zero rows behind the live ones
        return RepackPlan{nmove, pos};
    }

    // ---- tail: nothing left to refill with -> the width the live columns need.
    // On the count path a 256-column iteration (~250 us of GEMM at 50k x 2000) costs no more than a 64-column one on
    // the f32 pipe and far less than a 128-column one: leave it only for 32 columns.  General (non-count) split-operand
    // path, 6 MFMAs per product: a 256-column iteration still beats 128 columns on the f32 pipe (417 / 2 vs 157 TF of
    // roof per live column), not 64.  A WIDE batch (512+) narrows in steps of 256 columns and stays on the same kernels.
    static TailPlan tail_width(int live_cols, bool use3, bool usec) {
        int KCn = 32;
        while (KCn < live_cols && KCn < 256) KCn *= 2;
        if (live_cols > 256) KCn = (live_cols + 255) / 256 * 256;
        bool stay3 = false;
        if (use3 && KCn > (usec ? 32 : 64)) { KCn = (std::max(live_cols, 1) + 255) / 256 * 256; stay3 = true; }
        return TailPlan{KCn, stay3, false};
    }
    bool in_tail() const { return n_pending == 0 && n_active > 0 && KC > 32; }
    // (call only in_tail())  width < KC: narrow to it.  rebalance: same width, but the live restarts lie scattered:
    // pack them so that whole 32-column tiles fall dead (the GEMM passes skip those) -- when that frees at least 2 tiles
    // and an eighth of them, at most every 16 iterations.
    TailPlan tail_plan(bool use3, bool usec, bool use2h, bool part) const {
        const int live_cols = live_columns();
        TailPlan t = tail_width(live_cols, use3, usec);
        if (t.width == KC && use2h && part && it - last_tail_repack >= 16) {
            const int ng = KC / 256;
            int fullest = 0;
            live_tiles(&fullest);
            const int ideal = ((live_cols + 31) / 32 + ng - 1) / ng;       // tiles per group if dealt evenly
            t.rebalance = ideal <= 6 && fullest >= ideal + 2;
        }
        return t;
    }
    void rebalanced() { last_tail_repack = it; }
    void narrowed(int width) { last_tail_repack = it; KC = width; rebuild_cols(); }

    void print_debug() const {
        fprintf(stderr, "[cnmf] %lld defragmentations\n", (long long)n_defrag);
        for (int i = 1; i <= 64; ++i)
            if (dbg_it[i]) fprintf(stderr, "[cnmf] KC=%d: %lld iterations, mean host-live columns %.1f\n", i * 32,
                                   (long long)dbg_it[i], (double)dbg_live[i] / dbg_it[i]);
    }
};
