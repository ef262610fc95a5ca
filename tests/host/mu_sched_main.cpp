// The round scheduler of the multiplicative-update driver (cnmf_amd/csrc/mu_sched.h) against a fake device: every job
// has a scripted divergence indexed by iteration (held at its last value beyond the script).  The loop below is the
// protocol of the header's comment, as mu_drive (mu_host.hip.h) runs it, with the invariants checked after every step.
// Prints "ok"; any failed check prints its line and exits 1.  Built with -fsanitize=address,undefined (tests/test_host_mu_sched.py).
#include "../../cnmf_amd/csrc/mu_sched.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

typedef std::vector<double> Script;
static double at(const Script& s, int it) { return s[std::min<size_t>(it, s.size() - 1)]; }

struct Result { int n_iter = -1; double err = 0; std::vector<int> evals; int placed = 0, retired = 0; };
struct Run { std::vector<Result> res; int refills_beside_live = 0, rounds = 0; };

static Run run(int nslots, const std::vector<Script>& jobs, int max_iter, double tol, bool want_err)
{
    MuSched sc(nslots, (int)jobs.size(), max_iter, tol, want_err);
    Run out;
    out.res.resize(jobs.size());
    std::vector<MuPlacement> placed;
    std::vector<MuFinal> finals;
    std::vector<int> ids, converged;
    std::vector<double> errs;
    auto retire = [&](int si) {
        const MuHostSlot& s = sc.slots[si];
        Result& r = out.res[s.job];
        r.n_iter = s.it; r.err = s.err; ++r.retired;
        sc.retire(si);
    };
    for (int pass = 0;; ++pass) {
        CHECK(pass < 100000);
        bool al = true;                                      // the aligned point, worked out here
        int nlive = 0;
        for (const MuHostSlot& s : sc.slots) if (s.job >= 0) { ++nlive; if (s.it % 10 != 0 && s.it < max_iter) al = false; }
        CHECK(nlive <= nslots && sc.aligned() == al);
        if (sc.aligned()) {
            sc.refill(&placed);
            if (!placed.empty() && nlive > 0) ++out.refills_beside_live;
            for (size_t i = 0; i < placed.size(); ++i) {
                CHECK(sc.slots[placed[i].slot].job == placed[i].job && sc.slots[placed[i].slot].it == 0);
                CHECK(i == 0 || (placed[i].slot > placed[i - 1].slot && placed[i].job == placed[i - 1].job + 1));
                ++out.res[placed[i].job].placed;
            }
            sc.due(&ids);
            errs.clear();
            for (int si : ids) {
                const MuHostSlot& s = sc.slots[si];
                CHECK(s.job >= 0 && (s.it % 10 == 0 || s.it >= max_iter));
                out.res[s.job].evals.push_back(s.it);
                errs.push_back(at(jobs[s.job], s.it));
            }
            sc.report(ids, errs, &converged);
            for (int si : converged) retire(si);
        }
        sc.exhausted(&finals);
        for (const MuFinal& f : finals) {
            const MuHostSlot& s = sc.slots[f.slot];
            CHECK(s.job >= 0 && s.it == max_iter);
            if (f.eval) {
                CHECK(want_err);
                out.res[s.job].evals.push_back(s.it);
                sc.report_final(f.slot, at(jobs[s.job], s.it));
            }
            retire(f.slot);
        }
        sc.live(&ids);
        CHECK((int)ids.size() <= nslots);
        if (ids.empty()) { if (sc.finished()) break; else continue; }
        for (int si : ids) CHECK(sc.slots[si].it < max_iter && !sc.slots[si].fresh);
        sc.advance(ids);
        ++out.rounds;
    }
    for (const Result& r : out.res) {
        CHECK(r.placed == 1 && r.retired == 1 && r.n_iter >= 0 && r.n_iter <= max_iter);
        CHECK(std::set<int>(r.evals.begin(), r.evals.end()).size() == r.evals.size());     // none twice
    }
    return out;
}

// piecewise-constant script from (iteration, value) pairs
static Script steps(std::initializer_list<std::pair<int, double>> pts, int len)
{
    Script s(len, 0.0);
    for (const auto& p : pts) for (int i = p.first; i < len; ++i) s[i] = p.second;
    return s;
}

static void hand_derived()
{
    typedef std::vector<int> V;
    // (prev - err) / err0 at 10, 20, 30: 0.1, 0.05, 0.005 -> the first multiple of 10 below tol = 0.01 is 30
    const Script a = steps({{0, 100.0}, {10, 90.0}, {20, 85.0}, {30, 84.5}, {40, 84.4}}, 60);
    Run r = run(1, {a}, 200, 0.01, true);
    CHECK(r.res[0].n_iter == 30 && r.res[0].err == 84.5 && r.res[0].evals == V({0, 10, 20, 30}) && r.rounds == 30);
    // tol = 0: to max_iter, no evaluation after the one at installation, one at the end when errors are wanted
    Script lin(300);
    for (int i = 0; i < 300; ++i) lin[i] = 1000.0 - i;                    // never converges at tol = 0.001: 10 / 1000 per period
    r = run(1, {lin}, 25, 0.0, true);
    CHECK(r.res[0].n_iter == 25 && r.res[0].err == 975.0 && r.res[0].evals == V({0, 25}));
    r = run(1, {lin}, 25, 0.0, false);
    CHECK(r.res[0].n_iter == 25 && r.res[0].err == 1000.0 && r.res[0].evals == V({0}));
    r = run(1, {lin}, 30, 0.0, true);
    CHECK(r.res[0].n_iter == 30 && r.res[0].err == 970.0 && r.res[0].evals == V({0, 30}));
    // exactly one final evaluation, at it == max_iter
    r = run(1, {lin}, 7, 0.001, true);
    CHECK(r.res[0].n_iter == 7 && r.res[0].err == 993.0 && r.res[0].evals == V({0, 7}));
    r = run(1, {lin}, 10, 0.001, true);
    CHECK(r.res[0].n_iter == 10 && r.res[0].err == 990.0 && r.res[0].evals == V({0, 10}));
    r = run(1, {lin}, 25, 0.001, true);
    CHECK(r.res[0].n_iter == 25 && r.res[0].err == 975.0 && r.res[0].evals == V({0, 10, 20, 25}));
    // max_iter = 0: every job retires at it = 0 with err = err0 (three jobs through two slots)
    r = run(2, {lin, a, lin}, 0, 0.001, true);
    for (int j = 0; j < 3; ++j) CHECK(r.res[j].n_iter == 0 && r.res[j].evals == V({0}) && r.res[j].err == (j == 1 ? 100.0 : 1000.0));
    CHECK(r.rounds == 0);
    // a slot that converges at an aligned point is refilled only at the next one: job 0 stops at 10, job 2 starts in round 20
    const Script quick = steps({{0, 10.0}}, 10);
    r = run(2, {quick, lin, quick}, 40, 0.001, true);
    CHECK(r.res[0].n_iter == 10 && r.res[1].n_iter == 40 && r.res[2].n_iter == 10 && r.rounds == 40 && r.refills_beside_live == 1);
    r = run(1, {quick, lin, quick}, 40, 0.001, true);
    CHECK(r.rounds == 10 + 40 + 10);                                        // one slot: nothing live is an aligned point at once
}

static void seeded(int nslots, int njobs, unsigned seed, bool expect_refill)
{
    std::mt19937 rng(seed);
    std::vector<Script> jobs(njobs);
    for (Script& s : jobs) {
        const int len = 10 + (int)(rng() % 191);                            // 10 .. 200
        const double base = 1.0 + (rng() % 1000) / 100.0, rate = 0.90 + (rng() % 90) / 1000.0;
        s.resize(len);
        for (int i = 0; i < len; ++i) s[i] = base * (1.0 + 5.0 * std::pow(rate, i));
    }
    const int max_iter = 150;
    const double tol = 1e-4;
    const Run batch = run(nslots, jobs, max_iter, tol, true);
    std::set<int> distinct;
    for (int j = 0; j < njobs; ++j) {                                       // batch independence of the schedule
        const Run alone = run(1, {jobs[j]}, max_iter, tol, true);
        CHECK(alone.res[0].n_iter == batch.res[j].n_iter && alone.res[0].err == batch.res[j].err);
        CHECK(alone.res[0].evals == batch.res[j].evals);
        CHECK(batch.res[j].n_iter == max_iter || batch.res[j].n_iter % 10 == 0);
        CHECK(batch.res[j].err == at(jobs[j], batch.res[j].n_iter));
        distinct.insert(batch.res[j].n_iter);
    }
    CHECK(njobs < 30 || distinct.size() >= 3);
    CHECK(!expect_refill || batch.refills_beside_live >= 1);
}

int main()
{
    hand_derived();
    seeded(32, 70, 1u, true);
    seeded(32, 33, 2u, true);
    seeded(1, 5, 3u, false);
    puts("ok");
    return 0;
}
