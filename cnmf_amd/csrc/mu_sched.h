// The round scheduler of the multiplicative-update driver (mu_host.hip.h), without a device: which job sits in which
// slot, when the divergence is evaluated, the stopping rule of sklearn's _fit_multiplicative_update (_nmf.py:871-884) and
// retirement.  Plain C++ over the standard library only, so a CPU program can drive it (tests/host/mu_sched_main.cpp);
// mu_host.hip.h does the copies and launches that go with every decision made here.
//
// All live slots advance one iteration per round.  The divergence is evaluated, and free slots are refilled, only at an
// ALIGNED point: every live slot sits at a multiple of 10 iterations (or has used up max_iter), so one host
// synchronisation per 10 iterations serves the whole batch.  One pass of the driver's loop, in this order:
//     if (aligned())  { refill(&placements);  -> install them
//                       due(&slots);          -> evaluate them;  report(slots, errors, &converged);  -> retire those }
//     exhausted(&finals);                     -> per slot: evaluate if .eval, report_final();  retire
//     live(&slots);   none: finished() ? stop : next pass;   else one iteration of them;  advance(slots)
// Slots are always listed in ascending order and jobs are taken in list order.  A slot that converges at an aligned
// point is refilled only at the NEXT aligned point, because the refill runs before the divergence (kept on purpose: a
// restart's iterations do not depend on it, only the round it starts in).
#pragma once

#include <cstddef>
#include <vector>

constexpr int MU_SCHED_MAXSLOTS = 32;      // = MU_MAXSLOTS (kernels_mu_mfma.hip.h): mu_host.hip.h asserts it
constexpr int MU_EVAL_PERIOD = 10;         // iterations between two evaluations of the divergence (sklearn: every 10)

struct MuHostSlot {
    int job = -1;                          // index into the call's job list, -1: free
    int it = 0, err_it = -1;               // iterations done; the iteration `err` was evaluated at
    double err0 = 0, prev = 0, err = 0;    // divergence at installation, at the previous evaluation, at the last one
    bool fresh = false;                    // installed, not yet evaluated
};
struct MuPlacement { int slot, job; };
struct MuFinal { int slot; bool eval; };   // eval: the last evaluation is older than the last iteration -> one more first

struct MuSched {
    const int njobs, max_iter;
    const double tol;
    const bool want_err;                   // the caller asked for the errors: a retiring slot reports the FINAL factors' divergence
    std::vector<MuHostSlot> slots;
    int next = 0;                          // head of the job queue

    MuSched(int nslots, int njobs_, int max_iter_, double tol_, bool want_err_)
        : njobs(njobs_), max_iter(max_iter_), tol(tol_), want_err(want_err_), slots(nslots) {}

    bool aligned() const {
        for (const MuHostSlot& s : slots) if (s.job >= 0 && s.it % MU_EVAL_PERIOD != 0 && s.it < max_iter) return false;
        return true;
    }
    // (aligned points only) the free slots take the next jobs
    void refill(std::vector<MuPlacement>* out) {
        out->clear();
        for (int si = 0; si < (int)slots.size() && next < njobs; ++si)
            if (slots[si].job < 0) {
                slots[si] = MuHostSlot{};
                slots[si].job = next; slots[si].fresh = true;
                out->push_back(MuPlacement{si, next++});
            }
    }
    // (aligned points only) the slots whose divergence is due: at installation, and for the convergence test
    void due(std::vector<int>* out) const {
        out->clear();
        for (int si = 0; si < (int)slots.size(); ++si) {
            const MuHostSlot& s = slots[si];
            if (s.job >= 0 && (s.fresh || (tol > 0 && s.it > 0 && s.it % MU_EVAL_PERIOD == 0))) out->push_back(si);
        }
    }
    // the divergences of due()'s slots; *converged: those the stopping rule ends here (the caller retires them)
    void report(const std::vector<int>& ids, const std::vector<double>& errs, std::vector<int>* converged) {
        converged->clear();
        for (size_t i = 0; i < ids.size(); ++i) {
            MuHostSlot& s = slots[ids[i]];
            s.err_it = s.it;
            if (s.fresh) { s.err0 = s.prev = s.err = errs[i]; s.fresh = false; continue; }
            s.err = errs[i];
            if ((s.prev - s.err) / s.err0 < tol) converged->push_back(ids[i]);
            else s.prev = s.err;
        }
    }
    // the slots that have used up max_iter
    void exhausted(std::vector<MuFinal>* out) const {
        out->clear();
        for (int si = 0; si < (int)slots.size(); ++si) {
            const MuHostSlot& s = slots[si];
            if (s.job >= 0 && s.it >= max_iter) out->push_back(MuFinal{si, want_err && s.err_it != s.it});
        }
    }
    void report_final(int si, double err) { slots[si].err = err; slots[si].err_it = slots[si].it; }
    // the caller has read job, it and err of the slot: it is free from the next aligned point on
    void retire(int si) { slots[si].job = -1; }

    void live(std::vector<int>* out) const {
        out->clear();
        for (int si = 0; si < (int)slots.size(); ++si) if (slots[si].job >= 0) out->push_back(si);
    }
    bool finished() const { return next >= njobs; }        // (ask when nothing is live)
    void advance(const std::vector<int>& ids) { for (int si : ids) slots[si].it++; }
};
