// The plan of the coordinate-descent GEMM passes and sweeps, without a device: split counts, stream-K cuts, sweep
// geometry, the batch width, and the two selectors that name the kernel form a launch takes (gemm_host.hip.h turns the
// names into kernels).  Plain C++ over the standard library only, integer arithmetic over the padded shape and the knob
// values the caller hands in, so a CPU program can check it (tests/host/pass_plan_main.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

// = BK (kernels_gemm.hip.h), G3_MW, G3_JW, G3_BK, G3C_JW (kernels_gemm3.hip.h), KSMALL (kernels_sweep.hip.h):
// batch_host.hip.h asserts all six
constexpr int PLAN_BK = 32, PLAN_G3_MW = 256, PLAN_G3_JW = 128, PLAN_G3C_JW = 256, PLAN_G3_BK = 16, PLAN_KSMALL = 64;

struct PadShape { int N_pad, G_pad; };        // the resident matrix, cells x genes, padded (cnmf_set_matrix)

static inline int plan_round_up(int64_t v, int m) { return (int)(((v + m - 1) / m) * m); }

// ------------------------------------------------------------------ launches that build the X-side operands
// Most blocks a launch may put on grid.y or grid.z.
constexpr int PLAN_GRID_YZ = 65535;

// Does every builder and detection launch of the matrix-pipe path that CNMF_GEMM3 = gemm3 selects fit its grid?  (grid.x
// carries the long dimension everywhere else.)  What rides on grid.y:
//   * the column passes of the count detection (ensure_counts, modes 3 and 4): one chunk of 256 rows each;
//   * the bf16 plane split of X (split3_tiled_kernel, ensure_planes): 64 rows each.  Modes 1 and 2 always take it; mode 3
//     when the matrix turns out to have no count structure; any mode on a shape that is not whole 256 x 256 tiles, where
//     neither the count nor the general f16 path applies.  Mode 4 on whole tiles never does: without the structure it
//     builds the general f16 planes, whose direct builder is flat on grid.x;
//   * every transposed builder (x_planes_kernel, split3_transpose_kernel): 256 genes each.
// A shape that does not fit keeps the f32 pipe (gemm3_enabled).
static inline bool x_launches_fit(PadShape s, int gemm3)
{
    if (gemm3 <= 0) return true;
    const bool whole = s.N_pad % PLAN_G3C_JW == 0 && s.G_pad % PLAN_G3C_JW == 0;
    const bool detects = gemm3 >= 3 && whole;
    const bool bf16_planes = gemm3 <= 3 || !whole;
    if ((s.G_pad + 255) / 256 > PLAN_GRID_YZ) return false;
    if (detects && (s.N_pad + 255) / 256 > PLAN_GRID_YZ) return false;
    if (bf16_planes && s.N_pad % 64 == 0 && s.G_pad % 64 == 0 && s.N_pad / 64 > PLAN_GRID_YZ) return false;
    return true;
}

// ------------------------------------------------------------------ sweeps
// a sweep workgroup walks `sweep_chunks` 256-row tiles; parts_knob = CNMF_SWEEP_PARTS, most workgroups per slot
static inline int sweep_chunks(int parts_knob, int L) { const int64_t m = 256ll * parts_knob; return std::max(1, (int)(((int64_t)L + m - 1) / m)); }
// partials per slot of a half-step: one per sweep workgroup
static inline int sweep_parts(int parts_knob, int L) { const int c = sweep_chunks(parts_knob, L); return (L + 256 * c - 1) / (256 * c); }

// The six forms of sweep_kernel.  W: the W half-step (32-bit slot-relative addressing), W_PLN: ... writing the f16 planes
// of its result, *_A64: their flat-address twins, H_RMX: exact row maxima (the H half-step of the f16 split), H_PSUM:
// ... with the split-K planes summed in the sweep.  Tier 8 (ranks 65..128) runs sweep_big_kernel beside whichever form
// the smaller ranks take, and has neither a PSUM nor a planes form.
enum class SweepForm { W, W_A64, W_PLN, W_PLN_A64, H_RMX, H_PSUM, INVALID };

// the W half-step kernels address a slot with 32-bit byte offsets from its first column (sweep_body, B32): the largest
// is 64 columns * ldv * 4.  A leading dimension too long for 31 bits takes their flat-address form.
static inline bool sweep_a64(int ldv) { return 64ll * ldv * 4 > 0x7fffffffll; }

static inline SweepForm sweep_form(bool has_planes_out, bool psum, bool exact_rmax, bool a64, int tiers = 7)
{
    if (has_planes_out) {           // ranks <= 64 only, no other report, products already reduced
        if (psum || exact_rmax || (tiers & 8)) return SweepForm::INVALID;
        return a64 ? SweepForm::W_PLN_A64 : SweepForm::W_PLN;
    }
    if (psum) return (tiers & 8) ? SweepForm::INVALID : SweepForm::H_PSUM;     // (ranks > 64: the caller reduces first)
    if (exact_rmax) return SweepForm::H_RMX;
    return a64 ? SweepForm::W_A64 : SweepForm::W;
}

// ------------------------------------------------------------------ K splits of the GEMM passes
static inline int pick_nsplit(PadShape s, int KC)
{
    // pass B grid = ceil(G_pad/128) x (KC/128 or 1) x nsplit ; aim at ~2 workgroups per CU
    const int jt = (s.G_pad + 127) / 128;
    const int mg = std::max(1, KC / 128);
    int n = std::max(1, 512 / (jt * mg));
    const int max_by_k = std::max(1, s.N_pad / 256);   // at least 256 cells of K per split
    return std::min(n, max_by_k);
}

// splits that actually receive work once the per-split K range is rounded up to whole stages
static inline int effective_splits(int Ktot, int nsplit)
{
    const int Kper = plan_round_up((Ktot + nsplit - 1) / nsplit, PLAN_BK);
    return (Ktot + Kper - 1) / Kper;
}

// pass A on few cells: fewer than one 128-cell tile per CU -> split the gene (K) range too, so
// that ~2 workgroups per CU are in flight; the planes are summed by reduce_splits_kernel.
static inline int pick_nsplit_A(PadShape s, int KC)
{
    const int T = (s.N_pad / 128) * std::max(1, KC / 128);
    if (T > 256) return 1;                                  // stream-K territory
    int n = std::max(1, 512 / T);
    n = std::min(n, std::max(1, s.G_pad / (4 * PLAN_BK)));  // at least 4 stages per split
    return effective_splits(s.G_pad, std::min(n, 16));
}

// persistent workgroups of the split-operand GEMMs (CNMF_WG_SLOTS: fewer than CUs -- leaves whole CUs to the kernels of
// another stream); gemm3 = CNMF_GEMM3
static inline int gemm3_wg_slots(int gemm3, int wg_slots_knob)
{
    if (wg_slots_knob >= 32 && gemm3 >= 2) return wg_slots_knob;
    return gemm3 >= 2 ? 256 : 512;
}

// pass A of the split-operand kernels on few cell tiles (no stream-K below 3/4 of the workgroup slots):
// K splits so that about one workgroup per slot is in flight, >= 8 blocks each
static inline int pick_nsplit_A3(PadShape s, int KC, int jw, int wg_slots)
{
    const int T = std::max(1, s.N_pad / jw) * std::max(1, KC / PLAN_G3_MW);
    const int Kb = s.G_pad / PLAN_G3_BK;
    int n = std::max(1, std::min(wg_slots / T, Kb / 8));
    const int kb_per = (Kb + n - 1) / n;
    return (Kb + kb_per - 1) / kb_per;
}

static inline int pick_nsplit3(PadShape s, int KC, int jw, int wg_slots)
{
    // pass B grid = (G_pad/jw) x (KC/256) x nsplit; aim at one (two) workgroups per CU, >= 16 blocks per split
    const int tiles = std::max(1, s.G_pad / jw) * std::max(1, KC / PLAN_G3_MW);
    const int Kb = s.N_pad / PLAN_G3_BK;
    int n = std::max(1, std::min(wg_slots / std::max(1, tiles), Kb / 16));
    const int kb_per = (Kb + n - 1) / n;
    return (Kb + kb_per - 1) / kb_per;
}

// partial planes the product buffers of a batch are sized for (ensure_batch): every pipe the width KC may run on
struct SplitCaps { int nsplit, nsplitA; };
static inline SplitCaps size_splits(PadShape s, int KC, bool use3, int wg_slots)
{
    SplitCaps c{pick_nsplit(s, KC), pick_nsplit_A(s, KC)};
    if (use3) {
        c.nsplit = std::max(c.nsplit, std::max(pick_nsplit3(s, KC, PLAN_G3_JW, wg_slots), pick_nsplit3(s, KC, PLAN_G3C_JW, wg_slots)));
        c.nsplitA = std::max(c.nsplitA, std::max(pick_nsplit_A3(s, KC, PLAN_G3_JW, wg_slots), pick_nsplit_A3(s, KC, PLAN_G3C_JW, wg_slots)));
    }
    return c;
}

// ------------------------------------------------------------------ stream-K pass A
// T layout of the f32 pipe: 128 components x 128 cells per tile, one cut per tile
struct StreamK {
    bool on = false;
    int MG = 1, T = 0, nk = 0, P = 0, mw = 128;      // mw: component rows per workgroup tile
    std::vector<unsigned char> split;
};

static inline StreamK plan_streamk(int KC, PadShape s, int n_wg_slots, bool no_streamk)
{
    StreamK sk;
    if (KC % 128 != 0 || no_streamk) return sk;
    sk.MG = KC / sk.mw;
    sk.T = sk.MG * (s.N_pad / 128);
    sk.nk = s.G_pad / PLAN_BK;                             // stages per tile, as the kernel counts them
    sk.P = n_wg_slots;
    if (sk.T <= sk.P) sk.P = n_wg_slots / 2;              // one workgroup per CU
    if (sk.T <= sk.P || sk.T % sk.P == 0) return sk;      // nothing to balance
    sk.on = true;
    sk.split.assign(sk.T, 0);
    const long long U = (long long)sk.T * sk.nk;
    for (int p = 1; p < sk.P; ++p) {
        const long long b = U * p / sk.P;                  // first unit of workgroup p
        if (b % sk.nk) sk.split[b / sk.nk] = 1;            // boundary inside a tile -> that tile is cut
    }
    return sk;
}

// split-operand pass A: tile = 256 components x jw cells, up to 2 cuts per tile
struct StreamK3 {
    bool on = false;
    int T = 0, Kb = 0, P = 0, MG = 1;     // Kb: work units per tile (16-k blocks / `unit`)
    std::vector<unsigned char> flags;     // bit 0: >= 1 cut (plane 1 holds the tail), bit 1: 2 cuts (plane 2 the middle)
};

static inline StreamK3 plan_streamk3(int KC, PadShape s, int n_wg_slots, int jw, int unit, bool no_streamk)
{
    StreamK3 sk;
    sk.MG = KC / PLAN_G3_MW;
    sk.T = sk.MG * (s.N_pad / jw);
    sk.Kb = s.G_pad / (PLAN_G3_BK * unit);
    sk.P = n_wg_slots;
    if (sk.T < sk.P / 2 + sk.P / 4 || sk.P > 2 * sk.T || no_streamk) return sk;   // few tiles: K split + reduce instead
    sk.on = true;
    sk.flags.assign(sk.T, 0);
    const long long U = (long long)sk.T * sk.Kb;
    // the kernels walk the tiles component-group-major (o = mg * NJ + jt); the sweep looks the flags up by jt * MG + mg
    const int NJ = sk.T / sk.MG;
    for (int p = 1; p < sk.P; ++p) {
        const long long b = U * p / sk.P;
        if (b % sk.Kb) {
            const int o = (int)(b / sk.Kb);
            unsigned char& f = sk.flags[(o % NJ) * sk.MG + o / NJ];
            f = f ? 3 : 1;
        }
    }
    return sk;
}

// ------------------------------------------------------------------ f16 two-plane GEMMs (kernels_gemm2h.hip.h)
// livemask of a width: bit t = the 32 packed columns 32 t .. 32 t + 31
static inline unsigned long long g2_full_mask(int KC) { const int t = KC / 32; return t >= 64 ? ~0ull : ((1ull << t) - 1ull); }

// number of K splits a K-split launch will actually use (the partial planes the reduce must add)
static inline int gemm2h_splits(int Kb, int nsplit, int nsub)
{
    int kb_per = (Kb + nsplit - 1) / nsplit;
    kb_per = ((kb_per + nsub - 1) / nsub) * nsub;            // whole steps
    return (Kb + kb_per - 1) / kb_per;
}

// 16-k sub-blocks per barrier pair: 2 on the one-plane count path (nsub_knob = CNMF_G2_NSUB = 1: one), 1 with a second X plane
static inline int gemm2h_nsub(bool hi, int Kb, int nsub_knob) { return (!hi && nsub_knob == 2 && Kb % 2 == 0) ? 2 : 1; }

// The instantiation of gemm2h_kernel / gemm2h_streamk_kernel a launch takes (the K-split kernel has no NTB parameter).
//   hi     : X has a second plane                gen    : ... and a column scale: a general matrix (X itself as two planes)
//   gen4   : CNMF_G2_GEN4, all four plane pairs of a general matrix instead of three (GEN)
//   gvar   : CNMF_G2_GVAR, 0 = general matrices on the burst loop, else the spread stream (VAR 4); same bits
//   nsub   : gemm2h_nsub of the launch            part   : the live mask has a dead 32-column tile
//   shared : several component groups share every X tile in the L2 -- no non-temporal loads then (NTB)
//   u8     : the count plane is held as bytes (ensure_counts; CNMF_G2_U8) -- the byte form (U8) of the two-block count stream
// A column scale without a second plane does not exist (invalid).  The one-block count stream (nsub 1 without a second
// plane) has no partial-tile form: it multiplies the dead tiles too.
struct G2Form {
    bool valid; int NSUB; bool HI; int VAR; bool NTB, PART, GEN; bool U8 = false;
    bool operator==(const G2Form& o) const { return valid == o.valid && NSUB == o.NSUB && HI == o.HI && VAR == o.VAR && NTB == o.NTB && PART == o.PART && GEN == o.GEN && U8 == o.U8; }
};

static inline G2Form g2_form(bool hi, bool gen, bool gen4, int gvar, int nsub, bool part, bool shared, bool u8 = false)
{
    // (a byte plane exists only where the two-block count stream reads it: no second plane, nsub 2)
    if (u8) return (hi || gen || nsub != 2) ? G2Form{false, 1, false, 0, false, false, false} : G2Form{true, 2, false, 4, !part && !shared, part, false, true};
    if (gen && !hi) return G2Form{false, 1, false, 0, false, false, false};
    const bool ntb = !part && !shared;
    if (hi && gen && !gen4) return G2Form{true, 1, true, gvar == 0 ? 0 : 4, ntb, part, true};
    if (hi) return G2Form{true, 1, true, 0, ntb, part, false};
    if (nsub == 2) return G2Form{true, 2, false, 4, ntb, part, false};
    return G2Form{true, 1, false, 4, !shared, false, false};
}

// XCD mapping of the persistent stream-K workgroups (kernel comment).  Count path: every XCD inside ONE component group (1).
// General path (GEN: both X planes, 410 MB at 50 000 x 2 000, re-streamed per component group): the identity order (0) --
// the four groups of a row tile share it in one L2 -- measured +1.3 % (133.7 / 134.1 vs 131.9 / 132.4 restarts/s, round
// 6); the count path measured -2 % with it (round 3).  xmap_knob = CNMF_G2_XMAP = 0|1 forces either.
static inline int g2_xmap(const G2Form& f, int xmap_knob) { return xmap_knob >= 0 ? xmap_knob : (f.GEN ? 0 : 1); }

// geometry of the f16 plane split: tiles of 16 rows x 256 k when K % 256 == 0 (1 KB contiguous per row), else 64 x 64;
// every workgroup walks its k tiles with stride `groups`, so that all workgroups are resident at once (<= 7 per CU)
// and the row scale is reduced once per workgroup
static inline bool split2h_wide(int K) { return K % 256 == 0; }
static inline int split2h_col_groups(int K, int rows)
{
    const int tk = split2h_wide(K) ? 256 : 64, trows = split2h_wide(K) ? 16 : 64;
    const int tiles = K / tk, rg = std::max(1, rows / trows);
    const int cap = std::max(1, (256 * 7) / rg);
    int per = (tiles + cap - 1) / cap;                     // k tiles per workgroup
    return (tiles + per - 1) / per;
}

// ------------------------------------------------------------------ the two GEMM passes at one width
// K splits of pass B (nsplit3 on the split-operand kernels, nsplit on the f32 pipe), and pass A either as a stream-K
// plan (sk3 / sk) or, on few tiles, as nsplitA K splits + reduce.  cap / capA: the partial planes the product buffers
// hold (size_splits at the width they were allocated for).
struct PassPlan {
    int nsplit = 1, nsplit3 = 1, nsplitA = 1;
    StreamK sk;
    StreamK3 sk3;
};

static inline void plan_pass_splits(PassPlan& p, PadShape s, int KC, bool use3, int jwA, int nsubA, int wg_slots, bool no_streamk,
                                    int cap, int capA)
{
    if (use3) {
        p.nsplit3 = std::max(1, std::min(pick_nsplit3(s, KC, jwA, wg_slots), cap));
        p.sk3 = plan_streamk3(KC, s, wg_slots, jwA, nsubA, no_streamk);
        if (!p.sk3.on) p.nsplitA = std::max(1, std::min(pick_nsplit_A3(s, KC, jwA, wg_slots), capA));
    } else {
        p.nsplit = std::max(1, std::min(pick_nsplit(s, KC), cap));
        p.sk = plan_streamk(KC, s, 2 * 256, no_streamk);        // T-layout pass A: 2 workgroups per CU (73.7 KB LDS each)
        if (p.sk.on) p.nsplitA = 1;
        else p.nsplitA = std::max(1, std::min(pick_nsplit_A(s, KC), capA));
    }
}

// ------------------------------------------------------------------ batch width
// Packed component columns of a call.  32 ... 256 by the total rank of the job (powers of two); on the matrix-pipe
// split-operand paths (`wide_ok`) a larger job runs WIDE, up to 1024 columns = four 256-column component groups per GEMM
// pass: both passes then read every X tile once per 1024 columns instead of once per 256, the stream-K partial planes of
// pass A and the latency-bound H half-step are amortised over four times the columns (169 -> 198 -> 215 restarts/s at
// 256 / 512 / 1024 columns, 50 000 x 2000); the batch narrows in 256-column steps once the queue is dry (compact()).
// kc_max: 0 = auto, else an upper bound (multiple of 32; above 256 in steps of 256, up to kc_limit = CNMF_KC_LIMIT,
// default 1024); kc_knob = CNMF_KC.
static inline int pick_kc(int kc_knob, int kc_limit, int64_t total_k, int max_k, int kc_max, bool wide_ok)
{
    if (kc_knob >= 32) kc_max = kc_knob;
    const bool autosize = kc_max <= 0;
    if (autosize) kc_max = 256;
    kc_max = std::max(32, std::min(kc_limit, (kc_max / 32) * 32));
    if (kc_max > 256) kc_max = wide_ok ? (kc_max / 256) * 256 : 256;
    int kc = 32;
    while (kc < std::min(kc_max, 256) && kc < total_k) kc *= 2;
    kc = std::min(kc, kc_max);
    if (wide_ok && kc == 256 && total_k > 256) {
        // as wide as the job, up to the limit: a job that fits entirely starts every restart at once and the batch
        // narrows behind the ones that finish (compact()); measured and simulated on the iteration counts of the
        // north-star job (tools/sim_schedule.py): 113 restarts run 187 / 172 / 145 restarts/s at 1024 / 512 / 256 columns
        if (autosize) kc = (int)std::min<int64_t>(kc_limit, plan_round_up(total_k, 256));
        else if (!autosize && kc_max > 256) kc = (int)std::min<int64_t>(kc_max, plan_round_up(total_k, 256));
    }
    if (kc < max_k) kc = plan_round_up(max_k, 32);
    return kc;
}
