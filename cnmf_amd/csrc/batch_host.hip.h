// The restart engine: batch buffers, the slot scheduler (run_batch) and the NNLS refit
// (included by cnmf_hip.hip after gemm_host.hip.h).  The scheduler's decisions and books are batch_sched.h (no HIP).
#pragma once

#include "batch_sched.h"

// ------------------------------------------------------------------ batch buffers
static_assert(PLAN_BK == BK && PLAN_G3_MW == G3_MW && PLAN_G3_JW == G3_JW && PLAN_G3C_JW == G3C_JW && PLAN_G3_BK == G3_BK &&
              PLAN_KSMALL == KSMALL, "pass_plan.h repeats the tile constants of the kernel headers");
static PadShape pad_shape(const cnmf_ctx* ctx) { return PadShape{ctx->N_pad, ctx->G_pad}; }
static int sweep_chunks(const cnmf_ctx* ctx, int L) { return sweep_chunks(ctx->knobs.sweep_parts, L); }
static int sweep_parts(const cnmf_ctx* ctx, int L) { return sweep_parts(ctx->knobs.sweep_parts, L); }

static int ensure_batch(cnmf_ctx* ctx, int KC, int max_k = KMAX, int min_k = 1)
{
    const bool use3 = gemm3_enabled(ctx, KC);
    const SplitCaps caps = size_splits(pad_shape(ctx), KC, use3, gemm3_wg_slots(ctx->knobs));
    const int nsplit = caps.nsplit, nsplitA = caps.nsplitA;
    const int parts = std::max(sweep_parts(ctx, (int)ctx->N), sweep_parts(ctx, (int)ctx->G));
    const size_t gp_need = (size_t)(KC / std::max(1, min_k) + 1) * parts * max_k * max_k;
    if (ctx->bat.kc == KC && ctx->bat.nsplit == nsplit && ctx->bat.nsplitA == nsplitA &&
        ctx->bat.parts == parts && ctx->bat.gram_part_floats >= gp_need && (!use3 || ctx->bat.H3)) return CNMF_OK;
    ctx->bat.release();
    OwnedLocal<BatchBuffersF> b;          // committed below: a failed allocation leaves the context without batch buffers
    const size_t hb = (size_t)KC * ctx->G_pad * sizeof(float);
    const size_t wb = (size_t)KC * ctx->N_pad * sizeof(float);
    HIP_TRY(ctx, hipMalloc(&b.H, hb));
    HIP_TRY(ctx, hipMalloc(&b.Wt, wb));
    HIP_TRY(ctx, hipMalloc(&b.XHt, wb * nsplitA));
    HIP_TRY(ctx, hipMalloc(&b.XHt1, wb));
    if (use3) {
        HIP_TRY(ctx, hipMalloc(&b.XHt2, wb));
        HIP_TRY(ctx, hipMalloc(&b.H3, (size_t)KC * (ctx->G_pad / 16) * G3_ROWB));
        HIP_TRY(ctx, hipMalloc(&b.Wt3, (size_t)KC * (ctx->N_pad / 16) * G3_ROWB));
        HIP_TRY(ctx, hipMemsetAsync(b.Wt3, 0, (size_t)KC * (ctx->N_pad / 16) * G3_ROWB, ctx->stream));
        // f16 two-plane split: row-maximum partials written by the sweeps ([KC][parts]) and 2^-s per row
        HIP_TRY(ctx, hipMalloc(&b.rmaxH, (size_t)KC * parts * sizeof(float)));
        HIP_TRY(ctx, hipMalloc(&b.rmaxW, (size_t)KC * parts * sizeof(float)));
        HIP_TRY(ctx, hipMalloc(&b.iscaleH, (size_t)KC * sizeof(float)));
        HIP_TRY(ctx, hipMalloc(&b.iscaleW, (size_t)KC * sizeof(float)));
        HIP_TRY(ctx, hipMemsetAsync(b.rmaxH, 0, (size_t)KC * parts * sizeof(float), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(b.rmaxW, 0, (size_t)KC * parts * sizeof(float), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(b.iscaleH, 0, (size_t)KC * sizeof(float), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(b.iscaleW, 0, (size_t)KC * sizeof(float), ctx->stream));
        HIP_TRY(ctx, hipMalloc(&b.shiftW, (size_t)3 * KC * sizeof(int)));
        HIP_TRY(ctx, hipMemsetAsync(b.shiftW, 0, (size_t)3 * KC * sizeof(int), ctx->stream));
    }
    HIP_TRY(ctx, hipMalloc(&b.d_split, (size_t)(KC / 32 + 1) * (ctx->N_pad / 128 + 1)));
    HIP_TRY(ctx, hipMalloc(&b.XtW, hb * nsplit));
    HIP_TRY(ctx, hipMalloc(&b.gramH, (size_t)KC * GRAM_SZ * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(&b.gramW, (size_t)KC * GRAM_SZ * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(&b.gram_part, gp_need * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(&b.viol_part, (size_t)KC * parts * sizeof(double)));
    HIP_TRY(ctx, hipMalloc(&b.d_slots, (size_t)KC * sizeof(SlotDesc)));
    HIP_TRY(ctx, hipMalloc(&b.d_slot_list, (size_t)KC * RING * sizeof(int)));
    HIP_TRY(ctx, hipHostMalloc(&b.h_slots, (size_t)KC * sizeof(SlotDesc)));
    // device-written, host-polled: coherent mapped pinned memory (zero-copy snapshots of the slot table)
    HIP_TRY(ctx, hipHostMalloc(&b.h_snap, (size_t)KC * RING * sizeof(SlotDesc),
                               hipHostMallocMapped | hipHostMallocCoherent));
    memset(b.h_snap, 0, (size_t)KC * RING * sizeof(SlotDesc));
    HIP_TRY(ctx, hipHostMalloc(&b.h_slot_list, (size_t)KC * RING * sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(b.H, 0, hb, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b.Wt, 0, wb, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b.XHt, 0, wb * nsplitA, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b.XtW, 0, hb * nsplit, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(b.d_slots, 0, (size_t)KC * sizeof(SlotDesc), ctx->stream));
    b.kc = KC; b.nsplit = nsplit; b.nsplitA = nsplitA; b.parts = parts; b.gram_part_floats = gp_need;
    ctx->bat.take(b);
    return CNMF_OK;
}

static int ensure_stage(cnmf_ctx* ctx, size_t wfloats, size_t hfloats)
{
    if (wfloats > ctx->stageW_sz) {
        hipFree(ctx->stageW); ctx->stageW = nullptr;
        HIP_TRY(ctx, hipMalloc(&ctx->stageW, wfloats * sizeof(float)));
        ctx->stageW_sz = wfloats;
    }
    if (hfloats > ctx->stageH_sz) {
        hipFree(ctx->stageH); ctx->stageH = nullptr;
        HIP_TRY(ctx, hipMalloc(&ctx->stageH, hfloats * sizeof(float)));
        ctx->stageH_sz = hfloats;
    }
    return CNMF_OK;
}

// Poll the stamps of one zero-copy snapshot (finalize_kernel -> publish_slot) until all `n` slots carry
// `stamp`.  The snapshot is `lag` iterations old when it is needed, so this normally returns at once.
static int wait_snapshot(cnmf_ctx* ctx, const SlotDesc* sp, int n, int stamp)
{
    // Pure spinning on the host-mapped stamp.  The stream is queried (to notice a dead stream instead of spinning for
    // ever) only after 20 ms without progress: hipStreamQuery on a busy stream makes the runtime append a completion
    // marker behind the last enqueued kernel -- here always the H finalize -- and the GPU then pays ~6 us for that
    // barrier packet in front of every pass A (measured: the finalize -> pass A gap of round 2's kernel traces).
    using clk = std::chrono::steady_clock;
    for (int s = 0; s < n; ++s) {
        const volatile int* flag = &sp[s].pad_;
        long spins = 0;
        clk::time_point t0;
        bool timing = false;
        while (*flag != stamp) {
            if (++spins % 4096 != 0) continue;
            if (!timing) { t0 = clk::now(); timing = true; continue; }
            if (std::chrono::duration_cast<std::chrono::milliseconds>(clk::now() - t0).count() < 20) continue;
            t0 = clk::now();
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) {                       // stream drained: the stamp must be there
                if (*flag == stamp) break;
                SET_ERR(ctx, "slot snapshot %d was never published (slot %d)", stamp, s);
                return CNMF_EHIP;
            }
            if (q != hipErrorNotReady) {
                SET_ERR(ctx, "stream failed while waiting for a slot snapshot: %s", hipGetErrorString(q));
                return CNMF_EHIP;
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return CNMF_OK;
}

static int validate_params(cnmf_ctx* ctx, const cnmf_cd_params* p)
{
    if (!p) { SET_ERR(ctx, "params is NULL"); return CNMF_EINVAL; }
    if (!(p->tol >= 0) || p->max_iter < 1) { SET_ERR(ctx, "bad tol/max_iter"); return CNMF_EINVAL; }
    if (p->l1_reg_W < 0 || p->l2_reg_W < 0 || p->l1_reg_H < 0 || p->l2_reg_H < 0) {
        SET_ERR(ctx, "negative regularisation"); return CNMF_EINVAL;
    }
    return CNMF_OK;
}

// ------------------------------------------------------------------ the operand scheme of the GEMM passes
static_assert(SCHED_KMAX == KMAX && SCHED_RING == RING, "batch_sched.h repeats KMAX and RING");

// Which kernels the two GEMM passes of an iteration run on, and what they read of X.  Filled once per call by
// pick_scheme; the tail turns it into the f32 scheme when it narrows below 256 packed columns.
struct PassScheme {
    bool use3 = false;      // split-operand bf16 MFMA path (whole 256-column tiles only)
    bool usec = false;      // ... with X as one integer plane (count-structured data)
    bool use2g = false;     // any OTHER matrix in the default mode: X itself as two f16 planes with a per-row exponent, 4 MFMAs
                            // per product (gemm_mode 5; CNMF_GEMM3=1|2 keep the 3 x 3 bf16 planes of rounds 1-2, 6 MFMAs)
    bool use2h = false;     // ... on the f16 pipe: two f16 factor planes
    int mode = 0;           // cnmf_batch_stats.gemm_mode
    // the X-side operands of the count and f16 kernels: the integer count plane(s), or the two planes of a general matrix
    XOperand xA{}, xB{};
    const double* dsc = nullptr;            // per-gene scale of the count path
    int jwA = G3_JW;                        // width of a pass-A / pass-B tile
    int nsubA = 1, nsubB = 1, KbA = 0, KbB = 0;
    void leave_matrix_pipe() { use3 = usec = use2h = use2g = false; }     // fewer than 256 packed columns: the f32 pipe
};

static int pick_scheme(cnmf_ctx* ctx, int KC, PassScheme* out)
{
    const CdKnobs& kn = ctx->knobs;
    PassScheme p;
    int rc;
    p.use3 = gemm3_enabled(ctx, KC);
    if (p.use3 && kn.gemm3 >= 3) {
        if ((rc = ensure_counts(ctx))) return rc;
        p.usec = ctx->counts.state == 1;
    }
    p.use2g = p.use3 && !p.usec && kn.gemm3 >= 4 && ctx->G_pad % G3C_JW == 0 && ctx->N_pad % G3C_JW == 0;
    if (p.use2g && (rc = ensure_x2planes(ctx))) return rc;
    p.use2h = (p.usec && ctx->counts.fmt >= 4) || p.use2g;
    p.mode = !p.use3 ? 0 : (p.use2g ? 5 : (p.usec ? (p.use2h ? 4 : 3) : std::min(kn.gemm3, 2)));
    p.KbA = ctx->G_pad / 16; p.KbB = ctx->N_pad / 16;
    p.xA = p.use2g ? ctx->x2.passA() : ctx->counts.passA();
    p.xB = p.use2g ? ctx->x2.passB() : ctx->counts.passB();
    p.dsc = p.use2g ? nullptr : ctx->counts.d_scale;
    p.nsubA = p.use2h ? gemm2h_nsub(p.xA.hi != nullptr, p.KbA, kn.g2_nsub) : 1;
    p.nsubB = p.use2h ? gemm2h_nsub(p.xB.hi != nullptr, p.KbB, kn.g2_nsub) : 1;
    if (p.use3 && !p.usec && !p.use2g && (rc = ensure_planes(ctx))) return rc;
    p.jwA = (p.usec || p.use2g) ? G3C_JW : G3_JW;
    *out = p;
    return CNMF_OK;
}

// ------------------------------------------------------------------ the restart hot loop
// Everything one call of run_batch works with: the job, the call's device buffers, the operand scheme and pass plan, and
// the scheduler (batch_sched.h), which decides and keeps the books while the functions below copy and launch.
struct BatchRun {
    cnmf_ctx* ctx; const cnmf_cd_params* prm; hipStream_t st;
    int n; const int32_t* kk; int init_mode; const double* avg; const float *W0, *H0;
    int32_t* n_iter_out; double* viol_out; bool resident;
    int N, G, max_k; int64_t total_k;
    std::vector<size_t> hoff, woff;                  // first float of restart r in the H / W results and inits
    DevPool pool;
    EventPool events;
    struct PinnedInts { int* p = nullptr; ~PinnedInts() { if (p) hipHostFree(p); } } repack_host;
    float *d_Hres = nullptr, *d_Wres = nullptr;      // device result buffers
    float *d_H0 = nullptr, *d_Wt0 = nullptr;         // init_mode 1: the random factors of every restart, component-major;
                                                     // init_mode 2: the context's init store (same layout)
    int* d_repack = nullptr;                         // re-packing: column map, moved slot ids, their new offsets
    int n_repack = 0;
    PassScheme ps;
    // W planes written by the W sweep itself (kernels_sweep.hip.h, PLN) instead of a separate pass over W; ranks above
    // 64 (sweep_big_kernel) keep the separate split for the whole call.
    bool fuseW = false;
    int shgen = 0;                                   // generation of the exponents the NEXT W sweep uses
    int* shW[2] = {nullptr, nullptr};
    bool h3_valid = false;                           // H3 holds the planes of the current H (split-operand modes)
    int fin_y = 1, lag = 2;                          // finalize blocks per slot; iterations the inspected snapshot lies behind
    int chunksW, partsW, chunksH, partsH;
    float l1W, l2W, l1H, l2H;
    PassPlan plan;                                   // the two GEMM passes at the current width, on the pipe `ps.use3` names (plan_passes)
    // HIP events around the two GEMM passes of every `time_stride`-th iteration (an event record costs
    // ~6 us of queue time: bracketing every launch would take 4 % off the throughput it measures)
    int time_stride = 0;
    std::vector<hipEvent_t> gev;                     // (a0,a1,b0,b1) per iteration when timing is requested
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_tail = nullptr;     // ev_tail: recorded when the queue runs dry
    int nsplit3_first = 1;                           // (reported: the tail narrows the batch and re-plans)
    BatchSched sched;
    BatchRun(int n_, const int32_t* kk_, int KC, const double* hint, bool dbg) : n(n_), kk(kk_), sched(n_, kk_, KC, hint, dbg) {}
};

// The plan of the two GEMM passes at the current width KC (plan_pass_splits, pass_plan.h), the cut flags of a stream-K
// pass A uploaded to d_split.  cap / capA: the partial planes the product buffers hold at this width.  Made before the
// loop, and again whenever compact() narrows the batch.
static int plan_passes(BatchRun& b, int cap, int capA)
{
    cnmf_ctx* ctx = b.ctx;
    PassPlan& p = b.plan;
    plan_pass_splits(p, pad_shape(ctx), b.sched.KC, b.ps.use3, b.ps.jwA, b.ps.nsubA, gemm3_wg_slots(ctx->knobs), ctx->knobs.no_streamk, cap, capA);
    const std::vector<unsigned char>* flags = b.ps.use3 ? (p.sk3.on ? &p.sk3.flags : nullptr) : (p.sk.on ? &p.sk.split : nullptr);
    // (the flags of the old plan may still be read by an in-flight sweep: same stream -> ordered)
    if (flags) HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.d_split, flags->data(), flags->size(), hipMemcpyHostToDevice, b.st));
    return CNMF_OK;
}

// copy the factors of a finished slot out of the packed columns and clear its rows; the books: sched.retire
static int retire_slot(BatchRun& b, int s, const SlotDesc& snap)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const HostSlot& h = b.sched.hs[s];
    const int r = h.restart, k = h.k, N = b.N, G = b.G;
    dim3 gH((G + 255) / 256, k), gW((N + 255) / 256, k);
    extract_kernel<<<gH, 256, 0, st>>>(ctx->bat.H, ctx->G_pad, G, h.off, k, b.d_Hres + b.hoff[r], 0);
    if (b.d_Wres) extract_kernel<<<gW, 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, N, h.off, k, b.d_Wres + b.woff[r], 1);
    clear_rows_kernel<<<gH, 256, 0, st>>>(ctx->bat.H, ctx->G_pad, ctx->G_pad, h.off, k);
    clear_rows_kernel<<<gW, 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, ctx->N_pad, h.off, k);
    HIP_TRY(ctx, hipGetLastError());
    if (b.n_iter_out) b.n_iter_out[r] = snap.iter;
    if (b.viol_out) b.viol_out[r] = snap.viol_last;
    b.sched.retire(s, snap.iter);
    return CNMF_OK;
}

// Move the live slots as sched.plan_repack says (through the stage buffers) and zero the rows it leaves free up to
// `width`.  Used by the tail compaction (narrower batch, or balanced at the same width) and by the refill's
// defragmentation (same width).
// (one launch sequence per re-packing, whatever the number of slots: at 1024 packed columns the per-slot moves of
//  round 2 -- four launches each, host-bound at ~5 us per launch -- had grown to 10 % of the wall time)
static int repack(BatchRun& b, int width, bool balanced = false)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const int KC0 = b.sched.KC0;
    int* hm = b.repack_host.p + (size_t)(b.n_repack++ % RING) * 3 * KC0;      // [colmap | slot ids | new offsets], pinned
    int* d_colmap = b.d_repack, *d_ids = b.d_repack + KC0, *d_offs = b.d_repack + 2 * KC0;
    const RepackPlan pl = b.sched.plan_repack(width, balanced, hm);
    if (pl.nmove || pl.pos < width) {
        HIP_TRY(ctx, hipMemcpyAsync(d_colmap, hm, (size_t)width * sizeof(int), hipMemcpyHostToDevice, st));
        // staging = the product buffers (scratch between two iterations): XHt [>= KC0][N_pad], XtW [>= KC0][G_pad]
        gather_rows_cm_kernel<<<dim3((ctx->N_pad / 4 + 255) / 256, width), 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, d_colmap, ctx->bat.XHt);
        gather_rows_cm_kernel<<<dim3((ctx->G_pad / 4 + 255) / 256, width), 256, 0, st>>>(ctx->bat.H, ctx->G_pad, d_colmap, ctx->bat.XtW);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.Wt, ctx->bat.XHt, (size_t)width * ctx->N_pad * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.H, ctx->bat.XtW, (size_t)width * ctx->G_pad * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (b.fuseW) {
            int* tmp = ctx->bat.shiftW + 2 * ctx->bat.kc;
            for (int g2 = 0; g2 < 2; ++g2) {
                permute_ints_kernel<<<(width + 255) / 256, 256, 0, st>>>(b.shW[g2], d_colmap, tmp, width);
                HIP_TRY(ctx, hipMemcpyAsync(b.shW[g2], tmp, (size_t)width * sizeof(int), hipMemcpyDeviceToDevice, st));
            }
            HIP_TRY(ctx, hipGetLastError());
        }
        if (pl.nmove) {
            HIP_TRY(ctx, hipMemcpyAsync(d_ids, hm + KC0, (size_t)pl.nmove * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_offs, hm + 2 * KC0, (size_t)pl.nmove * sizeof(int), hipMemcpyHostToDevice, st));
            set_slot_offs_kernel<<<(pl.nmove + 255) / 256, 256, 0, st>>>(ctx->bat.d_slots, d_ids, d_offs, pl.nmove);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    b.h3_valid = false;               // rows of H moved: its planes are stale
    // moved rows of slots that no longer iterate are not swept again: refresh their row maxima here
    if (b.ps.use2h) HIP_TRY(ctx, launch_rowmax_part(st, ctx->bat.Wt, ctx->N_pad, b.N, b.sched.KC, b.chunksW * 256, nullptr, b.partsW, ctx->bat.rmaxW));
    return CNMF_OK;
}

// copy the initial factors of one placed restart into its packed columns and write its slot descriptor
static int install(BatchRun& b, const Placement& p)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const int r = p.restart, k = p.k, off = p.off, N = b.N, G = b.G;
    dim3 gI((std::max(N, G) + 255) / 256, k);
    if (b.init_mode == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->stageH, b.H0 + b.hoff[r], (size_t)k * G * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->stageW, b.W0 + b.woff[r], (size_t)k * N * sizeof(float), hipMemcpyHostToDevice, st));
        install_kernel<<<gI, 256, 0, st>>>(ctx->stageH, ctx->stageW, ctx->bat.H, ctx->G_pad, G, ctx->bat.Wt, ctx->N_pad, N, off, k);
    } else {
        install_cm_kernel<<<gI, 256, 0, st>>>(b.d_H0 + b.hoff[r], b.d_Wt0 + b.woff[r], ctx->bat.H, ctx->G_pad, G, ctx->bat.Wt, ctx->N_pad, N, off);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (b.fuseW) {
        // exponent of the planes the FIRST W sweep of this restart writes: from the size of its W0 (random init:
        // avg |N(0,1)|, the maximum of 50 000 draws is ~4.5 avg), two bits of headroom; the check behind the sweep
        // re-converts the rows whose first update left the window
        float mx = 0.f;
        if (b.init_mode == 1) mx = 6.0f * (float)b.avg[r];
        else if (b.init_mode == 2) mx = ctx->inits.maxW[r];
        else for (size_t q = 0; q < (size_t)k * N; ++q) mx = std::max(mx, b.W0[b.woff[r] + q]);
        int e2 = 0;
        if (mx > 0.f) std::frexp(mx, &e2);
        const int sh0 = mx > 0.f ? std::max(-110, std::min(120, 13 - e2)) : 0;
        set_ints_kernel<<<1, 128, 0, st>>>(b.shW[0], b.shW[1], off, k, sh0);
        HIP_TRY(ctx, hipGetLastError());
    }
    SlotDesc* d = &ctx->bat.h_slots[p.slot];
    memset(d, 0, sizeof *d);
    d->off = off; d->k = k; d->active = 1; d->iter = 0; d->restart = r;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.d_slots + p.slot, d, sizeof(SlotDesc), hipMemcpyHostToDevice, st));
    return CNMF_OK;
}

// ---- step 1: refill free columns from the pending list (n_new = slots installed)
static int refill(BatchRun& b, int& n_new)
{
    cnmf_ctx* ctx = b.ctx;
    BatchSched& sc = b.sched;
    n_new = 0;
    int* new_list = ctx->bat.h_slot_list + (size_t)(sc.it % RING) * sc.KC0;
    int rc;
    sc.begin_refill();
    while (true) {
        Placement p;
        while (sc.next_placement(&p)) {
            if ((rc = install(b, p))) return rc;
            new_list[n_new++] = p.slot;
        }
        if (!sc.defrag_due()) break;
        if ((rc = repack(b, sc.KC))) return rc;
        sc.defragmented();
    }
    if (n_new) {
        int* dl = ctx->bat.d_slot_list + (size_t)(sc.it % RING) * sc.KC0;
        HIP_TRY(ctx, hipMemcpyAsync(dl, new_list, n_new * sizeof(int), hipMemcpyHostToDevice, b.st));
        gram_rows_kernel<<<n_new, 256, 0, b.st>>>(ctx->bat.H, ctx->G_pad, b.G, ctx->bat.d_slots, dl, ctx->bat.gramH, b.l2W);
        HIP_TRY(ctx, hipGetLastError());
    }
    return CNMF_OK;
}

// ---- step 2: the launches of one coordinate-descent outer iteration, in order
// pass A : XHt[KC][N] = H_all . X^T                       (sklearn _nmf.py:387)
// *cutA: where the W sweep finds the stream-K partial planes (plane1 = NULL: one plane, after launch_reduce_splits)
static int launch_pass_a(BatchRun& b, int n_new, unsigned long long livemask, hipEvent_t ev_begin, CutPlanes* cutA)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const PassScheme& ps = b.ps;
    const PassPlan& pl = b.plan;
    const int KC = b.sched.KC, gm = ctx->knobs.gemm3;
    const long long plane = (long long)KC * ctx->N_pad;
    *cutA = NO_CUT;
    if (!ps.use3) {
        if (pl.sk.on) {
            HIP_TRY(ctx, launch_streamk_passA(st, pl.sk, ctx->bat.H, ctx->G_pad, ctx->X, ctx->G_pad, ctx->bat.XHt,
                                              ctx->bat.XHt1, ctx->N_pad, ctx->N_pad));
            *cutA = CutPlanes{ctx->bat.XHt1, ctx->bat.d_split, 128, pl.sk.mw, pl.sk.MG, nullptr};
        } else
            HIP_TRY(ctx, launch_gemm<false>(st, 0, ctx->bat.H, ctx->G_pad, ctx->X, ctx->G_pad, ctx->bat.XHt,
                                            ctx->N_pad, plane, KC, ctx->G_pad, ctx->N_pad, pl.nsplitA));
        return CNMF_OK;
    }
    // H3 was produced together with the previous iteration's H finalize; rows installed since then
    // (and the very first iteration) need a split of their own.  Count path: H' = H * d.
    if ((n_new > 0 || !b.h3_valid) && ps.use2h) {
        HIP_TRY(ctx, launch_rowmax_part(st, ctx->bat.H, ctx->G_pad, b.G, KC, b.chunksH * 256, ps.dsc, b.partsH, ctx->bat.rmaxH));
        HIP_TRY(ctx, launch_split2h(st, ctx->bat.H, ctx->G_pad, KC, ctx->G_pad, ctx->bat.H3, G3_MW, ps.dsc, ctx->bat.rmaxH,
                                    b.partsH, ctx->bat.iscaleH));
    } else if (n_new > 0 || !b.h3_valid)
        HIP_TRY(ctx, launch_split3(st, ctx->bat.H, ctx->G_pad, KC, ctx->G_pad, ctx->bat.H3, G3_MW, ps.usec ? ctx->counts.d_scale : nullptr));
    if (ev_begin) hipEventRecord(ev_begin, st);          // (timed iterations: the pass without the split in front of it)
    if (ps.use2h) {
        G2Launch g;
        g.A2 = ctx->bat.H3; g.rscale = ctx->bat.iscaleH; g.x = ps.xA; g.Kb = ps.KbA;
        g.C[0] = ctx->bat.XHt; g.C[1] = ctx->bat.XHt1; g.C[2] = ctx->bat.XHt2; g.ldc = ctx->N_pad;
        g.livemask = livemask; g.kn = &ctx->knobs;
        if (pl.sk3.on) { g.sk = &pl.sk3; HIP_TRY(ctx, launch_gemm2h_streamk(st, g)); }
        else { g.cstride = plane; g.KC = KC; g.Jpad = ctx->N_pad; g.nsplit = pl.nsplitA; HIP_TRY(ctx, launch_gemm2h(st, g)); }
    } else if (pl.sk3.on) {
        if (ps.usec)
            HIP_TRY(ctx, launch_gemm3c_streamk(st, pl.sk3, ctx->bat.H3, ps.xA.plane, ps.xA.hi, ps.xA.flags, ctx->bat.XHt, ctx->bat.XHt1,
                                               ctx->bat.XHt2, ctx->N_pad));
        else
            HIP_TRY(ctx, launch_gemm3_streamk(st, pl.sk3, ctx->bat.H3, ctx->planes.X3, ctx->bat.XHt, ctx->bat.XHt1, ctx->bat.XHt2, ctx->N_pad, gm));
    } else if (ps.usec)
        HIP_TRY(ctx, launch_gemm3c(st, ctx->bat.H3, ps.xA.plane, ps.xA.hi, ps.xA.flags, ctx->G_pad / 16, ctx->bat.XHt, ctx->N_pad,
                                   plane, KC, ctx->N_pad, pl.nsplitA));
    else
        HIP_TRY(ctx, launch_gemm3(st, ctx->bat.H3, ctx->planes.X3, ctx->G_pad / 16, ctx->bat.XHt, ctx->N_pad,
                                  plane, KC, ctx->N_pad, pl.nsplitA, gm));
    if (pl.sk3.on) *cutA = CutPlanes{ctx->bat.XHt1, ctx->bat.d_split, ps.jwA, G3_MW, pl.sk3.MG, ctx->bat.XHt2};
    return CNMF_OK;
}

// the finalize of a half-step on the f32 pipe, without a plane split
static void launch_finalize(BatchRun& b, const FinalizeArgs& fa)
{
    finalize_kernel<<<dim3(b.sched.nslots, b.fin_y), 256, 0, b.st>>>(fa.gram_part, fa.viol_part, fa.nparts, fa.gram_out, fa.l2_reg,
                                                                   fa.slots, fa.phase, fa.tol, fa.max_iter, fa.want_gram, fa.gld,
                                                                   fa.snap_out, fa.stamp);
}

// finalize of the W sweep: Gram matrix of W and the stopping rule's sums; on the split-operand paths the plane split of
// the sweep's result rides in the same launch (writing the bf16 planes from inside the sweep was measured slower: 2-byte
// stores, lower occupancy; f16, fused: the sweep wrote the planes, this launch checks their exponents, publishes 2^-s and
// the next exponents)
static int launch_w_finalize(BatchRun& b)
{
    cnmf_ctx* ctx = b.ctx;
    const int KC = b.sched.KC, nslots = b.sched.nslots;
    const FinalizeArgs fa{ctx->bat.gram_part, ctx->bat.viol_part, b.partsW, ctx->bat.gramW, b.l2H, ctx->bat.d_slots, 0, b.prm->tol,
                          b.prm->max_iter, 1, b.max_k, nullptr, 0};
    if (b.ps.use2h) {
        const bool fuse_now = b.fuseW;
        HIP_TRY(ctx, launch_split2h_finalize(b.st, ctx->bat.Wt, ctx->N_pad, KC, ctx->N_pad, ctx->bat.Wt3, G3_MW, nullptr, ctx->bat.rmaxW,
                                             b.partsW, ctx->bat.iscaleW, fa, nslots, b.fin_y,
                                             fuse_now ? SplitFused{b.shW[b.shgen], b.shW[b.shgen ^ 1]} : SplitFused{nullptr, nullptr}));
        if (fuse_now) b.shgen ^= 1;
    } else if (b.ps.use3)
        HIP_TRY(ctx, launch_split3_finalize(b.st, ctx->bat.Wt, ctx->N_pad, KC, ctx->N_pad, ctx->bat.Wt3, G3_MW, nullptr, fa,
                                            nslots, b.fin_y));
    else
        launch_finalize(b, fa);
    return CNMF_OK;
}

// pass B : XtW[S][KC][G] = Wt_all . X  (split over cells)  (sklearn _nmf.py:505-507); *nsB: partial planes it wrote
static int launch_pass_b(BatchRun& b, unsigned long long livemask, int* nsB)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const PassScheme& ps = b.ps;
    const PassPlan& pl = b.plan;
    const int KC = b.sched.KC;
    const long long plane = (long long)KC * ctx->G_pad;
    *nsB = ps.use2h ? gemm2h_splits(ps.KbB, pl.nsplit3, ps.nsubB) : (ps.use3 ? pl.nsplit3 : pl.nsplit);
    if (ps.use2h) {
        G2Launch g;
        g.A2 = ctx->bat.Wt3; g.rscale = ctx->bat.iscaleW; g.x = ps.xB; g.Kb = ps.KbB;
        g.C[0] = ctx->bat.XtW; g.ldc = ctx->G_pad; g.livemask = livemask; g.kn = &ctx->knobs;
        g.cstride = plane; g.KC = KC; g.Jpad = ctx->G_pad; g.nsplit = pl.nsplit3;
        HIP_TRY(ctx, launch_gemm2h(st, g));
    } else if (ps.usec)
        HIP_TRY(ctx, launch_gemm3c(st, ctx->bat.Wt3, ps.xB.plane, ps.xB.hi, ps.xB.flags, ctx->N_pad / 16, ctx->bat.XtW, ctx->G_pad,
                                   plane, KC, ctx->G_pad, pl.nsplit3));
    else if (ps.use3)
        HIP_TRY(ctx, launch_gemm3(st, ctx->bat.Wt3, ctx->planes.Xt3, ctx->N_pad / 16, ctx->bat.XtW, ctx->G_pad,
                                  plane, KC, ctx->G_pad, pl.nsplit3, ctx->knobs.gemm3));
    else
        HIP_TRY(ctx, launch_gemm<true>(st, 0, ctx->bat.Wt, ctx->N_pad, ctx->X, ctx->G_pad, ctx->bat.XtW,
                                       ctx->G_pad, plane, KC, ctx->N_pad, ctx->G_pad, pl.nsplit));
    return CNMF_OK;
}

// what every sweep on the batch buffers shares: the slot table and the partials its finalize reduces
static SweepLaunch batch_sweep(const cnmf_ctx* ctx, int nslots, int kmax, int tiers)
{
    SweepLaunch s;
    s.nslots = nslots; s.kmax = kmax; s.tiers = tiers;
    s.slots = ctx->bat.d_slots; s.gram_part = ctx->bat.gram_part; s.viol_part = ctx->bat.viol_part;
    return s;
}

// H half-step.  On the f16 path the split-K partials are summed (and scaled by d) inside the sweep itself.
static int launch_h_sweep(BatchRun& b, int tiers, int nsB)
{
    cnmf_ctx* ctx = b.ctx;
    const PassScheme& ps = b.ps;
    const long long plane = (long long)b.sched.KC * ctx->G_pad;
    SweepLaunch s = batch_sweep(ctx, b.sched.nslots, b.max_k, tiers);
    s.V = ctx->bat.H; s.ldv = ctx->G_pad; s.L = b.G; s.P = ctx->bat.XtW; s.gram = ctx->bat.gramW; s.l1 = b.l1H;
    s.chunks = b.chunksH; s.parts = b.partsH; s.want_gram = 1;
    if (ps.use2h) { s.rmax_part = ctx->bat.rmaxH; s.rmax_scale = ps.dsc; }
    if (ps.use2h && !ctx->knobs.no_psum && !(tiers & 8)) {      // (ranks above 64 take the separately reduced product)
        s.from = SweepLaunch::SPLIT_SUM; s.sum = SplitSum{nsB, plane, ps.dsc};
    } else
        HIP_TRY(ctx, launch_reduce_splits(b.st, ctx->bat.XtW, nsB, plane, plane, ps.usec ? ps.dsc : nullptr, ctx->G_pad));
    HIP_TRY(ctx, launch_sweep(b.st, s));
    return CNMF_OK;
}

// the H finalize also publishes every slot's state into the host-mapped ring entry of this
// iteration (stamp it + 1): no copy kernel and no event per iteration
static int launch_h_finalize(BatchRun& b)
{
    cnmf_ctx* ctx = b.ctx;
    const PassScheme& ps = b.ps;
    const BatchSched& sc = b.sched;
    SlotDesc* snap = ctx->bat.h_snap + (size_t)(sc.it % RING) * sc.KC0;
    SlotDesc* snap_dev = nullptr;
    HIP_TRY(ctx, hipHostGetDevicePointer((void**)&snap_dev, snap, 0));
    const FinalizeArgs fa{ctx->bat.gram_part, ctx->bat.viol_part, b.partsH, ctx->bat.gramH, b.l2W, ctx->bat.d_slots, 1, b.prm->tol,
                          b.prm->max_iter, 1, b.max_k, snap_dev, (int)(sc.it + 1)};
    if (ps.use2h)
        HIP_TRY(ctx, launch_split2h_finalize(b.st, ctx->bat.H, ctx->G_pad, sc.KC, ctx->G_pad, ctx->bat.H3, G3_MW, ps.dsc,
                                             ctx->bat.rmaxH, b.partsH, ctx->bat.iscaleH, fa, sc.nslots, b.fin_y));
    else if (ps.use3)
        HIP_TRY(ctx, launch_split3_finalize(b.st, ctx->bat.H, ctx->G_pad, sc.KC, ctx->G_pad, ctx->bat.H3, G3_MW,
                                            ps.usec ? ctx->counts.d_scale : nullptr, fa, sc.nslots, b.fin_y));
    else
        launch_finalize(b, fa);
    if (ps.use3) b.h3_valid = true;
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// enqueue one coordinate-descent outer iteration for every slot in flight
static int iterate(BatchRun& b, int n_new)
{
    cnmf_ctx* ctx = b.ctx;
    hipStream_t st = b.st;
    const PassScheme& ps = b.ps;
    BatchSched& sc = b.sched;
    int tiers = 0, rc;
    for (int s2 = 0; s2 < sc.nslots; ++s2)
        if (sc.hs[s2].state) tiers |= sc.hs[s2].k <= 16 ? 1 : (sc.hs[s2].k <= 32 ? 2 : (sc.hs[s2].k <= KSMALL ? 4 : 8));
    // the tail (nothing left to refill with): the f16 kernels skip the 32-column tiles without a live restart.
    // Partial-tile passes were built and measured in round 3 -- 183.0 vs 182.2 restarts/s on the 113-restart shard, 216.5 vs
    // 215.7 on the full job: within noise (a tail pass is bound by streaming the count plane as much as by its MFMAs).
    // Opt-in: CNMF_PART=1 (knobs.part).
    unsigned long long livemask = ~0ull;
    if (ps.use2h && sc.n_pending == 0 && ctx->knobs.part) {
        // the skipping variant of the kernels is ~4 % slower with everything live, and a pass lasts as long as its
        // fullest component group: use it only when EVERY group has at least two dead tiles
        int fullest = 0;
        livemask = sc.live_tiles(&fullest);
        if (fullest > 6) livemask = ~0ull;
    }
    hipEvent_t* ev = nullptr;                       // (a0, a1, b0, b1) of a timed iteration
    if (b.time_stride > 0 && sc.it % b.time_stride == 0) {
        for (int i = 0; i < 4; ++i) b.gev.push_back(b.events.get());
        POOL_TRY(ctx, b.events);
        ev = &b.gev[b.gev.size() - 4];
        hipEventRecord(ev[0], st);
    }
    SweepLaunch w = batch_sweep(ctx, sc.nslots, b.max_k, tiers);
    if ((rc = launch_pass_a(b, n_new, livemask, ev ? ev[0] : nullptr, &w.cut))) return rc;
    if (ev) hipEventRecord(ev[1], st);
    if (w.cut.plane1) w.from = SweepLaunch::CUT_PLANES;
    else
        HIP_TRY(ctx, launch_reduce_splits(st, ctx->bat.XHt, ps.use2h ? gemm2h_splits(ps.KbA, b.plan.nsplitA, ps.nsubA) : b.plan.nsplitA,
                                          (long long)sc.KC * ctx->N_pad, (long long)sc.KC * ctx->N_pad));
    // W half-step                                             (sklearn _nmf.py:500)
    w.V = ctx->bat.Wt; w.ldv = ctx->N_pad; w.L = b.N; w.P = ctx->bat.XHt; w.gram = ctx->bat.gramH; w.l1 = b.l1W;
    w.chunks = b.chunksW; w.parts = b.partsW; w.want_gram = 1;
    if (ps.use2h) w.rmax_part = ctx->bat.rmaxW;
    const PlaneOut wplanes{(unsigned short*)ctx->bat.Wt3, b.shW[b.shgen], ps.KbB, G3_MW};
    if (b.fuseW && ps.use2h) w.planes = &wplanes;
    HIP_TRY(ctx, launch_sweep(st, w));
    if ((rc = launch_w_finalize(b))) return rc;
    if (ev) hipEventRecord(ev[2], st);
    int nsB = 1;
    if ((rc = launch_pass_b(b, livemask, &nsB))) return rc;
    if (ev) hipEventRecord(ev[3], st);
    if ((rc = launch_h_sweep(b, tiers, nsB))) return rc;
    if ((rc = launch_h_finalize(b))) return rc;
    sc.end_iteration();
    return CNMF_OK;
}

// ---- step 3: look at the snapshot `lag` iterations behind the GPU and retire what has converged
static int inspect(BatchRun& b)
{
    BatchSched& sc = b.sched;
    const int64_t si = sc.it - 1 - b.lag;   // snapshot index to inspect now
    if (si < 0) return CNMF_OK;
    const SlotDesc* sp = b.ctx->bat.h_snap + (size_t)(si % RING) * sc.KC0;
    const int ns = sc.snap_nslots[si % RING];
    int rc = wait_snapshot(b.ctx, sp, ns, (int)(si + 1));
    if (rc) return rc;
    for (int s = 0; s < ns; ++s)
        if (sc.retirable(s, si, sp[s].active, sp[s].restart) && (rc = retire_slot(b, s, sp[s]))) return rc;
    sc.resort_pending();
    return CNMF_OK;
}

// ---- step 4: tail compaction -- nothing left to refill with and at most half of the packed
// columns still iterate: repack the live slots into a narrower batch so the two GEMM passes
// shrink with the work (their cost is proportional to KC).
static int compact(BatchRun& b)
{
    BatchSched& sc = b.sched;
    PassScheme& ps = b.ps;
    if (!sc.in_tail()) return CNMF_OK;
    const bool part = b.ctx->knobs.part;
    const TailPlan t = sc.tail_plan(ps.use3, ps.usec, ps.use2h, part);
    int rc;
    if (t.rebalance) {
        if ((rc = repack(b, sc.KC, true))) return rc;
        sc.rebalanced();
    }
    if (t.width < sc.KC) {
        const int KC0 = sc.KC0;
        if ((rc = repack(b, t.width, t.stay3 && ps.use2h && part))) return rc;
        sc.narrowed(t.width);
        if (!t.stay3) ps.leave_matrix_pipe();
        // (the buffers were sized for KC0 columns: a narrower batch may keep more partial planes in them)
        if ((rc = plan_passes(b, (b.ctx->bat.nsplit * KC0) / sc.KC, (b.ctx->bat.nsplitA * KC0) / sc.KC))) return rc;
    }
    return CNMF_OK;
}

// where the call's results go: the resident spectra store (grown as needed) or a buffer of the call; the re-packing
// scratch on both sides
static int alloc_call_buffers(BatchRun& b, bool want_W)
{
    cnmf_ctx* ctx = b.ctx;
    const int G = b.G, n = b.n, KC0 = b.sched.KC0;
    if (b.resident) {
        if (ctx->spectra_rows && ctx->spectra_G != G) {
            SET_ERR(ctx, "the resident store holds spectra over %lld genes, this matrix has %d: cnmf_spectra_reset first",
                    (long long)ctx->spectra_G, G);
            return CNMF_ESTATE;
        }
        ctx->spectra_G = G;
        const size_t need = (ctx->spectra_rows + (size_t)b.total_k) * G;
        if (need > ctx->spectra_cap) {
            float* nb = nullptr;
            const size_t cap = std::max(need, ctx->spectra_cap * 2);
            HIP_TRY(ctx, hipMalloc(&nb, cap * sizeof(float)));
            hipError_t ce = hipSuccess;
            if (ctx->spectra_rows)
                ce = hipMemcpyAsync(nb, ctx->spectra, ctx->spectra_rows * G * sizeof(float), hipMemcpyDeviceToDevice, b.st);
            if (ce == hipSuccess) ce = hipStreamSynchronize(b.st);
            if (ce != hipSuccess) { hipFree(nb); HIP_TRY(ctx, ce); }
            hipFree(ctx->spectra);
            ctx->spectra = nb; ctx->spectra_cap = cap;
        }
        b.d_Hres = ctx->spectra + ctx->spectra_rows * G;
    } else {
        b.d_Hres = b.pool.get<float>(b.hoff[n]);
    }
    if (want_W) b.d_Wres = b.pool.get<float>(b.woff[n]);
    b.d_repack = b.pool.get<int>((size_t)3 * KC0);
    POOL_TRY(ctx, b.pool);
    HIP_TRY(ctx, hipHostMalloc(&b.repack_host.p, (size_t)RING * 3 * KC0 * sizeof(int)));
    return CNMF_OK;
}

// init_mode 1: sklearn's init='random' for EVERY restart of the call, generated up front on the
// device (one workgroup per restart) into a component-major store; install = row copy.
static int generate_inits(BatchRun& b, const uint32_t* seeds)
{
    cnmf_ctx* ctx = b.ctx;
    const int n = b.n, N = b.N, G = b.G;
    b.d_H0 = b.pool.get<float>(b.hoff[n]);
    b.d_Wt0 = b.pool.get<float>(b.woff[n]);
    RngJob* d_jobs = b.pool.get<RngJob>((size_t)n);
    POOL_TRY(ctx, b.pool);
    std::vector<RngJob> jobs(n);
    int rowoff = 0;
    for (int r = 0; r < n; ++r) {
        jobs[r] = RngJob{seeds[r], b.kk[r], rowoff, b.avg[r], (long long)b.kk[r] * ((long long)G + N)};
        rowoff += b.kk[r];
    }
    HIP_TRY(ctx, hipMemcpy(d_jobs, jobs.data(), (size_t)n * sizeof(RngJob), hipMemcpyHostToDevice));
    rng_kernel<1><<<n, 256, 0, b.st>>>(d_jobs, nullptr, b.d_H0, G, G, b.d_Wt0, N, N);
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// init_mode 2: the init store must hold exactly the restarts of the call, on this matrix
static int check_init_store(cnmf_ctx* ctx, int n, const int32_t* kk)
{
    const cnmf_ctx::InitStore& is = ctx->inits;
    if (is.k.empty()) { SET_ERR(ctx, "init_mode 2: the init store is empty"); return CNMF_EINVAL; }
    if (is.N != ctx->N || is.G != ctx->G) { SET_ERR(ctx, "init_mode 2: the init store belongs to another matrix shape"); return CNMF_EINVAL; }
    if ((int)is.k.size() != n) { SET_ERR(ctx, "init_mode 2: the init store holds %d restarts, the call has %d", (int)is.k.size(), n); return CNMF_EINVAL; }
    for (int r = 0; r < n; ++r)
        if (is.k[r] != kk[r]) { SET_ERR(ctx, "init_mode 2: restart %d has rank %d in the init store, %d in the call", r, is.k[r], (int)kk[r]); return CNMF_EINVAL; }
    return CNMF_OK;
}

// Packed columns of the call: pick_kc on the job's total rank, wide where the matrix-pipe kernels can run it
static int pick_batch_width(cnmf_ctx* ctx, const cnmf_cd_params* prm, int64_t total_k, int max_k, int* KC_out)
{
    const CdKnobs& kn = ctx->knobs;
    // (wide batches need the whole-tile matrix-pipe kernels and a matrix large enough to be worth them)
    const bool wide_can = kn.gemm3 != 0 && gemm3_enabled(ctx, 512);
    // round 6: a SMALL matrix (BASELINE config 2: 2 700 x 2 000) is launch-latency-bound -- an iteration costs its six
    // launches whatever the width -- so a job of >= 512 columns also runs wide there (C2: 1 000 columns in one batch instead
    // of four 256-column rounds, 17 -> 8 ms per job); CNMF_WIDE_SMALL=0: the round-5 rule (A/B)
    const bool wide_small = total_k >= 512 && kn.wide_small;
    const bool wide_auto = wide_can && ((int64_t)ctx->N_pad * ctx->G_pad >= (1ll << 24) || wide_small);
    int KC = pick_kc(kn.kc, kn.kc_limit, total_k, max_k, prm->kc_max, (prm->kc_max > 256 || kn.kc_set) ? wide_can : wide_auto);
    // 65..128 columns of a count-structured matrix: the 256-column integer-plane kernels (half empty) are still
    // faster than 128 columns on the f32 pipe
    if (KC == 128 && prm->kc_max <= 0 && !kn.kc_set && kn.gemm3 >= 3 && gemm3_enabled(ctx, 256) &&
        (int64_t)ctx->N_pad * ctx->G_pad >= (1ll << 24)) {
        int rc = ensure_counts(ctx);
        if (rc) return rc;
        if (ctx->counts.state == 1) KC = 256;
    }
    *KC_out = KC;
    return CNMF_OK;
}

// the end of a call: results to the host, what the call learned about its ranks, the statistics
static int finish_batch(BatchRun& b, float* H_out, float* W_out, cnmf_batch_stats* stats)
{
    cnmf_ctx* ctx = b.ctx;
    const BatchSched& sc = b.sched;
    if (sc.dbg) sc.print_debug();
    HIP_TRY(ctx, hipEventRecord(b.ev_end, b.st));
    if (!b.resident)
        HIP_TRY(ctx, hipMemcpyAsync(H_out, b.d_Hres, b.hoff[b.n] * sizeof(float), hipMemcpyDeviceToHost, b.st));
    if (W_out)
        HIP_TRY(ctx, hipMemcpyAsync(W_out, b.d_Wres, b.woff[b.n] * sizeof(float), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(ctx, hipStreamSynchronize(b.st));
    if (b.resident) ctx->spectra_rows += (size_t)b.total_k;
    // the mean iteration count per rank this call saw (cnmf_get_iteration_means)
    if (ctx->iter_prior.size() != (size_t)KMAX + 1) ctx->iter_prior.assign((size_t)KMAX + 1, 0.0);
    for (int k = 1; k <= KMAX; ++k)
        if (sc.k_done[k]) ctx->iter_prior[k] = (double)sc.k_iters[k] / (double)sc.k_done[k];
    if (!stats) return CNMF_OK;
    float ms = 0.f;
    hipEventElapsedTime(&ms, b.ev_begin, b.ev_end);
    stats->gpu_ms = ms;
    stats->outer_iterations = sc.it;
    stats->restart_iterations = sc.restart_iters;
    stats->column_iterations = sc.column_iters;
    stats->restart_column_iterations = sc.restart_col_iters;
    stats->kc = sc.KC0; stats->nsplit = b.ps.mode ? b.nsplit3_first : ctx->bat.nsplit;
    stats->gemm_mode = b.ps.mode;
    stats->tail_iterations = sc.tail_its; stats->tail_live_columns = sc.tail_live;
    if (b.ev_tail) { float tms = 0.f; hipEventElapsedTime(&tms, b.ev_tail, b.ev_end); stats->tail_ms = tms; }
    for (size_t i = 0; i + 3 < b.gev.size(); i += 4) {
        float a = 0.f, c = 0.f;
        hipEventElapsedTime(&a, b.gev[i], b.gev[i + 1]);
        hipEventElapsedTime(&c, b.gev[i + 2], b.gev[i + 3]);
        stats->passA_ms += a; stats->passB_ms += c;
        stats->passA_launches++; stats->passB_launches++;
    }
    return CNMF_OK;
}

static int run_batch(cnmf_ctx* ctx, int n, const int32_t* kk, int init_mode, const uint32_t* seeds,
                     const double* avg, const float* W0, const float* H0, const cnmf_cd_params* prm,
                     float* H_out, float* W_out, bool resident, int32_t* n_iter_out,
                     double* viol_out, cnmf_batch_stats* stats)
{
    if (!ctx) { SET_ERR(ctx, "ctx is NULL"); return CNMF_EINVAL; }
    if (int rcd_ = ensure_dense(ctx)) return rcd_;
    const CdKnobs& kn = ctx->knobs;
    int rc = validate_params(ctx, prm);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !kk)) { SET_ERR(ctx, "bad restart list"); return CNMF_EINVAL; }
    if (init_mode == 0 && n > 0 && (!W0 || !H0)) { SET_ERR(ctx, "init_mode 0 needs W0 and H0"); return CNMF_EINVAL; }
    if (init_mode == 1 && n > 0 && (!seeds || !avg)) { SET_ERR(ctx, "init_mode 1 needs seeds and avg"); return CNMF_EINVAL; }
    if (init_mode < 0 || init_mode > 2) { SET_ERR(ctx, "unknown init_mode %d", init_mode); return CNMF_EINVAL; }
    if (init_mode == 2 && n > 0 && (rc = check_init_store(ctx, n, kk))) return rc;
    if (!resident && n > 0 && !H_out) { SET_ERR(ctx, "H_out is NULL"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return CNMF_OK;

    const int N = (int)ctx->N, G = (int)ctx->G;
    int64_t total_k = 0; int max_k = 0, min_k = 1 << 30;
    std::vector<size_t> hoff(n + 1, 0), woff(n + 1, 0);
    for (int r = 0; r < n; ++r) {
        if (kk[r] < 1) { SET_ERR(ctx, "n_components must be >= 1 (restart %d)", r); return CNMF_EINVAL; }
        if (kk[r] > KMAX) { SET_ERR(ctx, "n_components=%d > CNMF_KMAX=%d is not supported by the device sweep", kk[r], KMAX); return CNMF_EUNSUPPORTED; }
        total_k += kk[r]; max_k = std::max(max_k, (int)kk[r]); min_k = std::min(min_k, (int)kk[r]);
        hoff[r + 1] = hoff[r] + (size_t)kk[r] * G;
        woff[r + 1] = woff[r] + (size_t)kk[r] * N;
    }
    int KC = 0;
    if ((rc = pick_batch_width(ctx, prm, total_k, max_k, &KC))) return rc;
    if ((rc = ensure_batch(ctx, KC, max_k, min_k))) return rc;
    if ((rc = ensure_stage(ctx, (size_t)N * KMAX, (size_t)G * KMAX))) return rc;

    BatchRun b(n, kk, KC, ctx->iter_hint.size() == (size_t)KMAX + 1 ? ctx->iter_hint.data() : nullptr, kn.debug);
    b.ctx = ctx; b.prm = prm; b.st = ctx->stream;
    b.init_mode = init_mode; b.avg = avg; b.W0 = W0; b.H0 = H0;
    b.n_iter_out = n_iter_out; b.viol_out = viol_out; b.resident = resident;
    b.N = N; b.G = G; b.max_k = max_k; b.total_k = total_k;
    b.hoff.swap(hoff); b.woff.swap(woff);
    if ((rc = pick_scheme(ctx, KC, &b.ps))) return rc;
    b.fuseW = b.ps.use2h && max_k <= KSMALL && ctx->bat.shiftW != nullptr;
    b.shW[0] = ctx->bat.shiftW; b.shW[1] = ctx->bat.shiftW ? ctx->bat.shiftW + ctx->bat.kc : nullptr;
    if (b.fuseW) HIP_TRY(ctx, hipMemsetAsync(ctx->bat.shiftW, 0, (size_t)3 * ctx->bat.kc * sizeof(int), b.st));
    b.fin_y = (max_k * max_k + 255) / 256;
    b.lag = std::max(1, std::min(RING - 2, prm->lag > 0 ? prm->lag : (kn.lag > 0 ? kn.lag : 2)));
    b.chunksW = sweep_chunks(ctx, N); b.partsW = sweep_parts(ctx, N);
    b.chunksH = sweep_chunks(ctx, G); b.partsH = sweep_parts(ctx, G);
    b.l1W = (float)prm->l1_reg_W; b.l2W = (float)prm->l2_reg_W;
    b.l1H = (float)prm->l1_reg_H; b.l2H = (float)prm->l2_reg_H;
    b.time_stride = (stats && prm->profile > 0) ? prm->profile : 0;
    if ((rc = alloc_call_buffers(b, W_out != nullptr))) return rc;
    if (init_mode == 1 && (rc = generate_inits(b, seeds))) return rc;
    if (init_mode == 2) { b.d_H0 = ctx->inits.H; b.d_Wt0 = ctx->inits.Wt; }

    // stamps restart at 1 in every call: forget the ones a previous call left in the ring (nothing is in flight here)
    memset(ctx->bat.h_snap, 0, (size_t)ctx->bat.kc * RING * sizeof(SlotDesc));
    b.ev_begin = b.events.get(); b.ev_end = b.events.get();
    POOL_TRY(ctx, b.events);
    HIP_TRY(ctx, hipEventRecord(b.ev_begin, b.st));
    if ((rc = plan_passes(b, ctx->bat.nsplit, ctx->bat.nsplitA))) return rc;
    b.nsplit3_first = b.plan.nsplit3;

    while (true) {
        int n_new = 0;
        if ((rc = refill(b, n_new))) return rc;
        if (b.sched.finished()) break;
        if (b.sched.n_pending == 0 && !b.ev_tail && stats) {
            b.ev_tail = b.events.get();
            POOL_TRY(ctx, b.events);
            HIP_TRY(ctx, hipEventRecord(b.ev_tail, b.st));
        }
        if ((rc = iterate(b, n_new))) return rc;
        if ((rc = inspect(b))) return rc;
        if ((rc = compact(b))) return rc;
    }
    return finish_batch(b, H_out, W_out, stats);
}

// mean outer iterations per rank seen by the batch calls on the resident matrix: out[KMAX + 1], 0 = rank not seen
extern "C" int cnmf_get_iteration_means(cnmf_ctx* ctx, double* out)
{
    if (!ctx || !out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    for (int k = 0; k <= KMAX; ++k) out[k] = (ctx->iter_prior.size() == (size_t)KMAX + 1) ? ctx->iter_prior[k] : 0.0;
    return CNMF_OK;
}

// expected outer iterations per rank for the queue order of the following batch calls on this matrix (n pairs; n = 0
// clears them; a new matrix clears them too)
extern "C" int cnmf_set_iteration_hints(cnmf_ctx* ctx, int n, const int32_t* k, const double* mean_iterations)
{
    if (!ctx || n < 0 || (n > 0 && (!k || !mean_iterations))) { SET_ERR(ctx, "bad argument"); return CNMF_EINVAL; }
    ctx->iter_hint.clear();
    if (n == 0) return CNMF_OK;
    ctx->iter_hint.assign((size_t)KMAX + 1, 0.0);
    for (int i = 0; i < n; ++i) {
        if (k[i] < 1 || k[i] > KMAX || !(mean_iterations[i] >= 0)) { ctx->iter_hint.clear(); SET_ERR(ctx, "bad hint %d", i); return CNMF_EINVAL; }
        ctx->iter_hint[k[i]] = mean_iterations[i];
    }
    return CNMF_OK;
}

extern "C" int cnmf_nmf_cd_batch(cnmf_ctx* ctx, int n, const int32_t* k, int init_mode,
                                 const uint32_t* seeds, const double* avg, const float* W0,
                                 const float* H0, const cnmf_cd_params* prm, float* H_out,
                                 float* W_out, int32_t* n_iter_out, double* viol_out,
                                 cnmf_batch_stats* stats)
{
    return run_batch(ctx, n, k, init_mode, seeds, avg, W0, H0, prm, H_out, W_out, false, n_iter_out, viol_out, stats);
}

extern "C" int cnmf_nmf_cd_batch_resident(cnmf_ctx* ctx, int n, const int32_t* k, int init_mode,
                                          const uint32_t* seeds, const double* avg, const float* W0,
                                          const float* H0, const cnmf_cd_params* prm,
                                          int32_t* n_iter_out, double* viol_out,
                                          cnmf_batch_stats* stats)
{
    return run_batch(ctx, n, k, init_mode, seeds, avg, W0, H0, prm, nullptr, nullptr, true, n_iter_out, viol_out, stats);
}

// ------------------------------------------------------------------ NNLS refit
extern "C" int cnmf_nnls(cnmf_ctx* ctx, int k, const float* Hin, const cnmf_cd_params* prm,
                         float* W_out, int32_t* n_iter_out, double* viol_out)
{
    if (!ctx) { SET_ERR(ctx, "ctx is NULL"); return CNMF_EINVAL; }
    if (int rcd_ = ensure_dense(ctx)) return rcd_;
    int rc = validate_params(ctx, prm);
    if (rc) return rc;
    if (!Hin || !W_out || k < 1) { SET_ERR(ctx, "bad argument"); return CNMF_EINVAL; }
    if (k > KMAX) { SET_ERR(ctx, "n_components=%d > CNMF_KMAX=%d", k, KMAX); return CNMF_EUNSUPPORTED; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int N = (int)ctx->N, G = (int)ctx->G;
    const int KC = k <= 32 ? 32 : (k <= 64 ? 64 : 128);
    rc = ensure_batch(ctx, KC, k, k);
    if (rc) return rc;
    rc = ensure_stage(ctx, (size_t)N * KMAX, (size_t)G * KMAX);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->stageH, Hin, (size_t)k * G * sizeof(float), hipMemcpyHostToDevice, st));
    dim3 gI((std::max(N, G) + 255) / 256, k);
    install_kernel<<<gI, 256, 0, st>>>(ctx->stageH, nullptr, ctx->bat.H, ctx->G_pad, G, ctx->bat.Wt, ctx->N_pad, N, 0, k);
    if (k < KC) {   // unused component rows of the 32-wide tile must be zero
        dim3 gc((ctx->G_pad + 255) / 256, KC - k), gw((ctx->N_pad + 255) / 256, KC - k);
        clear_rows_kernel<<<gc, 256, 0, st>>>(ctx->bat.H, ctx->G_pad, ctx->G_pad, k, KC - k);
        clear_rows_kernel<<<gw, 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, ctx->N_pad, k, KC - k);
    }
    SlotDesc* d = &ctx->bat.h_slots[0];
    memset(d, 0, sizeof *d);
    d->off = 0; d->k = k; d->active = 1; d->restart = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.d_slots, d, sizeof(SlotDesc), hipMemcpyHostToDevice, st));
    ctx->bat.h_slot_list[0] = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bat.d_slot_list, ctx->bat.h_slot_list, sizeof(int), hipMemcpyHostToDevice, st));
    gram_rows_kernel<<<1, 256, 0, st>>>(ctx->bat.H, ctx->G_pad, G, ctx->bat.d_slots, ctx->bat.d_slot_list, ctx->bat.gramH, (float)prm->l2_reg_W);
    HIP_TRY(ctx, launch_gemm<false>(st, 0, ctx->bat.H, ctx->G_pad, ctx->X, ctx->G_pad, ctx->bat.XHt, ctx->N_pad, 0, KC, ctx->G_pad, ctx->N_pad, 1));
    SweepLaunch sw = batch_sweep(ctx, 1, k, k <= 16 ? 1 : (k <= 32 ? 2 : (k <= KSMALL ? 4 : 8)));
    sw.V = ctx->bat.Wt; sw.ldv = ctx->N_pad; sw.L = N; sw.P = ctx->bat.XHt; sw.gram = ctx->bat.gramH; sw.l1 = (float)prm->l1_reg_W;
    sw.chunks = sweep_chunks(ctx, N); sw.parts = sweep_parts(ctx, N);
    DevPool pool;
    EventPool events;
    hipEvent_t ev = events.get(hipEventDisableTiming);
    float* d_W = pool.get<float>((size_t)N * k);
    POOL_TRY(ctx, events);
    POOL_TRY(ctx, pool);
    const int burst = 8;        // sweeps enqueued between two looks at the slot state
    int done = 0;
    SlotDesc* snap = ctx->bat.h_snap;
    for (int it = 0; it < prm->max_iter && !done; it += burst) {
        for (int b = 0; b < burst; ++b) {
            HIP_TRY(ctx, launch_sweep(st, sw));
            finalize_kernel<<<dim3(1, 1), 256, 0, st>>>(ctx->bat.gram_part, ctx->bat.viol_part, sw.parts, ctx->bat.gramW, 0.f,
                                               ctx->bat.d_slots, 2, prm->tol, prm->max_iter, 0, k);
        }
        HIP_TRY(ctx, hipMemcpyAsync(snap, ctx->bat.d_slots, sizeof(SlotDesc), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(ev, st));
        HIP_TRY(ctx, hipEventSynchronize(ev));
        done = (snap->active == 0);
    }
    dim3 gW((N + 255) / 256, k);
    extract_kernel<<<gW, 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, N, 0, k, d_W, 1);
    HIP_TRY(ctx, hipMemcpyAsync(W_out, d_W, (size_t)N * k * sizeof(float), hipMemcpyDeviceToHost, st));
    dim3 gH((ctx->G_pad + 255) / 256, k), gWc((ctx->N_pad + 255) / 256, k);
    clear_rows_kernel<<<gH, 256, 0, st>>>(ctx->bat.H, ctx->G_pad, ctx->G_pad, 0, k);
    clear_rows_kernel<<<gWc, 256, 0, st>>>(ctx->bat.Wt, ctx->N_pad, ctx->N_pad, 0, k);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_iter_out) *n_iter_out = snap->iter;
    if (viol_out) *viol_out = snap->viol_last;
    return CNMF_OK;
}
