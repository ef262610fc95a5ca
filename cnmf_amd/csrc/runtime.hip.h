// Context, error plumbing and scope-bound device resources of libcnmf_hip (included by cnmf_hip.hip).
#pragma once

#include <map>
static thread_local std::string g_last_error;

struct cnmf_comm;

// Workspace of the consensus entry points, kept by the context between calls: blocks are handed out by a bump
// pointer and stay allocated (the ~30 hipMalloc / hipFree pairs of one consensus call cost more than its kernels),
// released when the context is destroyed or when a call left more than `keep_limit` bytes behind.
struct Arena {
    struct Block { char* p; size_t cap, used; };
    std::vector<Block> blocks;
    hipError_t err = hipSuccess;
    static constexpr size_t keep_limit = (size_t)2 << 30;      // (the R x R distance matrix of a large consensus is given back)
    void reset() { err = hipSuccess; for (Block& b : blocks) b.used = 0; }
    size_t total() const { size_t t = 0; for (const Block& b : blocks) t += b.cap; return t; }
    void release() { for (Block& b : blocks) hipFree(b.p); blocks.clear(); }
    template <typename T> T* get(size_t n, bool zero = false, hipStream_t st = nullptr) {
        const size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
        Block* hit = nullptr;
        for (Block& b : blocks) if (b.cap - b.used >= bytes) { hit = &b; break; }
        if (!hit) {
            void* p = nullptr;
            const size_t cap = std::max(bytes, (size_t)16 << 20);
            hipError_t e = hipMalloc(&p, cap);
            if (e != hipSuccess) { err = e; return nullptr; }
            blocks.push_back(Block{(char*)p, cap, 0});
            hit = &blocks.back();
        }
        T* out = (T*)(hit->p + hit->used);
        hit->used += bytes;
        if (zero) hipMemsetAsync(out, 0, bytes, st);
        return out;
    }
};

// An owning group of device arrays.  F is a plain struct of device pointers (and what describes them) with a free_all().
// Not copyable, and no destructor: like Arena a group is released explicitly, by an owner that has
// synchronised the stream that may still use the arrays.
template <typename F>
struct Owned : F {
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    void release() { this->free_all(); static_cast<F&>(*this) = F{}; }
    // the commit step: this group becomes s (what it held is released), s is left empty
    void take(Owned& s) { release(); static_cast<F&>(*this) = s; static_cast<F&>(s) = F{}; }
};
// A group under construction, local to one call: released on EVERY return path (the HIP_TRY early returns included;
// hipFree waits for work that still uses the arrays, as for DevPool) unless an owner took it -- the one place where its
// arrays are cleaned up after a failure.  Whoever builds an image fills a local and commits it with take() after the
// final stream synchronisation succeeded: a failed build leaves the owner as it was, never with half an image.
template <typename F>
struct OwnedLocal : Owned<F> {
    ~OwnedLocal() { this->release(); }
};

// A rows x cols compressed-row matrix on the device: 64-bit row pointers, values of type V (float: the resident matrix,
// double: the staging paths).  nnz = -1: empty.
template <typename V>
struct CsrF {
    int64_t rows = 0, cols = 0, nnz = -1;
    long long* ptr = nullptr; int* idx = nullptr; V* val = nullptr;
    void free_all() { hipFree(ptr); hipFree(idx); hipFree(val); }
    hipError_t alloc_ptr(int64_t r, int64_t c) {
        rows = r; cols = c;
        return hipMalloc((void**)&ptr, ((size_t)r + 1) * sizeof(long long));
    }
    hipError_t alloc_entries(long long n) {           // (an array without entries still gets one element)
        const size_t n1 = (size_t)std::max<long long>(n, 1);
        hipError_t e = hipMalloc((void**)&idx, n1 * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&val, n1 * sizeof(V));
        if (e == hipSuccess) nnz = n;
        return e;
    }
};
template <typename V> using DevCsr = Owned<CsrF<V>>;
template <typename V> using DevCsrLocal = OwnedLocal<CsrF<V>>;

// blocked sliced-ELL image of the non-zeros of one orientation of X (kernels_mu_sparse.hip.h); ent = NULL: none
struct SpImageF {
    int R = 0, C = 0, BS = 0, nblk = 0, nslice = 0;
    int* perm = nullptr; long long* off = nullptr; int* len = nullptr; void* ent = nullptr;
    size_t n_ent = 0;
    void free_all() { hipFree(perm); hipFree(off); hipFree(len); hipFree(ent); }
};
using SpImage = Owned<SpImageF>;
// X^T as a dense float32 image [round_up(G_pad, 128)][N_pad] (the matrix-pipe kernels of the multiplicative updates)
struct DenseTF {
    float* p = nullptr;
    void free_all() { hipFree(p); }
};

// ---- the images of the resident matrix X that the GEMM passes of the coordinate-descent batch read (gemm_host.hip.h)
// What a GEMM pass reads of X: the plane, an optional second plane with its block flags (one bit per tile row and block),
// an optional 2^-s per output column.  Both providers below hand it out for pass A (X) and pass B (X^T).
// bytes: `plane` is a count plane of one byte per element (CountU8, kernels_planes.hip.h), read by the byte form of the kernels.
struct XOperand { const unsigned char *plane, *hi; const unsigned int* flags; const float* colscale; bool bytes = false; };

// bf16 planes of X and X^T (split-operand GEMM, CNMF_GEMM3=1|2), built on first use
struct Bf16PlanesF {
    unsigned char *X3 = nullptr, *Xt3 = nullptr;
    int tr = 0;                                      // row-tile height they were built with
    void free_all() { hipFree(X3); hipFree(Xt3); }
};

// count structure X = n * d (kernels_counts.hip.h)
struct CountPlanesF {
    int state = 0;                                   // 0 = not examined, 1 = present (the planes below exist), -1 = absent
    int fmt = 0;                                     // 3 = bf16 planes (base 256), 4 = f16 planes (base 2048, swizzled slots),
                                                     // 5 = as 4, built with the byte plane allowed (CNMF_G2_U8) ...
    bool bytes = false;                              // ... and taken: no count exceeds 255, C1 / Ct1 hold one byte per element
    unsigned char *C1 = nullptr, *Ct1 = nullptr;     // integer planes of n and n^T (one plane, 256-row tiles)
    unsigned char *C1h = nullptr, *Ct1h = nullptr;   // second planes (the high digit) when some count exceeds the base, else NULL
    unsigned int *hiA = nullptr, *hiB = nullptr;     // their flags
    double* d_scale = nullptr;                       // per-gene scale d [G_pad]
    void free_all() { hipFree(C1); hipFree(Ct1); hipFree(C1h); hipFree(Ct1h); hipFree(hiA); hipFree(hiB); hipFree(d_scale); }
    XOperand passA() const { return {C1, C1h, hiA, nullptr, bytes}; }
    XOperand passB() const { return {Ct1, Ct1h, hiB, nullptr, bytes}; }
};

// any OTHER matrix on the f16 pipe (gemm_mode 5): two f16 planes of x * 2^s_row for X (rows = cells) and X^T (rows =
// genes), the per-row 2^-s, and all-ones block flags for the two-plane ("HI") instantiation of the count kernels
struct GeneralPlanesF {
    unsigned char *X2h = nullptr, *X2m = nullptr, *Xt2h = nullptr, *Xt2m = nullptr;
    float *sA = nullptr, *sB = nullptr;
    unsigned int *onesA = nullptr, *onesB = nullptr;
    void free_all() { hipFree(X2h); hipFree(X2m); hipFree(Xt2h); hipFree(Xt2m); hipFree(sA); hipFree(sB); hipFree(onesA); hipFree(onesB); }
    XOperand passA() const { return {X2h, X2m, onesA, sA}; }
    XOperand passB() const { return {Xt2h, Xt2m, onesB, sB}; }
};

// the raw cells x genes counts a stage keeps (CSR, float64 values) and their transpose (genes x cells)
struct CountStage {
    DevCsr<double> counts, columns;
    bool staged() const { return counts.nnz >= 0; }
    void release_counts() { counts.release(); columns.release(); }
};

// staging of the cnmf_prepare_* entry points (prepare_host.hip.h): the counts (their transpose is built on first use)
// and the float64 result of cnmf_prepare_select until it is fetched: `out` (cells x selected genes; out.nnz = -1: no
// selection to fetch) and, for a densified selection, its dense image `odense` beside it
struct PrepStage : CountStage {
    DevCsr<double> out;
    double* odense = nullptr;
    int out_dense = 0;
    void release_out() { out.release(); hipFree(odense); odense = nullptr; }
    void release() { release_counts(); release_out(); }
};

// staging of the cnmf_preprocess_* entry points (preprocess_host.hip.h), apart from both the resident matrix and the
// prepare staging: the counts and their transpose, two result slots (cells x selected genes, CSR or dense float64) and
// the ridge factors R^T / Phi^T of the last moments pass
struct PreSlot {
    int64_t n = 0;                                   // columns
    DevCsr<double> csr;
    double* dense = nullptr;                         // [N][n] row-major; a dense slot has no csr
    bool empty() const { return !dense && csr.nnz < 0; }
    void release() { csr.release(); hipFree(dense); dense = nullptr; n = 0; }
};

struct PreStage : CountStage {
    int64_t N = 0;                                   // cells of the staged counts and of the slots
    PreSlot slot[2];
    double *Rt = nullptr, *Pt = nullptr;             // [N][K], [N][B1]
    int K = 0, B1 = 0;
    void release_ridge() { hipFree(Rt); hipFree(Pt); Rt = Pt = nullptr; K = B1 = 0; }
    // the batch-grouped transpose of the counts (hvg_batch_host.hip.h), cached for the batch codes it was built for:
    // genes x cells with the cells in the stable order of their batch code, so that column g lists the entries of
    // batch b as one run of rows [gstart[b], gstart[b + 1]); gB = 0: none.  It speaks of the staged cells and genes,
    // so whatever replaces or restricts the staging goes through release() and drops it
    DevCsr<double> grouped;
    int* gstart = nullptr;                           // [gB + 1] (device)
    std::vector<int32_t> gcodes;                     // [N] (host): the codes the cache answers to
    int gB = 0;
    void release_grouped() { grouped.release(); hipFree(gstart); gstart = nullptr; gcodes.clear(); gB = 0; }
    // the last Householder tridiagonalisation (pca_host.hip.h): the working matrix and the reflector store [tri_n][tri_n],
    // tau [tri_n] and, for the scatter of a slot (tri_slot; -1: a host-supplied matrix), that slot's column means;
    // replaced by the next tridiagonalisation; triR = NULL: none
    double *triA = nullptr, *triR = nullptr, *tri_tau = nullptr, *tri_mu = nullptr;
    double *tri_d = nullptr, *tri_e = nullptr;       // the tridiagonal form itself [tri_n] (tridiag_eig_host.hip.h reads it)
    int tri_n = 0, tri_slot = -1;
    void release_tridiag() {
        hipFree(triA); hipFree(triR); hipFree(tri_tau); hipFree(tri_mu); hipFree(tri_d); hipFree(tri_e);
        triA = triR = tri_tau = tri_mu = tri_d = tri_e = nullptr; tri_n = 0; tri_slot = -1;
    }
    void release() {
        release_counts(); release_ridge(); release_grouped(); release_tridiag();
        slot[0].release(); slot[1].release(); N = 0;
    }
};

// state of the cnmf_harmony_* entry points (harmony_host.hip.h): Harmony's soft clustering of N cells over d components
// into K clusters.  Cell-indexed arrays are component- or cluster-major with rows of N_pad (a multiple of 64) doubles.
struct HarStage {
    int N = 0, Np = 0, d = 0, K = 0, V = 0, B = 0;       // V variables with B levels in all; N = 0: nothing begun
    bool ready = false;                                  // cnmf_harmony_init has run
    double *Zo = nullptr, *Zcos = nullptr, *Zcorr = nullptr;          // [d][Np]
    double *R = nullptr, *dist = nullptr, *S = nullptr;              // [K][Np]
    double *ZoT = nullptr, *ZcT = nullptr, *Rt = nullptr, *Pt = nullptr;   // [N][d], [N][d], [N][K], [N][B + 1] (the ridge step)
    double *Y = nullptr, *theta = nullptr, *sigma = nullptr, *prb = nullptr;   // [d][K], [B], [K], [B]
    double *E = nullptr, *O = nullptr, *tab = nullptr, *obj = nullptr;     // [K][B] x 3, [3]
    double *ypart = nullptr, *opart = nullptr, *part_old = nullptr, *part_new = nullptr;
    size_t part_old_cap = 0, part_new_cap = 0;           // doubles
    int *codes = nullptr, *lvar = nullptr, *perm = nullptr;               // [V][Np] level of every cell, [B] variable of a level, [N]
    void release() {
        void* all[] = {Zo, Zcos, Zcorr, R, dist, S, ZoT, ZcT, Rt, Pt, Y, theta, sigma, prb, E, O, tab, obj, ypart, opart,
                       part_old, part_new, codes, lvar, perm};
        for (void* p : all) hipFree(p);
        *this = HarStage{};
    }
};

// The buffers of the coordinate-descent batch and of the NNLS refits, sized for kc packed columns (ensure_batch,
// batch_host.hip.h); kc = 0: none.  Device memory but for the three pinned host blocks.
struct BatchBuffersF {
    int kc = 0, nsplit = 0, nsplitA = 0, parts = 0;
    size_t gram_part_floats = 0;
    float *H = nullptr, *Wt = nullptr, *XHt = nullptr, *XHt1 = nullptr, *XHt2 = nullptr, *XtW = nullptr;
    unsigned char *H3 = nullptr, *Wt3 = nullptr;   // planes of the packed factors, refreshed every iteration
    unsigned char* d_split = nullptr;   // stream-K cut flags of the current plan
    // f16 two-plane factor split (kernels_gemm2h.hip.h): per-row maxima reported by the sweeps, 2^-s per row
    float *rmaxH = nullptr, *rmaxW = nullptr, *iscaleH = nullptr, *iscaleW = nullptr;
    int* shiftW = nullptr;              // [3][kc]: exponents of the W planes written by the sweep (two generations + scratch)
    float *gramH = nullptr, *gramW = nullptr, *gram_part = nullptr;
    double* viol_part = nullptr;
    SlotDesc* d_slots = nullptr;
    int* d_slot_list = nullptr;
    SlotDesc* h_slots = nullptr;      // pinned: per-slot install descriptors
    SlotDesc* h_snap = nullptr;       // pinned: snapshot ring [RING][kc]
    int* h_slot_list = nullptr;       // pinned ring of new-slot lists
    void free_all() {
        void* dev[] = {H, Wt, XHt, XHt1, XHt2, XtW, H3, Wt3, d_split, rmaxH, rmaxW, iscaleH, iscaleW, shiftW, gramH, gramW,
                       gram_part, viol_part, d_slots, d_slot_list};
        for (void* p : dev) hipFree(p);
        if (h_slots) hipHostFree(h_slots);
        if (h_snap) hipHostFree(h_snap);
        if (h_slot_list) hipHostFree(h_slot_list);
    }
};

static constexpr int RING = 8;
#ifndef CNMF_GEMM3_DEFAULT
#define CNMF_GEMM3_DEFAULT 4
#endif

// The CNMF_* switches of the coordinate-descent batch path (batch_host.hip.h, gemm_host.hip.h): parsed in ONE place,
// parse_cd_knobs below, whenever the context's snapshot of the environment is taken.  The host code reads these fields.
struct CdKnobs {
    int  gemm3 = CNMF_GEMM3_DEFAULT;   // CNMF_GEMM3=0..4: operand scheme of the GEMM passes at >= 256 packed columns (gemm_host.hip.h)
    int  g2_gvar = 4;                  // CNMF_G2_GVAR=0: general matrices on the burst-issue loop, not the spread stream (same bits)
    bool g2_gen4 = false;              // CNMF_G2_GEN4: general matrices multiply all four f16 plane pairs instead of three
    int  g2_nsub = 2;                  // CNMF_G2_NSUB=1|2: 16-k sub-blocks per barrier pair of the one-plane f16 GEMMs
    int  g2_xmap = -1;                 // CNMF_G2_XMAP=0|1: XCD mapping of the persistent f16 GEMM workgroups (-1: by path)
    bool g2_u8 = true;                 // CNMF_G2_U8=0: the f16 count plane even where every count fits a byte (same bits)
    bool part = false;                 // CNMF_PART: the tail's GEMM passes skip 32-column tiles without a live restart
    bool no_psum = false;              // CNMF_NO_PSUM: a separate split-K reduce in front of the H sweep
    bool wide_small = true;            // CNMF_WIDE_SMALL=0: a small matrix never runs wider than 256 columns
    bool kc_set = false;               // CNMF_KC is set ...
    int  kc = 0;                       // ... and from 32 up it is the batch width (a bound like cnmf_cd_params.kc_max)
    int  kc_limit = 1024;              // CNMF_KC_LIMIT: widest batch, a multiple of 256 in [256, 2048] (the 64 tile bits of the live mask)
    int  lag = 0;                      // CNMF_LAG: iterations between the device and the snapshot the host inspects (0: the caller's, or 2)
    int  sweep_parts = 64;             // CNMF_SWEEP_PARTS >= 1: most workgroups (partials) per slot of a half-step
    int  wg_slots = 0;                 // CNMF_WG_SLOTS >= 32: persistent GEMM workgroups, leaving CUs to another stream (0: one per CU)
    bool no_streamk = false;           // CNMF_NO_STREAMK: pass A always as K splits + reduce
    bool s_mtw2 = false;               // CNMF_S_MTW2: the "S" f32 GEMM layout with two tiles per wave (diagnostic entry point only)
    bool no_counts = false;            // CNMF_NO_COUNTS: no count-structure detection
    bool debug = false;                // CNMF_DEBUG: scheduler statistics of the batch path on stderr (consensus reads the snapshot itself)
};
// ... and those of the multiplicative-update solver (mu_host.hip.h): parse_mu_knobs
struct MuKnobs {
    bool valu = false;                 // CNMF_MU_VALU=1: the vector-ALU kernels, one restart at a time (kernels_mu.hip.h)
    int  sparse = -1;                  // CNMF_MU_SPARSE=0: never the non-zero path, =1: always, else (-1) by density and memory
    bool sp_order = true;              // CNMF_SP_ORDER=0: the non-zero images keep every row's entries in storage order
    bool debug = false;                // CNMF_DEBUG: what mu_sparse_prepare decided, on stderr
};

struct cnmf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // the CNMF_* environment variables as they were when the context was created (cnmf_create) or last re-read
    // (cnmf_reload_env): the host paths of a call consult THIS snapshot (ctx_getenv, knobs), never the process environment
    // -- a knob that steers a numerics-affecting path cannot change between two calls on one context behind the caller's back
    std::map<std::string, std::string> env;
    CdKnobs knobs;                                 // ... and the switches of the coordinate-descent batch path, parsed from it
    MuKnobs mu_knobs;                              // ... and of the multiplicative-update solver
    int mu_rank_limit = CNMF_MU_KMAX;              // cnmf_set_mu_rank_limit(): CNMF_MU_KMAX, or CNMF_MU_KMAX_WIDE by opt-in (never from the environment)
    int mu_sparse_rank_limit = CNMF_MU_SPARSE_KMAX;  // cnmf_set_mu_sparse_rank_limit(): largest rank on the non-zero path, 32 or (opt-in) 64

    // data matrix
    int64_t N = 0, G = 0;
    int N_pad = 0, G_pad = 0;
    float* X = nullptr;
    bool count_detect = true;                      // cnmf_set_count_detection(): look for the count structure at all?
    // Everything from here to csr / csc is an image DERIVED from X, built on first use.  drop_derived_images
    // (cnmf_hip.hip) is the one function that drops them all: whoever replaces or rewrites X calls it.
    Owned<Bf16PlanesF> planes;                     // ensure_planes
    Owned<CountPlanesF> counts;                    // ensure_counts; counts.state says whether X has the structure at all
    Owned<GeneralPlanesF> x2;                      // ensure_x2planes
    Owned<DenseTF> XtF;                            // mu_ensure_xt (mu_host.hip.h)
    // Kullback-Leibler on the non-zeros (kernels_mu_sparse.hip.h): images for padded ranks 16, 32 and 64 (sp_image_index), cells x
    // genes (A) and genes x cells (B); x_nnz = -1 until the first Kullback-Leibler call counted the matrix
    static constexpr int SP_IMAGES = 3;
    static constexpr int sp_image_index(int KP) { return KP <= 16 ? 0 : (KP <= 32 ? 1 : 2); }
    SpImage spA[SP_IMAGES], spB[SP_IMAGES];
    long long x_nnz = -1;
    // compressed rows of X (cells x genes) and of X^T (genes x cells), csr_host.hip.h: kept from cnmf_set_matrix_csr or
    // built from the dense matrix on first use; 64-bit row pointers, float32 values like the dense image
    DevCsr<float> csr, csc;

    Owned<BatchBuffersF> bat;                      // ensure_batch (batch_host.hip.h); bat.kc = 0: none
    float *stageW = nullptr, *stageH = nullptr;
    size_t stageW_sz = 0, stageH_sz = 0;

    // resident spectra store (device) for the gather / consensus
    float* spectra = nullptr;
    size_t spectra_cap = 0, spectra_rows = 0;
    int64_t spectra_G = 0;             // gene count of the rows in the store (the matrix they were computed on)
    // init store (nndsvd_tail_host.hip.h): the NNDSVD start factors of the restarts of cnmf_nndsvd_group calls, appended
    // group after group in generate_inits()'s layout -- H0 [sum k][G], Wt0 [sum k][N], component-major -- for init_mode 2
    struct InitStore {
        float *H = nullptr, *Wt = nullptr;
        size_t cap_rows = 0, rows = 0;             // component rows allocated / held
        int64_t N = 0, G = 0;                      // shape of the matrix the factors belong to
        std::vector<int> k;                        // rank of every stored restart
        std::vector<float> maxW;                   // max W0 of every stored restart
        void release() { hipFree(H); hipFree(Wt); H = Wt = nullptr; cap_rows = rows = 0; N = G = 0; k.clear(); maxW.clear(); }
    } inits;
    // what the batch calls on THIS matrix learned about the restarts' length: mean outer iterations per rank (0 = nothing
    // yet; cnmf_get_iteration_means), and the caller's hints for the NEXT calls (cnmf_set_iteration_hints): with hints the
    // queue starts longest-expected-first instead of learning the order again.  Never applied implicitly: the queue order
    // decides the packed columns a restart occupies, and its float32 result moves in the last bits with them.
    std::vector<double> iter_prior, iter_hint;

    Arena cons_ws;                    // consensus workspace (consensus_host.hip.h)
    void* cons_pinned = nullptr;      // pinned host block of the consensus calls (k-means state read-backs)
    size_t cons_pinned_bytes = 0;
    double clustergram_ms[5] = {0, 0, 0, 0, 0};   // steps of the last cnmf_clustergram (linkage_host.hip.h)
    double teig_ms[5] = {0, 0, 0, 0, 0};          // steps of the last device tridiagonal solve (tridiag_eig_host.hip.h)

    cnmf_comm* comm = nullptr;        // RCCL communicator (comm_host.hip.h); NULL = single GPU

    PrepStage prep;                   // cnmf_prepare_* staging (prepare_host.hip.h), apart from the resident matrix
    PreStage pre;                     // cnmf_preprocess_* staging (preprocess_host.hip.h)
    HarStage har;                     // cnmf_harmony_* state (harmony_host.hip.h)
};

static const char* ctx_getenv(const cnmf_ctx* ctx, const char* name)
{
    if (!ctx) return getenv(name);
    auto it = ctx->env.find(name);
    return it == ctx->env.end() ? nullptr : it->second.c_str();
}
static void parse_cd_knobs(cnmf_ctx* ctx)
{
    CdKnobs k;
    auto num = [](const char* s, int dflt) { return s ? atoi(s) : dflt; };
    k.gemm3 = num(ctx_getenv(ctx, "CNMF_GEMM3"), CNMF_GEMM3_DEFAULT);
    if (k.gemm3 < 0 || k.gemm3 > 4) k.gemm3 = CNMF_GEMM3_DEFAULT;
    k.g2_gvar = num(ctx_getenv(ctx, "CNMF_G2_GVAR"), 4) == 0 ? 0 : 4;
    k.g2_gen4 = ctx_getenv(ctx, "CNMF_G2_GEN4") != nullptr;
    k.g2_nsub = num(ctx_getenv(ctx, "CNMF_G2_NSUB"), 2) == 1 ? 1 : 2;
    k.g2_xmap = num(ctx_getenv(ctx, "CNMF_G2_XMAP"), -1);
    k.g2_u8 = num(ctx_getenv(ctx, "CNMF_G2_U8"), 1) != 0;
    k.part = ctx_getenv(ctx, "CNMF_PART") != nullptr;
    k.no_psum = ctx_getenv(ctx, "CNMF_NO_PSUM") != nullptr;
    k.wide_small = num(ctx_getenv(ctx, "CNMF_WIDE_SMALL"), 1) != 0;
    k.kc_set = ctx_getenv(ctx, "CNMF_KC") != nullptr;
    k.kc = num(ctx_getenv(ctx, "CNMF_KC"), 0);
    k.kc_limit = std::max(256, std::min(2048, (num(ctx_getenv(ctx, "CNMF_KC_LIMIT"), 1024) / 256) * 256));
    k.lag = num(ctx_getenv(ctx, "CNMF_LAG"), 0);
    k.sweep_parts = std::max(1, num(ctx_getenv(ctx, "CNMF_SWEEP_PARTS"), 64));
    k.wg_slots = num(ctx_getenv(ctx, "CNMF_WG_SLOTS"), 0);
    k.no_streamk = ctx_getenv(ctx, "CNMF_NO_STREAMK") != nullptr;
    k.s_mtw2 = ctx_getenv(ctx, "CNMF_S_MTW2") != nullptr;
    k.no_counts = ctx_getenv(ctx, "CNMF_NO_COUNTS") != nullptr;
    k.debug = ctx_getenv(ctx, "CNMF_DEBUG") != nullptr;
    ctx->knobs = k;
}
static void parse_mu_knobs(cnmf_ctx* ctx)
{
    MuKnobs m;
    auto num = [](const char* s, int dflt) { return s ? atoi(s) : dflt; };
    m.valu = num(ctx_getenv(ctx, "CNMF_MU_VALU"), 0) != 0;
    const int sp = num(ctx_getenv(ctx, "CNMF_MU_SPARSE"), -1);
    m.sparse = sp == 0 || sp == 1 ? sp : -1;
    m.sp_order = num(ctx_getenv(ctx, "CNMF_SP_ORDER"), 1) != 0;
    m.debug = ctx_getenv(ctx, "CNMF_DEBUG") != nullptr;
    ctx->mu_knobs = m;
}

extern char** environ;
static void ctx_snapshot_env(cnmf_ctx* ctx)
{
    ctx->env.clear();
    for (char** e = environ; e && *e; ++e) {
        if (strncmp(*e, "CNMF_", 5) != 0) continue;
        const char* eq = strchr(*e, '=');
        if (eq) ctx->env[std::string(*e, eq - *e)] = std::string(eq + 1);
    }
    parse_cd_knobs(ctx);
    parse_mu_knobs(ctx);
}

#define SET_ERR(ctx, ...)                                                   \
    do {                                                                    \
        char buf_[512];                                                     \
        snprintf(buf_, sizeof buf_, __VA_ARGS__);                           \
        if (ctx) (ctx)->err = buf_;                                         \
        g_last_error = buf_;                                                \
    } while (0)

#define HIP_TRY(ctx, call)                                                  \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            SET_ERR(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? CNMF_ENOMEM : CNMF_EHIP;   \
        }                                                                   \
    } while (0)

// Scope-bound device allocations / events: released when the entry point returns, on EVERY path
// (the HIP_TRY early returns included; hipFree waits for work that still uses the buffer).
struct DevPool {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    template <typename T> T* get(size_t n, bool zero = false, hipStream_t st = nullptr) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) { err = e; return nullptr; }
        ptrs.push_back(p);
        if (zero) hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), st);
        return (T*)p;
    }
    // n elements holding a copy of host[0 .. n), queued on st (a failed copy is reported by POOL_TRY like a failed allocation)
    template <typename T> T* put(const T* host, size_t n, hipStream_t st) {
        T* p = get<T>(n);
        if (p && n > 0) {
            hipError_t e = hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) err = e;
        }
        return p;
    }
    ~DevPool() { for (void* p : ptrs) hipFree(p); }
};

// queues the copy of n device elements to the host array `host` on st (the caller synchronises)
template <typename T>
static inline hipError_t dev_fetch(hipStream_t st, void* host, const T* dev, size_t n)
{
    return hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st);
}

struct EventPool {
    std::vector<hipEvent_t> evs;
    hipError_t err = hipSuccess;
    hipEvent_t get(unsigned flags = hipEventDefault) {
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) { err = r; return nullptr; }
        evs.push_back(e);
        return e;
    }
    ~EventPool() { for (hipEvent_t e : evs) hipEventDestroy(e); }
};

#define POOL_TRY(ctx, pool)                                                                   \
    do {                                                                                      \
        if ((pool).err != hipSuccess) {                                                       \
            SET_ERR(ctx, "device allocation failed: %s (%s:%d)", hipGetErrorString((pool).err), __FILE__, __LINE__); \
            return ((pool).err == hipErrorOutOfMemory) ? CNMF_ENOMEM : CNMF_EHIP;             \
        }                                                                                     \
    } while (0)

// Opt a kernel into more than the default 64 KB of dynamic LDS -- once per (kernel, DEVICE): the attribute belongs to
// the device's code object, so a process that drives several GPUs (one context each) must set it on every one of them
// (a function-local `static bool` did it for the first device only).  Thread-safe; the return code is checked.
#include <mutex>
#include <set>
#include <utility>
static hipError_t dyn_lds_optin(const void* fn, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, dev})) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({fn, dev});
    return e;
}

static inline int round_up(int64_t v, int m) { return (int)(((v + m - 1) / m) * m); }
