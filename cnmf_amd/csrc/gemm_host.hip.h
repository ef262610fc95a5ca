// Host side of the GEMM / sweep kernels: launchers, stream-K plans, operand planes, count-structure
// detection (included by cnmf_hip.hip after runtime.hip.h).
#pragma once

#include "pass_plan.h"

// ------------------------------------------------------------------ GEMM dispatch
// variant : 0 = auto; 1 = "S" (waves split components, 32 j per workgroup);
//           2 = "T" (every wave owns all the workgroup's components, 128 j per workgroup)
//           3 = 2x2 wave grid (64 j per workgroup)

template <int MTW, int WM, int WN, bool NN, int TBK = BK>
static hipError_t launch_gemm_t(hipStream_t st, const float* A, int lda, const float* B, int ldb,
                                float* C, int ldc, long long cstride, int KC, int Ktot, int J,
                                int nsplit)
{
    constexpr int MW = WM * MTW * 32, JW = WN * 32;
    const int Kper = round_up((Ktot + nsplit - 1) / nsplit, BK);
    dim3 grid((J + JW - 1) / JW, KC / MW, nsplit);
    constexpr size_t lds = gemm_lds_bytes<MTW, WM, WN, NN, TBK>();
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm_kernel<MTW, WM, WN, NN, TBK>, (int)lds)) return e_;
    }
    gemm_kernel<MTW, WM, WN, NN, TBK><<<grid, 256, lds, st>>>(A, lda, B, ldb, C, ldc, cstride, Kper,
                                                             Ktot, J);
    return hipGetLastError();
}

template <bool NN>
static hipError_t launch_gemm(hipStream_t st, int variant, const float* A, int lda, const float* B,
                              int ldb, float* C, int ldc, long long cstride, int KC, int Ktot,
                              int J, int nsplit, bool s_mtw2 = false)   // s_mtw2: CNMF_S_MTW2 (the diagnostic "S" layout only)
{
#define GO(MTW, WM, WN) \
    return launch_gemm_t<MTW, WM, WN, NN>(st, A, lda, B, ldb, C, ldc, cstride, KC, Ktot, J, nsplit)
    if (variant == 0) variant = 2;
    if (variant == 1 && KC < 128) variant = (KC >= 64) ? 3 : 2;
    if (variant == 3 && KC < 64) variant = 2;
    switch (variant) {
        case 1:  // S: 4 waves x (MTW tiles of 32 comps), 32 j
            if (KC % 256 == 0 && KC >= 256 && s_mtw2) GO(2, 4, 1);
            GO(1, 4, 1);
        case 3:  // 2x2
            if (KC % 128 == 0) GO(2, 2, 2);
            GO(1, 2, 2);
        default:  // T: every wave all comps of the M group, 128 j
            if (KC % 128 == 0) GO(4, 1, 4);
            if (KC % 64 == 0) GO(2, 1, 4);
            GO(1, 1, 4);
    }
#undef GO
}

// ------------------------------------------------------------------ sweep dispatch
static constexpr CutPlanes NO_CUT{nullptr, nullptr, 1, 1, 1, nullptr};
static constexpr PlaneOut NO_PLANES{nullptr, nullptr, 0, 0};

// One half-step sweep over `nslots` slots.  The form of sweep_kernel it takes follows from the fields (sweep_form,
// pass_plan.h): where the product comes from, whether the row maxima are wanted exactly, whether planes are written.
struct SweepLaunch {
    int nslots = 0;
    float* V = nullptr; int ldv = 0, L = 0;         // the factor being solved, component-major, L valid entries per row
    const float* P = nullptr;                       // its product with X, as ...
    enum { ONE_PLANE, CUT_PLANES, SPLIT_SUM } from = ONE_PLANE;
    CutPlanes cut = NO_CUT;                         // CUT_PLANES: ... the stream-K planes to add where a tile was cut
    SplitSum sum{1, 0, nullptr};                    // SPLIT_SUM: ... split-K planes summed (and scaled) in the sweep itself
    const float* gram = nullptr;
    const SlotDesc* slots = nullptr;
    float l1 = 0.f;
    float* gram_part = nullptr; double* viol_part = nullptr;
    int chunks = 1, parts = 1;                      // a workgroup walks `chunks` 256-row tiles; `parts` workgroups (= partials) per slot
    int want_gram = 0, kmax = 0, tiers = 0;         // tiers: bit t = a live slot has a rank of tier t (8: ranks 65..128)
    float* rmax_part = nullptr;                     // row-maximum report: the bound, or with rmax_scale the exact maximum x scale
    const double* rmax_scale = nullptr;
    const PlaneOut* planes = nullptr;               // f16 planes of the result written by the sweep (ranks <= 64)
};

using SweepFn = void (*)(float*, int, int, const float*, SplitInfo, const float*, const SlotDesc*, float, float*, double*, int, int, int,
                         int, float*, const double*, PlaneOut);
static constexpr SweepFn SWEEP_KERNELS[6][3] = {    // [SweepForm][tier]
    {sweep_kernel<0>, sweep_kernel<1>, sweep_kernel<2>},
    {sweep_kernel<0, false, false, false, true>, sweep_kernel<1, false, false, false, true>, sweep_kernel<2, false, false, false, true>},
    {sweep_kernel<0, false, false, true>, sweep_kernel<1, false, false, true>, sweep_kernel<2, false, false, true>},
    {sweep_kernel<0, false, false, true, true>, sweep_kernel<1, false, false, true, true>, sweep_kernel<2, false, false, true, true>},
    {sweep_kernel<0, true>, sweep_kernel<1, true>, sweep_kernel<2, true>},
    {sweep_kernel<0, true, true>, sweep_kernel<1, true, true>, sweep_kernel<2, true, true>}};

static hipError_t launch_sweep(hipStream_t st, const SweepLaunch& s)
{
    const bool pln = s.planes != nullptr, exact = s.rmax_part && s.rmax_scale;
    const SweepForm form = sweep_form(pln, s.from == SweepLaunch::SPLIT_SUM, exact, sweep_a64(s.ldv), s.tiers);
    if (form == SweepForm::INVALID || (pln && s.planes->TR != G3_MW)) return hipErrorInvalidValue;
    SplitInfo sp;
    if (form == SweepForm::H_PSUM) sp.sum = s.sum;
    else sp.cut = s.from == SweepLaunch::CUT_PLANES ? s.cut : NO_CUT;
    const dim3 grid(s.parts, s.nslots);
    // one launch per rank tier present among the live slots; a launch skips the slots of other tiers at once
    // (ranks above 32 need more than the default 64 KB of dynamic LDS)
    for (int t = 0; t < 3; ++t) {
        if (!(s.tiers & (1 << t))) continue;
        const SweepFn fn = SWEEP_KERNELS[(int)form][t];
        if (hipError_t e_ = dyn_lds_optin((const void*)fn, (int)sweep_lds_bytes(KSMALL, pln))) return e_;
        fn<<<grid, 256, sweep_lds_bytes(s.kmax, pln), st>>>(s.V, s.ldv, s.L, s.P, sp, s.gram, s.slots, s.l1, s.gram_part, s.viol_part, s.chunks,
                                                           s.want_gram, sweep_kg(s.kmax), s.kmax, s.rmax_part, pln ? nullptr : s.rmax_scale,
                                                           pln ? *s.planes : NO_PLANES);
    }
    if (s.tiers & 8) {            // ranks 65..128: sweep_big_kernel (+ the Gram of the updated rows as its own launch)
        const size_t blds = sweep_big_lds_bytes();
        const auto big = exact ? sweep_big_kernel<true> : sweep_big_kernel<false>;
        if (hipError_t e_ = dyn_lds_optin((const void*)big, (int)blds)) return e_;
        big<<<grid, 256, blds, st>>>(s.V, s.ldv, s.L, s.P, sp, s.gram, s.slots, s.l1, s.viol_part, s.chunks, exact ? s.rmax_part : nullptr,
                                     exact ? s.rmax_scale : nullptr);
        if (s.want_gram)
            gram_big_kernel<<<grid, 256, 0, st>>>(s.V, s.ldv, s.L, s.slots, s.gram_part, s.chunks, s.kmax,
                                                  (s.rmax_part && !s.rmax_scale) ? s.rmax_part : nullptr);
    }
    return hipGetLastError();
}

// ---- stream-K pass A (T layout: 128 components x 128 cells per tile; the plan: plan_streamk, pass_plan.h)
static hipError_t launch_streamk_passA(hipStream_t st, const StreamK& sk, const float* A, int lda,
                                       const float* B, int ldb, float* C0, float* C1, int ldc, int Jtot)
{
    constexpr size_t lds = gemm_lds_bytes<4, 1, 4, false>();
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm_streamk_kernel<4, 1, 4, false>, (int)lds)) return e_;
    }
    gemm_streamk_kernel<4, 1, 4, false><<<sk.P, 256, lds, st>>>(A, lda, B, ldb, C0, C1, ldc, sk.MG, sk.T,
                                                               sk.nk, Jtot);
    return hipGetLastError();
}

static hipError_t launch_reduce_splits(hipStream_t st, float* P, int nsplit, long long split_stride,
                                       long long n_floats, const double* colscale = nullptr, int ld = 1)
{
    if (nsplit <= 1 && !colscale) return hipSuccess;
    const long long nv = n_floats / 4;
    reduce_splits_kernel<<<(unsigned)((nv + 255) / 256), 256, 0, st>>>(P, nsplit, split_stride, P, nv, colscale, ld);
    return hipGetLastError();
}


// ------------------------------------------------------------------ split-operand GEMM launchers
// planes of a K-contiguous f32 matrix, block-major with row tiles of TR rows (rows % TR == 0)
static hipError_t launch_split3(hipStream_t st, const float* src, int ld, int rows, int K, unsigned char* dst, int TR,
                                const double* kscale = nullptr)
{
    if (rows % 64 == 0 && K % 64 == 0 && TR % 64 == 0) {        // tiled through LDS: both sides coalesced
        if (rows / 64 > PLAN_GRID_YZ) return hipErrorInvalidValue;
        dim3 grid(K / 64, rows / 64);
        split3_tiled_kernel<<<grid, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale);
        return hipGetLastError();
    }
    const long long total = (long long)rows * (K / 16);
    split3_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, ld, rows, K, TR, (unsigned short*)dst, kscale);
    return hipGetLastError();
}

// CNMF_GEMM3: 0 = exact-f32 matrix pipe only, 1 = split-operand bf16 path, two register-staged 4-wave
// workgroups per CU (the simple reference variant), 2 = split-operand bf16 path, one 8-wave LDS-DMA
// ping-pong workgroup per CU; 3 (default) = 2, plus the count-structured path (one integer plane for X, 3 MFMAs
// per product on 256 x 256 tiles) whenever the resident matrix has that structure; 4 (default) = 3 on the f16 matrix
// pipe (kernels_gemm2h.hip.h): counts <= 2048 in one f16 plane, the factor as two f16 planes with a per-row exponent,
// 2 MFMAs per product.  Tests switch it between calls (cnmf_reload_env).
// (Tried and dropped, all within 3 % of variant 2 at the 50k x 2000 shape: the same ping-pong with register
//  staging; 256 x 256 tiles with the two wave groups half a block apart (2/3 of the DMA bytes per flop).)
static int gemm3_wg_slots(const CdKnobs& k) { return gemm3_wg_slots(k.gemm3, k.wg_slots); }
static int gemm3_jw() { return G3_JW; }     // j extent of a tile = row tile of the B planes

static hipError_t launch_gemm3(hipStream_t st, const unsigned char* A3, const unsigned char* B3, int Kb,
                               float* C, int ldc, long long cstride, int KC, int Jpad, int nsplit, int gemm3_mode)
{
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3_kernel, G3_LDS_BYTES)) return e_;
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3g_kernel, G3G_LDS_BYTES)) return e_;
    }
    const int kb_per = (Kb + nsplit - 1) / nsplit;
    dim3 grid(Jpad / gemm3_jw(), KC / G3_MW, (Kb + kb_per - 1) / kb_per);
    if (gemm3_mode >= 2)
        gemm3g_kernel<<<grid, 512, G3G_LDS_BYTES, st>>>(A3, B3, Kb, C, ldc, cstride, kb_per);
    else
        gemm3_kernel<<<grid, 256, G3_LDS_BYTES, st>>>(A3, B3, Kb, C, ldc, cstride, kb_per);
    return hipGetLastError();
}


// plane split of a packed factor + finalize of the sweep that produced it, in one launch (kernels_sweep.hip.h)
static hipError_t launch_split3_finalize(hipStream_t st, const float* src, int ld, int rows, int K, unsigned char* dst,
                                         int TR, const double* kscale, const FinalizeArgs& fa, int nslots, int fin_y)
{
    const int bx = K / 64, by = rows / 64;
    split3_finalize_kernel<<<bx * by + nslots * fin_y, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale, bx, by,
                                                                  fa, fin_y);
    return hipGetLastError();
}

static hipError_t launch_split2h_finalize(hipStream_t st, const float* src, int ld, int rows, int K, unsigned char* dst,
                                          int TR, const double* kscale, const float* rmax_part, int parts,
                                          float* inv_scale, const FinalizeArgs& fa, int nslots, int fin_y,
                                          SplitFused fu = SplitFused{nullptr, nullptr});

// ---- stream-K pass A of the split-operand kernels (the plan: plan_streamk3, pass_plan.h)
static hipError_t launch_gemm3_streamk(hipStream_t st, const StreamK3& sk, const unsigned char* A3,
                                       const unsigned char* B3, float* C0, float* C1, float* C2, int ldc,
                                       int gemm3_mode)
{
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3_streamk_kernel, G3_LDS_BYTES)) return e_;
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3g_streamk_kernel, G3G_LDS_BYTES)) return e_;
    }
    if (gemm3_mode >= 2)
        gemm3g_streamk_kernel<<<sk.P, 512, G3G_LDS_BYTES, st>>>(A3, B3, sk.Kb, C0, C1, C2, ldc, sk.MG, sk.T);
    else
        gemm3_streamk_kernel<<<sk.P, 256, G3_LDS_BYTES, st>>>(A3, B3, sk.Kb, C0, C1, C2, ldc, sk.MG, sk.T);
    return hipGetLastError();
}

// ---- X-side planes of the count and general paths (x_planes_kernel, kernels_planes.hip.h): the one place that knows the
// two grid shapes.  X is N x G with leading dimension ld; the planes have rows_pad rows of K k (row tiles of G3C_JW):
// transpose = false, rows = cells and k = genes, or transpose = true, rows = genes and k = cells.
//   COUNT_BF16 / COUNT_F16 : aux = the per-gene unit (float), plane1 / flags = the second plane and its block flags or nullptr
//   COUNT_U8               : aux = the per-gene unit (float), plane0 = one byte per count (every count <= 255, K % 32 == 0); no second plane
//   SPLIT_F16              : aux = the per-row exponent (int), plane0 / plane1 = the h and m planes
enum class XPlaneFormat { COUNT_BF16, COUNT_F16, SPLIT_F16, COUNT_U8 };

template <class F>
static hipError_t launch_x_planes_t(hipStream_t st, bool transpose, const float* X, int ld, int N, int G, int rows_pad, int K,
                                    const void* aux, unsigned char* plane0, unsigned char* plane1, unsigned int* flags)
{
    const auto* a = static_cast<const typename F::Aux*>(aux);
    auto* p0 = reinterpret_cast<unsigned short*>(plane0);
    auto* p1 = reinterpret_cast<unsigned short*>(plane1);
    if (transpose) {                // lanes along the output row; the 16-k blocks (the long dimension: cells) on grid.x
        const int groups = (rows_pad + 255) / 256;
        if (groups > PLAN_GRID_YZ) return hipErrorInvalidValue;
        x_planes_kernel<F, true><<<dim3(K / 16, groups), 256, 0, st>>>(X, ld, N, G, rows_pad, K, G3C_JW, a, p0, p1, flags);
    } else {                        // one thread per (row, block), flat
        const long long blocks = ((long long)rows_pad * (K / 16) + 255) / 256;
        if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
        x_planes_kernel<F, false><<<(unsigned)blocks, 256, 0, st>>>(X, ld, N, G, rows_pad, K, G3C_JW, a, p0, p1, flags);
    }
    return hipGetLastError();
}

static hipError_t launch_x_planes(hipStream_t st, XPlaneFormat fmt, bool transpose, const float* X, int ld, int N, int G,
                                  int rows_pad, int K, const void* aux, unsigned char* plane0, unsigned char* plane1,
                                  unsigned int* flags = nullptr)
{
    switch (fmt) {
        case XPlaneFormat::COUNT_BF16: return launch_x_planes_t<CountBf16>(st, transpose, X, ld, N, G, rows_pad, K, aux, plane0, plane1, flags);
        case XPlaneFormat::COUNT_F16: return launch_x_planes_t<CountF16>(st, transpose, X, ld, N, G, rows_pad, K, aux, plane0, plane1, flags);
        case XPlaneFormat::COUNT_U8:
            if (K % 32 || plane1) return hipErrorInvalidValue;
            return launch_x_planes_t<CountU8>(st, transpose, X, ld, N, G, rows_pad, K, aux, plane0, nullptr, nullptr);
        default: return launch_x_planes_t<SplitF16>(st, transpose, X, ld, N, G, rows_pad, K, aux, plane0, plane1, flags);
    }
}

// planes of X (pass A) and of X^T (pass B), built once per matrix on first use
static int ensure_planes(cnmf_ctx* ctx)
{
    const int TR = gemm3_jw();
    if (ctx->planes.X3 && ctx->planes.tr == TR) return CNMF_OK;
    ctx->planes.release();                                 // (planes of another tile height go before their successors are allocated)
    const size_t bA = (size_t)ctx->N_pad * (ctx->G_pad / 16) * G3_ROWB;
    const size_t bB = (size_t)ctx->G_pad * (ctx->N_pad / 16) * G3_ROWB;
    OwnedLocal<Bf16PlanesF> L;
    L.tr = TR;
    HIP_TRY(ctx, hipMalloc(&L.X3, bA));
    HIP_TRY(ctx, hipMalloc(&L.Xt3, bB));
    HIP_TRY(ctx, launch_split3(ctx->stream, ctx->X, ctx->G_pad, ctx->N_pad, ctx->G_pad, L.X3, TR));
    dim3 grid(ctx->N_pad / 16, (ctx->G_pad + 255) / 256);
    split3_transpose_kernel<<<grid, 256, 0, ctx->stream>>>(ctx->X, ctx->G_pad, ctx->N_pad, ctx->G_pad, ctx->N_pad,
                                                            TR, (unsigned short*)L.Xt3);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->planes.take(L);
    return CNMF_OK;
}

// planes of a general (not count-structured) matrix for the f16 pipe (gemm_mode 5, SplitF16 of kernels_planes.hip.h)
static int ensure_x2planes(cnmf_ctx* ctx)
{
    if (ctx->x2.X2h) return CNMF_OK;
    hipStream_t st = ctx->stream;
    const int N = (int)ctx->N, G = (int)ctx->G, Np = ctx->N_pad, Gp = ctx->G_pad;
    const size_t pb = (size_t)Np * Gp * 2;
    const size_t fa = (size_t)(Np / G3C_JW) * ((Gp / 16 + 31) / 32) * sizeof(unsigned), fb = (size_t)(Gp / G3C_JW) * ((Np / 16 + 31) / 32) * sizeof(unsigned);
    DevPool pool;
    int* shA = pool.get<int>(Np);
    int* shB = pool.get<int>(Gp);
    POOL_TRY(ctx, pool);
    OwnedLocal<GeneralPlanesF> L;
    HIP_TRY(ctx, hipMalloc(&L.X2h, pb));
    HIP_TRY(ctx, hipMalloc(&L.X2m, pb));
    HIP_TRY(ctx, hipMalloc(&L.Xt2h, pb));
    HIP_TRY(ctx, hipMalloc(&L.Xt2m, pb));
    HIP_TRY(ctx, hipMalloc(&L.sA, (size_t)Np * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(&L.sB, (size_t)Gp * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(&L.onesA, fa));
    HIP_TRY(ctx, hipMalloc(&L.onesB, fb));
    HIP_TRY(ctx, hipMemsetAsync(L.onesA, 0xff, fa, st));
    HIP_TRY(ctx, hipMemsetAsync(L.onesB, 0xff, fb, st));
    x2h_rowshift_kernel<<<(Np + 3) / 4, 256, 0, st>>>(ctx->X, Gp, N, G, 0, Np, shA, L.sA);
    x2h_rowshift_kernel<<<(Gp + 255) / 256, 256, 0, st>>>(ctx->X, Gp, N, G, 1, Gp, shB, L.sB);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, launch_x_planes(st, XPlaneFormat::SPLIT_F16, false, ctx->X, Gp, N, G, Np, Gp, shA, L.X2h, L.X2m));
    HIP_TRY(ctx, launch_x_planes(st, XPlaneFormat::SPLIT_F16, true, ctx->X, Gp, N, G, Gp, Np, shB, L.Xt2h, L.Xt2m));
    HIP_TRY(ctx, hipStreamSynchronize(st));                // the shift scratch is freed on return
    ctx->x2.take(L);
    return CNMF_OK;
}

// ---- count-structured data: launchers of the 256 x 256 integer-plane kernel
// Bhi / hiflag: second integer plane and its block flags (nullptr when no count exceeds 256)
static hipError_t launch_gemm3c(hipStream_t st, const unsigned char* A3, const unsigned char* B1,
                                const unsigned char* Bhi, const unsigned int* hiflag, int Kb,
                                float* C, int ldc, long long cstride, int KC, int Jpad, int nsplit)
{
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3c_kernel, g3c_lds_bytes(true))) return e_;
    }
    const int kb_per = (Kb + nsplit - 1) / nsplit;
    dim3 grid(Jpad / G3C_JW, KC / G3_MW, (Kb + kb_per - 1) / kb_per);
    gemm3c_kernel<<<grid, 512, g3c_lds_bytes(Bhi != nullptr), st>>>(A3, B1, Bhi, hiflag, Kb, C, ldc, cstride, kb_per);
    return hipGetLastError();
}

static hipError_t launch_gemm3c_streamk(hipStream_t st, const StreamK3& sk, const unsigned char* A3,
                                        const unsigned char* B1, const unsigned char* Bhi,
                                        const unsigned int* hiflag, float* C0, float* C1, float* C2, int ldc)
{
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm3c_streamk_kernel, g3c_lds_bytes(true))) return e_;
    }
    gemm3c_streamk_kernel<<<sk.P, 512, g3c_lds_bytes(Bhi != nullptr), st>>>(A3, B1, Bhi, hiflag, sk.Kb, C0, C1, C2, ldc,
                                                                            sk.MG, sk.T);
    return hipGetLastError();
}

// ---- f16 two-plane count path (kernels_gemm2h.hip.h)
// Instruction streams (the VAR parameter of kernels_gemm2h.hip.h): production launches use 4, the spread stream, and 0,
// the burst loop, on the two-plane count path; general matrices (GEN) take 0 instead of 4 with CNMF_G2_GVAR=0 (same bits).

// One GEMM pass on the f16 pipe.  Its kernel instantiation is g2_form's (pass_plan.h) from the operand, the knobs, the
// live mask and -- stream-K -- the number of component groups.
struct G2Launch {
    const unsigned char* A2 = nullptr;      // the factor's two f16 planes ...
    const float* rscale = nullptr;          // ... and its 2^-s per row
    XOperand x{};                           // X: the count plane(s), or the two planes and column scale of a general matrix
    int Kb = 0;                             // 16-k blocks of the contraction
    float* C[3] = {nullptr, nullptr, nullptr};      // output: K-split partial planes from C[0]; stream-K: the plane and its two cut planes
    int ldc = 0;
    // livemask: bit t = the 32 packed columns 32 t .. 32 t + 31 hold a restart that still iterates (all ones: everything)
    unsigned long long livemask = ~0ull;
    long long cstride = 0; int KC = 0, Jpad = 0, nsplit = 1;    // K split: `nsplit` planes `cstride` floats apart, KC x Jpad each
    const StreamK3* sk = nullptr;           // ... or stream-K: the plan, made with unit = gemm2h_nsub(x.hi != nullptr, Kb, g2_nsub)
    const CdKnobs* kn = nullptr;            // reads g2_gen4, g2_gvar, g2_nsub, g2_xmap
};
// (x.bytes: the count plane as bytes -- the U8 instantiations; what ensure_counts built decides, not a knob read here)
using G2Fn = hipError_t (*)(hipStream_t, const G2Launch&);
struct G2Entry { G2Form form; G2Fn fn; };

template <int NSUB, bool HI, int VAR = 0, bool PART = false, bool GEN = false, bool U8 = false>
static hipError_t launch_gemm2h_t(hipStream_t st, const G2Launch& g)
{
    constexpr int lds = G2Geom<NSUB, HI, U8>::LDS_BYTES;
    if (g.x.bytes != U8) return hipErrorInvalidValue;
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm2h_kernel<NSUB, HI, VAR, PART, GEN, U8>, lds)) return e_;
    }
    int kb_per = (g.Kb + g.nsplit - 1) / g.nsplit;
    kb_per = ((kb_per + NSUB - 1) / NSUB) * NSUB;            // whole steps
    dim3 grid(g.Jpad / G3C_JW, g.KC / G3_MW, (g.Kb + kb_per - 1) / kb_per);
    gemm2h_kernel<NSUB, HI, VAR, PART, GEN, U8><<<grid, 512, lds, st>>>(g.A2, g.x.plane, HI ? g.x.hi : nullptr, HI ? g.x.flags : nullptr, g.rscale,
                                                                   g.Kb, g.C[0], g.ldc, g.cstride, kb_per, g.x.colscale,
                                                                   PART ? g.livemask : ~0ull);
    return hipGetLastError();
}

template <int NSUB, bool HI, int VAR = 0, bool NTB = true, bool PART = false, bool GEN = false, bool U8 = false>
static hipError_t launch_gemm2h_streamk_t(hipStream_t st, const G2Launch& g)
{
    constexpr int lds = G2Geom<NSUB, HI, U8>::LDS_BYTES;
    if (g.x.bytes != U8) return hipErrorInvalidValue;
    {
        if (hipError_t e_ = dyn_lds_optin((const void*)gemm2h_streamk_kernel<NSUB, HI, VAR, NTB, PART, GEN, U8>, lds)) return e_;
    }
    const int xmap = g2_xmap(G2Form{true, NSUB, HI, VAR, NTB, PART, GEN, U8}, g.kn->g2_xmap);
    gemm2h_streamk_kernel<NSUB, HI, VAR, NTB, PART, GEN, U8><<<g.sk->P, 512, lds, st>>>(g.A2, g.x.plane, HI ? g.x.hi : nullptr,
                                                                                    HI ? g.x.flags : nullptr, g.rscale, g.Kb, g.C[0], g.C[1],
                                                                                    g.C[2], g.ldc, g.sk->MG, g.sk->T, xmap, g.x.colscale,
                                                                                    PART ? g.livemask : ~0ull);
    return hipGetLastError();
}

template <int NSUB, bool HI, int VAR, bool PART, bool GEN, bool U8 = false>
static constexpr G2Entry g2_ksplit() { return {G2Form{true, NSUB, HI, VAR, false, PART, GEN, U8}, launch_gemm2h_t<NSUB, HI, VAR, PART, GEN, U8>}; }
template <int NSUB, bool HI, int VAR, bool NTB, bool PART, bool GEN, bool U8 = false>
static constexpr G2Entry g2_streamk() { return {G2Form{true, NSUB, HI, VAR, NTB, PART, GEN, U8}, launch_gemm2h_streamk_t<NSUB, HI, VAR, NTB, PART, GEN, U8>}; }

// the instantiations production launches take: 11 of gemm2h_kernel, 17 of gemm2h_streamk_kernel (the last rows: the
// byte forms of the two-block count stream)
static constexpr G2Entry G2_KSPLIT[] = {
    g2_ksplit<1, true, 0, false, true>(),  g2_ksplit<1, true, 0, true, true>(),  g2_ksplit<1, true, 4, false, true>(),
    g2_ksplit<1, true, 4, true, true>(),   g2_ksplit<1, true, 0, false, false>(), g2_ksplit<1, true, 0, true, false>(),
    g2_ksplit<2, false, 4, false, false>(), g2_ksplit<2, false, 4, true, false>(), g2_ksplit<1, false, 4, false, false>(),
    g2_ksplit<2, false, 4, false, false, true>(), g2_ksplit<2, false, 4, true, false, true>()};
static constexpr G2Entry G2_STREAMK[] = {
    g2_streamk<1, true, 0, false, true, true>(),   g2_streamk<1, true, 0, false, false, true>(),  g2_streamk<1, true, 0, true, false, true>(),
    g2_streamk<1, true, 4, false, true, true>(),   g2_streamk<1, true, 4, false, false, true>(),  g2_streamk<1, true, 4, true, false, true>(),
    g2_streamk<1, true, 0, false, true, false>(),  g2_streamk<1, true, 0, false, false, false>(), g2_streamk<1, true, 0, true, false, false>(),
    g2_streamk<2, false, 4, false, true, false>(), g2_streamk<2, false, 4, false, false, false>(), g2_streamk<2, false, 4, true, false, false>(),
    g2_streamk<1, false, 4, false, false, false>(), g2_streamk<1, false, 4, true, false, false>(),
    g2_streamk<2, false, 4, false, true, false, true>(), g2_streamk<2, false, 4, false, false, false, true>(), g2_streamk<2, false, 4, true, false, false, true>()};

static G2Form g2_form_of(const G2Launch& g, int KC, bool shared)
{
    const unsigned long long full = g2_full_mask(KC);
    return g2_form(g.x.hi != nullptr, g.x.colscale != nullptr, g.kn->g2_gen4, g.kn->g2_gvar, gemm2h_nsub(false, g.Kb, g.kn->g2_nsub),
                   (g.livemask & full) != full, shared, g.x.bytes);
}

// Instruction streams (the VAR parameter of kernels_gemm2h.hip.h): production launches use 4, the spread stream, and 0,
// the burst loop, on the two-plane count path; general matrices (GEN) take 0 instead of 4 with CNMF_G2_GVAR=0 (same bits).
static hipError_t launch_gemm2h(hipStream_t st, const G2Launch& g)
{
    G2Form f = g2_form_of(g, g.KC, false);
    f.NTB = false;                                           // (the K-split kernel has no such parameter)
    for (const G2Entry& e : G2_KSPLIT) if (e.form == f) return e.fn(st, g);
    return hipErrorInvalidValue;
}

static hipError_t launch_gemm2h_streamk(hipStream_t st, const G2Launch& g)
{
    const G2Form f = g2_form_of(g, g.sk->MG * G3_MW, g.sk->MG > 1);
    for (const G2Entry& e : G2_STREAMK) if (e.form == f) return e.fn(st, g);
    return hipErrorInvalidValue;
}

// f16 planes of a packed factor (rows, K multiples of 64) from the sweep's row-maximum partials
static hipError_t launch_split2h(hipStream_t st, const float* src, int ld, int rows, int K, unsigned char* dst, int TR,
                                 const double* kscale, const float* rmax_part, int parts, float* inv_scale)
{
    if (split2h_wide(K)) {
        dim3 grid(split2h_col_groups(K, rows), rows / 16);
        split2h_tiled_kernel<16, 16><<<grid, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale, rmax_part, parts, inv_scale);
    } else {
        dim3 grid(split2h_col_groups(K, rows), rows / 64);
        split2h_tiled_kernel<64, 4><<<grid, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale, rmax_part, parts, inv_scale);
    }
    return hipGetLastError();
}

// row-maximum partials of rows the sweep has not produced (installed / moved slots): [rows][parts]
static hipError_t launch_rowmax_part(hipStream_t st, const float* V, int ld, int L, int rows, int span,
                                     const double* kscale, int parts, float* rmax_part)
{
    dim3 grid(parts, rows / 4);
    rowmax_part_kernel<<<grid, 256, 0, st>>>(V, ld, L, span, kscale, parts, rmax_part);
    return hipGetLastError();
}

// Examine the resident matrix once: is every column (integers <= 256) x one constant?  If so build the
// integer planes of X and X^T and the per-gene scale (kernels_counts.hip.h, kernels_planes.hip.h).  counts.state leaves "not examined" at two
// points only: `absent`, where the examination has decided so, and the commit after the last synchronisation -- a
// failed call leaves it "not examined", and the next call on this matrix examines it again.
static int ensure_counts(cnmf_ctx* ctx)
{
    // plane format the current mode multiplies; 5: the f16 pipe with the count plane as bytes where every count fits one
    // (CNMF_G2_U8; the byte plane is read by the two-block stream only: not with CNMF_G2_NSUB=1)
    const int fmt = ctx->knobs.gemm3 == 4 ? ((ctx->knobs.g2_u8 && ctx->knobs.g2_nsub == 2) ? 5 : 4) : 3;
    if (ctx->counts.state == 1 && ctx->counts.fmt != fmt) {
        // the mode was switched between two calls on the same matrix (tests, A/B runs): rebuild the planes
        hipStreamSynchronize(ctx->stream);
        ctx->counts.release();
    }
    if (ctx->counts.state != 0) return CNMF_OK;
    auto absent = [ctx] { ctx->counts.state = -1; return CNMF_OK; };
    const int N = (int)ctx->N, G = (int)ctx->G;
    if (ctx->N_pad % G3C_JW || ctx->G_pad % G3C_JW || ctx->knobs.no_counts || !ctx->count_detect) return absent();
    hipStream_t st = ctx->stream;
    const int chunks = (N + CNT_ROWS - 1) / CNT_ROWS;      // on grid.y of the column passes
    if (chunks > PLAN_GRID_YZ) { SET_ERR(ctx, "count detection: too many rows for one launch"); return CNMF_EINVAL; }
    DevPool pool;
    float* part = pool.get<float>((size_t)chunks * G);
    float* vmin = pool.get<float>(G);
    unsigned* fail = pool.get<unsigned>(G, true, st);
    float* unit = pool.get<float>(G);
    double* psx = pool.get<double>((size_t)chunks * G);
    double* psn = pool.get<double>((size_t)chunks * G);
    POOL_TRY(ctx, pool);
    dim3 grid((G + 255) / 256, chunks);
    col_minpos_kernel<<<grid, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, part);
    col_min_combine_kernel<<<(G + 255) / 256, 256, 0, st>>>(part, chunks, G, vmin);
    count_check_kernel<<<grid, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, vmin, fail);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<float> h_v(G), h_unit(G);
    std::vector<unsigned> h_fail(G);
    HIP_TRY(ctx, hipMemcpyAsync(h_v.data(), vmin, (size_t)G * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(h_fail.data(), fail, (size_t)G * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int g = 0; g < G; ++g) {
        int m = 0;
        for (int c = 1; c <= CNT_MAXMULT && !m; ++c) if (!(h_fail[g] & (1u << (c - 1)))) m = c;
        if (!m) return absent();                           // this gene is not (small integers) x constant
        h_unit[g] = h_v[g] > 0.f ? h_v[g] / (float)m : 0.f;
    }
    HIP_TRY(ctx, hipMemcpyAsync(unit, h_unit.data(), (size_t)G * sizeof(float), hipMemcpyHostToDevice, st));
    OwnedLocal<CountPlanesF> L;
    L.fmt = fmt;
    HIP_TRY(ctx, hipMalloc(&L.d_scale, (size_t)ctx->G_pad * sizeof(double)));
    count_sums_kernel<<<grid, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, unit, psx, psn);
    count_scale_kernel<<<(ctx->G_pad + 255) / 256, 256, 0, st>>>(psx, psn, chunks, G, ctx->G_pad, L.d_scale);
    // does any count exceed 256?  then a second plane (256 hi) with per-block flags rides along
    // (fmt 5: and does any exceed 255?  if none does, ONE plane of bytes; else exactly the f16 planes of fmt 4)
    unsigned* any_big = pool.get<unsigned>(2, true, st);
    POOL_TRY(ctx, pool);
    count_max_base_kernel<<<grid, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, unit, fmt >= 4 ? G2_COUNT_BASE : 256.0f, any_big);
    if (fmt == 5) count_max_base_kernel<<<grid, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, unit, 255.0f, any_big + 1);
    unsigned h_bigs[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(h_bigs, any_big, sizeof h_bigs, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const unsigned h_big = h_bigs[0];
    L.bytes = fmt == 5 && !h_bigs[1];
    const size_t bytes = (size_t)ctx->N_pad * ctx->G_pad * (L.bytes ? 1 : 2);
    HIP_TRY(ctx, hipMalloc(&L.C1, bytes));
    HIP_TRY(ctx, hipMalloc(&L.Ct1, bytes));
    if (h_big) {
        const size_t nfA = (size_t)(ctx->N_pad / G3C_JW) * ((ctx->G_pad / 16 + 31) / 32) * sizeof(unsigned int);
        const size_t nfB = (size_t)(ctx->G_pad / G3C_JW) * ((ctx->N_pad / 16 + 31) / 32) * sizeof(unsigned int);
        HIP_TRY(ctx, hipMalloc(&L.C1h, bytes));
        HIP_TRY(ctx, hipMalloc(&L.Ct1h, bytes));
        HIP_TRY(ctx, hipMalloc(&L.hiA, nfA));
        HIP_TRY(ctx, hipMalloc(&L.hiB, nfB));
        HIP_TRY(ctx, hipMemsetAsync(L.hiA, 0, nfA, st));
        HIP_TRY(ctx, hipMemsetAsync(L.hiB, 0, nfB, st));
    }
    const XPlaneFormat pf = L.bytes ? XPlaneFormat::COUNT_U8 : (fmt >= 4 ? XPlaneFormat::COUNT_F16 : XPlaneFormat::COUNT_BF16);
    HIP_TRY(ctx, launch_x_planes(st, pf, false, ctx->X, ctx->G_pad, N, G, ctx->N_pad, ctx->G_pad, unit, L.C1, L.C1h, L.hiA));
    HIP_TRY(ctx, launch_x_planes(st, pf, true, ctx->X, ctx->G_pad, N, G, ctx->G_pad, ctx->N_pad, unit, L.Ct1, L.Ct1h, L.hiB));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));                // the pool's scratch is freed on return
    L.state = 1;
    ctx->counts.take(L);
    return CNMF_OK;
}

// the split-operand path needs whole 256 x 128 tiles
static bool gemm3_enabled(const cnmf_ctx* ctx, int KC)
{
    // (the plane builders carry the 16-cell blocks on grid.x, so matrices beyond 65 535 x 16 = 1 048 560 cells keep the
    //  matrix-pipe path -- probed at 1 100 000 x 2 000, 2.25e9 padded elements: tools/probe_big_matrix.py; a shape one of
    //  whose builder or detection launches would not fit its grid takes the f32 pipe: x_launches_fit, pass_plan.h)
    return ctx->knobs.gemm3 != 0 && KC % G3_MW == 0 && ctx->G_pad % gemm3_jw() == 0 && ctx->N_pad % gemm3_jw() == 0 &&
           x_launches_fit(PadShape{ctx->N_pad, ctx->G_pad}, ctx->knobs.gemm3);
}

static hipError_t launch_split2h_finalize(hipStream_t st, const float* src, int ld, int rows, int K, unsigned char* dst,
                                          int TR, const double* kscale, const float* rmax_part, int parts,
                                          float* inv_scale, const FinalizeArgs& fa, int nslots, int fin_y, SplitFused fu)
{
    const int bx = split2h_col_groups(K, rows);
    if (split2h_wide(K)) {
        const int by = rows / 16;
        split2h_finalize_kernel<16, 16><<<bx * by + nslots * fin_y, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale,
                                                                                rmax_part, parts, inv_scale, bx, by, fa, fin_y, fu);
    } else {
        const int by = rows / 64;
        split2h_finalize_kernel<64, 4><<<bx * by + nslots * fin_y, 256, 0, st>>>(src, ld, K, TR, (unsigned short*)dst, kscale,
                                                                               rmax_part, parts, inv_scale, bx, by, fa, fin_y, fu);
    }
    return hipGetLastError();
}
