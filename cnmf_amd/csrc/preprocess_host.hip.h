// The O(N G) passes of the reference's Preprocess.normalize_batchcorrect (preprocess.py:314-358) on the device, over a
// staging slot of their own (ctx->pre) that leaves the resident matrix, the spectra store and the prepare staging alone:
//
//   * one upload of the raw counts (CSR, float64 values) and its transpose serve every selection: normalize_total's row
//     scale (x * target / row sum) is applied on the fly, so the library-size-normalised copy for the PCA and the raw
//     copy for the correction come from the same staged counts (preprocess.py:316-321);
//   * sc.pp.scale(zero_center=False, max_value) + the global quantile ceiling (stdscale_quantile_celing, :21-29): the
//     column moments and the gather are prepare_host.hip.h's (float64 sums in the order of kernels_segments.hip.h,
//     counting-sort transposes); the
//     ceiling's order statistics come from a radix select over the float64 bit patterns (all values >= 0, so the bit
//     order is the value order; -0.0 is taken as +0.0) with integer counters only, the implicit zeros of a CSR slot counted analytically;
//   * PCA (sc.pp.pca(zero_center=True)): column means and the G x G scatter matrix, then the scores (X - mean) V, on the
//     float64 MFMA pipe; the eigendecomposition runs on the host (or, opt-in, as a Householder tridiagonalisation on the
//     device with only the tridiagonal problem on the host: pca_host.hip.h);
//   * Harmony's ridge correction (moe_correct_ridge, :9-18): every cluster's W_k = (Phi_Rk Phi^T + lamb)^-1 Phi_Rk X is
//     formed from the UNcorrected X, so the K updates are independent.  With A[(k,b), n] = R[k,n] Phi[b,n] (formed on
//     the fly from R^T / Phi^T, never stored): one moments pass M = A X and Gram_k = A Phi^T (split-K over the cells,
//     fixed-order second stage), the K small solves on the host, and one apply pass X = max(X - A^T W, 0) in place.
//
// No float atomics anywhere: two calls on the same input give the same bits.
// Included by cnmf_hip.hip (after prepare_host.hip.h and kernels_consensus.hip.h).
#pragma once

namespace cnmf {

// ---------------------------------------------------------------- order statistics and ceilings on a value array
// histogram of digit (key >> shift) & 255 over the keys whose bits above shift + 8 equal those of prefix; -0.0 counts
// as +0.0 (numpy orders them as equal), so only values < 0 (and NaNs with the sign bit) reach the digits 128..255
__global__ __launch_bounds__(256) void pre_radix_hist_kernel(const double* __restrict__ v, long long n,
                                                             unsigned long long prefix, int shift,
                                                             unsigned long long* __restrict__ hist)
{
    __shared__ unsigned int h[256];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const unsigned long long mask = shift + 8 >= 64 ? 0ull : (~0ull << (shift + 8));
    for (long long i = (long long)blockIdx.x * 256 + t; i < n; i += (long long)gridDim.x * 256) {
        unsigned long long key = (unsigned long long)__double_as_longlong(v[i]);
        if (key == 0x8000000000000000ull) key = 0ull;
        if ((key & mask) == prefix) atomicAdd(&h[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[t]) atomicAdd(&hist[t], (unsigned long long)h[t]);
}

// v > thresh -> thresh (the reference's `X[X > t] = t`)
__global__ __launch_bounds__(256) void pre_ceiling_kernel(double* __restrict__ v, long long n, double thresh)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        if (v[i] > thresh) v[i] = thresh;
}

// out[p] = cval[p] * scale[crow[p]]: the row-scaled values of the transposed counts
__global__ __launch_bounds__(256) void pre_scale_cols_kernel(const int* __restrict__ crow, const double* __restrict__ cval,
                                                             long long n, const double* __restrict__ scale,
                                                             double* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = cval[i] * scale[crow[i]];
}

// ---------------------------------------------------------------- column means of a dense [N][C] matrix
// partial sums over row chunk s (rows s*rpc .. ), 64 columns per block, 4 row phases summed in a fixed order
__global__ __launch_bounds__(256) void pre_colsum_partial_kernel(const double* __restrict__ X, int N, int C, int rpc,
                                                                 double* __restrict__ part)
{
    __shared__ double red[4][64];
    const int t = threadIdx.x, c = blockIdx.x * 64 + (t & 63), ph = t >> 6, s = blockIdx.y;
    const int r0 = s * rpc, r1 = min(N, r0 + rpc);
    double acc = 0.0;
    if (c < C)
        for (int r = r0 + ph; r < r1; r += 4) acc += X[(size_t)r * C + c];
    red[ph][t & 63] = acc;
    __syncthreads();
    if (ph == 0 && c < C) part[(size_t)s * C + c] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void pre_colmean_kernel(const double* __restrict__ part, int S, int N, int C,
                                                          double* __restrict__ mean)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += part[(size_t)i * C + c];
    mean[c] = s / (double)N;
}

// out[m][n] = sum over s of part[s][m][n], s in order
__global__ __launch_bounds__(256) void pre_splitk_sum_kernel(const double* __restrict__ part, long long stride, int S,
                                                             long long n, double* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        double s = 0.0;
        for (int k = 0; k < S; ++k) s += part[(size_t)k * stride + i];
        out[i] = s;
    }
}

// ---------------------------------------------------------------- float64 MFMA products with generated operands
// C[m][n] = sum_k A(m, k) B(k, n) over k in [z * kps, (z + 1) * kps) (z = blockIdx.z), M x Nn outputs.
// A modes:  0  A(m, k) = X[k][m] - mu[m]          (scatter matrix; k = cell, m = gene)
//           1  A(m, k) = Rt[k][m / B1] Pt[k][m % B1]   (ridge moments; k = cell, m = (cluster, covariate))
//           2  A(m, k) = X[m][k] - mu[k]          (PCA scores; m = cell, k = gene)
//           3  A(m, k) = Rt[m][k / B1] Pt[m][k % B1]   (ridge apply; m = cell, k = (cluster, covariate))
// B modes:  0  B(k, n) = Bm[k][n]                 1  B(k, n) = X[k][n] - mu[n]
// Epilogues: 0  C[z][m][n] = acc (split-K partial, z stride cs)     1  X[m][n] = max(X[m][n] - acc, 0) (in place)
//            2  X[m][n] = X[m][n] - acc (in place, no clip: a matrix with negative entries, Harmony's PCA scores)
// Workgroup tile 64 x 64, 4 waves (2 x 2) of 32 x 32 = 2 x 2 v_mfma_f64_16x16x4f64 tiles, k steps of 16 through LDS
// (double-buffered).  Every global access is guarded: the edges of every dimension are zero-filled.
//   A operand lane l: A[m = l&15][k = l>>4]   B operand lane l: B[k = l>>4][n = l&15]
//   D reg r lane l  : row = (l>>4) + 4 r, col = l&15                  (the f64 layout, not the f32 one)
struct PreGemm {
    int M, Nn, K, kps;
    double* X; int ldx; const double* mu;           // (the apply epilogue writes X in place)
    const double* Rt; const double* Pt; int KR, B1;
    const double* Bm; int ldb;
    double* C; int ldc; long long cs;
};

constexpr int PLD = 64 + 4;     // LDS row (doubles) of a k-major 16 x 64 operand tile

template <int AM>
__device__ __forceinline__ double pre_a(const PreGemm& g, int m, int k)
{
    if (m >= g.M || k >= g.K) return 0.0;
    if (AM == 0) return g.X[(size_t)k * g.ldx + m] - g.mu[m];
    if (AM == 1) return g.Rt[(size_t)k * g.KR + m / g.B1] * g.Pt[(size_t)k * g.B1 + m % g.B1];
    if (AM == 2) return g.X[(size_t)m * g.ldx + k] - g.mu[k];
    return g.Rt[(size_t)m * g.KR + k / g.B1] * g.Pt[(size_t)m * g.B1 + k % g.B1];
}

template <int BM>
__device__ __forceinline__ double pre_b(const PreGemm& g, int k, int n)
{
    if (n >= g.Nn || k >= g.K) return 0.0;
    if (BM == 0) return g.Bm[(size_t)k * g.ldb + n];
    return g.X[(size_t)k * g.ldx + n] - g.mu[n];
}

template <int AM, int BM, int EPI>
__global__ __launch_bounds__(256) void pre_gemm_kernel(const PreGemm g)
{
    __shared__ __attribute__((aligned(16))) double As[2][16 * PLD];
    __shared__ __attribute__((aligned(16))) double Bs[2][16 * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int kb = blockIdx.z * g.kps, ke = min(g.K, kb + g.kps);
    constexpr bool A_KMAJOR = AM <= 1;
    double ar[4], br[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int m, k;
            if (A_KMAJOR) { m = tid & 63; k = (tid >> 6) + 4 * r; }
            else { k = tid & 15; m = (tid >> 4) + 16 * r; }
            ar[r] = k0 + k < ke ? pre_a<AM>(g, m0 + m, k0 + k) : 0.0;
            const int n = tid & 63, kk = (tid >> 6) + 4 * r;
            br[r] = k0 + kk < ke ? pre_b<BM>(g, k0 + kk, n0 + n) : 0.0;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int m, k;
            if (A_KMAJOR) { m = tid & 63; k = (tid >> 6) + 4 * r; }
            else { k = tid & 15; m = (tid >> 4) + 16 * r; }
            As[buf][k * PLD + m] = ar[r];
            Bs[buf][((tid >> 6) + 4 * r) * PLD + (tid & 63)] = br[r];
        }
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nk = ke > kb ? (ke - kb + 15) / 16 : 0;
    if (nk > 0) { load(kb); store(0); }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load(kb + (kt + 1) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double* as = &As[buf][(q * 4 + lk) * PLD + wm * 32 + li];
            const double* bs = &Bs[buf][(q * 4 + lk) * PLD + wn * 32 + li];
            const double a0 = as[0], a1 = as[16], b0 = bs[0], b1 = bs[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + i * 16 + lk + 4 * r, n = n0 + wn * 32 + j * 16 + li;
                if (m >= g.M || n >= g.Nn) continue;
                if (EPI == 0) {
                    g.C[(size_t)blockIdx.z * g.cs + (size_t)m * g.ldc + n] = acc[i][j][r];
                } else if (EPI == 1) {
                    double* p = g.X + (size_t)m * g.ldx + n;
                    *p = fmax(*p - acc[i][j][r], 0.0);
                } else {
                    double* p = g.X + (size_t)m * g.ldx + n;
                    *p = *p - acc[i][j][r];
                }
            }
}

}  // namespace cnmf

static inline unsigned pre_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192)); }

// split-K factor for an M x Nn product over K: about 2048 workgroups, at most 16 splits, at least 256 k per split;
// a function of the shape alone (the partition, hence the bits, never depends on anything else)
static int pre_splits(int M, int Nn, int K, int* kps)
{
    const long long tiles = (long long)((M + 63) / 64) * ((Nn + 63) / 64);
    long long S = std::max<long long>(1, std::min<long long>(16, 2048 / std::max<long long>(1, tiles)));
    S = std::max<long long>(1, std::min<long long>(S, K / 256));
    int k = (int)((K + S - 1) / S);
    k = (k + 15) / 16 * 16;
    *kps = std::max(16, k);
    return (int)((K + *kps - 1) / *kps);
}

// C [M][Nn] (device) = the product of g over all of K, split-K partials summed in a fixed order
template <int AM, int BM>
static int pre_product(cnmf_ctx* ctx, cnmf::PreGemm g, double* C)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    int kps = 16;
    const int S = pre_splits(g.M, g.Nn, g.K, &kps);
    DevPool pool;
    double* part = pool.get<double>((size_t)S * g.M * g.Nn);
    POOL_TRY(ctx, pool);
    g.kps = kps; g.C = part; g.ldc = g.Nn; g.cs = (long long)g.M * g.Nn;
    dim3 grid((g.Nn + 63) / 64, (g.M + 63) / 64, S);
    pre_gemm_kernel<AM, BM, 0><<<grid, 256, 0, st>>>(g);
    const long long n = (long long)g.M * g.Nn;
    pre_splitk_sum_kernel<<<pre_grid(n), 256, 0, st>>>(part, g.cs, S, n, C);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the pool frees `part` on return)
    return CNMF_OK;
}

static int pre_slot_arg(cnmf_ctx* ctx, int slot, bool need_data)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (slot < 0 || slot > 1) { SET_ERR(ctx, "slot %d outside [0, 1]", slot); return CNMF_EINVAL; }
    if (need_data && ctx->pre.slot[slot].empty()) { SET_ERR(ctx, "preprocess slot %d is empty", slot); return CNMF_ESTATE; }
    return CNMF_OK;
}

static int pre_need_dense(cnmf_ctx* ctx, int slot)
{
    if (int rc = pre_slot_arg(ctx, slot, true)) return rc;
    if (!ctx->pre.slot[slot].dense) { SET_ERR(ctx, "preprocess slot %d is not dense (cnmf_preprocess_densify)", slot); return CNMF_ESTATE; }
    return CNMF_OK;
}

// the values of a slot: the stored entries of a CSR slot, every entry of a dense one; *zeros = implicit zeros
static double* pre_values(cnmf_ctx* ctx, int slot, long long* n, long long* zeros)
{
    PreSlot& S = ctx->pre.slot[slot];
    const long long all = ctx->pre.N * S.n;
    if (S.dense) { *n = all; *zeros = 0; return S.dense; }
    *n = S.csr.nnz; *zeros = all - S.csr.nnz;
    return S.csr.val;
}

extern "C" int cnmf_preprocess_upload_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                                          int data_is_f64, int64_t n_cells, int64_t n_genes)
{
    if (int rc = prep_csr_args(ctx, indptr, indices, data, n_cells, n_genes)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PreStage& P = ctx->pre;
    hipStreamSynchronize(ctx->stream);
    P.release();
    if (int rc = stage_counts(ctx, indptr, indices, data, data_is_f64, n_cells, n_genes, false, true, P)) return rc;
    P.N = n_cells;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_set_dense(cnmf_ctx* ctx, int32_t slot, const double* X, int64_t n_rows, int64_t n_cols)
{
    if (int rc = pre_slot_arg(ctx, slot, false)) return rc;
    PreStage& P = ctx->pre;
    if (!X) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (n_rows <= 0 || n_cols <= 0 || n_rows > (1ll << 30) || n_cols > (1ll << 24)) {
        SET_ERR(ctx, "bad matrix shape %lld x %lld", (long long)n_rows, (long long)n_cols);
        return CNMF_EINVAL;
    }
    const bool other = P.staged() || !P.slot[1 - slot].empty();
    if (other && P.N != n_rows) {
        SET_ERR(ctx, "%lld rows where the staged data has %lld cells", (long long)n_rows, (long long)P.N);
        return CNMF_EINVAL;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipStreamSynchronize(st);
    PreSlot& S = P.slot[slot];
    S.release();
    const size_t bytes = (size_t)n_rows * n_cols * sizeof(double);
    HIP_TRY(ctx, hipMalloc((void**)&S.dense, bytes));
    hipError_t e = hipMemcpyAsync(S.dense, X, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) S.release();
    HIP_TRY(ctx, e);
    P.N = n_rows; S.n = n_cols;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_select(cnmf_ctx* ctx, int32_t slot, int32_t n_sel, const int32_t* genes, double target_sum,
                                      double max_value, double* std_out, int64_t* nnz_out)
{
    using namespace cnmf;
    if (int rc = pre_slot_arg(ctx, slot, false)) return rc;
    if (!genes || !std_out || !nnz_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (!P.staged()) { SET_ERR(ctx, "cnmf_preprocess_upload_csr has not been called"); return CNMF_ESTATE; }
    if (int rc = select_check_genes(ctx, P, n_sel, genes)) return rc;
    if (std::isnan(max_value)) { SET_ERR(ctx, "max_value is NaN"); return CNMF_EINVAL; }
    const int N = (int)P.N;
    const long long nnz = P.counts.nnz;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PreSlot& S = P.slot[slot];
    hipStreamSynchronize(st);
    S.release();
    DevPool pool;
    double *rs, *scale = nullptr;
    double* sval = target_sum > 0.0 ? pool.get<double>((size_t)std::max<long long>(nnz, 1)) : nullptr;
    POOL_TRY(ctx, pool);
    if (sval) {
        // normalize_total over ALL genes of the staged counts, then the row-scaled values of the transpose
        if (int rc = stage_row_scale(ctx, P, target_sum, pool, &rs, &scale)) return rc;
        pre_scale_cols_kernel<<<pre_grid(nnz), 256, 0, st>>>(P.columns.idx, P.columns.val, nnz, scale, sval);
    }
    if (int rc = select_scaled_columns(ctx, P, scale ? sval : P.columns.val, n_sel, genes, std_out, &S.csr)) return rc;
    S.n = n_sel;
    const long long nnz_sel = S.csr.nnz;
    if (!(max_value == INFINITY) && nnz_sel > 0) {
        pre_ceiling_kernel<<<pre_grid(nnz_sel), 256, 0, st>>>(S.csr.val, nnz_sel, max_value);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *nnz_out = nnz_sel;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_order_stats(cnmf_ctx* ctx, int32_t slot, int64_t k, double* lo, double* hi)
{
    using namespace cnmf;
    if (int rc = pre_slot_arg(ctx, slot, true)) return rc;
    if (!lo || !hi) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    long long n = 0, zeros = 0;
    const double* v = pre_values(ctx, slot, &n, &zeros);
    const long long total = n + zeros;
    if (k < 0 || k >= total) { SET_ERR(ctx, "rank %lld outside [0, %lld)", (long long)k, total); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    unsigned long long* hist = pool.get<unsigned long long>(256);
    POOL_TRY(ctx, pool);
    std::vector<unsigned long long> h(256);
    const long long ranks[2] = {(long long)k, std::min<long long>(k + 1, total - 1)};
    double out[2];
    for (int w = 0; w < 2; ++w) {
        long long rank = ranks[w];
        if (rank < zeros) { out[w] = 0.0; continue; }     // the implicit zeros sort first (every value is >= 0)
        rank -= zeros;
        unsigned long long prefix = 0;
        for (int shift = 56; shift >= 0; shift -= 8) {
            HIP_TRY(ctx, hipMemsetAsync(hist, 0, 256 * sizeof(unsigned long long), st));
            pre_radix_hist_kernel<<<pre_grid(n), 256, 0, st>>>(v, n, prefix, shift, hist);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(h.data(), hist, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (shift == 56) {
                unsigned long long neg = 0;
                for (int d = 128; d < 256; ++d) neg += h[d];
                if (neg) { SET_ERR(ctx, "the quantile ceiling needs values >= 0 (%llu negative)", neg); return CNMF_EINVAL; }
            }
            int d = 0;
            while (d < 255 && (long long)h[d] <= rank) rank -= (long long)h[d++];
            prefix |= (unsigned long long)d << shift;
        }
        std::memcpy(&out[w], &prefix, sizeof(double));
    }
    *lo = out[0]; *hi = out[1];
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_ceiling(cnmf_ctx* ctx, int32_t slot, double thresh)
{
    using namespace cnmf;
    if (int rc = pre_slot_arg(ctx, slot, true)) return rc;
    if (std::isnan(thresh)) { SET_ERR(ctx, "threshold is NaN"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    long long n = 0, zeros = 0;
    double* v = pre_values(ctx, slot, &n, &zeros);
    if (n > 0) pre_ceiling_kernel<<<pre_grid(n), 256, 0, st>>>(v, n, thresh);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_densify(cnmf_ctx* ctx, int32_t slot)
{
    using namespace cnmf;
    if (int rc = pre_slot_arg(ctx, slot, true)) return rc;
    PreSlot& S = ctx->pre.slot[slot];
    if (S.dense) return CNMF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = (int)ctx->pre.N, C = (int)S.n;
    const size_t bytes = (size_t)N * C * sizeof(double);
    double* d = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemsetAsync(d, 0, bytes, st);
    if (e == hipSuccess) {
        prep_store_kernel<<<seg_grid(N), 256, 0, st>>>(S.csr.ptr, S.csr.idx, S.csr.val, N, C, 0, nullptr, nullptr, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) hipFree(d);
    HIP_TRY(ctx, e);
    S.csr.release();
    S.dense = d;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_fetch(cnmf_ctx* ctx, int32_t slot, int64_t* indptr, int32_t* indices, double* values)
{
    if (int rc = pre_slot_arg(ctx, slot, true)) return rc;
    if (!values) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PreSlot& S = ctx->pre.slot[slot];
    const size_t N = (size_t)ctx->pre.N;
    if (S.dense) {
        HIP_TRY(ctx, hipMemcpyAsync(values, S.dense, N * (size_t)S.n * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        if (!indptr || (!indices && S.csr.nnz > 0)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
        if (int rc = csr_fetch<double>(ctx, S.csr, indptr, indices, values)) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

// the column means mu [n] and the scatter matrix out [n][n] of a dense slot, both on the device
static int pre_scatter_device(cnmf_ctx* ctx, int slot, double* mu, double* out)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    PreSlot& S = ctx->pre.slot[slot];
    const int N = (int)ctx->pre.N, C = (int)S.n;
    const int rpc = std::max(64, (N + 63) / 64), nch = (N + rpc - 1) / rpc;
    DevPool pool;
    double* part = pool.get<double>((size_t)nch * C);
    POOL_TRY(ctx, pool);
    pre_colsum_partial_kernel<<<dim3((C + 63) / 64, nch), 256, 0, st>>>(S.dense, N, C, rpc, part);
    pre_colmean_kernel<<<(C + 255) / 256, 256, 0, st>>>(part, nch, N, C, mu);
    HIP_TRY(ctx, hipGetLastError());
    PreGemm g{};
    g.M = C; g.Nn = C; g.K = N; g.X = S.dense; g.ldx = C; g.mu = mu;
    return pre_product<0, 1>(ctx, g, out);
}

extern "C" int cnmf_preprocess_scatter(cnmf_ctx* ctx, int32_t slot, double* mean, double* scatter)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!mean || !scatter) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int C = (int)ctx->pre.slot[slot].n;
    DevPool pool;
    double* mu = pool.get<double>(C);
    double* out = pool.get<double>((size_t)C * C);
    POOL_TRY(ctx, pool);
    if (int rc = pre_scatter_device(ctx, slot, mu, out)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(mean, mu, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(scatter, out, (size_t)C * C * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_project(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, const double* mean, const double* V,
                                       double* scores)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!mean || !V || !scores) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreSlot& S = ctx->pre.slot[slot];
    const int N = (int)ctx->pre.N, C = (int)S.n;
    if (n_comp <= 0 || n_comp > C) { SET_ERR(ctx, "n_comp = %d outside [1, %d]", n_comp, C); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* mu = pool.get<double>(C);
    double* dV = pool.get<double>((size_t)C * n_comp);
    double* out = pool.get<double>((size_t)N * n_comp);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(mu, mean, (size_t)C * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dV, V, (size_t)C * n_comp * sizeof(double), hipMemcpyHostToDevice, st));
    PreGemm g{};
    g.M = N; g.Nn = n_comp; g.K = C; g.X = S.dense; g.ldx = C; g.mu = mu; g.Bm = dV; g.ldb = n_comp;
    if (int rc = pre_product<2, 0>(ctx, g, out)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(scores, out, (size_t)N * n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_ridge_moments(cnmf_ctx* ctx, int32_t slot, int32_t K, int32_t B1, const double* Rt,
                                             const double* Phit, double* M, double* gram)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!Rt || !Phit || !M || !gram) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (K <= 0 || B1 <= 0) { SET_ERR(ctx, "K = %d, B1 = %d must be positive", K, B1); return CNMF_EINVAL; }
    if ((long long)K * B1 > CNMF_RIDGE_MAX) {
        SET_ERR(ctx, "K * (B + 1) = %lld above %d", (long long)K * B1, CNMF_RIDGE_MAX);
        return CNMF_EUNSUPPORTED;
    }
    PreStage& P = ctx->pre;
    PreSlot& S = P.slot[slot];
    const int N = (int)P.N, C = (int)S.n, KB = K * B1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipStreamSynchronize(st);
    P.release_ridge();
    hipError_t e = hipMalloc((void**)&P.Rt, (size_t)N * K * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P.Pt, (size_t)N * B1 * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(P.Rt, Rt, (size_t)N * K * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(P.Pt, Phit, (size_t)N * B1 * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) P.release_ridge();
    HIP_TRY(ctx, e);
    P.K = K; P.B1 = B1;
    DevPool pool;
    double* dM = pool.get<double>((size_t)KB * C);
    double* dG = pool.get<double>((size_t)KB * B1);
    POOL_TRY(ctx, pool);
    PreGemm g{};
    g.M = KB; g.Nn = C; g.K = N; g.Rt = P.Rt; g.Pt = P.Pt; g.KR = K; g.B1 = B1; g.Bm = S.dense; g.ldb = C;
    if (int rc = pre_product<1, 0>(ctx, g, dM)) return rc;
    g.Nn = B1; g.Bm = P.Pt; g.ldb = B1;               // Gram_k[b][c] = sum_n R[k,n] Phi[b,n] Phi[c,n]
    if (int rc = pre_product<1, 0>(ctx, g, dG)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(M, dM, (size_t)KB * C * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(gram, dG, (size_t)KB * B1 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_ridge_apply(cnmf_ctx* ctx, int32_t slot, const double* W)
{
    return cnmf_preprocess_ridge_apply_mode(ctx, slot, W, 1);
}

extern "C" int cnmf_preprocess_ridge_apply_mode(cnmf_ctx* ctx, int32_t slot, const double* W, int32_t clip)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!W) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (!P.Rt) { SET_ERR(ctx, "cnmf_preprocess_ridge_moments has not been called"); return CNMF_ESTATE; }
    PreSlot& S = P.slot[slot];
    const int N = (int)P.N, C = (int)S.n, KB = P.K * P.B1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dW = pool.get<double>((size_t)KB * C);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dW, W, (size_t)KB * C * sizeof(double), hipMemcpyHostToDevice, st));
    PreGemm g{};
    g.M = N; g.Nn = C; g.K = KB; g.kps = KB; g.X = S.dense; g.ldx = C; g.Rt = P.Rt; g.Pt = P.Pt; g.KR = P.K; g.B1 = P.B1;
    g.Bm = dW; g.ldb = C;
    const dim3 grid((C + 63) / 64, (N + 63) / 64, 1);
    if (clip) pre_gemm_kernel<3, 0, 1><<<grid, 256, 0, st>>>(g);
    else pre_gemm_kernel<3, 0, 2><<<grid, 256, 0, st>>>(g);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_release(cnmf_ctx* ctx)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pre.release();
    return CNMF_OK;
}
