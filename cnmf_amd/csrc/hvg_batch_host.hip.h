// The per-batch form of the two O(nnz) passes of hvg_host.hip.h (scanpy's flavor='seurat_v3' with batch_key): the integer
// moments S1[b][g], S2[b][g] and the clipped sums C1[b][g], C2[b][g] of every (batch, gene) pair over the cells of that
// batch alone.
//
//   * the grouped transpose: a SECOND transpose of the staged counts (csr_transpose with a row selection), genes x cells
//     with the cells in the stable order of their batch code.  A column lists its entries by ascending row
//     (csr_host.hip.h), so the entries of batch b in column g are one contiguous run, rows [start[b], start[b + 1]), in
//     the cell order of the staging.  Built on first use and cached in ctx->pre for the codes it was built for; release,
//     subset and every upload drop it (PreStage::release).  The staging the later steps read (counts, columns) is not
//     touched;
//   * both kernels: one wavefront per (batch, gene) pair w = b G + g, all pairs on grid.x (ceil(G B / 4) blocks).  Two
//     binary searches over the rows of column g, uniform over the wavefront, find the run; the lanes stride it FROM ITS
//     FIRST ENTRY and reduce with the 64-lane butterfly of the one-batch kernels.  The additions of a pair are therefore
//     the very sequence hvg_gene_moments_kernel / hvg_clipped_sums_kernel perform on the staging restricted to the cells
//     of b (cnmf_preprocess_subset keeps the stored order): the float64 sums have those bits.  An empty run gives zeros.
//
// Limits, checked on the host before anything is launched: at most HVG_CELLS_MAX cells in all (as for one batch), at most
// HVG_BATCHES_MAX = 4096 batches, none of them empty, and at most HVG_PAIRS_MAX = 2^26 (batch, gene) pairs: the [B][G]
// buffers then hold at most 512 MB each and grid.x at most 2^24 blocks.
// Integer counters and fixed-order float64 sums only -- no float atomics: two calls give the same bits.
// Included by cnmf_hip.hip (after hvg_host.hip.h).
#pragma once

namespace cnmf {

constexpr int HVG_BATCHES_MAX = 4096;
constexpr long long HVG_PAIRS_MAX = 1ll << 26;

// the first p in [lo, hi) with crow[p] >= key (hi when there is none); crow ascending over [lo, hi).  Every lane of the
// wavefront runs the same search
__device__ __forceinline__ long long hvg_first_row_at_least(const int* __restrict__ crow, long long lo, long long hi, int key)
{
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (crow[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wavefront per pair w = b G + g over the grouped transpose: s1[w] = sum x, s2[w] = sum x^2 over the run of batch b
// in column g, flags[w] as in hvg_gene_moments_kernel
__global__ __launch_bounds__(256) void hvg_gene_moments_batched_kernel(const long long* __restrict__ cptr,
                                                                       const int* __restrict__ crow,
                                                                       const double* __restrict__ cval, int G, int B,
                                                                       const int* __restrict__ start,
                                                                       long long* __restrict__ s1, long long* __restrict__ s2,
                                                                       int* __restrict__ flags)
{
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (long long)G * B) return;
    const int bt = (int)(w / G), g = (int)(w - (long long)bt * G);
    const long long end = cptr[g + 1];
    const long long p0 = hvg_first_row_at_least(crow, cptr[g], end, start[bt]);
    const long long p1 = hvg_first_row_at_least(crow, p0, end, start[bt + 1]);
    long long a = 0, b = 0;
    int f = 0;
    for (long long p = p0 + lane; p < p1; p += 64) {
        const double v = cval[p];
        if (!(v >= 0.0) || v != floor(v)) { f |= HVG_FLAG_NOT_COUNT; continue; }
        if (v > HVG_COUNT_MAX) { f |= HVG_FLAG_TOO_LARGE; continue; }
        const long long iv = (long long)v;
        a += iv;
        b += iv * iv;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); f |= __shfl_xor(f, o, 64); }
    if (lane == 0) { s1[w] = a; s2[w] = b; flags[w] = f; }
}

// one wavefront per pair w = b G + g: c1[w] = sum min(x, clip[w]), c2[w] = sum of its square (the square rounded, then
// added) over the run of batch b in column g, in the order of hvg_clipped_sums_kernel on that batch alone
__global__ __launch_bounds__(256) void hvg_clipped_sums_batched_kernel(const long long* __restrict__ cptr,
                                                                       const int* __restrict__ crow,
                                                                       const double* __restrict__ cval, int G, int B,
                                                                       const int* __restrict__ start,
                                                                       const double* __restrict__ clip, double* __restrict__ c1,
                                                                       double* __restrict__ c2)
{
#pragma clang fp contract(off)
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (long long)G * B) return;
    const int bt = (int)(w / G), g = (int)(w - (long long)bt * G);
    const long long end = cptr[g + 1];
    const long long p0 = hvg_first_row_at_least(crow, cptr[g], end, start[bt]);
    const long long p1 = hvg_first_row_at_least(crow, p0, end, start[bt + 1]);
    const double c = clip[w];
    double a = 0.0, b = 0.0;
    for (long long p = p0 + lane; p < p1; p += 64) {
        const double m = fmin(cval[p], c);
        a += m;
        b += m * m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if (lane == 0) { c1[w] = a; c2[w] = b; }
}

}  // namespace cnmf

// The checks both entry points share, and the grouped transpose for (codes, n_batches): built unless the cached one
// answers to the same codes.  Nothing is launched before every check has passed.
static int hvg_ensure_grouped(cnmf_ctx* ctx, const char* who, const int32_t* codes, int32_t n_batches)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!codes) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    const int64_t N = P.N, G = P.counts.cols;
    if (N > HVG_CELLS_MAX) {
        SET_ERR(ctx, "%s: %lld cells, more than %lld (sum x^2 must stay an exact int64)", who, (long long)N, HVG_CELLS_MAX);
        return CNMF_EINVAL;
    }
    if (n_batches < 1 || n_batches > HVG_BATCHES_MAX) {
        SET_ERR(ctx, "%s: %d batches (1 <= n_batches <= %d)", who, (int)n_batches, HVG_BATCHES_MAX);
        return CNMF_EINVAL;
    }
    if (G * (int64_t)n_batches > HVG_PAIRS_MAX) {
        SET_ERR(ctx, "%s: %lld genes x %d batches, more than %lld pairs", who, (long long)G, (int)n_batches, HVG_PAIRS_MAX);
        return CNMF_EINVAL;
    }
    const int B = n_batches;
    std::vector<int> start((size_t)B + 1, 0);
    for (int64_t i = 0; i < N; ++i) {
        if (codes[i] < 0 || codes[i] >= B) {
            SET_ERR(ctx, "%s: batch code %d of cell %lld outside [0, %d)", who, (int)codes[i], (long long)i, B);
            return CNMF_EINVAL;
        }
        ++start[(size_t)codes[i] + 1];
    }
    for (int b = 0; b < B; ++b) {
        if (start[(size_t)b + 1] == 0) { SET_ERR(ctx, "%s: batch %d has no cell", who, b); return CNMF_EINVAL; }
        start[(size_t)b + 1] += start[b];
    }
    if (P.grouped.ptr && P.gB == B && P.gcodes.size() == (size_t)N && std::equal(P.gcodes.begin(), P.gcodes.end(), codes))
        return CNMF_OK;
    // sel: the cells in the stable order of their batch code (row r of the grouped transpose is cell sel[r])
    std::vector<int> sel((size_t)N), next(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < N; ++i) sel[(size_t)next[codes[i]]++] = (int)i;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    int* dsel = pool.get<int>((size_t)N);
    POOL_TRY(ctx, pool);
    int* dstart = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&dstart, ((size_t)B + 1) * sizeof(int)));
    DevCsrLocal<double> grouped;
    hipError_t e = hipMemcpyAsync(dsel, sel.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dstart, start.data(), ((size_t)B + 1) * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                // (sel and start live in this call only)
    int rc = CNMF_OK;
    if (e != hipSuccess) { SET_ERR(ctx, "%s: %s", who, hipGetErrorString(e)); rc = CNMF_EHIP; }
    if (!rc) rc = prep_transpose(ctx, P.counts, dsel, nullptr, N, P.counts.nnz, &grouped);
    if (rc) { hipFree(dstart); return rc; }
    P.release_grouped();
    P.grouped.take(grouped);
    P.gstart = dstart;
    P.gcodes.assign(codes, codes + N);
    P.gB = B;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_gene_moments_batched(cnmf_ctx* ctx, const int32_t* codes, int32_t n_batches, int64_t* s1,
                                                    int64_t* s2, int32_t* flags)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!codes || !s1 || !s2 || !flags) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = hvg_ensure_grouped(ctx, "gene_moments_batched", codes, n_batches)) return rc;
    PreStage& P = ctx->pre;
    const int G = (int)P.counts.cols, B = n_batches;
    const size_t W = (size_t)G * B;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    long long* d1 = pool.get<long long>(W);
    long long* d2 = pool.get<long long>(W);
    int* df = pool.get<int>(W);
    POOL_TRY(ctx, pool);
    std::vector<int> hf(W);
    hvg_gene_moments_batched_kernel<<<(unsigned)((W + 3) / 4), 256, 0, st>>>(P.grouped.ptr, P.grouped.idx, P.grouped.val, G, B,
                                                                            P.gstart, d1, d2, df);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(s1, d1, W * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(s2, d2, W * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(hf.data(), df, W * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
        int all = 0;
        for (int g = 0; g < G; ++g) all |= hf[(size_t)b * G + g];
        flags[b] = all;
    }
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_clipped_sums_batched(cnmf_ctx* ctx, const int32_t* codes, int32_t n_batches, const double* clip,
                                                    double* c1, double* c2)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!codes || !clip || !c1 || !c2) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = hvg_ensure_grouped(ctx, "clipped_sums_batched", codes, n_batches)) return rc;
    PreStage& P = ctx->pre;
    const int G = (int)P.counts.cols, B = n_batches;
    const size_t W = (size_t)G * B;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dc = pool.get<double>(W);
    double* d1 = pool.get<double>(W);
    double* d2 = pool.get<double>(W);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dc, clip, W * sizeof(double), hipMemcpyHostToDevice, st));
    hvg_clipped_sums_batched_kernel<<<(unsigned)((W + 3) / 4), 256, 0, st>>>(P.grouped.ptr, P.grouped.idx, P.grouped.val, G, B,
                                                                            P.gstart, dc, d1, d2);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(c1, d1, W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(c2, d2, W * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}
