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
//   * the kernels are the one-batch kernels of hvg_host.hip.h, handed the run starts: one wavefront per (batch, gene)
//     pair w = b G + g, the genes on grid.x and the batches on grid.y.  Two binary searches over the rows of column g,
//     uniform over the wavefront, find the run (seg_row_run, kernels_segments.hip.h); the lanes stride it FROM ITS FIRST
//     ENTRY and reduce with the same butterfly.  The additions of a pair are therefore the very sequence the one-batch
//     call performs on the staging restricted to the cells of b (cnmf_preprocess_subset keeps the stored order): the
//     float64 sums have those bits.  An empty run gives zeros.
//
// Limits, checked on the host before anything is launched: at most HVG_CELLS_MAX cells in all (as for one batch), at most
// HVG_BATCHES_MAX = 4096 batches (grid.y), none of them empty, and at most HVG_PAIRS_MAX = 2^26 (batch, gene) pairs: the
// [B][G] buffers then hold at most 512 MB each.
// Integer counters and fixed-order float64 sums only (the order: kernels_segments.hip.h) -- no float atomics: two calls
// give the same bits.
// Included by cnmf_hip.hip (after hvg_host.hip.h).
#pragma once

namespace cnmf {

constexpr int HVG_BATCHES_MAX = 4096;
constexpr long long HVG_PAIRS_MAX = 1ll << 26;

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
    const PreStage& P = ctx->pre;
    return hvg_gene_moments(ctx, P.grouped, n_batches, P.gstart, s1, s2, flags);
}

extern "C" int cnmf_preprocess_clipped_sums_batched(cnmf_ctx* ctx, const int32_t* codes, int32_t n_batches, const double* clip,
                                                    double* c1, double* c2)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!codes || !clip || !c1 || !c2) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = hvg_ensure_grouped(ctx, "clipped_sums_batched", codes, n_batches)) return rc;
    const PreStage& P = ctx->pre;
    return hvg_clipped_sums(ctx, P.grouped, n_batches, P.gstart, clip, c1, c2);
}
