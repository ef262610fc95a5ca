// The O(nnz) passes of the reference's Preprocess.filter_adata (preprocess.py:60-132) and of the head of
// Preprocess.preprocess_for_cnmf (:210-243) on the staging of preprocess_host.hip.h (ctx->pre: the raw counts as CSR and
// as their transpose, float64 values, 64-bit row pointers):
//
//   * per-gene detection counts (value > 0; a stored zero is no detection) and totals walk the transpose, a wavefront per
//     column (sc.pp.filter_genes, the mitochondrial share); per-cell sums over a gene mask are prep_row_sums_kernel
//     with that mask (n_counts, the mitochondrial totals) -- with no mask they ARE cnmf_preprocess_row_sums, one body;
//   * the restriction of the staging to a subset of cells and genes never leaves the device: the kept entries of every
//     kept row are counted, an exclusive scan (FLT_SCAN_BLOCK items per workgroup: block sums, a scan of the block sums,
//     the blocks again) makes the new row pointers and the old -> new maps of rows and columns, and a wavefront per row
//     compacts its entries 64 at a time (a 64-bit ballot of "gene kept", the population count of the lower lanes as the
//     offset, a running offset from step to step): the kept entries keep their stored order, stored zeros stay;
//   * the staged CSR comes back raw or library-size normalised (x * scale[row], the scale of prep_row_scale_kernel: the
//     product cnmf_preprocess_select forms, bit for bit).
//
// Integer counters and fixed-order float64 sums only (the order: kernels_segments.hip.h) -- no float atomics: two calls on
// the same input give the same bits.
// Included by cnmf_hip.hip (after preprocess_host.hip.h).
#pragma once

namespace cnmf {

constexpr int FLT_SCAN_ITEMS = 4;                        // consecutive items per thread
constexpr int FLT_SCAN_BLOCK = 256 * FLT_SCAN_ITEMS;     // items one scan workgroup covers

// one wavefront per column g of the transposed counts: n_cells[g] = stored entries > 0, totals[g] = their sum, over the
// cells with mask[cell] != 0 (mask == nullptr: all cells), in the order of kernels_segments.hip.h
__global__ __launch_bounds__(256) void flt_gene_detect_kernel(const long long* __restrict__ cptr, const int* __restrict__ crow,
                                                              const double* __restrict__ cval, int G,
                                                              const unsigned char* __restrict__ mask,
                                                              long long* __restrict__ n_cells, double* __restrict__ totals)
{
    const int g = seg_index();
    if (g >= G) return;
    int n = 0;
    double s = 0.0;
    seg_for_each(cptr[g], cptr[g + 1], [&](long long p) {
        if (mask && !mask[crow[p]]) return;
        const double v = cval[p];
        n += v > 0.0 ? 1 : 0;
        s += v;
    });
    n = seg_sum(n);
    s = seg_sum(s);
    if (seg_lane() == 0) { n_cells[g] = n; totals[g] = s; }
}

// ---------------------------------------------------------------- exclusive scan over n items, 64-bit sums
// exclusive scan of one value per thread over the 256 threads of a workgroup; *total = the workgroup's sum
__device__ __forceinline__ long long flt_block_scan(long long v, long long* total)
{
    __shared__ long long ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    long long base = 0;
    for (int w = 0; w < wave; ++w) base += ws[w];
    *total = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    __syncthreads();                                     // (ws is free for the next call)
    return base + inc - v;
}

template <typename T>
__device__ __forceinline__ long long flt_item(const T* in, long long i, long long n)
{
    return i < n ? (long long)(in[i] != 0 ? (sizeof(T) == 1 ? 1 : in[i]) : 0) : 0;   // (a mask byte counts as 0 or 1)
}

// pass 1: bsum[b] = sum of the items of workgroup b
template <typename T>
__global__ __launch_bounds__(256) void flt_scan_sums_kernel(const T* in, long long n, long long* __restrict__ bsum)
{
    const long long i0 = (long long)blockIdx.x * FLT_SCAN_BLOCK + (long long)threadIdx.x * FLT_SCAN_ITEMS;
    long long v = 0;
#pragma unroll
    for (int k = 0; k < FLT_SCAN_ITEMS; ++k) v += flt_item(in, i0 + k, n);
    long long total = 0;
    flt_block_scan(v, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// pass 2: bsum := its exclusive scan, one workgroup walking it 256 at a time with a carry
__global__ __launch_bounds__(256) void flt_scan_blocks_kernel(long long* __restrict__ bsum, long long nb)
{
    long long carry = 0;
    for (long long i0 = 0; i0 < nb; i0 += 256) {
        const long long i = i0 + threadIdx.x;
        const long long v = i < nb ? bsum[i] : 0;
        long long total = 0;
        const long long ex = flt_block_scan(v, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
}

// pass 3: out[i] = sum of the items before i, out[n] = the sum of all (out may be in: every thread reads its items first)
template <typename T>
__global__ __launch_bounds__(256) void flt_scan_write_kernel(const T* in, long long n, const long long* __restrict__ bsum,
                                                             long long* out)
{
    const long long i0 = (long long)blockIdx.x * FLT_SCAN_BLOCK + (long long)threadIdx.x * FLT_SCAN_ITEMS;
    long long item[FLT_SCAN_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < FLT_SCAN_ITEMS; ++k) { item[k] = flt_item(in, i0 + k, n); v += item[k]; }
    long long total = 0;
    long long run = flt_block_scan(v, &total) + bsum[blockIdx.x];
    if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
#pragma unroll
    for (int k = 0; k < FLT_SCAN_ITEMS; ++k) {
        const long long i = i0 + k;
        if (i < n) out[i] = run;
        run += item[k];
        if (i == n - 1) out[n] = run;
    }
}

// ---------------------------------------------------------------- the restriction to kept cells and genes
// one wavefront per row: cnt[new row] = its entries whose gene is kept; rowmap [R + 1] (the scan of keep_rows) names the
// new row, keep_rows == nullptr: every row stays where it is
__global__ __launch_bounds__(256) void flt_row_count_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                            int R, const unsigned char* __restrict__ keep_rows,
                                                            const long long* __restrict__ rowmap,
                                                            const unsigned char* __restrict__ keep_cols, long long R_new,
                                                            long long* __restrict__ cnt)
{
    const int row = seg_index();
    if (row >= R || (keep_rows && !keep_rows[row])) return;
    const long long nr = keep_rows ? rowmap[row] : row;
    if (nr < 0 || nr >= R_new) return;
    int n = 0;
    seg_for_each(ptr[row], ptr[row + 1], [&](long long p) { n += (!keep_cols || keep_cols[idx[p]]) ? 1 : 0; });
    n = seg_sum(n);
    if (seg_lane() == 0) cnt[nr] = n;
}

// one wavefront per row compacts it in stored order: every step of 64 entries takes the ballot of "gene kept", an entry's
// place is the row's running offset plus the kept entries in the lower lanes; colmap [C + 1] (the scan of keep_cols) names
// the new column
__global__ __launch_bounds__(256) void flt_compact_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                          const double* __restrict__ val, int R, int C,
                                                          const unsigned char* __restrict__ keep_rows,
                                                          const long long* __restrict__ rowmap,
                                                          const unsigned char* __restrict__ keep_cols,
                                                          const long long* __restrict__ colmap, long long R_new,
                                                          const long long* __restrict__ nptr, int* __restrict__ nidx,
                                                          double* __restrict__ nval)
{
    const int row = seg_index(), lane = seg_lane();
    if (row >= R || (keep_rows && !keep_rows[row])) return;
    const long long nr = keep_rows ? rowmap[row] : row;
    if (nr < 0 || nr >= R_new) return;
    const long long b = ptr[row], e = ptr[row + 1], end = nptr[nr + 1];
    long long base = nptr[nr];
    for (long long p0 = b; p0 < e; p0 += 64) {           // (uniform over the wavefront: every lane takes every ballot)
        const long long p = p0 + lane;
        const int c = p < e ? idx[p] : -1;
        const bool keep = c >= 0 && c < C && (!keep_cols || keep_cols[c]);
        const unsigned long long kept = __ballot(keep);
        if (keep) {
            const long long q = base + __popcll(kept & ((1ull << lane) - 1ull));
            if (q < end) { nidx[q] = keep_cols ? (int)colmap[c] : c; nval[q] = val[p]; }
        }
        base += __popcll(kept);
    }
}

}  // namespace cnmf

// out [n + 1] (device) := the exclusive scan of in [n] (device; out may be in), on the device; bsum: scratch of
// flt_scan_blocks(n) 64-bit words
static long long flt_scan_blocks(long long n) { return std::max<long long>(1, (n + cnmf::FLT_SCAN_BLOCK - 1) / cnmf::FLT_SCAN_BLOCK); }

template <typename T>
static void flt_scan(hipStream_t st, const T* in, long long n, long long* bsum, long long* out)
{
    using namespace cnmf;
    const long long nb = flt_scan_blocks(n);
    flt_scan_sums_kernel<T><<<(unsigned)nb, 256, 0, st>>>(in, n, bsum);
    flt_scan_blocks_kernel<<<1, 256, 0, st>>>(bsum, nb);
    flt_scan_write_kernel<T><<<(unsigned)nb, 256, 0, st>>>(in, n, bsum, out);
}

static int flt_staged(cnmf_ctx* ctx)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (!ctx->pre.staged()) { SET_ERR(ctx, "cnmf_preprocess_upload_csr has not been called"); return CNMF_ESTATE; }
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_upload_csr_as_stored(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                                                    const double* data, int64_t n_cells, int64_t n_genes)
{
    if (int rc = prep_csr_args(ctx, indptr, indices, data, n_cells, n_genes)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PreStage& P = ctx->pre;
    hipStreamSynchronize(ctx->stream);
    P.release();
    if (int rc = stage_counts(ctx, indptr, indices, data, 1, n_cells, n_genes, true, true, P)) return rc;
    P.N = n_cells;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_gene_detect(cnmf_ctx* ctx, const uint8_t* cell_mask, int64_t* n_cells, double* totals)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!n_cells || !totals) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    const int N = (int)P.N, G = (int)P.counts.cols;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    unsigned char* dm = cell_mask ? pool.put<unsigned char>(cell_mask, (size_t)N, st) : nullptr;
    long long* dn = pool.get<long long>((size_t)G);
    double* dt = pool.get<double>((size_t)G);
    POOL_TRY(ctx, pool);
    flt_gene_detect_kernel<<<seg_grid(G), 256, 0, st>>>(P.columns.ptr, P.columns.idx, P.columns.val, G, dm, dn, dt);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, n_cells, dn, (size_t)G));
    HIP_TRY(ctx, dev_fetch(st, totals, dt, (size_t)G));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

// the one body of cnmf_preprocess_cell_sums and cnmf_preprocess_row_sums (select_mi_host.hip.h: no mask)
static int pre_cell_sums(cnmf_ctx* ctx, const uint8_t* gene_mask, double* sums)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!sums) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    const int N = (int)P.N, G = (int)P.counts.cols;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    unsigned char* dm = gene_mask ? pool.put<unsigned char>(gene_mask, (size_t)G, st) : nullptr;
    double* ds = pool.get<double>((size_t)N);
    POOL_TRY(ctx, pool);
    prep_row_sums_kernel<<<seg_grid(N), 256, 0, st>>>(P.counts.ptr, P.counts.idx, P.counts.val, N, dm, ds);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, sums, ds, (size_t)N));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_cell_sums(cnmf_ctx* ctx, const uint8_t* gene_mask, double* sums)
{
    return pre_cell_sums(ctx, gene_mask, sums);
}

extern "C" int cnmf_preprocess_subset(cnmf_ctx* ctx, const uint8_t* keep_cells, const uint8_t* keep_genes,
                                      int64_t* n_cells_out, int64_t* n_genes_out, int64_t* nnz_out)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!n_cells_out || !n_genes_out || !nnz_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    const int N = (int)P.N, G = (int)P.counts.cols;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    unsigned char* dkc = keep_cells ? pool.put<unsigned char>(keep_cells, (size_t)N, st) : nullptr;
    unsigned char* dkg = keep_genes ? pool.put<unsigned char>(keep_genes, (size_t)G, st) : nullptr;
    long long* rowmap = keep_cells ? pool.get<long long>((size_t)N + 1) : nullptr;
    long long* colmap = keep_genes ? pool.get<long long>((size_t)G + 1) : nullptr;
    long long* bsum = pool.get<long long>((size_t)flt_scan_blocks(std::max(N, G)));
    POOL_TRY(ctx, pool);
    long long Nn = N, Gn = G;
    if (dkc) {
        flt_scan<unsigned char>(st, dkc, N, bsum, rowmap);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&Nn, rowmap + N, sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    if (dkg) {
        flt_scan<unsigned char>(st, dkg, G, bsum, colmap);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&Gn, colmap + G, sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (Nn <= 0) { SET_ERR(ctx, "keep_cells keeps no cell"); return CNMF_EINVAL; }
    if (Gn <= 0) { SET_ERR(ctx, "keep_genes keeps no gene"); return CNMF_EINVAL; }
    // the new arrays first: the old staging stays as it is until every one of them stands
    const DevCsr<double>& old = P.counts;
    DevCsrLocal<double> counts, columns;
    long long nnz = 0;
    HIP_TRY(ctx, counts.alloc_ptr(Nn, Gn));
    flt_row_count_kernel<<<seg_grid(N), 256, 0, st>>>(old.ptr, old.idx, N, dkc, rowmap, dkg, Nn, counts.ptr);
    flt_scan<long long>(st, counts.ptr, Nn, bsum, counts.ptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&nnz, counts.ptr + Nn, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nnz < 0 || nnz > old.nnz) {
        SET_ERR(ctx, "subset: %lld entries counted of %lld staged", nnz, (long long)old.nnz);
        return CNMF_EHIP;
    }
    HIP_TRY(ctx, counts.alloc_entries(nnz));
    flt_compact_kernel<<<seg_grid(N), 256, 0, st>>>(old.ptr, old.idx, old.val, N, G, dkc, rowmap, dkg, colmap, Nn, counts.ptr,
                                                    counts.idx, counts.val);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (int rc = prep_transpose(ctx, counts, nullptr, nullptr, Nn, nnz, &columns)) return rc;
    // the slots and the ridge factors spoke of the old cells and genes
    P.release();
    P.counts.take(counts);
    P.columns.take(columns);
    P.N = Nn;
    *n_cells_out = Nn; *n_genes_out = Gn; *nnz_out = nnz;
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_fetch_counts(cnmf_ctx* ctx, double target_sum, int64_t* indptr, int32_t* indices, double* values)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!(target_sum >= 0.0) || !std::isfinite(target_sum)) { SET_ERR(ctx, "target_sum must be finite and >= 0"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    const int N = (int)P.N;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* sval = nullptr;
    if (target_sum > 0.0 && values && P.counts.nnz > 0) {
        double *rs, *scale;
        sval = pool.get<double>((size_t)P.counts.nnz);
        if (int rc = stage_row_scale(ctx, P, target_sum, pool, &rs, &scale)) return rc;
        prep_tpm_values_kernel<<<seg_grid(N), 256, 0, st>>>(P.counts.ptr, P.counts.val, N, scale, sval);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (int rc = csr_fetch<double>(ctx, P.counts, indptr, indices, values, sval)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}
