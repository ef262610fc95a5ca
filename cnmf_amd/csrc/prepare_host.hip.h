// The O(nnz) passes of the reference's prepare (cnmf.py:333-459) on the device: TPM (cnmf.py:245-251), the per-gene TPM
// moments that feed the high-variance-gene model (cnmf.py:436-447, 126-134) and get_norm_counts' column subset and
// unit-variance scaling (cnmf.py:522-548), over a STAGING copy of the raw cells x all-genes counts (ctx->prep).
//
//   * the counts arrive as CSR with 64-bit row pointers; values are kept in float64 on the device;
//   * per-gene statistics walk the columns: the CSR is transposed on the device by the counting sort of csr_host.hip.h
//     (row chunks in order, one wavefront per chunk, integer counters only), so every column lists its cells in
//     ascending order and a wavefront per gene sums them in the fixed order of kernels_segments.hip.h (lane-strided,
//     one butterfly) -- no float atomics, two calls give the same bits;
//   * the column subset is the same counting sort run the other way over the chosen columns, in list order: the rows of
//     the result list their new columns in ascending order by construction (scipy's canonical CSR), whatever the order
//     of the gene list.
// Included by cnmf_hip.hip (after csr_host.hip.h and normalize_host.hip.h).
#pragma once

namespace cnmf {

__global__ __launch_bounds__(256) void prep_widen_kernel(const float* __restrict__ in, long long n, double* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = (double)in[i];
}

// one wavefront per row: *bad |= 1 (columns not strictly increasing), 2 (column outside [0, C)), 4 (value not finite > 0),
// 8 (value not finite >= 0)
__global__ __launch_bounds__(256) void prep_check_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                         const double* __restrict__ val, int R, int C, int* __restrict__ bad)
{
    const int row = seg_index();
    if (row >= R) return;
    const long long b = ptr[row], e = ptr[row + 1];
    int flag = 0;
    seg_for_each(b, e, [&](long long p) {
        const int c = idx[p];
        if (c < 0 || c >= C) flag |= 2;
        if (p > b && idx[p - 1] >= c) flag |= 1;
        const double v = val[p];
        if (!(v > 0.0) || !isfinite(v)) flag |= 4;
        if (!(v >= 0.0) || !isfinite(v)) flag |= 8;
    });
    if (flag) atomicOr(bad, flag);
}

// one wavefront per row: the float64 sum of the stored values whose column has mask[column] != 0 (mask == nullptr: of
// all of them; idx is read only under a mask), in the order of kernels_segments.hip.h
__global__ __launch_bounds__(256) void prep_row_sums_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                            const double* __restrict__ val, int R,
                                                            const unsigned char* __restrict__ mask, double* __restrict__ out)
{
    const int row = seg_index();
    if (row >= R) return;
    double s = 0.0;
    seg_for_each(ptr[row], ptr[row + 1], [&](long long p) {
        if (mask && !mask[idx[p]]) return;
        s += val[p];
    });
    s = seg_sum(s);
    if (seg_lane() == 0) out[row] = s;
}

// TPM factor of every cell: target / total, 0 for a cell without counts (sc.pp.normalize_total)
__global__ __launch_bounds__(256) void prep_row_scale_kernel(const double* __restrict__ rs, int R, double target,
                                                             double* __restrict__ scale)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < R) scale[i] = rs[i] > 0.0 ? target / rs[i] : 0.0;
}

// the TPM values in CSR order: x * scale[row]
__global__ __launch_bounds__(256) void prep_tpm_values_kernel(const long long* __restrict__ ptr, const double* __restrict__ val,
                                                              int R, const double* __restrict__ scale, double* __restrict__ out)
{
    const int row = seg_index();
    if (row >= R) return;
    const double f = scale ? scale[row] : 1.0;
    seg_for_each(ptr[row], ptr[row + 1], [&](long long p) { out[p] = scale ? val[p] * f : val[p]; });
}

// the images of the selected matrix, a wavefront per row: the float32 dense image (X, leading dimension ld), the float32
// CSR values (v32) and the float64 dense matrix (d64, [R][C]); each may be nullptr
__global__ __launch_bounds__(256) void prep_store_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                         const double* __restrict__ val, int R, int C, int ld,
                                                         float* __restrict__ X, float* __restrict__ v32, double* __restrict__ d64)
{
    const int row = seg_index();
    if (row >= R) return;
    seg_for_each(ptr[row], ptr[row + 1], [&](long long p) {
        const double v = val[p];
        const int c = idx[p];
        if (X) X[(size_t)row * ld + c] = (float)v;
        if (v32) v32[p] = (float)v;
        if (d64) d64[(size_t)row * C + c] = v;
    });
}

}  // namespace cnmf

// The row sums of the staged counts S (*rs) and, when target_sum > 0, normalize_total's factor of every cell (*scale, else
// nullptr): both allocated from `pool`, both launches queued on the stream
static int stage_row_scale(cnmf_ctx* ctx, const CountStage& S, double target_sum, DevPool& pool, double** rs, double** scale)
{
    using namespace cnmf;
    const int N = (int)S.counts.rows;
    *rs = pool.get<double>(N);
    *scale = target_sum > 0.0 ? pool.get<double>(N) : nullptr;
    POOL_TRY(ctx, pool);
    prep_row_sums_kernel<<<seg_grid(N), 256, 0, ctx->stream>>>(S.counts.ptr, S.counts.idx, S.counts.val, N, nullptr, *rs);
    if (*scale) prep_row_scale_kernel<<<(N + 255) / 256, 256, 0, ctx->stream>>>(*rs, N, target_sum, *scale);
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// the transpose of the staging paths: float64 values, at least one row chunk (csr_host.hip.h)
static int prep_transpose(cnmf_ctx* ctx, const DevCsr<double>& in, const int* sel, const double* div, int64_t n_rows,
                          long long expect, DevCsr<double>* out, const double* in_val = nullptr)
{
    return csr_transpose<double>(ctx, in, sel, div, n_rows, 1, expect, "prepare transpose", out, in_val);
}

// the columns of the staged counts (their transpose), built once per upload
static int prep_ensure_columns(cnmf_ctx* ctx)
{
    PrepStage& P = ctx->prep;
    if (P.columns.ptr) return CNMF_OK;
    return prep_transpose(ctx, P.counts, nullptr, nullptr, P.counts.rows, P.counts.nnz, &P.columns);
}

// the host-side checks of a CSR upload (shape, row pointers, null arrays)
static int prep_csr_args(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data, int64_t n_cells,
                         int64_t n_genes)
{
    if (!ctx || !indptr) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (n_cells <= 0 || n_genes <= 0 || n_cells > (1ll << 30) || n_genes > (1ll << 24)) {
        SET_ERR(ctx, "bad matrix shape %lld x %lld", (long long)n_cells, (long long)n_genes);
        return CNMF_EINVAL;
    }
    if (indptr[0] != 0) { SET_ERR(ctx, "indptr[0] must be 0"); return CNMF_EINVAL; }
    for (int64_t i = 0; i < n_cells; ++i)
        if (indptr[i + 1] < indptr[i]) { SET_ERR(ctx, "indptr decreases at row %lld", (long long)i); return CNMF_EINVAL; }
    const int64_t nnz = indptr[n_cells];
    if (nnz > 0 && (!indices || !data)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    return CNMF_OK;
}

// Stages raw counts (checked by prep_csr_args) into S: CSR with float64 values, checked on the device, and with_columns
// their transpose too.  Both are built in locals and committed together at the end: after a failure S is as the caller
// left it (released: nothing staged).  as_stored: the rows may list their (distinct) columns in any order and zeros may be
// stored (cnmf_preprocess_upload_csr_as_stored).
static int stage_counts(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f64,
                        int64_t n_cells, int64_t n_genes, bool as_stored, bool with_columns, CountStage& S)
{
    using namespace cnmf;
    const int64_t nnz = indptr[n_cells];
    hipStream_t st = ctx->stream;
    DevPool pool;
    int* d_bad = pool.get<int>(1, true, st);
    float* tmp32 = data_is_f64 ? nullptr : pool.get<float>((size_t)std::max<int64_t>(nnz, 1));
    POOL_TRY(ctx, pool);
    DevCsrLocal<double> counts, columns;
    HIP_TRY(ctx, counts.alloc_ptr(n_cells, n_genes));
    HIP_TRY(ctx, counts.alloc_entries(nnz));
    HIP_TRY(ctx, hipMemcpyAsync(counts.ptr, indptr, (size_t)(n_cells + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(counts.idx, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, st));
        if (data_is_f64) {
            HIP_TRY(ctx, hipMemcpyAsync(counts.val, data, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(tmp32, data, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, st));
            const long long blocks = std::min<long long>((nnz + 255) / 256, 8192);
            prep_widen_kernel<<<(unsigned)blocks, 256, 0, st>>>(tmp32, nnz, counts.val);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    int bad = 0;
    prep_check_kernel<<<seg_grid(n_cells), 256, 0, st>>>(counts.ptr, counts.idx, counts.val, (int)n_cells, (int)n_genes, d_bad);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (as_stored) bad &= 2 | 8;
    if (bad & 2) { SET_ERR(ctx, "column index out of range in the CSR arrays"); return CNMF_EINVAL; }
    if (bad & 1) { SET_ERR(ctx, "every row must list strictly increasing columns (canonical CSR)"); return CNMF_EINVAL; }
    if (bad & 4) { SET_ERR(ctx, "stored values must be finite and > 0 (counts without stored zeros)"); return CNMF_EINVAL; }
    if (bad & 8) { SET_ERR(ctx, "stored values must be finite and >= 0"); return CNMF_EINVAL; }
    if (with_columns)
        if (int rc = prep_transpose(ctx, counts, nullptr, nullptr, n_cells, nnz, &columns)) return rc;
    S.counts.take(counts);
    S.columns.take(columns);
    return CNMF_OK;
}

// the three copies of a device CSR to the host, queued on the stream (the caller synchronises); a null host array is
// skipped; values_override != nullptr: device values in place of csr.val
template <typename V>
static int csr_fetch(cnmf_ctx* ctx, const DevCsr<V>& csr, int64_t* indptr, int32_t* indices, V* values,
                     const V* values_override = nullptr)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)std::max<int64_t>(csr.nnz, 0);
    if (indptr) HIP_TRY(ctx, hipMemcpyAsync(indptr, csr.ptr, ((size_t)csr.rows + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (indices && n > 0) HIP_TRY(ctx, hipMemcpyAsync(indices, csr.idx, n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (values && n > 0)
        HIP_TRY(ctx, hipMemcpyAsync(values, values_override ? values_override : csr.val, n * sizeof(V), hipMemcpyDeviceToHost, st));
    return CNMF_OK;
}

extern "C" int cnmf_prepare_upload_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                                       int data_is_f64, int64_t n_cells, int64_t n_genes)
{
    if (int rc = prep_csr_args(ctx, indptr, indices, data, n_cells, n_genes)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStreamSynchronize(ctx->stream);
    ctx->prep.release();
    return stage_counts(ctx, indptr, indices, data, data_is_f64, n_cells, n_genes, false, false, ctx->prep);
}

extern "C" int cnmf_prepare_tpm_stats(cnmf_ctx* ctx, double target_sum, double* row_sums, double* mean, double* var,
                                      double* tpm_data)
{
    using namespace cnmf;
    if (!ctx || !row_sums || !mean || !var) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (!P.staged()) { SET_ERR(ctx, "cnmf_prepare_upload_csr has not been called"); return CNMF_ESTATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = (int)P.counts.rows, G = (int)P.counts.cols;
    if (int rc = prep_ensure_columns(ctx)) return rc;
    DevPool pool;
    double *rs, *scale;
    double* m = pool.get<double>(G);
    double* q = pool.get<double>(G);
    double* tv = tpm_data ? pool.get<double>((size_t)std::max<long long>(P.counts.nnz, 1)) : nullptr;
    if (int rc = stage_row_scale(ctx, P, target_sum, pool, &rs, &scale)) return rc;
    col_moments_kernel<double><<<seg_grid(G), 256, 0, st>>>(P.columns.ptr, P.columns.idx, P.columns.val, nullptr, G, N, scale, m, q);
    if (tv) prep_tpm_values_kernel<<<seg_grid(N), 256, 0, st>>>(P.counts.ptr, P.counts.val, N, scale, tv);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, row_sums, rs, (size_t)N));
    HIP_TRY(ctx, dev_fetch(st, mean, m, (size_t)G));
    HIP_TRY(ctx, dev_fetch(st, var, q, (size_t)G));
    if (tv && P.counts.nnz > 0) HIP_TRY(ctx, dev_fetch(st, tpm_data, tv, (size_t)P.counts.nnz));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int g = 0; g < G; ++g) var[g] /= (double)N;
    return CNMF_OK;
}

// the checks of a gene list against the staged counts S, shared by cnmf_prepare_select and cnmf_preprocess_select
static int select_check_genes(cnmf_ctx* ctx, const CountStage& S, int32_t n_sel, const int32_t* genes)
{
    const int N = (int)S.counts.rows, G = (int)S.counts.cols;
    if (n_sel <= 0 || n_sel > G) { SET_ERR(ctx, "n_sel = %d outside [1, %d]", n_sel, G); return CNMF_EINVAL; }
    if (N < 2) { SET_ERR(ctx, "need at least two cells for a variance"); return CNMF_EINVAL; }
    for (int j = 0; j < n_sel; ++j)
        if (genes[j] < 0 || genes[j] >= G) { SET_ERR(ctx, "gene index %d outside [0, %d)", genes[j], G); return CNMF_EINVAL; }
    return CNMF_OK;
}

// The columns genes[0..n_sel) (checked) of the staged counts, scaled to unit variance and transposed back into the rows of
// `out` (cells x n_sel, columns ascending within every row whatever the order of the list): over the column values cval
// (S.columns.val, or a row-scaled copy of it) std_out[j] = the ddof = 1 standard deviation of column genes[j], y = x / std
// -- a column of zero variance (std_out[j] == 0) is left as it is, like sc.pp.scale(zero_center=False); a caller that
// cannot accept one passes zero_std_at: the first such column j ends the call before the transpose with *zero_std_at = j
// and CNMF_EINVAL (the caller words the error).
static int select_scaled_columns(cnmf_ctx* ctx, const CountStage& S, const double* cval, int32_t n_sel, const int32_t* genes,
                                 double* std_out, DevCsr<double>* out, int* zero_std_at = nullptr)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    const int N = (int)S.counts.rows, G = (int)S.counts.cols;
    DevPool pool;
    int* d_genes = pool.put<int>(genes, (size_t)n_sel, st);
    double* m = pool.get<double>(n_sel);
    double* q = pool.get<double>(n_sel);
    double* d_div = pool.get<double>(n_sel);
    POOL_TRY(ctx, pool);
    col_moments_kernel<double><<<seg_grid(n_sel), 256, 0, st>>>(S.columns.ptr, S.columns.idx, cval, d_genes, n_sel, N, nullptr, m, q);
    HIP_TRY(ctx, hipGetLastError());
    // one wait for both read-backs: the column pointers (the stored entries of the chosen columns) and the moments
    std::vector<long long> hc((size_t)G + 1);
    std::vector<double> hq(n_sel), div(n_sel);
    HIP_TRY(ctx, dev_fetch(st, hc.data(), S.columns.ptr, (size_t)G + 1));
    HIP_TRY(ctx, dev_fetch(st, hq.data(), q, (size_t)n_sel));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    long long nnz_sel = 0;
    for (int j = 0; j < n_sel; ++j) {
        nnz_sel += hc[genes[j] + 1] - hc[genes[j]];
        std_out[j] = std::sqrt(hq[j] / (double)(N - 1));
        if (std_out[j] == 0.0 && zero_std_at) { *zero_std_at = j; return CNMF_EINVAL; }
        div[j] = std_out[j] == 0.0 ? 1.0 : std_out[j];
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_div, div.data(), (size_t)n_sel * sizeof(double), hipMemcpyHostToDevice, st));
    return prep_transpose(ctx, S.columns, d_genes, d_div, n_sel, nnz_sel, out, cval);
}

extern "C" int cnmf_prepare_select(cnmf_ctx* ctx, int32_t n_sel, const int32_t* genes, int32_t densify, double* std_out,
                                   double* row_sums_out, int64_t* nnz_out)
{
    using namespace cnmf;
    if (!ctx || !genes || !std_out || !row_sums_out || !nnz_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (!P.staged()) { SET_ERR(ctx, "cnmf_prepare_upload_csr has not been called"); return CNMF_ESTATE; }
    if (int rc = select_check_genes(ctx, P, n_sel, genes)) return rc;
    const int N = (int)P.counts.rows;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = prep_ensure_columns(ctx)) return rc;
    P.release_out();
    // Everything below is formed first; P.out and ctx->csr are published by the last statements of this function, when
    // all of it stands.  A failure before them leaves "no selection to fetch" (P.out.nnz = -1).
    DevCsrLocal<double> out;
    int j0 = -1;
    if (int rc = select_scaled_columns(ctx, P, P.columns.val, n_sel, genes, std_out, &out, densify ? &j0 : nullptr)) {
        if (j0 >= 0) SET_ERR(ctx, "column %d (gene %d) has zero variance: X /= X.std(ddof=1) would leave NaN / inf", j0, genes[j0]);
        return rc;
    }
    const long long nnz_sel = out.nnz;
    DevPool pool;
    double* rs = pool.get<double>(N);
    POOL_TRY(ctx, pool);
    const unsigned rows_grid = seg_grid(N);
    prep_row_sums_kernel<<<rows_grid, 256, 0, st>>>(out.ptr, out.idx, out.val, N, nullptr, rs);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, row_sums_out, rs, (size_t)N));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // The staged counts and their transpose go BEFORE the images of the new resident matrix are allocated (alloc_matrix
    // lets go of the old resident matrix first): the peak is the larger of the two, not their sum.
    P.release_counts();
    // the new resident matrix: the images cnmf_set_matrix / cnmf_set_matrix_csr form from float32(y)
    if (int rc = alloc_matrix(ctx, N, n_sel, densify != 0)) return rc;
    DevCsrLocal<float> img;
    double* odense = nullptr;                // (a local until the commit; freed below if a step after it fails)
    hipError_t e = hipSuccess;
    if (densify) {
        const size_t bytes = (size_t)N * n_sel * sizeof(double);
        HIP_TRY(ctx, hipMalloc((void**)&odense, bytes));
        e = hipMemsetAsync(odense, 0, bytes, st);
        prep_store_kernel<<<rows_grid, 256, 0, st>>>(out.ptr, out.idx, out.val, N, n_sel, ctx->G_pad, ctx->X, nullptr, odense);
    } else {
        HIP_TRY(ctx, img.alloc_ptr(N, n_sel));
        HIP_TRY(ctx, img.alloc_entries(nnz_sel));
        HIP_TRY(ctx, hipMemcpyAsync(img.ptr, out.ptr, ((size_t)N + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st));
        if (nnz_sel > 0) HIP_TRY(ctx, hipMemcpyAsync(img.idx, out.idx, (size_t)nnz_sel * sizeof(int), hipMemcpyDeviceToDevice, st));
        prep_store_kernel<<<rows_grid, 256, 0, st>>>(out.ptr, out.idx, out.val, N, n_sel, 0, nullptr, img.val, nullptr);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) hipFree(odense);
    HIP_TRY(ctx, e);
    P.odense = odense; P.out_dense = densify ? 1 : 0;
    P.out.take(out);
    if (!densify) ctx->csr.take(img);
    *nnz_out = nnz_sel;
    return CNMF_OK;
}

extern "C" int cnmf_prepare_fetch(cnmf_ctx* ctx, int64_t* indptr, int32_t* indices, double* values)
{
    if (!ctx || !values) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (P.out.nnz < 0) { SET_ERR(ctx, "cnmf_prepare_select has not been called"); return CNMF_ESTATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (P.out_dense) {
        const size_t bytes = (size_t)P.out.rows * (size_t)P.out.cols * sizeof(double);
        HIP_TRY(ctx, hipMemcpyAsync(values, P.odense, bytes, hipMemcpyDeviceToHost, st));
    } else {
        if (!indptr || (!indices && P.out.nnz > 0)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
        if (int rc = csr_fetch<double>(ctx, P.out, indptr, indices, values)) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    P.release_out();
    return CNMF_OK;
}

extern "C" int cnmf_prepare_release(cnmf_ctx* ctx)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->prep.release();
    return CNMF_OK;
}
