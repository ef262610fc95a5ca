// The O(nnz) passes of the reference's prepare (cnmf.py:333-459) on the device: TPM (cnmf.py:245-251), the per-gene TPM
// moments that feed the high-variance-gene model (cnmf.py:436-447, 126-134) and get_norm_counts' column subset and
// unit-variance scaling (cnmf.py:522-548), over a STAGING copy of the raw cells x all-genes counts (ctx->prep).
//
//   * the counts arrive as CSR with 64-bit row pointers; values are kept in float64 on the device;
//   * per-gene statistics walk the columns: the CSR is transposed on the device by the counting sort of csr_host.hip.h
//     (row chunks in order, one wavefront per chunk, integer counters only), so every column lists its cells in
//     ascending order and a wavefront per gene sums them lane-strided with a fixed butterfly -- no float atomics, two
//     calls give the same bits;
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
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const long long b = ptr[row], e = ptr[row + 1];
    int flag = 0;
    for (long long p = b + lane; p < e; p += 64) {
        const int c = idx[p];
        if (c < 0 || c >= C) flag |= 2;
        if (p > b && idx[p - 1] >= c) flag |= 1;
        const double v = val[p];
        if (!(v > 0.0) || !isfinite(v)) flag |= 4;
        if (!(v >= 0.0) || !isfinite(v)) flag |= 8;
    }
    if (flag) atomicOr(bad, flag);
}

// one wavefront per row: float64 sum of the stored values (lane-strided, fixed butterfly order)
__global__ __launch_bounds__(256) void prep_row_sums_kernel(const long long* __restrict__ ptr, const double* __restrict__ val,
                                                            int R, double* __restrict__ out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    double s = 0.0;
    for (long long p = ptr[row] + lane; p < ptr[row + 1]; p += 64) s += val[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = s;
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
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const double f = scale ? scale[row] : 1.0;
    for (long long p = ptr[row] + lane; p < ptr[row + 1]; p += 64) out[p] = scale ? val[p] * f : val[p];
}

// Per-column moments over the transposed counts, a wavefront per output column j (gene sel[j], or j): with
// v = x * scale[cell] (scale == nullptr: v = x), mean[j] = sum v / N and ssd[j] = sum over ALL N cells of (v - mean)^2
// = sum_stored (v - mean)^2 + (N - stored) mean^2.  Two passes, float64, fixed order.
__global__ __launch_bounds__(256) void prep_col_moments_kernel(const long long* __restrict__ cptr, const int* __restrict__ crow,
                                                               const double* __restrict__ cval, const int* __restrict__ sel,
                                                               int n_out, int N, const double* __restrict__ scale,
                                                               double* __restrict__ mean, double* __restrict__ ssd)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n_out) return;
    const int g = sel ? sel[j] : j;
    const long long b = cptr[g], e = cptr[g + 1];
    double s = 0.0;
    for (long long p = b + lane; p < e; p += 64) s += scale ? cval[p] * scale[crow[p]] : cval[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const double mu = s / (double)N;
    double q = 0.0;
    for (long long p = b + lane; p < e; p += 64) {
        const double d = (scale ? cval[p] * scale[crow[p]] : cval[p]) - mu;
        q += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    if (lane == 0) { mean[j] = mu; ssd[j] = q + (double)(N - (e - b)) * mu * mu; }
}

// the images of the selected matrix, a wavefront per row: the float32 dense image (X, leading dimension ld), the float32
// CSR values (v32) and the float64 dense matrix (d64, [R][C]); each may be nullptr
__global__ __launch_bounds__(256) void prep_store_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                         const double* __restrict__ val, int R, int C, int ld,
                                                         float* __restrict__ X, float* __restrict__ v32, double* __restrict__ d64)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    for (long long p = ptr[row] + lane; p < ptr[row + 1]; p += 64) {
        const double v = val[p];
        const int c = idx[p];
        if (X) X[(size_t)row * ld + c] = (float)v;
        if (v32) v32[p] = (float)v;
        if (d64) d64[(size_t)row * C + c] = v;
    }
}

}  // namespace cnmf

// rows per chunk of a transpose of an R x C CSR: as many chunks as keep the T x C counters at <= 64 M ints, at most 4096
static int prep_chunks(int64_t R, int64_t C, int* rows_per_chunk)
{
    int64_t T = std::min<int64_t>(4096, std::max<int64_t>(1, (64ll << 20) / std::max<int64_t>(1, C)));
    T = std::max<int64_t>(1, std::min<int64_t>(T, R));
    const int rpc = (int)((R + T - 1) / T);
    *rows_per_chunk = rpc;
    return (int)((R + rpc - 1) / rpc);
}

// Counting-sort transpose (csr_host.hip.h's kernels) of the R x C CSR (ptr, idx, val), restricted to the rows sel[0..R)
// when sel != nullptr, values divided by div[r] when div != nullptr, into freshly allocated (tptr [C + 1], tidx, tval);
// `expect` (>= 0): the entries that must arrive.
static int prep_transpose(cnmf_ctx* ctx, const long long* ptr, const int* idx, const double* val, const int* sel,
                          const double* div, int R, int C, long long expect, long long** tptr_out, int** tidx_out,
                          double** tval_out)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    int rpc = 1;
    const int T = prep_chunks(R, C, &rpc);
    DevPool pool;
    int* cnt = pool.get<int>((size_t)T * C, true, st);
    POOL_TRY(ctx, pool);
    long long* tptr = nullptr;
    int* tidx = nullptr;
    double* tval = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&tptr, ((size_t)C + 1) * sizeof(long long)));
    csr_tr_hist_kernel<<<T, 256, 0, st>>>(ptr, idx, sel, R, C, rpc, cnt);
    csr_tr_total_kernel<<<(C + 255) / 256, 256, 0, st>>>(cnt, T, C, tptr);
    csr_tr_offsets_kernel<<<(C + 255) / 256, 256, 0, st>>>(cnt, T, C);
    long long total = 0;
    int rc = hipGetLastError() == hipSuccess ? csr_scan_to_ptr(ctx, tptr, (size_t)C, &total) : CNMF_EHIP;
    hipError_t e = hipSuccess;
    if (!rc && expect >= 0 && total != expect) {
        SET_ERR(ctx, "prepare transpose: %lld of %lld entries counted", total, expect);
        rc = CNMF_EHIP;
    }
    if (!rc) e = hipMalloc((void**)&tidx, (size_t)std::max<long long>(total, 1) * sizeof(int));
    if (!rc && e == hipSuccess) e = hipMalloc((void**)&tval, (size_t)std::max<long long>(total, 1) * sizeof(double));
    if (!rc && e == hipSuccess) {
        csr_tr_fill_kernel<double><<<T, 64, 0, st>>>(ptr, idx, val, sel, div, R, C, rpc, cnt, tptr, tidx, tval);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (rc || e != hipSuccess) {
        hipFree(tptr); hipFree(tidx); hipFree(tval);
        if (rc) return rc;
        HIP_TRY(ctx, e);
    }
    *tptr_out = tptr; *tidx_out = tidx; *tval_out = tval;
    return CNMF_OK;
}

// the columns of the staged counts (their transpose), built once per upload
static int prep_ensure_columns(cnmf_ctx* ctx)
{
    PrepStage& P = ctx->prep;
    if (P.cptr) return CNMF_OK;
    return prep_transpose(ctx, P.ptr, P.idx, P.val, nullptr, nullptr, (int)P.N, (int)P.G, P.nnz, &P.cptr, &P.crow, &P.cval);
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

// stages raw counts (checked by prep_csr_args) as CSR with float64 values into freshly allocated (*ptr_out, *idx_out,
// *val_out); frees them again on any failure.  Shared by cnmf_prepare_upload_csr and cnmf_preprocess_upload_csr.
// as_stored: the rows may list their (distinct) columns in any order and zeros may be stored
// (cnmf_preprocess_upload_csr_as_stored).
static int prep_stage_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data, int data_is_f64,
                          int64_t n_cells, int64_t n_genes, long long** ptr_out, int** idx_out, double** val_out,
                          bool as_stored = false)
{
    using namespace cnmf;
    const int64_t nnz = indptr[n_cells];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n1 = (size_t)std::max<int64_t>(nnz, 1);
    DevPool pool;
    int* d_bad = pool.get<int>(1, true, st);
    float* tmp32 = data_is_f64 ? nullptr : pool.get<float>(n1);
    POOL_TRY(ctx, pool);
    long long* ptr = nullptr;
    int* idx = nullptr;
    double* val = nullptr;
    hipError_t e = hipMalloc((void**)&ptr, (size_t)(n_cells + 1) * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&idx, n1 * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&val, n1 * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(ptr, indptr, (size_t)(n_cells + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(idx, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nnz > 0) {
        if (data_is_f64) {
            e = hipMemcpyAsync(val, data, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st);
        } else {
            e = hipMemcpyAsync(tmp32, data, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) {
                const long long blocks = std::min<long long>((nnz + 255) / 256, 8192);
                prep_widen_kernel<<<(unsigned)blocks, 256, 0, st>>>(tmp32, nnz, val);
                e = hipGetLastError();
            }
        }
    }
    int bad = 0;
    if (e == hipSuccess) {
        prep_check_kernel<<<(unsigned)((n_cells + 3) / 4), 256, 0, st>>>(ptr, idx, val, (int)n_cells, (int)n_genes, d_bad);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (as_stored) bad &= 2 | 8;
    if (e != hipSuccess || bad) { hipFree(ptr); hipFree(idx); hipFree(val); }
    HIP_TRY(ctx, e);
    if (bad & 2) { SET_ERR(ctx, "column index out of range in the CSR arrays"); return CNMF_EINVAL; }
    if (bad & 1) { SET_ERR(ctx, "every row must list strictly increasing columns (canonical CSR)"); return CNMF_EINVAL; }
    if (bad & 4) { SET_ERR(ctx, "stored values must be finite and > 0 (counts without stored zeros)"); return CNMF_EINVAL; }
    if (bad & 8) { SET_ERR(ctx, "stored values must be finite and >= 0"); return CNMF_EINVAL; }
    *ptr_out = ptr; *idx_out = idx; *val_out = val;
    return CNMF_OK;
}

extern "C" int cnmf_prepare_upload_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                                       int data_is_f64, int64_t n_cells, int64_t n_genes)
{
    if (int rc = prep_csr_args(ctx, indptr, indices, data, n_cells, n_genes)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PrepStage& P = ctx->prep;
    hipStreamSynchronize(ctx->stream);
    P.release();
    if (int rc = prep_stage_csr(ctx, indptr, indices, data, data_is_f64, n_cells, n_genes, &P.ptr, &P.idx, &P.val)) return rc;
    P.N = n_cells; P.G = n_genes; P.nnz = indptr[n_cells];
    return CNMF_OK;
}

extern "C" int cnmf_prepare_tpm_stats(cnmf_ctx* ctx, double target_sum, double* row_sums, double* mean, double* var,
                                      double* tpm_data)
{
    using namespace cnmf;
    if (!ctx || !row_sums || !mean || !var) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (P.nnz < 0) { SET_ERR(ctx, "cnmf_prepare_upload_csr has not been called"); return CNMF_ESTATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = (int)P.N, G = (int)P.G;
    if (int rc = prep_ensure_columns(ctx)) return rc;
    DevPool pool;
    double* rs = pool.get<double>(N);
    double* scale = target_sum > 0.0 ? pool.get<double>(N) : nullptr;
    double* m = pool.get<double>(G);
    double* q = pool.get<double>(G);
    double* tv = tpm_data ? pool.get<double>((size_t)std::max<long long>(P.nnz, 1)) : nullptr;
    POOL_TRY(ctx, pool);
    prep_row_sums_kernel<<<(N + 3) / 4, 256, 0, st>>>(P.ptr, P.val, N, rs);
    if (scale) prep_row_scale_kernel<<<(N + 255) / 256, 256, 0, st>>>(rs, N, target_sum, scale);
    prep_col_moments_kernel<<<(G + 3) / 4, 256, 0, st>>>(P.cptr, P.crow, P.cval, nullptr, G, N, scale, m, q);
    if (tv) prep_tpm_values_kernel<<<(N + 3) / 4, 256, 0, st>>>(P.ptr, P.val, N, scale, tv);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(row_sums, rs, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(mean, m, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(var, q, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
    if (tv && P.nnz > 0)
        HIP_TRY(ctx, hipMemcpyAsync(tpm_data, tv, (size_t)P.nnz * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int g = 0; g < G; ++g) var[g] /= (double)N;
    return CNMF_OK;
}

extern "C" int cnmf_prepare_select(cnmf_ctx* ctx, int32_t n_sel, const int32_t* genes, int32_t densify, double* std_out,
                                   double* row_sums_out, int64_t* nnz_out)
{
    using namespace cnmf;
    if (!ctx || !genes || !std_out || !row_sums_out || !nnz_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (P.nnz < 0) { SET_ERR(ctx, "cnmf_prepare_upload_csr has not been called"); return CNMF_ESTATE; }
    const int N = (int)P.N, G = (int)P.G;
    if (n_sel <= 0 || n_sel > G) { SET_ERR(ctx, "n_sel = %d outside [1, %d]", n_sel, G); return CNMF_EINVAL; }
    if (N < 2) { SET_ERR(ctx, "need at least two cells for a variance"); return CNMF_EINVAL; }
    for (int j = 0; j < n_sel; ++j)
        if (genes[j] < 0 || genes[j] >= G) { SET_ERR(ctx, "gene index %d outside [0, %d)", genes[j], G); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = prep_ensure_columns(ctx)) return rc;
    P.release_out();
    // the stored entries of the chosen columns
    std::vector<long long> hc((size_t)G + 1);
    HIP_TRY(ctx, hipMemcpyAsync(hc.data(), P.cptr, ((size_t)G + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    long long nnz_sel = 0;
    for (int j = 0; j < n_sel; ++j) nnz_sel += hc[genes[j] + 1] - hc[genes[j]];
    DevPool pool;
    int* d_genes = pool.get<int>(n_sel);
    double* m = pool.get<double>(n_sel);
    double* q = pool.get<double>(n_sel);
    double* d_div = pool.get<double>(n_sel);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(d_genes, genes, (size_t)n_sel * sizeof(int), hipMemcpyHostToDevice, st));
    prep_col_moments_kernel<<<(n_sel + 3) / 4, 256, 0, st>>>(P.cptr, P.crow, P.cval, d_genes, n_sel, N, nullptr, m, q);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> hq(n_sel), div(n_sel);
    HIP_TRY(ctx, hipMemcpyAsync(hq.data(), q, (size_t)n_sel * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int j = 0; j < n_sel; ++j) {
        std_out[j] = std::sqrt(hq[j] / (double)(N - 1));
        if (std_out[j] == 0.0 && densify) {
            SET_ERR(ctx, "column %d (gene %d) has zero variance: X /= X.std(ddof=1) would leave NaN / inf", j, genes[j]);
            return CNMF_EINVAL;
        }
        div[j] = std_out[j] == 0.0 ? 1.0 : std_out[j];        // sc.pp.scale(zero_center=False) leaves such a column as is
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_div, div.data(), (size_t)n_sel * sizeof(double), hipMemcpyHostToDevice, st));
    // rows of the result = the chosen columns of the counts in list order, transposed back: y = x / div, CSR, columns
    // ascending within every row
    long long* optr = nullptr;
    int* oidx = nullptr;
    double* oval = nullptr;
    if (int rc = prep_transpose(ctx, P.cptr, P.crow, P.cval, d_genes, d_div, n_sel, N, nnz_sel, &optr, &oidx, &oval)) return rc;
    P.optr = optr; P.oidx = oidx; P.oval = oval; P.out_nnz = nnz_sel; P.out_n = n_sel; P.out_dense = densify ? 1 : 0;
    double* rs = pool.get<double>(N);
    POOL_TRY(ctx, pool);
    prep_row_sums_kernel<<<(N + 3) / 4, 256, 0, st>>>(P.optr, P.oval, N, rs);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(row_sums_out, rs, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    P.release_counts();                      // (the staging counts are done with)
    // the new resident matrix: the images cnmf_set_matrix / cnmf_set_matrix_csr form from float32(y)
    if (int rc = alloc_matrix(ctx, N, n_sel, densify != 0)) return rc;
    const unsigned rows_grid = (unsigned)((N + 3) / 4);
    if (densify) {
        HIP_TRY(ctx, hipMalloc((void**)&P.odense, (size_t)N * n_sel * sizeof(double)));
        HIP_TRY(ctx, hipMemsetAsync(P.odense, 0, (size_t)N * n_sel * sizeof(double), st));
        prep_store_kernel<<<rows_grid, 256, 0, st>>>(P.optr, P.oidx, P.oval, N, n_sel, ctx->G_pad, ctx->X, nullptr, P.odense);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        const size_t n1 = (size_t)std::max<long long>(nnz_sel, 1);
        long long* cp = nullptr;
        int* ci = nullptr;
        float* cv = nullptr;
        hipError_t e = hipMalloc((void**)&cp, ((size_t)N + 1) * sizeof(long long));
        if (e == hipSuccess) e = hipMalloc((void**)&ci, n1 * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&cv, n1 * sizeof(float));
        if (e == hipSuccess) e = hipMemcpyAsync(cp, P.optr, ((size_t)N + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && nnz_sel > 0) e = hipMemcpyAsync(ci, P.oidx, (size_t)nnz_sel * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) {
            prep_store_kernel<<<rows_grid, 256, 0, st>>>(P.optr, P.oidx, P.oval, N, n_sel, 0, nullptr, cv, nullptr);
            e = hipGetLastError();
        }
        if (e != hipSuccess) { hipFree(cp); hipFree(ci); hipFree(cv); }
        HIP_TRY(ctx, e);
        ctx->csr_ptr = cp; ctx->csr_idx = ci; ctx->csr_val = cv; ctx->csr_nnz = nnz_sel;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *nnz_out = nnz_sel;
    return CNMF_OK;
}

extern "C" int cnmf_prepare_fetch(cnmf_ctx* ctx, int64_t* indptr, int32_t* indices, double* values)
{
    if (!ctx || !values) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PrepStage& P = ctx->prep;
    if (P.out_nnz < 0) { SET_ERR(ctx, "cnmf_prepare_select has not been called"); return CNMF_ESTATE; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)ctx->N;
    if (P.out_dense) {
        HIP_TRY(ctx, hipMemcpyAsync(values, P.odense, N * (size_t)P.out_n * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        if (!indptr || (!indices && P.out_nnz > 0)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
        HIP_TRY(ctx, hipMemcpyAsync(indptr, P.optr, (N + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
        if (P.out_nnz > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(indices, P.oidx, (size_t)P.out_nnz * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(values, P.oval, (size_t)P.out_nnz * sizeof(double), hipMemcpyDeviceToHost, st));
        }
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
