// The resident matrix as compressed rows -- of X (cells x genes: "CSR") and of X^T (genes x cells: "CSC") -- for the paths
// that only touch the stored entries: the float64 Kullback-Leibler refits of the consensus tail (mu_refit_host.hip.h) and
// the sliced-ELL images of the Kullback-Leibler restarts (mu_host.hip.h).  scikit-learn walks exactly these arrays when
// the reference hands it a scipy.sparse matrix (sklearn/decomposition/_nmf.py:192 `_special_sparse_dot`; cnmf.py:726, 873,
// 950: `norm_counts.X` / `tpm.X` as stored).
//
//   * cnmf_set_matrix_csr KEEPS the uploaded arrays on the device (round 5; they used to be dropped after the densify);
//   * a matrix that arrived dense gets its compressed rows from the resident float32 matrix on first use (two passes);
//   * X^T's compressed rows are built ON THE DEVICE from those of X -- no transposed upload: a counting sort whose order
//     is fixed by construction (row chunks in order, the rows of a chunk one after the other, the entries of a row -- distinct
//     columns -- side by side), so every column lists its entries by ascending row, run to run identical.
// Included by cnmf_hip.hip (after runtime.hip.h and kernels_segments.hip.h, whose indexing, walk and butterfly the
// wavefront-per-row kernels here use; csc_xtw_f64_kernel and csr_residual_rows_kernel still spell theirs out).
#pragma once

namespace cnmf {

// ---- dense -> compressed rows.  Pass 1: stored (non-zero) entries per row
__global__ __launch_bounds__(256) void csr_count_dense_kernel(const float* __restrict__ M, int ld, int R, int C,
                                                              long long* __restrict__ cnt)
{
    const int row = seg_index();
    if (row >= R) return;
    const float* m = M + (size_t)row * ld;
    int n = 0;
    seg_for_each(0, C, [&](long long c) { n += (m[c] != 0.f) ? 1 : 0; });
    n = seg_sum(n);
    if (seg_lane() == 0) cnt[row] = n;
}

// Pass 2: a wavefront per row compacts the row in column order
__global__ __launch_bounds__(256) void csr_fill_dense_kernel(const float* __restrict__ M, int ld, int R, int C,
                                                             const long long* __restrict__ ptr, int* __restrict__ idx,
                                                             float* __restrict__ val)
{
    const int row = seg_index(), lane = seg_lane();
    if (row >= R) return;
    const float* m = M + (size_t)row * ld;
    long long base = ptr[row];
    for (int cb = 0; cb < C; cb += 64) {
        const int c = cb + lane;
        const float x = c < C ? m[c] : 0.f;
        const bool nz = x != 0.f;
        const unsigned long long mask = __ballot(nz);
        if (nz) {
            const long long p = base + __popcll(mask & ((1ull << lane) - 1ull));
            idx[p] = c; val[p] = x;
        }
        base += __popcll(mask);
    }
}

__global__ __launch_bounds__(256) void csr_widen_ptr_kernel(const int* __restrict__ p32, long long n, long long* __restrict__ p64)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p64[i] = p32[i];
}

// ---- transpose.  Pass 1: entries per (row chunk, column).  sel != nullptr: row r of the input is the segment of row sel[r]
// (the transpose of a gathered, re-ordered subset of rows: the chosen columns of prepare_host.hip.h)
__global__ __launch_bounds__(256) void csr_tr_hist_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                          const int* __restrict__ sel, int R, int C, int rows_per_chunk,
                                                          int* __restrict__ cnt)
{
    const int t = blockIdx.x;
    const int r0 = t * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    if (r0 >= r1) return;
    int* c = cnt + (size_t)t * C;
    if (!sel) {
        for (long long p = ptr[r0] + threadIdx.x; p < ptr[r1]; p += 256) atomicAdd(&c[idx[p]], 1);
        return;
    }
    for (int r = r0; r < r1; ++r)
        for (long long p = ptr[sel[r]] + threadIdx.x; p < ptr[sel[r] + 1]; p += 256) atomicAdd(&c[idx[p]], 1);
}

// Pass 2a: entries per column
__global__ __launch_bounds__(256) void csr_tr_total_kernel(const int* __restrict__ cnt, int T, int C, long long* __restrict__ total)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    long long s = 0;
    for (int t = 0; t < T; ++t) s += cnt[(size_t)t * C + c];
    total[c] = s;
}

// Pass 2b: cnt[t][c] := first position of chunk t inside column c (64-bit positions kept relative to the column start)
__global__ __launch_bounds__(256) void csr_tr_offsets_kernel(int* __restrict__ cnt, int T, int C)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int run = 0;
    for (int t = 0; t < T; ++t) { const int v = cnt[(size_t)t * C + c]; cnt[(size_t)t * C + c] = run; run += v; }
}

// Pass 3: ONE wavefront per chunk walks its rows in order; the entries of a row name distinct columns, so the 64 lanes
// never meet on a counter, and the counters of a chunk belong to this wavefront alone (the atomic is only there to go
// through L2: a plain load could see the line as it was before the previous row's store).  sel as in pass 1; div != nullptr:
// the values of row r are divided by div[r] in float64 on the way (prepare's unit-variance scaling)
template <typename T>
__global__ __launch_bounds__(64) void csr_tr_fill_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                         const T* __restrict__ val, const int* __restrict__ sel,
                                                         const double* __restrict__ div, int R, int C, int rows_per_chunk,
                                                         int* __restrict__ cnt, const long long* __restrict__ tptr,
                                                         int* __restrict__ tidx, T* __restrict__ tval)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const int r0 = t * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    int* c = cnt + (size_t)t * C;
    for (int r = r0; r < r1; ++r) {
        const int s = sel ? sel[r] : r;
        const long long b = ptr[s], e = ptr[s + 1];
        const double d = div ? div[r] : 1.0;
        for (long long p = b + lane; p < e; p += 64) {
            const int col = idx[p];
            const long long q = tptr[col] + atomicAdd(&c[col], 1);
            tidx[q] = r;
            tval[q] = div ? (T)((double)val[p] / d) : val[p];
        }
        __builtin_amdgcn_s_waitcnt(0);            // the counters of this row are back before the next row asks for them
    }
}


// ---- the float64 statistics and products of the consensus tail on the compressed rows of X^T (round 5): a wavefront per
// gene, its stored entries lane-strided, fixed-order butterfly sums -- so that a Kullback-Leibler run's tail (whose refits
// walk the stored entries already) never needs the dense N x G_all image of the TPM matrix.

// Per-column moments, a wavefront per output column j (column sel[j] of the transpose, or j), for the float64 staging
// (prepare_host.hip.h) and the float32 resident matrix alike: with v = x * scale[cell] (scale == nullptr: v = x),
// mean[j] = sum v / N and ssd[j] = sum over ALL N cells of (v - mean)^2 = sum_stored (v - mean)^2 + (N - stored) mean^2.
// Two passes, float64, in the order of kernels_segments.hip.h.
template <typename V>
__global__ __launch_bounds__(256) void col_moments_kernel(const long long* __restrict__ cptr, const int* __restrict__ crow,
                                                          const V* __restrict__ cval, const int* __restrict__ sel,
                                                          int n_out, int N, const double* __restrict__ scale,
                                                          double* __restrict__ mean, double* __restrict__ ssd)
{
    const int j = seg_index();
    if (j >= n_out) return;
    const int g = sel ? sel[j] : j;
    const long long b = cptr[g], e = cptr[g + 1];
    auto value = [&](long long p) { return scale ? (double)cval[p] * scale[crow[p]] : (double)cval[p]; };
    double s = 0.0;
    seg_for_each(b, e, [&](long long p) { s += value(p); });
    const double mu = seg_sum(s) / (double)N;
    double q = 0.0;
    seg_for_each(b, e, [&](long long p) { const double d = value(p) - mu; q += d * d; });
    q = seg_sum(q);
    if (seg_lane() == 0) { mean[j] = mu; ssd[j] = q + (double)(N - (e - b)) * mu * mu; }
}

// column sums of W [N][k] (float64), one workgroup per component, fixed order
__global__ __launch_bounds__(256) void colsum_f64_kernel(const double* __restrict__ W, int N, int k, double* __restrict__ out)
{
    __shared__ double red[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) s += W[(size_t)i * k + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[c] = red[0];
}

// out[t][g] = sum_i W[i][t] z(x_ig),  z(x) = (x - mean[g]) inv_std[g] (zs) or x:  with the zeros of the column folded
// into the constant term,  = inv_std[g] (sum_stored W[i][t] x_ig - mean[g] wsum[t]).  Components in chunks of 16.
__global__ __launch_bounds__(256) void csc_xtw_f64_kernel(const long long* __restrict__ tptr, const int* __restrict__ tidx,
                                                          const float* __restrict__ tval, int G, const double* __restrict__ W,
                                                          int k, int zs, const double* __restrict__ mean,
                                                          const double* __restrict__ inv_std, const double* __restrict__ wsum,
                                                          double* __restrict__ out)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= G) return;
    const long long b = tptr[g], e = tptr[g + 1];
    const double mu = zs ? mean[g] : 0.0, is = zs ? inv_std[g] : 1.0;
    for (int t0 = 0; t0 < k; t0 += 16) {
        const int nt = min(16, k - t0);
        double acc[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.0;
        for (long long p = b + lane; p < e; p += 64) {
            const double x = (double)tval[p];
            const double* w = W + (size_t)tidx[p] * k + t0;
#pragma unroll
            for (int t = 0; t < 16; ++t) if (t < nt) acc[t] = fma(w[t], x, acc[t]);
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            double a = acc[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0 && t < nt) out[(size_t)(t0 + t) * G + g] = (a - mu * wsum[t0 + t]) * is;
        }
    }
}


// sum over the STORED entries of row i of  (x - w_i.h_j)^2 - (w_i.h_j)^2  (float64): with  ||W H||_F^2 = tr(W^T W . H H^T)  added
// by the host this is ||X - W H||_F^2 without ever touching the zeros of X.  Ht: [G][k].  A wavefront per row.
__global__ __launch_bounds__(256) void csr_residual_rows_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                                const float* __restrict__ val, int N, const double* __restrict__ W,
                                                                const double* __restrict__ Ht, int k, double* __restrict__ part)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const long long b = ptr[row], e = ptr[row + 1];
    const double* w = W + (size_t)row * k;
    double acc = 0.0;
    for (long long p = b + lane; p < e; p += 64) {
        const double* h = Ht + (size_t)idx[p] * k;
        double s = 0.0;
        for (int c = 0; c < k; ++c) s = fma(w[c], h[c], s);
        const double d = (double)val[p] - s;
        acc += d * d - s * s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) part[row] = acc;
}

}  // namespace cnmf

static void free_csr(cnmf_ctx* c) { c->csr.release(); c->csc.release(); }

// exclusive scan of n device counts (64-bit) into ptr[0..n] through the host (n <= 2^30 rows / 2^24 columns: a few MB)
static int csr_scan_to_ptr(cnmf_ctx* ctx, long long* d_cnt_in_ptr_out, size_t n, long long* total)
{
    std::vector<long long> h(n + 1);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_cnt_in_ptr_out, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    long long run = 0;
    for (size_t i = 0; i < n; ++i) { const long long v = h[i]; h[i] = run; run += v; }
    h[n] = run;
    *total = run;
    HIP_TRY(ctx, hipMemcpyAsync(d_cnt_in_ptr_out, h.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                   // (h is a stack object)
    return CNMF_OK;
}

// compressed rows of X: the uploaded ones, or built here from the resident dense matrix
static int ensure_csr(cnmf_ctx* ctx)
{
    using namespace cnmf;
    if (ctx->csr.ptr) return CNMF_OK;
    if (!ctx->X) { SET_ERR(ctx, "cnmf_set_matrix has not been called"); return CNMF_ESTATE; }       // (neither image: no matrix)
    const int N = (int)ctx->N, G = (int)ctx->G;
    hipStream_t st = ctx->stream;
    DevCsrLocal<float> L;
    HIP_TRY(ctx, L.alloc_ptr(N, G));
    csr_count_dense_kernel<<<(N + 3) / 4, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, L.ptr);
    HIP_TRY(ctx, hipGetLastError());
    long long nnz = 0;
    if (int rc = csr_scan_to_ptr(ctx, L.ptr, (size_t)N, &nnz)) return rc;
    HIP_TRY(ctx, L.alloc_entries(nnz));
    csr_fill_dense_kernel<<<(N + 3) / 4, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, L.ptr, L.idx, L.val);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->csr.take(L);
    return CNMF_OK;
}

// Counting-sort transpose (the kernels above) of the CSR `in` into `out` (in.cols x n_rows), on the device and in a fixed
// order.  sel != nullptr: row r of the input is row sel[r] of `in`, r < n_rows (the transpose of a gathered, re-ordered
// subset of rows); div != nullptr: the values of row r are divided by div[r]; in_val != nullptr: values in place of
// in.val; `expect` (>= 0): the entries that must arrive (`what` names the transpose in the error when they do not).  The rows go in chunks: as many as keep the chunks x in.cols
// counters at <= 64 M ints, between min_chunks and 4096 (and no more than there are rows).
// `out` is taken only when every step has succeeded; until then it keeps what it held.
template <typename V>
static int csr_transpose(cnmf_ctx* ctx, const DevCsr<V>& in, const int* sel, const double* div, int64_t n_rows,
                         int min_chunks, long long expect, const char* what, DevCsr<V>* out, const V* in_val = nullptr)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    const int R = (int)n_rows, C = (int)in.cols;
    int64_t chunks = std::min<int64_t>(4096, std::max<int64_t>(min_chunks, (64ll << 20) / std::max(1, C)));
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, R));
    const int rpc = (int)((R + chunks - 1) / chunks), T = (R + rpc - 1) / rpc;
    const V* val = in_val ? in_val : in.val;
    DevPool pool;
    int* cnt = pool.get<int>((size_t)T * C, true, st);
    POOL_TRY(ctx, pool);
    DevCsrLocal<V> L;
    HIP_TRY(ctx, L.alloc_ptr(C, R));
    csr_tr_hist_kernel<<<T, 256, 0, st>>>(in.ptr, in.idx, sel, R, C, rpc, cnt);
    csr_tr_total_kernel<<<(C + 255) / 256, 256, 0, st>>>(cnt, T, C, L.ptr);
    csr_tr_offsets_kernel<<<(C + 255) / 256, 256, 0, st>>>(cnt, T, C);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0;
    if (int rc = csr_scan_to_ptr(ctx, L.ptr, (size_t)C, &total)) return rc;
    if (expect >= 0 && total != expect) {
        SET_ERR(ctx, "%s: %lld of %lld entries counted", what, total, expect);
        return CNMF_EHIP;
    }
    HIP_TRY(ctx, L.alloc_entries(total));
    csr_tr_fill_kernel<V><<<T, 64, 0, st>>>(in.ptr, in.idx, val, sel, div, R, C, rpc, cnt, L.ptr, L.idx, L.val);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    out->take(L);
    return CNMF_OK;
}

// compressed rows of X^T, from those of X; at least 64 row chunks
static int ensure_csc(cnmf_ctx* ctx)
{
    if (ctx->csc.ptr) return CNMF_OK;
    if (int rc = ensure_csr(ctx)) return rc;
    return csr_transpose<float>(ctx, ctx->csr, nullptr, nullptr, ctx->N, 64, ctx->csr.nnz, "transpose of the compressed rows", &ctx->csc);
}
