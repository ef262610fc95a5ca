// The device steps of Preprocess.highly_variable_genes (scanpy's flavor='seurat_v3', one batch) on the staging of
// preprocess_host.hip.h (ctx->pre: the raw counts as CSR and as their transpose):
//
//   * per-gene moments S1 = sum x and S2 = sum x^2 as 64-bit integers over the transpose, a wavefront per column in the
//     order of kernels_segments.hip.h (lane-strided, a fixed butterfly), with a flag for a value that is no count
//     (negative, non-integer, not finite) and one for a count above HVG_COUNT_MAX = 2^20; with at most HVG_CELLS_MAX =
//     2^22 cells S2 <= 2^62 never wraps.  The host forms mean and the ddof=1 variance from the exact integers;
//   * the local fits of skmisc's loess(degree=2, family gaussian) at m evaluation points over n SORTED abscissae, one
//     workgroup per point: the q nearest neighbours of x0 in a sorted array are a contiguous window, found by binary
//     search (the first lo in [0, n - q] with x0 - x[lo] <= x[lo + q] - x0); h = max(x0 - x[lo], x[lo + q - 1] - x0)
//     is the q-th smallest distance; the workgroup strides the window and accumulates the eight weighted moments in
//     t = (x - x0) / h -- sum w, w t, w t^2, w t^3, w t^4, w y, w t y, w t^2 y, w = (1 - (|x - x0| / h)^3)^3 where
//     |x - x0| < h, else 0 -- reduces them in a fixed tree (a butterfly per wavefront, the four wavefronts through LDS),
//     and one thread solves the 3 x 3 normal equations by an LDL^T factorisation.  Normal equations square the
//     condition number of the design (about 6 inside the data, more at the end vertices), which a plain float64 sum and
//     solve pay with 10 to 50 times the rounding error of a least-squares solve on the design itself; so the moments
//     are COMPENSATED float64 sums (every partial sum a pair hi + lo of doubles, the error of each addition kept by
//     Knuth's two-sum) and the 3 x 3 solve runs on such pairs as well.  Status per point: HVG_FIT_ZERO_WIDTH when
//     h <= 0, HVG_FIT_DEFICIENT when a pivot of the factorisation falls below HVG_PIVOT_MIN of its diagonal entry (fewer
//     than three distinct weighted abscissae, or close to it): the caller redoes those few points on the host with the
//     minimum-norm formula; the pseudo-inverse's threshold is not emulated here;
//   * per-gene sums C1 = sum min(x, clip[g]) and C2 = sum min(x, clip[g])^2 over the transpose, float64, a wavefront per
//     column as above.
//
// Integer counters and fixed-order float64 sums only (the order: kernels_segments.hip.h) -- no float atomics: two calls
// on the same input give the same bits.  Included by cnmf_hip.hip (after filter_host.hip.h).
#pragma once

namespace cnmf {

constexpr double HVG_COUNT_MAX = 1048576.0;              // 2^20: a larger count is refused
constexpr long long HVG_CELLS_MAX = 1ll << 22;           // so that sum x^2 <= 2^62
constexpr int HVG_FLAG_NOT_COUNT = 1, HVG_FLAG_TOO_LARGE = 2;
constexpr int HVG_FIT_OK = 0, HVG_FIT_ZERO_WIDTH = 1, HVG_FIT_DEFICIENT = 2;
constexpr double HVG_PIVOT_MIN = 1e-6;
constexpr int HVG_FIT_THREADS = 256;

// Both O(nnz) kernels serve the one-batch and the per-batch entry points (hvg_batch_host.hip.h).  One wavefront per pair
// w = b G + g of a batch b = blockIdx.y and a column g of the transposed counts (kernels_segments.hip.h).  start == nullptr:
// one batch, the whole column.  Otherwise the column is one of the GROUPED transpose and the pair's entries are its run of
// the rows [start[b], start[b + 1]): the walk begins at the run's first entry, so the additions of a pair are the very
// sequence the one-batch call performs on the staging restricted to the cells of b.  An empty run gives zeros.

// s1[w] = sum x, s2[w] = sum x^2 as integers, flags[w] = what was met that is no count (left out of the sums)
__global__ __launch_bounds__(256) void hvg_gene_moments_kernel(const long long* __restrict__ cptr, const int* __restrict__ crow,
                                                               const double* __restrict__ cval, int G,
                                                               const int* __restrict__ start, long long* __restrict__ s1,
                                                               long long* __restrict__ s2, int* __restrict__ flags)
{
    const int g = seg_index(), bt = blockIdx.y;
    if (g >= G) return;
    long long p0 = cptr[g], p1 = cptr[g + 1];
    if (start) seg_row_run(crow, start[bt], start[bt + 1], &p0, &p1);
    long long a = 0, b = 0;
    int f = 0;
    seg_for_each(p0, p1, [&](long long p) {
        const double v = cval[p];
        if (!(v >= 0.0) || v != floor(v)) { f |= HVG_FLAG_NOT_COUNT; return; }
        if (v > HVG_COUNT_MAX) { f |= HVG_FLAG_TOO_LARGE; return; }
        const long long iv = (long long)v;
        a += iv;
        b += iv * iv;
    });
    a = seg_sum(a); b = seg_sum(b); f = seg_or(f);
    const size_t w = (size_t)bt * G + g;
    if (seg_lane() == 0) { s1[w] = a; s2[w] = b; flags[w] = f; }
}

// c1[w] = sum min(x, clip[w]), c2[w] = sum of its square (the square rounded, then added)
__global__ __launch_bounds__(256) void hvg_clipped_sums_kernel(const long long* __restrict__ cptr, const int* __restrict__ crow,
                                                               const double* __restrict__ cval, int G,
                                                               const int* __restrict__ start, const double* __restrict__ clip,
                                                               double* __restrict__ c1, double* __restrict__ c2)
{
#pragma clang fp contract(off)
    const int g = seg_index(), bt = blockIdx.y;
    if (g >= G) return;
    long long p0 = cptr[g], p1 = cptr[g + 1];
    if (start) seg_row_run(crow, start[bt], start[bt + 1], &p0, &p1);
    const size_t w = (size_t)bt * G + g;
    const double c = clip[w];
    double a = 0.0, b = 0.0;
    seg_for_each(p0, p1, [&](long long p) {
#pragma clang fp contract(off)
        const double m = fmin(cval[p], c);
        a += m;
        b += m * m;
    });
    a = seg_sum(a); b = seg_sum(b);
    if (seg_lane() == 0) { c1[w] = a; c2[w] = b; }
}

// ---------------------------------------------------------------- pairs of doubles (hi + lo, |lo| <= ulp(hi) / 2)
// The error term of a two-sum is exact only when every operation is rounded on its own: a product fused into the
// following addition (the compiler's default for device code) leaves a wrong error term behind and the pair is worth
// one double again.  Hence `fp contract(off)` in every function here and in the kernels that call them (the flag stays
// on the instructions when they are inlined); the one fused operation wanted, the error of a product, is an explicit fma.
struct hvg_dd { double hi, lo; };

__device__ __forceinline__ hvg_dd hvg_two_sum(double a, double b)
{
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

__device__ __forceinline__ hvg_dd hvg_renorm(double hi, double lo)          // (|hi| >= |lo|)
{
#pragma clang fp contract(off)
    const double s = hi + lo;
    return {s, lo - (s - hi)};
}

__device__ __forceinline__ hvg_dd hvg_add_d(hvg_dd a, double b)
{
#pragma clang fp contract(off)
    const hvg_dd s = hvg_two_sum(a.hi, b);
    return hvg_renorm(s.hi, s.lo + a.lo);
}

__device__ __forceinline__ hvg_dd hvg_add(hvg_dd a, hvg_dd b)
{
#pragma clang fp contract(off)
    hvg_dd s = hvg_two_sum(a.hi, b.hi);
    const hvg_dd t = hvg_two_sum(a.lo, b.lo);
    s = hvg_renorm(s.hi, s.lo + t.hi);
    return hvg_renorm(s.hi, s.lo + t.lo);
}

__device__ __forceinline__ hvg_dd hvg_neg(hvg_dd a) { return {-a.hi, -a.lo}; }

__device__ __forceinline__ hvg_dd hvg_mul(hvg_dd a, hvg_dd b)
{
#pragma clang fp contract(off)
    const double p = a.hi * b.hi;
    double e = fma(a.hi, b.hi, -p);
    e += a.hi * b.lo + a.lo * b.hi;
    return hvg_renorm(p, e);
}

__device__ __forceinline__ hvg_dd hvg_div(hvg_dd a, hvg_dd b)
{
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    hvg_dd r = hvg_add(a, hvg_neg(hvg_mul(b, {q1, 0.0})));
    const double q2 = r.hi / b.hi;
    r = hvg_add(r, hvg_neg(hvg_mul(b, {q2, 0.0})));
    const double q3 = r.hi / b.hi;
    return hvg_add_d(hvg_renorm(q1, q2), q3);
}

__device__ __forceinline__ hvg_dd hvg_sub(hvg_dd a, hvg_dd b) { return hvg_add(a, hvg_neg(b)); }

// one workgroup per evaluation point e: the local quadratic fit at x0[e] over the q nearest of the n sorted abscissae
// (see the head of this file); value[e] = c0, slope[e] = c1 / h, status[e]
__global__ __launch_bounds__(HVG_FIT_THREADS) void hvg_loess_fit_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                        int n, int q, const double* __restrict__ x0s, int m,
                                                                        double* __restrict__ value, double* __restrict__ slope,
                                                                        int* __restrict__ status)
{
#pragma clang fp contract(off)
    __shared__ hvg_dd part[HVG_FIT_THREADS / 64][8];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (e >= m) return;                                  // (uniform over the workgroup)
    const double x0 = x0s[e];
    int lo = 0, hi = n - q;                              // the window [lo, lo + q): uniform over the workgroup
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x0 - x[mid] <= x[mid + q] - x0) hi = mid; else lo = mid + 1;
    }
    const double h = fmax(x0 - x[lo], x[lo + q - 1] - x0);
    if (!(h > 0.0) || !(h < INFINITY)) {
        if (tid == 0) { value[e] = 0.0; slope[e] = 0.0; status[e] = HVG_FIT_ZERO_WIDTH; }
        return;
    }
    hvg_dd acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = {0.0, 0.0};
    for (int i = lo + tid; i < lo + q; i += HVG_FIT_THREADS) {
        const double dx = x[i] - x0, d = fabs(dx);
        if (!(d < h)) continue;                          // (a point tied at distance h weighs nothing)
        const double r = d / h, u = 1.0 - r * r * r;
        const double w = u * u * u, t = dx / h, yi = y[i];
        const double wt = w * t, wt2 = wt * t, wt3 = wt2 * t, wt4 = wt3 * t;
        acc[0] = hvg_add_d(acc[0], w);
        acc[1] = hvg_add_d(acc[1], wt);
        acc[2] = hvg_add_d(acc[2], wt2);
        acc[3] = hvg_add_d(acc[3], wt3);
        acc[4] = hvg_add_d(acc[4], wt4);
        acc[5] = hvg_add_d(acc[5], w * yi);
        acc[6] = hvg_add_d(acc[6], wt * yi);
        acc[7] = hvg_add_d(acc[7], wt2 * yi);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        seg_butterfly([&](int o) {
#pragma clang fp contract(off)
            const hvg_dd other = {__shfl_xor(acc[k].hi, o, 64), __shfl_xor(acc[k].lo, o, 64)};
            acc[k] = hvg_add(acc[k], other);             // (a + b on both lanes of a pair: the same bits on every lane)
        });
        if (lane == 0) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid != 0) return;
    hvg_dd M[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) M[k] = hvg_add(hvg_add(part[0][k], part[1][k]), hvg_add(part[2][k], part[3][k]));
    // G = [[m0, m1, m2], [m1, m2, m3], [m2, m3, m4]] = L D L^T, rhs (b0, b1, b2) = M[5..7]
    const hvg_dd m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4];
    int st = HVG_FIT_OK;
    double c0 = 0.0, c1 = 0.0;
    if (!(m0.hi > 0.0)) {
        st = HVG_FIT_DEFICIENT;
    } else {
        const hvg_dd l21 = hvg_div(m1, m0), l31 = hvg_div(m2, m0);
        const hvg_dd d2 = hvg_sub(m2, hvg_mul(l21, m1));
        if (!(d2.hi > HVG_PIVOT_MIN * m2.hi)) {
            st = HVG_FIT_DEFICIENT;
        } else {
            const hvg_dd ee = hvg_sub(m3, hvg_mul(l31, m1));
            const hvg_dd l32 = hvg_div(ee, d2);
            const hvg_dd d3 = hvg_sub(hvg_sub(m4, hvg_mul(l31, m2)), hvg_mul(l32, ee));
            if (!(d3.hi > HVG_PIVOT_MIN * m4.hi)) {
                st = HVG_FIT_DEFICIENT;
            } else {
                const hvg_dd z1 = M[5];
                const hvg_dd z2 = hvg_sub(M[6], hvg_mul(l21, z1));
                const hvg_dd z3 = hvg_sub(hvg_sub(M[7], hvg_mul(l31, z1)), hvg_mul(l32, z2));
                const hvg_dd k2 = hvg_div(z3, d3);
                const hvg_dd k1 = hvg_sub(hvg_div(z2, d2), hvg_mul(l32, k2));
                const hvg_dd k0 = hvg_sub(hvg_sub(hvg_div(z1, m0), hvg_mul(l21, k1)), hvg_mul(l31, k2));
                c0 = k0.hi + k0.lo;
                c1 = (k1.hi + k1.lo) / h;
            }
        }
    }
    value[e] = c0; slope[e] = c1; status[e] = st;
}

}  // namespace cnmf

// The launch and the read-backs of the gene moments over the transpose T: B batches with their row runs in `start`
// (device, [B + 1]), or one batch over whole columns (B = 1, start == nullptr).  s1, s2 [B][G], flags [B] (host)
static int hvg_gene_moments(cnmf_ctx* ctx, const DevCsr<double>& T, int B, const int* start, int64_t* s1, int64_t* s2,
                            int32_t* flags)
{
    using namespace cnmf;
    const int G = (int)T.rows;
    const size_t W = (size_t)G * B;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    long long* d1 = pool.get<long long>(W);
    long long* d2 = pool.get<long long>(W);
    int* df = pool.get<int>(W);
    POOL_TRY(ctx, pool);
    std::vector<int> hf(W);
    hvg_gene_moments_kernel<<<dim3(seg_grid(G), B), 256, 0, st>>>(T.ptr, T.idx, T.val, G, start, d1, d2, df);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, s1, d1, W));
    HIP_TRY(ctx, dev_fetch(st, s2, d2, W));
    HIP_TRY(ctx, dev_fetch(st, hf.data(), df, W));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
        int all = 0;
        for (int g = 0; g < G; ++g) all |= hf[(size_t)b * G + g];
        flags[b] = all;
    }
    return CNMF_OK;
}

// the same for the clipped sums: clip, c1, c2 [B][G] (host)
static int hvg_clipped_sums(cnmf_ctx* ctx, const DevCsr<double>& T, int B, const int* start, const double* clip, double* c1,
                            double* c2)
{
    using namespace cnmf;
    const int G = (int)T.rows;
    const size_t W = (size_t)G * B;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dc = pool.put<double>(clip, W, st);
    double* d1 = pool.get<double>(W);
    double* d2 = pool.get<double>(W);
    POOL_TRY(ctx, pool);
    hvg_clipped_sums_kernel<<<dim3(seg_grid(G), B), 256, 0, st>>>(T.ptr, T.idx, T.val, G, start, dc, d1, d2);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, c1, d1, W));
    HIP_TRY(ctx, dev_fetch(st, c2, d2, W));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_gene_moments(cnmf_ctx* ctx, int64_t* s1, int64_t* s2, int32_t* flags)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!s1 || !s2 || !flags) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (P.N > HVG_CELLS_MAX) {
        SET_ERR(ctx, "gene_moments: %lld cells, more than %lld (sum x^2 must stay an exact int64)", (long long)P.N, HVG_CELLS_MAX);
        return CNMF_EINVAL;
    }
    return hvg_gene_moments(ctx, P.columns, 1, nullptr, s1, s2, flags);
}

extern "C" int cnmf_preprocess_clipped_sums(cnmf_ctx* ctx, const double* clip, double* c1, double* c2)
{
    using namespace cnmf;
    if (int rc = flt_staged(ctx)) return rc;
    if (!clip || !c1 || !c2) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    return hvg_clipped_sums(ctx, ctx->pre.columns, 1, nullptr, clip, c1, c2);
}

extern "C" int cnmf_preprocess_loess_fit(cnmf_ctx* ctx, int64_t n, const double* x, const double* y, int64_t q, int64_t m,
                                         const double* x0, double* value, double* slope, int32_t* status)
{
    using namespace cnmf;
    if (!ctx || !x || !y || !x0 || !value || !slope || !status) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (n < 1 || n > (1ll << 30) || q < 1 || q > n || m < 0 || m > (1ll << 30)) {
        SET_ERR(ctx, "loess_fit: n = %lld, q = %lld, m = %lld (1 <= q <= n <= 2^30, 0 <= m <= 2^30)", (long long)n, (long long)q,
                (long long)m);
        return CNMF_EINVAL;
    }
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || !std::isfinite(y[i]) || (i && x[i] < x[i - 1])) {
            SET_ERR(ctx, "loess_fit: the abscissae must be finite and sorted, the ordinates finite (entry %lld)", (long long)i);
            return CNMF_EINVAL;
        }
    for (int64_t i = 0; i < m; ++i)
        if (!std::isfinite(x0[i])) { SET_ERR(ctx, "loess_fit: evaluation point %lld is not finite", (long long)i); return CNMF_EINVAL; }
    if (m == 0) return CNMF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dx = pool.put<double>(x, (size_t)n, st);
    double* dy = pool.put<double>(y, (size_t)n, st);
    double* d0 = pool.put<double>(x0, (size_t)m, st);
    double* dv = pool.get<double>((size_t)m);
    double* ds = pool.get<double>((size_t)m);
    int* dst = pool.get<int>((size_t)m);
    POOL_TRY(ctx, pool);
    hvg_loess_fit_kernel<<<(unsigned)m, HVG_FIT_THREADS, 0, st>>>(dx, dy, (int)n, (int)q, d0, (int)m, dv, ds, dst);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dev_fetch(st, value, dv, (size_t)m));
    HIP_TRY(ctx, dev_fetch(st, slope, ds, (size_t)m));
    HIP_TRY(ctx, dev_fetch(st, status, dst, (size_t)m));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}
