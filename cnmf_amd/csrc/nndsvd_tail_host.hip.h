// The tail of init='nndsvd' on the device (sklearn utils/extmath.py:588-602 + decomposition/_nmf.py:317-354), for one
// GROUP of restarts behind the range finder of nndsvd_host.hip.h: nothing comes from the host but the ranks, the seeds
// and a few scalars, and nothing goes back but a status and max W0 per restart.
//
//   start blocks   RandomState(seed_b).normal(size=(M_cols, c_b)) drawn by rng_kernel<2> (range_finder_run)
//   small SVD      of every B_b [c_b][M_cols] in float64: one-sided Jacobi (Hestenes) on the ROWS of B_b, one workgroup per
//                  block, one wave per pair of a round-robin round, the rows in global memory (L2); fixed-order reductions,
//                  no atomics, no grid-wide barrier -> the same bits on every run.  A = J B ends with orthogonal rows
//                  s_j v_j^T; the left vectors in the small basis are the rows of J.
//   back-transform UT[j] = J[j] . Q^T (float64), the k leading vectors only
//   flip / split   svd_flip on the matrix that was decomposed, positive / negative parts, lambda = sqrt(S_j sigma),
//                  < eps -> 0, ('nndsvda') 0 -> X.mean(); ONE rounding to float32 into the context's init store
//                  (cnmf_ctx::inits, the component-major layout of generate_inits(): init_mode 2 installs from it).
// status per restart: 0 accepted; bit 0 the sweep cap was hit, bit 1 a value is not finite, bit 2 S_j == 0 for a j < k
// (a block of rank below k, where scikit-learn's own arithmetic divides by zero).
#pragma once
#include <cfloat>

namespace cnmf {

constexpr int NNDSVD_MAX_SWEEPS = 30;
constexpr int JAC_WAVES = 16;

struct TailBlk { int off, c, k, row0; };        // first packed column, width k + 10, rank, first component row in the group

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);      // butterfly: every lane ends with the same bits
    return v;
}

// grid = blocks, 1024 threads.  A [C][L] float64 work rows, J [C][KMAX]; out: S [C] descending, order [C] (row of A / J
// that holds the j-th singular triplet), jstat[block] = 1 when the sweep cap was hit.
__global__ __launch_bounds__(64 * JAC_WAVES) void nndsvd_jacobi_kernel(const float* __restrict__ B, int ldb, int L,
                                                                        const TailBlk* __restrict__ blocks, double* A,
                                                                        double* J, double* __restrict__ S,
                                                                        int* __restrict__ order, int* __restrict__ jstat)
{
    __shared__ int rotated;
    __shared__ double snorm[KMAX];
    const TailBlk tb = blocks[blockIdx.x];
    const int c = tb.c, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* Ab = A + (size_t)tb.off * L;
    double* Jb = J + (size_t)tb.off * KMAX;
    for (int r = 0; r < c; ++r)
        for (int g = tid; g < L; g += 64 * JAC_WAVES) Ab[(size_t)r * L + g] = (double)B[(size_t)(tb.off + r) * ldb + g];
    for (int e = tid; e < c * KMAX; e += 64 * JAC_WAVES) Jb[e] = (e / KMAX == e % KMAX) ? 1.0 : 0.0;
    if (tid == 0) rotated = 0;
    __syncthreads();
    const int n = c + (c & 1);                       // players of the round robin; an odd block has a dummy that sits out
    const int npairs = n / 2;
    int sweeps = 0;
    bool conv = c < 2;
    while (!conv && sweeps < NNDSVD_MAX_SWEEPS) {
        for (int r = 0; r < n - 1; ++r) {
            for (int i = wave; i < npairs; i += JAC_WAVES) {
                int p = i == 0 ? n - 1 : (r + i) % (n - 1);
                int q = i == 0 ? r : (r - i + n - 1) % (n - 1);
                if (p > q) { const int t_ = p; p = q; q = t_; }
                if (q >= c) continue;
                double* ap = Ab + (size_t)p * L;
                double* aq = Ab + (size_t)q * L;
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int g = lane; g < L; g += 64) {
                    const double x = ap[g], y = aq[g];
                    al += x * x; be += y * y; ga += x * y;
                }
                al = wave_sum_f64(al); be = wave_sum_f64(be); ga = wave_sum_f64(ga);
                if (al == 0.0 || be == 0.0 || fabs(ga) <= 4.0 * DBL_EPSILON * sqrt(al * be)) continue;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int g = lane; g < L; g += 64) {
                    const double x = ap[g], y = aq[g];
                    ap[g] = cs * x - sn * y; aq[g] = sn * x + cs * y;
                }
                double* jp = Jb + (size_t)p * KMAX;
                double* jq = Jb + (size_t)q * KMAX;
                for (int m = lane; m < c; m += 64) {
                    const double x = jp[m], y = jq[m];
                    jp[m] = cs * x - sn * y; jq[m] = sn * x + cs * y;
                }
                if (lane == 0) rotated = 1;
            }
            __syncthreads();                         // the pairs of a round are disjoint; the next round reads their rows
        }
        ++sweeps;
        conv = rotated == 0;
        __syncthreads();
        if (tid == 0) rotated = 0;
        __syncthreads();
    }
    for (int j = wave; j < c; j += JAC_WAVES) {
        double s = 0.0;
        for (int g = lane; g < L; g += 64) { const double x = Ab[(size_t)j * L + g]; s += x * x; }
        s = wave_sum_f64(s);
        if (lane == 0) snorm[j] = sqrt(s);
    }
    __syncthreads();
    if (tid == 0) {                                  // stable descending insertion sort of at most 128 values
        int* ord = order + tb.off;
        for (int j = 0; j < c; ++j) {
            int pos = j;
            while (pos > 0 && snorm[ord[pos - 1]] < snorm[j]) { ord[pos] = ord[pos - 1]; --pos; }
            ord[pos] = j;
        }
        for (int j = 0; j < c; ++j) S[tb.off + j] = snorm[ord[j]];
        jstat[blockIdx.x] = conv ? 0 : 1;
    }
}

// UT[row0 + j][i] = sum_m J[order_j][m] * Q[m][i]  (Q component-major float32 [.][ldq]); grid (ceil(Lr / 256), kmax, blocks)
__global__ __launch_bounds__(256) void nndsvd_backtransform_kernel(const float* __restrict__ Q, int ldq, int Lr,
                                                                   const TailBlk* __restrict__ blocks,
                                                                   const double* __restrict__ J, const int* __restrict__ order,
                                                                   double* __restrict__ UT)
{
    const TailBlk tb = blocks[blockIdx.z];
    const int j = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (j >= tb.k || i >= Lr) return;
    const double* jr = J + (size_t)(tb.off + order[tb.off + j]) * KMAX;
    double acc = 0.0;
    for (int m = 0; m < tb.c; ++m) acc += jr[m] * (double)Q[(size_t)(tb.off + m) * ldq + i];
    UT[(size_t)(tb.row0 + j) * Lr + i] = acc;
}

// sum over the workgroup (256 threads) in a fixed order; every thread gets the result
__device__ __forceinline__ double wg_sum_f64(double v, double* red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per component row of the group: svd_flip, the split, the threshold and the one rounding to float32.
// variant 0: 'nndsvd', 1: 'nndsvda' (zeros become x_mean).  rowmax[row] = max of the W0 row, rowbad[row]: status bits.
__global__ __launch_bounds__(256) void nndsvd_split_kernel(const TailBlk* __restrict__ blocks, const int* __restrict__ rowblk,
                                                           const double* __restrict__ A, int Lc, const double* __restrict__ UT,
                                                           int Lr, const double* __restrict__ S, const int* __restrict__ order,
                                                           int transpose, int variant, double eps, double x_mean,
                                                           float* __restrict__ Wt0, int N, float* __restrict__ H0, int G,
                                                           float* __restrict__ rowmax, int* __restrict__ rowbad)
{
    __shared__ double red[256];
    __shared__ double amax[256];
    __shared__ int aidx[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const TailBlk tb = blocks[rowblk[row]];
    const int j = row - tb.row0;
    const double s = S[tb.off + j];
    const double* u = UT + (size_t)row * Lr;                                  // left vector, over M's rows
    const double* a = A + (size_t)(tb.off + order[tb.off + j]) * Lc;          // s * right vector, over M's columns
    // svd_flip: the first index of the largest magnitude of the vector over the ROWS of the matrix that was decomposed
    // (X itself: the samples) -- UT, or the right vector when M = X^T
    const int Ll = transpose ? Lc : Lr;
    double bm = -1.0; int bi = 0x7fffffff;
    for (int i = tid; i < Ll; i += 256) {
        const double v = fabs(transpose ? a[i] / s : u[i]);
        if (v > bm) { bm = v; bi = i; }
    }
    amax[tid] = bm; aidx[tid] = bi;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) {
            const double o = amax[tid + h]; const int oi = aidx[tid + h];
            if (o > amax[tid] || (o == amax[tid] && oi < aidx[tid])) { amax[tid] = o; aidx[tid] = oi; }
        }
        __syncthreads();
    }
    double sg = 0.0;
    if (aidx[0] < Ll) {
        const double lv = transpose ? a[aidx[0]] / s : u[aidx[0]];
        sg = lv > 0.0 ? 1.0 : (lv < 0.0 ? -1.0 : 0.0);
    }
    // x: the vector over the samples (length N), y: over the features (length G)
    auto xval = [&](int i) { return sg * (transpose ? a[i] / s : u[i]); };
    auto yval = [&](int g) { return sg * (transpose ? u[g] : a[g] / s); };
    double scale_x, scale_y, nx = 1.0, ny = 1.0;   // W = scale_x * part(x) / nx, H = scale_y * part(y) / ny
    bool pos = true, both = false;
    if (j == 0) {
        both = true;                            // |x|
        scale_x = scale_y = sqrt(s);
    } else {
        double xp = 0.0, xn = 0.0, yp = 0.0, yn = 0.0;
        for (int i = tid; i < N; i += 256) { const double v = xval(i); if (v > 0.0) xp += v * v; else xn += v * v; }
        for (int g = tid; g < G; g += 256) { const double v = yval(g); if (v > 0.0) yp += v * v; else yn += v * v; }
        xp = sqrt(wg_sum_f64(xp, red)); xn = sqrt(wg_sum_f64(xn, red));
        yp = sqrt(wg_sum_f64(yp, red)); yn = sqrt(wg_sum_f64(yn, red));
        const double m_p = xp * yp, m_n = xn * yn;
        pos = m_p > m_n;
        const double lbd = sqrt(s * (pos ? m_p : m_n));
        scale_x = lbd; scale_y = lbd;
        nx = pos ? xp : xn; ny = pos ? yp : yn;     // (u = x_p / x_p_nrm first, then lbd * u: the host's two roundings)
    }
    float mx = 0.f; int bad = (s == 0.0) ? 4 : 0;
    for (int i = tid; i < N; i += 256) {
        const double v = xval(i);
        const double part = both ? fabs(v) : (pos ? fmax(v, 0.0) : fabs(fmin(v, 0.0)));
        double w = both ? scale_x * part : scale_x * (part / nx);
        if (w < eps) w = 0.0;
        if (variant == 1 && w == 0.0) w = x_mean;
        const float wf = (float)w;
        if (!isfinite(wf)) bad |= 2;
        mx = fmaxf(mx, wf);
        Wt0[(size_t)row * N + i] = wf;
    }
    for (int g = tid; g < G; g += 256) {
        const double v = yval(g);
        const double part = both ? fabs(v) : (pos ? fmax(v, 0.0) : fabs(fmin(v, 0.0)));
        double h = both ? scale_y * part : scale_y * (part / ny);
        if (h < eps) h = 0.0;
        if (variant == 1 && h == 0.0) h = x_mean;
        const float hf = (float)h;
        if (!isfinite(hf)) bad |= 2;
        H0[(size_t)row * G + g] = hf;
    }
    __syncthreads();
    amax[tid] = (double)mx; aidx[tid] = bad;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) { amax[tid] = fmax(amax[tid], amax[tid + h]); aidx[tid] |= aidx[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { rowmax[row] = (float)amax[0]; rowbad[row] = aidx[0]; }
}

// ---- 'nndsvdar': the zeros become |X.mean() * z / 100|, z the first normals of a fresh RandomState(seed), handed out in
// row-major order of W [N][k] first and of H [k][G] then.  The positions of that order are cut into chunks of 256: zeros
// per chunk (ballot), an exclusive scan over the chunks of a restart, the draws of rng_kernel<3>, a scatter.
struct ArBlk { int k, row0, nch, zoff; long long T; };      // T = k (N + G) positions, nch chunks, first draw in Z

__device__ __forceinline__ float* nndsvdar_entry(float* Wt0, float* H0, int N, int G, const ArBlk& ab, long long p)
{
    const long long kN = (long long)ab.k * N;
    if (p < kN) return Wt0 + (size_t)(ab.row0 + (int)(p % ab.k)) * N + (size_t)(p / ab.k);
    const long long q = p - kN;
    return H0 + (size_t)(ab.row0 + (int)(q / G)) * G + (size_t)(q % G);
}

// grid (max chunks, restarts), 256 threads.  SCATTER = false: chunk[b][ch] = zeros of the chunk; true: chunk holds the
// exclusive scan and the zeros are filled
template <bool SCATTER>
__global__ __launch_bounds__(256) void nndsvdar_chunk_kernel(float* Wt0, float* H0, int N, int G, const ArBlk* __restrict__ blocks,
                                                             int* chunk, int maxch, const double* __restrict__ Z, double x_mean)
{
    __shared__ int wsum[4];
    const ArBlk ab = blocks[blockIdx.y];
    if ((int)blockIdx.x >= ab.nch) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = (long long)blockIdx.x * 256 + tid;
    float* e = p < ab.T ? nndsvdar_entry(Wt0, H0, N, G, ab, p) : nullptr;
    const bool zero = e && *e == 0.f;
    const unsigned long long bal = __ballot(zero);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; tot += wsum[w]; }
    int* cnt = chunk + (size_t)blockIdx.y * maxch + blockIdx.x;
    if (!SCATTER) { if (tid == 0) *cnt = tot; return; }
    if (zero) {
        const int rank = *cnt + before + __popcll(bal & ((1ull << lane) - 1ull));
        *e = (float)fabs((x_mean * Z[(size_t)ab.zoff + rank]) / 100.0);
    }
}

// exclusive scan of chunk[b][0 .. nch) in place, total[b] = zeros of the restart; grid = restarts, 256 threads
__global__ __launch_bounds__(256) void nndsvdar_scan_kernel(const ArBlk* __restrict__ blocks, int* chunk, int maxch,
                                                            int* __restrict__ total)
{
    __shared__ int part[256];
    const ArBlk ab = blocks[blockIdx.x];
    int* c = chunk + (size_t)blockIdx.x * maxch;
    const int tid = threadIdx.x, seg = (ab.nch + 255) / 256;
    const int lo = min(ab.nch, tid * seg), hi = min(ab.nch, lo + seg);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += c[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        total[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) { const int v = c[i]; c[i] = run; run += v; }
}

// rowmax[row] = max of the W0 row (after the fill); grid = component rows, 256 threads
__global__ __launch_bounds__(256) void nndsvd_rowmax_kernel(const float* __restrict__ Wt0, int N, float* __restrict__ rowmax)
{
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float m = 0.f;
    for (int i = tid; i < N; i += 256) m = fmaxf(m, Wt0[(size_t)blockIdx.x * N + i]);
    red[tid] = m;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
        __syncthreads();
    }
    if (tid == 0) rowmax[blockIdx.x] = red[0];
}

// room for `more` further component rows in the init store of a matrix of the context's shape
static int init_store_reserve(cnmf_ctx* ctx, size_t more)
{
    cnmf_ctx::InitStore& is = ctx->inits;
    if (is.rows && (is.N != ctx->N || is.G != ctx->G)) { SET_ERR(ctx, "the init store holds factors of another matrix shape"); return CNMF_ESTATE; }
    if (is.N != ctx->N || is.G != ctx->G) is.release();        // (empty, but sized for another shape)
    is.N = ctx->N; is.G = ctx->G;
    if (is.rows + more <= is.cap_rows) return CNMF_OK;
    const size_t cap = std::max(is.rows + more, 2 * is.cap_rows);
    float *nH = nullptr, *nW = nullptr;
    hipError_t e = hipMalloc(&nH, cap * (size_t)is.G * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&nW, cap * (size_t)is.N * sizeof(float));
    if (e == hipSuccess && is.rows) {
        e = hipMemcpyAsync(nH, is.H, is.rows * (size_t)is.G * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nW, is.Wt, is.rows * (size_t)is.N * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) { hipFree(nH); hipFree(nW); HIP_TRY(ctx, e); }
    hipFree(is.H); hipFree(is.Wt);
    is.H = nH; is.Wt = nW; is.cap_rows = cap;
    return CNMF_OK;
}

// the 'nndsvdar' fill of the group's factors (Wt0 / H0: the group's first rows in the init store), then their row maxima again
static int nndsvdar_fill(cnmf_ctx* ctx, int nblocks, const std::vector<TailBlk>& blk, const uint32_t* seeds, double x_mean,
                         float* Wt0, float* H0, int K, float* dRowmax)
{
    hipStream_t st = ctx->stream;
    const int N = (int)ctx->N, G = (int)ctx->G;
    std::vector<ArBlk> ab(nblocks);
    int maxch = 1;
    for (int b = 0; b < nblocks; ++b) {
        const long long T = (long long)blk[b].k * ((long long)N + G);
        ab[b] = ArBlk{blk[b].k, blk[b].row0, (int)((T + 255) / 256), 0, T};
        maxch = std::max(maxch, ab[b].nch);
    }
    DevPool pool;
    ArBlk* dAb = pool.get<ArBlk>(nblocks);
    int* dChunk = pool.get<int>((size_t)nblocks * maxch);
    int* dTotal = pool.get<int>(nblocks);
    RngJob* dJobs = pool.get<RngJob>(nblocks);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dAb, ab.data(), nblocks * sizeof(ArBlk), hipMemcpyHostToDevice, st));
    nndsvdar_chunk_kernel<false><<<dim3(maxch, nblocks), 256, 0, st>>>(Wt0, H0, N, G, dAb, dChunk, maxch, nullptr, x_mean);
    nndsvdar_scan_kernel<<<nblocks, 256, 0, st>>>(dAb, dChunk, maxch, dTotal);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int> total(nblocks);
    HIP_TRY(ctx, hipMemcpyAsync(total.data(), dTotal, nblocks * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::vector<RngJob> jobs(nblocks);
    long long nz = 0;
    for (int b = 0; b < nblocks; ++b) {
        if (nz + total[b] > 0x7fffffffLL) { SET_ERR(ctx, "too many zeros for one group"); return CNMF_EUNSUPPORTED; }
        ab[b].zoff = (int)nz;
        jobs[b] = RngJob{seeds[b], 1, (int)nz, 0.0, (long long)total[b]};
        nz += total[b];
    }
    double* dZ = pool.get<double>((size_t)nz);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dAb, ab.data(), nblocks * sizeof(ArBlk), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dJobs, jobs.data(), nblocks * sizeof(RngJob), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                           // `ab` and `jobs` are stack temporaries
    rng_kernel<3><<<nblocks, 256, 0, st>>>(dJobs, dZ, nullptr, 0, 1, nullptr, 0, 1);
    nndsvdar_chunk_kernel<true><<<dim3(maxch, nblocks), 256, 0, st>>>(Wt0, H0, N, G, dAb, dChunk, maxch, dZ, x_mean);
    nndsvd_rowmax_kernel<<<K, 256, 0, st>>>(Wt0, N, dRowmax);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));                           // the pool goes with this scope
    return CNMF_OK;
}

}  // namespace cnmf

extern "C" int cnmf_nndsvd_group(cnmf_ctx* ctx, int transpose, int nblocks, const int32_t* k, const uint32_t* seeds,
                                 int n_iter, int variant, double eps, double x_mean, int32_t* status_out)
{
    using namespace cnmf;
    if (!ctx || !k || !seeds || !status_out || nblocks < 1 || n_iter < 0) { SET_ERR(ctx, "bad argument"); return CNMF_EINVAL; }
    if (variant < 0 || variant > 2) { SET_ERR(ctx, "unknown variant %d (0: nndsvd, 1: nndsvda, 2: nndsvdar)", variant); return CNMF_EINVAL; }
    if (ctx->N <= 0) { SET_ERR(ctx, "cnmf_set_matrix has not been called"); return CNMF_ESTATE; }
    const int N = (int)ctx->N, G = (int)ctx->G;
    std::vector<int32_t> widths(nblocks);
    std::vector<TailBlk> blk(nblocks);
    int C = 0, K = 0, kmax = 0;
    for (int b = 0; b < nblocks; ++b) {
        if (k[b] < 1 || k[b] > std::min(N, G)) { SET_ERR(ctx, "rank %d outside 1..min(n_samples, n_features)", k[b]); return CNMF_EINVAL; }
        if (k[b] + 10 > KMAX) { SET_ERR(ctx, "rank %d + 10 columns exceed %d", k[b], KMAX); return CNMF_EUNSUPPORTED; }
        widths[b] = k[b] + 10;
        blk[b] = TailBlk{C, k[b] + 10, k[b], K};
        C += widths[b]; K += k[b]; kmax = std::max(kmax, (int)k[b]);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = init_store_reserve(ctx, (size_t)K))) return rc;
    RangeFinderRun run;
    if ((rc = range_finder_run(ctx, transpose, nblocks, widths.data(), nullptr, seeds, n_iter, run))) return rc;
    hipStream_t st = ctx->stream;
    const int Lr = run.Lr, Lc = run.Lc;
    DevPool pool;
    double* dA = pool.get<double>((size_t)C * Lc);
    double* dJ = pool.get<double>((size_t)C * KMAX);
    double* dS = pool.get<double>(C);
    int* dOrder = pool.get<int>(C);
    int* dJstat = pool.get<int>(nblocks);
    double* dUT = pool.get<double>((size_t)K * Lr);
    TailBlk* dBlk = pool.get<TailBlk>(nblocks);
    int* dRowblk = pool.get<int>(K);
    float* dRowmax = pool.get<float>(K);
    int* dRowbad = pool.get<int>(K);
    POOL_TRY(ctx, pool);
    std::vector<int> rowblk(K), jstat(nblocks), rowbad(K);
    std::vector<float> rowmax(K);
    for (int b = 0; b < nblocks; ++b)
        for (int j = 0; j < blk[b].k; ++j) rowblk[blk[b].row0 + j] = b;
    HIP_TRY(ctx, hipMemcpyAsync(dBlk, blk.data(), nblocks * sizeof(TailBlk), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dRowblk, rowblk.data(), K * sizeof(int), hipMemcpyHostToDevice, st));
    nndsvd_jacobi_kernel<<<nblocks, 64 * JAC_WAVES, 0, st>>>(run.dCm, run.Lcp, Lc, dBlk, dA, dJ, dS, dOrder, dJstat);
    HIP_TRY(ctx, hipGetLastError());
    nndsvd_backtransform_kernel<<<dim3((Lr + 255) / 256, kmax, nblocks), 256, 0, st>>>(run.dR, run.Lrp, Lr, dBlk, dJ, dOrder, dUT);
    HIP_TRY(ctx, hipGetLastError());
    cnmf_ctx::InitStore& is = ctx->inits;
    nndsvd_split_kernel<<<K, 256, 0, st>>>(dBlk, dRowblk, dA, Lc, dUT, Lr, dS, dOrder, transpose ? 1 : 0, variant == 1 ? 1 : 0, eps, x_mean,
                                           is.Wt + is.rows * (size_t)N, N, is.H + is.rows * (size_t)G, G, dRowmax, dRowbad);
    HIP_TRY(ctx, hipGetLastError());
    if (variant == 2 && (rc = nndsvdar_fill(ctx, nblocks, blk, seeds, x_mean, is.Wt + is.rows * (size_t)N, is.H + is.rows * (size_t)G, K, dRowmax))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(jstat.data(), dJstat, nblocks * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(rowmax.data(), dRowmax, K * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(rowbad.data(), dRowbad, K * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < nblocks; ++b) {
        int status = jstat[b];
        float mx = 0.f;
        for (int j = 0; j < blk[b].k; ++j) { status |= rowbad[blk[b].row0 + j]; mx = std::max(mx, rowmax[blk[b].row0 + j]); }
        status_out[b] = status;
        is.k.push_back(blk[b].k); is.maxW.push_back(mx);
    }
    is.rows += (size_t)K;
    return CNMF_OK;
}

extern "C" int cnmf_init_store_reset(cnmf_ctx* ctx)
{
    if (!ctx) return CNMF_EINVAL;
    hipStreamSynchronize(ctx->stream);
    ctx->inits.rows = 0; ctx->inits.k.clear(); ctx->inits.maxW.clear();
    return CNMF_OK;
}

// The store on the host, restart after restart: W0 packed [N][k_r] blocks, H0 [sum k][G]; n_out = restarts held.
// W0 / H0 may be NULL (only the count); rows_cap: the component rows (sum k) the caller's arrays have room for.
extern "C" int cnmf_init_store_fetch(cnmf_ctx* ctx, float* W0, float* H0, int64_t rows_cap, int32_t* n_out)
{
    if (!ctx) return CNMF_EINVAL;
    const cnmf_ctx::InitStore& is = ctx->inits;
    if (n_out) *n_out = (int32_t)is.k.size();
    if (!is.rows || (!W0 && !H0)) return CNMF_OK;
    if ((int64_t)is.rows > rows_cap) { SET_ERR(ctx, "the init store holds %lld component rows, the arrays have room for %lld", (long long)is.rows, (long long)rows_cap); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)is.N, G = (size_t)is.G;
    if (H0) HIP_TRY(ctx, hipMemcpyAsync(H0, is.H, is.rows * G * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> wt;
    if (W0) {
        wt.resize(is.rows * N);
        HIP_TRY(ctx, hipMemcpyAsync(wt.data(), is.Wt, is.rows * N * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (W0) {
        size_t row0 = 0;
        for (int kr : is.k) {
            float* w = W0 + row0 * N;
            for (int c = 0; c < kr; ++c)
                for (size_t i = 0; i < N; ++i) w[i * kr + c] = wt[(row0 + c) * N + i];
            row0 += (size_t)kr;
        }
    }
    return CNMF_OK;
}
