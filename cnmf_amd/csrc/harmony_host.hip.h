// Harmony's soft clustering on the device (cnmf_harmony_*): the loop harmonypy's run_harmony spends its time in --
// cluster() with its block-wise update_R(), the objective, and the mixture-of-experts ridge correction of the PCA scores.
// The host (cnmf_amd/preprocess.py, Preprocess.run_harmony) keeps the control flow: per k-means iteration it draws the
// permutation (numpy's global RandomState), calls cnmf_harmony_kmeans_step and reads three objective terms back.
//
// Float64 throughout.  Cell-indexed arrays are component- or cluster-major ([d][N_pad], [K][N_pad], N_pad a multiple of
// 64: a wave reads 64 consecutive cells); the batch variables are int32 level codes per variable, not a one-hot Phi.
// No float atomics: every sum over cells is taken over fixed cell chunks (HCH cells of the cell order, HSC positions of a
// block of the permutation), each chunk in ascending order, and the chunk partials are added in chunk order.  The chunks
// depend on N and the number of blocks alone, never on the launch shape: two runs give the same bits.
//
//   har_cos_kernel               Z_cos: every cell's scores divided by their largest (the first call only), then by their L2 norm
//   har_centroid_*_kernel        Y = Z_cos R^T, every centroid divided by its L2 norm
//   har_dist_kernel              dist = 2 (1 - Y^T Z_cos), S = exp(-dist / sigma - its maximum over the clusters of the cell)
//                                (and R = S / its sum over the clusters, at the start)
//   har_levelsum_kernel          sum of R over the cells of one sub-chunk of a block, per cluster and level (and over all)
//   har_eo_kernel                E, O with a block taken out / put back; ((E + 1) / (O + 1))^theta for the block taken out
//   har_update_kernel            R of a block's cells from S and that table, every cell divided by its L1 norm
//   har_tab_kernel / har_obj_*   theta log((O + 1) / (E + 1)); the three terms of the objective
//   har_pack_kernel              R^T and Phi_moe^T for the ridge products (pre_gemm_kernel, preprocess_host.hip.h)
// The blocks of one update_R are sequential by definition: per block one har_eo_kernel (a single workgroup: E and O are
// K x B), one har_update_kernel and one har_levelsum_kernel over the block's cells; the sums of the OLD R of every
// block are taken by one launch up front (a block's cells are untouched until its own turn).
#pragma once

namespace cnmf {

constexpr int HCH = 512;    // cells per chunk of the centroid and objective sums
constexpr int HSC = 256;    // positions per sub-chunk of a block of the permutation

// first position of block i of np.array_split(arange(N), nb): the first N % nb blocks hold N / nb + 1 cells
__host__ __device__ __forceinline__ int har_off(int i, int N, int nb) { return i * (N / nb) + (i < N % nb ? i : N % nb); }

__global__ __launch_bounds__(256) void har_transpose_in_kernel(const double* __restrict__ T, int N, int Np, int d,
                                                               double* __restrict__ Z)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    for (int c = 0; c < d; ++c) Z[(size_t)c * Np + n] = T[(size_t)n * d + c];
}

__global__ __launch_bounds__(256) void har_cos_kernel(const double* __restrict__ Zin, int N, int Np, int d, int with_max,
                                                      double* __restrict__ Zcos)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double mx = 1.0;
    if (with_max) {
        mx = Zin[n];
        for (int c = 1; c < d; ++c) mx = fmax(mx, Zin[(size_t)c * Np + n]);
    }
    double ss = 0.0;
    for (int c = 0; c < d; ++c) {
        double v = Zin[(size_t)c * Np + n];
        if (with_max) v = v / mx;
        ss = __dadd_rn(ss, __dmul_rn(v, v));
    }
    const double nrm = __dsqrt_rn(ss);
    for (int c = 0; c < d; ++c) {
        double v = Zin[(size_t)c * Np + n];
        if (with_max) v = v / mx;
        Zcos[(size_t)c * Np + n] = v / nrm;
    }
}

// ypart[chunk][k][c] = sum over the cells n of the chunk, ascending, of Zcos[c][n] R[k][n]; 16 clusters per workgroup
__global__ __launch_bounds__(256) void har_centroid_partial_kernel(const double* __restrict__ Zcos, const double* __restrict__ R,
                                                                   int N, int Np, int d, int K, double* __restrict__ ypart)
{
    __shared__ double Zs[64][33];
    __shared__ double Rs[16][33];
    const int tid = threadIdx.x, c = tid & 63, kq = tid >> 6;
    const int chunk = blockIdx.x, k0 = blockIdx.y * 16;
    const int n0 = chunk * HCH, n1 = min(N, n0 + HCH);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = n0; s < n1; s += 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i, cc = e >> 5, j = e & 31;
            Zs[cc][j] = (cc < d && s + j < n1) ? Zcos[(size_t)cc * Np + s + j] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i, kk = e >> 5, j = e & 31;
            Rs[kk][j] = (k0 + kk < K && s + j < n1) ? R[(size_t)(k0 + kk) * Np + s + j] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < 32; ++j) {
            const double z = Zs[c][j];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fma(z, Rs[kq * 4 + q][j], acc[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = k0 + kq * 4 + q;
        if (k < K && c < d) ypart[((size_t)chunk * K + k) * d + c] = acc[q];
    }
}

// one workgroup: Y[c][k] = the chunk partials added in chunk order, then every centroid divided by its L2 norm
__global__ __launch_bounds__(256) void har_centroid_final_kernel(const double* __restrict__ ypart, int nchunk, int d, int K,
                                                                 double* Y)
{
    for (int idx = threadIdx.x; idx < K * d; idx += 256) {
        const int k = idx / d, c = idx % d;
        double s = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) s += ypart[((size_t)ch * K + k) * d + c];
        Y[c * K + k] = s;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        double ss = 0.0;
        for (int c = 0; c < d; ++c) ss = __dadd_rn(ss, __dmul_rn(Y[c * K + k], Y[c * K + k]));
        const double nrm = __dsqrt_rn(ss);
        for (int c = 0; c < d; ++c) Y[c * K + k] = Y[c * K + k] / nrm;
    }
}

// one thread per cell, its scores in registers (D = d rounded up to 16, 32 or 64)
template <int D>
__global__ __launch_bounds__(256) void har_dist_kernel(const double* __restrict__ Zcos, const double* __restrict__ Y,
                                                       const double* __restrict__ sigma, int N, int Np, int d, int K,
                                                       double* __restrict__ dist, double* __restrict__ S, double* __restrict__ R)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = c < d ? Zcos[(size_t)c * Np + n] : 0.0;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c)
            if (c < d) acc = fma(Y[c * K + k], z[c], acc);
        const double dd = 2.0 * (1.0 - acc);
        dist[(size_t)k * Np + n] = dd;
        mx = fmax(mx, -dd / sigma[k]);
    }
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double e = exp(-dist[(size_t)k * Np + n] / sigma[k] - mx);
        S[(size_t)k * Np + n] = e;
        sum += e;
    }
    if (R)
        for (int k = 0; k < K; ++k) R[(size_t)k * Np + n] = S[(size_t)k * Np + n] / sum;
}

// part[blockIdx.y][sub][k][b]: over the positions [p0, p1) of sub-chunk `sub` of block blk0 + blockIdx.y, ascending, the
// sum of R[k][cell] over the cells whose level is b (b < B), over all of them (b == B).  perm == NULL: the cell order
// itself (nb = 1).  A sub-chunk past the end of its block (an empty block too) writes zeros.
__global__ __launch_bounds__(256) void har_levelsum_kernel(const double* __restrict__ R, const int* __restrict__ codes,
                                                           const int* __restrict__ lvar, const int* __restrict__ perm,
                                                           int blk0, int nb, int N, int Np, int K, int B, int nsub,
                                                           double* __restrict__ part)
{
    __shared__ double Rs[16][HSC + 1];
    __shared__ int cell[HSC];
    const int tid = threadIdx.x, sub = blockIdx.x, blk = blk0 + blockIdx.y, k0 = blockIdx.z * 16;
    const int p0 = min(har_off(blk, N, nb) + sub * HSC, har_off(blk + 1, N, nb));
    const int p1 = min(har_off(blk + 1, N, nb), p0 + HSC);
    const int cnt = p1 - p0;
    if (tid < cnt) cell[tid] = perm ? perm[p0 + tid] : p0 + tid;
    __syncthreads();
    for (int e = tid; e < 16 * HSC; e += 256) {
        const int kk = e / HSC, i = e % HSC;
        Rs[kk][i] = (k0 + kk < K && i < cnt) ? R[(size_t)(k0 + kk) * Np + cell[i]] : 0.0;
    }
    __syncthreads();
    const int kk = tid >> 4, slot = tid & 15;
    if (k0 + kk >= K) return;
    double* out = part + (((size_t)blockIdx.y * nsub + sub) * K + k0 + kk) * (B + 1);
    for (int b = slot; b <= B; b += 16) {
        double s = 0.0;
        if (b == B) {
            for (int i = 0; i < cnt; ++i) s += Rs[kk][i];
        } else {
            const int* cv = codes + (size_t)lvar[b] * Np;
            for (int i = 0; i < cnt; ++i)
                if (cv[cell[i]] == b) s += Rs[kk][i];
        }
        out[b] = s;
    }
}

// one workgroup.  With `add` (the sums of the block just updated): E += outer(sum, Pr_b), O += level sums; then with `sub`
// (the sums of the next block's old R): E -=, O -= and ratio = ((E + 1) / (O + 1))^theta.  The nsub partials of a block are
// added in sub-chunk order; the product and the sum round separately, as numpy's outer() followed by += does.
__global__ __launch_bounds__(256) void har_eo_kernel(const double* __restrict__ add, const double* __restrict__ sub, int nsub,
                                                     int K, int B, const double* __restrict__ prb,
                                                     const double* __restrict__ theta, double* __restrict__ E,
                                                     double* __restrict__ O, double* __restrict__ ratio)
{
    for (int idx = threadIdx.x; idx < K * B; idx += 256) {
        const int k = idx / B, b = idx % B;
        double e = E[idx], o = O[idx];
        if (add) {
            double tot = 0.0, lv = 0.0;
            for (int s = 0; s < nsub; ++s) {
                const double* p = add + ((size_t)s * K + k) * (B + 1);
                tot += p[B]; lv += p[b];
            }
            e = __dadd_rn(e, __dmul_rn(tot, prb[b]));
            o = __dadd_rn(o, lv);
        }
        if (sub) {
            double tot = 0.0, lv = 0.0;
            for (int s = 0; s < nsub; ++s) {
                const double* p = sub + ((size_t)s * K + k) * (B + 1);
                tot += p[B]; lv += p[b];
            }
            e = __dsub_rn(e, __dmul_rn(tot, prb[b]));
            o = __dsub_rn(o, lv);
            ratio[idx] = pow((e + 1.0) / (o + 1.0), theta[b]);
        }
        E[idx] = e; O[idx] = o;
    }
}

// one thread per position of [p0, p1): R[:, cell] = S[:, cell] * sum over the variables of ratio[:, its level], then
// divided by its L1 norm
__global__ __launch_bounds__(256) void har_update_kernel(const double* __restrict__ S, const double* __restrict__ ratio,
                                                         const int* __restrict__ codes, const int* __restrict__ perm,
                                                         int p0, int p1, int Np, int K, int V, int B, double* __restrict__ R)
{
    const int p = p0 + blockIdx.x * 256 + threadIdx.x;
    if (p >= p1) return;
    const int n = perm[p];
    double l1 = 0.0;
    for (int k = 0; k < K; ++k) {
        double f = 0.0;
        for (int v = 0; v < V; ++v) f += ratio[k * B + codes[(size_t)v * Np + n]];
        const double val = S[(size_t)k * Np + n] * f;
        R[(size_t)k * Np + n] = val;
        l1 += fabs(val);
    }
    for (int k = 0; k < K; ++k) R[(size_t)k * Np + n] = R[(size_t)k * Np + n] / l1;
}

__global__ __launch_bounds__(256) void har_tab_kernel(const double* __restrict__ E, const double* __restrict__ O,
                                                      const double* __restrict__ theta, int K, int B, double* __restrict__ tab)
{
    for (int idx = threadIdx.x; idx < K * B; idx += 256)
        tab[idx] = theta[idx % B] * log((O[idx] + 1.0) / (E[idx] + 1.0));
}

// opart[chunk][3]: sum R dist, sum sigma R log R (0 where not finite), sum sigma R (theta log((O + 1) / (E + 1)) Phi), over
// the HCH cells of the chunk: two cells per thread, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void har_obj_partial_kernel(const double* __restrict__ R, const double* __restrict__ dist,
                                                              const double* __restrict__ sigma, const double* __restrict__ tab,
                                                              const int* __restrict__ codes, int N, int Np, int K, int V,
                                                              int B, double* __restrict__ opart)
{
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < HCH / 256; ++j) {
        const int n = blockIdx.x * HCH + j * 256 + tid;
        if (n >= N) continue;
        for (int k = 0; k < K; ++k) {
            const double r = R[(size_t)k * Np + n];
            a0 += r * dist[(size_t)k * Np + n];
            double lg = r * log(r);
            if (!isfinite(lg)) lg = 0.0;
            a1 += sigma[k] * lg;
            double f = 0.0;
            for (int v = 0; v < V; ++v) f += tab[k * B + codes[(size_t)v * Np + n]];
            a2 += sigma[k] * r * f;
        }
    }
    red[0][tid] = a0; red[1][tid] = a1; red[2][tid] = a2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) opart[(size_t)blockIdx.x * 3 + tid] = red[tid][0];
}

__global__ void har_obj_final_kernel(const double* __restrict__ opart, int nchunk, double* __restrict__ obj)
{
    const int j = threadIdx.x;
    if (j >= 3) return;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += opart[(size_t)ch * 3 + j];
    obj[j] = s;
}

// Rt [N][K] = R^T and Pt [N][B + 1] = Phi_moe^T (a one, then the one-hot levels) for the ridge products
__global__ __launch_bounds__(256) void har_pack_kernel(const double* __restrict__ R, const int* __restrict__ codes, int N,
                                                       int Np, int K, int V, int B, double* __restrict__ Rt,
                                                       double* __restrict__ Pt)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    for (int k = 0; k < K; ++k) Rt[(size_t)n * K + k] = R[(size_t)k * Np + n];
    double* p = Pt + (size_t)n * (B + 1);
    p[0] = 1.0;
    for (int b = 0; b < B; ++b) p[1 + b] = 0.0;
    for (int v = 0; v < V; ++v) p[1 + codes[(size_t)v * Np + n]] = 1.0;
}

}  // namespace cnmf

static int har_need(cnmf_ctx* ctx, bool ready)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (ctx->har.N == 0) { SET_ERR(ctx, "cnmf_harmony_begin has not been called"); return CNMF_ESTATE; }
    if (ready && !ctx->har.ready) { SET_ERR(ctx, "cnmf_harmony_init has not been called"); return CNMF_ESTATE; }
    return CNMF_OK;
}

static inline unsigned har_cells_grid(int N) { return (unsigned)((N + 255) / 256); }

static void har_launch_dist(cnmf_ctx* ctx, bool init)
{
    using namespace cnmf;
    HarStage& H = ctx->har;
    hipStream_t st = ctx->stream;
    double* R = init ? H.R : nullptr;
    const unsigned grid = har_cells_grid(H.N);
    if (H.d <= 16) har_dist_kernel<16><<<grid, 256, 0, st>>>(H.Zcos, H.Y, H.sigma, H.N, H.Np, H.d, H.K, H.dist, H.S, R);
    else if (H.d <= 32) har_dist_kernel<32><<<grid, 256, 0, st>>>(H.Zcos, H.Y, H.sigma, H.N, H.Np, H.d, H.K, H.dist, H.S, R);
    else har_dist_kernel<64><<<grid, 256, 0, st>>>(H.Zcos, H.Y, H.sigma, H.N, H.Np, H.d, H.K, H.dist, H.S, R);
}

// the three objective terms of the current R, dist, E and O into host memory
static int har_objective(cnmf_ctx* ctx, double* objective)
{
    using namespace cnmf;
    HarStage& H = ctx->har;
    hipStream_t st = ctx->stream;
    const int nchunk = (H.N + HCH - 1) / HCH;
    har_tab_kernel<<<1, 256, 0, st>>>(H.E, H.O, H.theta, H.K, H.B, H.tab);
    har_obj_partial_kernel<<<nchunk, 256, 0, st>>>(H.R, H.dist, H.sigma, H.tab, H.codes, H.N, H.Np, H.K, H.V, H.B, H.opart);
    har_obj_final_kernel<<<1, 64, 0, st>>>(H.opart, nchunk, H.obj);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(objective, H.obj, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_harmony_begin(cnmf_ctx* ctx, int64_t n_cells, int32_t d, int32_t K, int32_t n_vars, int32_t n_levels,
                                  const double* pca, const int32_t* codes, const int32_t* level_var, const double* theta,
                                  const double* sigma, const double* pr_b)
{
    using namespace cnmf;
    if (!ctx || !pca || !codes || !level_var || !theta || !sigma || !pr_b) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (n_cells <= 0 || n_cells > (1ll << 26) || d <= 0 || K <= 0 || n_vars <= 0 || n_levels < n_vars) {
        SET_ERR(ctx, "bad shape: %lld cells, d = %d, K = %d, %d variables, %d levels", (long long)n_cells, d, K, n_vars, n_levels);
        return CNMF_EINVAL;
    }
    if (d > CNMF_HARMONY_DMAX || K > CNMF_HARMONY_KMAX || (long long)K * (n_levels + 1) > CNMF_RIDGE_MAX) {
        SET_ERR(ctx, "d = %d above %d, K = %d above %d or K * (B + 1) = %lld above %d", d, CNMF_HARMONY_DMAX, K,
                CNMF_HARMONY_KMAX, (long long)K * (n_levels + 1), CNMF_RIDGE_MAX);
        return CNMF_EUNSUPPORTED;
    }
    const int N = (int)n_cells, V = n_vars, B = n_levels, Np = round_up(N, 64);
    for (int b = 0; b < B; ++b)
        if (level_var[b] < 0 || level_var[b] >= V) { SET_ERR(ctx, "level %d names variable %d of %d", b, level_var[b], V); return CNMF_EINVAL; }
    for (int v = 0; v < V; ++v)
        for (int n = 0; n < N; ++n) {
            const int c = codes[(size_t)v * N + n];
            if (c < 0 || c >= B || level_var[c] != v) {
                SET_ERR(ctx, "cell %d has level %d for variable %d (%d levels)", n, c, v, B);
                return CNMF_EINVAL;
            }
        }
    for (int k = 0; k < K; ++k)
        if (!(sigma[k] > 0.0)) { SET_ERR(ctx, "sigma[%d] = %g must be positive", k, sigma[k]); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HarStage& H = ctx->har;
    H.release();
    const int nchunk = (N + HCH - 1) / HCH;
    const size_t dn = (size_t)d * Np, kn = (size_t)K * Np, kb = (size_t)K * B;
    hipError_t e = hipSuccess;
    auto dalloc = [&](double** p, size_t n) {
        if (e != hipSuccess) return;
        e = hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(double));
        if (e == hipSuccess) e = hipMemsetAsync(*p, 0, std::max<size_t>(n, 1) * sizeof(double), st);
    };
    auto ialloc = [&](int** p, size_t n) {
        if (e != hipSuccess) return;
        e = hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(int));
        if (e == hipSuccess) e = hipMemsetAsync(*p, 0, std::max<size_t>(n, 1) * sizeof(int), st);
    };
    H.N = N;                                         // (so that release() on a failure below frees what was made)
    dalloc(&H.Zo, dn); dalloc(&H.Zcos, dn); dalloc(&H.Zcorr, dn);
    dalloc(&H.R, kn); dalloc(&H.dist, kn); dalloc(&H.S, kn);
    dalloc(&H.ZoT, (size_t)N * d); dalloc(&H.ZcT, (size_t)N * d); dalloc(&H.Rt, (size_t)N * K); dalloc(&H.Pt, (size_t)N * (B + 1));
    dalloc(&H.Y, (size_t)d * K); dalloc(&H.theta, B); dalloc(&H.sigma, K); dalloc(&H.prb, B);
    dalloc(&H.E, kb); dalloc(&H.O, kb); dalloc(&H.tab, kb); dalloc(&H.obj, 3);
    dalloc(&H.ypart, (size_t)nchunk * K * d); dalloc(&H.opart, (size_t)nchunk * 3);
    ialloc(&H.codes, (size_t)V * Np); ialloc(&H.lvar, B); ialloc(&H.perm, N);
    if (e == hipSuccess) e = hipMemcpyAsync(H.ZoT, pca, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(H.codes, (size_t)Np * sizeof(int), codes, (size_t)N * sizeof(int),
                                              (size_t)N * sizeof(int), V, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(H.lvar, level_var, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(H.theta, theta, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(H.sigma, sigma, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(H.prb, pr_b, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { H.release(); HIP_TRY(ctx, e); }
    H.Np = Np; H.d = d; H.K = K; H.V = V; H.B = B;
    har_transpose_in_kernel<<<har_cells_grid(N), 256, 0, st>>>(H.ZoT, N, Np, d, H.Zo);
    har_cos_kernel<<<har_cells_grid(N), 256, 0, st>>>(H.Zo, N, Np, d, 1, H.Zcos);
    e = hipMemcpyAsync(H.Zcorr, H.Zo, dn * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { H.release(); HIP_TRY(ctx, e); }
    return CNMF_OK;
}

// grows a buffer of level-sum partials to `need` doubles
static int har_part(cnmf_ctx* ctx, double** p, size_t* cap, size_t need)
{
    if (*cap >= need) return CNMF_OK;
    hipFree(*p); *p = nullptr; *cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)p, need * sizeof(double)));
    *cap = need;
    return CNMF_OK;
}

extern "C" int cnmf_harmony_init(cnmf_ctx* ctx, const double* Y, double* objective)
{
    using namespace cnmf;
    if (int rc = har_need(ctx, false)) return rc;
    if (!Y || !objective) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HarStage& H = ctx->har;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nsub = (H.N + HSC - 1) / HSC, kt = (H.K + 15) / 16;
    if (int rc = har_part(ctx, &H.part_new, &H.part_new_cap, (size_t)nsub * H.K * (H.B + 1))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(H.Y, Y, (size_t)H.d * H.K * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(H.E, 0, (size_t)H.K * H.B * sizeof(double), st));
    HIP_TRY(ctx, hipMemsetAsync(H.O, 0, (size_t)H.K * H.B * sizeof(double), st));
    har_launch_dist(ctx, true);
    har_levelsum_kernel<<<dim3(nsub, 1, kt), 256, 0, st>>>(H.R, H.codes, H.lvar, nullptr, 0, 1, H.N, H.Np, H.K, H.B, nsub,
                                                           H.part_new);
    har_eo_kernel<<<1, 256, 0, st>>>(H.part_new, nullptr, nsub, H.K, H.B, H.prb, H.theta, H.E, H.O, H.tab);
    HIP_TRY(ctx, hipGetLastError());
    if (int rc = har_objective(ctx, objective)) return rc;
    H.ready = true;
    return CNMF_OK;
}

extern "C" int cnmf_harmony_kmeans_step(cnmf_ctx* ctx, const int32_t* perm, int32_t n_blocks, double* objective)
{
    using namespace cnmf;
    if (int rc = har_need(ctx, true)) return rc;
    if (!perm || !objective) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HarStage& H = ctx->har;
    const int N = H.N, K = H.K, B = H.B, nb = n_blocks;
    if (nb < 1 || nb > 4096) { SET_ERR(ctx, "%d blocks outside [1, 4096]", nb); return CNMF_EINVAL; }
    {
        std::vector<char> seen((size_t)N, 0);
        for (int i = 0; i < N; ++i) {
            if (perm[i] < 0 || perm[i] >= N || seen[perm[i]]) { SET_ERR(ctx, "perm is not a permutation of %d cells", N); return CNMF_EINVAL; }
            seen[perm[i]] = 1;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nchunk = (N + HCH - 1) / HCH, kt = (K + 15) / 16;
    const int nsub = std::max(1, ((N + nb - 1) / nb + HSC - 1) / HSC);      // sub-chunks of the largest block
    const size_t per_block = (size_t)nsub * K * (B + 1);
    if (int rc = har_part(ctx, &H.part_old, &H.part_old_cap, per_block * nb)) return rc;
    if (int rc = har_part(ctx, &H.part_new, &H.part_new_cap, per_block)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(H.perm, perm, (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
    // Y = Z_cos R^T, normalised; dist and S from it
    har_centroid_partial_kernel<<<dim3(nchunk, kt), 256, 0, st>>>(H.Zcos, H.R, N, H.Np, H.d, K, H.ypart);
    har_centroid_final_kernel<<<1, 256, 0, st>>>(H.ypart, nchunk, H.d, K, H.Y);
    har_launch_dist(ctx, false);
    // update_R: the sums of every block's old R, then block after block (H.tab holds the ratio table here, and
    // theta log((O + 1) / (E + 1)) for the objective after it)
    har_levelsum_kernel<<<dim3(nsub, nb, kt), 256, 0, st>>>(H.R, H.codes, H.lvar, H.perm, 0, nb, N, H.Np, K, B, nsub, H.part_old);
    for (int i = 0; i < nb; ++i) {
        const int p0 = har_off(i, N, nb), p1 = har_off(i + 1, N, nb);
        har_eo_kernel<<<1, 256, 0, st>>>(i > 0 ? H.part_new : nullptr, H.part_old + per_block * i, nsub, K, B, H.prb, H.theta,
                                         H.E, H.O, H.tab);
        if (p1 > p0)
            har_update_kernel<<<(p1 - p0 + 255) / 256, 256, 0, st>>>(H.S, H.tab, H.codes, H.perm, p0, p1, H.Np, K, H.V, B, H.R);
        har_levelsum_kernel<<<dim3(nsub, 1, kt), 256, 0, st>>>(H.R, H.codes, H.lvar, H.perm, i, nb, N, H.Np, K, B, nsub,
                                                               H.part_new);
    }
    har_eo_kernel<<<1, 256, 0, st>>>(H.part_new, nullptr, nsub, K, B, H.prb, H.theta, H.E, H.O, H.tab);
    HIP_TRY(ctx, hipGetLastError());
    return har_objective(ctx, objective);
}

// the moments of the ridge step over Z_orig^T with the current R: M [K*B1][d], gram [K*B1][B1] (cnmf_preprocess_ridge_moments)
extern "C" int cnmf_harmony_ridge_moments(cnmf_ctx* ctx, double* M, double* gram)
{
    using namespace cnmf;
    if (int rc = har_need(ctx, true)) return rc;
    if (!M || !gram) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HarStage& H = ctx->har;
    const int B1 = H.B + 1, KB = H.K * B1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dM = pool.get<double>((size_t)KB * H.d);
    double* dG = pool.get<double>((size_t)KB * B1);
    POOL_TRY(ctx, pool);
    har_pack_kernel<<<har_cells_grid(H.N), 256, 0, st>>>(H.R, H.codes, H.N, H.Np, H.K, H.V, H.B, H.Rt, H.Pt);
    HIP_TRY(ctx, hipGetLastError());
    PreGemm g{};
    g.M = KB; g.Nn = H.d; g.K = H.N; g.Rt = H.Rt; g.Pt = H.Pt; g.KR = H.K; g.B1 = B1; g.Bm = H.ZoT; g.ldb = H.d;
    if (int rc = pre_product<1, 0>(ctx, g, dM)) return rc;
    g.Nn = B1; g.Bm = H.Pt; g.ldb = B1;
    if (int rc = pre_product<1, 0>(ctx, g, dG)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(M, dM, (size_t)KB * H.d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(gram, dG, (size_t)KB * B1 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

// Z_corr = Z_orig - W^T A (the factors of the last moments, no clip), Z_cos = Z_corr with every cell at unit L2 norm
extern "C" int cnmf_harmony_ridge_apply(cnmf_ctx* ctx, const double* W)
{
    using namespace cnmf;
    if (int rc = har_need(ctx, true)) return rc;
    if (!W) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HarStage& H = ctx->har;
    const int B1 = H.B + 1, KB = H.K * B1, N = H.N, d = H.d;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dW = pool.get<double>((size_t)KB * d);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dW, W, (size_t)KB * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(H.ZcT, H.ZoT, (size_t)N * d * sizeof(double), hipMemcpyDeviceToDevice, st));
    PreGemm g{};
    g.M = N; g.Nn = d; g.K = KB; g.kps = KB; g.X = H.ZcT; g.ldx = d; g.Rt = H.Rt; g.Pt = H.Pt; g.KR = H.K; g.B1 = B1;
    g.Bm = dW; g.ldb = d;
    pre_gemm_kernel<3, 0, 2><<<dim3((d + 63) / 64, (N + 63) / 64, 1), 256, 0, st>>>(g);
    har_transpose_in_kernel<<<har_cells_grid(N), 256, 0, st>>>(H.ZcT, N, H.Np, d, H.Zcorr);
    har_cos_kernel<<<har_cells_grid(N), 256, 0, st>>>(H.Zcorr, N, H.Np, d, 0, H.Zcos);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

// any of the outputs may be NULL: Z_corr [d][N], Z_cos [d][N], R [K][N], Y [d][K]
extern "C" int cnmf_harmony_fetch(cnmf_ctx* ctx, double* Z_corr, double* Z_cos, double* R, double* Y)
{
    if (int rc = har_need(ctx, false)) return rc;
    HarStage& H = ctx->har;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t row = (size_t)H.N * sizeof(double), prow = (size_t)H.Np * sizeof(double);
    if (Z_corr) HIP_TRY(ctx, hipMemcpy2DAsync(Z_corr, row, H.Zcorr, prow, row, H.d, hipMemcpyDeviceToHost, st));
    if (Z_cos) HIP_TRY(ctx, hipMemcpy2DAsync(Z_cos, row, H.Zcos, prow, row, H.d, hipMemcpyDeviceToHost, st));
    if (R) HIP_TRY(ctx, hipMemcpy2DAsync(R, row, H.R, prow, row, H.K, hipMemcpyDeviceToHost, st));
    if (Y) HIP_TRY(ctx, hipMemcpyAsync(Y, H.Y, (size_t)H.d * H.K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_harmony_release(cnmf_ctx* ctx)
{
    if (!ctx) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->har.release();
    return CNMF_OK;
}
