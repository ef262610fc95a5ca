// The top eigenpairs of a symmetric float64 matrix without a dense eigen-solve on the host (Preprocess's PCA with
// pca="device"): Householder tridiagonalisation on the device, the tridiagonal eigenproblem on the host
// (scipy.linalg.eigh_tridiagonal, O(n n_comp)), back-transformation of the kept vectors, the PCA sign rule and the
// scores on the device.  The scatter matrix of a slot never leaves the device and V is never uploaded.
//
// Tridiagonalisation, LAPACK's convention (dsytd2 / dlarfg, lower form): for column k with x = A[k+1:, k], alpha = x[0]:
//   beta = -sign(alpha) hypot(alpha, |x[1:]|),  v = x / (alpha - beta) with v[0] = 1,  tau = (beta - alpha) / beta,
//   e[k] = beta;  a zero tail: tau = 0, e[k] = alpha;  then with p = A22 v:  w = tau p - (tau / 2)(tau p^T v) v,
//   A22 -= v w^T + w v^T.
// ONE launch per column, by deferring the rank-2 update: launch k first lets every workgroup form, redundantly and in
// one fixed summation order (so that all of them hold the same bits), (a) w_{k-1} from the raw product p_{k-1}, the
// reflector v_{k-1} and tau_{k-1} of the launch before, (b) row k as the pending update leaves it (read only: nobody
// writes row k in launch k) and (c) v_k, tau_k, beta_k from that row's tail.  Then a wavefront per row i > k applies
// the pending update in place to the columns j > k and writes p_k[i] = sum_{j > k} A[i][j] v_k[j].  Workgroup 0 alone
// writes d[k], e[k], tau_k and v_k.  p is a ping-pong pair and v_k goes into a separate n x n reflector store (row k,
// entries k+1 .. n-1, the leading 1 stored): what launch k reads of launch k - 1 was complete at the launch boundary.
// Every cross-workgroup dependency is a launch boundary: no grid barrier, no cooperative launch, no spin-wait, no
// atomics.  The host issues the n launches in stream order without synchronising in between.
// Both triangles of the working matrix are kept; the update of (i, j) and of (j, i) is the same sum of the same two
// rounded products, so the matrix stays symmetric to the bit.
//
// Back-transformation: one workgroup per kept column, the column in LDS (n <= CNMF_PCA_NMAX = 8192: 64 KB); for
// k = n-3 .. 0: z[k+1:] -= tau_k v_k (v_k^T z[k+1:]); a thread owns the entries j = t (mod 256) throughout, so the
// only barrier of a step is the one inside the dot product.  The same workgroup then applies the PCA sign rule (the
// entry of largest magnitude positive, the first index on ties: np.argmax(np.abs(V), axis=0)).
//
// Included by cnmf_hip.hip (after preprocess_host.hip.h).
#pragma once

namespace cnmf {

// the sum of v over the 256 threads in a fixed order; every thread returns the same bits.  red [4] must not be
// rewritten before every thread has read it (the callers alternate between two of them)
__device__ __forceinline__ double tri_block_sum(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

struct TriArgs {
    int n, k;
    double* A;                  // [n][n] working matrix
    double* R;                  // [n][n] reflector store
    double* tau;                // [n]
    double *d, *e;              // [n], [n - 1]
    const double* p_prev;       // p_{k-1} [n]
    double* p_cur;              // p_k [n]
};

// dynamic LDS: w_{k-1}[k ..] (m = n - k doubles), v_k[k ..] (m; entry 0 unused), two reduction scratches (8)
__global__ __launch_bounds__(256) void tri_column_kernel(const TriArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double tri_lds[];
    const int n = a.n, k = a.k, m = n - k, t = threadIdx.x;
    double* wS = tri_lds;
    double* vS = tri_lds + m;
    double* red = tri_lds + 2 * (size_t)m;
    const double* vp = k > 0 ? a.R + (size_t)(k - 1) * n : a.R;       // v_{k-1}: entries k .. n-1, entry k is 1
    const double taup = k > 0 ? a.tau[k - 1] : 0.0;
    const bool pend = taup != 0.0;                                    // (uniform over the grid)
    // (a) w_{k-1} over the rows k .. n-1
    if (pend) {
        double s = 0.0;
        for (int i = k + t; i < n; i += 256) s += a.p_prev[i] * vp[i];
        const double dot = tri_block_sum(s, red);
        const double c = 0.5 * taup * (taup * dot);
        for (int i = k + t; i < n; i += 256) wS[i - k] = taup * a.p_prev[i] - c * vp[i];
    } else {
        for (int q = t; q < m; q += 256) wS[q] = 0.0;
    }
    __syncthreads();
    // (b) row k as the pending update leaves it, into vS; the squared norm of its tail behind alpha
    const double* rowk = a.A + (size_t)k * n;
    const double wk = wS[0], vk = pend ? vp[k] : 0.0;
    double ss = 0.0;
    for (int j = k + t; j < n; j += 256) {
        double r = rowk[j];
        if (pend) r = __dsub_rn(r, __dadd_rn(__dmul_rn(vk, wS[j - k]), __dmul_rn(wk, vp[j])));
        vS[j - k] = r;
        if (j >= k + 2) ss += r * r;
    }
    const double x2 = tri_block_sum(ss, red + 4);                     // (its barrier publishes vS)
    // (c) the reflector of column k
    const double dk = vS[0];
    const bool has_e = m >= 2;
    double tau = 0.0, beta = 0.0, den = 1.0;
    if (has_e) {
        const double alpha = vS[1];
        beta = alpha;
        if (m >= 3 && x2 != 0.0) {
            beta = -copysign(hypot(alpha, sqrt(x2)), alpha);
            tau = (beta - alpha) / beta;
            den = alpha - beta;
        }
    }
    __syncthreads();                                                  // (vS[1] is read above, rewritten below)
    for (int q = 1 + t; q < m; q += 256) {
        const double v = q == 1 ? 1.0 : (tau != 0.0 ? vS[q] / den : 0.0);
        vS[q] = v;
        if (blockIdx.x == 0) a.R[(size_t)k * n + k + q] = v;
    }
    if (blockIdx.x == 0 && t == 0) {
        a.d[k] = dk;
        a.tau[k] = tau;
        if (has_e) a.e[k] = beta;
    }
    __syncthreads();
    // the rows i > k: the pending update on the columns j > k in place, then p_k[i].  Nothing pending and no reflector
    // (a column that is tridiagonal already): nothing to do, and p_k is never read (w_k = 0 whenever tau_k = 0)
    if (!pend && tau == 0.0) return;
    const int wave = t >> 6, lane = t & 63, nw = (int)gridDim.x * 4;
    for (int i = k + 1 + (int)blockIdx.x * 4 + wave; i < n; i += nw) {
        double* row = a.A + (size_t)i * n;
        const double wi = wS[i - k], vi = pend ? vp[i] : 0.0;
        double acc = 0.0;
        for (int j = k + 1 + lane; j < n; j += 64) {
            double x = row[j];
            if (pend) {
                x = __dsub_rn(x, __dadd_rn(__dmul_rn(vi, wS[j - k]), __dmul_rn(wi, vp[j])));
                row[j] = x;
            }
            acc += x * vS[j - k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) a.p_cur[i] = acc;
    }
}

// dynamic LDS: the column z (n doubles), two reduction scratches (8), the arg-max scratch (4 doubles + 4 ints)
__global__ __launch_bounds__(256) void tri_back_kernel(int n, int n_comp, const double* __restrict__ R,
                                                       const double* __restrict__ tau, const double* __restrict__ Z,
                                                       int sign_rule, double* __restrict__ V)
{
    extern __shared__ __attribute__((aligned(16))) double tri_lds[];
    double* z = tri_lds;
    double* red = tri_lds + n;
    double* amax = red + 8;
    int* aidx = (int*)(amax + 4);
    const int c = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int j = t; j < n; j += 256) z[j] = Z[(size_t)j * n_comp + c];
    int par = 0;
    for (int k = n - 3; k >= 0; --k) {
        const double tk = tau[k];
        if (tk == 0.0) continue;                                      // (uniform)
        const double* v = R + (size_t)k * n;
        const int j0 = k + 1 + ((t - (k + 1)) & 255);                 // the first j > k with j = t (mod 256)
        double s = 0.0;
        for (int j = j0; j < n; j += 256) s += v[j] * z[j];
        const double f = tk * tri_block_sum(s, red + 4 * par);
        for (int j = j0; j < n; j += 256) z[j] -= f * v[j];
        par ^= 1;
    }
    bool flip = false;
    if (sign_rule) {
        double best = -1.0;
        int bi = n;
        for (int j = t; j < n; j += 256) {
            const double x = fabs(z[j]);
            if (x > best) { best = x; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_down(best, o, 64);
            const int oi = __shfl_down(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { amax[wave] = best; aidx[wave] = bi; }
        __syncthreads();                                              // (also: every z entry is final)
        best = amax[0]; bi = aidx[0];
        for (int w = 1; w < 4; ++w)
            if (amax[w] > best || (amax[w] == best && aidx[w] < bi)) { best = amax[w]; bi = aidx[w]; }
        flip = bi < n && z[bi] < 0.0;
    }
    for (int j = t; j < n; j += 256) V[(size_t)j * n_comp + c] = flip ? -z[j] : z[j];
}

constexpr int TRI_COLUMN_LDS_MAX = (2 * CNMF_PCA_NMAX + 8) * (int)sizeof(double);
constexpr int TRI_BACK_LDS_MAX = (CNMF_PCA_NMAX + 16) * (int)sizeof(double);

}  // namespace cnmf

static int tri_size_arg(cnmf_ctx* ctx, long long n)
{
    if (n < 1) { SET_ERR(ctx, "n = %lld must be positive", n); return CNMF_EINVAL; }
    if (n > CNMF_PCA_NMAX) {
        SET_ERR(ctx, "n = %lld above %d (the back-transformation holds a column in LDS)", n, CNMF_PCA_NMAX);
        return CNMF_EUNSUPPORTED;
    }
    return CNMF_OK;
}

// replaces the staged tridiagonalisation by empty arrays for an n x n matrix
static int tri_alloc(cnmf_ctx* ctx, int n)
{
    PreStage& P = ctx->pre;
    hipStreamSynchronize(ctx->stream);
    P.release_tridiag();
    const size_t nn = (size_t)n * n * sizeof(double);
    hipError_t e = hipMalloc((void**)&P.triA, nn);
    if (e == hipSuccess) e = hipMalloc((void**)&P.triR, nn);
    if (e == hipSuccess) e = hipMalloc((void**)&P.tri_tau, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P.tri_mu, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P.tri_d, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P.tri_e, (size_t)n * sizeof(double));
    if (e != hipSuccess) P.release_tridiag();
    HIP_TRY(ctx, e);
    P.tri_n = n;
    return CNMF_OK;
}

// P.triA (filled) -> tridiagonal: the reflectors into P.triR / P.tri_tau, d [n] and e [n - 1] into P.tri_d / P.tri_e (they
// stay staged for tridiag_eig_host.hip.h).  Launches only; p is released when the launches have run
static int tri_reduce_launch(cnmf_ctx* ctx)
{
    using namespace cnmf;
    PreStage& P = ctx->pre;
    hipStream_t st = ctx->stream;
    const int n = P.tri_n;
    DevPool pool;
    double* p = pool.get<double>(2 * (size_t)n);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, dyn_lds_optin((const void*)tri_column_kernel, TRI_COLUMN_LDS_MAX));
    TriArgs a{};
    a.n = n; a.A = P.triA; a.R = P.triR; a.tau = P.tri_tau; a.d = P.tri_d; a.e = P.tri_e;
    for (int k = 0; k < n; ++k) {
        const int m = n - k;
        a.k = k; a.p_prev = p + (size_t)((k + 1) & 1) * n; a.p_cur = p + (size_t)(k & 1) * n;
        const int grid = std::max(1, std::min(256, (m - 1 + 3) / 4));          // (a function of n and k alone)
        tri_column_kernel<<<grid, 256, (2 * (size_t)m + 8) * sizeof(double), st>>>(a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// the staged d [n] and e [n - 1] to the host
static int tri_fetch(cnmf_ctx* ctx, double* d, double* e)
{
    PreStage& P = ctx->pre;
    hipStream_t st = ctx->stream;
    const int n = P.tri_n;
    HIP_TRY(ctx, hipMemcpyAsync(d, P.tri_d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n > 1) HIP_TRY(ctx, hipMemcpyAsync(e, P.tri_e, (size_t)(n - 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

static int tri_reduce(cnmf_ctx* ctx, double* d, double* e)
{
    if (int rc = tri_reduce_launch(ctx)) return rc;
    return tri_fetch(ctx, d, e);
}

// dV [n][n_comp] (device) = the back-transformed columns of dZ [n][n_comp] (device)
static int tri_back_launch(cnmf_ctx* ctx, int n_comp, const double* dZ, int sign_rule, double* dV)
{
    using namespace cnmf;
    PreStage& P = ctx->pre;
    const int n = P.tri_n;
    HIP_TRY(ctx, dyn_lds_optin((const void*)tri_back_kernel, TRI_BACK_LDS_MAX));
    tri_back_kernel<<<n_comp, 256, ((size_t)n + 16) * sizeof(double), ctx->stream>>>(n, n_comp, P.triR, P.tri_tau, dZ, sign_rule, dV);
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// the same for the host's Z [n][n_comp]; dZ: device scratch of that size
static int tri_back(cnmf_ctx* ctx, int n_comp, const double* Z, int sign_rule, double* dZ, double* dV)
{
    PreStage& P = ctx->pre;
    HIP_TRY(ctx, hipMemcpyAsync(dZ, Z, (size_t)P.tri_n * n_comp * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return tri_back_launch(ctx, n_comp, dZ, sign_rule, dV);
}

extern "C" int cnmf_symmetric_tridiagonalize(cnmf_ctx* ctx, int64_t n, const double* A, double* d, double* e)
{
    if (!ctx || !A || !d || (!e && n > 1)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = tri_size_arg(ctx, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = tri_alloc(ctx, (int)n)) return rc;
    PreStage& P = ctx->pre;
    P.tri_slot = -1;
    HIP_TRY(ctx, hipMemcpyAsync(P.triA, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return tri_reduce(ctx, d, e);
}

extern "C" int cnmf_tridiagonal_back_transform(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* Z, int32_t sign_rule,
                                               double* V)
{
    if (!ctx || !Z || !V) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (!P.triR) { SET_ERR(ctx, "no tridiagonalisation is staged"); return CNMF_EINVAL; }
    if (n != P.tri_n) { SET_ERR(ctx, "n = %lld where the staged tridiagonalisation has %d", (long long)n, P.tri_n); return CNMF_EINVAL; }
    if (n_comp < 1 || n_comp > n) { SET_ERR(ctx, "n_comp = %d outside [1, %lld]", n_comp, (long long)n); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    const size_t cnt = (size_t)n * n_comp;
    double* dZ = pool.get<double>(cnt);
    double* dV = pool.get<double>(cnt);
    POOL_TRY(ctx, pool);
    if (int rc = tri_back(ctx, n_comp, Z, sign_rule != 0, dZ, dV)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(V, dV, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_pca_tridiag(cnmf_ctx* ctx, int32_t slot, double* mean, double* d, double* e)
{
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    PreStage& P = ctx->pre;
    const int64_t n = P.slot[slot].n;
    if (!mean || !d || (!e && n > 1)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = tri_size_arg(ctx, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = tri_alloc(ctx, (int)n)) return rc;
    P.tri_slot = slot;
    if (int rc = pre_scatter_device(ctx, slot, P.tri_mu, P.triA)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(mean, P.tri_mu, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return tri_reduce(ctx, d, e);
}

extern "C" int cnmf_preprocess_pca_finish(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, const double* Z, double* V,
                                          double* scores)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!Z || !V || !scores) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    PreSlot& S = P.slot[slot];
    if (!P.triR || P.tri_slot != slot) { SET_ERR(ctx, "cnmf_preprocess_pca_tridiag has not been called on slot %d", slot); return CNMF_EINVAL; }
    if (S.n != P.tri_n) { SET_ERR(ctx, "slot %d has %lld columns where the staged tridiagonalisation has %d", slot, (long long)S.n, P.tri_n); return CNMF_EINVAL; }
    const int N = (int)P.N, C = (int)S.n;
    if (n_comp < 1 || n_comp > C) { SET_ERR(ctx, "n_comp = %d outside [1, %d]", n_comp, C); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    double* dZ = pool.get<double>((size_t)C * n_comp);
    double* dV = pool.get<double>((size_t)C * n_comp);
    double* out = pool.get<double>((size_t)N * n_comp);
    POOL_TRY(ctx, pool);
    if (int rc = tri_back(ctx, n_comp, Z, 1, dZ, dV)) return rc;
    PreGemm g{};
    g.M = N; g.Nn = n_comp; g.K = C; g.X = S.dense; g.ldx = C; g.mu = P.tri_mu; g.Bm = dV; g.ldb = n_comp;
    if (int rc = pre_product<2, 0>(ctx, g, out)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(V, dV, (size_t)C * n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(scores, out, (size_t)N * n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}
