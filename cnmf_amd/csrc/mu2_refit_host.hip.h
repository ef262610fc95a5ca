// Frobenius refit with the spectra fixed by MULTIPLICATIVE updates, in FLOAT64, on the dense image of the resident matrix.
//
// What it is for: projecting new cells onto a fixed set of programs (starCAT: Kotliar et al.), i.e.
//   non_negative_factorization(X, H=reference, update_H=False, solver='mu', beta_loss='frobenius')
// = scikit-learn's `_fit_multiplicative_update` with beta_loss = 2 and update_H = False (sklearn/decomposition/_nmf.py:731-893,
// `_multiplicative_update_w` :540-554 and :615-629, `_beta_divergence` :121-134).  With H fixed everything that touches X is
// constant: P = X H^T, Gram = H H^T and nX = sum x^2.  A row of W iterates on its own
//     w_t <- w_t * P_t / ( sum_r w_r Gram[r][t] + l1 + l2 w_t ),      a zero denominator replaced by float32 epsilon
// (every denominator of the row from the row's OLD values: Jacobi, not the Gauss-Seidel order of the coordinate-descent sweep)
// and only the stopping rule -- every 10 iterations, (previous - error) / error_at_init < tol -- couples the rows, through
//     error = sqrt( nX + sum_i sum_t w_it (W Gram)_it - 2 sum_i sum_t P_ti w_it )
// (scikit-learn's expansion for a sparse X, used here for every upload; not clamped, as scikit-learn does not clamp it).
//
// One launch runs a burst of up to ten iterations for its 64 rows (lane per row, the row's k values in an LDS strip of
// [k][64] doubles, a second strip for the row being formed, the Gram matrix read with wave-uniform loads, four components
// per pass over the strip) and leaves the workgroup's share of the two sums; a one-thread kernel adds the shares in block
// order and applies the rule into a small device state that later bursts read; the host polls that state.  Every sum runs
// in an order fixed by the shapes alone: two calls give the same bits.  Same layout as the float64 coordinate-descent
// refit of tail_host.hip.h (nnls_sweep_f64_kernel).  Included by cnmf_hip.hip after tail_host.hip.h.
#pragma once

namespace cnmf {

struct Mu2State { int iter; int done; double nx; double err0; double prev; double err; };

// part[b] = sum of x^2 over rows [64 b, 64 b + 64): a wave per row (rows 4 apart), lanes strided over the genes, butterfly,
// the four waves added in wave order
__global__ __launch_bounds__(256) void mu2_sumsq_kernel(const float* __restrict__ X, int ldx, int N, int G,
                                                        double* __restrict__ part)
{
    __shared__ double red[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = blockIdx.x * 64, r1 = min(r0 + 64, N);
    double s = 0.0;
    for (int r = r0 + w; r < r1; r += 4) {
        const float* x = X + (size_t)r * ldx;
        for (int g = lane; g < G; g += 64) { const double v = (double)x[g]; s = fma(v, v, s); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void mu2_fill_kernel(double* __restrict__ p, long long n, double v)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// acc[j] = sum_r w[r] Gram[r][t0 + j], j < 4, r ascending.  w: the lane's column of a strip (stride 64); gram rows padded
// with zeros to ldg = a multiple of 4, so a tile that overhangs k reads zeros
__device__ __forceinline__ void mu2_wg4(const double* w, const double* __restrict__ gram, int ldg, int k, int t0, double acc[4])
{
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    const double* g = gram + t0;
    for (int r = 0; r < k; ++r) {
        const double wr = w[r * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fma(wr, g[(size_t)r * ldg + j], acc[j]);
    }
}

// W, P: component-major [k][ld], L valid entries per row.  n_inner iterations of the rows of this workgroup, then (want_err)
// its shares part_ww[b] = sum w (W Gram), part_pw[b] = sum P w of the rows as they stand.
__global__ __launch_bounds__(64) void mu2_burst_f64_kernel(double* __restrict__ W, const double* __restrict__ P, int ld, int L,
                                                           int k, const double* __restrict__ gram, int ldg, double l1, double l2,
                                                           int n_inner, int want_err, double* __restrict__ part_ww,
                                                           double* __restrict__ part_pw, const Mu2State* __restrict__ state)
{
    if (state->done) return;
    extern __shared__ double mu2_ws[];                     // two strips [k][64]
    const int tid = threadIdx.x, row = blockIdx.x * 64 + tid;
    const bool live = row < L;
    const int rowc = min(row, L - 1);
    double* cur = mu2_ws + tid;
    double* nxt = mu2_ws + (size_t)k * 64 + tid;
    for (int t = 0; t < k; ++t) cur[t * 64] = live ? W[(size_t)t * ld + rowc] : 0.0;
    for (int it = 0; it < n_inner; ++it) {
        for (int t0 = 0; t0 < k; t0 += 4) {
            double den[4];
            mu2_wg4(cur, gram, ldg, k, t0, den);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = t0 + j;
                if (t < k) {
                    const double wt = cur[t * 64];
                    double d = den[j];
                    if (l1 > 0.0) d += l1;
                    if (l2 > 0.0) d += l2 * wt;
                    if (d == 0.0) d = MU_EPS32;
                    nxt[t * 64] = wt * (P[(size_t)t * ld + rowc] / d);
                }
            }
        }
        double* sw = cur; cur = nxt; nxt = sw;
    }
    if (n_inner > 0 && live)
        for (int t = 0; t < k; ++t) W[(size_t)t * ld + row] = cur[t * 64];
    if (want_err) {
        double a = 0.0, b = 0.0;
        for (int t0 = 0; t0 < k; t0 += 4) {
            double wg[4];
            mu2_wg4(cur, gram, ldg, k, t0, wg);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = t0 + j;
                if (t < k) {
                    const double wt = cur[t * 64];         // (a lane past the last row holds zeros: it adds nothing)
                    a = fma(wt, wg[j], a);
                    b = fma(P[(size_t)t * ld + rowc], wt, b);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (tid == 0) { part_ww[blockIdx.x] = a; part_pw[blockIdx.x] = b; }
    }
}

// mode 2: the start (nX from its partials, error_at_init); 1: a check after n_inner more iterations (_nmf.py:872-884);
// 0: n_inner more iterations without a check
__global__ __launch_bounds__(64) void mu2_decide_kernel(const double* __restrict__ part_ww, const double* __restrict__ part_pw,
                                                        int nparts, const double* __restrict__ part_x, double tol, int n_inner,
                                                        int mode, Mu2State* __restrict__ state)
{
    if (threadIdx.x != 0 || state->done) return;
    state->iter += n_inner;
    if (mode == 0) return;
    if (mode == 2) {
        double nx = 0.0;
        for (int p = 0; p < nparts; ++p) nx += part_x[p];
        state->nx = nx;
    }
    double a = 0.0, b = 0.0;
    for (int p = 0; p < nparts; ++p) { a += part_ww[p]; b += part_pw[p]; }
    const double err = sqrt((state->nx + a) - 2.0 * b);
    state->err = err;
    if (mode == 2) { state->err0 = err; state->prev = err; return; }
    if ((state->prev - err) / state->err0 < tol) state->done = 1;
    else state->prev = err;
}

}  // namespace cnmf

// H [k][G] float64 fixed, W_out [N][k] float64 from w_init everywhere.  prm: tol, max_iter, l1_reg_W, l2_reg_W.
// n_iter_out: iterations run; err_out: the last error evaluated (error_at_init when no check ran).
extern "C" int cnmf_mu2_refit_f64(cnmf_ctx* ctx, int k, const double* H, double w_init, const cnmf_cd_params* prm,
                                  double* W_out, int32_t* n_iter_out, double* err_out)
{
    using namespace cnmf;
    if (!ctx || !H || !W_out || k < 1) { SET_ERR(ctx, "bad argument"); return CNMF_EINVAL; }
    if (!ctx->X && !ctx->csr.ptr) { SET_ERR(ctx, "cnmf_set_matrix has not been called"); return CNMF_ESTATE; }
    int rc = validate_params(ctx, prm);
    if (rc) return rc;
    if (k > KMAX) { SET_ERR(ctx, "n_components=%d > CNMF_KMAX=%d", k, KMAX); return CNMF_EUNSUPPORTED; }
    if (int rcd_ = ensure_dense(ctx)) return rcd_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int N = (int)ctx->N, G = (int)ctx->G;
    hipStream_t st = ctx->stream;
    const int nblk = (N + 63) / 64, ldg = round_up(k, 4);
    DevPool pool;
    double* dHm = pool.get<double>((size_t)k * G);
    double* dP = pool.get<double>((size_t)k * N);
    double* dV = pool.get<double>((size_t)k * N);
    double* dgram = pool.get<double>((size_t)k * ldg);
    double* dOut = pool.get<double>((size_t)N * k);
    double* dpx = pool.get<double>(nblk);
    double* dpa = pool.get<double>(nblk);
    double* dpb = pool.get<double>(nblk);
    Mu2State* dstate = pool.get<Mu2State>(1, true, st);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dHm, H, (size_t)k * G * sizeof(double), hipMemcpyHostToDevice, st));
    std::vector<double> g, gp((size_t)k * ldg, 0.0);
    host_gram_f64(H, (size_t)G, k, true, 0.0, g);             // (the l2 term multiplies the row's own w_t: not a diagonal shift
    for (int a = 0; a < k; ++a)                               //  of the Gram matrix, which the error needs as it is)
        for (int b = 0; b < k; ++b) gp[(size_t)a * ldg + b] = g[(size_t)a * k + b];
    HIP_TRY(ctx, hipMemcpyAsync(dgram, gp.data(), gp.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const unsigned nb = (unsigned)((N + 3) / 4);
#define CNMF_XHT(KT_) xht_f64_kernel<KT_><<<nb, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, dHm, k, dP, N)
    if (k <= 8) CNMF_XHT(8); else if (k <= 16) CNMF_XHT(16); else if (k <= 32) CNMF_XHT(32); else if (k <= 64) CNMF_XHT(64);
    else CNMF_XHT(128);
#undef CNMF_XHT
    mu2_sumsq_kernel<<<nblk, 256, 0, st>>>(ctx->X, ctx->G_pad, N, G, dpx);
    {
        const long long n = (long long)k * N;
        mu2_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(dV, n, w_init);
    }
    HIP_TRY(ctx, hipGetLastError());
    const size_t lds = (size_t)2 * k * 64 * sizeof(double);
    HIP_TRY(ctx, dyn_lds_optin((const void*)mu2_burst_f64_kernel, (int)((size_t)2 * KMAX * 64 * sizeof(double))));
    const double l1 = prm->l1_reg_W, l2 = prm->l2_reg_W;
    auto burst = [&](int n_inner, int mode) {
        mu2_burst_f64_kernel<<<nblk, 64, lds, st>>>(dV, dP, N, N, k, dgram, ldg, l1, l2, n_inner, mode != 0, dpa, dpb, dstate);
        mu2_decide_kernel<<<1, 64, 0, st>>>(dpa, dpb, nblk, dpx, prm->tol, n_inner, mode, dstate);
    };
    burst(0, 2);
    Mu2State hs{};
    int it = 0;
    do {                                                      // up to four bursts between two looks at the state
        for (int b = 0; b < 4 && it < prm->max_iter; ++b) {
            const int n_inner = std::min(10 - it % 10, prm->max_iter - it);
            burst(n_inner, (prm->tol > 0 && (it + n_inner) % 10 == 0) ? 1 : 0);
            it += n_inner;
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&hs, dstate, sizeof hs, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    } while (it < prm->max_iter && !hs.done);
    cm_to_rows_f64_kernel<<<dim3((N + 255) / 256, k), 256, 0, st>>>(dV, N, N, k, dOut);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(W_out, dOut, (size_t)N * k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_iter_out) *n_iter_out = hs.iter;
    if (err_out) *err_out = hs.err;
    return CNMF_OK;
}
