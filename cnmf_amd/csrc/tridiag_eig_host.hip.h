// The n_comp largest eigenpairs of a symmetric tridiagonal matrix T = tridiag(e, d, e) on the device (Preprocess's PCA
// with pca="device_full", Engine.symmetric_eigh_top(solver="device")): what pca_host.hip.h leaves to the host.  Stated
// first in float64 numpy in tests/_tridiag_eig_ref.py, which is the yardstick: the eigenvalues here are that file's to
// the bit, the vectors are held to the residual and orthogonality contracts.  Double precision throughout; no atomics,
// no grid barrier, no spin-wait; every sum has one fixed order.  Four launches:
//
//   teig_bounds_kernel   (one workgroup) |T|_1 = max_i ((|d_i| + |e_i|) + |e_{i-1}|), the power of two that brings it
//       into [1, 2) (ldexp: exact), the scaled d, e and e^2, pivmin = tiny max(1, max e^2) and the Gershgorin interval
//       widened by 2 n eps max(|gl|, |gu|) + 2 pivmin.  Max / min reductions only: the bits do not depend on an order.
//       A non-finite entry (or a norm that overflows) sets `bad`; a zero matrix is flagged and answered directly.
//   teig_bisect_kernel   one wavefront per eigenvalue, lane l owns the section point lo + (hi - lo) ((l + 1) / 65).
//       Every lane runs the Sturm recurrence q_i = (d_i - x) - e^2_{i-1} / q_{i-1} (|q| < pivmin -> -pivmin) with
//       explicitly rounded operations and the IEEE division; a ballot of count > n-1-j gives f, the number of leading
//       points at or below the target, and the bracket becomes [point f-1, point f].  The round loop runs in the kernel
//       (lo and hi are the same in every lane: the exit is wave-uniform), at most 40 rounds.  d and e^2 are read at a
//       wave-uniform address, eight rows ahead of the chain.
//   teig_invit_kernel    one lane per eigenvector; the factors of T - x_j I (dlagtf's elimination order: pivots, two
//       super-diagonals, multipliers, a swap flag per row; the swap by select on |c| > |a|) and the work vector are
//       [n][n_comp], so a row of all lanes is one coalesced access.  dstein's shift separation, a hashed start vector,
//       exactly three iterations (scale to |.|_inf = 1, forward sweep, back sweep with pivots below pert replaced),
//       then the 2-norm.  Every sweep is a dependent chain of length n; the loops are unrolled so that the next rows'
//       operands are in flight ahead of it.
//   teig_ortho_kernel    (one workgroup of 16 wavefronts) CGS2 over the columns in descending order -- the dot products
//       of a pass with lanes over the earlier columns and wavefronts over the rows, summed across wavefronts through
//       LDS in wavefront order; the update with a wavefront per row -- and then the check, in the operation order of
//       _tridiag_eig_ref.check: finite, max |T Z - Z diag(w)| <= 2 u_T, max |Z^T Z - I| <= 2 n eps (u_T = n eps |T|_1).
//       info [4] = {accepted (1 / 0; -1: non-finite input), residual / u_T, |rayleigh - w| / u_T, orthogonality / (n eps)}.
//       The work is O(n n_comp^2) on one compute unit: meant for n_comp << n.  It is the largest of the four steps
//       (10.9 of 16.5 ms at n = 2000, n_comp = 50: DESIGN.md section 1b) and the next one to rework.
//
// Included by cnmf_hip.hip (after pca_host.hip.h).
#pragma once

#include <cfloat>

// Rounding: the header's __dmul_rn / __dadd_rn are a plain `*` / `+` compiled with contraction allowed, so a product
// that feeds a sum through them may still become one fma.  The operations the restatement fixes go through the four
// helpers below instead, each compiled with contraction off inside its own body (a block-scoped pragma: nothing
// outside the helpers is compiled differently).  The compiler fuses a product into a sum only where both carry the
// permission, and these never do, wherever they are inlined.
namespace cnmf {

__device__ __forceinline__ double teig_mul(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double teig_add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double teig_sub(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double teig_div(double a, double b)
{
#pragma clang fp contract(off)
    return a / b;
}

constexpr int TEIG_ROUNDS = 40;
constexpr double TEIG_EPS = 0x1p-52, TEIG_TINY = 0x1p-1022, TEIG_ACCEPT = 2.0;

struct TeigParams {
    double norm;                // the scaled |T|_1 in [1, 2); 0: the zero matrix
    double pivmin, lo0, hi0;
    int shift;                  // scaled = ldexp(given, shift)
    int bad;                    // a non-finite entry
};

// the maximum of v over the workgroup (any number of whole wavefronts up to 16); every thread returns it.  red [16]
__device__ __forceinline__ double teig_block_max(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int nw = (int)blockDim.x >> 6;
    __syncthreads();                                                  // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = red[0];
    for (int w = 1; w < nw; ++w) m = fmax(m, red[w]);
    return m;
}

// the sum in one fixed order: the shuffle tree of a wavefront, then the wavefronts in order
__device__ __forceinline__ double teig_block_sum(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int nw = (int)blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < nw; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ bool teig_finite(double x) { return fabs(x) <= DBL_MAX; }

__global__ __launch_bounds__(256) void teig_bounds_kernel(int n, const double* __restrict__ d, const double* __restrict__ e,
                                                          double* __restrict__ ds, double* __restrict__ es,
                                                          double* __restrict__ e2, TeigParams* __restrict__ P)
{
    __shared__ double red[16];
    const int t = threadIdx.x;
    double nm = 0.0, bad = 0.0;
    for (int i = t; i < n; i += 256) {
        const double di = d[i], ei = i + 1 < n ? e[i] : 0.0, eb = i > 0 ? e[i - 1] : 0.0;
        if (!teig_finite(di) || !teig_finite(ei)) bad = 1.0;
        nm = fmax(nm, teig_add(teig_add(fabs(di), fabs(ei)), fabs(eb)));
    }
    bad = teig_block_max(bad, red);
    nm = teig_block_max(nm, red);
    if (bad != 0.0 || !teig_finite(nm) || nm == 0.0) {
        if (t == 0) {
            P->norm = 0.0; P->pivmin = 0.0; P->lo0 = 0.0; P->hi0 = 0.0; P->shift = 0;
            P->bad = (bad != 0.0 || !teig_finite(nm)) ? 1 : 0;
        }
        return;
    }
    int ex;
    frexp(nm, &ex);
    const int shift = 1 - ex;
    double gl = DBL_MAX, gu = -DBL_MAX, m2 = 0.0, sn = 0.0;
    for (int i = t; i < n; i += 256) {
        const double di = ldexp(d[i], shift), ei = i + 1 < n ? ldexp(e[i], shift) : 0.0,
                     eb = i > 0 ? ldexp(e[i - 1], shift) : 0.0;
        const double sq = teig_mul(ei, ei), r = teig_add(fabs(ei), fabs(eb));
        ds[i] = di;
        if (i + 1 < n) { es[i] = ei; e2[i] = sq; }
        gl = fmin(gl, teig_sub(di, r));
        gu = fmax(gu, teig_add(di, r));
        m2 = fmax(m2, sq);
        sn = fmax(sn, teig_add(teig_add(fabs(di), fabs(ei)), fabs(eb)));
    }
    gl = -teig_block_max(-gl, red);
    gu = teig_block_max(gu, red);
    m2 = teig_block_max(m2, red);
    sn = teig_block_max(sn, red);
    if (t == 0) {
        const double pivmin = teig_mul(TEIG_TINY, fmax(1.0, m2));
        const double wid = teig_add(teig_mul(2.0 * n * TEIG_EPS, fmax(fabs(gl), fabs(gu))), teig_mul(2.0, pivmin));
        P->norm = sn; P->pivmin = pivmin; P->lo0 = teig_sub(gl, wid); P->hi0 = teig_add(gu, wid);
        P->shift = shift; P->bad = 0;
    }
}

#define TEIG_STURM_STEP(dv, ev)                                                   \
    do {                                                                          \
        q = teig_sub(teig_sub((dv), x), teig_div((ev), q));                    \
        q = fabs(q) < pivmin ? -pivmin : q;                                       \
        cnt += q < 0.0 ? 1 : 0;                                                   \
    } while (0)

// ws [n_comp]: the eigenvalues of the scaled matrix; w [n_comp]: scaled back
__global__ __launch_bounds__(256) void teig_bisect_kernel(int n, int k, const double* __restrict__ ds,
                                                          const double* __restrict__ e2, const TeigParams* __restrict__ P,
                                                          double* __restrict__ ws, double* __restrict__ w)
{
    const int lane = threadIdx.x & 63, j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (j >= k || P->bad) return;                                     // (wave-uniform)
    if (P->norm == 0.0) {
        if (lane == 0) { ws[j] = 0.0; w[j] = 0.0; }
        return;
    }
    const double pivmin = P->pivmin, frac = teig_div((double)(lane + 1), 65.0);
    double lo = P->lo0, hi = P->hi0;
    const int target = n - 1 - j;
    for (int round = 0; round < TEIG_ROUNDS; ++round) {
        const double tol = fmax(teig_mul(2.0 * TEIG_EPS, fmax(fabs(lo), fabs(hi))), pivmin);
        if (!(teig_sub(hi, lo) > tol)) break;                        // (lo and hi are the same in every lane)
        const double x = teig_add(lo, teig_mul(teig_sub(hi, lo), frac));
        double q = teig_sub(ds[0], x);
        q = fabs(q) < pivmin ? -pivmin : q;
        int cnt = q < 0.0 ? 1 : 0;
        int i = 1;
        for (; i + 8 <= n; i += 8) {
            double dv[8], ev[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { dv[u] = ds[i + u]; ev[u] = e2[i + u - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) TEIG_STURM_STEP(dv[u], ev[u]);
        }
        for (; i < n; ++i) TEIG_STURM_STEP(ds[i], e2[i - 1]);
        const unsigned long long above = __ballot(cnt > target);
        const int f = above ? __ffsll((long long)above) - 1 : 64;
        const double plo = __shfl(x, f > 0 ? f - 1 : 0, 64), phi = __shfl(x, f < 64 ? f : 63, 64);
        if (f > 0) lo = plo;
        if (f < 64) hi = phi;
    }
    if (lane == 0) {
        const double v = teig_mul(0.5, teig_add(lo, hi));
        ws[j] = v;
        w[j] = ldexp(v, -P->shift);
    }
}
#undef TEIG_STURM_STEP

__device__ __forceinline__ double teig_start(unsigned row, unsigned col)
{
    unsigned h = row * 0x9E3779B1u + col * 0x85EBCA6Bu + 0x165667B1u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return ((double)h + 0.5) * 0x1p-31 - 1.0;                         // (exact: in (-1, 1))
}

struct TeigFactors {
    double *piv, *s1, *s2, *mul, *y;        // [n][n_comp]
    unsigned char* swp;                     // [n][n_comp]
};

// Z [n][n_comp]: column j = three steps of inverse iteration at the shift of eigenvalue j, at unit 2-norm
__global__ __launch_bounds__(64) void teig_invit_kernel(int n, int k, const double* __restrict__ ds,
                                                        const double* __restrict__ es, const double* __restrict__ ws,
                                                        const TeigParams* __restrict__ P, const TeigFactors F,
                                                        double* __restrict__ Z)
{
    const int j = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (j >= k || P->bad) return;
    const size_t K = (size_t)k;
    if (P->norm == 0.0) {
        for (int r = 0; r < n; ++r) Z[r * K + j] = r == j ? 1.0 : 0.0;
        return;
    }
    // dstein's separation, downwards: a shift closer than 10 eps |w_i| to the one before is moved that far below it
    double x = ws[0];
    for (int i = 1; i <= j; ++i) {
        const double wi = ws[i], tol = teig_mul(10.0 * TEIG_EPS, fabs(wi));
        x = teig_sub(x, wi) < tol ? teig_sub(x, tol) : wi;
    }
    const double pert = fmax(teig_mul(TEIG_EPS, P->norm), TEIG_TINY);
    double* __restrict__ piv = F.piv + j;
    double* __restrict__ s1 = F.s1 + j;
    double* __restrict__ s2 = F.s2 + j;
    double* __restrict__ mul = F.mul + j;
    double* __restrict__ y = F.y + j;
    unsigned char* __restrict__ swp = F.swp + j;
    // the factors of T - x I
    double a = teig_sub(ds[0], x), b = n > 1 ? es[0] : 0.0;
#pragma unroll 4
    for (int r = 0; r + 1 < n; ++r) {
        const double c = es[r], an = teig_sub(ds[r + 1], x), bn = r + 2 < n ? es[r + 1] : 0.0;
        const bool sw = fabs(c) > fabs(a);
        const double den = sw ? c : a;
        const double m = c == 0.0 ? 0.0 : teig_div(sw ? a : c, den);
        piv[r * K] = den; s1[r * K] = sw ? an : b; s2[r * K] = sw ? bn : 0.0; mul[r * K] = m; swp[r * K] = sw ? 1 : 0;
        a = teig_sub(sw ? b : an, teig_mul(m, sw ? an : b));
        b = sw ? -teig_mul(m, bn) : bn;
    }
    piv[(size_t)(n - 1) * K] = a; s1[(size_t)(n - 1) * K] = 0.0; s2[(size_t)(n - 1) * K] = 0.0;
    // the start vector
    double mx = 0.0;
    for (int r = 0; r < n; ++r) {
        const double v = teig_start((unsigned)r, (unsigned)j);
        y[r * K] = v;
        mx = fmax(mx, fabs(v));
    }
    for (int it = 0; it < 3; ++it) {
        // scale to |y|_inf = 1 and solve L (the row swaps applied as they come)
        double cur = teig_div(y[0], mx);
#pragma unroll 8
        for (int r = 0; r + 1 < n; ++r) {
            const double nxt = teig_div(y[(r + 1) * K], mx), m = mul[r * K];
            const bool sw = swp[r * K] != 0;
            const double t = teig_sub(sw ? cur : nxt, teig_mul(m, sw ? nxt : cur));
            y[r * K] = sw ? nxt : cur;
            cur = t;
        }
        y[(size_t)(n - 1) * K] = cur;
        // solve U, upwards
        double y1 = 0.0, y2 = 0.0;
        mx = 0.0;
#pragma unroll 8
        for (int r = n - 1; r >= 0; --r) {
            double p = piv[r * K];
            p = fabs(p) < pert ? copysign(pert, p) : p;
            const double v = teig_div(teig_sub(teig_sub(y[r * K], teig_mul(s1[r * K], y1)), teig_mul(s2[r * K], y2)), p);
            y[r * K] = v;
            mx = fmax(mx, fabs(v));
            y2 = y1; y1 = v;
        }
    }
    double ss = 0.0;
    for (int r = 0; r < n; ++r) {
        const double v = teig_div(y[r * K], mx);
        ss = teig_add(ss, teig_mul(v, v));
    }
    const double nrm = sqrt(ss);
    for (int r = 0; r < n; ++r) Z[r * K + j] = teig_div(teig_div(y[r * K], mx), nrm);
}

// dynamic LDS: coef [n_comp rounded up to 64], part [16][64], red [16]
__global__ __launch_bounds__(1024) void teig_ortho_kernel(int n, int k, const double* __restrict__ ds,
                                                          const double* __restrict__ es, const double* __restrict__ ws,
                                                          const TeigParams* __restrict__ P, double* Z, double* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double teig_lds[];
    const int kpad = (k + 63) & ~63;
    double* coef = teig_lds;
    double* part = coef + kpad;
    double* red = part + 16 * 64;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const size_t K = (size_t)k;
    if (P->bad) {
        if (t == 0) { info[0] = -1.0; info[1] = info[2] = info[3] = 0.0; }
        return;
    }
    if (P->norm == 0.0) {
        if (t == 0) { info[0] = 1.0; info[1] = info[2] = info[3] = 0.0; }
        return;
    }
    for (int j = 0; j < k; ++j) {
        for (int pass = 0; pass < 2 && j > 0; ++pass) {
            // coef [i] = z_i . z_j for every i < j (classical: all of them from the same z_j)
            for (int i0 = 0; i0 < j; i0 += 64) {
                const int i = i0 + lane;
                double acc = 0.0;
                if (i < j)
                    for (int r = wave; r < n; r += 16) acc += Z[r * K + i] * Z[r * K + j];
                part[wave * 64 + lane] = acc;
                __syncthreads();
                if (wave == 0 && i < j) {
                    double s = part[lane];
                    for (int w = 1; w < 16; ++w) s += part[w * 64 + lane];
                    coef[i] = s;
                }
                __syncthreads();
            }
            // z_j -= sum_i coef [i] z_i: a wavefront per row
            for (int r = wave; r < n; r += 16) {
                double s = 0.0;
                for (int i = lane; i < j; i += 64) s += coef[i] * Z[r * K + i];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
                if (lane == 0) Z[r * K + j] -= s;
            }
            __syncthreads();
        }
        double ss = 0.0;
        for (int r = t; r < n; r += 1024) { const double v = Z[r * K + j]; ss += v * v; }
        const double nrm = sqrt(teig_block_sum(ss, red));
        for (int r = t; r < n; r += 1024) Z[r * K + j] = Z[r * K + j] / nrm;
        __syncthreads();
    }
    // the check (tests/_tridiag_eig_ref.py: check), every product rounded, every sum over the rows in order
    double res = 0.0, bad = 0.0;
    for (int r = wave; r < n; r += 16) {                              // (maxima: any order)
        const double el = r > 0 ? es[r - 1] : 0.0, er = r + 1 < n ? es[r] : 0.0, dr = ds[r];
        for (int c = lane; c < k; c += 64) {
            const size_t idx = r * K + c;
            const double z = Z[idx], zm = r > 0 ? Z[idx - K] : 0.0, zp = r + 1 < n ? Z[idx + K] : 0.0;
            const double tz = teig_add(teig_add(teig_mul(el, zm), teig_mul(dr, z)), teig_mul(er, zp));
            res = fmax(res, fabs(teig_sub(tz, teig_mul(ws[c], z))));
            if (!teig_finite(z) || !teig_finite(ws[c])) bad = 1.0;
        }
    }
    double ray = 0.0;
    for (int c = t; c < k; c += 1024) {
        double rq = 0.0;
        for (int r = 0; r < n; ++r) {
            const size_t idx = r * K + c;
            const double z = Z[idx], zm = r > 0 ? Z[idx - K] : 0.0, zp = r + 1 < n ? Z[idx + K] : 0.0;
            const double el = r > 0 ? es[r - 1] : 0.0, er = r + 1 < n ? es[r] : 0.0;
            const double tz = teig_add(teig_add(teig_mul(el, zm), teig_mul(ds[r], z)), teig_mul(er, zp));
            rq = teig_add(rq, teig_mul(z, tz));
        }
        ray = fmax(ray, fabs(teig_sub(rq, ws[c])));
    }
    double orth = 0.0;
    const size_t pairs = K * K;
    for (size_t p = t; p < pairs; p += 1024) {
        const int jj = (int)(p / K), i = (int)(p - (size_t)jj * K);
        if (i > jj) continue;
        double g = 0.0;
#pragma unroll 8
        for (int r = 0; r < n; ++r) g =teig_add(g, teig_mul(Z[r * K + i], Z[r * K + jj]));
        orth = fmax(orth, fabs(teig_sub(g, i == jj ? 1.0 : 0.0)));
    }
    bad = teig_block_max(bad, red);
    res = teig_block_max(res, red);
    ray = teig_block_max(ray, red);
    orth = teig_block_max(orth, red);
    if (t == 0) {
        const double uT = teig_mul(n * TEIG_EPS, P->norm), ne = n * TEIG_EPS;
        const bool ok = bad == 0.0 && res <= TEIG_ACCEPT * uT && orth <= TEIG_ACCEPT * ne;
        info[0] = ok ? 1.0 : 0.0;
        info[1] = res / uT; info[2] = ray / uT; info[3] = orth / ne;
    }
}

constexpr int TEIG_ORTHO_LDS_MAX = (CNMF_PCA_NMAX + 16 * 64 + 16) * (int)sizeof(double);

}  // namespace cnmf

static int teig_comp_arg(cnmf_ctx* ctx, long long n, long long n_comp)
{
    if (n_comp < 1 || n_comp > n) { SET_ERR(ctx, "n_comp = %lld outside [1, %lld]", n_comp, n); return CNMF_EINVAL; }
    return CNMF_OK;
}

// the n_comp largest eigenpairs of tridiag(de, dd, de) (device arrays): dW [n_comp] descending, dZ [n][n_comp], both on the
// device; info [4] on the host (teig_ortho_kernel).  Synchronises.  Non-finite input: CNMF_EINVAL.  A result that the
// check does not accept is no error: info [0] = 0, and dZ is not to be used.  ctx->teig_ms [0..3]: the four launches.
static int teig_solve(cnmf_ctx* ctx, int n, int k, const double* dd, const double* de, double* dW, double* dZ, double* info)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    DevPool pool;
    EventPool evs;
    const size_t nk = (size_t)n * k;
    double* ds = pool.get<double>(n);
    double* es = pool.get<double>(n);
    double* e2 = pool.get<double>(n);
    double* ws = pool.get<double>(k);
    double* dinfo = pool.get<double>(4);
    TeigParams* P = pool.get<TeigParams>(1);
    TeigFactors F{};
    F.piv = pool.get<double>(nk); F.s1 = pool.get<double>(nk); F.s2 = pool.get<double>(nk);
    F.mul = pool.get<double>(nk); F.y = pool.get<double>(nk); F.swp = pool.get<unsigned char>(nk);
    POOL_TRY(ctx, pool);
    hipEvent_t ev[5];
    for (int s = 0; s < 5; ++s) ev[s] = evs.get();
    HIP_TRY(ctx, evs.err);
    const int kpad = (k + 63) & ~63;
    const size_t lds = ((size_t)kpad + 16 * 64 + 16) * sizeof(double);
    HIP_TRY(ctx, dyn_lds_optin((const void*)teig_ortho_kernel, TEIG_ORTHO_LDS_MAX));
    HIP_TRY(ctx, hipEventRecord(ev[0], st));
    teig_bounds_kernel<<<1, 256, 0, st>>>(n, dd, de, ds, es, e2, P);
    HIP_TRY(ctx, hipEventRecord(ev[1], st));
    teig_bisect_kernel<<<(k + 3) / 4, 256, 0, st>>>(n, k, ds, e2, P, ws, dW);
    HIP_TRY(ctx, hipEventRecord(ev[2], st));
    teig_invit_kernel<<<(k + 63) / 64, 64, 0, st>>>(n, k, ds, es, ws, P, F, dZ);
    HIP_TRY(ctx, hipEventRecord(ev[3], st));
    teig_ortho_kernel<<<1, 1024, lds, st>>>(n, k, ds, es, ws, P, dZ, dinfo);
    HIP_TRY(ctx, hipEventRecord(ev[4], st));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(info, dinfo, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int s = 0; s < 4; ++s) {
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
        ctx->teig_ms[s] = ms;
    }
    ctx->teig_ms[4] = 0.0;
    if (info[0] < 0.0) { SET_ERR(ctx, "the tridiagonal matrix holds non-finite values"); return CNMF_EINVAL; }
    return CNMF_OK;
}

extern "C" int cnmf_tridiagonal_eigh_top(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* d, const double* e, double* w,
                                         double* Z, double* info)
{
    if (!ctx || !d || (!e && n > 1) || !w || !Z || !info) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = tri_size_arg(ctx, n)) return rc;
    if (int rc = teig_comp_arg(ctx, n, n_comp)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevPool pool;
    const size_t cnt = (size_t)n * n_comp;
    double* dd = pool.get<double>(n);
    double* de = pool.get<double>(n);
    double* dW = pool.get<double>(n_comp);
    double* dZ = pool.get<double>(cnt);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dd, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    if (n > 1) HIP_TRY(ctx, hipMemcpyAsync(de, e, (size_t)(n - 1) * sizeof(double), hipMemcpyHostToDevice, st));
    if (int rc = teig_solve(ctx, (int)n, n_comp, dd, de, dW, dZ, info)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(w, dW, (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(Z, dZ, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_tridiagonal_fetch(cnmf_ctx* ctx, int64_t n, double* d, double* e)
{
    if (!ctx || !d || (!e && n > 1)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (!P.triR) { SET_ERR(ctx, "no tridiagonalisation is staged"); return CNMF_EINVAL; }
    if (n != P.tri_n) { SET_ERR(ctx, "n = %lld where the staged tridiagonalisation has %d", (long long)n, P.tri_n); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return tri_fetch(ctx, d, e);
}

extern "C" int cnmf_symmetric_eigh_top(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* A, double* w, double* V,
                                       double* info)
{
    if (!ctx || !A || !w || !V || !info) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = tri_size_arg(ctx, n)) return rc;
    if (int rc = teig_comp_arg(ctx, n, n_comp)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = tri_alloc(ctx, (int)n)) return rc;
    PreStage& P = ctx->pre;
    hipStream_t st = ctx->stream;
    P.tri_slot = -1;
    HIP_TRY(ctx, hipMemcpyAsync(P.triA, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, st));
    if (int rc = tri_reduce_launch(ctx)) return rc;
    DevPool pool;
    const size_t cnt = (size_t)n * n_comp;
    double* dW = pool.get<double>(n_comp);
    double* dZ = pool.get<double>(cnt);
    double* dV = pool.get<double>(cnt);
    POOL_TRY(ctx, pool);
    if (int rc = teig_solve(ctx, (int)n, n_comp, P.tri_d, P.tri_e, dW, dZ, info)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(w, dW, (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    if (info[0] != 1.0) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return CNMF_NOT_ACCEPTED;
    }
    if (int rc = tri_back_launch(ctx, n_comp, dZ, 1, dV)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(V, dV, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_pca_device(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, double* mean, double* w, double* V,
                                          double* scores, double* info)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!mean || !w || !V || !scores || !info) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    PreSlot& S = P.slot[slot];
    const int64_t n = S.n;
    if (int rc = tri_size_arg(ctx, n)) return rc;
    if (int rc = teig_comp_arg(ctx, n, n_comp)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = tri_alloc(ctx, (int)n)) return rc;
    P.tri_slot = slot;
    if (int rc = pre_scatter_device(ctx, slot, P.tri_mu, P.triA)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(mean, P.tri_mu, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = tri_reduce_launch(ctx)) return rc;
    const int N = (int)P.N, C = (int)n;
    DevPool pool;
    EventPool evs;
    double* dW = pool.get<double>(n_comp);
    double* dZ = pool.get<double>((size_t)C * n_comp);
    double* dV = pool.get<double>((size_t)C * n_comp);
    double* out = pool.get<double>((size_t)N * n_comp);
    POOL_TRY(ctx, pool);
    hipEvent_t e0 = evs.get(), e1 = evs.get();
    HIP_TRY(ctx, evs.err);
    if (int rc = teig_solve(ctx, C, n_comp, P.tri_d, P.tri_e, dW, dZ, info)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(w, dW, (size_t)n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    if (info[0] != 1.0) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return CNMF_NOT_ACCEPTED;
    }
    HIP_TRY(ctx, hipEventRecord(e0, st));
    if (int rc = tri_back_launch(ctx, n_comp, dZ, 1, dV)) return rc;
    PreGemm g{};
    g.M = N; g.Nn = n_comp; g.K = C; g.X = S.dense; g.ldx = C; g.mu = P.tri_mu; g.Bm = dV; g.ldb = n_comp;
    if (int rc = pre_product<2, 0>(ctx, g, out)) return rc;
    HIP_TRY(ctx, hipEventRecord(e1, st));
    HIP_TRY(ctx, hipMemcpyAsync(V, dV, (size_t)C * n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(scores, out, (size_t)N * n_comp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    ctx->teig_ms[4] = ms;
    return CNMF_OK;
}

extern "C" int cnmf_tridiagonal_eigh_step_ms(const cnmf_ctx* ctx, double* out)
{
    if (!ctx || !out) return CNMF_EINVAL;
    for (int s = 0; s < 5; ++s) out[s] = ctx->teig_ms[s];
    return CNMF_OK;
}
