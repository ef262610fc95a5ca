// Count structure of the data matrix (gfx950 only).
//
// cNMF factorises  X = counts[:, HVGs] / std_g  (cnmf.py:540-548): every column of X is an INTEGER
// matrix times one per-gene constant,  X[i][g] = n[i][g] * d[g].  Counts of high-variance genes are
// small: n <= 256 is exactly representable in ONE bf16 plane; the rare larger count (up to 65 535) is
// n = lo + 256 hi with a second, almost empty plane whose (256 rows x 16 k) blocks are flagged so that the
// GEMM touches it only where it is non-zero.  Folding d into the factor side,
//     pass A :  X . H^T   = n . (H * d)^T          (scale the columns of H before splitting it)
//     pass B :  X^T . W   = d * (n^T . W)          (scale the rows of the product afterwards)
// the f32-accurate product needs 3 bf16 MFMAs (the factor's three planes x one integer plane) instead of
// 6, every partial product is exact, and X costs 2 bytes per element instead of 6.
// The structure is DETECTED on the device from the resident float32 matrix (so it also applies to a
// matrix that arrives already normalised, as the reference hands it to scikit-learn); a matrix without
// it simply keeps the general three-plane path.  This header holds the detection; the planes themselves are built by
// x_planes_kernel (kernels_planes.hip.h).  Included by cnmf_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace cnmf {

constexpr int CNT_ROWS = 256;           // rows per partial of the column passes
constexpr int CNT_MAXMULT = 8;          // the smallest positive entry may be this many counts
constexpr float CNT_MAX = 65535.0f;     // lo + 256 hi, both planes exact in bf16 (lo <= 256, hi <= 255)

// part[chunk][g] = smallest positive entry of column g among the chunk's rows (+inf if none)
__global__ __launch_bounds__(256) void col_minpos_kernel(const float* __restrict__ X, int ld, int N, int G,
                                                         float* __restrict__ part)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int r0 = blockIdx.y * CNT_ROWS, r1 = min(N, r0 + CNT_ROWS);
    float m = __builtin_inff();
    for (int r = r0; r < r1; ++r) { const float x = X[(size_t)r * ld + g]; if (x > 0.f) m = fminf(m, x); }
    part[(size_t)blockIdx.y * G + g] = m;
}

__global__ __launch_bounds__(256) void col_min_combine_kernel(const float* __restrict__ part, int chunks, int G,
                                                              float* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    float m = __builtin_inff();
    for (int c = 0; c < chunks; ++c) m = fminf(m, part[(size_t)c * G + g]);
    out[g] = isinf(m) ? 0.f : m;
}

// fail[g] bit (m-1) set  <=>  for multiplier m some entry x of column g is not (an integer <= 256) * vmin/m
__global__ __launch_bounds__(256) void count_check_kernel(const float* __restrict__ X, int ld, int N, int G,
                                                          const float* __restrict__ vmin, unsigned* __restrict__ fail)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const float v = vmin[g];
    if (v <= 0.f) return;                                 // empty column: n = 0 everywhere
    const int r0 = blockIdx.y * CNT_ROWS, r1 = min(N, r0 + CNT_ROWS);
    unsigned bad = 0;
    for (int r = r0; r < r1; ++r) {
        const float x = X[(size_t)r * ld + g];
        if (x <= 0.f) { if (x < 0.f) bad = 0xFFu; continue; }
        const float q = x / v;                            // in units of the smallest entry
#pragma unroll
        for (int m = 1; m <= CNT_MAXMULT; ++m) {
            const float t = q * (float)m, n = rintf(t);
            // float32 input: t carries ~2^-22 relative error -> 1e-3 absolute below ~2000, relative above
            if (n < 1.f || n > CNT_MAX || fabsf(t - n) > fmaxf(1e-3f, 4e-7f * n)) bad |= 1u << (m - 1);
        }
    }
    if (bad) atomicOr(&fail[g], bad);
}

// partial sums for the scale: sx = sum x, sn = sum n  (float64), n = rint(x / unit[g])
__global__ __launch_bounds__(256) void count_sums_kernel(const float* __restrict__ X, int ld, int N, int G,
                                                         const float* __restrict__ unit, double* __restrict__ psx,
                                                         double* __restrict__ psn)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const float u = unit[g];
    const int r0 = blockIdx.y * CNT_ROWS, r1 = min(N, r0 + CNT_ROWS);
    double sx = 0.0, sn = 0.0;
    if (u > 0.f)
        for (int r = r0; r < r1; ++r) { const float x = X[(size_t)r * ld + g]; sx += (double)x; sn += (double)rintf(x / u); }
    psx[(size_t)blockIdx.y * G + g] = sx;
    psn[(size_t)blockIdx.y * G + g] = sn;
}

__global__ __launch_bounds__(256) void count_scale_kernel(const double* __restrict__ psx, const double* __restrict__ psn,
                                                          int chunks, int G, int G_pad, double* __restrict__ scale)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G_pad) return;
    double sx = 0.0, sn = 0.0;
    if (g < G) for (int c = 0; c < chunks; ++c) { sx += psx[(size_t)c * G + g]; sn += psn[(size_t)c * G + g]; }
    scale[g] = sn > 0.0 ? sx / sn : 0.0;
}

}  // namespace cnmf
