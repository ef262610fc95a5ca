// Operand planes of the matrix-pipe GEMMs, built outside the GEMM kernels (gfx950 only):
//   * the X side, once per matrix: ONE builder template (x_planes_kernel) for the four formats the count and general
//     paths multiply -- bf16 counts (kernels_gemm3.hip.h, gemm3c), f16 counts, counts as bytes and the f16 two-plane split
//     of X itself (kernels_gemm2h.hip.h) -- in both orientations, with the kernels that decide what it needs (a second count plane?
//     the per-row exponents of a general matrix);
//   * the factor side, once per half-step: the f16 two-plane split of a packed factor (split2h_tiled_*), whose body
//     the sweeps' finalize launch shares (kernels_sweep.hip.h).
// All planes are block-major, [row tile of TR rows][16-k block][row][16 halfwords]: one (tile, block) is one contiguous
// run, the LDS image the GEMM's DMA writes.  The layouts and their swizzles are explained where they are read.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_gemm3.hip.h"

namespace cnmf {

constexpr float G2_COUNT_BASE = 2048.0f;           // f16 counts: lo plane holds n <= 2048, hi plane 2048 * hi (hi <= 31)

__device__ __forceinline__ unsigned short f16_bits(float x)
{
    const _Float16 h = (_Float16)x;                // v_cvt_f16_f32, round to nearest even
    return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float f16_to_f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }

// exponent shift of a row whose largest entry is mx:  mx * 2^s in [2^14, 2^15)   (0 for an empty row)
__device__ __forceinline__ int g2_row_shift(float mx)
{
    if (!(mx > 0.f)) return 0;
    int e;
    frexpf(mx, &e);                                // mx = f * 2^e, f in [0.5, 1)  ->  mx in [2^(e-1), 2^e)
    const int s = 15 - e;
    return s > 120 ? 120 : (s < -110 ? -110 : s);
}

// y -> (h, m): h = f16(y), m = f16(y - h)
__device__ __forceinline__ void split2h(float y, unsigned short& h, unsigned short& m)
{
    h = f16_bits(y);
    m = f16_bits(y - f16_to_f32(h));
}

// ------------------------------------------------------------------------------------------ X side
// n = lo + BASE hi: lo in [0, BASE] (BASE itself stays in lo); the hi plane holds BASE * hi.  Both exact in the format
// whose BASE this is (bf16: 256, hi <= 255; f16: 2048, hi <= 31).
template <int BASE>
__device__ __forceinline__ void count_lo_hi(float n, float& lo, float& hi)
{
    if (n <= (float)BASE) { lo = n; hi = 0.f; }
    else { hi = floorf(n * (1.0f / (float)BASE)); lo = n - (float)BASE * hi; hi *= (float)BASE; }
}

// The formats of x_planes_kernel.  Each names
//   Aux        : the per-gene unit of a count matrix (one count = unit[g]) / the per-row exponent of a general one,
//   value()    : the number an element contributes (outside the matrix: 0),
//   pair()     : the two halfwords it becomes, one per plane,
//   SWIZZLE    : the two 16-byte slots of a row swapped for rows with bit 3 set (the f16 GEMM's conflict-free LDS image),
//   BYTES      : one byte per element in the step-major layout of CountU8 (one plane only),
//   FLAGGED    : a bit per (row tile, block) whose second plane is not all zero ((Kb + 31) / 32 words per tile row).
template <int BASE>
struct CountFormat {
    using Aux = float;
    static constexpr bool FLAGGED = true, BYTES = false;
    static __device__ __forceinline__ float value(const float* __restrict__ X, size_t at, bool inside,
                                                  const float* __restrict__ unit, int /*row*/, int gene)
    {
        if (!inside) return 0.f;
        const float u = unit[gene];
        return u > 0.f ? rintf(X[at] / u) : 0.f;
    }
};
struct CountBf16 : CountFormat<256> {               // gemm3c: integers <= 256 in one bf16 plane
    static constexpr bool SWIZZLE = false;
    static __device__ __forceinline__ void pair(float n, unsigned short& a, unsigned short& b)
    {
        float lo, hi;
        count_lo_hi<256>(n, lo, hi);
        a = bf16_rne(lo); b = bf16_rne(hi);
    }
};
struct CountF16 : CountFormat<(int)G2_COUNT_BASE> {  // gemm2h: integers <= 2048 in one f16 plane
    static constexpr bool SWIZZLE = true;
    static __device__ __forceinline__ void pair(float n, unsigned short& a, unsigned short& b)
    {
        float lo, hi;
        count_lo_hi<(int)G2_COUNT_BASE>(n, lo, hi);
        a = f16_bits(lo); b = f16_bits(hi);
    }
};
// gemm2h, 16x16x32 body: integers <= 255 as ONE BYTE each (exact; the GEMM converts them to f16 in registers).  No second
// plane, no flags.  One (row tile, 32-k step) is one contiguous 8 KB run, laid out for the wave that reads it (g2_u8_chunk).
struct CountU8 : CountFormat<255> {
    static constexpr bool SWIZZLE = false, FLAGGED = false, BYTES = true;
    static __device__ __forceinline__ void pair(float n, unsigned short& a, unsigned short& b) { a = (unsigned short)n; b = 0; }
};
// Byte offset, inside the 8 KB run of a 32-k step, of the eight counts  k = 8 g .. 8 g + 7  (g = 0..3) of tile row rin
// (0..255).  rin = wn * 64 + nt * 16 + r  (wn: the GEMM wave's 64 columns, nt = 2 p + t its 16-row count tile, r the row in
// it): the 16-byte chunk  (wn * 2 + p) * 64 + g * 16 + r  holds the eight bytes of tile t = 0 and then those of t = 1 -- what
// lane g * 16 + r of wave wn fetches with ONE ds_read_b128 per tile pair p (kernels_gemm2h.hip.h, the byte form of mf16).
__host__ __device__ constexpr int g2_u8_chunk(int rin, int g) { return (rin >> 5) * 1024 + (g * 16 + (rin & 15)) * 16 + ((rin >> 4) & 1) * 8; }

// General (NOT count-structured) X on the f16 pipe, gemm_mode 5: every row r of the operand (a cell for pass A, a gene for
// pass B) is held as TWO f16 planes of  y = x * 2^s_r  (h = f16(y), m = f16(y - h): within 1 ulp_f32 of x, exactly like
// the factor planes), s_r from the row maximum (x2h_rowshift_kernel); the GEMM multiplies the plane pairs with the `HI`
// instantiation, every block flagged, and its epilogue undoes 2^s_r per OUTPUT column.
struct SplitF16 {
    using Aux = int;
    static constexpr bool SWIZZLE = true, FLAGGED = false, BYTES = false;
    static __device__ __forceinline__ float value(const float* __restrict__ X, size_t at, bool inside,
                                                  const int* __restrict__ shift, int row, int /*gene*/)
    {
        return ldexpf(inside ? X[at] : 0.f, shift[row]);
    }
    static __device__ __forceinline__ void pair(float y, unsigned short& h, unsigned short& m) { split2h(y, h, m); }
};

// 16 halfwords = the 32 bytes of one row and block; swz: the two slots swapped
__device__ __forceinline__ void store_plane_row(unsigned short* d, const unsigned short* p, int swz)
{
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        u32x4 w;
        w.x = p[8 * hf + 0] | ((unsigned)p[8 * hf + 1] << 16); w.y = p[8 * hf + 2] | ((unsigned)p[8 * hf + 3] << 16);
        w.z = p[8 * hf + 4] | ((unsigned)p[8 * hf + 5] << 16); w.w = p[8 * hf + 6] | ((unsigned)p[8 * hf + 7] << 16);
        *reinterpret_cast<u32x4*>(d + (hf ^ swz) * 8) = w;
    }
}

// The planes of X (TRANSPOSE = false: rows = cells, k = genes, pass A's operand) or of X^T (rows = genes, k = cells,
// pass B's).  One thread per (row, 16-k block) in both mappings:
//   direct     : flat over (row, block) on grid.x -- a thread reads 16 consecutive floats of its row;
//   transposed : grid = (16-k blocks, row groups of 256), lanes along the output row -- a wave reads 64 consecutive
//                floats of each of its 16 cells.  The long dimension, the cells, rides on x.
// plane1 == nullptr: the second plane is neither stored nor flagged.
template <class F, bool TRANSPOSE>
__global__ __launch_bounds__(256) void x_planes_kernel(const float* __restrict__ X, int ld, int N, int G, int rows_pad,
                                                       int K, int TR, const typename F::Aux* __restrict__ aux,
                                                       unsigned short* __restrict__ plane0,
                                                       unsigned short* __restrict__ plane1,
                                                       unsigned int* __restrict__ flags)
{
    const int Kb = K / 16;
    int row, kb;
    if constexpr (TRANSPOSE) {
        row = blockIdx.y * 256 + threadIdx.x;
        kb = blockIdx.x;
        if (row >= rows_pad) return;
    } else {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= (long long)rows_pad * Kb) return;
        row = (int)(t / Kb);
        kb = (int)(t % Kb);
    }
    unsigned short p0[16], p1[16];
    bool any1 = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int k = kb * 16 + i;
        const int cell = TRANSPOSE ? k : row, gene = TRANSPOSE ? row : k;
        const float v = F::value(X, (size_t)cell * ld + gene, cell < N && gene < G, aux, row, gene);
        F::pair(v, p0[i], p1[i]);
        any1 |= p1[i] != 0;                                  // (a hi part is 0 or >= BASE: never a negative zero)
    }
    if constexpr (F::BYTES) {
        // byte plane (TR = 256, Kb even): [row tile][32-k step][8 KB]; this thread's 16-k block is the half kb & 1 of its
        // step, that is the two 8-k groups g = 2 (kb & 1) + hf
        const int rin = row % TR;
        unsigned char* d = reinterpret_cast<unsigned char*>(plane0) + ((size_t)(row / TR) * (Kb / 2) + (kb >> 1)) * ((size_t)TR * 32);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            uint2 w;
            w.x = p0[8 * hf + 0] | ((unsigned)p0[8 * hf + 1] << 8) | ((unsigned)p0[8 * hf + 2] << 16) | ((unsigned)p0[8 * hf + 3] << 24);
            w.y = p0[8 * hf + 4] | ((unsigned)p0[8 * hf + 5] << 8) | ((unsigned)p0[8 * hf + 6] << 16) | ((unsigned)p0[8 * hf + 7] << 24);
            *reinterpret_cast<uint2*>(d + g2_u8_chunk(rin, 2 * (kb & 1) + hf)) = w;
        }
        return;
    }
    const int rin = row % TR, swz = F::SWIZZLE ? (rin >> 3) & 1 : 0;
    const size_t at = (((size_t)(row / TR) * Kb + kb) * TR + rin) * 16;
    store_plane_row(plane0 + at, p0, swz);
    if (plane1) {
        store_plane_row(plane1 + at, p1, swz);
        if (F::FLAGGED && any1) atomicOr(&flags[(size_t)(row / TR) * ((Kb + 31) / 32) + (kb >> 5)], 1u << (kb & 31));
    }
}

// does any column of a count matrix need the second plane?  (max n > base)
__global__ __launch_bounds__(256) void count_max_base_kernel(const float* __restrict__ X, int ld, int N, int G,
                                                             const float* __restrict__ unit, float base,
                                                             unsigned* __restrict__ any_big)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const float u = unit[g];
    if (u <= 0.f) return;
    const int r0 = blockIdx.y * 256, r1 = min(N, r0 + 256);
    bool big = false;
    for (int r = r0; r < r1; ++r) big |= rintf(X[(size_t)r * ld + g] / u) > base;
    if (big) atomicOr(any_big, 1u);
}

// exponents of a general matrix (SplitF16) from the row maxima: rows of X (transpose = 0: one wave per row) or columns of
// X (transpose = 1: one thread per column)
__global__ __launch_bounds__(256) void x2h_rowshift_kernel(const float* __restrict__ X, int ld, int N, int G,
                                                           int transpose, int rows_pad, int* __restrict__ shift,
                                                           float* __restrict__ inv_scale)
{
    if (!transpose) {
        const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (row >= rows_pad) return;
        float mx = 0.f;
        if (row < N) for (int g = lane; g < G; g += 64) mx = fmaxf(mx, X[(size_t)row * ld + g]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if (lane == 0) { const int s = g2_row_shift(mx); shift[row] = s; inv_scale[row] = ldexpf(1.0f, -s); }
    } else {
        const int g = blockIdx.x * 256 + threadIdx.x;
        if (g >= rows_pad) return;
        float mx = 0.f;
        if (g < G) for (int r = 0; r < N; ++r) mx = fmaxf(mx, X[(size_t)r * ld + g]);
        const int s = g2_row_shift(mx);
        shift[g] = s; inv_scale[g] = ldexpf(1.0f, -s);
    }
}

// ------------------------------------------------------------------------------------------ factor side
// f16 planes of the packed factor, through LDS: 64 B per row and block = four 16-B slots  c = 2 q + hf  (q: 0 = h, 1 = m;
// hf = 8-k half), stored at slot  c ^ ((row >> 2) & 3).  A workgroup converts tiles of TROWS rows x TKB 16-k blocks
// (TROWS * TKB = 256: 16 rows x 256 k -- 1 KB contiguous per row read and per block written -- when K % 256 == 0,
// else 64 rows x 64 k) and walks the k tiles bx, bx + nbx, ... of its rows (the row scale is reduced once).
//   rmax_part [rows][parts] : per-row maxima of the values to convert (after kscale), one per sweep workgroup
//   inv_scale [rows]        : 2^-s_c, written by the workgroups of the first k column (bx == 0)
// `tile` = unsigned short [TKB][TROWS][32] (16 KB), `red` = float [256 / TROWS][TROWS] (1 KB, may alias the tile)
// Fused mode (the W half-step: shift_in != nullptr): the sweep has ALREADY written the planes of its rows, scaled
// by the exponent shift_in[row] chosen one iteration earlier.  This body then only (i) reduces the row maxima the sweep
// reported, (ii) checks that the exponent used was adequate -- largest scaled entry below the f16 overflow and not more
// than 5 bits under the target (the f16 planes keep an absolute accuracy 2^-39 of the scale: 5 bits of slack is what the
// sqrt(sum w^2) bound costs anyway) --, (iii) publishes 2^-s for pass B and the exponent of the NEXT iteration
// (shift_out: unchanged while the scaled maximum stays in [2^13, 2^15.5), else re-centred), and (iv) re-converts its 16
// rows from the float32 factor ONLY when one of them failed the check (a restart's first iterations).
struct SplitFused { const int* shift_in; int* shift_out; };
template <int TROWS, int TKB>
__device__ __forceinline__ void split2h_tiled_body(const float* __restrict__ src, int ld, int K, int TR,
                                                   unsigned short* __restrict__ dst, const double* __restrict__ kscale,
                                                   const float* __restrict__ rmax_part, int parts,
                                                   float* __restrict__ inv_scale, int bx, int nbx, int by,
                                                   unsigned short* tile_, float* red_, SplitFused fu = SplitFused{nullptr, nullptr})
{
    static_assert(TROWS * TKB == 256, "tile = 256 (row, block) pairs");
    constexpr int NQ = 256 / TROWS;                      // threads per row in the maximum reduction
    constexpr int KQ = TKB * 4;                          // float4 per row of a tile
    constexpr int RPP = 256 / KQ;                        // rows per pass of the conversion
    unsigned short (*tile)[TROWS][32] = reinterpret_cast<unsigned short (*)[TROWS][32]>(tile_);
    float (*red)[TROWS] = reinterpret_cast<float (*)[TROWS]>(red_);
    const int t = threadIdx.x;
    const int r0 = by * TROWS;
    const int kq = t % KQ, rr = t / KQ;                  // float4 index along k, row within a pass
    const int ntiles = K / (16 * TKB);
    // the data of the first k tile and the row maxima are requested together (one memory latency, not two)
    const bool fused = fu.shift_in != nullptr;
    float4 v[4];
    if (!fused) {
        const int k0 = bx * 16 * TKB;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = *reinterpret_cast<const float4*>(src + (size_t)(r0 + rr + RPP * i) * ld + k0 + kq * 4);
    }
    {
        const int row = t % TROWS, qt = t / TROWS;
        float mx = 0.f;
        // (one partial per 256-row tile: 196 of them at 50 000 cells -- eight requests in flight per pass)
        for (int p0 = qt; p0 < parts; p0 += 8 * NQ) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (p0 + j * NQ < parts) ? rmax_part[(size_t)(r0 + row) * parts + p0 + j * NQ] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, v[j]);
        }
        red[qt][row] = mx;
    }
    __syncthreads();
    int sh[4];
    bool redo = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = rr + RPP * i;
        float mx = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) mx = fmaxf(mx, red[q][row]);
        sh[i] = g2_row_shift(mx);
        if (fused) {
            const int su = fu.shift_in[r0 + row];
            const float ymax = ldexpf(mx, su);
            const bool ok = !(mx > 0.f) || (ymax < 60000.0f && ymax >= 1024.0f);
            const bool keep = !(mx > 0.f) || (ymax < 46340.0f && ymax >= 8192.0f);
            if (bx == 0 && kq == 0) fu.shift_out[r0 + row] = (ok && keep) ? su : sh[i];
            if (ok) sh[i] = su; else redo = true;
        }
        if (bx == 0 && kq == 0) inv_scale[r0 + row] = ldexpf(1.0f, -sh[i]);
    }
    if (fused) {
        // every thread looked at 4 of the TROWS rows: does ANY row of the workgroup need the conversion?
        if (!__syncthreads_or(redo ? 1 : 0)) return;
        const int k0 = bx * 16 * TKB;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = *reinterpret_cast<const float4*>(src + (size_t)(r0 + rr + RPP * i) * ld + k0 + kq * 4);
    }
    __syncthreads();                                     // `red` may alias the tile
    const int Kb = K / 16;
    const int tr = r0 / TR, rin = r0 % TR;
    for (int kt = bx; kt < ntiles; kt += nbx) {
        const int k0 = kt * 16 * TKB;
        // request the NEXT tile before converting this one
        float4 vn[4];
        const bool has_next = kt + nbx < ntiles;
        if (has_next) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                vn[i] = *reinterpret_cast<const float4*>(src + (size_t)(r0 + rr + RPP * i) * ld + (k0 + nbx * 16 * TKB) + kq * 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = rr + RPP * i;
            float x[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            if (kscale) {                                 // count-structured data: the per-gene scale rides on the factor
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = (float)((double)x[e] * kscale[k0 + kq * 4 + e]);
            }
            unsigned short p[2][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2h(ldexpf(x[e], sh[i]), p[0][e], p[1][e]);
            // 16-k block kq >> 2, 8-k half (kq >> 1) & 1, element offset (kq & 1) * 4 inside the slot;
            // (r0, TR multiples of 16: bits 2..3 of the in-tile row are bits 2..3 of the local row)
            const int hf = (kq >> 1) & 1, swz = (row >> 2) & 3;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                uint2 w;
                w.x = p[q][0] | ((unsigned)p[q][1] << 16); w.y = p[q][2] | ((unsigned)p[q][3] << 16);
                *reinterpret_cast<uint2*>(&tile[kq >> 2][row][((2 * q + hf) ^ swz) * 8 + (kq & 1) * 4]) = w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int c = pass * 256 + t;                 // 16-byte chunk of the tile: [block][row][4 chunks]
            const int b = c / (TROWS * 4), within = c % (TROWS * 4);
            unsigned short* g = dst + (((size_t)tr * Kb + (k0 / 16 + b)) * TR + rin) * 32;
            reinterpret_cast<u32x4*>(g)[within] = reinterpret_cast<const u32x4*>(&tile[b][0][0])[within];
        }
        __syncthreads();
        if (has_next) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = vn[i];
        }
    }
}

// grid = (column groups, rows / TROWS)
template <int TROWS, int TKB>
__global__ __launch_bounds__(256) void split2h_tiled_kernel(const float* __restrict__ src, int ld, int K, int TR,
                                                            unsigned short* __restrict__ dst,
                                                            const double* __restrict__ kscale,
                                                            const float* __restrict__ rmax_part, int parts,
                                                            float* __restrict__ inv_scale)
{
    // 16 KB in all: the maxima scratch lives in the tile (it is consumed before the first tile is written), so that a
    // split workgroup fits beside a GEMM workgroup (144 of the 160 KB) when two batches share the GPU
    __shared__ __attribute__((aligned(16))) unsigned short tile[256 * 32];
    float* red = reinterpret_cast<float*>(tile);
    split2h_tiled_body<TROWS, TKB>(src, ld, K, TR, dst, kscale, rmax_part, parts, inv_scale, blockIdx.x, gridDim.x,
                                   blockIdx.y, tile, red);
}

// per-row maxima of a packed factor in the partials layout the sweep writes ([rows][parts], part p = rows' columns
// [p * span, (p+1) * span)): used for rows the sweep has not produced (freshly installed or moved slots).
// grid = (parts, rows / 4): one wave per row and part.
__global__ __launch_bounds__(256) void rowmax_part_kernel(const float* __restrict__ V, int ld, int L, int span,
                                                          const double* __restrict__ kscale, int parts,
                                                          float* __restrict__ rmax_part)
{
    const int row = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = blockIdx.x;
    const int j0 = p * span, j1 = min(L, j0 + span);
    float mx = 0.f;
    for (int j = j0 + lane; j < j1; j += 64) {
        float x = V[(size_t)row * ld + j];
        if (kscale) x = (float)((double)x * kscale[j]);
        mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) rmax_part[(size_t)row * parts + p] = mx;
}

}  // namespace cnmf
