// Count-structured data on the f16 matrix pipe: 2 MFMAs per f32-class product (gfx950 only).
//
// kernels_counts.hip.h explains the structure X[i][g] = n[i][g] * d[g] (n integer).  gemm3c_* (kernels_gemm3.hip.h)
// multiplies the integer plane (bf16: n <= 256 exact) with the factor's THREE bf16 planes: 3 MFMAs per product.
// Here both operands are f16 (same MFMA rate as bf16, 11 significand bits instead of 8):
//   * n <= 2048 is exact in ONE f16 plane (the second, flagged plane is needed only for counts > 2048: n = lo +
//     2048 hi, hi <= 31);
//   * the factor row  a[c][:]  is held as TWO f16 planes of  y = a * 2^s_c :  h = f16(y), m = f16(y - h).
//     y - h is exact in f32 and has at most 13 significant bits, so  h + m = y  exactly for 3 values in 4 and
//     |y - h - m| <= 1 ulp_f32(y) otherwise (when the 13th bit is set and the value is odd): the factor is
//     represented to ~23.5 bits, every partial product (11 x 11 bits) is exact, accumulation is f32.
//     s_c is a per-ROW exponent (max_j y = 2^14 .. 2^15, from the row maximum the sweep that produced the row
//     reports), so f16's narrow exponent range costs nothing: entries down to 2^-14 of the row maximum keep all 22
//     bits, smaller ones an ABSOLUTE error <= 2^-39 of the row maximum.  The product is scaled back by 2^-s_c
//     (exact) when the tile is stored.
//   => 2 MFMAs per product instead of 3, 24 KB instead of 32 KB of operands per 16-k block.
// A general (not count-structured) matrix rides the same kernels with X itself as two such planes (gemm_mode 5).
//
// Plane layouts, block-major like the bf16 ones ([row tile of 256][16-k block][row][...]), one (tile, block) = one
// contiguous run = the LDS image the DMA writes.  kernels_planes.hip.h builds them:
//   factor : 64 B per row and block = four 16-B slots  c = 2 q + hf  (q: 0 = h, 1 = m; hf = 8-k half), stored at
//            slot  c ^ ((row >> 2) & 3)  -- a ds_read_b128 lane group (16 rows, one slot each) then covers all 16
//            bank groups: conflict-free without padding;
//   X      : 32 B per row and block = two slots, stored at  hf ^ ((row >> 3) & 1)  (same argument).
// This header holds the image geometry, the two segment bodies and the two kernels.  The bodies are gemm3c's (256 x 256
// tile, 8 waves in two groups half a block apart, LDS-DMA images, counted vmcnt, raw barriers) with NSUB 16-k sub-blocks
// per barrier pair; the kernels call gemm2h_segment(G2Sub<NSUB>, ...), overloaded:
//   NSUB = 2 (one count plane, the production count path): "mf16", v_mfma_f32_16x16x32_f16, one MFMA per 32-k step --
//            half the barriers per flop, and the clock the chip holds under this load is higher with the smaller shape;
//   NSUB = 1 (second count plane, general matrices, CNMF_G2_NSUB=1): "m32", v_mfma_f32_32x32x16_f16, one MFMA per
//            16-k block.
// What the two bodies share is stated once (G2Geom, G2_DMA_PIECE, g2_wave_live).  Two things are NOT, because the shared
// form changed the instruction stream of a production kernel (tools/kernel_resources.py --isa against the parent build):
// abase / bbase / hbase are computed in each body in its own order, and the burst loop of m32 issues its pieces with the
// image and factor addresses formed once per step instead of through G2_DMA_PIECE.  For the same reason m32 is the
// G2Sub<1> overload itself and not a function behind a dispatcher (one more level of inlining reorders its prologue),
// and both bodies keep their early return on a null C (removing the test reschedules all 29 instantiations).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_gemm3.hip.h"
#include "kernels_planes.hip.h"

namespace cnmf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4_g __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_g __attribute__((ext_vector_type(2)));

// build-time A/B switch of the byte form (CNMF_HIPCC_FLAGS=-DG2_U8_SKIP=n): which of the spread stream's six piece places
// (0..2 in front of Y_s, 3..5 behind it) carries none of the five pieces.  Measured on the production pass-B launch and on
// the headline: 0 -- no piece behind the step's first eight MFMAs, where its first fragment batch is
// still landing -- is the fastest, 1 next, 2 and 4 slower than the f16 plane.
#ifndef G2_U8_SKIP
#define G2_U8_SKIP 0
#endif

constexpr int G2_ROWB = 64;                        // factor bytes per row and 16-k block
constexpr int G2_A = G3_MW * G2_ROWB;              // 16 384 B of factor planes per 16-k block
constexpr int G2_B = G3C_JW * 32;                  //  8 192 B of one X plane per 16-k block

// One step = NSUB 16-k blocks = one LDS image [A sub-blocks][B sub-blocks][hi sub-blocks], IMGS of them in flight.
// The workgroup moves an image in pieces of 8 KB (512 lanes x 16 B, one global_load_lds per wave and piece), numbered
// A 0 .. NA - 1, B NA .. NA + NB - 1, second plane NA + NB .. NA + 2 NB - 1.
// U8 (NSUB = 2 only): the count plane as bytes (CountU8, kernels_planes.hip.h) -- the 32 k of a step in ONE 8 KB piece, a
// 40 KB image.
template <int NSUB, bool HI, bool U8 = false>
struct G2Geom {
    static_assert(NSUB == 1 || (NSUB == 2 && !HI), "two blocks per step: one count plane only");
    static_assert(!U8 || NSUB == 2, "the byte plane is read by the 16x16x32 body only");
    static constexpr int IMGS = NSUB == 1 ? 4 : 3;
    static constexpr int IMG = U8 ? NSUB * G2_A + G2_B : NSUB * (G2_A + (HI ? 2 : 1) * G2_B);
    static constexpr int OFF_B = NSUB * G2_A, OFF_H = OFF_B + NSUB * G2_B;
    static constexpr int NA = NSUB * 2, NB = U8 ? 1 : NSUB;  // pieces per step (flagged steps of a second plane: NB more)
    static constexpr int AHEAD = IMGS - 1;               // steps requested ahead of the one being multiplied
    static constexpr int LDS_BYTES = IMGS * IMG;
};

// gemm2h_segment is overloaded on this tag: the kernels name the body of their NSUB by overload resolution (U8: the byte
// form of the NSUB = 2 body)
template <int NSUB, bool U8 = false> struct G2Sub {};

// Piece i_ of step s_ into its image: one global_load_lds per wave (no wait, no scheduling fence: the caller's).  Reads
// abase / bbase / hbase (this lane's 16 bytes of the first step's pieces), smem and wave of the body it is used in.
#define G2_DMA_PIECE(NSUB_, HI_, NTB_, s_, i_)                                                     \
    {                                                                                              \
        using GEO_ = G2Geom<NSUB_, HI_>;                                                           \
        unsigned char* d_ = smem + ((s_) % GEO_::IMGS) * GEO_::IMG + wave * 1024;                  \
        if ((i_) < GEO_::NA)                                                                       \
            __builtin_amdgcn_global_load_lds(G3_AS1(abase + (size_t)(s_) * ((NSUB_) * G2_A) + (i_) * 8192), \
                                             G3_AS3(d_ + (i_) * 8192), 16, 0, 0);                  \
        else if ((i_) < GEO_::NA + GEO_::NB)   /* the X planes are read once per pass: non-temporal */ \
            __builtin_amdgcn_global_load_lds(G3_AS1(bbase + (size_t)(s_) * ((NSUB_) * G2_B) + ((i_) - GEO_::NA) * 8192), \
                                             G3_AS3(d_ + GEO_::OFF_B + ((i_) - GEO_::NA) * 8192), 16, 0, (NTB_) ? 2 : 0); \
        else if constexpr (HI_)                                                                    \
            __builtin_amdgcn_global_load_lds(G3_AS1(hbase + (size_t)(s_) * ((NSUB_) * G2_B) + ((i_) - GEO_::NA - GEO_::NB) * 8192), \
                                             G3_AS3(d_ + GEO_::OFF_H + ((i_) - GEO_::NA - GEO_::NB) * 8192), 16, 0, (NTB_) ? 2 : 0); \
    }

// PART: the four bits of the live mask that belong to this wave group's 128 component rows, as a scalar
template <bool PART>
__device__ __forceinline__ unsigned g2_wave_live(unsigned live, int grp)
{
    return PART ? (unsigned)__builtin_amdgcn_readfirstlane((int)((live >> (grp * 4)) & 0xfu)) : 0xfu;
}

// ------------------------------------------------------------------------------------------
// One K segment [kb0, kb0 + nkb) (in 16-k blocks; kb0 and nkb multiples of NSUB) of one 256 x 256 tile.
//   A2 : f16 planes of the component-major factor (rows m0..), B1 : f16 X plane (rows j0..),
//   Bhi / hiflag : second X plane and its per-(tile, block) flags (HI),
//   rscale : 2^-s_c per component row, cscale : 2^-s_j per column of a general matrix (else nullptr); both applied to
//   the stored product.
// Timeline exactly as gemm3c_segment, in units of "steps" of NSUB blocks.
//
//   (NSUB, HI, GEN)      body   loop
//   (2, no,  no)         mf16   spread (VAR 4) / burst (VAR 0)          one count plane, production
//   (1, no,  no)         m32    spread (VAR 4) / burst (VAR 0)          one count plane, CNMF_G2_NSUB=1
//   (1, yes, no)         m32    burst, second plane where flagged       counts above 2048
//   (1, yes, yes)        m32    spread (VAR 4) / burst (VAR 0)          general matrices, three plane pairs
//
//   VAR   the instruction stream
//   0     burst: the pieces of step s + AHEAD in one run behind the X barrier, fragments read in one batch
//   4     spread (production): the pieces ride between the MFMA groups, fragments in two counted batches -- a burst of
//         DMA issues in front of 20 ds_read_b128 is the expensive place for them (MI355X_MICROARCH.md, "LDS-DMA piece
//         issue cost"); same MFMA order per accumulator as VAR 0, same bits
//   2     mf16 only, timing ablation: no MFMAs                              (results meaningless)
//   3     mf16 only, timing ablation: no steady-state DMA                   (results meaningless)
//   6     mf16 only, timing ablation: 3 and fragments read once             (results meaningless)
//   7     mf16 only, timing ablation: 6 and no barriers                     (results meaningless)
//   (1 and 5 were retired.)
// NTB: the X plane is loaded non-temporally (every tile is read by ONE workgroup per pass: 256 packed columns, or pass B
// with its XCD-aware order); with several component groups in pass A the workgroups p, p + P / MG stream the SAME tile at
// the same time and must find it in their L2: default cache policy (PMC, 1024 columns: profiles/r3_pmc_*).
// PART: only the 32-row component tiles named in `live` (bit t = rows 32 t .. 32 t + 31 of this 256-row group) are
// multiplied and stored -- the tail of a call, when restarts have finished and nothing is left to refill their columns:
// a wave skips the MFMAs of its dead tiles (wave-uniform scalar branches), so a pass costs what its live columns cost,
// down to the floor of streaming the X plane.  The operand traffic is unchanged.
// GEN (general matrices = X itself as two f16 planes, HI instantiation): the product of the two SMALL planes, x_m . f_m,
// is not formed -- |x_m| <= 2^-11 |x_h| and |f_m| <= 2^-11 |f_h|, so the term is <= 2^-22 of the product, random in sign,
// against the 2^-24 rounding of every float32 accumulation step: 3 MFMAs per product instead of 4.  The count path (HI
// there = a second EXACT integer plane) keeps all four.

// ---- NSUB = 2 ("mf16") with ONE count plane (the production count path, counts <= 2048) on v_mfma_f32_16x16x32_f16.
// One 32-k step holds the 16-k blocks u = 0, 1 in one image and one MFMA consumes
// both: lane (r = lane & 15, g = lane >> 4) holds the eight k  8 g .. 8 g + 7  of the step, that is block u = g >> 1,
// 8-k half hf = g & 1, of factor row  mt * 16 + r  (mt = 0..7: the wave's 128 rows) and of count row  nt * 16 + r
// (nt = 0..3: its 64 columns).  The plane swizzles stay conflict-free: the sixteen rows of a lane group with one logical
// slot c hit the 16-byte bank groups (row % 4) * 4 + (c ^ ((row >> 2) & 3)) of the factor image and
// (row % 8) * 2 + (hf ^ ((row >> 3) & 1)) of the count image -- sixteen distinct ones each.
// Per step and wave: 16 + 4 ds_read_b128 (80 fragment registers), 64 MFMAs on acc[8][4] (128 registers); per accumulator
// the small plane m first, then h.  Element i of acc[mt][nt] is component row mt * 16 + 4 g + i, column nt * 16 + r.
// Six pieces per step; spread: fragment reads 12 + 8.
//
// U8, the count plane as bytes (counts <= 255; CountU8 / g2_u8_chunk, kernels_planes.hip.h): the same operands from half the
// count bytes.  One step of one tile is one 8 KB piece (FIVE pieces per step, a 40 KB image), in which the 16-byte chunk
// (wn * 2 + p) * 64 + lane  holds what lane (r, g) of wave wn needs of the count tiles nt = 2 p and 2 p + 1: the bytes
// k = 8 g .. 8 g + 7 of row nt * 16 + r, tile 2 p in the low eight bytes.  The wave fetches them with TWO ds_read_b128
// (p = 0, 1) instead of four.  No swizzle is needed: a read is 64 consecutive chunks in lane order, so the sixteen lanes
// of every ds_read_b128 lane group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) read chunks whose indices
// are all different modulo 16 -- sixteen distinct 16-byte bank groups = all 64 banks once: conflict-free.
// Conversion in registers, exact: v_perm_b32 puts two bytes n under the high byte 0x64 -- the halves 0x6400 | n are
// f16(1024 + n), whose ulp is 1 --, v_pk_add_f16 takes the 1024 off again (n = 0 gives +0, like the f16 plane): 4 + 4
// instructions per fragment, bq[nt] bit for bit what the f16 plane holds, in the same element order.
// Spread stream: two pieces in front of Y_s (behind the second fragment batch and behind the next eight MFMAs), three behind
// it (G2_U8_SKIP); fragment reads 10 + 8.
template <int VAR, bool NTB, bool PART, bool U8 = false>
__device__ __forceinline__ void gemm2h_segment_mf16(const unsigned char* __restrict__ A2, const unsigned char* __restrict__ B1,
                                                    const float* __restrict__ rscale, int Kb, float* __restrict__ C,
                                                    int ldc, int m0, int j0, int kb0, int nkb, unsigned char* smem,
                                                    unsigned live)
{
    static_assert(VAR == 0 || VAR == 2 || VAR == 3 || VAR == 4 || VAR == 6 || VAR == 7, "instruction streams 1 and 5 were retired");
    static_assert(!U8 || VAR == 0 || VAR == 4, "the byte plane has the burst and the spread stream only");
    using GEO = G2Geom<2, false, U8>;
    constexpr int NSUB = 2, IMGS = GEO::IMGS, IMG = GEO::IMG, OFF_B = GEO::OFF_B, NA = GEO::NA, NB = GEO::NB, AHEAD = GEO::AHEAD;
    constexpr bool BURST = VAR == 0, NOMFMA = VAR == 2, NODMA = VAR == 3 || VAR == 6 || VAR == 7;
    constexpr bool NOREAD = VAR == 6 || VAR == 7, NOBAR = VAR == 7;
    static_assert(IMGS == 3 && NA + NB == (U8 ? 5 : 6), "three images, six pieces per step (bytes: five)");
    const int tid = threadIdx.x;                         // 0..511
    const int lane = tid & 63, wave = tid >> 6;
    const int grp = wave >> 2, wn = wave & 3;
    const int r = lane & 15, g = lane >> 4;
    const int ub = g >> 1, hf = g & 1;
    const int nst = nkb / NSUB;                          // steps in this segment
    // bit m of the live mask = the wave's rows 32 m .. 32 m + 31 = its 16-row tiles 2 m and 2 m + 1
    const unsigned lv = g2_wave_live<PART>(live, grp);
#define G2_LIVE(mt_) (!PART || ((lv >> ((mt_) >> 1)) & 1u))

    const unsigned char* abase = A2 + ((size_t)(m0 / G3_MW) * Kb + kb0) * G2_A + tid * 16;
    // (bytes: one G2_B run per STEP of the tile, not per block)
    const unsigned char* bbase = U8 ? B1 + ((size_t)(j0 / G3C_JW) * (Kb / NSUB) + kb0 / NSUB) * G2_B + tid * 16
                                    : B1 + ((size_t)(j0 / G3C_JW) * Kb + kb0) * G2_B + tid * 16;
    constexpr const unsigned char* hbase = nullptr;      // (G2_DMA_PIECE names it; no second plane here)

    f32x4_g acc[8][4];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[mt][nt][i] = 0.f;

    // fragment addresses inside an image (tile mt / nt: + mt * 16 rows of 64 B / + nt * 16 rows of 32 B)
    const int a_row = ub * G2_A + (grp * 128 + r) * G2_ROWB;
    const int a_s0 = ((0 + hf) ^ ((r >> 2) & 3)) * 16, a_s1 = ((2 + hf) ^ ((r >> 2) & 3)) * 16;
    const int b_off = U8 ? OFF_B + wn * 2048 + lane * 16 : OFF_B + ub * G2_B + (wn * 64 + r) * 32 + (hf ^ ((r >> 3) & 1)) * 16;

// bytes: pieces 0..3 the factor planes as ever, piece 4 the whole count run of the step
#define G2_DMA_PIECE_U8(s_, i_)                                                                    \
    {                                                                                              \
        unsigned char* d_ = smem + ((s_) % IMGS) * IMG + wave * 1024;                              \
        if ((i_) < NA)                                                                             \
            __builtin_amdgcn_global_load_lds(G3_AS1(abase + (size_t)(s_) * (NSUB * G2_A) + (i_) * 8192), \
                                             G3_AS3(d_ + (i_) * 8192), 16, 0, 0);                  \
        else                                                                                       \
            __builtin_amdgcn_global_load_lds(G3_AS1(bbase + (size_t)(s_) * G2_B), G3_AS3(d_ + OFF_B), 16, 0, NTB ? 2 : 0); \
    }
#define G2_PIECE(s_, i_) { if constexpr (U8) G2_DMA_PIECE_U8(s_, i_) else G2_DMA_PIECE(2, false, NTB, s_, i_) __builtin_amdgcn_sched_barrier(0); }
// the spread stream's six places: piece p_ of the f16 plane's six; of the bytes' five, none at place G2_U8_SKIP
#define G2_SPOT(MORE_, p_)                                                                         \
    if (!BURST && MORE_) {                                                                         \
        if constexpr (!U8) G2_PIECE(s + AHEAD, p_)                                                 \
        else if constexpr ((p_) != G2_U8_SKIP) G2_PIECE(s + AHEAD, (p_) < G2_U8_SKIP ? (p_) : (p_) - 1) \
    }
// two bytes of w_ (selected by sel_) under 0x64: two halves 1024 + n; minus 1024
#define G2_CVT2(w_, sel_) __builtin_bit_cast(unsigned, __builtin_bit_cast(f16x2_g, __builtin_amdgcn_perm(0x64646464u, (w_), (sel_))) - f16x2_g{(_Float16)1024.0f, (_Float16)1024.0f})
#define G2_SEL_LO 0x04010400u                              /* bytes 0, 1 of w_ */
#define G2_SEL_HI 0x04030402u                              /* bytes 2, 3 */
#define G2_CVT(nt_)                                                                                \
    {                                                                                              \
        const unsigned w0_ = braw[(nt_) >> 1][2 * ((nt_) & 1)], w1_ = braw[(nt_) >> 1][2 * ((nt_) & 1) + 1]; \
        u32x4 c_;                                                                                  \
        c_.x = G2_CVT2(w0_, G2_SEL_LO); c_.y = G2_CVT2(w0_, G2_SEL_HI);                            \
        c_.z = G2_CVT2(w1_, G2_SEL_LO); c_.w = G2_CVT2(w1_, G2_SEL_HI);                            \
        bq[nt_] = __builtin_bit_cast(f16x8, c_);                                                   \
    }
#define G2_ISSUE(s_) { _Pragma("unroll") for (int i = 0; i < NA + NB; ++i) G2_PIECE(s_, i) }
#define G2_FRAG(ptr_) __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(ptr_))
#define G2_AFRAG(bb_, mt_, q_) G2_FRAG((bb_) + a_row + (mt_) * 16 * G2_ROWB + ((q_) ? a_s1 : a_s0))
// fragment reads in two batches: the 12 the first half of the step needs, then -- behind its first 16 MFMAs -- the 8 of the
// second half: at most 12 LDS reads are outstanding, so the waits in front of the MFMAs can be counted (lgkmcnt is a
// 4-bit counter: behind 20 reads the compiler can only wait for all of them)
#define G2_READ_A(s_)                                                                              \
    {                                                                                              \
        const unsigned char* bb = smem + ((s_) % IMGS) * IMG;                                      \
        if constexpr (U8) { _Pragma("unroll") for (int p = 0; p < 2; ++p) braw[p] = *reinterpret_cast<const u32x4*>(bb + b_off + p * 1024); } \
        else { _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) bq[nt] = G2_FRAG(bb + b_off + nt * 16 * 32); } \
        _Pragma("unroll") for (int mp = 0; mp < 4; mp += 2) {                                      \
            aq[mp][1] = G2_AFRAG(bb, mp, 1); aq[mp + 1][1] = G2_AFRAG(bb, mp + 1, 1);              \
            aq[mp][0] = G2_AFRAG(bb, mp, 0); aq[mp + 1][0] = G2_AFRAG(bb, mp + 1, 0);              \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        /* (no fence behind the conversion: the compiler lays its 32 instructions among the first MFMAs) */ \
        if constexpr (U8) { _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) G2_CVT(nt) }          \
    }
#define G2_READ_B(s_)                                                                              \
    {                                                                                              \
        const unsigned char* bb = smem + ((s_) % IMGS) * IMG;                                      \
        _Pragma("unroll") for (int mp = 4; mp < 8; mp += 2) {                                      \
            aq[mp][1] = G2_AFRAG(bb, mp, 1); aq[mp + 1][1] = G2_AFRAG(bb, mp + 1, 1);              \
            aq[mp][0] = G2_AFRAG(bb, mp, 0); aq[mp + 1][0] = G2_AFRAG(bb, mp + 1, 0);              \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    }
// one factor tile and plane against the wave's four count tiles
#define G2_MF(mt_, q_)                                                                             \
    if constexpr (NOMFMA) { asm volatile("" :: "v"(aq[mt_][q_]), "v"(bq[0]), "v"(bq[1]), "v"(bq[2]), "v"(bq[3])); } \
    else if (G2_LIVE(mt_)) {                                                                       \
        _Pragma("unroll") for (int nt = 0; nt < 4; ++nt)                                           \
            acc[mt_][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq[mt_][q_], bq[nt], acc[mt_][nt], 0, 0, 0); \
    }
// eight MFMAs on eight accumulators; G2_MF8(.., 1) then G2_MF8(.., 0): small plane first
#define G2_MF8(ma_, mb_, q_) G2_MF(ma_, q_) G2_MF(mb_, q_)
#define G2_STEP(MORE_)                                                                             \
    {                                                                                              \
        if constexpr (!NOBAR) G3_RAW_BARRIER()                  /* X_s: image (s + 2) % 3 = (s - 1) % 3 is free */ \
        if (BURST && MORE_) G2_ISSUE(s + AHEAD)                                                    \
        if constexpr (NOREAD) { if (s == 0) { G2_READ_A(s) G2_READ_B(s) } } else { G2_READ_A(s) }  \
        G2_MF8(0, 1, 1)                                                                            \
        G2_SPOT(MORE_, 0)                                                                          \
        G2_MF8(0, 1, 0)                                                                            \
        if constexpr (!NOREAD) { G2_READ_B(s) }                                                    \
        G2_SPOT(MORE_, 1)                                                                          \
        G2_MF8(2, 3, 1)                                                                            \
        G2_SPOT(MORE_, 2)                                                                          \
        G2_MF8(2, 3, 0)                                                                            \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      /* this image is free once both groups pass here */ \
        /* step s+1 must have landed before Y_s; what was issued for step s+2 since X_s (three pieces, or the burst's six; \
           bytes: two, or the burst's five) may stay in flight */                                  \
        if (s + 1 < nst) {                                                                         \
            if (MORE_) {                                                                           \
                if constexpr (U8) { if constexpr (BURST) G3_WAIT_VM(5); else if constexpr (G2_U8_SKIP < 3) G3_WAIT_VM(2); else G3_WAIT_VM(3); } \
                else { if constexpr (BURST) G3_WAIT_VM(6); else G3_WAIT_VM(3); }                   \
            } else G3_WAIT_VM(0);                                                                  \
        }                                                                                          \
        if constexpr (!NOBAR) G3_RAW_BARRIER()                  /* Y_s */                          \
        G2_MF8(4, 5, 1)                                                                            \
        G2_SPOT(MORE_, 3)                                                                          \
        G2_MF8(4, 5, 0)                                                                            \
        G2_SPOT(MORE_, 4)                                                                          \
        G2_MF8(6, 7, 1)                                                                            \
        G2_SPOT(MORE_, 5)                                                                          \
        G2_MF8(6, 7, 0)                                                                            \
    }

    f16x8 bq[4], aq[8][2];
    u32x4 braw[2];                                          // (bytes only: the step's raw counts, two tiles per register quad)
    G3_WAIT_VM(0);                                          // stores of a previous segment
    G2_ISSUE(0)
    if (nst > 1) G2_ISSUE(1)
    // step 0 landed (step 1, six pieces or five, may stay in flight)
    if (nst > 1) { if constexpr (U8) G3_WAIT_VM(5); else G3_WAIT_VM(6); } else G3_WAIT_VM(0);
    if (grp == 1) G3_RAW_BARRIER()
    {
        int s = 0;
        const int n_main = NODMA ? 0 : nst - AHEAD;             // steps that still have a step to request
        for (; s < n_main; ++s) G2_STEP(true)
        for (; s < nst; ++s) G2_STEP(false)
    }
    if (grp == 0) G3_RAW_BARRIER()
#undef G2_STEP
#undef G2_MF8
#undef G2_MF
#undef G2_READ_B
#undef G2_READ_A
#undef G2_AFRAG
#undef G2_FRAG
#undef G2_ISSUE
#undef G2_CVT
#undef G2_SEL_HI
#undef G2_SEL_LO
#undef G2_CVT2
#undef G2_SPOT
#undef G2_PIECE
#undef G2_DMA_PIECE_U8

    if (C == nullptr) return;                                // (kept for the instruction stream: see the head comment)
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        if (!G2_LIVE(mt)) continue;                      // nobody reads the products of dead columns
        const int row0 = m0 + grp * 128 + mt * 16 + 4 * g;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float rs = rscale[row0 + i];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                C[(size_t)(row0 + i) * ldc + j0 + wn * 64 + nt * 16 + r] = acc[mt][nt][i] * rs;
        }
    }
#undef G2_LIVE
}

// ---- NSUB = 1 ("m32") on v_mfma_f32_32x32x16_f16: one 16-k block per step, four images, pieces A0 A1 B (Bhi).
// Lane (li = lane & 31, h = lane >> 5) holds the 8-k half h of factor row  m * 32 + li  (m = 0..3: the wave's 128 rows)
// and of X row  n * 32 + li  (n = 0..1: its 64 columns); acc[m][n] is one 32 x 32 tile.  Per accumulator the small factor
// plane m first, then h; the second X plane after the first.
// Spread loop: one count plane (!HI) and general matrices (HI && GEN, every block flagged) at VAR 4 -- the pieces of step
// s + 3 ride between the MFMA groups, fragment reads 8 + 4.  Burst loop: everything at VAR 0, and always the flagged
// second count plane (HI && !GEN), whose fourth piece and MFMAs exist only where a block's flag is set.
template <bool HI, int VAR, bool NTB, bool PART, bool GEN>
__device__ __forceinline__ void gemm2h_segment(G2Sub<1>, const unsigned char* __restrict__ A2, const unsigned char* __restrict__ B1,
                                                   const unsigned char* __restrict__ Bhi,
                                                   const unsigned int* __restrict__ hiflag,
                                                   const float* __restrict__ rscale,
                                                   int Kb, float* __restrict__ C, int ldc, int m0, int j0, int kb0,
                                                   int nkb, unsigned char* smem, const float* __restrict__ cscale,
                                                   unsigned live)
{
    static_assert(VAR == 0 || VAR == 4, "the 32x32x16 body has the burst and the spread stream only");
    using GEO = G2Geom<1, HI>;
    constexpr int IMGS = GEO::IMGS, IMG = GEO::IMG, OFF_B = GEO::OFF_B, AHEAD = GEO::AHEAD;
    static_assert(IMGS == 4 && GEO::NA == 2 && GEO::NB == 1, "four images, pieces A0 A1 B (Bhi)");
    const int tid = threadIdx.x;                         // 0..511
    const int lane = tid & 63, wave = tid >> 6;
    const int grp = wave >> 2, wn = wave & 3;
    const int li = lane & 31, h = lane >> 5;
    const int nst = nkb;                                 // steps in this segment
    // the wave's four component tiles (rows grp * 128 + m * 32 ...): which of them hold live columns?
    const unsigned lv = g2_wave_live<PART>(live, grp);
#define G2_LIVE(m_) (!PART || ((lv >> (m_)) & 1u))

    const size_t jblk = ((size_t)(j0 / G3C_JW) * Kb + kb0);
    const unsigned char* abase = A2 + ((size_t)(m0 / G3_MW) * Kb + kb0) * G2_A + tid * 16;
    const unsigned char* bbase = B1 + jblk * G2_B + tid * 16;
    const unsigned char* hbase = HI ? Bhi + jblk * G2_B + tid * 16 : nullptr;
    // flag bits of blocks kb0 .. kb0 + nkb - 1 (at most 5 words for up to 129 blocks; longer segments: all set)
    unsigned int fw[5] = {0u, 0u, 0u, 0u, 0u};
    if (HI) {
        const int KW = (Kb + 31) >> 5, w0 = kb0 >> 5;
        const unsigned int* fr = hiflag + (size_t)(j0 / G3C_JW) * KW;
#pragma unroll
        for (int w = 0; w < 5; ++w)
            fw[w] = (nkb > 129) ? 0xFFFFFFFFu : ((w0 + w < KW) ? __builtin_amdgcn_readfirstlane(fr[w0 + w]) : 0u);
    }
    const int fbit0 = kb0 & 31;

    f32x16_3 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    // fragment addresses inside an image: factor row (grp*128 + m*32 + li), slot (2q + h) ^ ((li >> 2) & 3);
    // X row (wn*64 + n*32 + li), slot h ^ ((li >> 3) & 1)
    const int a_row = (grp * 128 + li) * G2_ROWB;
    const int a_s0 = ((0 + h) ^ ((li >> 2) & 3)) * 16, a_s1 = ((2 + h) ^ ((li >> 2) & 3)) * 16;
    const int b_off = OFF_B + (wn * 64 + li) * 32 + (h ^ ((li >> 3) & 1)) * 16;

#define G2_BLKFLAG(b_) (HI && ((fw[(fbit0 + (b_)) >> 5 > 4 ? 4 : (fbit0 + (b_)) >> 5] >> ((fbit0 + (b_)) & 31)) & 1u))
#define G2_ISSUE(s_)                                                                               \
    {                                                                                              \
        unsigned char* d_ = smem + ((s_) % IMGS) * IMG + wave * 1024;                              \
        const unsigned char* a_ = abase + (size_t)(s_) * G2_A;                                     \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                              \
            __builtin_amdgcn_global_load_lds(G3_AS1(a_ + i * 8192), G3_AS3(d_ + i * 8192), 16, 0, 0); \
        __builtin_amdgcn_global_load_lds(G3_AS1(bbase + (size_t)(s_) * G2_B), G3_AS3(d_ + OFF_B), 16, 0, NTB ? 2 : 0); \
        if (HI) {                                                                                  \
            if (G2_BLKFLAG(s_))                                                                    \
                __builtin_amdgcn_global_load_lds(G3_AS1(hbase + (size_t)(s_) * G2_B), G3_AS3(d_ + GEO::OFF_H), 16, 0, NTB ? 2 : 0); \
        }                                                                                          \
    }
#define G2_PIECE(s_, i_) { G2_DMA_PIECE(1, HI, NTB, s_, i_) __builtin_amdgcn_sched_barrier(0); }
#define G2_FRAG(ptr_) __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(ptr_))
// two component tiles at a time, small plane first: consecutive MFMAs cycle through four accumulators
#define G2_MFMA(b_, m_, q_)                                                                        \
    if (G2_LIVE(m_)) {                                                                             \
    acc[m_][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[m_][q_], b_[0], acc[m_][0], 0, 0, 0);   \
    acc[m_][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[m_][q_], b_[1], acc[m_][1], 0, 0, 0); }
// "the step after this one has landed; cnt_ steps of three pieces behind it may stay in flight"
#define G2_WAIT_AHEAD(cnt_)                                                                        \
    {                                                                                              \
        if constexpr ((cnt_) == 1) G3_WAIT_VM(3);                                                  \
        else if constexpr ((cnt_) == 2) G3_WAIT_VM(6);                                             \
        else G3_WAIT_VM(0);                                                                        \
    }

    f16x8 bq[2], bh[2], aq[4][2];
    constexpr bool SPREAD = VAR == 4 && (!HI || GEN);
    G3_WAIT_VM(0);                                          // stores of a previous segment
    G2_ISSUE(0)
    if (nst > 1) G2_ISSUE(1)
    if (nst > 2) G2_ISSUE(2)
    // step 0 landed (everything issued after it may stay in flight)
    if (nst > 2) G2_WAIT_AHEAD(2) else if (nst > 1) G2_WAIT_AHEAD(1) else G2_WAIT_AHEAD(0)
    if (grp == 1) G3_RAW_BARRIER()
    if constexpr (SPREAD) {
#define G2_READ_A(s_)                                                                              \
        {                                                                                          \
            const unsigned char* bb = smem + ((s_) % IMGS) * IMG;                                  \
            _Pragma("unroll") for (int n = 0; n < 2; ++n) bq[n] = G2_FRAG(bb + b_off + n * 32 * 32); \
            _Pragma("unroll") for (int m = 0; m < 2; ++m) {                                        \
                aq[m][1] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s1);                          \
                aq[m][0] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s0);                          \
            }                                                                                      \
            if constexpr (HI) { _Pragma("unroll") for (int n = 0; n < 2; ++n) bh[n] = G2_FRAG(bb + b_off + G2_B + n * 32 * 32); } \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }
#define G2_READ_B(s_)                                                                              \
        {                                                                                          \
            const unsigned char* bb = smem + ((s_) % IMGS) * IMG;                                  \
            _Pragma("unroll") for (int m = 2; m < 4; ++m) {                                        \
                aq[m][1] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s1);                          \
                aq[m][0] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s0);                          \
            }                                                                                      \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }
#define G2_STEP(MORE_)                                                                             \
        {                                                                                          \
            G3_RAW_BARRIER()                                        /* X_s: image (s + 3) % 4 = (s - 1) % 4 is free */ \
            G2_READ_A(s)                                                                           \
            G2_MFMA(bq, 0, 1) G2_MFMA(bq, 1, 1)                                                    \
            if (MORE_) G2_PIECE(s + AHEAD, 0)                                                      \
            G2_MFMA(bq, 0, 0) G2_MFMA(bq, 1, 0)                                                    \
            G2_READ_B(s)                                                                           \
            if (MORE_) G2_PIECE(s + AHEAD, 1)                                                      \
            if constexpr (HI) { G2_MFMA(bh, 0, 0) G2_MFMA(bh, 1, 0) }                              \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                     \
            /* step s+1 must have landed before Y_s; step s+2 (4 / 3 pieces) and the two pieces of step s+3 just issued may stay in flight */ \
            if (s + 1 < nst) { if (MORE_) { if constexpr (HI) G3_WAIT_VM(6); else G3_WAIT_VM(5); } else G3_WAIT_VM(0); } \
            G3_RAW_BARRIER()                                        /* Y_s */                      \
            G2_MFMA(bq, 2, 1) G2_MFMA(bq, 3, 1)                                                    \
            if (MORE_) G2_PIECE(s + AHEAD, 2)                                                      \
            G2_MFMA(bq, 2, 0) G2_MFMA(bq, 3, 0)                                                    \
            if constexpr (HI) { if (MORE_) G2_PIECE(s + AHEAD, 3)                                  \
                                G2_MFMA(bh, 2, 0) G2_MFMA(bh, 3, 0) }                              \
        }
        {
            int s = 0;
            const int n_main = nst - AHEAD;                         // steps that still have a step to request
            for (; s < n_main; ++s) G2_STEP(true)
            for (; s < nst; ++s) G2_STEP(false)
        }
#undef G2_STEP
#undef G2_READ_B
#undef G2_READ_A
    } else {
#define G2_READ(s_)                                                                                \
        {                                                                                          \
            const unsigned char* bb = smem + ((s_) % IMGS) * IMG;                                  \
            _Pragma("unroll") for (int n = 0; n < 2; ++n) bq[n] = G2_FRAG(bb + b_off + n * 32 * 32); \
            if (HI) { _Pragma("unroll") for (int n = 0; n < 2; ++n) bh[n] = G2_FRAG(bb + b_off + G2_B + n * 32 * 32); } \
            _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                        \
                aq[m][0] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s0);                          \
                aq[m][1] = G2_FRAG(bb + a_row + m * 32 * G2_ROWB + a_s1);                          \
            }                                                                                      \
            __builtin_amdgcn_sched_barrier(0);                                                     \
        }
#define G2_MFMA4(b_, ma_, mb_) G2_MFMA(b_, ma_, 1) G2_MFMA(b_, mb_, 1) G2_MFMA(b_, ma_, 0) G2_MFMA(b_, mb_, 0)
#define G2_MFMA2H(b_, ma_, mb_) G2_MFMA(b_, ma_, 0) G2_MFMA(b_, mb_, 0)
#define G2_HALF(ma_, mb_)                                                                          \
        {                                                                                          \
            G2_MFMA4(bq, ma_, mb_)                                                                 \
            if (HI) { if (hi_blk) { if constexpr (GEN) { G2_MFMA2H(bh, ma_, mb_) } else { G2_MFMA4(bh, ma_, mb_) } } } \
        }
        for (int s = 0; s < nst; ++s) {
            const bool hi_blk = G2_BLKFLAG(s);
            G3_RAW_BARRIER()                                        // X_s
            if (s + AHEAD < nst) G2_ISSUE(s + AHEAD)
            G2_READ(s)
            G2_HALF(0, 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this image is free once both groups pass here
            // step s+1 must have landed before Y_s; later ones may stay in flight
            if (s + 1 < nst) {
                if (s + 3 < nst) G2_WAIT_AHEAD(2) else if (s + 2 < nst) G2_WAIT_AHEAD(1) else G2_WAIT_AHEAD(0)
            }
            G3_RAW_BARRIER()                                        // Y_s
            G2_HALF(2, 3)
        }
#undef G2_HALF
#undef G2_MFMA2H
#undef G2_MFMA4
#undef G2_READ
    }
    if (grp == 0) G3_RAW_BARRIER()
#undef G2_WAIT_AHEAD
#undef G2_MFMA
#undef G2_FRAG
#undef G2_PIECE
#undef G2_ISSUE
#undef G2_BLKFLAG

    if (C == nullptr) return;                                // (kept for the instruction stream: see the head comment)
    const int j = j0 + wn * 64 + li;
    // general (not count-structured) X as two f16 planes of x * 2^s_j (SplitF16, kernels_planes.hip.h): the per-column
    // exponent is undone here (a power of two: exact); 1 otherwise
    const float cs[2] = {(HI && cscale) ? cscale[j] : 1.0f, (HI && cscale) ? cscale[j + 32] : 1.0f};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (!G2_LIVE(m)) continue;                       // nobody reads the products of dead columns
        const int cbase = m0 + grp * 128 + m * 32 + 4 * h;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = cbase + (r & 3) + 8 * (r >> 2);
                C[(size_t)row * ldc + j + n * 32] = (acc[m][n][r] * rscale[row]) * cs[n];
            }
    }
#undef G2_LIVE
}

// ... and the overload for NSUB = 2: the 16x16x32 body (one X plane: no Bhi, hiflag, cscale), U8 deduced from the tag
template <bool HI, int VAR, bool NTB, bool PART, bool GEN, bool U8>
__device__ __forceinline__ void gemm2h_segment(G2Sub<2, U8>, const unsigned char* __restrict__ A2, const unsigned char* __restrict__ B1,
                                               const unsigned char* __restrict__, const unsigned int* __restrict__,
                                               const float* __restrict__ rscale, int Kb, float* __restrict__ C, int ldc,
                                               int m0, int j0, int kb0, int nkb, unsigned char* smem, const float* __restrict__,
                                               unsigned live)
{
    static_assert(!HI && !GEN, "two blocks per step: one count plane only");
    gemm2h_segment_mf16<VAR, NTB, PART, U8>(A2, B1, rscale, Kb, C, ldc, m0, j0, kb0, nkb, smem, live);
}

// pass B (and pass A on few tiles): split-K launch, XCD-aware order as gemm3c_kernel.  kb_per is a multiple of NSUB.
template <int NSUB, bool HI, int VAR = 0, bool PART = false, bool GEN = false, bool U8 = false>
__global__ __launch_bounds__(512) void gemm2h_kernel(const unsigned char* __restrict__ A2,
                                                     const unsigned char* __restrict__ B1,
                                                     const unsigned char* __restrict__ Bhi,
                                                     const unsigned int* __restrict__ hiflag,
                                                     const float* __restrict__ rscale, int Kb,
                                                     float* __restrict__ C, int ldc, long long c_split_stride,
                                                     int kb_per, const float* __restrict__ cscale = nullptr,
                                                     unsigned long long livemask = ~0ull)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
    int jt = blockIdx.x, mg = blockIdx.y, z = blockIdx.z;
    if ((gridDim.z & 7) == 0) {
        // XCD-aware order (block L runs on XCD L % 8, each XCD has its own L2): one XCD gets ALL row tiles jt and ALL
        // component groups mg of the K splits z = xcd, xcd + 8, ... -- the workgroups that share a factor segment
        // (same mg, z) or an X-plane segment (same jt, z) then share it in one L2.
        const int L = blockIdx.x + (int)gridDim.x * (blockIdx.y + (int)gridDim.y * blockIdx.z);
        const int xcd = L & 7, idx = L >> 3;
        jt = idx % (int)gridDim.x;
        mg = (idx / (int)gridDim.x) % (int)gridDim.y;
        z = xcd + 8 * (idx / (int)(gridDim.x * gridDim.y));
    }
    const int kb0 = z * kb_per;
    const int nkb = min(kb_per, Kb - kb0);
    gemm2h_segment<HI, VAR, true, PART, GEN>(G2Sub<NSUB, U8>{}, A2, B1, Bhi, hiflag, rscale, Kb, C ? C + (size_t)z * c_split_stride : nullptr, ldc, mg * G3_MW,
                                                   jt * G3C_JW, kb0, nkb, smem3, cscale, (unsigned)((livemask >> (8 * mg)) & 0xffu));
}

// pass A: stream-K over persistent workgroups, unit = one step of NSUB blocks (Kb % NSUB == 0)
template <int NSUB, bool HI, int VAR = 0, bool NTB = true, bool PART = false, bool GEN = false, bool U8 = false>
__global__ __launch_bounds__(512) void gemm2h_streamk_kernel(const unsigned char* __restrict__ A2,
                                                             const unsigned char* __restrict__ B1,
                                                             const unsigned char* __restrict__ Bhi,
                                                             const unsigned int* __restrict__ hiflag,
                                                             const float* __restrict__ rscale, int Kb,
                                                             float* __restrict__ C0, float* __restrict__ C1,
                                                             float* __restrict__ C2, int ldc, int MG, int T, int xmap,
                                                             const float* __restrict__ cscale = nullptr,
                                                             unsigned long long livemask = ~0ull)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
    const int Ks = Kb / NSUB;                             // steps per tile
    const long long U = (long long)T * Ks;
    // Work order: component group major (tile o = mg * NJ + jt), and -- xmap -- workgroup p takes the q-th share with
    // q = (p % MG) * (P / MG) + p / MG: block p runs on XCD p % 8, so each XCD works inside ONE component group and its
    // 4 MB L2 keeps that group's factor planes (2 MB at 2000 genes; the planes of four groups would thrash it: 1.5 GB
    // fetched per launch at 1024 columns, PMC), while neighbouring XCDs stream the SAME row tile jt of the X plane at
    // the same time (one HBM fetch, the others find it in the Infinity Cache).  The cut flags the sweep reads are indexed
    // jt * MG + mg (plan_streamk3); the set of cut positions does not depend on the permutation.
    const int P = (int)gridDim.x;
    const int q = (xmap && MG > 1 && P % MG == 0) ? ((int)blockIdx.x % MG) * (P / MG) + (int)blockIdx.x / MG : (int)blockIdx.x;
    long long u = U * q / P;
    const long long u1 = U * (q + 1) / P;
    const int NJ = T / MG;
    while (u < u1) {
        const int tile = (int)(u / Ks), ks = (int)(u % Ks);
        const int ke = (int)min((long long)Ks, ks + (u1 - u));
        const int mg = tile / NJ, jt = tile % NJ;
        gemm2h_segment<HI, VAR, NTB, PART, GEN>(G2Sub<NSUB, U8>{}, A2, B1, Bhi, hiflag, rscale, Kb, (ks == 0) ? C0 : (ke == Ks ? C1 : C2), ldc, mg * G3_MW,
                                                      jt * G3C_JW, ks * NSUB, (ke - ks) * NSUB, smem3, cscale,
                                                      (unsigned)((livemask >> (8 * mg)) & 0xffu));
        u += ke - ks;
        G3_WAIT_VM(0);
        __syncthreads();                 // the images are refilled by the next segment's DMA
    }
}

}  // namespace cnmf
