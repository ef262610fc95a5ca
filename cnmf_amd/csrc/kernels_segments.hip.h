// One wavefront per segment: the kernel shape of the staging statistics (prepare_host, preprocess_host, filter_host,
// hvg_host, hvg_batch_host, select_mi_host .hip.h and the column moments of csr_host.hip.h).  A segment is a row or a
// column of a compressed matrix, or a run inside one.
//
//   * a 256-thread workgroup holds four wavefronts; wavefront w of workgroup x serves segment 4 x + w (seg_index), so a
//     launch over n segments takes seg_grid(n) = ceil(n / 4) workgroups and every kernel starts with
//     `if (seg_index() >= n) return;`;
//   * the lanes walk the entry positions [begin, end) 64 apart (seg_for_each): lane l takes begin + l, begin + l + 64, ...
//     in that order and adds into accumulators of its own;
//   * the 64 lane partials are folded by a FIXED xor butterfly (seg_sum, seg_or): v += __shfl_xor(v, o, 64) for
//     o = 32, 16, 8, 4, 2, 1 in that order.  Every lane ends with the same value; lane 0 stores it.
//
// THE ORDER IS THE CONTRACT.  A float64 sum over a segment is exactly: lane l sums v[begin + l], v[begin + l + 64], ...
// sequentially from 0.0; then six rounds a[l] = a[l] + a[l ^ o], o = 32 ... 1.  "Two calls give the same bits" in the
// heads of the staging files, and "the batched kernels give the bits of the one-batch kernels on the restricted staging"
// in hvg_batch_host.hip.h, rest on every such kernel taking its order from here (tests/test_gpu_segment_order.py states
// it once more, in numpy).  A per-entry callable that multiplies before it adds says itself whether the two may fuse:
// `#pragma clang fp contract(off)` inside the callable where they must not.
//
// The index invariant: the reductions do not range-check the row or column index of an entry.  stage_counts
// (prepare_host.hip.h) refuses a column outside [0, C) on every upload path, and the row indices of a transpose are
// written by csr_tr_fill_kernel itself, so every index these kernels read is in range; a mask indexed by one needs no
// bound of its own.
// Included by cnmf_hip.hip (before csr_host.hip.h).
#pragma once

namespace cnmf {

__device__ __forceinline__ int seg_index() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
__device__ __forceinline__ int seg_lane() { return threadIdx.x & 63; }

// f(p) for the positions p of [begin, end) that fall to this lane, ascending
template <typename F>
__device__ __forceinline__ void seg_for_each(long long begin, long long end, F f)
{
    for (long long p = begin + seg_lane(); p < end; p += 64) f(p);
}

// the butterfly's rounds: step(o) for o = 32, 16, 8, 4, 2, 1; a step combines a lane's value with that of lane ^ o
template <typename F>
__device__ __forceinline__ void seg_butterfly(F step)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) step(o);
}

// the sum (seg_sum: double, long long or int) or the bit-or (seg_or) of v over the 64 lanes, on every lane
template <typename T>
__device__ __forceinline__ T seg_sum(T v)
{
    seg_butterfly([&](int o) { v += __shfl_xor(v, o, 64); });
    return v;
}

__device__ __forceinline__ int seg_or(int v)
{
    seg_butterfly([&](int o) { v |= __shfl_xor(v, o, 64); });
    return v;
}

// [*begin, *end) (a column whose rows crow ascend) := its run of the rows [row0, row1): two binary searches, the same on
// every lane of the wavefront
__device__ __forceinline__ void seg_row_run(const int* __restrict__ crow, int row0, int row1, long long* begin, long long* end)
{
    auto first_at_least = [&](long long lo, long long hi, int key) {     // the first p in [lo, hi) with crow[p] >= key
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (crow[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    *begin = first_at_least(*begin, *end, row0);
    *end = first_at_least(*begin, *end, row1);
}

}  // namespace cnmf

// workgroups of a launch over n segments
static inline unsigned seg_grid(long long n) { return (unsigned)((n + 3) / 4); }
