// The consensus clustergram (cnmf.py:986-1009, 1028) on the device (included by cnmf_hip.hip).
//
// cnmf_clustergram(): distances of the KEPT spectra (l2_rows_kernel + dist_sym_kernel on the kept rows only, cnmf.py:988)
// -> one m_c x m_c block per k-means cluster -> average-linkage (UPGMA) agglomeration of every block, one workgroup per
// cluster -> leaf order of every dendrogram, left child first -> the distance matrix permuted by that order.
//
// The agglomeration restates tests/_upgma_ref.py step for step (not scipy's nearest-neighbour chain):
//   * among live slots the pair a < b with the smallest distance merges, ties to the smallest a, then the smallest b;
//   * d(a,t) = (size_a * d(a,t) + size_b * d(b,t)) / (size_a + size_b): two products, one sum, one quotient, never fused;
//   * the merged group keeps slot a and takes id m + step, slot b is retired.
// With distinct heights the rows equal scipy.cluster.hierarchy.linkage(..., 'average'); where heights tie the rule above
// decides.
#pragma once
#include <vector>

#include "kernels_consensus.hip.h"

#define CNMF_LINKAGE_NT 512           /* threads of upgma_kernel (8 waves) */

namespace cnmf {

// B_c[i][j] = max(D[mem[seg_c + i]][mem[seg_c + j]], 0) for every cluster c (cnmf.py:1001-1002); one workgroup per
// cluster-ordered position p = seg_c + i.  mem: kept-row ids sorted by cluster, ascending inside a cluster.
__global__ __launch_bounds__(256) void cluster_blocks_gather(const double* __restrict__ D, int ldd,
                                                             const int* __restrict__ mem, const int* __restrict__ cl_of,
                                                             const int* __restrict__ seg, const long long* __restrict__ boff,
                                                             double* __restrict__ blocks)
{
    const int p = blockIdx.x, c = cl_of[p], b = seg[c], m = seg[c + 1] - b, i = p - b;
    const double* drow = D + (size_t)mem[p] * ldd;
    double* out = blocks + boff[c] + (size_t)i * m;
    for (int j = threadIdx.x; j < m; j += 256) {
        const double v = drow[mem[b + j]];
        out[j] = v < 0.0 ? 0.0 : v;
    }
}

// (d1, i1) goes before (d2, i2): no candidate yet, a smaller distance, or the same distance at a smaller index.  Written
// so that a NaN distance can still be taken when nothing else is there: the merge loop always finds a pair.
__device__ __forceinline__ bool lk_before(double d1, int i1, double d2, int i2)
{
    return i1 >= 0 && (i2 < 0 || d1 < d2 || (d1 == d2 && i1 < i2));
}

__device__ __forceinline__ void lk_wave_min(double& d, int& i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (lk_before(od, oi, d, i)) { d = od; i = oi; }
    }
}

// the weighted average of one merge with exactly four roundings (no contraction into an FMA)
__device__ __forceinline__ double lk_average(double sa, double x, double sb, double y, double st)
{
#pragma clang fp contract(off)
    const double p = sa * x;
    const double q = sb * y;
    const double s = p + q;
    return s / st;
}

// One workgroup per cluster, in place on its block B (m x m, symmetric, row-major).  LDS per slot (20 bytes): the nearest
// live neighbour ABOVE the slot (distance nd, index nn; -1 none, -2 to be rescanned), the group's size (0 = retired) and
// its id.  Each pair a < b is cached at slot a only, so the cached minimum with ties to the smallest slot IS the pair the
// rule asks for.  Per merge: argmin over the cached neighbours, the row update (row and column a), a rescan of slot a and
// of the slots below b whose cached neighbour was a or b.  After the m - 1 merges the Z rows of the cluster are copied
// into LDS and one lane walks them from the root down: offset(left) = offset(node), offset(right) = offset(node) +
// size(left); a leaf writes its member into order_out.
__global__ __launch_bounds__(CNMF_LINKAGE_NT) void upgma_kernel(double* blocks, const long long* __restrict__ boff,
                                                                const int* __restrict__ seg, const int* __restrict__ mem,
                                                                double* Z, int* __restrict__ order_out)
{
    constexpr int NT = CNMF_LINKAGE_NT, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) double lk_lds[];
    __shared__ double red_d[2][NW];
    __shared__ int red_i[2][NW];
    const int c = blockIdx.x, s0 = seg[c], m = seg[c + 1] - s0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (m == 1) { if (tid == 0) order_out[s0] = mem[s0]; return; }
    double* nd = lk_lds;                              // [m]
    int* nn = reinterpret_cast<int*>(lk_lds + m);     // [m]
    int* sz = nn + m;                                 // [m]
    int* id = sz + m;                                 // [m]
    double* B = blocks + boff[c];
    double* Zc = Z + (size_t)(s0 - c) * 4;            // clusters in label order: c clusters before this one gave s0 - c rows

    for (int i = tid; i < m; i += NT) { nn[i] = -2; sz[i] = 1; id[i] = i; nd[i] = 0.0; }
    __syncthreads();

    // nearest live neighbour above every flagged slot below `lim`: 64 slots per wave step, one wave per flagged row
    auto rescan = [&](int lim) {
        for (int base = wave * 64; base < lim; base += NW * 64) {
            const int s = base + lane;
            unsigned long long mask = __ballot(s < lim && nn[s] == -2);
            while (mask) {
                const int i = base + __builtin_ctzll(mask);
                mask &= mask - 1;
                const double* row = B + (size_t)i * m;
                double bd = 0.0; int bj = -1;
                for (int j = i + 1 + lane; j < m; j += 64)
                    if (sz[j] > 0) { const double d = row[j]; if (lk_before(d, j, bd, bj)) { bd = d; bj = j; } }
                lk_wave_min(bd, bj);
                if (lane == 0) { nd[i] = bd; nn[i] = bj; }
            }
        }
    };
    rescan(m);
    __syncthreads();

    for (int step = 0; step < m - 1; ++step) {
        // ---- the closest pair
        double bd = 0.0; int bi = -1;
        for (int i = tid; i < m; i += NT)
            if (sz[i] > 0 && nn[i] >= 0) { const double d = nd[i]; if (lk_before(d, i, bd, bi)) { bd = d; bi = i; } }
        lk_wave_min(bd, bi);
        double* rd = red_d[step & 1]; int* ri = red_i[step & 1];      // two buffers: the next step may write while this one is read
        if (lane == 0) { rd[wave] = bd; ri[wave] = bi; }
        __syncthreads();
        bd = rd[0]; bi = ri[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) if (lk_before(rd[w], ri[w], bd, bi)) { bd = rd[w]; bi = ri[w]; }
        const int a = bi;
        if (a < 0) return;                            // (cannot happen with two live slots; uniform)
        const int b = nn[a];
        const int sa = sz[a], sb = sz[b], ida = id[a], idb = id[b];
        __syncthreads();                              // every thread holds the pair before its slots change
        if (tid == 0) {
            Zc[(size_t)step * 4 + 0] = (double)min(ida, idb);
            Zc[(size_t)step * 4 + 1] = (double)max(ida, idb);
            Zc[(size_t)step * 4 + 2] = bd;
            Zc[(size_t)step * 4 + 3] = (double)(sa + sb);
            sz[a] = sa + sb; id[a] = m + step; sz[b] = 0; nn[a] = -2;
        }
        // ---- row update (threads touch slots other than a and b only)
        const double fa = (double)sa, fb = (double)sb, ft = (double)(sa + sb);
        const double* rowa = B + (size_t)a * m;
        const double* rowb = B + (size_t)b * m;
        for (int t = tid; t < m; t += NT) {
            if (t == a || t == b || sz[t] <= 0) continue;
            const double v = lk_average(fa, rowa[t], fb, rowb[t], ft);
            B[(size_t)a * m + t] = v;
            B[(size_t)t * m + a] = v;
            if (t < a) {
                const int n = nn[t];
                if (n == a || n == b) nn[t] = -2;
                else if (lk_before(v, a, nd[t], n)) { nd[t] = v; nn[t] = a; }
            } else if (t < b) {
                if (nn[t] == b) nn[t] = -2;
            }
        }
        __syncthreads();
        rescan(b);
        __syncthreads();
    }

    // ---- leaf order: Z of this cluster into LDS (left, right, size), then a walk from the root down
    int* left = nn; int* right = sz; int* cnt = id; int* off = reinterpret_cast<int*>(nd);
    for (int s = tid; s < m - 1; s += NT) {
        left[s] = (int)Zc[(size_t)s * 4 + 0];
        right[s] = (int)Zc[(size_t)s * 4 + 1];
        cnt[s] = (int)Zc[(size_t)s * 4 + 3];
    }
    __syncthreads();
    if (tid == 0) {
        off[m - 2] = 0;
        for (int s = m - 2; s >= 0; --s) {            // a node's parent has a larger id: its offset is already known
            const int o = off[s], l = left[s], r = right[s];
            const int nl = l < m ? 1 : cnt[l - m];
            if (l < m) order_out[s0 + o] = mem[s0 + l]; else off[l - m] = o;
            if (r < m) order_out[s0 + o + nl] = mem[s0 + r]; else off[r - m] = o + nl;
        }
    }
}

// out[p][q] = D[order[p]][order[q]]   (cnmf.py:1028), one coalesced write pass; grid (n / 256, n)
__global__ __launch_bounds__(256) void ordered_image_kernel(const double* __restrict__ D, int ldd,
                                                            const int* __restrict__ order, int n,
                                                            double* __restrict__ out)
{
    const int p = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) out[(size_t)p * n + q] = D[(size_t)order[p] * ldd + order[q]];
}

}  // namespace cnmf

extern "C" int cnmf_clustergram(cnmf_ctx* ctx, const double* spectra, const int64_t* store_rows, int R, int G,
                                const int32_t* labels, int k, int32_t* order_out, double* Z_out, int32_t* seg_out,
                                double* image_out)
{
    using namespace cnmf;
    if (!ctx || !labels || !order_out || !seg_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if ((spectra != nullptr) == (store_rows != nullptr)) { SET_ERR(ctx, "exactly one of spectra / store_rows must be given"); return CNMF_EINVAL; }
    if (R < 1 || G < 1 || k < 1 || k > R) { SET_ERR(ctx, "bad shape R=%d G=%d k=%d", R, G, k); return CNMF_EINVAL; }
    if (store_rows) {
        if ((int64_t)G != ctx->spectra_G) { SET_ERR(ctx, "the resident store holds spectra over %lld genes, not %d", (long long)ctx->spectra_G, G); return CNMF_EINVAL; }
        for (int r = 0; r < R; ++r)
            if (store_rows[r] < 0 || (size_t)store_rows[r] >= ctx->spectra_rows) { SET_ERR(ctx, "store row %lld outside 0..%lld", (long long)store_rows[r], (long long)ctx->spectra_rows - 1); return CNMF_EINVAL; }
    }
    // ---- everything that can be refused is refused here, before any launch
    std::vector<int> seg(k + 1, 0), keep_idx;
    for (int r = 0; r < R; ++r) {
        if (labels[r] < -1 || labels[r] >= k) { SET_ERR(ctx, "label %d of row %d outside -1..%d", (int)labels[r], r, k - 1); return CNMF_EINVAL; }
        if (labels[r] >= 0) { seg[labels[r] + 1]++; keep_idx.push_back(r); }
    }
    int max_m = 0;
    for (int c = 0; c < k; ++c) {
        if (seg[c + 1] == 0) { SET_ERR(ctx, "cluster %d is empty", c); return CNMF_EINVAL; }
        max_m = std::max(max_m, seg[c + 1]);
    }
    if (max_m > CNMF_LINKAGE_MAX) { SET_ERR(ctx, "a cluster of %d spectra is above the limit of %d", max_m, CNMF_LINKAGE_MAX); return CNMF_EUNSUPPORTED; }
    for (int c = 0; c < k; ++c) seg[c + 1] += seg[c];
    const int Rk = (int)keep_idx.size();
    // ints of one upload: mem [Rk] (kept-row ids by cluster, ascending inside) | cl_of [Rk] | seg [k+1] | kept rows [Rk]
    std::vector<int> ints((size_t)3 * Rk + k + 1);
    int* mem = ints.data(), *cl_of = mem + Rk, *hseg = cl_of + Rk, *krows = hseg + k + 1;
    std::vector<long long> boff(k);
    {
        std::vector<int> pos(seg.begin(), seg.begin() + k);
        for (int q = 0; q < Rk; ++q) { const int c = labels[keep_idx[q]], p = pos[c]++; mem[p] = q; cl_of[p] = c; krows[q] = keep_idx[q]; }
        long long run = 0;
        for (int c = 0; c < k; ++c) { hseg[c] = seg[c]; const long long m = seg[c + 1] - seg[c]; boff[c] = run; run += m * m; }
        hseg[k] = seg[k];
    }
    const size_t block_doubles = (size_t)(boff[k - 1] + (long long)(seg[k] - seg[k - 1]) * (seg[k] - seg[k - 1]));
    for (int c = 0; c <= k; ++c) seg_out[c] = seg[c];

    CONS_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Arena& pool = ctx->cons_ws;
    pool.reset();
    struct Trim { Arena& a; ~Trim() { if (a.total() > Arena::keep_limit) a.release(); } } trim{pool};
    struct Events {
        hipEvent_t e[6] = {};
        ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
    } ev;
    for (hipEvent_t& x : ev.e) CONS_TRY(hipEventCreate(&x));
    const int ld = round_up(G, 16), Rkp = round_up(Rk, 64);
    double* dS = pool.get<double>((size_t)Rk * G);
    double* dL2 = pool.get<double>((size_t)Rkp * ld, true, st);
    double* dsq = pool.get<double>(Rkp, true, st);
    double* dD = pool.get<double>((size_t)Rkp * Rkp);
    int* dints = pool.get<int>(ints.size());
    long long* dboff = pool.get<long long>(k);
    double* dblocks = pool.get<double>(block_doubles);
    double* dZ = pool.get<double>((size_t)std::max(Rk - k, 1) * 4);
    int* dorder = pool.get<int>(Rk, true, st);
    double* dimg = image_out ? pool.get<double>((size_t)Rk * Rk) : nullptr;
    if (pool.err) { SET_ERR(ctx, "device allocation failed"); return CNMF_ENOMEM; }
    const int* dmem = dints, *dcl = dints + Rk, *dseg = dints + 2 * Rk, *dkrows = dints + 2 * Rk + k + 1;
    CONS_TRY(hipMemcpyAsync(dints, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
    CONS_TRY(hipMemcpyAsync(dboff, boff.data(), (size_t)k * sizeof(long long), hipMemcpyHostToDevice, st));

    // ---- distances of the kept rows (cnmf.py:882, 988)
    CONS_TRY(hipEventRecord(ev.e[0], st));
    std::vector<long long> srows;                    // (lives until the stream has been synchronised)
    if (store_rows) {
        srows.resize(Rk);
        for (int q = 0; q < Rk; ++q) srows[q] = store_rows[keep_idx[q]];
        long long* drows = pool.get<long long>(Rk);
        if (pool.err) { SET_ERR(ctx, "device allocation failed"); return CNMF_ENOMEM; }
        CONS_TRY(hipMemcpyAsync(drows, srows.data(), (size_t)Rk * sizeof(long long), hipMemcpyHostToDevice, st));
        gather_store_rows_kernel<<<dim3((G + 255) / 256, Rk), 256, 0, st>>>(ctx->spectra, G, drows, dS);
    } else if (Rk == R) {
        CONS_TRY(hipMemcpyAsync(dS, spectra, (size_t)R * G * sizeof(double), hipMemcpyHostToDevice, st));
    } else {
        double* dall = pool.get<double>((size_t)R * G);
        if (pool.err) { SET_ERR(ctx, "device allocation failed"); return CNMF_ENOMEM; }
        CONS_TRY(hipMemcpyAsync(dall, spectra, (size_t)R * G * sizeof(double), hipMemcpyHostToDevice, st));
        gather_rows_kernel<<<dim3((G + 255) / 256, Rk), 256, 0, st>>>(dall, G, dkrows, Rk, G, dS, G);
    }
    l2_rows_kernel<<<Rk, 256, 0, st>>>(dS, Rk, G, dL2, ld, dsq);
    {
        const int nt = Rkp / 64;
        dist_sym_kernel<<<nt * (nt + 1) / 2, 256, 0, st>>>(dL2, ld, ld, dsq, Rk, dD, Rkp);
    }
    CONS_TRY(hipGetLastError());
    CONS_TRY(hipEventRecord(ev.e[1], st));

    // ---- one block per cluster, agglomerated in place; the matrix itself stays intact for the image
    cluster_blocks_gather<<<Rk, 256, 0, st>>>(dD, Rkp, dmem, dcl, dseg, dboff, dblocks);
    CONS_TRY(hipGetLastError());
    CONS_TRY(hipEventRecord(ev.e[2], st));
    const size_t lds = (size_t)max_m * 20;
    CONS_TRY(dyn_lds_optin((const void*)upgma_kernel, CNMF_LINKAGE_MAX * 20));
    upgma_kernel<<<k, CNMF_LINKAGE_NT, lds, st>>>(dblocks, dboff, dseg, dmem, dZ, dorder);
    CONS_TRY(hipGetLastError());
    CONS_TRY(hipEventRecord(ev.e[3], st));
    if (image_out) {
        ordered_image_kernel<<<dim3((Rk + 255) / 256, Rk), 256, 0, st>>>(dD, Rkp, dorder, Rk, dimg);
        CONS_TRY(hipGetLastError());
    }
    CONS_TRY(hipEventRecord(ev.e[4], st));
    CONS_TRY(hipMemcpyAsync(order_out, dorder, (size_t)Rk * sizeof(int), hipMemcpyDeviceToHost, st));
    if (Z_out && Rk > k) CONS_TRY(hipMemcpyAsync(Z_out, dZ, (size_t)(Rk - k) * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (image_out) CONS_TRY(hipMemcpyAsync(image_out, dimg, (size_t)Rk * Rk * sizeof(double), hipMemcpyDeviceToHost, st));
    CONS_TRY(hipEventRecord(ev.e[5], st));
    CONS_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < 5; ++s) {
        float ms = 0.0f;
        CONS_TRY(hipEventElapsedTime(&ms, ev.e[s], ev.e[s + 1]));
        ctx->clustergram_ms[s] = ms;
    }
    return CNMF_OK;
}

// device milliseconds of the last cnmf_clustergram by step (HIP events): distances | block gather | agglomeration and
// leaf order | ordered image | downloads
extern "C" int cnmf_clustergram_step_ms(const cnmf_ctx* ctx, double* out)
{
    if (!ctx || !out) return CNMF_EINVAL;
    for (int s = 0; s < 5; ++s) out[s] = ctx->clustergram_ms[s];
    return CNMF_OK;
}
