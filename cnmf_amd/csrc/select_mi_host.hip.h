// The mutual-information ranking of the reference's Preprocess.select_features_MI (preprocess.py:425-467):
// sklearn.feature_selection.mutual_info_classif(X, cluster, n_neighbors=3) over a dense preprocess slot, bit for bit.
//
//   * sklearn's _estimate_mi: X /= nanstd(X, 0) (ddof 0; a std below 10 eps -> 1), means = max(1, mean(|X|, 0)),
//     X += 1e-10 * means * standard_normal((N, G)) from numpy's GLOBAL RandomState.  sklearn reduces X[:, mask], which
//     numpy's fancy indexing lays out column-major, so every column statistic is numpy's pairwise sum over the
//     column's contiguous 8192-value blocks, the blocks added in order (the order of mean psi(m) too); the noise continues
//     the caller's MT19937 state (any pos, with or without a cached Gaussian) and the final state goes back to the host.
//   * The normals: one workgroup (the producer) runs the 3-phase twist of kernels_rng.hip.h over a chunk of blocks and
//     writes the raw key words; the consumers evaluate every 4-word candidate of the chunk in parallel, a prefix sum over
//     the accept flags places each accepted pair (f*x2, then f*x1) in the stream, and the emit writes the noisy copy
//     x / std + (1e-10 means) g in numpy's operation order.  Candidates straddling two chunks read the previous chunk's
//     last block, kept in slot 0 of the chunk buffer.
//   * Per gene (_compute_mi_cd): the kept cells (classes of >= 2 cells) sorted by the noisy value (LSD radix sort over
//     order-preserving 64-bit keys, 8 stable passes of 8 bits, segmented by gene), then a stable counting sort by class
//     gives each class its own sorted run.  The k-th distance to another member of the class: a two-pointer merge of
//     the left and right neighbours with |d| (sklearn's KD-tree), or for k >= n / 2 the expansion
//     sqrt(max((x_p x_p - 2 (x_p x_q)) + x_q x_q, 0)) over the whole class (sklearn's brute path).  radius =
//     nextafter(r_k, 0); m_i = two binary searches in the value-sorted column with the exact predicate
//     fl(c_j - c_i) <= radius.  mean psi(m) in numpy's order (pairwise sums of 8192-value blocks, added in order).
//
// Integer atomics only (radix histograms); no float atomics: two calls give the same bits.
// Included by cnmf_hip.hip after preprocess_host.hip.h.
#pragma once

namespace cnmf {

// ---------------------------------------------------------------- the noise stream
constexpr int MI_NB_MAX = 2048;          // MT blocks per producer chunk (5 MiB of words)

struct MiEmit {
    double* out;                         // MODE 0: the normals; MODE 1: the noisy copy [N][G]
    const double* X;                     // MODE 1: the slot [N][G]
    const double* scl;                   // MODE 1: the per-gene std divisor
    const double* cmul;                  // MODE 1: 1e-10 * means
    long long G;
};

struct MiFinal {
    long long c_last;                    // candidate that produced the last normal
    int e_last;                          // 0: it was f*x2 (f*x1 stays cached), 1: it was f*x1
};

// slots 1..nb of raw := the next nb MT blocks (block 0 of the stream is the caller's key, copied as it is)
__global__ __launch_bounds__(256) void mi_mt_produce_kernel(uint32_t* __restrict__ key, uint32_t* __restrict__ raw,
                                                            int nb, int first)
{
    __shared__ uint32_t s[2][MT_N];
    const int tid = threadIdx.x;
    for (int i = tid; i < MT_N; i += 256) s[0][i] = key[i];
    __syncthreads();
    int cur = 0;
    for (int b = 0; b < nb; ++b) {
        uint32_t* dst = raw + (size_t)(1 + b) * MT_N;
        if (first && b == 0) {
            for (int i = tid; i < MT_N; i += 256) dst[i] = s[cur][i];
            continue;
        }
        const uint32_t* o = s[cur];
        uint32_t* n = s[cur ^ 1];
        if (tid < MT_N - MT_M) { const uint32_t v = mt_mix(o[tid], o[tid + 1], o[tid + MT_M]); n[tid] = v; dst[tid] = v; }
        __syncthreads();
        if (tid < MT_N - MT_M) {
            const int i = tid + (MT_N - MT_M);
            const uint32_t v = mt_mix(o[i], o[i + 1], n[i - (MT_N - MT_M)]);
            n[i] = v; dst[i] = v;
        }
        __syncthreads();
        if (tid < MT_N - 2 * (MT_N - MT_M)) {
            const int i = tid + 2 * (MT_N - MT_M);
            const uint32_t nxt = (i == MT_N - 1) ? n[0] : o[i + 1];
            const uint32_t v = mt_mix(o[i], nxt, n[i - (MT_N - MT_M)]);
            n[i] = v; dst[i] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    __syncthreads();
    for (int i = tid; i < MT_N; i += 256) key[i] = s[cur][i];
}

// candidate c (stream words pos + 4c .. pos + 4c + 3; word p lives at raw[p - p0]): numpy's legacy_gauss body
__device__ __forceinline__ bool mi_candidate(const uint32_t* __restrict__ raw, long long rel, double& z0, double& z1)
{
#pragma clang fp contract(off)
    const uint32_t a0 = mt_temper(raw[rel]) >> 5, b0 = mt_temper(raw[rel + 1]) >> 6;
    const uint32_t a1 = mt_temper(raw[rel + 2]) >> 5, b1 = mt_temper(raw[rel + 3]) >> 6;
    const double d0 = ((double)a0 * 67108864.0 + (double)b0) / 9007199254740992.0;
    const double d1 = ((double)a1 * 67108864.0 + (double)b1) / 9007199254740992.0;
    const double x1 = 2.0 * d0 - 1.0, x2 = 2.0 * d1 - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    const bool acc = (r2 < 1.0) && (r2 != 0.0);
    if (acc) {
        const double f = sqrt(-2.0 * log(r2) / r2);
        z0 = f * x2;
        z1 = f * x1;
    }
    return acc;
}

struct MiChunk {
    long long c_lo, c_hi;                // candidates whose LAST word lies in this chunk's new blocks
    long long p0;                        // stream position of raw[0] (slot 0 = the previous chunk's last block)
    int pos;                             // the caller's pos: candidate c starts at word pos + 4c
};

__global__ __launch_bounds__(256) void mi_noise_count_kernel(const uint32_t* __restrict__ raw, const MiChunk ch,
                                                             unsigned* __restrict__ wcnt)
{
    __shared__ int ws[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = ch.c_lo + (long long)blockIdx.x * 256 + tid;
    bool acc = false;
    if (c < ch.c_hi) { double z0, z1; acc = mi_candidate(raw, ch.pos + 4 * c - ch.p0, z0, z1); }
    const unsigned long long bal = __ballot(acc);
    if (lane == 0) ws[wave] = __popcll(bal);
    __syncthreads();
    if (tid == 0) wcnt[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// woff[b] = accepted candidates before workgroup b of this chunk (over all chunks); *acc_total += this chunk's
__global__ __launch_bounds__(256) void mi_noise_scan_kernel(const unsigned* __restrict__ wcnt, int nwg,
                                                            long long* __restrict__ woff, long long* __restrict__ acc_total)
{
    __shared__ long long sc[256];
    const int tid = threadIdx.x;
    const int per = (nwg + 255) / 256, lo = min(nwg, tid * per), hi = min(nwg, lo + per);
    const long long base = *acc_total;
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += wcnt[i];
    sc[tid] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const long long v = tid >= o ? sc[tid - o] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    long long run = base + sc[tid] - s;
    for (int i = lo; i < hi; ++i) { woff[i] = run; run += wcnt[i]; }
    if (tid == 255) *acc_total = base + sc[255];
}

template <int MODE>
__device__ __forceinline__ void mi_emit_one(const MiEmit& e, long long t, double z)
{
#pragma clang fp contract(off)
    if (MODE == 0) { e.out[t] = z; return; }
    const int j = (int)(t % e.G);
    e.out[t] = e.X[t] / e.scl[j] + e.cmul[j] * z;
}

template <int MODE>
__global__ __launch_bounds__(256) void mi_noise_emit_kernel(const uint32_t* __restrict__ raw, const MiChunk ch,
                                                            const long long* __restrict__ woff, long long lead,
                                                            long long total, const MiEmit e, MiFinal* __restrict__ fin)
{
    __shared__ int ws[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c = ch.c_lo + (long long)blockIdx.x * 256 + tid;
    bool acc = false;
    double z0 = 0.0, z1 = 0.0;
    if (c < ch.c_hi) acc = mi_candidate(raw, ch.pos + 4 * c - ch.p0, z0, z1);
    const unsigned long long bal = __ballot(acc);
    const int within = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) ws[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += ws[w];
    if (!acc) return;
    const long long t = lead + 2 * (woff[blockIdx.x] + before + within);
    if (t < total) mi_emit_one<MODE>(e, t, z0);
    if (t + 1 < total) mi_emit_one<MODE>(e, t + 1, z1);
    if (t == total - 1 || t + 1 == total - 1) {
        fin->c_last = c;
        fin->e_last = t == total - 1 ? 0 : 1;
    }
}

// t = 0 is the cached Gaussian
template <int MODE>
__global__ void mi_noise_lead_kernel(const MiEmit e, double gauss)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) mi_emit_one<MODE>(e, 0, gauss);
}

// numpy's pairwise sum (loops_utils.h.src) of f(i0) .. f(i0 + n - 1); f(i) = v[i * stride] transformed by op:
//   0: v    1: (v - a) * (v - a)    2: |v / a|
struct MiSeq {
    const double* v; long long stride; int op; double a;
    __device__ __forceinline__ double operator()(long long i) const
    {
#pragma clang fp contract(off)
        const double x = v[i * stride];
        if (op == 0) return x;
        if (op == 1) { const double d = x - a; return d * d; }
        return fabs(x / a);
    }
};

__device__ __forceinline__ double mi_pw_leaf(const MiSeq& f, long long i0, int n)
{
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += f(i0 + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = f(i0 + u);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] += f(i0 + i + u);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += f(i0 + i);
    return res;
}

// (split at n / 2 rounded down to a multiple of 8 while n > 128; 8 levels cover n <= 8192)
template <int D>
__device__ __noinline__ double mi_pw(const MiSeq f, long long i0, int n)
{
#pragma clang fp contract(off)
    if (n <= 128) return mi_pw_leaf(f, i0, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return mi_pw<D - 1>(f, i0, n2) + mi_pw<D - 1>(f, i0 + n2, n - n2);
}
template <>
__device__ __noinline__ double mi_pw<0>(const MiSeq f, long long i0, int n)
{
    return mi_pw_leaf(f, i0, n);
}

// numpy's add.reduce of a contiguous run of n values: the pairwise sums of its 8192-value blocks, added in order
__device__ double mi_sum(const MiSeq& f, long long n)
{
#pragma clang fp contract(off)
    double total = 0.0;
    for (long long b = 0; b < n; b += 8192) total += mi_pw<8>(f, b, (int)min<long long>(8192, n - b));
    return total;
}

// ---------------------------------------------------------------- column statistics (sklearn's scale + means)
// sklearn reduces X[:, continuous_mask], an F-ordered copy: every column sum is numpy's blocked pairwise sum
__global__ __launch_bounds__(256) void mi_colstats_kernel(const double* __restrict__ X, long long N, int G,
                                                          double* __restrict__ scl, double* __restrict__ cmul)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= G) return;
    const double avg = mi_sum(MiSeq{X + j, G, 0, 0.0}, N) / (double)N;
    const double sd = sqrt(mi_sum(MiSeq{X + j, G, 1, avg}, N) / (double)N);
    const double sc = sd < 10.0 * 2.220446049250313e-16 ? 1.0 : sd;
    const double mean = mi_sum(MiSeq{X + j, G, 2, sc}, N) / (double)N;
    scl[j] = sc;
    cmul[j] = 1e-10 * (mean > 1.0 ? mean : 1.0);
}

// ---------------------------------------------------------------- per-gene sorts
__device__ __forceinline__ unsigned long long mi_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double mi_val(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// key[s][i] = the noisy value of kept cell i, gene j0 + s;  idx[s][i] = i
__global__ __launch_bounds__(256) void mi_gather_kernel(const double* __restrict__ Y, long long G,
                                                        const int* __restrict__ kept, int nk, int j0, int Gc,
                                                        unsigned long long* __restrict__ key, int* __restrict__ idx)
{
    const long long n = (long long)Gc * nk;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int s = (int)(e % Gc), i = (int)(e / Gc);
        const size_t o = (size_t)s * nk + i;
        key[o] = mi_key(Y[(size_t)kept[i] * G + j0 + s]);
        idx[o] = i;
    }
}

constexpr int MI_TILE = 2048;            // 256 threads x 8 rounds; tiles never span two genes

template <int MODE>                      // 0: digit of the key, 1: digit of the class of idx
__device__ __forceinline__ int mi_digit(unsigned long long k, int i, const int* cls, int shift)
{
    return MODE == 0 ? (int)((k >> shift) & 255ull) : ((cls[i] >> shift) & 255);
}

// H[(s * 256 + d) * T + t] = the tile's count of digit d
template <int MODE>
__global__ __launch_bounds__(256) void mi_radix_hist_kernel(const unsigned long long* __restrict__ key,
                                                            const int* __restrict__ idx, const int* __restrict__ cls,
                                                            int nk, int T, int shift, unsigned* __restrict__ H)
{
    __shared__ unsigned h[256];
    const int tid = threadIdx.x, s = blockIdx.x / T, t = blockIdx.x % T;
    h[tid] = 0;
    __syncthreads();
    const size_t base = (size_t)s * nk;
    const int lo = t * MI_TILE, hi = min(nk, lo + MI_TILE);
    for (int e = lo + tid; e < hi; e += 256) atomicAdd(&h[mi_digit<MODE>(key[base + e], idx[base + e], cls, shift)], 1u);
    __syncthreads();
    H[((size_t)s * 256 + tid) * T + t] = h[tid];
}

// per gene: the counts become the exclusive offsets, in (digit, tile) order
__global__ __launch_bounds__(256) void mi_radix_scan_kernel(unsigned* __restrict__ H, int T)
{
    __shared__ unsigned sc[256];
    const int d = threadIdx.x;
    unsigned* row = H + ((size_t)blockIdx.x * 256 + d) * T;
    unsigned tot = 0;
    for (int t = 0; t < T; ++t) tot += row[t];
    sc[d] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned v = d >= o ? sc[d - o] : 0u;
        __syncthreads();
        sc[d] += v;
        __syncthreads();
    }
    unsigned run = sc[d] - tot;
    for (int t = 0; t < T; ++t) { const unsigned v = row[t]; row[t] = run; run += v; }
}

// stable scatter: a tile's elements in order, 256 per round; the rank among equal digits comes from 8 ballots per wave
template <int MODE>
__global__ __launch_bounds__(256) void mi_radix_scatter_kernel(const unsigned long long* __restrict__ kin,
                                                               const int* __restrict__ iin,
                                                               unsigned long long* __restrict__ kout,
                                                               int* __restrict__ iout, const int* __restrict__ cls,
                                                               int nk, int T, int shift, const unsigned* __restrict__ H)
{
    __shared__ unsigned base[256];
    __shared__ unsigned cnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x / T, t = blockIdx.x % T;
    base[tid] = H[((size_t)s * 256 + tid) * T + t];
    for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const size_t sb = (size_t)s * nk;
    const int lo = t * MI_TILE, hi = min(nk, lo + MI_TILE);
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int r = 0; r < MI_TILE / 256; ++r) {
        const int e = lo + r * 256 + tid;
        const bool valid = e < hi;
        unsigned long long k = 0;
        int i = 0, d = 0;
        if (valid) { k = kin[sb + e]; i = iin[sb + e]; d = mi_digit<MODE>(k, i, cls, shift); }
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bb = __ballot(valid && bit);
            m &= bit ? bb : ~bb;
        }
        const int rank = __popcll(m & lt);
        if (valid && rank == 0) cnt[wave][d] = __popcll(m);
        __syncthreads();
        if (valid) {
            unsigned off = base[d] + rank;
            for (int w = 0; w < wave; ++w) off += cnt[w][d];
            kout[sb + off] = k;
            iout[sb + off] = i;
        }
        __syncthreads();
        base[tid] += ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
        for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- radius and neighbour counts
// A: the kept cells of each gene sorted by value; B, Bi: the same partitioned by class (a sorted run per class).
// P[i][s] = psi(m_i) of kept cell i, gene s.
__global__ __launch_bounds__(256) void mi_radius_count_kernel(const unsigned long long* __restrict__ A,
                                                              const unsigned long long* __restrict__ B,
                                                              const int* __restrict__ Bi, const int* __restrict__ cls,
                                                              const int* __restrict__ cstart, int nk, int Gc, int K,
                                                              const double* __restrict__ psi, double* __restrict__ P)
{
#pragma clang fp contract(off)
    const long long n = (long long)Gc * nk;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int s = (int)(e / nk), r = (int)(e % nk);
    const unsigned long long* a = A + (size_t)s * nk;
    const unsigned long long* b = B + (size_t)s * nk;
    const int i = Bi[e];
    const int c = cls[i], cs = cstart[c], ce = cstart[c + 1], cn = ce - cs;
    const int k = min(K, cn - 1);
    const double xp = mi_val(b[r]);
    double rk = 0.0;
    if (k >= cn / 2) {
        // sklearn's brute path: the k smallest expansion distances to the other members
        double best[8];
        for (int q = 0; q < 8; ++q) best[q] = INFINITY;
        for (int q = cs; q < ce; ++q) {
            if (q == r) continue;
            const double xq = mi_val(b[q]);
            const double sq = (xp * xp - 2.0 * (xp * xq)) + xq * xq;
            double d = sqrt(sq > 0.0 ? sq : 0.0);
            for (int u = 0; u < k; ++u)
                if (d < best[u]) { const double w = best[u]; best[u] = d; d = w; }
        }
        rk = best[k - 1];
    } else {
        int l = r - 1, h = r + 1;
        for (int step = 0; step < k; ++step) {
            const double dl = l >= cs ? xp - mi_val(b[l]) : INFINITY;
            const double dh = h < ce ? mi_val(b[h]) - xp : INFINITY;
            if (dl <= dh) { rk = dl; --l; } else { rk = dh; ++h; }
        }
    }
    const double rad = rk > 0.0 ? __longlong_as_double(__double_as_longlong(rk) - 1) : 0.0;   // nextafter(rk, 0)
    int lo = 0, hi = nk;                 // first j with a[j] >= xp or xp - a[j] <= rad
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double v = mi_val(a[mid]);
        if (v >= xp || xp - v <= rad) hi = mid; else lo = mid + 1;
    }
    const int first = lo;
    lo = first; hi = nk;                 // first j with a[j] > xp and a[j] - xp > rad
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double v = mi_val(a[mid]);
        if (v > xp && v - xp > rad) hi = mid; else lo = mid + 1;
    }
    P[(size_t)i * Gc + s] = psi[lo - first];
}

// MI of gene j0 + s: ((psi(n) + mean psi(k)) - mean psi(label counts)) - mean psi(m), clipped at 0
__global__ __launch_bounds__(64) void mi_finish_kernel(const double* __restrict__ P, int nk, int Gc, double cst,
                                                       double* __restrict__ mi, int j0)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= Gc) return;
    const double v = cst - mi_sum(MiSeq{P + s, Gc, 0, 0.0}, nk) / (double)nk;
    mi[j0 + s] = v > 0.0 ? v : 0.0;
}

// ---------------------------------------------------------------- normalize_total + sc.pp.scale on a dense slot
// d[row][c] = the staged counts times the row scale (normalize_total's x * (target / row sum)), a wavefront per row
__global__ __launch_bounds__(256) void mi_store_scaled_kernel(const long long* __restrict__ ptr, const int* __restrict__ idx,
                                                              const double* __restrict__ val, int R, int C,
                                                              const double* __restrict__ scale, double* __restrict__ d)
{
    const int row = seg_index();
    if (row >= R) return;
    seg_for_each(ptr[row], ptr[row + 1], [&](long long p) { d[(size_t)row * C + idx[p]] = scale ? val[p] * scale[row] : val[p]; });
}

// the ddof=1 std of every column, as numpy's std(axis=0) of a C-ordered matrix sums: row after row
__global__ __launch_bounds__(256) void mi_col_std_kernel(const double* __restrict__ X, long long N, int G,
                                                         double* __restrict__ sd)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= G) return;
    const double* x = X + j;
    double s = 0.0;
#pragma unroll 8
    for (long long i = 0; i < N; ++i) s += x[i * G];
    const double mean = s / (double)N;
    double v = 0.0;
#pragma unroll 8
    for (long long i = 0; i < N; ++i) { const double d = x[i * G] - mean; v += d * d; }
    sd[j] = sqrt(v / (double)(N - 1));
}

// x / (std or 1 for a zero std), then x > max_value -> max_value
__global__ __launch_bounds__(256) void mi_scale_clip_kernel(double* __restrict__ X, long long n, int G,
                                                            const double* __restrict__ sd, double max_value)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double s = sd[i % G];
        const double v = X[i] / (s == 0.0 ? 1.0 : s);
        X[i] = v > max_value ? max_value : v;
    }
}

}  // namespace cnmf

// f * x1 of the accepted candidate made of the raw key words w (numpy's legacy_gauss, host arithmetic)
static double mi_host_cached_gauss(const uint32_t* w)
{
#pragma clang fp contract(off)
    uint32_t t[4];
    for (int i = 0; i < 4; ++i) {
        uint32_t y = w[i];
        y ^= (y >> 11);
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= (y >> 18);
        t[i] = y;
    }
    const double d0 = ((double)(t[0] >> 5) * 67108864.0 + (double)(t[1] >> 6)) / 9007199254740992.0;
    const double d1 = ((double)(t[2] >> 5) * 67108864.0 + (double)(t[3] >> 6)) / 9007199254740992.0;
    const double x1 = 2.0 * d0 - 1.0, x2 = 2.0 * d1 - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    const double f = std::sqrt(-2.0 * std::log(r2) / r2);
    return f * x1;
}

// normals t = 0 .. total-1 of numpy's legacy standard_normal continuing *s, written by MODE's emit; *s := the final state
template <int MODE>
static int mi_noise(cnmf_ctx* ctx, cnmf_mt_state* s, long long total, const cnmf::MiEmit& em)
{
    using namespace cnmf;
    hipStream_t st = ctx->stream;
    const long long lead = s->has_gauss ? 1 : 0;
    if (lead && total > 0) mi_noise_lead_kernel<MODE><<<1, 64, 0, st>>>(em, s->gauss);
    HIP_TRY(ctx, hipGetLastError());
    if (total <= lead) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (lead && total > 0) { s->has_gauss = 0; s->gauss = 0.0; }
        return CNMF_OK;
    }
    const int nwg_max = (MI_NB_MAX * (MT_N / 4) + 3 + 255) / 256 + 1;
    DevPool pool;
    uint32_t* key = pool.get<uint32_t>(MT_N);
    uint32_t* raw = pool.get<uint32_t>((size_t)(MI_NB_MAX + 1) * MT_N);
    unsigned* wcnt = pool.get<unsigned>(nwg_max);
    long long* woff = pool.get<long long>(nwg_max);
    long long* acc = pool.get<long long>(1, true, st);
    MiFinal* fin = pool.get<MiFinal>(1, true, st);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(key, s->key, MT_N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const long long pos = s->pos;
    long long b0 = 0, accepted = 0;
    int nb = 0;
    while (lead + 2 * accepted < total) {
        const long long remaining = total - lead - 2 * accepted;
        if (b0 > 0)        // slot 0 := the previous chunk's last block
            HIP_TRY(ctx, hipMemcpyAsync(raw, raw + (size_t)nb * MT_N, MT_N * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        nb = (int)std::min<long long>(MI_NB_MAX, (long long)(remaining * 2.6 / MT_N) + 2);
        mi_mt_produce_kernel<<<1, 256, 0, st>>>(key, raw, nb, b0 == 0 ? 1 : 0);
        MiChunk ch;
        const long long x0 = (long long)MT_N * b0 - pos - 3, x1 = (long long)MT_N * (b0 + nb) - pos - 3;
        ch.c_lo = x0 <= 0 ? 0 : (x0 + 3) / 4;
        ch.c_hi = x1 <= 0 ? 0 : (x1 + 3) / 4;
        ch.p0 = (long long)MT_N * (b0 - 1);
        ch.pos = (int)pos;
        if (ch.c_hi > ch.c_lo) {
            const int nwg = (int)((ch.c_hi - ch.c_lo + 255) / 256);
            mi_noise_count_kernel<<<nwg, 256, 0, st>>>(raw, ch, wcnt);
            mi_noise_scan_kernel<<<1, 256, 0, st>>>(wcnt, nwg, woff, acc);
            mi_noise_emit_kernel<MODE><<<nwg, 256, 0, st>>>(raw, ch, woff, lead, total, em, fin);
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&accepted, acc, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        b0 += nb;
    }
    MiFinal f;
    HIP_TRY(ctx, hipMemcpyAsync(&f, fin, sizeof f, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const long long pl = pos + 4 * f.c_last + 3;             // the last word the stream consumed
    const long long bl = pl / MT_N, slot = bl - (b0 - nb) + 1;
    if (slot < 0 || slot > nb) { SET_ERR(ctx, "MT19937 stream bookkeeping: block %lld outside the last chunk", bl); return CNMF_EHIP; }
    HIP_TRY(ctx, hipMemcpyAsync(s->key, raw + (size_t)slot * MT_N, MT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    s->pos = (int32_t)(pl % MT_N + 1);
    s->has_gauss = f.e_last == 0 ? 1 : 0;
    s->gauss = 0.0;
    if (f.e_last == 0) {
        // the cached Gaussian goes back into numpy's state: recompute it with the host's log(), the one numpy calls (the
        // device's log() may differ from it by one ulp)
        uint32_t w[4];
        const long long rel = pos + 4 * f.c_last - (long long)MT_N * (b0 - nb - 1);
        HIP_TRY(ctx, hipMemcpyAsync(w, raw + rel, sizeof w, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        s->gauss = mi_host_cached_gauss(w);
    }
    return CNMF_OK;
}

static int mi_state_arg(cnmf_ctx* ctx, const cnmf_mt_state* s)
{
    if (!s) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (s->pos < 0 || s->pos > cnmf::MT_N) { SET_ERR(ctx, "MT19937 pos %d outside [0, 624]", s->pos); return CNMF_EINVAL; }
    if (s->has_gauss != 0 && s->has_gauss != 1) { SET_ERR(ctx, "has_gauss = %d is not 0 or 1", s->has_gauss); return CNMF_EINVAL; }
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_row_sums(cnmf_ctx* ctx, double* row_sums)
{
    if (!ctx || !row_sums) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }      // (before "nothing staged", as ever)
    return pre_cell_sums(ctx, nullptr, row_sums);        // (filter_host.hip.h: the cell sums over all genes)
}

extern "C" int cnmf_preprocess_normalize_dense(cnmf_ctx* ctx, int32_t slot, double target_sum, double max_value,
                                               double* std_out)
{
    using namespace cnmf;
    if (int rc = pre_slot_arg(ctx, slot, false)) return rc;
    if (!std_out) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    if (!P.staged()) { SET_ERR(ctx, "cnmf_preprocess_upload_csr has not been called"); return CNMF_ESTATE; }
    const int N = (int)P.N, G = (int)P.counts.cols;
    if (N < 2) { SET_ERR(ctx, "need at least two cells for a variance"); return CNMF_EINVAL; }
    if (std::isnan(max_value)) { SET_ERR(ctx, "max_value is NaN"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PreSlot& S = P.slot[slot];
    hipStreamSynchronize(st);
    S.release();
    DevPool pool;
    double *rs, *scale = nullptr;
    double* sd = pool.get<double>(G);
    POOL_TRY(ctx, pool);
    const long long n = (long long)N * G;
    HIP_TRY(ctx, hipMalloc((void**)&S.dense, (size_t)n * sizeof(double)));
    S.n = G;
    HIP_TRY(ctx, hipMemsetAsync(S.dense, 0, (size_t)n * sizeof(double), st));
    if (target_sum > 0.0)
        if (int rc = stage_row_scale(ctx, P, target_sum, pool, &rs, &scale)) return rc;
    mi_store_scaled_kernel<<<seg_grid(N), 256, 0, st>>>(P.counts.ptr, P.counts.idx, P.counts.val, N, G, scale, S.dense);
    mi_col_std_kernel<<<(G + 255) / 256, 256, 0, st>>>(S.dense, N, G, sd);
    mi_scale_clip_kernel<<<pre_grid(n), 256, 0, st>>>(S.dense, n, G, sd, max_value);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(std_out, sd, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return CNMF_OK;
}

extern "C" int cnmf_preprocess_select_mi(cnmf_ctx* ctx, int32_t slot, const int32_t* cls, int32_t n_classes,
                                         int32_t n_neighbors, cnmf_mt_state* state, const double* psi, double cst,
                                         double* mi)
{
    using namespace cnmf;
    if (int rc = pre_need_dense(ctx, slot)) return rc;
    if (!cls || !psi || !mi) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    if (int rc = mi_state_arg(ctx, state)) return rc;
    if (n_neighbors < 1 || n_neighbors > 8) { SET_ERR(ctx, "n_neighbors = %d outside [1, 8]", n_neighbors); return CNMF_EINVAL; }
    if (n_classes < 1 || n_classes > 65536) { SET_ERR(ctx, "n_classes = %d outside [1, 65536]", n_classes); return CNMF_EINVAL; }
    PreStage& P = ctx->pre;
    PreSlot& S = P.slot[slot];
    const long long N = P.N, G = S.n;
    // the kept cells (cell order) and the class runs
    std::vector<int> kept, ccount(n_classes + 1, 0), hcls;
    for (long long i = 0; i < N; ++i) {
        if (cls[i] < -1 || cls[i] >= n_classes) { SET_ERR(ctx, "class id %d outside [-1, %d)", cls[i], n_classes); return CNMF_EINVAL; }
        if (cls[i] >= 0) { kept.push_back((int)i); hcls.push_back(cls[i]); ccount[cls[i] + 1]++; }
    }
    const int nk = (int)kept.size();
    for (int c = 0; c < n_classes; ++c) {
        if (ccount[c + 1] < 2) { SET_ERR(ctx, "class %d has %d cells (each kept class needs >= 2)", c, ccount[c + 1]); return CNMF_EINVAL; }
        ccount[c + 1] += ccount[c];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // elements per gene chunk: about 2^25 (40 B each)
    const int Gc = (int)std::max<long long>(1, std::min<long long>(G, (1ll << 25) / std::max(nk, 1)));
    const int T = (nk + MI_TILE - 1) / MI_TILE;
    const size_t E = (size_t)Gc * nk;
    DevPool pool;
    double* Y = pool.get<double>((size_t)N * G);
    double* scl = pool.get<double>(G);
    double* cmul = pool.get<double>(G);
    double* dmi = pool.get<double>(G);
    double* dpsi = pool.get<double>(N + 1);
    int* dkept = pool.get<int>(nk);
    int* dcls = pool.get<int>(nk);
    int* dcs = pool.get<int>(n_classes + 1);
    unsigned long long* k0 = pool.get<unsigned long long>(E);
    unsigned long long* k1 = pool.get<unsigned long long>(E);
    unsigned long long* k2 = pool.get<unsigned long long>(E);
    int* i0 = pool.get<int>(E);
    int* i1 = pool.get<int>(E);
    int* i2 = pool.get<int>(E);
    double* Pm = pool.get<double>(E);
    unsigned* H = pool.get<unsigned>((size_t)Gc * 256 * T);
    POOL_TRY(ctx, pool);
    HIP_TRY(ctx, hipMemcpyAsync(dpsi, psi, (size_t)(N + 1) * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dkept, kept.data(), (size_t)nk * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dcls, hcls.data(), (size_t)nk * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dcs, ccount.data(), (size_t)(n_classes + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    mi_colstats_kernel<<<(unsigned)((G + 255) / 256), 256, 0, st>>>(S.dense, N, (int)G, scl, cmul);
    HIP_TRY(ctx, hipGetLastError());
    MiEmit em{Y, S.dense, scl, cmul, G};
    cnmf_mt_state s = *state;
    if (int rc = mi_noise<1>(ctx, &s, N * G, em)) return rc;
    const int cpasses = n_classes > 256 ? 2 : 1;
    for (int j0 = 0; j0 < G; j0 += Gc) {
        const int gc = (int)std::min<long long>(Gc, G - j0);
        const long long n = (long long)gc * nk;
        mi_gather_kernel<<<pre_grid(n), 256, 0, st>>>(Y, G, dkept, nk, j0, gc, k0, i0);
        unsigned long long* ka = k0; unsigned long long* kb = k1;
        int* ia = i0; int* ib = i1;
        for (int shift = 0; shift < 64; shift += 8) {     // 8 passes: the sorted keys end in k0 / i0
            mi_radix_hist_kernel<0><<<gc * T, 256, 0, st>>>(ka, ia, nullptr, nk, T, shift, H);
            mi_radix_scan_kernel<<<gc, 256, 0, st>>>(H, T);
            mi_radix_scatter_kernel<0><<<gc * T, 256, 0, st>>>(ka, ia, kb, ib, nullptr, nk, T, shift, H);
            std::swap(ka, kb); std::swap(ia, ib);
        }
        unsigned long long* kc = k1; int* ic = i1;         // class partition: k0 -> k1 (-> k2)
        ka = k0; ia = i0;
        for (int p = 0; p < cpasses; ++p) {
            mi_radix_hist_kernel<1><<<gc * T, 256, 0, st>>>(ka, ia, dcls, nk, T, 8 * p, H);
            mi_radix_scan_kernel<<<gc, 256, 0, st>>>(H, T);
            mi_radix_scatter_kernel<1><<<gc * T, 256, 0, st>>>(ka, ia, kc, ic, dcls, nk, T, 8 * p, H);
            ka = kc; ia = ic; kc = k2; ic = i2;
        }
        mi_radius_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(k0, ka, ia, dcls, dcs, nk, gc, n_neighbors, dpsi, Pm);
        mi_finish_kernel<<<(gc + 63) / 64, 64, 0, st>>>(Pm, nk, gc, cst, dmi, j0);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(mi, dmi, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *state = s;
    return CNMF_OK;
}

#ifdef CNMF_DEBUG_ABI
extern "C" int cnmf_debug_mt_normals(cnmf_ctx* ctx, cnmf_mt_state* state, int64_t n, double* out)
{
    if (!ctx || !out || n < 0) { SET_ERR(ctx, "bad argument"); return CNMF_EINVAL; }
    if (int rc = mi_state_arg(ctx, state)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevPool pool;
    double* d = pool.get<double>((size_t)n);
    POOL_TRY(ctx, pool);
    cnmf::MiEmit em{d, nullptr, nullptr, nullptr, 1};
    cnmf_mt_state s = *state;
    if (int rc = mi_noise<0>(ctx, &s, n, em)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *state = s;
    return CNMF_OK;
}
#endif  // CNMF_DEBUG_ABI
