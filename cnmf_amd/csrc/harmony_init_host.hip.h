// Harmony's k-means initialisation on the device (cnmf_harmony_kmeans_init): scikit-learn's KMeans(k-means++, n_init,
// max_iter) on the unit scores Z_cos that cnmf_harmony_begin left on the device, step by step as oracle/consensus.py
// restates it.  N is tens of thousands of cells or more, d <= 64, K <= 128: the opposite shape of the consensus k-means
// (kernels_consensus.hip.h), which reads an all-pairs distance matrix of a few thousand spectra.
//
// Float64 throughout, no float atomics, no barrier across workgroups but the end of a launch.  Every sum over cells is taken
// over fixed chunks -- HCH cells for the column moments, PCH cells for the seeding potentials, hki_lloyd_chunk(N) cells for
// the cluster sums -- each chunk in a fixed order, the chunk partials added in chunk order: two runs give the same bits.
// All n_init inits go through every launch together; an init whose Lloyd loop has stopped leaves each kernel at its first
// instruction.
//
//   hki_colsum / hki_mean / hki_center / hki_tol   column means, centred scores Xc and their row norms x_sq, tol_
//   hki_pp_trial_kernel   one thread per cell, its scores in registers, the n_init x (L + 1) candidate vectors in LDS:
//                         closest = min(closest, distance to the centre chosen last), and per trial the chunk's share
//                         of the potential sum min(closest, distance to the candidate)
//   hki_pp_pick_kernel    one workgroup per init: the potentials (chunk order), the first minimum, and the next L
//                         candidates -- searchsorted(cumsum(closest), u pot): the chunk from a scan of the chunk totals,
//                         the cell from a scan inside that chunk
//   hki_assign_kernel     labels = first minimum over k of c_sq[k] - 2 x.c_k, the centres of one init in LDS; in its
//                         final form the last E step of the inits that need one, and every init's inertia per chunk
//   hki_accum / hki_reduce   per-cluster sums and counts: per chunk in ascending cell order, then in chunk order
//   hki_finish_kernel     one workgroup per init: empty clusters to the farthest cells, the means, the shift, the stopping rule
#pragma once

namespace cnmf {

constexpr int PCH = 256;    // cells per chunk of the seeding sums and scans: one workgroup

// cells per chunk of the cluster sums: the smallest multiple of HCH that leaves at most 256 chunks (a partial is K x d doubles)
static inline int hki_lloyd_chunk(int N) { return HCH * std::max(1, (N + HCH * 256 - 1) / (HCH * 256)); }

struct HkiDims { int N, Np, d, K, I, L, npch; };     // cells, padded cells, components, clusters, inits, local trials, PCH chunks

struct HkiInit {          // the Lloyd loop of one init
    int done;             // the loop has stopped
    int strict;           // ... because no label changed: no final E step
    int iters;            // iterations run
    int changed;          // a label changed in the E step of this iteration
};

// scikit-learn's squared distance: -2 x.c, + c_sq, + x_sq, every step rounded on its own, clamped at 0
__device__ __forceinline__ double hki_sqdist(double dot, double csq, double xsq)
{
    return fmax(__dadd_rn(__dadd_rn(__dmul_rn(-2.0, dot), csq), xsq), 0.0);
}

// inclusive scan over the 64 lanes of a wave in a fixed order; lane 63 holds the wave's total
__device__ __forceinline__ double hki_wave_scan(double v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off, 64);
        if (lane >= off) v = __dadd_rn(v, o);
    }
    return v;
}

// part[chunk][c] = sum over the cells of the chunk, ascending, of Z[c][n] (its square with `square`)
__global__ __launch_bounds__(64) void hki_colsum_kernel(const double* __restrict__ Z, int N, int Np, int d, int square,
                                                        double* __restrict__ part)
{
    const int c = threadIdx.x;
    if (c >= d) return;
    const int n0 = blockIdx.x * HCH, n1 = min(N, n0 + HCH);
    double s = 0.0;
    for (int n = n0; n < n1; ++n) {
        const double v = Z[(size_t)c * Np + n];
        s = __dadd_rn(s, square ? __dmul_rn(v, v) : v);
    }
    part[(size_t)blockIdx.x * d + c] = s;
}

__global__ __launch_bounds__(64) void hki_mean_kernel(const double* __restrict__ part, int nchunk, int d, int N,
                                                      double* __restrict__ mean)
{
    const int c = threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s = __dadd_rn(s, part[(size_t)ch * d + c]);
    mean[c] = s / (double)N;
}

// tol_ = mean over the components of the variance over the cells (part: the chunk sums of Xc^2), times tol
__global__ void hki_tol_kernel(const double* __restrict__ part, int nchunk, int d, int N, double tol, double* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int c = 0; c < d; ++c) {
        double s = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) s = __dadd_rn(s, part[(size_t)ch * d + c]);
        tot = __dadd_rn(tot, s / (double)N);
    }
    *out = __dmul_rn(tot / (double)d, tol);
}

__global__ __launch_bounds__(256) void hki_center_kernel(const double* __restrict__ Z, const double* __restrict__ mean, int N,
                                                         int Np, int d, double* __restrict__ Xc, double* __restrict__ xsq)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double ss = 0.0;
    for (int c = 0; c < d; ++c) {
        const double v = __dsub_rn(Z[(size_t)c * Np + n], mean[c]);
        Xc[(size_t)c * Np + n] = v;
        ss = fma(v, v, ss);
    }
    xsq[n] = ss;
}

__global__ __launch_bounds__(256) void hki_fill_kernel(double* __restrict__ p, size_t n, double v)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// x.c with the cell's scores in registers and the vector in LDS, c ascending; hki_pp_pick_kernel adds in the same order
template <int D>
__device__ __forceinline__ double hki_dot(const double (&z)[D], const double* __restrict__ v, int d)
{
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (c < d) acc = fma(v[c], z[c], acc);
    return acc;
}

// One draw of k-means++ for every init: grid = PCH chunks, one thread per cell.  T trials per init (1 for the first centre,
// then L); with `fold` the centre chosen by the draw before (ids[i][draw - 1]) is taken into closest[i][] first.
// part[(i L + l) npch + chunk] = the chunk's sum of min(closest, distance to candidate l), in the order of hki_wave_scan and
// then wave by wave -- the order in which hki_pp_pick_kernel scans a chunk.
// dynamic LDS: I (L + 1) d + I (L + 1) + 4 I L doubles
template <int D>
__global__ __launch_bounds__(256) void hki_pp_trial_kernel(const double* __restrict__ Xc, const double* __restrict__ xsq,
                                                           HkiDims p, int draw, int T, int fold, const int* __restrict__ ids,
                                                           const int* __restrict__ cand, double* __restrict__ closest,
                                                           double* __restrict__ part)
{
    extern __shared__ double hki_lds[];
    const int d = p.d, L1 = p.L + 1;
    double* vec = hki_lds;                                   // [I][L + 1][d], slot L: the centre chosen last
    double* vsq = vec + (size_t)p.I * L1 * d;                // [I][L + 1]
    double* wt = vsq + p.I * L1;                             // [I][L][4 waves]
    const int tid = threadIdx.x, n = blockIdx.x * PCH + tid;
    const bool valid = n < p.N;
    for (int e = tid; e < p.I * L1 * d; e += 256) {
        const int c = e % d, l = (e / d) % L1, i = e / (d * L1);
        int idx = -1;
        if (l < T) idx = cand[i * p.L + l];
        else if (l == p.L && fold) idx = ids[i * p.K + draw - 1];
        vec[e] = idx >= 0 ? Xc[(size_t)c * p.Np + idx] : 0.0;
    }
    for (int e = tid; e < p.I * L1; e += 256) {
        const int l = e % L1, i = e / L1;
        int idx = -1;
        if (l < T) idx = cand[i * p.L + l];
        else if (l == p.L && fold) idx = ids[i * p.K + draw - 1];
        vsq[e] = idx >= 0 ? xsq[idx] : 0.0;
    }
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = (c < d && valid) ? Xc[(size_t)c * p.Np + n] : 0.0;
    const double xs = valid ? xsq[n] : 0.0;
    __syncthreads();
    for (int i = 0; i < p.I; ++i) {
        const double* base = vec + (size_t)i * L1 * d;
        double cl = valid ? closest[(size_t)i * p.Np + n] : 0.0;
        if (fold) {
            cl = fmin(cl, hki_sqdist(hki_dot<D>(z, base + (size_t)p.L * d, d), vsq[i * L1 + p.L], xs));
            if (valid) closest[(size_t)i * p.Np + n] = cl;
        }
        for (int l = 0; l < T; ++l) {
            double m = fmin(cl, hki_sqdist(hki_dot<D>(z, base + (size_t)l * d, d), vsq[i * L1 + l], xs));
            if (!valid) m = 0.0;
            const double s = hki_wave_scan(m);
            if ((tid & 63) == 63) wt[(i * p.L + l) * 4 + (tid >> 6)] = s;
        }
    }
    __syncthreads();
    for (int e = tid; e < p.I * T; e += 256) {
        const int l = e % T, i = e / T;
        const double* w = wt + (i * p.L + l) * 4;
        part[((size_t)i * p.L + l) * p.npch + blockIdx.x] = __dadd_rn(__dadd_rn(__dadd_rn(w[0], w[1]), w[2]), w[3]);
    }
}

// One workgroup per init, after hki_pp_trial_kernel of the same draw: the T potentials (chunk partials in chunk order),
// the first minimum -> ids[i][draw]; then, unless this was the last draw, the L candidates of the next one:
// searchsorted(cumsum(min(closest, distance to the new centre)), u pot, side = left), clipped to N - 1.  The cumulative sum
// is the chunk totals in chunk order, then inside the chunk the scan whose last value is that chunk's total.
__global__ __launch_bounds__(256) void hki_pp_pick_kernel(const double* __restrict__ Xc, const double* __restrict__ xsq,
                                                          HkiDims p, int draw, int T, const double* __restrict__ u,
                                                          int ustride, const double* __restrict__ part,
                                                          const double* __restrict__ closest, int* __restrict__ ids,
                                                          int* __restrict__ cand)
{
    __shared__ double cpot[8], s_tgt[8], s_pre[8], wt[4];
    __shared__ int s_best, s_ch[8], s_idx[8], s_pos;
    const int i = blockIdx.x, tid = threadIdx.x, d = p.d;
    if (tid < T) {
        const double* pp = part + ((size_t)i * p.L + tid) * p.npch;
        double s = 0.0;
        for (int ch = 0; ch < p.npch; ++ch) s = __dadd_rn(s, pp[ch]);
        cpot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int l = 1; l < T; ++l)
            if (cpot[l] < cpot[b]) b = l;
        s_best = b;
        ids[i * p.K + draw] = cand[i * p.L + b];
    }
    __syncthreads();
    if (draw == p.K - 1) return;
    const int best = s_best;
    const int center = cand[i * p.L + best];
    const double* pb = part + ((size_t)i * p.L + best) * p.npch;
    if (tid < p.L) {
        const double target = __dmul_rn(u[(size_t)i * ustride + 1 + (size_t)draw * p.L + tid], cpot[best]);
        double run = 0.0, pre = 0.0;
        int found = p.npch - 1;
        for (int ch = 0; ch < p.npch; ++ch) {
            const double nr = __dadd_rn(run, pb[ch]);
            pre = run;
            if (nr >= target) { found = ch; break; }
            run = nr;
        }
        s_tgt[tid] = target; s_pre[tid] = pre; s_ch[tid] = found;
    }
    __syncthreads();
    const double csq = xsq[center];
    for (int l = 0; l < p.L; ++l) {
        const int n = s_ch[l] * PCH + tid;
        const bool valid = n < p.N;
        double v = 0.0;
        if (valid) {
            double acc = 0.0;
            for (int c = 0; c < d; ++c) acc = fma(Xc[(size_t)c * p.Np + center], Xc[(size_t)c * p.Np + n], acc);
            v = fmin(closest[(size_t)i * p.Np + n], hki_sqdist(acc, csq, xsq[n]));
        }
        const double s = hki_wave_scan(v);
        if (tid == 0) s_pos = PCH;
        if ((tid & 63) == 63) wt[tid >> 6] = s;
        __syncthreads();
        double incl = s;
        if (tid >= 64) {
            double off = wt[0];
            for (int w = 1; w < (tid >> 6); ++w) off = __dadd_rn(off, wt[w]);
            incl = __dadd_rn(off, s);
        }
        if (valid && __dadd_rn(s_pre[l], incl) >= s_tgt[l]) atomicMin(&s_pos, tid);
        __syncthreads();
        if (tid == 0) s_idx[l] = min(s_ch[l] * PCH + s_pos, p.N - 1);   // (no cell of the chunk reaches the value: the next cell)
        __syncthreads();
    }
    if (tid == 0)
        for (int l = 0; l < p.L; ++l) cand[i * p.L + l] = s_idx[l];
}

// cen[i][k][c] = Xc[c][ids[i][k]]
__global__ __launch_bounds__(256) void hki_gather_kernel(const double* __restrict__ Xc, HkiDims p, const int* __restrict__ ids,
                                                         double* __restrict__ cen)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.I * p.K * p.d) return;
    const int c = e % p.d, ik = e / p.d;
    cen[e] = Xc[(size_t)c * p.Np + ids[ik]];
}

// cen[i][k][c] = centers0[i][k][c] - mean[c]
__global__ __launch_bounds__(256) void hki_given_kernel(const double* __restrict__ c0, const double* __restrict__ mean,
                                                        HkiDims p, double* __restrict__ cen)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.I * p.K * p.d) return;
    cen[e] = __dsub_rn(c0[e], mean[e % p.d]);
}

// The E step: grid (PCH chunks, n_init), one thread per cell, the K centres of the init and their squared norms in LDS.
// final == 0: an iteration of the loop (an init that is done returns); a changed label raises st[i].changed.
// final == 1: the inits that did not stop strictly take their labels once more; then ipart[i][chunk] = the chunk's sum of
// |x - c_label|^2 for every init (a fixed tree over the 256 threads).
// dynamic LDS: K d + K + 256 doubles
template <int D>
__global__ __launch_bounds__(256) void hki_assign_kernel(const double* __restrict__ Xc, HkiDims p, const double* __restrict__ cen,
                                                         int* __restrict__ labels, HkiInit* __restrict__ st, int final,
                                                         double* __restrict__ ipart)
{
    extern __shared__ double hki_lds[];
    const int i = blockIdx.y, d = p.d, K = p.K, tid = threadIdx.x;
    const bool assign = final ? !st[i].strict : !st[i].done;
    if (!final && !assign) return;
    double* cs = hki_lds;                 // [K][d]
    double* csq = cs + (size_t)K * d;     // [K]
    double* red = csq + K;                // [256]
    for (int e = tid; e < K * d; e += 256) cs[e] = cen[(size_t)i * K * d + e];
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int c = 0; c < d; ++c) s = fma(cs[k * d + c], cs[k * d + c], s);
        csq[k] = s;
    }
    __syncthreads();
    const int n = blockIdx.x * PCH + tid;
    const bool valid = n < p.N;
    double z[D];
#pragma unroll
    for (int c = 0; c < D; ++c) z[c] = (c < d && valid) ? Xc[(size_t)c * p.Np + n] : 0.0;
    int lab = valid ? labels[(size_t)i * p.Np + n] : 0;
    if (assign) {
        const int old = lab;
        double bv = INFINITY;
        lab = 0;
        for (int k = 0; k < K; ++k) {
            const double v = __dsub_rn(csq[k], __dmul_rn(2.0, hki_dot<D>(z, cs + (size_t)k * d, d)));
            if (v < bv) { bv = v; lab = k; }
        }
        if (valid) labels[(size_t)i * p.Np + n] = lab;
        if (!final) {
            if (__syncthreads_or(valid && lab != old) && tid == 0) atomicOr(&st[i].changed, 1);
            return;
        }
    }
    double r2 = 0.0;
    if (valid) {
        const double* c = cs + (size_t)lab * d;
#pragma unroll
        for (int j = 0; j < D; ++j)
            if (j < d) { const double df = __dsub_rn(z[j], c[j]); r2 = fma(df, df, r2); }
    }
    red[tid] = r2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __dadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) ipart[(size_t)i * p.npch + blockIdx.x] = red[0];
}

// psum[i][chunk][k][c], pcnt[i][chunk][k]: the sums and counts of the cells of one chunk (lch cells) by label, every cluster
// in ascending cell order: wave q of the four takes the clusters with k mod 4 = q, lane c the component c.
// grid (chunks, n_init); dynamic LDS: K d doubles + K ints
__global__ __launch_bounds__(256) void hki_accum_kernel(const double* __restrict__ Xc, HkiDims p, int lch, int nlch,
                                                        const int* __restrict__ labels, const HkiInit* __restrict__ st,
                                                        double* __restrict__ psum, int* __restrict__ pcnt)
{
    extern __shared__ double hki_lds[];
    __shared__ double Zs[64][33];
    __shared__ int ls[32];
    const int i = blockIdx.y, chunk = blockIdx.x, d = p.d, K = p.K, tid = threadIdx.x;
    if (st[i].done) return;
    double* sums = hki_lds;                       // [K][d]
    int* cnt = (int*)(sums + (size_t)K * d);      // [K]
    for (int e = tid; e < K * d; e += 256) sums[e] = 0.0;
    for (int k = tid; k < K; k += 256) cnt[k] = 0;
    const int c = tid & 63, q = tid >> 6;
    const int n0 = chunk * lch, n1 = min(p.N, n0 + lch);
    for (int s = n0; s < n1; s += 32) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = tid + 256 * r, cc = e >> 5, j = e & 31;
            Zs[cc][j] = (cc < d && s + j < n1) ? Xc[(size_t)cc * p.Np + s + j] : 0.0;
        }
        if (tid < 32) ls[tid] = s + tid < n1 ? labels[(size_t)i * p.Np + s + tid] : -1;
        __syncthreads();
        for (int j = 0; j < 32; ++j) {
            const int k = ls[j];
            if (k < 0 || (k & 3) != q) continue;          // uniform over the wave
            if (c < d) sums[k * d + c] = __dadd_rn(sums[k * d + c], Zs[c][j]);
            if (c == 0) cnt[k] += 1;
        }
    }
    __syncthreads();
    const size_t o = (size_t)i * nlch + chunk;
    for (int e = tid; e < K * d; e += 256) psum[o * K * d + e] = sums[e];
    for (int k = tid; k < K; k += 256) pcnt[o * K + k] = cnt[k];
}

// sums[i][k][c], counts[i][k]: the chunk partials added in chunk order.  grid (K, n_init)
__global__ __launch_bounds__(64) void hki_reduce_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt, HkiDims p,
                                                        int nlch, const HkiInit* __restrict__ st, double* __restrict__ sums,
                                                        int* __restrict__ counts)
{
    const int k = blockIdx.x, i = blockIdx.y, c = threadIdx.x, d = p.d, K = p.K;
    if (st[i].done) return;
    if (c < d) {
        double s = 0.0;
        for (int ch = 0; ch < nlch; ++ch) s = __dadd_rn(s, psum[(((size_t)i * nlch + ch) * K + k) * d + c]);
        sums[((size_t)i * K + k) * d + c] = s;
    }
    if (c == 0) {
        int m = 0;
        for (int ch = 0; ch < nlch; ++ch) m += pcnt[((size_t)i * nlch + ch) * K + k];
        counts[i * K + k] = m;
    }
}

// The rest of a Lloyd iteration, one workgroup per init (scikit-learn's _relocate_empty_clusters, _average_centers and the
// stopping rule, as oracle/consensus.py's lloyd_iter and kmeans_single restate them):
//  - empty clusters, in ascending id, take the cells farthest from their own (old) centre, in descending distance, the
//    first of equals; no cluster moves when the largest distance is 0;
//  - centre = sum * (1 / count); a cluster still empty copies the row of the heaviest cluster (the first of equals) as
//    the loop over ascending ids finds it: not yet divided for the ids below the heaviest, divided above it;
//  - shift2 = sum over the clusters of sqrt(|new - old|^2)^2; no label changed: done, strictly; else shift2 <= tol_ or the
//    last iteration: done, and hki_assign_kernel takes the labels once more.
__global__ __launch_bounds__(256) void hki_finish_kernel(const double* __restrict__ Xc, HkiDims p, double* __restrict__ cen,
                                                         double* __restrict__ sums, const int* __restrict__ counts,
                                                         const int* __restrict__ labels, double* __restrict__ dist,
                                                         HkiInit* __restrict__ st, const double* __restrict__ tol, int it,
                                                         int max_iter)
{
    __shared__ int cn[CNMF_HARMONY_KMAX];
    __shared__ double sh2[CNMF_HARMONY_KMAX];
    __shared__ double bv[256];
    __shared__ int bi[256];
    __shared__ int s_empty, s_amax;
    const int i = blockIdx.x, tid = threadIdx.x, d = p.d, K = p.K, N = p.N;
    if (st[i].done) return;
    double* ce = cen + (size_t)i * K * d;
    double* sm = sums + (size_t)i * K * d;
    const int* lab = labels + (size_t)i * p.Np;
    double* di = dist + (size_t)i * p.Np;
    for (int k = tid; k < K; k += 256) cn[k] = counts[i * K + k];
    __syncthreads();
    if (tid == 0) {
        int e = 0;
        for (int k = 0; k < K; ++k) e += cn[k] == 0;
        s_empty = e;
    }
    __syncthreads();
    if (s_empty > 0) {                                          // uniform
        for (int n = tid; n < N; n += 256) {
            const double* c = ce + (size_t)lab[n] * d;
            double s = 0.0;
            for (int j = 0; j < d; ++j) { const double df = __dsub_rn(Xc[(size_t)j * p.Np + n], c[j]); s = fma(df, df, s); }
            di[n] = s;
        }
        __syncthreads();
        bool first = true;
        for (int e = 0; e < K; ++e) {
            if (cn[e] != 0) continue;                           // uniform
            double v = -1.0; int idx = -1;
            for (int n = tid; n < N; n += 256)
                if (di[n] > v) { v = di[n]; idx = n; }
            bv[tid] = v; bi[tid] = idx;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if (tid < o && bi[tid + o] >= 0 &&
                    (bv[tid + o] > bv[tid] || (bv[tid + o] == bv[tid] && (bi[tid] < 0 || bi[tid + o] < bi[tid])))) {
                    bv[tid] = bv[tid + o]; bi[tid] = bi[tid + o];
                }
                __syncthreads();
            }
            const int far = bi[0];
            const double fv = bv[0];
            __syncthreads();
            if (far < 0 || (first && fv <= 0.0)) break;         // every cell sits on its centre
            first = false;
            const int old = lab[far];
            for (int j = tid; j < d; j += 256) {
                const double x = Xc[(size_t)j * p.Np + far];
                sm[(size_t)old * d + j] = __dsub_rn(sm[(size_t)old * d + j], x);
                sm[(size_t)e * d + j] = x;
            }
            if (tid == 0) { cn[e] = 1; cn[old] -= 1; di[far] = -1.0; }
            __syncthreads();
        }
    }
    if (tid == 0) {
        int a = 0;
        for (int k = 1; k < K; ++k)
            if (cn[k] > cn[a]) a = k;
        s_amax = a;
    }
    __syncthreads();
    const int amax = s_amax;
    for (int k = tid; k < K; k += 256) {
        const int src = cn[k] > 0 ? k : amax;
        const double alpha = cn[k] > 0 ? 1.0 / (double)cn[k] : (k < amax ? 1.0 : 1.0 / (double)cn[amax]);
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
            const double v = __dmul_rn(sm[(size_t)src * d + j], alpha);
            const double df = __dsub_rn(v, ce[(size_t)k * d + j]);
            s = fma(df, df, s);
            ce[(size_t)k * d + j] = v;
        }
        const double sh = __dsqrt_rn(s);
        sh2[k] = __dmul_rn(sh, sh);
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int k = 0; k < K; ++k) tot = __dadd_rn(tot, sh2[k]);
        st[i].iters = it + 1;
        if (st[i].changed == 0) { st[i].strict = 1; st[i].done = 1; }
        else if (tot <= *tol || it + 1 >= max_iter) st[i].done = 1;
        st[i].changed = 0;
    }
}

}  // namespace cnmf

// Scratch, freed when the call returns (doubles unless noted; I = n_init, L = 2 + int(ln K), Np = N rounded up to 64,
// c512 = ceil(N / 512), c256 = ceil(N / 256), cl = ceil(N / hki_lloyd_chunk(N)) <= 256):
//   (d + 1 + 2 I) Np + I Np int32              Xc, x_sq, closest and the relocation distances, labels
//   c512 d + I L c256 + I c256                 column-moment, potential and inertia partials
//   I cl K (d doubles + 1 int32)               cluster sums and counts per chunk
//   2 I K d + small                            centres, sums, counts, ids, candidates, uniforms, the per-init state
extern "C" int cnmf_harmony_kmeans_init(cnmf_ctx* ctx, int32_t n_init, int32_t max_iter, double tol, const double* uniforms,
                                        const double* centers0, double* Y, int32_t* labels, double* inertia, int32_t* n_iter,
                                        int32_t* best)
{
    using namespace cnmf;
    if (int rc = har_need(ctx, false)) return rc;
    if (!Y || !inertia || !n_iter || !best || (!uniforms && !centers0)) { SET_ERR(ctx, "null argument"); return CNMF_EINVAL; }
    HarStage& H = ctx->har;
    const int N = H.N, Np = H.Np, d = H.d, K = H.K, I = n_init;
    if (I < 1 || I > 16 || max_iter < 1 || K > N) {
        SET_ERR(ctx, "n_init = %d outside [1, 16], max_iter = %d below 1 or K = %d above %d cells", I, max_iter, K, N);
        return CNMF_EINVAL;
    }
    const int L = 2 + (int)std::log((double)K);
    if (L > 8) { SET_ERR(ctx, "too many local trials"); return CNMF_EUNSUPPORTED; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int c512 = (N + HCH - 1) / HCH, npch = (N + PCH - 1) / PCH;
    const int lch = hki_lloyd_chunk(N), nlch = (N + lch - 1) / lch;
    const HkiDims p{N, Np, d, K, I, L, npch};
    const size_t ikd = (size_t)I * K * d, ustride = 1 + (size_t)(K - 1) * L;
    DevPool pool;
    double* dXc = pool.get<double>((size_t)d * Np, true, st);
    double* dxsq = pool.get<double>(Np, true, st);
    double* dclosest = pool.get<double>((size_t)I * Np);
    double* ddist = pool.get<double>((size_t)I * Np);
    int* dlabels = pool.get<int>((size_t)I * Np);
    double* dcpart = pool.get<double>((size_t)c512 * d);
    double* dpart = pool.get<double>((size_t)I * L * npch);
    double* dipart = pool.get<double>((size_t)I * npch);
    double* dpsum = pool.get<double>((size_t)I * nlch * K * d);
    int* dpcnt = pool.get<int>((size_t)I * nlch * K);
    double* dcen = pool.get<double>(ikd);
    double* dsums = pool.get<double>(ikd);
    int* dcounts = pool.get<int>((size_t)I * K);
    int* dids = pool.get<int>((size_t)I * K);
    int* dcand = pool.get<int>((size_t)I * L);
    double* dmean = pool.get<double>(d);
    double* dtol = pool.get<double>(1);
    double* du = pool.get<double>(centers0 ? ikd : (size_t)I * ustride);     // the uniforms, or the given centres
    HkiInit* dst = pool.get<HkiInit>(I, true, st);
    POOL_TRY(ctx, pool);

    // ---- centring, x_sq and tol_ (sklearn _kmeans.py:1477-1484, 279-288)
    hki_colsum_kernel<<<c512, 64, 0, st>>>(H.Zcos, N, Np, d, 0, dcpart);
    hki_mean_kernel<<<1, 64, 0, st>>>(dcpart, c512, d, N, dmean);
    hki_center_kernel<<<har_cells_grid(N), 256, 0, st>>>(H.Zcos, dmean, N, Np, d, dXc, dxsq);
    hki_colsum_kernel<<<c512, 64, 0, st>>>(dXc, N, Np, d, 1, dcpart);
    hki_tol_kernel<<<1, 64, 0, st>>>(dcpart, c512, d, N, tol, dtol);
    HIP_TRY(ctx, hipGetLastError());

    const unsigned egrid = (unsigned)((ikd + 255) / 256);
    std::vector<int> c0((size_t)I * L, 0);                   // the first centre of every init, as the candidate of draw 0
    if (centers0) {
        HIP_TRY(ctx, hipMemcpyAsync(du, centers0, ikd * sizeof(double), hipMemcpyHostToDevice, st));
        hki_given_kernel<<<egrid, 256, 0, st>>>(du, dmean, p, dcen);
    } else {
        // ---- k-means++ (sklearn _kmeans.py:174-272): two launches per draw for all inits together
        for (int i = 0; i < I; ++i) c0[(size_t)i * L] = std::min(first_center_index(N, uniforms[(size_t)i * ustride]), N - 1);
        HIP_TRY(ctx, hipMemcpyAsync(dcand, c0.data(), c0.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(du, uniforms, (size_t)I * ustride * sizeof(double), hipMemcpyHostToDevice, st));
        hki_fill_kernel<<<(unsigned)(((size_t)I * Np + 255) / 256), 256, 0, st>>>(dclosest, (size_t)I * Np, INFINITY);
        const size_t lds = ((size_t)I * (L + 1) * (d + 1) + (size_t)4 * I * L) * sizeof(double);
        for (int draw = 0; draw < K; ++draw) {
            const int T = draw == 0 ? 1 : L, fold = draw > 0;
            if (d <= 16) hki_pp_trial_kernel<16><<<npch, 256, lds, st>>>(dXc, dxsq, p, draw, T, fold, dids, dcand, dclosest, dpart);
            else if (d <= 32) hki_pp_trial_kernel<32><<<npch, 256, lds, st>>>(dXc, dxsq, p, draw, T, fold, dids, dcand, dclosest, dpart);
            else hki_pp_trial_kernel<64><<<npch, 256, lds, st>>>(dXc, dxsq, p, draw, T, fold, dids, dcand, dclosest, dpart);
            hki_pp_pick_kernel<<<I, 256, 0, st>>>(dXc, dxsq, p, draw, T, du, (int)ustride, dpart, dclosest, dids, dcand);
        }
        hki_gather_kernel<<<egrid, 256, 0, st>>>(dXc, p, dids, dcen);
    }
    HIP_TRY(ctx, hipGetLastError());

    // ---- Lloyd for all inits in lock step (sklearn _kmeans.py:624-752); the stopping rule is applied on the device, so
    // the host looks at the state once per LLOYD_BATCH iterations
    const size_t alds = ((size_t)K * d + K + 256) * sizeof(double), mlds = (size_t)K * d * sizeof(double) + (size_t)K * sizeof(int);
    // (the most either kernel asks for, at K = CNMF_HARMONY_KMAX and d = CNMF_HARMONY_DMAX: just above the 64 KB a kernel gets unasked)
    constexpr int kd_max = CNMF_HARMONY_KMAX * CNMF_HARMONY_DMAX;
    constexpr int alds_max = (kd_max + CNMF_HARMONY_KMAX + 256) * 8, mlds_max = kd_max * 8 + CNMF_HARMONY_KMAX * 4;
    auto assign = [&](int final) -> hipError_t {
        const dim3 grid(npch, I);
#define HKI_ASSIGN(D)                                                                                              \
        do {                                                                                                       \
            hipError_t e_ = dyn_lds_optin((const void*)hki_assign_kernel<D>, alds_max);                       \
            if (e_ != hipSuccess) return e_;                                                                       \
            hki_assign_kernel<D><<<grid, 256, alds, st>>>(dXc, p, dcen, dlabels, dst, final, dipart);               \
        } while (0)
        if (d <= 16) HKI_ASSIGN(16); else if (d <= 32) HKI_ASSIGN(32); else HKI_ASSIGN(64);
#undef HKI_ASSIGN
        return hipSuccess;
    };
    HIP_TRY(ctx, dyn_lds_optin((const void*)hki_accum_kernel, mlds_max));
    HIP_TRY(ctx, hipMemsetAsync(dlabels, 0xff, (size_t)I * Np * sizeof(int), st));          // labels = -1
    std::vector<HkiInit> hst(I);
    constexpr int LLOYD_BATCH = 3;
    for (int it = 0; it < max_iter; ) {
        const int nb = std::min(LLOYD_BATCH, max_iter - it);
        for (int b = 0; b < nb; ++b, ++it) {
            HIP_TRY(ctx, assign(0));
            hki_accum_kernel<<<dim3(nlch, I), 256, mlds, st>>>(dXc, p, lch, nlch, dlabels, dst, dpsum, dpcnt);
            hki_reduce_kernel<<<dim3(K, I), 64, 0, st>>>(dpsum, dpcnt, p, nlch, dst, dsums, dcounts);
            hki_finish_kernel<<<I, 256, 0, st>>>(dXc, p, dcen, dsums, dcounts, dlabels, ddist, dst, dtol, it, max_iter);
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(hst.data(), dst, sizeof(HkiInit) * I, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        bool all_done = true;
        for (int i = 0; i < I; ++i) all_done &= hst[i].done != 0;
        if (all_done) break;
    }
    HIP_TRY(ctx, assign(1));
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> ipart((size_t)I * npch);
    HIP_TRY(ctx, hipMemcpyAsync(ipart.data(), dipart, ipart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < I; ++i) {
        double s = 0.0;
        for (int ch = 0; ch < npch; ++ch) s += ipart[(size_t)i * npch + ch];
        inertia[i] = s;
        n_iter[i] = hst[i].iters;
    }
    // best of n_init in init order (sklearn _kmeans.py:1525-1533); an init's labels are fetched only when its inertia is lower
    std::vector<int> best_labels, lab(N);
    int bi = -1;
    for (int i = 0; i < I; ++i) {
        if (bi >= 0 && !(inertia[i] < inertia[bi])) continue;
        HIP_TRY(ctx, hipMemcpy(lab.data(), dlabels + (size_t)i * Np, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
        if (bi < 0 || !same_clustering(lab, best_labels, K)) { best_labels = lab; bi = i; }
    }
    std::vector<double> cen((size_t)K * d), mean(d);
    HIP_TRY(ctx, hipMemcpy(cen.data(), dcen + (size_t)bi * K * d, cen.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(mean.data(), dmean, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < d; ++c) Y[(size_t)c * K + k] = cen[(size_t)k * d + c] + mean[c];
    if (labels) std::copy(best_labels.begin(), best_labels.end(), labels);
    *best = bi;
    return CNMF_OK;
}
