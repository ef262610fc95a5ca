// Host driver of the multiplicative-update solver (included by cnmf_hip.hip): cnmf_nmf_mu_batch, the reference's path
// for beta_loss != 'frobenius' (cnmf.py:618-631).  Restates _fit_multiplicative_update (sklearn/decomposition/_nmf.py:
// 731-893): W then H half-steps, the beta-divergence every 10 iterations, stop when (previous - error) / error_at_init < tol.
// mu_sched.h (standard library only) decides which restart sits in which slot, when the divergence is due, who stops and
// who is refilled; this file makes the HIP calls that go with each decision.  The restarts of a call are grouped by padded
// rank 16 / 32 / 64 (and 128 where the context's rank limit was raised) and run up to MU_MAXSLOTS at a time: one round of launches advances every live slot by one iteration.
// Three kernel families behind ONE driver (mu_drive) and one slot path (install_slots, retire_slot, reduce_divergence):
// MuMfma dense (Kullback-Leibler and Itakura-Saito on the matrix pipe, reading X and X^T), MuMfma sparse (Kullback-Leibler
// at padded ranks 16 / 32 / 64 on the non-zeros, chosen by mu_sparse_prepare) and MuValu (the vector-ALU kernels: the same
// driver with one slot, for CNMF_MU_VALU=1 and matrices beyond 2^24 cells or genes).
#pragma once
#include "kernels_mu.hip.h"
#include "kernels_mu_mfma.hip.h"
#include "kernels_mu_sparse.hip.h"
#include "mu_sched.h"

namespace cnmf {

static_assert(MU_SCHED_MAXSLOTS == MU_MAXSLOTS, "mu_sched.h repeats MU_MAXSLOTS");

// ---- X^T as a dense image, for the W half-step and the divergence of the matrix-pipe kernels
static int mu_ensure_xt(cnmf_ctx* ctx, int Gs)
{
    if (ctx->XtF.p) return CNMF_OK;
    if (Gs / 32 > 65535) { SET_ERR(ctx, "X^T build: %d gene rows exceed the launch grid", Gs); return CNMF_EUNSUPPORTED; }
    OwnedLocal<DenseTF> xt;
    HIP_TRY(ctx, hipMalloc((void**)&xt.p, (size_t)Gs * ctx->N_pad * sizeof(float)));
    dim3 grid(ctx->N_pad / 32, Gs / 32), block(32, 8);        // cells on grid.x: no 65 535-block limit on N_pad
    mu_transpose_kernel<<<grid, block, 0, ctx->stream>>>(ctx->X, ctx->G_pad, (int)ctx->N, (int)ctx->G, xt.p, ctx->N_pad, Gs);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));           // built once per matrix: check it really ran
    ctx->XtF.take(xt);
    return CNMF_OK;
}

// ---- Kullback-Leibler on the non-zeros: the blocked sliced-ELL images (kernels_mu_sparse.hip.h) of a matrix of R rows x C
// columns given as compressed rows (csr_host.hip.h: the CSR upload as it came, or X^T's rows built on the device; the
// N x G dense image and its transposed copy are not touched on this path).
// The host half: rows by decreasing non-zero count (ties in row order), so the rows of a slice are about equally long;
// per (slice, block) the padded length and the first entry.  Returns the number of entries.
static long long sp_layout(const std::vector<int>& cnt, int R, int nblk, int nslice, std::vector<int>& perm,
                           std::vector<int>& len, std::vector<long long>& off)
{
    std::vector<long long> tot(R, 0);
    for (int r = 0; r < R; ++r) for (int b = 0; b < nblk; ++b) tot[r] += cnt[(size_t)r * nblk + b];
    perm.assign((size_t)nslice * 64, -1);
    for (int r = 0; r < R; ++r) perm[r] = r;
    std::stable_sort(perm.begin(), perm.begin() + R, [&](int a, int b) { return tot[a] > tot[b]; });
    len.resize((size_t)nslice * nblk); off.resize((size_t)nslice * nblk);
    long long n_ent = 0;
    for (int s = 0; s < nslice; ++s)
        for (int b = 0; b < nblk; ++b) {
            int mx = 0;
            for (int l = 0; l < 64; ++l) { const int r = perm[(size_t)s * 64 + l]; if (r >= 0) mx = std::max(mx, cnt[(size_t)r * nblk + b]); }
            mx = round_up(mx, SP_UNROLL);
            len[(size_t)s * nblk + b] = mx; off[(size_t)s * nblk + b] = n_ent;
            n_ent += (long long)mx * 64;
        }
    return n_ent;
}

// `out` becomes the image, or stays as it was (CNMF_ENOMEM: the caller may fall back to the dense kernels)
static int sp_build_image(cnmf_ctx* ctx, const long long* ptr, const int* idx, const float* val, int R, int C, int BS, SpImage& out)
{
    hipStream_t st = ctx->stream;
    OwnedLocal<SpImageF> im;
    const int nblk = (C + BS - 1) / BS, nslice = (R + 63) / 64, npos = nslice * 64;
    DevPool pool;
    int* dcnt = pool.get<int>((size_t)R * nblk, true, st);
    int* dpre = pool.get<int>((size_t)R * nblk);
    POOL_TRY(ctx, pool);
    sp_count_csr_kernel<<<(R + 3) / 4, 256, 0, st>>>(ptr, idx, R, BS, nblk, dcnt);
    sp_prefix_kernel<<<(R + 255) / 256, 256, 0, st>>>(dcnt, R, nblk, dpre);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int> cnt((size_t)R * nblk), perm, len;
    std::vector<long long> off;
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), dcnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const long long n_ent = sp_layout(cnt, R, nblk, nslice, perm, len, off);
    const size_t ent_bytes = (size_t)std::max<long long>(n_ent, 64) * sizeof(uint2);
    HIP_TRY(ctx, hipMalloc((void**)&im.perm, perm.size() * sizeof(int)));
    HIP_TRY(ctx, hipMalloc((void**)&im.off, off.size() * sizeof(long long)));
    HIP_TRY(ctx, hipMalloc((void**)&im.len, len.size() * sizeof(int)));
    HIP_TRY(ctx, hipMalloc(&im.ent, ent_bytes));
    HIP_TRY(ctx, hipMemsetAsync(im.ent, 0, ent_bytes, st));
    HIP_TRY(ctx, hipMemcpyAsync(im.perm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(im.off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(im.len, len.data(), len.size() * sizeof(int), hipMemcpyHostToDevice, st));
    sp_fill_csr_kernel<<<(npos + 3) / 4, 256, 0, st>>>(ptr, idx, val, BS, nblk, npos, im.perm, im.off, dpre, (uint2*)im.ent, SP_LDS_BYTES / 4 / BS);
    HIP_TRY(ctx, hipGetLastError());
    // a conflict-free order of every row's entries (CNMF_SP_ORDER=0: storage order, the A/B reference)
    if (ctx->mu_knobs.sp_order && n_ent > 0 && BS / 16 <= 255) {                  // (its per-residue counters are bytes)
        uint2* tmp = pool.get<uint2>((size_t)n_ent);
        POOL_TRY(ctx, pool);
        const long long jobs = (long long)nslice * nblk * 4;
        sp_reorder_kernel<<<(unsigned)((jobs + 63) / 64), 64, 0, st>>>(nslice, nblk, C, BS, SP_LDS_BYTES / 4 / BS, im.off, im.len,
                                                                      (uint2*)im.ent, tmp);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));                            // the host vectors above are stack objects
    im.R = R; im.C = C; im.BS = BS; im.nblk = nblk; im.nslice = nslice; im.n_ent = (size_t)n_ent;
    out.take(im);
    return CNMF_OK;
}

// Does this call take the non-zero path?  CNMF_MU_SPARSE=0 never, =1 always, otherwise when at most a quarter of X (at
// padded rank 64: 15 %) is non-zero (the dense matrix-pipe kernels cost ~0.9 ns per ELEMENT and restart-iteration at k <= 16, these ~3 ns per NON-ZERO)
// and its images and partial numerators fit the free device memory (else: the dense kernels).
static int mu_sparse_prepare(cnmf_ctx* ctx, int KP, bool* use)
{
    *use = false;
    const int mode = ctx->mu_knobs.sparse;
    // padded rank 64 (ranks 33..64, two lanes per row) only under cnmf_set_mu_sparse_rank_limit(ctx, CNMF_MU_SPARSE_KMAX_WIDE)
    if (mode == 0 || (KP != 16 && KP != 32 && !(KP == 64 && ctx->mu_sparse_rank_limit >= CNMF_MU_SPARSE_KMAX_WIDE))) return CNMF_OK;
    const int N = (int)ctx->N, G = (int)ctx->G, idx = cnmf_ctx::sp_image_index(KP), BS = SP_LDS_BYTES / (KP * 4);
    // how many entries are stored?  From the compressed rows when the matrix came as CSR; a dense upload is only COUNTED here
    // (N + 1 counters) -- its compressed rows (12 B per entry) are built below, once the density and memory rules have chosen
    // this path, and not at all when they send the call back to the dense kernels
    int rc = CNMF_OK;
    if (ctx->csr.ptr) ctx->x_nnz = ctx->csr.nnz;
    else if (ctx->x_nnz < 0) {
        long long* cnt = nullptr;
        HIP_TRY(ctx, hipMalloc((void**)&cnt, ((size_t)N + 1) * sizeof(long long)));
        csr_count_dense_kernel<<<(N + 3) / 4, 256, 0, ctx->stream>>>(ctx->X, ctx->G_pad, N, G, cnt);
        long long nnz = 0;
        rc = hipGetLastError() == hipSuccess ? csr_scan_to_ptr(ctx, cnt, (size_t)N, &nnz) : CNMF_EHIP;
        hipFree(cnt);
        if (rc) return rc;
        ctx->x_nnz = nnz;
    }
    // (padded rank 64: measured at 50 000 x 2 000, the two routes meet at 23 / 19 / 16 % non-zero at k = 40 / 48 / 64 --
    // profiles/mu_sparse_ranks_33_64_50000x2000.json, between its 9 % and 34 % rows -- so that group switches at 15 %)
    const double max_density = KP == 64 ? 0.15 : 0.25;
    if (mode != 1 && (double)ctx->x_nnz > max_density * (double)N * (double)G) return CNMF_OK;
    if (!ctx->spA[idx].ent || !ctx->spB[idx].ent) {
        // the partial numerators of a half-step whose other side needs several blocks ([blocks][own rows][KP] per slot), the
        // two images (8 B per entry, padded: x 1.25 allowed for), X^T's compressed rows and the build's scratch
        const double nbA = std::ceil((double)G / BS), nbB = std::ceil((double)N / BS);
        const double part = 4.0 * KP * MU_MAXSLOTS * std::max(nbA > 1 ? nbA * ctx->N_pad : 0.0, nbB > 1 ? nbB * round_up(ctx->G_pad, 128) : 0.0);
        const double need = part + 2.0 * 1.25 * 8.0 * (double)ctx->x_nnz * 2.0 + 8.0 * (double)ctx->x_nnz + 8.0 * ((double)N * nbA + (double)G * nbB);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        if (mode != 1 && (part > 64e9 || need > 0.9 * (double)free_b)) {
            if (ctx->mu_knobs.debug) fprintf(stderr, "[cnmf] KL on the non-zeros: %.1f GB needed, %.1f GB free -> dense kernels\n", need / 1e9, free_b / 1e9);
            return CNMF_OK;
        }
    }
    rc = ensure_csr(ctx);                                       // (kept from the CSR upload, or two passes over the dense image)
    if (rc == CNMF_ENOMEM && mode != 1) return CNMF_OK;
    if (rc) return rc;
    if (!ctx->spA[idx].ent) rc = sp_build_image(ctx, ctx->csr.ptr, ctx->csr.idx, ctx->csr.val, N, G, BS, ctx->spA[idx]);
    if (!rc && !ctx->spB[idx].ent) {
        rc = ensure_csc(ctx);
        if (!rc) rc = sp_build_image(ctx, ctx->csc.ptr, ctx->csc.idx, ctx->csc.val, G, N, BS, ctx->spB[idx]);
    }
    if (rc == CNMF_ENOMEM) (void)hipGetLastError();             // (not to be found by the next launch check)
    if (rc == CNMF_ENOMEM && mode != 1) {                       // an allocation failed after all: the dense kernels still work
        ctx->spA[idx].release(); ctx->spB[idx].release();
        return CNMF_OK;
    }
    if (rc) return rc;
    if (ctx->mu_knobs.debug)
        fprintf(stderr, "[cnmf] KL on the non-zeros: %lld of %lld elements (%.1f %%), padded entries A %.3f x, B %.3f x\n",
                ctx->x_nnz, (long long)N * G, 100.0 * ctx->x_nnz / ((double)N * G),
                ctx->spA[idx].n_ent / std::max(1.0, (double)ctx->x_nnz), ctx->spB[idx].n_ent / std::max(1.0, (double)ctx->x_nnz));
    *use = true;
    return CNMF_OK;
}

// ---- the driver
struct MuJob { int restart; int k; size_t hoff, woff; };               // offsets into the caller's H / W arrays
struct MuCall {                                                         // the arguments of cnmf_nmf_mu_batch
    int init_mode, beta, update_H;
    const uint32_t* seeds; const double* avg; const float *W0, *H0; const cnmf_cd_params* prm;
    float *H_out, *W_out; int32_t* n_iter_out; double* err_out;
};
// What one run of the driver works on: one group of jobs of one padded rank in R slots.
struct MuRun {
    cnmf_ctx* ctx; hipStream_t st;
    const MuCall* c;
    const std::vector<MuJob>* jobs;
    int N, G, ldx, Np, Gs;                 // shape; floats per row of X and of X^T; gene rows of X^T and of a slot's Ht
    int KP, R, kmax;                       // padded rank, slots, largest rank among the jobs
    float l1W, l2W, l1H, l2H;
    DevPool pool;                          // everything below
    std::vector<MuSlotDev> slot;
    float *cmH = nullptr, *cmW = nullptr;  // component-major staging of the initial / final factors, one kmax-row band per slot
    RngJob* dj = nullptr;
    int ndiv = 0;                          // divergence partials per slot
    std::vector<double> hdiv;              // host: [R][ndiv]
    std::vector<float> hsums;              // host: [R][2][KP] column sums of H and W

    MuRun(cnmf_ctx* ctx_, const MuCall& c_, const std::vector<MuJob>& jobs_, int KP_, int R_)
        : ctx(ctx_), st(ctx_->stream), c(&c_), jobs(&jobs_), N((int)ctx_->N), G((int)ctx_->G), ldx(ctx_->G_pad), Np(ctx_->N_pad),
          Gs(round_up(ctx_->G_pad, 128)), KP(KP_), R(R_), kmax(1), l1W((float)c_.prm->l1_reg_W), l2W((float)c_.prm->l2_reg_W),
          l1H((float)c_.prm->l1_reg_H), l2H((float)c_.prm->l2_reg_H), slot(R_)
    {
        for (const MuJob& j : jobs_) kmax = std::max(kmax, j.k);
    }
    MuRun(const MuRun&) = delete;
    int alloc_staging(int ndiv_) {
        cmH = pool.get<float>((size_t)R * kmax * G);
        cmW = pool.get<float>((size_t)R * kmax * N);
        dj = pool.get<RngJob>(R);
        if (pool.err) { SET_ERR(ctx, "device allocation failed"); return CNMF_ENOMEM; }
        ndiv = ndiv_;
        hdiv.resize((size_t)R * ndiv); hsums.resize((size_t)R * 2 * KP);
        return CNMF_OK;
    }
};

// -- the matrix-pipe kernels (dense: X and X^T; sparse: the non-zero images), up to MU_MAXSLOTS slots per launch
template <int KP_, bool BETA1_>
struct MuMfma {
    static constexpr int KP = KP_, RPW = MuShape<KP_>::RPW, coop_lds = 2 * MuLds<KP_>::BUF;      // RPW: restarts per workgroup
    static constexpr bool BETA1 = BETA1_, batched = true;
    bool sparse = false;
    BSellDev dA{}, dB{};
    int grpA = 0, grpB = 0, tilesA = 0, spwB = 1;
    int nchunks = 0, tpc = 0;
};
static BSellDev sp_dev(const SpImage& a) { return BSellDev{a.R, a.C, a.BS, a.nblk, a.nslice, a.perm, a.off, a.len, (const uint2*)a.ent}; }

template <int KP, bool BETA1>
static int mu_setup(MuRun& r, MuMfma<KP, BETA1>& p, bool sparse)
{
    cnmf_ctx* ctx = r.ctx;
    p.sparse = sparse;
    if (sparse) {                          // same slots, same schedule, other kernels
        p.dA = sp_dev(ctx->spA[cnmf_ctx::sp_image_index(KP)]); p.dB = sp_dev(ctx->spB[cnmf_ctx::sp_image_index(KP)]);
        // cells: one slice per wave (sorted rows: the slices of a workgroup are equally long); genes: all slices of up to
        // 8192 genes in ONE workgroup per block of cells, long and short slices paired on the waves
        p.spwB = std::max(1, std::min(8, (p.dB.nslice + SP_WAVES - 1) / SP_WAVES));
        p.grpA = (p.dA.nslice + SP_WAVES - 1) / SP_WAVES; p.grpB = (p.dB.nslice + SP_WAVES * p.spwB - 1) / (SP_WAVES * p.spwB);
        p.tilesA = p.grpA * p.dA.nblk;
    } else {                               // (the non-zero path walks its images only)
        int rc = ensure_dense(ctx);
        if (!rc) rc = mu_ensure_xt(ctx, r.Gs);
        if (rc) return rc;
    }
    constexpr int SW = 32 * MuShape<KP>::NJT;                              // cells per divergence strip
    const int Np = r.Np, Gs = r.Gs, ntiles = Np / 32, nstrips = std::max((r.N + SW - 1) / SW, p.tilesA);
    p.nchunks = std::min(32, ntiles); p.tpc = (ntiles + p.nchunks - 1) / p.nchunks;
    DevPool& pool = r.pool;
    hipStream_t st = r.st;
    for (MuSlotDev& d : r.slot) {
        d.W = pool.get<float>((size_t)Np * KP, true, st);
        d.Ht = pool.get<float>((size_t)Gs * KP, true, st);
        d.Wp_hi = pool.get<mu_u16>((size_t)Np * KP, true, st); d.Wp_lo = pool.get<mu_u16>((size_t)Np * KP, true, st);
        d.Wc_hi = pool.get<mu_u16>((size_t)2 * Np * KP, true, st);
        d.Hp_hi = pool.get<mu_u16>((size_t)Gs * KP, true, st); d.Hp_lo = pool.get<mu_u16>((size_t)Gs * KP, true, st);
        d.Hc_hi = pool.get<mu_u16>((size_t)2 * Gs * KP, true, st);
        d.Hsum = pool.get<float>(KP, true, st); d.Wsum = pool.get<float>(KP, true, st);
        d.pnum = sparse ? pool.get<float>(std::max<size_t>(p.dA.nblk > 1 ? (size_t)p.dA.nblk * Np : 0, p.dB.nblk > 1 ? (size_t)p.dB.nblk * Gs : 0) * KP)
                        : pool.get<float>((size_t)p.nchunks * Gs * KP);
        d.pden = BETA1 ? nullptr : pool.get<float>((size_t)p.nchunks * Gs * KP);
        d.divpart = pool.get<double>(nstrips);
        d.cspart = pool.get<double>((size_t)256 * KP);
    }
    if (int rc = r.alloc_staging(sparse ? p.tilesA : (r.N + SW - 1) / SW)) return rc;
    HIP_TRY(ctx, dyn_lds_optin((const void*)mu_h_coop_kernel<KP, BETA1>, p.coop_lds));
    HIP_TRY(ctx, dyn_lds_optin((const void*)mu_w_coop_kernel<KP, 0, BETA1>, p.coop_lds));
    HIP_TRY(ctx, dyn_lds_optin((const void*)mu_w_coop_kernel<KP, 1, BETA1>, p.coop_lds));
    if constexpr (BETA1 && KP <= 64) if (sparse) {
        HIP_TRY(ctx, dyn_lds_optin((const void*)mu_sp_kernel<KP, 0, 0>, SP_LDS_BYTES));
        HIP_TRY(ctx, dyn_lds_optin((const void*)mu_sp_kernel<KP, 0, 1>, SP_LDS_BYTES));
        HIP_TRY(ctx, dyn_lds_optin((const void*)mu_sp_kernel<KP, 1, 0>, SP_LDS_BYTES));
    }
    return CNMF_OK;
}
static MuBatch mu_batch_of(const MuRun& r, const std::vector<int>& ids)
{
    MuBatch mb;
    for (mb.n = 0; mb.n < (int)ids.size(); ++mb.n) mb.s[mb.n] = r.slot[ids[mb.n]];
    return mb;
}
// column sums of W (which = 0) or Ht (1) of every slot of the batch
template <int KP>
static void mu_colsum_batch(const MuRun& r, const MuBatch& mb, int which)
{
    const int Rr = which ? r.G : r.N;
    const int nb = std::max(1, std::min(256, Rr / 256));
    mu_colsum_batch_part_kernel<KP><<<dim3(nb, mb.n), 256, 0, r.st>>>(mb, which, Rr);
    mu_colsum_batch_final_kernel<KP><<<dim3(1, mb.n), 1024, 0, r.st>>>(mb, which, nb);
}
// the bf16 planes of a freshly packed slot
template <int KP>
static void mu_planes(const MuRun& r, int si)
{
    const MuSlotDev& d = r.slot[si];
    mu_planes_kernel<KP><<<(int)(((size_t)r.Np * KP + 255) / 256), 256, 0, r.st>>>(d.W, r.Np, d.Wp_hi, d.Wp_lo, d.Wc_hi, d.Wc_hi + (size_t)r.Np * KP);
    mu_planes_kernel<KP><<<(r.Gs * KP + 255) / 256, 256, 0, r.st>>>(d.Ht, r.Gs, d.Hp_hi, d.Hp_lo, d.Hc_hi, d.Hc_hi + (size_t)r.Gs * KP);
}
// one iteration of the slots `ids`
template <int KP, bool BETA1>
static int mu_step(const MuRun& r, MuMfma<KP, BETA1>& p, const std::vector<int>& ids)
{
    hipStream_t st = r.st;
    const int N = r.N, G = r.G, Np = r.Np, Gs = r.Gs, update_H = r.c->update_H;
    const MuBatch mb = mu_batch_of(r, ids);
    const int gz4 = (mb.n + p.RPW - 1) / p.RPW;
    if (p.sparse) {
        if constexpr (BETA1 && KP <= 64) {
            mu_sp_kernel<KP, 0, 0><<<(p.tilesA + 7) / 8 * 8 * mb.n, SP_WAVES * 64, SP_LDS_BYTES, st>>>(p.dA, mb, p.grpA, 1, r.l1W, r.l2W, Np);
            if (p.dA.nblk > 1)
                mu_sp_finish_kernel<KP><<<dim3((unsigned)(((size_t)N * KP + 255) / 256), mb.n), 256, 0, st>>>(mb, 0, N, Np, p.dA.nblk, r.l1W, r.l2W);
            if (update_H) {
                mu_colsum_batch<KP>(r, mb, 0);
                const int tilesB = p.grpB * p.dB.nblk;
                mu_sp_kernel<KP, 0, 1><<<(tilesB + 7) / 8 * 8 * mb.n, SP_WAVES * 64, SP_LDS_BYTES, st>>>(p.dB, mb, p.grpB, p.spwB, r.l1H, r.l2H, Gs);
                if (p.dB.nblk > 1)
                    mu_sp_finish_kernel<KP><<<dim3((G * KP + 255) / 256, mb.n), 256, 0, st>>>(mb, 1, G, Gs, p.dB.nblk, r.l1H, r.l2H);
                mu_colsum_batch<KP>(r, mb, 1);
            }
        }
    } else {
        mu_w_coop_kernel<KP, 0, BETA1><<<dim3((N + 127) / 128, 1, gz4), 512, p.coop_lds, st>>>(r.ctx->XtF.p, Np, N, Gs, mb, r.l1W, r.l2W);
        if (update_H) {
            mu_colsum_batch<KP>(r, mb, 0);
            mu_h_coop_kernel<KP, BETA1><<<dim3(Gs / 128, p.nchunks, gz4), 512, p.coop_lds, st>>>(r.ctx->X, r.ldx, Np, Gs, mb, p.tpc, p.nchunks);
            mu_h_finish_mfma_kernel<KP, BETA1><<<dim3((Gs * KP + 255) / 256, mb.n), 256, 0, st>>>(mb, G, Gs, p.nchunks, r.l1H, r.l2H);
            mu_colsum_batch<KP>(r, mb, 1);
        }
    }
    HIP_TRY(r.ctx, hipGetLastError());
    return CNMF_OK;
}
// the divergence partials and column sums of the current factors of the slots `ids` (read_divergence fetches them)
template <int KP, bool BETA1>
static int mu_divergence(const MuRun& r, MuMfma<KP, BETA1>& p, const MuSched&, const std::vector<int>& ids)
{
    const MuBatch mb = mu_batch_of(r, ids);
    if (!r.c->update_H) mu_colsum_batch<KP>(r, mb, 0);           // refit: the iterations do not need the column sums of W
    if (p.sparse) {
        if constexpr (BETA1 && KP <= 64)
            mu_sp_kernel<KP, 1, 0><<<(p.tilesA + 7) / 8 * 8 * mb.n, SP_WAVES * 64, SP_LDS_BYTES, r.st>>>(p.dA, mb, p.grpA, 1, 0.f, 0.f, r.Np);
    } else
        mu_w_coop_kernel<KP, 1, BETA1><<<dim3((r.N + 127) / 128, 1, (mb.n + p.RPW - 1) / p.RPW), 512, p.coop_lds, r.st>>>(r.ctx->XtF.p, r.Np, r.N, r.Gs, mb, 0.f, 0.f);
    HIP_TRY(r.ctx, hipGetLastError());
    return CNMF_OK;
}

// -- the vector-ALU kernels (kernels_mu.hip.h): one slot, X only
template <int KP_, bool BETA1_>
struct MuValu {
    static constexpr int KP = KP_; static constexpr bool BETA1 = BETA1_, batched = false;
    int nchunks = 0, rpc = 0;              // row chunks of the H half-step / divergence kernels, rows per chunk
    bool hsum_valid = false;               // the slot's Hsum belongs to its current Ht
};
template <int KP, bool BETA1>
static int mu_setup(MuRun& r, MuValu<KP, BETA1>& v, bool)
{
    if (int rc = ensure_dense(r.ctx)) return rc;
    const int N = r.N, G = r.G;
    // ~8 waves per SIMD (2048 workgroups), >= 64 rows each
    v.nchunks = std::max(1, std::min(std::max(64, 2048 / std::max(1, (G + 255) / 256)), N / 64));
    v.rpc = (N + v.nchunks - 1) / v.nchunks;
    MuSlotDev& d = r.slot[0] = MuSlotDev{};
    d.W = r.pool.get<float>((size_t)N * KP);
    d.Ht = r.pool.get<float>((size_t)r.ldx * KP, true, r.st);
    d.Hsum = r.pool.get<float>(KP, true, r.st); d.Wsum = r.pool.get<float>(KP, true, r.st);
    d.pnum = r.pool.get<float>((size_t)v.nchunks * G * KP);
    d.pden = r.pool.get<float>(BETA1 ? 1 : (size_t)v.nchunks * G * KP);
    d.divpart = r.pool.get<double>((size_t)((G + 255) / 256) * v.nchunks);
    d.cspart = r.pool.get<double>((size_t)256 * 64);
    return r.alloc_staging((G + 255) / 256 * v.nchunks);
}
template <int KP>
static void mu_colsum_one(const MuRun& r, const float* M, int rows, float* out)
{
    const int nb = std::max(1, std::min(256, rows / 256));
    mu_colsum_part_kernel<KP><<<nb, 256, 0, r.st>>>(M, rows, r.slot[0].cspart);
    mu_colsum_final_kernel<KP><<<1, 64, 0, r.st>>>(r.slot[0].cspart, nb, out);
}
template <int KP, bool BETA1>
static int mu_step(const MuRun& r, MuValu<KP, BETA1>& v, const std::vector<int>&)
{
    const MuSlotDev& d = r.slot[0];
    const int N = r.N, G = r.G;
    constexpr int NQ = KP <= 32 ? 8 : 4;
    if (BETA1 && !v.hsum_valid) { mu_colsum_one<KP>(r, d.Ht, G, d.Hsum); v.hsum_valid = true; }
    mu_w_kernel<KP, BETA1, NQ><<<(N + 63) / 64, 64 * NQ, 0, r.st>>>(r.ctx->X, r.ldx, N, G, d.W, d.Ht, d.Hsum, r.l1W, r.l2W);
    if (r.c->update_H) {
        if (BETA1) mu_colsum_one<KP>(r, d.W, N, d.Wsum);
        mu_h_partial_kernel<KP, BETA1><<<dim3((G + 255) / 256, v.nchunks), 256, 0, r.st>>>(r.ctx->X, r.ldx, N, G, d.W, d.Ht, v.rpc, d.pnum, d.pden);
        mu_h_finish_kernel<KP, BETA1><<<(G * KP + 255) / 256, 256, 0, r.st>>>(d.Ht, G, d.pnum, d.pden, v.nchunks, d.Wsum, r.l1H, r.l2H);
        v.hsum_valid = false;
    }
    HIP_TRY(r.ctx, hipGetLastError());
    return CNMF_OK;
}
template <int KP, bool BETA1>
static int mu_divergence(const MuRun& r, MuValu<KP, BETA1>& v, const MuSched& sc, const std::vector<int>&)
{
    const MuSlotDev& d = r.slot[0];
    mu_colsum_one<KP>(r, d.Ht, r.G, d.Hsum);
    mu_colsum_one<KP>(r, d.W, r.N, d.Wsum);
    mu_divergence_kernel<KP, BETA1><<<dim3((r.G + 255) / 256, v.nchunks), 256, 0, r.st>>>(r.ctx->X, r.ldx, r.N, r.G, d.W, d.Ht, v.rpc, d.divpart);
    HIP_TRY(r.ctx, hipGetLastError());
    v.hsum_valid = !sc.slots[0].fresh;     // (as it always was: the first iteration sums H again after the evaluation at installation)
    return CNMF_OK;
}

// -- one slot path for all kernel families
// The initial factors of the placed jobs into their slots: update_H = 0 (the caller's H, W filled with avg: sklearn
// _nmf.py:1229-1231), the caller's factors (init_mode 0), or seeded (ONE launch for all placements: a workgroup per
// restart, the Mersenne twister is serial inside it).
template <class P>
static int install_slots(MuRun& r, const std::vector<MuPlacement>& pl)
{
    cnmf_ctx* ctx = r.ctx; hipStream_t st = r.st;
    const MuCall& c = *r.c;
    const int N = r.N, G = r.G, KP = r.KP;
    const int gHt = (G * KP + 255) / 256, gWp = (int)(((size_t)N * KP + 255) / 256);
    if (c.update_H && c.init_mode == 1) {
        std::vector<RngJob> hj(pl.size());
        for (size_t i = 0; i < pl.size(); ++i) {
            const MuJob& jb = (*r.jobs)[pl[i].job];
            hj[i] = RngJob{c.seeds[jb.restart], jb.k, pl[i].slot * r.kmax, c.avg[jb.restart], (long long)jb.k * ((long long)G + N)};
        }
        HIP_TRY(ctx, hipMemcpyAsync(r.dj, hj.data(), hj.size() * sizeof(RngJob), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                      // `hj` is a stack temporary
        rng_kernel<1><<<(int)pl.size(), 256, 0, st>>>(r.dj, nullptr, r.cmH, G, G, r.cmW, N, N);
    }
    std::vector<int> ids;
    for (const MuPlacement& q : pl) {
        MuSlotDev& d = r.slot[q.slot];
        const MuJob& jb = (*r.jobs)[q.job];
        const int k = jb.k;
        float* cH = r.cmH + (size_t)q.slot * r.kmax * G;
        float* cW = r.cmW + (size_t)q.slot * r.kmax * N;
        if (!c.update_H || c.init_mode == 0)
            HIP_TRY(ctx, hipMemcpyAsync(cH, c.H0 + jb.hoff, (size_t)k * G * sizeof(float), hipMemcpyHostToDevice, st));
        if (c.update_H && c.init_mode == 0)
            HIP_TRY(ctx, hipMemcpyAsync(cW, c.W0 + jb.woff, (size_t)k * N * sizeof(float), hipMemcpyHostToDevice, st));
        if (c.update_H && c.init_mode == 2) {                        // the init store: component-major like the seeded factors
            HIP_TRY(ctx, hipMemcpyAsync(cH, ctx->inits.H + jb.hoff, (size_t)k * G * sizeof(float), hipMemcpyDeviceToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(cW, ctx->inits.Wt + jb.woff, (size_t)k * N * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        mu_pack_kernel<<<gHt, 256, 0, st>>>(cH, k, G, d.Ht, KP);
        if (!c.update_H) mu_fill_kernel<<<gWp, 256, 0, st>>>(d.W, k, N, KP, (float)c.avg[jb.restart]);
        else if (c.init_mode == 0) mu_pack_rm_kernel<<<gWp, 256, 0, st>>>(cW, k, N, d.W, KP);
        else mu_pack_kernel<<<gWp, 256, 0, st>>>(cW, k, N, d.W, KP);
        d.k = k;
        if constexpr (P::batched) mu_planes<P::KP>(r, q.slot);
        ids.push_back(q.slot);
    }
    if constexpr (P::batched) {                                      // the column sums of all fresh slots
        const MuBatch mb = mu_batch_of(r, ids);
        mu_colsum_batch<P::KP>(r, mb, 0); mu_colsum_batch<P::KP>(r, mb, 1);
    }
    HIP_TRY(ctx, hipGetLastError());
    return CNMF_OK;
}

// the result of the restart in slot si to the caller: the factors unpacked, n_iter and err; the slot is free then
static int retire_slot(const MuRun& r, MuSched& sc, int si)
{
    const MuHostSlot& s = sc.slots[si];
    const MuCall& c = *r.c;
    const MuJob& jb = (*r.jobs)[s.job];
    const MuSlotDev& d = r.slot[si];
    const int N = r.N, G = r.G, k = jb.k;
    float* cH = r.cmH + (size_t)si * r.kmax * G;
    float* cW = r.cmW + (size_t)si * r.kmax * N;
    if (c.H_out && c.update_H) {
        mu_unpack_kernel<<<(G * k + 255) / 256, 256, 0, r.st>>>(d.Ht, k, G, r.KP, cH, 1);
        HIP_TRY(r.ctx, hipMemcpyAsync(c.H_out + jb.hoff, cH, (size_t)k * G * sizeof(float), hipMemcpyDeviceToHost, r.st));
    }
    if (c.W_out) {
        mu_unpack_kernel<<<(int)(((size_t)N * k + 255) / 256), 256, 0, r.st>>>(d.W, k, N, r.KP, cW, 0);
        HIP_TRY(r.ctx, hipMemcpyAsync(c.W_out + jb.woff, cW, (size_t)k * N * sizeof(float), hipMemcpyDeviceToHost, r.st));
    }
    HIP_TRY(r.ctx, hipStreamSynchronize(r.st));
    if (c.n_iter_out) c.n_iter_out[jb.restart] = s.it;
    if (c.err_out) c.err_out[jb.restart] = s.err;
    sc.retire(si);
    return CNMF_OK;
}

// sqrt(2 D) of the i-th fetched slot: the partials in index order, then + sum(WH) from the column sums (Kullback-Leibler)
// or - N G (Itakura-Saito: sum(X/WH) - N G - sum log(X/WH))
static double reduce_divergence(const MuRun& r, int i)
{
    double res = 0.0;
    for (int q = 0; q < r.ndiv; ++q) res += r.hdiv[(size_t)i * r.ndiv + q];
    const float* hs = r.hsums.data() + (size_t)i * 2 * r.KP;
    if (r.c->beta == 1) {
        double swh = 0.0;
        for (int c = 0; c < r.KP; ++c) swh += (double)hs[c] * (double)hs[r.KP + c];
        res += swh;
    } else res -= (double)r.N * (double)r.G;
    return std::sqrt(2.0 * std::max(res, 0.0));
}
// what mu_divergence left on the device for the slots `ids` -> err[] (host)
static int read_divergence(MuRun& r, const std::vector<int>& ids, std::vector<double>& err)
{
    const size_t KP = r.KP;
    for (size_t i = 0; i < ids.size(); ++i) {
        const MuSlotDev& d = r.slot[ids[i]];
        HIP_TRY(r.ctx, hipMemcpyAsync(r.hdiv.data() + i * r.ndiv, d.divpart, (size_t)r.ndiv * sizeof(double), hipMemcpyDeviceToHost, r.st));
        HIP_TRY(r.ctx, hipMemcpyAsync(r.hsums.data() + i * 2 * KP, d.Hsum, KP * sizeof(float), hipMemcpyDeviceToHost, r.st));
        HIP_TRY(r.ctx, hipMemcpyAsync(r.hsums.data() + i * 2 * KP + KP, d.Wsum, KP * sizeof(float), hipMemcpyDeviceToHost, r.st));
    }
    HIP_TRY(r.ctx, hipStreamSynchronize(r.st));
    err.resize(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) err[i] = reduce_divergence(r, (int)i);
    return CNMF_OK;
}

// The loop of mu_sched.h (its header comment gives the protocol) with the device work of every step.
template <class P>
static int mu_drive(MuRun& r, P& p)
{
    MuSched sc(r.R, (int)r.jobs->size(), r.c->prm->max_iter, r.c->prm->tol, r.c->err_out != nullptr);
    std::vector<MuPlacement> placed; std::vector<MuFinal> finals;
    std::vector<int> ids, converged; std::vector<double> errs;
    int rc = CNMF_OK;
    for (;;) {
        if (sc.aligned()) {
            sc.refill(&placed);
            if (!placed.empty() && (rc = install_slots<P>(r, placed))) return rc;
            sc.due(&ids);
            if (!ids.empty()) {
                if ((rc = mu_divergence(r, p, sc, ids)) || (rc = read_divergence(r, ids, errs))) return rc;
                sc.report(ids, errs, &converged);
                for (int si : converged) if ((rc = retire_slot(r, sc, si))) return rc;
            }
        }
        // (err_out is the divergence of the FINAL factors, what sklearn's reconstruction_err_ reports)
        sc.exhausted(&finals);
        for (const MuFinal& f : finals) {
            if (f.eval) {
                ids.assign(1, f.slot);
                if ((rc = mu_divergence(r, p, sc, ids)) || (rc = read_divergence(r, ids, errs))) return rc;
                sc.report_final(f.slot, errs[0]);
            }
            if ((rc = retire_slot(r, sc, f.slot))) return rc;
        }
        sc.live(&ids);
        if (ids.empty()) { if (sc.finished()) break; else continue; }
        if ((rc = mu_step(r, p, ids))) return rc;
        sc.advance(ids);
    }
    return CNMF_OK;
}

enum MuFamily { MU_DENSE, MU_SPARSE, MU_VALU };
template <class P>
static int mu_run_on(cnmf_ctx* ctx, const MuCall& c, const std::vector<MuJob>& jobs, int R, bool sparse)
{
    MuRun r(ctx, c, jobs, P::KP, R);
    P p;
    if (int rc = mu_setup(r, p, sparse)) return rc;
    return mu_drive(r, p);
}
template <int KP, bool BETA1>
static int mu_run(cnmf_ctx* ctx, const MuCall& c, const std::vector<MuJob>& jobs, MuFamily fam)
{
    if constexpr (KP <= 64) {              // (their per-lane w[KP], num[KP], den[KP] do not fit above; refused before any launch)
        if (fam == MU_VALU) return mu_run_on<MuValu<KP, BETA1>>(ctx, c, jobs, 1, false);
    } else if (fam == MU_VALU) return CNMF_EUNSUPPORTED;
    if constexpr (KP >= 16)
        return mu_run_on<MuMfma<KP, BETA1>>(ctx, c, jobs, (int)std::min<size_t>(MU_MAXSLOTS, jobs.size()), fam == MU_SPARSE);
    return CNMF_EINVAL;
}
// the one dispatch over (padded rank, beta)
static int mu_run_kp(cnmf_ctx* ctx, const MuCall& c, const std::vector<MuJob>& jobs, int KP, MuFamily fam)
{
    const bool b1 = c.beta == 1;
    switch (KP) {
    case 8:  return b1 ? mu_run<8, true>(ctx, c, jobs, fam) : mu_run<8, false>(ctx, c, jobs, fam);
    case 16: return b1 ? mu_run<16, true>(ctx, c, jobs, fam) : mu_run<16, false>(ctx, c, jobs, fam);
    case 32: return b1 ? mu_run<32, true>(ctx, c, jobs, fam) : mu_run<32, false>(ctx, c, jobs, fam);
    case 128: return b1 ? mu_run<128, true>(ctx, c, jobs, fam) : mu_run<128, false>(ctx, c, jobs, fam);
    default: return b1 ? mu_run<64, true>(ctx, c, jobs, fam) : mu_run<64, false>(ctx, c, jobs, fam);
    }
}

}  // namespace cnmf

// the largest rank the multiplicative-update entry points accept on this context: CNMF_MU_KMAX unless the caller opts in
extern "C" int cnmf_set_mu_rank_limit(cnmf_ctx* ctx, int limit)
{
    if (!ctx) { SET_ERR(ctx, "ctx is NULL"); return CNMF_EINVAL; }
    if (limit != CNMF_MU_KMAX && limit != CNMF_MU_KMAX_WIDE) {
        SET_ERR(ctx, "the multiplicative-update rank limit is %d or %d, not %d", CNMF_MU_KMAX, CNMF_MU_KMAX_WIDE, limit);
        return CNMF_EINVAL;
    }
    ctx->mu_rank_limit = limit;
    return CNMF_OK;
}
extern "C" int cnmf_get_mu_rank_limit(const cnmf_ctx* ctx) { return ctx ? ctx->mu_rank_limit : CNMF_MU_KMAX; }

// the largest rank of a Kullback-Leibler restart that may run on the non-zeros: CNMF_MU_SPARSE_KMAX unless the caller opts in
extern "C" int cnmf_set_mu_sparse_rank_limit(cnmf_ctx* ctx, int limit)
{
    if (!ctx) { SET_ERR(ctx, "ctx is NULL"); return CNMF_EINVAL; }
    if (limit != CNMF_MU_SPARSE_KMAX && limit != CNMF_MU_SPARSE_KMAX_WIDE) {
        SET_ERR(ctx, "the rank limit of the non-zero path is %d or %d, not %d", CNMF_MU_SPARSE_KMAX, CNMF_MU_SPARSE_KMAX_WIDE, limit);
        return CNMF_EINVAL;
    }
    ctx->mu_sparse_rank_limit = limit;
    return CNMF_OK;
}
extern "C" int cnmf_get_mu_sparse_rank_limit(const cnmf_ctx* ctx) { return ctx ? ctx->mu_sparse_rank_limit : CNMF_MU_SPARSE_KMAX; }

extern "C" int cnmf_nmf_mu_batch(cnmf_ctx* ctx, int n, const int32_t* kk, int init_mode,
                                 const uint32_t* seeds, const double* avg, const float* W0,
                                 const float* H0, int beta, int update_H, const cnmf_cd_params* prm,
                                 float* H_out, float* W_out, int32_t* n_iter_out, double* err_out)
{
    using namespace cnmf;
    if (!ctx) { SET_ERR(ctx, "ctx is NULL"); return CNMF_EINVAL; }
    if (!ctx->X && !ctx->csr.ptr) { SET_ERR(ctx, "cnmf_set_matrix has not been called"); return CNMF_ESTATE; }
    int rc = validate_params(ctx, prm);
    if (rc) return rc;
    if (beta != 0 && beta != 1) { SET_ERR(ctx, "beta_loss must be 1 (kullback-leibler) or 0 (itakura-saito)"); return CNMF_EUNSUPPORTED; }
    if (n < 0 || (n > 0 && !kk)) { SET_ERR(ctx, "bad restart list"); return CNMF_EINVAL; }
    if (!update_H && (!H0 || !avg)) { SET_ERR(ctx, "update_H=0 needs H0 and avg"); return CNMF_EINVAL; }
    if (update_H && init_mode == 0 && n > 0 && (!W0 || !H0)) { SET_ERR(ctx, "init_mode 0 needs W0 and H0"); return CNMF_EINVAL; }
    if (update_H && init_mode == 1 && n > 0 && (!seeds || !avg)) { SET_ERR(ctx, "init_mode 1 needs seeds and avg"); return CNMF_EINVAL; }
    if (update_H && (init_mode < 0 || init_mode > 2)) { SET_ERR(ctx, "unknown init_mode %d", init_mode); return CNMF_EINVAL; }
    if (update_H && init_mode == 2 && n > 0 && (rc = check_init_store(ctx, n, kk))) return rc;
    if (update_H && n > 0 && !H_out) { SET_ERR(ctx, "H_out is NULL"); return CNMF_EINVAL; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const MuCall call{init_mode, beta, update_H, seeds, avg, W0, H0, prm, H_out, W_out, n_iter_out, err_out};
    // jobs by padded rank 16 / 32 / 64 / 128 (the last under cnmf_set_mu_rank_limit(CNMF_MU_KMAX_WIDE) only), each group
    // batched on the matrix pipe; or one restart at a time on the vector-ALU
    // kernels: CNMF_MU_VALU=1, and matrices beyond 2^24 cells or genes (the matrix-pipe kernels address a 32-row step of
    // X / X^T with 32-bit byte offsets below 2^31, the buffer descriptor's range: 4 * 32 * row length)
    const bool valu = ctx->mu_knobs.valu || ctx->N_pad > (1 << 24) || ctx->G_pad > (1 << 24);
    std::vector<MuJob> group[4], one(1);
    size_t ho = 0, wo = 0;
    for (int r = 0; r < n; ++r) {
        const int k = kk[r];
        if (k < 1) { SET_ERR(ctx, "n_components must be >= 1"); return CNMF_EINVAL; }
        if (k > ctx->mu_rank_limit) {
            if (ctx->mu_rank_limit < CNMF_MU_KMAX_WIDE && k <= CNMF_MU_KMAX_WIDE)
                SET_ERR(ctx, "n_components=%d > %d is not supported by the multiplicative-update solver on the device under the rank limit in force "
                             "(%d); cnmf_set_mu_rank_limit(ctx, %d) admits ranks up to %d", k, ctx->mu_rank_limit, ctx->mu_rank_limit,
                        CNMF_MU_KMAX_WIDE, CNMF_MU_KMAX_WIDE);
            else
                SET_ERR(ctx, "n_components=%d > %d is not supported by the multiplicative-update solver on the device (rank limit in force %d, "
                             "the largest cnmf_set_mu_rank_limit accepts is %d)", k, ctx->mu_rank_limit, ctx->mu_rank_limit, CNMF_MU_KMAX_WIDE);
            return CNMF_EUNSUPPORTED;
        }
        if (valu && k > CNMF_MU_KMAX) {
            SET_ERR(ctx, "n_components=%d > %d is not supported on the vector-ALU route of the multiplicative-update solver (CNMF_MU_VALU=1, "
                         "or a matrix beyond 2^24 cells or genes): ranks %d..%d run on the matrix-pipe kernels only", k, CNMF_MU_KMAX,
                    CNMF_MU_KMAX + 1, CNMF_MU_KMAX_WIDE);
            return CNMF_EUNSUPPORTED;
        }
        group[valu ? 0 : (k <= 16 ? 0 : (k <= 32 ? 1 : (k <= 64 ? 2 : 3)))].push_back(MuJob{r, k, ho, wo});
        ho += (size_t)k * ctx->G; wo += (size_t)k * ctx->N;
    }
    if (valu) {
        for (const MuJob& j : group[0]) {
            one[0] = j;
            if ((rc = mu_run_kp(ctx, call, one, j.k <= 8 ? 8 : (j.k <= 16 ? 16 : (j.k <= 32 ? 32 : 64)), MU_VALU))) return rc;
        }
        return CNMF_OK;
    }
    // Kullback-Leibler at padded ranks 16 / 32 (and 64 under cnmf_set_mu_sparse_rank_limit) on a matrix that is mostly zeros:
    // only the non-zeros are touched; ranks 65..128 stay on the dense kernels
    bool sparse[4] = {false, false, false, false};
    for (int g = 0; g < 3; ++g)
        if (beta == 1 && !group[g].empty() && (rc = mu_sparse_prepare(ctx, 16 << g, &sparse[g]))) return rc;
    for (int g = 0; g < 4; ++g)
        if (!group[g].empty() && (rc = mu_run_kp(ctx, call, group[g], 16 << g, sparse[g] ? MU_SPARSE : MU_DENSE))) return rc;
    return CNMF_OK;
}
