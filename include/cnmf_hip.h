/* libcnmf_hip.so -- C ABI of the MI355X-native consensus-NMF engine.
 *
 * The reference (dylkot/cNMF v1.7.1) has no FFI: its hot path is Python method
 * dispatch on `class cNMF` that bottoms out in scikit-learn.  The entry points
 * below are what a ctypes binding behind those methods calls; each one names the
 * reference interface it replaces (paths are /root/reference/src/cnmf/cnmf.py
 * unless prefixed sklearn:).  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - plain pointers and sizes only; the CALLER owns every host buffer (numpy),
 *     the library owns all device memory behind the opaque context;
 *   - every call returns 0 on success or a negative CNMF_E* code; the message is
 *     available from cnmf_last_error() (the Python wrapper maps codes to the same
 *     exception types the reference path raises);
 *   - one context per GPU, one host thread per context; no global mutable state
 *     (multiprocessing fan-out with one process per GPU = one `worker_i` works);
 *   - matrices are C-order float32.  Factor packing for a batch of restarts
 *     r = 0..n-1 with ranks k[r]:  H blocks [k[r]][G] concatenated in r order,
 *     W blocks [N][k[r]] concatenated in r order (sklearn's own layouts).
 */
#ifndef CNMF_HIP_H
#define CNMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNMF_OK            0
#define CNMF_EINVAL       -1   /* bad argument (ValueError on the Python side)   */
#define CNMF_EHIP         -2   /* HIP runtime failure (RuntimeError)             */
#define CNMF_ENOMEM       -3   /* device allocation failed (MemoryError)         */
#define CNMF_ESTATE       -4   /* call order violated, e.g. no matrix set        */
#define CNMF_EUNSUPPORTED -5   /* e.g. rank > CNMF_KMAX (NotImplementedError)    */
#define CNMF_ECOMM        -6   /* RCCL failure                                   */

#define CNMF_HARMONY_KMAX 128  /* most clusters of cnmf_harmony_begin (CNMF_EUNSUPPORTED above)                             */
#define CNMF_HARMONY_DMAX 64   /* most components of cnmf_harmony_begin                                                     */
#define CNMF_RIDGE_MAX 4096    /* largest K * (B + 1) of cnmf_preprocess_ridge_moments (CNMF_EUNSUPPORTED above)      */
#define CNMF_PCA_NMAX 8192     /* largest matrix of the tridiagonalisation entry points (CNMF_EUNSUPPORTED above)            */
#define CNMF_LINKAGE_MAX 4096  /* largest cluster of cnmf_clustergram: 20 bytes of LDS per member (CNMF_EUNSUPPORTED above)        */
#define CNMF_KMAX 128          /* largest rank of the coordinate-descent / NNLS / consensus entry points
                                  (<= 64: register-resident sweep; 65..128: sweep_big_kernel)              */

#define CNMF_MU_KMAX 64        /* largest rank of the multiplicative-update entry points (cnmf_nmf_mu_batch,
                                  cnmf_mu_refit_f64) on a context as created ...                            */
#define CNMF_MU_KMAX_WIDE 128  /* ... and after cnmf_set_mu_rank_limit(ctx, CNMF_MU_KMAX_WIDE): ranks 65..128 on the
                                  matrix-pipe kernels and the float64 refit (the vector-ALU route stays at 64)  */

#define CNMF_MU_SPARSE_KMAX 32       /* largest rank of a Kullback-Leibler restart on the non-zeros of X on a context as created ... */
#define CNMF_MU_SPARSE_KMAX_WIDE 64  /* ... and after cnmf_set_mu_sparse_rank_limit(ctx, CNMF_MU_SPARSE_KMAX_WIDE): ranks 33..64 at padded
                                        rank 64, two lanes per row (ranks 65..128 stay on the dense kernels)                        */

typedef struct cnmf_ctx cnmf_ctx;

/* numpy's RandomState state (get_state()): the MT19937 key, pos in [0, 624], the cached Gaussian */
typedef struct cnmf_mt_state {
    uint32_t key[624];
    int32_t pos;
    int32_t has_gauss;
    double gauss;
} cnmf_mt_state;

/* Solver parameters = the yaml kwargs the reference persists (cnmf.py:618-631)
 * after sklearn's scaling of the regularisers (sklearn:decomposition/_nmf.py:1254-1265):
 *   l1_reg_W = G*alpha_W*l1_ratio   l2_reg_W = G*alpha_W*(1-l1_ratio)
 *   l1_reg_H = N*alpha_H*l1_ratio   l2_reg_H = N*alpha_H*(1-l1_ratio)        */
typedef struct cnmf_cd_params {
    double tol;          /* 1e-4 in the reference (cnmf.py:624)                  */
    int    max_iter;     /* 1000 (cnmf.py:567,625)                               */
    int    kc_max;       /* max packed component columns in flight: 32..256 in steps of 32, 512 / 768 / 1024 (wide batches:
                            several 256-column component groups per GEMM pass, matrix-pipe paths only); 0 = auto
                            (up to 256; as wide as the job up to 1024 on matrices of >= 2^24 padded entries)        */
    double l1_reg_W, l2_reg_W, l1_reg_H, l2_reg_H;
    int    lag;          /* host polls convergence `lag` iterations behind the GPU; 0 = default (2) */
    int    profile;      /* n > 0: bracket the two GEMM passes of every n-th iteration with HIP events
                            (fills passA_ms/passB_ms and the launch counts of the sampled iterations) */
} cnmf_cd_params;

/* Per-call statistics (optional, may be NULL). */
typedef struct cnmf_batch_stats {
    int64_t outer_iterations;      /* batch iterations enqueued (each = pass A + pass B)        */
    int64_t restart_iterations;    /* sum over restarts of their n_iter                         */
    int64_t column_iterations;     /* sum over batch iterations of KC (incl. idle columns)      */
    int64_t restart_column_iterations; /* sum over restarts of n_iter*k (algorithmic columns)  */
    double  gpu_ms;                /* device time of the whole call (hipEvent)                  */
    double  passA_ms, passB_ms;    /* summed hipEvent time of the two MFMA GEMM passes          */
    int64_t passA_launches, passB_launches;
    int32_t kc;                    /* packed column count used                                  */
    int32_t nsplit;                /* split-K factor of pass B                                  */
    int32_t gemm_mode;             /* GEMM path of the 256-column phase of this call: 0 = exact-f32 MFMA,
                                      1/2 = split-operand bf16 MFMA (3 x 3 planes, any X), 3 = count-structured X
                                      as one integer bf16 plane x 3 factor planes, 4 (the default when the count
                                      structure is detected) = integer f16 plane x 2 f16 factor planes         */
    int32_t reserved_;
    /* the tail of the call: from the moment the queue of pending restarts ran dry (nothing left to refill freed
     * columns with) to the end -- what strong scaling over more GPUs pays for (fewer restarts per rank)          */
    int64_t tail_iterations;       /* batch iterations enqueued after the queue ran dry                         */
    int64_t tail_live_columns;     /* sum over those iterations of the columns still iterating (host view)      */
    double  tail_ms;               /* device time of that phase (hipEvent)                                      */
} cnmf_batch_stats;

/* ---- lifecycle ------------------------------------------------------------------- */
int         cnmf_device_count(void);
cnmf_ctx*   cnmf_create(int device);           /* NULL on failure; see cnmf_last_error(NULL) */
void        cnmf_destroy(cnmf_ctx* ctx);
const char* cnmf_last_error(const cnmf_ctx* ctx);
/* The CNMF_* environment variables (INTEGRATION.md "Runtime switches") are read ONCE, when the context is created, into
 * the context; cnmf_reload_env re-reads all of them (A/B tools, tests).  A knob therefore cannot change between two
 * calls on one context unless the caller asks for it.  The one exception is CNMF_RCCL_LIB, the path RCCL is loaded
 * from: read from the process environment the first time a communicator is formed.
 * CNMF_G2_U8 (default 1): a count-structured matrix none of whose counts exceeds 255 keeps its integer planes as one byte
 * per count, which the f16 GEMM passes convert in registers -- the same operands, the same bits, half the plane bytes;
 * 0 = the f16 plane as before.  A change takes effect, like CNMF_GEMM3, at the next call: the planes are rebuilt.      */
int cnmf_reload_env(cnmf_ctx* ctx);
const char* cnmf_version(void);

/* ---- data matrix ------------------------------------------------------------------
 * Replaces the per-worker `norm_counts = sc.read(...)` + `norm_counts.X` hand-off of
 * cNMF.factorize (cnmf.py:726,741) and cNMF.consensus (cnmf.py:873,919): X (cells x
 * high-variance genes) is uploaded ONCE per context and stays resident in HBM.       */
int cnmf_set_matrix(cnmf_ctx* ctx, const float* X, int64_t n_cells, int64_t n_genes);
/* Count-structure detection (default on): the engine recognises X = (integers <= 65 535) x (one constant per gene)
 * -- what `norm_counts.X /= std` produces (cnmf.py:540-548) -- with a tolerance of 1e-3 count units and then
 * multiplies the exact integer planes; enabled = 0 keeps every matrix on the general float32-operand path.      */
int cnmf_set_count_detection(cnmf_ctx* ctx, int enabled);
/* CSR input (scipy.sparse.csr_matrix of float32, int32 indices/indptr) -- the reference hands `norm_counts.X` / `tpm.X`
 * to scikit-learn as stored (cnmf.py:726, 873, 950).  The arrays STAY on the device and serve the paths that walk the
 * stored entries (cnmf_mu_refit_f64, the non-zero images of cnmf_nmf_mu_batch) -- as uploaded when every row lists
 * strictly increasing columns without stored zeros (scipy's canonical format after eliminate_zeros(); the Python
 * wrapper compacts stored zeros before the call).  The dense float32 image is formed on the device ONLY when a path
 * that multiplies the dense matrix asks for it (coordinate descent, NNLS, Itakura-Saito restarts; duplicates summed like
 * .toarray()); arrays that are not canonical form it at once and the compressed rows are rebuilt from it on first use.
 * A column index outside [0, n_genes): CNMF_EINVAL.                                                              */
int cnmf_set_matrix_csr(cnmf_ctx* ctx, const int32_t* indptr, const int32_t* indices,
                        const float* data, int64_t n_cells, int64_t n_genes);
int cnmf_get_shape(const cnmf_ctx* ctx, int64_t* n_cells, int64_t* n_genes);
/* Which images of the matrix are resident right now (round 5): bit 0 the dense float32 image (a CSR upload forms it only when
 * a path that multiplies the dense matrix asks for it: a Kullback-Leibler run on a sparse matrix never does), bit 1 the
 * compressed rows of X, bit 2 those of X^T, bit 3 the dense X^T copy of the dense multiplicative-update kernels,
 * bits 4 / 5 the non-zero images at padded rank 16 / 32, bit 6 the integer count planes of the coordinate-descent path,
 * bit 7 those planes held as one byte per count (CNMF_G2_U8), bit 8 the non-zero images at padded rank 64. */
int cnmf_matrix_images(const cnmf_ctx* ctx, int32_t* flags);
/* the resident matrix back on the host ([n_cells][n_genes] float32) */
int cnmf_get_matrix(cnmf_ctx* ctx, float* out);

/* ---- gene-wise scaling of the resident matrix ------------------------------------------
 * The dense branch of the reference's get_norm_counts (cnmf.py:540-554): upload the raw counts of
 * the high-variance genes with cnmf_set_matrix, then
 *     cnmf_col_moments   -> mean[g] and ssd[g] = sum_i (x_ig - mean_g)^2   (float64, two passes)
 *                           std(ddof=1) = sqrt(ssd / (n_cells - 1)) is formed by the caller
 *     cnmf_scale_columns -> x_ig = float32(float64(x_ig) / divisor[g])     (divisors must be > 0)
 *     cnmf_row_sums      -> float64 sum over the genes of every cell: the "zero cells" check
 *                           (cnmf.py:550-554) and X.mean() for the random init are derived from it */
int cnmf_col_moments(cnmf_ctx* ctx, double* mean_out /* [G] */, double* ssd_out /* [G] */);
int cnmf_scale_columns(cnmf_ctx* ctx, const double* divisor /* [G] */);
int cnmf_row_sums(cnmf_ctx* ctx, double* out /* [N] */);

/* ---- prepare: TPM, gene statistics and the high-variance-gene matrix -----------------------
 * The O(nnz) passes of the reference's prepare (cnmf.py:333-459, get_norm_counts :487-556) on a STAGING matrix: the
 * raw cells x all-genes counts as CSR, held apart from the resident matrix and released by cnmf_prepare_fetch (or by
 * the next upload / cnmf_destroy).  Everything is accumulated in float64 in a fixed order (no float atomics): two
 * calls on the same input give the same bits.
 *   cnmf_prepare_upload_csr  indptr int64 [n_cells + 1], indices int32, data float32 (data_is_f64 = 0: counts up to
 *                            2^24 are exact) or float64 (data_is_f64 = 1: values that float32 would round keep their
 *                            bits).  Rows must list strictly increasing columns with finite values > 0 (scipy's
 *                            canonical format after eliminate_zeros()); a column index outside [0, n_genes), a bad
 *                            row pointer, a non-canonical row or a value <= 0: CNMF_EINVAL.
 *   cnmf_prepare_tpm_stats   row_sums[i] = sum_g x_ig; with target_sum > 0 the TPM is tpm_ig = x_ig * (target_sum /
 *                            row_sums[i]) (0 for a cell without counts; cnmf.py:245-251 / sc.pp.normalize_total), with
 *                            target_sum <= 0 the matrix as given (the tpm_fn route, cnmf.py:406-433).  mean / var: the
 *                            per-gene mean and POPULATION variance of that matrix (cnmf.py:436-447, two passes).
 *                            tpm_data (may be NULL): the TPM values in the uploaded CSR order [nnz].
 *   cnmf_prepare_select      gathers the columns genes[0..n_sel) (in list order) of the raw counts, std_out[j] = their
 *                            ddof=1 standard deviation, and divides: y = x / s in float64 with s = std, or 1 where
 *                            std == 0 and densify == 0 (sc.pp.scale(zero_center=False)); densify != 0 refuses a zero
 *                            std (CNMF_EINVAL: x /= std would leave NaN / inf, cnmf.py:544).  The result REPLACES the
 *                            resident matrix, as cnmf_set_matrix (densify) or cnmf_set_matrix_csr would build it from
 *                            float32(y): the same images, bit for bit.  row_sums_out[i] = float64 sum of row i of y
 *                            (the zero-cell check, cnmf.py:550-554); nnz_out = stored entries of y.  The staging counts
 *                            are released.
 *   cnmf_prepare_fetch       y in float64 for the normalised-counts file: densify == 0 -> CSR (indptr [n_cells + 1],
 *                            indices [nnz], values [nnz]; columns ascending in every row), densify != 0 -> values
 *                            [n_cells][n_sel] row-major (indptr / indices may be NULL).  Releases what select kept. */
int cnmf_prepare_upload_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                            int data_is_f64, int64_t n_cells, int64_t n_genes);
int cnmf_prepare_tpm_stats(cnmf_ctx* ctx, double target_sum, double* row_sums /* [N] */, double* mean /* [G] */,
                           double* var /* [G] */, double* tpm_data /* [nnz] or NULL */);
int cnmf_prepare_select(cnmf_ctx* ctx, int32_t n_sel, const int32_t* genes, int32_t densify, double* std_out /* [n_sel] */,
                        double* row_sums_out /* [N] */, int64_t* nnz_out);
int cnmf_prepare_fetch(cnmf_ctx* ctx, int64_t* indptr, int32_t* indices, double* values);
/* releases the staging and any result not fetched (a prepare that stops between upload and fetch); harmless otherwise */
int cnmf_prepare_release(cnmf_ctx* ctx);

/* ---- preprocess: scaling, quantile ceiling, PCA products and Harmony's ridge correction ------------------------
 * The O(N G) passes of the reference's Preprocess.normalize_batchcorrect (preprocess.py:9-29, 314-422) on a staging of
 * their own (two result slots, each cells x selected genes, CSR or dense float64), apart from the resident matrix, the
 * spectra store and the prepare staging.  Float64 throughout, fixed summation orders, no float atomics: two calls on the
 * same input give the same bits.
 *   cnmf_preprocess_upload_csr   the raw counts, as cnmf_prepare_upload_csr (same checks); releases the whole staging.
 *   cnmf_preprocess_set_dense    a dense row-major float64 matrix [n_rows][n_cols] into a slot (n_rows must match the
 *                                staged cells, if any).
 *   cnmf_preprocess_select       slot := the columns genes[0..n_sel) (list order) of the staged counts, each row scaled by
 *                                target_sum / its row sum over ALL genes when target_sum > 0 (sc.pp.normalize_total),
 *                                each column divided by its ddof=1 std (std_out; 1 where the std is 0), then v > max_value
 *                                -> max_value (+inf: no clip) -- sc.pp.scale(zero_center=False, max_value).  CSR result.
 *   cnmf_preprocess_order_stats  the k-th and (k+1)-th smallest (0-based; k+1 clamped to the last) of ALL n_cells x n
 *                                entries of a slot, implicit zeros of a CSR slot included; values must be >= 0.
 *   cnmf_preprocess_ceiling      v > thresh -> thresh over the slot, in place.
 *   cnmf_preprocess_densify      a CSR slot becomes dense (a no-op on a dense slot).
 *   cnmf_preprocess_fetch        a CSR slot: indptr [n_cells + 1], indices, values; a dense slot: values [n_cells][n].
 *   cnmf_preprocess_scatter      dense slot: mean [n] of its columns and scatter [n][n] = sum_i (x_i - mean)(x_i - mean)^T.
 *   cnmf_preprocess_project      dense slot: scores [n_cells][n_comp] = (X - mean) V, V [n][n_comp].
 *   cnmf_preprocess_ridge_moments  dense slot X [N][n], Rt [N][K] (R^T), Phit [N][B1] (Phi_moe^T), K * B1 <= CNMF_RIDGE_MAX:
 *                                M [K*B1][n] = A X and gram [K*B1][B1] = A Phi^T with A[k*B1 + b][i] = R[k][i] Phi[b][i].
 *                                Keeps Rt / Phit for the apply.
 *   cnmf_preprocess_ridge_apply  dense slot X := max(X - A^T W, 0) in place, W [K*B1][n] (the last moments' K, B1).
 *   cnmf_preprocess_ridge_apply_mode  the same with clip != 0; clip == 0: X := X - A^T W, for a matrix with negative entries.
 *   cnmf_preprocess_row_sums     row_sums [n_cells] of the staged counts (the sums normalize_total divides by).
 *   cnmf_preprocess_normalize_dense  slot := ALL genes of the staged counts as a dense [n_cells][n_genes] matrix, rows
 *                                scaled as cnmf_preprocess_select scales them (target_sum > 0), each column divided by its
 *                                ddof=1 std summed row after row as numpy's std(axis=0) of a C-ordered matrix sums (std_out;
 *                                1 where the std is 0), then v > max_value -> max_value (+inf: no clip).
 *   cnmf_preprocess_select_mi    sklearn's mutual_info_classif(X, cluster, n_neighbors) over a dense slot X [N][n]
 *                                (Preprocess.select_features_MI, preprocess.py:425-467): X / nanstd(X, 0) plus
 *                                1e-10 max(1, mean|X|) standard_normal((N, n)) drawn from *state (numpy's RandomState
 *                                state: any pos, with or without a cached Gaussian; the final state is written back),
 *                                then Ross's k-NN estimate per gene.  cls [N]: class id in [0, n_classes) of every cell,
 *                                -1 for a cell of a class with one cell (dropped); every class in [0, n_classes) has
 *                                >= 2 cells.  n_neighbors in [1, 8], psi [N + 1]: digamma(m) for m = 0..N, cst =
 *                                (psi(n_kept) + mean psi(k_all)) - mean psi(label_counts) computed by the caller.
 *                                mi [n]: the estimates, clipped at 0.  The slot itself is left as it is.
 *   cnmf_preprocess_release      frees the whole staging.
 * Filters over the staged counts (Preprocess.filter_adata, the head of preprocess_for_cnmf; filter_host.hip.h).  A mask is
 * one byte per cell / gene of the staging, non-zero = in; NULL = all.
 *   cnmf_preprocess_upload_csr_as_stored  as cnmf_preprocess_upload_csr for float64 values, but the arrays are staged as they
 *                                are: a row may list its (distinct) columns in any order and zeros (>= 0) may be stored.
 *   cnmf_preprocess_gene_detect  per gene, over the cells of cell_mask: n_cells = stored entries > 0 (a stored zero is no
 *                                detection), totals = the sum of its entries.
 *   cnmf_preprocess_cell_sums    per cell, the sum of its entries whose gene is in gene_mask, in the summation order of
 *                                cnmf_preprocess_row_sums (NULL mask: the same bits).
 *   cnmf_preprocess_subset       the staged counts := their restriction to the kept cells and genes, on the device; the kept
 *                                entries of a row keep their stored order, stored zeros stay.  Both slots and the ridge
 *                                factors are released (they named the old cells and genes).  CNMF_EINVAL when no cell or no
 *                                gene is kept; on any error the staging is left as it was.
 *   cnmf_preprocess_fetch_counts the staged CSR: target_sum > 0: values x * target_sum / row sum (0 for a cell without
 *                                counts; the bits of the normalised copy inside cnmf_preprocess_select), target_sum == 0:
 *                                the raw values.  Any of the three arrays may be NULL (skipped).
 * The device steps of Preprocess.highly_variable_genes (scanpy's flavor='seurat_v3', one batch; hvg_host.hip.h):
 *   cnmf_preprocess_gene_moments per gene of the staging as it is now: s1 = sum x, s2 = sum x^2 as exact integers (at most
 *                                2^22 cells); *flags: bit 0 = some value is negative, non-integer or not finite, bit 1 = some
 *                                count exceeds 2^20 (such entries are left out of the sums: the caller refuses the data).
 *   cnmf_preprocess_loess_fit    the local quadratic fits of loess(degree 2, family gaussian) at m evaluation points x0 over
 *                                the n points (x, y), x SORTED ascending (no staging needed): per point h = the q-th smallest
 *                                |x_i - x0|, tricube weights where |x_i - x0| < h, the weighted least-squares quadratic in
 *                                (x - x0) / h from its normal equations (compensated float64 sums in a fixed order: the same
 *                                bits on every call); value = the fit at x0, slope = its derivative there, status = 0, or
 *                                1 (h <= 0: a zero-width neighbourhood) or 2 (fewer than three distinct weighted abscissae, or
 *                                nearly so: the caller solves that point itself); value = slope = 0 where status != 0.
 *   cnmf_preprocess_clipped_sums per gene of the staging: c1 = sum min(x, clip[g]), c2 = sum min(x, clip[g])^2 (float64,
 *                                fixed order).
 * The same two passes per batch (flavor='seurat_v3' with batch_key; hvg_batch_host.hip.h).  codes [n_cells]: the batch of
 * every staged cell, in [0, n_batches); limits: 1 <= n_batches <= 4096, no batch without a cell, n_genes * n_batches <=
 * 2^26, at most 2^22 cells in all -- CNMF_EINVAL otherwise, before anything is launched.  Both work on a second transpose
 * of the staged counts whose cells are grouped by batch (built on first use, cached for these codes, dropped by release,
 * subset and every upload); the staging itself is not touched.  Results are [n_batches][n_genes], row b over the cells of
 * batch b alone:
 *   cnmf_preprocess_gene_moments_batched  s1, s2 as cnmf_preprocess_gene_moments gives them on the staging restricted to
 *                                the cells of batch b; flags [n_batches]: its flags, per batch.
 *   cnmf_preprocess_clipped_sums_batched  c1, c2 with clip [n_batches][n_genes]: the BITS cnmf_preprocess_clipped_sums
 *                                gives with clip[b] on the staging restricted to the cells of batch b (the same additions
 *                                in the same order). */
int cnmf_preprocess_upload_csr(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                               int data_is_f64, int64_t n_cells, int64_t n_genes);
int cnmf_preprocess_set_dense(cnmf_ctx* ctx, int32_t slot, const double* X, int64_t n_rows, int64_t n_cols);
int cnmf_preprocess_select(cnmf_ctx* ctx, int32_t slot, int32_t n_sel, const int32_t* genes, double target_sum,
                           double max_value, double* std_out /* [n_sel] */, int64_t* nnz_out);
int cnmf_preprocess_order_stats(cnmf_ctx* ctx, int32_t slot, int64_t k, double* lo, double* hi);
int cnmf_preprocess_ceiling(cnmf_ctx* ctx, int32_t slot, double thresh);
int cnmf_preprocess_densify(cnmf_ctx* ctx, int32_t slot);
int cnmf_preprocess_fetch(cnmf_ctx* ctx, int32_t slot, int64_t* indptr, int32_t* indices, double* values);
int cnmf_preprocess_scatter(cnmf_ctx* ctx, int32_t slot, double* mean /* [n] */, double* scatter /* [n][n] */);
int cnmf_preprocess_project(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, const double* mean, const double* V,
                            double* scores /* [n_cells][n_comp] */);
int cnmf_preprocess_ridge_moments(cnmf_ctx* ctx, int32_t slot, int32_t K, int32_t B1, const double* Rt, const double* Phit,
                                  double* M /* [K*B1][n] */, double* gram /* [K*B1][B1] */);
int cnmf_preprocess_ridge_apply(cnmf_ctx* ctx, int32_t slot, const double* W /* [K*B1][n] */);
int cnmf_preprocess_ridge_apply_mode(cnmf_ctx* ctx, int32_t slot, const double* W /* [K*B1][n] */, int32_t clip);
int cnmf_preprocess_row_sums(cnmf_ctx* ctx, double* row_sums /* [n_cells] */);
int cnmf_preprocess_normalize_dense(cnmf_ctx* ctx, int32_t slot, double target_sum, double max_value,
                                    double* std_out /* [n_genes] */);
int cnmf_preprocess_select_mi(cnmf_ctx* ctx, int32_t slot, const int32_t* cls, int32_t n_classes, int32_t n_neighbors,
                              cnmf_mt_state* state, const double* psi, double cst, double* mi /* [n] */);
int cnmf_preprocess_release(cnmf_ctx* ctx);
int cnmf_preprocess_upload_csr_as_stored(cnmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* data,
                                         int64_t n_cells, int64_t n_genes);
int cnmf_preprocess_gene_detect(cnmf_ctx* ctx, const uint8_t* cell_mask /* [n_cells] or NULL */,
                                int64_t* n_cells /* [n_genes] */, double* totals /* [n_genes] */);
int cnmf_preprocess_cell_sums(cnmf_ctx* ctx, const uint8_t* gene_mask /* [n_genes] or NULL */, double* sums /* [n_cells] */);
int cnmf_preprocess_subset(cnmf_ctx* ctx, const uint8_t* keep_cells /* [n_cells] or NULL */,
                           const uint8_t* keep_genes /* [n_genes] or NULL */, int64_t* n_cells_out, int64_t* n_genes_out,
                           int64_t* nnz_out);
int cnmf_preprocess_fetch_counts(cnmf_ctx* ctx, double target_sum, int64_t* indptr, int32_t* indices, double* values);
int cnmf_preprocess_gene_moments(cnmf_ctx* ctx, int64_t* s1 /* [n_genes] */, int64_t* s2 /* [n_genes] */, int32_t* flags);
int cnmf_preprocess_loess_fit(cnmf_ctx* ctx, int64_t n, const double* x /* [n] sorted */, const double* y /* [n] */, int64_t q,
                              int64_t m, const double* x0 /* [m] */, double* value /* [m] */, double* slope /* [m] */,
                              int32_t* status /* [m] */);
int cnmf_preprocess_clipped_sums(cnmf_ctx* ctx, const double* clip /* [n_genes] */, double* c1 /* [n_genes] */,
                                 double* c2 /* [n_genes] */);
int cnmf_preprocess_gene_moments_batched(cnmf_ctx* ctx, const int32_t* codes /* [n_cells] */, int32_t n_batches,
                                         int64_t* s1 /* [n_batches][n_genes] */, int64_t* s2 /* [n_batches][n_genes] */,
                                         int32_t* flags /* [n_batches] */);
int cnmf_preprocess_clipped_sums_batched(cnmf_ctx* ctx, const int32_t* codes /* [n_cells] */, int32_t n_batches,
                                         const double* clip /* [n_batches][n_genes] */, double* c1 /* [n_batches][n_genes] */,
                                         double* c2 /* [n_batches][n_genes] */);

/* ---- the top eigenpairs of a symmetric matrix through its tridiagonal form (pca_host.hip.h) ------------------------------
 * Householder tridiagonalisation on the device (LAPACK's dsytd2 / dlarfg convention, one launch per column), the
 * tridiagonal eigenproblem left to the caller (O(n n_comp) on the host), back-transformation of the kept vectors on the
 * device.  The reflectors of the LAST tridiagonalisation stay staged beside the preprocess slots: the next one replaces
 * them, cnmf_preprocess_release (and every cnmf_preprocess_upload_csr) frees them.  n > CNMF_PCA_NMAX: CNMF_EUNSUPPORTED,
 * before anything is allocated.
 *   cnmf_symmetric_tridiagonalize    A [n][n] symmetric (both triangles; not checked) -> d [n], e [n - 1] (e may be NULL
 *                                    for n = 1) with Q^T A Q = tridiag(e, d, e).
 *   cnmf_tridiagonal_back_transform  V [n][n_comp] = Q Z for Z [n][n_comp], 1 <= n_comp <= n; sign_rule != 0: every column
 *                                    then negated when its entry of largest magnitude (the first on ties) is negative.
 *                                    Nothing staged, or n not the staged one: CNMF_EINVAL.
 *   cnmf_preprocess_pca_tridiag      the same for the scatter matrix of a dense slot, formed as cnmf_preprocess_scatter forms
 *                                    it and left on the device: mean [n] (the bits of cnmf_preprocess_scatter), d, e.
 *   cnmf_preprocess_pca_finish       after cnmf_preprocess_pca_tridiag on the same slot (else CNMF_EINVAL): V = Q Z with the
 *                                    sign rule and scores [n_cells][n_comp] = (X - mean) V, V taken where it is.        */
int cnmf_symmetric_tridiagonalize(cnmf_ctx* ctx, int64_t n, const double* A, double* d /* [n] */, double* e /* [n-1] */);
int cnmf_tridiagonal_back_transform(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* Z /* [n][n_comp] */,
                                    int32_t sign_rule, double* V /* [n][n_comp] */);
int cnmf_preprocess_pca_tridiag(cnmf_ctx* ctx, int32_t slot, double* mean /* [n] */, double* d /* [n] */,
                                double* e /* [n-1] */);
int cnmf_preprocess_pca_finish(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, const double* Z /* [n][n_comp] */,
                               double* V /* [n][n_comp] */, double* scores /* [n_cells][n_comp] */);

/* ---- the tridiagonal eigenproblem on the device as well (tridiag_eig_host.hip.h) ------------------------------------------
 * The n_comp largest eigenpairs of tridiag(e, d, e): multisection on Sturm counts (a wavefront per eigenvalue), inverse
 * iteration (a lane per vector, three iterations), CGS2, and a check of the result on the device; the algorithm is stated
 * in tests/_tridiag_eig_ref.py.  info [4] = {accepted, max |T Z - Z diag(w)| / u_T, max_j |z_j^T T z_j - w_j| / u_T,
 * max |Z^T Z - I| / (n eps)} with u_T = n eps |T|_1; accepted = 1 iff every entry is finite, the residual is within
 * 2 u_T and the orthogonality within 2 n eps, else 0: inverse iteration without orthogonalisation inside fails on some
 * large tight clusters, and then w is valid and the vectors are not.  n > CNMF_PCA_NMAX: CNMF_EUNSUPPORTED before
 * anything is allocated; n_comp outside [1, n] or non-finite d / e (a non-finite A produces them): CNMF_EINVAL.  The
 * orthogonalisation is O(n n_comp^2) on one compute unit: meant for n_comp << n.
 *   cnmf_tridiagonal_eigh_top      the solver alone on a host (d, e): w [n_comp] descending, Z [n][n_comp], CNMF_OK
 *                                  whether accepted or not (info [0]).
 *   cnmf_symmetric_eigh_top        upload, tridiagonalise, solve, back-transform with the sign rule: w, V [n][n_comp].
 *   cnmf_preprocess_pca_device     the PCA of a dense slot (left as it was): mean [n] (the bits of cnmf_preprocess_scatter),
 *                                  w (of the scatter matrix), V, scores [n_cells][n_comp] = (X - mean) V.
 *                                  Both return CNMF_NOT_ACCEPTED (no error: w is written, V and scores are not) when the
 *                                  check fails, with the staging as cnmf_symmetric_tridiagonalize / cnmf_preprocess_pca_tridiag
 *                                  leave it: fetch (d, e) with cnmf_tridiagonal_fetch, solve on the host, and finish
 *                                  through cnmf_tridiagonal_back_transform / cnmf_preprocess_pca_finish.
 *   cnmf_tridiagonal_fetch         d [n], e [n - 1] of the staged tridiagonalisation (none, or another n: CNMF_EINVAL).
 *   cnmf_tridiagonal_eigh_step_ms  out [5]: milliseconds (HIP events) of the last solve's bounds, bisection, inverse
 *                                  iteration and orthogonalisation-plus-check launches and, after
 *                                  cnmf_preprocess_pca_device, of its back-transformation plus scores (else 0).          */
#define CNMF_NOT_ACCEPTED 1
int cnmf_tridiagonal_eigh_top(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* d /* [n] */, const double* e /* [n-1] */,
                              double* w /* [n_comp] */, double* Z /* [n][n_comp] */, double* info /* [4] */);
int cnmf_symmetric_eigh_top(cnmf_ctx* ctx, int64_t n, int32_t n_comp, const double* A /* [n][n] */, double* w /* [n_comp] */,
                            double* V /* [n][n_comp] */, double* info /* [4] */);
int cnmf_preprocess_pca_device(cnmf_ctx* ctx, int32_t slot, int32_t n_comp, double* mean /* [n] */, double* w /* [n_comp] */,
                               double* V /* [n][n_comp] */, double* scores /* [n_cells][n_comp] */, double* info /* [4] */);
int cnmf_tridiagonal_fetch(cnmf_ctx* ctx, int64_t n, double* d /* [n] */, double* e /* [n-1] */);
int cnmf_tridiagonal_eigh_step_ms(const cnmf_ctx* ctx, double* out /* [5] */);

/* ---- Harmony's clustering loop (harmony_host.hip.h) -----------------------------------------------------------------
 * The loop of harmonypy's run_harmony over N cells, d components, K clusters and n_vars batch variables with n_levels
 * levels in all (B): float64, state of its own in the context, fixed summation orders, no float atomics -- two runs give
 * the same bits.  The caller keeps the control flow (Preprocess.run_harmony) and supplies the k-means initialisation and
 * every permutation.  Limits: d <= CNMF_HARMONY_DMAX, K <= CNMF_HARMONY_KMAX, K * (B + 1) <= CNMF_RIDGE_MAX.
 *   cnmf_harmony_begin         pca [N][d] (row-major scores), codes [n_vars][N] (the level, in [0, B), of every cell for every
 *                              variable), level_var [B] (the variable of a level), theta [B], sigma [K] (> 0), pr_b [B].
 *                              Z_cos = the scores of a cell divided by their largest, then by their L2 norm.
 *   cnmf_harmony_init          Y [d][K] (unit centroids): dist = 2 (1 - Y^T Z_cos), R = softmax(-dist / sigma) per cell,
 *                              E = outer(R 1, pr_b), O = R Phi^T; objective[3] = sum R dist, sum sigma R log R (0 where not
 *                              finite), sum sigma R (theta log((O + 1) / (E + 1)) Phi).
 *   cnmf_harmony_kmeans_step   one k-means iteration: Y = Z_cos R^T with unit columns, dist, S = exp(-dist / sigma - max),
 *                              then update_R over the n_blocks blocks np.array_split(perm, n_blocks) in order (E, O without
 *                              the block; R = S ((E + 1) / (O + 1))^theta Phi, every cell divided by its L1 norm; the block
 *                              put back), and the objective.  perm [N]: a permutation of the cells.
 *   cnmf_harmony_ridge_moments M [K*B1][d] and gram [K*B1][B1] of cnmf_preprocess_ridge_moments over Z_orig^T with the
 *                              current R and Phi_moe = [1; Phi] (B1 = B + 1).
 *   cnmf_harmony_ridge_apply   Z_corr = Z_orig - W^T A (not clipped), W [K*B1][d]; Z_cos = Z_corr, every cell at unit L2 norm.
 *   cnmf_harmony_fetch         Z_corr [d][N], Z_cos [d][N], R [K][N], Y [d][K]; any may be NULL.
 *   cnmf_harmony_release       frees the state. */
int cnmf_harmony_begin(cnmf_ctx* ctx, int64_t n_cells, int32_t d, int32_t K, int32_t n_vars, int32_t n_levels,
                       const double* pca, const int32_t* codes, const int32_t* level_var, const double* theta,
                       const double* sigma, const double* pr_b);
int cnmf_harmony_init(cnmf_ctx* ctx, const double* Y /* [d][K] */, double* objective /* [3] */);
int cnmf_harmony_kmeans_step(cnmf_ctx* ctx, const int32_t* perm /* [N] */, int32_t n_blocks, double* objective /* [3] */);
int cnmf_harmony_ridge_moments(cnmf_ctx* ctx, double* M /* [K*B1][d] */, double* gram /* [K*B1][B1] */);
int cnmf_harmony_ridge_apply(cnmf_ctx* ctx, const double* W /* [K*B1][d] */);
int cnmf_harmony_fetch(cnmf_ctx* ctx, double* Z_corr, double* Z_cos, double* R, double* Y);
int cnmf_harmony_release(cnmf_ctx* ctx);

/* ---- Harmony's k-means initialisation (harmony_init_host.hip.h) ---------------------------------------------------
 * scikit-learn's KMeans(n_clusters = K, init = 'k-means++', n_init, max_iter, tol) on the unit scores Z_cos of
 * cnmf_harmony_begin (N cells, d components, K clusters), in float64 on the device, with scikit-learn's steps: centred
 * scores, tol_ = mean variance * tol, k-means++ with L = 2 + int(ln K) local trials per draw, Lloyd with empty clusters
 * moved to the farthest cells, one final E step unless no label changed, the best of n_init by inertia (an init with the
 * same clustering as the best so far does not replace it).  Every sum over cells has a fixed order: the same input gives
 * the same bits.  Needs cnmf_harmony_begin, not cnmf_harmony_init; R, E and O stay as they are.
 *   uniforms   [n_init][1 + (K - 1) L]: per init the doubles numpy's RandomState(random_state) hands KMeans -- one for the
 *              first centre, then L per further centre.  Ignored when centers0 is given.
 *   centers0   NULL, or [n_init][K][d] (in the coordinates of Z_cos): k-means++ is skipped and Lloyd starts there.
 *   Y          [d][K]: cluster_centers_ of the best init (not normalised); labels [N] of the best init, may be NULL;
 *              inertia [n_init], n_iter [n_init], best: the index of the best init.
 * With fewer distinct cells than clusters the centres of the surplus clusters are unspecified.
 * CNMF_EINVAL: n_init outside [1, 16], max_iter < 1, K > N.  CNMF_ESTATE: no cnmf_harmony_begin. */
int cnmf_harmony_kmeans_init(cnmf_ctx* ctx, int32_t n_init, int32_t max_iter, double tol,
                             const double* uniforms, const double* centers0, double* Y, int32_t* labels,
                             double* inertia, int32_t* n_iter, int32_t* best);

/* ---- the restart hot loop ---------------------------------------------------------
 * Replaces the loop body of cNMF.factorize (cnmf.py:735-741): for every restart r,
 *   (usages, spectra, n_iter) = non_negative_factorization(X, n_components=k[r],
 *        init='random'|custom, solver='cd', beta_loss='frobenius', tol, max_iter, ...)
 * i.e. cNMF._nmf (cnmf.py:661-674) -> sklearn:decomposition/_nmf.py:905-1131,
 * _fit_coordinate_descent :406-523, _update_cdnmf_fast sklearn:_cdnmf_fast.pyx:8-38.
 * All restarts share each pass over X.
 *
 *   init_mode 0 (custom): W0 / H0 hold the packed initial factors (what sklearn's
 *       _initialize_nmf :302-314 returns for the restart's seed).
 *   init_mode 1 (random): the library reproduces sklearn's init='random' on the device
 *       from `seeds` (numpy RandomState(seed): MT19937 + legacy polar gauss, H drawn
 *       before W) scaled by avg[r] = sqrt(X.mean()/k[r]); W0/H0 are ignored.
 *   init_mode 2 (init store): the factors cnmf_nndsvd_group left in the context's init store, no
 *       transfer; seeds / avg / W0 / H0 are ignored.  CNMF_EINVAL when the store is empty or does
 *       not hold exactly the ranks k[] of the call on this matrix.
 *
 *   H_out  [sum k][G]   required.   W_out packed [N][k[r]] blocks, may be NULL
 *   (cNMF.factorize drops the usages, cnmf.py:741-745).
 *   n_iter_out[r] = sklearn's n_iter;  viol_out[r] = final violation/violation_init.  */
int cnmf_nmf_cd_batch(cnmf_ctx* ctx, int n_restarts, const int32_t* k,
                      int init_mode, const uint32_t* seeds, const double* avg,
                      const float* W0, const float* H0,
                      const cnmf_cd_params* params,
                      float* H_out, float* W_out,
                      int32_t* n_iter_out, double* viol_out,
                      cnmf_batch_stats* stats);

/* Same, but the spectra stay on the device (for the RCCL gather / on-device consensus):
 * results are appended to the context's spectra store in restart order.               */
int cnmf_nmf_cd_batch_resident(cnmf_ctx* ctx, int n_restarts, const int32_t* k,
                               int init_mode, const uint32_t* seeds, const double* avg,
                               const float* W0, const float* H0,
                               const cnmf_cd_params* params,
                               int32_t* n_iter_out, double* viol_out,
                               cnmf_batch_stats* stats);
/* Queue hints (round 4).  A batch call learns, per rank, the mean number of outer iterations its restarts took
 * (cnmf_get_iteration_means: out[CNMF_KMAX + 1], 0 = rank not seen on this matrix).  Handing such numbers back with
 * cnmf_set_iteration_hints makes the FOLLOWING calls on this matrix start their queue longest-expected-first instead of
 * learning the order again (n = 0 clears the hints; so does a new matrix).  Never implicit: the queue order decides which
 * packed columns a restart occupies, and its float32 result moves in the last bits (1e-6 relative) with its placement --
 * without hints a call's result depends on its own arguments alone (bit for bit; tests/test_gpu_determinism.py). */
int cnmf_get_iteration_means(cnmf_ctx* ctx, double* out);
int cnmf_set_iteration_hints(cnmf_ctx* ctx, int n, const int32_t* k, const double* mean_iterations);

/* ---- multiplicative-update solver --------------------------------------------------------
 * The reference keeps solver='mu' whenever beta_loss != 'frobenius' (cnmf.py:618-631):
 *   non_negative_factorization(X, solver='mu', beta_loss='kullback-leibler'|'itakura-saito', ...)
 *   = sklearn:decomposition/_nmf.py:731-893 (_fit_multiplicative_update), :526-728 (updates),
 *     :84-194 (_beta_divergence, evaluated every 10 iterations for the stopping rule).
 * beta: 1 = kullback-leibler, 0 = itakura-saito.  Same packing / init modes as cnmf_nmf_cd_batch.
 * update_H = 0 is the refit (cnmf.py:776-802 with solver 'mu'): H0 holds the fixed spectra and W
 * starts from avg[r] everywhere (sklearn:_nmf.py:1229-1231); H_out is then ignored.
 * err_out[r] = sqrt(2 * beta-divergence) of the FINAL factors (sklearn's reconstruction_err_).
 * Restarts run batched on the matrix pipe (padded rank 16 / 32 / 64, both losses), up to 32 per round of
 * launches sharing each pass over X (kernels_mu_mfma.hip.h); a restart's result does not depend on the
 * batch it ran in.  Ranks above the context's limit (cnmf_get_mu_rank_limit: CNMF_MU_KMAX = 64 unless raised):
 * CNMF_EUNSUPPORTED.  With the limit raised to CNMF_MU_KMAX_WIDE, ranks 65..128 run as a fourth group at padded rank 128
 * (one restart per workgroup, the same arithmetic); on the vector-ALU route (CNMF_MU_VALU=1, or a matrix beyond 2^24
 * cells or genes) they are CNMF_EUNSUPPORTED before any launch.
 * The first call builds a resident transposed copy of X (freed with the matrix).
 * Kullback-Leibler on the NON-ZEROS (round 4, kernels_mu_sparse.hip.h) -- scikit-learn's own route for scipy.sparse input
 * (sklearn:_nmf.py:192 `_special_sparse_dot`): taken by itself, per group of restarts of one padded rank, when beta = 1,
 * the group's ranks are <= the context's non-zero rank limit (cnmf_get_mu_sparse_rank_limit: CNMF_MU_SPARSE_KMAX = 32
 * unless raised to CNMF_MU_SPARSE_KMAX_WIDE = 64; the other groups of the call run on the dense kernels) and at most
 * a quarter of X (15 % for the padded-rank-64 group) is non-zero (counted once per matrix); same mathematics (the quotient vanishes where X does), exact float32
 * products, another summation order than the dense kernels (results agree to float32 round-off, not bit for bit).
 * Extra device memory: per padded rank in use (16, 32, 64) two blocked sliced-ELL images, 8 B x non-zeros x 1.0-1.2 each
 * (round 5: built from the compressed rows of the matrix, csr_host.hip.h -- no dense transposed copy on this path), and per
 * restart in flight the partial numerators [blocks of the other side][own rows][padded rank] float32.  When those
 * allocations do not fit the call falls back to the dense kernels.  The environment variable CNMF_MU_SPARSE (read when the
 * context is created; 0 = never, 1 = always where the rank allows) overrides the density rule.                       */
/* The largest rank cnmf_nmf_mu_batch and cnmf_mu_refit_f64 accept on this context: CNMF_MU_KMAX (the default) or
 * CNMF_MU_KMAX_WIDE; any other value is CNMF_EINVAL.  Per context, set through this call only (no environment switch). */
int cnmf_set_mu_rank_limit(cnmf_ctx* ctx, int limit);
int cnmf_get_mu_rank_limit(const cnmf_ctx* ctx);
/* The largest rank of a Kullback-Leibler restart that cnmf_nmf_mu_batch may run on the non-zeros: CNMF_MU_SPARSE_KMAX (the
 * default) or CNMF_MU_SPARSE_KMAX_WIDE; any other value is CNMF_EINVAL.  Per context, set through this call only (no
 * environment switch); CNMF_MU_SPARSE and the fall-back to the dense kernels apply as at ranks <= 32; the density rule
 * takes ranks 33..64 to the non-zeros at up to 15 % non-zero (the measured crossover; a quarter at ranks <= 32).         */
int cnmf_set_mu_sparse_rank_limit(cnmf_ctx* ctx, int limit);
int cnmf_get_mu_sparse_rank_limit(const cnmf_ctx* ctx);
int cnmf_nmf_mu_batch(cnmf_ctx* ctx, int n_restarts, const int32_t* k, int init_mode,
                      const uint32_t* seeds, const double* avg, const float* W0, const float* H0,
                      int beta, int update_H, const cnmf_cd_params* params,
                      float* H_out, float* W_out, int32_t* n_iter_out, double* err_out);

/* Multiplicative-update refit in FLOAT64 on the stored entries (round 5, mu_refit_host.hip.h): the three
 *   non_negative_factorization(X, H=..., update_H=False, solver='mu', beta_loss=...)
 * calls of a consensus run with a beta loss (cnmf.py:776-820 via :920, :952, :972) on float64 matrices --
 * scikit-learn's `_fit_multiplicative_update` with H fixed (sklearn:_nmf.py:731-893, :526-631, :84-194).
 *   beta 1: Kullback-Leibler (only the stored entries count, like scikit-learn on scipy.sparse input);
 *   beta 0: Itakura-Saito (round 6).  scikit-learn refuses beta_loss <= 0 on a matrix that contains a zero
 *           (sklearn:_nmf.py:1679-1684), so must the caller's matrix be strictly positive: every entry is then a stored entry
 *           and the same walk is the dense update.  A matrix with a zero: CNMF_EINVAL with scikit-learn's message.
 *   side 0: rows = cells   (refit_usage):   H [k][n_genes],  W_out [n_cells][k]
 *   side 1: rows = GENES   (refit_spectra = the problem on X^T, cnmf.py:820): H = usages^T [k][n_cells], W_out [n_genes][k];
 *           walks the compressed rows of X^T built on the device -- no todense(), no transposed upload.
 * coldiv (NULL ok, [columns of the walked matrix]): x'_ij = x_ij / coldiv[j], coldiv[j] == 0 drops column j -- the final
 *   usage refit on tpm[:, hvgs] / std (cnmf.py:963-972) against the resident full TPM matrix.
 * w_init: W starts from this value everywhere (sklearn:_nmf.py:1229-1231: sqrt(X.mean() / k) of the matrix meant).
 * params: tol, max_iter, l1_reg_W, l2_reg_W.  n_iter_out as scikit-learn counts (a multiple of 10 or max_iter),
 * err_out = sqrt(2 x divergence) of the final factors.  Ranks above the context's limit (cnmf_get_mu_rank_limit):
 * CNMF_EUNSUPPORTED; ranks 65..128 (limit raised) keep the row's factor in LDS and accumulate the components in passes.  */
int cnmf_mu_refit_f64(cnmf_ctx* ctx, int side, int beta, int k, const double* H, const double* coldiv, double w_init,
                      const cnmf_cd_params* params, double* W_out, int32_t* n_iter_out, double* err_out);

/* ---- NNLS refit ---------------------------------------------------------------------
 * Replaces cNMF.refit_usage (cnmf.py:776-802): non_negative_factorization(X, H=spectra,
 * update_H=False, n_components=k, solver='cd', ...) with W0 = 0 (sklearn:_nmf.py:1232-1233).
 * X.Ht is computed once (sklearn recomputes it every outer iteration although H is fixed). */
int cnmf_nnls(cnmf_ctx* ctx, int k, const float* H /*[k][G]*/, const cnmf_cd_params* params,
              float* W_out /*[N][k]*/, int32_t* n_iter_out, double* viol_out);

/* ---- consensus core ---------------------------------------------------------------------
 * Replaces the numerical core of cNMF.consensus (cnmf.py:871-916 + the silhouette of the stats
 * branch, :923), float64 on the device:
 *   l2 = spectra / |spectra|_2 (:882) -> euclidean_distances (:891; sklearn:metrics/pairwise.py:
 *   391-438) -> local density = sum of the n_neighbors+1 smallest per row / n_neighbors (:893-898)
 *   -> keep density < threshold (:903) -> KMeans(k, n_init, random_state=1) on the kept rows
 *   (:908-909; sklearn:cluster/_kmeans.py:1427-1555) -> per-cluster per-gene median (:913) ->
 *   rows / row sum (:916).
 * `uniforms` = the draws KMeans takes from numpy RandomState(random_state):
 *   [n_init][1 + (k-1)*(2+int(log k))] doubles (first centre, then the local trials).
 * Outputs: density_out[R] (NULL ok; zeros when skip_density), keep_out[R] 0/1 (NULL ok),
 *   labels_out[R] (0..k-1, -1 for filtered rows), median_out[k][G], dist_out[R][R] (NULL ok),
 *   stats_out[4] = {rows kept, best inertia, silhouette (0 unless want_silhouette), n_iter of best run}.
 * Returns CNMF_ESTATE with the reference's message when the filter removes every row (:905-906).
 * Device memory: the float64 distance matrix is ALWAYS formed (k-means++ reads its squared distances from it, also with
 * skip_density): 8 R_pad^2 bytes (R_pad = R rounded up to 64: 0.2 GB at R = 5 000, 3.2 GB at R = 20 000) + ~24 R G
 * bytes of spectra copies; a call that leaves more than 2 GB in the context's workspace releases it on return.
 * k-means++ takes the squared distance of two rows as (Euclidean distance)^2 of the UNcentred rows where scikit-learn
 * subtracts the column means first: the same number up to the last bits, so the labels are scikit-learn's except where a
 * draw falls within rounding of a tie. */
typedef struct cnmf_consensus_params {
    int    k;
    int    n_neighbors;        /* int(local_neighborhood_size * R / k), cnmf.py:879 */
    double density_threshold;
    int    skip_density;       /* 1 = skip_density_and_return_after_stats (k_selection_plot)  */
    int    want_silhouette;
    int    n_init;             /* 10 */
    int    max_iter;           /* 300 (sklearn default) */
    double tol;                /* 1e-4 (sklearn default) */
} cnmf_consensus_params;

int cnmf_consensus(cnmf_ctx* ctx, const double* spectra, int R, int G,
                   const cnmf_consensus_params* params, const double* uniforms,
                   double* density_out, int32_t* keep_out, int32_t* labels_out,
                   double* median_out, double* dist_out, double* stats_out);

/* The other two scikit-learn calls of the reference's consensus body, on their own (round 4; INTEGRATION.md Option B
 * binds them): euclidean_distances(rows) (cnmf.py:891, :988) -> dist_out [R][R] (NULL ok), and
 * silhouette_score(rows, labels, metric='euclidean') (cnmf.py:923) -> *silhouette_out (NULL ok; labels [R] in 0..k-1,
 * 2 <= k <= n_samples - 1 as scikit-learn requires).  Float64; the rows are taken AS GIVEN (no normalisation).   */
int cnmf_pairwise_distances(cnmf_ctx* ctx, const double* rows, int R, int G, const int32_t* labels, int k,
                            double* dist_out, double* silhouette_out);

/* sum((X - W.H)^2) over the resident matrix: the prediction error of cnmf.py:926-930
 * (W [N][k], H [k][G], float64).  A matrix that lives as compressed rows only is NOT densified (the reference calls
 * todense() there): sum over the stored entries of (x - wh)^2 - (wh)^2, plus tr(W^T W . H H^T). */
int cnmf_prediction_error(cnmf_ctx* ctx, int k, const double* W, const double* H, double* err_out);

/* ---- products with the resident matrix ----------------------------------------------------
 * out = X . Q (trans = 0: Q [G][ncols] -> out [N][ncols]) or X^T . Q (trans = 1: Q [N][ncols] ->
 * out [G][ncols]), ncols <= 256, through the engine's MFMA GEMM.  This is the only O(N.G) work in
 * sklearn's NNDSVD initialisation (`--init nndsvd`, cnmf.py:1252 -> sklearn:_nmf.py:317 ->
 * sklearn:utils/extmath.py:287-357 `_randomized_range_finder`: 2*n_iter+2 such products); the small
 * LU / QR / SVD factorizations stay on the host (cnmf_amd/engine.py::Engine.nndsvd_init).        */
int cnmf_x_matmul(cnmf_ctx* ctx, int trans, const float* Q, int ncols, float* out);

/* ---- multi-GPU exchange (RCCL over xGMI) ---------------------------------------------------
 * The restarts shard with no collective: ledger row idx runs on rank idx % world, the
 * reference's worker_filter (cnmf.py:52-53).  The reference's "gather" is the filesystem:
 * combine_nmf re-reads one npz per restart (cnmf.py:755-770).  Here it is ONE ncclAllGather of
 * the packed float32 spectra.  One process per GPU, one context per process.  RCCL is bound
 * lazily (dlopen) on the first cnmf_comm_* call; single-GPU use never touches it, and without
 * a communicator the gathers below degenerate to copies (world = 1).
 *
 *   rank 0:     cnmf_comm_unique_id(id)  -> ship the 128 bytes to the other ranks out of band
 *               (a file, an environment variable, MPI, a torch.distributed store ...)
 *   every rank: cnmf_comm_init(ctx, id, rank, world)             (collective: ncclCommInitRank)
 *               cnmf_allgather_bytes(ctx, mine, n, all)          headers / row counts, host buffers
 *               cnmf_allgather_spectra(ctx, local, rows_local, rows_max, G, out)
 *                   local [rows_local][G] host floats, or NULL = the context's resident store
 *                   (cnmf_nmf_cd_batch_resident) -> then the spectra never visit the host before
 *                   the exchange;  out [world][rows_max][G] host floats, shards zero-padded to
 *                   rows_max (= max over ranks, from the header gather).
 *               cnmf_comm_finalize(ctx)                          (also done by cnmf_destroy)      */
#define CNMF_COMM_ID_BYTES 128
int cnmf_comm_unique_id(unsigned char* id_out /* [CNMF_COMM_ID_BYTES] */);
int cnmf_comm_init(cnmf_ctx* ctx, const unsigned char* id /* [CNMF_COMM_ID_BYTES] */, int rank, int world);
int cnmf_comm_finalize(cnmf_ctx* ctx);
int cnmf_comm_rank(const cnmf_ctx* ctx);
int cnmf_comm_world(const cnmf_ctx* ctx);
int cnmf_allgather_bytes(cnmf_ctx* ctx, const void* send, int64_t nbytes, void* recv /* [world][nbytes] */);
int cnmf_allgather_spectra(cnmf_ctx* ctx, const float* local, int64_t rows_local, int64_t rows_max,
                           int64_t n_genes, float* out);
/* the resident spectra store filled by cnmf_nmf_cd_batch_resident (rows in restart order) */
int64_t cnmf_spectra_rows(const cnmf_ctx* ctx);
int cnmf_spectra_reset(cnmf_ctx* ctx);
int cnmf_spectra_fetch(cnmf_ctx* ctx, float* out /* [rows][G] */);
/* rows [row0, row0 + n_rows) of the store: what ONE batch call appended (the store may hold earlier calls' rows too) */
int cnmf_spectra_fetch_rows(cnmf_ctx* ctx, int64_t row0, int64_t n_rows, float* out);
/* gene count of the rows in the store (round 4: the store outlives cnmf_set_matrix -- consensus() alternates between the
 * normalised counts and the TPM matrix while the spectra keep serving k selection and further consensus calls) */
int64_t cnmf_spectra_genes(const cnmf_ctx* ctx);
/* append rows [n_rows][n_genes] (float32) to the store: merged spectra read from the reference's files or gathered from
 * other GPUs, uploaded once for any number of cnmf_consensus_store calls (other k, other density thresholds)         */
int cnmf_spectra_append(cnmf_ctx* ctx, const float* rows, int64_t n_rows, int64_t n_genes);
/* cnmf_consensus / cnmf_kselect_stats with the merged spectra taken from the RESIDENT store instead of a host buffer:
 * store_rows[r] = row of the store holding merged row r (float32 there, widened to float64 on the device) -- what
 * combine_nmf (cnmf.py:748-773) would have concatenated, without the trip through the host.                   */
int cnmf_consensus_store(cnmf_ctx* ctx, const int64_t* store_rows, int R, int G,
                         const cnmf_consensus_params* params, const double* uniforms,
                         double* density_out, int32_t* keep_out, int32_t* labels_out,
                         double* median_out, double* dist_out, double* stats_out);
int cnmf_kselect_stats_store(cnmf_ctx* ctx, int n, const int32_t* ks, const int32_t* R, const int64_t* store_rows,
                             const cnmf_consensus_params* cprm, const double* uniforms, const cnmf_cd_params* prm,
                             double* silhouette_out, double* pred_err_out, double* median_out, int32_t* nnls_iter_out);

/* ---- consensus clustergram (cnmf.py:986-1009, :1028) ------------------------------------------------------------
 * What consensus(show_clustering=True) draws, without the drawing: the distance matrix of the KEPT spectra (labels[r]
 * >= 0), reordered so that every k-means cluster is contiguous (ascending label) and its members stand in the leaf order
 * of an average-linkage dendrogram of the cluster's own distance block.
 *   spectra [R][G] float64 (host) or store_rows [R] into the resident spectra store -- exactly one of them; the kept rows
 *   are L2-normalised and their all-pairs distances computed on the device, as cnmf.py:882 / :988 do;
 *   labels [R]: -1 = filtered out, else the cluster 0..k-1 (a value outside, or a cluster without a member: CNMF_EINVAL);
 *   order_out [Rk]: indices INTO THE KEPT ROWS (cnmf.py:995-1009), seg_out [k+1]: cluster c is order_out[seg[c]..seg[c+1]);
 *   Z_out (NULL ok) [Rk - k][4]: the linkage rows (id, id, height, size) of the clusters in label order, m_c - 1 each;
 *   image_out (NULL ok) [Rk][Rk]: D[order][:, order].
 * The agglomeration is defined by tests/_upgma_ref.py: the closest live pair merges, ties to the smallest first slot and
 * then the smallest second; d(a,t) = (n_a d(a,t) + n_b d(b,t)) / (n_a + n_b) rounded four times; entries < 0 count as 0.
 * With distinct heights this is scipy.cluster.hierarchy.linkage(..., 'average') row for row.  A cluster of more than
 * CNMF_LINKAGE_MAX members: CNMF_EUNSUPPORTED, before anything is launched.                                        */
int cnmf_clustergram(cnmf_ctx* ctx, const double* spectra, const int64_t* store_rows, int R, int G,
                     const int32_t* labels, int k, int32_t* order_out, double* Z_out, int32_t* seg_out,
                     double* image_out);
/* device milliseconds of the last cnmf_clustergram by step (HIP events), out[5]: distances of the kept rows | cluster
 * blocks | agglomeration and leaf order | ordered image | downloads                                                  */
int cnmf_clustergram_step_ms(const cnmf_ctx* ctx, double* out);

/* ---- consensus tail + k selection on the device ------------------------------------------------------------ */
/* out[k][G] (float64) = W^T . X, or W^T . zscore(X) with z = (x - mean[g]) * inv_std[g]: the X^T Y accumulation of
 * efficient_ols_all_cols(normalize_y=True) (cnmf.py:55-125, called at :958) over the RESIDENT matrix (the TPM matrix,
 * dense or uploaded as CSR) in float64 like the reference.  W is [N][k] float64 (k <= CNMF_KMAX).  A matrix that lives as
 * compressed rows only (a CSR upload whose dense image nobody asked for) is walked on its stored entries -- the zeros of
 * a column folded into the constant term; cnmf_col_moments likewise.                                          */
int cnmf_xt_matmul_f64(cnmf_ctx* ctx, int k, const double* W, int zscore, const double* mean,
                       const double* inv_std, double* out);
/* cNMF.refit_spectra (cnmf.py:805-820 = refit_usage(X.T, usage.T).T, sklearn:_nmf.py:1210-1233): NNLS for the
 * spectra H [k][G] with the usages W [N][k] fixed, H from zero, sklearn's CD stopping rule -- on the resident
 * matrix, without uploading its transpose (the constant product is W^T.X).  The solved factor takes sklearn's
 * "W" role: prm->l1_reg_W / l2_reg_W apply to it.  Float64 throughout (round 4: product, Gram, sweeps and result):
 * the reference pins gene_spectra_tpm -- values up to 1e5 TPM units -- to sum(diff^2) < 1e-4
 * (/root/reference/tests/test_reproducibility.py:96-115).                                                   */
int cnmf_nnls_spectra(cnmf_ctx* ctx, int k, const double* W, const cnmf_cd_params* prm, double* H_out,
                      int32_t* n_iter_out, double* viol_out);
/* cNMF.refit_usage (cnmf.py:776-802) in FLOAT64 -- what scikit-learn computes when the reference hands it float64
 * matrices (the consensus tail: rf_usages feed refit_spectra on the TPM matrix).  H [k][G] fixed, W_out [N][k] from
 * zero; the product X.H^T, the Gram matrix and the sweeps (sklearn:_cdnmf_fast.pyx:8-38) in float64 over the resident
 * (float32) matrix.  gram (nullable) [k][k]: used INSTEAD of H.H^T, as in cnmf_nnls_gram below.              */
int cnmf_nnls_f64(cnmf_ctx* ctx, int k, const double* H, const double* gram, const cnmf_cd_params* prm,
                  double* W_out, int32_t* n_iter_out, double* viol_out);
/* non_negative_factorization(X, H=H, update_H=False, solver='mu', beta_loss='frobenius') -- the refit starCAT projects
 * query cells with -- in FLOAT64 over the dense (float32) image of the resident matrix: scikit-learn's
 * _fit_multiplicative_update with beta_loss = 2 (sklearn:_nmf.py:731-893).  H [k][G] fixed, 1 <= k <= CNMF_KMAX
 * (CNMF_EUNSUPPORTED above); W_out [N][k] starts from w_init everywhere (scikit-learn: sqrt(X.mean() / k)).  The product
 * X.H^T, the Gram matrix and sum x^2 are formed once; every iteration is w_t *= P_t / (sum_r w_r Gram[r][t] + l1_reg_W +
 * l2_reg_W w_t) from the row's old values (a zero denominator -> float32 epsilon); the error
 * sqrt(sum x^2 + sum W.(W Gram) - 2 sum P.W) is evaluated at the start and after every 10th iteration when tol > 0 and
 * stops the loop when (previous - error) / error_at_start < tol.  n_iter_out: iterations run; err_out: the last error
 * evaluated.  Sums run in an order fixed by the shapes: two calls give the same bits.                          */
int cnmf_mu2_refit_f64(cnmf_ctx* ctx, int k, const double* H, double w_init, const cnmf_cd_params* prm,
                       double* W_out, int32_t* n_iter_out, double* err_out);
/* cnmf_nnls with a caller-supplied Gram matrix gram[k][k] = H.H^T: the rows H_prod [k][G] only enter the product
 * X.H_prod^T.  Lets the final usage refit of consensus() (cnmf.py:960-975: X = tpm[:, hvgs] / std) run on the
 * resident TPM matrix: H_prod = spectra / std on the HVG columns and 0 elsewhere, gram from the HVG block.    */
int cnmf_nnls_gram(cnmf_ctx* ctx, int k, const float* H_prod, const float* gram, const cnmf_cd_params* prm,
                   float* W_out, int32_t* n_iter_out, double* viol_out);
/* n usage refits (cnmf.py:776-802) with ranks ks[r] and fixed spectra H_r (packed [sum k][G]) as ONE pass over X
 * (all H_r are columns of a single X.H^T product) and joint sweeps.  W_out (nullable): [N][k_r] blocks;
 * err_out (nullable): ||X - W_r.H_r||^2 in float64 (cnmf.py:926-930) with W_r taken from the device.         */
int cnmf_nnls_batch(cnmf_ctx* ctx, int n, const int32_t* ks, const float* H, const cnmf_cd_params* prm,
                    float* W_out, int32_t* n_iter_out, double* viol_out, double* err_out);
/* The statistics loop of k_selection_plot (cnmf.py:1119-1135; per k: the stats branch of consensus, :871-936) in one
 * call: for each of the n values ks[i] the merged spectra (R[i] rows, concatenated in `spectra`) go through the
 * consensus core in stats mode (cprm[i]: skip_density = 1, want_silhouette = 1; `uniforms` = the KMeans draws of
 * every k concatenated), then ALL refits run as one batched cnmf_nnls_batch with the prediction errors.
 * Outputs: silhouette_out[n], pred_err_out[n], median_out (nullable) [sum k][G], nnls_iter_out (nullable) [n]. */
int cnmf_kselect_stats(cnmf_ctx* ctx, int n, const int32_t* ks, const int32_t* R, const double* spectra,
                       const cnmf_consensus_params* cprm, const double* uniforms, const cnmf_cd_params* prm,
                       double* silhouette_out, double* pred_err_out, double* median_out, int32_t* nnls_iter_out);

/* ---- text artefacts (host only, no context) ------------------------------------------------
 * rows x cols FINITE doubles (row-major) as the reference's DataFrame.to_csv(sep) prints them (cnmf.py:34-35): per row the
 * label (row_labels: the labels separated by '\n', labels_bytes bytes; NULL: none) and the values, every value as Python's
 * repr(float), `sep` between the fields, '\n' behind the row.  Returns the bytes written, or -(capacity needed) when `cap`
 * is too small (33 bytes per value + the labels + one separator per row).                                   */
int64_t cnmf_format_rows_f64(const double* vals, int64_t rows, int64_t cols, char sep, const char* row_labels,
                             int64_t labels_bytes, char* out, int64_t cap);

/* The range finder of sklearn's randomized_svd (utils/extmath.py:287-357) -- the O(N G) part of init='nndsvd'
 * (decomposition/_nmf.py:316-354; `--init nndsvd`, cnmf.py:1252) -- for a GROUP of restarts: `nblocks` blocks of
 * widths[b] = k_b + 10 columns side by side (sum <= 256, each <= CNMF_KMAX).  transpose = 0: M = X; 1: M = X^T
 * (sklearn transposes when n_samples < n_features).  Q0 [M_cols][C] row-major: the Gaussian start (host RNG, numpy's
 * stream).  n_iter power iterations, normalised by Cholesky-QR on the device; Q_out [M_rows][C]: orthonormal columns
 * per block, B_out [C][M_cols] = Q^T M.  The small SVD / sign flip / NNDSVD split stay with the caller.           */
int cnmf_range_finder(cnmf_ctx* ctx, int transpose, int nblocks, const int32_t* widths, const float* Q0, int n_iter,
                      float* Q_out, float* B_out);

/* init='nndsvd' / 'nndsvda' / 'nndsvdar' for one GROUP of restarts ENTIRELY on the device (nndsvd_tail_host.hip.h): `nblocks` restarts
 * of ranks k[b] (blocks of k[b] + 10 <= CNMF_KMAX columns, sum <= 256).  The start block of restart b is
 * RandomState(seeds[b]).normal(size=(M_cols, k[b] + 10)) cast to float32, drawn on the device; the range finder is the one
 * of cnmf_range_finder; the small SVD of every B_b is a float64 one-sided Jacobi (at most 30 sweeps); back-transformation,
 * svd_flip, the positive / negative split and the `eps` threshold follow in float64.  variant 0: 'nndsvd'; 1: 'nndsvda'
 * (zeros become x_mean = X.mean()); 2: 'nndsvdar' (zeros become |x_mean z / 100|, z the first normals of a fresh
 * RandomState(seeds[b]), handed out in row-major order of W [N][k], then of H).  The factors are rounded once to float32 and APPENDED to the context's init store
 * (H0 [sum k][G], W0^T [sum k][N]) together with max W0 of every restart; init_mode 2 of the batch calls starts from the
 * store.  status_out[b]: 0 accepted; bit 0: sweep cap hit, bit 1: a value is not finite, bit 2: S_j == 0 for a j < k[b]
 * (a block of rank below k[b]) -- the caller discards the store then.  Same bits on every run.
 * A new or rewritten matrix empties the store. */
int cnmf_nndsvd_group(cnmf_ctx* ctx, int transpose, int nblocks, const int32_t* k, const uint32_t* seeds, int n_iter,
                      int variant, double eps, double x_mean, int32_t* status_out);
/* Empty the init store (its memory stays with the context). */
int cnmf_init_store_reset(cnmf_ctx* ctx);
/* The init store on the host, restart after restart in the packing of the batch calls: W0 packed [N][k_r] blocks,
 * H0 [sum k][G]; *n_out = restarts held.  W0 / H0 may be NULL (only the count); rows_cap: the component rows (sum k) the
 * arrays have room for (CNMF_EINVAL when the store holds more). */
int cnmf_init_store_fetch(cnmf_ctx* ctx, float* W0, float* H0, int64_t rows_cap, int32_t* n_out);
/* (the diagnostic entry points the tests use -- cnmf_debug_* -- are declared in cnmf_hip_debug.h and exist only in a
 * library built with -DCNMF_DEBUG_ABI; they are not part of the drop-in boundary) */

#ifdef __cplusplus
}
#endif
#endif /* CNMF_HIP_H */
