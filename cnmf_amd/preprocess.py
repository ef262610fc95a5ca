"""Host-side mirror of the reference's ``Preprocess`` (src/cnmf/preprocess.py) for the batch-corrected input of
``cNMF.prepare``: ``stdscale_quantile_celing`` (:21-29), ``Preprocess.normalize_batchcorrect`` (:246-360) and
``Preprocess.harmony_correct_X`` (:362-422 with ``moe_correct_ridge``, :9-18).  Same names, argument meanings,
defaults and error texts; every O(N G) step runs on the device (csrc/preprocess_host.hip.h) in float64:

* library-size normalisation, the high-variance-gene subset and ``sc.pp.scale(zero_center=False, max_value)``: one
  upload of the raw counts serves both the normalised copy (for the PCA) and the raw copy (for the correction);
* the global quantile ceiling: the two order statistics around ``h = (N G - 1) q`` come from a radix select over all
  N G entries (implicit zeros of sparse input counted), and numpy interpolates between them
  (``np.quantile([lo, hi], frac)``), so the ceiling is the one ``np.quantile`` gives for the same matrix, bit for bit;
* the PCA of ``sc.pp.pca(zero_center=True)``: min(50, min(N, G) - 1) components; the column means, the G x G covariance
  and the scores ``(X - mean) V`` on the device, ``np.linalg.eigh`` on the host.  Sign rule: the loading of largest
  magnitude of every component is positive (scanpy's sign depends on its solver; Harmony's result does not depend on it).
  Opt-in, ``pca="device"`` on ``normalize_batchcorrect`` and ``preprocess_for_cnmf`` (the default, ``"lapack"``, is the
  route above): the covariance stays on the device and is reduced to tridiagonal form there by Householder reflections
  (csrc/pca_host.hip.h; LAPACK's dsytd2 convention, one launch per column), ``tridiagonal_top`` finds the kept
  eigenpairs of the tridiagonal matrix on the host (``scipy.linalg.eigh_tridiagonal`` by index, 'stebz'), and the
  back-transformation, the sign rule and the scores run on the device: the covariance is never fetched and the loadings
  never uploaded.  At most 8192 genes (``NotImplementedError`` above).  **The yardstick is the float64 numpy restatement
  in tests/_tridiag_ref.py** and gap-free contracts against ``np.linalg.eigh`` (residual and eigenvalues within
  8 n eps |A|_inf, orthogonality within 8 n eps); the loadings of the two routes agree only as far as the eigenvalue
  gaps allow.  ``pca="device_full"`` (named as ``harmony="device_full"`` is) solves the tridiagonal problem on the
  device as well (csrc/tridiag_eig_host.hip.h, ``Engine.preprocess_pca_device``: one library call, only the means, the
  loadings and the scores cross the bus): multisection on Sturm counts, three steps of inverse iteration per vector,
  CGS2; the float64 restatement is tests/_tridiag_eig_ref.py, and the eigenvalues are its bits.  The device checks its
  own result (residual within 2 n eps |T|_1, orthogonality within 2 n eps, all finite), because inverse iteration
  without orthogonalisation inside fails on some large tight clusters; a result that is not accepted is redone by
  ``tridiagonal_top`` (scipy is imported only then), and ``Engine.last_tridiagonal_solver`` says which of the two
  ran.  **Agreement with scanpy's own ``sc.pp.pca`` solver is unmeasured on this project's machines**, for all
  routes;
* Harmony's mixture-of-experts ridge correction: every cluster's ``W_k`` is formed from the uncorrected X (as in the
  reference), so the moments ``M_k = (R_k Phi) X`` and ``Gram_k = (R_k Phi) Phi^T`` of all K clusters come from one
  device pass, ``W_k = inv(Gram_k + lamb) @ M_k`` (``W_k[0] = 0``) runs in numpy, so that ``lamb`` broadcasts exactly as
  in the reference, and ``X - sum_k W_k^T (R_k Phi)`` clipped at 0 is a second device pass.  K (B + 1) is limited to
  4096 (``NotImplementedError`` above).

There is no AnnData here: data moves in the forms ``cNMF.prepare`` accepts (``counts_to_csr``): a DataFrame, an ndarray
or a tuple (scipy.sparse matrix, cell names, gene names); cell metadata is an ``obs`` DataFrame indexed by cell.
``highly_variable`` (a boolean mask or a list of gene names) plays the role of ``var['highly_variable']``; the genes keep
the data's order, as the reference's boolean subset does.  ``harmony_correct_X`` also takes a dense ``X`` (the
reference's ``.todense()`` needs a sparse one) and an optional ``harmony_res`` (any object with ``Z_corr``, ``R``,
``Phi_moe``, ``K`` and ``lamb``) instead of running harmonypy.

``Preprocess.select_features_MI`` (:425-467) ranks the genes by sklearn's ``mutual_info_classif(X, cluster,
n_neighbors=3)``: normalize_total with the median of the positive row sums as the target, the scaling and ceiling above,
then on the device (csrc/select_mi_host.hip.h) sklearn's own scaling and noise -- drawn from numpy's global RandomState,
whose state the call advances exactly as the reference does -- and Ross's k-NN estimate per gene, bit for bit.  The
ranking (``MI``, ``MI_Rank``, ``MI_diff``, ``highly_variable``) uses the reference's own pandas expressions.

``Preprocess.filter_adata`` (:60-132) and ``Preprocess.preprocess_for_cnmf`` (:135-267) stage the counts once and work on
that staging (csrc/filter_host.hip.h): the per-gene detection counts, the per-cell sums over a gene mask (``n_counts``, the
mitochondrial totals), the restriction of the staging to the kept cells and genes (one device pass, the stored order kept)
and the library-size-normalised matrix over all genes (``tp10k``); ``normalize_batchcorrect``'s body then runs on the
staging that is already there.  Counts are integers, so every sum is exact; ``pct_mito`` and the normalised values are one
rounding each: all of it equals the reference bit for bit.

``Preprocess.run_harmony`` is harmonypy's ``run_harmony`` with the clustering loop on the device
(csrc/harmony_host.hip.h), opt-in through ``harmony="device"`` or ``harmony="device_full"`` on ``harmony_correct_X``,
``normalize_batchcorrect`` and ``preprocess_for_cnmf`` (the default, ``"harmonypy"``, calls the library as before;
``harmony_res`` wins over all).  ``"device"`` leaves the k-means initialisation to scikit-learn on the host,
``"device_full"`` (``run_harmony(kmeans_init="device")``) runs it on the device too (csrc/harmony_init_host.hip.h) and
imports neither harmonypy nor scikit-learn.  With
Z = pca^T [d][N], Phi the one-hot levels of the variables in ``pd.get_dummies`` order (B rows), Pr_b their frequencies,
theta and lamb one value per level and sigma per cluster:

* start: Z_cos = Z / max over a cell's scores, then every cell at unit L2 norm; Y = the centres of KMeans(K, k-means++,
  n_init=10, max_iter=25, random_state) on Z_cos^T at unit norm -- **by default this initialisation runs in scikit-learn
  on the host**; with ``kmeans_init="device"`` the same steps (centring, k-means++ from the same RandomState draws, Lloyd
  with relocation of empty clusters, best of 10) run on the device, with fixed-order sums; dist = 2 (1 - Y^T Z_cos);
  R = softmax(-dist / sigma) per cell; E = outer(R 1, Pr_b), O = R Phi^T;
* objective = sum R dist + sum sigma R log R + sum sigma R (theta log((O + 1) / (E + 1)) Phi);
* a round: cluster() -- up to max_iter_kmeans times Y = Z_cos R^T at unit norm, dist, update_R, the objective, and from the
  fifth iteration on a stop when the sums of two overlapping windows of three objectives differ by less than
  epsilon_cluster (relative) -- then the ridge correction of Z with the current R (Z_corr; Z_cos = Z_corr at unit norm),
  and a stop when the objective fell by less than epsilon_harmony (relative);
* update_R: S = exp(-dist / sigma - max); the cells in ``np.random.shuffle`` order, split into ceil(1 / block_size) blocks
  (``np.array_split``); per block: E, O without the block, R = S * (((E + 1) / (O + 1))^theta Phi) at unit L1 norm per
  cell, the block put back.

The device differs from a numpy run in the order of its sums and in the last place of exp / log / pow.  **The yardstick is
the float64 numpy restatement of the above in tests/_harmony_ref.py** (rounds equal; R, Z_corr, Y and the objectives
within 16 x the restatement's distance from its own long double run).  **Agreement with harmonypy itself is unmeasured on
this project's machines**: the library is not installed on them; tests/test_host_harmony.py compares the restatement
with it wherever it can be imported.  The device initialisation is held to oracle/consensus.py's numpy restatement of
scikit-learn's KMeans (tests/test_gpu_harmony_init.py: the best init, its labels and every iteration count equal, the
centres within the rounding of a mean).  With fewer distinct cells than clusters the centres of the surplus clusters are
unspecified: the restatement and scikit-learn disagree there themselves, and no parity is claimed.

``Preprocess.highly_variable_genes`` is scanpy's ``highly_variable_genes(flavor='seurat_v3')``, for one batch (the call
``normalize_batchcorrect(n_top_genes=...)`` makes, :314-315) or per batch with ``batch_key`` (below), opt-in through ``hvg="device"`` together with a number for
``n_top_genes`` / ``n_top_rna_genes`` on ``normalize_batchcorrect`` and ``preprocess_for_cnmf`` (the default,
``hvg=None``, keeps the NotImplementedError for a number).  On the device (csrc/hvg_host.hip.h), over the staging as it
is after ``exclude_genes`` went:

* the per-gene moments S1 = sum x, S2 = sum x^2 as 64-bit integers (counts are non-negative integers: exact in any order);
  mean = S1 / N and var = (N S2 - S1^2) / (N (N - 1)) with the numerator in Python integers and one division;
* the local fits of skmisc's ``loess(x, y, span=0.3, degree=2)`` (family gaussian: no robustness iterations; no
  normalisation in one dimension) over the genes with var > 0, x = log10(mean), y = log10(var), n points,
  q = min(n, floor(n span + 1e-5)).  A local fit at x0: h = the q-th smallest |x_i - x0| (h <= 0: ValueError, skmisc's
  "zero-width neighborhood"); w_i = (1 - (|x_i - x0| / h)^3)^3 where |x_i - x0| < h, else 0; the weighted least-squares
  quadratic in t = (x - x0) / h, minimum-norm with the singular values below 100 eps sigma_max dropped; its value c0 and
  slope c1 / h.  The device finds the neighbourhood by binary search in the sorted abscissae, sums the eight weighted
  moments (compensated float64 sums, a fixed order) and solves the 3 x 3 normal equations; a neighbourhood with fewer
  than three distinct weighted abscissae (or nearly so) comes back flagged and is solved on the host
  (``loess_local_fit_host``).  surface="direct": the fitted value of a gene is the local fit at its own x.
  surface="interpolate" (skmisc's default): local fits at the vertices of ``loess_vertices`` (about 30), a cubic Hermite
  blend between the two vertices of a gene's cell (``loess_hermite``);
* est = 0 on constant genes, the fitted value elsewhere; reg_std = sqrt(10^est); clip = reg_std sqrt(N) + mean; the
  per-gene sums C1 = sum min(x, clip), C2 = sum min(x, clip)^2; variances_norm = (N mean^2 + C2 - 2 C1 mean) /
  ((N - 1) reg_std^2); rank by variances_norm descending, ties in gene order.

**The yardstick is the float64 numpy restatement of the above in tests/_seurat_v3_ref.py** (moments, means and variances
equal bit for bit; the local fits and variances_norm within 16 x the restatement's distance from its own long double run;
the selected set and the ranks equal).  **Agreement with skmisc's loess and with scanpy itself is unmeasured on this
project's machines**: neither library is installed on them; tests/test_host_hvg.py compares the restatement with both
wherever they can be imported.  The vertex rule is written from the published algorithm (Cleveland and Grosse's
dloess); that test is where a mismatch would show.

With ``batch_key`` (``hvg_batch_key`` on ``normalize_batchcorrect`` and ``preprocess_for_cnmf``) the selection is
scanpy's per-batch one (Seurat's SelectIntegrationFeatures).  The batches are the values of ``np.unique`` of the
column, in that order; every batch needs at least two cells and a label for every cell; at most 4096 batches and 2^26
(gene, batch) pairs.  For every batch b with N_b cells the computation above runs on that batch's cells alone --
S1_b, S2_b, mean_b, var_b, the loess over the genes with var_b > 0, reg_std_b, clip_b = reg_std_b sqrt(N_b) + mean_b,
C1_b, C2_b, variances_norm_b.  On the device (csrc/hvg_batch_host.hip.h) the two O(nnz) passes run for all batches at
once over a second transpose of the staged counts whose cells are grouped by batch: the entries of batch b in the
column of gene g are one run, found by binary search, and a wavefront per (gene, batch) pair sums it in the order the
one-batch kernel uses on that batch alone -- the clipped sums have the bits of ``preprocess_clipped_sums`` on the staging
restricted to the batch.  The staging itself keeps its cell order.  The loess fits are one ``preprocess_loess_fit`` call
per batch.  The host combines (``seurat_v3_combine``): a gene's rank in a batch is its position in the stable
descending sort of variances_norm_b (float32, as scanpy holds it); ``highly_variable_nbatches`` counts the batches with
rank < n_top_genes; ``highly_variable_rank`` is the median of those ranks (NaN when there is none); ``variances_norm``
is the mean over the batches; ``means`` and ``variances`` are those of the whole data (S1 = sum_b S1_b, S2 = sum_b S2_b:
the bits of a call without batches); ``highly_variable`` marks the first n_top_genes genes of a stable sort by (rank
ascending with NaN last, nbatches descending), ties in gene order.  With one batch every shared column equals the
one-batch frame.  **Its yardstick is tests/_seurat_v3_batch_ref.py**, the same restatement run per batch with scanpy's
combination written out (moments, means, variances, nbatches, ranks and the selected set equal; variances_norm within
16 x the restatement's distance from its long double run).  **Agreement with scanpy's ``batch_key`` result is unmeasured
on this project's machines**; tests/test_host_hvg_batch.py compares the restatement with it wherever scanpy and skmisc
can be imported.  No time is claimed for the batched passes: they have not been measured against B runs of the one-batch
entry points.

Out of scope: the other flavours of highly_variable_genes, scanpy's ``subset`` and ``inplace``, loess's robustness
iterations and ``degree != 2``, a batched loess entry point, plots (``makeplots`` is accepted and nothing is drawn) and
``.h5ad`` writing.
"""
import numpy as np
import pandas as pd

HARMONY_IMPORT_ERROR = "harmonypy is not installed. Please install it using 'pip install harmonypy' before proceeding."
HVG_REQUIRED_ERROR = ("If a numeric value for n_top_genes is not provided, you must include a highly_variable column "
                      "in _adata")
N_TOP_GENES_ERROR = ("n_top_genes (seurat_v3 HVG selection) needs skmisc's loess, which this package does not use: pass "
                     "highly_variable instead, or opt into this package's own selection on the device with hvg='device'")
ADT_CELL_COUNT_ERROR = "ADT and RNA AnnDatas don't have the same number of cells"
ADT_CELL_INDEX_ERROR = "Inconsistency of the index for the ADT and RNA AnnDatas"
DATA_FORM_ERROR = 'data should either be an AnnData object or a list of 2 AnnData objects'


class PreprocessResult:
    """What the reference's ``normalize_batchcorrect`` returns as an AnnData: ``X`` (cells x HVGs; a dense ndarray after
    Harmony or for dense input, a scipy CSR for sparse input without Harmony), ``obs_names``, ``var_names``, ``obs``
    and ``obsm`` ({'X_pca', 'X_pca_harmony'} when Harmony ran); ``var`` (indexed by ``var_names``) when
    ``select_features_MI`` made it."""

    def __init__(self, X, obs_names, var_names, obs=None, obsm=None, var=None):
        self.X, self.obs_names, self.var_names = X, obs_names, var_names
        self.obs = obs
        self.obsm = obsm if obsm is not None else {}
        self.var = var

    @property
    def shape(self):
        return self.X.shape


def _data_parts(data):
    """(matrix, cell names, gene names, dense?) of a DataFrame, an ndarray or a (matrix, cells, genes) tuple."""
    import scipy.sparse as sp
    if isinstance(data, tuple) and len(data) == 3:
        mat, cells, genes = data
    elif isinstance(data, pd.DataFrame):
        mat, cells, genes = data.values, data.index, data.columns
    else:
        mat = data
        n, g = mat.shape
        cells, genes = ["cell%d" % i for i in range(n)], ["gene%d" % j for j in range(g)]
    dense = not sp.issparse(mat)
    if dense:
        mat = np.asarray(mat)
    if mat.ndim != 2 or mat.shape != (len(cells), len(genes)):
        raise ValueError("matrix of shape %s with %d cell and %d gene names" % (mat.shape, len(cells), len(genes)))
    return mat, pd.Index([str(c) for c in cells]), pd.Index([str(x) for x in genes]), dense


def _to_csr(mat, what="Preprocess"):
    import scipy.sparse as sp
    X = sp.csr_matrix(mat, dtype=np.float64)
    if X.nnz and not (np.isfinite(X.data).all() and (X.data >= 0).all()):
        raise ValueError("%s expects finite non-negative values" % what)
    return X


def _hv_mask(highly_variable, genes):
    """the boolean mask over ``genes`` of a highly_variable mask or list of names"""
    hv = np.asarray(highly_variable)
    if hv.dtype == bool:
        if hv.shape != (len(genes),):
            raise ValueError("highly_variable mask of length %d for %d genes" % (hv.size, len(genes)))
        return hv
    names = pd.Index([str(x) for x in hv])
    unknown = names.difference(genes)
    if len(unknown):
        raise KeyError("highly_variable names not among the genes: %s" % list(unknown[:5]))
    return genes.isin(names)


def make_unique_names(names, join="-"):
    """anndata's ``var_names_make_unique``: the first occurrence of a name keeps it, later ones become ``name-1``,
    ``name-2``, ..., skipping any name that exists already (among the originals or made earlier)."""
    names = [str(x) for x in names]
    out = list(names)
    taken = set(names)
    counter = {}
    seen = set()
    for i, v in enumerate(names):
        if v not in seen:
            seen.add(v)
            continue
        k = counter.get(v, 0) + 1
        new = "%s%s%d" % (v, join, k)
        while new in taken:
            k += 1
            new = "%s%s%d" % (v, join, k)
        counter[v] = k
        taken.add(new)
        out[i] = new
    return pd.Index(out)


def mito_genes_mask(genes):
    """the reference's ``'MT-' in name`` (preprocess.py:109): a substring test, not a prefix test"""
    return np.array(['MT-' in str(x) for x in genes], dtype=bool)


def dot_genes_mask(genes):
    return np.array(['.' in str(x) for x in genes], dtype=bool)


def _is_single_matrix(data):
    import scipy.sparse as sp
    if isinstance(data, tuple):
        return len(data) == 3
    return isinstance(data, (pd.DataFrame, np.ndarray)) or sp.issparse(data)


def quantile_from_order_stats(lo, hi, n, q):
    """``np.quantile`` (method 'linear') of n values whose order statistics floor(h) and floor(h) + 1 are lo and hi,
    h = (n - 1) q: numpy's own interpolation between the two, so the result has the bits np.quantile gives."""
    h = (n - 1) * q
    frac = h - np.floor(h)
    return np.quantile(np.array([lo, hi], dtype=np.float64), frac)


def _check_quantile(q):
    if q is not None and not 0.0 <= q <= 1.0:
        raise ValueError("Quantiles must be in the range [0, 1]")


def _ceiling(eng, slot, n_rows, n_cols, quantile_thresh):
    """the reference's quantile ceiling over all n_rows x n_cols entries of a device slot; returns the threshold"""
    if quantile_thresh is None:
        return None
    total = int(n_rows) * int(n_cols)
    k = int(np.floor((total - 1) * quantile_thresh))
    lo, hi = eng.preprocess_order_stats(slot, min(k, total - 1))
    thresh = quantile_from_order_stats(lo, hi, total, quantile_thresh)
    eng.preprocess_ceiling(slot, thresh)
    return thresh


PCA_MODES = ("lapack", "device", "device_full")
PCA_NMAX = 8192                     # (include/cnmf_hip.h: CNMF_PCA_NMAX)


def _check_pca_mode(pca):
    if pca not in PCA_MODES:
        raise ValueError("pca must be one of %s, not %r" % (PCA_MODES, pca))


def tridiagonal_top(d, e, n_comps):
    """The ``n_comps`` largest eigenvalues of the symmetric tridiagonal matrix with diagonal ``d`` [n] and off-diagonal
    ``e`` [n - 1], descending, and their eigenvectors ``Z`` [n][n_comps]: ``scipy.linalg.eigh_tridiagonal`` by index
    with bisection and inverse iteration ('stebz': its vectors stay orthogonal through clustered eigenvalues), O(n n_comps).
    Host only.  ValueError on non-finite input."""
    from scipy.linalg import eigh_tridiagonal
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    n = d.size
    if d.ndim != 1 or n < 1 or e.shape != (n - 1,):
        raise ValueError("d [n] and e [n - 1] are expected, not shapes %s and %s" % (d.shape, e.shape))
    if not 1 <= n_comps <= n:
        raise ValueError("n_comps = %s outside [1, %d]" % (n_comps, n))
    if not (np.isfinite(d).all() and np.isfinite(e).all()):
        raise ValueError("the tridiagonal matrix holds non-finite values")
    if n == 1:
        return d.copy(), np.ones((1, 1))
    w, Z = eigh_tridiagonal(d, e, select='i', select_range=(n - int(n_comps), n - 1), lapack_driver='stebz')
    return w[::-1].copy(), np.ascontiguousarray(Z[:, ::-1])


def _pca_components(n_rows, n_cols):
    return 50 if 50 < min(n_rows, n_cols) else min(n_rows, n_cols) - 1


def _check_pca_size(pca, n_cols):
    if pca in ("device", "device_full") and n_cols > PCA_NMAX:
        raise NotImplementedError("pca=\"%s\" takes at most %d genes, not %d: use pca=\"lapack\"" % (pca, PCA_NMAX, n_cols))


def _pca(eng, slot, n_rows, n_cols, n_comps=None, pca="lapack"):
    """sc.pp.pca(zero_center=True) of a dense device slot: scores [n_rows][n_comps] (see the module docstring)."""
    if n_comps is None:
        n_comps = _pca_components(n_rows, n_cols)
    if pca == "device":
        _check_pca_size(pca, n_cols)
        _, d, e = eng.preprocess_pca_tridiag(slot)
        _, Z = tridiagonal_top(d, e, n_comps)
        return eng.preprocess_pca_finish(slot, Z)[1]
    if pca == "device_full":                             # (scipy is imported on the fallback alone)
        _check_pca_size(pca, n_cols)
        return eng.preprocess_pca_device(slot, n_comps)[3]
    mean, scatter = eng.preprocess_scatter(slot)
    w, V = np.linalg.eigh(scatter / (n_rows - 1))
    order = np.argsort(-w, kind="stable")[:n_comps]
    V = V[:, order]
    lead = V[np.argmax(np.abs(V), axis=0), np.arange(V.shape[1])]
    V = V * np.where(lead < 0, -1.0, 1.0)
    return eng.preprocess_project(slot, mean, V)


def stdscale_quantile_celing(data, max_value=None, quantile_thresh=None, engine=None, device=0):
    """preprocess.py:21-29 on the device: every column divided by its ddof=1 std (a zero-std column as it is), clipped
    at ``max_value``, then every entry above ``np.quantile(all entries, quantile_thresh)`` (zeros counted) set to that
    value.  ``data``: a dense array (dense result) or a scipy.sparse matrix (CSR result) of non-negative values; the
    reference changes its AnnData in place, this returns the new matrix."""
    import scipy.sparse as sp
    _check_quantile(quantile_thresh)
    dense = not sp.issparse(data)
    X = _to_csr(data)
    N, G = X.shape
    from .engine import Engine
    eng = engine if engine is not None else Engine(device)
    try:
        eng.preprocess_upload(X)
        eng.preprocess_select(0, np.arange(G), 0.0, max_value)
        _ceiling(eng, 0, N, G, quantile_thresh)
        if dense:
            eng.preprocess_densify(0)
        return eng.preprocess_fetch(0)
    finally:
        eng.preprocess_release()
        if engine is None:
            eng.close()


def _harmony_vars_list(harmony_vars):
    return [harmony_vars] if isinstance(harmony_vars, str) else list(harmony_vars)


def _check_harmony_vars(obs, harmony_vars):
    if obs is None:
        raise KeyError("obs is required for harmony_vars %s" % (_harmony_vars_list(harmony_vars),))
    missing = [v for v in _harmony_vars_list(harmony_vars) if v not in obs.columns]
    if missing:
        raise KeyError("harmony_vars %s are not columns of obs" % (missing,))


def _import_harmonypy():
    try:
        import harmonypy
    except Exception:
        raise ImportError(HARMONY_IMPORT_ERROR)
    return harmonypy


HARMONY_MODES = ("harmonypy", "device", "device_full")
KMEANS_INIT_MODES = ("sklearn", "device")
SKLEARN_IMPORT_ERROR = ("run_harmony(kmeans_init='sklearn') needs scikit-learn for its k-means initialisation "
                        "(sklearn.cluster.KMeans on the host); install it, pass init_centroids, or run the initialisation "
                        "on the device: kmeans_init='device' (harmony='device_full')")


def _check_harmony_mode(harmony):
    if harmony not in HARMONY_MODES:
        raise ValueError("harmony must be one of %s, not %r" % (HARMONY_MODES, harmony))


def _check_kmeans_init(kmeans_init):
    if kmeans_init not in KMEANS_INIT_MODES:
        raise ValueError("kmeans_init must be one of %s, not %r" % (KMEANS_INIT_MODES, kmeans_init))


HVG_MODES = (None, "device")
LOESS_SURFACES = ("interpolate", "direct")
HVG_COUNT_MAX = 1 << 20
HVG_CELLS_MAX = 1 << 22
HVG_BATCHES_MAX = 4096
HVG_PAIRS_MAX = 1 << 26
LOESS_ZERO_WIDTH_ERROR = "loess: zero-width neighborhood; make span bigger"
LOESS_RCOND = 100 * float(np.finfo(np.float64).eps)


def _check_hvg_mode(hvg):
    if hvg not in HVG_MODES:
        raise ValueError("hvg must be None or 'device', not %r" % (hvg,))


def _check_batch_key(obs, batch_key):
    if obs is None:
        raise KeyError("obs is required for batch_key %r" % (batch_key,))
    if batch_key not in obs.columns:
        raise KeyError("batch_key %r is not a column of obs" % (batch_key,))


def _check_hvg_batch_key(hvg_batch_key, select, obs):
    """hvg_batch_key goes with hvg='device' and a number only (never ignored); its column must be there"""
    if hvg_batch_key is None:
        return
    if not select:
        raise ValueError("hvg_batch_key is used only with hvg='device' and a number of top genes: without them no "
                         "selection is computed")
    _check_batch_key(obs, hvg_batch_key)


def _check_hvg_args(n_top_genes, span, surface, flavor="seurat_v3"):
    if flavor != "seurat_v3":
        raise NotImplementedError("highly_variable_genes: flavor %r is not implemented (only 'seurat_v3')" % (flavor,))
    if surface not in LOESS_SURFACES:
        raise ValueError("surface must be one of %s, not %r" % (LOESS_SURFACES, surface))
    if isinstance(n_top_genes, bool) or int(n_top_genes) != n_top_genes or n_top_genes < 1:
        raise ValueError("n_top_genes must be a positive integer, not %r" % (n_top_genes,))
    if not 0.0 < span <= 1.0:
        raise ValueError("span must be in (0, 1], not %r" % (span,))


def loess_neighbours(n, span):
    """q of skmisc's loess: the points of a neighbourhood among n"""
    return int(min(n, np.floor(n * span + 1e-5)))


def loess_vertices(xs, span):
    """The vertices of loess's interpolation surface over the SORTED abscissae ``xs`` (Cleveland and Grosse's dloess in
    one dimension): the ends of [min - mu, max + mu], mu = 0.005 max(max - min, 1e-10 max(|min|, |max|) + 1e-30), and
    the cuts of every cell that holds more than fc = floor(n span 0.2) points at (x_(m) + x_(m+1)) / 2, m the middle
    index (l + u) // 2 of the cell's points, moved by +1, -1, +2, ... until x_(m) != x_(m+1); no cut when no such m lies
    inside the cell or x_(m) equals an end of the cell.  Sorted, strictly increasing."""
    n = xs.size
    lo, hi = xs[0], xs[-1]
    mu = 0.005 * max(hi - lo, 1e-10 * max(abs(lo), abs(hi)) + 1e-30)
    fc = int(np.floor(n * span * 0.2))
    cuts, todo = [], [(lo - mu, hi + mu, 0, n - 1)]
    while todo:
        a, b, l, u = todo.pop()
        if u - l + 1 <= fc:
            continue
        m, mid = None, (l + u) // 2
        for k in range(2 * (u - l + 1)):
            c = mid + ((k + 1) // 2 if k % 2 else -(k // 2))      # offsets 0, +1, -1, +2, -2, ...
            if l <= c and c + 1 <= u and xs[c] != xs[c + 1]:
                m = c
                break
        if m is None or xs[m] == a or xs[m] == b:
            continue
        t = (xs[m] + xs[m + 1]) / 2
        cuts.append(t)
        todo += [(a, t, l, m), (t, b, m + 1, u)]
    return np.array(sorted([lo - mu, hi + mu] + cuts), dtype=np.float64)


def loess_local_fit_host(xs, ys, x0, q):
    """One local fit of loess(degree=2) on the host, as the module docstring states it: (value, slope) at x0 from the
    minimum-norm weighted least-squares quadratic over the q nearest points (singular values below 100 eps sigma_max
    dropped).  The device hands the rank-deficient neighbourhoods to this."""
    d = np.abs(xs - x0)
    h = np.partition(d, q - 1)[q - 1]
    if not h > 0:
        raise ValueError(LOESS_ZERO_WIDTH_ERROR)
    use = d < h
    r = d[use] / h
    sw = np.sqrt((1 - r * r * r) ** 3)
    t = (xs[use] - x0) / h
    coef = np.linalg.lstsq(np.stack([sw, sw * t, sw * t * t], axis=1), sw * ys[use], rcond=LOESS_RCOND)[0]
    return coef[0], coef[1] / h


def loess_hermite(v, value, slope, x):
    """the cubic Hermite interpolant through the vertices ``v`` (values, slopes) at the points ``x`` inside them"""
    c = np.clip(np.searchsorted(v, x, side="right") - 1, 0, v.size - 2)
    w = v[c + 1] - v[c]
    u = (x - v[c]) / w
    return ((1 - u) ** 2 * (1 + 2 * u) * value[c] + u ** 2 * (3 - 2 * u) * value[c + 1]
            + (u * (1 - u) ** 2 * slope[c] - u ** 2 * (1 - u) * slope[c + 1]) * w)


def loess_fitted(eng, x, y, span=0.3, surface="interpolate"):
    """The fitted values of skmisc's ``loess(x, y, span=span, degree=2)`` (family gaussian, no robustness iterations)
    at the points themselves, the local fits on the device (``eng.preprocess_loess_fit``): at the vertices of the
    interpolation surface (about 30 of them), or with surface="direct" at every point."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    q = loess_neighbours(x.size, span)
    if q < 1:
        raise ValueError("span = %g leaves no point in a neighbourhood of %d" % (span, x.size))
    at = xs if surface == "direct" else loess_vertices(xs, span)
    value, slope, status = eng.preprocess_loess_fit(xs, ys, q, at)
    if (status == 1).any():
        raise ValueError(LOESS_ZERO_WIDTH_ERROR)
    for i in np.flatnonzero(status != 0):                         # rank-deficient neighbourhoods: the minimum-norm fit
        value[i], slope[i] = loess_local_fit_host(xs, ys, at[i], q)
    fitted = np.empty_like(xs)
    fitted[order] = value if surface == "direct" else loess_hermite(at, value, slope, xs)
    return fitted


def exact_mean_var(s1, s2, N):
    """mean = S1 / N and the ddof=1 variance (N S2 - S1^2) / (N (N - 1)) from the integer sums: the numerator in Python
    integers, one division -- correctly rounded, whatever order the sums were taken in"""
    N = int(N)
    den = N * (N - 1)
    mean = np.array([int(a) / N for a in s1], dtype=np.float64)
    var = np.array([(N * int(b) - int(a) * int(a)) / den for a, b in zip(s1, s2)], dtype=np.float64)
    return mean, var


def _check_hvg_flags(flags):
    if flags & 1:
        raise ValueError("flavor='seurat_v3' expects raw counts: a negative or non-integer value was found")
    if flags & 2:
        raise ValueError("flavor='seurat_v3': a count above %d cannot be summed exactly and is refused" % HVG_COUNT_MAX)


def _regularised_std(eng, mean, var, span, surface):
    """reg_std = sqrt(10^est), est = the loess of log10 var on log10 mean over the genes with var > 0, 0 elsewhere"""
    not_const = var > 0
    est = np.zeros(len(mean))
    if not_const.any():
        est[not_const] = loess_fitted(eng, np.log10(mean[not_const]), np.log10(var[not_const]), span, surface)
    return np.sqrt(10 ** est)


def seurat_v3_combine(vnorm, n_top_genes):
    """The combination rule of scanpy's seurat_v3 with ``batch_key`` (Seurat's SelectIntegrationFeatures) over the
    per-batch ``vnorm`` [B][G].  Returns ``(variances_norm, highly_variable_rank, highly_variable_nbatches,
    highly_variable)`` per gene:

    * the rank of a gene in a batch: its position in the stable descending sort of that batch's row (ties in gene
      order), held as float32 as scanpy holds it; ranks >= n_top_genes count as NaN;
    * highly_variable_nbatches: the batches in which the rank is < n_top_genes;
    * highly_variable_rank: the median of the ranks that are not NaN -- the float32 sum of the two middle ones (the
      middle one twice when their number is odd) halved, as ``np.ma.median`` forms it -- NaN when all are NaN; returned
      as float64 (the value is the same), the dtype of the one-batch frame;
    * variances_norm: the mean over the batches (``np.mean(vnorm, axis=0)``);
    * highly_variable: the first n_top_genes genes of a stable sort by (rank ascending with NaN last, nbatches
      descending), ties in gene order."""
    vnorm = np.asarray(vnorm, dtype=np.float64)
    if vnorm.ndim != 2 or vnorm.shape[0] < 1:
        raise ValueError("vnorm must be [batches][genes], not of shape %s" % (vnorm.shape,))
    B, G = vnorm.shape
    ranks = np.empty((B, G), dtype=np.float32)
    for b in range(B):
        ranks[b, np.argsort(-vnorm[b], kind="stable")] = np.arange(G, dtype=np.float32)
    top = ranks < n_top_genes
    nbatches = top.sum(axis=0).astype(np.int64)
    s = np.sort(np.where(top, ranks, np.float32(np.inf)), axis=0)              # per gene: its ranks, then the dropped ones
    k = np.maximum(nbatches, 1)
    cols = np.arange(G)
    median = ((s[(k - 1) // 2, cols] + s[k // 2, cols]) / np.float32(2)).astype(np.float64)
    median[nbatches == 0] = np.nan
    order = np.lexsort((-nbatches, np.where(nbatches > 0, median, np.inf)))    # (a stable sort: ties in gene order)
    hv = np.zeros(G, dtype=bool)
    hv[order[:int(n_top_genes)]] = True
    return np.mean(vnorm, axis=0), median, nbatches, hv


def batch_codes(obs, batch_key):
    """(codes [N] int32, labels): the batches are the values of ``np.unique(obs[batch_key])``, in that order.  KeyError
    for a missing ``obs`` or column, ValueError for a missing label or a batch with fewer than two cells -- all of it
    before any device work."""
    _check_batch_key(obs, batch_key)
    values = np.asarray(obs[batch_key])
    if pd.isna(values).any():
        raise ValueError("batch_key %r: %d cells have no label (NaN / None)" % (batch_key, int(pd.isna(values).sum())))
    labels, codes = np.unique(values, return_inverse=True)
    sizes = np.bincount(codes.reshape(-1), minlength=len(labels))
    if (sizes < 2).any():
        b = int(np.flatnonzero(sizes < 2)[0])
        raise ValueError("batch_key %r: batch %r has %d cell, flavor='seurat_v3' needs at least 2 per batch"
                         % (batch_key, labels[b], sizes[b]))
    if len(labels) > HVG_BATCHES_MAX:
        raise NotImplementedError("batch_key %r: %d batches, more than the %d supported" % (batch_key, len(labels),
                                                                                          HVG_BATCHES_MAX))
    return codes.reshape(-1).astype(np.int32), labels


def _seurat_v3_frame_batched(eng, N, genes, n_top_genes, span, surface, codes):
    """seurat_v3_frame with ``batch_key``: the one-batch computation per batch over the two batched device passes, the
    batches combined by ``seurat_v3_combine``; means and variances are those of the whole data (the integer moments of
    the batches added up: the bits of a call without batches)"""
    codes = np.asarray(codes)
    sizes = np.bincount(codes)
    B = sizes.size
    if B > HVG_BATCHES_MAX or B * len(genes) > HVG_PAIRS_MAX:
        raise NotImplementedError("%d batches x %d genes: at most %d batches and %d (gene, batch) pairs are supported"
                                  % (B, len(genes), HVG_BATCHES_MAX, HVG_PAIRS_MAX))
    if codes.shape != (N,) or (sizes < 2).any():
        raise ValueError("flavor='seurat_v3' needs one batch code per cell and at least 2 cells in every batch")
    s1, s2, flags = eng.preprocess_gene_moments_batched(codes, B)
    _check_hvg_flags(int(np.bitwise_or.reduce(np.asarray(flags).reshape(-1))))
    mean, var = exact_mean_var(s1.sum(axis=0), s2.sum(axis=0), N)
    G = len(mean)
    mean_b, reg_std, clip = np.empty((B, G)), np.empty((B, G)), np.empty((B, G))
    for b in range(B):
        n = int(sizes[b])
        mean_b[b], var_b = exact_mean_var(s1[b], s2[b], n)
        reg_std[b] = _regularised_std(eng, mean_b[b], var_b, span, surface)
        clip[b] = reg_std[b] * np.sqrt(np.float64(n)) + mean_b[b]
    c1, c2 = eng.preprocess_clipped_sums_batched(codes, B, clip)
    vnorm = np.empty((B, G))
    for b in range(B):
        n = int(sizes[b])
        vnorm[b] = (n * mean_b[b] * mean_b[b] + c2[b] - 2 * c1[b] * mean_b[b]) / ((n - 1) * reg_std[b] * reg_std[b])
    vn, rank, nbatches, hv = seurat_v3_combine(vnorm, n_top_genes)
    return pd.DataFrame({"means": mean, "variances": var, "variances_norm": vn, "highly_variable_rank": rank,
                         "highly_variable": hv, "highly_variable_nbatches": nbatches}, index=pd.Index(genes))


def seurat_v3_frame(eng, N, genes, n_top_genes=2000, span=0.3, surface="interpolate", batch=None):
    """scanpy's ``highly_variable_genes(flavor='seurat_v3')`` frame over the counts ``eng`` has staged (N cells, the genes
    ``genes``): see Preprocess.highly_variable_genes.  ``batch``: None (batch_key=None), or the batch code of every
    staged cell (``batch_codes``): the per-batch route.  The caller uploads and releases."""
    if not 2 <= N <= HVG_CELLS_MAX:
        raise ValueError("flavor='seurat_v3' needs between 2 and %d cells, not %d" % (HVG_CELLS_MAX, N))
    if batch is not None:
        return _seurat_v3_frame_batched(eng, N, genes, n_top_genes, span, surface, batch)
    s1, s2, flags = eng.preprocess_gene_moments()
    _check_hvg_flags(flags)
    mean, var = exact_mean_var(s1, s2, N)
    reg_std = _regularised_std(eng, mean, var, span, surface)
    clip = reg_std * np.sqrt(np.float64(N)) + mean
    c1, c2 = eng.preprocess_clipped_sums(clip)
    vnorm = (N * mean * mean + c2 - 2 * c1 * mean) / ((N - 1) * reg_std * reg_std)
    order = np.argsort(-vnorm, kind="stable")                     # ties in gene order
    rank = np.empty(order.size, dtype=np.float64)
    rank[order] = np.arange(order.size)
    hv = rank < n_top_genes
    rank[~hv] = np.nan
    return pd.DataFrame({"means": mean, "variances": var, "variances_norm": vnorm, "highly_variable_rank": rank,
                         "highly_variable": hv}, index=pd.Index(genes))


class HarmonyResult:
    """What ``Preprocess.run_harmony`` returns, in harmonypy's old layout: ``Z_corr`` [d][N], ``Z_cos`` [d][N], ``R``
    [K][N], ``Y`` [d][K], ``Phi_moe`` [B + 1][N], ``K``, ``lamb`` ((B + 1) x (B + 1) diagonal, first entry 0),
    ``objective_harmony``, ``objective_kmeans`` and ``kmeans_rounds`` (per cluster() call, the index of its last k-means
    iteration, as harmonypy records it)."""


def harmony_nclust(N):
    """harmonypy's default number of clusters: N / 30 rounded half to even, at most 100"""
    return int(min(np.round(N / 30.0), 100))


def harmony_per_level(value, n_levels, what):
    """theta / lamb as one value per level: a scalar is repeated over all levels, one value per variable over its levels"""
    if np.ndim(value) == 0:
        return np.repeat([float(value)] * len(n_levels), n_levels).astype(np.float64)
    value = np.asarray(value, dtype=np.float64).reshape(-1)
    if len(value) == len(n_levels):
        return np.repeat(value, n_levels)
    if len(value) == int(np.sum(n_levels)):
        return value.copy()
    raise ValueError("%s has %d values for %d variables with %d levels" % (what, len(value), len(n_levels), np.sum(n_levels)))


def harmony_design(obs, harmony_vars):
    """The batch design of ``obs[harmony_vars]``: ``(Phi, codes, level_var, n_levels)`` with Phi [B][N] the one-hot matrix
    in ``pd.get_dummies(obs[vars])`` column order, codes [V][N] int32 the row of Phi each cell holds for every variable,
    level_var [B] the variable of every level and n_levels the levels per variable.  A variable that get_dummies does not
    expand (a numeric column) is refused: cast it to str or category."""
    vars_use = _harmony_vars_list(harmony_vars)
    Phi = pd.get_dummies(obs[vars_use]).to_numpy().T.astype(np.float64)
    n_levels = [pd.get_dummies(obs[[v]]).shape[1] for v in vars_use]
    if Phi.shape[0] != int(np.sum(n_levels)):
        raise ValueError("harmony_vars %s do not expand to one column per level" % (vars_use,))
    codes = np.empty((len(vars_use), Phi.shape[1]), dtype=np.int32)
    level_var = np.repeat(np.arange(len(vars_use), dtype=np.int32), n_levels)
    start = 0
    for v, L in enumerate(n_levels):
        block = Phi[start:start + L]
        if not (np.isin(block, (0.0, 1.0)).all() and (block.sum(axis=0) == 1).all()):
            raise ValueError("harmony variable %r is not categorical: every cell needs exactly one level (cast numbers "
                             "to str)" % (vars_use[v],))
        codes[v] = start + np.argmax(block, axis=0)
        start += L
    return Phi, codes, level_var, n_levels


def _host_kmeans_centroids(Z_cos, K, random_state):
    """Harmony's initialisation in scikit-learn on the host (``kmeans_init="sklearn"``): the centres [d][K] of
    KMeans(k-means++, n_init=10, max_iter=25) on the cells' unit scores, exactly the call harmonypy makes.  scikit-learn
    is an optional dependency of this route alone (as harmonypy is of the other one), so it is looked up by name when
    the route runs, never when the package is imported."""
    import importlib
    try:
        cluster = importlib.import_module("sklearn.cluster")
    except Exception:
        raise ImportError(SKLEARN_IMPORT_ERROR)
    model = cluster.KMeans(n_clusters=K, init='k-means++', n_init=10, max_iter=25, random_state=random_state)
    model.fit(Z_cos.T)
    return model.cluster_centers_.T


class Preprocess:
    def __init__(self, random_seed=None, device=0, engine=None):
        """preprocess.py:42-56: ``np.random.seed(random_seed)``.  ``device`` / ``engine``: where the device steps run
        (an engine given here is shared, its resident matrix and spectra store stay as they are); the engine is created
        on first use, so argument errors raise without a GPU."""
        np.random.seed(random_seed)
        self.device = int(device)
        self._engine = engine
        self._own_engine = False

    @property
    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self.device)
            self._own_engine = True
        return self._engine

    def close(self):
        if self._own_engine and self._engine is not None:
            self._engine.close()
        self._engine, self._own_engine = None, False

    # ------------------------------------------------------------------ harmony_correct_X (preprocess.py:362-422)
    def harmony_correct_X(self, X, obs, pca, harmony_vars, theta=1, max_iter_harmony=20, harmony_res=None,
                          harmony="harmonypy"):
        """Runs Harmony on ``pca`` (or takes ``harmony_res``) and applies its mixture-of-experts ridge correction to the
        cells x genes ``X`` (sparse or dense).  Returns ``(X_corr, X_pca_harmony)``: X_corr dense float64, clipped at 0.
        ``harmony``: "harmonypy" (the library's run_harmony), "device" (``self.run_harmony``, harmonypy never imported) or
        "device_full" (``self.run_harmony(kmeans_init="device")``: scikit-learn never imported either)."""
        import scipy.sparse as sp
        _check_harmony_mode(harmony)
        if harmony_res is None:
            harmony_res = self._harmony(pca, obs, harmony_vars, theta, max_iter_harmony, harmony)
        X = X.toarray() if sp.issparse(X) else np.asarray(X)
        X_corr, X_pca_harmony = self._ridge(X, None, pca, harmony_res)
        return X_corr, X_pca_harmony

    def _harmony(self, pca, obs, harmony_vars, theta, max_iter_harmony, harmony):
        """the Harmony result of the chosen route (a missing harmonypy is reported before a missing variable, as ever)"""
        run = _import_harmonypy().run_harmony if harmony == "harmonypy" else self.run_harmony
        _check_harmony_vars(obs, harmony_vars)
        kw = dict(kmeans_init="device") if harmony == "device_full" else {}
        return run(pca, obs, harmony_vars, max_iter_harmony=max_iter_harmony, theta=theta, **kw)

    # ------------------------------------------------------------------ run_harmony (harmonypy's run_harmony, on the device)
    def run_harmony(self, pca, obs, harmony_vars, theta=1, max_iter_harmony=20, *, nclust=None, sigma=0.1, lamb=1,
                    block_size=0.05, max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, random_state=0,
                    init_centroids=None, kmeans_init="sklearn"):
        """Harmony's soft clustering and correction of the PCA scores ``pca`` [N][d] for the batch variables
        ``obs[harmony_vars]``, with harmonypy's argument meanings and defaults (see the module docstring for the
        algorithm).  The clustering loop, the objective and the ridge correction run on the device in float64
        (csrc/harmony_host.hip.h).  The k-means initialisation, KMeans(K, k-means++, n_init=10, max_iter=25,
        random_state) on the unit scores, is skipped when ``init_centroids`` [d][K] is given; otherwise ``kmeans_init``
        says who runs it: "sklearn" (the default: scikit-learn on the host) or "device" (``Engine.harmony_kmeans_init``,
        csrc/harmony_init_host.hip.h: scikit-learn is never imported).  Per k-means iteration the host draws one
        permutation from numpy's global RandomState (seeded with ``random_state`` at the start, as harmonypy does) and
        reads the objective back.  Returns a HarmonyResult, which ``harmony_res=`` of harmony_correct_X /
        normalize_batchcorrect accepts.

        The device loop and the device initialisation give the same bits on every run.  scikit-learn's KMeans does not
        beyond 256 cells (its threads add their partial sums in completion order: the centroids move in the last bit from
        run to run), so with ``kmeans_init="sklearn"`` two calls agree bit for bit when they are given the same
        ``init_centroids``, and to rounding otherwise.  The device initialisation follows scikit-learn step by step from
        the same random draws; it differs in the order of its sums.  With fewer distinct cells than clusters the centres
        of the surplus clusters are unspecified (scikit-learn and its numpy restatement disagree there themselves).

        Limits: K <= 128, d <= 64, K (B + 1) <= 4096 (NotImplementedError above).  ``sigma`` is a scalar."""
        from .engine import Engine
        pca = np.asarray(pca, dtype=np.float64)
        if pca.ndim != 2:
            raise ValueError("pca must be cells x components, not %s" % (pca.shape,))
        _check_harmony_vars(obs, harmony_vars)
        _check_kmeans_init(kmeans_init)
        N, d = pca.shape
        if len(obs) != N:
            raise ValueError("obs has %d rows for %d cells" % (len(obs), N))
        if not np.isfinite(pca).all():
            raise ValueError("pca holds non-finite values")
        if np.ndim(sigma) != 0 or not float(sigma) > 0:
            raise ValueError("sigma must be a positive scalar")
        if not 0 < block_size <= 1:
            raise ValueError("block_size must be in (0, 1]")
        if max_iter_harmony < 0 or max_iter_kmeans < 1:
            raise ValueError("max_iter_harmony >= 0 and max_iter_kmeans >= 1 are required")
        K = int(nclust) if nclust is not None else harmony_nclust(N)
        if K < 1 or (K > N and init_centroids is None):
            raise ValueError("nclust = %d for %d cells (more clusters than cells need init_centroids)" % (K, N))
        Phi, codes, level_var, n_levels = harmony_design(obs, harmony_vars)
        B = Phi.shape[0]
        Engine.harmony_check_limits(d, K, B)
        theta_b = harmony_per_level(theta, n_levels, "theta")
        lamb_mat = np.diag(np.insert(harmony_per_level(lamb, n_levels, "lamb"), 0, 0))
        n_blocks = int(np.ceil(1 / block_size))
        if n_blocks > 4096:
            raise ValueError("block_size = %g gives more than 4096 blocks" % block_size)
        if init_centroids is not None:
            init_centroids = np.asarray(init_centroids, dtype=np.float64)
            if init_centroids.shape != (d, K):
                raise ValueError("init_centroids %s, expected %s" % (init_centroids.shape, (d, K)))
        Pr_b = Phi.sum(axis=1) / N
        np.random.seed(random_state)
        eng = self.engine
        res = HarmonyResult()
        res.K, res.lamb = K, lamb_mat
        res.Phi_moe = np.vstack((np.repeat(1.0, N), Phi))
        res.objective_harmony, res.objective_kmeans, res.kmeans_rounds = [], [], []
        total = lambda terms: terms[0] + terms[1] + terms[2]          # (kmeans error + entropy + cross entropy, in this order)
        try:
            eng.harmony_begin(pca, codes, level_var, theta_b, np.repeat(float(sigma), K), Pr_b)
            if init_centroids is None and kmeans_init == "device":
                Y = eng.harmony_kmeans_init(random_state, n_init=10, max_iter=25)[0]
            elif init_centroids is None:
                Y = _host_kmeans_centroids(eng.harmony_fetch(z_cos_only=True), K, random_state)
            else:
                Y = init_centroids
            Y = Y / np.sqrt((Y * Y).sum(axis=0))
            res.objective_kmeans.append(total(eng.harmony_init(Y)))
            res.objective_harmony.append(res.objective_kmeans[-1])
            for _ in range(max_iter_harmony):
                # cluster()
                i = -1
                for i in range(max_iter_kmeans):
                    order = np.arange(N)
                    np.random.shuffle(order)
                    res.objective_kmeans.append(total(eng.harmony_kmeans_step(order, n_blocks)))
                    if i > 3:
                        o = res.objective_kmeans
                        old, new = o[-2] + o[-3] + o[-4], o[-1] + o[-2] + o[-3]
                        if abs(old - new) / abs(old) < epsilon_cluster:
                            break
                res.kmeans_rounds.append(i)
                res.objective_harmony.append(res.objective_kmeans[-1])
                # moe_correct_ridge on Z_orig with the current R
                M, gram = eng.harmony_ridge_moments()
                W = np.empty_like(M)
                for k in range(K):
                    W[k] = np.linalg.inv(gram[k] + lamb_mat) @ M[k]
                    W[k][0, :] = 0
                eng.harmony_ridge_apply(W)
                old, new = res.objective_harmony[-2], res.objective_harmony[-1]
                if (old - new) / abs(old) < epsilon_harmony:
                    break
            res.Z_corr, res.Z_cos, res.R, res.Y = eng.harmony_fetch()
        finally:
            eng.harmony_release()
        return res

    def _ridge(self, X, slot, pca, harmony_res):
        """moe_correct_ridge on the device over X (uploaded to slot 1) or over the dense device slot ``slot``."""
        Z_corr = np.asarray(harmony_res.Z_corr)
        R = np.asarray(harmony_res.R, dtype=np.float64)
        Phi = np.asarray(harmony_res.Phi_moe, dtype=np.float64)
        new_harmony = Z_corr.shape[0] == np.asarray(pca).shape[0]      # (preprocess.py:405-414)
        if new_harmony:
            X_pca_harmony, R, Phi = Z_corr, R.T, Phi.T
        else:
            X_pca_harmony = Z_corr.T
        K = int(harmony_res.K)
        R = R[:K]                                                     # (the reference's loop reads rows 0..K-1)
        lamb = harmony_res.lamb
        eng = self.engine
        try:
            if slot is None:
                slot = 1
                eng.preprocess_release()
                eng.preprocess_set_dense(slot, X)
            N = eng._pre["N"]
            if R.shape != (K, N) or Phi.ndim != 2 or Phi.shape[1] != N:
                raise ValueError("Harmony's R %s / Phi_moe %s do not match %d cells" % (R.shape, Phi.shape, N))
            M, gram = eng.preprocess_ridge_moments(slot, R, Phi)
            W = np.empty_like(M)
            for k in range(K):
                W[k] = np.linalg.inv(gram[k] + lamb) @ M[k]
                W[k][0, :] = 0                                        # do not remove the intercept
            eng.preprocess_ridge_apply(slot, W)
            X_corr = eng.preprocess_fetch(slot)
        finally:
            eng.preprocess_release()
        return X_corr, X_pca_harmony

    # ------------------------------------------------------------------ normalize_batchcorrect (preprocess.py:246-360)
    def normalize_batchcorrect(self, data, obs=None, highly_variable=None, normalize_librarysize=False, harmony_vars=None,
                               n_top_genes=None, librarysize_targetsum=1e4, max_scaled_thresh=None, quantile_thresh=.9999,
                               theta=1, makeplots=True, max_iter_harmony=20, harmony_res=None, harmony="harmonypy",
                               hvg=None, hvg_batch_key=None, pca="lapack"):
        """Normalises the high-variance genes of raw counts and optionally corrects them with Harmony.  Returns
        ``(result, hvgs)``: ``result.X`` goes straight into ``cNMF.prepare(counts=(result.X, result.obs_names, hvgs),
        ...)``.  ``harmony``: who runs Harmony when ``harmony_res`` is not given: "harmonypy" (the library), "device"
        (``self.run_harmony``) or "device_full" (``self.run_harmony(kmeans_init="device")``).

        ``hvg``: None (the default: a number for ``n_top_genes`` raises NotImplementedError and ``highly_variable`` is
        required) or "device": a number for ``n_top_genes`` then runs ``highly_variable_genes`` (seurat_v3) on the
        staged counts and its selection replaces ``highly_variable``, as the reference overwrites
        ``var['highly_variable']``; the frame, restricted to the selected genes, is ``result.var``.
        ``hvg_batch_key``: a column of ``obs``; that selection is then made per batch and the ranks combined
        (``highly_variable_genes(batch_key=...)``; ``result.var`` carries ``highly_variable_nbatches``).  Given without
        ``hvg="device"`` and a number it raises ValueError.

        ``pca``: who solves the PCA's eigenproblem in the Harmony branch: "lapack" (the default: the gene covariance is
        fetched and ``np.linalg.eigh`` finds all its eigenpairs on the host) or "device" (Householder tridiagonalisation
        on the device, the tridiagonal problem for the kept components on the host, back-transformation and scores on
        the device; at most 8192 selected genes, NotImplementedError above) or "device_full" (the tridiagonal problem
        on the device too, with the host solve as the fallback for a result the device's check does not accept; the same
        limit).  Anything else raises ValueError."""
        _check_pca_mode(pca)
        _check_hvg_mode(hvg)
        _check_hvg_batch_key(hvg_batch_key, hvg == "device" and n_top_genes is not None, obs)
        if n_top_genes is not None and hvg is None:
            raise NotImplementedError(N_TOP_GENES_ERROR)
        select = n_top_genes is not None
        if select:
            _check_hvg_args(n_top_genes, 0.3, "interpolate")
        elif highly_variable is None:
            raise Exception(HVG_REQUIRED_ERROR)
        _check_quantile(quantile_thresh)
        _check_harmony_mode(harmony)
        if harmony_vars is not None:
            if harmony_res is None and harmony == "harmonypy":
                _import_harmonypy()
            _check_harmony_vars(obs, harmony_vars)
        mat, cells, genes, dense = _data_parts(data)
        if not select:
            sel = np.flatnonzero(_hv_mask(highly_variable, genes))
            if sel.size == 0:
                raise ValueError("highly_variable selects no gene")
        if obs is not None:
            obs = _align_obs(obs, cells)
        batch = None if hvg_batch_key is None else batch_codes(obs, hvg_batch_key)[0]
        X = _to_csr(mat)
        var = None
        eng = self.engine
        try:
            eng.preprocess_upload(X)
            if select:
                var = seurat_v3_frame(eng, X.shape[0], genes, n_top_genes, batch=batch)
                sel = np.flatnonzero(var["highly_variable"].values)
                var = var.iloc[sel]
            Xout, obsm = self._batchcorrect_staged(eng, X.shape[0], sel, dense, obs, normalize_librarysize, harmony_vars,
                                                   librarysize_targetsum, max_scaled_thresh, quantile_thresh, theta,
                                                   max_iter_harmony, harmony_res, harmony, pca)
        finally:
            eng.preprocess_release()
        hvgs = list(genes[sel])
        return PreprocessResult(Xout, cells, pd.Index(hvgs), obs, obsm, var=var), hvgs

    # ------------------------------------------------------------------ highly_variable_genes (scanpy, flavor='seurat_v3')
    def highly_variable_genes(self, data, n_top_genes=2000, span=0.3, surface="interpolate", flavor="seurat_v3",
                              batch_key=None, obs=None):
        """scanpy's ``sc.pp.highly_variable_genes(flavor='seurat_v3', n_top_genes, span, batch_key)`` (without
        ``batch_key`` the call the reference makes, preprocess.py:314-315), over raw counts in any of the forms
        ``data`` takes.  Returns scanpy's
        frame, indexed by gene in the data's order: ``means``, ``variances`` (ddof=1), ``variances_norm``,
        ``highly_variable_rank`` (float; NaN from ``n_top_genes`` on) and ``highly_variable``.

        The two O(nnz) passes (per-gene integer moments; per-gene sums of the counts clipped at
        ``reg_std sqrt(N) + mean``) and the local fits of the loess of log10(variance) on log10(mean) run on the device;
        the sort of the abscissae, the vertices, the Hermite blend, the few rank-deficient fits and the ranking run on
        the host (module docstring).  ``surface``: "interpolate" (skmisc's default: local fits at about 30 vertices, a
        cubic Hermite blend between them) or "direct" (a local fit at every gene); the two differ by up to about 5e-3 in
        log10 variance and by a gene or two in the selected set.  Ties of ``variances_norm`` are ranked in gene order (a
        stable sort; scanpy's own ``np.argsort`` leaves them unspecified).  Two calls on the same input give the same
        bits.

        Deliberate difference from scanpy, which warns on non-integer data and goes on: a negative or non-integer value
        raises ValueError, and so does a count above 2^20 or more than 2^22 cells (the bound under which the integer
        sums stay exact; nothing is ever wrapped).  Any other ``flavor`` raises NotImplementedError.

        ``batch_key``: a column of ``obs`` (a DataFrame over the cells, aligned by name or by position); ``obs`` is not
        read without it.  The batches are the values of ``np.unique`` of that column.  The computation above then runs
        on every batch's cells alone -- the two O(nnz) passes for all batches at once, over a second transpose of the
        staged counts whose cells are grouped by batch; one loess per batch -- and the batches are combined as scanpy
        combines them (``seurat_v3_combine``): ``highly_variable_rank`` is the median over the batches of a gene's ranks
        below ``n_top_genes``, ``variances_norm`` the mean over the batches, ``highly_variable`` the first
        ``n_top_genes`` genes by (rank ascending, NaN last; ``highly_variable_nbatches`` descending; gene order), and
        the frame gains the int column ``highly_variable_nbatches``.  ``means`` and ``variances`` are those of the
        whole data, with the bits of a call without ``batch_key``.  KeyError for a missing ``obs`` or column,
        ValueError for a missing label (NaN / None) or a batch with fewer than 2 cells, NotImplementedError for more
        than 4096 batches, all before any device work; more than 2^26 (gene, batch) pairs raise NotImplementedError
        before the first batched pass; the count and span errors arise per batch."""
        _check_hvg_args(n_top_genes, span, surface, flavor)
        if batch_key is not None:
            _check_batch_key(obs, batch_key)
        mat, cells, genes, dense = _data_parts(data)
        batch = None if batch_key is None else batch_codes(_align_obs(obs, cells), batch_key)[0]
        X = _to_csr(mat, what="flavor='seurat_v3'")
        eng = self.engine
        try:
            eng.preprocess_upload(X)
            return seurat_v3_frame(eng, X.shape[0], genes, n_top_genes, span, surface, batch)
        finally:
            eng.preprocess_release()

    def _batchcorrect_staged(self, eng, N, sel, dense, obs, normalize_librarysize, harmony_vars, librarysize_targetsum,
                             max_scaled_thresh, quantile_thresh, theta, max_iter_harmony, harmony_res,
                             harmony="harmonypy", pca="lapack"):
        """normalize_batchcorrect (preprocess.py:314-358) over the counts ``eng`` has staged (N cells), for the staged
        genes ``sel``: returns ``(X, obsm)``.  The caller uploads and releases."""
        n = int(sel.size)
        obsm = {}
        if harmony_vars is not None:
            _check_pca_size(pca, n)
            # anorm: normalize_total(copy=True) -> HVG subset -> scale + ceiling (preprocess.py:316-318)
            eng.preprocess_select(0, sel, float(librarysize_targetsum), max_scaled_thresh)
            _ceiling(eng, 0, N, n, quantile_thresh)
            # _adata: raw counts -> HVG subset -> scale + ceiling (:320-321)
            if not normalize_librarysize:
                eng.preprocess_select(1, sel, 0.0, max_scaled_thresh)
                _ceiling(eng, 1, N, n, quantile_thresh)
            eng.preprocess_densify(0)
            obsm["X_pca"] = _pca(eng, 0, N, n, pca=pca)            # (:326)
            slot = 0 if normalize_librarysize else 1
            eng.preprocess_densify(slot)
            if harmony_res is None:
                harmony_res = self._harmony(obsm["X_pca"], obs, harmony_vars, theta, max_iter_harmony, harmony)
            Xout, obsm["X_pca_harmony"] = self._ridge(None, slot, obsm["X_pca"], harmony_res)
        else:
            target = float(librarysize_targetsum) if normalize_librarysize else 0.0
            eng.preprocess_select(0, sel, target, max_scaled_thresh)
            _ceiling(eng, 0, N, n, quantile_thresh)
            if dense:
                eng.preprocess_densify(0)
            Xout = eng.preprocess_fetch(0)
        return Xout, obsm

    # ------------------------------------------------------------------ filter_adata (preprocess.py:60-132)
    def filter_adata(self, data, obs=None, filter_mito_thresh=None, min_cells_per_gene=10, min_counts_per_cell=500,
                     filter_mito_genes=False, filter_dot_genes=True, makeplots=True):
        """The reference's optional filter, in its order: genes detected (value > 0) in at least ``min_cells_per_gene``
        cells; ``n_counts`` = every cell's sum over those genes; cells with ``n_counts >= min_counts_per_cell``;
        ``pct_mito`` = the share of the genes whose name contains ``'MT-'`` and cells with ``pct_mito <
        filter_mito_thresh`` (a cell without counts has NaN and goes); then the genes containing ``'.'``
        (``filter_dot_genes``) and the mitochondrial genes (``filter_mito_genes``) are dropped.  Genes are not filtered
        again after cells went, as in the reference.  The counts are staged once, the sums and the one restriction to
        the kept cells and genes run on the device.

        Returns a PreprocessResult: ``X`` the raw filtered counts (float64; CSR for sparse input, dense for dense
        input), ``obs_names``, ``var_names``, ``obs`` (the given columns plus ``n_counts`` and, with a threshold,
        ``pct_mito``) and ``var`` with ``n_cells`` (the detection counts over all cells of the input; the reference has
        this column only when ``min_cells_per_gene`` is given).  A filter that leaves no cell or no gene raises
        ValueError.  The reference's ``ax.title(...)`` defect (plots with a threshold) is not reproduced."""
        mat, cells, genes, dense = _data_parts(data)
        obs = pd.DataFrame(index=cells) if obs is None else _align_obs(obs, cells).copy()
        X = _to_csr(mat)
        mt = mito_genes_mask(genes)
        eng = self.engine
        try:
            eng.preprocess_upload(X)
            n_cells, _ = eng.preprocess_gene_detect()
            keep_g = n_cells >= min_cells_per_gene if min_cells_per_gene is not None else np.ones(len(genes), dtype=bool)
            if not keep_g.any():
                raise ValueError("min_cells_per_gene = %s leaves no gene" % (min_cells_per_gene,))
            n_counts = eng.preprocess_cell_sums(None if keep_g.all() else keep_g)
            keep_c = n_counts >= min_counts_per_cell if min_counts_per_cell is not None else np.ones(len(cells), dtype=bool)
            if not keep_c.any():
                raise ValueError("min_counts_per_cell = %s leaves no cell" % (min_counts_per_cell,))
            obs["n_counts"] = n_counts
            mt_kept = mt & keep_g
            if filter_mito_thresh is not None:
                num_mito = eng.preprocess_cell_sums(mt_kept)
                with np.errstate(invalid="ignore", divide="ignore"):
                    pct_mito = num_mito / n_counts
                obs["pct_mito"] = pct_mito
                keep_c = keep_c & (pct_mito < filter_mito_thresh)
                if not keep_c.any():
                    raise ValueError("filter_mito_thresh = %s leaves no cell" % (filter_mito_thresh,))
            drop = np.zeros(len(genes), dtype=bool)
            if filter_dot_genes:
                drop |= dot_genes_mask(genes)
            if filter_mito_genes:
                drop |= mt_kept
            keep_g = keep_g & ~drop
            if not keep_g.any():
                raise ValueError("the gene filters leave no gene")
            eng.preprocess_subset(None if keep_c.all() else keep_c, None if keep_g.all() else keep_g)
            Xout = eng.preprocess_fetch_counts(0.0)
        finally:
            eng.preprocess_release()
        if dense:
            Xout = Xout.toarray()
        var = pd.DataFrame({"n_cells": n_cells[keep_g]}, index=genes[keep_g])
        return PreprocessResult(Xout, cells[keep_c], genes[keep_g], obs.loc[keep_c], var=var)

    # ------------------------------------------------------------------ preprocess_for_cnmf (preprocess.py:135-267)
    def preprocess_for_cnmf(self, data, obs=None, highly_variable=None, feature_type=None,
                            adt_feature_name='Antibody Capture', harmony_vars=None, n_top_rna_genes=None,
                            librarysize_targetsum=1e4, max_scaled_thresh=None, quantile_thresh=.9999, makeplots=True,
                            theta=1, save_output_base=None, max_iter_harmony=20, exclude_genes=None, harmony_res=None,
                            harmony="harmonypy", hvg=None, hvg_batch_key=None, pca="lapack"):
        """The reference's minimal preprocessing: the HVG-filtered, variance-normalised, optionally Harmony-corrected RNA
        matrix (the ``counts`` input of cNMF) and the library-size-normalised matrix over all genes, ADT features
        appended and normalised on their own (the ``tpm`` input).

        ``data``: one matrix (RNA only, or RNA and ADT told apart by ``feature_type``: an array-like over the genes, or
        a Series indexed by gene, that plays ``var[feature_type_col]``; ``== adt_feature_name`` is ADT) or a list
        ``[rna, adt]`` over the same cells.  A single-modality input gets anndata's ``var_names_make_unique``.

        Deliberate difference from the reference: ``n_top_rna_genes`` defaults to None (the reference: 2000) and
        ``highly_variable`` -- a boolean mask or a list of names over the RNA genes -- takes its place: the seurat_v3
        selection is opt-in.  With ``hvg=None`` (the default) a number raises normalize_batchcorrect's
        NotImplementedError, and None without ``highly_variable`` the reference's "you must include a highly_variable
        column".  With ``hvg="device"`` a number runs ``highly_variable_genes`` (seurat_v3; its yardstick is this
        project's restatement of skmisc's loess, see the module docstring) on the staged RNA counts after
        ``exclude_genes`` went, as the reference does: an excluded gene or an ADT feature is never selected, and the
        selection replaces ``highly_variable``.  The frame of the selected genes is ``result_rna.var``.
        ``hvg_batch_key`` (a column of ``obs``) makes that selection per batch, as in normalize_batchcorrect; given
        without ``hvg="device"`` and a number it raises ValueError.  ``pca``: "lapack" (the default), "device" or
        "device_full", as in normalize_batchcorrect.

        The RNA counts are uploaded once: ``tp10k`` comes from them over all RNA genes before ``exclude_genes`` are taken
        out (on the device), then normalize_batchcorrect's body runs on the same staging.

        Returns ``(result_rna, tp10k, hvgs)``, both PreprocessResult.  ``save_output_base``: ``<base>.Corrected.HVGs.txt``
        as the reference writes it; there is no ``.h5ad`` here: ``<base>.Corrected.HVG.Varnorm`` and ``<base>.TP10K``
        are ``.df.npz`` files (save_df_to_npz) when dense, ``.npz`` (save_csr_fast) plus ``.cells.txt`` / ``.genes.txt``
        when sparse."""
        import scipy.sparse as sp
        if isinstance(data, list) and len(data) == 2:
            rna, adt = data
        elif _is_single_matrix(data):
            rna, adt = data, None
        else:
            raise Exception(DATA_FORM_ERROR)
        _check_pca_mode(pca)
        _check_hvg_mode(hvg)
        _check_hvg_batch_key(hvg_batch_key, hvg == "device" and n_top_rna_genes is not None, obs)
        if n_top_rna_genes is not None and hvg is None:
            raise NotImplementedError(N_TOP_GENES_ERROR)
        select = n_top_rna_genes is not None
        if select:
            _check_hvg_args(n_top_rna_genes, 0.3, "interpolate")
        elif highly_variable is None:
            raise Exception(HVG_REQUIRED_ERROR)
        _check_quantile(quantile_thresh)
        _check_harmony_mode(harmony)
        if harmony_vars is not None:
            if harmony_res is None and harmony == "harmonypy":
                _import_harmonypy()
            _check_harmony_vars(obs, harmony_vars)
        mat, cells, genes, dense = _data_parts(rna)
        types_rna = types_adt = None
        hv = None if select else np.asarray(highly_variable)
        if adt is not None:
            amat, acells, agenes, _ = _data_parts(adt)
            if amat.shape[0] != mat.shape[0]:
                raise Exception(ADT_CELL_COUNT_ERROR)
            if np.sum(np.asarray(acells) != np.asarray(cells)) > 0:
                raise Exception(ADT_CELL_INDEX_ERROR)
        elif feature_type is not None:
            if isinstance(feature_type, pd.Series):
                ft = feature_type.copy()
                ft.index = [str(x) for x in ft.index]
                ft = ft.reindex(genes) if not ft.index.equals(genes) and ft.index.is_unique else ft
            else:
                ft = pd.Series(np.asarray(feature_type))
            if len(ft) != len(genes):
                raise ValueError("feature_type has %d entries for %d genes" % (len(ft), len(genes)))
            is_adt = np.asarray(ft.values == adt_feature_name)
            ft = np.asarray(ft.values)
            X_all = sp.csr_matrix(mat) if not dense else mat
            amat, agenes, types_adt = X_all[:, np.flatnonzero(is_adt)], genes[is_adt], ft[is_adt]
            if not select and hv.dtype == bool and hv.shape == (len(genes),) and is_adt.any():
                hv = hv[~is_adt]                                  # (a var['highly_variable'] column over all features)
            mat, genes, types_rna = X_all[:, np.flatnonzero(~is_adt)], genes[~is_adt], ft[~is_adt]
            adt = (amat, cells, agenes)
        else:
            genes = make_unique_names(genes)
        excluded = np.zeros(len(genes), dtype=bool)
        if exclude_genes is not None:
            excluded = np.asarray(genes.isin([str(x) for x in exclude_genes]))
        if not select:
            sel = np.flatnonzero(_hv_mask(hv, genes)[~excluded])
            if sel.size == 0:
                raise ValueError("highly_variable selects no gene")
        if excluded.all():
            raise ValueError("exclude_genes leaves no gene")
        if obs is not None:
            obs = _align_obs(obs, cells)
        batch = None if hvg_batch_key is None else batch_codes(obs, hvg_batch_key)[0]
        X = _to_csr(mat)
        Xa = _to_csr(adt[0]) if adt is not None else None
        target = float(librarysize_targetsum)
        hvg_var = None
        eng = self.engine
        try:
            eng.preprocess_upload(X)
            tp10k = eng.preprocess_fetch_counts(target)             # over ALL RNA genes (preprocess.py:232-233)
            if exclude_genes is not None:
                if excluded.any():
                    print(f"Excluding {excluded.sum()} genes from cNMF input (retained in tp10k):")
                    print(list(genes[excluded]))
                    eng.preprocess_subset(keep_genes=~excluded)
                else:
                    print("exclude_genes provided but none found in adata_RNA.var_names.")
            if select:                                              # on the RNA genes that are left (preprocess.py:314-315)
                hvg_var = seurat_v3_frame(eng, X.shape[0], genes[~excluded], n_top_rna_genes, batch=batch)
                sel = np.flatnonzero(hvg_var["highly_variable"].values)
                hvg_var = hvg_var.iloc[sel]
            Xout, obsm = self._batchcorrect_staged(eng, X.shape[0], sel, dense, obs, False, harmony_vars, target,
                                                   max_scaled_thresh, quantile_thresh, theta, max_iter_harmony,
                                                   harmony_res, harmony, pca)
            tp_genes, tp_types = genes, types_rna
            if adt is not None:
                eng.preprocess_upload(Xa)                           # normalised on its own (:254)
                tp10k = sp.hstack((tp10k, eng.preprocess_fetch_counts(target)), format="csr")
                tp_genes = pd.Index(list(genes) + list(adt[2]))
                if types_rna is not None:
                    tp_types = np.concatenate([types_rna, types_adt])
        finally:
            eng.preprocess_release()
        hvgs = list(genes[~excluded][sel])
        if dense:
            tp10k = tp10k.toarray()
        var = pd.DataFrame(index=tp_genes)
        if tp_types is not None:
            var["feature_type"] = tp_types
        elif adt is None:
            var["features_renamed"] = tp_genes
        result = PreprocessResult(Xout, cells, pd.Index(hvgs), obs, obsm, var=hvg_var)
        tp = PreprocessResult(tp10k, cells, tp_genes, obs, var=var)
        if save_output_base is not None:
            _save_result(save_output_base + '.Corrected.HVG.Varnorm', result)
            _save_result(save_output_base + '.TP10K', tp)
            with open(save_output_base + '.Corrected.HVGs.txt', 'w') as F:
                F.write('\n'.join(hvgs))
        return result, tp, hvgs

    # ------------------------------------------------------------------ select_features_MI (preprocess.py:425-467)
    def select_features_MI(self, data, cluster, max_scaled_thresh=None, quantile_thresh=.9999, n_top_features=70,
                           makeplots=True):
        """Ranks the genes by their mutual information with ``cluster`` (an array-like of N labels, or a Series indexed
        by the cell names).  Returns a PreprocessResult: ``X`` the normalised, scaled and ceilinged matrix (cells x all
        genes, in the input's sparsity; the noise goes on a copy), ``var`` with ``MI``, ``MI_Rank``, ``MI_diff`` and
        ``highly_variable`` (MI_Rank < n_top_features) in the data's gene order.  numpy's global RandomState advances as
        the reference's call advances it."""
        import scipy.sparse as sp
        from scipy.special import digamma
        _check_quantile(quantile_thresh)
        mat, cells, genes, dense = _data_parts(data)
        labels = _cluster_labels(cluster, cells)
        n_neighbors = 3
        cls, n_cls, cst = mi_classes(labels, n_neighbors)
        X = _to_csr(mat)
        N, G = X.shape
        psi = digamma(np.arange(N + 1, dtype=np.float64))
        psi[0] = 0.0                                                  # (m >= 1: a cell counts itself)
        eng = self.engine
        try:
            Xc = eng.preprocess_upload(X)
            rs = eng.preprocess_row_sums()                            # normalize_total(target_sum=None)
            if not (rs > 0).any():
                raise ValueError("no cell has counts")
            target = np.median(rs[rs > 0])
            # sc.pp.scale over the whole matrix: its std in numpy's order, as the reference's scale computes it
            eng.preprocess_normalize_dense(0, float(target), max_scaled_thresh)
            _ceiling(eng, 0, N, G, quantile_thresh)
            Xout = eng.preprocess_fetch(0)
            if not dense:                                             # on the staged counts' structure
                rows = np.repeat(np.arange(N), np.diff(Xc.indptr))
                Xout = sp.csr_matrix((Xout[rows, Xc.indices], Xc.indices.copy(), Xc.indptr.copy()), shape=(N, G))
            mi, state = eng.preprocess_select_mi(0, cls, n_cls, n_neighbors, np.random.get_state(), psi, cst)
            np.random.set_state(state)
        finally:
            eng.preprocess_release()
        return PreprocessResult(Xout, cells, genes, var=mi_ranking(mi, genes, n_top_features))


CONTINUOUS_LABELS_ERROR = ("Unknown label type: continuous. Maybe you are trying to fit a classifier, which expects "
                           "discrete classes on a regression target with continuous values.")


def _cluster_labels(cluster, cells):
    """the labels of the cells, in their order: a Series indexed by the cell names is aligned as _align_obs does;
    float labels must be integral (sklearn's check_classification_targets)"""
    if isinstance(cluster, pd.Series):
        cluster = _align_obs(cluster.to_frame(), cells).iloc[:, 0]
    y = np.asarray(cluster)
    if y.ndim != 1 or y.shape[0] != len(cells):
        raise ValueError("cluster has shape %s for %d cells" % (y.shape, len(cells)))
    if y.dtype.kind == "c" or (y.dtype.kind == "f" and not (np.isfinite(y).all() and (y == np.round(y)).all())):
        raise ValueError(CONTINUOUS_LABELS_ERROR)
    return y


def mi_classes(labels, n_neighbors):
    """what the device needs from the labels (sklearn's _compute_mi_cd): class ids [N] (-1 for a cell of a class with
    one cell, dropped), the number of kept classes and the gene-independent terms
    (psi(n_kept) + mean psi(k_all)) - mean psi(label_counts), computed with sklearn's own arrays and expression"""
    from scipy.special import digamma
    _, inv = np.unique(labels, return_inverse=True)
    inv = inv.reshape(-1)
    counts = np.bincount(inv)
    keep_cls = np.flatnonzero(counts > 1)
    if keep_cls.size == 0:
        raise ValueError("no cluster has two cells")
    code = np.full(counts.size, -1, dtype=np.int32)
    code[keep_cls] = np.arange(keep_cls.size, dtype=np.int32)
    cls = code[inv]
    label_counts = counts[inv].astype(np.float64)
    k_all = np.minimum(n_neighbors, label_counts - 1)
    mask = label_counts > 1
    n_samples = np.sum(mask)
    label_counts, k_all = label_counts[mask], k_all[mask]
    cst = digamma(n_samples) + np.mean(digamma(k_all)) - np.mean(digamma(label_counts))
    return cls, int(keep_cls.size), float(cst)


def mi_ranking(mi, genes, n_top_features):
    """the reference's var columns from the MI vector (preprocess.py:452-465), in the genes' order"""
    res = pd.Series(mi, index=genes)
    res = res.sort_values(ascending=False)
    resdf = pd.DataFrame([res.values, np.arange(res.shape[0])], columns=res.index, index=['MI', 'MI_Rank']).T
    resdf['MI_diff'] = resdf['MI'].diff()
    var = pd.DataFrame(index=genes)
    for v in resdf.columns:
        var[v] = resdf[v]
    var['highly_variable'] = var['MI_Rank'] < n_top_features
    return var


def _save_result(base, res):
    """a PreprocessResult on disk: ``<base>.df.npz`` (save_df_to_npz) when dense, ``<base>.npz`` (save_csr_fast) with
    ``<base>.cells.txt`` / ``<base>.genes.txt`` when sparse"""
    import scipy.sparse as sp
    from .cnmf import save_csr_fast, save_df_to_npz
    if not sp.issparse(res.X):
        save_df_to_npz(pd.DataFrame(res.X, index=res.obs_names, columns=res.var_names), base + '.df.npz')
        return
    save_csr_fast(base + '.npz', sp.csr_matrix(res.X))
    for ext, names in (('.cells.txt', res.obs_names), ('.genes.txt', res.var_names)):
        with open(base + ext, 'w') as F:
            F.write('\n'.join(str(x) for x in names))


def _align_obs(obs, cells):
    """obs in the order of the cells (by name when its index holds them all, else by position)"""
    idx = pd.Index([str(c) for c in obs.index])
    if len(idx) == len(cells) and idx.equals(cells):
        return obs
    if len(idx) == len(cells) and set(idx) == set(cells):
        return obs.iloc[idx.get_indexer(cells)]
    if len(obs) != len(cells):
        raise ValueError("obs has %d rows for %d cells" % (len(obs), len(cells)))
    return obs
