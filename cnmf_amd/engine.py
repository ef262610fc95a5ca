"""Python face of the C-ABI: one ``Engine`` = one ``cnmf_ctx`` = one MI355X.

The engine keeps the cells x genes matrix resident in HBM and runs batches of
NMF restarts / NNLS refits on it.  Everything numeric happens in
``libcnmf_hip.so``; this module only marshals numpy buffers through ctypes and
maps status codes to the exception types the reference path raises
(scikit-learn raises ValueError / TypeError).
"""
import ctypes as C
import os
import warnings

import numpy as np

from . import _lib

_ERR = {-1: ValueError, -2: RuntimeError, -3: MemoryError, -4: RuntimeError,
        -5: NotImplementedError, -6: RuntimeError}


class ConvergenceWarning(UserWarning):
    """Mirror of sklearn.exceptions.ConvergenceWarning (sklearn _nmf.py:1727-1732)."""


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def regularization(n_samples, n_features, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0):
    """sklearn's scaling of the penalties, decomposition/_nmf.py:1254-1265."""
    return (n_features * alpha_W * l1_ratio, n_samples * alpha_H * l1_ratio,
            n_features * alpha_W * (1.0 - l1_ratio), n_samples * alpha_H * (1.0 - l1_ratio))


def _nndsvd_finish(k, Q, B, transpose, eps=1e-6):
    """The host tail of one NNDSVD initialisation (sklearn utils/extmath.py:588-602 + decomposition/_nmf.py:317-354):
    Q [M_rows, c] orthonormal, B = Q^T M [c, M_cols] -> small SVD, svd_flip, positive / negative split, threshold.
    Everything runs on ROWS of length n_samples / n_features (the singular vectors are kept transposed: k x M_rows from
    ONE product Uhat[:, :k]^T Q^T, only the k vectors that are used) -- the column-wise form of the same arithmetic spent
    20 ms of its 40 in one strided arg-max."""
    from scipy import linalg
    Q = np.asarray(Q, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    UT = Uhat[:, :k].T @ Q.T                                      # [k, M_rows] = (Q Uhat)[:, :k]^T
    VT = Vt[:k, :]                                                # [k, M_cols]
    # svd_flip: u_based_decision on the matrix that was decomposed (M = X, or X^T when n_samples < n_features, where
    # sklearn transposes back BEFORE flipping: the decision is then taken on the rows of Vt)
    lead = VT if transpose else UT
    idx = np.argmax(np.abs(lead), axis=1)
    signs = np.sign(lead[np.arange(k), idx])
    UT = UT * signs[:, np.newaxis]
    VT = VT * signs[:, np.newaxis]
    WT, HR = (VT, UT) if transpose else (UT, VT)                  # rows: left vectors over samples, right over features
    S = s[:k]
    W = np.zeros_like(WT)
    H = np.zeros_like(HR)
    W[0] = np.sqrt(S[0]) * np.abs(WT[0])
    H[0] = np.sqrt(S[0]) * np.abs(HR[0])
    for j in range(1, k):
        x, y = WT[j], HR[j]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = np.sqrt(x_p @ x_p), np.sqrt(y_p @ y_p)
        x_n_nrm, y_n_nrm = np.sqrt(x_n @ x_n), np.sqrt(y_n @ y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[j] = lbd * u
        H[j] = lbd * v
    W[W < eps] = 0
    H[H < eps] = 0
    return np.ascontiguousarray(W.T), H


NNDSVD_VARIANTS = ("nndsvd", "nndsvda", "nndsvdar")


def _nndsvd_fill(W, H, variant, x_mean, random_state):
    """The zeros of an NNDSVD start (in place): ``'nndsvda'`` -> ``X.mean()``, ``'nndsvdar'`` -> small random values from
    ``check_random_state(random_state)`` (sklearn decomposition/_nmf.py, the end of ``_initialize_nmf``)."""
    if variant == "nndsvda":
        W[W == 0] = x_mean
        H[H == 0] = x_mean
    elif variant == "nndsvdar":
        rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        W[W == 0] = abs(x_mean * rng.standard_normal(size=len(W[W == 0])) / 100)
        H[H == 0] = abs(x_mean * rng.standard_normal(size=len(H[H == 0])) / 100)
    elif variant != "nndsvd":
        raise ValueError("Invalid init parameter: got %r instead of one of %r" % (variant, NNDSVD_VARIANTS))
    return W, H


class Engine:
    def __init__(self, device=0, detect_counts=True, mu_rank_limit=_lib.CNMF_MU_KMAX, mu_sparse_rank_limit=_lib.CNMF_MU_SPARSE_KMAX):
        """``detect_counts=False``: never take the integer-plane (count-structured) GEMM path -- see
        :meth:`set_count_detection`.  ``mu_rank_limit``: 64 (default) or 128, see :attr:`mu_rank_limit`.
        ``mu_sparse_rank_limit``: 32 (default) or 64, see :attr:`mu_sparse_rank_limit`."""
        self._lib = _lib.load()
        if self._lib.cnmf_device_count() <= 0:
            raise RuntimeError("cnmf_amd: no HIP device visible -- the engine has no CPU fallback")
        self._ctx = self._lib.cnmf_create(int(device))
        if not self._ctx:
            raise RuntimeError("cnmf_create failed: %s" % self._lib.cnmf_last_error(None).decode())
        self.device = int(device)
        self._env_snap = self._env_now()
        self.shape = None
        self._x_mean, self._x_mean_src = None, None
        self.x_dtype = None
        self.x_has_zero = False            # (scikit-learn refuses beta_loss <= 0 on a matrix that contains a zero)
        self.last_stats = None
        self._prep = None                  # (shape, nnz) of the counts staged by prepare_upload
        self.store_gen = 0                 # generation of the resident spectra store (bumped by spectra_reset)
        self.last_store_offsets = None     # first store row of every restart of the last resident batch
        self.last_store_gen = -1
        if not detect_counts:
            self.set_count_detection(False)
        if mu_rank_limit != _lib.CNMF_MU_KMAX:
            self.mu_rank_limit = mu_rank_limit
        if mu_sparse_rank_limit != _lib.CNMF_MU_SPARSE_KMAX:
            self.mu_sparse_rank_limit = mu_sparse_rank_limit

    @property
    def mu_rank_limit(self):
        """Largest rank :meth:`nmf_mu_batch`, :meth:`nnls_mu` and :meth:`mu_refit_f64` accept on this engine: 64
        (``CNMF_MU_KMAX``, the default) or, by opt-in, 128 (``CNMF_MU_KMAX_WIDE``: ranks 65..128 on the matrix-pipe kernels
        and the float64 refit; the vector-ALU route -- ``CNMF_MU_VALU=1`` or a matrix beyond 2^24 cells or genes -- stays at
        64).  Any other value raises ValueError."""
        return int(self._lib.cnmf_get_mu_rank_limit(self._ctx))

    @mu_rank_limit.setter
    def mu_rank_limit(self, limit):
        self._check(self._lib.cnmf_set_mu_rank_limit(self._ctx, int(limit)))

    @property
    def mu_sparse_rank_limit(self):
        """Largest rank at which a Kullback-Leibler restart of :meth:`nmf_mu_batch` / :meth:`nnls_mu` may run on the non-zeros
        of the matrix: 32 (``CNMF_MU_SPARSE_KMAX``, the default: ranks 33 up on the dense kernels) or, by opt-in, 64
        (``CNMF_MU_SPARSE_KMAX_WIDE``: ranks 33..64 at padded rank 64, two lanes per row).  ``CNMF_MU_SPARSE`` decides as
        at ranks up to 32, the density rule at 15 % non-zero instead of a quarter (the measured crossover); ranks 65..128 and
        Itakura-Saito stay on the dense kernels.
        Any other value raises ValueError."""
        return int(self._lib.cnmf_get_mu_sparse_rank_limit(self._ctx))

    @mu_sparse_rank_limit.setter
    def mu_sparse_rank_limit(self, limit):
        self._check(self._lib.cnmf_set_mu_sparse_rank_limit(self._ctx, int(limit)))

    def set_count_detection(self, enabled):
        """The engine recognises ``X = counts / std`` (integers x one constant per gene, tolerance 1e-3 count units;
        DESIGN.md section 4) and then multiplies exact integer planes.  A matrix that merely happens to lie that close
        to such a grid would be snapped onto it: switch the detection off for data that is not count-derived
        (same effect as the environment variable ``CNMF_NO_COUNTS=1``)."""
        self._check(self._lib.cnmf_set_count_detection(self._ctx, int(bool(enabled))))

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _env_now():
        return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("CNMF_")))

    def reload_env(self):
        """The library reads its ``CNMF_*`` switches once per context (cnmf_create); this re-reads them."""
        self._check(self._lib.cnmf_reload_env(self._ctx))
        self._env_snap = self._env_now()

    def _sync_env(self):
        # host-side convenience (tests and A/B tools flip a switch between two calls of one process): the context's
        # snapshot follows os.environ when -- and only when -- the process environment has changed since it was taken
        if self._env_now() != self._env_snap:
            self.reload_env()

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.cnmf_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.cnmf_last_error(self._ctx).decode()
            raise _ERR.get(rc, RuntimeError)("cnmf_hip: %s (code %d)" % (msg, rc))

    def _params(self, tol, max_iter, alpha_W, alpha_H, l1_ratio, kc_max=0, lag=0, profile=0, n_features=None):
        """``n_features``: the feature count sklearn would see (it scales the W penalties, _nmf.py:1254-1265) when the
        solved problem uses a column SUBSET of the resident matrix (nnls_gram)."""
        self._sync_env()
        N, G = self.shape
        l1W, l1H, l2W, l2H = regularization(N, G if n_features is None else int(n_features), alpha_W, alpha_H, l1_ratio)
        return _lib.CdParams(float(tol), int(max_iter), int(kc_max), l1W, l2W, l1H, l2H, int(lag), int(profile))

    # ------------------------------------------------------------------ data matrix
    def set_matrix(self, X):
        """Upload the cells x genes matrix (dense ndarray or scipy CSR), once per context.

        Mirrors sklearn's input validation for NMF (check_array + check_non_negative,
        decomposition/_nmf.py:1126,283): NaN/inf and negative entries raise ValueError."""
        import scipy.sparse as sp
        if sp.issparse(X):
            X = X.tocsr()
            if not X.has_canonical_format:          # (sorted rows without duplicates: the device keeps the arrays as uploaded)
                X = X.copy()
                X.sum_duplicates()
            data = X.data
            if not np.isfinite(data).all():
                raise ValueError("Input X contains NaN or infinity.")
            if data.size and data.min() < 0:
                raise ValueError("Negative values in data passed to NMF (input X)")
            self.x_dtype = np.dtype(X.dtype) if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
            # scipy's sparse mean (what scikit-learn's init='random' divides by) copies, divides and sums the whole matrix:
            # 0.17 s at 50 000 x 2 000 -- taken only when a restart asks for it (the TPM upload of consensus() never does)
            self._x_mean, self._x_mean_src = None, X
            self.x_has_zero = bool(X.nnz < X.shape[0] * X.shape[1] or (data.size and data.min() == 0))
            vals = np.ascontiguousarray(data, dtype=np.float32)
            if vals.size and not vals.all():
                # a STORED zero (explicit, or a float64 value that underflows in float32) would make the library treat the
                # arrays as non-canonical and form the dense image of the whole matrix (round-5 advice): compact them here
                Xc = sp.csr_matrix((vals, X.indices.copy(), X.indptr.copy()), shape=X.shape)    # (eliminate_zeros works in place:
                Xc.eliminate_zeros()                                                            #  never on the caller's arrays)
                X, vals = Xc, np.ascontiguousarray(Xc.data, dtype=np.float32)
            indptr = np.ascontiguousarray(X.indptr, dtype=np.int32)
            indices = np.ascontiguousarray(X.indices, dtype=np.int32)
            ip = C.POINTER(C.c_int32)
            self._check(self._lib.cnmf_set_matrix_csr(self._ctx, indptr.ctypes.data_as(ip),
                                                      indices.ctypes.data_as(ip), _fp(vals),
                                                      X.shape[0], X.shape[1]))
        else:
            X = np.asarray(X)
            if X.ndim != 2:
                raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
            if X.dtype not in (np.float32, np.float64):
                X = X.astype(np.float64)            # sklearn: ints -> float64
            if not np.isfinite(X).all():
                raise ValueError("Input X contains NaN or infinity.")
            if X.size and X.min() < 0:
                raise ValueError("Negative values in data passed to NMF (input X)")
            self.x_dtype = X.dtype
            self.x_has_zero = bool(X.size and X.min() == 0)
            self.x_mean = X.mean()                  # numpy scalar of X's dtype, like sklearn's X.mean()
            Xf = np.ascontiguousarray(X, dtype=np.float32)
            self._check(self._lib.cnmf_set_matrix(self._ctx, _fp(Xf), Xf.shape[0], Xf.shape[1]))
        self.shape = (int(X.shape[0]), int(X.shape[1]))
        return self

    def matrix_images(self):
        """Which images of the matrix the device holds right now (cnmf_matrix_images): a CSR upload keeps its compressed
        rows and forms the dense float32 image only when a path that multiplies the dense matrix asks for it."""
        f = C.c_int32(0)
        self._check(self._lib.cnmf_matrix_images(self._ctx, C.byref(f)))
        names = ("dense", "csr", "csr_of_transpose", "dense_transpose", "non_zero_images_16", "non_zero_images_32", "count_planes",
                 "count_planes_bytes", "non_zero_images_64")
        return {n: bool(f.value >> i & 1) for i, n in enumerate(names)}

    def get_matrix(self):
        """The resident matrix back on the host (float32 [n_cells, n_genes])."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        out = np.empty(self.shape, dtype=np.float32)
        self._check(self._lib.cnmf_get_matrix(self._ctx, _fp(out)))
        return out

    def col_mean_var(self):
        """Per-gene mean and POPULATION variance (ddof=0) of the resident matrix in float64 -- the
        O(cells x genes) part of the reference's high-variance-gene statistics (cnmf.py:195-196, 126-129)."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        dblp = C.POINTER(C.c_double)
        mean, ssd = np.empty(G), np.empty(G)
        self._check(self._lib.cnmf_col_moments(self._ctx, mean.ctypes.data_as(dblp), ssd.ctypes.data_as(dblp)))
        return mean, ssd / N

    def scale_genes_unit_variance(self):
        """``X /= X.std(axis=0, ddof=1)`` on the resident matrix -- the dense branch of the reference's
        ``get_norm_counts`` (cnmf.py:540-548), statistics in float64.  Returns ``(std, row_sums)``;
        ``row_sums == 0`` marks the reference's "zero cells" (cnmf.py:550-554).  Afterwards the matrix
        counts as float64 input, like ``norm_counts.X`` in the reference (cnmf.py:534)."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        if N < 2:
            raise ValueError("need at least two cells for a variance")
        dblp = C.POINTER(C.c_double)
        mean, ssd = np.empty(G), np.empty(G)
        self._check(self._lib.cnmf_col_moments(self._ctx, mean.ctypes.data_as(dblp), ssd.ctypes.data_as(dblp)))
        std = np.sqrt(ssd / (N - 1))
        self._check(self._lib.cnmf_scale_columns(self._ctx, std.ctypes.data_as(dblp)))
        rs = np.empty(N)
        self._check(self._lib.cnmf_row_sums(self._ctx, rs.ctypes.data_as(dblp)))
        self.x_dtype = np.dtype(np.float64)
        self.x_mean = np.float64(rs.sum() / (float(N) * float(G)))
        return std, rs

    # ------------------------------------------------------------------ prepare (cnmf_prepare_*, prepare_host.hip.h)
    def prepare_upload(self, counts):
        """Stage the raw cells x all-genes counts (scipy.sparse) on the device, apart from the resident matrix.  Stored
        zeros are dropped and duplicates summed (on a copy); integer data below 2^24 and float32 data travel as float32,
        anything else as float64 -- the device keeps float64 either way."""
        import scipy.sparse as sp
        X = sp.csr_matrix(counts)
        if not X.has_canonical_format or (X.nnz and not X.data.all()):
            X = X.copy()
            X.sum_duplicates()
            X.eliminate_zeros()
        data = X.data
        if data.dtype == np.float32 or (data.dtype.kind in "iub" and (data.size == 0 or np.abs(data).max() < (1 << 24))):
            vals, f64 = np.ascontiguousarray(data, dtype=np.float32), 0
        else:
            vals, f64 = np.ascontiguousarray(data, dtype=np.float64), 1
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        self._check(self._lib.cnmf_prepare_upload_csr(self._ctx, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      vals.ctypes.data_as(C.c_void_p), f64, X.shape[0], X.shape[1]))
        self._prep = (X.shape, X.nnz)
        return X

    def prepare_tpm_stats(self, target_sum=1e6, want_tpm=False):
        """Row sums of the staged counts, and the per-gene mean and POPULATION variance of their TPM
        (``x * target_sum / row_sum``; ``target_sum <= 0``: of the matrix as staged).  ``want_tpm``: also the TPM values in
        the staged CSR order.  Returns ``(row_sums, mean, var, tpm_data or None)``."""
        (N, G), nnz = self._prep
        dblp = C.POINTER(C.c_double)
        rs, mean, var = np.empty(N), np.empty(G), np.empty(G)
        tpm = np.empty(max(nnz, 1)) if want_tpm else None
        self._check(self._lib.cnmf_prepare_tpm_stats(self._ctx, float(target_sum), rs.ctypes.data_as(dblp),
                                                     mean.ctypes.data_as(dblp), var.ctypes.data_as(dblp),
                                                     tpm.ctypes.data_as(dblp) if want_tpm else None))
        return rs, mean, var, (tpm[:nnz] if want_tpm else None)

    def prepare_select(self, genes, densify):
        """The columns ``genes`` of the staged counts, in list order, divided by their ddof=1 std (float64), become the
        RESIDENT matrix (dense image when ``densify``, CSR otherwise -- what set_matrix makes of the float64 result); the
        staging is released.  Returns ``(std, row_sums, Y)``: Y the float64 result, an ndarray (densify) or a scipy CSR."""
        import scipy.sparse as sp
        (N, G), _ = self._prep
        genes = np.ascontiguousarray(genes, dtype=np.int32)
        n = int(genes.size)
        dblp = C.POINTER(C.c_double)
        std, rs, nnz = np.empty(max(n, 1)), np.empty(N), C.c_int64(0)
        self._check(self._lib.cnmf_prepare_select(self._ctx, n, genes.ctypes.data_as(C.POINTER(C.c_int32)), int(bool(densify)),
                                                  std.ctypes.data_as(dblp), rs.ctypes.data_as(dblp), C.byref(nnz)))
        self.shape = (int(N), n)
        self.x_dtype = np.dtype(np.float64)
        if densify:
            Y = np.empty((N, n))
            self._check(self._lib.cnmf_prepare_fetch(self._ctx, None, None, Y.ctypes.data_as(dblp)))
            self.x_has_zero = bool(Y.size and Y.min() == 0)
            self.x_mean = Y.mean()                  # (set_matrix's rule for a float64 array)
        else:
            nz = int(nnz.value)
            indptr, indices, data = np.empty(N + 1, dtype=np.int64), np.empty(max(nz, 1), dtype=np.int32), np.empty(max(nz, 1))
            self._check(self._lib.cnmf_prepare_fetch(self._ctx, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     indices.ctypes.data_as(C.POINTER(C.c_int32)), data.ctypes.data_as(dblp)))
            if indptr[-1] < (1 << 31):
                indptr = indptr.astype(np.int32)    # (scipy's own index type for a matrix of this size)
                Y = sp.csr_matrix((data[:nz], indices[:nz], indptr), shape=(N, n))
            else:
                Y = sp.csr_matrix((data[:nz], indices[:nz].astype(np.int64), indptr), shape=(N, n))
            Y.has_canonical_format = True           # (the device lists every row's columns ascending, without duplicates)
            self.x_has_zero = bool(nz < N * n)
            self._x_mean, self._x_mean_src = None, Y     # (set_matrix's rule for a sparse matrix: X.mean() when asked)
        self._prep = None
        return std[:n], rs, Y

    def prepare_release(self):
        """Free the staged counts and any selection not fetched (a prepare that stopped half way)."""
        self._check(self._lib.cnmf_prepare_release(self._ctx))
        self._prep = None

    # ------------------------------------------------------------------ preprocess (cnmf_preprocess_*, preprocess_host.hip.h)
    # A staging of its own with two result slots: the resident matrix, the spectra store and the prepare staging stay as
    # they are.
    def preprocess_upload(self, counts):
        """Stage raw counts (scipy.sparse, values > 0 once stored zeros are dropped) for preprocess_select; releases the
        previous preprocess staging.  Returns the canonical CSR that was staged."""
        import scipy.sparse as sp
        X = sp.csr_matrix(counts)
        if not X.has_canonical_format or (X.nnz and not X.data.all()):
            X = X.copy()
            X.sum_duplicates()
            X.eliminate_zeros()
        vals = np.ascontiguousarray(X.data, dtype=np.float64)
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        self._check(self._lib.cnmf_preprocess_upload_csr(self._ctx, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                         indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         vals.ctypes.data_as(C.c_void_p), 1, X.shape[0], X.shape[1]))
        self._pre = {"N": X.shape[0], "G": X.shape[1], 0: None, 1: None}
        return X

    def preprocess_set_dense(self, slot, X):
        """A dense float64 matrix (cells x genes) into ``slot``."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        self._check(self._lib.cnmf_preprocess_set_dense(self._ctx, int(slot), X.ctypes.data_as(C.POINTER(C.c_double)),
                                                        X.shape[0], X.shape[1]))
        pre = getattr(self, "_pre", None) or {"N": X.shape[0], 0: None, 1: None}
        pre["N"], pre[int(slot)] = X.shape[0], (X.shape[1], -2)
        self._pre = pre

    def preprocess_select(self, slot, genes, target_sum=0.0, max_value=None):
        """``slot`` := the columns ``genes`` of the staged counts (rows scaled to ``target_sum`` when > 0), each divided by
        its ddof=1 std (1 for a zero std), clipped at ``max_value``.  Returns the std."""
        genes = np.ascontiguousarray(genes, dtype=np.int32)
        n = int(genes.size)
        std, nnz = np.empty(max(n, 1)), C.c_int64(0)
        mv = np.inf if max_value is None else float(max_value)
        self._check(self._lib.cnmf_preprocess_select(self._ctx, int(slot), n, genes.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     float(target_sum), mv, std.ctypes.data_as(C.POINTER(C.c_double)),
                                                     C.byref(nnz)))
        self._pre[int(slot)] = (n, int(nnz.value))
        return std[:n]

    def preprocess_order_stats(self, slot, k):
        """The k-th and (k+1)-th smallest of all entries of ``slot`` (implicit zeros included), as float64."""
        lo, hi = C.c_double(0), C.c_double(0)
        self._check(self._lib.cnmf_preprocess_order_stats(self._ctx, int(slot), int(k), C.byref(lo), C.byref(hi)))
        return np.float64(lo.value), np.float64(hi.value)

    def preprocess_ceiling(self, slot, thresh):
        self._check(self._lib.cnmf_preprocess_ceiling(self._ctx, int(slot), float(thresh)))

    def preprocess_densify(self, slot):
        self._check(self._lib.cnmf_preprocess_densify(self._ctx, int(slot)))
        self._pre[int(slot)] = (self._pre[int(slot)][0], -2)

    def preprocess_fetch(self, slot):
        """The slot's matrix: an ndarray (dense slot) or a canonical scipy CSR."""
        import scipy.sparse as sp
        N = self._pre["N"]
        n, nnz = self._pre[int(slot)]
        dblp = C.POINTER(C.c_double)
        if nnz == -2:
            Y = np.empty((N, n))
            self._check(self._lib.cnmf_preprocess_fetch(self._ctx, int(slot), None, None, Y.ctypes.data_as(dblp)))
            return Y
        indptr, indices, data = np.empty(N + 1, dtype=np.int64), np.empty(max(nnz, 1), dtype=np.int32), np.empty(max(nnz, 1))
        self._check(self._lib.cnmf_preprocess_fetch(self._ctx, int(slot), indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    indices.ctypes.data_as(C.POINTER(C.c_int32)), data.ctypes.data_as(dblp)))
        if indptr[-1] < (1 << 31):
            indptr = indptr.astype(np.int32)
        Y = sp.csr_matrix((data[:nnz], indices[:nnz].astype(indptr.dtype), indptr), shape=(N, n))
        Y.has_canonical_format = True
        return Y

    def preprocess_scatter(self, slot):
        """Column means and the scatter matrix sum_i (x_i - mean)(x_i - mean)^T of a dense slot (float64)."""
        n = self._pre[int(slot)][0]
        mean, S = np.empty(n), np.empty((n, n))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_scatter(self._ctx, int(slot), mean.ctypes.data_as(dblp), S.ctypes.data_as(dblp)))
        return mean, S

    def preprocess_project(self, slot, mean, V):
        """(X - mean) V over a dense slot."""
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        out = np.empty((self._pre["N"], V.shape[1]))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_project(self._ctx, int(slot), V.shape[1], mean.ctypes.data_as(dblp),
                                                      V.ctypes.data_as(dblp), out.ctypes.data_as(dblp)))
        return out

    def preprocess_ridge_moments(self, slot, R, Phi):
        """R [K][N], Phi [B1][N] (harmonypy's old layout) over the dense slot X [N][n]: M [K][B1][n] with
        M[k, b] = sum_i R[k,i] Phi[b,i] X[i] and gram [K][B1][B1] = sum_i R[k,i] Phi[b,i] Phi[c,i]."""
        K, B1, n = R.shape[0], Phi.shape[0], self._pre[int(slot)][0]
        if K * B1 > _lib.CNMF_RIDGE_MAX:
            raise NotImplementedError("K * (B + 1) = %d is above the device limit %d" % (K * B1, _lib.CNMF_RIDGE_MAX))
        Rt = np.ascontiguousarray(np.asarray(R, dtype=np.float64).T)
        Pt = np.ascontiguousarray(np.asarray(Phi, dtype=np.float64).T)
        M, G = np.empty((K, B1, n)), np.empty((K, B1, B1))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_ridge_moments(self._ctx, int(slot), K, B1, Rt.ctypes.data_as(dblp),
                                                            Pt.ctypes.data_as(dblp), M.ctypes.data_as(dblp),
                                                            G.ctypes.data_as(dblp)))
        return M, G

    def preprocess_ridge_apply(self, slot, W, clip=True):
        """Dense slot X := max(X - sum_k sum_b (R[k] Phi[b])^T W[k, b], 0), W [K][B1][n], factors of the last moments.
        ``clip=False``: without the maximum (a matrix with negative entries)."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        dblp = C.POINTER(C.c_double)
        if clip:
            self._check(self._lib.cnmf_preprocess_ridge_apply(self._ctx, int(slot), W.ctypes.data_as(dblp)))
        else:
            self._check(self._lib.cnmf_preprocess_ridge_apply_mode(self._ctx, int(slot), W.ctypes.data_as(dblp), 0))

    # ------------------------------------------------------------------ top eigenpairs through the tridiagonal form (pca_host.hip.h)
    # The reflectors of the last tridiagonalisation stay staged beside the preprocess slots: the next one replaces them,
    # preprocess_release (and every preprocess_upload) frees them.
    @staticmethod
    def pca_check_limit(n):
        """NotImplementedError above the device limit of the tridiagonalisation entry points (nothing is allocated)"""
        if n > _lib.CNMF_PCA_NMAX:
            raise NotImplementedError("n = %d is above the device limit %d of the tridiagonalisation (Preprocess: use "
                                      "pca=\"lapack\")" % (n, _lib.CNMF_PCA_NMAX))

    def symmetric_tridiagonalize(self, A):
        """Householder tridiagonalisation of the symmetric float64 matrix ``A`` [n][n] (both triangles are read; symmetry
        is not checked) on the device: returns ``(d [n], e [n - 1])`` with Q^T A Q = tridiag(e, d, e).  Q stays staged
        for :meth:`tridiagonal_back_transform`."""
        if np.ndim(A) != 2 or np.shape(A)[0] != np.shape(A)[1] or np.shape(A)[0] < 1:
            raise ValueError("a square matrix is expected, not shape %s" % (np.shape(A),))
        n = int(np.shape(A)[0])
        self.pca_check_limit(n)
        A = np.ascontiguousarray(A, dtype=np.float64)
        d, e = np.empty(n), np.empty(max(n - 1, 1))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_symmetric_tridiagonalize(self._ctx, n, A.ctypes.data_as(dblp), d.ctypes.data_as(dblp),
                                                            e.ctypes.data_as(dblp)))
        return d, e[:n - 1]

    def tridiagonal_back_transform(self, Z, sign_rule=False):
        """``Q Z`` for ``Z`` [n][n_comp] (1 <= n_comp <= n; eigenvectors of the tridiagonal matrix give eigenvectors of
        A), Q of the last tridiagonalisation.  ``sign_rule``: every column then has its entry of largest magnitude
        positive (the first index on ties).  ValueError when nothing is staged or n differs."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] < 1:
            raise ValueError("Z [n][n_comp] is expected, not shape %s" % (Z.shape,))
        V = np.empty_like(Z)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_tridiagonal_back_transform(self._ctx, Z.shape[0], Z.shape[1], Z.ctypes.data_as(dblp),
                                                              int(bool(sign_rule)), V.ctypes.data_as(dblp)))
        return V

    def symmetric_eigh_top(self, A, k, solver="host"):
        """The ``k`` largest eigenvalues of the symmetric matrix ``A`` (descending) and their eigenvectors [n][k] (the
        sign rule applied): tridiagonalisation on the device, the tridiagonal problem on the host
        (``preprocess.tridiagonal_top``; ``solver="host"``, the default) or on the device as well (``solver="device"``:
        one library call, see :meth:`tridiagonal_eigh_top`; a result its check does not accept is replaced through the
        host solve, and ``last_tridiagonal_solver`` says which of the two it was), back-transformation on the device."""
        from .preprocess import tridiagonal_top
        if solver not in ("host", "device"):
            raise ValueError("solver must be \"host\" or \"device\", not %r" % (solver,))
        n = int(np.shape(A)[0]) if np.ndim(A) == 2 else 0
        if not 1 <= int(k) <= max(n, 1):
            raise ValueError("k = %s outside [1, %d]" % (k, n))
        if solver == "host":
            d, e = self.symmetric_tridiagonalize(A)
            w, Z = tridiagonal_top(d, e, int(k))
            return w, self.tridiagonal_back_transform(Z, sign_rule=True)
        if np.ndim(A) != 2 or np.shape(A)[0] != np.shape(A)[1]:
            raise ValueError("a square matrix is expected, not shape %s" % (np.shape(A),))
        self.pca_check_limit(n)
        A = np.ascontiguousarray(A, dtype=np.float64)
        w, V, info = np.empty(int(k)), np.empty((n, int(k))), np.empty(4)
        dblp = C.POINTER(C.c_double)
        rc = self._lib.cnmf_symmetric_eigh_top(self._ctx, n, int(k), A.ctypes.data_as(dblp), w.ctypes.data_as(dblp),
                                               V.ctypes.data_as(dblp), info.ctypes.data_as(dblp))
        if not self._tridiagonal_accepted(rc, info):
            w, Z = tridiagonal_top(*self.tridiagonal_fetch(n), int(k))
            V = self.tridiagonal_back_transform(Z, sign_rule=True)
        return w, V

    # The tridiagonal problem on the device (tridiag_eig_host.hip.h).  last_tridiagonal_solver: "device", or
    # "host_fallback" when the device's own check of its result (residual within 2 n eps |T|_1, orthogonality within
    # 2 n eps, every entry finite) did not accept it; last_tridiagonal_check: the measured (residual / u_T,
    # |rayleigh quotient - w| / u_T, orthogonality / (n eps)).
    last_tridiagonal_solver = None
    last_tridiagonal_check = None

    def _tridiagonal_accepted(self, rc, info):
        if rc != _lib.CNMF_NOT_ACCEPTED:
            self._check(rc)
        ok = rc == 0 and info[0] == 1.0
        self.last_tridiagonal_solver = "device" if ok else "host_fallback"
        self.last_tridiagonal_check = tuple(float(x) for x in info[1:4])
        return ok

    def tridiagonal_eigh_top(self, d, e, k):
        """The ``k`` largest eigenpairs of the symmetric tridiagonal matrix with diagonal ``d`` [n] and off-diagonal ``e``
        [n - 1], on the device: multisection on Sturm counts (the eigenvalues are those of the float64 restatement in
        tests/_tridiag_eig_ref.py, bit for bit), three steps of inverse iteration per vector, CGS2, and a check of the
        result.  Returns ``(w [k] descending, Z [n][k], accepted)``; ``accepted`` False: ``w`` is valid and ``Z`` is not
        (inverse iteration without orthogonalisation inside fails on some large tight clusters) -- take
        ``preprocess.tridiagonal_top`` then.  ValueError on non-finite input or ``k`` outside [1, n]."""
        d = np.ascontiguousarray(d, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64)
        n = d.size
        if d.ndim != 1 or n < 1 or e.shape != (n - 1,):
            raise ValueError("d [n] and e [n - 1] are expected, not shapes %s and %s" % (d.shape, e.shape))
        if not 1 <= int(k) <= n:
            raise ValueError("k = %s outside [1, %d]" % (k, n))
        self.pca_check_limit(n)
        e1 = e if n > 1 else np.zeros(1)
        w, Z, info = np.empty(int(k)), np.empty((n, int(k))), np.empty(4)
        dblp = C.POINTER(C.c_double)
        rc = self._lib.cnmf_tridiagonal_eigh_top(self._ctx, n, int(k), d.ctypes.data_as(dblp), e1.ctypes.data_as(dblp),
                                                 w.ctypes.data_as(dblp), Z.ctypes.data_as(dblp), info.ctypes.data_as(dblp))
        return w, Z, self._tridiagonal_accepted(rc, info)

    def tridiagonal_fetch(self, n):
        """``(d [n], e [n - 1])`` of the staged tridiagonalisation"""
        d, e = np.empty(n), np.empty(max(n - 1, 1))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_tridiagonal_fetch(self._ctx, int(n), d.ctypes.data_as(dblp), e.ctypes.data_as(dblp)))
        return d, e[:n - 1]

    def tridiagonal_eigh_step_ms(self):
        """HIP-event milliseconds of the last device tridiagonal solve: bounds, bisection, inverse iteration,
        orthogonalisation plus check and (after :meth:`preprocess_pca_device`) back-transformation plus scores"""
        out = np.zeros(5)
        self._check(self._lib.cnmf_tridiagonal_eigh_step_ms(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def preprocess_pca_device(self, slot, n_comps):
        """The PCA of a dense slot in one library call: the scatter matrix, its tridiagonalisation, the tridiagonal
        eigenproblem (:meth:`tridiagonal_eigh_top`), back-transformation, sign rule and scores on the device; only the
        results cross the bus and the slot is left as it was.  Returns ``(mean [n], w [n_comps] (eigenvalues of the scatter
        matrix, descending), V [n][n_comps], scores [n_cells][n_comps])``.  A solve the device's check does not accept is
        redone by ``preprocess.tridiagonal_top`` on the host (``last_tridiagonal_solver == "host_fallback"``)."""
        n = self._pre[int(slot)][0]
        self.pca_check_limit(n)
        k = int(n_comps)
        if not 1 <= k <= n:
            raise ValueError("n_comps = %s outside [1, %d]" % (n_comps, n))
        mean, w, V, scores, info = np.empty(n), np.empty(k), np.empty((n, k)), np.empty((self._pre["N"], k)), np.empty(4)
        dblp = C.POINTER(C.c_double)
        rc = self._lib.cnmf_preprocess_pca_device(self._ctx, int(slot), k, mean.ctypes.data_as(dblp), w.ctypes.data_as(dblp),
                                                  V.ctypes.data_as(dblp), scores.ctypes.data_as(dblp), info.ctypes.data_as(dblp))
        if not self._tridiagonal_accepted(rc, info):
            from .preprocess import tridiagonal_top
            w, Z = tridiagonal_top(*self.tridiagonal_fetch(n), k)
            V, scores = self.preprocess_pca_finish(slot, Z)
        return mean, w, V, scores

    def preprocess_pca_tridiag(self, slot):
        """The scatter matrix of a dense slot (as :meth:`preprocess_scatter` forms it), tridiagonalised where it is:
        returns ``(mean [n], d [n], e [n - 1])``."""
        n = self._pre[int(slot)][0]
        self.pca_check_limit(n)
        mean, d, e = np.empty(n), np.empty(n), np.empty(max(n - 1, 1))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_pca_tridiag(self._ctx, int(slot), mean.ctypes.data_as(dblp),
                                                          d.ctypes.data_as(dblp), e.ctypes.data_as(dblp)))
        return mean, d, e[:n - 1]

    def preprocess_pca_finish(self, slot, Z):
        """After :meth:`preprocess_pca_tridiag` on ``slot``: ``V = Q Z`` [n][n_comp] with the sign rule, and the scores
        ``(X - mean) V`` [n_cells][n_comp]; V stays on the device in between.  Returns ``(V, scores)``."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        n = self._pre[int(slot)][0]
        if Z.ndim != 2 or Z.shape[0] != n or Z.shape[1] < 1:
            raise ValueError("Z [%d][n_comp] is expected, not shape %s" % (n, Z.shape))
        V, scores = np.empty_like(Z), np.empty((self._pre["N"], Z.shape[1]))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_pca_finish(self._ctx, int(slot), Z.shape[1], Z.ctypes.data_as(dblp),
                                                         V.ctypes.data_as(dblp), scores.ctypes.data_as(dblp)))
        return V, scores

    # ------------------------------------------------------------------ harmony (cnmf_harmony_*, harmony_host.hip.h)
    # Harmony's clustering loop with a state of its own: the preprocess staging stays as it is.
    @staticmethod
    def harmony_check_limits(d, K, B):
        """NotImplementedError above the device limits of the harmony entry points"""
        if K > _lib.CNMF_HARMONY_KMAX:
            raise NotImplementedError("K = %d clusters is above the device limit %d" % (K, _lib.CNMF_HARMONY_KMAX))
        if d > _lib.CNMF_HARMONY_DMAX:
            raise NotImplementedError("d = %d components is above the device limit %d" % (d, _lib.CNMF_HARMONY_DMAX))
        if K * (B + 1) > _lib.CNMF_RIDGE_MAX:
            raise NotImplementedError("K * (B + 1) = %d is above the device limit %d" % (K * (B + 1), _lib.CNMF_RIDGE_MAX))

    def harmony_begin(self, pca, codes, level_var, theta, sigma, pr_b):
        """pca [N][d]; codes [V][N] int32: every cell's level (an index into the B levels of all variables) per variable;
        level_var [B]: the variable of each level; theta [B], sigma [K], pr_b [B]."""
        pca = np.ascontiguousarray(pca, dtype=np.float64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        level_var = np.ascontiguousarray(level_var, dtype=np.int32)
        theta, sigma, pr_b = (np.ascontiguousarray(a, dtype=np.float64) for a in (theta, sigma, pr_b))
        if pca.ndim != 2 or codes.ndim != 2 or codes.shape[1] != pca.shape[0] or level_var.ndim != 1:
            raise ValueError("pca %s, codes %s, level_var %s" % (pca.shape, codes.shape, level_var.shape))
        N, d = pca.shape
        V, B, K = codes.shape[0], level_var.shape[0], sigma.shape[0]
        if theta.shape != (B,) or pr_b.shape != (B,) or sigma.ndim != 1 or K < 1 or N < 1 or d < 1:
            raise ValueError("theta %s, pr_b %s for %d levels; sigma %s" % (theta.shape, pr_b.shape, B, sigma.shape))
        if not np.isfinite(pca).all():
            raise ValueError("pca holds non-finite values")
        if codes.size and (codes.min() < 0 or codes.max() >= B or not (level_var[codes] == np.arange(V)[:, None]).all()):
            raise ValueError("codes do not name levels of their variable")
        self.harmony_check_limits(d, K, B)
        dblp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._check(self._lib.cnmf_harmony_begin(self._ctx, N, d, K, V, B, pca.ctypes.data_as(dblp), codes.ctypes.data_as(i32p),
                                                 level_var.ctypes.data_as(i32p), theta.ctypes.data_as(dblp),
                                                 sigma.ctypes.data_as(dblp), pr_b.ctypes.data_as(dblp)))
        self._har = {"N": N, "d": d, "K": K, "B": B}

    def _har_state(self):
        har = getattr(self, "_har", None)
        if har is None:
            raise RuntimeError("harmony_begin has not been called")
        return har

    def harmony_init(self, Y):
        """Y [d][K] unit centroids; returns the three objective terms [3]."""
        har = self._har_state()
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.shape != (har["d"], har["K"]) or not np.isfinite(Y).all():
            raise ValueError("centroids %s for d = %d, K = %d (finite values)" % (Y.shape, har["d"], har["K"]))
        obj = np.empty(3)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_harmony_init(self._ctx, Y.ctypes.data_as(dblp), obj.ctypes.data_as(dblp)))
        return obj

    def harmony_kmeans_step(self, perm, n_blocks):
        """one k-means iteration with update_R over np.array_split(perm, n_blocks); returns the objective terms [3]."""
        har = self._har_state()
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        if perm.shape != (har["N"],):
            raise ValueError("perm %s for %d cells" % (perm.shape, har["N"]))
        if not 1 <= int(n_blocks) <= 4096:
            raise ValueError("n_blocks = %s outside [1, 4096]" % (n_blocks,))
        obj = np.empty(3)
        self._check(self._lib.cnmf_harmony_kmeans_step(self._ctx, perm.ctypes.data_as(C.POINTER(C.c_int32)), int(n_blocks),
                                                       obj.ctypes.data_as(C.POINTER(C.c_double))))
        return obj

    def harmony_ridge_moments(self):
        """M [K][B1][d] and gram [K][B1][B1] of the ridge step over Z_orig^T with the current R."""
        har = self._har_state()
        K, B1, d = har["K"], har["B"] + 1, har["d"]
        M, G = np.empty((K, B1, d)), np.empty((K, B1, B1))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_harmony_ridge_moments(self._ctx, M.ctypes.data_as(dblp), G.ctypes.data_as(dblp)))
        return M, G

    def harmony_ridge_apply(self, W):
        har = self._har_state()
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.shape != (har["K"], har["B"] + 1, har["d"]):
            raise ValueError("W %s, expected %s" % (W.shape, (har["K"], har["B"] + 1, har["d"])))
        self._check(self._lib.cnmf_harmony_ridge_apply(self._ctx, W.ctypes.data_as(C.POINTER(C.c_double))))

    def harmony_fetch(self, z_cos_only=False):
        """(Z_corr [d][N], Z_cos [d][N], R [K][N], Y [d][K]); ``z_cos_only``: Z_cos alone."""
        har = self._har_state()
        N, d, K = har["N"], har["d"], har["K"]
        dblp = C.POINTER(C.c_double)
        Zs = np.empty((d, N))
        if z_cos_only:
            self._check(self._lib.cnmf_harmony_fetch(self._ctx, None, Zs.ctypes.data_as(dblp), None, None))
            return Zs
        Zc, R, Y = np.empty((d, N)), np.empty((K, N)), np.empty((d, K))
        self._check(self._lib.cnmf_harmony_fetch(self._ctx, Zc.ctypes.data_as(dblp), Zs.ctypes.data_as(dblp),
                                                 R.ctypes.data_as(dblp), Y.ctypes.data_as(dblp)))
        return Zc, Zs, R, Y

    @staticmethod
    def kmeans_uniforms(K, n_init, random_state):
        """The doubles scikit-learn's KMeans(k-means++) draws from RandomState(random_state), [n_init][1 + (K - 1) L]:
        per init one for the first centre, then L = 2 + int(ln K) local trials per further centre.  The count does not
        depend on the data, so the whole stream is drawn up front."""
        L = 2 + int(np.log(K))
        per_init = 1 + (K - 1) * L
        return np.random.RandomState(random_state).random_sample(n_init * per_init).reshape(n_init, per_init)

    def harmony_kmeans_init(self, random_state, n_init=10, max_iter=25, tol=1e-4, init_centers=None):
        """scikit-learn's KMeans(K, init='k-means++', n_init, max_iter, tol, random_state) on the unit scores of
        harmony_begin, on the device (harmony_init_host.hip.h); the same bits on every run.  ``init_centers``
        [n_init][K][d]: Lloyd starts from these centres instead of k-means++ (``random_state`` is not used).
        Returns ``(Y [d][K], labels [N], inertia [n_init], n_iter [n_init], best)``: the centres (not normalised) and
        labels of the best init, every init's inertia and iteration count, the index of the best.  Harmony's own state
        (R, E, O) is left as it is.  With fewer distinct cells than clusters the surplus centres are unspecified."""
        har = self._har_state()
        N, d, K = har["N"], har["d"], har["K"]
        n_init, max_iter = int(n_init), int(max_iter)
        if not 1 <= n_init <= 16 or max_iter < 1:
            raise ValueError("n_init = %d outside [1, 16] or max_iter = %d below 1" % (n_init, max_iter))
        if K > N:
            raise ValueError("K = %d clusters for %d cells" % (K, N))
        dblp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        u = c0 = None
        if init_centers is not None:
            c0 = np.ascontiguousarray(init_centers, dtype=np.float64)
            if c0.shape != (n_init, K, d) or not np.isfinite(c0).all():
                raise ValueError("init_centers %s, expected %s (finite values)" % (c0.shape, (n_init, K, d)))
        else:
            u = self.kmeans_uniforms(K, n_init, random_state)
        Y, labels = np.empty((d, K)), np.empty(N, dtype=np.int32)
        inertia, n_iter, best = np.empty(n_init), np.empty(n_init, dtype=np.int32), C.c_int32(-1)
        self._check(self._lib.cnmf_harmony_kmeans_init(
            self._ctx, n_init, max_iter, float(tol), None if u is None else u.ctypes.data_as(dblp),
            None if c0 is None else c0.ctypes.data_as(dblp), Y.ctypes.data_as(dblp), labels.ctypes.data_as(i32p),
            inertia.ctypes.data_as(dblp), n_iter.ctypes.data_as(i32p), C.byref(best)))
        return Y, labels, inertia, n_iter, int(best.value)

    def harmony_release(self):
        self._check(self._lib.cnmf_harmony_release(self._ctx))
        self._har = None

    def preprocess_row_sums(self):
        """Row sums [N] of the staged counts (the sums normalize_total divides by)."""
        rs = np.empty(self._pre["N"])
        self._check(self._lib.cnmf_preprocess_row_sums(self._ctx, rs.ctypes.data_as(C.POINTER(C.c_double))))
        return rs

    def preprocess_normalize_dense(self, slot, target_sum=0.0, max_value=None):
        """``slot`` := all genes of the staged counts, dense (rows scaled to ``target_sum`` when > 0), each column divided
        by its ddof=1 std summed row after row (numpy's order for a C-ordered matrix; 1 for a zero std), clipped at
        ``max_value``.  Returns the std."""
        G = self._pre.get("G")
        std = np.empty(G)
        mv = np.inf if max_value is None else float(max_value)
        self._check(self._lib.cnmf_preprocess_normalize_dense(self._ctx, int(slot), float(target_sum), mv,
                                                              std.ctypes.data_as(C.POINTER(C.c_double))))
        self._pre[int(slot)] = (G, -2)
        return std

    def preprocess_select_mi(self, slot, cls, n_classes, n_neighbors, state, psi, cst):
        """sklearn's mutual_info_classif over the dense ``slot`` (select_mi_host.hip.h): ``cls`` [N] class ids (-1:
        dropped), ``state`` numpy's RandomState state to draw the noise from, ``psi`` [N + 1] digamma(0..N), ``cst`` the
        gene-independent terms.  Returns (mi [n], the RandomState state after the draws)."""
        n = self._pre[int(slot)][0]
        cls = np.ascontiguousarray(cls, dtype=np.int32)
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        if cls.shape != (self._pre["N"],) or psi.shape != (self._pre["N"] + 1,):
            raise ValueError("cls [%d] / psi [%d] for %d cells" % (cls.size, psi.size, self._pre["N"]))
        st = _lib.MtState.from_numpy(state)
        mi = np.empty(n)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_select_mi(self._ctx, int(slot), cls.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        int(n_classes), int(n_neighbors), C.byref(st),
                                                        psi.ctypes.data_as(dblp), float(cst), mi.ctypes.data_as(dblp)))
        return mi, st.to_numpy()

    # ---- filters over the staged counts (filter_host.hip.h): Preprocess.filter_adata / preprocess_for_cnmf
    def preprocess_upload_as_stored(self, counts):
        """Stage a scipy CSR exactly as it is stored: rows may list their (distinct) columns in any order and zeros may
        be stored.  Returns the CSR that was staged."""
        import scipy.sparse as sp
        X = sp.csr_matrix(counts)
        vals = np.ascontiguousarray(X.data, dtype=np.float64)
        indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_upload_csr_as_stored(self._ctx, indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                   indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                   vals.ctypes.data_as(dblp), X.shape[0], X.shape[1]))
        self._pre = {"N": X.shape[0], "G": X.shape[1], 0: None, 1: None}
        return X

    def _pre_mask(self, mask, axis, name):
        """(the bytes of a boolean mask over the staged cells 'N' / genes 'G', their pointer); None: (None, None)"""
        if getattr(self, "_pre", None) is None or self._pre.get("G") is None:
            raise RuntimeError("preprocess_upload has not been called")
        if mask is None:
            return None, None
        m = np.asarray(mask)
        if m.dtype != bool or m.shape != (self._pre[axis],):
            raise ValueError("%s must be a boolean mask of length %d (got %s of shape %s)"
                             % (name, self._pre[axis], m.dtype, m.shape))
        m = np.ascontiguousarray(m, dtype=np.uint8)
        return m, m.ctypes.data_as(C.POINTER(C.c_uint8))

    def preprocess_gene_detect(self, cell_mask=None):
        """Per staged gene, over the cells of ``cell_mask`` (None: all): the number of stored entries > 0 (int64) and the
        sum of its entries.  Returns ``(n_cells, totals)``."""
        m, mp = self._pre_mask(cell_mask, "N", "cell_mask")
        G = self._pre["G"]
        n_cells, totals = np.empty(G, dtype=np.int64), np.empty(G)
        self._check(self._lib.cnmf_preprocess_gene_detect(self._ctx, mp, n_cells.ctypes.data_as(C.POINTER(C.c_int64)),
                                                          totals.ctypes.data_as(C.POINTER(C.c_double))))
        return n_cells, totals

    def preprocess_cell_sums(self, gene_mask=None):
        """Per staged cell, the sum of its entries over the genes of ``gene_mask`` (None: all -- preprocess_row_sums)."""
        m, mp = self._pre_mask(gene_mask, "G", "gene_mask")
        sums = np.empty(self._pre["N"])
        self._check(self._lib.cnmf_preprocess_cell_sums(self._ctx, mp, sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def preprocess_subset(self, keep_cells=None, keep_genes=None):
        """The staged counts := their restriction to the kept cells and genes (on the device; stored order kept); both
        result slots are released.  Returns the new ``(n_cells, n_genes, nnz)``."""
        mc, mcp = self._pre_mask(keep_cells, "N", "keep_cells")
        mg, mgp = self._pre_mask(keep_genes, "G", "keep_genes")
        n, g, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.cnmf_preprocess_subset(self._ctx, mcp, mgp, C.byref(n), C.byref(g), C.byref(nnz)))
        self._pre = {"N": int(n.value), "G": int(g.value), 0: None, 1: None}
        return int(n.value), int(g.value), int(nnz.value)

    def preprocess_fetch_counts(self, target_sum=0.0):
        """The staged counts as a scipy CSR, as stored; ``target_sum > 0``: every cell scaled to that total
        (sc.pp.normalize_total over all staged genes; a cell without counts stays 0)."""
        import scipy.sparse as sp
        self._pre_mask(None, "N", "")
        N, G = self._pre["N"], self._pre["G"]
        i64p = C.POINTER(C.c_int64)
        indptr = np.empty(N + 1, dtype=np.int64)
        self._check(self._lib.cnmf_preprocess_fetch_counts(self._ctx, 0.0, indptr.ctypes.data_as(i64p), None, None))
        nnz = int(indptr[-1])
        indices, data = np.empty(max(nnz, 1), dtype=np.int32), np.empty(max(nnz, 1))
        self._check(self._lib.cnmf_preprocess_fetch_counts(self._ctx, float(target_sum), None,
                                                           indices.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           data.ctypes.data_as(C.POINTER(C.c_double))))
        if nnz < (1 << 31):
            indptr = indptr.astype(np.int32)
        return sp.csr_matrix((data[:nnz], indices[:nnz].astype(indptr.dtype), indptr), shape=(N, G))

    # ---- the device steps of Preprocess.highly_variable_genes (hvg_host.hip.h)
    def preprocess_gene_moments(self):
        """Per staged gene, over the staging as it is now: S1 = sum x and S2 = sum x^2 as exact int64.  Returns
        ``(s1, s2, flags)``: flags bit 0 = a negative, non-integer or non-finite value was met, bit 1 = a count above
        2^20 (both kinds are left out of the sums)."""
        self._pre_mask(None, "G", "")
        G = self._pre["G"]
        s1, s2, flags = np.empty(G, dtype=np.int64), np.empty(G, dtype=np.int64), C.c_int32(0)
        i64p = C.POINTER(C.c_int64)
        self._check(self._lib.cnmf_preprocess_gene_moments(self._ctx, s1.ctypes.data_as(i64p), s2.ctypes.data_as(i64p),
                                                           C.byref(flags)))
        return s1, s2, int(flags.value)

    def preprocess_loess_fit(self, x, y, q, x0):
        """The local quadratic fits of loess(degree=2) at the points ``x0`` over the points (``x`` sorted ascending,
        ``y``), each over its ``q`` nearest abscissae with tricube weights.  Returns ``(value, slope, status)`` per
        point: status 0, 1 (zero-width neighbourhood) or 2 (fewer than three distinct weighted abscissae, or nearly so);
        value and slope are 0 where the status is not 0.  The same bits on every call.  Needs no staging."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x.ndim != 1 or y.shape != x.shape or x0.ndim != 1 or not 1 <= int(q) <= x.size:
            raise ValueError("loess_fit: x %s, y %s, x0 %s, q = %s" % (x.shape, y.shape, x0.shape, q))
        m = x0.size
        value, slope, status = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.int32)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_loess_fit(self._ctx, x.size, x.ctypes.data_as(dblp), y.ctypes.data_as(dblp),
                                                        int(q), m, x0.ctypes.data_as(dblp), value.ctypes.data_as(dblp),
                                                        slope.ctypes.data_as(dblp),
                                                        status.ctypes.data_as(C.POINTER(C.c_int32))))
        return value, slope, status

    def preprocess_clipped_sums(self, clip):
        """Per staged gene: ``(C1, C2)``, the sums of min(x, clip[gene]) and of its square over the gene's entries."""
        self._pre_mask(None, "G", "")
        G = self._pre["G"]
        clip = np.ascontiguousarray(clip, dtype=np.float64)
        if clip.shape != (G,) or not np.isfinite(clip).all():
            raise ValueError("clip must hold %d finite values (got shape %s)" % (G, clip.shape))
        c1, c2 = np.empty(G), np.empty(G)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_clipped_sums(self._ctx, clip.ctypes.data_as(dblp), c1.ctypes.data_as(dblp),
                                                           c2.ctypes.data_as(dblp)))
        return c1, c2

    # ---- the same two passes per batch (hvg_batch_host.hip.h): Preprocess.highly_variable_genes(batch_key=...)
    def _pre_batches(self, codes, n_batches):
        """(int32 codes over the staged cells, B) after the checks the library would refuse them with"""
        self._pre_mask(None, "G", "")
        N, G, B = self._pre["N"], self._pre["G"], int(n_batches)
        codes = np.asarray(codes)
        if codes.shape != (N,) or codes.dtype.kind not in "iu":
            raise ValueError("codes must hold %d integers (got %s of shape %s)" % (N, codes.dtype, codes.shape))
        if not 1 <= B <= _lib.CNMF_HVG_BATCHES_MAX:
            raise NotImplementedError("%d batches: between 1 and %d are supported" % (B, _lib.CNMF_HVG_BATCHES_MAX))
        if G * B > _lib.CNMF_HVG_PAIRS_MAX:
            raise NotImplementedError("%d genes x %d batches: more than %d (gene, batch) pairs"
                                      % (G, B, _lib.CNMF_HVG_PAIRS_MAX))
        if codes.min() < 0 or codes.max() >= B:
            raise ValueError("batch codes outside [0, %d)" % B)
        empty = np.flatnonzero(np.bincount(codes, minlength=B) == 0)
        if empty.size:
            raise ValueError("batch %d has no cell" % empty[0])
        return np.ascontiguousarray(codes, dtype=np.int32), B

    def preprocess_gene_moments_batched(self, codes, n_batches):
        """``preprocess_gene_moments`` per batch: ``codes`` [N] the batch of every staged cell, in [0, n_batches), every
        batch with at least one cell.  Returns ``(s1 [B][G], s2 [B][G], flags [B])``: row b is what
        ``preprocess_gene_moments`` gives on the staging restricted to the cells of batch b.  The staging is not
        changed.  More than 4096 batches, or more than 2^26 (gene, batch) pairs: NotImplementedError."""
        codes, B = self._pre_batches(codes, n_batches)
        G = self._pre["G"]
        s1, s2 = np.empty((B, G), dtype=np.int64), np.empty((B, G), dtype=np.int64)
        flags = np.zeros(B, dtype=np.int32)
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        self._check(self._lib.cnmf_preprocess_gene_moments_batched(self._ctx, codes.ctypes.data_as(i32p), B,
                                                                   s1.ctypes.data_as(i64p), s2.ctypes.data_as(i64p),
                                                                   flags.ctypes.data_as(i32p)))
        return s1, s2, flags

    def preprocess_clipped_sums_batched(self, codes, n_batches, clip):
        """``preprocess_clipped_sums`` per batch with ``clip`` [B][G]: ``(C1 [B][G], C2 [B][G])``, row b with the bits
        ``preprocess_clipped_sums(clip[b])`` gives on the staging restricted to the cells of batch b."""
        codes, B = self._pre_batches(codes, n_batches)
        G = self._pre["G"]
        clip = np.ascontiguousarray(clip, dtype=np.float64)
        if clip.shape != (B, G) or not np.isfinite(clip).all():
            raise ValueError("clip must hold %d x %d finite values (got shape %s)" % (B, G, clip.shape))
        c1, c2 = np.empty((B, G)), np.empty((B, G))
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_preprocess_clipped_sums_batched(self._ctx, codes.ctypes.data_as(C.POINTER(C.c_int32)), B,
                                                                   clip.ctypes.data_as(dblp), c1.ctypes.data_as(dblp),
                                                                   c2.ctypes.data_as(dblp)))
        return c1, c2

    def preprocess_release(self):
        self._check(self._lib.cnmf_preprocess_release(self._ctx))
        self._pre = None

    @property
    def x_mean(self):
        if self._x_mean is None and self._x_mean_src is not None:
            X = self._x_mean_src
            self._x_mean = X.mean() if X.dtype in (np.float32, np.float64) else X.astype(np.float64).mean()
            self._x_mean_src = None
        return self._x_mean

    @x_mean.setter
    def x_mean(self, v):
        self._x_mean, self._x_mean_src = v, None

    def init_scale(self, k):
        """``avg = sqrt(X.mean() / n_components)`` exactly as sklearn computes it
        (numpy scalar arithmetic in X's dtype; decomposition/_nmf.py:303)."""
        return float(np.sqrt(self.x_mean / k))

    # ------------------------------------------------------------------ restarts
    def nmf_batch(self, ks, seeds=None, W0=None, H0=None, tol=1e-4, max_iter=1000,
                  alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, return_W=False, kc_max=0, lag=0,
                  resident=False, warn=True, profile=False, init_store=False):
        """Run ``len(ks)`` independent CD-NMF restarts on the resident matrix.

        Either ``seeds`` (sklearn ``init='random'`` reproduced on the device) or the lists
        ``W0`` / ``H0`` of explicit initial factors (sklearn layouts N x k and k x G), or ``init_store=True``: the start
        factors ``nndsvd_init_batch(ks, ..., tail="device", keep=True)`` left in the context's init store for the same
        ``ks`` (no transfer; the restarts run in the store's order, the results come back in the caller's).
        Returns ``(H_list, W_list_or_None, n_iter, violation)``."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        ks = np.ascontiguousarray(ks, dtype=np.int32).ravel()
        n = int(ks.size)
        if n and ks.min() < 1:
            raise ValueError("n_components must be >= 1")
        prm = self._params(tol, max_iter, alpha_W, alpha_H, l1_ratio, kc_max, lag, profile)
        i32p, u32p, dblp = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        perm = None
        if init_store:
            perm = self._init_store_perm(n)
            ks = np.ascontiguousarray(ks[perm])
            mode, w0p, h0p, seedp, avgp = 2, None, None, None, None
        elif seeds is not None:
            seeds_a = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).astype(np.uint32)).ravel()
            if seeds_a.size != n:
                raise ValueError("need one seed per restart")
            avg = np.ascontiguousarray([self.init_scale(int(k)) for k in ks], dtype=np.float64)
            mode, w0p, h0p = 1, None, None
            seedp, avgp = seeds_a.ctypes.data_as(u32p), avg.ctypes.data_as(dblp)
        else:
            if W0 is None or H0 is None or len(W0) != n or len(H0) != n:
                raise ValueError("need seeds, or W0 and H0 lists with one entry per restart")
            for r in range(n):
                if np.shape(W0[r]) != (N, ks[r]) or np.shape(H0[r]) != (ks[r], G):
                    raise ValueError("Array with wrong shape passed to NMF (input W/H) for restart %d" % r)
                if np.min(W0[r]) < 0 or np.min(H0[r]) < 0:
                    raise ValueError("Negative values in data passed to NMF (input W/H)")
            w0 = (np.concatenate([np.ascontiguousarray(w, dtype=np.float32).ravel() for w in W0])
                  if n else np.zeros(1, np.float32))
            h0 = (np.concatenate([np.ascontiguousarray(h, dtype=np.float32).ravel() for h in H0])
                  if n else np.zeros(1, np.float32))
            mode, w0p, h0p, seedp, avgp = 0, _fp(w0), _fp(h0), None, None
        tot_k = int(ks.sum()) if n else 0
        n_iter = np.zeros(max(n, 1), dtype=np.int32)
        viol = np.zeros(max(n, 1), dtype=np.float64)
        stats = _lib.BatchStats()
        if resident:
            # the spectra stay in the context's device store (appended behind what it holds); resident="keep" also
            # brings THIS call's rows to the host (ONE copy), and `last_store_offsets` says where each restart sits in the
            # store -- consensus() / kselect_stats() can then take their merged spectra from the device (store_rows)
            row0 = self.spectra_rows
            rc = self._lib.cnmf_nmf_cd_batch_resident(self._ctx, n, ks.ctypes.data_as(i32p), mode, seedp,
                                                      avgp, w0p, h0p, C.byref(prm),
                                                      n_iter.ctypes.data_as(i32p), viol.ctypes.data_as(dblp),
                                                      C.byref(stats))
            self._check(rc)
            H_list = W_list = None
            offs = row0 + np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
            self.last_store_offsets = offs[:-1].copy()
            if perm is not None:
                self.last_store_offsets[perm] = offs[:-1]
            self.last_store_gen = self.store_gen
            if resident == "keep":
                if return_W:
                    raise ValueError("resident='keep' returns spectra only")
                mine = self.spectra_fetch(row0, tot_k)            # THIS call's rows only (ONE copy)
                H_list = [mine[offs[r] - row0:offs[r + 1] - row0] for r in range(n)]
        else:
            H_out = np.empty((max(tot_k, 1), G), dtype=np.float32)
            W_out = np.empty(max(tot_k, 1) * N, dtype=np.float32) if return_W else None
            rc = self._lib.cnmf_nmf_cd_batch(self._ctx, n, ks.ctypes.data_as(i32p), mode, seedp, avgp,
                                             w0p, h0p, C.byref(prm), _fp(H_out),
                                             _fp(W_out) if return_W else None,
                                             n_iter.ctypes.data_as(i32p), viol.ctypes.data_as(dblp),
                                             C.byref(stats))
            self._check(rc)
            offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
            H_list = [H_out[offs[r]:offs[r + 1]] for r in range(n)]
            W_list = None
            if return_W:
                W_list = [W_out[offs[r] * N:offs[r + 1] * N].reshape(N, ks[r]) for r in range(n)]
        self.last_stats = stats.as_dict()
        n_iter, viol = n_iter[:n], viol[:n]
        if perm is not None:                                  # back to the caller's order
            n_iter, viol = self._unpermute(n_iter, perm), self._unpermute(viol, perm)
            H_list = self._unpermute(H_list, perm) if H_list is not None else None
            W_list = self._unpermute(W_list, perm) if W_list is not None else None
        if warn and n and tol > 0 and (n_iter == max_iter).any():
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return H_list, W_list, n_iter, viol

    last_init_store_order = None       # restart index of every entry of the init store (nndsvd_init_batch(keep=True))

    def _init_store_perm(self, n):
        """Order in which a batch call that starts from the init store runs the caller's ``n`` restarts (the library
        refuses a store that does not hold exactly their ranks: ValueError)."""
        order = self.last_init_store_order
        if order is None or len(order) != n:
            return np.arange(n, dtype=np.int64)
        return np.asarray(order, dtype=np.int64)

    @staticmethod
    def _unpermute(vals, perm):
        if isinstance(vals, np.ndarray):
            out = np.empty_like(vals)
            out[perm] = vals
            return out
        out = [None] * len(vals)
        for i, r in enumerate(perm):
            out[int(r)] = vals[i]
        return out

    def iteration_means(self):
        """``{rank: mean outer iterations}`` of the restarts the batch calls on the resident matrix have run so far."""
        out = np.zeros(_lib.CNMF_KMAX + 1, dtype=np.float64)
        self._check(self._lib.cnmf_get_iteration_means(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return {int(k): float(v) for k, v in enumerate(out) if v > 0}

    def set_iteration_hints(self, hints=None):
        """Expected iterations per rank (e.g. :meth:`iteration_means` of an earlier call) for the queue order of the following
        ``nmf_batch`` calls on this matrix -- longest-expected-first from the start instead of learning the order again;
        ``None`` clears them.  Explicit by design: the order decides which packed columns a restart occupies, and its
        float32 result moves in the last bits with its placement."""
        hints = hints or {}
        ks = np.ascontiguousarray(sorted(hints), dtype=np.int32)
        vals = np.ascontiguousarray([hints[int(k)] for k in ks], dtype=np.float64)
        self._check(self._lib.cnmf_set_iteration_hints(self._ctx, int(ks.size), ks.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       vals.ctypes.data_as(C.POINTER(C.c_double))))

    # ------------------------------------------------------------------ multiplicative update
    _BETA = {"kullback-leibler": 1, "itakura-saito": 0, 1: 1, 0: 0, 1.0: 1, 0.0: 0}

    def nmf_mu_batch(self, ks, seeds=None, W0=None, H0=None, beta_loss="kullback-leibler", tol=1e-4,
                     max_iter=1000, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, return_W=False, warn=True, init_store=False):
        """``solver='mu'`` restarts (the reference's path for beta_loss != 'frobenius',
        cnmf.py:618-631).  Same arguments / returns as :meth:`nmf_batch` (``init_store=True`` included); the last element
        of the returned tuple is sqrt(2*beta-divergence) at the final evaluation.  Ranks above :attr:`mu_rank_limit`
        (64 unless raised to 128) raise NotImplementedError.  Kullback-Leibler restarts on a matrix that is at most a quarter
        non-zero (or under ``CNMF_MU_SPARSE=1``) run on the stored entries only, at ranks up to
        :attr:`mu_sparse_rank_limit` (32 unless raised to 64; ranks 33..64 by themselves at up to 15 % non-zero); above it they
        run on the dense matrix-pipe kernels."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        if beta_loss not in self._BETA:
            raise NotImplementedError("beta_loss=%r is not implemented on the device" % (beta_loss,))
        self._refuse_zeros(beta_loss)
        N, G = self.shape
        ks = np.ascontiguousarray(ks, dtype=np.int32).ravel()
        n = int(ks.size)
        prm = self._params(tol, max_iter, alpha_W, alpha_H, l1_ratio)
        i32p, u32p, dblp = C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        perm = None
        if init_store:
            perm = self._init_store_perm(n)
            ks = np.ascontiguousarray(ks[perm])
        avg = np.ascontiguousarray([self.init_scale(int(k)) for k in ks], dtype=np.float64)
        if init_store:
            mode, w0p, h0p, seedp = 2, None, None, None
        elif seeds is not None:
            seeds_a = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).astype(np.uint32)).ravel()
            mode, w0p, h0p, seedp = 1, None, None, seeds_a.ctypes.data_as(u32p)
        else:
            w0 = np.concatenate([np.ascontiguousarray(w, dtype=np.float32).ravel() for w in W0])
            h0 = np.concatenate([np.ascontiguousarray(h, dtype=np.float32).ravel() for h in H0])
            mode, w0p, h0p, seedp = 0, _fp(w0), _fp(h0), None
        tot_k = int(ks.sum()) if n else 0
        H_out = np.empty((max(tot_k, 1), G), dtype=np.float32)
        W_out = np.empty(max(tot_k, 1) * N, dtype=np.float32) if return_W else None
        n_iter = np.zeros(max(n, 1), dtype=np.int32)
        err = np.zeros(max(n, 1), dtype=np.float64)
        self._check(self._lib.cnmf_nmf_mu_batch(self._ctx, n, ks.ctypes.data_as(i32p), mode, seedp,
                                                avg.ctypes.data_as(dblp), w0p, h0p, self._BETA[beta_loss], 1,
                                                C.byref(prm), _fp(H_out), _fp(W_out) if return_W else None,
                                                n_iter.ctypes.data_as(i32p), err.ctypes.data_as(dblp)))
        offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
        H_list = [H_out[offs[r]:offs[r + 1]] for r in range(n)]
        W_list = [W_out[offs[r] * N:offs[r + 1] * N].reshape(N, ks[r]) for r in range(n)] if return_W else None
        n_iter, err = n_iter[:n], err[:n]
        if perm is not None:                                  # back to the caller's order
            n_iter, err = self._unpermute(n_iter, perm), self._unpermute(err, perm)
            H_list = self._unpermute(H_list, perm)
            W_list = self._unpermute(W_list, perm) if W_list is not None else None
        if warn and n and tol > 0 and (n_iter == max_iter).any():
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return H_list, W_list, n_iter, err

    def nnls_mu(self, H, beta_loss="kullback-leibler", tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0,
                warn=True):
        """Refit with fixed H and ``solver='mu'``: W starts from avg everywhere (sklearn _nmf.py:1229-1231).
        Both losses: the float64 refit on the stored entries (:meth:`mu_refit_f64`; result cast to float32 like the
        other refits of this class).  Ranks above :attr:`mu_rank_limit` (64 unless raised to 128): NotImplementedError.
        The float64 refit walks the stored entries at every rank: :attr:`mu_sparse_rank_limit` does not bear on it."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        H = np.asarray(H)
        if H.ndim != 2 or H.shape[1] != G:
            raise ValueError("Array with wrong shape passed to NMF (input H).")
        if H.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if H.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        W, n, _ = self.mu_refit_f64(H, tol=tol, max_iter=max_iter, alpha_W=alpha_W, l1_ratio=l1_ratio, warn=warn,
                                    beta_loss=beta_loss)
        return W.astype(np.float32), n

    _ZERO_MSG = ("When beta_loss <= 0 and X contains zeros, the solver may diverge. Please add small values to X, or use a "
                 "positive beta_loss.")

    def _refuse_zeros(self, beta_loss):
        """scikit-learn's own refusal (``_fit_transform``, _nmf.py:1679-1684): ``beta_loss <= 0`` on a matrix that contains a
        zero raises ValueError -- what the reference's ``factorize`` / ``refit_usage`` do for every ordinary count matrix under
        ``--beta-loss itakura-saito``."""
        if self._BETA[beta_loss] <= 0 and self.x_has_zero:
            raise ValueError(self._ZERO_MSG)

    def mu_refit_f64(self, H, transposed=False, col_divisor=None, w_init=None, tol=1e-4, max_iter=1000, alpha_W=0.0,
                     l1_ratio=0.0, n_features=None, warn=True, beta_loss="kullback-leibler"):
        """``non_negative_factorization(X, H=H, update_H=False, solver='mu', beta_loss=...)`` in float64 on
        the stored entries of the resident matrix (cnmf_mu_refit_f64): returns ``(W float64, n_iter, err)``.
        ``beta_loss='itakura-saito'`` (round 6): the matrix must be strictly positive (scikit-learn's rule), so every entry
        is a stored entry.  ``H`` has at most :attr:`mu_rank_limit` rows (64 unless raised to 128), else NotImplementedError.

        ``transposed=False``: X = the resident cells x genes matrix, ``H`` [k, n_genes], W [n_cells, k] (refit_usage,
        cnmf.py:776-802).  ``transposed=True``: the problem on X^T -- ``H`` [k, n_cells] (usages^T), W [n_genes, k]
        (refit_spectra, cnmf.py:805-820) -- on the compressed rows of X^T built on the device.
        ``col_divisor`` [columns of the walked matrix]: the matrix meant is ``X[:, d != 0] / d[d != 0]`` (the final usage
        refit on the unit-variance high-variance-gene TPM, cnmf.py:963-972); then ``w_init`` (scikit-learn's
        sqrt(mean / k) of THAT matrix) must be given and ``n_features`` is its column count (scales the W penalties)."""
        self._sync_env()
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        if beta_loss not in self._BETA:
            raise NotImplementedError("beta_loss=%r is not implemented on the device" % (beta_loss,))
        self._refuse_zeros(beta_loss)
        N, G = self.shape
        rows, cols = (G, N) if transposed else (N, G)
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim != 2 or H.shape[1] != cols:
            raise ValueError("Array with wrong shape passed to NMF (input H). Expected (k, %d), but got %s"
                             % (cols, (H.shape,)))
        if not np.isfinite(H).all():
            raise ValueError("Input H contains NaN or infinity.")
        if H.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if H.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        k = int(H.shape[0])
        dblp = C.POINTER(C.c_double)
        div = None
        if col_divisor is not None:
            div = np.ascontiguousarray(col_divisor, dtype=np.float64)
            if div.shape != (cols,) or w_init is None:
                raise ValueError("col_divisor needs one entry per column of the walked matrix and an explicit w_init")
        if w_init is None:
            w_init = self.init_scale(k)
        # scikit-learn scales the W penalties by the FEATURE count of the matrix it is given (_nmf.py:1254-1265)
        feats = cols if n_features is None else int(n_features)
        l1W, _, l2W, _ = regularization(rows, feats, alpha_W, 0.0, l1_ratio)
        prm = _lib.CdParams(float(tol), int(max_iter), 0, l1W, l2W, 0.0, 0.0, 0, 0)
        W = np.empty((rows, k), dtype=np.float64)
        n_iter = C.c_int32(0)
        err = C.c_double(0.0)
        self._check(self._lib.cnmf_mu_refit_f64(self._ctx, 1 if transposed else 0, self._BETA[beta_loss], k, H.ctypes.data_as(dblp),
                                                div.ctypes.data_as(dblp) if div is not None else None, float(w_init),
                                                C.byref(prm), W.ctypes.data_as(dblp), C.byref(n_iter), C.byref(err)))
        if warn and tol > 0 and n_iter.value == max_iter:
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return W, int(n_iter.value), float(err.value)

    def mu_frobenius_refit(self, H, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0, w_init=None, n_features=None,
                           warn=True):
        """``non_negative_factorization(X, H=H, update_H=False, solver='mu', beta_loss='frobenius')`` in float64 on the
        dense image of the resident matrix (cnmf_mu2_refit_f64) -- the refit starCAT projects query cells with: returns
        ``(W float64 [N, k], n_iter, err)``, ``err`` the last error the stopping rule evaluated (the error at the start when
        no check ran).  W starts from ``w_init`` everywhere (default: scikit-learn's ``sqrt(X.mean() / k)``);
        ``n_features`` scales the W penalties as in :meth:`mu_refit_f64`.  Ranks above CNMF_KMAX: NotImplementedError.
        Timed once (a single measurement, profiles/starcat_probe_50000x2000.json): 2.2 ms for the whole call at
        50 000 x 2 000, k = 9 (30 iterations), what :meth:`nnls_f64` took on the same resident matrix (11 sweeps)."""
        self._sync_env()
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim != 2 or H.shape[1] != G:
            raise ValueError("Array with wrong shape passed to NMF (input H). Expected (k, %d), but got %s"
                             % (G, (H.shape,)))
        if not np.isfinite(H).all():
            raise ValueError("Input H contains NaN or infinity.")
        if H.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if H.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        k = int(H.shape[0])
        if w_init is None:
            w_init = self.init_scale(k)
        l1W, _, l2W, _ = regularization(N, G if n_features is None else int(n_features), alpha_W, 0.0, l1_ratio)
        prm = _lib.CdParams(float(tol), int(max_iter), 0, l1W, l2W, 0.0, 0.0, 0, 0)
        dblp = C.POINTER(C.c_double)
        W = np.empty((N, k), dtype=np.float64)
        n_iter = C.c_int32(0)
        err = C.c_double(0.0)
        self._check(self._lib.cnmf_mu2_refit_f64(self._ctx, k, H.ctypes.data_as(dblp), float(w_init), C.byref(prm),
                                                 W.ctypes.data_as(dblp), C.byref(n_iter), C.byref(err)))
        if warn and tol > 0 and n_iter.value == max_iter:
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return W, int(n_iter.value), float(err.value)

    # ------------------------------------------------------------------ NNLS refit
    def nnls(self, H, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0, warn=True):
        """``non_negative_factorization(X, H=H, update_H=False, solver='cd')`` on the
        resident matrix: returns ``(W [N x k], n_iter)``."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        H = np.asarray(H)
        if H.ndim != 2 or H.shape[1] != G:
            raise ValueError("Array with wrong shape passed to NMF (input H). Expected (k, %d), but got %s"
                             % (G, (H.shape,)))
        if not np.isfinite(H).all():
            raise ValueError("Input H contains NaN or infinity.")
        if H.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if H.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        k = int(H.shape[0])
        Hf = np.ascontiguousarray(H, dtype=np.float32)
        prm = self._params(tol, max_iter, alpha_W, 0.0, l1_ratio)
        W = np.empty((N, k), dtype=np.float32)
        n_iter = C.c_int32(0)
        viol = C.c_double(0.0)
        self._check(self._lib.cnmf_nnls(self._ctx, k, _fp(Hf), C.byref(prm), _fp(W),
                                        C.byref(n_iter), C.byref(viol)))
        if warn and tol > 0 and n_iter.value == max_iter:
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return W, int(n_iter.value)

    # ------------------------------------------------------------------ consensus tail + k selection
    def _check_H(self, H, G):
        H = np.asarray(H)
        if H.ndim != 2 or H.shape[1] != G:
            raise ValueError("Array with wrong shape passed to NMF (input H). Expected (k, %d), but got %s"
                             % (G, (H.shape,)))
        if not np.isfinite(H).all():
            raise ValueError("Input H contains NaN or infinity.")
        if H.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if H.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        return H

    def nnls_batch(self, H_list, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0, return_W=True,
                   prediction_error=False):
        """Several usage refits (``cNMF.refit_usage``, cnmf.py:776-802) as ONE pass over the resident matrix:
        every ``H`` of ``H_list`` (k_r x G) becomes columns of a single X.H^T product, the W sweeps run together.
        Returns ``(W_list or None, n_iter, errors or None)`` -- ``errors[r] = ||X - W_r H_r||_F^2`` in float64."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        Hs = [np.ascontiguousarray(self._check_H(H, G), dtype=np.float32) for H in H_list]
        n = len(Hs)
        ks = np.ascontiguousarray([h.shape[0] for h in Hs], dtype=np.int32)
        if n == 0:
            return ([] if return_W else None), np.zeros(0, np.int32), (np.zeros(0) if prediction_error else None)
        Hp = np.ascontiguousarray(np.concatenate(Hs, axis=0))
        prm = self._params(tol, max_iter, alpha_W, 0.0, l1_ratio)
        W_out = np.empty(int(ks.sum()) * N, dtype=np.float32) if return_W else None
        n_iter = np.zeros(n, dtype=np.int32)
        viol = np.zeros(n, dtype=np.float64)
        err = np.zeros(n, dtype=np.float64) if prediction_error else None
        i32p, dblp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        self._check(self._lib.cnmf_nnls_batch(self._ctx, n, ks.ctypes.data_as(i32p), _fp(Hp), C.byref(prm),
                                              _fp(W_out) if return_W else None, n_iter.ctypes.data_as(i32p),
                                              viol.ctypes.data_as(dblp),
                                              err.ctypes.data_as(dblp) if prediction_error else None))
        W_list = None
        if return_W:
            offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
            W_list = [W_out[offs[r] * N:offs[r + 1] * N].reshape(N, ks[r]) for r in range(n)]
        return W_list, n_iter, err

    def nnls_gram(self, H_prod, gram, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0, n_features=None):
        """Usage refit whose product uses the rows ``H_prod`` (k x G) but whose Gram matrix is GIVEN
        (``gram`` k x k): ``X_sub @ H_sub.T`` for a scaled column subset of the resident matrix is
        ``X @ H_prod.T`` with ``H_prod`` zero outside the subset (cnmf.py:960-975 without a second upload).
        ``n_features`` = the size of that subset: the reference refits on ``tpm[:, hvgs]``, so scikit-learn scales
        ``alpha_W`` by the number of HVGs, not by the width of the resident TPM matrix."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        Hf = np.ascontiguousarray(self._check_H(H_prod, G), dtype=np.float32)
        k = int(Hf.shape[0])
        g = np.ascontiguousarray(gram, dtype=np.float32)
        if g.shape != (k, k):
            raise ValueError("gram must be (k, k)")
        prm = self._params(tol, max_iter, alpha_W, 0.0, l1_ratio, n_features=n_features)
        W = np.empty((N, k), dtype=np.float32)
        n_iter = C.c_int32(0)
        viol = C.c_double(0.0)
        self._check(self._lib.cnmf_nnls_gram(self._ctx, k, _fp(Hf), _fp(g), C.byref(prm), _fp(W), C.byref(n_iter),
                                             C.byref(viol)))
        return W, int(n_iter.value)

    def nnls_spectra(self, W, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0):
        """``cNMF.refit_spectra`` (cnmf.py:805-820): NNLS for the spectra (k x G) with the usages ``W`` (N x k)
        fixed, on the resident matrix -- no transposed upload.  ``alpha_W`` plays the role it has in the reference's
        transposed call (it regularises the solved factor, scaled by the N 'features' of X.T)."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[0] != N:
            raise ValueError("Array with wrong shape passed to NMF (input H). Expected (%d, k), but got %s" % (N, (W.shape,)))
        if not np.isfinite(W).all():
            raise ValueError("Input H contains NaN or infinity.")
        if W.min() < 0:
            raise ValueError("Negative values in data passed to NMF (input H)")
        if W.max() == 0:
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        k = int(W.shape[1])
        # the transposed problem has G samples and N features: l1_reg_W = N * alpha_W * l1_ratio (sklearn _nmf.py:1254)
        prm = _lib.CdParams(float(tol), int(max_iter), 0, N * alpha_W * l1_ratio, N * alpha_W * (1.0 - l1_ratio),
                            0.0, 0.0, 0, 0)
        H = np.empty((k, G), dtype=np.float64)
        n_iter = C.c_int32(0)
        viol = C.c_double(0.0)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_nnls_spectra(self._ctx, k, W.ctypes.data_as(dblp), C.byref(prm),
                                                H.ctypes.data_as(dblp), C.byref(n_iter), C.byref(viol)))
        return H, int(n_iter.value)

    def nnls_f64(self, H, gram=None, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0, n_features=None, warn=True):
        """``cnmf_nnls_f64``: the usage refit of :meth:`nnls` with the product ``X @ H.T``, the Gram matrix and the
        coordinate-descent sweeps in FLOAT64 -- what scikit-learn computes when the reference hands it float64 matrices
        (the reference's own tolerance on the consensus tail, sum(diff^2) < 1e-4 on TPM-scale values, needs it).
        ``gram`` (k x k): used instead of ``H @ H.T`` (see :meth:`nnls_gram`).  Returns ``(W [N x k] float64, n_iter)``."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        Hd = np.ascontiguousarray(self._check_H(H, G), dtype=np.float64)
        k = int(Hd.shape[0])
        dblp = C.POINTER(C.c_double)
        gp = None
        if gram is not None:
            gd = np.ascontiguousarray(gram, dtype=np.float64)
            if gd.shape != (k, k):
                raise ValueError("gram must be (k, k)")
            gp = gd.ctypes.data_as(dblp)
        prm = self._params(tol, max_iter, alpha_W, 0.0, l1_ratio, n_features=n_features)
        W = np.empty((N, k), dtype=np.float64)
        n_iter = C.c_int32(0)
        viol = C.c_double(0.0)
        self._check(self._lib.cnmf_nnls_f64(self._ctx, k, Hd.ctypes.data_as(dblp), gp, C.byref(prm),
                                            W.ctypes.data_as(dblp), C.byref(n_iter), C.byref(viol)))
        if warn and tol > 0 and n_iter.value == max_iter:
            warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence."
                          % max_iter, ConvergenceWarning)
        return W, int(n_iter.value)

    def xt_matmul_f64(self, W, mean=None, std=None):
        """``W.T @ X`` in float64, or ``W.T @ ((X - mean) / std)`` when ``mean``/``std`` (length G) are given --
        the X^T Y accumulation of ``efficient_ols_all_cols(normalize_y=True)`` (cnmf.py:55-125)."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[0] != N:
            raise ValueError("W must be (%d, k)" % N)
        k = int(W.shape[1])
        dblp = C.POINTER(C.c_double)
        zs = mean is not None
        out = np.empty((k, G), dtype=np.float64)
        if zs:
            mean = np.ascontiguousarray(mean, dtype=np.float64)
            inv = np.ascontiguousarray(1.0 / np.asarray(std, dtype=np.float64))
            self._check(self._lib.cnmf_xt_matmul_f64(self._ctx, k, W.ctypes.data_as(dblp), 1, mean.ctypes.data_as(dblp),
                                                     inv.ctypes.data_as(dblp), out.ctypes.data_as(dblp)))
        else:
            self._check(self._lib.cnmf_xt_matmul_f64(self._ctx, k, W.ctypes.data_as(dblp), 0, None, None,
                                                     out.ctypes.data_as(dblp)))
        return out

    def kselect_stats(self, spectra_by_k, local_neighborhood_size=0.30, random_state=1, n_init=10, max_iter=300,
                      kmeans_tol=1e-4, nnls_tol=1e-4, nnls_max_iter=1000, alpha_W=0.0, l1_ratio=0.0, store_rows_by_k=None):
        """The statistics loop of ``k_selection_plot`` (cnmf.py:1119-1135) in ONE device call: ``spectra_by_k`` maps
        k -> merged spectra (R_k x G).  Every k goes through the stats branch of the consensus (no density filter,
        KMeans, medians, silhouette), the |K| usage refits run batched (one pass over X), the prediction errors are
        computed with the usages still on the device.  Returns ``{k: dict(silhouette, prediction_error,
        median_spectra, nnls_iter)}``."""
        self._sync_env()
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        # ``store_rows_by_k`` (k -> row indices into the resident spectra store) replaces ``spectra_by_k``: nothing is uploaded
        src = store_rows_by_k if store_rows_by_k is not None else spectra_by_k
        ks = sorted(int(k) for k in src)
        n = len(ks)
        if store_rows_by_k is not None:
            if self.spectra_genes != G:
                raise ValueError("the resident store holds spectra over %d genes, the matrix has %d" % (self.spectra_genes, G))
            rows = [np.ascontiguousarray(store_rows_by_k[k], dtype=np.int64).ravel() for k in ks]
            R = np.ascontiguousarray([r.size for r in rows], dtype=np.int32)
            rows_all = np.ascontiguousarray(np.concatenate(rows))
        else:
            S = [np.ascontiguousarray(spectra_by_k[k], dtype=np.float64) for k in ks]
            for k, s in zip(ks, S):
                if s.ndim != 2 or s.shape[1] != G:
                    raise ValueError("spectra for k=%d must be (R, %d)" % (k, G))
            R = np.ascontiguousarray([s.shape[0] for s in S], dtype=np.int32)
            Sp = np.ascontiguousarray(np.concatenate(S, axis=0))
        cprm = (_lib.ConsensusParams * n)()
        us = []
        for i, k in enumerate(ks):
            L = 2 + int(np.log(k))
            us.append(np.random.RandomState(random_state).random_sample(n_init * (1 + (k - 1) * L)))
            cprm[i] = _lib.ConsensusParams(k, int(local_neighborhood_size * int(R[i]) / k), 2.0, 1, 1, int(n_init),
                                           int(max_iter), float(kmeans_tol))
        u = np.ascontiguousarray(np.concatenate(us))
        prm = self._params(nnls_tol, nnls_max_iter, alpha_W, 0.0, l1_ratio)
        ks_a = np.ascontiguousarray(ks, dtype=np.int32)
        sil = np.zeros(n)
        err = np.zeros(n)
        med = np.zeros((int(ks_a.sum()), G))
        nit = np.zeros(n, dtype=np.int32)
        i32p, dblp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        outs = (cprm, u.ctypes.data_as(dblp), C.byref(prm), sil.ctypes.data_as(dblp), err.ctypes.data_as(dblp),
                med.ctypes.data_as(dblp), nit.ctypes.data_as(i32p))
        if store_rows_by_k is not None:
            rc = self._lib.cnmf_kselect_stats_store(self._ctx, n, ks_a.ctypes.data_as(i32p), R.ctypes.data_as(i32p),
                                                    rows_all.ctypes.data_as(C.POINTER(C.c_int64)), *outs)
        else:
            rc = self._lib.cnmf_kselect_stats(self._ctx, n, ks_a.ctypes.data_as(i32p), R.ctypes.data_as(i32p),
                                              Sp.ctypes.data_as(dblp), *outs)
        self._check(rc)
        out, off = {}, 0
        for i, k in enumerate(ks):
            out[k] = dict(silhouette=float(sil[i]), prediction_error=float(err[i]), median_spectra=med[off:off + k],
                          nnls_iter=int(nit[i]))
            off += k
        return out

    # ------------------------------------------------------------------ NNDSVD init
    def x_matmul(self, Q, trans=False):
        """``X @ Q`` (trans=False, Q is G x c) or ``X.T @ Q`` (trans=True, Q is N x c) on the device."""
        N, G = self.shape
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[0] != (N if trans else G):
            raise ValueError("shape mismatch in x_matmul")
        out = np.empty(((G if trans else N), Q.shape[1]), dtype=np.float32)
        self._check(self._lib.cnmf_x_matmul(self._ctx, int(bool(trans)), _fp(Q), Q.shape[1], _fp(out)))
        return out

    def range_finder(self, Q0_blocks, n_iter, transpose):
        """``cnmf_range_finder``: the power iterations of sklearn's ``randomized_range_finder`` for a GROUP of Gaussian
        start blocks (list of [M_cols, c_b] arrays, sum c_b <= 256) entirely on the device; returns the lists
        ``Q_b`` ([M_rows, c_b], orthonormal columns) and ``B_b = Q_b.T @ M`` ([c_b, M_cols]) in float32."""
        N, G = self.shape
        M_rows, M_cols = (G, N) if transpose else (N, G)
        widths = np.ascontiguousarray([q.shape[1] for q in Q0_blocks], dtype=np.int32)
        Ctot = int(widths.sum())
        Q0 = np.ascontiguousarray(np.concatenate(Q0_blocks, axis=1), dtype=np.float32)
        if Q0.shape != (M_cols, Ctot):
            raise ValueError("start blocks must be [%d, c]" % M_cols)
        Q = np.empty((M_rows, Ctot), dtype=np.float32)
        B = np.empty((Ctot, M_cols), dtype=np.float32)
        self._check(self._lib.cnmf_range_finder(self._ctx, int(bool(transpose)), len(Q0_blocks),
                                                widths.ctypes.data_as(C.POINTER(C.c_int32)), _fp(Q0), int(n_iter),
                                                _fp(Q), _fp(B)))
        offs = np.concatenate([[0], np.cumsum(widths)])
        return ([Q[:, offs[i]:offs[i + 1]] for i in range(len(widths))],
                [B[offs[i]:offs[i + 1]] for i in range(len(widths))])

    def nndsvd_init(self, n_components, random_state=None, eps=1e-6, tail="host", variant="nndsvd"):
        """sklearn's ``init='nndsvd'`` for ONE restart (decomposition/_nmf.py:316-354); see :meth:`nndsvd_init_batch`.
        Returns (W0, H0) in float64 (cast to X's dtype by the caller, like sklearn)."""
        return self.nndsvd_init_batch([n_components], [random_state], eps=eps, tail=tail, variant=variant)[0]

    # The tail of the last nndsvd_init_batch(tail="device"): "device", or "host_fallback" when a block was refused (rank
    # below k, sweep cap, a non-finite value) and the whole call took the host route.
    last_nndsvd_tail = None

    @staticmethod
    def _nndsvd_groups(ks, n_rand, n_iters, max_cols):
        """Groups of restarts whose blocks fit one pass AND that make the same number of power iterations."""
        order = sorted(range(len(ks)), key=lambda r: (n_iters[r], ks[r]))
        groups, cur, cols = [], [], 0
        for r in order:
            if cur and (cols + n_rand[r] > max_cols or n_iters[r] != n_iters[cur[0]]):
                groups.append(cur); cur, cols = [], 0
            cur.append(r); cols += n_rand[r]
        if cur:
            groups.append(cur)
        return groups

    def init_store_reset(self):
        """Empty the context's init store (the start factors ``nndsvd_init_batch(tail="device", keep=True)`` left)."""
        self._check(self._lib.cnmf_init_store_reset(self._ctx))
        self._init_store_ks = []
        self.last_init_store_order = None

    def init_store_fetch(self):
        """The init store on the host: the list of (W0 [N, k], H0 [k, G]) in float32, in the order of the batch call
        that starts from it (``init_store=True``)."""
        N, G = self.shape
        ks = list(getattr(self, "_init_store_ks", []))
        tot = max(int(sum(ks)), 1)
        W = np.empty(tot * N, dtype=np.float32)
        H = np.empty((tot, G), dtype=np.float32)
        n = C.c_int32(0)
        self._check(self._lib.cnmf_init_store_fetch(self._ctx, _fp(W), _fp(H), tot, C.byref(n)))
        if n.value != len(ks):
            raise RuntimeError("the init store holds %d restarts, %d were expected" % (n.value, len(ks)))
        offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
        return [(W[offs[r] * N:offs[r + 1] * N].reshape(N, ks[r]), H[offs[r]:offs[r + 1]]) for r in range(len(ks))]

    def _nndsvd_device_tail(self, ks, seeds, groups, n_iters, transpose, variant, eps):
        """One ``cnmf_nndsvd_group`` call per group into the (emptied) init store.  The store fills group after group:
        returns (status per restart, the restart index of every store entry)."""
        i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        self.init_store_reset()
        status = np.zeros(len(ks), dtype=np.int32)
        order = []
        for grp in groups:
            kk = np.ascontiguousarray([ks[r] for r in grp], dtype=np.int32)
            sd = np.ascontiguousarray(np.asarray([seeds[r] for r in grp], dtype=np.int64).astype(np.uint32))
            st = np.zeros(len(grp), dtype=np.int32)
            self._check(self._lib.cnmf_nndsvd_group(self._ctx, int(bool(transpose)), len(grp), kk.ctypes.data_as(i32p),
                                                    sd.ctypes.data_as(u32p), int(n_iters[grp[0]]),
                                                    NNDSVD_VARIANTS.index(variant), float(eps), float(self.x_mean),
                                                    st.ctypes.data_as(i32p)))
            status[grp] = st
            order.extend(grp)
        self._init_store_ks = [ks[r] for r in order]
        return status, order

    def nndsvd_init_batch(self, ks, random_states, eps=1e-6, max_cols=256, threads=None, device_range_finder=True,
                          tail="host", variant="nndsvd", keep=False):
        """sklearn's ``init='nndsvd'`` (decomposition/_nmf.py:316-354) for MANY restarts: ``_randomized_svd``
        (utils/extmath.py:531-602: n_oversamples=10, n_iter 7|4, LU-normalised power iterations, final QR, small
        SVD, svd_flip), then the positive/negative split.

        The range finders of a whole GROUP of restarts ride in one pass over X: their (k + 10)-column blocks sit side by
        side (up to ``max_cols`` = 256 columns: 13 restarts of rank 9), so the 2 * n_iter + 2 passes over X are paid
        once per group, not once per restart, and (``device_range_finder=True``, the default; needs k + 10 <= 128) the
        normalisation between two passes stays on the device too (``cnmf_range_finder``: Cholesky-QR instead of
        scikit-learn's pivoted LU -- any normaliser leaves the iterated subspace unchanged).  What remains on the host
        per restart is the (k + 10) x G SVD, the sign flip and the positive / negative split.
        ``device_range_finder=False``: every product on the device, LU / QR on a host thread pool (the round-2 scheme,
        batched).  Returns a list of (W0, H0) in float64.

        ``variant``: ``'nndsvd'``, ``'nndsvda'`` or ``'nndsvdar'`` -- what becomes of the zeros (:func:`_nndsvd_fill`).

        ``tail="device"`` (integer seeds, k + 10 <= 128, all three variants): ONE library call per group
        (``cnmf_nndsvd_group``: the start blocks drawn on the device, the range finder, a float64 one-sided Jacobi SVD of
        every block, flip, split and threshold); the factors come back as float64 arrays holding the float32 values the
        device rounded to.  ``keep=True`` leaves them in the context's init store instead, in the order
        ``last_init_store_order`` (restart indices; the groups are sorted by (n_iter, k)), and returns ``None``:
        ``nmf_batch(ks_in_that_order, init_store=True)`` then starts from the store without a transfer.  When the device
        refuses a block (status != 0: rank below k, sweep cap, non-finite value) the store is discarded, the WHOLE call
        takes the host route with one warning, the list is returned whatever ``keep`` says, and ``last_nndsvd_tail`` is
        ``"host_fallback"`` instead of ``"device"``."""
        from concurrent.futures import ThreadPoolExecutor
        from scipy import linalg
        import os
        N, G = self.shape
        ks = [int(k) for k in ks]
        if len(ks) != len(random_states):
            raise ValueError("need one random_state per restart")
        for k in ks:
            if k > min(N, G):
                raise ValueError("init = 'nndsvd' can only be used when n_components <= min(n_samples, n_features)")
        transpose = N < G                                     # M = X.T when n_samples < n_features
        M_rows, M_cols = (G, N) if transpose else (N, G)
        n_rand = [k + 10 for k in ks]
        n_iters = [7 if k < 0.1 * min(N, G) else 4 for k in ks]
        if max(n_rand) > max_cols:
            raise NotImplementedError("n_components + 10 = %d columns exceed one device pass (%d)" % (max(n_rand), max_cols))
        if variant not in NNDSVD_VARIANTS:
            raise ValueError("Invalid init parameter: got %r instead of one of %r" % (variant, NNDSVD_VARIANTS))
        if tail not in ("host", "device"):
            raise ValueError("tail must be 'host' or 'device'")
        groups = self._nndsvd_groups(ks, n_rand, n_iters, max_cols)
        if tail == "device":
            if any(not isinstance(rs, (int, np.integer)) for rs in random_states):
                raise TypeError("tail='device' draws the start blocks on the device: integer seeds only")
            if max(n_rand) > _lib.CNMF_KMAX or max_cols != 256:
                raise NotImplementedError("tail='device' needs n_components + 10 <= %d and max_cols = 256" % _lib.CNMF_KMAX)
            status, order = self._nndsvd_device_tail(ks, random_states, groups, n_iters, transpose, variant, eps)
            if not status.any():
                self.last_nndsvd_tail = "device"
                self.last_init_store_order = order
                if keep:
                    return None
                got = self.init_store_fetch()
                self.init_store_reset()
                results = [None] * len(ks)
                for r, (W, H) in zip(order, got):
                    results[r] = (W.astype(np.float64), H.astype(np.float64))
                return results
            self.init_store_reset()
            self.last_nndsvd_tail = "host_fallback"
            self.last_init_store_order = None
            warnings.warn("NNDSVD: the device tail refused %d of %d restarts (status %s); the whole call takes the host "
                          "route" % (int((status != 0).sum()), len(ks), sorted(set(int(v) for v in status[status != 0]))),
                          RuntimeWarning)
        if threads is None:                                  # CPUs this process may really use (affinity, cgroup quota)
            try:
                threads = len(os.sched_getaffinity(0))
            except AttributeError:
                threads = os.cpu_count() or 1
            try:
                quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
                if quota != "max":
                    threads = max(1, min(threads, int(float(quota) / float(period))))
            except Exception:
                pass
        pool = ThreadPoolExecutor(max(1, min(threads, 64)))
        # one LAPACK thread per factorization: the parallelism is ACROSS the restarts of a group (a BLAS that spawns its
        # own 64 threads inside each of 16 pool threads runs slower than one thread would)
        try:
            from threadpoolctl import threadpool_limits
            blas_limit = threadpool_limits(1)
        except Exception:
            blas_limit = None

        def passes(Qs, trans):
            """[M_r @ Q_r] (trans=False) or [M_r.T @ Q_r] for the blocks of one group: ONE device product."""
            out = self.x_matmul(np.concatenate(Qs, axis=1), trans=trans).astype(np.float64)
            offs = np.cumsum([0] + [q.shape[1] for q in Qs])
            return [out[:, offs[i]:offs[i + 1]] for i in range(len(Qs))]

        def lu_pl(A):
            return linalg.lu(A, permute_l=True, check_finite=False)[0]

        def finish(args):
            k, Q, B = args
            return _nndsvd_finish(k, Q, B, transpose, eps)

        results = [None] * len(ks)
        on_device = device_range_finder and max(n_rand) <= _lib.CNMF_KMAX
        pending = []

        def collect(item):
            for r, fut in zip(*item):
                results[r] = fut.result()

        try:
            for grp in groups:
                Qs = []
                for r in grp:
                    rs = random_states[r]
                    rng = rs if isinstance(rs, np.random.RandomState) else np.random.RandomState(rs)
                    Qs.append(rng.normal(size=(M_cols, n_rand[r])))
                if on_device:
                    Qd, Bd = self.range_finder(Qs, n_iters[grp[0]], transpose)
                    # the host tails of this group run on the pool WHILE the device finds the ranges of the next group
                    # (the ctypes call releases the GIL); at most two groups are in flight
                    pending.append((grp, [pool.submit(finish, (ks[r], Q, B)) for r, Q, B in zip(grp, Qd, Bd)]))
                    if len(pending) > 2:
                        collect(pending.pop(0))
                    continue
                for _ in range(n_iters[grp[0]]):
                    Qs = list(pool.map(lu_pl, passes(Qs, trans=transpose)))            # Q = PL of M @ Q
                    Qs = list(pool.map(lu_pl, passes(Qs, trans=not transpose)))        # Q = PL of M.T @ Q
                Qs = list(pool.map(lambda A: linalg.qr(A, mode="economic", check_finite=False)[0], passes(Qs, trans=transpose)))
                Bs = [b.T for b in passes(Qs, trans=not transpose)]                    # Q.T @ M
                for r, wh in zip(grp, pool.map(finish, [(ks[r], Q, B) for r, Q, B in zip(grp, Qs, Bs)])):
                    results[r] = wh
            while pending:
                collect(pending.pop(0))
        finally:
            pool.shutdown(wait=True)
            if blas_limit is not None:
                blas_limit.restore_original_limits()
        if variant != "nndsvd":
            for r, (W, H) in enumerate(results):
                _nndsvd_fill(W, H, variant, self.x_mean, random_states[r])
        return results

    # ------------------------------------------------------------------ consensus core
    def consensus(self, spectra, k, density_threshold=0.5, local_neighborhood_size=0.30,
                  skip_density=False, want_silhouette=False, random_state=1, n_init=10,
                  max_iter=300, tol=1e-4, return_dist=False, store_rows=None):
        """Numerical core of ``cNMF.consensus`` (cnmf.py:871-916) on the device, float64.

        ``spectra``: the merged per-restart spectra (R x G) -- or ``None`` with ``store_rows`` (R row indices into the
        context's resident spectra store, see ``nmf_batch(resident="keep")``): the merged spectra are then gathered on
        the device, nothing is uploaded.  Returns a dict with
        ``local_density`` (R,), ``density_filter`` (R,) bool, ``labels`` (R,) int (0-based,
        -1 = filtered), ``median_spectra`` (k x G, rows sum to 1), ``inertia``,
        ``silhouette`` (if requested), ``topics_dist`` (R x R, if requested)."""
        self._sync_env()
        if store_rows is not None:
            rows = np.ascontiguousarray(store_rows, dtype=np.int64).ravel()
            R, G = int(rows.size), self.spectra_genes
        else:
            S = np.ascontiguousarray(spectra, dtype=np.float64)
            if S.ndim != 2:
                raise ValueError("spectra must be 2-D")
            R, G = S.shape
        k = int(k)
        n_neighbors = int(local_neighborhood_size * R / k)                 # cnmf.py:879
        L = 2 + int(np.log(k))
        # the draws KMeans(random_state=1) takes: data-independent count, so the whole
        # stream is generated up front with numpy's legacy RNG (bit-identical to sklearn)
        u = np.random.RandomState(random_state).random_sample(n_init * (1 + (k - 1) * L))
        prm = _lib.ConsensusParams(k, n_neighbors, float(density_threshold), int(bool(skip_density)),
                                   int(bool(want_silhouette)), int(n_init), int(max_iter), float(tol))
        dens = np.zeros(R, dtype=np.float64)
        keep = np.zeros(R, dtype=np.int32)
        labels = np.zeros(R, dtype=np.int32)
        med = np.zeros((k, G), dtype=np.float64)
        dist = np.zeros((R, R), dtype=np.float64) if return_dist else None
        stats = np.zeros(4, dtype=np.float64)
        dblp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        tail_args = (R, G, C.byref(prm), u.ctypes.data_as(dblp), dens.ctypes.data_as(dblp),
                     keep.ctypes.data_as(i32p), labels.ctypes.data_as(i32p), med.ctypes.data_as(dblp),
                     dist.ctypes.data_as(dblp) if return_dist else None, stats.ctypes.data_as(dblp))
        if store_rows is not None:
            rc = self._lib.cnmf_consensus_store(self._ctx, rows.ctypes.data_as(C.POINTER(C.c_int64)), *tail_args)
        else:
            rc = self._lib.cnmf_consensus(self._ctx, S.ctypes.data_as(dblp), *tail_args)
        if rc == -4 and b"Zero components remain" in self._lib.cnmf_last_error(self._ctx):
            raise RuntimeError("Zero components remain after density filtering. Consider increasing density threshold")
        self._check(rc)
        out = dict(local_density=dens, density_filter=keep.astype(bool), labels=labels,
                   median_spectra=med, inertia=float(stats[1]), n_kept=int(stats[0]),
                   kmeans_n_iter=int(stats[3]), n_neighbors=n_neighbors)
        if want_silhouette:
            out["silhouette"] = float(stats[2])
        if return_dist:
            out["topics_dist"] = dist
        return out

    def pairwise_distances(self, rows, labels=None, return_dist=True):
        """``cnmf_pairwise_distances``: ``sklearn.metrics.euclidean_distances(rows)`` (cnmf.py:891, 988) and / or
        ``silhouette_score(rows, labels, metric='euclidean')`` (cnmf.py:923) on the device in float64, rows as given.
        Returns ``(D or None, silhouette or None)``."""
        self._sync_env()
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2:
            raise ValueError("rows must be 2-D")
        R, G = rows.shape
        dblp = C.POINTER(C.c_double)
        D = np.empty((R, R), dtype=np.float64) if return_dist else None
        sil, lp, k = None, None, 0
        if labels is not None:
            lab = np.asarray(labels)
            if lab.shape != (R,):
                raise ValueError("labels must have one entry per row")
            uniq, inv = np.unique(lab, return_inverse=True)          # LabelEncoder, sklearn metrics/cluster/_unsupervised.py
            k = len(uniq)
            if not 1 < k < R:
                raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % k)
            inv = np.ascontiguousarray(inv, dtype=np.int32)
            lp = inv.ctypes.data_as(C.POINTER(C.c_int32))
            sil = C.c_double(0.0)
        self._check(self._lib.cnmf_pairwise_distances(self._ctx, rows.ctypes.data_as(dblp), R, G, lp, k,
                                                      D.ctypes.data_as(dblp) if return_dist else None,
                                                      C.byref(sil) if sil is not None else None))
        return D, (float(sil.value) if sil is not None else None)

    def clustergram(self, spectra, labels, k, store_rows=None, return_image=True, return_linkage=False):
        """``cnmf_clustergram``: what ``consensus(show_clustering=True)`` orders before it draws (cnmf.py:986-1009, :1028),
        on the device in float64.  ``spectra`` (R x G, as merged: they are L2-normalised on the device) or ``None`` with
        ``store_rows`` (R rows of the resident spectra store); ``labels`` (R,) with -1 = removed by the density filter,
        else the 0-based k-means cluster.  Returns a dict with

        ``spectra_order``        indices into the KEPT rows: the clusters in ascending label, each in the leaf order of the
                                 average-linkage dendrogram of its own distance block (``tests/_upgma_ref.py`` is the
                                 definition; with distinct merge heights it is scipy's ``leaves_list(linkage(., 'average'))``)
        ``segments``             (k + 1,): cluster c is ``spectra_order[segments[c]:segments[c + 1]]``
        ``topics_dist_ordered``  distances of the kept rows, ``D[order][:, order]`` (``None`` without ``return_image``)
        ``linkage``              the k linkage matrices (``None`` without ``return_linkage``)

        A cluster above ``CNMF_LINKAGE_MAX`` members raises NotImplementedError; a label outside -1..k-1 or a cluster
        without a member raises ValueError."""
        self._sync_env()
        k = int(k)
        lab = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        R = int(lab.size)
        dblp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        if store_rows is not None:
            rows = np.ascontiguousarray(store_rows, dtype=np.int64).ravel()
            if rows.size != R:
                raise ValueError("labels must have one entry per store row")
            G, sp, rp = int(self.spectra_genes), None, rows.ctypes.data_as(C.POINTER(C.c_int64))
        else:
            S = np.ascontiguousarray(spectra, dtype=np.float64)
            if S.ndim != 2 or S.shape[0] != R:
                raise ValueError("spectra must be 2-D with one label per row")
            G, sp, rp = int(S.shape[1]), S.ctypes.data_as(dblp), None
        Rk = int((lab >= 0).sum())
        order = np.zeros(Rk, dtype=np.int32)
        seg = np.zeros(max(k, 0) + 1, dtype=np.int32)
        Z = np.zeros((max(Rk - k, 0), 4), dtype=np.float64) if return_linkage else None
        image = np.empty((Rk, Rk), dtype=np.float64) if return_image else None
        self._check(self._lib.cnmf_clustergram(self._ctx, sp, rp, R, G, lab.ctypes.data_as(i32p), k,
                                               order.ctypes.data_as(i32p),
                                               Z.ctypes.data_as(dblp) if Z is not None else None,
                                               seg.ctypes.data_as(i32p),
                                               image.ctypes.data_as(dblp) if image is not None else None))
        linkage = None
        if return_linkage:
            linkage = [Z[seg[c] - c:seg[c + 1] - c - 1].copy() for c in range(k)]
        return dict(spectra_order=order.astype(np.int64), segments=seg, topics_dist_ordered=image, linkage=linkage)

    def clustergram_step_ms(self):
        """Device milliseconds of the last :meth:`clustergram` by step (HIP events)."""
        out = np.zeros(5, dtype=np.float64)
        self._check(self._lib.cnmf_clustergram_step_ms(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return dict(zip(("distances", "cluster_blocks", "linkage_and_order", "ordered_image", "download"), out.tolist()))

    def prediction_error(self, W, H):
        """``((X - W @ H)**2).sum()`` over the resident matrix (cnmf.py:926-930)."""
        if self.shape is None:
            raise RuntimeError("set_matrix() has not been called")
        N, G = self.shape
        W = np.ascontiguousarray(W, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64)
        if W.shape[0] != N or H.shape[1] != G or W.shape[1] != H.shape[0]:
            raise ValueError("shape mismatch: W %s, H %s, X %s" % (W.shape, H.shape, (N, G)))
        err = C.c_double(0.0)
        dblp = C.POINTER(C.c_double)
        self._check(self._lib.cnmf_prediction_error(self._ctx, int(H.shape[0]), W.ctypes.data_as(dblp),
                                                    H.ctypes.data_as(dblp), C.byref(err)))
        return float(err.value)

    # ------------------------------------------------------------------ diagnostics
    # ------------------------------------------------------------------ multi-GPU exchange (RCCL)
    def comm_unique_id(self):
        """128-byte RCCL id (rank 0 creates it; ship it to the other ranks out of band)."""
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        self._check(self._lib.cnmf_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        """Collective: every rank calls it with the same id (ncclCommInitRank)."""
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % _lib.COMM_ID_BYTES)
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.cnmf_comm_init(self._ctx, buf, int(rank), int(world)))

    def comm_finalize(self):
        self._check(self._lib.cnmf_comm_finalize(self._ctx))

    @property
    def comm_rank(self):
        return int(self._lib.cnmf_comm_rank(self._ctx))

    @property
    def comm_world(self):
        return int(self._lib.cnmf_comm_world(self._ctx))

    def allgather_array(self, a):
        """All-gather equally-shaped host arrays: returns ``[world, *a.shape]``."""
        a = np.ascontiguousarray(a)
        out = np.empty((self.comm_world,) + a.shape, dtype=a.dtype)
        self._check(self._lib.cnmf_allgather_bytes(self._ctx, a.ctypes.data_as(C.c_void_p), a.nbytes,
                                                   out.ctypes.data_as(C.c_void_p)))
        return out

    def allgather_spectra(self, local, rows_max, n_genes=None):
        """THE data-path collective: one all-gather of this rank's packed float32 spectra
        (``local`` [rows, G], or ``None`` for the context's resident store) zero-padded to
        ``rows_max`` rows.  Returns ``[world, rows_max, G]`` float32."""
        if local is None:
            rows, G = self.spectra_rows, (self.spectra_genes or self.shape[1])
            lp = None
        else:
            local = np.ascontiguousarray(local, dtype=np.float32)
            rows, G = (int(local.shape[0]), int(local.shape[1] if local.ndim == 2 else n_genes))
            lp = _fp(local) if rows else None
            if not rows:
                lp = _fp(np.zeros(1, np.float32))
        if n_genes is not None and int(n_genes) != G:
            raise ValueError("n_genes does not match the block")
        out = np.empty((self.comm_world, int(rows_max), G), dtype=np.float32)
        if rows_max:
            self._check(self._lib.cnmf_allgather_spectra(self._ctx, lp, rows, int(rows_max), G, _fp(out)))
        return out

    @property
    def spectra_rows(self):
        """Rows in the resident spectra store (``nmf_batch(..., resident=True)`` appends to it)."""
        return int(self._lib.cnmf_spectra_rows(self._ctx))

    def spectra_reset(self):
        self._check(self._lib.cnmf_spectra_reset(self._ctx))
        self.store_gen += 1                      # row indices handed out before this point are void

    @property
    def spectra_genes(self):
        return int(self._lib.cnmf_spectra_genes(self._ctx))

    def spectra_append(self, rows):
        """Upload ``rows`` (n x G, float32) behind the store's content; returns the index of the first new row."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2:
            raise ValueError("rows must be 2-D")
        first = self.spectra_rows
        self._check(self._lib.cnmf_spectra_append(self._ctx, _fp(rows), rows.shape[0], rows.shape[1]))
        return first

    def spectra_fetch(self, row0=0, rows=None):
        """Rows ``[row0, row0 + rows)`` of the resident spectra store on the host (default: all of it)."""
        total = self.spectra_rows
        rows = total - int(row0) if rows is None else int(rows)
        out = np.empty((rows, self.spectra_genes if total else 0), dtype=np.float32)
        if out.size:
            self._check(self._lib.cnmf_spectra_fetch_rows(self._ctx, int(row0), rows, _fp(out)))
        return out

    def debug_gemm(self, mode, A, B, variant=0, nsplit=1, reps=0):
        A = np.ascontiguousarray(A, dtype=np.float32)
        B = np.ascontiguousarray(B, dtype=np.float32)
        KC, K = A.shape
        J = B.shape[0] if mode == 0 else B.shape[1]
        Cout = np.empty((KC, J), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(self._lib.cnmf_debug_gemm(self._ctx, mode, variant, _fp(A), _fp(B), _fp(Cout),
                                              KC, K, J, nsplit, C.byref(ms), reps))
        return Cout, ms.value

    def debug_gemm3(self, A, B, nsplit=1, reps=0):
        """A [KC, K] . B [J, K]^T through the split-operand bf16 MFMA path; returns (C, ms)."""
        A = np.ascontiguousarray(A, dtype=np.float32)
        B = np.ascontiguousarray(B, dtype=np.float32)
        KC, K = A.shape
        J = B.shape[0]
        Cout = np.empty((KC, J), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(self._lib.cnmf_debug_gemm3(self._ctx, _fp(A), _fp(B), _fp(Cout), KC, K, J, int(nsplit),
                                               C.byref(ms), int(reps)))
        return Cout, ms.value

    def debug_gemm3c(self, A, Bn, nsplit=1, reps=0):
        """A [KC, K] . Bn [J, K]^T through the count-path kernel (Bn: integers <= 256); returns (C, ms)."""
        A = np.ascontiguousarray(A, dtype=np.float32)
        Bn = np.ascontiguousarray(Bn, dtype=np.float32)
        KC, K = A.shape
        J = Bn.shape[0]
        Cout = np.empty((KC, J), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(self._lib.cnmf_debug_gemm3c(self._ctx, _fp(A), _fp(Bn), _fp(Cout), KC, K, J, int(nsplit),
                                                C.byref(ms), int(reps)))
        return Cout, ms.value

    def debug_gemm2h(self, A, Bn, nsplit=1, nsub=2, reps=0, sweep_bound=False, count_bytes=False):
        """A [KC, K] . Bn [J, K]^T through the f16 two-plane count kernel (A >= 0, Bn: integers <= 65535);
        returns (C, ms).  ``sweep_bound=True`` scales the rows of A by the bound the W half-step reports
        (sqrt(sum w^2) per 1024-entry block) instead of the exact row maximum -- the production pass-B scaling.
        ``count_bytes=True`` holds Bn as one byte per count (integers <= 255, nsub 2, streams 0 and 4; else ValueError)."""
        nsub = int(nsub) | (128 if sweep_bound else 0) | (256 if count_bytes else 0)
        A = np.ascontiguousarray(A, dtype=np.float32)
        Bn = np.ascontiguousarray(Bn, dtype=np.float32)
        KC, K = A.shape
        J = Bn.shape[0]
        Cout = np.empty((KC, J), dtype=np.float32)
        ms = C.c_double(0.0)
        self._check(self._lib.cnmf_debug_gemm2h(self._ctx, _fp(A), _fp(Bn), _fp(Cout), KC, K, J, int(nsplit),
                                                int(nsub), C.byref(ms), int(reps)))
        return Cout, ms.value

    def debug_mt_normals(self, state, n):
        """n draws of numpy's legacy standard_normal continuing the RandomState ``state``: (draws, final state)."""
        st = _lib.MtState.from_numpy(state)
        out = np.empty(max(n, 1), dtype=np.float64)
        self._check(self._lib.cnmf_debug_mt_normals(self._ctx, C.byref(st), n, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:n], st.to_numpy()

    def debug_standard_normal(self, seed, n):
        out = np.empty(max(n, 1), dtype=np.float64)
        self._check(self._lib.cnmf_debug_standard_normal(self._ctx, C.c_uint32(seed), n,
                                                         out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:n]
