"""Generate tests/golden/ref_preprocess.npz by running the UNMODIFIED reference's ``preprocess.py`` (stdscale_quantile_celing,
Preprocess.harmony_correct_X, Preprocess.normalize_batchcorrect) on the CPU.

oracle/scanpy_shim.py is not enough here (normalize_total(copy=True) changes its input, AnnData cannot take a boolean
column mask, no obsm / pca / scale(max_value)), so this tool carries its own scanpy stand-in, float64 throughout:
  normalize_total   X * (target / row sum) (0 for a cell without counts); copy=True leaves the input alone
  scale             zero_center=False: every column divided by its ddof=1 std (a zero std left as 1), then
                    X[X > max_value] = max_value
  pca               zero_center=True, min(50, min(N, G) - 1) components: float64 SVD of the centred matrix, scores
                    (X - mean) V, sign rule: the loading of largest magnitude of every component is positive
and a harmonypy stand-in whose ``run_harmony`` is deterministic in its inputs: Phi_moe = an intercept row plus a one-hot
row per level of every harmony var, lamb = diag([0, 1, ...]), R = a softmax over K = 10 centroids (cells chosen by a
seed; the distances do not depend on the sign of a component), Z_corr = 0.5 * the PCA scores, in harmonypy's old
(cells as columns) or new (cells as rows) layout.

Input: seeded ``synth.topic_counts`` (PARAMS), 100 high-variance genes chosen by a seed, 3 batches; the GPU test
regenerates them.  Stored:
  scale_<i>_std / scale_<i>_thresh   stdscale_quantile_celing of the raw HVG counts for SCALE_RUNS[i], dense and CSR
                                     input (the tool asserts both equal min(x / std, thresh) -- or max_value -- bit for bit)
  plain_data / plain_std / plain_max normalize_batchcorrect without Harmony, normalize_librarysize=True: the CSR
                                     values (the structure is that of the raw HVG counts), the std, the ceiling (= the
                                     largest value)
  X_pca, R, Phi, hvgs                the Harmony runs' PCA scores, R [K][N], Phi_moe [B+1][N], the HVG order
  corr_X / corr_norm_X               normalize_batchcorrect with Harmony (raw counts corrected) / with
                                     normalize_librarysize=True (normalised counts corrected); harmony_correct_X over
                                     min(raw / corr_scale_std, corr_thresh) in the old and in the new layout gives corr_X
                                     to 1e-12 (asserted)
  corr_scale_std, corr_thresh        the scaling of the corrected raw matrix (the input of harmony_correct_X)

Run:  python tools/make_golden_preprocess.py      (seconds; needs the reference source tree scanpy_shim.REFERENCE_SRC names)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import pandas as pd
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import synth  # noqa: E402

# (n_cells, n_genes, k_true, mu_lib, sigma_lib, seed), HVG count and seed, batches, Harmony's K and seed
PARAMS = (300, 400, 5, 6.0, 0.4, 11)
N_HVG, HVG_SEED, N_BATCH, HARMONY_K, HARMONY_SEED = 100, 4, 3, 10, 7
SCALE_RUNS = [(None, .9999), (None, .99), (5.0, None)]
TARGET = 1e4


def make_inputs():
    """counts (float64 ndarray), cell names, gene names, HVG mask, obs with a 'batch' column"""
    n, g, k, mu, sg, seed = PARAMS
    C, _ = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    C = C.astype(np.float64)
    rs = np.random.RandomState(HVG_SEED)
    ok = np.flatnonzero((C > 0).sum(axis=0) >= 2)
    mask = np.zeros(g, dtype=bool)
    mask[rs.choice(ok, N_HVG, replace=False)] = True
    cells = ["c%d" % i for i in range(n)]
    genes = ["g%d" % j for j in range(g)]
    obs = pd.DataFrame({"batch": ["b%d" % (i % N_BATCH) for i in range(n)]}, index=cells)
    return C, cells, genes, mask, obs


# ---------------------------------------------------------------- scanpy stand-in
class AnnData:
    def __init__(self, X, obs=None, var=None):
        self.X = X
        self.obs = obs if obs is not None else pd.DataFrame(index=[str(i) for i in range(X.shape[0])])
        self.var = var if var is not None else pd.DataFrame(index=[str(i) for i in range(X.shape[1])])
        self.obsm = {}

    @property
    def shape(self):
        return self.X.shape

    def copy(self):
        a = AnnData(self.X.copy(), self.obs.copy(), self.var.copy())
        a.obsm = {k: v.copy() for k, v in self.obsm.items()}
        return a

    def __getitem__(self, key):
        rows, cols = key
        assert rows == slice(None)
        cols = np.asarray(cols)
        X = self.X[:, np.flatnonzero(cols)] if cols.dtype == bool else self.X[:, cols]
        return AnnData(X.copy(), self.obs.copy(), self.var.iloc[np.flatnonzero(cols) if cols.dtype == bool else cols].copy())


def normalize_total(adata, target_sum=None, copy=False):
    a = adata.copy() if copy else adata
    X = a.X
    rs = np.asarray(X.sum(axis=1)).ravel()
    f = np.where(rs > 0, target_sum / np.where(rs > 0, rs, 1.0), 0.0)
    if sp.issparse(X):
        X = sp.csr_matrix(X)
        X.data = X.data * np.repeat(f, np.diff(X.indptr))
    else:
        X = X * f[:, None]
    a.X = X
    return a if copy else None


def column_std(X):
    D = np.asarray(X.todense()) if sp.issparse(X) else np.asarray(X)
    std = D.std(axis=0, ddof=1)
    std[std == 0] = 1.0
    return std


def scale(adata, zero_center=True, max_value=None):
    assert not zero_center
    X = adata.X
    std = column_std(X)
    if sp.issparse(X):
        X = sp.csr_matrix(X)
        X.data = X.data / std[X.indices]
        if max_value is not None:
            X.data[X.data > max_value] = max_value
    else:
        X = X / std
        if max_value is not None:
            X[X > max_value] = max_value
    adata.X = X
    adata.uns_std = std


def pca(adata, use_highly_variable=True, zero_center=True):
    assert zero_center
    X = np.asarray(adata.X.todense()) if sp.issparse(adata.X) else np.asarray(adata.X)
    n = 50 if 50 < min(X.shape) else min(X.shape) - 1
    Xc = X - X.mean(axis=0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    V = Vt[:n].T
    lead = V[np.argmax(np.abs(V), axis=0), np.arange(n)]
    V = V * np.where(lead < 0, -1.0, 1.0)
    adata.obsm["X_pca"] = Xc @ V


def make_scanpy():
    mod = types.ModuleType("scanpy")
    mod.AnnData = AnnData
    mod.pp = types.SimpleNamespace(normalize_total=normalize_total, scale=scale, pca=pca)
    mod.pl = types.SimpleNamespace(pca_variance_ratio=lambda *a, **k: None)
    return mod


# ---------------------------------------------------------------- harmonypy stand-in
class HarmonyResult:
    pass


def harmony_factors(pcs, meta, vars_use):
    """Phi_moe [B+1][N], lamb, R [K][N] of the stand-in"""
    N = pcs.shape[0]
    rows = [np.ones(N)]
    for v in ([vars_use] if isinstance(vars_use, str) else vars_use):
        col = meta[v].values
        for lev in sorted(set(col)):
            rows.append((col == lev).astype(np.float64))
    Phi = np.array(rows)
    lamb = np.diag(np.r_[0.0, np.ones(Phi.shape[0] - 1)])
    rs = np.random.RandomState(HARMONY_SEED)
    cent = pcs[rs.choice(N, HARMONY_K, replace=False)]
    d = ((pcs[:, None, :] - cent[None, :, :]) ** 2).sum(axis=2)          # [N][K]
    d = d / np.median(d)
    e = np.exp(-(d - d.min(axis=1, keepdims=True)))
    R = (e / e.sum(axis=1, keepdims=True)).T
    return Phi, lamb, R


def make_harmonypy(new_layout):
    mod = types.ModuleType("harmonypy")

    def run_harmony(data_mat, meta_data, vars_use, max_iter_harmony=20, theta=1, **kw):
        pcs = np.asarray(data_mat, dtype=np.float64)
        Phi, lamb, R = harmony_factors(pcs, meta_data, vars_use)
        res = HarmonyResult()
        res.K, res.lamb = HARMONY_K, lamb
        if new_layout:
            res.Z_corr, res.R, res.Phi_moe = 0.5 * pcs, R.T.copy(), Phi.T.copy()
        else:
            res.Z_corr, res.R, res.Phi_moe = (0.5 * pcs).T.copy(), R, Phi
        return res

    mod.run_harmony = run_harmony
    return mod


def load_reference():
    from oracle.scanpy_shim import REFERENCE_SRC
    import matplotlib
    matplotlib.use("Agg")
    sys.modules["scanpy"] = make_scanpy()
    spec = importlib.util.spec_from_file_location("ref_preprocess", os.path.join(REFERENCE_SRC, "cnmf", "preprocess.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    C, cells, genes, mask, obs = make_inputs()
    raw = C[:, mask]
    store = {"params": np.array(PARAMS, dtype=np.float64), "n_hvg": np.array(N_HVG), "hvg_seed": np.array(HVG_SEED),
             "n_batch": np.array(N_BATCH), "hvgs": np.array([genes[j] for j in np.flatnonzero(mask)])}

    def adata_of(X):
        return AnnData(X, obs.copy(), pd.DataFrame({"highly_variable": mask}, index=genes))

    # stdscale_quantile_celing on dense and CSR input
    for i, (mv, q) in enumerate(SCALE_RUNS):
        outs = []
        for X in (raw.copy(), sp.csr_matrix(raw)):
            a = AnnData(X)
            ref.stdscale_quantile_celing(a, max_value=mv, quantile_thresh=q)
            outs.append(np.asarray(a.X.todense()) if sp.issparse(a.X) else a.X)
            std = a.uns_std
        assert np.abs(outs[0] - outs[1]).max() <= 1e-12 * np.abs(outs[0]).max()
        y = raw / std
        if mv is not None:
            y[y > mv] = mv
        thresh = np.quantile(y.reshape(-1), q) if q is not None else np.inf
        assert np.array_equal(np.minimum(y, thresh), outs[0]), i
        store["scale_%d_std" % i], store["scale_%d_thresh" % i] = std, np.array(thresh)

    P = ref.Preprocess(random_seed=0)
    # without Harmony, library-size normalised
    a, hv = P.normalize_batchcorrect(adata_of(sp.csr_matrix(C)), normalize_librarysize=True, harmony_vars=None,
                                     librarysize_targetsum=TARGET, makeplots=False)
    assert sp.issparse(a.X) and hv == list(store["hvgs"])
    Xp = sp.csr_matrix(a.X)
    Xp.sort_indices()
    ref_structure = sp.csr_matrix(raw)
    assert np.array_equal(Xp.indptr, ref_structure.indptr) and np.array_equal(Xp.indices, ref_structure.indices)
    store["plain_data"], store["plain_std"], store["plain_max"] = Xp.data, a.uns_std, np.array(Xp.data.max())

    # with Harmony: raw counts corrected, then normalised counts corrected
    for tag, norm in (("corr", False), ("corr_norm", True)):
        sys.modules["harmonypy"] = make_harmonypy(new_layout=False)
        a, hv = P.normalize_batchcorrect(adata_of(sp.csr_matrix(C)), normalize_librarysize=norm, harmony_vars=["batch"],
                                         makeplots=False)
        assert hv == list(store["hvgs"]) and isinstance(a.X, np.ndarray)
        if "X_pca" in store:
            assert np.array_equal(store["X_pca"], a.obsm["X_pca"])
        store["X_pca"] = a.obsm["X_pca"]
        assert np.array_equal(a.obsm["X_pca_harmony"], 0.5 * a.obsm["X_pca"])
        store[tag + "_X"] = a.X
    Phi, lamb, R = harmony_factors(store["X_pca"], obs, ["batch"])
    store["R"], store["Phi"] = R, Phi

    # harmony_correct_X on the raw scaled + ceilinged HVG counts, both layouts: the same bits as the pipeline
    std = column_std(raw)
    y = raw / std
    thresh = np.quantile(y.reshape(-1), .9999)
    y = np.minimum(y, thresh)
    store["corr_scale_std"], store["corr_thresh"] = std, np.array(thresh)
    outs = []
    for new in (False, True):
        sys.modules["harmonypy"] = make_harmonypy(new_layout=new)
        Xc, Zh = P.harmony_correct_X(np.asmatrix(y), obs, store["X_pca"], ["batch"])
        assert np.array_equal(Zh, 0.5 * store["X_pca"])
        outs.append(Xc)
    assert np.abs(outs[0] - outs[1]).max() <= 1e-12 * np.abs(outs[0]).max()
    # (the layouts differ in the last bits -- BLAS over transposed operands -- and this y and the pipeline's differ in the
    # last bit of a few scaled entries)
    assert np.abs(outs[0] - store["corr_X"]).max() <= 1e-12 * np.abs(store["corr_X"]).max()
    out = os.path.join(ROOT, "tests", "golden", "ref_preprocess.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
