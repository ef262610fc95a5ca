"""Host side of the filter tests (test_host_filter.py, test_gpu_filter.py, test_gpu_filter_edges.py): a numpy / scipy
restatement of the four device entry points of csrc/filter_host.hip.h over a CSR taken exactly as it is stored, the
inputs of tools/make_golden_filter.py, and a device-free engine that plays ``cnmf_amd.engine.Engine``'s preprocess
methods with those restatements, so that the public ``Preprocess.filter_adata`` / ``preprocess_for_cnmf`` run on the CPU.

On integer counts every sum is exact in any order, the row scale ``target / row sum`` and the product ``x * scale`` are
one rounding each: restatement and device agree bit for bit there."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

SCAN_BLOCK = 1024            # items one scan workgroup covers: FLT_SCAN_BLOCK = 256 threads x FLT_SCAN_ITEMS = 4

# tools/make_golden_filter.py's input: (n_cells, n_genes, k_true, mu_lib, sigma_lib, seed), ADT features and their seed
PARAMS = (300, 400, 5, 5.0, 0.4, 23)
N_ADT, ADT_SEED, N_HVG, HVG_SEED = 12, 5, 80, 9
ADT_NAME = "Antibody Capture"
TARGET = 1e4
EXCLUDE = ["g7", "g8", "IGHV1.2", "not_a_gene"]
# filter_adata argument sets: the defaults scaled to the data, the mito threshold with filter_mito_genes, nothing
FILTER_RUNS = {
    "default": dict(min_cells_per_gene=10, min_counts_per_cell=120),
    # (no count threshold: cell 3, without counts, reaches the mito step with pct_mito = NaN and goes there)
    "mito": dict(min_cells_per_gene=10, min_counts_per_cell=None, filter_mito_thresh=0.02, filter_mito_genes=True),
    "none": dict(min_cells_per_gene=None, min_counts_per_cell=None, filter_mito_genes=False, filter_dot_genes=False),
}


def make_inputs():
    """(RNA counts float64 [N][G], cells, gene names, ADT counts [N][N_ADT], ADT names, HVG mask over the RNA genes).
    Gene names: 'MT-' at the start of five, inside one ('XMT-ND1'), '.' in six, one name twice; cell 3 has no counts."""
    from cnmf_amd import synth
    n, g, k, mu, sg, seed = PARAMS
    C, _ = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    C = C.astype(np.float64)
    C[3] = 0.0
    genes = ["g%d" % j for j in range(g)]
    for j, name in zip(range(20, 25), ["MT-CO1", "MT-CO2", "MT-ND1", "MT-ND2", "MT-ATP6"]):
        genes[j] = name
    genes[30] = "XMT-ND1"
    for j in range(40, 45):
        genes[j] = "AC%d.1" % j
    genes[45] = "IGHV1.2"
    genes[51] = "g50"                                   # a duplicated name
    genes[52] = "g50-1"                                 # ... whose first replacement exists already
    genes[53] = "g50"
    cells = ["c%d" % i for i in range(n)]
    rs = np.random.RandomState(ADT_SEED)
    A = rs.poisson(rs.gamma(2.0, 20.0, size=N_ADT), size=(n, N_ADT)).astype(np.float64)
    A[5] = 0.0
    adt_names = ["ADT_%d" % j for j in range(N_ADT)]
    ok = np.flatnonzero((C > 0).sum(axis=0) >= 2)
    hv = np.zeros(g, dtype=bool)
    hv[np.random.RandomState(HVG_SEED).choice(ok, N_HVG, replace=False)] = True
    hv[[7, 45]] = True                                  # two excluded genes among the HVGs
    return C, cells, genes, A, adt_names, hv


# ---------------------------------------------------------------- the four entry points, on a CSR as stored
def _rows(X):
    return np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))


def gene_detect(X, cell_mask=None):
    """(n_cells int64 [G], totals [G]): stored entries > 0 and the sum of the entries, over the masked cells"""
    G = X.shape[1]
    use = np.ones(X.nnz, dtype=bool) if cell_mask is None else np.asarray(cell_mask, dtype=bool)[_rows(X)]
    n_cells = np.bincount(X.indices[use & (X.data > 0)], minlength=G).astype(np.int64)
    totals = np.bincount(X.indices[use], weights=X.data[use], minlength=G)
    return n_cells, totals


def cell_sums(X, gene_mask=None):
    w = X.data if gene_mask is None else np.where(np.asarray(gene_mask, dtype=bool)[X.indices], X.data, 0.0)
    return np.bincount(_rows(X), weights=w, minlength=X.shape[0])


def subset(X, keep_cells=None, keep_genes=None):
    """the restriction, entries in their stored order, stored zeros kept, indices not sorted"""
    N, G = X.shape
    kc = np.ones(N, dtype=bool) if keep_cells is None else np.asarray(keep_cells, dtype=bool)
    kg = np.ones(G, dtype=bool) if keep_genes is None else np.asarray(keep_genes, dtype=bool)
    rows = _rows(X)
    keep = kc[rows] & kg[X.indices]
    colmap = np.cumsum(kg) - 1
    cnt = np.bincount(rows[keep], minlength=N)[kc]
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(X.indptr.dtype)
    return sp.csr_matrix((X.data[keep], colmap[X.indices[keep]].astype(X.indices.dtype), indptr),
                         shape=(int(kc.sum()), int(kg.sum())))


def fetch_counts(X, target_sum=0.0):
    data = X.data.astype(np.float64)
    if target_sum > 0:
        rs = cell_sums(X)
        scale = np.where(rs > 0, target_sum / np.where(rs > 0, rs, 1.0), 0.0)
        data = data * scale[_rows(X)]
    return sp.csr_matrix((data, X.indices.copy(), X.indptr.copy()), shape=X.shape)


def same_csr(A, B):
    """structure and value bits"""
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(np.asarray(A.data, dtype=np.float64).view(np.uint64),
                               np.asarray(B.data, dtype=np.float64).view(np.uint64)))


# ---------------------------------------------------------------- a device-free engine for the public methods
class FakeFilterEngine:
    """``Engine``'s preprocess methods in numpy: the filter entry points above, and select / ceiling as
    tools/make_golden_filter.py's scanpy stand-in computes them (the std in numpy's order over the dense matrix)."""

    def __init__(self):
        self._pre, self.X, self.slots = None, None, {}
        self.calls = []

    def _stage(self, X):
        self.X = X
        self._pre = {"N": X.shape[0], "G": X.shape[1], 0: None, 1: None}
        self.slots = {}
        return X

    def preprocess_upload(self, counts):
        self.calls.append("upload")
        X = sp.csr_matrix(counts, dtype=np.float64).copy()
        X.sum_duplicates()
        X.eliminate_zeros()
        return self._stage(X)

    def preprocess_upload_as_stored(self, counts):
        return self._stage(sp.csr_matrix(counts, dtype=np.float64))

    def preprocess_gene_detect(self, cell_mask=None):
        return gene_detect(self.X, cell_mask)

    def preprocess_cell_sums(self, gene_mask=None):
        return cell_sums(self.X, gene_mask)

    def preprocess_row_sums(self):
        return cell_sums(self.X)

    def preprocess_subset(self, keep_cells=None, keep_genes=None):
        self.calls.append("subset")
        for mask, what in ((keep_cells, "keep_cells keeps no cell"), (keep_genes, "keep_genes keeps no gene")):
            if mask is not None and not np.asarray(mask).any():
                raise ValueError(what)
        self._stage(subset(self.X, keep_cells, keep_genes))
        return self.X.shape[0], self.X.shape[1], self.X.nnz

    def preprocess_fetch_counts(self, target_sum=0.0):
        return fetch_counts(self.X, target_sum)

    def preprocess_select(self, slot, genes, target_sum=0.0, max_value=None):
        Y = fetch_counts(self.X, target_sum)[:, np.asarray(genes)].toarray()
        std = Y.std(axis=0, ddof=1)
        std[std == 0] = 1.0
        Y = Y / std
        if max_value is not None:
            Y[Y > max_value] = max_value
        self.slots[slot] = Y
        return std

    def preprocess_order_stats(self, slot, k):
        v = np.sort(self.slots[slot].reshape(-1))
        return v[k], v[min(k + 1, v.size - 1)]

    def preprocess_ceiling(self, slot, thresh):
        Y = self.slots[slot]
        Y[Y > thresh] = thresh

    def preprocess_densify(self, slot):
        self.slots[slot] = np.asarray(self.slots[slot])
        self.slots[(slot, "dense")] = True

    def preprocess_fetch(self, slot):
        Y = self.slots[slot]
        return Y.copy() if self.slots.get((slot, "dense")) else sp.csr_matrix(Y)

    def preprocess_release(self):
        self._pre, self.X, self.slots = None, None, {}

    def close(self):
        pass


def obs_frame(cells):
    return pd.DataFrame({"batch": ["b%d" % (i % 3) for i in range(len(cells))]}, index=cells)


# ---------------------------------------------------------------- the golden runs through the public interface
def gold_csr(gold, prefix, shape):
    return sp.csr_matrix((gold[prefix + "data"], gold[prefix + "indices"], gold[prefix + "indptr"]), shape=shape)


def _canonical(X):
    X = sp.csr_matrix(X, dtype=np.float64).copy()
    X.sort_indices()
    return X


def check_filter_run(P, gold, run, dense):
    """Preprocess.filter_adata for FILTER_RUNS[run] against the fixture: names, obs / var columns, CSR structure and
    value bits"""
    C, cells, genes, _, _, _ = make_inputs()
    data = pd.DataFrame(C, index=cells, columns=genes) if dense else (sp.csr_matrix(C), cells, genes)
    res = P.filter_adata(data, obs=obs_frame(cells), makeplots=False, **FILTER_RUNS[run])
    pre = "flt_%s_" % run
    assert list(res.obs_names) == list(gold[pre + "cells"]) and list(res.var_names) == list(gold[pre + "genes"])
    assert list(res.obs.index) == list(res.obs_names) and list(res.var.index) == list(res.var_names)
    assert "batch" in res.obs.columns
    assert np.array_equal(res.obs["n_counts"].values, gold[pre + "n_counts"])
    if pre + "pct_mito" in gold:
        assert np.array_equal(res.obs["pct_mito"].values.view(np.uint64), gold[pre + "pct_mito"].view(np.uint64))
    else:
        assert "pct_mito" not in res.obs.columns
    if pre + "n_cells" in gold:
        assert res.var["n_cells"].dtype == np.int64 and np.array_equal(res.var["n_cells"].values, gold[pre + "n_cells"])
    assert isinstance(res.X, np.ndarray) if dense else sp.issparse(res.X)
    assert same_csr(_canonical(res.X), gold_csr(gold, pre, res.X.shape))
    return res


def pf_inputs(run, dense):
    """(data, keyword arguments) of the preprocess_for_cnmf run ``run`` of the fixture"""
    C, cells, genes, A, adt_names, hv = make_inputs()
    wrap = (lambda M: np.array(M)) if dense else sp.csr_matrix
    kw = dict(obs=obs_frame(cells), highly_variable=hv, librarysize_targetsum=TARGET, makeplots=False)
    if run == "single":
        return (wrap(C), cells, genes), dict(kw, exclude_genes=EXCLUDE)
    if run == "ftype":
        ftype = np.array(["Gene Expression"] * len(genes) + [ADT_NAME] * len(adt_names))
        return (wrap(np.hstack([C, A])), cells, list(genes) + list(adt_names)), dict(kw, feature_type=ftype,
                                                                                     adt_feature_name=ADT_NAME)
    return [(wrap(C), cells, genes), (wrap(A), cells, adt_names)], kw


def check_pf_run(P, gold, run, dense, rna_rtol=0.0):
    """Preprocess.preprocess_for_cnmf against the fixture: the TP10K gene order, structure and bits, the HVG list and
    adata_RNA (bits when rna_rtol == 0, else its structure and the values to that relative error)"""
    data, kw = pf_inputs(run, dense)
    res, tp, hvgs = P.preprocess_for_cnmf(data, **kw)
    pre = "pf_%s_" % run
    rna_pre = "pf_ftype_rna_" if run == "list" else pre + "rna_"
    assert hvgs == list(gold[pre + "hvgs"]) and list(res.var_names) == hvgs
    assert list(tp.var_names) == list(gold[pre + "tp_genes"]) and list(tp.var.index) == list(tp.var_names)
    n, g = len(tp.obs_names), len(gold[pre + "tp_genes"])
    g_rna = g if run == "single" else g - N_ADT
    want = gold_csr(gold, "tp_rna_", (n, g_rna))
    if run != "single":
        want = sp.hstack((want, gold_csr(gold, "tp_adt_", (n, N_ADT))), format="csr")
        assert list(tp.var["feature_type"]) == ["Gene Expression"] * g_rna + [ADT_NAME] * N_ADT if run == "ftype" else True
    assert isinstance(tp.X, np.ndarray) if dense else sp.issparse(tp.X)
    assert same_csr(_canonical(tp.X), _canonical(want))
    ref = gold_csr(gold, rna_pre, (n, len(hvgs)))
    got = _canonical(res.X)
    got.eliminate_zeros()
    if rna_rtol == 0.0:
        assert same_csr(got, ref)
    else:
        assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
        assert np.abs(got.data - ref.data).max() <= rna_rtol * np.abs(ref.data).max()
    return res, tp, hvgs
