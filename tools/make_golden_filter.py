"""Generate tests/golden/ref_filter.npz by running the UNMODIFIED reference's ``preprocess.py`` (Preprocess.filter_adata,
Preprocess.preprocess_for_cnmf) on the CPU.

The tool carries its own scanpy stand-in (oracle/scanpy_shim.py and tools/make_golden_preprocess.py's have no filters, no
row / name indexing and no make-unique), float64 throughout:
  AnnData              X (ndarray or CSR), obs, var; ``a[rows, cols]`` with a slice, a boolean mask (array or Series) or a
                       list / Index of names per axis, always a copy; obs_names / var_names; copy();
                       var_names_make_unique (anndata's make_index_unique)
  pp.filter_genes      var['n_cells'] = (X > 0).sum(0), keeps n_cells >= min_cells, in place
  pp.filter_cells      obs['n_counts'] = X.sum(1), keeps n_counts >= min_counts, in place
  pp.normalize_total   X * (target / row sum) (0 for a cell without counts), in place or on a copy
  pp.scale             zero_center=False: every column divided by its ddof=1 std (a zero std left as 1), then
                       X[X > max_value] = max_value
  write                records the call (nothing is written)

Input (tests/_filter_ref.make_inputs): seeded ``synth.topic_counts``, gene names with 'MT-' at the start and inside,
with '.', a duplicated name whose first replacement exists already, a cell without counts, and an ADT block.  Stored:
  flt_<run>_cells / _genes / _n_counts / _pct_mito / _n_cells / _indptr / _indices / _data
        filter_adata for the argument sets _filter_ref.FILTER_RUNS (the kept names, obs and var columns of the result, its
        CSR arrays; no _pct_mito without a threshold, no _n_cells when min_cells_per_gene is None); CSR and dense input
        give the same values (asserted; for preprocess_for_cnmf where the reference
        takes dense input: without ADT data)
  tp_rna_* / tp_adt_*    the CSR arrays of the library-size-normalised RNA and ADT blocks: the three
        preprocess_for_cnmf inputs (single modality with exclude_genes, feature_type_col, the list of 2) share them --
        the tool asserts that every run's tp10k is exactly [RNA block] or [RNA block | ADT block]
  pf_<run>_tp_genes / _hvgs / _rna_indptr / _rna_indices / _rna_data
        the TP10K gene order, the HVG list and the CSR arrays of adata_RNA of every run ('list' shares 'ftype''s adata_RNA:
        asserted equal)

Run:  python tools/make_golden_filter.py      (seconds; needs the reference source tree scanpy_shim.REFERENCE_SRC names)
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

from tests import _filter_ref as F  # noqa: E402


# ---------------------------------------------------------------- scanpy stand-in
def make_index_unique(index, join="-"):
    """anndata/utils.py make_index_unique"""
    if index.is_unique:
        return index
    from collections import Counter
    values = index.values.copy()
    dup = index.duplicated(keep="first")
    values_dup = values[dup]
    taken = set(values)
    counter = Counter()
    for i, v in enumerate(values_dup):
        while True:
            counter[v] += 1
            name = v + join + str(counter[v])
            if name not in taken:
                taken.add(name)
                values_dup[i] = name
                break
    values[dup] = values_dup
    return pd.Index(values, name=index.name)


def _positions(key, index):
    if isinstance(key, slice):
        assert key == slice(None)
        return np.arange(len(index))
    if isinstance(key, pd.Series):
        key = key.values
    key = np.asarray(key)
    if key.dtype == bool:
        assert key.shape == (len(index),)
        return np.flatnonzero(key)
    if key.size == 0:
        return np.zeros(0, dtype=np.int64)
    where = {}
    for i, name in enumerate(index):
        where.setdefault(name, []).append(i)
    return np.array([i for name in key for i in where[name]], dtype=np.int64)


class AnnData:
    def __init__(self, X, obs=None, var=None):
        self.X = sp.csr_matrix(X) if sp.issparse(X) else np.asarray(X)
        self.obs = obs if obs is not None else pd.DataFrame(index=[str(i) for i in range(X.shape[0])])
        self.var = var if var is not None else pd.DataFrame(index=[str(i) for i in range(X.shape[1])])
        self.obsm = {}

    @property
    def shape(self):
        return self.X.shape

    @property
    def obs_names(self):
        return self.obs.index

    @property
    def var_names(self):
        return self.var.index

    def var_names_make_unique(self, join="-"):
        self.var.index = make_index_unique(self.var.index, join)

    def copy(self):
        return AnnData(self.X.copy(), self.obs.copy(), self.var.copy())

    def __getitem__(self, key):
        rows, cols = key
        r, c = _positions(rows, self.obs.index), _positions(cols, self.var.index)
        return AnnData(self.X[r][:, c].copy(), self.obs.iloc[r].copy(), self.var.iloc[c].copy())

    def _subset_inplace(self, r=None, c=None):
        if r is not None:
            self.X, self.obs = self.X[np.flatnonzero(r)], self.obs.iloc[np.flatnonzero(r)].copy()
        if c is not None:
            self.X, self.var = self.X[:, np.flatnonzero(c)], self.var.iloc[np.flatnonzero(c)].copy()


def filter_genes(adata, min_cells=None):
    n = np.asarray((adata.X > 0).sum(axis=0)).ravel()
    adata.var["n_cells"] = n
    adata._subset_inplace(c=n >= min_cells)


def filter_cells(adata, min_counts=None):
    n = np.asarray(adata.X.sum(axis=1)).ravel()
    adata.obs["n_counts"] = n
    adata._subset_inplace(r=n >= min_counts)


def normalize_total(adata, target_sum=None, copy=False):
    a = adata.copy() if copy else adata
    X = a.X
    rs = np.asarray(X.sum(axis=1)).ravel()
    f = np.where(rs > 0, target_sum / np.where(rs > 0, rs, 1.0), 0.0)
    if sp.issparse(X):
        X = sp.csr_matrix(X, dtype=np.float64)
        X.data = X.data * np.repeat(f, np.diff(X.indptr))
    else:
        X = X * f[:, None]
    a.X = X
    return a if copy else None


def scale(adata, zero_center=True, max_value=None):
    assert not zero_center
    X = adata.X
    D = np.asarray(X.todense()) if sp.issparse(X) else np.asarray(X)
    std = D.std(axis=0, ddof=1)
    std[std == 0] = 1.0
    if sp.issparse(X):
        X = sp.csr_matrix(X, dtype=np.float64)
        X.data = X.data / std[X.indices]
        if max_value is not None:
            X.data[X.data > max_value] = max_value
    else:
        X = X / std
        if max_value is not None:
            X[X > max_value] = max_value
    adata.X = X


WRITTEN = []


def make_scanpy():
    mod = types.ModuleType("scanpy")
    mod.AnnData = AnnData
    mod.pp = types.SimpleNamespace(filter_genes=filter_genes, filter_cells=filter_cells, normalize_total=normalize_total,
                                   scale=scale)
    mod.write = lambda path, adata: WRITTEN.append(path)
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


def csr_of(X):
    X = sp.csr_matrix(X, dtype=np.float64)
    X.sort_indices()
    return X


def put_csr(store, prefix, X):
    X = csr_of(X)
    store[prefix + "indptr"], store[prefix + "indices"], store[prefix + "data"] = X.indptr, X.indices, X.data


def save_npz_fixed(path, store):
    """np.savez_compressed's container with a fixed member date: the same arrays give the same bytes on any day"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, arr in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref = load_reference()
    C, cells, genes, A, adt_names, hv = F.make_inputs()
    obs = F.obs_frame(cells)
    P = ref.Preprocess(random_seed=0)
    store = {"params": np.array(F.PARAMS, dtype=np.float64)}

    # ---- filter_adata
    for run, kw in F.FILTER_RUNS.items():
        outs = []
        for X in (sp.csr_matrix(C), C.copy()):
            a = P.filter_adata(AnnData(X, obs.copy(), pd.DataFrame(index=genes)), makeplots=False, **kw)
            outs.append(a)
        a, d = outs
        assert np.array_equal(csr_of(a.X).toarray(), d.X) and list(a.obs_names) == list(d.obs_names)
        assert list(a.var_names) == list(d.var_names) and a.obs.equals(d.obs) and a.var.equals(d.var)
        pre = "flt_%s_" % run
        store[pre + "cells"], store[pre + "genes"] = np.array(list(a.obs_names)), np.array(list(a.var_names))
        store[pre + "n_counts"] = a.obs["n_counts"].values.astype(np.float64)
        if "pct_mito" in a.obs.columns:
            store[pre + "pct_mito"] = a.obs["pct_mito"].values.astype(np.float64)
        if "n_cells" in a.var.columns:
            store[pre + "n_cells"] = a.var["n_cells"].values.astype(np.int64)
        put_csr(store, pre, a.X)
        print(run, a.shape)

    # ---- preprocess_for_cnmf: single modality + exclude_genes, feature_type_col, list of 2
    ftype = np.array(["Gene Expression"] * len(genes) + [F.ADT_NAME] * len(adt_names))
    all_genes = list(genes) + list(adt_names)

    def rna_adata(X):
        return AnnData(X, obs.copy(), pd.DataFrame({"highly_variable": hv}, index=genes))

    def both_adata(X):
        var = pd.DataFrame({"highly_variable": np.r_[hv, np.zeros(len(adt_names), dtype=bool)], "ftype": ftype},
                           index=all_genes)
        return AnnData(X, obs.copy(), var)

    def adt_adata(X):
        return AnnData(X, obs.copy(), pd.DataFrame(index=adt_names))

    runs = {
        "single": lambda f: P.preprocess_for_cnmf(rna_adata(f(C)), n_top_rna_genes=None, makeplots=False,
                                                  librarysize_targetsum=F.TARGET, exclude_genes=F.EXCLUDE),
        "ftype": lambda f: P.preprocess_for_cnmf(both_adata(f(np.hstack([C, A]))), feature_type_col="ftype",
                                                 adt_feature_name=F.ADT_NAME, n_top_rna_genes=None, makeplots=False,
                                                 librarysize_targetsum=F.TARGET),
        "list": lambda f: P.preprocess_for_cnmf([rna_adata(f(C)), adt_adata(f(A))], n_top_rna_genes=None,
                                                makeplots=False, librarysize_targetsum=F.TARGET),
    }
    rna_block = adt_block = None
    for run, call in runs.items():
        a, tp, hvgs = call(sp.csr_matrix)
        if run == "single":             # (with ADT data the reference takes sparse input only: scipy's hstack of ndarrays)
            a_d, tp_d, hvgs_d = call(np.array)
            assert hvgs == hvgs_d and list(tp.var_names) == list(tp_d.var_names)
            assert np.array_equal(csr_of(tp.X).toarray(), tp_d.X)
            assert np.array_equal(csr_of(a.X).toarray(), a_d.X)
        assert list(tp.obs_names) == cells and list(a.var_names) == hvgs
        T = csr_of(tp.X)
        g = len(genes)
        if rna_block is None:
            rna_block = T[:, :g]
        assert F.same_csr(csr_of(T[:, :g]), csr_of(rna_block)), run
        if T.shape[1] > g:
            if adt_block is None:
                adt_block = T[:, g:]
            assert F.same_csr(csr_of(T[:, g:]), csr_of(adt_block)), run
        pre = "pf_%s_" % run
        store[pre + "tp_genes"], store[pre + "hvgs"] = np.array(list(tp.var_names)), np.array(hvgs)
        if run == "list":
            ref_a = sp.csr_matrix((store["pf_ftype_rna_data"], store["pf_ftype_rna_indices"], store["pf_ftype_rna_indptr"]),
                                  shape=a.shape)
            assert F.same_csr(csr_of(a.X), ref_a) and hvgs == list(store["pf_ftype_hvgs"])
        else:
            put_csr(store, pre + "rna_", a.X)
        print(run, a.shape, tp.shape, len(hvgs))
    put_csr(store, "tp_rna_", rna_block)
    put_csr(store, "tp_adt_", adt_block)
    assert not WRITTEN
    out = os.path.join(ROOT, "tests", "golden", "ref_filter.npz")
    save_npz_fixed(out, store)
    print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
