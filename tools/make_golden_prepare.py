"""Generate tests/golden/ref_prepare_sparse.npz by running the UNMODIFIED reference's sparse ``prepare``
(densify=False) through oracle/scanpy_shim.py, on the CPU.

Input: seeded ``synth.topic_counts`` -- a 6-programme matrix plus a one-programme ("housekeeping") matrix, so that the
genes of largest mean are not all programme genes -- 3 000 cells x 6 000 genes at mu_lib 5.5 (8 % non-zero), all-zero
genes dropped, int64 frame, cells ``c%d`` / genes ``g%d`` (make_counts: the GPU test regenerates it).  Three runs:

  top   num_highvar_genes=500          (top-N route, cnmf.py:160-163)
  thr   num_highvar_genes=None         (threshold route, cnmf.py:166-172) with tpm_fn = 5 x counts: at TPM scale
                                       T = 1 + std(fano) is far above every fano ratio and the route picks no gene
                                       (this data is Poisson around its programmes); on 5 x counts it picks a few,
                                       and the reference then stops at its zero-cell check (cnmf.py:550-554): stored
                                       are the genes it wrote (nmf_genes_list, written before the check) and the text
  file  genes_file = a shuffled list of 300 genes (cnmf.py:449-452: the file's order)

Stored (``<run>_`` prefix per run):
  genes                 the high-variance genes in the reference's column order
  indptr / indices      the norm_counts CSR structure (cells x genes)                          (top, file)
  counts / inv_std      its values in compact form: data = counts * inv_std[indices] in float64 is EXACTLY what the shim's
                        sc.pp.scale wrote (checked here before storing) -- 2 bytes per entry instead of 8
  tpm_stats             [G, 2]: __mean, __std (top and file share the TPM; thr has its own)
  gap                   relative fano-ratio gap at the cut (top / thr; the tool asserts > 1e-9 so that a last-bit
                        difference in the statistics cannot flip the list)
  error                 the exception text                                                     (thr)

Run:  python tools/make_golden_prepare.py          (a few seconds; needs the reference source tree scanpy_shim.REFERENCE_SRC names)
"""
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
import pandas as pd
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import synth  # noqa: E402
from oracle import scanpy_shim  # noqa: E402

# (n_cells, n_genes, k_true, mu_lib, sigma_lib, seed): the GPU test regenerates the counts from these
PARAMS = (3000, 6000, 6, 5.5, 0.4, 3)
N_TOP, N_FILE, FILE_SEED, THR_TPM_SCALE = 500, 300, 5, 5


def make_counts():
    n, g, k, mu, sg, seed = PARAMS
    C, _ = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    C += synth.topic_counts(n, g, 1, mu_lib=mu, sigma_lib=sg, seed=seed + 1)[0]
    C = C[:, C.sum(axis=0) > 0]
    return pd.DataFrame(C.astype(np.int64), index=["c%d" % i for i in range(C.shape[0])],
                        columns=["g%d" % j for j in range(C.shape[1])])


def file_genes(columns):
    rs = np.random.RandomState(FILE_SEED)
    return [columns[j] for j in rs.permutation(len(columns))[:N_FILE]]


def cut_gap(mean, var, numgenes):
    """Relative distance of the fano ratios next to the cut: top-N -> (r[N-1] - r[N]) / r[N-1] of the descending order;
    threshold -> min |r - T| / T over the genes with mean > 0.5, and min |mean - 0.5| / 0.5 over those with r > T."""
    from cnmf_amd.cnmf import select_highvar_genes
    _, p = select_highvar_genes(mean, var, numgenes=numgenes)
    r = p["fano_ratio"]
    if numgenes is not None:
        s = np.sort(r[np.isfinite(r)])[::-1]
        return float((s[numgenes - 1] - s[numgenes]) / s[numgenes - 1])
    T = p["T"]
    ok = np.isfinite(r)
    g1 = np.min(np.abs(r[ok & (mean > 0.5)] - T)) / T
    g2 = np.min(np.abs(mean[ok & (r > T)] - 0.5)) / 0.5
    return float(min(g1, g2))


def main():
    scanpy_shim.install()
    import scanpy as sc
    import cnmf as ref  # the unmodified reference
    from cnmf.cnmf import load_df_from_npz, save_df_to_npz

    counts = make_counts()
    print("counts", counts.shape, "non-zero %.2f %%" % (100.0 * (counts.values > 0).mean()))
    store = {"shape": np.array(counts.shape), "params": np.array(PARAMS), "thr_tpm_scale": np.array(THR_TPM_SCALE),
             "file_list": np.array(file_genes(list(counts.columns)))}
    tmp = tempfile.mkdtemp(prefix="cnmf_golden_prep_")
    try:
        counts_fn = os.path.join(tmp, "counts.df.npz")
        save_df_to_npz(counts, counts_fn)
        genes_fn = os.path.join(tmp, "genes.txt")
        with open(genes_fn, "w") as F:
            F.write("\n".join(file_genes(list(counts.columns))))
        tpm_fn = os.path.join(tmp, "tpm.df.npz")
        save_df_to_npz(counts * THR_TPM_SCALE, tpm_fn)
        runs = [("top", dict(num_highvar_genes=N_TOP)), ("thr", dict(num_highvar_genes=None, tpm_fn=tpm_fn)),
                ("file", dict(genes_file=genes_fn))]
        for tag, kw in runs:
            obj = ref.cNMF(output_dir=tmp, name=tag)
            err = None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                try:
                    obj.prepare(counts_fn, components=[5], n_iter=2, densify=False, seed=14, **kw)
                except Exception as e:       # the zero-cell check (cnmf.py:550-554)
                    err = str(e)
            stats = load_df_from_npz(obj.paths["tpm_stats"]).values
            store[tag + "_tpm_stats"] = stats
            if tag != "file":
                gap = cut_gap(stats[:, 0], stats[:, 1] ** 2, kw["num_highvar_genes"])
                assert gap > 1e-9, (tag, gap)
                store[tag + "_gap"] = np.array(gap)
            if err is not None:
                assert tag == "thr" and err.startswith("Error: "), (tag, err)
                store[tag + "_genes"] = np.array(open(obj.paths["nmf_genes_list"]).read().split("\n"))
                store[tag + "_error"] = np.array(err)
                print(tag, "genes", len(store[tag + "_genes"]), "gap", store[tag + "_gap"], "->", err[:60])
                continue
            nc = sc.read(obj.paths["normalized_counts"])
            X = nc.X.tocsr()
            assert X.has_sorted_indices
            genes = np.array(list(nc.var.index))
            raw = counts[list(genes)].values
            rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
            cnt = raw[rows, X.indices]
            assert cnt.max() < 65536 and (cnt > 0).all()
            # the shim's scale (oracle/scanpy_shim.py::_scale): X @ diags(1 / std) -- one float64 product per entry
            Xc = sp.csr_matrix(raw).astype(np.float64).tocsc()
            mean = np.asarray(Xc.mean(axis=0)).ravel()
            std = np.sqrt((np.asarray(Xc.multiply(Xc).mean(axis=0)).ravel() - mean ** 2) * raw.shape[0] / (raw.shape[0] - 1))
            std[std == 0] = 1
            inv = 1.0 / std
            assert np.array_equal(cnt.astype(np.float64) * inv[X.indices], X.data), tag
            store[tag + "_genes"] = genes
            store[tag + "_indptr"] = X.indptr.astype(np.int32)
            store[tag + "_indices"] = X.indices.astype(np.int16)
            store[tag + "_counts"] = cnt.astype(np.uint16)
            store[tag + "_inv_std"] = inv
            print(tag, "genes", len(genes), "nnz", X.nnz, "gap", store.get(tag + "_gap"))
        out = os.path.join(ROOT, "tests", "golden", "ref_prepare_sparse.npz")
        np.savez_compressed(out, **store)
        print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
