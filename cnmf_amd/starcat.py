"""Projection of query cells onto a fixed set of reference programs (starCAT) on the device.

Provenance.  The recipe is the published one (Kotliar et al., "Reproducible single cell annotation of programs underlying
T-cell subsets, activation states, and functions", starCAT): take the reference programs x genes matrix that
``cNMF.build_reference`` writes (``starcat_spectra``: TPM spectra renormalised and divided by the genes' TPM standard
deviation, high-variance genes only), keep the genes the query also has, scale every such gene of the query's raw counts to
unit variance WITHOUT centring (``sc.pp.scale(zero_center=False)``: x / std with ddof = 1, a gene of zero variance left as
it is), and refit the usages with the programs fixed by scikit-learn's
``non_negative_factorization(X, H=reference, update_H=False, solver='mu', beta_loss='frobenius')``; the usages of a cell
are then normalised to sum to 1.  Here the scaling is the device ``prepare`` path (``Engine.prepare_upload`` /
``prepare_select``) and the refit is ``Engine.mu_frobenius_refit`` (cnmf_mu2_refit_f64, float64).

What is and is not measured: the refit is held to a numpy restatement of scikit-learn 1.7.2's update and to live
scikit-learn by this package's tests.  Agreement with the starCAT package itself is UNMEASURED on this project's machines:
it is not installed on them.  starCAT's reference-specific scores and its download of published references are out of scope.
"""
import os
import warnings

import numpy as np
import pandas as pd

from .cnmf import counts_to_csr, load_df_from_npz


def _input_is_dense(query):
    """Whether ``counts_to_csr`` was handed a dense matrix (a file, a DataFrame, an ndarray) rather than a sparse one."""
    import scipy.sparse as sp
    if isinstance(query, tuple) and len(query) == 3:
        query = query[0]
    return not sp.issparse(query)


class StarCAT:
    def __init__(self, reference, device=0, engine=None):
        """``reference``: a DataFrame programs x genes, or the path of a ``starcat_spectra`` file (``.df.npz`` or
        tab-separated text).  Values must be non-negative; a gene whose column holds a non-finite value (a gene of zero TPM
        variance in the run that built the reference) is dropped with a warning.  The engine (one per GPU) is created on
        first use, so argument errors raise without a device."""
        if isinstance(reference, (str, bytes, os.PathLike)):
            p = os.fsdecode(reference)
            # (the text with the exact parser: pandas' default one misses the written value by up to 1e-14 relative)
            reference = (load_df_from_npz(p) if p.endswith(".npz") else
                         pd.read_csv(p, sep="\t", index_col=0, float_precision="round_trip"))
        if not isinstance(reference, pd.DataFrame):
            raise TypeError("reference must be a DataFrame (programs x genes) or the path of a starcat_spectra file")
        vals = np.asarray(reference.values, dtype=np.float64)
        genes = pd.Index([str(g) for g in reference.columns])
        bad = ~np.isfinite(vals).all(axis=0)
        if bad.any():
            warnings.warn("dropping %d reference genes with non-finite values, e.g. %s"
                          % (int(bad.sum()), ", ".join(genes[bad][:4])))
            vals, genes = vals[:, ~bad], genes[~bad]
        if vals.shape[0] == 0 or vals.shape[1] == 0:
            raise ValueError("the reference holds no program or no gene with finite values")
        if vals.min() < 0:
            raise ValueError("Negative values in the reference spectra")
        if genes.has_duplicates:
            raise ValueError("duplicate gene names in the reference: %s" % list(genes[genes.duplicated()][:4]))
        self.reference = pd.DataFrame(np.ascontiguousarray(vals), index=[str(i) for i in reference.index], columns=genes)
        self.device = device
        self._engine = engine
        self.overlap_genes = None        # the reference genes the last query had, in the reference's order
        self.n_missing = None            # how many reference genes it lacked
        self.n_iter = None               # iterations and final error of the last refit
        self.err = None

    @property
    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self.device)
        return self._engine

    def fit_transform(self, query, tol=1e-4, max_iter=1000, return_unnormalized=False):
        """Usages of the reference programs in the cells of ``query`` (raw counts in any form ``counts_to_csr`` takes: a
        file path, a DataFrame, an ndarray, or ``(scipy.sparse matrix, cell names, gene names)``): a DataFrame cells x
        programs whose rows sum to 1 (a cell whose usages are all zero stays zero); with ``return_unnormalized`` the pair
        ``(normalised, raw usages)``.  The scaled query (cells x overlap genes) stays resident on the engine.  A dense
        input is scaled as a dense matrix, for which the engine refuses a gene of zero variance (ValueError); a sparse
        one leaves such a gene as it is."""
        densify = _input_is_dense(query)
        counts, cells, genes = counts_to_csr(query)
        if genes.has_duplicates:
            raise ValueError("duplicate gene names in the query: %s" % list(genes[genes.duplicated()][:4]))
        ref = self.reference
        cols = genes.get_indexer(ref.columns)
        have = cols >= 0
        self.overlap_genes = ref.columns[have]
        self.n_missing = int((~have).sum())
        if not have.any():
            raise ValueError("the query shares no gene with the reference")
        H = np.ascontiguousarray(ref.values[:, have])
        eng = self.engine
        try:
            eng.prepare_upload(counts)
            eng.prepare_select(cols[have], densify)
        finally:
            eng.prepare_release()                    # (the staging, also when a step above raised)
        W, self.n_iter, self.err = eng.mu_frobenius_refit(H, tol=tol, max_iter=max_iter)
        raw = pd.DataFrame(W, index=cells, columns=ref.index)
        total = raw.sum(axis=1)
        usage = raw.div(total.where(total != 0, 1.0), axis=0)
        return (usage, raw) if return_unnormalized else usage
