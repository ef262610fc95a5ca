"""Host side of the per-batch HVG tests (test_host_hvg_batch.py, test_gpu_hvg_batch.py): a numpy restatement of scanpy's
``highly_variable_genes(flavor='seurat_v3', batch_key=...)`` on top of the one-batch restatement tests/_seurat_v3_ref.py
(imported, not changed), and a device-free engine whose two batched entry points are played by it.  **This file is the
yardstick of Preprocess.highly_variable_genes(batch_key=...)**: agreement with scanpy itself is unmeasured on this
project's machines (scanpy and skmisc are not installed on them); test_host_hvg_batch.py compares this restatement with
scanpy wherever both can be imported.

Batches.  With labels ``batch[N]`` the batches are the values of ``np.unique(batch)``, in that order.  For every batch b
with N_b cells the one-batch computation (``R.seurat_v3``) runs on that batch's rows alone: integer moments, mean and
ddof=1 variance, the loess over the genes with var_b > 0 (same span, surface and q rule), reg_std_b,
clip_b = reg_std_b sqrt(N_b) + mean_b, the clipped sums and variances_norm_b.

Combination (scanpy's own expressions, the sorts made stable):
* rank of gene g in batch b = ``argsort(argsort(-variances_norm_b))`` (stable: ties in gene order), as float32;
* highly_variable_nbatches = the number of batches with rank < n_top_genes; ranks >= n_top_genes become NaN;
* highly_variable_rank = ``np.ma.median`` over the batches of the ranks that are not NaN (NaN when all are);
* variances_norm = ``np.mean`` over the batches;
* means and variances are those of the whole data (S1 = sum_b S1_b, S2 = sum_b S2_b, one division each): the bits of the
  one-batch restatement on all cells;
* highly_variable = the first n_top_genes genes of ``DataFrame.sort_values([rank, nbatches], ascending=[True, False],
  na_position='last')`` (a stable sort: ties in gene order).
highly_variable_rank is kept as float64 (the one-batch frame's dtype; the values are scanpy's float32 ones)."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from tests import _seurat_v3_ref as R

BATCHES_MAX = 4096


def batches(batch):
    """(labels, codes [N], sizes [B]) of the labels ``batch``"""
    labels, codes = np.unique(np.asarray(batch), return_inverse=True)
    codes = codes.reshape(-1)
    return labels, codes, np.bincount(codes, minlength=labels.size)


def interleaved_labels(N, sizes, seed):
    """the labels of the GPU tests: batches of the given sizes, interleaved by a permutation"""
    assert sum(sizes) == N
    return np.repeat(np.arange(len(sizes)), sizes)[np.random.RandomState(seed + 10).permutation(N)]


def gene_moments_batched(X, codes, B):
    """(S1 int64 [B][G], S2 int64 [B][G], flags int32 [B]): ``R.gene_moments`` over the rows of every batch"""
    X = sp.csr_matrix(X)
    codes = np.asarray(codes)
    out = [R.gene_moments(X[np.flatnonzero(codes == b)]) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


def clipped_sums_batched(X, codes, B, clip, dtype=np.float64):
    """(C1 [B][G], C2 [B][G]): ``R.clipped_sums`` over the rows of every batch with clip[b]"""
    X = sp.csr_matrix(X)
    codes = np.asarray(codes)
    out = [R.clipped_sums(X[np.flatnonzero(codes == b)], clip[b], dtype) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def combine(vnorm, n_top_genes, mean, var, genes):
    """scanpy's combination of the per-batch variances_norm [B][G] into its frame (see the head of this file)"""
    vnorm = np.asarray(vnorm)
    ranked = np.argsort(np.argsort(-vnorm.astype(np.float64), axis=1, kind="stable"), axis=1, kind="stable")
    ranked = ranked.astype(np.float32)
    nbatches = np.sum((ranked < n_top_genes).astype(int), axis=0)
    ranked[ranked >= n_top_genes] = np.nan
    median = np.ma.median(np.ma.masked_invalid(ranked), axis=0).filled(np.nan)
    df = pd.DataFrame({"means": mean, "variances": var, "variances_norm": np.mean(vnorm, axis=0),
                       "highly_variable_rank": np.asarray(median, dtype=np.float64)}, index=pd.Index(genes))
    df["highly_variable"] = False
    df["highly_variable_nbatches"] = np.asarray(nbatches, dtype=np.int64)
    cols = ["highly_variable_rank", "highly_variable_nbatches"]
    order = df[cols].sort_values(cols, ascending=[True, False], na_position="last", kind="stable").index
    df.loc[order[:int(n_top_genes)], "highly_variable"] = True
    return df


def seurat_v3_batch(X, batch, n_top_genes=2000, span=0.3, surface="interpolate", genes=None, dtype=np.float64, parts=False):
    """scanpy's frame with batch_key for the cells x genes counts X and the labels ``batch`` [N]; ``parts``: also a dict of
    the per-batch arrays ([B][G]: s1, s2, mean, var, clip, c1, c2, vnorm) with ``codes`` and ``sizes``"""
    X = sp.csr_matrix(X)
    N, G = X.shape
    labels, codes, sizes = batches(batch)
    if codes.size != N:
        raise ValueError("%d labels for %d cells" % (codes.size, N))
    if (sizes < 2).any():
        raise ValueError("batch %r has fewer than 2 cells" % (labels[np.flatnonzero(sizes < 2)[0]],))
    B = labels.size
    per = [R.seurat_v3(X[np.flatnonzero(codes == b)], n_top_genes, span, surface, dtype=dtype, parts=True)[1] for b in range(B)]
    keys = ("s1", "s2", "mean", "var", "clip", "c1", "c2", "vnorm")
    P = {k: np.stack([p[k] for p in per]) for k in keys}
    mean, var = R.mean_var(P["s1"].sum(axis=0), P["s2"].sum(axis=0), N, dtype)
    genes = pd.Index(["gene%d" % j for j in range(G)]) if genes is None else pd.Index(genes)
    frame = combine(P["vnorm"], n_top_genes, mean, var, genes)
    if parts:
        return frame, dict(P, codes=codes, sizes=sizes, labels=labels)
    return frame


# ---------------------------------------------------------------- a device-free engine
class FakeHvgBatchEngine(R.FakeHvgEngine):
    """tests/_seurat_v3_ref.py's engine with the two batched entry points played by the restatement"""

    def _check_codes(self, codes, n_batches):
        codes, B = np.asarray(codes), int(n_batches)
        if not 1 <= B <= BATCHES_MAX:
            raise NotImplementedError("%d batches" % B)
        if codes.shape != (self.X.shape[0],) or codes.min() < 0 or codes.max() >= B:
            raise ValueError("batch codes outside [0, %d)" % B)
        if (np.bincount(codes, minlength=B) == 0).any():
            raise ValueError("a batch has no cell")
        return codes, B

    def preprocess_gene_moments_batched(self, codes, n_batches):
        self.calls.append("gene_moments_batched")
        codes, B = self._check_codes(codes, n_batches)
        return gene_moments_batched(self.X, codes, B)

    def preprocess_clipped_sums_batched(self, codes, n_batches, clip):
        self.calls.append("clipped_sums_batched")
        codes, B = self._check_codes(codes, n_batches)
        clip = np.asarray(clip, dtype=np.float64)
        assert clip.shape == (B, self.X.shape[1])
        return clipped_sums_batched(self.X, codes, B, clip)
