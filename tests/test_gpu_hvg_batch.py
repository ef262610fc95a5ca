"""Preprocess.highly_variable_genes(batch_key=...) and ``hvg_batch_key`` on the device against the float64 numpy
restatement tests/_seurat_v3_batch_ref.py: the two batched entry points of csrc/hvg_batch_host.hip.h one by one, then the
frame, the selected set and the public route end to end.

Data: test_gpu_hvg.py's Gamma-Poisson counts at 300 x 600 (seed 1) and 257 x 1000 (seed 2), n_top_genes = 120, with
interleaved batches of 64, 65 and 171 cells (exactly one wavefront, one more, an odd size) and of 128 and 129; genes 0 and
1 are empty everywhere and several genes have no entry in some batch.

What is exact: the integer moments, means and variances; the float64 clipped sums of a batch have the BITS of the
one-batch entry point on the staging restricted to that batch (the same additions in the same order).  variances_norm is
held to 16 x the restatement's distance from its own ``np.longdouble`` run; ranks, nbatches and the selected set are
equal on two conditions asserted on the restatement alone (test_preconditions).  Every test prints its distances;
measured on an MI355X, 300 x 600 and 257 x 1000:

  variances_norm (max abs difference, restatement vs long double / device vs restatement; CSR and dense input alike)
      interpolate 1.9e-15 / 2.0e-15 (1.07 x), 8.0e-15 / 8.9e-15 (1.10 x, the most)
      direct      3.3e-15 / 2.7e-15 (0.80 x), 8.6e-15 / 8.9e-15 (1.03 x)
  C1, C2 against the restatement: equal in every batch (the bound is 2 N_b u)
  smallest relative gap between unequal variances_norm of a batch: 2.2e-7 (300 x 600), 2.7e-8 (257 x 1000)
  genes tied bit for bit with another, per batch: 152 to 413; of them with any entry above the clip: 0 to 6, never more
  than one such entry"""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import _lib
from cnmf_amd.preprocess import Preprocess
from tests import _filter_ref as F
from tests import _seurat_v3_batch_ref as B
from tests import _seurat_v3_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHAPES = [(300, 600, 1, (64, 65, 171)), (257, 1000, 2, (128, 129))]
N_TOP = 120
SURFACES = ("interpolate", "direct")
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


class Case:
    def __init__(self, N, G, seed, sizes):
        self.N, self.G, self.sizes = N, G, sizes
        self.C = R.gamma_poisson_counts(N, G, seed)
        self.cells, self.genes = ["c%d" % i for i in range(N)], ["g%d" % j for j in range(G)]
        self.stored = R.with_stored_zeros(self.C, seed)
        self.labels = B.interleaved_labels(N, sizes, seed)
        self.obs = pd.DataFrame({"batch": ["b%d" % x for x in self.labels]}, index=self.cells)
        self.frame, self.parts, self.frame_ld = {}, {}, {}
        for surface in SURFACES:
            self.frame[surface], self.parts[surface] = B.seurat_v3_batch(self.C, self.labels, N_TOP, surface=surface,
                                                                         genes=self.genes, parts=True)
            self.frame_ld[surface] = B.seurat_v3_batch(self.C, self.labels, N_TOP, surface=surface, genes=self.genes, dtype=LD)
        self.codes = self.parts["interpolate"]["codes"]
        self.nb = len(sizes)

    def data(self, dense):
        return pd.DataFrame(self.C, index=self.cells, columns=self.genes) if dense else (sp.csr_matrix(self.C), self.cells,
                                                                                        self.genes)

    def rows(self, b):
        return self.codes == b


@pytest.fixture(scope="module")
def cases():
    return [Case(*s) for s in SHAPES]


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_preconditions(cases):
    """On the restatement alone: the inputs hold what the head of this file claims; in every batch two variances_norm that
    are not equal bit for bit differ by more than 1e-9 relatively; and no gene that is tied bit for bit with another has
    four or more entries above its clip (a tie of genes whose batch columns hold the same few counts survives any order
    of at most three clipped terms and the integers).  These make rank equality a fair demand on the device."""
    for c in cases:
        assert list(np.bincount(c.codes)) == list(c.sizes) and (np.diff(c.codes) != 0).sum() > c.N // 4    # interleaved
        assert not c.C[:, :2].any() and c.stored.nnz > (c.C != 0).sum() and not c.stored.has_sorted_indices
        empty_somewhere = sum(int(((c.C[c.rows(b)] != 0).sum(axis=0) == 0)[2:].sum()) for b in range(c.nb))
        assert empty_somewhere >= 3
        for surface in SURFACES:
            p = c.parts[surface]
            for b in range(c.nb):
                v = p["vnorm"][b]
                s = np.unique(v)
                gap = ((s[1:] - s[:-1]) / s[1:]).min()
                tied = np.flatnonzero(np.bincount(np.searchsorted(s, v))[np.searchsorted(s, v)] > 1)
                above = (c.C[c.rows(b)][:, tied] > p["clip"][b][tied]).sum(axis=0)
                print("%d x %d %s batch %d: smallest relative gap %.3e, %d tied genes, %d of them with a clipped entry "
                      "(at most %d)" % (c.N, c.G, surface, b, gap, tied.size, (above > 0).sum(), above.max()))
                assert gap > 1e-9
                assert above.max() < 4


def test_moments_are_exact_per_batch(engine, cases):
    """the batched S1 and S2 equal the restatement's integers over the CSR as stored, and the one-batch entry point on
    the staging restricted to each batch; flags are 0"""
    for c in cases:
        p = c.parts["interpolate"]
        engine.preprocess_upload_as_stored(c.stored)
        s1, s2, flags = engine.preprocess_gene_moments_batched(c.codes, c.nb)
        assert s1.dtype == np.int64 and s1.shape == (c.nb, c.G) and flags.shape == (c.nb,) and not flags.any()
        assert np.array_equal(s1, p["s1"]) and np.array_equal(s2, p["s2"])
        assert (s1[:, :2] == 0).all() and ((s1 == 0).sum(axis=1) > 2).all()       # empty runs give zeros
        again = engine.preprocess_gene_moments_batched(c.codes, c.nb)
        assert np.array_equal(again[0], s1) and np.array_equal(again[1], s2)
        for b in range(c.nb):
            engine.preprocess_upload_as_stored(c.stored)
            engine.preprocess_subset(keep_cells=c.rows(b))
            t1, t2, f = engine.preprocess_gene_moments()
            assert f == 0 and np.array_equal(t1, s1[b]) and np.array_equal(t2, s2[b])


def test_flags_name_the_batch(engine, cases):
    c = cases[0]
    for value, flag in ((0.5, R.FLAG_NOT_COUNT), (2.0 ** 20 + 1, R.FLAG_TOO_LARGE)):
        bad = c.stored.copy()
        k = int(np.flatnonzero(np.repeat(c.codes, np.diff(bad.indptr)) == 1)[3])   # a stored entry of a cell of batch 1
        bad.data[k] = value
        engine.preprocess_upload_as_stored(bad)
        flags = engine.preprocess_gene_moments_batched(c.codes, c.nb)[2]
        assert list(flags) == [0, flag, 0]
        assert list(B.gene_moments_batched(bad, c.codes, c.nb)[2]) == [0, flag, 0]


def test_clipped_sums_have_the_bits_of_the_one_batch_entry_point(engine, cases):
    """C1 and C2 of batch b with the restatement's clip[b]: the bits of ``preprocess_clipped_sums(clip[b])`` on the staging
    restricted to b; within 2 N_b u of the restatement, relatively (either sum of n <= N_b non-negative terms is within
    (n - 1) u of the exact sum, whatever its order); a second call gives the same bits."""
    for c in cases:
        p = c.parts["interpolate"]
        engine.preprocess_upload_as_stored(c.stored)
        c1, c2 = engine.preprocess_clipped_sums_batched(c.codes, c.nb, p["clip"])
        d1, d2 = engine.preprocess_clipped_sums_batched(c.codes, c.nb, p["clip"])
        assert np.array_equal(bits(c1), bits(d1)) and np.array_equal(bits(c2), bits(d2))
        for got, want, what in ((c1, p["c1"], "C1"), (c2, p["c2"], "C2")):
            rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
            print("%d x %d %s: max relative difference per batch %s" % (c.N, c.G, what, ["%.3e" % r.max() for r in rel]))
            for b in range(c.nb):
                assert rel[b].max() <= 2 * c.sizes[b] * U
        assert (c1[:, :2] == 0).all() and (c2[:, :2] == 0).all()
        for b in range(c.nb):
            engine.preprocess_upload_as_stored(c.stored)
            engine.preprocess_subset(keep_cells=c.rows(b))
            t1, t2 = engine.preprocess_clipped_sums(p["clip"][b])
            assert np.array_equal(bits(t1), bits(c1[b])) and np.array_equal(bits(t2), bits(c2[b])), b


def test_the_staging_is_left_intact(engine, cases):
    c = cases[1]
    p = c.parts["interpolate"]
    engine.preprocess_upload_as_stored(c.stored)
    before = (engine.preprocess_fetch_counts(), engine.preprocess_gene_moments(), engine.preprocess_clipped_sums(p["clip"][0]))
    engine.preprocess_gene_moments_batched(c.codes, c.nb)
    engine.preprocess_clipped_sums_batched(c.codes, c.nb, p["clip"])
    after = (engine.preprocess_fetch_counts(), engine.preprocess_gene_moments(), engine.preprocess_clipped_sums(p["clip"][0]))
    assert F.same_csr(before[0], after[0]) and F.same_csr(after[0], sp.csr_matrix(c.stored))
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1]) and after[1][2] == 0
    assert np.array_equal(bits(before[2][0]), bits(after[2][0])) and np.array_equal(bits(before[2][1]), bits(after[2][1]))
    # other codes: the cached grouping is rebuilt; a subset drops it
    other = (c.codes + 1) % c.nb
    s1 = engine.preprocess_gene_moments_batched(other, c.nb)[0]
    assert np.array_equal(s1, p["s1"][(np.arange(c.nb) - 1) % c.nb])
    keep = np.arange(c.N) % 3 != 0
    engine.preprocess_subset(keep_cells=keep)
    s1 = engine.preprocess_gene_moments_batched(c.codes[keep], c.nb)[0]
    assert np.array_equal(s1, B.gene_moments_batched(c.stored[np.flatnonzero(keep)], c.codes[keep], c.nb)[0])


def test_frame(engine, cases):
    """CSR and dense input, both surfaces: means and variances with the restatement's bits, variances_norm within 16 x the
    restatement's distance from its long double run, nbatches, rank and the selected set equal"""
    failures = []
    P = Preprocess(engine=engine)
    for c in cases:
        for surface in SURFACES:
            want, ld = c.frame[surface], c.frame_ld[surface]
            base = maxdiff(want["variances_norm"].values, ld["variances_norm"].values.astype(LD))
            for dense in (False, True):
                got = P.highly_variable_genes(c.data(dense), n_top_genes=N_TOP, surface=surface, batch_key="batch", obs=c.obs)
                assert list(got.index) == c.genes and list(got.columns) == list(want.columns)
                assert np.array_equal(bits(got["means"]), bits(want["means"]))
                assert np.array_equal(bits(got["variances"]), bits(want["variances"]))
                err = maxdiff(got["variances_norm"].values, want["variances_norm"].values)
                print("%d x %d %s %s variances_norm: restatement vs long double %.3e, device vs restatement %.3e (%.2f x)"
                      % (c.N, c.G, surface, "dense" if dense else "csr", base, err, err / base))
                if not err <= 16 * base:
                    failures.append((c.N, surface, dense, err, base))
                assert np.array_equal(got["highly_variable_nbatches"].values, want["highly_variable_nbatches"].values)
                assert np.array_equal(got["highly_variable_rank"].values, want["highly_variable_rank"].values, equal_nan=True)
                assert np.array_equal(got["highly_variable"].values, want["highly_variable"].values)
                assert got["highly_variable"].sum() == N_TOP
    assert not failures, failures


def test_normalize_batchcorrect_end_to_end(engine, cases):
    """hvg_batch_key selects the restatement's genes, and result.X is that of a call given those genes"""
    P = Preprocess(engine=engine)
    for c, dense in zip(cases, (False, True)):
        want = c.frame["interpolate"]
        mask = want["highly_variable"].values
        res, hvgs = P.normalize_batchcorrect(c.data(dense), obs=c.obs, hvg="device", n_top_genes=N_TOP, hvg_batch_key="batch",
                                             makeplots=False)
        ref, hvgs_ref = P.normalize_batchcorrect(c.data(dense), obs=c.obs, highly_variable=mask, makeplots=False)
        assert hvgs == hvgs_ref == list(want.index[mask]) and len(hvgs) == N_TOP
        assert list(res.var_names) == list(ref.var_names) and list(res.obs_names) == list(ref.obs_names)
        if sp.issparse(res.X):
            assert F.same_csr(sp.csr_matrix(res.X), sp.csr_matrix(ref.X))
        else:
            assert np.array_equal(bits(res.X), bits(ref.X))
        assert list(res.var.index) == hvgs and (res.var["highly_variable_nbatches"] >= 1).all()
        assert np.array_equal(res.var["highly_variable_nbatches"].values, want["highly_variable_nbatches"].values[mask])


def test_limits_are_refused_before_any_launch(engine, cases):
    """a code outside the range, an empty batch and too many batches: the wrapper's errors, and the library's own
    CNMF_EINVAL (with its text) when the wrapper is bypassed; nothing ran, the staging answers as before"""
    import ctypes as C
    c = cases[0]
    engine.preprocess_upload_as_stored(c.stored)
    bad = c.codes.copy()
    bad[11] = c.nb
    with pytest.raises(ValueError, match="outside"):
        engine.preprocess_gene_moments_batched(bad, c.nb)
    bad[11] = -1
    with pytest.raises(ValueError, match="outside"):
        engine.preprocess_clipped_sums_batched(bad, c.nb, np.ones((c.nb, c.G)))
    with pytest.raises(ValueError, match="batch 3 has no cell"):
        engine.preprocess_gene_moments_batched(c.codes, c.nb + 1)
    with pytest.raises(NotImplementedError, match="batches"):
        engine.preprocess_gene_moments_batched(c.codes, _lib.CNMF_HVG_BATCHES_MAX + 1)
    with pytest.raises(ValueError, match="clip"):
        engine.preprocess_clipped_sums_batched(c.codes, c.nb, np.ones(c.G))
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    s = np.full((c.nb + 1, c.G), -7, dtype=np.int64)
    f = np.zeros(c.nb + 1, dtype=np.int32)

    def raw(codes, nb):
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        rc = engine._lib.cnmf_preprocess_gene_moments_batched(engine._ctx, codes.ctypes.data_as(i32p), nb, s.ctypes.data_as(i64p),
                                                              s.ctypes.data_as(i64p), f.ctypes.data_as(i32p))
        return rc, engine._lib.cnmf_last_error(engine._ctx).decode()

    bad[11] = c.nb
    for codes, nb, text in ((bad, c.nb, "batch code 3 of cell 11 outside [0, 3)"), (c.codes, c.nb + 1, "batch 3 has no cell"),
                            (c.codes, _lib.CNMF_HVG_BATCHES_MAX + 1, "4097 batches"), (c.codes, 0, "0 batches")):
        rc, err = raw(codes, nb)
        assert rc != 0 and text in err, (rc, err)
    assert (s == -7).all()                                                         # nothing was written
    s1 = engine.preprocess_gene_moments_batched(c.codes, c.nb)[0]
    assert np.array_equal(s1, c.parts["interpolate"]["s1"])
    engine.preprocess_release()
    with pytest.raises(RuntimeError):
        engine.preprocess_gene_moments_batched(c.codes, c.nb)
