"""The per-batch seurat_v3 HVG selection (``batch_key``) without a device: the combination rule on hand-made input, the
numpy restatement (tests/_seurat_v3_batch_ref.py, the yardstick of ``Preprocess.highly_variable_genes(batch_key=...)``)
against the one-batch restatement and against its own invariances, the host half of the product route against the
restatement through an engine double whose batched device methods are played by it, the argument rules and the two
``hvg_batch_key`` routes.  The comparison with scanpy runs wherever scanpy and skmisc can be imported; they are not
installed on this project's machines."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import engine as engine_mod
from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import Preprocess
from tests import _filter_ref as F
from tests import _seurat_v3_batch_ref as B
from tests import _seurat_v3_ref as R

SHARED = ["means", "variances", "variances_norm", "highly_variable_rank", "highly_variable"]
COLUMNS = SHARED + ["highly_variable_nbatches"]
N, G, N_TOP = 150, 240, 40


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(engine_mod.Engine, "__init__", refuse)


@pytest.fixture(scope="module")
def case():
    C = R.gamma_poisson_counts(N, G, 3)
    cells, genes = ["c%d" % i for i in range(N)], ["g%d" % j for j in range(G)]
    labels = np.array(["A", "B", "C"])[B.interleaved_labels(N, (40, 45, 65), 3)]
    return C, cells, genes, labels


def data_of(C, cells, genes):
    return (sp.csr_matrix(C), cells, genes)


def obs_of(cells, labels, key="batch"):
    return pd.DataFrame({key: labels}, index=cells)


# ---------------------------------------------------------------- the combination rule
def combine_both(vnorm, n_top):
    """the product's rule and the restatement's on the same input: equal, returned as the product's tuple"""
    vnorm = np.asarray(vnorm, dtype=np.float64)
    vn, rank, nb, hv = pp.seurat_v3_combine(vnorm, n_top)
    g = ["g%d" % j for j in range(vnorm.shape[1])]
    want = B.combine(vnorm, n_top, np.zeros(len(g)), np.zeros(len(g)), g)
    assert np.array_equal(vn, want["variances_norm"].values)
    assert rank.dtype == np.float64 and np.array_equal(rank, want["highly_variable_rank"].values, equal_nan=True)
    assert nb.dtype == np.int64 and np.array_equal(nb, want["highly_variable_nbatches"].values)
    assert hv.dtype == bool and np.array_equal(hv, want["highly_variable"].values)
    return vn, rank, nb, hv


def test_combine_on_hand_made_input():
    # two batches, five genes, n_top_genes = 3: ranks (0, 1), (1, 0), (2, -), (-, 2), (-, -)
    vn, rank, nb, hv = combine_both([[5, 4, 3, 2, 1], [4, 5, 2, 3, 1]], 3)
    assert np.array_equal(rank, [0.5, 0.5, 2.0, 2.0, np.nan], equal_nan=True)      # an even number of ranks: x.5
    assert list(nb) == [2, 2, 1, 1, 0]                                             # the last gene: NaN in every batch
    assert list(hv) == [True, True, True, False, False]                            # (2.0, 1) tied: the earlier gene
    assert np.array_equal(vn, [4.5, 4.5, 2.5, 2.5, 1.0])
    # the same median rank, more batches first: gene 1 (rank 0 in two batches) before gene 0 (rank 0 in one)
    vn, rank, nb, hv = combine_both([[3, 2, 1], [1, 3, 2], [1, 3, 2]], 1)
    assert np.array_equal(rank, [0.0, 0.0, np.nan], equal_nan=True) and list(nb) == [1, 2, 0]
    assert list(hv) == [False, True, False]
    # three ranks: the middle one; values tied inside a batch rank in gene order
    vn, rank, nb, hv = combine_both([[2, 2, 2, 2], [2, 2, 2, 2], [1, 2, 3, 4]], 4)
    assert list(rank) == [0.0, 1.0, 2.0, 3.0] and list(nb) == [3, 3, 3, 3] and hv.all()
    # n_top_genes larger than G: nothing is NaN, everything is selected
    vn, rank, nb, hv = combine_both([[5, 4, 3, 2, 1], [4, 5, 2, 3, 1]], 7)
    assert np.array_equal(rank, [0.5, 0.5, 2.5, 2.5, 4.0]) and list(nb) == [2] * 5 and hv.all()
    # one batch: the rank itself
    vn, rank, nb, hv = combine_both([[1.0, 3.0, 3.0, 0.5, 3.0]], 2)
    assert np.array_equal(rank, [np.nan, 0.0, 1.0, np.nan, np.nan], equal_nan=True)
    assert list(hv) == [False, True, True, False, False] and list(nb) == [0, 1, 1, 0, 0]
    with pytest.raises(ValueError, match="batches"):
        pp.seurat_v3_combine(np.zeros(4), 2)


def test_combine_equals_the_restatement_on_tied_random_input():
    rs = np.random.RandomState(11)
    for nb, ng, n_top in ((1, 30, 7), (2, 31, 8), (3, 64, 20), (4, 50, 50), (5, 40, 3), (6, 25, 60)):
        combine_both(rs.randint(0, 12, size=(nb, ng)).astype(np.float64), n_top)    # many ties
        combine_both(rs.gamma(2.0, 1.0, size=(nb, ng)), n_top)


# ---------------------------------------------------------------- the restatement and the product's host half
def test_one_batch_is_the_one_batch_frame(case):
    C, cells, genes, _ = case
    want = R.seurat_v3(C, N_TOP, genes=genes)
    ref = B.seurat_v3_batch(C, np.zeros(N, dtype=int), N_TOP, genes=genes)
    eng = B.FakeHvgBatchEngine()
    got = Preprocess(engine=eng).highly_variable_genes(data_of(C, cells, genes), n_top_genes=N_TOP, batch_key="batch",
                                                       obs=obs_of(cells, ["only"] * N))
    for frame in (ref, got):
        assert list(frame.columns) == COLUMNS
        pd.testing.assert_frame_equal(frame[SHARED], want, check_exact=True)       # (NaN-aware, dtypes included)
        nb = frame["highly_variable_nbatches"].values
        assert nb.dtype == np.int64 and set(nb) == {0, 1} and np.array_equal(nb == 1, want["highly_variable"].values)
    assert eng._pre is None
    # without batch_key nothing changed: no extra column, the one-batch calls
    eng = B.FakeHvgBatchEngine()
    plain = Preprocess(engine=eng).highly_variable_genes(data_of(C, cells, genes), n_top_genes=N_TOP, obs=obs_of(cells, ["x"] * N))
    pd.testing.assert_frame_equal(plain, want, check_exact=True)
    assert "gene_moments" in eng.calls and "gene_moments_batched" not in eng.calls


def test_the_product_host_half_equals_the_restatement(case):
    """with the engine double the product's frame is the restatement's bit for bit on both surfaces -- so on the GPU any
    difference comes from the device entry points; means and variances have the bits of the call without batch_key"""
    C, cells, genes, labels = case
    for surface in ("interpolate", "direct"):
        eng = B.FakeHvgBatchEngine()
        got = Preprocess(engine=eng).highly_variable_genes(data_of(C, cells, genes), n_top_genes=N_TOP, surface=surface,
                                                           batch_key="batch", obs=obs_of(cells, labels))
        want = B.seurat_v3_batch(C, labels, N_TOP, surface=surface, genes=genes)
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        assert list(got.columns) == COLUMNS and got["highly_variable"].sum() == N_TOP
        assert eng.calls.count("gene_moments_batched") == 1 and eng.calls.count("clipped_sums_batched") == 1
        assert eng.calls.count("loess_fit") == 3 and "gene_moments" not in eng.calls and eng._pre is None
        plain = R.seurat_v3(C, N_TOP, surface=surface, genes=genes)
        for col in ("means", "variances"):
            assert np.array_equal(got[col].values.view(np.uint64), plain[col].values.view(np.uint64))
        nb = got["highly_variable_nbatches"].values
        assert nb.min() == 0 and nb.max() == 3
        assert np.array_equal(np.isnan(got["highly_variable_rank"].values), nb == 0)
        assert (got["variances_norm"].values[:2] == 0).all()                       # the all-zero genes
    # an obs in another order is aligned by name
    perm = np.random.RandomState(2).permutation(N)
    shuffled = obs_of(cells, labels).iloc[perm]
    again = Preprocess(engine=B.FakeHvgBatchEngine()).highly_variable_genes(data_of(C, cells, genes), n_top_genes=N_TOP,
                                                                            surface="direct", batch_key="batch", obs=shuffled)
    pd.testing.assert_frame_equal(again, want, check_exact=True)


def test_invariances(case):
    """A permutation of the cells and an order-preserving relabelling of the batches leave the frame as it is: the
    relabelling bit for bit; the permutation changes the order of the float64 clipped sums, so variances_norm moves by
    rounding (bound: 1e-12 relative) and the rest is equal, on the condition -- asserted on the restatement -- that
    unequal variances_norm of a batch differ by more than 1e-9 relatively."""
    C, cells, genes, labels = case
    want, parts = B.seurat_v3_batch(C, labels, N_TOP, genes=genes, parts=True)
    for v in parts["vnorm"]:
        s = np.unique(v)
        assert ((s[1:] - s[:-1]) / s[1:]).min() > 1e-9
    relabelled = np.array([{"A": 3, "B": 10, "C": 200}[x] for x in labels])
    pd.testing.assert_frame_equal(B.seurat_v3_batch(C, relabelled, N_TOP, genes=genes), want, check_exact=True)
    perm = np.random.RandomState(8).permutation(N)
    P = Preprocess(engine=B.FakeHvgBatchEngine())
    for got in (B.seurat_v3_batch(C[perm], labels[perm], N_TOP, genes=genes),
                P.highly_variable_genes(data_of(C[perm], [cells[i] for i in perm], genes), n_top_genes=N_TOP,
                                        batch_key="batch", obs=obs_of([cells[i] for i in perm], labels[perm]))):
        for col in ("means", "variances", "highly_variable_rank", "highly_variable", "highly_variable_nbatches"):
            assert np.array_equal(got[col].values, want[col].values, equal_nan=col == "highly_variable_rank"), col
        assert np.allclose(got["variances_norm"].values, want["variances_norm"].values, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- errors
def test_label_errors_come_before_any_device_work(no_device, case):
    C, cells, genes, labels = case
    P = Preprocess()
    data = data_of(C, cells, genes)
    with pytest.raises(KeyError, match="obs is required for batch_key"):
        P.highly_variable_genes(data, batch_key="batch")
    with pytest.raises(KeyError, match="'lab' is not a column of obs"):
        P.highly_variable_genes(data, batch_key="lab", obs=obs_of(cells, labels))
    for missing in (None, np.nan):
        bad = labels.astype(object)
        bad[7] = missing
        with pytest.raises(ValueError, match="no label"):
            P.highly_variable_genes(data, batch_key="batch", obs=obs_of(cells, bad))
    lone = labels.copy()
    lone[5] = "Z"
    with pytest.raises(ValueError, match="batch 'Z' has 1 cell"):
        P.highly_variable_genes(data, batch_key="batch", obs=obs_of(cells, lone))
    with pytest.raises(ValueError, match="obs has 3 rows"):
        P.highly_variable_genes(data, batch_key="batch", obs=obs_of(cells[:3], labels[:3]))
    many = 2 * (pp.HVG_BATCHES_MAX + 1)
    tall = (sp.csr_matrix((many, 3)), ["c%d" % i for i in range(many)], ["a", "b", "c"])
    with pytest.raises(NotImplementedError, match="batches"):
        P.highly_variable_genes(tall, batch_key="batch", obs=obs_of(tall[1], np.arange(many) // 2))
    # the same rules on the two routes, and the key is never ignored
    hv = np.arange(G) < 20
    for method, top in ((P.normalize_batchcorrect, "n_top_genes"), (P.preprocess_for_cnmf, "n_top_rna_genes")):
        def call(**k):
            return method(data, makeplots=False, **k)
        with pytest.raises(ValueError, match="hvg_batch_key is used only with hvg='device'"):
            call(highly_variable=hv, hvg_batch_key="batch", obs=obs_of(cells, labels))
        with pytest.raises(ValueError, match="hvg_batch_key is used only with hvg='device'"):
            call(highly_variable=hv, hvg="device", hvg_batch_key="batch", obs=obs_of(cells, labels))
        with pytest.raises(ValueError, match="hvg_batch_key is used only with hvg='device'"):
            call(highly_variable=hv, hvg_batch_key="batch", obs=obs_of(cells, labels), **{top: N_TOP})
        with pytest.raises(KeyError, match="obs is required for batch_key"):
            call(hvg="device", hvg_batch_key="batch", **{top: N_TOP})
        with pytest.raises(KeyError, match="is not a column of obs"):
            call(hvg="device", hvg_batch_key="lab", obs=obs_of(cells, labels), **{top: N_TOP})
        with pytest.raises(ValueError, match="batch 'Z' has 1 cell"):
            call(hvg="device", hvg_batch_key="batch", obs=obs_of(cells, lone), **{top: N_TOP})
    assert P._engine is None


def test_count_and_span_errors_arise_per_batch(case):
    C, cells, genes, labels = case
    data, obs = data_of(C, cells, genes), obs_of(cells, labels)
    P = Preprocess(engine=B.FakeHvgBatchEngine())
    for value in (1.5, float(R.COUNT_MAX + 1)):                   # in one cell of one batch
        bad = C.copy()
        bad[int(np.flatnonzero(labels == "B")[0]), 9] = value
        with pytest.raises(ValueError, match="seurat_v3"):
            P.highly_variable_genes(data_of(bad, cells, genes), n_top_genes=N_TOP, batch_key="batch", obs=obs)
    with pytest.raises(ValueError, match="leaves no point"):      # q = floor(n span) = 0 in every batch
        P.highly_variable_genes(data, n_top_genes=N_TOP, span=1e-3, batch_key="batch", obs=obs)
    # batch C: every gene with one count of 1 -- one abscissa for all genes, so a local fit AT it (surface "direct") has
    # h = 0; the other batches, and the data as a whole, fit
    flat = C.copy()
    rows = np.flatnonzero(labels == "C")
    flat[rows] = 0.0
    flat[rows[np.arange(G) % rows.size], np.arange(G)] = 1.0
    with pytest.raises(ValueError, match="zero-width"):
        P.highly_variable_genes(data_of(flat, cells, genes), n_top_genes=N_TOP, surface="direct", batch_key="batch", obs=obs)
    assert len(P.highly_variable_genes(data_of(flat, cells, genes), n_top_genes=N_TOP, surface="direct")) == G
    assert P.engine._pre is None                                  # released on every path


# ---------------------------------------------------------------- the two routes through an engine double
def test_normalize_batchcorrect_selects_per_batch(case):
    C, cells, genes, labels = case
    obs = obs_of(cells, labels, "donor")
    want = B.seurat_v3_batch(C, labels, N_TOP, genes=genes)
    want_hvgs = list(want.index[want["highly_variable"].values])
    assert want_hvgs != list(R.seurat_v3(C, N_TOP, genes=genes).query("highly_variable").index)    # the batches matter
    eng = B.FakeHvgBatchEngine()
    res, hvgs = Preprocess(engine=eng).normalize_batchcorrect(data_of(C, cells, genes), obs=obs, hvg="device", n_top_genes=N_TOP,
                                                              hvg_batch_key="donor", makeplots=False)
    assert hvgs == want_hvgs and len(hvgs) == N_TOP and list(res.var.index) == hvgs
    pd.testing.assert_frame_equal(res.var, want[want["highly_variable"].values], check_exact=True)
    assert list(res.var.columns) == COLUMNS and (res.var["highly_variable_nbatches"] >= 1).all()
    res2, hvgs2 = Preprocess(engine=B.FakeHvgBatchEngine()).normalize_batchcorrect(data_of(C, cells, genes), obs=obs,
                                                                                   highly_variable=want_hvgs, makeplots=False)
    assert hvgs2 == hvgs and F.same_csr(sp.csr_matrix(res.X), sp.csr_matrix(res2.X))


def test_preprocess_for_cnmf_selects_per_batch_after_the_exclusion(case):
    C, cells, genes, labels = case
    obs = obs_of(cells, labels)
    free = B.seurat_v3_batch(C, labels, N_TOP, genes=genes)
    exclude = list(free.index[free["highly_variable"].values][:8]) + ["not_a_gene"]
    keep = ~np.isin(np.array(genes), exclude)
    want = B.seurat_v3_batch(C[:, keep], labels, N_TOP, genes=np.array(genes)[keep])
    eng = B.FakeHvgBatchEngine()
    res, tp, hvgs = Preprocess(engine=eng).preprocess_for_cnmf(data_of(C, cells, genes), obs=obs, hvg="device",
                                                              n_top_rna_genes=N_TOP, hvg_batch_key="batch",
                                                              exclude_genes=exclude, makeplots=False)
    assert hvgs == list(want.index[want["highly_variable"].values]) and not set(hvgs) & set(exclude)
    pd.testing.assert_frame_equal(res.var, want[want["highly_variable"].values], check_exact=True)
    assert eng.calls.index("subset") < eng.calls.index("gene_moments_batched") and "gene_moments" not in eng.calls
    assert list(tp.var_names) == genes and res.X.shape == (N, N_TOP)


# ---------------------------------------------------------------- scanpy itself, where it exists
def test_restatement_against_scanpy(case):
    sc = pytest.importorskip("scanpy")
    pytest.importorskip("skmisc.loess")
    ad = pytest.importorskip("anndata")
    C, cells, genes, labels = case
    adata = ad.AnnData(sp.csr_matrix(C))
    adata.var_names, adata.obs_names = genes, cells
    adata.obs["batch"] = labels
    want = sc.pp.highly_variable_genes(adata, flavor="seurat_v3", n_top_genes=N_TOP, batch_key="batch", inplace=False)
    got = B.seurat_v3_batch(C, labels, N_TOP, genes=genes)
    assert np.allclose(got["means"].values, want["means"].values, rtol=1e-12, atol=0)
    assert np.allclose(got["variances"].values, want["variances"].values, rtol=1e-10, atol=0)
    assert np.allclose(got["variances_norm"].values, want["variances_norm"].values, rtol=1e-7, atol=0)
    assert np.array_equal(got["highly_variable_nbatches"].values, np.asarray(want["highly_variable_nbatches"].values))
    assert np.array_equal(got["highly_variable"].values, np.asarray(want["highly_variable"].values, dtype=bool))
