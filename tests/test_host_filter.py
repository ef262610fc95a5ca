"""Preprocess.filter_adata / preprocess_for_cnmf without a device: the argument and name rules raise before an engine
exists, the new engine methods check their masks before the library is called, and the numpy restatement of the device
entry points (tests/_filter_ref.py), driven through the public methods, reproduces the reference's results
(tests/golden/ref_filter.npz, written by tools/make_golden_filter.py) exactly."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from tests import _filter_ref as F
from cnmf_amd import engine as engine_mod
from cnmf_amd.preprocess import (HVG_REQUIRED_ERROR, Preprocess, dot_genes_mask, make_unique_names, mito_genes_mask)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_filter.npz")


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(engine_mod.Engine, "__init__", refuse)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture
def data():
    rs = np.random.RandomState(0)
    C = rs.poisson(1.0, size=(20, 8)).astype(np.float64)
    A = rs.poisson(5.0, size=(20, 3)).astype(np.float64)
    cells, genes = ["c%d" % i for i in range(20)], ["g%d" % j for j in range(8)]
    return (sp.csr_matrix(C), cells, genes), (sp.csr_matrix(A), cells, ["a0", "a1", "a2"]), np.arange(8) < 5


# ---------------------------------------------------------------- argument rules, no engine
def test_reference_error_texts(no_device, data):
    rna, adt, hv = data
    P = Preprocess()
    with pytest.raises(Exception) as e:
        P.preprocess_for_cnmf([rna, (adt[0][:19], adt[1][:19], adt[2])], highly_variable=hv)
    assert str(e.value) == "ADT and RNA AnnDatas don't have the same number of cells"
    other = ["c%d" % i for i in range(19)] + ["x"]
    with pytest.raises(Exception) as e:
        P.preprocess_for_cnmf([rna, (adt[0], other, adt[2])], highly_variable=hv)
    assert str(e.value) == "Inconsistency of the index for the ADT and RNA AnnDatas"
    for bad in ([rna, adt, adt], [rna], None, "counts.h5ad", (rna, adt)):
        with pytest.raises(Exception) as e:
            P.preprocess_for_cnmf(bad, highly_variable=hv)
        assert str(e.value) == 'data should either be an AnnData object or a list of 2 AnnData objects'
    assert P._engine is None


def test_hvg_rules(no_device, data):
    rna, adt, hv = data
    P = Preprocess()
    with pytest.raises(Exception) as e:
        P.preprocess_for_cnmf(rna)
    assert str(e.value) == HVG_REQUIRED_ERROR
    with pytest.raises(NotImplementedError) as e:
        P.preprocess_for_cnmf(rna, highly_variable=hv, n_top_rna_genes=2000)
    with pytest.raises(NotImplementedError) as e2:
        P.normalize_batchcorrect(rna, highly_variable=hv, n_top_genes=2000)
    assert str(e.value) == str(e2.value)
    with pytest.raises(NotImplementedError):
        P.preprocess_for_cnmf([rna, adt], n_top_rna_genes=5)
    with pytest.raises(ValueError):
        P.preprocess_for_cnmf(rna, highly_variable=hv, quantile_thresh=1.5)
    with pytest.raises(ValueError, match="selects no gene"):
        P.preprocess_for_cnmf(rna, highly_variable=["g1", "g2"], exclude_genes=["g2", "g1"])
    assert P._engine is None


def test_make_unique_names():
    assert list(make_unique_names(["a", "b", "c"])) == ["a", "b", "c"]
    assert list(make_unique_names(["a", "b", "a", "a"])) == ["a", "b", "a-1", "a-2"]
    # an existing name-1 is skipped, whether it comes before or after the duplicate
    assert list(make_unique_names(["a", "a-1", "a", "a"])) == ["a", "a-1", "a-2", "a-3"]
    assert list(make_unique_names(["a", "a", "a-1", "b", "b"])) == ["a", "a-2", "a-1", "b", "b-1"]
    # a made name counts as taken for the names after it
    assert list(make_unique_names(["a", "a", "a-1", "a-1"])) == ["a", "a-2", "a-1", "a-1-1"]
    _, _, genes, _, _, _ = F.make_inputs()
    u = make_unique_names(genes)
    assert u.is_unique and u[51] == "g50-2" and u[52] == "g50-1" and u[53] == "g50-3" and u[50] == "g50"


def test_mito_is_a_substring_test():
    names = ["MT-CO1", "XMT-ND1", "mt-co1", "MT", "AMT", "A.1", "B"]
    assert list(mito_genes_mask(names)) == [True, True, False, False, False, False, False]
    assert list(dot_genes_mask(names)) == [False, False, False, False, False, True, False]


# ---------------------------------------------------------------- the engine checks its masks before the library
class StubLib:
    """every entry point fails the test"""

    def __getattr__(self, name):
        def call(*a, **k):
            raise AssertionError("the library was called: " + name)
        return call


def stub_engine(N=5, G=7):
    eng = engine_mod.Engine.__new__(engine_mod.Engine)
    eng._lib, eng._ctx = StubLib(), None
    eng._pre = {"N": N, "G": G, 0: None, 1: None}
    return eng


@pytest.mark.parametrize("bad", ["short", "long", "ints", "2d"])
def test_mask_errors_raise_before_the_library(bad):
    eng = stub_engine()

    def mask(n):
        return {"short": np.ones(n - 1, dtype=bool), "long": np.ones(n + 1, dtype=bool),
                "ints": np.ones(n, dtype=np.int64), "2d": np.ones((n, 1), dtype=bool)}[bad]
    with pytest.raises(ValueError, match="cell_mask"):
        eng.preprocess_gene_detect(mask(5))
    with pytest.raises(ValueError, match="gene_mask"):
        eng.preprocess_cell_sums(mask(7))
    with pytest.raises(ValueError, match="keep_cells"):
        eng.preprocess_subset(keep_cells=mask(5))
    with pytest.raises(ValueError, match="keep_genes"):
        eng.preprocess_subset(keep_cells=np.ones(5, dtype=bool), keep_genes=mask(7))
    assert eng._pre["N"] == 5 and eng._pre["G"] == 7
    eng._pre = None
    with pytest.raises(RuntimeError, match="preprocess_upload"):
        eng.preprocess_fetch_counts()


# ---------------------------------------------------------------- the restatement against the reference's results
def test_restatement_edge_semantics():
    # row 0 unsorted with a stored zero, row 1 empty, column 3 empty
    X = sp.csr_matrix((np.array([2.0, 0.0, 5.0, 1.0, 4.0]), np.array([4, 0, 1, 2, 0]), np.array([0, 3, 3, 5])), shape=(3, 5))
    n_cells, totals = F.gene_detect(X)
    assert list(n_cells) == [1, 1, 1, 0, 1] and list(totals) == [4.0, 5.0, 1.0, 0.0, 2.0]
    assert list(F.cell_sums(X, np.array([1, 0, 0, 0, 1], dtype=bool))) == [2.0, 0.0, 4.0]
    S = F.subset(X, np.array([1, 0, 1], dtype=bool), np.array([1, 0, 1, 0, 1], dtype=bool))
    assert S.shape == (2, 3) and list(S.indptr) == [0, 2, 4]
    assert list(S.indices) == [2, 0, 1, 0] and list(S.data) == [2.0, 0.0, 1.0, 4.0]


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("run", list(F.FILTER_RUNS))
def test_filter_adata_reproduces_the_reference(gold, run, dense):
    eng = F.FakeFilterEngine()
    P = Preprocess(engine=eng)
    F.check_filter_run(P, gold, run, dense)
    assert eng.calls == ["upload", "subset"]            # one upload, one restriction
    assert eng.X is None                                # released


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("run", ["single", "ftype", "list"])
def test_preprocess_for_cnmf_reproduces_the_reference(gold, run, dense, capsys):
    eng = F.FakeFilterEngine()
    P = Preprocess(engine=eng)
    F.check_pf_run(P, gold, run, dense)
    out = capsys.readouterr().out
    if run == "single":
        assert out == "Excluding 3 genes from cNMF input (retained in tp10k):\n['g7', 'g8', 'IGHV1.2']\n"
        assert eng.calls == ["upload", "subset"]
    else:
        assert out == "" and eng.calls == ["upload", "upload"]       # RNA once, ADT once


def test_exclude_genes_not_found_message(gold, capsys):
    data, kw = F.pf_inputs("single", False)
    kw["exclude_genes"] = ["nothing"]
    eng = F.FakeFilterEngine()
    Preprocess(engine=eng).preprocess_for_cnmf(data, **kw)
    assert capsys.readouterr().out == "exclude_genes provided but none found in adata_RNA.var_names.\n"
    assert eng.calls == ["upload"]


def test_filters_that_leave_nothing_name_the_axis():
    C, cells, genes, _, _, _ = F.make_inputs()
    P = Preprocess(engine=F.FakeFilterEngine())
    with pytest.raises(ValueError, match="no gene"):
        P.filter_adata((sp.csr_matrix(C), cells, genes), min_cells_per_gene=10 ** 6)
    with pytest.raises(ValueError, match="no cell"):
        P.filter_adata((sp.csr_matrix(C), cells, genes), min_counts_per_cell=10 ** 9)
    with pytest.raises(ValueError, match="no cell"):
        P.filter_adata((sp.csr_matrix(C), cells, genes), min_counts_per_cell=None, filter_mito_thresh=0.0)


def test_save_output_base(gold, tmp_path):
    base = str(tmp_path / "out")
    data, kw = F.pf_inputs("single", False)
    res, tp, hvgs = Preprocess(engine=F.FakeFilterEngine()).preprocess_for_cnmf(data, save_output_base=base, **kw)
    assert open(base + ".Corrected.HVGs.txt").read() == "\n".join(hvgs)
    assert F.same_csr(sp.load_npz(base + ".TP10K.npz"), sp.csr_matrix(tp.X))
    assert open(base + ".TP10K.genes.txt").read().split("\n") == list(tp.var_names)
    assert open(base + ".Corrected.HVG.Varnorm.cells.txt").read().split("\n") == list(res.obs_names)
    data, kw = F.pf_inputs("single", True)
    res, tp, hvgs = Preprocess(engine=F.FakeFilterEngine()).preprocess_for_cnmf(data, save_output_base=base, **kw)
    z = np.load(base + ".TP10K.df.npz", allow_pickle=True)
    assert np.array_equal(z["data"], tp.X) and list(z["columns"]) == list(tp.var_names)
