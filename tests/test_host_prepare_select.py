"""cNMF.prepare's host half, no GPU: the over-dispersion model (select_highvar_genes) fed with the reference's own TPM
statistics returns the reference's gene lists exactly, and the input loaders (tests/golden/ref_prepare_sparse.npz from
tools/make_golden_prepare.py, ref_small.npz from tools/make_golden.py)."""
import os

import numpy as np
import pandas as pd
import pytest

from cnmf_amd.cnmf import counts_to_csr, read_counts_file, save_df_to_npz, select_highvar_genes

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def prep():
    return dict(np.load(os.path.join(GOLD, "ref_prepare_sparse.npz"), allow_pickle=False))


@pytest.mark.parametrize("tag, numgenes", [("top", 500), ("thr", None)])
def test_highvar_genes_match_reference(prep, tag, numgenes):
    st = prep[tag + "_tpm_stats"]
    genes = np.array(["g%d" % j for j in range(int(prep["shape"][1]))])
    mask, params = select_highvar_genes(st[:, 0], st[:, 1] ** 2, numgenes=numgenes)
    assert list(genes[mask]) == list(prep[tag + "_genes"])            # input gene order (a boolean mask)
    assert (params["T"] is None) == (numgenes is not None)


def test_top_route_on_dense_branch_statistics():
    g = np.load(os.path.join(GOLD, "ref_small.npz"), allow_pickle=False)
    st = g["tpm_stats"]
    mask, _ = select_highvar_genes(st[:, 0], st[:, 1] ** 2, numgenes=150)
    assert list(g["tpm_genes"][mask]) == list(g["genes"])


def test_zero_mean_genes_never_selected():
    rs = np.random.RandomState(0)
    mean = rs.gamma(1.0, 1.0, 200)
    var = mean * rs.gamma(2.0, 1.0, 200)
    mean[:5] = var[:5] = 0.0                                           # fano = 0 / 0
    mask, p = select_highvar_genes(mean, var, numgenes=195)
    assert mask.sum() == 195 and not mask[:5].any() and np.isnan(p["fano_ratio"][:5]).all()
    mask, _ = select_highvar_genes(mean, var, numgenes=None)
    assert not mask[:5].any()


def test_npz_and_text_loaders_agree(tmp_path):
    rs = np.random.RandomState(1)
    df = pd.DataFrame(rs.poisson(0.5, (20, 7)).astype(np.int64), index=["c%d" % i for i in range(20)],
                      columns=["g%d" % j for j in range(7)])
    save_df_to_npz(df, str(tmp_path / "x.df.npz"))
    df.to_csv(str(tmp_path / "x.txt"), sep="\t")
    a, b = read_counts_file(str(tmp_path / "x.df.npz")), read_counts_file(str(tmp_path / "x.txt"))
    pd.testing.assert_frame_equal(a, b)
    pd.testing.assert_frame_equal(a, df)
    m, cells, genes = counts_to_csr(str(tmp_path / "x.txt"))
    assert np.array_equal(m.toarray(), df.values) and list(cells) == list(df.index) and list(genes) == list(df.columns)
    m2, c2, g2 = counts_to_csr(df.values, like=(m, cells, genes))       # a bare array takes the names of `like`
    assert list(c2) == list(cells) and list(g2) == list(genes)


@pytest.mark.parametrize("name", ["x.h5ad", "matrix.mtx", "matrix.mtx.gz"])
def test_unreadable_formats_name_the_in_memory_route(name):
    with pytest.raises(NotImplementedError, match="in memory"):
        read_counts_file(name)
