"""The seurat_v3 HVG selection without a device: the numpy restatement (tests/_seurat_v3_ref.py, the yardstick of
Preprocess.highly_variable_genes) against what can be known in closed form, the host half of the product route
(vertices, Hermite blend, ranking) against the restatement, the argument rules, and the plumbing of ``hvg="device"``
through an engine double whose three device methods are played by the restatement.  The comparisons with skmisc's
loess and with scanpy run wherever those libraries can be imported; they are not installed on this project's machines."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import engine as engine_mod
from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import HVG_REQUIRED_ERROR, N_TOP_GENES_ERROR, Preprocess
from tests import _filter_ref as F
from tests import _seurat_v3_ref as R

SHAPES = [(300, 600, 1), (257, 1000, 2)]                # (cells, genes, seed): the shapes of test_gpu_hvg.py


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(engine_mod.Engine, "__init__", refuse)


@pytest.fixture(scope="module")
def loess_inputs():
    """per shape: the sorted (x, y) = log10 (mean, variance) of the non-constant genes"""
    out = []
    for N, G, seed in SHAPES:
        C = R.gamma_poisson_counts(N, G, seed)
        s1, s2, flags = R.gene_moments(C)
        assert flags == 0
        mean, var = R.mean_var(s1, s2, N)
        nc = var > 0
        x, y = np.log10(mean[nc]), np.log10(var[nc])
        order = np.argsort(x, kind="stable")
        out.append((x[order], y[order]))
    return out


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("surface", ["interpolate", "direct"])
def test_the_restatement_reproduces_an_exact_quadratic(surface):
    """A local quadratic fit of a quadratic is the quadratic, and the Hermite cubic through exact values and slopes of
    a quadratic is the quadratic as well: both surfaces within 1e-12 (measured: below 1e-14)."""
    rs = np.random.RandomState(7)
    x = np.sort(rs.uniform(-2.0, 3.0, size=400) ** 3 / 9.0)
    y = 0.7 - 1.3 * x + 0.45 * x * x
    fitted = R.loess_fitted(x, y, span=0.3, surface=surface)
    err = np.abs(fitted - y).max()
    print("exact quadratic, %s: max error %.3e" % (surface, err))
    assert err < 1e-12
    perm = rs.permutation(x.size)                        # the points in any order
    assert np.array_equal(R.loess_fitted(x[perm], y[perm], surface=surface), fitted[perm])


def test_moments_are_the_ddof1_variance_exactly():
    C = R.gamma_poisson_counts(120, 90, 5)
    s1, s2, flags = R.gene_moments(sp.csr_matrix(C))
    assert flags == 0 and np.array_equal(s1, C.sum(axis=0)) and np.array_equal(s2, (C * C).sum(axis=0))
    mean, var = R.mean_var(s1, s2, 120)
    ld = C.astype(np.longdouble)
    want = ((ld - ld.mean(axis=0)) ** 2).sum(axis=0) / 119
    assert np.array_equal(mean, C.sum(axis=0) / 120)
    assert np.abs(var - want.astype(np.float64)).max() <= 4 * R.EPS * var.max()
    mean_ld, var_ld = R.mean_var(s1, s2, 120, np.longdouble)
    assert np.array_equal(var_ld.astype(np.float64), var) and np.array_equal(mean_ld.astype(np.float64), mean)
    bad = C.copy()
    bad[3, 7] = 1.5
    assert R.gene_moments(bad)[2] == R.FLAG_NOT_COUNT
    bad[3, 7] = R.COUNT_MAX + 1.0
    assert R.gene_moments(bad)[2] == R.FLAG_TOO_LARGE
    with pytest.raises(ValueError, match="seurat_v3"):
        R.seurat_v3(bad, 10)


def test_ties_rank_one_zero_width_and_rank_two():
    """Ten copies each of the abscissae 0..4.  q = 15 at 2.0: h = 1 and only the ten points at 2.0 weigh (t = 0, rank
    one): the minimum-norm solution is their mean with slope 0.  q = 8 at 2.0: h = 0, the zero-width ValueError.
    q = 25 at 1.5: h = 1.5, the points at 1 and 2 weigh equally at t = -1/3 and +1/3 (rank two: the columns 1 and t^2 are
    proportional): the slope is the one of the line through the two means, and the minimum-norm split of their mid-value
    m between c0 and c2 gives c0 = m / (1 + a^4), a = 1/3."""
    x, y = R.tie_case()
    for dtype in (np.float64, np.longdouble):
        value, slope = R.local_fit(x, y, 2.0, 15, dtype)
        assert abs(float(value) - y[x == 2].mean()) < 1e-14 and abs(float(slope)) < 1e-14
        with pytest.raises(ValueError, match="zero-width"):
            R.local_fit(x, y, 2.0, 8, dtype)
        value, slope = R.local_fit(x, y, 1.5, 25, dtype)
        m1, m2 = y[x == 1].mean(), y[x == 2].mean()
        assert np.isfinite(float(value)) and abs(float(slope) - (m2 - m1)) < 1e-13
        assert abs(float(value) - 0.5 * (m1 + m2) / (1 + 3.0 ** -4)) < 1e-13
    assert pp.loess_local_fit_host(x, y, 2.0, 15) == R.local_fit(x, y, 2.0, 15)
    with pytest.raises(ValueError, match="zero-width"):
        pp.loess_local_fit_host(x, y, 2.0, 8)


def test_the_long_double_solver_agrees_with_lstsq(loess_inputs):
    """the restatement's long double run uses its own one-sided Jacobi SVD: on well-posed fits it agrees with lstsq to
    float64 rounding (this distance is the base of the GPU tests' tolerance)"""
    xs, ys = loess_inputs[0]
    v, _ = R.loess_vertices(xs, 0.3)
    q = R.loess_q(xs.size, 0.3)
    a, b = R.local_fits(xs, ys, v, q), R.local_fits(xs, ys, v, q, np.longdouble)
    for k in (0, 1):
        d = float(np.abs(a[k] - b[k]).max())
        assert 0 < d < 1e-12, d


def test_vertices(loess_inputs):
    """The vertices are sorted and strictly increasing, enclose the data, and every cell holds at most fc points (there
    are no ties long enough to forbid a cut in this data; with the tie case they do).  The two surfaces agree at the data
    points only approximately -- measured here: max |interpolate - direct| = 1.58e-2 in log10 variance at 300 x 600 (598
    points, 32 vertices) and 1.56e-2 at 257 x 1000 (997 points, 31 vertices); the bound asserted, 5e-2, only says that
    the two are the same curve."""
    for (N, G, _), (xs, ys) in zip(SHAPES, loess_inputs):
        v, fc = R.loess_vertices(xs, 0.3)
        assert fc == int(np.floor(xs.size * 0.3 * 0.2))
        assert (np.diff(v) > 0).all() and v[0] < xs[0] and v[-1] > xs[-1]
        per_cell = np.bincount(np.searchsorted(v, xs, side="right") - 1, minlength=v.size - 1)
        assert per_cell.sum() == xs.size and per_cell.max() <= fc, (per_cell.max(), fc)
        assert np.array_equal(pp.loess_vertices(xs, 0.3), v)                   # the product's host half
        a = R.loess_fitted(xs, ys, 0.3, "interpolate")
        b = R.loess_fitted(xs, ys, 0.3, "direct")
        d = np.abs(a - b).max()
        print("%d x %d: %d points, %d vertices, max |interpolate - direct| = %.3e" % (N, G, xs.size, v.size, d))
        assert 0 < d < 5e-2
    x, _ = R.tie_case()
    v, fc = R.loess_vertices(x, 0.3)                     # fc = 3 < ten tied points: cuts only between distinct values
    assert fc == 3 and (np.diff(v) > 0).all()
    assert set(v[1:-1]) <= {0.5, 1.5, 2.5, 3.5}
    one = np.full(20, 1.25)
    assert R.loess_vertices(one, 0.3)[0].size == 2       # no cut at all


def test_the_product_host_half_equals_the_restatement(loess_inputs):
    """with the engine double (local fits by the restatement) the product's loess and frame are the restatement's, bit
    for bit, on both surfaces -- so on the GPU any difference comes from the three device entry points"""
    eng = R.FakeHvgEngine()
    xs, ys = loess_inputs[0]
    perm = np.random.RandomState(3).permutation(xs.size)
    for surface in ("interpolate", "direct"):
        assert np.array_equal(pp.loess_fitted(eng, xs[perm], ys[perm], 0.3, surface),
                              R.loess_fitted(xs[perm], ys[perm], 0.3, surface))
    N, G, seed = SHAPES[0]
    C = R.gamma_poisson_counts(N, G, seed)
    genes = ["g%d" % j for j in range(G)]
    P = Preprocess(engine=eng)
    for surface in ("interpolate", "direct"):
        got = P.highly_variable_genes((sp.csr_matrix(C), ["c%d" % i for i in range(N)], genes), n_top_genes=120,
                                      surface=surface)
        want = R.seurat_v3(C, 120, surface=surface, genes=genes)
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        assert list(got.columns) == ["means", "variances", "variances_norm", "highly_variable_rank", "highly_variable"]
        assert got["highly_variable"].sum() == 120 and got["highly_variable_rank"].notna().sum() == 120
        assert sorted(got["highly_variable_rank"].dropna()) == list(range(120))
        assert (got["variances_norm"].values[:2] == 0).all()                   # the all-zero genes
    assert eng._pre is None                                                    # released


def test_ranking_breaks_ties_in_gene_order():
    vn = np.array([1.0, 3.0, 3.0, 0.5, 3.0])
    f = R.rank_frame(vn, vn, vn, 2, ["a", "b", "c", "d", "e"])
    assert list(f["highly_variable"]) == [False, True, True, False, False]
    assert list(f["highly_variable_rank"][["b", "c"]]) == [0.0, 1.0] and np.isnan(f["highly_variable_rank"]["e"])


# ---------------------------------------------------------------- argument rules: before any device call
@pytest.fixture
def small():
    rs = np.random.RandomState(0)
    C = rs.poisson(1.0, size=(20, 8)).astype(np.float64)
    cells, genes = ["c%d" % i for i in range(20)], ["g%d" % j for j in range(8)]
    return (sp.csr_matrix(C), cells, genes), np.arange(8) < 5


def test_argument_rules(no_device, small):
    counts, hv = small
    P = Preprocess()
    for call in (lambda **k: P.normalize_batchcorrect(counts, highly_variable=hv, n_top_genes=5, **k),
                 lambda **k: P.preprocess_for_cnmf(counts, highly_variable=hv, n_top_rna_genes=5, **k)):
        with pytest.raises(ValueError, match="hvg must be"):
            call(hvg="host")
        with pytest.raises(ValueError, match="hvg must be"):
            call(hvg="scanpy")
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == N_TOP_GENES_ERROR and "hvg='device'" in N_TOP_GENES_ERROR
    with pytest.raises(Exception) as e:
        P.normalize_batchcorrect(counts, hvg="device")
    assert str(e.value) == HVG_REQUIRED_ERROR and "you must include a highly_variable column" in str(e.value)
    with pytest.raises(Exception) as e:
        P.preprocess_for_cnmf(counts, hvg="device", n_top_rna_genes=None)
    assert str(e.value) == HVG_REQUIRED_ERROR
    with pytest.raises(ValueError, match="n_top_genes"):
        P.normalize_batchcorrect(counts, hvg="device", n_top_genes=0)
    with pytest.raises(NotImplementedError, match="flavor"):
        P.highly_variable_genes(counts, flavor="seurat")
    with pytest.raises(NotImplementedError, match="flavor"):
        P.highly_variable_genes(counts, flavor="cell_ranger")
    with pytest.raises(ValueError, match="surface"):
        P.highly_variable_genes(counts, surface="exact")
    with pytest.raises(ValueError, match="span"):
        P.highly_variable_genes(counts, span=0.0)
    with pytest.raises(ValueError, match="seurat_v3"):
        P.highly_variable_genes((-counts[0], counts[1], counts[2]))
    assert P._engine is None


# ---------------------------------------------------------------- plumbing through an engine double
def test_preprocess_for_cnmf_selects_after_the_exclusion_and_among_rna_only():
    C, cells, genes, A, adt_names, _ = F.make_inputs()
    ftype = np.array(["Gene Expression"] * len(genes) + [F.ADT_NAME] * len(adt_names))
    data = (sp.csr_matrix(np.hstack([C, A])), cells, list(genes) + list(adt_names))
    # the genes the selection would rank first when nothing is excluded: exclude ten of them
    free = R.seurat_v3(C, 50, genes=genes)
    top = list(free.index[free["highly_variable"].values][:10])
    exclude = top + ["not_a_gene"]
    eng = R.FakeHvgEngine()
    res, tp, hvgs = Preprocess(engine=eng).preprocess_for_cnmf(data, hvg="device", n_top_rna_genes=50, exclude_genes=exclude,
                                                              feature_type=ftype, adt_feature_name=F.ADT_NAME,
                                                              makeplots=False)
    assert len(hvgs) == 50 and not set(hvgs) & set(exclude) and not set(hvgs) & set(adt_names)
    order = {g: j for j, g in enumerate(genes)}
    pos = [order[g] for g in hvgs]
    assert pos == sorted(pos) and list(res.var_names) == hvgs                   # the data's gene order
    assert res.X.shape == (len(cells), 50)
    assert list(tp.var_names) == list(genes) + list(adt_names)                  # tp10k over ALL genes, ADT appended
    # the selection ran once, on the staging after the subset
    assert eng.calls.index("subset") < eng.calls.index("gene_moments") and eng.calls.count("gene_moments") == 1
    keep = ~np.isin(np.array(genes), exclude)
    want = R.seurat_v3(C[:, keep], 50, genes=np.array(genes)[keep])
    assert hvgs == list(want.index[want["highly_variable"].values])
    pd.testing.assert_frame_equal(res.var, want[want["highly_variable"].values], check_exact=True)
    # the same counts through the mask route: nothing downstream moved
    res2, tp2, hvgs2 = Preprocess(engine=R.FakeHvgEngine()).preprocess_for_cnmf(
        data, highly_variable=hvgs, exclude_genes=exclude, feature_type=ftype, adt_feature_name=F.ADT_NAME, makeplots=False)
    assert hvgs2 == hvgs and F.same_csr(sp.csr_matrix(res.X), sp.csr_matrix(res2.X))
    assert F.same_csr(sp.csr_matrix(tp.X), sp.csr_matrix(tp2.X))


def test_normalize_batchcorrect_computed_selection_wins():
    N, G, seed = 120, 200, 9
    C = R.gamma_poisson_counts(N, G, seed)
    cells, genes = ["c%d" % i for i in range(N)], ["g%d" % j for j in range(G)]
    given = np.arange(G) < 30
    want = R.seurat_v3(C, 40, genes=genes)
    res, hvgs = Preprocess(engine=R.FakeHvgEngine()).normalize_batchcorrect((sp.csr_matrix(C), cells, genes),
                                                                            highly_variable=given, n_top_genes=40,
                                                                            hvg="device", makeplots=False)
    assert hvgs == list(want.index[want["highly_variable"].values]) and len(hvgs) == 40
    assert list(res.var.index) == hvgs and res.var["highly_variable"].all()
    # hvg="device" without a number changes nothing: the mask is used
    res2, hvgs2 = Preprocess(engine=R.FakeHvgEngine()).normalize_batchcorrect((sp.csr_matrix(C), cells, genes),
                                                                              highly_variable=given, hvg="device",
                                                                              makeplots=False)
    assert hvgs2 == genes[:30] and res2.var is None


# ---------------------------------------------------------------- the libraries themselves, where they exist
@pytest.mark.parametrize("surface", ["interpolate", "direct"])
def test_restatement_against_skmisc(loess_inputs, surface):
    loess = pytest.importorskip("skmisc.loess")
    for xs, ys in loess_inputs:
        model = loess.loess(xs, ys, span=0.3, degree=2, surface=surface)
        model.fit()
        got = R.loess_fitted(xs, ys, 0.3, surface)
        d = np.abs(got - model.outputs.fitted_values).max()
        print("restatement vs skmisc, %s: %.3e" % (surface, d))
        assert d < 1e-9


def test_restatement_against_scanpy():
    sc = pytest.importorskip("scanpy")
    pytest.importorskip("skmisc.loess")
    ad = pytest.importorskip("anndata")
    for N, G, seed in SHAPES:
        C = R.gamma_poisson_counts(N, G, seed)
        genes = ["g%d" % j for j in range(G)]
        adata = ad.AnnData(sp.csr_matrix(C))
        adata.var_names = genes
        want = sc.pp.highly_variable_genes(adata, flavor="seurat_v3", n_top_genes=120, inplace=False)
        got = R.seurat_v3(C, 120, genes=genes)
        assert np.allclose(got["means"].values, want["means"].values, rtol=1e-12, atol=0)
        assert np.allclose(got["variances"].values, want["variances"].values, rtol=1e-10, atol=0)
        assert np.allclose(got["variances_norm"].values, want["variances_norm"].values, rtol=1e-7, atol=0)
        assert np.array_equal(got["highly_variable"].values, np.asarray(want["highly_variable"].values, dtype=bool))
