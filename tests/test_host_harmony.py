"""Preprocess.run_harmony and the ``harmony=`` keyword without a device: argument errors, limits, the defaults harmonypy
computes (nclust, theta / lamb per level, the level order of pd.get_dummies), and the numpy restatement the GPU tests are
held to (tests/_harmony_ref.py) -- against harmonypy itself where the library is importable."""
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import engine as engine_mod
from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import HARMONY_IMPORT_ERROR, Preprocess
from tests import _harmony_ref as ref


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(engine_mod.Engine, "__init__", refuse)


@pytest.fixture
def data():
    rs = np.random.RandomState(0)
    C = rs.poisson(1.0, size=(20, 8)).astype(np.float64)
    cells, genes = ["c%d" % i for i in range(20)], ["g%d" % j for j in range(8)]
    obs = pd.DataFrame({"batch": ["a", "b"] * 10, "donor": ["x"] * 5 + ["y"] * 10 + ["z"] * 5}, index=cells)
    return (sp.csr_matrix(C), cells, genes), obs, np.arange(8) < 5


def test_harmony_keyword_values(monkeypatch, no_device, data):
    counts, obs, hv = data
    P = Preprocess()
    for call in (lambda **k: P.normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["batch"], **k),
                 lambda **k: P.preprocess_for_cnmf(counts, obs=obs, highly_variable=hv, harmony_vars=["batch"], **k),
                 lambda **k: P.harmony_correct_X(counts[0], obs, np.zeros((20, 3)), ["batch"], **k)):
        with pytest.raises(ValueError, match="harmony must be one of"):
            call(harmony="gpu")
        with pytest.raises(ValueError, match="harmony must be one of"):
            call(harmony=None)
    # a bad value is refused even when harmony_res is given or Harmony is not asked for
    with pytest.raises(ValueError, match="harmony must be one of"):
        P.normalize_batchcorrect(counts, highly_variable=hv, harmony="x")


def test_default_route_still_raises_the_import_error_first(monkeypatch, no_device, data):
    monkeypatch.setitem(sys.modules, "harmonypy", None)
    counts, obs, hv = data
    P = Preprocess()
    for kw in ({}, {"harmony": "harmonypy"}):
        with pytest.raises(ImportError) as e:
            P.normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["nope"], **kw)   # (before the KeyError)
        assert str(e.value) == HARMONY_IMPORT_ERROR
        with pytest.raises(ImportError) as e:
            P.preprocess_for_cnmf(counts, obs=obs, highly_variable=hv, harmony_vars=["batch"], **kw)
        assert str(e.value) == HARMONY_IMPORT_ERROR
        with pytest.raises(ImportError) as e:
            P.harmony_correct_X(counts[0], obs, np.zeros((20, 3)), ["batch"], **kw)
        assert str(e.value) == HARMONY_IMPORT_ERROR
    assert P._engine is None


def test_device_route_does_not_ask_for_harmonypy(monkeypatch, no_device, data):
    """with harmony="device" a missing harmonypy is no error: the call gets as far as its own argument checks"""
    monkeypatch.setitem(sys.modules, "harmonypy", None)
    counts, obs, hv = data
    with pytest.raises(KeyError, match="donor2"):
        Preprocess().normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["donor2"], harmony="device")
    with pytest.raises(KeyError, match="donor2"):
        Preprocess().harmony_correct_X(counts[0], obs, np.zeros((20, 3)), ["donor2"], harmony="device")


def test_run_harmony_argument_errors(no_device, data):
    _, obs, _ = data
    P = Preprocess()
    pca = np.random.RandomState(0).randn(20, 3)
    with pytest.raises(KeyError):
        P.run_harmony(pca, obs, ["nope"])
    with pytest.raises(KeyError):
        P.run_harmony(pca, None, ["batch"])
    with pytest.raises(ValueError, match="cells x components"):
        P.run_harmony(pca[:, 0], obs, ["batch"])
    with pytest.raises(ValueError, match="rows for"):
        P.run_harmony(pca[:10], obs, ["batch"])
    with pytest.raises(ValueError, match="non-finite"):
        P.run_harmony(np.where(np.arange(60).reshape(20, 3) == 7, np.nan, pca), obs, ["batch"])
    with pytest.raises(ValueError, match="sigma"):
        P.run_harmony(pca, obs, ["batch"], sigma=0.0)
    with pytest.raises(ValueError, match="sigma"):
        P.run_harmony(pca, obs, ["batch"], sigma=[0.1, 0.1])
    with pytest.raises(ValueError, match="block_size"):
        P.run_harmony(pca, obs, ["batch"], block_size=0)
    with pytest.raises(ValueError, match="nclust"):
        P.run_harmony(pca, obs, ["batch"], nclust=0)
    with pytest.raises(ValueError, match="init_centroids"):
        P.run_harmony(pca, obs, ["batch"], nclust=2, init_centroids=np.ones((2, 3)))
    with pytest.raises(ValueError, match="theta"):
        P.run_harmony(pca, obs, ["batch", "donor"], theta=[1, 2, 3])
    with pytest.raises(ValueError, match="not categorical"):
        P.run_harmony(pca, obs.assign(depth=np.arange(20.0)), ["depth"])
    assert P._engine is None


def test_run_harmony_limits(no_device, data):
    _, obs, _ = data
    P = Preprocess()
    rs = np.random.RandomState(0)
    big = pd.DataFrame({"batch": ["l%d" % (i % 40) for i in range(200)]})
    with pytest.raises(NotImplementedError, match="K = 129"):
        P.run_harmony(rs.randn(200, 3), big, ["batch"], nclust=129)
    with pytest.raises(NotImplementedError, match="d = 65"):
        P.run_harmony(rs.randn(20, 65), obs, ["batch"], nclust=2)
    with pytest.raises(NotImplementedError, match=r"K \* \(B \+ 1\) = 4100"):
        P.run_harmony(rs.randn(200, 3), big, ["batch"], nclust=100)      # 100 x 41
    assert P._engine is None


def test_nclust_rounds_half_to_even():
    assert pp.harmony_nclust(75) == 2 and pp.harmony_nclust(45) == 2        # 2.5 -> 2, 1.5 -> 2
    assert pp.harmony_nclust(105) == 4 and pp.harmony_nclust(3000) == 100 and pp.harmony_nclust(10 ** 6) == 100


def test_theta_and_lamb_expand_over_two_variables(data):
    _, obs, _ = data
    _, _, _, n_levels = pp.harmony_design(obs, ["batch", "donor"])
    assert n_levels == [2, 3]
    assert pp.harmony_per_level(2, n_levels, "theta").tolist() == [2.0] * 5
    assert pp.harmony_per_level([1, 3], n_levels, "theta").tolist() == [1.0, 1.0, 3.0, 3.0, 3.0]
    assert pp.harmony_per_level([1, 2, 3, 4, 5], n_levels, "lamb").tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert ref.per_level([1, 3], n_levels).tolist() == [1.0, 1.0, 3.0, 3.0, 3.0]


def test_level_order_is_get_dummies(data):
    _, obs, _ = data
    obs = obs.assign(donor=pd.Categorical(obs["donor"], categories=["z", "x", "y"]))     # not the sorted order
    Phi, codes, level_var, n_levels = pp.harmony_design(obs, ["donor", "batch"])
    dummies = pd.get_dummies(obs[["donor", "batch"]])
    assert list(dummies.columns) == ["donor_z", "donor_x", "donor_y", "batch_a", "batch_b"]
    assert np.array_equal(Phi, dummies.to_numpy().T.astype(np.float64))
    assert level_var.tolist() == [0, 0, 0, 1, 1] and codes.dtype == np.int32 and codes.shape == (2, 20)
    onehot = np.zeros_like(Phi)
    for v in range(2):
        onehot[codes[v], np.arange(20)] = 1
    assert np.array_equal(onehot, Phi)
    assert np.array_equal(ref.design(obs, ["donor", "batch"])[0], Phi)
    # a single variable given as a string
    assert np.array_equal(pp.harmony_design(obs, "batch")[0], pd.get_dummies(obs[["batch"]]).to_numpy().T.astype(float))


# ---------------------------------------------------------------- the restatement itself
def test_restatement_invariants():
    pca, obs = ref.make_case(257, 7, [3, 2], seed=10)
    h = ref.run_harmony(pca, obs, ["var0", "var1"], random_state=0)
    assert h.K == 9 and h.R.shape == (9, 257) and h.Z_corr.shape == (7, 257) and h.Y.shape == (7, 9)
    assert np.allclose(h.R.sum(axis=0), 1.0, rtol=0, atol=1e-12) and (h.R >= 0).all()
    assert np.allclose(np.sqrt((h.Y ** 2).sum(axis=0)), 1.0, rtol=0, atol=1e-12)
    # E and O are what their definitions give for the final R (the block updates keep them consistent)
    assert np.allclose(h.E, np.outer(h.R.sum(axis=1), h.Pr_b), rtol=0, atol=1e-10)
    assert np.allclose(h.O, h.R @ h.Phi.T, rtol=0, atol=1e-10)
    assert len(h.objective_harmony) == len(h.kmeans_rounds) + 1
    assert len(h.objective_kmeans) == 1 + sum(r + 1 for r in h.kmeans_rounds)
    assert h.lamb.shape == (6, 6) and h.lamb[0, 0] == 0 and np.array_equal(np.diag(h.lamb)[1:], np.ones(5))
    # the same call again: the same bits (the global RandomState is seeded inside)
    h2 = ref.run_harmony(pca, obs, ["var0", "var1"], random_state=0)
    assert np.array_equal(h.R, h2.R) and h.objective_kmeans == h2.objective_kmeans


def test_restatement_long_double_agrees():
    pca, obs = ref.make_case(19, 3, [2], seed=10)
    h = ref.run_harmony(pca, obs, ["var0"], random_state=0)
    hl = ref.run_harmony(pca, obs, ["var0"], random_state=0, dtype=np.longdouble)
    assert h.K == 1 and hl.R.dtype == np.longdouble and h.kmeans_rounds == hl.kmeans_rounds
    assert np.max(np.abs(h.Z_corr - hl.Z_corr)) < 1e-12


def test_gpu_cases_are_not_decided_by_rounding():
    """every case of tests/test_gpu_harmony.py keeps its convergence ratios 1e-3 (relative) away from the thresholds"""
    from tests import test_gpu_harmony as g
    for name in g.CASES:
        pca, obs, hvars, kw = g.case_inputs(name)
        h = ref.run_harmony(pca, obs, hvars, **kw)
        assert ref.threshold_margin(h) >= 1e-3, name


@pytest.mark.parametrize("shape", [(600, 10, [3], 12, 2), (257, 7, [3, 2], 10, 0)], ids=["a", "b"])
def test_restatement_against_harmonypy(shape):
    """where the library is installed: R, Z_corr and the histories of its run_harmony (it is not installed on the
    project's machines: no agreement with it is claimed there)"""
    harmonypy = pytest.importorskip("harmonypy")
    N, d, levels, seed, random_state = shape
    pca, obs = ref.make_case(N, d, levels, seed=seed)
    obs = obs.astype(str)
    hvars = list(obs.columns)
    ho = harmonypy.run_harmony(pca, obs, hvars, max_iter_harmony=20, random_state=random_state)
    if not hasattr(ho, "objective_kmeans") or np.shape(ho.R) != (ho.K, N):
        pytest.skip("this harmonypy does not have the numpy layout the restatement mirrors")
    h = ref.run_harmony(pca, obs, hvars, random_state=random_state)
    assert list(ho.kmeans_rounds) == h.kmeans_rounds
    assert np.allclose(ho.objective_kmeans, h.objective_kmeans, rtol=1e-9, atol=0)
    assert np.allclose(ho.objective_harmony, h.objective_harmony, rtol=1e-9, atol=0)
    assert np.allclose(ho.R, h.R, rtol=0, atol=1e-9)
    assert np.allclose(ho.Z_corr, h.Z_corr, rtol=0, atol=1e-9)
