"""Preprocess's argument errors raise before any device call (no GPU needed), and the ceiling's interpolation between
two order statistics gives np.quantile's bits."""
import sys
import types

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import engine as engine_mod
from cnmf_amd.preprocess import HARMONY_IMPORT_ERROR, Preprocess, quantile_from_order_stats


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
    obs = pd.DataFrame({"batch": ["a", "b"] * 10}, index=cells)
    return (sp.csr_matrix(C), cells, genes), obs, np.arange(8) < 5


def test_missing_harmonypy_raises_the_reference_text(monkeypatch, no_device, data):
    monkeypatch.setitem(sys.modules, "harmonypy", None)          # import harmonypy -> ImportError
    counts, obs, hv = data
    P = Preprocess()
    with pytest.raises(ImportError) as e:
        P.harmony_correct_X(counts[0], obs, np.zeros((20, 3)), ["batch"])
    assert str(e.value) == HARMONY_IMPORT_ERROR
    assert str(e.value) == ("harmonypy is not installed. Please install it using 'pip install harmonypy' before "
                            "proceeding.")
    with pytest.raises(ImportError) as e:
        P.normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["batch"], makeplots=False)
    assert str(e.value) == HARMONY_IMPORT_ERROR
    assert P._engine is None


def test_n_top_genes_is_not_implemented(no_device, data):
    counts, obs, hv = data
    with pytest.raises(NotImplementedError):
        Preprocess().normalize_batchcorrect(counts, obs=obs, highly_variable=hv, n_top_genes=2000)
    with pytest.raises(NotImplementedError):
        Preprocess().normalize_batchcorrect(counts, n_top_genes=5)


def test_missing_highly_variable_raises_the_reference_text(no_device, data):
    counts, obs, _ = data
    with pytest.raises(Exception, match="you must include a highly_variable column"):
        Preprocess().normalize_batchcorrect(counts, obs=obs)


def test_missing_harmony_var_raises_key_error(monkeypatch, no_device, data):
    fake = types.ModuleType("harmonypy")
    fake.run_harmony = lambda *a, **k: pytest.fail("run_harmony reached")
    monkeypatch.setitem(sys.modules, "harmonypy", fake)
    counts, obs, hv = data
    with pytest.raises(KeyError):
        Preprocess().normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["donor"])
    with pytest.raises(KeyError):
        Preprocess().normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars="donor")
    with pytest.raises(KeyError):
        Preprocess().harmony_correct_X(counts[0], obs, np.zeros((20, 3)), ["batch", "donor"])


def test_random_seed_is_set(no_device):
    Preprocess(random_seed=12)
    a = np.random.rand()
    np.random.seed(12)
    assert a == np.random.rand()


@pytest.mark.parametrize("n,q", [(1000, .9999), (1000, .99), (30000, .9999), (12345, .5), (7, 1.0), (7, 0.0),
                                 (99991, 0.123456789)])
def test_interpolation_between_order_statistics_is_np_quantile(n, q):
    rs = np.random.RandomState(n)
    v = rs.gamma(0.7, 3.0, size=n)
    v[rs.rand(n) < 0.4] = 0.0
    h = (n - 1) * q
    k = int(np.floor(h))
    s = np.sort(v)
    lo, hi = s[k], s[min(k + 1, n - 1)]
    assert quantile_from_order_stats(lo, hi, n, q) == np.quantile(v, q)
