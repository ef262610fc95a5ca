"""The k-means initialisation of run_harmony without a device: the ``kmeans_init`` keyword and the "device_full" mode, the
uniform stream handed to the device, the C ABI entry, and the inputs of tests/test_gpu_harmony_init.py -- on each of them
the numpy restatement of KMeans (oracle/consensus.py) must agree with scikit-learn itself, where that is importable."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd import _lib
from cnmf_amd import engine as engine_mod
from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import Preprocess
from oracle import consensus as oc
from tests import _kmeans_ref as kref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(engine_mod.Engine, "__init__", refuse)


def test_keyword_values_are_checked_before_any_engine_is_made(no_device):
    pca, obs = kref.ref.make_case(40, 4, [3], seed=1)
    P = Preprocess()
    with pytest.raises(ValueError, match="kmeans_init must be one of"):
        P.run_harmony(pca, obs, list(obs.columns), kmeans_init="nonsense")
    counts = (sp.csr_matrix(np.ones((40, 6))), list(obs.index), ["g%d" % j for j in range(6)])
    hv = np.arange(6) < 4
    for call in (lambda **k: P.normalize_batchcorrect(counts, obs=obs, highly_variable=hv, harmony_vars=["var0"], **k),
                 lambda **k: P.preprocess_for_cnmf(counts, obs=obs, highly_variable=hv, harmony_vars=["var0"], **k),
                 lambda **k: P.harmony_correct_X(counts[0], obs, pca, ["var0"], **k)):
        with pytest.raises(ValueError, match="harmony must be one of"):
            call(harmony="nonsense")
    assert pp.HARMONY_MODES == ("harmonypy", "device", "device_full")
    assert pp.KMEANS_INIT_MODES == ("sklearn", "device")


def test_more_clusters_than_cells(no_device):
    pca, obs = kref.ref.make_case(12, 3, [3], seed=1)
    with pytest.raises(ValueError, match=r"nclust = 13 for 12 cells \(more clusters than cells need init_centroids\)"):
        Preprocess().run_harmony(pca, obs, list(obs.columns), nclust=13, kmeans_init="device")


@pytest.mark.parametrize("K", [1, 2, 8, 100, 128])
def test_uniform_stream(K):
    for n_init, random_state in ((10, 0), (3, 7)):
        got = engine_mod.Engine.kmeans_uniforms(K, n_init, random_state)
        assert np.array_equal(got, oc.kmeans_uniforms(K, n_init=n_init, random_state=random_state))
        assert got.shape == (n_init, 1 + (K - 1) * (2 + int(np.log(K))))


def test_the_entry_is_declared():
    assert "cnmf_harmony_kmeans_init" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "cnmf_hip.h")).read()
    assert re.search(r"\bint cnmf_harmony_kmeans_init\s*\(cnmf_ctx\*", header)
    for name in ("engine.py", "preprocess.py"):                            # the package draws the stream itself
        src = open(os.path.join(ROOT, "cnmf_amd", name)).read()
        assert "import oracle" not in src and "from oracle" not in src


def test_traced_single_run_is_kmeans_single():
    """tests/_kmeans_ref.single_trace restates oracle.consensus.kmeans_single: equal on runs that stop strictly, on the
    tolerance and on max_iter"""
    X = kref.unit_scores(257, 7, 10)[0]
    Xc, mean, tol_ = kref.centred(X)
    x_sq = (Xc * Xc).sum(axis=1)
    for max_iter, tol in ((25, tol_), (25, 0.0), (1, tol_), (3, 1.0)):
        c0, _ = oc.kmeans_plusplus(Xc, 9, x_sq, np.random.RandomState(0))
        a = oc.kmeans_single(Xc, c0, max_iter, tol)
        b = kref.single_trace(Xc, c0, max_iter, tol)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
    want = oc.kmeans(X, 9, n_init=10, random_state=0, max_iter=25)
    got = kref.kmeans_all(X, 9, n_init=10, random_state=0, max_iter=25)
    assert np.array_equal(want[0], got["labels"][got["best"]]) and want[2] == got["inertia"][got["best"]]
    assert np.array_equal(want[1], got["centers"][got["best"]])


@pytest.mark.parametrize("case", kref.PARITY_CASES, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_the_oracle_agrees_with_scikit_learn_on_the_gpu_inputs(case):
    pytest.importorskip("sklearn.cluster")
    N, d, K, seed, random_state = case
    X = kref.unit_scores(N, d, seed)[0]
    want = kref.kmeans_all(X, K, random_state=random_state)
    assert np.array_equal(kref.sklearn_labels(X, K, random_state), want["labels"][want["best"]])
