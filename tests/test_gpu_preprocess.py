"""Preprocess on the device against what the UNMODIFIED reference's preprocess.py computed for the same counts
(tests/golden/ref_preprocess.npz, tools/make_golden_preprocess.py; the counts are regenerated here from its seeds), a
full-size ridge correction against a float64 numpy restatement, determinism, and the hand-off to cNMF.prepare."""
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import synth
from cnmf_amd.cnmf import cNMF
from cnmf_amd.engine import Engine
from cnmf_amd.preprocess import Preprocess, stdscale_quantile_celing

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SCALE_RUNS = [(None, .9999), (None, .99), (5.0, None)]       # tools/make_golden_preprocess.py
HARMONY_K = 10


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "ref_preprocess.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def inputs(gold):
    """tools/make_golden_preprocess.py's make_inputs"""
    n, g, k, mu, sg, seed = gold["params"].tolist()
    n, g, k, seed = int(n), int(g), int(k), int(seed)
    Cm, _ = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    Cm = Cm.astype(np.float64)
    rs = np.random.RandomState(int(gold["hvg_seed"]))
    ok = np.flatnonzero((Cm > 0).sum(axis=0) >= 2)
    mask = np.zeros(g, dtype=bool)
    mask[rs.choice(ok, int(gold["n_hvg"]), replace=False)] = True
    cells = ["c%d" % i for i in range(n)]
    genes = ["g%d" % j for j in range(g)]
    obs = pd.DataFrame({"batch": ["b%d" % (i % int(gold["n_batch"])) for i in range(n)]}, index=cells)
    assert [genes[j] for j in np.flatnonzero(mask)] == list(gold["hvgs"])
    return Cm, cells, genes, mask, obs


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as e:
        yield e


class FakeHarmony:
    """the golden tool's harmonypy stand-in, replayed from the stored factors"""

    def __init__(self, gold, new_layout):
        self.R, self.Phi, self.pca = gold["R"], gold["Phi"], gold["X_pca"]
        self.new_layout = new_layout

    def result(self):
        res = types.SimpleNamespace(K=HARMONY_K, lamb=np.diag(np.r_[0.0, np.ones(self.Phi.shape[0] - 1)]))
        if self.new_layout:
            res.Z_corr, res.R, res.Phi_moe = 0.5 * self.pca, self.R.T.copy(), self.Phi.T.copy()
        else:
            res.Z_corr, res.R, res.Phi_moe = (0.5 * self.pca).T.copy(), self.R.copy(), self.Phi.copy()
        return res

    def module(self):
        mod = types.ModuleType("harmonypy")

        def run_harmony(data_mat, meta_data, vars_use, max_iter_harmony=20, theta=1):
            assert list(vars_use) == ["batch"] and data_mat.shape == self.pca.shape
            assert list(meta_data["batch"][:3]) == ["b0", "b1", "b2"]
            return self.result()
        mod.run_harmony = run_harmony
        return mod


def same_up_to_column_sign(a, b, rel):
    assert a.shape == b.shape
    for j in range(a.shape[1]):
        s = 1.0 if np.dot(a[:, j], b[:, j]) >= 0 else -1.0
        assert np.abs(s * a[:, j] - b[:, j]).max() <= rel * np.abs(b[:, j]).max(), j


# ---------------------------------------------------------------- 1. scaling and the quantile ceiling
@pytest.mark.parametrize("run", range(len(SCALE_RUNS)))
def test_stdscale_quantile_celing_dense_and_csr(engine, gold, inputs, run):
    C, _, _, mask, _ = inputs
    raw = C[:, mask]
    mv, q = SCALE_RUNS[run]
    ref = raw / gold["scale_%d_std" % run]
    if mv is not None:
        ref[ref > mv] = mv
    thresh_ref = gold["scale_%d_thresh" % run]
    ref = np.minimum(ref, thresh_ref)
    dense = stdscale_quantile_celing(raw, max_value=mv, quantile_thresh=q, engine=engine)
    csr = stdscale_quantile_celing(sp.csr_matrix(raw), max_value=mv, quantile_thresh=q, engine=engine)
    assert isinstance(dense, np.ndarray) and sp.isspmatrix_csr(csr)
    assert np.array_equal(csr.toarray(), dense)
    assert rel_err(dense, ref) <= 1e-12
    if q is not None:
        # the ceiling is np.quantile of the device's own scaled matrix, bit for bit, and the reference's to 1e-12
        pre = stdscale_quantile_celing(raw, max_value=mv, quantile_thresh=None, engine=engine)
        ceiling = dense.max()
        assert ceiling == np.quantile(pre.reshape(-1), q)
        assert abs(ceiling - thresh_ref) <= 1e-12 * thresh_ref
        pre_ref = raw / gold["scale_%d_std" % run]
        if np.array_equal(pre, pre_ref):                    # (same scaled bits -> the same ceiling bits)
            assert ceiling == thresh_ref


def test_order_statistics_count_implicit_zeros(engine):
    rs = np.random.RandomState(3)
    X = sp.random(500, 300, density=0.07, random_state=rs, format="csr")
    X.data = np.ceil(X.data * 40)
    pre = stdscale_quantile_celing(X, quantile_thresh=None, engine=engine).toarray()
    for q in (0.0, 0.5, 0.93, 0.95, 0.999, 1.0):
        out = stdscale_quantile_celing(X, quantile_thresh=q, engine=engine)
        assert out.toarray().max() == np.quantile(pre.reshape(-1), q), q
        assert np.array_equal(out.toarray(), np.minimum(pre, np.quantile(pre.reshape(-1), q))), q


# ---------------------------------------------------------------- 2. the ridge correction
@pytest.mark.parametrize("new_layout", [False, True])
def test_harmony_correct_X_both_layouts(engine, gold, inputs, new_layout):
    C, _, _, mask, obs = inputs
    X = np.minimum(C[:, mask] / gold["corr_scale_std"], gold["corr_thresh"])
    P = Preprocess(engine=engine)
    Xc, Zh = P.harmony_correct_X(X, obs, gold["X_pca"], ["batch"],
                                 harmony_res=FakeHarmony(gold, new_layout).result())
    ref = gold["corr_X"]
    assert rel_err(Xc, ref) <= 1e-10
    far = np.abs(ref) > 1e-12
    assert np.array_equal(Xc[far] == 0, ref[far] == 0)
    assert np.array_equal(Zh, 0.5 * gold["X_pca"])
    # sparse input: the same bits
    Xs, _ = P.harmony_correct_X(sp.csr_matrix(X), obs, gold["X_pca"], ["batch"],
                                harmony_res=FakeHarmony(gold, new_layout).result())
    assert np.array_equal(Xs, Xc)


# ---------------------------------------------------------------- 3. the whole pipeline
def test_normalize_batchcorrect_without_harmony(engine, gold, inputs):
    C, cells, genes, mask, obs = inputs
    P = Preprocess(engine=engine)
    res, hvgs = P.normalize_batchcorrect((sp.csr_matrix(C), cells, genes), obs=obs, highly_variable=mask,
                                         normalize_librarysize=True, makeplots=False)
    assert hvgs == list(gold["hvgs"]) and list(res.var_names) == hvgs and list(res.obs_names) == cells
    assert sp.isspmatrix_csr(res.X)
    ref = sp.csr_matrix(C[:, mask])
    assert np.array_equal(res.X.indptr, ref.indptr) and np.array_equal(res.X.indices, ref.indices)
    assert rel_err(res.X.data, gold["plain_data"]) <= 1e-12
    # highly_variable as gene names, dense input: same values, dense result
    res2, hvgs2 = P.normalize_batchcorrect(pd.DataFrame(C, index=cells, columns=genes), highly_variable=list(gold["hvgs"]),
                                           normalize_librarysize=True, makeplots=False)
    assert hvgs2 == hvgs and isinstance(res2.X, np.ndarray)
    assert np.array_equal(res2.X, res.X.toarray())


@pytest.mark.parametrize("norm", [False, True])
def test_normalize_batchcorrect_with_harmony(monkeypatch, engine, gold, inputs, norm):
    C, cells, genes, mask, obs = inputs
    monkeypatch.setitem(sys.modules, "harmonypy", FakeHarmony(gold, new_layout=False).module())
    P = Preprocess(engine=engine)
    res, hvgs = P.normalize_batchcorrect((sp.csr_matrix(C), cells, genes), obs=obs, highly_variable=mask,
                                         normalize_librarysize=norm, harmony_vars=["batch"], makeplots=False)
    assert hvgs == list(gold["hvgs"])
    assert isinstance(res.X, np.ndarray)
    same_up_to_column_sign(res.obsm["X_pca"], gold["X_pca"], 1e-9)
    assert np.array_equal(res.obsm["X_pca_harmony"], 0.5 * gold["X_pca"])
    assert rel_err(res.X, gold["corr_norm_X" if norm else "corr_X"]) <= 1e-10


# ---------------------------------------------------------------- 4. full size, determinism
def test_full_size_ridge_against_numpy_and_determinism(engine):
    N, G, K, nb = 50000, 2000, 100, 4
    rs = np.random.RandomState(5)
    X = rs.gamma(0.5, 1.0, size=(N, G))
    batch = rs.randint(0, nb, size=N)
    Phi = np.vstack([np.ones(N)] + [(batch == b).astype(np.float64) for b in range(nb)])
    logits = rs.randn(K, N) * 2
    R = np.exp(logits - logits.max(axis=0))
    R /= R.sum(axis=0)
    lamb = np.diag(np.r_[0.0, np.ones(nb)])
    res = types.SimpleNamespace(Z_corr=np.zeros((10, N)), R=R, Phi_moe=Phi, K=K, lamb=lamb)
    P = Preprocess(engine=engine)
    out1, _ = P.harmony_correct_X(X, None, np.zeros((N, 10)), ["batch"], harmony_res=res)
    out2, _ = P.harmony_correct_X(X, None, np.zeros((N, 10)), ["batch"], harmony_res=res)
    assert np.array_equal(out1.view(np.uint64), out2.view(np.uint64))
    A = (R[:, None, :] * Phi[None, :, :]).reshape(K * (nb + 1), N)
    M = (A @ X).reshape(K, nb + 1, G)
    gram = (A @ Phi.T).reshape(K, nb + 1, nb + 1)
    W = np.empty_like(M)
    for k in range(K):
        W[k] = np.linalg.inv(gram[k] + lamb) @ M[k]
        W[k][0, :] = 0
    ref = X - A.T @ W.reshape(K * (nb + 1), G)
    ref[ref < 0] = 0
    assert rel_err(out1, ref) <= 1e-11


# ---------------------------------------------------------------- 5. hand-off and a shared engine
def test_handoff_to_prepare_and_shared_engine(tmp_path, monkeypatch, gold, inputs):
    C, cells, genes, mask, obs = inputs
    monkeypatch.setitem(sys.modules, "harmonypy", FakeHarmony(gold, new_layout=False).module())
    with Engine(0) as eng:
        res, hvgs = Preprocess(engine=eng).normalize_batchcorrect((sp.csr_matrix(C), cells, genes), obs=obs,
                                                                  highly_variable=mask, harmony_vars=["batch"],
                                                                  makeplots=False)
        genes_fn = os.path.join(str(tmp_path), "hvgs.txt")
        with open(genes_fn, "w") as F:
            F.write("\n".join(hvgs))
        obj = cNMF(output_dir=str(tmp_path), name="pp", engine=eng)
        obj.prepare((res.X, res.obs_names, hvgs), components=[4], n_iter=2, seed=3, genes_file=genes_fn)
        obj.factorize(write_iter_files=False)
        first = {k: v.copy() for k, v in obj.spectra_cache.items()}
        # a Preprocess call on the same engine between two factorize runs changes nothing
        Preprocess(engine=eng).normalize_batchcorrect((sp.csr_matrix(C), cells, genes), obs=obs, highly_variable=mask,
                                                      harmony_vars=["batch"], makeplots=False)
        obj.factorize(write_iter_files=False)
        assert sorted(first) == sorted(obj.spectra_cache)
        for key, H in first.items():
            assert np.array_equal(H, obj.spectra_cache[key]), key
