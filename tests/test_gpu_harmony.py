"""Preprocess.run_harmony on the device against the float64 numpy restatement (tests/_harmony_ref.py).

1. Every case: the same number of harmony rounds and the same kmeans_rounds; R, Z_corr, Y and both objective histories
   within 16 x the distance of the restatement from its own long double run (measured here, per case and per quantity:
   the device differs from numpy in the summation order over at most N terms, repeated over at most 400 updates, and
   in the last place of exp / log / pow).  The restatement's convergence ratios stay at least 1e-3 (relative) away
   from both thresholds, so that no case is decided by rounding.
   The baselines (max |float64 - long double| of R, Z_corr, Y, objective_kmeans) measured when this file was written:
     a        N 600 d 10 one variable (3) K 20            4.1e-15  1.1e-13  8.1e-15  2.7e-13
     b        N 257 d 7 two variables (3 + 2) K 9         2.6e-14  6.5e-14  9.0e-15  3.0e-13
     c        N 19 d 3 one (2) K 1, 20 blocks, one empty  0        2.9e-15  2.7e-17  1.3e-15
     d        N 64 d 5 one (2) nclust 128 (given init)    1.1e-15  9.1e-15  1.3e-15  5.8e-15
     e        N 300 d 64 one (4), a level with one cell   5.9e-15  6.3e-14  2.9e-15  7.0e-14
     a-theta0 / a-theta2 / a-one-round / a-init (R)       2.1e-15 / 9.6e-15 / 3.3e-15 / 3.3e-15
     n63 / n65 / n129 (d 4, K 3, two rounds) (R)          1.5e-15 / 4.9e-15 / 1.7e-16
   (they move in the last digit with the host's BLAS; the test measures them again on every run).  The device's own
   differences were between 0.01 and 7.0 times these (CHANGELOG.md).
   Case d has more clusters than cells, which scikit-learn's KMeans refuses: its centroids are given (init_centroids).
   Cases of more than 256 cells share one KMeans result among their runs (case_inputs says why).
2. Two device runs on the same centroids agree bit for bit; numpy's global RandomState after the call equals the restatement's.
3. normalize_batchcorrect(harmony="device") equals the same call with harmony_res=run_harmony(...) bit for bit, with
   harmonypy not importable.
4. Two batches shifted along one component come together: the distance of the batch centroids in Z_corr is below half
   of that in Z (the restatement alone: 4.102 -> 0.567 at seed 0).
5. The unclipped ridge apply against the long double product of tests/_pre_ref.py on a matrix with negative entries."""
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd.preprocess import Preprocess
from tests import _harmony_ref as ref
from tests import _pre_ref as pre_ref

pytestmark = pytest.mark.gpu
LD = np.longdouble

# name: (N, d, levels per variable, data seed, singleton level, run_harmony keywords)
CASES = {
    "a": (600, 10, [3], 12, False, dict(random_state=2)),
    "b": (257, 7, [3, 2], 10, False, dict(random_state=0)),
    "c": (19, 3, [2], 10, False, dict(random_state=0)),
    "d": (64, 5, [2], 11, False, dict(random_state=1, nclust=128, init_seed=1)),
    "e": (300, 64, [4], 12, True, dict(random_state=2)),
    "a-theta0": (600, 10, [3], 12, False, dict(random_state=2, theta=0)),
    "a-theta2": (600, 10, [3], 12, False, dict(random_state=2, theta=2)),
    "a-one-round": (600, 10, [3], 12, False, dict(random_state=2, max_iter_harmony=1)),
    "a-init": (600, 10, [3], 12, False, dict(random_state=2, init_seed=7)),
    "n63": (63, 4, [2], 63, False, dict(random_state=1, nclust=3, max_iter_harmony=2)),
    "n65": (65, 4, [2], 65, False, dict(random_state=1, nclust=3, max_iter_harmony=2)),
    "n129": (129, 4, [2], 129, False, dict(random_state=1, nclust=3, max_iter_harmony=2)),
}
_CACHE = {}


_INIT = {}


def case_inputs(name):
    """(pca, obs, variables, run_harmony keywords).  scikit-learn's Lloyd iteration works in chunks of 256 cells and its
    threads add their partial sums in completion order: beyond one chunk its centroids vary in the last bit from run to
    run (3 distinct results in 60 runs of case a).  The cases of more than 256 cells therefore make that same KMeans call
    once and hand its centroids to every run, restatement and device alike; the smaller ones leave the call to
    run_harmony."""
    N, d, levels, seed, singleton, kw = CASES[name]
    pca, obs = ref.make_case(N, d, levels, seed=seed, singleton=singleton)
    kw = dict(kw)
    init_seed = kw.pop("init_seed", None)
    K = kw.get("nclust") or int(min(np.round(N / 30.0), 100))
    if init_seed is not None:
        kw["init_centroids"] = np.random.RandomState(init_seed).randn(d, K)
    elif N > 256:
        if name not in _INIT:
            Z_cos = pca.T / pca.T.max(axis=0)
            _INIT[name] = ref.kmeans_centroids(Z_cos / np.sqrt((Z_cos * Z_cos).sum(axis=0)), K, kw["random_state"])
        kw["init_centroids"] = _INIT[name]
    return pca, obs, list(obs.columns), kw


def reference(name):
    """(float64 restatement, long double restatement, numpy's RandomState after the float64 run), computed once"""
    if name not in _CACHE:
        pca, obs, hvars, kw = case_inputs(name)
        h64 = ref.run_harmony(pca, obs, hvars, **kw)
        state = np.random.get_state()
        hld = ref.run_harmony(pca, obs, hvars, dtype=LD, **kw)
        _CACHE[name] = (h64, hld, state)
    return _CACHE[name]


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


@pytest.fixture
def P(engine):
    return Preprocess(engine=engine)


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(P, name):
    h64, hld, state = reference(name)
    margin = ref.threshold_margin(h64)
    print("%s: K %d, kmeans_rounds %s, threshold margin %.3g" % (name, h64.K, h64.kmeans_rounds, margin))
    assert margin >= 1e-3
    assert hld.kmeans_rounds == h64.kmeans_rounds          # the baseline compares like with like
    pca, obs, hvars, kw = case_inputs(name)
    got = P.run_harmony(pca, obs, hvars, **kw)
    assert same_state(np.random.get_state(), state)
    failures = []
    for what in ("R", "Z_corr", "Y", "objective_harmony", "objective_kmeans"):
        if np.shape(getattr(got, what)) != np.shape(getattr(h64, what)):
            continue                                        # (reported by the assertions on the rounds below)
        base = maxdiff(getattr(h64, what), getattr(hld, what))
        err = maxdiff(getattr(got, what), getattr(h64, what))
        print("%s %s: restatement vs long double %.3e, device vs restatement %.3e (%.2f x)" % (
            name, what, base, err, err / base if base else np.inf if err else 0.0))
        if not err <= 16 * base:
            failures.append((what, err, base))
    assert got.kmeans_rounds == h64.kmeans_rounds
    assert len(got.objective_harmony) == len(h64.objective_harmony)
    assert len(got.objective_kmeans) == len(h64.objective_kmeans)
    assert got.K == h64.K and np.array_equal(got.lamb, np.asarray(h64.lamb, dtype=np.float64))
    assert np.array_equal(got.Phi_moe, np.asarray(h64.Phi_moe, dtype=np.float64))
    assert got.Z_cos.shape == got.Z_corr.shape == (pca.shape[1], pca.shape[0])
    assert np.allclose(np.sqrt((got.Z_cos ** 2).sum(axis=0)), 1.0, rtol=0, atol=1e-14)
    assert not failures, failures


def test_case_c_has_an_empty_block():
    assert sum(len(b) == 0 for b in np.array_split(np.arange(19), 20)) == 1


@pytest.mark.parametrize("name", ["a", "b", "d", "n129"])
def test_two_runs_agree_bit_for_bit(P, name):
    pca, obs, hvars, kw = case_inputs(name)
    one = P.run_harmony(pca, obs, hvars, **kw)
    two = P.run_harmony(pca, obs, hvars, **kw)
    for what in ("R", "Z_corr", "Z_cos", "Y"):
        assert np.array_equal(getattr(one, what), getattr(two, what)), what
    assert one.objective_kmeans == two.objective_kmeans and one.objective_harmony == two.objective_harmony
    assert one.kmeans_rounds == two.kmeans_rounds


@pytest.fixture
def counts():
    rs = np.random.RandomState(3)
    N, G = 240, 40
    batch = rs.randint(0, 2, size=N)
    rate = rs.gamma(2.0, 1.0, size=(3, G))[rs.randint(0, 3, size=N)] * (1 + 0.8 * batch[:, None] * (np.arange(G) % 3 == 0))
    C = rs.poisson(rate).astype(np.float64)
    C[:, 0] += 1                                            # no empty cell
    cells, genes = ["c%d" % i for i in range(N)], ["g%d" % j for j in range(G)]
    obs = pd.DataFrame({"batch": ["b%d" % b for b in batch]}, index=cells)
    return (sp.csr_matrix(C), cells, genes), obs, np.arange(G) < 30


def test_normalize_batchcorrect_device_route(P, counts, monkeypatch):
    monkeypatch.setitem(sys.modules, "harmonypy", None)     # import harmonypy -> ImportError
    data, obs, hv = counts
    res, hvgs = P.normalize_batchcorrect(data, obs=obs, highly_variable=hv, harmony_vars=["batch"], harmony="device",
                                         makeplots=False)
    assert res.X.shape == (240, 30) and np.isfinite(res.X).all() and (res.X >= 0).all()
    hres = P.run_harmony(res.obsm["X_pca"], obs, ["batch"])
    res2, _ = P.normalize_batchcorrect(data, obs=obs, highly_variable=hv, harmony_vars=["batch"], harmony_res=hres,
                                       makeplots=False)
    assert np.array_equal(res.X, res2.X)
    assert np.array_equal(res.obsm["X_pca_harmony"], res2.obsm["X_pca_harmony"])
    assert np.array_equal(res.obsm["X_pca_harmony"], hres.Z_corr.T)
    # harmony_correct_X takes the same route
    X = P.normalize_batchcorrect(data, highly_variable=hv, makeplots=False)[0].X
    Xc, Zh = P.harmony_correct_X(X, obs, res.obsm["X_pca"], ["batch"], harmony="device")
    assert np.array_equal(Zh, hres.Z_corr.T) and Xc.shape == (240, 30)


def test_two_shifted_batches_come_together(P):
    pca, obs, batch = ref.make_two_batches(400, 6, seed=0)
    before = ref.batch_gap(pca.T, batch)
    h = ref.run_harmony(pca, obs, "batch", random_state=0)
    after_ref = ref.batch_gap(h.Z_corr, batch)
    got = P.run_harmony(pca, obs, "batch", random_state=0)
    after = ref.batch_gap(got.Z_corr, batch)
    print("batch centroid distance: %.4f before, %.4f restatement, %.4f device" % (before, after_ref, after))
    assert after_ref < 0.5 * before                         # 4.102 -> 0.567
    assert after < 0.5 * before


@pytest.mark.parametrize("case", [(257, 65, 7, 5), (63, 10, 3, 2), (4097, 3, 13, 5)], ids=["257x65", "63x10", "4097x3"])
def test_unclipped_ridge_apply(engine, case):
    N, G, K, B1 = case
    X = pre_ref.make_X(N, G, seed=N + G)
    X[:, 1::4] -= 1e6
    X -= 0.5                                                # entries of both signs
    R, Phi = pre_ref.make_ridge(N, K, B1, seed=N + G)
    W = pre_ref.make_W(K, B1, G, seed=N + G)
    try:
        engine.preprocess_set_dense(0, X)
        engine.preprocess_ridge_moments(0, R, Phi)
        engine.preprocess_ridge_apply(0, W, clip=False)
        got = engine.preprocess_fetch(0)
        engine.preprocess_set_dense(0, X)
        engine.preprocess_ridge_moments(0, R, Phi)
        engine.preprocess_ridge_apply(0, W)
        clipped = engine.preprocess_fetch(0)
    finally:
        engine.preprocess_release()
    A = pre_ref.ridge_operand(R, Phi)
    prod, mag = pre_ref.ld_product(A.T, W.reshape(K * B1, G))
    want = X.astype(LD) - prod
    bound = pre_ref.gemm_bound(K * B1, mag) + pre_ref.U * np.abs(want).astype(np.float64)
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    print("unclipped apply: worst err / bound %.3f, %d negative entries" % (np.max(err / bound), int((got < 0).sum())))
    assert np.all(err <= bound)
    assert (got < 0).any() and (got > 0).any()
    assert np.array_equal(clipped, np.maximum(got, 0.0))   # the clipped mode: the same difference, then the maximum
