"""Harmony's k-means initialisation on the device (Engine.harmony_kmeans_init, csrc/harmony_init_host.hip.h) against
oracle/consensus.py's numpy restatement of scikit-learn's KMeans (tests/_kmeans_ref.py), and the plumbing of
``run_harmony(kmeans_init="device")`` / ``harmony="device_full"``.

The cells the oracle clusters are the unit scores the device holds after harmony_begin (harmony_fetch): those are what
the device clusters, and numpy's own unit scores differ from them in the last bit where d >= 8 (numpy adds the squares
of a cell pairwise, the device one after the other).

Bounds.  A returned centre is the mean of the n_j cells the last M step averaged (``labels_m`` of the oracle's run: the
returned labels after a strict stop); cells are unit vectors and centred values are below 2, so in any summation order
it lies within 2 (n_j + 6) 2^-53 of the long double mean.  The inertia is compared with the long double inertia of the
returned Y and labels within (N + 2 d + 8) 2^-53 relative, plus 4 N d 2^-106: Y = c + mean and x - mean are each rounded
once (below 2^-53 per component), the square of which is what is left of the recomputed inertia where the device's own
is exactly 0 (K = N: every cell is its own centre)."""
import sys

import numpy as np
import pytest

from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import Preprocess
from oracle import consensus as oc
from tests import _kmeans_ref as kref
from tests.test_gpu_harmony import counts, same_state  # noqa: F401  (the 240 x 40 counts fixture)

pytestmark = pytest.mark.gpu
EPS = kref.EPS
_REF = {}


def begin(engine, pca, obs, K):
    """harmony_begin as run_harmony calls it; returns the unit scores [N][d] the device holds"""
    Phi, codes, level_var, n_levels = pp.harmony_design(obs, list(obs.columns))
    N = pca.shape[0]
    engine.harmony_begin(pca, codes, level_var, np.ones(Phi.shape[0]), np.repeat(0.1, K), Phi.sum(axis=1) / N)
    return np.ascontiguousarray(engine.harmony_fetch(z_cos_only=True).T)


def reference(case, X, **kw):
    key = (case, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = kref.kmeans_all(X, case[2], random_state=case[4], **kw)
    return _REF[key]


def check_centres(Y, X, labels_m, K, oracle_centres=None, what=""):
    means, n = kref.cluster_means_ld(X, labels_m, K)
    bound = kref.center_bound(n)[:, None]
    held = n > 0
    dev = np.abs(np.asarray(Y.T, dtype=kref.LD) - means)[held] / bound[held]
    msg = "%s centres: device %.3f of the bound" % (what, float(dev.max()))
    if oracle_centres is not None:
        orc = np.abs(np.asarray(oracle_centres, dtype=kref.LD) - means)[held] / bound[held]
        msg += ", oracle %.3f of the bound" % float(orc.max())
    print(msg)
    assert dev.max() <= 1.0


def check_inertia(inertia, Y, X, labels, what=""):
    N, d = X.shape
    ld = kref.inertia_ld(X, labels, Y.T)
    err = abs(kref.LD(inertia) - ld)
    bound = (N + 2 * d + 8) * EPS * ld + 4.0 * N * d * 2.0 ** -106
    print("%s inertia: device %.17g, long double %.17g, |difference| %.3e, bound %.3e" % (what, inertia, float(ld), float(err), float(bound)))
    assert err <= bound


@pytest.mark.parametrize("case", kref.PARITY_CASES, ids=lambda c: "n%d-d%d-k%d" % c[:3])
def test_parity_with_the_oracle(engine, case):
    N, d, K, seed, random_state = case
    _, pca, obs = kref.unit_scores(N, d, seed)
    try:
        X = begin(engine, pca, obs, K)
        Y, labels, inertia, n_iter, best = engine.harmony_kmeans_init(random_state)
    finally:
        engine.harmony_release()
    want = reference(case, X)
    sk = kref.sklearn_labels(X, K, random_state)
    if sk is not None:
        assert np.array_equal(sk, want["labels"][want["best"]]), "invalid input: the oracle and scikit-learn disagree"
    print("n_iter device %s oracle %s; best device %d oracle %d" % ([int(x) for x in n_iter], want["n_iter"], best, want["best"]))
    assert best == want["best"]
    assert np.array_equal(labels, want["labels"][best])
    assert list(n_iter) == want["n_iter"]
    check_centres(Y, X, want["labels_m"][best], K, want["centers"][best], "n%d" % N)
    check_inertia(inertia[best], Y, X, labels, "n%d" % N)


def test_one_init_one_iteration(engine):
    """n_init = 1, max_iter = 1: the run stops on max_iter, so the final E step runs"""
    case = (257, 7, 9, 10, 0)
    N, d, K, seed, random_state = case
    _, pca, obs = kref.unit_scores(N, d, seed)
    try:
        X = begin(engine, pca, obs, K)
        Y, labels, inertia, n_iter, best = engine.harmony_kmeans_init(random_state, n_init=1, max_iter=1)
    finally:
        engine.harmony_release()
    want = reference(case, X, n_init=1, max_iter=1)
    assert best == 0 and list(n_iter) == want["n_iter"] == [1]
    assert np.array_equal(labels, want["labels"][0])
    assert not np.array_equal(want["labels"][0], want["labels_m"][0])      # the final E step moved cells
    check_centres(Y, X, want["labels_m"][0], K, want["centers"][0], "one iteration")
    check_inertia(inertia[0], Y, X, labels, "one iteration")


def empties_case(engine, N, d, K, n_empty):
    """Lloyd from K distinct cells, the last n_empty of them replaced by points far outside the sphere"""
    rs = np.random.RandomState(0)
    cells = rs.randn(N, d)
    cells /= np.sqrt((cells * cells).sum(axis=1))[:, None]
    obs = kref.ref.make_case(N, d, [3], seed=0)[1]
    X = begin(engine, cells, obs, K)
    centres = X[rs.choice(N, K, replace=False)].copy()
    for j in range(n_empty):
        centres[K - 1 - j] = 5.0 * (1 + j)
    got = engine.harmony_kmeans_init(0, n_init=1, init_centers=centres[None])
    want = kref.lloyd_from(X, centres)
    Xc, mean, _ = kref.centred(X)
    first = oc.lloyd_iter(Xc, centres - mean, update=False)[0]
    assert K - len(np.unique(first)) == n_empty                            # the first step does leave n_empty clusters empty
    return X, got, want


def test_lloyd_from_given_centres_one_empty_cluster(engine):
    N, d, K = 257, 7, 9
    try:
        X, (Y, labels, inertia, n_iter, best), (wl, wi, wc, wn, wm) = empties_case(engine, N, d, K, 1)
    finally:
        engine.harmony_release()
    print("n_iter device %d oracle %d" % (n_iter[0], wn))
    assert best == 0 and n_iter[0] == wn
    assert np.array_equal(labels, wl)
    check_centres(Y, X, wm, K, wc, "one empty")
    check_inertia(inertia[0], Y, X, labels, "one empty")


@pytest.mark.parametrize("N,d,K,n_empty", [(300, 5, 8, 3), (1025, 17, 34, 5)])
def test_lloyd_from_given_centres_several_empty_clusters(engine, N, d, K, n_empty):
    """numpy's argpartition does not order the relocated cells among themselves: compared as clusterings"""
    try:
        X, (Y, labels, inertia, n_iter, best), (wl, wi, wc, wn, wm) = empties_case(engine, N, d, K, n_empty)
    finally:
        engine.harmony_release()
    print("n_iter device %d oracle %d" % (n_iter[0], wn))
    assert n_iter[0] == wn
    assert oc._same_clustering(labels, wl, K) and oc._same_clustering(wl, labels, K)
    got_rows = Y.T[np.lexsort(Y[::-1])]
    want_rows = wc[np.lexsort(wc.T[::-1])]
    bound = 2 * kref.center_bound(np.bincount(wm, minlength=K).max())      # (each side within the bound of the true mean)
    print("sorted centre rows: largest difference %.3e, bound %.3e" % (np.abs(got_rows - want_rows).max(), bound))
    assert np.abs(got_rows - want_rows).max() <= bound
    check_inertia(inertia[0], Y, X, labels, "%d empty" % n_empty)


@pytest.mark.parametrize("case", [(600, 10, 20, 12, 2), (4097, 3, 100, 5, 0)], ids=lambda c: "n%d" % c[0])
def test_two_runs_give_the_same_bits(engine, case):
    N, d, K, seed, random_state = case
    _, pca, obs = kref.unit_scores(N, d, seed)
    runs = []
    for _ in range(2):
        try:
            begin(engine, pca, obs, K)
            runs.append(engine.harmony_kmeans_init(random_state))
        finally:
            engine.harmony_release()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    P = Preprocess(engine=engine)
    one, two = (P.run_harmony(pca, obs, list(obs.columns), nclust=K, random_state=random_state, kmeans_init="device",
                              max_iter_harmony=2) for _ in range(2))
    for what in ("R", "Z_corr", "Y"):
        assert np.array_equal(getattr(one, what), getattr(two, what)), what
    assert one.objective_kmeans == two.objective_kmeans and one.objective_harmony == two.objective_harmony


def test_run_harmony_device_init_is_init_centroids_of_the_same_call(engine):
    N, d, K, seed, random_state = 600, 10, 20, 12, 2
    _, pca, obs = kref.unit_scores(N, d, seed)
    try:
        begin(engine, pca, obs, K)
        Y = engine.harmony_kmeans_init(random_state)[0]
    finally:
        engine.harmony_release()
    P = Preprocess(engine=engine)
    kw = dict(nclust=K, random_state=random_state, max_iter_harmony=2)
    one = P.run_harmony(pca, obs, list(obs.columns), kmeans_init="device", **kw)
    state = np.random.get_state()
    two = P.run_harmony(pca, obs, list(obs.columns), init_centroids=Y, **kw)
    assert same_state(np.random.get_state(), state)
    for what in ("R", "Z_corr", "Z_cos", "Y"):
        assert np.array_equal(getattr(one, what), getattr(two, what)), what
    assert one.objective_kmeans == two.objective_kmeans and one.objective_harmony == two.objective_harmony
    assert one.kmeans_rounds == two.kmeans_rounds


def test_device_full_route_needs_neither_library(engine, counts, monkeypatch):  # noqa: F811
    monkeypatch.setitem(sys.modules, "sklearn.cluster", None)
    monkeypatch.setitem(sys.modules, "harmonypy", None)
    P = Preprocess(engine=engine)
    data, obs, hv = counts
    res, _ = P.normalize_batchcorrect(data, obs=obs, highly_variable=hv, harmony_vars=["batch"], harmony="device_full",
                                      makeplots=False)
    hres = P.run_harmony(res.obsm["X_pca"], obs, ["batch"], kmeans_init="device")
    res2, _ = P.normalize_batchcorrect(data, obs=obs, highly_variable=hv, harmony_vars=["batch"], harmony_res=hres,
                                       makeplots=False)
    assert res.X.shape == (240, 30) and np.isfinite(res.X).all()
    assert np.array_equal(res.X, res2.X)
    assert np.array_equal(res.obsm["X_pca_harmony"], res2.obsm["X_pca_harmony"])
    assert np.array_equal(res.obsm["X_pca_harmony"], hres.Z_corr.T)
    with pytest.raises(ImportError):                                      # (the host route does need scikit-learn)
        P.run_harmony(res.obsm["X_pca"], obs, ["batch"])


def test_harmony_state_is_untouched(engine):
    N, d, K, seed = 600, 10, 20, 12
    _, pca, obs = kref.unit_scores(N, d, seed)
    Y0 = np.random.RandomState(5).randn(d, K)
    Y0 /= np.sqrt((Y0 * Y0).sum(axis=0))
    perm = np.random.RandomState(6).permutation(N)
    out = []
    for with_call in (False, True):
        try:
            begin(engine, pca, obs, K)
            if with_call:
                engine.harmony_kmeans_init(2)
            first = engine.harmony_init(Y0)
            R0 = engine.harmony_fetch()[2]
            if with_call:
                engine.harmony_kmeans_init(2, n_init=2, max_iter=3)
                assert np.array_equal(engine.harmony_fetch()[2], R0)
            out.append((first, engine.harmony_kmeans_step(perm, 20), engine.harmony_fetch()))
        finally:
            engine.harmony_release()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    for a, b in zip(out[0][2], out[1][2]):
        assert np.array_equal(a, b)
