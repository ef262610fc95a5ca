"""What the tests of the device k-means initialisation (Engine.harmony_kmeans_init) are held to: oracle/consensus.py's
numpy restatement of scikit-learn's KMeans, run init by init so that every init's labels, inertia and iteration count are
at hand, and the long double per-cluster means and inertia of given labels.  Inputs are the unit scores of
tests/_harmony_ref.make_case, as Preprocess.run_harmony forms them."""
import numpy as np

from oracle import consensus as oc
from tests import _harmony_ref as ref

LD = np.longdouble
EPS = 2.0 ** -53


def unit_scores(N, d, seed):
    """(X [N][d] unit rows, pca, obs) of make_case(N, d, [3], seed): every cell's scores over their largest, at unit L2 norm"""
    pca, obs = ref.make_case(N, d, [3], seed=seed)
    Z = pca.T / pca.T.max(axis=0)
    Z = Z / np.sqrt((Z * Z).sum(axis=0))
    return np.ascontiguousarray(Z.T), pca, obs


def centred(X, tol=1e-4):
    """(X - its column means, the means, tol_) as KMeans.fit forms them"""
    X = np.array(X, dtype=np.float64)
    tol_ = np.mean(np.var(X, axis=0)) * tol
    mean = X.mean(axis=0)
    return X - mean, mean, tol_


def single_trace(Xc, centers, max_iter, tol_):
    """oracle.consensus.kmeans_single, line for line, which also returns the labels its last M step averaged
    (``labels_m``): the returned centres are the means of those cells.  After a strict stop they are the returned labels;
    after a stop on the tolerance or on max_iter the final E step may move a few cells.
    tests/test_host_harmony_init.py holds this loop to kmeans_single itself."""
    labels_old = np.full(Xc.shape[0], -1, dtype=np.int32)
    strict = False
    it = 0
    for it in range(max_iter):
        labels, new, shift = oc.lloyd_iter(Xc, centers)
        centers = new
        labels_m = labels
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if (shift ** 2).sum() <= tol_:
            break
        labels_old = labels
    if not strict:
        labels, _, _ = oc.lloyd_iter(Xc, centers, update=False)
    inertia = float(((Xc - centers[labels]) ** 2).sum())
    return labels, inertia, centers, it + 1, labels_m


def kmeans_all(X, k, n_init=10, random_state=1, max_iter=25, tol=1e-4):
    """oracle.consensus.kmeans as a loop over kmeans_plusplus and the single run.  Returns a dict: ``labels`` [n_init][N],
    ``inertia`` [n_init], ``n_iter`` [n_init], ``centers`` [n_init][k][d] (the mean added back), ``labels_m`` [n_init][N]
    and ``best``."""
    Xc, mean, tol_ = centred(X, tol)
    x_sq = (Xc * Xc).sum(axis=1)
    rng = np.random.RandomState(random_state)
    out = dict(labels=[], inertia=[], n_iter=[], centers=[], labels_m=[], best=None)
    for i in range(n_init):
        c0, _ = oc.kmeans_plusplus(Xc, k, x_sq, rng)
        labels, inertia, centers, n_iter, labels_m = single_trace(Xc, c0, max_iter, tol_)
        b = out["best"]
        if b is None or (inertia < out["inertia"][b] and not oc._same_clustering(labels, out["labels"][b], k)):
            out["best"] = i
        out["labels"].append(labels); out["inertia"].append(inertia); out["n_iter"].append(n_iter)
        out["centers"].append(centers + mean); out["labels_m"].append(labels_m)
    return out


def lloyd_from(X, centers0, max_iter=25, tol=1e-4):
    """kmeans_single from the given centres (coordinates of X), as KMeans(init=centers0, n_init=1) runs it:
    (labels, inertia, centers, n_iter, labels_m)"""
    Xc, mean, tol_ = centred(X, tol)
    labels, inertia, centers, n_iter, labels_m = single_trace(Xc, np.asarray(centers0, dtype=np.float64) - mean, max_iter, tol_)
    return labels, inertia, centers + mean, n_iter, labels_m


def cluster_means_ld(X, labels, k):
    """(long double mean of the cells of every label [k][d], counts [k]); a label nobody holds gives a row of NaN"""
    X = np.asarray(X, dtype=LD)
    means = np.full((k, X.shape[1]), np.nan, dtype=LD)
    counts = np.bincount(labels, minlength=k)
    for j in range(k):
        if counts[j]:
            means[j] = X[labels == j].sum(axis=0) / LD(counts[j])
    return means, counts


def inertia_ld(X, labels, centers):
    diff = np.asarray(X, dtype=LD) - np.asarray(centers, dtype=LD)[labels]
    return (diff * diff).sum()


def center_bound(counts):
    """|centre - long double mean| per component, for unit cells (centred values below 2) in any summation order"""
    return 2.0 * (np.asarray(counts, dtype=np.float64) + 6.0) * EPS


def sklearn_labels(X, k, random_state, n_init=10, max_iter=25):
    """labels_ of scikit-learn's own KMeans, or None where the library is absent"""
    try:
        from sklearn.cluster import KMeans
    except Exception:
        return None
    return KMeans(n_clusters=k, init="k-means++", n_init=n_init, max_iter=max_iter, random_state=random_state).fit(X).labels_


# (N, d, K, data seed, random_state): the wave edge, the 256- and 512-cell chunk edges plus one, the largest d and K,
# L = 2 .. 6, K = 1 and K = N
PARITY_CASES = [
    (63, 4, 3, 63, 1), (64, 4, 3, 64, 1), (65, 4, 3, 65, 1),
    (129, 5, 128, 4, 0), (257, 7, 9, 10, 0), (300, 64, 10, 12, 2), (600, 10, 20, 12, 2), (1025, 17, 34, 3, 1),
    (4097, 3, 100, 5, 0), (5000, 50, 128, 7, 3),
    (100, 4, 1, 100, 1), (16, 4, 16, 16, 1),
]
