"""A numpy restatement of Harmony's clustering loop as ``Preprocess.run_harmony`` specifies it: the yardstick of the
device path.  Written from the algorithm's description, in float64 by default; ``dtype=np.longdouble`` runs the same
control flow in extended precision (the k-means initialisation and the small matrix inverses stay float64: numpy's
``linalg`` has no long double), which measures how far a float64 run is from its own exact arithmetic.

``run_harmony(pca, obs, harmony_vars, ...)`` takes the arguments of ``Preprocess.run_harmony`` and returns an object
with the same attributes, plus ``ratios_harmony`` / ``ratios_kmeans``: every convergence ratio the run compared with its
thresholds, so that a test can show that a case is not decided by rounding.  ``np.random`` (the global RandomState) is
seeded once and consumed by one ``shuffle`` per ``update_R``, as the device path does."""
import numpy as np
import pandas as pd


class HarmonyRef:
    pass


def design(obs, harmony_vars):
    """(Phi [B][N] float64 one-hot in pd.get_dummies(obs[vars]) column order, levels per variable)"""
    vars_use = [harmony_vars] if isinstance(harmony_vars, str) else list(harmony_vars)
    dummies = pd.get_dummies(obs[vars_use])
    Phi = dummies.to_numpy().T.astype(np.float64)
    n_levels = [pd.get_dummies(obs[[v]]).shape[1] for v in vars_use]
    return Phi, n_levels


def per_level(value, n_levels):
    """a scalar repeated over all levels, or one value per variable repeated over its levels"""
    if np.isscalar(value):
        return np.repeat([float(value)] * len(n_levels), n_levels)
    value = np.asarray(value, dtype=np.float64)
    if len(value) == len(n_levels):
        return np.repeat(value, n_levels)
    assert len(value) == sum(n_levels)
    return value


def kmeans_centroids(Z_cos, K, random_state):
    from sklearn.cluster import KMeans
    model = KMeans(n_clusters=K, init='k-means++', n_init=10, max_iter=25, random_state=random_state)
    model.fit(np.asarray(Z_cos, dtype=np.float64).T)
    return model.cluster_centers_.T


def _objective(h):
    kmeans_error = np.sum(h.R * h.dist)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = h.R * np.log(h.R)
    ent[~np.isfinite(ent)] = 0
    entropy = np.sum(ent * h.sigma[:, None])
    w = (h.theta[None, :] * np.log((h.O + 1) / (h.E + 1))) @ h.Phi
    cross = np.sum(h.R * h.sigma[:, None] * w)
    return kmeans_error + entropy + cross


def _dist(h):
    return 2 * (1 - h.Y.T @ h.Z_cos)


def _update_R(h, block_size):
    S = -h.dist / h.sigma[:, None]
    S = np.exp(S - S.max(axis=0))
    order = np.arange(h.N)
    np.random.shuffle(order)
    for b in np.array_split(order, int(np.ceil(1 / block_size))):
        h.E -= np.outer(h.R[:, b].sum(axis=1), h.Pr_b)
        h.O -= h.R[:, b] @ h.Phi[:, b].T
        Rb = S[:, b] * (np.power((h.E + 1) / (h.O + 1), h.theta[None, :]) @ h.Phi[:, b])
        Rb = Rb / np.abs(Rb).sum(axis=0)
        h.R[:, b] = Rb
        h.E += np.outer(Rb.sum(axis=1), h.Pr_b)
        h.O += Rb @ h.Phi[:, b].T


def _cluster(h, max_iter_kmeans, epsilon_cluster, block_size):
    h.dist = _dist(h)
    i = -1
    for i in range(max_iter_kmeans):
        Y = h.Z_cos @ h.R.T
        h.Y = Y / np.sqrt((Y * Y).sum(axis=0))
        h.dist = _dist(h)
        _update_R(h, block_size)
        h.objective_kmeans.append(_objective(h))
        if i > 3:
            o = h.objective_kmeans
            old, new = o[-2] + o[-3] + o[-4], o[-1] + o[-2] + o[-3]
            ratio = abs(old - new) / abs(old)
            h.ratios_kmeans.append(float(ratio))
            if ratio < epsilon_cluster:
                break
    h.kmeans_rounds.append(i)
    h.objective_harmony.append(h.objective_kmeans[-1])


def _ridge(h):
    """the mixture-of-experts ridge correction of Z_orig with the current R; the (B + 1) x (B + 1) inverses in float64"""
    dt = h.Z_orig.dtype
    Z_corr = h.Z_orig.copy()
    for k in range(h.K):
        Phi_Rk = h.Phi_moe * h.R[k]
        x = Phi_Rk @ h.Phi_moe.T + h.lamb
        inv = np.linalg.inv(np.asarray(x, dtype=np.float64)).astype(dt)
        W = inv @ (Phi_Rk @ h.Z_orig.T)
        W[0, :] = 0
        Z_corr -= W.T @ Phi_Rk
    h.Z_corr = Z_corr
    h.Z_cos = Z_corr / np.sqrt((Z_corr * Z_corr).sum(axis=0))


def run_harmony(pca, obs, harmony_vars, theta=1, max_iter_harmony=20, *, nclust=None, sigma=0.1, lamb=1, block_size=0.05,
                max_iter_kmeans=20, epsilon_cluster=1e-5, epsilon_harmony=1e-4, random_state=0, init_centroids=None,
                dtype=np.float64):
    h = HarmonyRef()
    pca = np.asarray(pca, dtype=np.float64)
    N = h.N = pca.shape[0]
    Phi64, n_levels = design(obs, harmony_vars)
    K = h.K = int(nclust) if nclust is not None else int(min(np.round(N / 30.0), 100))
    h.theta = per_level(theta, n_levels).astype(dtype)
    lam = per_level(lamb, n_levels)
    h.lamb = np.diag(np.insert(lam, 0, 0)).astype(dtype)
    h.sigma = np.repeat(float(sigma), K).astype(dtype) if np.isscalar(sigma) else np.asarray(sigma, dtype=dtype)
    h.Phi = Phi64.astype(dtype)
    h.Phi_moe = np.vstack((np.ones(N, dtype=dtype), h.Phi))
    h.Pr_b = h.Phi.sum(axis=1) / N
    np.random.seed(random_state)
    h.Z_orig = pca.T.astype(dtype)
    h.Z_corr = h.Z_orig.copy()
    Z_cos = h.Z_orig / h.Z_orig.max(axis=0)
    h.Z_cos = Z_cos / np.sqrt((Z_cos * Z_cos).sum(axis=0))
    h.objective_harmony, h.objective_kmeans, h.kmeans_rounds = [], [], []
    h.ratios_harmony, h.ratios_kmeans = [], []
    # the start
    Y = kmeans_centroids(h.Z_cos, K, random_state) if init_centroids is None else np.asarray(init_centroids, dtype=np.float64)
    Y = Y / np.sqrt((Y * Y).sum(axis=0))                # (float64 in every mode: the device is handed these bits)
    h.Y = Y.astype(dtype)
    h.dist = _dist(h)
    R = -h.dist / h.sigma[:, None]
    R = np.exp(R - R.max(axis=0))
    h.R = R / R.sum(axis=0)
    h.E = np.outer(h.R.sum(axis=1), h.Pr_b)
    h.O = h.R @ h.Phi.T
    h.objective_kmeans.append(_objective(h))
    h.objective_harmony.append(h.objective_kmeans[-1])
    for _ in range(max_iter_harmony):
        _cluster(h, max_iter_kmeans, epsilon_cluster, block_size)
        _ridge(h)
        old, new = h.objective_harmony[-2], h.objective_harmony[-1]
        ratio = (old - new) / abs(old)
        h.ratios_harmony.append(float(ratio))
        if ratio < epsilon_harmony:
            break
    return h


def threshold_margin(h, epsilon_cluster=1e-5, epsilon_harmony=1e-4):
    """the smallest relative distance of a convergence ratio of the run from the threshold it was compared with"""
    m = [abs(r - epsilon_cluster) / epsilon_cluster for r in h.ratios_kmeans]
    m += [abs(r - epsilon_harmony) / epsilon_harmony for r in h.ratios_harmony]
    return min(m) if m else np.inf


def make_case(N, d, levels, seed, shift=1.0, singleton=False):
    """PCA-like scores [N][d] with a few loose groups and a per-batch shift, and an obs frame with one column per
    variable (``levels``: the number of levels of each).  ``singleton``: the last level of the first variable is held
    by exactly one cell."""
    rs = np.random.RandomState(seed)
    groups = rs.randint(0, 4, size=N)
    centers = rs.randn(4, d) * 3
    scale = 1.0 / np.sqrt(1 + np.arange(d))
    pca = (centers[groups] + rs.randn(N, d)) * scale
    obs = {}
    for v, L in enumerate(levels):
        lv = rs.randint(0, L, size=N)
        lv[:L] = np.arange(L)                           # every level occurs
        if singleton and v == 0:
            lv[lv == L - 1] = 0
            lv[N // 2] = L - 1
        obs["var%d" % v] = pd.Categorical(["l%d" % x for x in lv])
        pca = pca + shift * rs.randn(L, d)[lv] * scale
    return pca, pd.DataFrame(obs, index=["cell%d" % i for i in range(N)])


def make_two_batches(N, d, seed, shift=4.0):
    """three cell groups present in both batches; the second batch is shifted along component 1"""
    rs = np.random.RandomState(seed)
    groups = rs.randint(0, 3, size=N)
    batch = rs.randint(0, 2, size=N)
    centers = rs.randn(3, d) * 4
    pca = centers[groups] + rs.randn(N, d)
    pca[:, 1] += shift * batch
    obs = pd.DataFrame({"batch": pd.Categorical(["b%d" % b for b in batch])}, index=["cell%d" % i for i in range(N)])
    return pca, obs, batch


def batch_gap(Z, batch):
    """distance between the two batch centroids of Z [d][N]"""
    Z = np.asarray(Z, dtype=np.float64)
    return float(np.linalg.norm(Z[:, batch == 0].mean(axis=1) - Z[:, batch == 1].mean(axis=1)))
