"""Host references for the mutual-information tests (test_gpu_select_mi.py, test_gpu_select_mi_edges.py,
test_host_mi_reference.py): sklearn's own scaling, noise and `_compute_mi_cd`, evaluated on the host."""
import numpy as np


def assert_state_equal(a, b):
    assert a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
    assert (int(a[2]), int(a[3])) == (int(b[2]), int(b[3]))
    assert np.float64(a[4]).view(np.uint64) == np.float64(b[4]).view(np.uint64)


def host_noise(X, state, perturb=None):
    """sklearn's _estimate_mi scaling and noise on the host from ``state``, as it writes them (X[:, mask] is a
    column-major copy, which sets numpy's summation order).  ``perturb``: an int8 array of X's shape, -1 / 0 / +1 ulp
    added to every standard-normal draw before it is used (what a log() one ulp off the host's does to the noise)."""
    from sklearn.preprocessing import scale
    rs = np.random.RandomState()
    rs.set_state(state)
    X = X.astype(np.float64, copy=True)
    mask = np.ones(X.shape[1], dtype=bool)
    X[:, mask] = scale(X[:, mask], with_mean=False, copy=False)
    means = np.maximum(1, np.mean(np.abs(X[:, mask]), axis=0))
    z = rs.standard_normal(size=X.shape)
    if perturb is not None:
        z = (z.view(np.int64) + perturb.astype(np.int64)).view(np.float64)
    X[:, mask] += 1e-10 * means * z
    return X, rs.get_state()


def psi_table(n):
    """digamma(0..n) with psi[0] = 0, the table Engine.preprocess_select_mi takes"""
    from scipy.special import digamma
    psi = digamma(np.arange(n + 1, dtype=np.float64))
    psi[0] = 0.0
    return psi


def sklearn_mi(Xn, labels, n_neighbors, picks):
    """max(0, _compute_mi_cd) of the noisy columns ``picks``: what mutual_info_classif returns for them"""
    from sklearn.feature_selection._mutual_info import _compute_mi_cd
    return np.array([max(0, _compute_mi_cd(Xn[:, j], labels, n_neighbors)) for j in picks], dtype=np.float64)


def device_mi(engine, X, labels, n_neighbors, state):
    """Engine.preprocess_select_mi over X with the class terms of ``labels``: (mi [G], the final RandomState state)"""
    from cnmf_amd.preprocess import mi_classes
    cls, n_cls, cst = mi_classes(labels, n_neighbors)
    engine.preprocess_set_dense(0, X)
    try:
        return engine.preprocess_select_mi(0, cls, n_cls, n_neighbors, state, psi_table(X.shape[0]), cst)
    finally:
        engine.preprocess_release()
