"""The device tail of init='nndsvd', restated in numpy (tests/_nndsvd_tail_ref.py: Hestenes sweeps, then the steps of
_nndsvd_finish), against ``_nndsvd_finish`` itself; the host variants 'nndsvda' / 'nndsvdar' against scikit-learn's
``_initialize_nmf``; and what ``cNMF._check_kwargs`` lets through.  The range finder is scikit-learn's -- no device."""
import numpy as np
import pytest
from sklearn.decomposition._nmf import _initialize_nmf
from sklearn.utils.extmath import randomized_range_finder

from tests._nndsvd_tail_ref import hestenes_svd, round_robin, tail_ref

SHAPES = [((300, 60), 5, 3), ((60, 300), 4, 11), ((200, 200), 7, 42), ((90, 40), 6, 0), ((1100, 257), 1, 1),
          ((1100, 257), 2, 2), ((700, 300), 118, 5), ((150, 260), 9, 7)]


def make_x(shape, seed):
    rs = np.random.RandomState(seed + 100)
    return rs.gamma(0.6, 1.0, shape) * (rs.uniform(size=shape) < 0.7)


def sklearn_qb(X, k, seed):
    """Q, B of scikit-learn's own range finder, rounded to float32 (what the device hands its tail), and `transpose`."""
    transpose = X.shape[0] < X.shape[1]
    M = X.T if transpose else X
    n_iter = 7 if k < 0.1 * min(X.shape) else 4
    Q = randomized_range_finder(M, size=k + 10, n_iter=n_iter, power_iteration_normalizer="auto", random_state=seed)
    return Q.astype(np.float32), (Q.T @ M).astype(np.float32), transpose


@pytest.mark.parametrize("c", [1, 2, 11, 12, 33, 128])
def test_round_robin_meets_every_pair_once(c):
    seen = set()
    for ps, qs in round_robin(c):
        rows = list(ps) + list(qs)
        assert len(set(rows)) == len(rows)                       # the pairs of a round are disjoint
        assert (ps < qs).all() and (qs < c).all()
        seen |= set(zip(ps.tolist(), qs.tolist()))
    assert len(seen) == c * (c - 1) // 2


@pytest.mark.parametrize("shape,k,seed", SHAPES)
def test_restatement_matches_nndsvd_finish(shape, k, seed):
    from cnmf_amd.engine import _nndsvd_finish
    X = make_x(shape, seed)
    Q, B, transpose = sklearn_qb(X, k, seed)
    W_ref, H_ref = _nndsvd_finish(k, Q, B, transpose)
    W, H, info = tail_ref(k, Q, B, transpose)
    assert info["converged"] and info["sweeps"] <= 12
    assert W.shape == W_ref.shape and H.shape == H_ref.shape
    assert np.abs(W - W_ref).max() <= 1e-10 * np.abs(W_ref).max()
    assert np.abs(H - H_ref).max() <= 1e-10 * np.abs(H_ref).max()
    # and its long-double run stays as close: the yardstick of the device test
    Wl, Hl, _ = tail_ref(k, Q, B, transpose, dtype=np.longdouble)
    assert np.abs(W - Wl).max() <= 1e-10 * np.abs(W_ref).max()
    assert np.abs(H - Hl).max() <= 1e-10 * np.abs(H_ref).max()


def test_restatement_svd_is_an_svd():
    rs = np.random.RandomState(0)
    B = rs.standard_normal((13, 70))
    S, VT, J, sweeps, conv = hestenes_svd(B)
    assert conv and (np.diff(S) <= 0).all()
    assert np.abs(J.T @ (S[:, None] * VT) - B).max() <= 1e-13 * S[0]
    assert np.abs(J @ J.T - np.eye(13)).max() <= 1e-13
    assert np.abs(S - np.linalg.svd(B, compute_uv=False)).max() <= 1e-13 * S[0]


@pytest.mark.parametrize("variant", ["nndsvda", "nndsvdar"])
@pytest.mark.parametrize("shape,k,seed", [((300, 60), 5, 3), ((60, 300), 4, 11), ((90, 40), 6, 0)])
def test_host_variants_match_sklearn(variant, shape, k, seed):
    from cnmf_amd.engine import _nndsvd_fill, _nndsvd_finish
    X = make_x(shape, seed)
    W_ref, H_ref = _initialize_nmf(X, k, init=variant, random_state=seed)
    transpose = X.shape[0] < X.shape[1]
    M = X.T if transpose else X
    n_iter = 7 if k < 0.1 * min(X.shape) else 4
    Q = randomized_range_finder(M, size=k + 10, n_iter=n_iter, power_iteration_normalizer="auto", random_state=seed)
    W, H = _nndsvd_finish(k, Q, Q.T @ M, transpose)
    assert (W == 0).any() and (H == 0).any()                     # there is something to fill
    W, H = _nndsvd_fill(W, H, variant, X.mean(), seed)
    assert (W > 0).all() and (H > 0).all()
    assert np.abs(W - W_ref).max() <= 1e-10 * np.abs(W_ref).max()
    assert np.abs(H - H_ref).max() <= 1e-10 * np.abs(H_ref).max()


def test_fill_refuses_an_unknown_variant():
    from cnmf_amd.engine import _nndsvd_fill
    with pytest.raises(ValueError):
        _nndsvd_fill(np.zeros((3, 2)), np.zeros((2, 4)), "nndsvdx", 1.0, 0)


def test_check_kwargs_accepts_the_variants(tmp_path):
    from cnmf_amd.cnmf import cNMF
    obj = cNMF.__new__(cNMF)
    for init in ("random", "nndsvd", "nndsvda", "nndsvdar"):
        obj._check_kwargs(dict(solver="cd", beta_loss="frobenius", init=init))
        obj._check_kwargs(dict(solver="mu", beta_loss="kullback-leibler", init=init))
    with pytest.raises(NotImplementedError):
        obj._check_kwargs(dict(solver="cd", beta_loss="frobenius", init="nndsvdx"))
    assert cNMF.nndsvd == "host"
