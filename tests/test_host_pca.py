"""The host half of the PCA through the tridiagonal form, without a GPU: the numpy restatement of the device algorithm
(tests/_tridiag_ref.py: plain and deferred-update form) against LAPACK, ``preprocess.tridiagonal_top`` with the
restated back-transformation against the three contracts, and the validation of the ``pca`` argument."""
import numpy as np
import pytest

from cnmf_amd import preprocess as pp
from tests import _tridiag_ref as ref

F = ref.DEVICE_FACTOR
CASES = ref.cases()


@pytest.mark.parametrize("n", ref.RANDOM_SIZES)
def test_plain_and_deferred_forms_agree_and_reproduce_lapack(n):
    A = ref.random_symmetric(n, 100 + n, zero_tail=(n == 17))
    u = ref.unit(A)
    d0, e0, R0, tau0 = ref.tridiag_plain(A)
    d1, e1, R1, tau1 = ref.tridiag_deferred(A)
    if n == 17:
        assert tau0[0] == 0.0 and tau1[0] == 0.0 and e0[0] == A[1, 0] and e1[0] == A[1, 0]
    assert np.abs(d0 - d1).max() <= F * u and np.abs(e0 - e1).max() <= F * u
    want = np.linalg.eigvalsh(A)
    for d, e in ((d0, e0), (d1, e1)):
        assert np.abs(ref.tridiagonal_eigvals(d, e) - want).max() <= F * u


@pytest.mark.parametrize("form", ["plain", "deferred"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_tridiagonal_top_and_back_transform_meet_the_contracts(case, form):
    name, A, k = CASES[case]
    d, e, R, tau = (ref.tridiag_plain if form == "plain" else ref.tridiag_deferred)(A)
    w, Z = pp.tridiagonal_top(d, e, k)
    assert w.shape == (k,) and Z.shape == (A.shape[0], k)
    V = ref.back_transform(R, tau, Z, rule=True)
    res, eig, orth, desc = ref.contracts(A, w, V)
    print("%s %s: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (name, form, res, eig, orth))
    assert res <= F and eig <= F and orth <= F and desc
    lead = V[np.argmax(np.abs(V), axis=0), np.arange(k)]
    assert (lead > 0).all()


def test_back_transform_of_the_identity_is_the_orthogonal_factor():
    A = ref.random_symmetric(17, 5)
    d, e, R, tau = ref.tridiag_deferred(A)
    Q = ref.back_transform(R, tau, np.eye(17))
    n, u = 17, ref.unit(A)
    assert np.abs(Q.T @ Q - np.eye(n)).max() <= F * n * ref.EPS
    assert np.abs(Q.T @ A @ Q - ref.tridiagonal_matrix(d, e)).max() <= F * u


def test_tridiagonal_top_refuses_non_finite_input_and_bad_shapes():
    d, e = np.arange(4.0), np.ones(3)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            pp.tridiagonal_top(np.r_[d[:3], bad], e, 2)
        with pytest.raises(ValueError, match="non-finite"):
            pp.tridiagonal_top(d, np.r_[bad, e[1:]], 2)
    with pytest.raises(ValueError):
        pp.tridiagonal_top(d, e[:2], 2)
    with pytest.raises(ValueError):
        pp.tridiagonal_top(d, e, 5)
    w, Z = pp.tridiagonal_top(np.array([3.0]), np.zeros(0), 1)
    assert w.tolist() == [3.0] and Z.tolist() == [[1.0]]


def test_pca_argument_is_validated_before_any_device_work():
    """fails on a tree without the feature: there is no such argument"""
    P = pp.Preprocess()                                   # (the engine is created on first use: none here)
    X = np.ones((4, 3))
    with pytest.raises(ValueError, match="pca must be one of"):
        P.normalize_batchcorrect(X, highly_variable=np.ones(3, dtype=bool), pca="bogus")
    with pytest.raises(ValueError, match="pca must be one of"):
        P.preprocess_for_cnmf(X, highly_variable=np.ones(3, dtype=bool), pca="bogus")
    assert P._engine is None
    with pytest.raises(NotImplementedError, match='pca="lapack"'):
        pp._check_pca_size("device", pp.PCA_NMAX + 1)
    pp._check_pca_size("lapack", pp.PCA_NMAX + 1)
    pp._check_pca_size("device", pp.PCA_NMAX)
