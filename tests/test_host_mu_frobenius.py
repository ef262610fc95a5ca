"""The numpy restatement of the multiplicative Frobenius refit (tests/_mu_frobenius_ref.py: the yardstick of
tests/test_gpu_mu_frobenius.py) against live scikit-learn: ``non_negative_factorization(solver='mu',
beta_loss='frobenius', update_H=False)`` on dense and CSR input.  CPU only.

Required: the same ``n_iter`` and W within 16 x the restatement's distance from its own ``np.longdouble`` run.  Data:
tests/_mu_frobenius_ref.planted at 60 x 25, k = 4 (a zero gene, a zero cell, a zero in H)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd.engine import regularization
from tests import _mu_frobenius_ref as R

LD = np.longdouble
N, G, K = 60, 25, 4
CASES = {
    "plain": dict(),
    "l2": dict(alpha_W=0.05, l1_ratio=0.0),
    "l1_l2": dict(alpha_W=0.05, l1_ratio=0.5),
    "l1": dict(alpha_W=0.05, l1_ratio=1.0),
    "max_iter_25": dict(max_iter=25),
    "tol_0_max_iter_7": dict(tol=0.0, max_iter=7),
}


@pytest.fixture(scope="module")
def data():
    X, H = R.planted(N, G, K, seed=11)
    assert not X[:, 1].any() and not X[2].any() and (H == 0).sum() == 1
    return X, H


def sklearn_refit(X, H, tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0):
    from sklearn.decomposition import non_negative_factorization
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W, _, n_iter = non_negative_factorization(X, H=H, n_components=H.shape[0], init="custom", update_H=False, solver="mu",
                                                  beta_loss="frobenius", tol=tol, max_iter=max_iter, alpha_W=alpha_W,
                                                  l1_ratio=l1_ratio)
    return W, n_iter


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_scikit_learn(data, case, sparse):
    X, H = data
    kw = dict(tol=1e-4, max_iter=1000, alpha_W=0.0, l1_ratio=0.0)
    kw.update(CASES[case])
    l1, _, l2, _ = regularization(N, G, kw["alpha_W"], 0.0, kw["l1_ratio"])
    W, n_iter, errors = R.mu_frobenius_refit(X, H, tol=kw["tol"], max_iter=kw["max_iter"], l1=l1, l2=l2)
    W_ld, n_ld, _ = R.mu_frobenius_refit(X, H, tol=kw["tol"], max_iter=kw["max_iter"], l1=l1, l2=l2, dtype=LD)
    W_sk, n_sk = sklearn_refit(sp.csr_matrix(X) if sparse else X, H, **kw)
    d_self = float(np.abs(W.astype(LD) - W_ld).max())
    d_sk = float(np.abs(W_sk - W).max())
    print("%s %s: n_iter %d / long double %d / scikit-learn %d; restatement vs long double %.3e, scikit-learn vs restatement "
          "%.3e; checks %d, closest to tol %.3e" % (case, "csr" if sparse else "dense", n_iter, n_ld, n_sk, d_self, d_sk,
                                                   len(errors) - 1, min(R.stop_margins(errors, kw["tol"]), default=np.inf)))
    assert n_iter == n_ld == n_sk
    if kw["tol"] == 0 or kw["max_iter"] % 10:
        assert n_iter == kw["max_iter"]
    assert d_sk <= 16 * d_self
    # the zero cell stays zero, nothing is negative or non-finite
    assert not W[2].any() and np.isfinite(W).all() and W.min() >= 0


def test_errors_listed_are_the_checks_made(data):
    X, H = data
    _, n_iter, errors = R.mu_frobenius_refit(X, H, tol=1e-4, max_iter=1000)
    assert n_iter % 10 == 0 and len(errors) == 1 + n_iter // 10
    _, n7, e7 = R.mu_frobenius_refit(X, H, tol=0.0, max_iter=7)
    assert n7 == 7 and len(e7) == 1
    _, n25, e25 = R.mu_frobenius_refit(X, H, tol=1e-12, max_iter=25)
    assert n25 == 25 and len(e25) == 3
