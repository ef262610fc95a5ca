"""``Engine.mu_frobenius_refit`` (cnmf_mu2_refit_f64: scikit-learn's multiplicative Frobenius update with the spectra
fixed, float64) on the device against the numpy restatement tests/_mu_frobenius_ref.py, which
tests/test_host_mu_frobenius.py holds to live scikit-learn.

Data: tests/_mu_frobenius_ref.planted -- Poisson counts over a planted W H divided by the genes' std, one all-zero gene,
one all-zero cell, one zero in H -- uploaded through ``set_matrix`` dense and as CSR.  The reference of every comparison
is the restatement run on ``engine.get_matrix().astype(float64)`` from the engine's own start value.  Shapes (N, G, k):
(67, 20, 3), (130, 37, 5), (200, 64, 9); (65, 20, 1) and (129, 37, 33), one row past a workgroup of 64; (70, 150, 128), the
largest rank (two LDS strips of 64 KB).

Required: ``n_iter`` equal; |W - W_ref| <= 16 max(d_self, 2^-52 max|W_ref|) with d_self the restatement's float64 versus
``np.longdouble`` distance; ``err`` within 16 x its own d_self.  The factor is the one of tests/test_gpu_hvg*.py.  Input
guard, on the restatement: every evaluated (previous - error) / error_at_start lies at least 1e-9 from tol.

Measured on an MI355X, one run (max abs difference device vs restatement / restatement vs long double = ratio; dense and
CSR uploads gave the same figures):

  shape            n_iter   W                            err
  (67, 20, 3)        40     1.6e-15 / 1.1e-15 = 1.44     7.1e-15 / 1.5e-15 = 4.71
  (130, 37, 5)       40     1.4e-15 / 2.1e-15 = 0.67     1.4e-14 / 7.3e-15 = 1.95
  (200, 64, 9)       60     4.2e-15 / 3.6e-15 = 1.18     8.5e-14 / 1.5e-14 = 5.58
  (65, 20, 1)        20     4.4e-16 / 1.4e-15 = 0.32     7.1e-15 / 4.3e-15 = 1.65
  (129, 37, 33)     180     1.4e-14 / 1.3e-14 = 1.03     0       / 7.5e-14
  (70, 150, 128)    240     1.7e-14 / 1.5e-14 = 1.14     9.7e-13 / 4.5e-13 = 2.14
  (130, 37, 5) with l1 / l1 + l2 / l2 / max_iter=25 / tol=0, max_iter=7: W 1.04 / 1.09 / 0.97 / 0.90 / 1.20, err equal bits

The closest any check of the restatement came to tol: 6.8e-7 (l1 + l2), 4.0e-6 on the default runs."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd.engine import regularization
from tests import _mu_frobenius_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHAPES = [(67, 20, 3), (130, 37, 5), (200, 64, 9), (65, 20, 1), (129, 37, 33), (70, 150, 128)]
OPTION_SHAPE = (130, 37, 5)
OPTIONS = {
    "l2": dict(alpha_W=0.05, l1_ratio=0.0),
    "l1_l2": dict(alpha_W=0.05, l1_ratio=0.5),
    "l1": dict(alpha_W=0.05, l1_ratio=1.0),
    "max_iter_25": dict(max_iter=25),
    "tol_0_max_iter_7": dict(tol=0.0, max_iter=7),
}
_inputs, _refs = {}, {}


def inputs(shape):
    if shape not in _inputs:
        N, G, k = shape
        X, H = R.planted(N, G, k, seed=100 + k)
        assert not X[:, 1 % G].any() and not X[2].any() and (H == 0).sum() == 1
        _inputs[shape] = (X, H)
    return _inputs[shape]


def upload(engine, shape, sparse):
    X, H = inputs(shape)
    engine.set_matrix(sp.csr_matrix(X) if sparse else X)
    return engine.get_matrix().astype(np.float64), H


def reference(Xres, H, w_init, shape, **kw):
    """The restatement in float64 and long double on the resident matrix, computed once per (shape, options)."""
    key = (shape, tuple(sorted(kw.items())))
    hit = _refs.get(key)
    if hit is not None and np.array_equal(hit[0], Xres) and hit[1] == w_init:
        return hit[2]
    N, G, _ = shape
    tol, max_iter = kw.get("tol", 1e-4), kw.get("max_iter", 1000)
    l1, _, l2, _ = regularization(N, G, kw.get("alpha_W", 0.0), 0.0, kw.get("l1_ratio", 0.0))
    W, n, errs = R.mu_frobenius_refit(Xres, H, w_init=w_init, tol=tol, max_iter=max_iter, l1=l1, l2=l2)
    W_ld, n_ld, errs_ld = R.mu_frobenius_refit(Xres, H, w_init=LD(w_init), tol=tol, max_iter=max_iter, l1=l1, l2=l2, dtype=LD)
    assert n == n_ld
    margins = R.stop_margins(errs, tol)
    assert all(m >= 1e-9 for m in margins), margins               # the input guard
    out = dict(W=W, n_iter=n, err=float(errs[-1]), d_W=float(np.abs(W.astype(LD) - W_ld).max()),
               d_err=float(abs(LD(errs[-1]) - errs_ld[-1])), margin=min(margins, default=np.inf))
    _refs[key] = (Xres, w_init, out)
    return out


def check(engine, shape, sparse, label, **kw):
    Xres, H = upload(engine, shape, sparse)
    w_init = engine.init_scale(H.shape[0])
    ref = reference(Xres, H, w_init, shape, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W, n_iter, err = engine.mu_frobenius_refit(H, **kw)
    dW, de = float(np.abs(W - ref["W"]).max()), abs(err - ref["err"])
    bound_W = 16 * max(ref["d_W"], 2.0 ** -52 * float(np.abs(ref["W"]).max()))
    print("%s %s %s: n_iter %d / %d; W device vs restatement %.3e, restatement vs long double %.3e (%.2f x); err %.3e, "
          "%.3e (%.2f x); closest check to tol %.3e" % (label, shape, "csr" if sparse else "dense", n_iter, ref["n_iter"], dW,
                                                        ref["d_W"], dW / ref["d_W"] if ref["d_W"] else np.inf, de, ref["d_err"],
                                                        de / ref["d_err"] if ref["d_err"] else np.inf, ref["margin"]))
    assert W.shape == (shape[0], shape[2]) and W.dtype == np.float64
    assert n_iter == ref["n_iter"]
    assert dW <= bound_W
    assert de <= 16 * ref["d_err"]
    assert not W[2].any() and np.isfinite(W).all() and W.min() >= 0
    return W, n_iter, err


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_matches_the_restatement(engine, shape, sparse):
    check(engine, shape, sparse, "default")


@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_options_match_the_restatement(engine, option):
    kw = OPTIONS[option]
    _, n_iter, _ = check(engine, OPTION_SHAPE, False, option, **kw)
    if "max_iter" in kw:
        assert n_iter == kw["max_iter"]


def test_two_calls_give_the_same_bits(engine):
    _, H = upload(engine, (200, 64, 9), True)
    a = engine.mu_frobenius_refit(H)
    b = engine.mu_frobenius_refit(H)
    assert a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


def test_convergence_warning_as_mu_refit_f64(engine):
    from cnmf_amd.engine import ConvergenceWarning
    _, H = upload(engine, (67, 20, 3), False)
    with pytest.warns(ConvergenceWarning, match="Maximum number of iterations 10 reached"):
        engine.mu_frobenius_refit(H, tol=1e-12, max_iter=10)


def test_rank_above_kmax_is_refused(engine):
    upload(engine, (67, 20, 3), False)
    H = np.random.RandomState(0).uniform(size=(129, 20))
    with pytest.raises(NotImplementedError):
        engine.mu_frobenius_refit(H)


def test_bad_spectra_raise_as_mu_refit_f64(engine):
    _, H = upload(engine, (67, 20, 3), False)
    with pytest.raises(ValueError, match="Array with wrong shape passed to NMF"):
        engine.mu_frobenius_refit(H[:, :-1])
    bad = H.copy()
    bad[1, 3] = -1.0
    with pytest.raises(ValueError, match="Negative values in data passed to NMF"):
        engine.mu_frobenius_refit(bad)
    with pytest.raises(ValueError, match="full of zeros"):
        engine.mu_frobenius_refit(np.zeros_like(H))
    with pytest.raises(ValueError, match="NaN or infinity"):
        engine.mu_frobenius_refit(np.where(H == H.max(), np.nan, H))


def test_the_other_mu_entry_points_still_refuse_frobenius(engine):
    _, H = upload(engine, (67, 20, 3), False)
    with pytest.raises(NotImplementedError):
        engine.mu_refit_f64(H, beta_loss="frobenius")
    with pytest.raises(NotImplementedError):
        engine.nmf_mu_batch([3], seeds=[1], beta_loss="frobenius")
