"""numpy restatement of the multiplicative-update Frobenius refit (scikit-learn 1.7.2 ``_fit_multiplicative_update`` with
``beta_loss=2, update_H=False``) as ``cnmf_mu2_refit_f64`` states it: the constants P = X H^T, Gram = H H^T and
nX = sum x^2 once; W = w_init everywhere; per iteration ``W *= P / (W Gram + l1 + l2 W)`` with a zero denominator replaced
by float32 epsilon, every denominator from the OLD W; the error ``sqrt(nX + sum W (W Gram) - 2 sum P W)`` (scikit-learn's
expansion for a sparse X, not clamped) at the start and after every 10th iteration when ``tol > 0``; stop when
``(previous - error) / error_at_start < tol``.  ``dtype``: float64 or ``np.longdouble`` (the yardstick of the tolerances)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def mu_frobenius_refit(X, H, w_init=None, tol=1e-4, max_iter=1000, l1=0.0, l2=0.0, dtype=np.float64):
    """Returns ``(W [N, k], n_iter, errors)``: ``errors`` = every error evaluated, the one at the start first."""
    X = np.asarray(X, dtype=dtype)
    H = np.asarray(H, dtype=dtype)
    N, k = X.shape[0], H.shape[0]
    P = X @ H.T
    gram = H @ H.T
    nX = (X * X).sum()
    if w_init is None:
        w_init = np.sqrt(X.mean() / k)
    W = np.full((N, k), w_init, dtype=dtype)

    def error(W):
        return np.sqrt(nX + (W * (W @ gram)).sum() - 2 * (P * W).sum())

    errors = [error(W)]
    err0 = prev = errors[0]
    n_iter = 0
    for it in range(1, max_iter + 1):
        den = W @ gram
        if l1 > 0:
            den = den + dtype(l1)
        if l2 > 0:
            den = den + dtype(l2) * W
        den[den == 0] = dtype(EPS32)
        W = W * (P / den)
        n_iter = it
        if tol > 0 and it % 10 == 0:
            err = error(W)
            errors.append(err)
            if (prev - err) / err0 < tol:
                break
            prev = err
    return W, n_iter, errors


def stop_margins(errors, tol):
    """|(previous - error) / error_at_start - tol| of every check the run made (the last one included)."""
    e = [float(v) for v in errors]
    return [abs((e[i - 1] - e[i]) / e[0] - tol) for i in range(1, len(e))]


def planted(N, G, k, seed, dtype=np.float64):
    """Poisson counts over a planted W H, every gene divided by its ddof=1 std (a gene of zero variance left as it is);
    gene 1 and cell 2 all zero; ``H`` (non-negative, one exact zero) to refit against.  Returns ``(X, H)``."""
    rs = np.random.RandomState(seed)
    Wp = rs.gamma(1.0, 1.0, size=(N, k))
    Hp = rs.gamma(0.5, 1.0, size=(k, G))
    X = rs.poisson(Wp @ Hp + 0.2).astype(np.float64)
    X[:, 1 % G] = 0.0
    X[2 % N, :] = 0.0
    std = X.std(axis=0, ddof=1)
    X = X / np.where(std == 0, 1.0, std)
    H = Hp * rs.uniform(0.5, 1.5, size=Hp.shape)
    H[0, (G - 1) // 2] = 0.0
    return X.astype(dtype), H
