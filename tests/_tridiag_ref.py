"""Host side of the PCA-through-the-tridiagonal-form tests (test_host_pca.py, test_gpu_pca.py): a sequential float64
numpy restatement of csrc/pca_host.hip.h -- the yardstick for its step order and its reflector convention --, the test
matrices and the three gap-free contracts.

The restatement has two forms.  ``tridiag_plain`` is the textbook algorithm (LAPACK's dsytd2, lower form): per column
the reflector, p = tau A22 v, w = p - (tau / 2)(p^T v) v, A22 -= v w^T + w v^T.  ``tridiag_deferred`` is what the
kernel does, one step per launch: step k first forms w_{k-1} from the RAW product p_{k-1} = A22 v_{k-1} of the step
before, reads row k as the pending update leaves it, derives v_k from it, and only then applies the pending update to
the rows behind k and forms p_k.  Both return (d, e, R, tau): R[k, k+1:] is the reflector of column k with its leading
1 stored.

Tolerance unit of a matrix A: u = n eps |A|_inf with eps = 2^-52.  Contracts for (w, V) against A: the residual
max |A V - V diag(w)| and the eigenvalue error max |w - w_lapack| in units of u, the orthogonality max |V^T V - I| in
units of n eps.  The device is given 8 of each (the O(n eps) backward-error bound of Householder reduction, the factor
for its other summation order and FMA contraction); this restatement shows at most 0.46 u and 2.5 n eps on the cases
here (test_host_pca.py prints them)."""
import numpy as np

EPS = 2.0 ** -52
DEVICE_FACTOR = 8.0


def unit(A):
    A = np.asarray(A)
    return A.shape[0] * EPS * np.abs(A).sum(axis=1).max()


def reflector(x):
    """dlarfg on x (length >= 1): (v with v[0] = 1, tau, beta)"""
    alpha = x[0]
    v = np.zeros(x.size)
    v[0] = 1.0
    if x.size < 2:
        return v, 0.0, alpha
    x2 = np.sum(x[1:] * x[1:])
    if x2 == 0.0:
        return v, 0.0, alpha
    beta = -np.copysign(np.hypot(alpha, np.sqrt(x2)), alpha)
    v[1:] = x[1:] / (alpha - beta)
    return v, (beta - alpha) / beta, beta


def tridiag_plain(A):
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    d, e, tau, R = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(n), np.zeros((n, n))
    for k in range(n - 1):
        d[k] = A[k, k]
        v, tau[k], e[k] = reflector(A[k, k + 1:])
        R[k, k + 1:] = v
        if tau[k] != 0.0:
            p = A[k + 1:, k + 1:] @ v
            w = tau[k] * p - 0.5 * tau[k] * (tau[k] * (p @ v)) * v
            A[k + 1:, k + 1:] -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = A[n - 1, n - 1]
    return d, e, R, tau


def tridiag_deferred(A):
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    d, e, tau, R = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(n), np.zeros((n, n))
    p = np.zeros(n)
    for k in range(n):                                   # one launch
        taup = tau[k - 1] if k > 0 else 0.0
        pend = taup != 0.0
        w = np.zeros(n - k)
        if pend:                                         # (a) w_{k-1} over the rows k ..
            vp = R[k - 1, k:]
            c = 0.5 * taup * (taup * (p[k:] @ vp))
            w = taup * p[k:] - c * vp
        row = A[k, k:].copy()                            # (b) row k as the pending update leaves it (read only)
        if pend:
            row -= vp[0] * w + w[0] * vp
        d[k] = row[0]
        v = np.zeros(0)
        if n - k >= 2:                                   # (c)
            v, tau[k], e[k] = reflector(row[1:])
            R[k, k + 1:] = v
        if pend:                                         # the rows behind k: the pending update, then p_k
            A[k + 1:, k + 1:] -= np.outer(vp[1:], w[1:]) + np.outer(w[1:], vp[1:])
        p = np.zeros(n)
        p[k + 1:] = A[k + 1:, k + 1:] @ v
    return d, e, R, tau


def sign_rule(V):
    lead = V[np.argmax(np.abs(V), axis=0), np.arange(V.shape[1])]
    return V * np.where(lead < 0, -1.0, 1.0)


def back_transform(R, tau, Z, rule=False):
    """Q Z: for k = n-3 .. 0, z[k+1:] -= tau_k v_k (v_k^T z[k+1:])"""
    Z = np.array(Z, dtype=np.float64)
    n = Z.shape[0]
    for k in range(n - 3, -1, -1):
        if tau[k] != 0.0:
            v = R[k, k + 1:]
            Z[k + 1:] -= tau[k] * np.outer(v, v @ Z[k + 1:])
    return sign_rule(Z) if rule else Z


def tridiagonal_matrix(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def tridiagonal_eigvals(d, e):
    from scipy.linalg import eigvalsh_tridiagonal
    return np.array(d, dtype=np.float64) if len(d) == 1 else eigvalsh_tridiagonal(d, e)


# ---------------------------------------------------------------- the test matrices
def random_symmetric(n, seed, zero_tail=False):
    B = np.random.RandomState(seed).randn(n, n)
    A = B + B.T
    if zero_tail:                                        # column 0 is tridiagonal already: tau_0 = 0
        A[0, 2:] = 0.0
        A[2:, 0] = 0.0
    return A


def poisson_counts(N, n, seed):
    """scaled Poisson counts [N][n] (every column at unit ddof=1 variance, as the PCA's input is)"""
    rs = np.random.RandomState(seed)
    lam = rs.gamma(0.6, 2.0, size=(1, n)) + 0.05
    lib = rs.lognormal(0.0, 0.4, size=(N, 1))
    X = rs.poisson(lib * lam).astype(np.float64)
    X[0] += 1.0                                          # (no constant column)
    return X / X.std(axis=0, ddof=1)


def scatter_of(X):
    D = X - X.mean(axis=0)
    return D.T @ D


def clustered(seed=7):
    """n = 65: eigenvalues 3 (x 5), 3 (1 + 1e-13) (x 5), 20 values from 2 to 1 and 35 zeros under a random orthogonal
    basis"""
    lam = np.r_[np.full(5, 3.0), np.full(5, 3.0 * (1 + 1e-13)), np.linspace(2.0, 1.0, 20), np.zeros(35)]
    Q, _ = np.linalg.qr(np.random.RandomState(seed).randn(65, 65))
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


RANDOM_SIZES = (2, 3, 4, 17, 130)                        # (the restatement's own test; 17: zero tail in row 0)


def cases():
    """(name, A, n_comps): the smallest that reach every branch of the kernels"""
    rs = np.random.RandomState(11)
    tri = tridiagonal_matrix(rs.randn(33), rs.randn(32))
    return [
        ("n1", np.array([[2.5]]), 1),
        ("n2", random_symmetric(2, 1), 2),
        ("n3", random_symmetric(3, 2), 3),
        ("n17_zero_tail", random_symmetric(17, 3, zero_tail=True), 6),
        ("n65_poisson", scatter_of(poisson_counts(300, 65, 4)), 50),
        ("n257_poisson", scatter_of(poisson_counts(300, 257, 5)), 50),
        ("n130_rank39", scatter_of(poisson_counts(40, 130, 6)), 39),
        ("n65_clustered", clustered(), 30),
        ("diagonal", np.diag(rs.randn(20)), 7),
        ("zero", np.zeros((9, 9)), 4),
        ("tridiagonal", tri, 10),
    ]


def contracts(A, w, V):
    """(residual / u, eigenvalue error / u, orthogonality / (n eps), w descending?) of (w, V) against A; a zero u (the
    zero matrix) asks for exact zeros: 0 / 0 counts as 0, x / 0 as inf"""
    A = np.asarray(A, dtype=np.float64)
    n, k = A.shape[0], len(w)
    u = unit(A)
    res = np.abs(A @ V - V * w).max()
    eig = np.abs(w - np.linalg.eigvalsh(A)[::-1][:k]).max()
    orth = np.abs(V.T @ V - np.eye(k)).max() / (n * EPS)

    def ratio(x):
        return x / u if u > 0 else (0.0 if x == 0 else np.inf)
    return ratio(res), ratio(eig), orth, bool(np.all(np.diff(w) <= 0))
