"""Host side of the HVG tests (test_host_hvg.py, test_gpu_hvg.py): a numpy restatement of scanpy's
``highly_variable_genes(flavor='seurat_v3')`` for one batch, with skmisc's ``loess(x, y, span=0.3, degree=2)`` (family
gaussian: no robustness iterations; one dimension: no normalisation) written out, and a device-free engine whose three
HVG entry points are played by it.  **This file is the yardstick of Preprocess.highly_variable_genes**: agreement with
skmisc and scanpy themselves is unmeasured on this project's machines (neither is installed on them);
test_host_hvg.py compares this restatement with both wherever they can be imported.

Every function takes ``dtype``: float64 is the yardstick, ``np.longdouble`` the run the yardstick's own rounding error is
measured against (the tolerance rule of the Harmony tests).

Moments.  Over N cells, per gene: S1 = sum x, S2 = sum x^2 (counts are non-negative integers: both are exact),
mean = S1 / N, var = (N S2 - S1^2) / (N (N - 1)) with the numerator formed in Python integers and ONE division: the ddof=1
variance, correctly rounded, whatever the order of the sums.  Bound: every count <= 2^20 and N <= 2^22 cells, so that
S2 <= 2^62 stays an exact int64 on the device; a larger count, a negative or a non-integer value raises ValueError
(scanpy warns and goes on).

Loess over the genes with var > 0, x = log10(mean), y = log10(var); n points, q = min(n, floor(n span + 1e-5)).
A local fit at x0: h = the q-th smallest |x_i - x0| (h <= 0: ValueError, skmisc's "zero-width neighborhood"); weights
(1 - (|x_i - x0| / h)^3)^3 where |x_i - x0| < h, else 0 (a point tied at h weighs nothing); the weighted least-squares
quadratic in t = (x - x0) / h, minimum-norm solution with the singular values below 100 eps sigma_max dropped
(``np.linalg.lstsq(rcond=100 eps)`` on the sqrt(w)-scaled design); the result is the value c0 and the slope c1 / h.
surface="direct": the fitted value of point i is the local fit at x_i.  surface="interpolate" (skmisc's default): the
interval [min - mu, max + mu], mu = 0.005 max(max - min, 1e-10 max(|min|, |max|) + 1e-30); a cell holding more than
fc = floor(n span 0.2) points is cut at (x_(m) + x_(m+1)) / 2, m = (l + u) // 2 over the cell's sorted points, m moved by
+1, -1, +2, ... until x_(m) != x_(m+1) (no cut when no such m lies inside the cell or x_(m) equals an end of the cell);
the vertices are the two ends and all cuts; a local fit (value, slope) at every vertex; a point's fitted value is the
cubic Hermite interpolant of its cell (written from Cleveland and Grosse's published dloess).

Standardised variance.  est = 0 on constant genes, the fitted value elsewhere; reg_std = sqrt(10^est);
clip = reg_std sqrt(N) + mean; C1 = sum min(x, clip), C2 = sum min(x, clip)^2 (zeros contribute nothing);
variances_norm = (N mean^2 + C2 - 2 C1 mean) / ((N - 1) reg_std^2).

Ranking.  By variances_norm descending, ties in gene order (a STABLE sort: scanpy's own ``np.argsort`` leaves ties
unspecified); highly_variable = rank < n_top_genes; highly_variable_rank = the rank as float, NaN from n_top_genes on."""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from tests import _filter_ref as F

EPS = float(np.finfo(np.float64).eps)
RCOND = 100 * EPS
COUNT_MAX = 1 << 20
CELLS_MAX = 1 << 22
FLAG_NOT_COUNT, FLAG_TOO_LARGE = 1, 2
STATUS_OK, STATUS_ZERO_WIDTH, STATUS_DEFICIENT = 0, 1, 2
ZERO_WIDTH_ERROR = "loess: zero-width neighborhood; make span bigger"


# ---------------------------------------------------------------- moments
def gene_moments(X):
    """(S1 int64 [G], S2 int64 [G], flags) over a CSR as stored: flags bit 0 = a negative or non-integer value, bit 1 = a
    value above COUNT_MAX (such entries are left out of the sums)"""
    X = sp.csr_matrix(X)
    v = np.asarray(X.data, dtype=np.float64)
    bad = ~(np.isfinite(v) & (v >= 0) & (v == np.floor(v)))
    big = ~bad & (v > COUNT_MAX)
    ok = ~(bad | big)
    iv = np.where(ok, v, 0).astype(np.int64)
    G = X.shape[1]
    s1, s2 = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    np.add.at(s1, X.indices, iv)
    np.add.at(s2, X.indices, iv * iv)
    return s1, s2, (FLAG_NOT_COUNT if bad.any() else 0) | (FLAG_TOO_LARGE if big.any() else 0)


def mean_var(s1, s2, N, dtype=np.float64):
    """mean = S1 / N and the ddof=1 variance (N S2 - S1^2) / (N (N - 1)): exact integers, one division each"""
    N = int(N)
    den = N * (N - 1)
    if dtype is np.float64:
        mean = np.array([int(a) / N for a in s1], dtype=np.float64)
        var = np.array([(N * int(b) - int(a) * int(a)) / den for a, b in zip(s1, s2)], dtype=np.float64)
        return mean, var
    mean = np.array([dtype(int(a)) / dtype(N) for a in s1], dtype=dtype)
    num = [N * int(b) - int(a) * int(a) for a, b in zip(s1, s2)]
    # (a numerator beyond the long double's 64 bits: split into two exact halves)
    var = np.array([(dtype(v >> 32) * dtype(2.0 ** 32) + dtype(v & 0xffffffff)) / dtype(den) for v in num], dtype=dtype)
    return mean, var


# ---------------------------------------------------------------- loess
def loess_q(n, span):
    return int(min(n, np.floor(n * span + 1e-5)))


def _min_norm_jacobi(A, b):
    """the minimum-norm least-squares solution of A c = b with the singular values below RCOND sigma_max dropped, by a
    one-sided Jacobi SVD in A's own precision (np.linalg has no long double)"""
    dtype = A.dtype.type
    U, V = A.copy(), np.eye(A.shape[1], dtype=A.dtype)
    for _ in range(60):
        moved = False
        for i in range(A.shape[1] - 1):
            for j in range(i + 1, A.shape[1]):
                a, bb, g = U[:, i] @ U[:, i], U[:, j] @ U[:, j], U[:, i] @ U[:, j]
                if g == 0 or abs(g) <= dtype(np.finfo(A.dtype).eps) * np.sqrt(a * bb):
                    continue
                moved = True
                z = (bb - a) / (2 * g)
                t = np.sign(z) / (abs(z) + np.sqrt(1 + z * z)) if z != 0 else dtype(1)
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                U[:, i], U[:, j] = c * U[:, i] - s * U[:, j], s * U[:, i] + c * U[:, j]
                V[:, i], V[:, j] = c * V[:, i] - s * V[:, j], s * V[:, i] + c * V[:, j]
        if not moved:
            break
    sig = np.sqrt((U * U).sum(axis=0))
    keep = sig > dtype(RCOND) * sig.max()
    coef = np.zeros(A.shape[1], dtype=A.dtype)
    for k in np.flatnonzero(keep):
        coef += V[:, k] * ((U[:, k] @ b) / (sig[k] * sig[k]))
    return coef


def local_fit(x, y, x0, q, dtype=np.float64):
    """(value, slope) of the local quadratic at x0 over the points (x, y) with the q nearest weighted"""
    x, y, x0 = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), dtype(x0)
    d = np.abs(x - x0)
    h = np.partition(d, q - 1)[q - 1]
    if not h > 0:
        raise ValueError(ZERO_WIDTH_ERROR)
    use = d < h
    r = d[use] / h
    w = (1 - r * r * r) ** 3
    t = (x[use] - x0) / h
    sw = np.sqrt(w)
    A = np.stack([sw, sw * t, sw * t * t], axis=1)
    b = sw * y[use]
    if dtype is np.float64:
        coef = np.linalg.lstsq(A, b, rcond=RCOND)[0]
    else:
        coef = _min_norm_jacobi(A, b)
    return coef[0], coef[1] / h


def local_fits(x, y, x0s, q, dtype=np.float64):
    out = [local_fit(x, y, x0, q, dtype) for x0 in np.asarray(x0s, dtype=dtype)]
    return np.array([o[0] for o in out], dtype=dtype), np.array([o[1] for o in out], dtype=dtype)


def loess_vertices(xs, span):
    """the vertices of the interpolation surface over the SORTED abscissae xs: sorted, strictly increasing"""
    xs = np.asarray(xs)
    n = xs.size
    lo, hi = xs[0], xs[-1]
    mu = 0.005 * max(hi - lo, 1e-10 * max(abs(lo), abs(hi)) + 1e-30)
    fc = int(np.floor(n * span * 0.2))
    cuts = []
    todo = [(lo - mu, hi + mu, 0, n - 1)]
    while todo:
        a, b, l, u = todo.pop()
        if u - l + 1 <= fc:
            continue
        m0 = (l + u) // 2
        m = None
        for k in range(2 * (u - l + 1)):
            off = (k + 1) // 2 if k % 2 else -(k // 2)            # 0, +1, -1, +2, -2, ...
            c = m0 + off
            if l <= c and c + 1 <= u and xs[c] != xs[c + 1]:
                m = c
                break
        if m is None or xs[m] == a or xs[m] == b:
            continue
        t = (xs[m] + xs[m + 1]) / 2
        cuts.append(t)
        todo.append((a, t, l, m))
        todo.append((t, b, m + 1, u))
    return np.array(sorted([lo - mu, hi + mu] + cuts), dtype=xs.dtype), fc


def hermite(v, val, slope, x):
    """the cubic Hermite interpolant through (v, val, slope) at the points x (every x inside [v[0], v[-1]])"""
    c = np.clip(np.searchsorted(v, x, side="right") - 1, 0, v.size - 2)
    w = v[c + 1] - v[c]
    u = (x - v[c]) / w
    return ((1 - u) ** 2 * (1 + 2 * u) * val[c] + u ** 2 * (3 - 2 * u) * val[c + 1]
            + (u * (1 - u) ** 2 * slope[c] - u ** 2 * (1 - u) * slope[c + 1]) * w)


def loess_fitted(x, y, span=0.3, surface="interpolate", dtype=np.float64, fits=local_fits):
    """the fitted values of loess(x, y, span, degree=2) at the points themselves; ``fits(xs, ys, x0s, q, dtype)`` does the
    local fits (the device plays it in Preprocess)"""
    if surface not in ("interpolate", "direct"):
        raise ValueError("surface must be 'interpolate' or 'direct', not %r" % (surface,))
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    q = loess_q(x.size, span)
    if q < 1:
        raise ValueError("span = %g leaves no point in a neighbourhood of %d" % (span, x.size))
    if surface == "direct":
        fitted_sorted = fits(xs, ys, xs, q, dtype)[0]
    else:
        v, _ = loess_vertices(xs, span)
        val, slope = fits(xs, ys, v, q, dtype)
        fitted_sorted = hermite(v, val, slope, xs)
    out = np.empty_like(xs)
    out[order] = fitted_sorted
    return out


# ---------------------------------------------------------------- the clipped sums and the frame
def clipped_sums(X, clip, dtype=np.float64):
    """(C1, C2) per gene over a CSR as stored: the sums of min(x, clip[gene]) and of its square"""
    X = sp.csr_matrix(X)
    c = np.minimum(np.asarray(X.data, dtype=dtype), np.asarray(clip, dtype=dtype)[X.indices])
    G = X.shape[1]
    c1, c2 = np.zeros(G, dtype=dtype), np.zeros(G, dtype=dtype)
    np.add.at(c1, X.indices, c)
    np.add.at(c2, X.indices, c * c)
    return c1, c2


def rank_frame(mean, var, vnorm, n_top_genes, genes):
    order = np.argsort(-np.asarray(vnorm, dtype=np.float64), kind="stable")
    rank = np.empty(order.size, dtype=np.float64)
    rank[order] = np.arange(order.size)
    hv = rank < n_top_genes
    rank[~hv] = np.nan
    return pd.DataFrame({"means": mean, "variances": var, "variances_norm": vnorm, "highly_variable_rank": rank,
                         "highly_variable": hv}, index=genes)


def seurat_v3(X, n_top_genes=2000, span=0.3, surface="interpolate", genes=None, dtype=np.float64, parts=False):
    """scanpy's frame (batch_key=None) for the cells x genes counts X; ``parts``: also a dict of the intermediate arrays"""
    X = sp.csr_matrix(X)
    N, G = X.shape
    if N < 2 or N > CELLS_MAX:
        raise ValueError("seurat_v3 needs 2 <= cells <= %d" % CELLS_MAX)
    s1, s2, flags = gene_moments(X)
    if flags & FLAG_NOT_COUNT:
        raise ValueError("flavor='seurat_v3' expects raw counts: a negative or non-integer value was found")
    if flags & FLAG_TOO_LARGE:
        raise ValueError("flavor='seurat_v3': a count above %d" % COUNT_MAX)
    mean, var = mean_var(s1, s2, N, dtype)
    nc = var > 0
    est = np.zeros(G, dtype=dtype)
    if nc.any():
        est[nc] = loess_fitted(np.log10(mean[nc]), np.log10(var[nc]), span, surface, dtype)
    reg_std = np.sqrt(dtype(10) ** est)
    clip = reg_std * np.sqrt(dtype(N)) + mean
    c1, c2 = clipped_sums(X, clip, dtype)
    vnorm = (N * mean * mean + c2 - 2 * c1 * mean) / ((N - 1) * reg_std * reg_std)
    genes = pd.Index(["gene%d" % j for j in range(G)]) if genes is None else pd.Index(genes)
    frame = rank_frame(mean, var, vnorm, n_top_genes, genes)
    if parts:
        return frame, dict(s1=s1, s2=s2, mean=mean, var=var, est=est, clip=clip, c1=c1, c2=c2, vnorm=vnorm)
    return frame


# ---------------------------------------------------------------- test data
def gamma_poisson_counts(N, G, seed):
    """Gamma-Poisson counts [N][G] (float64): gene means exp(N(-1, 1.5)), dispersions Gamma(2, 0.5) + 0.05; genes 0 and 1
    all zero, gene 2 with one non-zero entry, gene 3 with exactly 64 and gene 4 with exactly 65"""
    rs = np.random.RandomState(seed)
    mu = np.exp(rs.normal(-1.0, 1.5, size=G))
    disp = rs.gamma(2.0, 0.5, size=G) + 0.05
    lam = rs.gamma(1.0 / disp, mu * disp, size=(N, G))
    C = rs.poisson(lam).astype(np.float64)
    C[:, :5] = 0.0
    C[N // 2, 2] = 3.0
    C[rs.permutation(N)[:64], 3] = 1.0 + rs.poisson(1.0, size=64)
    C[rs.permutation(N)[:65], 4] = 1.0 + rs.poisson(2.0, size=65)
    return C


def with_stored_zeros(C, seed=0, every=11):
    """the CSR of C with some of its zeros stored explicitly, rows in a shuffled column order"""
    rs = np.random.RandomState(seed)
    S = (C != 0)
    zr, zc = np.nonzero(~S)
    pick = np.arange(0, zr.size, every)
    S[zr[pick], zc[pick]] = True
    rows, cols = np.nonzero(S)
    key = rs.rand(rows.size)
    order = np.lexsort((key, rows))
    rows, cols = rows[order], cols[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=C.shape[0]))]).astype(np.int64)
    return sp.csr_matrix((C[rows, cols], cols.astype(np.int32), indptr), shape=C.shape)


def tie_case():
    """ten copies each of the abscissae 0..4 with irregular ordinates"""
    x = np.repeat(np.arange(5, dtype=np.float64), 10)
    y = np.random.RandomState(4).normal(size=x.size) + 0.5 * x
    return x, y


# ---------------------------------------------------------------- a device-free engine
class FakeHvgEngine(F.FakeFilterEngine):
    """tests/_filter_ref.py's engine with the three HVG entry points played by the restatement"""

    def preprocess_gene_moments(self):
        self.calls.append("gene_moments")
        return gene_moments(self.X)

    def preprocess_loess_fit(self, x, y, q, x0):
        self.calls.append("loess_fit")
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        x0 = np.asarray(x0, dtype=np.float64)
        val, slope, status = np.zeros(x0.size), np.zeros(x0.size), np.zeros(x0.size, dtype=np.int32)
        for i, p in enumerate(x0):
            try:
                val[i], slope[i] = local_fit(x, y, p, q)
            except ValueError:
                status[i] = STATUS_ZERO_WIDTH
        return val, slope, status

    def preprocess_clipped_sums(self, clip):
        self.calls.append("clipped_sums")
        return clipped_sums(self.X, clip)
