"""Host side of the device tridiagonal eigen-solver tests (test_host_tridiag_eig.py, test_gpu_tridiag_eig.py): a float64
numpy restatement of csrc/tridiag_eig_host.hip.h -- the yardstick for its arithmetic --, the extra matrices and the fuzz
set.  The k largest eigenpairs of T = tridiag(e, d, e):

* scaling: |T|_1 = max_i ((|d_i| + |e_i|) + |e_{i-1}|); zero: w = 0 and the first k unit vectors; otherwise d and e
  times the power of two that brings |T|_1 into [1, 2) (ldexp: exact), the eigenvalues scaled back at the end;
* eigenvalues: multisection on Sturm counts, 64 points lo + (hi - lo) ((l + 1) / 65) per round; with f the number of
  leading points whose count is <= n-1-j the bracket becomes [point f-1, point f] (an old end where there is no such
  point), which keeps count(lo) <= n-1-j < count(hi) whatever the counts between do; finished at
  hi - lo <= max(2 eps max(|lo|, |hi|), pivmin), at most 40 rounds, the eigenvalue (lo + hi) / 2.  **The device holds
  these to the bit**;
* eigenvectors: inverse iteration on all k at once, dstein's shift separation (10 eps |lambda_j|), dlagtf's elimination
  order and storage with the plain magnitude test |c_k| > |a_k| for a row swap, a fixed hashed start vector in (-1, 1),
  exactly three iterations (scale to |.|_inf = 1, forward sweep, back sweep with pivots below pert = max(eps |T|_1,
  tiny) replaced by copysign(pert, .)), no orthogonalisation inside, a 2-norm normalisation behind;
* classical Gram-Schmidt twice (CGS2) over the columns in descending order of eigenvalue;
* the check, u_T = n eps |T|_1: accepted iff every entry is finite, max |T Z - Z diag(w)| <= 2 u_T and
  max |Z^T Z - I| <= 2 n eps; a third ratio, max_j |z_j^T T z_j - w_j| / u_T, is reported and not judged.  ``check`` is
  written in the device's operation order (rounded products, sums over the rows in order), so that on the device's own
  Z it reproduces the device's figures.

Without orthogonalisation inside the iterations the scheme fails on some large tight clusters; that is what the check
and the host fallback (preprocess.tridiagonal_top) are for.  **The fuzz set departs from the issue that asked for it**:
its prototype failed on integer diagonals with couplings of 1e-9; this restatement, whose start vector differs from
column to column, is right on all of those (80 of 80, also at 1e-8 ... 1e-5), because every shift then sees an
isotropic cluster and CGS2 separates the random projections.  It does fail where the spread of a cluster of n / 2 ... n
eigenvalues is a small multiple of dstein's shift separation, so the integer-diagonal kind below draws one or two
integer values jittered at, and coupled at, a scale of 10^U(-15.5, -13); the set was chosen so that it holds such
failures (2 of 400 at this seed, at 2.8 and 2.9 u_T against the 2 accepted), not so that any code passes.  The GPU test
of the fallback takes the one rejected by the widest margin (``fuzz_rejected``); there the residual is the mixing inside
the cluster, not rounding: the device reported the restatement's 2.857 u_T to every printed digit.  test_host_tridiag_eig.py
prints the ratios this restatement reaches."""
import functools

import numpy as np

from tests import _tridiag_ref as tref

EPS = 2.0 ** -52
TINY = float(np.finfo(np.float64).tiny)
NPTS = 64
MAX_ROUNDS = 40
N_ITER = 3
ACCEPT = 2.0
FRAC = np.arange(1, NPTS + 1, dtype=np.float64) / (NPTS + 1.0)


# ---------------------------------------------------------------- scaling and bounds
def scale_and_bounds(d, e):
    """(ds, es, e2, shift, pivmin, lo0, hi0, norm): the scaled matrix (ds = ldexp(d, shift)), the squared couplings,
    pivmin, the widened Gershgorin interval and the scaled |T|_1; norm = 0: the zero matrix, everything else None"""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    ef = np.zeros(n)
    ef[:n - 1] = np.asarray(e, dtype=np.float64)
    eb = np.r_[0.0, ef[:n - 1]]                                      # e_{i-1}
    norm = float(((np.abs(d) + np.abs(ef)) + np.abs(eb)).max())
    if norm == 0.0:
        return None, None, None, 0, None, None, None, 0.0
    shift = 1 - int(np.frexp(norm)[1])
    ds, es = np.ldexp(d, shift), np.ldexp(ef, shift)
    esb = np.r_[0.0, es[:n - 1]]
    e2 = es * es
    pivmin = TINY * max(1.0, float(e2.max()))
    r = np.abs(es) + np.abs(esb)
    gl, gu = float((ds - r).min()), float((ds + r).max())
    wid = (2.0 * n * EPS) * max(abs(gl), abs(gu)) + 2.0 * pivmin
    snorm = float(((np.abs(ds) + np.abs(es)) + np.abs(esb)).max())
    return ds, es[:n - 1], e2[:n - 1], shift, pivmin, gl - wid, gu + wid, snorm


def sturm_count(ds, e2, pivmin, x):
    """#{q_i < 0} at every entry of x"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = ds[0] - x
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        cnt = (q < 0).astype(np.int64)
        for i in range(1, ds.size):
            q = (ds[i] - x) - e2[i - 1] / q
            q = np.where(np.abs(q) < pivmin, -pivmin, q)
            cnt += q < 0
    return cnt


def eigenvalues(ds, e2, pivmin, lo0, hi0, k):
    """the k largest eigenvalues of the scaled matrix, descending, and the number of rounds the slowest took"""
    n = ds.size
    target = (n - 1 - np.arange(k))[:, None]
    lo, hi = np.full(k, lo0), np.full(k, hi0)
    rounds = 0

    def live():
        return hi - lo > np.maximum(2.0 * EPS * np.maximum(np.abs(lo), np.abs(hi)), pivmin)
    while rounds < MAX_ROUNDS and live().any():
        a = live()
        pts = lo[:, None] + (hi - lo)[:, None] * FRAC[None, :]
        above = sturm_count(ds, e2, pivmin, pts) > target
        f = np.where(above.any(axis=1), above.argmax(axis=1), NPTS)
        rows = np.arange(k)
        nlo = np.where(f > 0, pts[rows, np.maximum(f - 1, 0)], lo)
        nhi = np.where(f < NPTS, pts[rows, np.minimum(f, NPTS - 1)], hi)
        lo, hi = np.where(a, nlo, lo), np.where(a, nhi, hi)
        rounds += 1
    return 0.5 * (lo + hi), rounds


# ---------------------------------------------------------------- inverse iteration
def start_vector(n, k):
    """[n][k] in (-1, 1): a 32-bit integer hash of (row, column)"""
    M = np.uint64(0xFFFFFFFF)
    r = np.arange(n, dtype=np.uint64)[:, None]
    c = np.arange(k, dtype=np.uint64)[None, :]
    h = (r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA6B) + np.uint64(0x165667B1)) & M
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M
    h ^= h >> np.uint64(16)
    return (h.astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0


def shifts(w):
    x = np.array(w, dtype=np.float64)
    for j in range(1, x.size):
        tol = 10.0 * EPS * abs(x[j])
        if x[j - 1] - x[j] < tol:
            x[j] = x[j - 1] - tol
    return x


def inverse_iteration(ds, es, w, snorm):
    """[n][k]: three iterations per shift, every column at unit 2-norm"""
    n, k = ds.size, w.size
    x = shifts(w)
    pert = max(EPS * snorm, TINY)
    piv, s1, s2, mul = np.zeros((n, k)), np.zeros((n, k)), np.zeros((n, k)), np.zeros((n, k))
    swp = np.zeros((n, k), dtype=bool)
    with np.errstate(all="ignore"):
        a = ds[0] - x
        b = np.full(k, es[0]) if n > 1 else np.zeros(k)
        for r in range(n - 1):
            c = es[r]
            an = ds[r + 1] - x
            bn = es[r + 1] if r + 2 < n else 0.0
            sw = np.abs(c) > np.abs(a)
            m = np.where(sw, a, c) / np.where(sw, c, a)
            m = np.where(c == 0.0, 0.0, m)
            piv[r], s1[r], s2[r], mul[r], swp[r] = np.where(sw, c, a), np.where(sw, an, b), np.where(sw, bn, 0.0), m, sw
            a, b = np.where(sw, b, an) - m * np.where(sw, an, b), np.where(sw, -m * bn, bn)
        piv[n - 1] = a
        y = start_vector(n, k)
        for _ in range(N_ITER):
            y = y / np.abs(y).max(axis=0)
            for r in range(n - 1):
                t = np.where(swp[r], y[r], y[r + 1]) - mul[r] * np.where(swp[r], y[r + 1], y[r])
                y[r] = np.where(swp[r], y[r + 1], y[r])
                y[r + 1] = t
            y1, y2 = np.zeros(k), np.zeros(k)
            for r in range(n - 1, -1, -1):
                p = np.where(np.abs(piv[r]) < pert, np.copysign(pert, piv[r]), piv[r])
                y0 = ((y[r] - s1[r] * y1) - s2[r] * y2) / p
                y[r] = y0
                y1, y2 = y0, y1
        y = y / np.abs(y).max(axis=0)
        return y / np.sqrt((y * y).sum(axis=0))


def cgs2(Z):
    Z = np.array(Z, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(Z.shape[1]):
            for _ in range(2):
                Z[:, j] -= Z[:, :j] @ (Z[:, :j].T @ Z[:, j])
            Z[:, j] /= np.sqrt(Z[:, j] @ Z[:, j])
    return Z


# ---------------------------------------------------------------- the check
def check(ds, es, ws, Z, snorm):
    """(accepted, residual / u_T, |rayleigh - w| / u_T, orthogonality / (n eps)) on the scaled matrix, in the device's
    operation order: t_r = (e_{r-1} z_{r-1} + d_r z_r) + e_r z_{r+1}, the residual t_r - w z_r, the Rayleigh quotient
    and the Gram matrix summed over the rows in order"""
    n, k = Z.shape
    uT = n * EPS * snorm
    with np.errstate(all="ignore"):
        finite = bool(np.isfinite(Z).all() and np.isfinite(ws).all())
        zero = np.zeros((1, k))
        el = np.r_[0.0, es][:, None]
        er = np.r_[es, 0.0][:, None]
        t = (el * np.vstack([zero, Z[:-1]]) + ds[:, None] * Z) + er * np.vstack([Z[1:], zero])
        res = np.abs(t - ws[None, :] * Z).max()
        rq, G = np.zeros(k), np.zeros((k, k))
        for r in range(n):
            rq = rq + Z[r] * t[r]
            G = G + Z[r][:, None] * Z[r][None, :]
        ray = np.abs(rq - ws).max()
        orth = np.abs(G - np.eye(k)).max()
    ratios = (float(res / uT), float(ray / uT), float(orth / (n * EPS)))
    ok = finite and res <= ACCEPT * uT and orth <= ACCEPT * n * EPS
    return bool(ok), ratios


def eigh_top(d, e, k):
    """(w [k] descending, Z [n][k], accepted, ratios, rounds); Z is meaningless when not accepted"""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    assert 1 <= k <= n
    ds, es, e2, shift, pivmin, lo0, hi0, snorm = scale_and_bounds(d, e)
    if snorm == 0.0:
        return np.zeros(k), np.eye(n)[:, :k].copy(), True, (0.0, 0.0, 0.0), 0
    ws, rounds = eigenvalues(ds, e2, pivmin, lo0, hi0, k)
    Z = cgs2(inverse_iteration(ds, es, ws, snorm))
    ok, ratios = check(ds, es, ws, Z, snorm)
    return np.ldexp(ws, -shift), Z, ok, ratios, rounds


def t_contracts(d, e, w, Z):
    """(residual / u_T, orthogonality / (n eps)) against the unscaled T, plain numpy"""
    T = tref.tridiagonal_matrix(d, e)
    n = T.shape[0]
    u = tref.unit(T)
    res = np.abs(T @ Z - Z * w).max()
    orth = np.abs(Z.T @ Z - np.eye(Z.shape[1])).max() / (n * EPS)
    return (res / u if u > 0 else (0.0 if res == 0 else np.inf)), orth


# ---------------------------------------------------------------- the extra matrices (given as (d, e), k)
def wilkinson(m=21):
    return np.abs(np.arange(m) - (m - 1) / 2.0), np.ones(m - 1)


def glued_wilkinson(copies=5, m=21, glue=1e-8):
    d, e = wilkinson(m)
    return np.tile(d, copies), np.r_[tuple([e, [glue]] * (copies - 1) + [e])]


def extras():
    """(name, d, e, k)"""
    rs = np.random.RandomState(23)
    dg, eg = glued_wilkinson()
    n = 40
    graded = 10.0 ** -np.arange(n, dtype=np.float64) * 1.0
    out = [("glued_wilkinson", dg, eg, 40),
           ("graded", graded[:20], 0.1 * np.sqrt(graded[:19] * graded[1:20]), 8),
           ("identity", np.ones(12), np.zeros(11), 5),
           ("n64_full", rs.randn(64), rs.randn(63), 64)]
    return out


def poisson_2000():
    """a Poisson scatter with n = 2000 (2400 cells), reduced by LAPACK (the restatement of the device's reduction
    would take minutes at this size): the bisection and the sweeps at the length the PCA runs them"""
    from scipy.linalg import hessenberg
    H = hessenberg(tref.scatter_of(tref.poisson_counts(2400, 2000, 31)))
    return np.diag(H).copy(), np.diag(H, -1).copy(), 50


# Names only at import: a test module parametrises over them, and the matrices (the restated reduction of every case,
# a 2000 x 2000 Hessenberg reduction) are built inside the tests that ask for them, once each.
CASE_NAMES = ("n1", "n2", "n3", "n17_zero_tail", "n65_poisson", "n257_poisson", "n130_rank39", "n65_clustered",
              "diagonal", "zero", "tridiagonal")                 # (_tridiag_ref.cases(); test_host_tridiag_eig.py checks)
EXTRA_NAMES = ("glued_wilkinson", "graded", "identity", "n64_full")
ALL_NAMES = CASE_NAMES + EXTRA_NAMES + ("n2000_poisson", "n65_poisson_2^300", "n65_poisson_2^-300")


@functools.lru_cache(maxsize=None)
def case_reduction(name):
    """(A, k, d, e, R, tau) of the _tridiag_ref.cases() entry ``name``, reduced by the restatement of the device's
    reduction"""
    _, A, k = next(c for c in tref.cases() if c[0] == name)
    d, e, R, tau = tref.tridiag_deferred(A)
    return A, k, d, e, R, tau


@functools.lru_cache(maxsize=None)
def tridiagonal(name):
    """(d, e, k) of the entry of ALL_NAMES called ``name``"""
    if name in CASE_NAMES:
        _, k, d, e, _, _ = case_reduction(name)
        return d, e, k
    if name in EXTRA_NAMES:
        return next(c[1:] for c in extras() if c[0] == name)
    if name == "n2000_poisson":
        return poisson_2000()
    power = {"n65_poisson_2^300": 300, "n65_poisson_2^-300": -300}[name]
    d, e, k = tridiagonal("n65_poisson")
    return np.ldexp(d, power), np.ldexp(e, power), k


@functools.lru_cache(maxsize=None)
def solved(name):
    """eigh_top of tridiagonal(name), computed once"""
    return eigh_top(*tridiagonal(name))


# ---------------------------------------------------------------- the fuzz set
FUZZ_KINDS = ("random", "integer_diagonal", "graded", "wilkinson_like", "sparse_coupling")
FUZZ_PER_KIND = 80


def fuzz(seed=1234):
    """400 matrices, n < 48: (kind, d, e, k)"""
    rs = np.random.RandomState(seed)
    out = []
    for kind in FUZZ_KINDS:
        for _ in range(FUZZ_PER_KIND):
            n = int(rs.randint(2, 48))
            k = int(rs.randint(1, n + 1))
            if kind == "random":
                d, e = rs.randn(n), rs.randn(n - 1)
            elif kind == "integer_diagonal":             # 1 or 2 distinct values: clusters of n / 2 to n eigenvalues
                m = int(rs.randint(1, 3))                # whose spread is a small multiple of the shift separation
                s = 10.0 ** rs.uniform(-15.5, -13)       # (the diagonal jittered at that scale too)
                d = rs.randint(1, 1 + m, n) + s * rs.randn(n)
                e = s * rs.randn(n - 1)
            elif kind == "graded":
                g = 10.0 ** (-rs.uniform(0, 12) * np.arange(n) / n)
                d, e = g * rs.randn(n), np.sqrt(g[:-1] * g[1:]) * rs.randn(n - 1) * 0.3
            elif kind == "wilkinson_like":
                d, e = np.abs(np.arange(n) - (n - 1) / 2.0), np.ones(n - 1) * rs.choice([1.0, 0.5, 1e-3])
            else:
                d, e = rs.randn(n), rs.randn(n - 1) * (rs.rand(n - 1) < 0.3)
            out.append((kind, d, e, k))
    return out


@functools.lru_cache(maxsize=None)
def fuzz_rejected():
    """(kind, d, e, k, ratios) of the fuzz matrix that the restatement's check rejects by the widest margin (the largest
    of residual / 2 u_T and orthogonality / 2 n eps): the subject of the GPU test of the fallback"""
    best = None
    for kind, d, e, k in fuzz():
        _, _, ok, ratios, _ = eigh_top(d, e, k)
        if not ok and (best is None or max(ratios[0], ratios[2]) > max(best[4][0], best[4][2])):
            best = (kind, d, e, k, ratios)
    return best
