"""The PCA through the tridiagonal form on the device (csrc/pca_host.hip.h) against gap-free contracts: with the unit
u = n eps |A|_inf (eps = 2^-52) the device is given 8 u for residuals and eigenvalues and 8 n eps for orthogonality --
the O(n eps) backward-error bound of Householder reduction, the factor for the device's summation order and FMA
contraction (tests/_tridiag_ref.py, whose numpy restatement of the same algorithm shows at most 0.46 u and 2.5 n eps).
Eigenvectors are compared entry by entry nowhere; the one comparison of loadings uses the bound the eigenvalue gaps give."""
import types

import numpy as np
import pandas as pd
import pytest

from cnmf_amd import preprocess as pp
from tests import _pre_ref as pre_ref
from tests import _tridiag_ref as ref

pytestmark = pytest.mark.gpu
F = ref.DEVICE_FACTOR
CASES = ref.cases()
CASE_IDS = [c[0] for c in CASES]
LD = pre_ref.LD


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def report(what, res, eig, orth):
    print("%s: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (what, res, eig, orth))


# ---------------------------------------------------------------- 1. the tridiagonalisation alone
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_tridiagonal_form_has_the_eigenvalues(engine, case):
    name, A, _ = CASES[case]
    n, u = A.shape[0], ref.unit(A)
    d, e = engine.symmetric_tridiagonalize(A)
    assert d.shape == (n,) and e.shape == (n - 1,)
    err = np.abs(ref.tridiagonal_eigvals(d, e) - np.linalg.eigvalsh(A)).max()
    print("%s: eigenvalues of (d, e) off by %.3g u" % (name, err / u if u else err))
    assert err <= F * u
    if name == "n17_zero_tail":
        assert e[0] == A[1, 0] and d[0] == A[0, 0]                       # tau_0 = 0: nothing moved


# ---------------------------------------------------------------- 2. the back-transformation alone
@pytest.mark.parametrize("name", ["n17_zero_tail", "n65_poisson"])
def test_back_transform_of_the_identity(engine, name):
    A = next(c[1] for c in CASES if c[0] == name)
    n, u = A.shape[0], ref.unit(A)
    d, e = engine.symmetric_tridiagonalize(A)
    Q = engine.tridiagonal_back_transform(np.eye(n))
    orth = np.abs(Q.T @ Q - np.eye(n)).max()
    sim = np.abs(Q.T @ A @ Q - ref.tridiagonal_matrix(d, e)).max()
    print("%s: |Q^T Q - I| = %.3g n eps, |Q^T A Q - T| = %.3g u" % (name, orth / (n * ref.EPS), sim / u))
    assert orth <= F * n * ref.EPS and sim <= F * u


# ---------------------------------------------------------------- 3, 4. symmetric_eigh_top and the sign rule
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_symmetric_eigh_top_meets_the_contracts(engine, case):
    name, A, k = CASES[case]
    w, V = engine.symmetric_eigh_top(A, k)
    assert w.shape == (k,) and V.shape == (A.shape[0], k)
    res, eig, orth, desc = ref.contracts(A, w, V)
    report(name, res, eig, orth)
    assert res <= F and eig <= F and orth <= F and desc
    lead = V[np.argmax(np.abs(V), axis=0), np.arange(k)]
    assert (lead > 0).all()


def test_sign_rule_takes_the_first_index_on_ties_and_can_be_left_off(engine):
    """a diagonal matrix moves nothing (every tau is 0), so the back-transformation returns Z itself"""
    engine.symmetric_tridiagonalize(np.diag(np.arange(5.0)))
    Z = np.array([[-2.0, 1.0, 0.5], [2.0, -3.0, -0.5], [1.0, 3.0, 0.5], [0.0, 0.0, 0.0], [-2.0, 1.0, -0.5]])
    assert np.array_equal(engine.tridiagonal_back_transform(Z), Z)
    want = Z * np.array([-1.0, -1.0, 1.0])               # first of the ties: -2 at row 0, -3 at row 1, 0.5 at row 0
    assert np.array_equal(engine.tridiagonal_back_transform(Z, sign_rule=True), want)
    assert np.array_equal(want, ref.sign_rule(Z))
    one = engine.tridiagonal_back_transform(Z[:, 1:2], sign_rule=True)   # any 1 <= n_comp <= n
    assert np.array_equal(one, want[:, 1:2])


# ---------------------------------------------------------------- 5. determinism
def test_two_calls_give_the_same_bits(engine):
    _, A, k = CASES[CASE_IDS.index("n257_poisson")]
    a, b = engine.symmetric_eigh_top(A, k), engine.symmetric_eigh_top(A, k)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    d0, e0 = engine.symmetric_tridiagonalize(A)
    d1, e1 = engine.symmetric_tridiagonalize(A)
    assert np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(e0), bits(e1))


# ---------------------------------------------------------------- 6. staging
def test_staging_is_replaced_and_released(engine):
    A65, A17 = CASES[CASE_IDS.index("n65_poisson")][1], CASES[CASE_IDS.index("n17_zero_tail")][1]
    engine.symmetric_tridiagonalize(A65)
    d, e = engine.symmetric_tridiagonalize(A17)
    with pytest.raises(ValueError, match="staged tridiagonalisation has 17"):
        engine.tridiagonal_back_transform(np.eye(65))
    Q = engine.tridiagonal_back_transform(np.eye(17))
    assert np.abs(Q.T @ A17 @ Q - ref.tridiagonal_matrix(d, e)).max() <= F * ref.unit(A17)
    with pytest.raises(ValueError, match="n_comp"):
        engine.tridiagonal_back_transform(np.zeros((17, 18)))
    engine.preprocess_release()
    with pytest.raises(ValueError, match="no tridiagonalisation is staged"):
        engine.tridiagonal_back_transform(np.eye(17))


# ---------------------------------------------------------------- 7. the slot route
@pytest.mark.parametrize("shape", [(300, 257, 50), (40, 130, 39)], ids=["300x257", "40x130"])
def test_slot_route(engine, shape):
    N, n, k = shape
    X = ref.poisson_counts(N, n, seed=N + n)
    engine.preprocess_set_dense(0, X)
    mean0, S = engine.preprocess_scatter(0)
    with pytest.raises(ValueError, match="cnmf_preprocess_pca_tridiag has not been called"):
        engine.preprocess_pca_finish(0, np.eye(n)[:, :k])
    mean, d, e = engine.preprocess_pca_tridiag(0)
    assert np.array_equal(bits(mean), bits(mean0))
    w, Z = pp.tridiagonal_top(d, e, k)
    V, scores = engine.preprocess_pca_finish(0, Z)
    res, eig, orth, desc = ref.contracts(S, w, V)
    report("%d x %d" % (N, n), res, eig, orth)
    assert res <= F and eig <= F and orth <= F and desc
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0).all()
    want, mag = pre_ref.ld_product(X.astype(LD) - mean.astype(LD), V)
    err = np.abs(scores.astype(LD) - want).astype(np.float64)
    bound = pre_ref.gemm_bound(n, mag)
    print("scores: worst ratio %.3f" % np.max(err / np.where(bound > 0, bound, 1.0)))
    assert np.all(err <= bound)
    assert np.array_equal(bits(engine.preprocess_fetch(0)), bits(X))     # the slot is as it was
    # the free-standing pair shares the staging: it takes the slot route's place
    engine.symmetric_tridiagonalize(np.eye(3))
    with pytest.raises(ValueError, match="cnmf_preprocess_pca_tridiag has not been called"):
        engine.preprocess_pca_finish(0, Z)


# ---------------------------------------------------------------- 8. end to end
N_E2E, G_ALL, G_SEL, N_FACTORS = 400, 150, 120, 6
BLOCKS = (30, 24, 19, 15, 12, 9)                         # genes per planted factor: six well separated eigenvalues


@pytest.fixture(scope="module")
def planted():
    rs = np.random.RandomState(21)
    sel = np.sort(rs.choice(G_ALL, G_SEL, replace=False))
    H = np.zeros((N_FACTORS, G_ALL))
    at = 0
    for f, b in enumerate(BLOCKS):
        H[f, sel[at:at + b]] = rs.gamma(4.0, 1.0, size=b) + 2.0
        at += b
    U = rs.gamma(1.0, 1.0, size=(N_E2E, N_FACTORS))
    mask = np.zeros(G_ALL, dtype=bool)
    mask[sel] = True
    # (the genes left out carry most of a cell's counts: library-size normalisation then leaves the six factors apart)
    counts = rs.poisson(0.3 + U @ H + 60.0 * ~mask).astype(np.float64)
    cells = ["c%d" % i for i in range(N_E2E)]
    obs = pd.DataFrame({"batch": ["b%d" % (i % 3) for i in range(N_E2E)]}, index=cells)
    R, Phi = pre_ref.make_ridge(N_E2E, 5, 4, seed=3)
    res = types.SimpleNamespace(K=5, lamb=np.diag(np.r_[0.0, np.ones(3)]), R=R, Phi_moe=Phi, Z_corr=np.zeros((50, N_E2E)))
    return counts, cells, ["g%d" % j for j in range(G_ALL)], mask, obs, res


def test_normalize_batchcorrect_end_to_end(engine, planted):
    counts, cells, genes, mask, obs, res = planted
    P = pp.Preprocess(engine=engine)
    out = {}
    for mode in pp.PCA_MODES:
        out[mode], _ = P.normalize_batchcorrect((counts, cells, genes), obs=obs, highly_variable=mask,
                                                harmony_vars=["batch"], harmony_res=res, makeplots=False, pca=mode)
    # the ridge correction does not read the scores: any difference here is a disturbance of the staged slots
    assert np.array_equal(bits(out["device"].X), bits(out["lapack"].X))
    assert out["device"].obsm["X_pca"].shape == out["lapack"].obsm["X_pca"].shape == (N_E2E, 50)
    # the loadings of both routes, on the same staged matrix (normalize_batchcorrect's own staging steps)
    import scipy.sparse as sp
    sel = np.flatnonzero(mask)
    engine.preprocess_upload(sp.csr_matrix(counts))
    engine.preprocess_select(0, sel, 1e4, None)
    pp._ceiling(engine, 0, N_E2E, G_SEL, .9999)
    engine.preprocess_densify(0)
    _, S = engine.preprocess_scatter(0)
    lam, Vh = np.linalg.eigh(S)
    lam, Vh = lam[::-1], Vh[:, ::-1]
    _, d, e = engine.preprocess_pca_tridiag(0)
    w, Z = pp.tridiagonal_top(d, e, 50)
    Vd, scores = engine.preprocess_pca_finish(0, Z)
    assert np.array_equal(bits(scores), bits(out["device"].obsm["X_pca"]))
    # Davis-Kahan with a backward error of 8 u = 8 n eps |S|_inf: sin(angle) <= 8 u / gap_i = 8 n eps / g_i with the
    # relative gap g_i = min_j |lam_i - lam_j| / |S|_inf
    norm = np.abs(S).sum(axis=1).max()
    for i in range(N_FACTORS):
        g = np.abs(np.delete(lam, i) - lam[i]).min() / norm
        bound = F * G_SEL * ref.EPS / g
        c = abs(float(Vh[:, i] @ Vd[:, i]))
        sin = np.linalg.norm(Vd[:, i] - np.sign(Vh[:, i] @ Vd[:, i]) * Vh[:, i] * c)      # |v_d - (v_h . v_d) v_h|
        print("component %d: relative gap %.3g, sin %.3g, bound %.3g" % (i, g, sin, bound))
        assert bound < 1e-8, (i, g)                          # the fixture: every planted component counts
        assert sin <= bound, (i, sin, bound)


# ---------------------------------------------------------------- the largest size: both kernels above 64 KB of LDS
def test_largest_size_takes_the_large_lds_launches(engine):
    """n = 8192 = CNMF_PCA_NMAX: the column kernel asks for 128 KB of LDS and the back-transformation for 64 KB plus
    its scratch, both more than a launch gets without opting in.  A dense 200 x 200 block in front of a diagonal keeps
    it cheap: the block's reflectors and updates run over full-length rows (the block structure is preserved), the
    columns behind it are tridiagonal already and cost a launch each.  The contracts, with A's structure used on the
    host side only to avoid an 8192 x 8192 eigen-solve."""
    n, b, k = 8192, 200, 12
    rs = np.random.RandomState(8)
    block = ref.random_symmetric(b, 9)
    diag = rs.uniform(-20.0, 20.0, n - b)
    diag[[5, 4000, 7000, n - b - 1]] = [45.0, 33.0, 31.0, 29.0]      # (the block's own spectrum ends near 40)
    A = np.zeros((n, n))
    A[:b, :b] = block
    A[np.arange(b, n), np.arange(b, n)] = diag
    u = n * ref.EPS * max(np.abs(block).sum(axis=1).max(), np.abs(diag).max())
    lam = np.sort(np.r_[np.linalg.eigvalsh(block), diag])[::-1][:k]
    assert 1 <= np.isin(lam, diag).sum() < k                          # both parts are among the kept pairs
    w, V = engine.symmetric_eigh_top(A, k)
    res = np.abs(np.vstack([block @ V[:b], diag[:, None] * V[b:]]) - V * w).max()
    eig = np.abs(w - lam).max()
    orth = np.abs(V.T @ V - np.eye(k)).max()
    report("n8192", res / u, eig / u, orth / (n * ref.EPS))
    assert res <= F * u and eig <= F * u and orth <= F * n * ref.EPS and np.all(np.diff(w) <= 0)
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0).all()


# ---------------------------------------------------------------- 9. the limit
def test_limit_is_checked_before_anything_is_allocated(engine):
    n = 8193
    A = np.broadcast_to(np.float64(0.0), (n, n))             # (no memory behind it)
    with pytest.raises(NotImplementedError, match="8192"):
        engine.symmetric_tridiagonalize(A)
    with pytest.raises(NotImplementedError, match='pca="lapack"'):
        pp._pca(engine, 0, 10 * n, n, pca="device")
    # the library's own check (the Python layer never reaches it): CNMF_EUNSUPPORTED with a pointer it never reads
    import ctypes as C
    one = np.zeros(1)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert engine._lib.cnmf_symmetric_tridiagonalize(engine._ctx, n, p, p, p) == -5
