"""The tridiagonal eigen-solver on the device (csrc/tridiag_eig_host.hip.h) against its float64 restatement
(tests/_tridiag_eig_ref.py: the eigenvalues bit for bit) and the gap-free contracts of tests/_tridiag_ref.py (8 units
for the device), through every layer: the solver alone, ``symmetric_eigh_top(solver="device")``, the slot route
``preprocess_pca_device`` and ``pca="device_full"`` end to end."""
import types

import numpy as np
import pandas as pd
import pytest

from cnmf_amd import preprocess as pp
from tests import _pre_ref as pre_ref
from tests import _tridiag_eig_ref as er
from tests import _tridiag_ref as ref

pytestmark = pytest.mark.gpu
F = ref.DEVICE_FACTOR
LD = pre_ref.LD


def case(name):
    """(A, k) of the _tridiag_ref.cases() entry"""
    return er.case_reduction(name)[:2]


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def agree(a, b):
    """to a factor of 2"""
    return a <= 2 * b and b <= 2 * a


# ---------------------------------------------------------------- 1. the solver alone
@pytest.mark.parametrize("name", er.ALL_NAMES)
def test_solver_alone(engine, name):
    d, e, k = er.tridiagonal(name)
    w_ref = er.solved(name)[0]
    w, Z, accepted = engine.tridiagonal_eigh_top(d, e, k)
    reported = engine.last_tridiagonal_check
    assert np.array_equal(bits(w), bits(w_ref))
    assert accepted and engine.last_tridiagonal_solver == "device"
    res, orth = er.t_contracts(d, e, w, Z)
    ds, es, _, shift, _, _, _, snorm = er.scale_and_bounds(d, e)
    _, again = er.check(ds, es, np.ldexp(w, shift), Z, snorm) if snorm else (True, (0.0, 0.0, 0.0))
    print("%s: residual %.3g u_T, orthogonality %.3g n eps; reported %s, recomputed %s"
          % (name, res, orth, ["%.3g" % r for r in reported], ["%.3g" % r for r in again]))
    assert res <= F and orth <= F
    assert all(agree(a, b) for a, b in zip(reported, again))


# ---------------------------------------------------------------- 2. symmetric_eigh_top(solver="device")
@pytest.mark.parametrize("name", er.CASE_NAMES)
def test_symmetric_eigh_top_on_the_device(engine, name):
    A, k = case(name)
    w, V = engine.symmetric_eigh_top(A, k, solver="device")
    assert engine.last_tridiagonal_solver == "device"
    assert w.shape == (k,) and V.shape == (A.shape[0], k)
    res, eig, orth, desc = ref.contracts(A, w, V)
    print("%s: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (name, res, eig, orth))
    assert res <= F and eig <= F and orth <= F and desc
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0).all()


# ---------------------------------------------------------------- 3. more vectors than a wavefront has lanes
def test_more_than_64_components(engine):
    A = case("n130_rank39")[0]
    w, V = engine.symmetric_eigh_top(A, 100, solver="device")
    assert engine.last_tridiagonal_solver == "device"
    res, eig, orth, desc = ref.contracts(A, w, V)
    print("n130 k100: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (res, eig, orth))
    assert res <= F and eig <= F and orth <= F and desc


# ---------------------------------------------------------------- 4. determinism
def test_two_calls_give_the_same_bits(engine):
    A, k = case("n257_poisson")
    a, b = engine.symmetric_eigh_top(A, k, solver="device"), engine.symmetric_eigh_top(A, k, solver="device")
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


# ---------------------------------------------------------------- 5. a result the check rejects
def test_rejected_solve_falls_back_to_the_host(engine):
    kind, d, e, k, ratios = er.fuzz_rejected()           # (the one the restatement rejects by the widest margin)
    w_ref = er.eigh_top(d, e, k)[0]
    w, Z, accepted = engine.tridiagonal_eigh_top(d, e, k)
    print("%s n = %d k = %d: the restatement reports %s, the device %s" % (kind, len(d), k, ratios,
                                                                        engine.last_tridiagonal_check))
    assert not accepted and engine.last_tridiagonal_solver == "host_fallback"
    assert np.array_equal(bits(w), bits(w_ref))
    A = ref.tridiagonal_matrix(d, e)
    w, V = engine.symmetric_eigh_top(A, k, solver="device")
    assert engine.last_tridiagonal_solver == "host_fallback"
    res, eig, orth, desc = ref.contracts(A, w, V)
    print("after the fallback: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (res, eig, orth))
    assert res <= F and eig <= F and orth <= F and desc


# ---------------------------------------------------------------- 6. the slot route
@pytest.mark.parametrize("shape", [(300, 257, 50), (40, 130, 39)], ids=["300x257", "40x130"])
def test_slot_route(engine, shape):
    N, n, k = shape
    X = ref.poisson_counts(N, n, seed=N + n)
    engine.preprocess_set_dense(0, X)
    mean0, S = engine.preprocess_scatter(0)
    mean, w, V, scores = engine.preprocess_pca_device(0, k)
    assert engine.last_tridiagonal_solver == "device"
    assert np.array_equal(bits(mean), bits(mean0))
    res, eig, orth, desc = ref.contracts(S, w, V)
    print("%d x %d: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (N, n, res, eig, orth))
    assert res <= F and eig <= F and orth <= F and desc
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0).all()
    want, mag = pre_ref.ld_product(X.astype(LD) - mean.astype(LD), V)
    err = np.abs(scores.astype(LD) - want).astype(np.float64)
    bound = pre_ref.gemm_bound(n, mag)
    print("scores: worst ratio %.3f" % np.max(err / np.where(bound > 0, bound, 1.0)))
    assert np.all(err <= bound)
    assert np.array_equal(bits(engine.preprocess_fetch(0)), bits(X))     # the slot is as it was


# ---------------------------------------------------------------- 7. end to end (the planted fixture of test_gpu_pca.py)
N_E2E, G_ALL, G_SEL, N_FACTORS = 400, 150, 120, 6
BLOCKS = (30, 24, 19, 15, 12, 9)


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
    counts = rs.poisson(0.3 + U @ H + 60.0 * ~mask).astype(np.float64)
    cells = ["c%d" % i for i in range(N_E2E)]
    obs = pd.DataFrame({"batch": ["b%d" % (i % 3) for i in range(N_E2E)]}, index=cells)
    R, Phi = pre_ref.make_ridge(N_E2E, 5, 4, seed=3)
    res = types.SimpleNamespace(K=5, lamb=np.diag(np.r_[0.0, np.ones(3)]), R=R, Phi_moe=Phi, Z_corr=np.zeros((50, N_E2E)))
    return counts, cells, ["g%d" % j for j in range(G_ALL)], mask, obs, res


def test_device_full_end_to_end(engine, planted):
    counts, cells, genes, mask, obs, res = planted
    P = pp.Preprocess(engine=engine)
    out = {}
    for mode in ("device", "device_full"):
        out[mode], _ = P.normalize_batchcorrect((counts, cells, genes), obs=obs, highly_variable=mask,
                                                harmony_vars=["batch"], harmony_res=res, makeplots=False, pca=mode)
    assert engine.last_tridiagonal_solver == "device"
    assert np.array_equal(bits(out["device_full"].X), bits(out["device"].X))
    assert out["device_full"].obsm["X_pca"].shape == (N_E2E, 50)
    import scipy.sparse as sp
    engine.preprocess_upload(sp.csr_matrix(counts))
    engine.preprocess_select(0, np.flatnonzero(mask), 1e4, None)
    pp._ceiling(engine, 0, N_E2E, G_SEL, .9999)
    engine.preprocess_densify(0)
    _, S = engine.preprocess_scatter(0)
    lam, Vh = np.linalg.eigh(S)
    lam, Vh = lam[::-1], Vh[:, ::-1]
    _, w, Vd, scores = engine.preprocess_pca_device(0, 50)
    assert np.array_equal(bits(scores), bits(out["device_full"].obsm["X_pca"]))
    norm = np.abs(S).sum(axis=1).max()
    for i in range(N_FACTORS):
        g = np.abs(np.delete(lam, i) - lam[i]).min() / norm
        bound = F * G_SEL * ref.EPS / g                  # Davis-Kahan with a backward error of 8 u (test_gpu_pca.py)
        c = float(Vh[:, i] @ Vd[:, i])
        sin = np.linalg.norm(Vd[:, i] - np.sign(c) * Vh[:, i] * abs(c))
        print("component %d: relative gap %.3g, sin %.3g, bound %.3g" % (i, g, sin, bound))
        assert bound < 1e-8, (i, g)
        assert sin <= bound, (i, sin, bound)


# ---------------------------------------------------------------- 8. the largest size
def test_largest_size(engine):
    """the construction of test_gpu_pca.py's test_largest_size_takes_the_large_lds_launches"""
    n, b, k = 8192, 200, 12
    rs = np.random.RandomState(8)
    block = ref.random_symmetric(b, 9)
    diag = rs.uniform(-20.0, 20.0, n - b)
    diag[[5, 4000, 7000, n - b - 1]] = [45.0, 33.0, 31.0, 29.0]
    A = np.zeros((n, n))
    A[:b, :b] = block
    A[np.arange(b, n), np.arange(b, n)] = diag
    u = n * ref.EPS * max(np.abs(block).sum(axis=1).max(), np.abs(diag).max())
    lam = np.sort(np.r_[np.linalg.eigvalsh(block), diag])[::-1][:k]
    w, V = engine.symmetric_eigh_top(A, k, solver="device")
    assert engine.last_tridiagonal_solver == "device"
    res = np.abs(np.vstack([block @ V[:b], diag[:, None] * V[b:]]) - V * w).max()
    eig = np.abs(w - lam).max()
    orth = np.abs(V.T @ V - np.eye(k)).max()
    print("n8192: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (res / u, eig / u, orth / (n * ref.EPS)))
    assert res <= F * u and eig <= F * u and orth <= F * n * ref.EPS and np.all(np.diff(w) <= 0)
    assert (V[np.argmax(np.abs(V), axis=0), np.arange(k)] > 0).all()


# ---------------------------------------------------------------- 9. limits
def test_limits(engine):
    n = 8193
    A = np.broadcast_to(np.float64(0.0), (n, n))             # (no memory behind it)
    with pytest.raises(NotImplementedError, match="8192"):
        engine.symmetric_eigh_top(A, 3, solver="device")
    import ctypes as C
    one = np.zeros(4)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert engine._lib.cnmf_symmetric_eigh_top(engine._ctx, n, 1, p, p, p, p) == -5
    assert engine._lib.cnmf_tridiagonal_eigh_top(engine._ctx, n, 1, p, p, p, p, p) == -5
    B = ref.random_symmetric(6, 1)
    B[2, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        engine.symmetric_eigh_top(B, 2, solver="device")
    with pytest.raises(ValueError, match="non-finite"):
        engine.tridiagonal_eigh_top(np.r_[1.0, np.inf, 2.0], np.ones(2), 1)
    B = ref.random_symmetric(6, 1)
    for k in (0, 7):
        with pytest.raises(ValueError):
            engine.symmetric_eigh_top(B, k, solver="device")
        with pytest.raises(ValueError):
            engine.tridiagonal_eigh_top(np.ones(6), np.ones(5), k)
    assert engine._lib.cnmf_tridiagonal_eigh_top(engine._ctx, 3, 4, p, p, p, p, p) == -1
