"""The device tridiagonal eigen-solver's float64 restatement (tests/_tridiag_eig_ref.py) without a GPU: its Sturm count
against LAPACK's eigenvalues, its eigenvalues within its own stopping tolerance, the three contracts (<= 8, through the
restated back-transformation) on every test matrix, the fuzz set (what the check accepts meets the contracts, what it
rejects is rescued by the host fallback) and the validation of ``pca="device_full"``.

The eigenvalues are held in two ways.  (1) The bracket property itself, through ``sturm_count`` on the scaled matrix:
with tol_j = max(2 eps |w_j|, pivmin), the stopping tolerance, count(w_j - tol_j) <= n-1-j < count(w_j + tol_j).  The
bisection ends with a bracket no wider than that tolerance around the midpoint it returns, so both ends lie inside
[w - tol, w + tol]; a bisection that stops rounds early, or returns an end of a wider bracket, fails this.  (2) Against
``eigvalsh_tridiagonal`` within 4 u_T, u_T = n eps |T|_1: 3 for LAPACK, whose worst measured error here is 2.84 u_T (the
n = 3 case, where the restatement agrees with a 40-digit solve to the last bit; 0.27 u_T at most on the others), and 1
for the restatement's own stopping tolerance and the backward error of the Sturm recurrence (a few eps |T|_1)."""
import numpy as np
import pytest

from cnmf_amd import preprocess as pp
from tests import _tridiag_eig_ref as er
from tests import _tridiag_ref as ref

F = ref.DEVICE_FACTOR
LAPACK_UNITS = 4.0


def lapack_eigvals(d, e):
    from scipy.linalg import eigvalsh_tridiagonal
    return np.array(d, dtype=np.float64) if len(d) == 1 else eigvalsh_tridiagonal(d, e)


def test_the_names_are_those_of_the_cases():
    assert er.CASE_NAMES == tuple(c[0] for c in ref.cases())
    assert er.EXTRA_NAMES == tuple(c[0] for c in er.extras())


@pytest.mark.parametrize("name", ["n65_poisson", "n65_clustered", "glued_wilkinson", "graded", "tridiagonal"])
def test_sturm_count_counts_the_eigenvalues_below(name):
    d, e, _ = er.tridiagonal(name)
    ds, es, e2, shift, pivmin, lo0, hi0, snorm = er.scale_and_bounds(d, e)
    lam = lapack_eigvals(ds, es)
    rs = np.random.RandomState(3)
    x = rs.uniform(lo0, hi0, 200)
    x = x[np.abs(x[:, None] - lam[None, :]).min(axis=1) > 64 * len(d) * er.EPS * snorm]     # away from eigenvalues
    assert x.size > 50
    got = er.sturm_count(ds, e2, pivmin, x)
    assert np.array_equal(got, (lam[None, :] < x[:, None]).sum(axis=1))
    assert er.sturm_count(ds, e2, pivmin, np.array([lo0]))[0] == 0
    assert er.sturm_count(ds, e2, pivmin, np.array([hi0]))[0] == len(d)


@pytest.mark.parametrize("name", er.ALL_NAMES)
def test_eigenvalues_and_contracts(name):
    d, e, k = er.tridiagonal(name)
    n = len(d)
    w, Z, ok, ratios, rounds = er.solved(name)
    assert rounds < er.MAX_ROUNDS and np.all(np.diff(w) <= 0)
    ds, es, e2, shift, pivmin, lo0, hi0, snorm = er.scale_and_bounds(d, e)
    if snorm:                                                        # (1) the bracket property at the stopping tolerance
        ws = np.ldexp(w, shift)
        tol = np.maximum(2.0 * er.EPS * np.abs(ws), pivmin)
        target = n - 1 - np.arange(k)
        below, above = er.sturm_count(ds, e2, pivmin, ws - tol), er.sturm_count(ds, e2, pivmin, ws + tol)
        assert np.all(below <= target) and np.all(target < above), (below, target, above)
    T_u = ref.unit(ref.tridiagonal_matrix(d, e))                     # (2) LAPACK
    err = np.abs(w - lapack_eigvals(d, e)[::-1][:k])
    print("%s: %d rounds, check %s, eigenvalues off LAPACK's by %.3g u_T" % (name, rounds, ["%.3g" % r for r in ratios],
                                                                           (err / T_u).max() if T_u else err.max()))
    assert np.all(err <= LAPACK_UNITS * T_u)
    assert ok and ratios[0] <= er.ACCEPT and ratios[2] <= er.ACCEPT
    res, orth = er.t_contracts(d, e, w, Z)
    assert res <= F and orth <= F


@pytest.mark.parametrize("name", er.CASE_NAMES)
def test_contracts_through_the_back_transformation(name):
    A, k, d, e, R, tau = er.case_reduction(name)
    w, Z, ok, ratios, _ = er.solved(name)
    V = ref.back_transform(R, tau, Z, rule=True)
    res, eig, orth, desc = ref.contracts(A, w, V)
    print("%s: residual %.3g u, eigenvalues %.3g u, orthogonality %.3g n eps" % (name, res, eig, orth))
    assert ok and res <= F and eig <= F and orth <= F and desc


def test_scaling_by_powers_of_two_changes_nothing_but_the_exponent():
    w0, Z0 = er.solved("n65_poisson")[:2]
    for p in (300, -300):
        w, Z = er.solved("n65_poisson_2^%d" % p)[:2]
        assert np.array_equal(w, np.ldexp(w0, p)) and np.array_equal(Z, Z0)


def test_zero_matrix_and_start_vector():
    w, Z, ok, ratios, rounds = er.eigh_top(np.zeros(5), np.zeros(4), 3)
    assert ok and rounds == 0 and not w.any() and np.array_equal(Z, np.eye(5)[:, :3])
    y = er.start_vector(100, 70)
    assert np.abs(y).max() < 1.0 and abs(y.mean()) < 0.05 and len(np.unique(y)) == y.size


def test_fuzz_accepted_results_meet_the_contracts_and_rejected_ones_are_rescued():
    fuzz = er.fuzz()
    assert len(fuzz) == 400 and max(len(d) for _, d, _, _ in fuzz) < 48
    rejected, worst = [], np.zeros(3)
    for kind, d, e, k in fuzz:
        w, Z, ok, ratios, _ = er.eigh_top(d, e, k)
        u = ref.unit(ref.tridiagonal_matrix(d, e))
        lam = lapack_eigvals(d, e)[::-1][:k]
        assert np.abs(w - lam).max() <= F * u                        # (the eigenvalues are valid either way)
        if not ok:
            rejected.append(kind)
            w, Z = pp.tridiagonal_top(d, e, k)                       # the fallback
        else:
            worst = np.maximum(worst, ratios)
        res, orth = er.t_contracts(d, e, w, Z)
        assert res <= F and orth <= F, (kind, ok, res, orth)
    print("rejected %d of %d (%s); worst accepted: residual %.3g u_T, rayleigh %.3g u_T, orthogonality %.3g n eps"
          % (len(rejected), len(fuzz), sorted(set(rejected)), *worst))
    assert set(rejected) <= {"integer_diagonal"}
    assert 1 <= len(rejected) <= len(fuzz) // 10                     # (the GPU test of the fallback takes one of them)
    kind, d, e, k, ratios = er.fuzz_rejected()
    assert kind == "integer_diagonal" and max(ratios[0], ratios[2]) > er.ACCEPT


def test_pca_device_full_is_a_mode_and_bogus_is_not():
    """fails on a tree without the feature: "device_full" is refused there"""
    assert "device_full" in pp.PCA_MODES
    pp._check_pca_mode("device_full")
    P = pp.Preprocess()
    X = np.ones((4, 3))
    with pytest.raises(ValueError, match="pca must be one of"):
        P.normalize_batchcorrect(X, highly_variable=np.ones(3, dtype=bool), pca="bogus")
    with pytest.raises(ValueError, match="pca must be one of"):
        P.preprocess_for_cnmf(X, highly_variable=np.ones(3, dtype=bool), pca="bogus")
    assert P._engine is None
    with pytest.raises(NotImplementedError, match='pca="lapack"'):
        pp._check_pca_size("device_full", pp.PCA_NMAX + 1)
    pp._check_pca_size("device_full", pp.PCA_NMAX)
