"""The Preprocess device kernels on the paths the pipeline tests never enter.

1. pre_gemm_kernel's four generated-operand products (scatter, PCA scores, ridge moments + Gram, ridge apply) against
   the same operands and product formed in long double, over shapes taken from the kernel's constants (tests/_pre_ref.py):
   output dimensions below, at and one past a 64-tile, k extents below and past the 16-deep step, and split-K with a last
   slice that is not a multiple of 16.  The tolerance is the a-priori bound of a float64 dot product, elementwise.
   The ridge apply has no split-K (one pass over K (B + 1) <= 512); its ragged k tail is K (B + 1) % 16 != 0.
2. cnmf_preprocess_order_stats against np.partition, bit for bit, and the ceiling built on it."""
import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd.preprocess import stdscale_quantile_celing
from tests import _pre_ref as ref

pytestmark = pytest.mark.gpu
LD = ref.LD
CASE_IDS = ["N%d-G%d-c%d-K%d-B%d" % c for c in ref.CASES]


def staged(engine, X):
    engine.preprocess_set_dense(0, X)


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


def check(got, want, bound, what):
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s: max err %.3e, bound there %.3e, worst ratio %.3f" % (
        what, err[worst], bound[worst], np.max(err / np.where(bound > 0, bound, 1.0))))
    assert np.all(err <= bound), (what, worst, float(err[worst]), float(bound[worst]))


def test_the_sweep_covers_what_it_claims():
    """every listed value appears, and every split product has a case with S > 1 and a ragged last slice"""
    Ns, Gs, cs, KBs = (set(v) for v in zip(*[(c[0], c[1], c[2], (c[3], c[4])) for c in ref.CASES]))
    assert {1, 15, 17, 255, 257, 511, 4097, 20011} <= Ns
    assert {1, 63, 64, 65, 130} <= Gs
    assert {1, 50, 65} <= cs
    assert {(1, 1), (3, 2), (7, 5), (13, 5)} <= KBs
    for name, shape in ref.PRODUCT_SHAPES.items():
        assert any(ref.ragged_split(*shape(*c)) for c in ref.CASES), name
    # the apply runs in one pass; its k extent must leave a partial 16-step after at least one full one
    assert any(c[3] * c[4] > 16 and (c[3] * c[4]) % 16 for c in ref.CASES)
    assert all(c[3] * c[4] <= 512 for c in ref.CASES)


# ---------------------------------------------------------------- 1. the four products
@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_scatter_and_means(engine, case):
    N, G, _, _, _ = case
    X = ref.make_X(N, G, seed=N + G)
    staged(engine, X)
    mean, S = engine.preprocess_scatter(0)
    Xl = X.astype(LD)
    check(mean, Xl.sum(axis=0) / N, ref.gemm_bound(N, np.abs(X).sum(axis=0) / N), "mean")
    # the operand is X minus the mean the device holds (the one it returned), rounded once
    A = Xl - mean.astype(LD)
    want, mag = ref.ld_product(A.T, A)
    check(S, want, ref.gemm_bound(N, mag), "scatter")
    assert np.all(S[3::4] == 0) and np.all(S[:, 3::4] == 0)        # the all-zero columns
    if G > 1 and N > 16:
        # a mean subtracted after the sum would be off by ~ 1e6^2 N u here, far above the bound
        assert ref.gemm_bound(N, mag)[1, 1] < 1e-6 * N * (1e6 ** 2) * ref.U


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_project(engine, case):
    N, G, n_comp, _, _ = case
    X = ref.make_X(N, G, seed=N + G)
    mean = X.mean(axis=0)
    V = ref.make_V(G, n_comp, seed=N + G)
    staged(engine, X)
    got = engine.preprocess_project(0, mean, V)
    want, mag = ref.ld_product(X.astype(LD) - mean.astype(LD), V)
    check(got, want, ref.gemm_bound(G, mag), "scores")


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_ridge_moments_and_apply(engine, case):
    N, G, _, K, B1 = case
    X = ref.make_X(N, G, seed=N + G)
    X[:, 1::4] -= 1e6 - 3.0            # the correction works on scaled data; keep a shifted column, drop the 1e6
    R, Phi = ref.make_ridge(N, K, B1, seed=N + G)
    staged(engine, X)
    M, gram = engine.preprocess_ridge_moments(0, R, Phi)
    A = ref.ridge_operand(R, Phi)
    want, mag = ref.ld_product(A, X)
    check(M.reshape(K * B1, G), want, ref.gemm_bound(N, mag), "moments")
    want, mag = ref.ld_product(A, Phi.T)
    check(gram.reshape(K * B1, B1), want, ref.gemm_bound(N, mag), "gram")
    W = ref.make_W(K, B1, G, seed=N + G)
    engine.preprocess_ridge_apply(0, W)
    got = engine.preprocess_fetch(0)
    prod, mag = ref.ld_product(A.T, W.reshape(K * B1, G))
    unclipped = X.astype(LD) - prod
    want = np.maximum(unclipped, 0)
    bound = ref.gemm_bound(K * B1, mag) + ref.U * np.abs(want).astype(np.float64)
    check(got, want, bound, "apply")
    far = np.abs(unclipped).astype(np.float64) > bound
    assert np.array_equal(got[far] == 0, want[far] == 0)
    assert (got[far] == 0).any() or N * G < 64, "the clip is not exercised"
    assert np.all(got >= 0)


def _split_case(name):
    return next(c for c in ref.CASES if ref.ragged_split(*ref.PRODUCT_SHAPES[name](*c)))


def test_two_calls_give_the_same_bits(engine):
    """at one split-K shape per product"""
    def bits(a):
        return np.ascontiguousarray(a).view(np.uint64)

    N, G, _, _, _ = _split_case("scatter")
    X = ref.make_X(N, G, seed=1)
    staged(engine, X)
    a, b = engine.preprocess_scatter(0), engine.preprocess_scatter(0)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))

    N, G, n_comp, _, _ = _split_case("project")
    X = ref.make_X(N, G, seed=2)
    V = ref.make_V(G, n_comp, seed=2)
    staged(engine, X)
    a, b = engine.preprocess_project(0, X.mean(axis=0), V), engine.preprocess_project(0, X.mean(axis=0), V)
    assert np.array_equal(bits(a), bits(b))

    case = _split_case("moments")
    assert ref.ragged_split(*ref.PRODUCT_SHAPES["gram"](*case))
    N, G, _, K, B1 = case
    X = ref.make_X(N, G, seed=3)
    R, Phi = ref.make_ridge(N, K, B1, seed=3)
    W = ref.make_W(K, B1, G, seed=3)
    outs = []
    for _ in range(2):
        staged(engine, X)
        M, gram = engine.preprocess_ridge_moments(0, R, Phi)
        engine.preprocess_ridge_apply(0, W)
        outs.append((M, gram, engine.preprocess_fetch(0)))
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- 2. order statistics and the ceiling
def assert_ranks(engine, values, ks, bits=True):
    """preprocess_order_stats(0, k) against np.partition of all the slot's values"""
    flat = np.asarray(values, dtype=np.float64).reshape(-1)
    n = flat.size
    for k in ks:
        k = int(k)
        k1 = min(k + 1, n - 1)
        want = np.partition(flat, sorted({k, k1}))[[k, k1]]
        got = np.array(engine.preprocess_order_stats(0, k))
        if bits:
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (k, got, want)
        else:
            assert np.array_equal(got, want), (k, got, want)


def test_order_stats_all_equal_and_two_values(engine):
    X = np.full((37, 11), 2.5)
    staged(engine, X)
    assert_ranks(engine, X, [0, 1, 200, X.size - 2, X.size - 1])
    X = np.full((40, 10), 7.0)
    X.reshape(-1)[::3] = 0.125                       # 134 low values
    n_low = int((X == 0.125).sum())
    staged(engine, X)
    assert_ranks(engine, X, [0, n_low - 2, n_low - 1, n_low, X.size - 1])


def exponent_range_values():
    """non-negative doubles over the whole exponent range, and for every byte of the key a run of values whose keys
    differ first in that byte"""
    rs = np.random.RandomState(8)
    keys = [rs.randint(0, 0x7FF0000000000000, size=3000, dtype=np.int64).astype(np.uint64)]
    for b in range(8):
        base = np.uint64(0x3FF0000000000000 if b < 6 else 0)
        top = 200 if b < 7 else 0x7F
        keys.append(base + (np.arange(1, top, dtype=np.uint64) << np.uint64(8 * b)))
    v = np.concatenate(keys).view(np.float64)
    v = np.concatenate([v, [0.0, 5e-324, 2.2250738585072014e-308, 1e300, 1e-300, 1.0]])
    return v[np.isfinite(v)]


def test_order_stats_whole_exponent_range(engine):
    v = exponent_range_values()
    rs = np.random.RandomState(9)
    v = v[rs.permutation(v.size)]
    v = v[:v.size // 7 * 7]
    s = np.sort(v).view(np.uint64)
    diff = s[1:] ^ s[:-1]
    deciding = {int(d).bit_length() - 1 >> 3 for d in diff if d}
    assert deciding == set(range(8)), deciding        # every radix byte separates two neighbours somewhere
    assert (v < 2.2250738585072014e-308).sum() > 1 and v.max() >= 1e300
    X = v.reshape(-1, 7)
    staged(engine, X)
    assert_ranks(engine, X, np.r_[0, 1, v.size - 2, v.size - 1, np.arange(3, v.size, 97)])


def test_order_stats_single_value_and_extreme_ranks(engine):
    X = np.array([[3.25]])
    staged(engine, X)
    assert_ranks(engine, X, [0])
    X = np.random.RandomState(1).gamma(0.5, 1.0, size=(123, 9))
    staged(engine, X)
    assert_ranks(engine, X, [0, X.size - 1])
    with pytest.raises(ValueError, match="rank"):
        engine.preprocess_order_stats(0, X.size)


def test_order_stats_csr_implicit_zeros_boundary(engine):
    rs = np.random.RandomState(2)
    X = sp.random(211, 17, density=0.2, random_state=rs, format="csr")
    X.data = rs.gamma(0.5, 1.0, size=X.nnz) + 1e-3
    engine.preprocess_upload(X)
    engine.preprocess_select(0, np.arange(17), 0.0, None)
    Y = engine.preprocess_fetch(0)
    assert sp.issparse(Y) and Y.nnz == X.nnz
    zeros = 211 * 17 - Y.nnz
    assert_ranks(engine, Y.toarray(), [0, zeros - 2, zeros - 1, zeros, zeros + 1, 211 * 17 - 1])


def test_order_stats_dense_with_explicit_zeros(engine):
    rs = np.random.RandomState(3)
    X = rs.gamma(0.5, 1.0, size=(150, 20))
    X[rs.rand(150, 20) < 0.4] = 0.0
    zeros = int((X == 0).sum())
    staged(engine, X)
    assert_ranks(engine, X, [0, zeros - 1, zeros, X.size // 2, X.size - 1])


def test_order_stats_more_values_than_one_grid_pass(engine):
    n = 8192 * 256 + 1
    rows = -(-n // 1024)
    X = np.random.RandomState(4).gamma(0.5, 1.0, size=(rows, 1024))
    assert X.size >= n
    staged(engine, X)
    assert_ranks(engine, X, [0, 12345, X.size // 2, int(0.9999 * (X.size - 1)), X.size - 1])


def test_negative_zero_ranks_with_zero(engine):
    rs = np.random.RandomState(5)
    X = rs.gamma(0.5, 1.0, size=(90, 12))
    X[rs.rand(90, 12) < 0.2] = 0.0
    X[rs.rand(90, 12) < 0.2] = -0.0
    n_neg0 = int((np.signbit(X)).sum())
    zeros = int((X == 0).sum())
    assert 0 < n_neg0 < zeros
    staged(engine, X)
    # the device returns +0.0 for such a rank; it compares equal to numpy's zero of either sign
    assert_ranks(engine, X, [0, n_neg0 - 1, n_neg0, zeros - 1, zeros, X.size // 2, X.size - 1], bits=False)
    lo, hi = engine.preprocess_order_stats(0, 0)
    assert not np.signbit(lo) and not np.signbit(hi)
    engine.preprocess_release()
    for q in (0.0, 0.3, 0.5, 0.97, 1.0):
        pre = X / X.std(axis=0, ddof=1)
        want = np.minimum(pre, np.quantile(pre.reshape(-1), q))
        got = stdscale_quantile_celing(X, quantile_thresh=q, engine=engine)
        assert np.abs(got - want).max() <= 1e-12 * want.max() and np.array_equal(got == 0, want == 0), q
        pre_dev = stdscale_quantile_celing(X, quantile_thresh=None, engine=engine)
        assert np.array_equal(got, np.minimum(pre_dev, np.quantile(pre_dev.reshape(-1), q))), q


def test_a_negative_entry_is_still_refused(engine):
    X = np.random.RandomState(6).gamma(0.5, 1.0, size=(50, 6))
    X[7, 3] = -1e-300
    X[9, 1] = -0.0
    staged(engine, X)
    with pytest.raises(ValueError, match=r"the quantile ceiling needs values >= 0 \(1 negative\)"):
        engine.preprocess_order_stats(0, 10)
