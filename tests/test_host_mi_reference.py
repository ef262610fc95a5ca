"""The premises of the GPU edge tests, checked on the host.

1. Why test_gpu_select_mi_edges.py can ask for bit equality.  The device's log() may differ from the host's by one ulp
   in a noise draw.  With count data equal counts tie and the 1e-10 noise alone orders them, so one ulp can move a
   neighbour count (the slack the fixture tests allow).  With real-valued data the noise decides no comparison, and
   sklearn's estimate keeps its bits when every draw moves by -1 / 0 / +1 ulp.
2. tests/_pre_ref.py's restatement of pre_splits against shapes worked by hand from csrc/preprocess_host.hip.h.
3. The error bound of test_gpu_preprocess_edges.py is one a correct float64 product meets: numpy's own A @ B stays
   inside it on the sweep's operands, the high-mean columns included."""
import numpy as np
import pytest

from tests import _pre_ref as ref
from tests._mi_ref import host_noise, sklearn_mi

LD = ref.LD


# ---------------------------------------------------------------- 1. one ulp of noise
def mi_changes(X, labels, K):
    state = np.random.RandomState(4).get_state()
    perturb = np.random.RandomState(5).randint(-1, 2, size=X.shape).astype(np.int8)
    picks = np.arange(X.shape[1])
    a = sklearn_mi(host_noise(X, state)[0], labels, K, picks)
    b = sklearn_mi(host_noise(X, state, perturb=perturb)[0], labels, K, picks)
    return int((a.view(np.uint64) != b.view(np.uint64)).sum()), float(np.abs(a - b).max())


def test_one_ulp_of_noise_moves_counts_but_not_real_values():
    rs = np.random.RandomState(12)
    N, G = 400, 8
    labels = rs.randint(0, 40, size=N)
    real = rs.gamma(0.5, 1.0, size=(N, G)) + (labels % 4)[:, None] * 0.5
    counts = rs.poisson(rs.gamma(0.4, 2.0, size=G), size=(N, G)).astype(np.float64)
    moved = 0
    for K in (1, 3, 8):
        changed, diff = mi_changes(real, labels, K)
        assert (changed, diff) == (0, 0.0), (K, changed, diff)
        moved += mi_changes(counts, labels, K)[0]
    assert moved >= 1


# ---------------------------------------------------------------- 2. pre_splits
@pytest.mark.parametrize("M, Nn, K, S, kps", [
    (100, 100, 300, 1, 304),          # the fixture's scatter: 4 tiles, 300 / 256 = 1 split
    (300, 50, 100, 1, 112),           # the fixture's scores: K below 256
    (40, 100, 300, 1, 304),           # the fixture's ridge moments
    (500, 2000, 50000, 8, 6256),      # full-size ridge moments: 256 tiles -> 8 splits, 7 x 6256 + 6208
    (500, 5, 50000, 16, 3136),        # its Gram: 8 tiles -> 16 splits of ceil(3125 / 16) * 16, tail 2960
    (130, 130, 4097, 16, 272),        # 9 tiles; ceil(4097 / 16) = 257 -> 272; 15 x 272 + 17
    (65, 65, 20011, 16, 1264),        # 4 tiles; ceil(20011 / 16) = 1251 -> 1264; 15 x 1264 + 1051
    (257, 65, 530, 2, 272),           # scores over 530 genes: 530 / 256 = 2; 265 -> 272; 272 + 258
    (1, 1, 1, 1, 16),                 # kps never below one k step
    (2000, 2000, 50000, 2, 25008),    # 1024 tiles -> 2048 / 1024 = 2 splits
    (4096, 4096, 100000, 1, 100000),  # 4096 tiles -> no split; 100000 is a multiple of 16
    (64, 64, 511, 1, 512),            # 511 / 256 = 1
    (64, 64, 512, 2, 256),            # the first K with two splits
])
def test_pre_splits_restatement(M, Nn, K, S, kps):
    assert ref.pre_splits(M, Nn, K) == (S, kps)
    assert (S - 1) * kps < K <= S * kps and kps % 16 == 0


def test_the_sweep_has_ragged_splits():
    assert ref.ragged_split(130, 130, 4097) and ref.ragged_split(65, 65, 20011) and ref.ragged_split(257, 65, 530)
    assert not ref.ragged_split(500, 2000, 50000)       # tail 6208 = 388 x 16: the shape the older test runs
    for name, shape in ref.PRODUCT_SHAPES.items():
        assert any(ref.ragged_split(*shape(*c)) for c in ref.CASES), name


# ---------------------------------------------------------------- 3. the bound holds for a correct float64 product
def inside(got, want, bound):
    return bool(np.all(np.abs(got.astype(LD) - want).astype(np.float64) <= bound))


@pytest.mark.parametrize("case", [c for c in ref.CASES if c[0] * c[1] <= 4097 * 130])
def test_numpy_float64_products_meet_the_bound(case):
    N, G, n_comp, K, B1 = case
    X = ref.make_X(N, G, seed=N + G)
    mean = X.mean(axis=0)
    assert inside(mean, X.astype(LD).sum(axis=0) / N, ref.gemm_bound(N, np.abs(X).sum(axis=0) / N))
    A64, Al = X - mean, X.astype(LD) - mean.astype(LD)
    want, mag = ref.ld_product(Al.T, Al)
    assert inside(A64.T @ A64, want, ref.gemm_bound(N, mag))
    V = ref.make_V(G, n_comp, seed=N + G)
    want, mag = ref.ld_product(Al, V)
    assert inside(A64 @ V, want, ref.gemm_bound(G, mag))
    R, Phi = ref.make_ridge(N, K, B1, seed=N + G)
    P64 = (R[:, None, :] * Phi[None, :, :]).reshape(K * B1, N)
    Pl = ref.ridge_operand(R, Phi)
    want, mag = ref.ld_product(Pl, X)
    assert inside(P64 @ X, want, ref.gemm_bound(N, mag))
    want, mag = ref.ld_product(Pl, Phi.T)
    assert inside(P64 @ Phi.T, want, ref.gemm_bound(N, mag))
    W = ref.make_W(K, B1, G, seed=N + G).reshape(K * B1, G)
    prod, mag = ref.ld_product(Pl.T, W)
    want = np.maximum(X.astype(LD) - prod, 0)
    bound = ref.gemm_bound(K * B1, mag) + ref.U * np.abs(want).astype(np.float64)
    assert inside(np.maximum(X - P64.T @ W, 0), want, bound)


def test_a_mean_subtracted_after_the_sum_misses_the_bound():
    """the cancellation the high-mean columns are there for: sum x x' - N mean mean' is outside the bound"""
    N, G = 4097, 65
    X = ref.make_X(N, G, seed=N + G)
    mean = X.mean(axis=0)
    Al = X.astype(LD) - mean.astype(LD)
    want, mag = ref.ld_product(Al.T, Al)
    late = X.T @ X - N * np.outer(mean, mean)
    assert not inside(late, want, ref.gemm_bound(N, mag))
