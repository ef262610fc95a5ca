"""Host side of the Preprocess edge tests (test_gpu_preprocess_edges.py, test_host_mi_reference.py): a restatement of
pre_splits (csrc/preprocess_host.hip.h), the sweep's shapes and operands, the four products in long double and the
error bound a float64 product has to meet.

The shapes come from the kernel's constants: 64 x 64 output tiles, k steps of 16, split-K with at most 16 splits of at
least 256 k each, the k per split rounded up to a multiple of 16."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def pre_splits(M, Nn, K):
    """(S, kps) of an M x Nn product over K, as pre_splits computes them"""
    tiles = ((M + 63) // 64) * ((Nn + 63) // 64)
    S = max(1, min(16, 2048 // max(1, tiles)))
    S = max(1, min(S, K // 256))
    kps = (K + S - 1) // S
    kps = max(16, (kps + 15) // 16 * 16)
    return (K + kps - 1) // kps, kps


def ragged_split(M, Nn, K):
    """more than one split, and a last slice that is not a multiple of the 16-deep k step"""
    S, kps = pre_splits(M, Nn, K)
    return S > 1 and (K - (S - 1) * kps) % 16 != 0


# (cells N, genes G, PCA components, clusters K, covariates B + 1)
CASES = [
    (1, 1, 1, 1, 1),
    (15, 63, 50, 3, 2),
    (17, 64, 1, 7, 5),
    (255, 65, 65, 13, 5),
    (257, 130, 50, 1, 1),
    (511, 64, 50, 3, 2),
    (4097, 130, 65, 7, 5),       # scatter, moments and Gram: 16 splits of 272 cells, a tail of 17
    (20011, 65, 50, 13, 5),      # scatter, moments and Gram: 16 splits of 1264 cells, a tail of 1051
    (257, 530, 65, 3, 2),        # scores: 2 splits of 272 genes, a tail of 258
]
# the shapes of each product, (M, Nn, K) from a case
PRODUCT_SHAPES = {
    "scatter": lambda N, G, c, K, B1: (G, G, N),
    "project": lambda N, G, c, K, B1: (N, c, G),
    "moments": lambda N, G, c, K, B1: (K * B1, G, N),
    "gram": lambda N, G, c, K, B1: (K * B1, B1, N),
}


def make_X(N, G, seed):
    """gamma values; every fourth column from 1 sits at 1e6 times its spread (a mean subtracted after the sum instead of
    before loses 6 digits there), every fourth column from 3 is all zeros"""
    rs = np.random.RandomState(seed)
    X = rs.gamma(0.5, 1.0, size=(N, G))
    X[:, 1::4] += 1e6
    X[:, 3::4] = 0.0
    return X


def make_ridge(N, K, B1, seed):
    """soft cluster memberships R [K][N] (columns sum to 1) and the design Phi [B1][N]: intercept + one-hot batches"""
    rs = np.random.RandomState(seed + 1000)
    logits = rs.randn(K, N) * 2
    R = np.exp(logits - logits.max(axis=0))
    R /= R.sum(axis=0)
    batch = rs.randint(0, max(B1 - 1, 1), size=N)
    Phi = np.vstack([np.ones(N)] + [(batch == b).astype(np.float64) for b in range(B1 - 1)])
    return R, Phi


def make_V(G, n_comp, seed):
    return np.random.RandomState(seed + 2000).randn(G, n_comp)


def make_W(K, B1, G, seed):
    """ridge coefficients of both signs, scaled so that X - A^T W crosses zero in many entries"""
    return np.random.RandomState(seed + 3000).randn(K, B1, G) * 0.7


def ld_product(A, B):
    """A @ B in long double, with its magnitude bound term |A| @ |B| (float64 is plenty for the bound itself)"""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    return A @ B, np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)


def gemm_bound(K, absprod):
    """|fl(A B) - A B| for a length-K float64 dot product in any summation order with one rounding per generated
    operand: (1 + u)^(K + 2) - 1 <= (K + 4) u for K u << 1"""
    return (K + 4) * U * absprod


def ridge_operand(R, Phi):
    """A[(k, b), n] = R[k, n] Phi[b, n] in long double"""
    K, B1, N = R.shape[0], Phi.shape[0], R.shape[1]
    return (R.astype(LD)[:, None, :] * Phi.astype(LD)[None, :, :]).reshape(K * B1, N)
