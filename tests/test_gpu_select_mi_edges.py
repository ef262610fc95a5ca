"""cnmf_preprocess_select_mi on the paths the fixture tests never enter: the second class-partition pass (more than 256
kept classes), the gene-chunk loop past its first chunk, every n_neighbors from 1 to 8 on both sides of sklearn's
brute / tree switch, degenerate columns, the tile edges of the segmented sort and a single class.

Every case calls Engine.preprocess_select_mi directly and compares with sklearn's own _compute_mi_cd on noise built
on the host (tests/_mi_ref.py).  The inputs are real-valued, so no two cells tie: a noise value one ulp off (the device's
log() against the host's) cannot change an order comparison, and every compared gene must have sklearn's bits
(tests/test_host_mi_reference.py keeps that premise checked).  The cap on differing genes is 0."""
import numpy as np
import pytest

from cnmf_amd.preprocess import mi_classes
from tests._mi_ref import assert_state_equal, device_mi, host_noise, psi_table, sklearn_mi

pytestmark = pytest.mark.gpu
MI_TILE = 2048                       # select_mi_host.hip.h
CHUNK_ELEMS = 1 << 25


def state_for(seed):
    return np.random.RandomState(seed).get_state()


def shifted_gamma(rs, labels, G):
    """gamma values with a class-dependent shift in every other gene, so that MI is not all zero"""
    _, inv = np.unique(labels, return_inverse=True)
    X = rs.gamma(0.5, 1.0, size=(labels.size, G))
    shift = rs.rand(inv.max() + 1, G) * 2.0
    shift[:, 1::2] = 0.0
    return X + shift[inv]


def assert_bits(engine, X, labels, K, picks, seed=4):
    state = state_for(seed)
    mi, fin = device_mi(engine, X, labels, K, state)
    Xn, want_state = host_noise(X, state)
    assert_state_equal(fin, want_state)
    picks = np.asarray(picks)
    ref = sklearn_mi(Xn, labels, K, picks)
    same = mi[picks].view(np.uint64) == ref.view(np.uint64)
    print("K", K, "bit-equal", int(same.sum()), "of", picks.size, "max diff", np.abs(mi[picks] - ref).max(),
          "max MI", ref.max())
    assert same.all(), (K, picks[~same], mi[picks][~same], ref[~same])
    assert np.all(mi >= 0)
    return mi, ref


# ---------------------------------------------------------------- more than 256 classes: the second partition pass
@pytest.mark.parametrize("n_kept", [256, 257, 300])
def test_many_classes(engine, n_kept):
    rs = np.random.RandomState(n_kept)
    N, G, n_single = 3000, 64, 5
    sizes = 2 + rs.multinomial(N - n_single - 2 * n_kept, np.ones(n_kept) / n_kept)
    labels = np.concatenate([np.repeat(np.arange(n_kept), sizes), 10000 + np.arange(n_single)])
    labels = labels[rs.permutation(N)]                           # class ids in shuffled cell order
    cls, n_cls, _ = mi_classes(labels, 3)
    assert n_cls == n_kept and (cls == -1).sum() == n_single
    X = shifted_gamma(rs, labels, G)
    picks = [0, 1, 2, 3, 17, 30, 31, 32, 33, 62, 63, 40]
    _, ref = assert_bits(engine, X, labels, 3, picks)
    assert ref.max() > 0.05


# ---------------------------------------------------------------- more than one gene chunk, a ragged last one
def test_gene_chunks(engine):
    N, G, n_classes = 50000, 700, 8
    rs = np.random.RandomState(21)
    labels = rs.randint(0, n_classes, size=N)
    Gc = max(1, min(G, CHUNK_ELEMS // N))                        # all cells are kept
    assert Gc < G and G % Gc not in (0, Gc) and G - Gc < Gc, Gc  # two chunks, the second shorter
    X = shifted_gamma(rs, labels, G)
    picks = [0, 5, 300, Gc - 2, Gc - 1, Gc, Gc + 1, Gc + 13, G - 2, G - 1]
    mi, ref = assert_bits(engine, X, labels, 3, picks)
    assert ref[[0, 4, 6, 8]].min() > 0.01                        # odd genes carry no signal, these (even) do
    # a gene of the second chunk read from the first chunk's columns (j0 ignored) would repeat the value of gene j - Gc
    assert np.all(mi[Gc:] != mi[:G - Gc])


# ---------------------------------------------------------------- n_neighbors 1..8 across the brute / tree switch
def switch_sizes(K):
    return [2, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 2 * K + 2, 2 * K + 3]


def interleaved(sizes, rs):
    labels = np.repeat(np.arange(len(sizes)), sizes)
    return labels[rs.permutation(labels.size)]


@pytest.mark.parametrize("K", range(1, 9))
def test_every_n_neighbors_across_the_switch(engine, K):
    """sklearn fits each class with min(K, cn - 1) neighbours and takes the brute path when that is >= cn // 2: class
    sizes on both sides of it (a size below 2 is a dropped singleton), with and without a large class beside them.
    Without it the cells number 12 K + 8 <= 104, and a wrong radius in one cell moves MI visibly."""
    rs = np.random.RandomState(100 + K)
    sizes = switch_sizes(K)
    sides = {min(K, cn - 1) >= cn // 2 for cn in sizes if cn >= 2}
    assert sides == {True, False}
    for extra in ([], [400]):
        labels = interleaved(sizes + extra, rs)
        assert extra or labels.size <= 104
        X = shifted_gamma(rs, labels, 24)
        assert_bits(engine, X, labels, K, np.arange(24), seed=K)


@pytest.mark.parametrize("K", [0, 9])
def test_n_neighbors_outside_1_to_8_is_refused(engine, K):
    labels = np.arange(40) % 2
    X = np.random.RandomState(0).gamma(0.5, 1.0, size=(40, 3))
    cls, n_cls, cst = mi_classes(labels, 3)
    engine.preprocess_set_dense(0, X)
    try:
        with pytest.raises(ValueError, match=r"n_neighbors = %d outside \[1, 8\]" % K):
            engine.preprocess_select_mi(0, cls, n_cls, K, state_for(0), psi_table(40), cst)
    finally:
        engine.preprocess_release()


# ---------------------------------------------------------------- degenerate columns
@pytest.mark.parametrize("K", [1, 3, 8])
def test_degenerate_columns(engine, K):
    rs = np.random.RandomState(31)
    labels = interleaved([2, 3, 7, 16, 17, 300, 500], rs)
    N = labels.size
    X = shifted_gamma(rs, labels, 8)
    X[:, 0] = 0.0                                   # all zero: sd = 0 -> scale 1, the values are the noise alone
    X[:, 1] = 4.25                                  # constant: the same
    X[:, 2] = 0.0
    X[N // 3, 2] = 9.0                              # one non-zero entry
    X[:, 3] = 1e4 + rs.gamma(0.5, 1.0, size=N)      # mean |x| / sd ~ 1e4: the noise scale takes the mean branch
    X[:, 4] = 1e4 + X[:, 6]                         # the same with signal
    sd = X.std(axis=0)
    assert sd[0] == 0 and sd[1] == 0 and np.abs(X[:, 3]).mean() / sd[3] > 1e3
    mi, _ = assert_bits(engine, X, labels, K, np.arange(8), seed=K)
    assert np.all(mi >= 0)


# ---------------------------------------------------------------- the tile edges of the sort
@pytest.mark.parametrize("n_kept", [200, MI_TILE - 1, MI_TILE, MI_TILE + 1, 2 * MI_TILE + 1])
@pytest.mark.parametrize("n_classes", [2, 3])
def test_sort_tile_edges(engine, n_kept, n_classes):
    rs = np.random.RandomState(n_kept + n_classes)
    sizes = [n_kept - (n_classes - 1) * (n_kept // 4)] + [n_kept // 4] * (n_classes - 1)
    labels = np.concatenate([interleaved(sizes, rs), [500, 501, 502]])      # three dropped singletons
    labels = labels[rs.permutation(labels.size)]
    cls, n_cls, _ = mi_classes(labels, 3)
    assert (cls >= 0).sum() == n_kept and n_cls == n_classes
    X = shifted_gamma(rs, labels, 6)
    assert_bits(engine, X, labels, 3, np.arange(6))


# ---------------------------------------------------------------- one class only
@pytest.mark.parametrize("N", [2, 7, 3000])
def test_one_class(engine, N):
    rs = np.random.RandomState(N)
    labels = np.zeros(N, dtype=np.int64)
    X = rs.gamma(0.5, 1.0, size=(N, 5))
    cls, n_cls, _ = mi_classes(labels, 3)
    assert n_cls == 1
    assert_bits(engine, X, labels, 3, np.arange(5))
