"""The four filter entry points (csrc/filter_host.hip.h) at their edges, each against the numpy restatement of
tests/_filter_ref.py: equality unless stated.

Shapes come from the kernels' constants: a wavefront takes 64 entries of a row per step (rows of 63, 64, 65 and 129
entries: below, at and past one step, and past two), one scan workgroup covers SCAN_BLOCK = 1024 items (cell counts one
below, at and one above it, and two workgroups plus one)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import _filter_ref as F

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


def edge_matrix(N, G=150, seed=0, zeros=True, shuffle=True):
    """integer counts as stored: row 0 empty, rows 1..4 of exactly 63, 64, 65 and 129 entries, the others random; column
    G - 1 empty; every row's columns in a shuffled order; every seventh stored value an explicit zero"""
    rs = np.random.RandomState(seed + N)
    lens = rs.randint(0, 40, size=N)
    lens[:5] = [0, 63, 64, 65, 129][:min(N, 5)]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([rs.permutation(G - 1)[:n] if shuffle else np.sort(rs.permutation(G - 1)[:n]) for n in lens]
                             + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = rs.randint(1, 20, size=indptr[-1]).astype(np.float64)
    if zeros:
        data[::7] = 0.0
    return sp.csr_matrix((data, indices, indptr), shape=(N, G))


def masks(n, seed):
    rs = np.random.RandomState(seed)
    one = np.ones(n, dtype=bool)
    one[n // 2] = False
    return {"none": None, "all": np.ones(n, dtype=bool), "but_one": one, "alternating": np.arange(n) % 2 == 0,
            "random": rs.rand(n) < 0.5, "first_only": np.arange(n) == 0, "last_only": np.arange(n) == n - 1}


def test_the_inputs_hold_what_they_claim():
    X = edge_matrix(70)
    assert list(np.diff(X.indptr)[:5]) == [0, 63, 64, 65, 129]
    assert (X.data == 0).any() and not X.has_sorted_indices
    assert not (X.indices == X.shape[1] - 1).any()
    assert F.SCAN_BLOCK == 1024


@pytest.mark.parametrize("N", [F.SCAN_BLOCK - 1, F.SCAN_BLOCK, F.SCAN_BLOCK + 1, 2 * F.SCAN_BLOCK + 1, 7])
def test_subset_against_the_restatement(engine, N):
    X = edge_matrix(N)
    G = X.shape[1]
    mc, mg = masks(N, 1), masks(G, 2)
    combos = [(c, g) for c in mc for g in mg] if N == 7 else [
        ("all", "all"), ("but_one", "all"), ("alternating", "all"), ("all", "but_one"), ("all", "alternating"),
        ("none", "none"), ("none", "random"), ("random", "none"), ("random", "random"), ("last_only", "first_only")]
    for cname, gname in combos:
        kc, kg = mc[cname], mg[gname]
        staged = engine.preprocess_upload_as_stored(X)
        assert F.same_csr(engine.preprocess_fetch_counts(), X) and staged is not None
        want = F.subset(X, kc, kg)
        n, g, nnz = engine.preprocess_subset(kc, kg)
        assert (n, g, nnz) == (want.shape[0], want.shape[1], want.nnz), (cname, gname)
        assert engine._pre["N"] == n and engine._pre["G"] == g
        got = engine.preprocess_fetch_counts()
        assert F.same_csr(got, want), (cname, gname)        # the stored order and the stored zeros survive
        # the rebuilt transpose serves the column walks
        n_cells, totals = engine.preprocess_gene_detect()
        wn, wt = F.gene_detect(want)
        assert np.array_equal(n_cells, wn) and np.array_equal(totals, wt), (cname, gname)


def test_gene_detect_and_cell_sums_against_the_restatement(engine):
    N = F.SCAN_BLOCK + 1
    X = edge_matrix(N)
    engine.preprocess_upload_as_stored(X)
    for name, m in masks(N, 3).items():
        n_cells, totals = engine.preprocess_gene_detect(m)
        wn, wt = F.gene_detect(X, m)
        assert n_cells.dtype == np.int64 and np.array_equal(n_cells, wn) and np.array_equal(totals, wt), name
    # a stored zero is no detection: counting every stored entry would differ
    stored = np.bincount(X.indices, minlength=X.shape[1])
    assert (stored != F.gene_detect(X)[0]).any()
    assert engine.preprocess_gene_detect()[0][-1] == 0                  # the gene without entries
    for name, m in masks(X.shape[1], 4).items():
        got = engine.preprocess_cell_sums(m)
        assert np.array_equal(got, F.cell_sums(X, m)), name
        assert got[0] == 0.0                                            # the cell without entries
    none = engine.preprocess_cell_sums(np.zeros(X.shape[1], dtype=bool))
    assert np.array_equal(none, np.zeros(N))
    assert np.array_equal(engine.preprocess_cell_sums(None).view(np.uint64), engine.preprocess_row_sums().view(np.uint64))


def test_fetch_counts_normalised_against_the_restatement(engine):
    X = edge_matrix(200)
    engine.preprocess_upload_as_stored(X)
    for target in (1e4, 1.0, 12345.678):
        assert F.same_csr(engine.preprocess_fetch_counts(target), F.fetch_counts(X, target))
    got = engine.preprocess_fetch_counts(1e4)
    assert got[0].nnz == 0 and np.all(np.diff(got.indptr)[1:5] == [63, 64, 65, 129])


def test_subset_twice_and_select_after_subset(engine):
    X = edge_matrix(300, zeros=False, shuffle=False)
    kc1, kg1 = masks(300, 5)["random"], masks(150, 6)["random"]
    kg1[:3] = True
    once = F.subset(X, kc1, kg1)
    kc2, kg2 = masks(once.shape[0], 7)["alternating"], masks(once.shape[1], 8)["but_one"]
    twice = F.subset(once, kc2, kg2)
    engine.preprocess_upload(X)
    engine.preprocess_subset(kc1, kg1)
    engine.preprocess_subset(kc2, kg2)
    assert F.same_csr(engine.preprocess_fetch_counts(), twice)
    # select on the device-made subset == select on the same subset freshly uploaded, for raw and normalised rows
    sel = np.arange(0, twice.shape[1], 3)
    outs = []
    for fresh in (False, True):
        if fresh:
            engine.preprocess_upload(twice)
        res = []
        for target in (0.0, 1e4):
            std = engine.preprocess_select(0, sel, target, None)
            res.append((std, engine.preprocess_fetch(0)))
        outs.append(res)
    for (s1, Y1), (s2, Y2) in zip(*outs):
        assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64)) and F.same_csr(Y1, Y2)
    # the normalised copy inside select and fetch_counts scale by the same factor: x * scale, then / std
    std, Y = outs[1][1]
    T = engine.preprocess_fetch_counts(1e4)[:, sel]
    T.sort_indices()
    assert np.array_equal((T.data / std[T.indices]).view(np.uint64), Y.data.view(np.uint64))


def test_all_false_masks_are_refused_and_the_staging_survives(engine):
    X = edge_matrix(100)
    engine.preprocess_upload_as_stored(X)
    engine.preprocess_select(0, np.arange(5), 0.0, None)
    for kc, kg in ((np.zeros(100, dtype=bool), None), (None, np.zeros(150, dtype=bool)),
                   (np.zeros(100, dtype=bool), np.zeros(150, dtype=bool))):
        with pytest.raises(ValueError, match="keeps no"):
            engine.preprocess_subset(kc, kg)
    assert engine._pre["N"] == 100 and engine._pre["G"] == 150
    assert F.same_csr(engine.preprocess_fetch_counts(), X)
    assert engine.preprocess_fetch(0).shape == (100, 5)                 # a refused call leaves the slots too
    n, g, nnz = engine.preprocess_subset(np.arange(100) < 10, None)
    assert (n, g) == (10, 150) and F.same_csr(engine.preprocess_fetch_counts(), F.subset(X, np.arange(100) < 10))


def test_a_matrix_without_entries(engine):
    X = sp.csr_matrix((5, 9), dtype=np.float64)
    engine.preprocess_upload_as_stored(X)
    n_cells, totals = engine.preprocess_gene_detect()
    assert not n_cells.any() and not totals.any() and not engine.preprocess_cell_sums().any()
    assert engine.preprocess_fetch_counts(1e4).nnz == 0
    assert engine.preprocess_subset(np.arange(5) > 1, np.arange(9) < 4) == (3, 4, 0)
    assert engine.preprocess_fetch_counts().shape == (3, 4)


def test_as_stored_upload_still_checks_its_values(engine):
    X = sp.csr_matrix((np.array([1.0, -2.0]), np.array([1, 0]), np.array([0, 2])), shape=(1, 3))
    with pytest.raises(ValueError, match=">= 0"):
        engine.preprocess_upload_as_stored(X)
    X = sp.csr_matrix((np.array([1.0, np.inf]), np.array([1, 0]), np.array([0, 2])), shape=(1, 3))
    with pytest.raises(ValueError, match=">= 0"):
        engine.preprocess_upload_as_stored(X)


# ---------------------------------------------------------------- the chunk edge of the staging transpose
def test_select_across_the_chunk_edge_of_the_staging_transpose(engine):
    """4133 cells x 37 genes: the counting-sort transpose of the upload walks at most 4096 row chunks, so here a chunk
    holds two rows and the last one a single row; cell 2000 and the last cell are empty, gene 11 too.  All genes in
    reversed order, no target_sum, no ceiling, against scipy: the structure exactly, the values bit for bit -- the fill
    kernel forms the one correctly rounded float64 quotient x / div, div = the returned std (1 where it is 0)."""
    rs = np.random.RandomState(4133)
    D = rs.poisson(3.0, size=(4133, 37)) * (rs.random_sample((4133, 37)) < 0.15)
    D[2000] = 0
    D[-1] = 0
    D[:, 11] = 0
    X = sp.csr_matrix(D.astype(np.float64))
    N, G = X.shape
    assert N > 4096 and (N + 4095) // 4096 == 2 and N % 2 == 1
    lens = np.diff(X.indptr)
    assert lens[2000] == 0 and lens[-1] == 0 and lens[1999] > 0 and not (X.indices == 11).any()
    genes = np.arange(G)[::-1]
    engine.preprocess_upload(X)
    std = engine.preprocess_select(0, genes, 0.0, None)
    Y = engine.preprocess_fetch(0)
    want = sp.csr_matrix(X[:, genes])
    want.sum_duplicates()
    want.sort_indices()
    assert Y.shape == want.shape and Y.nnz == want.nnz == X.nnz
    assert np.array_equal(Y.indptr, want.indptr) and np.array_equal(Y.indices, want.indices)
    assert std.dtype == np.float64 and std[genes == 11][0] == 0.0 and np.count_nonzero(std == 0.0) == 1
    div = np.where(std == 0.0, 1.0, std)
    assert np.array_equal(Y.data.view(np.uint64), (want.data / div[want.indices]).view(np.uint64))


# ---------------------------------------------------------------- real values: the sums against math.fsum
def test_real_valued_sums_are_within_their_bounds(engine):
    """4 097 cells of at most 700 stored entries, gamma values.  A float64 sum of n non-negative terms in any order is
    within (n - 1) u of the exact sum, relatively (u = 2^-53): cell_sums <= 699 u < 1e-13, gene_detect's totals <= 4 096 u
    < 1e-12.  fetch_counts(1e4) is x * fl(t / fl(s)): the row sum's (n - 1) u, one rounding for the quotient and one for
    the product against x * t / s with the exact s -- (699 + 2) u (1 + O(u)) < 7.8e-14, so rtol 1e-13 there too."""
    N, G, target = 4097, 900, 1e4
    rs = np.random.RandomState(11)
    lens = rs.randint(0, 701, size=N)
    lens[:3] = [700, 0, 1]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rs.permutation(G)[:n]) for n in lens]).astype(np.int32)
    data = rs.gamma(0.7, 3.0, size=indptr[-1]) + 1e-3
    X = sp.csr_matrix((data, indices, indptr), shape=(N, G))
    assert 701 * U < 1e-13 and 4096 * U < 1e-12 and np.diff(X.tocsc().indptr).max() <= 4097
    engine.preprocess_upload(X)
    gmask = np.arange(G) % 3 != 0
    exact = np.array([math.fsum(X.data[a:b]) for a, b in zip(indptr[:-1], indptr[1:])])
    exact_m = np.array([math.fsum(X.data[a:b][gmask[X.indices[a:b]]]) for a, b in zip(indptr[:-1], indptr[1:])])
    for m, want in ((None, exact), (gmask, exact_m)):
        got = engine.preprocess_cell_sums(m)
        err = np.abs(got - want) / np.where(want > 0, want, 1.0)
        print("cell_sums: max relative error %.3e" % err.max())
        assert err.max() <= 1e-13 and np.array_equal(got == 0, want == 0)
    Xc = X.tocsc()
    cmask = np.arange(N) % 2 == 1
    for m in (None, cmask):
        n_cells, totals = engine.preprocess_gene_detect(m)
        want = np.array([math.fsum(Xc.data[a:b][np.ones(b - a, dtype=bool) if m is None else m[Xc.indices[a:b]]])
                         for a, b in zip(Xc.indptr[:-1], Xc.indptr[1:])])
        err = np.abs(totals - want) / np.where(want > 0, want, 1.0)
        print("gene_detect totals: max relative error %.3e" % err.max())
        assert err.max() <= 1e-12
        assert np.array_equal(n_cells, F.gene_detect(X, m)[0])
    T = engine.preprocess_fetch_counts(target)
    assert np.array_equal(T.indptr, X.indptr) and np.array_equal(T.indices, X.indices)
    rows = np.repeat(np.arange(N), lens)
    want = X.data * (target / exact[rows])
    err = np.abs(T.data - want) / want
    print("fetch_counts: max relative error %.3e" % err.max())
    assert err.max() <= 1e-13
    # two calls, the same bits
    assert np.array_equal(engine.preprocess_cell_sums(gmask).view(np.uint64), engine.preprocess_cell_sums(gmask).view(np.uint64))
    assert np.array_equal(engine.preprocess_gene_detect(cmask)[1].view(np.uint64), totals.view(np.uint64))
    assert F.same_csr(engine.preprocess_fetch_counts(target), T)
