"""The fixed summation order of the staging statistics (csrc/kernels_segments.hip.h), pinned bit for bit against its numpy
restatement (tests/_wave_ref.py): a wavefront per row or column, the lanes 64 entries apart, the xor butterfly 32 ... 1.

The other staging tests mostly feed integer counts, whose float64 sums are exact in any order; here the values are real
(gamma(0.7, 3.0) * 1.37) and a column holds up to 1000 of them, so another order gives other bits
(test_the_inputs_hold_what_they_claim).  Column lengths sit around the walk's edges: nothing, one entry, one step of 64
less one / exactly / plus one, two steps likewise, and many steps.  4 columns fill one workgroup of four wavefronts, 5
and 11 leave the last one ragged.  The column moments (their `q += d * d` is a fused multiply-add) are not restated here."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests._wave_ref import sequential_sum, wave_sum

N = 1000
LENGTHS = {11: (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1000), 5: (65, 0, 127, 1000, 129), 4: (1000, 127, 64, 1)}
SEED = 20


@pytest.fixture(autouse=True)
def release(request):
    yield
    if "engine" in request.fixturenames:
        request.getfixturevalue("engine").preprocess_release()


@functools.lru_cache(maxsize=None)
def matrix(G):
    """N cells x G genes, canonical CSR: column g stores LENGTHS[G][g] real values in random cells"""
    rs = np.random.RandomState(SEED + G)
    M = np.zeros((N, G), dtype=bool)
    for g, n in enumerate(LENGTHS[G]):
        M[rs.permutation(N)[:n], g] = True
    X = sp.csr_matrix(M.astype(np.float64))
    X.data = rs.gamma(0.7, 3.0, size=X.nnz) * 1.37
    X.data.setflags(write=False)
    return X


def column_entries(X):
    """per gene: (cells, values) of its stored entries by ascending cell, as the transposed staging lists them"""
    C = sp.csc_matrix(X)
    assert C.has_sorted_indices
    return [(C.indices[C.indptr[g]:C.indptr[g + 1]], C.data[C.indptr[g]:C.indptr[g + 1]]) for g in range(X.shape[1])]


def columns(X, cells=None):
    """per gene: the stored values by ascending cell (cells: of those cells only)"""
    return [v if cells is None else v[cells[r]] for r, v in column_entries(X)]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def test_the_inputs_hold_what_they_claim():
    for G, lengths in LENGTHS.items():
        X = matrix(G)
        assert X.shape == (N, G) and X.has_canonical_format and (X.data > 0).all()
        assert tuple(np.diff(sp.csc_matrix(X).indptr)) == lengths
    assert 4 % 4 == 0 and 5 % 4 == 1 and 11 % 4 == 3 and 11 > 2 * 4
    # the orders can be told apart: a column whose wave-order sum has other bits than numpy's pairwise sum, and one
    # whose wave-order sum has other bits than the sum from the left (columns of 127 and 1000 entries do both)
    cols = columns(matrix(11))
    wave = [wave_sum(v) for v in cols]
    not_numpy = [len(v) for v, w in zip(cols, wave) if w != np.sum(v)]
    not_left = [len(v) for v, w in zip(cols, wave) if w != sequential_sum(v)]
    print("wave order differs from np.sum at lengths %s, from the sequential sum at %s" % (not_numpy, not_left))
    assert 127 in not_numpy and 1000 in not_numpy and 127 in not_left and 1000 in not_left
    # ... and so can the clipped squares and a row's butterfly
    c2 = [wave_sum(np.minimum(v, 2.3) ** 2) for v in cols]
    assert any(w != sequential_sum(np.minimum(v, 2.3) ** 2) for v, w in zip(cols, c2))
    X = matrix(11)
    rows = [X.data[X.indptr[i]:X.indptr[i + 1]] for i in range(N)]
    assert max(len(r) for r in rows) >= 4 and any(wave_sum(r) != sequential_sum(r) for r in rows)
    assert matrix(11)[500].nnz > 0                           # (the single cell of test_clipped_sums_batched's batch 1)


@pytest.mark.gpu
@pytest.mark.parametrize("G", sorted(LENGTHS))
def test_gene_detect_totals(engine, G):
    X = matrix(G)
    engine.preprocess_upload_as_stored(X)
    cells = np.arange(N) % 3 != 1
    for mask in (None, cells):
        n_cells, totals = engine.preprocess_gene_detect(mask)
        keep = [np.ones(len(r), dtype=bool) if mask is None else mask[r] for r, _ in column_entries(X)]
        assert same_bits(totals, [wave_sum(v, k) for v, k in zip(columns(X), keep)])    # (a skipped entry keeps its lane)
        assert list(n_cells) == [int(k.sum()) for k in keep]


@pytest.mark.gpu
@pytest.mark.parametrize("G", sorted(LENGTHS))
def test_cell_sums_and_row_sums(engine, G):
    X = matrix(G)
    engine.preprocess_upload_as_stored(X)
    rows = [(X.indices[X.indptr[i]:X.indptr[i + 1]], X.data[X.indptr[i]:X.indptr[i + 1]]) for i in range(N)]
    plain = engine.preprocess_cell_sums()
    assert same_bits(plain, [wave_sum(v) for _, v in rows])
    assert same_bits(engine.preprocess_row_sums(), plain)
    genes = np.arange(G) % 3 != 1
    assert same_bits(engine.preprocess_cell_sums(genes), [wave_sum(v, genes[c]) for c, v in rows])


@pytest.mark.gpu
@pytest.mark.parametrize("G", sorted(LENGTHS))
def test_clipped_sums(engine, G):
    X = matrix(G)
    engine.preprocess_upload_as_stored(X)
    clip = 2.3 + 0.71 * np.arange(G)
    c1, c2 = engine.preprocess_clipped_sums(clip)
    m = [np.minimum(v, c) for v, c in zip(columns(X), clip)]
    assert any((v > c).any() for v, c in zip(columns(X), clip)) and any((v < c).any() for v, c in zip(columns(X), clip))
    assert same_bits(c1, [wave_sum(x) for x in m])
    assert same_bits(c2, [wave_sum(x * x) for x in m])      # (the square rounded, then added: fp contract(off))


@pytest.mark.gpu
def test_clipped_sums_batched(engine):
    """every (batch, gene) pair against the restatement over that batch's entries alone, and against the one-batch entry
    point on the staging restricted to the batch"""
    G, B = 11, 3
    X = matrix(G)
    codes = (np.arange(N) % 2 * 2).astype(np.int32)
    codes[500] = 1                                          # batch 1 is a single cell
    assert list(np.bincount(codes)) == [499, 1, 500]
    assert X[500].nnz > 0
    clip = 2.3 + 0.71 * np.arange(G)[None, :] + 0.13 * np.arange(B)[:, None]
    engine.preprocess_upload_as_stored(X)
    c1, c2 = engine.preprocess_clipped_sums_batched(codes, B, clip)
    for b in range(B):
        cells = codes == b
        m = [np.minimum(v, c) for v, c in zip(columns(X, cells), clip[b])]
        assert same_bits(c1[b], [wave_sum(x) for x in m]), b
        assert same_bits(c2[b], [wave_sum(x * x) for x in m]), b
        engine.preprocess_upload_as_stored(X)
        assert engine.preprocess_subset(cells, None)[:2] == (int(cells.sum()), G)
        o1, o2 = engine.preprocess_clipped_sums(clip[b])
        assert same_bits(o1, c1[b]) and same_bits(o2, c2[b]), b
