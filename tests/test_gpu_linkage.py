"""``Engine.clustergram`` (csrc/linkage_host.hip.h) against the float64 restatement tests/_upgma_ref.py, bit for bit.

Inputs: L2-normalised |N(0,1)| rows over 40 genes, labels assigned by hand (no k-means), the clusters' rows interleaved and
about a tenth of the rows filtered (-1) among them.

Where the distances come from.  ``cnmf_clustergram`` L2-normalises the kept rows itself (its callers hand it the merged
spectra as they are, cnmf.py:882) and then runs the consensus core's distance kernel.  Dividing an already normalised row
by its computed norm (1 to within a few eps, not always 1.0) moves some entries by an ulp, so
``engine.pairwise_distances`` -- which takes rows AS GIVEN -- is not the same matrix to the bit.  The bit-for-bit yardstick
is therefore the restatement run on the matrix of the device's own normalise-then-distance route over the same kept rows
(``engine.consensus(kept_rows, ..., skip_density=True, return_dist=True)``: the very two kernels).  Against
``engine.pairwise_distances`` of the kept rows the dendrogram's structure (ids, sizes, leaf order) is compared as well:
the inputs' smallest relative height gap is ~1e-7, nine orders above that perturbation.
"""
import numpy as np
import pytest

import _upgma_ref as ref

pytestmark = pytest.mark.gpu

G = 40
SIZES = [1, 2, 3, 64, 65, 256, 257, 1100]      # no merge, one merge, the wave (64) and workgroup (512) edges, strided loops


def unit_rows(n, g=G, seed=0):
    x = np.abs(np.random.RandomState(seed).standard_normal((n, g)))
    return x / np.sqrt((x ** 2).sum(axis=1))[:, None]


def device_distances(engine, kept_rows):
    """Distances of the L2-normalised rows by the consensus core's own kernels (l2_rows_kernel + dist_sym_kernel)."""
    return engine.consensus(kept_rows, 2, skip_density=True, return_dist=True, n_init=1)["topics_dist"]


def check_against_restatement(out, labels, D):
    kept = labels[labels >= 0]
    links = ref.cluster_linkages(kept, D)
    assert len(out["linkage"]) == len(links)
    pos = 0
    for c, (members, Z) in enumerate(links):
        Zd = out["linkage"][c]
        assert Zd.shape == Z.shape, c
        assert Zd.tobytes() == Z.tobytes(), (c, len(members))
        assert (np.diff(Zd[:, 2]) >= 0).all(), c
        got = out["spectra_order"][pos:pos + len(members)]
        assert sorted(got.tolist()) == members.tolist(), c              # a permutation of the cluster's members
        assert np.array_equal(got, members[ref.leaves(Z, len(members))]), c
        assert out["segments"][c] == pos
        pos += len(members)
    assert out["segments"][-1] == pos == len(kept)
    order = out["spectra_order"]
    assert out["topics_dist_ordered"].tobytes() == np.ascontiguousarray(D[order][:, order]).tobytes()
    return links


@pytest.fixture(scope="module")
def mixed(engine):
    """All cluster sizes in one call: rows, labels (with -1), the device's distances of the kept rows, the result."""
    rs = np.random.RandomState(11)
    labels = np.concatenate([np.full(m, c) for c, m in enumerate(SIZES)] + [np.full(sum(SIZES) // 9, -1)])
    labels = labels[rs.permutation(len(labels))].astype(np.int32)
    rows = unit_rows(len(labels), seed=12)
    D = device_distances(engine, rows[labels >= 0])
    out = engine.clustergram(rows, labels, len(SIZES), return_image=True, return_linkage=True)
    return rows, labels, D, out


def test_every_cluster_size_in_one_call(mixed):
    rows, labels, D, out = mixed
    assert (labels == -1).sum() >= len(labels) // 11
    links = check_against_restatement(out, labels, D)
    assert [len(mb) for mb, _ in links] == SIZES
    for _, Z in links:                                                     # tie-free, as the scipy comparison below needs
        if len(Z) > 1:
            assert (np.diff(Z[:, 2]) / Z[1:, 2]).min() > 1e-9


def test_order_equals_scipy_on_tie_free_input(mixed):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    rows, labels, D, out = mixed
    kept = labels[labels >= 0]
    want = []
    for c in range(len(SIZES)):
        members = np.where(kept == c)[0]
        if len(members) > 1:
            block = D[np.ix_(members, members)]
            members = members[hierarchy.leaves_list(hierarchy.linkage(squareform(block, checks=False), "average"))]
        want += members.tolist()
    assert out["spectra_order"].tolist() == want


def test_structure_equals_restatement_on_pairwise_distances(engine, mixed):
    rows, labels, D, out = mixed
    Dp, _ = engine.pairwise_distances(rows[labels >= 0])
    print("entries of the two distance matrices that differ: %d of %d, largest difference %.3g"
          % ((Dp != D).sum(), D.size, np.abs(Dp - D).max()))
    kept = labels[labels >= 0]
    for c, (members, Z) in enumerate(ref.cluster_linkages(kept, Dp)):
        assert np.array_equal(out["linkage"][c][:, [0, 1, 3]], Z[:, [0, 1, 3]]), c
    assert np.array_equal(out["spectra_order"], ref.spectra_order(kept, Dp))


def test_exact_ties_and_zero_distances(engine):
    base = unit_rows(8, seed=21)
    tied = np.tile(base, (5, 1))                                           # 40 rows: 8 distinct ones, five copies each
    other = unit_rows(7, seed=22)
    rows = np.concatenate([other[:3], tied[:20], other[3:], tied[20:]])
    labels = np.concatenate([np.zeros(3), np.ones(20), np.zeros(4), np.ones(20)]).astype(np.int32)
    D = device_distances(engine, rows)
    block = D[np.ix_(labels == 1, labels == 1)]
    # copies of one row are at distance zero up to the rounding of |x|^2 + |y|^2 - 2 x.y (0 or ~1e-8, the same value for
    # every pair of copies); the 25 distances between two groups take at most two values (the kernel adds the two squared
    # norms in the element's own row, column order)
    upper = block[np.triu_indices(40, 1)]
    assert (upper <= 1e-7).sum() == 8 * 10
    assert len(np.unique(upper)) <= 8 + 2 * 28
    out = engine.clustergram(rows, labels, 2, return_linkage=True)
    check_against_restatement(out, labels, D)
    assert (out["linkage"][1][:32, 2] <= 1e-7).all() and (out["linkage"][1][32:, 2] > 1e-3).all()


def test_one_cluster_all_rows_kept(engine):
    rows = unit_rows(131, seed=31)
    labels = np.zeros(131, dtype=np.int32)
    out = engine.clustergram(rows, labels, 1, return_linkage=True)
    check_against_restatement(out, labels, device_distances(engine, rows))
    assert out["segments"].tolist() == [0, 131]
    # without the image and the linkage the order is the same
    lean = engine.clustergram(rows, labels, 1, return_image=False)
    assert lean["topics_dist_ordered"] is None and lean["linkage"] is None
    assert np.array_equal(lean["spectra_order"], out["spectra_order"])


def test_store_rows_give_the_uploaded_result(engine):
    rs = np.random.RandomState(41)
    rows = unit_rows(300, seed=42).astype(np.float32)
    labels = rs.randint(-1, 5, size=300).astype(np.int32)
    engine.spectra_reset()
    try:
        engine.spectra_append(unit_rows(17, seed=43).astype(np.float32))           # the rows do not start at 0
        first = engine.spectra_append(rows)
        up = engine.clustergram(rows.astype(np.float64), labels, 5, return_linkage=True)
        st = engine.clustergram(None, labels, 5, store_rows=first + np.arange(300), return_linkage=True)
    finally:
        engine.spectra_reset()
    assert np.array_equal(up["spectra_order"], st["spectra_order"])
    assert up["topics_dist_ordered"].tobytes() == st["topics_dist_ordered"].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(up["linkage"], st["linkage"]))


def test_errors(engine):
    big = unit_rows(4097, g=8, seed=51)
    with pytest.raises(NotImplementedError, match="4097"):
        engine.clustergram(big, np.zeros(4097, dtype=np.int32), 1)
    rows = unit_rows(12, seed=52)
    with pytest.raises(ValueError, match="empty"):
        engine.clustergram(rows, np.array([0, 0, 2, 2, -1, 0, 2, 0, 0, 2, 2, 0], dtype=np.int32), 3)
    with pytest.raises(ValueError, match="outside"):
        engine.clustergram(rows, np.array([0, 0, 1, 1, -1, 0, 3, 0, 0, 1, 2, 0], dtype=np.int32), 3)
    with pytest.raises(ValueError, match="outside"):
        engine.clustergram(rows, np.array([0, 0, 1, 1, -2, 0, 2, 0, 0, 1, 2, 0], dtype=np.int32), 3)
    # the context is as usable as before
    out = engine.clustergram(rows, np.array([0, 0, 1, 1, -1, 0, 2, 0, 0, 1, 2, 0], dtype=np.int32), 3)
    assert sorted(out["spectra_order"].tolist()) == list(range(11))


def test_two_calls_give_identical_bytes(engine, mixed):
    rows, labels, D, out = mixed
    again = engine.clustergram(rows, labels, len(SIZES), return_image=True, return_linkage=True)
    assert again["spectra_order"].tobytes() == out["spectra_order"].tobytes()
    assert again["topics_dist_ordered"].tobytes() == out["topics_dist_ordered"].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again["linkage"], out["linkage"]))
