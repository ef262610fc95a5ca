"""tests/_upgma_ref.py -- the float64 restatement the device clustergram is held to -- against scipy's average linkage.

With distinct merge heights the restatement and ``scipy.cluster.hierarchy.linkage(squareform(D), 'average')`` describe the
same dendrogram row for row: ids, sizes and the leaf order are compared exactly, heights within 4 m eps relative (each
level of the dendrogram adds at most three roundings of positive terms -- two products and a sum; the quotient is a fourth
-- over at most m levels, on either side).  The comparison means something only while the heights ARE distinct, so every
input's smallest relative gap between consecutive heights is asserted to be above 1e-9.
"""
import numpy as np
import pytest

import _upgma_ref as ref

hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
distance = pytest.importorskip("scipy.spatial.distance")

EPS = np.finfo(np.float64).eps
SIZES = [2, 3, 5, 64, 65, 257, 600]


def unit_rows(m, g=40, seed=0):
    x = np.abs(np.random.RandomState(seed).standard_normal((m, g)))
    return x / np.sqrt((x ** 2).sum(axis=1))[:, None]


def distances(x):
    d = np.sqrt(np.maximum(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2), 0.0))
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


@pytest.mark.parametrize("m", SIZES)
def test_restatement_equals_scipy_average_linkage(m):
    D = distances(unit_rows(m, seed=m))
    Z = ref.upgma(D)
    Zs = hierarchy.linkage(distance.squareform(D, checks=False), "average")
    assert Z.shape == Zs.shape == (m - 1, 4)
    h = Z[:, 2]
    assert (np.diff(h) >= 0).all()                                   # average linkage is reducible
    if m > 2:
        gap = (np.diff(h) / h[1:]).min()
        print("m=%d smallest relative height gap %.3g" % (m, gap))
        assert gap > 1e-9
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    rel = np.abs(h - Zs[:, 2]) / Zs[:, 2]
    print("m=%d largest relative height difference %.3g (bound %.3g)" % (m, rel.max(), 4 * m * EPS))
    assert rel.max() <= 4 * m * EPS
    assert np.array_equal(ref.leaves(Z, m), hierarchy.leaves_list(Zs))


def test_single_member_and_pair():
    assert ref.upgma(np.zeros((1, 1))).shape == (0, 4)
    assert ref.leaves(ref.upgma(np.zeros((1, 1))), 1).tolist() == [0]
    Z = ref.upgma(np.array([[0.0, 0.25], [0.25, 0.0]]))
    assert Z.tolist() == [[0.0, 1.0, 0.25, 2.0]]
    assert ref.leaves(Z, 2).tolist() == [0, 1]


def test_negative_entries_are_clamped():
    D = distances(unit_rows(6, seed=3))
    Dn = D.copy()
    i, j = np.unravel_index(np.argmin(D + 10 * np.eye(6)), D.shape)
    Dn[i, j] = Dn[j, i] = -1e-9                                       # (cnmf.py:1002: "rarely get floating point issues")
    Dz = D.copy()
    Dz[i, j] = Dz[j, i] = 0.0
    Z = ref.upgma(Dn)
    assert np.array_equal(Z, ref.upgma(Dz)) and Z[0, 2] == 0.0 and (Z[:, 2] >= 0).all()
    assert Dn[i, j] < 0                                               # the caller's matrix is left alone


def test_ties_go_to_the_smallest_slots():
    # four points, all six distances equal: (0,1) merge first, then slot 0 (id 4) with slot 2, then with slot 3
    D = np.ones((4, 4)) - np.eye(4)
    Z = ref.upgma(D)
    assert Z.tolist() == [[0, 1, 1, 2], [2, 4, 1, 3], [3, 5, 1, 4]]
    assert ref.leaves(Z, 4).tolist() == [3, 2, 0, 1]


def test_spectra_order_on_interleaved_labels():
    labels = np.array([2, 0, 1, 0, 2, 2, 0, 3, 0, 2, 0, 2, 1])       # cluster 3: one member, cluster 1: a pair
    D = distances(unit_rows(len(labels), seed=9))
    order = ref.spectra_order(labels, D)
    assert sorted(order.tolist()) == list(range(len(labels)))
    pos = 0
    for c in range(4):
        members = np.where(labels == c)[0]
        block = D[np.ix_(members, members)]
        if len(members) > 1:
            want = members[hierarchy.leaves_list(hierarchy.linkage(distance.squareform(block, checks=False), "average"))]
        else:
            want = members
        assert np.array_equal(order[pos:pos + len(members)], want)
        pos += len(members)
    # the labels' values do not matter, their order does
    assert np.array_equal(ref.spectra_order(labels * 7 + 1, D), order)
