"""Average-linkage (UPGMA) agglomeration and the clustergram's leaf order, restated in float64 numpy from the definition.

This is the yardstick of the device clustergram (``Engine.clustergram``, csrc/linkage_host.hip.h): the kernels are held to it
bit for bit.  It is not scipy's algorithm (a nearest-neighbour chain followed by a sort); where merge heights are distinct
both give the same rows, where they tie the rule below decides and scipy may differ.

``upgma(D)`` for the m x m distance block of one cluster (m >= 1):

* entries < 0 are set to 0 first (cnmf.py:1002);
* every member starts as its own group in slot i, with id i and size 1;
* m - 1 times: among live slots the pair a < b with the smallest distance merges -- ties to the smallest a, then the smallest
  b; the row ``(min(id_a, id_b), max(id_a, id_b), height, size_a + size_b)`` is emitted; for every other live slot t
  ``d(a,t) = (size_a * d(a,t) + size_b * d(b,t)) / (size_a + size_b)`` with exactly these roundings (two products, one sum,
  one quotient; numpy never fuses them); the merged group keeps slot a and takes id m + step, slot b is retired.

``leaves(Z, m)``: the leaves of the dendrogram from the root down, column 0 before column 1.
``spectra_order(labels_kept, D)``: over the clusters in ascending label, ``np.where(labels == c)[0][leaves]`` -- indices into
the kept rows, as cnmf.py:995-1009 builds them.
"""
import numpy as np


def upgma(D):
    D = np.array(D, dtype=np.float64)
    m = D.shape[0]
    if D.shape != (m, m) or m < 1:
        raise ValueError("a square distance block with at least one member is required")
    Z = np.zeros((m - 1, 4), dtype=np.float64)
    if m == 1:
        return Z
    D[D < 0] = 0.0
    # only pairs a < b of live slots are finite: a row-major argmin is then the rule's tie order
    W = np.where(np.triu(np.ones((m, m), dtype=bool), 1), D, np.inf)
    size = np.ones(m, dtype=np.float64)
    ident = np.arange(m)
    live = np.ones(m, dtype=bool)
    for step in range(m - 1):
        a, b = divmod(int(np.argmin(W)), m)
        Z[step] = (min(ident[a], ident[b]), max(ident[a], ident[b]), W[a, b], size[a] + size[b])
        live[b] = False
        t = np.flatnonzero(live)
        t = t[t != a]
        new = (size[a] * D[a, t] + size[b] * D[b, t]) / (size[a] + size[b])
        D[a, t] = new
        D[t, a] = new
        lo, hi = t[t < a], t[t > a]
        W[lo, a] = D[lo, a]
        W[a, hi] = D[a, hi]
        W[b, :] = np.inf
        W[:, b] = np.inf
        size[a] += size[b]
        ident[a] = m + step
    return Z


def leaves(Z, m):
    if m == 1:
        return np.zeros(1, dtype=np.int64)
    out, stack = [], [2 * m - 2]
    while stack:
        node = stack.pop()
        if node < m:
            out.append(node)
        else:
            stack.append(int(Z[node - m, 1]))       # popped after the left child's whole subtree
            stack.append(int(Z[node - m, 0]))
    return np.asarray(out, dtype=np.int64)


def cluster_linkages(labels_kept, D):
    """[(members, Z)] over the clusters in ascending label; D is the distance matrix of the kept rows."""
    labels_kept = np.asarray(labels_kept)
    out = []
    for c in sorted(set(labels_kept.tolist())):
        members = np.where(labels_kept == c)[0]
        out.append((members, upgma(D[np.ix_(members, members)])))
    return out


def spectra_order(labels_kept, D):
    order = [members[leaves(Z, len(members))] for members, Z in cluster_linkages(labels_kept, D)]
    return np.concatenate(order).astype(np.int64)
