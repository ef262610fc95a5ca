"""Plain-numpy restatement of the device tail of init='nndsvd' (cnmf_amd/csrc/nndsvd_tail_host.hip.h): a one-sided Jacobi
(Hestenes) SVD on the rows of B in a fixed round-robin pairing, then the steps of ``cnmf_amd.engine._nndsvd_finish``
(back-transformation, svd_flip, positive / negative split, threshold).  ``dtype`` = np.float64 is the arithmetic of the
device; np.longdouble gives the yardstick for its rounding error (the convention of tests/_harmony_ref.py)."""
import numpy as np

MAX_SWEEPS = 30
EPS64 = float(np.finfo(np.float64).eps)


def round_robin(c):
    """The rounds of disjoint pairs (p < q) the kernel walks: circle method on c players (+ a dummy when c is odd)."""
    n = c + (c & 1)
    rounds = []
    for r in range(n - 1):
        ps, qs = [], []
        for i in range(n // 2):
            p, q = (n - 1, r) if i == 0 else ((r + i) % (n - 1), (r - i + n - 1) % (n - 1))
            p, q = min(p, q), max(p, q)
            if q < c:
                ps.append(p); qs.append(q)
        rounds.append((np.asarray(ps, dtype=np.int64), np.asarray(qs, dtype=np.int64)))
    return rounds


def hestenes_svd(B, dtype=np.float64, max_sweeps=MAX_SWEEPS):
    """B [c, L] -> (S descending [c], VT [c, L] = right vectors as rows, J [c, c] whose ROWS are the left vectors in the
    small basis, sweeps made, converged).  A = J B is driven to orthogonal rows."""
    A = np.array(B, dtype=dtype)
    c = A.shape[0]
    J = np.eye(c, dtype=dtype)
    rounds = round_robin(c)
    sweeps, conv = 0, c < 2
    one, two = dtype(1), dtype(2)
    while not conv and sweeps < max_sweeps:
        rotated = False
        for ps, qs in rounds:
            if ps.size == 0:
                continue
            ap, aq = A[ps], A[qs]
            al, be, ga = (ap * ap).sum(axis=1), (aq * aq).sum(axis=1), (ap * aq).sum(axis=1)
            act = ~((al == 0) | (be == 0) | (np.abs(ga) <= dtype(4 * EPS64) * np.sqrt(al * be)))
            if not act.any():
                continue
            rotated = True
            p, q = ps[act], qs[act]
            zeta = (be[act] - al[act]) / (two * ga[act])
            t = np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
            cs = one / np.sqrt(one + t * t)
            sn = cs * t
            cs, sn = cs[:, None], sn[:, None]
            ap, aq = A[p], A[q]
            A[p], A[q] = cs * ap - sn * aq, sn * ap + cs * aq
            jp, jq = J[p], J[q]
            J[p], J[q] = cs * jp - sn * jq, sn * jp + cs * jq
        sweeps += 1
        conv = not rotated
    s = np.sqrt((A * A).sum(axis=1))
    order = np.argsort(-s, kind="stable")
    S = s[order]
    with np.errstate(divide="ignore", invalid="ignore"):
        VT = A[order] / S[:, None]
    return S, VT, J[order], sweeps, conv


def tail_ref(k, Q, B, transpose, eps=1e-6, dtype=np.float64):
    """(W [N, k], H [k, G], info) from Q [M_rows, c] and B = Q^T M [c, M_cols].  info: the un-thresholded factors, the
    singular values, and the margins of the three discrete decisions (split choice, flip arg-max, order of S)."""
    Q = np.asarray(Q, dtype=dtype)
    S, VT, J, sweeps, conv = hestenes_svd(B, dtype)
    UT = J[:k] @ Q.T
    VT = VT[:k]
    lead = VT if transpose else UT
    mag = np.abs(lead)
    idx = np.argmax(mag, axis=1)
    signs = np.sign(lead[np.arange(k), idx])
    top2 = np.sort(mag, axis=1)[:, -2:] if mag.shape[1] > 1 else np.concatenate([np.zeros_like(mag), mag], axis=1)
    flip_margin = float(((top2[:, 1] - top2[:, 0]) / top2[:, 1]).min())
    UT = UT * signs[:, None]
    VT = VT * signs[:, None]
    WT, HR = (VT, UT) if transpose else (UT, VT)
    W = np.zeros_like(WT)
    H = np.zeros_like(HR)
    W[0] = np.sqrt(S[0]) * np.abs(WT[0])
    H[0] = np.sqrt(S[0]) * np.abs(HR[0])
    split_margin = np.inf
    for j in range(1, k):
        x, y = WT[j], HR[j]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = np.sqrt(x_p @ x_p), np.sqrt(y_p @ y_p)
        x_n_nrm, y_n_nrm = np.sqrt(x_n @ x_n), np.sqrt(y_n @ y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        split_margin = min(split_margin, float(abs(m_p - m_n) / max(m_p, m_n)))
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[j] = lbd * u
        H[j] = lbd * v
    W_raw, H_raw = np.ascontiguousarray(W.T), H.copy()
    W[W < eps] = 0
    H[H < eps] = 0
    gaps = (S[:k] - S[1:k + 1]) / S[0] if S.size > k else (S[:k - 1] - S[1:k]) / S[0]
    info = dict(W_raw=W_raw, H_raw=H_raw, S=S, sweeps=sweeps, converged=conv, flip_margin=flip_margin,
                split_margin=split_margin, s_gap=float(gaps.min()) if gaps.size else np.inf)
    return np.ascontiguousarray(W.T), H, info
