"""Reference side of tests/test_gpu_cd_steps.py: single coordinate-descent iterations of oracle/nmf_cd.py from explicit
float32 start factors, once in float64 (the reference) and once in float32 (the restatement whose own distance from the
reference is the yardstick), the distances between two such runs, and float64 mutants of the oracle's loop.

Nothing here touches the device.  Every reference is computed once per process (functools.lru_cache) and returned
read-only.
"""
import functools

import numpy as np

from cnmf_amd import synth
from oracle import nmf_cd

FACTOR = 16                 # the bar: device distance <= FACTOR x the float32 restatement's own distance
TS = (1, 2, 3)

REGS = {
    "none": dict(alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0),
    "mixed": dict(alpha_W=0.002, alpha_H=0.001, l1_ratio=0.3),
    "l1": dict(alpha_W=0.002, alpha_H=0.001, l1_ratio=1.0),
    "l2": dict(alpha_W=0.002, alpha_H=0.001, l1_ratio=0.0),
}

RANKS_R = tuple(list(range(1, 17)) * 2 + [17, 20, 21, 24, 25, 28, 29, 32, 33, 47, 48, 49, 63, 64])
RANKS_S = (5, 128, 9, 70, 33, 96, 64, 65)
EDGES = (256, 512, 768)


def tier(k):
    """Register tier of a rank: rounded up to a multiple of 4 up to 32, then 48, 64, 128."""
    if k <= 32:
        return (k + 3) // 4 * 4
    return 48 if k <= 48 else 64 if k <= 64 else 128


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def matrix(name):
    """A: 517 x 500 count-structured (C1 truncated); B: A made general (a row scale and a small dense offset)."""
    A = synth.make_config("C1", dtype=np.float64, n_cells=517)
    if name == "A":
        return _frozen(A)
    assert name == "B"
    rs = np.random.RandomState(12)
    return _frozen(A * np.exp(0.5 * rs.standard_normal((A.shape[0], 1))) + 0.01 * np.abs(rs.standard_normal(A.shape)))


@functools.lru_cache(maxsize=None)
def batch(name):
    """(ranks, seeds) of batch R (46 restarts, 772 packed columns) or S (sweep_big_kernel beside the small tiers)."""
    ks = {"R": RANKS_R, "S": RANKS_S}[name]
    rs = np.random.RandomState(41 if name == "R" else 43)
    return ks, tuple(int(s) for s in rs.randint(1, 2**31 - 1, size=len(ks)))


@functools.lru_cache(maxsize=None)
def inits(mname, bname):
    """Float32 start factors [(W0, H0)] of every restart: drawn once, the same bits go to all three runs."""
    X32 = matrix(mname).astype(np.float32)
    ks, seeds = batch(bname)
    return tuple(tuple(_frozen(a) for a in nmf_cd.random_init(X32, k, seed)) for k, seed in zip(ks, seeds))


# ---------------------------------------------------------------- distances
def d_cols(W, W64):
    """max over components c of max_i |W[i,c] - W64[i,c]| / max_i |W64[i,c]| (no matching, no normalisation)."""
    W64 = np.asarray(W64, dtype=np.float64)
    return float((np.abs(np.asarray(W, dtype=np.float64) - W64).max(axis=0) / np.abs(W64).max(axis=0)).max())


def d_rows(H, H64):
    return d_cols(np.asarray(H).T, np.asarray(H64).T)


def run_pair(X64, W0, H0, reg, ts=TS):
    """One restart from the float32 factors (W0, H0): the float64 oracle and its float32 restatement (the same oracle on
    ``X.astype(float32)``), both with tol = 0 for max(ts) iterations.  Returns a dict with, per t of ``ts``: the float64
    factors ``W`` / ``H``, the float64 violation ratio ``ratio`` = trace[t-1] / trace[0], and the restatement's own
    distances ``yW``, ``yH``, ``yv``."""
    tmax = max(ts)
    snap64, tr64 = {t: None for t in ts}, []
    n = nmf_cd.nmf(X64, W0.shape[1], W0=W0.astype(np.float64), H0=H0.astype(np.float64), tol=0.0, max_iter=tmax,
                   trace=tr64, snapshots=snap64, **reg)[2]
    snap32, tr32 = {t: None for t in ts}, []
    X32 = X64.astype(np.float32)
    W32, H32, n32 = nmf_cd.nmf(X32, W0.shape[1], W0=W0, H0=H0, tol=0.0, max_iter=tmax, trace=tr32, snapshots=snap32, **reg)
    assert n == n32 == tmax and W32.dtype == H32.dtype == np.float32
    out = {"k": W0.shape[1], "W": {}, "H": {}, "ratio": {}, "yW": {}, "yH": {}, "yv": {}}
    for t in ts:
        W, H = snap64[t]
        out["W"][t], out["H"][t] = _frozen(W), _frozen(H)
        out["ratio"][t] = tr64[t - 1] / tr64[0]
        out["yW"][t], out["yH"][t] = d_cols(snap32[t][0], W), d_rows(snap32[t][1], H)
        out["yv"][t] = abs(tr32[t - 1] / tr32[0] - out["ratio"][t])
    return out


class Reference:
    """The reference runs of some restarts and the pooled yardsticks over them."""

    def __init__(self, runs):
        self.runs = runs                # {restart index: run_pair dict}

    def Y(self, what, t, tr=None):
        """Yardstick ``what`` in ("yW", "yH", "yv") at iteration t: the maximum over the restarts of tier ``tr``
        (``None``: over all of them)."""
        return max(r[what][t] for r in self.runs.values() if tr is None or tier(r["k"]) == tr)

    def tiers(self):
        return sorted({tier(r["k"]) for r in self.runs.values()})


@functools.lru_cache(maxsize=None)
def reference(mname, bname, regname, ts=TS):
    X64 = matrix(mname)
    return Reference({i: run_pair(X64, W0, H0, REGS[regname], ts) for i, (W0, H0) in enumerate(inits(mname, bname))})


# ---------------------------------------------------------------- where the scheduler puts a restart
def first_fill(ks, kc):
    """{restart: first packed column} of the restarts the scheduler installs before the first iteration of a ``kc``-column
    batch without iteration hints (BatchSched, batch_sched.h): whatever order the ranks are listed in, the queue is
    round-robin over the distinct ranks, largest rank first inside a round, restarts of one rank in listed order; columns
    are handed out first-fit from 0, and a rank that does not fit bars the ranks >= it for the rest of the fill."""
    by_k = {}
    for r, k in enumerate(ks):
        by_k.setdefault(k, []).append(r)
    order = [by_k[k][j] for j in range(max(map(len, by_k.values()))) for k in sorted(by_k, reverse=True) if j < len(by_k[k])]
    off, pos, failed_k = {}, 0, 1 << 30
    for r in order:
        if ks[r] >= failed_k:
            continue
        if pos + ks[r] > kc:
            failed_k = ks[r]
            continue
        off[r] = pos
        pos += ks[r]
    return off


def edge_slots(ks, kc):
    """(straddlers, touchers) of the first fill: the restarts whose columns lie on both sides of a component-group edge
    (256, 512, 768), and those that begin or end exactly on an edge no slot straddles."""
    off = first_fill(ks, kc)
    straddlers = sorted(r for r, o in off.items() if any(o < e < o + ks[r] for e in EDGES))
    bare = [e for e in EDGES if not any(off[r] < e < off[r] + ks[r] for r in straddlers)]
    touchers = sorted(r for r, o in off.items() if any(e in (o, o + ks[r]) for e in bare) and o + ks[r] <= kc)
    return straddlers, touchers


# ---------------------------------------------------------------- stream-K job (12 500 cells: built on demand, not cached)
def streamk_ranks():
    """The rank list of test_stream_k_cut_tiles_match_oracle (ranks 5..13, 110 restarts, 1021 columns: one fill of a
    1024-column batch), its seeds, and the slots to compare: in the scheduler's placement two slots straddle a group
    edge (512 and 768: they carry both cut flags) and 256 is hit exactly, where the slot that ends on it and the slot
    that begins on it are taken instead."""
    rs = np.random.RandomState(7)
    ks, total = [], 0
    while True:
        k = int(rs.randint(5, 14))
        if total + k > 1024:
            break
        ks.append(k)
        total += k
    seeds = [int(s) for s in rs.randint(1, 2**31 - 1, size=len(ks))]
    straddlers, touchers = edge_slots(ks, 1024)
    return ks, seeds, straddlers, touchers


# ---------------------------------------------------------------- refit
@functools.lru_cache(maxsize=None)
def refit_spectra():
    """Three float32 spectra matrices (ranks 5, 16, 33) from bounded oracle runs on A, rows normalised to sum 1."""
    A = matrix("A")
    out = []
    for k, seed in ((5, 11), (16, 12), (33, 13)):
        H = nmf_cd.nmf(A, k, seed=seed, max_iter=20)[1]
        out.append(_frozen((H / H.sum(axis=1, keepdims=True)).astype(np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refit_reference(regname, ts=(1, 3)):
    """Per spectra matrix: {"k", "W": {t: W64}, "yW": {t: restatement distance}} of ``nmf_cd.nnls`` with tol = 0."""
    A = matrix("A")
    A32 = A.astype(np.float32)
    reg = {k: v for k, v in REGS[regname].items() if k != "alpha_H"}
    runs = {}
    for i, H32 in enumerate(refit_spectra()):
        s64, s32 = {t: None for t in ts}, {t: None for t in ts}
        n64 = nmf_cd.nnls(A, H32.astype(np.float64), tol=0.0, max_iter=max(ts), snapshots=s64, **reg)[1]
        W32, n32 = nmf_cd.nnls(A32, H32, tol=0.0, max_iter=max(ts), snapshots=s32, **reg)
        assert n64 == n32 == max(ts) and W32.dtype == np.float32
        runs[i] = {"k": H32.shape[0], "W": {t: _frozen(s64[t][0]) for t in ts},
                   "yW": {t: d_cols(s32[t][0], s64[t][0]) for t in ts}}
    return Reference(runs)


# ---------------------------------------------------------------- float64 mutants of the oracle's loop
def round_mantissa(a, bits):
    """Round to ``bits`` significant binary digits (11 = what one f16 plane holds), without f16's range."""
    m, e = np.frexp(a)
    return np.ldexp(np.round(m * 2.0**bits) / 2.0**bits, e)


def _sweep(W, HHt, XHt, drop_rows=0, stale_last=False):
    """nmf_cd.cd_sweep with two switches: the violation sum without the last ``drop_rows`` rows; the last component's
    gradient from the factor as it stood before the sweep."""
    k = W.shape[1]
    before = W.copy() if stale_last else None
    violation = 0.0
    for t in range(k):
        src = before if stale_last and t == k - 1 else W
        grad = src @ HHt[t, :] - XHt[:, t]
        wt = W[:, t]
        pg = np.where(wt == 0, np.minimum(0.0, grad), grad)
        a = np.abs(pg)
        violation += float((a[:-drop_rows] if drop_rows else a).sum(dtype=np.float64))
        hess = HHt[t, t]
        if hess != 0:
            W[:, t] = np.maximum(wt - grad / hess, 0.0)
    return violation


def _half(X, W, Ht, l1_reg, l2_reg, round_bits=0, **sweep):
    """nmf_cd.update_coordinate_descent with one switch: the factor operand of the X.Ht product rounded."""
    k = Ht.shape[1]
    HHt = Ht.T @ Ht
    XHt = X @ (round_mantissa(Ht, round_bits) if round_bits else Ht)
    if l2_reg != 0.0:
        HHt.flat[:: k + 1] += l2_reg
    if l1_reg != 0.0:
        XHt -= l1_reg
    return _sweep(W, HHt, XHt, **sweep)


MUTANTS = {
    None: ({}, {}),
    "a": (dict(round_bits=11), {}),             # W half-step: a lost low f16 plane of the factor operand
    "b": (dict(drop_rows=13), {}),              # W half-step: a dead-lane slip in the violation sum
    "c": ({}, dict(no_l1=True)),                # H half-step: l1_reg left out
    "d": (dict(stale_last=True), {}),           # W half-step: the last component reads the factor of before the sweep
}


def mutant_run(X, W0, H0, reg, mutant, ts=TS):
    """The loop of nmf_cd.fit_coordinate_descent (tol = 0, update_H) in float64 with one mutation.
    Returns ({t: (W, H)}, {t: violation ratio})."""
    w_kw, h_kw = (dict(d) for d in MUTANTS[mutant])
    X = np.asarray(X, dtype=np.float64)
    W, Ht = W0.astype(np.float64), np.ascontiguousarray(H0.astype(np.float64).T)
    l1W, l1H, l2W, l2H = nmf_cd.regularization(X.shape[0], X.shape[1], **reg)
    if h_kw.pop("no_l1", False):
        l1H = 0.0
    snaps, ratio, trace = {}, {}, []
    for it in range(1, max(ts) + 1):
        v = 0.0
        v += _half(X, W, Ht, l1W, l2W, **w_kw)
        v += _half(X.T, Ht, W, l1H, l2H, **h_kw)
        trace.append(v)
        if it in ts:
            snaps[it] = (W.copy(), Ht.T.copy())
            ratio[it] = v / trace[0]
    return snaps, ratio
