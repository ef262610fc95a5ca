"""Reference side of tests/test_gpu_mu_steps.py: single multiplicative-update iterations of oracle/nmf_mu.py from explicit
float32 start factors -- the float64 oracle (the reference), its float32 restatement and the plane restatement (the two
yardsticks), the distances between such runs, and mutants of the plane restatement.

Nothing here touches the device.  Every reference is computed once per process (functools.lru_cache) and returned
read-only.

The plane restatement (``model_fit`` with ``planes=True``) follows nmf_mu.fit_mu line by line in float64 and applies only
the roundings that the header of cnmf_amd/csrc/kernels_mu_mfma.hip.h declares:
  * W and H enter ``S = W.H`` as two bf16 planes hi + lo                               (header lines 9-10)
  * the quotient enters the second product as two bf16 planes (mu_planes8, line 114; for Itakura-Saito both ratios,
    header lines 5-6), and so does the factor it is multiplied with (the plane copies, header lines 16-17)
  * S is a float32 accumulator when it is clamped and divided                          (header line 11)
  * the updated factor is stored as float32 (MuSlotDev.W / .Ht, lines 43-44)
It knows nothing of tiles, chunks, register layouts or the order of the kernel's sums.  With ``planes=False`` and no mutant
it IS nmf_mu.fit_mu, bit for bit (test_the_unmutated_model_is_the_oracle).
"""
import functools

import numpy as np

from cnmf_amd import synth
from oracle import nmf_cd, nmf_mu
from tests._cd_steps_ref import FACTOR, REGS, TS, d_cols, d_rows      # noqa: F401  (the test module reads them from here)
from tests._cd_steps_ref import matrix as _cd_matrix

EPS = nmf_mu.EPSILON
BETAS = {"kl": 1, "is": 0}
BETA_NAMES = {"kl": "kullback-leibler", "is": "itakura-saito"}

RANKS_M = tuple(list(range(1, 17)) * 2 + [1, 16] + [17, 20, 24, 31, 32] + [33, 40, 48, 63, 64])
# name: (matrix, ranks, seed of the RandomState the restart seeds come from)
BATCHES = {
    "M": ("A", RANKS_M, 51),                          # matrix pipe and (ranks <= 32) non-zero path, Kullback-Leibler
    "I": ("A+", (3, 9, 16, 17, 24, 40, 64), 52),      # matrix pipe, Itakura-Saito
    "T": ("T", (1, 3, 16, 17, 33), 53),
    "T+": ("T+", (1, 3, 16, 17, 33), 53),
    "L": ("L", (5, 12, 24, 40), 54),
    "Ln": ("L", (7, 16, 24, 32), 55),                 # non-zero path
    "P": ("P", (7, 16, 24, 32), 56),
    "V": ("A", (1, 5, 8, 9, 16, 17, 32, 33, 64), 57),  # vector-ALU
    "V+": ("A+", (1, 5, 8, 9, 16, 17, 32, 33, 64), 57),
    "VT": ("T", (3, 9), 58),
    "VT+": ("T+", (3, 9), 58),
    "E": ("A", (5, 20), 59),                          # planted edges (PLANTS below)
    "Ez": ("Az", (5, 20), 59),
    "C": ("A", (5, 9, 20), 61),                       # the clamp planted (plant "tiny"); mutant (e)
    "B+": ("A+", (5, 9, 20), 60),                     # Itakura-Saito variant of mutant (b): CPU only
}
PLANTS = ("dead", "hplant", "xzero", "tiny")                   # test_the_inputs_hold_what_they_claim describes them
ZERO_CELL, ZERO_GENE = 77, 123
TINY_GENES = {10: 0.3, 200: 1.0, 400: 3.0}             # gene: the median of column g of W0.H0 in units of eps (plant "tiny")
PLANT_BATCH = {"dead": "E", "hplant": "E", "xzero": "Ez", "tiny": "C"}


def pad_mfma(k):
    return 16 if k <= 16 else 32 if k <= 32 else 64


def pad_valu(k):
    return 8 if k <= 8 else pad_mfma(k)


PAD = {"mfma": pad_mfma, "nz": pad_mfma, "valu": pad_valu}


def _frozen(a):
    a.setflags(write=False)
    return a


def sparse_counts(n, g, mu_lib, seed):
    """As test_gpu_mu_sparse._sparse_counts, in float64."""
    C, _ = synth.topic_counts(n, g, 6, mu_lib, 0.4, seed)
    return synth.normalise_like_prepare(C, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """A (517 x 500, tests/_cd_steps_ref.py), T = its first 45 cells x 70 genes, L = C1 at 1061 cells x its first 300
    genes, P = sparse topic counts (under 25 % non-zero), Az = A with one all-zero cell and one all-zero gene; ``+``:
    plus 1e-3 (strictly positive, for Itakura-Saito).  float64, every value a float32 value."""
    if name.endswith("+"):
        X = matrix(name[:-1]) + 1e-3
    elif name == "A":
        X = _cd_matrix("A")
    elif name == "T":
        X = _cd_matrix("A")[:45, :70]
    elif name == "L":
        X = synth.make_config("C1", dtype=np.float64, n_cells=1061)[:, :300]
    elif name == "P":
        X = sparse_counts(1301, 1100, 4.6, 31)
    else:
        assert name == "Az"
        X = _cd_matrix("A").copy()
        X[ZERO_CELL, :] = 0.0
        X[:, ZERO_GENE] = 0.0
    return _frozen(np.ascontiguousarray(X.astype(np.float32).astype(np.float64)))


@functools.lru_cache(maxsize=None)
def batch(name):
    mname, ks, s = BATCHES[name]
    rs = np.random.RandomState(s)
    return mname, tuple(ks), tuple(int(x) for x in rs.randint(1, 2**31 - 1, size=len(ks)))


@functools.lru_cache(maxsize=None)
def inits(bname, plant=None):
    """Float32 start factors [(W0, H0)] of every restart: drawn once, the same bits go to every side.  ``plant``:
    "dead" -- component 1 of W0 all zero (the planted batches have ranks >= 5);
    "hplant" -- about 8 % of H0 exactly 0 and another 8 % equal to 1e-30;
    "tiny" -- the columns TINY_GENES of H0 scaled down so that S = W0.H0 sits around eps = 1.2e-7 there (medians 0.3, 1
    and 3 eps): the only inputs here on which max(S, eps) acts at entries where X is not zero."""
    mname, ks, seeds = batch(bname)
    X32 = matrix(mname).astype(np.float32)
    out = []
    for j, (k, seed) in enumerate(zip(ks, seeds)):
        W0, H0 = nmf_cd.random_init(X32, k, seed)
        assert W0.dtype == H0.dtype == np.float32
        if plant == "dead":
            W0[:, 1] = 0.0
        elif plant == "hplant":
            u = np.random.RandomState(700 + j).random_sample(H0.shape)
            H0[u < 0.08] = 0.0
            H0[u > 0.92] = np.float32(1e-30)
        elif plant == "tiny":
            for g, units in TINY_GENES.items():
                med = np.median(W0.astype(np.float64) @ H0[:, g].astype(np.float64))
                H0[:, g] *= np.float32(units * float(EPS) / med)
        else:
            assert plant in (None, "xzero")
        out.append((_frozen(W0), _frozen(H0)))
    return tuple(out)


# ---------------------------------------------------------------- the bf16 plane split
def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even) as float32.  A finite input whose rounding would overflow takes the
    largest finite bf16 instead (the hardware conversion gives infinity there; no factor or quotient comes near 3.4e38)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000)
    over = ((r & 0x7F800000) == 0x7F800000) & ((u & 0x7F800000) != 0x7F800000)
    r = np.where(over, u & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def split_bf16(x):
    """(hi, lo) float32 arrays, both bf16 values: hi = bf16(x), lo = bf16(x - hi) -- mu_split_bf16 of the kernel header."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_round(x)
    with np.errstate(over="ignore"):
        lo = bf16_round(x - hi)                       # (x - hi has at most 16 significant bits: exact in float32)
    return hi, lo


def planes(x, lo_plane=True):
    """x as the matrix pipe sees it, in float64: hi + lo (``lo_plane=False``: hi alone)."""
    hi, lo = split_bf16(x)
    return hi.astype(np.float64) + lo.astype(np.float64) if lo_plane else hi.astype(np.float64)


def _r32(a):
    return a.astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------- the model: fit_mu with declared roundings and mutants
MUTANTS = ("a", "b", "c", "d", "e", "f", "g")
#   a  the lo plane of W is dropped in S = W.H
#   b  the lo plane of the quotient is dropped (Itakura-Saito: of 1 / S)
#   c  the last 32 genes (the reduced dimension) are missing from the W half-step's numerator
#   d  one 32-cell chunk (cells 224..255, the 8th of 24) is missing from the H half-step's numerator
#   e  S + eps instead of max(S, eps)
#   f  the Kullback-Leibler denominator of the W half-step comes from the H of the previous iteration
#   g  the divergence misses the sum(WH) - sum(X) term
CHUNK_D = 7


class _Model:
    def __init__(self, beta, use_planes, mutant):
        assert mutant is None or mutant in MUTANTS
        self.beta, self.pl, self.m = beta, use_planes, mutant
        self.stale_hsum = None

    def P(self, a):                                    # a factor operand of an MFMA
        return planes(a) if self.pl else a

    def S(self, W, H):
        Wp = planes(W, lo_plane=self.m != "a") if self.pl else W
        S = Wp @ self.P(H)
        return _r32(S) if self.pl else S

    def ratio(self, X, W, H):
        """nmf_mu._ratio."""
        WH_safe = self.S(W, H)
        WH = WH_safe.copy()
        if self.m == "e":
            WH_safe += EPS
            WH += EPS
        else:
            if self.beta - 1.0 < 0:
                WH[WH < EPS] = EPS
            WH_safe[WH_safe < EPS] = EPS
        if self.beta == 1:
            R = X / WH_safe
            return (planes(R, lo_plane=self.m != "b") if self.pl else R), None
        R = WH_safe ** -1
        R **= 2
        R *= X
        WH **= self.beta - 1
        if self.pl:
            R, WH = planes(R), planes(WH, lo_plane=self.m != "b")
        return R, WH

    def update_w(self, X, W, H, l1, l2, gamma):
        """nmf_mu.mu_update_w."""
        R, WHp = self.ratio(X, W, H)
        Hp = self.P(H)
        num = R[:, :-32] @ Hp[:, :-32].T if self.m == "c" else R @ Hp.T
        if self.beta == 1:
            den = np.sum(H, axis=1)[np.newaxis, :]
            if self.m == "f":
                den, self.stale_hsum = (den if self.stale_hsum is None else self.stale_hsum), den
        else:
            den = WHp @ Hp.T
        if l1 > 0:
            den = den + l1
        if l2 > 0:
            den = den + l2 * W
        den = np.array(np.broadcast_to(den, W.shape))
        den[den == 0] = EPS
        num /= den
        if gamma != 1:
            num **= gamma
        W *= num
        return _r32(W) if self.pl else W

    def update_h(self, X, W, H, l1, l2, gamma):
        """nmf_mu.mu_update_h."""
        R, WHp = self.ratio(X, W, H)
        Wp = self.P(W)
        if self.m == "d":
            keep = np.r_[0:32 * CHUNK_D, 32 * (CHUNK_D + 1):X.shape[0]]
            num = Wp[keep].T @ R[keep]
        else:
            num = Wp.T @ R
        if self.beta == 1:
            W_sum = np.sum(W, axis=0)
            W_sum[W_sum == 0] = 1.0
            den = W_sum[:, np.newaxis]
        else:
            den = Wp.T @ WHp
        if l1 > 0:
            den = den + l1
        if l2 > 0:
            den = den + l2 * H
        den = np.array(np.broadcast_to(den, H.shape))
        den[den == 0] = EPS
        num /= den
        if gamma != 1:
            num **= gamma
        H *= num
        return _r32(H) if self.pl else H

    def divergence(self, X, W, H):
        """nmf_mu.beta_divergence(square_root=True), S formed as the updates form it."""
        WH_data = self.S(W, H).ravel()
        X_data = X.ravel()
        idx = X_data > EPS
        WH_data = WH_data[idx]
        X_data = X_data[idx]
        WH_data[WH_data < EPS] = EPS
        div = X_data / WH_data
        if self.beta == 1:
            res = np.dot(X_data, np.log(div))
            if self.m != "g":
                res += np.dot(W.sum(axis=0), H.sum(axis=1)) - X_data.sum()
        else:
            res = np.sum(div) - np.prod(X.shape) - np.sum(np.log(div))
        return np.sqrt(2 * max(res, 0))


def model_fit(X, W0, H0, beta, reg, ts=TS, use_planes=True, mutant=None):
    """The loop of nmf_mu.fit_mu (tol = 0) on float64 copies of the float32 start factors.  Returns {t: (W, H, err)}."""
    X = np.asarray(X, dtype=np.float64)
    m = _Model(beta, use_planes, mutant)
    W, H = W0.astype(np.float64), H0.astype(np.float64)
    l1W, l1H, l2W, l2H = nmf_cd.regularization(X.shape[0], X.shape[1], **reg)
    gamma = 1.0 / (2.0 - beta) if beta < 1 else 1.0
    out = {}
    for n_iter in range(1, max(ts) + 1):
        W = m.update_w(X, W, H, l1W, l2W, gamma)
        if beta < 1:
            W[W < np.finfo(np.float64).eps] = 0.0
        H = m.update_h(X, W, H, l1H, l2H, gamma)
        if beta <= 1:
            H[H < np.finfo(np.float64).eps] = 0.0
        if n_iter in ts:
            out[n_iter] = (W.copy(), H.copy(), float(m.divergence(X, W, H)))
    return out


# ---------------------------------------------------------------- distances that survive a dead component
def dist_W(W, W64):
    """d_cols over the components that live in the float64 oracle; a component that is all zero there must be all zero in
    ``W`` (else: inf)."""
    W, W64 = np.asarray(W), np.asarray(W64)
    live = np.abs(W64).max(axis=0) > 0
    if not (np.asarray(W)[:, ~live] == 0).all():
        return np.inf
    return d_cols(W[:, live], W64[:, live]) if live.any() else 0.0


def dist_H(H, H64):
    return dist_W(np.asarray(H).T, np.asarray(H64).T)


def d_err(e, e64):
    return abs(float(e) - e64) / e64


# ---------------------------------------------------------------- the reference runs
def run_triple(X64, W0, H0, beta, reg, ts=TS):
    """One restart from the float32 factors (W0, H0), tol = 0, max(ts) iterations: the float64 oracle, its float32
    restatement (nmf_mu.fit_mu on float32 X, W0, H0) and the plane restatement.  Per t: the oracle's ``W``, ``H``, ``e``
    = sqrt(2 D); ``y32`` / ``ypl``: {"W", "H", "e"} -> each restatement's own distance from the oracle."""
    tmax = max(ts)
    l1W, l1H, l2W, l2H = nmf_cd.regularization(X64.shape[0], X64.shape[1], **reg)
    s64 = {t: None for t in ts}
    n64 = nmf_mu.fit_mu(X64, W0.astype(np.float64), H0.astype(np.float64), beta, 0.0, tmax, l1W, l1H, l2W, l2H,
                        snapshots=s64)[2]
    X32 = X64.astype(np.float32)
    s32 = {t: None for t in ts}
    W32, H32, n32 = nmf_mu.fit_mu(X32, W0.copy(), H0.copy(), beta, 0.0, tmax, l1W, l1H, l2W, l2H, snapshots=s32)
    assert n64 == n32 == tmax and W32.dtype == H32.dtype == np.float32
    spl = model_fit(X64, W0, H0, beta, reg, ts)
    out = {"k": W0.shape[1], "W": {}, "H": {}, "e": {}, "y32": {}, "ypl": {}}
    for t in ts:
        W, H = s64[t]
        e = float(nmf_mu.beta_divergence(X64, W, H, beta, square_root=True))
        out["W"][t], out["H"][t], out["e"][t] = _frozen(W), _frozen(H), e
        w32, h32 = s32[t]
        assert w32.dtype == h32.dtype == np.float32
        e32 = nmf_mu.beta_divergence(X32, w32, h32, beta, square_root=True)
        # (Itakura-Saito: the float32 sums meet the integer N G of nmf_mu.beta_divergence, as in scikit-learn; numpy makes
        # that last subtraction a float64 one)
        assert beta == 0 or np.asarray(e32).dtype == np.float32
        out["y32"][t] = {"W": dist_W(w32, W), "H": dist_H(h32, H), "e": d_err(e32, e)}
        wp, hp, ep = spl[t]
        out["ypl"][t] = {"W": dist_W(wp, W), "H": dist_H(hp, H), "e": d_err(ep, e)}
    return out


class Reference:
    """The reference runs of the restarts of a batch."""

    def __init__(self, runs):
        self.runs = runs                # {restart index: run_triple dict}


@functools.lru_cache(maxsize=None)
def reference(bname, loss, regname, plant=None):
    mname = batch(bname)[0]
    X64 = matrix(mname)
    return Reference({i: run_triple(X64, W0, H0, BETAS[loss], REGS[regname])
                      for i, (W0, H0) in enumerate(inits(bname, plant))})


# ---------------------------------------------------------------- the cells and their yardsticks
_PLANTED = tuple((PLANT_BATCH[p], "kl", "none", p, None) for p in PLANTS)
# path: every case the device is compared on, as (batch, loss, penalty, plant, largest rank compared)
CASES = {
    "mfma": (("M", "kl", "none", None, None), ("M", "kl", "mixed", None, None), ("I", "is", "none", None, None),
             ("I", "is", "mixed", None, None), ("T", "kl", "none", None, None), ("T+", "is", "none", None, None),
             ("L", "kl", "none", None, None), ("P", "kl", "none", None, None)) + _PLANTED,
    "nz": (("M", "kl", "none", None, 32), ("M", "kl", "mixed", None, 32), ("T", "kl", "none", None, 32),
           ("Ln", "kl", "none", None, None), ("P", "kl", "none", None, None)) + _PLANTED,
    "valu": (("V", "kl", "none", None, None), ("V", "kl", "mixed", None, None), ("V+", "is", "none", None, None),
             ("V+", "is", "mixed", None, None), ("VT", "kl", "none", None, None), ("VT+", "is", "none", None, None))
            + _PLANTED,
}


def members(path, case):
    """The restarts of a case that are compared on ``path``."""
    bname, loss, regname, plant, max_rank = case
    assert case in CASES[path], (path, case)
    return [i for i, r in sorted(reference(bname, loss, regname, plant).runs.items()) if max_rank is None or r["k"] <= max_rank]


@functools.lru_cache(maxsize=None)
def yardstick(path, loss, what, t, pad):
    """The yardstick of the cell (path, loss, padded rank, quantity, t): the maximum, over every restart of that padded
    rank in every case of CASES[path] with that loss, of the float32 restatement's distance from the oracle and, on the
    matrix pipe, of the plane restatement's."""
    ys = []
    for case in CASES[path]:
        if case[1] != loss:
            continue
        runs = reference(*case[:4]).runs
        for i in members(path, case):
            if PAD[path](runs[i]["k"]) == pad:
                ys.append(runs[i]["y32"][t][what])
                if path == "mfma":
                    ys.append(runs[i]["ypl"][t][what])
    return max(ys)


def cells(path):
    """{(loss, padded rank)} of CASES[path]."""
    return sorted({(c[1], PAD[path](reference(*c[:4]).runs[i]["k"])) for c in CASES[path] for i in members(path, c)})
