"""Reference side of tests/test_gpu_mu_wide_steps.py and tests/test_gpu_mu_wide.py: the multiplicative-update solver at
ranks 65..128 (padded rank 128, the opt-in ``Engine.mu_rank_limit = 128``).

Everything that defines the comparison comes from tests/_mu_steps_ref.py unchanged: the matrices, ``run_triple`` (the
float64 oracle, its float32 restatement and the plane restatement from the same float32 start factors), the distances, the
penalties, TS = (1, 2, 3) and FACTOR = 16.  This file adds the batches of wide ranks, their planted start factors (R.inits
is keyed to its own batches) and the yardstick of the one padded rank there is.

Nothing here touches the device.  Every reference is computed once per process and returned read-only.
"""
import contextlib
import functools

import numpy as np

from oracle import nmf_cd
from tests import _mu_steps_ref as R

PAD = 128
FILL_RANKS = (9, 9, 40)                       # ride along with the Kullback-Leibler batch on A: a mixed-group call
# name: (matrix, ranks, seed of the RandomState the restart seeds come from)
BATCHES = {
    "WA": ("A", (65, 80, 96, 127, 128, 128, 65), 71),
    "WI": ("A+", (65, 96, 128), 72),
    "WT": ("T", (65, 128), 73),
    "WT+": ("T+", (65,), 73),
    "WL": ("L", (80,), 74),
    "WE": ("A", (70,), 75),                   # planted edges
    "FILL": ("A", FILL_RANKS, 76),
}
PLANTS = ("dead", "tiny")
DEAD_COMPONENT = 66                           # (>= 64: a component of the second component half of the workgroup)
# every case the device is compared on, as (batch, loss, penalty, plant)
CASES = (("WA", "kl", "none", None), ("WA", "kl", "mixed", None), ("WI", "is", "none", None), ("WI", "is", "mixed", None),
         ("WT", "kl", "none", None), ("WT+", "is", "none", None), ("WL", "kl", "none", None),
         ("WE", "kl", "none", "dead"), ("WE", "kl", "none", "tiny"))


@contextlib.contextmanager
def wide_limit(engine):
    """The engine accepts multiplicative-update ranks up to 128 inside the block and its previous limit afterwards."""
    prev = engine.mu_rank_limit
    engine.mu_rank_limit = 128
    try:
        yield engine
    finally:
        engine.mu_rank_limit = prev


@functools.lru_cache(maxsize=None)
def batch(name):
    mname, ks, s = BATCHES[name]
    rs = np.random.RandomState(s)
    return mname, tuple(ks), tuple(int(x) for x in rs.randint(1, 2**31 - 1, size=len(ks)))


@functools.lru_cache(maxsize=None)
def inits(bname, plant=None):
    """Float32 start factors [(W0, H0)] of every restart (nmf_cd.random_init on the float32 matrix).  ``plant``:
    "dead" -- component DEAD_COMPONENT of W0 all zero; "tiny" -- the gene columns R.TINY_GENES of H0 scaled down so that
    S = W0.H0 sits around eps there (medians 0.3, 1 and 3 eps), as in R.inits."""
    mname, ks, seeds = batch(bname)
    X32 = R.matrix(mname).astype(np.float32)
    out = []
    for k, seed in zip(ks, seeds):
        W0, H0 = nmf_cd.random_init(X32, k, seed)
        assert W0.dtype == H0.dtype == np.float32
        if plant == "dead":
            W0[:, DEAD_COMPONENT] = 0.0
        elif plant == "tiny":
            for g, units in R.TINY_GENES.items():
                med = np.median(W0.astype(np.float64) @ H0[:, g].astype(np.float64))
                H0[:, g] *= np.float32(units * float(R.EPS) / med)
        else:
            assert plant is None
        for a in (W0, H0):
            a.setflags(write=False)
        out.append((W0, H0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(bname, loss, regname, plant=None):
    """{restart index: R.run_triple dict} of the restarts of a batch."""
    X64 = R.matrix(batch(bname)[0])
    return {i: R.run_triple(X64, W0, H0, R.BETAS[loss], R.REGS[regname]) for i, (W0, H0) in enumerate(inits(bname, plant))}


@functools.lru_cache(maxsize=None)
def yardstick(loss, what, t):
    """The yardstick of the cell (loss, quantity, t) at padded rank 128: the maximum, over every restart of every case of
    that loss, of the float32 restatement's and the plane restatement's own distance from the float64 oracle."""
    ys = []
    for case in CASES:
        if case[1] != loss:
            continue
        for r in reference(*case).values():
            ys += [r["y32"][t][what], r["ypl"][t][what]]
    return max(ys)
