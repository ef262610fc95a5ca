"""Reference side of tests/test_gpu_mu_nz_wide_steps.py and tests/test_gpu_mu_nz_wide.py: Kullback-Leibler multiplicative
updates on the NON-ZEROS of the matrix at ranks 33..64 (padded rank 64, two lanes per row; the opt-in
``Engine.mu_sparse_rank_limit = 64``).

Everything that defines the comparison comes from tests/_mu_steps_ref.py unchanged: the matrices, ``run_triple`` (the
float64 oracle and its float32 restatement from the same float32 start factors), the distances, the penalties,
TS = (1, 2, 3) and FACTOR = 16.  This file adds the batches of ranks 33..64, their planted start factors, the filler
restarts that ride along in every call and the yardstick of the one padded rank there is: as on the ``nz`` path of
_mu_steps_ref.py, the float32 restatement's own distance from the float64 oracle (``y32``), pooled over every restart of
every case.

Nothing here touches the device.  Every reference is computed once per process and returned read-only.
"""
import contextlib
import functools

import numpy as np

from oracle import nmf_cd
from tests import _mu_steps_ref as R

PAD = 64
BS = 128 * 1024 // (4 * PAD)                 # rows of the other side per block of the factor in LDS: 512
FILL_RANKS = (9, 24, 70)                     # behind the compared restarts: non-zero groups 16 / 32, a dense group at 128
# name: (matrix, ranks, seed of the RandomState the restart seeds come from)
BATCHES = {
    "NA": ("A", (33, 37, 41, 45, 49, 53, 57, 61, 64), 81),   # every live-quad count 9..16; an odd-sized batch
    "NP": ("P", (33, 40, 64), 82),
    "NT": ("T", (33, 64), 83),
    "NL": ("L", (40,), 84),
    "NE": ("A", (40,), 85),                  # planted edges
    "NEz": ("Az", (40,), 85),
}
PLANTS = ("dead", "xzero", "tiny")
PLANT_BATCH = {"dead": "NE", "xzero": "NEz", "tiny": "NE"}
EXACT_ZERO_PLANTS = ("dead", "xzero")        # the exact zeros of these equal the oracle's
# Lane half h of a pair holds the logical quads h, h + 2, h + 4, ... of its row (kernels_mu_sparse.hip.h, sp_slices_pair):
# the components of the odd quads sit in the SECOND lane half.
DEAD_COMPONENT = 22                          # quad 5 of the 10 live quads of rank 40


def lane_half(component):
    return (component // 4) % 2


# every case the device is compared on, as (batch, loss, penalty, plant)
CASES = (("NA", "kl", "none", None), ("NA", "kl", "mixed", None), ("NP", "kl", "none", None), ("NT", "kl", "none", None),
         ("NL", "kl", "none", None)) + tuple((PLANT_BATCH[p], "kl", "none", p) for p in PLANTS)


@contextlib.contextmanager
def nz_wide_limit(engine):
    """The engine runs Kullback-Leibler on the non-zeros up to rank 64 inside the block and as before afterwards."""
    prev = engine.mu_sparse_rank_limit
    engine.mu_sparse_rank_limit = 64
    try:
        yield engine
    finally:
        engine.mu_sparse_rank_limit = prev


@functools.lru_cache(maxsize=None)
def batch(name):
    mname, ks, s = BATCHES[name]
    rs = np.random.RandomState(s)
    return mname, tuple(ks), tuple(int(x) for x in rs.randint(1, 2**31 - 1, size=len(ks)))


def _frozen_pair(W0, H0):
    assert W0.dtype == H0.dtype == np.float32
    for a in (W0, H0):
        a.setflags(write=False)
    return W0, H0


@functools.lru_cache(maxsize=None)
def inits(bname, plant=None):
    """Float32 start factors [(W0, H0)] of every restart (nmf_cd.random_init on the float32 matrix).  ``plant``:
    "dead" -- component DEAD_COMPONENT of W0 all zero; "tiny" -- the gene columns R.TINY_GENES of H0 scaled down so that
    S = W0.H0 sits around eps there (medians 0.3, 1 and 3 eps), as in R.inits; "xzero" -- nothing (the matrix is planted)."""
    mname, ks, seeds = batch(bname)
    X32 = R.matrix(mname).astype(np.float32)
    out = []
    for k, seed in zip(ks, seeds):
        W0, H0 = nmf_cd.random_init(X32, k, seed)
        if plant == "dead":
            W0[:, DEAD_COMPONENT] = 0.0
        elif plant == "tiny":
            for g, units in R.TINY_GENES.items():
                med = np.median(W0.astype(np.float64) @ H0[:, g].astype(np.float64))
                H0[:, g] *= np.float32(units * float(R.EPS) / med)
        else:
            assert plant in (None, "xzero")
        out.append(_frozen_pair(W0, H0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fill_inits(mname):
    """Start factors of the filler restarts (ranks FILL_RANKS) on matrix ``mname``."""
    X32 = R.matrix(mname).astype(np.float32)
    return tuple(_frozen_pair(*nmf_cd.random_init(X32, k, 9000 + k)) for k in FILL_RANKS)


@functools.lru_cache(maxsize=None)
def reference(bname, loss, regname, plant=None):
    """{restart index: R.run_triple dict} of the restarts of a batch."""
    X64 = R.matrix(batch(bname)[0])
    return {i: R.run_triple(X64, W0, H0, R.BETAS[loss], R.REGS[regname]) for i, (W0, H0) in enumerate(inits(bname, plant))}


@functools.lru_cache(maxsize=None)
def yardstick(what, t):
    """The yardstick of the cell (quantity, t) at padded rank 64: the maximum, over every restart of every case, of the
    float32 restatement's own distance from the float64 oracle."""
    return max(r["y32"][t][what] for case in CASES for r in reference(*case).values())
