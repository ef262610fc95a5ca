"""Generate tests/golden/ref_select_mi.npz by running the UNMODIFIED reference's ``Preprocess.select_features_MI``
(preprocess.py:425-467) on the CPU with the installed sklearn (``mutual_info_classif``).

The scanpy stand-in is tools/make_golden_preprocess.py's, with ``normalize_total(target_sum=None)``: the target is the
median of the positive row sums (scanpy's rule), X * (target / row sum), 0 for a cell without counts.

Input: seeded ``synth.topic_counts`` (PARAMS); labels: the topic that best explains a cell's counts (the big classes),
plus classes of 1, 2, 3, 5, 7 and 8 cells (TINY) at the end; the GPU test regenerates them.
  Run A: dense input, fresh Preprocess(random_seed=SEED_A), the defaults, integer labels.
  Run B: CSR input, max_scaled_thresh=5.0, quantile_thresh=None, n_top_features=20, string labels; before the call the
         global RandomState draws PRE_B_INTS integers and one normal, so that pos is mid-block and a Gaussian is cached.
Stored per run (prefix a_ / b_): MI, MI_Rank, MI_diff, highly_variable; target (the median), std (the ddof=1 std of the
normalised columns), thresh (the ceiling, +inf for none); the global RandomState state before and after the call
(key, pos, has_gauss, gauss).  The tool asserts that the reference's X equals min(normalised / std, thresh) bit for bit.

Run:  python tools/make_golden_select_mi.py      (seconds; needs the reference source tree scanpy_shim.REFERENCE_SRC names)
"""
import os
import sys

import numpy as np
import pandas as pd
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_preprocess as mgp  # noqa: E402
from cnmf_amd import synth  # noqa: E402

# (n_cells, n_genes, k_true, mu_lib, sigma_lib, seed)
PARAMS = (500, 120, 4, 6.0, 0.4, 23)
TINY = (1, 2, 3, 5, 7, 8)
SEED_A, SEED_B, PRE_B_INTS = 3, 17, 101


def make_inputs():
    """counts (float64 ndarray), cell names, gene names, integer labels"""
    n, g, k, mu, sg, seed = PARAMS
    C, H = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    C = C.astype(np.float64)
    labels = np.argmax(C @ H.T.astype(np.float64), axis=1).astype(np.int64)
    start = n - sum(TINY)
    for c, size in enumerate(TINY):
        labels[start:start + size] = 100 + c
        start += size
    return C, ["c%d" % i for i in range(n)], ["g%d" % j for j in range(g)], labels


def normalize_total(adata, target_sum=None, copy=False):
    if target_sum is None:
        rs = np.asarray(adata.X.sum(axis=1)).ravel()
        target_sum = np.median(rs[rs > 0])
        adata.uns_target = target_sum
    return mgp.normalize_total(adata, target_sum=target_sum, copy=copy)


def state_dict(prefix, st):
    return {prefix + "_key": np.asarray(st[1], dtype=np.uint32), prefix + "_pos": np.array(st[2]),
            prefix + "_has_gauss": np.array(st[3]), prefix + "_gauss": np.array(st[4])}


def main():
    mgp.AnnData.uns_target = None
    scanpy = mgp.make_scanpy()
    scanpy.pp.normalize_total = normalize_total
    sys.modules["scanpy"] = scanpy
    ref = mgp.load_reference()
    sys.modules["scanpy"] = scanpy
    ref.sc = scanpy
    C, cells, genes, labels = make_inputs()
    store = {"params": np.array(PARAMS, dtype=np.float64), "tiny": np.array(TINY), "labels": labels,
             "seeds": np.array([SEED_A, SEED_B, PRE_B_INTS])}
    runs = {"a": dict(X=C.copy(), cluster=labels, kw={}, seed=SEED_A),
            "b": dict(X=sp.csr_matrix(C), cluster=np.array(["L%d" % v for v in labels]),
                      kw=dict(max_scaled_thresh=5.0, quantile_thresh=None, n_top_features=20), seed=SEED_B)}
    for tag, run in runs.items():
        P = ref.Preprocess(random_seed=run["seed"])
        if tag == "b":
            np.random.randint(0, 1000, size=PRE_B_INTS)
            np.random.standard_normal(1)
            st = np.random.get_state()
            assert st[3] == 1 and 0 < st[2] < 624, st[2:]
        store.update(state_dict(tag + "_before", np.random.get_state()))
        a = mgp.AnnData(run["X"], pd.DataFrame(index=cells), pd.DataFrame(index=genes))
        P.select_features_MI(a, run["cluster"], makeplots=False, **run["kw"])
        store.update(state_dict(tag + "_after", np.random.get_state()))
        var = a.var
        assert list(var.index) == genes
        for col in ("MI", "MI_Rank", "MI_diff", "highly_variable"):
            store["%s_%s" % (tag, col)] = var[col].values
        assert var["MI_Rank"].dtype == np.float64 and var["highly_variable"].dtype == bool
        # the reference's X: min(normalised / std, thresh)
        target, std = a.uns_target, a.uns_std
        rs = C.sum(axis=1)
        norm = C * np.where(rs > 0, target / np.where(rs > 0, rs, 1.0), 0.0)[:, None]
        y = norm / std
        mv = run["kw"].get("max_scaled_thresh")
        if mv is not None:
            y[y > mv] = mv
        q = run["kw"].get("quantile_thresh", .9999)
        thresh = np.quantile(y.reshape(-1), q) if q is not None else np.inf
        X = np.asarray(a.X.todense()) if sp.issparse(a.X) else a.X
        assert np.array_equal(np.minimum(y, thresh), X), tag
        store[tag + "_target"], store[tag + "_std"], store[tag + "_thresh"] = np.array(target), std, np.array(thresh)
        print(tag, "MI > 0 for %d of %d genes" % ((var["MI"] > 0).sum(), len(genes)), "state pos", store[tag + "_after_pos"])
    out = os.path.join(ROOT, "tests", "golden", "ref_select_mi.npz")
    np.savez_compressed(out, **store)
    print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
