"""Multiplicative updates at ranks 65..128 (Engine.mu_rank_limit = 128) against rank 64 on the unchanged kernels, at
50000 x 2000 (synth C3): time per restart-iteration of a batch of 32 restarts, Kullback-Leibler and Itakura-Saito, and the
float64 refit (mu_refit_f64) at k = 128 against k = 64.  Every timed call ends in a device synchronise (the results come
back to the host); a warm-up call first, then the median of --repeats.  Writes one JSON file.

    python tools/mu_wide_probe.py --out profiles/mu_wide_ranks_50000x2000.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnmf_amd import synth                                      # noqa: E402
from cnmf_amd.engine import Engine                              # noqa: E402


def median_of(fn, repeats):
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), [round(x, 4) for x in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--refit-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    X = synth.make_config("C3", dtype=np.float32, n_cells=a.cells)
    out = {"shape": list(X.shape), "batch": a.batch, "iterations": a.iters, "repeats": a.repeats, "mu_batch": [], "mu_refit_f64": []}
    eng = Engine(0, mu_rank_limit=128)
    seeds = list(range(7, 7 + a.batch))
    for loss, M in (("kullback-leibler", X), ("itakura-saito", X + np.float32(1e-3))):
        eng.set_matrix(M)
        for k in (64, 96, 128):
            kw = dict(seeds=seeds, beta_loss=loss, tol=0, warn=False)
            eng.nmf_mu_batch([k] * a.batch, max_iter=2, **kw)                                   # warm up (X^T, code objects, pools)
            # two lengths: the difference leaves out what a call pays once (the seeded start factors, the results back)
            med1, ts1 = median_of(lambda: eng.nmf_mu_batch([k] * a.batch, max_iter=a.iters, **kw), a.repeats)
            med3, ts3 = median_of(lambda: eng.nmf_mu_batch([k] * a.batch, max_iter=3 * a.iters, **kw), a.repeats)
            row = {"loss": loss, "k": k, "iterations": [a.iters, 3 * a.iters], "seconds": [ts1, ts3],
                   "us_per_restart_iteration": round((med3 - med1) / (a.batch * 2 * a.iters) * 1e6, 1),
                   "us_per_restart_iteration_whole_call": round(med3 / (a.batch * 3 * a.iters) * 1e6, 1)}
            print(json.dumps(row), flush=True)
            out["mu_batch"].append(row)
    rs = np.random.RandomState(3)
    eng.set_matrix(X)
    for k in (64, 128):
        H = np.abs(rs.standard_normal((k, X.shape[1]))) + 0.01
        kw = dict(tol=0, warn=False)
        eng.mu_refit_f64(H, max_iter=1, **kw)
        # two lengths: the difference leaves out what a call pays once (staging H, the first and last divergence, W back)
        med1, ts1 = median_of(lambda: eng.mu_refit_f64(H, max_iter=a.refit_iters, **kw), a.repeats)
        med3, ts3 = median_of(lambda: eng.mu_refit_f64(H, max_iter=3 * a.refit_iters, **kw), a.repeats)
        row = {"loss": "kullback-leibler", "k": k, "iterations": [a.refit_iters, 3 * a.refit_iters], "seconds": [ts1, ts3],
               "ms_per_iteration": round((med3 - med1) / (2 * a.refit_iters) * 1e3, 2)}
        print(json.dumps(row), flush=True)
        out["mu_refit_f64"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as F:
        json.dump(out, F, indent=1)
        F.write("\n")


if __name__ == "__main__":
    main()
