"""Kullback-Leibler on the non-zeros at ranks 33..64 (Engine.mu_sparse_rank_limit = 64) against the dense matrix-pipe
kernels (CNMF_MU_SPARSE=0) in the same run, at 50000 x 2000: time per restart-iteration of a batch of 32 restarts at ranks
40 / 48 / 64, on topic counts of library size e^5.2 (about 9 % non-zero, a real count matrix's density) and e^6.8 (the
benchmark's density, above a quarter: the non-zero route forced).  Every timed call ends in a device synchronise (the
results come back to the host); a warm-up call first (it also builds the images: its time is recorded), then the median of
--repeats at two call lengths, so that what a call pays once cancels.  Writes one JSON file.

    python tools/mu_sparse_ranks_probe.py --out profiles/mu_sparse_ranks_33_64_50000x2000.json
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
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ranks", type=int, nargs="+", default=[40, 48, 64])
    ap.add_argument("--lib-sizes", type=float, nargs="+", default=[5.2, 6.8])
    a = ap.parse_args()
    out = {"shape": [a.cells, a.genes], "batch": a.batch, "iterations": a.iters, "repeats": a.repeats, "rows": []}
    eng = Engine(0, mu_sparse_rank_limit=64)
    seeds = list(range(7, 7 + a.batch))
    for mu_lib in a.lib_sizes:
        C, _ = synth.topic_counts(a.cells, a.genes, 20, mu_lib, 0.4, 3)
        X = synth.normalise_like_prepare(C, dtype=np.float32)
        density = float((X != 0).mean())
        del C
        for k in a.ranks:
            row = {"log_library_size": mu_lib, "shape": list(X.shape), "density": round(density, 4), "k": k,
                   "iterations": [a.iters, 3 * a.iters]}
            for route, env in (("non_zero", "1"), ("dense", "0")):
                os.environ["CNMF_MU_SPARSE"] = env              # (the engine re-reads its switches when they change)
                eng.set_matrix(X)                               # drops every image: the warm-up call builds this route's
                kw = dict(seeds=seeds, beta_loss="kullback-leibler", tol=0, warn=False)
                t = time.perf_counter()
                eng.nmf_mu_batch([k] * a.batch, max_iter=2, **kw)
                first = time.perf_counter() - t
                t = time.perf_counter()
                eng.nmf_mu_batch([k] * a.batch, max_iter=2, **kw)
                second = time.perf_counter() - t
                im = eng.matrix_images()
                assert im["non_zero_images_64"] == (route == "non_zero"), (route, im)
                med1, ts1 = median_of(lambda: eng.nmf_mu_batch([k] * a.batch, max_iter=a.iters, **kw), a.repeats)
                med3, ts3 = median_of(lambda: eng.nmf_mu_batch([k] * a.batch, max_iter=3 * a.iters, **kw), a.repeats)
                row[route] = {"seconds": [ts1, ts3],
                              "us_per_restart_iteration": round((med3 - med1) / (a.batch * 2 * a.iters) * 1e6, 1),
                              "us_per_restart_iteration_whole_call": round(med3 / (a.batch * 3 * a.iters) * 1e6, 1),
                              # the first call of a matrix builds the images (or the transposed copy) of its route
                              "image_build_seconds": round(first - second, 3)}
            row["dense_over_non_zero"] = round(row["dense"]["us_per_restart_iteration"] / row["non_zero"]["us_per_restart_iteration"], 2)
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as F:
        json.dump(out, F, indent=1)
        F.write("\n")


if __name__ == "__main__":
    main()
