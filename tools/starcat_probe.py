"""Time the projection refit of StarCAT at an atlas-like shape (default 50 000 cells x 2 000 genes, k = 9): the
multiplicative Frobenius refit ``Engine.mu_frobenius_refit`` (cnmf_mu2_refit_f64) beside the coordinate-descent Frobenius
refit ``Engine.nnls_f64`` on the SAME resident matrix and spectra, each call host-timed end to end (upload of H, the
product X.H^T, the iterations, the fetch of W), --repeats times.  The two solve the same least-squares problem by different
iterations and stop by different rules: the iteration counts are reported beside the times, and no speed is claimed.

Usage:  python tools/starcat_probe.py [--cells 50000] [--genes 2000] [--k 9] [--repeats 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import synth  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C, Hgt = synth.topic_counts(a.cells, a.genes, a.k, seed=2)
    X = synth.normalise_like_prepare(C, dtype=np.float64)
    keep = C.sum(axis=0) > 0
    H = np.ascontiguousarray(Hgt[:, keep] * 1e3 + 1e-3)
    res = dict(shape=[int(X.shape[0]), int(X.shape[1])], k=a.k, repeats=a.repeats, mu_frobenius_refit=[], nnls_f64=[])
    with Engine(0) as eng:
        eng.set_matrix(X)
        eng.nnls_f64(H, max_iter=2, warn=False)                    # (first touch of the device and of the dense image)
        for _ in range(a.repeats):
            t = time.perf_counter()
            W, n, err = eng.mu_frobenius_refit(H, warn=False)
            res["mu_frobenius_refit"].append(dict(seconds=time.perf_counter() - t, n_iter=n, err=err))
            t = time.perf_counter()
            V, m = eng.nnls_f64(H, warn=False)
            res["nnls_f64"].append(dict(seconds=time.perf_counter() - t, n_iter=m))
        res["residual_mu"] = float(np.linalg.norm(X - W @ H))
        res["residual_cd"] = float(np.linalg.norm(X - V @ H))
    for key in ("mu_frobenius_refit", "nnls_f64"):
        best = min(res[key], key=lambda r: r["seconds"])
        res[key + "_best"] = dict(best, ms_per_iteration=1e3 * best["seconds"] / max(best["n_iter"], 1))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
