"""Time the device steps of Preprocess.normalize_batchcorrect (Harmony branch) at an atlas-like shape (default 50 000
cells x 2 000 HVGs of synth.sparse_counts-like counts, K = 100 Harmony clusters, 4 batches -> K (B + 1) = 500), and
the host work they replace on the same machine:

  device   upload of the counts, the two selections (normalised / raw) with their quantile ceilings (order statistics +
           clamp), densify, column means + covariance, host eigh, scores, ridge moments, host solves, ridge apply,
           fetch -- each step timed with a synchronising call around it
  host     np.quantile over all N G entries (the reference's ceiling) and the reference's moe_correct_ridge loop restated
           in numpy; the loop is timed over its first --host-clusters clusters and scaled to K (each pass costs the
           same), which the JSON says

Usage:  python tools/preprocess_probe.py [--cells 50000] [--genes 2000] [--K 100] [--batches 4] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import preprocess as pp  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402


def make_inputs(N, G, K, nb, seed=0):
    rs = np.random.RandomState(seed)
    lib = rs.lognormal(0.0, 0.5, size=(N, 1))
    lam = rs.gamma(0.3, 1.0, size=(1, G))
    C = sp.csr_matrix(rs.poisson(lib * lam).astype(np.float64))
    batch = rs.randint(0, nb, size=N)
    Phi = np.vstack([np.ones(N)] + [(batch == b).astype(np.float64) for b in range(nb)])
    logits = rs.randn(K, N) * 2
    R = np.exp(logits - logits.max(axis=0))
    R /= R.sum(axis=0)
    lamb = np.diag(np.r_[0.0, np.ones(nb)])
    return C, Phi, R, lamb


def device_steps(eng, C, Phi, R, lamb, q=.9999):
    N, G = C.shape
    sel = np.arange(G)
    t, names = [time.perf_counter()], []

    def mark(name):
        t.append(time.perf_counter())
        names.append(name)

    eng.preprocess_upload(C); mark("upload_counts")
    eng.preprocess_select(0, sel, 1e4, None); mark("select_normalised")
    pp._ceiling(eng, 0, N, G, q); mark("ceiling_normalised")
    eng.preprocess_select(1, sel, 0.0, None); mark("select_raw")
    pp._ceiling(eng, 1, N, G, q); mark("ceiling_raw")
    eng.preprocess_densify(0); eng.preprocess_densify(1); mark("densify_both")
    mean, S = eng.preprocess_scatter(0); mark("means_covariance")
    w, V = np.linalg.eigh(S / (N - 1)); V = V[:, np.argsort(-w, kind="stable")[:50]]; mark("host_eigh")
    eng.preprocess_project(0, mean, V); mark("pca_scores")
    M, gram = eng.preprocess_ridge_moments(1, R, Phi); mark("ridge_moments")
    W = np.empty_like(M)
    for k in range(R.shape[0]):
        W[k] = np.linalg.inv(gram[k] + lamb) @ M[k]
        W[k][0, :] = 0
    mark("host_solves")
    eng.preprocess_ridge_apply(1, W); mark("ridge_apply")
    X = eng.preprocess_fetch(1); mark("fetch_corrected")
    eng.preprocess_release()
    return {n: round(1e3 * (b - a), 3) for n, a, b in zip(names, t[:-1], t[1:])}, X


def host_steps(C, Phi, R, lamb, n_clusters, q=.9999):
    D = C.toarray()
    t0 = time.perf_counter()
    np.quantile(D.reshape(-1), q)
    t1 = time.perf_counter()
    Z_orig = D.T
    Z_corr = Z_orig.copy()
    for i in range(n_clusters):                           # preprocess.py:9-18, as written
        Phi_Rk = np.multiply(Phi, R[i, :])
        x = np.dot(Phi_Rk, Phi.T) + lamb
        W = np.dot(np.dot(np.linalg.inv(x), Phi_Rk), Z_orig.T)
        W[0, :] = 0
        Z_corr -= np.dot(W.T, Phi_Rk)
    t2 = time.perf_counter()
    return {"np_quantile_ms": round(1e3 * (t1 - t0), 1), "ridge_loop_clusters_timed": n_clusters,
            "ridge_loop_ms_timed": round(1e3 * (t2 - t1), 1),
            "ridge_loop_ms_scaled_to_K": round(1e3 * (t2 - t1) * R.shape[0] / n_clusters, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--host-clusters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C, Phi, R, lamb = make_inputs(a.cells, a.genes, a.K, a.batches)
    out = {"cells": a.cells, "genes": a.genes, "K": a.K, "B_plus_1": a.batches + 1,
           "density": round(C.nnz / (a.cells * a.genes), 4), "device_ms": []}
    with Engine(0) as eng:
        device_steps(eng, C, Phi, R, lamb)                # warm-up (code objects, allocations)
        for _ in range(a.repeats):
            d, _ = device_steps(eng, C, Phi, R, lamb)
            out["device_ms"].append(d)
    best = {k: min(r[k] for r in out["device_ms"]) for k in out["device_ms"][0]}
    out["device_ms_best"] = best
    out["device_ms_best_total"] = round(sum(best.values()), 3)
    out["device_ms_best_without_transfers_and_host"] = round(sum(
        v for k, v in best.items() if k not in ("upload_counts", "fetch_corrected", "host_eigh", "host_solves")), 3)
    out["host"] = host_steps(C, Phi, R, lamb, a.host_clusters)
    out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as F:
            json.dump(out, F, indent=1)


if __name__ == "__main__":
    main()
