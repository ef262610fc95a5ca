"""Time cNMF.prepare at an atlas-like shape (default 50 000 cells x 20 000 genes, ~7 % non-zero, synth.sparse_counts):

  device   the engine's steps one by one: upload of the staged counts, TPM + gene statistics, HVG model (host),
           column subset + scaling (+ fetch of the float64 result)
  prepare  the whole cNMF.prepare() call (sparse branch, num_highvar_genes=2000), artefact writes included, and where
           its time goes (cNMF.last_prepare_seconds: inputs + upload, device TPM statistics, HVG model, device
           selection + fetch, host frames, file writes + ledger)
  host     the same steps restated on the host through oracle/scanpy_shim.py (normalize_total, StandardScaler's
           mean / variance as get_mean_var, the HVG model, the column subset, scale) -- what the reference's
           prepare spends before it writes a file

Usage:  python tools/prepare_probe.py [--cells 50000] [--genes 20000] [--density 0.07] [--out FILE.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import synth  # noqa: E402
from cnmf_amd.cnmf import cNMF, select_highvar_genes  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402


def device_steps(eng, M, n_hvg):
    t = [time.perf_counter()]
    eng.prepare_upload(M)
    t.append(time.perf_counter())
    _, mean, var, tpm = eng.prepare_tpm_stats(1e6, want_tpm=True)
    t.append(time.perf_counter())
    mask, _ = select_highvar_genes(mean, var, numgenes=n_hvg)
    t.append(time.perf_counter())
    eng.prepare_select(np.flatnonzero(mask), densify=False)
    t.append(time.perf_counter())
    return dict(upload=t[1] - t[0], tpm_stats=t[2] - t[1], hvg_model=t[3] - t[2], select_scale_fetch=t[4] - t[3],
                total=t[4] - t[0]), mask


def host_steps(M, n_hvg):
    from oracle import scanpy_shim as shim
    from sklearn.preprocessing import StandardScaler
    t = [time.perf_counter()]
    ad = shim.AnnData(M.astype(np.float64))
    shim._normalize_total(ad, target_sum=1e6)
    t.append(time.perf_counter())
    sc = StandardScaler(with_mean=False).fit(ad.X)
    mean, var = sc.mean_, sc.var_
    t.append(time.perf_counter())
    mask, _ = select_highvar_genes(mean, var, numgenes=n_hvg)
    t.append(time.perf_counter())
    sub = shim.AnnData(M[:, np.flatnonzero(mask)].astype(np.float64))
    t.append(time.perf_counter())
    shim._scale(sub, zero_center=False)
    t.append(time.perf_counter())
    return dict(normalize_total=t[1] - t[0], tpm_stats=t[2] - t[1], hvg_model=t[3] - t[2], column_subset=t[4] - t[3],
                scale=t[5] - t[4], total=t[5] - t[0]), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--density", type=float, default=0.07)
    ap.add_argument("--hvg", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M = synth.sparse_counts(a.cells, a.genes, density=a.density, seed=1)
    res = dict(shape=[a.cells, a.genes], nnz=int(M.nnz), density=M.nnz / float(a.cells * a.genes), hvg=a.hvg)
    cells = ["c%d" % i for i in range(a.cells)]
    genes = ["g%d" % j for j in range(a.genes)]
    with Engine(0) as eng:
        device_steps(eng, M, a.hvg)                                   # warm-up: code objects, allocations
        dev = []
        for _ in range(a.reps):
            d, mask_d = device_steps(eng, M, a.hvg)
            dev.append(d)
        res["device"] = {k: min(d[k] for d in dev) for k in dev[0]}
        tmp = tempfile.mkdtemp(prefix="cnmf_prep_probe_")
        obj = cNMF(output_dir=tmp, name="p", engine=eng)
        calls, steps = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            obj.prepare((M, cells, genes), components=[5, 7], n_iter=10, seed=14, num_highvar_genes=a.hvg)
            calls.append(time.perf_counter() - t0)
            steps.append(obj.last_prepare_seconds)
        res["prepare_seconds"] = calls
        res["prepare_steps"] = {k: min(d[k] for d in steps) for k in steps[0]}       # (cNMF.last_prepare_seconds)
        shutil.rmtree(tmp, ignore_errors=True)
    host, mask_h = host_steps(M, a.hvg)
    res["host_shim"] = host
    res["hvg_lists_equal"] = bool(np.array_equal(mask_h, mask_d))
    res["speedup_prepare_vs_host_steps"] = host["total"] / min(calls)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as F:
            json.dump(res, F, indent=1)


if __name__ == "__main__":
    main()
