"""Time the consensus clustergram on the C5 stress input (``synth.consensus_stress``: 5 000 spectra x 2 000 genes, k = 20,
100 outliers): the device call beside the host route it replaces, on the same box, --repeats times after one warm-up.

  device   ``Engine.clustergram`` as a whole (host clock around the call: upload of the spectra, kernels, download of the
           order and of the R_kept x R_kept image) and its steps by HIP events (``Engine.clustergram_step_ms``); also the
           call without the image, which is what only the ordering costs.
  host     what a caller has to do without it: ``Engine.consensus(return_dist=True)``'s fetch of the whole R x R matrix
           (timed as the difference to the same call without the fetch), the density filter ``D[keep][:, keep]``, scipy
           ``linkage(squareform(block), 'average')`` + ``leaves_list`` per cluster, and the two permutations
           ``D[order][:, order]``.

The consensus core (density, k-means) runs once before either side and is not part of either time; both sides start from
its labels.  The orders of the two routes are compared (they are equal unless merge heights tie).

Usage:  python tools/consensus_clustergram_probe.py [--repeats 5] [--out profiles/consensus_clustergram_5000x2000.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_amd import synth  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402

KERNEL_SOURCES = ["cnmf_amd/csrc/linkage_host.hip.h", "cnmf_amd/csrc/kernels_consensus.hip.h",
                  "cnmf_amd/csrc/consensus_host.hip.h"]


def stamp():
    try:
        head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, capture_output=True, text=True,
                              check=True).stdout.strip()
        if subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, capture_output=True, text=True).stdout.strip():
            head += "+uncommitted changes"
    except (OSError, subprocess.CalledProcessError):
        head = "unknown (no git metadata beside the sources)"
    sha = {f: hashlib.sha256(open(os.path.join(ROOT, f), "rb").read()).hexdigest()[:16] for f in KERNEL_SOURCES}
    return dict(git_head=head, kernel_source_sha256=sha)


def summary(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], all=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=5000)
    ap.add_argument("--G", type=int, default=2000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--outliers", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy.cluster.hierarchy import leaves_list, linkage
    from scipy.spatial.distance import squareform
    S, _ = synth.consensus_stress(R=a.R, G=a.G, k=a.k, n_outliers=a.outliers, seed=0)
    res = dict(shape=[a.R, a.G], k=a.k, n_outliers=a.outliers, repeats=a.repeats, unit="milliseconds")
    ms = lambda t0: 1e3 * (time.perf_counter() - t0)      # noqa: E731

    with Engine(0) as eng:
        core = eng.consensus(S, a.k)                       # (first touch of the device; the labels both sides start from)
        labels, keep = core["labels"], core["density_filter"]
        kept_labels = labels[keep]
        res["n_kept"] = int(keep.sum())
        res["cluster_sizes"] = np.bincount(kept_labels, minlength=a.k).tolist()

        # ---- device
        dev = eng.clustergram(S, labels, a.k)              # warm-up (workspace, code objects)
        whole, order_only, steps = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            dev = eng.clustergram(S, labels, a.k)
            whole.append(ms(t0))
            steps.append(eng.clustergram_step_ms())
            t0 = time.perf_counter()
            eng.clustergram(S, labels, a.k, return_image=False)
            order_only.append(ms(t0))
        res["device"] = dict(whole_call=summary(whole), without_image=summary(order_only),
                             steps_hip_events={key: summary([s[key] for s in steps]) for key in steps[0]})

        # ---- host route
        eng.consensus(S, a.k, return_dist=True)            # warm-up
        t_fetch, t_filter, t_linkage, t_permute, t_core = [], [], [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            eng.consensus(S, a.k)
            plain = ms(t0)
            t0 = time.perf_counter()
            full = eng.consensus(S, a.k, return_dist=True)
            t_core.append(plain)
            t_fetch.append(ms(t0) - plain)
            t0 = time.perf_counter()
            D = full["topics_dist"][keep, :][:, keep]
            t_filter.append(ms(t0))
            t0 = time.perf_counter()
            order = []
            for c in range(a.k):
                members = np.where(kept_labels == c)[0]
                if len(members) > 1:
                    cl = squareform(D[members, :][:, members], checks=False)
                    cl[cl < 0] = 0
                    members = members[leaves_list(linkage(cl, "average"))]
                order += members.tolist()
            t_linkage.append(ms(t0))
            t0 = time.perf_counter()
            image = D[order, :][:, order]
            t_permute.append(ms(t0))
        total = [f + g + h + p for f, g, h, p in zip(t_fetch, t_filter, t_linkage, t_permute)]
        res["host_route"] = dict(total=summary(total), fetch_of_the_full_matrix=summary(t_fetch),
                                 density_filter=summary(t_filter), scipy_linkage_per_cluster=summary(t_linkage),
                                 two_permutations=summary(t_permute), consensus_core_for_scale=summary(t_core))
        res["orders_equal"] = bool(np.array_equal(dev["spectra_order"], np.asarray(order)))
        res["largest_image_difference"] = float(np.abs(dev["topics_dist_ordered"] - image).max())
    res["host_over_device"] = res["host_route"]["total"]["median"] / res["device"]["whole_call"]["median"]
    res["_source"] = "tools/consensus_clustergram_probe.py (defaults), one run on one MI355X"
    res.update(stamp())
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
