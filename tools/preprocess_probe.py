"""Time the device steps of Preprocess.normalize_batchcorrect (Harmony branch) at an atlas-like shape (default 50 000
cells x 2 000 HVGs of synth.sparse_counts-like counts, K = 100 Harmony clusters, 4 batches -> K (B + 1) = 500), and
the host work they replace on the same machine:

  device   upload of the counts, the two selections (normalised / raw) with their quantile ceilings (order statistics +
           clamp), densify, column means + covariance, host eigh, scores, ridge moments, host solves, ridge apply,
           fetch -- each step timed with a synchronising call around it
  host     np.quantile over all N G entries (the reference's ceiling) and the reference's moe_correct_ridge loop restated
           in numpy; the loop is timed over its first --host-clusters clusters and scaled to K (each pass costs the
           same), which the JSON says

``--filter`` times the entry points instead: Preprocess.filter_adata followed by Preprocess.preprocess_for_cnmf without
Harmony (2 000 random HVGs) on raw counts of --filter-cells x --filter-genes (default 50 000 x 20 000, about 6.7 %
non-zero, CSR input), end to end as a user calls them (uploads and fetches included), and the same steps written with
scipy / numpy on the same machine (detection counts, sums, the two subsets, normalize_total, the HVG subset, the
ddof=1 scaling and the quantile ceiling over the dense N x HVG matrix).

``--harmony`` times Preprocess.run_harmony (the clustering loop on the device) on --cells x --components synthetic PCA
scores with one batch variable of --batches levels and --K clusters: the k-means initialisation is timed on its own both
ways in the same run -- scikit-learn on the host, and Engine.harmony_kmeans_init on the device (best of --repeats, after
harmony_begin) -- and the device loop after each (best of --repeats, the centroids handed over as init_centroids);
then the whole device route (run_harmony(kmeans_init="device")), and the loop from scikit-learn's centroids through the
numpy restatement tests/_harmony_ref.py on this machine's cores.

``--hvg`` times Preprocess.highly_variable_genes (seurat_v3) on the raw counts of ``--filter`` (default 50 000 x 20 000,
about 6.7 % non-zero, 2 000 genes selected): the whole call with both loess surfaces (upload included, best of
--repeats), its three device steps on their own (the integer moments, the local fits at the vertices and at every gene,
the clipped sums), and the numpy restatement tests/_seurat_v3_ref.py on this machine's cores.

``--pca`` times the PCA of the Harmony branch three ways on one staged slot of --cells x --genes (the normalised,
scaled and ceilinged counts of the default leg), the median of --repeats, every step between two synchronising calls:
``pca="device"`` (scatter + Householder tridiagonalisation on the device; ``tridiagonal_top`` on the host;
back-transformation + sign rule + scores on the device), ``pca="device_full"`` (``preprocess_pca_device``: one call,
its device steps -- bounds, bisection, inverse iteration, orthogonalisation + check, back-transformation + scores -- by
HIP events; the same (d, e) through ``tridiagonal_eigh_top`` and ``tridiagonal_top`` alone beside it) and
``pca="lapack"`` (scatter + fetch; ``np.linalg.eigh`` on this machine's cores; upload + scores), the contracts of
tests/_tridiag_ref.py for the device's eigenpairs at that size, and writes
profiles/preprocess_probe_pca_full_<N>x<G>.json unless --out says otherwise (profiles/preprocess_probe_pca_<N>x<G>.json
is the two-arm run from before the third arm).

Usage:  python tools/preprocess_probe.py --pca [--cells 50000] [--genes 2000] --repeats 5 [--out FILE.json]
        python tools/preprocess_probe.py [--cells 50000] [--genes 2000] [--K 100] [--batches 4] [--out FILE.json]
        python tools/preprocess_probe.py --filter [--filter-cells 50000] [--filter-genes 20000] [--out FILE.json]
        python tools/preprocess_probe.py --harmony [--cells 50000] [--components 50] [--K 100] [--batches 4] [--out FILE.json]
        python tools/preprocess_probe.py --hvg [--filter-cells 50000] [--filter-genes 20000] [--out FILE.json]
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


# ---------------------------------------------------------------- the entry points: filter_adata + preprocess_for_cnmf
def make_raw_counts(N, G, density=0.067, seed=0, rows_per_chunk=2000):
    """CSR counts with gene-specific detection rates averaging ``density``, built a block of rows at a time"""
    rs = np.random.RandomState(seed)
    p = rs.gamma(0.5, 1.0, size=G)
    p = np.minimum(p * density / p.mean(), 0.9)
    blocks = []
    for r0 in range(0, N, rows_per_chunk):
        n = min(rows_per_chunk, N - r0)
        B = sp.csr_matrix(rs.random_sample((n, G)) < p, dtype=np.float64)
        B.data = 1.0 + rs.poisson(1.5, size=B.nnz)
        blocks.append(B)
    X = sp.vstack(blocks, format="csr")
    genes = np.array(["g%d" % j for j in range(G)], dtype=object)
    genes[:13] = ["MT-%d" % j for j in range(13)]
    genes[13:113] = ["AC%d.1" % j for j in range(100)]
    return X, ["c%d" % i for i in range(N)], list(genes)


FILTER_ARGS = dict(min_cells_per_gene=10, min_counts_per_cell=500, filter_mito_thresh=0.2)
N_HVG = 2000


def hvg_choice(n_genes, seed=1):
    mask = np.zeros(n_genes, dtype=bool)
    mask[np.random.RandomState(seed).choice(n_genes, min(N_HVG, n_genes), replace=False)] = True
    return mask


def device_route(P, X, cells, genes):
    t0 = time.perf_counter()
    flt = P.filter_adata((X, cells, genes), makeplots=False, **FILTER_ARGS)
    t1 = time.perf_counter()
    hv = hvg_choice(flt.X.shape[1])
    res, tp, hvgs = P.preprocess_for_cnmf((flt.X, flt.obs_names, flt.var_names), obs=flt.obs, highly_variable=hv,
                                          makeplots=False)
    t2 = time.perf_counter()
    return {"filter_adata_ms": round(1e3 * (t1 - t0), 1), "preprocess_for_cnmf_ms": round(1e3 * (t2 - t1), 1),
            "total_ms": round(1e3 * (t2 - t0), 1)}, (flt, res, tp)


def scipy_route(X, genes):
    genes = np.asarray(genes)
    t0 = time.perf_counter()
    n_cells = np.asarray((X > 0).sum(axis=0)).ravel()
    Xg = X[:, np.flatnonzero(n_cells >= FILTER_ARGS["min_cells_per_gene"])]
    g1 = genes[n_cells >= FILTER_ARGS["min_cells_per_gene"]]
    n_counts = np.asarray(Xg.sum(axis=1)).ravel()
    keep = n_counts >= FILTER_ARGS["min_counts_per_cell"]
    Xc, n_counts = Xg[np.flatnonzero(keep)], n_counts[keep]
    mt = np.array(["MT-" in x for x in g1])
    pct = np.asarray(Xc[:, np.flatnonzero(mt)].sum(axis=1)).ravel() / n_counts
    Xc = Xc[np.flatnonzero(pct < FILTER_ARGS["filter_mito_thresh"])]
    dot = np.array(["." in x for x in g1])
    Xf = Xc[:, np.flatnonzero(~dot)]
    t1 = time.perf_counter()
    hv = hvg_choice(Xf.shape[1])
    rs = np.asarray(Xf.sum(axis=1)).ravel()
    tp = sp.csr_matrix(Xf, dtype=np.float64, copy=True)
    tp.data *= np.repeat(np.where(rs > 0, 1e4 / np.where(rs > 0, rs, 1.0), 0.0), np.diff(tp.indptr))
    H = Xf[:, np.flatnonzero(hv)]
    D = H.toarray()
    std = D.std(axis=0, ddof=1)
    std[std == 0] = 1.0
    H.data = H.data / std[H.indices]
    thresh = np.quantile((D / std).reshape(-1), .9999)
    H.data[H.data > thresh] = thresh
    t2 = time.perf_counter()
    return {"filter_adata_ms": round(1e3 * (t1 - t0), 1), "preprocess_for_cnmf_ms": round(1e3 * (t2 - t1), 1),
            "total_ms": round(1e3 * (t2 - t0), 1)}, (Xf, H, tp)


def filter_leg(a):
    X, cells, genes = make_raw_counts(a.filter_cells, a.filter_genes)
    out = {"cells": a.filter_cells, "genes": a.filter_genes, "density": round(X.nnz / (X.shape[0] * X.shape[1]), 4),
           "filter_args": FILTER_ARGS, "n_hvg": N_HVG, "device": [], "host_threads": os.environ.get("OMP_NUM_THREADS")}
    with Engine(0) as eng:
        P = pp.Preprocess(engine=eng)
        small = make_raw_counts(2000, 500, density=0.3, seed=3)
        P.filter_adata(small, makeplots=False, min_cells_per_gene=1, min_counts_per_cell=1)     # warm-up (code objects)
        for _ in range(a.repeats):
            d, (flt, res, tp) = device_route(P, X, cells, genes)
            out["device"].append(d)
    out["device_best"] = min(out["device"], key=lambda r: r["total_ms"])
    out["scipy"], (Xf, H, tp_h) = scipy_route(X, genes)
    out["filtered_shape"] = list(flt.X.shape)
    Xf.sort_indices()
    out["same_filtered_counts"] = bool(flt.X.shape == Xf.shape and (flt.X != Xf).nnz == 0)
    out["same_tp10k_bits"] = bool(np.array_equal(tp.X.data.view(np.uint64), tp_h.data.view(np.uint64)))
    out["speedup_end_to_end"] = round(out["scipy"]["total_ms"] / out["device_best"]["total_ms"], 2)
    return out


def harmony_leg(a):
    from tests import _harmony_ref as ref
    N, d, K = a.cells, a.components, a.K
    pca, obs = ref.make_case(N, d, [a.batches], seed=0)
    hvars = list(obs.columns)
    out = {"cells": N, "components": d, "K": K, "batches": a.batches, "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "device_s": []}
    Z = pca.T
    Z_cos = Z / Z.max(axis=0)
    Z_cos = Z_cos / np.sqrt((Z_cos * Z_cos).sum(axis=0))
    t0 = time.perf_counter()
    Y0 = pp._host_kmeans_centroids(Z_cos, K, 0)
    out["host_kmeans_init_s"] = round(time.perf_counter() - t0, 3)
    with Engine(0) as eng:
        P = pp.Preprocess(engine=eng)
        small = ref.make_case(500, 8, [2], seed=1)
        P.run_harmony(small[0], small[1], ["var0"], max_iter_harmony=1)              # warm-up (code objects)
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = P.run_harmony(pca, obs, hvars, nclust=K, init_centroids=Y0)
            out["device_s"].append(round(time.perf_counter() - t0, 3))
        # the initialisation on the device: alone (after harmony_begin), then the loop from its centroids, then the whole route
        Phi, codes, level_var, n_levels = pp.harmony_design(obs, hvars)
        out["device_kmeans_init_s"], out["device_s_after_device_init"], out["device_full_route_s"] = [], [], []
        for _ in range(a.repeats):
            eng.harmony_begin(pca, codes, level_var, np.ones(Phi.shape[0]), np.repeat(0.1, K), Phi.sum(axis=1) / N)
            try:
                t0 = time.perf_counter()
                Yd, _, inertia, n_iter, best_init = eng.harmony_kmeans_init(0)
                out["device_kmeans_init_s"].append(round(time.perf_counter() - t0, 4))
            finally:
                eng.harmony_release()
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got_d = P.run_harmony(pca, obs, hvars, nclust=K, init_centroids=Yd)
            out["device_s_after_device_init"].append(round(time.perf_counter() - t0, 3))
            t0 = time.perf_counter()
            full = P.run_harmony(pca, obs, hvars, nclust=K, kmeans_init="device")
            out["device_full_route_s"].append(round(time.perf_counter() - t0, 3))
        out["device_full_route_equals_init_centroids_run"] = bool(np.array_equal(full.Z_corr, got_d.Z_corr))
    init_d = min(out["device_kmeans_init_s"])
    out.update({"device_kmeans_init_s_best": init_d, "device_kmeans_n_iter": [int(x) for x in n_iter],
                "device_kmeans_best_init": int(best_init), "device_kmeans_inertia": float(inertia[best_init]),
                "host_over_device_kmeans_init": round(out["host_kmeans_init_s"] / init_d, 1),
                "kmeans_rounds_after_device_init": [int(r) for r in got_d.kmeans_rounds],
                "device_s_after_device_init_best": min(out["device_s_after_device_init"]),
                "device_full_route_s_best": min(out["device_full_route_s"]),
                "device_kmeans_init_share_of_full_route": round(init_d / min(out["device_full_route_s"]), 3),
                "max_abs_diff_Y_host_vs_device_init": float(np.max(np.abs(Y0 - Yd)))})
    best = min(out["device_s"])
    iters = sum(r + 1 for r in got.kmeans_rounds)
    out.update({"harmony_rounds": len(got.kmeans_rounds), "kmeans_rounds": [int(r) for r in got.kmeans_rounds],
                "kmeans_iterations": iters, "device_s_best": best,
                "device_s_per_harmony_round": round(best / max(len(got.kmeans_rounds), 1), 4),
                "device_ms_per_kmeans_iteration": round(1e3 * best / max(iters, 1), 3),
                "host_kmeans_init_share_of_total": round(out["host_kmeans_init_s"] / (out["host_kmeans_init_s"] + best), 3)})
    t0 = time.perf_counter()
    h = ref.run_harmony(pca, obs, hvars, nclust=K, init_centroids=Y0)
    out["numpy_restatement_s"] = round(time.perf_counter() - t0, 3)
    out["same_rounds_as_restatement"] = bool(h.kmeans_rounds == got.kmeans_rounds)
    if out["same_rounds_as_restatement"]:
        out["max_abs_diff_R"] = float(np.max(np.abs(h.R - got.R)))
        out["max_abs_diff_Z_corr"] = float(np.max(np.abs(h.Z_corr - got.Z_corr)))
    out["restatement_over_device_loop"] = round(out["numpy_restatement_s"] / best, 2)
    return out


def hvg_leg(a):
    from tests import _seurat_v3_ref as ref
    X, cells, genes = make_raw_counts(a.filter_cells, a.filter_genes)
    N, G = X.shape
    out = {"cells": N, "genes": G, "density": round(X.nnz / (N * G), 4), "n_top_genes": N_HVG, "span": 0.3,
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "device_call_s": {}, "device_steps_ms": [], "restatement_s": {}}
    frames = {}
    with Engine(0) as eng:
        P = pp.Preprocess(engine=eng)
        small = make_raw_counts(2000, 500, density=0.3, seed=3)
        P.highly_variable_genes(small, n_top_genes=50)                              # warm-up (code objects)
        for surface in pp.LOESS_SURFACES:
            out["device_call_s"][surface] = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                frames[surface] = P.highly_variable_genes((X, cells, genes), n_top_genes=N_HVG, surface=surface)
                out["device_call_s"][surface].append(round(time.perf_counter() - t0, 3))
        for _ in range(a.repeats):
            t, names = [time.perf_counter()], []

            def mark(name):
                t.append(time.perf_counter())
                names.append(name)

            eng.preprocess_upload(X); mark("upload_counts")
            s1, s2, _ = eng.preprocess_gene_moments(); mark("gene_moments")
            mean, var = pp.exact_mean_var(s1, s2, N)
            nc = var > 0
            x, y = np.log10(mean[nc]), np.log10(var[nc])
            order = np.argsort(x, kind="stable")
            xs, ys = x[order], y[order]
            v = pp.loess_vertices(xs, 0.3)
            q = pp.loess_neighbours(xs.size, 0.3); mark("host_mean_var_sort_vertices")
            eng.preprocess_loess_fit(xs, ys, q, v); mark("loess_fit_vertices")
            _, _, status = eng.preprocess_loess_fit(xs, ys, q, xs); mark("loess_fit_every_gene")
            clip = np.sqrt(10 ** np.zeros(G)) * np.sqrt(np.float64(N)) + mean
            eng.preprocess_clipped_sums(clip); mark("clipped_sums")
            eng.preprocess_release()
            out["device_steps_ms"].append({n: round(1e3 * (b - c), 3) for n, c, b in zip(names, t[:-1], t[1:])})
        out.update({"loess_points": int(xs.size), "loess_q": int(q), "loess_vertices": int(v.size),
                    "loess_fits_flagged_for_the_host": int((status != 0).sum())})
    out["device_call_s_best"] = {k: min(v) for k, v in out["device_call_s"].items()}
    out["device_steps_ms_best"] = {k: min(r[k] for r in out["device_steps_ms"]) for k in out["device_steps_ms"][0]}
    for surface in pp.LOESS_SURFACES:
        t0 = time.perf_counter()
        want = ref.seurat_v3(X, N_HVG, surface=surface, genes=genes)
        out["restatement_s"][surface] = round(time.perf_counter() - t0, 3)
        got = frames[surface]
        out["same_selected_set_" + surface] = bool(np.array_equal(got["highly_variable"].values, want["highly_variable"].values))
        out["max_rel_diff_variances_norm_" + surface] = float(np.max(
            np.abs(got["variances_norm"].values - want["variances_norm"].values) / np.maximum(want["variances_norm"].values, 1e-300)))
        out["restatement_over_device_" + surface] = round(out["restatement_s"][surface] / out["device_call_s_best"][surface], 2)
    out["selected_genes_that_differ_between_the_surfaces"] = int(
        (frames["interpolate"]["highly_variable"].values != frames["direct"]["highly_variable"].values).sum() // 2)
    return out


def pca_leg(a):
    """the PCA of normalize_batchcorrect's Harmony branch both ways on the same staged slot, every step between two
    synchronising calls, the median of --repeats"""
    from tests import _tridiag_ref as ref
    N, G = a.cells, a.genes
    C = make_inputs(N, G, 1, 1)[0]
    n_comps = pp._pca_components(N, G)
    steps = {"device": {"scatter_and_tridiagonalise_ms": [], "host_tridiagonal_solve_ms": [],
                        "back_transform_and_scores_ms": []},
             "device_full": {"one_call_ms": []},
             "lapack": {"scatter_and_fetch_ms": [], "host_eigh_ms": [], "upload_and_project_ms": []}}
    events = {k: [] for k in ("bounds_ms", "bisection_ms", "inverse_iteration_ms", "orthogonalisation_and_check_ms",
                              "back_transform_and_scores_ms")}
    solver_alone = {"device_tridiagonal_eigh_top_ms": [], "host_tridiagonal_top_ms": []}
    free = []
    with Engine(0) as eng:
        eng.symmetric_eigh_top(np.eye(8), 2)                         # warm-up (code objects), both solvers
        eng.symmetric_eigh_top(np.eye(8) + np.diag(np.ones(7), 1) + np.diag(np.ones(7), -1), 2, solver="device")
        eng.preprocess_upload(C)
        eng.preprocess_select(0, np.arange(G), 1e4, None)
        pp._ceiling(eng, 0, N, G, .9999)
        eng.preprocess_densify(0)
        eng.preprocess_scatter(0)
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            mean, d, e = eng.preprocess_pca_tridiag(0)
            t1 = time.perf_counter()
            w, Z = pp.tridiagonal_top(d, e, n_comps)
            t2 = time.perf_counter()
            Vd, scores_d = eng.preprocess_pca_finish(0, Z)
            t3 = time.perf_counter()
            for k, v in zip(steps["device"], (t1 - t0, t2 - t1, t3 - t2)):
                steps["device"][k].append(1e3 * v)
            # pca="device_full": one library call; its device steps by HIP events
            t0 = time.perf_counter()
            mean_f, w_f, Vf, scores_f = eng.preprocess_pca_device(0, n_comps)
            steps["device_full"]["one_call_ms"].append(1e3 * (time.perf_counter() - t0))
            solver_used, check_f = eng.last_tridiagonal_solver, eng.last_tridiagonal_check
            for k, v in zip(events, eng.tridiagonal_eigh_step_ms()):
                events[k].append(float(v))
            # the same (d, e) through both solvers alone (the device one with its transfers of d, e, w and Z)
            t0 = time.perf_counter()
            eng.tridiagonal_eigh_top(d, e, n_comps)
            t1 = time.perf_counter()
            pp.tridiagonal_top(d, e, n_comps)
            t2 = time.perf_counter()
            solver_alone["device_tridiagonal_eigh_top_ms"].append(1e3 * (t1 - t0))
            solver_alone["host_tridiagonal_top_ms"].append(1e3 * (t2 - t1))
            t0 = time.perf_counter()
            mean_l, S = eng.preprocess_scatter(0)
            t1 = time.perf_counter()
            lam, V = np.linalg.eigh(S / (N - 1))
            V = ref.sign_rule(V[:, np.argsort(-lam, kind="stable")[:n_comps]])
            t2 = time.perf_counter()
            scores_l = eng.preprocess_project(0, mean_l, V)
            t3 = time.perf_counter()
            for k, v in zip(steps["lapack"], (t1 - t0, t2 - t1, t3 - t2)):
                steps["lapack"][k].append(1e3 * v)
        eng.preprocess_release()
        for _ in range(a.repeats):                                   # the tridiagonalisation of a host matrix: upload + n launches
            t0 = time.perf_counter()
            eng.symmetric_tridiagonalize(S)
            free.append(1e3 * (time.perf_counter() - t0))
        eng.preprocess_release()
    out = {"cells": N, "genes": G, "n_comps": n_comps, "repeats": a.repeats, "host_threads": os.environ.get("OMP_NUM_THREADS"),
           "form": "one launch per column (deferred rank-2 update)"}
    for route, r in steps.items():
        out[route] = {k: round(float(np.median(v)), 3) for k, v in r.items()}
        out[route]["total_ms"] = round(sum(out[route].values()), 3)
        out[route + "_all_ms"] = {k: [round(x, 3) for x in v] for k, v in r.items()}
    out["upload_and_tridiagonalise_host_matrix_ms"] = round(float(np.median(free)), 3)
    out["lapack_over_device"] = round(out["lapack"]["total_ms"] / out["device"]["total_ms"], 2)
    out["device_full_over_device"] = round(out["device_full"]["total_ms"] / out["device"]["total_ms"], 3)
    out["device_full_event_ms"] = {k: round(float(np.median(v)), 3) for k, v in events.items()}
    out["tridiagonal_solver_alone"] = {k: round(float(np.median(v)), 3) for k, v in solver_alone.items()}
    out["device_full_solver"] = solver_used
    out["device_full_check"] = {"residual_over_uT": check_f[0], "rayleigh_over_uT": check_f[1],
                                "orthogonality_over_n_eps": check_f[2]}
    res, eig, orth, desc = ref.contracts(S, w, Vd)
    out["device_contracts"] = {"residual_over_u": float(res), "eigenvalues_over_u": float(eig),
                               "orthogonality_over_n_eps": float(orth), "descending": desc}
    res, eig, orth, desc = ref.contracts(S, w_f, Vf)
    out["device_full_contracts"] = {"residual_over_u": float(res), "eigenvalues_over_u": float(eig),
                                    "orthogonality_over_n_eps": float(orth), "descending": desc}
    out["max_abs_diff_scores_full_over_max_abs"] = float(np.abs(scores_f - scores_l).max() / np.abs(scores_l).max())
    out["max_abs_diff_scores_over_max_abs"] = float(np.abs(scores_d - scores_l).max() / np.abs(scores_l).max())
    out["relative_gap_of_the_last_kept_component"] = float((lam[-n_comps] - lam[-n_comps - 1]) / lam[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pca", action="store_true")
    ap.add_argument("--filter", action="store_true")
    ap.add_argument("--harmony", action="store_true")
    ap.add_argument("--hvg", action="store_true")
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--filter-cells", type=int, default=50000)
    ap.add_argument("--filter-genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--host-clusters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pca and not a.out:
        a.out = os.path.join(ROOT, "profiles", "preprocess_probe_pca_full_%dx%d.json" % (a.cells, a.genes))
    if a.pca or a.filter or a.harmony or a.hvg:
        out = pca_leg(a) if a.pca else filter_leg(a) if a.filter else harmony_leg(a) if a.harmony else hvg_leg(a)
        print(json.dumps(out, indent=1))
        if a.out:
            with open(a.out, "w") as F:
                json.dump(out, F, indent=1)
        return
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
