"""Fixed seeded jobs through whichever build of the library CNMF_LIB_PATH names, for bit-identity A/B runs of two builds:
    CNMF_LIB_PATH=/path/to/libcnmf_hip.so [CNMF_GEMM3=2 ...] python tools/ab_identity.py wide|general|f32|mode|hi|init|streamk|streamk_general|hints|staging|mu
Prints one JSON line: SHA-256 digests of everything the job's batch calls returned (H, n_iter, viol) and of the
last_stats fields that describe the schedule.  One process per library and per knob value; the lines must be equal.
``hi`` is ``mode`` with three counts raised above the bases of both count formats: under CNMF_GEMM3=3 and 4 both builders
write a flagged second plane and the GEMM passes take their two-plane count stream.
``staging`` runs no coordinate-descent batch: it digests every array the prepare / preprocess / filter / HVG entry points,
the column moments of a CSR-resident matrix and a Kullback-Leibler batch on the non-zeros return for one small count matrix
(staging_matrix) and for a real-valued copy of it, whose fixed-order float64 sums depend on their order.  ``mu`` digests H, W, n_iter
and err of multiplicative-update calls that refill slots, on the dense matrix pipe and on the non-zeros; run it once per
arm: no knob, CNMF_MU_VALU=1 (then the first 6 restarts of every call), CNMF_MU_SPARSE=0|1, CNMF_SP_ORDER=0."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cnmf_amd import synth  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402

STATS = ("kc", "nsplit", "gemm_mode", "outer_iterations", "column_iterations", "restart_iterations", "tail_iterations",
         "tail_live_columns")


def draw(rs, n, lo=5, hi=14):
    return [int(k) for k in rs.randint(lo, hi, size=n)], [int(s) for s in rs.randint(1, 2**31 - 1, size=n)]


def calls(job):
    """(matrix, [keyword arguments of one nmf_batch call, ...]) of a job"""
    rs = np.random.RandomState(5)
    if job in ("wide", "mode", "hi", "init", "hints"):            # count path; 150 restarts: 1024 columns, refill, defragmentation, 768 / 512 / 256, f32 tail
        X = synth.make_config("C3", dtype=np.float32, n_cells=6000)
        if job == "init":                           # caller-supplied factors of very different size (the exponent guess of the W planes)
            ks = [40, 64, 50, 30, 60, 45, 33]
            W0 = [np.abs(rs.standard_normal((X.shape[0], k))).astype(np.float32) * np.float32(10.0 ** (i - 3)) for i, k in enumerate(ks)]
            H0 = [np.abs(rs.standard_normal((k, X.shape[1]))).astype(np.float32) for k in ks]
            return X, [dict(ks=ks, W0=W0, H0=H0, max_iter=40)]
        if job == "hints":                          # the same call twice: the second one ordered by what the first one learned
            ks, seeds = draw(rs, 60)
            return X, [dict(ks=ks, seeds=seeds, max_iter=60), dict(ks=ks, seeds=seeds, max_iter=60, hints=True)]
        if job == "hi":                             # counts of 300, 2500 and 5000 in three places (tests/test_gpu_nmf.py)
            N, G, K, mu, sg, seed = synth.CONFIGS["C3"]
            C, _ = synth.topic_counts(X.shape[0], G, K, mu, sg, seed)
            C = C[:, C.sum(axis=0) > 0]
            assert C.shape == X.shape
            for (i, g, c) in ((3, 5, 300), (700, 400, 2500), (11, 17, 5000)):
                X[i, g] = np.float64(X[:, g][X[:, g] > 0].min()) * c / C[:, g][C[:, g] > 0].min()
        ks, seeds = draw(rs, 150 if job == "wide" else 44)
        return X, [dict(ks=ks, seeds=seeds, max_iter=60)]
    if job == "general":                            # tests/test_gpu_nmf.py: the perturbed matrix, 256 and 1024 columns
        X = synth.make_config("C3", dtype=np.float32, n_cells=9000)
        X = (X * np.exp(0.3 * rs.standard_normal((X.shape[0], 1)))).astype(np.float32) + np.float32(0.003)
        out = []
        for n, kc in ((40, 256), (150, 1024)):
            ks, seeds = draw(rs, n)
            out.append(dict(ks=ks, seeds=seeds, max_iter=60, kc_max=kc))
        return X, out
    if job in ("streamk", "streamk_general"):      # 12 500 cells x 1024 columns = 196 pass-A tiles: the stream-K launcher of the f16 kernels
        X = synth.make_config("C3", dtype=np.float32, n_cells=12500)
        if job == "streamk_general":
            X = (X * np.exp(0.3 * rs.standard_normal((X.shape[0], 1)))).astype(np.float32) + np.float32(0.003)
        ks, seeds = draw(rs, 150)
        return X, [dict(ks=ks, seeds=seeds, max_iter=60, kc_max=1024)]
    if job == "f32":                                # ragged: the f32 pipe at every rank tier, then a 128-column batch that refills
        X = rs.gamma(0.4, 1.0, size=(300, 170)).astype(np.float32)
        out = []
        for ks in ([3, 16, 33, 65, 128], [96, 33, 16, 65, 3]):
            out.append(dict(ks=ks, seeds=draw(rs, len(ks))[1], max_iter=100))
        out.append(dict(ks=[9] * 40, seeds=draw(rs, 40)[1], max_iter=100, kc_max=128))
        return X, out
    raise SystemExit("unknown job %r" % job)


def staging_matrix():
    """4133 cells x 37 genes of integer counts, about 15 % stored: more than 4096 rows, so the staging transpose puts two
    rows into a chunk and its last chunk is short; cell 2000 and the last cell are empty, and so is gene 11"""
    import scipy.sparse as sp
    rs = np.random.RandomState(4133)
    D = rs.poisson(3.0, size=(4133, 37)) * (rs.random_sample((4133, 37)) < 0.15)
    D[2000] = 0
    D[-1] = 0
    D[:, 11] = 0
    return sp.csr_matrix(D.astype(np.float64))


def staging():
    """{name: SHA-256} of every array the staging entry points return for staging_matrix()"""
    import ctypes as C
    import scipy.sparse as sp
    out = {}

    def put(name, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            if sp.issparse(a):
                a = np.concatenate([np.asarray(a.shape, dtype=np.int64), a.indptr.astype(np.int64), a.indices.astype(np.int64),
                                    a.data.view(np.int64)])
            h.update(np.ascontiguousarray(a).tobytes())
        assert name not in out
        out[name] = h.hexdigest()

    X = staging_matrix()
    N, G = X.shape
    genes = np.arange(G - 1, -1, -3)                          # descending, gene 11 (no entries: zero variance) among them
    live = genes[genes != 11]
    eng = Engine(0)
    for dt in (np.float32, np.float64):
        t = np.dtype(dt).name
        Xd = X.astype(dt)
        for densify, sel in ((False, genes), (True, live)):
            eng.prepare_upload(Xd)
            put("prepare_tpm_stats_%s_%d" % (t, densify), *eng.prepare_tpm_stats(1e6, want_tpm=True))
            put("prepare_select_%s_%d" % (t, densify), *eng.prepare_select(sel, densify))
            put("prepare_resident_%s_%d" % (t, densify), eng.get_matrix())
        if dt == np.float32:                                   # (Engine.preprocess_upload widens on the host: the float32 upload by hand)
            ip, ix, v = X.indptr.astype(np.int64), X.indices.astype(np.int32), Xd.data
            eng._check(eng._lib.cnmf_preprocess_upload_csr(eng._ctx, ip.ctypes.data_as(C.POINTER(C.c_int64)),
                                                           ix.ctypes.data_as(C.POINTER(C.c_int32)), v.ctypes.data_as(C.c_void_p),
                                                           0, N, G))
            eng._pre = {"N": N, "G": G, 0: None, 1: None}
        else:
            eng.preprocess_upload(Xd)
        put("select_std_%s" % t, eng.preprocess_select(0, genes, 1e4, 2.5), eng.preprocess_select(1, genes, 0.0, 2.5))
        put("select_fetch_%s" % t, eng.preprocess_fetch(0), eng.preprocess_fetch(1))
        eng.preprocess_densify(1)
        put("select_dense_%s" % t, eng.preprocess_fetch(1))
        cells, kept = np.arange(N) % 3 != 1, np.arange(G) % 5 != 2
        put("gene_detect_%s" % t, *eng.preprocess_gene_detect(), *eng.preprocess_gene_detect(cells))
        put("cell_sums_%s" % t, eng.preprocess_cell_sums(), eng.preprocess_cell_sums(kept))
        put("subset_%s" % t, np.asarray(eng.preprocess_subset(cells, kept), dtype=np.int64))
        put("fetch_counts_%s" % t, eng.preprocess_fetch_counts(), eng.preprocess_fetch_counts(1e4))
        put("select_after_subset_%s" % t, eng.preprocess_select(0, np.arange(int(kept.sum()))[::-1], 1e4, None),
            eng.preprocess_fetch(0))
        eng.preprocess_release()
    # The fixed-order sums.  The counts above are integers, whose float64 sums are exact in any order: a real-valued copy
    # (every entry times a non-dyadic factor of its own) makes the sums depend on their order.
    R = X.copy()
    R.data = R.data * (1.0 + 0.37 * np.sin(1.0 + np.arange(R.nnz)))
    cells, kept = np.arange(N) % 3 != 1, np.arange(G) % 5 != 2
    codes = (np.arange(N) * 7 % 11 >= np.array([0, 5, 9])[:, None]).sum(axis=0) - 1      # three batches of unequal size
    assert len(set(np.bincount(codes, minlength=3))) == 3 and codes.min() == 0 and codes.max() == 2
    eng.preprocess_upload_as_stored(R)
    put("real_row_sums", eng.preprocess_row_sums())
    put("real_gene_detect", *eng.preprocess_gene_detect(), *eng.preprocess_gene_detect(cells))
    put("real_cell_sums", eng.preprocess_cell_sums(), eng.preprocess_cell_sums(kept))
    put("real_fetch_counts", eng.preprocess_fetch_counts(1e4))
    put("real_clipped_sums", *eng.preprocess_clipped_sums(0.9 + 0.613 * np.arange(G)))
    put("real_normalize_dense", eng.preprocess_normalize_dense(0, 1e4, 2.5), eng.preprocess_fetch(0))
    eng.preprocess_upload_as_stored(X)
    put("int_gene_moments", *(np.asarray(a) for a in eng.preprocess_gene_moments()))
    put("int_clipped_sums", *eng.preprocess_clipped_sums(1.0 + np.arange(G) % 4))
    put("int_gene_moments_batched", *eng.preprocess_gene_moments_batched(codes, 3))
    put("int_clipped_sums_batched", *eng.preprocess_clipped_sums_batched(codes, 3, 1.0 + np.arange(3 * G).reshape(3, G) % 5))
    put("int_normalize_dense", eng.preprocess_normalize_dense(1, 0.0, None), eng.preprocess_fetch(1))
    eng.preprocess_release()
    # the resident matrix as CSR: the column moments from the compressed rows of X^T (ensure_csc), then Kullback-Leibler
    # on the non-zeros
    eng.set_matrix(R.astype(np.float32))
    assert not eng.matrix_images()["dense"], eng.matrix_images()
    put("csc_col_mean_var", *eng.col_mean_var())
    eng.set_matrix(X.astype(np.float32))
    H, W, n_iter, err = eng.nmf_mu_batch([5, 5], seeds=[11, 12], max_iter=10, return_W=True, warn=False)
    images = eng.matrix_images()
    assert images["csr_of_transpose"] and images["non_zero_images_16"], images
    put("kl_batch", *H, *W, n_iter, err)
    eng.close()
    return out


def mu():
    """{name: SHA-256} of what the multiplicative-update calls return: the 70- and 40-restart refill calls of
    tests/test_gpu_mu_refill.py, Itakura-Saito, padded rank 64 at a max_iter that is no multiple of 10, a caller-initialised
    regularised restart and the refit with H fixed"""
    from oracle import nmf_cd
    out = {}
    valu = os.environ.get("CNMF_MU_VALU", "0") not in ("", "0")

    def put(name, eng, ks, **kw):
        n = 6 if valu else len(ks)
        for key in ("seeds", "W0", "H0"):
            if kw.get(key) is not None:
                kw[key] = kw[key][:n]
        H, W, n_iter, err = eng.nmf_mu_batch(ks[:n], return_W=True, warn=False, **kw)
        h = hashlib.sha256()
        for a in list(H) + list(W) + [np.asarray(n_iter, dtype=np.int32), np.asarray(err, dtype=np.float64)]:
            h.update(np.ascontiguousarray(a).tobytes())
        out[name] = h.hexdigest()
        out[name + "_n_iter"] = [int(v) for v in n_iter]

    X = synth.make_config("C1", dtype=np.float64, n_cells=700)
    eng = Engine(0)
    eng.set_matrix(X)
    put("kl_refill_70", eng, [2 + (7 * i) % 15 for i in range(70)], seeds=[1000 + i for i in range(70)], max_iter=200)
    put("kl_rank_64", eng, [40, 33, 64, 48, 57], seeds=[300 + i for i in range(5)], max_iter=25, tol=0.0)
    W0, H0 = nmf_cd.random_init(X, 6, 11)
    put("kl_custom_init", eng, [6], W0=[W0], H0=[H0], max_iter=200, alpha_W=0.001, alpha_H=0.002, l1_ratio=0.5)
    Hn = H0 / H0.sum(axis=1, keepdims=True)
    W, n = eng.nnls_mu(Hn, max_iter=100, warn=False)
    out["nnls_mu"] = hashlib.sha256(np.ascontiguousarray(W).tobytes() + str(int(n)).encode()).hexdigest()
    # ... and the same refit through cnmf_nmf_mu_batch itself (update_H = 0: W starts at avg, H0 stays), which the engine
    # does not call any more
    import ctypes as C
    from cnmf_amd import _lib
    ks = np.asarray([6, 6], dtype=np.int32)
    h0 = np.ascontiguousarray(np.concatenate([Hn, 2.0 * Hn]), dtype=np.float32)
    avg = np.asarray([eng.init_scale(6)] * 2, dtype=np.float64)
    prm = _lib.CdParams(1e-4, 100, 0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    Wf = np.zeros(12 * X.shape[0], dtype=np.float32)
    n_it, er = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.float64)
    f32p = C.POINTER(C.c_float)
    eng._check(eng._lib.cnmf_nmf_mu_batch(eng._ctx, 2, ks.ctypes.data_as(C.POINTER(C.c_int32)), 0, None,
                                          avg.ctypes.data_as(C.POINTER(C.c_double)), None, h0.ctypes.data_as(f32p), 1, 0,
                                          C.byref(prm), None, Wf.ctypes.data_as(f32p), n_it.ctypes.data_as(C.POINTER(C.c_int32)),
                                          er.ctypes.data_as(C.POINTER(C.c_double))))
    out["update_h_0"] = hashlib.sha256(Wf.tobytes() + n_it.tobytes() + er.tobytes()).hexdigest()
    out["update_h_0_n_iter"] = [int(v) for v in n_it]
    eng.set_matrix(X + 1e-3)
    put("is_batch", eng, [5, 3, 16, 17, 9, 24, 7, 40], seeds=[40 + i for i in range(8)], beta_loss="itakura-saito", max_iter=60)
    C, _ = synth.topic_counts(1200, 900, 6, 4.6, 0.4, 1200)
    eng.set_matrix(synth.normalise_like_prepare(C, dtype=np.float32))
    put("kl_sparse_40", eng, [3 + i % 14 for i in range(40)], seeds=[2000 + i for i in range(40)], max_iter=60)
    out["images"] = {k: v for k, v in eng.matrix_images().items() if k.startswith("non_zero")}
    eng.close()
    return out


def main():
    job = sys.argv[1]
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("CNMF_") and k != "CNMF_LIB_PATH"}
    if job in ("staging", "mu"):
        print(json.dumps({"job": job, "env": env, "seen": [], "sha256": staging() if job == "staging" else mu()}))
        return
    X, jobs = calls(job)
    eng = Engine(0)
    eng.set_matrix(X)
    h = {name: hashlib.sha256() for name in ("H", "n_iter", "viol") + STATS}
    seen = []
    for kw in jobs:
        if kw.pop("hints", False):
            eng.set_iteration_hints(eng.iteration_means())
        H, _, n_iter, viol = eng.nmf_batch(kw.pop("ks"), warn=False, **kw)
        for a in H:
            h["H"].update(np.ascontiguousarray(a).tobytes())
        h["n_iter"].update(np.ascontiguousarray(n_iter, dtype=np.int32).tobytes())
        h["viol"].update(np.ascontiguousarray(viol, dtype=np.float64).tobytes())
        for name in STATS:
            h[name].update(str(int(eng.last_stats[name])).encode() + b";")
        seen.append({name: int(eng.last_stats[name]) for name in ("kc", "gemm_mode", "outer_iterations", "tail_iterations")})
    print(json.dumps({"job": job, "env": env, "seen": seen,
                      "sha256": {name: d.hexdigest() for name, d in h.items()}}))


if __name__ == "__main__":
    main()
