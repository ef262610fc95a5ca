"""cNMF.prepare on the device against what the UNMODIFIED reference's prepare wrote for the same raw counts:
tests/golden/ref_small.npz / ref_small_is.npz (dense branch, tools/make_golden.py) and ref_prepare_sparse.npz (sparse
branch, tools/make_golden_prepare.py).  The counts are regenerated here from the seeds those tools used."""
import ctypes as C
import os
import time

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import synth
from cnmf_amd.cnmf import cNMF, load_csr, load_df_from_npz, select_highvar_genes
from cnmf_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL = 1e-12


def close(a, b, rel=REL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return np.abs(a - b).max() <= rel * np.abs(b).max()


def small_counts(plus_one=False):
    """tools/make_golden.py's input."""
    Cm, _ = synth.topic_counts(240, 400, 5, mu_lib=7.0, sigma_lib=0.3, seed=7)
    Cm = Cm[:, Cm.sum(axis=0) > 0]
    if plus_one:
        Cm = Cm + 1
    return pd.DataFrame(Cm.astype(np.int64), index=["c%d" % i for i in range(Cm.shape[0])],
                        columns=["g%d" % j for j in range(Cm.shape[1])])


@pytest.fixture(scope="module")
def prep_gold():
    return dict(np.load(os.path.join(GOLD, "ref_prepare_sparse.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def sparse_counts(prep_gold):
    """tools/make_golden_prepare.py's input (make_counts)."""
    n, g, k, mu, sg, seed = prep_gold["params"].tolist()
    n, g, k, seed = int(n), int(g), int(k), int(seed)
    Cm, _ = synth.topic_counts(n, g, k, mu_lib=mu, sigma_lib=sg, seed=seed)
    Cm += synth.topic_counts(n, g, 1, mu_lib=mu, sigma_lib=sg, seed=seed + 1)[0]
    Cm = Cm[:, Cm.sum(axis=0) > 0]
    assert Cm.shape == tuple(prep_gold["shape"])
    return pd.DataFrame(Cm.astype(np.int64), index=["c%d" % i for i in range(Cm.shape[0])],
                        columns=["g%d" % j for j in range(Cm.shape[1])])


def genes_written(obj):
    return open(obj.paths["nmf_genes_list"]).read().split("\n")


# ---------------------------------------------------------------- 1. dense branch against ref_small / ref_small_is
@pytest.mark.parametrize("fixture, beta_loss", [("ref_small.npz", "frobenius"), ("ref_small_is.npz", "itakura-saito")])
def test_dense_branch_matches_reference(tmp_path, engine, fixture, beta_loss):
    g = dict(np.load(os.path.join(GOLD, fixture), allow_pickle=False))
    counts = small_counts(plus_one=beta_loss == "itakura-saito")
    from cnmf_amd.cnmf import save_df_to_npz
    counts_fn = str(tmp_path / "counts.df.npz")
    save_df_to_npz(counts, counts_fn)
    obj = cNMF(output_dir=str(tmp_path), name="d", engine=engine)
    obj.prepare(counts_fn, components=[4, 5, 6], n_iter=12, densify=True, seed=14, num_highvar_genes=150,
                beta_loss=beta_loss)
    assert genes_written(obj) == list(g["genes"])
    led = load_df_from_npz(obj.paths["nmf_replicate_parameters"])
    assert np.array_equal(led[["n_components", "iter", "nmf_seed"]].values.astype(np.int64), g["ledger"])
    nc = load_df_from_npz(obj.paths["normalized_counts"])
    assert list(nc.columns) == list(g["genes"]) and nc.values.dtype == np.float64
    assert close(nc.values, g["norm_counts"])
    tpm = load_df_from_npz(obj.paths["tpm"])
    assert list(tpm.columns) == list(g["tpm_genes"]) and close(tpm.values, g["tpm"])
    stats = load_df_from_npz(obj.paths["tpm_stats"])
    assert close(stats.values[:, 0], g["tpm_stats"][:, 0]) and close(stats.values[:, 1], g["tpm_stats"][:, 1])
    if beta_loss != "frobenius":
        return          # (the Itakura-Saito restarts: tests/test_gpu_is_tail.py holds them to the reference per restart)
    # the matrix stayed resident: factorize -> combine meets the pipeline test's bar
    obj.factorize()
    obj.combine()
    for k in (4, 5, 6):
        merged = load_df_from_npz(obj.paths["merged_spectra"] % k).values
        assert ((merged - g["merged_k%d" % k]) ** 2).sum() < 1e-4, k


# ---------------------------------------------------------------- 2. sparse branch against ref_prepare_sparse
def check_sparse_run(obj, gold, tag):
    assert genes_written(obj) == list(gold[tag + "_genes"])
    path = obj.paths["normalized_counts_sparse"]
    X = load_csr(path)
    assert open(path + ".genes.txt").read().split("\n") == list(gold[tag + "_genes"])
    assert np.array_equal(X.indptr, gold[tag + "_indptr"]) and np.array_equal(X.indices, gold[tag + "_indices"])
    ref = gold[tag + "_counts"].astype(np.float64) * gold[tag + "_inv_std"][gold[tag + "_indices"].astype(np.int64)]
    assert X.data.dtype == np.float64 and close(X.data, ref)
    stats = load_df_from_npz(obj.paths["tpm_stats"]).values
    st = gold[tag + "_tpm_stats"]
    assert close(stats[:, 0], st[:, 0]) and close(stats[:, 1], st[:, 1])


def test_sparse_branch_top_route(tmp_path, engine, prep_gold, sparse_counts):
    obj = cNMF(output_dir=str(tmp_path), name="s", engine=engine)
    obj.prepare(sparse_counts, components=[5], n_iter=2, seed=14, num_highvar_genes=500)
    check_sparse_run(obj, prep_gold, "top")
    assert os.path.exists(obj.paths["tpm_sparse"]) and not os.path.exists(obj.paths["tpm"])


def test_sparse_branch_genes_file_route(tmp_path, engine, prep_gold, sparse_counts):
    fn = str(tmp_path / "genes.txt")
    with open(fn, "w") as F:
        F.write("\n".join(prep_gold["file_list"]))
    m = sp.csr_matrix(sparse_counts.values)
    obj = cNMF(output_dir=str(tmp_path), name="f", engine=engine)
    obj.prepare((m, sparse_counts.index, sparse_counts.columns), components=[5], n_iter=2, seed=14, genes_file=fn)
    assert list(prep_gold["file_genes"]) == list(prep_gold["file_list"])            # the file's order, not the input's
    check_sparse_run(obj, prep_gold, "file")


def test_sparse_branch_threshold_route_and_zero_cells(tmp_path, engine, prep_gold, sparse_counts):
    """threshold route on the tpm= input; the reference stops at its zero-cell check: the same exception text
    (cell count and examples) -- and the HVG list the device statistics give is the reference's."""
    tpm = sparse_counts * int(prep_gold["thr_tpm_scale"])
    obj = cNMF(output_dir=str(tmp_path), name="t", engine=engine)
    with pytest.raises(Exception) as ei:
        obj.prepare(sparse_counts, components=[5], n_iter=2, seed=14, num_highvar_genes=None, tpm=tpm)
    assert str(ei.value) == str(prep_gold["thr_error"])
    # what the reference has on disk when its check fires (cnmf.py:407-447, 545): the gene list, the TPM, its statistics
    assert genes_written(obj) == list(prep_gold["thr_genes"])
    st = load_df_from_npz(obj.paths["tpm_stats"]).values
    assert close(st[:, 0], prep_gold["thr_tpm_stats"][:, 0]) and close(st[:, 1], prep_gold["thr_tpm_stats"][:, 1])
    assert os.path.exists(obj.paths["tpm_sparse"])
    engine.prepare_upload(sp.csr_matrix(tpm.values))
    _, mean, var, _ = engine.prepare_tpm_stats(0.0)
    st = prep_gold["thr_tpm_stats"]
    assert close(mean, st[:, 0]) and close(np.sqrt(var), st[:, 1])
    mask, _ = select_highvar_genes(mean, var, numgenes=None)
    assert list(sparse_counts.columns[mask]) == list(prep_gold["thr_genes"])


def test_threshold_route_without_genes_stops_at_the_zero_cell_check(tmp_path, engine, sparse_counts):
    """At TPM scale this data has no gene above T = 1 + std(fano): the reference's norm_counts has no column and every
    cell fails its zero-cell check (tools/make_golden_prepare.py)."""
    obj = cNMF(output_dir=str(tmp_path), name="e", engine=engine)
    with pytest.raises(Exception) as ei:
        obj.prepare(sparse_counts, components=[5], n_iter=2, seed=14, num_highvar_genes=None)
    n = sparse_counts.shape[0]
    assert str(ei.value) == ("Error: %d cells have zero counts of overdispersed genes. E.g. c0, c1, c2, c3. Filter those "
                             "cells and re-run or adjust the number of overdispersed genes. Quitting!" % n)
    assert open(obj.paths["nmf_genes_list"]).read() == ""
    assert os.path.exists(obj.paths["tpm_sparse"]) and os.path.exists(obj.paths["tpm_stats"])


def test_failed_prepare_leaves_no_stale_resident_matrix(tmp_path, engine, sparse_counts):
    """prepare A; a second prepare on the same object replaces the resident matrix and then stops at the zero-cell check
    (same gene count); factorize must still run on A's files -- bit for bit what a fresh worker computes from them."""
    obj = cNMF(output_dir=str(tmp_path), name="a", engine=engine)
    obj.prepare(sparse_counts, components=[5], n_iter=3, seed=14, num_highvar_genes=300)
    bad = sparse_counts.copy()
    bad.iloc[0] = 0
    with pytest.raises(Exception, match="^Error: 1 cells have zero counts"):
        obj.prepare(bad, components=[5], n_iter=3, seed=14, num_highvar_genes=300)
    assert engine.shape == (sparse_counts.shape[0], 300)          # (the failed selection IS resident now)
    obj.factorize(write_iter_files=False)
    fresh = cNMF(output_dir=str(tmp_path), name="a")
    try:
        fresh.factorize(write_iter_files=False)
        assert sorted(obj.spectra_cache) == sorted(fresh.spectra_cache)
        for key, H in obj.spectra_cache.items():
            assert np.array_equal(H, fresh.spectra_cache[key]), key
    finally:
        fresh.engine.close()


def test_staging_is_released_when_prepare_stops_early(tmp_path, engine, sparse_counts):
    fn = str(tmp_path / "genes.txt")
    open(fn, "w").write("g1\nno_such_gene")
    obj = cNMF(output_dir=str(tmp_path), name="k", engine=engine)
    with pytest.raises(KeyError):
        obj.prepare(sparse_counts, components=[5], n_iter=2, genes_file=fn)
    rs, mean, var = np.empty(1), np.empty(1), np.empty(1)
    dblp = C.POINTER(C.c_double)
    rc = engine._lib.cnmf_prepare_tpm_stats(engine._ctx, 1e6, rs.ctypes.data_as(dblp), mean.ctypes.data_as(dblp),
                                            var.ctypes.data_as(dblp), None)
    assert rc == -4                                                 # CNMF_ESTATE: nothing staged any more


# ---------------------------------------------------------------- 3. determinism, int64 row pointers, 4. handoff
def run_files(obj):
    X = load_csr(obj.paths["normalized_counts_sparse"])
    T = load_csr(obj.paths["tpm_sparse"])
    S = load_df_from_npz(obj.paths["tpm_stats"]).values
    return [X.indptr, X.indices, X.data, T.indptr, T.indices, T.data, S]


def test_determinism_int64_indptr_and_resident_images(tmp_path, engine, sparse_counts):
    m32 = sp.csr_matrix(sparse_counts.values.astype(np.float32))
    m64 = m32.copy()
    m64.indices, m64.indptr = m32.indices.astype(np.int64), m32.indptr.astype(np.int64)   # (scipy's constructor would narrow them)
    assert m64.indptr.dtype == np.int64
    files, images = [], []
    for i, m in enumerate([m32, m64, m64]):
        obj = cNMF(output_dir=str(tmp_path), name="r%d" % i, engine=engine)
        obj.prepare((m, sparse_counts.index, sparse_counts.columns), components=[5], n_iter=2, seed=14,
                    num_highvar_genes=500)
        files.append(run_files(obj))
        flags = engine.matrix_images()
        assert flags["csr"] and not flags["dense"]
        images.append((flags, engine.get_matrix()))
    for f in files[1:]:
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(files[0], f))
    for flags, im in images[1:]:
        assert flags == images[0][0] and np.array_equal(im.view(np.uint32), images[0][1].view(np.uint32))
    # the images another worker builds from the written file (set_matrix) are the same, bit for bit
    other = Engine(0)
    try:
        other.set_matrix(load_csr(obj.paths["normalized_counts_sparse"]))
        assert other.matrix_images() == images[0][0]
        assert np.array_equal(other.get_matrix().view(np.uint32), images[0][1].view(np.uint32))
    finally:
        other.close()


@pytest.mark.parametrize("densify", [False, True])
def test_resident_handoff_matches_a_fresh_worker(tmp_path, engine, sparse_counts, densify):
    obj = cNMF(output_dir=str(tmp_path), name="h", engine=engine)
    obj.prepare(sparse_counts, components=[5, 7], n_iter=3, seed=14, num_highvar_genes=300, densify=densify)
    flags = engine.matrix_images()
    assert flags["dense"] == densify and flags["csr"] == (not densify)
    x_mean = engine.x_mean
    obj.factorize(write_iter_files=False)
    fresh = cNMF(output_dir=str(tmp_path), name="h")                     # its own engine, reads the files
    try:
        fresh.factorize(write_iter_files=False)
        assert fresh.engine.x_mean == x_mean and fresh.engine.x_dtype == engine.x_dtype
        assert sorted(obj.spectra_cache) == sorted(fresh.spectra_cache)
        for key, H in obj.spectra_cache.items():
            assert np.array_equal(H, fresh.spectra_cache[key]), key
    finally:
        fresh.engine.close()


# ---------------------------------------------------------------- 5. errors and edge rows
def test_zero_total_cell_gets_zero_tpm_row(engine):
    rs = np.random.RandomState(3)
    D = rs.poisson(0.8, (50, 30)).astype(np.float64)
    D[7] = 0.0
    engine.prepare_upload(sp.csr_matrix(D))
    row_sums, mean, var, tpm = engine.prepare_tpm_stats(1e6, want_tpm=True)
    m = sp.csr_matrix(D)
    T = sp.csr_matrix((tpm, m.indices, m.indptr), shape=m.shape).toarray()
    tot = D.sum(axis=1)
    ref = np.zeros_like(D)
    ref[tot > 0] = D[tot > 0] * (1e6 / tot[tot > 0])[:, None]          # oracle/scanpy_shim.py::_normalize_total
    assert row_sums[7] == 0 and not T[7].any()
    assert close(T, ref) and close(mean, ref.mean(axis=0)) and close(var, ref.var(axis=0))


def test_bad_staging_input_is_refused(engine):
    lib = engine._lib
    indptr = np.array([0, 2, 3], dtype=np.int64)
    data = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    for idx in ([0, 5, 1], [1, 0, 2], [0, -1, 2]):                     # out of range / not increasing / negative
        indices = np.array(idx, dtype=np.int32)
        rc = lib.cnmf_prepare_upload_csr(engine._ctx, indptr.ctypes.data_as(i64p), indices.ctypes.data_as(i32p),
                                         data.ctypes.data_as(C.c_void_p), 0, 2, 4)
        assert rc == -1, idx
    indices = np.array([0, 5, 1], dtype=np.int32)
    lib.cnmf_prepare_upload_csr(engine._ctx, indptr.ctypes.data_as(i64p), indices.ctypes.data_as(i32p),
                                data.ctypes.data_as(C.c_void_p), 0, 2, 4)
    assert b"out of range" in lib.cnmf_last_error(engine._ctx)
    with pytest.raises(ValueError):
        engine.prepare_upload(sp.csr_matrix(np.array([[1.0, -2.0], [0.0, 3.0]])))


def test_dense_branch_refuses_zero_variance_gene(tmp_path, engine):
    D = np.ones((10, 4), dtype=np.int64)
    D[:, 1] = np.arange(10)
    fn = str(tmp_path / "g.txt")
    open(fn, "w").write("gene0\ngene1")
    obj = cNMF(output_dir=str(tmp_path), name="z", engine=engine)
    with pytest.raises(ValueError, match="zero variance"):
        obj.prepare(D, components=[2], n_iter=1, densify=True, genes_file=fn)
    obj.prepare(D, components=[2], n_iter=1, densify=False, genes_file=fn)   # sc.pp.scale leaves such a column as is
    X = load_csr(obj.paths["normalized_counts_sparse"]).toarray()
    assert np.array_equal(X[:, 0], np.ones(10))


# ---------------------------------------------------------------- 6. scale
def test_moments_at_atlas_shape(engine):
    M = synth.sparse_counts(50000, 20000, density=0.07, seed=1)
    N, G = M.shape
    t0 = time.perf_counter()
    engine.prepare_upload(M)
    t1 = time.perf_counter()
    row_sums, mean, var, tpm = engine.prepare_tpm_stats(1e6, want_tpm=True)
    t2 = time.perf_counter()
    # float64 numpy restatement: TPM, column means, two-pass population variance
    scale = 1e6 / np.asarray(M.sum(axis=1), dtype=np.float64).ravel()
    rows = np.repeat(np.arange(N), np.diff(M.indptr))
    v = M.data.astype(np.float64) * scale[rows]
    assert np.array_equal(tpm, v)
    cnt = np.bincount(M.indices, minlength=G)
    m_ref = np.bincount(M.indices, weights=v, minlength=G) / N
    ssd = np.bincount(M.indices, weights=(v - m_ref[M.indices]) ** 2, minlength=G) + (N - cnt) * m_ref ** 2
    var_ref = ssd / N
    assert np.abs(mean - m_ref).max() <= REL * np.abs(m_ref).max()
    nz = m_ref > 0
    assert (np.abs(mean - m_ref)[nz] / m_ref[nz]).max() <= 1e-12
    assert (np.abs(var - var_ref)[nz] / var_ref[nz]).max() <= 1e-12
    mask_dev, _ = select_highvar_genes(mean, var, numgenes=2000)
    mask_ref, _ = select_highvar_genes(m_ref, var_ref, numgenes=2000)
    assert np.array_equal(mask_dev, mask_ref)
    t3 = time.perf_counter()
    std, rs, Y = engine.prepare_select(np.flatnonzero(mask_dev), densify=False)
    t4 = time.perf_counter()
    assert Y.shape == (N, 2000) and std.shape == (2000,)
    print("\n50000 x 20000, nnz %d: upload %.3f s, tpm stats %.3f s, select %.3f s" % (M.nnz, t1 - t0, t2 - t1, t4 - t3))
