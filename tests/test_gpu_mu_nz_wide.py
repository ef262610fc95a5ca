"""Kullback-Leibler on the non-zeros at ranks 33..64 beyond single iterations (tests/test_gpu_mu_nz_wide_steps.py): the
opt-in rank limit itself (``Engine.mu_sparse_rank_limit``), the batching contract, a seeded run to the stopping rule, the
refit, the CSR upload and the mirror class.  The bars are the ones the project holds the lower ranks and the dense kernels
to (test_gpu_mu_sparse.py, test_gpu_mu_wide.py).  Every test that raises the limit leaves it at 32.

Measured on an MI355X (pytest -s; the 9 GPU tests take 4 s together):
  rank 40 on A, 20 iterations: non-zero path against the dense kernels, relative Frobenius distance 2.62e-06 (bar 1e-3)
  rank 48 on P, tol 1e-4: oracle 60 iterations, both routes 60; max |WH - WH_ref| / max WH_ref 4.00e-06 on the non-zeros,
    3.59e-05 on the dense kernels (bar 2e-3); err 1.9e-08 on both (bar 1e-3)
  rank 48 on P, tol 3e-3: the oracle's stopping rule fires at 50, both routes stop at 50; 2.20e-06 on the non-zeros,
    3.23e-05 on the dense kernels; err 1.9e-08 and 5.3e-09
  update_H = 0 through the batch kernels at rank 40 on P: the rule stops it at 40 iterations like the oracle, max |W - W_ref|
    / max W_ref 1.50e-07 (bar 1e-3), err 2.0e-08 (bar 1e-3)
  mirror class at rank 36: max |H - H_ref| / max H_ref 4.0e-06 and 5.0e-06 on the non-zeros, 4.5e-05 and 2.1e-05 on the
    dense kernels (bar 2e-3)
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd import _lib
from cnmf_amd.cnmf import cNMF, ledger_seeds
from oracle import nmf_cd, nmf_mu
from tests import _mu_nz_wide_ref as Nz
from tests import _mu_steps_ref as R
from tests._mu_wide_ref import wide_limit

gpu = pytest.mark.gpu
KL = "kullback-leibler"
SEEDED_BAR = 2e-3                          # max |WH - WH_ref| / max WH_ref of a seeded run (tests/test_gpu_mu_wide.py)


@pytest.fixture
def nzwide(engine):
    assert engine.mu_sparse_rank_limit == 32
    with Nz.nz_wide_limit(engine):
        yield engine
    assert engine.mu_sparse_rank_limit == 32


def _same(a, b, i, j=0):
    """Restart i of result a and restart j of result b: H, W, n_iter and err bit for bit."""
    return (np.asarray(a[0][i]).tobytes() == np.asarray(b[0][j]).tobytes() and np.asarray(a[1][i]).tobytes() == np.asarray(b[1][j]).tobytes()
            and int(a[2][i]) == int(b[2][j]) and np.float64(a[3][i]).tobytes() == np.float64(b[3][j]).tobytes())


# ---------------------------------------------------------------- CPU: the Python-only parts
def test_lib_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cnmf_hip.h")).read()
    defs = dict(re.findall(r"^#define (CNMF_MU_SPARSE_KMAX(?:_WIDE)?)\s+(\d+)", hdr, flags=re.M))
    assert int(defs["CNMF_MU_SPARSE_KMAX"]) == _lib.CNMF_MU_SPARSE_KMAX == 32
    assert int(defs["CNMF_MU_SPARSE_KMAX_WIDE"]) == _lib.CNMF_MU_SPARSE_KMAX_WIDE == 64 == _lib.CNMF_MU_KMAX
    assert "cnmf_set_mu_sparse_rank_limit" in _lib.SYMBOLS and "cnmf_get_mu_sparse_rank_limit" in _lib.SYMBOLS


def test_the_scope_restores_a_shared_engine():
    class Eng:
        mu_rank_limit = 64
        mu_sparse_rank_limit = 32
    assert cNMF.mu_sparse_ranks is None
    obj, eng = cNMF.__new__(cNMF), Eng()
    with obj._mu_rank_scope(eng):
        assert eng.mu_sparse_rank_limit == 32                 # no opt-in: nothing is touched
    obj.mu_sparse_ranks = "wide"
    with pytest.raises(RuntimeError):
        with obj._mu_rank_scope(eng):
            assert eng.mu_sparse_rank_limit == 64 and eng.mu_rank_limit == 64
            raise RuntimeError("a device call failed")
    assert eng.mu_sparse_rank_limit == 32
    eng.mu_sparse_rank_limit = 64                             # raised by its owner: stays raised
    with obj._mu_rank_scope(eng):
        assert eng.mu_sparse_rank_limit == 64
    assert eng.mu_sparse_rank_limit == 64
    obj.mu_sparse_ranks = "broad"
    with pytest.raises(ValueError, match="mu_sparse_ranks"):
        with obj._mu_rank_scope(eng):
            pass
    assert cNMF.mu_sparse_ranks is None


def test_get_nmf_iter_params_refuses_a_mistyped_switch(tmp_path):
    obj = cNMF(output_dir=str(tmp_path), name="lim", engine=object())
    obj.mu_sparse_ranks = "broad"
    with pytest.raises(ValueError, match="mu_sparse_ranks"):
        obj.get_nmf_iter_params([40], n_iter=2, random_state_seed=1, beta_loss=KL)
    obj.mu_sparse_ranks = "wide"
    assert len(obj.get_nmf_iter_params([40], n_iter=2, random_state_seed=1, beta_loss=KL)[0]) == 2


# ---------------------------------------------------------------- GPU 1: the limit
@gpu
def test_the_limit_and_what_it_moves(engine, monkeypatch):
    """Default 32; 48 refused; rank 40 forced: the dense kernels' bits under the default, another path (to 1e-3) under the
    limit of 64; Itakura-Saito at rank 40 and Kullback-Leibler at rank 70 do not move."""
    assert engine.mu_sparse_rank_limit == 32
    with pytest.raises(ValueError):
        engine.mu_sparse_rank_limit = 48
    assert engine.mu_sparse_rank_limit == 32
    X = R.matrix("A")
    kw = dict(max_iter=20, return_W=True, warn=False)

    def runs():
        engine.set_matrix(X)
        kl40 = engine.nmf_mu_batch([40], seeds=[3], **kw)
        with wide_limit(engine):
            kl70 = engine.nmf_mu_batch([70], seeds=[4], **kw)
        engine.set_matrix(X + 1e-3)
        is40 = engine.nmf_mu_batch([40], seeds=[3], beta_loss="itakura-saito", **kw)
        return kl40, kl70, is40

    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    d40, d70, di = runs()
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    s40, s70, si = runs()
    assert _same(d40, s40, 0) and _same(d70, s70, 0) and _same(di, si, 0)
    with Nz.nz_wide_limit(engine):
        assert engine.mu_sparse_rank_limit == 64
        w40, w70, wi = runs()
        assert engine.matrix_images()["dense"]                # (the Itakura-Saito call: the last matrix)
    assert engine.mu_sparse_rank_limit == 32
    assert _same(d70, w70, 0) and _same(di, wi, 0)
    assert not np.array_equal(w40[0][0], d40[0][0])
    _, rel = nmf_cd.spectra_error(d40[0][0].astype(np.float64), w40[0][0])
    print("rank 40 on A, 20 iterations: non-zero path vs dense kernels, relative Frobenius distance %.2e" % rel)
    assert rel <= 1e-3
    monkeypatch.delenv("CNMF_MU_SPARSE")


@gpu
def test_the_density_rule_of_padded_rank_64(nzwide, monkeypatch):
    """A matrix between 15 % and a quarter non-zero: by itself rank 24 takes the non-zeros and rank 40 the dense kernels (the
    measured crossover of padded rank 64 lies below a quarter); forced, rank 40 takes them too."""
    X = R.sparse_counts(700, 500, 4.8, 41)
    assert 0.15 < (X != 0).mean() < 0.25
    kw = dict(max_iter=20, return_W=True, warn=False)
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    nzwide.set_matrix(X)
    dense = nzwide.nmf_mu_batch([24, 40], seeds=[5, 6], **kw)
    monkeypatch.delenv("CNMF_MU_SPARSE")
    nzwide.set_matrix(X)
    auto = nzwide.nmf_mu_batch([24, 40], seeds=[5, 6], **kw)
    im = nzwide.matrix_images()
    assert im["non_zero_images_32"] and not im["non_zero_images_64"]
    assert not _same(auto, dense, 0, 0) and _same(auto, dense, 1, 1)
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    forced = nzwide.nmf_mu_batch([24, 40], seeds=[5, 6], **kw)
    assert nzwide.matrix_images()["non_zero_images_64"]
    assert _same(forced, auto, 0, 0) and not _same(forced, dense, 1, 1)


# ---------------------------------------------------------------- GPU 2: batching
@gpu
def test_nz_wide_batch_matches_single_runs(nzwide, monkeypatch):
    """A restart's result does not depend on what else is in the batch, and is the same on a second run."""
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    nzwide.set_matrix(R.matrix("A"))
    ks, seeds = [33, 9, 48, 64, 24, 48], [700, 701, 702, 703, 704, 705]
    kw = dict(max_iter=20, return_W=True, warn=False)
    full = nzwide.nmf_mu_batch(ks, seeds=seeds, **kw)
    again = nzwide.nmf_mu_batch(ks, seeds=seeds, **kw)
    for i in range(len(ks)):
        assert _same(full, again, i, i), i
        if ks[i] > 32:
            assert _same(full, nzwide.nmf_mu_batch([ks[i]], seeds=[seeds[i]], **kw), i), i


@gpu
def test_nz_wide_second_round_of_slots(nzwide, monkeypatch):
    """Thirty-four rank-33 restarts: more than MU_MAXSLOTS = 32, the last two wait for retired slots."""
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    nzwide.set_matrix(R.matrix("T"))
    seeds = [3000 + i for i in range(34)]
    kw = dict(max_iter=10, return_W=True, warn=False)
    full = nzwide.nmf_mu_batch([33] * 34, seeds=seeds, **kw)
    for i in (0, 31, 33):
        assert _same(full, nzwide.nmf_mu_batch([33], seeds=[seeds[i]], **kw), i), i


# ---------------------------------------------------------------- GPU 3: a seeded run to the stopping rule
_ORACLE = {}


def _oracle_run(k, seed, max_iter, tol):
    key = (k, seed, max_iter, tol)
    if key not in _ORACLE:
        _ORACLE[key] = nmf_mu.nmf_mu(R.matrix("P"), k, seed=seed, max_iter=max_iter, tol=tol)
    return _ORACLE[key]


def _seeded_distance(engine, X, k, seed, max_iter, tol):
    """(n_iter, max |WH - WH_ref| / max WH_ref, |err - err_ref| / err_ref, n_ref) of a seeded device run against the oracle
    at the device's iteration count."""
    H, W, n, err = engine.nmf_mu_batch([k], seeds=[seed], max_iter=max_iter, tol=tol, return_W=True, warn=False)
    W_ref, H_ref, n_ref = _oracle_run(k, seed, max_iter, tol)
    n_ref0 = n_ref
    if int(n[0]) != n_ref:
        W_ref, H_ref, _ = _oracle_run(k, seed, int(n[0]), 0.0)
    P, P_ref = W[0].astype(np.float64) @ H[0], W_ref @ H_ref
    ref_err = nmf_mu.beta_divergence(X, W_ref, H_ref, 1, square_root=True)
    return int(n[0]), np.abs(P - P_ref).max() / np.abs(P_ref).max(), abs(err[0] - ref_err) / ref_err, n_ref0


@gpu
@pytest.mark.parametrize("tol", [1e-4, 3e-3])
def test_nz_wide_seeded_run_vs_oracle(nzwide, monkeypatch, tol):
    """P at rank 48, seed 6, at most 60 iterations.  With the default tol = 1e-4 the oracle uses all 60; with tol = 3e-3 its
    stopping rule fires at 50, so the iteration count is the rule's doing (the divergence kernel between the iterations
    decides it on the device).  The bar on max |WH - WH_ref| / max WH_ref is the larger of 2e-3 and 4 x the same distance of
    the dense kernels in this test."""
    X = R.matrix("P")
    nzwide.set_matrix(X)
    assert _oracle_run(48, 6, 60, tol)[2] == (60 if tol == 1e-4 else 50)
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    n_d, dist_d, err_d, n_ref = _seeded_distance(nzwide, X, 48, 6, 60, tol)
    monkeypatch.delenv("CNMF_MU_SPARSE")                      # (under a quarter non-zero: chosen by density)
    n_s, dist_s, err_s, _ = _seeded_distance(nzwide, X, 48, 6, 60, tol)
    assert nzwide.matrix_images()["non_zero_images_64"]
    print("rank 48 on P, tol %g: oracle %d iterations; non-zero path %d, max |WH - WH_ref| / max WH_ref = %.3e, err %.2e; "
          "dense kernels %d, %.3e, err %.2e" % (tol, n_ref, n_s, dist_s, err_s, n_d, dist_d, err_d))
    assert abs(n_s - n_ref) <= 10
    assert dist_s <= max(SEEDED_BAR, 4 * dist_d)
    assert err_s <= 1e-3


# ---------------------------------------------------------------- GPU 4: the refit and the CSR upload
def _refit_f32(engine, ks, Hs, tol, max_iter):
    """cnmf_nmf_mu_batch with update_H = 0, Kullback-Leibler (the float32 refit through the batch kernels: W starts at avg,
    H stays; the W half-step alone, and the divergence kernel every ten iterations for the stopping rule)."""
    import ctypes as C
    N = engine.shape[0]
    kk = np.asarray(ks, dtype=np.int32)
    h0 = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float32).ravel() for h in Hs]))
    avg = np.asarray([engine.init_scale(int(k)) for k in ks], dtype=np.float64)
    prm = _lib.CdParams(tol, max_iter, 0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    Wf = np.zeros(int(kk.sum()) * N, dtype=np.float32)
    n_it, er = np.zeros(len(ks), dtype=np.int32), np.zeros(len(ks), dtype=np.float64)
    f32p, i32p, dblp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    engine._sync_env()
    engine._check(engine._lib.cnmf_nmf_mu_batch(engine._ctx, len(ks), kk.ctypes.data_as(i32p), 0, None, avg.ctypes.data_as(dblp), None,
                                                h0.ctypes.data_as(f32p), 1, 0, C.byref(prm), None, Wf.ctypes.data_as(f32p),
                                                n_it.ctypes.data_as(i32p), er.ctypes.data_as(dblp)))
    offs = np.concatenate([[0], np.cumsum(kk)]) * N
    return [Wf[offs[r]:offs[r + 1]].reshape(N, int(kk[r])) for r in range(len(ks))], n_it, er


@gpu
def test_nz_wide_refit_update_H_0(nzwide, monkeypatch):
    """The refit with H fixed through the batch kernels at rank 40 on P, forced onto the non-zeros: the W half-step of padded
    rank 64 alone, the column sums of W and the divergence kernel between the iterations.  Against ``nmf_mu.nnls_mu`` at the
    bars of test_gpu_mu_sparse.py::test_kl_non_zero_path_refit_regularisation_and_custom_init (iterations within 10, W to
    1e-3 of its maximum) and err to 1e-3; the dense kernels give other bits."""
    X64 = R.matrix("P")
    nzwide.set_matrix(X64)
    _, Hr, _ = nmf_mu.nmf_mu(X64, 40, seed=1, max_iter=30)
    Hn = (Hr / Hr.sum(axis=1, keepdims=True)).astype(np.float32)
    H64 = Hn.astype(np.float64)
    W_ref, n_ref = nmf_mu.nnls_mu(X64, H64, max_iter=100)
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    (Wd,), _, _ = _refit_f32(nzwide, [40], [Hn], 1e-4, 100)
    assert not nzwide.matrix_images()["non_zero_images_64"]
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    (W,), n_it, er = _refit_f32(nzwide, [40], [Hn], 1e-4, 100)
    assert nzwide.matrix_images()["non_zero_images_64"]
    n = int(n_it[0])
    assert 10 < n_ref < 100 and abs(n - n_ref) <= 10              # (the stopping rule fired, on both sides)
    if n != n_ref:
        W_ref, _ = nmf_mu.nnls_mu(X64, H64, max_iter=n, tol=0.0)
    ref_err = nmf_mu.beta_divergence(X64, W_ref, H64, 1, square_root=True)
    print("update_H=0 at rank 40 on P: %d iterations (oracle %d), max |W - W_ref| / max W_ref = %.2e, err %.2e"
          % (n, n_ref, np.abs(W - W_ref).max() / np.abs(W_ref).max(), abs(er[0] - ref_err) / ref_err))
    assert np.isfinite(W).all() and W.min() >= 0 and not np.array_equal(W, Wd)
    assert np.abs(W - W_ref).max() <= 1e-3 * np.abs(W_ref).max()
    assert abs(er[0] - ref_err) <= 1e-3 * ref_err


@gpu
def test_nz_wide_csr_upload_gives_the_same_bits(nzwide):
    """The images of a CSR upload are built from the compressed rows as they came: the bits of the dense upload."""
    P32 = R.matrix("P").astype(np.float32)
    kw = dict(max_iter=20, return_W=True, warn=False)
    nzwide.set_matrix(P32)
    dense = nzwide.nmf_mu_batch([40], seeds=[77], **kw)
    assert nzwide.matrix_images()["non_zero_images_64"]
    nzwide.set_matrix(sp.csr_matrix(P32))
    assert not nzwide.matrix_images()["non_zero_images_64"]   # (the old matrix's images went with it)
    csr = nzwide.nmf_mu_batch([40], seeds=[77], **kw)
    im = nzwide.matrix_images()
    assert im["non_zero_images_64"] and im["csr"] and not im["dense"]
    assert _same(dense, csr, 0)


# ---------------------------------------------------------------- GPU 5: the mirror class
@gpu
def test_nz_wide_through_the_cnmf_callsite(engine, tmp_path):
    """``cNMF.mu_sparse_ranks = "wide"`` on a shared engine: factorize takes the non-zero path at rank 36 (another result
    than without the switch), the merged spectra are the oracle's restarts, and the engine's limit is back at 32."""
    X = np.ascontiguousarray(R.matrix("P")[:, :600])
    assert (X != 0).mean() < 0.15 and (X.sum(axis=1) > 0).all()      # (where padded rank 64 takes the non-zeros by itself)
    args = dict(components=[36], n_iter=2, seed=14, beta_loss=KL, max_NMF_iter=60)
    merged = {}
    try:
        for ranks in (None, "wide"):
            cNMF.mu_sparse_ranks = ranks
            obj = cNMF(output_dir=str(tmp_path), name="nzwide_%s" % ranks, engine=engine)
            obj.prepare_from_matrix(X.astype(np.float32), **args)
            obj.factorize()
            assert engine.mu_sparse_rank_limit == 32
            assert engine.matrix_images()["non_zero_images_64"] == (ranks == "wide")
            merged[ranks] = obj.combine_nmf(36).values
    finally:
        cNMF.mu_sparse_ranks = None
    wide, dense = merged["wide"], merged[None]
    assert wide.shape == (72, 600) and np.isfinite(wide).all() and (wide >= 0).all()
    assert not np.array_equal(wide, dense)
    led = ledger_seeds([36], 2, 14)
    for it in range(2):
        seed = [row[2] for row in led if row[0] == 36 and row[1] == it][0]
        _, H_ref, _ = nmf_mu.nmf_mu(X, 36, seed=seed, max_iter=60)
        d_w = np.abs(wide[36 * it:36 * (it + 1)] - H_ref).max() / np.abs(H_ref).max()
        d_d = np.abs(dense[36 * it:36 * (it + 1)] - H_ref).max() / np.abs(H_ref).max()
        print("restart %d at rank 36: max |H - H_ref| / max H_ref: non-zero path %.3e, dense kernels %.3e" % (it, d_w, d_d))
        assert d_w <= max(SEEDED_BAR, 4 * d_d)
