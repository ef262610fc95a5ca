"""The multiplicative-update route at ranks 65..128 beyond single iterations (tests/test_gpu_mu_wide_steps.py): the
opt-in rank limit itself, the batching contract, seeded runs to the stopping rule, the float64 refit, and the mirror class
from prepare to consensus.  The bars are the ones the project holds the lower ranks to (test_gpu_edges.py, test_gpu_mu.py,
test_gpu_kl_tail.py).  Every test that raises the limit leaves it at 64.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd import _lib, synth
from cnmf_amd.cnmf import cNMF, load_df_from_npz
from oracle import nmf_mu
from tests import _mu_steps_ref as R
from tests import _mu_wide_ref as Wd

gpu = pytest.mark.gpu
IS = "itakura-saito"


@pytest.fixture
def wide(engine):
    with Wd.wide_limit(engine):
        yield engine
    assert engine.mu_rank_limit == 64


def _same(a, b, i, j=0):
    """Restart i of result a and restart j of result b: H, W, n_iter and err bit for bit."""
    return (np.asarray(a[0][i]).tobytes() == np.asarray(b[0][j]).tobytes() and np.asarray(a[1][i]).tobytes() == np.asarray(b[1][j]).tobytes()
            and int(a[2][i]) == int(b[2][j]) and np.float64(a[3][i]).tobytes() == np.float64(b[3][j]).tobytes())


# ---------------------------------------------------------------- CPU: the Python-only parts
def test_lib_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cnmf_hip.h")).read()
    defs = dict(re.findall(r"^#define (CNMF_MU_KMAX(?:_WIDE)?)\s+(\d+)", hdr, flags=re.M))
    assert int(defs["CNMF_MU_KMAX"]) == _lib.CNMF_MU_KMAX == 64
    assert int(defs["CNMF_MU_KMAX_WIDE"]) == _lib.CNMF_MU_KMAX_WIDE == 128 == _lib.CNMF_KMAX
    assert "cnmf_set_mu_rank_limit" in _lib.SYMBOLS and "cnmf_get_mu_rank_limit" in _lib.SYMBOLS


def test_get_nmf_iter_params_limits(tmp_path):
    obj = cNMF(output_dir=str(tmp_path), name="lim", engine=object())
    assert cNMF.mu_ranks is None
    for loss in ("kullback-leibler", IS):
        with pytest.raises(NotImplementedError, match="n_components=65 > 64 is not supported by the device engine"):
            obj.get_nmf_iter_params([5, 65], n_iter=2, random_state_seed=1, beta_loss=loss)
        assert len(obj.get_nmf_iter_params([64], n_iter=2, random_state_seed=1, beta_loss=loss)[0]) == 2
    obj.mu_ranks = "wide"
    for loss in ("kullback-leibler", IS):
        assert len(obj.get_nmf_iter_params([65, 128], n_iter=2, random_state_seed=1, beta_loss=loss)[0]) == 4
        with pytest.raises(NotImplementedError, match="n_components=129 > 128"):
            obj.get_nmf_iter_params([129], n_iter=2, random_state_seed=1, beta_loss=loss)
    with pytest.raises(NotImplementedError, match="n_components=129 > 128"):
        obj.get_nmf_iter_params([129], n_iter=2, random_state_seed=1, beta_loss="frobenius")
    obj.mu_ranks = "broad"
    with pytest.raises(ValueError, match="mu_ranks"):
        obj.get_nmf_iter_params([70], n_iter=2, random_state_seed=1, beta_loss="kullback-leibler")
    assert cNMF.mu_ranks is None


def test_the_limit_scope_restores_a_shared_engine():
    class Eng:
        mu_rank_limit = 64
    obj, eng = cNMF.__new__(cNMF), Eng()
    with obj._mu_rank_scope(eng):
        assert eng.mu_rank_limit == 64                    # no opt-in: nothing is touched
    obj.mu_ranks = "wide"
    with pytest.raises(RuntimeError):
        with obj._mu_rank_scope(eng):
            assert eng.mu_rank_limit == 128
            raise RuntimeError("a device call failed")
    assert eng.mu_rank_limit == 64
    eng.mu_rank_limit = 128                               # raised by its owner: stays raised
    with obj._mu_rank_scope(eng):
        assert eng.mu_rank_limit == 128
    assert eng.mu_rank_limit == 128


# ---------------------------------------------------------------- GPU 1: the limit
def _h65(cols):
    rs = np.random.RandomState(5)
    return np.abs(rs.standard_normal((65, cols))) + 0.01


@gpu
def test_default_limit_refuses_rank_65(engine):
    engine.set_matrix(R.matrix("T"))
    assert engine.mu_rank_limit == 64
    with pytest.raises(NotImplementedError, match="64"):
        engine.nmf_mu_batch([65], seeds=[1], max_iter=5)
    with pytest.raises(NotImplementedError, match="64"):
        engine.mu_refit_f64(_h65(70), max_iter=5, warn=False)


@gpu
def test_wide_limit_admits_ranks_to_128(engine, monkeypatch):
    engine.set_matrix(R.matrix("T"))
    with pytest.raises(ValueError):
        engine.mu_rank_limit = 96
    assert engine.mu_rank_limit == 64
    with Wd.wide_limit(engine):
        assert engine.mu_rank_limit == 128
        H, _, n, err = engine.nmf_mu_batch([65], seeds=[1], max_iter=5, warn=False)
        assert H[0].shape == (65, 70) and int(n[0]) == 5 and np.isfinite(H[0]).all() and np.isfinite(err[0])
        W, it, e = engine.mu_refit_f64(_h65(70), max_iter=5, warn=False)
        assert W.shape == (45, 65) and it == 5 and np.isfinite(W).all() and np.isfinite(e)
        with pytest.raises(NotImplementedError, match="129"):
            engine.nmf_mu_batch([129], seeds=[1], max_iter=5)
        with pytest.raises(NotImplementedError):
            engine.mu_refit_f64(np.ones((129, 70)), max_iter=5, warn=False)
        monkeypatch.setenv("CNMF_MU_VALU", "1")
        with pytest.raises(NotImplementedError, match="vector-ALU"):
            engine.nmf_mu_batch([65], seeds=[1], max_iter=5)
        H64, _, _, _ = engine.nmf_mu_batch([64], seeds=[1], max_iter=2, warn=False)      # (the route itself still runs)
        assert np.isfinite(H64[0]).all()
        monkeypatch.delenv("CNMF_MU_VALU")
    assert engine.mu_rank_limit == 64
    with pytest.raises(NotImplementedError):
        engine.nmf_mu_batch([65], seeds=[1], max_iter=5)


# ---------------------------------------------------------------- GPU 2: batching
@gpu
def test_wide_batch_matches_single_runs(engine, monkeypatch):
    """A restart's result does not depend on what else is in the batch, and the members up to rank 64 do not depend on the
    limit."""
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    engine.set_matrix(R.matrix("A"))
    ks, seeds = [128, 70, 128, 9, 65], [900, 901, 902, 903, 904]
    kw = dict(max_iter=20, return_W=True, warn=False)
    with Wd.wide_limit(engine):
        full = engine.nmf_mu_batch(ks, seeds=seeds, **kw)
        for i in range(len(ks)):
            assert _same(full, engine.nmf_mu_batch([ks[i]], seeds=[seeds[i]], **kw), i), i
    assert engine.mu_rank_limit == 64
    assert _same(full, engine.nmf_mu_batch([9], seeds=[903], **kw), 3)


@gpu
def test_wide_second_round_of_slots(wide):
    """Thirty-four rank-65 restarts: more than MU_MAXSLOTS = 32, the last two wait for retired slots."""
    wide.set_matrix(R.matrix("T"))
    seeds = [3000 + i for i in range(34)]
    kw = dict(max_iter=10, return_W=True, warn=False)
    full = wide.nmf_mu_batch([65] * 34, seeds=seeds, **kw)
    for i in (0, 31, 33):
        assert _same(full, wide.nmf_mu_batch([65], seeds=[seeds[i]], **kw), i), i


# ---------------------------------------------------------------- GPU 3: seeded runs to the stopping rule
@gpu
@pytest.mark.parametrize("k,loss,shift,max_iter,bar", [(100, "kullback-leibler", 0.0, 60, 2e-3), (72, IS, 0.05, 40, 5e-3)])
def test_wide_seeded_run_vs_oracle(wide, k, loss, shift, max_iter, bar):
    X = R.matrix("A") + shift
    wide.set_matrix(X)
    W_ref, H_ref, n_ref = nmf_mu.nmf_mu(X, k, seed=6, beta_loss=loss, max_iter=max_iter)
    H, W, n, _ = wide.nmf_mu_batch([k], seeds=[6], beta_loss=loss, max_iter=max_iter, return_W=True, warn=False)
    print("rank %d %s: device %d iterations, oracle %d" % (k, loss, int(n[0]), n_ref))
    assert abs(int(n[0]) - n_ref) <= 10
    if int(n[0]) != n_ref:
        W_ref, H_ref, _ = nmf_mu.nmf_mu(X, k, seed=6, beta_loss=loss, max_iter=int(n[0]), tol=0.0)
    P, P_ref = W[0].astype(np.float64) @ H[0], W_ref @ H_ref
    print("max |WH - WH_ref| / max WH_ref = %.3e" % (np.abs(P - P_ref).max() / np.abs(P_ref).max()))
    assert np.abs(P - P_ref).max() <= bar * np.abs(P_ref).max()


# ---------------------------------------------------------------- GPU 4: the float64 refit
def _refit_inputs(n, g_, k):
    rs = np.random.RandomState(k)
    H = np.abs(rs.standard_normal((k, g_))) * (rs.rand(k, g_) < 0.5)
    H /= H.sum(axis=1, keepdims=True)
    U = np.abs(rs.standard_normal((n, k)))
    U /= U.sum(axis=1, keepdims=True)
    return H, U


@gpu
@pytest.mark.parametrize("k", [65, 100, 128])
@pytest.mark.parametrize("mname", ["A", "A+", "P"])
def test_wide_mu_refit_f64_vs_oracle(wide, mname, k):
    """refit_usage and refit_spectra in float64: the oracle's iteration count, W to 1e-9, err to 1e-10; the same bits on a
    second call.  P stays resident as compressed rows."""
    X64 = R.matrix(mname)
    loss, beta = (IS, 0) if mname.endswith("+") else ("kullback-leibler", 1)
    n, g_ = X64.shape
    H, U = _refit_inputs(n, g_, k)
    wide.set_matrix(sp.csr_matrix(X64.astype(np.float32)) if mname == "P" else X64)
    for transposed, M, F in ((False, X64, H), (True, np.ascontiguousarray(X64.T), np.ascontiguousarray(U.T))):
        W_ref, n_ref = nmf_mu.nnls_mu(M, F, beta_loss=loss, max_iter=300)
        assert np.isfinite(W_ref).all()
        W, it, err = wide.mu_refit_f64(F, transposed=transposed, beta_loss=loss, max_iter=300, warn=False)
        ref_err = nmf_mu.beta_divergence(M, W_ref, F, beta, square_root=True)
        print("%s k=%d transposed=%s: %d iterations (oracle %d), W %.2e, err %.2e" % (
            mname, k, transposed, it, n_ref, np.abs(W - W_ref).max() / np.abs(W_ref).max(), abs(err - ref_err) / ref_err))
        assert W.dtype == np.float64 and it == n_ref
        assert np.abs(W - W_ref).max() <= 1e-9 * np.abs(W_ref).max()
        assert abs(err - ref_err) <= 1e-10 * ref_err
        W2, it2, err2 = wide.mu_refit_f64(F, transposed=transposed, beta_loss=loss, max_iter=300, warn=False)
        assert it2 == it and err2 == err and W2.tobytes() == W.tobytes()


@gpu
@pytest.mark.parametrize("mname", ["A", "A+"])
def test_wide_mu_refit_f64_column_subset_and_penalty(wide, mname):
    """tol = 0, 25 iterations at rank 100: a third of the columns dropped and the rest divided by a constant each
    (col_divisor); and a mixed penalty on the whole matrix."""
    X64 = R.matrix(mname)
    loss, beta = (IS, 0) if mname.endswith("+") else ("kullback-leibler", 1)
    n, g_ = X64.shape
    k = 100
    rs = np.random.RandomState(11)
    wide.set_matrix(X64)
    keep = np.arange(g_) % 3 != 0
    div = np.where(keep, rs.uniform(0.5, 2.0, g_), 0.0)
    Xs = X64[:, keep] / div[keep]
    Hs = np.abs(rs.standard_normal((k, int(keep.sum())))) + 0.01
    H_full = np.zeros((k, g_))
    H_full[:, keep] = Hs
    W_ref, n_ref = nmf_mu.nnls_mu(Xs, Hs, beta_loss=loss, tol=0.0, max_iter=25)
    W, it, err = wide.mu_refit_f64(H_full, col_divisor=div, w_init=float(np.sqrt(Xs.mean() / k)), n_features=int(keep.sum()),
                                   beta_loss=loss, tol=0.0, max_iter=25, warn=False)
    ref_err = nmf_mu.beta_divergence(Xs, W_ref, Hs, beta, square_root=True)
    assert it == n_ref == 25 and np.abs(W - W_ref).max() <= 1e-9 * np.abs(W_ref).max() and abs(err - ref_err) <= 1e-10 * ref_err
    H = np.abs(rs.standard_normal((k, g_))) + 0.01
    pen = dict(alpha_W=0.002, l1_ratio=0.3)
    W_ref, n_ref = nmf_mu.nnls_mu(X64, H, beta_loss=loss, tol=0.0, max_iter=25, **pen)
    W, it, err = wide.mu_refit_f64(H, beta_loss=loss, tol=0.0, max_iter=25, warn=False, **pen)
    ref_err = nmf_mu.beta_divergence(X64, W_ref, H, beta, square_root=True)
    assert it == n_ref == 25 and np.abs(W - W_ref).max() <= 1e-9 * np.abs(W_ref).max() and abs(err - ref_err) <= 1e-10 * ref_err


# ---------------------------------------------------------------- GPU 5: the mirror class, end to end
@gpu
def test_wide_pipeline_prepare_to_consensus(engine, tmp_path):
    import pandas as pd
    import yaml
    C, _ = synth.topic_counts(300, 400, 6, 5.5, 0.4, 21)
    X = synth.normalise_like_prepare(C, dtype=np.float64)
    N, G = X.shape
    nc = pd.DataFrame(X, index=["c%d" % i for i in range(N)], columns=["g%d" % j for j in range(G)])
    # (four restarts, not two: consensus takes int(0.30 x restarts) neighbours for its density filter and refuses 0)
    args = dict(components=[70], n_iter=4, seed=14, beta_loss="kullback-leibler", max_NMF_iter=30)
    obj = cNMF(output_dir=str(tmp_path), name="wide", engine=engine)
    with pytest.raises(NotImplementedError):
        obj.prepare_from_matrix(nc, **args)
    obj.mu_ranks = "broad"
    with pytest.raises(ValueError):
        obj.prepare_from_matrix(nc, **args)
    obj.mu_ranks = "wide"
    obj.prepare_from_matrix(nc, **args)
    obj.factorize()
    assert engine.mu_rank_limit == 64
    obj.combine()
    obj.consensus(70, density_threshold=2.0, show_clustering=False)
    assert engine.mu_rank_limit == 64
    rep = (70, "2_0")
    spectra = load_df_from_npz(obj.paths["consensus_spectra"] % rep)
    usages = load_df_from_npz(obj.paths["consensus_usages"] % rep)
    assert spectra.shape == (70, G) and usages.shape == (N, 70)
    for a in (spectra.values, usages.values):
        assert np.isfinite(a).all() and a.min() >= 0
    kw = yaml.load(open(obj.paths["nmf_run_parameters"]), Loader=yaml.FullLoader)
    engine.set_matrix(X)
    with Wd.wide_limit(engine):
        W, _, _ = engine.mu_refit_f64(spectra.values.astype(np.float64), tol=kw["tol"], max_iter=kw["max_iter"], warn=False)
    assert np.abs(usages.values - W).max() <= 1e-9 * np.abs(W).max()
    assert engine.mu_rank_limit == 64


# ---------------------------------------------------------------- GPU 6: the other ways into the batch call
def _refit_f32(engine, ks, Hs, beta, max_iter):
    """cnmf_nmf_mu_batch with update_H = 0 (the float32 refit through the batch kernels: W starts at avg, H stays)."""
    import ctypes as C
    N = engine.shape[0]
    kk = np.asarray(ks, dtype=np.int32)
    h0 = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float32).ravel() for h in Hs]))
    avg = np.asarray([engine.init_scale(int(k)) for k in ks], dtype=np.float64)
    prm = _lib.CdParams(0.0, max_iter, 0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    Wf = np.zeros(int(kk.sum()) * N, dtype=np.float32)
    n_it, er = np.zeros(len(ks), dtype=np.int32), np.zeros(len(ks), dtype=np.float64)
    f32p, i32p, dblp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    engine._sync_env()
    engine._check(engine._lib.cnmf_nmf_mu_batch(engine._ctx, len(ks), kk.ctypes.data_as(i32p), 0, None, avg.ctypes.data_as(dblp), None,
                                                h0.ctypes.data_as(f32p), beta, 0, C.byref(prm), None, Wf.ctypes.data_as(f32p),
                                                n_it.ctypes.data_as(i32p), er.ctypes.data_as(dblp)))
    offs = np.concatenate([[0], np.cumsum(kk)]) * N
    return [Wf[offs[r]:offs[r + 1]].reshape(N, int(kk[r])) for r in range(len(ks))], n_it, er


@gpu
@pytest.mark.parametrize("mname,beta", [("A", 1), ("A+", 0)])
def test_wide_update_H_0_through_the_batch_kernels(wide, monkeypatch, mname, beta):
    """The float32 refit with H fixed at ranks 100 and 65 next to rank 9: 20 iterations from avg against the float64 refit
    of the same problem (the same iteration in float64), W.H within the end-of-run bar of the seeded runs above (2e-3
    Kullback-Leibler, 5e-3 Itakura-Saito, relative to the maximum); and each restart alone gives the same bits."""
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    X = R.matrix(mname)
    wide.set_matrix(X)
    rs = np.random.RandomState(17)
    ks = [100, 9, 65]
    Hs = [(np.abs(rs.standard_normal((k, X.shape[1]))) + 0.01).astype(np.float32) for k in ks]
    Ws, n_it, er = _refit_f32(wide, ks, Hs, beta, 20)
    assert list(n_it) == [20, 20, 20] and np.isfinite(er).all()
    for r, k in enumerate(ks):
        W1, n1, e1 = _refit_f32(wide, [k], [Hs[r]], beta, 20)
        assert W1[0].tobytes() == Ws[r].tobytes() and n1[0] == 20 and e1[0] == er[r]
        H64 = Hs[r].astype(np.float64)
        W64, it, err = wide.mu_refit_f64(H64, beta_loss=IS if beta == 0 else "kullback-leibler", tol=0.0, max_iter=20, warn=False)
        P, P_ref = Ws[r].astype(np.float64) @ H64, W64 @ H64
        print("update_H=0 %s rank %d: max |WH - WH_ref| / max WH_ref = %.3e, err %.6e vs %.6e" % (
            mname, k, np.abs(P - P_ref).max() / np.abs(P_ref).max(), er[r], err))
        assert it == 20 and np.abs(P - P_ref).max() <= (2e-3 if beta else 5e-3) * np.abs(P_ref).max()
        assert abs(er[r] - err) <= 2e-3 * err                      # (test_gpu_mu.py's bar on err)


@gpu
def test_wide_batch_from_the_init_store(wide):
    """init_mode 2 at ranks 70 and 65: the batch started from the engine's init store equals, bit for bit, the batch started
    from the same factors handed over as W0 / H0."""
    wide.set_matrix(R.matrix("A"))
    ks, seeds = [70, 65], [7, 8]
    assert wide.nndsvd_init_batch(ks, seeds, tail="device", variant="nndsvda", keep=True) is None
    order = list(wide.last_init_store_order)
    got = wide.init_store_fetch()
    H_a, W_a, n_a, e_a = wide.nmf_mu_batch(ks, init_store=True, max_iter=10, return_W=True, warn=False)
    H_b, W_b, n_b, e_b = wide.nmf_mu_batch([ks[r] for r in order], W0=[w for w, _ in got], H0=[h for _, h in got],
                                           max_iter=10, return_W=True, warn=False)
    for i, r in enumerate(order):
        np.testing.assert_array_equal(H_a[r], H_b[i])
        np.testing.assert_array_equal(W_a[r], W_b[i])
        assert n_a[r] == n_b[i] and e_a[r] == e_b[i]
