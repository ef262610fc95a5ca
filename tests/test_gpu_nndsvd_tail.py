"""The device tail of init='nndsvd' (Engine.nndsvd_init_batch(tail="device"): start blocks, range finder, one-sided Jacobi
SVD, flip, split, threshold -- cnmf_nndsvd_group) against its float64 / long-double numpy restatement
(tests/_nndsvd_tail_ref.py) fed by numpy's draws and ``Engine.range_finder``; the hand-over to the solvers through the init
store (init_mode 2); the fallback on a block of rank below k; the route through ``cNMF``.

Bound of the parity test, per entry: |dev - ref| <= 2^-23 |ref| + 16 d -- the one rounding of the output to float32, and d
= the largest distance between the restatement's float64 and long-double runs on that input (the rounding error of the
float64 arithmetic itself, measured; convention of tests/_harmony_ref.py).  Entries whose un-thresholded value lies within
1e-6 relative of eps may fall on either side of the threshold and are left out (at most 0.1 % of the entries)."""
import warnings

import numpy as np
import pytest

from cnmf_amd.engine import Engine, _nndsvd_fill
from tests._nndsvd_tail_ref import tail_ref

pytestmark = pytest.mark.gpu

EPS = 1e-6
# name: (shape, ranks, seeds); the matrix is the generator of tests/test_host_nndsvd.py at the first seed
CASES = {
    "300x60_k5": ((300, 60), [5], [3]),
    "60x300_k4": ((60, 300), [4], [11]),                  # transpose
    "200x200_k7": ((200, 200), [7], [42]),
    "90x40_k6": ((90, 40), [6], [0]),
    "1100x257_k1_k2": ((1100, 257), [1, 2], [1, 2]),      # c = 11 and 12 in one group; k = 1: no split loop
    "700x300_k118": ((700, 300), [118], [5]),             # c = 128, the widest block
    "150x260_k9": ((150, 260), [9], [7]),                 # transpose
    "333x129_k22_k23": ((333, 129), [22, 23], [8, 9]),    # even and odd c in one group, L off every multiple of 64
}
_REF = {}


def make_x(shape, seed):
    rs = np.random.RandomState(seed + 100)
    return rs.gamma(0.6, 1.0, shape) * (rs.uniform(size=shape) < 0.7)


def load_case(engine, name):
    """The matrix of the case resident on the engine; the reference (computed once per case): per restart the float64 and
    long-double restatements on numpy's start blocks sent through ``Engine.range_finder`` in the device tail's grouping."""
    shape, ks, seeds = CASES[name]
    X = make_x(shape, seeds[0])
    engine.set_matrix(X)
    if name not in _REF:
        N, G = shape
        transpose = N < G
        M_cols = N if transpose else G
        n_rand = [k + 10 for k in ks]
        n_iters = [7 if k < 0.1 * min(N, G) else 4 for k in ks]
        ref = [None] * len(ks)
        for grp in Engine._nndsvd_groups(ks, n_rand, n_iters, 256):
            Qs = [np.random.RandomState(seeds[r]).normal(size=(M_cols, n_rand[r])) for r in grp]
            Qd, Bd = engine.range_finder(Qs, n_iters[grp[0]], transpose)
            for r, Q, B in zip(grp, Qd, Bd):
                W64, H64, i64 = tail_ref(ks[r], Q, B, transpose, EPS, np.float64)
                Wld, Hld, ild = tail_ref(ks[r], Q, B, transpose, EPS, np.longdouble)
                d = max(float(np.abs(W64 - Wld).max()), float(np.abs(H64 - Hld).max()))
                ref[r] = dict(W64=W64, H64=H64, Wld=Wld, Hld=Hld, info=ild, d=d)
        _REF[name] = (X, ref)
    return X, ks, seeds, _REF[name][1]


def near_threshold(raw):
    return np.abs(np.asarray(raw, dtype=np.float64) - EPS) <= 1e-6 * EPS


def assert_close(dev, ref_ld, raw_ld, d, what):
    ref = np.asarray(ref_ld, dtype=np.float64)
    skip = near_threshold(raw_ld)
    assert skip.mean() <= 1e-3, (what, float(skip.mean()))
    err = np.abs(dev - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 16.0 * d
    worst = float((err / bound)[~skip].max())
    print("%s: d = %.3g, max |dev - ref| = %.3g, worst err / bound = %.3g, left out %d" % (what, d, float(err[~skip].max()), worst, int(skip.sum())))
    assert worst <= 1.0, (what, worst, d)


@pytest.mark.parametrize("name", list(CASES))
def test_device_tail_matches_the_restatement(engine, name):
    X, ks, seeds, ref = load_case(engine, name)
    for r, e in enumerate(ref):                      # the margins that make an entry-wise comparison meaningful
        i = e["info"]
        assert i["converged"], (name, r)
        assert i["split_margin"] >= 1e-5 and i["flip_margin"] >= 1e-5 and i["s_gap"] >= 1e-5, (name, r, i["split_margin"], i["flip_margin"], i["s_gap"])
    dev = engine.nndsvd_init_batch(ks, seeds, tail="device")
    assert engine.last_nndsvd_tail == "device"
    for r, ((W, H), e) in enumerate(zip(dev, ref)):
        assert W.shape == (X.shape[0], ks[r]) and H.shape == (ks[r], X.shape[1]) and W.dtype == np.float64
        assert (W >= 0).all() and (H >= 0).all()
        assert np.array_equal(W, W.astype(np.float32)) and np.array_equal(H, H.astype(np.float32))    # float32 values
        assert_close(W, e["Wld"], e["info"]["W_raw"], e["d"], "%s W[%d]" % (name, r))
        assert_close(H, e["Hld"], e["info"]["H_raw"], e["d"], "%s H[%d]" % (name, r))


@pytest.mark.parametrize("name", ["300x60_k5", "60x300_k4", "333x129_k22_k23", "700x300_k118"])
def test_device_tail_same_bits(engine, name):
    _, ks, seeds, _ = load_case(engine, name)
    a = engine.nndsvd_init_batch(ks, seeds, tail="device")
    b = engine.nndsvd_init_batch(ks, seeds, tail="device")
    for (Wa, Ha), (Wb, Hb) in zip(a, b):
        np.testing.assert_array_equal(Wa, Wb)
        np.testing.assert_array_equal(Ha, Hb)


@pytest.mark.parametrize("name", ["300x60_k5", "60x300_k4", "1100x257_k1_k2", "333x129_k22_k23"])
def test_device_nndsvda_matches_the_host_variant(engine, name):
    """'nndsvda' on the device against the host fill applied to the restatement: the same zeros, filled with X.mean() up
    to the one float32 rounding; the other entries as in the parity test."""
    X, ks, seeds, ref = load_case(engine, name)
    dev = engine.nndsvd_init_batch(ks, seeds, tail="device", variant="nndsvda")
    assert engine.last_nndsvd_tail == "device"
    mean32 = float(np.float32(X.mean()))
    for r, ((W, H), e) in enumerate(zip(dev, ref)):
        for got, ref_ld, raw in ((W, e["Wld"], e["info"]["W_raw"]), (H, e["Hld"], e["info"]["H_raw"])):
            skip = near_threshold(raw)
            assert skip.mean() <= 1e-3
            zeros = np.asarray(ref_ld == 0)                      # (the leading pair of a positive matrix has none)
            filled = _nndsvd_fill(np.array(ref_ld, dtype=np.float64), np.zeros((1, 1)), "nndsvda", X.mean(), seeds[r])[0]
            assert np.array_equal((got == mean32)[~skip] | ~zeros[~skip], np.ones((~skip).sum(), dtype=bool))   # zeros filled
            assert (np.abs(got - filled)[zeros & ~skip] <= 2.0 ** -23 * filled[zeros & ~skip]).all()
            # no entry that is not a zero of the reference was filled (a kept value equals float32(mean) only by accident)
            keep = ~zeros & ~skip
            assert (np.abs(got - filled)[keep] <= 2.0 ** -23 * np.abs(filled[keep]) + 16.0 * e["d"]).all()


@pytest.mark.parametrize("name", ["300x60_k5", "60x300_k4", "1100x257_k1_k2", "333x129_k22_k23"])
def test_device_nndsvdar_matches_the_host_variant(engine, name):
    """'nndsvdar' on the device against the host fill (numpy's draws of a fresh RandomState(seed), row-major over W, then H)
    applied to the restatement: the same zeros, the filled values up to the one float32 rounding.  A restart with an entry
    at the threshold is left out: one flipped zero shifts every later draw."""
    X, ks, seeds, ref = load_case(engine, name)
    dev = engine.nndsvd_init_batch(ks, seeds, tail="device", variant="nndsvdar")
    assert engine.last_nndsvd_tail == "device"
    host = engine.nndsvd_init_batch(ks, seeds, tail="host", variant="nndsvdar")
    compared = 0
    for r, ((W, H), e) in enumerate(zip(dev, ref)):
        if near_threshold(e["info"]["W_raw"]).any() or near_threshold(e["info"]["H_raw"]).any():
            continue
        compared += 1
        Wz, Hz = np.asarray(e["Wld"] == 0), np.asarray(e["Hld"] == 0)
        Wf, Hf = _nndsvd_fill(np.array(e["Wld"], dtype=np.float64), np.array(e["Hld"], dtype=np.float64), "nndsvdar",
                              X.mean(), seeds[r])
        assert (W > 0).all() and (H > 0).all()
        for got, filled, zeros in ((W, Wf, Wz), (H, Hf, Hz)):
            assert (np.abs(got - filled)[zeros] <= 2.0 ** -23 * filled[zeros]).all()
            assert (np.abs(got - filled)[~zeros] <= 2.0 ** -23 * np.abs(filled[~zeros]) + 16.0 * e["d"]).all()
        # and the host route of the engine fills the same zeros with the same draws
        assert np.array_equal(host[r][0] == 0, np.zeros_like(Wz)) and np.abs(host[r][0] - W)[Wz].max(initial=0) <= 1e-6 * X.mean()
    assert compared >= 1


def test_device_tail_refuses_what_it_does_not_implement(engine):
    load_case(engine, "300x60_k5")
    with pytest.raises(TypeError):
        engine.nndsvd_init_batch([5], [np.random.RandomState(3)], tail="device")
    with pytest.raises(ValueError):
        engine.nndsvd_init_batch([5], [3], tail="gpu")
    with pytest.raises(ValueError):
        engine.nndsvd_init_batch([5], [3], tail="device", variant="nndsvdx")


@pytest.mark.parametrize("name,ks", [("300x60_k5", [3, 7, 5, 5]), ("1100x257_k1_k2", [9, 2, 4])])
def test_batch_from_the_init_store_equals_batch_from_fetched_factors(engine, name, ks):
    """init_mode 2 (no transfer) against init_mode 0 fed with the factors fetched from the same store: bit for bit."""
    load_case(engine, name)
    seeds = [50 + i for i in range(len(ks))]
    assert engine.nndsvd_init_batch(ks, seeds, tail="device", keep=True) is None
    order = list(engine.last_init_store_order)
    assert sorted(order) == list(range(len(ks)))
    got = engine.init_store_fetch()
    assert [w.shape[1] for w, _ in got] == [ks[r] for r in order]
    H_a, W_a, n_a, v_a = engine.nmf_batch(ks, init_store=True, max_iter=30, return_W=True, warn=False)
    ks_b = [ks[r] for r in order]
    H_b, W_b, n_b, v_b = engine.nmf_batch(ks_b, W0=[w for w, _ in got], H0=[h for _, h in got], max_iter=30,
                                          return_W=True, warn=False)
    for i, r in enumerate(order):
        np.testing.assert_array_equal(H_a[r], H_b[i])
        np.testing.assert_array_equal(W_a[r], W_b[i])
        assert n_a[r] == n_b[i] and v_a[r] == v_b[i]
    # and the kept factors are the ones the call returns without keep
    plain = engine.nndsvd_init_batch(ks, seeds, tail="device")
    for i, r in enumerate(order):
        np.testing.assert_array_equal(plain[r][0], got[i][0])
        np.testing.assert_array_equal(plain[r][1], got[i][1])


def test_mu_batch_from_the_init_store(engine):
    load_case(engine, "300x60_k5")
    ks, seeds = [4, 6, 3], [7, 8, 9]
    assert engine.nndsvd_init_batch(ks, seeds, tail="device", variant="nndsvda", keep=True) is None
    order = list(engine.last_init_store_order)
    got = engine.init_store_fetch()
    H_a, W_a, n_a, e_a = engine.nmf_mu_batch(ks, init_store=True, max_iter=30, return_W=True, warn=False)
    H_b, W_b, n_b, e_b = engine.nmf_mu_batch([ks[r] for r in order], W0=[w for w, _ in got], H0=[h for _, h in got],
                                             max_iter=30, return_W=True, warn=False)
    for i, r in enumerate(order):
        np.testing.assert_array_equal(H_a[r], H_b[i])
        np.testing.assert_array_equal(W_a[r], W_b[i])
        assert n_a[r] == n_b[i] and e_a[r] == e_b[i]


def test_init_store_must_hold_the_ranks_of_the_call(engine):
    load_case(engine, "300x60_k5")
    engine.init_store_reset()
    with pytest.raises(ValueError):
        engine.nmf_batch([5], init_store=True, max_iter=5, warn=False)
    with pytest.raises(ValueError):
        engine.nmf_mu_batch([5], init_store=True, max_iter=5, warn=False)
    engine.nndsvd_init_batch([5, 6], [1, 2], tail="device", keep=True)
    with pytest.raises(ValueError):
        engine.nmf_batch([5, 7], init_store=True, max_iter=5, warn=False)
    with pytest.raises(ValueError):
        engine.nmf_batch([5], init_store=True, max_iter=5, warn=False)
    engine.init_store_reset()


def test_rank_deficient_block_falls_back_to_the_host(engine):
    """A block of rank below k (12 x 200 of rank 5, k = 8): the device reports it and the whole call takes the host route."""
    rs = np.random.RandomState(5)
    X = rs.gamma(1.0, 1.0, size=(12, 5)) @ rs.gamma(1.0, 1.0, size=(5, 200))
    engine.set_matrix(X)
    ks, seeds = [8, 3], [7, 8]
    n_rand, n_iters = [k + 10 for k in ks], [7 if k < 0.1 * 12 else 4 for k in ks]
    status, _ = engine._nndsvd_device_tail(ks, seeds, Engine._nndsvd_groups(ks, n_rand, n_iters, 256), n_iters, True, "nndsvd", EPS)
    assert status[0] != 0 and status[1] == 0, status
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = engine.nndsvd_init_batch(ks, seeds, tail="host")
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning, match="host route"):
        dev = engine.nndsvd_init_batch(ks, seeds, tail="device", keep=True)
    assert engine.last_nndsvd_tail == "host_fallback" and dev is not None
    for (Wd, Hd), (Wh, Hh) in zip(dev, host):
        assert np.array_equal(Wd, Wh, equal_nan=True) and np.array_equal(Hd, Hh, equal_nan=True)
    with pytest.raises(ValueError):                  # the store was discarded
        engine.nmf_batch(ks, init_store=True, max_iter=5, warn=False)


def test_cnmf_route(engine, tmp_path):
    """cNMF.nndsvd = "device": factorize starts from the init store; the default stays the host route of the parent."""
    from cnmf_amd.cnmf import cNMF, load_df_from_npz
    X = make_x((300, 60), 3).astype(np.float32)
    X = X[X.sum(axis=1) > 0]
    spectra = {}
    for mode in ("device", "host"):
        obj = cNMF(output_dir=str(tmp_path), name="nn_" + mode, engine=engine)
        obj.nndsvd = mode
        obj.prepare_from_matrix(X, components=[3, 5], n_iter=2, seed=14, init="nndsvd", max_NMF_iter=40)
        engine.last_nndsvd_tail = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            obj.factorize()
        assert engine.last_nndsvd_tail == ("device" if mode == "device" else None)
        rp = load_df_from_npz(obj.paths["nmf_replicate_parameters"])
        ks, its = [int(v) for v in rp["n_components"].values], [int(v) for v in rp["iter"].values]
        seeds = [int(v) for v in rp["nmf_seed"].values]
        spectra[mode] = [obj.spectra_cache[(k, it)] for k, it in zip(ks, its)]
    engine.set_matrix(X)
    assert engine.nndsvd_init_batch(ks, seeds, tail="device", keep=True) is None
    H_dev = engine.nmf_batch(ks, init_store=True, max_iter=40, warn=False)[0]
    inits = engine.nndsvd_init_batch(ks, seeds, tail="host")
    H_host = engine.nmf_batch(ks, W0=[w for w, _ in inits], H0=[h for _, h in inits], max_iter=40, warn=False)[0]
    for r in range(len(ks)):
        np.testing.assert_array_equal(spectra["device"][r], H_dev[r])
        np.testing.assert_array_equal(spectra["host"][r], H_host[r])
    # a single restart through the call site
    obj.nndsvd = "device"
    engine.last_nndsvd_tail = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        H1, W1 = obj._nmf(X, dict(n_components=3, init="nndsvda", random_state=5, solver="cd", beta_loss="frobenius", max_iter=20))
    assert engine.last_nndsvd_tail == "device" and H1.shape == (3, X.shape[1]) and np.isfinite(H1).all()
