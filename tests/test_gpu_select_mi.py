"""Preprocess.select_features_MI on the device against what the UNMODIFIED reference computed with sklearn
(tests/golden/ref_select_mi.npz, tools/make_golden_select_mi.py; the counts are regenerated here from its seeds), the noise
stream against numpy from arbitrary RandomState states, a full-size check against sklearn's _compute_mi_cd, and
determinism, a shared engine and the hand-off to normalize_batchcorrect."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import synth
from cnmf_amd.engine import Engine
from cnmf_amd.preprocess import Preprocess, mi_classes
from tests._mi_ref import assert_state_equal, host_noise

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "ref_select_mi.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def inputs(gold):
    """tools/make_golden_select_mi.py's make_inputs"""
    n, g, k, mu, sg, seed = gold["params"].tolist()
    C, H = synth.topic_counts(int(n), int(g), int(k), mu_lib=mu, sigma_lib=sg, seed=int(seed))
    C = C.astype(np.float64)
    labels = np.argmax(C @ H.T.astype(np.float64), axis=1).astype(np.int64)
    start = int(n) - int(gold["tiny"].sum())
    for c, size in enumerate(gold["tiny"].tolist()):
        labels[start:start + size] = 100 + c
        start += size
    assert np.array_equal(labels, gold["labels"])
    return C, ["c%d" % i for i in range(int(n))], ["g%d" % j for j in range(int(g))], labels


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as e:
        yield e


def state_of(gold, prefix):
    return ("MT19937", gold[prefix + "_key"], int(gold[prefix + "_pos"]), int(gold[prefix + "_has_gauss"]),
            float(gold[prefix + "_gauss"]))


def run_fixture(tag, gold, inputs, engine):
    C, cells, genes, labels = inputs
    seeds = gold["seeds"].tolist()
    if tag == "a":
        P = Preprocess(random_seed=seeds[0], engine=engine)
        res = P.select_features_MI(C.copy(), labels, makeplots=False)
        norm_q, mv = .9999, None
    else:
        P = Preprocess(random_seed=seeds[1], engine=engine)
        np.random.randint(0, 1000, size=seeds[2])
        np.random.standard_normal(1)
        assert_state_equal(np.random.get_state(), state_of(gold, "b_before"))
        res = P.select_features_MI((sp.csr_matrix(C), cells, genes), np.array(["L%d" % v for v in labels]),
                                   max_scaled_thresh=5.0, quantile_thresh=None, n_top_features=20, makeplots=False)
        norm_q, mv = None, 5.0
    return res, norm_q, mv


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_reference(tag, gold, inputs, engine):
    C = inputs[0]
    res, q, mv = run_fixture(tag, gold, inputs, engine)
    assert_state_equal(np.random.get_state(), state_of(gold, tag + "_after"))
    mi, ref = res.var["MI"].values, gold[tag + "_MI"]
    same = mi.view(np.uint64) == ref.view(np.uint64)
    # the device's log() in the noise may differ from the host's by one ulp (the existing RNG's known-answer test allows
    # it), and a noise value one ulp away can move one neighbour count of a gene
    assert same.mean() >= 0.99
    assert np.abs(mi - ref).max() <= 1e-5
    for col in ("MI_Rank", "highly_variable"):
        np.testing.assert_array_equal(res.var[col].values, gold["%s_%s" % (tag, col)])
    order = np.argsort(-ref, kind="stable")
    d_ok = np.zeros_like(same)
    d_ok[order[1:]] = same[order[1:]] & same[order[:-1]]
    np.testing.assert_array_equal(res.var["MI_diff"].values[d_ok], gold[tag + "_MI_diff"][d_ok])
    assert res.var["highly_variable"].dtype == bool and list(res.var.index) == list(res.var_names)
    if tag == "b":
        assert list(res.var.index) == list(inputs[2])
    # X = min(normalised / std, thresh), in the input's sparsity
    rs = C.sum(axis=1)
    norm = C * np.where(rs > 0, gold[tag + "_target"] / np.where(rs > 0, rs, 1.0), 0.0)[:, None]
    y = norm / gold[tag + "_std"]
    if mv is not None:
        y[y > mv] = mv
    X = res.X.toarray() if sp.issparse(res.X) else res.X
    assert sp.issparse(res.X) == (tag == "b")
    assert np.array_equal(np.minimum(y, gold[tag + "_thresh"]), X)


# ---------------------------------------------------------------- the noise stream from arbitrary states
@pytest.mark.parametrize("pos", [0, 1, 623, 624])
@pytest.mark.parametrize("cached", [False, True])
def test_noise_stream_from_any_state(pos, cached, engine):
    rs = np.random.RandomState(pos + 7)
    st = rs.get_state()
    st = (st[0], st[1], pos, int(cached), 0.375 if cached else 0.0)
    n = 5 * 624 + 3
    got, fin = engine.debug_mt_normals(st, n)
    ref_rs = np.random.RandomState()
    ref_rs.set_state(st)
    want = ref_rs.standard_normal(n)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert (got.view(np.uint64) == want.view(np.uint64)).mean() > 0.5
    assert_state_equal(fin, ref_rs.get_state())


# ---------------------------------------------------------------- full size against sklearn's _compute_mi_cd
def test_full_size_against_sklearn(engine):
    from scipy.special import digamma
    from sklearn.feature_selection._mutual_info import _compute_mi_cd
    N, G = 50000, 256
    rs = np.random.RandomState(11)
    X = rs.poisson(rs.gamma(0.4, 2.0, size=G), size=(N, G)).astype(np.float64)
    labels = rs.randint(0, 15, size=N)
    labels[:26] = np.repeat(100 + np.arange(6), [1, 2, 3, 5, 7, 8])
    state = np.random.RandomState(4).get_state()
    psi = digamma(np.arange(N + 1, dtype=np.float64))
    psi[0] = 0.0
    picks = [0, 1, 37, 100, 128, 200, 254, 255]
    for K in (3, 5):
        cls, n_cls, cst = mi_classes(labels, K)
        engine.preprocess_set_dense(0, X)
        try:
            mi, fin = engine.preprocess_select_mi(0, cls, n_cls, K, state, psi, cst)
        finally:
            engine.preprocess_release()
        Xn, want_state = host_noise(X, state)
        assert_state_equal(fin, want_state)
        ref = np.array([max(0, _compute_mi_cd(Xn[:, j], labels, K)) for j in picks], dtype=np.float64)
        same = mi[picks].view(np.uint64) == ref.view(np.uint64)
        print("K", K, "bit-equal", same.sum(), "of", len(picks), "max diff", np.abs(mi[picks] - ref).max())
        assert same.sum() >= len(picks) - 1 and np.abs(mi[picks] - ref).max() <= 1e-5, (K, mi[picks], ref)


# ---------------------------------------------------------------- dense / CSR, determinism, shared engine, hand-off
def test_dense_csr_determinism_shared_engine_and_handoff(inputs):
    C, cells, genes, labels = inputs
    with Engine(0) as eng:
        Xr = np.random.RandomState(2).rand(300, 40).astype(np.float32)
        eng.set_matrix(Xr)
        before = eng.get_matrix().copy() if hasattr(eng, "get_matrix") else None
        outs = []
        for data in (pd.DataFrame(C, index=cells, columns=genes), (sp.csr_matrix(C), cells, genes)):
            P = Preprocess(random_seed=5, engine=eng)
            r = P.select_features_MI(data, pd.Series(labels, index=cells), makeplots=False)
            outs.append((r, np.random.get_state()))
        P = Preprocess(random_seed=5, engine=eng)
        again = P.select_features_MI((sp.csr_matrix(C), cells, genes), labels, makeplots=False)
        for r, st in outs[1:]:
            assert np.array_equal(r.var["MI"].values.view(np.uint64), outs[0][0].var["MI"].values.view(np.uint64))
            assert_state_equal(st, outs[0][1])
        assert np.array_equal(again.var["MI"].values.view(np.uint64), outs[0][0].var["MI"].values.view(np.uint64))
        assert np.array_equal(outs[1][0].X.toarray(), outs[0][0].X)
        if before is not None:
            assert np.array_equal(eng.get_matrix(), before)
        hv = outs[0][0].var["highly_variable"]
        a, hv_a = Preprocess(engine=eng).normalize_batchcorrect((sp.csr_matrix(C), cells, genes), highly_variable=hv.values,
                                                                makeplots=False)
        b, hv_b = Preprocess(engine=eng).normalize_batchcorrect((sp.csr_matrix(C), cells, genes),
                                                                highly_variable=list(hv.index[hv.values]), makeplots=False)
        assert hv_a == hv_b and len(hv_a) == 70
        assert np.array_equal(a.X.toarray(), b.X.toarray())
