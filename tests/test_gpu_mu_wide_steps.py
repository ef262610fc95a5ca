"""Single multiplicative-update iterations at ranks 65..128 (padded rank 128, ``Engine.mu_rank_limit = 128``) against the
float64 oracle.  The protocol is that of tests/test_gpu_mu_steps.py: the device, the float64 oracle (oracle/nmf_mu.py) and
both restatements start from the SAME float32 factors (nmf_cd.random_init on the float32 matrix, handed over as W0= /
H0=) and run t = 1, 2, 3 iterations with tol = 0; no matching, no normalisation.

  d_W, d_H = _mu_steps_ref.dist_W / dist_H, d_e = |err - e64| / e64.

The bar: every device distance <= 16 x Y (_cd_steps_ref.FACTOR).  Y belongs to a cell (loss, quantity, t) at padded rank
128 and is pooled (maximum) over every restart of every case of that loss (_mu_wide_ref.CASES): the larger of the float32
restatement's and the plane restatement's own distance from the oracle.  Exact: n_iter == t, factors finite and >= 0, and
on the planted cases the same entries exactly zero as in the oracle.

Cases: Kullback-Leibler on A (517 x 500) at ranks 65, 80, 96, 127, 128, 128, 65 with no and with the mixed penalty, in ONE
call together with two rank-9 and one rank-40 restart (three kernel groups in a call, seven workgroup layers in the wide
one); Itakura-Saito on A + 1e-3 at 65, 96, 128; T (45 x 70: below one block and one 32-row tile on every side, more
components than cells or genes) at 65 and 128, T + 1e-3 at 65; L (1061 x 300: N_pad = 1280, empty row chunks) at 80.
Planted at rank 70 on A: component 66 of W0 dead (the second component half of the workgroup), and three gene columns of H0
so small that S sits around eps.

The CPU tests (not marked gpu) hold the inputs and references to what they claim.

Measured on an MI355X: device distance / yardstick per cell, the worst over t and over the cases (the bar is 16; no defect
was found).  The 11 GPU tests take 3 s together.
  loss       ratio  worst entry: yardstick vs device
  kl   d_W    1.06  T none t=3 rank 128: 4.590e-06 vs 4.867e-06
  kl   d_H    1.11  T none t=2 rank 128: 3.345e-06 vs 3.706e-06
  kl   d_e    0.54  T none t=3 rank 65: 1.870e-07 vs 1.002e-07
  is   d_W    1.80  T+ none t=2 rank 65: 1.102e-06 vs 1.981e-06
  is   d_H    1.31  T+ none t=3 rank 65: 1.595e-06 vs 2.096e-06
  is   d_e    0.90  T+ none t=3 rank 65: 4.127e-08 vs 3.732e-08
On A and L every ratio is 0.2 ... 1.2 x; the planted zeros came out exact, the planted clamp case sits at 0.56 x at worst.
"""
import numpy as np
import pytest

from tests import _mu_steps_ref as R
from tests import _mu_wide_ref as Wd

gpu = pytest.mark.gpu


@pytest.fixture
def wide(engine):
    with Wd.wide_limit(engine):
        yield engine
    assert engine.mu_rank_limit == 64


def check_within(label, y, d, failures):
    print("%s: yardstick %.3e, device vs float64 %.3e (%.2f x)" % (label, y, d, d / y if y else np.inf if d else 0.0))
    if not d <= R.FACTOR * y:
        failures.append((label, d, y))


def compare(label, case, t, H, W, n_iter, err, failures):
    """Every restart of ``case`` (the order the device was given them) at iteration t; the case's worst device distance
    per quantity meets the cell's bar."""
    bname, loss, regname, plant = case
    runs = Wd.reference(*case)
    worst = {}
    for i, r in sorted(runs.items()):
        w, h = np.asarray(W[i]), np.asarray(H[i])
        assert w.shape == r["W"][t].shape and h.shape == r["H"][t].shape
        if n_iter[i] != t:
            failures.append((label, t, "n_iter", i, int(n_iter[i])))
        if not (np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0 and np.isfinite(err[i])):
            failures.append((label, t, "not finite or negative", i, r["k"]))
            continue
        if plant is not None and not (np.array_equal(w == 0, r["W"][t] == 0) and np.array_equal(h == 0, r["H"][t] == 0)):
            failures.append((label, t, "exact zeros differ", i, r["k"], int(((w == 0) != (r["W"][t] == 0)).sum()),
                             int(((h == 0) != (r["H"][t] == 0)).sum())))
        for what, d in (("W", R.dist_W(w, r["W"][t])), ("H", R.dist_H(h, r["H"][t])), ("e", R.d_err(err[i], r["e"][t]))):
            if not d <= worst.get(what, (-1.0, 0))[0]:                    # (a NaN distance is kept: it fails the bar)
                worst[what] = (d, i)
    for what, (d, i) in sorted(worst.items()):
        check_within("%s t=%d d_%s (restart %d, rank %d)" % (label, t, what, i, runs[i]["k"]),
                     Wd.yardstick(loss, what, t), d, failures)


def run_case(engine, monkeypatch, case, fill=False):
    bname, loss, regname, plant = case
    label = "wide %s %s %s%s" % (bname, loss, regname, " planted " + plant if plant else "")
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    engine.set_matrix(R.matrix(Wd.batch(bname)[0]))
    ks, st = list(Wd.batch(bname)[1]), list(Wd.inits(bname, plant))
    if fill:                                              # behind the compared restarts: their indices stay
        ks += list(Wd.batch("FILL")[1])
        st += list(Wd.inits("FILL"))
    failures = []
    for t in R.TS:
        H, W, n_iter, err = engine.nmf_mu_batch(ks, W0=[s[0] for s in st], H0=[s[1] for s in st], beta_loss=R.BETA_NAMES[loss],
                                                tol=0.0, max_iter=t, return_W=True, warn=False, **R.REGS[regname])
        assert len(H) == len(ks) and (np.asarray(n_iter) == t).all()
        compare(label, case, t, H, W, n_iter, err, failures)
    assert not failures, failures


# ---------------------------------------------------------------- CPU: the inputs and the references
def test_the_inputs_hold_what_they_claim():
    assert Wd.batch("WA")[1] == (65, 80, 96, 127, 128, 128, 65) and Wd.batch("WA")[0] == "A" and len(Wd.batch("WA")[1]) % 2 == 1
    assert Wd.batch("WI") [:2] == ("A+", (65, 96, 128)) and Wd.batch("WT")[:2] == ("T", (65, 128))
    assert Wd.batch("WT+")[:2] == ("T+", (65,)) and Wd.batch("WL")[:2] == ("L", (80,)) and Wd.batch("WE")[:2] == ("A", (70,))
    assert Wd.batch("FILL")[1] == (9, 9, 40)
    for b in Wd.BATCHES:
        if b != "FILL":
            assert all(64 < k <= 128 for k in Wd.batch(b)[1])
        assert len(set(Wd.batch(b)[2])) == len(Wd.batch(b)[1])
    assert R.matrix("T").shape == (45, 70) and R.matrix("L").shape == (1061, 300) and (1061 + 255) // 256 * 256 == 1280
    assert 64 <= Wd.DEAD_COMPONENT < 70
    (W0, H0), (Wc, Hc) = Wd.inits("WE", "dead")[0], Wd.inits("WE")[0]
    assert (W0[:, Wd.DEAD_COMPONENT] == 0).all() and (np.delete(W0, Wd.DEAD_COMPONENT, axis=1) > 0).all() and np.array_equal(H0, Hc)
    (W0, H0) = Wd.inits("WE", "tiny")[0]
    S = (W0.astype(np.float64) @ H0.astype(np.float64)) / float(R.EPS)
    genes = sorted(R.TINY_GENES)
    assert np.array_equal(W0, Wc) and np.array_equal(np.delete(H0, genes, axis=1), np.delete(Hc, genes, axis=1))
    assert 0.03 < S[:, genes].min() and S[:, genes].max() < 30 and (H0 > 0).all()
    assert (S[:, genes] < 1).sum() > 500 and (S[:, genes] > 1).sum() > 500
    assert np.delete(S, genes, axis=1).min() > 1e3


@pytest.mark.parametrize("case", Wd.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_references_are_finite_and_the_planted_zeros_are_there(case):
    """The oracle and both restatements finite and >= 0, every restart's own yardsticks finite and > 0 for the factors, no
    component dead in the oracle but the planted one, and no entry of an unplanted run near the flush-to-zero edge."""
    plant = case[3]
    runs = Wd.reference(*case)
    assert sorted(runs) == list(range(len(Wd.batch(case[0])[1])))
    for i, r in runs.items():
        for t in R.TS:
            W, H = r["W"][t], r["H"][t]
            assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0 and r["e"][t] > 0
            for y in (r["y32"][t], r["ypl"][t]):
                assert all(np.isfinite(y[q]) for q in "WHe"), (i, t, y)
                assert y["W"] > 0 and y["H"] > 0
            dead_W, dead_H = (W.max(axis=0) == 0), (H.max(axis=1) == 0)
            if plant == "dead":
                assert list(np.flatnonzero(dead_W)) == [Wd.DEAD_COMPONENT] and list(np.flatnonzero(dead_H)) == [Wd.DEAD_COMPONENT]
            else:
                assert not dead_W.any() and not dead_H.any()
            if plant is None:
                print("%s restart %d t=%d: smallest entry %.3e" % (case, i, t, min(W.min(), H.min())))
                # the flush rule acts below float64 eps = 2.2e-16; a relative error of 1e-4 could not carry these across it
                assert min(W.min(), H.min()) > 1e-12


@pytest.mark.parametrize("loss", ["kl", "is"])
def test_the_yardsticks_are_positive(loss):
    for what in "WHe":
        ys = [Wd.yardstick(loss, what, t) for t in R.TS]
        print("wide %s d_%s: %s" % (loss, what, " ".join("%.3e" % y for y in ys)))
        assert min(ys) > 0 and np.isfinite(ys).all()


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_wide_kl_on_A_in_a_mixed_call(wide, monkeypatch, regname):
    """Seven wide restarts (an odd count) and three of padded ranks 16 and 64 in one call."""
    run_case(wide, monkeypatch, ("WA", "kl", regname, None), fill=True)


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_wide_is_on_A(wide, monkeypatch, regname):
    """Itakura-Saito on A + 1e-3: both ratios through their own accumulators, both component halves."""
    run_case(wide, monkeypatch, ("WI", "is", regname, None))


@gpu
@pytest.mark.parametrize("bname,loss", [("WT", "kl"), ("WT+", "is"), ("WL", "kl")])
def test_wide_small_and_long(wide, monkeypatch, bname, loss):
    """T: below one 128-cell block and one 32-row tile on every side.  L: N_pad = 1280, row chunks without a tile."""
    run_case(wide, monkeypatch, (bname, loss, "none", None))


@gpu
@pytest.mark.parametrize("plant", Wd.PLANTS)
def test_wide_planted_edges(wide, monkeypatch, plant):
    """Rank 70 on A, Kullback-Leibler.  dead: component 66 of W0 is zero -- its H row becomes exactly 0 at t = 1 and the W
    column stays 0.  tiny: S = W0.H0 around eps in three gene columns, max(S, eps) decides those quotients at t = 1."""
    run_case(wide, monkeypatch, ("WE", "kl", "none", plant))
