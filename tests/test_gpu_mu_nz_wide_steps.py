"""Single Kullback-Leibler multiplicative-update iterations on the NON-ZEROS of the matrix at ranks 33..64 (padded rank 64,
two lanes per row, ``Engine.mu_sparse_rank_limit = 64``) against the float64 oracle.  The protocol is that of
tests/test_gpu_mu_steps.py: the device, the float64 oracle (oracle/nmf_mu.py) and its float32 restatement start from the
SAME float32 factors (nmf_cd.random_init on the float32 matrix, handed over as W0= / H0=) and run t = 1, 2, 3 iterations
with tol = 0; no matching, no normalisation.

  d_W, d_H = _mu_steps_ref.dist_W / dist_H, d_e = |err - e64| / e64.

The bar: every device distance <= 16 x Y (_cd_steps_ref.FACTOR).  Y belongs to a cell (quantity, t) at padded rank 64 and is
pooled (maximum) over every restart of every case (_mu_nz_wide_ref.CASES): the float32 restatement's own distance from the
oracle, the definition of the ``nz`` path of _mu_steps_ref.py.  Exact: n_iter == t, factors finite and >= 0, and on the
planted cases ``dead`` and ``xzero`` the same entries exactly zero as in the oracle.

Cases: A (517 x 500: genes in one block of 512, the in-kernel finish; cells in two blocks, the second of 5 rows, the
finish kernel) at ranks 33, 37, ..., 61, 64 -- every live-quad count 9..16, nine restarts -- with no and with the mixed
penalty; P (1301 x 1100, 8.5 % non-zero: three blocks on both sides, the last of 76 genes / 277 cells) at 33, 40,
64, once chosen by density and once forced, equal bit for bit; T (45 x 70: the cells fill less than one 64-row slice, its
second pass of 32 holds 13 rows; the genes one slice and 6 rows of a second, whose second pass holds no row; more
components than cells) at 33 and 64; L (1061 x 300, up to 300 entries a row and block) at 40.  Planted at rank 40:
component 22 of W0 dead (a component of the second lane half), one all-zero cell and one all-zero gene (rows without an
entry), and three gene columns of H0 so small that S sits around eps.  Every call carries three filler restarts of ranks
9, 24 and 70 behind the compared ones (the last under ``mu_rank_limit = 128``): non-zero groups at padded ranks 16 / 32 /
64 and a dense group at 128 in one call.

The CPU tests (not marked gpu) hold the inputs and references to what they claim.

Measured on an MI355X: device distance / yardstick per quantity, the worst over t and over the cases (the bar is 16; no
defect was found).  The 10 GPU tests take 4 s together.
  ratio  worst entry: yardstick vs device
  d_W    1.42  NA none t=1 rank 45: 7.275e-07 vs 1.031e-06
  d_H    0.69  NA mixed t=2 rank 57: 2.126e-06 vs 1.476e-06
  d_e    0.15  NT none t=2 rank 33: 2.353e-07 vs 3.514e-08
Per matrix the worst d_W / d_H / d_e ratios: A 1.42 / 0.69 / 0.14, P 0.53 / 0.24 / 0.10, T 0.51 / 0.25 / 0.15, L 0.94 /
0.46 / 0.11; planted dead 1.12 / 0.62 / 0.10, xzero 1.18 / 0.51 / 0.11, tiny at most 1.06; the planted zeros came out
exact, and P chosen by density equals P forced bit for bit.
"""
import numpy as np
import pytest

from tests import _mu_nz_wide_ref as Nz
from tests import _mu_steps_ref as R
from tests._mu_wide_ref import wide_limit

gpu = pytest.mark.gpu


@pytest.fixture
def nzwide(engine):
    assert engine.mu_sparse_rank_limit == 32
    with Nz.nz_wide_limit(engine):
        assert engine.mu_sparse_rank_limit == 64
        yield engine
    assert engine.mu_sparse_rank_limit == 32


def check_within(label, y, d, failures):
    print("%s: yardstick %.3e, device vs float64 %.3e (%.2f x)" % (label, y, d, d / y if y else np.inf if d else 0.0))
    if not d <= R.FACTOR * y:
        failures.append((label, d, y))


def compare(label, case, t, H, W, n_iter, err, failures):
    """Every restart of ``case`` (the order the device was given them) at iteration t; the case's worst device distance
    per quantity meets the cell's bar."""
    plant = case[3]
    runs = Nz.reference(*case)
    worst = {}
    for i, r in sorted(runs.items()):
        w, h = np.asarray(W[i]), np.asarray(H[i])
        assert w.shape == r["W"][t].shape and h.shape == r["H"][t].shape
        if n_iter[i] != t:
            failures.append((label, t, "n_iter", i, int(n_iter[i])))
        if not (np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0 and np.isfinite(err[i])):
            failures.append((label, t, "not finite or negative", i, r["k"]))
            continue
        if plant in Nz.EXACT_ZERO_PLANTS and not (np.array_equal(w == 0, r["W"][t] == 0) and np.array_equal(h == 0, r["H"][t] == 0)):
            failures.append((label, t, "exact zeros differ", i, r["k"], int(((w == 0) != (r["W"][t] == 0)).sum()),
                             int(((h == 0) != (r["H"][t] == 0)).sum())))
        for what, d in (("W", R.dist_W(w, r["W"][t])), ("H", R.dist_H(h, r["H"][t])), ("e", R.d_err(err[i], r["e"][t]))):
            if not d <= worst.get(what, (-1.0, 0))[0]:                    # (a NaN distance is kept: it fails the bar)
                worst[what] = (d, i)
    for what, (d, i) in sorted(worst.items()):
        check_within("%s t=%d d_%s (restart %d, rank %d)" % (label, t, what, i, runs[i]["k"]), Nz.yardstick(what, t), d, failures)


def run_case(engine, monkeypatch, case, forced=True):
    """The case's restarts and the three fillers in one call per t.  Returns what the device gave, per t."""
    bname, loss, regname, plant = case
    label = "nz-wide %s %s%s%s" % (bname, regname, " planted " + plant if plant else "", "" if forced else " by density")
    if forced:
        monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    else:
        monkeypatch.delenv("CNMF_MU_SPARSE", raising=False)
    mname = Nz.batch(bname)[0]
    engine.set_matrix(R.matrix(mname))
    n = len(Nz.batch(bname)[1])
    ks = list(Nz.batch(bname)[1]) + list(Nz.FILL_RANKS)                   # the fillers behind: the compared indices stay
    st = list(Nz.inits(bname, plant)) + list(Nz.fill_inits(mname))
    failures, out = [], {}
    for t in R.TS:
        with wide_limit(engine):                                          # (the rank-70 filler)
            H, W, n_iter, err = engine.nmf_mu_batch(ks, W0=[s[0] for s in st], H0=[s[1] for s in st], beta_loss=R.BETA_NAMES[loss],
                                                    tol=0.0, max_iter=t, return_W=True, warn=False, **R.REGS[regname])
        assert len(H) == len(ks) and (np.asarray(n_iter) == t).all()
        assert engine.matrix_images()["non_zero_images_64"]
        compare(label, case, t, H, W, n_iter, err, failures)
        out[t] = ([np.array(h) for h in H[:n]], [np.array(w) for w in W[:n]], list(err[:n]))
    assert not failures, failures
    return out


# ---------------------------------------------------------------- CPU: the inputs and the references
def test_the_inputs_hold_what_they_claim():
    assert Nz.batch("NA")[:2] == ("A", (33, 37, 41, 45, 49, 53, 57, 61, 64)) and len(Nz.batch("NA")[1]) % 2 == 1
    assert sorted({(k + 3) // 4 for k in Nz.batch("NA")[1]}) == list(range(9, 17))          # every live-quad count
    assert sorted({((k + 3) // 4 + 1) // 2 for k in Nz.batch("NA")[1]}) == [5, 6, 7, 8]     # every body of the kernel
    assert Nz.batch("NP")[:2] == ("P", (33, 40, 64)) and Nz.batch("NT")[:2] == ("T", (33, 64))
    assert Nz.batch("NL")[:2] == ("L", (40,)) and Nz.batch("NE")[:2] == ("A", (40,)) and Nz.batch("NEz")[:2] == ("Az", (40,))
    assert Nz.FILL_RANKS == (9, 24, 70)
    for b in Nz.BATCHES:
        assert all(32 < k <= 64 for k in Nz.batch(b)[1])
        assert len(set(Nz.batch(b)[2])) == len(Nz.batch(b)[1])
    # blocks of the other side at BS = 512
    assert Nz.BS == 512
    A, P, T, L = (R.matrix(m) for m in "APTL")
    assert A.shape == (517, 500) and (500 + 511) // 512 == 1 and (517 + 511) // 512 == 2 and 517 - 512 == 5
    assert P.shape == (1301, 1100) and (1100 + 511) // 512 == 3 and 1100 - 1024 == 76 and (1301 + 511) // 512 == 3 and 1301 - 1024 == 277
    assert (P != 0).mean() < 0.15                                         # (where padded rank 64 switches by itself)
    assert T.shape == (45, 70) and 45 < 64 and 70 > 64 and 70 - 64 < 32 and min(Nz.batch("NT")[1]) > 32
    assert L.shape == (1061, 300) and int((L != 0).sum(axis=1).max()) > 250
    # the plants
    assert Nz.DEAD_COMPONENT < 40 and Nz.lane_half(Nz.DEAD_COMPONENT) == 1 and Nz.DEAD_COMPONENT // 4 < (40 + 3) // 4
    (W0, H0), (Wc, Hc) = Nz.inits("NE", "dead")[0], Nz.inits("NE")[0]
    assert (W0[:, Nz.DEAD_COMPONENT] == 0).all() and (np.delete(W0, Nz.DEAD_COMPONENT, axis=1) > 0).all() and np.array_equal(H0, Hc)
    Az = R.matrix("Az")
    assert (Az[R.ZERO_CELL] == 0).all() and (Az[:, R.ZERO_GENE] == 0).all()
    assert ((Az != 0).sum(axis=1) == 0).sum() == 1 and ((Az != 0).sum(axis=0) == 0).sum() == 1
    assert all(np.array_equal(a, b) for a, b in zip(Nz.inits("NEz", "xzero")[0], Nz.inits("NEz")[0]))
    (W0, H0) = Nz.inits("NE", "tiny")[0]
    S = (W0.astype(np.float64) @ H0.astype(np.float64)) / float(R.EPS)
    genes = sorted(R.TINY_GENES)
    assert np.array_equal(W0, Wc) and np.array_equal(np.delete(H0, genes, axis=1), np.delete(Hc, genes, axis=1))
    assert 0.03 < S[:, genes].min() and S[:, genes].max() < 30 and (H0 > 0).all()
    assert (S[:, genes] < 1).sum() > 500 and (S[:, genes] > 1).sum() > 500
    assert np.delete(S, genes, axis=1).min() > 1e3
    assert (A[:, genes] != 0).sum() > 100                                 # (the clamp decides quotients of stored entries)
    for m in "APTL":
        assert [f[0].shape[1] for f in Nz.fill_inits(m)] == list(Nz.FILL_RANKS)


@pytest.mark.parametrize("case", Nz.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_references_are_finite_and_the_planted_zeros_are_there(case):
    """The oracle and its float32 restatement finite and >= 0, every restart's own yardsticks finite and > 0 for the factors,
    no component dead in the oracle but the planted one, the planted rows and columns exactly zero."""
    plant = case[3]
    runs = Nz.reference(*case)
    assert sorted(runs) == list(range(len(Nz.batch(case[0])[1])))
    for i, r in runs.items():
        for t in R.TS:
            W, H = r["W"][t], r["H"][t]
            assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0 and r["e"][t] > 0
            y = r["y32"][t]
            assert all(np.isfinite(y[q]) for q in "WHe"), (i, t, y)
            assert y["W"] > 0 and y["H"] > 0
            dead_W, dead_H = (W.max(axis=0) == 0), (H.max(axis=1) == 0)
            if plant == "dead":
                assert list(np.flatnonzero(dead_W)) == [Nz.DEAD_COMPONENT] and list(np.flatnonzero(dead_H)) == [Nz.DEAD_COMPONENT]
            else:
                assert not dead_W.any() and not dead_H.any()
            if plant == "xzero":
                assert (W[R.ZERO_CELL] == 0).all() and (H[:, R.ZERO_GENE] == 0).all()


def test_the_yardsticks_are_positive():
    for what in "WHe":
        ys = [Nz.yardstick(what, t) for t in R.TS]
        print("nz-wide d_%s: %s" % (what, " ".join("%.3e" % y for y in ys)))
        assert min(ys) > 0 and np.isfinite(ys).all()


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_nz_wide_on_A_in_a_mixed_call(nzwide, monkeypatch, regname):
    """Nine restarts of every live-quad count 9..16 with the fillers: four kernel groups in one call."""
    run_case(nzwide, monkeypatch, ("NA", "kl", regname, None))


@gpu
def test_nz_wide_on_P_by_density_and_forced(nzwide, monkeypatch):
    """Three blocks on both sides, the last short.  Under 15 % non-zero the library takes the path by itself, and
    gives the bits of the forced run."""
    auto = run_case(nzwide, monkeypatch, ("NP", "kl", "none", None), forced=False)
    forced = run_case(nzwide, monkeypatch, ("NP", "kl", "none", None), forced=True)
    for t in R.TS:
        for a, b in zip(auto[t][0] + auto[t][1], forced[t][0] + forced[t][1]):
            np.testing.assert_array_equal(a, b)
        assert auto[t][2] == forced[t][2]


@gpu
@pytest.mark.parametrize("bname", ["NT", "NL"])
def test_nz_wide_small_and_long(nzwide, monkeypatch, bname):
    """T: one slice on either side, 45 cells (the second pass of 32 holds 13 rows), 70 genes (a second slice of 6 rows: no
    row in its second pass), more components than cells.  L: up to 300 entries per row and block."""
    run_case(nzwide, monkeypatch, (bname, "kl", "none", None))


@gpu
@pytest.mark.parametrize("plant", Nz.PLANTS)
def test_nz_wide_planted_edges(nzwide, monkeypatch, plant):
    """Rank 40, Kullback-Leibler.  dead: component 22 of W0 (second lane half) is zero -- its H row becomes exactly 0 at
    t = 1 and the W column stays 0.  xzero: a cell and a gene without a stored entry.  tiny: S = W0.H0 around eps in three
    gene columns, max(S, eps) decides those quotients at t = 1."""
    run_case(nzwide, monkeypatch, (Nz.PLANT_BATCH[plant], "kl", "none", plant))
