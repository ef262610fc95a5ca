"""Single multiplicative-update iterations of the device against the float64 oracle, on every kernel family.

The end-of-run tests (test_gpu_mu.py, test_gpu_mu_sparse.py, test_gpu_mu_refill.py, test_gpu_kl_tail.py,
test_gpu_is_tail.py) compare after 12 to 400 iterations; multiplicative updates contract towards a fixed point, so a lost
lo plane, a dropped 32-row tile or a partial numerator that is never added ends within their 1e-3 / 2e-3 bars.  Here the
device, the float64 oracle (oracle/nmf_mu.py) and the restatements start from the SAME float32 factors
(nmf_cd.random_init on the float32 matrix, handed over as W0= / H0=) and run t = 1, 2, 3 iterations with tol = 0.  No
matching and no normalisation: the component order is the same on all sides.

  d_W, d_H = _cd_steps_ref.d_cols / d_rows (a component that is all zero in the oracle is compared for equality instead),
  d_e = |err - e64| / e64 with e64 = nmf_mu.beta_divergence(X, W64_t, H64_t, beta, square_root=True).

The bar: every device distance <= 16 x Y (_cd_steps_ref.FACTOR).  Y belongs to a cell (path, loss, padded rank, quantity,
t) and is pooled (maximum) over every restart of that padded rank in every case the path is compared on
(_mu_steps_ref.CASES: all matrices, penalties and planted cases; the two losses are different kernel instantiations and
keep separate cells).  Vector-ALU (CNMF_MU_VALU=1, padded ranks 8 / 16 / 32 / 64) and non-zero path (CNMF_MU_SPARSE=1 or
chosen by density; 16 / 32): Y = the distance of the float32 restatement (nmf_mu.fit_mu on float32 X, W0, H0) from the
oracle.  Matrix pipe (CNMF_MU_SPARSE=0; 16 / 32 / 64): Y = the larger of that and the distance of the plane restatement
(_mu_steps_ref.model_fit: fit_mu in float64 with only the roundings the kernel header declares: factors and quotients as
bf16 hi + lo planes, S and the updated factors as float32).  d_e is held to the same restatements' own d_e (float32
sums; S from the split planes).  Exact: n_iter == t, factors finite and >= 0, and on the planted cases the same entries
exactly zero as in the oracle.  (A first version pooled per test case only; there the two-restart cases on T leave one
restart per cell, d_e is ONE signed rounding error per restart, and the vector-ALU Itakura-Saito cell of rank 9 on T +
1e-3 drew a yardstick of 5.0e-10 against a device d_e of 2.9e-08 -- half a float32 ulp -- 57 x.  Pooled over the cell as
defined above that yardstick is 6.6e-08.)

Data (_mu_steps_ref.matrix): A = 517 x 500 (517 % 32 = 5: N_pad = 768 = 24 one-tile cell chunks, seven past the data;
500 % 32 = 20), T = 45 x 70 (below one slice, one block, one vector-ALU chunk), L = 1061 x 300 (N_pad = 1280: 32 chunks of
two tiles, twelve of them empty; two 1024-blocks on the non-zero path at padded rank 32), P = 1301 x 1100 sparse counts
(8.5 % non-zero: the library takes the non-zero path by itself; two blocks on both half-steps at padded rank 32, one at
16); Itakura-Saito on A + 1e-3 and T + 1e-3.  Batch M on A = ranks 1..16 twice + 1, 16 (34 restarts of padded rank 16: a
second round of MU_MAXSLOTS = 32 slots, every position of a 4-restart workgroup) + 17, 20, 24, 31, 32 + 33, 40, 48, 63,
64.  Planted edges (Kullback-Leibler, ranks 5 and 20, every path): a dead component in W0; exact zeros and 1e-30 entries
in H0; an all-zero cell and an all-zero gene in X; and, at ranks 5, 9 and 20, three gene columns of H0 so small that
S = W0.H0 lies around eps there ("tiny": the only inputs on which max(S, eps) acts where X is not zero).

The CPU tests (not marked gpu) hold the inputs, the bf16 split and the oracle's snapshots to what they claim and show
that the bar has teeth (seven mutants of the plane restatement).

Measured on an MI355X: device distance / yardstick per cell, the worst over t and over the cases of the path (the bar is
16; no defect was found).  The 31 GPU tests take 15 s together, 6 s of them the float64 references of batch M.
  path  loss       pad:    8    16    32    64  worst entry: yardstick vs device
  mfma  kl   d_W           -  1.01  1.00  1.13  T none t=1 rank 33: 2.477e-06 vs 2.787e-06
  mfma  kl   d_H           -  1.00  1.07  1.04  T none t=2 rank 17: 4.322e-06 vs 4.608e-06
  mfma  kl   d_e           -  1.05  0.92  1.13  T none t=1 rank 33: 2.226e-07 vs 2.508e-07
  mfma  is   d_W           -  1.07  1.23  1.13  I mixed t=3 rank 17: 1.490e-06 vs 1.837e-06
  mfma  is   d_H           -  1.08  1.12  1.18  I mixed t=2 rank 40: 1.558e-06 vs 1.835e-06
  mfma  is   d_e           -  0.99  0.53  0.92  T+ none t=3 rank 1: 6.161e-08 vs 6.106e-08
  nz    kl   d_W           -  1.87  1.67     -  M mixed t=1 rank 16: 5.482e-07 vs 1.027e-06
  nz    kl   d_H           -  2.27  0.87     -  M none t=1 rank 1: 1.344e-06 vs 3.046e-06
  nz    kl   d_e           -  0.22  0.23     -  M mixed t=1 rank 17: 1.842e-07 vs 4.307e-08
  valu  kl   d_W        0.49  0.54  0.53  0.64  V none t=1 rank 33: 4.547e-07 vs 2.904e-07
  valu  kl   d_H        0.53  0.31  0.30  0.29  V mixed t=1 rank 1: 8.411e-07 vs 4.460e-07
  valu  kl   d_e        0.52  0.26  0.16  0.17  V none t=1 rank 1: 1.664e-07 vs 8.650e-08
  valu  is   d_W        1.13  0.49  0.54  0.62  V+ none t=2 rank 1: 4.920e-07 vs 5.570e-07
  valu  is   d_H        1.07  0.53  0.48  0.56  V+ none t=2 rank 1: 5.951e-07 vs 6.394e-07
  valu  is   d_e        0.49  0.51  0.62  0.51  V+ none t=3 rank 32: 4.689e-08 vs 2.912e-08
The largest figure anywhere is 2.27 x (d_H of a rank-1 restart on the non-zero path at t = 1).  The matrix pipe sits at
1.0 ... 1.2 x the plane restatement: its error IS the declared 2^-17 of the planes, 2 to 10 times the float32 yardstick.
Forced and chosen non-zero runs on P: equal bit for bit; CNMF_SP_ORDER=0 on A: other bits, the same ratios to two digits.
The planted zeros came out exact on all three paths; the planted clamp case sits at 0.81 x (matrix pipe), 1.28 x (non-zero
path) and 0.49 x (vector-ALU) at worst.

The mutants of test_the_bar_has_teeth, in the best quantity of each restart of ranks 5, 9, 20 (the bar is 16):
(a) 277 ... 448 x, (b) 55 ... 119 x, Itakura-Saito (b) 56 ... 123 x, (c) 39 000 ... 77 000 x, (d) 35 000 ... 62 000 x,
(f) 2400 ... 4200 x, (g) 3300 ... 10 100 x in d_e under the mixed penalty (with no penalty 0.6 ... 1.0 x: there a
Kullback-Leibler H half-step leaves sum(WH) == sum(X) to rounding and the missing term is zero).
(e) 32 500 ... 88 900 x in d_H at t = 1 from the start factors of the planted case "tiny".  From random_init it lands at
0.6 ... 1.1 x: no product S comes near eps there, S + eps and max(S, eps) differ by a float32 rounding, and nothing told
the two clamps apart -- on the CPU or on the device.  That is why "tiny" was planted.
"""
import numpy as np
import pytest

from tests import _mu_steps_ref as R

gpu = pytest.mark.gpu

KNOBS = {"mfma": {"CNMF_MU_SPARSE": "0"}, "nz": {"CNMF_MU_SPARSE": "1"}, "valu": {"CNMF_MU_VALU": "1"}, "auto": {}}


# ---------------------------------------------------------------- comparison
def check_within(label, y, d, failures):
    """Print yardstick, device distance and their ratio; note a failure above the bar."""
    print("%s: yardstick %.3e, device vs float64 %.3e (%.2f x)" % (label, y, d, d / y if y else np.inf if d else 0.0))
    if not d <= R.FACTOR * y:
        failures.append((label, d, y))


def compare(label, path, case, t, H, W, n_iter, err, failures):
    """Every compared restart of ``case`` (R.members, the order the device was given them) at iteration t.  The yardstick
    of a cell is shared by its restarts, so the case's worst device distance per cell is what meets the bar."""
    bname, loss, regname, plant, _ = case
    runs = R.reference(bname, loss, regname, plant).runs
    worst = {}
    for j, i in enumerate(R.members(path, case)):
        r = runs[i]
        w, h = np.asarray(W[j]), np.asarray(H[j])
        assert w.shape == r["W"][t].shape and h.shape == r["H"][t].shape
        if n_iter[j] != t:
            failures.append((label, t, "n_iter", i, int(n_iter[j])))
        if not (np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0 and np.isfinite(err[j])):
            failures.append((label, t, "not finite or negative", i, r["k"]))
            continue
        if plant is not None and not (np.array_equal(w == 0, r["W"][t] == 0) and np.array_equal(h == 0, r["H"][t] == 0)):
            failures.append((label, t, "exact zeros differ", i, r["k"], int(((w == 0) != (r["W"][t] == 0)).sum()),
                             int(((h == 0) != (r["H"][t] == 0)).sum())))
        pad = R.PAD[path](r["k"])
        for what, d in (("W", R.dist_W(w, r["W"][t])), ("H", R.dist_H(h, r["H"][t])), ("e", R.d_err(err[j], r["e"][t]))):
            if not d <= worst.get((what, pad), (-1.0, 0))[0]:             # (a NaN distance is kept: it fails the bar)
                worst[(what, pad)] = (d, i)
    for (what, pad), (d, i) in sorted(worst.items()):
        check_within("%s t=%d d_%s pad %d (restart %d, rank %d)" % (label, t, what, pad, i, runs[i]["k"]),
                     R.yardstick(path, loss, what, t, pad), d, failures)


def device_steps(engine, case, t, only=None):
    bname, loss, regname, plant, _ = case
    _, ks, _ = R.batch(bname)
    st = R.inits(bname, plant)
    idx = range(len(ks)) if only is None else only
    return engine.nmf_mu_batch([ks[i] for i in idx], W0=[st[i][0] for i in idx], H0=[st[i][1] for i in idx],
                               beta_loss=R.BETA_NAMES[loss], tol=0.0, max_iter=t, return_W=True, warn=False,
                               **R.REGS[regname])


def run_case(engine, monkeypatch, path, bname, loss, regname, plant=None, max_rank=None, knobs=None, keep=None, tag=""):
    """``path``: the family whose cells the case belongs to (the case must be listed in R.CASES[path]); ``knobs``: the
    KNOBS entry to set (default: that of the path).  ``keep``: a dict that receives {t: device result}."""
    case = (bname, loss, regname, plant, max_rank)
    label = "%s%s %s %s %s%s" % (path, tag, bname, loss, regname, " planted " + plant if plant else "")
    for name, value in KNOBS[path if knobs is None else knobs].items():
        monkeypatch.setenv(name, value)
    engine.set_matrix(R.matrix(R.batch(bname)[0]))
    failures = []
    for t in R.TS:
        H, W, n_iter, err = device_steps(engine, case, t, R.members(path, case))
        if keep is not None:
            keep[t] = (H, W, n_iter, err)
        compare(label, path, case, t, H, W, n_iter, err, failures)
    assert not failures, failures


def same_bits(a, b):
    return (all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[0] + a[1], b[0] + b[1]))
            and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes())


# ---------------------------------------------------------------- CPU: the oracle's snapshots, the split, the inputs, the mutants
@pytest.mark.parametrize("loss", ["kl", "is"])
def test_oracle_snapshots_equal_separate_runs(loss):
    """``snapshots`` records what a run with max_iter = t returns, bit for bit, and leaves the run itself unchanged."""
    bname = "M" if loss == "kl" else "I"
    X = R.matrix(R.batch(bname)[0])
    i = R.batch(bname)[1].index(9)
    W0, H0 = (a.astype(np.float64) for a in R.inits(bname)[i])
    kw = dict(beta_loss=R.BETA_NAMES[loss], tol=0.0, **R.REGS["mixed"])
    snaps = {1: None, 2: None, 3: None, 9: None}
    W3, H3, n3 = R.nmf_mu.nmf_mu(X, 9, W0=W0, H0=H0, max_iter=3, snapshots=snaps, **kw)
    assert n3 == 3 and snaps[9] is None
    Wp, Hp, _ = R.nmf_mu.nmf_mu(X, 9, W0=W0, H0=H0, max_iter=3, **kw)
    assert Wp.tobytes() == W3.tobytes() and Hp.tobytes() == H3.tobytes()
    for t in (1, 2, 3):
        Wt, Ht, nt = R.nmf_mu.nmf_mu(X, 9, W0=W0, H0=H0, max_iter=t, **kw)
        assert nt == t and Wt.tobytes() == snaps[t][0].tobytes() and Ht.tobytes() == snaps[t][1].tobytes()
    ref = R.reference(bname, loss, "mixed").runs[i]
    assert ref["W"][3].tobytes() == W3.tobytes() and ref["H"][3].tobytes() == H3.tobytes()


@pytest.mark.parametrize("loss,regname", [("kl", "none"), ("kl", "mixed"), ("is", "mixed")])
def test_the_unmutated_model_is_the_oracle(loss, regname):
    """The copy of the oracle's loop that carries the planes and the mutants equals the oracle bit for bit when both are
    switched off, divergence included."""
    bname = "M" if loss == "kl" else "I"
    X = R.matrix(R.batch(bname)[0])
    for k in (9, 17):
        i = R.batch(bname)[1].index(k)
        W0, H0 = R.inits(bname)[i]
        got = R.model_fit(X, W0, H0, R.BETAS[loss], R.REGS[regname], use_planes=False)
        run = R.reference(bname, loss, regname).runs[i]
        for t in R.TS:
            assert got[t][0].tobytes() == run["W"][t].tobytes() and got[t][1].tobytes() == run["H"][t].tobytes()
            assert got[t][2] == run["e"][t]


def test_the_bf16_split():
    """hi + lo is within 2^-17 of |x|, both planes are bf16 values, zeros, subnormals and the float32 maximum stay finite."""
    rs = np.random.RandomState(3)
    fmax, tiny = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    x = np.concatenate([np.exp(rs.uniform(np.log(1e-30), np.log(1e30), 20000)) * rs.choice([-1.0, 1.0], 20000),
                        rs.standard_normal(20000), [1.0, 1.0 + 2.0**-8, 1.0 + 2.0**-7 + 2.0**-8, 3.0e38, fmax, -fmax]]
                       ).astype(np.float32)
    hi, lo = R.split_bf16(x)
    for p in (hi, lo):
        assert p.dtype == np.float32 and np.isfinite(p).all() and (p.view(np.uint32) & 0xFFFF == 0).all()
    x64 = x.astype(np.float64)
    assert (np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x64) <= 2.0**-17 * np.abs(x64)).all()
    assert np.array_equal(R.planes(x), hi.astype(np.float64) + lo.astype(np.float64))
    assert np.array_equal(R.planes(x, lo_plane=False), hi.astype(np.float64))
    # ties go to even: 1 + 2^-8 is half way between the bf16 neighbours 1 and 1 + 2^-7
    assert hi[40000] == 1.0 and hi[40001] == 1.0 and hi[40002] == np.float32(1.0 + 2.0**-6)
    edge = np.array([0.0, -0.0, tiny, -tiny, tiny / 2, 2.0**-149, -2.0**-149, fmax, -fmax], dtype=np.float32)
    eh, el = R.split_bf16(edge)
    assert np.isfinite(eh).all() and np.isfinite(el).all() and np.isfinite(R.planes(edge)).all()
    assert (eh[:2] == 0).all() and (el[:2] == 0).all()
    assert np.abs(R.planes(edge) - edge.astype(np.float64)).max() <= 2.0**-17 * float(fmax)


def test_the_inputs_hold_what_they_claim():
    A, T, L, P, Az = (R.matrix(n) for n in ("A", "T", "L", "P", "Az"))
    for X in (A, T, L, P, Az, R.matrix("A+"), R.matrix("T+")):
        assert X.dtype == np.float64 and np.array_equal(X, X.astype(np.float32).astype(np.float64)) and X.min() >= 0
    N, G = A.shape
    assert (N, G) == (517, 500) and N % 32 == N % 128 == 5 and G % 32 == 20 and G % 128 == 116
    assert (N + 255) // 256 * 256 == 768 and 768 // 32 == 24 and 24 - (N + 31) // 32 == 7 and R.CHUNK_D < (N + 31) // 32
    assert T.shape == (45, 70) and np.array_equal(T, A[:45, :70]) and max(1, 45 // 64) == 1
    assert L.shape == (1061, 300) and (1061 + 255) // 256 * 256 == 1280 and 1280 // 32 == 40 and 2 * 20 == 40
    assert 300 % 32 == 12 and 1061 > 1024
    for X in (A, T, L):                                   # no zero row or column: planted below, where wanted
        assert (X != 0).mean() > 0.25 and (X.sum(axis=0) > 0).all() and (X.sum(axis=1) > 0).all()
    n, g = P.shape
    print("P: %d x %d, %.1f %% non-zero" % (n, g, 100 * (P != 0).mean()))
    assert 1025 <= n <= 2047 and 1025 <= g <= 2047 and n % 32 and g % 32 and (P != 0).mean() < 0.25
    assert (P.sum(axis=0) > 0).all() and (P.sum(axis=1) > 0).all()
    assert R.matrix("A+").min() > 0 and R.matrix("T+").min() > 0
    assert (Az[R.ZERO_CELL] == 0).all() and (Az[:, R.ZERO_GENE] == 0).all() and (Az != A).sum() < N + G
    ks = R.batch("M")[1]
    assert len(ks) == 44 == len(set(R.batch("M")[2]))
    assert [sum(R.pad_mfma(k) == p for k in ks) for p in (16, 32, 64)] == [34, 5, 5] and 34 > 32 and 34 % 4 == 2
    assert R.batch("I")[1] == (3, 9, 16, 17, 24, 40, 64)
    assert R.batch("C")[1] == (5, 9, 20)
    for plant, bname in R.PLANT_BATCH.items():
        for (W0, H0), (Wc, Hc) in zip(R.inits(bname, plant), R.inits(bname)):
            if plant == "dead":
                assert (W0[:, 1] == 0).all() and (np.delete(W0, 1, axis=1) > 0).all() and np.array_equal(H0, Hc)
            elif plant == "hplant":
                assert np.array_equal(W0, Wc)
                assert 0.05 < (H0 == 0).mean() < 0.12 and 0.05 < (H0 == np.float32(1e-30)).mean() < 0.12
            elif plant == "tiny":
                # S = W0.H0 around eps in three gene columns, on both sides of it, where most of X is not zero
                S = (W0.astype(np.float64) @ H0.astype(np.float64)) / float(R.EPS)
                genes = sorted(R.TINY_GENES)
                assert np.array_equal(W0, Wc) and np.array_equal(np.delete(H0, genes, axis=1), np.delete(Hc, genes, axis=1))
                assert 0.03 < S[:, genes].min() and S[:, genes].max() < 30 and (H0 > 0).all()
                assert (S[:, genes] < 1).sum() > 500 and (S[:, genes] > 1).sum() > 500 and (A[:, genes] > 0).mean() > 0.6
                assert np.delete(S, genes, axis=1).min() > 1e3
            else:
                assert np.array_equal(W0, Wc) and np.array_equal(H0, Hc)


ALL_CASES = sorted({c[:4] for cs in R.CASES.values() for c in cs}, key=str)


@pytest.mark.parametrize("bname,loss,regname,plant", ALL_CASES)
def test_the_references_are_finite_and_the_planted_zeros_are_there(bname, loss, regname, plant):
    """Every reference a GPU test below uses: the oracle and both restatements finite and >= 0 (the dtypes are asserted
    inside run_triple), every restart's own yardsticks > 0, and the planted zeros where they are planted -- in the oracle
    AND in both restatements (their dist_W / dist_H are finite only then)."""
    ref = R.reference(bname, loss, regname, plant)
    assert sorted(ref.runs) == list(range(len(R.batch(bname)[1])))                # no restart is left out
    for i, r in ref.runs.items():
        for t in R.TS:
            W, H = r["W"][t], r["H"][t]
            assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0 and r["e"][t] > 0
            for y in (r["y32"][t], r["ypl"][t]):
                assert all(np.isfinite(y[q]) for q in "WHe"), (i, t, y)
            assert r["y32"][t]["W"] > 0 and r["y32"][t]["H"] > 0 and r["ypl"][t]["W"] > 0 and r["ypl"][t]["H"] > 0
            dead_W, dead_H = (W.max(axis=0) == 0), (H.max(axis=1) == 0)
            if plant == "dead":
                assert list(np.flatnonzero(dead_W)) == [1] and list(np.flatnonzero(dead_H)) == [1]
            else:
                assert not dead_W.any() and not dead_H.any()
            if plant == "hplant":
                H0 = R.inits(bname, plant)[i][1]
                assert np.array_equal(H == 0, (H0 == 0) | (H0 == np.float32(1e-30)))
            if plant == "xzero":
                assert np.array_equal(W == 0, np.broadcast_to((np.arange(W.shape[0]) == R.ZERO_CELL)[:, None], W.shape))
                assert np.array_equal(H == 0, np.broadcast_to(np.arange(H.shape[1]) == R.ZERO_GENE, H.shape))
            if plant is None:
                assert (W > 0).all() and (H > 0).all()


@pytest.mark.parametrize("path", list(R.CASES))
def test_the_yardsticks_are_positive(path):
    """Every cell (path, loss, padded rank, quantity, t) has a yardstick > 0, and every padded rank of the path occurs."""
    cells = R.cells(path)
    pads = {"mfma": {16, 32, 64}, "nz": {16, 32}, "valu": {8, 16, 32, 64}}[path]
    assert {p for l, p in cells if l == "kl"} == pads and (path == "nz" or {p for l, p in cells if l == "is"} == pads)
    for loss, pad in cells:
        for what in "WHe":
            ys = [R.yardstick(path, loss, what, t, pad) for t in R.TS]
            print("%s %s pad %d d_%s: %s" % (path, loss, pad, what, " ".join("%.3e" % y for y in ys)))
            assert min(ys) > 0


@pytest.mark.parametrize("mutant", ["a", "b", "b-is", "c", "d", "e", "f", "g"])
def test_the_bar_has_teeth(mutant):
    """Every restart of ranks 5, 9, 20 (batch M on A; "b-is": batch B+ on A + 1e-3, Itakura-Saito, the lo plane of 1 / S),
    run through a mutant of the plane restatement, lands above 16 x the matrix-pipe yardstick of its cell in d_W, d_H or
    d_e at some t <= 3.  (e) runs from the start factors of the planted case "tiny" (batch C, the same three ranks on A): from
    random_init no product S comes near eps = 1.2e-7, S + eps differs from max(S, eps) by a relative 1e-7 / S per quotient
    -- a float32 rounding -- and the mutant lands at 0.6 ... 1.1 x (measured on batch M); no bar that the honest arithmetic
    passes can tell the two clamps apart there.  That was a hole in the inputs, not only in the mutant: nothing exercised
    the device's clamp at an entry where X is not zero.  "tiny" does, on all three paths (test_planted_edges)."""
    bname, loss, plant = ("B+", "is", None) if mutant == "b-is" else ("C", "kl", "tiny") if mutant == "e" else ("M", "kl", None)
    # (g) under the mixed penalty: without one a Kullback-Leibler H half-step leaves sum(WH) == sum(X) to rounding, the
    # missing term is 1e-3 of 2.4e5 and the mutant IS the oracle (measured with no penalty: 0.6 ... 1.0 x)
    regname = "mixed" if mutant == "g" else "none"
    X = R.matrix(R.batch(bname)[0])
    ref = R.reference(bname, loss, regname, plant)
    slipped = []
    for i, k in enumerate(R.batch(bname)[1]):
        if k not in (5, 9, 20):
            continue
        W0, H0 = R.inits(bname, plant)[i]
        got = R.model_fit(X, W0, H0, R.BETAS[loss], R.REGS[regname], mutant=mutant[0])
        run, best = ref.runs[i], (0.0, None)
        for t in R.TS:
            for what, d in (("W", R.dist_W(got[t][0], run["W"][t])), ("H", R.dist_H(got[t][1], run["H"][t])),
                            ("e", R.d_err(got[t][2], run["e"][t]))):
                y = R.yardstick("mfma", loss, what, t, R.pad_mfma(k))
                if d / y > best[0]:
                    best = (d / y, (t, what, y, d))
        print("mutant %s rank %d restart %d: best %.1f x at t=%d d_%s (yardstick %.3e, mutant %.3e)" % (
            (mutant, k, i, best[0]) + best[1]))
        if not best[0] > R.FACTOR:
            slipped.append((mutant, k, i, best))
    assert not slipped, slipped


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_matrix_pipe_kl_batch_M(engine, monkeypatch, regname):
    """44 restarts on A, Kullback-Leibler: 34 of padded rank 16 (a second round of 32 slots: slots retired and explicit
    W0 / H0 installed into reused ones), 5 of 32, 5 of 64 (the last workgroup of two holds one)."""
    run_case(engine, monkeypatch, "mfma", "M", "kl", regname)


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_matrix_pipe_is(engine, monkeypatch, regname):
    """Itakura-Saito on A + 1e-3: the second ratio 1 / S through its own accumulators, gamma = 1/2, both flushes."""
    run_case(engine, monkeypatch, "mfma", "I", "is", regname)


@gpu
@pytest.mark.parametrize("bname,loss", [("T", "kl"), ("T+", "is"), ("L", "kl")])
def test_matrix_pipe_small_and_long(engine, monkeypatch, bname, loss):
    """T: below one 128-cell block and one 32-row tile of padding on every side.  L: N_pad = 1280, 32 chunks of two
    tiles of which twelve hold no tile at all."""
    run_case(engine, monkeypatch, "mfma", bname, loss, "none")


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_non_zero_path_forced_on_A(engine, monkeypatch, regname):
    """The 39 restarts of batch M up to rank 32 on the sliced-ELL image of a 76 % non-zero matrix."""
    run_case(engine, monkeypatch, "nz", "M", "kl", regname, max_rank=32)


@gpu
@pytest.mark.parametrize("bname", ["T", "Ln"])
def test_non_zero_path_forced_small_and_long(engine, monkeypatch, bname):
    """T: below one 64-row slice.  L: at padded rank 32 the H half-step's other side (1061 cells) needs two blocks."""
    run_case(engine, monkeypatch, "nz", bname, "kl", "none", max_rank=32 if bname == "T" else None)


@gpu
def test_non_zero_path_chosen_by_density_on_P(engine, monkeypatch):
    """P (8.5 % non-zero): the library takes the non-zero path by itself -- the same bits as forced, other bits than the
    matrix pipe -- and meets the float32 yardstick; two blocks on both half-steps at padded rank 32, one at 16."""
    chosen, forced, dense = {}, {}, {}
    run_case(engine, monkeypatch, "nz", "P", "kl", "none", knobs="auto", keep=chosen, tag="(auto)")
    run_case(engine, monkeypatch, "nz", "P", "kl", "none", keep=forced)
    run_case(engine, monkeypatch, "mfma", "P", "kl", "none", keep=dense)
    for t in R.TS:
        assert same_bits(chosen[t], forced[t]), t
        assert not same_bits(chosen[t], dense[t]), t


@gpu
def test_non_zero_path_in_storage_order(engine, monkeypatch):
    """CNMF_SP_ORDER=0 (the images keep every row's entries in storage order) meets the same bar as the default order."""
    default, storage = {}, {}
    run_case(engine, monkeypatch, "nz", "M", "kl", "none", max_rank=32, keep=default)
    monkeypatch.setenv("CNMF_SP_ORDER", "0")
    try:
        run_case(engine, monkeypatch, "nz", "M", "kl", "none", max_rank=32, keep=storage, tag="(order 0)")
    finally:
        monkeypatch.delenv("CNMF_SP_ORDER")
        engine.set_matrix(R.matrix("A"))              # (drops the images built in storage order)
    assert not same_bits(default[3], storage[3])      # (the knob reached the build: another order of every row's sum)


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
@pytest.mark.parametrize("bname,loss", [("V", "kl"), ("V+", "is")])
def test_vector_alu_on_A(engine, monkeypatch, bname, loss, regname):
    """Every padded rank of the vector-ALU kernels on both sides of its edge (1, 5, 8 | 9, 16 | 17, 32 | 33, 64)."""
    keep = {}
    run_case(engine, monkeypatch, "valu", bname, loss, regname, keep=keep)
    monkeypatch.delenv("CNMF_MU_VALU")
    monkeypatch.setenv("CNMF_MU_SPARSE", "0")
    other = device_steps(engine, (bname, loss, regname, None, None), 3)
    assert not same_bits(keep[3], other)              # (the knob chose other kernels)


@gpu
@pytest.mark.parametrize("bname,loss", [("VT", "kl"), ("VT+", "is")])
def test_vector_alu_on_T(engine, monkeypatch, bname, loss):
    """45 cells: the H half-step and the divergence run in one chunk."""
    run_case(engine, monkeypatch, "valu", bname, loss, "none")


@gpu
@pytest.mark.parametrize("plant", R.PLANTS)
@pytest.mark.parametrize("path", ["mfma", "nz", "valu"])
def test_planted_edges(engine, monkeypatch, path, plant):
    """Kullback-Leibler on A at ranks 5 and 20 with exact expectations from the float64 oracle.  dead: component 1 of W0
    is zero -- its H row becomes exactly 0 at t = 1 (the ``W_sum == 0 -> 1`` branch) and the W column stays 0 at t = 2, 3
    through ``den == 0 -> eps``.  hplant: exact zeros in H0 stay zero, entries of 1e-30 are flushed by the ``< float64
    eps -> 0`` rule.  xzero: an all-zero cell and an all-zero gene in X empty a row of W and a column of H.  tiny (ranks 5,
    9, 20): three gene columns of H0 so small that S = W0.H0 lies between 0.06 and 7 eps there: max(S, eps) decides the
    quotient of about 1300 non-zero entries of X at t = 1, and those genes' H entries grow by seven orders of magnitude."""
    run_case(engine, monkeypatch, path, R.PLANT_BATCH[plant], "kl", "none", plant=plant)
