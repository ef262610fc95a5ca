"""Single coordinate-descent iterations of the device against the float64 oracle, on every kernel path.

The end-of-run tests (test_gpu_nmf.py, test_gpu_sweep_ranks.py, test_gpu_edges.py) compare stationary points; CD pulls
a slightly wrong iteration back to the same one, so they cannot see a lost low plane of a GEMM operand or a violation sum
that misses a few rows.  Here the device, the float64 oracle (oracle/nmf_cd.py) and the oracle's float32 restatement start
from the SAME float32 factors (nmf_cd.random_init on the float32 matrix) and run t = 1, 2, 3 iterations with tol = 0.  No
matching and no normalisation: the component order is the same on all sides.

  d_W = max_c max_i |dW[i,c]| / max_i |W64[i,c]|,   d_H the same over the rows of H,   d_v = |viol - a_t / a_1|
  (a = the float64 oracle's violation trace; the device reports violation / violation_init).

The bar calibrates itself: every device distance <= 16 x Y, where Y is the float32 restatement's own distance from the
float64 oracle -- for W and H pooled (maximum) over the restarts of the batch in the same register tier (rank rounded up
to a multiple of 4 up to 32, then 48, 64, 128), for the violation ratio over the whole batch.  n_iter == t exactly, factors
finite and >= 0, viol == 1.0 exactly at t = 1.

Data: A = C1 truncated to 517 cells x 500 genes (517 % 16 = 517 % 64 = 517 % 256 = 5, 500 % 64 = 52, 500 % 128 = 116: a
partial last chunk, dead lanes, a last 16-cell block past the data; count-structured, gemm_mode 4), B = A made general
(gemm_mode 5).  Batch R = ranks 1..16 twice + 17, 20, 21, 24, 25, 28, 29, 32, 33, 47, 48, 49, 63, 64 (46 restarts, 772
packed columns: every exact-rank body of the W half-step, every padded tier of the H half-step on both sides of its
edge, and -- where the scheduler places them, R.first_fill -- slots across the 256 / 512 / 768 group edges).  Batch S =
[5, 128, 9, 70, 33, 96, 64, 65] (sweep_big_kernel beside the small tiers).  Regularisation: none, mixed (alpha_W 0.002, alpha_H 0.001, l1_ratio 0.3), l1 (l1_ratio 1), l2 (0).

The CPU tests (not marked gpu) hold the inputs to what they claim and show that the bar has teeth: four float64 mutants of
the oracle's loop must land above it.

Measured on an MI355X: device distance / yardstick, the worst over t per tier (the bar is 16; nothing needed the pooled
yardstick, and no defect was found).  "256" = kc_max 256 with CNMF_GEMM3 = g3, "wide" = 1024 packed columns.
  path               tier:    4    8   12   16   20   24   28   32   48   64  128  worst entry: restatement vs device
  R/A 256 g3=0 none      d_H 0.68 1.32 0.83 1.08 0.68 0.85 0.75 0.88 0.92 0.72    -  t=1: 2.93e-06 vs 3.86e-06
  R/A 256 g3=0 none      d_W 0.69 1.34 0.76 0.81 0.90 0.73 0.68 1.25 0.79 1.04    -  t=3: 3.29e-06 vs 4.40e-06
  R/A 256 g3=0 none      d_v (pooled over the batch)                                 0.58 x at t=2: 6.13e-07 vs 3.56e-07
  R/A 256 g3=0 mixed     d_H 0.77 0.83 0.68 0.97 0.88 0.83 0.56 0.88 0.88 1.28    -  t=2: 1.45e-05 vs 1.86e-05
  R/A 256 g3=0 mixed     d_W 0.80 0.95 0.72 0.72 0.89 1.09 0.74 1.08 0.75 0.77    -  t=2: 1.01e-05 vs 1.10e-05
  R/A 256 g3=0 mixed     d_v (pooled over the batch)                                 0.61 x at t=3: 8.06e-07 vs 4.92e-07
  R/A 256 g3=1 none      d_H 0.67 0.79 0.61 0.70 0.59 0.85 0.56 1.02 0.65 0.69    -  t=1: 7.00e-06 vs 7.14e-06
  R/A 256 g3=1 none      d_W 0.63 0.60 0.73 0.72 0.55 0.58 0.69 0.84 0.84 0.74    -  t=1: 9.78e-06 vs 8.24e-06
  R/A 256 g3=1 none      d_v (pooled over the batch)                                 1.49 x at t=3: 9.67e-07 vs 1.44e-06
  R/A 256 g3=1 mixed     d_H 0.62 1.03 0.75 0.88 0.92 0.77 0.51 0.90 0.71 0.61    -  t=3: 3.80e-06 vs 3.90e-06
  R/A 256 g3=1 mixed     d_W 0.68 0.74 0.80 0.55 0.47 0.58 0.57 0.78 1.14 0.56    -  t=3: 1.27e-05 vs 1.45e-05
  R/A 256 g3=1 mixed     d_v (pooled over the batch)                                 4.07 x at t=3: 8.06e-07 vs 3.28e-06
  R/A 256 g3=2 none      d_H 0.35 0.50 0.51 0.64 0.60 0.66 0.50 0.63 0.51 0.63    -  t=3: 1.43e-05 vs 9.39e-06
  R/A 256 g3=2 none      d_W 0.44 0.61 0.57 0.44 0.60 0.70 0.54 1.18 0.78 0.85    -  t=3: 8.37e-06 vs 9.91e-06
  R/A 256 g3=2 none      d_v (pooled over the batch)                                 0.36 x at t=2: 6.13e-07 vs 2.20e-07
  R/A 256 g3=2 mixed     d_H 0.34 0.50 0.60 0.48 0.59 0.81 0.45 0.55 0.75 0.44    -  t=3: 1.35e-05 vs 1.09e-05
  R/A 256 g3=2 mixed     d_W 0.51 0.48 0.59 0.46 0.45 0.84 0.49 0.67 0.74 0.44    -  t=3: 1.57e-05 vs 1.31e-05
  R/A 256 g3=2 mixed     d_v (pooled over the batch)                                 0.32 x at t=3: 8.06e-07 vs 2.58e-07
  R/A 256 g3=3 none      d_H 0.40 0.73 0.45 0.59 0.53 0.53 0.45 0.81 0.81 0.56    -  t=1: 7.00e-06 vs 5.65e-06
  R/A 256 g3=3 none      d_W 0.47 0.68 0.39 0.40 0.83 0.59 0.56 0.80 0.78 0.73    -  t=3: 7.39e-06 vs 6.17e-06
  R/A 256 g3=3 none      d_v (pooled over the batch)                                 0.39 x at t=2: 6.13e-07 vs 2.39e-07
  R/A 256 g3=3 mixed     d_H 0.68 0.54 0.73 0.71 0.72 0.59 0.49 0.91 0.74 0.54    -  t=2: 7.58e-06 vs 6.87e-06
  R/A 256 g3=3 mixed     d_W 0.49 0.89 0.68 0.53 0.99 0.45 0.51 0.69 1.10 0.62    -  t=3: 1.27e-05 vs 1.40e-05
  R/A 256 g3=3 mixed     d_v (pooled over the batch)                                 4.05 x at t=3: 8.06e-07 vs 3.26e-06
  R/A 256 g3=4 none      d_H 0.34 0.52 0.50 0.52 0.45 0.42 0.52 0.78 0.61 0.68    -  t=1: 7.00e-06 vs 5.45e-06
  R/A 256 g3=4 none      d_W 0.60 0.50 0.39 0.40 0.52 0.42 0.53 1.10 0.76 1.00    -  t=3: 8.37e-06 vs 9.23e-06
  R/A 256 g3=4 none      d_v (pooled over the batch)                                 0.33 x at t=3: 9.67e-07 vs 3.19e-07
  R/A 256 g3=4 mixed     d_H 0.44 0.88 0.52 0.54 0.53 0.53 0.43 0.70 0.62 0.71    -  t=3: 3.80e-06 vs 3.35e-06
  R/A 256 g3=4 mixed     d_W 0.58 0.61 0.47 0.59 0.90 0.45 0.58 0.98 0.65 0.50    -  t=2: 7.80e-06 vs 7.67e-06
  R/A 256 g3=4 mixed     d_v (pooled over the batch)                                 0.56 x at t=3: 8.06e-07 vs 4.53e-07
  R/A wide none          d_H 0.34 0.52 0.50 0.52 0.45 0.42 0.52 0.78 0.61 0.68    -  t=1: 7.00e-06 vs 5.45e-06
  R/A wide none          d_W 0.60 0.50 0.40 0.40 0.52 0.42 0.53 1.10 0.76 1.00    -  t=3: 8.37e-06 vs 9.23e-06
  R/A wide none          d_v (pooled over the batch)                                 0.33 x at t=3: 9.67e-07 vs 3.19e-07
  R/A wide mixed         d_H 0.44 0.88 0.52 0.54 0.53 0.53 0.43 0.70 0.62 0.71    -  t=3: 3.80e-06 vs 3.35e-06
  R/A wide mixed         d_W 0.58 0.61 0.47 0.59 0.90 0.45 0.58 0.98 0.65 0.50    -  t=2: 7.80e-06 vs 7.67e-06
  R/A wide mixed         d_v (pooled over the batch)                                 0.56 x at t=3: 8.06e-07 vs 4.53e-07
  R/A wide l1            d_H 0.34 0.63 0.57 0.57 0.50 0.42 0.38 0.68 0.75 0.55    -  t=3: 1.49e-05 vs 1.11e-05
  R/A wide l1            d_W 0.61 0.43 0.44 0.47 0.48 0.35 0.63 0.88 0.82 0.59    -  t=2: 8.99e-06 vs 7.89e-06
  R/A wide l1            d_v (pooled over the batch)                                 1.00 x at t=2: 1.20e-05 vs 1.20e-05
  R/A wide l2            d_H 0.33 0.83 0.46 0.55 0.50 0.57 0.59 0.64 0.87 0.77    -  t=3: 1.45e-05 vs 1.26e-05
  R/A wide l2            d_W 0.65 0.61 0.39 0.51 0.46 0.56 0.51 0.76 0.78 0.53    -  t=3: 1.19e-05 vs 9.20e-06
  R/A wide l2            d_v (pooled over the batch)                                 0.49 x at t=3: 7.37e-07 vs 3.59e-07
  R/B wide none          d_H 0.70 0.56 0.74 0.67 0.51 0.47 0.70 0.64 0.68 0.38    -  t=1: 4.99e-06 vs 3.70e-06
  R/B wide none          d_W 2.00 0.60 0.60 0.42 0.48 0.42 0.93 0.55 0.58 0.58    -  t=3: 1.59e-06 vs 3.19e-06
  R/B wide none          d_v (pooled over the batch)                                 0.56 x at t=2: 6.85e-07 vs 3.83e-07
  R/B wide mixed         d_H 0.58 0.56 0.65 0.64 0.73 0.62 0.82 0.67 0.52 0.36    -  t=3: 1.25e-05 vs 1.03e-05
  R/B wide mixed         d_W 1.49 0.34 0.59 0.37 0.78 0.60 0.73 0.46 0.34 0.48    -  t=3: 2.17e-06 vs 3.24e-06
  R/B wide mixed         d_v (pooled over the batch)                                 0.43 x at t=2: 8.73e-07 vs 3.77e-07
  R/B wide l1            d_H 0.60 0.82 0.58 1.00 0.67 0.68 0.61 0.71 0.53 0.54    -  t=3: 1.12e-05 vs 1.12e-05
  R/B wide l1            d_W 0.78 0.52 0.56 0.81 0.78 0.67 0.71 0.54 0.53 0.73    -  t=3: 1.93e-05 vs 1.57e-05
  R/B wide l1            d_v (pooled over the batch)                                 0.64 x at t=2: 7.25e-07 vs 4.60e-07
  R/B wide l2            d_H 0.69 0.48 0.54 0.67 0.68 0.58 0.82 0.52 0.48 0.49    -  t=1: 5.96e-06 vs 4.90e-06
  R/B wide l2            d_W 0.68 0.60 0.53 0.53 0.56 0.55 0.91 0.47 0.44 0.79    -  t=1: 9.60e-06 vs 8.78e-06
  R/B wide l2            d_v (pooled over the batch)                                 0.44 x at t=2: 6.33e-07 vs 2.77e-07
  S/A none               d_H    - 0.44 0.49    -    -    -    -    - 0.58 0.31 0.67  t=1: 1.89e-05 vs 1.27e-05
  S/A none               d_W    - 0.52 0.37    -    -    -    -    - 0.44 0.37 0.48  t=1: 1.33e-06 vs 6.85e-07
  S/A none               d_v (pooled over the batch)                                 0.24 x at t=2: 3.46e-07 vs 8.21e-08
  S/A mixed              d_H    - 0.57 0.35    -    -    -    -    - 0.62 0.32 0.53  t=2: 7.01e-06 vs 4.36e-06
  S/A mixed              d_W    - 0.61 0.37    -    -    -    -    - 0.64 0.37 0.55  t=2: 9.19e-06 vs 5.88e-06
  S/A mixed              d_v (pooled over the batch)                                 2.30 x at t=2: 2.81e-07 vs 6.47e-07
  stream-K               d_H (pooled over the four edge slots)                       0.59 x at t=2: 3.35e-06 vs 1.99e-06
  stream-K               d_W (pooled over the four edge slots)                       0.70 x at t=2: 4.56e-06 vs 3.17e-06
  stream-K               d_v (pooled over the four edge slots)                       0.68 x at t=2: 2.09e-07 vs 1.43e-07
  refit none             d_W rank 5: 1.33 x (t=3: 6.06e-07 vs 8.06e-07), rank 16: 1.23 x (t=3: 3.53e-06 vs 4.33e-06),
                             rank 33: 1.89 x (t=3: 2.75e-06 vs 5.20e-06)
  refit mixed            d_W rank 5: 1.79 x (t=1: 3.91e-07 vs 6.99e-07), rank 16: 2.01 x (t=1: 3.58e-07 vs 7.18e-07),
                             rank 33: 2.50 x (t=3: 4.40e-07 vs 1.10e-06)       (nnls and nnls_batch gave the same figures)
The largest figure anywhere is 4.07 x (the violation ratio at t = 3 under CNMF_GEMM3 = 1 with the mixed penalty).  The
mutants of test_the_bar_has_teeth, in the best quantity of each of the six restarts of ranks 5, 7, 9: (a) 60 ... 430 x,
(b) 720 ... 8300 x (d_v; W and H are untouched), (c) 630 ... 1020 x, (d) 9.4e5 ... 1.5e6 x.
"""
import numpy as np
import pytest

from tests import _cd_steps_ref as R

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- comparison
def check_within(label, y, d, failures):
    """Print restatement distance, device distance and their ratio; note a failure above the bar."""
    print("%s: restatement vs float64 %.3e, device vs float64 %.3e (%.2f x)" % (
        label, y, d, d / y if y else np.inf if d else 0.0))
    if not d <= R.FACTOR * y:
        failures.append((label, d, y))


def compare(label, ref, t, H, W, n_iter, viol, failures, only=None, pool_all=False):
    """Every restart of ``ref`` (or the indices ``only``) at iteration t.  The yardstick of a tier is shared by its
    restarts, so the tier's worst device distance is what meets the bar: one line per tier and quantity, with the restart
    that set it.  ``pool_all``: the W / H yardstick over all compared restarts instead of the tier."""
    worst = {}
    for i in (sorted(ref.runs) if only is None else only):
        r = ref.runs[i]
        w, h = np.asarray(W[i]), np.asarray(H[i])
        assert w.shape == r["W"][t].shape and h.shape == r["H"][t].shape
        if n_iter[i] != t:
            failures.append((label, t, "n_iter", i, int(n_iter[i])))
        if not (np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0):
            failures.append((label, t, "not finite or negative", i, r["k"]))
            continue
        tr = None if pool_all else R.tier(r["k"])
        found = [("W", tr, R.d_cols(w, r["W"][t])), ("H", tr, R.d_rows(h, r["H"][t]))]
        if t == 1:
            if viol[i] != 1.0:
                failures.append((label, t, "viol != 1.0", i, float(viol[i])))
        else:
            found.append(("v", None, abs(float(viol[i]) - r["ratio"][t])))
        for what, tr, d in found:
            if not d <= worst.get((what, tr), (-1.0, 0))[0]:          # (a NaN distance is kept: it fails the bar)
                worst[(what, tr)] = (d, i)
    for (what, tr), (d, i) in sorted(worst.items(), key=lambda kv: (kv[0][0], kv[0][1] or 0)):
        check_within("%s t=%d d_%s tier %s (restart %d, rank %d)" % (label, t, what, tr or "all", i, ref.runs[i]["k"]),
                     ref.Y("y" + what, t, tr), d, failures)


def device_steps(engine, mname, bname, regname, t, **kw):
    ks, _ = R.batch(bname)
    st = R.inits(mname, bname)
    return engine.nmf_batch(list(ks), W0=[w for w, _ in st], H0=[h for _, h in st], tol=0.0, max_iter=t, return_W=True,
                            warn=False, **R.REGS[regname], **kw)


def run_case(engine, label, mname, bname, regname, ts, mode=None, kc=None, **kw):
    ref = R.reference(mname, bname, regname)
    engine.set_matrix(R.matrix(mname))
    failures = []
    for t in ts:
        H, W, n_iter, viol = device_steps(engine, mname, bname, regname, t, **kw)
        st = engine.last_stats
        assert mode is None or st["gemm_mode"] == mode, st
        assert kc is None or st["kc"] == kc, st
        compare(label, ref, t, H, W, n_iter, viol, failures)
    assert not failures, failures


# ---------------------------------------------------------------- CPU: the oracle's snapshots, the inputs, the mutants
def test_oracle_snapshots_equal_separate_runs():
    """``snapshots`` records what a run with max_iter = t returns, bit for bit, and leaves the run itself unchanged."""
    X = R.matrix("A")
    W0, H0 = R.inits("A", "R")[R.RANKS_R.index(7)]
    W0, H0 = W0.astype(np.float64), H0.astype(np.float64)
    reg = R.REGS["mixed"]
    snaps, trace = {1: None, 2: None, 3: None, 9: None}, []
    W3, H3, n3 = R.nmf_cd.nmf(X, 7, W0=W0, H0=H0, tol=0.0, max_iter=3, trace=trace, snapshots=snaps, **reg)
    assert n3 == 3 and snaps[9] is None and len(trace) == 3
    for t in (1, 2, 3):
        tr = []
        Wt, Ht, nt = R.nmf_cd.nmf(X, 7, W0=W0, H0=H0, tol=0.0, max_iter=t, trace=tr, **reg)
        assert nt == t and tr == trace[:t]
        assert Wt.tobytes() == snaps[t][0].tobytes() and np.ascontiguousarray(Ht).tobytes() == snaps[t][1].tobytes()
    Hn = R.refit_spectra()[0].astype(np.float64)
    s = {1: None, 2: None}
    W2, n2 = R.nmf_cd.nnls(X, Hn, tol=0.0, max_iter=2, snapshots=s)
    W1, n1 = R.nmf_cd.nnls(X, Hn, tol=0.0, max_iter=1)
    assert (n1, n2) == (1, 2) and W1.tobytes() == s[1][0].tobytes() and W2.tobytes() == s[2][0].tobytes()
    assert np.array_equal(s[1][1], Hn)


def test_the_unmutated_loop_is_the_oracle():
    """The copy of the oracle's loop that carries the mutants equals the oracle bit for bit when nothing is switched on."""
    X = R.matrix("A")
    for k, regname in ((5, "none"), (9, "mixed")):
        i = R.RANKS_R.index(k)
        W0, H0 = R.inits("A", "R")[i]
        snaps, ratio = R.mutant_run(X, W0, H0, R.REGS[regname], None)
        run = R.reference("A", "R", regname).runs[i]
        for t in R.TS:
            assert snaps[t][0].tobytes() == run["W"][t].tobytes() and snaps[t][1].tobytes() == run["H"][t].tobytes()
            assert ratio[t] == run["ratio"][t]


@pytest.mark.parametrize("regname", list(R.REGS))
def test_the_inputs_hold_what_they_claim(regname):
    A = R.matrix("A")
    N, G = A.shape
    assert (N, G) == (517, 500) and N % 16 == N % 64 == N % 256 == 5 and G % 64 == 52 and G % 128 == 116
    ks, seeds = R.batch("R")
    assert len(ks) == 46 and sum(ks) == 772 and len(set(seeds)) == 46
    # where the scheduler puts them (R.first_fill): all 46 in the first fill of 1024 columns, a slot across every group edge
    # (in the listed order a slot would end exactly on 256)
    off = R.first_fill(ks, 1024)
    assert sorted(off) == list(range(46)) and sorted(off[r] + ks[r] for r in off)[-1] == 772
    straddlers, _ = R.edge_slots(ks, 1024)
    for edge in R.EDGES:
        assert any(off[r] < edge < off[r] + ks[r] for r in straddlers), edge
    assert set(ks) >= set(range(1, 17)) and {R.tier(k) for k in ks} == {4, 8, 12, 16, 20, 24, 28, 32, 48, 64}
    ref = R.reference("A", "R", regname)
    assert sorted(ref.runs) == list(range(46))            # no restart is left out
    zW = zH = 0.0
    for r in ref.runs.values():
        for t in R.TS:
            W, H = r["W"][t], r["H"][t]
            assert np.isfinite(W).all() and np.isfinite(H).all() and W.min() >= 0 and H.min() >= 0
            assert (W.max(axis=0) > 0).all() and (H.max(axis=1) > 0).all(), (r["k"], t)
            assert r["yW"][t] > 0 and r["yH"][t] > 0, (r["k"], t)
        assert r["ratio"][1] == 1.0 and r["yv"][1] == 0.0
        for t in (2, 3):
            assert r["ratio"][t] >= 1e-3 and r["yv"][t] > 0, (r["k"], t, r["ratio"][t])
        zW, zH = max(zW, float((r["W"][3] == 0).mean())), max(zH, float((r["H"][3] == 0).mean()))
    print("%s: largest share of exact zeros at t=3: W %.3f H %.3f; smallest violation ratio %.3e" % (
        regname, zW, zH, min(r["ratio"][t] for r in ref.runs.values() for t in (2, 3))))
    assert zW >= 0.45 and zH >= 0.45, (zW, zH)
    for tr in ref.tiers():
        for t in R.TS:
            assert ref.Y("yW", t, tr) > 0 and ref.Y("yH", t, tr) > 0


def test_the_stream_k_slots_lie_on_the_group_edges():
    """The slots test_stream_k_cut_tiles_after_two_iterations compares, in the order the scheduler places them (not the
    listed one): one fill, restarts 80 and 96 across 512 and 768, and 256 hit exactly -- there the slot that ends on it
    and the slot that begins on it."""
    ks, seeds, straddlers, touchers = R.streamk_ranks()
    assert len(ks) == 110 == len(set(seeds)) and sum(ks) == 1021
    off = R.first_fill(ks, 1024)
    assert sorted(off) == list(range(110))                         # one fill: nothing is placed later, nothing moves
    spans = sorted((off[r], off[r] + ks[r]) for r in off)
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == 1021
    assert [(r, ks[r], off[r]) for r in straddlers] == [(80, 11, 511), (96, 9, 761)]
    assert not any(off[r] < 256 < off[r] + ks[r] for r in off)
    assert sorted((off[r], off[r] + ks[r]) for r in touchers) == [(243, 256), (256, 268)]
    assert 3 <= len(straddlers) + len(touchers) <= 6


def test_the_refit_yardsticks_are_positive():
    for regname in ("none", "mixed"):
        ref = R.refit_reference(regname)
        assert [r["k"] for r in ref.runs.values()] == [5, 16, 33]
        for r in ref.runs.values():
            for t in (1, 3):
                assert r["yW"][t] > 0 and (r["W"][t].max(axis=0) > 0).all(), (regname, r["k"], t)


@pytest.mark.parametrize("mutant", ["a", "b", "c", "d"])
def test_the_bar_has_teeth(mutant):
    """Every restart of ranks 5, 7, 9 of batch R, run through a float64 mutant of the oracle's loop, lands above 16 x the
    yardstick in d_W, d_H or d_v at some t <= 3."""
    regname = "mixed" if mutant == "c" else "none"
    X = R.matrix("A")
    ref = R.reference("A", "R", regname)
    slipped = []
    for i, k in enumerate(R.RANKS_R):
        if k not in (5, 7, 9):
            continue
        W0, H0 = R.inits("A", "R")[i]
        snaps, ratio = R.mutant_run(X, W0, H0, R.REGS[regname], mutant)
        run, over = ref.runs[i], []
        for t in R.TS:
            for what, d, y in (("W", R.d_cols(snaps[t][0], run["W"][t]), ref.Y("yW", t, R.tier(k))),
                               ("H", R.d_rows(snaps[t][1], run["H"][t]), ref.Y("yH", t, R.tier(k))),
                               ("v", abs(ratio[t] - run["ratio"][t]), ref.Y("yv", t))):
                if t == 1 and what == "v":
                    continue
                print("mutant %s rank %d restart %d t=%d %s: restatement %.3e, mutant %.3e (%.1f x)" % (
                    mutant, k, i, t, what, y, d, d / y))
                if d > R.FACTOR * y:
                    over.append((t, what))
        if not over:
            slipped.append((mutant, k, i))
    assert not slipped, slipped


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
@pytest.mark.parametrize("g3mode", ["0", "1", "2", "3", "4"])
def test_batch_R_in_every_gemm_mode_at_256_columns(engine, monkeypatch, g3mode, regname):
    """772 columns through a 256-column batch (three fills: slots are retired and explicit W0 / H0 installed into reused
    ones) on the exact-f32 pipe (0), both general split-operand variants (1, 2), three bf16 planes (3), two f16 planes (4).
    On a count-structured matrix modes 1-3 are reachable only through the knob: a build that ignores it fails here."""
    monkeypatch.setenv("CNMF_GEMM3", g3mode)
    run_case(engine, "R/A g3=%s %s" % (g3mode, regname), "A", "R", regname, R.TS, mode=min(int(g3mode), 4), kc=256,
             kc_max=256)


@gpu
@pytest.mark.parametrize("regname", list(R.REGS))
@pytest.mark.parametrize("mname,mode", [("A", 4), ("B", 5)])
def test_batch_R_at_the_automatic_width(engine, mname, mode, regname):
    """All 772 columns at once (1024 packed columns, four component groups): the W sweep that writes the f16 planes, the
    H half-step's partial sums and the wide finalize, each with every kind of penalty."""
    run_case(engine, "R/%s wide %s" % (mname, regname), mname, "R", regname, R.TS, mode=mode, kc=1024)


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_batch_S_big_ranks_beside_small_ones(engine, regname):
    """Ranks up to 128 (sweep_big_kernel) beside the small tiers in one batch at the default width."""
    run_case(engine, "S/A %s" % regname, "A", "S", regname, (1, 2), mode=4)


@gpu
def test_stream_k_cut_tiles_after_two_iterations(engine):
    """The matrix and rank list of test_stream_k_cut_tiles_match_oracle (12 500 cells, 1024 columns: pass A cuts tiles).
    Compared: the slots that lie across a component-group edge WHERE THE SCHEDULER PUTS THEM (restarts 80 and 96, across
    512 and 768: they carry the two cut flags of one slot), and at 256, which this list hits exactly, the slot that ends
    on it and the slot that begins on it (test_the_stream_k_slots_lie_on_the_group_edges).  Yardstick pooled over them."""
    ks, seeds, straddlers, touchers = R.streamk_ranks()
    slots = straddlers + touchers
    X32 = R.synth.make_config("C3", dtype=np.float32, n_cells=12500)
    st = [R.nmf_cd.random_init(X32, k, seed) for k, seed in zip(ks, seeds)]
    X64 = X32.astype(np.float64)
    ref = R.Reference({i: R.run_pair(X64, st[i][0], st[i][1], R.REGS["none"], ts=(2,)) for i in slots})
    engine.set_matrix(X32)
    engine.set_iteration_hints(None)          # the placement above is that of a queue without hints
    H, W, n_iter, viol = engine.nmf_batch(ks, W0=[w for w, _ in st], H0=[h for _, h in st], tol=0.0, max_iter=2,
                                          return_W=True, warn=False, kc_max=1024)
    assert engine.last_stats["kc"] == 1024 and engine.last_stats["gemm_mode"] == 4, engine.last_stats
    assert (np.asarray(n_iter) == 2).all()
    failures = []
    compare("stream-K", ref, 2, H, W, n_iter, viol, failures, only=slots, pool_all=True)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("regname", ["none", "mixed"])
def test_refit_steps(engine, regname):
    """Phase 2 of the finalize: engine.nnls and engine.nnls_batch against nmf_cd.nnls after 1 and 3 sweeps.  W starts at
    zero, so the ``w == 0 -> min(0, grad)`` branch carries the whole first sweep."""
    ref = R.refit_reference(regname)
    Hs = R.refit_spectra()
    reg = {k: v for k, v in R.REGS[regname].items() if k != "alpha_H"}
    engine.set_matrix(R.matrix("A"))
    failures = []
    for t in (1, 3):
        Wb, nb, _ = engine.nnls_batch(list(Hs), tol=0.0, max_iter=t, **reg)
        for i, H in enumerate(Hs):
            W1, n1 = engine.nnls(H, tol=0.0, max_iter=t, warn=False, **reg)
            r = ref.runs[i]
            for label, w, n in (("nnls", W1, n1), ("nnls_batch", Wb[i], nb[i])):
                assert n == t, (label, i, n, t)
                assert w.shape == r["W"][t].shape and np.isfinite(w).all() and w.min() >= 0
                check_within("%s %s t=%d d_W rank %d" % (label, regname, t, r["k"]), r["yW"][t], R.d_cols(w, r["W"][t]),
                             failures)
    assert not failures, failures


@gpu
def test_three_iterations_are_deterministic(engine):
    engine.set_matrix(R.matrix("A"))
    a = device_steps(engine, "A", "R", "none", 3)
    assert engine.last_stats["gemm_mode"] == 4
    b = device_steps(engine, "A", "R", "none", 3)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
