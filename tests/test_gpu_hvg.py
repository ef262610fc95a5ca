"""Preprocess.highly_variable_genes (seurat_v3) and ``hvg="device"`` on the device against the float64 numpy restatement
tests/_seurat_v3_ref.py: the three entry points of csrc/hvg_host.hip.h one by one, then the frame, the selected set and
the two public routes end to end.

Data: Gamma-Poisson counts at 300 x 600 and 257 x 1000 (neither a multiple of 64 or 256), gene means exp(N(-1, 1.5)),
dispersions Gamma(2, 0.5) + 0.05; two all-zero genes, a gene with one entry, a column of exactly 64 entries and one of
65; as a CSR with stored zeros and shuffled columns for the entry points, as a canonical CSR and as a dense array for the
public methods.

Tolerance of everything that is not exact: 16 x the restatement's distance from its own ``np.longdouble`` run, the rule
of the Harmony tests.  Every test prints both distances; measured on an MI355X (max abs difference, restatement vs long
double / device vs restatement), 300 x 600 and 257 x 1000:

  vertices          value 3.3e-15 / 3.6e-15, 5.4e-15 / 5.3e-15;   slope 2.2e-15 / 2.0e-15, 7.2e-15 / 6.8e-15
  every point       value 1.5e-15 / 1.6e-15, 3.3e-15 / 3.1e-15;   slope 4.6e-15 / 4.7e-15, 4.9e-15 / 4.8e-15
  span 1.0 (q = n)  value 5.6e-15 / 1.6e-15, 6.4e-15 / 1.4e-14;   slope 1.4e-15 / 4.9e-15, 2.1e-15 / 9.3e-15 (4.5 x, the most)
  n = 100, q = 30   value 1.6e-15 / 2.2e-15, 3.2e-15 / 3.1e-15;   slope 4.6e-15 / 1.3e-14, 3.2e-15 / 3.0e-15
  variances_norm    interpolate 8.7e-15 / 7.2e-15, 1.2e-14 / 1.1e-14;   direct 6.3e-15 / 6.9e-15, 1.0e-14 / 1.1e-14
  relative gap of variances_norm across the cut: 2.6e-3, 1.9e-3 (300 x 600), 1.3e-3, 8.7e-4 (257 x 1000)

(With plain float64 sums, or with a product fused into a compensated sum, the local fits miss the bound: up to 75 x.)"""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd import preprocess as pp
from cnmf_amd.preprocess import Preprocess
from tests import _filter_ref as F
from tests import _seurat_v3_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
SHAPES = [(300, 600, 1), (257, 1000, 2)]
N_TOP = 120


@pytest.fixture(autouse=True)
def release(engine):
    yield
    engine.preprocess_release()


class Case:
    def __init__(self, N, G, seed):
        self.N, self.G = N, G
        self.C = R.gamma_poisson_counts(N, G, seed)
        self.cells, self.genes = ["c%d" % i for i in range(N)], ["g%d" % j for j in range(G)]
        self.stored = R.with_stored_zeros(self.C, seed)
        self.frame, self.parts, self.frame_ld, self.parts_ld = {}, {}, {}, {}
        for surface in ("interpolate", "direct"):
            self.frame[surface], self.parts[surface] = R.seurat_v3(self.C, N_TOP, surface=surface, genes=self.genes, parts=True)
            self.frame_ld[surface], self.parts_ld[surface] = R.seurat_v3(self.C, N_TOP, surface=surface, genes=self.genes,
                                                                         dtype=LD, parts=True)
        p = self.parts["direct"]
        nc = p["var"] > 0
        x, y = np.log10(p["mean"][nc]), np.log10(p["var"][nc])
        order = np.argsort(x, kind="stable")
        self.xs, self.ys = x[order], y[order]

    def data(self, dense):
        return pd.DataFrame(self.C, index=self.cells, columns=self.genes) if dense else (sp.csr_matrix(self.C), self.cells,
                                                                                        self.genes)


@pytest.fixture(scope="module")
def cases():
    return [Case(*s) for s in SHAPES]


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)))) if np.size(a) else 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_within(label, got, f64, ld, failures):
    base, err = maxdiff(f64, ld), maxdiff(got, f64)
    print("%s: restatement vs long double %.3e, device vs restatement %.3e (%.2f x)" % (
        label, base, err, err / base if base else np.inf if err else 0.0))
    if not err <= 16 * base:
        failures.append((label, err, base))


def test_the_inputs_hold_what_they_claim(cases):
    for c in cases:
        nnz = (c.C != 0).sum(axis=0)
        assert list(nnz[:5]) == [0, 0, 1, 64, 65]
        assert c.stored.nnz > (c.C != 0).sum() and (c.stored.data == 0).any() and not c.stored.has_sorted_indices
        assert np.array_equal(c.stored.toarray(), c.C)
        assert c.N % 64 and c.G % 64 and c.N % 256 and c.G % 256
        assert (c.parts["direct"]["var"] > 0).sum() == c.xs.size < c.G


def test_moments_are_exact(engine, cases):
    """S1 and S2 equal the restatement's integers over the CSR as stored (stored zeros, shuffled columns), and the
    frame's means and variances have the restatement's bits for CSR and for dense input."""
    for c in cases:
        engine.preprocess_upload_as_stored(c.stored)
        s1, s2, flags = engine.preprocess_gene_moments()
        p = c.parts["interpolate"]
        assert flags == 0 and s1.dtype == np.int64 and np.array_equal(s1, p["s1"]) and np.array_equal(s2, p["s2"])
        engine.preprocess_release()
        P = Preprocess(engine=engine)
        for dense in (False, True):
            got = P.highly_variable_genes(c.data(dense), n_top_genes=N_TOP)
            want = c.frame["interpolate"]
            assert np.array_equal(bits(got["means"]), bits(want["means"]))
            assert np.array_equal(bits(got["variances"]), bits(want["variances"]))
            assert list(got.index) == c.genes


def test_moments_see_the_staging_as_restricted(engine, cases):
    c = cases[0]
    rs = np.random.RandomState(5)
    kc, kg = rs.rand(c.N) < 0.7, rs.rand(c.G) < 0.6
    engine.preprocess_upload_as_stored(c.stored)
    engine.preprocess_subset(kc, kg)
    want = R.gene_moments(F.subset(c.stored, kc, kg))
    got = engine.preprocess_gene_moments()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 0
    clip = rs.gamma(2.0, 1.0, size=int(kg.sum())) + 0.5
    c1, c2 = engine.preprocess_clipped_sums(clip)
    w1, w2 = R.clipped_sums(F.subset(c.stored, kc, kg), clip)
    for got, want in ((c1, w1), (c2, w2)):
        assert (np.abs(got - want) <= 2 * c.N * 2.0 ** -53 * want).all()


def test_clipped_sums(engine, cases):
    """C1 and C2 over the CSR as stored with the restatement's own clip.  Either sum of n <= N non-negative terms is within
    (n - 1) u of the exact sum, relatively (u = 2^-53), whatever its order: the two are within 2 N u of each other
    (measured: a few u); a gene nothing is clipped in has integer terms and is exact."""
    for c in cases:
        p = c.parts["interpolate"]
        engine.preprocess_upload_as_stored(c.stored)
        c1, c2 = engine.preprocess_clipped_sums(p["clip"])
        for got, want, what in ((c1, p["c1"], "C1"), (c2, p["c2"], "C2")):
            rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
            print("%d x %d %s: max relative difference %.3e" % (c.N, c.G, what, rel.max()))
            assert rel.max() <= 2 * c.N * 2.0 ** -53
        unclipped = c.C.max(axis=0) <= p["clip"]
        assert unclipped.any() and np.array_equal(c1[unclipped], c.C.sum(axis=0)[unclipped])
        assert np.array_equal(c2[unclipped], (c.C * c.C).sum(axis=0)[unclipped])
        assert (c1[:2] == 0).all() and (c2[:2] == 0).all()


def test_local_fits(engine, cases):
    """Value and slope of the device's local fits within 16 x the restatement's distance from its long double run: at the
    vertices of the interpolation surface (the two end vertices lie below the smallest and above the largest abscissa),
    at every point (surface "direct"), with q = n (span 1.0) and with q = 30 smaller than the workgroup (n = 100)."""
    failures = []
    for c in cases:
        xs, ys = c.xs, c.ys
        v, _ = R.loess_vertices(xs, 0.3)
        assert v[0] < xs[0] and v[-1] > xs[-1]
        sub = slice(None, None, max(1, xs.size // 100))
        x100, y100 = xs[sub][:100], ys[sub][:100]
        sets = [("vertices", xs, ys, R.loess_q(xs.size, 0.3), v), ("direct", xs, ys, R.loess_q(xs.size, 0.3), xs),
                ("span 1.0", xs, ys, xs.size, np.concatenate([v[:1], xs[::37], v[-1:]])),
                ("n = 100", x100, y100, 30, np.concatenate([[x100[0] - 0.1], x100, [x100[-1] + 0.1]]))]
        for name, x, y, q, at in sets:
            assert x.size == 100 or name != "n = 100"
            value, slope, status = engine.preprocess_loess_fit(x, y, q, at)
            assert (status == 0).all(), (name, np.flatnonzero(status))
            f64, ld = R.local_fits(x, y, at, q), R.local_fits(x, y, at, q, LD)
            check_within("%d x %d %s value" % (c.N, c.G, name), value, f64[0], ld[0], failures)
            check_within("%d x %d %s slope" % (c.N, c.G, name), slope, f64[1], ld[1], failures)
    assert not failures, failures


def test_tie_cases_come_back_flagged_and_the_host_solves_them(engine):
    """ten copies each of 0..4: rank one (q = 15 at 2.0) and rank two (q = 25 at 1.5) come back with status 2, the
    zero-width neighbourhood (q = 8) with status 1; the host path gives the restatement's values bit for bit."""
    x, y = R.tie_case()
    value, slope, status = engine.preprocess_loess_fit(x, y, 15, [2.0])
    assert list(status) == [2] and value[0] == 0 and slope[0] == 0
    assert list(engine.preprocess_loess_fit(x, y, 8, [2.0])[2]) == [1]
    assert list(engine.preprocess_loess_fit(x, y, 25, [1.5])[2]) == [2]
    # q = 25 at 1.75: h = 1.25, the points at 3 are tied at h and weigh nothing: two distinct abscissae again
    assert list(engine.preprocess_loess_fit(x, y, 25, [1.5, 1.75])[2]) == [2, 2]
    # q = 35 at 1.75: h = 1.75, the points at 1, 2 and 3 weigh: three distinct abscissae, solved on the device
    value, slope, status = engine.preprocess_loess_fit(x, y, 35, [1.75])
    f64, ld = R.local_fit(x, y, 1.75, 35), R.local_fit(x, y, 1.75, 35, LD)
    print("three distinct abscissae: value %.3e (restatement vs long double %.3e), slope %.3e (%.3e)" % (
        abs(value[0] - f64[0]), abs(f64[0] - ld[0]), abs(slope[0] - f64[1]), abs(f64[1] - ld[1])))
    assert list(status) == [0]
    assert abs(value[0] - f64[0]) <= 16 * abs(f64[0] - ld[0]) and abs(slope[0] - f64[1]) <= 16 * abs(f64[1] - ld[1])
    got = pp.loess_fitted(engine, x, y, span=0.3, surface="direct")                     # q = 15: every fit is rank one
    assert np.array_equal(bits(got), bits(R.loess_fitted(x, y, 0.3, "direct")))
    assert np.abs(got - np.repeat([y[x == k].mean() for k in range(5)], 10)).max() < 1e-14
    with pytest.raises(ValueError, match="zero-width"):
        pp.loess_fitted(engine, x, y, span=0.16, surface="direct")                      # q = 8


def test_frame_and_selected_set(engine, cases):
    """variances_norm within 16 x the restatement's long double distance on both surfaces; the selected set and
    highly_variable_rank equal the restatement's.  Condition, on the restatement alone: the relative gap of
    variances_norm across the cut is at least 1e-6."""
    failures = []
    P = Preprocess(engine=engine)
    for c in cases:
        for surface in ("interpolate", "direct"):
            want, ld = c.frame[surface], c.frame_ld[surface]
            v = np.sort(want["variances_norm"].values)[::-1]
            gap = (v[N_TOP - 1] - v[N_TOP]) / v[N_TOP - 1]
            print("%d x %d %s: relative gap across the cut %.3e" % (c.N, c.G, surface, gap))
            assert gap >= 1e-6
            got = P.highly_variable_genes(c.data(False), n_top_genes=N_TOP, surface=surface)
            check_within("%d x %d %s variances_norm" % (c.N, c.G, surface), got["variances_norm"].values,
                         want["variances_norm"].values, ld["variances_norm"].values.astype(LD), failures)
            assert np.array_equal(got["highly_variable"].values, want["highly_variable"].values)
            assert got["highly_variable"].sum() == N_TOP
            assert np.array_equal(got["highly_variable_rank"].values, want["highly_variable_rank"].values, equal_nan=True)
    assert not failures, failures


def test_determinism(engine, cases):
    c = cases[1]
    v, _ = R.loess_vertices(c.xs, 0.3)
    at = np.concatenate([v, c.xs])
    q = R.loess_q(c.xs.size, 0.3)
    a, b = engine.preprocess_loess_fit(c.xs, c.ys, q, at), engine.preprocess_loess_fit(c.xs, c.ys, q, at)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    P = Preprocess(engine=engine)
    for surface in ("interpolate", "direct"):
        f1 = P.highly_variable_genes(c.data(False), n_top_genes=N_TOP, surface=surface)
        f2 = P.highly_variable_genes(c.data(True), n_top_genes=N_TOP, surface=surface)
        pd.testing.assert_frame_equal(f1, f2, check_exact=True)
        assert np.array_equal(bits(f1["variances_norm"]), bits(f2["variances_norm"]))


def same_result(a, b):
    assert list(a.var_names) == list(b.var_names) and list(a.obs_names) == list(b.obs_names)
    if sp.issparse(a.X):
        assert sp.issparse(b.X) and F.same_csr(sp.csr_matrix(a.X), sp.csr_matrix(b.X))
    else:
        assert np.array_equal(bits(a.X), bits(b.X))


def test_normalize_batchcorrect_end_to_end(engine, cases):
    """hvg="device" equals the mask route given the restatement's own mask, bit for bit"""
    P = Preprocess(engine=engine)
    for c, dense in zip(cases, (False, True)):
        mask = c.frame["interpolate"]["highly_variable"].values
        res, hvgs = P.normalize_batchcorrect(c.data(dense), hvg="device", n_top_genes=N_TOP, makeplots=False)
        ref, hvgs_ref = P.normalize_batchcorrect(c.data(dense), highly_variable=mask, makeplots=False)
        assert hvgs == hvgs_ref and len(hvgs) == N_TOP
        same_result(res, ref)
        assert list(res.var.index) == hvgs and res.var["highly_variable"].all() and ref.var is None


def test_preprocess_for_cnmf_end_to_end(engine, cases):
    """with exclude_genes and a feature_type column: the selection runs on the RNA genes that are left (the restatement on
    exactly those columns gives the mask), tp10k keeps every gene, nothing downstream moved"""
    P = Preprocess(engine=engine)
    c = cases[0]
    n_adt = 7
    A = np.random.RandomState(3).poisson(30.0, size=(c.N, n_adt)).astype(np.float64)
    adt_names = ["ADT_%d" % j for j in range(n_adt)]
    ftype = np.array(["Gene Expression"] * c.G + [F.ADT_NAME] * n_adt)
    top = c.frame["interpolate"]
    exclude = list(top.index[top["highly_variable"].values][:15]) + ["not_a_gene"]
    keep = ~np.isin(np.array(c.genes), exclude)
    want = R.seurat_v3(c.C[:, keep], N_TOP, genes=np.array(c.genes)[keep])
    v = np.sort(want["variances_norm"].values)[::-1]
    assert (v[N_TOP - 1] - v[N_TOP]) / v[N_TOP - 1] >= 1e-6
    want_hvgs = list(want.index[want["highly_variable"].values])
    for dense in (False, True):
        M = np.hstack([c.C, A])
        data = (M if dense else sp.csr_matrix(M), c.cells, c.genes + adt_names)
        kw = dict(exclude_genes=exclude, feature_type=ftype, adt_feature_name=F.ADT_NAME, makeplots=False)
        res, tp, hvgs = P.preprocess_for_cnmf(data, hvg="device", n_top_rna_genes=N_TOP, **kw)
        ref, tp_ref, hvgs_ref = P.preprocess_for_cnmf(data, highly_variable=want_hvgs, **kw)
        assert hvgs == want_hvgs == hvgs_ref and not set(hvgs) & set(exclude) and not set(hvgs) & set(adt_names)
        same_result(res, ref)
        same_result(tp, tp_ref)
        assert list(tp.var_names) == c.genes + adt_names


def test_values_that_are_no_counts_are_refused(engine, cases):
    c = cases[0]
    P = Preprocess(engine=engine)
    for value in (1.5, -2.0):
        bad = c.C.copy()
        bad[17, 9] = value
        with pytest.raises(ValueError, match="seurat_v3"):
            P.highly_variable_genes((sp.csr_matrix(bad), c.cells, c.genes), n_top_genes=N_TOP)
    bad = c.stored.copy()
    bad.data[5] = 0.25
    engine.preprocess_upload_as_stored(bad)
    assert engine.preprocess_gene_moments()[2] == R.FLAG_NOT_COUNT
    bad.data[5] = R.COUNT_MAX + 1.0
    engine.preprocess_upload_as_stored(bad)
    assert engine.preprocess_gene_moments()[2] == R.FLAG_TOO_LARGE
    with pytest.raises(ValueError, match="seurat_v3"):
        P.normalize_batchcorrect((sp.csr_matrix(np.where(c.C == 2, 2.5, c.C)), c.cells, c.genes), hvg="device",
                                 n_top_genes=N_TOP, makeplots=False)
