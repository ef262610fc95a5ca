"""The host half of the starCAT feature, without a device: ``cNMF.build_reference`` / ``load_results`` on a small
hand-written run directory (against a numpy restatement written here, and against the unmodified reference class where its
tree is present), ``StarCAT``'s gene matching and bookkeeping with a numpy-backed stand-in for the engine, and the solver
pairs ``cNMF._check_kwargs`` admits."""
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cnmf_amd.cnmf import cNMF, load_df_from_npz, save_df_to_npz, save_df_to_text
from cnmf_amd.starcat import StarCAT
from tests import _mu_frobenius_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REFERENCE = os.path.isdir("/root/reference/src/cnmf")
K, THR = 3, 0.5
GENES = ["g%d" % j for j in range(12)]
HVGS = ["g7", "g2", "g9", "g4", "g0"]                    # list order differs from the column order; g4 has zero std


def write_run(tmp, name="run"):
    """The files of a finished ``consensus(3, 0.5)`` that build_reference / load_results read, with made-up values."""
    rs = np.random.RandomState(5)
    obj = cNMF(output_dir=str(tmp), name=name)
    tpm = pd.DataFrame(rs.gamma(0.7, 50.0, size=(K, len(GENES))), index=np.arange(1, K + 1), columns=GENES)
    score = pd.DataFrame(rs.standard_normal((K, len(GENES))), index=np.arange(1, K + 1), columns=GENES)
    usage = pd.DataFrame(rs.gamma(1.0, 1.0, size=(9, K)), index=["c%d" % i for i in range(9)], columns=np.arange(1, K + 1))
    std = rs.gamma(2.0, 3.0, size=len(GENES))
    std[4] = 0.0
    stats = pd.DataFrame({"__mean": rs.gamma(2.0, 5.0, size=len(GENES)), "__std": std}, index=GENES)
    rep = (K, "0_5")
    save_df_to_text(tpm, obj.paths["gene_spectra_tpm__txt"] % rep)
    save_df_to_text(score, obj.paths["gene_spectra_score__txt"] % rep)
    save_df_to_text(usage, obj.paths["consensus_usages__txt"] % rep)
    save_df_to_npz(stats, obj.paths["tpm_stats"])
    with open(obj.paths["nmf_genes_list"], "w") as F:
        F.write("\n".join(HVGS))
    return obj, tpm, score, usage, stats


def reference_restated(tpm, stats, target_sum=1e6):
    """build_reference in plain numpy: rows to ``target_sum``, divided by the std, the HVG columns in list order."""
    v = tpm.values / tpm.values.sum(axis=1, keepdims=True) * target_sum
    with np.errstate(divide="ignore", invalid="ignore"):
        v = v / stats["__std"].values[None, :]
    return v[:, [GENES.index(g) for g in HVGS]]


def reference_class():
    sys.path.insert(0, ROOT)
    from oracle import scanpy_shim
    scanpy_shim.install()
    import cnmf as ref
    return ref.cNMF


# ---------------------------------------------------------------- build_reference / load_results
@pytest.mark.parametrize("target_sum", [1e6, 1e4])
def test_build_reference_matches_its_restatement(tmp_path, target_sum):
    obj, tpm, _, _, stats = write_run(tmp_path)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = obj.build_reference(K, THR, target_sum=target_sum)
    want = reference_restated(tpm, stats, target_sum)
    assert np.isinf(want[:, 3]).all()                                       # g4: zero std, as in the reference
    for got in (out, load_df_from_npz(obj.paths["starcat_spectra"] % (K, "0_5")),
                pd.read_csv(obj.paths["starcat_spectra__txt"] % (K, "0_5"), sep="\t", index_col=0)):
        assert list(got.index) == ["GEP1", "GEP2", "GEP3"] and list(got.columns) == HVGS
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got.values.astype(float)), fin)
        assert np.abs(got.values.astype(float)[fin] / want[fin] - 1).max() < 1e-12    # (the TPM text through pandas' default parser)
    assert np.allclose(out.values[:, [0, 1, 2, 4]].sum(axis=1) > 0, True)


def test_starcat_paths_are_the_reference_names(tmp_path):
    obj = cNMF(output_dir=str(tmp_path), name="nm")
    assert obj.paths["starcat_spectra"] == os.path.join(str(tmp_path), "nm", "cnmf_tmp", "nm.starcat_spectra.k_%d.dt_%s.df.npz")
    assert obj.paths["starcat_spectra__txt"] == os.path.join(str(tmp_path), "nm", "nm.starcat_spectra.k_%d.dt_%s.txt")


def check_load_results(res, tpm, score, usage, n_top, norm):
    u, s, t, top = res
    want_u = usage.values / usage.values.sum(axis=1, keepdims=True) if norm else usage.values
    assert list(u.index) == list(usage.index) and list(u.columns) == [1, 2, 3] and np.allclose(u.values, want_u, rtol=1e-12, atol=0)
    assert s.shape == (len(GENES), K) and list(s.index) == GENES and np.allclose(s.values, score.values.T, rtol=1e-12, atol=0)
    assert t.shape == (len(GENES), K) and np.allclose(t.values, tpm.values.T, rtol=1e-12, atol=0)      # (pandas' default text parser: 1e-14)
    assert top.shape == (n_top, K)
    for j, gep in enumerate(s.columns):
        order = np.argsort(-score.values[j], kind="stable")[:n_top]
        assert list(top[gep]) == [GENES[i] for i in order]


@pytest.mark.parametrize("n_top, norm", [(4, True), (100, False)])
def test_load_results_matches_its_restatement(tmp_path, n_top, norm):
    obj, tpm, score, usage, _ = write_run(tmp_path)
    res = obj.load_results(K, THR, n_top_genes=n_top, norm_usage=norm)
    check_load_results(res, tpm, score, usage, min(n_top, len(GENES)), norm)


@pytest.mark.skipif(not HAVE_REFERENCE, reason="needs the reference tree (build container)")
def test_build_reference_and_load_results_match_the_reference_class(tmp_path):
    obj, *_ = write_run(tmp_path)
    with np.errstate(divide="ignore", invalid="ignore"):
        obj.build_reference(K, THR)
    mine = load_df_from_npz(obj.paths["starcat_spectra"] % (K, "0_5"))
    mine_txt = open(obj.paths["starcat_spectra__txt"] % (K, "0_5")).read()
    mine_res = obj.load_results(K, THR, n_top_genes=5)
    os.remove(obj.paths["starcat_spectra"] % (K, "0_5"))
    os.remove(obj.paths["starcat_spectra__txt"] % (K, "0_5"))
    ref = reference_class()(output_dir=str(tmp_path), name="run")           # the same files under the same names
    assert ref.paths["starcat_spectra"] == obj.paths["starcat_spectra"]
    assert ref.paths["starcat_spectra__txt"] == obj.paths["starcat_spectra__txt"]
    with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
        warnings.simplefilter("ignore")
        ref.build_reference(K, THR)
    theirs = load_df_from_npz(ref.paths["starcat_spectra"] % (K, "0_5"))
    assert list(mine.index) == list(theirs.index) and list(mine.columns) == list(theirs.columns)
    assert np.array_equal(mine.values, theirs.values)
    assert mine_txt == open(ref.paths["starcat_spectra__txt"] % (K, "0_5")).read()
    for a, b in zip(mine_res, ref.load_results(K, THR, n_top_genes=5)):
        assert list(a.index) == list(b.index) and list(a.columns) == list(b.columns)
        assert a.values.dtype == b.values.dtype and (a.values == b.values).all()


# ---------------------------------------------------------------- StarCAT's host logic
class NumpyEngine:
    """What StarCAT calls on an Engine, in numpy: the scaling of prepare_select and the restated refit."""

    def __init__(self, fail_in_select=False):
        self.fail_in_select, self.staged, self.released, self.calls = fail_in_select, None, 0, []
        self.X = self.shape = None

    def prepare_upload(self, counts):
        self.staged = sp.csr_matrix(counts).astype(np.float64)
        return self.staged

    def prepare_select(self, genes, densify):
        self.calls.append(("prepare_select", list(genes), bool(densify)))
        if self.fail_in_select:
            raise ValueError("injected")
        Y = self.staged[:, list(genes)].toarray()
        std = Y.std(axis=0, ddof=1)
        self.X = Y / np.where(std == 0, 1.0, std)
        self.shape = self.X.shape
        self.staged = None
        return std, self.X.sum(axis=1), self.X

    def prepare_release(self):
        self.released += 1
        self.staged = None

    def mu_frobenius_refit(self, H, tol=1e-4, max_iter=1000):
        self.calls.append(("mu_frobenius_refit", np.array(H), tol, max_iter))
        W, n, errs = R.mu_frobenius_refit(self.X, H, tol=tol, max_iter=max_iter)
        return W, n, float(errs[-1])


def reference_frame(seed=3):
    rs = np.random.RandomState(seed)
    genes = ["r%d" % j for j in range(10)]
    return pd.DataFrame(rs.gamma(0.8, 1.0, size=(3, 10)), index=["GEP1", "GEP2", "GEP3"], columns=genes)


def query_frame(genes, n=30, seed=4):
    rs = np.random.RandomState(seed)
    C = rs.poisson(2.0, size=(n, len(genes)))
    C[5] = 0
    return pd.DataFrame(C, index=["q%d" % i for i in range(n)], columns=genes)


def test_overlap_follows_the_reference_order_and_counts_the_missing():
    ref = reference_frame()
    qgenes = ["r8", "x1", "r0", "r5", "x2", "r3", "r9", "r1"]                # r2 r4 r6 r7 missing, two foreign genes
    q = query_frame(qgenes)
    eng = NumpyEngine()
    star = StarCAT(ref, engine=eng)
    usage, raw = star.fit_transform(q, tol=1e-5, max_iter=300, return_unnormalized=True)
    overlap = ["r0", "r1", "r3", "r5", "r8", "r9"]
    assert list(star.overlap_genes) == overlap and star.n_missing == 4
    assert eng.calls[0] == ("prepare_select", [qgenes.index(g) for g in overlap], True)
    kind, H, tol, max_iter = eng.calls[1]
    assert kind == "mu_frobenius_refit" and np.array_equal(H, ref[overlap].values) and (tol, max_iter) == (1e-5, 300)
    assert eng.released == 1 and eng.staged is None
    assert list(usage.index) == list(q.index) and list(usage.columns) == ["GEP1", "GEP2", "GEP3"]
    # rows sum to 1; the cell without counts keeps all-zero usages instead of 0 / 0
    assert not raw.values[5].any() and not usage.values[5].any()
    live = np.arange(len(q)) != 5
    assert np.allclose(usage.values[live].sum(axis=1), 1.0, rtol=1e-12) and np.isfinite(usage.values).all()
    assert np.allclose(usage.values[live], raw.values[live] / raw.values[live].sum(axis=1, keepdims=True), rtol=1e-14)
    # a sparse query is not densified; without return_unnormalized only the normalised frame comes back
    only = star.fit_transform((sp.csr_matrix(q.values), q.index, q.columns), tol=1e-5, max_iter=300)
    assert eng.calls[2][2] is False and np.array_equal(only.values, usage.values)


def test_argument_errors_need_no_device():
    ref = reference_frame()
    star = StarCAT(ref, device=0)                                            # no engine is created for any of these
    q = query_frame(["r1", "r2", "r1"])
    with pytest.raises(ValueError, match="duplicate gene names in the query"):
        star.fit_transform(q)
    with pytest.raises(ValueError, match="shares no gene"):
        star.fit_transform(query_frame(["x1", "x2"]))
    assert star.n_missing == 10 and len(star.overlap_genes) == 0 and star._engine is None
    neg = ref.copy()
    neg.iloc[1, 2] = -0.5
    with pytest.raises(ValueError, match="Negative values"):
        StarCAT(neg)
    with pytest.raises(TypeError):
        StarCAT(ref.values)


def test_non_finite_reference_genes_are_dropped_with_a_warning(tmp_path):
    ref = reference_frame()
    ref.iloc[0, 4] = np.inf
    ref.iloc[2, 7] = np.nan
    with pytest.warns(UserWarning, match="dropping 2 reference genes"):
        star = StarCAT(ref)
    assert list(star.reference.columns) == [g for g in ref.columns if g not in ("r4", "r7")]
    # the two files build_reference writes are read back alike
    clean = reference_frame()
    save_df_to_npz(clean, str(tmp_path / "ref.df.npz"))
    save_df_to_text(clean, str(tmp_path / "ref.txt"))
    for path in (str(tmp_path / "ref.df.npz"), tmp_path / "ref.txt"):
        got = StarCAT(path).reference
        assert list(got.index) == list(clean.index) and list(got.columns) == list(clean.columns)
        assert np.array_equal(got.values, clean.values)                         # (the text is parsed round-trip exact)


def test_the_staging_is_released_after_an_error():
    eng = NumpyEngine(fail_in_select=True)
    star = StarCAT(reference_frame(), engine=eng)
    with pytest.raises(ValueError, match="injected"):
        star.fit_transform(query_frame(["r0", "r1", "r2"]))
    assert eng.released == 1 and eng.staged is None


# ---------------------------------------------------------------- the solver pairs cNMF admits
def test_check_kwargs_admits_mu_frobenius_as_a_refit_only(tmp_path):
    obj = cNMF(output_dir=str(tmp_path), name="kw")
    H = np.ones((2, 3))
    for beta in ("frobenius", 2):
        obj._check_kwargs(dict(solver="mu", beta_loss=beta, update_H=False, H=H))
        with pytest.raises(NotImplementedError, match="only as a refit"):
            obj._check_kwargs(dict(solver="mu", beta_loss=beta, n_components=2))
        with pytest.raises(NotImplementedError, match="only as a refit"):
            obj._check_kwargs(dict(solver="mu", beta_loss=beta, n_components=2, update_H=True))
    obj._check_kwargs(dict(solver="cd", beta_loss="frobenius"))
    obj._check_kwargs(dict(solver="mu", beta_loss="kullback-leibler"))
    with pytest.raises(NotImplementedError):
        obj._check_kwargs(dict(solver="cd", beta_loss="kullback-leibler"))
