"""Preprocess.filter_adata / preprocess_for_cnmf on the device against the unmodified reference
(tests/golden/ref_filter.npz, tools/make_golden_filter.py).

Counts are integers, so every sum (n_cells, n_counts, the mitochondrial totals, the row sums) is exact in any order;
``pct_mito`` (one division), the row scale (one division) and the TP10K values (one product) are one rounding each: names,
masks, columns, CSR structure and value bits all equal the reference's.  adata_RNA divides by a standard deviation whose
float64 sums run in another order on the device than in numpy: its structure is equal and its values are held to 1e-12
(tests/test_gpu_preprocess.py's bound for the same step); that preprocess_for_cnmf forms them exactly as
normalize_batchcorrect does is pinned bit for bit."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from cnmf_amd.preprocess import Preprocess
from tests import _filter_ref as F

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_filter.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture
def P(engine):
    yield Preprocess(engine=engine)
    engine.preprocess_release()


@pytest.mark.parametrize("dense", [False, True], ids=["csr", "dense"])
@pytest.mark.parametrize("run", list(F.FILTER_RUNS))
def test_filter_adata_matches_the_reference(P, gold, run, dense):
    F.check_filter_run(P, gold, run, dense)


@pytest.mark.parametrize("dense", [False, True], ids=["csr", "dense"])
@pytest.mark.parametrize("run", ["single", "ftype", "list"])
def test_preprocess_for_cnmf_matches_the_reference(P, gold, run, dense):
    F.check_pf_run(P, gold, run, dense, rna_rtol=1e-12)


@pytest.mark.parametrize("dense", [False, True], ids=["csr", "dense"])
@pytest.mark.parametrize("run", ["single", "list"])
def test_rna_result_is_normalize_batchcorrect_bit_for_bit(P, run, dense):
    """the factored-out body on the staged (and, for 'single', device-restricted) counts against the method on its own,
    given the same RNA genes"""
    data, kw = F.pf_inputs(run, dense)
    res, _, hvgs = P.preprocess_for_cnmf(data, **kw)
    C, cells, genes, _, _, hv = F.make_inputs()
    if run == "single":
        from cnmf_amd.preprocess import make_unique_names
        genes = make_unique_names(genes)
        keep = ~genes.isin(F.EXCLUDE)
        C, genes, hv = C[:, keep], genes[keep], hv[keep]
    X = C if dense else sp.csr_matrix(C)
    alone, hvgs2 = P.normalize_batchcorrect((X, cells, list(genes)), obs=kw["obs"], highly_variable=hv, makeplots=False)
    assert hvgs == hvgs2
    if dense:
        assert np.array_equal(res.X.view(np.uint64), alone.X.view(np.uint64))
    else:
        assert F.same_csr(res.X, alone.X)


def test_two_calls_give_the_same_bits(P):
    outs = []
    for _ in range(2):
        data, kw = F.pf_inputs("ftype", False)
        res, tp, _ = P.preprocess_for_cnmf(data, **kw)
        C, cells, genes, _, _, _ = F.make_inputs()
        flt = P.filter_adata((sp.csr_matrix(C), cells, genes), **F.FILTER_RUNS["mito"])
        outs.append((res.X, tp.X, flt.X, flt.obs["pct_mito"].values, flt.obs["n_counts"].values))
    for a, b in zip(*outs):
        if sp.issparse(a):
            assert F.same_csr(a, b)
        else:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
