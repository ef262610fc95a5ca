"""The W half-step sweep at every rank it has a body of its own for (kernels_sweep.hip.h: one exact-rank body per rank
1..16, every factor / product / cut-plane access through a descriptor rebased to the slot with one shared 32-bit offset).

Spectra are held to the float64 oracle (oracle/nmf_cd.py) at the bars of tests/test_gpu_nmf.py: rows L2-normalised and
matched by best cosine, max-abs <= 1e-4 and relative Frobenius <= 1e-3, |delta n_iter| <= max(slack, n_ref // 100).

  * count path (the kernel that also writes the f16 planes: >= 256 packed columns): 1037 cells -- no multiple of 16, 64 or
    256, so the last chunk is partial, lanes are dead and the last 16-cell block lies past the padded length -- three
    restarts per rank 1..16 in one batch (408 columns);
  * the f32 pipe (the kernel without planes): a 300 x 170 gamma matrix, 128 columns, ranks 1..16;
  * stream-K cut tiles (the plane1 / plane2 loads): 12 500 cells x 1024 columns, the smallest shape at which the launcher
    cuts tiles, ranks 5..13 with slots straddling every component-group edge;
  * two runs of the first batch in one process return the same bytes.

Parity iteration by iteration (W, H and the violation ratio after 1, 2, 3 sweeps): tests/test_gpu_cd_steps.py.
"""
import numpy as np
import pytest

from cnmf_amd import synth
from oracle import nmf_cd

TOL_MAXABS = 1e-4
TOL_RELFRO = 1e-3
RANKS = list(range(1, 17))
MAX_ITER = 40               # bounded: every restart runs the same 40 outer iterations on both sides or stops within them


def _check(H_ref, n_ref, H, n, slack=2):
    maxabs, relfro = nmf_cd.spectra_error(H_ref, H)
    print("k=%d maxabs=%.3g relfro=%.3g n_ref=%d n=%d" % (H_ref.shape[0], maxabs, relfro, n_ref, n))
    assert np.isfinite(H).all()
    assert maxabs <= TOL_MAXABS and relfro <= TOL_RELFRO, (maxabs, relfro, n_ref, n)
    assert abs(int(n) - int(n_ref)) <= max(slack, n_ref // 100), (n_ref, n)


def _seeds(rs, n):
    return [int(s) for s in rs.randint(1, 2**31 - 1, size=n)]


@pytest.fixture(scope="module")
def counts_1037():
    return synth.make_config("C3", dtype=np.float64, n_cells=1037)


@pytest.fixture(scope="module")
def count_batch(engine, counts_1037):
    """(ks, seeds, H, n_iter, viol) of the one count-path batch every rank's test reads (left unchanged)"""
    ks = RANKS * 3
    seeds = _seeds(np.random.RandomState(41), len(ks))
    engine.set_matrix(counts_1037)
    H, _, n_iter, viol = engine.nmf_batch(ks, seeds=seeds, max_iter=MAX_ITER, warn=False)
    assert sum(ks) == 408 and engine.last_stats["kc"] >= 256 and engine.last_stats["gemm_mode"] == 4, engine.last_stats
    return ks, seeds, H, n_iter, viol


def test_oracle_is_finite_and_non_degenerate_at_the_edge_ranks(counts_1037):
    """The reference the rank tests lean on, at its two ends (no GPU): finite factors, no dead component, and distinct
    components at rank 16 (a degenerate oracle would make the cosine matching of spectra_error meaningless)."""
    for k in (1, 16):
        W, H, n = nmf_cd.nmf(counts_1037, k, seed=12345, max_iter=MAX_ITER)
        assert np.isfinite(W).all() and np.isfinite(H).all() and 1 <= n <= MAX_ITER
        norms = np.linalg.norm(H, axis=1)
        assert (norms > 0).all() and (W.max(axis=0) > 0).all()
        if k > 1:
            Hn = H / norms[:, None]
            cos = Hn @ Hn.T - np.eye(k)
            assert cos.max() < 0.999, cos.max()


@pytest.mark.gpu
@pytest.mark.parametrize("k", RANKS)
def test_count_path_every_rank_matches_oracle(count_batch, counts_1037, k):
    ks, seeds, H, n_iter, _ = count_batch
    mine = [i for i, kk in enumerate(ks) if kk == k]
    assert len(mine) == 3
    for i in mine:
        assert H[i].shape == (k, counts_1037.shape[1])
        _, H_ref, n_ref = nmf_cd.nmf(counts_1037, k, seed=seeds[i], max_iter=MAX_ITER)
        _check(H_ref, n_ref, H[i], n_iter[i])


@pytest.mark.gpu
def test_count_path_batch_is_deterministic(engine, count_batch, counts_1037):
    ks, seeds, H, n_iter, viol = count_batch
    engine.set_matrix(counts_1037)
    H2, _, n2, viol2 = engine.nmf_batch(ks, seeds=seeds, max_iter=MAX_ITER, warn=False)
    assert list(n2) == list(n_iter) and np.asarray(viol2).tobytes() == np.asarray(viol).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(H, H2))


@pytest.mark.gpu
def test_f32_pipe_every_rank_matches_oracle(engine):
    """The W kernel without planes (gemm_mode 0): 136 columns of ranks 1..16 through a 128-column batch (one refill)."""
    rs = np.random.RandomState(5)
    X = rs.gamma(0.4, 1.0, size=(300, 170)).astype(np.float32)
    seeds = _seeds(rs, len(RANKS))
    engine.set_matrix(X)
    H, _, n_iter, _ = engine.nmf_batch(RANKS, seeds=seeds, max_iter=100, warn=False, kc_max=128)
    assert engine.last_stats["kc"] == 128 and engine.last_stats["gemm_mode"] == 0, engine.last_stats
    X64 = X.astype(np.float64)
    for k, seed, h, n in zip(RANKS, seeds, H, n_iter):
        _, H_ref, n_ref = nmf_cd.nmf(X64, k, seed=seed, max_iter=100)
        _check(H_ref, n_ref, h, n)


@pytest.mark.gpu
def test_stream_k_cut_tiles_match_oracle(engine):
    """12 500 cells x 1024 columns = 196 pass-A tiles: the f16 kernels' stream-K launcher cuts tiles, and the W sweep adds
    the partial planes of a cut tile through its slot-relative descriptors.  Ranks 5..13, packed in order, with a slot
    across each of the three component-group edges (256, 512, 768) -- those take the two cut flags of one slot."""
    rs = np.random.RandomState(7)
    ks, total = [], 0
    while True:
        k = int(rs.randint(5, 14))
        if total + k > 1024:
            break
        ks.append(k)
        total += k
    ends = np.cumsum(ks)
    for edge in (256, 512, 768):
        assert any(e - k < edge < e for e, k in zip(ends, ks)), (edge, "no slot straddles it")
    seeds = _seeds(rs, len(ks))
    X = synth.make_config("C3", dtype=np.float32, n_cells=12500)
    engine.set_matrix(X)
    H, _, n_iter, _ = engine.nmf_batch(ks, seeds=seeds, max_iter=6, warn=False, kc_max=1024)
    assert engine.last_stats["kc"] == 1024 and engine.last_stats["gemm_mode"] == 4, engine.last_stats
    X64 = X.astype(np.float64)
    straddlers = [i for i, (e, k) in enumerate(zip(ends, ks)) if any(e - k < edge < e for edge in (256, 512, 768))]
    for i in sorted(set(straddlers + list(range(0, len(ks), 40)))):
        _, H_ref, n_ref = nmf_cd.nmf(X64, ks[i], seed=seeds[i], max_iter=6)
        _check(H_ref, n_ref, H[i], n_iter[i])
