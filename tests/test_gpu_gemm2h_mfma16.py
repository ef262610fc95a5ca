"""The production count path (kernels_gemm2h.hip.h, two 16-k blocks per step, one count plane) on
v_mfma_f32_16x16x32_f16: the fragment / accumulator mapping in exact arithmetic, and both launches (split-K and
stream-K with cut planes) through the engine against the exact-f32 pipe."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KS = (64, 128, 192)          # 2, 4 and 6 steps of 32 k: at and past the three-image prologue (no / some steady-state steps)
JS = (1, 17, 256, 300)       # one column, a ragged tile, a whole tile, two tiles
NSPLITS = (1, 3)


def _exact(engine, A, B, ns):
    out, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=2)
    out2, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=2)
    assert np.array_equal(out, out2)                            # the same call twice: the same bits
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    bad = np.argwhere(out.astype(np.float64) != ref)
    assert bad.size == 0, (A.shape, B.shape, ns, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("ns", NSPLITS)
@pytest.mark.parametrize("K", KS)
def test_integer_product_is_exact(engine, K, ns):
    """A = integers <= 1024 times a power of two per row (one row zero), B = integers <= 15: every partial sum is below
    192 * 1024 * 15 < 2^24 (times the row's power of two), so float32 accumulation in any order gives the integer product."""
    rs = np.random.RandomState(1000 * K + ns)
    for J in JS:
        A = rs.randint(0, 1025, size=(256, K)).astype(np.float32)
        A *= np.exp2(rs.randint(-20, 21, size=(256, 1))).astype(np.float32)
        A[37] = 0.0
        B = rs.randint(0, 16, size=(J, K)).astype(np.float32)
        _exact(engine, A, B, ns)
        assert not engine.debug_gemm2h(A, B, nsplit=ns, nsub=2)[0][37].any()


@pytest.mark.parametrize("ns", NSPLITS)
@pytest.mark.parametrize("value", [1.0, 4097.0])
@pytest.mark.parametrize("K", KS)
def test_one_hot_rows_pick_single_elements(engine, K, value, ns):
    """Row c of A holds ONE entry, at k0(c): output (c, j) must be value * B[j, k0(c)] -- every (lane, k slot) of the factor
    fragments pinned to one element of the count fragments.  value 4097 = 2^12 + 1 does not fit one f16 plane: the large
    plane carries 4096 and the small plane the 1, so both planes' fragments are pinned (products <= 4097 * 15: exact)."""
    rs = np.random.RandomState(7 * K + ns)
    k0 = (np.arange(256) * 5 + 3 + (np.arange(256) // K)) % K    # every k of the step taken by some row of every 16-row tile group
    A = np.zeros((256, K), np.float32)
    A[np.arange(256), k0] = value
    for J in JS:
        B = rs.randint(0, 16, size=(J, K)).astype(np.float32)
        _exact(engine, A, B, ns)


def _against_f32_pipe(engine, monkeypatch, X, ks, seeds, max_iter, kc_max):
    engine.set_matrix(X)
    H, _, n_iter, _ = engine.nmf_batch(ks, seeds=seeds, tol=0.0, max_iter=max_iter, kc_max=kc_max, warn=False)
    st = dict(engine.last_stats)
    assert st["gemm_mode"] == 4 and (np.asarray(n_iter) == max_iter).all()
    monkeypatch.setenv("CNMF_GEMM3", "0")
    engine.set_matrix(X)
    H0, _, _, _ = engine.nmf_batch(ks, seeds=seeds, tol=0.0, max_iter=max_iter, kc_max=kc_max, warn=False)
    assert engine.last_stats["gemm_mode"] == 0
    monkeypatch.delenv("CNMF_GEMM3")
    # the bound tests/test_gpu_nmf.py::test_count_structured_detection_and_f16_path holds the count path to against this pipe
    for a, b in zip(H, H0):
        assert np.abs(a - b).max() <= 1e-4 * max(1.0, np.abs(b).max())
    return st


def test_split_k_launch_matches_f32_pipe(engine, monkeypatch):
    """The 1024 x 520 Poisson matrix of tests/test_gpu_schedule_pins.py at 256 packed columns: both passes are split-K launches."""
    from test_gpu_schedule_pins import jobs
    XB, _, calls = jobs()["B"]
    ks, seeds, kc_max = calls[1]
    assert kc_max == 256
    st = _against_f32_pipe(engine, monkeypatch, XB, ks, seeds, 3, kc_max)
    assert st["kc"] == 256


def test_stream_k_launch_matches_f32_pipe(engine, monkeypatch):
    """12 544 cells x 520 genes at 1024 packed columns: pass A is the stream-K launch over 49 x 4 = 196 tiles, with cut planes."""
    rs = np.random.RandomState(12544)
    X = rs.poisson(1.5, size=(12544, 520)).astype(np.float32)
    ks = [9] * 114                                               # 1026 columns: the full width, one restart queued
    st = _against_f32_pipe(engine, monkeypatch, X, ks, list(range(1, 115)), 2, 0)
    assert st["kc"] == 1024
