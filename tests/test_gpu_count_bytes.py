"""The count plane as bytes (CountU8, kernels_planes.hip.h; the byte form of the 16x16x32 body, kernels_gemm2h.hip.h):
one byte per count, five LDS-DMA pieces per 32-k step, the conversion to f16 in registers.  Everything here is exact:
the byte form must give the bits the f16 plane gives -- in exact integer arithmetic through the debug entry point, against
the f16 plane on the same operands, and through the engine against ``CNMF_G2_U8=0``."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# 2, 4, 6 and 10 steps of 32 k: only the prologue; the first steady-state steps; the three-image ring wrapping at a step count
# that is not a multiple of three; and (2048: 64 steps) a full-length segment
KS = (64, 128, 192, 320)
JS = (1, 17, 256, 300)       # one column, a ragged tile, a whole tile, two tiles
NSPLITS = (1, 3)
VARS = (0, 4)                # the burst loop and the spread stream


def _nsub(var):
    return 2 | (var << 4)


def _bytes_B(rs, J, K):
    """integers in [0, 255], 0 and 255 present in every row"""
    B = rs.randint(0, 256, size=(J, K)).astype(np.float32)
    cols = np.stack([rs.permutation(K)[:2] for _ in range(J)])
    B[np.arange(J), cols[:, 0]] = 0.0
    B[np.arange(J), cols[:, 1]] = 255.0
    return B


def _exact(engine, A, B, ns, var):
    out, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=_nsub(var), count_bytes=True)
    out2, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=_nsub(var), count_bytes=True)
    assert np.array_equal(out, out2)                            # the same call twice: the same bits
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    bad = np.argwhere(out.astype(np.float64) != ref)
    assert bad.size == 0, (A.shape, B.shape, ns, var, len(bad), bad[:8].tolist())
    return out


def _small_A(rs, K):
    """integers <= 32 times a power of two per row, one row zero"""
    A = rs.randint(0, 33, size=(256, K)).astype(np.float32)
    A *= np.exp2(rs.randint(-20, 21, size=(256, 1))).astype(np.float32)
    A[37] = 0.0
    return A


@pytest.mark.parametrize("var", VARS)
@pytest.mark.parametrize("ns", NSPLITS)
@pytest.mark.parametrize("K", KS + (2048,))
def test_integer_product_is_exact(engine, K, ns, var):
    """A = integers <= 32 times a power of two per row (one row zero), B = integers in [0, 255] with 0 and 255 in every row:
    every partial sum is below 2048 * 32 * 255 < 2^24 (times the row's power of two), so float32 accumulation in any order
    gives the integer product exactly.  A piece waited for too late, or an image read before it landed, shows here."""
    rs = np.random.RandomState(1000 * K + 10 * ns + var)
    for J in (JS if K != 2048 else (256,)):
        A, B = _small_A(rs, K), _bytes_B(rs, J, K)
        out = _exact(engine, A, B, ns, var)
        assert not out[37].any()


@pytest.mark.parametrize("var", VARS)
@pytest.mark.parametrize("ns", NSPLITS)
@pytest.mark.parametrize("value", [1.0, 4097.0])
@pytest.mark.parametrize("K", KS)
def test_one_hot_rows_pick_single_elements(engine, K, value, ns, var):
    """The construction of tests/test_gpu_gemm2h_mfma16.py: row c of A holds ONE entry, at k0(c), so output (c, j) must be
    value * B[j, k0(c)].  B[j, k] = (j K + k) mod 256 at J = 300: every byte value and every (lane, k slot) of the count
    fragments is pinned to one element (4097 = 2^12 + 1 rides on both factor planes; products <= 4097 * 255: exact)."""
    k0 = (np.arange(256) * 5 + 3 + (np.arange(256) // K)) % K
    A = np.zeros((256, K), np.float32)
    A[np.arange(256), k0] = value
    J = 300
    B = ((np.arange(J)[:, None] * K + np.arange(K)[None, :]) % 256).astype(np.float32)
    _exact(engine, A, B, ns, var)


@pytest.mark.parametrize("var", VARS)
@pytest.mark.parametrize("J", (17, 300))
@pytest.mark.parametrize("K", (192, 320))
def test_same_bits_as_the_f16_plane(engine, K, J, var):
    """Random non-integer A, rows scaled by 2^+-20, B integers in [0, 255]: the byte plane and the f16 plane feed the MFMAs
    the same operands in the same order -- the same bits, whatever the rounding of the sums."""
    rs = np.random.RandomState(31 * K + J + var)
    A = rs.gamma(0.7, 1.0, size=(256, K)).astype(np.float32)
    A *= np.exp2(rs.randint(-20, 21, size=(256, 1))).astype(np.float32)
    B = _bytes_B(rs, J, K)
    for ns in NSPLITS:
        a, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=_nsub(var), count_bytes=True)
        b, _ = engine.debug_gemm2h(A, B, nsplit=ns, nsub=_nsub(var), count_bytes=False)
        assert np.array_equal(a, b), (K, J, var, ns, int((a != b).sum()))


def test_byte_plane_refuses_a_count_above_255(engine):
    A = np.ones((256, 64), np.float32)
    B = np.full((3, 64), 7.0, np.float32)
    B[1, 5] = 256.0
    with pytest.raises(ValueError):
        engine.debug_gemm2h(A, B, nsub=2, count_bytes=True)


def _run(engine, X, ks, seeds, max_iter, kc_max, tol):
    engine.set_matrix(X)
    H, W, n_iter, viol = engine.nmf_batch(ks, seeds=seeds, tol=tol, max_iter=max_iter, kc_max=kc_max, warn=False, return_W=True)
    return H, W, np.asarray(n_iter), np.asarray(viol), dict(engine.last_stats), engine.matrix_images()


def _bytes_against_f16(engine, monkeypatch, X, ks, seeds, max_iter, kc_max, tol=0.0, expect_bytes=True):
    """the job with the knob unset and with CNMF_G2_U8=0: every bit of every result equal; the statistics of the default run"""
    H, W, n_iter, viol, st, img = _run(engine, X, ks, seeds, max_iter, kc_max, tol)
    assert st["gemm_mode"] == 4 and img["count_planes"] and img["count_planes_bytes"] == expect_bytes, (st, img)
    monkeypatch.setenv("CNMF_G2_U8", "0")
    H0, W0, n0, viol0, st0, img0 = _run(engine, X, ks, seeds, max_iter, kc_max, tol)
    monkeypatch.delenv("CNMF_G2_U8")
    assert st0["gemm_mode"] == 4 and img0["count_planes"] and not img0["count_planes_bytes"], (st0, img0)
    assert np.array_equal(n_iter, n0) and np.array_equal(viol, viol0)
    assert all(np.array_equal(a, b) for a, b in zip(H, H0))
    assert all(np.array_equal(a, b) for a, b in zip(W, W0))
    return st, n_iter


def test_engine_split_k_passes(engine, monkeypatch):
    """Job "B" of tests/test_gpu_schedule_pins.py: 1024 x 520 Poisson at 256 packed columns, 3 iterations -- both passes split-K."""
    from test_gpu_schedule_pins import jobs
    XB, _, calls = jobs()["B"]
    ks, seeds, kc_max = calls[1]
    assert kc_max == 256
    st, n_iter = _bytes_against_f16(engine, monkeypatch, XB, ks, seeds, 3, kc_max)
    assert st["kc"] == 256 and (n_iter == 3).all()


def test_engine_stream_k_pass_a(engine, monkeypatch):
    """12 544 x 520 Poisson(1.5) at 1024 packed columns, 2 iterations: pass A is the stream-K launch with cut planes."""
    rs = np.random.RandomState(12544)
    X = rs.poisson(1.5, size=(12544, 520)).astype(np.float32)
    st, n_iter = _bytes_against_f16(engine, monkeypatch, X, [9] * 114, list(range(1, 115)), 2, 0)
    assert st["kc"] == 1024 and (n_iter == 2).all()


def test_engine_partial_tiles_in_the_tail(engine, monkeypatch):
    """CNMF_PART=1 and a job that ends in a tail: the 150 restarts of job "B" (about 1350 columns) at 1024 packed columns --
    once the first 1024 columns have finished nothing is left to refill the batch with, and the passes over the last third
    skip the dead 32-column tiles: the live-mask instantiation of the byte form."""
    from test_gpu_schedule_pins import jobs
    XB, _, calls = jobs()["B"]
    ks, seeds, kc_max = calls[0]
    monkeypatch.setenv("CNMF_PART", "1")
    st, n_iter = _bytes_against_f16(engine, monkeypatch, XB, ks, seeds, 6, kc_max)
    monkeypatch.delenv("CNMF_PART")
    assert st["kc"] == 1024 and st["tail_iterations"] > 0 and (n_iter == 6).all(), (st, n_iter)


@pytest.mark.parametrize("top, expect_bytes", [(255.0, True), (256.0, False)])
def test_eligibility_is_every_count_at_most_255(engine, monkeypatch, top, expect_bytes):
    """The 1024 x 520 matrix with one entry raised to 255 units (byte planes) and to 256 units (the f16 plane): both give the
    bits of CNMF_G2_U8=0."""
    from test_gpu_schedule_pins import jobs
    XB, _, calls = jobs()["B"]
    ks, seeds, kc_max = calls[1]
    X = XB.copy()
    X[500, 77] = top
    _bytes_against_f16(engine, monkeypatch, X, ks[:30], seeds[:30], 3, kc_max, expect_bytes=expect_bytes)
