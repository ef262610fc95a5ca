"""The slot refill of the multiplicative-update batch (cnmf_amd/csrc/mu_sched.h, mu_host.hip.h): more restarts of one
padded rank than the 32 slots hold, so slots retire beside live ones, wait for the next aligned point and are installed
again.  A restart's result must not depend on the slot, the round or the company it ran in (bit for bit against a call
of its own), one refilled restart is held to the float64 oracle under the bounds of test_gpu_mu.py, and the iteration
counts are pinned (tests/golden/mu_pins.json, recorded before the driver was split into scheduler and launches)."""
import json
import os

import numpy as np
import pytest

from cnmf_amd import synth
from oracle import nmf_cd, nmf_mu
from test_gpu_mu_sparse import _sparse_counts

pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mu_pins.json")

# 70 Kullback-Leibler restarts, all at padded rank 16: a first fill of 32 slots and two refills.  The float64 oracle stops
# the first 24 of them after 50 ... 200 iterations, so slots retire at different aligned points.
DENSE_KS = [2 + (7 * i) % 15 for i in range(70)]
DENSE_SEEDS = [1000 + i for i in range(70)]
DENSE_ALONE = (0, 31, 32, 45, 69)          # first slot, last of the first fill, two installed by a refill, the last one
# 40 restarts of ranks 3..16 on the non-zero path: one refill
SPARSE_KS = [3 + i % 14 for i in range(40)]
SPARSE_SEEDS = [2000 + i for i in range(40)]
SPARSE_ALONE = (0, 33, 39)


def dense_matrix():
    return synth.make_config("C1", dtype=np.float64, n_cells=700)             # 700 x 500, 76 % non-zero: the dense matrix pipe


def sparse_matrix():
    return _sparse_counts(1200, 900, 4.6, seed=1200)


def run_dense(engine, idx=None):
    idx = range(70) if idx is None else idx
    return engine.nmf_mu_batch([DENSE_KS[i] for i in idx], seeds=[DENSE_SEEDS[i] for i in idx], max_iter=200,
                               return_W=True, warn=False)


def run_sparse(engine, idx=None):
    idx = range(40) if idx is None else idx
    return engine.nmf_mu_batch([SPARSE_KS[i] for i in idx], seeds=[SPARSE_SEEDS[i] for i in idx], max_iter=60,
                               return_W=True, warn=False)


@pytest.fixture(scope="module")
def X():
    return dense_matrix()


@pytest.fixture(scope="module")
def dense_batch(engine, X):
    engine.set_matrix(X)
    return run_dense(engine)


@pytest.fixture(scope="module")
def pins():
    return json.load(open(PINS))


def test_slots_retire_at_different_aligned_points(dense_batch, pins):
    n_iter = [int(n) for n in dense_batch[2]]
    assert len(set(n_iter)) >= 3 and min(n_iter) < 200, sorted(set(n_iter))       # (else no slot is refilled beside live ones)
    assert all(n == 200 or n % 10 == 0 for n in n_iter)
    assert n_iter == pins["dense_n_iter"]


def test_refilled_restarts_equal_their_single_calls(engine, X, dense_batch):
    H, W, n_iter, err = dense_batch
    engine.set_matrix(X)
    for i in DENSE_ALONE:
        H1, W1, n1, e1 = run_dense(engine, [i])
        assert int(n1[0]) == int(n_iter[i]) and float(e1[0]) == float(err[i]), i
        np.testing.assert_array_equal(H1[0], H[i])
        np.testing.assert_array_equal(W1[0], W[i])


def test_a_refilled_restart_vs_oracle(X, dense_batch):
    H, W, n_iter, err = dense_batch
    i = 32                                                                         # installed by the first refill
    W_ref, H_ref, n_ref = nmf_mu.nmf_mu(X, DENSE_KS[i], seed=DENSE_SEEDS[i], max_iter=200)
    assert abs(int(n_iter[i]) - n_ref) <= 10, (n_iter[i], n_ref)
    if int(n_iter[i]) != n_ref:
        W_ref, H_ref, _ = nmf_mu.nmf_mu(X, DENSE_KS[i], seed=DENSE_SEEDS[i], max_iter=int(n_iter[i]), tol=0.0)
    maxabs, relfro = nmf_cd.spectra_error(H_ref, H[i])
    assert maxabs <= 1e-4 and relfro <= 1e-3, (maxabs, relfro)
    assert np.abs(W[i] - W_ref).max() <= 2e-3 * np.abs(W_ref).max()
    ref_err = nmf_mu.beta_divergence(X, W_ref, H_ref, 1, square_root=True)
    assert abs(err[i] - ref_err) <= 2e-3 * ref_err


def test_refill_on_the_non_zero_path(engine, monkeypatch, pins):
    engine.set_matrix(sparse_matrix())
    monkeypatch.setenv("CNMF_MU_SPARSE", "1")
    H, W, n_iter, err = run_sparse(engine)
    assert engine.matrix_images()["non_zero_images_16"]
    assert [int(n) for n in n_iter] == pins["sparse_n_iter"]
    for i in SPARSE_ALONE:
        H1, W1, n1, e1 = run_sparse(engine, [i])
        assert int(n1[0]) == int(n_iter[i]) and float(e1[0]) == float(err[i]), i
        np.testing.assert_array_equal(H1[0], H[i])
        np.testing.assert_array_equal(W1[0], W[i])
