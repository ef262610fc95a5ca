"""`bench.py --dump-outputs DIR` end to end: the files hold what the bench's LAST timed step computed -- the restarts of
that step's job (ledger rows step * restarts_per_k ... of every K, sharded idx % world), each under its own index in the
job -- checked against the engine run on the same matrix with the same ledger seeds, one call per shard exactly as the
bench batches them (the packing of a batch decides the last bits of a result, tests/test_gpu_determinism.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cnmf_amd import synth
from cnmf_amd.cnmf import ledger_seeds, worker_filter
from cnmf_amd.engine import Engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, RPK, STEPS, WARMUP, CELLS = [5, 6], 3, 2, 1, 400


def _bench(args, env, out):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "CNMF_GATHER", "CNMF_BENCH_BACKEND", "CNMF_RCCL_ID_FILE"):
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(STEPS), "--warmup", str(WARMUP), "--workload", "C1",
           "--n-cells", str(CELLS), "--kmin", str(KS[0]), "--kmax", str(KS[-1]), "--restarts-per-k", str(RPK),
           "--dump-outputs", str(out)] + args
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}


def _expected(shards, world):
    """{job index: (k, spectra, n_iter, violation)} for the last timed step, one engine call per shard."""
    step = WARMUP + STEPS - 1
    led = ledger_seeds(KS, RPK * (WARMUP + STEPS), 14)
    ks, seeds = [], []
    for k in KS:
        ks += [k] * RPK
        seeds += [int(s) for (kk, _, s) in led if kk == k][step * RPK:(step + 1) * RPK]
    C, _ = synth.topic_counts(CELLS, *synth.CONFIGS["C1"][1:])
    X = synth.normalise_like_prepare(C, dtype=np.float32)
    out = {}
    with Engine(0) as eng:
        eng.set_matrix(X)
        for r in shards:
            mine = list(worker_filter(range(len(ks)), r, world))
            H, _, n_it, viol = eng.nmf_batch([ks[i] for i in mine], seeds=[seeds[i] for i in mine], warn=False)
            for i, j in enumerate(mine):
                out[j] = (ks[j], H[i], n_it[i], viol[i])
    return out


def _check(got, exp):
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    ids = sorted(exp)
    assert got["restart"].tolist() == ids
    assert got["n_iter"].tolist() == [float(exp[j][2]) for j in ids]
    np.testing.assert_array_equal(got["violation"], [exp[j][3] for j in ids])
    for k in KS:
        mine = [j for j in ids if exp[j][0] == k]
        assert got["spectra_k%02d_restart" % k].tolist() == mine
        np.testing.assert_array_equal(got["spectra_k%02d" % k], np.stack([exp[j][1] for j in mine]))


def test_dump_outputs_single_gpu(tmp_path):
    _check(_bench([], {}, tmp_path / "dump"), _expected([0], 1))


def test_dump_outputs_emulated_shard(tmp_path):
    """--emulate-rank 1/2: the files carry the odd rows of the job under their indices in the WHOLE job."""
    exp = _expected([1], 2)
    assert sorted(exp) == list(range(1, len(KS) * RPK, 2))
    _check(_bench(["--emulate-rank", "1/2"], {}, tmp_path / "dump"), exp)


def test_dump_outputs_two_ranks(tmp_path):
    """--gpus 2 (both ranks on the one GPU, over gloo): every restart of the job, spectra and per-restart files alike."""
    got = _bench(["--gpus", "2"], dict(CNMF_BENCH_BACKEND="gloo", CNMF_BENCH_ONE_GPU="1", CNMF_GATHER="torch"),
                 tmp_path / "dump")
    _check(got, _expected([0, 1], 2))
