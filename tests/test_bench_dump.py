"""`bench.py --dump-outputs DIR`: the files dump_outputs() writes from what the last timed step computed -- float32 /
float64 only, under the size budget, and the same files for the same results (the sample of a large output is fixed).
CPU only: the step's results are stood in for by seeded arrays."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step(G=50, per_k=20, ks=(5, 7, 9)):
    rng = np.random.default_rng(3)
    order = [k for k in ks for _ in range(per_k)]
    spectra = {(k, j): rng.random((k, G), dtype=np.float32) for j, k in enumerate(order)}
    return spectra, list(range(len(order))), np.arange(len(order)) + 10, rng.random(len(order))


def _read(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole(tmp_path):
    bench = _bench()
    spectra, restarts, n_iter, viol = _step()
    bench.dump_outputs(str(tmp_path), spectra, restarts, n_iter, viol)
    got = _read(str(tmp_path))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["n_iter.npy"], n_iter) and np.array_equal(got["violation.npy"], viol)
    for k in (5, 7, 9):
        ids = got["spectra_k%02d_restart.npy" % k].astype(int)
        assert len(ids) == 20 and got["spectra_k%02d.npy" % k].shape == (20, k, 50)
        assert all(np.array_equal(got["spectra_k%02d.npy" % k][i], spectra[(k, j)]) for i, j in enumerate(ids))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SPECTRA_BYTES", 40_000)
    spectra, restarts, n_iter, viol = _step()
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        bench.dump_outputs(d, spectra, restarts, n_iter, viol)
        runs.append(_read(d))
    assert runs[0].keys() == runs[1].keys()
    assert all(np.array_equal(runs[0][f], runs[1][f]) for f in runs[0])
    spectra_bytes = sum(a.nbytes for f, a in runs[0].items() if f.startswith("spectra_") and "restart" not in f)
    assert 0 < spectra_bytes <= 40_000
    for k in (5, 7, 9):
        ids = runs[0]["spectra_k%02d_restart.npy" % k].astype(int)
        assert 1 <= len(ids) < 20 and np.all(np.diff(ids) > 0)
        assert all(np.array_equal(runs[0]["spectra_k%02d.npy" % k][i], spectra[(k, j)]) for i, j in enumerate(ids))
