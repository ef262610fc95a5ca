"""Fixed seeded jobs through whichever build of the library CNMF_LIB_PATH names, for bit-identity A/B runs of two builds:
    CNMF_LIB_PATH=/path/to/libcnmf_hip.so [CNMF_GEMM3=2 ...] python tools/ab_identity.py wide|general|f32|mode|init|streamk|streamk_general
Prints one JSON line: SHA-256 digests of everything the job's batch calls returned (H, n_iter, viol) and of the
last_stats fields that describe the schedule.  One process per library and per knob value; the lines must be equal."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cnmf_amd import synth  # noqa: E402
from cnmf_amd.engine import Engine  # noqa: E402

STATS = ("kc", "nsplit", "gemm_mode", "outer_iterations", "column_iterations", "restart_iterations", "tail_iterations",
         "tail_live_columns")


def draw(rs, n, lo=5, hi=14):
    return [int(k) for k in rs.randint(lo, hi, size=n)], [int(s) for s in rs.randint(1, 2**31 - 1, size=n)]


def calls(job):
    """(matrix, [keyword arguments of one nmf_batch call, ...]) of a job"""
    rs = np.random.RandomState(5)
    if job in ("wide", "mode", "init"):            # count path; 150 restarts: 1024 columns, refill, defragmentation, 768 / 512 / 256, f32 tail
        X = synth.make_config("C3", dtype=np.float32, n_cells=6000)
        if job == "init":                           # caller-supplied factors of very different size (the exponent guess of the W planes)
            ks = [40, 64, 50, 30, 60, 45, 33]
            W0 = [np.abs(rs.standard_normal((X.shape[0], k))).astype(np.float32) * np.float32(10.0 ** (i - 3)) for i, k in enumerate(ks)]
            H0 = [np.abs(rs.standard_normal((k, X.shape[1]))).astype(np.float32) for k in ks]
            return X, [dict(ks=ks, W0=W0, H0=H0, max_iter=40)]
        ks, seeds = draw(rs, 150 if job == "wide" else 44)
        return X, [dict(ks=ks, seeds=seeds, max_iter=60)]
    if job == "general":                            # tests/test_gpu_nmf.py: the perturbed matrix, 256 and 1024 columns
        X = synth.make_config("C3", dtype=np.float32, n_cells=9000)
        X = (X * np.exp(0.3 * rs.standard_normal((X.shape[0], 1)))).astype(np.float32) + np.float32(0.003)
        out = []
        for n, kc in ((40, 256), (150, 1024)):
            ks, seeds = draw(rs, n)
            out.append(dict(ks=ks, seeds=seeds, max_iter=60, kc_max=kc))
        return X, out
    if job in ("streamk", "streamk_general"):      # 12 500 cells x 1024 columns = 196 pass-A tiles: the stream-K launcher of the f16 kernels
        X = synth.make_config("C3", dtype=np.float32, n_cells=12500)
        if job == "streamk_general":
            X = (X * np.exp(0.3 * rs.standard_normal((X.shape[0], 1)))).astype(np.float32) + np.float32(0.003)
        ks, seeds = draw(rs, 150)
        return X, [dict(ks=ks, seeds=seeds, max_iter=60, kc_max=1024)]
    if job == "f32":                                # ragged: the f32 pipe at every rank tier, then a 128-column batch that refills
        X = rs.gamma(0.4, 1.0, size=(300, 170)).astype(np.float32)
        out = []
        for ks in ([3, 16, 33, 65, 128], [96, 33, 16, 65, 3]):
            out.append(dict(ks=ks, seeds=draw(rs, len(ks))[1], max_iter=100))
        out.append(dict(ks=[9] * 40, seeds=draw(rs, 40)[1], max_iter=100, kc_max=128))
        return X, out
    raise SystemExit("unknown job %r" % job)


def main():
    job = sys.argv[1]
    X, jobs = calls(job)
    eng = Engine(0)
    eng.set_matrix(X)
    h = {name: hashlib.sha256() for name in ("H", "n_iter", "viol") + STATS}
    seen = []
    for kw in jobs:
        H, _, n_iter, viol = eng.nmf_batch(kw.pop("ks"), warn=False, **kw)
        for a in H:
            h["H"].update(np.ascontiguousarray(a).tobytes())
        h["n_iter"].update(np.ascontiguousarray(n_iter, dtype=np.int32).tobytes())
        h["viol"].update(np.ascontiguousarray(viol, dtype=np.float64).tobytes())
        for name in STATS:
            h[name].update(str(int(eng.last_stats[name])).encode() + b";")
        seen.append({name: int(eng.last_stats[name]) for name in ("kc", "gemm_mode", "outer_iterations", "tail_iterations")})
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("CNMF_") and k != "CNMF_LIB_PATH"}
    print(json.dumps({"job": job, "env": env, "seen": seen,
                      "sha256": {name: d.hexdigest() for name, d in h.items()}}))


if __name__ == "__main__":
    main()
