"""The schedule of the restart loop, pinned: two jobs whose schedule does not depend on the numerics (``tol = 0`` and a
small ``max_iter``: every restart runs exactly ``max_iter`` iterations) must report the batch statistics recorded in
tests/golden/schedule_pins.json -- width, operand scheme, outer / column / restart iterations and the tail figures.
The same file is replayed on the CPU against the scheduler alone (tests/test_host_batch_sched.py).

    python tests/test_gpu_schedule_pins.py        prints the file's content for the library CNMF_LIB_PATH names
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_pins.json")
FIELDS = ("kc", "gemm_mode", "outer_iterations", "column_iterations", "restart_iterations", "tail_iterations",
          "tail_live_columns")


def jobs():
    """{name: (matrix, max_iter, [(ks, seeds, kc_max), ...])}"""
    rs = np.random.RandomState(5)
    XA = rs.gamma(0.4, 1.0, size=(300, 170)).astype(np.float32)             # the f32 pipe: ragged ranks, then a refilling batch

    def seeds(n):
        return [int(s) for s in rs.randint(1, 2**31 - 1, size=n)]

    A = [([3, 16, 33, 65, 128], seeds(5), 0), ([9] * 40, seeds(40), 128)]
    # 1024 x 768 padded: the smallest matrix with whole tiles of the split-operand kernels; counts -> the count path, wide
    XB = rs.poisson(1.5, size=(1024, 520)).astype(np.float32)
    B = []
    for n, kc in ((150, 0), (70, 256)):
        B.append(([int(k) for k in rs.randint(5, 14, size=n)], seeds(n), kc))
    return {"A": (XA, 12, A), "B": (XB, 10, B)}


def run(engine):
    """{job: {"max_iter": m, "calls": [{"ks", "kc_max", "n_iter_all_max_iter", <FIELDS>}, ...]}}"""
    out = {}
    for name, (X, max_iter, calls) in jobs().items():
        engine.set_matrix(X)
        rows = []
        for ks, seeds, kc_max in calls:
            _, _, n_iter, _ = engine.nmf_batch(ks, seeds=seeds, tol=0.0, max_iter=max_iter, kc_max=kc_max, warn=False)
            row = {"ks": ks, "kc_max": kc_max, "n_iter_all_max_iter": bool((np.asarray(n_iter) == max_iter).all())}
            row.update({f: int(engine.last_stats[f]) for f in FIELDS})
            rows.append(row)
        out[name] = {"max_iter": max_iter, "calls": rows}
    return out


def test_schedule_statistics_equal_the_pins(engine):
    pins = json.load(open(PINS))
    got = run(engine)
    for name in ("A", "B"):
        assert got[name]["max_iter"] == pins[name]["max_iter"]
        for i, (g, p) in enumerate(zip(got[name]["calls"], pins[name]["calls"])):
            assert g["n_iter_all_max_iter"], (name, i)
            assert g["ks"] == p["ks"], (name, i)
            assert {f: g[f] for f in FIELDS} == {f: p[f] for f in FIELDS}, (name, i)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cnmf_amd.engine import Engine
    with Engine(0) as eng:
        doc = {"_source": sys.argv[1] if len(sys.argv) > 1 else ""}
        doc.update(run(eng))
    print(json.dumps(doc, indent=1))
