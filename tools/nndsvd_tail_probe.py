"""Both tails of init='nndsvd' in one run at the north-star shape (C3, K = 5..13, PER_K restarts per rank): the batched
initialisation with tail="host" (LAPACK on the host thread pool, factors uploaded per restart by the batch call) and with
tail="device" (cnmf_nndsvd_group into the init store, the batch starts from it), and the restarts behind each
-> OUT (default profiles/nndsvd_device_tail_c3.json).  GIT_HEAD in the environment names the commit when there is no .git to ask."""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnmf_amd import synth
from cnmf_amd.cnmf import ledger_seeds
from cnmf_amd.engine import Engine

per_k = int(os.environ.get("PER_K", 10))
head = os.environ.get("GIT_HEAD")
if not head:
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        head = ""
X = synth.make_config("C3", dtype=np.float32)
led = ledger_seeds(list(range(5, 14)), per_k, 14)
ks, seeds = [k for k, _, _ in led], [int(s) for _, _, s in led]
try:                                       # the CPUs the control group really grants (what the host tail's pool is sized by)
    quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
    cpu_quota = None if quota == "max" else float(quota) / float(period)
except (OSError, ValueError):
    cpu_quota = None
res = {"config": "C3 50000 x 2000, K=5..13, %d restarts with init='nndsvd'" % len(ks),
       "host_threads": len(os.sched_getaffinity(0)), "cpu_quota": cpu_quota,
       "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "git_head": head or None}
with Engine(0) as eng:
    eng.set_matrix(X)
    eng.nndsvd_init_batch(ks[:2], seeds[:2])                                    # warm-up of both routes
    eng.nndsvd_init_batch(ks[:2], seeds[:2], tail="device")
    eng.nmf_batch(ks[:2], seeds=seeds[:2], max_iter=3, warn=False)
    for rep in range(2):                                                        # the second round is the one reported
        t0 = time.perf_counter(); inits = eng.nndsvd_init_batch(ks, seeds, tail="host"); t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, n_host, _ = eng.nmf_batch(ks, W0=[w for w, _ in inits], H0=[h for _, h in inits], warn=False)
        r_host = time.perf_counter() - t0
        t0 = time.perf_counter(); kept = eng.nndsvd_init_batch(ks, seeds, tail="device", keep=True); t_dev = time.perf_counter() - t0
        route = eng.last_nndsvd_tail
        t0 = time.perf_counter()
        _, _, n_dev, _ = (eng.nmf_batch(ks, init_store=True, warn=False) if kept is None else
                          eng.nmf_batch(ks, W0=[w for w, _ in kept], H0=[h for _, h in kept], warn=False))
        r_dev = time.perf_counter() - t0
    eng.init_store_reset()
for name, t, r, n in (("host", t_host, r_host, n_host), ("device", t_dev, r_dev, n_dev)):
    res["tail_" + name] = {"init_s": t, "init_ms_per_restart": 1e3 * t / len(ks), "restarts_s": r,
                           "mean_iterations": float(np.mean(n)), "restarts_per_s_incl_init": len(ks) / (t + r),
                           "restarts_per_s_excl_init": len(ks) / r}
res["tail_device"]["route"] = route
print(json.dumps(res, indent=1))
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "nndsvd_device_tail_c3.json"))
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
