#!/usr/bin/env python
"""bench.py -- NMF restarts/s of the MI355X-native cNMF hot path (BASELINE.json metric).

Workload (default, ``config.workload``): the north-star headline shape -- 50 000 cells x
2000 high-variance genes (synthetic gamma-Poisson counts, reference `prepare` scaling,
cnmf_amd/synth.py "C3"), K in {5..13}.  One STEP = one pass of the hot path over one
batch of restarts: ``--restarts-per-k`` restarts for every K (default 100 = the north star's
n_iter -> one step is one whole factorize() job of 900 restarts, streamed through up to 1024
packed component columns by the slot work-queue; every step learns its queue order from scratch), run to sklearn's stopping rule (tol 1e-4, max_iter 1000)
with sklearn's init='random' generated on the device from the cNMF ledger seeds
(master seed 14).  X is resident in HBM before the timed region.

Multi-GPU, one process per GPU.  ``python bench.py --gpus N`` with N > 1 SPAWNS its N ranks itself (no launcher, no
torch: RANK / LOCAL_RANK / WORLD_SIZE in the environment, the 128-byte RCCL id through a file); under an external
launcher (``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N``: WORLD_SIZE already set) it runs
as that launcher's rank.  Either way the world size must equal ``--gpus`` or the run fails.
  --scaling strong (default): one step is the SAME fixed job at every N -- the north-star factorize() of
      |K| x restarts-per-k restarts -- sharded over the ranks exactly like the reference's worker_filter (ledger row idx
      -> rank idx % N, cnmf.py:52-53); the step ends when the ONE all-gather of the per-restart spectra (RCCL over
      xGMI, inside the library) has completed on every rank; value = restarts of the job / max-over-ranks time.
  --scaling weak: every rank runs its own |K| x restarts-per-k restarts per step (per-GPU work fixed).
Every rank holds a replica of X; there is no collective inside the restart loop.

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step), with extra objects:
  roofline     -- the dominant kernel (MFMA GEMM passes): algorithmic flops / launch duration measured
                  with HIP events inside the library (every --event-stride-th iteration, default 64) during the timed
                  steps, vs the roofline of the scheme the pass runs (f16 / bf16 dense MFMA peak / MFMAs per f32-class
                  product: 2 on the default count path, 3 or 6 on the others; f32 MFMA peak on the exact-f32 pipe)
A plain run stops there.  ``--full`` (N = 1) adds the measurements that take runs of their own:
  cpu_baseline -- scikit-learn's non_negative_factorization (the call the reference makes,
                  cnmf.py:672) timed on this box's host cores on a bounded sample.
  consensus    -- BASELINE config 5 (consensus-only stress) wall-clock, GPU next to the sklearn/pandas calls; with the
                  spectra uploaded and with the spectra already resident on the device (as after factorize)
  with_queue_hints -- the same job once more with the iteration counts per rank that the timed steps learned handed back
                  explicitly (cnmf_set_iteration_hints): reported beside the headline, never part of it
  general_path -- the same step with count detection OFF (any-X split-operand kernels), bounded
  e2e          -- prepare -> factorize -> combine -> k selection -> consensus(k=9) with the TPM tail, seconds per stage,
                  next to the CPU reference path (prepare like for like, k selection and consensus measured, factorize an
                  extrapolation from the measured restart-iterations/s; no total, no speed-up)
  kl_non_zero_path -- Kullback-Leibler restarts (beta_loss != 'frobenius') on a 50 000 x 2 000 count matrix with a real matrix's
                  sparsity (9 % non-zero): the non-zero kernels beside the dense matrix-pipe kernels, us per restart-iteration
``--dump-outputs DIR`` writes what the last timed step computed as .npy files (dump_outputs); the inputs are seeded, so
two builds run with the same arguments can be compared output for output.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16 / _f16, dense
# MFMAs per f32-accurate product, by cnmf_batch_stats.gemm_mode:
#   1/2: both operands as three bf16 planes, ah*bh + (ah*bm + am*bh) + (ah*bl + am*bm + al*bh)   (kernels_gemm3.hip.h)
#   3  : count-structured X = (integers <= 256) x per-gene scale -> ONE integer plane, (ah + am + al)*n, all exact
#   4  : the same on the f16 pipe (kernels_gemm2h.hip.h): counts <= 2048 in one f16 plane, the factor as TWO f16 planes
#        with a per-row exponent (within 1 ulp_f32 of the f32 value, exact for 3 in 4), partial products exact
#   5  : any other X on the f16 pipe: X and the factor both as two f16 planes with a per-row exponent; round 4: three of
#        the four plane products (x_m . f_m <= 2^-22 of the product is not formed; the 3 x 3 bf16 scheme of modes 1/2 drops
#        the terms below 2^-18); CNMF_G2_GEN4=1 brings the fourth back
SPLIT_MFMAS_PER_PRODUCT = {1: 6, 2: 6, 3: 3, 4: 2, 5: 4 if os.environ.get("CNMF_G2_GEN4") else 3}
HBM_PEAK_GBS = 8000.0
# device sources whose text the committed PMC / ablation profiles describe: a profile taken from other sources is stale
PROFILED_SOURCES = ("cnmf_amd/csrc/kernels_gemm2h.hip.h", "cnmf_amd/csrc/kernels_sweep.hip.h",
                    "cnmf_amd/csrc/kernels_gemm3.hip.h", "cnmf_amd/csrc/gemm_host.hip.h")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong")
    ap.add_argument("--workload", default="C3", help="C1|C2|C3 (cnmf_amd/synth.py)")
    ap.add_argument("--n-cells", type=int, default=None, help="truncate the workload (debug only)")
    ap.add_argument("--restarts-per-k", type=int, default=100)
    ap.add_argument("--kmin", type=int, default=5)
    ap.add_argument("--kmax", type=int, default=13)
    ap.add_argument("--event-stride", type=int, default=64,
                    help="HIP events around the two GEMM passes of every n-th iteration (the roofline's launch durations)")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: after the headline also measure with_queue_hints, cpu_baseline, consensus, general_path, e2e "
                         "and kl_non_zero_path (off by default: a plain run times the steps and prints the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step computed (the spectra of its restarts, "
                         "per K; n_iter; violation) as DIR/<name>.npy, float32 / float64, at most 64 MB in all")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and consensus")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip with_queue_hints, general_path, e2e and "
                                                             "kl_non_zero_path (profiling runs)")
    ap.add_argument("--emulate-rank", default=None, metavar="R/W",
                    help="single GPU: run only the shard rank R of a world of W would run in --scaling strong "
                         "(tools/shard_scaling.py: the projected strong-scaling curve from one GPU)")
    ap.add_argument("--allow-transport-fallback", action="store_true",
                    help="N > 1 only: when the in-library RCCL communicator fails to form, carry the gather over torch.distributed "
                         "instead of exiting non-zero; the line is then reported under a DIFFERENT metric name")
    ap.add_argument("--comm-dry-run", action="store_true",
                    help="N > 1: form the RCCL communicator, run one all-gather across all ranks, print what RCCL saw, exit")
    ap.add_argument("--cpu-iters", type=int, default=30)
    ap.add_argument("--cpu-baseline-full", default=None, metavar="OUT.json",
                    help="OFFLINE, no GPU: k in (5, 9, 13) x the first 3 ledger seeds each, scikit-learn float64 to the "
                         "stopping rule, in both modes of SURVEY 8d; writes OUT.json (profiles/r6_cpu_full_restarts.json) and exits")
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-workers-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--spawn-selftest", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


# ------------------------------------------------------------------------------------------ self-launch (N > 1)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks (this same command line, one per GPU), relay
    rank 0's JSON line, fail if any rank fails.  No torch, no torch.distributed.run.  The launcher itself is the
    product's (cnmf_amd/dist.py::launch_ranks, round 4: the one ``cNMF.factorize_multi_gpu`` uses)."""
    from cnmf_amd import dist as cd
    try:
        out0 = cd.launch_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], n,
                               env=dict(os.environ, CNMF_BENCH_SPAWNED="1"))
    except cd.RankFailure as e:
        sys.stderr.write("bench.py: %s\n-- no result\n" % e)
        sys.exit(1)
    lines = [ln for ln in out0.decode().splitlines() if ln.startswith("{")]
    if len(lines) != 1:
        sys.stderr.write("bench.py: expected ONE JSON line from rank 0, got %d\n" % len(lines))
        sys.exit(1)
    d = json.loads(lines[0])
    if d.get("n_gpus") != n:
        sys.stderr.write("bench.py: the ranks report n_gpus=%r, asked for %d\n" % (d.get("n_gpus"), n))
        sys.exit(1)
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()


# ------------------------------------------------------------------------------------------ CPU baseline
def _cpu_worker(job):
    """One cNMF-style worker: a single-threaded scikit-learn restart capped at ``max_iter`` outer iterations."""
    k, seed, max_iter = job
    from threadpoolctl import threadpool_limits
    from oracle import sklearn_ref
    with threadpool_limits(1):
        t0 = time.perf_counter()
        _, _, n_it = sklearn_ref.nmf(_CPU_X64, k, seed=seed, max_iter=max_iter)
        return int(n_it), time.perf_counter() - t0


_CPU_X64 = None


def granted_cpus():
    """CPUs this process may use: affinity mask, capped by the cgroup v2 quota."""
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            ncpu = max(1, min(ncpu, int(float(q) / float(per))))
    except Exception:
        pass
    return ncpu


def _cpu_full_worker(job):
    k, seed = job
    from threadpoolctl import threadpool_limits
    from oracle import sklearn_ref
    with threadpool_limits(1):
        t0 = time.perf_counter()
        _, _, n_it = sklearn_ref.nmf(_CPU_X64, k, seed=seed)
        return {"k": int(k), "seed": int(seed), "n_iter": int(n_it), "seconds": time.perf_counter() - t0}


def cpu_baseline_full(out_path, workload="C3"):
    """Round-5 review, item 8 -- the end of the "EXTRAPOLATED" caveat: whole restarts, not capped samples.  The bench's own
    matrix, k in (5, 9, 13), the first three rows of each in the north-star ledger (seed 14, K = 5..13, n_iter = 100),
    scikit-learn float64 through the reference's call (cnmf.py:672 via oracle/sklearn_ref.py) to its stopping rule (tol 1e-4,
    max_iter 1000), in both modes of SURVEY 8d: (1) one worker with all BLAS threads, restart after restart; (2) cNMF's own
    parallelism -- one single-thread process per CPU, the nine restarts dealt to them.  Offline (tens of minutes), never part
    of the driver's run; the bench line cites the committed file beside its sampled `value`."""
    global _CPU_X64
    import multiprocessing as mp
    from threadpoolctl import threadpool_info, threadpool_limits
    from cnmf_amd import synth
    from cnmf_amd.cnmf import ledger_seeds
    from oracle import sklearn_ref
    X32 = synth.make_config(workload, dtype=np.float32)
    _CPU_X64 = X32.astype(np.float64)
    led = ledger_seeds(list(range(5, 14)), 100, 14)
    jobs = [(k, int(s)) for kk in (13, 9, 5) for (k, it, s) in led if k == kk and it < 3]        # longest first
    ncpu = granted_cpus()
    blas = ", ".join(sorted({"%s %s" % (p.get("internal_api"), p.get("version")) for p in threadpool_info()}))
    cpu_model = "unknown"
    try:
        cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        pass
    res = {"workload": "%s: %d x %d, scikit-learn non_negative_factorization(solver='cd', float64, init='random', tol=1e-4, "
                       "max_iter=1000) -- whole restarts to the stopping rule" % (workload, X32.shape[0], X32.shape[1]),
           "restarts": [{"k": k, "seed": s} for k, s in jobs], "cpu_model": cpu_model, "cpu_count": os.cpu_count(),
           "cpus_granted": ncpu, "blas": blas}
    # mode 1: one worker, all BLAS threads
    rows, t0 = [], time.perf_counter()
    with threadpool_limits(ncpu):
        for k, s in jobs:
            t1 = time.perf_counter()
            _, _, n_it = sklearn_ref.nmf(_CPU_X64, k, seed=s)
            rows.append({"k": k, "seed": s, "n_iter": int(n_it), "seconds": time.perf_counter() - t1})
            sys.stderr.write("mode 1: k=%d seed=%d n_iter=%d %.1f s\n" % (k, s, n_it, rows[-1]["seconds"]))
    dt1 = time.perf_counter() - t0
    it1 = sum(r["n_iter"] for r in rows)
    res["one_worker_all_threads"] = {"threads": ncpu, "restarts": rows, "seconds": dt1, "iterations": it1,
                                     "restarts_per_s": len(rows) / dt1, "restart_iterations_per_s": it1 / dt1}
    # mode 2: single-thread worker processes (forked: they share the matrix pages)
    workers = max(1, min(ncpu, len(jobs)))
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(workers) as pool:
        rows2 = pool.map(_cpu_full_worker, jobs, chunksize=1)
    dt2 = time.perf_counter() - t0
    it2 = sum(r["n_iter"] for r in rows2)
    res["workers_single_thread"] = {"workers": workers, "restarts": rows2, "seconds": dt2, "iterations": it2,
                                    "restarts_per_s": len(rows2) / dt2, "restart_iterations_per_s": it2 / dt2,
                                    "note": "%d restarts on %d workers: the wall time includes the idle tail of the workers that "
                                            "finish first (as a real cNMF run's does)" % (len(jobs), workers)}
    best = max(("one_worker_all_threads", "workers_single_thread"), key=lambda m: res[m]["restart_iterations_per_s"])
    res["best_mode"] = best
    res["restart_iterations_per_s"] = res[best]["restart_iterations_per_s"]
    res["restarts_per_s"] = res[best]["restarts_per_s"]
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("one_worker_all_threads", "workers_single_thread", "restarts")}))


def cpu_workers_child(npy_path, iters):
    """Mode 2 of SURVEY 8d, in its OWN interpreter started with OPENBLAS/OMP/MKL_NUM_THREADS=1 (set before numpy is
    imported, so that every forked worker is single-threaded by construction): one process per available core, each
    running ONE scikit-learn restart capped at ``iters`` outer iterations -- how cNMF is parallelised in practice
    (Extras/run_parallel.py: total_workers independent processes).  The clock of a worker starts AFTER it holds the
    matrix; scikit-learn's own input checks and init are inside (they are inside the reference's call too)."""
    global _CPU_X64
    import multiprocessing as mp
    _CPU_X64 = np.load(npy_path).astype(np.float64)
    ks = (5, 9, 13)
    ncpu = granted_cpus()
    try:
        avail = [int(l.split()[1]) * 1024 for l in open("/proc/meminfo") if l.startswith("MemAvailable")][0]
    except Exception:
        avail = 64 << 30
    per_worker = int(1.3 * _CPU_X64.nbytes)              # each worker holds its own X^T copy (sklearn _nmf.py:491)
    workers = max(1, min(ncpu, int(0.5 * avail // per_worker)))
    jobs = [(ks[i % len(ks)], 2000 + i, iters) for i in range(workers)]
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(workers) as pool:
        res = pool.map(_cpu_worker, jobs, chunksize=1)
    dt = time.perf_counter() - t0
    it = sum(r[0] for r in res)
    busy = max(r[1] for r in res)                         # the slowest worker's own clock: excludes fork/teardown
    print(json.dumps({"restart_iterations_per_s": it / busy, "workers": workers, "iterations": it, "seconds": busy,
                      "wall_seconds_incl_fork": dt, "iterations_per_worker": iters}))


def cpu_baseline_child(npy_path, max_iter):
    """Runs in a FRESH interpreter (no HIP context).  SURVEY.md section 8d: time (1) one worker with all BLAS threads
    here (capped at the CPUs this job is granted) and (2) cNMF-style single-thread worker processes
    (cpu_workers_child, its own interpreter) on a stratified k sample; report both."""
    from oracle import sklearn_ref
    X64 = np.load(npy_path).astype(np.float64)
    ks = (5, 9, 13)
    ncpu = granted_cpus()
    blas = "unknown"
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        blas = ", ".join(sorted({"%s %s" % (p.get("internal_api"), p.get("version")) for p in threadpool_info()}))
        limiter = threadpool_limits(ncpu)                # BLAS threads = the CPUs actually granted (not the box's 256)
    except Exception:
        limiter = None
    # (1) one worker, BLAS threads = granted CPUs
    t0 = time.perf_counter()
    it1 = 0
    for k in ks:
        _, _, n_it = sklearn_ref.nmf(X64, k, seed=1000 + k, max_iter=max_iter)
        it1 += n_it
    dt1 = time.perf_counter() - t0
    del X64, limiter
    # (2) single-thread workers, bounded: 10 outer iterations each, 180 s at most
    env = dict(os.environ, OPENBLAS_NUM_THREADS="1", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    mode2 = None
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-workers-child", npy_path, "--cpu-iters", "10"],
                           capture_output=True, text=True, timeout=180, env=env)
        if p.returncode == 0:
            mode2 = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        else:
            mode2 = {"error": p.stderr[-400:]}
    except subprocess.TimeoutExpired:
        mode2 = {"error": "timed out after 180 s"}
    cpu_model = "unknown"
    try:
        cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        pass
    print(json.dumps({
        "one_worker_all_threads": {"restart_iterations_per_s": it1 / dt1, "threads": int(ncpu),
                                   "iterations": it1, "seconds": dt1},
        "workers_single_thread": mode2,
        "cpu_count": os.cpu_count(), "cpus_granted": ncpu, "cpu_model": cpu_model, "blas": blas, "ks": list(ks)}))


def full_restarts_profile():
    """The committed OFFLINE measurement of whole scikit-learn restarts to the stopping rule (bench.py --cpu-baseline-full ->
    profiles/r6_cpu_full_restarts.json): cited beside the sampled `value`, never mixed into it (another box, its core
    count is in the entry)."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "r6_cpu_full_restarts.json")))
    except Exception:
        return None
    m = d[d["best_mode"]]
    return {"source": "profiles/r6_cpu_full_restarts.json (build container, offline)", "cpu_model": d.get("cpu_model"),
            "cores": d.get("cpus_granted"), "mode": d["best_mode"], "restarts": len(m["restarts"]),
            "restarts_per_s": d["restarts_per_s"], "restart_iterations_per_s": d["restart_iterations_per_s"],
            "seconds": m["seconds"], "iterations": m["iterations"],
            "note": "k in (5, 9, 13) x 3 ledger seeds, float64, every restart run to scikit-learn's stopping rule: measured "
                    "restarts per second, no extrapolation"}


def cpu_baseline(X32, mean_iters_per_restart, max_iter):
    """scikit-learn CD-NMF (float64, the reference dtype, cnmf.py:534) on the host cores -- the call the
    reference makes (cnmf.py:672), in the better of SURVEY 8d's two modes.  The primary number is restart-
    ITERATIONS per second (measured, no extrapolation); restarts/s divides it by the GPU run's mean
    iteration count per restart."""
    import tempfile
    import shutil
    tmpdir = tempfile.gettempdir()
    try:
        if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * X32.nbytes:
            tmpdir = "/dev/shm"
    except OSError:
        pass
    path = os.path.join(tmpdir, "cnmf_bench_X_%d.npy" % os.getpid())
    np.save(path, X32)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", path,
                            "--cpu-iters", str(max_iter)], capture_output=True, text=True, timeout=900)
    finally:
        os.remove(path)
    if p.returncode != 0:
        raise RuntimeError("cpu baseline child failed: %s" % p.stderr[-2000:])
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    a, b = d["one_worker_all_threads"], d["workers_single_thread"]
    ok2 = isinstance(b, dict) and "restart_iterations_per_s" in b
    best_is_workers = ok2 and b["restart_iterations_per_s"] >= a["restart_iterations_per_s"]
    best = b if best_is_workers else a
    it_per_s = best["restart_iterations_per_s"]
    return {
        "value": it_per_s,
        "unit": "restart-iterations/s",
        "cores": int(b["workers"] if best_is_workers else a["threads"]),
        "kind": "reference",
        "mode": ("%d single-thread worker processes (cNMF's own parallelism, total_workers = workers)" % b["workers"]
                 if best_is_workers else "1 worker x %d BLAS threads" % a["threads"]),
        "restarts_per_s_extrapolated": it_per_s / max(mean_iters_per_restart, 1.0),
        "modes": d,
        "full_restarts_offline": full_restarts_profile(),
        "sample": ("sklearn.decomposition.non_negative_factorization (solver=cd, float64, init=random) on the same X, "
                   "k in (5, 9, 13): mode 1 = one worker with BLAS threads = the %d CPUs granted to this job, %d outer "
                   "iterations per k (%d iterations in %.1f s); mode 2 = one single-thread process per granted CPU, one "
                   "restart each capped at 10 outer iterations (%s); the better mode is `value`; "
                   "restarts_per_s_extrapolated = value / mean iterations per restart of the GPU run (%.1f)"
                   % (d.get("cpus_granted", a["threads"]), max_iter, a["iterations"], a["seconds"],
                      ("%d workers, %d iterations, slowest worker %.1f s" % (b["workers"], b["iterations"], b["seconds"]))
                      if ok2 else "failed: %s" % (b or {}).get("error", "?"), mean_iters_per_restart)),
    }


# ------------------------------------------------------------------------------------------ committed profiles
def source_hashes():
    out = {}
    for rel in PROFILED_SOURCES:
        try:
            out[rel] = hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()[:16]
        except OSError:
            out[rel] = None
    return out


def load_profile(name):
    """A committed counter / ablation profile (profiles/<name>) together with a staleness verdict: the file records
    the sha256 of the kernel sources it was measured on (tools/stamp_profile.py); if they differ from the tree's, the
    numbers describe ANOTHER kernel and are not used."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", name)))
    except Exception:
        return None, "absent"
    rec = d.get("kernel_source_sha256")
    if not isinstance(rec, dict):
        return d, "unstamped (taken before round 3: kernel sources not recorded)"
    now = source_hashes()
    changed = sorted(k for k in rec if now.get(k) != rec[k])
    if changed:
        return d, "stale: %s changed since the profile was taken (git %s)" % (", ".join(changed), d.get("git_head", "?"))
    return d, None


def pmc_traffic(key, gemm_mode):
    """HBM bytes per launch of the dominant kernel from the PMC counters (FETCH_SIZE, WRITE_SIZE),
    collected in separate rocprofv3 --pmc passes (tools/gpu_pmc_bench.sh) and committed under
    profiles/ -- counters cannot be read from inside an un-profiled run.  (detail, usable)."""
    name = {0: "r1_pmc_traffic.json", 1: "r1_pmc_traffic_split.json", 2: "r1_pmc_traffic_split.json",
            3: "r1_pmc_traffic_counts.json", 4: "r6_pmc_traffic_f16.json", 5: "r6_pmc_traffic_general.json"}[gemm_mode]
    d, verdict = load_profile(name)
    if d is None or key not in d:
        return None, False
    try:
        det = {"hbm_bytes_per_launch": d[key]["hbm_bytes_per_launch"],
               "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"][key],
               "source": "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes; FETCH doubled per the "
                         "gfx950 note of MI355X_MICROARCH.md)" % name,
               "git_head": d.get("git_head"), "stale": verdict}
    except Exception:
        return None, False
    return det, verdict is None


# ------------------------------------------------------------------------------------------ extras (N = 1)
def consensus_wallclock(eng, with_cpu=True):
    """BASELINE config 5 (consensus-only stress: 5000 stacked spectra x 2000 genes, k=20):
    wall-clock of the consensus core on the GPU (host call incl. transfers) next to the
    reference's sklearn/pandas calls on the host cores.  Reported beside the headline metric."""
    from cnmf_amd import synth
    S, _ = synth.consensus_stress(R=5000, G=2000, k=20, n_outliers=100, seed=0)
    eng.consensus(S, 20, density_threshold=0.5)                     # warm-up (allocations, code objects)
    t0 = time.perf_counter()
    out = eng.consensus(S, 20, density_threshold=0.5)
    gpu_s = time.perf_counter() - t0
    res = {"workload": "C5: 5000 spectra x 2000 genes, k=20, density_threshold 0.5, n_neighbors 75",
           "gpu_ms": 1e3 * gpu_s, "rows_kept": int(out["n_kept"]), "dtype": "f64"}
    # the same call with the merged spectra already ON the device (round 4: after factorize they sit in the engine's
    # resident store -- float32, as the restarts produced them -- and are gathered / widened there: no 80 MB upload)
    S32 = S.astype(np.float32)
    gen_rows = eng.spectra_rows
    first = eng.spectra_append(S32)
    rows = first + np.arange(S32.shape[0])
    eng.consensus(None, 20, density_threshold=0.5, store_rows=rows)
    t0 = time.perf_counter()
    out_r = eng.consensus(None, 20, density_threshold=0.5, store_rows=rows)
    res["gpu_ms_spectra_resident"] = 1e3 * (time.perf_counter() - t0)
    ref32 = eng.consensus(S32.astype(np.float64), 20, density_threshold=0.5)
    res["resident_equals_upload_path"] = bool(np.array_equal(out_r["labels"], ref32["labels"])
                                              and np.array_equal(out_r["median_spectra"], ref32["median_spectra"]))
    if gen_rows == 0:
        eng.spectra_reset()
    if with_cpu:
        import pandas as pd
        from sklearn.cluster import KMeans
        from sklearn.metrics.pairwise import euclidean_distances
        t0 = time.perf_counter()
        l2 = (S.T / np.sqrt((S ** 2).sum(axis=1))).T
        D = euclidean_distances(l2)
        n = int(0.30 * S.shape[0] / 20)
        po = np.argpartition(D, n + 1)[:, :n + 1]
        dens = D[np.arange(D.shape[0])[:, None], po].sum(1) / n
        l2k = l2[dens < 0.5]
        km = KMeans(n_clusters=20, n_init=10, random_state=1).fit(l2k)
        pd.DataFrame(l2k).groupby(pd.Series(km.labels_ + 1)).median()
        res["cpu_reference_ms"] = 1e3 * (time.perf_counter() - t0)
        res["cpu_cores"] = granted_cpus()
        res["labels_match_cpu"] = bool(np.array_equal(out["labels"][out["density_filter"]], km.labels_))
    return res


def general_path_step(X, ks_all, by_k, restarts_per_k, event_stride):
    """The same step on a matrix that is NOT count-structured as far as the engine is concerned (count detection off:
    what a Harmony-corrected or TPM-normalised input gets, reference preprocess.py:270-358): X itself as two f16
    planes with a per-row exponent, 3 MFMAs per f32-class product (gemm_mode 5).  Bounded (restarts_per_k restarts per K)."""
    from cnmf_amd.engine import Engine
    N, G = X.shape
    eng = Engine(0, detect_counts=False)
    try:
        eng.set_matrix(X)
        ks, seeds = [], []
        for k in ks_all:
            ks += [k] * restarts_per_k
            seeds += by_k[k][:restarts_per_k]
        eng.nmf_batch(ks[::9], seeds=seeds[::9], warn=False)                       # warm-up: planes of X, code objects
        t0 = time.perf_counter()
        _, _, n_iter, _ = eng.nmf_batch(ks, seeds=seeds, warn=False, profile=event_stride)
        dt = time.perf_counter() - t0
        st = dict(eng.last_stats)
    finally:
        eng.close()
    launches = max(int(st["outer_iterations"]), 1)
    avgA = st["passA_ms"] / max(int(st["passA_launches"]), 1)
    avgB = st["passB_ms"] / max(int(st["passB_launches"]), 1)
    alg = 2.0 * N * G * int(st["restart_column_iterations"])
    per = SPLIT_MFMAS_PER_PRODUCT.get(int(st["gemm_mode"]), 1)
    peak = BF16_MFMA_PEAK_TFLOPS / per if int(st["gemm_mode"]) > 0 else FP32_MFMA_PEAK_TFLOPS
    tfA = alg / max(avgA * launches, 1e-9) / 1e9
    tfB = alg / max(avgB * launches, 1e-9) / 1e9
    dom = "A" if avgA >= avgB else "B"
    return {"workload": "the same matrix with count detection off (Engine(detect_counts=False)): %d restarts, K=%d..%d"
                        % (len(ks), ks_all[0], ks_all[-1]),
            "restarts_per_s": len(ks) / dt, "restart_iterations_per_s": float(np.sum(n_iter)) / dt,
            "mean_iterations_per_restart": float(np.mean(n_iter)), "gemm_mode": int(st["gemm_mode"]),
            "kernel": (("gemm3g_streamk_kernel (pass A, 3 x 3 bf16 planes)" if dom == "A" else "gemm3g_kernel (pass B, 3 x 3 bf16 planes)")
                       if int(st["gemm_mode"]) in (1, 2) else
                       ("gemm2h_streamk_kernel<1, HI> (pass A, 2 x 2 f16 planes)" if dom == "A" else "gemm2h_kernel<1, HI> (pass B, 2 x 2 f16 planes)")
                       if int(st["gemm_mode"]) == 5 else "gemm_mode %d" % int(st["gemm_mode"])),
            "avg_launch_ms": {"passA": avgA, "passB": avgB},
            "achieved_TFLOPs": tfA if dom == "A" else tfB, "peak_TFLOPs": peak, "frac": (tfA if dom == "A" else tfB) / peak,
            "flop_basis": "f32-equivalent flops; peak = bf16 / f16 dense MFMA peak / %d MFMAs per product" % per,
            "column_utilisation": int(st["restart_column_iterations"]) / max(int(st["column_iterations"]), 1),
            "gemm_share_of_gpu_time": (avgA + avgB) * launches / max(st["gpu_ms"], 1e-9)}


def kl_non_zero_path(ks_all, n_cells=50000, iters=100):
    """Kullback-Leibler restarts (the reference's solver for beta_loss != 'frobenius', cnmf.py:618-631) on a count matrix
    with a real matrix's sparsity (library size e^5.2 over 2 000 genes: ~9 % non-zero): the device touches only the
    non-zeros (kernels_mu_sparse.hip.h, scikit-learn's scipy.sparse path) -- timed beside the dense matrix-pipe kernels
    (CNMF_MU_SPARSE=0) on the same matrix.  Bounded: 4 restarts per K, `iters` iterations each, tol = 0."""
    from cnmf_amd import synth
    from cnmf_amd.engine import Engine
    Cs, _ = synth.topic_counts(n_cells, 2000, 20, 5.2, 0.4, 3)
    Xs = synth.normalise_like_prepare(Cs, dtype=np.float32)
    del Cs
    ks = [k for k in ks_all if k <= 32] * 4
    seeds = list(range(11, 11 + len(ks)))
    out = {"workload": "%d x %d, %.1f %% non-zero; %d KL restarts, K=%d..%d, %d iterations each"
                       % (Xs.shape[0], Xs.shape[1], 100.0 * float((Xs != 0).mean()), len(ks), min(ks), max(ks), iters)}
    eng = Engine(0)
    old = os.environ.get("CNMF_MU_SPARSE")
    results = {}
    try:
        import scipy.sparse as sp
        eng.set_matrix(sp.csr_matrix(Xs))          # as the reference hands it over when the normalised counts are stored sparse
        for label, mode in (("non_zero_path", "1"), ("dense_matrix_pipe", "0")):
            os.environ["CNMF_MU_SPARSE"] = mode
            eng.nmf_mu_batch(ks[:2], seeds=seeds[:2], max_iter=3, tol=0, warn=False)        # warm-up: images / X^T, code objects
            t0 = time.perf_counter()
            H_list, _, n_iter, err = eng.nmf_mu_batch(ks, seeds=seeds, max_iter=iters, tol=0, warn=False)
            dt = time.perf_counter() - t0
            out[label] = {"us_per_restart_iteration": 1e6 * dt / float(np.sum(n_iter)), "restart_iterations_per_s": float(np.sum(n_iter)) / dt}
            results[label] = (H_list, np.asarray(err))
            # (round 5: the non-zero leg runs on the compressed rows of the upload -- no dense image, no dense transposed copy)
            out[label]["resident_images"] = [k for k, v in eng.matrix_images().items() if v]
        # no speed-up without a correctness check beside it (round-4 review): the two paths must agree restart by restart
        # (same mathematics, another summation order: float32 round-off over `iters` iterations), and the first restart
        # is held to the float64 oracle's spectra over 20 iterations (bounded: ~10 s on the host)
        from oracle import nmf_cd, nmf_mu
        worst = (0.0, 0.0)
        for hs, hd in zip(results["non_zero_path"][0], results["dense_matrix_pipe"][0]):
            ma, rf = nmf_cd.spectra_error(hd.astype(np.float64), hs)
            worst = (max(worst[0], ma), max(worst[1], rf))
        derr = float(np.max(np.abs(results["non_zero_path"][1] - results["dense_matrix_pipe"][1]) / results["dense_matrix_pipe"][1]))
        os.environ["CNMF_MU_SPARSE"] = "1"
        H20, _, _, _ = eng.nmf_mu_batch(ks[:1], seeds=seeds[:1], max_iter=20, tol=0, warn=False)
        _, H_ref, _ = nmf_mu.nmf_mu(Xs.astype(np.float64), ks[0], seed=seeds[0], max_iter=20, tol=0.0)
        oma, orf = nmf_cd.spectra_error(H_ref, H20[0])
        out["agreement"] = {"non_zero_vs_dense_spectra_maxabs": worst[0], "non_zero_vs_dense_spectra_relfro": worst[1],
                            "non_zero_vs_dense_divergence_rel": derr,
                            "non_zero_vs_float64_oracle_20_iterations": {"maxabs": oma, "relfro": orf},
                            "bars": "spectra 1e-4 / 1e-3 (rows L2-normalised, matched by cosine), divergence 1e-3"}
        out["agreement"]["ok"] = bool(worst[0] <= 1e-4 and worst[1] <= 1e-3 and derr <= 1e-3 and oma <= 1e-4 and orf <= 1e-3)
    finally:
        if old is None:
            os.environ.pop("CNMF_MU_SPARSE", None)
        else:
            os.environ["CNMF_MU_SPARSE"] = old
        eng.close()
    # (a speed-up is only reported beside a passed agreement check)
    out["speed_up"] = (out["dense_matrix_pipe"]["us_per_restart_iteration"] / out["non_zero_path"]["us_per_restart_iteration"]
                       if out.get("agreement", {}).get("ok") else None)
    return out


def e2e_wallclock(eng, C, X, ks_all, restarts_per_k, cpu_it_per_s):
    """prepare -> factorize -> combine -> k selection -> consensus(k = K_true) WITH the TPM tail through the host mirror
    of the reference's cNMF object (what tools/e2e_c3.py does), seconds per stage; beside it the CPU reference path
    stage by stage: prepare like for like (numpy normalisation + the same statistics and file writes), factorize EXTRAPOLATED (sum of the GPU run's iteration counts / the
    measured CPU restart-iterations/s -- running it takes hours), k selection and consensus by oracle/ (numpy / pandas
    / scikit-learn restatement of cnmf.py:871-985), k selection on 3 of the 9 ranks and scaled."""
    import contextlib
    import io
    import shutil
    import tempfile
    import pandas as pd
    import scipy.sparse as sp
    from cnmf_amd.cnmf import cNMF
    keep = C.sum(axis=0) > 0
    Ck = C[:, keep]
    genes = ["g%d" % j for j in range(X.shape[1])]
    cells = ["c%d" % i for i in range(X.shape[0])]
    tpm_csr = sp.csr_matrix((Ck / Ck.sum(axis=1, keepdims=True) * 1e6).astype(np.float32))
    out = tempfile.mkdtemp(prefix="cnmf_bench_e2e_")
    t, buf = {}, io.StringIO()
    try:
        obj = cNMF(output_dir=out, name="c3", engine=eng, compress_merged=False)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            obj.prepare_from_counts(pd.DataFrame(Ck, index=cells, columns=genes), components=list(ks_all),
                                    n_iter=restarts_per_k, seed=14, beta_loss="frobenius", tpm=(tpm_csr, genes))
        t["prepare_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            obj.factorize(write_iter_files=False)
        t["factorize_s"] = time.perf_counter() - t0
        n_iter = np.asarray(obj.last_factorize_stats["n_iter"])
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            obj.combine()
        t["combine_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        obj.k_selection_stats()
        t["k_selection_s"] = time.perf_counter() - t0
        k_cons = 9 if 9 in ks_all else ks_all[len(ks_all) // 2]
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            med, usages = obj.consensus(k_cons, density_threshold=0.5)
        t["consensus_s"] = time.perf_counter() - t0
        merged = {k: obj.merged_cache[k][1].values for k in ks_all}
        gpu_med = med.values
    finally:
        shutil.rmtree(out, ignore_errors=True)
    res = {"workload": "prepare_from_counts (device normalisation) -> factorize (%d restarts) -> combine -> k selection "
                       "(%d ranks, batched) -> consensus(k=%d, density 0.5) incl. TPM spectra / OLS z-scores / final "
                       "usage refit from one CSR upload" % (len(ks_all) * restarts_per_k, len(ks_all), k_cons),
           "stages_s": t, "total_s": sum(t.values()), "restarts": int(len(n_iter)),
           "restart_iterations": int(n_iter.sum()),
           "factorize_host_s": {k: round(float(v), 4) for k, v in (obj.last_factorize_stats.get("host_seconds") or {}).items()}}
    # ---- the CPU reference path beside it
    from oracle import consensus as oc
    c = {}
    # prepare, like for like (round-3 review, weak #11): the SAME artefacts as the device stage above -- normalised
    # matrix (cnmf.py:540-554: unit variance per gene, zero-cell check), TPM statistics, ledger, yaml, and the same file
    # writes through the same host code (prepare_from_matrix) -- with the normalisation in numpy instead of on the device
    out_cpu = tempfile.mkdtemp(prefix="cnmf_bench_e2e_cpu_")
    try:
        t0 = time.perf_counter()
        X64 = Ck.astype(np.float64)
        X64 /= X64.std(axis=0, ddof=1)                                   # cnmf.py:540-548
        if (X64.sum(axis=1) == 0).any():
            raise RuntimeError("zero cells")
        with contextlib.redirect_stdout(buf):
            cNMF(output_dir=out_cpu, name="c3cpu", engine=None, compress_merged=False).prepare_from_matrix(
                pd.DataFrame(X64, index=cells, columns=genes), components=list(ks_all), n_iter=restarts_per_k, seed=14,
                beta_loss="frobenius", tpm=(tpm_csr, genes))
        c["prepare_s"] = time.perf_counter() - t0
    finally:
        shutil.rmtree(out_cpu, ignore_errors=True)
    c["factorize_s_extrapolated"] = float(n_iter.sum()) / cpu_it_per_s if cpu_it_per_s else None
    sample = [k for k in (ks_all[0], k_cons, ks_all[-1])]
    t0 = time.perf_counter()
    for k in sample:
        oc.consensus_core(merged[k].astype(np.float64), X64, k, stats_mode=True)     # incl. silhouette + prediction error
    c["k_selection_s"] = (time.perf_counter() - t0) * len(ks_all) / len(sample)
    t0 = time.perf_counter()
    core = oc.consensus_core(merged[k_cons].astype(np.float64), X64, k_cons, density_threshold=0.5)
    tpm64 = np.asarray(tpm_csr.todense(), dtype=np.float64)
    tail = oc.consensus_tail(core, tpm64, tpm64.std(axis=0), np.arange(X64.shape[1]))
    del tpm64
    c["consensus_s"] = time.perf_counter() - t0
    c["combine_s"] = t["combine_s"]                                      # file gather: the same host work either way
    res["cpu_reference"] = {"stages_s": c, "cores": granted_cpus(),
                            "kind": "prepare: numpy normalisation + the same host code and file writes as the device stage; "
                                    "factorize: scikit-learn, EXTRAPOLATED, not run (hours); k selection (sampled on K = %s "
                                    "and scaled) and consensus + tail: oracle/consensus.py (numpy / pandas / scikit-learn "
                                    "restatement of cnmf.py:871-985)" % sample,
                            "factorize_basis": "sum of the device run's iteration counts (%d) / measured CPU "
                                               "restart-iterations/s (%.1f)" % (int(n_iter.sum()), cpu_it_per_s or 0.0),
                            "note": "no total and no speed-up are reported: the factorize stage is an extrapolation from a "
                                    "bounded sample, the other stages are measured (compare them stage by stage)"}
    d = tail["median_spectra"] - gpu_med
    res["consensus_spectra_sumsq_vs_cpu"] = float((d ** 2).sum())       # the reference's bar: < 1e-4
    return res


def form_transport(bootstrap, rank, world, id_path, allow_fallback, explicit=False, timeout=None):
    """Form the in-library RCCL communicator (`bootstrap()`), then let ALL ranks agree on what happened before anyone moves
    on (cnmf_amd/dist.py::agree_on_outcome).  The in-library communicator has never met more than one GPU (DESIGN.md section
    6), so its first N > 1 run must not be able to turn "RCCL did not work" into a green number (round-5 review, item 6):

    * every rank succeeded                      -> ("rccl", None);
    * some rank failed, default                 -> EVERY rank exits non-zero, no JSON line;
    * some rank failed, --allow-transport-fallback -> ("torch", reason) on every rank: torch.distributed (backend nccl = the
      same RCCL) carries the gather, and the line's "metric" says so (FALLBACK_METRIC) -- it cannot be mistaken for the
      headline."""
    from cnmf_amd import dist as cd
    err = None
    if world > 1:
        try:
            os.remove("%s.status.%d" % (id_path, rank))      # (a stale report of an earlier launch under the same name)
        except OSError:
            pass
    try:
        bootstrap()
    except Exception as e:                           # noqa: BLE001 -- whatever the library / the rendezvous raised
        if world == 1 or explicit:
            raise
        err = repr(e)
    if world == 1:
        return "rccl", None
    reports = cd.agree_on_outcome(id_path, rank, world, err is None, err or "",
                                  timeout=timeout or float(os.environ.get("CNMF_BENCH_AGREE_TIMEOUT", "120")))
    failed = [(r, m) for r, ok, m in reports if not ok]
    if not failed:
        return "rccl", None
    reason = "; ".join("rank %d: %s" % rm for rm in failed)
    if not allow_fallback:
        raise SystemExit("bench.py: the in-library RCCL communicator did not form on %d of %d ranks (%s).  No number is "
                         "reported.  (--allow-transport-fallback re-runs the gather over torch.distributed and reports it "
                         "under a different metric name; CNMF_GATHER=torch selects that transport explicitly.)"
                         % (len(failed), world, reason))
    sys.stderr.write("bench.py: rank %d: in-library RCCL init failed (%s): --allow-transport-fallback given, all ranks "
                     "switch to torch.distributed\n" % (rank, reason))
    return "torch", reason


FALLBACK_METRIC = "NMF restarts/sec over torch.distributed (TRANSPORT FALLBACK: the in-library RCCL gather FAILED to initialise)"


# ------------------------------------------------------------------------------------------ main
DUMP_SPECTRA_BYTES = 60_000_000        # --dump-outputs: the spectra files stay under this; the rest is a few kB


def dump_outputs(out_dir, spectra, restarts, n_iter, violation):
    """--dump-outputs: what the last timed step handed its caller.  ``spectra`` maps (k, restart index in the step's job)
    to the k x G float32 spectra; ``restarts`` / ``n_iter`` / ``violation`` cover the same restarts, in order.
    Writes, all float32 / float64:
      spectra_kNN.npy          [m, k, G] float32 -- the spectra of every restart with k components; when all
                                of them would pass DUMP_SPECTRA_BYTES, a fixed sample (numpy default_rng(k)) of each k
      spectra_kNN_restart.npy  [m] float64        -- which restarts of the step's job those are
      restart.npy, n_iter.npy, violation.npy  [n] float64 -- every restart of the step (all ranks), its outer
                                iterations and its final violation"""
    os.makedirs(out_dir, exist_ok=True)
    by_k = {}
    for (k, j) in sorted(spectra):
        by_k.setdefault(int(k), []).append(j)
    G = next(iter(spectra.values())).shape[1] if spectra else 0
    total = sum(k * G * 4 * len(js) for k, js in by_k.items())
    for k, js in sorted(by_k.items()):
        if total > DUMP_SPECTRA_BYTES:
            m = max(1, len(js) * DUMP_SPECTRA_BYTES // total)
            js = [js[i] for i in np.sort(np.random.default_rng(k).choice(len(js), m, replace=False))]
        np.save(os.path.join(out_dir, "spectra_k%02d.npy" % k),
                np.stack([np.asarray(spectra[(k, j)], dtype=np.float32) for j in js]))
        np.save(os.path.join(out_dir, "spectra_k%02d_restart.npy" % k), np.asarray(js, dtype=np.float64))
    np.save(os.path.join(out_dir, "restart.npy"), np.asarray(restarts, dtype=np.float64))
    np.save(os.path.join(out_dir, "n_iter.npy"), np.asarray(n_iter, dtype=np.float64))
    np.save(os.path.join(out_dir, "violation.npy"), np.asarray(violation, dtype=np.float64))


def main():
    args = parse()
    if args.cpu_baseline_child:
        cpu_baseline_child(args.cpu_baseline_child, args.cpu_iters)
        return
    if args.cpu_workers_child:
        cpu_workers_child(args.cpu_workers_child, args.cpu_iters)
        return
    if args.cpu_baseline_full:
        cpu_baseline_full(args.cpu_baseline_full, args.workload)
        return
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus)                       # the parent: N ranks of this very command line, no launcher
        return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started a world of %d ranks (WORLD_SIZE): refusing to "
                         "report a number under the wrong n_gpus" % (args.gpus, world))
    if args.spawn_selftest:                           # (tests/test_bench_spawn.py: the launch plumbing without a GPU)
        if os.environ.get("CNMF_BENCH_SELFTEST_FAIL_RANK") == str(rank):
            raise SystemExit(3)
        fb = None
        if os.environ.get("CNMF_BENCH_SELFTEST_RCCL_FAIL_RANKS") is not None:
            # (the transport decision of the N > 1 path without a GPU: the communicator set-up "fails" on the listed ranks)
            bad = [int(r) for r in os.environ["CNMF_BENCH_SELFTEST_RCCL_FAIL_RANKS"].split(",") if r != ""]

            def fake_bootstrap():
                if rank in bad:
                    raise RuntimeError("ncclCommInitRank: simulated failure on rank %d" % rank)
            idp = os.environ.get("CNMF_RCCL_ID_FILE") or os.path.join(
                "/tmp", "cnmf_rccl_id.%d.%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0")))     # (as the real path below)
            mode, fb = form_transport(fake_bootstrap, rank, world, idp, args.allow_transport_fallback, timeout=20.0)
            if rank == 0:
                print(json.dumps({"n_gpus": world, "gather": mode, "gather_fallback": fb,
                                  "metric": (FALLBACK_METRIC if fb else "NMF restarts/sec") + " (selftest)"}))
            return
        if rank == 0:
            print(json.dumps({"n_gpus": world, "rank": rank, "local_rank": local_rank,
                              "id_file": os.environ.get("CNMF_RCCL_ID_FILE"), "spawned": os.environ.get("CNMF_BENCH_SPAWNED"),
                              "master": "%s:%s" % (os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))}))
        return
    # stdout must carry exactly ONE JSON line, but RCCL prints a version banner to the C-level
    # stdout (flushed at exit): keep the real stdout aside and point fd 1 at stderr meanwhile
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    multi = world > 1 or bool(os.environ.get("CNMF_BENCH_FORCE_DIST"))     # (the override exercises the N > 1 code at world 1)
    if os.environ.get("CNMF_BENCH_ONE_GPU"):                               # test hook: every rank on GPU 0
        local_rank = 0
    emu = None
    if args.emulate_rank:
        if multi:
            raise SystemExit("--emulate-rank is a single-GPU projection")
        emu = tuple(int(v) for v in args.emulate_rank.split("/"))
        assert 0 <= emu[0] < emu[1]
    # Transport of everything that crosses ranks (the one data-path gather, the barrier, the max/sum over ranks):
    #   "rccl"  (default) -- ncclAllGather inside the C-ABI library (cnmf_comm_* / cnmf_allgather_*); NO torch:
    #                        the launcher only provides RANK / WORLD_SIZE, the 128-byte RCCL id travels through a file;
    #   "torch" -- torch.distributed (backend nccl = RCCL, or gloo for the one-GPU test hook).
    gather_mode = "none"
    if multi:
        gather_mode = os.environ.get("CNMF_GATHER", "torch" if os.environ.get("CNMF_BENCH_BACKEND") else "rccl")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # before the HIP runtime starts (dmabuf IPC only)
    dist = None
    if gather_mode == "torch":
        import torch
        import torch.distributed as dist
        # (test hook: CNMF_BENCH_BACKEND=gloo CNMF_BENCH_ONE_GPU=1 runs several ranks on ONE GPU to exercise the
        #  N > 1 bookkeeping -- ledger sharding, ragged gather, max-over-ranks -- where only one GPU exists)
        backend = os.environ.get("CNMF_BENCH_BACKEND", "nccl")
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend)
    tdev = "cpu" if os.environ.get("CNMF_BENCH_BACKEND", "nccl") == "gloo" else "cuda"

    from cnmf_amd import synth
    from cnmf_amd.cnmf import ledger_seeds, worker_filter
    from cnmf_amd.engine import Engine

    Ncfg, Gcfg, Kt, mu, sg, dseed = synth.CONFIGS[args.workload]
    C, _ = synth.topic_counts(args.n_cells or Ncfg, Gcfg, Kt, mu, sg, dseed)      # raw counts (the e2e leg needs them too)
    X = synth.normalise_like_prepare(C, dtype=np.float32)
    N, G = X.shape
    eng = Engine(local_rank)
    eng.set_matrix(X)
    rccl_info = None
    gather_fallback = None
    if gather_mode == "rccl":
        from cnmf_amd import dist as cd
        # all ranks of one node are children of the same launcher process: its pid + the rendezvous port
        # name the id file uniquely for this launch
        id_path = os.environ.get("CNMF_RCCL_ID_FILE") or os.path.join(
            "/tmp", "cnmf_rccl_id.%d.%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0")))
        gather_mode, gather_fallback = form_transport(
            lambda: cd.comm_bootstrap_file(eng, rank, world, id_path), rank, world, id_path, args.allow_transport_fallback,
            explicit=bool(os.environ.get("CNMF_GATHER") or os.environ.get("CNMF_BENCH_ONE_GPU")))
        if gather_mode == "torch":
            eng.comm_finalize()                      # a communicator that formed on this rank is not used by anybody
            import torch
            import torch.distributed as dist
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl")
    if gather_mode == "rccl":
        # proof in the line itself that RCCL formed a communicator of `world` ranks and that a collective crossed ALL of them
        # (round-4 review, item 8): every rank contributes its rank and device to one ncclAllGather
        seen = eng.allgather_array(np.array([rank, local_rank], dtype=np.int64))
        rccl_info = {"communicator_ranks": int(eng.comm_world), "ranks_seen_by_allgather": sorted(int(r) for r in seen[:, 0]),
                     "devices": [int(d) for d in seen[:, 1]], "transport": "ncclAllGather in libcnmf_hip.so (RCCL via dlopen)"}
        if args.comm_dry_run:
            if rank == 0:
                os.write(json_fd, (json.dumps({"dry_run": "communicator only: no factorisation was run", "n_gpus": world,
                                               "rccl": rccl_info}) + "\n").encode())
            os.close(json_fd)
            eng.close()
            return

    ks_all = list(range(args.kmin, args.kmax + 1))
    n_steps_total = args.warmup + args.steps
    strong = args.scaling == "strong"
    jobs_per_step = 1 if strong else world                   # whole jobs (|K| x restarts_per_k restarts) per step
    led = ledger_seeds(ks_all, args.restarts_per_k * n_steps_total * jobs_per_step, 14)      # the product's own ledger
    by_k = {k: [int(s) for (kk, _, s) in led if kk == k] for k in ks_all}
    shard_rank, shard_world = emu if emu else (rank, world)

    def step_jobs(step):
        """strong: the step's job = restarts_per_k ledger rows of every K, in ledger order (k-major); this rank runs the
        rows idx with (idx - rank) % world == 0 (cnmf.py:52-53).  weak: every rank its own job."""
        ks, seeds = [], []
        if strong:
            for k in ks_all:
                base = step * args.restarts_per_k
                ks += [k] * args.restarts_per_k
                seeds += by_k[k][base:base + args.restarts_per_k]
            mine = list(worker_filter(range(len(ks)), shard_rank, shard_world))
            return [ks[i] for i in mine], [seeds[i] for i in mine], len(ks) if not emu else len(mine)
        for k in ks_all:
            base = (step * world + rank) * args.restarts_per_k
            ks += [k] * args.restarts_per_k
            seeds += by_k[k][base:base + args.restarts_per_k]
        return ks, seeds, len(ks) * world

    def barrier():
        # every engine call returns with its stream drained, so a barrier over ranks is also a device barrier
        if gather_mode == "rccl":
            eng.allgather_array(np.zeros(1, dtype=np.int64))     # one tiny ncclAllGather + stream sync
        elif dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    def over_ranks(vec):
        """[world, len(vec)] float64: every rank's row."""
        v = np.asarray(vec, dtype=np.float64)
        if gather_mode == "rccl":
            return eng.allgather_array(v)
        if dist is not None:
            import torch
            t = torch.tensor(v, dtype=torch.float64, device=tdev)
            out = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(out, t)
            return np.stack([o.cpu().numpy() for o in out])
        return v[None, :]

    def gather(H_list, ks, step):
        """The one data-path collective: all-gather of the packed per-restart spectra.  Returns what every rank now
        holds, ``{(k, restart index in the step's job): spectra}``; None when there is nothing to gather (N = 1)."""
        if gather_mode == "none":
            return None
        from cnmf_amd import dist as cd
        if gather_mode == "rccl":
            hdr = np.array([(i, int(k), rank + world * i) for i, k in enumerate(ks)], dtype=np.int32).reshape(-1, 3)
            return cd.allgather_spectra_rccl(eng, hdr, None, G)        # blk=None: the device-resident spectra store
        import torch
        rows = [(i, int(H.shape[0]), rank + world * i) for i, H in enumerate(H_list)]
        hdr, blk = cd.pack_local(rows, H_list, G)
        merged = cd.allgather_spectra(hdr, blk, G, device=None if tdev == "cpu" else "cuda:%d" % local_rank)
        torch.cuda.synchronize()
        return merged

    last = {}                                                    # what the latest step computed (--dump-outputs)

    def run_step(step, profile):
        ks, seeds, job_restarts = step_jobs(step)
        if gather_mode == "rccl":
            eng.spectra_reset()
            _, _, n_it, viol = eng.nmf_batch(ks, seeds=seeds, warn=False, profile=args.event_stride if profile else 0,
                                             resident=True)
            st = dict(eng.last_stats)
            H = None
            got = gather(None, ks, step)
        else:
            H, _, n_it, viol = eng.nmf_batch(ks, seeds=seeds, warn=False, profile=args.event_stride if profile else 0)
            st = dict(eng.last_stats)
            got = gather(H, ks, step)
        st["n_iter"] = np.asarray(n_it, dtype=np.int64)
        if multi and world > 1:
            assert len(got) == job_restarts, "gather returned %d restarts, the step's job has %d" % (len(got), job_restarts)
        last.update(ks=ks, H=H, merged=got, n_iter=n_it, violation=viol)
        return ks, st, job_restarts

    agg = dict(restarts=0, restart_iters=0, rc_iters=0, outer=0, col_iters=0, passA_ms=0.0,
               passB_ms=0.0, nA=0, nB=0, gpu_ms=0.0, kc=0, nsplit=0, gemm_mode=0, tail_ms=0.0, tail_its=0, tail_live=0,
               job_restarts=0, at_max_iter=0, iters_above_500=0)
    for step in range(args.warmup):
        run_step(step, False)
    barrier()
    t0 = time.perf_counter()
    for step in range(args.warmup, n_steps_total):
        ks, st, job_restarts = run_step(step, True)
        agg["restarts"] += len(ks)
        agg["job_restarts"] += job_restarts
        agg["restart_iters"] += int(st["restart_iterations"])
        agg["at_max_iter"] += int((st["n_iter"] >= 1000).sum())              # (max_iter = 1000: cnmf.py:618-631)
        agg["iters_above_500"] += int(st["n_iter"][st["n_iter"] > 500].sum())
        agg["rc_iters"] += int(st["restart_column_iterations"])
        agg["outer"] += int(st["outer_iterations"])
        agg["col_iters"] += int(st["column_iterations"])
        agg["passA_ms"] += st["passA_ms"]; agg["passB_ms"] += st["passB_ms"]
        agg["nA"] += int(st["passA_launches"]); agg["nB"] += int(st["passB_launches"])
        agg["gpu_ms"] += st["gpu_ms"]; agg["kc"] = int(st["kc"]); agg["nsplit"] = int(st["nsplit"])
        agg["gemm_mode"] = int(st["gemm_mode"])
        agg["tail_ms"] += st["tail_ms"]; agg["tail_its"] += int(st["tail_iterations"]); agg["tail_live"] += int(st["tail_live_columns"])
    barrier()
    elapsed_local = time.perf_counter() - t0
    per_rank = over_ranks([elapsed_local, agg["restarts"], agg["restart_iters"], agg["rc_iters"], agg["col_iters"],
                           agg["gpu_ms"], agg["tail_ms"], agg["outer"]])
    elapsed = float(per_rank[:, 0].max())                      # MAX over ranks
    total_restarts = float(per_rank[:, 1].sum())
    total_riters = float(per_rank[:, 2].sum())
    if args.dump_outputs and args.steps > 0:
        # restart i of this rank is row (shard_rank + shard_world * i) of the step's job (worker_filter), as in gather()
        ids = [(shard_rank + shard_world * i) if strong else (rank + world * i) for i in range(len(last["ks"]))]
        # every rank's (restart, n_iter, violation), padded to the longest shard, so that the per-restart files cover the
        # same restarts as the gathered spectra at any world size (a collective: every rank takes part)
        width = -(-len(ks_all) * args.restarts_per_k // world) if strong and world > 1 else len(ids)
        mine = np.full((3, width), -1.0)
        mine[0, :len(ids)], mine[1, :len(ids)], mine[2, :len(ids)] = ids, last["n_iter"], last["violation"]
        rows = over_ranks(mine.ravel()).reshape(-1, 3, width).transpose(1, 0, 2).reshape(3, -1)
        rows = rows[:, rows[0] >= 0]
        rows = rows[:, np.argsort(rows[0], kind="stable")]
        if rank == 0:
            spectra = last["merged"] if last["merged"] is not None else {
                (int(k), j): h for k, j, h in zip(last["ks"], ids, last["H"])}
            dump_outputs(args.dump_outputs, spectra, rows[0], rows[1], rows[2])

    if rank == 0:
        # roofline of the dominant kernel (rank 0's launches): the MFMA GEMM pass
        flops_per_col_iter = 2.0 * N * G                        # one pass, one component column
        alg_flops_A = flops_per_col_iter * agg["rc_iters"]      # algorithmic (converged columns excluded)
        # the passes of every n-th iteration (--event-stride) are bracketed by HIP events (an event record costs ~6 us of
        # queue time): average duration of the sampled launches x all launches = time in the pass
        launches = max(agg["outer"], 1)
        avgA = agg["passA_ms"] / max(agg["nA"], 1)
        avgB = agg["passB_ms"] / max(agg["nB"], 1)
        tfA = alg_flops_A / max(avgA * launches, 1e-9) / 1e9
        tfB = alg_flops_A / max(avgB * launches, 1e-9) / 1e9
        dom = "A" if avgA >= avgB else "B"
        ach = tfA if dom == "A" else tfB
        split = agg["gemm_mode"] > 0
        per_product = SPLIT_MFMAS_PER_PRODUCT.get(agg["gemm_mode"], 1)
        if split:
            # f32-accurate products on the f16 / bf16 matrix pipe: 2 / 3 / 6 MFMAs per product, so the roofline of the
            # scheme in f32-equivalent flops is the dense peak / that
            peak = BF16_MFMA_PEAK_TFLOPS / per_product
            if agg["gemm_mode"] == 5:
                kern = ("gemm2h_streamk_kernel<1, HI> (pass A: X.Ht; X and the factor as 2 f16 planes each, 3 MFMAs per product)"
                        if dom == "A" else
                        "gemm2h_kernel<1, HI> (pass B: Xt.W; X and the factor as 2 f16 planes each, 3 MFMAs per product)")
            elif agg["gemm_mode"] == 4:
                kern = ("gemm2h_streamk_kernel (pass A: X.Ht; X = one integer f16 plane x per-gene scale, factor = 2 f16 planes)"
                        if dom == "A" else
                        "gemm2h_kernel (pass B: Xt.W; X = one integer f16 plane x per-gene scale, factor = 2 f16 planes)")
            elif agg["gemm_mode"] == 3:
                kern = ("gemm3c_streamk_kernel (pass A: X.Ht; X = one integer bf16 plane x per-gene scale, factor = 3 planes)"
                        if dom == "A" else
                        "gemm3c_kernel (pass B: Xt.W; X = one integer bf16 plane x per-gene scale, factor = 3 planes)")
            else:
                kern = ("gemm3g_streamk_kernel (pass A: X.Ht, 3 x bf16 planes)" if dom == "A"
                        else "gemm3g_kernel (pass B: Xt.W, 3 x bf16 planes)")
        else:
            peak = FP32_MFMA_PEAK_TFLOPS
            kern = "gemm_streamk_kernel<NT> (pass A: X.Ht)" if dom == "A" else "gemm_kernel<NN> (pass B: Xt.W)"
        xbytes = {0: 4, 1: 6, 2: 6, 3: 2, 4: 2, 5: 4}[agg["gemm_mode"]]     # bytes per element of X as the GEMM reads it
        tr, tr_ok = pmc_traffic("passA" if dom == "A" else "passB", agg["gemm_mode"])
        roof = {
            "bound": "mfma",
            "kernel": kern,
            "achieved": ach, "peak": peak, "unit": "TFLOP/s",
            "flop_basis": ("f32-equivalent flops (2.N.G per column and pass); peak = bf16/f16 dense MFMA peak / %d MFMAs per product"
                           % per_product if split else "f32 flops; peak = f32 MFMA peak"),
            "frac": ach / peak,
            # HBM bytes per launch from the PMC counters -- only when the committed profile was taken on THESE kernel
            # sources (load_profile); a stale or unstamped profile is reported in traffic_detail but not used
            "traffic": tr["hbm_bytes_per_launch"] if (tr and tr_ok) else None,
            "traffic_detail": tr,
            "avg_launch_ms": {"passA": avgA, "passB": avgB},
            "launches": {"per_pass": agg["outer"], "timed_with_hip_events": agg["nA"]},
            "achieved_passA": tfA, "achieved_passB": tfB,
            "alg_flops_per_launch": alg_flops_A / launches,
            "issued_flops_per_launch": flops_per_col_iter * agg["kc"],
            "x_stream_GBs": {"passA": N * G * xbytes / max(avgA, 1e-9) / 1e6,
                             "passB": N * G * xbytes / max(avgB, 1e-9) / 1e6,
                             "peak": HBM_PEAK_GBS},
            "gemm_share_of_gpu_time": (avgA + avgB) * launches / max(agg["gpu_ms"], 1e-9),
            # both passes over the whole step: the end-to-end fraction of the scheme's roofline
            "end_to_end": {"achieved": 2.0 * alg_flops_A / max(agg["gpu_ms"], 1e-9) / 1e9, "peak": peak,
                           "frac": 2.0 * alg_flops_A / max(agg["gpu_ms"], 1e-9) / 1e9 / peak,
                           "basis": "2 passes x algorithmic flops / device time of the whole call (all kernels)"},
            "kernel_source_sha256": source_hashes(),
        }
        if tr and tr_ok:
            # the pass is nearly balanced between the two roofs: also quote the HBM side (PMC bytes / measured time)
            dur = (avgA if dom == "A" else avgB) * 1e-3
            roof["hbm"] = {"achieved_GBs": tr["hbm_bytes_per_launch"] / dur / 1e9, "peak_GBs": HBM_PEAK_GBS,
                           "frac": tr["hbm_bytes_per_launch"] / dur / 1e9 / HBM_PEAK_GBS,
                           "traffic_over_algorithmic": tr["hbm_bytes_per_launch"] / tr["algorithmic_bytes_per_launch"]}
        if agg["gemm_mode"] == 4:
            # measured ceiling of THIS instruction stream with everything but the MFMAs removed (tools/
            # probe_gemm2h_ablate.py var 7): the matrix pipe on non-zero data at the clock the power budget allows --
            # not a roofline, but the reason `frac` cannot approach 1.  Read from a stamped profile, never a literal.
            abl, verdict = load_profile("r6_gemm2h_ablation.json")
            if abl and "mfma_only_tflops_issued" in abl:
                issued = ach * per_product * agg["col_iters"] / max(agg["rc_iters"], 1)
                roof["mfma_only_ablation"] = {"tflops_issued": abl["mfma_only_tflops_issued"],
                                              "source": "profiles/r6_gemm2h_ablation.json (production pass-B launch shape, random operands)", "stale": verdict,
                                              "issued_over_mfma_only": (issued / abl["mfma_only_tflops_issued"]) if verdict is None else None,
                                              "production_over_mfma_only_on_the_probes_data": (abl.get("production_tflops_issued", 0.0) / abl["mfma_only_tflops_issued"]),
                                              "note": "the ablation probe multiplies RANDOM operands (the chip clocks to its power budget: the "
                                                      "same launch is ~1.35 x slower there than on the bench's real count plane); the like-for-like "
                                                      "ratio is production_over_mfma_only_on_the_probes_data"}
        if split:
            roof["matrix_pipe"] = {
                "scheme": ("X = n * d detected (n integer <= 2048: one exact f16 plane; d per gene, folded into the factor); "
                           "factor = 2 f16 planes of a * 2^s_row (within 1 ulp_f32, exact for 3 values in 4); 2 exact partial "
                           "products per product; f32 accumulate" if agg["gemm_mode"] == 4 else
                           "X = n * d detected (n integer <= 256: one exact bf16 plane; d per gene, folded into the factor); "
                           "factor = 3 bf16 planes; 3 exact partial products per product; f32 accumulate"
                           if agg["gemm_mode"] == 3 else
                           "x = h + m + l (3 bf16 planes); a*b from the 6 partial products of weight >= 2^-18; f32 accumulate"),
                "mfma_tflops_issued": ach * per_product * agg["col_iters"] / max(agg["rc_iters"], 1),
                "bf16_dense_peak": BF16_MFMA_PEAK_TFLOPS,
                "vs_f32_matrix_peak": ach / FP32_MFMA_PEAK_TFLOPS,
                "note": "launch averages include the tail launches (< 256 packed columns) that run on the exact-f32 pipe",
            }
        mean_it = total_riters / max(total_restarts, 1.0)
        ranks = [{"rank": r, "seconds": float(per_rank[r, 0]), "restarts": int(per_rank[r, 1]),
                  "column_utilisation": float(per_rank[r, 3] / max(per_rank[r, 4], 1.0)),
                  "gpu_ms": float(per_rank[r, 5]), "tail_ms": float(per_rank[r, 6]),
                  "tail_share_of_gpu_time": float(per_rank[r, 6] / max(per_rank[r, 5], 1e-9))} for r in range(per_rank.shape[0])]
        out = {
            "metric": (FALLBACK_METRIC if gather_fallback else "NMF restarts/sec") + " (%dx%dxK%d..%d)" % (N, G, args.kmin, args.kmax),
            "value": total_restarts / elapsed,
            "unit": "restarts/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(args.steps, 1),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            # f32 results; the products run on the f16 / bf16 matrix pipe from exact operand planes
            "dtype": ({1: "f32 (3x3 bf16 planes, f32 accumulate)", 2: "f32 (3x3 bf16 planes, f32 accumulate)",
                       3: "f32 (exact integer bf16 plane x 3 bf16 planes, f32 accumulate)",
                       4: "f32 (exact integer f16 plane x 2 f16 planes with per-row exponent, f32 accumulate)",
                       5: "f32 (2 f16 planes with per-row exponent for X and for the factor, f32 accumulate)"}.get(agg["gemm_mode"], "f32")),
            "data": "synthetic",
            "config": {"workload": "%s: %d cells x %d HVGs synthetic dense, K=%d..%d, %d restarts per K per step (%s), "
                                   "sklearn CD solver tol=1e-4 max_iter=1000, init=random from ledger seeds"
                                   % (args.workload, N, G, args.kmin, args.kmax, args.restarts_per_k,
                                      "ONE job of %d restarts sharded idx %% %d over the GPUs" % (len(ks_all) * args.restarts_per_k, world)
                                      if strong else "per GPU"),
                       "restarts_per_step": int(total_restarts / max(args.steps, 1)),
                       "restarts_per_step_per_gpu": int(agg["restarts"] / max(args.steps, 1)),
                       "packed_columns": agg["kc"], "splitk_passB": agg["nsplit"],
                       "mean_iterations_per_restart": mean_it,
                       # the regime the timed job itself ran in (rank 0's restarts): long, ill-conditioned restarts are where
                       # float32 trajectories drift furthest from float64 ones -- pinned end to end by
                       # tests/test_gpu_golden_big.py::test_C3_pipeline_consensus_vs_sklearn_f64_golden
                       "regime": {"share_of_restarts_at_max_iter": agg["at_max_iter"] / max(agg["restarts"], 1),
                                  "share_of_restart_iterations_in_restarts_above_500": agg["iters_above_500"] / max(agg["restart_iters"], 1)},
                       "restart_iterations_per_s": total_riters / elapsed,
                       "column_utilisation": agg["rc_iters"] / max(agg["col_iters"], 1),
                       "tail": {"ms_per_step": agg["tail_ms"] / max(args.steps, 1),
                                "share_of_gpu_time": agg["tail_ms"] / max(agg["gpu_ms"], 1e-9),
                                "iterations_per_step": agg["tail_its"] / max(args.steps, 1),
                                "mean_live_columns": agg["tail_live"] / max(agg["tail_its"], 1),
                                "meaning": "from the moment the queue of pending restarts ran dry to the end of the call"},
                       "per_rank": ranks,
                       "parallelism": "restart-sharded x%d (%s scaling)" % (world, args.scaling), "gather": gather_mode,
                       "rccl": rccl_info, "gather_fallback": gather_fallback,
                       "torch_in_process": "torch" in sys.modules},
            "roofline": roof,
        }
        if emu:
            out["config"]["emulated_shard"] = {"rank": emu[0], "world": emu[1],
                                               "note": "single GPU running only the shard that rank would own"}
        if args.full and world == 1 and not emu and not args.no_extras and gather_mode == "none":
            # the same job once more WITH queue hints (what the timed steps learned about the iterations per rank, handed back
            # explicitly: Engine.set_iteration_hints) -- reported beside the headline, never part of it: the headline steps
            # each learn their queue order from scratch
            eng.set_iteration_hints(eng.iteration_means())
            try:
                th = time.perf_counter()
                ks_h, st_h, _ = run_step(args.warmup, False)
                dt_h = time.perf_counter() - th
            finally:
                eng.set_iteration_hints(None)
            out["with_queue_hints"] = {"restarts_per_s": len(ks_h) / dt_h, "ms_per_step": 1e3 * dt_h,
                                       "tail_share_of_gpu_time": st_h["tail_ms"] / max(st_h["gpu_ms"], 1e-9),
                                       "column_utilisation": int(st_h["restart_column_iterations"]) / max(int(st_h["column_iterations"]), 1),
                                       "note": "one more step of the same job with cnmf_set_iteration_hints(cnmf_get_iteration_means()); "
                                               "not the headline"}
        if args.full and world == 1 and not emu:
            cpu = None
            if not args.no_cpu_baseline:
                cpu = cpu_baseline(X, mean_it, args.cpu_iters)
                out["cpu_baseline"] = cpu
                out["consensus"] = consensus_wallclock(eng)
            if not args.no_extras:
                rpk = max(1, min(args.restarts_per_k, 20))
                try:
                    out["general_path"] = general_path_step(X, ks_all, by_k, rpk, args.event_stride)
                except Exception as e:                    # an extra must never cost the headline line
                    out["general_path"] = {"error": repr(e)}
                try:
                    out["e2e"] = e2e_wallclock(eng, C, X, ks_all, args.restarts_per_k, cpu["value"] if cpu else None)
                except Exception as e:
                    out["e2e"] = {"error": repr(e)}
                try:
                    out["kl_non_zero_path"] = kl_non_zero_path(ks_all)
                except Exception as e:
                    out["kl_non_zero_path"] = {"error": repr(e)}
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    os.close(json_fd)
    barrier()
    if multi and world > 1:
        try:                                      # (every rank is past the barrier: nobody reads the reports any more)
            os.remove("%s.status.%d" % (id_path, rank))
        except (OSError, NameError):
            pass
    if dist is not None:
        dist.destroy_process_group()
    if gather_mode == "rccl":
        eng.comm_finalize()
    eng.close()


if __name__ == "__main__":
    main()
