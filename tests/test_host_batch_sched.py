"""The restart scheduler of the coordinate-descent batch (cnmf_amd/csrc/batch_sched.h) on the CPU: tests/host/batch_sched_main.cpp
drives it against a fake device, compiled with the address and undefined-behaviour sanitizers as a stand-alone program.
``check``: hand-written expectations (queue order, column allocator, re-packing plans, tail widths) and the invariants of
seeded synthetic jobs.  ``replay``: the pinned GPU jobs of tests/test_gpu_schedule_pins.py with every restart ``max_iter``
iterations long -- the scheduler alone must arrive at the statistics the device run reported (tests/golden/schedule_pins.json)."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYED = ("outer_iterations", "column_iterations", "restart_iterations", "tail_iterations", "tail_live_columns")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_sched") / "batch_sched_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "host", "batch_sched_main.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_includes_the_standard_library_only():
    src = open(os.path.join(ROOT, "cnmf_amd", "csrc", "batch_sched.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", src, flags=re.M)
    assert includes and all(re.fullmatch(r"<[a-z_]+>", i) for i in includes), includes


def test_expectations_and_invariants(program):
    out = subprocess.run([program, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-4000:]


def test_replay_of_the_pinned_gpu_jobs(program):
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "schedule_pins.json")))
    for name in ("A", "B"):
        for i, call in enumerate(pins[name]["calls"]):
            assert call["n_iter_all_max_iter"]
            out = subprocess.run([program, "replay", str(call["kc"]), str(call["gemm_mode"]), "2", "0", str(pins[name]["max_iter"]),
                                  ",".join(str(k) for k in call["ks"])], capture_output=True, text=True)
            assert out.returncode == 0, out.stderr[-4000:]
            assert json.loads(out.stdout) == {f: call[f] for f in REPLAYED}, (name, i)
