"""The round scheduler of the multiplicative-update driver (cnmf_amd/csrc/mu_sched.h) on the CPU: tests/host/mu_sched_main.cpp
drives it against a fake device whose jobs have scripted divergences, compiled with the address and undefined-behaviour
sanitizers as a stand-alone program.  Hand-derived stopping points and evaluation counts, and the invariants of seeded
jobs (70 and 33 jobs through 32 slots, 5 through one): every job placed and retired once, evaluations only at aligned
points or at max_iter, a job's n_iter and err independent of the batch, refills beside live slots."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mu_sched") / "mu_sched_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "host", "mu_sched_main.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_includes_the_standard_library_only():
    src = open(os.path.join(ROOT, "cnmf_amd", "csrc", "mu_sched.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", src, flags=re.M)
    assert includes and all(re.fullmatch(r"<[a-z_]+>", i) for i in includes), includes


def test_expectations_and_invariants(program):
    out = subprocess.run([program], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-4000:]
