"""The plan of the coordinate-descent GEMM passes and sweeps (cnmf_amd/csrc/pass_plan.h) on the CPU:
tests/host/pass_plan_main.cpp, compiled with the address and undefined-behaviour sanitizers as a stand-alone program.

``check``: hand-derived expectations -- the stream-K plans at the 50 176 x 2 048 shape (unit ranges cover the work once,
flags count the boundaries inside a tile, flags sit at ``jt * MG + mg``), the "off" rules, split counts never above what
was asked, no planned launch writing more partial planes than ``size_splits`` sized, ``g2_form`` over its 128 inputs
against the two if-ladders it replaced (typed out in the program; 9 and 14 distinct kernel instantiations), ``sweep_form``
over its 16 inputs and the flat-address predicate at its threshold, and ``x_launches_fit`` on both sides of the three
grid.y limits of the X-side builder and detection launches (16 776 960 / 16 777 216 rows where the count detection runs,
4 194 240 / 4 194 304 rows where X is split into bf16 planes, ``G_pad`` = 65 535 * 256 and one tile more).

``golden``: every planner over padded shapes {256, 512, 2 048, 50 176, 1 100 032}^2, widths {32 ... 256, 512, 1 024} and the
knobs ``no_streamk`` in {0, 1}, ``wg_slots`` in {0, 32, 128}, ``g2_nsub`` in {1, 2}, against tests/golden/pass_plans.json
(one line per shape and width; stream-K plans as their cut counts and an FNV-1a digest of their fields and flags).  That
file was recorded ONCE from the function bodies of commit 714445a, the last one before the planners moved into pass_plan.h: the bodies of plan_streamk, plan_streamk3, gemm3_wg_slots, g2_full_mask,
gemm2h_splits, gemm2h_nsub, split2h_wide, split2h_col_groups, pick_nsplit3 (gemm_host.hip.h) and sweep_chunks, sweep_parts,
pick_nsplit, effective_splits, pick_nsplit_A, pick_nsplit_A3, pick_kc and ensure_batch's sizing expression
(batch_host.hip.h), pasted verbatim into a scratch program beside a stub ``cnmf_ctx {N_pad, G_pad, knobs}`` and the
thread-local knob pointer they read, with thin adapters giving them the signatures of pass_plan.h, and the ``golden()``
function of pass_plan_main.cpp printing the table.  To redo it: ``git show 714445a:cnmf_amd/csrc/...``, the same adapters.

No GPU test that runs in a few seconds reaches the flat-address (A64) sweep forms or a matrix above 2^20 padded cells: for
the 1 100 032-cell plans and for the A64 choice this table and ``check`` are the only check there is."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_plan") / "pass_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "host", "pass_plan_main.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_includes_the_standard_library_only():
    src = open(os.path.join(ROOT, "cnmf_amd", "csrc", "pass_plan.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", src, flags=re.M)
    assert includes and all(re.fullmatch(r"<[a-z_]+>", i) for i in includes), includes


def test_hand_derived_expectations(program):
    out = subprocess.run([program, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-4000:]


def test_every_planner_matches_the_recorded_plans(program):
    out = subprocess.run([program, "golden"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    got = json.loads(out.stdout)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "pass_plans.json")))
    assert len(want["records"]) == 5 * 5 * 6
    assert got["wg_slots"] == want["wg_slots"] and got["pick_kc"] == want["pick_kc"]
    for g, w in zip(got["records"], want["records"]):
        assert g == w, (w["N_pad"], w["G_pad"], w["KC"])
    assert len(got["records"]) == len(want["records"])
