"""The tap-GEMM planner (csrc/tapgemm_plan.cpp) held to a recorded behaviour, on the CPU: tests/golden/tapgemm_plans.json holds
the plan and the split-K workspace size that the library of the commit named in it answered for ~550 launches
(tests/golden/make_plan_golden.py says which, and why those).  Planner refactors must reproduce every row exactly; a change
that MEANS to move a plan regenerates the file and says so."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from vgen_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_plan_golden as mg  # noqa: E402


def _golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "tapgemm_plans.json")))
    assert tuple(g["fields"]) == mg.FIELDS
    return {f"{grp}/{name}": row for grp in ("cases", "bench", "direct") for name, row in g[grp].items()}


def test_every_recorded_launch_gets_its_recorded_plan():
    l = lib.load()
    rows = _golden()
    assert len(rows) >= 500
    wrong = {name: (tuple(row[-4:]), mg.ask(l, row)) for name, row in rows.items() if mg.ask(l, row) != tuple(row[-4:])}
    assert not wrong, wrong
    # the fixture reaches every block shape, every column tile / panel width, split-K and none, tabled and planned rows
    assert {r[-4] for r in rows.values()} == {0, 1, 2, 3, 4, 5}
    assert {r[-3] for r in rows.values()} == {64, 80, 128, 160, 256}
    assert {r[-2] > 1 for r in rows.values()} == {False, True} and {r[15] >= 0 for r in rows.values()} == {False, True}


def test_planner_is_host_only_and_clean_under_sanitizers(tmp_path):
    """csrc/tapgemm_plan.cpp + tests/plan_driver.cpp (its own main, its own vgen_set_error) built by the HOST compiler with
    -fsanitize=address,undefined and run as a process of its own: the unit needs nothing of HIP, agrees with the golden
    outside the library, and installs / replaces / empties / resets the plan table without a leak or a stale read."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rows = _golden()
    data = tmp_path / "rows.txt"
    data.write_text("".join(" ".join(str(v) for v in row) + "\n" for row in rows.values()))
    exe = tmp_path / "plan_driver"
    src = [os.path.join(ROOT, "vgen_amd", "csrc", "tapgemm_plan.cpp"), os.path.join(ROOT, "tests", "plan_driver.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include")] + src + ["-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"{len(rows)} rows ok" in r.stdout, r.stdout[-2000:]
