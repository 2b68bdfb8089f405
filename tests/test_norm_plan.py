"""The norm planner (csrc/norm_plan.cpp) held to a recorded behaviour, on the CPU: tests/golden/norm_plans.json holds, for
~1700 GroupNorm shapes and 80 LayerNorm shapes, the algorithm, split count, slab height, LDS size, grid and workspace size
that the dispatch of the commit named in it gave (tests/golden/make_norm_plan_golden.py says which shapes, and from what).
Planner refactors must reproduce every row exactly; a change that MEANS to move a threshold regenerates the file and says so."""
import ctypes as C
import os
import shutil
import subprocess
import sys

from vgen_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_norm_plan_golden as mg  # noqa: E402

VGEN_E_BADARG = -1


def test_every_recorded_shape_gets_its_recorded_plan():
    l = lib.load()
    gn, ln = mg.load_golden()
    assert len(gn) >= 500 and len(ln) >= 60
    wrong = {name: (tuple(row[5:9]), mg.ask_gn(l, row)[:4]) for name, row in gn.items() if mg.ask_gn(l, row)[:4] != tuple(row[5:9])}
    assert not wrong, wrong
    wrong = {name: (tuple(row[3:]), mg.ask_ln(l, row)) for name, row in ln.items() if mg.ask_ln(l, row) != tuple(row[3:])}
    assert not wrong, wrong
    # the fixture reaches all five GroupNorm paths, both LayerNorm kernels (NS = 0: one-shot) and all three LPR
    assert {r[5] for r in gn.values()} == set(range(len(mg.PATHS)))
    assert {r[4] for r in ln.values()} == {0, 5, 8} and {r[3] for r in ln.values()} == {16, 32, 64}
    assert {(r[3], r[4] > 0) for r in ln.values()} == {(lpr, s) for lpr in (16, 32, 64) for s in (False, True)}


def test_workspace_size_is_unchanged():
    l = lib.load()
    gn, _ = mg.load_golden()
    wrong = {name: (row[9], int(l.vgen_groupnorm_ws_bytes(row[0], row[1]))) for name, row in gn.items()
             if int(l.vgen_groupnorm_ws_bytes(row[0], row[1])) != row[9]}
    assert not wrong, wrong
    assert len({r[9] for r in gn.values()}) >= 5


def test_queries_refuse_what_the_entries_refuse_without_a_gpu():
    l = lib.load()
    o4, o3 = (C.c_int32 * 4)(), (C.c_int32 * 3)()
    gn = lambda nb=2, S=1792, C1=320, C2=0, groups=32, cs=0, out=o4: l.vgen_groupnorm_query_plan(nb, S, C1, C2, groups, cs, out)  # noqa: E731
    assert gn() == 0 and gn(cs=1) == 0
    assert gn(out=None) == VGEN_E_BADARG
    assert gn(groups=7) == VGEN_E_BADARG and b"groups=7" in l.vgen_last_error()
    assert gn(C1=322) == VGEN_E_BADARG and gn(C1=4096) == VGEN_E_BADARG and gn(C1=2048, C2=2048) == VGEN_E_BADARG
    assert gn(nb=70000) == VGEN_E_BADARG and gn(nb=0) == VGEN_E_BADARG and gn(S=0) == VGEN_E_BADARG
    assert gn(S=1800) == 0 and gn(S=1800, cs=1) == VGEN_E_BADARG and b"64-row slab" in l.vgen_last_error()
    ln = lambda M=64, d=320, dt=lib.VGEN_F16, out=o3: l.vgen_layernorm_query_plan(M, d, dt, out)  # noqa: E731
    assert ln() == 0 and tuple(o3) == (16, 5, 4)
    assert ln(out=None) == VGEN_E_BADARG and ln(dt=5) == VGEN_E_BADARG
    assert ln(d=322) == VGEN_E_BADARG and ln(d=1 << 20) == VGEN_E_BADARG and ln(M=1 << 33) == VGEN_E_BADARG
    assert ln(M=0) == 0 and o3[2] == 0                      # an empty batch is a no-op of vgen_layernorm: no block


def test_planner_is_host_only_and_clean_under_sanitizers(tmp_path):
    """csrc/norm_plan.cpp + tests/norm_plan_driver.cpp (its own main, its own vgen_set_error) built by the HOST compiler with
    -fsanitize=address,undefined and run as a process of its own: the unit needs nothing of HIP and agrees with the golden
    outside the library."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    gn, ln = mg.load_golden()
    data = tmp_path / "rows.txt"
    data.write_text("".join("G " + " ".join(str(v) for v in row) + "\n" for row in gn.values()) +
                    "".join("L " + " ".join(str(v) for v in row) + "\n" for row in ln.values()))
    exe = tmp_path / "norm_plan_driver"
    src = [os.path.join(ROOT, "vgen_amd", "csrc", "norm_plan.cpp"), os.path.join(ROOT, "tests", "norm_plan_driver.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include")] + src + ["-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("VGEN_GN_FUSED_MAX_MB", "VGEN_GN_REGS")}
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"{len(gn) + len(ln)} rows ok" in r.stdout, r.stdout[-2000:]
