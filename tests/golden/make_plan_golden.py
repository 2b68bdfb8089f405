"""Regression fixture of the tap-GEMM PLANNER: the (block shape, BN, split-K) and the workspace size that the library of a
chosen commit (its sha goes into the file) answers for a fixed set of launches, so that a later host-side refactor of the
planner can be held to "same plan for every launch" without trusting the code under test.  Only the C ABI is used to ask:
`vgen_tapgemm_query_plan`, `vgen_tapgemm_ws_bytes`, `vgen_tapgemm_set_plans`; the planner never dereferences an operand, so
everything runs on the CPU.

Three groups of launches:
  cases   every spec of tests/kernel_cases.py (`tapgemm_cases`, `splitk_specs`, `panel_cases` plain and dual-W,
          `tapgemm_dw_cases`) in fp16 and bf16, and every `r06_shape_cases` spec twice: without a plan table, and with its
          one-row table installed;
  bench   every launch signature of the benchmark step (tests/test_abi_contract.py::_signatures), crossed with the residual
          and column-statistics flags as test_plans_of_the_benchmark_launches_are_legal sweeps them;
  direct  rows built by hand so that every branch of the planner's legality rule and of the panel rule is reached: row bias,
          two-term output rows, an N only the 64-column tile divides, M just below and at the panel's 2048-row threshold,
          K = 640 with and without a two-term weight.

A row is a flat list of integers, FIELDS below: the planner's inputs (sizes, strides, which optional pointers are set), the
plan of the one-row table installed for the query (`t_shape` = -1: none; its key is the row's own signature) and the answer.
tests/test_abi_contract.py rebuilds the argument block from the row and asserts exact equality; the stand-alone planner
driver (tests/plan_driver.cpp) reads the same rows.

    python tests/golden/make_plan_golden.py     # rewrites tests/golden/tapgemm_plans.json from the commit that is checked out
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vgen_amd import lib  # noqa: E402

FIELDS = ("dtype", "mode", "M", "N", "C1", "C2", "taps", "epilogue", "out_dtype", "dualw", "split_out", "ldo", "ldr",
          "rowbias_ld", "flags",                       # flags: residual | rowbias << 1 | colstats << 2 (the plan table's)
          "t_shape", "t_bn", "t_splitk", "shape", "bn", "splitk", "ws_bytes")
FAKE = 0x7f0000001000        # an aligned non-null address: the planner never dereferences operands


def args_of(row):
    """the vgen_tapgemm_args block a row describes (what the planner reads of it)"""
    r = dict(zip(FIELDS, row))
    a = lib.TapGemmArgs()
    for k in ("dtype", "mode", "M", "N", "C1", "C2", "taps", "epilogue", "out_dtype", "dualw", "split_out", "ldo", "ldr",
              "rowbias_ld"):
        setattr(a, k, r[k])
    a.A, a.W, a.out, a.lda, a.lda2 = FAKE, FAKE, FAKE, r["C1"], r["C2"]
    a.A2 = FAKE if r["C2"] else 0
    a.residual = FAKE if r["flags"] & 1 else 0
    a.rowbias, a.rows_per_rb = (FAKE, 1) if r["flags"] & 2 else (0, 0)
    a.colstats = FAKE if r["flags"] & 4 else 0
    return a


def table_of(row):
    """the one-row plan table (12 int64, vgen_tapgemm_set_plans) of a row, or None"""
    r = dict(zip(FIELDS, row))
    if r["t_shape"] < 0:
        return None
    return (C.c_int64 * 12)(r["mode"], r["M"], r["N"], r["C1"], r["C2"], r["taps"], r["epilogue"], r["out_dtype"], r["flags"],
                            r["t_shape"], r["t_bn"], r["t_splitk"])


def ask(l, row):
    """-> (shape, bn, splitk, ws_bytes) the library answers for the inputs of a row"""
    a, tab = args_of(row), table_of(row)
    out3 = (C.c_int32 * 3)()
    try:
        if tab is not None:
            assert l.vgen_tapgemm_set_plans(tab, 1) == 0
        assert l.vgen_tapgemm_query_plan(C.byref(a), out3) == 0, row
        return tuple(out3) + (int(l.vgen_tapgemm_ws_bytes(C.byref(a))),)
    finally:
        if tab is not None:
            l.vgen_tapgemm_set_plans(None, -1)


def inputs_of(a, table=(-1, 0, 0)):
    flags = (1 if a.residual else 0) | (2 if a.rowbias else 0) | (4 if a.colstats else 0)
    return [a.dtype, a.mode, a.M, a.N, a.C1, a.C2, a.taps, a.epilogue, a.out_dtype, a.dualw, a.split_out, a.ldo, a.ldr,
            a.rowbias_ld, flags] + list(table)


def case_rows():
    import torch
    import kernel_cases as kc
    from vgen_amd import ops
    be = ops.HipBackend()
    rows = {}
    for tag, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        groups = {"tapgemm": kc.tapgemm_cases(dt), "splitk": kc.splitk_specs(dt), "panel": kc.panel_cases(dt),
                  "panel_dw": kc.panel_cases(dt, dualw=True), "dw": kc.tapgemm_dw_cases(dt)}
        for gname, specs in groups.items():
            for name, spec in specs.items():
                rows[f"{gname}/{name}/{tag}"] = inputs_of(be._tapgemm_args(spec, alloc=False)[0])
        for name, (spec, plan) in kc.r06_shape_cases(dt).items():
            a = be._tapgemm_args(spec, alloc=False)[0]
            rows[f"r06/{name}/{tag}"] = inputs_of(a)
            rows[f"r06/{name}/{tag}/tabled"] = inputs_of(a, plan)
    return rows


def bench_rows():
    import test_abi_contract as tc
    rows = {}
    for mode, M, N, C1, C2, taps, epi, f32, dw in tc._signatures():
        for colstats in (False, True):
            for residual in (False, True):
                if colstats and (not f32 or epi):
                    continue
                n_out = N // 2 if epi else N
                flags = (1 if residual else 0) | (4 if colstats else 0)
                name = f"{mode}_{M}x{N}x{C1}+{C2}_e{epi}_{'f32' if f32 else 'f16'}{'_dw' if dw else ''}_f{flags}"
                rows[name] = [lib.VGEN_F16, mode, M, N, C1, C2, taps, epi, lib.VGEN_F32 if f32 else lib.VGEN_F16, int(dw), 0,
                              n_out, n_out if residual else 0, 0, flags, -1, 0, 0]
    return rows


def direct_rows():
    def lin(M=57344, N=320, C1=320, f32=True, epi=lib.EPI_NONE, dw=0, split_out=0, ldo=None, ldr=0, rowbias_ld=0, flags=0,
            table=(-1, 0, 0), mode=lib.TAP_LINEAR, taps=1, C2=0):
        n_out = N // 2 if epi else N
        return [lib.VGEN_F16, mode, M, N, C1, C2, taps, epi, lib.VGEN_F32 if f32 else lib.VGEN_F16, dw, split_out,
                n_out if ldo is None else ldo, ldr, rowbias_ld, flags] + list(table)
    return {
        "rowbias_keeps_off_the_panel": lin(rowbias_ld=320, flags=2),
        "rowbias_unaligned_ld_no_splitk": lin(M=448, N=1280, C1=5120, rowbias_ld=1282, flags=2),
        "rowbias_splitk": lin(M=448, N=1280, C1=5120, rowbias_ld=1280, flags=2),
        "split_out_keeps_off_the_panel": lin(f32=False, split_out=1, ldo=640),
        "split_out_no_splitk": lin(M=448, N=1280, C1=5120, f32=False, split_out=1, ldo=2560),
        "N_only_64_divides": lin(M=3000, N=192, C1=1280),
        "N_only_64_divides_geglu": lin(M=3000, N=192, C1=1280, f32=False, epi=lib.EPI_GEGLU),
        "N_tail_not_64": lin(M=3000, N=200, C1=1280),
        "N_odd_not_vec": lin(M=3000, N=77, C1=1280),
        "bn64_tabled_where_128_divides": lin(M=448, N=1280, C1=1280, table=(0, 64, 1)),
        "bn64_tabled_illegal_N": lin(M=448, N=200, C1=1280, table=(0, 64, 1)),
        "bn160_tabled_geglu_illegal": lin(M=3000, N=640, C1=1280, f32=False, epi=lib.EPI_GEGLU, table=(0, 160, 1)),
        "splitk_tabled_over_bound": lin(M=448, N=1280, C1=1280, table=(0, 128, 6)),
        "dual_tabled_colstats": lin(M=9000, N=1280, C1=128, flags=4, table=(1, 128, 1)),
        "pp128_tabled_colstats_illegal": lin(M=9000, N=1280, C1=128, flags=4, table=(2, 128, 1)),
        "pp256_tabled_ldo_not_8": lin(M=1000, N=512, C1=1280, f32=False, ldo=516, table=(4, 256, 1)),
        "panel_M_2047": lin(M=2047),
        "panel_M_2048": lin(M=2048),
        "panel_M_2047_dw": lin(M=2047, dw=1),
        "panel_M_2048_dw": lin(M=2048, dw=1),
        "panel_k640": lin(M=14336, N=640, C1=640, flags=1, ldr=640),
        "panel_k640_dw": lin(M=14336, N=640, C1=640, dw=1),
        "panel_k640_geglu": lin(M=14336, N=5120, C1=640, f32=False, epi=lib.EPI_GEGLU),
        "panel_k640_N_not_80": lin(M=14336, N=576, C1=640),
        "panel_geglu_f32_not_taken": lin(N=2560, epi=lib.EPI_GEGLU),
        "panel_geglu_dw_64": lin(N=2560, f32=False, epi=lib.EPI_GEGLU, dw=1),
        "panel_ldo_not_4": lin(ldo=322),
        "panel_ldo16_not_8": lin(f32=False, ldo=324),
        "panel_ldr_not_4": lin(flags=1, ldr=322),
        "panel_N_not_160": lin(N=336),
        "panel_tabled_away": lin(N=2560, f32=False, epi=lib.EPI_GEGLU, table=(4, 256, 1)),
        "panel_dw_ignores_table": lin(dw=1, table=(0, 160, 1)),
        "temporal_not_panel": lin(M=57344, N=320, C1=64, mode=lib.TAP_TEMPORAL3, taps=3),
        "conv_skipseg_colstats": lin(M=57344, N=320, C1=320, C2=640, mode=lib.TAP_CONV3X3, taps=9, flags=5, ldr=320),
    }


def main():
    sha = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "vgen_amd/csrc", "include"], cwd=ROOT, capture_output=True,
                           text=True, check=True).stdout.strip()
    assert not dirty, f"record from a clean checkout:\n{dirty}"
    l = lib.load()
    res = {}
    for gname, rows in (("cases", case_rows()), ("bench", bench_rows()), ("direct", direct_rows())):
        res[gname] = {k: v + list(ask(l, v + [0, 0, 0, 0])) for k, v in rows.items()}
        plans = {tuple(r[-4:-1]) for r in res[gname].values()}
        print(gname, len(rows), "rows;", "shapes", sorted({p[0] for p in plans}), "BN", sorted({p[1] for p in plans}),
              "split-K", sorted({p[2] for p in plans}), flush=True)
    with open(os.path.join(HERE, "tapgemm_plans.json"), "w") as f:          # one row per line
        groups = ",\n".join('"%s":{\n%s\n}' % (g, ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                                                              for k, v in rows.items())) for g, rows in res.items())
        f.write('{"recorded_from":"%s","fields":%s,\n%s}\n' % (sha, json.dumps(list(FIELDS), separators=(",", ":")), groups))


if __name__ == "__main__":
    main()
