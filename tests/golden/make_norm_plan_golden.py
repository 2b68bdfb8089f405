"""Regression fixture of the norm PLANNER (csrc/norm_plan.cpp): which of the five GroupNorm algorithms and which LayerNorm
kernel a launch takes, with the split count, slab height, dynamic LDS, grid and workspace size, for a fixed set of shapes, so
that a host-side refactor of the dispatch can be held to "same answer for every shape" without trusting the code under test.

The committed file was recorded on the commit whose sha it names, BEFORE the planner existed: from the Python restatement
of groupnorm_impl's inline ladder that tests/norm_cases.py then held (`gn_path`, `gn_nsplit`, `ln_lpr`, the streaming-width
table; `restated` below is the only reader of those names), and the workspace size from that commit's library.  On a
checkout whose library has `vgen_groupnorm_query_plan` the same rows are asked of the library instead (`ask_gn`, `ask_ln`:
what tests/test_norm_plan.py and tests/norm_plan_driver.cpp compare with); nothing is launched, so everything runs on the CPU.

GroupNorm rows (GN_FIELDS; 32 groups throughout, as in the reference):
  cases   every row of norm_cases.GN_SHAPES, with and without producer statistics where S % 64 == 0;
  step    every (nb, S, C) of tools/norm_ab.py (read from its source: the file runs on import) and of
          kernel_cases.GN_CS_CASES;
  sweep   nb x S x C below, C2 = 0 and one C1 | C2 split each, with and without statistics: S straddles every threshold of
          the ladder at C = 1280 (614 | 615 LDS slice, 1836 | 1837 register slice), the 24 / 96 MiB rule, the nsplit floor
          and cap, the 2048-item cs threshold.
LayerNorm rows (LN_FIELDS): the six streaming widths and four other widths x M around the rows per block, a ragged wrap of
the 2048-block grid, the benchmark's 57344 x all three output types.

    python tests/golden/make_norm_plan_golden.py     # rewrites tests/golden/norm_plans.json from the commit checked out
"""
from __future__ import annotations

import ast
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

GROUPS = 32
PATHS = ("fused", "regs", "stream", "cs256", "cs1024")       # enum GnPath of csrc/norm_plan.h, in its order
GN_FIELDS = ("nb", "S", "C1", "C2", "has_cs", "path", "nsplit", "rows_per", "lds_bytes", "ws_bytes")
LN_FIELDS = ("M", "d", "dtype", "lpr", "ns", "grid")
SWEEP_NB = (1, 2, 4, 16, 32)
SWEEP_S = (28, 49, 112, 448, 614, 615, 1792, 1836, 1837, 7168, 7344, 7345, 13056, 28672, 114688)
SWEEP_C = (128, 320, 640, 960, 1280, 1920, 2560, 3072)
LN_D = (320, 512, 640, 1024, 1280, 2048, 64, 192, 768, 1536)
LN_M = (1, 3, 5, 4097, 65539, 57344)


def ask_gn(l, row):
    """-> (path, nsplit, rows per slab, dynamic LDS bytes, workspace bytes) the library answers for the inputs of a row"""
    nb, S, C1, C2, has_cs = row[:5]
    out4 = (C.c_int32 * 4)()
    assert l.vgen_groupnorm_query_plan(nb, S, C1, C2, GROUPS, has_cs, out4) == 0, row
    return tuple(out4) + (int(l.vgen_groupnorm_ws_bytes(nb, S)),)


def ask_ln(l, row):
    """-> (lanes per row, NS (0 = the one-shot kernel), grid)"""
    out3 = (C.c_int32 * 3)()
    assert l.vgen_layernorm_query_plan(row[0], row[1], row[2], out3) == 0, row
    return tuple(out3)


def restated(l):
    """the same two answers from the restatement of tests/norm_cases.py, for a library without the query entries"""
    import norm_cases as nc
    ns_of = {d: d // (4 * nc.ln_lpr(d)) for d in nc.LN_STREAM_WIDTHS}        # d = NS * 4 * LPR exactly

    def gn(l_, row):
        nb, S, C1, C2, has_cs = row[:5]
        path = nc.gn_path(nb, S, C1, C2, bool(has_cs))
        ns, rp = nc.gn_nsplit(nb, S, C1 + C2)[:2] if path not in ("fused", "regs") else (0, 0)
        lds = S * ((C1 + C2) // GROUPS) * 4 if path == "fused" else 0      # the staged (batch, group) slice
        return PATHS.index(path), ns, rp, lds, int(l.vgen_groupnorm_ws_bytes(nb, S))

    def ln(l_, row):
        M, d, dtype = row[:3]
        lpr = nc.ln_lpr(d)
        ns = ns_of.get(d, 0) if dtype != lib.VGEN_F32 else 0
        row_groups = -(-M // (256 // lpr))
        return lpr, ns, min(row_groups, 2048) if ns else row_groups
    return gn, ln


def norm_ab_shapes():
    """every (nb, S, C) literal of the loops of tools/norm_ab.py"""
    tree = ast.parse(open(os.path.join(ROOT, "tools", "norm_ab.py")).read())
    shapes = []
    for node in ast.walk(tree):
        if isinstance(node, ast.For) and isinstance(node.iter, ast.List):
            for t in node.iter.elts:
                if isinstance(t, ast.Tuple) and len(t.elts) == 3:
                    shapes.append(tuple(ast.literal_eval(e) for e in t.elts))
    assert len(shapes) >= 16, shapes
    return sorted(set(shapes))


def gn_rows():
    import kernel_cases as kc
    import norm_cases as nc
    rows = {"cases": {}, "step": {}, "sweep": {}}

    def add(group, nb, S, C1, C2):
        for has_cs in (0, 1) if S % 64 == 0 else (0,):
            rows[group][f"{nb}x{S}x{C1}+{C2}{'/cs' if has_cs else ''}"] = [nb, S, C1, C2, has_cs]
    for shapes in nc.GN_SHAPES.values():
        for s in shapes:
            add("cases", *s)
    for nb, S, Cn in norm_ab_shapes():
        add("step", nb, S, Cn, 0)
    for nb, S, C1, C2, _ in kc.GN_CS_CASES:
        add("step", nb, S, C1, C2)
    for nb in SWEEP_NB:
        for S in SWEEP_S:
            for Cn in SWEEP_C:
                add("sweep", nb, S, Cn, 0)
                C1 = -(-Cn // 128) * 64                 # the multiple of 64 at or above half
                add("sweep", nb, S, C1, Cn - C1)
    return rows


def ln_rows():
    rows = {}
    for d in LN_D:
        for M in LN_M:
            for dtype in (lib.VGEN_F16,) if M != 57344 else (lib.VGEN_BF16, lib.VGEN_F16, lib.VGEN_F32):
                rows[f"{M}x{d}/{dtype}"] = [M, d, dtype]
    return rows


def load_golden():
    g = json.load(open(os.path.join(HERE, "norm_plans.json")))
    assert tuple(g["gn_fields"]) == GN_FIELDS and tuple(g["ln_fields"]) == LN_FIELDS
    gn = {f"{grp}/{name}": row for grp in ("cases", "step", "sweep") for name, row in g[grp].items()}
    return gn, g["layernorm"]


def main():
    sha = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "vgen_amd/csrc", "include", "tests/norm_cases.py"], cwd=ROOT,
                           capture_output=True, text=True, check=True).stdout.strip()
    assert not dirty, f"record from a clean checkout:\n{dirty}"
    l = lib.load()
    gn, ln = (ask_gn, ask_ln) if hasattr(l, "vgen_groupnorm_query_plan") else restated(l)
    res = {g: {k: v + list(gn(l, v)) for k, v in rows.items()} for g, rows in gn_rows().items()}
    res["layernorm"] = {k: v + list(ln(l, v)) for k, v in ln_rows().items()}
    every = [r for g in ("cases", "step", "sweep") for r in res[g].values()]
    print(len(every), "GroupNorm rows:", {p: sum(r[5] == i for r in every) for i, p in enumerate(PATHS)}, flush=True)
    print(len(res["layernorm"]), "LayerNorm rows: lpr", sorted({r[3] for r in res["layernorm"].values()}), "ns",
          sorted({r[4] for r in res["layernorm"].values()}), flush=True)
    with open(os.path.join(HERE, "norm_plans.json"), "w") as f:          # one row per line
        groups = ",\n".join('"%s":{\n%s\n}' % (g, ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                                                              for k, v in rows.items())) for g, rows in res.items())
        f.write('{"recorded_from":"%s","gn_fields":%s,"ln_fields":%s,\n%s}\n' % (
            sha, json.dumps(list(GN_FIELDS), separators=(",", ":")), json.dumps(list(LN_FIELDS), separators=(",", ":")), groups))


if __name__ == "__main__":
    main()
