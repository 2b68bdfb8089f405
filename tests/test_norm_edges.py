"""GroupNorm (its five algorithms: gn_fused, gn_regs, the streaming pipeline, gn_finalize_cs<256 | 1024>) and LayerNorm
(one-shot and streaming kernels, VGEN_F32 output) on ill-conditioned inputs: per-ELEMENT parity with an fp64 reference of the
fp32 tensor the kernel read, under the bound derived in tests/norm_cases.py (one output rounding + a counted fp32 part that
allows NO (mean / sigma)^2 growth of the rstd error; never tuned to what a GPU gives), plus guard rows: inputs framed by
NaN rows, outputs written through the C ABI between sentinel rows.

CPU tests (unmarked): every family has its property at every shape used; torch's own fp32 norms sit inside the bound; the
CPU models of the kernels' arithmetic stay under 0.7; eight modelled mistakes are each CAUGHT by the statistic on the family
built for them (two of them are shown to pass the whole-tensor rel-L2 of the older tests); the case table reaches every
dispatch path and edge of groupnorm_impl.  GPU tests: the real kernels.  Measured values: DESIGN.md section 3.4."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402

DEV = "cuda:0"
DTN = ["fp16", "bf16"]
_sid = lambda s: "x".join(str(v) for v in s)      # noqa: E731


# ---- CPU: families, reference inside the bound -----------------------------------------------------------------------
def _torch_inside(x, nb, S, groups, gamma, beta, silu, what):
    """torch's fp32 norm of x against the fp64 reference: fp32 output <= 0.5 of the fp32 part, rounded once <= 1."""
    ref = nc.reference(x, nb, S, groups, gamma, beta, nc.EPS, silu)
    y32 = nc.torch_norm(x, nb, S, groups, gamma, beta, nc.EPS, silu)
    w32 = nc.worst_ratio(y32, ref.y, ref.f32)
    assert w32 <= 0.5, (what, "fp32 part used", w32)
    worst = 0.0
    for dt in nc.DTS.values():
        w = nc.worst_ratio(y32.to(dt), ref.y, nc.bound(ref, dt))
        assert w <= 1, (what, dt, w)
        worst = max(worst, w)
    return w32, worst


@pytest.mark.parametrize("path,shape", [(p, s) for p, ss in nc.GN_SHAPES.items() for s in ss], ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_groupnorm_families_and_torch_fp32_inside_the_bound(path, shape):
    """Every (family, shape) the GPU tests use: the family has its property, and torch's fp32 group_norm + SiLU, rounded once,
    passes the statistic — with at most half of the fp32 part, and not vacuously."""
    nb, S, C1, C2 = shape
    gamma, beta = nc.affine(C1 + C2)
    used, worst = {}, 0.0
    for fam in nc.gn_families(shape):
        x = nc.family(fam, nb, S, C1 + C2)
        try:
            nc.family_property(fam, x, nb, S)
        except AssertionError as e:
            raise AssertionError(f"{fam} {shape}: {e}") from e
        used[fam], w = _torch_inside(x, nb, S, nc.GROUPS, gamma, beta, True, (fam, shape))
        worst = max(worst, w)
    print(f"torch fp32 group_norm {shape}: fp32 part used " + " ".join(f"{k}={v:.2f}" for k, v in used.items()) + f"; worst/bound {worst:.3f}")
    assert worst > 0.1


def test_layernorm_families_and_torch_fp32_inside_the_bound():
    n, worst, used = 0, 0.0, 0.0
    for M, d, _, fams in nc.ln_cases():
        gamma, beta = nc.affine(d)
        for fam in fams:
            x = nc.ln_family(fam, M, d)
            try:
                nc.family_property(fam, x, M, 1, groups=1)
            except AssertionError as e:
                raise AssertionError(f"{fam} M={M} d={d}: {e}") from e
            w32, w = _torch_inside(x, M, 1, 1, gamma, beta, False, (fam, M, d))
            used, worst, n = max(used, w32), max(worst, w), n + 1
    print(f"torch fp32 layer_norm over {n} (family, shape): fp32 part used {used:.2f}; worst/bound {worst:.3f}")
    assert n > 300 and worst > 0.1


def test_a_degenerate_family_is_noticed():
    """The property checks bite: Gaussian data has none of the properties."""
    x = nc.family("gauss", 2, 615, 1280)
    for fam in nc.FAMILIES[1:]:
        with pytest.raises(AssertionError):
            nc.family_property(fam, x, 2, 615)
    x = nc.ln_family("gauss", 37, 320)
    for fam in nc.LN_FAMILIES[1:]:
        with pytest.raises(AssertionError):
            nc.family_property(fam, x, 37, 1, groups=1)


def test_case_table_reaches_every_path_and_edge():
    """gn_path asks the library's planner; the table hits every algorithm and the edges between them."""
    for path, shapes in nc.GN_SHAPES.items():
        for nb, S, C1, C2 in shapes:
            assert nc.gn_path(nb, S, C1, C2, path.startswith("cs")) == path, (path, nb, S, C1, C2)
            assert nb * S * (C1 + C2) * 4 <= 72e6
    assert (nc.gn_path(2, 614, 1280, 0, False), nc.gn_path(2, 615, 1280, 0, False)) == ("fused", "regs")   # last slice that fits the LDS / first that does not
    assert (2, 33, 640, 320) in nc.GN_SHAPES["fused"] and 640 % (960 // 32) != 0     # group 21 straddles x1 | x2
    assert 128 // 32 == 4                                                            # cpg = 4: one float4 slot per group
    assert (nc.gn_path(2, 1836, 1280, 0, False), nc.gn_path(2, 1837, 1280, 0, False)) == ("regs", "stream")  # last slice that fits the registers / first that does not
    assert any(C2 for _, _, _, C2 in nc.GN_SHAPES["regs"])
    st = nc.GN_SHAPES["stream"]
    assert {-(-(C1 + C2) // 4 // 256) for _, _, C1, C2 in st} == {1, 2, 3}          # float4 slots per thread
    ns, rp, ns0 = nc.gn_nsplit(2, 12000, 320)
    assert (ns, rp) == (512, 24) and ns > ns0 and ns * rp > 12000 + rp               # floor-raised nsplit, short slabs, EMPTY trailing slabs
    ns, rp, ns0 = nc.gn_nsplit(4, 13056, 320)
    assert ns == ns0 == 256 and rp == 51 == 16384 // 320 and 13056 % 51 == 0        # full 51-row slabs, nsplit not raised
    assert nc.gn_path(4, 13056, 320, 0, False) == "stream"
    items = lambda S, C: (S // 64) * (C // 32)                                      # noqa: E731
    assert items(2496, 320) == 390 and items(3328, 1280) == 2080 > 2048 >= items(640, 1280)
    assert any(C2 and S % 64 == 0 and nc.gn_path(nb, S, C1, C2, False) != "fused" for nb, S, C1, C2 in nc.GN_SHAPES["cs256"])   # a slice too big for the LDS
    # after drop_colstats the cs shapes take other paths: all of them held to the same bound
    assert {nc.gn_path(*s, False) for p in ("cs256", "cs1024") for s in nc.GN_SHAPES[p]} == {"regs", "stream"}
    # every path has one shape that takes the raw copies
    for path, shapes in nc.GN_SHAPES.items():
        assert {v[2] for v in nc.gn_variants(path, shapes[0])} == {False, True, "split"}
        assert all(len({(v[0], v[1]) for v in nc.gn_variants(path, s)}) == 4 for s in shapes)
    # LayerNorm: six streaming widths, one off-width per LPR, M around the rows per block, the persistent grid wrapped twice
    lc = nc.ln_cases()
    assert {d for _, d, k, _ in lc if k == "16"} >= set(nc.LN_STREAM_WIDTHS) | set(nc.LN_OFF_WIDTHS)
    assert {nc.ln_lpr(d) for d in nc.LN_OFF_WIDTHS} == {16, 32, 64} and not set(nc.LN_OFF_WIDTHS) & set(nc.LN_STREAM_WIDTHS)
    for d in nc.LN_STREAM_WIDTHS + nc.LN_OFF_WIDTHS:
        rpb = 256 // nc.ln_lpr(d)
        assert {M for M, d2, k, _ in lc if d2 == d and k == "16"} >= {1, rpb - 1, rpb + 1}
    assert {nc.ln_lpr(d) for _, d in nc.LN_WRAP} == {16, 32, 64}
    for M, d in nc.LN_WRAP:
        rpb = 256 // nc.ln_lpr(d)
        assert d in nc.LN_STREAM_WIDTHS and -(-M // rpb) > 2 * 2048 and M % rpb != 0
    assert any(k == "f32" for _, _, k, _ in lc)


# ---- CPU: the models inside the bound, the defects outside -------------------------------------------------------------
MODEL_SHAPES = [(2, 615, 1280, 0), (2, 33, 640, 320)]


def _gn_model_worst(fam, shape, dt, silu, defect=None):
    nb, S, C1, C2 = shape
    x = nc.family(fam, nb, S, C1 + C2)
    gamma, beta = nc.affine(C1 + C2)
    ref = nc.reference(x, nb, S, nc.GROUPS, gamma, beta, nc.EPS, silu)
    out = nc.gn_centred_model(x, nb, S, gamma, beta, nc.EPS, silu, dt, defect=defect, C1=C1)
    return nc.worst_ratio(out, ref.y, nc.bound(ref, dt)), nc.rel_l2(out, ref.y)


def test_gn_centred_model_is_inside_the_bound():
    """Two-pass fp32 statistics by blocked sums + the fp32 apply: the UNROUNDED model uses <= 0.7 of the fp32 part of the bound
    on every family (one rounding to 16 bit alone reaches 1.0 of u |y*| next to a power of two, so the 0.7 can only be asked
    of the part before it), and rounded once to either type it is <= 1."""
    worst = {}
    for fam in nc.FAMILIES:
        for nb, S, C1, C2 in MODEL_SHAPES:
            x = nc.family(fam, nb, S, C1 + C2)
            gamma, beta = nc.affine(C1 + C2)
            for silu in (True, False):
                ref = nc.reference(x, nb, S, nc.GROUPS, gamma, beta, nc.EPS, silu)
                out = nc.gn_centred_model(x, nb, S, gamma, beta, nc.EPS, silu, torch.float32)
                w = nc.worst_ratio(out, ref.y, ref.f32)
                worst[fam] = max(worst.get(fam, 0.0), w)
                assert w <= 0.7, (fam, (nb, S, C1, C2), silu, w)
                for dt in nc.DTS.values():
                    w16 = nc.worst_ratio(out.to(dt), ref.y, nc.bound(ref, dt))
                    assert 0.1 < w16 <= 1 or fam == "const", (fam, dt, w16)
    print("gn_centred_model, fp32 part used: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) > 0.1


def test_ln_model_is_inside_the_bound():
    worst = {}
    for fam in nc.LN_FAMILIES:
        for M, d in ((37, 320), (9, 1280), (5, 768)):
            x = nc.ln_family(fam, M, d)
            gamma, beta = nc.affine(d)
            ref = nc.reference(x, M, 1, 1, gamma, beta, nc.EPS, False)
            out = nc.ln_model(x, gamma, beta, nc.EPS, torch.float32)
            w = nc.worst_ratio(out, ref.y, ref.f32)             # the VGEN_F32 output: the fp32 part is the whole bound
            worst[fam] = max(worst.get(fam, 0.0), w)
            assert w <= 0.7, (fam, M, d, w)
            for dt in nc.DTS.values():
                assert nc.worst_ratio(out.to(dt), ref.y, nc.bound(ref, dt)) <= 1, (fam, M, d, dt)
    print("ln_model, fp32 part used: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) > 0.1


STREAM_SHAPE = (2, 1837, 1280, 0)          # 12-row slabs of 16 K elements
DEFECT_CASES = [("raw_moments", "offset_1000", STREAM_SHAPE), ("no_clamp", "const", (2, 1000, 2560, 0)),
                ("drop_last_row", "edge_outlier", MODEL_SHAPES[0]), ("neighbour_group", "group_scales", MODEL_SHAPES[0]),
                ("batch0_stats", "group_scales", MODEL_SHAPES[0]), ("eps_omitted", "tiny_var", MODEL_SHAPES[0]),
                ("x2_stride_of_x1", "gauss", MODEL_SHAPES[1])]


@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("defect,fam,shape", DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_modelled_defect_is_caught(dtname, defect, fam, shape):
    """Acceptance test of the metric and the families: each modelled mistake pushes the statistic over 1 on the family built
    for it, and the same model without the mistake passes."""
    dt = nc.DTS[dtname]
    ok, _ = _gn_model_worst(fam, shape, dt, True)
    bad, _ = _gn_model_worst(fam, shape, dt, True, defect=defect)
    print(f"{defect} on {fam} {shape} {dtname}: worst {ok:.3f} -> {bad:.3g}")
    assert ok <= 1 < bad, (defect, ok, bad)
    if defect == "raw_moments":            # raw second moments lose (mean / sigma)^2: harmless at 30, outside the bound at 1000
        mild, _ = _gn_model_worst("offset_30", shape, dt, True, defect=defect)
        clamped, _ = _gn_model_worst("const", shape, dt, True, defect=defect)
        print(f"raw_moments on offset_30: {mild:.3f}; on const (clamped): {clamped:.3f}")
        assert mild <= 1 and clamped <= 1
    if defect == "no_clamp":
        assert math.isinf(bad)             # NaN from a negative variance


@pytest.mark.parametrize("dtname", DTN)
def test_ln_row_from_neighbour_is_caught(dtname):
    dt = nc.DTS[dtname]
    x = nc.ln_family("row_scales", 37, 320)
    gamma, beta = nc.affine(320)
    ref = nc.reference(x, 37, 1, 1, gamma, beta, nc.EPS, False)
    ok = nc.worst_ratio(nc.ln_model(x, gamma, beta, nc.EPS, dt), ref.y, nc.bound(ref, dt))
    bad = nc.worst_ratio(nc.ln_model(x, gamma, beta, nc.EPS, dt, defect="ln_row_from_neighbour"), ref.y, nc.bound(ref, dt))
    assert ok <= 1 < bad, (ok, bad)


def test_local_mistakes_pass_the_whole_tensor_rel_l2_on_gaussian_data():
    """Why this file exists: on Gaussian data a statistics pass that drops the last row, or one (batch, group) normalised
    with its neighbour's statistics, stays under the rel-L2 the older GroupNorm tests allow (kernel_cases.TOL16_EMU) while the
    per-element statistic leaves the bound by two orders.  (`neighbour_group` in bf16 only: at fp16's ten times smaller
    rounding the same mistake moves the rel-L2 to 4.5e-4, over the fp16 limit of 3e-4 — there the old metric sees it.)"""
    import kernel_cases as kc
    for defect, dtn in (("drop_last_row", "fp16"), ("drop_last_row", "bf16"), ("neighbour_group", "bf16")):
        good = _gn_model_worst("gauss", STREAM_SHAPE, nc.DTS[dtn], True)
        bad = _gn_model_worst("gauss", STREAM_SHAPE, nc.DTS[dtn], True, defect=defect)
        print(f"{defect} on gauss {dtn}: rel-L2 {good[1]:.3e} -> {bad[1]:.3e} (limit {kc.TOL16_EMU[dtn]:.1e}); worst/bound {good[0]:.3f} -> {bad[0]:.3g}")
        assert good[1] < bad[1] <= kc.TOL16_EMU[dtn] and good[0] <= 1 < bad[0]


def test_emulator_statistics_path_mirrors_the_conditioning_guard():
    """EMU.groupnorm fed by fp32 column sums (the `_cs` branch): with gn_finalize_cs_kernel's guard mirrored it stays inside
    the bound at mean / sigma = 1000, where the sums alone do not carry the variance; where the guard is not taken it is
    the raw-moment result as before."""
    from oracle import abi_emulator as emu
    from vgen_amd.ops import TapGemm, drop_colstats
    EMU = emu.EmuBackend()
    nb, S, Cn, dt = 2, 128, 320, torch.float16
    gamma, beta = nc.affine(Cn)
    g = nc._gen("emu")
    A, W = torch.randn(nb * S, 64, generator=g).to(dt), (torch.randn(Cn, 64, generator=g) / 800).to(dt)
    taken = {}
    for fam in ("gauss", "offset_1000", "tiny_var", "const"):
        x = EMU.tapgemm(TapGemm(A=A, W=W, M=nb * S, N=Cn, C1=64, residual=nc.family(fam, nb, S, Cn), colstats=True))
        assert x.vgen_cs is not None
        ref = nc.reference(x, nb, S, nc.GROUPS, gamma, beta, nc.EPS, True)
        y, _ = EMU.groupnorm(x, None, nb, S, nc.GROUPS, nc.EPS, gamma, beta, True, False, dt)
        assert nc.worst_ratio(y, ref.y, nc.bound(ref, dt)) <= 1, fam
        taken[fam] = bool((ref.mu ** 2 * (ref.rstd ** 2) > emu.GN_CS_GUARD).any())       # mu^2 / (var + eps): a lower bound of N M^2 / Q
        cs = x.vgen_cs
        drop_colstats(x)
        y_plain, _ = EMU.groupnorm(x, None, nb, S, nc.GROUPS, nc.EPS, gamma, beta, True, False, dt)
        if fam == "gauss":          # guard not taken: the statistics path as it was, a rounding or two from the plain path
            assert float((y.float() - y_plain.float()).abs().max()) <= 2 * 2.0 ** -10 * float(y_plain.float().abs().max())
        x.vgen_cs = cs
    assert taken == {"gauss": False, "offset_1000": True, "tiny_var": True, "const": True}


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32], ids=str)
def test_guard_row_harness_reports_a_stray_store(dt):
    x = nc.family("gauss", 1, 7, 64)
    fr = nc.nan_framed(x)
    assert bool(torch.isnan(fr[:nc.GUARD]).all()) and bool(torch.isnan(fr[-nc.GUARD:]).all()) and torch.equal(fr[nc.GUARD:-nc.GUARD], x)
    s = nc.sentinel(7 + 2 * nc.GUARD, 64, dt)
    assert bool(torch.isfinite(s.float()).all()) and len(nc.bits(s).unique()) > 50
    after = s.clone()
    after[nc.GUARD:-nc.GUARD] = 0                                 # an honest kernel: live rows only
    assert not nc.guard_violations(s, after)
    for at in (0, (nc.GUARD - 1) * 64 + 63, (nc.GUARD + 7) * 64, s.numel() - 1):
        b2 = after.clone()
        nc.bits(b2).view(-1)[at] ^= 1
        assert nc.guard_violations(s, b2) == [at]


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _record(key, val):
    from test_gpu_model import _record as rec
    rec(key, val)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _gn_call(be, x1, x2, cs1, cs2, nb, S, gamma, beta, silu, raw, dt):
    """One vgen_groupnorm[_cs] through the C ABI into sentinel-framed outputs; returns (y frame, raw frame, the pristine
    sentinels of both) on the CPU."""
    from vgen_amd import lib as L
    from vgen_amd.ops import _ENUM
    rows, Cn = nb * S, x1.shape[1] + (x2.shape[1] if x2 is not None else 0)
    y0 = nc.sentinel(rows + 2 * nc.GUARD, Cn, dt)
    r0 = nc.sentinel(rows + 2 * nc.GUARD, Cn * (2 if raw == "split" else 1), dt) if raw else None
    yd, rd = y0.to(DEV), (r0.to(DEV) if raw else None)
    nbytes = be.lib.vgen_groupnorm_ws_bytes(nb, S)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
    C1, C2 = x1.shape[1], (x2.shape[1] if x2 is not None else 0)
    tail = (_p(gamma), _p(beta), int(silu), _p(yd[nc.GUARD:]), _p(rd[nc.GUARD:]) if raw else None, int(raw == "split"), _ENUM[dt],
            _p(ws), nbytes, _stream())
    if cs1 is not None:
        rc = be.lib.vgen_groupnorm_cs(_p(x1), C1, _p(cs1), _p(x2), C2, _p(cs2), nb, S, nc.GROUPS, nc.EPS, *tail)
    else:
        rc = be.lib.vgen_groupnorm(_p(x1), C1, _p(x2), C2, nb, S, nc.GROUPS, nc.EPS, *tail)
    L.check(rc, "vgen_groupnorm")
    torch.cuda.synchronize()
    return yd.cpu(), (rd.cpu() if raw else None), y0, r0


def _framed_dev(x):
    """x inside NaN guard rows on the device; the live rows as a contiguous slice."""
    fr = nc.nan_framed(x).to(DEV)
    return fr, fr[nc.GUARD:-nc.GUARD]


def _gemm_through(be, res, nb, S, dt, seed):
    """x = A W^T + res from a real tap-GEMM with column statistics, written into NaN-framed rows: W is scaled per output
    column so that the product adds ~1 % of the column's own spread (0 for a constant column)."""
    from vgen_amd.ops import TapGemm
    M, N = res.shape
    g = nc._gen("gemm", M, N, seed)
    sig = res.view(nb, S, N)[:, 1:-1].double().std(1, unbiased=False).amin(0).float()     # without the rows `edge_outlier` plants
    A = torch.randn(M, 64, generator=g).to(dt)
    W = (torch.randn(N, 64, generator=g) / 8 * (0.01 * sig).view(N, 1)).to(dt)
    fr = torch.full((M + 2 * nc.GUARD, N), float("nan"), device=DEV)
    out = be.tapgemm(TapGemm(A=A.to(DEV), W=W.to(DEV), M=M, N=N, C1=64, residual=res.to(DEV), out=fr[nc.GUARD:-nc.GUARD], colstats=True))
    torch.cuda.synchronize()
    assert getattr(out, "vgen_cs", None) is not None, "the tap-GEMM attached no column statistics"
    assert bool(torch.isnan(fr[:nc.GUARD]).all()) and bool(torch.isnan(fr[-nc.GUARD:]).all())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("path,shape,fam", nc.gn_cases(), ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_groupnorm_per_element_on_device(hip_backend, path, shape, fam):
    """One (path, shape, family): every launch variant (both dtypes, SiLU on / off, raw copies on the first shape of the path)
    within the bound per element against the fp64 reference of the tensor the kernel read; outputs finite although the
    input is framed by NaN rows; sentinel rows around y and raw untouched; the raw copies exact.  The cs paths read x from a
    real tap-GEMM with column statistics, and run the same device tensor through the plain path as well."""
    from vgen_amd.ops import colstats_of, drop_colstats
    nb, S, C1, C2 = shape
    Cn, rows = C1 + C2, nb * S
    x = nc.family(fam, nb, S, Cn)
    gamma, beta = nc.affine(Cn)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    is_cs = path.startswith("cs")
    refs, fails, worst = {}, [], {}
    for dtname, silu, raw in nc.gn_variants(path, shape):
        dt = nc.DTS[dtname]
        if is_cs:       # the producer runs in the launch's 16-bit type: one x (and one reference) per dtype
            x1 = _gemm_through(hip_backend, x[:, :C1].contiguous(), nb, S, dt, 1)
            x2 = _gemm_through(hip_backend, x[:, C1:].contiguous(), nb, S, dt, 2) if C2 else None
            xr = torch.cat([x1.cpu()] + ([x2.cpu()] if C2 else []), 1)
            nc.family_property(fam, xr, nb, S)
            key = (dtname, silu)
        else:
            _, x1 = _framed_dev(x[:, :C1].contiguous())
            _, x2 = _framed_dev(x[:, C1:].contiguous()) if C2 else (None, None)
            xr, key = x, silu
        if key not in refs:
            refs[key] = nc.reference(xr, nb, S, nc.GROUPS, gamma, beta, nc.EPS, silu)
        ref = refs[key]
        bnd = nc.bound(ref, dt)
        runs = [(path, colstats_of(x1, rows), colstats_of(x2, rows) if C2 else None)] if is_cs else [(path, None, None)]
        if is_cs:
            assert runs[0][1] is not None and (not C2 or runs[0][2] is not None)
            runs.append((nc.gn_path(nb, S, C1, C2, False), None, None))
        for p, cs1, cs2 in runs:
            if cs1 is None:
                drop_colstats(x1)
                if x2 is not None:
                    drop_colstats(x2)
            yf, rf, y0, r0 = _gn_call(hip_backend, x1, x2, cs1, cs2, nb, S, gd, bd, silu, raw, dt)
            tag = f"{p} {shape} {fam} {dtname} silu={silu} raw={raw}"
            y = yf[nc.GUARD:-nc.GUARD]
            w = nc.worst_ratio(y, ref.y, bnd)
            worst[(p, dtname)] = max(worst.get((p, dtname), 0.0), w)
            if not w <= 1:
                fails.append(f"{tag}: worst/bound {w:.3g}\n" + nc.offenders(y, ref.y, bnd, nb, S, nc.GROUPS))
            if fam == "const":          # sigma^2 = 0 exactly: finite, act(beta) within the bound (checked above), every row alike
                if not bool((nc.bits(y) == nc.bits(y[:1])).all()):
                    fails.append(f"{tag}: rows of a constant input differ")
            if nc.guard_violations(y0, yf):
                fails.append(f"{tag}: sentinel rows of y written at {nc.guard_violations(y0, yf)[:10]}")
            if raw:
                if nc.guard_violations(r0, rf):
                    fails.append(f"{tag}: sentinel rows of raw written at {nc.guard_violations(r0, rf)[:10]}")
                hi = xr.to(dt)
                want = torch.cat([hi, (xr - hi.float()).to(dt)], 1) if raw == "split" else hi
                if not torch.equal(nc.bits(rf[nc.GUARD:-nc.GUARD]), nc.bits(want)):
                    fails.append(f"{tag}: raw copy differs in {int((nc.bits(rf[nc.GUARD:-nc.GUARD]) != nc.bits(want)).sum())} elements")
    for (p, dtname), w in worst.items():
        print(f"norm_edges/gn/{p}/{_sid(shape)}/{fam}/{dtname}: worst/bound {w:.3f}")
        _record(f"norm_edges/gn/{p}/{_sid(shape)}/{fam}/{dtname}", round(w, 4))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("M,d,kind", [c[:3] for c in nc.ln_cases()], ids=lambda v: str(v))
def test_layernorm_per_element_on_device(hip_backend, M, d, kind):
    """One (M, d): every family, both 16-bit types (or the VGEN_F32 output), per element against fp64; NaN rows around the
    input, sentinel rows around the output."""
    from vgen_amd import lib as L
    from vgen_amd.ops import _ENUM
    fams = next(c[3] for c in nc.ln_cases() if c[:3] == (M, d, kind))
    gamma, beta = nc.affine(d)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    fails, worst = [], {}
    for fam in fams:
        x = nc.ln_family(fam, M, d)
        ref = nc.reference(x, M, 1, 1, gamma, beta, nc.EPS, False)
        _, xd = _framed_dev(x)
        for dt in ([torch.float32] if kind == "f32" else list(nc.DTS.values())):
            y0 = nc.sentinel(M + 2 * nc.GUARD, d, dt)
            yd = y0.to(DEV)
            rc = hip_backend.lib.vgen_layernorm(_p(xd), M, d, nc.EPS, _p(gd), _p(bd), _p(yd[nc.GUARD:]), _ENUM[dt], _stream())
            L.check(rc, "vgen_layernorm")
            torch.cuda.synchronize()
            yf = yd.cpu()
            y = yf[nc.GUARD:-nc.GUARD]
            bnd = nc.bound(ref, dt)
            w = nc.worst_ratio(y, ref.y, bnd)
            worst[str(dt)] = max(worst.get(str(dt), 0.0), w)
            if not w <= 1:
                fails.append(f"M={M} d={d} {fam} {dt}: worst/bound {w:.3g}\n" + nc.offenders(y, ref.y, bnd, M, 1, 1))
            if nc.guard_violations(y0, yf):
                fails.append(f"M={M} d={d} {fam} {dt}: sentinel rows written at {nc.guard_violations(y0, yf)[:10]}")
    for k, w in worst.items():
        print(f"norm_edges/ln/{M}x{d}/{kind}/{k}: worst/bound {w:.3f}")
        _record(f"norm_edges/ln/{M}x{d}/{kind}/{k}", round(w, 4))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTN)
def test_groupnorm_cs_without_the_guard_keeps_the_parent_bits(hip_backend, dtname):
    """Where gn_finalize_cs_kernel's conditioning guard is not taken (every kernel_cases.GN_CS_CASES input: N M^2 / Q < 1) the
    output is the one the kernel gave before the guard existed, bit for bit: sha-256 of y against the values recorded with
    the parent commit's library (tests/golden/groupnorm_cs_parent_sha256.json)."""
    import hashlib
    import json
    import kernel_cases as kc
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_cs_parent_sha256.json")))["sha256"]
    dt = kc.DTS[dtname]
    for nb, S, C1, C2, silu in kc.GN_CS_CASES:
        g1 = kc.make_tapgemm(dt, nb * S, C1, 64, residual=True, colstats=True, seed=0)
        g2 = kc.make_tapgemm(dt, nb * S, C2, 128, colstats=True, seed=1) if C2 else None
        gen = kc._g(2)
        gamma = 1 + 0.2 * torch.randn(C1 + C2, generator=gen)
        beta = 0.3 * torch.randn(C1 + C2, generator=gen)
        x1 = hip_backend.tapgemm(kc._clone_spec(g1, DEV))
        x2 = hip_backend.tapgemm(kc._clone_spec(g2, DEV)) if g2 else None
        assert getattr(x1, "vgen_cs", None) is not None
        y, _ = hip_backend.groupnorm(x1, x2, nb, S, 32, 1e-5, gamma.to(DEV), beta.to(DEV), silu, False, dt)
        torch.cuda.synchronize()
        got = hashlib.sha256(y.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
        assert got == want[f"{dtname}/{nb}x{S}x{C1}+{C2}"], (dtname, nb, S, C1, C2)
