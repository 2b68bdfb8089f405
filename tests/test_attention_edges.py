"""Attention kernels (flash_kernel, its causal mask, temporal_kernel, flash_d80_kernel) and vgen_softmax_rows on adversarial
inputs: per-ELEMENT parity with an fp64 reference of the same 16-bit operands, under the bound derived in
tests/attn_cases.py (3 u P|v| + the fp16 subnormal term; never tuned to what a GPU gives), plus what a launch reads and
writes beyond its operands (guard rows / columns with sentinels, NaN / Inf padding).

CPU tests (unmarked): every input family has the property it is meant to have; the CPU model of the kernels' arithmetic
stays inside the bound; six modelled kernel mistakes are each CAUGHT by the statistic (and one of them is shown to pass
the whole-tensor rel-L2 the older tests use); the guard-band harness reports a stray store.  GPU tests: the real kernels.

Measured on one MI355X (worst = max |err| / bound over all shapes of the family; rel-L2 for comparison with the older
whole-tensor tests): see DESIGN.md section 3.2 for the table."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402

DEV = "cuda:0"
DTN = ["fp16", "bf16"]


# ---- CPU: families -------------------------------------------------------------------------------------------------
def _family_shapes():
    """Every (family, nq, nk, D, causal) the GPU tests use, once."""
    seen = set()
    for kernel, (D, causal, _) in ac.KERNELS.items():
        for fam in ac.FAMILIES:
            for _, _, nq, nk, _, _ in ac.shapes_for(kernel, fam):
                seen.add((fam, nq, nk, D, causal))
    return sorted(seen)


@pytest.mark.parametrize("dtname", DTN)
def test_families_have_their_property_at_every_shape_used(dtname):
    dt = ac.DTS[dtname]
    n = 0
    for fam, nq, nk, D, causal in _family_shapes():
        for seed in (0, (0, 1, 0, 2)):
            q, k, v = ac.family(fam, nq, nk, D, dt, seed, causal)
            try:
                ac.family_property(fam, q, k, v, D, seed, causal)
            except AssertionError as e:
                raise AssertionError(f"{fam} nq={nq} nk={nk} D={D} causal={causal} seed={seed}: {e}") from e
            n += 1
    assert n > 400
    for fam in ac.TILE_ORDER:                                    # the tile-order families only run where a second tile exists
        assert all(s[3] > ac.BKV for kern in ac.KERNELS for s in ac.shapes_for(kern, fam))
    for kern in ac.KERNELS:
        assert len(ac.shapes_for(kern, "v_outlier")) == 3 and len(ac.shapes_for(kern, "gauss")) == len(ac.KERNELS[kern][2])
    assert len({(s[2], s[3]) for s in ac.TEMPORAL_SHAPES}) == 25 and {s[4] * s[1] for s in ac.TEMPORAL_SHAPES} == {1, 5, 8}


def test_a_degenerate_family_is_noticed():
    """The property checks bite: Gaussian operands have none of the properties."""
    q, k, v = ac.family("gauss", 130, 257, 64, torch.float16)
    for fam in ("late_max", "late_half", "ascending", "descending", "all_negative", "flat", "onehot", "v_outlier"):
        with pytest.raises(AssertionError):
            ac.family_property(fam, q, k, v, 64)


# ---- CPU: the model inside the bound, the defects outside --------------------------------------------------------------
MODEL_SHAPES = [(130, 257, False), (33, 77, False), (200, 200, True)]


def _model_worst(fam, nq, nk, D, dt, causal, defect=None, model=None):
    q, k, v = ac.family(fam, nq, nk, D, dt, 0, causal)
    O, A = ac.reference(q, k, v, ac.head_scale(D), causal)
    bnd = ac.bound(A, v, dt)
    out = (model or ac.flash_model)(q, k, v, ac.head_scale(D), dt, **({} if model else dict(causal=causal, defect=defect)))
    return ac.worst_ratio(out, O, bnd), ac.worst_ratio(O.to(dt), O, bnd)


@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("D", [64, 80])
def test_flash_model_is_inside_the_bound(dtname, D):
    """The kernels' arithmetic, modelled on the CPU, has nearly 2 x room under the bound for every family; the fp64
    reference merely rounded to 16 bit needs a third of it (the bound is not loose either)."""
    dt = ac.DTS[dtname]
    worst = {}
    for fam in ac.FAMILIES:
        for nq, nk, causal in MODEL_SHAPES:
            if causal and (D == 80 or fam in ("flat", "late_max", "late_half", "descending")):
                continue
            w, w0 = _model_worst(fam, nq, nk, D, dt, causal)
            worst[fam] = max(worst.get(fam, 0.0), w)
            assert w <= 0.7 and w0 <= 0.34, (fam, nq, nk, causal, w, w0)
    print(f"flash_model worst/bound {dtname} d{D}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) > 0.1                              # ... and the statistic is not vacuous


@pytest.mark.parametrize("dtname", DTN)
def test_temporal_model_is_inside_the_bound(dtname):
    dt = ac.DTS[dtname]
    for fam in ("gauss", "onehot", "all_negative", "flat"):
        for nq, nk in ((3, 15), (16, 16), (1, 4), (15, 1)):
            w, _ = _model_worst(fam, nq, nk, 64, dt, False, model=ac.temporal_model)
            assert w <= 0.7, (fam, nq, nk, w)


DEFECT_CASES = [("ragged_mask", "all_negative", 33, 77, False), ("causal_mask", "ascending", 200, 200, True),
                ("no_acc_rescale", "late_half", 130, 257, False), ("no_sum_rescale", "ascending", 130, 257, False),
                ("swap_keys", "onehot", 130, 257, False), ("row_from_neighbour", "gauss", 130, 257, False)]


@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("defect,fam,nq,nk,causal", DEFECT_CASES)
def test_modelled_defect_is_caught(dtname, defect, fam, nq, nk, causal):
    """Acceptance test of the metric and the families: each modelled mistake pushes the statistic over 1 on the family
    built for it, for head_dim 64 and 80, and the same model without the mistake passes."""
    dt = ac.DTS[dtname]
    for D in (64, 80):
        ok, _ = _model_worst(fam, nq, nk, D, dt, causal)
        bad, _ = _model_worst(fam, nq, nk, D, dt, causal, defect=defect)
        print(f"{defect} on {fam} d{D} {dtname}: worst {ok:.3f} -> {bad:.3g}")
        assert ok <= 1 < bad, (defect, D, ok, bad)


def test_one_wrong_row_passes_the_whole_tensor_rel_l2_but_not_the_bound():
    """Why this file exists: on the image tower's 5 x 16 heads x 257 x 257 (bf16), ONE (batch, head, row) returned from its
    neighbour moves the whole-tensor rel-L2 to about 1.0e-2 — under the 3 x TOL16 = 1.2e-2 the older d80 test allows."""
    import kernel_cases as kc
    dt = torch.bfloat16
    g = torch.Generator("cpu").manual_seed(7)
    q = (torch.randn(5, 16, 257, 80, generator=g) * 1.5).to(dt)
    k = (torch.randn(5, 16, 257, 80, generator=g) * 1.5).to(dt)
    v = torch.randn(5, 16, 257, 80, generator=g).to(dt)
    O, A = ac.reference(q, k, v, 80 ** -0.5)
    bnd = ac.bound(A, v, dt)
    out = torch.stack([torch.stack([ac.flash_model(q[b, h], k[b, h], v[b, h], 80 ** -0.5, dt) for h in range(16)]) for b in range(5)])
    good = ac.rel_l2(out, O), ac.worst_ratio(out, O, bnd)
    out[3, 11, 256] = out[3, 11, 255]                             # row 256: the only live row of its query tile
    bad = ac.rel_l2(out, O), ac.worst_ratio(out, O, bnd)
    print(f"rel-L2 {good[0]:.3e} -> {bad[0]:.3e} (limit {3 * kc.TOL16['bf16']:.1e}); worst/bound {good[1]:.3f} -> {bad[1]:.3g}")
    assert good[0] < bad[0] <= 3 * kc.TOL16["bf16"] and bad[0] > 8e-3
    assert good[1] <= 1 < bad[1]


# ---- CPU: the cases and the harness ----------------------------------------------------------------------------------
def test_case_addressing_round_trips():
    """The strided reference reads what fill_family wrote, in every layout (cross shares K / V among `inner` sequences)."""
    for kernel, shape in (("flash", ac.FLASH_SHAPES[4]), ("flash", ac.FLASH_SHAPES[5]), ("flash", ac.FLASH_SHAPES[9]),
                          ("temporal", ac.TEMPORAL_SHAPES[2]), ("d80", ac.D80_SHAPES[3])):
        c = ac.build(kernel, shape, torch.float16, "gauss")
        layout, heads, nq, nk, nbatch, inner = shape
        q, k, v = c.operand("q"), c.operand("k"), c.operand("v")
        assert q.shape == (nbatch, heads, nq, c.D) and k.shape == (nbatch, heads, nk, c.D)
        b, h = nbatch - 1, heads - 1
        shared = c.ops["k"][2][2] == 0
        q0, k0, v0 = ac.family("gauss", nq, nk, c.D, c.dt, (0, b // inner, 0 if shared else b % inner, h))
        assert torch.equal(k[b, h], k0) and torch.equal(v[b, h], v0)
        assert torch.equal(q[b, h], q0.roll(b % inner, 0) if shared else q0)
        bufs = {n: t.clone() for n, t in c.bufs.items()}
        ac.torch_kernel(c, bufs)
        O, bnd = ac.case_reference(c)
        assert ac.worst_ratio(c.operand("out", bufs), O, bnd) <= 0.34
        assert not ac.footprint_violations(c.bufs["out"], bufs["out"], c.live_mask("out"))


@pytest.mark.parametrize("dtname", DTN)
def test_guard_band_harness_reports_a_stray_store(dtname):
    dt = ac.DTS[dtname]
    c = ac.fill_family(ac.make_case("banded", 80, 3, 129, 64, 2, dt, pad=float("nan")), "gauss")
    live = c.live_mask("out")
    assert int(live.sum()) == 2 * 3 * 129 * 80 and live.numel() == 2 * (129 + 16) * (240 + 8)
    assert bool(torch.isfinite(c.bufs["out"].float()).all())     # the sentinel is a finite pattern, compared by bits
    assert bool(torch.isnan(c.bufs["k"].float()[~c.live_mask("k")]).all()) and bool(torch.isfinite(c.operand("k").float()).all())
    bufs = {n: t.clone() for n, t in c.bufs.items()}
    ac.torch_kernel(c, bufs)                                      # an honest 'kernel': nothing outside the live elements
    assert not ac.footprint_violations(c.bufs["out"], bufs["out"], live)
    rs, slot = c.ops["out"][2][0], c.ops["out"][2][1]
    strays = {"row nq of sequence 0": c.ops["out"][1] + 129 * rs, "column gap of row 0": c.ops["out"][1] + 240,
              "guard row before sequence 1": slot + 7 * rs + 5}
    for what, at in strays.items():
        b2 = bufs["out"].clone()
        b2.view(torch.int16)[at] ^= 1                             # one bit of one guard element
        assert ac.footprint_violations(c.bufs["out"], b2, live) == [at], what


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _launch(be, case, bufs_cpu=None):
    """One launch of a case on the device; returns its buffers copied back."""
    from vgen_amd.ops import Attn
    bufs = {n: t.to(DEV) for n, t in (bufs_cpu or case.bufs).items()}
    t = {n: bufs[b][off:] for n, (b, off, _) in case.ops.items()}
    g = Attn(q=t["q"], k=t["k"], v=t["v"], out=t["out"], heads=case.heads, nq=case.nq, nk=case.nk, nbatch=case.nbatch,
             inner=case.inner, q_s=case.ops["q"][2], k_s=case.ops["k"][2], v_s=case.ops["v"][2], o_s=case.ops["out"][2],
             scale=case.scale, causal=case.causal)
    (be.attention_d80 if case.D == 80 else be.attention)(g)
    torch.cuda.synchronize()
    return {n: b.cpu() for n, b in bufs.items()}


def _record(key, val):
    from test_gpu_model import _record as rec
    rec(key, val)


def _check(kernel, case, shape, out, O, bnd, fails):
    w = ac.worst_ratio(out, O, bnd)
    if not w <= 1:
        fails.append(f"{kernel} {shape}: worst/bound {w:.3g}\n" + ac.offenders(out, O, bnd))
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("kernel,fam", [(k, f) for k in ac.KERNELS for f in ac.FAMILIES if ac.shapes_for(k, f)])
def test_attention_per_element_on_device(hip_backend, kernel, fam, dtname):
    """Every shape of the (kernel, family): |out - O| <= bound per element against the fp64 reference (computed once per
    case), outputs finite, two launches bit-identical, nothing outside the live output elements written."""
    dt = ac.DTS[dtname]
    shapes = ac.shapes_for(kernel, fam)
    worst, l2, fails = 0.0, 0.0, []
    for shape in shapes:
        case = ac.build(kernel, shape, dt, fam)
        O, bnd = ac.case_reference(case)
        a, b = _launch(hip_backend, case), _launch(hip_backend, case)
        out = case.operand("out", a)
        w = _check(kernel, case, shape, out, O, bnd, fails)
        worst, l2 = max(worst, w), max(l2, ac.rel_l2(out, O))
        if not torch.equal(a["out"].view(torch.int16), b["out"].view(torch.int16)):
            fails.append(f"{kernel} {shape}: two launches differ")
        stray = ac.footprint_violations(case.bufs["out"], a["out"], case.live_mask("out"))
        if stray:
            fails.append(f"{kernel} {shape}: {len(stray)} elements outside the output written, first {stray[:20]}")
        if kernel == "causal":                                    # row 0 sees one key: v[0] to one rounding (exactly, here)
            v0 = case.operand("v")[:, :, 0]
            if not bool(((out[:, :, 0].double() - v0.double()).abs() <= ac.U[dt] * v0.double().abs()).all()):
                fails.append(f"{kernel} {shape}: causal row 0 is not v[0]")
        if case.nq == 257:                                        # row 256: alone in its query tile; row 0: the CLS row
            for r in (256, 0):
                wr = ac.worst_ratio(out[:, :, r], O[:, :, r], bnd[:, :, r])
                print(f"{kernel}/{dtname}/{fam} {shape} row {r}: worst/bound {wr:.3f}")
                if not wr <= 1:
                    fails.append(f"{kernel} {shape}: row {r} worst/bound {wr:.3g}")
    print(f"attn_edges/{kernel}/{dtname}/{fam}: worst/bound {worst:.3f} rel-L2 {l2:.3e} over {len(shapes)} shapes")
    _record(f"attn_edges/{kernel}/{dtname}/{fam}", {"worst": round(worst, 4), "rel_l2": float(f"{l2:.3e}"), "shapes": len(shapes)})
    assert not fails, "\n".join(fails)


FOOTPRINT = [("flash", 64, 3, 33, 77, False), ("causal", 64, 3, 12, 12, True), ("temporal", 64, 1, 3, 15, False),
             ("d80", 80, 3, 129, 64, False), ("d80", 80, 16, 257, 257, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("kernel,D,heads,nq,nk,causal", FOOTPRINT)
def test_attention_footprint_on_device(hip_backend, kernel, D, heads, nq, nk, causal, dtname):
    """Guard rows before / after every sequence and a column gap after the live columns, all inside one allocation per
    operand: the output outside its nq x heads x head_dim live elements keeps its sentinel bits, and NaN or +Inf in the
    inputs' padding (rows >= nq / nk, the column gap) gives the same bits as zero padding."""
    dt = ac.DTS[dtname]
    nbatch = 5 if kernel == "temporal" else 2                     # temporal: 5 pairs, the second block partly idle
    outs = {}
    for pad in (0.0, float("nan"), float("inf")):
        case = ac.fill_family(ac.make_case("banded", D, heads, nq, nk, nbatch, dt, causal=causal, pad=pad), "gauss")
        got = _launch(hip_backend, case)
        stray = ac.footprint_violations(case.bufs["out"], got["out"], case.live_mask("out"))
        assert not stray, f"pad {pad}: {len(stray)} guard elements written, first {stray[:20]} (row stride {case.ops['out'][2][0]})"
        for n in ("q", "k", "v"):
            assert torch.equal(got[n].view(torch.int16), case.bufs[n].view(torch.int16)), f"input {n} modified"
        outs[pad] = case.operand("out", got)
        if pad == 0.0:
            O, bnd = ac.case_reference(case)
            fails = []
            _check(kernel, case, (nq, nk), outs[pad], O, bnd, fails)
            assert not fails, "\n".join(fails)
    zero = outs.pop(0.0)
    for pad, o in outs.items():
        diff = (o.view(torch.int16) != zero.view(torch.int16))
        assert not bool(diff.any()), f"padding {pad} reaches the output: {int(diff.sum())} elements, first {diff.nonzero()[:10].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("kind", ac.SOFTMAX_KINDS)
def test_softmax_rows_per_element_on_device(hip_backend, kind, dtname):
    """vgen_softmax_rows against fp64 softmax(S * scale): per element 2 u P + 2^-25, row sums within 2 u + cols * 2^-25
    of 1; cols below / at / above the 256-thread stride and at 4096 (the VAE's 64 x 64 latent)."""
    dt = ac.DTS[dtname]
    worst, fails = 0.0, []
    for rows in ac.SOFTMAX_ROWS:
        for cols in ac.SOFTMAX_COLS:
            S = ac.softmax_input(kind, rows, cols)
            scale = 0.37 if kind == "gauss" else 1.0
            P, bnd = ac.softmax_reference(S, scale, dt)
            got = hip_backend.softmax_rows(S.to(DEV), cols, scale, dt).cpu().double()
            torch.cuda.synchronize()
            w = ac.worst_ratio(got, P, bnd)
            worst = max(worst, w)
            if not w <= 1:
                fails.append(f"{kind} {rows} x {cols}: worst/bound {w:.3g}\n" + ac.offenders(got, P, bnd))
            sums = (got.sum(1) - 1).abs().max()
            if not float(sums) <= 2 * ac.U[dt] + cols * 2.0 ** -25:
                fails.append(f"{kind} {rows} x {cols}: row sum off by {float(sums):.3g}")
    print(f"attn_edges/softmax_rows/{dtname}/{kind}: worst/bound {worst:.3f}")
    _record(f"attn_edges/softmax_rows/{dtname}/{kind}", {"worst": round(worst, 4)})
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dtname", DTN)
@pytest.mark.parametrize("cols", [200, 257])
def test_softmax_rows_footprint_on_device(hip_backend, cols, dtname):
    """lds > cols with NaN / +Inf in the gap of S, ldp > cols with sentinels in the gap of P."""
    dt = ac.DTS[dtname]
    rows, lds, ldp = 70, cols + 3, cols + 55
    S = ac.softmax_input("gauss", rows, cols)
    outs = []
    for pad in (0.0, float("nan"), float("inf")):
        base = torch.full((rows + 2, lds), pad)
        base[1:-1, :cols] = S
        Pb = ac.sentinel((rows + 2) * ldp, dt).view(rows + 2, ldp)
        Pd = Pb.to(DEV)
        hip_backend.softmax_rows(base.to(DEV)[1:-1, :cols], cols, 0.37, dt, out=Pd[1:-1, :cols])
        torch.cuda.synchronize()
        live = torch.zeros(rows + 2, ldp, dtype=torch.bool)
        live[1:-1, :cols] = True
        stray = ac.footprint_violations(Pb.flatten(), Pd.cpu().flatten(), live.flatten())
        assert not stray, f"pad {pad}: {len(stray)} elements outside P written, first {stray[:20]}"
        outs.append(Pd.cpu()[1:-1, :cols].clone())
    P, bnd = ac.softmax_reference(S, 0.37, dt)
    assert ac.worst_ratio(outs[0].double(), P, bnd) <= 1
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
