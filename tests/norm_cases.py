"""Ill-conditioned GroupNorm / LayerNorm cases: input families, the fp64 reference, a DERIVED per-element bound, CPU models
of the kernels' arithmetic (with switchable modelled defects), the case table that reaches every dispatch path of
csrc/norms.hip, and a guard-row harness.  Pure torch on the CPU; shared by tests/test_norm_edges.py (CPU and GPU tests).

Reference, in float64 from the fp32 tensor the kernel actually read (mu, var exact over the group / the row):

    rstd = (var + eps)^-1/2,   z = gamma (x - mu) rstd + beta,   y* = act(z),   A = (|x| + |mu|) rstd |gamma|

Bound per output element, e = 2^-24 (half an ulp of fp32), u = 2^-11 (fp16) / 2^-8 (bf16):

    |y - y*|  <=  u |y*|  +  2^-25 (fp16 only)  +  C_SUM e L (A + |z - beta| + |beta|)  +  C_ACT e |y*|  (SiLU only)

u |y*| is the one rounding of the output, 2^-25 half the spacing of fp16 subnormals; the VGEN_F32 LayerNorm output has
neither.  L is the Lipschitz constant of the activation (1.1 for SiLU, whose slope peaks at 1.0998).  The fp32 part,
counted in half-ulps of the quantity each rounding acts on:

  * the evaluation x * scale + shift with scale = gamma rstd, shift = beta - mu scale: one rounding each for the two
    products, for scale, for shift and for the final sum: <= 2 |x scale| + 3 |mu scale| + 2 |beta| + |z - beta|
    <= 3 (A + |z - beta| + |beta|);
  * rstd: 1 / sqrt(var + eps) is two roundings, and half the relative error of var, which is a centred sum of squares
    (3 roundings per term) reduced by a BLOCKED fp32 sum: per-thread chains of at most 51 terms (gn_stats), 36 (gn_regs)
    or 48 (gn_fused), then at most 6 butterfly + 4 wave + 10 Chan-merge levels = 71 roundings deep at the very worst.
    Roundings of a sum are independent and centred: sqrt(71) = 8.4 half-ulps, so rstd carries (3 + 8.4) / 2 + 2 = 7.7,
    which acts on |z - beta|;
  * mu: the same blocked sum, 8.4 half-ulps of mean |x| <= |mu| + sigma, acting through scale: <= 8.4 (A / 2 + |z - beta|
    in the mean); the A term already holds 3 of its 8.4 above.

  C_SUM = 12 covers 3 + 7.7 on |z - beta| and 3 + 8.4 / 2 on A.  SiLU (common.h silu_f: x * rcp(1 + exp2(-log2(e) x)))
  is a constant product (1), v_exp_f32 (1 ulp = 2), a sum (1), v_rcp_f32 (1 ulp = 2) and a product (1): C_ACT = 8 with the
  rounding of the argument, amplified by |x| (1 - sigmoid(x)) <= 0.28 for the x > 0 that are not already tiny in y.

torch's own fp32 group_norm + SiLU uses 0.1 - 0.33 of this fp32 part (asserted <= 0.5 in test_norm_edges.py), so the
constants are neither tight on a correct fp32 algorithm nor loose by an order.  They hardly matter: u >= 8192 e, the fp32 part
counts only where A >~ 10^3.  What matters is what the bound does NOT contain: a (mu / sigma)^2 growth of the rstd error.  A
centred fp32 variance does not have one; raw second moments sum x^2 - (sum x)^2 / n do (model `raw_moments` below: outside
the bound at mu / sigma = 1000, inside at 30).  The statistic is worst = max |err| / bound; a test asserts worst <= 1.
The bound is never to be re-derived from what a GPU gives."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
DTS = {"fp16": torch.float16, "bf16": torch.bfloat16}
E32 = 2.0 ** -24
C_SUM = 12.0
C_ACT = 8.0
L_SILU = 1.1
GROUPS = 32
EPS = 1e-5
FAMILIES = ("gauss", "offset_30", "offset_1000", "group_scales", "chan_offsets", "tiny_var", "const", "edge_outlier")
CONST = 37.3


def _gen(*key):
    return torch.Generator("cpu").manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def affine(C, seed=0):
    """gamma, beta [C] fp32: gamma of both signs around 1, beta 0.3 N."""
    g = _gen("affine", C, seed)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0)
    return gamma, 0.3 * torch.randn(C, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# input families.  GroupNorm: x [nb * S, C] (the virtual concat [x1 | x2]), 32 groups.  LayerNorm: the same call with
# groups = 1 and S = 1 (one "group" per row), plus a per-row scale so that neighbouring rows never share statistics.
def family(name, nb, S, C, groups=GROUPS, seed=0):
    """Every family but `gauss` carries a property that `family_property` asserts in fp64, so that it cannot silently turn
    into Gaussian noise."""
    G, cpg = groups, C // groups
    g = _gen(name, nb, S, C, groups, seed)
    r = torch.randn(nb, S, G, cpg, generator=g)
    if S * cpg > 1 and name != "gauss":     # exactly standardised per slice: a family's ratios hold at 64 elements as at 10^6
        r = (r - r.mean((1, 3), keepdim=True)) / r.std((1, 3), unbiased=False, keepdim=True)

    def sign(*shape):
        return torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    if name == "gauss":                             # the distribution of the older tests (kernel_cases.case_groupnorm)
        x = r * 1.7 + 0.6
    elif name in ("offset_30", "offset_1000"):      # every (batch, group): |mean| / sigma = 30 or 1000, sigma in [0.5, 2]
        k = float(name.split("_")[1])
        x = (0.5 + 1.5 * torch.rand(nb, 1, G, 1, generator=g)) * (sign(nb, 1, G, 1) * k + r)
    elif name == "group_scales":                    # every (batch, group) its own mean (<= 50, random sign) and scale (10^+-2)
        n = nb * G
        logs = torch.randperm(n, generator=g).double() / max(n - 1, 1) * 4 - 2
        sc = (10.0 ** logs).float().view(nb, 1, G, 1)
        mean = sign(nb, 1, G, 1) * (5 + 45 * torch.rand(nb, 1, G, 1, generator=g))
        x = mean + sc * r
    elif name == "chan_offsets":                    # a constant per channel + 1 % smooth noise: the trained-checkpoint shape
        off = sign(1, 1, G, cpg) * (2 + 3 * torch.rand(1, 1, G, cpg, generator=g))
        f = torch.randint(1, 4, (1, 1, G, cpg), generator=g).float()
        ph = torch.rand(nb, 1, G, cpg, generator=g)
        t = (torch.arange(S, dtype=torch.float32) / max(S, 1)).view(1, S, 1, 1)
        x = off * (1 + 0.01 * torch.sin(2 * math.pi * (f * t + ph)))
        if S < 8:                                   # LayerNorm rows: no row axis to be smooth along — 1 % white noise instead
            x = off * (1 + 0.01 * r)
    elif name == "tiny_var":                        # sigma^2 = eps / 10 around a mean of 1.5 .. 4.6 (mean / sigma up to 4600)
        m = sign(nb, 1, G, 1) * (1.5 + 0.1 * torch.arange(G, dtype=torch.float32).view(1, 1, G, 1))
        x = m + math.sqrt(EPS / 10) * r
    elif name == "const":
        x = torch.full_like(r, CONST)
    elif name == "edge_outlier":                    # first and last row of every slice ~ 10^3 (LayerNorm: first / last column)
        # both of a slice's outlier rows carry the slice's sign: the mean stays comparable with mean |x| (the bound prices the
        # error of an fp32 mean through |mu|; two rows that cancel would leave |mu| << mean |x| and nothing to price it with)
        x = r.clone()
        sg = sign(nb, G, 1)
        if S > 1:
            x[:, 0] = 1000 * (1 + 0.1 * r[:, 0]) * sg
            x[:, -1] = 1000 * (1 + 0.1 * r[:, -1]) * sg
        else:
            x[..., 0] = 1000 * (1 + 0.1 * r[..., 0]) * sg
            x[..., -1] = 1000 * (1 + 0.1 * r[..., -1]) * sg
    else:
        raise ValueError(name)
    return x.reshape(nb * S, C).contiguous()


def ln_family(name, M, d, seed=0):
    """LayerNorm input [M, d]: family `name` per row; every row additionally has its own scale (and `row_scales`, the
    analogue of `group_scales`, its own offset), so that statistics or data taken from another row are grossly wrong."""
    g = _gen("ln", name, M, d, seed)
    if name == "row_scales":
        # golden-ratio sequence: consecutive rows are 0.38 or 0.62 of the two decades apart, never close
        sc = (10.0 ** ((torch.arange(M, dtype=torch.float64) * 0.6180339887498949) % 1.0 * 2 - 1)).float().view(M, 1)
        off = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0) * (2 + 18 * torch.rand(M, 1, generator=g)) * sc
        return (off + sc * torch.randn(M, d, generator=g)).contiguous()
    x = family(name, M, 1, d, groups=1, seed=seed)
    if name in ("gauss", "tiny_var"):
        return x
    if name == "const":
        return x + (torch.arange(M) % 3).float().view(M, 1)
    return (x * 2.0 ** ((torch.arange(M) * 5 % 7).float() - 3).view(M, 1)).contiguous()      # exact scaling: ratios unchanged


LN_FAMILIES = FAMILIES[:3] + ("row_scales",) + FAMILIES[4:]


def _group_stats(x, nb, S, groups):
    v = x.double().view(nb, S, groups, -1)
    mu = v.mean((1, 3), keepdim=True)
    var = ((v - mu) ** 2).mean((1, 3), keepdim=True)
    return v, mu, var


def family_property(name, x, nb, S, groups=GROUPS, eps=EPS):
    """Asserts the property of family `name` on x [nb * S, C] in fp64."""
    v, mu, var = _group_stats(x, nb, S, groups)
    sd = var.sqrt()
    rstd = (var + eps) ** -0.5
    G = groups
    if name in ("offset_30", "offset_1000"):
        k = float(name.split("_")[1])
        ratio = (mu.abs() / sd.clamp_min(1e-300)).flatten()
        assert bool(((ratio > 0.9 * k) & (ratio < 1.1 * k)).all()), (float(ratio.min()), float(ratio.max()))
    elif name in ("group_scales", "row_scales"):
        # statistics of the neighbouring group / row, or of batch 0, are grossly wrong for every slice
        def gross(mu2, rstd2):
            return ((rstd2 / rstd - 1).abs() >= 0.05) | (((mu2 - mu) * rstd).abs() >= 1.0)
        if name == "row_scales":
            assert nb == 1 or bool(gross(mu.roll(1, 0), rstd.roll(1, 0)).all())
        else:
            assert bool(gross(mu.roll(-1, 2), rstd.roll(-1, 2)).all())
            assert nb > 1 and bool(gross(mu[:1].expand_as(mu), rstd[:1].expand_as(rstd))[1:].all())
    elif name == "chan_offsets":
        cm = v.mean(1, keepdim=True)
        if S >= 8:        # per channel: constant to ~1 % over the rows, and that is what a 64-row slab sees
            cs = ((v - cm) ** 2).mean(1, keepdim=True).sqrt()
            assert float((cm.abs() / cs.clamp_min(1e-300)).min()) >= 50
        else:             # LayerNorm: the columns of a row differ by O(1) offsets, mean / sigma of a row stays O(1)
            assert float((v.abs().amin(3) / sd.squeeze(3)).min()) > 0.1
    elif name == "tiny_var":
        assert float(var.max()) < eps / 5 and float(mu.abs().min()) >= 1
    elif name == "const":
        assert float((v.amax((1, 3)) - v.amin((1, 3))).abs().max()) == 0.0 and float(v.abs().min()) >= CONST - 1e-5
    elif name == "edge_outlier":
        if S > 1:
            drops = (v[:, 1:], v[:, :-1])
        else:
            drops = (v[..., 1:], v[..., :-1])
        for w in drops:      # without its first or its last row (column) every slice has a grossly different rstd
            m2 = w.mean((1, 3), keepdim=True)
            r2 = (((w - m2) ** 2).mean((1, 3), keepdim=True) + eps) ** -0.5
            assert float((r2 / rstd - 1).abs().min()) >= 0.1
    elif name != "gauss":
        raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------------
# reference, bound, statistic
@dataclass
class Ref:
    y: torch.Tensor        # fp64 [rows, C]
    f32: torch.Tensor      # the fp32 part of the bound
    mu: torch.Tensor
    rstd: torch.Tensor


def reference(x, nb, S, groups, gamma, beta, eps, silu):
    """fp64 norm of the fp32 tensor x [nb * S, C] over (rows of a batch) x (channels of a group)."""
    rows, C = x.shape
    v, mu, var = _group_stats(x, nb, S, groups)
    rstd = (var + eps) ** -0.5
    ga = gamma.double().view(1, 1, groups, -1)
    be = beta.double().view(1, 1, groups, -1)
    f32 = (v.abs() + mu.abs()) * (rstd * ga.abs())              # A
    v = (v - mu) * (rstd * ga)                                   # z - beta
    f32 += v.abs() + be.abs()
    f32 *= C_SUM * E32 * (L_SILU if silu else 1.0)
    v = v + be
    if silu:
        v = v * torch.sigmoid(v)
        f32 += (C_ACT * E32) * v.abs()
    return Ref(v.reshape(rows, C), f32.reshape(rows, C), mu, rstd)


def bound(ref, dt):
    if dt == torch.float32:
        return ref.f32
    return ref.f32 + U[dt] * ref.y.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)


def worst_ratio(out, y, bnd):
    """max over elements of |err| / bound (a zero bound demands exactness; a non-finite output is inf)."""
    err = (out.double() - y).abs()
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(torch.isfinite(out.double()), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def rel_l2(out, y):
    return float((out.double() - y).norm() / y.norm().clamp_min(1e-300))


def offenders(out, y, bnd, nb, S, groups, limit=12):
    """What a failing GPU test prints: the elements over the bound and which (batch, group) slices / rows hold them."""
    err = (out.double() - y).abs()
    bad = ~(err <= bnd) | ~torch.isfinite(out.double())
    idx = bad.nonzero()
    C = out.shape[1]
    lines = [f"{int(bad.sum())} of {bad.numel()} elements over the bound, shape {tuple(out.shape)}"]
    for r, c in idx[:limit].tolist():
        lines.append(f"  row {r} (batch {r // S}, row {r % S}) ch {c} (group {c // (C // groups)}): out {float(out[r, c]):.6g} "
                     f"ref {float(y[r, c]):.6g} err/bound {float(err[r, c] / bnd[r, c]):.3g}")
    if len(idx):
        sl = (idx[:, 0] // S * groups + idx[:, 1] // (C // groups)).unique().tolist()
        lines.append(f"  (batch * groups + group) slices hit: {sl[:40]}{' ...' if len(sl) > 40 else ''} of {nb * groups}")
        rr = (idx[:, 0] % S).unique().tolist()
        lines.append(f"  rows within a batch hit: {len(rr)} of {S}, first {rr[:10]}, last {rr[-3:]}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# CPU models (fp32 torch, vectorised)
GN_DEFECTS = ("raw_moments", "no_clamp", "drop_last_row", "neighbour_group", "batch0_stats", "eps_omitted", "x2_stride_of_x1")


def _bsum(t, block=64):
    """fp32 sum over dims (1, 3) of [nb, R, G, c] as the kernels do it: within a row, then blocks of rows, then the blocks."""
    s = t.sum(3)
    nb, R, G = s.shape
    pad = (-R) % block
    if pad:
        s = torch.cat([s, torch.zeros(nb, pad, G)], 1)
    return s.view(nb, -1, block, G).sum(2).sum(1).view(nb, 1, G, 1)


def silu32(z):
    return z * (1.0 / (1.0 + torch.exp2(-1.44269504088896340736 * z)))


def gn_centred_model(x, nb, S, gamma, beta, eps, silu, dt, groups=GROUPS, defect=None, C1=None, slab_elems=16384):
    """gn_fused / gn_regs (and the streaming pipeline with shifted moments) on the CPU: fp32 mean by blocked sums, centred
    second pass, y = act(x * scale + shift) in fp32, one rounding.  `defect` switches on one modelled mistake;
    `raw_moments` / `no_clamp` replace the statistics by fp32 sum x^2 - (sum x)^2 / n per slab of `slab_elems` elements
    followed by a Chan merge (the streaming pipeline before this file existed), with / without the clamp at zero."""
    assert defect is None or defect in GN_DEFECTS, defect
    rows, C = x.shape
    G, cpg = groups, C // groups
    v = x.float().view(nb, S, G, cpg)
    if defect == "x2_stride_of_x1":          # the straddling group reads its x2 part with x1's row stride
        assert C1 is not None and C1 % cpg
        x2 = x[:, C1:].contiguous().flatten()
        g0 = C1 // cpg
        r_ = torch.arange(rows).view(rows, 1)
        c_ = torch.arange(0, (g0 + 1) * cpg - C1).view(1, -1)
        v = v.clone()
        v.view(rows, C)[:, C1:(g0 + 1) * cpg] = x2[(r_ * C1 + c_) % x2.numel()]
    st = v[:, :-1] if defect == "drop_last_row" and S > 1 else v
    n = float(st.shape[1] * cpg)
    if defect in ("raw_moments", "no_clamp"):
        rp = max(slab_elems // C, 1)
        pad = (-S) % rp
        vp = torch.cat([v, torch.zeros(nb, pad, G, cpg)], 1).view(nb, -1, rp, G, cpg)
        cnt = torch.full((vp.shape[1],), float(rp * cpg))
        cnt[-1] = float((rp - pad) * cpg)
        cnt = cnt.view(1, -1, 1)
        a = torch.zeros(nb, vp.shape[1], G, cpg)                   # per-thread chains down the rows of a slab, as gn_stats ran them
        b = torch.zeros_like(a)
        for i in range(rp):
            a += vp[:, :, i]
            b += vp[:, :, i] * vp[:, :, i]
        a, b = a.sum(3), b.sum(3)                                  # [nb, slabs, G]
        mb = a / cnt
        m2 = b - a * mb
        if defect == "raw_moments":
            m2 = m2.clamp_min(0)
        mean = ((mb * cnt).sum(1) / n).view(nb, 1, G, 1)
        var = ((m2 + cnt * (mb - mean.view(nb, 1, G)) ** 2).sum(1) / n).view(nb, 1, G, 1)
    else:
        mean = _bsum(st) / n
        d = st - mean
        var = _bsum(d * d) / n
    if defect == "neighbour_group":          # ONE (batch, group) normalised with its neighbour's statistics
        mean, var = mean.clone(), var.clone()
        mean[nb - 1, 0, 5], var[nb - 1, 0, 5] = mean[nb - 1, 0, 6].clone(), var[nb - 1, 0, 6].clone()
    if defect == "batch0_stats":
        mean, var = mean[:1].expand(nb, 1, G, 1), var[:1].expand(nb, 1, G, 1)
    rstd = 1.0 / torch.sqrt(var if defect == "eps_omitted" else var + eps)
    scale = gamma.float().view(1, 1, G, cpg) * rstd
    shift = beta.float().view(1, 1, G, cpg) - mean * scale
    o = v * scale + shift
    if silu:
        o = silu32(o)
    return o.reshape(rows, C).to(dt)


def ln_model(x, gamma, beta, eps, dt, defect=None):
    """layernorm_kernel / layernorm_stream_kernel: two passes from registers in fp32, (x - mean) * rstd * gamma + beta."""
    assert defect in (None, "ln_row_from_neighbour")
    M, d = x.shape
    v = x.float().view(M, -1, 4)
    mean = (v.sum(2).sum(1) / d).view(M, 1)
    c = x.float() - mean
    q = (c * c).view(M, -1, 4).sum(2).sum(1).view(M, 1)
    rstd = 1.0 / torch.sqrt(q / d + eps)
    out = (c * rstd * gamma.float() + beta.float()).to(dt)
    if defect and M > 1:
        out[M // 2] = out[M // 2 - 1]
    return out


def torch_norm(x, nb, S, groups, gamma, beta, eps, silu):
    """torch's own fp32 group_norm / layer_norm (+ SiLU): the yardstick the bound is held against on the CPU."""
    rows, C = x.shape
    if groups == 1 and S == 1:
        y = torch.nn.functional.layer_norm(x, (C,), gamma, beta, eps)
    else:
        y = torch.nn.functional.group_norm(x.view(nb, S, C).permute(0, 2, 1).contiguous(), groups, gamma, beta, eps)
        y = y.permute(0, 2, 1).reshape(rows, C)
    return torch.nn.functional.silu(y) if silu else y


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of csrc/norm_plan.cpp, ASKED of the library (vgen_groupnorm_query_plan / vgen_layernorm_query_plan launch
# nothing and need no GPU): nothing of the rule is written down here
GN_PATHS = ("fused", "regs", "stream", "cs256", "cs1024")        # enum GnPath


def _gn_query(nb, S, C1, C2, has_cs):
    import ctypes
    from vgen_amd import lib
    out4 = (ctypes.c_int32 * 4)()
    lib.check(lib.load().vgen_groupnorm_query_plan(nb, S, C1, C2, GROUPS, int(bool(has_cs)), out4), "vgen_groupnorm_query_plan")
    return tuple(out4)


def gn_path(nb, S, C1, C2, has_cs):
    return GN_PATHS[_gn_query(nb, S, C1, C2, has_cs)[0]]


def gn_nsplit(nb, S, C):
    """(nsplit, rows per slab) of the streaming pipeline, and nsplit before the planner's 1024-block floor: the slabs of ~16 K
    elements (at least 2 rows) that the shapes of GN_SHAPES["stream"] were chosen around — a property of that choice, not of
    the dispatch."""
    _, ns, rows_per, _ = _gn_query(nb, S, C, 0, False)
    return ns, rows_per, -(-S // max(16384 // C, 2))


# (nb, S, C1, C2): the smallest shape per path and edge; ALL families where the tensor is <= 6 M elements, the conditioning
# families above that
GN_SHAPES = {
    "fused": [(3, 50, 128, 0), (2, 33, 640, 320), (2, 614, 1280, 0)],
    "regs": [(2, 615, 1280, 0), (2, 1836, 1280, 0), (2, 448, 1280, 1280)],
    "stream": [(2, 1837, 1280, 0), (2, 1000, 2560, 0), (2, 12000, 320, 0), (4, 13056, 320, 0)],
    "cs256": [(2, 2496, 320, 0), (2, 640, 640, 640)],
    "cs1024": [(2, 3328, 1280, 0)],
}
BIG_FAMILIES = ("offset_1000", "group_scales", "chan_offsets", "edge_outlier")


def gn_families(shape):
    nb, S, C1, C2 = shape
    return FAMILIES if nb * S * (C1 + C2) <= 6_000_000 else BIG_FAMILIES


def gn_cases():
    """(path, shape, family) of every GPU GroupNorm case."""
    return [(p, s, f) for p, shapes in GN_SHAPES.items() for s in shapes for f in gn_families(s)]


def gn_variants(path, shape):
    """(dtype name, silu, raw) launches of a case: both dtypes x SiLU on / off on every shape; the first shape of each path
    also takes the raw copies (plain and two-term)."""
    first = shape == GN_SHAPES[path][0]
    return [("fp16", True, True if first else False), ("bf16", False, "split" if first else False), ("fp16", False, False),
            ("bf16", True, False)]


# LayerNorm: (M, d, out) with out in {"16", "f32"}; RPB = 256 / LPR rows per block
def ln_lpr(d):
    """lanes per row of the LayerNorm kernels at width d (the same for both kernels and every output type)"""
    import ctypes
    from vgen_amd import lib
    out3 = (ctypes.c_int32 * 3)()
    lib.check(lib.load().vgen_layernorm_query_plan(1, d, lib.VGEN_F16, out3), "vgen_layernorm_query_plan")
    return out3[0]


LN_STREAM_WIDTHS = (320, 512, 640, 1024, 1280, 2048)
LN_OFF_WIDTHS = (192, 768, 1536)               # one per LPR, the one-shot kernel
LN_WRAP = [(16 * 4097 + 3, 320), (8 * 4097 + 3, 640), (4 * 4097 + 3, 1280)]     # > 2 x 2048 row groups + a ragged tail


def ln_small_ms(d):
    rpb = 256 // ln_lpr(d)
    return (1, rpb - 1, rpb + 1, 3 * rpb + 2)


def ln_cases():
    """(M, d, out kind, families)"""
    c = []
    for d in LN_STREAM_WIDTHS + LN_OFF_WIDTHS:
        for M in ln_small_ms(d):
            c.append((M, d, "16", LN_FAMILIES))
    for d in (320, 768, 2048, 64):
        c.append((256 // ln_lpr(d) + 1, d, "f32", LN_FAMILIES))
    for M, d in LN_WRAP:
        c.append((M, d, "16", ("row_scales",)))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# guard rows: inputs are a row slice of a buffer whose other rows are NaN, outputs land between sentinel rows
GUARD = 3


def nan_framed(x):
    """(buffer [rows + 2 GUARD, C] with NaN guard rows, the live contiguous row slice)"""
    buf = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), float("nan"), dtype=x.dtype)
    buf[GUARD:-GUARD] = x
    return buf


def sentinel(rows, cols, dt):
    """A fixed finite bit pattern (fp16 / bf16 values in [1, 2), fp32 around 1.0), compared by bits after a launch."""
    i = torch.arange(rows * cols, dtype=torch.int64)
    if dt == torch.float32:
        return (0x3F800000 + (i * 7919 + 13) % 1021).to(torch.int32).view(torch.float32).view(rows, cols)
    return ((0x3C00 if dt == torch.float16 else 0x3F80) + (i * 7919 + 13) % 101).to(torch.int16).view(dt).view(rows, cols)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def guard_violations(before, after):
    """Flat indices in the guard rows (first / last GUARD rows of [rows + 2 GUARD, cols]) whose bits changed."""
    ch = bits(before) != bits(after)
    ch[GUARD:-GUARD] = False
    return ch.flatten().nonzero().flatten().tolist()
