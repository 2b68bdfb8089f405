"""Adversarial attention cases: input families, the fp64 reference, a DERIVED per-element bound, a CPU model of the flash
kernels' arithmetic (with switchable modelled defects) and a guard-band harness for what a launch reads and writes beyond
its operands.  Pure torch on the CPU; shared by tests/test_attention_edges.py (CPU and GPU tests) and tests/gpu_diag.py.

Reference, for one (sequence, head), in float64 from the SAME 16-bit operands the kernel gets:

    P = softmax(q k^T * scale [causal mask]),   O = P v,   A = P |v|

Bound per output element (i, d), u = 2^-11 (fp16) / 2^-8 (bf16) = half an ulp (both conversions of csrc/common.h round
to nearest even):

    |out[i, d] - O[i, d]|  <=  3 u A[i, d]  +  nk * 2^-25 * max_j |v[j, d]|        (second term fp16 only)

Derivation: every P entry is rounded ONCE to 16 bit before the P.V MFMA (relative error <= u each, so <= u A on the
output); the output is rounded once (<= u |O| <= u A); the fp32 effects (MFMA accumulation, v_exp_f32, the online
rescales) are orders below u for nk <= 4096.  That is 2 u A; the factor 3 is the margin for the lower-order terms.  The
fp16 term covers P entries below the fp16 normal range (absolute error <= 2^-25 each, unnormalised P <= 1, row sum >= 1).
temporal_kernel rounds P / sum rather than P: the same bound holds.  The statistic is worst = max |err| / bound; a test
asserts worst <= 1.  `flash_model` (64-key tiles, online softmax in fp32, P rounded to 16 bit, fp32 accumulation, one output
rounding) stays between 0.03 and 0.59 over the families below; the fp64 reference merely rounded to 16 bit reaches 0.33.
The bound is never to be re-derived from what a GPU gives."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTS = {"fp16": torch.float16, "bf16": torch.bfloat16}
BKV = 64                      # KV tile of flash_kernel / flash_d80_kernel
FAMILIES = ("gauss", "late_max", "late_half", "ascending", "descending", "all_negative", "flat", "onehot", "v_outlier")
TILE_ORDER = ("late_max", "late_half", "ascending", "descending")       # need nk > BKV
STEP = 0.35                   # ascending / descending: scaled-score step per key along the shared direction


def head_scale(D):
    return 0.125 if D == 64 else D ** -0.5


def _gen(*key):
    return torch.Generator("cpu").manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _unit(D, g):
    return torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)


# ---------------------------------------------------------------------------------------------------------------------
# input families
def family(name, nq, nk, D, dt, seed=0, causal=False):
    """One (sequence, head) of family `name`: q [nq, D], k, v [nk, D] in `dt`.  Every family but `gauss` carries a property
    that `family_property` asserts on the fp64 reference, so that it cannot silently turn into Gaussian noise."""
    g = _gen(name, nq, nk, D, seed)
    scale = head_scale(D)
    q = torch.randn(nq, D, generator=g)
    k = torch.randn(nk, D, generator=g)
    v = torch.randn(nk, D, generator=g)
    if name == "gauss":
        pass
    elif name == "late_max":          # the last key dominates every row by a wide margin
        k[-1] = 0
        k[-1, :8] = 6.0
        q[:, :8] = q[:, :8].abs() + 4
    elif name == "late_half":         # the last key alone balances everything before the last tile
        k *= 0.7
        q[:, 0] = 1.0
        k[:, 0] = 0.0
        k[-1] = 0
        t0 = (nk - 1) // BKV * BKV
        e = torch.exp(q.to(dt).double() @ k.to(dt).double().T * scale)
        need = (e[:, :t0].sum(1) - e[:, t0:nk - 1].sum(1)).median().clamp_min(1.0)
        k[-1, 0] = float(torch.log(need)) / scale
    elif name in ("ascending", "descending"):
        u = _unit(D, g)
        sign = 1.0 if name == "ascending" else -1.0
        ramp = sign * (torch.arange(nk, dtype=torch.float32) - nk / 2) * (STEP / (8.0 * scale))
        k = 0.03 * k + u[None, :] * ramp[:, None]
        q = 0.03 * q + u[None, :] * 8.0
    elif name == "all_negative":      # q and k anti-aligned: every scaled score <= -20; V offset
        u = _unit(D, g)
        q = 0.3 * q + u[None, :] * 18.0
        k = 0.3 * k - u[None, :] * 18.0
        v = v + 2
    elif name == "flat":
        k[:] = k[0].clone()
    elif name == "onehot":
        k = torch.nn.functional.normalize(k, dim=1) * 8
        q = k[onehot_perm(nq, nk, D, seed, causal)] * 1.5
    elif name == "v_outlier":
        v = v * 3 + 5
        v = torch.where(v.abs() < 2, 4 - v, v)          # |v| >= 2 everywhere: A >= 2 even for a row that sees one key
        v[torch.randint(0, nk, (4,), generator=g), torch.randint(0, D, (4,), generator=g)] = 2.0e4
    else:
        raise ValueError(name)
    return q.to(dt), k.to(dt), v.to(dt)


def onehot_perm(nq, nk, D, seed=0, causal=False):
    """The seeded non-monotone map i -> key of family `onehot` (under a causal mask: a key <= i)."""
    g = _gen("perm", nq, nk, D, seed)
    if causal:
        return (torch.rand(nq, generator=g) * (torch.arange(nq) + 1)).long().clamp_max(nk - 1)
    return torch.randperm(nk, generator=g)[torch.arange(nq) % nk]


def _probs(q, k, scale, causal):
    s = q.double() @ k.double().transpose(-1, -2) * scale
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), -math.inf)
    return s, torch.softmax(s, -1)


def family_property(name, q, k, v, D, seed=0, causal=False):
    """Asserts the property of family `name` on the fp64 reference of one (sequence, head)."""
    nq, nk = q.shape[0], k.shape[0]
    s, p = _probs(q, k, head_scale(D), causal)
    t0 = (nk - 1) // BKV * BKV                                  # first key of the last KV tile
    ntile = (nk + BKV - 1) // BKV
    if name == "late_max":
        assert nk > BKV and bool((p.argmax(1) >= t0).all()) and float(p.max(1).values.min()) >= 0.999
    elif name == "late_half":
        mass = p[:, t0:].sum(1)
        assert nk > BKV and float(((mass >= 0.3) & (mass <= 0.7)).double().mean()) >= 0.9, mass
    elif name == "ascending":
        assert nk > BKV
        tmax = torch.stack([s[:, t * BKV:(t + 1) * BKV].max(1).values for t in range(ntile)], 1)
        if causal:
            vis = s[:-1]                                         # rows i < nq - 1; -inf above the diagonal
            nxt = (q.double() @ k.double().T * head_scale(D))[torch.arange(nq - 1), torch.arange(1, nq)]
            assert float((nxt > vis.max(1).values).double().mean()) >= 0.95
        else:
            assert float((tmax[:, 1:] > tmax[:, :-1]).all(1).double().mean()) >= 0.95
    elif name == "descending":
        assert nk > BKV and float(p[:, :BKV].sum(1).min()) >= 1 - 1e-6
        assert any(float(p[:, t * BKV:(t + 1) * BKV].max()) < 2.0 ** -30 for t in range(1, ntile))
    elif name == "all_negative":
        assert float(s[torch.isfinite(s)].max()) <= -20 and float(s.max(1).values.max()) <= -20
    elif name == "flat":
        assert not causal
        assert float((p - 1.0 / nk).abs().max()) <= 1e-12
        assert float((p @ v.double() - v.double().mean(0)[None]).abs().max()) <= 1e-9 * max(1.0, float(v.double().abs().max()))
    elif name == "onehot":
        pm = p.max(1)
        assert float(pm.values.median()) >= 0.98 and bool((pm.indices == onehot_perm(nq, nk, D, seed, causal)).all())
    elif name == "v_outlier":
        o, a = p @ v.double(), p @ v.double().abs()
        assert bool(torch.isfinite(o).all()) and float(o.abs().max()) < 3e4 and float(a.min()) >= 2
        assert int((v.double() >= 1.9e4).sum()) >= 1
    elif name != "gauss":
        raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------------
# reference, bound, statistic (batched over leading dimensions: [..., n, D])
def reference(q, k, v, scale, causal=False):
    """fp64 attention of 16-bit operands q [..., nq, D], k / v [..., nk, D] -> (O, A = P |v|)."""
    _, p = _probs(q, k, scale, causal)
    v64 = v.double()
    return p @ v64, p @ v64.abs()


def bound(A, v, dt):
    """The per-element bound of the module docstring; A [..., nq, D], v [..., nk, D]."""
    b = 3 * U[dt] * A
    if dt == torch.float16:
        b = b + v.shape[-2] * 2.0 ** -25 * v.double().abs().amax(-2, keepdim=True)
    return b


def worst_ratio(out, O, bnd):
    """max over elements of |err| / bound (an element with a zero bound must be exact; a non-finite output is inf)."""
    err = (out.double() - O).abs()
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(torch.isfinite(out.double()), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def rel_l2(out, O):
    return float((out.double() - O).norm() / O.norm().clamp_min(1e-300))


def offenders(out, O, bnd, limit=20):
    """What a failing GPU test prints: the first elements over the bound and where they sit (query rows, 16-column d tiles,
    leading (batch, head) index) — the evidence one run leaves for finding the cause."""
    err = (out.double() - O).abs()
    bad = ~(err <= bnd) | ~torch.isfinite(out.double())
    idx = bad.nonzero()
    lines = [f"{int(bad.sum())} of {bad.numel()} elements over the bound, shape {tuple(out.shape)}"]
    for i in idx[:limit].tolist():
        t = tuple(i)
        lines.append(f"  {t}: out {float(out[t]):.6g} ref {float(O[t]):.6g} err/bound {float(err[t] / bnd.expand_as(err)[t]):.3g}")
    if len(idx):
        rows = torch.bincount(idx[:, -2], minlength=out.shape[-2])
        cols = torch.bincount(idx[:, -1] // 16, minlength=(out.shape[-1] + 15) // 16)
        lines.append("  per query row: " + str({i: int(c) for i, c in enumerate(rows.tolist()) if c}))
        lines.append("  per 16-column d tile: " + str(cols.tolist()))
        if out.dim() > 2:
            lead = idx[:, :-2].unique(dim=0).tolist()
            lines.append(f"  leading (batch, head) indices hit: {lead[:limit]}{' ...' if len(lead) > limit else ''}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# CPU model of the flash kernels' arithmetic
DEFECTS = ("ragged_mask", "causal_mask", "no_acc_rescale", "no_sum_rescale", "swap_keys", "row_from_neighbour")


def flash_model(q, k, v, scale, dt, causal=False, bkv=BKV, defect=None):
    """flash_kernel / flash_d80_kernel for one (sequence, head) on the CPU: fp32 scores, online softmax per `bkv`-key tile in
    the log2 domain, P rounded to `dt` before the P.V product, fp32 accumulation, one rounding of the output.  The padded
    keys of a ragged tile are staged as ZEROS and masked, as in the kernels.  `defect` switches on one modelled mistake."""
    assert defect is None or defect in DEFECTS, defect
    nq, D = q.shape
    nk = k.shape[0]
    npad = (nk + bkv - 1) // bkv * bkv
    kf = torch.zeros(npad, D)
    vf = torch.zeros(npad, D)
    kf[:nk], vf[:nk] = k.float(), v.float()
    qf = q.float()
    c = torch.tensor(scale * 1.44269504088896340736, dtype=torch.float32)
    m = torch.full((nq,), -math.inf)
    l = torch.zeros(nq)
    o = torch.zeros(nq, D)
    qi = torch.arange(nq)[:, None]
    for t in range(0, npad, bkv):
        s = qf @ kf[t:t + bkv].T
        idx = torch.arange(t, t + bkv)[None, :]
        s = s.masked_fill(idx > nk if defect == "ragged_mask" else idx >= nk, -math.inf)
        if causal:
            s = s.masked_fill(idx > qi + (1 if defect == "causal_mask" else 0), -math.inf)
        mn = torch.maximum(m, s.max(1).values)
        p = torch.exp2(s * c - (mn * c)[:, None])
        alpha = torch.exp2((m - mn) * c)
        alpha[torch.isnan(alpha)] = 0
        l = (l if defect == "no_sum_rescale" else l * alpha) + p.sum(1)
        p16 = p.to(dt).float()
        if defect == "swap_keys":        # keys 4 g + 1 and 4 g + 2 exchanged between P and the V fragment
            p16 = p16.view(nq, bkv // 4, 4)[:, :, [0, 2, 1, 3]].reshape(nq, bkv)
        o = (o if defect == "no_acc_rescale" else o * alpha[:, None]) + p16 @ vf[t:t + bkv]
        m = mn
    out = (o / l[:, None]).to(dt)
    if defect == "row_from_neighbour" and nq > 1:
        out[nq // 2] = out[nq // 2 - 1]
    return out


def temporal_model(q, k, v, scale, dt):
    """temporal_kernel for one (sequence, head): one tile, P / sum rounded to `dt`, fp32 product, one output rounding."""
    c = torch.tensor(scale * 1.44269504088896340736, dtype=torch.float32)
    s = q.float() @ k.float().T
    e = torch.exp2((s - s.max(1, keepdim=True).values) * c)
    p = (e * (1.0 / e.sum(1, keepdim=True))).to(dt).float()
    return (p @ v.float()).to(dt)


# ---------------------------------------------------------------------------------------------------------------------
# cases in the ABI's strided addressing
@dataclass
class Case:
    """One launch: operands live in flat 16-bit buffers `bufs` (several operands may share one), `ops[name] = (buffer,
    element offset of (bi = 0, row 0, head 0, 0), (rs, bo, bi))` exactly as vgen_attn_args addresses them."""
    D: int
    heads: int
    nq: int
    nk: int
    nbatch: int
    inner: int
    dt: torch.dtype
    causal: bool = False
    bufs: dict = field(default_factory=dict)
    ops: dict = field(default_factory=dict)

    @property
    def scale(self):
        return head_scale(self.D)

    def seqs(self, name, bufs=None):
        """Strided view [nbatch / inner, inner, n, heads, D] of operand `name` (in `bufs`, default the case's own)."""
        buf, off, (rs, bo, bi) = self.ops[name]
        n = self.nq if name in ("q", "out") else self.nk
        base = (bufs or self.bufs)[buf]
        return torch.as_strided(base, (self.nbatch // self.inner, self.inner, n, self.heads, self.D), (bo, bi, rs, self.D, 1), off)

    def operand(self, name, bufs=None):
        """[nbatch, heads, n, D] copy of operand `name`."""
        return self.seqs(name, bufs).permute(0, 1, 3, 2, 4).reshape(self.nbatch, self.heads, -1, self.D).clone()

    def live_mask(self, name):
        m = {b: torch.zeros(t.numel(), dtype=torch.bool) for b, t in self.bufs.items()}
        self.seqs(name, m).fill_(True)
        return m[self.ops[name][0]]

    def check(self):
        """Every address the ABI may form is inside its buffer and the ABI's alignment rules hold."""
        assert self.nbatch % self.inner == 0
        for name, (buf, off, st) in self.ops.items():
            n = self.nq if name in ("q", "out") else self.nk
            assert off % 8 == 0 and all(s % 8 == 0 for s in st), (name, off, st)
            last = off + (self.nbatch // self.inner - 1) * st[1] + (self.inner - 1) * st[2] + (n - 1) * st[0] + self.heads * self.D
            assert last <= self.bufs[buf].numel(), (name, last, self.bufs[buf].numel())
        assert int(self.live_mask("out").sum()) == self.nbatch * self.heads * self.nq * self.D   # no two rows overlap
        return self


def fill_family(case, name, seed=0):
    """Writes one family sequence per (sequence, head) into the case's q / k / v."""
    Q, K, V = case.seqs("q"), case.seqs("k"), case.seqs("v")
    for bo in range(case.nbatch // case.inner):
        for bi in range(case.inner):
            for h in range(case.heads):
                # cross attention (k_bi = 0) shares K / V among the `inner` sequences of a context: one draw per context,
                # the queries of sequence bi rotated by bi rows so that no two sequences have the same output
                shared = case.ops["k"][2][2] == 0
                q, k, v = family(name, case.nq, case.nk, case.D, case.dt, (seed, bo, 0 if shared else bi, h), case.causal)
                if shared:
                    q = q.roll(bi, 0)
                Q[bo, bi, :, h], K[bo, bi, :, h], V[bo, bi, :, h] = q, k, v
    return case


def _noise(n, dt, seed):
    return torch.randn(n, generator=_gen("noise", n, seed)).to(dt)


def make_case(layout, D, heads, nq, nk, nbatch, dt, causal=False, inner=1, guard=8, gap=8, pad=0.0):
    """Layouts: `plain` (q, k, v, out each dense), `packed` (fused [rows, 3 d] QKV, nq == nk), `cross` (q / out with `inner`
    sequences per context, K / V columns of a wider context buffer, k_bi = 0), `temporal` (sequences over frames at a row
    stride of `inner` pixels; K / V fused), `banded` (the guard-band harness: `guard` rows before and after every sequence's
    rows and `gap` columns after the live ones, inputs padded with `pad`, the output pre-filled with a sentinel pattern)."""
    d = heads * D
    c = Case(D=D, heads=heads, nq=nq, nk=nk, nbatch=nbatch, inner=inner, dt=dt, causal=causal)
    nbo = nbatch // inner
    if layout == "plain":
        assert inner == 1
        c.bufs = dict(q=_noise(nbatch * nq * d, dt, 1), k=_noise(nbatch * nk * d, dt, 2), v=_noise(nbatch * nk * d, dt, 3),
                      out=sentinel(nbatch * nq * d, dt))
        c.ops = dict(q=("q", 0, (d, nq * d, 0)), k=("k", 0, (d, nk * d, 0)), v=("v", 0, (d, nk * d, 0)),
                     out=("out", 0, (d, nq * d, 0)))
    elif layout == "packed":
        assert inner == 1 and nq == nk
        ld = 3 * d
        c.bufs = dict(qkv=_noise(nbatch * nq * ld, dt, 1), out=sentinel(nbatch * nq * d, dt))
        c.ops = dict(q=("qkv", 0, (ld, nq * ld, 0)), k=("qkv", d, (ld, nq * ld, 0)), v=("qkv", 2 * d, (ld, nq * ld, 0)),
                     out=("out", 0, (d, nq * d, 0)))
    elif layout == "cross":
        kw, off = 2 * d + 64, 64                                  # K at column 64, V behind it, of a wider context row
        c.bufs = dict(q=_noise(nbatch * nq * d, dt, 1), kv=_noise(nbo * nk * kw, dt, 2), out=sentinel(nbatch * nq * d, dt))
        c.ops = dict(q=("q", 0, (d, inner * nq * d, nq * d)), k=("kv", off, (kw, nk * kw, 0)),
                     v=("kv", off + d, (kw, nk * kw, 0)), out=("out", 0, (d, inner * nq * d, nq * d)))
    elif layout == "temporal":
        S = inner
        c.bufs = dict(q=_noise(nbo * nq * S * d, dt, 1), kv=_noise(nbo * nk * S * 2 * d, dt, 2),
                      out=sentinel(nbo * nq * S * d, dt))
        c.ops = dict(q=("q", 0, (S * d, nq * S * d, d)), k=("kv", 0, (S * 2 * d, nk * S * 2 * d, 2 * d)),
                     v=("kv", d, (S * 2 * d, nk * S * 2 * d, 2 * d)), out=("out", 0, (S * d, nq * S * d, d)))
    elif layout == "banded":
        assert inner == 1 and guard % 8 == 0 and gap % 8 == 0
        rs = d + gap
        for name, n in (("q", nq), ("k", nk), ("v", nk), ("out", nq)):
            slot = (n + 2 * guard) * rs
            c.bufs[name] = sentinel(nbatch * slot, dt) if name == "out" else torch.full((nbatch * slot,), pad, dtype=dt)
            c.ops[name] = (name, guard * rs, (rs, slot, 0))
    else:
        raise ValueError(layout)
    return c.check()


def sentinel(n, dt):
    """A fixed finite 16-bit pattern (values in [1, 2) for fp16): compared by bits after a launch."""
    i = torch.arange(n, dtype=torch.int64)
    return (0x3C00 + (i * 7919 + 13) % 1021).to(torch.int16).view(dt)


def footprint_violations(before, after, live):
    """Flat indices outside `live` whose bits changed."""
    return ((before.view(torch.int16) != after.view(torch.int16)) & ~live).nonzero().flatten().tolist()


def case_reference(case):
    """(O, bound) of a case, [nbatch, heads, nq, D] in fp64 — computed once and reused for every launch of the case."""
    q, k, v = case.operand("q"), case.operand("k"), case.operand("v")
    O, A = reference(q, k, v, case.scale, case.causal)
    return O, bound(A, v, case.dt)


def torch_kernel(case, bufs, model=None):
    """A stand-in 'kernel' in torch that writes the case's output through the ABI's addressing (harness self-tests)."""
    q, k, v = (case.operand(n, bufs) for n in ("q", "k", "v"))
    O = reference(q, k, v, case.scale, case.causal)[0].to(case.dt)
    case.seqs("out", bufs).copy_(O.view(case.nbatch // case.inner, case.inner, case.heads, case.nq, case.D).permute(0, 1, 3, 2, 4))


# ---------------------------------------------------------------------------------------------------------------------
# shapes (query tiles of 128 = 4 waves x 2 fragments of 16, KV tiles of 64)
# flash_kernel, non-causal: (layout, heads, nq, nk, nbatch, inner)
FLASH_SHAPES = [
    ("cross", 1, 1, 64, 4, 2), ("cross", 3, 1, 65, 2, 1), ("plain", 3, 16, 17, 2, 1), ("cross", 1, 17, 16, 6, 3),
    ("cross", 3, 33, 77, 4, 2), ("packed", 3, 128, 128, 2, 1), ("plain", 1, 129, 63, 2, 1), ("cross", 1, 130, 257, 4, 2),
    ("cross", 3, 257, 1, 2, 2), ("temporal", 1, 32, 32, 10, 5), ("packed", 1, 200, 200, 3, 1),
]
CAUSAL_SHAPES = [("packed", h, n, n, 2, 1) for h, n in ((1, 1), (3, 12), (1, 64), (3, 65), (3, 77), (1, 129), (1, 200))]
# temporal_kernel: every (nq, nk) of {1, 3, 4, 15, 16}^2 in a strided and a plain layout; 1, 5 or 8 (sequence, head) pairs
# (4 per block: the last block partly idle)
_T = (1, 3, 4, 15, 16)
TEMPORAL_SHAPES = []
for _i, _nq in enumerate(_T):
    for _j, _nk in enumerate(_T):
        _pairs = (1, 5, 8)[(_i + _j) % 3]
        TEMPORAL_SHAPES.append(("temporal", 1, _nq, _nk, _pairs, _pairs))
        _pairs = (1, 5, 8)[(_i + _j + 1) % 3]
        TEMPORAL_SHAPES.append(("plain", 1, _nq, _nk, _pairs, 1) if _pairs != 8 else ("plain", 2, _nq, _nk, 4, 1))
D80_SHAPES = [
    ("plain", 16, 1, 257, 2, 1), ("plain", 16, 257, 257, 2, 1), ("plain", 3, 129, 64, 2, 1), ("packed", 3, 130, 130, 2, 1),
    ("plain", 3, 20, 300, 3, 1), ("cross", 3, 257, 1, 2, 2), ("packed", 3, 257, 257, 1, 1),
]
KERNELS = {"flash": (64, False, FLASH_SHAPES), "causal": (64, True, CAUSAL_SHAPES), "temporal": (64, False, TEMPORAL_SHAPES),
           "d80": (80, False, D80_SHAPES)}
# `flat` / `v_outlier`: three shapes per kernel (indices into the lists above); v_outlier needs A >= 2, i.e. enough keys
FEW = {"flash": (4, 5, 7), "causal": (3, 4, 6), "temporal": (36, 46, 48), "d80": (1, 3, 4)}


def shapes_for(kernel, fam):
    D, causal, shapes = KERNELS[kernel]
    if fam in ("flat", "v_outlier"):
        if fam == "flat" and causal:
            return []                                            # a causal row is not uniform over all keys
        return [shapes[i] for i in FEW[kernel]]
    if fam in TILE_ORDER:
        if causal and fam != "ascending":
            return []                                            # the last tile is invisible to most causal rows
        return [s for s in shapes if s[3] > BKV]
    return list(shapes)


def build(kernel, shape, dt, fam, seed=0):
    D, causal, _ = KERNELS[kernel]
    layout, heads, nq, nk, nbatch, inner = shape
    return fill_family(make_case(layout, D, heads, nq, nk, nbatch, dt, causal=causal, inner=inner), fam, seed)


# ---------------------------------------------------------------------------------------------------------------------
# vgen_softmax_rows: fp64 reference softmax(S * scale), bound per element 2 u P + 2^-25 (one rounding of a value computed
# in fp32; the factor 2 is the margin for the fp32 terms), row sums within 2 u + cols * 2^-25 of 1
SOFTMAX_COLS = (1, 2, 255, 256, 257, 1000, 4096)
SOFTMAX_ROWS = (1, 70)
SOFTMAX_KINDS = ("gauss", "onehot", "equal", "last_max", "deep")


def softmax_input(kind, rows, cols, seed=0):
    g = _gen("softmax", kind, rows, cols, seed)
    if kind == "gauss":
        return torch.randn(rows, cols, generator=g) * 4
    if kind == "onehot":
        S = torch.zeros(rows, cols)
        S[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 80.0
        return S
    if kind == "equal":
        return torch.full((rows, cols), 3.25)
    if kind == "last_max":
        S = torch.randn(rows, cols, generator=g)
        S[:, -1] = 9.0
        return S
    if kind == "deep":
        S = torch.full((rows, cols), -1.0e4)
        S[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 0.0
        return S
    raise ValueError(kind)


def softmax_reference(S, scale, dt):
    P = torch.softmax(S.double() * scale, -1)
    return P, 2 * U[dt] * P + 2.0 ** -25
