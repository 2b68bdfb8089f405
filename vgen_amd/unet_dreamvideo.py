"""UNetSD_DreamVideo — MI355X-native drop-in for the reference's DreamVideo UNet (tools/modules/unet/unet_dreamvideo.py:
19-293; engine tools/inferences/inference_dreamvideo_entrance.py): the t2v trunk, block for block, with the identity
adapter (`spatial_adapter_list`, inside every SpatialTransformer) and the motion adapter (`temporal_adapter_list`, inside
every TemporalTransformer, conditioned on the CLIP image embedding `y_image`) of util.py:499-519, 603-672.

Interface parity: registry name, constructor keywords and `state_dict()` keys are the reference's (the engine's
`load_state_dict(base + identity adapter + motion adapter, strict=True)` works unchanged; with both lists empty the key
set and the output are UNetSD_T2VBase's); `forward(x, t, y=None, y_image=None, ..., ag_strength=1)` as :220-293,
`y_image` None, [B, 1, D] (broadcast over the frames, :270-271) or [B, F, D].

Execution.  An Adapter is ONE launch of vgen_adapter (include/vgen_hip.h) on the fp32 token stream: 16-bit operands, fp32
accumulation, the hidden activation never in memory.  In the 'parallel' position (util.py:645, 656, 665; the position of
every stock config) its output simply IS the tensor the branch's out-projection GEMM adds to (`residual`; for the
feed-forward adapter `_ff_out` keeps its 16-bit emission for proj_out).  The condition does not cost a pass over the
tokens: down(x + lam (Wc c + bc)) = down(x) + lam Wd (Wc c + bc), so per (unit, frame) the term
hb = b_down + Wd (lam (Wc c + bc)) is a PROMPT CONSTANT — evaluated once per prompt in fp32 from the fp32 parameters
(vgen_linear_f32) and handed to the kernel as a hidden row bias; a sampling session (vgen_amd/session.py) keeps it in a
static buffer next to the K/V rows.  The 'serial' position (the adapter after the branch) is not built: the constructor
rejects it by keyword.

Precision.  Adapter weights are always one to-nearest 16-bit matrix (outside the two-term / calibrated sets).  Measured on
the two full-width fixtures, fp16, rel-L2 from the reference's fp32 output (profiles/dreamvideo_parity.json): "fast" 1.19e-3
(the reference's own autocast: 1.98e-3), "mixed" 7.6e-4 / 6.0e-4, "high" 7.2e-4; "calibrated" not measured at full width.
"fast" misses the project's 1e-3, "mixed" is the fastest mode that meets it on both: the default stays the trunk's, "mixed".
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .unet import UNetSD_T2VBase, _SpatialTransformerP, _TemporalTransformerP, _f32

# adapter_list entry -> (attribute of BasicTransformerBlockWithAdapter, slot of UNetSD_T2VBase._adapt, index into the
# position list) — util.py:630-635, 642-670
_SLOTS = {"self_attention": ("attn_adapter", "a1", 0), "cross_attention": ("cross_attn_adapter", "a2", 1),
          "feedforward": ("ff_adapter", "ff", 2)}
HP_MULT = 32       # vgen_adapter: hidden width padded to a multiple of 32 (zero rows / columns)


class _AdapterP(nn.Module):
    # reference: Adapter, util.py:499-509
    def __init__(self, d, hidden, cond_dim=None):
        super().__init__()
        self.down_linear = nn.Linear(d, hidden)
        self.up_linear = nn.Linear(hidden, d)
        self.condition_dim = cond_dim
        if cond_dim is not None:
            self.condition_linear = nn.Linear(cond_dim, d)
        nn.init.zeros_(self.up_linear.weight)
        nn.init.zeros_(self.up_linear.bias)


class UNetSD_DreamVideo(UNetSD_T2VBase):
    def __init__(self, *args, spatial_adapter_list=[], spatial_adapter_position_list=['', 'parallel', ''],
                 spatial_adapter_hidden_dim=None, temporal_adapter_list=[],
                 temporal_adapter_position_list=['parallel', 'parallel', 'parallel'], temporal_adapter_condition_dim=None,
                 temporal_adapter_hidden_dim=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.spatial_adapter_list, self.temporal_adapter_list = list(spatial_adapter_list), list(temporal_adapter_list)
        for kw, lst, pos in (("spatial_adapter", self.spatial_adapter_list, list(spatial_adapter_position_list)),
                             ("temporal_adapter", self.temporal_adapter_list, list(temporal_adapter_position_list))):
            for a in lst:
                if a not in _SLOTS:
                    raise ValueError(f"{kw}_list: unknown adapter {a!r} (one of {sorted(_SLOTS)})")
                i = _SLOTS[a][2]
                p = pos[i] if i < len(pos) else ''
                if p == "serial":
                    raise NotImplementedError(f"{kw}_position_list[{i}] = 'serial' ({a}) is not built in vgen_amd: "
                                              f"only the 'parallel' adapter position runs natively")
                if p != "parallel":
                    raise ValueError(f"{kw}_position_list[{i}] = {p!r} for the {a} adapter: expected 'parallel'")
        for m in list(self.modules()):
            if isinstance(m, _SpatialTransformerP):
                lst, hid, cond = self.spatial_adapter_list, spatial_adapter_hidden_dim, None
            elif isinstance(m, _TemporalTransformerP):
                lst, hid, cond = self.temporal_adapter_list, temporal_adapter_hidden_dim, temporal_adapter_condition_dim
            else:
                continue
            d = m.inner
            h = hid if hid else d // 2
            if lst and (h % 8 or d % 64 or d > 1280 or (h + HP_MULT - 1) // HP_MULT * HP_MULT > 640):
                raise NotImplementedError(f"adapter {d} -> {h}: vgen_adapter needs d % 64 == 0, d <= 1280, h % 8 == 0, h <= 640")
            tb = m.transformer_blocks[0]
            for a in ("self_attention", "cross_attention", "feedforward"):        # the reference's creation order
                if a in lst:
                    setattr(tb, _SLOTS[a][0], _AdapterP(d, h, cond))
        self._hb = None            # {adapter key: [units, F, hp] hidden row biases} of the evaluation in flight

    # -- packing -----------------------------------------------------------------------------
    def _pack(self, device=None):
        P = super()._pack(device)
        dt = self.compute_dtype
        self._cond_keys = []
        for name, m in self.named_modules():
            if not isinstance(m, (_SpatialTransformerP, _TemporalTransformerP)):
                continue
            tb = m.transformer_blocks[0]
            ad = {}
            for attr, slot, _ in _SLOTS.values():
                a = getattr(tb, attr, None)
                if a is None:
                    continue
                h, d = a.down_linear.weight.shape
                hp = (h + HP_MULT - 1) // HP_MULT * HP_MULT
                wd32 = torch.zeros((hp, d), dtype=torch.float32, device=a.down_linear.weight.device)
                wd32[:h] = a.down_linear.weight.detach().float()
                bd32 = torch.zeros((hp,), dtype=torch.float32, device=wd32.device)
                bd32[:h] = a.down_linear.bias.detach().float()
                wu32 = torch.zeros((d, hp), dtype=torch.float32, device=wd32.device)
                wu32[:, :h] = a.up_linear.weight.detach().float()
                e = dict(wd=wd32.to(dt).contiguous(), wu=wu32.to(dt).contiguous(), bu=_f32(a.up_linear.bias), h=int(h),
                         hb0=bd32.view(1, hp).contiguous(), key=f"{name}.{slot}", cond=a.condition_dim is not None)
                if e["cond"]:
                    # the condition path runs in fp32 on the fp32 parameters (once per prompt): [hp, d] incl. zero padding
                    e.update(wd32=wd32, bd32=bd32, wc=_f32(a.condition_linear.weight), bc=_f32(a.condition_linear.bias))
                    self._cond_keys.append((name, slot))
                ad[slot] = e
            if ad:
                P[name]["tb"]["ad"] = ad
        return P

    def _cond_adapters(self):
        if self._packed is None:
            self.pack()
        return [self._packed[name]["tb"]["ad"][slot] for name, slot in self._cond_keys]

    # -- the condition: hidden row biases, once per prompt ---------------------------------------------
    def _expand_y_image(self, y_image, F, device):
        c = y_image.to(device=device, dtype=torch.float32)
        if c.dim() != 3 or c.shape[1] not in (1, F):
            raise ValueError(f"y_image must be [B, 1, D] or [B, F = {F}, D], got {tuple(y_image.shape)}")
        return (c.expand(-1, F, -1) if c.shape[1] == 1 else c).contiguous()       # unet_dreamvideo.py:270-271

    def _cond_rows(self, c, lams):
        """c [U, F, D] fp32 (the units' y_image), lams: U floats (ag_strength) -> {key: [U, F, hp] fp32}:
        hb = b_down + Wd (lam (Wc c + bc)), util.py:513-515 pushed through down_linear."""
        be = ops.backend()
        U, F, D = c.shape
        out = {}
        groups = {}
        for u, lam in enumerate(lams):                      # units of one ag_strength share their launches
            groups.setdefault(float(lam), []).append(u)
        for e in self._cond_adapters():
            hp = e["wd32"].shape[0]
            hb = torch.empty((U, F, hp), dtype=torch.float32, device=c.device)
            for lam, us in groups.items():
                rows = (c if len(us) == U else c[us]).reshape(len(us) * F, D).contiguous()
                cl = be.linear_f32(rows, e["wc"], e["bc"])
                if lam != 1.0:
                    cl = be.lincomb4(cl, None, None, None, lam, 0.0, 0.0, 0.0)
                r = be.linear_f32(cl, e["wd32"], e["bd32"]).view(len(us), F, hp)
                if len(us) == U:
                    hb = r
                else:
                    hb[us] = r
            out[e["key"]] = hb
        return out

    def _adapt(self, T, slot, tok, M, geom=None):
        e = T.get("ad", {}).get(slot)
        if e is None:
            return tok
        hb, rows_per_hb = e["hb0"], M
        if e["cond"] and self._hb is not None:
            nB, F, S = geom
            t = self._hb[e["key"]]
            assert t.shape[0] >= nB and t.shape[1] == F, (tuple(t.shape), geom)
            hb, rows_per_hb = t[:nB].reshape(nB * F, t.shape[2]), S          # rows are (unit, frame, pixel)
        return ops.backend().adapter(tok, e["wd"], e["wu"], e["bu"], hb, rows_per_hb, e["h"])

    # -- forward -------------------------------------------------------------------------------
    def _prepare_units(self, shape, device, kwargs_list):
        prep = super()._prepare_units(shape, device, kwargs_list)
        if prep is None:
            return None
        have = [kw.get("y_image") is not None for kw in kwargs_list]
        if any(have) and not all(have):
            return None
        if all(have) and self._cond_adapters():
            B, _, F = shape[:3]
            c = torch.cat([self._expand_y_image(kw["y_image"], F, device) for kw in kwargs_list], 0)
            if c.shape[0] != len(kwargs_list) * B:
                return None
            lams = [float(kw.get("ag_strength", 1)) for kw in kwargs_list for _ in range(B)]
            prep["cond"] = (c, lams)
            prep["body"] = {"adapters": self._cond_rows(c, lams)}
        return prep

    @staticmethod
    def shared_prefix_groups(prep, G, B):
        """The first TemporalTransformer sits in the prefix `_body` evaluates once for all G sets: with a motion adapter
        whose condition (y_image, ag_strength) differs between the sets that prefix is NOT shared."""
        g = UNetSD_T2VBase.shared_prefix_groups(prep, G, B)
        cond = prep.get("cond")
        if g > 1 and cond is not None:
            c, lams = cond
            for k in range(1, G):
                if lams[:B] != lams[k * B:(k + 1) * B] or not torch.equal(c[:B], c[k * B:(k + 1) * B]):
                    return 1
        return g

    def _body(self, *args, adapters=None, **kwargs):
        prev = self._hb
        if adapters is not None:
            self._hb = adapters
        try:
            return super()._body(*args, **kwargs)
        finally:
            self._hb = prev

    @torch.no_grad()
    def forward(self, x, t, y=None, y_image=None, fps=None, masked=None, video_mask=None, focus_present_mask=None,
                prob_focus_present=0., mask_last_frame_num=0, ag_strength=1, **kwargs):
        self._maybe_auto_calibrate(tuple(x.shape), x.device, dict(y=y, fps=fps, y_image=y_image, ag_strength=ag_strength),
                                   t.dtype)
        ctx = y if y is not None else self.zero_y.repeat(x.shape[0], 1, 1)[:, :1, :]
        body = None
        if y_image is not None and self._cond_adapters():
            c = self._expand_y_image(y_image, x.shape[2], x.device)
            body = {"adapters": self._cond_rows(c, [float(ag_strength)] * x.shape[0])}
        return self._trunk(x, t, ctx, fps, body_kw=body)
