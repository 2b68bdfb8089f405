"""Native sketch annotator: PiDiNet + sketch simplification (tools/annotator/sketch/pidinet.py,
sketch_simplification.py), the two CNNs behind the `sketch` / `single_sketch` compositions of the VideoComposer configs
(tools/inferences/inference_tft2v_vcomposer_entrance.py:54,319-322,414-435):

    sketch = pidinet(misc_imgs.sub(pidi_mean).div_(pidi_std))
    sketch = 1.0 - cleaner(1.0 - sketch)

`PiDiNet` and `SketchSimplification` are nn.Modules used as parameter containers: state_dict() keys and shapes are those
of the reference's converted models (`pidinet_bsd(vanilla_cnn=True)`, `sketch_simplification_gan()`); forward() runs the
HIP kernels of csrc/sketch.hip and the tap-GEMM through vgen_amd.ops (arithmetic contract: include/vgen_hip.h, "Sketch
annotator").  There is no fallback: CPU tensors go to whatever backend `ops.backend()` holds (the tests' ABI emulator).
"""
from __future__ import annotations

import re

import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .ops import TapGemm
from .unet import _f32, pack_small_conv3x3

__all__ = ["PiDiNet", "SketchSimplification", "pidinet_bsd", "sketch_simplification_gan", "convert_checkpoint",
           "sketch_condition", "install", "pack_deconv4x4"]

CARV4 = ["cd", "ad", "rd", "cv"] * 4          # op of init_block, block1_1..3, block2_1..4, block3_1..4, block4_1..4
_RD_OUTER = [0, 2, 4, 10, 14, 20, 22, 24]     # 5x5 positions that take +w[1..8] of a radial-difference kernel
_RD_INNER = [6, 7, 8, 11, 13, 16, 17, 18]     # ... and -w[1..8]
_AD_SHIFT = [3, 0, 1, 6, 4, 2, 7, 8, 5]       # clockwise neighbour of each 3x3 position (angular difference)


def _pad64(c):
    return (c + 63) // 64 * 64


def _check_hw(x, cin):
    if x.dim() != 4 or x.shape[1] != cin:
        raise ValueError(f"expected [n, {cin}, H, W], got {tuple(x.shape)}")
    H, W = x.shape[2:]
    if H % 8 or W % 8 or H == 0 or W == 0:
        raise ValueError(f"H = {H} and W = {W} must be positive multiples of 8")


# ---- checkpoint conversion -------------------------------------------------------------------------------------------------
def _convert_op(op, w):
    """A pixel-difference conv's weight as the plain conv that computes the same thing (pidinet.py:346-369): central
    difference = the 3x3 kernel minus its sum at the centre; angular = each tap minus its clockwise neighbour; radial = a
    5x5 kernel with +w on the outer ring's 8 compass points and -w on the inner ring."""
    if op == "cv":
        return w
    o, i = w.shape[:2]
    if op == "cd":
        s = w.sum(dim=[2, 3])
        out = w.clone().view(o, i, -1)
        out[:, :, 4] = out[:, :, 4] - s
        return out.view(w.shape)
    flat = w.reshape(o, i, -1)
    if op == "ad":
        return (flat - flat[:, :, _AD_SHIFT]).view(w.shape)
    if op == "rd":
        buf = torch.zeros(o, i, 25, device=w.device)
        buf[:, :, _RD_OUTER] = flat[:, :, 1:]
        buf[:, :, _RD_INNER] = -flat[:, :, 1:]
        return buf.view(o, i, 5, 5)
    raise ValueError(f"unknown pixel-difference op {op!r}")


def _op_index(key):
    """Index into the 16-entry op list of the conv a state-dict key belongs to, or None."""
    if key.endswith("init_block.weight"):
        return 0
    m = re.search(r"block(\d)_(\d)\.conv1\.weight$", key)
    if not m:
        return None
    lvl, k = int(m.group(1)), int(m.group(2))
    return k if lvl == 1 else 4 * (lvl - 1) + (k - 1)


def convert_checkpoint(sd, config="carv4"):
    """State dict of the pixel-difference PiDiNet -> that of its vanilla-CNN form (every other entry passes through)."""
    if config != "carv4":
        raise NotImplementedError(f"convert_checkpoint: only config='carv4' (pidinet_bsd) is supported, got {config!r}")
    out = {}
    for k, v in sd.items():
        i = _op_index(k)
        out[k] = v if i is None else _convert_op(CARV4[i], v)
    return out


# ---- PiDiNet -----------------------------------------------------------------------------------------------------------------
class _BlockP(nn.Module):
    def __init__(self, op, cin, cout, stride=1):
        super().__init__()
        self.stride, self.k, self.cin, self.cout = stride, (5 if op == "rd" else 3), cin, cout
        if stride > 1:
            self.shortcut = nn.Conv2d(cin, cout, 1)
        self.conv1 = nn.Conv2d(cin, cin, self.k, padding=self.k // 2, groups=cin, bias=False)
        self.conv2 = nn.Conv2d(cin, cout, 1, bias=False)


class _CDCMP(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 1)
        for i, d in enumerate((5, 7, 9, 11)):
            setattr(self, f"conv2_{i + 1}", nn.Conv2d(cout, cout, 3, dilation=d, padding=d, bias=False))


class _CSAMP(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv2d(c, 4, 1)
        self.conv2 = nn.Conv2d(4, 1, 3, padding=1, bias=False)


class _MapReduceP(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, 1, 1)


class _Packed:
    """Packed operands of one (dtype, device); dropped when the parameters change."""

    def _init_pack(self, compute_dtype):
        self.compute_dtype = ops.sixteen("fp16" if compute_dtype is None else compute_dtype)
        self._packed = None

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def _ensure_packed(self, device):
        stamp = (self.compute_dtype, str(device))
        if self._packed is None or self._packed["stamp"] != stamp:
            with torch.no_grad():
                self._packed = self.pack()
            self._packed["stamp"] = stamp
        return self._packed


def _rows_padded(w2d, n_pad, k_pad, dt):
    """[N, K] -> zero-padded [n_pad, k_pad] in dt."""
    out = torch.zeros((n_pad, k_pad), dtype=torch.float32, device=w2d.device)
    out[: w2d.shape[0], : w2d.shape[1]] = w2d.detach().float()
    return out.to(dt).contiguous()


def _vec_padded(b, n_pad):
    out = torch.zeros(n_pad, dtype=torch.float32, device=b.device)
    out[: b.shape[0]] = b.detach().float()
    return out


class PiDiNet(_Packed, nn.Module):
    """PiDiNet(60, carv4 converted, dil=24, sa=True) — the model pidinet_bsd(vanilla_cnn=True) builds."""

    def __init__(self, inplane=60, pdcs=None, dil=24, sa=True, convert=True, compute_dtype="fp16"):
        nn.Module.__init__(self)
        pdcs = list(CARV4 if pdcs is None else pdcs)
        if not convert:
            raise NotImplementedError("PiDiNet: convert=False (vanilla_cnn=False, the pixel-difference form) is not supported")
        if list(pdcs) != CARV4 or dil is None or not sa:
            raise NotImplementedError("PiDiNet: only the carv4 configuration with dil and sa (pidinet_bsd) is supported")
        self.inplane, self.dil = inplane, dil
        C = inplane
        self.init_block = nn.Conv2d(3, C, 3, padding=1, bias=False)
        planes = [C, 2 * C, 4 * C, 4 * C]
        self.fuseplanes = planes
        names, i, cin = [], 1, C
        for lvl in range(4):
            for k in range(3 if lvl == 0 else 4):
                first = lvl > 0 and k == 0
                name = f"block{lvl + 1}_{k + 1}"
                setattr(self, name, _BlockP(pdcs[i], cin if first else planes[lvl], planes[lvl], stride=2 if first else 1))
                names.append((lvl, name))
                i += 1
            cin = planes[lvl]
        self._block_names = names
        self.conv_reduces = nn.ModuleList(_MapReduceP(dil) for _ in range(4))
        self.attentions = nn.ModuleList(_CSAMP(dil) for _ in range(4))
        self.dilations = nn.ModuleList(_CDCMP(planes[i], dil) for i in range(4))
        self.classifier = nn.Conv2d(4, 1, 1)
        nn.init.constant_(self.classifier.weight, 0.25)
        nn.init.constant_(self.classifier.bias, 0)
        if dil > 32 or dil % 8:
            raise NotImplementedError("PiDiNet: the side-head kernel holds dil <= 32 channels, a multiple of 8")
        self._init_pack(compute_dtype)

    def pack(self):
        dt = self.compute_dtype
        P = {"blocks": [], "heads": []}
        ib = self.init_block.weight
        kpad = _pad64(27 * 3)
        w = torch.zeros((_pad64(ib.shape[0]), 3, 3, 3), dtype=torch.float32, device=ib.device)
        w[: ib.shape[0]] = ib.detach().float()
        P["stem"] = (pack_small_conv3x3(w, kpad, dt, split=True), kpad)
        for lvl, name in self._block_names:
            m = getattr(self, name)
            cip, cop = _pad64(m.cin), _pad64(m.cout)
            dw = torch.zeros((m.k * m.k, cip), dtype=torch.float32, device=ib.device)
            dw[:, : m.cin] = m.conv1.weight.detach().float().reshape(m.cin, m.k * m.k).t()
            w2 = _rows_padded(m.conv2.weight.reshape(m.cout, m.cin), cop, cip, dt)
            bias = None
            if m.stride > 1:
                w2 = torch.cat([w2, _rows_padded(m.shortcut.weight.reshape(m.cout, m.cin), cop, cip, dt)], 1).contiguous()
                bias = _vec_padded(m.shortcut.bias, cop)
            P["blocks"].append(dict(lvl=lvl, k=m.k, stride=m.stride, cip=cip, cop=cop, dw=dw.contiguous(), w2=w2, bias=bias))
        d = self.dil
        for i in range(4):
            cd, at, mr = self.dilations[i], self.attentions[i], self.conv_reduces[i]
            cp = _pad64(self.fuseplanes[i])
            Wd = torch.zeros((4, 9, 32, 32), dtype=torch.float32, device=ib.device)
            for j in range(4):
                Wd[j, :, :d, :d] = getattr(cd, f"conv2_{j + 1}").weight.detach().float().permute(2, 3, 0, 1).reshape(9, d, d)
            Wa = torch.zeros((4, 32), dtype=torch.float32, device=ib.device)
            Wa[:, :d] = at.conv1.weight.detach().float().reshape(4, d)
            P["heads"].append(dict(
                cp=cp, w1=_rows_padded(cd.conv1.weight.reshape(d, -1), 32, cp, dt), b1=_vec_padded(cd.conv1.bias, 32),
                Wd=Wd.to(dt).contiguous(), Wa=Wa.contiguous(), ba=_f32(at.conv1.bias), wr=_vec_padded(mr.conv.weight.reshape(d), 32),
                w2=at.conv2.weight.detach().float()[0].permute(1, 2, 0).reshape(9, 4).contiguous(), br=float(mr.conv.bias)))
        P["wc"] = [float(v) for v in self.classifier.weight.detach().float().reshape(4)]
        P["bc"] = float(self.classifier.bias)
        return P

    @torch.no_grad()
    def forward(self, x):
        """x [n, 3, H, W] fp32, already normalised -> edge probability [n, 1, H, W] fp32 in (0, 1)."""
        _check_hw(x, 3)
        P = self._ensure_packed(x.device)
        be, dt = ops.backend(), self.compute_dtype
        n, _, H, W = x.shape
        x = x.float().contiguous()
        Ws, kpad = P["stem"]
        col = be.im2col3x3_small(x, n, 1, 3, H, W, (3 * H * W, 0, H * W, W, 1), kpad, dt, split=True)
        s = be.tapgemm(TapGemm(A=col, W=Ws, M=n * H * W, N=Ws.shape[0], C1=kpad))
        h, w = H, W
        es = []
        for bi, b in enumerate(P["blocks"]):
            if b["stride"] > 1:
                _, xp16, y16 = be.dwconv_relu(s, n, h, w, b["dw"], b["k"], dt, pool=True)
                h, w = h // 2, w // 2
                s = be.tapgemm(TapGemm(A=y16, W=b["w2"], M=n * h * w, N=b["cop"], C1=b["cip"], A2=xp16, C2=b["cip"], bias=b["bias"]))
            else:
                y16 = be.dwconv_relu(s, n, h, w, b["dw"], b["k"], dt)
                s = be.tapgemm(TapGemm(A=y16, W=b["w2"], M=n * h * w, N=b["cop"], C1=b["cip"], residual=s))
            last = bi + 1 == len(P["blocks"]) or P["blocks"][bi + 1]["lvl"] != b["lvl"]
            if last:
                hd = P["heads"][b["lvl"]]
                r16 = be.dwconv_relu(s, n, h, w, None, 1, dt)
                t = be.tapgemm(TapGemm(A=r16, W=hd["w1"], M=n * h * w, N=32, C1=hd["cp"], bias=hd["b1"], out_dtype=dt))
                mr = be.cdcm_head(t, n, h, w, hd["Wd"], hd["Wa"], hd["ba"], hd["wr"])
                es.append(be.pidinet_emap(mr, n, h, w, hd["w2"], hd["br"]))
        return be.pidinet_fuse(es, n, H, W, P["wc"], P["bc"])


# ---- sketch simplification -----------------------------------------------------------------------------------------------------
# (kind, cin, cout, kernel, stride) of layers.0, layers.2, ... (a ReLU follows each but the last, which ends in a sigmoid)
_CLEANER = [("conv", 1, 48, 5, 2), ("conv", 48, 128, 3, 1), ("conv", 128, 128, 3, 1), ("conv", 128, 128, 3, 2),
            ("conv", 128, 256, 3, 1), ("conv", 256, 256, 3, 1), ("conv", 256, 256, 3, 2), ("conv", 256, 512, 3, 1),
            ("conv", 512, 1024, 3, 1), ("conv", 1024, 1024, 3, 1), ("conv", 1024, 1024, 3, 1), ("conv", 1024, 1024, 3, 1),
            ("conv", 1024, 512, 3, 1), ("conv", 512, 256, 3, 1), ("deconv", 256, 256, 4, 2), ("conv", 256, 256, 3, 1),
            ("conv", 256, 128, 3, 1), ("deconv", 128, 128, 4, 2), ("conv", 128, 128, 3, 1), ("conv", 128, 48, 3, 1),
            ("deconv", 48, 48, 4, 2), ("conv", 48, 24, 3, 1), ("conv", 24, 1, 3, 1)]


def pack_deconv4x4(wt, cp):
    """ConvTranspose2d(C, C, 4, 2, 1).weight [ci, co, 4, 4] -> fp32 [4 cp, 9 cp]: row (py * 2 + px) * cp + co, column
    ((dy + 1) * 3 + (dx + 1)) * cp + ci = wt[ci, co, py + 1 - 2 dy, px + 1 - 2 dx] where that index is in 0..3, else 0 — the
    3x3 / stride-1 / pad-1 conv whose 4 cp output columns are the four output-pixel parities (include/vgen_hip.h)."""
    ci, co = wt.shape[:2]
    out = torch.zeros((2, 2, cp, 3, 3, cp), dtype=torch.float32, device=wt.device)
    w = wt.detach().float()
    for py in range(2):
        for px in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ky, kx = py + 1 - 2 * dy, px + 1 - 2 * dx
                    if 0 <= ky < 4 and 0 <= kx < 4:
                        out[py, px, :co, dy + 1, dx + 1, :ci] = w[:, :, ky, kx].t()
    return out.reshape(4 * cp, 9 * cp)


class SketchSimplification(_Packed, nn.Module):
    """Input / output [n, 1, H, W] in [0, 1], sketch lines dark; H and W multiples of 8."""

    def __init__(self, mean, std, compute_dtype="fp16"):
        assert isinstance(mean, float) and isinstance(std, float)
        nn.Module.__init__(self)
        self.mean, self.std = mean, std
        mods = []
        for i, (kind, cin, cout, k, s) in enumerate(_CLEANER):
            mods.append(nn.Conv2d(cin, cout, k, s, k // 2) if kind == "conv" else nn.ConvTranspose2d(cin, cout, k, s, 1))
            mods.append(nn.ReLU(inplace=True) if i + 1 < len(_CLEANER) else nn.Sigmoid())
        self.layers = nn.Sequential(*mods)
        self._init_pack(compute_dtype)

    def pack(self):
        dt = self.compute_dtype
        P = {"convs": []}
        for i, (kind, cin, cout, k, s) in enumerate(_CLEANER):
            m = self.layers[2 * i]
            cip, cop = _pad64(cin), _pad64(cout)
            if i == 0:
                w = torch.zeros((25, cop), dtype=torch.float32, device=m.weight.device)
                w[:, :cout] = m.weight.detach().float().reshape(cout, 25).t()
                P["stem"] = (w.contiguous(), _vec_padded(m.bias, cop))
            elif i + 1 == len(_CLEANER):
                P["head"] = (m.weight.detach().float()[0].permute(1, 2, 0).reshape(9, cin).contiguous(), float(m.bias), cin)
            elif kind == "conv":
                w = torch.zeros((cop, 3, 3, cip), dtype=torch.float32, device=m.weight.device)
                w[:cout, :, :, :cin] = m.weight.detach().float().permute(0, 2, 3, 1)
                P["convs"].append(dict(kind=kind, W=w.reshape(cop, 9 * cip).to(dt).contiguous(), b=_vec_padded(m.bias, cop),
                                       cip=cip, cop=cop, stride=s))
            else:
                P["convs"].append(dict(kind=kind, W=pack_deconv4x4(m.weight, cop).to(dt).contiguous(),
                                       b=_vec_padded(m.bias, cop).repeat(4).contiguous(), cip=cip, cop=cop, stride=1))
        return P

    @torch.no_grad()
    def forward(self, x, flip_in=False, flip_out=False):
        """x [n, 1, H, W] -> [n, 1, H, W] fp32.  flip_in / flip_out: evaluate 1 - net(1 - x) with both `1 - .` inside the
        first and the last kernel (sketch_condition)."""
        _check_hw(x, 1)
        P = self._ensure_packed(x.device)
        be, dt = ops.backend(), self.compute_dtype
        n, _, H, W = x.shape
        a = be.sketch_stem(x.float().contiguous(), flip_in, self.mean, self.std, *P["stem"], dt)
        h, w = H // 2, W // 2
        for c in P["convs"]:
            ho, wo = (h // 2, w // 2) if c["stride"] == 2 else (h, w)
            nout = c["W"].shape[0]
            a = be.tapgemm(TapGemm(A=a, W=c["W"], M=n * ho * wo, N=nout, C1=c["cip"], mode=L.TAP_CONV3X3, taps=9, Hi=h, Wi=w,
                                   Ho=ho, Wo=wo, stride=c["stride"], pad_t=1, pad_l=1, bias=c["b"], out_dtype=dt))
            if c["kind"] == "deconv":
                a = be.relu_shuffle16(a, c["cop"], 2, ho, wo)
                ho, wo = 2 * ho, 2 * wo
            else:
                a = be.relu_shuffle16(a, nout)
            h, w = ho, wo
        wh, bh, ch = P["head"]
        return be.sketch_head(a, n, H, W, ch, wh, bh, flip_out)


# ---- factories (the reference's signatures) ----------------------------------------------------------------------------------
def pidinet_bsd(pretrained=False, vanilla_cnn=True, compute_dtype="fp16"):
    if not vanilla_cnn:
        raise NotImplementedError("pidinet_bsd: vanilla_cnn=False (the unconverted pixel-difference model) is not supported; "
                                  "every engine builds it with vanilla_cnn=True")
    model = PiDiNet(60, CARV4, dil=24, sa=True, convert=True, compute_dtype=compute_dtype)
    if pretrained:
        state = torch.load("models/table5_pidinet.pth", map_location="cpu")["state_dict"]
        state = convert_checkpoint(state, "carv4")
        state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}
        model.load_state_dict(state)
    return model


def sketch_simplification_gan(pretrained=False, compute_dtype="fp16"):
    model = SketchSimplification(mean=0.9664114577640158, std=0.0858381272736797, compute_dtype=compute_dtype)
    if pretrained:
        model.load_state_dict(torch.load("models/sketch_simplification_gan.pth", map_location="cpu"))
    return model


@torch.no_grad()
def sketch_condition(frames, pidinet, cleaner, mean, std):
    """frames [n, 3, H, W] in [0, 1] -> sketch [n, 1, H, W]: the engine's two lines as one call.  mean / std: the PiDiNet
    input normalisation (cfg.sketch_mean / sketch_std; tensors broadcastable to frames, or 3 numbers).  Both `1 - .` and the
    cleaner's own normalisation run inside its first and last kernel: no elementwise torch op between the two nets."""
    mean = torch.as_tensor(mean, dtype=torch.float32, device=frames.device).reshape(1, -1, 1, 1)
    std = torch.as_tensor(std, dtype=torch.float32, device=frames.device).reshape(1, -1, 1, 1)
    edge = pidinet(frames.float().sub(mean).div_(std))
    return cleaner(edge, flip_in=True, flip_out=True)


def install():
    """Rebind `pidinet_bsd` and `sketch_simplification_gan` to the native factories in the reference's
    `tools.annotator.sketch` package and in every already-imported `tools.inferences.*` module that holds those names
    (the engines import them directly, with no registry in between).  Returns the list of (module name, attribute)
    rebindings; does nothing when the package is not importable."""
    import importlib
    import sys
    try:
        pkg = importlib.import_module("tools.annotator.sketch")
    except Exception:
        return []
    native = {"pidinet_bsd": pidinet_bsd, "sketch_simplification_gan": sketch_simplification_gan}
    done = []
    mods = [pkg] + [m for name, m in sorted(sys.modules.items()) if name.startswith("tools.inferences.") and m is not None]
    for m in mods:
        for attr, fn in native.items():
            if hasattr(m, attr):
                setattr(m, attr, fn)
                done.append((m.__name__, attr))
    return done
