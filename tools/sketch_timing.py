"""Timing of the native sketch annotator (vgen_amd/sketch.py) against torch-ROCm's eager fp16 evaluation of the same two
nets, on the workload of the VideoComposer configs: 32 frames of 256 x 448 in chunks of 2 (the yaml's chunk_size) and of 16.

    python tools/sketch_timing.py [--out profiles/sketch_annotator_timing.json] [--frames 32] [--min-seconds 1.0]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sketch_timing.py --profile-pass      (per-kernel split)

Same process, same seeded weights (vgen_amd.synth, the golden fixtures' recipe), the two paths alternated window by window;
every window is warmed up first, ends in a device synchronise and lasts at least --min-seconds.  The composed path is a
plain-torch restatement of the two nets (F.conv2d / max_pool2d / interpolate on the native modules' own parameters, cast to
fp16).  Reported per net: time per 32 frames, and the rate the ALGORITHM needs computed from shapes — FLOP/s for the cleaner
(dense 3x3 convs), bytes/s of fp32 stream traffic for PiDiNet (depthwise, memory-bound) — with the roof that bounds it.
There is no pass / fail threshold: what is slower than the composed path is reported as plainly as what is faster.
A run without a GPU fails; it does not fall back.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FLOPS_16 = 2.5e15          # dense fp16 / bf16 MFMA, spec
PEAK_HBM = 8.0e12               # spec; ~6.3e12 achievable
H, W = 256, 448


# ---- work from shapes ----------------------------------------------------------------------------------------------------------
def cleaner_flop(n, h, w):
    """Algorithmic FLOP of the sketch-simplification net on n images (2 * MACs of every layer; ConvTranspose2d counted at its
    own 4 taps per output pixel, not at the 9 the packed form executes)."""
    from vgen_amd.sketch import _CLEANER
    total, ch, cw = 0.0, h, w
    for kind, cin, cout, k, s in _CLEANER:
        if kind == "conv":
            ch, cw = ch // s, cw // s
            total += 2.0 * ch * cw * cin * cout * k * k
        else:
            ch, cw = ch * 2, cw * 2
            total += 2.0 * ch * cw * cin * cout * 4
    return total * n


def pidinet_bytes(n, h, w):
    """fp32 stream traffic of PiDiNet on n images if every block read its input once (4 B), wrote the 16-bit depthwise result
    and read it back (2 + 2 B), read the residual (4 B) and wrote its output (4 B) — per pixel and REAL channel; plus the side
    heads' read of each level's output and the 16-bit t rows."""
    total, c = 0.0, 60
    ch, cw = h, w
    total += ch * cw * (3 * 4 + 60 * 4)
    for lvl, (cout, blocks) in enumerate(((60, 3), (120, 4), (240, 4), (240, 4))):
        if lvl:
            total += ch * cw * c * 4                  # the pool's read of the previous level
            ch, cw = ch // 2, cw // 2
        for _ in range(blocks):
            total += ch * cw * (c * (4 + 2 + 2 + 4) + cout * 4)
            c = cout
        total += ch * cw * (c * 4 + 24 * 2 * 2 + 5 * 4 * 2 + 4)
    total += h * w * 4
    return total * n


# ---- the composed path: plain torch on the same parameters ------------------------------------------------------------------------
def torch_pidinet(sd, x):
    Hh, Ww = x.shape[2:]
    s = F.conv2d(x, sd["init_block.weight"], padding=1)
    es = []
    for lvl in range(4):
        for k in range(1, 4 if lvl == 0 else 5):
            p = f"block{lvl + 1}_{k}."
            if p + "shortcut.weight" in sd:
                s = F.max_pool2d(s, 2, 2)
            w1 = sd[p + "conv1.weight"]
            y = F.conv2d(torch.relu(F.conv2d(s, w1, padding=w1.shape[-1] // 2, groups=w1.shape[0])), sd[p + "conv2.weight"])
            s = y + (F.conv2d(s, sd[p + "shortcut.weight"], sd[p + "shortcut.bias"]) if p + "shortcut.weight" in sd else s)
        d = f"dilations.{lvl}."
        t = F.conv2d(torch.relu(s), sd[d + "conv1.weight"], sd[d + "conv1.bias"])
        u = sum(F.conv2d(t, sd[d + f"conv2_{j + 1}.weight"], padding=dl, dilation=dl) for j, dl in enumerate((5, 7, 9, 11)))
        a = f"attentions.{lvl}."
        yy = torch.sigmoid(F.conv2d(F.conv2d(torch.relu(u), sd[a + "conv1.weight"], sd[a + "conv1.bias"]), sd[a + "conv2.weight"], padding=1))
        e = F.conv2d(u * yy, sd[f"conv_reduces.{lvl}.conv.weight"], sd[f"conv_reduces.{lvl}.conv.bias"])
        es.append(F.interpolate(e, (Hh, Ww), mode="bilinear", align_corners=False))
    return torch.sigmoid(F.conv2d(torch.cat(es, 1), sd["classifier.weight"], sd["classifier.bias"]))


def torch_cleaner(layers, mean, std, x):
    return layers((x - mean) / std)


# ---- timing ----------------------------------------------------------------------------------------------------------------------
def window(fn, min_seconds):
    """(seconds per call, calls) over a device-synchronised window of at least min_seconds."""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 2 == 0 or calls == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_annotator_timing.json"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile-pass", action="store_true", help="one warmed native pass per chunk size, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sketch_timing: no GPU; a timing taken elsewhere says nothing (not measured)")
    from vgen_amd import ops, sketch
    from vgen_amd.synth import seeded_state_dict, shapes_of
    dev = "cuda:0"
    pidi, clean = sketch.pidinet_bsd(), sketch.sketch_simplification_gan()
    pidi.load_state_dict(seeded_state_dict(shapes_of(pidi), seed=3, gain=1.0))
    clean.load_state_dict(seeded_state_dict(shapes_of(clean), seed=4, gain=2.0 ** 0.5))
    pidi, clean = pidi.to(dev).eval(), clean.to(dev).eval()
    sd16 = {k: v.half() for k, v in pidi.state_dict().items()}
    layers16 = copy.deepcopy(clean.layers).half()
    g = torch.Generator("cpu").manual_seed(9300)
    frames = (F.avg_pool2d(torch.rand(a.frames, 3, H, W, generator=g), 5, 1, 2) * 0.5
              + 0.5 * torch.rand(a.frames, 3, 1, 1, generator=g)).to(dev)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    xn = (frames - mean) / std
    assert ops.backend().name == "hip"
    res = {"workload": dict(frames=a.frames, H=H, W=W), "peaks": dict(flops_16bit=PEAK_FLOPS_16, hbm=PEAK_HBM), "chunks": {}}
    with torch.no_grad():
        edge_all = torch.cat([pidi(xn[i:i + 2]) for i in range(0, a.frames, 2)])
        for chunk in (2, 16):
            idx = range(0, a.frames, chunk)
            paths = {
                "native/pidinet": lambda: [pidi(xn[i:i + chunk]) for i in idx],
                "native/cleaner": lambda: [clean(edge_all[i:i + chunk], flip_in=True, flip_out=True) for i in idx],
                "native/both": lambda: [sketch.sketch_condition(frames[i:i + chunk], pidi, clean, mean, std) for i in idx],
                "torch_fp16/pidinet": lambda: [torch_pidinet(sd16, xn[i:i + chunk].half()) for i in idx],
                "torch_fp16/cleaner": lambda: [1.0 - torch_cleaner(layers16, clean.mean, clean.std, 1.0 - edge_all[i:i + chunk].half())
                                               for i in idx],
            }
            if a.profile_pass:
                for k in ("native/pidinet", "native/cleaner"):
                    paths[k]()
                    torch.cuda.synchronize()
                    paths[k]()
                    torch.cuda.synchronize()
                continue
            # parity of the two paths at the size that is timed
            nat = torch.cat(paths["native/both"]())
            comp = torch.cat([1.0 - torch_cleaner(layers16, clean.mean, clean.std, 1.0 - torch_pidinet(sd16, xn[i:i + chunk].half()))
                              for i in idx]).float()
            parity = float((nat - comp).norm() / comp.norm())
            times = {k: [] for k in paths}
            for _ in range(a.rounds):                       # alternate the paths, round by round
                for k, fn in paths.items():
                    times[k].append(window(fn, a.min_seconds)[0])
            out = {"native_vs_torch_fp16_rel_l2": parity}
            fl, by = cleaner_flop(a.frames, H, W), pidinet_bytes(a.frames, H, W)
            for k, ts in times.items():
                t = min(ts)
                e = dict(seconds_per_32_frames=t * 32.0 / a.frames, windows=[round(v, 6) for v in ts])
                if k.endswith("cleaner"):
                    e.update(algorithmic_flop=fl, flop_per_s=fl / t, share_of_16bit_matrix_peak=fl / t / PEAK_FLOPS_16,
                             least_time_s=max(fl / PEAK_FLOPS_16, 0.0), bound="compute (dense 3x3 convs on the matrix units)")
                if k.endswith("pidinet"):
                    e.update(algorithmic_bytes=by, bytes_per_s=by / t, share_of_hbm_peak=by / t / PEAK_HBM,
                             least_time_s=by / PEAK_HBM, bound="memory (depthwise convs, fp32 stream)")
                out[k] = e
            for net in ("pidinet", "cleaner"):
                out[f"speedup/{net}"] = out[f"torch_fp16/{net}"]["seconds_per_32_frames"] / out[f"native/{net}"]["seconds_per_32_frames"]
            res["chunks"][str(chunk)] = out
            print(chunk, json.dumps({k: (round(v["seconds_per_32_frames"] * 1e3, 2) if isinstance(v, dict) else round(v, 4))
                                     for k, v in out.items()}), flush=True)
    if not a.profile_pass:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
