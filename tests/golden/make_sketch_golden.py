"""Golden fixtures of the sketch annotator (vgen_amd/sketch.py), computed by the reference's own classes
(tools/annotator/sketch/pidinet.py, sketch_simplification.py) on the CPU in fp32.

Both reference files import nothing but torch; they are loaded by path at run time.  Weights: vgen_amd.synth.
seeded_state_dict over the reference's converted key shapes — PiDiNet gain 1.0 (seed 3), cleaner gain sqrt(2) (seed 4): the
default gain 0.8 lets the signal die in the cleaner's 26 norm-free ReLU layers (two different images then differ by 9e-8),
and sqrt(2) on PiDiNet saturates 80 % of the pixels.  Inputs are smoothed uniform noise in [0, 1].  The fixtures store
shapes, seeds, gains, the input seed and the fp32 outputs — no weights, no program text — plus the reference's OWN autocast
deviation on the same evaluations under "yardstick" (the project's tolerance base, like the DreamVideo fixtures).

Per evaluation i (frames [n, 3, H, W] in [0, 1]):
  edge    = pidinet((frames - mean) / std)                       the engine's first line
  sketch  = 1 - cleaner(1 - edge)                                its second line, chained in fp32
  edge16  = edge rounded to fp16 (exactly representable in fp32): the stored INPUT of the cleaner-only evaluation
  clean   = 1 - cleaner(1 - edge16.float())                      the cleaner alone, from a stored input
  convert_sha256: digest of the reference's convert_pidinet on raw_pidinet_state(shapes) (tests compare bit for bit).
  yardstick "i/edge/<dt>", "i/sketch/<dt>" (chained), "i/clean/<dt>" (cleaner alone): rel-L2 of the same evaluation under
  torch.autocast("cpu", <dt>) against fp32.
The full fixture keeps every `sub_step`-th row of edge / sketch and every `row_step`-th of clean (plus the norms of the whole
maps), so the file stays under 1 MiB.  The yardsticks are taken over EXACTLY the stored rows, so a test compares like with
like, and the steps are coprime to 8: the error is not uniform over rows — the reference's own fp16 autocast run deviates by
7.9e-4 over all rows of the full sketch but by 1.15e-3 over rows = 0 mod 4 or mod 8 (the parity pattern of the three
transposed convs) — so a power-of-two row step against a whole-map yardstick would compare two different statistics.  The
whole-map figures are kept under "yardstick_all_rows" for information.

A recipe change cannot silently empty the test: the generator asserts logit std in [0.5, 3], saturated share < 0.25 and
input sensitivity (rel-L2 between the sketches of the two images of a batch) > 0.1.

    python tests/golden/make_sketch_golden.py [tiny] [full]
"""
from __future__ import annotations

import importlib.util
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SKETCH_MEAN, SKETCH_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # tools/modules/config.py:81-82
COMMON = dict(pidi_seed=3, pidi_gain=1.0, cleaner_seed=4, cleaner_gain=math.sqrt(2.0), mean=SKETCH_MEAN, std=SKETCH_STD)
CASES = {
    # 40 x 72: the 1/8 level is 5 x 9, smaller than every dilation of the side heads
    "tiny": dict(COMMON, input_seed=9200, evals=[(2, 3, 40, 72), (2, 3, 64, 96)], row_step=1, sub_step=1),
    "full": dict(COMMON, input_seed=9201, evals=[(2, 3, 256, 448)], row_step=5, sub_step=7),
}


def _load(name):
    from oracle.ref_import import REF
    mod = "vgen_ref_sketch_" + name
    if mod not in sys.modules:
        spec = importlib.util.spec_from_file_location(mod, os.path.join(REF, "tools", "annotator", "sketch", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[mod] = m
        spec.loader.exec_module(m)
    return sys.modules[mod]


def reference_models(case):
    """(pidinet, cleaner): the reference's classes with the case's seeded weights, plus their key shapes."""
    from vgen_amd.synth import seeded_state_dict
    pidi = _load("pidinet").pidinet_bsd(pretrained=False, vanilla_cnn=True).eval()
    clean = _load("sketch_simplification").sketch_simplification_gan(pretrained=False).eval()
    shapes = {}
    for tag, m, seed, gain in (("pidinet", pidi, case["pidi_seed"], case["pidi_gain"]),
                               ("cleaner", clean, case["cleaner_seed"], case["cleaner_gain"])):
        shapes[tag] = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict(seeded_state_dict(shapes[tag], seed=seed, gain=gain), strict=True)
    return pidi, clean, shapes


def inputs(case, i):
    """frames [n, 3, H, W] in [0, 1] of evaluation i — tests call this with the stored case."""
    n, c, H, W = case["evals"][i]
    g = torch.Generator("cpu").manual_seed(case["input_seed"] + i)
    r = torch.rand(n, c, H, W, generator=g)
    return F.avg_pool2d(r, 5, 1, 2) * 0.5 + 0.5 * torch.rand(n, c, 1, 1, generator=g)


def raw_pidinet_state(shapes, seed=11):
    """A seeded UNCONVERTED pixel-difference state dict with `module.` prefixes, as models/table5_pidinet.pth holds it: the
    converted key shapes with every 5 x 5 (radial-difference) kernel back at its 3 x 3 parameter shape."""
    from vgen_amd.synth import seeded_state_dict
    raw = {"module." + k: (tuple(v[:2]) + (3, 3) if len(v) == 4 and v[2] == 5 else tuple(v)) for k, v in shapes.items()}
    return seeded_state_dict(raw, seed=seed)


def digest(sd):
    """sha256 over the fp32 bytes of a state dict, keys in sorted order."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().float().contiguous().numpy().tobytes())
    return h.hexdigest()


def _rel(a, b):
    return float((a.float() - b).norm() / b.norm())


@torch.no_grad()
def make(name):
    case = CASES[name]
    pidi, clean, shapes = reference_models(case)
    mean = torch.tensor(case["mean"]).view(1, -1, 1, 1)
    std = torch.tensor(case["std"]).view(1, -1, 1, 1)
    outs, yard, yard_all = [], {}, {}
    rs, ss = case["row_step"], case["sub_step"]
    for i in range(len(case["evals"])):
        x = inputs(case, i)
        xn = (x - mean) / std
        t0 = time.time()
        edge = pidi(xn)
        sketch = 1.0 - clean(1.0 - edge)
        edge16 = edge.half()
        cl = 1.0 - clean(1.0 - edge16.float())
        print(name, i, tuple(x.shape), "fp32 %.1f s" % (time.time() - t0), flush=True)
        logit = torch.logit(edge.double())
        lstd = float(logit.std())
        sat = float(((edge < 0.02) | (edge > 0.98)).float().mean())
        sens = _rel(sketch[0], sketch[1])
        print(name, i, "logit std %.3f saturated %.3f sensitivity %.3f" % (lstd, sat, sens), flush=True)
        assert 0.5 <= lstd <= 3.0, lstd
        assert sat < 0.25, sat
        assert sens > 0.1, sens
        assert _rel(cl[0], cl[1]) > 0.1
        for dn, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            t0 = time.time()
            with torch.autocast("cpu", dtype=dt):
                e = pidi(xn).float()
                s = 1.0 - clean(1.0 - e).float()
                c = 1.0 - clean(1.0 - edge16.float()).float()
            for tag, a, b, st in (("edge", e, edge, ss), ("sketch", s, sketch, ss), ("clean", c, cl, rs)):
                yard[f"{i}/{tag}/{dn}"] = _rel(a[:, :, ::st], b[:, :, ::st])
                yard_all[f"{i}/{tag}/{dn}"] = _rel(a, b)
            print(name, i, dn, {k: "%.3e" % v for k, v in yard.items() if k.startswith(f"{i}/") and k.endswith(dn)},
                  "%.1f s" % (time.time() - t0), flush=True)
        outs.append(dict(edge16=edge16.contiguous(),
                         edge=edge[:, :, ::ss].contiguous(), edge_norm=float(edge.norm()),
                         sketch=sketch[:, :, ::ss].contiguous(), sketch_norm=float(sketch.norm()),
                         clean=cl[:, :, ::rs].contiguous(), clean_norm=float(cl.norm()),
                         logit_std=lstd, saturated=sat, sensitivity=sens))
    # the reference's own conversion of a seeded raw checkpoint (pidinet.py:371-409), as a digest
    raw = raw_pidinet_state(shapes["pidinet"])
    conv = _load("pidinet").convert_pidinet({k: v.clone() for k, v in raw.items()}, "carv4")
    assert {k[len("module."):]: tuple(v.shape) for k, v in conv.items()} == shapes["pidinet"]
    path = os.path.join(HERE, f"sketch_{name}.pt")
    torch.save(dict(case, shapes=shapes, outs=outs, yardstick=yard, yardstick_all_rows=yard_all, convert_sha256=digest(conv)), path)
    print(path, os.path.getsize(path), "bytes", flush=True)
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    for n_ in (sys.argv[1:] or list(CASES)):
        make(n_)
