"""Golden fixtures of FrozenOpenCLIPTextVisualEmbedder (vgen_amd/clip_visual.py), computed by the reference tree's OWN copy of
open_clip 2.x (utils/reward/open_clip/, version 2.16.0) — the package the reference's clip_embedder.py imports but does
not pin — so that both CLIP towers are pinned to open_clip code rather than to a restatement in this repository.

Loading that copy on a CPU box without torchvision: its utils.py imports torchvision.ops.misc.FrozenBatchNorm2d (used only
by ResNet towers), so a stub module stands in for it while the package loads (with `__spec__` set on every stub module:
transformers, which hf_model.py imports, looks that attribute up); and the package's modules are loaded from that
directory under a private package name without running its __init__.py, which imports torchvision's transforms.  The
stubs are removed from sys.modules again afterwards.

Weights: vgen_amd.synth.seeded_state_dict over the EMBEDDER's own key names (`model.` prefix included — the seeded draws
follow the sorted key names, so a test that knows the seed rebuilds the same weights from the embedder alone), loaded
into the fork's CLIP with the prefix stripped.  The forward restates clip_embedder.py:183-213 (forward, encode_with_
transformer, text_transformer_forward) around the fork's modules.  The fixtures store seeds and token ids; images come
from a CPU generator.

    python tests/golden/make_clip_golden.py [REFERENCE_ROOT]     # writes clip_visual_tiny.pt and clip_visual_full.pt
"""
from __future__ import annotations

import importlib
import importlib.machinery
import os
import sys
import types

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TINY_TEXT = dict(vocab=300, ctx=20, width=128, layers=3, heads=2, embed_dim=64)      # tests/test_clip_text.py TINY
TINY_VISION = dict(image_size=224, patch_size=14, width=320, layers=2, head_width=80)  # 4 heads of 80, 257 tokens
CASES = {
    "tiny": dict(text_cfg=TINY_TEXT, vision_cfg=TINY_VISION, seed=11, B=2, image_seed=3, token_seed=1),
    "full": dict(text_cfg=None, vision_cfg=None, seed=21, B=2, image_seed=4, token_seed=2),
}
LAYER = "penultimate"                  # what every stock config asks for


def load_fork(ref):
    """The fork's open_clip `model` module, loaded from <ref>/utils/reward/open_clip without its __init__.py."""
    pkg_dir = os.path.join(ref, "utils", "reward", "open_clip")
    name = "_ref_open_clip"
    if name + ".model" in sys.modules:
        return sys.modules[name + ".model"]
    stubs = {}
    for mod in ("torchvision", "torchvision.ops", "torchvision.ops.misc"):
        if mod not in sys.modules:
            m = types.ModuleType(mod)
            m.__spec__ = importlib.machinery.ModuleSpec(mod, None)
            stubs[mod] = m
    if stubs:
        class FrozenBatchNorm2d(nn.Module):            # never instantiated by a ViT tower
            pass
        stubs.get("torchvision.ops.misc", types.SimpleNamespace()).FrozenBatchNorm2d = FrozenBatchNorm2d
        sys.modules.update(stubs)
    try:
        pkg = types.ModuleType(name)
        pkg.__path__ = [pkg_dir]
        pkg.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        pkg.__spec__.submodule_search_locations = [pkg_dir]
        sys.modules[name] = pkg
        return importlib.import_module(name + ".model")
    finally:
        for mod in stubs:
            sys.modules.pop(mod, None)


def fork_clip(model_mod, text_cfg, vision_cfg):
    """The fork's CLIP for our config dicts (vgen_amd.clip_text / clip_visual naming)."""
    t, v = text_cfg, vision_cfg
    vc = model_mod.CLIPVisionCfg(layers=v["layers"], width=v["width"], head_width=v["head_width"],
                                 patch_size=v["patch_size"], image_size=v["image_size"])
    tc = model_mod.CLIPTextCfg(context_length=t["ctx"], vocab_size=t["vocab"], width=t["width"], heads=t["heads"],
                               layers=t["layers"])
    return model_mod.CLIP(embed_dim=t["embed_dim"], vision_cfg=vc, text_cfg=tc).eval()


def embedder(case):
    from vgen_amd.clip_visual import FrozenOpenCLIPTextVisualEmbedder
    return FrozenOpenCLIPTextVisualEmbedder(text_cfg=case["text_cfg"], vision_cfg=case["vision_cfg"], layer=LAYER)


def weights(emb, seed):
    from vgen_amd.synth import seeded_state_dict
    return seeded_state_dict({k: tuple(v.shape) for k, v in emb.state_dict().items()}, seed=seed)


def inputs(cfg_text, cfg_vision, B, image_seed, token_seed):
    g = torch.Generator("cpu").manual_seed(image_seed)
    S = cfg_vision["image_size"]
    img = torch.randn((B, 3, S, S), generator=g)                    # already-normalised images
    g = torch.Generator("cpu").manual_seed(token_seed)
    tok = torch.randint(1, cfg_text["vocab"] - 2, (B, cfg_text["ctx"]), generator=g)
    for b in range(B):                                              # an EOT (largest id) somewhere, zeros after it
        e = 3 + 5 * b
        tok[b, e] = cfg_text["vocab"] - 1
        tok[b, e + 1:] = 0
    return img, tok


@torch.no_grad()
def reference_forward(model, image, tokens, layer_idx):
    """clip_embedder.py:183-213 around the fork's CLIP: (xi, xt, x)."""
    xi = model.encode_image(image)
    x = model.token_embedding(tokens) + model.positional_embedding
    x = x.permute(1, 0, 2)
    for i, r in enumerate(model.transformer.resblocks):
        if i == len(model.transformer.resblocks) - layer_idx:
            break
        x = r(x, attn_mask=model.attn_mask)
    x = model.ln_final(x.permute(1, 0, 2))
    xt = x[torch.arange(x.shape[0]), tokens.argmax(dim=-1)] @ model.text_projection
    return xi, xt, x


def make(name, ref):
    from vgen_amd.clip_text import ARCHS
    from vgen_amd.clip_visual import VISION_ARCHS
    case = dict(CASES[name])
    case["text_cfg"] = case["text_cfg"] or ARCHS["ViT-H-14"]
    case["vision_cfg"] = case["vision_cfg"] or VISION_ARCHS["ViT-H-14"]
    emb = embedder(case)
    sd = weights(emb, case["seed"])
    model = fork_clip(load_fork(ref), case["text_cfg"], case["vision_cfg"])
    model.load_state_dict({k[len("model."):]: v for k, v in sd.items()}, strict=True)
    img, tok = inputs(case["text_cfg"], case["vision_cfg"], case["B"], case["image_seed"], case["token_seed"])
    xi, xt, x = reference_forward(model, img, tok, 1 if LAYER == "penultimate" else 0)
    out = dict(case, layer=LAYER, tokens=tok, xi=xi.float().contiguous(), xt=xt.float().contiguous(),
               x=x.float().contiguous(), open_clip="reference utils/reward/open_clip 2.16.0")
    path = os.path.join(HERE, f"clip_visual_{name}.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes", {k: tuple(v.shape) for k, v in out.items() if torch.is_tensor(v)})


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from oracle.ref_import import REF
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    for n in CASES:
        make(n, ref)
