"""FrozenOpenCLIPTextVisualEmbedder — the OpenCLIP ViT-H/14 text AND image towers on the C ABI (the embedder every stock
config names: configs/*.yaml `embedder: {type: FrozenOpenCLIPTextVisualEmbedder, ...}`).

Reference: tools/modules/clip_embedder.py:144-227.  `forward(image, text) -> (xi, xt, x)`: xi = `model.encode_image`
(open_clip VisionTransformer, the `visual` branch of CLIP), (xt, x) = the text path of vgen_amd/clip_text.py (penultimate
or last layer, EOT feature through text_projection).  The image tower, restated from open_clip 2.x
(transformer.py::VisionTransformer.forward, no patch dropout / attentional pool / patch norm in ViT-H-14):

    x = conv1(image)                      3 -> 1280, kernel = stride = 14, no bias: 16 x 16 patches
    x = ln_pre([class_embedding; x] + positional_embedding)                  257 tokens
    x = resblocks(x)                      32 blocks, 16 heads of 80, exact GELU, no mask
    xi = ln_post(x[:, 0]) @ proj          [B, 1024]

Execution: conv1 is a tap-GEMM over patch rows (vgen_patchify: K order (c, ky, kx), padded 588 -> 640, an all-zero row
in each image's CLS slot) whose fp32 residual is the positional table with class_embedding folded into row 0, repeated
per image; ln_pre is the LayerNorm kernel with fp32 output; the blocks are clip_text.residual_blocks with the head_dim-80
attention (vgen_attention_d80); ln_post + proj run on the B CLS rows only (LayerNorm is per row).  Images must be
[B, 3, 224, 224] and already normalised (the engines' vit_trans does that): the positional table fixes 257 tokens.

Device moves: the engines move the INNER module (`clip_encoder.model.to(gpu)`, inference_i2vgen_entrance.py:138), which
this wrapper does not see — the packed kernel operands are rebuilt whenever a parameter's storage, device or version
(an in-place copy such as load_state_dict) differs from the one they were packed from.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .clip_text import ARCHS as TEXT_ARCHS, HEAD_DIM, FrozenOpenCLIPEmbedder, _TextModelP, _TransformerP, pack_blocks, \
    residual_blocks
from .ops import TapGemm

VISION_ARCHS = {"ViT-H-14": dict(image_size=224, patch_size=14, width=1280, layers=32, head_width=80)}
KALIGN = 64                                    # tap-GEMM: C1 % 64 == 0


class _VisualP(nn.Module):
    """open_clip VisionTransformer parameter container (conv1, class / positional embedding, ln_pre, transformer,
    ln_post, proj)."""

    def __init__(self, image_size, patch_size, width, layers, head_width, output_dim):
        super().__init__()
        grid = image_size // patch_size
        scale = width ** -0.5
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(grid * grid + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = _TransformerP(width, layers, width // head_width)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))


class _CLIPP(_TextModelP):
    """open_clip CLIP parameter container: the text branch of clip_text plus `visual` — the 686 keys of a stock
    open_clip_pytorch_model.bin for ViT-H-14."""

    def __init__(self, text_cfg, vision_cfg):
        super().__init__(**text_cfg)
        self.visual = _VisualP(**vision_cfg, output_dim=text_cfg["embed_dim"])


class FrozenOpenCLIPTextVisualEmbedder(FrozenOpenCLIPEmbedder):
    LAYERS = ["last", "penultimate"]

    def __init__(self, pretrained=None, arch="ViT-H-14", device="cuda", max_length=77, freeze=True, layer="last",
                 compute_dtype=None, text_cfg=None, vision_cfg=None, **kwargs):
        nn.Module.__init__(self)
        assert layer in self.LAYERS
        tcfg = dict(text_cfg) if text_cfg is not None else TEXT_ARCHS.get(arch)
        vcfg = dict(vision_cfg) if vision_cfg is not None else VISION_ARCHS.get(arch)
        if tcfg is None or vcfg is None:
            raise NotImplementedError(f"FrozenOpenCLIPTextVisualEmbedder: unknown arch {arch!r} (ViT-H-14 is built)")
        if tcfg["width"] != tcfg["heads"] * HEAD_DIM:
            raise NotImplementedError("the text tower's attention kernels are built for head_dim 64")
        if vcfg["head_width"] != 80 or vcfg["width"] % vcfg["head_width"] or vcfg["width"] % KALIGN:
            raise NotImplementedError("the image tower's attention kernel is built for head_dim 80 (width % 64 == 0)")
        self.cfg, self.vision_cfg = tcfg, vcfg
        self.model = _CLIPP(tcfg, vcfg)
        self.device = device
        self.max_length = max_length
        self.layer = layer
        self.layer_idx = 0 if layer == "last" else 1
        self.compute_dtype = ops.sixteen(compute_dtype)
        self._packed = None
        if pretrained is not None:
            sd = torch.load(pretrained, map_location="cpu")
            sd = sd.get("state_dict", sd)
            own = self.state_dict()
            self.load_state_dict({k: v for k, v in (("model." + k if not k.startswith("model.") else k, v)
                                                    for k, v in sd.items()) if k in own}, strict=True)
        if freeze:
            self.freeze()

    # -- packed operands -------------------------------------------------------------------------------------
    def _stamp(self):
        return tuple((p.device, p.data_ptr(), p._version) for p in self.model.parameters())

    def _ensure_packed(self):
        stamp = self._stamp()
        if self._packed is None or self._packed.get("stamp") != stamp:
            self.pack()
            self._packed["stamp"] = stamp
        return self._packed

    @torch.no_grad()
    def pack(self):
        P = super().pack()                                   # text tower: tok, pos, lnf, proj, blocks
        dt = self.compute_dtype
        f32 = lambda t: t.detach().float().contiguous()
        v = self.model.visual
        width, Kc = v.conv1.weight.shape[0], v.conv1.weight[0].numel()
        Kpad = -(-Kc // KALIGN) * KALIGN
        wc = torch.zeros((width, Kpad), dtype=torch.float32, device=v.conv1.weight.device)
        wc[:, :Kc] = v.conv1.weight.detach().float().reshape(width, Kc)      # K order (c, ky, kx)
        pos = f32(v.positional_embedding).clone()
        pos[0] += v.class_embedding.detach().float()                           # the CLS slot's GEMM row is all zero
        P["visual"] = {"conv": wc.to(dt).contiguous(), "Kpad": Kpad, "pos": pos,
                       "ln_pre": (f32(v.ln_pre.weight), f32(v.ln_pre.bias)),
                       "ln_post": (f32(v.ln_post.weight), f32(v.ln_post.bias)),
                       "proj": f32(v.proj.t()), "blocks": pack_blocks(v.transformer.resblocks, dt), "posrep": {}}
        self._packed = P
        return P

    # -- towers ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _tower(self, tokens):
        self._ensure_packed()
        return super()._tower(tokens)

    @torch.no_grad()
    def encode_image(self, image):
        """[B, 3, 224, 224] normalised images -> [B, embed_dim] fp32 (clip_embedder.py:220-221, `model.visual`)."""
        be, dt = ops.backend(), self.compute_dtype
        V = self._ensure_packed()["visual"]
        vc = self.vision_cfg
        S, Pz = vc["image_size"], vc["patch_size"]
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, S, S):
            raise ValueError(f"encode_image: expected [B, 3, {S}, {S}] images (the positional table fixes "
                             f"{V['pos'].shape[0]} tokens), got {tuple(image.shape)}")
        B = image.shape[0]
        L = V["pos"].shape[0]
        width = V["conv"].shape[0]
        img = image.to(device=V["pos"].device, dtype=torch.float32).contiguous()
        a = be.patchify(img, Pz, V["Kpad"], 1, dt)                            # [B*257, Kpad], zero CLS rows
        res = V["posrep"].get(B)
        if res is None:                                  # positional table repeated per image (kept for the last B)
            V["posrep"].clear()
            res = V["posrep"][B] = be.repeat_rows(V["pos"], B)
        x = be.tapgemm(TapGemm(A=a, W=V["conv"], M=B * L, N=width, C1=V["Kpad"], residual=res))
        x = be.layernorm(x, *V["ln_pre"], 1e-5, torch.float32)
        x = residual_blocks(be, x, V["blocks"], B, L, width // vc["head_width"], vc["head_width"], False, dt)
        cls = x.view(B, L, width)[:, 0].contiguous()
        cls = be.layernorm(cls, *V["ln_post"], 1e-5, torch.float32)
        return be.linear_f32(cls, V["proj"], None)

    @torch.no_grad()
    def encode_with_transformer(self, text):
        """(xt, x): clip_embedder.py:190-198 (layer choice as the reference: penultimate drops the last block)."""
        return self.encode_text_and_tokens(text)

    def _tokens(self, text):
        if torch.is_tensor(text):
            return text
        try:
            import open_clip
        except ImportError as e:                               # the BPE tokenizer lives in the un-vendored package
            raise RuntimeError("FrozenOpenCLIPEmbedder.forward(str) needs open_clip.tokenize; pass token ids "
                               "[B, 77] (int64) to run the tower without it") from e
        return open_clip.tokenize(text)

    def forward(self, image=None, text=None):
        xi = self.encode_image(image) if image is not None else None
        xt, x = self.encode_with_transformer(self._tokens(text))
        return xi, xt, x

    def encode(self, text):
        return self(text=text)
