"""Measurements of the DreamVideo path (GPU): what the adapters cost per CFG step, and what fusing one buys.

  python tools/bench_dreamvideo.py step     [--rounds 5 --steps 10]   -> <out>/dreamvideo_step_timing.json
  python tools/bench_dreamvideo.py adapter  [--rounds 7 --iters 20]   -> <out>/dreamvideo_adapter_timing.json
  python tools/bench_dreamvideo.py trace    [--steps 4]               (the joint step alone, for a profiler run of its own:
                                                                       rocprofv3 --kernel-trace --stats -- python ... trace)
  python tools/bench_dreamvideo.py stats CSV --steps 4                -> <out>/dreamvideo_kernel_stats.json   (--out DIR, default profiles/)

step:    one classifier-free-guidance DDIM step through the public DiffusionDDIM.ddim_sample (session / graph replay) at the
         latent [1, 4, 32, 32, 32], fp16, the class's default precision, seeded weights: (a) both adapter lists empty — the
         configuration the t2v trunk alone also runs: the baseline —, (b) the motion adapter, (c) identity + motion.  The three
         models alternate in one process; device events around windows of `steps` replays; median and spread per
         configuration, and (c) - (a).
adapter: the fused kernel against the same operator composed from the existing exports (cast, tap-GEMM with the hidden
         width padded to a multiple of 64, GELU pass, tap-GEMM with `residual`) at the four full-size shapes, alternating
         in one call.  The composed sequence is a yardstick of this tool only, never a product path.  Bytes model of the
         fused kernel: x read + out written in fp32, both weights once (they stay in L2) — achieved B/s against the HBM
         peak of 8 TB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E
LATENT = (1, 4, 32, 32, 32)
BASE = dict(in_dim=4, dim=320, y_dim=1024, context_dim=1024, out_dim=4, dim_mult=[1, 2, 4, 4], num_heads=8, head_dim=64,
            num_res_blocks=2, attn_scales=[1.0, 0.5, 0.25], temporal_attention=True, use_fps_condition=False)
MOTION = dict(temporal_adapter_list=["self_attention", "cross_attention", "feedforward"], temporal_adapter_condition_dim=1024)
CONFIGS = {"a_no_adapters": {}, "b_motion": MOTION, "c_joint": dict(MOTION, spatial_adapter_list=["cross_attention"])}
SHAPES = [(65536, 320, 160), (65536, 512, 256), (16384, 640, 320), (4096, 1280, 640)]


OUT_DIR = "profiles"


def out_path(name):
    d = os.path.join(ROOT, OUT_DIR)
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, name)


def build(extra, sd_all=None):
    from vgen_amd.synth import seeded_state_dict
    from vgen_amd.unet_dreamvideo import UNetSD_DreamVideo
    with torch.device("meta"):
        m = UNetSD_DreamVideo(**BASE, **extra, compute_dtype="fp16")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = seeded_state_dict(shapes, seed=0)
    m = m.to_empty(device="cpu").eval()
    m.load_state_dict(sd, strict=True, assign=True)
    return m.to(DEV)


def step_inputs():
    g = torch.Generator("cpu").manual_seed(1)
    x = torch.randn(LATENT, generator=g).to(DEV)
    y = torch.randn(1, 77, 1024, generator=g).to(DEV)
    yi = torch.randn(1, 1, 1024, generator=g).to(DEV)
    t = torch.full((1,), 601, dtype=torch.long, device=DEV)
    kw = [dict(y=y, y_image=yi, ag_strength=1.0), dict(y=torch.zeros_like(y), y_image=torch.zeros_like(yi), ag_strength=1.0)]
    return x, t, kw


def diffusion():
    from vgen_amd.diffusion import DiffusionDDIM
    d = DiffusionDDIM(schedule="linear_sd", schedule_param=dict(num_timesteps=1000, init_beta=0.00085, last_beta=0.012,
                                                                zero_terminal_snr=True),
                      mean_type="eps", loss_type="mse", var_type="fixed_small", rescale_timesteps=False)
    d.rng_parity = False
    return d


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def cmd_step(a):
    x, t, kw = step_inputs()
    runs = {}
    for name, extra in CONFIGS.items():
        m, d = build(extra), diffusion()
        fn = lambda m=m, d=d: d.ddim_sample(x, t, m, kw, guide_scale=9.0, ddim_timesteps=50, eta=0.0)
        for _ in range(4):                                # eager, capture, replays
            fn()
        runs[name] = (fn, m.precision)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (fn, _) in runs.items():
            ms[name].append(window(fn, a.steps))
    res = {k: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), precision=runs[k][1]) for k, v in ms.items()}
    res["c_minus_a_ms"] = res["c_joint"]["ms_median"] - res["a_no_adapters"]["ms_median"]
    res["b_minus_a_ms"] = res["b_motion"]["ms_median"] - res["a_no_adapters"]["ms_median"]
    res["meta"] = dict(latent=LATENT, dtype="fp16", rounds=a.rounds, steps_per_window=a.steps, device=torch.cuda.get_device_name(0))
    json.dump(res, open(out_path("dreamvideo_step_timing.json"), "w"), indent=1)
    print(json.dumps(res))


def cmd_trace(a):
    x, t, kw = step_inputs()
    m, d = build(CONFIGS["c_joint"]), diffusion()
    d.sessions = None                                     # eager launches: every kernel appears in the trace by name
    for _ in range(a.steps):
        d.ddim_sample(x, t, m, kw, guide_scale=9.0, ddim_timesteps=50, eta=0.0)
    torch.cuda.synchronize()


def cmd_stats(a):
    import csv
    rows = list(csv.DictReader(open(a.csv)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    tot = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    ad = [r for r in rows if "adapter_kernel" in r[name]]
    all_ns = sum(float(r[tot]) for r in rows)
    res = dict(steps=a.steps, adapter_ms_per_step=sum(float(r[tot]) for r in ad) / 1e6 / a.steps,
               all_kernels_ms_per_step=all_ns / 1e6 / a.steps,
               by_instantiation={r[name][-60:]: dict(calls_per_step=int(r[calls]) / a.steps, ms_per_step=float(r[tot]) / 1e6 / a.steps)
                                 for r in ad})
    json.dump(res, open(out_path("dreamvideo_kernel_stats.json"), "w"), indent=1)
    print(json.dumps(res))


def cmd_adapter(a):
    from vgen_amd import ops
    from vgen_amd.ops import TapGemm
    be = ops.backend()
    dt = torch.float16
    res = {}
    for M, d, h in SHAPES:
        g = torch.Generator("cpu").manual_seed(M + d)
        hp32, hp64 = (h + 31) // 32 * 32, (h + 63) // 64 * 64
        x = (torch.randn(M, d, generator=g) * 2).to(DEV)
        wd = torch.zeros(hp64, d)
        wd[:h] = torch.randn(h, d, generator=g) / d ** 0.5
        wu = torch.zeros(d, hp64)
        wu[:, :h] = torch.randn(d, h, generator=g) / h ** 0.5
        bu = (0.1 * torch.randn(d, generator=g)).to(DEV)
        bd = torch.zeros(hp64)
        bd[:h] = torch.randn(h, generator=g)
        wd16, wu16, bd = wd.to(dt).to(DEV), wu.to(dt).to(DEV), bd.to(DEV)
        wd32p, wu32p = wd16[:hp32].contiguous(), wu16[:, :hp32].contiguous()
        hb = bd[:hp32].view(1, hp32).contiguous()

        def fused():
            return be.adapter(x, wd32p, wu32p, bu, hb, M, h)

        def composed():
            a16 = be.act_cast(x, 0, dt)
            s = be.tapgemm(TapGemm(A=a16, W=wd16, M=M, N=hp64, C1=d, bias=bd))
            g16 = be.act_cast(s, 2, dt)
            return be.tapgemm(TapGemm(A=g16, W=wu16, M=M, N=d, C1=hp64, bias=bu, residual=x))

        o1, o2 = fused(), composed()
        dev = float((o1 - o2).norm() / o2.norm())           # the two differ by the erf polynomial of the GELU pass only
        for fn in (fused, composed):
            window(fn, 3)
        tf, tc = [], []
        for _ in range(a.rounds):
            tf.append(window(fused, a.iters))
            tc.append(window(composed, a.iters))
        fbytes = 8.0 * M * d + 4.0 * d * hp32
        cbytes = (4 + 2) * M * d + (2.0 * M * d + 4.0 * M * hp64) + 6.0 * M * hp64 + (2.0 * M * hp64 + 8.0 * M * d)
        mf, mc = statistics.median(tf), statistics.median(tc)
        res[f"{M}x{d}x{h}"] = dict(fused_us=mf * 1e3, fused_us_min_max=[min(tf) * 1e3, max(tf) * 1e3], composed_us=mc * 1e3,
                                   composed_us_min_max=[min(tc) * 1e3, max(tc) * 1e3], composed_over_fused=mc / mf,
                                   fused_bytes=fbytes, composed_bytes=cbytes, fused_bytes_per_s=fbytes / (mf * 1e-3),
                                   fused_share_of_hbm_peak=fbytes / (mf * 1e-3) / HBM_PEAK, rel_l2_fused_vs_composed=dev)
        print(f"{M}x{d}x{h}", json.dumps(res[f"{M}x{d}x{h}"]), flush=True)
    res["meta"] = dict(dtype="fp16", rounds=a.rounds, iters=a.iters, hbm_peak=HBM_PEAK, device=torch.cuda.get_device_name(0))
    json.dump(res, open(out_path("dreamvideo_adapter_timing.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["step", "adapter", "trace", "stats"])
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=OUT_DIR, help="directory (relative to the repository root) the result files go to")
    a = ap.parse_args()
    OUT_DIR = a.out
    with torch.no_grad():
        {"step": cmd_step, "adapter": cmd_adapter, "trace": cmd_trace, "stats": cmd_stats}[a.cmd](a)
