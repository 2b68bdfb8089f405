"""GPU probe for same-box A/B runs of two builds of norms.hip (VGEN_HIP_LIB selects the library): GroupNorm on the step's
shapes (those of tools/norm_probe.py) with statistics from x ("plain"), with statistics from a producing tap-GEMM ("cs"), and
one statistics-fed launch whose input takes gn_finalize_cs_kernel's conditioning guard on every group ("cs_guarded": mean /
sigma = 1000).  Prints one JSON line, microseconds per launch; run it alternately with both libraries in one session."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vgen_amd import ops
from vgen_amd.ops import TapGemm

be = ops.backend()
dev = "cuda:0"
dt = torch.bfloat16


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n * 1e3, 2)


def gn(x, nb, S, C):
    g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    return timeit(lambda: be.groupnorm(x, None, nb, S, 32, 1e-5, g, b, True, False, dt))


def produced(nb, S, C, offset):
    M = nb * S
    A = torch.randn(M, 64, device=dev).to(dt)
    W = (torch.randn(C, 64, device=dev) / 8).to(dt)
    x = be.tapgemm(TapGemm(A=A, W=W, M=M, N=C, C1=64, residual=torch.randn(M, C, device=dev) + offset, colstats=True))
    assert x.vgen_cs is not None
    return x


res = {}
for nb, S, C in [(2, 28672, 320), (32, 1792, 320), (2, 7168, 640), (2, 1792, 1280), (2, 448, 1280), (32, 28, 1280), (32, 448, 640),
                 (32, 112, 1280), (32, 112, 2560), (32, 28, 2560)]:
    res[f"plain/{nb}x{S}x{C}"] = gn(torch.randn(nb * S, C, device=dev), nb, S, C)
for nb, S, C in [(2, 28672, 320), (32, 1792, 320), (2, 7168, 640), (2, 3328, 1280)]:
    res[f"cs/{nb}x{S}x{C}"] = gn(produced(nb, S, C, 0.0), nb, S, C)
for nb, S, C in [(2, 3328, 1280), (2, 28672, 320)]:
    res[f"cs_guarded/{nb}x{S}x{C}"] = gn(produced(nb, S, C, 1000.0), nb, S, C)
for kind in ("plain", "cs"):
    res[kind + "_sum"] = round(sum(v for k, v in res.items() if k.startswith(kind + "/")), 2)
print(json.dumps({"lib": os.path.basename(os.environ.get("VGEN_HIP_LIB", "libvgen_hip.so")), **res}))
