"""Per-launch times of the persistent GEMM form as the correlation pyramid calls it, against K, output width and the
transposed twin (dev tool, GPU only; wrote profiles/r04_a_corr_resident_per_tile.md).  One JSON line per case.

    python tools/corr_gemm_probe.py [out.json]            VFML_LIB=<other build> for the same table on another library"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd")); sys.path.insert(0, ROOT)
import torch
from vfml import hip

M = 32400          # rows of a 1080p pair's volume (135 x 240)
rows = []


def run(K, cout, twin, f16=False, reps=8):
    x = torch.randn(M * K, device="cuda")
    x16 = torch.empty_like(x)
    hip.to_s16(x, M, K, K, x16, K)
    wt = torch.randn(cout * K, device="cuda") / math.sqrt(K)
    w = hip.SplitWeight(cout, K, x.device).fill(wt, scale=hip.SplitWeight.auto_scale(float(wt.abs().max())))
    ld, ldt = (cout + 3) // 4 * 4, M
    out = torch.empty(M * ld // (2 if f16 else 1), device="cuda")
    out_t = torch.empty(cout * ldt, device="cuda") if twin else None
    kw = dict(out_scale=1.0 / 16.0, in_fmt=hip.FMT_S16, mfma=1, out_t=out_t, ld_out_t=ldt if twin else 0,
              out_fmt=hip.FMT_F16 if f16 else hip.FMT_F32)
    name = hip.conv2d(x16, K, K, 1, 1, M, w, None, cout, 1, 1, out, ld, variant_only=True, **kw)
    for _ in range(2):
        hip.conv2d(x16, K, K, 1, 1, M, w, None, cout, 1, 1, out, ld, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        hip.conv2d(x16, K, K, 1, 1, M, w, None, cout, 1, 1, out, ld, **kw)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    tiles = ((M + 127) // 128) * ((cout + 127) // 128)           # 128 x 128 tiles of the streaming walk
    stored = M * cout * (2 if f16 else 4) * (2 if twin else 1)
    r = dict(K=K, cout=cout, twin=twin, f16=f16, us=round(us, 1), tiles=tiles, us_per_tile=round(us / (tiles / 512.0), 2),
             TBps=round(stored / us / 1e6, 2), name=name)
    rows.append(r)
    print(json.dumps(r), flush=True)
    del out, out_t, x, x16, wt, w
    torch.cuda.empty_cache()


if __name__ == "__main__":
    for K in (64, 128, 256, 512):
        run(K, 32640, True)
    for K in (128, 256, 512):
        run(K, 32640, False)
    for K in (128, 256, 512):
        run(K, 8640, False)
    run(256, 16320, True)
    run(256, 16320, False)
    run(256, 2400, False)
    run(256, 512, False, f16=True, reps=20)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
