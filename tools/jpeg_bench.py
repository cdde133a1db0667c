"""vfml_jpeg_encode_rgb_sampled on device-resident frames (`--sampling 4:2:0|4:2:2|4:4:4`, default 4:2:0): time per frame at 3840x2160 (the 1080p job's TAA grid), 1920x1080 and
3840x3240 (the --flow-input grid), the scan's size, and what crosses PCIe per frame against the uncompressed picture
(dev tool, GPU only; not bench.py).

Protocol: every size warmed up, device events around windows of `--calls` back-to-back encodes of one picture (a smooth
scene with texture and noise, about the compression ratio of the render stage's frames), `--windows` windows, median
and spread.  The five kernels' own times come from a separate run under the profiler, whose tracing slows the host:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/jpeg_bench.py --size 3840x2160 --windows 1

`--size WxH` runs that one size only, so the profile's per-kernel averages belong to it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-flow-ml_amd"), ROOT):
    sys.path.insert(0, p)

import numpy as np
import torch

SIZES = [(3840, 2160), (1920, 1080), (3840, 3240)]


def picture(w, h, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(xx / 61 + yy / 97), 128 + 80 * np.cos(xx / 23 - yy / 131),
                     128 + 70 * np.sin((xx + yy) / 11)], axis=-1)
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH: this size only")
    ap.add_argument("--sampling", default="4:2:0", choices=["4:2:0", "4:2:2", "4:4:4"], help="chroma sampling of the frames")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench: needs a GPU; nothing is measured without one")
    from vfml import hip
    sizes = [tuple(int(v) for v in args.size.lower().split("x"))] if args.size else SIZES
    out = {"calls_per_window": args.calls, "sampling": args.sampling}
    code = hip.JPEG_ENCODE_SAMPLINGS[args.sampling]
    for w, h in sizes:
        img = torch.from_numpy(picture(w, h)).cuda()
        scan = torch.empty(hip.jpeg_scan_capacity(h, w, args.sampling), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            _, length = hip.jpeg_encode(img, out=scan, sampling=args.sampling)
        torch.cuda.synchronize()
        n = int(length.item())
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                hip.jpeg_encode(img, out=scan, sampling=args.sampling)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / args.calls * 1e3)
        med = statistics.median(us)
        raw = 3 * w * h
        print(f"{w}x{h} {args.sampling}: {med:8.1f} us per frame (windows {min(us):.1f} .. {max(us):.1f}); scan {n / 1e6:.3f} MB of "
              f"{raw / 1e6:.1f} MB RGB = 1/{raw / n:.1f} back over PCIe; workspace "
              f"{hip.lib().vfml_jpeg_sampled_workspace_bytes(h, w, code) / 1e6:.0f} MB, scan capacity {scan.numel() / 1e6:.0f} MB")
        out[f"{w}x{h}"] = {"us_median": med, "us_windows": us, "scan_bytes": n, "rgb_bytes": raw}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
