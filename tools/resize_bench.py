"""vfml_resize_u8 on device-resident frames: time per frame for 1080p, 4K and 720p sources to their --fast sizes (the
separable path) and for 512x512 (the 2x2 mean), with the bytes moved over the time as a share of the HBM peak (dev tool,
GPU only; not bench.py).

Protocol: every shape warmed up, device events around windows of `--calls` back-to-back calls, `--windows` windows,
median and spread reported - twice: one frame per launch (what the feeder issues; at these sizes a window's time per
call is the host's launch rate, an upper bound of the kernel's time, which a `rocprofv3 --kernel-trace` run gives) and
`--batch` frames per launch (the kernel's own time per frame with the launch shared out).  Bytes moved per frame: the source pixels the taps name, once each (separable: the distinct
tap columns of the distinct tap rows; 2x2: the whole source), plus the destination written once.  A --fast frame reads a
small part of its source, so the separable figures say how far from a bandwidth limit a latency-bound launch sits; the
comparison that matters for the feeder is with the frame's host-to-device copy."""
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

HBM_PEAK = 8.0e12      # bytes / s
SOURCES = [("1080p", 1920, 1080), ("4K", 3840, 2160), ("720p", 1280, 720), ("512x512", 512, 512)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: needs a GPU; nothing is measured without one")
    from vfml import hip
    from video import fast_mode_dimensions
    rng = np.random.default_rng(0)
    out = {"calls_per_window": args.calls, "batch": args.batch}

    def windows(fn, calls, frames):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / (calls * frames) * 1e3)
        return statistics.median(us), us
    for name, W, H in SOURCES:
        w, h, _ = fast_mode_dimensions(W, H)
        src = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        area = H == 2 * h and W == 2 * w
        if area:
            read = 3.0 * H * W
        else:
            tx, ty = hip.resize_tables(W, w), hip.resize_tables(H, h)
            read = 3.0 * len(np.unique(tx[:, :2])) * len(np.unique(ty[:, :2]))
        nbytes = read + 3.0 * h * w
        med, us = windows(lambda: hip.resize_u8(src, (h, w), out=dst), args.calls, 1)
        srcs = src.expand(args.batch, H, W, 3).contiguous()
        srcs[1::2] = srcs[1::2].flip(1)
        dsts = torch.empty((args.batch, h, w, 3), dtype=torch.uint8, device="cuda")
        bmed, bus = windows(lambda: hip.resize_u8(srcs, (h, w), out=dsts), max(1, args.calls // args.batch), args.batch)
        print(f"{name:8s} {W}x{H} -> {w}x{h} ({'2x2 mean' if area else 'separable'}): {med:7.2f} us per frame (windows "
              f"{min(us):.2f} .. {max(us):.2f}); {nbytes / 1e6:.3f} MB moved = {nbytes / med / 1e3:.1f} GB/s, "
              f"{100 * nbytes / HBM_PEAK / (med * 1e-6):.2f} % of the {HBM_PEAK / 1e12:.1f} TB/s peak; {args.batch} frames per "
              f"launch: {bmed:6.2f} us per frame ({min(bus):.2f} .. {max(bus):.2f}) = {nbytes / bmed / 1e3:.1f} GB/s, "
              f"{100 * nbytes / HBM_PEAK / (bmed * 1e-6):.2f} %")
        out[name] = {"source": [W, H], "size": [w, h], "path": "2x2" if area else "separable", "us_median": med,
                     "us_windows": us, "batched_us_per_frame": bmed, "batched_us_windows": bus, "bytes_moved": nbytes, "share_of_hbm_peak": nbytes / HBM_PEAK / (med * 1e-6)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
