"""vfml_flow_turbulence_map on a device-resident 1080p field, k = 25: time per map, the share of the algorithmic HBM
traffic it achieves, and the numpy restatement's time on the host (dev tool, GPU only; not bench.py).

Protocol: every shape warmed up, device events around windows of `--calls` back-to-back calls (a window is a good
fraction of a second), `--windows` windows, median and spread reported.  Kernel-by-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/turbulence_bench.py --windows 1` run (tracing slows the host).

Algorithmic traffic per pixel: the field read once (8 B), tv written once (4 B) and read again by the two refinement
passes of the selection and by the colour pass (3 x 4 B), the picture written (3 B) = 27 B."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-flow-ml_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.29e12      # bytes / s: spec, and a float4 copy measured on this part
LAUNCHES = 8                                    # one memset, the moments pass, 3 selects, 2 refinements, the colour pass


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--kernel-size", type=int, default=25)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement's time")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("turbulence_bench: needs a GPU; nothing is measured without one")
    import flow_maps
    import turbulence_oracle as to
    h, w, k = args.height, args.width, args.kernel_size
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    flow = np.stack([5 * np.sin(xx / 41 + yy / 67), 4 * np.cos(yy / 31 - xx / 83)], axis=2).astype(np.float32)
    flow += (rng.normal(0, 1, (h, w, 2)) * rng.choice([0.01, 0.1, 1.0, 4.0], (-(-h // 40), -(-w // 40), 1)
                                                      ).repeat(40, 0).repeat(40, 1)[:h, :w]).astype(np.float32)
    dev = torch.from_numpy(flow).cuda()
    fields = {"full-resolution field": dev,
              "LOD-1 field": torch.from_numpy(np.ascontiguousarray(flow[::2, ::2])).cuda()}
    out = {"height": h, "width": w, "kernel_size": k, "launches": LAUNCHES, "calls_per_window": args.calls}
    nbytes = 27.0 * h * w
    for name, fl in fields.items():
        for _ in range(20):
            flow_maps.turbulence_map_resident(fl, h, w, k)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                flow_maps.turbulence_map_resident(fl, h, w, k)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / args.calls * 1e3)
        med = statistics.median(us)
        print(f"{name:24s} {med:8.1f} us per {h}x{w} map (windows {min(us):.1f} .. {max(us):.1f}); algorithmic traffic "
              f"{nbytes / 1e6:.1f} MB = {nbytes / med / 1e6:.2f} TB/s: {100 * nbytes / HBM_ACHIEVABLE / (med * 1e-6):.1f} % of "
              f"the achievable {HBM_ACHIEVABLE / 1e12:.2f} TB/s, {100 * nbytes / HBM_PEAK / (med * 1e-6):.1f} % of the "
              f"{HBM_PEAK / 1e12:.1f} TB/s peak; {LAUNCHES} launches")
        out[name] = {"us_median": med, "us_windows": us, "algorithmic_bytes": nbytes,
                     "share_of_achievable_hbm": nbytes / HBM_ACHIEVABLE / (med * 1e-6)}
    if not args.no_host:
        to.turbulence_map(flow, h, w, k)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            to.turbulence_map(flow, h, w, k)
            t.append(time.perf_counter() - t0)
        threads = os.environ.get("OMP_NUM_THREADS", "unset")
        print(f"numpy restatement        {min(t) * 1e3:8.1f} ms per map on the host (best of 3, OMP_NUM_THREADS={threads})")
        out["numpy_restatement_ms"] = min(t) * 1e3
        out["host_threads"] = threads
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
