"""vfml_jpeg_decode_rgb on device-resident files: time per picture at 1920x1080, at 1920x2160 with rows=(1080, 2160) (the
--flow-input window of a 1080p job) next to the full decode of the same file, and at 3840x2160 - each beside Pillow's
decode of the same bytes on the same box (dev tool, GPU only; not bench.py).

Protocol (that of tools/jpeg_bench.py): the scene of jpeg_bench.picture encoded by the device encoder at quality 95,
every case warmed up, device events around windows of `--calls` back-to-back decodes of the one file - its bytes
already on the device, so a window holds the five kernels and the upload of nothing - `--windows` windows, median and
spread.  Pillow: the median of `--windows` single decodes on one host thread.  The kernels' own times come from a
separate run under the profiler, whose tracing slows the host:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/jpeg_decode_bench.py --size 1920x1080 --windows 1

`--size WxH` runs that one size only (full decode), so the profile's per-kernel averages belong to it.

`--restart 0`: the files are Pillow's instead (quality 95, no DRI segment: the scan is one interval, as OpenCV's and
ffmpeg's MJPG writers leave it) at 1920x1080 and 1920x2160, and every window measures, one after the other on the same
bytes, the self-synchronising kernel (`--plan sync`) at each `--subseq` size, the interval
kernel (`--plan interval`: one wave walks the whole scan; `--interval-calls` decodes per window) and one Pillow decode.
`--plan` picks one of the two kernels.

`--sampling 4:2:0,4:2:2,4:4:4,grey` (any of them): Pillow's files of the scene in those samplings at quality 95 (1920x1080, or
`--size`), each written twice - one MCU row per restart interval for the interval kernel, no markers for the
self-synchronising kernel at its default subsequence size - and every window measures every sampling and both kernels
one after the other, so the figures of a run stand beside each other; `--plan` picks one kernel."""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-flow-ml_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np
import torch

from jpeg_bench import picture

CASES = [(1920, 1080, None), (1920, 2160, None), (1920, 2160, (1080, 2160)), (3840, 2160, None)]


def norestart(args, hip, jpeg_parse, Image):
    if Image is None:
        raise SystemExit("jpeg_decode_bench --restart 0: the files are Pillow's; Pillow is not installed")
    sizes = [tuple(int(v) for v in args.size.lower().split("x"))] if args.size else [(1920, 1080), (1920, 2160)]
    configs = []
    if args.plan in (None, "sync"):
        configs += [(f"sync S={int(v)}", dict(plan="sync", subseq_bytes=int(v)), args.calls) for v in args.subseq.split(",")]
    if args.plan in (None, "interval"):
        configs.append(("interval", dict(plan="interval"), args.interval_calls))
    out = {"calls_per_window": args.calls, "interval_calls_per_window": args.interval_calls}
    for w, h in sizes:
        buf = io.BytesIO()
        Image.fromarray(picture(w, h), "RGB").save(buf, format="JPEG", quality=95)
        data = buf.getvalue()
        info = jpeg_parse.parse(data)
        assert info.restart_interval == 0
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        res = {"file_bytes": len(data), "scan_bytes": info.scan[1] - info.scan[0]}
        for name, kw, _ in configs:
            _, status = hip.jpeg_decode(dev, out=rgb, info=info, **kw)
            hip.jpeg_decode_check(status)
            res[name] = {"us_windows": [], "same_bytes": bool(np.array_equal(rgb.cpu().numpy(), ref))}
        pil = []
        for _ in range(args.windows):
            for name, kw, calls in configs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    hip.jpeg_decode(dev, out=rgb, info=info, **kw)
                e1.record()
                torch.cuda.synchronize()
                res[name]["us_windows"].append(e0.elapsed_time(e1) / calls * 1e3)
            t0 = time.perf_counter()
            np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            pil.append((time.perf_counter() - t0) * 1e6)
        print(f"{w}x{h}, Pillow's file without restart markers: {len(data) / 1e6:.3f} MB")
        for name, _, _ in configs:
            us = res[name]["us_windows"]
            res[name]["us_median"] = statistics.median(us)
            print(f"  {name:12s} {statistics.median(us):10.1f} us per picture (windows {min(us):.1f} .. {max(us):.1f}); "
                  f"same bytes: {res[name]['same_bytes']}")
        print(f"  {'Pillow':12s} {statistics.median(pil):10.1f} us per picture ({min(pil):.1f} .. {max(pil):.1f})")
        res["pillow_us_median"], res["pillow_us"] = statistics.median(pil), pil
        out[f"{w}x{h}"] = res
    print(json.dumps(out))
    return 0


def pillow_sampled(Image, img, sampling, **kw):
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(img, "RGB").convert("L").save(buf, format="JPEG", quality=95, **kw)
    else:
        Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=95, subsampling=sampling, **kw)
    return buf.getvalue()


def sampled(args, hip, jpeg_parse, Image):
    if Image is None:
        raise SystemExit("jpeg_decode_bench --sampling: the files are Pillow's; Pillow is not installed")
    names = args.sampling.split(",")
    for name in names:
        if name not in jpeg_parse.DEVICE_SAMPLINGS:
            raise SystemExit(f"jpeg_decode_bench --sampling {name}: one of {', '.join(jpeg_parse.DEVICE_SAMPLINGS)}")
    w, h = (int(v) for v in args.size.lower().split("x")) if args.size else (1920, 1080)
    img = picture(w, h)
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    configs, out = [], {"calls_per_window": args.calls, "size": f"{w}x{h}"}
    for name in names:
        for plan, kw in (("interval", dict(restart_marker_rows=1)), ("sync", {})):
            if args.plan not in (None, plan):
                continue
            data = pillow_sampled(Image, img, name, **kw)
            info = jpeg_parse.parse(data, jpeg_parse.DEVICE_SAMPLINGS)
            assert info.sampling == name and jpeg_parse.decode_plan(info) == plan
            dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            for _ in range(3):
                _, status = hip.jpeg_decode(dev, out=rgb, info=info, plan=plan)
            hip.jpeg_decode_check(status)
            same = bool(np.array_equal(rgb.cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))
            configs.append((f"{name} {plan}", dev, info, plan))
            out[f"{name} {plan}"] = {"us_windows": [], "same_bytes": same, "file_bytes": len(data), "intervals": info.intervals}
    for _ in range(args.windows):
        for key, dev, info, plan in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                hip.jpeg_decode(dev, out=rgb, info=info, plan=plan)
            e1.record()
            torch.cuda.synchronize()
            out[key]["us_windows"].append(e0.elapsed_time(e1) / args.calls * 1e3)
    print(f"{w}x{h}, Pillow's files at quality 95")
    for key, *_ in configs:
        us = out[key]["us_windows"]
        out[key]["us_median"] = statistics.median(us)
        print(f"  {key:16s} {statistics.median(us):10.1f} us per picture (windows {min(us):.1f} .. {max(us):.1f}); file "
              f"{out[key]['file_bytes'] / 1e6:.3f} MB; same bytes: {out[key]['same_bytes']}")
    print(json.dumps(out))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH: the full decode of this size only")
    ap.add_argument("--restart", type=int, default=None, choices=[0],
                    help="0: Pillow-written files without restart markers, both kernels and Pillow alternating")
    ap.add_argument("--plan", default=None, choices=["interval", "sync"], help="with --restart 0: that kernel only")
    ap.add_argument("--subseq", default="64,128,256", help="with --restart 0: the sync kernel's subsequence sizes")
    ap.add_argument("--interval-calls", type=int, default=2)
    ap.add_argument("--sampling", default=None, help="comma-separated, of 4:2:0 4:2:2 4:4:4 grey: Pillow's files in those "
                    "samplings, both kernels")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench: needs a GPU; nothing is measured without one")
    from storage import jpeg_parse
    from vfml import hip
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if args.sampling:
        return sampled(args, hip, jpeg_parse, Image)
    if args.restart == 0:
        return norestart(args, hip, jpeg_parse, Image)
    cases = [(*(int(v) for v in args.size.lower().split("x")), None)] if args.size else CASES
    out = {"calls_per_window": args.calls}
    files = {}
    for w, h, rows in cases:
        if (w, h) not in files:
            img = torch.from_numpy(picture(w, h)).cuda()
            files[(w, h)] = hip.jpeg_file(hip.jpeg_header(h, w, 95), hip.jpeg_scan(*hip.jpeg_encode(img)))
            del img
        data = files[(w, h)]
        info = jpeg_parse.parse(data)
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        y0, y1 = rows or (0, h)
        rgb = torch.empty((y1 - y0, w, 3), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            _, status = hip.jpeg_decode(dev, rows=rows, out=rgb, info=info)
        hip.jpeg_decode_check(status)
        us = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                hip.jpeg_decode(dev, rows=rows, out=rgb, info=info)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / args.calls * 1e3)
        med = statistics.median(us)
        name = f"{w}x{h}" + (f" rows {y0}..{y1}" if rows else "")
        line = f"{name}: {med:9.1f} us per picture (windows {min(us):.1f} .. {max(us):.1f}); file {len(data) / 1e6:.3f} MB, " \
               f"{info.intervals} intervals"
        res = {"us_median": med, "us_windows": us, "file_bytes": len(data), "intervals": info.intervals}
        if Image is not None:
            pil = []
            for _ in range(args.windows):
                t0 = time.perf_counter()
                ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                pil.append((time.perf_counter() - t0) * 1e6)
            same = bool(np.array_equal(rgb.cpu().numpy(), ref[y0:y1]))
            line += f"; Pillow (whole picture) {statistics.median(pil):9.1f} us ({min(pil):.1f} .. {max(pil):.1f}); " \
                    f"same bytes: {same}"
            res.update(pillow_us_median=statistics.median(pil), pillow_us=pil, same_bytes=same)
        print(line)
        out[name] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
