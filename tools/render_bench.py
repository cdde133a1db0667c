#!/usr/bin/env python3
"""Render-stage throughput: the visualiser's "Run TAA processor" command (flow_processor.py --taa --skip-lods --tile
--flow-format hsv --use-flow-cache <cache>) on a synthetic:WxHxN clip with a complete cache of seeded fields, MJPG and
--uncompressed.  Prints one JSON line per codec: frames, seconds, frames/s, file size, and for MJPG who encoded the frames
("device": vfml_jpeg_encode_rgb behind the composer, only the scan copied back; "pillow": the host pool).  With --flow-input each codec gets
a second job: the same cache rendered with --flow-only --flow-format motion-vectors-rg8 (the flow video), then
--taa --flow-input <that video> --flow-format motion-vectors-rg8, the 2x3 comparison grid.  With --labels the MJPG --taa
job (the 2x2 grid) is instead rendered --repeats times with the text labels off and on in turn (VFML_LABELS=0 / 1,
vfml_text_draw behind the composer), one line each and a closing line with both lists of frames/s.

    python tools/render_bench.py --size 1920x1080 --frames 60 [--device cuda] [--codec mjpg|raw|both] [--flow-input]
    python tools/render_bench.py --size 1920x1080 --frames 60 --labels [--repeats 3]
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--codec", choices=["mjpg", "raw", "both"], default="both")
    ap.add_argument("--flow-input", action="store_true", help="also render the 2x3 --flow-input grid")
    ap.add_argument("--labels", action="store_true", help="the MJPG 2x2 job with the text labels off and on, alternating")
    ap.add_argument("--repeats", type=int, default=3, help="off/on pairs of --labels")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    import flow_processor as fp
    from storage import FlowCacheManager
    w, h = (int(v) for v in a.size.split("x"))
    work = a.work or tempfile.mkdtemp(prefix="vfml_render_bench_")
    cache = os.path.join(work, "cache_corrected")
    os.makedirs(cache, exist_ok=True)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    mgr = FlowCacheManager()
    for i in range(a.frames):
        f = np.stack([4 * np.sin(xx / 97 + i / 7), 3 * np.cos(yy / 61 - i / 5)], axis=2).astype(np.float32)
        f += rng.normal(0, 0.3, f.shape).astype(np.float32)
        mgr.save_flow_to_cache(f, cache, i, 'npz')
    spec = f"synthetic:{w}x{h}x{a.frames}"
    def run(job, codec, extra, keep=False, labels=None):
        out = os.path.join(work, f"out_{job}_{codec}")
        if labels is not None:
            os.environ["VFML_LABELS"] = labels
        os.makedirs(out, exist_ok=True)
        argv = ["--input", spec, "--output", out, "--device", a.device, "--frames", str(a.frames), "--skip-lods",
                "--tile", "--use-flow-cache", cache] + extra
        if codec == "raw":
            argv.append("--uncompressed")
        buf = io.StringIO()
        t0 = time.time()
        with contextlib.redirect_stdout(buf):
            rc = fp.main(argv)
        dt = time.time() - t0
        line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Video written")]
        avi = [os.path.join(out, n) for n in os.listdir(out) if n.endswith(".avi")]
        encoder = None
        if codec == "mjpg":
            encoder = "device" if str(a.device).startswith("cuda") and hasattr(fp, "DEVICE_MJPG") else "pillow"
        if labels is not None:
            del os.environ["VFML_LABELS"]
            m = re.search(r"([0-9.]+) frames/s", line[0]) if line else None
            rates[labels].append(float(m.group(1)) if m else None)
        print(json.dumps({"job": job, "codec": codec, "mjpg_encoder": encoder, "labels": labels, "size": a.size,
                          "frames": a.frames, "rc": rc,
                          "wall_s": round(dt, 3), "render_line": line[0] if line else None,
                          "bytes": os.path.getsize(avi[0]) if avi else None}), flush=True)
        if not keep:
            for p in avi:
                os.remove(p)
        return rc, avi

    rates = {"0": [], "1": []}
    if a.labels:
        run("taa", "mjpg", ["--taa", "--flow-format", "hsv"], labels="0")        # warm-up: library load, first launches
        rates = {"0": [], "1": []}
        for _ in range(a.repeats):
            for labels in ("0", "1"):
                rc, _ = run("taa", "mjpg", ["--taa", "--flow-format", "hsv"], labels=labels)
                if rc != 0:
                    return rc
        print(json.dumps({"job": "labels", "size": a.size, "frames": a.frames, "frames_per_s_off": rates["0"],
                          "frames_per_s_on": rates["1"]}), flush=True)
        return 0
    for codec in (["mjpg", "raw"] if a.codec == "both" else [a.codec]):
        rc, _ = run("taa", codec, ["--taa", "--flow-format", "hsv"])
        if rc != 0:
            return rc
        if a.flow_input:
            mv = ["--flow-format", "motion-vectors-rg8"]
            rc, avi = run("flow_only", codec, ["--flow-only"] + mv, keep=True)
            if rc == 0:
                rc, _ = run("flow_input", codec, ["--taa", "--flow-input", avi[0]] + mv)
            for p in avi:
                os.remove(p)
            if rc != 0:
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
