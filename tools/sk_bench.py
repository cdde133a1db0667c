#!/usr/bin/env python3
"""What the SK update block costs on an MI355X, in one process:

  (a) vfml_dwconv2d alone at the shapes one 1080p seq-5 iteration runs - the five 15 x 15 ones and the 7 x 7 one, split
      rows in and out, residual and GELU fused: device events, warm-up, median and spread, each set against its two bounds
      (k^2 FMAs per output at the 157.3 TFLOP/s vector peak; one read and one write of the map at the HBM rate);
  (b) where a field's device time goes: one eager (ungraphed) 1080p field with every launch of the iteration body between
      two events, summed per class - depthwise launches, GELU passes, the PCBlocks' dense 1x1 convolutions, everything else;
  (c) fields/s of a sliding 1080p seq-5 depth-12 job with a seeded SK checkpoint and with a plain one, through the job
      loop bench.py times (vfml.runner.run_sharded: host frames in, fields in host memory out).

Writes profiles/sk_bench.json and prints it.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

VALU_PEAK = 157.3e12        # f32 FLOP/s of the vector ALUs (spec)
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def _stats(ms):
    ms = sorted(ms)
    return {"median_us": round(1000 * statistics.median(ms), 1), "min_us": round(1000 * ms[0], 1),
            "max_us": round(1000 * ms[-1], 1), "p10_us": round(1000 * ms[len(ms) // 10], 1),
            "p90_us": round(1000 * ms[-1 - len(ms) // 10], 1), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def dwconv_alone(n, h, w, reps, dev):
    from vfml import hip
    out = []
    g = torch.Generator().manual_seed(0)
    for layer, c, k in (("encoder.convc1", 672, 15), ("encoder.convc2", 256, 15), ("encoder.convf2", 128, 15),
                        ("encoder.conv", 256, 15), ("flow_head", 128, 15), ("gru", 512, 7)):
        rows = n * h * w
        x32 = torch.randn(rows * c, generator=g).to(dev)
        x = torch.empty(rows * c, device=dev)
        hip.to_s16(x32, rows, c, c, x, c)
        y = torch.empty(rows * c, device=dev)
        wgt = ((torch.rand(c * k * k, generator=g) * 2 - 1) / k).to(dev)
        b = (torch.rand(c, generator=g) * 2 - 1).to(dev)

        def run():
            hip.dwconv2d(x, c, n, h, w, c, k, wgt, b, y, c, in_fmt=hip.FMT_S16, out_fmt=hip.FMT_S16, residual=True, gelu=True)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        st = _stats([_timed(run) for _ in range(reps)])
        flops, nbytes = 2.0 * k * k * c * rows, 2.0 * 4 * c * rows
        t = st["median_us"] * 1e-6
        st.update({"layer": layer, "frames": n, "h": h, "w": w, "c": c, "k": k, "reps": reps, "gflop": round(flops / 1e9, 2),
                   "mbytes": round(nbytes / 1e6, 1), "valu_bound_us": round(1e6 * flops / VALU_PEAK, 1),
                   "hbm_bound_us": round(1e6 * nbytes / HBM_ACHIEVABLE, 1), "tflops": round(flops / t / 1e12, 2),
                   "pct_of_valu_peak": round(100 * flops / t / VALU_PEAK, 1),
                   "pct_of_hbm_achievable": round(100 * nbytes / t / HBM_ACHIEVABLE, 1)})
        out.append(st)
        del x32, x, y
    return out


def _processor(sk, T, depth):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    cfg = get_cfg()
    cfg.sk = sk
    work = tempfile.mkdtemp(prefix="vfml_sk_bench_")
    write_seeded_checkpoint(work, cfg, seed=0)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            proc = VideoFlowProcessor("cuda", sequence_length=T)
            proc.load_model()
    finally:
        os.chdir(cwd)
    assert proc.core.cfg.sk == sk
    proc.core.cfg.decoder_depth = depth
    return proc


def shares(H, W, T, depth, dev):
    """One eager field of an SK checkpoint, every launch the engine makes through vfml.hip between two events."""
    from vfml import hip
    from vfml.synth import synthetic_clip
    proc = _processor(True, T, depth)
    net = proc.core.model
    net.cfg.use_graph = False
    clip = torch.from_numpy(np.stack(synthetic_clip(T, H, W))).to(dev)
    net.forward_u8(clip)                    # (allocations, kernel attributes)
    torch.cuda.synchronize()
    rec, inside = [], [False]
    orig = {n: getattr(hip, n) for n in ("dwconv2d", "gelu_rows", "conv2d", "corr_lookup", "coords_update", "window_seed",
                                          "convex_upsample", "coords_init")}
    orig_block = net._pcblock

    def wrap(name, fn):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            cls = {"dwconv2d": "depthwise", "gelu_rows": "gelu"}.get(name) or ("pcblock dense 1x1" if name == "conv2d" and inside[0]
                                                                              else "other (encoders, volumes, lookups, tprop, mask, upsampling)")
            rec.append((cls, e0, e1))
            return r
        return f

    def block(*a, **kw):
        inside[0] = True
        try:
            return orig_block(*a, **kw)
        finally:
            inside[0] = False
    for n, fn in orig.items():
        setattr(hip, n, wrap(n, fn))
    net._pcblock = block
    try:
        total = _timed(lambda: net.forward_u8(clip))
    finally:
        for n, fn in orig.items():
            setattr(hip, n, fn)
        del net._pcblock
    torch.cuda.synchronize()
    out = {}
    for cls, e0, e1 in rec:
        d = out.setdefault(cls, {"launches": 0, "ms": 0.0})
        d["launches"] += 1
        d["ms"] += e0.elapsed_time(e1)
    timed = sum(d["ms"] for d in out.values())
    for d in out.values():
        d["ms"] = round(d["ms"], 3)
        d["share_of_timed_pct"] = round(100 * d["ms"] / timed, 1)
    net.release_workspace()
    return {"field_ms_eager_uncached": round(total, 2), "timed_launch_ms": round(timed, 2), "classes": out,
            "note": "one unkeyed window run eagerly: encoders and correlation volumes of all frames are in `other`; a launch's "
                    "time is between two events around it, so gaps between launches are in no class"}


def sliding(sk, H, W, T, depth, warm, K, dev):
    from vfml.runner import ClipFeeder, run_sharded
    from vfml.synth import synthetic_clip
    proc = _processor(sk, T, depth)
    half = T // 2
    fields = [half + i for i in range(warm + K)]
    clip = synthetic_clip(fields[-1] + half + 1, H, W)
    feeder = ClipFeeder(clip, dev)
    run_sharded(proc, None, fields[:warm], tile_mode=False, rank=0, world=1, feeder=feeder, collect=False)
    torch.cuda.synchronize()
    run_sharded(proc, None, fields[warm:], tile_mode=False, rank=0, world=1, feeder=feeder, prepare_only=True)
    out = np.zeros((K, H, W, 2), dtype=np.float32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_sharded(proc, None, fields[warm:], tile_mode=False, rank=0, world=1, feeder=feeder, out=out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(out).all()
    res = {"sk": sk, "precision": proc.core.cfg.precision, "fields": K, "fields_per_s": round(K / dt, 2),
           "ms_per_field": round(1000 * dt / K, 2), "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    proc.core.model.release_workspace()
    del proc, feeder
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--skip-sliding", action="store_true")
    ap.add_argument("--dwconv-only", action="store_true", help="part (a) alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sk_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sk_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0),
           "dwconv": dwconv_alone(args.seq - 2, args.height // 8, args.width // 8, args.reps, dev)}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    save()
    if args.dwconv_only:
        print(json.dumps(res))
        return
    torch.cuda.empty_cache()
    res["shares"] = shares(args.height, args.width, args.seq, args.depth, dev)
    save()
    torch.cuda.empty_cache()
    if not args.skip_sliding:
        res["sliding"] = []
        for sk in (False, True):
            res["sliding"].append(sliding(sk, args.height, args.width, args.seq, args.depth, args.warmup, args.steps, dev))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
