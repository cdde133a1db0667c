#!/usr/bin/env python3
"""What the Twins-SVT encoders cost on an MI355X, in one process:

  (a) where a new frame's encoder time goes: `_twins_encoder` on ONE 1080p frame, run eagerly with every launch the engine
      makes through vfml.hip between two events, summed per class - the three new kernels (layernorm_rows, window_attention,
      attention_shared_keys), the dense layers (vfml_conv2d_split), the rest (position encoding, GELU, the split of the
      frames); the space-to-depth copies are torch's and show up only in the call's total;
  (b) vfml_attention_shared_keys alone at the two shapes of a 1080p frame: device events, warm-up, median and spread, achieved
      TFLOP/s (4 p pk c FLOP per frame: two products of 2 p pk 32 per head) against the f32 matrix peak;
  (c) fields/s of a sliding 1080p seq-5 depth-12 job with a seeded Twins checkpoint and with a plain one, through the job loop
      bench.py times (vfml.runner.run_sharded: host frames in, fields in host memory out).

Writes profiles/twins_bench.json and prints it.
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

F32_MATRIX_PEAK = 155e12        # FLOP/s of v_mfma_f32_32x32x2_f32, as measured on the part


def _stats(ms):
    ms = sorted(ms)
    return {"median_us": round(1000 * statistics.median(ms), 1), "min_us": round(1000 * ms[0], 1),
            "max_us": round(1000 * ms[-1], 1), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _processor(twins, T, depth):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import get_cfg
    from vfml.weights import write_seeded_checkpoint
    cfg = get_cfg()
    cfg.twins = twins
    work = tempfile.mkdtemp(prefix="vfml_twins_bench_")
    write_seeded_checkpoint(work, cfg, seed=0)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            proc = VideoFlowProcessor("cuda", sequence_length=T)
            proc.load_model()
    finally:
        os.chdir(cwd)
    assert proc.core.cfg.twins == twins
    proc.core.cfg.decoder_depth = depth
    return proc


CLASSES = {"layernorm_rows": "layernorm_rows", "window_attention": "window_attention",
           "attention_shared_keys": "attention_shared_keys", "conv2d": "dense layers (vfml_conv2d_split)"}
OTHER = "other (position encoding, GELU, split of the frames)"


def encoder_shares(H, W, T, depth, dev):
    """One new frame through the feature encoder, per class of launch."""
    from vfml import hip
    proc = _processor(True, T, depth)
    net = proc.core.model
    P = net._pack(dev)
    frames = torch.rand(H * W * 4, device=dev) * 2 - 1
    h, w = H // 8, W // 8
    out = torch.empty(h * w * 256, device=dev)

    def run():
        net._twins_encoder("fnet", frames, 1, H, W, P, dev, out, 256, 0, hip.EPI_NONE, 0)
    run()                                   # (allocations, kernel attributes)
    torch.cuda.synchronize()
    rec = []
    names = ("layernorm_rows", "window_attention", "attention_shared_keys", "conv2d", "dwconv2d", "gelu_rows", "to_s16")
    orig = {n: getattr(hip, n) for n in names}

    def wrap(name, fn):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            rec.append((CLASSES.get(name, OTHER), e0, e1))
            return r
        return f
    for n, fn in orig.items():
        setattr(hip, n, wrap(n, fn))
    try:
        total = _timed(run)
    finally:
        for n, fn in orig.items():
            setattr(hip, n, fn)
    torch.cuda.synchronize()
    cls = {}
    for c, e0, e1 in rec:
        d = cls.setdefault(c, {"launches": 0, "ms": 0.0})
        d["launches"] += 1
        d["ms"] += e0.elapsed_time(e1)
    timed = sum(d["ms"] for d in cls.values())
    for d in cls.values():
        d["ms"] = round(d["ms"], 3)
        d["share_of_timed_pct"] = round(100 * d["ms"] / timed, 1)
    untimed = total - timed
    net.release_workspace()
    return {"encoder_ms_per_new_frame": round(total, 3), "timed_launch_ms": round(timed, 3),
            "space_to_depth_copies_and_gaps_ms": round(untimed, 3), "classes": cls,
            "note": "fnet on one frame, eager; a window's first field encodes T frames with fnet and T - 2 with cnet, a sliding "
                    "job's later fields one frame with each"}


def shared_keys_alone(H, W, reps, dev):
    from vfml import hip
    out = []
    g = torch.Generator().manual_seed(0)
    for stage, (div, c, heads, sr) in enumerate(((4, 128, 4, 8), (8, 256, 8, 4))):
        h, w = H // div, W // div
        p, pk = h * w, (h // sr) * (w // sr)
        q = torch.randn(p * c, generator=g).to(dev)
        kv = torch.randn(pk * 2 * c, generator=g).to(dev)
        y = torch.empty(p * c, device=dev)

        def run():
            hip.attention_shared_keys(q, c, kv, 2 * c, 1, p, pk, c, heads, y, c, out_fmt=hip.FMT_S16)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        st = _stats([_timed(run) for _ in range(reps)])
        flops = 4.0 * p * pk * c
        t = st["median_us"] * 1e-6
        st.update({"stage": stage, "p": p, "pk": pk, "c": c, "heads": heads, "gflop": round(flops / 1e9, 1),
                   "tflops": round(flops / t / 1e12, 1), "pct_of_f32_matrix_peak": round(100 * flops / t / F32_MATRIX_PEAK, 1)})
        out.append(st)
    return out


def sliding(twins, H, W, T, depth, warm, K, dev):
    from vfml.runner import ClipFeeder, run_sharded
    from vfml.synth import synthetic_clip
    proc = _processor(twins, T, depth)
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
    res = {"twins": twins, "precision": proc.core.cfg.precision, "fields": K, "fields_per_s": round(K / dt, 2),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twins_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("twins_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "height": args.height, "width": args.width, "seq": args.seq,
           "depth": args.depth, "warmup": args.warmup, "steps": args.steps, "f32_matrix_peak_tflops": F32_MATRIX_PEAK / 1e12}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    res["attention_shared_keys"] = shared_keys_alone(args.height, args.width, args.reps, dev)
    save()
    res["encoder"] = encoder_shares(args.height, args.width, args.seq, args.depth, dev)
    save()
    torch.cuda.empty_cache()
    if not args.skip_sliding:
        res["sliding"] = []
        for twins in (False, True):
            res["sliding"].append(sliding(twins, args.height, args.width, args.seq, args.depth, args.warmup, args.steps, dev))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
