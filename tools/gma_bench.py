#!/usr/bin/env python3
"""What the GMA aggregator costs on an MI355X, in one process:

  (a) building one frame's attention plane at P = 32400 (1080p): the fused kernel (hip.attention_plane) against the
      two-call path (score GEMM to f32 + row softmax to f16), alternating, device events, median and spread;
  (b) one read-out (V^T to split rows, the long-K GEMM against the plane, the residual add);
  (c) fields/s of a sliding 1080p seq-5 depth-12 job with a seeded GMA checkpoint and with a plain one, through the
      job loop bench.py times (vfml.runner.run_sharded: host frames in, fields in host memory out).

Writes profiles/gma_bench.json and prints it.
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


def plane_and_readout(P, reps, dev):
    from vfml import hip
    from vfml.network import ATT_SCALE, MOFNetHIP
    AD = 128
    _, ldA, plain = MOFNetHIP._attention_geometry(P)
    assert plain
    g = torch.Generator().manual_seed(0)
    q = torch.randn(P * AD, generator=g).to(dev)
    k = torch.randn(P * AD, generator=g).to(dev)
    q16 = torch.empty(P * AD, device=dev)
    hip.to_s16(q, P, AD, AD, q16, AD)
    kw = hip.SplitWeight(P, AD, dev)
    scores = torch.empty(P * ldA, device=dev)
    a_two, a_new = hip.PlainWeight(P, ldA, dev, scale=ATT_SCALE), hip.PlainWeight(P, ldA, dev, scale=ATT_SCALE)
    ws = torch.empty(2 * P, device=dev)
    sc = 1.0 / AD ** 0.5

    def two_call(split_q=False):
        # (in the engine q leaves to_qk as split rows, so the two-call build never pays for splitting it; the fused kernel splits
        # both operands itself - "two_call_with_q_split" is the like-for-like figure from f32 q and k)
        if split_q:
            hip.to_s16(q, P, AD, AD, q16, AD)
        kw.fill(k, scale=16.0)
        hip.conv2d(q16, AD, AD, 1, 1, P, kw, None, P, 1, 1, scores, ldA, out_scale=sc, in_fmt=hip.FMT_S16)
        hip.softmax_rows_f16(scores, P, P, ldA, a_two)

    def fused():
        hip.attention_plane(q, k, P, a_new, score_scale=sc, workspace=ws)

    for _ in range(3):
        two_call()
        fused()
    torch.cuda.synchronize()
    t_two, t_twoq, t_new = [], [], []
    for _ in range(reps):
        t_two.append(_timed(two_call))
        t_new.append(_timed(fused))
        t_twoq.append(_timed(lambda: two_call(True)))
    # the two planes against one another (f16 probabilities times 2^14)
    diff = (a_two.hi.view(P, ldA)[:256].float() - a_new.hi.view(P, ldA)[:256].float()).abs().sum(1).max().item() / ATT_SCALE

    val = torch.randn(P * AD, generator=g).to(dev)
    G = torch.zeros(P * 896, device=dev)
    vrows = torch.empty(AD * ldA, device=dev)
    ro = torch.empty(AD * ldA, device=dev)
    ro_t = torch.empty(P * AD, device=dev)
    ro_ws = torch.empty(AD * ldA + P * AD, device=dev)

    def readout():
        hip.transpose_to_s16(val, P, AD, AD, vrows, ldA, scale=16.0)
        hip.conv2d(vrows, ldA, ldA, AD, 1, 1, a_new, None, P, 1, 1, ro, ldA, out_scale=1.0 / 16.0, in_fmt=hip.FMT_S16,
                   out_t=ro_t, ld_out_t=AD, mfma=1, ksplit_ws=ro_ws)
        hip.add_to_s16(ro_t, AD, G, 896, G, 896, P, AD, scale=0.5, aux_off=512, out_off=768)

    for _ in range(3):
        readout()
    torch.cuda.synchronize()
    t_ro = [_timed(readout) for _ in range(reps)]
    return {"P": P, "ld_plane": ldA, "two_call": _stats(t_two), "two_call_with_q_split": _stats(t_twoq), "fused": _stats(t_new),
            "row_l1_between_the_two_planes_first_256_rows": diff, "readout": _stats(t_ro)}


def sliding(gma, H, W, T, depth, warm, K, dev):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import get_cfg
    from vfml.runner import ClipFeeder, run_sharded
    from vfml.synth import synthetic_clip
    from vfml.weights import write_seeded_checkpoint
    cfg = get_cfg()
    cfg.gma = gma
    work = tempfile.mkdtemp(prefix="vfml_gma_bench_")
    write_seeded_checkpoint(work, cfg, seed=0)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            proc = VideoFlowProcessor("cuda", sequence_length=T)
            proc.load_model()
    finally:
        os.chdir(cwd)
    assert proc.core.cfg.gma == gma
    proc.core.cfg.decoder_depth = depth
    half = T // 2
    fields = [half + i for i in range(warm + K)]
    clip = synthetic_clip(fields[-1] + half + 1, H, W)
    feeder = ClipFeeder(clip, dev)
    run_sharded(proc, None, fields[:warm], tile_mode=False, rank=0, world=1, feeder=feeder, collect=False)
    torch.cuda.synchronize()
    run_sharded(proc, None, fields[warm:], tile_mode=False, rank=0, world=1, feeder=feeder, prepare_only=True)
    out = np.zeros((K, H, W, 2), dtype=np.float32)
    out.fill(0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_sharded(proc, None, fields[warm:], tile_mode=False, rank=0, world=1, feeder=feeder, out=out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(out).all()
    res = {"gma": gma, "precision": proc.core.cfg.precision, "fields": K, "fields_per_s": round(K / dt, 2),
           "ms_per_field": round(1000 * dt / K, 2), "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    proc.core.model.release_workspace()
    del proc, feeder
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=32400, help="P of parts (a) and (b)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--seq", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--skip-sliding", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gma_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gma_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "plane": plane_and_readout(args.cells, args.reps, dev)}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    save()
    torch.cuda.empty_cache()
    if not args.skip_sliding:
        res["sliding"] = []
        for g in (False, True):
            res["sliding"].append(sliding(g, args.height, args.width, args.seq, args.depth, args.warmup, args.steps, dev))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
