#!/usr/bin/env python3
"""What the warm start of a MemFlow stream costs on an MI355X, in one process:

  (a) vfml_flow_forward_interpolate alone at 135 x 240 (1080p) and 270 x 480 (4K) cells, on random flows of sigma = 0.5 and
      sigma = 20 cells (at 20 most sources leave the frame), input and output rows of 4 floats as the stream calls it, index map
      on: device events behind a warm-up, alternating, median and spread - each beside the arithmetic bound of its P^2 distance
      evaluations at VALU_OPS vector-ALU instructions each (the inner loop as compiled: two subtractions, two multiplications,
      an addition, a comparison, two selects and the index move) on 32 lanes per SIMD and cycle at 2.4 GHz;
  (b) fields/s of a sliding 1080p depth-12 job through the job loop bench.py times (vfml.runner.run_sharded), warm start off
      and on, for M = 0 (a field per pass: VFML_PAIR_BATCH 1 - a stream cannot batch pairs) and M = 1: timed windows one after
      the other behind a warm-up job, as tools/memflow_memory_bench.py; the added milliseconds per field.

Writes profiles/memflow_warm_bench.json and prints it.
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

VALU_OPS = 9            # per (target, source) pair in forward_interpolate_search_kernel's inner loop
CLOCK_HZ = 2.4e9
LANES_PER_SIMD_CYCLE = 32
GRIDS = ((135, 240), (270, 480))
SIGMAS = (0.5, 20.0)


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "p10_ms": round(ms[len(ms) // 10], 4), "p90_ms": round(ms[-1 - len(ms) // 10], 4), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_alone(reps, dev):
    from vfml import hip
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lane_ops_per_s = cus * 4 * LANES_PER_SIMD_CYCLE * CLOCK_HZ
    fns, meta = {}, {}
    for h, w in GRIDS:
        P = h * w
        ws = hip.flow_forward_interpolate_workspace(1, h, w, dev)
        out = torch.empty(P * 4, device=dev)
        idx = torch.empty(P, dtype=torch.int32, device=dev)
        for sigma in SIGMAS:
            g = torch.Generator().manual_seed(int(sigma * 10) + h)
            flow = torch.zeros(P, 4)
            flow[:, :2] = torch.randn(P, 2, generator=g) * sigma
            flow = flow.view(-1).to(dev)
            key = f"{h}x{w}_sigma{sigma:g}"
            fns[key] = (lambda f=flow, h=h, w=w, o=out, i=idx, s=ws:
                        hip.flow_forward_interpolate(f, h, w, ld_in=4, out=o, ld_out=4, index=i, workspace=s))
            fns[key]()
            torch.cuda.synchronize()
            meta[key] = {"cells": P, "sources_chosen": int(torch.unique(idx[idx >= 0]).numel()),
                         "pairs": P * P, "workspace_bytes": ws.numel() * 8,
                         "valu_bound_ms": round(1e3 * P * P * VALU_OPS / lane_ops_per_s, 4)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):                       # alternating: every figure sees the same neighbours on the machine
        for k, fn in fns.items():
            times[k].append(_timed(fn))
    res = {"compute_units": cus, "valu_ops_per_pair": VALU_OPS, "clock_hz": CLOCK_HZ}
    for k in fns:
        res[k] = dict(meta[k], **_stats(times[k]))
        res[k]["times_the_bound"] = round(res[k]["median_ms"] / res[k]["valu_bound_ms"], 2)
    return res


def sliding(M, warm_start, clip, depth, warm, K, windows, dev):
    """`windows` timed jobs of K fields each, one after the other on one clip, behind a warm-up job of `warm` fields; every timed
    job goes on where the one before ended (continue_stream=True), so a streaming configuration never starts a field cold or
    on a bank that is not full - asserted."""
    from processing.memflow_inference import MemFlowInference
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    from vfml.runner import ClipFeeder, run_sharded
    assert M <= warm and len(clip) == 2 + warm + windows * K
    H, W = clip[0].shape[:2]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory(prefix="vfml_memflow_warm_bench_") as work:
        os.makedirs(os.path.join(work, "MemFlow_ckpt"))
        torch.save(seeded_memflow_state_dict(memflow_cfg(), 0), os.path.join(work, "MemFlow_ckpt", "MemFlowNet_sintel.pth"))
        os.chdir(work)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                eng = MemFlowInference("cuda", sequence_length=3, memory_frames=M, warm_start=warm_start)
                eng.load_model()
        finally:
            os.chdir(cwd)
    proc = eng.get_processor()
    core = proc.core_engine
    proc.PAIR_BATCH = 1                         # a field per pass in every configuration: what a stream runs
    core.cfg.decoder_depth = depth
    fields = list(range(1, 1 + warm + windows * K))
    feeder = ClipFeeder(clip, dev)
    run_sharded(proc, None, fields[:warm], tile_mode=False, rank=0, world=1, feeder=feeder, collect=False)
    torch.cuda.synchronize()
    run_sharded(proc, None, fields[warm:warm + K], tile_mode=False, rank=0, world=1, feeder=feeder, prepare_only=True)
    out = np.zeros((K, H, W, 2), dtype=np.float32)
    out.fill(0.0)
    st = core.stream
    ms = []
    for n in range(windows):
        part = fields[warm + n * K:warm + (n + 1) * K]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_sharded(proc, None, part, tile_mode=False, rank=0, world=1, feeder=feeder, out=out, continue_stream=True)
        torch.cuda.synchronize()
        ms.append(1000 * (time.perf_counter() - t0) / K)
        assert np.isfinite(out).all()
        if M or warm_start:
            assert core.stream is st and len(st.entries) == M
            assert (st.flow_index is not None) == warm_start and (st.flow_size == (H, W)) == warm_start
    med = statistics.median(ms)
    res = {"memory_frames": M, "warm_start": warm_start, "fields_per_window": K, "windows": windows,
           "fields_per_s": round(1000 / med, 2), "ms_per_field": round(med, 2), "ms_per_field_windows": [round(x, 2) for x in ms],
           "fields_per_s_min": round(1000 / max(ms), 2), "fields_per_s_max": round(1000 / min(ms), 2),
           "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    core.model.release_workspace()
    del proc, core, eng, feeder, st
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32, help="fields of one timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure, one after the other (median, min .. max)")
    ap.add_argument("--skip-sliding", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memflow_warm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("memflow_warm_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_alone(args.reps, dev)}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    save()
    torch.cuda.empty_cache()
    if not args.skip_sliding:
        from vfml.synth import synthetic_clip
        res["sliding"] = []
        clip = synthetic_clip(2 + args.warmup + args.windows * args.steps, args.height, args.width)   # (once: host work)
        for M, ws in [(0, False), (0, True), (1, False), (1, True), (0, False)]:      # (the yardstick twice: its spread)
            res["sliding"].append(sliding(M, ws, clip, args.depth, args.warmup, args.steps, args.windows, dev))
            save()
        by = {(r["memory_frames"], r["warm_start"]): r for r in res["sliding"][:4]}
        res["added_ms_per_field"] = {f"M{M}": round(by[(M, True)]["ms_per_field"] - by[(M, False)]["ms_per_field"], 2) for M in (0, 1)}
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
