#!/usr/bin/env python3
"""What scene-cut detection costs on an MI355X, in one process:

  (a) vfml_scene_distances on one frame against a kept signature - the call a ClipFeeder makes behind every upload - at
      1080 x 1920 and 2160 x 3840, on a textured frame (vfml.synth) and on a frame of one colour (every pixel of a cell in one
      bin: the worst case for the LDS atomics).  The frames are slots of a ring larger than the Infinity Cache, visited in turn,
      so every call reads its frame from HBM; device events behind a warm-up, the four cases alternating, median and spread -
      each beside the time to read the frame's bytes once at HBM_BYTES_PER_S.
  (b) fields/s of a sliding 1080p depth-12 MOF job (T = 5) on a cut-free clip through the job loop bench.py times
      (vfml.runner.run_sharded with a fresh ClipFeeder per job, so every frame's upload - and with cuts on its measurement -
      falls inside the timed job), scene cuts off and on, alternating, three jobs each: what the feature costs where it
      finds nothing.

No pass mark: the figures are recorded.  Writes profiles/scene_cut_bench.json and prints it.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

HBM_BYTES_PER_S = 6.29e12       # measured float4 copy rate of an MI355X (8.0 TB/s is the specification's peak)
RING_BYTES = 600 << 20          # more than the 256 MB Infinity Cache
SIZES = ((1080, 1920), (2160, 3840))


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "p10_ms": round(ms[len(ms) // 10], 4), "p90_ms": round(ms[-1 - len(ms) // 10], 4), "n": len(ms)}


def kernel_alone(reps, dev):
    from vfml import hip
    from vfml.synth import synthetic_clip
    cases = {}
    for h, w in SIZES:
        slots = -(-RING_BYTES // (h * w * 3))
        textured = torch.from_numpy(synthetic_clip(1, h, w)[0]).to(dev)
        for name, frame in (("textured", textured), ("flat", torch.full((h, w, 3), 128, dtype=torch.uint8, device=dev))):
            ring = frame.unsqueeze(0).repeat(slots, 1, 1, 1).contiguous()
            sig = torch.empty((1, hip.SCENE_CELLS * hip.SCENE_BINS), dtype=torch.int32, device=dev)
            dist = torch.empty((1,), dtype=torch.int32, device=dev)
            prev = torch.zeros(hip.SCENE_CELLS * hip.SCENE_BINS, dtype=torch.int32, device=dev)
            cases[f"{h}x{w}_{name}"] = {"ring": ring, "out": (sig, dist), "prev": prev, "at": 0, "bytes": h * w * 3}

    def call(c):
        c["at"] = (c["at"] + 1) % c["ring"].shape[0]
        hip.scene_distances(c["ring"][c["at"]:c["at"] + 1], prev_sig=c["prev"], out=c["out"])

    for c in cases.values():
        for _ in range(3):
            call(c)
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(reps):                       # alternating: every figure sees the same neighbours on the machine
        for k, c in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(c)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "launches_per_call": "memset + 2 kernels"}
    for k, c in cases.items():
        floor = 1e3 * c["bytes"] / HBM_BYTES_PER_S
        res[k] = dict(_stats(times[k]), frame_bytes=c["bytes"], ring_slots=int(c["ring"].shape[0]),
                      hbm_read_once_ms=round(floor, 4))
        res[k]["times_the_read"] = round(res[k]["median_ms"] / floor, 2)
        assert int(c["out"][1].cpu().numpy().view(np.uint32)[0]) == c["bytes"] // 3      # against an empty signature: H W
    return res


def sliding(depth, fields, jobs, height, width, dev):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import build_network, get_cfg
    from vfml.runner import ClipFeeder, run_sharded
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.decoder_depth = depth
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    net.cuda().eval()
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.core.model = net
    clip = synthetic_clip(fields, height, width)                 # one continuous shot: nothing to find
    out = np.zeros((fields, height, width, 2), dtype=np.float32)
    feeders = {False: ClipFeeder(clip, dev), True: ClipFeeder(clip, dev, scene_cuts=(200, 3))}

    def job(cuts):
        feeders[cuts].reset(clip)                                # every frame goes up again inside the job
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_sharded(proc, None, range(fields), feeder=feeders[cuts], out=out)
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0) / fields

    job(False), job(True)                                        # warm-up: buffers, plans, the clocks
    ms = {False: [], True: []}
    for _ in range(jobs):
        for cuts in (False, True):
            ms[cuts].append(job(cuts))
    assert feeders[True].scenes.scene_of(fields - 1) == (0, fields)
    res = {"fields_per_job": fields, "jobs_each": jobs, "depth": depth, "size": [height, width], "order": "off, on alternating"}
    for cuts, key in ((False, "cuts_off"), (True, "cuts_on")):
        med = statistics.median(ms[cuts])
        res[key] = {"ms_per_field_jobs": [round(x, 3) for x in ms[cuts]], "ms_per_field": round(med, 3),
                    "fields_per_s": round(1000 / med, 2)}
    res["added_ms_per_field"] = round(res["cuts_on"]["ms_per_field"] - res["cuts_off"]["ms_per_field"], 3)
    res["spread_ms_per_field_cuts_off"] = round(max(ms[False]) - min(ms[False]), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--fields", type=int, default=24, help="fields (= frames) of one timed job")
    ap.add_argument("--jobs", type=int, default=3, help="timed jobs per setting")
    ap.add_argument("--skip-sliding", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_cut_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_cut_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_alone(args.reps, dev)}
    torch.cuda.empty_cache()
    if not args.skip_sliding:
        res["sliding"] = sliding(args.depth, args.fields, args.jobs, 1080, 1920, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
