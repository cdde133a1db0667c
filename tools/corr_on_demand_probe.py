#!/usr/bin/env python3
"""On-demand level 0 of the correlation pyramids (csrc/corr_ensure.hip) in numbers.  GPU only.

    python tools/corr_on_demand_probe.py job [--drift C] [--fields N]   a keyed sliding 1080p job, mixed plan: ms per field and
                                                                        the fraction of a pair's level-0 tiles computed, on
                                                                        demand and with the dense build (C: tests_support
                                                                        drift_state_dict's c - 1 gives flows of ~13 cells)
    python tools/corr_on_demand_probe.py worst                          every tile of one 1080p pair requested by coordinates
                                                                        scattered over the image, against the dense launch
                                                                        with its transposed twin
One JSON line each."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-flow-ml_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def job(args):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import build_network, get_cfg
    from vfml.synth import synthetic_clip
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.precision = "mixed"
    sd = seeded_state_dict(cfg, 0)
    if args.drift:
        import tests_support as ts
        sd = ts.drift_state_dict(sd, args.drift)
    net = build_network(cfg)
    net.load_state_dict(sd)
    net.cuda().eval()
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.core.model = net
    n, warm = args.fields, 6
    clip = torch.from_numpy(np.stack(synthetic_clip(n + 4, 1080, 1920))).cuda()
    out = {"drift": args.drift, "fields": n - warm}
    for mode in (True, False):
        net.corr_on_demand = mode
        net.clear_feature_cache()
        for i in range(2, 2 + warm):
            proc.compute_optical_flow_resident(clip, i)
        net.corr_tiles_computed()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(2 + warm, 2 + n):
            f = proc.compute_optical_flow_resident(clip, i)
        torch.cuda.synchronize()
        ms = 1000.0 * (time.perf_counter() - t0) / (n - warm)
        tiles = net.corr_tiles_computed()
        key = "on_demand" if mode else "dense"
        out[key + "_ms_per_field"] = round(ms, 3)
        if mode:
            # a steady-state field brings one new frame: two new pairs (newest centre -> new frame and back)
            out["tiles_per_pair"] = round(tiles / (2.0 * (n - warm)), 1)
            out["fraction_of_pair"] = round(tiles / (2.0 * (n - warm)) / (255 * 510), 5)
        out[key + "_max_abs_flow_px"] = round(float(f.abs().max()), 2)
    print(json.dumps(out))


def worst(args):
    from vfml import hip
    H, W, D, R, SC = 135, 240, 256, 4, 16.0
    vt = hip.VolTile(2, 3)
    Pv, Pn = vt.count(H, W), H * W
    ld = (Pv + 31) // 32 * 32
    ld = ld if (ld // 32) % 2 else ld + 32
    g = torch.Generator(device="cuda").manual_seed(1)
    ops = []
    for _ in range(2):
        f = vt.rows(torch.randn(Pn * D, device="cuda", generator=g), H, W, D)
        r = torch.empty(Pv * D, device="cuda")
        hip.to_s16(f * SC, Pv, D, D, r, D)
        ops.append((r, hip.SplitWeight(Pv, D, torch.device("cuda")).fill(f.contiguous(), scale=SC)))
    vol, twin = torch.empty(Pv * ld, device="cuda"), torch.empty(Pv * ld, device="cuda")
    scale = 1.0 / 16.0 / SC

    def timed(fn, reps):
        fn()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        e[0].record()
        for i in range(reps):
            fn()
            e[i + 1].record()
        torch.cuda.synchronize()
        return min(e[i].elapsed_time(e[i + 1]) for i in range(reps)) * 1000.0

    dense = timed(lambda: hip.conv2d(ops[0][0], D, D, 1, 1, Pv, ops[1][1], None, Pv, 1, 1, vol, ld, out_scale=scale,
                                     in_fmt=hip.FMT_S16, out_t=twin, ld_out_t=ld, mfma=1), 3)
    bits = [torch.zeros(hip.corr_bitmap_words(Pv, Pv), dtype=torch.int32, device="cuda") for _ in range(2)]
    cells = torch.zeros(64, dtype=torch.int64, device="cuda")
    hip.ptr_table_set(cells, [ops[0][0], ops[1][1].hi, vol, bits[0], ops[1][0], ops[0][1].hi, twin, bits[1]])
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    total = 2 * (Pv // 128) * ((Pv + 63) // 64)
    us, done, passes = 0.0, 0, 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while done < total and passes < 40:
        c = torch.rand(Pn, 4, device="cuda", generator=g) * torch.tensor([W, H, W, H], device="cuda")
        e0.record()
        hip.corr_level0_ensure(ops[0][0], D, ops[1][1], vol, Pv, Pv, ld, scale, cells, 1, 2, 1, c.reshape(-1).contiguous(), 0,
                               4, 2, H, W, R, vt.code, counter=counter)
        e1.record()
        torch.cuda.synchronize()
        us += e0.elapsed_time(e1) * 1000.0
        done = int(counter.item())
        passes += 1
        if passes == 1:
            first = (done, e0.elapsed_time(e1) * 1000.0)
    print(json.dumps({"dense_with_twin_us": round(dense, 1), "tiles_of_both_directions": total, "tiles_computed": done,
                      "passes": passes, "ensure_total_us": round(us, 1), "first_pass_tiles": first[0],
                      "first_pass_us": round(first[1], 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["job", "worst"])
    ap.add_argument("--drift", type=float, default=0.0)
    ap.add_argument("--fields", type=int, default=26)
    a = ap.parse_args()
    job(a) if a.what == "job" else worst(a)
