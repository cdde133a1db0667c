#!/usr/bin/env python3
"""On-demand levels of the correlation pyramids (csrc/corr_ensure.hip) in numbers.  GPU only.

    python tools/corr_on_demand_probe.py job [--drift C] [--fields N] [--sets 0,01,012,dense] [--rounds R]
            a keyed sliding 1080p job, mixed plan, once per level set (0: level 0 alone on demand, 01: levels 0 and 1,
            012: levels 0, 1 and 2, dense: every level built whole), the sets alternating R times: ms per field of every
            run, and per level the tiles computed per new pyramid and their share of the level's tiles (C: tests_support
            drift_state_dict's c - 1 gives flows of ~13 cells)
    python tools/corr_on_demand_probe.py worst
            every tile of one 1080p pair requested by coordinates scattered over the image, for the level sets 0, 01 and
            012, against the dense launches of those levels (level 0 with its transposed twin)
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

SETS = {"0": (), "01": (1,), "012": (1, 2), "dense": None}      # -> net.corr_on_demand_levels (None: corr_on_demand off)
TILES_1080P = [255 * 510, 255 * 135, 255 * 38]                  # 128 x 64 tiles of a pyramid's f32 levels


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
    sets = args.sets.split(",")
    out = {"drift": args.drift, "fields": n - warm, "rounds": args.rounds, "ms_per_field": {s: [] for s in sets}}
    for _ in range(args.rounds):
        for name in sets:
            net.corr_on_demand = SETS[name] is not None
            net.corr_on_demand_levels = SETS[name] or ()
            net.clear_feature_cache()
            for i in range(2, 2 + warm):
                proc.compute_optical_flow_resident(clip, i)
            net.corr_level_tiles_computed()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(2 + warm, 2 + n):
                f = proc.compute_optical_flow_resident(clip, i)
            torch.cuda.synchronize()
            out["ms_per_field"][name].append(round(1000.0 * (time.perf_counter() - t0) / (n - warm), 3))
            tiles = net.corr_level_tiles_computed()
            if SETS[name] is not None:
                # a steady-state field brings one new frame: two new pyramids (newest centre -> new frame and back)
                per = [t / (2.0 * (n - warm)) for t in tiles[:3]]
                out["tiles_per_pyramid_" + name] = [round(p, 1) for p in per]
                out["share_of_level_" + name] = [round(p / full, 5) for p, full in zip(per, TILES_1080P)]
            out["max_abs_flow_px"] = round(float(f.abs().max()), 2)
    print(json.dumps(out))


def worst(args):
    from vfml import hip
    H, W, D, R, SC = 135, 240, 256, 4, 16.0
    vt = hip.VolTile(2, 3)
    hl, wl = [H >> l for l in range(3)], [W >> l for l in range(3)]
    Nl = [vt.count(hl[l], wl[l]) for l in range(3)]
    Pv, Pn = Nl[0], H * W
    ld = []
    for n in Nl:
        v = (n + 31) // 32 * 32
        ld.append(v if (v // 32) % 2 else v + 32)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows, planes = [], []
    for _ in range(2):
        f = vt.rows(torch.randn(Pn * D, device="cuda", generator=g), H, W, D)
        r = torch.empty(Pv * D, device="cuda")
        hip.to_s16(f * SC, Pv, D, D, r, D)
        rows.append(r)
        pl = [hip.SplitWeight(Pv, D, torch.device("cuda")).fill(f.contiguous(), scale=SC)]
        for l in (1, 2):       # (any values: the pooling is not what is timed)
            fl = vt.rows(torch.randn(hl[l] * wl[l] * D, device="cuda", generator=g), hl[l], wl[l], D)
            pl.append(hip.SplitWeight(Nl[l], D, torch.device("cuda")).fill(fl.contiguous(), scale=SC))
        planes.append(pl)
    vols = [[torch.empty(Pv * ld[l], device="cuda") for l in range(3)] for _ in range(2)]     # (0 -> 1, and its reverse)
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

    dense = [timed(lambda: hip.conv2d(rows[0], D, D, 1, 1, Pv, planes[1][0], None, Pv, 1, 1, vols[0][0], ld[0], out_scale=scale,
                                      in_fmt=hip.FMT_S16, out_t=vols[1][0], ld_out_t=ld[0], mfma=1), 3)]
    for l in (1, 2):           # both directions' launches of a pooled level
        def both(l=l):
            for q, t in ((0, 1), (1, 0)):
                hip.conv2d(rows[q], D, D, 1, 1, Pv, planes[t][l], None, Nl[l], 1, 1, vols[q][l], ld[l], out_scale=scale,
                           in_fmt=hip.FMT_S16, mfma=1)
        dense.append(timed(both, 3))
    out = {"dense_us": {"level0_with_twin": round(dense[0], 1), "level1_both": round(dense[1], 1),
                        "level2_both": round(dense[2], 1)}}
    counter = torch.zeros(4, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, levels in (("0", [0]), ("01", [0, 1]), ("012", [0, 1, 2])):
        words = [hip.corr_bitmap_words(Pv, Nl[l]) for l in levels]
        bits = [torch.zeros(sum(words), dtype=torch.int32, device="cuda") for _ in range(2)]
        cells = torch.zeros(64, dtype=torch.int64, device="cuda")
        ptrs = []
        for q, t in ((0, 1), (1, 0)):
            ptrs.append(rows[q])
            for j, l in enumerate(levels):
                ptrs += [planes[t][l].hi, vols[q][l], bits[q].data_ptr() + 4 * sum(words[:j])]
        hip.ptr_table_set(cells, ptrs)
        lv = [(l, planes[1][l], vols[0][l], Nl[l], ld[l], hl[l], wl[l]) for l in levels]
        total = sum(2 * (Pv // 128) * ((Nl[l] + 63) // 64) for l in levels)
        counter.zero_()
        gen = torch.Generator(device="cuda").manual_seed(2)
        us, done, passes, first = 0.0, 0, 0, None
        while done < total and passes < 40:
            c = torch.rand(Pn, 4, device="cuda", generator=gen) * torch.tensor([W, H, W, H], device="cuda")
            c = c.reshape(-1).contiguous()
            e0.record()
            hip.corr_levels_ensure(rows[0], D, Pv, lv, scale, cells, 1, 2, 1, c, 0, 4, 2, H, W, R, vt.code, counters=counter)
            e1.record()
            torch.cuda.synchronize()
            us += e0.elapsed_time(e1) * 1000.0
            per = counter.tolist()
            done = sum(per)
            passes += 1
            if passes == 1:
                first = (per[:3], e0.elapsed_time(e1) * 1000.0)
        out["levels_" + name] = {"tiles_of_both_directions": total, "tiles_computed": done, "passes": passes,
                                 "ensure_total_us": round(us, 1), "first_pass_tiles_per_level": first[0],
                                 "first_pass_us": round(first[1], 1),
                                 "dense_us": round(sum(dense[l] for l in levels), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["job", "worst"])
    ap.add_argument("--drift", type=float, default=0.0)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--sets", default="0,01,012,dense")
    ap.add_argument("--rounds", type=int, default=1)
    a = ap.parse_args()
    job(a) if a.what == "job" else worst(a)
