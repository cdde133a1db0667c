#!/usr/bin/env python3
"""The lookup's patch cache (csrc/flow_ops.hip corr_lookup_fixed_kernel<.., CACHED = true>) in numbers.  GPU only.

    python tools/lookup_cache_probe.py [--drift 0,1] [--fields N] [--rounds R]
            a keyed sliding 1080p job, mixed plan, per clip (drift C: tests_support.drift_state_dict's c - 0 is the
            benchmark clip with the seeded weights, flows below a cell; 1 gives flows of ~13 cells):
              hit_share       per update iteration, the share of the lookup's queries whose patch was read back, over the
                              steady-state fields of the job (MOFNetHIP.lookup_cache_count)
              lookup_us       per update iteration, microseconds per lookup launch with the cache on and off, from events
                              around the eager launches of the same fields (graph replay off), the two alternating R times
              ms_per_field    of the replayed job with the cache on and off (no counters), alternating R times
One JSON line per clip."""
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

WARM = 6                # fields until buffers, graphs and the sliding window's caches are in their steady state


def _net(drift, graph):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.precision = "mixed"
    cfg.use_graph = graph
    sd = seeded_state_dict(cfg, 0)
    if drift:
        import tests_support as ts
        sd = ts.drift_state_dict(sd, drift)
    net = build_network(cfg)
    net.load_state_dict(sd)
    net.cuda().eval()
    return net


def _proc(net):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.core.model = net
    return proc


def _fields(proc, clip, lo, hi):
    for i in range(lo, hi):
        proc.compute_optical_flow_resident(clip, i)
    torch.cuda.synchronize()


def clip_numbers(drift, args, clip):
    from vfml import hip
    n = args.fields
    out = {"drift": drift, "fields": n, "rounds": args.rounds}
    # ---- hit share per iteration, and field time, on the replayed job
    net = _net(drift, True)
    proc = _proc(net)
    depth = net.cfg.decoder_depth
    net.lookup_cache, net.lookup_cache_count = True, True
    _fields(proc, clip, 2, 2 + WARM)
    net.lookup_cache_counts()
    _fields(proc, clip, 2 + WARM, 2 + WARM + n)
    counts = net.lookup_cache_counts()
    out["queries_per_field"] = [(h + m) // n for h, m in counts]
    out["hit_share"] = [round(h / max(1, h + m), 4) for h, m in counts]
    net.lookup_cache_count = False
    ms = {"on": [], "off": []}
    for _ in range(args.rounds):
        for name in ("on", "off"):
            net.lookup_cache = name == "on"
            net.clear_feature_cache()
            _fields(proc, clip, 2, 2 + WARM)
            t0 = time.perf_counter()
            _fields(proc, clip, 2 + WARM, 2 + WARM + n)
            ms[name].append(round((time.perf_counter() - t0) * 1e3 / n, 3))
    out["ms_per_field"] = ms
    del net, proc
    torch.cuda.empty_cache()
    # ---- microseconds per lookup launch, eager, events around every launch
    net = _net(drift, False)
    proc = _proc(net)
    os.environ["VFML_PREFETCH"] = "0"          # (no encoder of the next window beside the timed launches)
    us ={"on": [[] for _ in range(depth)], "off": [[] for _ in range(depth)]}
    for _ in range(args.rounds):
        for name in ("on", "off"):
            net.lookup_cache = name == "on"
            net.clear_feature_cache()
            _fields(proc, clip, 2, 2 + WARM)
            for i in range(2 + WARM, 2 + WARM + n):
                hip.profile_begin()
                proc.compute_optical_flow_resident(clip, i)
                torch.cuda.synchronize()
                rec = [e0.elapsed_time(e1) * 1e3 for k, _, e0, e1 in hip._PROFILE_HBM if k == "corr_lookup"]
                hip.profile_end()
                if len(rec) == depth:
                    for it, v in enumerate(rec):
                        us[name][it].append(v)
    os.environ.pop("VFML_PREFETCH")
    out["lookup_us"] = {k: [round(float(np.median(v)), 1) if v else None for v in per] for k, per in us.items()}
    out["lookup_us_per_field"] = {k: round(sum(v for v in per if v is not None), 1) for k, per in out["lookup_us"].items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--drift", default="0,1")
    ap.add_argument("--fields", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lookup_cache_probe: needs a GPU")
    from vfml.synth import synthetic_clip
    clip = torch.from_numpy(np.stack(synthetic_clip(args.fields + WARM + 4, 1080, 1920))).cuda()
    for d in args.drift.split(","):
        print(json.dumps(clip_numbers(float(d), args, clip)), flush=True)


if __name__ == "__main__":
    main()
