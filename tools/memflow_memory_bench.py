#!/usr/bin/env python3
"""What MemFlow's memory bank costs on an MI355X, in one process, at 1080p and depth 12:

  (a) building the planes of one field at P = 32400 for banks of M = 0, 1, 2, 4 entries (hip.attention_bank_planes over
      M + 1 key sets; M = 0 beside hip.attention_plane, alternating), device events, median and spread;
  (b) R_mem, the bank's part of the read-out: per entry V^T to split rows, the long-K GEMM against its plane and the f32
      accumulation - once per field;
  (c) fields/s of a sliding job through the job loop bench.py times (vfml.runner.run_sharded: host frames in, fields in
      host memory out) for M = 0, 1, 2, 4: several timed windows one after the other behind a warm-up job, each going on
      with the bank the one before left (full from its first field - asserted), median and spread over the windows; M = 0 at
      VFML_PAIR_BATCH 1 and 3: the memory-free path a field at a time and as shipped - how much of a bank's cost is the
      lost pair batching;
  (d) bytes of planes the stream holds.

Writes profiles/memflow_memory_bench.json and prints it.
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
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))

import numpy as np      # noqa: E402
import torch            # noqa: E402

BANKS = (0, 1, 2, 4)


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
            "p10_ms": round(ms[len(ms) // 10], 3), "p90_ms": round(ms[-1 - len(ms) // 10], 3), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def planes_and_rmem(P, reps, dev):
    from vfml import hip, update_block
    from vfml.memflow_net import ATT_SCALE, MemFlowNetHIP
    AD = 128
    _, ldA, plain = MemFlowNetHIP._attention_geometry(P)
    assert plain
    g = torch.Generator().manual_seed(0)
    n_max = max(BANKS) + 1
    q = torch.randn(P * AD, generator=g).to(dev)
    keys = [torch.randn(P * AD, generator=g).to(dev) for _ in range(n_max)]
    vals = [torch.randn(P * AD, generator=g).to(dev) for _ in range(n_max)]
    planes = [hip.PlainWeight(P, ldA, dev, scale=ATT_SCALE) for _ in range(n_max)]
    ws = torch.empty(2 * P, device=dev)
    sc = 1.0 / AD ** 0.5
    s = types.SimpleNamespace(Pn=P, AF=hip.FMT_S16)
    ro = update_block.readout_scratch(lambda name, n, d: torch.empty(n, device=d), dev, P, P, AD, ldA, True)
    r_mem = torch.zeros(P * AD, device=dev)

    def build(n):
        return lambda: hip.attention_bank_planes(q, keys[:n], P, planes[:n], score_scale=sc, workspace=ws)

    def single():
        hip.attention_plane(q, keys[0], P, planes[0], score_scale=sc, workspace=ws)

    def rmem(n):
        def run():
            for j in range(n):
                update_block.plane_readout(s, planes[j], ldA, ro, vals[j])
                if j == 0:
                    r_mem.copy_(ro.out_t)
                else:
                    hip.axpy_f32(ro.out_t, r_mem, P * AD)
        return run

    fns = {"plane_single_call": single}
    for M in BANKS:
        fns[f"planes_M{M}"] = build(M + 1)
        if M:
            fns[f"rmem_M{M}"] = rmem(M)
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):                       # alternating: every figure sees the same neighbours on the machine
        for k, fn in fns.items():
            times[k].append(_timed(fn))
    res = {"P": P, "ld_plane": ldA, "plane_bytes": P * ldA * 2}
    res.update({k: _stats(v) for k, v in times.items()})
    for M in BANKS[1:]:
        res[f"planes_M{M}"]["ms_per_extra_plane"] = round(
            (res[f"planes_M{M}"]["median_ms"] - res["planes_M0"]["median_ms"]) / M, 3)
        res[f"rmem_M{M}"]["ms_per_entry"] = round(res[f"rmem_M{M}"]["median_ms"] / M, 3)
    return res


def sliding(M, pair_batch, clip, depth, warm, K, windows, dev):
    """`windows` timed jobs of K fields each, one after the other on one clip, behind a warm-up job of `warm` fields: every
    timed job goes on where the one before ended (run_sharded(..., continue_stream=True)), so with M <= warm each of them
    runs all its fields on a full bank and allocates nothing - asserted."""
    from processing.memflow_inference import MemFlowInference
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    from vfml.runner import ClipFeeder, run_sharded
    assert M <= warm and len(clip) == 2 + warm + windows * K
    H, W = clip[0].shape[:2]
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory(prefix="vfml_memflow_memory_bench_") as work:
        os.makedirs(os.path.join(work, "MemFlow_ckpt"))
        torch.save(seeded_memflow_state_dict(memflow_cfg(), 0), os.path.join(work, "MemFlow_ckpt", "MemFlowNet_sintel.pth"))
        os.chdir(work)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                eng = MemFlowInference("cuda", sequence_length=3, memory_frames=M)
                eng.load_model()
        finally:
            os.chdir(cwd)
    proc = eng.get_processor()
    core = proc.core_engine
    proc.PAIR_BATCH = pair_batch
    core.cfg.decoder_depth = depth
    fields = list(range(1, 1 + warm + windows * K))
    feeder = ClipFeeder(clip, dev)
    run_sharded(proc, None, fields[:warm], tile_mode=False, rank=0, world=1, feeder=feeder, collect=False)
    torch.cuda.synchronize()
    run_sharded(proc, None, fields[warm:warm + K], tile_mode=False, rank=0, world=1, feeder=feeder, prepare_only=True)
    out = np.zeros((K, H, W, 2), dtype=np.float32)
    out.fill(0.0)
    st = core.stream
    held = (st.planes_held, st.plane_bytes) if M else (0, 0)
    ms = []
    for n in range(windows):
        part = fields[warm + n * K:warm + (n + 1) * K]
        if M:
            assert core.stream is st and len(st.entries) == M, "the timed window must start on the warm-up's full bank"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_sharded(proc, None, part, tile_mode=False, rank=0, world=1, feeder=feeder, out=out, continue_stream=True)
        torch.cuda.synchronize()
        ms.append(1000 * (time.perf_counter() - t0) / K)
        assert np.isfinite(out).all()
        if M:       # the same stream all through: no field of the window started from an empty bank or took a new plane
            assert core.stream is st and len(st.entries) == M and (st.planes_held, st.plane_bytes) == held
            assert st.planes_in_use == M + 1 == st.planes_held
    med = statistics.median(ms)
    res = {"memory_frames": M, "pair_batch": pair_batch if M == 0 else 1, "fields_per_window": K, "windows": windows,
           "fields_per_s": round(1000 / med, 2), "ms_per_field": round(med, 2),
           "ms_per_field_windows": [round(x, 2) for x in ms],
           "fields_per_s_min": round(1000 / max(ms), 2), "fields_per_s_max": round(1000 / min(ms), 2),
           "bank_entries": len(st.entries) if M else 0, "planes_held": held[0], "plane_bytes_held": held[1],
           "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    core.model.release_workspace()
    del proc, core, eng, feeder, st
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=32400, help="P of parts (a) and (b)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=48, help="fields of one timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per figure, one after the other (median, min .. max)")
    ap.add_argument("--skip-sliding", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memflow_memory_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("memflow_memory_bench.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "planes": planes_and_rmem(args.cells, args.reps, dev)}

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
        for M, pb in [(0, 1), (0, 3)] + [(M, 1) for M in BANKS[1:]] + [(0, 3)]:     # (the yardstick twice: its spread)
            res["sliding"].append(sliding(M, pb, clip, args.depth, args.warmup, args.steps, args.windows, dev))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
