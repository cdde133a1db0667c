"""Digests of the engines' output fields, and a census of the kernels they launch, on small seeded cases.

    python tests/golden/make_engine_digests.py [--tree DIR] [--out FILE]

runs on the GPU, imports `vfml` and `processing` from DIR/video-flow-ml_amd (default: the tree this file lies in) and writes
FILE (default: engine_digests.json beside this file): per case one SHA-1 per output tensor, over shape and bytes, and for
three cases {kernel variant: {layer shape: launches}} of one profiled run.  tests/test_gpu_engine_digests.py recomputes
every case on the working tree and requires the same digests and the same census: a change that is meant to move launches
around without changing them shows there that it did only that.

The committed file is recorded from the tree of the commit BEFORE a change of that kind, never from the code under test.
Record it again when a change alters the arithmetic or the order of launches on purpose, or when the toolchain changes
(compiler, HIP runtime, torch): in both cases from the parent of the commit that carries the new file, and twice in two
processes - a case whose two recordings differ is not reproducible and does not belong in the fixture.

Only public entry points are used (forward, forward_u8 through VideoFlowProcessor, forward_pairs, hip.profile_*), so that
the script runs unchanged on older trees."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTH = 4          # update iterations of every case that does not need another count


def digest(*tensors):
    """As tests_support._digest: SHA-1 over shape and bytes."""
    h = hashlib.sha1()
    for t in tensors:
        assert torch.isfinite(t).all(), "a field with a NaN or an infinity is no fixture"
        h.update(str(tuple(t.shape)).encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def frames(T, H, W):
    return torch.rand(1, T, 3, H, W, generator=torch.Generator().manual_seed(T * 1000 + H))


def mof_net(**over):
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.precision, cfg.decoder_depth = "f16x3", DEPTH
    for k, v in over.items():
        setattr(cfg, k, v)
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    return net.cuda().eval()


def memflow_net():
    from vfml.memflow_net import build_memflow_network, memflow_cfg, seeded_memflow_state_dict
    cfg = memflow_cfg()
    cfg.decoder_depth = DEPTH
    net = build_memflow_network(cfg)
    net.load_state_dict(seeded_memflow_state_dict(cfg, 0))
    return net.cuda().eval()


def mof_fields(T, H, W, **over):
    """Unkeyed `forward`: the field and the low-resolution flows."""
    flow, low = mof_net(**over)(frames(T, H, W).cuda(), {})
    return {"flow": digest(flow), "low": digest(low)}


def memflow_fields(B, H, W):
    low, flow = memflow_net().forward_pairs((frames(B + 1, H, W) * 2 - 1).cuda())
    return {"flow": digest(flow), "low": digest(low)}


def u8_clip(T, H, W):
    return (frames(T, H, W)[0] * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()


def sliding_job():
    """Case 3: a 9-frame clip through VideoFlowProcessor, every index, three passes - keyed caches, the context ring, cold
    and warm iteration 0, pick_only, the prefetch; the body eager (first pass), captured (second) and replayed (third)."""
    from processing.videoflow_processor import VideoFlowProcessor
    net = mof_net(precision="mixed", decoder_depth=12)
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=5)
    proc.core.model = net
    clip = u8_clip(9, 128, 192)
    out = {}
    for p in range(3):
        for i in range(clip.shape[0]):
            out[f"pass{p}.field{i}"] = digest(proc.compute_optical_flow_resident(clip, i))
    return out


def memflow_split_rows():
    """Case 12: the plane-sized frame with the probabilities kept as split rows."""
    from vfml import memflow_net as mn
    old = mn.ATT_PLAIN
    mn.ATT_PLAIN = False
    try:
        return memflow_fields(1, 256, 320)
    finally:
        mn.ATT_PLAIN = old


FAST = dict(decoder_depth=6, corr_levels=3, corr_radius=3)

CASES = {
    "01_mof_f16x3_T5_128x192": lambda: mof_fields(5, 128, 192),
    "02_mof_f32_T4_136x160": lambda: mof_fields(4, 136, 160, precision="f32"),
    "03_mof_mixed_sliding_job_9x128x192": sliding_job,
    "04_mof_two_tables_T7_128x128": lambda: mof_fields(7, 128, 128),
    "05_mof_depth0_T3_128x128": lambda: mof_fields(3, 128, 128, decoder_depth=0),
    "06_mof_fast_T3_128x160": lambda: mof_fields(3, 128, 160, **FAST),
    "07_bof_T9_128x160": lambda: mof_fields(9, 128, 160, network="BOFNet"),
    "08a_gma_plane_T5_256x264": lambda: mof_fields(5, 256, 264, gma=True),
    "08b_gma_rows_T3_136x152": lambda: mof_fields(3, 136, 152, gma=True),
    "09_gma_bof_T5_256x264": lambda: mof_fields(5, 256, 264, gma=True, network="BOFNet"),
    "10_sk_T3_136x152": lambda: mof_fields(3, 136, 152, sk=True),
    "11a_memflow_B3_256x320": lambda: memflow_fields(3, 256, 320),
    "11b_memflow_B1_128x192": lambda: memflow_fields(1, 128, 192),
    "12_memflow_split_rows_256x320": memflow_split_rows,
}


def census_of(run):
    """{kernel variant: {layer shape: launches}} of the convolutions, and the lookups, `run` launches."""
    from vfml import hip
    hip.profile_begin()
    try:
        run()
        hbm = hip.profile_end_hbm()
    finally:
        rec = hip.profile_end()
    out = {v: {s: d["launches"] for s, d in sorted(e["shapes"].items())} for v, e in sorted(rec.items())}
    out["corr_lookup"] = {"all": hbm.get("corr_lookup", {}).get("launches", 0)}
    return out


def _census_mixed_window():
    net = mof_net(precision="mixed", decoder_depth=12)
    clip = u8_clip(9, 128, 192)
    return census_of(lambda: net.forward_u8(clip[0:5]))


def _census_gma_plane():
    net, x = mof_net(gma=True), frames(5, 256, 264).cuda()
    return census_of(lambda: net(x, {}))


def _census_memflow():
    net, x = memflow_net(), (frames(4, 256, 320) * 2 - 1).cuda()
    return census_of(lambda: net.forward_pairs(x))


CENSUS = {
    "03_mof_mixed_one_window_unkeyed": _census_mixed_window,
    "08a_gma_plane_T5_256x264": _census_gma_plane,
    "11a_memflow_B3_256x320": _census_memflow,
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose video-flow-ml_amd is imported")
    ap.add_argument("--out", default=os.path.join(HERE, "engine_digests.json"))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    for p in (tree, os.path.join(tree, "video-flow-ml_amd")):
        sys.path.insert(0, p)
    import vfml
    assert os.path.abspath(vfml.__file__).startswith(tree + os.sep), (vfml.__file__, tree)
    out = {"digests": {}, "census": {}}
    for name, fn in CASES.items():
        out["digests"][name] = fn()
        print(f"[digests] {name}: {len(out['digests'][name])} tensors", flush=True)
    for name, fn in CENSUS.items():
        out["census"][name] = fn()
        print(f"[census] {name}: {sum(sum(s.values()) for s in out['census'][name].values())} launches", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"[digests] wrote {args.out}")


if __name__ == "__main__":
    main()
