#!/usr/bin/env python3
"""GPU time of the flow cache's deflate and inflate per field (vfml_deflate_huffman / vfml_inflate_chunks, DESIGN.md
section 14) on a seeded field of smooth motion plus 0.05 px noise, with and without the reference's LOD levels, beside
zlib's Z_HUFFMAN_ONLY on one host core.  One JSON line.  Under `rocprofv3 --kernel-trace --stats -- python
tools/deflate_bench.py` the per-kernel times come out of the trace.

    python tools/deflate_bench.py [--size 1920x1080] [--reps 20]
"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    import deflate_oracle as do
    from vfml import hip
    dev = torch.device("cuda:0")
    field = do.flow_field(H, W, seed=0)
    levels = hip.flow_lods(torch.from_numpy(field).to(dev), 5)
    outs = [torch.empty(hip.deflate_capacity(t.numel() * 4), dtype=torch.uint8, device=dev) for t in levels]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    res = [None] * len(levels)

    def enc(n):
        for i in range(n):
            res[i] = hip.deflate(levels[i], 32768, 0, out=outs[i])

    ms_field = timed(lambda: enc(1))
    ms_lods = timed(lambda: enc(5))
    stream, crc, offsets = hip.deflate_stream(*res[0])
    raw = field.tobytes()
    assert zlib.decompress(stream, -15) == raw and crc == zlib.crc32(raw)
    data = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(dev)
    offs = torch.tensor(offsets, dtype=torch.int32, device=dev)
    back = [None]

    def dec():
        back[0] = hip.inflate(data, offs, 32768, len(raw))

    ms_inflate = timed(dec)
    assert back[0][0].cpu().numpy().tobytes() == raw and hip.inflate_check(back[0][1], crc) == crc
    t0 = time.perf_counter()
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    host = co.compress(raw) + co.flush()
    t1 = time.perf_counter()
    zlib.decompress(host, -15)
    t2 = time.perf_counter()
    print(json.dumps({"size": args.size, "raw_bytes": len(raw), "stream_bytes": len(stream), "host_stream_bytes": len(host),
                      "deflate_ms_field": round(ms_field, 4), "deflate_ms_field_and_lods_1_to_4": round(ms_lods, 4),
                      "inflate_ms_field": round(ms_inflate, 4), "host_deflate_ms": round(1e3 * (t1 - t0), 2),
                      "host_inflate_ms": round(1e3 * (t2 - t1), 2)}))


if __name__ == "__main__":
    main()
