"""Writes tests/golden/memflow_memory.json: sampled values of the memory oracle's fields (tests/memflow_memory_oracle.py) on
the fixture clip at 128 x 192, depth 12, seed-0 weights, banks of 0, 1 and 2 entries.  Run from the repository root:
    python tests/golden/make_memflow_memory_fixture.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-flow-ml_amd"), os.path.join(ROOT, "tests")]

SAMPLES = [(0, 0), (17, 40), (64, 96), (100, 5), (127, 191)]       # (y, x)


def main():
    import torch
    import memflow_memory_oracle as mo
    from oracle import memflow_oracle as mm
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    ora = mm.build_network(mm.get_cfg())
    ora.load_state_dict(seeded_memflow_state_dict(memflow_cfg(), 0))
    ora.eval()
    clip = mo.fixture_clip(128, 192)
    out = {"size": [128, 192], "samples": SAMPLES, "fields": {}}
    for M in (0, 1, 2):
        rows = []
        for _, up in mo.run_fields(ora, clip, M):
            rows.append({"at": [[float(up[0, c, y, x]) for c in (0, 1)] for y, x in SAMPLES],
                         "mean_abs": float(up.abs().mean()), "mean": [float(up[0, c].mean()) for c in (0, 1)]})
        out["fields"][str(M)] = rows
    with open(os.path.join(HERE, "memflow_memory.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
