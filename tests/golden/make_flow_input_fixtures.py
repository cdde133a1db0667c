"""Cut golden vectors from the REFERENCE's --flow-input comparison mode (build container only).

    python tests/golden/make_flow_input_fixtures.py <reference checkout>

Runs the reference's own `VideoFlowProcessor.process_video(..., taa=True, flow_input=<flow video>,
use_flow_cache=<fixture fields>)` on the 6-frame 40 x 56 clip and fields of render.npz, with the stand-in modules of
make_render_fixtures.py (a `cv2` with VideoCapture over arrays, a collecting VideoWriter, RGB<->BGR, no-op text) plus
`cv2.rectangle` as this project defines a filled rectangle (both corners inclusive, clipped to the picture).  Four jobs:
rg8 and rgb8 with a 6-frame flow video, rg8 with a 4-frame one (last frame repeated), rgb8 with an 8-frame one (cut).
The external flows are the fixture fields plus block-wise offsets of 0, 0.05, 0.3, 0.8, 1.5 and 5 px, so that all five
difference classes occur in every job (asserted: each holds at least 1 % of the job's difference-tile pixels outside
the legend).  Stored as data in flow_input.npz: the flow-video frames fed, every written output frame, the `[Flow
Input]` log lines, and the reference's decode_motion_vectors / create_difference_overlay outputs on special inputs
(threshold magnitudes and their float32 neighbours, NaN, +-inf; pictures of 40 x 56, 20 x 300 and 37 x 53).  Nothing of
the reference's source text is stored.  The GPU box never runs this file."""
import contextlib
import io
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_render_fixtures as base  # noqa: E402  (takes the reference checkout from sys.argv[1], puts our tree on the path)
from storage.cache_manager import FlowCacheManager  # noqa: E402
from visualization.video_composer import RADAR_COLORS, fill_rectangle  # noqa: E402

OFFSETS = (0.0, 0.05, 0.3, 0.8, 1.5, 5.0)
CLAMP = 32.0


def external_fields(fields):
    """The fixture fields with one x offset per block of a 2 x 3 block grid."""
    out = fields.copy()
    h, w = fields.shape[1:3]
    ys, xs = np.array_split(np.arange(h), 2), np.array_split(np.arange(w), 3)
    for k, off in enumerate(OFFSETS):
        yy, xx = ys[k // 3], xs[k % 3]
        out[:, yy[0]:yy[-1] + 1, xx[0]:xx[-1] + 1, 0] += np.float32(off)
    return out


def legend_mask(h, w):
    m = np.zeros((h, w, 3), np.uint8)
    for i in range(5):
        fill_rectangle(m, (10 + 45 * i - 1, h - 33), (10 + 45 * i + 13, h - 19), (1, 1, 1))
    return m[:, :, 0].astype(bool)


def overlay_specials(rng):
    """(a, b) flow pairs: magnitudes at the class bounds and one float32 step either side, NaN and +-inf components,
    the rest random over all classes."""
    f32 = np.float32
    out = {}
    for name, (h, w) in {"40x56": (40, 56), "20x300": (20, 300), "37x53": (37, 53)}.items():
        a = (rng.integers(-48, 49, (h, w, 2)) / f32(16)).astype(f32)        # |a - b| over all five classes
        b = np.zeros((h, w, 2), f32)
        if name == "40x56":
            b = (rng.integers(-8, 9, (h, w, 2)) / f32(16)).astype(f32)
        marks = []
        for t in (0.1, 0.5, 1.0, 2.0):
            t = f32(t)
            marks += [np.nextafter(t, f32(0)), t, np.nextafter(t, f32(4))]
        for k, m in enumerate(marks):                                       # along x, along y, and against an offset b
            a[0, k], b[0, k] = (m, 0), (0, 0)
            a[1, k], b[1, k] = (0, -m), (0, 0)
            a[2, k], b[2, k] = (f32(3) + m, 1), (3, 1)
        a[3, :6] = [(np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (np.inf, np.inf), (3e38, 3e38)]
        b[3, :6] = [(0, 0), (0, 0), (0, 0), (0, 0), (np.inf, 0), (-3e38, 0)]
        out[name] = (a, b)
    return out


def main():
    base._install_stand_ins()
    cv2 = sys.modules["cv2"]
    cv2.rectangle = lambda img, p0, p1, color, thickness=-1: fill_rectangle(img, p0, p1, color)
    ours_root = os.path.join(base.ROOT, "video-flow-ml_amd")
    sys.path[:] = [p for p in sys.path if os.path.abspath(p) != ours_root]
    for m in [m for m in sys.modules if m.split(".")[0] in ("encoding", "storage", "effects", "visualization", "config",
                                                             "video")]:
        del sys.modules[m]
    sys.path.insert(0, base.REF)
    import flow_processor as ref   # the reference's CLI module

    gold = np.load(os.path.join(HERE, "render.npz"))
    frames, fields = gold["frames"], gold["fields"]
    n, h, w = frames.shape[:3]
    ext = external_fields(fields)
    work = tempfile.mkdtemp(prefix="vfml_flow_input_fx_")
    clip_path = os.path.join(work, "clip.avi")
    open(clip_path, "wb").close()
    base.CLIPS[clip_path] = frames
    cache = os.path.join(work, "cache")
    os.makedirs(cache)
    for i in range(n):
        FlowCacheManager().save_flow_to_cache(fields[i], cache, i, 'npz')

    proc = ref.VideoFlowProcessor.__new__(ref.VideoFlowProcessor)
    proc.device, proc.fast_mode, proc.tile_mode, proc.sequence_length = 'cpu', False, False, 5
    proc.flow_model, proc.motion_vectors_clamp_range, proc.flow_input = 'videoflow', CLAMP, None
    proc.vf_dataset, proc.vf_architecture, proc.vf_variant, proc.stage = 'sintel', 'mof', 'standard', 'sintel'
    proc.cache_manager = ref.FlowCacheManager()
    proc.video_composer = ref.VideoComposer()

    out = {}
    legend = legend_mask(h, w)
    jobs = {"rg8_6": ("motion-vectors-rg8", 6), "rgb8_6": ("motion-vectors-rgb8", 6), "rg8_4": ("motion-vectors-rg8", 4),
            "rgb8_8": ("motion-vectors-rgb8", 8)}
    for name, (fmt, nf) in jobs.items():
        enc = ref.FlowEncoderFactory.create_encoder(fmt, clamp_range=CLAMP)
        idx = [min(i, n - 1) for i in range(nf)]
        # top half: a ramp, not the clip (nothing reads it, and the clip's noise would not compress a second time)
        top = np.broadcast_to((np.arange(w, dtype=np.uint8) * 4)[None, :, None], (h, w, 3))
        video = np.stack([np.concatenate([top, enc.encode(ext[i].copy(), w, h)], axis=0) for i in idx])
        flow_path = os.path.join(work, name + "_flow.avi")
        open(flow_path, "wb").close()
        base.CLIPS[flow_path] = video
        proc.taa_flow_processor = ref.TAAProcessor(alpha=0.1)
        proc.taa_simple_processor = ref.TAAProcessor(alpha=0.1)
        proc.taa_external_processor = ref.TAAProcessor(alpha=0.1)
        base.WRITTEN.clear()
        log = io.StringIO()
        with contextlib.redirect_stdout(log), contextlib.redirect_stderr(io.StringIO()):
            proc.process_video(clip_path, os.path.join(work, name + ".avi"), max_frames=n, taa=True, flow_format=fmt,
                               use_flow_cache=cache, auto_play=False, skip_lods=True, uncompressed=True,
                               flow_input=flow_path)
        written = np.stack(base.WRITTEN)
        assert written.shape == (n, 3 * h, 2 * w, 3), (name, written.shape)
        lines = log.getvalue().splitlines()
        at = next(k for k, ln in enumerate(lines) if ln.startswith("[Flow Input]"))
        block = []
        for ln in lines[at:]:
            if ln == "":
                break
            if re.match(r"(\[Flow Input\]|  \S|Extracting flow from)", ln):
                block.append(ln)
        diff = written[:, 2 * h:, w:, ::-1][:, ~legend]                    # RGB, outside the legend
        for colour in RADAR_COLORS:
            share = np.all(diff == np.array(colour, np.uint8), axis=-1).mean()
            assert share >= 0.01, (name, colour, share)
        out[f"video_{name}"], out[f"out_{name}"], out[f"log_{name}"] = video, written, np.array(block)

    rng = np.random.default_rng(20261017)
    pic = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    pic[0, :8] = [(0, 0, 0), (255, 255, 255), (127, 128, 0), (128, 127, 255), (0, 255, 128), (255, 0, 1), (1, 1, 1),
                  (254, 254, 254)]
    out["decode_in"] = pic
    from encoding.flow_encoders import decode_motion_vectors      # the reference's (its checkout leads sys.path now)
    assert os.path.abspath(sys.modules["encoding"].__file__).startswith(os.path.abspath(base.REF))
    for variant in ("rg8", "rgb8"):
        for clamp in (32.0, 7.3):
            out[f"decode_{variant}_{clamp}"] = decode_motion_vectors(pic.copy(), clamp_range=clamp,
                                                                         format_variant=variant)
    for name, (a, b) in overlay_specials(rng).items():
        with np.errstate(all="ignore"), contextlib.redirect_stderr(io.StringIO()):
            out[f"overlay_a_{name}"], out[f"overlay_b_{name}"] = a, b
            out[f"overlay_{name}"] = proc.create_difference_overlay(a.copy(), b.copy())
    path = os.path.join(HERE, "flow_input.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
