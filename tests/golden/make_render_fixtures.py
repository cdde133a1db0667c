"""Cut golden vectors from the REFERENCE's video render (build container only).

    python tests/golden/make_render_fixtures.py <reference checkout>

Runs the reference's own `VideoFlowProcessor.process_video(..., use_flow_cache=<fixture fields>)` on a small clip for
three jobs: side by side / gamedev, --flow-only / torchvision, --taa / hsv.  OpenCV and torchvision are not
dependencies of this project, so stand-in modules are installed: `cv2` with this project's HSV2RGB (DESIGN.md section
9; it also records the H, S, V bytes the reference's HSV encoder hands to it), RGB<->BGR, a VideoCapture over an array,
a VideoWriter that collects the frames, no-op text drawing; `torchvision.utils.flow_to_image` with the colour wheel as
this project defines it.  The flow model packages are stubbed (the cache is complete, no model is loaded).  Frames,
fields, every written output frame and the encoders' outputs on special-value flows are stored as data (render.npz);
nothing of the reference's source text is.  The GPU box never runs this file."""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else sys.exit("usage: make_render_fixtures.py <reference checkout>")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))
from encoding import flow_encoders as ours  # noqa: E402
from storage.cache_manager import FlowCacheManager  # noqa: E402

CLIPS = {}          # path -> RGB frames the stand-in VideoCapture serves
WRITTEN = []        # frames handed to the stand-in VideoWriter
HSV_SEEN = []       # (H, S, V) arrays handed to cvtColor(COLOR_HSV2RGB)


def _install_stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB, cv2.COLOR_HSV2RGB = 4, 5, 55
    cv2.CAP_PROP_POS_FRAMES, cv2.CAP_PROP_FPS, cv2.CAP_PROP_FRAME_WIDTH = 1, 5, 3
    cv2.CAP_PROP_FRAME_HEIGHT, cv2.CAP_PROP_FRAME_COUNT = 4, 7
    cv2.FONT_HERSHEY_SIMPLEX, cv2.LINE_AA = 0, 16

    def cvtColor(img, code):
        if code in (cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2RGB):
            return np.ascontiguousarray(img[:, :, ::-1])
        assert code == cv2.COLOR_HSV2RGB and img.dtype == np.uint8
        HSV_SEEN.append(img.copy())
        return ours.hsv2rgb_u8(img)

    class VideoCapture:
        def __init__(self, path):
            self.frames, self.pos = CLIPS[str(path)], 0

        def isOpened(self):
            return True

        def get(self, prop):
            f = self.frames
            return {cv2.CAP_PROP_FPS: 30.0, cv2.CAP_PROP_FRAME_WIDTH: f.shape[2], cv2.CAP_PROP_FRAME_HEIGHT: f.shape[1],
                    cv2.CAP_PROP_FRAME_COUNT: f.shape[0], cv2.CAP_PROP_POS_FRAMES: self.pos}[prop]

        def set(self, prop, v):
            assert prop == cv2.CAP_PROP_POS_FRAMES
            self.pos = int(v)

        def read(self):
            if self.pos >= len(self.frames):
                return False, None
            self.pos += 1
            return True, np.ascontiguousarray(self.frames[self.pos - 1][:, :, ::-1])

        def release(self):
            pass

    class VideoWriter:
        def __init__(self, path, fourcc, fps, size):
            self.size = size

        def isOpened(self):
            return True

        def write(self, frame):
            assert frame.shape == (self.size[1], self.size[0], 3) and frame.dtype == np.uint8
            WRITTEN.append(frame.copy())

        def release(self):
            pass

    cv2.cvtColor, cv2.VideoCapture, cv2.VideoWriter = cvtColor, VideoCapture, VideoWriter
    cv2.VideoWriter_fourcc = lambda *c: sum(ord(x) << (8 * i) for i, x in enumerate(c))
    cv2.putText = lambda *a, **k: None
    cv2.getTextSize = lambda text, font, scale, thick: ((int(len(text) * 20 * scale), int(22 * scale)), 0)
    sys.modules["cv2"] = cv2

    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")

    def flow_to_image(flow):        # [N,2,H,W] float tensor -> [N,3,H,W] uint8 tensor
        import torch
        f = flow[0].permute(1, 2, 0).numpy()
        return torch.from_numpy(ours.flow_to_wheel_u8(f)).permute(2, 0, 1)[None]

    tvu.flow_to_image = flow_to_image
    tv.utils = tvu
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    for name in ("processing", "processing.flow_inference", "processing.memflow_inference"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["processing.flow_inference"].VideoFlowInference = object
    sys.modules["processing.memflow_inference"].MemFlowInference = object


def _clip(rng, n, h, w):
    base = rng.integers(0, 256, size=(h + 16, w + 16, 3)).astype(np.float32)
    k = np.ones(3, np.float32) / 3
    for ax in (0, 1):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, base)
    frames = [np.clip(base[8 - i:8 - i + h, 8 + i:8 + i + w] + rng.normal(0, 3, (h, w, 3)), 0, 255).astype(np.uint8)
              for i in range(n)]
    return np.stack(frames)


def _fields(rng, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for i in range(n):
        f = np.stack([-1.0 + 0.05 * (xx - w / 2) + rng.normal(0, 0.7, (h, w)),
                      1.0 + 0.04 * (yy - h / 2) * (i % 2 * 2 - 1) + rng.normal(0, 0.7, (h, w))], axis=2)
        out.append(f.astype(np.float32) * (1 + i))
    return np.stack(out)


def main():
    _install_stand_ins()
    sys.path[:] = [p for p in sys.path if os.path.abspath(p) != os.path.join(ROOT, "video-flow-ml_amd")]
    for m in [m for m in sys.modules if m.split(".")[0] in ("encoding", "storage", "effects", "visualization", "config",
                                                             "video")]:
        del sys.modules[m]
    sys.path.insert(0, REF)
    import flow_processor as ref   # the reference's CLI module

    rng = np.random.default_rng(20261016)
    n, h, w = 6, 40, 56
    frames = _clip(rng, n, h, w)
    fields = _fields(rng, n, h, w)
    work = tempfile.mkdtemp(prefix="vfml_render_fx_")
    clip_path = os.path.join(work, "clip.avi")
    open(clip_path, "wb").close()
    CLIPS[clip_path] = frames
    cache = os.path.join(work, "cache")
    os.makedirs(cache)
    mgr = FlowCacheManager()
    for i in range(n):
        mgr.save_flow_to_cache(fields[i], cache, i, 'npz')

    proc = ref.VideoFlowProcessor.__new__(ref.VideoFlowProcessor)
    proc.device, proc.fast_mode, proc.tile_mode, proc.sequence_length = 'cpu', False, False, 5
    proc.flow_model, proc.motion_vectors_clamp_range, proc.flow_input = 'videoflow', 32.0, None
    proc.vf_dataset, proc.vf_architecture, proc.vf_variant, proc.stage = 'sintel', 'mof', 'standard', 'sintel'
    proc.taa_flow_processor = ref.TAAProcessor(alpha=0.1)
    proc.taa_simple_processor = ref.TAAProcessor(alpha=0.1)
    proc.taa_external_processor = ref.TAAProcessor(alpha=0.1)
    proc.cache_manager = ref.FlowCacheManager()
    proc.video_composer = ref.VideoComposer()

    out = {"frames": frames, "fields": fields}
    jobs = {"sbs_gamedev": dict(flow_format="gamedev"), "flowonly_torchvision": dict(flow_format="torchvision",
                                                                                      flow_only=True),
            "taa_hsv": dict(flow_format="hsv", taa=True)}
    for name, kw in jobs.items():
        WRITTEN.clear()
        HSV_SEEN.clear()
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            proc.process_video(clip_path, os.path.join(work, name + ".avi"), max_frames=n, use_flow_cache=cache,
                               auto_play=False, skip_lods=True, uncompressed=True, **kw)
        assert len(WRITTEN) == n, (name, len(WRITTEN))
        out[f"out_{name}"] = np.stack(WRITTEN)
        if HSV_SEEN:
            out[f"hsv_{name}"] = np.stack(HSV_SEEN)

    # the encoders alone on the special-value flows of flow_encoders.npz, plus all-zero and all-inf fields
    enc = np.load(os.path.join(HERE, "flow_encoders.npz"))
    specials = {"flow": enc["flow"], "small": enc["small"], "zero": np.zeros((37, 53, 2), np.float32)}
    big = enc["small"].copy()
    big[3, 4] = (3e38, -3e38)                       # |f| overflows float32: the frame maximum is inf
    specials["huge"] = big
    hsv_enc, tv_enc = ref.FlowEncoderFactory.create_encoder('hsv'), ref.FlowEncoderFactory.create_encoder('torchvision')
    for key, f in specials.items():
        HSV_SEEN.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            out[f"enc_in_{key}"] = f
            out[f"enc_hsv_{key}"] = hsv_enc.encode(f.copy(), f.shape[1], f.shape[0])
            out[f"enc_hsvbytes_{key}"] = HSV_SEEN[-1]
            out[f"enc_tv_{key}"] = tv_enc.encode(f.copy(), f.shape[1], f.shape[0])
    np.savez_compressed(os.path.join(HERE, "render.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
