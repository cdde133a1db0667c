"""Cut golden vectors from the REFERENCE's batch flow-cache correction (build container only).

    python tests/golden/make_correction_fixtures.py <reference checkout>

Runs the reference's own `worker_process` (correction_worker.py) on small scenes.  OpenCV is not a dependency of this
project, so a stand-in `cv2` module is installed whose cvtColor / phaseCorrelate / matchTemplate / minMaxLoc are this
project's definitions of those primitives (tests/correction_oracle.py; `normalize` and `circle` only feed the GUI's
response image).  The VideoFlow `.flo` writer is stubbed with the repository's own, and `generate_quality_frame_gpu`
runs on torch's CPU device.  `perform_coarse_correction` / `perform_fine_correction` / `calculate_pixel_quality` are
wrapped so that every bad pixel's intermediates are recorded.  Inputs, the corrected files, the printed counts and the
intermediates are stored as data (correction.npz); nothing of the reference's source text is.  The GPU box never runs
this file."""
import contextlib
import io
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else sys.exit("usage: make_correction_fixtures.py <reference checkout>")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "video-flow-ml_amd"))
import correction_oracle as co  # noqa: E402
from storage.cache_manager import FlowFileHandler, LODGenerator  # noqa: E402


def _install_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2GRAY, cv2.COLOR_GRAY2BGR, cv2.TM_CCOEFF_NORMED, cv2.NORM_MINMAX, cv2.CV_8U = 7, 8, 5, 32, 0

    def cvtColor(img, code):
        if code == cv2.COLOR_RGB2GRAY:
            assert img.dtype == np.uint8 and img.ndim == 3
            return co.grey(img)
        return np.repeat(img[..., None], 3, axis=2)

    def phaseCorrelate(a, b):
        assert a.shape == b.shape and a.dtype == np.float32
        return co.phase_correlate(a, b), 0.0

    def matchTemplate(search, templ, method):
        assert method == cv2.TM_CCOEFF_NORMED and search.dtype == np.uint8 and templ.dtype == np.uint8
        return co.match_template(search, templ)

    def minMaxLoc(res):
        lo, hi = int(np.argmin(res)), int(np.argmax(res))
        w = res.shape[1]
        return float(res.flat[lo]), float(res.flat[hi]), (lo % w, lo // w), (hi % w, hi // w)

    cv2.cvtColor, cv2.phaseCorrelate, cv2.matchTemplate, cv2.minMaxLoc = cvtColor, phaseCorrelate, matchTemplate, minMaxLoc
    cv2.normalize = lambda res, *a, **k: np.zeros(res.shape, np.uint8)
    cv2.circle = lambda *a, **k: None
    sys.modules["cv2"] = cv2
    for name in ("VideoFlow", "VideoFlow.core", "VideoFlow.core.utils", "VideoFlow.core.utils.frame_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["VideoFlow.core.utils.frame_utils"].writeFlow = lambda path, flow: FlowFileHandler.save_flow_flo(flow, path)


def _texture(rng, h, w, pad=40):
    base = rng.integers(0, 256, size=(h + 2 * pad, w + 2 * pad, 3)).astype(np.float32)
    k = np.ones(5, np.float32) / 5
    for ax in (0, 1):
        base = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, base)
    base = (base - base.mean()) * 3.0 + 128.0
    return base


def _crop(base, pad, dy, dx, h, w, rng, noise=2.0):
    out = base[pad + dy:pad + dy + h, pad + dx:pad + dx + w] + rng.normal(0, noise, (h, w, 3))
    return np.clip(out, 0, 255).astype(np.uint8)


def scene_a(rng):
    """96x128, .npz cache.  Frame 0: true motion (-3, +2) with correct, slightly wrong and grossly wrong vectors,
    bad pixels on all four borders, engine LODs.  Frame 1: identical frames, zero flow (no bad pixel, no file).
    Frame 2: no LOD files (level-0 fallback), vectors sending the coarse target far outside the frame.  Frame 3: no
    flow (skipped)."""
    h, w, pad = 96, 128, 40
    base = _texture(rng, h, w, pad)
    f0 = _crop(base, pad, 0, 0, h, w, rng)
    f1 = _crop(base, pad, -2, 3, h, w, rng)       # content moves by (-3, +2): frame2[y, x] ~ frame1[y + 2, x - 3]
    f2 = f1.copy()
    f3 = _crop(base, pad, 1, -2, h, w, rng)       # from f2: moves by (-5, +3)
    flow0 = np.tile(np.array([3.0, -2.0], np.float32), (h, w, 1)) + rng.normal(0, 0.15, (h, w, 2)).astype(np.float32)
    flow0[20:34, 30:50] += np.float32(0.9)                                    # slightly wrong
    flow0[50:62, 60:80] += np.array([14.0, -9.0], np.float32)               # grossly wrong
    flow0[0:3, 40:60] = [0.0, 30.0]                                           # top border
    flow0[h - 3:h, 70:90] = [5.0, -30.0]                                      # bottom border
    flow0[40:55, 0:3] = [-20.0, 0.0]                                          # left border
    flow0[60:70, w - 3:w] = [25.0, 4.0]                                       # right border
    flow1 = np.zeros((h, w, 2), np.float32)
    flow3 = np.tile(np.array([-5.0, 3.0], np.float32), (h, w, 1)) + rng.normal(0, 0.2, (h, w, 2)).astype(np.float32)
    flow3[10:16, 10:30] = [70.0, 0.5]           # target x = x - 70: 40..60 px left of the frame
    flow3[30:36, 90:110] = [-2.0, 75.0]          # target y far above
    flow3[60:66, 20:40] = [-140.0, -1.0]         # target x far right
    flow3[80:86, 50:70] = [3.0, -90.0]           # target y far below
    flow3[44:48, 100:124] = [135.0, 0.0]         # negative slice stop: search area as wide as the frame
    frames = [f0, f1, f2, f3]
    flows = {0: flow0, 1: flow1, 2: flow3}
    lods = {(0, k): l for k, l in enumerate(LODGenerator.generate_lods(flow0, 5)) if k > 0}
    lods.update({(1, k): l for k, l in enumerate(LODGenerator.generate_lods(flow1, 5)) if k > 0})
    return frames, flows, lods, [0, 1, 2, 3], "npz"


def scene_b(rng):
    """64x80, .flo cache.  Frame 0: a constant-colour patch in both frames (template and windows with zero
    variance), engine LODs.  Frame 1: identical frames with a perturbed flow."""
    h, w, pad = 64, 80, 40
    base = _texture(rng, h, w, pad)
    f0 = _crop(base, pad, 0, 0, h, w, rng)
    f1 = _crop(base, pad, 1, 2, h, w, rng)          # content moves by (-2, -1)
    f0[20:44, 24:52] = [90, 140, 60]
    f1[19:43, 22:50] = [90, 140, 60]
    f2 = f1.copy()
    flow0 = np.tile(np.array([2.0, 1.0], np.float32), (h, w, 1)) + rng.normal(0, 0.2, (h, w, 2)).astype(np.float32)
    flow0[26:38, 30:46] += np.array([6.0, -5.0], np.float32)
    flow0[5:12, 5:20] += np.array([-4.0, 3.0], np.float32)
    flow1 = np.zeros((h, w, 2), np.float32)
    flow1[10:40, 10:50] = rng.normal(0, 2.5, (30, 40, 2)).astype(np.float32)
    frames = [f0, f1, f2]
    flows = {0: flow0, 1: flow1}
    lods = {(0, k): l for k, l in enumerate(LODGenerator.generate_lods(flow0, 5)) if k > 0}
    lods.update({(1, k): l for k, l in enumerate(LODGenerator.generate_lods(flow1, 5)) if k > 0})
    return frames, flows, lods, [0, 1], "flo"


def run_scene(ref, tag, frames, flows, lods, indices, ext, out):
    rec = {"pixels": [], "calls": []}

    def q(*a):
        v = ref_q(*a)
        rec["calls"].append(float(v))
        return v

    def coarse(frame1, frame2, source_pixel, lod_vec, r):
        orig = rec["calls"][-1] if rec["calls"] else 0.0
        rec["calls"].clear()
        res = ref_coarse(frame1, frame2, source_pixel, lod_vec, r)
        x, y = int(source_pixel[0]), int(source_pixel[1])
        row = np.zeros(16, np.float64)
        row[:9] = [y * frame1.shape[1] + x, orig, lod_vec[0], lod_vec[1], res["phase_shift"][0], res["phase_shift"][1],
                   res["flow"][0], res["flow"][1], res["similarity"]]
        rec["pixels"].append(row)
        rec["calls"].clear()
        return res

    def fine(*a):
        res = ref_fine(*a)
        row = rec["pixels"][-1]
        row[9] = 1
        if res is not None:
            row[10:14] = [1, res["flow"][0], res["flow"][1], res["similarity"]]
        rec["calls"].clear()
        return res

    ref_q, ref_coarse, ref_fine = ref.calculate_pixel_quality, ref.perform_coarse_correction, ref.perform_fine_correction
    ref_qmap = ref.generate_quality_frame_gpu
    ref.calculate_pixel_quality, ref.perform_coarse_correction, ref.perform_fine_correction = q, coarse, fine
    ref.generate_quality_frame_gpu = lambda f1, f2, fl, dev, thr: ref_qmap(f1, f2, fl, torch.device("cpu"), thr)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            cache = os.path.join(tmp, "cache")
            os.makedirs(cache)
            files = [os.path.join(cache, f"flow_frame_{i:06d}.{ext}") for i in range(len(frames))]
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                results = ref.worker_process(0, indices, frames, dict(flows), dict(lods), "cuda:0", 5, files,
                                             dict(co.DEFAULT_CONSTANTS))
            log = buf.getvalue()
            written = sorted(os.listdir(os.path.join(tmp, "cache_corrected")))
            for name in written:
                path = os.path.join(tmp, "cache_corrected", name)
                fl = np.load(path)["flow"] if ext == "npz" else FlowFileHandler.load_flow_flo(path)
                if ext == "npz":
                    assert list(np.load(path).keys()) == ["flow"]
                idx = int(re.search(r"(\d+)\.", name).group(1))
                out[f"{tag}_corrected_{idx}"] = fl
                out[f"{tag}_corrected_bytes_{idx}"] = np.frombuffer(open(path, "rb").read(), np.uint8) if ext == "flo" \
                    else np.zeros(0, np.uint8)
    finally:
        ref.calculate_pixel_quality, ref.perform_coarse_correction, ref.perform_fine_correction = ref_q, ref_coarse, ref_fine
        ref.generate_quality_frame_gpu = ref_qmap
    counts = [[int(m.group(1)), int(m.group(2)), int(m.group(3))] for m in
              re.finditer(r"Frame\s+(\d+) \| Errors:\s+(\d+) ->\s+(\d+)", log)]
    print(log)
    out[f"{tag}_frames"] = np.stack(frames)
    for i, fl in flows.items():
        out[f"{tag}_flow_{i}"] = fl
    for (i, k), l in lods.items():
        out[f"{tag}_lod_{i}_{k}"] = l
    out[f"{tag}_indices"] = np.array(indices, np.int64)
    out[f"{tag}_ext"] = np.array(ext)
    out[f"{tag}_written"] = np.array(written)
    out[f"{tag}_counts"] = np.array(counts, np.int64).reshape(-1, 3)
    out[f"{tag}_skipped"] = np.array([bool(r["skipped"]) for r in results])
    out[f"{tag}_records"] = np.array(rec["pixels"], np.float64).reshape(-1, 16)
    return len(rec["pixels"])


def main():
    _install_cv2()
    sys.path.insert(0, REF)
    import correction_worker as ref
    rng = np.random.default_rng(20261016)
    out = {}
    for tag, make in (("a", scene_a), ("b", scene_b)):
        n = run_scene(ref, tag, *make(rng), out)
        print(f"scene {tag}: {n} bad pixels corrected, counts {out[tag + '_counts'].tolist()}")
    np.savez_compressed(os.path.join(HERE, "correction.npz"), **out)
    print("wrote correction.npz:", len(out), "arrays;", os.path.getsize(os.path.join(HERE, "correction.npz")), "bytes")


if __name__ == "__main__":
    main()
