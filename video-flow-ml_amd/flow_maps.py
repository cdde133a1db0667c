"""Flow QA maps of the reference visualiser without Tk, and a headless QA video.

`generate_turbulence_map` mirrors `FlowVisualizer.generate_turbulence_map(flow, kernel_size=25)` (reference
flow_visualizer.py :2997-3052): a JET heat map of the local standard deviation of the flow vectors, normalised between
the frame's 5th and 95th percentile - where a user looks for flicker and torn regions before deciding what to correct.
numpy in, numpy uint8 [H,W,3] out in cv2's channel order (B first); the frame size the method takes from the visualiser
is the `frame_shape` argument here.  `turbulence_map_resident` is the same for a field that already lives in HBM.  The
work is `vfml_flow_turbulence_map` (csrc/turbulence.hip): box moments in LDS, an exact radix selection of the
percentiles on the device, one colour pass; no host synchronisation.

`python flow_maps.py --input FRAMES --flow-cache DIR --output qa.avi` writes the QA pictures of a finished flow cache to
a video, for a box without a display: every cached frame i becomes a 2x2 grid
    original            | flow on the HSV wheel
    quality map (i,i+1) | turbulence map
composed on the device (vfml_flow_colorize, vfml_flow_quality_map, vfml_compose_frame) and written by
storage/avi_writer.py, MJPG or --uncompressed.

What to know:
  * OpenCV is not a dependency.  boxFilter (BORDER_REFLECT), resize (INTER_LINEAR, the quality map's taps) and
    COLORMAP_JET are defined in this project from the OpenCV 4.x algorithms and are not pinned against cv2 itself.
  * `flow is None` or a field with a zero dimension gives a zero picture, as in the reference.
  * kernel_size: odd, 1..63; anything else is a ValueError.
  * Divergence: a cache frame without a successor frame has no quality map; it is skipped with correction_worker's
    message.
  * There is no CPU path: a non-cuda device is a RuntimeError."""
import argparse
import os
import sys

import numpy as np
import torch


def _check_kernel_size(kernel_size):
    k = int(kernel_size)
    if k != kernel_size or k % 2 == 0 or not 1 <= k <= 63:
        raise ValueError(f"kernel_size {kernel_size!r}: an odd number in 1..63 is built")
    return k


def _require_cuda(device, what):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what}: device {device} - the turbulence map is a HIP kernel, there is no CPU path in "
                           "this build")
    return device


def turbulence_map_resident(flow, height, width, kernel_size=25):
    """Device float32 [fh,fw,2] in, device uint8 [height,width,3] out (B first)."""
    from vfml import hip
    return hip.flow_turbulence_map(flow, height, width, _check_kernel_size(kernel_size))


def generate_turbulence_map(flow, frame_shape, device='cuda', kernel_size=25):
    """numpy flow [fh,fw,2] (or None) and the frame's shape (H, W[, 3]) -> numpy uint8 [H,W,3], B first."""
    k = _check_kernel_size(kernel_size)
    h, w = int(frame_shape[0]), int(frame_shape[1])
    device = _require_cuda(device, "generate_turbulence_map")
    if flow is None or flow.shape[0] == 0 or flow.shape[1] == 0:
        return np.zeros((h, w, 3), np.uint8)
    fl = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).to(device)
    return turbulence_map_resident(fl, h, w, k).cpu().numpy()


# ---- headless QA video --------------------------------------------------------------------------------------------
def qa_tiles_resident(frame1, frame2, flow, kernel_size=25, threshold=0.8):
    """The four tiles of one QA frame, device uint8 [H,W,3] RGB each: original, flow on the HSV wheel, quality map,
    turbulence map (its channels reversed to RGB)."""
    from vfml import hip
    h, w = frame1.shape[:2]
    wheel = hip.flow_colorize(flow, hip.COLORIZE_HSV)
    if tuple(wheel.shape[:2]) != (h, w):
        raise ValueError(f"flow {tuple(flow.shape)} is not at the frame's resolution {h}x{w}")
    quality = hip.flow_quality_map(frame1, frame2, flow, threshold)
    turbulence = turbulence_map_resident(flow, h, w, kernel_size).flip(-1)
    return [frame1, wheel, quality, turbulence]


QA_LABELS = ((0, "Original"), (2, "Quality map"), (3, "Turbulence map"))      # (tile of the 2x2 grid, its label)


def qa_label_ops(h, w):
    """The draw list of the QA grid's labels for tiles of h x w: each at its tile's top-left corner, clipped to it."""
    from visualization import text as vtext
    ops = []
    for tile, label in QA_LABELS:
        ops += vtext.overlay_ops(label, 'top-left', h, w, ((tile % 2) * w, (tile // 2) * h))
    return ops


def render_qa_video(frames, cache_dir, output, frame_indices, device='cuda', kernel_size=25, threshold=0.8,
                    uncompressed=False, fps=30.0, log=print, sampling="4:2:0", labels=False):
    """Write the QA grid of every cache frame in `frame_indices` to `output`; -> the number of frames written.
    sampling: '4:2:0', '4:2:2' or '4:4:4', the chroma sampling of the MJPG frames.  labels: draw "Original",
    "Quality map" and "Turbulence map" on their tiles (vfml_text_draw behind the composer)."""
    from storage.avi_writer import AviWriter, dib_stride
    from storage.cache_manager import FlowCacheManager
    from vfml import hip
    device = _require_cuda(device, "render_qa_video")
    k = _check_kernel_size(kernel_size)
    mgr = FlowCacheManager()
    cache_dir = os.path.normpath(str(cache_dir))
    h, w = frames[0].shape[:2]
    writer = AviWriter(output, 0 if uncompressed else 'MJPG', fps, (2 * w, 2 * h), log=log, encoder='external',
                       sampling=sampling)
    stride = dib_stride(2 * w) if uncompressed else None
    jpeg = None
    if not uncompressed:           # MJPG frames are encoded on the device (vfml_jpeg_encode_rgb); only the scan comes back
        from storage.device_mjpg import DeviceMjpgEncoder
        jpeg = DeviceMjpgEncoder(writer, 2 * h, 2 * w, device, sampling=sampling)
    text_plan = None
    if labels:
        from visualization.text import build_plan
        text_plan = hip.TextPlan(build_plan(qa_label_ops(h, w), 2 * h, 2 * w), device)
    written = 0
    try:
        for i in frame_indices:
            try:
                flow = mgr.load_cached_flow(cache_dir, i)
            except FileNotFoundError:
                log(f"Worker skipping frame {i}: No flow data.")
                continue
            if i + 1 >= len(frames):
                log(f"Worker skipping frame {i}: no frame {i + 1} to correct against.")
                continue
            f1 = torch.from_numpy(np.ascontiguousarray(frames[i])).to(device)
            f2 = torch.from_numpy(np.ascontiguousarray(frames[i + 1])).to(device)
            fl = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).to(device)
            out = hip.compose_frame(qa_tiles_resident(f1, f2, fl, k, threshold), hip.COMPOSE_GRID_2X2, bgr=uncompressed,
                                    bottom_up=uncompressed, row_stride=stride)
            if text_plan is not None:
                hip.text_draw(text_plan, out, 2 * h, 2 * w, row_stride=stride, bottom_up=uncompressed)
            if jpeg is not None:
                jpeg.submit(out.view(2 * h, 2 * w, 3))
            else:
                writer.write_payload(out.cpu().numpy())
            written += 1
        if jpeg is not None:
            jpeg.finish()
    finally:
        writer.release()
    return written


def _load_frames(spec):
    if spec.startswith("synthetic:"):
        w, h, n = (int(v) for v in spec[len("synthetic:"):].lower().split("x"))
        from vfml.synth import synthetic_clip
        return synthetic_clip(n, h, w)
    arr = np.load(spec)
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError(f"{spec}: want uint8 frames [F,H,W,3], got {arr.dtype} {arr.shape}")
    return list(arr)


def build_parser():
    ap = argparse.ArgumentParser(description="Write the flow QA pictures of a flow cache (original | flow / quality map "
                                             "| turbulence map) to an AVI, on the GPU.")
    ap.add_argument("--input", required=True, help="frames: a .npy of uint8 [F,H,W,3], or synthetic:WxHxF")
    ap.add_argument("--flow-cache", required=True, help="cache directory (flow_frame_NNNNNN.npz/.flo)")
    ap.add_argument("--output", required=True, help="the .avi to write")
    ap.add_argument("--start-frame", type=int, default=0, help="first cache frame")
    ap.add_argument("--frames", type=int, default=None, help="number of cache frames (default: all)")
    ap.add_argument("--kernel-size", type=int, default=25, help="side of the turbulence window, odd, 1..63")
    ap.add_argument("--threshold", type=float, default=0.8, help="good-quality threshold of the quality map")
    ap.add_argument("--uncompressed", action="store_true", help="24-bit DIB frames instead of MJPG")
    ap.add_argument("--device", default="cuda", help="cuda device (there is no CPU path)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    _check_kernel_size(args.kernel_size)
    _require_cuda(args.device, "flow_maps")
    from visualization.video_composer import labels_switch
    labels = labels_switch()                # VFML_LABELS=1: the tiles are labelled; any value but 1 / 0 is refused
    frames = _load_frames(args.input)
    stop = len(frames) if args.frames is None else min(len(frames), args.start_frame + args.frames)
    written = render_qa_video(frames, args.flow_cache, args.output, list(range(args.start_frame, stop)),
                              device=args.device, kernel_size=args.kernel_size, threshold=args.threshold,
                              uncompressed=args.uncompressed, labels=labels)
    print(f"wrote {written} QA frames to {args.output}")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
