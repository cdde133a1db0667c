"""Flow quality map and batch flow-cache correction, API mirror of the reference correction_worker.py.

`generate_quality_frame_gpu` (:175-208): same arguments and result (numpy uint8 [H,W,3]: green = match above the
threshold, red = below, full red = the vector leaves the image; fields at a cached LOD's resolution are resized
inside).  The work is one HIP kernel (`vfml_flow_quality_map`) instead of ~25 torch ops; `quality_frame_resident` is
the same for inputs that already live in HBM.

`worker_process` (:221-341): the engine behind the visualiser's "correct errors / correct all frames / correct range"
buttons, same signature, files and console line.  For every bad pixel of a frame (red byte of the quality map > 0) it
re-estimates the vector with a phase correlation of two 50x50 grey regions seeded from the coarsest cached LOD, falls
back to an 11x11 TM_CCOEFF_NORMED template match over the search area plus a spiral search, and writes the better
result when it beats the pixel's current match; the corrected field goes to `<cache>_corrected/<name>`.  Here the
whole frame is one call into HIP (`vfml_flow_correct`: every bad pixel on its own workgroup) instead of a Python loop
with two OpenCV calls per pixel.  `correct_flow_resident` is the same for device tensors, `correct_flow_cache` runs
it over a cache directory, and `python correction_worker.py --input ... --flow-cache DIR` from a shell.

What to know:
  * OpenCV is not a dependency.  cvtColor(RGB2GRAY), phaseCorrelate and matchTemplate(TM_CCOEFF_NORMED) are defined
    in this project from the OpenCV 4.x algorithms (f64 direct DFTs with a fixed summation order, exact integer window
    sums); they are written from the published algorithms and are not pinned against cv2 itself.
  * The flow must be at the frame's resolution (a cache's level 0 always is): with a coarser field the reference's
    in-place loop depends on the pixel order, because several pixels share one cell.  Anything else is a ValueError.
  * Only the visualiser's geometry is built: region radius 25, template radius 5.5, search radius 25.  Other radii are
    a ValueError, never a silent fallback.
  * Divergence: where `frame_idx + 1` is past the last frame the reference raises IndexError in its thread; this
    prints a message and skips the frame.
  * There is no CPU path: a non-cuda device is a RuntimeError."""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

DEFAULT_CONSTANTS = {"GOOD_QUALITY_THRESHOLD": 0.8, "FINE_CORRECTION_THRESHOLD": 0.9, "DETAIL_ANALYSIS_REGION_SIZE": 25,
                     "TEMPLATE_RADIUS": 5.5, "SEARCH_RADIUS": 25}
_BUILT_RADII = {"DETAIL_ANALYSIS_REGION_SIZE": 25.0, "TEMPLATE_RADIUS": 5.5, "SEARCH_RADIUS": 25.0}
_DFT_SIZE = 50


def quality_frame_resident(frame1, frame2, flow, good_quality_threshold):
    """Device tensors in (uint8 [H,W,3] x2, float32 [fh,fw,2]), device uint8 [H,W,3] out."""
    from vfml import hip
    return hip.flow_quality_map(frame1, frame2, flow, good_quality_threshold)


def generate_quality_frame_gpu(frame1, frame2, flow, device, good_quality_threshold):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"generate_quality_frame_gpu: device {device} - the quality map is a HIP kernel, there is no "
                           "CPU path in this build")
    f1 = torch.from_numpy(np.ascontiguousarray(frame1)).to(device)
    f2 = torch.from_numpy(np.ascontiguousarray(frame2)).to(device)
    fl = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).to(device)
    return quality_frame_resident(f1, f2, fl, good_quality_threshold).cpu().numpy()


# ---- batch correction ---------------------------------------------------------------------------------------------
def _constants(constants):
    c = dict(DEFAULT_CONSTANTS)
    if constants:
        c.update(constants)
    bad = {k: c[k] for k, v in _BUILT_RADII.items() if float(c[k]) != v}
    if bad:
        raise ValueError(f"correction radii {bad} are not built: only region 25, template 5.5, search 25 "
                         "(the visualiser's geometry)")
    return c


def _require_cuda(device, what):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{what}: device {device} - the correction search is a HIP kernel, there is no CPU path in "
                           "this build")
    return device


def twiddles(n=_DFT_SIZE):
    """float64 [2, n]: cos and sin of 2 pi m / n, the table the phase correlation's DFTs read."""
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.stack([np.cos(ang), np.sin(ang)])


_TW = {}


def correct_flow_resident(frame1, frame2, flow, lod_flow=None, constants=None, records=False):
    """Device tensors in: uint8 frames [H,W,3], float32 flow [H,W,2] at the frame's resolution, float32 LOD [lh,lw,2]
    (None: the flow itself).  -> (corrected flow [H,W,2] device tensor, initial bad count, final bad count), plus the
    per-bad-pixel detail records (float64 [initial, 16], hip.CORRECT_RECORD layout) when `records`."""
    from vfml import hip
    c = _constants(constants)
    _require_cuda(frame1.device, "correct_flow_resident")
    h, w = frame1.shape[:2]
    if flow.dim() != 3 or tuple(flow.shape) != (h, w, 2):
        raise ValueError(f"correct_flow_resident: flow {tuple(flow.shape)} is not at the frame's resolution {h}x{w} "
                         "(correct the cache's level 0)")
    lod = flow if lod_flow is None else lod_flow
    dev = frame1.device
    if dev not in _TW:
        _TW[dev] = torch.from_numpy(twiddles()).to(dev)
    rec = torch.empty((h * w, hip.CORRECT_RECORD), dtype=torch.float64, device=dev) if records else None
    out, counts = hip.flow_correct(frame1, frame2, flow, lod, _TW[dev], c["GOOD_QUALITY_THRESHOLD"],
                                   c["FINE_CORRECTION_THRESHOLD"], c["DETAIL_ANALYSIS_REGION_SIZE"],
                                   c["TEMPLATE_RADIUS"], c["SEARCH_RADIUS"], records=rec)
    initial, final = (int(v) for v in counts.cpu().tolist())
    if records:
        return out, initial, final, rec[:initial]
    return out, initial, final


def get_highest_available_lod(frame_idx, flow_data, lod_data, max_lod_levels):
    """(level, field) of the coarsest LOD cached for the frame; level 0 is the flow itself."""
    for level in range(max_lod_levels - 1, -1, -1):
        if level == 0 and flow_data is not None:
            return 0, flow_data
        lod = lod_data.get((frame_idx, level))
        if lod is not None:
            return level, lod
    return None, None


def _save_corrected(flow_file, flow):
    from storage.cache_manager import FlowFileHandler
    src = Path(flow_file)
    out_dir = src.parent.with_name(src.parent.name + "_corrected")
    out_dir.mkdir(exist_ok=True)
    dst = out_dir / src.name
    if dst.suffix == ".flo":
        FlowFileHandler.save_flow_flo(flow, str(dst))
    elif dst.suffix == ".npz":
        np.savez_compressed(str(dst), flow=flow)


def worker_process(worker_id, frame_indices, frames, flow_data_cache, lod_data_cache, device_str, max_lod_levels,
                   flow_files, constants):
    """Correct the bad pixels of every frame in `frame_indices` and write `<cache>_corrected/<name>` (reference :221)."""
    device = _require_cuda(device_str, "worker_process")
    c = _constants(constants)
    print(f"Worker {worker_id} (PID: {os.getpid()}) starting, processing {len(frame_indices)} frames: "
          f"{frame_indices[0]} to {frame_indices[-1]}")
    results = []
    for frame_idx in frame_indices:
        start = time.time()
        flow_data = flow_data_cache.get(frame_idx)
        if flow_data is None:
            print(f"Worker skipping frame {frame_idx}: No flow data.")
            results.append({'initial': 0, 'final': 0, 'improved': 0, 'failed': 0, 'skipped': True})
            continue
        if frame_idx + 1 >= len(frames):
            print(f"Worker skipping frame {frame_idx}: no frame {frame_idx + 1} to correct against.")
            results.append({'initial': 0, 'final': 0, 'improved': 0, 'failed': 0, 'skipped': True})
            continue
        frame1, frame2 = frames[frame_idx], frames[frame_idx + 1]
        h, w = frame1.shape[:2]
        flow = np.ascontiguousarray(flow_data, dtype=np.float32)
        if flow.shape != (h, w, 2):
            raise ValueError(f"worker_process: flow of frame {frame_idx} is {flow.shape}, not at the frame's "
                             f"resolution {h}x{w}")
        _, lod = get_highest_available_lod(frame_idx, flow_data, lod_data_cache, max_lod_levels)
        f1 = torch.from_numpy(np.ascontiguousarray(frame1)).to(device)
        f2 = torch.from_numpy(np.ascontiguousarray(frame2)).to(device)
        fl = torch.from_numpy(flow).to(device)
        ld = torch.from_numpy(np.ascontiguousarray(lod, dtype=np.float32)).to(device)
        out, initial, final = correct_flow_resident(f1, f2, fl, ld, c)
        if initial == 0:
            results.append({'initial': 0, 'final': 0, 'improved': 0, 'failed': 0, 'skipped': False})
            continue
        corrected = out.cpu().numpy()
        try:
            _save_corrected(flow_files[frame_idx], corrected)
        except Exception as e:  # the reference reports a failed save and goes on
            print(f"Worker for frame {frame_idx} failed to save: {e}")
        duration = time.time() - start
        rate = (initial - final) / initial * 100
        print(f"  [Worker {worker_id}] Frame {frame_idx:4d} | Errors: {initial:4d} -> {final:4d} | "
              f"Success: {rate:5.1f}% | Time: {duration:.2f}s")
        results.append({'initial': initial, 'final': final, 'improved': 0, 'failed': 0, 'skipped': False})
    print(f"Worker {worker_id} finished.")
    return results


def correct_flow_cache(cache_dir, frames, frame_indices=None, device='cuda', constants=None, max_lod_levels=5):
    """Correct a flow cache directory (frame i of the cache pairs frames[i] with frames[i + 1]): loads the flows and
    LOD files through FlowCacheManager, runs `worker_process`, returns its per-frame results.  The corrected fields
    land in `<cache_dir>_corrected/`."""
    _require_cuda(device, "correct_flow_cache")
    from storage.cache_manager import FlowCacheManager
    mgr = FlowCacheManager()
    cache_dir = os.path.normpath(str(cache_dir))
    if frame_indices is None:
        frame_indices = list(range(max(0, len(frames) - 1)))
    frame_indices = list(frame_indices)
    if not frame_indices:
        raise ValueError("correct_flow_cache: no frames to correct")
    flows, lods, files = {}, {}, []
    for i in range(max(len(frames), max(frame_indices) + 1)):
        npz, flo = mgr._frame_file(cache_dir, i, "npz"), mgr._frame_file(cache_dir, i, "flo")
        files.append(npz if os.path.exists(npz) or not os.path.exists(flo) else flo)
    for i in frame_indices:
        try:
            flows[i] = mgr.load_cached_flow(cache_dir, i)
        except FileNotFoundError:
            continue
        for level in range(1, max_lod_levels):
            try:
                lods[(i, level)] = mgr.load_flow_lod(cache_dir, i, level)
            except FileNotFoundError:
                pass
    return worker_process(0, frame_indices, frames, flows, lods, device, max_lod_levels, files, constants)


def _load_frames(spec):
    if spec.startswith("synthetic:"):
        w, h, n = (int(v) for v in spec[len("synthetic:"):].lower().split("x"))
        from vfml.synth import synthetic_clip
        return synthetic_clip(n, h, w)
    arr = np.load(spec)
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError(f"{spec}: want uint8 frames [F,H,W,3], got {arr.dtype} {arr.shape}")
    return list(arr)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Batch-correct the bad pixels of a flow cache on the GPU; writes "
                                             "<flow-cache>_corrected/.")
    ap.add_argument("--input", required=True, help="frames: a .npy of uint8 [F,H,W,3], or synthetic:WxHxF")
    ap.add_argument("--flow-cache", required=True, help="cache directory (flow_frame_NNNNNN.npz/.flo and LOD files)")
    ap.add_argument("--start-frame", type=int, default=0, help="first cache frame to correct")
    ap.add_argument("--frames", type=int, default=None, help="number of cache frames to correct (default: all)")
    ap.add_argument("--device", default="cuda", help="cuda device (there is no CPU path)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    frames = _load_frames(args.input)
    stop = len(frames) - 1 if args.frames is None else min(len(frames) - 1, args.start_frame + args.frames)
    indices = list(range(args.start_frame, stop))
    results = correct_flow_cache(args.flow_cache, frames, indices, device=args.device)
    done = [r for r in results if not r['skipped']]
    print(f"corrected {len(done)} of {len(results)} frames: {sum(r['initial'] for r in done)} -> "
          f"{sum(r['final'] for r in done)} bad pixels")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
