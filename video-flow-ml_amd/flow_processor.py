#!/usr/bin/env python3
"""flow_processor.py — command line of the drop-in, flow-field part.

Same flags as the reference CLI (flow_processor.py:1272-1332) and the same flow-cache contract
(cache directory name, flow_frame_%06d.npz members, completeness check, optional LODs), with the
frame loop of its cache-filling paths (:959-976 normal mode, :1460-1470 --interactive) running on
the MI355X engine and, under `python -m torch.distributed.run --nproc-per-node N flow_processor.py …`,
sharded over N GPUs (vfml.runner): whole-frame jobs with no collective at all - every rank writes the
cache files of its own fields - tiled jobs with the tiles streaming to rank 0 in chunked RCCL gathers.

Without --interactive (the reference's normal mode) the complete cache is then rendered into the output video
(`render_video`, reference process_video :635-1173): original | flow side by side, stacked (--flow-only) or a 2x2 grid
with the two TAA results (--taa), MJPG or --uncompressed AVI, on the device by vfml_flow_encode / vfml_flow_colorize /
vfml_taa_blend / vfml_compose_frame, or with the host paths under --device cpu.  With `--taa --flow-input VIDEO` (the
reference's comparison mode, :436-578, :724-765, :1009-1127) a second video carries external motion vectors in its
bottom half - the layout `--flow-only --flow-format motion-vectors-rg8|rgb8` writes - and the output is a 2x3 grid:
original | external flow picture over TAA | TAA simple over TAA with the external flow | flow difference
(vfml_flow_decode, vfml_flow_diff_overlay, the GRID_2X3 layout of vfml_compose_frame).  The reference's text labels
("Original", "TAA + Inv.Flow", the legend's numbers, ...) are drawn with the project's own text (vfml_text_draw on the
device path, visualization/text.py on the host) when DRAW_LABELS / VFML_LABELS=1 says so; off by default.  Out of scope
(DESIGN.md): the Tk/Qt tools; flags that only concern those are accepted and reported as skipped.
With --fast the frames are first reduced by the reference's rule (video/frame_extractor.py: fit 256x256, at most a
quarter / a half of the source, even sides, at least 64) and the whole job runs at that size: on a GPU the frames go up at
source size and vfml_resize_u8 reduces them behind the upload (vfml.runner.ClipFeeder), --device cpu resizes on the host.
Inputs: a `.npy` file holding uint8 frames [F,H,W,3]; `synthetic:WxHxF` (vfml.synth); an `.avi` file of the kinds
storage/avi_writer.py writes (storage/avi_reader.py); or any video file when OpenCV is importable.
"""
import argparse
import os
import sys
import time

script_dir = os.path.dirname(os.path.abspath(__file__))
if script_dir not in sys.path:
    sys.path.insert(0, script_dir)

import numpy as np
import torch

from config import DeviceManager
from processing.flow_inference import VideoFlowInference
from processing.memflow_inference import MemFlowInference
from storage import AsyncFlowCacheWriter, FlowCacheManager
from vfml import dist as vdist
from vfml.runner import ClipFeeder, check_memory_job, check_scene_job, run_sharded
from video.frame_extractor import fast_mode_dimensions, resize_frame
from video.video_info import (SYNTHETIC_FPS, own_avi_reader, probe_video, read_frames, time_to_frame,
                              validate_frame_range)


def build_parser():
    p = argparse.ArgumentParser(description='VideoFlow Optical Flow Processor (MI355X engine)')
    p.add_argument('--input', default='big_buck_bunny_720p_h264.mov', help='Input video (.npy frames, synthetic:WxHxF, or a video file)')
    p.add_argument('--output', default='results', help='Output directory')
    p.add_argument('--device', default='auto', choices=['auto', 'cuda', 'cpu'])
    p.add_argument('--frames', type=int, default=1000, help='Maximum number of frames to process')
    p.add_argument('--start-frame', type=int, default=0)
    p.add_argument('--start-time', type=float, default=None)
    p.add_argument('--duration', type=float, default=None)
    p.add_argument('--fast', action='store_true', help='Fast mode (reduced resolution; depth 6, 3 levels, radius 3)')
    p.add_argument('--flow-only', action='store_true')
    p.add_argument('--taa', action='store_true')
    p.add_argument('--flow-input', type=str, default=None)
    p.add_argument('--flow-format', choices=['gamedev', 'hsv', 'torchvision', 'motion-vectors-rg8', 'motion-vectors-rgb8'],
                   default='gamedev')
    p.add_argument('--motion-vectors-clamp-range', type=float, default=32.0)
    p.add_argument('--tile', action='store_true', help='1280x1280 tile mode')
    p.add_argument('--sequence-length', type=int, default=5)
    p.add_argument('--save-flow', choices=['flo', 'npz', 'both'], default=None)
    p.add_argument('--force-recompute', action='store_true')
    p.add_argument('--use-flow-cache', type=str, default=None)
    p.add_argument('--interactive', action='store_true')
    p.add_argument('--show-tiles', action='store_true')
    p.add_argument('--no-autoplay', action='store_true')
    p.add_argument('--skip-lods', action='store_true')
    p.add_argument('--uncompressed', action='store_true')
    p.add_argument('--model', choices=['videoflow', 'memflow'], default='videoflow')
    p.add_argument('--model-path', type=str, default=None)
    p.add_argument('--stage', choices=['sintel', 'things', 'kitti'], default='sintel')
    p.add_argument('--vf-dataset', choices=['sintel', 'things', 'kitti'], default='sintel')
    p.add_argument('--vf-architecture', choices=['mof', 'bof'], default='mof')
    p.add_argument('--vf-variant', choices=['standard', 'noise'], default='standard')
    return p


def probe_input(spec):
    """-> (fps, total_frames) of an input without decoding it."""
    info = probe_video(spec)
    return info["fps"], info["total_frames"]


def resolve_frame_range(spec, start_frame, max_frames, start_time=None, duration=None, log=print):
    """--start-time / --duration -> (start_frame, max_frames) exactly as the reference converts them
    (flow_processor.py:667-677, :1403-1420; video/frame_extractor.py:88-98): `int(seconds * fps)` replaces the frame
    arguments, then the range is clamped to the clip.  The resolved pair is what the cache directory is named after
    (storage/filename_generator.py: `_start{s}_frames{n}`)."""
    fps, total = probe_input(spec)
    if start_time is not None or duration is not None:
        log(f"Video FPS: {fps:.2f}")
        if start_time is not None:
            start_frame = time_to_frame(start_time, fps)
            log(f"Start time: {start_time}s -> frame {start_frame}")
        if duration is not None:
            max_frames = time_to_frame(duration, fps)
            log(f"Duration: {duration}s -> {max_frames} frames")
    return validate_frame_range(start_frame, max_frames, total)


def load_frames(spec, start_frame, max_frames, fps_default=SYNTHETIC_FPS):
    """-> (frames list of uint8 [H,W,3], fps, width, height, start_frame): the 5-tuple shape of the
    reference's FrameExtractor.extract_frames (video/frame_extractor.py:139), at the source's size."""
    frames, fps = read_frames(spec, start_frame, max_frames, fps_default)
    if not frames:
        raise SystemExit(f"No frames read from {spec}")
    h, w = frames[0].shape[:2]
    return frames, fps, w, h, start_frame


def fast_mode_size(width, height, log=print):
    """--fast's resolution rule on the source size (reference video/frame_extractor.py:26-62, :103-104, :129-130) ->
    (width, height) the job runs at, with the reference's line.  Frames are resized only when the rule's factor is not
    1.0; a source it leaves alone keeps its own size here (the reference reports the rule's sides even then, which for a
    source under 64 pixels are not the frames')."""
    w, h, scale = fast_mode_dimensions(width, height)
    log(f"Fast mode: aggressive resolution reduction from {width}x{height} to {w}x{h} (scale: {scale:.2f})")
    return (w, h) if scale != 1.0 else (width, height)


ENCODER_LINES = {
    'hsv': "[Encoder] Using HSV color space encoder",
    'torchvision': "[Encoder] Using TorchVision color wheel encoder",
    'motion-vectors-rg8': "[Encoder] Using Motion Vectors RG8 encoder (clamp_range={c})",
    'motion-vectors-rgb8': "[Encoder] Using Motion Vectors RGB8 encoder (direction+magnitude format, clamp_range={c})",
    'gamedev': "[Encoder] Using GameDev RG channel encoder",
}


def render_encoder(flow_format, clamp_range):
    """The render stage's own table of the five --flow-format names (FlowEncoderFactory keeps its three)."""
    from encoding.flow_encoders import (GamedevFlowEncoder, HSVFlowEncoder, MotionVectorsRG8FlowEncoder,
                                        MotionVectorsRGB8FlowEncoder, TorchvisionFlowEncoder)
    if flow_format == 'hsv':
        return HSVFlowEncoder()
    if flow_format == 'torchvision':
        return TorchvisionFlowEncoder()
    if flow_format == 'motion-vectors-rg8':
        return MotionVectorsRG8FlowEncoder(clamp_range=clamp_range)
    if flow_format == 'motion-vectors-rgb8':
        return MotionVectorsRGB8FlowEncoder(clamp_range=clamp_range)
    return GamedevFlowEncoder()


def render_output_path(args, fps, log=print):
    """The reference's rule (:686-693): a directory gets a generated file name, anything else is the path itself."""
    output_path = args.output
    if os.path.isdir(output_path):
        from storage.filename_generator import generate_output_filepath
        output_path = generate_output_filepath(
            input_path=args.input, output_dir=args.output, start_time=args.start_time, duration=args.duration,
            start_frame=args.start_frame, max_frames=args.frames, flow_only=args.flow_only, taa=args.taa,
            fast_mode=args.fast, tile_mode=args.tile, uncompressed=args.uncompressed, flow_format=args.flow_format,
            motion_vectors_clamp_range=args.motion_vectors_clamp_range, fps=fps)
        log(f"Auto-generated output filename: {os.path.basename(output_path)}")
    return output_path


FLOW_INPUT_VARIANTS = {'motion-vectors-rg8': 'rg8', 'motion-vectors-rgb8': 'rgb8'}


def check_flow_input(args):
    """--flow-input's argument checks, before anything is computed or rendered (reference :648-650, :483-484)."""
    if not os.path.exists(args.flow_input):
        raise ValueError(f"Flow input video not found: {args.flow_input}")
    if args.flow_format not in FLOW_INPUT_VARIANTS:
        raise ValueError(f"Unsupported flow format: {args.flow_format}")


class FlowInputVideo:
    """The --flow-input video: frames in order from frame 0, one at a time (`.npy` stack, an AVI through
    storage/avi_reader.py, anything else through OpenCV).  `total`, `width`, `height` come from the headers."""

    def __init__(self, spec):
        self.spec, self._arr, self._avi, self._cap, self._pos = spec, None, None, None, 0
        if spec.endswith('.npy'):
            arr = np.load(spec, mmap_mode='r')
            if arr.ndim != 4 or arr.shape[3] != 3 or arr.dtype != np.uint8:
                raise ValueError(f"{spec}: expected uint8 [F,H,W,3], got {arr.dtype} {arr.shape}")
            self._arr, self.total, self.height, self.width = arr, *(int(v) for v in arr.shape[:3])
        elif own_avi_reader(spec):
            from storage.avi_reader import AviReader
            self._avi = AviReader(spec)
            self.total, self.height, self.width = self._avi.frame_count, self._avi.height, self._avi.width
        else:
            try:
                import cv2
            except ImportError:
                raise SystemExit(f"Cannot decode {spec}: OpenCV is not installed. Use a .npy frame stack or an .avi "
                                 f"file (uncompressed or MJPG).")
            self._cv2, self._cap = cv2, cv2.VideoCapture(spec)
            self.total = int(self._cap.get(cv2.CAP_PROP_FRAME_COUNT))
            self.height = int(self._cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
            self.width = int(self._cap.get(cv2.CAP_PROP_FRAME_WIDTH))

    def read(self):
        """-> the next RGB frame [H,W,3] uint8, or None after the last."""
        if self._arr is not None:
            frame = np.ascontiguousarray(self._arr[self._pos]) if self._pos < self.total else None
        elif self._avi is not None:
            frame = self._avi.read()
        else:
            ok, bgr = self._cap.read()
            frame = self._cv2.cvtColor(bgr, self._cv2.COLOR_BGR2RGB) if ok else None
        self._pos += frame is not None
        return frame

    @property
    def mjpg_chunks(self):
        """True when the frames can be handed out undecoded, as JPEG files (an MJPG .avi read by storage/avi_reader.py)."""
        return self._avi is not None and self._avi._mjpg

    def read_chunk(self):
        """-> the next frame's JPEG file (b'': repeat the frame before it) or None after the last."""
        data = self._avi.read_chunk()
        self._pos += data is not None
        return data

    def decode_chunk(self, data):
        return self._avi._decode(data)

    def close(self):
        if self._avi is not None:
            self._avi.close()
        if self._cap is not None:
            self._cap.release()


class _ExternalFlowSource:
    """The encoded pictures of --flow-input, one per main frame (reference :724-765 and extract_flow_from_video
    :436-488): taken from frame 0 of the flow video whatever the main clip's start frame is, rows H//2... of each frame;
    a shorter flow video repeats its last picture.  The reference decodes the whole list up front; here the next
    pictures are read ahead on one thread and decoded when their frame is rendered.
    device: the job's GPU.  The frames of an MJPG .avi then stay JPEG files: the thread reads a chunk's bytes and parses
    its header, and the render loop decodes rows H//2... on the device (a frame without restart
    intervals, as OpenCV writes them, by the self-synchronising kernel of section 13.1).  A frame the device decoder
    does not take is decoded on the host as before."""

    def __init__(self, spec, n, width, height, log, device=None):
        from concurrent.futures import ThreadPoolExecutor
        log("[Flow Input] Extracting flow from external video...")
        self.video = FlowInputVideo(spec)
        try:
            self.take = min(n, self.video.total)
            log(f"  Flow input has {self.video.total} frames")
            log(f"  Main video has {n} frames")
            log(f"  Will extract {self.take} flow frames starting from frame 0")
            self.top = self.video.height // 2
            got = (self.video.height - self.top, self.video.width)
            if got != (height, width):
                raise ValueError(f"Flow input video is {self.video.width}x{self.video.height}: its encoded bottom half "
                                 f"is {got[1]}x{got[0]}, the main video is {width}x{height}")
            log(f"Extracting flow from {self.take} frames...")
            if self.take == 0:
                raise ValueError("No flow data could be extracted from flow input video")
            if self.take < n:
                log(f"  Warning: Flow input shorter than main video. Extended from {self.take} to {n} frames using last "
                    f"frame.")
            log(f"  Successfully prepared {n} flow frames")
            log("")
        except Exception:
            self.video.close()
            raise
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="flow-input")
        self.futs, self.next = {}, 0
        self.files = device is not None and str(device).startswith('cuda') and self.video.mjpg_chunks
        self.rows = (self.top, self.video.height)
        self._seen = False

    def _read(self):
        """-> the picture [h,w,3] uint8; or (file bytes, JpegInfo): a JPEG the device decodes; or None: no new picture."""
        if self.files:
            from storage.jpeg_parse import DEVICE_SAMPLINGS, JpegUnsupported, parse
            data = self.video.read_chunk()
            if data is None or (not data and self._seen):
                return None
            self._seen = True
            try:
                info = parse(data, DEVICE_SAMPLINGS)
                if (info.h, info.w) == (self.video.height, self.video.width):
                    return data, info
            except JpegUnsupported:
                pass
            return self.video.decode_chunk(data)[self.top:]
        frame = self.video.read()
        return None if frame is None else frame[self.top:]

    def get(self, i, ahead=2):
        """-> the encoded picture [h,w,3] uint8 of main frame i (i ascending) - or its JPEG file and header, see _read -
        or None: repeat the one before."""
        while self.next < min(self.take, i + ahead + 1):
            self.futs[self.next] = self.pool.submit(self._read)
            self.next += 1
        return self.futs.pop(i).result() if i in self.futs else None

    def close(self):
        self.pool.shutdown(cancel_futures=True)
        self.video.close()


class _FieldReader:
    """Reads cache fields ahead of use on a small thread pool, in frame order.  With `device` (the device render path,
    DEVICE_NPZ) an .npz whose `flow` member carries a chunk index (storage/device_npz.py) is only read by the pool: get()
    uploads its bytes and inflates them on the device, and returns a device tensor whose CRC is looked at one field
    later.  Files without an index - the reference's, zlib's, .flo - are decoded by the pool as before."""

    def __init__(self, mgr, cache_dir, fmt, n, ahead=4, device=None):
        from concurrent.futures import ThreadPoolExecutor
        self.mgr, self.cache_dir, self.fmt, self.n, self.ahead = mgr, cache_dir, fmt, n, ahead
        self.device = device if fmt == 'npz' else None
        self.pool = ThreadPoolExecutor(max_workers=2, thread_name_prefix="render-read")
        self.futs = {}
        self.next = 0
        self.unchecked = None

    def _load(self, i):
        if self.device is not None:
            from storage import device_npz
            plan = device_npz.load_indexed(self.mgr._frame_file(self.cache_dir, i, 'npz'), 'flow')
            if plan is not None:
                return plan
        return self.mgr.load_cached_flow(self.cache_dir, i, self.fmt)

    def _check(self):
        if self.unchecked is not None:
            from vfml import hip
            (cells, crc), self.unchecked = self.unchecked, None
            hip.inflate_check(cells, crc)

    def get(self, i):
        while self.next < min(self.n, i + self.ahead + 1):
            self.futs[self.next] = self.pool.submit(self._load, self.next)
            self.next += 1
        got = self.futs.pop(i).result()
        if isinstance(got, dict):
            from storage import device_npz
            field, cells, crc = device_npz.inflate_indexed(got, self.device)
            self._check()                      # the field before this one, now that this one's work is queued
            self.unchecked = (cells, crc)
            return field
        return np.asarray(got, dtype=np.float32)

    def close(self):
        self.pool.shutdown(cancel_futures=True)
        self._check()


# The device render path's MJPG frames are encoded on the GPU (vfml_jpeg_encode_rgb); False: its
# composed frames go back uncompressed to the writer's Pillow pool, as --device cpu's do.
DEVICE_MJPG = True
# True: the flow cache's .npz members are deflated (the job) and inflated (the render stage) on the GPU
# (vfml_deflate_huffman / vfml_inflate_chunks); False: the writer's and the reader's host threads
# run zlib, as they always do for tiled jobs, --save-flow flo / both, --device cpu and an explicitly set
# VFML_NPZ_DEFLATE.  Off until fields/s and rendered frames/s have been measured against the host path (section 14's
# rule for the default); a device-written cache is read by either setting.
DEVICE_NPZ = False
# The chroma sampling of the output video's MJPG frames, on either path (vfml_jpeg_encode_rgb_sampled, or Pillow's
# subsampling= under --device cpu): "4:2:0", "4:2:2" or "4:4:4" ("Samplings").  The environment
# variable VFML_MJPG_SAMPLING overrides it.  A flow video for --flow-input should be 4:4:4: its vectors live in R and G,
# and sampled chroma smears them at every motion edge.
MJPG_SAMPLING = "4:2:0"
MJPG_SAMPLINGS = ("4:2:0", "4:2:2", "4:4:4")


def mjpg_sampling():
    """MJPG_SAMPLING, or VFML_MJPG_SAMPLING when it is set; a value outside MJPG_SAMPLINGS is refused."""
    value = os.environ.get("VFML_MJPG_SAMPLING") or MJPG_SAMPLING
    if value not in MJPG_SAMPLINGS:
        source = "VFML_MJPG_SAMPLING" if os.environ.get("VFML_MJPG_SAMPLING") else "flow_processor.MJPG_SAMPLING"
        raise ValueError(f"{source} = {value!r}: the MJPG frames are written as {', '.join(MJPG_SAMPLINGS)}")
    return value


# Fields of earlier frames whose keys and values a MemFlow field reads: 0, every field with an empty
# memory bank, as the reference runs it; 1..8, a job walks its frames in order through one stream with a bank of that many
# entries (one GPU, whole frames; the cache directory carries _mem{N}).  The environment variable VFML_MEMFLOW_MEMORY
# overrides it.  No command-line flag: the parser stays the reference's.
MEMFLOW_MEMORY = 0


def memflow_memory():
    """MEMFLOW_MEMORY, or VFML_MEMFLOW_MEMORY when it is set: an integer 0..8; anything else is refused."""
    from vfml.memflow_net import check_memory_frames
    env = os.environ.get("VFML_MEMFLOW_MEMORY")
    if env:
        return check_memory_frames(env, "VFML_MEMFLOW_MEMORY")
    return check_memory_frames(MEMFLOW_MEMORY, "flow_processor.MEMFLOW_MEMORY")


# True: in a MemFlow job every field's recurrence starts from the previous field's 1/8-resolution flow projected forward along
# itself (upstream's flow_init) instead of from zero: the job walks its frames in order through one
# stream, as with a memory bank (one GPU, whole frames; the cache directory carries _warm).  The environment variable
# VFML_MEMFLOW_WARM_START (0 or 1) overrides it.  No command-line flag: the parser stays the reference's.
MEMFLOW_WARM_START = False


def memflow_warm_start():
    """MEMFLOW_WARM_START, or VFML_MEMFLOW_WARM_START when it is set: 0 or 1; anything else is refused."""
    from vfml.memflow_net import check_warm_start
    env = os.environ.get("VFML_MEMFLOW_WARM_START")
    if env:
        return check_warm_start(env, "VFML_MEMFLOW_WARM_START")
    return check_warm_start(MEMFLOW_WARM_START, "flow_processor.MEMFLOW_WARM_START")


# Scene cuts: None, the clip is one continuous shot, as the reference treats it; (TH, R) or "TH,R" -
# or True / "1" for the defaults 200,3 - the job finds the clip's cuts from the frames on the device (vfml_scene_distances
# behind every upload) and keeps what it carries across frames inside a scene: the MOF / BOF window, MemFlow's pair, bank
# and warm start, and the output video's TAA histories (one GPU; the cache directory carries _cuts and a scenes.json).  The
# environment variable VFML_SCENE_CUTS (0, 1 or TH,R) overrides it.  No command-line flag: the parser stays the reference's.
SCENE_CUTS = None


def scene_cuts():
    """SCENE_CUTS, or VFML_SCENE_CUTS when it is set -> None or (TH, R); anything else is refused."""
    from video.scene_cuts import check_scene_cuts
    env = os.environ.get("VFML_SCENE_CUTS")
    if env:
        return check_scene_cuts(env, "VFML_SCENE_CUTS")
    return check_scene_cuts(SCENE_CUTS, "flow_processor.SCENE_CUTS")


# True: the output video carries the reference's text labels, drawn with the project's own text (DESIGN.md section 9,
# "Text"): vfml_text_draw behind the composer on the device path, visualization/text.py under --device cpu.  The
# environment variable VFML_LABELS=1|0 overrides it.  Off: the fixtures cut from the reference and the render tests pin
# the frames without text.
DRAW_LABELS = False


def draw_labels():
    """DRAW_LABELS, or VFML_LABELS when it is set; a value other than 1 or 0 is refused."""
    from visualization.video_composer import labels_switch
    return labels_switch(DRAW_LABELS)


def render_video(args, frames, fps, width, height, cache_dir, fmt, device, feeder=None, log=print):
    """Render the complete flow cache into the output AVI (reference process_video :958-1130, one frame at a time in
    its order): flow picture, the two TAA histories (--taa), the composed frame, the writer.  Device path: the frames
    are the clip on the device, each field goes up through a pinned ring, every step is a HIP kernel, and the composed
    frame - already in the AVI chunk's layout - comes back through a pinned ring one frame behind the GPU.  --device
    cpu runs the same loop with the host implementations.  With --taa --flow-input the frame is the 2x3 grid: the
    flow video's encoded half is decoded per frame (vfml_flow_decode), feeds a third TAA history and the difference
    overlay (vfml_flow_diff_overlay), and its re-encoded picture takes the flow tile's place.
    width x height is the size the job ran at: the frames' own, or under --fast the reduced one - then `frames` are
    already reduced (--device cpu) or still at the source's size on the host, and the ClipFeeder built here or handed in
    resizes them on the device (vfml_resize_u8).  A cache whose fields have another size is refused.
    A cache directory with a scenes.json (a job with scene cuts on) restarts every TAA history at each
    scene start: the first frame of a scene is rendered as frame 0 is."""
    from effects.taa_processor import TAAProcessor
    from storage.avi_writer import AviWriter, dib_stride
    from visualization.video_composer import (compose_device, create_6_video_grid, create_difference_overlay,
                                              create_side_by_side)

    n = len(frames)
    from video.scene_cuts import read_scenes
    scenes = read_scenes(cache_dir)
    cuts = frozenset(s for s in scenes["starts"] if 0 < s < n) if scenes else frozenset()
    if scenes:
        log(f"Scene cuts: {len(cuts) + 1} scenes, the TAA histories restart at frames {sorted(cuts)}")
    cached = tuple(np.shape(FlowCacheManager().load_cached_flow(cache_dir, 0, fmt))[:2])
    if cached != (height, width):
        raise ValueError(f"Flow cache {cache_dir} holds {cached[1]}x{cached[0]} fields, the frames are {width}x{height}: "
                         f"it was written at another resolution (a `fast` cache from before --fast reduced the "
                         f"frames, or a foreign --use-flow-cache). Recompute it with --force-recompute.")
    output_path = render_output_path(args, fps, log)
    log(f"Processing: {args.input} -> {output_path}")
    log(f"Video FPS: {fps:.2f}")
    flow_only, taa = args.flow_only, args.taa and not args.flow_only     # --flow-only's stacked frame shows no TAA
    size = (width, height * 2) if args.flow_only else ((width * 2, height * 2) if args.taa else (width * 2, height))
    external = None
    if args.flow_input is not None:
        check_flow_input(args)
        if args.flow_only:
            log("note: --flow-only writes the stacked frame without TAA, so --flow-input's 2x3 grid is not rendered")
        elif not args.taa:
            log("note: --flow-input is compared in the --taa grid only; without --taa the ordinary video is rendered")
        else:
            external = _ExternalFlowSource(args.flow_input, n, width, height, log, device=device)
            size = (width * 2, height * 3)
    sampling = mjpg_sampling()
    labels = draw_labels()
    model_name = "VideoFlow"    # (the reference's process_video :1124 never sees its other name: it has no `model` attribute)
    if args.uncompressed:
        log("Using uncompressed video codec. Output will be .avi and file size will be very large.")
    else:
        log("Using MJPG codec. Output will be .avi for compatibility.")
        if args.flow_only and args.flow_format in FLOW_INPUT_VARIANTS and sampling == "4:2:0":
            log(f"note: MJPG_SAMPLING is 4:2:0: a {args.flow_format} video with sampled chroma loses its vectors at motion "
                f"edges (R and G are smeared there); set VFML_MJPG_SAMPLING=4:4:4 for a video that --flow-input reads back")
    gpu = str(device).startswith('cuda')
    from vfml.dist import host_cpu_share
    jpeg_workers = max(1, min(8, host_cpu_share()))
    # MJPG on the device path: the frames are encoded on the GPU (vfml_jpeg_encode_rgb) and the writer takes finished JPEGs
    writer = AviWriter(output_path, 0 if args.uncompressed else 'MJPG', fps, size, workers=jpeg_workers,
                       depth=jpeg_workers + 1, log=log, encoder='external' if gpu and DEVICE_MJPG else 'pillow',
                       sampling=sampling)
    encoder = render_encoder(args.flow_format, args.motion_vectors_clamp_range)
    taa_flow, taa_simple, taa_external = TAAProcessor(alpha=0.1), TAAProcessor(alpha=0.1), TAAProcessor(alpha=0.1)
    variant = FLOW_INPUT_VARIANTS.get(args.flow_format)
    reader = _FieldReader(FlowCacheManager(), cache_dir, fmt, n, device=device if gpu and DEVICE_NPZ else None)
    log(ENCODER_LINES.get(args.flow_format, ENCODER_LINES['gamedev']).format(c=args.motion_vectors_clamp_range))
    t0 = time.time()
    try:
        if not gpu:
            from encoding.flow_encoders import decode_motion_vectors
            prev = ext_flow = None
            for i in range(n):
                field = reader.get(i)
                viz = encoder.encode(field, width, height) if external is None else None
                taa_frame = taa_simple_frame = None
                if i in cuts:               # a scene starts: nothing of the old one is blended in
                    prev = None
                    for t in (taa_flow, taa_simple, taa_external):
                        t.reset_history()
                if taa:
                    taa_frame = taa_flow.apply_taa(frames[i], flow_pixels=prev, alpha=0.1, use_flow=True,
                                                   sequence_id='flow_taa')
                    taa_simple_frame = taa_simple.apply_taa(frames[i], flow_pixels=None, alpha=0.1, use_flow=False,
                                                            sequence_id='simple_taa')
                prev = field
                if external is not None:
                    # this frame's external flow from frame 0 on, where the computed-flow TAA uses the previous field
                    picture = external.get(i)
                    if picture is not None:
                        ext_flow = decode_motion_vectors(picture, clamp_range=args.motion_vectors_clamp_range,
                                                         format_variant=variant)
                    taa_ext = taa_external.apply_taa(frames[i], flow_pixels=ext_flow, alpha=0.1, use_flow=True,
                                                     sequence_id='external_taa')
                    writer.write(create_6_video_grid(frames[i], encoder.encode(ext_flow, width, height), taa_frame,
                                                     taa_simple_frame, taa_ext,
                                                     create_difference_overlay(field, ext_flow, labels=labels),
                                                     labels=labels))
                    continue
                writer.write(create_side_by_side(frames[i], viz, flow_only=flow_only, taa_frame=taa_frame,
                                                 taa_simple_frame=taa_simple_frame, model_name=model_name,
                                                 fast_mode=args.fast, flow_format=args.flow_format, labels=labels))
        else:
            _render_device(frames, width, height, device, feeder, reader, encoder, taa, flow_only, writer, size,
                           args.uncompressed, taa_flow, taa_simple, dib_stride, compose_device, external=external,
                           taa_external=taa_external, variant=variant, clamp_range=args.motion_vectors_clamp_range,
                           label_ops=_label_ops(width, height, taa, flow_only, external is not None, model_name,
                                                args.fast, args.flow_format) if labels else None, cuts=cuts)
    finally:
        if external is not None:
            external.close()
        reader.close()
        writer.release()
    dt = time.time() - t0
    log(f"Video written: {output_path} ({n} frames {size[0]}x{size[1]}, {n / max(dt, 1e-9):.2f} frames/s)")
    return 0


def _label_ops(width, height, taa, flow_only, grid6, model_name, fast_mode, flow_format):
    """The draw list of a layout's labels in frame coordinates, as the host composer draws them: the tiles' labels with
    tile clips; for the 2x3 grid the legend's numbers on the difference tile, then the six grid labels.  Black and
    white only, so the list serves RGB and BGR frames alike."""
    from visualization import text as vtext
    if flow_only:
        return []
    if grid6:
        return vtext.legend_ops(height, width, tile=(width, 2 * height)) + vtext.grid6_ops(height, width)
    return vtext.side_by_side_ops(height, width, 2 if taa else 0, model_name, fast_mode, flow_format)


def _render_device(frames, width, height, device, feeder, reader, encoder, taa, flow_only, writer, size, uncompressed,
                   taa_flow, taa_simple, dib_stride, compose_device, external=None, taa_external=None, variant=None,
                   clamp_range=32.0, label_ops=None, cuts=frozenset()):
    from vfml import hip
    n = len(frames)
    text_plan = None            # the labels of the layout, compiled once: drawn on every composed frame
    if label_ops:
        from visualization.text import build_plan
        text_plan = hip.TextPlan(build_plan(label_ops, size[1], size[0]), device)
        if text_plan.boxes == 0:
            text_plan = None
    if feeder is None:
        feeder = ClipFeeder(frames, device, size=(height, width))      # (host frames of another size: --fast's source frames)
    stream = torch.cuda.current_stream()
    # fields: host -> pinned slot -> device; a slot is refilled once its copy has left it
    fslots = [torch.empty((height, width, 2), dtype=torch.float32).pin_memory() for _ in range(3)]
    fevents = [None] * len(fslots)
    # --flow-input: the encoded pictures (3 bytes per pixel) take the same way and are decoded on the device
    eslots, eevents = [], []    # (made when the first picture comes: a flow video of JPEG files does not need them)
    uploads = 0
    ext_flow = None
    mjpg = None                 # --flow-input from an MJPG .avi: its frames are decoded here (DeviceMjpgDecoder)
    decode_mode = hip.ENCODE_RG8 if variant == 'rg8' else hip.ENCODE_RGB8
    # composed frames: device -> pinned slot -> writer; a slot is reused once the writer no longer holds it.  MJPG: the
    # frame stays on the device, the JPEG encoder runs behind the composer and only its scan comes back
    stride = dib_stride(size[0]) if uncompressed else 3 * size[0]
    jpeg = None
    if writer.external:
        from storage.device_mjpg import DeviceMjpgEncoder
        jpeg = DeviceMjpgEncoder(writer, size[1], size[0], device, sampling=writer.sampling)
    nslots = 0 if jpeg is not None else writer.in_flight_limit() + 3
    oslots = [torch.empty((size[1], stride), dtype=torch.uint8).pin_memory() for _ in range(nslots)]
    oevents = [None] * nslots
    pending = None              # (slot) composed on the device, not yet handed to the writer
    prev = None
    for i in range(n):
        feeder.ensure(min(i + 2, n - 1), need=i)
        frame = feeder.clip[i]
        k = i % len(fslots)
        host = reader.get(i)
        if torch.is_tensor(host):
            field = host            # an indexed .npz member: inflated on the device, it never was on the host uncompressed
        else:
            if fevents[k] is not None:
                fevents[k].synchronize()
            np.copyto(fslots[k].numpy(), host)
            field = fslots[k].to(device, non_blocking=True)
            fevents[k] = torch.cuda.Event()
            fevents[k].record(stream)
        viz = encoder.encode(field, width, height) if external is None else None
        taa_frame = taa_simple_frame = None
        if i in cuts:                       # a scene starts: nothing of the old one is blended in
            prev = None
            for t in (taa_flow, taa_simple, taa_external):
                if t is not None:
                    t.reset_history()
        if taa:
            taa_frame = taa_flow.apply_taa(frame, flow_pixels=prev, alpha=0.1, use_flow=True, sequence_id='flow_taa')
            taa_simple_frame = taa_simple.apply_taa(frame, flow_pixels=None, alpha=0.1, use_flow=False,
                                                    sequence_id='simple_taa')
        prev = field
        taa_ext = diff = None
        if external is not None:
            picture = external.get(i)
            if isinstance(picture, tuple):
                # the JPEG file goes up instead of the picture; rows H//2... are decoded into the tensor flow_decode reads
                if mjpg is None:
                    from storage.device_mjpg import DeviceMjpgDecoder
                    mjpg = DeviceMjpgDecoder(device)
                encoded = mjpg.submit(picture[0], picture[1], rows=external.rows)
                ext_flow = hip.flow_decode(encoded, decode_mode, clamp_range)
            elif picture is not None:
                if not eslots:
                    eslots = [torch.empty((height, width, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
                    eevents = [None] * len(eslots)
                e = uploads % len(eslots)
                uploads += 1
                if eevents[e] is not None:
                    eevents[e].synchronize()
                np.copyto(eslots[e].numpy(), picture)
                encoded = eslots[e].to(device, non_blocking=True)
                eevents[e] = torch.cuda.Event()
                eevents[e].record(stream)
                ext_flow = hip.flow_decode(encoded, decode_mode, clamp_range)
            taa_ext = taa_external.apply_taa(frame, flow_pixels=ext_flow, alpha=0.1, use_flow=True,
                                             sequence_id='external_taa')
            viz = encoder.encode(ext_flow, width, height)     # the flow tile shows the external flow, re-encoded
            diff = hip.flow_diff_overlay(field, ext_flow)
        out = compose_device(frame, viz, taa_frame, taa_simple_frame, flow_only=flow_only, bgr=uncompressed,
                             bottom_up=uncompressed, row_stride=stride, taa_external_frame=taa_ext,
                             difference_overlay=diff)
        if text_plan is not None:
            hip.text_draw(text_plan, out, size[1], size[0], row_stride=stride, bottom_up=uncompressed)
        if jpeg is not None:
            jpeg.submit(out.view(size[1], size[0], 3))
            continue
        s = i % nslots
        writer.drain(keep=nslots - 2)        # the slot's previous frame is no longer in the writer's hands
        oslots[s].copy_(out, non_blocking=True)
        oevents[s] = torch.cuda.Event()
        oevents[s].record(stream)
        if pending is not None:
            _hand_over(writer, oslots[pending], oevents[pending], size, uncompressed)
        pending = s
    if pending is not None:
        _hand_over(writer, oslots[pending], oevents[pending], size, uncompressed)
    if jpeg is not None:
        jpeg.finish()
    if mjpg is not None:
        mjpg.finish()


def _hand_over(writer, slot, event, size, uncompressed):
    event.synchronize()
    buf = slot.numpy()
    writer.write_payload(buf if uncompressed else buf.reshape(size[1], size[0], 3))


def main(argv=None):
    args = build_parser().parse_args(argv)
    rank, local_rank, world = vdist.init_distributed()
    log = print if rank == 0 else (lambda *a, **k: None)

    if args.show_tiles:
        log("note: --show-tiles concerns video composition / visualisation, which this build does not do; ignored")
    if args.flow_input is not None:
        check_flow_input(args)
    mjpg_sampling()             # a setting that is not built is refused before anything is computed or rendered
    draw_labels()               # (likewise VFML_LABELS)
    memory = memflow_memory()   # (likewise VFML_MEMFLOW_MEMORY)
    warm = memflow_warm_start()  # (likewise VFML_MEMFLOW_WARM_START)
    try:
        cuts = scene_cuts()     # (likewise VFML_SCENE_CUTS)
    except ValueError as e:
        log(f"Error: {e}")
        return 1
    if args.model != 'memflow':
        memory, warm = 0, False
    try:
        check_memory_job(memory, bool(args.tile), world, warm)
        check_scene_job(cuts, not args.tile, world)
    except ValueError as e:
        log(f"Error: {e}")
        return 1
    if not (args.input.startswith('synthetic:') or os.path.exists(args.input)):
        log(f"Error: Input video not found: {args.input}")
        return 1

    device = DeviceManager().get_device(args.device)
    if device == 'cuda' and world > 1:
        torch.cuda.set_device(local_rank)
        device = f"cuda:{local_rank}"
    try:
        start_frame, max_frames = resolve_frame_range(args.input, args.start_frame, args.frames, args.start_time,
                                                      args.duration, log)
    except ValueError as e:
        log(f"Error: {e}")
        return 1
    if max_frames <= 0:
        log(f"Error: empty frame range (start {start_frame}, {max_frames} frames)")
        return 1
    frames, fps, width, height, start = load_frames(args.input, start_frame, max_frames)
    n = len(frames)
    if args.fast:
        # the whole job runs at the reduced size.  On a GPU the frames stay as they are on the host and every ClipFeeder
        # resizes them behind their upload; --device cpu resizes them here
        width, height = fast_mode_size(width, height, log)
        if frames[0].shape[:2] != (height, width) and not str(device).startswith('cuda'):
            frames = [resize_frame(f, (width, height)) for f in frames]
    mgr = FlowCacheManager()
    cache_src = args.input if not args.input.startswith('synthetic:') else os.path.join(args.output, args.input.replace(':', '_') + ".npy")
    memflow = args.model == 'memflow'
    cache_dir = args.use_flow_cache or mgr.generate_cache_path(
        cache_src, start, n, args.sequence_length, args.fast, args.tile, args.model,
        args.stage if memflow else args.vf_dataset, args.vf_architecture, args.vf_variant, memory_frames=memory,
        warm_start=warm, scene_cuts=cuts)
    complete, fmt, missing = mgr.check_cache_exists(cache_dir, n)
    if complete and not args.force_recompute:
        if args.interactive:
            log(f"Flow cache complete ({fmt}), nothing to compute: {cache_dir}")
            return 0
        if rank != 0:
            return 0
        log(f"Using optical flow cache from: {cache_dir} (format: {fmt})")
        return render_video(args, frames, fps, width, height, cache_dir, fmt, device, log=log)

    if memflow:     # reference flow_processor.py:64-75: model path defaults to MemFlow_ckpt/MemFlowNet_{stage}.pth
        eng = MemFlowInference(device, args.model_path or f"MemFlow_ckpt/MemFlowNet_{args.stage}.pth", args.stage,
                               args.sequence_length, memory_frames=memory, warm_start=warm)
    else:
        eng = VideoFlowInference(device, args.fast, args.tile, args.sequence_length, args.vf_dataset,
                                 args.vf_architecture, args.vf_variant)
    eng.load_model()
    proc = eng.get_processor()
    # frames go up through a pinned ring while earlier fields compute (--fast: and are resized on the device behind it)
    # (with scene cuts on: and measured against their predecessor there)
    feeder = ClipFeeder(frames, device, size=(height, width), scene_cuts=cuts)
    save_format = args.save_flow or 'npz'
    tiled = bool(args.tile and not memflow)
    num_lods = 0 if args.skip_lods else 5
    gpu_lods = 0 if (args.skip_lods or save_format == 'flo') else 5
    # Whole-frame jobs: EVERY rank writes the cache files of its own fields (one node = one filesystem; the reference's
    # cache is a directory of per-frame files, storage/cache_manager.py:247-262) - no gather, and the writers' compression
    # threads scale with the GPUs instead of funnelling every field into rank 0's.  Tiled jobs: tiles of one frame come
    # from several ranks, so they stream to rank 0 (chunked gathers), which pastes and writes.
    per_rank = not tiled
    cpus = max(1, vdist.host_cpu_share() // (world if per_rank else 1))
    writer = AsyncFlowCacheWriter(cache_dir, save_format, workers=min(16, cpus), num_lods=num_lods,
                                  manager=mgr) if (per_rank or rank == 0) else None
    t0 = time.time()
    # LOD levels are reduced on the GPU that computed the field (bit-identical to the reference's loop) and travel
    # with it; tiled frames are assembled on rank 0 and reduced by the writer's threads
    sink = (lambda k, field, lods: writer.submit(field, k, lods)) if writer is not None else None
    # whole-frame .npz jobs on a GPU: fields and LOD levels are deflated on the device, the writer gets finished streams
    device_npz = (DEVICE_NPZ and per_rank and save_format == 'npz' and str(device).startswith('cuda')
                  and "VFML_NPZ_DEFLATE" not in os.environ)
    if device_npz:
        from storage.device_npz import CHUNK_BYTES, DeviceNpzWriter
        from vfml import hip
        device_npz = hip.deflate_capacity(height * width * 8, CHUNK_BYTES) > 0     # (a field of more chunks than an index holds)
    if device_npz:
        npz = DeviceNpzWriter(device, writer.submit_members)
        run_sharded(proc, None, range(n), tile_mode=False, rank=rank, world=world, feeder=feeder, device_npz=npz,
                    collect=False, num_lods=gpu_lods)
        npz.finish()
    elif per_rank:
        run_sharded(proc, None, range(n), tile_mode=False, rank=rank, world=world, feeder=feeder, local_sink=sink,
                    collect=False, num_lods=gpu_lods)
    else:
        run_sharded(proc, None, range(n), tile_mode=True, rank=rank, world=world, feeder=feeder, on_field=sink,
                    collect=False, num_lods=gpu_lods)
    if str(device).startswith('cuda'):
        torch.cuda.synchronize()
    if torch.distributed.is_initialized():
        torch.distributed.barrier()                 # every rank's fields are computed and handed to a writer
    dt = time.time() - t0
    if writer is not None:
        writer.close()
    if cuts and rank == 0:
        from video.scene_cuts import write_scenes
        feeder.ensure(n - 1)                        # (every frame has been measured: the job reached the last one)
        index = feeder.scenes
        write_scenes(cache_dir, index)
        log(f"Scene cuts (threshold {index.th}, ratio {index.r}): {len(index.starts)} scenes, starting at frames "
            f"{index.starts}")
    if torch.distributed.is_initialized():
        torch.distributed.barrier()                 # every rank's files are on disk
    if rank == 0:
        dt_all = time.time() - t0
        log(f"{n} flow fields ({width}x{height}, seq {args.sequence_length}) in {dt:.2f} s = {n / dt:.2f} fields/s "
            f"on {world} GPU(s)")
        log(f"Flow cache written: {cache_dir} ({n / max(dt_all, 1e-9):.1f} fields/s end to end, incl. "
            f"{'no ' if args.skip_lods else ''}LODs)")
        complete, _, missing = mgr.check_cache_exists(cache_dir, n)
        if not complete:
            log(f"Error: flow cache incomplete after the job, missing frames {missing[:8]}{'...' if len(missing) > 8 else ''}")
            return 1
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    if rank == 0 and not args.interactive:
        _, fmt, _ = mgr.check_cache_exists(cache_dir, n)
        return render_video(args, frames, fps, width, height, cache_dir, fmt, device, feeder=feeder, log=log)
    return 0


if __name__ == "__main__":
    sys.exit(main())
