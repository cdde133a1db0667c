"""Flow cache: .flo / .npz files, completeness check, LOD pyramids.

File formats and names are byte-compatible with reference storage/cache_manager.py:
  .flo  b'PIEH' + <I width + <I height + float32 [H][W][2]                   (:18-30, :50-64)
  .npz  np.savez_compressed with members flow f32[H,W,2], frame_idx, shape, dtype   (:33-47, :247-262)
  names flow_frame_{i:06d}.{flo,npz} and flow_frame_{i:06d}_lod{k}.npz        (:208, :290-299)
The LOD generator keeps the reference's semantics (:77-161: pad odd sides bottom/right with zero
weight, 2x2 weighted mean, vectors x0.5) but is vectorised instead of a per-pixel Python loop.
"""
import collections
import os
import struct
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

try:
    from tqdm import tqdm
except Exception:  # pragma: no cover - tqdm is optional plumbing
    def tqdm(it, **_):
        return it


def _to_numpy(flow):
    return flow.cpu().numpy() if torch.is_tensor(flow) else flow


# ---- .npz writer ----------------------------------------------------------------------------------------------------
# `np.savez_compressed` (reference storage/cache_manager.py:47, :262) = a zip archive whose members `<name>.npy` are
# deflated at zlib's default level.  What a reader (np.load, the reference's load_flow_npz) depends on is the member
# layout - names, dtypes, shapes, values - not on how the deflate stream was produced.  A float32 flow field is nearly
# incompressible to LZ77 (its mantissa bytes are noise); all of deflate's ~12 % comes from entropy-coding the exponent
# bytes.  Z_HUFFMAN_ONLY skips the match search and lands on the same size 7x faster (130 vs 930 ms per 1080p field,
# 0.876 of the raw size either way), which is what lets the cache writer keep up with the engine.
# VFML_NPZ_DEFLATE = huffman (default) | zlib (np.savez_compressed itself, the reference's call) | stored (no compression).
_ZIP_LOCAL = struct.Struct('<4sHHHHHIIIHH')
_ZIP_CENTRAL = struct.Struct('<4sHHHHHHIIIHHHHHII')
_ZIP_END = struct.Struct('<4sHHHHIIH')


def _npy_parts(value):
    """-> (header bytes, C-contiguous array) of the .npy serialisation np.savez would store for `value`."""
    import io
    arr = np.asanyarray(value)
    if not arr.flags.c_contiguous:              # (np.ascontiguousarray would also turn a 0-d member into a 1-d one)
        arr = np.ascontiguousarray(arr)
    if arr.dtype.hasobject:
        raise ValueError("object arrays are not written to the flow cache")
    head = io.BytesIO()
    np.lib.format.write_array_header_1_0(head, np.lib.format.header_data_from_array_1_0(arr))
    return head.getvalue(), arr


class ZipMember(collections.namedtuple("ZipMember", "name method crc size chunks extra")):
    """A ready-made member `<name>.npy` of an archive: zip method (8 deflate, 0 stored), CRC-32 and size of the
    uncompressed .npy bytes, the pieces of the data as they go into the file, the extra field of both headers."""
    __slots__ = ()


def host_member(name, value, method):
    """The ZipMember of `value`, coded on the host: method 8 = Z_HUFFMAN_ONLY deflate, 0 = stored."""
    import zlib
    head, arr = _npy_parts(value)
    raw = memoryview(arr.reshape(-1).view(np.uint8)) if arr.size else memoryview(b'')
    crc = zlib.crc32(raw, zlib.crc32(head))
    size = len(head) + raw.nbytes
    if method == 8:
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        chunks = [co.compress(head), co.compress(raw), co.flush()]
    else:
        chunks = [head, raw]
    return ZipMember(name, method, crc, size, chunks, b'')


def write_zip(filename, members):
    """Lay out a zip archive from ZipMembers (host_member's, or storage.device_npz's with a stream that the GPU coded):
    local headers, data, central directory."""
    central, offset = [], 0
    with open(filename, 'wb') as f:
        for name, method, crc, size, chunks, extra in members:
            csize = sum(len(c) for c in chunks)
            if size >= 0xFFFFFFFF or csize >= 0xFFFFFFFF:
                raise ValueError("flow-cache member of 4 GiB or more")
            if len(extra) > 0xFFFF:
                raise ValueError("zip extra field of more than 65535 bytes")
            fname = (name + '.npy').encode()
            # version 2.0, no flags, DOS time 1980-01-01 (as zipfile stamps members without a file behind them)
            f.write(_ZIP_LOCAL.pack(b'PK\x03\x04', 20, 0, method, 0, 0x21, crc, csize, size, len(fname), len(extra)))
            f.write(fname)
            f.write(extra)
            for c in chunks:
                f.write(c)
            central.append(_ZIP_CENTRAL.pack(b'PK\x01\x02', 20, 20, 0, method, 0, 0x21, crc, csize, size, len(fname),
                                             len(extra), 0, 0, 0, 0x01800000, offset) + fname + extra)
            offset += _ZIP_LOCAL.size + len(fname) + len(extra) + csize
        cd = b''.join(central)
        f.write(cd)
        f.write(_ZIP_END.pack(b'PK\x05\x06', 0, 0, len(central), len(central), len(cd), offset, 0))


def npz_mode(mode=None):
    mode = mode or os.environ.get("VFML_NPZ_DEFLATE", "huffman")
    if mode not in ("huffman", "stored", "zlib"):
        raise ValueError(f"VFML_NPZ_DEFLATE={mode!r}: huffman, zlib or stored")
    return mode


def write_npz(filename, members, mode=None):
    """Write {name: array-like} as an .npz archive np.load reads back member for member like np.savez_compressed's.
    A value may also be a ZipMember: it is laid out as it is."""
    mode = npz_mode(mode)
    if mode == "zlib":
        np.savez_compressed(filename, **members)
        return
    if not str(filename).endswith('.npz'):       # (np.savez appends the suffix too)
        filename = str(filename) + '.npz'
    method = 8 if mode == "huffman" else 0
    write_zip(filename, [value if isinstance(value, ZipMember) else host_member(name, value, method)
                         for name, value in members.items()])


class FlowFileHandler:
    @staticmethod
    def save_flow_flo(flow: np.ndarray, filename: str):
        flow = _to_numpy(flow)
        h, w = flow.shape[:2]
        with open(filename, 'wb') as f:
            f.write(b'PIEH' + struct.pack('<II', w, h))
            f.write(flow.astype(np.float32).tobytes())

    @staticmethod
    def save_flow_npz(flow: np.ndarray, filename: str, frame_idx: Optional[int] = None,
                      metadata: Optional[Dict[str, Any]] = None):
        members = {'flow': _to_numpy(flow).astype(np.float32)}
        if frame_idx is not None:
            members['frame_idx'] = frame_idx
        if metadata is not None:
            members.update(metadata)
        write_npz(filename, members)

    @staticmethod
    def load_flow_flo(filename: str) -> np.ndarray:
        with open(filename, 'rb') as f:
            magic = f.read(4)
            if magic != b'PIEH':
                raise ValueError(f"Invalid .flo file magic number: {magic}")
            w, h = struct.unpack('<II', f.read(8))
            data = f.read(w * h * 8)
        return np.frombuffer(data, dtype=np.float32).reshape(h, w, 2)

    @staticmethod
    def load_flow_npz(filename: str) -> Dict[str, Any]:
        return dict(np.load(filename))


class LODGenerator:
    @staticmethod
    def generate_lods(flow: np.ndarray, num_lods: int = 5) -> List[np.ndarray]:
        """[original, lod1, ...]; each level halves H and W (rounding up) and halves the vectors.
        A flow tensor that is still on the GPU is reduced there (vfml_flow_lod, bit-identical)."""
        if torch.is_tensor(flow) and flow.is_cuda and flow.dtype == torch.float32:
            from vfml import hip
            return [t.cpu().numpy() for t in hip.flow_lods(flow, num_lods)]
        flow = _to_numpy(flow)
        lods = [flow]
        cur = flow
        for _ in range(1, num_lods):
            h, w = cur.shape[:2]
            ph, pw = h % 2, w % 2
            wgt = np.pad(np.ones((h, w), np.float32), ((0, ph), (0, pw)))
            val = np.pad(cur.astype(np.float32), ((0, ph), (0, pw), (0, 0)))
            nh, nw = (h + ph) // 2, (w + pw) // 2
            v4 = val.reshape(nh, 2, nw, 2, 2)
            w4 = wgt.reshape(nh, 2, nw, 2)
            # same summation order as np.sum over the 2x2 block in the reference (row-major)
            num = (v4 * w4[..., None]).transpose(0, 2, 1, 3, 4).reshape(nh, nw, 4, 2)
            den = w4.transpose(0, 2, 1, 3).reshape(nh, nw, 4)
            tot = ((den[..., 0] + den[..., 1]) + den[..., 2]) + den[..., 3]
            acc = ((num[..., 0, :] + num[..., 1, :]) + num[..., 2, :]) + num[..., 3, :]
            with np.errstate(invalid='ignore', divide='ignore'):
                out = np.where(tot[..., None] > 0, acc / tot[..., None] * np.float32(0.5), 0).astype(np.float32)
            lods.append(out)
            cur = out
        return lods


class FlowCacheManager:
    def __init__(self):
        self.file_handler = FlowFileHandler()
        self.lod_generator = LODGenerator()

    @staticmethod
    def _frame_file(cache_dir, frame_idx, ext, lod=None):
        tail = "" if lod is None else f"_lod{lod}"
        return os.path.join(cache_dir, f"flow_frame_{frame_idx:06d}{tail}.{ext}")

    def generate_cache_path(self, input_path: str, start_frame: int, max_frames: int, sequence_length: int,
                            fast_mode: bool, tile_mode: bool, model: str = 'videoflow', dataset: str = 'things',
                            architecture: str = 'mof', variant: str = 'noise', memory_frames: int = 0,
                            warm_start: bool = False, scene_cuts=None) -> str:
        from .filename_generator import generate_cache_directory
        return generate_cache_directory(input_path=input_path, start_frame=start_frame, max_frames=max_frames,
                                        sequence_length=sequence_length, fast_mode=fast_mode, tile_mode=tile_mode,
                                        model=model, dataset=dataset, architecture=architecture, variant=variant,
                                        memory_frames=memory_frames, warm_start=warm_start, scene_cuts=scene_cuts)

    def check_cache_exists(self, cache_dir: str, max_frames: int) -> Tuple[bool, Optional[str], List[int]]:
        """(complete?, 'npz'|'flo'|None, missing frame indices).  Any .npz in the directory (LOD files
        included) selects the npz format, as in the reference (:201-206)."""
        everything = list(range(max_frames))
        if not os.path.exists(cache_dir):
            return False, None, everything
        names = os.listdir(cache_dir)
        if any(n.endswith('.npz') for n in names):
            fmt = 'npz'
        elif any(n.endswith('.flo') for n in names):
            fmt = 'flo'
        else:
            return False, None, everything
        missing = [i for i in everything if not os.path.exists(self._frame_file(cache_dir, i, fmt))]
        return (not missing), (None if missing else fmt), missing

    def load_cached_flow(self, cache_dir: str, frame_idx: int, format_type: str = 'auto') -> np.ndarray:
        npz = self._frame_file(cache_dir, frame_idx, 'npz')
        flo = self._frame_file(cache_dir, frame_idx, 'flo')
        if format_type == 'auto':
            if os.path.exists(npz):
                format_type = 'npz'
            elif os.path.exists(flo):
                format_type = 'flo'
            else:
                raise FileNotFoundError(f"No cached flow found for frame {frame_idx}")
        if format_type == 'npz':
            return self.file_handler.load_flow_npz(npz)['flow']
        if format_type == 'flo':
            return self.file_handler.load_flow_flo(flo)
        raise ValueError(f"Invalid format_type: {format_type}")

    def save_flow_to_cache(self, flow: np.ndarray, cache_dir: str, frame_idx: int, save_format: str = 'npz'):
        os.makedirs(cache_dir, exist_ok=True)
        if save_format in ('flo', 'both'):
            self.file_handler.save_flow_flo(flow, self._frame_file(cache_dir, frame_idx, 'flo'))
        if save_format in ('npz', 'both'):
            meta = {'frame_idx': frame_idx, 'shape': flow.shape, 'dtype': str(flow.dtype)}
            self.file_handler.save_flow_npz(flow, self._frame_file(cache_dir, frame_idx, 'npz'), frame_idx, meta)

    def save_optical_flow_files(self, flow: np.ndarray, base_filename: str, frame_idx: int, save_format: str):
        flow = _to_numpy(flow)
        meta = {'frame_idx': frame_idx, 'shape': flow.shape, 'dtype': str(flow.dtype),
                'min_flow': float(np.min(flow)), 'max_flow': float(np.max(flow)),
                'mean_magnitude': float(np.mean(np.sqrt(flow[:, :, 0] ** 2 + flow[:, :, 1] ** 2)))}
        stem = f"{base_filename}_frame_{frame_idx:06d}"
        if save_format in ('flo', 'both'):
            self.file_handler.save_flow_flo(flow, stem + ".flo")
        if save_format in ('npz', 'both'):
            self.file_handler.save_flow_npz(flow, stem + ".npz", frame_idx, meta)

    def save_flow_lods(self, lods: List[np.ndarray], cache_dir: str, frame_idx: int):
        os.makedirs(cache_dir, exist_ok=True)
        for level, data in enumerate(lods):
            meta = {'frame_idx': frame_idx, 'lod_level': level, 'shape': data.shape, 'dtype': str(data.dtype)}
            self.file_handler.save_flow_npz(data, self._frame_file(cache_dir, frame_idx, 'npz', level), frame_idx, meta)

    def load_flow_lod(self, cache_dir: str, frame_idx: int, lod_level: int = 0) -> np.ndarray:
        name = self._frame_file(cache_dir, frame_idx, 'npz', lod_level)
        if not os.path.exists(name):
            raise FileNotFoundError(f"LOD {lod_level} not found for frame {frame_idx}")
        return self.file_handler.load_flow_npz(name)['flow']

    def check_flow_lods_exist(self, cache_dir: str, max_frames: int, num_lods: int = 5) -> bool:
        return os.path.exists(cache_dir) and all(
            os.path.exists(self._frame_file(cache_dir, i, 'npz', k))
            for i in range(max_frames) for k in range(num_lods))

    def generate_lods_for_cache(self, cache_dir: str, max_frames: int, num_lods: int = 5):
        print(f"Generating LOD pyramids (levels 0-{num_lods-1}) for {max_frames} frames...")
        for i in tqdm(range(max_frames), desc="Generating LODs"):
            self.save_flow_lods(self.lod_generator.generate_lods(self.load_cached_flow(cache_dir, i), num_lods),
                                cache_dir, i)
        print(f"LOD generation complete. Generated {num_lods} levels for {max_frames} frames.")
