"""AVI reader in pure Python: reads back what storage/avi_writer.py writes (and files of the same kinds from elsewhere).
No OpenCV.

* uncompressed: 24-bit BI_RGB DIB frames - BGR, bottom-up rows (top-down when the header's height is negative), each
  row padded to 4 bytes.
* MJPG: each chunk a JPEG, decoded with Pillow; without Pillow the reader says so when a frame is asked for.
* single RIFF files and OpenDML (AVI 2.0) ones: the `AVIX` segments are walked like the first.
* `probe(path)` takes frame count, rate, size and codec from the headers (`odml/dmlh` total when present, else `strh`)
  without touching a frame; `AviReader.read()` hands out RGB [H,W,3] uint8 frames in order, seeking from chunk to chunk
  (no index chunk is needed, a frame's bytes are read when it is asked for).

Any other codec or pixel format is an error that names it.
"""
import struct

import numpy as np

from .avi_writer import dib_stride


class AviError(ValueError):
    pass


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _read_headers(f):
    """-> dict(width, height, top_down, bits, codec, fps, frames, stream, movi_end_of_headers) from the first RIFF."""
    head = f.read(12)
    if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'AVI ':
        raise AviError("not an AVI file (no RIFF/AVI header)")
    info = {"frames_avih": 0, "frames_strh": 0, "frames_dmlh": 0, "stream": None}
    riff_end = 8 + struct.unpack('<I', head[4:8])[0]
    nstreams = [0]

    def walk(start, end):
        p = start
        while p + 8 <= end:
            f.seek(p)
            hdr = f.read(8)
            if len(hdr) < 8:
                return
            fcc, size = hdr[:4], struct.unpack('<I', hdr[4:])[0]
            body = p + 8
            if fcc == b'LIST':
                kind = f.read(4)
                if kind == b'movi':
                    info.setdefault("movi", (body + 4, body + size))
                    return True
                if walk(body + 4, body + size):
                    return True
            elif fcc == b'avih':
                v = struct.unpack('<10I', f.read(40))
                info.update(usec=v[0], frames_avih=v[4])
            elif fcc == b'strh':
                d = f.read(56)
                info["_strh"] = d
                nstreams[0] += 1
            elif fcc == b'strf':
                d = info.pop("_strh", None)
                if d is not None and d[:4] == b'vids' and info["stream"] is None:
                    scale, rate, _, length = struct.unpack_from('<4I', d, 20)
                    _, w, h, _, bits, comp = struct.unpack('<IiiHH4s', f.read(20))
                    info.update(stream=nstreams[0] - 1, width=w, height=abs(h), top_down=h < 0, bits=bits, codec=comp,
                                fps=(rate / scale) if scale else 0.0, frames_strh=length, handler=d[4:8])
            elif fcc == b'dmlh':
                info["frames_dmlh"] = struct.unpack('<I', f.read(4))[0]
            p = body + size + (size & 1)
        return False

    walk(12, riff_end)
    if info["stream"] is None:
        raise AviError("no video stream in the AVI headers")
    if not info.get("fps") and info.get("usec"):
        info["fps"] = 1e6 / info["usec"]
    info["frames"] = info["frames_dmlh"] or info["frames_strh"] or info["frames_avih"]
    info["riff_end"] = riff_end
    return info


def codec_name(info):
    c = info["codec"]
    return "BI_RGB" if c == b'\0\0\0\0' else c.decode('latin-1')


def probe(path):
    """-> dict(frames, fps, width, height, codec) from the headers alone."""
    with open(path, 'rb') as f:
        info = _read_headers(f)
    return {"frames": info["frames"], "fps": info["fps"], "width": info["width"], "height": info["height"],
            "codec": codec_name(info)}


class AviReader:
    """Frames of one AVI file's video stream, in order, as RGB [H,W,3] uint8."""

    def __init__(self, path):
        self.path = path
        self._f = open(path, 'rb')
        try:
            info = _read_headers(self._f)
            self.width, self.height, self.fps = info["width"], info["height"], info["fps"]
            self.frame_count, self.codec = info["frames"], codec_name(info)
            self._top_down = info["top_down"]
            if info["codec"] in (b'MJPG', b'mjpg'):
                self._mjpg = True
            elif info["codec"] in (b'\0\0\0\0', b'DIB ', b'RGB ') and info["bits"] == 24:
                self._mjpg = False
            else:
                raise AviError(f"{path}: unsupported codec {self.codec!r} ({info['bits']} bits per pixel); 24-bit "
                               f"uncompressed (BI_RGB) and MJPG are built")
            if "movi" not in info:
                raise AviError(f"{path}: no movi list")
        except Exception:
            self._f.close()
            raise
        self._ids = tuple(b'%02d' % info["stream"] + k for k in (b'db', b'dc'))
        self._size = self._f.seek(0, 2)
        self._stack = [info["movi"]]        # (next position, end) of the lists being walked, innermost last
        self._next_riff = info["riff_end"] + (info["riff_end"] & 1)
        self._last = None
        self.pos = 0

    # -- chunks --------------------------------------------------------------------------------------------------
    def _next_chunk(self):
        """-> (offset, size) of the next frame chunk's data, or None at the end of the file."""
        f = self._f
        while True:
            while self._stack:
                p, end = self._stack[-1]
                if p + 8 > min(end, self._size):
                    self._stack.pop()
                    continue
                f.seek(p)
                hdr = f.read(8)
                fcc, size = hdr[:4], struct.unpack('<I', hdr[4:])[0]
                self._stack[-1] = (p + 8 + size + (size & 1), end)
                if fcc == b'LIST':
                    self._stack.append((p + 12, p + 8 + size))       # 'rec ' groups hold the chunks one level down
                elif fcc in self._ids:
                    return p + 8, size
            # the next RIFF segment (OpenDML): RIFF size 'AVIX' LIST size 'movi'
            p = self._next_riff
            if p + 12 > self._size:
                return None
            f.seek(p)
            hdr = f.read(12)
            if hdr[:4] != b'RIFF':
                return None
            end = p + 8 + struct.unpack('<I', hdr[4:8])[0]
            self._next_riff = end + (end & 1)
            self._stack = [(p + 12, end)]

    def _decode(self, data):
        h, w = self.height, self.width
        if self._mjpg:
            Image = _pillow()
            if Image is None:
                raise AviError(f"{self.path}: MJPG frames need Pillow to be decoded, and it is not installed")
            import io
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            if rgb.shape != (h, w, 3):
                raise AviError(f"{self.path}: JPEG of {rgb.shape[1]}x{rgb.shape[0]} in a {w}x{h} stream")
            return rgb
        stride = dib_stride(w)
        if len(data) < stride * h:
            raise AviError(f"{self.path}: frame chunk of {len(data)} bytes, want {stride * h}")
        rows = np.frombuffer(data, np.uint8, stride * h).reshape(h, stride)[:, :3 * w].reshape(h, w, 3)
        if not self._top_down:
            rows = rows[::-1]
        return np.ascontiguousarray(rows[:, :, ::-1])

    # -- frames --------------------------------------------------------------------------------------------------
    def skip(self, n=1):
        """Pass over n frames without decoding them; -> how many there were."""
        k = 0
        while k < n and self._next_chunk() is not None:
            k += 1
        self.pos += k
        self._last = None
        return k

    def read_chunk(self):
        """-> the next frame chunk's bytes, undecoded (an MJPG stream's JPEG file), or None after the last one.  An
        empty chunk (b'') still means: repeat the frame before it."""
        at = self._next_chunk()
        if at is None:
            return None
        self._f.seek(at[0])
        data = self._f.read(at[1])
        self._last = None
        self.pos += 1
        return data

    def read(self):
        """-> the next frame, RGB [H,W,3] uint8, or None after the last one.  An empty chunk repeats the frame before it
        (a dropped frame)."""
        at = self._next_chunk()
        if at is None:
            return None
        off, size = at
        if size == 0 and self._last is not None:
            frame = self._last
        else:
            self._f.seek(off)
            frame = self._decode(self._f.read(size))
        self._last = frame
        self.pos += 1
        return frame

    def __iter__(self):
        while True:
            frame = self.read()
            if frame is None:
                return
            yield frame

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _read_frames_device(path, start, count, device):
    """read_frames with an MJPG stream's frames decoded on `device` (storage/device_mjpg.py DeviceMjpgDecoder); None:
    the file is not for it - no MJPG stream, or a first frame the device decoder does not take.  Later frames of that
    kind, and frames whose scan turns out damaged, go to Pillow one by one.  A frame without restart intervals (Pillow's,
    OpenCV's, ffmpeg's) is decoded on the device like any other, by the kernel jpeg_parse.decode_plan names; so are
    4:2:2, 4:4:4 and grey frames (jpeg_parse.DEVICE_SAMPLINGS), which a stream may mix."""
    import torch

    from .device_mjpg import DeviceMjpgDecoder
    from .jpeg_parse import DEVICE_SAMPLINGS, JpegUnsupported, parse

    def parsed(chunk):
        try:
            return parse(chunk, DEVICE_SAMPLINGS)
        except JpegUnsupported:
            return None

    with AviReader(path) as r:
        if not r._mjpg:
            return None
        r.skip(start)
        chunk = r.read_chunk()
        if not chunk or parsed(chunk) is None:
            return None
        h, w = r.height, r.width
        out, chunks, redo, repeats = [], {}, [], []
        dec = DeviceMjpgDecoder(device, on_error=lambda tag, e: redo.append(tag))
        slots = [torch.empty((h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
        events, waiting = [None] * len(slots), []       # (index in out, slot) on their way to the host, oldest first
        sent = 0                                         # frames given to the device: they alone take turns at the slots

        def collect(keep):
            while len(waiting) > keep:
                k, s = waiting.pop(0)
                events[s].synchronize()
                out[k] = slots[s].numpy().copy()

        with torch.cuda.device(device):
            while chunk is not None and (count is None or len(out) < count):
                k = len(out)
                info = parsed(chunk) if chunk else None
                if not chunk and out:
                    repeats.append(k)                    # an empty chunk repeats the frame before it, once that is final
                    out.append(None)
                elif info is None:
                    out.append(r._decode(chunk))
                elif (info.h, info.w) != (h, w):
                    raise AviError(f"{path}: JPEG of {info.w}x{info.h} in a {w}x{h} stream")
                else:
                    collect(len(slots) - 1)              # the slots in flight are the last ones used: the next is free
                    s = sent % len(slots)
                    sent += 1
                    chunks[k] = chunk
                    slots[s].copy_(dec.submit(chunk, info, tag=k), non_blocking=True)
                    events[s] = torch.cuda.Event()
                    events[s].record()
                    waiting.append((k, s))
                    out.append(None)
                    for j in [j for j in chunks if j != k and j not in redo]:
                        del chunks[j]                    # submit looked at the status of the frame before: it is whole
                chunk = r.read_chunk() if count is None or len(out) < count else None
            collect(0)
            dec.finish()
        for k in redo:                                   # a damaged scan: what Pillow makes of it, as without a device
            out[k] = r._decode(chunks[k])
        for k in repeats:
            out[k] = out[k - 1]
        return out


def read_frames(path, start=0, count=None, device=None):
    """-> list of RGB frames [start, start + count) of the file.  device: a GPU that decodes an MJPG stream's frames
    (the pictures are Pillow's byte for byte); None: everything on the host."""
    if device is not None and str(device).startswith('cuda'):
        frames = _read_frames_device(path, start, count, device)
        if frames is not None:
            return frames
    with AviReader(path) as r:
        r.skip(start)
        out = []
        while count is None or len(out) < count:
            frame = r.read()
            if frame is None:
                break
            out.append(frame)
    return out
