"""AVI writer in pure Python: the container of flow_processor's output video (reference: cv2.VideoWriter, MJPG or
uncompressed, flow_processor.py:876-897).  No OpenCV.

* MJPG: each frame a baseline JPEG at quality 95 (4:2:0 unless `sampling` names 4:2:2 or 4:4:4), encoded with Pillow on a
  thread pool (frames stay in order).  Without
  Pillow the writer says so and writes uncompressed frames instead.  `encoder='external'`: the caller hands in finished
  JPEG files (`write_encoded`: the device encoder's frames, vfml_jpeg_encode_rgb) - no Pillow, no pool.
* uncompressed: 24-bit BI_RGB DIB frames - BGR, bottom-up rows, each row padded to 4 bytes.
* Files larger than one RIFF segment are OpenDML (AVI 2.0): `AVIX` segments, an `indx` super index pointing at one
  `ix00` standard index per segment, the total frame count in `odml/dmlh`, and a legacy `idx1` for the first segment.
  `segment_bytes` (default 1 GiB) bounds each RIFF; tests lower it to force several segments.

`write(frame)` takes a BGR [H,W,3] uint8 frame, as cv2.VideoWriter does.  `write_payload(buf)` takes a frame already
in the chunk's layout (what vfml_compose_frame writes): the DIB bytes, or for MJPG an RGB top-down [H,W,3] image.
"""
import struct
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

AVIF_HASINDEX, AVIF_ISINTERLEAVED = 0x10, 0x100
AVIIF_KEYFRAME = 0x10
SUPER_INDEX_ENTRIES = 256          # room in `indx` for this many RIFF segments (256 GiB at the default segment size)
JPEG_QUALITY = 95


def dib_stride(width):
    """Bytes per row of a 24-bit DIB: 3 x width rounded up to 4."""
    return (3 * width + 3) // 4 * 4


def bgr_to_dib(frame):
    """BGR [H,W,3] uint8 (top-down) -> the bytes of a bottom-up 24-bit DIB with 4-byte row padding."""
    h, w = frame.shape[:2]
    stride = dib_stride(w)
    out = np.zeros((h, stride), np.uint8)
    out[:, :3 * w] = np.ascontiguousarray(frame[::-1]).reshape(h, 3 * w)
    return out.tobytes()


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


# sampling -> Pillow's subsampling= of the same kind of file (None: its default at this quality, 4:2:0, as always written)
PILLOW_SUBSAMPLING = {"4:2:0": None, "4:2:2": 1, "4:4:4": 0}


def _jpeg(rgb, subsampling=None):
    import io
    buf = io.BytesIO()
    kw = {} if subsampling is None else {"subsampling": subsampling}
    _pillow().fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, format="JPEG", quality=JPEG_QUALITY, **kw)
    return buf.getvalue()


class AviWriter:
    """cv2.VideoWriter-like AVI writer (one video stream).  `fourcc`: 'MJPG' or 0 / None (uncompressed).
    `encoder`: who makes the JPEGs of an MJPG file - 'pillow' (write / write_payload, on the writer's pool) or
    'external' (the caller, through write_encoded).  `sampling`: '4:2:0', '4:2:2' or '4:4:4', what the 'pillow' encoder
    writes (an 'external' caller's files are its own, the name is only kept)."""

    def __init__(self, path, fourcc, fps, size, segment_bytes=1 << 30, workers=None, depth=None, log=print,
                 encoder='pillow', sampling='4:2:0'):
        self.path, self.fps = path, float(fps)
        self.width, self.height = (int(v) for v in size)
        self.mjpg = fourcc not in (0, None)
        if self.mjpg and fourcc != 'MJPG':
            raise ValueError(f"AviWriter: fourcc {fourcc!r}; 'MJPG' or 0 (uncompressed) are built")
        if encoder not in ('pillow', 'external'):
            raise ValueError(f"AviWriter: encoder {encoder!r}; 'pillow' or 'external'")
        if sampling not in PILLOW_SUBSAMPLING:
            raise ValueError(f"AviWriter: sampling {sampling!r}; {', '.join(PILLOW_SUBSAMPLING)} are built")
        self.sampling = sampling
        self.external = self.mjpg and encoder == 'external'
        if self.mjpg and not self.external and _pillow() is None:
            log("Warning: Pillow is not installed; writing uncompressed frames instead of MJPG")
            self.mjpg = False
        self.ckid = b'00dc' if self.mjpg else b'00db'
        self.frame_bytes = dib_stride(self.width) * self.height
        self.segment_bytes = int(segment_bytes)
        self._f = open(path, 'wb')
        self._segments = []           # (ix00 offset, ix00 size, frames) of closed segments
        self._idx1 = []               # (offset from 'movi' fourcc, size) of the first segment's chunks
        self._seg = []                # (absolute data offset, size) of the current segment's chunks
        self.frames = 0
        self._max_chunk = 0
        if self.mjpg and not self.external:
            if workers is None:
                from vfml.dist import host_cpu_share
                workers = host_cpu_share()
            self._pool = ThreadPoolExecutor(max_workers=max(1, min(16, workers)), thread_name_prefix="avi-jpeg")
            self._pending = deque()
            self._depth = depth or 2 * self._pool._max_workers     # JPEGs in flight at most
        self._write_headers()
        self._open_segment(first=True)

    # -- layout ------------------------------------------------------------------------------------------------
    def _write_headers(self):
        f = self._f
        f.write(b'RIFF\0\0\0\0AVI ')
        hdrl = f.tell()
        f.write(b'LIST\0\0\0\0hdrl')
        rate = Fraction(self.fps).limit_denominator(1001000)
        self._rate, self._scale = rate.numerator, rate.denominator
        self._avih = f.tell() + 8
        f.write(b'avih' + struct.pack('<I', 56) + bytes(56))
        f.write(b'LIST' + struct.pack('<I', 4 + 8 + 56 + 8 + 40 + 8 + 24 + 16 * SUPER_INDEX_ENTRIES) + b'strl')
        self._strh = f.tell() + 8
        f.write(b'strh' + struct.pack('<I', 56) + bytes(56))
        comp = b'MJPG' if self.mjpg else b'\0\0\0\0'
        f.write(b'strf' + struct.pack('<I', 40) + struct.pack(
            '<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, comp,
            self.frame_bytes if not self.mjpg else 3 * self.width * self.height, 0, 0, 0, 0))
        self._indx = f.tell()
        f.write(b'indx' + struct.pack('<I', 24 + 16 * SUPER_INDEX_ENTRIES) + bytes(24 + 16 * SUPER_INDEX_ENTRIES))
        f.write(b'LIST' + struct.pack('<I', 4 + 8 + 248) + b'odml')
        self._dmlh = f.tell() + 8
        f.write(b'dmlh' + struct.pack('<I', 248) + bytes(248))
        self._patch_size(hdrl)
        self._patch_main_headers()

    def _patch_size(self, at, end=None):
        end = self._f.tell() if end is None else end
        here = self._f.tell()
        self._f.seek(at + 4)
        self._f.write(struct.pack('<I', end - at - 8))
        self._f.seek(here)

    def _patch_main_headers(self):
        f, here = self._f, self._f.tell()
        first = self._segments[0][2] if self._segments else self.frames
        usec = int(round(1e6 * self._scale / self._rate))
        f.seek(self._avih)
        f.write(struct.pack('<IIIIIIIIII', usec, min(int(self._max_chunk * self.fps), 0xFFFFFFFF), 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED,
                            first, 0, 1, self._max_chunk, self.width, self.height) + bytes(16))
        f.seek(self._strh)
        f.write(b'vids' + (b'MJPG' if self.mjpg else b'DIB ') + struct.pack(
            '<IHHIIIIIIIIhhhh', 0, 0, 0, 0, self._scale, self._rate, 0, self.frames, self._max_chunk, 0xFFFFFFFF, 0,
            0, 0, self.width, self.height))
        f.seek(self._dmlh)
        f.write(struct.pack('<I', self.frames))
        f.seek(self._indx + 8)
        f.write(struct.pack('<HBBI4sIII', 4, 0, 0, len(self._segments), self.ckid, 0, 0, 0))
        for off, size, n in self._segments:
            f.write(struct.pack('<QII', off, size, n))
        f.seek(here)

    def _open_segment(self, first=False):
        f = self._f
        if not first:
            self._riff = f.tell()
            f.write(b'RIFF\0\0\0\0AVIX')
        else:
            self._riff = 0
        self._movi = f.tell()
        f.write(b'LIST\0\0\0\0movi')
        self._seg = []

    def _close_segment(self):
        f = self._f
        if self._seg:
            base = self._seg[0][0]
            ix = f.tell()
            f.write(b'ix00' + struct.pack('<I', 24 + 8 * len(self._seg)))
            f.write(struct.pack('<HBBI4sQI', 2, 0, 1, len(self._seg), self.ckid, base, 0))
            for off, size in self._seg:
                f.write(struct.pack('<II', off - base, size))
            self._segments.append((ix, 24 + 8 + 8 * len(self._seg), len(self._seg)))
        self._patch_size(self._movi)
        if self._riff == 0:
            f.write(b'idx1' + struct.pack('<I', 16 * len(self._idx1)))
            for off, size in self._idx1:
                f.write(self.ckid + struct.pack('<III', AVIIF_KEYFRAME, off, size))
        self._patch_size(self._riff)

    def _chunk(self, data):
        f = self._f
        n = len(data)
        need = 8 + n + (n & 1) + 32 + 8 * (len(self._seg) + 1) + (16 * (len(self._idx1) + 1) if self._riff == 0 else 0)
        if self._seg and f.tell() + need - self._riff > self.segment_bytes:
            self._close_segment()
            self._open_segment()
        at = f.tell()
        f.write(self.ckid + struct.pack('<I', n))
        f.write(data)
        if n & 1:
            f.write(b'\0')
        self._seg.append((at + 8, n))
        if self._riff == 0:
            self._idx1.append((at - (self._movi + 8), n))
        self.frames += 1
        self._max_chunk = max(self._max_chunk, n)

    # -- frames ------------------------------------------------------------------------------------------------
    def isOpened(self):
        return self._f is not None

    def write(self, frame):
        """BGR [H,W,3] uint8, top-down (cv2.VideoWriter.write)."""
        frame = np.asarray(frame)
        if frame.shape != (self.height, self.width, 3) or frame.dtype != np.uint8:
            raise ValueError(f"AviWriter: frame {frame.dtype} {frame.shape}, want uint8 {(self.height, self.width, 3)}")
        if self.mjpg:
            self.write_payload(frame[:, :, ::-1])
        else:
            self._chunk(bgr_to_dib(frame))

    def write_payload(self, buf):
        """A frame in the chunk's layout: uncompressed - the DIB bytes (height x dib_stride(width)); MJPG - an RGB
        [H,W,3] uint8 image (encoded on the pool; the buffer must stay unchanged until `drain` says it was used)."""
        if self.external:
            raise ValueError("AviWriter: encoder='external' takes finished JPEGs through write_encoded")
        if not self.mjpg:
            data = np.asarray(buf).reshape(-1)
            if data.size != self.frame_bytes:
                raise ValueError(f"AviWriter: payload of {data.size} bytes, want {self.frame_bytes}")
            self._chunk(data.tobytes())
            return
        self._pending.append(self._pool.submit(_jpeg, buf, PILLOW_SUBSAMPLING[self.sampling]))
        while len(self._pending) > self._depth:
            self._chunk(self._pending.popleft().result())

    def write_encoded(self, data):
        """One finished JPEG file (bytes-like) as the next frame of an encoder='external' writer."""
        if not self.external:
            raise ValueError("AviWriter: write_encoded needs an MJPG writer with encoder='external'")
        self._chunk(data)

    def drain(self, keep=0):
        """Write encoded frames until at most `keep` are still in flight."""
        if self.mjpg and not self.external:
            while len(self._pending) > keep:
                self._chunk(self._pending.popleft().result())

    def in_flight(self):
        return len(self._pending) if self.mjpg and not self.external else 0

    def in_flight_limit(self):
        """Most payload buffers the writer may still hold after write_payload returns."""
        return self._depth if self.mjpg and not self.external else 0

    def release(self):
        if self._f is None:
            return
        self.drain()
        if self.mjpg and not self.external:
            self._pool.shutdown()
        self._close_segment()
        self._patch_main_headers()
        self._f.close()
        self._f = None
