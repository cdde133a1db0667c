"""MJPG frames encoded and decoded on the device.

DeviceMjpgEncoder: MJPG frames encoded on the device (vfml_jpeg_encode_rgb_sampled; 4:2:0 unless
the caller names 4:2:2 or 4:4:4) on their way into an AviWriter(encoder='external'): the composed frame never leaves the
device uncompressed, only its scan comes back.

Per frame, all on the caller's current stream: the encoder runs behind the kernel that wrote the picture; the length
cell is copied to pinned memory; one frame later the host reads it and copies exactly that many bytes into a pinned slot
that already holds the file header; one frame after that the slot - header, scan, EOI - is appended to the AVI.  The
host therefore never waits for the frame the GPU is working on, and never copies the worst-case capacity.

DeviceMjpgDecoder is its mirror for the MJPG frames that are read (vfml_jpeg_decode_rgb_sampled, DESIGN.md section 13;
4:2:0, 4:2:2, 4:4:4 and grey frames, in any mix): the
file's bytes go up through a small ring of pinned slots, the picture is decoded where it is used, and the status cell of
a frame comes back and is looked at while the next frame is on its way.
"""
import numpy as np
import torch

from .avi_writer import JPEG_QUALITY

SLOTS = 3      # a slot is encoded into at frame i, fetched at i + 1, written at i + 2 and free again at i + 3


class DeviceMjpgEncoder:
    def __init__(self, writer, height, width, device, quality=JPEG_QUALITY, sampling="4:2:0"):
        from vfml import hip
        from . import jpeg_tables
        if not getattr(writer, "external", False):
            raise ValueError("DeviceMjpgEncoder: the writer must be an MJPG AviWriter with encoder='external'")
        if (writer.height, writer.width) != (height, width):
            raise ValueError(f"DeviceMjpgEncoder: frames of {width}x{height} for a {writer.width}x{writer.height} writer")
        self._hip, self._writer, self._quality, self._sampling = hip, writer, int(quality), sampling
        self._header = hip.jpeg_header(height, width, self._quality, sampling)
        capacity = hip.jpeg_scan_capacity(height, width, sampling)
        self._scan = [torch.empty(capacity, dtype=torch.uint8, device=device) for _ in range(SLOTS)]
        self._length = [torch.empty(1, dtype=torch.int32).pin_memory() for _ in range(SLOTS)]
        # a first guess of a third of a byte per sample, i.e. per coefficient of the sampling's blocks; _fetch grows it
        rows, cols = jpeg_tables.mcu_grid(height, width, sampling)
        blocks = rows * cols * jpeg_tables.BLOCKS_PER_MCU[sampling]
        self._host = [self._slot(max(4096, blocks * 64 // 3)) for _ in range(SLOTS)]
        self._bytes = [0] * SLOTS
        self._length_event = [None] * SLOTS
        self._copy_event = [None] * SLOTS
        self._encoded = self._copying = None      # slots whose length / whose scan is on its way to the host
        self._frames = 0

    def _slot(self, scan_bytes):
        """Pinned bytes for a file with a scan of `scan_bytes`: header in place, room for the scan and EOI."""
        n = len(self._header)
        t = torch.empty(n + scan_bytes + 2, dtype=torch.uint8).pin_memory()
        t[:n] = torch.frombuffer(bytearray(self._header), dtype=torch.uint8)
        return t

    def submit(self, rgb):
        """rgb: the frame, uint8 device tensor [H,W,3] with contiguous rows, written on the current stream."""
        s = self._frames % SLOTS
        self._frames += 1
        _, length = self._hip.jpeg_encode(rgb, self._quality, out=self._scan[s], sampling=self._sampling)
        self._length[s].copy_(length, non_blocking=True)
        self._length_event[s] = torch.cuda.Event()
        self._length_event[s].record()
        self._advance()
        self._encoded = s

    def _advance(self):
        if self._copying is not None:
            self._write(self._copying)
        self._copying = self._encoded
        self._encoded = None
        if self._copying is not None:
            self._fetch(self._copying)

    def _fetch(self, s):
        self._length_event[s].synchronize()
        n = int(self._length[s][0]) & 0xFFFFFFFF
        if n > self._scan[s].numel():
            raise RuntimeError(f"DeviceMjpgEncoder: the scan needs {n} bytes, its buffer holds {self._scan[s].numel()}")
        at = len(self._header)
        if at + n + 2 > self._host[s].numel():      # a frame that outgrows its pinned slot grows the slot
            self._host[s] = self._slot(n + n // 4)
        self._host[s][at:at + n].copy_(self._scan[s][:n], non_blocking=True)
        self._copy_event[s] = torch.cuda.Event()
        self._copy_event[s].record()
        self._bytes[s] = n

    def _write(self, s):
        self._copy_event[s].synchronize()
        buf = self._host[s].numpy()
        end = len(self._header) + self._bytes[s]
        buf[end], buf[end + 1] = 0xFF, 0xD9         # EOI
        self._writer.write_encoded(buf[:end + 2])

    def finish(self):
        """Write the frames still on their way."""
        self._advance()
        self._advance()


class DeviceMjpgDecoder:
    """JPEG files decoded on `device`, in order, on the caller's current stream.  submit() never waits for the frame it
    starts; a damaged scan is reported one submit later (or by finish) through `on_error(tag, RuntimeError)` - raised
    when there is no such callback.  stats: frames submitted per kernel, {'interval': n, 'sync': n}."""

    def __init__(self, device, slots=SLOTS, on_error=None):
        from vfml import hip
        self._hip, self._device, self._on_error = hip, torch.device(device), on_error
        self._host = [torch.empty(1 << 16, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._status = [torch.empty(1, dtype=torch.int32).pin_memory() for _ in range(slots)]
        self._event = [None] * slots
        self._tag = [None] * slots
        self._frames = 0
        self._unchecked = None                    # the slot whose status has not been looked at
        self.stats = {"interval": 0, "sync": 0}

    def submit(self, data, info=None, rows=None, out=None, tag=None, plan=None, subseq_bytes=None):
        """data: the file's bytes (bytes-like); info: storage.jpeg_parse.parse(data) when the caller has it.  -> the
        picture (rows y0 <= y < y1 of it), a uint8 device tensor, valid in stream order.  plan, subseq_bytes: the
        kernel, as hip.jpeg_decode takes them (None: by the file's restart interval; subseq_bytes is then left unused by a
        file that the rule gives to 'interval')."""
        from storage import jpeg_parse
        if info is None:
            info = jpeg_parse.parse(data, jpeg_parse.DEVICE_SAMPLINGS)
        s = self._frames % len(self._host)
        self._frames += 1
        if self._event[s] is not None:
            self._event[s].synchronize()          # the slot's last upload and decode have run
            if self._unchecked == s:
                self._check(s)
        n = len(data)
        if n > self._host[s].numel():             # a file that outgrows its pinned slot grows the slot
            self._host[s] = torch.empty(n + n // 4, dtype=torch.uint8).pin_memory()
        self._host[s].numpy()[:n] = np.frombuffer(data, np.uint8)
        if plan is None:
            plan = jpeg_parse.decode_plan(info)
            if plan == "interval":
                subseq_bytes = None               # as hip.jpeg_decode(plan=None) does: it raises for a named 'interval' alone
        rgb, status = self._hip.jpeg_decode(self._host[s][:n], rows=rows, out=out, device=self._device, info=info,
                                            plan=plan, subseq_bytes=subseq_bytes)
        self.stats[plan] += 1
        self._status[s].copy_(status, non_blocking=True)
        self._event[s] = torch.cuda.Event()
        self._event[s].record()
        self._tag[s] = tag
        previous, self._unchecked = self._unchecked, s
        if previous is not None:
            self._event[previous].synchronize()
            self._check(previous)
        return rgb

    def _check(self, s):
        try:
            self._hip.jpeg_decode_check(int(self._status[s][0]))
        except RuntimeError as e:
            if self._on_error is None:
                raise
            self._on_error(self._tag[s], e)
        finally:
            if self._unchecked == s:
                self._unchecked = None

    def finish(self):
        """Wait for the frames still on their way and look at their status."""
        if self._unchecked is not None:
            s = self._unchecked
            self._event[s].synchronize()
            self._check(s)
