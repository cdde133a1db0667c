"""Flow-cache .npz members deflated and inflated on the device.

A member written here is an ordinary deflated zip member - np.load, zipfile and the reference's load_flow_npz read it -
whose stream is a stored block with the .npy header (made here) followed by the chunks vfml_deflate_huffman coded, and
whose local and central headers carry a private extra field, the CHUNK INDEX:

    <H id 0x4656> <H size>  <H version 1> <H 0> <I chunk_bytes> <I n_chunks> <I offset of chunk 0 in the stream> ...

Readers that do not know the field ignore it; read_member uses it to inflate the chunks in parallel on the device.

DeviceNpzWriter is the slot ring of storage/device_mjpg.py's encoder for these members: a field (and its LOD levels) is
coded behind the kernel that wrote it; its lengths are copied to pinned memory; one field later the host reads them and
copies exactly that many bytes; one field after that the members are handed to the sink.  The host never waits for the
field the GPU is working on and only the compressed bytes cross PCIe.
"""
import io
import struct
import zlib

import numpy as np
import torch

from .cache_manager import ZipMember

EXTRA_ID = 0x4656
VERSION = 1
CHUNK_BYTES = 32768
SLOTS = 3
_EXTRA_HEAD = struct.Struct('<HHHHII')


def build_extra(chunk_bytes, offsets):
    """The chunk index as a zip extra field; offsets count from the start of the member's stream."""
    body = _EXTRA_HEAD.pack(EXTRA_ID, 12 + 4 * len(offsets), VERSION, 0, chunk_bytes, len(offsets))
    return body + struct.pack(f'<{len(offsets)}I', *offsets)


def max_chunks():
    """Chunks an extra field (16-bit length, shared with nothing else here) can index."""
    return (0xFFFF - _EXTRA_HEAD.size) // 4


def parse_extra(extra):
    """(chunk_bytes, [offsets]) of the chunk index in a member's extra field; None when there is none or it is malformed."""
    pos = 0
    while pos + 4 <= len(extra):
        fid, size = struct.unpack_from('<HH', extra, pos)
        body = extra[pos + 4:pos + 4 + size]
        pos += 4 + size
        if fid != EXTRA_ID:
            continue
        if len(body) != size or size < 12:
            return None
        version, _, chunk_bytes, n = struct.unpack_from('<HHII', body, 0)
        if (version != VERSION or n < 1 or size != 12 + 4 * n or not 1024 <= chunk_bytes <= 32768
                or chunk_bytes & (chunk_bytes - 1)):
            return None
        offsets = list(struct.unpack_from(f'<{n}I', body, 12))
        if any(b < a for a, b in zip(offsets, offsets[1:])):
            return None
        return chunk_bytes, offsets
    return None


def npy_head(shape, dtype=np.float32):
    """The .npy header np.savez writes for a C-contiguous array of this shape."""
    head = io.BytesIO()
    np.lib.format.write_array_header_1_0(head, {'descr': np.lib.format.dtype_to_descr(np.dtype(dtype)),
                                                'fortran_order': False, 'shape': tuple(int(s) for s in shape)})
    return head.getvalue()


def head_block(head):
    """The stored block (BFINAL = 0) that carries the .npy header in front of the device's chunks."""
    n = len(head)
    return b'\x00' + struct.pack('<HH', n, n ^ 0xFFFF) + head


def assemble_member(name, shape, stream, crc, offsets, chunk_bytes, dtype=np.float32):
    """ZipMember of `<name>.npy` from the device's stream of the array's bytes (crc: continued from head_crc(shape))."""
    head = npy_head(shape, dtype)
    front = head_block(head)
    size = len(head) + int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return ZipMember(name, 8, crc, size, [front, stream], build_extra(chunk_bytes, [len(front) + o for o in offsets]))


def head_crc(shape, dtype=np.float32):
    return zlib.crc32(npy_head(shape, dtype))


def supported(tensor, chunk_bytes=CHUNK_BYTES):
    """Is this value coded on the device: a non-empty float32 device tensor of at most max_chunks() chunks."""
    from vfml import hip
    return (torch.is_tensor(tensor) and tensor.is_cuda and tensor.dtype == torch.float32 and tensor.numel() >= 1
            and hip.deflate_chunks(tensor.numel() * 4, chunk_bytes) <= max_chunks()
            and hip.deflate_capacity(tensor.numel() * 4, chunk_bytes) > 0)


def device_member(name, tensor, chunk_bytes=CHUNK_BYTES):
    """ZipMember of a float32 device tensor, coded now (synchronises: tests and tools; jobs use DeviceNpzWriter)."""
    from vfml import hip
    if not supported(tensor, chunk_bytes):
        raise ValueError("device_member: a non-empty float32 device tensor of at most 16000 chunks expected")
    t = tensor.contiguous()
    stream, cells = hip.deflate(t, chunk_bytes, head_crc(t.shape))
    data, crc, offsets = hip.deflate_stream(stream, cells)
    return assemble_member(name, tuple(t.shape), data, crc, offsets, chunk_bytes)


# ---- reader ---------------------------------------------------------------------------------------------------------
_LOCAL = struct.Struct('<4sHHHHHIIIHH')
_CENTRAL = struct.Struct('<4sHHHHHHIIIHHHHHII')
_END = struct.Struct('<4sHHHHIIH')


def find_member(data, name):
    """(method, crc, csize, size, extra, data offset) of member `<name>.npy` in the archive bytes; None if absent or the
    archive is not laid out plainly (zip64, a comment that hides the end record, encryption)."""
    want = (name + '.npy').encode()
    if len(data) < _END.size:
        return None
    sig, disk, cd_disk, n_here, n_all, cd_size, cd_off, comment = _END.unpack_from(data, len(data) - _END.size)
    if sig != b'PK\x05\x06' or comment or disk or cd_disk or cd_off + cd_size > len(data) or cd_off == 0xFFFFFFFF:
        return None
    pos = cd_off
    for _ in range(n_all):
        if pos + _CENTRAL.size > len(data):
            return None
        (sig, _, _, flags, method, _, _, crc, csize, size, nlen, elen, clen, _, _, _, local) = _CENTRAL.unpack_from(data, pos)
        if sig != b'PK\x01\x02':
            return None
        fname = bytes(data[pos + _CENTRAL.size:pos + _CENTRAL.size + nlen])
        extra = bytes(data[pos + _CENTRAL.size + nlen:pos + _CENTRAL.size + nlen + elen])
        pos += _CENTRAL.size + nlen + elen + clen
        if fname != want:
            continue
        if flags & 0x0009 or local + _LOCAL.size > len(data) or 0xFFFFFFFF in (csize, size, local):
            return None
        lsig, _, _, _, _, _, _, _, _, lnlen, lelen = _LOCAL.unpack_from(data, local)
        start = local + _LOCAL.size + lnlen + lelen
        if lsig != b'PK\x03\x04' or start + csize > len(data):
            return None
        return method, crc, csize, size, extra, start
    return None


def load_indexed(path, name):
    """The host half of read_member: the file is read and its chunk index checked against the member.  -> a plan for
    inflate_indexed, or None when the member has no (usable) index or is no float32 C-order array."""
    from vfml import hip
    with open(path, 'rb') as f:
        data = f.read()
    found = find_member(data, name)
    if found is None:
        return None
    method, crc, csize, size, extra, start = found
    index = parse_extra(extra)
    if index is None or method != 8 or csize < 5:
        return None
    chunk_bytes, offsets = index
    # the header block: stored, not final, LEN = the .npy header
    n_head, n_inv = struct.unpack_from('<HH', data, start + 1)
    if data[start] != 0 or n_head ^ n_inv != 0xFFFF or 5 + n_head > csize:
        return None
    head = data[start + 5:start + 5 + n_head]
    try:
        fp = io.BytesIO(head)
        if np.lib.format.read_magic(fp) != (1, 0):
            return None
        shape, fortran, dtype = np.lib.format.read_array_header_1_0(fp)
    except Exception:
        return None
    raw_bytes = size - n_head
    if (fortran or dtype != np.dtype('<f4') or fp.tell() != n_head or raw_bytes < 1
            or raw_bytes != int(np.prod(shape, dtype=np.int64)) * 4
            or len(offsets) != hip.deflate_chunks(raw_bytes, chunk_bytes) or offsets[0] != 5 + n_head
            or offsets[-1] > csize or raw_bytes > 0x7FFFFFFF or len(offsets) > 16000):
        return None
    return {"body": data[start + 5 + n_head:start + csize], "offsets": [o - offsets[0] for o in offsets],
            "chunk_bytes": chunk_bytes, "raw_bytes": raw_bytes, "crc_init": zlib.crc32(head), "crc": crc, "shape": shape}


def inflate_indexed(plan, device):
    """The device half: upload the member's bytes and inflate them -> (float32 device tensor, cells, crc of the archive);
    hip.inflate_check(cells, crc) is the caller's (it synchronises)."""
    from vfml import hip
    body = torch.frombuffer(bytearray(plan["body"]), dtype=torch.uint8).to(device)
    raw, cells = hip.inflate(body, plan["offsets"], plan["chunk_bytes"], plan["raw_bytes"], plan["crc_init"])
    return raw.view(torch.float32).view(*plan["shape"]), cells, plan["crc"]


def read_member(path, name, device):
    """Member `<name>.npy` of the .npz at `path` as a device tensor, inflated on `device` through its chunk index.
    None when the member has no (usable) index - written by zlib, np.savez_compressed or the reference - or is no
    float32 C-order array: the caller falls back to np.load.  A damaged stream or a CRC mismatch raises."""
    from vfml import hip
    plan = load_indexed(path, name)
    if plan is None:
        return None
    out, cells, crc = inflate_indexed(plan, device)
    hip.inflate_check(cells, crc)
    return out


# ---- writer ---------------------------------------------------------------------------------------------------------
class DeviceNpzWriter:
    """sink(key, [(ZipMember named 'flow', shape), ...]) is called, two submits behind, for every submit(key, tensors):
    tensors = float32 device tensors written on the current stream (a field and its LOD levels) that stay unchanged
    until the kernels queued here have run (stream order: a later kernel on the same stream may overwrite them)."""

    def __init__(self, device, sink, chunk_bytes=CHUNK_BYTES):
        from vfml import hip
        self._hip, self._device, self._sink, self._chunk = hip, torch.device(device), sink, int(chunk_bytes)
        self._slots = [None] * SLOTS          # per slot: dict of the submit in flight
        self._frames = 0
        self._encoded = self._copying = None

    def _buffers(self, slot, shapes):
        """Device streams, pinned cells and pinned bytes of a slot, made once per geometry."""
        if slot is not None and slot["shapes"] == shapes:
            return slot
        dev, hip = self._device, self._hip
        sizes = [int(np.prod(s)) * 4 for s in shapes]
        return {
            "shapes": shapes,
            "stream": [torch.empty(hip.deflate_capacity(n, self._chunk), dtype=torch.uint8, device=dev) for n in sizes],
            "cells": [torch.empty(2 + hip.deflate_chunks(n, self._chunk), dtype=torch.int32).pin_memory() for n in sizes],
            "host": [torch.empty(hip.deflate_capacity(n, self._chunk), dtype=torch.uint8).pin_memory() for n in sizes],
            "crc0": [head_crc(s) for s in shapes],
        }

    def submit(self, key, tensors):
        shapes = [tuple(int(v) for v in t.shape) for t in tensors]
        for t in tensors:
            if not (supported(t, self._chunk) and t.is_contiguous()):
                raise ValueError("DeviceNpzWriter: contiguous non-empty float32 device tensors expected")
        s = self._frames % SLOTS
        self._frames += 1
        slot = self._slots[s] = self._buffers(self._slots[s], shapes)
        slot["key"] = key
        for i, t in enumerate(tensors):
            _, cells = self._hip.deflate(t, self._chunk, slot["crc0"][i], out=slot["stream"][i])
            slot["cells"][i].copy_(cells, non_blocking=True)
        slot["cells_event"] = torch.cuda.Event()
        slot["cells_event"].record()
        self._advance()
        self._encoded = s

    def _advance(self):
        if self._copying is not None:
            self._hand_over(self._copying)
        self._copying, self._encoded = self._encoded, None
        if self._copying is not None:
            self._fetch(self._copying)

    def _fetch(self, s):
        slot = self._slots[s]
        slot["cells_event"].synchronize()
        slot["meta"] = []
        for i, cells in enumerate(slot["cells"]):
            host = [int(v) & 0xFFFFFFFF for v in cells.tolist()]
            n = host[0]
            if n > slot["stream"][i].numel():
                raise RuntimeError(f"DeviceNpzWriter: the stream needs {n} bytes, its buffer holds {slot['stream'][i].numel()}")
            slot["host"][i][:n].copy_(slot["stream"][i][:n], non_blocking=True)
            slot["meta"].append((n, host[1], host[2:]))
        slot["copy_event"] = torch.cuda.Event()
        slot["copy_event"].record()

    def _hand_over(self, s):
        slot = self._slots[s]
        slot["copy_event"].synchronize()
        members = []
        for i, (n, crc, offsets) in enumerate(slot["meta"]):
            data = slot["host"][i].numpy()[:n].tobytes()      # the pinned slot is reused; the sink's threads keep these
            members.append((assemble_member('flow', slot["shapes"][i], data, crc, offsets, self._chunk), slot["shapes"][i]))
        self._sink(slot["key"], members)

    def finish(self):
        """Hand over the submits still on their way."""
        self._advance()
        self._advance()
