"""avi_reader.read_frames(path, device=gpu) and DeviceMjpgDecoder on MJPG streams whose frames do not all take the same
way: device-decoded frames with Pillow-decoded ones (no restart intervals) and repeats between them, a frame whose scan
is damaged, and a file that outgrows its pinned slot.  Every list equals read_frames(path) - Pillow - frame for frame."""
import numpy as np
import pytest
import torch

import jpeg_oracle as jo
from storage import jpeg_parse as jp
from test_jpeg_decode_cpu import PICTURES, damaged_files, own_file, pillow_decode, pillow_file

pytestmark = pytest.mark.gpu


def _avi(path, files, size):
    from storage.avi_writer import AviWriter
    wr = AviWriter(str(path), 'MJPG', 25.0, size, encoder='external')
    for f in files:
        wr.write_encoded(f)
    wr.release()
    return str(path)


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), f"frame {k}"


def test_pillow_frames_and_repeats_between_device_frames(gpu, tmp_path):
    """D D P D D D P P D - D D: more device frames than pinned slots on either side of a Pillow frame, so a slot is used
    again while frames before the Pillow frame are still on their way to the host."""
    from storage import avi_reader
    base = PICTURES["random45x67"]
    kinds = "DDPDDDPPD-DD"
    files = []
    for k, kind in enumerate(kinds):
        img = np.roll(base, 5 * k + 1, axis=1)                      # every frame another picture
        files.append(b'' if kind == '-' else jo.encode(img, 95) if kind == 'D' else pillow_file(img, quality=90))
    assert [jp.parse(f).restart_interval > 0 for f in files if f] == [k == 'D' for k in kinds if k != '-']
    path = _avi(tmp_path / "mixed.avi", files, (67, 45))
    want = avi_reader.read_frames(path)
    assert len(want) == len(kinds) and len({w.tobytes() for w in want}) == len(kinds) - 1
    _same(avi_reader.read_frames(path, device=gpu), want)
    _same(avi_reader.read_frames(path, 1, 7, device=gpu), want[1:8])
    _same(avi_reader.read_frames(path, 3, device=gpu), want[3:])
    # a stream that opens with a Pillow frame is the host's as a whole
    _same(avi_reader.read_frames(path, 2, 4, device=gpu), want[2:6])


def test_a_damaged_frame_and_its_repeat_are_the_hosts(gpu, tmp_path):
    """The status of a frame is known one frame late: the damaged frame and the empty chunk that repeats it both end as
    what the host path makes of that file."""
    from storage import avi_reader
    good = [own_file(name, 95) for name in ("noise150x40", "checker150x40", "frequency150x40")]
    bad = damaged_files()["zeros_150x40"]
    files = [good[0], bad, b'', good[1], damaged_files()["rst_removed_150x40"], good[2]]
    path = _avi(tmp_path / "damaged.avi", files, (40, 150))
    want = avi_reader.read_frames(path)
    assert np.array_equal(want[1], want[2])
    _same(avi_reader.read_frames(path, device=gpu), want)


def test_a_file_larger_than_its_pinned_slot(gpu):
    """Two slots of 64 KiB: the large file grows its slot, the small ones before and behind it are not disturbed."""
    from storage.device_mjpg import DeviceMjpgDecoder
    rng = np.random.default_rng(5)
    small = [own_file("random45x67", 95), own_file("noise150x40", 95)]
    large = jo.encode(rng.integers(0, 256, (208, 240, 3), dtype=np.uint8), 100)
    assert len(large) > 1 << 16 > max(len(f) for f in small)
    failed = []
    dec = DeviceMjpgDecoder(gpu, slots=2, on_error=lambda tag, e: failed.append(tag))
    order = [small[0], large, small[1], large, small[0]]
    with torch.cuda.device(gpu):
        got = [dec.submit(f, tag=k).cpu().numpy() for k, f in enumerate(order)]
        dec.finish()
    assert not failed
    for g, f in zip(got, order):
        assert np.array_equal(g, pillow_decode(f))
