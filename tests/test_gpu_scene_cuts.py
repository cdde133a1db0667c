"""Scene cuts on the GPU: vfml_scene_distances against the numpy oracle bit for bit, the feeder's
scores, and jobs with cuts on - MOF, BOF, MemFlow, tiles, the render stage - against each scene run as a clip of its own."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import scene_cut_oracle as so

pytestmark = pytest.mark.gpu

CUTS = (so.TH, so.R)
_CLIPS = {}


def _graded(h, w):
    if (h, w) not in _CLIPS:
        _CLIPS[(h, w)] = so.graded_clip(h, w)
    return _CLIPS[(h, w)]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check(frames_np, prev=None, skip=0):
    """frames_np [n,H,W,3] through the kernel - as frames skip.. of a larger clip, so that the base address takes every
    alignment an odd frame size gives - against the oracle, signatures and distances bit for bit."""
    from vfml import hip
    n = frames_np.shape[0]
    big = torch.zeros((n + skip,) + frames_np.shape[1:], dtype=torch.uint8, device="cuda")
    big[skip:] = torch.from_numpy(frames_np).cuda()
    prev_sig = None if prev is None else torch.from_numpy(so.signature(prev).reshape(-1).view(np.int32)).cuda()
    sig, dist = hip.scene_distances(big[skip:], prev_sig=prev_sig)
    want_sig, want_dist = so.distances(list(frames_np), None if prev is None else so.signature(prev))
    assert np.array_equal(_u32(sig).reshape(n, 16, 64), want_sig)
    assert np.array_equal(_u32(dist), want_dist)
    assert int(want_sig[0].sum()) == frames_np.shape[1] * frames_np.shape[2]
    return want_dist


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (4, 4), (30, 46), (64, 96), (135, 240)])
def test_kernel_equals_the_oracle(gpu, h, w, n, with_prev):
    rng = np.random.default_rng(1000 * h + 10 * n + with_prev)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    prev = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if with_prev else None
    for skip in (0, 1, 2, 3):                # h * w * 3 odd: four alignments of the first frame
        d = _check(frames, prev, skip)
        assert prev is not None or d[0] == 0


def test_kernel_on_textured_frames(gpu):
    """Smooth pictures take the four-equal-bins path of the group loop that random bytes almost never take."""
    frames = np.stack(_graded(30, 46)[3:7])
    _check(frames, _graded(30, 46)[2], skip=1)
    _check(np.stack(_graded(128, 192)[4:6]))


def test_one_colour_and_random_frames(gpu):
    flat = np.empty((2, 135, 240, 3), dtype=np.uint8)
    flat[0] = (200, 100, 50)
    flat[1] = (10, 20, 30)
    d = _check(flat)
    assert d[1] == 2 * 135 * 240                        # every pixel changed its bin: the largest distance there is
    sig = so.signature(flat[0])
    assert np.count_nonzero(sig) == 16 and sig.sum() == 135 * 240      # one bin per cell holds the cell
    _check(flat[:1])
    rng = np.random.default_rng(5)
    _check(rng.integers(0, 256, (3, 67, 129, 3), dtype=np.uint8), skip=1)


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
def test_a_pair_at_full_size(gpu, h, w):
    """1080p: two textured frames; 2160 x 3840: a frame of one colour against random bytes, for the sums (d near 2 H W)."""
    g = torch.Generator(device="cuda").manual_seed(h)
    pair = torch.randint(0, 256, (2, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    if h == 1080:
        pair = (pair.float() * torch.linspace(0.2, 1.0, w, device="cuda").view(1, 1, w, 1)).to(torch.uint8)
    else:
        pair[0] = 128
    d = _check(pair.cpu().numpy())
    assert d[1] > (0 if h == 1080 else h * w)          # (two draws of one distribution are close; flat against noise is not)


def test_refusals_launch_nothing(gpu):
    from vfml import hip
    L = hip.lib()
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    sig = torch.full((1, 1024), 77, dtype=torch.int32, device="cuda")
    dist = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, word in (((None, 1, 8, 8, None, p(sig), p(dist), s), b"null"),
                       ((p(frames), 1, 8, 8, None, None, p(dist), s), b"null"),
                       ((p(frames), 1, 8, 8, None, p(sig), None, s), b"null"),
                       ((p(frames), 0, 8, 8, None, p(sig), p(dist), s), b"frames"),
                       ((p(frames), 1, 0, 8, None, p(sig), p(dist), s), b"empty"),
                       ((p(frames), 1, 8, 0, None, p(sig), p(dist), s), b"empty"),
                       ((p(frames), 1, 65536, 32768, None, p(sig), p(dist), s), b"2^31")):
        assert L.vfml_scene_distances(*args) != 0
        assert word in L.vfml_last_error(), (word, L.vfml_last_error())
    torch.cuda.synchronize()
    assert bool((sig == 77).all()) and int(dist[0]) == 77
    with pytest.raises(ValueError):
        hip.scene_distances(frames.cpu())
    with pytest.raises(ValueError):
        hip.scene_distances(frames, prev_sig=torch.zeros(1023, dtype=torch.int32, device="cuda"))
    assert hip.lib().vfml_abi_version() == 27


# ------------------------------------------------------------------------------------------------------------ the feeder
@pytest.mark.parametrize("src", [(128, 192), (192, 288), (256, 384)])
def test_feeder_finds_the_cuts_of_the_clip_as_held(gpu, src):
    """Without a resize, with the table resize (3:2) and with the 2:1 box: starts [0, 5, 9]; the scores are the oracle's on
    the clip the feeder holds."""
    from vfml.runner import ClipFeeder
    frames = _graded(*src)
    feeder = ClipFeeder(frames, "cuda", size=(128, 192), scene_cuts=CUTS)
    assert (feeder.size is None) == (src == (128, 192))
    feeder.ensure(6)
    assert feeder.scenes.scene_of(5, 0) == (5, 6) and feeder.scenes.known == 7
    with pytest.raises(LookupError):
        feeder.scenes.scene_of(6, 0)                    # needs frame 7, which has not gone up
    feeder.ensure(12)
    assert feeder.scenes.scene_of(12) == (9, 13)
    torch.cuda.synchronize()
    held = list(feeder.clip.cpu().numpy())
    assert feeder.scenes.hs == so.scores(held)
    assert feeder.scenes.starts == so.GRADED_STARTS
    assert np.array_equal(_u32(feeder.cut_sig).reshape(13, 16, 64), so.distances(held)[0])
    # a second clip through the same feeder starts over
    feeder.reset(frames[5:] + frames[:5])
    feeder.ensure(12)
    assert feeder.scenes.scene_of(12) == (8, 13) and feeder.scenes.starts == [0, 4, 8]
    assert ClipFeeder(frames, "cuda", size=(128, 192)).scenes is None


# ---------------------------------------------------------------------------------------------------------------- jobs
def _mof(T, **over):
    from processing.videoflow_processor import VideoFlowProcessor
    from vfml import build_network, get_cfg
    from vfml.weights import seeded_state_dict
    cfg = get_cfg()
    cfg.decoder_depth = 4
    for k, v in over.items():
        setattr(cfg, k, v)
    net = build_network(cfg)
    net.load_state_dict(seeded_state_dict(cfg, 0))
    net.cuda().eval()
    kw = dict(architecture="bof", dataset="things") if over.get("network") == "BOFNet" else {}
    with contextlib.redirect_stdout(io.StringIO()):
        proc = VideoFlowProcessor("cuda", sequence_length=T, **kw)
    proc.core.model = net
    return proc


def _job(proc, frames, cuts, tile=False):
    """A sliding job over all frames through a fresh feeder -> float32 [F,H,W,2]."""
    from vfml.runner import ClipFeeder, run_sharded
    out = run_sharded(proc, None, range(len(frames)), tile_mode=tile, feeder=ClipFeeder(frames, "cuda", scene_cuts=cuts))
    assert proc.scenes is None                          # the index belongs to the job
    return out


def _per_scene(proc, frames, tile=False):
    return np.concatenate([_job(proc, frames[a:b], None, tile) for a, b in so.GRADED_SCENES])


def test_mof_job_keeps_every_window_inside_its_scene(gpu):
    """T = 5, 128 x 192, depth 4, seed 0, the 13-frame graded clip as a sliding job.  Cuts on: every field is the field of
    its scene run as a clip of its own through a fresh feeder, bit for bit.  Cuts off: today's job.  Fields 3, 4, 5, 6 - the
    windows that straddled the first cut - differ between the two."""
    frames = _graded(128, 192)
    proc = _mof(5)
    on = _job(proc, frames, CUTS)
    off = _job(proc, frames, None)
    own = _per_scene(proc, frames)
    for f in range(13):
        assert np.array_equal(on[f], own[f]), f
    from vfml.runner import run_sharded
    today = run_sharded(proc, proc.upload_clip(frames), range(13))
    assert np.array_equal(off, today)
    differ = [f for f in range(13) if not np.array_equal(on[f], off[f])]
    assert {3, 4, 5, 6} <= set(differ) and not {0, 1, 2, 12} & set(differ), differ
    # a resident clip without a feeder: all distances in one call before the job, the same fields
    resident = run_sharded(proc, proc.upload_clip(frames), range(13), scene_cuts=CUTS)
    assert np.array_equal(resident, on)


def test_bof_batched_job_equals_the_scenes(gpu):
    """T = 3, the tri-frame network: runs of triples break at a scene start, whose first field goes alone as frame 0 does."""
    frames = _graded(128, 192)
    proc = _mof(3, network="BOFNet")
    assert proc.core.model.tri_frame
    on = _job(proc, frames, CUTS)
    own = _per_scene(proc, frames)
    for f in range(13):
        assert np.array_equal(on[f], own[f]), f
    off = _job(proc, frames, None)
    assert [f for f in range(13) if not np.array_equal(on[f], off[f])] == [4, 5, 8, 9]


def test_one_tiled_job_equals_the_scenes(gpu):
    """128 x 192 cut into a 128 x 128 and a 128 x 64 tile on one rank: the same windows as whole frames.  (--fast's
    three-level pyramid with radius 3: a 64-pixel tile is 8 cells wide, too few for four levels.)"""
    frames = _graded(128, 192)
    proc = _mof(5, corr_levels=3, corr_radius=3)
    proc.tile_mode = True
    grid = proc.calculate_tile_grid
    proc.calculate_tile_grid = lambda w, h, tile_size=1280: grid(w, h, 128)
    assert len(proc.calculate_tile_grid(192, 128)[4]) == 2
    on = _job(proc, frames, CUTS, tile=True)
    own = _per_scene(proc, frames, tile=True)
    for f in range(13):
        assert np.array_equal(on[f], own[f]), f
    assert not np.array_equal(on[5], _job(proc, frames, None, tile=True)[5])


def _memflow(memory, warm):
    from processing.memflow_processor import MemFlowProcessor
    from vfml.memflow_net import build_memflow_network, memflow_cfg, seeded_memflow_state_dict
    cfg = memflow_cfg()
    cfg.decoder_depth = 4
    net = build_memflow_network(cfg)
    net.load_state_dict(seeded_memflow_state_dict(cfg, 0))
    net.cuda().eval()
    with contextlib.redirect_stdout(io.StringIO()):
        proc = MemFlowProcessor("cuda", sequence_length=3, memory_frames=memory, warm_start=warm)
    proc.core_engine.model = net
    return proc


def test_memflow_pairs_and_streams_stop_at_a_cut(gpu):
    """256 x 264.  Memory-free (pair batching): the fields at 5 and 9 are the pair (a, a), every field its scene's own.
    M = 1 with the warm start: the stream over the graded clip equals three fresh streams over the three scenes; field 5
    differs from the cuts-off stream's."""
    frames = _graded(256, 264)
    proc = _memflow(0, False)
    on = _job(proc, frames, CUTS)
    own = _per_scene(proc, frames)
    for f in range(13):
        assert np.array_equal(on[f], own[f]), f
    for a in (5, 9):
        pair = proc.compute_optical_flow_resident(proc.upload_clip([frames[a], frames[a]]), 1).cpu().numpy()
        assert np.array_equal(on[a], pair), a
    off = _job(proc, frames, None)
    assert [f for f in range(13) if not np.array_equal(on[f], off[f])] == [5, 9]

    st = _memflow(1, True)
    s_on = _job(st, frames, CUTS)
    s_own = _per_scene(st, frames)
    for f in range(13):
        assert np.array_equal(s_on[f], s_own[f]), f
    s_off = _job(st, frames, None)
    assert np.array_equal(s_on[:5], s_off[:5]) and not np.array_equal(s_on[5], s_off[5])


# -------------------------------------------------------------------------------------------------------------- render
def _render(tmp_path, name, frames, fields, scenes, device="cuda"):
    import flow_processor as fp
    from storage import FlowCacheManager
    from test_render_cpu import read_frames
    from video.scene_cuts import index_of, write_scenes
    work = tmp_path / name
    work.mkdir()
    clip = str(work / "clip.npy")
    np.save(clip, np.stack(frames))
    cache = work / "cache"
    cache.mkdir()
    for i, f in enumerate(fields):
        FlowCacheManager().save_flow_to_cache(f, str(cache), i, 'npz')
    if scenes:
        write_scenes(str(cache), index_of(so.scores(frames)))
    out = work / "out"
    out.mkdir()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = fp.main(["--input", clip, "--output", str(out), "--device", device, "--taa", "--skip-lods", "--uncompressed",
                      "--use-flow-cache", str(cache)])
    assert rc == 0, buf.getvalue()
    (avi,) = [n for n in os.listdir(out) if n.endswith(".avi")]
    return read_frames(str(out / avi))[0], buf.getvalue()


def test_taa_render_restarts_its_histories_at_a_scene_start(gpu, tmp_path):
    """A --taa render from a cache with scenes.json: every scene's frames are those of the scene rendered alone - its first
    frame with fresh histories, which is a reset by hand.  Without the file the old scene is blended into frames 5 and 9."""
    h, w = 64, 96
    frames = _graded(h, w)
    rng = np.random.default_rng(11)
    fields = [rng.uniform(-3, 3, (h, w, 2)).astype(np.float32) for _ in frames]
    cut, log = _render(tmp_path, "cut", frames, fields, True)
    assert "Scene cuts: 3 scenes" in log and "[5, 9]" in log
    plain, log = _render(tmp_path, "plain", frames, fields, False)
    assert "Scene cuts" not in log
    assert cut.shape == plain.shape == (13, 2 * h, 2 * w, 3)
    for k, (a, b) in enumerate(so.GRADED_SCENES):
        alone, _ = _render(tmp_path, f"scene{k}", frames[a:b], fields[a:b], False)
        assert np.array_equal(cut[a:b], alone), (a, b)
    assert np.array_equal(cut[:5], plain[:5])
    for f in (5, 9):
        assert np.array_equal(cut[f][:h], plain[f][:h])                 # original | flow do not look back
        assert not np.array_equal(cut[f][h:], plain[f][h:])             # the TAA tiles do
    # the host path reads the same file
    host, _ = _render(tmp_path, "host", frames, fields, True, device="cpu")
    d = np.abs(host.astype(int) - cut.astype(int))
    assert d.max() <= 1
