"""Scene cuts without a GPU: the oracle against a plain loop, the rule, the graded clips with their
margins, the scene windows of both processors, the setting, the cache names, scenes.json, and the host path of the feeder
and the runner (a CPU "device" with a stand-in model) against the oracle."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import scene_cut_oracle as so


def _rand_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ definition and oracle
@pytest.mark.parametrize("h,w", [(3, 5), (7, 9)])
def test_oracle_signature_equals_a_plain_loop(h, w):
    from video.scene_cuts import frame_signature
    for seed in range(3):
        f = _rand_frame(h, w, seed)
        loop = so.signature_loop(f)
        assert loop.sum() == h * w
        assert np.array_equal(so.signature(f), loop)
        assert np.array_equal(frame_signature(f), loop)
    # 3 rows leave cell rows empty: y * 4 // 3 is 0, 1, 2
    assert so.signature_loop(_rand_frame(3, 5, 0))[12:].sum() == 0


def test_luma_is_the_integer_formula_at_its_corners():
    for rgb, y in (((0, 0, 0), 0), ((255, 255, 255), 255), ((255, 0, 0), 77), ((0, 255, 0), 149), ((0, 0, 255), 29)):
        f = np.array(rgb, dtype=np.uint8).reshape(1, 1, 3)
        assert (77 * rgb[0] + 150 * rgb[1] + 29 * rgb[2] + 128) >> 8 == y
        assert so.signature(f)[0, y >> 2] == 1


RULE_CASES = [
    # scores (hs[0] is ignored), starts at TH = 200, R = 3
    ([0, 5, 6, 700, 8, 4], [0, 3]),                     # an isolated peak
    ([0, 5, 900, 910, 6, 4], [0]),                      # a flash: two high scores side by side
    ([0, 300, 320, 350, 400, 470], [0]),                # a fade: a run of them
    ([0, 5, 6, 7, 650], [0, 4]),                        # a peak at the last frame: the neighbour outside counts as 0
    ([0, 650, 7, 6], [0, 1]),                           # a peak at frame 1: hs[0] counts as 0
    ([900, 5, 6], [0]),                                 # hs[0] itself is never looked at
    ([0, 10, 199, 10], [0]),                            # TH: 199 is below
    ([0, 10, 200, 10], [0, 2]),                         # TH: 200 is not
    ([0, 67, 200, 10], [0]),                            # R: 200 < 3 * 67
    ([0, 66, 200, 10], [0, 2]),                         # R: 200 >= 3 * 66
    ([0, 10, 600, 200, 10], [0, 2]),                    # R on the other side: 600 >= 3 * 200, and 200 < 3 * 600
    ([0, 10, 600, 201, 10], [0]),
    ([0, 800, 800, 5], [0]),                            # two cuts one frame apart cannot both fire: neither does
    ([0], [0]),
]


@pytest.mark.parametrize("hs,want", RULE_CASES)
def test_rule_on_hand_written_scores(hs, want):
    from video.scene_cuts import index_of, scene_starts
    assert so.starts(hs) == want
    assert scene_starts(hs, 200, 3) == want
    idx = index_of(hs, 200, 3)
    assert idx.starts == want
    bounds = want + [len(hs)]
    for f in range(len(hs)):
        k = max(j for j, s in enumerate(want) if s <= f)
        assert idx.scene_of(f) == (bounds[k], bounds[k + 1])


def test_rule_settings_move_the_boundaries():
    from video.scene_cuts import scene_starts
    hs = [0, 40, 150, 40, 10]
    assert scene_starts(hs, 200, 3) == [0]
    assert scene_starts(hs, 150, 3) == [0, 2]
    assert scene_starts(hs, 151, 3) == [0]
    assert scene_starts(hs, 150, 4) == [0]            # 150 < 4 * 40
    assert scene_starts(hs, 150, 2) == [0, 2]


@pytest.mark.parametrize("h,w", [(30, 46), (128, 192), (256, 264)])
def test_graded_clip_starts_with_margins(h, w):
    from video.scene_cuts import host_scene_index
    frames = so.graded_clip(h, w)
    hs = so.scores(frames)
    print(f"{h}x{w} scores {hs}")
    assert so.starts(hs) == so.GRADED_STARTS
    for cut in (5, 9):
        assert hs[cut] >= so.TH
        assert hs[cut] >= so.R * max(hs[cut - 1], hs[cut + 1])
    idx = host_scene_index(frames)
    assert idx.hs == hs and idx.starts == so.GRADED_STARTS
    assert [idx.scene_of(f) for f in (0, 4, 5, 8, 9, 12)] == [(0, 5), (0, 5), (5, 9), (5, 9), (9, 13), (9, 13)]


@pytest.mark.parametrize("h,w", [(30, 46), (128, 192), (256, 264)])
@pytest.mark.parametrize("clip", ["flash_clip", "fade_clip", "insert_clip"])
def test_no_start_on_flash_fade_and_one_frame_insert(h, w, clip):
    from video.scene_cuts import host_scene_index
    frames = getattr(so, clip)(h, w)
    hs = so.scores(frames)
    print(f"{clip} {h}x{w} scores {hs}")
    assert max(hs) >= so.TH                   # the clip does reach the threshold: it is the isolation that fails
    assert so.starts(hs) == [0]
    assert host_scene_index(frames).starts == [0]


# ---------------------------------------------------------------------------------------------------------- the index
def test_index_grows_with_the_scores_and_refuses_what_it_does_not_know():
    from video.scene_cuts import SceneIndex
    hs = [0, 5, 6, 7, 8, 800, 6, 5, 4, 900, 5, 4, 3]
    idx = SceneIndex(13)
    with pytest.raises(LookupError):
        idx.scene_of(0, 0)
    for v in hs[:6]:
        idx.push(v)                                     # scores 0..5: frames 0..4 are decided, 5 needs hs[6]
    assert idx.scene_of(2, 2) == (0, 5)                 # nothing starts in (2, 4]: the scene goes on at least to 5
    with pytest.raises(LookupError, match="frame 6"):
        idx.scene_of(3, 2)
    with pytest.raises(LookupError):
        idx.scene_of(4)                                 # the true end needs every score
    idx.push(hs[6])
    assert idx.scene_of(3, 2) == (0, 5) and idx.scene_of(5, 0) == (5, 6)
    for v in hs[7:]:
        idx.push(v)
    assert idx.starts == [0, 5, 9] and idx.scene_of(4) == (0, 5) and idx.scene_of(12) == (9, 13)
    with pytest.raises(IndexError):
        idx.push(1)
    with pytest.raises(LookupError):
        idx.scene_of(13)


def test_index_takes_scores_from_a_source_on_demand():
    from video.scene_cuts import SceneIndex
    hs = [0, 5, 6, 7, 8, 800, 6, 5, 4, 900, 5, 4, 3]
    asked, ready = [], [7]
    idx = SceneIndex(13, source=lambda f: (asked.append(f), hs[f])[1] if f < ready[0] else None)
    assert idx.scene_of(1, 2) == (0, 4) and asked == [0, 1, 2, 3, 4]       # no more than the question needs
    assert idx.scene_of(5, 0) == (5, 6)
    with pytest.raises(LookupError):
        idx.scene_of(5, 2)
    ready[0] = 13
    assert idx.scene_of(5, 2) == (5, 8) and idx.scene_of(7, 2) == (5, 9)


def test_index_from_a_later_first_frame():
    from video.scene_cuts import SceneIndex
    idx = SceneIndex(10, first=4)
    for v in (999, 5, 700, 5, 5, 5):                    # frames 4..9; frame 4 has no predecessor here: its score is not used
        idx.push(v)
    assert idx.starts == [4, 6]
    assert idx.scene_of(5) == (4, 6) and idx.scene_of(9) == (6, 10)
    with pytest.raises(LookupError):
        idx.scene_of(3)


# ------------------------------------------------------------------------------------------------------------- windows
def _vf(T):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        return VideoFlowProcessor("cpu", sequence_length=T)


def _mf(T):
    from processing.memflow_processor import MemFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        return MemFlowProcessor("cpu", sequence_length=T)


def _thirteen():
    from video.scene_cuts import index_of
    return index_of([0, 5, 6, 7, 8, 800, 6, 5, 4, 900, 5, 4, 3])


@pytest.mark.parametrize("T", [3, 5])
def test_videoflow_window_is_the_scenes_own_window_shifted(T):
    proc, plain = _vf(T), _vf(T)
    proc.scenes = _thirteen()
    for a, b in so.GRADED_SCENES:
        for f in range(a, b):
            want = [a + i for i in plain.window_indices(b - a, f - a)]
            assert proc.window_indices(13, f) == want
            assert len(want) == T and all(a <= i < b for i in want)
    # a growing index gives the same windows as the complete one, from the scores up to f + T // 2 + 1 alone
    from video.scene_cuts import SceneIndex
    hs = _thirteen().hs
    for f in range(13):
        part = SceneIndex(13)
        for v in hs[:min(13, f + T // 2 + 2)]:
            part.push(v)
        grown = _vf(T)
        grown.scenes = part
        assert grown.window_indices(13, f) == proc.window_indices(13, f)


def test_memflow_pairs_clamp_at_the_scene_start():
    proc = _mf(2)
    proc.scenes = _thirteen()
    assert proc.window_indices(5) == [5, 5] and proc.window_indices(9) == [9, 9] and proc.window_indices(0) == [0, 0]
    assert proc.window_indices(6) == [5, 6] and proc.window_indices(12) == [11, 12] and proc.window_indices(4) == [3, 4]
    long = _mf(4)
    long.scenes = _thirteen()
    assert long.window_indices(6) == [5, 5, 5, 6] and long.window_indices(8) == [5, 6, 7, 8]


@pytest.mark.parametrize("T", [3, 5])
def test_without_an_index_both_processors_return_todays_windows(T):
    vf, mf = _vf(T), _mf(T)
    assert vf.scenes is None and mf.scenes is None
    for n in (1, 2, 13):
        for f in range(n):
            half = T // 2
            start = max(0, f - half)
            idx = list(range(start, min(n, f + half + 1)))
            while len(idx) < T:
                idx = [idx[0]] + idx if start == 0 else idx + [idx[-1]]
            assert vf.window_indices(n, f) == idx[:T]
            want = list(range(max(0, f + 1 - mf.sequence_length), f + 1))
            want = [want[0]] * (mf.sequence_length - len(want)) + want
            assert mf.window_indices(f) == want


# ------------------------------------------------------------------------------------------------------------ interface
def test_check_scene_cuts_accepts_and_refuses():
    from video.scene_cuts import check_scene_cuts
    assert check_scene_cuts(None) is None and check_scene_cuts("0") is None and check_scene_cuts(0) is None
    assert check_scene_cuts(False) is None
    assert check_scene_cuts("1") == (200, 3) and check_scene_cuts(1) == (200, 3) and check_scene_cuts(True) == (200, 3)
    assert check_scene_cuts("150,4") == (150, 4) and check_scene_cuts(" 1 , 2 ") == (1, 2) and check_scene_cuts((300, 5)) == (300, 5)
    for bad in ("2", "yes", "", "0,3", "200,1", "200", "200,3,1", "-200,3", "200,-3", "2.5,3", "200;3", 1.5, (200,), [200, 3]):
        with pytest.raises(ValueError, match="VFML_SCENE_CUTS.*TH,R"):
            check_scene_cuts(bad, "VFML_SCENE_CUTS")


def test_setting_comes_from_the_module_or_the_environment(monkeypatch):
    import flow_processor as fp
    monkeypatch.delenv("VFML_SCENE_CUTS", raising=False)
    assert fp.SCENE_CUTS is None and fp.scene_cuts() is None
    monkeypatch.setenv("VFML_SCENE_CUTS", "1")
    assert fp.scene_cuts() == (200, 3)
    monkeypatch.setenv("VFML_SCENE_CUTS", "120,5")
    assert fp.scene_cuts() == (120, 5)
    monkeypatch.setenv("VFML_SCENE_CUTS", "on")
    with pytest.raises(ValueError, match="VFML_SCENE_CUTS"):
        fp.scene_cuts()
    assert fp.main(["--input", "synthetic:64x64x3", "--output", "unused"]) == 1     # refused before anything is computed
    monkeypatch.delenv("VFML_SCENE_CUTS")
    monkeypatch.setattr(fp, "SCENE_CUTS", "250,4")
    assert fp.scene_cuts() == (250, 4)
    assert "--scene" not in fp.build_parser().format_help()         # no new flag: the parser stays the reference's


def test_cache_names_unchanged_when_off_and_suffixed_when_on():
    from storage import FlowCacheManager
    from storage.filename_generator import generate_cache_directory as gen
    base = gen("clips/a.mov", 3, 40, 5, True, True, 'videoflow', 'sintel', 'mof', 'standard')
    assert base == "clips/a_flow_cache_videoflow_mof_sintel_standard_seq5_start3_frames40_fast_tile"
    assert gen("clips/a.mov", 3, 40, 5, True, True, 'videoflow', 'sintel', 'mof', 'standard', scene_cuts=None) == base
    assert gen("clips/a.mov", 3, 40, 5, True, True, 'videoflow', 'sintel', 'mof', 'standard', scene_cuts=(200, 3)) == base + "_cuts"
    assert gen("clips/a.mov", 3, 40, 5, True, True, 'videoflow', 'sintel', 'mof', 'standard', scene_cuts=(150, 4)) == base + "_cuts150x4"
    mem = gen("a.mov", 0, 9, 3, False, False, 'memflow', 'sintel', memory_frames=2, warm_start=True)
    assert mem == "a_flow_cache_memflow_sintel_seq3_start0_frames9_mem2_warm"
    assert gen("a.mov", 0, 9, 3, False, False, 'memflow', 'sintel', memory_frames=2, warm_start=True,
               scene_cuts=(200, 3)) == mem + "_cuts"                                  # last
    mgr = FlowCacheManager()
    assert mgr.generate_cache_path("a.mov", 0, 9, 3, False, False, 'memflow', 'sintel') == "a_flow_cache_memflow_sintel_seq3_start0_frames9"
    assert mgr.generate_cache_path("a.mov", 0, 9, 3, False, False, 'memflow', 'sintel', scene_cuts=(200, 4)).endswith("_cuts200x4")


def test_scenes_json_round_trip(tmp_path):
    import json
    from video.scene_cuts import SceneIndex, read_scenes, write_scenes
    idx = _thirteen()
    assert read_scenes(str(tmp_path)) is None
    path = write_scenes(str(tmp_path / "cache"), idx)
    assert os.path.basename(path) == "scenes.json"
    doc = read_scenes(str(tmp_path / "cache"))
    assert doc == {"threshold": 200, "ratio": 3, "starts": [0, 5, 9], "score": idx.hs}
    assert json.load(open(path)) == doc
    part = SceneIndex(13)
    part.push(0)
    with pytest.raises(LookupError):
        write_scenes(str(tmp_path / "cache"), part)       # an index that is not complete is not written
    (tmp_path / "bad").mkdir()
    (tmp_path / "bad" / "scenes.json").write_text('{"starts": "0,5"}')
    with pytest.raises(ValueError):
        read_scenes(str(tmp_path / "bad"))


# ------------------------------------------------------------------------------------ the host path: feeder and runner
class FakeModel(torch.nn.Module):
    """Stands in for the network: a field that depends on every frame of its window and on their order."""
    tri_frame = False

    def forward(self, x, _):
        B, T, C, H, W = x.shape
        wts = torch.arange(1, T + 1, dtype=x.dtype).view(1, T, 1, 1, 1)
        base = (x[:, :, :2] * wts).sum(dim=1, keepdim=True)
        flows = torch.cat([base * (k + 1) for k in range(2 * (T - 2))], dim=1)
        return flows.view(B, 2 * (T - 2), 2, H, W), None


def _fake_proc(T=5, tile=False):
    from processing.videoflow_processor import VideoFlowProcessor
    with contextlib.redirect_stdout(io.StringIO()):
        p = VideoFlowProcessor("cpu", tile_mode=tile, sequence_length=T)
    p.core.model = FakeModel()
    grid = p.calculate_tile_grid
    p.calculate_tile_grid = lambda w, h, tile_size=1280: grid(w, h, 24)
    return p


@pytest.mark.parametrize("size", [None, (24, 32)])
def test_cpu_feeder_scores_equal_the_oracle(size):
    """--device cpu: the feeder measures the frames as the clip holds them (behind the host resize where there is one)."""
    from vfml.runner import ClipFeeder
    frames = so.graded_clip(48, 64)
    feeder = ClipFeeder(frames, "cpu", size=size, scene_cuts=(200, 3))
    with pytest.raises(LookupError):
        feeder.scenes.scene_of(0, 0)                    # nothing uploaded, nothing known
    feeder.ensure(6)
    assert feeder.scenes.scene_of(5, 0) == (5, 6)
    with pytest.raises(LookupError):
        feeder.scenes.scene_of(6, 0)
    feeder.ensure(12)
    held = [f for f in feeder.clip.numpy()]
    assert feeder.scenes.scene_of(12) == (9, 13)
    assert feeder.scenes.hs == so.scores(held) and feeder.scenes.starts == so.GRADED_STARTS
    assert ClipFeeder(frames, "cpu").scenes is None


@pytest.mark.parametrize("T,tile", [(5, False), (3, False), (5, True)])
def test_cpu_job_with_cuts_equals_the_scenes_run_as_clips_of_their_own(T, tile):
    from vfml.runner import ClipFeeder, run_sharded
    frames = so.graded_clip(48, 64)
    on = run_sharded(_fake_proc(T, tile), None, range(13), tile_mode=tile, feeder=ClipFeeder(frames, "cpu", scene_cuts=(200, 3)))
    off = run_sharded(_fake_proc(T, tile), None, range(13), tile_mode=tile, feeder=ClipFeeder(frames, "cpu"))
    today = run_sharded(_fake_proc(T, tile), None, range(13), tile_mode=tile, feeder=ClipFeeder(frames, "cpu", scene_cuts=None))
    assert np.array_equal(off, today)
    for a, b in so.GRADED_SCENES:
        own = run_sharded(_fake_proc(T, tile), None, range(b - a), tile_mode=tile, feeder=ClipFeeder(frames[a:b], "cpu"))
        assert np.array_equal(on[a:b], own)
    differ = [f for f in range(13) if not np.array_equal(on[f], off[f])]
    # exactly the fields whose window changed (T = 5 includes frame 11: a 4-frame scene pads [9, 9, 10, 11, 12] at the front
    # where the clip's end pads [9, 10, 11, 12, 12] at the back)
    plain, scened = _vf(T), _vf(T)
    scened.scenes = _thirteen()
    assert differ == [f for f in range(13) if plain.window_indices(13, f) != scened.window_indices(13, f)]
    assert {3, 4, 5, 6} <= set(differ) if T == 5 else {4, 5} <= set(differ)
    # a resident clip without a feeder: the same fields, the index made before the job
    proc = _fake_proc(T, tile)
    resident = run_sharded(proc, proc.upload_clip(frames), range(13), tile_mode=tile, scene_cuts=(200, 3))
    assert np.array_equal(resident, on) and proc.scenes is None


def test_jobs_over_several_ranks_are_refused():
    from vfml.runner import check_scene_job, run_sharded
    check_scene_job(None, True, 8)
    check_scene_job((200, 3), True, 1)
    check_scene_job((200, 3), False, 1)
    with pytest.raises(ValueError, match="one GPU"):
        check_scene_job((200, 3), True, 2)
    proc = _fake_proc()
    with pytest.raises(ValueError, match="one GPU"):
        run_sharded(proc, proc.upload_clip(so.graded_clip(48, 64)), range(13), rank=0, world=2, scene_cuts=(200, 3))
