"""The project's text on the host ("Text"): the stroke font's invariants, text_size and the anchors
against numbers worked out by hand, visualization/text.py byte for byte against tests/text_oracle.py, the composer's
labels behind their switch, create_video_grid, the plan compiler's boxes and vfml_text_draw's argument checks (which
need no GPU)."""
import ctypes
import functools

import numpy as np
import pytest

import text_oracle as oracle
from visualization import text as vtext
from visualization import video_composer as vc
from visualization.stroke_font import GLYPHS

ALL_GLYPHS = "".join(chr(c) for c in range(0x20, 0x7F))
REFERENCE_LABELS = ("Original", "Optical Flow", "VideoFlow (GAMEDEV)", "TAA + Inv.Flow", "Alpha: 0.1", "TAA Simple",
                    "Original (Fast)", "Optical Flow (Fast)", "VideoFlow (MOTION-VECTORS-RGB8)", "External Flow",
                    "TAA + Original Flow", "TAA + External Flow", "Flow Difference", "0.100", "0.500", "1.000", "2.000",
                    ">2.000")


def noise(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the font ----------------------------------------------------------------------------------------------------------
def test_font_table_invariants():
    assert sorted(GLYPHS) == sorted(ALL_GLYPHS)
    assert GLYPHS[' '][1] == ()
    seen = {}
    for ch, (adv, segs) in GLYPHS.items():
        assert isinstance(adv, int) and 8 <= adv <= 26, (ch, adv)
        if ch != ' ':
            assert len(segs) >= 1, ch
        for seg in segs:
            assert all(isinstance(v, int) for v in seg) and len(seg) == 4, (ch, seg)
            assert 0 <= seg[0] <= adv and 0 <= seg[2] <= adv and -7 <= seg[1] <= 24 and -7 <= seg[3] <= 24, (ch, seg)
        assert segs not in seen, f"{ch!r} is drawn as {seen.get(segs)!r}"
        seen[segs] = ch
    for ch in "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789":
        ys = [y for s in GLYPHS[ch][1] for y in (s[1], s[3])]
        assert max(ys) == 21 and min(ys) >= -2, ch                       # cap height; only Q's tail dips
    for ch in "acemnorsuvwxz":
        ys = [y for s in GLYPHS[ch][1] for y in (s[1], s[3])]
        assert max(ys) == 14 and min(ys) == 0, ch                        # x-height
    for ch in "gjpqy":
        assert min(y for s in GLYPHS[ch][1] for y in (s[1], s[3])) == -7, ch
    for ch in ".:!ij?;":
        assert any(s[0] == s[2] and s[1] == s[3] for s in GLYPHS[ch][1]), f"{ch!r} has no dot"
    assert vtext.glyph("é") is GLYPHS['?'] and vtext.glyph("\n") is GLYPHS['?']


def test_text_size_and_anchors_by_hand():
    # "Original": advances O 22, r 13, i 8, g 19, i 8, n 19, a 19, l 8 = 116; S = round(0.4 * 256) = 102
    # width (116 * 102 + 128) >> 8 = 11960 >> 8 = 46, + thickness 1 = 47; height (21 * 102 + 128) >> 8 = 8, + (1 + 1) // 2 = 9
    assert sum(GLYPHS[c][0] for c in "Original") == 116
    assert vtext.scale_of(0.4) == 102 and vtext.scale_of(0.7) == 179 and vtext.scale_of(0.3) == 77
    assert vtext.text_size("Original", 0.4, 1) == oracle.text_size("Original", 0.4, 1) == (47, 9)
    got = {p: vtext.anchor(p, "Original", 0.4, 1, 48, 128) for p in ('top-left', 'top-right', 'bottom-left',
                                                                     'bottom-right', 'elsewhere', (7, 9))}
    assert got == {'top-left': (5, 14), 'top-right': (76, 14), 'bottom-left': (5, 43), 'bottom-right': (76, 43),
                   'elsewhere': (5, 14), (7, 9): (7, 9)}
    # "TAA + Inv.Flow": T 16, A 18, A 18, ' ' 12, + 22, ' ' 12, I 10, n 19, v 16, . 10, F 18, l 8, o 19, w 22 = 220; S = 179
    # width (220 * 179 + 128) >> 8 = 39508 >> 8 = 154, + 2 = 156; height (21 * 179 + 128) >> 8 = 15, + 3 // 2 = 16
    assert sum(GLYPHS[c][0] for c in "TAA + Inv.Flow") == 220
    assert vtext.text_size("TAA + Inv.Flow", 0.7, 2) == oracle.text_size("TAA + Inv.Flow", 0.7, 2) == (156, 16)
    for p, want in (('top-left', (5, 21)), ('top-right', (239, 21)), ('bottom-left', (5, 95)), ('bottom-right', (239, 95))):
        assert vtext.anchor(p, "TAA + Inv.Flow", 0.7, 2, 100, 400) == want
        assert oracle.anchor(p, "TAA + Inv.Flow", 0.7, 2, 100, 400) == want


# ---- host path against the oracle ------------------------------------------------------------------------------------------
def label_cases():
    """(name, h, w, operations): the draw lists shared by the host tests and tests/test_gpu_text.py."""
    cases = []
    for h, w, tag in ((48, 128, "tile"), (48, 40, "clipped")):
        ops = []
        for k, text in enumerate(REFERENCE_LABELS):
            ops += oracle.overlay_ops(text, ('top-left', 'bottom-left', 'top-right', 'bottom-right')[k % 4], h, w)
        cases.append((f"labels_{tag}", h, w, ops))
        cases.append((f"legend_{tag}", h, w, oracle.legend_ops(h, w)))
    a = oracle.overlay_ops("TAA + Inv.Flow", (6, 20), 48, 128, font_scale=0.7, colour=(255, 200, 40), thickness=2)
    b = oracle.overlay_ops("Alpha: 0.1", (30, 24), 48, 128, colour=(20, 220, 90))
    cases.append(("overlap_ab", 48, 128, a + b))
    cases.append(("overlap_ba", 48, 128, b + a))
    edges = []
    for origin in ((-12, 20), (110, 30), (40, 3), (40, 52)):              # left, right, top, bottom edge
        edges += oracle.overlay_ops("Edge gjpqy", origin, 48, 128, font_scale=0.7, thickness=2)
    cases.append(("edges", 48, 128, edges))
    cases.append(("outside", 48, 128, oracle.overlay_ops("Nowhere", (300, 20), 48, 128) +
                  oracle.overlay_ops("Nowhere", (10, -40), 48, 128) + oracle.overlay_ops("Nowhere", (10, 200), 48, 128)))
    cases.append(("dots", 48, 128, oracle.overlay_ops(".:!i", (10, 30), 48, 128, font_scale=0.7, thickness=2) +
                  [("text", ".:!i", (70, 30), 77, 1, (255, 255, 255), False, (0, 0, 127, 47))]))
    cases.append(("video_grid_label", 36, 64, oracle.video_grid_label_ops("TAA-Flow\nalpha 0.1", 36, 64)))
    for scale in (0.3, 0.4, 0.7):
        for thickness in (1, 2):
            for aa in (True, False):
                S = oracle.scale_of(scale)
                cases.append((f"glyphs_{scale}_{thickness}_{'aa' if aa else 'plain'}", 64, 700,
                              [("text", ALL_GLYPHS, (3, 40), S, thickness, (250, 240, 30), aa, (0, 0, 699, 63))]))
    return cases


CASES = {c[0]: c for c in label_cases()}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's picture of a case on its noise background, computed once per session."""
    _, h, w, ops = CASES[name]
    out = oracle.draw_ops(noise(h, w), ops)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_host_path_equals_oracle(name):
    _, h, w, ops = CASES[name]
    src = noise(h, w)
    got = vtext.draw_ops(src, ops)
    np.testing.assert_array_equal(got, expected(name))
    if name == "outside":
        np.testing.assert_array_equal(got, src)
    else:
        assert (got != src).any()


def test_overlapping_labels_depend_on_their_order():
    assert (expected("overlap_ab") != expected("overlap_ba")).any()


def test_all_glyph_string_covers_the_picture_width():
    assert oracle.text_size(ALL_GLYPHS, 0.7, 2)[0] > 700 > oracle.text_size(ALL_GLYPHS, 0.3, 1)[0]    # clips at 0.7 only


# ---- the composer behind the switch ------------------------------------------------------------------------------------------
def _tiles(h, w):
    rng = np.random.default_rng(h * w)
    u8 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    hist = [rng.uniform(-40, 300, (h, w, 3)).astype(np.float32) for _ in range(3)]
    return u8, hist


def _only_inside_boxes(on, off, ops):
    h, w = off.shape[:2]
    allowed = np.zeros((h, w), bool)
    for x0, y0, x1, y1, _, _ in vtext.plan_boxes(vtext.build_plan(ops, h, w)):
        allowed[y0:y1 + 1, x0:x1 + 1] = True
    changed = (on != off).any(2)
    assert changed.any() and not (changed & ~allowed).any()


def test_composer_labels_are_off_by_default_and_stay_in_their_boxes(monkeypatch):
    monkeypatch.delenv("VFML_LABELS", raising=False)
    h, w = 48, 128
    (a, b, c), (t0, t1, t2) = _tiles(h, w)
    assert vc.add_text_overlay(a, "Original") is a                         # today's behaviour: the frame itself
    for taa, kw in ((0, {}), (1, {"taa_frame": t0}), (2, {"taa_frame": t0, "taa_simple_frame": t1})):
        off = vc.create_side_by_side(a, b, **kw)
        np.testing.assert_array_equal(off, vc.create_side_by_side(a, b, labels=False, **kw))
        on = vc.create_side_by_side(a, b, model_name="MemFlow", fast_mode=True, flow_format="hsv", labels=True, **kw)
        ops = oracle.side_by_side_ops(h, w, taa, "MemFlow", True, "hsv")
        np.testing.assert_array_equal(on, oracle.draw_ops(off, ops))
        _only_inside_boxes(on, off, ops)
    stacked = vc.create_side_by_side(a, b, flow_only=True)
    np.testing.assert_array_equal(vc.create_side_by_side(a, b, flow_only=True, labels=True), stacked)   # none under flow_only
    f0 = np.random.default_rng(1).normal(0, 1, (h, w, 2)).astype(np.float32)
    f1 = np.random.default_rng(2).normal(0, 1, (h, w, 2)).astype(np.float32)
    legend_off = vc.create_difference_overlay(f0, f1)
    legend_on = vc.create_difference_overlay(f0, f1, labels=True)
    np.testing.assert_array_equal(legend_on, oracle.draw_ops(legend_off, oracle.legend_ops(h, w)))
    _only_inside_boxes(legend_on, legend_off, oracle.legend_ops(h, w))
    grid_off = vc.create_6_video_grid(a, b, t0, t1, t2, legend_off)
    grid_on = vc.create_6_video_grid(a, b, t0, t1, t2, legend_off, labels=True)
    np.testing.assert_array_equal(grid_on, oracle.draw_ops(grid_off, oracle.grid6_ops(h, w)))
    _only_inside_boxes(grid_on, grid_off, oracle.grid6_ops(h, w))
    # the environment switch is the default of `labels`
    monkeypatch.setenv("VFML_LABELS", "1")
    np.testing.assert_array_equal(vc.create_6_video_grid(a, b, t0, t1, t2, legend_off), grid_on)
    np.testing.assert_array_equal(vc.add_text_overlay(a, "Original"), vc.draw_text(a, "Original"))
    monkeypatch.setenv("VFML_LABELS", "0")
    np.testing.assert_array_equal(vc.create_6_video_grid(a, b, t0, t1, t2, legend_off), grid_off)
    np.testing.assert_array_equal(vc.draw_text(a, "Original", 'bottom-right', 0.7, (10, 200, 30), 2),
                                  oracle.draw_ops(a, oracle.overlay_ops("Original", 'bottom-right', h, w, font_scale=0.7,
                                                                        colour=(10, 200, 30), thickness=2)))


def test_create_video_grid_canvas_offsets_and_backdrop():
    import visualization
    h, w = 36, 64
    rng = np.random.default_rng(7)
    frames = {"Original": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
              "Flow Viz": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
              "TAA-Flow\nalpha 0.1": rng.uniform(-40, 300, (h, w, 3)),
              "x": np.full((h, w, 3), 200, np.uint8)}
    grid = visualization.create_video_grid(frames, (2, 2), target_aspect=4 / 3)
    assert grid.shape == (96, 128, 3) and grid.dtype == np.uint8          # 2 * 64 wide, int(128 / (4 / 3)) high
    assert not grid[:12].any() and not grid[84:].any()                     # y offset (96 - 72) // 2 = 12, x offset 0
    for k, (label, frame) in enumerate(frames.items()):
        bgr = vc.history_to_u8(frame)[:, :, ::-1]
        want = oracle.draw_ops(bgr, oracle.video_grid_label_ops(label, h, w))
        cell = grid[12 + (k // 2) * h:12 + (k // 2 + 1) * h, (k % 2) * w:(k % 2 + 1) * w]
        np.testing.assert_array_equal(cell, want, err_msg=label)
    # backdrop bytes: "x" at 0.7 / 2 is ((17 * 179 + 128) >> 8) + 2 = 14 wide, so (0, 0)..(29, 40) is dimmed:
    # (3 * 200 + 5) // 10 = 60 where no stroke falls, 200 outside
    cell = grid[48:84, 64:128]
    assert oracle.text_size("x", 0.7, 2) == (14, 16)
    assert (cell[0, :30] == 60).all() and (cell[:, 30:] == 200).all() and (cell[35, :30] == 60).all()
    assert visualization.create_video_grid({}, (2, 2)) is None
    assert visualization.create_video_grid(frames, (2, 2)).shape == (72, 128, 3)      # the default 16:9: int(128 / (16 / 9))
    # a canvas lower than the two rows: cells that do not fit are left out
    low = visualization.create_video_grid(frames, (2, 2), target_aspect=2.0)
    assert low.shape == (64, 128, 3) and not low.any()


def test_draw_labels_switch(monkeypatch):
    import flow_processor as fp
    monkeypatch.delenv("VFML_LABELS", raising=False)
    assert fp.DRAW_LABELS is False and fp.draw_labels() is False
    monkeypatch.setenv("VFML_LABELS", "1")
    assert fp.draw_labels() is True
    monkeypatch.setenv("VFML_LABELS", "0")
    monkeypatch.setattr(fp, "DRAW_LABELS", True)
    assert fp.draw_labels() is False
    monkeypatch.setenv("VFML_LABELS", "maybe")
    with pytest.raises(ValueError, match="VFML_LABELS"):
        fp.draw_labels()
    with pytest.raises(ValueError, match="VFML_LABELS"):                   # refused before anything is computed
        fp.main(["--input", "synthetic:64x64x2", "--output", "nowhere", "--device", "cpu"])


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_build_plan_merges_overlapping_operations_into_disjoint_boxes():
    h, w = 96, 256
    ops = oracle.side_by_side_ops(48, 128, 2)
    plan = vtext.build_plan(ops, h, w)
    assert plan.dtype == np.int32 and plan[0] == vtext.PLAN_MAGIC and plan[1] == plan.size and plan[5] == len(ops)
    boxes = vtext.plan_boxes(plan)
    assert len(boxes) == 7 and sorted(b[5] for b in boxes) == [2] * 7      # outline and fill of every label share a box
    assert sum(b[5] for b in boxes) == len(ops)
    for i, a in enumerate(boxes):
        assert 0 <= a[0] <= a[2] < w and 0 <= a[1] <= a[3] < h
        for b in boxes[:i]:
            assert a[0] > b[2] or b[0] > a[2] or a[1] > b[3] or b[1] > a[3], (a, b)
    # two labels that overlap each other end in one box with all four operations, in draw order
    _, _, _, both = CASES["overlap_ab"]
    merged = vtext.plan_boxes(vtext.build_plan(both, 48, 128))
    assert len(merged) == 1 and merged[0][4:] == (0, 4)
    # small tiles: the top and the bottom label of a tile touch and are merged too; still disjoint
    small = vtext.plan_boxes(vtext.build_plan(oracle.side_by_side_ops(24, 64, 2), 48, 128))
    assert len(small) < 7
    for i, a in enumerate(small):
        for b in small[:i]:
            assert a[0] > b[2] or b[0] > a[2] or a[1] > b[3] or b[1] > a[3], (a, b)
    assert vtext.build_plan(CASES["outside"][3], 48, 128)[4] == 0          # nothing can touch the frame: no box
    with pytest.raises(ValueError):
        vtext.build_plan([("text", "x", (0, 0), 256 * 9, 1, (0, 0, 0), True, (0, 0, 9, 9))], 10, 10)


def test_text_draw_rejects_malformed_plans_without_a_gpu():
    """Like test_abi.test_argument_validation_needs_no_gpu: the plan's host words are checked before any launch."""
    from vfml import hip
    L = hip.lib()
    h, w = 48, 128
    plan = vtext.build_plan(CASES["labels_tile"][3], h, w)
    img = np.zeros((h, 3 * w), np.uint8)

    def call(words, n=None, hh=h, ww=w, stride=3 * w, flags=0, image=img):
        words = np.ascontiguousarray(words, dtype=np.int32)
        return L.vfml_text_draw(words.ctypes.data_as(ctypes.c_void_p), len(words) if n is None else n,
                                None if image is None else image.ctypes.data_as(ctypes.c_void_p), hh, ww, stride, flags, None)

    assert call(plan[:-4]) != 0 and b"truncated" in L.vfml_last_error()
    assert call(plan, n=plan.size - 1) != 0 and b"truncated" in L.vfml_last_error()
    assert call(plan[:5]) != 0 and b"header" in L.vfml_last_error()
    assert call(plan, hh=20) != 0 and b"outside the 128 x 20 image" in L.vfml_last_error()
    assert call(plan, ww=100, stride=300) != 0 and b"outside" in L.vfml_last_error()
    bad = plan.copy()
    bad[vtext.PLAN_HEADER + 4] = int(plan[5])                              # a box whose operations end past the list
    assert call(bad) != 0 and b"operations" in L.vfml_last_error()
    bad = plan.copy()
    bad[6] += 1                                                            # one glyph more than the plan holds
    assert call(bad) != 0 and b"truncated" in L.vfml_last_error()
    two = vtext.build_plan(oracle.side_by_side_ops(48, 128, 2), 96, 256)
    bad = two.copy()
    bad[vtext.PLAN_HEADER + vtext.BOX_WORDS:vtext.PLAN_HEADER + vtext.BOX_WORDS + 4] = bad[vtext.PLAN_HEADER:vtext.PLAN_HEADER + 4]
    assert call(bad, hh=96, ww=256, stride=768, image=np.zeros((96, 768), np.uint8)) != 0
    assert b"intersect" in L.vfml_last_error() or b"block" in L.vfml_last_error()
    assert call(plan, stride=3 * w - 1) != 0 and b"stride" in L.vfml_last_error()
    assert call(plan, flags=1) != 0 and b"flags" in L.vfml_last_error()      # VFML_COMPOSE_BGR is not text_draw's
    assert call(plan, image=None) != 0
    assert L.vfml_text_draw(None, 8, img.ctypes.data_as(ctypes.c_void_p), h, w, 3 * w, 0, None) != 0
    # a well-formed plan without its device copy is refused as well: still nothing launched, nothing written
    assert plan[2] == 0 and plan[3] == 0
    assert call(plan) != 0 and b"device copy" in L.vfml_last_error()
    assert not img.any()
    assert "vfml_text_draw" in hip.EXPORTS
