"""The uint8 picture resize on the host: the --fast dimension rule against its hand-derived table,
video.resize_frame against the numpy restatement (tests/resize_oracle.py) byte for byte, the properties that let the
definition go without a clip, and the launcher's argument checks (no GPU needed: nothing is launched on error)."""
import ctypes

import numpy as np
import pytest

import resize_oracle as ro

# source WxH -> (w, h, scale), derived by hand from the rule
DIMENSIONS = [
    ((1920, 1080), (256, 144, 2 / 15)), ((3840, 2160), (256, 144, 1 / 15)), ((1280, 720), (256, 144, 0.2)),
    ((640, 480), (160, 120, 0.25)), ((400, 300), (200, 150, 0.5)), ((512, 512), (256, 256, 0.5)),
    ((513, 300), (128, 74, 0.25)), ((300, 100), (150, 64, 0.5)), ((256, 256), (256, 256, 1.0)),
    ((200, 40), (200, 64, 1.0)), ((320, 200), (160, 100, 0.5)), ((262, 131), (130, 64, 0.5)),
    ((258, 258), (128, 128, 0.5)), ((1000, 90), (250, 64, 0.25)), ((700, 1030), (172, 256, 256 / 1030)),
]

# source HxW -> hxw: the shapes the device tests run (tests/test_gpu_resize.py)
SHAPES = [
    ((200, 320), (100, 160)),       # 2x2, the CLI case
    ((66, 130), (33, 65)),          # 2x2, odd destination
    ((131, 262), (64, 130)),        # near 2, must be separable
    ((64, 88), (16, 22)),           # exact 4
    ((100, 300), (64, 150)),        # anisotropic: x exactly 2, y not
    ((31, 45), (64, 90)),           # enlargement, both edge clamps
    ((50, 37), (50, 64)),           # one axis unchanged
    ((1080, 1920), (144, 256)),     # the headline size
]
IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES]


def pictures(shape, seed=0):
    """name -> uint8 [H,W,3]: random bytes, all 0, all 255."""
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, shape + (3,), dtype=np.uint8), "zeros": np.zeros(shape + (3,), np.uint8),
            "full": np.full(shape + (3,), 255, np.uint8)}


_EXPECTED = {}


def expected(src, dst, name, seed=0):
    """The oracle's result for a picture of `pictures`, computed once and shared (read-only)."""
    key = (src, dst, name, seed)
    if key not in _EXPECTED:
        out = ro.resize(pictures(src, seed)[name], dst)
        out.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


@pytest.mark.parametrize("source, want", DIMENSIONS, ids=[f"{s[0]}x{s[1]}" for s, _ in DIMENSIONS])
def test_fast_mode_dimension_table(source, want):
    from video import FrameExtractor, fast_mode_dimensions
    for got in (fast_mode_dimensions(*source), ro.fast_mode_dimensions(*source)):
        assert got[:2] == want[:2] and got[2] == pytest.approx(want[2], rel=1e-15), (source, got)
        assert got[0] % 2 == 0 and got[1] % 2 == 0 and min(got[:2]) >= 64
    ex = FrameExtractor.__new__(FrameExtractor)
    ex.fast_mode = True
    assert ex.calculate_fast_mode_dimensions(*source) == fast_mode_dimensions(*source)
    ex.fast_mode = False
    assert ex.calculate_fast_mode_dimensions(*source) == (source[0], source[1], 1.0)


@pytest.mark.parametrize("src, dst", SHAPES, ids=IDS)
def test_resize_frame_equals_the_oracle(src, dst):
    from video import resize_frame
    for name, img in pictures(src).items():
        got = resize_frame(img, (dst[1], dst[0]))
        assert got.dtype == np.uint8 and got.shape == dst + (3,)
        np.testing.assert_array_equal(got, expected(src, dst, name), err_msg=name)


@pytest.mark.parametrize("src, dst", SHAPES, ids=IDS)
def test_definition_needs_no_clip(src, dst):
    """Every weight pair sums to 2048, an all-255 picture stays 255, and the value before the cast stays in 0..255."""
    from vfml.hip import resize_tables
    for S, D in ((src[0], dst[0]), (src[1], dst[1])):
        s, s1, a0, a1 = ro.taps(S, D)
        assert np.all(a0 + a1 == 2048) and a0.min() >= 0 and a1.min() >= 0
        assert s.min() >= 0 and s1.max() <= S - 1 and np.all((s1 == s + 1) | (s1 == S - 1))
        tab = resize_tables(S, D)
        assert tab.dtype == np.int32 and tab.shape == (D, 4) and not tab.flags.writeable
        np.testing.assert_array_equal(tab, np.stack([s, s1, a0, a1], axis=1))
        assert resize_tables(S, D) is tab                    # cached
    imgs = pictures(src)
    assert np.all(ro.resize_values(imgs["full"], dst) == 255)
    assert np.all(ro.resize_values(imgs["zeros"], dst) == 0)
    v = ro.resize_values(imgs["random"], dst)
    assert v.min() >= 0 and v.max() <= 255


def test_own_size_returns_the_picture_unchanged():
    from video import resize_frame
    img = pictures((37, 53), seed=3)["random"]
    np.testing.assert_array_equal(resize_frame(img, (53, 37)), img)
    np.testing.assert_array_equal(ro.resize(img, (37, 53)), img)


def test_2x2_mean_only_when_both_axes_halve_exactly():
    from video import resize_frame
    img = pictures((100, 300), seed=4)["random"]
    x = img.astype(np.int64)
    mean = ((x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    np.testing.assert_array_equal(resize_frame(img, (150, 50)), mean)                    # both exactly 2
    np.testing.assert_array_equal(ro.resize(img, (50, 150)), mean)
    # x exactly 2, y not: the separable form, written out here with the taps
    got = resize_frame(img, (150, 64))
    xs, xs1, a0, a1 = ro.taps(300, 150)
    ys, ys1, b0, b1 = ro.taps(100, 64)
    want = np.empty((64, 150, 3), np.uint8)
    for y in range(64):
        for c in range(3):
            r0 = x[ys[y], xs, c] * a0 + x[ys[y], xs1, c] * a1
            r1 = x[ys1[y], xs, c] * a0 + x[ys1[y], xs1, c] * a1
            want[y, :, c] = (((b0[y] * (r0 >> 4)) >> 16) + ((b1[y] * (r1 >> 4)) >> 16) + 2) >> 2
    np.testing.assert_array_equal(got, want)


def test_resize_frame_rejects_what_is_not_a_picture():
    from video import resize_frame
    with pytest.raises(ValueError):
        resize_frame(np.zeros((8, 8, 3), np.float32), (4, 4))
    with pytest.raises(ValueError):
        resize_frame(np.zeros((8, 8), np.uint8), (4, 4))
    with pytest.raises(ValueError):
        resize_frame(np.zeros((8, 8, 3), np.uint8), (0, 4))


def test_launcher_rejects_bad_arguments_without_a_gpu():
    from vfml import hip
    L = hip.lib()
    p, q, t = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)

    def call(src=p, n=1, H=8, W=8, ss=192, dst=q, h=3, w=5, ds=45, xt=t, yt=t):
        return L.vfml_resize_u8(src, n, H, W, ss, dst, h, w, ds, xt, yt, None)
    assert call(src=None) != 0 and b"null" in L.vfml_last_error()
    assert call(dst=None) != 0
    assert call(n=0) != 0 and b"bad size" in L.vfml_last_error()
    assert call(h=0) != 0 and call(W=-1) != 0
    assert call(W=40000, ss=3 * 8 * 40000) != 0 and b"too large" in L.vfml_last_error()
    assert call(ss=191) != 0 and b"stride" in L.vfml_last_error()
    assert call(ds=44) != 0
    assert call(xt=None) != 0 and b"table" in L.vfml_last_error()
    assert call(yt=ctypes.c_void_p((3 << 20) + 4)) != 0 and b"aligned" in L.vfml_last_error()


def test_composer_resizes_a_flow_picture_of_another_size():
    from video import resize_frame
    from visualization.video_composer import create_side_by_side
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    full = resize_frame(small, (64, 48))
    assert full.shape == frame.shape
    taa = rng.random((48, 64, 3)).astype(np.float32) * 255
    for kw in ({}, {"flow_only": True}, {"taa_frame": taa, "taa_simple_frame": taa}):
        np.testing.assert_array_equal(create_side_by_side(frame, small, **kw), create_side_by_side(frame, full, **kw))
