"""vfml_corr_levels_ensure without a GPU: argument validation returns before any launch, and the sections of a pyramid's
bitmap buffer (one per on-demand level, level 0's first)."""
import ctypes
import types


def _level(hip, cout, ldo, hl, wl, level, out_fmt=None, rows=1280):
    d = hip.ConvDesc()
    d.in0, d.c0, d.ld0, d.n, d.h, d.w = 64, 256, 256, 1, 1, rows
    d.cout, d.kh, d.kw, d.stride, d.out, d.ldo, d.out_scale = cout, 1, 1, 1, 64, ldo, 1.0
    d.flags = hip.CONV_MFMA1
    lv = hip.CorrLevelDesc()
    lv.d = ctypes.pointer(d)
    lv.w_hi, lv.w_lo, lv.kp, lv.w_scale = 64, 128, 256, 16.0
    lv.out_fmt, lv.level, lv.h, lv.w = hip.FMT_F32 if out_fmt is None else out_fmt, level, hl, wl
    return lv, d          # (d: kept alive by the caller)


def _call(hip, lvs, n=None, in_fmt=None, cells=64, coords=64, h=30, w=38):
    arr = (hip.CorrLevelDesc * max(len(lvs), 1))(*[lv for lv, _ in lvs])
    return hip.lib().vfml_corr_levels_ensure(arr if lvs else None, len(lvs) if n is None else n,
                                             hip.FMT_S16 if in_fmt is None else in_fmt, 0, cells, 1, 2, 1, coords, 4, 2, h, w, 4,
                                             2 + 16 * 3, None, None)


def test_levels_ensure_validates_its_arguments_without_a_gpu():
    from vfml import hip
    L = hip.lib()
    name = b"vfml_corr_levels_ensure"
    # the 30 x 38 query map in 4 x 8 tiles: 1280 rows; its level 0 has 1280 columns, its level 1 (15 x 19) has 320
    lv0 = _level(hip, 1280, 1312, 30, 38, 0)
    assert _call(hip, []) != 0 and name in L.vfml_last_error()                       # null level list
    assert _call(hip, [lv0], cells=None) != 0 and name in L.vfml_last_error()        # null cells
    assert _call(hip, [lv0], coords=None) != 0 and name in L.vfml_last_error()       # null coordinates
    assert _call(hip, [lv0], n=0) != 0 and name in L.vfml_last_error()
    assert _call(hip, [lv0], n=4) != 0 and name in L.vfml_last_error()               # more levels than a launch takes
    nod = hip.CorrLevelDesc()
    assert _call(hip, [(nod, None)]) != 0 and name in L.vfml_last_error()            # a level without its call
    # a level below 1024 columns is not a call of the resident-A walk: refused, not run some other way
    assert _call(hip, [lv0, _level(hip, 320, 352, 15, 19, 1)]) != 0
    assert name in L.vfml_last_error() and b"resident-A walk" in L.vfml_last_error()
    # so is a level stored as f16
    assert _call(hip, [_level(hip, 1280, 1344, 30, 38, 0, out_fmt=hip.FMT_F16)]) != 0
    assert name in L.vfml_last_error() and b"resident-A walk" in L.vfml_last_error()
    # and plain f32 query rows
    assert _call(hip, [lv0], in_fmt=hip.FMT_F32) != 0 and b"resident-A walk" in L.vfml_last_error()
    # columns that are not the tiled level image; rows that are not the tiled query map; levels out of order
    assert _call(hip, [_level(hip, 1280, 1312, 31, 41, 0)]) != 0 and b"tiled" in L.vfml_last_error()
    assert _call(hip, [lv0], h=31, w=41) != 0 and b"tiled" in L.vfml_last_error()
    assert _call(hip, [_level(hip, 1280, 1312, 30, 38, 1), lv0]) != 0 and b"ascending" in L.vfml_last_error()


def test_bitmap_sections():
    from vfml import hip
    from vfml.network import MOFNetHIP
    geo = types.SimpleNamespace(Pv=32640, Nl=[32640, 8640, 2400, 512])              # 1080p
    at, total = MOFNetHIP._bitmap_sections(geo, (0, 1, 2))
    # 255 row tiles x (510 -> 16, 135 -> 5, 37.5 -> 38 -> 2) words
    assert at == {0: 0, 1: 255 * 16, 2: 255 * 21} and total == 255 * 23
    assert MOFNetHIP._bitmap_sections(geo, (0,)) == ({0: 0}, hip.corr_bitmap_words(32640, 32640))
    assert MOFNetHIP._bitmap_sections(geo, (0, 2)) == ({0: 0, 2: 255 * 16}, 255 * 18)
    assert hip.corr_bitmap_words(5152, 1056) == 41 * 1 and hip.corr_bitmap_words(5152, 5152) == 41 * 3
