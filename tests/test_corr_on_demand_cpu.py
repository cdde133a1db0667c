"""vfml_corr_level0_ensure without a GPU: argument validation returns before any launch, and the bitmap's size rule."""
import ctypes


def test_ensure_validates_its_arguments_without_a_gpu():
    from vfml import hip
    L = hip.lib()
    assert L.vfml_corr_level0_ensure(None, None, None, 256, 16.0, hip.FMT_S16, hip.FMT_F32, 0, None, 1, 2, 1, None, 4, 2,
                                     30, 38, 4, 2 + 16 * 3, None, None) != 0
    assert b"vfml_corr_level0_ensure" in L.vfml_last_error()
    # a level-0 call that is not the GEMM form's resident-A walk (plain f32 rows) is refused, not run some other way
    d = hip.ConvDesc()
    d.in0, d.c0, d.ld0, d.n, d.h, d.w = 64, 256, 256, 1, 1, 1280
    d.cout, d.kh, d.kw, d.stride, d.out, d.ldo, d.out_scale = 1280, 1, 1, 1, 64, 1312, 1.0
    d.flags = hip.CONV_MFMA1
    assert L.vfml_corr_level0_ensure(ctypes.byref(d), 64, 128, 256, 16.0, hip.FMT_F32, hip.FMT_F32, 0, 64, 1, 2, 1, 64, 4, 2,
                                     30, 38, 4, 2 + 16 * 3, None, None) != 0
    assert b"resident-A walk" in L.vfml_last_error()
    # rows / columns that are not the tiled level image
    assert L.vfml_corr_level0_ensure(ctypes.byref(d), 64, 128, 256, 16.0, hip.FMT_S16, hip.FMT_F32, 0, 64, 1, 2, 1, 64, 4, 2,
                                     31, 41, 4, 2 + 16 * 3, None, None) != 0
    assert b"tiled" in L.vfml_last_error()


def test_bitmap_words():
    from vfml import hip
    assert hip.corr_bitmap_words(32640, 32640) == 255 * 16        # 1080p: 255 row tiles x 510 column tiles
    assert hip.corr_bitmap_words(1280, 1280) == 10
    assert hip.corr_bitmap_words(129, 65) == 2
