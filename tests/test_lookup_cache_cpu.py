"""The cached bidirectional lookup (vfml_corr_lookup_indirect_bidir_cached) refuses what it cannot
run before any launch: no GPU is needed to see that."""
import ctypes


def test_argument_validation_needs_no_gpu():
    from vfml import hip
    L = hip.lib()
    assert "vfml_corr_lookup_indirect_bidir_cached" in hip.EXPORTS
    assert hip.LOOKUP_KEY_NONE == -2 ** 31
    # never dereferenced: every call below is refused
    T, C, O, P, K = 0x10000, 0x20000, 0x40000, 0x80000, 0x100000
    i32 = ctypes.c_int32
    h, w = 30, 38
    Pn = h * w

    def call(table=T, levels=4, radius=4, nmaps=2, coords=C, out=O, ld_out=656, dir_tab=2, out_fmt=hip.FMT_S16,
             vol_fmt=hip.FMT_F32, cache=P, key=K, rows=2 * Pn, row0=0, store=1, counter=None):
        hl = (i32 * 6)(*[h >> l for l in range(4)], 0, 0)
        wl = (i32 * 6)(*[w >> l for l in range(4)], 0, 0)
        ld = (i32 * 6)(*[(h >> l) * (w >> l) for l in range(4)], 0, 0)
        return L.vfml_corr_lookup_indirect_bidir_cached(table, hl, wl, ld, levels, radius, nmaps, Pn, coords, 4, 2, out, ld_out,
                                                        328, dir_tab, out_fmt, vol_fmt, 0, cache, key, rows, row0, store,
                                                        counter, None)

    for kw, text in ((dict(cache=None), b"null cache / key"), (dict(key=None), b"null cache / key"),
                     (dict(table=None), b"table"), (dict(table=T + 4), b"table"),
                     (dict(radius=2), b"radius=2"), (dict(radius=5), b"radius=5"), (dict(radius=1), b"radius=1"),
                     (dict(levels=5), b"levels=5"), (dict(levels=6), b"levels=6"), (dict(levels=0), b"out of range"),
                     (dict(cache=P + 4), b"16-byte aligned"), (dict(cache=P + 8), b"16-byte aligned"),
                     (dict(key=K + 4), b"16-byte aligned"), (dict(key=K + 8), b"16-byte aligned"),
                     (dict(rows=2 * Pn - 1), b"outside the cache"), (dict(row0=1), b"outside the cache"),
                     (dict(row0=-1), b"outside the cache"), (dict(nmaps=1, row0=Pn + 1), b"outside the cache"),
                     (dict(rows=0), b"outside the cache"), (dict(counter=0x200002), b"misaligned counter"),
                     (dict(nmaps=5), b"nmaps=5"), (dict(dir_tab=1), b"dir_tab=1"),
                     # what the uncached call refuses is refused here too
                     (dict(coords=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(out=O + 16), b"32-byte"),
                     (dict(ld_out=4), b"ld_out=4"), (dict(vol_fmt=hip.FMT_S16), b"vol_fmt"), (dict(out_fmt=7), b"out_fmt")):
        assert call(**kw) != 0, kw
        assert text in L.vfml_last_error(), (kw, L.vfml_last_error())
