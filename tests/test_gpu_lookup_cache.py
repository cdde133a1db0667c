"""The bidirectional lookup with a patch cache (csrc/flow_ops.hip, vfml_corr_lookup_indirect_bidir_cached, which launches
corr_lookup_fixed_kernel with CACHED set): a query whose eight window origins are the ones its cache
row was gathered at reads the patch back instead of gathering it again.

Oracle: the uncached vfml_corr_lookup_indirect_bidir on the same inputs - the same kernel body without the cache steps,
which mixes the same LDS patch - so the comparison is BYTE equality of the whole output buffer, pad channels and rows
outside a launch's range (which hold a sentinel) included.  Which queries hit is pinned per query, not only counted: after
a fill the volumes are overwritten with a NaN pattern, so a query that gathers again shows the pattern's output and one
that hits the original's.

Geometry: the on-demand tests' - a 30 x 38 map in 4 x 8 tiles (1280 volume rows), M = 2 centres, both directions: 4 560
queries, 1 140 blocks of four waves.  Every case runs for radius 4 and 3 and for every volume form the dispatcher has a
kernel for: f32, f16 from level 3 (the shipped plan), from level 2, from level 1, and all f16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, L, M = 30, 38, 4, 2
Pn = H * W
NAN_BITS = 0x7FC0BEEF      # f32 volumes overwritten / buffers nobody may write
NAN_HALF = 0x7E00
VOL_FMTS = ("f32", "f16@3", "f16@2", "f16@1", "f16")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _origins(coords, R):
    """window_origin of every level restated on the CPU: coords [M * Pn][4] -> int64 [2 (direction)][M * Pn][L][2 (x, y)],
    the layout of the key buffer.  NaN clamps to the lower bound, as fmaxf(floorf(NaN), -65536) does."""
    c = coords.detach().cpu().numpy().astype(np.float32).reshape(M * Pn, 2, 2)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            v = np.floor(c * np.float32(2.0 ** -l))
            v = np.where(np.isnan(v), np.float32(-65536.0), np.clip(v, np.float32(-65536.0), np.float32(65536.0)))
            out.append(v.astype(np.int64) - R)
    return np.stack(out, 2).transpose(1, 0, 2, 3)


def _same(a, b):
    """[2][M * Pn] bool: the queries whose eight origins agree"""
    return (a == b).all(axis=(2, 3))


class _Setup:
    def __init__(self, R, vol):
        from vfml import hip
        from vfml.network import cor_pad
        self.hip, self.R = hip, R
        g = torch.Generator(device="cuda").manual_seed(7100 + R)
        self.vt = vt = hip.VolTile(2, 3)
        self.hl, self.wl = [H >> l for l in range(L)], [W >> l for l in range(L)]
        self.Pv = vt.count(H, W)
        self.ld = [(vt.count(self.hl[l], self.wl[l]) + 31) // 32 * 32 + 32 for l in range(L)]
        mask = {"f32": 0, "f16@3": 8, "f16@2": 12, "f16@1": 14, "f16": 15}[vol]
        self.half = [bool((mask >> l) & 1) for l in range(L)]
        self.vf = hip.FMT_F32 if mask == 0 else (hip.FMT_F16 if mask == 15 else hip.vol_f16_levels(mask))

        def pyramids():
            out = []
            for _ in range(2 * M):                              # direction-major: f of centres 0, 1, then b
                lv = []
                for l in range(L):
                    v = torch.randn(self.Pv * self.ld[l], generator=g, device="cuda")
                    lv.append(v.half() if self.half[l] else v)
                out.append(lv)
            return out
        self.A, self.B = pyramids(), pyramids()
        self.work = [[v.clone() for v in lv] for lv in self.A]   # what a test may overwrite
        self.tab = {k: self._table(p) for k, p in (("A", self.A), ("B", self.B), ("work", self.work))}
        self.nout = L * (2 * R + 1) ** 2
        self.cor_p = {hip.FMT_S16: cor_pad(self.nout, True), hip.FMT_F32: cor_pad(self.nout, False)}
        self.psz = 4 * (2 * R + 2) ** 2
        self.patches = torch.empty(2 * M * Pn * self.psz, device="cuda")
        self.keys = torch.empty(2 * M * Pn * 8, dtype=torch.int32, device="cuda")
        self.counter = torch.zeros(2, dtype=torch.int32, device="cuda")
        self._oracle = {}
        self.base = self._base_coords()
        torch.cuda.synchronize()

    def _table(self, pyrs):
        tab = torch.zeros(64, dtype=torch.int64, device="cuda")
        self.hip.ptr_table_set(tab, [v for lv in pyrs for v in lv])
        return tab

    def _base_coords(self):
        """the grid plus flows of a cell or two, a displaced block, windows over every image edge"""
        g = torch.Generator().manual_seed(11)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xs, ys, xs, ys], -1).reshape(1, Pn, 4).repeat(M, 1, 1)
        c = (grid + (torch.rand(M, Pn, 4, generator=g) - 0.5) * 3.0).view(M, H, W, 4)
        c[0, 8:20, 10:24] += torch.tensor([12.3, -11.6, -12.7, 11.2])
        c[1, 0:3, :, 1] -= 6.6
        c[1, -3:, :, 3] += 7.4
        c[0, :, 0:2, 0] -= 5.5
        c[0, :, -2:, 2] += 6.5
        return c.reshape(-1).cuda().contiguous()

    def refraction(self, coords, seed):
        """the same cells, other fractions: floor(c) + [0, 0.99)"""
        g = torch.Generator().manual_seed(seed)
        return (torch.floor(coords.cpu()) + torch.rand(coords.numel(), generator=g) * 0.99).cuda().contiguous()

    def reset(self):
        """empty keys; patches hold a pattern that no gather leaves"""
        self.keys.fill_(self.hip.LOOKUP_KEY_NONE)
        _bits(self.patches).fill_(NAN_BITS)

    def poison(self):
        for lv in self.work:
            for v in lv:
                (v.view(torch.int16).fill_(NAN_HALF) if v.dtype == torch.float16 else _bits(v).fill_(NAN_BITS))

    def restore(self):
        for lw, la in zip(self.work, self.A):
            for w, a in zip(lw, la):
                w.copy_(a)

    def new_out(self, fmt):
        return torch.full((M * Pn * 2 * self.cor_p[fmt],), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)

    def launch(self, coords, tab, cached=True, n=M, c0=0, store=True, fmt=None, out=None):
        """-> (the whole output buffer, hits, misses)"""
        hip = self.hip
        fmt = hip.FMT_S16 if fmt is None else fmt
        out = self.new_out(fmt) if out is None else out
        cor_p, r0 = self.cor_p[fmt], c0 * Pn
        self.counter.zero_()
        cache = (self.patches, self.keys, M * Pn, store, self.counter) if cached else None
        hip.corr_lookup(None, self.hl, self.wl, self.ld, self.R, Pn, coords, r0 * 4, 4, out, r0 * 2 * cor_p, 2 * cor_p, out_fmt=fmt,
                        table=self.tab[tab][c0 * L:], nmaps=n, vol_fmt=self.vf, vol_tile=self.vt.code, bidir=(2, cor_p, M),
                        cache=cache[:3] + (r0,) + cache[3:] if cache else None)
        hits, misses = self.counter.tolist()
        return out, hits, misses

    def oracle(self, name, coords, tab, fmt=None):
        """the uncached launch over every row, computed once per (name, table, format)"""
        key = (name, tab, fmt)
        if key not in self._oracle:
            self._oracle[key] = _bits(self.launch(coords, tab, cached=False, fmt=fmt)[0]).clone()
        return self._oracle[key]

    def keys_now(self):
        return self.keys.cpu().numpy().astype(np.int64).reshape(2, M * Pn, L, 2)


@pytest.fixture(scope="module", params=[(R, v) for R in (4, 3) for v in VOL_FMTS], ids=lambda p: f"R{p[0]}-{p[1]}")
def setup(gpu, request):
    return _Setup(*request.param)


@pytest.fixture
def s(setup):
    setup.restore()
    setup.reset()
    return setup


def _rows(n, c0, cor_p):
    """the floats of a whole output buffer that a launch on centres c0 .. c0 + n - 1 owns"""
    m = torch.zeros(M * Pn, 2 * cor_p, dtype=torch.bool, device="cuda")
    m[c0 * Pn:(c0 + n) * Pn] = True
    return m.view(-1)


def test_fill_then_repeat(s):
    for fmt in (s.hip.FMT_S16, s.hip.FMT_F32):
        s.reset()
        ref = s.oracle("base", s.base, "A", fmt)
        out, hits, misses = s.launch(s.base, "A", fmt=fmt)
        assert (hits, misses) == (0, 2 * M * Pn) and torch.equal(_bits(out), ref)
        assert (s.keys_now() == _origins(s.base, s.R)).all()
        out, hits, misses = s.launch(s.base, "A", fmt=fmt)
        assert (hits, misses) == (2 * M * Pn, 0) and torch.equal(_bits(out), ref)


def test_same_origin_new_fraction(s):
    s.launch(s.base, "A")
    moved = s.refraction(s.base, 21)
    assert _same(_origins(moved, s.R), _origins(s.base, s.R)).all() and not torch.equal(moved, s.base)
    out, hits, misses = s.launch(moved, "A")
    assert (hits, misses) == (2 * M * Pn, 0)
    assert torch.equal(_bits(out), s.oracle("refraction21", moved, "A"))


def test_the_cache_is_what_is_read(s):
    s.launch(s.base, "work")
    s.poison()
    moved = s.refraction(s.base, 22)
    out, hits, misses = s.launch(moved, "work")
    assert (hits, misses) == (2 * M * Pn, 0)
    assert torch.equal(_bits(out), s.oracle("refraction22", moved, "A"))      # (A: what `work` held at the fill)
    assert not torch.equal(_bits(out), _bits(s.launch(moved, "work", cached=False)[0]))


def _moves(s):
    """base with eight kinds of move, each on its own queries -> (coords, [2][M * Pn] bool: the queries that moved)"""
    c = s.refraction(s.base, 23).cpu().view(M, H, W, 4).clone()
    b = c.clone()
    c[0, 2, 3:9, 0] += 1.0                                        # x alone across an integer (forward queries)
    c[0, 4, 3:9, 3] += 1.0                                        # y alone (backward queries)
    c[1, 6, 3:9, 0] = torch.floor(c[1, 6, 3:9, 0]) - 0.25         # a negative step
    c[1, 8, 3:9, 2] = 70000.0                                     # (outside: level 0 clamped at 65536, level 1 at 35000)
    c[1, 10, 3:9] = torch.tensor([-20.5, -30.25, W + 15.5, H + 21.75])     # outside the image
    c[0, 12, 3:6] = torch.tensor([float("inf"), 3.5, 4.5, float("-inf")])
    c[0, 14, 3:6] = torch.tensor([float("nan"), 3.5, 4.5, float("nan")])
    c[0, 16, 3:6] = torch.tensor([1e30, 3.5, 4.5, -1e30])
    even = torch.floor(b[1, 20, 3:9, 1]) % 2 == 0                 # level 0 alone: an even cell's upper neighbour
    c[1, 20, 3:9, 1] += even.float()
    moved = ~_same(_origins(c.reshape(-1), s.R), _origins(b.reshape(-1), s.R))
    return c.reshape(-1).cuda().contiguous(), b.reshape(-1).cuda().contiguous(), moved


def test_moves_miss_and_the_rest_hits(s):
    c, b, moved = _moves(s)
    nm = int(moved.sum())
    assert 54 <= nm <= 60                                         # 4 x 6 + 2 x 6 + 3 x 3 x 2 + the even cells among six
    s.launch(b, "work")
    out, hits, misses = s.launch(c, "work")
    assert (hits, misses) == (2 * M * Pn - nm, nm)
    assert torch.equal(_bits(out), s.oracle("moves", c, "A"))
    assert (s.keys_now() == _origins(c, s.R)).all()
    # after the moves: the same coordinates hit everywhere
    out, hits, misses = s.launch(c, "work")
    assert (hits, misses) == (2 * M * Pn, 0) and torch.equal(_bits(out), s.oracle("moves", c, "A"))
    # a move that changes only a coarse level's origin: level 0 stays clamped
    d = c.clone().view(M, H, W, 4)
    d[1, 8, 3:9, 2] = 90000.0
    d = d.reshape(-1).contiguous()
    oc, od = _origins(c, s.R), _origins(d, s.R)
    coarse = ~_same(oc, od)
    assert coarse.sum() == 6 and (oc[:, :, 0] == od[:, :, 0]).all()
    out, hits, misses = s.launch(d, "work")
    assert (hits, misses) == (2 * M * Pn - 6, 6) and torch.equal(_bits(out), s.oracle("coarse", d, "A"))


def test_which_queries_gather_again(s):
    """per query: over volumes overwritten after the fill, exactly the moved queries show the overwritten values"""
    c, b, moved = _moves(s)
    s.launch(b, "work")
    s.poison()
    out, hits, misses = s.launch(c, "work")
    cor_p = s.cor_p[s.hip.FMT_S16]
    good = s.oracle("moves", c, "A").view(M * Pn, 2, cor_p)
    bad = _bits(s.launch(c, "work", cached=False)[0]).view(M * Pn, 2, cor_p)
    m = torch.from_numpy(moved.T.copy()).cuda().view(M * Pn, 2, 1)
    assert torch.equal(_bits(out).view(M * Pn, 2, cor_p), torch.where(m, bad, good))
    assert misses == int(moved.sum())


def test_reset_and_new_pyramids(s):
    s.launch(s.base, "A")
    s.keys.fill_(s.hip.LOOKUP_KEY_NONE)
    out, hits, misses = s.launch(s.base, "B")
    assert (hits, misses) == (0, 2 * M * Pn)
    assert torch.equal(_bits(out), s.oracle("base", s.base, "B"))
    assert not torch.equal(s.oracle("base", s.base, "B"), s.oracle("base", s.base, "A"))


@pytest.mark.parametrize("c0", [M - 1, 0])
def test_row_ranges(s, c0):
    """the warm iteration 0 looks up the newest centre alone, a shortened last iteration the first ones"""
    c, b, moved = _moves(s)
    s.launch(b, "work")
    s.poison()
    keys0, patches0 = s.keys.clone(), _bits(s.patches).clone()
    out, hits, misses = s.launch(c, "work", n=1, c0=c0)
    cor_p = s.cor_p[s.hip.FMT_S16]
    mine = slice(c0 * Pn, (c0 + 1) * Pn)
    nm = int(moved[:, mine].sum())
    assert nm > 0 and (hits, misses) == (2 * Pn - nm, nm)
    good = s.oracle("moves", c, "A").view(M * Pn, 2, cor_p)
    bad = _bits(s.launch(c, "work", cached=False)[0]).view(M * Pn, 2, cor_p)
    m = torch.from_numpy(moved.T.copy()).cuda().view(M * Pn, 2, 1)
    want = torch.where(m, bad, good).reshape(-1)
    own = _rows(1, c0, cor_p)
    assert torch.equal(_bits(out)[own], want[own]) and (_bits(out)[~own] == NAN_BITS).all()
    # cache and key: the range's entries follow the launch, every other row is what it was
    kown = torch.zeros(2, M * Pn, dtype=torch.bool, device="cuda")
    kown[:, mine] = True
    assert torch.equal(s.keys.view(2, M * Pn, 8)[~kown], keys0.view(2, M * Pn, 8)[~kown])
    assert torch.equal(_bits(s.patches).view(2, M * Pn, -1)[~kown], patches0.view(2, M * Pn, -1)[~kown])
    assert (s.keys_now()[:, mine] == _origins(c, s.R)[:, mine]).all()


def test_store_flag_off(s):
    c, b, moved = _moves(s)
    # on empty keys: every query is computed, nothing is kept
    out, hits, misses = s.launch(b, "work", store=False)
    assert (hits, misses) == (0, 2 * M * Pn) and torch.equal(_bits(out), s.oracle("moves_base", b, "A"))
    assert (s.keys == s.hip.LOOKUP_KEY_NONE).all() and (_bits(s.patches) == NAN_BITS).all()
    # on filled entries: the moved queries are computed, and key and patch still belong together afterwards
    s.launch(b, "work")
    keys0, patches0 = s.keys.clone(), _bits(s.patches).clone()
    out, hits, misses = s.launch(c, "work", store=False)
    nm = int(moved.sum())
    assert (hits, misses) == (2 * M * Pn - nm, nm) and torch.equal(_bits(out), s.oracle("moves", c, "A"))
    assert torch.equal(s.keys, keys0) and torch.equal(_bits(s.patches), patches0)
    s.poison()
    back = s.refraction(b, 24)
    out, hits, misses = s.launch(back, "work")
    assert (hits, misses) == (2 * M * Pn, 0) and torch.equal(_bits(out), s.oracle("refraction24", back, "A"))
