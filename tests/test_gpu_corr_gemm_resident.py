"""The resident-A walk of the persistent GEMM form (csrc/conv_gemm_split.hip, SplitPlan::resident): a 1x1 over one
split-row source with one MFMA per product over 64-channel steps and K <= 256 keeps its row tile in LDS across a run
of column tiles and fetches the other operand a whole column tile ahead.

Oracle: the streaming walk, which every such call with K > 256 still takes.  The same problem at K = 320, with source
channels K..319 zero and the weight rows extended by arbitrary values, runs the same MFMAs on the same operands in the
same K order from a zeroed accumulator and then adds exact zeros, so the resident walk's output at K must be BYTE-equal
to it (seeded normal data: no sum is exactly -0).  All calls go through the C ABI (hip.conv2d), operands are seeded
split rows and two-plane weights of which the one-MFMA product reads the hi plane.

Case c runs with VFML_FMT_F16 outputs: a plain-f32 output of 132 columns is below the GEMM form's minimum width and
would not reach either walk.  Case d's K + 64 comparison runs the resident walk on both sides when K + 64 <= 256, so
the streaming oracle of every case is the K = 320 problem; the K + 64 problem is checked against it as well."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = 320             # K of the streaming oracle: five 64-channel steps, beyond what the resident walk holds
SC = 16.0            # both operands carry x16 (weight lo halves normal), undone by out_scale
TOL = 5e-6           # CONV_TOL["f16x3"] of tests/test_gpu_kernels.py: what its persistent-GEMM tests ask of one-term products


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _f16(t):
    return t.half().double()


class _Problem:
    """f1 [M][K], f2 [cout][K] seeded; device operands at K and zero-extended / arbitrarily extended to `kpad`."""

    def __init__(self, seed, M, cout, K, gpu):
        g = torch.Generator().manual_seed(seed)
        self.M, self.cout, self.K, self.gpu = M, cout, K, gpu
        self.f1 = torch.randn(M, K, generator=g)
        self.f2 = torch.randn(cout, K, generator=g)
        self.ext = torch.randn(cout, KS - K, generator=g)

    def rows(self, kpad):
        from vfml import hip
        f = torch.cat([self.f1, torch.zeros(self.M, kpad - self.K)], 1) if kpad > self.K else self.f1
        t = torch.empty(f.numel(), device=self.gpu)
        hip.to_s16((f * SC).cuda().reshape(-1), self.M, kpad, kpad, t, kpad)
        return t

    def planes(self, kpad):
        from vfml import hip
        f = torch.cat([self.f2, self.ext[:, :kpad - self.K]], 1) if kpad > self.K else self.f2
        return hip.SplitWeight(self.cout, kpad, torch.device("cuda")).fill(f.cuda().reshape(-1).contiguous(), scale=SC)

    def emu(self):
        """float64 product of the f16-rounded operands: what one MFMA per product computes, up to f32 accumulation"""
        return ((_f16(self.f1 * SC) / SC).cuda() @ (_f16(self.f2 * SC) / SC).cuda().t() / 16.0)


def _gemm(p, kpad, *, f16=False, twin=False, bias=None, out_scale=1.0 / 16.0 / SC, margin=0, fill=7.0, fill_t=9.0):
    """out [M][ld] (and out_t [cout][ldt]) of the problem at K = kpad, inside canary-filled buffers with `margin`
    elements in front and behind; returns (whole out buffer, whole out_t buffer or None, ld, ldt)"""
    from vfml import hip
    dt = torch.float16 if f16 else torch.float32
    ld, ldt = (p.cout + 31) // 32 * 32, (p.M + 31) // 32 * 32
    out = torch.full((2 * margin + p.M * ld,), fill, dtype=dt, device=p.gpu)
    out_t = torch.full((2 * margin + p.cout * ldt,), fill_t, dtype=dt, device=p.gpu) if twin else None
    per = 2 if f16 else 1                      # elements per float of storage
    hip.conv2d(p.rows(kpad), kpad, kpad, 1, 1, p.M, p.planes(kpad), bias, p.cout, 1, 1, out.view(torch.float32), ld,
               out_off=margin // per, out_scale=out_scale, in_fmt=hip.FMT_S16, out_fmt=hip.FMT_F16 if f16 else hip.FMT_F32,
               out_t=out_t.view(torch.float32) if twin else None, ld_out_t=ldt if twin else 0, out_t_off=margin // per, mfma=1)
    return out, out_t, ld, ldt


def _inner(buf, margin, rows, ld):
    return buf[margin:margin + rows * ld].view(rows, ld)


def test_long_walks_f32_with_transposed_twin(gpu):
    """Case a (seed 101): 17 row tiles (the last of 4 rows) x 257 column tiles of 64 (the last of 8 columns) = 4369 tiles
    on 512 resident workgroups: runs of 9 column tiles per staged row tile (the last run shorter), ragged tiles in both
    directions, ld_out_t > M."""
    p = _Problem(101, 2052, 16392, 256, gpu)
    out, out_t, ld, ldt = _gemm(p, 256, twin=True)
    ref, ref_t, _, _ = _gemm(p, KS, twin=True)
    assert ldt > p.M
    assert torch.equal(_bits(out), _bits(ref))             # canary columns past cout included
    assert torch.equal(_bits(out_t), _bits(ref_t))
    got, got_t = out.view(p.M, ld), out_t.view(p.cout, ldt)
    assert torch.equal(_bits(got_t[:, :p.M]), _bits(got[:, :p.cout].t()))     # the same accumulators, stored twice
    assert (got[:, p.cout:] == 7.0).all() and (got_t[:, p.M:] == 9.0).all()
    assert _rel_err(got[:300, :p.cout].double(), p.emu()[:300]) < TOL


def test_f16_output_with_bias_and_scale(gpu):
    """Case b (seed 102): VFML_FMT_F16 output, no twin, bias and out_scale != 1; 9 row tiles x 9 column tiles."""
    p = _Problem(102, 1028, 520, 256, gpu)
    b = torch.randn(520, generator=torch.Generator().manual_seed(1020)).cuda()
    out, _, ld, _ = _gemm(p, 256, f16=True, bias=b, out_scale=1.0 / 64.0 / SC)
    ref, _, _, _ = _gemm(p, KS, f16=True, bias=b, out_scale=1.0 / 64.0 / SC)
    assert torch.equal(_bits(out), _bits(ref))
    want = (p.emu() * 16.0 + b.double() / SC) / 64.0      # (the bias is added to the x16 sums)
    assert _rel_err(out.view(p.M, ld)[:, :p.cout].double(), want) < 1e-3      # f16 rounding of the stored value
    assert (out.view(p.M, ld)[:, p.cout:] == 7.0).all()


def test_fewer_tiles_than_workgroups_writes_nothing_outside(gpu):
    """Case c (seed 103): one ragged row tile, three column tiles (the last of 4 columns); canary margins around out and
    out_t stay untouched.  VFML_FMT_F16 outputs (see the module docstring)."""
    p = _Problem(103, 36, 132, 256, gpu)
    margin = 4096
    out, out_t, ld, ldt = _gemm(p, 256, f16=True, twin=True, margin=margin)
    ref, ref_t, _, _ = _gemm(p, KS, f16=True, twin=True, margin=margin)
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(_bits(out_t), _bits(ref_t))
    assert (out[:margin] == 7.0).all() and (out[margin + p.M * ld:] == 7.0).all()
    assert (out_t[:margin] == 9.0).all() and (out_t[margin + p.cout * ldt:] == 9.0).all()
    got, got_t = _inner(out, margin, p.M, ld), _inner(out_t, margin, p.cout, ldt)
    assert (got[:, p.cout:] == 7.0).all() and (got_t[:, p.M:] == 9.0).all()
    assert torch.equal(_bits(got_t[:, :p.M]), _bits(got[:, :p.cout].t()))
    assert _rel_err(got[:, :p.cout].double(), p.emu()) < 1e-3


@pytest.mark.parametrize("K", [128, 192])
def test_shorter_k(gpu, K):
    """Case d (seeds 104 + K): two steps, and three rounded up to four by a zero step; against the streaming walk
    (K = 320, zero-padded), against the K + 64 zero-padded problem, and against the float64 product."""
    p = _Problem(104 + K, 260, 1032, K, gpu)
    out, out_t, ld, ldt = _gemm(p, K, twin=True)
    ref, ref_t, _, _ = _gemm(p, KS, twin=True)
    mid, mid_t, _, _ = _gemm(p, K + 64, twin=True)
    assert torch.equal(_bits(out), _bits(ref)) and torch.equal(_bits(out_t), _bits(ref_t))
    assert torch.equal(_bits(mid), _bits(ref)) and torch.equal(_bits(mid_t), _bits(ref_t))
    assert _rel_err(out.view(p.M, ld)[:, :p.cout].double(), p.emu()) < TOL


def test_source_at_an_offset_inside_a_wider_buffer(gpu):
    """Case e (seed 105): the source is rows 5.. / channels 64.. of a wider split-row buffer (a frame inside a window
    buffer: nonzero in0_off, row stride > K)."""
    from vfml import hip
    p = _Problem(105, 516, 1100, 256, gpu)
    LD, R0, C0 = 384, 5, 64
    buf = torch.zeros((R0 + p.M) * LD, device=gpu)         # channels C0 + 256 .. C0 + 319 of every row stay zero
    hip.to_s16((p.f1 * SC).cuda().reshape(-1), p.M, 256, 256, buf, LD, dst_off=R0 * LD + C0)
    ld, ldt = (p.cout + 31) // 32 * 32, (p.M + 31) // 32 * 32
    res = []
    for k in (256, KS):
        out = torch.full((p.M * ld,), 7.0, device=gpu)
        out_t = torch.full((p.cout * ldt,), 9.0, device=gpu)
        hip.conv2d(buf, k, LD, 1, 1, p.M, p.planes(k), None, p.cout, 1, 1, out, ld, in0_off=R0 * LD + C0,
                   out_scale=1.0 / 16.0 / SC, in_fmt=hip.FMT_S16, out_t=out_t, ld_out_t=ldt, mfma=1)
        res.append((out, out_t))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert _rel_err(res[0][0].view(p.M, ld)[:, :p.cout].double(), p.emu()) < TOL


def test_k_320_keeps_the_streaming_walk(gpu):
    """Case f (seed 106): K = 320 is beyond what the resident walk holds; the call takes the streaming walk and meets
    the float64 product."""
    p = _Problem(106, 300, 1024, KS, gpu)
    out, _, ld, _ = _gemm(p, KS)
    assert _rel_err(out.view(p.M, ld)[:, :p.cout].double(), p.emu()) < TOL


def test_more_row_tiles_than_workgroups(gpu):
    """(seed 107) 514 row tiles x 2 column tiles on 512 resident workgroups: the walk keeps whole rows (splitting them
    would cost a third round), so two workgroups stage a second row tile behind their first."""
    p = _Problem(107, 513 * 128 + 4, 72, 64, gpu)
    out, _, ld, _ = _gemm(p, 64, f16=True)
    ref, _, _, _ = _gemm(p, KS, f16=True)
    assert torch.equal(_bits(out), _bits(ref))
    assert _rel_err(out.view(p.M, ld)[-200:, :p.cout].double(), p.emu()[-200:]) < 1e-3
