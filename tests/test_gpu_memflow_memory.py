"""MemFlow's memory bank on the GPU: the bank-plane kernel against float64, the engine's stream
against the CPU oracle of tests/memflow_memory_oracle.py, the bitwise guards around the memory-free path, the job loop."""
import contextlib
import io
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

EPE_TOL = 1e-3                 # the project's contract, px of mean end-point error
PLANE_SCALE = 16384.0
AD = 128


# ----------------------------------------------------------------------------- the kernel
def _problem(P, n_seg, gain):
    g = torch.Generator().manual_seed(P)
    q = (torch.randn(P, AD, generator=g) * gain).contiguous()
    keys = [(torch.randn(P, AD, generator=g) * gain).contiguous() for _ in range(n_seg)]
    return q, keys


def _metrics(got, ref):
    """(row L1 error, row mass error) of probabilities [rows][cols] against float64 `ref`."""
    return float((got - ref).abs().sum(1).max()), float((got.sum(1) - 1).abs().max())


def _bank_planes(P, n_seg, ld, canary=True):
    from vfml import hip
    planes = [hip.PlainWeight(P, ld, "cuda", scale=PLANE_SCALE) for _ in range(n_seg)]
    if canary:
        for a in planes:
            a.hi.view(torch.int16).fill_(0x5A5A)
    return planes


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("n_seg", [1, 2, 3])
@pytest.mark.parametrize("P", [323, 1056, 1100])
def test_bank_planes_against_float64_softmax(gpu, P, n_seg, gain):
    """hip.attention_bank_planes against softmax in float64 over the concatenated keys.  Yardstick: hip.attention_plane on
    the same problem made square (n_seg * P keys, the queries zero-padded to as many rows, the first P rows taken): at most
    twice its error in either metric - room for another summation order, not for a dropped split term (about ten times) or
    for a pad key counted as score 0 (323 and 1100 put a partial tile at every boundary between two key sets: 61 and 52 dead
    keys each, a mass error of percents)."""
    from vfml import hip
    q, keys = _problem(P, n_seg, gain)
    kcat = torch.cat(keys)
    ref = torch.softmax(q.double() @ kcat.double().T / AD ** 0.5, dim=1)
    N = n_seg * P
    ldN = (N + 63) // 64 * 64
    qpad = torch.zeros(N, AD)
    qpad[:P] = q
    sq = hip.PlainWeight(N, ldN, "cuda", scale=PLANE_SCALE)
    hip.attention_plane(qpad.cuda().view(-1), kcat.cuda().view(-1), N, sq)
    l1_sq, mass_sq = _metrics(sq.hi.view(N, ldN)[:P, :N].cpu().double() / PLANE_SCALE, ref)

    ld = (P + 63) // 64 * 64
    planes = _bank_planes(P, n_seg, ld)
    dq, dk = q.cuda().view(-1), [k.cuda().view(-1) for k in keys]
    hip.attention_bank_planes(dq, dk, P, planes)
    got = torch.cat([a.hi.view(P, ld)[:, :P].cpu().double() for a in planes], dim=1) / PLANE_SCALE
    l1, mass = _metrics(got, ref)
    print(f"[bank planes] P={P} n_seg={n_seg} gain={gain:g}: row L1 {l1:.3e} (square {l1_sq:.3e}), "
          f"row mass {mass:.3e} (square {mass_sq:.3e})")
    assert l1 <= 2 * l1_sq, (l1, l1_sq)
    assert mass <= 2 * mass_sq, (mass, mass_sq)
    if n_seg == 1:      # one key set: the plane vfml_attention_plane_f16 writes, to the bit (include/vfml.h says so)
        assert torch.equal(planes[0].hi.view(torch.int16)[:P * ld], sq.hi.view(torch.int16)[:P * ld])
    for a in planes:
        assert not a.hi.view(P, ld)[:, P:].any()                    # pad columns, over the canary
    first = [a.hi.clone() for a in planes]
    hip.attention_bank_planes(dq, dk, P, planes)
    for a, b in zip(first, planes):
        assert torch.equal(a.view(torch.int16), b.hi.view(torch.int16))


def test_bank_planes_offsets_at_1080p(gpu):
    """P = 32400 (1080p), two key sets, two planes of 2.1 GB each: the kernel at the size the engine runs it - 507 key
    tiles per set, 254 workgroups, rows of 32448 halves, the largest the plane form takes.  The planes are separate
    allocations, each below 2 GiB (the largest byte offset in one is 2.10e9; into a key set 16.6e6), so this does NOT
    exercise addressing past 2^31: it checks that rows and key sets land where they belong at full size.  64 sampled rows,
    the last ones among them, against float64.

    Bound (reasoned, not measured): every stored value is one round-to-nearest f16 of a normal number (a probability of
    about 1.5e-5 times 2^14), relative error at most 2^-11, so at most 2^-11 of row L1 error on a row of mass one; the
    scores (22 bits on |score| of a few units) and the f32 sum of 64800 terms (tile-wise, some 2000 sequential additions of
    2^-24 each at worst) add less than 2^-13.  A misplaced row or key set is an error of order one."""
    from vfml import hip
    P, n_seg = 32400, 2
    ld = (P + 63) // 64 * 64
    q, keys = _problem(P, n_seg, 1.0)
    rows = torch.cat([torch.arange(0, P, P // 60)[:60], torch.tensor([P - 3, P - 2, P - 1, 16544])])
    assert len(rows) == 64
    ref = torch.softmax(q[rows].double() @ torch.cat(keys).double().T / AD ** 0.5, dim=1)
    planes = _bank_planes(P, n_seg, ld, canary=False)
    hip.attention_bank_planes(q.cuda().view(-1), [k.cuda().view(-1) for k in keys], P, planes)
    dev_rows = rows.cuda()
    got = torch.cat([a.hi.view(P, ld)[dev_rows, :P].cpu().double() for a in planes], dim=1) / PLANE_SCALE
    l1, mass = _metrics(got, ref)
    print(f"[bank planes] P={P} n_seg={n_seg}: row L1 {l1:.3e}, row mass {mass:.3e} over {len(rows)} rows")
    bound = 2.0 ** -11 + 2.0 ** -13
    assert l1 <= bound and mass <= bound, (l1, mass, bound)
    for a in planes:
        assert not a.hi.view(P, ld)[dev_rows, P:].any()


def test_bank_planes_bad_arguments_launch_nothing(gpu):
    from ctypes import c_void_p
    from vfml import hip
    P = 70
    q = torch.randn(P * AD, device="cuda")
    ws = torch.empty(2 * P, device="cuda")

    def canary(rows, kp, n):
        return _bank_planes(rows, n, kp)

    good, narrow, wide, ten = canary(P, 128, 2), canary(P, 96, 2), canary(2, 32832, 1), canary(P, 128, 10)
    with pytest.raises(RuntimeError, match="d = 64"):
        hip.attention_bank_planes(q, [q, q], P, good, d=64, workspace=ws)
    with pytest.raises(RuntimeError, match="score_scale nan"):
        hip.attention_bank_planes(q, [q, q], P, good, score_scale=float("nan"), workspace=ws)
    with pytest.raises(RuntimeError, match="ld_plane = 96"):
        hip.attention_bank_planes(q, [q, q], P, narrow, workspace=ws)
    with pytest.raises(RuntimeError, match="ld_plane = 32832"):
        hip.attention_bank_planes(q, [q], 2, wide, workspace=ws)
    with pytest.raises(RuntimeError, match="n_seg = 10"):
        hip.attention_bank_planes(q, [q] * 10, P, ten, workspace=ws)
    with pytest.raises(RuntimeError, match="n_seg = 0"):
        hip.attention_bank_planes(q, [], P, [], workspace=ws)
    L = hip.lib()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(qp, kp, pp, wp):
        return L.vfml_attention_bank_planes_f16(qp, 128, kp, 128, 2, P, 128, 0.088, PLANE_SCALE, pp, 128, wp, stream)

    kptr = (c_void_p * 2)(q.data_ptr(), q.data_ptr())
    pptr = (c_void_p * 2)(*[a.hi.data_ptr() for a in good])
    knul = (c_void_p * 2)(q.data_ptr(), None)
    pnul = (c_void_p * 2)(None, good[1].hi.data_ptr())
    qp, wp = c_void_p(q.data_ptr()), c_void_p(ws.data_ptr())
    for args in ((None, kptr, pptr, wp), (qp, None, pptr, wp), (qp, kptr, None, wp), (qp, kptr, pptr, None),
                 (qp, knul, pptr, wp), (qp, kptr, pnul, wp)):
        assert call(*args) != 0 and b"null pointer" in L.vfml_last_error()
    torch.cuda.synchronize()
    for a in good + narrow + wide + ten:
        assert bool((a.hi.view(torch.int16) == 0x5A5A).all())


# ----------------------------------------------------------------------------- the engine
def _pair():
    from oracle import memflow_oracle as mm
    from vfml.memflow_net import build_memflow_network, memflow_cfg, seeded_memflow_state_dict
    cfg = memflow_cfg()
    sd = seeded_memflow_state_dict(cfg, 0)
    net = build_memflow_network(cfg)
    net.load_state_dict(sd)
    net.cuda().eval()
    ora = mm.build_network(mm.get_cfg())
    ora.load_state_dict(sd)
    return net, ora.eval()


_SHARED = {}


def _shared():
    """Once per session: the engine, the fixture clip at 256 x 320 (P = 1280, the smallest plane-form class), the oracle's
    four fields at M = 0, 1, 2 and the engine's through a stream at M = 1, 2."""
    if not _SHARED:
        import memflow_memory_oracle as mo
        net, ora = _pair()
        clip = mo.fixture_clip(256, 320)
        threads = torch.get_num_threads()
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        try:
            ref = {M: [f[1] for f in mo.run_fields(ora, clip, M)] for M in (0, 1, 2)}
        finally:
            torch.set_num_threads(threads)               # (the session's other tests keep their setting)
        dclip = clip.cuda()
        got, counts = {}, {}
        for M in (1, 2):
            st = net.stream(M)
            got[M], counts[M] = [], []
            for i in range(4):
                got[M].append(st.step(dclip[:, i:i + 2])[1].cpu())
                counts[M].append((st.planes_in_use, len(st.entries)))
        _SHARED.update(net=net, clip=dclip, ref=ref, got=got, counts=counts)
    return _SHARED


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(1).sqrt().mean().item()


@pytest.mark.parametrize("M", [1, 2])
def test_stream_matches_memory_oracle(gpu, M):
    """Depth 12, four fields: every field within the contract of its oracle - in the mean.  Every statistic of every field and
    of its 1/8-resolution flow, at 8 times the oracle's own noise: tests/test_gpu_elementwise_memflow.py's stream cases."""
    s = _shared()
    for f in range(4):
        e = _epe(s["got"][M][f], s["ref"][M][f])
        print(f"[memflow memory] M={M} field {f}: mean EPE {e:.3e} px")
        assert e < EPE_TOL, (M, f, e)


def test_stream_tells_the_bank_sizes_apart(gpu):
    """The engine at M = 1 is at least ten times nearer to the M = 1 oracle than to the M = 2 oracle on fields 2 and 3 (the
    first at which the two differ), and the same with the roles swapped; at field 1 it is ten times nearer to its oracle
    than to the memory-free one.  The oracle's own separations are pinned in tests/test_memflow_memory_cpu.py."""
    s = _shared()
    got, ref = s["got"], s["ref"]
    for f in (2, 3):
        for a, b in ((1, 2), (2, 1)):
            near, far = _epe(got[a][f], ref[a][f]), _epe(got[a][f], ref[b][f])
            print(f"[memflow memory] field {f}: engine M={a} to oracle M={a} {near:.3e} px, to oracle M={b} {far:.3e} px")
            assert 10 * near <= far, (f, a, near, far)
    near, far = _epe(got[1][1], ref[1][1]), _epe(got[1][1], ref[0][1])
    print(f"[memflow memory] field 1: engine M=1 to its oracle {near:.3e} px, to the memory-free oracle {far:.3e} px")
    assert 10 * near <= far, (near, far)


def test_plane_count_follows_the_bank(gpu):
    s = _shared()
    for M in (1, 2):
        assert s["counts"][M] == [(min(f, M) + 1, min(f + 1, M)) for f in range(4)], s["counts"][M]


def test_memory_free_steps_are_forward(gpu):
    """Field 0 of any stream, every field of a stream at M = 0, and the field after end=True or reset() are net.forward on
    the pair, bit for bit."""
    s = _shared()
    net, clip = s["net"], s["clip"]
    fwd = [[t.clone() for t in net.forward(clip[:, i:i + 2])] for i in range(4)]
    st0 = net.stream(0)
    for i in range(4):
        low, up = st0.step(clip[:, i:i + 2])
        assert torch.equal(low, fwd[i][0]) and torch.equal(up, fwd[i][1]), i
        assert st0.planes_in_use == 1 and not st0.entries
    st = net.stream(2)
    low, up = st.step(clip[:, 0:2])
    assert torch.equal(low, fwd[0][0]) and torch.equal(up, fwd[0][1])
    _, up = st.step(clip[:, 1:3], end=True)
    assert not torch.equal(up, fwd[1][1]) and not st.entries            # (the bank was read, then cleared)
    _, up = st.step(clip[:, 2:4])
    assert torch.equal(up, fwd[2][1])
    assert len(st.entries) == 1
    st.reset()
    assert not st.entries
    _, up = st.step(clip[:, 3:5])
    assert torch.equal(up, fwd[3][1])


def test_stream_refuses_what_it_cannot_hold(gpu):
    s = _shared()
    net, clip = s["net"], s["clip"]
    st = net.stream(1)
    st.step(clip[:, 0:2])
    _, before = st.step(clip[:, 1:3])
    before = before.clone()
    with pytest.raises(ValueError, match="256x320"):
        st.step(clip[:, 0:2, :, :192, :256].contiguous())
    small = torch.rand(1, 2, 3, 128, 192, device="cuda") * 2 - 1
    with pytest.raises(ValueError, match=r"plane form.*128x192 has P = 384"):
        net.stream(1).step(small)
    net.stream(0).step(small)                                            # memory-free: any size forward takes
    for bad in (-1, 9, "x", 1.5):
        with pytest.raises(ValueError, match="0..8"):
            net.stream(bad)
    assert len(st._planes) == 2 and st.plane_bytes == 2 * 1280 * 1280 * 2
    net.release_workspace()
    assert not st._planes and len(st.entries) == 1                       # the planes go, the bank stays
    st.reset()
    st.step(clip[:, 0:2])
    _, after = st.step(clip[:, 1:3])
    assert torch.equal(before, after) and len(st._planes) == 2


# ----------------------------------------------------------------------------- the job loop
def _processor(tmp_path, monkeypatch, memory):
    from processing.memflow_inference import MemFlowInference
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    os.makedirs(tmp_path / "MemFlow_ckpt", exist_ok=True)
    torch.save(seeded_memflow_state_dict(memflow_cfg(), 0), tmp_path / "MemFlow_ckpt" / "MemFlowNet_sintel.pth")
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = MemFlowInference("cuda", sequence_length=3, memory_frames=memory)
        eng.load_model()
    return eng.get_processor()


def _u8_clip():
    import memflow_memory_oracle as mo
    x = mo.fixture_clip(256, 320)[0]                                     # [5, 3, H, W] in [-1, 1]
    return [f for f in ((x + 1) * 127.5).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()]


def test_job_walks_one_stream(gpu, tmp_path, monkeypatch):
    """A job over the 5-frame clip with a bank of 2 equals stepping MemFlowStream by hand over the pairs (0, 0), (0, 1), ...,
    bit for bit; with the setting at 0 the job is today's batch path; the memory job's cache directory carries _mem2."""
    import numpy as np
    from storage.filename_generator import generate_cache_directory
    from vfml.runner import run_sharded
    frames = _u8_clip()
    proc = _processor(tmp_path, monkeypatch, 2)
    clip = proc.upload_clip(frames)
    job = run_sharded(proc, clip, range(5))
    core = proc.core_engine
    st = core.model.stream(2)
    x = torch.from_numpy(np.stack(frames)).cuda().permute(0, 3, 1, 2).float()[None]
    x = core.normalise_as(x, 0)
    for i in range(5):
        _, up = st.step(x[:, [max(0, i - 1), i]].contiguous())
        assert np.array_equal(job[i], up[0].permute(1, 2, 0).cpu().numpy()), i
    again = run_sharded(proc, clip, range(5))                            # a job starts from an empty bank
    assert np.array_equal(again, job)
    proc0 = _processor(tmp_path, monkeypatch, 0)
    clip0 = proc0.upload_clip(frames)
    job0 = run_sharded(proc0, clip0, range(5))
    batch = proc0.compute_optical_flow_resident_batch(clip0, list(range(5)))
    for i in range(5):
        assert np.array_equal(job0[i], batch[i].cpu().numpy()), i
    assert np.array_equal(job0[0], job[0]) and not np.array_equal(job0[2], job[2])
    kw = dict(start_frame=0, max_frames=5, sequence_length=3, model="memflow", dataset="sintel")
    assert generate_cache_directory("/data/clip.mp4", memory_frames=proc.memory_frames, **kw).endswith("_frames5_mem2")
    assert generate_cache_directory("/data/clip.mp4", memory_frames=proc0.memory_frames, **kw).endswith("_frames5")
