"""Elementwise parity of the MemFlow engine: tests/test_gpu_elementwise.py's scheme on the MemFlow oracles.

The older MemFlow tests (test_gpu_memflow.py, test_gpu_memflow_memory.py) bound the MEAN end-point error by 1e-3 px against
the float32 oracle, 400 to 600 times the oracle's own rounding noise; attention rows that ignore their last 8 keys pass them
(tests/test_memflow_noise_cpu.py).  Here every field of the pair path (`forward`, `forward_pairs`) and of `MemFlowStream` is
compared with the float64 oracle - oracle.memflow_oracle through tests/memflow_memory_oracle.py's stream of the same
capacity - and every statistic of tests_support.error_stats (px) and low_stats (the 1/8-resolution flow, cells) must stay
within 8 times N, the float32 oracle's distance from the float64 oracle for the same field, weights and depth.  8 is
tests_support.K_OF['f16x3']; MemFlow runs nothing else.  Nothing in a bound comes from the engine.

The resident f16 plane rounds the probabilities to f16 at 2^14 on purpose; in float64 that rounding stays below 1 N in every
statistic of every field (test_memflow_noise_cpu.py::test_plane_rounding_costs_less_than_the_noise_floor), so the plain
oracle is the reference of both attention forms.

Depth 4 and seed 0 throughout; frames are memflow_memory_oracle.fixture_clip(H, W, frames=5).  Cells per frame:
    128 x 192 = 16 x 24 =  384: split-row probabilities
    136 x 152 = 17 x 19 =  323: split rows with P % 8 != 0 (P8 = 328): pad columns in the read-out
    256 x 264 = 32 x 33 = 1056: the resident f16 plane, row stride 1088, a ragged last key tile; the only form the bank takes
    264 x 264 = 33 x 33 = 1089: P >= 1024 and P % 4 != 0 keeps the split rows at a plane-sized P
The `large_flow` cases drift the flow head's bias (tests_support.drift_state_dict) to more than 4 and 8 cells.  Measured
ratios: DESIGN.md, "Elementwise parity".  Every case prints its lines (`PARITY|...`) before it asserts."""
import time

import pytest
import torch

import tests_support as ts

pytestmark = pytest.mark.gpu

DEPTH = 4
PRECISION = "f16x3"
K = ts.K_OF[PRECISION]
_SD = {}


def _state(drift=None):
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    if "sd" not in _SD:
        _SD["sd"] = seeded_memflow_state_dict(memflow_cfg(), 0)
    return _SD["sd"] if drift is None else ts.drift_state_dict(_SD["sd"], drift)   # the same dict for oracles and engine


def _clip(H, W, fields=4):
    import memflow_memory_oracle as mo
    return mo.fixture_clip(H, W, frames=5)[:, :fields + 1].contiguous()


def _engine(sd):
    from vfml.memflow_net import build_memflow_network, memflow_cfg
    cfg = memflow_cfg()
    cfg.decoder_depth = DEPTH
    assert cfg.precision == PRECISION
    net = build_memflow_network(cfg)
    net.load_state_dict(sd)
    return net.cuda().eval()


def _attention_form(net, plane, pairs=1):
    """The form of the attention the last memory-free pass ran: `pairs` resident planes, or the split-row buffers."""
    if plane:
        assert len(net._att_planes) == pairs and not any(k.startswith("att_probs") for k in net._ws)
    else:
        assert not net._att_planes and sum(k.startswith("att_probs") for k in net._ws) == pairs


def _run(H, W, M, fields, run, drift=None):
    """`run(net, clip on the GPU)` -> [(oracle field index, low [1, 2, h, w], flow [1, 2, H, W])] on a fresh engine, whose
    workspace is released afterwards; with it the oracle pair of capacity M over `fields` fields of the clip."""
    sd = _state(drift)
    clip = _clip(H, W, fields)
    t0 = time.time()
    pair = ts.memflow_oracle_fields(clip, DEPTH, sd, M)
    t_ora = time.time() - t0
    net = _engine(sd)
    try:
        got = [(f, low.cpu(), up.cpu()) for f, low, up in run(net, clip.cuda())]
    finally:
        net.release_workspace()
        del net
        torch.cuda.empty_cache()
    return got, pair, t_ora


def _compare(name, H, W, got, pair, t_ora, drift=None):
    """Prints every field's PARITY lines, then asserts every field: the field (px) and the 1/8-resolution flow (cells)."""
    (r32, l32), (r64, l64) = pair["f32"], pair["f64"]
    todo = []
    for f, low, up in got:
        assert up.shape == (1, 2, H, W) and low.shape == (1, 2, H // 8, W // 8)
        assert torch.isfinite(up).all() and torch.isfinite(low).all()
        ref, ref_low = ts.field_of(r64, f), ts.field_of(l64, f)
        N, Nl = ts.error_stats(ts.field_of(r32, f), ref), ts.low_stats(ts.field_of(l32, f), ref_low)
        E, El = ts.error_stats(up[None], ref), ts.low_stats(low[None], ref_low)
        tag = f"memflow-{name}-{H}x{W}|seed0|{PRECISION}" + ("" if drift is None else f"|drift{drift:g}") + f"|field{f}"
        for what, e, n in (("full", E, N), ("low", El, Nl)):
            print(f"PARITY|{tag}|{what}|N " + " ".join(f"{n[k]:.2e}" for k in ts.STAT_KEYS) + "|engine " +
                  " ".join(f"{e[k]:.2e}" for k in ts.STAT_KEYS) + "|ratio " +
                  " ".join(f"{e[k] / n[k] if n[k] else float('inf'):.2f}" for k in ts.STAT_KEYS) +
                  f"|max |low| {float(ref_low.abs().max()):.2f} cells"
                  f"|oracle s f32 {pair['seconds'][0]:.1f} f64 {pair['seconds'][1]:.1f} (this test waited {t_ora:.1f})")
        todo.append((tag, E, N, El, Nl))
    for tag, E, N, El, Nl in todo:
        ts.assert_within(E, N, K, f"[{tag}] field (px)")
        ts.assert_within(El, Nl, K, f"[{tag}] 1/8-resolution flow (cells)")


# ----------------------------------------------------------------------------- the pair path
def _forward(plane, fields):
    def run(net, clip):
        out = []
        for f in fields:
            low, up = net.forward(clip[:, f:f + 2])
            _attention_form(net, plane)
            out.append((f, low.clone(), up.clone()))
        return out
    return run


# (H, W, plane form expected?, fields of the clip that are run)
FORWARD = [(128, 192, False, 4), (136, 152, False, 3), (256, 264, True, 4), (264, 264, False, 2)]


@pytest.mark.parametrize("H,W,plane,fields", FORWARD, ids=[f"{c[0]}x{c[1]}" for c in FORWARD])
def test_forward_within_k_times_the_oracles_own_noise(gpu, H, W, plane, fields):
    """net.forward on every pair of the clip against MemFlowNetOracle.forward in float64."""
    got, pair, t = _run(H, W, 0, fields, _forward(plane, range(fields)))
    _compare("forward", H, W, got, pair, t)


def test_forward_with_split_rows_at_the_planes_size(gpu, monkeypatch):
    """256 x 264 with memflow_net.ATT_PLAIN = False: the split-row probabilities where the plane would run, held to the same
    plain oracle."""
    from vfml import memflow_net
    monkeypatch.setattr(memflow_net, "ATT_PLAIN", False)
    got, pair, t = _run(256, 264, 0, 4, _forward(False, range(4)))
    _compare("forward-rows", 256, 264, got, pair, t)


@pytest.mark.parametrize("H,W,plane,fields", [c for c in FORWARD if c[:2] in ((136, 152), (256, 264))],
                         ids=["136x152", "256x264"])
def test_forward_pairs_within_k_times_the_oracles_own_noise(gpu, H, W, plane, fields):
    """Three overlapping pairs in one pass: every field against the oracle's own fresh-memory field of that pair (the oracle
    run of the `forward` case of the size)."""
    def run(net, clip):
        low, up = net.forward_pairs(clip[:, :4].contiguous())
        assert low.shape[0] == up.shape[0] == 3
        _attention_form(net, plane, pairs=3)
        return [(f, low[f:f + 1].clone(), up[f:f + 1].clone()) for f in range(3)]
    got, pair, t = _run(H, W, 0, fields, run)
    _compare("pairs3", H, W, got, pair, t)


# ----------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("M", [1, 2])
def test_stream_within_k_times_the_memory_oracles_own_noise(gpu, M):
    """256 x 264, four fields through net.stream(M): every field against the field of the oracle's stream of the same
    capacity; fields 1 to 3 read a bank (the entry and plane counts say so).  The last step ends the stream; the field after
    it - pair (2, 3) again - is held to the MEMORY-FREE oracle's field 2, from which the M-oracle's is 5e-3 px away."""
    H, W = 256, 264
    after = []

    def run(net, clip):
        st = net.stream(M)
        out = []
        for f in range(4):
            low, up = st.step(clip[:, f:f + 2], end=f == 3)
            assert st.planes_in_use == min(f, M) + 1 and len(st.entries) == (0 if f == 3 else min(f + 1, M)), (f, len(st.entries))
            out.append((f, low.clone(), up.clone()))
        low, up = st.step(clip[:, 2:4])
        assert st.planes_in_use == 1 and len(st.entries) == 1
        after.append((2, low.cpu(), up.cpu()))
        return out
    got, pair, t = _run(H, W, M, 4, run)
    free = ts.memflow_oracle_fields(_clip(H, W), DEPTH, _state(), 0)
    _compare(f"stream{M}", H, W, got, pair, t)
    _compare(f"stream{M}-after-end", H, W, after, free, 0.0)


# ----------------------------------------------------------------------------- large flow
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("H,W,plane", [(128, 192, False), (256, 264, True)], ids=["128x192", "256x264"])
def test_large_flow_forward_within_k_times_the_oracles_own_noise(gpu, H, W, plane, c):
    """The same K at more than 4 and 8 cells of flow (test_memflow_noise_cpu.py asserts the reach): K comes from operand
    widths, and N, computed for these weights, grows with the flow on its own."""
    got, pair, t = _run(H, W, 0, 1, _forward(plane, (0,)), drift=c)
    _compare("forward", H, W, got, pair, t, drift=c)


@pytest.mark.parametrize("c", [1, 2])
def test_large_flow_stream_within_k_times_the_memory_oracles_own_noise(gpu, c):
    """net.stream(2) at 256 x 264 under drift: field 0 (memory-free) and field 2 (two entries held)."""
    def run(net, clip):
        st = net.stream(2)
        out = []
        for f in range(3):
            low, up = st.step(clip[:, f:f + 2])
            assert len(st.entries) == min(f + 1, 2) and st.planes_in_use == f + 1
            if f != 1:
                out.append((f, low.clone(), up.clone()))
        return out
    got, pair, t = _run(256, 264, 2, 3, run, drift=c)
    _compare("stream2", 256, 264, got, pair, t, drift=c)
