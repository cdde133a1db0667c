"""What the elementwise bound of tests/test_gpu_elementwise_memflow.py can see, measured on the MemFlow oracles alone (no GPU).

N is the float32 oracle's field against the float64 oracle's on the very input (tests_support.memflow_oracle_fields): depth 4,
seed 0, memflow_memory_oracle.fixture_clip, one stream of capacity M.  Every figure below is a multiple of N per field, for
the full-resolution field (px) and for the 1/8-resolution flow (cells, "Nl").

  * the resident plane's rounding - one f16 per attention probability at 2^14 - moves no statistic by more than 1 N, so the
    plain float64 oracle is the reference of the plane form and of the split-row form alike;
  * an oracle whose attention rows ignore their last 8 keys stays below the older tests' 1e-3 px mean bound and is more than
    8 N off in every statistic;
  * a bank that takes the value map of iteration depth - 2 instead of the last: measured and printed, see the test;
  * tests_support.drift_state_dict reaches more than 4 and more than 8 cells on MemFlow's two-channel flow head."""
import pytest
import torch

import tests_support as ts

DEPTH = 4
ATT_SCALE = 16384.0               # vfml.memflow_net.ATT_SCALE: the plane holds 2^14 x probability in f16
K = ts.K_OF["f16x3"]
_CACHE = {}


def _state(drift=None):
    from vfml.memflow_net import memflow_cfg, seeded_memflow_state_dict
    if "sd" not in _CACHE:
        _CACHE["sd"] = seeded_memflow_state_dict(memflow_cfg(), 0)
    return _CACHE["sd"] if drift is None else ts.drift_state_dict(_CACHE["sd"], drift)


def _clip(H, W):
    import memflow_memory_oracle as mo
    return mo.fixture_clip(H, W, frames=5)


def _mutant_fields(clip, M, alter=None, net=None):
    """The float64 oracle's fields of `clip` through one stream of capacity M with `alter` on every attention row."""
    net = net or ts.memflow_oracle_net(DEPTH, _state(), double=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return ts.memflow_stream_fields(net, clip.double(), M, alter)


def _in_N(dev, pair, f, g=None):
    """Field g (default f) of (flow, low) `dev` against field f of the float64 oracle, and field f's noise: four dicts
    (deviation, N, 1/8-resolution deviation, Nl)."""
    g = f if g is None else g
    (r32, l32), (r64, l64) = pair["f32"], pair["f64"]
    return (ts.error_stats(ts.field_of(dev[0], g), ts.field_of(r64, f)), ts.error_stats(ts.field_of(r32, f), ts.field_of(r64, f)),
            ts.low_stats(ts.field_of(dev[1], g), ts.field_of(l64, f)), ts.low_stats(ts.field_of(l32, f), ts.field_of(l64, f)))


def _line(what, d, n):
    print(f"{what}: {ts.fmt_stats(d)} | N {ts.fmt_stats(n)} | / N " + " ".join(f"{k} {d[k] / n[k]:.2f}" for k in ts.STAT_KEYS))
    return {k: d[k] / n[k] for k in ts.STAT_KEYS}


def test_helpers_are_the_oracles_own_runs():
    """memflow_oracle_fields is cached, its float32 half is memflow_memory_oracle.run_fields on the float32 network bit for
    bit (M = 0: MemFlowNetOracle.forward on every pair), its float64 half is float64, and both are in error_stats' layout."""
    import memflow_memory_oracle as mo
    clip = _clip(128, 192)
    for M in (0, 2):
        pair = ts.memflow_oracle_fields(clip, DEPTH, _state(), M)
        assert pair is ts.memflow_oracle_fields(clip, DEPTH, _state(), M)
        flow, low = pair["f32"]
        assert flow.shape == (1, 4, 2, 128, 192) and low.shape == (1, 4, 2, 16, 24) and flow.dtype == torch.float32
        assert pair["f64"][0].dtype == pair["f64"][1].dtype == torch.float64 and pair["f64"][0].shape == flow.shape
        net = ts.memflow_oracle_net(DEPTH, _state())
        for i, (lo, up) in enumerate(mo.run_fields(net, clip, M)):
            assert torch.equal(flow[0, i], up[0]) and torch.equal(low[0, i], lo[0]), (M, i)
            if M == 0:
                lo0, up0 = net(clip[:, i:i + 2])
                assert torch.equal(up, up0) and torch.equal(lo, lo0), i
    a, b = ts.memflow_oracle_fields(clip, DEPTH, _state(), 0), ts.memflow_oracle_fields(clip, DEPTH, _state(), 2)
    assert torch.equal(a["f64"][0][:, 0], b["f64"][0][:, 0]) and not torch.equal(a["f64"][0][:, 1], b["f64"][0][:, 1])


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("H,W", [(128, 192), (256, 264)])
def test_plane_rounding_costs_less_than_the_noise_floor(H, W, M):
    """The attention probabilities of the float64 oracle rounded to one f16 at 2^14 (that softmax only: upsample_flow's 9-way
    softmax is untouched): on every field of the stream, every statistic of the field and of the 1/8-resolution flow moves by
    at most 1 N - the cap tests/test_noise_floor.py holds the GMA plane to.  Measured 0.05 to 0.25 N.  The cap is the
    condition under which the plain oracle is the reference of the plane cases, not a fit."""
    clip = _clip(H, W)
    pair = ts.memflow_oracle_fields(clip, DEPTH, _state(), M)
    dev = _mutant_fields(clip, M, lambda a: (a * ATT_SCALE).half().double() / ATT_SCALE)
    for f in range(4):
        d, n, dl, nl = _in_N(dev, pair, f)
        _line(f"plane rounding {H}x{W} M={M} field {f} (px)", d, n)
        _line(f"plane rounding {H}x{W} M={M} field {f} (cells)", dl, nl)
        for k in ts.STAT_KEYS:
            assert 0.0 < d[k] <= n[k], (f, k, d[k], n[k])
            assert 0.0 < dl[k] <= nl[k], (f, k, dl[k], nl[k])


def _dropped(a):
    """Rows that ignore their last 8 keys: the softmax over the others."""
    a = a.clone()
    a[..., -8:] = 0
    return a / a.sum(-1, keepdim=True)


@pytest.mark.parametrize("M", [0, 2])
def test_a_mean_bound_is_blind_to_eight_dropped_keys(M):
    """256 x 264 (P = 1056), field 2, float64 against float64: attention rows that ignore their last 8 keys (of the frame's own
    key set, the last of the joint softmax) move the field by less than 1e-3 px in the mean - all the older MemFlow tests
    assert - and by more than 8 N in EVERY statistic of the field and of the 1/8-resolution flow.  Measured: M = 0 2.6e-4 px
    mean, 105 N, at least 45 N (36 Nl); M = 2 (the defect in fields 0 and 1 too, so in the bank) 34 N in the mean, at least
    21 N (11 Nl)."""
    clip = _clip(256, 264)
    pair = ts.memflow_oracle_fields(clip, DEPTH, _state(), M)
    if M == 0:           # memory-free: field 2 is a run of its own
        dev, g = _mutant_fields(clip[:, 2:4], 0, _dropped), 0
    else:
        dev, g = _mutant_fields(clip[:, :4], M, _dropped), 2
    d, n, dl, nl = _in_N(dev, pair, 2, g)
    r = _line(f"last 8 keys dropped, M={M} field 2 (px)", d, n)
    rl = _line(f"last 8 keys dropped, M={M} field 2 (cells)", dl, nl)
    assert d["mean"] < ts.EPE_TOL
    for k in ts.STAT_KEYS:
        assert r[k] > K and rl[k] > K, (k, r[k], rl[k])


def test_a_bank_that_takes_an_earlier_value_map():
    """A mutant of the bank itself, 256 x 264, M = 2: every entry holds the value map of iteration depth - 2 instead of the
    last one's.  Fields 1 to 3 read it.  Measured: 7.2e-4 to 9.5e-4 px in the mean - below the older tests' 1e-3 px - which is
    290 to 360 N, and at least 90 N (50 Nl) in every statistic.  The mean is asserted above 8 N on each of the three fields."""
    clip = _clip(256, 264)
    pair = ts.memflow_oracle_fields(clip, DEPTH, _state(), 2)
    net = ts.memflow_oracle_net(DEPTH, _state(), double=True)
    import memflow_memory_oracle as mo
    seen = []
    hook = net.update_block.value.register_forward_hook(lambda mod, args, out: seen.append(out))
    st = mo.Stream(net, 2)
    fields = []
    for i in range(4):
        del seen[:]
        fields.append(st.step(clip[:, i:i + 2].double()))
        assert len(seen) == DEPTH
        k, v = st.bank[-1]
        assert torch.equal(v, seen[-1].flatten(2).transpose(1, 2))
        st.bank[-1] = (k, seen[DEPTH - 2].flatten(2).transpose(1, 2).clone())
    hook.remove()
    dev = ts.memflow_stack(fields)
    assert torch.equal(dev[0][:, 0], pair["f64"][0][:, 0])              # field 0 reads no bank
    for f in (1, 2, 3):
        d, n, dl, nl = _in_N(dev, pair, f)
        r = _line(f"bank holds v of iteration {DEPTH - 2}, field {f} (px)", d, n)
        _line(f"bank holds v of iteration {DEPTH - 2}, field {f} (cells)", dl, nl)
        assert r["mean"] > K, (f, r)


def test_drift_makes_memflows_flow_large():
    """drift_state_dict on MemFlow's two-channel flow head (the first two components of DRIFT_DIRECTION), float64 oracle,
    128 x 192 and 256 x 264, depth 4: more than 4 cells at c = 1 and more than 8 at c = 2 (4.3 and 8.3 measured; the seeded
    weights alone stay near one cell)."""
    sd = _state()
    assert sd[ts.DRIFT_KEY].numel() == 2
    d1 = ts.drift_state_dict(sd, 1)
    assert [k for k in sd if not torch.equal(d1[k], sd[k])] == [ts.DRIFT_KEY]
    assert torch.equal(d1[ts.DRIFT_KEY], sd[ts.DRIFT_KEY] + torch.tensor(ts.DRIFT_DIRECTION[:2]))
    with pytest.raises(ValueError, match="3 entries"):
        ts.drift_state_dict({ts.DRIFT_KEY: torch.zeros(3)}, 1)
    for H, W in ((128, 192), (256, 264)):
        pair = _clip(H, W)[:, :2].double()
        for c in (0, 1, 2):
            low, _ = ts.memflow_oracle_net(DEPTH, _state(c) if c else sd, double=True)(pair)
            top = float(low.abs().max())
            print(f"memflow {H}x{W} c = {c}: max |low| {top:.2f} cells")
            if c:
                assert top > 4 * c
                assert float(low[0, 0].mean()) > 0 > float(low[0, 1].mean())       # x and y each drift their own way
