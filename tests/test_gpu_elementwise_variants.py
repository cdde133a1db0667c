"""Elementwise parity of the GMA, SK, BOF and Twins engines: tests/test_gpu_elementwise.py's scheme on the variants' own
oracles.

The older field tests of these engines bound the MEAN end-point error alone (test_gpu_gma.py and the BOF test of
test_gpu_e2e.py by 1e-3 px, test_gpu_sk.py by 8 N), and never look at the 1/8-resolution flows.  An aggregator that drops the
last 8 keys of every attention row moves the 256 x 264 field by 6.5e-4 px in the mean - 246 N, and below 1e-3
(tests/test_noise_floor.py::test_a_mean_bound_is_blind_to_eight_dropped_keys).  Here the engine's field and its 1/8-resolution
flows are compared with the variant's oracle in float64 - tests/mof_gma_oracle.py, tests/mof_sk_oracle.py, oracle.mof_oracle
for the plain update block on the BOF network, tests/mof_twins_oracle.py for a checkpoint with the Twins-SVT encoders (whose
own field test in tests/test_gpu_twins.py holds three of its four cases by the mean alone) - and every statistic of
tests_support.error_stats / low_stats must stay within K times N, the same oracle's float32-against-float64 noise for the same
input, weights and depth.  K is tests_support.K_OF's: 8 for 'f16x3', 4 for 'f32' (which only the plain update block on the
residual encoders accepts).  Nothing in a bound comes from the engine.

The attention store's resident f16 plane rounds the probabilities to f16 at 2^14 on purpose; in float64 that rounding moves
the 256 x 264 field by less than 0.1 N (test_noise_floor.py::test_plane_rounding_costs_less_than_the_noise_floor, which caps
it at 1 N), so the plain GMA oracle is the reference of both attention forms.

Depth 4 and seed 0 throughout; `randf` frames are test_gpu_gma._frames' (= test_gpu_elementwise's).  The `large_flow` cases
drift the flow head's bias (tests_support.drift_state_dict) to about 4 and 8 cells.  Measured ratios: DESIGN.md,
"Elementwise parity".  Every test prints its lines (`PARITY|...`) before it asserts."""
import time

import pytest
import torch

import test_gpu_elementwise as te
import tests_support as ts

pytestmark = pytest.mark.gpu

DEPTH = 4


def _builder(name):
    if name == "gma":
        import mof_gma_oracle as go
        return go
    if name == "sk":
        import mof_sk_oracle as so
        return so
    if name == "twins":
        import mof_twins_oracle as to
        return to
    from oracle import mof_oracle as mo
    return mo


# variant -> (cfg overrides of engine and oracle alike, the oracle's module, the drifted bias)
VARIANTS = {
    "gma": ({"gma": True}, "gma", ts.DRIFT_KEY),
    "gma+bof": ({"gma": True, "network": "BOFNet"}, "gma", ts.DRIFT_KEY),
    "sk": ({"sk": True}, "sk", ts.DRIFT_KEY_SK),
    "sk+bof": ({"sk": True, "network": "BOFNet"}, "sk", ts.DRIFT_KEY_SK),
    "sk+gma": ({"sk": True, "gma": True}, "sk", ts.DRIFT_KEY_SK),
    "bof": ({"network": "BOFNet"}, "plain", ts.DRIFT_KEY),
    # the Twins-SVT encoders; mof_twins_oracle builds the update block the other switches name
    "twins": ({"twins": True}, "twins", ts.DRIFT_KEY),
    "twins+bof": ({"twins": True, "network": "BOFNet"}, "twins", ts.DRIFT_KEY),
    "twins+sk+gma": ({"twins": True, "sk": True, "gma": True}, "twins", ts.DRIFT_KEY_SK),
}
PRECISIONS = {v: ("f16x3", "f32") if v == "bof" else ("f16x3",) for v in VARIANTS}     # GMA, SK and Twins refuse 'f32'

# (variant, input kind, T, H, W, plain-f16 attention plane expected? (None: no attention)).  Cells per frame:
#   256 x 264 = 32 x 33 = 1056: the resident f16 plane, row stride 1088, a ragged last key tile
#   264 x 264 = 33 x 33 = 1089: P >= 1024 and P % 4 != 0 keeps the split-row probabilities
#   136 x 152 = 17 x 19 =  323: split rows; one depthwise tile (8 x 32 cells) across, three down
#   136 x 312 = 17 x 39 =  663: two depthwise tiles across, both ragged, three down
FIELDS = [("gma", "randf", 5, 256, 264, True), ("gma", "randf", 3, 264, 264, False),
          ("gma", "randf", 3, 136, 152, False), ("gma", "randf", 5, 136, 152, False),
          ("gma+bof", "randf", 5, 256, 264, True),
          ("sk", "randf", 3, 136, 152, None), ("sk", "randf", 5, 136, 152, None), ("sk", "randf", 3, 136, 312, None),
          ("sk+bof", "randf", 5, 136, 152, None), ("sk+gma", "randf", 3, 136, 152, False),
          ("bof", "randf", 5, 128, 192, None), ("bof", "randf", 4, 136, 160, None),
          # uint8 frames of the synthetic clip through forward_u8, at each variant's smallest size
          ("gma", "clip", 3, 136, 152, False), ("gma+bof", "clip", 5, 256, 264, True), ("sk", "clip", 3, 136, 152, None),
          ("sk+bof", "clip", 5, 136, 152, None), ("sk+gma", "clip", 3, 136, 152, False), ("bof", "clip", 4, 136, 160, None),
          # Twins checkpoints at test_gpu_twins.py's own size (17 x 19 cells: ragged 7 x 7 windows both ways)
          ("twins", "randf", 3, 136, 152, None), ("twins", "randf", 5, 136, 152, None),
          ("twins+bof", "randf", 5, 136, 152, None), ("twins+sk+gma", "randf", 3, 136, 152, False),
          ("twins", "clip", 3, 136, 152, None)]
CASES = [f + (p,) for f in FIELDS for p in PRECISIONS[f[0]]]
# large flow: (variant, T, H, W, plane?) x drift c; about 4 and 8 cells at depth 4 (test_noise_floor.py asserts it)
LARGE = [f + (c, p) for f in (("gma", "randf", 5, 256, 264, True), ("sk", "randf", 3, 136, 152, None),
                              ("bof", "randf", 5, 128, 192, None), ("twins", "randf", 3, 136, 152, None))
         for c in (1, 2) for p in PRECISIONS[f[0]]]


def _id(case):
    variant, kind, T, H, W, _, *rest = case
    return f"{variant}-{kind}-T{T}-{H}x{W}" + "".join(f"-drift{r}" if isinstance(r, int) else f"-{r}" for r in rest)


def _engine(variant, sd, precision):
    from vfml import build_network, get_cfg
    cfg = get_cfg()
    for k, v in VARIANTS[variant][0].items():
        setattr(cfg, k, v)
    cfg.precision, cfg.decoder_depth = precision, DEPTH
    net = build_network(cfg)
    net.load_state_dict(sd)
    return net.cuda().eval()


def _state(variant, drift=None):
    from vfml import get_cfg
    from vfml.weights import seeded_state_dict
    over, _, key = VARIANTS[variant]
    cfg = get_cfg()
    for k, v in over.items():
        setattr(cfg, k, v)
    sd = seeded_state_dict(cfg, 0)
    return sd if drift is None else ts.drift_state_dict(sd, drift, key)     # the same dict for the oracles and the engine


def _check(variant, kind, T, H, W, plane, precision, drift=None):
    over, oracle, _ = VARIANTS[variant]
    sd = _state(variant, drift)
    feed, x = te._input(kind, T, H, W)
    ocfg = ts.oracle_cfg(decoder_depth=DEPTH, **over)
    t0 = time.time()
    pair = ts.oracle_pair(x, ocfg, sd, builder=_builder(oracle))
    N = ts.error_stats(pair["f32"][0], pair["f64"][0])
    Nl = ts.low_stats(pair["f32"][1], pair["f64"][1])
    t_ora = time.time() - t0
    net = _engine(variant, sd, precision)
    try:
        got, low = te._run_engine(net, feed, "forward" if kind == "randf" else "forward_u8")
        store = net._att_store
    finally:
        net.release_workspace()
        del net
        torch.cuda.empty_cache()
    if plane is None:
        assert store is None
    else:
        assert store.plain == plane, (H // 8 * (W // 8), store.plain)
    ref, ref_low = pair["f64"]
    M = 1 if over.get("network") == "BOFNet" else T - 2
    assert got.shape == ref.shape == (1, 2 * M, 2, H, W)
    assert low.shape == ref_low.shape == (1, 2 * M, 2, H // 8, W // 8)
    assert torch.isfinite(got).all() and torch.isfinite(low).all()
    E, El = ts.error_stats(got, ref), ts.low_stats(low, ref_low)
    K = ts.K_OF[precision]
    tag = f"{variant}-{kind}-T{T}-{H}x{W}|seed0|{precision}" + ("" if drift is None else f"|drift{drift:g}")
    for name, e, n in (("full", E, N), ("low", El, Nl)):
        print(f"PARITY|{tag}|{name}|N " + " ".join(f"{n[k]:.2e}" for k in ts.STAT_KEYS) + "|engine " +
              " ".join(f"{e[k]:.2e}" for k in ts.STAT_KEYS) + "|ratio " +
              " ".join(f"{e[k] / n[k] if n[k] else float('inf'):.2f}" for k in ts.STAT_KEYS) +
              f"|max |low| {float(ref_low.abs().max()):.2f} cells"
              f"|oracle s f32 {pair['seconds'][0]:.1f} f64 {pair['seconds'][1]:.1f} (this test waited {t_ora:.1f})")
    ts.assert_within(E, N, K, f"[{tag}] field (px)")
    ts.assert_within(El, Nl, K, f"[{tag}] 1/8-resolution flows (cells)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_variant_field_within_k_times_its_oracles_own_noise(gpu, case):
    _check(*case)


@pytest.mark.parametrize("case", LARGE, ids=_id)
def test_variant_large_flow_field_within_k_times_its_oracles_own_noise(gpu, case):
    """The same K at about 4 and 8 cells of flow: K comes from operand widths, and N, computed for these weights, grows with
    the flow on its own.  The seeded weights alone stay below half a cell at depth 4."""
    variant, kind, T, H, W, plane, c, precision = case
    _check(variant, kind, T, H, W, plane, precision, drift=c)
