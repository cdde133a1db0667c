"""MemFlowNetHIP — the MemFlow pair network on the vfml HIP kernels.

Stands in for what reference processing/memflow_inference_isolated.py:54-107 builds out of the
(absent) MemFlow submodule: `build_network(cfg)` + `InferenceCore(model).step(pair, end=True)` on the
last two frames of the window, with an empty memory bank.  Architecture: DESIGN.md §2b / oracle/
memflow_oracle.py — RAFT encoders and one correlation pyramid (previous -> current frame), an update
block whose motion features get a memory read-out added,  m_global = m + gamma * softmax(q k^T/sqrt(d)) v,
where (with the empty bank) keys and values are the frame's own.

MI355X shape of the read-out: q and k come from the context features and do not change over the
iterations, so the P x P attention matrix is computed ONCE per field, kept resident in HBM as
split-row halves (4.2 GB at 1080p; no flash-style re-computation needed with 288 GB), and every
iteration is one long-K GEMM  attn[P,P] . v[P,128]  on the MFMA kernel with the residual add fused.

MemFlowStream (below) is the bank that is not empty: fields in frame order, each reading the keys and
values of up to `memory_frames` fields before it; with none held a step is forward() launch for launch.  With
warm_start=True a field's recurrence also starts from the previous field's 1/8-resolution flow projected
forward along itself (hip.flow_forward_interpolate), upstream's `flow_init`.
"""
import weakref

import torch
import torch.nn as nn

from . import hip, update_block
from .network import MOFNetHIP, _Holder
from .weights import pack_conv_weight

# attention probabilities are stored times 2^14 (split rows hold f16 halves: an unscaled 1080p row, 32400 probabilities
# of 3e-5 on average, would sit in the f16 subnormals); the read-out GEMM divides it out through out_scale
ATT_SCALE = 16384.0
ATT_PLAIN = True            # False: keep the probabilities as split rows (hi + lo)


def memflow_conv_spec(cfg):
    from .weights import _encoder_spec
    cor = cfg.corr_levels * (2 * cfg.corr_radius + 1) ** 2
    hid, ad = cfg.feat_dim // 2, cfg.att_dim
    ub = "update_block"
    s = _encoder_spec("fnet", cfg.feat_dim) + _encoder_spec("cnet", cfg.feat_dim)
    s += [("query", ad, hid, 1, 1), ("key", ad, hid, 1, 1),
          (f"{ub}.encoder.convc1", 256, cor, 1, 1), (f"{ub}.encoder.convc2", 192, 256, 3, 3),
          (f"{ub}.encoder.convf1", 128, 2, 7, 7), (f"{ub}.encoder.convf2", 64, 128, 3, 3),
          (f"{ub}.encoder.conv", 128 - 4, 192 + 64, 3, 3), (f"{ub}.value", ad, 128, 1, 1)]
    for nm, kh, kw in (("z1", 1, 5), ("r1", 1, 5), ("q1", 1, 5), ("z2", 5, 1), ("r2", 5, 1), ("q2", 5, 1)):
        s.append((f"{ub}.gru.conv{nm}", hid, hid + 3 * 128, kh, kw))
    s += [(f"{ub}.flow_head.conv1", 256, hid, 3, 3), (f"{ub}.flow_head.conv2", 2, 256, 3, 3),
          (f"{ub}.mask.0", 256, hid, 3, 3), (f"{ub}.mask.2", 64 * 9, 256, 1, 1)]
    return s


def memflow_cfg():
    from .cfg import Cfg
    return Cfg(restore_ckpt="", network="MemFlowNet", feat_dim=256, down_ratio=8, corr_levels=4, corr_radius=4,
               decoder_depth=12, att_dim=128, precision="f16x3",
               input_scale=1.0, input_shift=0.0)   # frames reach the network already in [-1, 1]


def seeded_memflow_state_dict(cfg, seed=0, gamma=0.5):
    import math
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cout, cin, kh, kw in memflow_conv_spec(cfg):
        bound = 1.0 / math.sqrt(cin * kh * kw)
        sd[f"{name}.weight"] = (torch.rand(cout, cin, kh, kw, generator=g) * 2 - 1) * bound
        sd[f"{name}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound
    sd["update_block.gamma"] = torch.tensor([gamma])      # upstream initialises 0; non-zero exercises the read-out
    return sd


class MemFlowNetHIP(MOFNetHIP):
    def __init__(self, cfg):
        _Holder.__init__(self)
        import collections
        self.cfg = cfg
        self.hidden_dim = self.context_dim = cfg.feat_dim // 2
        self.tri_frame = False
        self._spec = memflow_conv_spec(cfg)
        for name, cout, cin, kh, kw in self._spec:
            leaf = self
            for p in name.split("."):
                leaf = leaf.child(p)
            leaf.weight = nn.Parameter(torch.zeros(cout, cin, kh, kw), requires_grad=False)
            leaf.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        self.child("update_block").gamma = nn.Parameter(torch.zeros(1), requires_grad=False)
        self._packed = None
        self._packed_key = None
        self._packed_serial = 0
        self._ws = {}
        self._graphs = {}
        self._pyr_free = []
        self._att_planes = {}            # attention matrices as plain f16 planes (hip.PlainWeight), per pair of a pass
        self._feat_cache = collections.OrderedDict()
        self._streams = weakref.WeakSet()    # the MemFlowStreams on this network: release_workspace drops their planes

    def release_workspace(self):
        super().release_workspace()
        self._att_planes.clear()
        for st in list(self._streams):
            st._planes.clear()
            st._scratch.clear()          # (the kept flow stays, as the bank does)

    # ------------------------------------------------------------------ weights
    def _pack(self, device):
        split = self._precision() == "f16x3"
        key = (str(device), split, tuple(p._version for p in self.parameters()),
               tuple(p.data_ptr() for p in self.parameters()))
        if self._packed is not None and self._packed_key == key:
            return self._packed
        P, cblock_names = {}, set()
        ub = "update_block"
        for name, cout, cin, kh, kw in self._spec:
            leaf = self._param(name)
            w = leaf.weight.detach().to(device=device, dtype=torch.float32)
            b = leaf.bias.detach().to(device=device, dtype=torch.float32).contiguous()
            if name.endswith(".encoder.convc1"):       # lookup block padded to whole units (zero weights)
                cor_p = (cin + 31) // 32 * 32 if split else (cin + 3) // 4 * 4   # whole K steps: the uniform-step loader
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, cor_p - cin))
            # update-block convolutions read split-row activations (all but convf1): channel-block K order
            cb = split and ((name.startswith(ub + ".") and not name.endswith(".convf1")) or
                            (name.split(".")[0] in ("fnet", "cnet") and name.count(".") > 1) or
                            name in ("fnet.conv2", "cnet.conv2"))
            if cb:
                cblock_names.add(name)
            P[name] = (pack_conv_weight(w, cin_pad=4 if cin in (2, 3) else None, cblock=cb), b)
        # (three MFMAs per product everywhere: every split-row layer in 32-channel K blocks)
        self._pack_gates(P, device, split, self._block_of(split, set()), cblock_names)
        if split:
            self._split_planes(P, device, cblock_names)
        self._gamma = float(self._param(ub).gamma.item())   # read once per load: .item() synchronises
        self._packed, self._packed_key = P, key
        self._packed_serial += 1
        self._feat_cache.clear()
        return P

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, pair, data=None, frame_keys=None, flow_init=None):
        """pair: float [1, 2, 3, H, W] in [-1, 1] on the GPU (previous, current).
        Returns (flow_low [1,2,h,w], flow [1,2,H,W]) like InferenceCore.step(..., end=True).
        frame_keys: optional pair of hashable ids of the two frames (same id = same normalised pixels): the
        feature encoder output of a frame is then kept, so a frame that is "current" in one call and
        "previous" in the next is encoded once (results bit-identical).
        flow_init: optional 1/8-resolution flow the recurrence starts from, in cells, float32 on the pair's device:
        [1, 2, h, w] or [h, w, 2] (or the rows [h * w, 4] = (x, y, 0, 0) a stream hands over); None: zero, today's launches."""
        if isinstance(pair, torch.Tensor) and pair.dim() == 5 and pair.shape[1] != 2:
            raise ValueError(f"pair must be [1,2,3,H,W], got {tuple(pair.shape)}")
        return self._run_pairs(pair, frame_keys, None, flow_init)

    @torch.no_grad()
    def forward_pairs(self, frames, data=None, frame_keys=None, flow_init=None):
        """frames: float [1, B+1, 3, H, W] in [-1, 1] on the GPU: B overlapping pairs (k, k+1) - B consecutive
        fields of a job in one pass (every pair its own fresh-memory step, exactly as B separate calls; at
        1080p one pair leaves most tiles of the update-block convolutions' last round empty).
        Returns (flow_low [B,2,h,w], flow [B,2,H,W]).  flow_init: None, or a single pair's (forward): a starting flow belongs
        to one field."""
        return self._run_pairs(frames, frame_keys, None, flow_init)

    def stream(self, memory_frames=0, warm_start=False):
        """A stream of fields in frame order that carries the memory bank and, with warm_start, the flow (MemFlowStream)."""
        return MemFlowStream(self, memory_frames, warm_start)

    @staticmethod
    def _check_flow_init(flow_init, B, h, w, dev):
        """The form of a starting flow (forward's docstring); raises before anything is launched."""
        if B != 1:
            raise ValueError(f"flow_init starts ONE field's recurrence: it is refused with {B} pairs in a pass")
        if not isinstance(flow_init, torch.Tensor) or flow_init.dtype != torch.float32:
            raise ValueError(f"flow_init must be a float32 tensor, got {getattr(flow_init, 'dtype', type(flow_init))}")
        if flow_init.device != dev:
            raise ValueError(f"flow_init is on {flow_init.device}, the pair on {dev}")
        if tuple(flow_init.shape) not in ((1, 2, h, w), (h, w, 2), (h * w, 4)):
            raise ValueError(f"flow_init must be [1,2,{h},{w}] or [{h},{w},2] (the 1/8-resolution grid of the pair, in cells), "
                             f"got {tuple(flow_init.shape)}")

    def _run_pairs(self, frames, frame_keys, mem, flow_init=None):
        """forward_pairs; mem: the MemFlowStream whose bank this (single) pair reads and, after its last iteration, joins -
        with no entry held the launches are forward_pairs' own.  flow_init: forward's."""
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise RuntimeError("MemFlowNetHIP runs on an MI355X (HIP) device only; got "
                               f"{getattr(frames, 'device', type(frames))}. There is no CPU fallback in the shipped engine.")
        if frames.dim() != 5 or frames.shape[0] != 1 or frames.shape[1] < 2 or frames.shape[2] != 3:
            raise ValueError(f"frames must be [1,B+1,3,H,W], got {tuple(frames.shape)}")
        if flow_init is not None:
            self._check_flow_init(flow_init, frames.shape[1] - 1, frames.shape[3] // 8, frames.shape[4] // 8, frames.device)
        cfg = self.cfg
        src = frames[0].float().contiguous()
        B = src.shape[0] - 1
        H, W = src.shape[2], src.shape[3]
        if H % 8 or W % 8:
            raise ValueError("H and W must be multiples of 8 (use InputPadder)")
        L, R, D, AD = cfg.corr_levels, cfg.corr_radius, cfg.feat_dim, cfg.att_dim
        h, w = H // 8, W // 8
        if (h >> (L - 1)) < 2 or (w >> (L - 1)) < 2:
            raise ValueError(f"frame {H}x{W} too small for a {L}-level correlation pyramid")
        dev = src.device
        Pn = h * w
        MP = B * Pn
        P8, ldA, plain = self._attention_geometry(Pn)
        if mem is not None and mem.memory_frames and not (ATT_PLAIN and plain):       # before anything is launched
            if not ATT_PLAIN:
                raise ValueError("the memory bank needs the plane form of the attention, which memflow_net.ATT_PLAIN = False "
                                 "switches off")
            raise ValueError(f"the memory bank needs the plane form of the attention (P >= 1024 cells, P % 4 == 0, a plane "
                             f"below 2 GiB, row stride <= 32768): {H}x{W} has P = {Pn}")
        plain = ATT_PLAIN and plain
        P = self._pack(dev)
        if self._precision() != "f16x3":
            raise ValueError("the MemFlow path is built on the split-f16 kernels: cfg.precision must be 'f16x3'")
        AF = hip.FMT_S16
        cor_p = (L * (2 * R + 1) ** 2 + 31) // 32 * 32        # the lookup block in whole K steps: the uniform-step loader

        with torch.cuda.device(dev):
            # volumes in tiles under tile-ordered rows, row strides an odd number of 128-byte lines, as the MOF engine's
            geo = self._volume_geometry(H, W, L, AF)
            keys = None
            if frame_keys is not None:
                if len(frame_keys) != B + 1:
                    raise ValueError("frame_keys must hold one id per frame")
                keys = [("memflow", k, H, W, L, self._precision(), geo.TILE, self._packed_serial) for k in frame_keys]
            feats = self._frame_features(src, list(range(B + 1)), keys, H, W, P, dev, L, geo.hl, geo.wl, geo.Sl, vt=geo.VT)
            ctx = self._frame_context_plain(src, B, H, W, P, dev, Pn, AF)       # cnet on the B previous frames
            pyrs = []
            for k in range(B):       # pair k: queries = frame k, targets = frame k+1
                pyr = [self._buf(f"mpyr{k}_{l}", geo.psz[l], dev) for l in range(L)]
                for l in range(L):
                    hip.conv2d(feats[k][0], D, D, 1, 1, geo.Pv, feats[k + 1][1][l], None, geo.Nl[l], 1, 1, pyr[l], geo.ldl[l],
                               out_scale=1.0 / float(D) ** 0.5 / self.FMAP_ROW_SCALE, in_fmt=AF)   # query rows carry x16
                pyrs.append(pyr)

            def rows(name, c, zero=False):
                return self._buf(name, MP * c, dev, zero=zero)
            GLD, cols = self._state_columns()
            s = update_block.window_state(
                P, self._nm, AF, h, w, geo, R, rows("gru_state", GLD), GLD, cols, cor_p, cor_p, False, False,
                corr=rows("mcorr", cor_p, zero=True), c1=rows("c1", 256), cf=rows("cf", 256), f1=rows("f1", 128),
                fh=rows("fh", 256), flow4=rows("flow4", 4), coords1=rows("coords1", 4),
                delta=rows("mdelta", 4, zero=True),     # channels 2,3 stay zero: no backward flow here
                fh_taps=None, frows=None)
            G, INP = s.G, s.INP
            G.view(MP, GLD)[:, s.HH:s.HH + 256].copy_(ctx.view(MP, 256))
            # context parts of the GRU gates (+ bias), once per field
            gate_add = {}
            for k, (kh, kw) in (("1", (1, 5)), ("2", (5, 1))):
                for g, co in (("zr", 256), ("q", 128)):
                    wgt, b = P[f"update_block.gru.conv{g}{k}.ctx"]
                    a = self._buf(f"gate_add_{g}{k}", MP * co, dev)
                    hip.conv2d(G, 128, GLD, B, h, w, wgt, b, co, kh, kw, a, co, in0_off=INP, pad_h=kh // 2,
                               pad_w=kw // 2, in_fmt=AF)
                    gate_add[g + k] = a

            # memory read-out operator: attn = softmax(q k^T / sqrt(d)), P x P per pair, once per field
            qmap = self._buf("att_q", MP * AD, dev)
            kmap = self._buf("att_k", MP * AD, dev)
            bank = mem.entries if mem is not None else ()
            wgt, b = P["query"]
            if bank:       # the bank form takes q as f32 rows (csrc/attention.hip)
                hip.conv2d(G, 128, GLD, B, h, w, wgt, b, AD, 1, 1, qmap, AD, in0_off=INP, in_fmt=AF)
            else:
                hip.conv2d(G, 128, GLD, B, h, w, wgt, b, AD, 1, 1, qmap, AD, in0_off=INP, in_fmt=AF, out_fmt=AF)
            wgt, b = P["key"]
            hip.conv2d(G, 128, GLD, B, h, w, wgt, b, AD, 1, 1, kmap, AD, in0_off=INP, in_fmt=AF)
            # probabilities as ONE f16 each (round to nearest, times ATT_SCALE): 2^-12 relative per probability, unbiased -
            # the 1080p EPE does not move (tests/test_gpu_memflow.py); else - small or odd frames - as split rows
            # (update_block.attention_readout has the two forms of the read-out)
            attn, r_mem = [], None
            if bank:
                # [bank keys ..., k_t]: one joint softmax, one plane per key set (the stream's, kept across fields)
                planes = mem._planes_for(len(bank) + 1, Pn, ldA, dev)
                hip.attention_bank_planes(qmap, [e[0] for e in bank] + [kmap], Pn, planes, score_scale=1.0 / float(AD) ** 0.5,
                                          d=AD, workspace=self._buf("att_stats", 2 * Pn, dev))
                attn.append(planes[-1])
            else:
                scores = self._buf("att_scores", Pn * ldA, dev)
            for k in range(0 if bank else B):
                kw_ = hip.SplitWeight(Pn, AD, dev).fill(kmap, src_off=k * Pn * AD, scale=16.0)
                hip.conv2d(qmap, AD, AD, 1, 1, Pn, kw_, None, Pn, 1, 1, scores, ldA, in0_off=k * Pn * AD,
                           out_scale=1.0 / float(AD) ** 0.5, in_fmt=AF)
                if plain:
                    if mem is not None and mem.memory_frames:
                        a = mem._planes_for(1, Pn, ldA, dev)[0]  # a stream's memory-free field: into the stream's first plane
                    else:
                        a = self._att_planes.get(k)
                        if a is None or a.rows != Pn or a.kp != ldA or a.hi.device != dev:
                            a = self._att_planes[k] = hip.PlainWeight(Pn, ldA, dev, scale=ATT_SCALE)
                    hip.softmax_rows_f16(scores, Pn, Pn, ldA, a)
                else:
                    a = self._buf(f"att_probs{k}", Pn * ldA, dev)
                    hip.softmax_rows_s16(scores, Pn, Pn, ldA, a, ldA, scale=ATT_SCALE)
                attn.append(a)
            ro = update_block.readout_scratch(self._buf, dev, MP, Pn, AD, ldA, plain,
                                              None if plain else hip.SplitWeight(AD, P8, dev))
            gate_off = dict.fromkeys(gate_add, 0)
            if bank:
                # the bank's part of the read-out, sum_j A_j . V_j: the same for every iteration of the field
                r_mem = self._buf("att_rmem", Pn * AD, dev)
                for j, (_, vj) in enumerate(bank):
                    update_block.plane_readout(s, planes[j], ldA, ro, vj)
                    if j == 0:
                        r_mem.copy_(ro.out_t)
                    else:
                        hip.axpy_f32(ro.out_t, r_mem, Pn * AD)

            if flow_init is not None and tuple(flow_init.shape) != (Pn, 4):
                xy = flow_init[0].permute(1, 2, 0) if flow_init.dim() == 4 else flow_init
                flow_init = self._buf("flow_init", Pn * 4, dev, zero=True).view(Pn, 4)      # channels 2,3 stay zero
                flow_init[:, :2].copy_(xy.reshape(Pn, 2))
            update_block.init_coords(s, B, None if flow_init is None else flow_init.contiguous())
            for it in range(cfg.decoder_depth):
                update_block.lookup(s, B, 0, pyrs=pyrs)
                update_block.convc1(s, B, 0)
                update_block.convc2(s, B, 0)
                update_block.flow_half(s, B, 0)
                update_block.encoder_conv(s, B, 0)
                # value map and memory read-out  m_global = m + gamma * attn . v  (per pair: its own attention)
                update_block.attention_readout(s, "update_block.value", attn, plain, ldA, P8, self._gamma, ATT_SCALE,
                                               s.MF, s.MT, ro, addend=r_mem)
                update_block.sep_conv_gru(s, B, gate_add, gate_off)
                update_block.flow_head(s, B, cout=2)

            if mem is not None and mem.memory_frames:
                mem._take(kmap, ro.val, Pn * AD, (H, W))      # (k_t, the last iteration's value map) joins the bank
            if mem is not None and mem.warm_start:
                mem._keep_flow(s.flow4, Pn, (H, W))           # the next field's recurrence starts from its projection
            mask = self._buf("mmask", MP * 576, dev)
            update_block.mask_head(s, B, mask, 576)
            up = torch.empty(B, H, W, 2, device=dev, dtype=torch.float32)
            for k in range(B):
                hip.convex_upsample(s.coords1, k * Pn * 4, 0, mask, k * Pn * 576, 576, h, w, up.view(-1), out_off=k * H * W * 2)
            low = s.flow4.view(B, h, w, 4)[..., :2].permute(0, 3, 1, 2).clone()
        return low, up.permute(0, 3, 1, 2)

    def _frame_context_plain(self, src, B, H, W, P, dev, Pn, AF):
        """cnet on the previous frame of every pair (frames 0..B-1): [B*Pn*256] = tanh | relu halves."""
        frames = self._buf("frames", B * H * W * 4, dev)
        hip.frames_to_nhwc4(src[0:B].contiguous(), B, H, W, float(self.cfg.input_scale), float(self.cfg.input_shift),
                            frames)
        ctx = torch.empty(B * Pn * 256, device=dev)
        self._encoder("cnet", frames, B, H, W, P, dev, ctx, 256, 0, hip.EPI_TANH_RELU, self.hidden_dim, out_fmt=AF)
        return ctx


MEMORY_FRAMES_MAX = hip.ATT_BANK_MAX - 1       # bank entries: with the frame's own keys one hip.attention_bank_planes call


def check_memory_frames(value, source="memory_frames"):
    """The bank capacity as an integer 0..MEMORY_FRAMES_MAX; anything else is refused."""
    text = str(value).strip() if isinstance(value, (int, str)) and not isinstance(value, bool) else ""
    if not (text.isdigit() and int(text) <= MEMORY_FRAMES_MAX):
        raise ValueError(f"{source} = {value!r}: the memory bank holds an integer 0..{MEMORY_FRAMES_MAX} of earlier fields")
    return int(text)


def check_warm_start(value, source="warm_start"):
    """The warm-start switch as a bool: False / True, 0 / 1, "0" / "1"; anything else is refused."""
    if isinstance(value, bool):
        return value
    text = str(value).strip() if isinstance(value, (int, str)) else ""
    if text not in ("0", "1"):
        raise ValueError(f"{source} = {value!r}: the warm start of a MemFlow stream is switched with 0 or 1")
    return text == "1"


class MemFlowStream:
    """The fields of a video in frame order, each reading the keys and values of the fields before it (DESIGN.md section
    18; upstream's InferenceCore.step).  The bank holds up to `memory_frames` pairs (k_j, v_j), oldest first: a field's keys
    as f32 rows and the value map of its last iteration, on the device.  With entries held the attention rows are the softmax
    JOINTLY over the bank's keys and the frame's own, as one resident f16 plane per key set; the bank's part of the read-out
    is computed once per field.  With none - the first field, memory_frames = 0, after end=True or reset() - a step is
    net.forward on the pair, launch for launch.

    warm_start=True (upstream's flow_init): the stream also keeps the last field's final 1/8-resolution
    flow (flow4, in a buffer of its own: the network's workspace is reused) and starts the next field's recurrence from
    hip.flow_forward_interpolate of it, coords1 = coords0 + that.  The stream's first field and the first after end=True or
    reset() start from zero.  It needs no attention plane: with memory_frames = 0 it runs at every size forward takes.  With
    warm_start=False nothing of this is allocated or launched."""

    def __init__(self, net, memory_frames=0, warm_start=False):
        self.net = net
        self.memory_frames = check_memory_frames(memory_frames)
        self.warm_start = check_warm_start(warm_start)
        self.flow_size = None        # (H, W) of the kept flow; None: the next field starts cold
        self.flow_index = None       # int32 [Pn]: the source cell every cell of the last warm field started from (-1: none)
        self._flow = None            # f32 [Pn * 4]: the last field's flow4
        self._scratch = {}           # the projection's delta rows, index map and workspace
        self.entries = []            # [(k [Pn*AD] f32, v [Pn*AD] f32)], oldest first
        self.size = None             # (H, W) of the entries
        self.planes_in_use = 0       # planes the last step read: entries held before it + 1
        self._planes = []            # hip.PlainWeight [Pn][ldA], kept across fields
        self._spare = []             # an evicted entry's tensors, taken again by the next one
        net._streams.add(self)

    def reset(self):
        self._spare += self.entries
        self.entries = []
        self.size = None
        self.flow_size = None

    @property
    def planes_held(self):
        return len(self._planes)

    @property
    def plane_bytes(self):
        return sum(a.hi.numel() * 2 for a in self._planes)

    def _planes_for(self, n, Pn, ldA, dev):
        ps = self._planes
        if ps and (ps[0].rows != Pn or ps[0].kp != ldA or ps[0].hi.device != dev):
            ps.clear()
        while len(ps) < n:
            ps.append(hip.PlainWeight(Pn, ldA, dev, scale=ATT_SCALE))
        return ps[:n]

    def _take(self, k, v, n, size):
        if self.entries and self.size != size:
            raise ValueError(f"the bank holds fields of {self.size[0]}x{self.size[1]}, this one is {size[0]}x{size[1]}")
        if len(self.entries) == self.memory_frames:
            self._spare.append(self.entries.pop(0))
        self._spare = [e for e in self._spare if e[0].numel() == n and e[0].device == k.device]
        kk, vv = self._spare.pop() if self._spare else (torch.empty_like(k[:n]), torch.empty_like(v[:n]))
        kk.copy_(k[:n])
        vv.copy_(v[:n])
        self.entries.append((kk, vv))
        self.size = size

    def _keep_flow(self, flow4, Pn, size):
        if self._flow is None or self._flow.numel() != Pn * 4 or self._flow.device != flow4.device:
            self._flow = torch.empty(Pn * 4, device=flow4.device)
        self._flow.copy_(flow4[:Pn * 4])
        self.flow_size = size

    def _projected_flow(self, h, w):
        """hip.flow_forward_interpolate of the kept flow as delta rows [Pn][4]; the chosen sources go to flow_index."""
        dev, Pn, sc = self._flow.device, h * w, self._scratch
        if "delta" not in sc or sc["delta"].numel() != Pn * 4 or sc["delta"].device != dev:
            sc.update(delta=torch.empty(Pn * 4, device=dev), index=torch.empty(Pn, dtype=torch.int32, device=dev),
                      ws=hip.flow_forward_interpolate_workspace(1, h, w, dev))
        hip.flow_forward_interpolate(self._flow, h, w, ld_in=4, out=sc["delta"], ld_out=4, index=sc["index"], workspace=sc["ws"])
        self.flow_index = sc["index"]
        return sc["delta"].view(Pn, 4)

    @torch.no_grad()
    def step(self, pair, end=False, frame_keys=None, flow_init=None):
        """pair: float [1, 2, 3, H, W] in [-1, 1] on the GPU (previous, current), the next field of the stream.
        Returns (flow_low [1,2,h,w], flow [1,2,H,W]).  end=True: the bank and the kept flow are cleared after the step.
        flow_init (warm_start=False only): the field's starting flow as net.forward takes it."""
        if not isinstance(pair, torch.Tensor) or pair.dim() != 5 or pair.shape[1] != 2:
            raise ValueError(f"pair must be [1,2,3,H,W], got {tuple(getattr(pair, 'shape', ()))}")
        size = (int(pair.shape[3]), int(pair.shape[4]))
        if self.entries and self.size != size:
            raise ValueError(f"the bank holds fields of {self.size[0]}x{self.size[1]}, this pair is {size[0]}x{size[1]}: "
                             f"reset() the stream before a clip of another size")
        if self.flow_size is not None and self.flow_size != size:
            raise ValueError(f"the stream holds the flow of a {self.flow_size[0]}x{self.flow_size[1]} field, this pair is "
                             f"{size[0]}x{size[1]}: reset() the stream before a clip of another size")
        if flow_init is not None and self.warm_start:
            raise ValueError("a warm_start stream projects its own starting flow: flow_init is for warm_start=False")
        n = len(self.entries)
        self.flow_index = None
        if self.warm_start and self.flow_size is not None:       # (a field of this size has run: H, W are multiples of 8)
            flow_init = self._projected_flow(size[0] // 8, size[1] // 8)
        out = self.net._run_pairs(pair, frame_keys, self, flow_init)
        self.planes_in_use = n + 1
        if end:
            self.reset()
        return out


def build_memflow_network(cfg):
    return MemFlowNetHIP(cfg)
