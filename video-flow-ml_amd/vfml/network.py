"""MOFNetHIP — the multi-frame optical-flow network executed by the vfml HIP kernels.

`build_network(cfg)` stands in for `core.Networks.build_network` of the VideoFlow submodule
(reference processing/videoflow_core.py:28,101).  The returned module honours the call the
reference makes at :188, `model(images[B,N,3,H,W], {}) -> (flow[B,2(N-2),2,H,W], aux)`, with the
forward flows of the N-2 centre frames first and the backward flows after them, so that the
reference's `flow[0, shape[1]//2]` pick (:194-195) lands on the same field.

Python only sequences kernels; all arithmetic runs in libvfml_hip.so (include/vfml.h) on NHWC
fp32 buffers.  There is no CPU execution path in this module: on a non-GPU device `forward`
raises.

Pipeline per call (names from SURVEY.md §2b):
  K1 frames -> NHWC4, normalised           vfml_frames_to_nhwc4
  K2 fnet (N frames) / cnet (N-2 frames)   vfml_conv2d + vfml_instnorm_{stats,apply}
  K3/K4 correlation pyramid, 2(N-2) problems: level l = GEMM of centre features against the
        2^l-pooled target features (avg-pool commutes with the dot product)   vfml_avgpool2x2, vfml_conv2d
  loop decoder_depth times:
     K5 lookup (fwd, bwd)                  vfml_corr_lookup
     K6 motion encoder, temporal fusion, SepConvGRU (gates fused into the conv epilogues),
        flow head                          vfml_conv2d, vfml_coords_update   (each layer's launch: vfml/update_block.py)
  mask head (last iteration only) + K8 8x convex upsampling   vfml_conv2d, vfml_convex_upsample
"""
import os
import types

import torch
import torch.nn as nn

from . import hip, update_block
from .frame_store import FrameContext, Iter0Ring, SlotRing, window_base
from .weights import (BASE_CORR_LEVELS, BASE_CORR_RADIUS, GMA_NO_BIAS, TWINS_STAGES, TWINS_WS, conv_spec, corr_channel_subset,
                      is_depthwise, pack_conv_weight, pcblock_hidden, sk_blocks, twins_spec)

# GMA attention probabilities are stored times 2^14, as MemFlow's are (memflow_net.ATT_SCALE: an unscaled 1080p row would sit in
# the f16 subnormals); the read-out divides it out again
ATT_SCALE = 16384.0


def cor_pad(cor, split):
    """Channels of one direction's lookup block in the motion encoder's input: whole float4s (f32 path), or, in split
    rows, a multiple of 16 - the two directions then make whole 32-channel K steps (324 -> 336, K = 672) and the 1x1
    `convc1` takes the uniform-step loader of the LDS-DMA kernel (340 instead of 210 TFLOP/s on it at 1080p); the pad
    channels are zero on both sides (the buffer is zero-filled once, the weights are zero there)."""
    return (cor + 15) // 16 * 16 if split else (cor + 3) // 4 * 4


def take_frames(src, idx):
    """src[idx] along dim 0 without a host->device index upload (a pageable H2D copy would make the
    host wait for all queued GPU work): a view when idx is a contiguous run, device-side copies otherwise."""
    idx = list(idx)
    if all(b == a + 1 for a, b in zip(idx, idx[1:])):
        return src[idx[0]:idx[0] + len(idx)]
    return torch.stack([src[i] for i in idx])


class _Holder(nn.Module):
    """Parameter container; children are created on demand so that dotted checkpoint keys
    (`fnet.layer2.0.downsample.0.weight`) map onto a module tree for load_state_dict."""

    def child(self, name):
        if name not in self._modules:
            self.add_module(name, _Holder())
        return self._modules[name]


class MOFNetHIP(_Holder):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.hidden_dim = self.context_dim = cfg.feat_dim // 2
        if cfg.feat_dim != 256:
            raise ValueError("MOFNetHIP is built for feat_dim=256")
        # 'BOFNet': the tri-frame member of the family - the same blocks on the centre triple of the
        # window (previous, current, next), output [B, 2, 2, H, W] = (forward, backward) of the centre frame
        self.tri_frame = getattr(cfg, "network", "MOFNetStack") == "BOFNet"
        # the GMA global-motion aggregator: per centre frame, attention over its own cells computed
        # once from the context map; every iteration adds gamma * (attention . to_v(mf)) to the motion features as a fourth
        # input block `mg` of the GRU
        self.gma = bool(getattr(cfg, "gma", False))
        # the SK update block: PCBlocks - dense 1x1 pairs, depthwise 15 x 15 / 7 x 7 convolutions,
        # residuals and GELU - in place of the motion encoder's convolutions, the SepConvGRU and the flow head
        self.sk = bool(getattr(cfg, "sk", False))
        self._sk_blocks = {}
        if self.sk:
            if (cfg.corr_levels, cfg.corr_radius) != (BASE_CORR_LEVELS, BASE_CORR_RADIUS):
                raise ValueError(f"the SK update block needs the base lookup (corr_levels, corr_radius) = ({BASE_CORR_LEVELS}, "
                                 f"{BASE_CORR_RADIUS}), got ({cfg.corr_levels}, {cfg.corr_radius}): --fast takes a channel subset of "
                                 f"convc1's input, and a channel subset of a residual block is not defined")
            self._sk_blocks = {n: (ci, co, k) for n, ci, co, k in sk_blocks(cfg)}
        # Twins-SVT encoders in place of the two BasicEncoders: their parameters - linear layers,
        # LayerNorms, the patch and reduction convolutions, the depthwise position encodings - come first in the state dict
        self.twins = bool(getattr(cfg, "twins", False))
        self._twins_spec = twins_spec(cfg)
        for name, _, shape in self._twins_spec:
            leaf = self
            for p in name.split("."):
                leaf = leaf.child(p)
            leaf.weight = nn.Parameter(torch.zeros(*shape), requires_grad=False)
            leaf.bias = nn.Parameter(torch.zeros(shape[0]), requires_grad=False)
        self._spec = conv_spec(cfg)
        for name, cout, cin, kh, kw in self._spec:
            leaf = self
            for p in name.split("."):
                leaf = leaf.child(p)
            leaf.weight = nn.Parameter(torch.zeros(cout, cin, kh, kw), requires_grad=False)
            if name not in GMA_NO_BIAS:
                leaf.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        if self.gma:
            self.child("update_block").child("aggregator").gamma = nn.Parameter(torch.zeros(1), requires_grad=False)
        self._packed = None
        self._packed_key = None
        self._packed_serial = 0
        self._ws = {}
        self._graphs = {}
        self._side2 = {}      # per device: the stream of the flow half of the motion encoder (_iteration)
        self._pyr_free = []
        self._side = {}                # per device: the stream the next window's encoders run on (prefetch_frames)
        self._prefetch_done = None     # event: the last prefetch's launches
        self._prefetch_dev = None
        self._pre_body = None          # event: the last field's inputs are ready, its iterations not yet queued
        import collections
        self._feat_cache = collections.OrderedDict()
        self.iter0_stats = {"warm": 0, "cold": 0}       # windows that reused / filled the iteration-zero store
        self.iter0_last = None                          # (warm, slots of the centre frames) of the last such window

    # ------------------------------------------------------------------ weights
    def _param(self, name):
        node = self
        for p in name.split("."):
            node = node._modules[p]
        return node

    def _pack(self, device):
        """Repack every conv weight into the kernels' [cout][kh][kw][cin] order (once per load)."""
        split = self._split()
        if self.sk and not split:
            raise ValueError("the SK update block is built on the split-f16 kernels: cfg.precision 'f32' cannot run a "
                             "checkpoint that has it")
        if self.twins and not split:
            raise ValueError("the Twins-SVT encoders are built on the split-f16 kernels: cfg.precision 'f32' cannot run a "
                             "checkpoint that has them")
        key = (str(device), split, self._plan_key(), tuple(p._version for p in self.parameters()),
               tuple(p.data_ptr() for p in self.parameters()))
        if self._packed is not None and self._packed_key == key:
            return self._packed
        self._join_prefetch()          # (a prefetch in flight reads the planes this call replaces)
        P, cblock_names, cb64_names = {}, set(), set()
        cout_packed = {}       # layers whose packed matrix has another row count than their bias
        rows7 = set()          # convf1 as a 7x1 convolution over the horizontal taps' rows
        block_of = self._block_of(split, cb64_names)
        sk_names = self._pack_sk(P, device, block_of, cblock_names, cout_packed) if self.sk else ()
        tw_raw = self._pack_twins(P, device, block_of, cblock_names, cout_packed) if self.twins else {}
        for name, cout, cin, kh, kw in self._spec:
            if name in sk_names:
                continue
            leaf = self._param(name)
            w = leaf.weight.detach().to(device=device, dtype=torch.float32)
            if name.endswith(".encoder.convc1"):
                # input columns of the configured lookup (a sub-window / sub-pyramid of the checkpoint's
                # base lookup under --fast); each direction's block is padded to whole float4s /
                # split-row units with zero weights
                base = cin // 2
                sel = torch.tensor(corr_channel_subset(self.cfg.corr_levels, self.cfg.corr_radius), device=device)
                cor = sel.numel()
                cor_p = cor_pad(cor, split)
                wp = torch.zeros(cout, 2 * cor_p, 1, 1, device=device)
                wp[:, :cor] = w[:, sel]
                wp[:, cor_p:cor_p + cor] = w[:, base + sel]
                w = wp
            if name.endswith(".flow_head.conv2") and split and cout == 4 and (kh, kw) == (3, 3):
                # 3x3 to four channels as a 1x1 to 36 (tap-major) + vfml_tapsum3x3: nine times fewer MFMA steps than a
                # 3x3 convolution padded to a 32-column tile
                w = w.permute(2, 3, 0, 1).reshape(36, cin, 1, 1).contiguous()
                cout_packed[name] = 36
            if name.endswith(".encoder.convf1") and split and (cin, kh, kw) == (4, 7, 7):
                # 7x7 over the 4-channel flow as 7x1 over 32 channels = the seven horizontal taps' quads per pixel
                # (vfml_flow_rows7): [cout][kx*4 + c][ky][1], channels 28..31 zero
                w7 = torch.zeros(cout, 32, 7, 1, device=device)
                w7[:, :28, :, 0] = w.permute(0, 3, 1, 2).reshape(cout, 28, 7)
                w = w7
                rows7.add(name)
            if name.endswith(".tprop"):
                # 1x1 conv over [prev | cur | next] motion features == 3x1 conv along the frame axis
                w = w.reshape(cout, 3, cin // 3, 1).permute(0, 2, 1, 3)  # -> [cout, cin/3, kh=3, kw=1]
            # update-block convolutions read split-row activations (all but convf1, whose input is the
            # 4-channel f32 flow), and so do the encoders behind their 4-channel stem: those weights go in
            # channel-block K order (include/vfml.h)
            cb = split and (name == "att.to_qk" or (name.startswith("update_block.") and (not name.endswith(".convf1") or name in rows7)) or
                            (name.split(".")[0] in ("fnet", "cnet") and name.count(".") > 1) or
                            name in ("fnet.conv2", "cnet.conv2"))
            if cb:
                cblock_names.add(name)
                cb = block_of(name, w.shape[1], w.shape[1], cout)
            if name in GMA_NO_BIAS:
                cout_packed[name] = cout
            P[name] = (pack_conv_weight(w, cin_pad=4 if cin == 3 else None, cblock=cb),
                       leaf.bias.detach().to(device=device, dtype=torch.float32).contiguous() if name not in GMA_NO_BIAS else None)
        self._pack_gates(P, device, split, block_of, cblock_names, () if self.sk else ("1", "2"))   # (SK: `gru` is a PCBlock)
        if split:
            self._split_planes(P, device, cblock_names, cb64_names, cout_packed)
            for enc in () if self.twins else ("fnet", "cnet"):
                leaf = self._param(f"{enc}.conv1")
                if tuple(leaf.weight.shape) == (64, 3, 7, 7):
                    with torch.cuda.device(device):
                        P[f"{enc}.conv1.stem"] = (hip.pack_stem_weight(leaf.weight, device),
                                                  leaf.bias.detach().to(device=device, dtype=torch.float32).contiguous())
        P.update(tw_raw)       # (f32 operands of the vector-ALU kernels: no planes)
        self._tapsum = any(n.endswith(".flow_head.conv2") for n in cout_packed)
        self._rows7 = bool(rows7)
        if self.gma:
            if not split:
                raise ValueError("the GMA aggregator is built on the split-f16 kernels: cfg.precision 'f32' cannot run a "
                                 "checkpoint that has it")
            self._gamma = float(self._param("update_block.aggregator").gamma.item())   # read once per load: .item() synchronises
        self._packed, self._packed_key = P, key
        self._graphs.clear()              # captured launches hold the old planes' addresses
        self._packed_serial += 1          # new weights: cached encoder outputs are stale
        self._feat_cache.clear()
        return P

    def _block_of(self, split, cb64_names):
        def block_of(layer, c0, ctot, cout):
            """K-axis block of a split-row layer's weight planes: 64 channels where the layer runs one MFMA per product
            over whole 64-channel blocks, more than 32 outputs wide (the kernel then steps 64 channels of hi halves at a
            time: include/vfml.h VFML_KORDER_CBLOCK64), else 32."""
            if split and self._nm(layer) == 1 and c0 % 64 == 0 and ctot % 64 == 0 and cout > 32:
                cb64_names.add(layer)
                return 64
            return True
        return block_of

    def _pack_gates(self, P, device, split, block_of, cblock_names, passes=("1", "2")):
        """GRU gates.  Input channels are [h | inp | motion | temporal]; `inp` (the context map) does not
        change over the iterations, so its part of every gate convolution (+ bias) is computed once per
        frame and added in the epilogue ("addend"): P[gate + ".ctx"]; the per-iteration convolutions, P[gate + ".iter"],
        see [h | motion | temporal] only (K 2560 -> 1920).  z and r share their input: one conv with 2*hidden outputs."""
        hid = self.hidden_dim
        self._cout_of = {}
        for k in passes:
            self._cout_of[f"update_block.gru.convzr{k}.iter"] = 2 * hid
            self._cout_of[f"update_block.gru.convq{k}.iter"] = hid
            raw = {g: self._param(f"update_block.gru.conv{g}{k}") for g in "zrq"}
            wzr = torch.cat([raw["z"].weight, raw["r"].weight]).detach().to(device=device, dtype=torch.float32)
            bzr = torch.cat([raw["z"].bias, raw["r"].bias]).detach().to(device=device, dtype=torch.float32)
            wq = raw["q"].weight.detach().to(device=device, dtype=torch.float32)
            bq = raw["q"].bias.detach().to(device=device, dtype=torch.float32)
            for nm, wfull, bfull in ((f"update_block.gru.convzr{k}", wzr, bzr), (f"update_block.gru.convq{k}", wq, bq)):
                it = torch.cat([wfull[:, :hid], wfull[:, 2 * hid:]], dim=1)
                P[nm + ".iter"] = (pack_conv_weight(it, cblock=block_of(nm + ".iter", hid, it.shape[1], it.shape[0]) if split else False), None)
                P[nm + ".ctx"] = (pack_conv_weight(wfull[:, hid:2 * hid], cblock=block_of(nm + ".ctx", hid, hid, wfull.shape[0]) if split else False),
                                  bfull.contiguous())
                if split:
                    cblock_names.update((nm + ".iter", nm + ".ctx"))
            for g in "zrq":
                del P[f"update_block.gru.conv{g}{k}"]

    def _split_planes(self, P, device, cblock_names, cb64_names=(), cout_packed={}):
        """split-f16 planes (hi, lo*2^11) of every [cout][K] matrix of P, made once per load.  cout_packed: layers whose
        packed matrix has another row count than their bias."""
        with torch.cuda.device(device):
            for name, (wflat, b) in list(P.items()):
                if is_depthwise(name):      # [c][k][k] f32 with their bias: the vector-ALU kernel's operands, no planes
                    continue
                cout = self._cout_of[name] if name in self._cout_of else cout_packed[name] if name in cout_packed else b.numel()
                sc = hip.SplitWeight.auto_scale(float(wflat.abs().max()))
                sw = hip.SplitWeight(cout, wflat.numel() // cout, device).fill(wflat, scale=sc)
                sw.order = (hip.KORDER_CBLOCK64 if name in cb64_names else
                            hip.KORDER_CBLOCK if name in cblock_names else hip.KORDER_TAP)
                P[name] = (sw, b)

    sk = False                 # (class defaults: engines that share this class's plumbing but have no such block)
    _sk_blocks = {}
    twins = False

    def _pack_twins(self, P, device, block_of, cblock_names, cout_packed):
        """The Twins-SVT encoders' weights: every linear layer, and the patch and reduction convolutions (kernel = stride, so
        a 1x1 over the space-to-depth rows [ky][kx][channel]), as [cout][K] matrices in the dense kernel's K order, into P
        (split into planes by _pack).  Returns what stays f32 - LayerNorm (gamma, beta) and the depthwise position encodings
        ([c][3][3], bias) - for _pack to add behind the planes."""
        raw = {}
        for name, kind, shape in self._twins_spec:
            leaf = self._param(name)
            w = leaf.weight.detach().to(device=device, dtype=torch.float32)
            b = leaf.bias.detach().to(device=device, dtype=torch.float32).contiguous()
            if kind == "ln":
                raw[name] = (w.contiguous(), b)
                continue
            if kind == "dw":
                raw[name] = (w.reshape(-1).contiguous(), b)
                continue
            if kind == "conv":
                cout, cin, k, _ = shape
                w = w.permute(0, 2, 3, 1)
                if cin % 4:
                    w = torch.nn.functional.pad(w, (0, 4 - cin % 4))      # (the frames are NHWC4)
                w = w.reshape(cout, -1)
            w = w.reshape(w.shape[0], w.shape[1], 1, 1)
            cblock_names.add(name)
            cout_packed[name] = w.shape[0]
            P[name] = (pack_conv_weight(w, cblock=block_of(name, w.shape[1], w.shape[1], w.shape[0])), b)
        return raw

    def _twins_encoder(self, prefix, x, n, H, W, P, dev, out, ldo, out_off, epilogue, split, out_fmt=hip.FMT_F32):
        """Twins-SVT encoder on NHWC4 input x [n,H,W,4]; writes [n,H/8,W/8,256] into `out` - the
        contract of _encoder.  Token rows are split rows throughout; the dense layers run on vfml_conv2d_split (residuals
        through VFML_EPI_ADD_AUX), q | k | v leave them as f32 rows for the two attention kernels.  The patch and reduction
        convolutions do not overlap: a space-to-depth copy of the grid, then a 1x1."""
        S, F32 = hip.FMT_S16, hip.FMT_F32
        sv = f"{prefix}.svt"

        def buf(name, numel):
            return self._buf(f"tw_{name}", numel, dev)

        def dense(name, src, k, rows, dst, co, ldo_=None, dst_off=0, aux=None, fmt=S):
            wgt, b = P[name]
            hip.conv2d(src, k, k, 1, 1, rows, wgt, b, co, 1, 1, dst, ldo_ or co, out_off=dst_off,
                       epilogue=hip.EPI_ADD_AUX if aux is not None else hip.EPI_NONE, aux0=aux, ld_aux0=co if aux is not None else 0,
                       in_fmt=S, out_fmt=fmt, aux_fmt=S, mfma=self._nm(name))

        def norm(name, src, dst, rows, c):
            g, b = P[name]
            hip.layernorm_rows(src, c, dst, c, rows, c, g, b, in_fmt=S, out_fmt=S)

        def patches(grid, hh, ww, c, p, ho, wo):
            """[n][hh][ww][c] -> rows [n*ho*wo][p*p*c] of the p x p patches ([ky][kx][channel]; rows and columns behind
            ho * p, wo * p are dropped).  Whole channel rows move: split rows stay split rows."""
            g = grid[:n * hh * ww * c].view(n, hh, ww, c)[:, :ho * p, :wo * p]
            return g.reshape(n, ho, p, wo, p, c).permute(0, 1, 3, 2, 4, 5).reshape(-1)

        grid, hh, ww, cin = x, H, W, 4
        last = len(TWINS_STAGES) - 1
        for i, (p, _, c, heads, sr) in enumerate(TWINS_STAGES):
            h, w = hh // p, ww // p
            rows, k = n * h * w, p * p * cin
            src = patches(grid, hh, ww, cin, p, h, w)
            if i == 0:      # the frames are f32
                src16 = buf("in", rows * k)
                hip.to_s16(src, rows, k, k, src16, k)
                src = src16
            X, Y, T, A = (buf(f"{t}{i}", rows * c) for t in "xyta")
            Hd = buf(f"hid{i}", rows * 4 * c)          # the MLP's hidden rows; q | k | v (3c) and q (c) as f32 before them
            dense(f"{sv}.patch_embeds.{i}.proj", src, k, rows, X, c)
            norm(f"{sv}.patch_embeds.{i}.norm", X, X, rows, c)

            def mlp(b, src_, dst, final=False):
                norm(f"{b}.norm2", src_, T, rows, c)
                dense(f"{b}.mlp.fc1", T, c, rows, Hd, 4 * c)
                hip.gelu_rows(Hd, 4 * c, Hd, 4 * c, rows, 4 * c, in_fmt=S, out_fmt=S)
                if not final:
                    dense(f"{b}.mlp.fc2", Hd, 4 * c, rows, dst, c, aux=src_)
                elif epilogue == hip.EPI_NONE:
                    dense(f"{b}.mlp.fc2", Hd, 4 * c, rows, out, c, ldo_=ldo, dst_off=out_off, aux=src_, fmt=out_fmt)
                elif epilogue == hip.EPI_TANH_RELU:
                    fin = buf("fin", rows * c)
                    dense(f"{b}.mlp.fc2", Hd, 4 * c, rows, fin, c, aux=src_, fmt=F32)
                    v = fin.view(rows, c)
                    v[:, :split].tanh_()
                    v[:, split:].relu_()
                    if out_fmt == S:
                        hip.to_s16(fin, rows, c, c, out, ldo, dst_off=out_off)
                    else:
                        torch.as_strided(out, (rows, c), (ldo, 1), out_off).copy_(v)
                else:
                    raise ValueError(f"_twins_encoder: epilogue {epilogue} is not one the encoders end in")

            # blocks.i.0: locally-grouped attention over 7 x 7 windows, then the MLP
            b = f"{sv}.blocks.{i}.0"
            norm(f"{b}.norm1", X, T, rows, c)
            dense(f"{b}.attn.qkv", T, c, rows, Hd, 3 * c, fmt=F32)
            hip.window_attention(Hd, 3 * c, n, h, w, c, heads, TWINS_WS, P[f"{b}.attn.qkv"][1], A, c, out_fmt=S)
            dense(f"{b}.attn.proj", A, c, rows, Y, c, aux=X)
            mlp(b, Y, X)
            # pos_block.i: x + depthwise 3 x 3
            wgt, bias = P[f"{sv}.pos_block.{i}.proj.0"]
            hip.dwconv2d(X, c, n, h, w, c, 3, wgt, bias, Y, c, in_fmt=S, out_fmt=S, residual=True)
            # blocks.i.1: every query against the frame's sub-sampled keys and values, then the MLP
            b = f"{sv}.blocks.{i}.1"
            hr, wr = h // sr, w // sr
            rk = n * hr * wr
            if rk == 0:
                raise ValueError(f"Twins-SVT encoder: a {h} x {w} token grid has no {sr} x {sr} patch to reduce (frame too small)")
            norm(f"{b}.norm1", Y, T, rows, c)
            dense(f"{b}.attn.q", T, c, rows, Hd, c, fmt=F32)
            KR, KV = buf(f"r{i}", rk * c), buf(f"kv{i}", rk * 2 * c)
            dense(f"{b}.attn.sr", patches(T, h, w, c, sr, hr, wr), sr * sr * c, rk, KR, c)
            norm(f"{b}.attn.norm", KR, KR, rk, c)
            dense(f"{b}.attn.kv", KR, c, rk, KV, 2 * c, fmt=F32)
            hip.attention_shared_keys(Hd, c, KV, 2 * c, n, h * w, hr * wr, c, heads, A, c, out_fmt=S)
            dense(f"{b}.attn.proj", A, c, rows, X, c, aux=Y)
            mlp(b, X, Y, final=i == last)
            grid, hh, ww, cin = Y, h, w, c
        return hh, ww

    def _sk_padded(self, bname):
        """(positions of a PCBlock's channels in its padded rows, padded width, padded hidden width).  convc1 reads the
        lookup's rows, each direction's 324 channels in a block of cor_pad's 336; the hidden width (int(1.5 C)) is padded
        to whole 32-channel K steps of the dense kernel's uniform-step loader.  Pad channels carry zero weights and biases:
        gelu(0 + 0) = 0 keeps them zero through the block."""
        cin = self._sk_blocks[bname][0]
        hp = (pcblock_hidden(cin) + 31) // 32 * 32
        if bname.endswith(".encoder.convc1"):
            cor = cin // 2
            cp = cor_pad(cor, True)
            return torch.cat([torch.arange(cor), cp + torch.arange(cor)]), 2 * cp, hp
        return torch.arange(cin), cin, hp

    def _pack_sk(self, P, device, block_of, cblock_names, cout_packed):
        """The PCBlocks' weights into P: depthwise ones as flat [c][k][k] f32 with their bias, the dense 1x1 ones as padded
        [cout][cin] matrices in the dense kernel's K order (split into planes by _pack).  Returns the names handled."""
        done = set()

        def grow(t, dim, n, at):
            shape = list(t.shape)
            shape[dim] = n
            out = torch.zeros(shape, device=device)
            out.index_copy_(dim, at, t)
            return out
        for bname, (cin, cout, ks) in self._sk_blocks.items():
            pos, cp, hp = self._sk_padded(bname)
            pos = pos.to(device)
            hpos = torch.arange(pcblock_hidden(cin), device=device)
            opos = torch.arange(cout, device=device)

            def get(sub):
                leaf = self._param(f"{bname}.{sub}")
                return (leaf.weight.detach().to(device=device, dtype=torch.float32),
                        leaf.bias.detach().to(device=device, dtype=torch.float32))
            for i, k in enumerate(ks):
                w, b = get(f"conv_list.{i}")
                P[f"{bname}.conv_list.{i}"] = (grow(w.reshape(cin, k * k), 0, cp, pos).reshape(-1).contiguous(), grow(b, 0, cp, pos))
                done.add(f"{bname}.conv_list.{i}")
            for sub, (orow, on), (icol, inn) in (("ffn1.0", (hpos, hp), (pos, cp)), ("ffn1.2", (pos, cp), (hpos, hp)),
                                                 ("pw", (pos, cp), (pos, cp)), ("ffn2.0", (hpos, hp), (pos, cp)),
                                                 ("ffn2.2", (opos, cout), (hpos, hp))):
                name = f"{bname}.{sub}"
                w, b = get(sub)
                w = grow(grow(w, 0, on, orow), 1, inn, icol)
                cblock_names.add(name)
                cout_packed[name] = on
                P[name] = (pack_conv_weight(w, cblock=block_of(name, inn, inn, on)), grow(b, 0, on, orow).contiguous())
                done.add(name)
        return done

    def _sk_workspace(self, rows, dev):
        """The three scratch maps a PCBlock's launches pass through, sized for the widest block (allocated with cfg.sk only)."""
        cp = max(self._sk_padded(b)[1] for b in self._sk_blocks)
        hp = max(self._sk_padded(b)[2] for b in self._sk_blocks)
        return (self._buf("sk_a", rows * cp, dev), self._buf("sk_b", rows * cp, dev), self._buf("sk_hid", rows * hp, dev))

    def _pcblock(self, name, P, x, ld_x, x_off, n, h, w, out, ld_out, out_off, ws, out_fmt=hip.FMT_S16, gelu_out=False):
        """One PCBlock on n frames of h x w cells: split rows x (row stride ld_x, float offset x_off,
        read in place) -> out (ld_out, out_off; out_fmt).  Twelve launches: the dense 1x1 convolutions on vfml_conv2d_split
        (the residual of ffn1.2 and pw through VFML_EPI_ADD_AUX), a GELU pass behind four of them, the two depthwise
        convolutions with residual and GELU fused (vfml_dwconv2d).  ws: _sk_workspace's maps."""
        cin, cout, ks = self._sk_blocks[name]
        _, cp, hp = self._sk_padded(name)
        A, B, Hd = ws
        S, rows = hip.FMT_S16, n * h * w

        def dense(sub, src, c, ld, off, dst, co, ldo, dst_off=0, aux=None, ld_aux=0, aux_off=0, fmt=S):
            wgt, b = P[f"{name}.{sub}"]
            hip.conv2d(src, c, ld, n, h, w, wgt, b, co, 1, 1, dst, ldo, in0_off=off, out_off=dst_off,
                       epilogue=hip.EPI_ADD_AUX if aux is not None else hip.EPI_NONE, aux0=aux, ld_aux0=ld_aux, aux0_off=aux_off,
                       in_fmt=S, out_fmt=fmt, aux_fmt=S, mfma=self._nm(f"{name}.{sub}"))

        def gelu(t, ld, c, off=0, fmt=S):
            hip.gelu_rows(t, ld, t, ld, rows, c, x_off=off, out_off=off, in_fmt=fmt, out_fmt=fmt)

        def depthwise(i, src, dst):
            wgt, b = P[f"{name}.conv_list.{i}"]
            hip.dwconv2d(src, cp, n, h, w, cp, ks[i], wgt, b, dst, cp, in_fmt=S, out_fmt=S, residual=True, gelu=True)
        dense("ffn1.0", x, cp, ld_x, x_off, Hd, hp, hp)
        gelu(Hd, hp, hp)
        dense("ffn1.2", Hd, hp, hp, 0, A, cp, cp, aux=x, ld_aux=ld_x, aux_off=x_off)
        gelu(A, cp, cp)
        depthwise(0, A, B)
        depthwise(1, B, A)
        dense("pw", A, cp, cp, 0, B, cp, cp, aux=A, ld_aux=cp)
        gelu(B, cp, cp)
        dense("ffn2.0", B, cp, cp, 0, Hd, hp, hp)
        gelu(Hd, hp, hp)
        dense("ffn2.2", Hd, hp, hp, 0, out, cout, ld_out, dst_off=out_off, fmt=out_fmt)
        if gelu_out:
            gelu(out, ld_out, cout, off=out_off, fmt=out_fmt)

    PRECISIONS = ("f16x3", "f16x2", "f16", "mixed", "f32")

    def _precision(self):
        p = getattr(self.cfg, "precision", "f16x3")
        if p not in self.PRECISIONS:
            raise ValueError(f"cfg.precision must be one of {self.PRECISIONS}, got {p!r}")
        return p

    def _split(self):
        """Every arithmetic but 'f32' runs the split-f16 kernels on split-row activations; they differ in the
        number of MFMAs a layer spends per product (`_nm`)."""
        return self._precision() != "f32"

    def _nm(self, layer):
        """MFMAs per product for `layer` (a conv_spec name, '.iter' / '.ctx' for the two parts of a GRU gate
        convolution, or 'corr' for the correlation GEMMs): 3 = fp32-grade split product, 2 / "2w" = weights as plain f16,
        "2a" = activations as plain f16, 1 = both operands plain f16.  'f16x3' / 'f16x2' / 'f16' = 3 / 2 / 1 everywhere; 'mixed' = cfg.mfma_plan,
        {name prefix: count}, longest prefix wins, 3 where nothing matches."""
        p = self._precision()
        if p == "f16x3":
            nm = 3
        elif p == "f16x2":
            nm = 2
        elif p == "f16":
            nm = 1
        else:
            plan = self._mixed_plan()
            best, nm = -1, 3
            for prefix, n in plan.items():
                if layer.startswith(prefix) and len(prefix) > best and self._plan_applies(layer, prefix):
                    best, nm = len(prefix), (n if isinstance(n, str) else int(n))
            if nm == "2w":
                nm = 2
            if nm not in (1, 2, "2a", 3):
                raise ValueError(f"cfg.mfma_plan[{layer!r}] = {nm!r}: 1, 2 ('2w'), '2a' or 3")
        if layer == "corr" and nm in (2, "2a"):
            nm = 3       # a volume and its transpose must stay the same numbers: the symmetric forms only
        return nm

    def _plan_applies(self, layer, prefix):
        """An SK checkpoint's layers carry their parameter names (`update_block.encoder.convc1.ffn1.0`, ...), which the
        plain block's layer names prefix: an entry measured for the plain `convc1` must not reach the PCBlock of that name.
        A layer of a PCBlock (and the SK block's 1x1 convf1) takes the "" default or an entry that names it INSIDE its
        block (longer than the block's name); no plan shipped has one, and no EPE budget is claimed for SK under them."""
        if not self.sk:
            return True
        for b in list(self._sk_blocks) + ["update_block.encoder.convf1"]:
            if layer == b or layer.startswith(b + "."):
                return prefix == "" or len(prefix) > len(b)
        return True

    def _mixed_plan(self):
        """cfg.mfma_plan, or - as vfml/cfg.py says - DEFAULT_MIXED_PLAN when precision is 'mixed' and none is given
        (an explicit empty dict means "3 everywhere")."""
        plan = getattr(self.cfg, "mfma_plan", None)
        if plan is None:
            from .cfg import DEFAULT_MIXED_PLAN
            plan = DEFAULT_MIXED_PLAN
        return plan

    def _plan_key(self):
        """The arithmetic as part of a cached frame's identity."""
        p = self._precision()
        vol = getattr(self.cfg, "corr_volume", "f32")
        if vol not in self.CORR_VOLUMES:
            raise ValueError(f"cfg.corr_volume must be one of {tuple(self.CORR_VOLUMES)}, got {vol!r}")
        key = (p, tuple(sorted((k, str(v)) for k, v in self._mixed_plan().items()))) if p == "mixed" else p
        if self._tile() is None:
            key = (key, "row-major")
        return key if vol == "f32" else (key, vol)

    # cfg.corr_volume -> mask of the pyramid levels stored as one f16 per value (bit l = level l)
    CORR_VOLUMES = {"f32": 0, "f16": 15, "f16@1": 14, "f16@2": 12, "f16@3": 8}
    _VOL_TILE = hip.VolTile(2, 3)

    def _tile(self):
        """Layout of the correlation volumes: 4 x 8 tiles (hip.VolTile) on the split-row path - a lookup window then lies in
        ~8 lines of 128 bytes instead of ~13, 149 -> 107 us per lookup at 1080p (tools/exp/lookup_tiled.py) - for the price
        of whole edge tiles (+3.4 % GEMM columns at 1080p).  'f32': row-major."""
        if not self._split():
            return None
        return self._VOL_TILE

    # ------------------------------------------------------------------ workspace
    def _buf(self, name, numel, device, dtype=torch.float32, zero=False):
        """Named scratch buffer, cached per exact size (a resolution change reallocates)."""
        t = self._ws.get(name)
        if t is None or t.numel() != numel or t.device != device or t.dtype != dtype:
            if t is not None:
                self._graphs.clear()       # captured launches hold this buffer's address
                self._join_prefetch()      # (the encoders' workspaces are shared with a prefetch in flight)
            t = (torch.zeros if zero else torch.empty)(int(numel), device=device, dtype=dtype)
            self._ws[name] = t
        return t

    _prefetch_done = None      # (class defaults: engines that share this class's plumbing but never prefetch)
    _prefetch_dev = None

    def _join_prefetch(self):
        """Order the current stream behind a prefetch in flight (prefetch_frames): it runs on a side stream over workspaces,
        weights and cache entries that were allocated under this one - whatever frees or replaces any of them, or reads what
        the prefetch produces, has to come after it."""
        if self._prefetch_done is not None:
            torch.cuda.current_stream(self._prefetch_dev).wait_event(self._prefetch_done)
            self._prefetch_done = None

    def release_workspace(self):
        self._join_prefetch()
        self._graphs.clear()
        self._ws.clear()
        self._feat_cache.clear()
        self._ctx_store = None
        self._it0_store = None
        self._att_store = None

    # ------------------------------------------------------------------ the per-frame stores
    # Three results are computed once per frame and kept in device memory across the windows the frame is a centre of: the
    # gates' context parts, the GMA attention planes, the motion features of iteration 0.  Each store is a ring of frame
    # slots with the bookkeeping of vfml/frame_store.py (SlotRing: round-robin handout past the slots in use, the old
    # owner's `_feat_cache` entry evicted, a serial that marks the entries of a rebuilt store as stale).  The engine owns the
    # tensors and the rule by which a store is rebuilt - always behind a prefetch in flight (_join_prefetch).  Below, per
    # store, only what differs.
    _ctx_store = _att_store = _it0_store = None       # (class defaults: engines that share this class's plumbing build none)

    # ------------------------------------------------------------------ per-frame context parts of the gate convolutions
    # The context part of the four GRU gate convolutions is computed once per frame and ADDED by the gate convolutions of
    # every iteration of every window the frame is a centre of (vfml_conv_desc.addend): [centre frames][cells][256 | 128]
    # floats, 300 MB per 1080p window.  They live in ONE store per gate, its slots handed out in the order frames
    # arrive: the centre frames of a sliding job's window are then consecutive slots, and the gate convolutions - fixed
    # launches of a replayed graph - reach them through a device cell that holds the window's first slot
    # (vfml_conv_desc.addend_ind).  Nothing is gathered per field (round 2: twelve device copies, 0.6 GB of traffic).  The
    # first slots are mirrored behind the ring so that a window that wraps is consecutive too (frame_store.window_base); a
    # window whose centres are not in arrival order (random access) is gathered into slots kept for that, behind the mirror.
    CTX_RING = 12            # >= FEATURE_CACHE_FRAMES: a cached context entry owns its slot until the ring comes round
    CTX_GATES = (("zr1", 256), ("q1", 128), ("zr2", 256), ("q2", 128))

    def _context_store(self, dev, Pn, M):
        st = self._ctx_store
        if st is None or st.key != (str(dev), Pn) or st.M < M:
            self._join_prefetch()
            # (a coming window's centres are prefetched while the current one's are being read: two windows' worth and some)
            R = max(self.CTX_RING, 2 * M + 4)
            for k in [k for k in self._feat_cache if k[0] == "c"]:     # (entries of another store)
                del self._feat_cache[k]
            st = self._ctx_store = types.SimpleNamespace(
                key=(str(dev), Pn), M=M, ring=SlotRing("context", R, self._feat_cache),
                S={g: torch.empty((R + 2 * M - 1) * Pn * co, device=dev) for g, co in (() if self.sk else self.CTX_GATES)})
        return st

    # ------------------------------------------------------------------ per-frame attention of the GMA aggregator
    # attn = softmax(q k^T / sqrt(128)) over the cells of ONE centre frame, q | k = att.to_qk(inp): it depends on the frame's
    # context map alone, so it is built beside the gates' context parts (_frame_context) and kept like them - in a slot of a
    # ring, named by the frame's context cache entry (FrameContext.att_slot: this ring evicts "c" entries too), reused by
    # every window the frame is a centre of.  Two forms, chosen by _attention_geometry for this engine and for MemFlow
    # (update_block.attention_readout reads both): the probabilities times ATT_SCALE as ONE f16 each, the weight plane
    # (hip.PlainWeight) of a long-K GEMM (2.1 GB per 1080p frame), or - small or odd frames - as split rows.
    # The read-out GEMMs are fixed launches of the replayed graph and take the plane's ADDRESS, so the window's slots are part
    # of the graph's key; the ring is therefore short (M + 2: a window's centres, the centre a prefetch adds, one spare) and a
    # sliding job comes back to the same slots, and graphs, every M + 2 fields.
    ATT_DIM = 128
    gma = False                # (class default: engines that share this class's plumbing but have no such block)

    @staticmethod
    def _attention_geometry(Pn):
        """(row length of the probabilities in whole 8-cell units, their row stride, plain-f16 form?)"""
        P8 = (Pn + 7) // 8 * 8
        ldA = (P8 + 63) // 64 * 64
        plain = Pn >= 1024 and Pn % 4 == 0 and Pn * ldA * 2 <= 0x7ffffff0 and ldA <= 32768
        return P8, ldA, plain

    def _attention_store(self, dev, Pn, M):
        st = self._att_store
        if st is None or st.key != (str(dev), Pn) or st.ring.R < M + 2:
            self._join_prefetch()
            self._graphs.clear()           # captured read-outs hold the old planes' addresses
            self._att_store = None         # (let the old planes go before the new ones are asked for)
            P8, ldA, plain = self._attention_geometry(Pn)
            R = M + 2
            st = self._att_store = types.SimpleNamespace(
                key=(str(dev), Pn), ring=SlotRing("attention", R, self._feat_cache), plain=plain, P8=P8, ldA=ldA,
                k=None if plain else hip.SplitWeight(Pn, self.ATT_DIM, dev),
                vt=None if plain else hip.SplitWeight(self.ATT_DIM, P8, dev),
                A=[hip.PlainWeight(Pn, ldA, dev, scale=ATT_SCALE) if plain else torch.empty(Pn * ldA, device=dev)
                   for _ in range(R)])
        return st

    def _build_attention(self, st, slot, cx, h8, w8, Pn, P, dev, AF):
        """The attention of one frame (context map cx, [Pn][256] rows) into slot `slot` of the store."""
        AD, ldA = self.ATT_DIM, st.ldA
        wgt, _ = P["att.to_qk"]
        nmq = self._nm("att.to_qk")
        if st.plain:
            # q | k as f32 rows of one map, then the plane in one call: scores and softmax on chip (csrc/attention.hip)
            qk = self._buf("att_qk", Pn * 2 * AD, dev)
            hip.conv2d(cx, 128, 256, 1, h8, w8, wgt, None, 2 * AD, 1, 1, qk, 2 * AD, in0_off=128, in_fmt=AF, mfma=nmq)
            hip.attention_plane(qk, qk, Pn, st.A[slot], score_scale=1.0 / float(AD) ** 0.5, d=AD, ld_q=2 * AD, ld_k=2 * AD,
                                k_off=AD, workspace=self._buf("att_stats", 2 * Pn, dev))
            return
        # small or odd frames: q (rows 0..127 of to_qk) as the score GEMM's split-row operand, k (rows 128..255) as f32 for its
        # weight planes, f32 scores, row softmax to split rows - MemFlow's path
        qmap = self._buf("att_q", Pn * AD, dev)
        kmap = self._buf("att_k", Pn * AD, dev)
        hip.conv2d(cx, 128, 256, 1, h8, w8, wgt, None, AD, 1, 1, qmap, AD, in0_off=128, in_fmt=AF, out_fmt=AF, mfma=nmq)
        hip.conv2d(cx, 128, 256, 1, h8, w8, wgt, None, AD, 1, 1, kmap, AD, in0_off=128, weight_off=AD, in_fmt=AF, mfma=nmq)
        kw_ = st.k.fill(kmap, scale=16.0)
        scores = self._buf("att_scores", Pn * ldA, dev)
        hip.conv2d(qmap, AD, AD, 1, 1, Pn, kw_, None, Pn, 1, 1, scores, ldA, out_scale=1.0 / float(AD) ** 0.5, in_fmt=AF)
        hip.softmax_rows_s16(scores, Pn, Pn, ldA, st.A[slot], ldA, scale=ATT_SCALE)

    # ------------------------------------------------------------------ per-frame motion features of iteration 0
    # At iteration 0 the flow is zero and the lookups, convc1, convc2, the flow half and encoder.conv act on every centre
    # frame by itself: the `mf` columns of the state after them depend on the frame and its two neighbours only, and a frame
    # is a centre of M consecutive windows of a sliding job.  Each centre's rows ([cells][128] floats in the update block's
    # activation format, 16.6 MB at 1080p) are kept in a ring of slots (frame_store.Iter0Ring: the entry's key names the
    # frame AND its two neighbours); a window whose older centres all have theirs runs those five launches of iteration 0
    # on its newest centre alone ("warm").  The captured launch that moves the rows (vfml_window_seed) reaches the slots
    # through device cells, so one graph serves every window.
    # Eight slots: a sliding job takes one per field and reads the two taken before it.  Jobs that interleave more streams
    # of windows than that (the six tiles of a 4K frame walked frame by frame) find their entries evicted and run cold - as
    # before, plus the 25 us store.
    ITER0_RING = 8
    iter0_store = True       # False: every window computes iteration 0 for all its centres (tests, A/B runs)

    def _iter0_store(self, dev, Pn, M):
        st = self._it0_store
        if st is None or st.key != (str(dev), Pn) or st.ring.R < M + 1:
            self._join_prefetch()
            for k in [k for k in self._feat_cache if k[0] == "m"]:     # (entries of another store)
                del self._feat_cache[k]
            R = max(self.ITER0_RING, M + 1)
            st = self._it0_store = types.SimpleNamespace(key=(str(dev), Pn), ring=Iter0Ring(R, self._feat_cache),
                                                         S=torch.empty(R * Pn * 128, device=dev))
        return st

    # ------------------------------------------------------------------ graph replay of the iteration body
    GRAPHS_KEPT = 8

    def _use_graph(self):
        use = getattr(self.cfg, "use_graph", None)
        if use is None:
            use = os.environ.get("VFML_GRAPH", "1") != "0"
        return bool(use) and hip._PROFILE is None       # (per-launch events of the roofline pass cannot be captured)

    def _run_body(self, body, key, dev):
        """Run `body` (a fixed sequence of kernel launches on fixed buffers): eagerly the first time a configuration
        is seen (workspaces get allocated, kernel attributes set), captured into a HIP graph the second time, replayed
        afterwards.  The launches go to torch's current stream through the C ABI, which during capture is the capture
        stream.  Anything that moves a buffer the launches address (a workspace reallocation, new weights) drops the
        graphs."""
        if not self._use_graph():
            body()
            return
        st = self._graphs.get(key)
        if st is None:
            body()
            while len(self._graphs) >= self.GRAPHS_KEPT:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = "seen"
            return
        if st == "seen":
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                body()
            self._graphs[key] = st = g
        st.replay()

    # ------------------------------------------------------------------ encoder
    def _encoder(self, prefix, x, n, H, W, P, dev, out, ldo, out_off, epilogue, split, out_fmt=hip.FMT_F32):
        """RAFT BasicEncoder on NHWC4 input x [n,H,W,4]; writes [n,H/8,W/8,256] into `out`."""
        h2, w2 = H // 2, W // 2
        big = n * h2 * w2 * 64
        raw = self._buf("enc_raw", big, dev)
        raw2 = self._buf("enc_raw2", big, dev)
        act = [self._buf("enc_act0", big, dev), self._buf("enc_act1", big, dev), self._buf("enc_act2", big, dev)]
        st = self._buf("enc_stats", 3 * n * 128 * 2, dev)
        nws = hip.instnorm_workspace_bytes(n, h2 * w2, 128)
        ws = self._buf("enc_statws", (nws + 7) // 8, dev, torch.float64)

        def stats_of(t, hw, c, slot):
            s = st[slot * n * 128 * 2:]
            hip.instnorm_stats(t, n, hw, c, s, ws)
            return s

        # split-f16 path: activations are split rows (written by instnorm_apply, read by the LDS-DMA convolution
        # kernel); every convolution leaves per-block sums of its raw result behind (its tile is in LDS anyway) and
        # only the fold remains.  Blocks (128 output pixels after the f32-source stem, 32 after split-row sources)
        # must not straddle frames.  Measured at 1080p against f32 rows split while register-staged: 0.2 ms per field
        # faster (26.27 / 26.26 vs 26.42 / 26.50 ms, profiles/r02_kernel_anatomy.md).
        split_prec = self._split()
        AF = hip.FMT_S16 if split_prec else hip.FMT_F32
        part_len = n * ((h2 * w2 + 31) // 32) * 64 * 2            # largest layer: half resolution, 64 channels
        parts = self._buf("enc_part", 3 * part_len, dev, torch.float64) if split_prec else None
        # (the norm fold's first pass; like every encoder workspace it belongs to this engine, and whatever runs the
        # encoders on another stream - prefetch_frames - is ordered against the main stream's use by _join_prefetch)
        fold_ws = self._buf("enc_foldws", min(n, 8) * 64 * 128 * 2, dev, torch.float64) if split_prec else None

        def conv_stats(src, c, hh_, ww_, name, planes, dst, slot, k, stride=1, pad=0, src_fmt=hip.FMT_F32):
            wgt, b = P[name]
            nm = self._nm(name) if split_prec else 3
            ho_, wo_ = (hh_ + 2 * pad - k) // stride + 1, (ww_ + 2 * pad - k) // stride + 1
            hw = ho_ * wo_
            rows = hip.STATS_ROWS_S16 if src_fmt == hip.FMT_S16 else hip.STATS_ROWS_F32
            if not (split_prec and (n == 1 or hw % rows == 0)):
                hip.conv2d(src, c, c, n, hh_, ww_, wgt, b, planes, k, k, dst, planes, stride=stride, pad_h=pad, pad_w=pad,
                           mfma=nm, in_fmt=src_fmt)
                return stats_of(dst, hw, planes, slot)
            chunks = (hw + rows - 1) // rows
            part = parts[slot * part_len:]
            if (c == 64 and planes == 64 and k == 3 and stride == 1 and pad == 1 and nm == 3 and src_fmt == hip.FMT_S16
                    and ww_ % 32 == 0 and getattr(wgt, "order", None) == hip.KORDER_CBLOCK and wgt.kp == 576 and wgt.lo is not None):
                # the residual blocks of layer1: persistent workgroups, weights in registers, one patch per tile (same bits)
                hip.conv3x3_c64(src, c, n, hh_, ww_, wgt, b, dst, planes, stats_part=part)
            else:
                hip.conv2d(src, c, c, n, hh_, ww_, wgt, b, planes, k, k, dst, planes, stride=stride, pad_h=pad, pad_w=pad,
                           stats_part=part, mfma=nm, in_fmt=src_fmt)
            s = st[slot * n * 128 * 2:]
            hip.instnorm_finalize(part, n, chunks, planes, hw, s, workspace=fold_ws)
            return s

        stem = P.get(f"{prefix}.conv1.stem")
        if stem is not None and split_prec and self._nm(f"{prefix}.conv1") == 3:
            # the 7x7 / 2 stem as one patch-resident kernel (csrc/stem.hip): its statistics partials are one chunk per
            # 8 x 64-pixel output tile
            chunks = hip.stem_chunks(H, W)
            part = parts[0:]
            hip.stem7x7s2(x, n, H, W, stem[0], stem[1], raw, stats_part=part)
            s0 = st[0:]
            hip.instnorm_finalize(part, n, chunks, 64, h2 * w2, s0, workspace=fold_ws)
        else:
            s0 = conv_stats(x, 4, H, W, f"{prefix}.conv1", 64, raw, 0, 7, stride=2, pad=3)
        cur = act[0]
        hip.instnorm_apply(raw, s0, n, h2 * w2, 64, cur, out_fmt=AF)
        ch, hh, ww, ci = 64, h2, w2, 0
        for li, (planes, stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
            for bi in range(2):
                stv = stride if bi == 0 else 1
                ho, wo = (hh, ww) if stv == 1 else ((hh - 1) // 2 + 1, (ww - 1) // 2 + 1)
                name = f"{prefix}.layer{li}.{bi}"
                y = act[(ci + 1) % 3]
                nxt = act[(ci + 2) % 3]
                s1 = conv_stats(cur, ch, hh, ww, f"{name}.conv1", planes, raw, 0, 3, stride=stv, pad=1, src_fmt=AF)
                hip.instnorm_apply(raw, s1, n, ho * wo, planes, y, out_fmt=AF)
                s2 = conv_stats(y, planes, ho, wo, f"{name}.conv2", planes, raw, 1, 3, pad=1, src_fmt=AF)
                if stv != 1:
                    s3 = conv_stats(cur, ch, hh, ww, f"{name}.downsample.0", planes, raw2, 2, 1, stride=stv, src_fmt=AF)
                    hip.instnorm_apply(raw, s2, n, ho * wo, planes, nxt, res=raw2, res_stats=s3, out_fmt=AF)
                else:
                    hip.instnorm_apply(raw, s2, n, ho * wo, planes, nxt, res=cur, out_fmt=AF)
                cur, ci = nxt, (ci + 2) % 3
                ch, hh, ww = planes, ho, wo
        wgt, b = P[f"{prefix}.conv2"]
        hip.conv2d(cur, 128, 128, n, hh, ww, wgt, b, 256, 1, 1, out, ldo, out_off=out_off, epilogue=epilogue,
                   split=split, out_fmt=out_fmt, in_fmt=AF, mfma=self._nm(f"{prefix}.conv2") if split_prec else 3)
        return hh, ww

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, images, data=None, return_lowres=True):
        """images: float [B=1, N, 3, H, W] on the GPU (the tensor the reference builds at
        processing/videoflow_processor.py:160-161). Returns (flow [1, 2(N-2), 2, H, W], low-res flows)."""
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise RuntimeError("MOFNetHIP runs on an MI355X (HIP) device only; got "
                               f"{getattr(images, 'device', type(images))}. There is no CPU fallback in the shipped engine.")
        if images.dim() != 5 or images.shape[2] != 3:
            raise ValueError(f"images must be [B,N,3,H,W], got {tuple(images.shape)}")
        if images.shape[0] != 1:
            raise ValueError(f"Batch size must be 1, got {images.shape[0]}")
        src = images[0]
        if src.dtype != torch.float32:
            src = src.float()
        return self._run(src.contiguous(), src.shape[0], src.shape[2], src.shape[3], return_lowres)

    @torch.no_grad()
    def forward_u8(self, frames, return_lowres=True, frame_keys=None, tri_batch=False, pick_only=False, dense_corr=False):
        """frames: uint8 [N, H, W, 3] RGB on the GPU; /255 happens in the K1 kernel (same fp32 ops
        as the reference's host-side conversion), saving the 4x larger float upload.

        frame_keys: optional list of N hashable ids, one per frame.  The encoders act on each frame
        independently (instance norm is per image), so their outputs depend on the frame alone:
        with keys the engine keeps the per-frame feature maps, pooled target pyramids and context
        maps of recently seen frames and encodes only the frames it has not seen - in a sliding
        window that is 1 of N.  The caller promises that equal keys mean equal pixels.

        tri_batch (tri-frame networks, `--vf-architecture bof`): the N frames are B = N-2 overlapping triples
        (j-1, j, j+1) - B consecutive fields of a job in one pass, every centre frame its own problem; the
        output holds their 2B flows (forward flows first), field j's pick is flow B + j.  Same values as B
        separate calls; at 720p one triple fills a third of the chip.

        pick_only (with return_lowres=False): return only the flow the reference takes from the output,
        `[0, shape[1]//2]` = the backward flow of the first centre frame, as [1, 1, 2, H, W]; the last
        iterations then skip the centre frames that can no longer influence it (same bits for that flow).

        dense_corr: build every correlation pyramid's level 0 whole, whatever `corr_on_demand` says (the crops of a tiled
        job; same bits)."""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8
                and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError("forward_u8 expects a uint8 [N,H,W,3] device tensor")
        if frame_keys is not None and len(frame_keys) != frames.shape[0]:
            raise ValueError("frame_keys must have one entry per frame")
        if tri_batch and not self.tri_frame:
            raise ValueError("tri_batch applies to tri-frame (BOF) networks")
        return self._run(frames.contiguous(), frames.shape[0], frames.shape[1], frames.shape[2], return_lowres,
                         frame_keys, tri_batch, pick_only and not return_lowres, dense_corr)

    # ------------------------------------------------------------------ per-frame encoder cache
    FEATURE_CACHE_FRAMES = 12
    FMAP_ROW_SCALE = 16.0       # power of two: exact; undone by the correlation GEMM's out_scale

    def clear_feature_cache(self):
        self._join_prefetch()
        self._feat_cache.clear()
        self._pyr_free = []

    def prefetch_frames(self, frames, frame_keys):
        """The encoders a COMING window will need - feature maps / target planes of its frames, context maps of its centre
        frames, whatever of them is not cached yet - queued on a side stream, behind the inputs of the field just launched
        and BESIDE its update iterations: the encoders' short-K convolutions and HBM-bound norm passes fill what the
        iterations' MFMA-bound launches leave idle (tails of half-empty rounds, memory bandwidth).  Same kernels, same
        inputs: the cached results are the bits a later forward_u8 would compute itself.  frames: uint8 [N,H,W,3] of the
        coming window, frame_keys as for forward_u8.

        ON by default (VFML_PREFETCH=0 turns it off; VFML_PREFETCH_DBG=serial queues the same work BEHIND the field -
        what bench.py's per-launch roofline pass does, so that every timed launch has the GPU to itself).  Fields are
        bit-identical with and without it (tests/test_gpu_e2e.py::test_prefetched_encoders_give_the_same_fields); they were
        not while the fixed-radius lookup mixed its samples with a packed-f32 op straight behind a ds_read, which reads a
        stale register when another kernel's MFMAs share the SIMD (profiles/r02_kernel_anatomy.md section 7)."""
        if (frame_keys is None or self._pre_body is None or os.environ.get("VFML_PREFETCH", "1") == "0" or self.tri_frame):
            return
        cfg = self.cfg
        N, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        if N < 3 or H % 8 or W % 8 or len(frame_keys) != N:
            return
        L, dev = cfg.corr_levels, frames.device
        h, w = H // 8, W // 8
        AF = hip.FMT_S16 if self._split() else hip.FMT_F32
        geo = self._volume_geometry(H, W, L, AF)
        hl, wl, Sl = geo.hl, geo.wl, geo.Sl
        keys = [(k, H, W, L, self._plan_key(), self._packed_serial) for k in frame_keys]
        need_f = [j for j in range(N) if ("f", keys[j]) not in self._feat_cache]
        need_c = [j for j in range(1, N - 1) if ("c", keys[j]) not in self._feat_cache]
        if not need_f and not need_c:
            return
        main = torch.cuda.current_stream(dev)
        side = self._side.get(dev)
        if side is None:
            side = self._side[dev] = torch.cuda.Stream(device=dev)
        P = self._pack(dev)
        if "serial" in os.environ.get("VFML_PREFETCH_DBG", ""):
            side.wait_stream(main)
        else:
            side.wait_event(self._pre_body)
        frames.record_stream(side)       # (a view of the caller's clip: its block must outlive the side stream's reads)
        with torch.cuda.stream(side):
            new = []
            if need_f:
                new += list(self._frame_features(frames, need_f, keys, H, W, P, dev, L, hl, wl, Sl, vt=geo.VT).values())
            if need_c:
                new += list(self._frame_context(frames, need_c, keys, H, W, P, dev, h * w, N - 2).values())
            done = torch.cuda.Event()
            done.record(side)
        # the cached tensors were allocated on the side stream and will be read (and one day freed) under the main one

        def walk(x):
            if isinstance(x, torch.Tensor):
                x.record_stream(main)
            elif isinstance(x, (list, tuple)):
                for y in x:
                    walk(y)
            elif isinstance(x, dict):
                for y in x.values():
                    walk(y)
            elif hasattr(x, "planes") and isinstance(getattr(x, "planes"), torch.Tensor):
                x.planes.record_stream(main)
        walk(new)
        self._prefetch_done, self._prefetch_dev = done, dev

    def _pyramid_buffers(self, sizes, dev, limit):
        """Level buffers for a new correlation pyramid (5.6 GB at 1080p).  When the pyramid cache is at its
        limit the least recently used pyramid is retired FIRST and its buffers are handed to the new one:
        in the steady state of a sliding job no field allocates (a 5.6 GB hipMalloc costs up to 150 ms, and
        retiring only after the new allocation made the third field of every job pay for one)."""
        while sum(1 for k in self._feat_cache if k[0] == "p") >= limit:
            oldest = next(k for k in self._feat_cache if k[0] == "p")
            self._pyr_free.append(self._feat_cache.pop(oldest))
        for i, bufs in enumerate(self._pyr_free):
            if [b.numel() for b in bufs] == sizes and bufs[0].device == dev:
                return self._pyr_free.pop(i)
        del self._pyr_free[:]          # other geometry: let the allocator have the memory back
        return [torch.empty(n, device=dev) for n in sizes]

    def _cache_get(self, kind, key):
        ent = self._feat_cache.get((kind, key))
        if ent is not None:
            self._feat_cache.move_to_end((kind, key))
        return ent

    def _cache_put(self, kind, key, value, limit=None):
        self._feat_cache[(kind, key)] = value
        while sum(1 for k in self._feat_cache if k[0] == kind) > (limit or self.FEATURE_CACHE_FRAMES):
            oldest = next(k for k in self._feat_cache if k[0] == kind)
            del self._feat_cache[oldest]

    def _volume_geometry(self, H, W, L, AF):
        """Shapes of a window's correlation volumes: level sizes, the tile layout, element format, row strides, buffer sizes."""
        cfg = self.cfg
        h, w = H // 8, W // 8
        hl, wl = [h], [w]
        for l in range(1, L):
            hl.append(hl[-1] // 2)
            wl.append(wl[-1] // 2)
        Sl = [hl[l] * wl[l] for l in range(L)]
        # volume geometry: Nl columns per level, Pv rows - the pixels, or the whole tiles of a tiled volume (_tile)
        VT = self._tile()
        Nl = [VT.count(hl[l], wl[l]) for l in range(L)] if VT is not None else Sl
        Pv = Nl[0]
        TILE = VT.code if VT is not None else 0
        # cfg.corr_volume 'f16' / 'f16@k': the pyramids (from level k up) as one f16 per value, written by the GEMM form
        # (which needs every level's width a multiple of 4 and split-row query features) - other geometries keep f32
        # volumes.  The lookup reads as many texels of every level (a (2r+2)^2 window each), so levels 1-3 carry three
        # quarters of what f16 texels save it, at 13 % of the volume's bytes
        mask = self.CORR_VOLUMES[getattr(cfg, "corr_volume", "f32")] & ((1 << L) - 1)
        if not (mask and AF == hip.FMT_S16 and Pv % 4 == 0 and all(s % 4 == 0 for s in Nl) and L <= 4
                and cfg.corr_radius in (3, 4)):
            mask = 0
        v16 = [bool((mask >> l) & 1) for l in range(L)]
        VFl = [hip.FMT_F16 if v16[l] else hip.FMT_F32 for l in range(L)]
        VF = (hip.FMT_F32 if not mask else hip.FMT_F16 if mask == (1 << L) - 1 else hip.vol_f16_levels(mask))   # the lookups' vol_fmt
        # row stride of a level: whole 128-byte lines, an ODD number of them - the transposed second output of the
        # level-0 GEMM walks down a column, and at an even multiple (32640 floats = 255 x 512 bytes at 1080p) its
        # stores queue on half the memory channels: 1989 us per launch against 1652 (tools/exp/volume_gemm_shapes.py)
        ldl = []
        for l in range(L):
            unit = 64 if v16[l] else 32
            n = (Nl[l] + unit - 1) // unit * unit
            ldl.append(n if (n // unit) % 2 else n + unit)
        psz = [(Pv * ldl[l] + 1) // 2 if v16[l] else Pv * ldl[l] for l in range(L)]     # floats per level buffer
        return types.SimpleNamespace(L=L, AF=AF, hl=hl, wl=wl, Sl=Sl, VT=VT, Nl=Nl, Pv=Pv, TILE=TILE, vol16=mask, VF=VF,
                                     VFl=VFl, ldl=ldl, psz=psz)

    corr_on_demand = True    # False: every level of every pyramid is built whole by the dense GEMMs (tests, A/B runs)
    # Pooled levels that are computed on demand too, where level 0 is and the level qualifies (_on_demand_levels).  Level 2
    # works the same way ((1, 2)) but its gain at 1080p stayed inside the run-to-run noise: off.
    corr_on_demand_levels = (1,)

    # The bidirectional lookup of the update iterations keeps every query's gathered texel patch, keyed by its window
    # origins, and gathers again only where a window moved (vfml_corr_lookup_indirect_bidir_cached).
    # False: the uncached launch (tests, A/B runs).  Same bits either way.
    lookup_cache = True
    lookup_cache_count = False      # True: count hits and misses per iteration (lookup_cache_counts; tests, the probe)

    def _lookup_cache_plan(self, win, s, M, L, R, dev):
        """The patch cache of a window's lookups -> (patches, keys, rows, counts or None), or None where the lookup stays
        uncached: the cache goes with the split arithmetic's one-launch bidirectional lookup on a fixed-radius kernel."""
        if not (self.lookup_cache and win.bidir is not None and self._split() and not self.sk and not self.tri_frame
                and R in (3, 4) and L == 4):
            return None
        rows = M * s.Pn
        counts = None
        if self.lookup_cache_count:
            counts = self._buf("lookup_count", 2 * max(1, self.cfg.decoder_depth), dev, torch.int32, zero=True)
        return (self._buf("lookup_patches", 2 * rows * 4 * (2 * R + 2) ** 2, dev),
                self._buf("lookup_keys", 2 * rows * 8, dev, torch.int32), rows, counts)

    def lookup_cache_counts(self, reset=True):
        """[(hits, misses)] per update iteration since the last reset, with lookup_cache_count on (this synchronises)."""
        count = self._ws.get("lookup_count")
        if count is None:
            return []
        n = [int(v) for v in count.tolist()]
        if reset:
            count.zero_()
        return list(zip(n[0::2], n[1::2]))

    def _corr_scale(self, AF):
        scale = 1.0 / float(self.cfg.feat_dim) ** 0.5
        if AF == hip.FMT_S16:
            scale /= self.FMAP_ROW_SCALE       # the split-row query features carry a factor 16
        return scale

    def _level0_on_demand(self, keys, N, geo, dense_corr=False):
        """Whether a window's pyramids get their level 0 tile by tile, in front of the lookups that read it
        (vfml_corr_level0_ensure), instead of whole: keyed MOF windows of the mixed plan's arithmetic - the GEMM form with one
        MFMA per product and an f32 level 0, the lookups of both directions as one launch."""
        return (self.corr_on_demand and not dense_corr and keys is not None and self._split() and not self.tri_frame
                and not self.gma and not self.sk and geo.AF == hip.FMT_S16 and geo.Pv % 4 == 0 and geo.Nl[0] >= 1024
                and geo.VT is not None and geo.Pv == geo.Nl[0] and geo.VFl[0] == hip.FMT_F32 and self._nm("corr") == 1
                and self.cfg.feat_dim <= 256 and 2 * (N - 2) <= 8 and (geo.Nl[0] + 63) // 64 <= 2048)

    def _on_demand_levels(self, on_demand, geo):
        """The levels of a window's pyramids that are not built but filled tile by tile (vfml_corr_levels_ensure), ascending:
        none, or level 0 and those of corr_on_demand_levels whose dense GEMM runs on the same walk - an f32 level of at
        least 1024 columns (and at most 2048 column tiles); at most three in all."""
        if not on_demand:
            return ()
        more = [l for l in range(1, geo.L) if l in self.corr_on_demand_levels and geo.VFl[l] == hip.FMT_F32
                and geo.Nl[l] >= 1024 and (geo.Nl[l] + 63) // 64 <= 2048]
        return (0,) + tuple(more[:2])

    @staticmethod
    def _bitmap_sections(geo, levels):
        """Where each on-demand level's bitmap starts in the pyramid's one bitmap buffer (level 0's first), and the total."""
        at, n = {}, 0
        for l in levels:
            at[l] = n
            n += hip.corr_bitmap_words(geo.Pv, geo.Nl[l])
        return at, n

    @staticmethod
    def _pyramid_bitmap(pyr, L):
        """The bitmaps of an on-demand pyramid (which 128 x 64 tiles of its on-demand levels are computed, a section per
        level: _bitmap_sections): one more buffer of the pyramid's entry behind its L levels, so it is recycled and freed
        with them; it is cleared whenever the buffers are handed to a new pair."""
        return pyr[L].view(torch.int32)

    def corr_level_tiles_computed(self, reset=True):
        """Tiles the on-demand passes computed since the last reset, per pyramid level (tests, profiles: this synchronises)."""
        count = self._ws.get("ensure_count")
        if count is None:
            return [0, 0, 0, 0]
        n = [int(v) for v in count.tolist()]
        if reset:
            count.zero_()
        return n

    def corr_tiles_computed(self, reset=True):
        """Level-0 tiles the on-demand passes computed since the last reset (tests, profiles: this synchronises)."""
        return self.corr_level_tiles_computed(reset)[0]

    def _window_pyramids(self, feats, keys, N, geo, dev, od_levels=()):
        """K3/K4: the correlation pyramids of a window, one per problem (query frame -> target frame): level l is one GEMM of
        the query frame's features against the 2^l-pooled features of the target frame.  A pyramid depends on its two frames
        only, so with frame keys it is kept across windows: consecutive sliding windows share 2(N-3) of their 2(N-2)
        problems.  Returns {"f": [...], "b": [...]} (per centre frame, a list of level buffers).
        od_levels (_on_demand_levels): these levels are not built here - for level 0 neither the GEMM nor its transposed twin
        is launched; the pyramid gets empty bitmaps and the iterations fill the tiles their lookups read
        (update_block.ensure_level0)."""
        D, L = self.cfg.feat_dim, geo.L
        AF, VFl, Nl, Pv, ldl, psz = geo.AF, geo.VFl, geo.Nl, geo.Pv, geo.ldl, geo.psz
        scale = self._corr_scale(AF)
        lim = 2 * (N - 2) + 2
        pyrs = {"f": [], "b": []}
        on_demand = bool(od_levels)
        # (a pyramid without some of its levels is not the dense one, nor one that lacks other levels: its own cache entry)
        od = (tuple(od_levels), "od") if on_demand else ()
        if on_demand:
            psz = psz + [self._bitmap_sections(geo, od_levels)[1]]      # (the bitmaps travel with the level buffers)
        built = [l for l in range(L) if l not in od_levels]
        for c in range(1, N - 1):
            for d, tgt in (("f", c + 1), ("b", c - 1)):
                pk = ("p", keys[c], keys[tgt]) + od if keys is not None else None
                if pk is not None and self.gma and d == "b" and keys[c] == keys[tgt]:
                    # a frame against ITSELF (a window clamped at an end of the clip repeats a frame): the backward problem's
                    # level 0 adds its cross terms in the order of a transposed forward volume (VFML_CONV_SWAP_CROSS below),
                    # the forward problem's in the direct order - <a_i, a_j> then differs from itself in the last bit, so the
                    # two directions must not share one entry.  Without this a keyed window's backward lookups read the
                    # forward volume and the field is a few 1e-6 px from the same window run unkeyed.
                    # GMA checkpoints only: every other checkpoint keeps the entries, and the bits, it had.
                    pk += ("b",)
                pyr = self._cache_get("p", pk) if pk is not None else None
                if pyr is None:
                    if pk is None:    # uncached call: reuse one workspace set per problem slot
                        pyr = [self._buf(f"pyr_{d}{c}_{l}", psz[l], dev) for l in range(L)]
                    else:
                        # (registered before it is filled: same stream, and the next allocation then sees
                        # the right count and retires a stale pyramid instead of asking the allocator)
                        pyr = self._pyramid_buffers(psz, dev, limit=lim)
                        self._cache_put("p", pk, pyr, limit=lim)
                    # Level 0 of the reverse problem (tgt -> c) is the transpose of this one's: when it is
                    # going to be needed (tgt is, or next field becomes, a centre frame: the "f" problems of
                    # a forward-sliding job) the same pass of MFMAs stores it too (vfml_conv_desc.out_t), and
                    # only its three pooled levels are separate GEMMs.  In the steady state a field then
                    # builds its two new pyramids with one 32400 x 32400 GEMM instead of two.
                    # (a backward problem's level 0 computed directly uses VFML_CONV_SWAP_CROSS, the addition
                    # order of a transposed forward volume: both routes give the same bits)
                    rk = ("p", keys[tgt], keys[c]) + od if pk is not None else None
                    gemm_form = AF == hip.FMT_S16 and Pv % 4 == 0 and Nl[0] >= 1024
                    dual = rk is not None and d == "f" and gemm_form and ("p", rk) not in self._feat_cache
                    rev = None
                    if dual:
                        rev = self._pyramid_buffers(psz, dev, limit=lim)
                        self._cache_put("p", rk, rev, limit=lim)
                    cnm = self._nm("corr") if self._split() else 3
                    for l in built:
                        # (one MFMA per product is symmetric in its operands: no swapped cross terms to order)
                        hip.conv2d(feats[c][0], D, D, 1, 1, Pv, feats[tgt][1][l], None, Nl[l], 1, 1, pyr[l],
                                   ldl[l], out_scale=scale, in_fmt=AF, out_fmt=VFl[l],
                                   swap_cross=(d == "b" and l == 0 and gemm_form and cnm == 3),
                                   out_t=rev[0] if dual and l == 0 else None, ld_out_t=ldl[0] if dual and l == 0 else 0,
                                   mfma=cnm)
                    if dual:
                        for l in built if on_demand else range(1, L):
                            hip.conv2d(feats[tgt][0], D, D, 1, 1, Pv, feats[c][1][l], None, Nl[l], 1, 1, rev[l],
                                       ldl[l], out_scale=scale, in_fmt=AF, out_fmt=VFl[l], mfma=cnm)
                    if on_demand:
                        # (on the stream that builds the pooled levels, behind whatever read these buffers' last pair)
                        for p in (pyr, rev) if dual else (pyr,):
                            self._pyramid_bitmap(p, L).zero_()
                pyrs[d].append(pyr)
        return pyrs

    def _ensure_plan(self, pyrs, feats, N, geo, dev, od_levels):
        """What the on-demand passes of a window need (update_block.ensure_level0): the device cells that name, per direction
        and centre, the query frame's rows and, per on-demand level, the target frame's hi plane of that level, the level's
        buffer and its bitmap; and the dense call of every such level (of one of the pyramids: shapes and arithmetic)."""
        M = N - 2
        cells = self._buf("ensure_cells", 128, dev, torch.int64)      # (8 problems x (1 + 3 x 3 levels) at most)
        at, _ = self._bitmap_sections(geo, od_levels)
        ptrs = []
        for d, step in (("f", 1), ("b", -1)):
            for i, c in enumerate(range(1, N - 1)):
                pyr = pyrs[d][i]
                bits = self._pyramid_bitmap(pyr, geo.L)
                ptrs.append(feats[c][0])
                for l in od_levels:
                    ptrs += [feats[c + step][1][l].hi, pyr[l], bits.data_ptr() + 4 * at[l]]
        hip.ptr_table_set(cells, ptrs)
        count = self._buf("ensure_count", 4, dev, torch.int32, zero=True)     # (through _buf: captured launches hold its address)
        levels = [(l, feats[2][1][l], pyrs["f"][0][l], geo.Nl[l], geo.ldl[l], geo.hl[l], geo.wl[l]) for l in od_levels]
        return types.SimpleNamespace(cells=cells, M=M, rows=feats[1][0], levels=levels, per=1 + 3 * len(od_levels),
                                     D=self.cfg.feat_dim, scale=self._corr_scale(geo.AF), counter=count)

    def _frame_features(self, src, sel, keys, H, W, P, dev, L, hl, wl, Sl, vt=None):
        """Feature map + target pyramid of frames `sel` of the window.
        Returns {j: (fmap [Pn*256] f32, [target operand per level])}.
        vt (hip.VolTile): both operands' rows in tile order (zero rows at the positions no pixel has), so that the volume
        GEMMs write tiled level images under tile-ordered rows."""
        D = self.cfg.feat_dim
        split = self._split()
        out, todo = {}, []
        for j in sel:
            ent = self._cache_get("f", keys[j]) if keys is not None else None
            if ent is not None:
                out[j] = ent
            else:
                todo.append(j)
        if todo:
            m, Pn = len(todo), hl[0] * wl[0]
            frames = self._buf("frames", m * H * W * 4, dev)
            hip.frames_to_nhwc4(take_frames(src, todo).contiguous(), m, H, W, float(self.cfg.input_scale), float(self.cfg.input_shift),
                                frames)
            fmap = torch.empty(m * Pn * D, device=dev)          # owned by the cache entries (views)
            (self._twins_encoder if self.twins else self._encoder)("fnet", frames, m, H, W, P, dev, fmap, D, 0, hip.EPI_NONE, 0)
            levels = [fmap]
            for l in range(1, L):
                t = torch.empty(m * Sl[l] * D, device=dev)
                hip.avgpool2x2(levels[-1], m, hl[l - 1], wl[l - 1], D, t)
                levels.append(t)
            for i, j in enumerate(todo):
                tg = []
                for l in range(L):
                    f = levels[l][i * Sl[l] * D:(i + 1) * Sl[l] * D]
                    nl = Sl[l]
                    if vt is not None:
                        f, nl = vt.rows(f, hl[l], wl[l], D), vt.count(hl[l], wl[l])
                    # features are O(1): x16 keeps the lo halves of the split normal
                    tg.append(hip.SplitWeight(nl, D, dev).fill(f, scale=16.0) if split else f)
                fm = fmap[i * Pn * D:(i + 1) * Pn * D]
                if vt is not None:
                    fm, Pn_rows = vt.rows(fm, hl[0], wl[0], D), vt.count(hl[0], wl[0])
                else:
                    Pn_rows = Pn
                if split:
                    # the GEMM's A operand in split rows, made once per frame - of the SAME x16 copy the target
                    # planes are split from, so that a frame's hi / lo halves are the same numbers on either
                    # side of a correlation GEMM (then <a, b> and <b, a> are the same products, and with
                    # VFML_CONV_SWAP_CROSS the same sums: a volume and its transpose are bit-identical)
                    fm16 = torch.empty(Pn_rows * D, device=dev)
                    hip.to_s16(fm, Pn_rows, D, D, fm16, D, scale=self.FMAP_ROW_SCALE)
                    fm = fm16
                ent = (fm, tg)
                out[j] = ent
                if keys is not None:
                    self._cache_put("f", keys[j], ent)
        return out

    def _frame_context(self, src, sel, keys, H, W, P, dev, Pn, M=1):
        """Context maps (tanh | relu halves, [Pn*256] f32) of frames `sel`, and the context part of their gate convolutions:
        {j: frame_store.FrameContext}, with the frame's attention slot under the GMA aggregator."""
        out, todo = {}, []
        st = self._context_store(dev, Pn, max(M, len(sel)))
        att = self._attention_store(dev, Pn, max(M, len(sel))) if self.gma else None
        for j in sel:
            ent = self._cache_get("c", keys[j]) if keys is not None else None
            if ent is not None and ent.serial == st.ring.serial and (att is None or ent.att_serial == att.ring.serial):
                out[j] = ent
            else:
                todo.append(j)
        if todo:
            m = len(todo)
            frames = self._buf("frames", m * H * W * 4, dev)
            hip.frames_to_nhwc4(take_frames(src, todo).contiguous(), m, H, W,
                                float(self.cfg.input_scale), float(self.cfg.input_shift), frames)
            ctx = torch.empty(m * Pn * 256, device=dev)
            AF = hip.FMT_S16 if self._split() else hip.FMT_F32
            (self._twins_encoder if self.twins else self._encoder)("cnet", frames, m, H, W, P, dev, ctx, 256, 0, hip.EPI_TANH_RELU,
                                                                   self.hidden_dim, out_fmt=AF)
            h8, w8 = H // 8, W // 8
            R, Mst = st.ring.R, st.M
            for i, j in enumerate(todo):
                cx = ctx[i * Pn * 256:(i + 1) * Pn * 256]
                owner = ("c", keys[j]) if keys is not None else None
                slot = st.ring.take(owner, {e.slot for e in out.values()})
                # context part of the GRU gate convolutions (+ bias), per pass: [z|r] (256) and q (128), into the frame's slot
                add = {}
                for k, (kh, kw) in () if self.sk else (("1", (1, 5)), ("2", (5, 1))):      # (the SK block has no gates)
                    for g, co in (("zr", 256), ("q", 128)):
                        wgt, b = P[f"update_block.gru.conv{g}{k}.ctx"]
                        S = st.S[g + k]
                        hip.conv2d(cx, 128, 256, 1, h8, w8, wgt, b, co, kh, kw, S, co, in0_off=128, out_off=slot * Pn * co,
                                   pad_h=kh // 2, pad_w=kw // 2, in_fmt=AF,
                                   mfma=self._nm(f"update_block.gru.conv{g}{k}.ctx") if self._split() else 3)
                        add[g + k] = S[slot * Pn * co:(slot + 1) * Pn * co]
                        if slot < Mst - 1:          # the ring's first slots again behind it: a window that wraps stays consecutive
                            S[(R + slot) * Pn * co:(R + slot + 1) * Pn * co].copy_(add[g + k])
                ent = FrameContext(cx, add, slot, st.ring.serial)
                if att is not None:
                    aslot = att.ring.take(owner, {e.att_slot for e in out.values()})
                    self._build_attention(att, aslot, cx, h8, w8, Pn, P, dev, AF)
                    ent = ent._replace(att_slot=aslot, att_serial=att.ring.serial)
                out[j] = ent
                if keys is not None:
                    self._cache_put("c", keys[j], out[j])
        return out

    # ------------------------------------------------------------------ a window's recurrent state (vfml/update_block.py)
    def _state_columns(self):
        """(GLD, columns) of the recurrent state, one row of GLD floats per cell:  [ z | r*h | h | inp | mf | mt ]"""
        # (one allocation, so that cat([r*h, x]) and cat([h, x]) are channel slices of it; XC: what the gates read behind h,
        # [mf | mt])
        GLD, cols = 768, dict(Z=0, RH=128, HH=256, INP=384, MF=512, MT=640, MG=None, XC=256)
        if self.gma:        # ... | mg ]: the aggregated motion features, a fourth block of the gates' input
            GLD = 896
            cols.update(MG=768, XC=384)
        if self.sk:
            # the SK block's `gru` is a PCBlock over [h | inp | mf | mt (| mg)], read in place: no gate columns, and the
            # context half `inp` sits in the row (the plain block's gates take it as a per-frame addend)
            GLD = 640 if self.gma else 512
            cols.update(HH=0, INP=128, MF=256, MT=384, MG=512)
        return GLD, cols

    def _window_state(self, P, dev, M, h, w, geo, R, AF, cor_p):
        """Window layout and buffers: the update block's record of a window of M centre frames."""
        MP = M * h * w
        GLD, cols = self._state_columns()
        if self.gma and self._att_store is not None:
            self._att_store.ring.live = set()     # (the last window's read-outs are ahead of this one on the stream)

        def rows(name, c):
            return self._buf(name, MP * c, dev)
        return update_block.window_state(
            P, self._nm if self._split() else (lambda layer: 3),      # MFMAs per product of a layer (cfg.precision)
            AF, h, w, geo, R, rows("gru_state", GLD), GLD, cols, 2 * cor_p, cor_p, self._rows7, self._tapsum,
            corr=self._buf("corr", MP * 2 * cor_p, dev, zero=True),   # pad channels stay zero
            c1=rows("c1", 256), cf=rows("cf", 256), f1=rows("f1", 128), fh=rows("fh", 256), flow4=rows("flow4", 4),
            delta=rows("delta", 4), fh_taps=rows("fh_taps", 2 * 36),     # (two partial maps with the fused flow head)
            frows=rows("flow_rows7", 32), coords1=rows("coords1", 4))

    def _seed_plan(self, s, ctx, keys, dev, M, R, pick_only):
        """The iteration-zero seed plan -> (store, warm, keys of the entries this window fills, seed cells)."""
        # h = tanh half of the context map (the relu half reaches the gates as their addends), and the `mf` columns of the
        # centres whose iteration 0 an earlier window ran: one launch inside the body (vfml_window_seed), told what to copy
        # by three device cells per centre.  The store applies where iteration 0 covers every centre of a keyed window.
        cfg, it0 = self.cfg, None
        # (not for SK checkpoints: the window set-up copies h | inp as ONE 256-column block, and vfml_window_seed moves a
        # slot of the same width as the context block - DESIGN.md section 16)
        if (self.iter0_store and not self.sk and keys is not None and self._split() and not self.tri_frame and M >= 2
                and cfg.decoder_depth >= 1 and not (pick_only and cfg.decoder_depth + 1 < M)):
            it0 = self._iter0_store(dev, s.Pn, M)
            warm, seeds, it0_new = it0.ring.plan(keys, tail=(R,))
            self.iter0_stats["warm" if warm else "cold"] += 1
            self.iter0_last = (warm, [slot for slot, _ in seeds])
        else:
            warm, seeds, it0_new = False, [(None, hip.SEED_NONE)] * M, []
        seed_cells = self._buf("seed_cells", 64, dev, torch.int64)
        hip.ptr_table_set(seed_cells, [v for i, (slot, mode) in enumerate(seeds) for v in
                                       (ctx[i + 1].map, it0.S[slot * s.Pn * 128:] if slot is not None else 0, mode)])
        return it0, warm, it0_new, seed_cells

    def _gate_addends(self, ctx, dev, Pn, M):
        """The gates' context parts -> (gate_add, gate_off, gate_ind) of update_block.sep_conv_gru."""
        # the centre frames' slots, consecutive in a sliding job (through the mirror when the ring wraps) - else gathered
        # into the store's spare slots
        st = self._ctx_store
        RING, Mst = st.ring.R, st.M
        slots = [ctx[c].slot for c in range(1, M + 1)]
        st.ring.live = set(slots)
        first = window_base(slots, RING, Mst - 1)
        # (the exact-f32 kernel takes the pointer itself - a captured launch needs it fixed: always the gathered copy)
        # (A/B switch: VFML_CTX_GATHER=1 gathers every window, as round 2 did)
        if self.sk:
            first = slots[0]
        elif not self._split() or os.environ.get("VFML_CTX_GATHER", "0") == "1" or first is None:
            first = RING + Mst - 1
            for i, c in enumerate(range(1, M + 1)):
                for name, co in self.CTX_GATES:
                    st.S[name][(first + i) * Pn * co:(first + i + 1) * Pn * co].copy_(ctx[c].addends[name])
        gate_add = {name: st.S.get(name) for name, _ in self.CTX_GATES}
        gate_off = {name: first * Pn * co for name, co in self.CTX_GATES}
        gate_ind = None
        if self._split() and not self.sk:      # (the exact-f32 kernel takes the pointer itself)
            cells = self._buf("gate_add_cells", 8, dev, torch.int64)
            hip.ptr_table_set(cells, [st.S[name][gate_off[name]:] for name, _ in self.CTX_GATES])
            gate_ind = {name: (cells, i) for i, (name, _) in enumerate(self.CTX_GATES)}
        return gate_add, gate_off, gate_ind

    def _pyramid_tables(self, pyrs, dev, M, L, cor_p):
        """The device tables that name a window's pyramids -> (tables, bidir) of update_block.lookup."""
        # both directions behind one another in one table where they fit: the two lookups of an iteration as ONE launch
        # (at most 8 maps)
        if 2 * M <= 8 and 2 * M * L <= 48:
            tab_fb = self._buf("pyr_table_fb", 64, dev, torch.int64)
            hip.ptr_table_set(tab_fb, [p for d in ("f", "b") for m in pyrs[d] for p in m[:L]])
            return (tab_fb,), (2, cor_p, M)
        tab_f = self._buf("pyr_table_f", 64, dev, torch.int64)
        tab_b = self._buf("pyr_table_b", 64, dev, torch.int64)
        hip.ptr_table_set(tab_f, [p for m in pyrs["f"] for p in m[:L]])
        hip.ptr_table_set(tab_b, [p for m in pyrs["b"] for p in m[:L]])
        return (tab_f, tab_b), None

    def _gma_readout(self, s, win, ng):
        """mg = mf + gamma * attn . to_v(mf), per centre frame with its own attention, on the ng centres whose GRU runs."""
        att = self._att_store
        update_block.attention_readout(s, "update_block.aggregator.to_v", [att.A[k] for k in win.att_slots[:ng]],
                                       att.plain, att.ldA, att.P8, self._gamma, ATT_SCALE, s.MF, s.MG, win.readout)

    def _iteration(self, s, win, it, ng, nm, branch):
        """One iteration of the plain update block: GRU + flow head on `ng` centres, lookups + motion encoder on `nm`."""
        # The flow half of the motion encoder (flow -> convf1 -> convf2 -> channels 192..255 of `cf`) needs nothing of the
        # correlation half (lookups -> convc1 -> convc2 -> channels 0..191): on a second stream (`branch`, VFML_FLOW_BRANCH)
        # its small MFMA-bound convolutions run BESIDE the HBM-bound lookups (a fork / join of two events; inside a captured
        # graph, two branches).  Same kernels on the same inputs: bit-identical fields.
        # Iteration 0 of a warm window: the per-frame launches (lookups, motion encoder up to encoder.conv) run on the newest
        # centre alone - ne frames from row r0 on - and the seed pass brings the other centres' rows.
        ub = update_block
        ne, r0 = (1, (win.M - 1) * s.Pn) if win.warm and it == 0 else (nm, 0)
        join = None
        if branch is not None:
            fork = torch.cuda.Event()
            fork.record()                      # (flow4 of the previous iteration is complete on this stream)
            with torch.cuda.stream(branch):
                branch.wait_event(fork)
                ub.flow_half(s, ne, r0)
                join = torch.cuda.Event()
                join.record()
        if win.ensure is not None:
            ub.ensure_level0(s, ne, r0, win.ensure)     # the tiles this lookup reads and the pyramids lack
        cache = None
        if win.cache is not None:
            # (nobody reads the patches of the last iteration's launch: it stores none)
            patches, keys, rows, counts = win.cache
            cache = (patches, keys, rows, it + 1 < self.cfg.decoder_depth, counts[2 * it:] if counts is not None else None)
        ub.lookup(s, ne, r0, win.tables, win.bidir, cache=cache)
        ub.convc1(s, ne, r0)
        ub.convc2(s, ne, r0)
        if join is None:
            ub.flow_half(s, ne, r0)
        else:
            torch.cuda.current_stream(win.dev).wait_event(join)
        ub.encoder_conv(s, ne, r0)
        if it == 0:
            # h of every centre from its context map; mf rows (with the zero flow in channels 124..127) out of the
            # older centres' slots and into the new ones
            hip.window_seed(win.seed_cells, win.M, s.Pn, 128, s.G, s.GLD, s.HH, s.MF, 256)
        if self.gma:
            self._gma_readout(s, win, ng)
        update_block.temporal_fusion(s, win.M if self.tri_frame else nm, stack=not self.tri_frame)
        ub.sep_conv_gru(s, ng, *win.gates)
        ub.flow_head(s, ng)

    def _sk_iteration(self, s, win, ng, nm):
        """One iteration of the SK update block: lookup, the five PCBlocks of the motion encoder, the GMA read-out,
        the temporal fusion, `gru` and `flow_head`."""
        ub, P, h, w, G, GLD, ws = "update_block", s.P, s.h, s.w, s.G, s.GLD, win.sk_ws
        blk = self._pcblock
        update_block.lookup(s, nm, 0, win.tables, win.bidir)
        blk(f"{ub}.encoder.convc1", P, s.corr, s.ld_corr, 0, nm, h, w, s.c1, 256, 0, ws, gelu_out=True)
        blk(f"{ub}.encoder.convc2", P, s.c1, 256, 0, nm, h, w, s.cf, 256, 0, ws)
        wgt, b = P[f"{ub}.encoder.convf1"]
        hip.conv2d(s.flow4, 4, 4, nm, h, w, wgt, b, 128, 1, 1, s.f1, 128, out_fmt=s.AF, mfma=s.nm(f"{ub}.encoder.convf1"))
        blk(f"{ub}.encoder.convf2", P, s.f1, 128, 0, nm, h, w, s.cf, 256, 192, ws)
        blk(f"{ub}.encoder.conv", P, s.cf, 256, 0, nm, h, w, G, GLD, s.MF, ws)
        if self.gma:
            self._gma_readout(s, win, ng)
        update_block.temporal_fusion(s, win.M if self.tri_frame else nm, stack=not self.tri_frame)
        blk(f"{ub}.gru", P, G, GLD, 0, ng, h, w, G, GLD, s.HH, ws)
        blk(f"{ub}.flow_head", P, G, GLD, s.HH, ng, h, w, s.delta, 4, 0, ws, out_fmt=hip.FMT_F32)
        update_block.update_coords(s, ng)

    def _run(self, src, N, H, W, return_lowres, frame_keys=None, tri_batch=False, pick_only=False, dense_corr=False):
        cfg = self.cfg
        if N < 3:
            raise ValueError(f"need at least 3 frames, got {N}")
        if self.tri_frame and N > 3 and not tri_batch:
            lo = N // 2 - 1
            src = src[lo:lo + 3].contiguous()
            frame_keys = frame_keys[lo:lo + 3] if frame_keys is not None else None
            N = 3
        if H % 8 or W % 8:
            raise ValueError("H and W must be multiples of 8 (use InputPadder)")
        L, R = cfg.corr_levels, cfg.corr_radius
        h, w = H // 8, W // 8
        if (h >> (L - 1)) < 2 or (w >> (L - 1)) < 2:
            raise ValueError(f"frame {H}x{W} too small for a {L}-level correlation pyramid")
        dev = src.device
        self._join_prefetch()      # a prefetch shares the encoders' workspaces and fills the caches read below
        M = N - 2
        Pn = h * w          # cells per map
        if self.gma and Pn > 32768:
            raise ValueError(f"frame {H}x{W}: the GMA aggregator attends over all {Pn} cells of a frame and is built for at "
                             f"most 32768; process larger frames in tiles (--tile)")
        MP = M * Pn
        P = self._pack(dev)
        AF = hip.FMT_S16 if self._split() else hip.FMT_F32   # update-block activations
        cor_p = cor_pad(L * (2 * R + 1) ** 2, AF == hip.FMT_S16)   # per-direction channel block
        short = pick_only and not self.tri_frame      # only the reference's pick is wanted: flow M of the full output

        with torch.cuda.device(dev):
            geo = self._volume_geometry(H, W, L, AF)
            keys = None
            if frame_keys is not None:   # geometry and arithmetic are part of a cached frame's identity
                keys = [(k, H, W, L, self._plan_key(), self._packed_serial) for k in frame_keys]

            # K1 + K2: feature maps and pooled target pyramids, per frame (cached across windows)
            feats = self._frame_features(src, list(range(N)), keys, H, W, P, dev, L, geo.hl, geo.wl, geo.Sl, vt=geo.VT)
            # K3/K4 correlation pyramids, one per problem (query frame -> target frame)
            on_demand = self._level0_on_demand(keys, N, geo, dense_corr)
            od_levels = self._on_demand_levels(on_demand, geo)
            pyrs = self._window_pyramids(feats, keys, N, geo, dev, od_levels)
            s = self._window_state(P, dev, M, h, w, geo, R, AF, cor_p)
            # K2 context encoder on the centre frames -> h = tanh(first half), inp = relu(second half)
            ctx = self._frame_context(src, list(range(1, N - 1)), keys, H, W, P, dev, Pn, M)
            win = types.SimpleNamespace(M=M, dev=dev, att_slots=(), readout=None)
            if self.gma:
                att = self._att_store
                win.att_slots = tuple(ctx[c].att_slot for c in range(1, N - 1))
                att.ring.live = set(win.att_slots)
                win.readout = update_block.readout_scratch(self._buf, dev, MP, Pn, self.ATT_DIM, att.ldA, att.plain, att.vt)
            it0, win.warm, it0_new, win.seed_cells = self._seed_plan(s, ctx, keys, dev, M, R, pick_only)
            win.gates = self._gate_addends(ctx, dev, Pn, M)
            win.sk_ws = self._sk_workspace(MP, dev) if self.sk else None
            win.tables, win.bidir = self._pyramid_tables(pyrs, dev, M, L, cor_p)
            win.ensure = self._ensure_plan(pyrs, feats, N, geo, dev, od_levels) if on_demand else None
            win.cache = self._lookup_cache_plan(win, s, M, L, R, dev)
            no, nflows = (1, 1) if short else (M, 2 * M)
            up_fixed = self._buf("up_out", nflows * H * W * 2, dev)
            mask = self._buf("mask", MP * 1152, dev)

            # ---- the update iterations + mask head + upsampling: a FIXED launch sequence for a given geometry,
            # window length and arithmetic - only the correlation pyramids it looks up differ from field to field,
            # and those are named by device tables.  With cfg.use_graph the sequence is captured into a HIP
            # graph the second time a configuration is seen and replayed from then on (~250 launches per field
            # become one; same kernels, same order: bit-identical results).
            def body():
                update_block.init_coords(s, M)
                if win.cache is not None:
                    # no patch of an earlier field, pyramid set or plan can hit: every key starts the field empty
                    win.cache[1].fill_(hip.LOOKUP_KEY_NONE)
                branch = None
                if os.environ.get("VFML_FLOW_BRANCH", "0") == "1" and self._split():
                    branch = self._side2.get(dev)
                    if branch is None:
                        branch = self._side2[dev] = torch.cuda.Stream(device=dev)
                if self.sk:
                    # h | inp of every centre from its context map (one 256-column block), before the first iteration
                    hip.window_seed(win.seed_cells, M, Pn, 256, s.G, s.GLD, s.HH, s.MF, 256)
                for it in range(cfg.decoder_depth):
                    # pick_only: the caller takes flow M (the backward flow of the first centre frame - the reference's
                    # `[0, shape[1]//2]`).  Going back from the last iteration, centre 0's result depends on one centre
                    # more per iteration (through the temporal fusion), so the last iterations run on the centres
                    # that still matter only: GRU + flow head on `ng`, lookups + motion encoder on `nm` of them.
                    left = cfg.decoder_depth - 1 - it
                    ng = min(M, left + 1) if short else M
                    nm = min(M, left + 2) if short else M
                    if self.sk:
                        self._sk_iteration(s, win, ng, nm)
                    else:
                        self._iteration(s, win, it, ng, nm, branch)
                if cfg.decoder_depth == 0 and not self.sk:       # (no iteration ran the window set-up: h for the mask head)
                    hip.window_seed(win.seed_cells, M, Pn, 128, s.G, s.GLD, s.HH, s.MF, 256)
                # mask head on the final hidden state, then K8 for every flow of the output tensor (pick_only: of
                # the first centre frame, and its backward flow alone)
                update_block.mask_head(s, no, mask, 1152)
                if short:
                    hip.convex_upsample(s.coords1, 0, 2, mask, 576, 1152, h, w, up_fixed)
                else:
                    for d in range(2):
                        for c in range(M):
                            hip.convex_upsample(s.coords1, c * Pn * 4, 2 * d, mask, c * Pn * 1152 + d * 576, 1152, h, w,
                                                up_fixed, out_off=(d * M + c) * H * W * 2)

            gkey = (H, W, N, M, bool(tri_batch), bool(pick_only), cfg.decoder_depth, L, R, self._plan_key(), geo.vol16, od_levels,
                    self._packed_serial, str(dev), os.environ.get("VFML_FLOW_BRANCH", "0"),
                    # (the lookup's patch cache, and whether its launches count)
                    win.cache is not None, win.cache is not None and win.cache[3] is not None,
                    win.warm, win.att_slots, on_demand)
            if self.sk:
                gkey += ("sk",)
            self._pre_body = torch.cuda.Event()
            self._pre_body.record(torch.cuda.current_stream(dev))      # (what a prefetch of the next window waits for)
            try:
                self._run_body(body, gkey, dev)
            except BaseException:
                if it0_new:      # (slots promised to this window's centres that may not have been filled)
                    it0.ring.forget(it0_new)
                raise
            up = up_fixed.clone().view(nflows, H, W, 2)          # the caller owns its field; the fixed buffer is reused
            # [2M,H,W,2] stored HWC; expose the reference's [B, 2M, 2, H, W] as a view ([1, 1, 2, H, W] of a pick)
            flow = up.permute(0, 3, 1, 2).unsqueeze(0)
            if short:
                return flow, None
            low = s.flow4.view(M, h, w, 4)[..., :].clone() if return_lowres else None
        return flow, low


def build_network(cfg):
    return MOFNetHIP(cfg)
