"""The CPU oracle with the roundings of a mixed-precision plan applied (TEST INFRASTRUCTURE ONLY).

`cfg.precision = 'mixed'` lets the engine spend fewer f16 matrix products on named layers (vfml/network.py `_nm`,
vfml/cfg.py DEFAULT_MIXED_PLAN / BOF_F16_PLAN) and keep pyramid levels as f16 (`cfg.corr_volume`).  Each of those is one
well-defined rounding of an operand, pinned kernel by kernel in tests/test_gpu_kernels.py
(test_conv2d_reduced_mfma_counts_drop_exactly_the_lo_terms, test_gemm_form_reduced_mfma_counts).  This module restates
them on top of oracle/mof_oracle.py, in whatever dtype the module is converted to, so that the mixed engine can be compared
with a reference that rounds where the plan says instead of being given an error budget:

  count 1     activations and weights of the layer rounded to one f16
  count "2a"  the activations only
  count 2     ("2w") the weights only
  weights     f16(w * s) / s with s = the power of two that brings the absolute maximum of the layer's PACKED matrix just
              below 2^14 (hip.SplitWeight.auto_scale).  The packed matrix is the layer's own weight, except for the GRU
              gates: z and r of one pass share a matrix, and every gate matrix is split into the part over
              [h | motion | temporal] ('<gate>.iter', evaluated every iteration) and the part over the context map
              ('<gate>.ctx', evaluated once per frame), each with its own count and its own scale
  "corr": 1   query features and (after pooling, per level) target features rounded as f16(16 x) / 16; level l of a
              pyramid is the product of the query features with the 2^l-pooled target features, as in the engine
              (counts 2 / "2a" on "corr" mean 3, as in `_nm`: a volume and its transpose stay the same numbers)
  f16@k       pyramid levels k and up rounded to f16 ('f16' = every level)

Longest matching prefix of the layer name wins, 3 where nothing matches.  The mechanism is generic over layer names, so
BOF_F16_PLAN is covered as well as DEFAULT_MIXED_PLAN.  Not restated: the f32 accumulation order of the kernels and the
~2^-22 relative error of their split-f16 operands - that is the arithmetic noise the tests bound separately.

With an empty plan and an 'f32' volume no module is touched and the result is bit-identical to mof_oracle.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import mof_oracle as mo

FMAP_ROW_SCALE = 16.0
CORR_VOLUMES = {"f32": None, "f16": 0, "f16@1": 1, "f16@2": 2, "f16@3": 3}


def f16(t):
    """Round to the nearest f16 value, keeping the dtype."""
    return t.to(torch.float16).to(t.dtype)


def auto_scale(absmax):
    """Largest power of two that keeps scale * absmax below 2^14."""
    if not (absmax > 0.0) or not math.isfinite(absmax):
        return 1.0
    return 2.0 ** math.floor(math.log2(16384.0 / absmax))


def round_weight(w, packed=None):
    """f16(w * s) / s with s from the absolute maximum of `packed` (the matrix w is a part of; default: w itself)."""
    s = auto_scale(float((w if packed is None else packed).abs().max()))
    return f16(w * s) / s


def count_of(plan, layer):
    best, nm = -1, 3
    for prefix, n in plan.items():
        if layer.startswith(prefix) and len(prefix) > best:
            best, nm = len(prefix), (n if isinstance(n, str) else int(n))
    if nm == "2w":
        nm = 2
    if nm not in (1, 2, "2a", 3):
        raise ValueError(f"plan[{layer!r}] = {nm!r}: 1, 2 ('2w'), '2a' or 3")
    if layer == "corr" and nm in (2, "2a"):
        nm = 3
    return nm


def _operands(nm, x, w, packed=None):
    return (f16(x) if nm in (1, "2a") else x), (round_weight(w, packed) if nm in (1, 2) else w)


class _PlanConv:
    """Replacement for the forward of one nn.Conv2d that runs at a count other than 3."""

    def __init__(self, conv, nm):
        self.conv, self.nm = conv, nm

    def __call__(self, x):
        c = self.conv
        x, w = _operands(self.nm, x, c.weight)
        return F.conv2d(x, w, c.bias, c.stride, c.padding)


class PlanCorrBlock(mo.CorrBlock):
    """All-pairs volume of f16-rounded features, level l from the 2^l-pooled (then rounded) target features."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels, self.radius = num_levels, radius
        b, d, h, w = fmap1.shape
        q = (f16(fmap1 * FMAP_ROW_SCALE) / FMAP_ROW_SCALE).view(b, d, h * w).transpose(1, 2)
        self.pyramid = []
        for l in range(num_levels):
            if l:
                fmap2 = F.avg_pool2d(fmap2, 2, stride=2)
            hl, wl = fmap2.shape[-2:]
            t = (f16(fmap2 * FMAP_ROW_SCALE) / FMAP_ROW_SCALE).view(b, d, hl * wl)
            self.pyramid.append((torch.matmul(q, t) / math.sqrt(d)).reshape(b * h * w, 1, hl, wl))


class PlanOracle(mo.MOFNetOracle):
    def __init__(self, cfg, plan, corr_volume="f32"):
        super().__init__(cfg)
        if corr_volume not in CORR_VOLUMES:
            raise ValueError(f"corr_volume must be one of {tuple(CORR_VOLUMES)}, got {corr_volume!r}")
        self.plan, self.corr_volume = dict(plan), corr_volume
        ub = self.update_block
        for name, m in self.named_modules():
            if not isinstance(m, nn.Conv2d) or name.startswith("update_block.gru.") or name.endswith(".convc1"):
                continue
            if self.count(name) != 3:
                m.forward = _PlanConv(m, self.count(name))
        if self.count("update_block.encoder.convc1") != 3:
            ub.encoder.forward = self._motion_encoder
        if any(self.count(f"update_block.gru.conv{g}{k}.{part}") != 3
               for g in ("zr", "q") for k in "12" for part in ("iter", "ctx")):
            ub.gru.forward = self._gru

    def count(self, layer):
        return count_of(self.plan, layer)

    # ---- the first motion-encoder convolution (mof_oracle.MotionEncoder.forward with its operands rounded)
    def _motion_encoder(self, fflow, bflow, fcorr, bcorr):
        e = self.update_block.encoder
        flow = torch.cat([fflow, bflow], dim=1)
        w = e.convc1.weight
        if e.sel is not None:
            half = w.shape[1] // 2
            w = torch.cat([w[:, e.sel], w[:, half + e.sel]], dim=1)
        x, w = _operands(self.count("update_block.encoder.convc1"), torch.cat([fcorr, bcorr], dim=1), w)
        cor = F.relu(F.conv2d(x, w, e.convc1.bias))
        cor = F.relu(e.convc2(cor))
        flo = F.relu(e.convf1(flow))
        flo = F.relu(e.convf2(flo))
        out = F.relu(e.conv(torch.cat([cor, flo], dim=1)))
        return torch.cat([out, flow], dim=1)

    # ---- SepConvGRU with every gate convolution as its two packed parts
    def _gate(self, convs, name, k, h, x):
        """conv([h | x]) of the gate(s) `convs` (z and r together, or q): the part over [h | motion | temporal] and the
        part over the context map (x = [inp | motion | temporal]), each rounded by its own count and scale."""
        hid = h.shape[1]
        w = torch.cat([c.weight for c in convs])
        b = torch.cat([c.bias for c in convs])
        pad = convs[0].padding
        w_it = torch.cat([w[:, :hid], w[:, 2 * hid:]], dim=1)
        w_cx = w[:, hid:2 * hid]
        a_it, w_it = _operands(self.count(f"update_block.gru.conv{name}{k}.iter"), torch.cat([h, x[:, hid:]], dim=1), w_it)
        a_cx, w_cx = _operands(self.count(f"update_block.gru.conv{name}{k}.ctx"), x[:, :hid], w_cx)
        return F.conv2d(a_it, w_it, None, 1, pad) + F.conv2d(a_cx, w_cx, b, 1, pad)

    def _gru(self, h, x):
        g = self.update_block.gru
        hid = h.shape[1]
        for k, (cz, cr, cq) in (("1", (g.convz1, g.convr1, g.convq1)), ("2", (g.convz2, g.convr2, g.convq2))):
            zr = torch.sigmoid(self._gate((cz, cr), "zr", k, h, x))
            z, r = zr[:, :hid], zr[:, hid:]
            q = torch.tanh(self._gate((cq,), "q", k, r * h, x))
            h = (1 - z) * h + z * q
        return h

    # ---- correlation volumes
    def _corr_block(self, fmap1, fmap2):
        cfg = self.cfg
        cls = PlanCorrBlock if self.count("corr") == 1 else mo.CorrBlock
        blk = cls(fmap1, fmap2, cfg.corr_levels, cfg.corr_radius)
        first = CORR_VOLUMES[self.corr_volume]
        if first is not None:
            blk.pyramid = [f16(p) if l >= first else p for l, p in enumerate(blk.pyramid)]
        return blk

    @torch.no_grad()
    def forward(self, images, data=None, return_lowres=False):
        if self.count("corr") == 3 and self.corr_volume == "f32":
            return super().forward(images, data, return_lowres)
        # mof_oracle.MOFNetOracle.forward with the volumes built by _corr_block
        cfg = self.cfg
        if getattr(cfg, "network", "MOFNetStack") == "BOFNet" and images.shape[1] > 3:
            lo = images.shape[1] // 2 - 1
            images = images[:, lo:lo + 3]
        B, N, _, H, W = images.shape
        M = N - 2
        h, w = H // 8, W // 8
        images = cfg.input_scale * images + cfg.input_shift
        fmaps = self.fnet(images.reshape(B * N, 3, H, W)).reshape(B, N, -1, h, w)
        centre = fmaps[:, 1:N - 1].reshape(B * M, -1, h, w)
        fcorr_fn = self._corr_block(centre, fmaps[:, 2:N].reshape(B * M, -1, h, w))
        bcorr_fn = self._corr_block(centre, fmaps[:, 0:N - 2].reshape(B * M, -1, h, w))
        cnet = self.cnet(images[:, 1:N - 1].reshape(B * M, 3, H, W))
        net, inp = torch.split(cnet, [self.hidden_dim, self.context_dim], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        coords0 = mo.coords_grid(B * M, h, w, images.dtype)
        fcoords1, bcoords1 = coords0.clone(), coords0.clone()
        for _ in range(cfg.decoder_depth):
            fcorr, bcorr = fcorr_fn(fcoords1), bcorr_fn(bcoords1)
            net, up_mask, delta = self.update_block(net, inp, fcorr, bcorr, fcoords1 - coords0, bcoords1 - coords0, B)
            fcoords1 = fcoords1 + delta[:, 0:2]
            bcoords1 = bcoords1 + delta[:, 2:4]
        fmask, bmask = torch.split(up_mask, [576, 576], dim=1)
        fup = mo.upsample_flow(fcoords1 - coords0, fmask).reshape(B, M, 2, H, W)
        bup = mo.upsample_flow(bcoords1 - coords0, bmask).reshape(B, M, 2, H, W)
        low = torch.cat([(fcoords1 - coords0).reshape(B, M, 2, h, w),
                         (bcoords1 - coords0).reshape(B, M, 2, h, w)], dim=1)
        return torch.cat([fup, bup], dim=1), low


def build_network(cfg, plan, corr_volume="f32"):
    return PlanOracle(cfg, plan, corr_volume)
