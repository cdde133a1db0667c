"""CPU oracle of the MOF / BOF network WITH Twins-SVT encoders (TEST INFRASTRUCTURE ONLY).

The oracle that cfg.sk / cfg.gma select today (tests/mof_sk_oracle.py, tests/mof_gma_oracle.py, oracle.mof_oracle) with `fnet`
and `cnet` replaced by the encoder of DESIGN.md section 17, in plain PyTorch: parameter names are the engine's
(`fnet.svt.blocks.0.1.attn.sr`, ...), so a state dict of vfml.weights.seeded_state_dict(cfg with twins=True) loads strictly.

    encoder = `<prefix>.svt`: timm 0.4.12 twins_svt_large cut to two stages, [n, 3, H, W] -> [n, 256, H/8, W/8]
    stage i:  patch_embeds.i (Conv2d kernel = stride = p, then LayerNorm) -> blocks.i.0 (LSA, 7 x 7 windows) ->
              pos_block.i (x + depthwise 3 x 3) -> blocks.i.1 (GSA, keys and values sub-sampled by `sr`) -> back to the grid
    block:    x = x + attn(norm1(x));  x = x + fc2(gelu(fc1(norm2(x))))        (exact GELU, LayerNorm eps 1e-5)
    LSA:      the normed grid is zero-padded right and bottom to multiples of 7 BEFORE qkv (a pad token's q, k, v are the
              qkv bias), cut into windows anchored at (0, 0), softmax(q k^T / sqrt 32) v per head over the 49 tokens of a
              window - pad tokens are NOT masked -, pad rows dropped before proj
    GSA:      q of every token against k | v = kv(norm(sr(x))) of the frame's floor(h / sr) * floor(w / sr) reduced tokens
    `svt.norm` (1024 channels, the four-stage backbone's final norm) is carried and unused.

Like the rest of the oracle this restates a published block as recalled; it is pinned by the known answers and the distance
tests of tests/test_twins_cpu.py, NOT against upstream code or weights.

VARIANT (a module-level dict, all False) switches on the deliberately WRONG readings that tests/test_twins_cpu.py measures the
definition's distance from: "pad_left_top", "mask_pad_keys", "uniform_attention".
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import mof_oracle as mo

WS = 7
STAGES = ((4, 3, 128, 4, 8), (2, 128, 256, 8, 4))     # patch, channels in, channels, heads, sr
VARIANT = {"pad_left_top": False, "mask_pad_keys": False, "uniform_attention": False}


def _softmax(scores):
    if VARIANT["uniform_attention"]:
        finite = torch.isfinite(scores).to(scores.dtype)
        return finite / finite.sum(-1, keepdim=True)
    return scores.softmax(-1)


class Mlp(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1 = nn.Linear(c, 4 * c)
        self.fc2 = nn.Linear(4 * c, c)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class LSA(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(c, 3 * c)
        self.proj = nn.Linear(c, c)

    def forward(self, x, size):
        B, N, C = x.shape
        h, w = size
        ph, pw = -h % WS, -w % WS
        x = x.view(B, h, w, C)
        real = torch.ones(1, h, w, 1, dtype=x.dtype)
        pad = (0, 0, pw, 0, ph, 0) if VARIANT["pad_left_top"] else (0, 0, 0, pw, 0, ph)
        x, real = F.pad(x, pad), F.pad(real, pad)
        Hp, Wp = h + ph, w + pw
        gh, gw = Hp // WS, Wp // WS

        def windows(t, c):
            return t.reshape(t.shape[0], gh, WS, gw, WS, c).transpose(2, 3).reshape(t.shape[0], gh * gw, WS * WS, c)
        d = C // self.heads
        qkv = self.qkv(windows(x, C)).reshape(B, gh * gw, WS * WS, 3, self.heads, d).permute(3, 0, 1, 4, 2, 5)
        q, k, v = qkv[0], qkv[1], qkv[2]                       # [B, windows, heads, 49, d]
        scores = (q @ k.transpose(-2, -1)) * d ** -0.5
        if VARIANT["mask_pad_keys"]:
            keep = windows(real, 1)[:, :, :, 0]                # [1, windows, 49]
            scores = scores.masked_fill(keep[:, :, None, None, :] == 0, float("-inf"))
        out = (_softmax(scores) @ v).transpose(2, 3).reshape(B, gh, gw, WS, WS, C).transpose(2, 3).reshape(B, Hp, Wp, C)
        out = out[:, ph:, pw:] if VARIANT["pad_left_top"] else out[:, :h, :w]
        return self.proj(out.reshape(B, N, C))


class GSA(nn.Module):
    def __init__(self, c, heads, sr):
        super().__init__()
        self.heads = heads
        self.q = nn.Linear(c, c)
        self.kv = nn.Linear(c, 2 * c)
        self.proj = nn.Linear(c, c)
        self.sr = nn.Conv2d(c, c, sr, stride=sr)
        self.norm = nn.LayerNorm(c)

    def forward(self, x, size):
        B, N, C = x.shape
        d = C // self.heads
        q = self.q(x).reshape(B, N, self.heads, d).transpose(1, 2)
        r = self.sr(x.transpose(1, 2).reshape(B, C, *size)).reshape(B, C, -1).transpose(1, 2)
        kv = self.kv(self.norm(r)).reshape(B, -1, 2, self.heads, d).permute(2, 0, 3, 1, 4)
        k, v = kv[0], kv[1]
        out = _softmax((q @ k.transpose(-2, -1)) * d ** -0.5) @ v
        return self.proj(out.transpose(1, 2).reshape(B, N, C))


class Block(nn.Module):
    def __init__(self, c, heads, sr=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(c)
        self.attn = LSA(c, heads) if sr is None else GSA(c, heads, sr)
        self.norm2 = nn.LayerNorm(c)
        self.mlp = Mlp(c)

    def forward(self, x, size):
        x = x + self.attn(self.norm1(x), size)
        return x + self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, p, cin, c):
        super().__init__()
        self.proj = nn.Conv2d(cin, c, p, stride=p)
        self.norm = nn.LayerNorm(c)

    def forward(self, x):
        x = self.proj(x)
        size = x.shape[2:]
        return self.norm(x.flatten(2).transpose(1, 2)), size


class PosConv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(c, c, 3, padding=1, groups=c))

    def forward(self, x, size):
        B, N, C = x.shape
        g = x.transpose(1, 2).reshape(B, C, *size)
        return (self.proj(g) + g).flatten(2).transpose(1, 2)


class Twins(nn.Module):
    def __init__(self):
        super().__init__()
        self.patch_embeds = nn.ModuleList([PatchEmbed(p, cin, c) for p, cin, c, _, _ in STAGES])
        self.blocks = nn.ModuleList([nn.ModuleList([Block(c, hd), Block(c, hd, sr)]) for _, _, c, hd, sr in STAGES])
        self.pos_block = nn.ModuleList([PosConv(c) for _, _, c, _, _ in STAGES])
        self.norm = nn.LayerNorm(1024)            # carried by the checkpoints, unused by the two-stage cut

    def forward(self, x):
        B = x.shape[0]
        for embed, blocks, pos in zip(self.patch_embeds, self.blocks, self.pos_block):
            x, size = embed(x)
            for j, blk in enumerate(blocks):
                x = blk(x, size)
                if j == 0:
                    x = pos(x, size)
            x = x.reshape(B, *size, -1).permute(0, 3, 1, 2).contiguous()
        return x


class TwinsEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.svt = Twins()

    def forward(self, x):
        return self.svt(x)


def build_network(cfg):
    if getattr(cfg, "sk", False):
        import mof_sk_oracle as base
    elif getattr(cfg, "gma", False):
        import mof_gma_oracle as base
    else:
        base = mo
    net = base.build_network(cfg)
    if cfg.feat_dim != 256:
        raise ValueError("the Twins-SVT encoders give 256 channels")
    net.fnet = TwinsEncoder()
    net.cnet = TwinsEncoder()
    return net
