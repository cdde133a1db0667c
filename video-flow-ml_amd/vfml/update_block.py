"""The launches of the recurrent update block, each layer's in one place.

`MOFNetHIP._run` (vfml/network.py: MOF, BOF, with or without the GMA aggregator; the SK block's iteration shares the lookup,
the read-out and the temporal fusion) and `MemFlowNetHIP.forward_pairs` (vfml/memflow_net.py) build one record per call -
`window_state(...)`: the packed weights, the arithmetic, the geometry, the state buffer with its columns, the scratch maps -
and sequence the functions below over it.  A function takes the record and the frames it acts on (n frames from state row r0
on) and issues the hip.* calls; what differs between the engines is data that is a launch argument anyway (a column, a
width, a table or a list of pyramids, an addend's offset): no function asks which engine calls it.

State rows, GLD floats per cell:  [ z | r*h | h | inp | mf | mt (| mg) ]  at the columns Z, RH, HH, INP, MF, MT, MG; the
gates read [h | XC columns from MF on].  One allocation, so that cat([r*h, x]) and cat([h, x]) are channel slices of it."""
import types

from . import hip

UB = "update_block"


def window_state(P, nm, AF, h, w, geo, R, G, GLD, cols, ld_corr, cor_p, rows7, tapsum, **maps):
    """P: packed weights; nm(layer): MFMAs per product; AF: the activations' format; geo: _volume_geometry's shapes; R: the
    lookup radius; cols: {Z, RH, HH, INP, MF, MT, MG, XC}; ld_corr / cor_p: row stride of the lookup's output and one
    direction's block in it; rows7 / tapsum: the packed forms of convf1 and flow_head.conv2 (MOFNetHIP._pack);
    maps: corr, c1, cf, f1, fh, fh_taps, frows, delta, flow4, coords1."""
    return types.SimpleNamespace(P=P, nm=nm, AF=AF, h=h, w=w, Pn=h * w, geo=geo, R=R, G=G, GLD=GLD, ld_corr=ld_corr, cor_p=cor_p,
                                 rows7=rows7, tapsum=tapsum,
                                 fuse=AF == hip.FMT_S16,      # the fused flow-head / flow-half launches read split rows
                                 **cols, **maps)


def _put_flow(s):
    """Where a coordinate update leaves the flow: the 4-channel map and channels 124..127 of the motion features."""
    return dict(flow_a=s.flow4, ld_a=4, flow_b=s.G, ld_b=s.GLD, flow_b_off=s.MF + 124, fmt_b=s.AF)


def init_coords(s, n, flow_init=None):
    """coords1 = the grid, flow = 0; flow_init: f32 rows [n * Pn][4] (x, y, 0, 0) in cells that the recurrence starts from
    instead (coords1 = grid + flow_init: the warm start of a MemFlow stream) - the same two launches, the second with a delta."""
    hip.coords_init(s.coords1, n, s.h, s.w)
    hip.coords_update(s.coords1, flow_init, n, s.h, s.w, **_put_flow(s))


def lookup(s, n, r0, tables=(), bidir=None, pyrs=None, cache=None):
    """K5 on n query maps from row r0 on."""
    # pyrs: the maps' pyramids as a list (one direction); else `tables` of their pointers, one per direction and launch - or
    # ONE table with both directions behind one another and `bidir` (the two lookups of an iteration as one launch)
    # cache (with bidir) = (patches, keys, rows, store, counter): the launch keeps each query's gathered texel patch at its
    # state row and gathers only where a window moved since the row's last launch (hip.corr_lookup)
    g = s.geo
    if pyrs is not None:
        hip.corr_lookup(pyrs, g.hl, g.wl, g.ldl, s.R, s.Pn, s.coords1, r0 * 4, 4, s.corr, r0 * s.ld_corr, s.ld_corr,
                        out_fmt=s.AF, vol_fmt=g.VF, vol_tile=g.TILE)
        return
    # (the tables from the first looked-up centre's pyramids on: the second direction's lie M maps behind still)
    t0 = r0 // s.Pn * g.L
    for d, tab in enumerate(tables):
        hip.corr_lookup(None, g.hl, g.wl, g.ldl, s.R, s.Pn, s.coords1, r0 * 4 + 2 * d, 4, s.corr, r0 * s.ld_corr + d * s.cor_p,
                        s.ld_corr, out_fmt=s.AF, table=tab[t0:], nmaps=n, vol_fmt=g.VF, vol_tile=g.TILE, bidir=bidir,
                        cache=cache[:3] + (r0,) + cache[3:] if cache is not None else None)


def ensure_level0(s, n, r0, en):
    """In front of `lookup` on the same n query maps from row r0 on, both directions: compute the tiles of their pyramids'
    on-demand levels (level 0, and the pooled levels of en.levels) that the lookup's windows read and that are not there
    yet, as ONE launch (hip.corr_levels_ensure).  en: the window's record - cells (en.per per direction and centre, the
    second direction M centres behind the first), the dense calls of the levels of one of the pyramids (rows, D, scale,
    levels) and the counters."""
    g = s.geo
    c0 = r0 // s.Pn
    hip.corr_levels_ensure(en.rows, en.D, g.Pv, en.levels, en.scale, en.cells[en.per * c0:], n, 2, en.M, s.coords1, r0 * 4, 4, 2,
                           g.hl[0], g.wl[0], s.R, g.TILE, counters=en.counter, in_fmt=s.AF)


# ---------------------------------------------------------------------- motion encoder
def convc1(s, n, r0):
    wgt, b = s.P[f"{UB}.encoder.convc1"]
    hip.conv2d(s.corr, s.ld_corr, s.ld_corr, n, s.h, s.w, wgt, b, 256, 1, 1, s.c1, 256, epilogue=hip.EPI_RELU,
               in0_off=r0 * s.ld_corr, out_off=r0 * 256, in_fmt=s.AF, out_fmt=s.AF, mfma=s.nm(f"{UB}.encoder.convc1"))


def convc2(s, n, r0):
    wgt, b = s.P[f"{UB}.encoder.convc2"]
    hip.conv2d(s.c1, 256, 256, n, s.h, s.w, wgt, b, 192, 3, 3, s.cf, 256, in0_off=r0 * 256, out_off=r0 * 256,
               pad_h=1, pad_w=1, epilogue=hip.EPI_RELU, in_fmt=s.AF, out_fmt=s.AF, mfma=s.nm(f"{UB}.encoder.convc2"))


def flow_half(s, n, r0):
    """flow -> convf1 -> convf2 -> channels 192..255 of `cf`."""
    nm1, nm2 = s.nm(f"{UB}.encoder.convf1"), s.nm(f"{UB}.encoder.convf2")
    wgt, b = s.P[f"{UB}.encoder.convf1"]
    wgt2, b2 = s.P[f"{UB}.encoder.convf2"]
    if (s.fuse and s.rows7 and nm1 == 1 and nm2 == 1
            and getattr(wgt2, "order", None) == hip.KORDER_CBLOCK64 and wgt.kp == 224 and wgt2.kp == 1152):
        # both layers in one launch, the 128-channel map between them in LDS (vfml_flow_half; same bits)
        hip.flow_half(s.flow4[r0 * 4:], n, s.h, s.w, wgt, b, wgt2, b2, s.cf, 256, out_off=r0 * 256 + 192)
        return
    if s.rows7:
        # 7x7 over the 4-channel flow as 7x1 over the seven horizontal taps' quads per pixel (MOFNetHIP._pack)
        hip.flow_rows7(s.flow4[r0 * 4:], n, s.h, s.w, s.frows[r0 * 32:])
        hip.conv2d(s.frows, 32, 32, n, s.h, s.w, wgt, b, 128, 7, 1, s.f1, 128, pad_h=3, epilogue=hip.EPI_RELU,
                   in0_off=r0 * 32, out_off=r0 * 128, in_fmt=s.AF, out_fmt=s.AF, mfma=nm1)
    else:
        hip.conv2d(s.flow4, 4, 4, n, s.h, s.w, wgt, b, 128, 7, 7, s.f1, 128, pad_h=3, pad_w=3, epilogue=hip.EPI_RELU,
                   in0_off=r0 * 4, out_off=r0 * 128, out_fmt=s.AF, mfma=nm1)
    hip.conv2d(s.f1, 128, 128, n, s.h, s.w, wgt2, b2, 64, 3, 3, s.cf, 256, in0_off=r0 * 128, out_off=r0 * 256 + 192,
               pad_h=1, pad_w=1, epilogue=hip.EPI_RELU, in_fmt=s.AF, out_fmt=s.AF, mfma=nm2)


def encoder_conv(s, n, r0):
    """Motion features [conv out (124) | fx, fy, bx, by]: the flow quad is written by the coordinate update."""
    wgt, b = s.P[f"{UB}.encoder.conv"]
    hip.conv2d(s.cf, 256, 256, n, s.h, s.w, wgt, b, 124, 3, 3, s.G, s.GLD, in0_off=r0 * 256, out_off=r0 * s.GLD + s.MF,
               pad_h=1, pad_w=1, epilogue=hip.EPI_RELU, in_fmt=s.AF, out_fmt=s.AF, mfma=s.nm(f"{UB}.encoder.conv"))


# ---------------------------------------------------------------------- attention read-out (GMA, MemFlow)
def readout_scratch(buf, dev, rows, Pn, AD, ldA, plain, vt=None):
    """The read-out's scratch maps; buf: the engine's named-buffer allocator.  vt (split-row form): the planes V^T is split
    into."""
    ro = types.SimpleNamespace(AD=AD, vt=vt, val=buf("att_v", rows * AD, dev))
    if plain:
        ro.vrows = buf("att_vt", AD * ldA, dev)                  # V^T as split rows [AD][ldA]
        ro.out = buf("att_ro", AD * ldA, dev)                    # the GEMM's primary output [AD][ldA] (unused)
        ro.out_t = buf("att_ro_t", Pn * AD, dev)                 # its transpose: attn . v, [Pn][AD]
        ro.ws = buf("att_ro_ws", AD * ldA + Pn * AD, dev)        # second half of the K axis (vfml.h ksplit_ws)
    return ro


def plane_readout(s, a, ldA, ro, val, val_off=0):
    """ro.out_t [Pn][AD] = plane a . rows `val` (f32 [Pn][AD] from float offset val_off): the plain form's long-K GEMM."""
    hip.transpose_to_s16(val, s.Pn, ro.AD, ro.AD, ro.vrows, ldA, scale=16.0, src_off=val_off)
    hip.conv2d(ro.vrows, ldA, ldA, ro.AD, 1, 1, a, None, s.Pn, 1, 1, ro.out, ldA, out_scale=1.0 / 16.0,
               in_fmt=s.AF, out_t=ro.out_t, ld_out_t=ro.AD, mfma=1, ksplit_ws=ro.ws)


def attention_readout(s, layer, planes, plain, ldA, P8, gamma, att_scale, src, dst, ro, addend=None):
    """columns dst = columns src + gamma * attn . v,  v = `layer`(columns src), per frame with its own attention: planes[k]
    is frame k's P x P matrix of probabilities times att_scale, resident in HBM (4.2 GB at 1080p as split rows, 2.1 GB as a
    plane), and every iteration is one long-K GEMM over it on the MFMA kernel.
    addend (plain form, one frame): f32 rows [Pn][AD] added to attn . v before the scaling - the part of a read-out that
    does not change over the iterations (MemFlow's memory bank); None: no launch is added."""
    if addend is not None and not (plain and len(planes) == 1):
        raise ValueError("attention_readout: an addend needs the plane form and a single frame")
    # plain: the probabilities as ONE f16 each, the WEIGHT plane (hip.PlainWeight) of the GEMM  out^T = V^T . A^T  (V as plain
    # f16 too: one MFMA per product, 64-channel steps of hi halves); the read-out streams the matrix once per iteration and
    # is bound by its bytes.  Else split rows [Pn][ldA] of P8 columns, with the residual add fused.
    n, Pn, AD, G, GLD, AF = len(planes), s.Pn, ro.AD, s.G, s.GLD, s.AF
    wgt, b = s.P[layer]
    hip.conv2d(G, 128, GLD, n, s.h, s.w, wgt, b, AD, 1, 1, ro.val, AD, in0_off=src, in_fmt=AF, mfma=s.nm(layer))
    for k, a in enumerate(planes):
        if plain:
            plane_readout(s, a, ldA, ro, ro.val, k * Pn * AD)
            if addend is not None:
                hip.axpy_f32(addend, ro.out_t, Pn * AD)
            hip.add_to_s16(ro.out_t, AD, G, GLD, G, GLD, Pn, AD, scale=gamma, aux_off=k * Pn * GLD + src,
                           out_off=k * Pn * GLD + dst)
        else:
            vt = ro.vt.fill_transposed(ro.val, Pn, ld=AD, scale=16.0, src_off=k * Pn * AD)
            # rows as the batch axis (1x1 "images"): one GEMM over the whole attention matrix - the LDS-DMA kernel bases
            # its source descriptor at each tile's first row
            hip.conv2d(a, P8, ldA, Pn, 1, 1, vt, None, AD, 1, 1, G, GLD, out_off=k * Pn * GLD + dst,
                       out_scale=gamma / att_scale, epilogue=hip.EPI_ADD_AUX, aux0=G, ld_aux0=GLD,
                       aux0_off=k * Pn * GLD + src, in_fmt=AF, out_fmt=AF, aux_fmt=AF,
                       mfma=s.nm(layer.rsplit(".", 1)[0] + ".readout"))


# ---------------------------------------------------------------------- temporal fusion, GRU, heads
def temporal_fusion(s, n, stack):
    """`tprop`: a 3x1 convolution along the frame axis of the motion features (MOFNetHIP._pack), mf -> mt."""
    # stack: the n frames are one stack - on the first n frames of a window: row n-1 of a shortened stack sees zero padding
    # where its lower neighbour was, and that row is not among the ng < n the GRU reads.  Else every frame is its own problem
    # (tri-frame networks): its neighbours are the zero padding.
    wgt, b = s.P[f"{UB}.tprop"]
    nb, nh = (1, n) if stack else (n, 1)
    hip.conv2d(s.G, 128, s.GLD, nb, nh, s.Pn, wgt, b, 128, 3, 1, s.G, s.GLD, in0_off=s.MF, out_off=s.MT, pad_h=1,
               epilogue=hip.EPI_RELU, in_fmt=s.AF, out_fmt=s.AF, mfma=s.nm(f"{UB}.tprop"))


def sep_conv_gru(s, n, gate_add, gate_off, gate_ind=None):
    """SepConvGRU, horizontal then vertical."""
    # The context part of every gate convolution (+ bias) reaches it as an addend: gate_add[gate] from float offset
    # gate_off[gate] on - or, gate_ind[gate] = (table, entry), through the device cell that holds the addend's address
    # (fixed launches of a replayed graph).
    G, GLD, AF = s.G, s.GLD, s.AF
    for k, (kh, kw) in (("1", (1, 5)), ("2", (5, 1))):
        ind = {g: gate_ind[g + k] if gate_ind else None for g in ("zr", "q")}
        off = {g: 0 if gate_ind else gate_off[g + k] for g in ("zr", "q")}
        wgt, _ = s.P[f"{UB}.gru.convzr{k}.iter"]
        # [z | r*h] = gates(conv([h | motion | temporal]) + context part)
        hip.conv2d(G, 128, GLD, n, s.h, s.w, wgt, None, 256, kh, kw, G, GLD, in0_off=s.HH, out_off=s.Z,
                   in1=G, c1=s.XC, ld1=GLD, in1_off=s.MF, pad_h=kh // 2, pad_w=kw // 2,
                   epilogue=hip.EPI_GRU_ZR, split=128, aux0=G, ld_aux0=GLD, aux0_off=s.HH,
                   addend=gate_add["zr" + k], ld_addend=256, in_fmt=AF, out_fmt=AF, aux_fmt=AF,
                   addend_off=off["zr"], addend_ind=ind["zr"], mfma=s.nm(f"{UB}.gru.convzr{k}.iter"))
        wgt, _ = s.P[f"{UB}.gru.convq{k}.iter"]
        # h = (1 - z) h + z tanh(conv([r*h | motion | temporal]) + context part), in place
        hip.conv2d(G, 128, GLD, n, s.h, s.w, wgt, None, 128, kh, kw, G, GLD, in0_off=s.RH, out_off=s.HH,
                   in1=G, c1=s.XC, ld1=GLD, in1_off=s.MF, pad_h=kh // 2, pad_w=kw // 2,
                   epilogue=hip.EPI_GRU_Q, aux0=G, ld_aux0=GLD, aux0_off=s.Z,
                   aux1=G, ld_aux1=GLD, aux1_off=s.HH, addend=gate_add["q" + k], ld_addend=128,
                   addend_off=off["q"], addend_ind=ind["q"],
                   in_fmt=AF, out_fmt=AF, aux_fmt=AF, mfma=s.nm(f"{UB}.gru.convq{k}.iter"))


def flow_head(s, n, cout=4):
    """The flow head and the coordinate update behind it.  cout: channels of the plain 3x3 form's output (its map `delta`
    has four per cell)."""
    G, GLD, AF = s.G, s.GLD, s.AF
    wgt, b = s.P[f"{UB}.flow_head.conv1"]
    wgt2, b2 = s.P[f"{UB}.flow_head.conv2"]
    nm1, nm2 = s.nm(f"{UB}.flow_head.conv1"), s.nm(f"{UB}.flow_head.conv2")
    if s.tapsum and s.fuse and nm1 in (3, "2a") and nm2 == nm1:
        # both layers in ONE launch (vfml_conv_desc.proj_out): the 256-channel map stays in LDS, the launch
        # leaves two partial 36-column maps (one per 128-channel half) that the tap sum adds
        hip.conv2d(G, 128, GLD, n, s.h, s.w, wgt, b, 256, 3, 3, s.fh, 256, in0_off=s.HH, pad_h=1, pad_w=1,
                   epilogue=hip.EPI_RELU, in_fmt=AF, out_fmt=AF, mfma=nm1, proj=wgt2, proj_out=s.fh_taps, ld_proj=36)
        hip.tapsum3x3_update(s.fh_taps, 36, b2, n, s.h, s.w, s.coords1, parts=2, part_stride=n * s.Pn * 36, **_put_flow(s))
        return
    hip.conv2d(G, 128, GLD, n, s.h, s.w, wgt, b, 256, 3, 3, s.fh, 256, in0_off=s.HH, pad_h=1, pad_w=1,
               epilogue=hip.EPI_RELU, in_fmt=AF, out_fmt=AF, mfma=nm1)
    if s.tapsum:
        # 256 -> 4 over 3x3 as a 1x1 to 36 tap-major columns + the nine taps summed per pixel (MOFNetHIP._pack)
        hip.conv2d(s.fh, 256, 256, n, s.h, s.w, wgt2, None, 36, 1, 1, s.fh_taps, 36, in_fmt=AF, mfma=nm2)
        hip.tapsum3x3_update(s.fh_taps, 36, b2, n, s.h, s.w, s.coords1, **_put_flow(s))
        return
    hip.conv2d(s.fh, 256, 256, n, s.h, s.w, wgt2, b2, cout, 3, 3, s.delta, 4, pad_h=1, pad_w=1, in_fmt=AF, mfma=nm2)
    update_coords(s, n)


def update_coords(s, n):
    hip.coords_update(s.coords1, s.delta, n, s.h, s.w, **_put_flow(s))


def mask_head(s, n, mask, width):
    """The mask head on the final hidden state: width = 9 * 64 upsampling weights per flow of a cell."""
    wgt, b = s.P[f"{UB}.mask.0"]
    hip.conv2d(s.G, 128, s.GLD, n, s.h, s.w, wgt, b, 256, 3, 3, s.fh, 256, in0_off=s.HH, pad_h=1, pad_w=1,
               epilogue=hip.EPI_RELU, in_fmt=s.AF, out_fmt=s.AF, mfma=s.nm(f"{UB}.mask.0"))
    wgt, b = s.P[f"{UB}.mask.2"]
    hip.conv2d(s.fh, 256, 256, n, s.h, s.w, wgt, b, width, 1, 1, mask, width, out_scale=0.25, in_fmt=s.AF,
               mfma=s.nm(f"{UB}.mask.2"))
