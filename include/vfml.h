/* vfml.h — C ABI of libvfml_hip.so, the MI355X (gfx950) kernels behind the multi-frame
 * optical-flow hot path.
 *
 * The reference (IvanPopov/video-flow-ml) has no FFI of its own: its boundary is the Python
 * object protocol `build_network(cfg)(images, {})` (processing/videoflow_core.py:28,101,188).
 * Everything below that call is PyTorch-CUDA library work (cuDNN conv, cuBLAS bmm, grid_sample,
 * unfold, softmax) launched by the un-vendored VideoFlow submodule.  Each entry point here
 * replaces one of those implicit library ops; the Python host
 * (video-flow-ml_amd/vfml/hip.py) binds them with ctypes and sequences them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA tensor .data_ptr()) unless
 *     the name says host; buffers are borrowed for the duration of the call only;
 *   - activations are NHWC fp32: tensor[n][y][x][c], `ld` = floats between consecutive pixels
 *     (>= channels; lets a kernel read or write a channel slice of a wider buffer);
 *   - channel counts, ld values and base pointers are multiples of 4 floats / 16 bytes;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - return 0 on success, non-zero on a rejected argument or launch error
 *     (text from vfml_last_error(), thread-local).  Nothing is launched on error.
 */
#ifndef VFML_H
#define VFML_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 25 also covers vfml_flow_decode, vfml_flow_diff_overlay, VFML_COMPOSE_GRID_2X3, vfml_resize_u8 and the vfml_jpeg_*
 * entry points (encoder and decoder): additions only, every earlier entry point keeps its signature and its results, so
 * the number did not move.  26 also covers the vfml_jpeg_decode_*_sampled entry points and VFML_JPEG_420 .. _GREY, in the
 * same way: additions only, and the four entry points they generalise forward to them with VFML_JPEG_420; and likewise
 * the three vfml_jpeg_*_sampled entry points of the encoder; and vfml_text_draw, an addition as well; and likewise
 * vfml_attention_plane_f16, vfml_dwconv2d and vfml_gelu_rows.  27 adds vfml_conv2d_split_variant_at; it also covers
 * vfml_layernorm_rows, vfml_window_attention and vfml_attention_shared_keys (the Twins-SVT encoders): additions only;
 * and vfml_attention_bank_planes_f16 and vfml_axpy_f32 (MemFlow's memory bank), additions as well; and likewise
 * vfml_flow_forward_interpolate with its workspace size (the warm start of a MemFlow stream). */
#define VFML_ABI_VERSION 27

/* Epilogue selector of vfml_conv2d.  v = out_scale * (acc + addend[p][c] + bias[c]). */
enum {
  VFML_EPI_NONE = 0,       /* out = v                                                        */
  VFML_EPI_RELU = 1,       /* out = max(v, 0)                                                */
  VFML_EPI_TANH = 2,
  VFML_EPI_SIGMOID = 3,
  VFML_EPI_TANH_RELU = 4,  /* c <  split: tanh(v)   else relu(v)   (cnet -> net | inp)       */
  VFML_EPI_GRU_ZR = 5,     /* c <  split: sigmoid(v) else sigmoid(v) * aux0[p][c - split]    */
  VFML_EPI_GRU_Q = 6,      /* out = (1 - z) * h + z * tanh(v), z = aux0[p][c], h = aux1[p][c] */
  VFML_EPI_ADD_AUX = 7,    /* out = aux0[p][c] + v   (residual / memory read-out: m + gamma*acc)   */
};

/* Activation storage formats.
 *   VFML_FMT_F32  plain NHWC float32.
 *   VFML_FMT_S16  "split rows": same addressing and the same 4 bytes per channel, but every group of
 *                 8 channels (32 bytes, a "unit") holds 8 f16 hi halves then 8 f16 lo halves with
 *                 x = hi + lo (hi = f16(x) rounded to nearest, lo = f16(x - hi)): the operand format of the
 *                 split-f16 MFMA kernel, written once by the producer instead of being re-derived by
 *                 every consumer.  Channel offsets / counts / ld are multiples of 8 (a producer may
 *                 write a 4-channel half unit), bases 32-byte aligned. */
enum { VFML_FMT_F32 = 0, VFML_FMT_S16 = 1,
/* one f16 (round to nearest) per element, row pitches counted in ELEMENTS: only as the output of vfml_conv2d_split's GEMM
 * form (out and out_t: the correlation volumes) and as `vol_fmt` of the lookups that read them back - the opt-in half-size
 * correlation pyramid (cfg.corr_volume = "f16": half the store bytes of the volume GEMMs, half the pyramid memory, fewer
 * sectors per gathered window; the volume's values then carry 11 bits) */
       VFML_FMT_F16 = 2 };

/* Implicit-GEMM 2-D convolution / plain GEMM on the f32 matrix cores.
 *   out[p][co] = epi( sum_{ky,kx,ci} in(p; ky,kx)[ci] * w[co][ky][kx][ci] + bias[co] )
 * The input is the channel-concatenation of up to two NHWC sources (in1 may be NULL).
 * A 1x1/stride-1 conv with N*H*W = rows is a row-major GEMM  out[rows][cout] = A[rows][K]·W[cout][K]^T
 * (used for the all-pairs correlation volume).
 * Replaces: cuDNN conv2d + bias + activation, cuBLAS bmm. */
typedef struct vfml_conv_desc {
  const float* in0; int32_t c0; int32_t ld0;
  const float* in1; int32_t c1; int32_t ld1;       /* optional second source (NULL, 0, 0)     */
  int32_t n, h, w;                                  /* input batch / height / width            */
  const float* weight;                              /* [cout][kh][kw][c0+c1]                   */
  const float* bias;                                /* [cout] or NULL                          */
  int32_t cout, kh, kw, stride, pad_h, pad_w;
  float* out; int32_t ldo;                          /* [n][ho][wo][ldo], ho=(h+2ph-kh)/s+1     */
  int32_t epilogue; int32_t split; float out_scale;
  const float* aux0; int32_t ld_aux0;
  const float* aux1; int32_t ld_aux1;
  const float* addend; int32_t ld_addend;           /* optional f32 map [pixels][ld_addend] added to the
                                                       accumulator before bias/epilogue (a per-pixel bias:
                                                       the part of a convolution whose input does not
                                                       change between calls, computed once)             */
  float* out_t; int32_t ld_out_t;                   /* optional (vfml_conv2d_split, GEMM form only): the
                                                       TRANSPOSE of the result, out_t[co][pixel], row stride
                                                       ld_out_t floats - the all-pairs correlation of frame
                                                       pair (a, b) read the other way round is the volume of
                                                       (b, a): one pass of MFMAs, two stores             */
  int32_t flags;                                    /* VFML_CONV_* bits (vfml_conv2d_split)               */
  double* stats_part;                               /* optional (vfml_conv2d_split, plain f32 output): per block of G
                                                       consecutive output pixels and output channel, the sum and
                                                       the sum of squares of the stored result,
                                                       [n][ceil(hw/G)][cout][2] doubles (hw = output pixels per
                                                       image; n == 1 or hw % G == 0; G = 128 with f32 sources,
                                                       32 with split-row sources - VFML_STATS_ROWS_*): the first
                                                       pass of vfml_instnorm_stats done where the tile still is
                                                       in LDS; fold with vfml_instnorm_finalize               */
  float* ksplit_ws;                                 /* optional (vfml_conv2d_split, GEMM form, plain f32 out): a workspace
                                                       shaped like out ([n*h*w][ldo] floats), followed - when out_t is
                                                       given - by one shaped like out_t ([cout][ld_out_t]).  A GEMM with
                                                       few output tiles and a long K axis (the MemFlow read-out: 254
                                                       tiles on 512 resident slots, K = 32 400) is then run as two work
                                                       items per tile, one per half of K: the second half's sums go to
                                                       the workspace and are added to out / out_t (first + second, a
                                                       fixed order) by passes the call launches itself */
  /* optional projection epilogue (vfml_conv2d_split; split-row sources, VFML_EPI_RELU, no addend, cout % 128 == 0, the
     full split product): relu(out) is NOT stored (out is not written).  Per 128-column tile t of the output the kernel
     multiplies the tile, still in LDS, by that tile's slice of a second weight [proj_n][cout] and stores the partial sums
         proj_out[t][p][j] = sum_{c in 128 t .. 128 t + 127} relu(out[p][c]) * proj_w[j][c],   j < proj_n <= 48,
     proj_out = [cout / 128][n*ho*wo][ld_proj] floats; the caller adds the cout / 128 maps (vfml_tapsum3x3 does).  proj_hi /
     proj_lo: the f16 planes [proj_n][proj_kp] of proj_w * proj_scale (vfml_split_f16; lo behind hi within 1 GiB), three
     MFMAs per product (with VFML_CONV_MFMA2A two, in the projection as in the convolution: relu(out) as plain f16).  The flow head - 3x3 to 256 channels, ReLU, 256 -> 4 over 3x3 as a 1x1 to 36 tap-major columns -
     as ONE launch whose 256-channel map never travels to HBM and back.  Replaces: the second cuDNN conv of
     FlowHead. */
  const void* proj_hi; const void* proj_lo; int32_t proj_n; int32_t proj_kp; float proj_scale;
  float* proj_out; int32_t ld_proj;
  /* optional (vfml_conv2d_split): a DEVICE cell (8-byte aligned) holding the addend pointer to use, read when the kernel
     runs - the launch can sit in a replayed HIP graph while the per-pixel bias it adds (the context part of a GRU gate
     convolution, kept per frame) lives somewhere else from field to field.  `addend` must still be given: a pointer of the
     same shape and alignment, which is what the call validates (vfml_ptr_table_set writes such cells). */
  const float* const* addend_ind;
} vfml_conv_desc;

/* flags: accumulate the two cross terms of the split product in the order (a_lo*b_hi, a_hi*b_lo) instead of
 * (a_hi*b_lo, a_lo*b_hi).  out[q][s] of a call with operands (A, B) and out[s][q] of the call with operands
 * (B, A) and this flag are then the same sequence of f32 additions, i.e. bit-identical - which makes a
 * correlation volume computed directly equal to the one obtained as another call's out_t. */
enum { VFML_STATS_ROWS_F32 = 128, VFML_STATS_ROWS_S16 = 32 };
enum { VFML_CONV_SWAP_CROSS = 1,
/* Fewer MFMAs per product, per call (the per-layer precision plan of the network, cfg.precision):
 *   VFML_CONV_MFMA2  the weight operand as ONE f16 (its hi plane; hi is the round-to-nearest f16 of the weight, so the
 *                    dropped a*w_lo term is an unbiased 2^-12 relative perturbation of each weight): a_hi w + a_lo w;
 *   VFML_CONV_MFMA2A the ACTIVATION operand as one f16 instead: a_hi w_hi + a_hi w_lo.  The weights keep their 22 bits;
 *                    the activations' rounding is independent from pixel to pixel and iteration to iteration, where a
 *                    rounded weight is the same perturbation everywhere (measured at 1080p: 10-30x less end-point
 *                    error than VFML_CONV_MFMA2 on the same layer), and the activation operand is the larger stream;
 *   VFML_CONV_MFMA1  both operands as one f16: a_hi w_hi - plain f16 inputs, f32 accumulate ("fp16" arithmetic).
 * The lo halves that are not used are not fetched.  Where a tile shape / loader combination is not built for the
 * reduced count the call runs with three MFMAs (never less accurate than asked). */
       VFML_CONV_MFMA2 = 2, VFML_CONV_MFMA1 = 4, VFML_CONV_MFMA2A = 8,
/* Stage the activations once per TAP (conv_gemm_dma_kernel) even where the kernel that stages them once per filter
 * ROW and shifts the fragment reads (conv_gemm_tapx_kernel: stride-1 "same" convolutions over split-row sources with
 * 2..5 taps per row) would take the call.  Same arithmetic in the same order - bit-identical results; for A/B
 * measurements and the test that says so. */
       VFML_CONV_PER_TAP = 16 };

int vfml_conv2d(const vfml_conv_desc* d, void* stream);

/* The kernel the same vfml_conv2d / vfml_conv2d_split call would launch, as a profiler prints it (for instance
 * "conv_gemm_dma_kernel<2, 1, 2, 2, false, true, false, 3, true, false>"), written to buf[len]: the call is validated and
 * planned, nothing is launched.  A descriptor the launching call rejects is rejected here with the same error.  Needs
 * no GPU: pointers are compared and checked for alignment, never followed. */
int vfml_conv2d_variant(const vfml_conv_desc* d, char* buf, int len);
int vfml_conv2d_split_variant(const vfml_conv_desc* d, const void* w_hi, const void* w_lo, int kp, float w_scale,
                              int in_fmt, int out_fmt, int aux_fmt, int k_order, char* buf, int len);
/* The instantiations of the vfml_conv2d_split kernels that exist, one per index from 0: the rows of the register-staged
 * kernel's table, then the LDS-DMA kernel's, then the shared-stage kernel's, each named as vfml_conv2d_split_variant names
 * it.  Non-zero (and no error text) past the last row; for the test that holds the tables against the calls that reach
 * them.  Needs no GPU. */
int vfml_conv2d_split_variant_at(int index, char* buf, int len);

/* Same contract on the f16 matrix cores with fp32-grade accuracy ("split-f16": x = hi + lo with
 * hi = f16(x), lo = f16(x - hi); a*b ~= ah*bh + ah*bl + al*bh, 3 MFMAs per product, ~22 mantissa
 * bits).  d->weight is ignored; w_hi / w_lo are the two f16 planes [cout][kp] made by
 * vfml_split_f16 from the [cout][K] weight matrix times `w_scale`, kp = K rounded up to a multiple
 * of 32; the kernel divides the accumulator by w_scale.  Activations stay fp32 in HBM and are split
 * while staged into LDS.
 * w_lo == NULL: the second operand is ONE plain f16 plane (up to 2 GiB), a product is two MFMAs (a_hi b + a_lo b);
 * GEMM form only (split-row source, 1x1 over whole 32-channel blocks, plain f32 out, cout >= 1024). */
int vfml_conv2d_split(const vfml_conv_desc* d, const void* w_hi, const void* w_lo, int kp, float w_scale,
                      int in_fmt, int out_fmt, int aux_fmt, int k_order, void* stream);
/* in_fmt: format of in0/in1; out_fmt: of out; aux_fmt: of aux0/aux1 (VFML_FMT_*).
 * k_order: order of the K axis of the weight planes.
 *   VFML_KORDER_TAP     [cout][ky][kx][ci], kp = kh*kw*(c0+c1) rounded up to 32 (as d->weight).
 *   VFML_KORDER_CBLOCK  [cout][ci/32][ky][kx][ci%32], channels zero padded to a multiple of 32,
 *                       kp = kh*kw*roundup32(c0+c1); split-row sources only.  All taps of one
 *                       32-channel block are consecutive K steps, so the kh*kw reads of an input line
 *                       happen while it is still in L2 (tap-major order re-reads it ctot/32 steps later,
 *                       from the Infinity Cache or HBM).  For 1x1 convolutions the two orders coincide.
 * Split-row sources (in_fmt VFML_FMT_S16) are staged by LDS-DMA: c0, c1, ld0, ld1 multiples of 8, at least 32
 * channels, and w_hi / w_lo within 1 GiB of each other (halves of one allocation, as vfml_split_f16's callers
 * make them) because both planes are read through one buffer descriptor.  A 1x1 / stride-1 convolution over ONE
 * split-row source (GEMM rows) may span any number of bytes (the descriptor is rebased per tile); every other
 * source must span < 1 GiB, both sources of a two-source call must lie within 2 GiB of each other.  Plain f32
 * outputs at least 1024 channels wide (cout % 4 == 0) take the persistent GEMM form of the kernel. */
/*   VFML_KORDER_CBLOCK64 [cout][ci/64][ky][kx][ci%64]: the order of VFML_CONV_MFMA1 calls whose sources are whole 64-channel
 *                       blocks (c0, c0+c1 multiples of 64; kp = K): the kernel then steps 64 channels of hi halves at a
 *                       time (half the K steps and LDS-DMA instructions of the 32-channel steps, no lo half fetched). */
enum { VFML_KORDER_TAP = 0, VFML_KORDER_CBLOCK = 1, VFML_KORDER_CBLOCK64 = 2 };

/* scale * f32 rows [rows][c] (row stride ld_src floats) -> split rows [rows][ld_dst] (VFML_FMT_S16); c % 4 == 0.
 * (scale: a power of two keeps the split exact - the correlation GEMM's query rows carry x16.) */
int vfml_to_s16(const float* src, int64_t rows, int c, int ld_src, float* dst, int ld_dst, float scale, void* stream);

/* y = scale * src (f32 [rows][k], row stride ld floats) -> hi = f16(y), lo = f16(y - hi), each
 * [rows][kp], zero padded from k to kp (kp % 32 == 0).  A power-of-two scale that brings max|y|
 * near 2^14 keeps the lo halves out of the f16 subnormal range. */
int vfml_split_f16(const float* src, int64_t rows, int k, int ld, float scale, void* hi, void* lo, int kp,
                   void* stream);

/* Row softmax: out[r][c] = scale * exp(x[r][c] - max_r) / sum_r for c < cols, written as split rows
 * (VFML_FMT_S16) and zero-filled up to ld_out (ld_out % 8 == 0, ld_out >= cols).  x: f32 [rows][ld_in].
 * scale (a power of two <= 2^15; the consumer divides it out through out_scale) keeps small probabilities out of
 * the f16 subnormal range: a 1080p row has 32400 of them, 3e-5 on average, and unscaled every one would lose up to
 * 6e-8 - 0.1 % of the row's mass.
 * Replaces: torch.softmax over the key axis of the attention scores (materialised:
 * with 288 GB of HBM the P x P score matrix of one frame simply stays resident). */
int vfml_softmax_rows_s16(const float* x, int64_t rows, int cols, int64_t ld_in, float* out, int64_t ld_out, float scale,
                          void* stream);

/* The same softmax as ONE round-to-nearest f16 per element, rows of ld_out halves (ld_out % 8 == 0, <= 32768): the
 * hi-only weight plane of vfml_conv2d_split (w_lo == NULL).  For MemFlow's attention matrix this halves the bytes
 * its 12 read-outs per field stream; 2^-12 relative per probability, unbiased (measured: 1080p EPE unchanged). */
int vfml_softmax_rows_f16(const float* x, int64_t rows, int cols, int64_t ld_in, void* out, int64_t ld_out, float scale,
                          void* stream);

/* The attention plane of one frame in one call (csrc/attention.hip; SURVEY.md K7 for the GMA aggregator of MOF / BOF):
 *   plane[i][j] = RTN_f16(prob_scale * softmax_j(score_scale * q_i . k_j)),  0 <= i, j < p;  columns p .. ld_plane-1 zero.
 * q, k: f32 rows [p][d] (row strides ld_q, ld_k in floats: multiples of 4, 16-byte aligned bases), the layout a 1x1
 * convolution with VFML_FMT_F32 output writes; d = 128 is the only value built; |q|, |k| < 4094 (the operands are split as
 * f16 halves of 16 x).  plane: [p][ld_plane] f16, the weight plane vfml_conv2d_split takes with w_lo == NULL:
 * ld_plane % 64 == 0, p <= ld_plane <= 32768, 16-byte aligned.  Two passes over the key tiles on the matrix cores, three
 * split terms per product in both: pass 1 leaves every row's maximum and sum in `workspace`
 * (vfml_attention_plane_workspace_bytes(p) = 2 p floats), pass 2 forms the scores again and stores the probabilities - the
 * p x p scores never reach memory.  prob_scale in [1, 2^15].  Stream-ordered, no host synchronisation (capturable); a bad
 * argument returns non-zero with vfml_last_error set and launches nothing. */
int64_t vfml_attention_plane_workspace_bytes(int p);
int vfml_attention_plane_f16(const float* q, int64_t ld_q, const float* k, int64_t ld_k, int p, int d, float score_scale,
                             float prob_scale, void* plane, int64_t ld_plane, void* workspace, void* stream);

/* The bank form of the call above (MemFlow's memory): the p queries of one frame against n_seg key
 * sets of p rows each - the keys of earlier fields and the frame's own -, the softmax taken JOINTLY over all n_seg * p
 * columns, written as n_seg planes:
 *   planes[s][i][j] = RTN_f16(prob_scale * exp(t_isj) / sum_{s', j'} exp(t_is'j')),  t_isj = score_scale * q_i . keys[s]_j,
 * columns p .. ld_plane-1 of every plane zero.  keys / planes: HOST arrays of n_seg device pointers (copied into the
 * launch: they may be freed when the call returns); every key set f32 rows [p][d] of the common row stride ld_k
 * (ld_k % 4 == 0, 16-byte aligned), every plane [p][ld_plane] f16 (ld_plane % 64 == 0, p <= ld_plane <= 32768, 16-byte
 * aligned; offsets into a plane are computed in 64 bits).  1 <= n_seg <= 9.  Arithmetic, operand domain (|x| < 4094), d = 128,
 * prob_scale and the workspace (vfml_attention_plane_workspace_bytes(p): every row's joint maximum and sum) as above; a
 * set's last key tile is partial whenever p % 64 != 0 and its dead keys count as -inf.  With n_seg = 1 the plane is the one
 * vfml_attention_plane_f16 writes, bit for bit (tests/test_gpu_memflow_memory.py).  Stream-ordered, no host
 * synchronisation; a bad argument returns non-zero with vfml_last_error set and launches nothing. */
int vfml_attention_bank_planes_f16(const float* q, int64_t ld_q, const float* const* keys, int64_t ld_k, int n_seg, int p, int d,
                                   float score_scale, float prob_scale, void* const* planes, int64_t ld_plane, void* workspace,
                                   void* stream);

/* y += scale * x over n floats (n % 4 == 0, both 16-byte aligned, no overlap): the memory part of MemFlow's read-out is
 * summed over the bank's planes, and added to every iteration's own, with it. */
int vfml_axpy_f32(const float* x, float* y, int64_t n, float scale, void* stream);

/* src f32 [rows][c] (row stride ld) -> SPLIT ROWS of its transpose times scale: dst[c][ld_dst] (VFML_FMT_S16, ld_dst =
 * rows rounded up to 32, pad channels zero): the activation operand of out^T = V^T . A^T. */
int vfml_transpose_to_s16(const float* src, int rows, int c, int ld, float scale, float* dst, int64_t ld_dst, void* stream);

/* Depthwise k x k convolution over NHWC rows, bias, optional residual and optional GELU fused (csrc/dwconv.hip; SURVEY.md
 * K6 for the SK update block of MOF / BOF):
 *   out[p][ch] = act(res ? x[p][ch] + conv : conv),  conv = bias[ch] + sum_{ky,kx} weight[ch][ky][kx] * x(p; ky - k/2, kx - k/2)[ch]
 * a cross-correlation, as nn.Conv2d(groups = c) is, with zero padding at the edges of each of the n frames (which are
 * independent).  x: [n][h][w] rows of ld_x floats, out: rows of ld_out floats - the pointers already at the first channel, so
 * a block reads its input in place from a wider row; in_fmt / out_fmt: VFML_FMT_F32 (c, ld multiples of 4, 16-byte aligned)
 * or VFML_FMT_S16 (c, ld multiples of 8, 32-byte aligned; x = hi + lo on load, hi = RTN f16(y), lo = f16(y - hi) on store).
 * weight: [c][k][k] f32, bias: [c] f32, both 16-byte aligned; k odd, 1 <= k <= 15 (k = 1: a per-channel scale).  flags:
 * VFML_DW_RESIDUAL | VFML_DW_GELU; GELU is the exact one, 0.5 v (1 + erf(v / sqrt 2)).  f32 FMAs on the vector ALU, the
 * operands never rounded to f16.  In place (out == x) is refused: a tile's halo is another tile's output.  Stream-ordered,
 * no host synchronisation (capturable); a bad argument returns non-zero with vfml_last_error set and launches nothing.
 * Replaces: cuDNN's grouped convolution + add + GELU of SKFlow's PCBlock. */
enum { VFML_DW_RESIDUAL = 1, VFML_DW_GELU = 2 };
int vfml_dwconv2d(const float* x, int64_t ld_x, int n, int h, int w, int c, int k, const float* weight, const float* bias,
                  float* out, int64_t ld_out, int in_fmt, int out_fmt, int flags, void* stream);

/* out[r][ch] = gelu(x[r][ch]) over [rows][c] in either format (as vfml_dwconv2d's); in place allowed where format and row
 * stride agree.  The GELU behind a dense 1x1 convolution of a PCBlock. */
int vfml_gelu_rows(const float* x, int64_t ld_x, float* out, int64_t ld_out, int64_t rows, int c, int in_fmt, int out_fmt,
                   void* stream);

/* The three kernels of the Twins-SVT encoders (csrc/twins.hip).  Rows are in either format, as
 * vfml_dwconv2d's (the pointers already at the first channel of a possibly wider row); the head dimension is 32.  All three
 * are stream-ordered without host synchronisation (capturable); a bad argument returns non-zero with vfml_last_error set and
 * launches nothing.
 *
 * vfml_layernorm_rows: out[r][ch] = gamma[ch] * (x[r][ch] - mean_r) / sqrt(var_r + eps) + beta[ch] over the c channels of each
 * row, biased variance, f32 statistics (mean first, then the variance of x - mean: no cancellation); c a multiple of 8, at
 * most 2048; the row is read once.  In place allowed where the row strides agree (the formats may differ).
 * Replaces: nn.LayerNorm over the token dimension. */
int vfml_layernorm_rows(const float* x, int64_t ld_x, float* out, int64_t ld_out, int64_t rows, int c, const float* gamma,
                        const float* beta, float eps, int in_fmt, int out_fmt, void* stream);

/* vfml_window_attention: locally-grouped self attention.  qkv: [n*h*w] rows of the real token grid, channels q | k | v (c each,
 * head-major, c = heads * 32); the grid is cut into ws x ws windows anchored at (0, 0) (ws = 7 is the only size built), and a
 * window position outside the grid (right / bottom) takes pad_row ([3c] f32: its q | k | v) - it is a key like any other, not
 * masked.  Per window and head out = softmax(q k^T / sqrt 32) v over the 49 tokens; out: [n*h*w] rows of c channels, real
 * tokens only.  Scores, softmax and read-out stay on chip.  Replaces: timm's LocallyGroupedAttn between qkv and proj. */
int vfml_window_attention(const float* qkv, int64_t ld, int n, int h, int w, int c, int heads, int ws, const float* pad_row,
                          float* out, int64_t ld_out, int in_fmt, int out_fmt, void* stream);

/* vfml_attention_shared_keys: per frame and head, p queries against the same pk keys and values.  q: [n*p] rows of c = heads * 32
 * channels; kv: [n*pk] rows, channels k | v (c each); out[i] = softmax_j(q_i . k_j / sqrt 32) v_j, [n*p] rows of c channels.
 * f32 products on the f32 matrix cores (v_mfma_f32_32x32x2_f32), online softmax over key chunks staged in LDS: no score
 * reaches memory; pk >= 1, any size.  Replaces: timm's GlobalSubSampleAttn between q / kv and proj (cuBLAS bmm + softmax). */
int vfml_attention_shared_keys(const float* q, int64_t ld_q, const float* kv, int64_t ld_kv, int n, int p, int pk, int c, int heads,
                               float* out, int64_t ld_out, int q_fmt, int kv_fmt, int out_fmt, void* stream);

/* out = aux + scale * x:  x f32 [rows][ldx], aux / out split rows (c % 8 == 0 channels). */
int vfml_add_to_s16(const float* x, int64_t ldx, const float* aux, int64_t ld_aux, float* out, int64_t ld_out, int64_t rows,
                    int c, float scale, void* stream);

/* src f32 [rows][c] (row stride ld) -> split-f16 planes of its TRANSPOSE times scale: hi/lo [c][kp],
 * kp >= rows, kp % 32 == 0, zero padded: the "weight" operand of out = attn . V. */
int vfml_transpose_split_f16(const float* src, int rows, int c, int ld, float scale, void* hi, void* lo, int kp,
                             void* stream);

/* K1: frames -> normalised NHWC4 (4th channel zero):  dst = scale * x + shift.
 * kind 0: src is uint8 [n][H][W][3] (values 0..255, x = u8/255 as the reference does at
 *         processing/videoflow_processor.py:154);  kind 1: src is float32 [n][3][H][W]. */
int vfml_frames_to_nhwc4(const void* src, int kind, int n, int H, int W,
                         float scale, float shift, float* dst, void* stream);

/* Instance norm (affine-free, eps, biased variance) over NHWC x[n][hw][c] (dense, ld == c).
 * stats[n][c] = {mean, rstd}; workspace >= vfml_instnorm_workspace_bytes(n, hw, c).
 * Replaces: nn.InstanceNorm2d in the encoders. */
int64_t vfml_instnorm_workspace_bytes(int n, int hw, int c);
int vfml_instnorm_stats(const float* x, int n, int hw, int c, float eps,
                        float* stats, void* workspace, void* stream);
/* out = relu( norm(x; stats) )                                  if res == NULL
 * out = relu( res' + relu(norm(x; stats)) )                     otherwise, where
 *       res' = res (res_stats == NULL) or norm(res; res_stats)  (down-sampled shortcut).
 * out_fmt VFML_FMT_S16: out - and a res without res_stats, which is an earlier out - are split rows (c % 8 == 0): the
 * operand format of the LDS-DMA convolution kernel that consumes them; x (a convolution's raw result) and a res with
 * res_stats stay f32. */
int vfml_instnorm_apply(const float* x, const float* stats, const float* res,
                        const float* res_stats, int n, int hw, int c, float* out, int out_fmt, void* stream);

/* 2x2/stride-2 average pooling (floor) of an NHWC map; used to build the pooled target-feature
 * pyramid so that pyramid level l of the correlation volume is one GEMM against level-l
 * features (avg-pool commutes with the dot product). */
int vfml_avgpool2x2(const float* x, int n, int h, int w, int c, float* out, void* stream);

/* K5: correlation lookup.  nmaps query maps (correlation problems) of q_per_map queries each; query q
 * of map m reads row q of that map's pyramid.  For each query sample a (2r+1)^2 window around
 * coords/2^l with bilinear interpolation, zeros outside, RAFT's window order (channel i*(2r+1)+j
 * samples x+d[i], y+d[j]).
 *   pyr[m*levels+l] : float [q_per_map][ld[l]]  (columns = hl[l]*wl[l] targets, row-major); host array
 *                     of device pointers - each problem's pyramid may live in its own allocation
 *   vol_tile        : 0, or tws + 16 * ths: every level image is stored as tiles of 2^tws x 2^ths texels (tile after
 *                     tile, left to right then down; a tile row-major; edge tiles whole, so ld[l] >= the tiles' texels),
 *                     and so is the query grid that orders the ROWS: query q = (y, x) of the hl[0] x wl[0] grid reads
 *                     row tile_position(y, x) (q_per_map == hl[0]*wl[0]; rows of pad positions are never read).  What the
 *                     volume GEMM writes when both its operands' rows are in that order (the engine: 4 x 8 tiles - a
 *                     lookup window then lies in ~8 lines of 128 bytes instead of ~13)
 *   coords          : float [nmaps*q_per_map][ld_coords], x at +0, y at +1
 *   out             : [nmaps*q_per_map][ld_out], levels*(2r+1)^2 channels written from out
 * Replaces: F.grid_sample(align_corners=True) x levels. */
int vfml_corr_lookup(const float* const* pyr, const int32_t* hl, const int32_t* wl,
                     const int32_t* ld, int levels, int radius, int nmaps, int q_per_map,
                     const float* coords, int ld_coords, float* out, int ld_out, int out_fmt, int vol_fmt, int vol_tile,
                     void* stream);
/* out_fmt VFML_FMT_S16: channels are written as split rows; the channel count is rounded up to a
 * multiple of 8 with zero channels (out is 32-byte aligned, ld_out % 8 == 0).
 * vol_fmt VFML_FMT_F32, or VFML_FMT_F16: the pyramids hold one f16 per element (ld in elements; radius 3 or 4, at most four
 * levels), or VFML_VOL_F16_LEVELS(m): only the levels whose bit is set in m do (m = 14: levels 1-3, 12: levels 2-3, 8: level
 * 3; the coarse levels cost the fewest bits of the flow and the lookup reads as many texels of each level as of level 0). */
#define VFML_VOL_F16_LEVELS(m) (0x100 | (m))

/* The same lookup with the pyramid pointers read from a DEVICE table at run time: table[m * levels + l] is what
 * pyr[m * levels + l] is above.  A launch recorded in a HIP graph (the update iterations of a field are a fixed launch
 * sequence, replayed per field) then follows whatever pyramids the table names when the graph runs.
 * vfml_ptr_table_set writes n <= 48 device pointers into such a table, asynchronously on `stream` (the values travel as
 * kernel arguments: no host buffer has to outlive the call). */
int vfml_corr_lookup_indirect(const float* const* table, const int32_t* hl, const int32_t* wl, const int32_t* ld,
                              int levels, int radius, int nmaps, int q_per_map, const float* coords, int ld_coords,
                              float* out, int ld_out, int out_fmt, int vol_fmt, int vol_tile, void* stream);
/* Both directions of a window's centre frames in ONE launch: `table` holds the forward problems' pyramids of the query maps
 * from entry 0 and their backward problems' from entry dir_tab * levels (dir_tab >= nmaps; 2 * nmaps <= 8 maps per launch).
 * The second direction of query map m reads the coordinates at coords[row * ld_coords + dir_coords ..] and writes to
 * out[row * ld_out + dir_out ..] - what two calls of vfml_corr_lookup_indirect with shifted table / coords / out pointers
 * do, bit for bit. */
int vfml_corr_lookup_indirect_bidir(const float* const* table, const int32_t* hl, const int32_t* wl, const int32_t* ld,
                                    int levels, int radius, int nmaps, int q_per_map, const float* coords, int ld_coords,
                                    int dir_coords, float* out, int ld_out, int dir_out, int dir_tab, int out_fmt, int vol_fmt,
                                    int vol_tile, void* stream);
/* vfml_corr_lookup_indirect_bidir with a patch cache (radius 3 or 4, at most four levels).  What a query gathers - the
 * (2r+2)^2 integer-grid texels of every level, zero outside the level, f16 levels converted - depends on the origins of its
 * windows only, not on the fraction of its coordinate; while the pyramids stay what they are, a query whose origins did not
 * change since its last launch reads that patch back (contiguous, 16-byte loads) instead of gathering it again, and mixes
 * it with the new bilinear weights: the output is the uncached call's, bit for bit.
 *   cache           : float [2][cache_rows][4][(2r+2)^2], 16-byte aligned: a patch per (direction, row)
 *   key             : int32 [2][cache_rows][8], 16-byte aligned: x0, y0 of levels 0..3 as the patch was gathered.  A row
 *                     whose key holds INT32_MIN (a value no origin takes: they are clamped to +-65536 - r) never hits; the
 *                     caller resets the keys whenever a pyramid the table names changes.
 *   cache_rows, row0: rows per direction, and the row of the launch's first query (the launch covers rows row0 ..
 *                     row0 + nmaps * q_per_map - 1 of both directions, and touches no other row of cache and key)
 *   store           : nonzero - a query whose origins differ (a miss) writes its patch and origins; 0 - a miss gathers
 *                     as the uncached call does and leaves cache and key as they are
 *   counter         : optional device cells: [0] += queries that hit, [1] += queries that missed (tests, profiles). */
int vfml_corr_lookup_indirect_bidir_cached(const float* const* table, const int32_t* hl, const int32_t* wl, const int32_t* ld,
                                           int levels, int radius, int nmaps, int q_per_map, const float* coords,
                                           int ld_coords, int dir_coords, float* out, int ld_out, int dir_out, int dir_tab,
                                           int out_fmt, int vol_fmt, int vol_tile, float* cache, int32_t* key, int cache_rows,
                                           int row0, int store, uint32_t* counter, void* stream);
int vfml_ptr_table_set(void* table, const void* const* ptrs, int n, void* stream);

/* Level 0 of correlation pyramids on demand: in front of a lookup, compute the 128 x 64 tiles of the level-0 volumes that
 * the lookup's windows will read and that are not there yet - instead of the dense level-0 GEMM of every frame pair, most
 * of whose values no lookup ever reads.  The values are the ones that GEMM writes, bit for bit.
 *   d, w_hi .. k_order : the dense level-0 call (vfml_conv2d_split's arguments: query rows of one frame as split rows,
 *                     target planes of the other, out = the level-0 buffer, no out_t) of ANY one of the pyramids - it gives
 *                     the shapes and the arithmetic, and must be a call the library runs on the resident-A walk of its GEMM
 *                     form (one MFMA per product, f32 volume, at most 256 channels).  Its three pointers are not used:
 *   cells           : DEVICE table read when the kernel runs (vfml_ptr_table_set), four 8-byte cells per (direction,
 *                     centre), direction 1 starting dir_cells centres behind direction 0:
 *                       [0] query frame's split rows   [1] target frame's hi plane (level 0)
 *                       [2] the pyramid's level-0 buffer   [3] its bitmap: (rows / 128) x ceil(cout / 64 / 32) uint32,
 *                     bit t of row tile m set = tile (m, t) is computed.  A new pair's bitmap is all zero.
 *   coords .. vol_tile : as vfml_corr_lookup_indirect_bidir's, for `centres` query maps of h x w cells.
 *   counter         : optional device cell: the number of tiles computed is added to it (tests, profiles). */
int vfml_corr_level0_ensure(const vfml_conv_desc* d, const void* w_hi, const void* w_lo, int kp, float w_scale, int in_fmt,
                            int out_fmt, int k_order, const void* const* cells, int centres, int dirs, int dir_cells,
                            const float* coords, int ld_coords, int dir_coords, int h, int w, int radius, int vol_tile,
                            uint32_t* counter, void* stream);

/* The same for a list of levels of the pyramids, in ONE launch: level 0 and / or pooled levels whose dense GEMM stores far
 * more than the lookups read (1080p: 6 % of level 1 and 16 % of level 2 are read).  A work unit - (direction, centre, row
 * tile) - goes through the listed levels in ascending order; per level the window of a query lies around its coordinate
 * times 2^-level in the level image, exactly as the lookup places it.
 *   levels[i]       : d, w_hi, w_lo, kp, w_scale, out_fmt - the dense call of that level of ANY one of the pyramids, under
 *                     the conditions of vfml_corr_level0_ensure (a level stored as f16, with fewer than 1024 columns or more
 *                     than 2048 column tiles is refused, never run some other way); level - its number in the pyramid;
 *                     h, w - its image.  Every level has the query map's rows.  At most three levels.
 *   cells           : 1 + 3 * nlevels cells per (direction, centre): [0] the query frame's split rows, then per listed level
 *                     [1 + 3i] the target frame's hi plane of that level  [2 + 3i] the pyramid's buffer of that level
 *                     [3 + 3i] that level's bitmap (rows / 128) x ceil(cout / 64 / 32) uint32.  One level: the layout above.
 *   h, w            : the query map (the level-0 image), which orders the volumes' rows, listed or not.
 *   counters        : optional device array with one cell per pyramid level: the tiles computed at level l are added to
 *                     counters[l].
 * Everything else as vfml_corr_level0_ensure, which is this call with the one level 0. */
typedef struct vfml_corr_level_desc {
  const vfml_conv_desc* d;
  const void* w_hi;
  const void* w_lo;
  int32_t kp;
  float w_scale;
  int32_t out_fmt, level, h, w;
} vfml_corr_level_desc;
int vfml_corr_levels_ensure(const vfml_corr_level_desc* levels, int nlevels, int in_fmt, int k_order,
                            const void* const* cells, int centres, int dirs, int dir_cells, const float* coords,
                            int ld_coords, int dir_coords, int h, int w, int radius, int vol_tile, uint32_t* counters,
                            void* stream);

/* Window set-up of the recurrent state, one launch: state is [ncentres * rows][ld_state] floats, centre frame c owns rows
 * c * rows .. (c + 1) * rows - 1.  `cells` is a DEVICE table of three 8-byte cells per centre frame, read when the kernel
 * runs (vfml_ptr_table_set writes them; a captured launch follows what they hold at replay):
 *   cells[3c]     context map of the frame, [rows][ld_ctx] floats, or 0: its first `cols` columns are copied to columns
 *                 h_off .. h_off + cols - 1 of the frame's state rows (h = the tanh half of the context map);
 *   cells[3c + 1] the frame's slot, [rows][cols] floats, or 0;
 *   cells[3c + 2] VFML_SEED_LOAD: the slot is copied to columns mf_off .. mf_off + cols - 1 of the frame's state rows,
 *                 VFML_SEED_STORE: those columns are copied to the slot, VFML_SEED_NONE: neither.
 * Plain copies of 16-byte quads, whatever activation format the rows hold: every pointer 16-byte aligned, cols, ld_state,
 * ld_ctx, h_off and mf_off multiples of 4, the two column blocks disjoint.  Slots named by two centres of one launch must
 * not be loaded by one and stored by the other.  Replaces the per-centre strided copies that seeded h, and carries a
 * frame's first-iteration motion features from the window that computed them to the windows that reuse them. */
#define VFML_SEED_NONE 0
#define VFML_SEED_LOAD 1
#define VFML_SEED_STORE 2
int vfml_window_seed(const void* cells, int ncentres, int rows, int cols, float* state, int ld_state, int h_off, int mf_off,
                     int ld_ctx, void* stream);

/* The 7x7 convolution over the 4-channel flow map (motion encoder, convf1) as a 7x1 convolution over 32 channels: this pass
 * writes, per pixel, the seven horizontal taps' flow quads (zeros outside the image row) as one split-row block of 32
 * channels - channel kx*4 + c = flow[y][x + kx - 3][c], channels 28..31 zero - 12 MB at 1080p/8; the vertical taps are then
 * the LDS-DMA convolution kernel's own (kh = 7, kw = 1, weights repacked to [cout][ky][kx*4 + c]).  flow: [n*h*w][4] f32,
 * rows: [n*h*w][32] split rows (VFML_FMT_S16, 32-byte aligned). */
int vfml_flow_rows7(const float* flow, int n, int h, int w, float* rows, void* stream);

/* The encoders' 64 -> 64 channel 3x3 convolution (stride 1, padding 1; K2: the residual blocks of `layer1`) with persistent
 * workgroups that keep the weights in registers and one input patch per 4 x 32-pixel tile in LDS:
 *   out[p][0..63] = conv3x3(in)[p] + bias   (plain f32 rows, ldo floats apart),
 * in: split rows (VFML_FMT_S16), the 64 channels from in[p * ld_in]; w_hi / w_lo: the f16 planes [64][576] of the weights *
 * w_scale in VFML_KORDER_CBLOCK order; stats_part (optional): as vfml_conv_desc.stats_part with VFML_STATS_ROWS_S16 (one
 * {sum, sum of squares} pair per 32 consecutive pixels and channel).  The image width must be a multiple of 32.  Full split
 * product, the K order of vfml_conv2d_split: the result and the partial sums are bit-identical to that call's. */
int vfml_conv3x3_c64(const float* in, int ld_in, int n, int h, int w, const void* w_hi, const void* w_lo, int kp, float w_scale,
                     const float* bias, float* out, int ldo, double* stats_part, void* stream);

/* The flow half of the motion encoder as one launch (K6, BasicMotionEncoder.convf1 + convf2 with their ReLUs), for plans that
 * run both layers with ONE MFMA per product (VFML_CONV_MFMA1: plain f16 operands, f32 accumulate):
 *   out[p][0..63] = relu(conv3x3(relu(conv7x7(flow) + b1)) + b2),   flow: [n*h*w][4] f32,
 * out: split rows (VFML_FMT_S16), 64 channels from out[p * ld_out] (32-byte aligned, ld_out % 8 == 0).  w1_hi: the f16 hi
 * plane [128][224] of convf1's weights * w1_scale in the vfml_flow_rows7 layout (K = ky * 32 + kx * 4 + c), w2_hi: the hi
 * plane [64][1152] of convf2's * w2_scale in VFML_KORDER_CBLOCK64 order (K = (c / 64) * 576 + (ky * 3 + kx) * 64 + c % 64);
 * kp1 / kp2 their row pitches in halves (224 / 1152).  The 128-channel map between the two layers lives in LDS only; the
 * result is bit-identical to vfml_flow_rows7 + two vfml_conv2d_split calls with VFML_CONV_MFMA1. */
int vfml_flow_half(const float* flow, int n, int h, int w, const void* w1_hi, int kp1, float w1_scale, const float* b1,
                   const void* w2_hi, int kp2, float w2_scale, const float* b2, float* out, int ld_out, void* stream);

/* A 3x3 "same" convolution with FOUR output channels as a 1x1 convolution to 36 (tap-major: column (ky*3+kx)*4 + o holds
 * sum_c w[o][c][ky][kx] x[.][c]) followed by this pass: out[p][o] = bias[o] + sum over the nine taps inside the image of
 * t[p + (ky-1) w + (kx-1)][(ky*3+kx)*4 + o], taps in ky-major order.  The update block's flow head (256 -> 4) costs nine
 * times fewer MFMA steps this way than as a 3x3 convolution padded to a 32-column tile.  t: [n*h*w][ld_t] f32 (ld_t >= 36,
 * multiple of 4, 16-byte aligned rows), bias: 4 floats or NULL, out: [n*h*w][4] f32.  parts (1..4): t is that many such maps
 * part_stride floats apart (a multiple of 4) whose sum is meant - the partial maps of vfml_conv_desc.proj_out; per tap they
 * are added in order, map 0 first. */
int vfml_tapsum3x3(const float* t, int ld_t, const float* bias, int n, int h, int w, float* out, int parts, int64_t part_stride,
                   void* stream);
/* The same sum used at once as an iteration's flow update: coords1[p] += it, then the flows are emitted as by
 * vfml_coords_update(coords1, delta = that sum, ...) - one launch instead of two, same values. */
int vfml_tapsum3x3_update(const float* t, int ld_t, const float* bias, int n, int h, int w, int parts, int64_t part_stride,
                          float* coords1, float* flow_a, int ld_a, float* flow_b, int ld_b, int fmt_b, void* stream);

/* coords1 += delta (4 floats per pixel: fwd x,y, bwd x,y); flow = coords1 - grid is written to
 * flow_a[p*ld_a..+4] and flow_b[p*ld_b..+4] (either may be NULL).  h,w give the pixel grid,
 * n maps. delta may be NULL (just (re)emit flow).  */
int vfml_coords_update(float* coords1, const float* delta, int n, int h, int w,
                       float* flow_a, int ld_a, float* flow_b, int ld_b, int fmt_b, void* stream);
/* fmt_b VFML_FMT_S16: flow_b points at channel 4 of a split-row unit (16-byte aligned + 8): the four
 * flow values become the second quad of that unit (hi at +0..7, lo at +16..23 of the quad slot). */

/* forward_interpolate: a 1/8-resolution flow projected forward along itself, what the next field of a
 * video starts its recurrence from.  flow: n independent maps of [h][w] rows of ld_in floats (ld_in >= 2), channels 0..1 =
 * (x, y) in cells; flow4 of the update block has ld_in = 4.  Source cell s = (xs, ys) lands at x1 = f32(xs) + f.x,
 * y1 = f32(ys) + f.y (one f32 addition each) and is VALID iff 0 < x1 < w and 0 < y1 < h (strict; NaN and infinities fail).
 * Target cell (x, y) takes flow[s*] of the valid source of least d2 = (x1 - x)*(x1 - x) + (y1 - y)*(y1 - y) - every
 * operation a single f32 one rounded to nearest, nothing contracted -, ties to the LOWEST row-major source index; with no
 * valid source the map is zero.  out: rows of ld_out floats (ld_out >= 2), channels 0..1 written, and with ld_out >= 4
 * channels 2..3 written as zero - with ld_out = 4 the `delta` operand of vfml_coords_update; out may not overlap flow.
 * index: NULL, or int32 [n][h*w] that receives s* per cell (-1: no valid source).  An exact brute-force search, h*w <= 2^24:
 * (h*w)^2 distance evaluations per map; partial minima of 2048-source chunks go through `workspace`
 * (vfml_flow_forward_interpolate_workspace_bytes(n, h, w) bytes, 8-byte aligned; 0 for sizes that are refused) as 64-bit
 * keys and are combined by an integer minimum: results are bit-identical from run to run.  Two launches, stream-ordered, no
 * host synchronisation (capturable); a bad argument returns non-zero with vfml_last_error set and launches nothing. */
int64_t vfml_flow_forward_interpolate_workspace_bytes(int n, int h, int w);
int vfml_flow_forward_interpolate(const float* flow, int ld_in, int n, int h, int w, float* out, int ld_out, int32_t* index,
                                  void* workspace, int64_t workspace_bytes, void* stream);
/* coords1[p] = (x, y, x, y) */
int vfml_coords_init(float* coords1, int n, int h, int w, void* stream);

/* K8: 8x convex upsampling of one flow (2 of the 4 coords channels) of one map.
 *   coords1: [h][w][4] of that map (flow = coords1[ch..ch+1] - grid), mask: [h][w][ld_mask]
 *   (576 logits used: tap k (3x3, row-major) * 64 + sy*8 + sx), out: [8h][8w][2] (HWC).
 * Replaces: softmax + F.unfold + sum + permute and the CHW->HWC permute of
 * processing/videoflow_processor.py:185. */
int vfml_convex_upsample(const float* coords1, int ch, const float* mask, int ld_mask,
                         int h, int w, float* out, void* stream);

/* Second pass of vfml_instnorm_stats on partial sums a convolution left behind (vfml_conv_desc.stats_part):
 * part [n][chunks][c][2] doubles -> stats [n][c][2] = {mean, 1/sqrt(var + eps)}, folded in a fixed order.
 * With many partials per channel (chunks >= 1024, c % 8 == 0) they are first folded slice-wise with coalesced reads into
 * `workspace` (caller-owned device memory, at least vfml_instnorm_finalize_workspace_bytes(chunks, c) bytes; a larger
 * one lets more frames of a batch go through per launch).  The route depends on (chunks, c) alone - never on n or on
 * the workspace's size - so a frame's statistics are the same bits alone or in a batch; where the fold route applies a
 * NULL / too small workspace is an error, not another route.  The library keeps no hidden device allocation: calls on
 * different streams are independent as long as their workspaces are (ABI 23; until ABI 22 a per-device static scratch). */
int64_t vfml_instnorm_finalize_workspace_bytes(int chunks, int c);   /* 0: this shape folds without a workspace */
int vfml_instnorm_finalize(const double* part, int n, int chunks, int c, int hw, float eps, float* stats,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* The encoders' stem (K2's first layer): 7x7 convolution, stride 2, padding 3, 4 -> 64 channels, over NHWC4 frames
 * (vfml_frames_to_nhwc4's output) in the split-f16 arithmetic (three MFMAs per product), as one kernel that keeps a tile's
 * input patch and all weights in LDS (csrc/stem.hip).
 *   frames      [n][h][w][4] f32;  out [n][ho][wo][64] f32, ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1
 *   w_hi, w_lo  f16 planes [64][224] of the weights times w_scale, K order ky-major: k = ky * 32 + kx * 4 + c with kx < 8
 *               (kx = 7: zeros) and c < 4 - what vfml_split_f16 makes of a [64][7][8][4] f32 tensor
 *   stats_part  NULL, or [n][vfml_stem7x7s2_chunks(h, w)][64][2] doubles: {sum, sum of squares} of the stored values per
 *               8 x 64-pixel output tile and channel - fold with vfml_instnorm_finalize(chunks = that count)
 * Replaces: the first nn.Conv2d(3, 64, 7, stride=2, padding=3) of the RAFT encoder. */
int vfml_stem7x7s2_chunks(int h, int w);
int vfml_stem7x7s2(const float* frames, int n, int h, int w, const void* w_hi, const void* w_lo, float w_scale,
                   const float* bias, float* out, double* stats_part, void* stream);

/* One level of the flow-cache LOD pyramid (reference storage/cache_manager.py:77-161): out[y][x] =
 * 0.5 * (sum of the 2x2 block's in-image vectors) / (number of in-image cells); odd sides are padded
 * bottom/right with weight 0.  flow: [h][w][2] f32, out: [(h+1)/2][(w+1)/2][2].  Same association as
 * the reference's per-block np.sum, divisions by 1, 2 or 4: bit-exact. */
int vfml_flow_lod(const float* flow, int h, int w, float* out, void* stream);

/* Flow field [h][w][2] f32 (pixels) -> 8-bit RGB image [h][w][3] as the reference's encoders produce it, byte for
 * byte (encoding/flow_encoders.py: GamedevFlowEncoder :70-117, MotionVectorsRG8FlowEncoder :120-153,
 * MotionVectorsRGB8FlowEncoder 'rgb+' :242-293).  gamedev: (flow / (width, height)) * scale, clamp, map to
 * [0,1]; rg8: clamp, map; rgb8: direction / magnitude code.  clamp / two_clamp are float32(clamp_range) and
 * float32(2 * clamp_range) (numpy promotes the Python floats that way).  SURVEY.md 8(f)-3. */
enum { VFML_ENCODE_GAMEDEV = 0, VFML_ENCODE_RG8 = 1, VFML_ENCODE_RGB8 = 2 };
int vfml_flow_encode(const float* flow, int h, int w, int mode, float width, float height, float scale,
                     float clamp, float two_clamp, unsigned char* out, void* stream);

/* One temporal-anti-aliasing step: blend the current frame into its history, the history reprojected along the flow
 * field (reference effects/taa_processor.py: apply_taa :42-89, _apply_flow_based_taa :92-146,
 * _bilateral_reprojection_sample :148-216, _bilinear_sample :218-263).  SURVEY.md 8(f)-3.
 *   current: [h][w][3] u8 or f32 (0..255); flow: [h][w][2] f32, pixels, pointing from a pixel to where it was in the
 *   history image (NULL in SIMPLE mode); history: [h][w][3] f32 or f64; out: [h][w][3], never the history buffer.
 *   SIMPLE    out = alpha*current + (1-alpha)*history                         (out type = history type)
 *   BILINEAR  history sampled bilinearly at (x, y) + flow, clamped to the image (out f32)
 *   BILATERAL the four neighbours weighted by bilinear weight x exp(-(lum - lum_k)^2 / (0.2 sigma_color^2 + 1e-6)),
 *             renormalised (out f64)
 * Every intermediate has the dtype numpy's promotion gives it in the reference, so a sequence of steps tracks the
 * reference's history to the last few ulps (exp() is the only step that is not reproduced bit for bit). */
enum { VFML_TAA_SIMPLE = 0, VFML_TAA_BILINEAR = 1, VFML_TAA_BILATERAL = 2 };
enum { VFML_PIX_U8 = 0, VFML_PIX_F32 = 1, VFML_PIX_F64 = 2 };
int vfml_taa_blend(const void* current, int cur_type, const float* flow, const void* history, int hist_type,
                   void* out, int out_type, int h, int w, int mode, double alpha, double sigma_color, void* stream);

/* Flow quality map (reference correction_worker.py: generate_quality_frame_gpu :175-208): how well frame2, warped
 * back along the flow, matches frame1.  frame1, frame2, out: [h][w][3] u8; flow: [fh][fw][2] f32 at the frame's
 * resolution or at a cached LOD's (then resized bilinearly, align_corners = False, and rescaled by w/fw, h/fh).
 * Per pixel: target = (x, y) - flow, truncated to a texel; similarity = mean of (1 - |d|_2 / 1.732),
 * (1 - mean |d|), (cos + 1) / 2 of the two colours in [0,1]; out = (0, 2 (s - 0.5), 0) * 255 if s > threshold else
 * ((1 - s), 0, 0) * 255; (255, 0, 0) where the target is outside the image.  SURVEY.md 8(f)-4. */
int vfml_flow_quality_map(const unsigned char* frame1, const unsigned char* frame2, const float* flow, int fh, int fw,
                          int h, int w, float threshold, unsigned char* out, void* stream);

/* Batch flow-cache correction (reference correction_worker.py: worker_process :221-341), one frame per call, all on
 * `stream`, no host synchronisation.  frame1, frame2: [h][w][3] u8 RGB; flow: [h][w][2] f32 at the frame's resolution;
 * lod: [lh][lw][2] f32, the coarsest cached LOD of the frame (the flow itself when there is none); twiddles: device
 * [2][50] f64, cos and sin of 2 pi m / 50.  Bad pixels are those whose quality map (vfml_flow_quality_map at
 * good_threshold) has a red byte > 0.  Each is re-estimated by a phase correlation of two 50x50 grey regions around
 * the pixel and its LOD target; where that similarity is < fine_threshold, by an 11x11 TM_CCOEFF_NORMED match over the
 * 50-row search area (as wide as the frame where the reference's slice is) and a spiral search; the better result is
 * written to out_flow (a copy of flow, which it may not alias) when its similarity is > good_threshold or > the
 * pixel's current one.  counts: device int32[2] <- bad pixels before and after.  Only radii 25 / 5.5 / 25 (region,
 * template, search) are built.  records: null, or device f64 [record_capacity][VFML_CORRECT_RECORD] <- per bad pixel
 * in raster order: pixel index, original similarity, LOD vector x/y, phase shift x/y, coarse vector x/y, coarse
 * similarity, fine attempted, fine valid, fine vector x/y, fine similarity, accepted, 0.  workspace: device, at least
 * vfml_flow_correct_workspace_bytes(h, w) bytes.  DESIGN.md section 8 defines every rounding step. */
#define VFML_CORRECT_RECORD 16
size_t vfml_flow_correct_workspace_bytes(int h, int w);
int vfml_flow_correct(const unsigned char* frame1, const unsigned char* frame2, const float* flow, const float* lod,
                      int lh, int lw, int h, int w, const double* twiddles, double good_threshold,
                      double fine_threshold, double region_radius, double template_radius, double search_radius,
                      float* out_flow, int* counts, double* records, int64_t record_capacity, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Flow field [h][w][2] f32 -> RGB [h][w][3] u8 on a colour wheel (reference encoding/flow_encoders.py: HSVFlowEncoder
 * :30-67, TorchvisionFlowEncoder :367-427).  Both normalise by the frame's maximum magnitude, reduced on the device
 * into a u32 cell of `workspace` (4 bytes, 4-byte aligned; cleared by the call) - no host synchronisation.
 *   HSV    nan_to_num(0, 1, -1); H = u8(clip((atan2(y, x) + pi) / 2pi * 180, 0, 180)), S = u8(|f| / max * 255) (0
 *          when max == 0), V = 255; then this project's 8-bit HSV2RGB (OpenCV's sector table, round half to even)
 *   WHEEL  torchvision.utils.flow_to_image's Middlebury wheel on f / (max + FLT_EPSILON), floor(255 col) as u8, then
 *          the reference wrapper's uint8 `* 255`, which wraps: the byte written is (256 - x) mod 256
 * Every f32 step is rounded separately; atan2 is the f64 one rounded to f32.  DESIGN.md section 9.  SURVEY.md row 12. */
enum { VFML_COLORIZE_HSV = 0, VFML_COLORIZE_WHEEL = 1 };
int vfml_flow_colorize(const float* flow, int h, int w, int mode, void* workspace, unsigned char* out, void* stream);

/* Encoded motion vectors -> flow field: the inverse of vfml_flow_encode's RG8 / RGB8 modes as the reference decodes them
 * (encoding/flow_encoders.py: MotionVectorsRG8FlowEncoder.decode, MotionVectorsRGB8FlowEncoder.decode 'rgb+' :336-343).
 * encoded: [h][w][3] u8 RGB, rows contiguous, any alignment (the bottom half of an uploaded --flow-input frame is
 * such a block); flow: [h][w][2] f32, 8-byte aligned; clamp = float32(clamp_range).  n = u8 / 255;
 *   RG8   flow = (n * 2) * clamp - clamp                                   (B is not read)
 *   RGB8  dx = n_r * 2 - 1, dy = n_g * 2 - 1, mag = (1 / sqrt(dx dx + dy dy + n_b n_b)) * clamp, flow = (dx, dy) * mag
 * Every f32 step is rounded separately, quotient and root correctly: bit for bit the host decoder.  VFML_ENCODE_GAMEDEV
 * and unknown modes are rejected.  DESIGN.md section 9. */
int vfml_flow_decode(const unsigned char* encoded, int h, int w, int mode, float clamp, float* flow, void* stream);

/* Radar picture of the difference of two flow fields (reference flow_processor.py: create_difference_overlay :490-578).
 * flow_a, flow_b: [h][w][2] f32, 8-byte aligned; out: [h][w][3] u8 RGB.  m = sqrt(dx dx + dy dy) of a - b in f32, classes
 * against the f32 values of the thresholds: m <= 0.1 green (0,255,0), <= 0.5 yellow (255,255,0), <= 1 orange
 * (255,165,0), <= 2 red (255,0,0), > 2 magenta (255,0,255), NaN black.  The legend is drawn in the same pass: for
 * i = 0..4, x = 10 + 45 i, y0 = h - 20, a white rectangle (x-1, y0-13)..(x+13, y0+1) and over it class i's colour
 * (x, y0-12)..(x+12, y0), corners inclusive, clipped to the picture; its numbers are not drawn.  DESIGN.md section 9. */
int vfml_flow_diff_overlay(const float* flow_a, const float* flow_b, int h, int w, unsigned char* out, void* stream);

/* One output video frame from its tiles (reference visualization/video_composer.py: create_side_by_side :67-122,
 * flow_processor.py: create_6_video_grid :1218-1269), in one pass.  tiles / tile_types: host arrays of 2 (SIDE_BY_SIDE,
 * STACKED), 4 (GRID_2X2) or 6 (GRID_2X3) device images [h][w][3],
 * each VFML_PIX_U8 (RGB bytes) or an f32 / f64 TAA history, which becomes u8 by clip(0, 255) and truncation (NaN -> 0).
 *   SIDE_BY_SIDE  (2w x h)   tile 0 | tile 1                 (original | flow)
 *   STACKED       (w x 2h)   tile 0 over tile 1              (--flow-only)
 *   GRID_2X2      (2w x 2h)  tile 0 | tile 1 over 2 | 3      (original | flow over TAA | TAA simple)
 *   GRID_2X3      (2w x 3h)  0 | 1 over 2 | 3 over 4 | 5     (... over TAA external flow | flow difference; --flow-input)
 * out: rows of row_stride bytes (>= 3 x output width; padding bytes are 0), channels RGB or BGR (VFML_COMPOSE_BGR),
 * top-down or bottom-up (VFML_COMPOSE_BOTTOM_UP, an AVI DIB).  DESIGN.md section 9.  SURVEY.md row 14. */
enum { VFML_COMPOSE_SIDE_BY_SIDE = 0, VFML_COMPOSE_STACKED = 1, VFML_COMPOSE_GRID_2X2 = 2,
       VFML_COMPOSE_GRID_2X3 = 3 };
enum { VFML_COMPOSE_BGR = 1, VFML_COMPOSE_BOTTOM_UP = 2 };
int vfml_compose_frame(const void* const* tiles, const int* tile_types, int h, int w, int layout, int flags,
                       int64_t row_stride, unsigned char* out, void* stream);

/* Text labels and dimmed rectangles on a composed frame, in place (the reference's cv2.putText / addWeighted calls:
 * visualization/video_composer.py :60-63, :206-218, flow_processor.py :570-576).  The text is this project's own: the
 * stroke font of visualization/stroke_font.py, positions in 1/64 px, integer coverage and blending (DESIGN.md section 9,
 * "Text"; tests/text_oracle.py states the rule).  Not pinned against cv2.
 * img: [h][w][3] u8, rows of row_stride bytes (>= 3 w; bytes past 3 w are not touched), channels in memory order - a
 * colour's byte k goes to channel k; flags: VFML_COMPOSE_BOTTOM_UP when row 0 of the picture is the buffer's last row.
 * Stream-ordered, no allocation, no synchronisation.
 * plan: a HOST pointer to plan_words int32 words, written by visualization.text.build_plan.  The entry point checks
 * these words completely before the launch (a truncated plan, an offset outside plan_words, a box or clip outside the
 * image, intersecting boxes and out-of-range geometry are rejected; no GPU is needed for that).  The kernel reads an
 * identical copy in device memory, whose address the host words carry (words 2..3), and bounds again every count,
 * offset and coordinate it takes from that copy.
 *   header   [0] 0x54584656  [1] plan_words  [2] [3] device address of the copy, low and high half
 *            [4] boxes  [5] operations  [6] glyphs  [7] segments            the sections follow in this order, packed
 *   box      x0 y0 x1 y1 (pixels, inclusive, inside the image)  first operation  operations  first block  0
 *            Boxes are pairwise disjoint.  One thread owns one pixel of one box and applies the box's operations in
 *            order; a box takes ceil(width / 32) * ceil(height / 8) blocks, `first block` is the running sum.
 *   op       kind  clip x0 y0 x1 y1 (pixels, inclusive, inside the image)  colour c0 | c1 << 8 | c2 << 16
 *            radius = 32 thickness  anti-aliased 0 / 1  origin x y (1/64 px)  first glyph  glyphs
 *            kind 0 TEXT: out = (colour n + dst (16 - n) + 8) >> 4, n = samples of the pixel within `radius` of a segment
 *            (16 samples at 4 (2 i + 1), 4 (2 j + 1) when anti-aliased, else the pixel centre and n = 0 or 16);
 *            kind 1 DIM_RECT: out = (3 dst + 5) / 10 inside the clip; the words behind the clip are 0.
 *   glyph    x0 y0 x1 y1: the box of its segments relative to the origin (1/64 px, at most 2^14 wide and high)
 *            first segment  segments  0  0
 *   segment  x0 y0 x1 y1 relative to the origin (1/64 px), inside its glyph's box */
int vfml_text_draw(const int32_t* plan, int plan_words, unsigned char* img, int h, int w, int64_t row_stride, int flags,
                   void* stream);

/* Turbulence map of a flow field (reference flow_visualizer.py: generate_turbulence_map :2997-3052): a heat map of the
 * local standard deviation of the flow vectors, all on `stream`, no host synchronisation, no allocation.
 * flow: [fh][fw][2] f32; when (fh, fw) != (h, w) it is first resized bilinearly to h x w with the taps of
 * vfml_flow_quality_map and its x / y scaled by f32(w / fw) / f32(h / fh).  Then, per pixel:
 *   four ksize x ksize box means (x, y, x*x, y*y; squares in f32), BORDER_REFLECT, each the f64 sum times
 *   1.0 / ksize^2 rounded once to f32;  var = mean2 - mean * mean (f32, unfused);
 *   tv = sqrt(max(0, var_x) + max(0, var_y)), correctly rounded.
 * lo, hi = numpy.percentile(tv, 5 / 95) (method 'linear' on the f32 array as numpy 2 evaluates it, found by an exact
 * radix selection on the device);  index = u8(clip((tv - lo) / (hi - lo), 0, 1) * 255) when hi - lo > 1e-6f, else 0;
 * out_bgr: [h][w][3] u8 <- JET[index], B first.  The box filter, the resize and the JET table are this project's
 * definitions of the OpenCV 4 algorithms, not pinned against cv2.
 * ksize: odd, 1..63.  workspace: device, 256-byte aligned, the workspace_bytes function's count; not shared by calls
 * that may run at once.  Optional outputs (null to skip): out_index [h][w] u8, out_tv [h][w] f32 (16-byte aligned),
 * out_lohi [2] f32.  Non-finite vectors give an unspecified picture; every access stays in bounds.  SURVEY.md row 15. */
size_t vfml_flow_turbulence_workspace_bytes(int h, int w);
int vfml_flow_turbulence_map(const float* flow, int fh, int fw, int h, int w, int ksize, void* workspace,
                             unsigned char* out_bgr, unsigned char* out_index, float* out_tv, float* out_lohi,
                             void* stream);

/* Resize n RGB pictures [H][W][3] u8 into [h][w][3] u8: OpenCV's 8-bit INTER_LINEAR scheme as this project defines it
 * (reference video/frame_extractor.py: cv2.resize of every --fast frame), not pinned against cv2.
 * Rows are contiguous; picture f starts at src + f * src_frame_stride / dst + f * dst_frame_stride (bytes, any
 * alignment), so a frame of a clip or a row slice of a larger frame is addressed in place.  All on `stream`, no
 * allocation, no host synchronisation.
 *   (h, w) == (H, W)        the pictures are copied unchanged (tables not read);
 *   H == 2h and W == 2w     out = (a + b + c + d + 2) >> 2 over each 2x2 block (tables not read, may be null);
 *   otherwise               separable, integer only: xtab [w][4] / ytab [h][4] are device tables of int32 rows
 *                           (s, s1, a0, a1), 16-byte aligned, written by the host (vfml/hip.py resize_tables: the tap
 *                           positions and the 11-bit weights, the only float work of the scheme);
 *                           r_y = p[y][s] * a0 + p[y][s1] * a1 for the y table's two rows y0, y1 with weights b0, b1,
 *                           out = u8((((b0 * (r_y0 >> 4)) >> 16) + ((b1 * (r_y1 >> 4)) >> 16) + 2) >> 2), arithmetic shifts.
 * Tap positions are clamped to the picture on the device: every access stays in bounds whatever the tables hold.
 * Sides up to 32768.  SURVEY.md row 11. */
int vfml_resize_u8(const unsigned char* src, int n, int H, int W, int64_t src_frame_stride, unsigned char* dst, int h,
                   int w, int64_t dst_frame_stride, const int32_t* xtab, const int32_t* ytab, void* stream);

/* Baseline JPEG of an RGB picture (the output video's MJPG frames): 8-bit sequential DCT, YCbCr
 * 4:2:0, the T.81 Annex K Huffman tables unoptimised, one MCU row (16 pixel rows) per restart interval.  All integer, all
 * on `stream`, no host synchronisation, no allocation; tests/jpeg_oracle.py is the definition in numpy and the scan
 * equals its scan byte for byte:
 *   the picture is padded to multiples of 16 by edge replication;
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16;  chroma = (a + b + c + d + 2) >> 2 over 2x2 cells;
 *   per 8x8 block X - 128:  T = (C X + 1024) >> 11,  Y = (T C^T + 16384) >> 15  with
 *   C[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16));  q = sign(Y) ((|Y| + (Q >> 1)) / Q), AC clamped to +-1023 and the
 *   DC difference to +-2047;  MCUs in raster order, each Y00 Y01 Y10 Y11 Cb Cr;  predictors zero at the start of every
 *   interval, intervals padded with 1-bits, FF followed by 00, RSTm (m modulo 8) after every interval but the last.
 * rgb: [h][row_stride] bytes, a row = w RGB triples (row_stride >= 3w: a row slice of a larger buffer is addressed in
 * place).  qtables: device, [2][64] bytes, luma then chroma, natural order (storage/jpeg_tables.py quant_tables).
 * workspace: device, 256-byte aligned, vfml_jpeg_workspace_bytes(h, w); not shared by calls that may run at once.
 * scan: receives the entropy-coded data that goes between the SOS segment (storage/jpeg_tables.py jpeg_header) and EOI;
 * *scan_bytes (device, 4-byte aligned) its length.  vfml_jpeg_scan_capacity(h, w) bytes always suffice; with a smaller
 * scan_capacity nothing is written at or past scan + scan_capacity and *scan_bytes still holds the length the picture
 * needs (the caller compares).  Sides of 1..65535 with a worst-case scan below 4 GiB; 0 from the size functions
 * otherwise. */
int64_t vfml_jpeg_workspace_bytes(int h, int w);
int64_t vfml_jpeg_scan_capacity(int h, int w);
int vfml_jpeg_encode_rgb(const unsigned char* rgb, int h, int w, int64_t row_stride, const unsigned char* qtables,
                         void* workspace, unsigned char* scan, int64_t scan_capacity, uint32_t* scan_bytes, void* stream);

/* Decoder of baseline JPEG files (the MJPG frames the drop-in reads): sequential DCT, 8-bit, three
 * components sampled 2x2 / 1x1 / 1x1 in one interleaved scan, any Huffman tables, any restart interval.  All integer, all
 * on `stream`, no host synchronisation, no allocation, no host pass over the entropy data; the picture equals libjpeg's
 * (Pillow's) decode byte for byte and tests/jpeg_decode_oracle.py is the definition in numpy:
 *   entropy  T.81 F.2.2: canonical codes from BITS / HUFFVAL, EXTEND, ZRL = 16 zeros, EOB; DC predictors per component,
 *            zero at the start of every interval; FF 00 is the byte FF, FF D0..D7 ends an interval; ceil(MCUs / Ri)
 *            intervals with markers m = 0, 1, ... modulo 8; MCUs in raster order, each Y00 Y01 Y10 Y11 Cb Cr.
 *   IDCT     coefficient x table entry, then libjpeg's jidctint "islow" butterfly in int32, columns first: pass 1 keeps
 *            (x + 1024) >> 11, pass 2 gives clamp(((x + (1 << 17)) >> 18) + 128, 0, 255).
 *   chroma   libjpeg's h2v2 "fancy" triangle filter on the planes of ceil(h/2) x ceil(w/2): for output row 2r the
 *            neighbour row is r - 1, for 2r + 1 it is r + 1 (clamped); s[c] = 3 C[r][c] + C[nb][c];
 *            out[2c] = (3 s[c] + s[c-1] + 8) >> 4, out[2c+1] = (3 s[c] + s[c+1] + 7) >> 4 (columns clamped).
 *   colour   cb, cr less 128:  R = Y + ((91881 cr + 32768) >> 16),  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *            B = Y + ((116130 cb + 32768) >> 16), clamped to 0..255.
 * scan: device, the scan_bytes of entropy-coded data between the SOS segment and EOI.  restart_interval: the file's Ri, 0:
 * one interval.  qtables: device, [3][64] bytes, the table of Y, Cb, Cr in natural order.  tables: device, 392 int32
 * (storage/jpeg_parse.py decode_tables): tables[2c], tables[2c+1] = which of the four Huffman tables (0..3 = DC0 AC0 DC1
 * AC1) component c's DC and AC codes use; from tables[8] on, 96 ints per table: limit[16], offset[16] and HUFFVAL as 256
 * bytes - a code has the first length l whose limit[l-1] exceeds the next 16 bits v of the stream and the symbol
 * HUFFVAL[offset[l-1] + (v >> (16 - l))].
 * Rows y0 <= y < y1 of the picture are written, row y at rgb + (y - y0) * row_stride as w RGB triples (row_stride >= 3w:
 * a row slice of a larger buffer is a valid destination).  When Ri is a positive multiple of the MCUs per MCU row, only
 * the intervals that hold those luma rows and chroma rows (y0 >> 1) - 1 .. ((y1 - 1) >> 1) + 1 are read at all.
 * workspace: device, 256-byte aligned, vfml_jpeg_decode_workspace_bytes(h, w, scan_bytes) (every region sized for the
 * worst case of h, w and scan_bytes; 0: sides outside 1..65535 or a scan of 2 GiB or more); not shared by calls that may
 * run at once.  *status (device, 4-byte aligned) receives 0 or the OR of VFML_JPEG_ERR_*: a damaged scan is a defined
 * result - every index is clamped or checked on the device, nothing is written outside the workspace and the output
 * rows, whose content is then unspecified. */
enum {
  VFML_JPEG_ERR_INTERVALS = 1,   /* the scan does not hold ceil(MCUs / Ri) intervals          */
  VFML_JPEG_ERR_SEQUENCE = 2,    /* restart markers out of sequence                           */
  VFML_JPEG_ERR_CODE = 4,        /* a code that is in no Huffman table                        */
  VFML_JPEG_ERR_INDEX = 8,       /* a coefficient index past 63                               */
  VFML_JPEG_ERR_DATA = 16        /* an interval's bits ran out before its MCUs did            */
};
int64_t vfml_jpeg_decode_workspace_bytes(int h, int w, int64_t scan_bytes);
int vfml_jpeg_decode_rgb(const unsigned char* scan, int64_t scan_bytes, int h, int w, int restart_interval,
                         const unsigned char* qtables, const int32_t* tables, int y0, int y1, void* workspace,
                         unsigned char* rgb, int64_t row_stride, int32_t* status, void* stream);

/* The same decoder with an entropy stage that does not take its parallelism from restart markers (DESIGN.md section
 * 13.1; tests/jpeg_selfsync_oracle.py is the definition): the scan is cut into subsequences of subseq_bytes raw bytes (a
 * power of two, 16..1024), one lane each.  Every lane decodes its subsequence from a guessed state (block 0, DC next, at
 * its first bit); a lane decodes again whenever the exit state of the subsequence in front of it is not the state it
 * decoded from, until nothing changes - the fixed point is the serial decode, whether or not a guess was ever right; a
 * prefix sum of completed blocks places every subsequence; a last decode writes coefficients and DC differences, and a
 * prefix sum per component and interval makes the DC values.  Any Ri, 0 included: a marker is a known state inside its
 * subsequence.  A fixed number of launches; every loop is bounded by a count (rounds by subsequences in scope, a decode
 * by the symbols that 8 subseq_bytes + 31 bits hold, blocks by the interval's 6 MCUs).  Arguments, picture, status bits
 * and guarantees are those of vfml_jpeg_decode_rgb (status: the bit of the first error in stream order is set, others
 * may be); the whole scan is entropy-decoded whatever the rows, only the transform is windowed.
 * workspace: vfml_jpeg_decode_sync_workspace_bytes(h, w, scan_bytes, subseq_bytes) = that of vfml_jpeg_decode_rgb plus
 * 20 bytes per subsequence, each region rounded up to 256 (0: as there, or subseq_bytes no such power of two). */
int64_t vfml_jpeg_decode_sync_workspace_bytes(int h, int w, int64_t scan_bytes, int subseq_bytes);
int vfml_jpeg_decode_rgb_sync(const unsigned char* scan, int64_t scan_bytes, int h, int w, int restart_interval,
                              const unsigned char* qtables, const int32_t* tables, int y0, int y1, int subseq_bytes,
                              void* workspace, unsigned char* rgb, int64_t row_stride, int32_t* status, void* stream);

/* Both decoders for the other samplings a baseline file may have ("Samplings";
 * tests/jpeg_sampling_oracle.py is the definition).  Entropy decoding, IDCT and colour conversion are those above; the
 * sampling sets the MCU and the chroma filter:
 *   VFML_JPEG_420   2x2 / 1x1 / 1x1   MCU 16x16   Y00 Y01 Y10 Y11 Cb Cr   h2v2 triangle filter, as above
 *   VFML_JPEG_422   2x1 / 1x1 / 1x1   MCU 16x8    Y0 Y1 Cb Cr             libjpeg's h2v1 "fancy" filter per row:
 *                   out[2c] = (3 C[c] + C[c-1] + 1) >> 2, out[2c+1] = (3 C[c] + C[c+1] + 2) >> 2 (columns clamped); where
 *                   the chroma plane is at most 2 samples wide (w <= 4) every sample is repeated instead, as libjpeg does
 *   VFML_JPEG_444   1x1 / 1x1 / 1x1   MCU 8x8     Y Cb Cr                 no filter
 *   VFML_JPEG_GREY  one component, whatever factors its header names: a scan that is not interleaved (T.81 A.2.2), an
 *                   MCU is one block, ceil(h/8) x ceil(w/8) of them, Ri counts blocks; the picture is R = G = B = Y.
 *                   tables[0], tables[1] select its Huffman tables and qtables[0..63] is its table; the other entries
 *                   are not read
 * Chroma planes are ceil(h V / Vmax) x ceil(w H / Hmax).  Only 4:2:0 has a vertical filter: for the other samplings a row
 * window reads the intervals of its luma rows alone.  Every other argument, the status bits and the guarantees on a
 * damaged scan are those of vfml_jpeg_decode_rgb and vfml_jpeg_decode_rgb_sync, which are these with VFML_JPEG_420 and
 * give the bytes they always gave.  A sampling outside the enum returns non-zero (vfml_last_error) and launches nothing;
 * the workspace functions return 0 for it.  A workspace sized for one sampling does not fit another. */
enum { VFML_JPEG_420 = 0, VFML_JPEG_422 = 1, VFML_JPEG_444 = 2, VFML_JPEG_GREY = 3 };
int64_t vfml_jpeg_decode_sampled_workspace_bytes(int h, int w, int sampling, int64_t scan_bytes);
int vfml_jpeg_decode_rgb_sampled(const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                                 int restart_interval, const unsigned char* qtables, const int32_t* tables, int y0, int y1,
                                 void* workspace, unsigned char* rgb, int64_t row_stride, int32_t* status, void* stream);
int64_t vfml_jpeg_decode_sync_sampled_workspace_bytes(int h, int w, int sampling, int64_t scan_bytes, int subseq_bytes);
int vfml_jpeg_decode_rgb_sync_sampled(const unsigned char* scan, int64_t scan_bytes, int h, int w, int sampling,
                                      int restart_interval, const unsigned char* qtables, const int32_t* tables, int y0,
                                      int y1, int subseq_bytes, void* workspace, unsigned char* rgb, int64_t row_stride,
                                      int32_t* status, void* stream);

/* The encoder for the samplings a flow video wants ("Samplings";
 * tests/jpeg_encode_sampling_oracle.py is the definition and the scan equals its scan byte for byte).  Colour conversion,
 * DCT, quantisation, clamps, Huffman tables, stuffing, padding and restart markers are those of vfml_jpeg_encode_rgb; the
 * sampling sets the MCU, the chroma sample and the SOF0 / DRI bytes of the header (storage/jpeg_tables.py jpeg_header):
 *   VFML_JPEG_420   2x2 / 1x1 / 1x1   MCU 16x16   Y00 Y01 Y10 Y11 Cb Cr   chroma = (a + b + c + d + 2) >> 2 over 2x2 cells
 *   VFML_JPEG_422   2x1 / 1x1 / 1x1   MCU 16x8    Y0 Y1 Cb Cr             chroma = (a + b + 1) >> 1 over the horizontal pair
 *   VFML_JPEG_444   1x1 / 1x1 / 1x1   MCU 8x8     Y Cb Cr                 chroma = the sample itself
 * The picture is padded to multiples of the MCU by edge replication (4:2:2, 4:4:4: a height multiple of 8), one MCU row
 * is one restart interval, and the DC predictors are per component and zero at the start of each interval.  Every other
 * argument and every guarantee is that of vfml_jpeg_encode_rgb, which is this with VFML_JPEG_420 and writes the bytes it
 * always wrote: nothing is written at or past scan + scan_capacity, *scan_bytes holds the length the picture needs, every
 * workspace region is sized for the worst case of this sampling (416 bytes per block, MCUs per row x blocks per MCU x
 * 416 + 2 per interval), and the worst-case scan stays below 4 GiB (0 from the size functions otherwise).
 * VFML_JPEG_GREY and a sampling outside the enum return non-zero (vfml_last_error) and launch nothing; the size functions
 * return 0 for them.  A workspace sized for one sampling does not fit another. */
int64_t vfml_jpeg_sampled_workspace_bytes(int h, int w, int sampling);
int64_t vfml_jpeg_sampled_scan_capacity(int h, int w, int sampling);
int vfml_jpeg_encode_rgb_sampled(const unsigned char* rgb, int h, int w, int64_t row_stride, int sampling,
                                 const unsigned char* qtables, void* workspace, unsigned char* scan,
                                 int64_t scan_capacity, uint32_t* scan_bytes, void* stream);

/* Deflate / inflate of the flow cache's .npz members (tests/deflate_oracle.py is the definition of
 * the stream, vfml/csrc/deflate_code.h of its code lengths).  The raw bytes are cut into chunks of chunk_bytes (a power of
 * two, 1024..32768); a chunk becomes one dynamic-Huffman block of literals and the end-of-block symbol - or one stored
 * block when that is not larger - and every chunk but the last is followed by an empty stored block (00 00 FF FF after
 * padding), so that every chunk starts on a byte boundary; the last block carries BFINAL.  Any inflater reads the result;
 * with the chunks' offsets it is decoded in parallel.  All integer, all on `stream`, no host synchronisation, no
 * allocation.
 * raw: device, any alignment (a slice of a larger buffer is coded in place).  workspace: device, 256-byte aligned,
 * vfml_deflate_workspace_bytes / vfml_inflate_workspace_bytes; not shared by calls that may run at once.
 * out: receives the stream, any alignment; vfml_deflate_capacity(raw_bytes, chunk_bytes) bytes always suffice; with a
 * smaller capacity nothing is written at or past out + capacity and *stream_bytes still holds the length the stream
 * needs.  offsets: device uint32[ceil(raw_bytes / chunk_bytes)], the byte offset of every chunk in the stream;
 * *stream_bytes, *crc: device, 4-byte aligned.  *crc = CRC-32 (the zip polynomial) of the raw bytes continued from
 * crc_init (the CRC of whatever the caller puts in front, 0 for nothing): chunk 0 continues crc_init, the others start
 * from 0, and the values are folded on the device with multiplications by x^(8 len).
 * 1 <= raw_bytes < 2 GiB and at most 16000 chunks (what a zip extra field can index); the size functions return 0
 * otherwise. */
int64_t vfml_deflate_capacity(int64_t raw_bytes, int chunk_bytes);
int64_t vfml_deflate_workspace_bytes(int64_t raw_bytes, int chunk_bytes);
int vfml_deflate_huffman(const unsigned char* raw, int64_t raw_bytes, int chunk_bytes, uint32_t crc_init, void* workspace,
                         unsigned char* out, int64_t capacity, uint32_t* offsets, uint32_t* stream_bytes, uint32_t* crc,
                         void* stream);

/* The inflater: a wave per chunk, chunk i = data[offsets[i] .. offsets[i+1]) (the last one ends at data_bytes) and
 * decodes to raw[i * chunk_bytes ..), min(chunk_bytes, what is left of raw_bytes) bytes.  A chunk is any sequence of
 * dynamic, fixed and stored blocks of literals that ends with BFINAL or with the chunk's bytes; n_chunks =
 * ceil(raw_bytes / chunk_bytes).  *crc as above.  *status (device, 4-byte aligned) receives 0 or the OR of
 * VFML_INFLATE_ERR_*: damaged data is a defined result - every index is checked on the device, nothing outside `data` is
 * read and nothing outside `raw` written, whose content (and *crc) is then unspecified. */
enum {
  VFML_INFLATE_ERR_CODE = 1,     /* bits that are no code of the block's table, or a block header that describes none */
  VFML_INFLATE_ERR_MATCH = 2,    /* a length / distance symbol: this codec has literals only                           */
  VFML_INFLATE_ERR_LENGTH = 4,   /* a chunk that decodes to another length than its share of raw_bytes                  */
  VFML_INFLATE_ERR_BITS = 8,     /* a chunk's bits ran out inside a block                                               */
  VFML_INFLATE_ERR_STORED = 16,  /* a stored block whose LEN and NLEN do not agree                                      */
  VFML_INFLATE_ERR_CHUNK = 32    /* offsets that are not ascending inside data_bytes, or a chunk whose compressed form is
                                    longer than 9/8 chunk_bytes + 64 bytes (more than fixed codes need)                 */
};
int64_t vfml_inflate_workspace_bytes(int64_t raw_bytes, int chunk_bytes);
int vfml_inflate_chunks(const unsigned char* data, int64_t data_bytes, const uint32_t* offsets, int n_chunks, int chunk_bytes,
                        int64_t raw_bytes, uint32_t crc_init, void* workspace, unsigned char* raw, uint32_t* crc,
                        int32_t* status, void* stream);

/* Scene-cut statistic of uint8 RGB frames (tests/scene_cut_oracle.py is the definition).
 * frames: device, [n][H][W][3] contiguous, any alignment (a frame inside a clip).  Per frame t the signature
 * sig_out[t][16][64] counts the pixels per cell c = (y * 4 / H) * 4 + (x * 4 / W) and per bin Y >> 2 of the luma
 * Y = (77 R + 150 G + 29 B + 128) >> 8; dist_out[t] = sum |sig[t] - sig[t-1]| over the 1024 counts (at most 2 H W).
 * Frame 0 is measured against prev_sig (device, uint32[1024], the signature of the frame before this call's first) or
 * gets 0 when prev_sig is null.  sig_out, dist_out, prev_sig: device, 4-byte aligned; prev_sig may be a row of an earlier
 * call's sig_out but not of this one's.  All integer, all on `stream` (a memset and two launches), no host
 * synchronisation, no allocation, the same bytes on every run.  Null frames / sig_out / dist_out, n outside 1..65535, an
 * empty frame and H * W >= 2^31 return non-zero (vfml_last_error) before anything is launched. */
int vfml_scene_distances(const unsigned char* frames, int n, int H, int W, const uint32_t* prev_sig, uint32_t* sig_out,
                         uint32_t* dist_out, void* stream);

const char* vfml_last_error(void);
int vfml_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
