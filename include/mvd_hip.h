/* mvd_hip.h -- C ABI of the MI355X-native (gfx950) MVD-Fusion denoising hot path.
 *
 * The reference (zhizdev/mvdfusion) is pure Python/PyTorch and has no FFI of its own; this ABI is the new
 * boundary *below* the reference's config-driven classes.  Each entry point replaces a
 * cluster of torch ops on the per-DDIM-step path; the reference site is cited next to it (paths relative to the
 * reference root).  The Python mirror classes in mvdfusion_amd/ (GridAttn, UNetModel, ViewFusion, DDIMSampler)
 * bind these symbols with ctypes -- see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr()); the library never
 *     allocates, frees or retains memory beyond a call;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t); no host synchronisation => calls are capturable
 *     in a hipGraph (mvd_graph_*);
 *   - return 0 on success, <0 on error; the message is available from mvd_last_error(); nothing throws;
 *   - activations are fp32, channels-last: an image tensor is (B, H, W, C) == a row-major (B*H*W, C) matrix;
 *   - GEMM-shaped math runs on 16-bit MFMA (fp16 by default, bf16 in the -DMVD_OPERAND_BF16 build; same rate).
 *     `prec` selects MVD_PREC_X1 (= one product per operand pair) or MVD_PREC_X3 (= operands split
 *     x = hi + lo, three products hi*hi + hi*lo + lo*hi, fp32 accumulate: ~2^-22 (fp16) / ~2^-17 (bf16) relative
 *     operand error; the 50-step stochastic trajectory amplifies operand error by ~10^3, so the split is what keeps it
 *     within the 1e-3 latent-RMSE budget).
 *   - Operand range (fp16 flavour): every GEMM / attention operand is stored as x ~= hi + lo in fp16.  For
 *     6e-5 <= |x| < 65504 the relative operand error is <= 2^-22; below that the ABSOLUTE resolution is 2^-25 (fp16
 *     subnormals), i.e. a tensor whose values are all << 1e-3 loses relative precision; |x| >= 65504 overflows to inf and
 *     the outputs become non-finite (no silent saturation).  Weights are pre-scaled by a power of two at pack time
 *     (mvd_pack_*, undone exactly through acc_scale) so they always sit in the normal range.  The host mirrors check the
 *     final latents / images once per sample (mvdfusion_amd/hip.py: check_finite) and raise FloatingPointError; the bf16
 *     flavour (libmvd_hip_bf16.so, precision "bf16x3") has fp32's exponent range at ~2^-16 relative operand error.
 *     The per-element bars that follow from this contract (operand error, fp32 roundings of the k loop, the absolute floor), their
 *     derivation and the measurements against float64: tests/gemm_f64.py, tests/test_gpu_gemm_f64.py (CPU proof: tests/test_cpu_gemm_f64.py).
 *   - one host thread per process / GPU (matches the reference's mp.spawn model, demo.py:208).
 */
#ifndef MVD_HIP_H
#define MVD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* mvd_stream_t; /* hipStream_t */

#define MVD_VERSION 100
#define MVD_PREC_X1 1   /* one product per operand pair (hi only) */
#define MVD_PREC_X3 3 /* hi*hi + hi*lo + lo*hi */
#define MVD_PREC_X4 4     /* all four partial products of the (hi+lo)(hi+lo) split: fp32-class products */

int mvd_version(void);
const char* mvd_last_error(void);
/* MFMA operand element type this library was built for: 0xf16 (fp16, default) or 0xbf16 (-DMVD_OPERAND_BF16).
 * Every "split planes" / packed-weight buffer holds that type; the two flavours are separate .so files. */
int mvd_operand_format(void);

/* ------------------------------------------------------------------------------------------------
 * Weight packing (once per model load).  Packed image: [K/32][N/16][hi image | lo image] (2 KiB micro-tiles of 16 n x 32 k); an
 * image (1 KiB) is the 16x16x32 MFMA B fragment as a wave holds it: lane l = (n & 15) + 16 * ((k & 31) >> 3) owns the 8 elements
 * k & 7 = 0..7 at byte 16 l -- a granule of the LDS-DMA is one contiguous KiB and the fragment read from LDS is lane-contiguous.
 * K padded to 32, N padded to 16 with zeros.  Bytes = mvd_packed_weight_bytes(N, K).
 * (tests/gemm_f64.py: packed_index / decode_packed decode an image from this text alone; tests/test_gpu_gemm_f64.py holds the packers to it.)
 * Replaces nothing in the reference (its weights stay fp32 nn.Parameters); the Python mirrors keep the
 * fp32 parameters under the reference's state_dict keys and pack on first use. */
size_t mvd_packed_weight_bytes(int N, int K);
/* w: (N, K) row-major fp32 with leading dimension ldw.  geglu != 0 interleaves value/gate row blocks of 16
 * (rows [0,N/2) = value, [N/2,N) = gate, attention.py:43-44) so a GEMM tile holds matching value/gate columns. */
/* scale: power of two applied to the weights before the split (keeps the low part out of fp16's subnormal range);
 * the GEMM undoes it exactly through mvd_gemm_desc.acc_scale = 1/scale. */
int mvd_pack_linear_weight(const float* w, int N, int K, int ldw, int geglu, float scale, void* packed,
                           mvd_stream_t stream);
/* The same image from the TRANSPOSED source: wt is (K, N) row-major with leading dimension ldw, the packed weight is its transpose
 * (N, K) -- the dgrad weight W^T of a Linear packed straight from the parameter, without a transposed copy. */
int mvd_pack_linear_weight_t(const float* wt, int N, int K, int ldw, float scale, void* packed, mvd_stream_t stream);
/* w: (Cout, Cin, 3, 3) fp32 (nn.Conv2d layout).  Packed K index = ((ci/32)*9 + ky*3+kx)*32 + ci%32: the nine taps of one
 * 32-channel block are consecutive k-tiles, so the implicit-GEMM kernel re-reads a pixel's 128-byte line back to back. */
int mvd_pack_conv3x3_weight(const float* w, int Cout, int Cin, int cin_pad, float scale, void* packed,
                            mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM convolution with fused epilogue.
 *   nn.Linear                      external/sd1/ldm/modules/attention.py:161-168, 41, 60; mvdfusion/attention.py:100,114;
 *                                  view_attn_efficient2.py:52-61,83,158,167 (timm Attention/Mlp linears)
 *   nn.Conv2d 1x1                  attention.py:245,259; openaimodel.py:241
 *   nn.Conv2d 3x3 (s1, s2, after nearest-2x upsample)   openaimodel.py:107,116,151,204,229-231; unet.py:323,499 */
#define MVD_A_DENSE 0   /* A: (M, K) row-major planes, leading dim lda (elements) */
#define MVD_A_CONV3X3 1 /* A: NHWC (B, Hin, Win, Cin) planes, pad 1; M = B*Hout*Wout, K = 9*Cin */
/* Conv geometry (Hin / Win / Hout / Wout, stride, upsample, no_pad_tl, the centre-tap tail and the four-tap form below): stated as an explicit
 * gather over (b, oy, ox, ky, kx) in tests/gemm_f64.py (conv_taps, up4_taps) and pinned bit for bit, at non-square and odd sizes, by the
 * `geometry` fixture of tests/test_gpu_gemm_f64.py. */

#define MVD_EPI_STORE 0 /* out[m,n] = res[m,n] + colscale[n] * act(acc + bias[n] + bias_b[m / rows_per_batch, n]) */
#define MVD_EPI_GEGLU 1 /* out[m,j] = (acc_v + bias[j]) * gelu(acc_g + bias[N/2 + j]);  out has N/2 columns */
#define MVD_EPI_QKV 2   /* route N = 3*heads*dhead columns to the attention operand planes (see mvd_attention) */

#define MVD_ACT_NONE 0
#define MVD_ACT_GELU 1 /* exact erf GELU (nn.GELU(), F.gelu) */
#define MVD_ACT_SILU 2
#define MVD_ACT_QUICKGELU 3 /* x * sigmoid(1.702 x): the MLP activation of OpenAI CLIP's vision transformer */

#define MVD_GEMM_TILES 5 /* tile shapes of mvd_gemm_desc.cfg */
#define MVD_GEMM_LOOPS 8 /* k-loop variants of mvd_gemm_desc.cfg (0 ... 7; 3 removed) */
#define MVD_GEMM_CFG_STRIDE 32 /* cfg = 1 + MVD_GEMM_CFG_STRIDE * tile + 2 * loop + order */
#define MVD_B_PACKED 0   /* B: weight image of mvd_pack_linear_weight / mvd_pack_conv3x3_weight */
#define MVD_B_PLANES 1   /* B: (N, ldb) row-major split planes (an activation), N % 16 == 0 */

/* one weight (or any read-only operand) a later launch of the step will read: mvd_gemm_desc.pf_items */
typedef struct mvd_prefetch_item_s {
  const void* ptr;
  unsigned long long bytes;
  int start_after;      /* host bookkeeping (launch index of the host kernel); not read by the device */
  int consumer;         /* host bookkeeping (launch index of the consumer); not read by the device */
} mvd_prefetch_item;

typedef struct mvd_gemm_desc {
  int M, N, K;      /* logical sizes; N % 16 == 0 after padding of the packed weight, K as packed (multiple of 32) */
  /* A operand: activations in the SPLIT-PLANES format, produced by the previous kernel (mvd_groupnorm_nhwc,
   * mvd_layernorm, mvd_attention, a GEMM epilogue, mvd_split_planes ...):  x ~= hi + lo as bf16; a (rows, lda) matrix
   * is stored per row as lda/32 blocks of [32 x hi | 32 x lo] (128 contiguous bytes per row and 32-element k-block,
   * the unit the kernel's LDS-DMA moves).  Same bytes as fp32.  128-byte aligned. */
  const void* A;
  int lda;          /* elements per row; multiple of 32 */
  int a_mode;       /* MVD_A_* */
  /* conv geometry (a_mode == MVD_A_CONV3X3) */
  int B, Hin, Win, Cin, Hout, Wout, stride, upsample; /* upsample: input is nearest-2x upsampled before the conv */
  int no_pad_tl;         /* 1: no zero padding on the top / left edge, i.e. F.pad(x, (0,1,0,1)) + conv(stride 2, padding 0) of
                            the VAE Downsample (diffusionmodules/model.py:72-76); taps past the bottom / right edge read zeros */
  const void* Wp;   /* B operand: packed weight (mvd_pack_*), or -- b_mode == MVD_B_PLANES -- an (N, ldb) activation matrix in split
                       planes, i.e. out = A B^T of two activation tensors (the VAE mid-block attention: Q K^T and P V,
                       external/sd1/ldm/modules/diffusionmodules/model.py:184-199) */
  int b_mode;       /* MVD_B_* */
  int ldb;          /* elements per row of a planes B operand; multiple of 32 */
  float acc_scale;  /* accumulator scale = 1 / (pack scale); 0 is treated as 1 */
  int prec;         /* MVD_PREC_* */
  /* epilogue */
  int epi;          /* MVD_EPI_* */
  int act;          /* MVD_ACT_* */
  float* out;       /* fp32 output or NULL */
  int ldo;
  void* out_sp;     /* optional split-planes output (feeds the next GEMM's A operand) */
  int ldp;          /* elements per row of out_sp; multiple of 32 */
  int n_store;      /* columns actually stored (<= N; lets N be padded to 16, e.g. the 5-channel UNet head) */
  const float* bias;     /* [N] or NULL */
  const float* bias_b;   /* [M / rows_per_batch][ldbb] or NULL (per-view vector, e.g. the kv_len==1 cross-attention) */
  int rows_per_batch;
  int ldbb;              /* row stride of bias_b in floats (multiple of 4); 0 = N */
  const float* colscale; /* [N] or NULL (adaLN gate) */
  const float* res;      /* [M][ldr] or NULL */
  int ldr;
  /* MVD_EPI_QKV */
  void *q_hi, *q_lo, *k_hi, *k_lo, *vt_hi, *vt_lo;
  int heads, dhead, L, Lpad; /* rows m = b*L + token.  heads*dhead % 32 == 0 (the epilogue routes 32-column blocks, each inside one of
                                q / k / v), dhead % 4 == 0, L % 4 == 0: anything else is refused */
  float qscale;              /* dhead^-0.5 * log2(e), applied to q in fp32 before the split: mvd_attention computes its
                                softmax with exp2 on the raw q.k products */
  /* split-K: 1 = none; >1 = that many K slices; 0 = choose automatically (fills the 256 CUs when the tile grid
   * is small or divides badly over them -- a small time model, gemm.hip: choose_splits).  Partial fp32 slabs
   * (splitk*M*N) go to `workspace`; a second kernel sums them in slice order 0..splitk-1 and applies the
   * epilogue; without a workspace (or when it is too small: workspace_elems) the GEMM runs unsplit. */
  int splitk;
  float* workspace;
  size_t workspace_elems;
  /* kernel configuration: 0 = built-in heuristic; otherwise cfg = 1 + MVD_GEMM_CFG_STRIDE * tile + 2 * loop + order with
   *   tile : 0 = 64x64 (4 waves)  1 = 128x128 (8 waves)  2 = 128x80 (4 waves)  3 = 64x80 (4 waves)  4 = 128x160 (8 waves);
   *          tiles >= 2 (the 80-column family for N = 320 * k: no N padding, 256 workgroups at M = 8192, N = 320) serve
   *          MVD_EPI_STORE only (the GEGLU / QKV epilogues walk a wave tile in 32-column blocks)
   *   loop : 0 = plain two-buffer loop, 1 = register-pipelined loop (two k-tiles in LDS, MFMA fragments double-buffered in
   *          registers), 2 = staggered (8-wave tiles only: three k-tiles in LDS, the two wavefronts of a SIMD half an
   *          iteration apart, so one issues LDS-DMA / fragment reads while the other runs MFMAs), 4 = the register-pipelined loop over a ring of up to 4 k-tiles in LDS, 5 = over a
   *          ring of up to 8 (4-wave tiles): one workgroup per CU keeps 3 / 7 k-tiles of operands in flight, for the small grids
   *          of the low-resolution levels whose k-loop is otherwise one DMA round trip per k-tile, 6 = the input-patch kernel for
   *          stride-1 padded 3x3 convolutions (tiles 1, 2, 4): the tile's pixels + halo are staged once per 32-channel block and the
   *          nine taps read shifted slots of that patch (4-6x less A traffic into LDS), 7 = the wave-specialised kernel (tiles 1, 2,
   *          4; tile 1 with every epilogue, 2 and 4 MVD_EPI_STORE): four consumer wavefronts (fragment reads + MFMAs) and four loader wavefronts (all LDS-DMAs) per
   *          workgroup;
   *          3 = removed (a four-buffer staggered loop, round 3: never the fastest on any shape; the register-staged deliveries 8 / 9 and
   *          the persistent role-split kernel 10 of rounds 4 / 5 went the same way -- tools/probes/gemm_pt.hip keeps the latter);
   *          mvd_gemm rejects it, and mvd_gemm_cfg_supported() tells whether a cfg serves a problem
   *   order: 0 = n-fastest, 1 = m-fastest order of the output tiles over the 8 XCDs.
   * The host mirror times the candidates once per distinct problem shape during the eager warm-up step and passes the
   * winner from then on (mvdfusion_amd/hip.py: autotune). */
  int cfg;
  /* GroupNorm statistics of the OUTPUT, emitted by the producer instead of a separate statistics kernel (MVD_EPI_STORE, n_store == N
   * <= 2560, M % 16 == 0): gn_stats = [M / gn_hw images][gn_groups][2] int64, zeroed by the caller, receives {sum, sum of squares}
   * of every (image, group) as 2^24 fixed point (integer atomics: deterministic); consumed by mvd_groupnorm_from_stats.  gn_hw =
   * rows per image (multiple of 16).  NULL = off. */
  long long* gn_stats;
  int gn_hw, gn_groups;
  /* Row statistics of the OUTPUT for a LayerNorm that is folded into the CONSUMER GEMM (MVD_EPI_STORE, n_store == N): rs_out =
   * [M][rs_ld] pairs of floats {sum, sum of squares} of the stored values of row m over one column slot (a wave tile of the kernel
   * that ran, or a 256-column span of the split-K reduce); the number of slots written per row goes to rs_count[0] (device int).
   * rs_ld >= N / 32 (the narrowest wave tile).  No atomics: the consumer adds the slots in order.  NULL = off.
   * Precision: a slot is a plain fp32 {sum x, sum x^2} over <= 256 columns and the consumer forms var = E[x^2] - mean^2 in double, so the
   * relative error of the variance is ~1e-7 mean^2 / var -- the kappa term of the conditioning contract at mvd_groupnorm_nhwc below:
   * validated for rows with |mean| / std <= 3 (tests/test_gpu_ops.py::test_gemm_layernorm_fold, 2e-6) and at 8 std against float64
   * (tests/test_gpu_norm_f64.py::test_layernorm_folded_into_the_gemm); residual streams with outlier channels (|mean| / std in the
   * hundreds) should use mvd_layernorm (two-pass) -- the host mirror's switch is Ctx.ln_fold. */
  float* rs_out;
  int* rs_count;
  int rs_ld;
  /* LayerNorm folded into THIS GEMM (MVD_EPI_QKV / MVD_EPI_GEGLU): A holds the raw rows x (the producer's split planes), the packed
   * weight is W' = W * diag(gamma), and the epilogue forms  rstd_m (x_m . W'_n - mean_m ln_colsum[n]) + bias[n]  with
   * ln_colsum[n] = sum_k W'[n][k] (logical column order, like bias), bias[n] = sum_k beta[k] W[n][k] (+ the layer's own bias),
   * mean / rstd of row m over its ln_dim real columns from the producer's ln_stats = rs_out, ln_count = rs_count, ln_ld = rs_ld,
   * eps = ln_eps.  Exact algebra: LayerNorm is affine per row -- exact in arithmetic only as far as the MFMA operands carry W' and x:
   * use it with the fp16 hi + lo modes (MVD_PREC_X3 / X4 of the f16 library); with one product or bf16 operands the uncancelled
   * mean * sum(W~' - W') term grows with |mean| / std (the host mirror runs mvd_layernorm there).  Runs without split-K.  NULL = off. */
  const float* ln_stats;
  const int* ln_count;
  const float* ln_colsum;
  int ln_ld, ln_dim;
  float ln_eps;
  /* GroupNorm APPLY of the output behind the GEMM (openaimodel.py:201-204: GroupNorm32 -> SiLU -> conv of the next layer; needs gn_stats /
   * gn_hw / gn_groups, MVD_EPI_STORE, out != NULL): after the call gna_out_sp (M, N split planes) holds act(GroupNorm(out) * gamma + beta),
   * gna_flags bit 0 = SiLU, bit 1 = round the normalised value to fp16 first (as mvd_groupnorm_from_stats' `silu`), bit 2 = `out` itself
   * has no other reader: the fused path may leave it unwritten.  How: a split-K GEMM whose (image, group) slab of gn_hw x N / gn_groups
   * values fits 64 KB of LDS runs ONE reduce kernel -- a workgroup per (image, group) sums the slabs, applies the epilogue, keeps the values
   * in LDS, forms mean / rstd and writes the normalised planes: the separate reduce and apply launches and the fp32 round trip between them
   * disappear; otherwise the library launches mvd_groupnorm_from_stats behind the GEMM / the reduce.  NULL = off. */
  void* gna_out_sp;
  const float* gna_gamma;
  const float* gna_beta;
  float gna_eps;
  int gna_flags;
  /* ... over a CONCATENATION (unet.py:550: h = torch.cat([h, hs.pop()], 1) feeding the next ResBlock): with cat_b = the (M, cat_cb) fp32
   * skip tensor the GroupNorm of gna_* runs over [out | cat_b] (N + cat_cb channels; gn_stats / gna_out_sp / gamma / beta refer to the
   * concatenation), and cat_raw_sp (optional) receives the split planes of [out | cat_b] itself (operand of the ResBlock's 1x1 skip
   * convolution).  Split GEMM: the one reduce kernel reads the skip tensor next to the slabs; else mvd_concat_groupnorm runs behind the
   * GEMM.  Shapes: mvd_concat_groupnorm_fits(N, cat_cb, gn_hw, gn_groups).  NULL = off. */
  const float* cat_b;
  int cat_cb;
  void* cat_raw_sp;
  /* Optional DEVICE scalar multiplied into acc_scale (NULL = 1): the backward GEMMs undo the power-of-two scale of their gradient operand
   * (mvd_pow2_scale) with it, without the host ever reading the scale. */
  const float* acc_scale_dev;
  /* In-kernel weight prefetch (hosts: gemm_ws_kernel, cfg loop 7, and the fused reduce + GroupNorm kernel of a split GEMM with gna_out_sp;
   * ignored by every other kernel): pf_n entries of a device table of weights
   * that LATER launches of the step will read (mvd_prefetch_item: ptr, bytes; the other fields unused).  The launch's consumer wavefronts
   * request every 128-byte line of them once at kernel start and drop the data.  Why: a denoising step streams its whole weight set (3.4 GB of
   * packed operands at model_channels 320) through a 256 MB Infinity Cache once per step, so every GEMM meets its weights cold and its short
   * k-loop is a chain of HBM round trips (2 - 7 us per launch of the small and medium GEMMs, profiles/r05_prefetch_probe_whole_weight.log); the
   * role-split convolutions have idle consumer wavefronts and idle HBM bandwidth to spend on the launches behind them.  NULL = off. */
  const struct mvd_prefetch_item_s* pf_items;
  int pf_n;
  /* Tap schedule of a convolution (a_mode == MVD_A_CONV3X3): which (operand, 32-channel block, tap) each k-tile reads.
   *   MVD_TAPS_FULL        every channel block of A at all nine taps: K = 9 * Cin (the default).
   *   MVD_TAPS_CENTRE_TAIL the nine taps of A's Cin / 32 blocks, then Cin2 / 32 blocks of a SECOND operand A2 (split planes, (M, lda2),
   *                        lda2 >= Cin2, multiples of 32) at the centre tap only: K = 9 * Cin + Cin2 and
   *                          out = conv3x3(A, W[:, :9 Cin]) + A2 W[:, 9 Cin:]^T
   *                        in one launch -- a ResBlock's conv2 and its 1x1 skip convolution (openaimodel.py:241,274) without the skip's own
   *                        GEMM, its fp32 output and the residual read.  The packed weight is the k-tile concatenation of the conv image
   *                        and the linear image (same N padding and pack scale).  Stride 1, padded, no upsample, Hin == Hout, Win == Wout;
   *                        served by every cfg except the input-patch kernel (loop 6).
   *   MVD_TAPS_UP4         the four-tap form of a convolution behind a nearest-2x upsample (upsample == 1, stride 1, packed weight): the
   *                        3x3 window of output pixel (2i + a, 2j + c) covers a 2x2 block of low-resolution pixels, rows i - 1 + a + dy and
   *                        columns j - 1 + c + dx (dy, dx = 0, 1), so each of the four output parities (a, c) is a 2x2 convolution of the
   *                        LOW-resolution image with its own weight, the 3x3 taps that land on one pixel summed at pack time (row weights
   *                        a = 0: w[0], w[1] + w[2]; a = 1: w[0] + w[1], w[2]; columns alike): K = 4 * Cin, 4/9 of the multiply-accumulates.
   *                        Wp = the four parity images (index 2a + c) one after the other, each [K / 32][N / 16] micro-tiles with k-tile
   *                        order (32-channel block, tap dy * 2 + dx), all at one pack scale.  The launch walks its M rows as (parity,
   *                        image, i, j) -- B * Hin * Win rows per parity, a block tile lies inside one parity -- and stores row (b, 2i + a,
   *                        2j + c) of the ordinary (B, Hout, Wout, N) output / split-K slab, so everything behind the tile epilogue (split-K
   *                        reduces, GroupNorm apply, concat) is unchanged.  MVD_EPI_STORE with bias, act, out, out_sp, n_store, split-K,
   *                        gn_stats (then Hin * Win % 16 == 0), gna_out_sp and cat_b; REFUSED: res, bias_b, colscale, rs_out, the GEGLU /
   *                        QKV epilogues, no_pad_tl.  Served by every cfg except the input-patch kernel (loop 6). */
  int tap_mode;
  const void* A2;
  int lda2, Cin2;
} mvd_gemm_desc;
#define MVD_TAPS_FULL 0
#define MVD_TAPS_UP4 1
#define MVD_TAPS_CENTRE_TAIL 2
#define MVD_GNA_SILU 1
#define MVD_GNA_ROUND_F16 2
#define MVD_GNA_OUT_UNUSED 4

int mvd_gemm(const mvd_gemm_desc* d, mvd_stream_t stream);
/* 1 if kernel configuration `cfg` (see mvd_gemm_desc.cfg) serves the problem `d` describes (tile family vs epilogue, loop variant vs
 * tile, the input-patch kernel vs the convolution's geometry), else 0.  The host autotuner enumerates with it. */
int mvd_gemm_cfg_supported(const mvd_gemm_desc* d, int cfg);

/* fp32 (rows, cols) matrix with leading dim ldx -> split planes (rows, ldp), ldp % 32 == 0; columns [cols, ldp) are 0.
 * Used where a GEMM consumes a tensor that only exists in fp32 (residual stream into the 1x1 skip / up / down convs). */
int mvd_split_planes(const float* x, void* sp, size_t rows, int cols, int ldx, int ldp, mvd_stream_t stream);
/* ... of x * (*scale_dev): the power-of-two gradient scale of mvd_pow2_scale applied on the way into the planes (scale_dev NULL = 1). */
int mvd_split_planes_scaled(const float* x, void* sp, size_t rows, int cols, int ldx, int ldp, const float* scale_dev, mvd_stream_t stream);

/* fp32 matrix-vector products for the M<=16 cases (exact fp32 FMA):
 *   y[m, n] = act_out( sum_k W[n,k] * act_in(x[m,k]) + bias[n] ),  W (N,K) row-major fp32.
 * time_embed / emb_layers / adaLN / cc_projection / kv_len==1 cross-attention vectors:
 *   unet.py:309-314,537-538; openaimodel.py:218-224,264; view_attn_efficient2.py:58-61,64;
 *   viewfusion_zero_depth_rgb.py:110,126-132,276-279,322; attention.py:221 (context length 1). */
int mvd_gemv(const float* W, const float* bias, const float* x, float* y, int M, int N, int K, int ldx, int ldy,
             int act_in, int act_out, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation.
 * GroupNorm(32 groups) on channels-last data; `silu` bit 0 = fused SiLU, bit 1 = round the normalised value to fp16 first
 * (the VAE decoder tail, diffusionmodules/model.py:564-570) (openaimodel.py:201-203,225-227 eps 1e-5;
 * attention.py:76,243,274 and mvdfusion/attention.py:92,132 eps 1e-6; unet.py:496-498).
 * ws: B * chunks * groups * 2 doubles with chunks = mvd_groupnorm_chunks(HW); ws_elems = its capacity in doubles (checked).
 *
 * Conditioning contract (the counterpart of the operand range contract above; bars and measurements: tests/norm_f64.py,
 * tests/test_gpu_norm_f64.py).  Every FORWARD GroupNorm path -- mvd_groupnorm_nhwc, mvd_groupnorm_from_stats behind
 * mvd_gemm_desc.gn_stats / mvd_concat_channels, mvd_gemm_desc.gna_out_sp, mvd_concat_groupnorm -- and the LayerNorm folded into a
 * GEMM (mvd_gemm_desc.ln_stats) form  var = E[x^2] - mean^2  from fp32 partial sums in one pass.  With
 *     kappa = (mean^2 + var) / (var + eps)      per (image, group) or row
 * each x^2 carries a rounding of 2^-24, so E[x^2] is off by up to 2^-24 (mean^2 + var), var + eps by 2^-24 kappa relative and rstd
 * by half of that; the fp32 mean in the folded shift beta - mean * rstd * gamma adds 2^-24 sqrt(kappa).  Per (image, group):
 *     |y - GroupNorm(x)| <= (3e-6 + 2^-24 * c * kappa) * max|y|       (+ the split-plane representation of y)
 * with c = 1 while no thread adds more than 16 terms in fp32 (the 8-rows-per-workgroup geometry of mvd_groupnorm_chunks; a float32
 * emulation of the kernel's summation order stays below half of this: tests/test_cpu_norm_f64.py).  Longer fp32 chains pay for their
 * length R with c = (R + 1) / 2: a prime HW leaves ONE chunk (R = HW / TY with the TY = 1 ... 4 row slices of gn_stats_kernel), the
 * 16-row slab producers add the group's C / groups columns in order (R = C / groups + 6), the GEMM tile epilogue its wave tile's
 * rows first (R <= 64 + C / groups).
 * kappa is ~1 for activations with |mean| <= sigma, 65 at |mean| = 8 sigma (c = 1: 4e-6) and 4097 at 64 sigma (2.4e-4): a tensor
 * whose groups sit many sigma off zero loses that much, silently.
 * Statistics slot (gn_stats): {sum, sum of squares} * 2^24 in 64-bit integers.  Capacity 2^63 / 2^24 = 5.5e11 for either total, i.e.
 * HW * (C / groups) * mean(x^2) < 5.5e11 (a 1024 x 40 group: rms |x| < 3.6e3; the `big` fixture of tests/norm_f64.py sits at a fifth
 * of it: tests/test_cpu_norm_f64.py::test_fixture_conditions).  Resolution 2^-25 of the sum, 2^-25 / n of the mean: y moves by
 * 2^-25 / n * rstd * gamma, which only shows for a group of a handful of elements without variance.
 * NOT subject to kappa: mvd_groupnorm_backward takes its moments in fp64 per element (gn_moments_kernel) and mvd_layernorm /
 * mvd_layernorm_backward take the variance in a second pass over (x - mean); only the mean rounded to fp32 enters:
 *     error <= (project bar + 2^-23 sqrt(kappa)) * max|result| of the group / row. */
int mvd_groupnorm_chunks(int HW);
/* y_sp: the normalised activations in split-planes format (B*HW, C), C % 32 == 0 -- GroupNorm only feeds GEMMs / convs. */
int mvd_groupnorm_nhwc(const float* x, void* y_sp, const float* gamma, const float* beta, int B, int HW, int C,
                       int groups, float eps, int silu, double* ws, size_t ws_elems, mvd_stream_t stream);
/* GroupNorm whose statistics were emitted by the producer of x (mvd_gemm_desc.gn_stats, mvd_concat_channels): one launch
 * (finalise mean / rstd per (image, group) from the fixed-point sums, apply, optional SiLU, write split planes). */
int mvd_groupnorm_from_stats(const float* x, void* y_sp, const float* gamma, const float* beta, const long long* stats, int B, int HW,
                             int C, int groups, float eps, int silu, mvd_stream_t stream);
/* Row softmax: y[r, :] = out_scale * softmax(scale * x[r, :]) of an fp32 (rows, cols) matrix (row stride ldx), written as
 * split planes (rows, cols), cols % 32 == 0, cols <= 4096.  out_scale (a power of two, e.g. 1024) lifts the probabilities of
 * wide rows out of the fp16 subnormal range; the consumer GEMM divides it out through its weight's acc_scale.  Replaces
 * F.softmax in the VAE AttnBlock (external/sd1/ldm/modules/diffusionmodules/model.py:191-193), whose single 512-wide head is
 * run as two GEMMs. */
int mvd_softmax_rows(const float* x, void* y_sp, int rows, int cols, int ldx, float scale, float out_scale,
                     mvd_stream_t stream);

/* LayerNorm over the last dim.  w/b may be NULL (no affine).  w_plus_one: y = norm * (1 + w) + b
 * (adaLN "modulate", view_attn_efficient2.py:15-16,51,53,65-66); attention.py:211-213, mvdfusion/attention.py:35-37. */
int mvd_layernorm(const float* x, void* y_sp, float* y_f32, const float* w, const float* b, int rows, int C, float eps,
                  int w_plus_one, mvd_stream_t stream); /* y_sp: split planes (rows, C), C % 32 == 0, and / or y_f32: fp32 (rows, C) */
/* mvd_layernorm with one modulation per row group (a scene of a multi-scene training step): rows [g*rows_per_group, (g+1)*rows_per_group)
 * use w + g*ldw / b + g*ldw (w_plus_one as above).  rows_per_group must divide rows; ldw >= 0, a multiple of 4 (0: all groups share
 * w / b).  mvd_layernorm is rows_per_group = rows. */
int mvd_layernorm_groups(const float* x, void* y_sp, float* y_f32, const float* w, const float* b, int ldw, int rows, int rows_per_group,
                         int C, float eps, int w_plus_one, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Self-attention over the tokens of one view (CrossAttention with context=None, attention.py:170-193).
 * Operand planes are written by mvd_gemm(MVD_EPI_QKV):
 *   q/k : [B][heads][Lpad][dq]   16-bit hi/lo planes, dq = roundup(dhead, 16), zero padded (32-channel MFMA steps + one 16-channel tail step), q pre-scaled by
 *                                dhead^-0.5 * log2(e) (mvd_gemm_desc.qscale): the softmax is evaluated with exp2
 *   vt  : [B][heads][dv][Lpad]   16-bit hi/lo planes, dv = roundup(dhead, 16)   (V transposed: keys contiguous)
 * out : (B*L, ldo) split planes, head-major channels ('b n (h d)'): feeds the to_out GEMM. */
size_t mvd_attn_qk_plane_elems(int B, int heads, int L, int dhead);
size_t mvd_attn_vt_plane_elems(int B, int heads, int L, int dhead);
int mvd_attn_lpad(int L);
/* L = tokens (rows) per batch item; Lkeys (0 = L) = the leading tokens that take part as KEYS: a sequence padded to a multiple
 * of 4 rows (CLIP: 257 -> 260) keeps its padding rows out of every softmax.
 * Head widths served: dhead % 4 == 0 with roundup(dhead, 16) in {16, 32, 48, 64, 80, 160}, i.e. 4..80 and 148..160; any other
 * width (84..144, above 160) is refused.  Key rows / V^T columns [Lkeys, Lpad) and query rows [L, Lpad) may hold any finite
 * values (they are masked or never stored); channels [dhead, roundup(dhead, 16)) of q and k must be zero. */
int mvd_attention(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi,
                  const void* vt_lo, void* out_sp, int ldo, int B, int heads, int L, int Lkeys, int dhead, int prec,
                  mvd_stream_t stream);

/* Per-pixel cross attention of one query token against D context tokens (DualAttnetionBlock attn2,
 * mvdfusion/attention.py:56-62; D = n_pts_per_ray).  q (P, C), k/v (P*D, C), out (P, C), C = heads*dhead. */
int mvd_pixel_cross_attn(const float* q, const float* k, const float* v, void* out_sp, int P, int D, int heads,
                         int dhead, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layout / data-movement kernels. */
/* UNet input (unet.py:167-187): x (V,5,S,S) NCHW, input_latents (1,5,S,S) NCHW ->
 * out (2V*S*S, cpad) NHWC in split-planes format: rows [0,V) = [x, il[:4]/0.18215, il[4]] , rows [V,2V) = [x, 0]; channels >= 10 zero.
 * With cfg == 0 only the first V rows are produced. */
int mvd_unet_input(const float* x, const float* input_latents, void* out_sp, int V, int S, int cpad, int cfg,
                   mvd_stream_t stream);
/* mvd_unet_input for nscene scenes of V views each (nscene >= 1; mvd_unet_input is nscene = 1): x (nscene*V,5,S,S) scene-major
 * (global view g = scene*V + v), input_latents (nscene,5,S,S) -> out (2*nscene*V*S*S, cpad): conditional row g = [x[g], il[g / V]],
 * null rows [nscene*V, 2*nscene*V) = [x, 0]. */
int mvd_unet_input_scenes(const float* x, const float* input_latents, void* out_sp, int nscene, int V, int S, int cpad, int cfg,
                          mvd_stream_t stream);
/* out[r, 0:Ca] = a[r], out[r, Ca:Ca+Cb] = b[r]  (torch.cat([h, hs.pop()], dim=1), unet.py:550) */
int mvd_concat_channels(const float* a, int Ca, const float* b, int Cb, float* out, void* out_sp, int rows, long long* gn_stats,
                        int gn_hw, int gn_groups, mvd_stream_t stream);
/* concat + the GroupNorm (+ SiLU) that consumes it, in one launch (unet.py:550 -> openaimodel.py:201-204): y_sp (B*hw, Ca+Cb planes) =
 * act(GroupNorm([a | b]) * gamma + beta), raw_sp (optional) = planes of [a | b] itself (the ResBlock's 1x1 skip convolution reads them),
 * out (optional) = the fp32 concatenation, gn_stats (optional) = the {sum, sum of squares} slot of the result as mvd_concat_channels
 * writes it.  `silu`: bit 0 SiLU, bit 1 fp16 rounding first.  A workgroup per (image, group) holds its hw x (C / groups) values in LDS:
 * mvd_concat_groupnorm_fits() tells whether a shape is served (even Ca, Cb and group width, <= 128 KiB per group); otherwise use
 * mvd_concat_channels + mvd_groupnorm_from_stats. */
int mvd_concat_groupnorm_fits(int Ca, int Cb, int hw, int groups);
int mvd_concat_groupnorm(const float* a, int Ca, const float* b, int Cb, float* out, void* raw_sp, void* y_sp, const float* gamma,
                         const float* beta, long long* gn_stats, int B, int hw, int groups, float eps, int silu, mvd_stream_t stream);
/* out_sp optional: split planes for the 1x1 skip conv; gn_stats optional: GroupNorm statistics of `out` (as mvd_gemm_desc.gn_stats;
 * rows % 16 == 0, gn_hw % 16 == 0, (Ca + Cb) % gn_groups == 0, Ca + Cb <= 2560) */
/* area pooling by `factor` of vol (B, S, S, D, C) -> (B, S/f, S/f, D, C)  (unet.py:198-209).  Output: split planes with
 * ldp elements per row (0 = C): the pooled levels only feed GEMMs, and with D == 1 they are written straight into the
 * [attention output | volume features] operand of the merged to_out / cross-attention GEMM (out_sp then points at the
 * volume columns of that wider buffer). */
int mvd_area_pool(const float* vol, void* out_sp, int B, int S, int D, int C, int factor, int ldp, mvd_stream_t stream);
/* out[i] = 0 (memset as a kernel so it is graph-capturable on any stream) */
int mvd_fill_zero(float* p, size_t n, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-step scalars.  A device table `steps` of nsteps x MVD_STEP_STRIDE floats, indexed by a device-resident
 * iteration counter *iter (so a captured graph needs no per-step host input):
 *   [0] t  [1] sqrt(alpha_bar_t)  [2] depth_std = sqrt(1-ab)/sqrt(ab)/10  [3] a_t  [4] a_prev  [5] sigma_t
 *   [6] sqrt(1-a_t)  [7] 1 if noise is added at this step (sampler.py:63-65) */
#define MVD_STEP_STRIDE 8
/* sinusoidal embedding, cos first (diffusionmodules/util.py:152-172; mvdfusion/embedder.py:114-134): out (dim).
 * freqs (dim/2) = exp(-ln(1e4) * i / (dim/2)) is computed once on the host exactly as the reference does. */
int mvd_timestep_embedding(const float* steps, const int* iter, const float* freqs, float* out, int dim,
                           mvd_stream_t stream);
/* nscene sinusoid rows: out row n (dim floats) from step row *iter + n*steps_scene_stride (each scene of a training step has its own
 * timestep).  steps must hold that many rows; steps_scene_stride is 0 when nscene = 1 (then = mvd_timestep_embedding). */
int mvd_timestep_embedding_scenes(const float* steps, const int* iter, const float* freqs, float* out, int dim, int nscene,
                                  int steps_scene_stride, mvd_stream_t stream);
int mvd_advance_iter(int* iter, mvd_stream_t stream);

/* Vectors of a step that depend on the conditioning or on the schedule only: computed once per sample by the step's own launches
 * (mvd_gemv per <= 16 rows, mvd_timestep_embedding_scenes), so every row is bit-identical to what the step would compute in place.
 *
 * mvd_cond_vectors: cc_projection (viewfusion_zero_depth_rgb.py:96-104,322) and the length-1 cross-attention vectors of all layers:
 *   h1 = SiLU(w0 clip + b0), h2 = SiLU(w2 h1 + b2), context[:rows] = w4 h2 + b4      (rows x width each; clip rows x k_in, ld_clip)
 *   xvec = wx context + bx over ALL ctx_rows rows of context (rows of the null branch beyond `rows` are read as they are), (ctx_rows, nx).
 * mvd_step_table: for every row r of `steps` (n_rows x MVD_STEP_STRIDE; row0 points at a device int holding 0):
 *   tsin[r] = sinusoid(dim) of t_r, h[r] = SiLU(w0 tsin[r] + b0), emb[r] = w2 h[r] + b2 (hidden), and with w3: out3[r] = w3 SiLU(emb[r]) + b3
 *   (n3) -- ViewFusion.time_embed (w3 NULL) and the UNet's time_embed + row-concatenated emb_layers (unet.py:537-538).
 * mvd_select_step_rows: d_i[0 .. w_i) = t_i[*iter][0 .. w_i) for up to three tables of n_rows rows (w_i floats, multiples of 4, 16-byte
 *   aligned; w1 / w2 = 0 skip a table): the one launch of a captured step that picks the row of the device iteration counter.  A counter
 *   outside [0, n_rows) copies nothing. */
int mvd_cond_vectors(const float* clip, int ld_clip, int rows, int k_in, int width, const float* w0, const float* b0, const float* w2,
                     const float* b2, const float* w4, const float* b4, float* h1, float* h2, float* context, const float* wx,
                     const float* bx, int nx, int ctx_rows, float* xvec, mvd_stream_t stream);
int mvd_step_table(const float* steps, const int* row0, int n_rows, const float* freqs, int dim, int hidden, const float* w0,
                   const float* b0, const float* w2, const float* b2, const float* w3, const float* b3, int n3, float* tsin, float* h,
                   float* emb, float* out3, mvd_stream_t stream);
int mvd_select_step_rows(const int* iter, int n_rows, const float* t0, float* d0, int w0, const float* t1, float* d1, int w1,
                         const float* t2, float* d2, int w2, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GridAttn: depth-conditioned cross-view aggregation (mvdfusion/view_attn_efficient2.py).
 * Camera record (20 floats): R row-major (9), T (3), focal (2), principal point (2), centre C = -T R^T (3), pad. */
#define MVD_CAM_RECORD 20
#define MVD_TOKEN_DIM 723
#define MVD_TOKEN_LD 736
/* z_embedder: Linear(5->256)+GELU per pixel (:152,434-437).  lat (N,5,S,S) NCHW -> feat (N,S,S,256) NHWC. */
int mvd_zembed(const float* lat, const float* w, const float* b, float* feat, int N, int S, mvd_stream_t stream);
/* G1-G3 (:269-370, :418-432; utils/ray_utils.py:128-212,263-269,367-369; utils/common_utils.py:229-244):
 * depth sample -> unproject -> reproject into every view and the input view -> bilinear gather (border,
 * align_corners) -> Plucker / harmonic embeddings.  Writes the (T, MVD_TOKEN_LD) token matrix, row
 * ((b*S*S + pix)*D + d)*V + v_ref, T = V*S*S*D*V; columns >= 723 are zero.
 * x (V,5,S,S) NCHW noisy latents; depth_noise (nsteps, V, D, S, S) standard normal (host-ordered, trap T2). */
int mvd_gridattn_tokens(const float* x, const float* depth_noise, const float* steps, const int* iter,
                        const float* grid_lin /* (S) = linspace(1-1/S, -1+1/S, S), ray_utils.py:263-267 */,
                        const float* feat, const float* in_feat, const float* cams, const float* in_cam,
                        void* tokens_sp, int V, int q0, int Vq, int S, int D, float depth_scale, float depth_shift,
                        mvd_stream_t stream);
/* mvd_gridattn_tokens for nscene independent scenes of V views each in one launch (nscene >= 1; mvd_gridattn_tokens is nscene = 1).
 * Global view g = scene*V + v: x (nscene*V,5,S,S), feat (nscene*V,S,S,256), cams (nscene*V, MVD_CAM_RECORD), depth_noise
 * (nsteps, nscene*V, D, S, S); per scene: in_feat (nscene,S,S,256), in_cam (nscene, MVD_CAM_RECORD).  Rows are scene-major:
 * scene*(Vq*S*S*D*V) + the single-scene row; every scene takes the query views [q0, q0+Vq) of its own rig. */
int mvd_gridattn_tokens_scenes(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                               const float* feat, const float* in_feat, const float* cams, const float* in_cam, void* tokens_sp,
                               int nscene, int V, int q0, int Vq, int S, int D, float depth_scale, float depth_shift,
                               mvd_stream_t stream);
/* mvd_gridattn_tokens_scenes with a timestep per scene: scene n reads step row *iter + n*steps_scene_stride (its x0-depth divisor and
 * depth std); the depth noise stays indexed by *iter.  The step table must hold those rows.  steps_scene_stride = 0 is
 * mvd_gridattn_tokens_scenes (bit-identical); nscene = 1 requires 0. */
int mvd_gridattn_tokens_scenes_t(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                                 const float* feat, const float* in_feat, const float* cams, const float* in_cam, void* tokens_sp,
                                 int nscene, int V, int q0, int Vq, int S, int D, float depth_scale, float depth_shift,
                                 int steps_scene_stride, mvd_stream_t stream);
/* Fused G1-G4 (:269-397): tokens are generated in registers and pushed through pre_layer_b, the 3 DiTBlocks over the V views,
 * and the weight_layer softmax pooling in ONE launch; output = the pooled (Vq*S*S*D, 256) rows as split planes (the final
 * Linear 256->768 is a plain mvd_gemm).  1 <= V <= 16: a wavefront owns 16 token rows = 16 / Vp points, Vp = the next power of
 * two >= V; the Vp - V padding slots of a point are masked as attention keys and in the pooling (the reference ships V = 15, 7, 5:
 * configs/mvd_gso.yaml:97, mvd_train.yaml:90,97); Vq*S*S*D*Vp must be a multiple of 64.  V > 16: the unfused kernels above / below.
 *   prec    : MVD_PREC_X4 = all four partial products of the operand split, MVD_PREC_X3 = without lo*lo (every MFMA of the kernel:
 *             the five Linear layers per block and Q K^T)
 *   wstream : the aggregation weights as fp16 (bf16) hi + lo in the kernel's consumption order, mvd_gridattn_fused_slots()
 *             slots of 32 KiB (layout: csrc/gridattn_fused.hip header; packer: mvdfusion_amd/view_attn_efficient2.py)
 *   vecs    : mvd_gridattn_fused_vec_floats() floats -- per DiT block [adaLN modulation of this step 1536 | b_qkv 768 |
 *             b_proj 256 | b_fc1 512 | b_fc2 256], then [b_pre 256 | weight_layer.w 256 | weight_layer.b 1 ... accumulator
 *             scales at +520: pre, then (qkv, proj, fc1, fc2) per block] */
int mvd_gridattn_fused_slots(void);
size_t mvd_gridattn_fused_stream_bytes(void);
size_t mvd_gridattn_fused_vec_floats(void);
int mvd_gridattn_fused(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                       const float* feat, const float* in_feat, const float* cams, const float* in_cam, const void* wstream,
                       const float* vecs, void* pooled_sp, int V, int q0, int Vq, int S, int D, float depth_scale,
                       float depth_shift, int prec /* MVD_PREC_X3 | MVD_PREC_X4: partial products per MAC, as mvd_gemm_desc.prec */,
                       mvd_stream_t stream);
/* mvd_gridattn_fused for nscene independent scenes of V views each in one launch (nscene >= 1; mvd_gridattn_fused is nscene = 1),
 * same per-view / per-scene layouts as mvd_gridattn_tokens_scenes; pooled rows scene-major (scene*Vq*S*S*D + the single-scene row).
 * Vq*S*S*D*Vp (one scene's padded token rows) must be a multiple of 64: a workgroup never straddles two scenes.  The weight stream
 * and vecs are shared by all scenes (one timestep; mvd_gridattn_fused_scenes_t: one per scene). */
int mvd_gridattn_fused_scenes(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                              const float* feat, const float* in_feat, const float* cams, const float* in_cam, const void* wstream,
                              const float* vecs, void* pooled_sp, int nscene, int V, int q0, int Vq, int S, int D, float depth_scale,
                              float depth_shift, int prec, mvd_stream_t stream);
/* mvd_gridattn_fused_scenes with a timestep per scene: scene n reads step row *iter + n*steps_scene_stride and the whole vector table at
 * vecs + n*vecs_scene_stride floats (its adaLN modulation; the biases / scales are repeated per scene), e.g. vecs_scene_stride =
 * mvd_gridattn_fused_vec_floats() for an (nscene, vec_floats) table.  The depth noise stays indexed by *iter.  Both strides 0 is
 * mvd_gridattn_fused_scenes (bit-identical); nscene = 1 requires both 0; vecs_scene_stride % 4 == 0 (16-byte alignment). */
int mvd_gridattn_fused_scenes_t(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                                const float* feat, const float* in_feat, const float* cams, const float* in_cam, const void* wstream,
                                const float* vecs, void* pooled_sp, int nscene, int V, int q0, int Vq, int S, int D, float depth_scale,
                                float depth_shift, int prec, int steps_scene_stride, int vecs_scene_stride, mvd_stream_t stream);
/* Windowed cross-view aggregation (GridAttn keep_top_k_views, :375-384): a 3-D point of query view b is aggregated over W rig
 * neighbours of b, not over all V views.  `window` = W = 2*(top_k/2) + 1 (odd); window = 0 = all views, which is exactly the
 * _scenes_t form of the same name (bit-identical: every entry point above is the window = 0 case).
 *   rows     : (scene, (query view, pixel, depth sample), slot) -- scene*(Vq*S*S*D*W) + ((qv*S*S + pix)*D + d)*W + slot for the token
 *              matrix (T = nscene*Vq*S*S*D*W rows); the fused kernel pads the W slots of a point to the next power of two internally.
 *   slot j   : reference view (b + j - W/2) mod V of the query view's own rig, b = q0 + qv = the view's index in the WHOLE rig (not in a
 *              shard [q0, q0+Vq)).  W > V repeats views through the modulo, as the reference does.
 * The rig size V indexes cameras, feature maps, latents and depth noise only; the rows per point -- hence the 16-row bound of the
 * kernels, mvd_view_mha / mvd_view_pool sequence lengths and the padded-row multiple of 64 -- go by W, so V > 16 runs with W <= 16
 * (fused: V <= 65535). */
int mvd_gridattn_tokens_window(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                               const float* feat, const float* in_feat, const float* cams, const float* in_cam, void* tokens_sp,
                               int nscene, int V, int q0, int Vq, int S, int D, float depth_scale, float depth_shift,
                               int steps_scene_stride, int window, mvd_stream_t stream);
int mvd_gridattn_fused_window(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                              const float* feat, const float* in_feat, const float* cams, const float* in_cam, const void* wstream,
                              const float* vecs, void* pooled_sp, int nscene, int V, int q0, int Vq, int S, int D, float depth_scale,
                              float depth_shift, int prec, int steps_scene_stride, int vecs_scene_stride, int window,
                              mvd_stream_t stream);
/* timm Attention core over the V reference views (:52): qkv (Nseq*V, 3*heads*dhead) -> out (Nseq*V, heads*dhead); V = the sequence
 * length: the window W with mvd_gridattn_tokens_window rows */
int mvd_view_mha(const float* qkv, void* out_sp, int Nseq, int V, int heads, int dhead,
                 mvd_stream_t stream); /* output: split planes */
/* weight_layer + softmax over V + weighted sum (:83,396-397): x (Nseq*V, C) -> out (Nseq, C) */
int mvd_view_pool(const float* x, const float* w, const float* b, void* out_sp, int Nseq, int V, int C,
                  mvd_stream_t stream); /* output: split planes */

/* ------------------------------------------------------------------------------------------------
 * CFG combine + DDIM update (unet.py:195; sampler.py:43-66), fused elementwise.
 * eps_nhwc (2V or V, S, S, ldc) UNet head output; x (V,5,S,S) NCHW updated IN PLACE; x0 (V,5,S,S) out.
 * ddim_noise (nsteps, V, 5, S, S).  eps_out (V,5,S,S) NCHW or NULL receives the guided prediction. */
int mvd_cfg_ddim_update(const float* eps_nhwc, int ldc, float* x, float* x0, float* eps_out,
                        const float* ddim_noise, size_t noise_stride /* floats between consecutive steps */,
                        const float* steps, const int* iter, int V, int S, int cfg, float cfg_scale, int do_update,
                        mvd_stream_t stream);

/* Pinned views (sampler.py:109-110,123-124 `overwrite_x_noisy`, generalised): rewrite the first K view rows of every group of
 * group_views rows of x (groups*group_views, 5, S, S) from known (groups*K, 5, S, S); every other row of x / x0 is left alone.
 *   mode 0 (clean) : x[g*group_views + k] = known[g*K + k]; x0 untouched; noise / steps / iter may be NULL
 *   mode 1 (noised): x[row] = steps[*iter][1] * known + steps[*iter][6] * noise[*iter][g*K + k] (sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t)
 *                    of the step the device counter points at) and x0[row] = known; noise (nsteps, groups*K, 5, S, S)
 * 0 < K <= group_views.  With S*S % 4 == 0 the rows move as float4: every pointer 16-byte aligned, noise_stride % 4 == 0. */
int mvd_pin_views(float* x, float* x0, const float* known, const float* noise, size_t noise_stride /* floats between consecutive steps */,
                  const float* steps, const int* iter, int groups, int group_views, int K, int S, int mode, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fusion of the sampled RGB-D views into one depth-consistent coloured point cloud (csrc/fusion.hip; host: mvdfusion_amd/fusion.py).
 * Not in the reference, whose driver stops at decoded images and a depth PNG; the cameras, NDC convention and depth map are GridAttn's.
 *
 * mvd_fuse_points: one output point per pixel of a P x P grid per view, P = S * up (integer up >= 1), ordered
 *   pt = ((scene*V + b)*P + Y)*P + X.  Fine pixel (Y, X) takes the depth of latent pixel (Y / up, X / up) (nearest replication) and its ray
 *   goes through its own centre: NDC (ndc_lin[X], ndc_lin[Y]) with ndc_lin (P) = linspace(1 - 1/P, -1 + 1/P, P) in fp32 from the host.
 *   lat (nscene*V, 5, S, S) NCHW, channel 4 = depth; rgb (nscene*V, 3, P, P) or NULL; cams (nscene*V, MVD_CAM_RECORD).
 *   Own point : dn = clamp((lat + 1) / 2, 0, 1); foreground iff lo < dn < hi; z = dn * depth_scale + depth_shift (GridAttn's map of a
 *               depth sample); xyz[pt] = unproject(cam_b, ndc, z) for EVERY point; color[pt] = rgb[.., Y, X] bit for bit (rgb NULL: color
 *               is not touched and may be NULL); flags[pt] = MVD_FUSE_FOREGROUND or 0.
 *   Pair rule : for every other view v of the scene's rig, camera-space (xc, yc, zc) and NDC (u, w) of the point.  Seen iff zc > 0,
 *               |u| <= 1 and |w| <= 1 (NaN: unseen).  Continuous latent pixel ix = clamp((1 - u) * S / 2 - 0.5, 0, S - 1), iy alike --
 *               geometric pixel centres with a border clamp, NOT GridAttn's align_corners lookup (half a pixel off at the image edge:
 *               harmless for features, wrong for a depth comparison).  Taps x0 = floor(ix), x1 = min(x0 + 1, S - 1), y alike; if any of
 *               the four is not foreground the pair casts no vote.  Else zs = bilinear of the four metric depths, dz = zc - zs:
 *               |dz| <= tau supports, dz < -tau conflicts (the point floats in front of the surface v sees), dz > tau is occlusion.
 *   support[pt], conflict[pt]: uint8 counts over the other views (1 <= V <= 255; V = 1: all zero).
 *   stage     : the two forms of the kernel give the same bits.  MVD_FUSE_STAGE_GLOBAL reads the depth maps from global memory;
 *               MVD_FUSE_STAGE_LDS stages the scene's V depth planes and camera records in LDS per workgroup (refused beyond 128 KiB) and
 *               walks the scene's points in a grid-stride loop.  MVD_FUSE_STAGE_AUTO is the global form: measured on an MI355X the staged
 *               one is nowhere faster by more than 1 % and up to 3x slower.
 *   All fp32, compiled without contraction.  nscene * V * P * P < 2^31.
 *
 * mvd_compact_points: stable stream compaction of those arrays.  keep = foreground && support >= min_support && conflict <= max_conflicts;
 *   kept points go, in point order, to out_xyz (n, 3), out_color (n, 3; with color, both or neither), out_support (n), out_index (n) = pt;
 *   *count = n (device).  Rows >= n are not touched.  No atomics: wavefront ballots, block counts, one scan, scatter -- deterministic.
 *   The foreground bit travels in the flags byte written by the fuse kernel (not recomputed from lat: the compaction needs no geometry
 *   arguments and any caller-made mask can be compacted).  scratch: mvd_compact_points_scratch bytes for npts, 4-byte aligned. */
#define MVD_FUSE_FOREGROUND 1
#define MVD_FUSE_STAGE_AUTO 0
#define MVD_FUSE_STAGE_GLOBAL 1
#define MVD_FUSE_STAGE_LDS 2
int mvd_fuse_points(const float* lat, const float* rgb, const float* cams, const float* ndc_lin, float* xyz, float* color,
                    uint8_t* support, uint8_t* conflict, uint8_t* flags, int nscene, int V, int S, int up, float depth_scale,
                    float depth_shift, float lo, float hi, float tau, int stage, mvd_stream_t stream);
size_t mvd_compact_points_scratch(size_t npts);
int mvd_compact_points(const float* xyz, const float* color, const uint8_t* support, const uint8_t* conflict, const uint8_t* flags,
                       size_t npts, int min_support, int max_conflicts, float* out_xyz, float* out_color, uint8_t* out_support,
                       int* out_index, unsigned* count, void* scratch, size_t scratch_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rendering a point cloud into cameras: z-buffered point splatting (csrc/fusion.hip; host: mvdfusion_amd/fusion.py render_points).
 * Not in the reference either.  One primitive gives a novel view, the depth map the rig as a whole implies for a view, and the map of
 * which source point each pixel shows: project every point into a camera and keep, per pixel, the nearest one.
 *
 * mvd_render_points:
 *   xyz (n, 3) fp32 world points; color (n, 3) fp32 or NULL; scene_start: nscene + 1 int32 DEVICE values, points
 *   [scene_start[s], scene_start[s + 1]) belong to scene s (the arrays are sorted by scene; values are clamped to [0, n]);
 *   cams (nscene*M, MVD_CAM_RECORD): M target cameras per scene, camera c = s*M + j; P: output side in pixels;
 *   radius r: integer, 0 <= r <= MVD_SPLAT_MAX_RADIUS; znear >= 0; empty_depth; background: 3 floats on the HOST (read at the call;
 *   may be NULL when color is NULL).
 *   Projection: for point i of scene s and camera j of that scene, (u, w, zc) = NDC and camera-space z exactly as mvd_fuse_points'
 *               pair rule computes them (one function in the source).  cx = (1 - u) * P / 2 - 0.5, cy alike from w: geometric pixel
 *               centres, the expression and operation order of the fuse kernel's depth lookup with P for S and no clamp.
 *               Centre pixel px = floor(cx + 0.5), py = floor(cy + 0.5).
 *   Dropped   : the pair draws nothing unless zc > znear and cx, cy are finite (a NaN anywhere drops it; the float-to-int conversion
 *               happens only for centres within r + 2 pixels of the image -- any other covers no pixel).
 *   Footprint : the pixels (py + dy, px + dx), |dx|, |dy| <= r, clipped to the image; a centre outside the image still draws the part of
 *               its footprint that is inside.
 *   Depth rule: every covered pixel takes the minimum of key = (uint64(bits(zc)) << 32) | i.  zc > 0, so the bit pattern orders like the
 *               value: the nearest point wins, between points with identical zc bits the one that comes first in the input.  The result
 *               is a pure function of the inputs, bit-identical run to run whatever order the atomics arrive in.  An empty pixel holds
 *               all ones (no key equals it: i <= 2^31 - 2, and bits of all ones are a NaN, which is dropped).
 *   Outputs per (camera, pixel): index (nscene*M, P, P) int32 = the winner's position i in the input arrays, or -1;
 *               depth (nscene*M, P, P) fp32 = the winner's zc bit for bit, or empty_depth; rgb (nscene*M, 3, P, P) fp32 planar =
 *               color[index] bit for bit, or background -- with color NULL rgb is not touched and may be NULL.
 *   All fp32, compiled without contraction.  n <= 2^31 - 1; nscene * M * P * P < 2^31; nscene * M <= 65535.
 *   scratch   : the 64-bit z-buffer, mvd_render_points_scratch(nscene*M, P) bytes, 8-byte aligned.
 *   Three enqueues on the caller's stream: fill the z-buffer with ones, the splat kernel (one 64-bit unsigned atomicMin per covered
 *   pixel, device scope; workgroups never straddle scenes or cameras), the resolve kernel (one thread per output pixel).  Every argument
 *   is checked before anything is enqueued.
 * mvd_render_points_stages: the same call restricted to the stages in `stages` (an OR of MVD_RENDER_FILL / _SPLAT / _RESOLVE;
 *   MVD_RENDER_ALL is mvd_render_points) -- for timing one stage (tools/bench_render.py) or re-resolving a z-buffer. */
#define MVD_SPLAT_MAX_RADIUS 4
#define MVD_RENDER_FILL 1
#define MVD_RENDER_SPLAT 2
#define MVD_RENDER_RESOLVE 4
#define MVD_RENDER_ALL 7
size_t mvd_render_points_scratch(int ncam, int P);
int mvd_render_points(const float* xyz, const float* color, const int* scene_start, const float* cams, size_t n, int nscene, int M, int P,
                      int radius, float znear, float empty_depth, const float* background, int* index, float* depth, float* rgb,
                      void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_render_points_stages(const float* xyz, const float* color, const int* scene_start, const float* cams, size_t n, int nscene, int M,
                             int P, int radius, float znear, float empty_depth, const float* background, int* index, float* depth,
                             float* rgb, void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rendering a triangle mesh into cameras: z-buffered rasterisation (csrc/raster.hip; host: mvdfusion_amd/fusion.py render_mesh).
 * Not in the reference either.  The mesh counterpart of mvd_render_points with the same 64-bit z-buffer: a hole-free novel view, the depth
 * map the surface implies for a camera, and the map of which face each pixel shows.  It takes the arrays mvd_mesh_emit (below) makes.
 *
 * mvd_render_mesh:
 *   vertices (nvert, 3) fp32 world points; colors (nvert, 3) fp32 or NULL; faces (nface, 3) int32 GLOBAL vertex ids; vertex_start,
 *   face_start: nscene + 1 int32 DEVICE values each, as mvd_mesh_count writes them -- scene s owns the vertices
 *   [vertex_start[s], vertex_start[s + 1]) and the faces [face_start[s], face_start[s + 1]) (values are clamped to [0, nvert] and
 *   [0, nface]); cams (nscene*M, MVD_CAM_RECORD): M target cameras per scene, camera c = s*M + j; P: output side in pixels; cull: 0 or 1;
 *   znear >= 0; empty_depth; background: 3 floats on the HOST (read at the call; may be NULL when colors is NULL).
 *   Projection: for every vertex of face f of scene s and camera j of that scene, (u, w, zc) = NDC and camera-space z exactly as
 *               mvd_render_points computes them (one function in the source).  px = (1 - u) * P / 2 - 0.5, py alike from w: the pixel
 *               coordinates of the point renderer, in which pixel (x, y) has its centre at the integers (x, y).  Below a, b, c are the
 *               face's three vertices in the order faces lists them, (ax, ay) ... their pixel coordinates, z_a ... their zc.
 *   Dropped   : face f = (a, b, c) draws nothing into camera j unless ALL of
 *                 - the three ids lie in the scene's vertex range (no other vertex is ever read);
 *                 - z_a, z_b, z_c > znear.  There is NO near-plane clipping: a face with one vertex at or behind znear is dropped whole
 *                   (the rigs here look at an object in front of them);
 *                 - the six pixel coordinates are finite (a NaN anywhere drops the face);
 *                 - area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) is finite and non-zero (mvd_mesh_emit emits zero-area
 *                   triangles by design: they draw nothing);
 *                 - with cull = 1: area2 < 0, the face is a FRONT face.  A face is front when its geometric normal n = (b - a) x (c - a)
 *                   -- which mvd_mesh_emit winds out of the surface -- faces the camera: n . a < 0 with a, b, c in camera space (a
 *                   rotation keeps the cross product).  n . a is the determinant det[a; b; c], and the signed area of the triangle
 *                   (x / z, y / z) is det[a; b; c] / (z_a z_b z_c); px and py both DEcrease with x / z and y / z, which cancels, and the
 *                   focal lengths (assumed of one sign, as in every camera here) and z are positive: area2 has the sign of n . a.
 *                   cull = 0 draws both sides.
 *   Coverage  : with e_a = (bx - x) * (cy - y) - (by - y) * (cx - x), e_b = (cx - x) * (ay - y) - (cy - y) * (ax - x),
 *               e_c = (ax - x) * (by - y) - (ay - y) * (bx - x) and sg = +1 for area2 > 0, else -1, pixel (x, y) is covered when
 *               e_a * sg >= 0, e_b * sg >= 0 and e_c * sg >= 0.  Edges are inclusive and there is no top-left rule: a centre exactly on a
 *               shared edge is covered by both faces and the depth rule decides.  Candidates are the integer pixels of
 *               [ceil(min x), floor(max x)] x [ceil(min y), floor(max y)] clipped to [0, P - 1] (the conversion to int happens after
 *               the clip).
 *   Depth, barycentrics (perspective-correct), in THIS order: q_i = (e_i / area2) / z_i; iz = (q_a + q_b) + q_c; z = 1 / iz;
 *               b_i = q_i * z.  A covered pixel whose z is not finite or not > znear draws nothing.
 *   Depth rule: every drawn pixel takes the minimum of key = (uint64(bits(z)) << 32) | f.  z > 0, so the bit pattern orders like the
 *               value: the nearest face wins, between faces with identical z bits the one with the lowest id.  The result is a pure
 *               function of the inputs, bit-identical run to run whatever order the atomics arrive in.  An empty pixel holds all ones.
 *   Outputs per (camera, pixel), planar like those of mvd_render_points:
 *               face_out (nscene*M, P, P) int32 = the winner's f, or -1;
 *               depth (nscene*M, P, P) fp32 = its z, the bits of the key's high word, or empty_depth;
 *               bary (nscene*M, 3, P, P) fp32 = b_a, b_b, b_c of the winner at the pixel, or 0;
 *               normal (nscene*M, 3, P, P) fp32 = the face's unit normal in camera space, or 0: n = (b - a) x (c - a) from the WORLD
 *               positions, divided by its largest |component| m, rotated (n_j = n_0 R[0][j] + n_1 R[1][j] + n_2 R[2][j], the
 *               convention of the projection), divided by sqrt((n_0^2 + n_1^2) + n_2^2), and negated when n_2 > 0: normal_z <= 0 always,
 *               the normal points at the image plane whichever side of the face is seen.  (Decided on normal_z, not on n . a: at a
 *               grazing angle off the optical axis the two can differ.)  m == 0 or not finite: 0;
 *               rgb (nscene*M, 3, P, P) fp32 = (b_a * c_a + b_b * c_b) + b_c * c_c per channel, or background -- with colors NULL rgb must
 *               be NULL.
 *   All fp32, compiled without contraction.  nface, nvert <= 2^31 - 1; nscene * M * P * P < 2^31; nscene * M <= 65535.  nface = 0 is a
 *   valid call (vertices and faces may be NULL) and gives empty images.
 *   scratch   : the 64-bit z-buffer, mvd_render_mesh_scratch(nscene*M, P) = nscene*M*P*P*8 bytes (0 for a non-positive argument),
 *               8-byte aligned.
 *   Three enqueues on the caller's stream: fill the z-buffer with ones; the raster kernel -- one thread per (face, camera), workgroups
 *   never straddle scenes or cameras; a thread walks a clipped bounding box of at most 64 pixels itself, larger boxes are walked by the
 *   thread's whole wavefront, 64 pixels at a time; one 64-bit unsigned atomicMin per drawn pixel, device scope; the resolve kernel -- one
 *   thread per output pixel, which evaluates the winner again through the same expressions.  Every argument is checked before anything
 *   is enqueued.
 * mvd_render_mesh_stages: the same call restricted to the stages in `stages` (an OR of MVD_RENDER_FILL / _SPLAT / _RESOLVE as for the
 *   points, _SPLAT being the raster kernel; MVD_RENDER_ALL is mvd_render_mesh). */
size_t mvd_render_mesh_scratch(int ncam, int P);
int mvd_render_mesh(const float* vertices, const float* colors, const int* faces, const int* vertex_start, const int* face_start,
                    const float* cams, size_t nvert, size_t nface, int nscene, int M, int P, int cull, float znear, float empty_depth,
                    const float* background, int* face_out, float* depth, float* bary, float* normal, float* rgb, void* scratch,
                    size_t scratch_bytes, mvd_stream_t stream);
int mvd_render_mesh_stages(const float* vertices, const float* colors, const int* faces, const int* vertex_start, const int* face_start,
                           const float* cams, size_t nvert, size_t nface, int nscene, int M, int P, int cull, float znear,
                           float empty_depth, const float* background, int* face_out, float* depth, float* bary, float* normal, float* rgb,
                           void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Measuring geometry: the exact nearest target point of every query point (csrc/nearest.hip; host: mvdfusion_amd/fusion.py
 * nearest_points, compare_geometry).  Not in the reference either.  Accuracy, completeness, Chamfer distance and precision / recall /
 * F-score between two fused clouds (or the surface samples of two meshes) are reductions of these distances.
 *
 * mvd_nearest_points:
 *   query (nq, 3), target (nt, 3) fp32 world points; query_start, target_start: nscene + 1 int32 DEVICE values each, non-decreasing (the
 *   arrays are sorted by scene); every value is clamped to [0, nq] or [0, nt] before it indexes anything.
 *   Scenes    : query i belongs to scene s when query_start[s] <= i < query_start[s + 1]; its candidates are the targets j with
 *               target_start[s] <= j < target_start[s + 1].
 *   Distance  : d2(i, j) = ((qx - tx) * (qx - tx) + (qy - ty) * (qy - ty)) + (qz - tz) * (qz - tz) in fp32, in exactly this order, every
 *               operation rounded once (compiled without contraction).
 *   Selection : starts from best = +inf with no winner; candidate j wins only with d2 < best, or d2 == best and j below the winner so
 *               far.  The result is the minimum of d2 over the candidates, between equal minima the lowest j: a pure function of the
 *               inputs, whatever order the candidates are met in.
 *   Outputs   : index (nq,) int32 = the winner's j, a global row of target; dist2 (nq,) fp32 = its d2.  Without a winner index = -1 and
 *               dist2 = +inf.  Every element [0, nq) of both is written.
 *   The strict comparison against +inf decides every odd case, with no rule of its own: a target with a NaN or infinite coordinate (or
 *   so far away that d2 overflows) is never chosen; a query with a non-finite coordinate has no winner; neither has a query whose scene
 *   holds no target, nor a query outside [query_start[0], query_start[nscene]).
 *   method    : MVD_NN_BRUTE -- every query of a scene against every target of the scene, the targets staged through LDS in tiles of
 *               16-byte records (x, y, z, j) that all lanes read at the same address.
 *               MVD_NN_GRID -- per scene a uniform grid over the bounding box of the scene's finite targets (found on the device;
 *               minimum and maximum are exact in any order): cubic cells of side h = max(largest extent / grid, 1e-30), per axis
 *               clamp(floor(extent / h) + 1, 1, grid) of them, so coincident, collinear and coplanar targets give a valid grid.  Build:
 *               box, count per cell (integer atomics), exclusive scan, scatter into a cell-sorted copy of records (x, y, z, j); a target
 *               with a non-finite coordinate is in no cell.  The order inside a cell differs from run to run; the selection rule does
 *               not see it.  Query: one thread per query, clamped to its cell, visits the Chebyshev shells of cells r = 0, 1, ... around
 *               it and stops after shell r once best lies strictly below a lower bound of d2 to every point of an unvisited cell.  The
 *               bound is taken from the query's own position in cell units against the faces of the visited block, plus what the query
 *               lies outside the box along the other axes, shrunk by 0.1 % and 0.001 cell -- orders above the fp32 rounding of the
 *               cell assignment, the bound and d2.  The search is exact: index and dist2 are the bits MVD_NN_BRUTE gives.
 *               MVD_NN_AUTO -- chosen from nt / nscene on the host (csrc/nearest.hip: kGridMinTargets; DESIGN.md section
 *               6.000000000000000 has the sweep); nt = 0 runs the brute kernel, which writes -1 / +inf.
 *   grid      : cells per axis of MVD_NN_GRID, 1 .. 256, or 0 for the library's choice from nt / nscene (a host computation that aims
 *               at a few targets per occupied cell of a surface, at most 256).  Ignored by MVD_NN_BRUTE.
 *   Bounded whatever the data: the shell loop ends at r = grid at the latest; cell ranges read back from the scratch are clamped to
 *   [0, nt] and a record counts only when its j lies in the scene's target range; no NaN or out-of-range value reaches a float-to-int
 *   conversion unclamped.
 *   nq, nt <= 2^31 - 1; 1 <= nscene <= 65535; nscene * grid^3 <= 2^31 - 1.  nq = 0 and nt = 0 are valid calls (query, index, dist2 may
 *   be NULL with nq = 0, target with nt = 0).
 *   scratch   : mvd_nearest_points_scratch(nt, nscene, method, grid) bytes, 16-byte aligned; 0 bytes (NULL allowed) for MVD_NN_BRUTE
 *               and wherever MVD_NN_AUTO resolves to it.  The function returns 0 for a non-positive or out-of-range argument.
 *   Everything is enqueued on the caller's stream with no host synchronisation; every argument is checked before anything is enqueued.
 * mvd_nearest_points_stages: the same call restricted to the stages in `stages` (an OR of MVD_NN_BUILD -- box, count, scan, scatter;
 *   nothing for MVD_NN_BRUTE -- and MVD_NN_QUERY; MVD_NN_ALL is mvd_nearest_points) -- for timing the two (tools/bench_nearest.py) or
 *   for several query sets against one built grid. */
#define MVD_NN_AUTO 0
#define MVD_NN_BRUTE 1
#define MVD_NN_GRID 2
#define MVD_NN_BUILD 1
#define MVD_NN_QUERY 2
#define MVD_NN_ALL 3
size_t mvd_nearest_points_scratch(size_t nt, int nscene, int method, int grid);
int mvd_nearest_points(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq, size_t nt,
                       int nscene, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                       mvd_stream_t stream);
int mvd_nearest_points_stages(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq,
                              size_t nt, int nscene, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                              int stages, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbourhoods: the k nearest target points of every query point, and a normal per point from such a list (csrc/nearest.hip,
 * csrc/normals.hip; host: mvdfusion_amd/fusion.py knn_points, estimate_normals).  Not in the reference either.
 *
 * mvd_knn_points: the search of mvd_nearest_points -- its scenes, its d2 in fp32 in the same operation order without contraction, its
 *   method / grid / scratch conventions, its grid build (one copy of the code) -- returning the k best candidates instead of one.
 *   Order     : the candidates of a query (the targets of its scene with d2 < +inf) are totally ordered by (d2, j) lexicographically,
 *               d2 compared in fp32.  The result is the first min(k, candidates) of that order, ascending: a pure function of the
 *               inputs, whatever order cells and records are met in (the grid's scatter order differs run to run).
 *   Outputs   : index (nq, k) int32 and dist2 (nq, k) fp32, row-major; unfilled slots hold -1 / +inf.  Every element is written.
 *   The strict comparison against +inf decides every odd case exactly as in mvd_nearest_points: a non-finite target is in no list, a
 *   non-finite query, a query of an empty scene and a query of no scene get k empty slots.
 *   k         : 1 <= k <= MVD_KNN_MAX_K.  k = 1 gives the bits of mvd_nearest_points.
 *   Self      : query may be target.  A point is then its own candidate at d2 = 0 and stays in the list (in slot 0 unless a coincident
 *               point with a lower row precedes it).  There is no exclude flag.
 *   MVD_NN_GRID : the shell walk of mvd_nearest_points, which stops after shell r once the k-th best so far lies strictly below the
 *               same lower bound; with fewer than k found it runs to the last shell.  The loop is bounded by the host value grid.
 *   MVD_NN_BRUTE: the LDS-tiled scan with a k-list per thread.  MVD_NN_AUTO resolves as for mvd_nearest_points, whatever k.
 *   The list  : kept in registers: the kernels are compiled for list sizes 1, 2, 4, 8, 16 and 32 with the insertion unrolled, and a
 *               call runs the smallest size that holds k.
 *   scratch   : mvd_nearest_points_scratch(nt, nscene, method, grid) bytes, the same layout: a grid built by either search
 *               (MVD_NN_BUILD) serves the MVD_NN_QUERY of both, with the same target, target_start, nt, nscene, method and grid.
 *   All pointers 4-byte aligned, the scratch 16-byte.  Limits, empty sides, enqueue-only and checked-before-enqueue as for
 *   mvd_nearest_points; a refused call writes nothing.
 * mvd_knn_points_stages: the same call restricted to `stages`, as mvd_nearest_points_stages.
 *
 * mvd_point_normals: one normal per point from its neighbour rows, in fp64 throughout, in list order.
 *   target (nt, 3) fp32; index (n, k) int32 rows of target (a row of mvd_knn_points' index, or any list); 1 <= k <= MVD_NORMALS_MAX_K.
 *   Used rows : the entries j of the point's row with 0 <= j < nt and three finite coordinates; m of them.  x = (double) of each.
 *   Centre    : c = (sum of x in list order) / m, per axis.
 *   Covariance: C_ab = sum (x_a - c_a) * (x_b - c_b) for ab = xx, xy, xz, yy, yz, zz: each difference and each product rounded once in
 *               fp64 (no contraction), the addends added in list order.
 *   Eigen     : cyclic Jacobi on C in fp64, MVD_NORMALS_SWEEPS sweeps over (0,1), (0,2), (1,2) with the conventions of mvd_align_solve
 *               (a rotation is skipped where the off-diagonal is 0; tan = 1 / (|theta| + sqrt(theta^2 + 1)), 1 / (2 |theta|) beyond
 *               |theta| = 1e150).  The eigenvalues are the diagonal, each raised to 0 where rounding left it negative; l0 <= l1 <= l2.
 *   Normal    : the eigenvector of the smallest eigenvalue (between equal diagonal entries the lowest column), divided by its length.
 *   Sign      : the component of largest magnitude is made positive, between equal magnitudes the lowest axis decides -- on the fp64
 *               vector.  Then, with toward (n, 3) fp32 and the points themselves p (n, 3) fp32, the normal is negated when
 *               (n_x * (t_x - p_x) + n_y * (t_y - p_y)) + n_z * (t_z - p_z) < 0 in fp64 (a NaN negates nothing).  toward == NULL: no
 *               second step, and points may be NULL.  The normal is rounded to fp32 once, at the end.
 *   variation : (n,) fp32 = l0 / ((l0 + l1) + l2): the surface variation, 0 on a plane, at most 1 / 3.
 *   Valid     : m >= 3 and l1 > 0 (the rows are neither coincident nor collinear) and every sum, eigenvalue and component finite.
 *               Otherwise normal = (0, 0, 0) and variation = NaN: a valid point is one whose variation is not NaN.
 *   normal (n, 3), variation (n,): every element is written.  n = 0 is valid.  n * k <= 2^31 - 1.  One thread per point; enqueued on
 *   the caller's stream, nothing synchronised or allocated, every argument checked before the enqueue. */
#define MVD_KNN_MAX_K 32
#define MVD_NORMALS_MAX_K 256
#define MVD_NORMALS_SWEEPS 10
int mvd_knn_points(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq, size_t nt,
                   int nscene, int k, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                   mvd_stream_t stream);
int mvd_knn_points_stages(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq, size_t nt,
                          int nscene, int k, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                          int stages, mvd_stream_t stream);
int mvd_point_normals(const float* target, size_t nt, const int* index, size_t n, int k, const float* points, const float* toward,
                      float* normal, float* variation, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Aligning geometry: a similarity transform per scene that takes a source cloud onto a target -- the closed form for given pairs, and
 * point-to-point ICP around the search above (csrc/align.hip; host: mvdfusion_amd/fusion.py fit_similarity, align_geometry,
 * Alignment.apply).  Not in the reference either.  A distance between two geometries means something only in one frame.
 *
 * Scenes are those of mvd_nearest_points: nscene + 1 int32 DEVICE offsets, clamped to [0, n] before they index anything.
 * Transform : per scene 12 doubles m[3][4], row-major, m[r][0..2] = s R[r], m[r][3] = t[r]; (nscene, 12) on the device.
 * Apply     : moved[r] = (float)(((m[r][0] * (double)x + m[r][1] * (double)y) + m[r][2] * (double)z) + m[r][3]) in fp64, in this order,
 *             every operation rounded once (compiled without contraction), one rounding to fp32 at the end.  A point of no scene is
 *             copied unchanged.  ICP applies the accumulated transform to the ORIGINAL source every time, never transform on transform.
 * Pairs     : source row i goes with target row j = index[i], or j = i with index == NULL; no pair unless 0 <= j < nt.  Its d2 is
 *             dist2[i], or with dist2 == NULL the distance of mvd_nearest_points ((dx * dx + dy * dy) + dz * dz in fp32) between the
 *             moved point p and the target q.  The pair is ACCEPTED when d2 < +inf and d2 <= max_dist2, compared in fp32 (a NaN is
 *             not accepted; max_dist2 = +inf is no gate).  An accepted pair has finite p and q.
 * Sums      : per scene, over the accepted pairs of its rows, MVD_ALIGN_SUMS = 19 doubles: [0] the count, [1..3] sum p, [4..6] sum q,
 *             [7 + 3 a + b] sum p_a q_b, [16] sum (px px + py py) + pz pz, [17] the same of q, [18] sum (double)d2.  Every product of
 *             two fp32 values is exact in fp64; only the additions round.  A scene is cut into chunks of MVD_ALIGN_CHUNK consecutive
 *             rows counted from the scene's own first row; one workgroup reduces a chunk in a fixed order (thread t its rows
 *             t, t + 256, ...; the lanes of a wavefront in an xor butterfly; the four wavefronts as (w0 + w1) + (w2 + w3)) and the
 *             chunk sums are added per scene in ascending chunk order.  No float atomics: the same bits run to run, and for a scene
 *             alone and inside a batch.  The workgroup-to-(scene, chunk) map is a device prefix of ceil(len_s / chunk); the launch is
 *             sized by the host bound ceil(n / chunk) + nscene.
 *             The moments are raw, not centred in a first pass: their cancellation costs a relative (1 + |mu|^2 / sigma^2) n 2^-53
 *             (mu, sigma^2: mean and variance of the points) -- nothing for objects in the +-0.75 box.
 * Solve     : with n = sums[0], M = sum pq / n - (sum p / n)(sum q / n)^T and var = sum |p|^2 / n - |sum p / n|^2: Horn's symmetric
 *             4 x 4 matrix of M, its dominant eigenvector by cyclic Jacobi in fp64 (a fixed number of sweeps; a rotation is skipped
 *             where the off-diagonal is 0; tan = 1 / (|theta| + sqrt(theta^2 + 1)), and 1 / (2 |theta|) beyond |theta| = 1e150 where
 *             the square would overflow), normalised to a unit quaternion, R formed from it -- a proper rotation whatever the data.
 *             s = sum_ab R_ba M_ab / var with MVD_ALIGN_SCALE, else exactly 1;  t = sum q / n - s R sum p / n.  The step D = [s R | t]
 *             composes as m <- D m in fp64.  D is the identity (s = 1) when fewer than 3 pairs were accepted, when var is not
 *             positive, when a sum or a result is not finite, or when MVD_ALIGN_SCALE finds s <= 0.
 * History   : a row is MVD_ALIGN_HISTORY = 3 doubles per scene: rms = sqrt(sums[18] / n) (NaN with n = 0), n, and the scale so far: the s
 *             of the step (1 without one) times that entry of the row before -- one product per row, in row order, exactly 1 while no
 *             step fits a scale.
 *
 * mvd_align_apply: out (n, 3) = src (n, 3) under transform.  n = 0 is valid.
 * mvd_align_fit  : sums, solve and composition for given pairs: moved (n, 3), start its scene offsets, target (nt, 3), index / dist2
 *             (n,) or NULL as above.  flags: MVD_ALIGN_SCALE; MVD_ALIGN_NO_STEP writes history_row only and leaves transform alone.
 *             history_row (nscene, 3) describes the pairs as given, before the step.  transform is read and written.
 *             scratch: mvd_align_scratch(n, 0, nscene, MVD_NN_BRUTE, 0) bytes, 16-byte aligned.
 * mvd_align_icp  : MVD_NN_BUILD once over target; then iters times { apply transform to source -> moved; MVD_NN_QUERY of moved through
 *             mvd_nearest_points_stages -> index, dist2 (so the correspondences are mvd_nearest_points' bits); fit; history row k };
 *             then a last apply, query and history row (iters) without a step.  transform holds the start on entry and the result on
 *             return; moved, index, dist2 are left as that last pass wrote them; history is (iters + 1, nscene, 3).
 *             0 <= iters <= MVD_ALIGN_MAX_ITERS, a fixed count: nothing is read back, there is no early exit.  method, grid: those
 *             of mvd_nearest_points.  scratch: mvd_align_scratch(nq, nt, nscene, method, grid) bytes (0 for an argument out of range).
 * mvd_align_solve: the solve alone, on the host, the same function the kernel calls: sums[19] -> step[12], *scale.  Needs no GPU.
 * Everything else is enqueued on the caller's stream with no host synchronisation and no allocation; every argument is checked before
 * anything is enqueued, a refused call writes nothing (a failed ENQUEUE inside mvd_align_icp's loop ends the call there, with what the
 * earlier iterations wrote).  Every word of the scratch that is read is written earlier in the same call. */
#define MVD_ALIGN_SCALE 1
#define MVD_ALIGN_NO_STEP 2
#define MVD_ALIGN_CHUNK 1024
#define MVD_ALIGN_SUMS 19
#define MVD_ALIGN_HISTORY 3
#define MVD_ALIGN_MAX_ITERS 1024
size_t mvd_align_scratch(size_t nq, size_t nt, int nscene, int method, int grid);
int mvd_align_solve(const double* sums, int flags, double* step, double* scale);
int mvd_align_apply(const float* src, const int* src_start, size_t n, int nscene, const double* transform, float* out,
                    mvd_stream_t stream);
int mvd_align_fit(const float* moved, const int* start, const float* target, const int* index, const float* dist2, size_t n, size_t nt,
                  int nscene, int flags, float max_dist2, double* transform, double* history_row, void* scratch, size_t scratch_bytes,
                  mvd_stream_t stream);
int mvd_align_icp(const float* source, const int* source_start, const float* target, const int* target_start, size_t nq, size_t nt,
                  int nscene, int method, int grid, int iters, int flags, float max_dist2, double* transform, double* history,
                  float* moved, int* index, float* dist2, void* scratch, size_t scratch_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Aligning to a surface: point-to-plane ICP -- the loop, the pairs, the chunked reduction and the apply of the section above with the
 * linearised point-to-plane error and its six-parameter solve in place of the moments and Horn's closed form (csrc/align.hip; host:
 * mvdfusion_amd/fusion.py fit_plane_step, align_to_surface).  Not in the reference either.  Rigid only: a step is [R | t] with R a
 * proper rotation, so a scale in the transform given on entry is carried through untouched.
 *
 * normals   : (nt, 3) fp32, one per TARGET row (mvd_point_normals' output, or any); unit length is not required.
 * Pairs     : those of mvd_align_fit, accepted as there (d2 < +inf and d2 <= max_dist2 in fp32); in addition the target's normal must
 *             have three finite components, not all zero.
 * Per pair  : in fp64, with p the moved source point, q the target, n its normal (all exact conversions of fp32 values):
 *             e = p - q;  r = (e_x n_x + e_y n_y) + e_z n_z;  c = p x n, each component one subtraction of two exact products
 *             (c_x = p_y n_z - p_z n_y, ...);  a = (c_x, c_y, c_z, n_x, n_y, n_z).  r + a . (omega, t) is the distance of the pair
 *             along n after the small motion x -> x + omega x x + t.
 * Sums      : per scene MVD_PLANE_SUMS = 30 doubles: [0] the count, [1..21] the upper triangle of sum a_i a_j, row-major (00, 01, ..,
 *             05, 11, .., 55), [22..27] sum a_i r, [28] sum r r, [29] sum (double)d2.  Reduced exactly as MVD_ALIGN_SUMS are -- chunks of
 *             MVD_ALIGN_CHUNK rows from the scene's first row, the fixed in-workgroup order, chunk sums added in ascending order, no
 *             float atomics, the device prefix map (one copy of that code): the same bits run to run and for a scene alone or in a batch.
 * Solve     : H (6 x 6, symmetric) from [1..21], g from [22..27].  H is eigen-decomposed by cyclic Jacobi in fp64 (a fixed number of
 *             sweeps, the conventions of mvd_align_solve); lambda_max is the largest diagonal entry; the directions i with
 *             lambda_i > MVD_PLANE_EPS_RANK * lambda_max are KEPT and x = - sum_kept v_i (v_i . g) / lambda_i (i ascending, every dot
 *             product summed in component order).  A direction the data does not constrain is left alone, not blown up: in-plane
 *             motion on a plane target, rotation about the centre on a sphere.  omega = x[0..2], t = x[3..5]; R = exp([omega]x) through
 *             the quaternion (cos(a / 2), omega sin(a / 2) / a), a = |omega| (below a = 1e-4 from the series 1 - a^2 / 8 + a^4 / 384
 *             and 1 / 2 - a^2 / 48 + a^4 / 3840), normalised to unit length -- a proper rotation whatever the data.  D = [R | t]
 *             composes as m <- D m in fp64.  D is the identity, with rank 0, when fewer than 3 pairs were accepted, when lambda_max
 *             is not positive, or when a sum or a result is not finite.
 * History   : a row is MVD_PLANE_HISTORY = 4 doubles per scene: the plane rms sqrt(sums[28] / n), n, the point rms sqrt(sums[29] / n)
 *             (what mvd_align_fit reports; both NaN with n = 0), and the rank the solve of these sums keeps (computed for a row
 *             without a step too).
 *
 * mvd_plane_fit  : mvd_align_fit with normals: sums, solve and composition for given pairs.  flags: MVD_PLANE_NO_STEP writes history_row
 *             only.  scratch: mvd_plane_scratch(n, 0, nscene, MVD_NN_BRUTE, 0) bytes, 16-byte aligned.
 * mvd_plane_icp  : mvd_align_icp's loop with this fit: MVD_NN_BUILD once over target; iters times { apply transform to the ORIGINAL
 *             source -> moved; MVD_NN_QUERY through mvd_nearest_points_stages -> index, dist2; fit; history row k }; then a last apply,
 *             query and row (iters) without a step.  history is (iters + 1, nscene, 4); moved, index, dist2 are left as the last pass
 *             wrote them.  0 <= iters <= MVD_ALIGN_MAX_ITERS, a fixed count, nothing read back.  scratch: mvd_plane_scratch(nq, nt,
 *             nscene, method, grid) bytes (0 for an argument out of range).
 * mvd_plane_solve: the solve alone, on the host, the same function the kernel calls: sums[30] -> step[12], *rank.  Needs no GPU.  (The
 *             rotation goes through cos and sin, so host and device may differ in the last bits; everything before it is sqrt, +, *, /.)
 * Enqueue-only, nothing allocated, every argument checked before anything is enqueued, a refused call writes nothing, and every word of
 * the scratch that is read is written earlier in the same call -- as in the section above. */
#define MVD_PLANE_NO_STEP 2
#define MVD_PLANE_SUMS 30
#define MVD_PLANE_HISTORY 4
#define MVD_PLANE_EPS_RANK 1e-9
size_t mvd_plane_scratch(size_t nq, size_t nt, int nscene, int method, int grid);
int mvd_plane_solve(const double* sums, double* step, int* rank);
int mvd_plane_fit(const float* moved, const int* start, const float* target, const float* normals, const int* index, const float* dist2,
                  size_t n, size_t nt, int nscene, int flags, float max_dist2, double* transform, double* history_row, void* scratch,
                  size_t scratch_bytes, mvd_stream_t stream);
int mvd_plane_icp(const float* source, const int* source_start, const float* target, const int* target_start, const float* normals,
                  size_t nq, size_t nt, int nscene, int method, int grid, int iters, float max_dist2, double* transform, double* history,
                  float* moved, int* index, float* dist2, void* scratch, size_t scratch_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Distance to a surface: the exact closest point of a triangle mesh for every query point, and point-to-plane ICP whose target is the
 * mesh itself (csrc/meshdist.hip, csrc/align.hip; host: mvdfusion_amd/fusion.py nearest_on_mesh, compare_geometry(exact=True),
 * align_to_mesh).  Not in the reference either.  The distance to the nearest SAMPLE of a mesh is an upper bound with a floor of the
 * sample spacing; this is the distance to the triangles.
 *
 * mvd_nearest_on_mesh:
 *   query (nq, 3) fp32; vertices (nv, 3) fp32; faces (nf, 3) int32 GLOBAL rows of vertices; query_start, face_start: nscene + 1 int32
 *   DEVICE values each, non-decreasing, clamped to [0, nq] or [0, nf] before they index anything.
 *   Scenes    : those of mvd_nearest_points: query i of scene s searches the faces f with face_start[s] <= f < face_start[s + 1].
 *   Candidates: a face whose three ids lie in [0, nv) and whose nine coordinates are finite.  A query with a non-finite coordinate, a
 *               query of no scene, or one whose scene holds no candidate gets face = -1, dist2 = +inf, point = NaN, bary = 0,
 *               region = -1, normal = 0.
 *   Per pair  : fp64 throughout, on the exact conversions of the fp32 inputs, every operation rounded once (compiled without
 *               contraction), only + - * / and comparisons.  dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z; a cross product component is one
 *               subtraction of two products (n_x = ab_y ac_z - ab_z ac_y, ...).  With p the query and A, B, C the face's vertices:
 *                 ab = B - A, ac = C - A, n = ab x ac.  If n_x, n_y, n_z are all exactly 0 go to DEGENERATE.
 *                 ap = p - A, d1 = dot(ab, ap), d2 = dot(ac, ap).      d1 <= 0 and d2 <= 0                : region 0, b = (1, 0, 0)
 *                 bp = p - B, d3 = dot(ab, bp), d4 = dot(ac, bp).      d3 >= 0 and d4 <= d3               : region 1, b = (0, 1, 0)
 *                 vc = d1 d4 - d3 d2.        vc <= 0, d1 >= 0, d3 <= 0 : region 3 (edge AB), v = d1 / (d1 - d3),     b = (1 - v, v, 0)
 *                 cp = p - C, d5 = dot(ab, cp), d6 = dot(ac, cp).      d6 >= 0 and d5 <= d6               : region 2, b = (0, 0, 1)
 *                 vb = d5 d2 - d1 d6.        vb <= 0, d2 >= 0, d6 <= 0 : region 5 (edge CA), w = d2 / (d2 - d6),     b = (1 - w, 0, w)
 *                 va = d3 d6 - d5 d4, e = d4 - d3, f = d5 - d6.
 *                                            va <= 0, e >= 0, f >= 0   : region 4 (edge BC), w = e / (e + f),        b = (0, 1 - w, w)
 *                 den = (va + vb) + vc;      den != 0                  : region 6 (interior), v = vb / den, w = vc / den,
 *                                                                        b = ((1 - v) - w, v, w);   den == 0: go to DEGENERATE.
 *               The tests are made in this order and the first that holds decides (Ericson, Real-Time Collision Detection, 5.1.5).  An
 *               edge denominator that is exactly 0 is not divided by: the parameter is 0.
 *               DEGENERATE (collinear or coincident vertices): the three segments A -> B, B -> C, C -> A in this order, each S -> E with
 *               se = E - S, sp = p - S, len2 = dot(se, se), t = dot(sp, se) / len2 (t = 0 when len2 == 0: the segment is its first end
 *               point), t raised to 0 unless t > 0 and lowered to 1 where t > 1; b has 1 - t at S and t at E; region = the vertex code of S
 *               when t == 0, of E when t == 1, else the edge code (3, 4, 5 in segment order).  The first segment stands; a later one
 *               replaces it only with a strictly smaller d2.
 *               Then, for every path: c_k = (b0 A_k + b1 B_k) + b2 C_k per axis k, and d2 = (dx dx + dy dy) + dz dz with d = p - c.
 *               A numpy float64 restatement in this order gives the same bits (tests/meshdist_f64.py).
 *   Selection : per query the minimum of (d2 in fp64, face row) in that lexicographic order, a total order: between equal d2 the lowest
 *               row wins, and the result cannot depend on the order the faces are met in or on how often one is met.
 *   Outputs   : each optional -- a NULL is not written; every element [0, nq) of the others is.
 *               face (nq,) int32 the chosen row; dist2 (nq,) fp32 the fp64 d2 rounded once (+inf when it overflows fp32: the face is
 *               still reported); point (nq, 3) fp32 c; bary (nq, 3) fp32 b; region (nq,) int32 0..2 a vertex (A, B, C), 3..5 an edge
 *               (AB, BC, CA), 6 the interior; normal (nq, 3) fp32: the fp64 (B - A) x (C - A) divided by its length sqrt((n_x n_x +
 *               n_y n_y) + n_z n_z), rounded once; 0 where that length is 0 or not finite.  It is the normal mvdfusion_amd/fusion.py
 *               sample_normals gives for the face (to the rounding of its norm).
 *   method    : MVD_NN_BRUTE -- every query of a scene against every face of the scene, staged through LDS as resolved 48-byte records.
 *               MVD_NN_GRID -- the grid of mvd_nearest_points (its box keys, cell side, cell function, shell walk and stop rule: one
 *               copy of the code, csrc/nn_grid.hpp) over the box of the vertices of the scene's candidate faces.  A face is referenced
 *               from every cell the axis-aligned box of its three vertices overlaps.  A face whose box spans more than MVD_MESH_SPAN
 *               cells along an axis goes to the scene's OVERSIZE list instead, which every query of the scene scans in full before its
 *               walk; every other face has at most MVD_MESH_SPAN^3 references.  The search is exact for any input -- face, region and
 *               every output are the bits MVD_NN_BRUTE gives; a mesh of huge faces only degrades to a brute scan.  Build: box, count,
 *               scan, fill, with integer atomics only; the order of the references differs run to run and the selection does not see it.
 *               MVD_NN_AUTO -- chosen from nf / nscene on the host (csrc/meshdist.hip: kMDGridMinFaces, an interface default).
 *   grid      : cells per axis of MVD_NN_GRID, 1 .. 256, or 0 for the library's choice, a host computation from nf / nscene.
 *   Bounded whatever the data, as mvd_nearest_points is: the shell loop ends at r = grid; ranges and counts read back from the scratch
 *   are clamped, a reference counts only inside the scene's face range, and every face is validated where it is evaluated.
 *   nq, nv, nf <= 2^31 - 1; 1 <= nscene <= 65535; for MVD_NN_GRID nscene * grid^3 <= 2^31 - 1 and nf * MVD_MESH_SPAN^3 <= 2^31 - 1.
 *   nq = 0 and nf = 0 are valid calls (query may be NULL with nq = 0, faces with nf = 0, vertices with nv = 0).  All pointers 4-byte
 *   aligned.
 *   scratch   : mvd_nearest_on_mesh_scratch(nf, nscene, method, grid) bytes, 16-byte aligned -- a function of these four alone; 0 bytes
 *               (NULL allowed) for MVD_NN_BRUTE; the function returns 0 for an argument out of range.
 *   Enqueued on the caller's stream with no host synchronisation and no allocation; every argument is checked before anything is
 *   enqueued, a refused call writes nothing; every scratch word that is read is written earlier in the same call.
 * mvd_nearest_on_mesh_stages: the same call restricted to `stages` (MVD_NN_BUILD -- nothing for MVD_NN_BRUTE --, MVD_NN_QUERY), for
 *   timing the two or for several query sets against one built grid (same vertices, faces, face_start, nf, nscene, method, grid).
 *
 * mvd_mesh_icp: mvd_plane_icp's loop with this search as its correspondence.  MVD_NN_BUILD once over the mesh; iters times { apply
 *   transform to the ORIGINAL source -> moved; MVD_NN_QUERY of moved -> face, dist2, point, normal; the fit of mvd_plane_fit on the pairs
 *   (moved[i], point[i], normal[i]) -- target = point, normals = normal, index == NULL, this dist2 --; history row k }; then a last
 *   apply, query and row (iters) without a step.  No arithmetic is added: the sums, the solve, the gate max_dist2, the row layout
 *   (MVD_PLANE_HISTORY) and the refusal of a zero normal (a degenerate face takes no part) are mvd_plane_fit's, so the result equals,
 *   bit for bit, the same sequence issued by the caller through mvd_align_apply, mvd_nearest_on_mesh_stages and mvd_plane_fit.
 *   transform (nscene, 12) holds the start on entry and the result on return; history is (iters + 1, nscene, 4); moved (nq, 3), face
 *   (nq,), dist2 (nq,), point (nq, 3), normal (nq, 3) are all required with nq > 0 and are left as the last pass wrote them.
 *   0 <= iters <= MVD_ALIGN_MAX_ITERS.  scratch: mvd_mesh_icp_scratch(nq, nf, nscene, method, grid) bytes, 16-byte aligned (0 for an
 *   argument out of range).  Enqueue-only, checked before the first enqueue, as the sections above. */
#define MVD_MESH_SPAN 3
size_t mvd_nearest_on_mesh_scratch(size_t nf, int nscene, int method, int grid);
int mvd_nearest_on_mesh(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start, size_t nq,
                        size_t nv, size_t nf, int nscene, int method, int grid, int* face, float* dist2, float* point, float* bary,
                        int* region, float* normal, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_nearest_on_mesh_stages(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start,
                               size_t nq, size_t nv, size_t nf, int nscene, int method, int grid, int* face, float* dist2, float* point,
                               float* bary, int* region, float* normal, void* scratch, size_t scratch_bytes, int stages,
                               mvd_stream_t stream);
size_t mvd_mesh_icp_scratch(size_t nq, size_t nf, int nscene, int method, int grid);
int mvd_mesh_icp(const float* source, const int* source_start, const float* vertices, const int* faces, const int* face_start, size_t nq,
                 size_t nv, size_t nf, int nscene, int method, int grid, int iters, float max_dist2, double* transform, double* history,
                 float* moved, int* face, float* dist2, float* point, float* normal, void* scratch, size_t scratch_bytes,
                 mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Global registration: the start ICP needs.  H pose hypotheses per scene are scored by the truncated squared distance of a sample of the
 * source to its nearest target points, and K distinct best are picked for refinement (csrc/register.hip; host: mvdfusion_amd/fusion.py
 * register_geometry, rotation_grid).  Not in the reference either.
 *
 * mvd_register_score:
 *   sample (ns, 3) fp32 with sample_start, target (nt, 3) fp32 with target_start: scenes as in mvd_nearest_points (nscene + 1 int32 DEVICE
 *   offsets, clamped before they index anything).  hyp (nscene, H, 12) fp64: per scene and hypothesis a transform in mvd_align_apply's
 *   layout.  Per (scene s, hypothesis h, sample row i of the scene):
 *     p  = sample[i] under hyp[s][h] by THE apply rule of mvd_align_apply: fp64 in its operation order, one cast to fp32.
 *     d2 = dist2 of mvd_nearest_points for the query p among the scene's targets: the least (dx * dx + dy * dy) + dz * dz in fp32 under
 *          the strict comparison, +inf when nothing is found (no target in the scene, a non-finite p).
 *     The row is an INLIER when d2 <= trunc2, compared in fp32 (a NaN compares false); its cost c is d2 for an inlier, else trunc2.
 *   score[s][h] = sum (double)c over the rows of scene s, reduced exactly as MVD_ALIGN_SUMS are: chunks of MVD_ALIGN_CHUNK rows counted from
 *   the scene's first row, thread t of a workgroup its rows t, t + 256, .. in order, the lanes of a wavefront in an xor butterfly, the four
 *   wavefronts as (w0 + w1) + (w2 + w3), the chunk sums added in ascending chunk order.  No float atomics: the same bits run to run, and
 *   for a scene alone and inside a batch.  inliers[s][h]: the count, int32.  A row of no scene contributes nothing; a scene without rows
 *   scores 0.  Nothing per row is written: there is no H x ns array.
 *   method, grid: those of mvd_nearest_points, resolved by the same host rule from nt / nscene.  MVD_NN_GRID walks the grid that
 *   mvd_nearest_points_stages(.., MVD_NN_BUILD) left in the HEAD of `scratch` -- call it with this scratch pointer and the same target,
 *   target_start, nt, nscene, method and grid before the first score; any number of scores may follow one build.  The walk holds
 *   min(best, trunc2) against its bound, so it ends as soon as no unvisited cell can hold a target within the truncation; c and the
 *   inlier bit are those of the full search (csrc/register.hip has the argument).  MVD_NN_BRUTE scans the scene's targets through LDS
 *   and gives the same bits.
 *   trunc2 finite and > 0.  1 <= H <= MVD_REGISTER_MAX_H.  ns, nt <= 2^31 - 1.
 *   scratch: mvd_register_scratch(ns, nt, nscene, H, method, grid) bytes, 16-byte aligned; its first
 *   mvd_nearest_points_scratch(nt, nscene, method, grid) bytes are the search's scratch, whatever ns and H.  0 for an argument out of range.
 *
 * mvd_register_select: per scene, K <= MVD_REGISTER_MAX_K distinct best of H hypotheses.  score (nscene, H) fp64; quat (H, 4) fp64 unit
 *   quaternions, shared by all scenes.  K rounds: (1) take the live h with the lowest (score, h): the lower score, between equal scores
 *   the lower h; a NaN score is never live, +inf is.  (2) kill h and every h' with |q_h . q_h'| >= cos_half, the product formed in fp64 as
 *   ((q0 q0' + q1 q1') + q2 q2') + q3 q3' without contraction.  cos_half = cos(angle / 2) suppresses the rotations within `angle` of a
 *   winner; cos_half > 1 suppresses nothing and the result is the plain top K.  top (nscene, K) int32: h, or -1 once nothing is live;
 *   top_score (nscene, K) fp64: its score, +inf for -1.  One workgroup per scene; H <= MVD_REGISTER_MAX_H.
 *
 * Both are enqueued on the caller's stream with no host synchronisation and no allocation.  Every argument is checked before anything is
 * enqueued -- a NULL pointer, a misaligned one (8 bytes for fp64, 4 otherwise, 16 for the scratch), an argument out of range, a scratch
 * too small, a trunc2 that is not finite and positive, a NaN cos_half -- and a refused call returns non-zero with its name in
 * mvd_last_error() and writes nothing. */
#define MVD_REGISTER_MAX_H 16384
#define MVD_REGISTER_MAX_K 32
size_t mvd_register_scratch(size_t ns, size_t nt, int nscene, int H, int method, int grid);
int mvd_register_score(const float* sample, const int* sample_start, const float* target, const int* target_start, size_t ns, size_t nt,
                       int nscene, int H, const double* hyp, float trunc2, int method, int grid, double* score, int* inliers, void* scratch,
                       size_t scratch_bytes, mvd_stream_t stream);
int mvd_register_select(const double* score, const double* quat, int nscene, int H, int K, double cos_half, int* top, double* top_score,
                        mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Volumetric fusion: the sampled RGB-D views integrated into a truncated signed distance volume (TSDF), and a watertight indexed triangle
 * mesh with vertex colours extracted from it by marching tetrahedra (csrc/tsdf.hip, csrc/tsdf_mesh.hpp; host: mvdfusion_amd/fusion.py
 * integrate_tsdf, extract_mesh).  Not in the reference either.  Cameras, projection, depth map and depth lookup are those of the point
 * fusion above (one copy of each in the source, csrc/fusion_common.hpp).
 *
 * The integrate call:
 *   lat (nscene*V, 5, S, S), rgb (nscene*V, 3, P, P) or NULL with P = S * up, cams (nscene*V, MVD_CAM_RECORD) as for the point fusion.
 *   Volume    : G^3 voxels per scene, arrays (nscene, G, G, G) in z, y, x order (x fastest).  The world box is center +- half_extent
 *               (cx, cy, cz, half_extent: host floats, one box for all scenes).  With vs = 2 * half_extent / G in fp32, voxel (k, j, i)
 *               has its centre at X = ((cx - half_extent) + (i + 0.5) * vs, (cy - half_extent) + (j + 0.5) * vs,
 *               (cz - half_extent) + (k + 0.5) * vs), evaluated in fp32 as written.
 *   View rule : views v = 0 .. V-1 of the voxel's scene in that order.  (u, w, zc) = NDC and camera-space z of X exactly as the point
 *               fusion's pair rule computes them.  Skipped unless zc > 0, |u| <= 1 and |w| <= 1 (a NaN: skipped).  Depth lookup as in the
 *               pair rule: ix = clamp((1 - u) * S / 2 - 0.5, 0, S - 1), iy alike, taps x0 = floor(ix), x1 = min(x0 + 1, S - 1), y alike,
 *               dn = clamp((lat + 1) / 2, 0, 1) per tap, a tap is foreground iff lo < dn < hi, zs = the bilinear mix of
 *               dn * depth_scale + depth_shift in the pair rule's evaluation order.
 *                 four foreground taps : sdf = zs - zc.  sdf < -trunc: the voxel is hidden behind the surface view v sees -- skipped.
 *                                        Else the observation d = min(1, sdf / trunc).
 *                 four background taps : with carve != 0 the observation d = 1 (free space in front of nothing); carve == 0: skipped.
 *                 mixed taps (a silhouette): skipped.
 *   Outputs   : weight (nscene, G, G, G) uint8 = the number of observations (1 <= V <= 255); tsdf fp32 = (sum of d in view order) /
 *               weight, and exactly 1.0f where weight == 0.  With rgb: the observations with four foreground taps and |sdf| <= trunc
 *               also sample rgb of view v bilinearly at (u, w) -- the same pixel-centre lookup at side P, border clamp, the same mix
 *               per channel; color (nscene, G, G, G, 3) fp32 = their mean in view order, cweight uint8 = their number, the mean is 0
 *               where cweight == 0.  rgb NULL: color and cweight are not touched and may be NULL.
 *   One thread per voxel sums its views in order: no atomics, the same bits run to run.  All fp32, compiled without contraction.
 *   Refused   : G outside [2, 256]; 7 * nscene * G^3 >= 2^31; trunc <= 0; half_extent <= 0 (NaN included); lo >= hi; V outside [1, 255];
 *               nscene outside [1, 65535]; S < 2; up < 1; S * up > 46340.
 *
 * The mesh calls: marching tetrahedra over a volume (tsdf, weight as above; any caller-made volume will do).
 *   Cells     : the cube between voxel centres (k..k+1, j..j+1, i..i+1), (G-1)^3 per scene, split into the six Kuhn tetrahedra around
 *               its main diagonal: tetrahedron q = 0 .. 5 follows the axis permutation (a, b, c) = xyz, xzy, yxz, yzx, zxy, zyx and has
 *               the corners v0, v0 + e_a, v0 + e_a + e_b, v0 + (1,1,1).  The split is the same in every cell, so neighbours agree on
 *               their shared faces and the surface is closed wherever the volume is observed.
 *   Edges     : a lattice edge belongs to its lower corner; a corner owns the 7 directions (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1),
 *               (0,1,1), (1,1,1) in (x, y, z); edge number e = ((scene*G^3 + (k*G + j)*G + i) * 7 + direction.  Edges that leave the
 *               grid do not exist.  A voxel is observed iff weight > 0, inside iff observed and tsdf < 0 (zero is outside).
 *   Vertices  : an edge carries a vertex iff both ends are observed and exactly one is inside.  With a the inside end, b the other:
 *               t = d_a / (d_a - d_b) in fp32 (the denominator is never 0) and position x_a + t * (x_b - x_a) per axis from the voxel
 *               centres above.  Colour: c_a + t * (c_b - c_a) when both ends have cweight > 0, the one available colour when one has,
 *               `fill` (3 host floats) when neither has.  The vertex id is the rank of its edge among the carrying edges of the whole
 *               call in edge-number order: ids are global, scene s owns [vertex_start[s], vertex_start[s + 1]).
 *   Triangles : a tetrahedron emits only when its four corners are observed.  One or three corners inside: 1 triangle; two: a quad cut
 *               into 2 triangles along the diagonal through its smallest vertex id.  Every triangle is wound so that its normal points
 *               from inside to outside and rotated so that its smallest vertex id comes first.  Of a quad wound (m, n1, n2, n3) with m
 *               its smallest id, the FIRST triangle is (m, n1, n2) and the second (m, n2, n3).  Faces are ordered by (scene, cell k, j,
 *               i, tetrahedron, triangle); scene s owns [face_start[s], face_start[s + 1]).  A corner with tsdf == 0 is outside and
 *               puts the vertices of its crossing edges on itself (t = 1): such triangles are DEGENERATE (zero area) but are emitted,
 *               so the surface stays closed.
 *   The count call flags the edges and ranks them (wavefront ballots, block counts, the single-workgroup carry scan of the point
 *               compaction: no atomic decides an order), writes the dense int32 map edge -> vertex id (-1: no vertex) to scratch,
 *               counts and scans the triangles per cell, and writes vertex_start and face_start ((nscene + 1) int32 each, DEVICE).
 *               Blocks are padded per scene: none straddles scenes.  The host reads those 2 (nscene + 1) values and allocates.
 *   The emit call writes vertices (nvert, 3) fp32, colors (nvert, 3) fp32 (with color and cweight non-NULL; all three NULL: no
 *               colour), faces (nface, 3) int32 from the SAME scratch; nvert = vertex_start[nscene] and nface = face_start[nscene] as read
 *               by the host -- ids beyond them are not written.
 *   mvd_mesh_scratch(nscene, G): the bytes of scratch (edge map, block counts, per-cell face offsets); 4-byte aligned; 0 for arguments
 *               the calls refuse: G outside [2, 256], nscene outside [1, 65535], 7 * nscene * G^3 >= 2^31 or 12 * nscene * (G-1)^3 >= 2^31
 *               (the most faces there can be). */
int mvd_tsdf_integrate(const float* lat, const float* rgb, const float* cams, float* tsdf, uint8_t* weight, float* color, uint8_t* cweight,
                       int nscene, int V, int S, int up, int G, float cx, float cy, float cz, float half_extent, float trunc, int carve,
                       float depth_scale, float depth_shift, float lo, float hi, mvd_stream_t stream);
size_t mvd_mesh_scratch(int nscene, int G);
int mvd_mesh_count(const float* tsdf, const uint8_t* weight, int nscene, int G, int* vertex_start, int* face_start, void* scratch,
                   size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_emit(const float* tsdf, const uint8_t* weight, const float* color, const uint8_t* cweight, int nscene, int G, float cx, float cy,
                  float cz, float half_extent, const float* fill, float* vertices, float* colors, int* faces, size_t nvert, size_t nface,
                  const void* scratch, size_t scratch_bytes, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh topology: what lies between extracting a mesh and handing it on -- the vertex -> face incidence table, connected components, a
 * topology report, a face filter (the floater remover), area-weighted vertex normals and Taubin smoothing (csrc/meshtopo.hip; host:
 * mvdfusion_amd/fusion.py mesh_components, mesh_topology, filter_mesh, keep_components, vertex_normals, smooth_mesh).  Not in the
 * reference either.
 *
 * The mesh is that of mvd_mesh_emit / mvd_render_mesh / mvd_nearest_on_mesh: vertices (nv, 3) fp32, faces (nf, 3) int32 GLOBAL ids,
 * vertex_start and face_start nscene + 1 int32 DEVICE values each, non-decreasing, clamped to [0, nv] or [0, nf] before they index
 * anything.  Face f belongs to the scene s with face_start[s] <= f < face_start[s + 1].
 *   Face classes: INVALID -- a face of no scene, or one with an id outside [vertex_start[s], vertex_start[s + 1]) of its own scene; it
 *               takes no part in anything, is counted, and has the face label -1.  REPEATED -- a valid face with two equal ids; it
 *               joins its vertices into one component and is counted, but has no edges, no incidence entries, no normal and no umbrella
 *               contribution.  REGULAR -- every other face; a zero-area face with three distinct ids (the marcher emits them at
 *               tsdf == 0) is regular.  No entry reads a coordinate to classify a face.
 *
 * mvd_mesh_incidence: the CSR table vertex -> (face, corner) of the REGULAR faces.  inc_start (nv + 1) int32: the list of vertex v is
 *   inc[inc_start[v] .. inc_start[v + 1]); inc (3 nf) int32: entries face * 3 + corner in ASCENDING order within a list, that is in
 *   ascending (face, corner) order; inc_start[nv] entries are written, the rest of inc is not touched.  Count (an integer atomic per
 *   corner), the exclusive scan of the searches' grids (csrc/nn_grid.hpp around the single-workgroup scan of the point compaction), fill
 *   (an integer atomic hands out the slot) and an insertion sort of every list in place by one thread: the sorted table does not depend
 *   on the arrival order, so it has the same bits run to run.  A list has no bound but 3 nf; the sort costs O(d^2) for a vertex of
 *   valence d.
 * mvd_mesh_label: connected components.  Two valid faces are connected when they share a vertex id, transitively; a scene's faces name
 *   only its own vertices, so a component never crosses scenes.  Per vertex the LABEL is the smallest vertex id of its component -- a
 *   unique answer, so no race can change it.  A component is NUMBERED iff it has a face, and its compact id is the rank of its label among
 *   the labels of the numbered components: components are numbered scene after scene, in the order of their smallest vertex.
 *     vertex_component (nv,) int32: the compact id, -1 for a vertex no valid face uses.  face_component (nf,) int32: the compact id, -1
 *     for an invalid face.  component_start (nscene + 1) int32: scene s owns the ids [component_start[s], component_start[s + 1]).
 *   Lock-free union-find: parent[v] = v, one thread per face hooks the larger root under the smaller by atomicCAS and halves paths by
 *   atomicMin, a flatten pass, a scan of the root flags.  BOUNDS: parent[v] <= v holds from initialisation and across every write and a
 *   word only decreases, so a find is a strictly descending walk of at most nv steps whatever the memory holds; a hook is retried only
 *   after ANOTHER thread lowered the same word and goes on from the lower value, so the larger of its two roots strictly decreases: at
 *   most nv attempts.  Both loops also carry nv as an explicit cap.  No thread waits for another, nothing is persistent or cooperative,
 *   and the host issues a fixed sequence of launches.
 * mvd_mesh_component_table: after the host read component_start[nscene] = ncomp: root (ncomp,) int32 the label, faces (ncomp,) and
 *   vertices (ncomp,) int32 the valid faces and used vertices per component.  Integer atomics (counts and a minimum); ids outside
 *   [0, ncomp) are not counted.
 * mvd_mesh_topology: takes the table of mvd_mesh_incidence and vertex_component, component_start of mvd_mesh_label for the same mesh.
 *   An EDGE is an unordered pair of ids that a regular face has at consecutive corners (corner 2 is followed by corner 0); its USERS are
 *   the regular faces that contain both ids.  Per face and edge the incidence list of the endpoint with the shorter list (the edge's
 *   first id between equal lengths) is walked; the user with the lowest (face, edge number) owns the edge, and only the owner adds to the
 *   totals.  totals (nscene, MVD_TOPO_TOTALS) int32 per scene, in this order:
 *     0 vertices_used (vertex_component >= 0), 1 unreferenced (the scene's other vertices), 2 faces_regular, 3 faces_repeated,
 *     4 faces_invalid (a face of no scene is counted nowhere), 5 edges, 6 boundary_edges (one user), 7 nonmanifold_edges (more than two),
 *     8 misoriented_edges (two users that run along the edge in the same direction), 9 components,
 *     10 euler = vertices_used - edges + faces_regular.
 *   vertex_flags (nv,) uint8: MVD_TOPO_FLAG_BOUNDARY -- on a boundary edge; MVD_TOPO_FLAG_NONMANIFOLD -- on a non-manifold edge.  The bits
 *   are gathered by integer atomicOr on 32-bit words of the scratch and narrowed by the thread that owns the vertex: no byte is read,
 *   modified and written back.  Integer atomics only: the same bits run to run.  A vertex of valence d costs O(d^2) here: fine for a
 *   marched mesh (d <= 14 or so), a limit for a caller's mesh with a huge fan.
 * mvd_mesh_filter_count / _emit: the faces f with keep[f] != 0 (keep (nf,) uint8) that are not invalid survive, in their order; the
 *   vertices they name survive, in their order; ids are rebased.  The count call flags (plain stores of one value), scans twice and
 *   writes new_vertex_start and new_face_start ((nscene + 1) int32 each, DEVICE); the host reads those 2 (nscene + 1) values, allocates,
 *   and the emit call -- same nv, nf and scratch -- writes out_vertices (nvo, 3), out_rgb (nvo, 3) (with rgb non-NULL; both NULL: no
 *   colour) bit for bit, out_faces (nfo, 3), and the old rows vertex_index (nvo,), face_index (nfo,); rows beyond nvo / nfo are not
 *   written.
 * mvd_mesh_vertex_normals: per vertex the fp64 sum, over its incidence list in list order, of the raw cross products n = ab x ac of the
 *   faces (ab = B - A, ac = C - A from the face's own corner order; each component one subtraction of two products, n_x = ab_y ac_z -
 *   ab_z ac_y, ... as mvd_nearest_on_mesh forms its normal) -- area weighting -- divided by its length sqrt((s_x s_x + s_y s_y) + s_z s_z)
 *   and rounded once to fp32; 0 where that length is 0 or not finite or the list is empty.  normals (nv, 3) fp32.
 * mvd_mesh_smooth: `passes` umbrella passes whose factor f alternates lam, mu, lam, .. (Taubin).  Per vertex and pass, from the
 *   positions x of the previous pass: S = the fp64 sum per axis, over the incidence list in list order, of the two OTHER vertices of the
 *   face, the next corner and then the previous one (so an interior neighbour is met twice and a boundary neighbour once: the stated
 *   rule); c = the number of terms; x' = fp32(x + f * (S / c - x)) in fp64 in exactly this order, without contraction.  The vertex is
 *   copied unchanged when c == 0, when a coordinate it would read (its own or a neighbour's) is not finite, or when
 *   vertex_flags[v] & pin_mask != 0 (pin_mask 0: nothing is pinned and vertex_flags may be NULL).  Positions go back and forth between
 *   `out` and `tmp` ((nv, 3) fp32 each, distinct from `vertices`, which is only read) such that the last pass writes `out`; passes == 0
 *   copies; tmp may be NULL for passes < 2.  0 <= passes <= MVD_SMOOTH_MAX_PASSES; lam and mu finite.
 *
 * For all of them: nv <= 2^31 - 1 - 4096, 3 nf <= 2^31 - 1, 1 <= nscene <= 65535; nv = 0 and nf = 0 are valid calls (a pointer to an
 * array without elements may be NULL).  Pointers 4-byte aligned (uint8 arrays: any), the scratch 16-byte aligned.  Every index read
 * back from inc_start, inc or the scratch is clamped or range-checked before it addresses anything.  Scratch sizes: mvd_mesh_*_scratch(nv,
 * nf) bytes, 0 for an argument out of range, never 0 otherwise; mvd_mesh_filter_scratch serves both filter calls;
 * mvd_mesh_component_table, mvd_mesh_vertex_normals and mvd_mesh_smooth take no scratch.  Enqueued on the caller's stream with no host
 * synchronisation and no allocation; every argument is checked before anything is enqueued, a refused call returns non-zero with its name
 * in mvd_last_error() and writes nothing; every scratch word that is read is written earlier in the same call (the emit call reads what
 * the count call wrote). */
#define MVD_TOPO_TOTALS 11
#define MVD_TOPO_FLAG_BOUNDARY 1
#define MVD_TOPO_FLAG_NONMANIFOLD 2
#define MVD_SMOOTH_MAX_PASSES 2000
size_t mvd_mesh_incidence_scratch(size_t nv, size_t nf);
int mvd_mesh_incidence(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene, int* inc_start,
                       int* inc, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
size_t mvd_mesh_label_scratch(size_t nv, size_t nf);
int mvd_mesh_label(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene, int* vertex_component,
                   int* face_component, int* component_start, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_component_table(const int* vertex_component, const int* face_component, size_t nv, size_t nf, size_t ncomp, int* root, int* faces,
                             int* vertices, mvd_stream_t stream);
size_t mvd_mesh_topology_scratch(size_t nv, size_t nf);
int mvd_mesh_topology(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene, const int* inc_start,
                      const int* inc, const int* vertex_component, const int* component_start, int* totals, uint8_t* vertex_flags,
                      void* scratch, size_t scratch_bytes, mvd_stream_t stream);
size_t mvd_mesh_filter_scratch(size_t nv, size_t nf);
int mvd_mesh_filter_count(const int* faces, const uint8_t* keep, const int* vertex_start, const int* face_start, size_t nv, size_t nf,
                          int nscene, int* new_vertex_start, int* new_face_start, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_filter_emit(const float* vertices, const float* rgb, const int* faces, size_t nv, size_t nf, float* out_vertices, float* out_rgb,
                         int* out_faces, int* vertex_index, int* face_index, size_t nvo, size_t nfo, const void* scratch,
                         size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_vertex_normals(const float* vertices, const int* faces, const int* inc_start, const int* inc, size_t nv, size_t nf,
                            float* normals, mvd_stream_t stream);
int mvd_mesh_smooth(const float* vertices, const int* faces, const int* inc_start, const int* inc, const uint8_t* vertex_flags, size_t nv,
                    size_t nf, int passes, double lam, double mu, int pin_mask, float* out, float* tmp, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh simplification: vertex clustering (Rossignac-Borrel) with Lindstrom's quadric placement (csrc/meshsimplify.hip; host:
 * mvdfusion_amd/fusion.py simplify_mesh).  Every vertex of a cubic cell becomes one vertex; a face survives when its three vertices
 * fall into three cells.  Data-parallel, with a unique answer.  Not in the reference either.
 *
 * The mesh arrays, the face classes and the conventions are those of the mesh topology section above.  The call sequence is
 *   mvd_mesh_incidence(faces) -> mvd_mesh_cluster_count -> host reads cluster_start[nscene] = nc -> mvd_mesh_cluster_emit ->
 *   mvd_mesh_incidence(mapped_faces, cluster_start as the vertex offsets, nv = nc) -> mvd_mesh_cluster_dedupe ->
 *   mvd_mesh_filter_count / _emit(out_vertices, out_rgb, mapped_faces, the second keep mask, cluster_start, nv = nc),
 * and the filter pair drops the clusters no surviving face names and rebases the ids.
 *
 * mvd_mesh_cluster_count.  A MEMBER is a vertex of a scene with three finite coordinates and a non-empty list in the table of
 *   mvd_mesh_incidence (inc_start (nv + 1) is an input; only the list lengths are read).
 *   Box     : per scene lo_a, hi_a = the least and the greatest fp32 coordinate of its members per axis (integer atomicMin on the
 *             order-preserving keys of the searches' grids, the greatest as the minimum of the complemented key).
 *   Grid    : fp64 from here on.  extent_a = hi_a - lo_a; h = (the greatest extent_a) / cells.  With h > 0: n_a = clamp(floor(extent_a /
 *             h) + 1, 1, cells) and a member's cell along axis a is i_a = clamp(floor((x_a - lo_a) / h), 0, n_a - 1), in exactly this
 *             order, without contraction; with h == 0 (or in a scene without a member) n_a = 1 and every member has the cell 0.  The
 *             linear id is (i_z n_y + i_y) n_x + i_x.
 *   Clusters: occupied cells are flagged by plain stores of one value into a dense table of cells^3 words per scene (nscene * cells^3
 *             <= 2^28), the table is scanned (the exclusive scan of the searches' grids), and a cluster's id is the rank of its
 *             (scene, linear id): clusters are numbered scene after scene, in cell order.
 *   vertex_cluster (nv,) int32: the id, -1 for a vertex that is no member.  cluster_start (nscene + 1) int32 DEVICE: scene s owns the
 *   ids [cluster_start[s], cluster_start[s + 1]); the host reads cluster_start[nscene] = nc.  The call also counts the members per
 *   cluster (an integer atomic each) and scans the counts: box, nc and these list offsets stay in the scratch for the emit call.
 * mvd_mesh_cluster_emit: same nv, nf, nscene, cells and scratch as the count call, vertex_cluster as it wrote it, inc_start and inc of
 *   the same mesh.
 *   Lists   : the cluster -> member lists, ASCENDING by vertex id.  Fill (an integer atomic hands out the slot), then a rank pass: every
 *             member counts the smaller ids of its own list and stores itself at that position.  COST: a member of a list of length L
 *             reads L words, so a list costs L^2 reads spread over L threads, O(L) per thread; no thread is quadratic (the insertion
 *             sort of mvd_mesh_incidence would be: a cluster of a 128^3 mesh at cells = 8 holds thousands of vertices).
 *   Vertex  : per member (one thread, fp64, incidence-list order), over the faces of its list that name only finite vertices: the raw
 *             cross product n = ab x ac formed exactly as mvd_mesh_vertex_normals forms it; l = sqrt((n_x n_x + n_y n_y) + n_z n_z); a
 *             face with l == 0 or l not finite is skipped; u = n / l per component, w = l / 2, d = (u_x a_x + u_y a_y) + u_z a_z with a
 *             the face's first corner.  Sums, one add per face each: A_v = sum (w u_r) u_c for (r, c) = xx xy xz yy yz zz and
 *             g_v = sum (w u_r) d.
 *   Cluster : per cluster (one thread, ascending members): c = the count; m = (sum x) / c per axis; rgb = (sum rgb) / c rounded once
 *             to fp32; A = sum A_v, g = sum g_v; b_r = ((A_rx m_x + A_ry m_y) + A_rz m_z) - g_r, the gradient of the quadric at m up to
 *             a factor of 2.
 *             placement MVD_SIMPLIFY_MEAN: x = fp32(m), rank = 0, placed = MVD_SIMPLIFY_PLACED_MEAN.
 *             placement MVD_SIMPLIFY_QUADRIC: the cyclic Jacobi of mvd_point_normals (MVD_NORMALS_SWEEPS sweeps, csrc/jacobi3.hpp) on
 *             A gives lambda_i and e_i (column i); rank = the number of i with lambda_i > MVD_SIMPLIFY_RANK_RATIO * lambda_max
 *             (Lindstrom's threshold; 0 when lambda_max is not positive and finite); y = m, then for i = 0, 1, 2 if kept:
 *             t = ((e_ix b_x + e_iy b_y) + e_iz b_z) / lambda_i, y_a = y_a - t e_ia.  y is ACCEPTED when rank > 0, it is finite and
 *             (lo_a + i_a h) - h / MVD_SIMPLIFY_BOX_SLACK_DIV <= y_a <= (lo_a + (i_a + 1) h) + h / MVD_SIMPLIFY_BOX_SLACK_DIV on every
 *             axis, i the cluster's cell (a corner of the scene's box lies exactly on its cell's outer face and the solve lands 1e-16
 *             beside it: hence the slack).  Accepted: x = fp32(y), placed = MVD_SIMPLIFY_PLACED_QUADRIC; otherwise x = fp32(m),
 *             placed = MVD_SIMPLIFY_PLACED_FALLBACK.
 *   Faces   : mapped_faces (nf, 3) int32: the cluster ids of the face's vertices (ids of the OUTPUT, global), -1 for a vertex that is no
 *             member and for every id of an invalid face; keep (nf,) uint8: 1 iff the face is regular, its three vertices are members
 *             and its three cluster ids are distinct.
 *   out_vertices (nc, 3) fp32, out_rgb (nc, 3) fp32 (with rgb non-NULL; both NULL: no colour), size, rank, placed (nc,) int32.
 *   nc is compared ON THE DEVICE with the count the count call left in the scratch: when they differ, no kernel of the call writes
 *   anything, neither outputs nor scratch.  The host cannot know without a synchronisation, so that call returns 0.
 * mvd_mesh_cluster_dedupe: takes mvd_mesh_incidence of mapped_faces.  A kept face walks the list of its smallest id and loses its
 *   keep when a LOWER face row with keep set names the same unordered id set: the lowest row of a set survives (Open3D's rule; a sheet
 *   thinner than a cell loses one of its two sides).  The rule depends on the emit call's keep only, which is read; the result goes to
 *   keep_out (nf,) uint8, a second buffer.
 *
 * 1 <= cells <= MVD_SIMPLIFY_MAX_CELLS.  Scratch: mvd_mesh_cluster_scratch(nv, nf, nscene, cells) bytes serve the count and the emit
 * call, 16-byte aligned; 0 for an argument out of range, never 0 otherwise.  Everything else as for the mesh topology section: sizes,
 * alignment, empty meshes, clamped reads, no host synchronisation, every argument checked before anything is enqueued, a refused call
 * writes nothing and names itself in mvd_last_error(), every scratch word that is read is written earlier in the same call (the emit
 * call reads what the count call wrote).  Integer atomics only: the same bits run to run, and for a scene alone or in a batch. */
#define MVD_SIMPLIFY_MAX_CELLS 256
#define MVD_SIMPLIFY_MEAN 0
#define MVD_SIMPLIFY_QUADRIC 1
#define MVD_SIMPLIFY_PLACED_MEAN 0
#define MVD_SIMPLIFY_PLACED_QUADRIC 1
#define MVD_SIMPLIFY_PLACED_FALLBACK 2
#define MVD_SIMPLIFY_RANK_RATIO 1e-3
#define MVD_SIMPLIFY_BOX_SLACK_DIV 1024
size_t mvd_mesh_cluster_scratch(size_t nv, size_t nf, int nscene, int cells);
int mvd_mesh_cluster_count(const float* vertices, const int* vertex_start, const int* inc_start, size_t nv, size_t nf, int nscene, int cells,
                           int* vertex_cluster, int* cluster_start, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_cluster_emit(const float* vertices, const float* rgb, const int* faces, const int* vertex_start, const int* face_start,
                          const int* inc_start, const int* inc, const int* vertex_cluster, size_t nv, size_t nf, int nscene, int cells,
                          int placement, size_t nc, float* out_vertices, float* out_rgb, int* size, int* rank, int* placed, int* mapped_faces,
                          uint8_t* keep, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_mesh_cluster_dedupe(const int* mapped_faces, const uint8_t* keep, const int* inc_start, const int* inc, size_t nc, size_t nf,
                            uint8_t* keep_out, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Inside or outside a mesh: the generalized winding number (Jacobson, Kavan, Sorkine-Hornung 2013) of a triangle mesh at every query
 * point (csrc/winding.hip; host: mvdfusion_amd/fusion.py winding_number, signed_distance, voxelize_mesh, volume_iou).  Not in the
 * reference either.  It is the sum over the faces of the signed solid angle seen from the query, divided by 4 pi: an integer for a
 * closed oriented mesh (1 inside a mesh whose normals point out, as mvd_mesh_emit winds them) and a smooth function otherwise, so it
 * degrades gracefully on the open and non-manifold meshes the mesh filter and the simplification can leave, where ray parity does not.
 *
 * mvd_winding_number:
 *   Inputs, scenes, clamping of the two start tables, pointer alignment and size limits are those of mvd_nearest_on_mesh: query (nq, 3)
 *   fp32; vertices (nv, 3) fp32; faces (nf, 3) int32 GLOBAL rows; query_start, face_start nscene + 1 int32 DEVICE values each, clamped to
 *   [0, nq] or [0, nf]; query i of scene s sees the faces f with face_start[s] <= f < face_start[s + 1].
 *   Candidates: a face whose three ids lie in [0, nv), whose nine coordinates are finite and whose fp64 normal n = (B - A) x (C - A) has
 *               three components that are not all exactly 0; the components are formed as mvd_nearest_on_mesh forms them, one
 *               subtraction of two products each (n_x = ab_y ac_z - ab_z ac_y, ...).  A face that is no candidate contributes nothing
 *               under either method.
 *   Per pair  : fp64 on the exact conversions of the fp32 inputs, every operation rounded once (compiled without contraction).
 *               dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z.  With q the query: a = A - q, b = B - q, c = C - q; la = sqrt(dot(a, a)),
 *               lb, lc likewise; x = b x c (components as above); num = dot(a, x);
 *               den = (((la lb) lc + dot(a, b) lc) + dot(b, c) la) + dot(c, a) lb.
 *               Omega = 0 when num == 0 (a query in the face's plane: no sign of zero to argue about), else Omega = 2 atan2(num, den)
 *               (Van Oosterom and Strackee 1983).
 *   MVD_WIND_EXACT: S = the sum of Omega over the scene's faces in ascending face row, started from 0.  The value does not depend on
 *               the launch geometry.
 *   MVD_WIND_CELLS(cells, beta): one level of cells with a dipole far field (Barill et al. 2018, first order).
 *     Grid    : per scene the box of the vertices of its candidate faces (integer atomicMin on the order-preserving keys of
 *               mvd_nearest_points), then fp64 by the expressions of the mesh simplification: h = longest extent / cells;
 *               n_k = clamp(floor(extent_k / h) + 1, 1, cells) (1 when h == 0); a face belongs to the cell of its centroid
 *               g = ((A + B) + C) / 3 per axis, cell index clamp(floor((g_k - lo_k) / h), 0, n_k - 1) (0 when h == 0), linear id
 *               (iz n_y + iy) n_x + ix.  1 <= cells <= MVD_WIND_MAX_CELLS and nscene * cells^3 <= 2^28.
 *     Members : the list of a cell ascends by face row (count, scan, fill through an atomic cursor, rank: the pattern of the mesh
 *               simplification).
 *     Moments : per occupied cell over its members ascending, with the weight m_f = sqrt(dot(n_f, n_f)): M = sum m_f;
 *               p = (sum m_f g_f) / M per axis (each term one product); N = 0.5 * sum n_f per axis; rho2 = the maximum over the
 *               members' three vertices X of dot(X - p, X - p).  Every sum starts from 0.
 *     Query   : over the scene's occupied cells in ascending cell id, with d = p - q and r2 = dot(d, d): the cell is FAR iff
 *               r2 > (beta * beta) * rho2 -- strictly, so r2 == 0 is never far; beta * beta is formed once on the host.  A far cell
 *               contributes dot(N, d) / (r2 * sqrt(r2)); a near cell the sum of Omega over its members ascending, started from 0.
 *               S = the sum of the cells' contributions in that order, started from 0.
 *               beta = +inf makes every cell near, beta = 0 every cell with r2 > 0 far.  cells = 1 with beta = +inf gives the bits of
 *               MVD_WIND_EXACT.  The far field's error is a property of this rule, not of the arithmetic: DESIGN.md has it measured.
 *   MVD_WIND_AUTO : chosen from nf / nscene on the host; cells = 0 asks for the library's choice, a host function of nf / nscene
 *               (csrc/winding.hip: kWCellsMinFaces, kWCellsFactor).  Both are INTERFACE defaults from a cost model, not from a sweep.
 *   Outputs   : each optional -- a NULL is not written.  winding (nq,) fp64 (8-byte aligned): w = S / (4.0 * 3.141592653589793);
 *               inside (nq,) uint8: w >= 0.5.  A query with a non-finite coordinate, or of no scene, gets w = NaN, inside = 0; a query
 *               whose scene has no candidate face gets w = 0, inside = 0.
 *   beta >= 0 or +inf; a NaN is refused (MVD_WIND_EXACT checks it too).  nq = 0 and nf = 0 are valid calls.
 *   scratch   : mvd_winding_scratch(nf, nscene, method, cells) bytes, 16-byte aligned -- a function of these four alone; 0 bytes (NULL
 *               allowed) for MVD_WIND_EXACT and wherever MVD_WIND_AUTO resolves to it; the function returns 0 for an argument out of
 *               range.
 *   Enqueued on the caller's stream with no host synchronisation and no allocation; every argument is checked before anything is
 *   enqueued; a refused call writes nothing and names the entry in mvd_last_error(); every scratch word that is read is written
 *   earlier in the same call; everything read back from the scratch is clamped.  Integer atomics only and every fp64 sum in list
 *   order: the same bits run to run, and for a scene alone or inside a batch.
 *   Kernels   : MVD_WIND_EXACT stages resolved face records through LDS in tiles of MVD_WIND_FACE_TILE, one thread per query;
 *               MVD_WIND_CELLS stages the 64-byte occupied-cell records in tiles of MVD_WIND_CELL_TILE and walks a near cell's
 *               resolved 36-byte member records from global memory.
 * mvd_winding_number_stages: the same call restricted to `stages` (MVD_NN_BUILD -- nothing for MVD_WIND_EXACT --, MVD_NN_QUERY), for
 *   timing the two or for several query sets against one built grid (same vertices, faces, face_start, nf, nscene, method, cells).
 *
 * Out of scope: a tree or several levels of cells and higher-order expansions; winding numbers of point clouds; ray casting; mesh
 * volume and area; repairing orientation; hole filling; gradients. */
#define MVD_WIND_AUTO 0
#define MVD_WIND_EXACT 1
#define MVD_WIND_CELLS 2
#define MVD_WIND_MAX_CELLS 64
#define MVD_WIND_FACE_TILE 512
#define MVD_WIND_CELL_TILE 128
size_t mvd_winding_scratch(size_t nf, int nscene, int method, int cells);
int mvd_winding_number(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start, size_t nq,
                       size_t nv, size_t nf, int nscene, int method, int cells, double beta, double* winding, unsigned char* inside,
                       void* scratch, size_t scratch_bytes, mvd_stream_t stream);
int mvd_winding_number_stages(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start,
                              size_t nq, size_t nv, size_t nf, int nscene, int method, int cells, double beta, double* winding,
                              unsigned char* inside, void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Texturing a mesh from views: a per-face atlas, the bake of the views into it and the lookup that brings it back into images
 * (csrc/texture.hip; host: mvdfusion_amd/fusion.py bake_texture, sample_texture, render_mesh(texture=...), write_obj).  Not in the
 * reference either.  A vertex colour of mvd_mesh_emit is about one colour sample per voxel and the simplification averages it again; the
 * decoded views hold several times that detail.  The mesh arrays, scenes and clamping of the start tables are those of mvd_render_mesh.
 *
 * The atlas (closed form: no search, no texel-to-face table, no dilation pass):
 *   T = texels in [1, MVD_TEX_MAX_TEXELS] texel intervals along a chart's legs; a cell is K = T + 3 texels square and holds two faces;
 *   C >= 1 cells per row; the texture is A = C * K texels square, the same A for every scene of a call.  Texel (x, y) has its centre
 *   at the integers (x, y), as a pixel of mvd_render_mesh has.
 *   Cells   : local face l = f - face_start[s] of scene s is half h = l & 1 of cell c = l >> 1, which sits at column c % C, row c / C:
 *             origin (ox, oy) = ((c % C) * K, (c / C) * K).  A face with l >= 2 * C * C has no chart: it is not baked and is looked up
 *             as background.
 *   Corners : of (a, b, c) -- lower half (h = 0): (ox, oy), (ox + T, oy), (ox, oy + T); upper half: the point reflection through the
 *             cell, (ox + K - 1, oy + K - 1), (ox + K - 1 - T, oy + K - 1), (ox + K - 1, oy + K - 1 - T).
 *   Owned   : cell-local (i, j) belongs to the lower face when i <= T, j <= T and i + j <= T + 1; to the upper face when the same test
 *             holds for (i', j') = (K - 1 - i, K - 1 - j); to no face otherwise (the tests exclude each other: i + j <= T + 1 against
 *             i + j >= T + 3), and to no face when its half has l >= the scene's face count.  A face owns (T + 1)(T + 2) / 2 + T
 *             texels: the closed texel triangle and the T texels of the next diagonal, which are exactly the taps of non-zero weight
 *             of a bilinear lookup anywhere in the closed triangle.
 *   Barycentrics of an owned texel, with (i, j) the chart's own indices (mirrored for the upper half): b_b = i / T, b_c = j / T,
 *             b_a = (1 - b_b) - b_c.  On the extra diagonal b_a = -1 / T: the texel extrapolates across the hypotenuse -- the gutter.
 *   mvd_texture_atlas_side(nface_max, texels, nscene) = the smallest such A for scenes of at most nface_max faces:
 *             C = max(1, ceil(sqrt(ceil(nface_max / 2)))) in integers.  0 for what the calls refuse: texels outside its range,
 *             A > MVD_TEX_MAX_SIDE, nscene outside [1, 65535] or nscene * A * A >= 2^31.  The calls take any multiple A of K inside those limits.
 *
 * mvd_texture_bake: one thread per texel of (nscene, A, A).
 *   vertices, colors (or NULL), faces, vertex_start, face_start, nvert, nface, nscene: as mvd_render_mesh takes them.
 *   cams (nscene*V, MVD_CAM_RECORD): camera c = s*V + v is view v of scene s, 1 <= V <= MVD_TEX_MAX_VIEWS; rgb (nscene*V, 3, H, H) fp32
 *   planar: the views; depth (nscene*V, Pd, Pd) fp32: the depth each view sees of the surface -- mvd_render_mesh's `depth` of this mesh
 *   in these cameras, or any other depth map of them (then a consistency gate) --, an empty pixel not finite; Pd need not equal H;
 *   1 <= H, Pd <= 32768.  tol finite >= 0; min_cos in [0, 1); power in [0, 8]; cull 0 or 1; blend MVD_TEX_MEAN / MVD_TEX_BEST;
 *   znear >= 0; fill: 3 floats on the HOST, read at the call.
 *   No face   : a texel that no face owns gets fill, views = 0, best = 255.
 *   No view   : a face with an id outside its scene's vertex range reads no vertex: its texels get fill, views = 0, best = 255.
 *               Otherwise the texel starts from fallback = (b_a c_a + b_b c_b) + b_c c_c per channel from the vertex colours, or fill
 *               with colors NULL.  With n = (B - A) x (C - A) from the world positions (components as mvd_render_mesh forms them) and
 *               nn = (n_0^2 + n_1^2) + n_2^2: a face whose nn is not finite or not > 0 has no contributing view.
 *   Point     : X = (b_a * A + b_b * B) + b_c * C per axis.
 *   Per view v = 0 .. V - 1 ascending, with (u, w) and the camera-space point xc of X exactly as mvd_render_mesh projects a vertex (one
 *               function in the source), zc = xc_2.  View v CONTRIBUTES when all of, in this order:
 *                 - zc > znear; u and w are finite;
 *                 - cx = (1 - u) * (Pd / 2) - 0.5 and cy alike from w lie in [-0.5, Pd - 0.5];
 *                 - d = depth[c, min(floor(cy + 0.5), Pd - 1), min(floor(cx + 0.5), Pd - 1)] is finite and zc <= d + tol.  An empty
 *                   depth pixel is NOT visible: that keeps the background colour off the rim of the object;
 *                 - cosv > min_cos, where n_cam_j = n_0 R[0][j] + n_1 R[1][j] + n_2 R[2][j], dot = (n_cam_0 xc_0 + n_cam_1 xc_1) +
 *                   n_cam_2 xc_2, len = sqrt((xc_0^2 + xc_1^2) + xc_2^2), cosv = -dot / (sqrt(nn) * len), and with cull = 0
 *                   cosv = |cosv|.
 *               Weight: wt = 1, multiplied by cosv `power` times.  Colour: col_k = bilinear_mix(pixel_taps(u, w, H)) of channel k of
 *               view v -- the lookup of mvd_fuse_points, one copy in the source.
 *   Blend     : MVD_TEX_MEAN: sw += wt, sc_k += wt * col_k from 0 in view order; the texel is sc_k / sw.  MVD_TEX_BEST: col of the
 *               largest wt, the lowest view between equal weights.  No contributing view: fallback.
 *   Outputs   : texture (nscene, 3, A, A) fp32 planar; views (nscene, A, A) uint8 = the number of contributing views, or NULL;
 *               best (nscene, A, A) uint8 = the view of the largest wt (under either blend), 255 without one, or NULL.
 *   All fp32, compiled without contraction; no atomics, no scratch, one enqueue on the caller's stream, no host synchronisation.  A
 *   texel is a pure function of its face, its chart indices and its scene's views, and A is common to the scenes of a call: the same
 *   bits run to run, for a scene alone or inside a batch baked at the same A, and with either optional output NULL.  Every argument is
 *   checked before anything is enqueued; a refused call writes nothing and names the entry in mvd_last_error().  nface = 0 is a valid
 *   call.  Workgroups take whole cells and stage the resolved records of their faces in LDS.
 *
 * mvd_texture_sample: one thread per pixel of a mvd_render_mesh result.
 *   face_out (nscene*M, P, P) int32 and bary (nscene*M, 3, P, P) fp32 as mvd_render_mesh wrote them; face_start, nface, nscene, M, P
 *   with its limits; texture (nscene, 3, A, A); texels, A as above; filter; background: 3 floats on the HOST.
 *   A pixel whose f = face_out lies in its scene's face range with l < 2 * C * C gets, with (t_a, t_b, t_c) the corners above,
 *   t = (b_a t_a + b_b t_b) + b_c t_c per axis, clamped to [0, A - 1] (the clamp never moves a point of the chart);
 *   MVD_TEX_NEAREST : the texel (floor(tx + 0.5), floor(ty + 0.5));
 *   MVD_TEX_BILINEAR: x0 = floor(tx), x1 = min(x0 + 1, A - 1), wx = tx - x0, likewise in y; the four taps (y0, x0), (y0, x1), (y1, x0),
 *                     (y1, x1) mixed as (z0 (1 - wx) + z1 wx) (1 - wy) + (z2 (1 - wx) + z3 wx) wy.  A tap whose weight is exactly 0
 *                     (wx == 0 or wy == 0) is not read and enters as 0.
 *   Any other pixel gets background.  rgb (nscene*M, 3, P, P) fp32.  One enqueue; checked as above.
 *
 * Out of scope: unwrapping into charts and seam minimisation (one chart per face is the whole atlas: simplify first); mip-maps and
 * anisotropic filtering; inpainting unseen texels; exposure matching between views; gradients. */
#define MVD_TEX_MEAN 0
#define MVD_TEX_BEST 1
#define MVD_TEX_NEAREST 0
#define MVD_TEX_BILINEAR 1
#define MVD_TEX_MAX_TEXELS 64
#define MVD_TEX_MAX_SIDE 16384
#define MVD_TEX_MAX_VIEWS 254
int mvd_texture_atlas_side(size_t nface_max, int texels, int nscene);
int mvd_texture_bake(const float* vertices, const float* colors, const int* faces, const int* vertex_start, const int* face_start,
                     const float* cams, const float* rgb, const float* depth, size_t nvert, size_t nface, int nscene, int V, int H, int Pd,
                     int texels, int A, float tol, float min_cos, int power, int cull, int blend, float znear, const float* fill,
                     float* texture, unsigned char* views, unsigned char* best, mvd_stream_t stream);
int mvd_texture_sample(const int* face_out, const float* bary, const int* face_start, const float* texture, size_t nface, int nscene, int M,
                       int P, int texels, int A, int filter, const float* background, float* rgb, mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring views against ground truth: squared error / PSNR, SSIM and the depth-error family (csrc/view_metrics.hip; host:
 * mvdfusion_amd/view_metrics.py compare_images, compare_depth, compare_views, ViewFusion.compare).  Not in the reference, which scores
 * its views with library calls.  Everything is accumulated in fp64, compiled without contraction.
 *
 * mvd_image_metrics: a, b (B, C, H, W) fp32 contiguous; mask (B, H, W) uint8 or NULL, non-zero = the pixel counts (NULL: every pixel).
 *   Squared error, per image: count = the number of counted pixels; sq_sum = the sum over counted pixels and all channels of d * d with
 *             d = double(a) - double(b) (exact: only the square rounds).
 *   SSIM      : with weights = `window` doubles on the HOST (read at the call, passed by value into the launch; no transcendental runs
 *             on the device), per (image, channel) plane over the "valid" region of Ho x Wo = (H - window + 1) x (W - window + 1)
 *             window positions, position (r, c) covering pixels (r .. r + window - 1, c .. c + window - 1):
 *               1. the five maps x = double(a), y = double(b), x * x, x * y, y * y (products of two fp32 values: exact);
 *               2. each filtered horizontally: h(r, c) = the sum over k = 0 .. window - 1 ASCENDING of weights[k] * map(r, c + k), from 0.0;
 *               3. each filtered vertically: E(r, c) = the sum over k ascending of weights[k] * h(r + k, c), from 0.0;
 *               4. sxx = E[xx] - mx * mx, sxy = E[xy] - mx * my, syy = E[yy] - my * my with mx = E[x], my = E[y];
 *               5. ssim = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2)), products left to right.
 *             ssim_map (B, C, Ho, Wo) fp64 or NULL.  Position (r, c) COUNTS when mask[b, r + window / 2, c + window / 2] is non-zero (the
 *             mask cropped by window / 2 on each side); ssim_count = the number of counting positions of the image (not times C),
 *             ssim_sum = the sum of ssim over the channels and the counting positions, so the mean SSIM is ssim_sum / (C * ssim_count).
 *             Only + - * / : the map is the same bits wherever these operations round correctly.
 *             weights NULL: no SSIM; window, c1, c2 are not looked at and ssim_sum, ssim_count, ssim_map are not written.
 *   A pixel that is not finite enters the sums it belongs to like any other: under the mask it makes sq_sum, and ssim_sum through every
 *   counting position whose window holds it, not finite; it is not left out.
 *   Limits    : window odd in [3, MVD_SSIM_MAX_WINDOW]; H, W >= window with weights; 1 <= H, W <= 32768; C >= 1; B >= 0 with
 *             B * C <= 65535 (offsets are 64-bit: no limit on B * C * H * W below those); weights, c1, c2 finite.  B = 0 succeeds and
 *             enqueues nothing.
 *   scratch   : mvd_image_metrics_scratch(B, C, H, W, window) bytes (window = 0 without weights), 8-byte aligned; 0 for arguments outside
 *             the limits.  It holds one partial per (image, chunk of MVD_METRIC_CHUNK pixels) and per (plane, tile).
 *   Kernels   : squared error: a workgroup per chunk; SSIM: a workgroup per tile of MVD_SSIM_TILE_W x MVD_SSIM_TILE_H window positions of
 *             a plane, the fp32 tile plus halo of both images staged in LDS, the five moments taken one after the other through ONE
 *             row-filtered fp64 plane in LDS -- 36.3 KiB per workgroup whatever the window, four workgroups per CU; then one workgroup
 *             per image sums the partials.  Three enqueues (two without weights).
 *
 * mvd_depth_metrics: pred, target (B, H, W) fp32; valid (B, H, W) uint8 or NULL.  A pixel COUNTS when valid is non-zero (or NULL) and
 *   both values are finite and > 0 (the renderers' empty depth, +inf, drops out by itself).
 *   Pass 1    : per image n, Sp, St, Spp, Spt over the counting pixels with p = double(pred), t = double(target) (the products exact),
 *             and the fit (s, b):  MVD_DEPTH_ALIGN_NONE: (1, 0);  _SCALE: (Spt / Spp, 0) (0 / 0 = NaN without a pixel);
 *             _SCALE_SHIFT: det = n * Spp - Sp * Sp; s = (n * Spt - Sp * St) / det, b = (Spp * St - Sp * Spt) / det, and s = b = NaN
 *             unless det > 0 (one pixel: det is exactly 0);  _GIVEN: pass 1 does not run, (s, b) = fit_in[image] (B, 2) fp64 on the
 *             device -- required with _GIVEN, refused otherwise.
 *   Pass 2    : q = s * p + b (the product, then the sum).  A counting pixel whose q is not > 0 (a NaN fit: all of them) is DROPPED and
 *             counted as such.  Over the others, with d = q - t:
 *               sums   (B, 4) fp64 : |d| / t;  (d * d) / t;  d * d;  l * l with l = log(q) - log(t)
 *               counts (B, 5) int64: r < 1.25;  r < 1.5625;  r < 1.953125 with r = max(q / t, t / q) (strict: p = 4, t = 5 is not
 *                                    below 1.25);  the pixels summed;  the pixels dropped
 *             fit (B, 2) fp64: the (s, b) used.  Every output may be NULL.  log is the device library's fp64 logarithm, the one
 *             operation here that is not correctly rounded (DESIGN.md has its error measured).
 *   Limits    : 0 <= B <= 65535 (B = 0 succeeds and enqueues nothing), 1 <= H, W <= 32768.
 *   scratch   : mvd_depth_metrics_scratch(B, H, W) bytes, 8-byte aligned; 0 outside the limits.
 *   Kernels   : a workgroup per chunk of MVD_METRIC_CHUNK pixels and one per image for the second stage, in both passes: four
 *             enqueues, two with _GIVEN.
 *
 * Both: every sum is fp64 with a fixed order -- in a thread ascending, in a workgroup a fixed tree, over the partials in the scratch
 * thread t takes partials t, t + 256, ... and the tree again -- a function of (C, H, W, window) alone: the same bits run to run, for
 * an image alone or at any place in a batch, and with any subset of the outputs NULL.  No floating-point atomics; the counts are
 * integers.  Every argument is checked before anything is enqueued; a refused call returns non-zero, writes nothing and names the entry
 * in mvd_last_error().  Work goes to the caller's stream with no host synchronisation.
 *
 * Out of scope: LPIPS and any other learned metric; multi-scale SSIM; "same"-padded SSIM; gradients. */
#define MVD_SSIM_MAX_WINDOW 33
#define MVD_SSIM_TILE_W 32
#define MVD_SSIM_TILE_H 16
#define MVD_METRIC_CHUNK 2048
#define MVD_DEPTH_ALIGN_NONE 0
#define MVD_DEPTH_ALIGN_SCALE 1
#define MVD_DEPTH_ALIGN_SCALE_SHIFT 2
#define MVD_DEPTH_ALIGN_GIVEN 3
size_t mvd_image_metrics_scratch(int B, int C, int H, int W, int window);
int mvd_image_metrics(const float* a, const float* b, const unsigned char* mask, int B, int C, int H, int W, const double* weights,
                      int window, double c1, double c2, double* sq_sum, long long* count, double* ssim_sum, long long* ssim_count,
                      double* ssim_map, void* scratch, size_t scratch_bytes, mvd_stream_t stream);
size_t mvd_depth_metrics_scratch(int B, int H, int W);
int mvd_depth_metrics(const float* pred, const float* target, const unsigned char* valid, int B, int H, int W, int align,
                      const double* fit_in, double* fit, double* sums, long long* counts, void* scratch, size_t scratch_bytes,
                      mvd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * hipGraph capture of a whole denoising step and HIP-event timing on the caller's stream. */
int mvd_graph_begin(mvd_stream_t stream);
int mvd_graph_end(mvd_stream_t stream, void** graph_exec);
int mvd_graph_launch(void* graph_exec, mvd_stream_t stream);
int mvd_graph_destroy(void* graph_exec);
int mvd_event_create(void** ev);
int mvd_event_record(void* ev, mvd_stream_t stream);
int mvd_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int mvd_event_destroy(void* ev);

/* ------------------------------------------------------------------------------------------------
 * Backward of the conv / linear / GroupNorm family (training step, reference train.py:90-95 `loss.backward()`; SURVEY.md
 * section 8(f) rank 4).  The products run on mvd_gemm:  dgrad = mvd_gemm(planes of dY, packed W^T / rotated 3x3 filter);
 * wgrad = mvd_gemm(A = (dY)^T planes, B = MVD_B_PLANES (X)^T or (im2col X)^T planes) -> the parameter's own memory layout.
 * These entries produce the transposed operands, the bias gradient and the GroupNorm(+SiLU) backward.  Deterministic. */
/* x: fp32 (rows, ldx) [src_planes = 0] or split planes (rows, 2*ldx) [1]  ->  out_sp: split planes of x^T, (cols, 2*ldo),
 * ldo % 32 == 0, ldo >= rows rounded up to 32 (columns [rows, ceil32(rows)) are written as zeros). */
int mvd_transpose_planes(const void* x, int src_planes, int rows, int cols, int ldx, void* out_sp, int ldo, mvd_stream_t stream);
/* ... of an fp32 source multiplied by *scale_dev first (see mvd_split_planes_scaled). */
int mvd_transpose_planes_scaled(const float* x, int rows, int cols, int ldx, void* out_sp, int ldo, const float* scale_dev,
                                mvd_stream_t stream);
/* x_sp: channels-last (B,H,W,Cin) activation in split planes, Cin % 32 == 0  ->  out_sp (9*Cin, 2*ldo): row ci*9 + ky*3 + kx,
 * column = output pixel of the 3x3 / stride 1 / pad 1 conv (F.unfold order, transposed). */
int mvd_im2col3x3_t_planes(const void* x_sp, int B, int H, int W, int Cin, void* out_sp, int ldo, mvd_stream_t stream);
/* out2 = {s, 1/s}: the power of two s that brings max|x| of the n floats into [1024, 2048) (1 if the maximum is 0 or not finite) -- the
 * scale a gradient is multiplied with before its fp16 hi + lo split (operand range contract above), on the device, one launch.
 * scratch2: two zero-initialised 32-bit words owned by the caller; the kernel leaves them zero. */
int mvd_pow2_scale(const float* x, size_t n, float* out2, unsigned* scratch2, mvd_stream_t stream);
/* torch.optim.AdamW (no amsgrad) for a list of fp32 tensors in ONE launch (train.py:95 optimizer.step()).  tensors: device array of
 * {float* p; const float* g; float* m; float* v; unsigned long long numel; unsigned first_chunk; unsigned pad;} (48 bytes): parameter,
 * gradient, exp_avg, exp_avg_sq; first_chunk = running sum of ceil(numel / 4096) over the preceding entries, n_chunks = that sum over all.
 * bias_c1 = 1 - beta1^step, bias_c2_sqrt = sqrt(1 - beta2^step); grad_scale multiplies every gradient first (1 = none). */
int mvd_adamw_multi(const void* tensors, int n_tensors, int n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                    float bias_c1, float bias_c2_sqrt, float grad_scale, mvd_stream_t stream);
/* out[c] = sum_r x[r][c] (bias gradient): fp64 partials, fixed order.  ws: mvd_col_sum_workspace_doubles(rows, cols) doubles. */
size_t mvd_col_sum_workspace_doubles(int rows, int cols);
int mvd_col_sum(const float* x, int rows, int cols, int ldx, float* out, double* ws, size_t ws_doubles, mvd_stream_t stream);
/* mvd_col_sum and mvd_pow2_scale of the same (rows, cols) matrix (ldx == cols: the scale is over exactly the summed elements) in ONE pass:
 * out[c] = column sums, out2 = {s, 1/s}.  scratch1: one zero-initialised word per stream (left zero). */
int mvd_col_sum_pow2(const float* x, int rows, int cols, int ldx, float* out, double* ws, size_t ws_doubles, float* out2, unsigned* scratch1,
                     mvd_stream_t stream);
/* Backward of y = act(GroupNorm(x)) (act = SiLU when silu != 0; torch.nn.GroupNorm semantics, openaimodel.py GroupNorm32):
 * dy = dL/dy  ->  dx (B,HW,C), dgamma (C), dbeta (C).  ws: B*groups*2 + B*C*2 floats. */
int mvd_groupnorm_backward(const float* x, const float* dy, const float* gamma, const float* beta, int B, int HW, int C, int groups,
                           float eps, int silu, float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_floats,
                           mvd_stream_t stream);

/* Backward of y = LayerNorm(x) * w + b (last dimension, w may be null): dx, and dyxhat = dy * xhat so that
 * dw = mvd_col_sum(dyxhat), db = mvd_col_sum(dy).  dyxhat may be null. */
int mvd_layernorm_backward(const float* x, const float* dy, const float* w, int rows, int C, float eps, float* dx, float* dyxhat,
                           mvd_stream_t stream);
/* Column sums per row group: out[g][c] = sum over rows [g*rows_per_group, (g+1)*rows_per_group) of x[r][c] (ngroups x cols), same
 * fixed-order fp64 reduction as mvd_col_sum per group.  ws: mvd_col_sum_groups_workspace_doubles(ngroups, rows_per_group, cols). */
size_t mvd_col_sum_groups_workspace_doubles(int ngroups, int rows_per_group, int cols);
int mvd_col_sum_groups(const float* x, int ngroups, int rows_per_group, int cols, int ldx, float* out, double* ws, size_t ws_doubles,
                       mvd_stream_t stream);
/* mvd_layernorm_backward with one weight per row group (the backward of mvd_layernorm_groups): rows of group g use w + g*ldw.  Writes dx,
 * dyxhat (rows, C; required when dw is given) and, when non-null, dw / db (ngroups, C) = the column sums of dyxhat / dy per group (the
 * per-scene dscale / dshift of adaLN).  ws: mvd_col_sum_groups_workspace_doubles(rows / rows_per_group, rows_per_group, C) doubles. */
int mvd_layernorm_backward_groups(const float* x, const float* dy, const float* w, int ldw, int rows, int rows_per_group, int C, float eps,
                                  float* dx, float* dyxhat, float* dw, float* db, double* ws, size_t ws_doubles, mvd_stream_t stream);
/* Activations of the training step (viewfusion_zero_depth_rgb.py:362-397 -> view_attn_efficient2.py:42-67 DiTBlock / Mlp, pre_layer_b):
 * mvd_act_planes: y = act(x), act = MVD_ACT_GELU (exact erf) or MVD_ACT_SILU, of the fp32 matrix x (rows, cols; leading dim ldx) as split
 * planes (sp, ldp % 32 == 0, padded columns zero; NULL = none) and / or fp32 (y, leading dim ldy; NULL = none) in one pass.
 * mvd_act_backward: dx[i] = dy[i] * act'(x[i]) over n elements (dx may alias dy). */
int mvd_act_planes(const float* x, void* sp, float* y, size_t rows, int cols, int ldx, int ldp, int ldy, int act, mvd_stream_t stream);
int mvd_act_backward(const float* dy, const float* x, float* dx, size_t n, int act, mvd_stream_t stream);
/* Backward of GEGLU y = a * gelu(g), [a | g] = h (rows, 2*half) (sd1 attention.py:43-44): dh (rows, 2*half). */
int mvd_geglu_backward(const float* h, const float* dy, int rows, int half, float* dh, mvd_stream_t stream);
/* Backward of the self-attention core softmax(Q K^T / sqrt(d)) V per (batch, head); q, k, v, dout, dq, dk, dv: token-major
 * (B*L, heads*dhead) fp32.  stats: B*heads*L*3 floats of scratch ({max, sum, delta} per query row).  Training path, deterministic.
 * Sequences longer than 16 run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: fp32 operands and accumulation, two kernels -- dQ +
 * row statistics, then dK / dV); the L <= 16 sequences over GridAttn's reference views stay on the VALU kernel. */
int mvd_attention_backward(const float* q, const float* k, const float* v, const float* dout, int B, int heads, int L, int dhead,
                           float* dq, float* dk, float* dv, float* stats, size_t stats_floats, mvd_stream_t stream);
/* Backward of mvd_pixel_cross_attn (D context tokens per pixel): q, dout, dq (P, C); k, v, dk, dv (P*D, C). */
int mvd_pixel_cross_attn_backward(const float* q, const float* k, const float* v, const float* dout, int P, int D, int heads, int dhead,
                                  float* dq, float* dk, float* dv, mvd_stream_t stream);

/* Backward of mvd_gridattn_tokens w.r.t. the feature maps (grid_sample backward, view_attn_efficient2.py:320-341): dtok (T, ldt)
 * fp32 token gradients (columns [0,256) reference-view samples, [256,512) input-view samples) are scattered with the forward's
 * taps into 64-bit fixed-point accumulators dfeat_acc (V,S,S,256) / din_feat_acc (S,S,256) (value * scale; zeroed by the caller). */
int mvd_gridattn_tokens_backward(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                                 const float* cams, const float* in_cam, const float* dtok, int ldt, long long* dfeat_acc,
                                 long long* din_feat_acc, float scale, int V, int q0, int Vq, int S, int D, float depth_scale,
                                 float depth_shift, mvd_stream_t stream);
/* mvd_gridattn_tokens_backward for nscene scenes (the layouts of mvd_gridattn_tokens_scenes_t, per-scene step rows included):
 * dtok rows scene-major, dfeat_acc (nscene*V,S,S,256), din_feat_acc (nscene,S,S,256).  Same 64-bit fixed-point scatter: bit-identical to
 * one mvd_gridattn_tokens_backward per scene at that scene's step row.  nscene = 1, steps_scene_stride = 0 is mvd_gridattn_tokens_backward. */
int mvd_gridattn_tokens_backward_scenes(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                                        const float* cams, const float* in_cam, const float* dtok, int ldt, long long* dfeat_acc,
                                        long long* din_feat_acc, float scale, int nscene, int V, int q0, int Vq, int S, int D,
                                        float depth_scale, float depth_shift, int steps_scene_stride, mvd_stream_t stream);
/* mvd_gridattn_tokens_backward_scenes over the rows of mvd_gridattn_tokens_window (dtok row pt*W + slot scatters into view
 * (b + slot - W/2) mod V; a view repeated by W > V accumulates every repeat).  window = 0 is mvd_gridattn_tokens_backward_scenes. */
int mvd_gridattn_tokens_backward_window(const float* x, const float* depth_noise, const float* steps, const int* iter, const float* grid_lin,
                                        const float* cams, const float* in_cam, const float* dtok, int ldt, long long* dfeat_acc,
                                        long long* din_feat_acc, float scale, int nscene, int V, int q0, int Vq, int S, int D,
                                        float depth_scale, float depth_shift, int steps_scene_stride, int window, mvd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVD_HIP_H */
