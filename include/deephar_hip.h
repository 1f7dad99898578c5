/*
 * deephar_hip.h -- C-ABI of libdeephar_hip.so, the MI355X (gfx950) execution back-end for the
 * pose-regression hot path of dluvizon/deephar.
 *
 * The reference has no FFI of its own: its arithmetic is reached through Keras 2.1.4 layer objects that
 * lower to TensorFlow 1.6 kernels (reference deephar/layers.py:6-42, requirements.txt:2-3).  The seam is
 * therefore "what a Keras layer call computes".  Each entry point below names the Keras layer(s) /
 * reference function it replaces; the Python host (deephar_amd/) and any other host bind exactly these.
 *
 * Conventions
 *   - fp32, NHWC ("channels_last", reference deephar/config.py:4).  A tensor view is (pointer, ld) where
 *     ld = number of floats between consecutive pixels, so channel slices / concatenation targets are
 *     expressed by pointer offset + ld (no copies for keras.layers.concatenate / Lambda slicing).
 *   - all pointers are DEVICE pointers unless the name ends in _host; `stream` is a hipStream_t passed as
 *     void*; every call is asynchronous on that stream and captures cleanly into a hipGraph.
 *   - return value: 0 = OK, <0 = error (see dh_error_string).  Nothing throws, nothing allocates.
 */
#ifndef DEEPHAR_HIP_H_
#define DEEPHAR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK 0
#define DH_EINVAL (-1)       /* bad argument / shape */
#define DH_EUNSUPPORTED (-2) /* valid request the kernels do not cover */
#define DH_ELAUNCH (-3)      /* HIP reported a launch/runtime error */

int dh_version(void);
const char* dh_error_string(int rc);
/* name of the gfx target of device `dev`, CU count; rc<0 when no HIP device is visible */
int dh_device_info(int dev, char* arch_name, int arch_name_len, int* cu_count);

/* ---------------------------------------------------------------------------------------------------
 * Conv2D (+ folded BatchNormalization / ReLU / add / UpSampling2D):
 *   replaces layers.conv2d (layers.py:66-71) and its compositions conv_bn (:202), conv_act (:219),
 *   conv_bn_act (:230), act_conv_bn (:258), act_conv (:317); the pointwise half of sepconv2d (:74-80,
 *   288-301); common.residual_unit's BN->ReLU->conv chains (models/common.py:25-67).
 *   y[m,co] = relu?( (sum_k pro(x)[m,k] * w[k,co]) * post_scale[co] + post_shift[co] + res1 + res2 )
 *   pro(v)  = relu?( v * pre_scale[ci] + pre_shift[ci] ), applied to in-bounds taps only
 *   Padding is explicit (pt, pl) so TF-"SAME" asymmetric padding is the caller's arithmetic.
 *   up2 = 1 fuses keras UpSampling2D((2,2)) + add (reception.py:122-127): y is [N,2*OH,2*OW,Cout],
 *   res1 is read at conv resolution, res2 at the up-sampled resolution.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_conv_args {
  const float* x;
  const float* w; /* packed by dh_conv2d_pack_weights_host */
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  const float* post_scale;
  const float* post_shift;
  const float* res1;
  const float* res2;
  const float* in_lut; /* x_u8 only: [Cin][256] value of every byte after the loader's normalisation */
  int32_t N, H, W, Cin, ldx;
  int32_t OH, OW, Cout, ldy;
  int32_t KH, KW, SH, SW, PT, PL;
  int32_t K;      /* KH*KW*Cin */
  int32_t Kp, Np; /* padded dims of the packed weight */
  int32_t ldr1, ldr2;
  int32_t pre_relu, post_relu;
  int32_t up2;
  int32_t x_u8; /* 1: x points to uint8 frames [N,H,W,ldx]; every byte goes through in_lut before the (optional)
                   BN prologue, zero padding is applied after it.  This is utils/transform.normalize_channels
                   (transform.py:212-231: /255, power, -0.5, *2 in float32) fused into the first convolution; only
                   the general K x K path (tile_cfg < 0, or one of its tilings 0..8) and the first-layer kernel
                   (dh_conv2d_uses_first_layer_kernel) take it */
  int32_t w_split; /* weight layout.  0: fp32, [Kp/4][Np][4], K tap-major.  2: fp32, same container, K chunk-major for the
                      halo-resident K x K kernel (see dh_conv2d_halo_eligible).
                      1 ("bf16x3"): `w` was packed by dh_conv2d_pack_weights_split_host (every weight split exactly into three bf16
                      parts) and the convolution runs on the bf16 matrix cores: fp32 activations are split the same way
                      on the fly, six of the nine partial products are accumulated in fp32 (gemm1x1s.hip).  Same
                      inputs / outputs / epilogue; per-product error <= 2^-23 relative, i.e. below the rounding of the
                      fp32 accumulation -- NOT bit-identical to w_split = 0.  Only shapes the LDS-DMA GEMM covers
                      (pointwise, or K x K with Cin % 32 == 0; 16-byte aligned x; no BN prologue), else DH_EUNSUPPORTED.
                      3 ("bf16x2") / 4 ("bf16"): the reduced-precision members of the same family, `w` packed by
                      dh_conv2d_pack_weights_parts_host with parts = 2 / 1.  Operands are split by repeated round-to-nearest-even
                      (x1 = bf16(x), x2 = bf16(x - x1)), activations after the optional ReLU prologue; with P parts every output is
                      sum_k sum_{i + j <= P + 1} a_i[k] b_j[k] -- three products (a2 b1, a1 b2, a1 b1; ~2^-16 per product) or one
                      (a1 b1; ~2^-8) instead of six, each exact, fp32 accumulation, smallest first, K ascending in every tiling; the
                      fp32 epilogue is unchanged.  Same shapes, same refusals as 1.
                      5 / 6 / 7: the EXTENDED SCOPE of 1 / 3 / 4 (gemm1x1s_ext.hip) -- the same packings byte for byte, the same
                      arithmetic contract, and for a layer that 1 / 3 / 4 accept the same bits; accepted in addition (see
                      dh_conv2d_split_wide_eligible): a pointwise convolution with a BatchNormalization prologue (operand =
                      relu?(fmaf(x, pre_scale, pre_shift)), the one fused multiply-add of the fp32 kernel, then split) and a dense
                      K x K convolution with Cin % 16 == 0.  A layer that rule refuses returns DH_EUNSUPPORTED and is never
                      run on another kernel.  Any other value is DH_EINVAL */
  int32_t res2_down; /* 1: res2 is at HALF the output resolution, [N, OH/2, OW/2, Cout]: out(oh, ow) += res2(oh/2, ow/2), i.e.
                        add([., UpSampling2D((2, 2))(res2)]) with the up-sampling folded into the residual read
                        (reception.py:122-127: `b = UpSampling2D((2, 2))(b); x = add([a, b])` fused into the convolution
                        that produces a).  Needs OH, OW even and up2 = 0 */
  int32_t ldyp;
  int32_t x_resample; /* [r06] skinny-conv layers only (dh_conv2d_uses_split_k; DH_EUNSUPPORTED elsewhere): x is not stored at the
                         resolution H x W the convolution sees --
                           1: x is [N, H/2, W/2, Cin] and is read as UpSampling2D((2, 2))(x)      (spnet.py:89-91: the action head's
                              conv3 on the up-sampled class maps);
                           2: x is [N, 2H, 2W, Cin] and is read through MaxPooling2D((2, 2));
                           3: ... through layers.max_min_pooling((2, 2)) = max + min of the window (layers.py:411-425; spnet.py:77-79).
                         BN / ReLU prologue and zero padding act on the resampled pixels: bit for bit the convolution of the
                         tensor a stand-alone up-sampling / pooling launch would have written.  The field sits in what was
                         padding in front of y_pool: a zero-initialised struct is unchanged */
  float* y_pool; /* optional second output: MaxPooling2D((2, 2)) of the convolution's FINAL output (after BN / residuals /
                    ReLU), [N, OH/2, OW/2, Cout] with pixel pitch ldyp -- the hourglass reads every level both at full and
                    at half resolution (reception.py:105-116: x = ...; MaxPooling2D((2, 2))(x)), and a stand-alone pool
                    has to read the whole tensor back.  Built for OW == 32, OH even, 16-byte aligned rows, no up2, on the
                    tilings whose waves own 32-row blocks in pairs (an image row per wave, the pair pools through the
                    epilogue's LDS slab), and [r06] for OW == 16 / OW == 8 with OH * OW a multiple of 32 on every tiling
                    with 32-row waves (a wave's block is two / four whole image rows: it pools its own slab -- SPNet's
                    down path below 32 x 32, common.py:70-86); anything else returns DH_EUNSUPPORTED */
} dh_conv_args;

/* padded dims of the packed weight for a [KH,KW,Cin,Cout] (Keras HWIO) kernel */
int dh_conv2d_packed_dims(int KH, int KW, int Cin, int Cout, int* Kp, int* Np);
/* host-side repack HWIO -> [Kp/4][Np][4]; `packed_host` holds Kp*Np floats */
int dh_conv2d_pack_weights_host(const float* w_hwio_host, float* packed_host, int KH, int KW, int Cin,
                                int Cout);
/* split packing for w_split = 1: `packed_host` holds 3 * Kp * Np uint16 (bf16 bit patterns) laid out
 * [Kp/8][3 parts][Np][8]; same Kp / Np as dh_conv2d_packed_dims */
int dh_conv2d_pack_weights_split_host(const float* w_hwio_host, uint16_t* packed_host, int KH, int KW, int Cin,
                                      int Cout);
/* the same for `parts` = 3 / 2 / 1 bf16 parts per weight (w_split = 1 / 3 / 4): `packed_host` holds parts * Kp * Np uint16
 * laid out [Kp/8][parts][Np][8]; parts = 3 is dh_conv2d_pack_weights_split_host byte for byte, the parts of a smaller
 * mode are the leading parts of a larger one.  DH_EINVAL for any other `parts` */
int dh_conv2d_pack_weights_parts_host(const float* w_hwio_host, uint16_t* packed_host, int KH, int KW, int Cin,
                                      int Cout, int parts);
/* tile_cfg < 0: library heuristic; 0..dh_conv2d_num_tile_cfgs()-1 forces a tiling (autotuning hook): 0..8 the general
 * implicit-GEMM kernel, 9..17 the same tile shapes on the LDS-DMA GEMM (pointwise, K x K with Cin % 32 == 0; also with a
 * BatchNormalization prologue when pointwise).  A tiling that does not cover the layer returns DH_EUNSUPPORTED.  All
 * tilings of a layer give the same bits. */
int dh_conv2d_num_tile_cfgs(void);
int dh_conv2d_num_split_tile_cfgs(void); /* tilings of the w_split = 1 / 3 / 4 kernels: tile_cfg in [0, this) for every mode;
                                            a tiling a mode does not have answers DH_EUNSUPPORTED */
int dh_conv2d_pick_tile_cfg(int M, int Cout);
/* Inputs must be FINITE.  K is padded to the kernels' step with zero weights, and on the LDS-DMA GEMM a padded k slot of
 * a pixel holds the following floats in memory (the next pixel's first channels, clamped inside the buffer; on a view with
 * ldx > Cin the channels BEHIND the view inside the same pixel, i.e. the neighbouring tensor of a shared slab -- which is why
 * planner rule R4b keeps convolutions out of _VIEW_READERS): an Inf / NaN
 * there would reach this pixel's output as 0 * Inf.  The first-layer kernel (raw frames) and the skinny-conv
 * kernel zero the padded A operand instead; activations inside a model are finite by construction. */
/* 1 when dh_conv2d_f32 runs this convolution on the skinny-conv kernel (conv_splitk.hip: a tiny output map -- at most 256
 * positions per frame / clip, at most 256 output channels, K >= 64 [r05; was K >= 768, Cin % 4 == 0]: the action heads,
 * deephar/models/spnet.py:51-148, action.py:20-42, and the coarse heat-map heads, spnet.py:24-48): a rule on OH*OW, K, Cout and
 * Cin only, so that a layer's result bits never depend on tiling choice, batch size or alignment.  Such a layer takes
 * fp32-packed weights (w_split = 0) and ignores tile_cfg. */
int dh_conv2d_uses_split_k(const dh_conv_args* a);
/* 1 when dh_conv2d_f32 runs this convolution on the first-layer kernel (conv_stem.hip): 3 dense input channels (ldx = 3,
 * float or x_u8 frames), stride 2, 3x3 or 7x7, 128 output columns, an even number of output rows, 32 or 64 output
 * channels, fp32 tap-major weights (w_split = 0), BN / ReLU epilogue only -- layers.conv_bn_act of reception.py:61-66 and
 * the 7x7 entry conv of spnet.py:317-322 on 256 x 256 frames.  Like the split-K rule it looks at the layer's geometry
 * only; such a layer ignores tile_cfg. */
int dh_conv2d_uses_first_layer_kernel(const dh_conv_args* a);
/* 1 when dh_conv2d_f32 would accept this convolution with w_split = 1, 3 or 4 -- one rule for the three modes (every field but `w` / `w_split` filled in as for
 * the launch): an LDS-DMA GEMM shape (pointwise, or K x K with Cin % 32 == 0, no fused up-sampling), 16-byte aligned
 * float input, no BN prologue, not a split-K layer, operands within the 32-bit buffer offsets of the kernel.  A
 * binding asks this BEFORE it packs the weights, so that a layer is never bound with a packing its launch rejects. */
int dh_conv2d_split_eligible(const dh_conv_args* a);
/* 1 when dh_conv2d_f32 would accept this convolution with w_split = 5, 6 or 7, the extended scope of the same three modes --
 * again one rule for the three, on the layer's per-frame geometry and alignment only (never on timing or on `w` / `w_split`;
 * the batch size only enters through the 32-bit buffer offsets, as above): everything dh_conv2d_split_eligible accepts, and
 * (a) a pointwise convolution with a BatchNormalization prologue (pre_scale AND pre_shift, Kp <= 4096: the tables live in
 * LDS), (b) a dense K x K convolution with Cin % 16 == 0 at any stride and explicit padding; both with a 16-byte aligned
 * float input, no fused up-sampling, not a split-K layer, not the first layer.  K x K with Cin % 16 != 0 or with a BN
 * prologue stays refused.  A binding asks this BEFORE it packs the weights. */
int dh_conv2d_split_wide_eligible(const dh_conv_args* a);
/* 1 when this convolution belongs to the halo-resident K x K kernel (conv_halo.hip): dense K x K, stride 1, Cin % 16
 * == 0 but Cin % 32 != 0 (the layers the LDS-DMA tap-major kernel cannot take), maps of >= 1024 pixels per frame whose
 * rows tile into runs of 128 output pixels, 16-byte aligned float input, no BN prologue / fused up-sampling.  (The
 * kernel itself also runs Cin % 32 == 0 when asked with w_split = 2.)  A rule on the per-frame geometry only -- never on the batch size or on timing --
 * because that kernel sums K chunk-major ([16-channel chunk][kh][kw][16]) and its results differ in the last bits
 * from the tap-major kernels'.  Such a layer is launched with w_split = 2 and weights packed in that K order: HWIO
 * re-ordered to [Cin/16][KH][KW][16] rows, then dh_conv2d_pack_weights_host with (1, 1, KH*KW*Cin, Cout);
 * tile_cfg in [0, dh_conv2d_num_halo_tile_cfgs()) or < 0. */
int dh_conv2d_halo_eligible(const dh_conv_args* a);
int dh_conv2d_num_halo_tile_cfgs(void);
/* What dh_conv2d_f32(a, tile_cfg, .) will do, decided from the arguments alone: no pointer is dereferenced, nothing is
 * launched.  dh_conv2d_f32 launches exactly what this says, so `rc` is its return code unless HIP itself fails
 * (DH_ELAUNCH). */
#define DH_CONV_GENERAL 1     /* implicit GEMM, register-staged (conv_igemm.hip): tile_cfg 0..8 */
#define DH_CONV_DMA 2         /* LDS-DMA GEMM, fp32 (gemm1x1.hip): tile_cfg 9..17, reported as 0..8 */
#define DH_CONV_SPLIT 3       /* LDS-DMA GEMM, split-bf16 (w_split 1 / 3 / 4, and the layers of 5 / 6 / 7 that rule accepts) */
#define DH_CONV_SPLIT_EXT 4   /* the two layer classes the extended scope adds (w_split 5 / 6 / 7) */
#define DH_CONV_HALO 5        /* halo-resident K x K (w_split 2) */
#define DH_CONV_SKINNY 6      /* dh_conv2d_uses_split_k */
#define DH_CONV_FIRST_LAYER 7 /* dh_conv2d_uses_first_layer_kernel */
typedef struct dh_conv_route {
  int32_t rc;       /* DH_OK, or the DH_EINVAL / DH_EUNSUPPORTED dh_conv2d_f32 answers: every other field is 0, tile_cfg -1 */
  int32_t kernel;   /* DH_CONV_* */
  int32_t tile_cfg; /* the tiling inside that family after the heuristic (tile_cfg < 0) and every remap: the pooled-output
                       pick, 128 x 192 -> 128 x 96 under fused up-sampling, the halo kernel's widest TN that fits; -1 for the
                       skinny-conv and the first-layer kernel, which have none */
  int32_t parts;    /* bf16 parts per operand (DH_CONV_SPLIT, DH_CONV_SPLIT_EXT), else 0 */
  int32_t bm, bn;   /* output pixels x output channels of a work-group's tile (0 x 0: first-layer kernel) */
  int32_t tm;       /* 32-row blocks per wave: 1 = the tilings that prefetch a residual tile and may store direct; 0: no MFMA tile */
  int32_t vec4;     /* 16-byte loads of x: the float4 gather of DH_CONV_GENERAL / DH_CONV_SKINNY (0: dword loads, same bits);
                       always 1 for the LDS-DMA and halo kernels, 0 for the first layer */
  int32_t epi;      /* bit 0: the 16-byte epilogue (0: scalar, as soon as one of y / res1 / res2 / the BN tables is
                       misaligned or Cout % 4 != 0); bit 1: interior tiles store straight from the accumulators -- set for
                       DH_CONV_DMA and DH_CONV_HALO only (halo: not with a second residual), used by tilings with tm == 1 */
  int32_t pool;     /* y_pool: 1 = pairs of waves pool two image rows (OW = 32), 2 = a wave pools its own rows; 0: no y_pool */
  uint32_t tiles;   /* work-groups of the launch */
} dh_conv_route;
/* DH_EINVAL only for a NULL argument; every other answer, refusals included, is in out->rc. */
int dh_conv2d_route(const dh_conv_args* a, int tile_cfg, dh_conv_route* out);
int dh_conv2d_f32(const dh_conv_args* a, int tile_cfg, void* stream);

/* Stand-alone version of the same normalisation for inputs that do not feed a convolution directly:
 * y[i, c] = lut[c*256 + x[i, c]] for n_pixels x C bytes (transform.py:212-231). */
int dh_normalize_u8_f32(const uint8_t* x, const float* lut, float* y, int64_t n_pixels, int C, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Depthwise KxK conv, stride 1 (stride 2: dh_dwconv2d_strided_f32 below), explicit padding: the depthwise half of keras SeparableConv2D
 * (layers.py:74-80, 288-301; depth_multiplier 1, no bias).  w is [KH,KW,C] (= Keras [KH,KW,C,1]).
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_dw_args {
  const float* x;
  const float* w;
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  int32_t N, H, W, C, ldx, ldy;
  int32_t KH, KW, PT, PL;
  int32_t pre_relu;
  int32_t up_in; /* [r06] 1: x is stored at HALF resolution, [N, H/2, W/2, C] (H, W even), and the convolution reads
                    UpSampling2D((2, 2))(x): input pixel (h, w) = x(h/2, w/2) -- the nearest up-sampling in front of SPNet's
                    up-scaling unit (deephar/models/common.py:89-108: residual_unit(UpSampling2D(x))) is never written out;
                    BN / ReLU prologue and zero padding as without it (both act on the up-sampled pixels).  The field
                    occupies what was tail padding of the struct: a caller that zero-initialises it is unchanged */
} dh_dw_args;
int dh_dwconv2d_f32(const dh_dw_args* a, void* stream);
/* 1 when dh_dwconv2d_f32 runs this launch on its LDS-tiled kernel (32-bit buffer offsets inside a frame), 0 when on a
 * register kernel (64-bit addresses) or not at all.  Every field filled in as for the launch; no pointer is dereferenced.
 * All stride-1 kernels sum in one order: the answer never changes a bit of the result. */
int dh_dwconv2d_uses_lds_kernel(const dh_dw_args* a);

/* ---------------------------------------------------------------------------------------------------
 * Strided depthwise KxK conv: the depthwise half of keras SeparableConv2D(k, strides=(2, 2), padding='same',
 * use_bias=False) -- the stride-2 residual unit of SPNet's learned-resampling flavour (downsampling_type='conv':
 * deephar/models/common.py:70-86, 25-67; layers.py:74-80), replaces the depthwise half of layers.sepconv2d at a stride.
 *   y[n, oh, ow, c] = sum_{kh, kw} pro(x)[n, oh*SH - PT + kh, ow*SW - PL + kw, c] * w[kh, kw, c]
 *   pro(v) = relu?( v * pre_scale[c] + pre_shift[c] ) on in-bounds taps, zero outside (padding AFTER the prologue).
 * Padding is explicit (PT, PL): TF-"SAME" at stride 2 is asymmetric on even extents (k = 5: one row above, two below),
 * the caller's arithmetic.  w is [KH, KW, C].  Built for KH = KW in {3, 5} and SH = SW = 2 (DH_EUNSUPPORTED otherwise);
 * any ldx / ldy >= C (channel slabs of joint buffers), any C.  Taps are summed kh ascending, kw ascending, one fused
 * multiply-add each -- the order of dh_dwconv2d_f32, so an output equals the stride-1 output at the same window position
 * bit for bit.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_dw_strided {
  const float* x;
  const float* w;
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  int32_t N, H, W, C, ldx, ldy;
  int32_t OH, OW;
  int32_t KH, KW, SH, SW, PT, PL;
  int32_t pre_relu;
  int32_t reserved; /* 0 */
} dh_dw_strided;
int dh_dwconv2d_strided_f32(const dh_dw_strided* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Conv2DTranspose(filters, (2, 2), strides=(2, 2), padding='same', use_bias=False) (+ folded BatchNormalization / ReLU
 * in front, add / ReLU behind): replaces layers.conv2dtranspose (deephar/layers.py:83-89) as common.upscaling_unit uses
 * it (deephar/models/common.py:103-106: BN -> ReLU -> Conv2DTranspose) and the pyramid's add([xp, lp[i]]) behind the
 * unit (spnet.py:303).
 *   y[n, 2i+a, 2j+b, co] = relu?( sum_ci W[a, b, co, ci] * pro(x)[n, i, j, ci] + res[n, 2i+a, 2j+b, co] )     (no kernel flip)
 *   pro(v) = relu?( v * pre_scale[ci] + pre_shift[ci] );  x is [N, H, W, Cin], y and res are [N, 2H, 2W, Cout].
 * One GEMM [N*H*W, Cin] x [Cin, 4*Cout] on the fp32 matrix cores with a depth-to-space store.  `w` is the Keras kernel
 * [2, 2, Cout, Cin] re-ordered to the matrix B[ci][(2a + b) * Cout + co] and packed by dh_conv2d_pack_weights_host(B, .,
 * 1, 1, Cin, 4 * Cout); Kp / Np are dh_conv2d_packed_dims(1, 1, Cin, 4 * Cout).  The four column blocks are contiguous
 * (the padding to Np follows the last one); the kernel finds a column's block by comparison, for any Cout.
 * K is summed ascending in every tiling: result bits depend on neither tile_cfg (< 0: library heuristic, else
 * 0 .. dh_conv2d_transpose2x2_num_tile_cfgs() - 1) nor batch size.  The reduced-precision forms of the layer (the engine's
 * gemm_precision = 'bf16x3' / 'bf16x2' / 'bf16') are dh_conv2d_transpose2x2_split_f32 below; the layer is 4 % of the FLOPs of
 * a two-pyramid SPNet at 256 px, 11 % of an eight-pyramid one.
 * Needs Cin % 4 == 0, ldx % 4 == 0, 16-byte aligned x (DH_EUNSUPPORTED otherwise); inputs must be finite (see dh_conv2d_f32).
 * Other transposed-convolution geometries are not built.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_conv_transpose {
  const float* x;
  const float* w;
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  const float* res; /* optional, at the OUTPUT resolution, pixel pitch ldr */
  int32_t N, H, W, Cin, ldx;
  int32_t Cout, ldy, ldr;
  int32_t Kp, Np;
  int32_t pre_relu, post_relu;
} dh_conv_transpose;
int dh_conv2d_transpose2x2_num_tile_cfgs(void);
int dh_conv2d_transpose2x2_f32(const dh_conv_transpose* a, int tile_cfg, void* stream);
/* The same layer on the split-bf16 precision ladder (csrc/convt2x2s.hip): `parts` = 3 / 2 / 1 bf16 parts per operand
 * ("bf16x3" / "bf16x2" / "bf16", the modes of dh_conv_args.w_split = 1 / 3 / 4); any other value is DH_EINVAL.  `a` as for
 * dh_conv2d_transpose2x2_f32 except a->w: the same matrix B[ci][(2a + b) * Cout + co] packed by
 * dh_conv2d_pack_weights_parts_host(B, ., 1, 1, Cin, 4 * Cout, parts) as [Kp/8][parts][Np][8] bf16.
 *   operand  a[m, k] = relu?( fmaf(x[m, k], pre_scale[k], pre_shift[k]) ) in fp32 -- the ONE fused multiply-add of the fp32
 *            kernel, so the operand has its bits (a[m, k] = relu?(x[m, k]) without a prologue) -- then split by repeated
 *            round-to-nearest-even into `parts` bf16 parts: the split follows the prologue and the ReLU;
 *   sum      E_P = sum_k sum_{i + j <= parts + 1} a_i[k] b_j[k], products exact, fp32 accumulation, smallest product first
 *            per 16 k, K ascending in every tiling;
 *   store    the depth-to-space epilogue of the fp32 kernel, unchanged: residual at the output resolution, then ReLU.
 * Result bits depend on `parts` and the layer's geometry only: not on tile_cfg (< 0: library heuristic, else
 * 0 .. dh_conv2d_transpose2x2_num_split_tile_cfgs() - 1), batch size, position in the batch, or the vector / scalar store
 * path.  NOT bit-identical to dh_conv2d_transpose2x2_f32.  A layer dh_conv2d_transpose2x2_split_eligible refuses answers
 * DH_EUNSUPPORTED.  Inputs must be finite (see dh_conv2d_f32: a padded k slot holds the next pixel's floats, here times a
 * zero scale or a zero weight). */
int dh_conv2d_transpose2x2_num_split_tile_cfgs(void);
/* 1 when dh_conv2d_transpose2x2_split_f32 accepts this layer -- ONE rule for the three modes, on geometry and alignment only
 * (never on batch size or timing; every field but `w` filled in as for the launch, no pointer is dereferenced): Cin % 4 == 0,
 * ldx % 4 == 0, 16-byte aligned x, operands within the 32-bit buffer offsets of the kernel, and with a BatchNormalization
 * prologue Kp <= 4096 (its scale / shift tables live in LDS).  A binding asks this BEFORE it packs the weights. */
int dh_conv2d_transpose2x2_split_eligible(const dh_conv_transpose* a);
int dh_conv2d_transpose2x2_split_f32(const dh_conv_transpose* a, int parts, int tile_cfg, void* stream);

/* [r06] The two independent first layers of a pre-activation residual unit in ONE launch (deephar/models/common.py:25-67:
 * `shortcut = conv2d(relu(BN(x)), out, (1, 1))` beside `sepconv2d(relu(BN(x)), ...)`, whose depthwise half is `dw`): the
 * 1x1 convolution `conv` (BatchNormalization + ReLU prologue, w_split = 0, any epilogue of dh_conv_args but up2 / y_pool)
 * and the 5x5 depthwise convolution `dw` (BatchNormalization + ReLU prologue).  Work-groups of the one grid run either
 * kernel's own code, so the results are bit for bit those of dh_conv2d_f32 + dh_dwconv2d_f32; what is saved is one
 * dependent launch (~5 us plus the shorter of the two kernels) -- the latency regime of a couple of clips per call
 * (exp/pennaction/eval_speed2d.py).  DH_EUNSUPPORTED for any pair outside that description (call the two entry points). */
int dh_conv2d_dw_group_f32(const dh_conv_args* conv, const dh_dw_args* dw, void* stream);

/* [r06] A skinny-conv layer (dh_conv2d_uses_split_k) whose input is a concatenation that is never written out:
 *   concatenate([MaxPooling2D((2, 2), strides=(pool_sh, 2), padding='same')(x), x2])
 * -- SPNet's action head pools its pose and appearance features and concatenates them with the features handed on by the
 * previous head in front of its second residual unit (deephar/models/spnet.py:126-141: x1, x2 = maxpooling2d(...);
 * concat_tensorlist([x1, x2, xa]); residual(...)).  `a` describes the convolution as dh_conv2d_f32 would see the concatenated
 * tensor (H, W: the pooled extent; Cin: all channels; ldx: the pixel pitch of x; x_resample = 0); `seg` says where the second
 * run of channels lives.  x is [N, H * pool_sh, 2 W, c_split] (pool_sh = 1: windows of two rows starting at EVERY row, the last
 * one a single row -- the reference's time_stride = 1 for clips shorter than 16 frames; pool_sh = 2: disjoint windows).  The
 * BatchNormalization / ReLU prologue and the zero padding act on the concatenated pixels: bit for bit dh_conv2d_f32 on the
 * tensor a pooling launch and the concatenation would have written. */
typedef struct dh_conv_seg {
  const float* x2;   /* channels [c_split, Cin): [N, H, W, Cin - c_split], pixel pitch ldx2; may be NULL when c_split == Cin */
  int32_t ldx2;
  int32_t c_split;   /* channels [0, c_split) are the pooled x */
  int32_t pool_sh;   /* 1 or 2: row stride of the pooling window (its column stride is 2) */
  int32_t reserved;  /* 0 */
} dh_conv_seg;
int dh_conv2d_seg_f32(const dh_conv_args* a, const dh_conv_seg* seg, void* stream);

/* [r06] Two INDEPENDENT convolutions with a tiny output map in ONE launch -- in SPNet's action head (deephar/models/spnet.py:
 * 113-133) the residual unit on the pose features and `conv2d(af, num_visual_features, (1, 1))` on the appearance features
 * meet only at the concatenation behind them.  Both must be layers of the skinny-conv kernel (dh_conv2d_uses_split_k), read
 * their inputs as stored (x_resample = 0) and neither may read or overwrite what the other writes (the caller's business:
 * they run concurrently).  Work-groups [0, tiles of a) run `a`, the rest `b`, each with the code its own launch would run:
 * the results are bit for bit those of two dh_conv2d_f32 calls.  DH_EUNSUPPORTED for any other pair. */
int dh_conv2d_pair_f32(const dh_conv_args* a, const dh_conv_args* b, void* stream);

/* MaxPooling2D (reception.py:74,86,108,115; layers.py:92-97), padding cells ignored;
 * mode 1 = layers.max_min_pooling (layers.py:411-425): maxpool(x) - maxpool(-x) */
typedef struct dh_pool_args {
  const float* x;
  float* y;
  int32_t N, H, W, C, ldx;
  int32_t OH, OW, ldy;
  int32_t KH, KW, SH, SW, PT, PL;
  int32_t mode;
} dh_pool_args;
int dh_pool2d_f32(const dh_pool_args* a, void* stream);

/* UpSampling2D((2,2)) [+ add]: y[n,h,w,c] = a[n,h,w,c] + b[n,h/2,w/2,c]; a may be NULL */
int dh_upsample2x_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int N, int H,
                          int W, int C, void* stream);

/* element-wise glue: keras add / multiply / Activation('sigmoid') / standalone BatchNormalization+ReLU.
 *   op 0: y = relu?( (a*scale+shift) + b + c )    op 1: y = (a*scale+shift) * b
 *   op 2: y = sigmoid( (a*scale+shift) + b )      bcast_b: b has one channel, broadcast over C
 * scale and shift are [C] tables given together or not at all: scale without shift is DH_EINVAL (shift alone is ignored). */
typedef struct dh_elt_args {
  const float* a;
  const float* b;
  const float* c;
  float* y;
  const float* scale;
  const float* shift;
  int32_t lda, ldb, ldc, ldy;
  int64_t npix;
  int32_t C;
  int32_t relu;
  int32_t op;
  int32_t bcast_b;
} dh_elt_args;
int dh_eltwise_f32(const dh_elt_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Soft-argmax decoder: activations.channel_softmax_2d (activations.py:3-16) + layers.lin_interpolation_2d /
 * softargmax2d (layers.py:122-129,160-200) + keypoint_confidence / build_joints_probability
 * (layers.py:107-119, blocks.py:328-343) in one pass over the maps.
 *   xy[f,c]        = sum_hw softmax(alpha*h)[h,w,c] * (gx[w], gy[h])
 *   conf_raw[f,c]  = max over 2x2 windows of conf_scale * (sum of the 4 raw values)
 *   conf_prob[f,c] = the same on the soft-max probabilities (spnet.py:183)
 *   prob           = the probability maps themselves (needed by kronecker_prod), may be NULL
 *   gmax[f,c]      = max_hw h  (GlobalMaxPooling2D on the raw maps, reception.py:216), may be NULL
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_sam_args {
  const float* h;
  const float* gx;
  const float* gy;
  float* xy;
  float* conf_raw;
  float* conf_prob;
  float* prob;
  float* gmax;
  int32_t F, H, W, C, ldh, ldxy, ldcr, ldcp, ldp;
  float alpha;
  float conf_scale;
  int32_t xy_times_conf; /* [r06] 1: xy receives (x, y) * conf_prob -- `multiply([p, c])` in front of the action head's pose
                            convolutions (spnet.py:108) folded into the read-out that produces both factors (the same two
                            fp32 values, one multiplication each: bit-identical); conf_prob itself may be NULL.  The field sits
                            in what was tail padding of the struct */
} dh_sam_args;
int dh_softargmax2d_f32(const dh_sam_args* a, void* stream);

/* The 2-D decoder with context of reception.pose_regression_2d_context (reception.py:167-182) in ONE launch: soft-argmax
 * of the J joint maps (channels [0, J) of `a->h`) and of the J*nctx context maps (channels J + j*nctx + k), their
 * confidences (keypoint_confidence of the raw maps) and blocks.build_context_aggregation (blocks.py:217-285):
 *   y[f, j] = agg_alpha * xy_j + (1 - agg_alpha) * sum_k xy_jk * conf_jk / sum_k conf_jk      -> y [F, J, 2], pitch ldy
 * a->conf_raw (optional, pitch ldcr) receives the J joint confidences; a->C = J * (1 + nctx); the other outputs of
 * dh_sam_args must be NULL.  Needs J % 4 == 0, nctx <= 3, ldh % 4 == 0 and a 16-byte aligned `h` (DH_EUNSUPPORTED
 * otherwise: use dh_softargmax2d_f32 twice + dh_context_aggregation_f32).  The kernel stages a frame's maps, 16 channel
 * lanes wide, and both grids in LDS and has no unstaged variant: (H * W * 16 + W + H) * 4 bytes above 128 KiB (45 x 45 and
 * 40 x 48 maps fit, 44 x 48 and 40 x 52 do not) are DH_EUNSUPPORTED as well, nothing is launched. */
int dh_softargmax2d_context_f32(const dh_sam_args* a, int J, int nctx, float agg_alpha, float* y, int ldy,
                                void* stream);
/* What the two launches above will do, decided from the arguments alone (nothing is dereferenced or launched; both
 * launchers run exactly this). */
typedef struct dh_sam_route {
  int32_t rc;       /* dh_softargmax2d_f32(a): DH_OK or DH_EINVAL */
  int32_t channels; /* ... channels per work-group: 16 once F * ceil(C / 16) >= 1024 work-groups fill the chip, else 4 */
  int32_t staged;   /* ... 1: a work-group's maps are staged in LDS ((H * W * channels + W + H) * 4 bytes, at most 128 KiB
                       with 16 channels, 60 KiB with 4); 0: read from memory twice */
  int32_t ctx_rc;   /* dh_softargmax2d_context_f32(a, J, nctx, ., y, ldy) with a valid y and ldy >= 2: DH_OK, DH_EINVAL or
                       DH_EUNSUPPORTED (J, nctx are not looked at for the first three fields) */
} dh_sam_route;
/* DH_EINVAL only for a NULL argument. */
int dh_softargmax2d_route(const dh_sam_args* a, int J, int nctx, dh_sam_route* out);

/* blocks.build_context_aggregation (blocks.py:217-285); ys [F,J,2], yc [F,J*nctx,2], pc [F,J*nctx] */
int dh_context_aggregation_f32(const float* ys, const float* yc, const float* pc, float* y, int F, int J,
                               int nctx, float alpha, int ldy, void* stream);

/* reception.pose_regression_3d (reception.py:193-222): depth/spatial means of the D*J maps ... */
int dh_depth_means_f32(const float* h, int ldh, float* hxy, float* hz, int F, int HW, int D, int J,
                       void* stream);
/* ... and blocks.build_softargmax_1d (blocks.py:288-303, layers.py:132-157, activations.py:18-30);
 * vz = max_d hz (GlobalMaxPooling1D, reception.py:217) */
int dh_softargmax1d_f32(const float* hz, const float* grid, float* z, int ldz, float* vz, int F, int D, int J,
                        void* stream);

/* layers.kronecker_prod (layers.py:478-508): f[b,j,c] = sum_p hm[b,p,j] * x[b,p,c] */
int dh_kronecker_f32(const float* hm, int ldh, const float* x, int ldx, float* f, int ldf, int B, int P, int J,
                     int C, void* stream);

/* layers.global_max_min_pooling (+ Activation('softmax')) (layers.py:428-442, action.py:14-17) */
int dh_global_maxmin_softmax_f32(const float* x, int ldx, float* y, int B, int P, int C, int softmax,
                                 void* stream);

/* keras concatenate / Lambda channel slicing fallback, ZeroPadding2D (spnet.py:98-107) */
int dh_copy_channels_f32(const float* x, int ldx, float* y, int ldy, int64_t npix, int C, void* stream);
/* y is [B,OH,OW,C]; x [B,H,W,C] lands at row offset PT, column offset PL, zeros elsewhere */
int dh_zeropad2d_f32(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, int PT, int PL,
                     void* stream);

/* SPNet depth read-out (spnet.py:201-205): z[f,j] = sum_hw sigmoid(d[f,h,w,j]) * prob[f,h,w,j]
 * (Activation('sigmoid') -> multiply -> Lambda K.sum over (H,W)) */
int dh_depth_from_maps_f32(const float* d, int ldd, const float* h, int ldh, float* z, int ldz, int F, int HW,
                           int J, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Plan / execute pair: a whole model forward behind three calls, for hosts without Python (what a C or
 * C++ replacement of Keras' Model.predict -- exp/common/mpii_tools.py:25,86, h36m_tools.py:46, penn_tools.py:124 -- binds).
 *   blob   : written by deephar_amd.Model.export_plan(path, batch) (deephar_amd/engine/serialize.py): the bound,
 *            autotuned launch list of Model.predict for `batch` items, device pointers relative to the activation
 *            arena / the weight image, plus the weight image itself (packed kernels, BN affines, grids).
 *   create : allocates arena + weights on the current device, uploads the weights, patches the pointers.  One plan
 *            per device; a plan is not re-entrant (one forward at a time), different plans are independent.
 *   forward: m <= batch items; inputs[i] / outputs[i] are DEVICE pointers to dense float32 [m, ...] tensors in the
 *            model's input / output order (outputs[i] may be NULL: not wanted); everything is enqueued on `stream`,
 *            nothing synchronises.  Results are bit-identical to Model.predict of the exporting process.
 *   forward_host: the same with HOST pointers (H2D, forward, D2H on an internal stream; returns when done).
 * uint8-input plans (Model.export_plan(path, batch, uint8=True): raw frames, normalised on the GPU like
 * utils/transform.normalize_channels, inside the first convolution where possible): dh_plan_input_is_u8(plan, i) == 1 and
 * inputs[i] points to m * dh_plan_input_items(plan, i) BYTES (cast the uint8 pointer to const float*).
 * rc != 0 -> the host raises its own error.
 * Multi-stream plans (Model.export_plan(path, batch, multi_stream=True) of a model with num_streams > 1: blob version 5,
 * the same layout plus a schedule section): create validates the section (a malformed or truncated one is DH_EINVAL),
 * opens dh_plan_num_streams(plan) - 1 non-blocking streams of the plan's own and the events that order them.  forward
 * runs the engine's enqueue program with the caller's stream as stream 0: input copies and input staging, fork, every
 * step on its scheduled stream with event waits for the cross-stream dependencies, join -- everything the side streams
 * did is ordered before whatever the caller enqueues on `stream` next, so the contract above does not change and the
 * results are the same bits.  If a launch fails behind the fork the side streams are still joined before the code is
 * returned.  A plan has at most 4 streams, the caller's included: every stream a process opens takes one of ROCm's four
 * hardware queues (GPU_MAX_HW_QUEUES), and the library never raises that number -- a host that keeps streams of its own
 * counts them against the same four.  Without multi_stream=True every blob is the one-stream order it always was.
 * ROCm 7.2 quirk 2: the graph exec of a capture that spans several streams cannot be destroyed
 * safely, and dh_graph_destroy would do just that -- capturing a multi-stream dh_forward is neither promised nor tested;
 * run it eagerly (the two-stream forward costs the same device time eager and replayed).
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_plan dh_plan;
int dh_plan_create(const void* blob, size_t blob_bytes, dh_plan** plan_out);
int dh_plan_destroy(dh_plan* plan);
int dh_plan_batch(const dh_plan* plan);
int dh_plan_num_inputs(const dh_plan* plan);
int dh_plan_num_outputs(const dh_plan* plan);
int64_t dh_plan_input_items(const dh_plan* plan, int i);  /* elements (floats, or bytes of a uint8 input) per batch item */
int dh_plan_input_is_u8(const dh_plan* plan, int i);      /* 1: input i takes raw uint8 frames, 0: float32, -1: no such input */
int64_t dh_plan_output_items(const dh_plan* plan, int i); /* floats per batch item of output i */
int dh_plan_output_channels(const dh_plan* plan, int i);  /* its last dimension (D of a pose output [J, D]); -1: no such output */
int dh_forward(dh_plan* plan, const float* const* inputs_dev, int m, float* const* outputs_dev, void* stream);
int dh_forward_host(dh_plan* plan, const float* const* inputs_host, int m, float* const* outputs_host);
/* The device address dh_forward copies input i to (float inputs; NULL for a uint8 input or no such input).  A caller that
 * WRITES its data there (dh_clip_forward's unpack launch does) passes that same address as inputs_dev[i]: dh_forward then
 * skips the copy of that input -- the strided torch copy per cut tensor that Executor.run_device makes for
 * deephar_amd/parallel.py's head stage has no counterpart here.  A NULL input stays DH_EINVAL. */
float* dh_plan_input_ptr(const dh_plan* plan, int i);
int dh_plan_num_streams(const dh_plan* plan);             /* streams a forward runs on, the caller's included (1: versions 1 - 4) */
/* test aid, like dh_stream_spin_us: the plan's own side stream k (1 <= k < dh_plan_num_streams), so a test can delay it
 * against the caller's stream; NULL for any other k.  The handle belongs to the plan. */
void* dh_plan_side_stream(const dh_plan* plan, int k);
/* The plan blob on its own, GPU-free (csrc/plan_blob.h; dh_plan_create parses with exactly this before it allocates).
 *   inspect: every check of dh_plan_create that needs no device -- magic, version, header limits, the input and output
 *            tables and their extents, every step record (an id the blob's version knows, the payload size of that id, every
 *            tagged pointer inside its region), the schedule section, "the rest is the weight image".  Every malformed or
 *            truncated blob is DH_EINVAL; nothing is allocated on a device.  num_ops / num_events: the enqueue program of a
 *            version-5 blob and the events it needs (0 / 0 and nstreams 1 below version 5).
 *   record : the step record of function id `fn` (the index into serialize.ALL_FUNCTIONS): the entry point dh_forward calls,
 *            the first blob version that knows the id, the payload bytes, and the byte offsets of the payload's pointer slots
 *            (*num_offsets of them; at most max_offsets are written to `offsets`, which may be NULL).  DH_EINVAL outside the
 *            table.  The writer packs from the ctypes signatures; tests/test_plan_blob_host.py holds the two against each other. */
typedef struct dh_plan_info {
  int32_t version, batch, num_inputs, num_outputs, num_steps, nstreams, num_ops, num_events;
  uint64_t arena_bytes, weight_bytes, byte_bytes;   /* regions 1, 2, 3 of the tagged pointers */
} dh_plan_info;
int dh_plan_inspect(const void* blob, size_t bytes, dh_plan_info* out);
int dh_plan_record(int fn, const char** name, int* first_version, size_t* payload_bytes, int32_t* offsets, int max_offsets,
                   int* num_offsets);

/* ---------------------------------------------------------------------------------------------------
 * Every wanted output of a forward in one launch: the counterpart of dh_unpack_cut_f32 at the other end.  dh_forward ends
 * with it (instead of one dh_copy_channels_f32 launch per output), dh_forward_host packs all outputs into one staging
 * buffer with it and reads them back with ONE device-to-host copy.
 *   segment s: dst_s[p * C_s + c] = src_s[p * ld_s + c] for p < npix_s, c < C_s  (npix = pixels per batch item x items;
 *              ld >= C floats; the columns beyond C of the source are not read)
 * `segs` is a table in HOST memory: the segments travel by value in the kernel arguments, at most 64 per launch (more go
 * out as further launches), so nothing is uploaded per call and the launch is capturable.  A segment whose dst is NULL is
 * dropped before the launch.  A segment moves 16 bytes per lane when C and ld are multiples of 4 and both base addresses
 * are 16-byte aligned, one float per lane otherwise (poses: C = 2 / 3, confidences: C = 1, action scores: npix = items);
 * work-groups are dealt to the segments by a prefix table over those units.  Plain vector loads and stores, no atomics.
 * dh_pack_outputs_host: the same index arithmetic as a plain host loop over HOST pointers.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_out_seg { const float* src; float* dst; int64_t npix; int32_t C; int32_t ld; } dh_out_seg;
int dh_pack_outputs_f32(const dh_out_seg* segs, int nseg, void* stream);
int dh_pack_outputs_host(const dh_out_seg* segs, int nseg);
/* 1 when a segment (C, ld) with these base addresses takes the 16-byte path, else 0 */
int dh_pack_outputs_vec4(int C, int ld, const void* src, const void* dst);

/* ---------------------------------------------------------------------------------------------------
 * The schedule of a multi-stream plan as an enqueue program, GPU-free (csrc/plan_sched.h; dh_plan_create and dh_forward
 * run exactly this).  Table: n schedule entries -- step[i] the blob step entry i launches or -1 (its work moved into an
 * earlier grouped / paired launch), stream[i], record[i] != 0 when an event is recorded behind it, and the earlier entries
 * waits[wait_off[i] .. wait_off[i + 1]) it waits for; the first npre entries are input staging; the launching entries name
 * the steps 0 .. nsteps - 1 in order.  DH_EINVAL unless 1 <= nstreams <= 4, every stream < nstreams, the staging entries
 * are on stream 0 without waits or events, every wait names an EARLIER entry that records and sits on ANOTHER stream, and
 * the table sizes agree (wait_off[0] == 0, ascending, wait_off[n] == nwaits).
 * Program: LAUNCH of the staging entries | RECORD fork on stream 0, WAIT fork on every side stream | per entry its WAITs,
 * its LAUNCH (none for -1), its RECORD | per side stream RECORD join on it, WAIT join on stream 0.  A side stream never
 * waits directly on an event of a higher-numbered side stream: stream 0 waits and re-records it on a relay event.
 * Event ids: 0 fork, k the join of side stream k, then one per recording entry, then the relays; *nevents counts them.
 * *nops receives the length of the program; at most max_ops ops are written to `ops` (which may be NULL).
 * ------------------------------------------------------------------------------------------------- */
#define DH_SCHED_LAUNCH 0 /* arg: blob step */
#define DH_SCHED_RECORD 1 /* arg: event id */
#define DH_SCHED_WAIT 2   /* arg: event id */
typedef struct dh_sched_op { int32_t kind; int32_t stream; int32_t arg; int32_t entry; /* -1: fork / join */ } dh_sched_op;
int dh_sched_build_ops(int n, const int32_t* step, const int32_t* stream, const int32_t* record, const int32_t* wait_off,
                       const int32_t* waits, int nwaits, int nstreams, int npre, int nsteps, dh_sched_op* ops, int max_ops,
                       int* nops, int* nevents);

/* ---------------------------------------------------------------------------------------------------
 * The clip boundary in one launch.  Replaces, for a host without Python, what the reference does with Keras slicing
 * Lambdas between the frame stage and the temporal head (action.py:357-366: the per-frame pose / visibility / feature
 * tensors of a clip re-assembled on the time axis; spnet.py:219-235: the same per pyramid of an SPNet) and what
 * deephar_amd/parallel.py's ShardedClipModel does with one strided torch copy per cut tensor.
 *   gathered : the all-gather's result, rank-major [G, m, Tl, P, Cp] floats (G ranks, m clips, Tl frames per rank, P pixels
 *              -- joints -- per frame, Cp packed channels)
 *   segment s: dst_s[n, g * Tl + t, p, 0 : c_s] (pixel pitch ld_s >= c_s floats; columns beyond c_s are not touched)
 *              = gathered[g, n, t, p, coff_s : coff_s + c_s]
 * One launch covers all segments; `segs_dev` is a table in DEVICE memory (a segment that leaves the packed axis or whose
 * pitch is below its channels is skipped by the kernel).  A segment moves 16 bytes per lane when Cp, coff, c and ld are
 * multiples of 4 and both base addresses are 16-byte aligned, one float per lane otherwise (poses: c = 2 / 3,
 * confidences: c = 1).  Plain vector loads and stores, no atomics.  Cp <= 8192.
 * dh_unpack_cut_host: the same index arithmetic as a plain host loop over HOST pointers (segment table included).
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_cut_seg { float* dst; int32_t ld; int32_t coff; int32_t c; int32_t pad; } dh_cut_seg;
int dh_unpack_cut_f32(const float* gathered, int G, int m, int Tl, int64_t P, int Cp, const dh_cut_seg* segs_dev, int nseg,
                      void* stream);
int dh_unpack_cut_host(const float* gathered, int G, int m, int Tl, int64_t P, int Cp, const dh_cut_seg* segs, int nseg);
/* 1 when segment (coff, c, ld) with these base addresses takes the 16-byte path, else 0 */
int dh_unpack_cut_vec4(int Cp, int coff, int c, int ld, const void* gathered, const void* dst);

/* ---------------------------------------------------------------------------------------------------
 * Frame-sharded clip models for hosts without Python: the frame stage, ONE all-gather, the temporal head -- what
 * deephar_amd/parallel.py's ShardedClipModel runs (the reference runs a clip on one GPU:
 * action.py:357-366, spnet.py:219-235).
 *   blob   : written by ShardedClipModel.export_clip_plan(path, clips) (layout: deephar_amd/engine/serialize.py, 'DHCL'):
 *            the cut table and the two plan blobs in one container.
 *   inspect: GPU-free.  Parses and bounds-checks; every malformed or truncated blob is DH_EINVAL; nothing is allocated.
 *            dh_clip_inspect_cut / _output read entry i of the two tables of a blob that inspects clean.
 *   create : this rank's two plans on the current device, the persistent [G, clips, Tl, P, Cp] gather buffer and the
 *            segment table of the unpack launch.  `gather` is the host's collective:
 *              all-gather `floats_per_rank` floats from every rank into `recv`, rank-major (rank r's floats at
 *              recv + r * floats_per_rank), ordered on `stream` (enqueue, do not synchronise); 0 = success.  `send` and
 *              `recv` are device pointers owned by the dh_clip.  The library never calls RCCL itself and does not link
 *              it: the collective enters only here (ncclAllGather(send, recv, floats_per_rank, ncclFloat, comm, stream)
 *              is a complete callback, tools/c_host/predict_clip.c).
 *            NULL is allowed only when world == 1: the packed tensor is then read where the frame plan left it.
 *   forward: m <= clips; frames_dev is this rank's [m, Tl, H, W, C] (float32, or uint8 when dh_clip_input_is_u8);
 *            outputs_dev[k] is a device pointer to the dense float32 [m, ...] output k in MODEL order (NULL: not wanted).
 *            Enqueued on `stream` in this order: frame plan, gather, ONE dh_unpack_cut_f32 launch (head inputs written in
 *            place, pass-through outputs written straight to outputs_dev), head plan.  Nothing synchronises.  The segment
 *            table is uploaded at create and again only when the pass-through pointers differ from the previous call
 *            (that one call waits for `stream` while the table is read: keep the output pointers when capturing a graph).
 *            Results are bit-identical to Model.predict of the exporting process.
 *   forward_host: the same with HOST pointers on an internal stream; returns when done.
 * Serial form only: the two-slot pipelined form of parallel.py (frame stage of step i + 1 under the collective of step i)
 * is out of scope here.  Either stage may be a multi-stream plan (export_clip_plan(path, clips, multi_stream=True)): its
 * dh_forward forks from and joins back into `stream`, so the order above holds.  A dh_clip is not re-entrant.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_clip dh_clip;
typedef struct dh_clip_info {
  int32_t version, world, T, Tl, packed_channels, num_cut, num_outputs, num_head_outputs;
  int64_t P;                                          /* pixels per frame of every cut tensor */
  uint64_t frames_offset, frames_bytes, head_offset, head_bytes;   /* the two plan blobs inside the container; head_bytes 0: no head */
} dh_clip_info;
/* all-gather of `floats_per_rank` floats from every rank, rank-major, stream-ordered on `stream`; world 1: recv = send */
typedef int (*dh_allgather_fn)(void* ctx, const float* send, float* recv, int64_t floats_per_rank, void* stream);
int dh_clip_inspect(const void* blob, size_t bytes, dh_clip_info* out);
int dh_clip_inspect_cut(const void* blob, size_t bytes, int i, int32_t* channel_offset, int32_t* channels);
int dh_clip_inspect_output(const void* blob, size_t bytes, int k, int32_t* is_head, int32_t* index);
int dh_clip_create(const void* blob, size_t bytes, int rank, dh_allgather_fn gather, void* ctx, dh_clip** out);
int dh_clip_forward(dh_clip* clip, const void* frames_dev, int m, float* const* outputs_dev, void* stream);
int dh_clip_forward_host(dh_clip* clip, const void* frames_host, int m, float* const* outputs_host);
int dh_clip_destroy(dh_clip* clip);
int dh_clip_world(const dh_clip* clip);
int dh_clip_batch(const dh_clip* clip);                     /* clips per step the plans were made for */
int dh_clip_num_outputs(const dh_clip* clip);
int64_t dh_clip_output_items(const dh_clip* clip, int k);   /* floats per clip of model output k */
int64_t dh_clip_frame_items(const dh_clip* clip);           /* elements per clip of this rank's frames: Tl * H * W * C */
int dh_clip_input_is_u8(const dh_clip* clip);

/* ---------------------------------------------------------------------------------------------------
 * Crop-and-resize front end: full frames + integer boxes in, the network's uint8 input out, in ONE launch per chunk.
 * Replaces the TEST-MODE crop of the reference's loaders -- T.rotate_crop(0, objpos, winsize), T.resize(crop_resolution),
 * optional T.horizontal_flip() (deephar/utils/transform.py:56-120 as deephar/data/mpii.py:114-118 and pennaction.py:157-161
 * call it), i.e. PIL's Image.crop(box).resize(size, BILINEAR) [.transpose(FLIP_LEFT_RIGHT)] on 8-bit RGB -- bit for bit:
 * PIL's 8-bit resize is integer arithmetic on fixed-point coefficients, restated in csrc/crop_index.h.
 *   crop   : C[y, x] = S[y0 + y, x0 + x] inside the image, 0 outside; cw = x1 - x0, ch = y1 - y0.
 *   axis   : (in, out) = (cw, OW) or (ch, OH), all in double, never fused: scale = in / out, fs = max(scale, 1), support = fs,
 *            ss = 1 / fs; output i: center = (i + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)),
 *            xmax = min(in, (int)(center + support + 0.5)), w_j = max(0, 1 - |(j + xmin - center + 0.5) * ss|) normalised by
 *            their sum, k_j = (int)(0.5 + w_j * 2^22).
 *   passes : horizontal, then vertical: out = clip_0_255((2^21 + sum_j k_j * in[xmin + j]) >> 22); the horizontal result is
 *            rounded to uint8 before the vertical pass reads it (it lives in LDS, never in memory); int32 accumulators.
 *   flip   : hflip reverses the columns of the result.
 * Scope: angle 0, integer window, bilinear, 3 channels, uint8; per-axis down-scaling up to 16 (33 taps), any up-scaling.
 * Rotation, random augmentation and file decoding stay with the caller.  The reference pins Pillow 5.1.0; the fixtures of
 * the tests were produced with the Pillow they record (12.2.0) -- equality with 5.1.0 itself is not verified.
 * A CROP PROGRAM is one contiguous table the host builds and the launch reads: the source descriptors, the jobs, and per job
 * both axes' first / count / k tables (layout: csrc/crop_index.h).  The size query answers its bytes, the builder fills HOST
 * memory (8-byte aligned) that the caller copies to the device as it likes; the sources' `ptr` are the addresses the READER
 * will use (device pointers for the launch, host pointers for the host twin).  Output item j (job j) is [OH, OW, 3] bytes at
 * y + j * item_pitch.  One work-group owns a band of output rows of one job; rows move 16 bytes per lane when 3 * OW, y and
 * item_pitch are multiples of 16 (a 256 x 3 row is), one byte per lane otherwise.  No atomics.  Nothing allocates, nothing
 * synchronises.  DH_EINVAL: NULL pointer, empty box, pitch < 3 * W, item_pitch < OH * OW * 3, a malformed program (builder
 * and host twin; the launch cannot read device memory and trusts what the builder wrote).  DH_EUNSUPPORTED: a window beyond
 * the scale cap, or an output so wide that the rows one output row reads do not fit LDS -- answered by the size query, the
 * builder and the host twin, which then write nothing.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_crop_src { const uint8_t* ptr; int64_t pitch; /* bytes between rows, >= 3 * W */ int32_t H, W; } dh_crop_src;
typedef struct dh_crop_job { int32_t src; int32_t x0, y0, x1, y1; /* window [x0, x1) x [y0, y1), may leave the image */
                             int32_t hflip; } dh_crop_job;
int dh_crop_program_bytes(const dh_crop_job* jobs, int njobs, int nsrc, int OH, int OW, size_t* bytes);
int dh_crop_program_build_host(const dh_crop_src* srcs, int nsrc, const dh_crop_job* jobs, int njobs, int OH, int OW,
                               void* program_host, size_t bytes);
int dh_crop_resize_u8(const void* program_dev, int njobs, int OH, int OW, uint8_t* y, int64_t item_pitch, void* stream);
int dh_crop_resize_host(const void* program_host, size_t bytes, int njobs, int OH, int OW, uint8_t* y, int64_t item_pitch);
/* one axis on its own (what the builder writes per job and axis): taps per output row of k, and the three tables
 * first[out], count[out], k[out * taps] with taps >= dh_crop_axis_taps(in, out) */
int dh_crop_axis_taps(int in, int out);
int dh_crop_axis_coeffs_host(int in, int out, int taps, int32_t* first, int32_t* count, int32_t* k);
/* The crop program built ON THE DEVICE from a job table in device memory, for callers whose boxes never visit the host.
 *   max_bytes: what a program of njobs jobs over nsrc sources can take at most (both axis tables of every job at the 33 taps
 *            of the scale cap): what the caller allocates before the boxes are known.  >= dh_crop_program_bytes of every
 *            table that query accepts.  DH_EINVAL: njobs / nsrc < 1, extents, NULL; DH_EUNSUPPORTED: above 2^31 - 1 bytes.
 *   build_dev: srcs_dev (8-byte aligned), jobs_dev, program_dev (8-byte aligned, `capacity` bytes) and status_dev (njobs
 *            int32, may be NULL) are DEVICE memory; two small launches on `stream` (layout: one work-group validates the
 *            jobs, scans their table sizes into offsets, writes header, source table and job records; tables: one work-group
 *            per job and axis, one lane per output index), nothing synchronises, no atomics.  The doubles are the host
 *            builder's, operation for operation, with contraction into fused multiply-adds switched off on both sides
 *            (csrc/crop_index.h): for a table in which every job is good, the first header.bytes bytes of program_dev are,
 *            byte for byte, what dh_crop_program_build_host writes for the same sources and jobs, and header.bytes is what
 *            dh_crop_program_bytes answers.  Nothing is written at or beyond program_dev + header.bytes.
 *            A job that is no good -- empty box, source index out of range, a source descriptor dh_crop_program_build_host
 *            would refuse (status DH_EINVAL), or a window beyond the scale cap (DH_EUNSUPPORTED) -- gets a record without
 *            tables that dh_crop_resize_u8 skips: its output item is left untouched, the other jobs run; status[j] of a good
 *            job is DH_OK.  Reading the status back is the caller's business (and a synchronisation).
 *            Refused on the host, before anything is enqueued: DH_EINVAL for NULL / misaligned pointers, extents and
 *            capacity < max_bytes; DH_EUNSUPPORTED when 33 rows of the output width do not fit LDS (OW > 661: narrower than
 *            what the host builder takes for windows of small scale, because here the scale is not known on the host). */
int dh_crop_program_max_bytes(int njobs, int nsrc, int OH, int OW, size_t* bytes);
int dh_crop_program_build_dev(const dh_crop_src* srcs_dev, int nsrc, const dh_crop_job* jobs_dev, int njobs, int OH, int OW,
                              void* program_dev, size_t capacity, int32_t* status_dev /* may be NULL */, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Frames and boxes through a plan, for hosts without Python: what deephar_amd/frontend.py's predict_from_frames does.
 *   frames : dh_frames_create uploads n full uint8 [H, W, 3] frames ONCE (frames_host[i].ptr is HOST memory, pitch >= 3 * W
 *            bytes between rows; sizes may differ) and keeps the device source table dh_frames_table_dev returns (n
 *            descriptors with device `ptr`, dense rows) -- what dh_crop_program_build_dev takes as srcs_dev.  Create and
 *            destroy synchronise; DH_EINVAL: NULL, n < 1, a descriptor with NULL ptr / H or W < 1 / pitch < 3 * W.
 *   forward_frames: `plan` has exactly one input and it is uint8 (Model.export_plan(path, batch, uint8=True)).  The blob does
 *            not carry the input's height and width, so the caller states OH and OW: dh_plan_input_items(plan, 0) must be
 *            T * OH * OW * 3 for a whole T (1: an image model; T frames per clip of a clip model) and njobs = m * T for an
 *            m in [1, dh_plan_batch]; job j is frame j % T of item j / T.  Anything else is DH_EINVAL
 *            (dh_forward_frames_shape is that test on its own, GPU-free; it answers m and T).
 *            jobs_dev is DEVICE memory (src indexes the frames of `f`).  Enqueued on `stream`, in this order:
 *            dh_crop_program_build_dev into the plan's program buffer (allocated on first use for a full batch, freed by
 *            dh_plan_destroy), dh_crop_resize_u8 straight into the plan's uint8 input, the forward of dh_forward with its
 *            input copy skipped.  Nothing synchronises.  A multi-stream plan runs the two launches on `stream` in front of
 *            its fork.  A job the builder refuses leaves its frame of the input as the previous call left it: a caller
 *            that cannot vouch for its boxes calls dh_crop_program_build_dev itself and reads the status.
 *            outputs_dev as in dh_forward.  Results are bit-identical to predict_from_frames of the exporting process.
 *   forward_frames_host: jobs and outputs are HOST memory; the table is validated on the host first (dh_crop_program_bytes:
 *            a bad table is refused with that code before anything is enqueued), staged, run on the plan's internal stream;
 *            returns when the outputs are on the host, like dh_forward_host.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_frames dh_frames;
int dh_frames_create(const dh_crop_src* frames_host, int n, dh_frames** out);
int dh_frames_destroy(dh_frames* f);
int dh_frames_count(const dh_frames* f);
const dh_crop_src* dh_frames_table_dev(const dh_frames* f);
int dh_forward_frames_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int njobs, int OH, int OW, int* m,
                            int* frames_per_item);
int dh_forward_frames(dh_plan* plan, const dh_frames* f, const dh_crop_job* jobs_dev, int njobs, int OH, int OW,
                      float* const* outputs_dev, void* stream);
int dh_forward_frames_host(dh_plan* plan, const dh_frames* f, const dh_crop_job* jobs_host, int njobs, int OH, int OW,
                           float* const* outputs_host);

/* ---------------------------------------------------------------------------------------------------
 * Box refinement on the device: the pose -> box -> re-crop loop of the MPII evaluation (exp/common/mpii_tools.py:13-52 in
 * the reference, deephar_amd/evaltools/bbox.py: refine_pred_frames) with the boxes resident in device memory -- the caller
 * dh_crop_program_build_dev was made for.  The arithmetic is csrc/refine_index.h, in double, never fused, the same bits on
 * the host (`_host` twins over host pointers) and on the device.
 *   window of a float box b = (bx0, by0, bx2, by2) -- crop_box(*bbox_to_objposwin(b)): cx = (bx0 + bx2) / 2, w = bx2 - bx0
 *            (cy, h likewise); corners cx - w/2, cy - h/2, cx + w/2, cy + h/2, each truncated toward zero to int32.  A corner
 *            that is not finite or of magnitude >= 2^31 makes the job the EMPTY job (src, 0, 0, 0, 0, 0), which the program
 *            builders refuse (DH_EINVAL) and dh_crop_program_build_dev skips.
 *   jobs_from_boxes: jobs[i] = (src[i], window of boxes[4 i .. 4 i + 3], hflip 0), one lane per sample.
 *   refine_boxes: per sample i, from job (src, x0, y0, x1, y1, hflip), box b and the J joints (u_j, v_j) of its pose in
 *            crop-normalised coordinates (float32 at poses[i * sample_stride + j * joint_stride + {0, 1}], strides in floats:
 *            the launch reads a plan's output where it lies in the arena): cw = x1 - x0, ch = y1 - y0; ulo, uhi, vlo, vhi the
 *            min / max over the joints; lx = x0 + ulo cw, hx = x0 + uhi cw, ly = y0 + vlo ch, hy = y0 + vhi ch; p = the
 *            centre of that extent; side = winsize_scale max(hx - lx, hy - ly); t = the centre of b; o = momentum t +
 *            (1 - momentum) p; the new box is o -+ side / 2 and the new job its window with the same src, unflipped.  An input
 *            job that is flipped or empty yields the empty job and passes its box through; a NaN joint coordinate makes the
 *            box NaN (every NaN leaves as the one quiet NaN 0x7ff8000000000000) and the job empty.  Joints are not filtered.
 *            One wavefront per sample, lanes over the joints, cross-lane min / max (exact: no order dependence), lane 0 does
 *            the doubles.  boxes_out / jobs_out may alias the inputs.  No atomics; nothing allocates, nothing synchronises.
 *   DH_EINVAL: NULL (or misaligned device) pointers, n < 1, J < 1, joint_stride < 2, sample_stride < (J - 1) joint_stride + 2.
 *   refine_frames_host: the whole num_iter-pass loop of ONE batch (n <= dh_plan_batch) from a C host: src (frame indices into
 *            `f`) and boxes0 (float64 [n, 4]) are uploaded once; per iteration dh_crop_program_build_dev from the resident job
 *            table (status kept per job), dh_crop_resize_u8 into the plan's input, the forward, and -- but for the last --
 *            dh_refine_boxes_f64 on output `outidx` in the arena, all on the plan's internal stream with ONE synchronisation
 *            at the end.  poses_out [num_iter, n, J, D] are the RAW outputs (crop-normalised; the image-space poses follow on
 *            the host from jobs_out), jobs_out [num_iter, n] the windows every iteration cropped, status_out [num_iter, n] the
 *            builder's codes (a refused job leaves its input frame as the previous iteration left it).
 *   refine_frames_shape: the refusals of refine_frames_host on their own, GPU-free: more than one input, a float input, a clip
 *            plan (input_items != OH * OW * 3), n outside [1, batch], num_iter < 1, outidx outside [0, num_outputs), an output
 *            of fewer than two channels (out_channels: dh_plan_output_channels; out_items: dh_plan_output_items).  Answers J.
 * ------------------------------------------------------------------------------------------------- */
int dh_jobs_from_boxes_f64(const double* boxes, const int32_t* src, int n, dh_crop_job* jobs, void* stream);
int dh_jobs_from_boxes_host(const double* boxes, const int32_t* src, int n, dh_crop_job* jobs);
int dh_refine_boxes_f64(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                        const double* boxes_in, int n, double winsize_scale, double momentum, double* boxes_out,
                        dh_crop_job* jobs_out, void* stream);
int dh_refine_boxes_host(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                         const double* boxes_in, int n, double winsize_scale, double momentum, double* boxes_out,
                         dh_crop_job* jobs_out);
int dh_refine_frames_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW, int num_outputs,
                           int outidx, int64_t out_items, int out_channels, int num_iter, int* J);
int dh_refine_frames_host(dh_plan* plan, const dh_frames* f, const int32_t* src, const double* boxes0, int n, int OH, int OW,
                          int outidx, int num_iter, double winsize_scale, double momentum,
                          float* poses_out /* [num_iter, n, J, D] raw */, dh_crop_job* jobs_out /* [num_iter, n] */,
                          int32_t* status_out /* [num_iter, n] */);

/* ---------------------------------------------------------------------------------------------------
 * Person boxes from predicted poses on the device: the pose -> box step of the per-frame box pass (exp/common/generic.py:7-27
 * and exp/{ntu,pennaction}/predict_bboxes.py in the reference, deephar_amd/evaltools/bbox.py: get_bbox_from_poses,
 * predict_frame_bboxes_frames) as one small launch behind the forward, so that 52 bytes per item leave the device instead of
 * the packed outputs.  The arithmetic is csrc/posebox_index.h: float32 where numpy keeps the float32 pose, double for the
 * pixels, never fused, the same bits on the host (`_host` twin over host pointers) and on the device.
 *   An ITEM is F poses (F = 1 for an image model, F = T for a clip model) of J joints, all predicted in ONE unflipped integer
 *   window (x0, y0, x1, y1): job jobs[i * job_stride] of the crop job table (job_stride = frames per item).  Joint j of frame f
 *   is float32 at poses[i * item_stride + f * frame_stride + j * joint_stride + {0, 1, conf_channel}] (strides in floats: the
 *   launch reads a plan's output where it lies in the arena).
 *   kept:    joint j of frame f is kept when its channel conf_channel is > 0.25 as a float32 comparison (the Python side
 *            passes D - 2, the reference's poses[..., -2:-1]); a NaN confidence keeps nothing.
 *   span:    per frame, in float32, over the kept joints: cx = (xmin + xmax) / 2, w = relsize (xmax - xmin) (cy, h likewise;
 *            relsize is the double rounded once to float32), s = max(w, h); corners cx - s/2, cy - s/2, cx + s/2, cy + s/2.
 *   union:   the exact float min of the first two and max of the last two corners over the item's frames: (u0, v0, u1, v1).
 *   pixels:  X = x0 + (double)u (x1 - x0), Y = y0 + (double)v (y1 - y0) for both corners, each product and each sum one IEEE
 *            double operation; the two corners ordered by min / max; boxes_f64_out[4 i ..] holds them, boxes_out[4 i ..] each
 *            truncated toward zero (numpy's astype(int)).
 *   status_out[i]: 0 ok; 1 a frame of the item keeps no joint (the reference raises ValueError('get_valid_bbox: all points
 *            are invalid!')); 2 a kept joint has a NaN coordinate; 3 a corner is not finite or of magnitude >= 2^31; 4 the window
 *            is empty or flipped.  When several hold: 1, else 2, else 4, else 3.  A non-zero status writes both boxes as four
 *            zeros; no NaN is stored and no unrepresentable double is converted.
 *            One wavefront per item, lanes over the joints, cross-lane min / max per frame (exact: no order dependence), lane 0
 *            does the doubles.  No atomics; nothing allocates, nothing synchronises.
 *   DH_EINVAL: NULL (or misaligned device) pointers; n < 1, F < 1, J < 1; conf_channel < 0; job_stride < 1; with e = max(2,
 *            conf_channel + 1) the floats a joint spans: joint_stride < e, frame_stride < (J - 1) joint_stride + e, item_stride
 *            < (F - 1) frame_stride + (J - 1) joint_stride + e; any stride above 2^40; (n - 1) item_stride or (n - 1) job_stride
 *            above 2^58.
 *   frame_boxes_host: the pass of ONE batch (n <= dh_plan_batch, single-image uint8 plans) from a C host: src (frame indices
 *            into `f`) and windows (int32 [n, 4]) become the job table, uploaded once; dh_crop_program_build_dev,
 *            dh_crop_resize_u8 into the plan's input, the forward (no output is packed), dh_pose_boxes_f64 on output `outidx`
 *            in the arena with conf_channel = D - 2, and three small copies back, all on the plan's internal stream with ONE
 *            synchronisation.  A window the host program builder refuses (empty, a frame index outside `f`, beyond the 16x scale
 *            cap) is refused here, with its code, before anything is enqueued.
 *   frame_boxes_shape: the refusals of frame_boxes_host on their own, GPU-free: more than one input, a float input, a clip
 *            plan (input_items != OH * OW * 3), n outside [1, batch], outidx outside [0, num_outputs), an output of fewer than
 *            two channels (out_channels: dh_plan_output_channels; out_items: dh_plan_output_items).  Answers J.
 * ------------------------------------------------------------------------------------------------- */
int dh_pose_boxes_f64(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                      int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, double relsize,
                      int32_t* boxes_out /* [n, 4] */, double* boxes_f64_out /* [n, 4] */, int32_t* status_out /* [n] */,
                      void* stream);
int dh_pose_boxes_host(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                       int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, double relsize, int32_t* boxes_out,
                       double* boxes_f64_out, int32_t* status_out);
int dh_frame_boxes_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW, int num_outputs,
                         int outidx, int64_t out_items, int out_channels, int* J);
int dh_frame_boxes_host(dh_plan* plan, const dh_frames* f, const int32_t* src, const int32_t* windows /* [n, 4] */, int n, int OH,
                        int OW, int outidx, double relsize, int32_t* boxes_out /* [n, 4] */, double* boxes_f64_out /* [n, 4] */,
                        int32_t* status_out /* [n] */);

/* ---------------------------------------------------------------------------------------------------
 * The multi-clip action vote on the device: the product of the per-clip class probabilities of every sequence and the running
 * arg-max label behind every clip (exp/common/penn_tools.py:85-163, exp/common/ntu_tools.py:53-152 in the reference,
 * deephar_amd/evaltools/action.py: _multiclip, vote_products, multiclip_votes_frames) as one small launch behind the forward, so
 * that no model output leaves the device.  The arithmetic is csrc/vote_index.h: the same bits on the host (`_host` twin over host
 * pointers) and on the device.
 *   An ITEM k is one clip's result: nb rows of C float32 class probabilities, row k of output b at srcs[b].p + k *
 *   srcs[b].item_stride (strides in floats: the launch reads a plan's outputs where they lie in the arena), of sequence seq[k].
 *   `srcs` is a HOST table: it travels by value in the kernel arguments, at most 32 sources per launch, more as further launches
 *   over disjoint b; nothing is uploaded per call and the launches are capturable.
 *   For k = 0 .. n-1 IN THAT ORDER and every b:
 *     acc[b, seq[k], c] *= (double)p_b[k, c]      one IEEE double multiply per class; the caller initialises acc to 1.0
 *     label_out[b, k]    = argmax_c acc[b, seq[k], :] with np.argmax's rule: the first maximum wins, a NaN beats every number,
 *                          the first NaN wins (+0 and -0 are equal)
 *     scores_out[b, k, c] = p_b[k, c]             if scores_out is not NULL
 *   Items need not be sorted by sequence.  Two calls over [0, n1) and [n1, n) with the same acc equal one call over [0, n) bit
 *   for bit (label_out and scores_out are dense [nb, n(, C)] of EACH call).  There is no status word: products go subnormal,
 *   reach zero or become inf * 0 = NaN as numpy's do; double denormals are not flushed.  seq is device data: an item whose
 *   seq[k] is outside [0, nseq) is skipped -- label -1, acc and its scores_out rows untouched.
 *   One wavefront per output b, lanes over the classes, a serial loop over the items, a cross-lane arg-max under a total order
 *   (no order dependence).  No atomics; nothing allocates, nothing synchronises.
 *   DH_EINVAL: NULL or misaligned pointers (acc to 8 bytes, the rest to 4; scores_out may be NULL); nb < 1, C < 1, n < 1,
 *            nseq < 1; an item_stride < C or above 2^40; (n - 1) item_stride, nb nseq C or nb n C above 2^58.
 * ------------------------------------------------------------------------------------------------- */
typedef struct dh_vote_src { const float* p; int64_t item_stride; } dh_vote_src;   /* row k at p + k * item_stride, C dense floats */
int dh_vote_products_f64(const dh_vote_src* srcs /* HOST table */, int nb, int C, const int32_t* seq /* device [n] */, int n,
                         int nseq, double* acc /* device [nb, nseq, C], in/out */, int32_t* label_out /* device [nb, n] */,
                         float* scores_out /* device [nb, n, C] or NULL */, void* stream);
int dh_vote_products_host(const dh_vote_src* srcs, int nb, int C, const int32_t* seq /* [n] */, int n, int nseq,
                          double* acc /* [nb, nseq, C], in/out */, int32_t* label_out /* [nb, n] */,
                          float* scores_out /* [nb, n, C] or NULL */);

/* ---------------------------------------------------------------------------------------------------
 * Stream-ordered runtime helpers (no torch types): graphs for launch-bound replay, events for timing.
 * ------------------------------------------------------------------------------------------------- */
int dh_graph_begin_capture(void* stream);
int dh_graph_end_capture(void* stream, void** graph_exec_out);
int dh_graph_launch(void* graph_exec, void* stream);
int dh_graph_destroy(void* graph_exec);

int dh_event_create(void** event_out);
int dh_event_record(void* event, void* stream);
int dh_event_synchronize(void* event);
int dh_event_elapsed_ms(void* start, void* stop, float* ms_out);
int dh_event_destroy(void* event);
int dh_stream_synchronize(void* stream);
/* extra non-blocking streams + cross-stream ordering, so independent branches of a model can be captured as
 * parallel branches of one hipGraph (fork: side stream waits on an event of the origin stream; join: origin waits
 * on an event recorded at the tail of every side stream) */
int dh_stream_create(void** stream_out);
int dh_stream_destroy(void* stream);
int dh_event_create_sync(void** event_out); /* hipEventDisableTiming */
int dh_stream_wait_event(void* stream, void* event);
/* test aid for multi-stream schedules: one idle wave occupies `stream` for about `us` microseconds (<= 20 000), so a
 * test can delay one stream of a plan against the others and check that every cross-stream dependency is an event wait
 * (tests/test_gpu_speed2d.py: the 'tail' policy of the latency regime under random delays). */
int dh_stream_spin_us(void* stream, int us);

#ifdef __cplusplus
}
#endif
#endif /* DEEPHAR_HIP_H_ */
