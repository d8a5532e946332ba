/*
 * imvoxel.h -- C-ABI of libimvoxel_hip.so, the MI355X (gfx950) implementation of the
 * ImVoxelNet forward hot path.
 *
 * Boundary convention.  The reference reaches native code on this
 * path in exactly two ways:
 *   (1) torch.nn ops (Conv2d/Conv3d/BatchNorm/ReLU/max_pool/interpolate/bmm/index/topk)
 *       that dispatch into cuDNN/cuBLAS, and
 *   (2) its own pybind module iou3d_cuda:  int nms_gpu(Tensor boxes, Tensor keep,
 *       float thr, int device_id)   (mmdet3d/ops/iou3d/src/iou3d.cpp:95-147,203-208).
 * Every entry point below replaces one of those call sites and keeps convention (2):
 * plain pointers + sizes, caller-owned buffers, int status return (0 = ok, <0 = error;
 * the library never exit()s, unlike gpuAssert at iou3d.cpp:27-36), no torch types, no
 * hidden allocation, asynchronous on the HIP stream handed in (hipStream_t as void*;
 * NULL = the default stream).  All pointers are DEVICE pointers unless marked "host".
 *
 * Layouts: activations are channels-last fp32 -- NHWC for 2-D, NDHWC for 3-D (a 2-D
 * tensor is the D == 1 case).  For the feature volume the reference's (X, Y, Z) axes are
 * (D, H, W), so a voxel's C channels are contiguous and z is the fastest spatial axis,
 * matching the reference's flat voxel index n = (i*Y + j)*Z + k
 * (mmdet3d/models/detectors/imvoxelnet.py:148).
 */
#ifndef IMVOXEL_H_
#define IMVOXEL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVX_OK 0
#define IVX_ERR_INVALID_ARG (-1)
#define IVX_ERR_HIP (-2)
#define IVX_ERR_UNSUPPORTED (-3)
#define IVX_ERR_WORKSPACE (-4)

typedef void *ivx_stream_t; /* hipStream_t */

/* Library version (major*10000 + minor*100 + patch; 400 = 0.4.0, the struct layouts of this header; 420 = 0.4.2: bf16 storage with
 * DCNv2 stages and the LayoutHead, ivx_dcn_im2col_fwd_bf16 / ivx_global_avgpool_fwd_bf16; 430 = 0.4.3: ivx_image_prep_u8 / ivx_rescale_size; 440 = 0.4.4: ivx_backproject_fwd_ex / ivx_model_cfg.sampling, the optional
 * bilinear sampling rule of the unprojection; 450 = 0.4.5: ivx_conv_route / ivx_bf16_pair_pack_filters; 460 = 0.4.6: ivx_backproject_gather_fwd, the mean lift of
 * views listed by slot, for sliding-window scenes; 470 = 0.4.7: ivx_backproject_lists_fwd, the listed lift with per-sample rows and `first` flags, for
 * batches of scenes and ragged batches; 480 = 0.4.8: ivx_backproject_weighted_fwd / ivx_volume_wmean_fwd, the listed lift with per-view weights,
 * per-sample decay and a forgetting threshold, for fading scenes; 490 = 0.4.9: ivx_volume_scroll_fwd, the in-place voxel shift of rows of the state
 * pools, for scrolling scenes; 500 = 0.5.0: ivx_backproject_mapped_fwd, the weighted lift with a per-pixel confidence map and a gated depth map
 * per view; 501 = 0.5.1: ivx_view_coverage_fwd, the integer count of the voxels a candidate view would see and of those the scene has no evidence
 * for yet, before its trunk runs; 502 = 0.5.2: ivx_image_prep_lens_u8 / ivx_map_prep_lens, the image pipeline through a lens model (undistortion
 * in the prep launch) and the cover / depth maps of the same geometry at feature resolution; 503 = 0.5.3: ivx_image_prep_fmt_u8 / ivx_yuv_matrix, the image pipeline on decoder pixel
 * formats (RGB, BGRA / RGBA, gray, NV12, YUYV) converted in the fetch of the prep launch; 540 = 0.5.4: ivx_volume_warp_fwd, the rigid out-of-place
 * resample of rows of the state pools, for scenes that turn with their platform; 550 = 0.5.5: ivx_volume_merge_fwd, the rigid in-place merge of
 * rows of the state pools, for scenes that become one; 560 = 0.5.6: ivx_volume_pack_fwd / ivx_volume_unpack_fwd / ivx_volume_pack_scratch_bytes, the
 * ordered compaction of the seen voxels of rows of the state pools and its inverse, for scene snapshots; 570 = 0.5.7: ivx_volume_match_fwd /
 * ivx_volume_match_scratch_bytes, the read-only scoring of candidate poses between two rows of the state pools, for matching scenes; 580 = 0.5.8: ivx_volume_align_fwd / ivx_volume_align_scratch_bytes, the Gauss-Newton
 * normal equations of a six-DoF pose between two rows of the state pools, for aligning scenes) and the message of the last failing call on this
 * thread (never NULL). */
int ivx_version(void);
const char *ivx_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Channels-last convolution with fused epilogue -- replaces nn.Conv2d / nn.Conv3d followed
 * by eval-mode BatchNorm, residual add and ReLU:
 *   ResNet-50 / FPN call sites  mmdet3d/models/detectors/imvoxelnet.py:48,50
 *   3-D necks                   mmdet3d/models/necks/imvoxelnet.py:46-60,99-113,181-230
 *   head convs                  mmdet3d/models/dense_heads/anchor3d_head.py:122-153
 *
 *   out[b,do,ho,wo,co] = act( (sum_{kd,kh,kw,ci} in[b, do*sd-pd+kd, ho*sh-ph+kh, wo*sw-pw+kw, ci]
 *                              * wgt[co,kd,kh,kw,ci]) * scale[co] + shift[co] + res[...] )
 *
 * in    [B,D,H,W,Cin]   Cin % 4 == 0 (pad the image to 4 channels with ivx_nchw_to_nhwc)
 * wgt   wgt_layout 0: [Cout,KD,KH,KW,Cin]   (k = tap*Cin + ci)
 *       wgt_layout 1: [Cout,Cin/32,KD,KH,KW,32]  (k = (ci/32)*taps*32 + tap*32 + ci%32; needs Cin % 32 == 0).
 *       Layout 1 walks all taps of one 32-channel chunk back to back, so the 27 shifted re-reads of an input row
 *       are one K-slab apart and hit L1/L2 instead of going back to the fabric.
 * scale,shift [Cout] or NULL (1 / 0).  Conv bias and BN fold into them on the host.
 * Epilogue order: v = acc*scale + shift; [v += res]; [ReLU]; [v += res if res_after_act]; v *= post_scale.
 * res   NULL, or res_mode 1: same shape as out; res_mode 2: [B,1,res_h,res_w,Cout] read with
 *       nearest-neighbour up-sampling to (Ho,Wo) (FPN top-down path, F.interpolate 'nearest').
 * Arithmetic: fp32 inputs, fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate -- the reference's precision and
 * the default.  Optional reduced-precision storage (the reference has no such mode; BASELINE config 5):
 *   in_dtype  IVX_BF16: in and wgt are bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulate); needs Cin % 8 == 0,
 *             wgt_layout 1 then uses 64-channel chunks [Cout,Cin/64,KD,KH,KW,64]; scale/shift stay fp32.
 *   out_dtype IVX_BF16: out and res are bf16 (epilogue in fp32, one round-to-nearest-even at the store).  */
#define IVX_F32 0
#define IVX_BF16 1
#define IVX_FP8 2      /* OCP e4m3 bytes (gfx950) with a per-tensor scale kept by the caller: see res_scale below */
/* in_dtype only.  Split-operand fp32: every fp32 value x of `in` and `wgt` is stored as the bf16 pair hi = bf16(x),
 * lo = bf16(x - hi) (round to nearest even; hi + lo carries 16 significant bits of x), channels in groups of 16 as
 * [hi c0..c15 | lo c0..c15] (4 bytes per value, like fp32).  The contraction issues hi*hi + hi*lo + lo*hi on the bf16 matrix
 * cores (v_mfma_f32_32x32x16_bf16, 16x the fp32 MFMA rate) with fp32 accumulation: products are exact in fp32, the dropped lo*lo
 * term and the pair rounding are each <= 2^-17 of the product -- 64x finer than the TF32 operands the reference's cuDNN
 * convolutions use by default on its published GPUs, and below the rounding of the F(6x6,3x3) form of the fp32 path (measured in
 * DESIGN.md 4.1e).  Cin (real channels) % 16 == 0; wgt_layout 1 needs Cin % 32 == 0 (64 stored elements per 128-byte chunk);
 * out_mode 0; out / res / scale / shift as for IVX_F32 input.  ivx_bf16_pair_split makes the activation operand, the caller packs
 * the filters the same way once (imvoxelnet_amd/conv.py: pack_pair_weights). */
#define IVX_BF16_PAIR 3
/* The same with fp16 halves: hi = fp16(s*x), lo = fp16(s*x - hi) for a power-of-two tensor scale s kept by the caller (folded into
 * scale[] like the fp8 scales).  hi + lo carries 22 significant bits (pair rounding <= 2^-23, dropped lo*lo <= 2^-22 of a product:
 * fp32-level), at the price of fp16's range: |s*x| must stay below 65504 (ivx_f16_pair_split saturates) and values below
 * 2^-14 * 2^11 = 0.125 lose relative (not absolute: fp16 subnormals, spacing 2^-24) precision in lo.  Used by the Winograd-domain
 * GEMMs (ivx_conv_desc.wino_operands), where operand precision is amplified by the output transform and bf16 pairs are not enough. */
#define IVX_F16_PAIR 4
typedef struct ivx_conv_desc {
  int32_t B, D, H, W, Cin;
  int32_t Cout, KD, KH, KW;
  int32_t sd, sh, sw;
  int32_t pd, ph, pw;
  int32_t relu;
  int32_t res_mode, res_h, res_w;
  int32_t wgt_layout;
  int32_t out_mode;      /* 0: normal.  1: nn.ConvTranspose3d(kernel 2, stride 2) as a 1x1x1 GEMM with
                            Cout = 8*C columns n = ((a*2+e)*2+f)*C + co, scattered to out[b, 2d+a, 2h+e, 2w+f, co]
                            (out is [B,2D,2H,2W,C]; scale/shift have C entries; res, if any, has the out shape) */
  int32_t res_after_act; /* 1: the residual is added after the ReLU (skip adds of the U-shaped necks) */
  float post_scale;      /* final multiplier, 0 or 1 = none (Atlas neck: (x + y) / 2) */
  int32_t in_dtype;      /* IVX_F32 (default), IVX_BF16, IVX_FP8 or IVX_BF16_PAIR: element type of in and wgt */
  int32_t out_dtype;     /* IVX_F32 (default), IVX_BF16 or IVX_FP8: element type of out and res */
  float res_scale;       /* multiplier of the residual before it is added, 0 or 1 = none.  IVX_FP8 tensors are e4m3 bytes with a
                            per-tensor scale kept by the caller (x = byte_value * s_x): the caller folds s_in * s_wgt[co] / s_out
                            into scale[], 1 / s_out into shift[] and passes res_scale = s_res / s_out; the store saturates at
                            +-448 (+-inf included) and rounds to nearest even; a NaN is stored as a NaN byte (0x7F / 0xFF), and one
                            that reaches the ReLU as 0, as in every epilogue (v > 0 ? v : 0).  fp8 input needs Cin % 16 == 0
                            (wgt_layout 1: Cin % 128 == 0). */
  int32_t wino_operands; /* ivx_conv_winograd_* only (in / out stay fp32): operand type of the transformed-domain GEMMs.  IVX_F32 (0,
                            default): fp32 MFMA, exact fp32 arithmetic.  IVX_F16_PAIR: the input / filter transforms write V and U as
                            fp16 (hi, lo) pairs (power-of-two scales taken from max |in| / max |U| on the device, undone exactly by the
                            output transform; the workspace's last 256 bytes carry them between the stages) and the GEMMs issue three
                            fp16 MFMA products per pair -- same bytes, ~3.3x the GEMM rate, error at the level of the fp32 form's own
                            rounding.  Needs tile 4 or 6 and Cin % 16 == 0 (wgt_layout 1: Cin % 32 == 0).  Filters
                            made by ivx_conv_winograd_weights carry the operand type they were made with
                            (ivx_conv_winograd_weight_elems counts one more plane for the pair form: it holds the filter scale). */
} ivx_conv_desc;

int ivx_conv_out_dims(const ivx_conv_desc *d, int32_t *Do, int32_t *Ho, int32_t *Wo);
int ivx_conv_fwd(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                 const float *shift, const void *res, void *out, ivx_stream_t stream);
/* Same as ivx_conv_fwd with a caller-owned workspace of ivx_conv_workspace_bytes(d) bytes (0 for most layers): lets
 * the library split K across workgroups for layers whose output is too small to fill the chip (ResNet stage 4, FPN
 * laterals on C5, coarse levels of the indoor necks); slices are summed in a fixed order (deterministic).        */
int64_t ivx_conv_workspace_bytes(const ivx_conv_desc *d);
int ivx_conv_fwd_ws(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale, const float *shift,
                    const void *res, void *out, void *workspace, int64_t workspace_bytes, ivx_stream_t stream);

/* fp32 [n] -> bf16 pairs [2n] in the IVX_BF16_PAIR order (n % 16 == 0; channels-last tensors with C % 16 == 0 keep their shape
 * with 2C stored elements per voxel).  A streaming kernel: 4 bytes read + 4 written per value.
 * ivx_conv_pair_supported: 1 when ivx_conv_fwd_ws can run the fp32 convolution `d` (in_dtype / out_dtype IVX_F32) in the pair form,
 * i.e. with in_dtype = IVX_BF16_PAIR on operands converted as above (channel multiples, 31-bit operand offsets, out_mode 0). */
int ivx_bf16_pair_split(const float *in, int64_t n, void *out, ivx_stream_t stream);
int ivx_f16_pair_split(const float *in, int64_t n, float scale, void *out, ivx_stream_t stream);   /* IVX_F16_PAIR of scale * in, saturating */
int ivx_conv_pair_supported(const ivx_conv_desc *d);
/* Host-only (both hosts of the library call it): fp32 filters w [Cout][taps][Cin] (tap-major, Cin % 16 == 0) -> the IVX_BF16_PAIR operand
 * `packed` (2 * Cout * taps * Cin bf16 values): hi = bf16(w), lo = bf16(w - hi), 16-channel groups [hi x16 | lo x16];
 * wgt_layout 0: [Cout][taps][2 Cin], 1 (Cin % 32 == 0): chunk-major [Cout][2 Cin / 64][taps][64]. */
int ivx_bf16_pair_pack_filters(const float *w, int32_t Cout, int32_t taps, int32_t Cin, int32_t wgt_layout, void *packed);

/* ---------------------------------------------------------------------------------------
 * Chained fp16-pair activations (0.4.0): the 2-D trunk on the 16-bit matrix cores without split passes.
 * Replaces the same call sites as ivx_conv_fwd (ResNet-50 / FPN: mmdet3d/models/detectors/imvoxelnet.py:48,50) -- same arithmetic
 * contract, fp32 values, fp32 accumulation -- with the ACTIVATIONS between the layers stored as IVX_F16_PAIR tensors [B,D,H,W,2C]
 * (hi = fp16(s x), lo = fp16(s x - hi), 16-channel groups [hi x16 | lo x16], 4 bytes per value like fp32; 22 significant bits) so
 * that every convolution issues hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (16x the fp32 MFMA rate, three products per
 * multiply-add) and the epilogue of the PRODUCING layer writes the operand the consuming layer reads: no conversion pass.
 * The power-of-two scale s of a tensor lives in device memory and is chosen on the device, without a pass over the tensor, from a
 * bound of the output:  |out| <= max|in| * wbound + sbound + max|res|,  wbound = max_co |scale[co]| * sum_k |w[co][k]|,
 * sbound = max_co |shift[co]|, with the MEASURED maxima of the operands: every epilogue accumulates max |out| (true values) into
 * IVX_AMAX_SLOTS words of the tensor (atomic max on the bits; the caller zeroes them before the producer runs).  The bound
 * puts the largest value below 2^15 (fp16 holds 65504); a bound that is loose by a factor L costs accuracy only beyond L = 2^17
 * (error relative to the tensor's maximum: max(2^-22, 2^-39 L) -- s * bound may sit at 2^14, the bottom of its binade, and a subnormal
 * lo half rounds to 2^-25 in scaled units; tests/ref_pair.py derives it and tests/test_*_pair_range.py check both ends of the rule).
 *   in      IVX_F16_PAIR (d->in_dtype), written with *in_scale (NULL: 1); wgt: IVX_F16_PAIR filters (ivx_conv_desc), their
 *           power-of-two scale folded into scale[] by the caller (scale[co] = bn_scale[co] / s_w: exact)
 *   out     d->out_dtype IVX_F32 or IVX_F16_PAIR (then *out_scale receives its scale; needs amax_in, and amax_res with a residual)
 *   res     res_dtype IVX_F32 or IVX_F16_PAIR (*res_scale), independent of the output's type
 *   amax_out  slots that receive max |out| (or NULL)
 * Restrictions: out_mode 0, Cout % 4 == 0 (pair output / residual: Cout % 16 == 0), tensors below 2 GiB. */
#define IVX_AMAX_SLOTS 64
typedef struct ivx_pair_io {
  const float *in_scale;       /* device [1] or NULL */
  const float *res_scale;      /* device [1]; res_dtype IVX_F16_PAIR */
  int32_t res_dtype;           /* IVX_F32 | IVX_F16_PAIR */
  float *out_scale;            /* device [1]; out_dtype IVX_F16_PAIR */
  const uint32_t *amax_in;     /* device [IVX_AMAX_SLOTS]: bits of max |in| */
  const uint32_t *amax_res;    /* device [IVX_AMAX_SLOTS]: bits of max |res| */
  uint32_t *amax_out;          /* device [IVX_AMAX_SLOTS] or NULL */
  float wbound, sbound;
} ivx_pair_io;
int64_t ivx_conv_pio_workspace_bytes(const ivx_conv_desc *d, const ivx_pair_io *io);
int ivx_conv_fwd_pio(const ivx_conv_desc *d, const ivx_pair_io *io, const void *in, const void *wgt, const float *scale, const float *shift,
                     const void *res, void *out, void *workspace, int64_t workspace_bytes, ivx_stream_t stream);
/* validation kernel of the same contract (tests only): plain fp32 products of the values the pairs stand for */
int ivx_conv_fwd_pio_naive(const ivx_conv_desc *d, const ivx_pair_io *io, const void *in, const void *wgt, const float *scale, const float *shift,
                           const void *res, void *out, ivx_stream_t stream);
/* Host-only (both hosts of the library call it, so they hand the kernels identical bits): fp32 filters w [Cout][taps][Cin] (tap-major,
 * Cin % 32 == 0) -> IVX_F16_PAIR filters `packed` (2 * Cout * taps * Cin halves, chunk-major K: [Cout][Cin/32][taps][hi16|lo16|hi16|lo16])
 * of s_w * w with s_w the power of two that puts max |w| into [2^14, 2^15); scale_out[co] = scale[co] / s_w (scale NULL: 1 / s_w);
 * *wbound = max_co |scale[co]| * sum_k |w[co][k]|, *sbound = max_co |shift[co]| (shift NULL: 0) -- the terms of ivx_pair_io's bound. */
int ivx_pair_pack_filters(const float *w, int32_t Cout, int32_t taps, int32_t Cin, const float *scale, const float *shift, void *packed,
                          float *scale_out, float *wbound, float *sbound);
/* The head of such a chain.  ivx_nchw_to_nhwc that also accumulates max |in| into amax (the image);  nn.MaxPool2d on an fp32 map
 * (the stem's output) that writes an IVX_F16_PAIR tensor with the scale of the bound amax_in * wbound + sbound (the stem as a function
 * of the image: a maximum over a window cannot exceed it), leaves that scale in *out_scale and max |out| in amax_out.  C % 16 == 0.
 * ivx_nchw_to_nhwc_amax takes the maximum over the elements that are not NaN, and an Inf counts: the bound built from it has to hold
 * every finite value of the chain, an Inf selects the fixed scale and the saturating split, and a NaN stays a NaN under any scale, so it
 * needs none (ivx_amax_f32 below differs on purpose: there a NaN counts as Inf). */
int ivx_nchw_to_nhwc_amax(const float *in, int32_t B, int32_t C, int64_t S, int32_t Cpad, float *out, uint32_t *amax, ivx_stream_t stream);
int ivx_maxpool2d_fwd_pair(const float *in, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, int32_t p, void *out,
                           const uint32_t *amax_in, float wbound, float sbound, float *out_scale, uint32_t *amax_out, ivx_stream_t stream);
/* IVX_F16_PAIR [n] (scale *scale_dev or 1) -> fp32 [n] (tests / hosts that want to look at an intermediate tensor) */
int ivx_f16_pair_merge(const void *in, int64_t n, const float *scale_dev, float *out, ivx_stream_t stream);

/* The head of the 2-D trunk in ONE launch (csrc/stem.hip), inside the pair chain: conv 7x7 stride 2 pad 3 (3 -> 64) + BatchNorm + ReLU +
 * MaxPool2d(3, 2, 1) from the fp32 NCHW image [B,3,H,W] to the IVX_F16_PAIR map [B,1,Hp,Wp,64] (ivx_stem_pool_out_dims) -- mmdet ResNet's
 * conv1 / bn1 / relu / maxpool (mmdet3d/models/detectors/imvoxelnet.py:22,48; configs/imvoxelnet/imvoxelnet_kitti.py:4-12).  The conv runs on
 * fp16 (hi, lo) pair operands (image values split in registers with the power-of-two scale of amax_img; three MFMA products per multiply-add),
 * the pool is exact, the output scale is the one of ivx_maxpool2d_fwd_pair (bound amax_img * wbound + sbound).
 *   ivx_amax_f32                 max |x| of an fp32 buffer into IVX_AMAX_SLOTS zeroed words (the image's maximum; a NaN counts as Inf)
 *   ivx_stem_pool_pack_filters   host-only: [64,3,7,7] fp32 filters + BN scale -> the kernel's fragment-ordered pair filters
 *                                (ivx_stem_pool_filter_bytes() bytes) and scale / s_w
 *   ivx_stem_pool_fwd_pair       wfrag / scale_p / shift: device copies of those and of the BN shift; out_scale / amax_out as ivx_pair_io */
int ivx_amax_f32(const float *x, int64_t n, uint32_t *amax, ivx_stream_t stream);
int64_t ivx_stem_pool_filter_bytes(void);
int ivx_stem_pool_pack_filters(const float *w, const float *scale, void *packed, float *scale_out);
int ivx_stem_pool_out_dims(int32_t H, int32_t W, int32_t *Hp, int32_t *Wp);
int ivx_stem_pool_fwd_pair(const float *img, int32_t B, int32_t H, int32_t W, const void *wfrag, const float *scale_p, const float *shift,
                           float wbound, float sbound, const uint32_t *amax_img, void *out, float *out_scale, uint32_t *amax_out,
                           ivx_stream_t stream);

/* One ResNet bottleneck with an identity shortcut in ONE launch (csrc/bottleneck.hip), inside the pair chain:
 *   out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(in)))))))) + in),  conv1 1x1 4P -> P, conv2 3x3 pad 1 P -> P, conv3 1x1 P -> 4P, stride 1
 * -- the identity blocks of mmdet's ResNet(depth=50, style='pytorch') the reference builds at mmdet3d/models/detectors/imvoxelnet.py:22 from
 * configs/imvoxelnet/imvoxelnet_kitti.py:4-12 and runs at :48 (`self.backbone(img)`); stages 1 and 2 (P = 64, 128).  The P-channel
 * intermediates stay in LDS as pair tiles.  in / out: IVX_F16_PAIR [B,1,H,W,4P]; w1 / w2 / w3, scale* / shift*: the pair filters, scale / s_w
 * and shift of ivx_pair_pack_filters for the three layers (w1 [P][4P/32][1][64], w2 [P][P/32][9][64], w3 [4P][P/32][1][64] halves).
 * Scales: powers of two from the BOUND chain b1 = max|in| * wbound[0] + sbound[0], b2 = b1 * wbound[1] + sbound[1],
 * b3 = b2 * wbound[2] + sbound[2] + max|in| (max|in| read from amax_in); *out_scale receives the output's, amax_out max |out|.
 * Differs from three ivx_conv_fwd_pio calls only by the scales of the two intermediates (a-priori bound instead of the measured maximum):
 * fp32-level rounding.  ivx_bottleneck_supported: P in {64, 128} and the tensor below 2 GiB. */
typedef struct ivx_bottleneck_desc {
  int32_t B, H, W, P;
} ivx_bottleneck_desc;
typedef struct ivx_bottleneck_io {
  const float *in_scale;       /* device [1] */
  const uint32_t *amax_in;     /* device [IVX_AMAX_SLOTS] */
  float *out_scale;            /* device [1] */
  uint32_t *amax_out;          /* device [IVX_AMAX_SLOTS] or NULL */
  float wbound[3], sbound[3];
} ivx_bottleneck_io;
int ivx_bottleneck_supported(const ivx_bottleneck_desc *d);
int ivx_bottleneck_fwd_pio(const ivx_bottleneck_desc *d, const ivx_bottleneck_io *io, const void *in, const void *w1, const float *scale1,
                           const float *shift1, const void *w2, const float *scale2, const float *shift2, const void *w3, const float *scale3,
                           const float *shift3, void *out, ivx_stream_t stream);
/* The FIRST block of ResNet stage 1 in one launch (layer1.0 of mmdet's ResNet-50: stride 1, shortcut = 1x1 conv + BN of the block's input; same
 * reference lines as above):  out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(in)))))))) + bnd(convd(in))),  in: IVX_F16_PAIR [B,1,H,W,Cin],
 * out: [B,1,H,W,4P]; built for Cin = P = 64 (ivx_bottleneck_proj_supported).  conv3 and the shortcut conv run as ONE GEMM over K = Cin + P:
 *   ivx_bottleneck_proj_pack   host-only (both hosts call it): w3 [4P][P], wd [4P][Cin] fp32 + the two BatchNorms' scale / shift -> the joint pair
 *                              filter bank `packed` [4P][(Cin + P) / 32][1][64] halves of s_w * [scaled * wd | scale3 * w3] (the BN scales folded
 *                              into the filters), scale_out[n] = 1 / s_w, shift_out = shift3 + shiftd; *wbound3 = max_n sum_k |scale3 w3|,
 *                              *wboundd = max_n sum_k |scaled wd|, *sbound = max_n |shift_out|
 *   ivx_bottleneck_proj_fwd_pio  w1 / w2 and their vectors as ivx_bottleneck_fwd_pio; w3d / scale3d / shift3d: the packed bank and its vectors;
 *                              io->wbound[2] = wbound3, io->sbound[2] = sbound, wbound_shortcut = wboundd: b3 = b2 * wbound3 + sbound + max|in| * wboundd.
 * Differs from the four-launch chain by fp32-level rounding (scales from bounds; BN scales folded into the filters; one accumulation). */
int ivx_bottleneck_proj_supported(const ivx_bottleneck_desc *d, int32_t Cin);
int ivx_bottleneck_proj_pack(const float *w3, const float *scale3, const float *shift3, const float *wd, const float *scaled, const float *shiftd,
                             int32_t P, int32_t Cin, void *packed, float *scale_out, float *shift_out, float *wbound3, float *sbound, float *wboundd);
int ivx_bottleneck_proj_fwd_pio(const ivx_bottleneck_desc *d, int32_t Cin, const ivx_bottleneck_io *io, float wbound_shortcut, const void *in,
                                const void *w1, const float *scale1, const float *shift1, const void *w2, const float *scale2, const float *shift2,
                                const void *w3d, const float *scale3d, const float *shift3d, void *out, ivx_stream_t stream);

/* Validation kernel: same contract, one thread per output element, plain FMA loop. Used by the
 * GPU tests to cross-check the MFMA kernel at full size; never called by the product path.   */
int ivx_conv_fwd_naive(const ivx_conv_desc *d, const void *in, const void *wgt, const float *scale,
                       const float *shift, const void *res, void *out, ivx_stream_t stream);

/* Fraction of the 3 x slices tap-slices the Winograd-domain GEMM of this layer issues under the library's default kernel rule (FLOP
 * accounting of bench.py / the stage trace): 7/9 for stride-1, pad-1 layers on 3-slice columns with fp16 pair operands and more than 64
 * output channels (their z-blocked tile skips the taps outside the column), else 1.  d: the layer descriptor (W = slices). */
float ivx_conv_winograd_issued_fraction(const ivx_conv_desc *d);
/* Minimal-filtering (Winograd F(m x m, 3x3), tile m = 2, 4 or 6) form of the same convolution for 3x3xKW kernels with
 * stride 1 on the first two spatial axes (D, H) -- the 3x3x3 layers of the KITTI / nuScenes necks
 * (mmdet3d/models/necks/imvoxelnet.py:99-113,181-230), which are bound by the fp32 MFMA rate: (m+2)^2 instead of 9*m*m
 * multiplications per m x m output tile and W-tap (16 vs 36, 36 vs 144, 64 vs 324).  Same contract, epilogue and fp32
 * arithmetic as ivx_conv_fwd; the result differs by fp32 rounding only (max deviation from the direct kernel on a
 * 256-channel layer, as a fraction of the output range: tile 2 4e-6, tile 4 2e-5, tile 6 4e-5).  The W axis keeps its kernel
 * extent, stride and padding as a direct convolution.
 * Restrictions: KD = KH = 3, sd = sh = 1, fp32, out_mode 0, res_mode 0/1, Cin % 4 == 0, Cout % 4 == 0, and one transformed
 * plane [B, ceil(Do/m), ceil(Ho/m), W, Cin] below 2 GiB (ivx_conv_winograd_supported returns 1 when all hold).
 *   u          transformed filters, ivx_conv_winograd_weight_elems(d, tile) floats: [(m+2)^2][Cout][KW*Cin] with the K order
 *              of d->wgt_layout; made once per layer by ivx_conv_winograd_weights from wgt in layout 0 [Cout,3,3,KW,Cin].
 *   workspace  ivx_conv_winograd_workspace_bytes(d, tile) bytes (the transformed input and the (m+2)^2 partial outputs).
 * ivx_conv_winograd_fwd = _input (transform the input into the workspace) + _gemm ((m+2)^2 independent 1x1xKW
 * convolutions, one grouped launch of the implicit-GEMM kernel) + _output (inverse transform + epilogue); the stages are
 * exported separately so that a caller can time them. */
int ivx_conv_winograd_supported(const ivx_conv_desc *d, int32_t tile);
int64_t ivx_conv_winograd_weight_elems(const ivx_conv_desc *d, int32_t tile);
int ivx_conv_winograd_weights(const ivx_conv_desc *d, int32_t tile, const float *wgt, float *u, ivx_stream_t stream);
int64_t ivx_conv_winograd_workspace_bytes(const ivx_conv_desc *d, int32_t tile);
int ivx_conv_winograd_input(const ivx_conv_desc *d, int32_t tile, const void *in, void *workspace, int64_t workspace_bytes,
                            ivx_stream_t stream);
int ivx_conv_winograd_gemm(const ivx_conv_desc *d, int32_t tile, const float *u, void *workspace, int64_t workspace_bytes,
                           ivx_stream_t stream);
int ivx_conv_winograd_output(const ivx_conv_desc *d, int32_t tile, const float *scale, const float *shift, const void *res,
                             void *out, void *workspace, int64_t workspace_bytes, ivx_stream_t stream);
int ivx_conv_winograd_fwd(const ivx_conv_desc *d, int32_t tile, const void *in, const float *u, const float *scale,
                          const float *shift, const void *res, void *out, void *workspace, int64_t workspace_bytes,
                          ivx_stream_t stream);
/* Host-only: the form a convolution layer runs in -- the ONE routing rule of the library, asked by every host of the kernels (the model
 * handle and imvoxelnet_amd/conv.py FusedConv), so both launch the same kernels on the same shapes.  All thresholds and their measurements
 * are in csrc/api_common.cpp.
 *   d         the layer as ivx_conv_fwd sees it (Cin = padded channels, wgt_layout = the layout of its direct filters, res_mode, dtypes);
 *             B == 0: no shape yet -- only the candidate flags are answered (what the host keeps / packs when it loads the filters) and
 *             `run` carries the kernel as the Winograd form would see it and the wino_operands a forced tile o->winograd_tile would take
 *   cin_real  input channels of the layer before padding (the Winograd and split-operand forms need Cin unpadded)
 * Gates that are a host's own stay with the host: a validation run on the naive kernel, quantised epilogues, transposed / linear / DCN-column
 * layers, the storage mode of a handle. */
typedef struct ivx_conv_route_opts {      /* model-level switches that bear on the route */
  int32_t winograd;                       /* Winograd form on (ivx_model_cfg.winograd / FusedConv.winograd, IVX_WINOGRAD) */
  int32_t winograd_tile;                  /* 0 = by plane size | 2 | 4 | 6 (IVX_WINOGRAD_TILE) */
  int32_t wino_operands;                  /* 0 | IVX_F16_PAIR (IVX_WINO_OPERANDS) */
  int32_t split;                          /* split-operand rule on (IVX_CONV_PAIR != 0) */
  int64_t winograd_min_pos;               /* < 0: the rule's own value; fewest input positions of the Winograd form otherwise (lab) */
  int32_t winograd_2d_min_ch;             /* <= 0: the rule's own value; channel floor of the 2-D Winograd candidates otherwise (lab) */
} ivx_conv_route_opts;
typedef struct ivx_conv_route {
  int32_t form;                           /* 0 direct, 1 Winograd, 2 split-operand direct (only where the Winograd form does not apply) */
  int32_t tile;                           /* m of F(m x m, 3x3) when form == 1, else 0 */
  int32_t wino_candidate, split_candidate;/* shape-independent: keep the tap-major fp32 filters / pack the IVX_BF16_PAIR filters (under `o`) */
  int32_t split_fits;                     /* the split-operand rule holds for this shape, whether or not the Winograd form comes first */
  int32_t prefers_winograd;               /* a 2-D layer of the pair chain that should keep fp32 tensors and run its Winograd form here */
  ivx_conv_desc run;                      /* descriptor to launch: form 1 the Winograd view (a 2-D layer [B,1,H,W,C] as [B,H,W,1,C] with a 3x3x1
                                             kernel) with wino_operands set; form 2 in_dtype IVX_BF16_PAIR, wgt_layout 1; form 0 = *d */
} ivx_conv_route_out;
int ivx_conv_route(const ivx_conv_desc *d, int32_t cin_real, const ivx_conv_route_opts *o, ivx_conv_route_out *r);
/* Chained Winograd layers with fp16-pair operands: the scale of V needs max |in|, which ivx_conv_winograd_input takes with a pass over
 * the tensor.  When `in` is the output of another Winograd layer, that layer's output transform can leave one maximum per workgroup
 * (`partials`, ivx_conv_winograd_output_blocks(d, tile) floats, caller-owned device memory) and the consumer's input stage reduces those
 * few KB instead: ivx_conv_winograd_output_amax / ivx_conv_winograd_input_amax (partials NULL = the plain entry points).  The maxima are
 * those of the stored tensor (after the epilogue), so both routes give the same scale, bit for bit. */
int32_t ivx_conv_winograd_output_blocks(const ivx_conv_desc *d, int32_t tile);
int ivx_conv_winograd_output_amax(const ivx_conv_desc *d, int32_t tile, const float *scale, const float *shift, const void *res, void *out,
                                  void *workspace, int64_t workspace_bytes, float *partials, ivx_stream_t stream);
int ivx_conv_winograd_input_amax(const ivx_conv_desc *d, int32_t tile, const void *in, void *workspace, int64_t workspace_bytes,
                                 const float *partials, int32_t n_partials, ivx_stream_t stream);
/* F(4x4,3x3) on IVX_F16_PAIR operands with the GEMM stage and the output stage fused into ONE launch (round 5): the workgroup that
 * multiplies a block of tile rows walks all 36 frequency points, folds every partial product block into the output domain on chip
 * (out = At M A accumulated in registers) and applies the epilogue -- M is never written to the workspace.  Replaces the pair
 * ivx_conv_winograd_gemm + ivx_conv_winograd_output[_amax] after ivx_conv_winograd_input[_amax] on the SAME workspace; applies to the
 * stride-1, pad-1, 3-tap z kernels of the ResModules (mmdet3d/models/necks/imvoxelnet.py:94-123) with wgt_layout 1 and Cin % 32 == 0
 * while the 36 planes of V stay below 2 GiB (ivx_conv_winograd_fused_supported).  Results equal the three-stage form up to fp32
 * rounding (another summation order of the same products).  partials (or NULL): ivx_conv_winograd_fused_blocks(d, tile) floats, one
 * max |out| per workgroup, for the consumer's ivx_conv_winograd_input_amax. */
int ivx_conv_winograd_fused_supported(const ivx_conv_desc *d, int32_t tile);
int32_t ivx_conv_winograd_fused_blocks(const ivx_conv_desc *d, int32_t tile);
int ivx_conv_winograd_gemm_output_amax(const ivx_conv_desc *d, int32_t tile, const float *u, const float *scale, const float *shift,
                                       const void *res, void *out, void *workspace, int64_t workspace_bytes, float *partials,
                                       ivx_stream_t stream);
/* Background tiles of a neck whose first layer reads the unprojection's output.  `valid` [B, X, Y, Z] (ivx_backproject_mean_fwd) marks the
 * voxels a camera sees; every other voxel of the volume is exactly 0.  For a chain of consecutive F(6x6,3x3) layers with stride 1 and
 * padding 1 in x and y (each reads the previous one's output; a residual is the volume or an earlier layer's output) a tile of layer L
 * (1-based) is QUIET when no tile within Chebyshev distance L - 1 of it has a valid voxel in its 8 x 8 layer-1 input window, and two quiet
 * tiles whose four distances to the edges of the tile grid, capped at L - 1, are equal (their KEY) have bit-identical input windows.
 * ivx_conv_winograd_bg_plan (two small launches, nothing returns to the host) writes per layer, into `block` (ivx_conv_winograd_bg_bytes,
 * layer l at ivx_conv_winograd_bg_layer_offset(d, l)): int32 {slots, slots * out_slices[l], image-dependent tiles, keys}, then list[B TX TY]
 * -- the image-dependent tiles in their order, then one representative (the lowest tile index) per key present, keys ascending by
 * ((left * L + right) * L + top) * L + bottom -- and src[B TX TY], the slot of every tile.  The _bg stage entry points take a layer's
 * block: the input transform and the GEMM run over the slots only (their grids keep the dense size; surplus workgroups return at once),
 * the output transform visits every tile and reads M at its slot, so every tensor is bit-identical to the dense path's.  bg NULL = the
 * plain entry points.  d: the first layer (all layers share B, X, Y and hence the tile grid); at most 9 layers. */
int ivx_conv_winograd_bg_supported(const ivx_conv_desc *d, int32_t tile);
int64_t ivx_conv_winograd_bg_bytes(const ivx_conv_desc *d, int32_t n_layers);
int64_t ivx_conv_winograd_bg_layer_offset(const ivx_conv_desc *d, int32_t layer);
int ivx_conv_winograd_bg_plan(const ivx_conv_desc *d, const uint8_t *valid, int32_t n_layers, const int32_t *out_slices, void *block,
                              int64_t block_bytes, ivx_stream_t stream);
int ivx_conv_winograd_input_bg(const ivx_conv_desc *d, int32_t tile, const void *in, void *workspace, int64_t workspace_bytes,
                               const float *partials, int32_t n_partials, const int32_t *bg, ivx_stream_t stream);
int ivx_conv_winograd_gemm_bg(const ivx_conv_desc *d, int32_t tile, const float *u, void *workspace, int64_t workspace_bytes,
                              const int32_t *bg, ivx_stream_t stream);
int ivx_conv_winograd_output_bg(const ivx_conv_desc *d, int32_t tile, const float *scale, const float *shift, const void *res, void *out,
                                void *workspace, int64_t workspace_bytes, float *partials, const int32_t *bg, ivx_stream_t stream);


/* Modulated deformable convolution (DCNv2; mmcv ModulatedDeformConv2dPack, deform_groups = 1) -- nuScenes reference
 * backbone, configs/imvoxelnet/imvoxelnet_nuscenes.py:13-14.  Builds the modulated, bilinearly sampled columns
 *   col[b,ho,wo,k,c] = sigmoid(m_k) * bilinear(x[b,:,:,c], ho*s - p + i*d + dh_k, wo*s - p + j*d + dw_k)     (k = i*kw + j)
 * from x [B,H,W,C] and the raw output offset_mask [B,Ho,Wo,om_channels] of the companion conv_offset (channels
 * dh_0,dw_0,...,dh_{K-1},dw_{K-1},m_0..m_{K-1}).  The contraction over (k,c) is ivx_conv_fwd with a 1x1 kernel and
 * Cin = kh*kw*C on col viewed as [B,1,Ho,Wo,kh*kw*C].  C % 4 == 0. */
int ivx_dcn_im2col_fwd(const float *x, const float *offset_mask, int32_t B, int32_t H, int32_t W, int32_t C, int32_t kh,
                       int32_t kw, int32_t stride, int32_t pad, int32_t dil, int32_t om_channels, float *col,
                       ivx_stream_t stream);
/* The same inside a chain of fp16-pair activations (0.4.0): x is an IVX_F16_PAIR map [B,H,W,2C] with the scale *x_scale (device), col an
 * IVX_F16_PAIR tensor [B,Ho,Wo,2*kh*kw*C]; the columns keep x's scale (every column is a convex combination of values of x times a mask
 * in (0, 1)): *col_scale = *x_scale, and max |col| goes to the amax slots col_amax (may be NULL).  The decoded columns are the fp32
 * columns of the decoded x rounded to the pair format.  C % 16 == 0.  The contraction is ivx_conv_fwd_pio with Cin = kh*kw*C. */
int ivx_dcn_im2col_fwd_pair(const void *x, const float *x_scale, const float *offset_mask, int32_t B, int32_t H, int32_t W, int32_t C,
                            int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t dil, int32_t om_channels, void *col,
                            float *col_scale, uint32_t *col_amax, ivx_stream_t stream);
/* The same on bf16 storage (0.4.2): x a bf16 map [B,H,W,C], offset_mask fp32 as above (the conv_offset layer writes fp32 on a bf16 handle),
 * col a bf16 tensor [B,Ho,Wo,kh*kw*C] in the (tap, c) order of ivx_dcn_im2col_fwd.  Blend and mask multiply in fp32 as in
 * ivx_dcn_im2col_fwd, one rounding to bf16 (nearest even) per column element.  C % 8 == 0; x and col 16-byte aligned (else
 * IVX_ERR_INVALID_ARG).  The contraction is ivx_conv_fwd on bf16 operands with Cin = kh*kw*C. */
int ivx_dcn_im2col_fwd_bf16(const void *x, const float *offset_mask, int32_t B, int32_t H, int32_t W, int32_t C, int32_t kh,
                            int32_t kw, int32_t stride, int32_t pad, int32_t dil, int32_t om_channels, void *col,
                            ivx_stream_t stream);

/* nn.MaxPool2d(kernel, stride, padding) on NHWC (ResNet stem: 3, 2, 1). */
int ivx_maxpool2d_fwd(const float *in, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                      int32_t s, int32_t p, float *out, ivx_stream_t stream);
/* Same on bf16 storage (optional reduced-precision mode; a max of bf16 values is exact). */
int ivx_maxpool2d_fwd_bf16(const void *in, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                           int32_t s, int32_t p, void *out, ivx_stream_t stream);
/* The same pool on e4m3 bytes (IVX_FP8 storage; C % 16 == 0): exact, the tensor's scale is unchanged. */
int ivx_maxpool2d_fwd_fp8(const void *in, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, int32_t p,
                          void *out, ivx_stream_t stream);

/* F.interpolate(scale_factor=2, mode='trilinear', align_corners=False) on NDHWC [B,D,H,W,C] -> [B,2D,2H,2W,C]
 * (Atlas decoder of ImVoxelNeck, mmdet3d/models/necks/imvoxelnet.py:359).  C % 4 == 0. */
int ivx_upsample_trilinear2x_fwd(const float *in, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, float *out,
                                 ivx_stream_t stream);

/* NCHW [B,C,H,W] -> NHWC [B,H,W,Cpad] (channels >= C zero filled), and NHWC/NDHWC -> NCHW/NCDHW
 * ([B,S,C] -> [B,C,S] with S = product of the spatial dims). */
int ivx_nchw_to_nhwc(const float *in, int32_t B, int32_t C, int64_t S, int32_t Cpad, float *out,
                     ivx_stream_t stream);
/* bf16 mode only: image [B,3,H,W] fp32 NCHW (H, W even) -> 2x2 space-to-depth blocks [B, H/2+1, W/2+1, 16] bf16 with
 * out[b][ph][pw][(a*2+e)*3+c] = img[b][c][2ph-1+a][2pw-1+e] (zero outside, channels 12..15 zero): the 7x7 stride-2 pad-3 stem
 * (mmdet ResNet.conv1) becomes a 4x4 stride-1 pad-1 convolution over it (weights re-indexed kh = 2*th + a, kw = 2*tw + e). */
int ivx_image_s2d_bf16(const float *img, int32_t B, int32_t H, int32_t W, void *out, ivx_stream_t stream);
int ivx_nhwc_to_nchw(const float *in, int32_t B, int64_t S, int32_t C, float *out, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Device-side image pipeline (0.4.3) -- the Resize(keep_ratio) -> Normalize -> Pad(32) steps of the reference test pipelines
 * (configs/imvoxelnet/imvoxelnet_kitti.py:94-105) from uint8 HWC BGR frames to the fp32 NCHW input of the model, in one launch
 * (csrc/image_prep.hip).  The result is bit-identical to data.prepare_image of the Python package, zero pad region included:
 *   resize     the integer restatement of cv2.resize(INTER_LINEAR) on uint8 held by data.imresize_cv2_linear / data._linear_tables:
 *              fx = float32((d + 0.5) * (double(src) / double(dst)) - 0.5) with the product and the difference in double, floor, both
 *              borders clamped, 11-bit weights rounded half to even; int32 horizontal pass S[sx] * a0 + S[sx1] * a1; vertical pass
 *              (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2, clamped to 0..255.  dst == src is a copy; src == 2 * dst on
 *              BOTH axes takes the INTER_AREA shortcut (a + b + c + d + 2) >> 2.  Up-scaling goes through the same formulas.
 *              Parity with cv2 ITSELF is UNPINNED: the restatement is checked against hand-derived vectors, not against OpenCV.
 *   normalise  optional swap of channels 0 and 2 (BGR -> RGB), then (float(v) - mean[c]) / std[c] in fp32 with an IEEE divide;
 *              mean / std in OUTPUT-channel order (IMG_NORM_CFG).
 *   pad        out is [n, 3, pad_h, pad_w]; y >= dst_h or x >= dst_w is written as +0.0f by the same launch (no memset needed).  pad_h /
 *              pad_w may exceed the image's own padded size (the common plane of a batch of mixed sizes).
 * Limits: every extent (src, dst, pad) <= IVX_IMAGE_PREP_MAX_DIM, n <= 2^20.  Any pad_w and any 4-byte aligned `out` are accepted: the
 * 16-byte store path needs pad_w % 4 == 0 and a 16-byte aligned out, everything else takes scalar stores (same bits). */
#define IVX_IMAGE_PREP_MAX_DIM 32768
typedef struct ivx_image_prep_desc {
  int32_t src_h, src_w;      /* source frame, HWC uint8, 3 channels */
  int32_t src_row_bytes;     /* >= 3 * src_w (decoder pitch) */
  int32_t dst_h, dst_w;      /* resized size = img_shape */
  int32_t pad_h, pad_w;      /* output plane = pad_shape, >= dst */
  int32_t to_rgb;            /* swap channels 0 and 2 before normalising */
  float mean[3], std[3];     /* output-channel order */
} ivx_image_prep_desc;

/* mmcv.rescale_size for a (long, short) scale: the Resize(keep_ratio=True) size. Host only.  Equals data.rescale_size: double
 * arithmetic, f = min(max_long / max(h, w), max_short / min(h, w)), size = int(h * f + 0.5); the two scale values in either order. */
int ivx_rescale_size(int32_t src_h, int32_t src_w, int32_t scale_a, int32_t scale_b,
                     int32_t *dst_h, int32_t *dst_w);

/* n frames of one geometry, src + i * src_image_bytes; out [n,3,pad_h,pad_w] fp32; caller-owned buffers, no sync.
 * IVX_ERR_INVALID_ARG (before any launch): null pointers, non-positive sizes, pad < dst, src_row_bytes < 3 * src_w, a std entry that is
 * zero or not finite, n <= 0, src_image_bytes < src_h * src_row_bytes with n > 1, an extent or n above the limits. */
int ivx_image_prep_u8(const ivx_image_prep_desc *d, const void *src, int64_t src_image_bytes,
                      int32_t n, float *out, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Lens-aware device image pipeline (0.5.2) -- Undistort -> Resize -> Normalize -> Pad in the one launch that reads the raw frame
 * (csrc/image_prep.hip), and the feature-resolution maps of the same geometry.  ivx_image_prep_u8 assumes an ideal pinhole camera; a real
 * one (handheld RGB-D scanners, wide-angle and fisheye heads) has radial distortion, and undistorting on the host costs a second
 * interpolation, a host pass per frame and the uint8 path.  Here ONE geometric map G takes a pixel of the network input back to the raw
 * frame; the image is sampled through it once, and the border mask and the depth frame at feature resolution follow from the same rule.
 *
 * The lens (all double, in pixels of the SOURCE frame): */
#define IVX_LENS_BROWN 0   /* OpenCV's 5-coefficient model: coef = (k1, k2, p1, p2, k3) */
#define IVX_LENS_FISHEYE 1 /* OpenCV's equidistant fisheye model: coef = (k1, k2, k3, k4), coef[4] unused (must be finite) */
typedef struct ivx_lens {
  int32_t model;                           /* IVX_LENS_BROWN | IVX_LENS_FISHEYE (the doubles that follow are 8-byte aligned) */
  double fx, fy, cx, cy;                   /* the real camera */
  double coef[5];                          /* the distortion coefficients */
  double new_fx, new_fy, new_cx, new_cy;   /* the ideal pinhole camera the network input shows, at the source size: what the
                                              caller's lidar2img intrinsic must describe */
  double r2_max;                           /* normalised radius squared beyond which the polynomial is not trusted; +inf: no limit */
} ivx_lens;
/* The map G.  For the input pixel (x, y), 0 <= x < dst_w, 0 <= y < dst_h, every step in fp64, each operation rounded on its own (no
 * fused multiply-add), in exactly this order (k1.. / p1, p2 name the entries of coef by the model's list above):
 *   px = (x + 0.5) * (double(src_w) / double(dst_w)) - 0.5 ;  py = (y + 0.5) * (double(src_h) / double(dst_h)) - 0.5
 *   xn = (px - new_cx) / new_fx ;  yn = (py - new_cy) / new_fy ;  r2 = xn * xn + yn * yn
 *   BROWN:    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *             xd  = (xn * rad + ((2 * p1) * xn) * yn) + p2 * (r2 + (2 * xn) * xn)
 *             yd  = (yn * rad + p1 * (r2 + (2 * yn) * yn)) + ((2 * p2) * xn) * yn
 *   FISHEYE:  r = sqrt(r2) ;  th = atan(r) ;  t2 = th * th
 *             thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
 *             s = r > 0 ? thd / r : 1 ;  xd = xn * s ;  yd = yn * s
 *   u = fx * xd + cx ;  v = fy * yd + cy
 *   inside = r2 <= r2_max  and  -0.5 <= u <= src_w - 0.5  and  -0.5 <= v <= src_h - 0.5        (false when anything is NaN)
 * Pixels of the pad region (x >= dst_w or y >= dst_h) and pixels with inside == false are BORDER.  lens == NULL (the map entry only)
 * is the ideal camera: u = px, v = py, inside by the same range test.
 *
 * ivx_image_prep_lens_u8: ivx_image_prep_u8 through G, reusing ivx_image_prep_desc unchanged.  An inside pixel is the bilinear blend
 * of the four source bytes around (u, v), taps clamped to the frame (replicate):
 *   iu = floor(u), iv = floor(v) ;  fu = float32(u - iu), fv = float32(v - iv)       (the fractions rounded ONCE to fp32)
 *   x0 = max(iu, 0), x1 = min(iu + 1, src_w - 1) ;  y0 = max(iv, 0), y1 = min(iv + 1, src_h - 1)
 *   a = S[y0][x0], b = S[y0][x1], c = S[y1][x0], d = S[y1][x1] as fp32 ;  then, every operation in fp32 and rounded on its own:
 *   top = a + fu * (b - a) ;  bot = c + fu * (d - c) ;  val = top + fv * (bot - top)
 *   out = (val - mean[c]) / std[c]                 (one subtract, one IEEE divide, as the plain entry; NO rounding to uint8)
 * Border and pad pixels are written as +0.0f; to_rgb as in the plain entry; one lens per call; every element of out is written.
 * The same work split as the plain kernel: 4 consecutive x of one row per thread, three 16-byte stores (scalar stores when
 * pad_w % 4 != 0 or out is not 16-byte aligned; same bits).  Error against the exact blend at the exact (u, v):
 * at most 8 * 2^-24 * 255 / |std[c]| plus the divide's own rounding (tests/test_gpu_lens_prep.py counts the operations).
 * IVX_ERR_INVALID_ARG (before any launch): everything ivx_image_prep_u8 refuses, a null lens, an unknown model, fx / fy / new_fx /
 * new_fy zero or not finite, cx / cy / new_cx / new_cy or a coefficient not finite, r2_max that is neither > 0 nor +inf (NaN refused). */
int ivx_image_prep_lens_u8(const ivx_image_prep_desc *d, const ivx_lens *lens, const void *src, int64_t src_image_bytes,
                           int32_t n, float *out, ivx_stream_t stream);

/* The feature-resolution maps of the same geometry.  out is [n, ceil(pad_h / stride), ceil(pad_w / stride)] fp32; feature pixel
 * (i, j) is input pixel (y, x) = (stride * i, stride * j) -- the strided pick rule of the scenes' pixel maps.  Of `d` only src_h,
 * src_w, dst_h, dst_w, pad_h, pad_w are read (the sizes of the image pipeline this map belongs to).
 *   src == NULL   the COVER map: 1.0f where that input pixel is inside, 0.0f where it is border; every one of the n planes is written
 *                 (src_dtype, src_row_bytes, src_map_bytes and scale are ignored).
 *   src != NULL   n maps at the SOURCE size, src + i * src_map_bytes, rows src_row_bytes apart, IVX_MAP_F32 or IVX_MAP_U16 elements
 *                 (a depth frame in millimetres): out = scale * float32(value at the nearest source pixel (floor(u + 0.5),
 *                 floor(v + 0.5)), clamped to the frame) -- one fp32 multiply -- and 0.0f at border pixels: the lifts' "no measurement".
 * lens == NULL is the ideal camera, which takes depth frames through the plain pipeline as well.
 * IVX_ERR_INVALID_ARG (before any launch): null d / out, the size rules of ivx_image_prep_u8 (positive sizes, pad >= dst, extents and
 * n within the limits), stride < 1, an invalid lens (as above), and with src: an unknown src_dtype, src_row_bytes below src_w elements
 * or not a multiple of the element size, a misaligned src or src_map_bytes, src_map_bytes < src_h * src_row_bytes with n > 1, a scale
 * that is not finite. */
#define IVX_MAP_F32 0
#define IVX_MAP_U16 1
int ivx_map_prep_lens(const ivx_image_prep_desc *d, const ivx_lens *lens_or_null, const void *src_or_null, int32_t src_dtype,
                      int64_t src_row_bytes, int64_t src_map_bytes, float scale, int32_t stride, int32_t n, float *out,
                      ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Decoder pixel formats in the device image pipeline (0.5.3) -- the two image entries above take packed 3-byte BGR, which no decoder or
 * camera stack on the device side produces: a hardware video decoder hands out pitched NV12 surfaces, UVC cameras YUYV, compositors BGRA
 * or RGBA, IR sensors 8-bit gray.  Here the colour conversion happens inside the fetch of the same one launch (csrc/pixel_fetch.h): no
 * extra pass, no 3-byte intermediate frame, and ONE stated rounding rule.
 *
 * The definition.  A frame in any layout IS a BGR uint8 frame through the integer rule below, and the result of the pipeline is the
 * existing entry applied to that BGR frame: nothing about the resize, the lens map G, the blend, the normalisation or the pad changes. */
#define IVX_PIX_BGR8  0   /* 3 bytes / pixel: the input of ivx_image_prep_u8 */
#define IVX_PIX_RGB8  1   /* 3 bytes / pixel */
#define IVX_PIX_BGRA8 2   /* 4 bytes / pixel, byte 3 ignored */
#define IVX_PIX_RGBA8 3   /* 4 bytes / pixel, byte 3 ignored */
#define IVX_PIX_GRAY8 4   /* 1 byte / pixel, B = G = R = the byte */
#define IVX_PIX_NV12  5   /* plane 0: Y [src_h][src_w]; plane 1: interleaved (U, V) [ceil(src_h/2)][ceil(src_w/2)][2] */
#define IVX_PIX_YUYV  6   /* packed 4:2:2, macropixel (Y0, U, Y1, V) for pixels (2k, 2k+1); ceil(src_w/2) macropixels per row */
typedef struct ivx_frame_format {
  int32_t layout;            /* IVX_PIX_* */
  int32_t plane1_row_bytes;  /* NV12 only: pitch of the UV plane, >= 2 * ceil(src_w / 2) */
  int64_t plane1_offset;     /* NV12 only: bytes from the frame's first byte to its UV plane, >= src_h * src_row_bytes */
  int32_t y_off, cy, cub, cug, cvg, cvr;   /* YUV layouts only: the integer matrix, 20 fractional bits */
} ivx_frame_format;
/* Geometry.  ivx_image_prep_desc is reused unchanged; its src_row_bytes is the pitch of plane 0, with a lower bound per layout (in the
 * order of the list above): 3 * src_w, 3 * src_w, 4 * src_w, 4 * src_w, src_w, src_w, 4 * ceil(src_w / 2).  Odd src_w and src_h are
 * legal for every layout.  Chroma is taken at the NEAREST sample -- replicated, as cv2.cvtColor does, never interpolated: for NV12 pixel
 * (x, y) uses the (U, V) pair [y >> 1][x >> 1] of plane 1, for YUYV the pair of macropixel x >> 1 of its own row.  Fields that a layout
 * does not use are not read.
 *
 * YUV -> BGR, per pixel, in integers (every >> is a floor; clamp(v, 0, 255) = min(max(v, 0), 255)):
 *   yy = max(0, Y - y_off) * cy ;  u = U - 128 ;  v = V - 128
 *   R = clamp((yy + (1 << 19) + cvr * v) >> 20, 0, 255)
 *   G = clamp((yy + (1 << 19) + cvg * v + cug * u) >> 20, 0, 255)
 *   B = clamp((yy + (1 << 19) + cub * u) >> 20, 0, 255)
 * Every coefficient magnitude must be <= 3 << 20 and 0 <= y_off <= 255; then no intermediate leaves int32
 * (255 * 3 * 2^20 + 2 * 128 * 3 * 2^20 + 2^19 < 2^31).  The entry refuses anything larger.
 *
 * The named matrices (host only): fills y_off, cy, cub, cug, cvg, cvr of *f and touches nothing else.  IVX_YUV_BT601 with
 * full_range == 0 is OpenCV's table VERBATIM -- y_off 16, cy 1220542, cub 2116026, cug -409993, cvg -852492, cvr 1673527, the constants
 * of cvtColor(COLOR_YUV2BGR_NV12 / _YUY2), which are rounded decimals and not the exact matrix; that row is therefore listed by value.
 * The other three rows (BT.601 full range, BT.709 limited, BT.709 full) are the exact real matrix times 2^20 rounded half to even, with
 * (Kr, Kb) = (0.299, 0.114) for BT.601 or (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb; limited range: y_off = 16, cy = 255/219,
 * chroma scale s = 255/224; full range: y_off = 0, cy = 1, s = 1; cvr = 2s(1-Kr), cub = 2s(1-Kb), cug = -2s*Kb(1-Kb)/Kg,
 * cvg = -2s*Kr(1-Kr)/Kg.  A caller with another standard writes the six integers themselves.  Parity with cv2 ITSELF is UNPINNED (as
 * for the resize): the rule is held to an independent integer restatement, not to OpenCV.
 * IVX_ERR_INVALID_ARG: a null f, an unknown standard. */
#define IVX_YUV_BT601 0
#define IVX_YUV_BT709 1
int ivx_yuv_matrix(int32_t standard, int32_t full_range, ivx_frame_format *f);

/* n frames of one geometry and one format, src + i * src_image_bytes (planes included: plane 1 of frame i is at
 * src + i * src_image_bytes + plane1_offset); out [n,3,pad_h,pad_w] fp32; caller-owned buffers, no sync.
 *   lens_or_null == NULL   the result equals ivx_image_prep_u8 on the converted BGR frames BIT FOR BIT: the three resize modes (copy,
 *                          exact-half area, linear) and both store paths.
 *   lens_or_null != NULL   the result equals ivx_image_prep_lens_u8 on the converted frames BIT FOR BIT: the four taps are converted
 *                          bytes, the fp32 blend is the stated one.
 * d->to_rgb keeps its meaning: swap channels 0 and 2 of the BGR frame defined above (IVX_PIX_RGB8 with to_rgb = 1 therefore reads its
 * bytes straight through).  Every tap is converted once for its three channels; the (U, V) pair of NV12 is read with one 2-byte load and
 * the macropixel of YUYV / the pixel of BGRA, RGBA with one 4-byte load when base, offset, pitches and frame stride make every such
 * address aligned, with byte loads otherwise (same bits): no alignment is required of the caller.
 * IVX_ERR_INVALID_ARG (before any launch): everything the two existing entries refuse, with the row-bytes bound taken per layout; a null
 * fmt or an unknown layout; NV12 with plane1_row_bytes or plane1_offset below their bounds (or plane1_offset above 2^46); a coefficient
 * or y_off out of range on a YUV layout; with n > 1 a src_image_bytes that does not cover the last plane.  ivx_image_prep_u8,
 * ivx_image_prep_lens_u8 and ivx_map_prep_lens keep their signatures, messages and bits. */
int ivx_image_prep_fmt_u8(const ivx_image_prep_desc *d, const ivx_frame_format *fmt, const ivx_lens *lens_or_null, const void *src,
                          int64_t src_image_bytes, int32_t n, float *out, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused image-to-voxel unprojection -- replaces the per-sample Python loop
 * mmdet3d/models/detectors/imvoxelnet.py:58-76 (get_points :132-141, backproject :145-160,
 * view sum / count / divide / zero-fill :70-74) for a whole batch in one launch.
 *
 * feat        [B*V, FH, FW, C]  FPN level-0 features, NHWC
 * proj        [B, V, 3, 4]      per-view K' @ E[:3] (built on the host exactly as :114-129)
 * new_origin  [B, 3]            origin - n_voxels/2 * voxel_size (fp32, :139)
 * crop_hw     [B, 2] int32      img_shape // stride (h, w): the crop at :67-69
 * voxel_size  host float[3]
 * volume      [B, X, Y, Z, C]   mean over valid views, 0 where no view sees the voxel
 * valid       [B, X, Y, Z] u8   1 where >= 1 view sees the voxel (the reference's `valids`)
 * Projection arithmetic is the reference's bit for bit: fp32 FMA chain in k order (what
 * torch.bmm does), IEEE division, round-half-even, nearest-pixel gather.                    */
int ivx_backproject_mean_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                             const float *proj, const float *new_origin, const int32_t *crop_hw,
                             const float *voxel_size /*host*/, int32_t X, int32_t Y, int32_t Z,
                             float *volume, uint8_t *valid, ivx_stream_t stream);

/* bf16 storage variants (optional reduced-precision mode; sums, divisions and interpolation weights in fp32, one
 * rounding at the store): multi-view lift and the Atlas decoder's trilinear x2 up-sampling.  A single-view bf16 lift
 * is a byte copy: pass the map to ivx_backproject_mean_fwd as C/2 32-bit words.                                 */
int ivx_backproject_mean_fwd_bf16(const void *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                                  const float *proj, const float *new_origin, const int32_t *crop_hw,
                                  const float *voxel_size, int32_t X, int32_t Y, int32_t Z, void *volume,
                                  uint8_t *valid, ivx_stream_t stream);
int ivx_upsample_trilinear2x_fwd_bf16(const void *in, int32_t B, int32_t D, int32_t H, int32_t W, int32_t C, void *out,
                                      ivx_stream_t stream);

/* View-sharded multi-GPU mode (second mode: one exchange step): every rank lifts ITS views with
 * ivx_backproject_sum_fwd -- same geometry, but the raw sum over the rank's views (volume_sum [B,X,Y,Z,C]) and the
 * per-voxel number of views that saw the voxel (count [B,X,Y,Z] int32) instead of the mean --, the two tensors are
 * all-reduced over the ranks (RCCL), and ivx_volume_normalize_fwd turns the totals into the reference's result in
 * place: volume = count ? sum / count : 0, valid = count > 0 (detectors/imvoxelnet.py:70-74).  C % 4 == 0.
 * The view sum is then ordered rank by rank instead of strictly by view: equal to the single-GPU result to fp32
 * rounding of the additions (the valid mask is exact).                                                         */
/* ivx_backproject_mean_fwd that also leaves one max |volume| per workgroup (single view only: ivx_backproject_amax_blocks floats, 0 when the
 * shape does not take that kernel) for the operand scale of the first neck layer (ivx_conv_winograd_input_amax). */
int32_t ivx_backproject_amax_blocks(int32_t B, int32_t V, int32_t X, int32_t Y, int32_t Z);
int ivx_backproject_mean_fwd_amax(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                                  const float *new_origin, const int32_t *crop_hw, const float *voxel_size, int32_t X, int32_t Y,
                                  int32_t Z, float *volume, uint8_t *valid, float *partials, ivx_stream_t stream);
int ivx_backproject_sum_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                            const float *proj, const float *new_origin, const int32_t *crop_hw,
                            const float *voxel_size, int32_t X, int32_t Y, int32_t Z, float *volume_sum,
                            int32_t *count, ivx_stream_t stream);
int ivx_volume_normalize_fwd(float *volume, const int32_t *count, int64_t n_voxels, int32_t C, uint8_t *valid,
                             ivx_stream_t stream);

/* Streaming scenes: the views of a scene arrive one after another and are folded into a running volume.
 * ivx_backproject_accum_fwd adds the V views of this call to a caller-owned state and, optionally, emits the mean in the same
 * pass.  Geometry and arithmetic are ivx_backproject_mean_fwd's (same kernel template).  C % 4 == 0, C <= 1024.
 *
 * feat        [B*V, FH, FW, C]      features of the NEW views only (fp32; bf16 for the _bf16 form)
 * proj        [B, V, 3, 4]          their projection rows; new_origin [B,3], crop_hw [B,2], voxel_size as above
 * volume_sum  [B, X, Y, Z, C] fp32  in/out: running sum over the valid views (fp32 in both forms)
 * count       [B, X, Y, Z] int32    in/out: number of views that saw the voxel so far
 * first       != 0: the state starts from 0.f / 0 and is NOT read (no memset needed, uninitialised memory is never read);
 *             0: the accumulators start from the stored sum / count
 * mean_out    [B, X, Y, Z, C] or NULL  count ? sum / count : 0 after this call (fp32; bf16 with one rounding at the store for
 *             the _bf16 form); valid_out [B, X, Y, Z] u8 or NULL: count > 0.  Both given or both NULL; with NULL neither is written.
 * Ordering guarantee: a voxel's views are added strictly in view order with round-to-nearest fp32 additions, continuing the stored
 * sum.  Views that arrive in the same order therefore give, after the last call, bit for bit the volume and mask of ONE
 * ivx_backproject_mean_fwd over all of them, whatever the chunking.  One lane group owns a voxel: no atomics, reproducible.
 * IVX_ERR_INVALID_ARG before any launch: null state or inputs, only one of mean_out / valid_out, non-positive dims, C % 4 != 0,
 * a grid or feature stack beyond the 31-bit limits of ivx_backproject_mean_fwd.
 *
 * ivx_volume_mean_fwd is the out-of-place ivx_volume_normalize_fwd: out = count ? volume_sum / count : 0 (out_dtype IVX_F32 or
 * IVX_BF16), valid = count > 0, the sums stay intact -- the mean after calls that passed mean_out = NULL.                    */
int ivx_backproject_accum_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                              const float *new_origin, const int32_t *crop_hw, const float *voxel_size /*host*/, int32_t X, int32_t Y,
                              int32_t Z, float *volume_sum, int32_t *count, int32_t first, float *mean_out, uint8_t *valid_out,
                              ivx_stream_t stream);
int ivx_backproject_accum_fwd_bf16(const void *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                                   const float *new_origin, const int32_t *crop_hw, const float *voxel_size /*host*/, int32_t X, int32_t Y,
                                   int32_t Z, float *volume_sum, int32_t *count, int32_t first, void *mean_out, uint8_t *valid_out,
                                   ivx_stream_t stream);
int ivx_volume_mean_fwd(const float *volume_sum, const int32_t *count, int64_t n_voxels, int32_t C, void *out, int32_t out_dtype,
                        uint8_t *valid, ivx_stream_t stream);

/* (0.4.4) Sampling rule of the unprojection.  The entry points above gather the NEAREST pixel, as the reference does
 * (detectors/imvoxelnet.py:151-152); every reference-parity claim of this library is made for that rule.  IVX_SAMPLE_BILINEAR is an
 * optional extra mode outside those claims: the four pixels around the projected point, blended in fp32.  It is pinned to an fp64
 * reference written from the definition below (tests/ref_unproject.py), not to the reference implementation.
 *
 * Definition.  Points, projection chain, crop and the two quotients xf = u / d, yf = v / d (fp32, IEEE division) are those of
 * ivx_backproject_mean_fwd.
 *   validity  UNCHANGED: a view sees a voxel iff 0 <= rint(xf) < wc, 0 <= rint(yf) < hc and d > 0 (wc, hc: the crop clamped to the
 *             map).  The valid mask and the per-voxel view count are bit for bit those of the nearest rule.
 *   corners   x0 = floor(xf), x1 = x0 + 1, y0 = floor(yf), y1 = y0 + 1, each clamped to [0, wc-1] / [0, hc-1] (border rule; a valid
 *             sample has xf in [-0.5, wc-0.5], so a clamp moves a corner by at most one pixel); converted to int after the validity test.
 *   weights   ax = xf - floorf(xf), ay = yf - floorf(yf)                       (one fp32 subtraction each, exact for xf, yf >= 0)
 *             bx = 1 - ax, by = 1 - ay                                          (fp32 subtractions)
 *             w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay        (fp32 products; wXY weighs pixel (xX, yY))
 *   blend     sample = fma(w11, f11, fma(w01, f01, fma(w10, f10, w00 * f00)))   (ONE fixed order: a rounded product, then three fused
 *             multiply-adds, innermost first; f = the pixel's value converted to fp32)
 *   mean      the samples are added over the valid views in view order (fp32 additions) and divided by the count (IEEE division),
 *             0 where no view sees the voxel -- as for the nearest rule.  bf16 storage: weights, blend, sum and division in fp32, one
 *             rounding at the store.
 * With ax = ay = 0 the sample is the nearest pixel's value (as a number: -0 becomes +0).  One device function computes the sample in
 * every mode and element type and the view order is shared, so every chunking of the accumulate mode reproduces the one-shot launch
 * bit for bit, as for the nearest rule.
 *
 * ivx_backproject_fwd_ex is the one entry point for both rules and all modes; the entry points above keep their names and behaviour.
 *   mode IVX_LIFT_MEAN   volume [B,X,Y,Z,C] (feat_dtype) + valid; count and mean_out must be NULL
 *        IVX_LIFT_SUM    volume = fp32 view sum + count (ivx_backproject_sum_fwd); valid and mean_out must be NULL.  bf16 features: the
 *                        accumulate kernel from a zero state (fp32 sums)
 *        IVX_LIFT_ACCUM  volume = running fp32 sum + count, in/out, `first` as for ivx_backproject_accum_fwd; mean_out (feat_dtype) and
 *                        valid both given or both NULL
 * With sampling = IVX_SAMPLE_NEAREST it runs what the entry points above run (same checks, same launches).  A single-view bilinear lift
 * runs the multi-view kernel (bf16 maps through the bf16 kernel; no per-workgroup maxima: ivx_backproject_amax_blocks describes the
 * nearest single-view kernel only).  IVX_ERR_INVALID_ARG before any launch: a null descriptor, an unknown sampling, mode or feat_dtype,
 * and the rules of the mode's entry point above -- null or superfluous pointers, non-positive dims, C % 4 != 0 (every form but the fp32
 * mean), C above 1024 (256 when C % 4 != 0), a grid or feature stack beyond the 31-bit limits, B > 65535.                    */
#define IVX_SAMPLE_NEAREST 0
#define IVX_SAMPLE_BILINEAR 1
#define IVX_LIFT_MEAN 0
#define IVX_LIFT_SUM 1
#define IVX_LIFT_ACCUM 2
typedef struct ivx_backproject_desc {
  int32_t B, V, FH, FW, C, X, Y, Z;
  float voxel_size[3];
  int32_t feat_dtype; /* IVX_F32 | IVX_BF16: element type of feat, of the mean volume and of mean_out */
  int32_t mode;       /* IVX_LIFT_MEAN | IVX_LIFT_SUM | IVX_LIFT_ACCUM */
  int32_t sampling;   /* IVX_SAMPLE_NEAREST | IVX_SAMPLE_BILINEAR */
  int32_t first;      /* IVX_LIFT_ACCUM only */
} ivx_backproject_desc;
int ivx_backproject_fwd_ex(const ivx_backproject_desc *d, const void *feat, const float *proj, const float *new_origin,
                           const int32_t *crop_hw, void *volume, int32_t *count, void *mean_out, uint8_t *valid, ivx_stream_t stream);

/* (0.4.6) Gathered mean lift: the views are listed by slot.  A caller that keeps the maps of a changing set of views (a sliding window over a
 * scan, a replaced keyframe: scene.py) lifts the set it holds NOW in one launch, straight from its ring of slots, with no copy into a
 * contiguous stack and no subtraction from a running sum.
 *
 * d           the descriptor of ivx_backproject_fwd_ex; d->V is the number of LISTED views per sample, d->mode must be IVX_LIFT_MEAN,
 *             sampling and feat_dtype as there; C % 4 == 0, C <= 1024
 * feat_pool   [S, FH, FW, C]   (feat_dtype) the slots' FPN level-0 maps
 * proj_pool   [S, 3, 4]        the slots' projection rows
 * view_slot   [B, V] int32     DEVICE: view v of sample b is slot view_slot[b*V + v] of both pools
 * new_origin, crop_hw, volume [B,X,Y,Z,C] (feat_dtype), valid [B,X,Y,Z] u8: as for the mean mode of ivx_backproject_fwd_ex
 * Contract.  The result equals ivx_backproject_fwd_ex (IVX_LIFT_MEAN, same sampling and feat_dtype) over a contiguous copy of the listed
 * views, in list order, bit for bit: the same kernel template, of which only the projecting lane's addressing differs.  (One listed view runs
 * this kernel too: its sum starts from +0, so a -0 feature comes out as +0 where the nearest single-view copy kernel keeps the sign.)  Slots may
 * repeat: a slot listed twice counts as two views.  A slot outside [0, S) is an unseen view: nothing of it is read and no voxel counts it
 * (a guard in the kernel, tested before any address is formed; callers should validate their lists).  Unlisted slots are never read, so
 * they may hold anything.
 * IVX_ERR_INVALID_ARG before any launch: a null descriptor or pointer, S <= 0, non-positive dims, C % 4 != 0, C > 1024, a mode other than
 * IVX_LIFT_MEAN, an unknown sampling or feat_dtype, X*Y*Z or S*FH*FW at or beyond 2^31, B > 65535 (or B*V at or beyond 2^31).          */
int ivx_backproject_gather_fwd(const ivx_backproject_desc *d, int32_t S, const void *feat_pool, const float *proj_pool,
                               const int32_t *view_slot /*device [B,V]*/, const float *new_origin, const int32_t *crop_hw,
                               void *volume, uint8_t *valid, ivx_stream_t stream);

/* (0.4.7) Listed lift with per-sample state: N scenes that share pools, ragged numbers of views.  The gathered form above in the mean AND the
 * accumulate mode, in which every sample names the row of the state / output pools it owns and, in the accumulate mode, carries its own `first`
 * flag.  A batch of streaming scenes (scene.py, SceneBatch) adds this tick's views -- 0, 1 or several per scene -- to the touched scenes in ONE
 * launch; a one-shot batch whose samples have different numbers of views (simple_test_ragged) lifts in one launch too.
 *
 * d           the descriptor of ivx_backproject_fwd_ex; d->B samples, d->V = the length of a row of view_slot (the longest list); d->mode
 *             IVX_LIFT_MEAN or IVX_LIFT_ACCUM (IVX_LIFT_SUM is refused); both sampling rules, both feat_dtypes; C % 4 == 0, C <= 1024
 * l->S, feat_pool [S,FH,FW,C], proj_pool [S,3,4]: as for ivx_backproject_gather_fwd
 * l->view_slot  DEVICE [B, V] int32: view v of sample b is that slot of both pools; a slot outside [0, S) is no view, so -1 pads ragged rows
 *               (anywhere in a row, not only at its end)
 * l->R, l->row  the pools volume / count / mean_out / valid have R rows ([R,X,Y,Z,C] / [R,X,Y,Z]); DEVICE [B] int32 or NULL: sample b reads and
 *               writes row row[b]; NULL: row b (then R >= B)
 * l->first      DEVICE [B] int32 or NULL, IVX_LIFT_ACCUM only: sample b starts its row from zero without reading it where first[b] != 0;
 *               NULL: d->first for every sample
 * new_origin [B,3], crop_hw [B,2]: per SAMPLE (indexed by b, not by row)
 * pointer rules per mode: those of ivx_backproject_fwd_ex (mean: volume + valid, no count / mean_out; accumulate: volume = fp32 sums + count,
 *               mean_out and valid both given or both NULL)
 * Contract.
 *   Equality.   For every sample b, row row[b] of volume / count / mean_out / valid after the call is bit for bit what the B = 1 launch of
 *               ivx_backproject_fwd_ex leaves (same mode, sampling and feat_dtype, first = first[b]) over a contiguous copy of sample b's
 *               in-range listed views in list order, starting from that row's stored state: the view-order fp32 addition chain, the sample
 *               function, the division and the stores are the shared code of the one kernel template.
 *   Zero views. A sample whose row of view_slot holds no in-range slot adds nothing: with first[b] != 0 its state becomes zero sum / zero count
 *               (mean 0 / valid 0 where emitted); with first[b] == 0 its state is stored back unchanged, bit for bit (mean / valid, where
 *               emitted, are those of the stored state).
 *   Untouched rows.  Rows named by no sample are neither read nor written.
 *   Row guard.  A row[b] outside [0, R) makes sample b do nothing at all (tested per workgroup before any address is formed, like the slot guard).
 *   Distinct rows.  The rows of one call must be distinct: two samples on one row race.  This entry cannot check a device list; callers validate
 *               (ops.backproject_lists_accum_ / _mean_ take the rows as a host list and always do).
 *   Same as the gather.  With row == NULL, first == NULL and IVX_LIFT_MEAN the launch and the bits are those of ivx_backproject_gather_fwd.
 * IVX_ERR_INVALID_ARG before any launch: everything ivx_backproject_gather_fwd rejects (with this entry's modes), a null l, R <= 0 (or R < B with
 * no row list), first != NULL in the mean mode, the sum mode.                                                                                    */
typedef struct ivx_lift_lists {
  int32_t S;                 /* slots of feat_pool / proj_pool */
  int32_t R;                 /* rows of volume / count / mean_out / valid */
  const int32_t *view_slot;  /* DEVICE [B, V]: view v of sample b is that slot; a slot outside [0, S) is no view (-1 pads ragged rows) */
  const int32_t *row;        /* DEVICE [B] or NULL (= b): sample b reads and writes THIS row of the output / state pools */
  const int32_t *first;      /* DEVICE [B] or NULL (= d->first for every sample); IVX_LIFT_ACCUM only */
} ivx_lift_lists;
int ivx_backproject_lists_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const void *feat_pool, const float *proj_pool,
                              const float *new_origin /*[B,3]*/, const int32_t *crop_hw /*[B,2]*/, void *volume, int32_t *count,
                              void *mean_out, uint8_t *valid, ivx_stream_t stream);

/* (0.4.8) Weighted listed lift: every view carries a confidence, the running state fades by a factor per call and a voxel that has not been seen
 * for long enough becomes unseen again -- the weighted running mean of a fusing volume, with O(1) state (fading scenes: scene.py,
 * open_scene(meta, decay=...)).  It is ivx_backproject_lists_fwd with three more inputs and one more state field; like the bilinear rule it lies
 * outside the reference-parity claims and is pinned to an fp64 reference written from the definition below (tests/ref_unproject_weighted.py).
 *
 * Definition.  The geometry, the validity rule, both sampling rules and the sample function are those of ivx_backproject_lists_fwd.  Per voxel
 * and per channel, in this order, every operation fp32 and round-to-nearest:
 *   1. start   S (the sum, [C]), W (the weight sum) and cnt are loaded from the sample's row of volume / wsum / count; with `first` they are
 *              +0, +0, 0 and the row is not read.
 *   2. fade    (accumulate mode, and only when the row was read)  lambda = decay[b]:
 *              if lambda != 1:  S = lambda * S, W = lambda * W                     (one rounded product each; lambda == 1 multiplies nothing)
 *              then, if forget_below > 0 and !(W >= forget_below):  S = +0, W = +0, cnt = 0        (the voxel is unseen again)
 *              The branch on lambda is uniform per sample.  For every W >= 0 -- every W this entry ever stores -- the forgetting rule is
 *              "!(W >= forget_below)"; the threshold 0 forgets nothing, so that with forget_below == 0 and lambda == 1 the state of a sample that
 *              adds nothing is stored back with every bit pattern intact (no arithmetic touches it), as for ivx_backproject_lists_fwd.
 *   3. add     over the listed views in list order.  A view counts only if its slot is in [0, S) and its weight w = view_weight[slot] passes
 *              w > 0 && w < inf: NaN, 0, negative values and +inf fail, and such a view is an unseen view, exactly like a slot outside [0, S) (its
 *              projection rows may be read, its map is not).
 *              The view must also see the voxel.  Then  S = fma(w, sample, S),  W = W + w,  ++cnt.
 *   4. store   S, W and cnt are stored.  Where the mean is emitted: mean = W > 0 ? S / W : 0 (IEEE division; one rounding to bf16 in bf16
 *              storage), valid = W > 0.
 * The mean mode has no state and no fade: steps 3 and 4 from zero, and only volume (the mean) and valid are written.
 * cnt is the number of counted views since the voxel was last forgotten.
 *
 * w->view_weight  DEVICE [S] fp32: the weight of slot s (indexed by slot, like the pools); NULL: 1 for every slot
 * w->decay        DEVICE [B] fp32 or NULL (= 1): lambda of sample b (indexed by b, not by row); IVX_LIFT_ACCUM only
 * w->forget_below >= 0, finite; IVX_LIFT_ACCUM only (must be 0 in the mean mode)
 * w->wsum         DEVICE [R,X,Y,Z] fp32 in/out, a state pool beside volume and count; IVX_LIFT_ACCUM: required; mean mode: must be NULL
 * Everything else, and every rule of ivx_backproject_lists_fwd (rows, row guard, distinct rows, untouched rows, `first`), as there.
 *
 * Properties that follow from the definition.
 *   Unit weights.  With every weight 1, every decay 1 and forget_below 0, the fields volume, count, mean_out and valid are bit for bit those of
 *               ivx_backproject_lists_fwd on the same lists, and wsum == (float)count: fma(1, f, S) is S + f rounded once, and a sum of k ones
 *               is exact below 2^24.
 *   Zero weight.  A view of weight 0 (or NaN, negative, +inf) is bit for bit the same call with that view not listed.
 *   Power-of-two scale.  Multiplying all weights by 2^k leaves the mean and the mask bit-identical; the sums and wsum scale exactly
 *               (barring overflow and underflow).
 *   Guards.     No address depends on a weight or on a decay: bad values can only change numbers.
 * IVX_ERR_INVALID_ARG before any launch: everything ivx_backproject_lists_fwd rejects, a null w, a missing wsum in the accumulate mode, a
 * superfluous wsum, a decay list or a nonzero forget_below in the mean mode, a negative or non-finite forget_below.
 *
 * ivx_volume_wmean_fwd is the out-of-place mean of a (sum, weight sum) state after calls that passed mean_out = NULL: out = wsum > 0 ?
 * volume_sum / wsum : 0 (out_dtype IVX_F32 or IVX_BF16), valid = wsum > 0 -- bit for bit the mean_out / valid of the same state.             */
typedef struct ivx_lift_weights {
  const float *view_weight;  /* DEVICE [S], the weight of slot s; NULL = 1 for every slot */
  const float *decay;        /* DEVICE [B] or NULL (= 1); IVX_LIFT_ACCUM only */
  float forget_below;        /* >= 0, finite; IVX_LIFT_ACCUM only (must be 0 in the mean mode) */
  float *wsum;               /* DEVICE [R,X,Y,Z] fp32 in/out; IVX_LIFT_ACCUM: required; mean mode: must be NULL */
} ivx_lift_weights;
int ivx_backproject_weighted_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_weights *w, const void *feat_pool,
                                 const float *proj_pool, const float *new_origin /*[B,3]*/, const int32_t *crop_hw /*[B,2]*/, void *volume,
                                 int32_t *count, void *mean_out, uint8_t *valid, ivx_stream_t stream);
int ivx_volume_wmean_fwd(const float *volume_sum, const float *wsum, int64_t n_voxels, int32_t C, void *out, int32_t out_dtype, uint8_t *valid,
                         ivx_stream_t stream);

/* (0.5.0) Pixel maps for the weighted listed lift: every view may bring a per-pixel confidence and a measured depth per pixel, both at feature
 * resolution, and the lift honours them in its one launch.  The confidence multiplies the view's weight per pixel (a person walking through the
 * scan, the robot's own arm, the black border after undistortion); the depth, with a gate (behind, front), lets a view count at a voxel only
 * where the voxel lies within the gate of the surface the pixel shows (occlusion carving, or a truncation band, for RGB-D cameras) instead of
 * smearing the pixel's feature along its whole ray.  It is ivx_backproject_weighted_fwd with one more struct; like the bilinear rule, fading
 * and scrolling it lies outside the reference-parity claims and is pinned to an fp64 reference written from the definition below
 * (tests/ref_unproject_maps.py).
 *
 * Definition.  Everything in the definition of ivx_backproject_weighted_fwd stays: start, fade, forget, store, both modes, both sampling rules,
 * both storage types, rows, `first`, guards.  Only step 3, "a view counts", gains two tests.  Both are evaluated at the NEAREST pixel (xr, yr) =
 * (rint(u / d), rint(v / d)), the pixel the validity rule rounds to -- under the bilinear rule as well: the mask is the nearest rule's, and so
 * are the maps.  Every operation is fp32, round-to-nearest, no contraction.
 *   As before: the view's slot is in [0, S); its weight wv = view_weight[slot] passes wv > 0 && wv < inf; the view sees the voxel, with third
 *              homogeneous coordinate d -- the d of the validity test; with the usual intrinsic (last row 0 0 1) the depth along the optical
 *              axis in the extrinsic's units.
 *   3a. gate   (depth != NULL)  D = depth[slot, yr, xr].  If D > 0 && D < inf (a measurement) the view counts only if d <= D + behind and
 *              d >= D - front; the sum and the difference are each rounded once.  A pixel without a measurement (0, negative, NaN, +inf)
 *              gates nothing.
 *   3b. weight w = wv * pixel_weight[slot, yr, xr], one rounded product (w = wv when the map is NULL).  The view counts only if
 *              w > 0 && w < inf.
 *   Then, as before:  S = fma(w, sample, S),  W = W + w,  ++cnt.
 * No address depends on a map's value, and the map addresses are formed from slot and pixel only after the validity test has passed: unlisted
 * slots of the maps, and pixels no voxel projects to, are never read.
 *
 * m->pixel_weight  DEVICE [S, FH, FW] fp32, indexed by slot like the pools; NULL: 1 everywhere
 * m->depth         DEVICE [S, FH, FW] fp32, in the units of the third homogeneous coordinate; NULL: no gate
 * m->behind, m->front  >= 0, may be +inf (no limit on that side), never NaN; read only when depth != NULL
 * Everything else as for ivx_backproject_weighted_fwd.
 *
 * Properties that follow from the definition.
 *   No maps.       m == NULL, or both pointers NULL, launches the kernel of ivx_backproject_weighted_fwd and gives its bits.
 *   Neutral maps.  A pixel_weight of all ones gives, bit for bit, ivx_backproject_weighted_fwd (wv * 1 is wv).  So does a depth of nothing but
 *                  non-measurements, and so does any depth with behind = front = +inf.
 *   Constant map.  pixel_weight[slot] == c everywhere is bit for bit ivx_backproject_weighted_fwd with view_weight[slot] replaced by the
 *                  rounded wv * c.
 *   Blocked view.  A pixel_weight that is 0, NaN, negative or +inf on every pixel of a slot is bit for bit the call with that view not listed;
 *                  so is a gate that excludes every voxel the view sees.
 *   Power of two.  Scaling every pixel_weight by 2^k keeps the mean and the mask bit-identical and scales the sums and wsum exactly
 *                  (barring overflow and underflow).
 * IVX_ERR_INVALID_ARG before any launch: everything ivx_backproject_weighted_fwd rejects; depth != NULL with a behind or front that is
 * negative or NaN.                                                                                                                       */
typedef struct ivx_lift_maps {
  const float *pixel_weight; /* DEVICE [S, FH, FW] fp32, indexed by slot like the pools; NULL = 1 everywhere */
  const float *depth;        /* DEVICE [S, FH, FW] fp32, same units as the third homogeneous coordinate; NULL = no gate */
  float behind, front;       /* >= 0, may be +inf (no limit on that side), never NaN; read only when depth != NULL */
} ivx_lift_maps;
int ivx_backproject_mapped_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_weights *w, const ivx_lift_maps *m,
                               const void *feat_pool, const float *proj_pool, const float *new_origin /*[B,3]*/, const int32_t *crop_hw /*[B,2]*/,
                               void *volume, int32_t *count, void *mean_out, uint8_t *valid, ivx_stream_t stream);

/* (0.4.9) In-place voxel shift of rows of the state pools: a scene's grid moves with its platform (scrolling scenes: scene.py,
 * SceneSession.scroll / SceneBatch.scroll).  Moving the state by whole voxels is a pure move of bits, and everything a scene does afterwards is
 * the existing lift at the moved origin, so the operation is pinned bit for bit with no tolerance (tests/ref_volume_scroll.py restates the
 * definition in numpy).  Like the bilinear rule and fading it lies outside the reference-parity claims.
 *
 * Definition.  For sample b with r = row[b] and (sx, sy, sz) = shift[3b .. 3b+2], on row r of every field:
 *     new[i,j,k] = old[i+sx, j+sy, k+sz]      where (i+sx, j+sy, k+sz) lies inside [0,X) x [0,Y) x [0,Z)
 *     new[i,j,k] = unseen                      everywhere else: sums +0, count 0, weight sum +0 (all bits zero)
 *   The fields are moved as raw words -- volume_sum as 16-byte words, count and wsum as 4-byte words -- with no float arithmetic.
 *
 * B           samples of this call
 * row         HOST [B] int32: sample b moves row row[b] of the pools
 * shift       HOST [B,3] int32: its shift in voxels along x, y, z (any int32; content at index i+s is afterwards at index i)
 * R, X, Y, Z, C  the pools have R rows of X*Y*Z voxels; C % 4 == 0
 * volume_sum  DEVICE [R,X,Y,Z,C] fp32 in/out, 16-byte aligned
 * count       DEVICE [R,X,Y,Z] int32 in/out
 * wsum        DEVICE [R,X,Y,Z] fp32 in/out, or NULL (a state without a weight sum)
 * row and shift are host lists on purpose: unlike the device lists of the lifts this entry checks everything before any launch, and nothing
 * is uploaded (rows and shifts reach the kernel by value, 32 samples per launch).
 *
 * Properties.
 *   Named rows.      Bit for bit the definition: every bit pattern survives the move, NaN payloads, -0 and denormals included.
 *   Untouched rows.  Rows named by no sample are neither read nor written.
 *   In place.        No scratch, no atomics, no barriers: one pass per axis with a non-zero shift, in the order x, y, z (the three axis maps
 *                    commute, so the order does not show in the result), at most three launches for the sums and three for count / wsum per 32
 *                    samples.  csrc/volume_scroll.hip states why a pass may overwrite the line it reads.
 *   Large shifts.    |s| >= the axis length on any axis leaves the row all zero.
 *   Zero shifts.     A sample whose shift is (0,0,0) is not touched; a call whose shifts are all zero is valid and launches nothing.
 *   Composition.     scroll(s) then scroll(t) equals scroll(s + t) on every voxel whose source stayed inside the grid in between, and zero elsewhere;
 *                    scroll(s) then scroll(-s) zeroes exactly the shell the first one vacated.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: a null row, shift, volume_sum or count; a non-positive B, R, X, Y,
 * Z or C; C % 4 != 0; X*Y*Z at or beyond 2^31; a row outside [0, R); two samples on one row (they would race).                                  */
int ivx_volume_scroll_fwd(int32_t B, const int32_t *row /*host [B]*/, const int32_t *shift /*host [B,3]*/, int32_t R, int32_t X, int32_t Y, int32_t Z,
                          int32_t C, float *volume_sum, int32_t *count, float *wsum /*or NULL*/, ivx_stream_t stream);

/* (0.5.4) Rigid resample of rows of the state pools: a scene's state is brought into a frame that has turned and moved by any amount while the grid
 * stays where the head expects it (scenes that turn with their platform: scene.py, SceneSession.warp / SceneBatch.warp).  A fading state (sum,
 * weight sum) resamples linearly: both take the same trilinear weights, so the mean stays a convex combination of neighbouring means.  Out of
 * place, because a resample reads the neighbours of what it writes.  Like the bilinear rule, fading and scrolling it lies outside the
 * reference-parity claims and is pinned to an fp64 reference written from the definition below (tests/ref_volume_warp.py).
 *
 * Definition.  Every operation is fp32, round-to-nearest, no contraction.  M = xform[b] [3,4] maps a point of the NEW grid frame to the OLD frame
 * in which the state was written: x_old = R x_new + t.  For sample b and destination voxel (i,j,k) of row row_dst[b], reading row row_src[b]:
 *   1. centre   p_a = float(idx_a) * voxel_size_a + new_origin_a                              (a product, a sum: the lift's voxel centre)
 *   2. source   q_a = fma(M_a3, 1, fma(M_a2, p_z, fma(M_a1, p_y, M_a0 * p_x)))                (the lift's projection row)
 *   3. grid     g_a = (q_a - new_origin_a) / voxel_size_a     one rounded difference, one IEEE division.  If !(g_a > -1 && g_a < N_a) on any
 *               axis (N = X, Y, Z; NaN and inf fail too) the voxel becomes unseen -- sums +0, weight sum +0, count 0 -- and nothing is read.
 *               Otherwise i0_a = floor(g_a) and f_a = g_a - i0_a, one rounded difference (exact for g_a >= 0; for g_a in (-2^-24, 0) it rounds
 *               to 1, which puts the whole weight on index 0).
 *   4. corners  The eight corners (i0_x + dx, i0_y + dy, i0_z + dz) in the order dx, dy, dz with dz fastest.  Axis weights: 1 - f_a (one
 *               rounding) for d = 0, f_a for d = 1; corner weight w = (w_x * w_y) * w_z, two rounded products.  A corner outside the grid, or
 *               with w == 0 exactly, is not read and contributes nothing.  Starting from +0, over the corners that are read:
 *                   S'[c] = fma(w, S_corner[c], S'[c]) per channel,   W' = fma(w, W_corner, W'),   cnt' = max(cnt', cnt_corner).
 *   5. forget   if forget_below > 0 && !(W' >= forget_below):  S' = +0, W' = +0, cnt' = 0     (the weighted lift's rule)
 *   6. store    S', W', cnt' into row row_dst[b].  Every voxel of a named destination row is written.
 *
 * B            samples of this call
 * row_src      HOST [B] int32: sample b reads row row_src[b] of the source pools (two samples may read one row)
 * row_dst      HOST [B] int32: ... and writes row row_dst[b] of the destination pools; distinct
 * xform        HOST [B,3,4] fp32, finite; rigidity is NOT required here (ops.volume_warp checks it)
 * new_origin   HOST [B,3] fp32, finite: the grid's corner term, the new_origin of the lifts
 * voxel_size   HOST [3] fp32, finite and > 0
 * forget_below >= 0, finite
 * R_src, R_dst, X, Y, Z, C   the source / destination pools have R_src / R_dst rows of X*Y*Z voxels; C % 4 == 0
 * sum_src, wsum_src, count_src   DEVICE [R_src,X,Y,Z,C] fp32 (16-byte aligned), [R_src,X,Y,Z] fp32, [R_src,X,Y,Z] int32
 * sum_dst, wsum_dst, count_dst   DEVICE the same with R_dst rows, written
 * The lists are host lists, as for ivx_volume_scroll_fwd: everything is checked before any launch and nothing is uploaded (rows, transforms and
 * origins reach the kernel by value, 32 samples per launch).
 *
 * Properties.
 *   Untouched rows.  Rows named by no sample are neither read (source) nor written (destination).
 *   Zero weights.    A corner of weight 0 is never read, so an unseen, NaN or inf cell there cannot leak.  Where g is an integer on all three axes
 *                    a voxel has one corner, of weight 1: S' = fma(1, S, +0) is S with every bit (of a finite or infinite S; -0 becomes +0 and a NaN
 *                    stays a NaN), W' and cnt' likewise.  A transform whose g is integer everywhere -- a whole-voxel translation on a grid where
 *                    the chain above is exact, a quarter turn about the centre of a square one -- makes the call a permutation of the voxels, equal
 *                    to ivx_volume_scroll_fwd for the translation.
 *   Constant mean.   S / W == c on every read corner gives S' / W' == c within a few ulp.
 *   Thinning.        At the grid's border and at the edge of what was seen both sums lose the same weights: evidence thins, and the mean S' / W'
 *                    stays a convex combination of the neighbouring means.
 *   Error.           Against the exact value of step 4 on the same i0 and f:  |S' - exact| <= 11 * 2^-24 * sum_corners |w S_corner| (+ 2^-126): one
 *                    rounding in 1 - f, two in the products, eight accumulations (tests/ref_volume_warp.py derives it); the same for W'.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: a null pointer; a non-positive B, R_src, R_dst, X, Y, Z or C;
 * C % 4 != 0; X*Y*Z at or beyond 2^31; a row outside its pool; two samples on one destination row; source and destination sum pools that overlap
 * in memory (or are not 16-byte aligned); a non-finite xform, new_origin or voxel_size; voxel_size <= 0; a negative or non-finite forget_below. */
int ivx_volume_warp_fwd(int32_t B, const int32_t *row_src /*host [B]*/, const int32_t *row_dst /*host [B]*/, const float *xform /*host [B,3,4]*/,
                        const float *new_origin /*host [B,3]*/, const float *voxel_size /*host [3]*/, float forget_below, int32_t R_src, int32_t R_dst,
                        int32_t X, int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const int32_t *count_src,
                        float *sum_dst, float *wsum_dst, int32_t *count_dst, ivx_stream_t stream);

/* (0.5.5) Rigid merge of rows of the state pools: the fused state of one scene is ADDED to another's under a rigid transform that relates their
 * frames (two robots or two passes that fused the same rooms, a relocalisation against an earlier map, two rows of a batch that turn out to be one
 * flat: scene.py, SceneSession.merge / SceneBatch.merge).  A fading state (sum, weight sum, count) is linear, so two states named in one frame add;
 * the source is read by the trilinear rule of ivx_volume_warp_fwd -- the same kernel, a second instantiation of csrc/volume_warp.hip -- and added in
 * place: no scratch row, voxels the source never saw are not rewritten, and the two grids may have different origins (a scrolled scene).  Like the
 * warp it lies outside the reference-parity claims and is pinned to an fp64 reference written from the definition below (tests/ref_volume_merge.py).
 *
 * Definition.  Every operation is fp32, round-to-nearest, no contraction.  M = xform[b] [3,4] maps a point of the DESTINATION grid's frame to the
 * SOURCE grid's frame: x_src = R x_dst + t.  For sample b and voxel (i,j,k) of destination row row_dst[b], reading source row row_src[b]:
 *   1. centre   p_a = float(idx_a) * voxel_size_a + origin_dst[b]_a                           (warp step 1: the lift's voxel centre)
 *   2. source   q_a = fma(M_a3, 1, fma(M_a2, p_z, fma(M_a1, p_y, M_a0 * p_x)))                (warp step 2: the same fma chain)
 *   3. grid     g_a = (q_a - origin_src[b]_a) / voxel_size_a: the grid coordinate in the SOURCE grid.  The inside test !(g_a > -1 && g_a < N_a),
 *               i0_a = floor(g_a) and f_a = g_a - i0_a are exactly warp step 3, taken against the source origin.
 *   4. sample   S_s[c], W_s and cnt_s exactly as warp step 4: the same corner order and weights (w_x * w_y) * w_z; a corner outside the grid or
 *               with w == 0 is not read; the fma chains start from +0; cnt_s is the maximum over the corners read.
 *   5. merged?  The voxel is merged iff it is inside and W_s > 0 (the state's own "seen" rule).  Otherwise the destination voxel is NOT WRITTEN:
 *               source evidence that is unseen, outside or NaN changes no bit of the destination.
 *   6. add      S'[c] = fma(alpha_b, S_s[c], S_d[c]),   W' = fma(alpha_b, W_s, W_d),   cnt' = min(cnt_d + cnt_s, 2^31 - 1), formed in 64 bits.
 *   7. forget   if forget_below > 0 && !(W' >= forget_below):  S' = +0, W' = +0, cnt' = 0     (the weighted lift's rule; it can only fire where
 *               W_d was below the threshold, that is 0 in a session's state, and alpha * W_s is small: the session's invariant is kept)
 *   8. store    S', W', cnt' into the destination voxel.  In place on the destination: a voxel reads only itself there, so there is no race.
 *
 * B            samples of this call
 * row_src      HOST [B] int32: sample b reads row row_src[b] of the source pools (two samples may read one row)
 * row_dst      HOST [B] int32: ... and adds into row row_dst[b] of the destination pools; distinct
 * xform        HOST [B,3,4] fp32, finite; rigidity is NOT required here (ops.volume_merge_ checks it)
 * origin_dst   HOST [B,3] fp32, finite: the corner term (the new_origin of the lifts) of the destination grid
 * origin_src   HOST [B,3] fp32, finite: ... and of the source grid
 * alpha        HOST [B] fp32, finite and > 0: the weight of the source's evidence
 * voxel_size   HOST [3] fp32, finite and > 0, common to both grids
 * forget_below >= 0, finite
 * R_src, R_dst, X, Y, Z, C   the source / destination pools have R_src / R_dst rows of X*Y*Z voxels; C % 4 == 0
 * sum_src, wsum_src, count_src   DEVICE [R_src,X,Y,Z,C] fp32 (16-byte aligned), [R_src,X,Y,Z] fp32, [R_src,X,Y,Z] int32, read only
 * sum_dst, wsum_dst, count_dst   DEVICE the same with R_dst rows, read and written.  They may BE the source pools (the same base and R_src ==
 *              R_dst: rows of one batch) as long as no row is named both as a source and as a destination; any other overlap is refused.
 * The lists are host lists, as for ivx_volume_warp_fwd: everything is checked before any launch and nothing is uploaded (32 samples per launch).
 *
 * Properties.
 *   Untouched.   Rows that no sample names are neither read nor written.  Unmerged voxels of named rows are not written and their sums are not
 *                read (the weight sum and count of a voxel whose source point lies inside the grid are loaded beside the corners, before the
 *                decision).  The source pools are read only.
 *   Empty destination.  On an all-zero destination row, with alpha = 1 and origin_src == origin_dst, the row after the call equals bit for bit
 *                what ivx_volume_warp_fwd writes for the same source, transform and forget_below -- on valid states (W = 0 implies S = 0, cnt = 0).
 *   Identity.    M = I and equal origins on a grid where the chain is exact (dyadic voxel sizes, the origin on their lattice): every merged voxel
 *                has one corner of weight 1, so S' = fma(alpha, S_s, S_d) -- with alpha = 1 the correctly rounded S_d + S_s, with alpha = 0.5
 *                S_d + 0.5 * S_s, bit for bit -- W' by the same rule, and the counts add.
 *   Error.       Against the exact value of steps 4 and 6 on the same i0 and f:
 *                    |S' - exact| <= |alpha| * 11 * 2^-24 * sum_corners |w S_corner| + 2^-24 * |exact| + 2^-126
 *                (the warp's derived K = 11 on the sample, one rounding of the final fma; tests/ref_volume_merge.py); the same for W'.  Counts are equal.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: everything ivx_volume_warp_fwd rejects (a null pointer; a
 * non-positive B, R_src, R_dst, X, Y, Z or C; C % 4 != 0; X*Y*Z at or beyond 2^31; a row outside its pool; two samples on one destination row; sum
 * pools that are not 16-byte aligned; a non-finite xform, origin or voxel_size; voxel_size <= 0; a negative or non-finite forget_below) with its
 * memory rule replaced by: source and destination sum pools that overlap without being the same pool; with the same pool, a row named both as a
 * source and as a destination.  And an alpha[b] that is not finite or not > 0.                                                                    */
int ivx_volume_merge_fwd(int32_t B, const int32_t *row_src /*host [B]*/, const int32_t *row_dst /*host [B]*/, const float *xform /*host [B,3,4]*/,
                         const float *origin_dst /*host [B,3]*/, const float *origin_src /*host [B,3]*/, const float *alpha /*host [B]*/,
                         const float *voxel_size /*host [3]*/, float forget_below, int32_t R_src, int32_t R_dst, int32_t X, int32_t Y, int32_t Z,
                         int32_t C, const float *sum_src, const float *wsum_src, const int32_t *count_src, float *sum_dst, float *wsum_dst,
                         int32_t *count_dst, ivx_stream_t stream);

/* (0.5.7) Scoring candidate poses between two rows of the state pools: how well do two fused scenes agree under a rigid transform?  scroll, warp,
 * merge and restore all take the transform between two frames as given; this entry judges one (scene.py, SceneSession.match / register,
 * SceneBatch.match / register).  Two fading states are per-voxel mean feature vectors with weights: for a candidate M the correlation of the two
 * means over the voxels both scenes have seen says how well they agree, and the trilinear read of the source is the merge's.  A read-only
 * reduction: it writes its outputs and its scratch, nothing else.  Like the merge it lies outside the reference-parity claims and is pinned to an
 * fp64 reference written from the definition below (tests/ref_volume_match.py).
 *
 * Definition.  Sample b names a destination row row_dst[b], a source row row_src[b] and the two grids' origins, as in ivx_volume_merge_fwd, and
 * carries K candidates M = xform[b,k] [3,4] that map the DESTINATION grid's frame to the SOURCE grid's: x_src = R x_dst + t.  The lattice step
 * (px, py, pz) >= 1 (NULL: 1, 1, 1) visits the destination voxels (i,j,k) with i % px == 0 && j % py == 0 && k % pz == 0, in ascending order of
 * (i, j, k) with k fastest.  For every visited voxel n of the row and every candidate k, in fp32, round-to-nearest, no contraction:
 *   1. own      W_d = wsum_dst[n]; the voxel is OWN iff W_d > 0 (a NaN is not).  own_out[b] counts the own voxels; it does not depend on k.
 *               Nothing further happens at a voxel that is not own.
 *   2. sample   steps 1 - 4 of ivx_volume_merge_fwd give inside, S_s[c] and W_s: the centre from origin_dst[b], the fma chain of M, the grid
 *               coordinate against origin_src[b] with the same inside test, floor and fraction, the same corner order and weights
 *               (w_x * w_y) * w_z, the fma chains from +0 over the corners read.  A corner outside the grid or of weight exactly 0 is not read.
 *               Counts are not read.
 *   3. paired   the voxel is PAIRED iff it is own, inside and W_s > 0.  Of an unpaired voxel only W_d and, where it is own and inside, the corner
 *               words of wsum_src are read: neither S_d nor any source sum.
 *   4. terms    r_d = 1 / W_d and r_s = 1 / W_s, one IEEE division each;  a_c = S_d[c] * r_d  and  b_c = S_s[c] * r_s, one rounded product
 *               each.  The channels of a voxel are taken in words of four, c = 4 w .. 4 w + 3.  Per word and per statistic, four rounded
 *               products and three rounded sums in channel order:
 *                   d_w = ((a_0 b_0 + a_1 b_1) + a_2 b_2) + a_3 b_3,   and the same with a a for na and b b for nb.
 *               An fp32 chain is never longer than these four terms: each d_w is widened to fp64 at once, and everything after it is fp64.
 *   5. sums     dot = sum d_w over the paired voxels and their words, na and nb likewise, in fp64, in an order that is a function of
 *               (X, Y, Z, C, step) alone: a lane's ascending walk, a fixed tree over the lanes of a wave, the waves of a workgroup in order, one
 *               partial per workgroup in the scratch slab, and a second launch that adds the partials of a candidate in a fixed order
 *               (csrc/volume_match.hip has the schedule).  pairs counts the paired voxels.
 *   6. outputs  pairs_out [B,K] int64 and own_out [B] int64, exact; stats_out [B,K,3] fp64 = (dot, na, nb).
 * The host forms the score: ncc = dot / sqrt(na * nb), the cosine of the two mean fields over the overlap, and overlap = pairs / own.
 *
 * B, K         samples of this call; candidates per sample
 * row_src      HOST [B] int32: sample b reads row row_src[b] of the source pools
 * row_dst      HOST [B] int32: ... and row row_dst[b] of the destination pools (rows may repeat: nothing is written)
 * xform        HOST [B,K,3,4] fp32, finite; rigidity is NOT required here (ops.volume_match checks it)
 * origin_dst, origin_src   HOST [B,3] fp32, finite: the corner terms (the new_origin of the lifts) of the two grids
 * voxel_size   HOST [3] fp32, finite and > 0, common to both grids
 * step         HOST [3] int32, each >= 1, or NULL for (1, 1, 1)
 * R_src, R_dst, X, Y, Z, C   the source / destination pools have R_src / R_dst rows of X*Y*Z voxels; C % 4 == 0
 * sum_src, wsum_src   DEVICE [R_src,X,Y,Z,C] fp32 (16-byte aligned), [R_src,X,Y,Z] fp32, read only
 * sum_dst, wsum_dst   DEVICE the same with R_dst rows, read only.  They may be the source pools, and a row may be matched against itself:
 *              there is no memory rule beyond the alignment.
 * pairs_out, own_out, stats_out   DEVICE [B,K] int64, [B] int64, [B,K,3] fp64, written
 * scratch      DEVICE, ivx_volume_match_scratch_bytes(B, K, X, Y, Z, C) bytes (-1 for non-positive arguments, C % 4 != 0 or X*Y*Z at or beyond
 *              2^31), 8-byte aligned; it serves every step
 * The lists are host lists, as for ivx_volume_merge_fwd: everything is checked before any launch and nothing is uploaded (the candidates reach
 * the kernel by value, 32 per launch, one sample per launch: B * ceil(K / 32) launches and one that sums).
 *
 * Properties.
 *   Read only.      The pools keep every bit; rows that no sample names are not read.
 *   Zero weights.   A corner of weight 0 is never read, and the sums of an unpaired voxel are never read: a NaN there cannot reach the statistics.
 *   Deterministic.  No float atomics, no spinning, no dependence between the workgroups of a launch.  The same two states give the same bits in
 *                   any row of any pool, alone or beside other samples and candidates.
 *   Identity.       M = I and equal origins on a grid where the chain is exact (dyadic voxel sizes, the origin on their lattice), source and
 *                   destination the same state: every paired voxel has one corner of weight 1, b_c == a_c bit for bit, so dot == na == nb bit
 *                   for bit and ncc == 1.
 *   Error.          Against the exact value of steps 2 - 5 on the same i0 and f, to first order, with A_c = |a_c| and
 *                   B_c = sum_corners |w S_corner[c]| / W_s (>= |b_c|):
 *                       |dot - exact| <= 31 * 2^-24 * sum A_c B_c,   |na - exact| <= 9 * 2^-24 * sum A_c^2,   |nb - exact| <= 53 * 2^-24 * sum B_c^2
 *                   (+ 2^-126 per term): the sample's 11 on S_s and on W_s, a reciprocal and a product (2) per factor, the product of the two
 *                   factors (1), three sums of the four-term chain (3), and 1 for every fp64 sum together (below 2^29 terms);
 *                   tests/ref_volume_match.py derives it.  pairs and own are exact.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: a null pointer (a null scratch too; step may be NULL); a
 * non-positive B, K, R_src, R_dst, X, Y, Z or C; C % 4 != 0; X*Y*Z at or beyond 2^31; a row outside its pool; sum pools that are not 16-byte
 * aligned; a scratch that is not 8-byte aligned; a non-finite xform, origin or voxel_size; voxel_size <= 0; a step below 1.                         */
int64_t ivx_volume_match_scratch_bytes(int32_t B, int32_t K, int32_t X, int32_t Y, int32_t Z, int32_t C);
int ivx_volume_match_fwd(int32_t B, int32_t K, const int32_t *row_src /*host [B]*/, const int32_t *row_dst /*host [B]*/,
                         const float *xform /*host [B,K,3,4]*/, const float *origin_dst /*host [B,3]*/, const float *origin_src /*host [B,3]*/,
                         const float *voxel_size /*host [3]*/, const int32_t *step /*host [3] or NULL*/, int32_t R_src, int32_t R_dst, int32_t X,
                         int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const float *sum_dst, const float *wsum_dst,
                         int64_t *pairs_out, int64_t *own_out, double *stats_out, void *scratch, ivx_stream_t stream);

/* (0.5.8) The Gauss-Newton normal equations of a six-DoF pose between two rows of the state pools: which small rigid motion makes two fused scenes
 * agree better?  ivx_volume_match_fwd judges a candidate; this entry also says where to go from it (scene.py, SceneSession.refine,
 * SceneBatch.refine, register(refine=True)).  The mean field b(x) = S_s(x) / W_s(x) is read trilinearly, so its spatial gradient comes from the
 * eight corners the match already loads, and one launch returns the cost e = sum r^2 of the residual r = b - a, its half gradient g = sum J r
 * and the Gauss-Newton matrix H = sum J J^T over all six degrees of freedom.  The kernel is the match kernel's ALIGN instantiation
 * (csrc/volume_match.hip); a read-only reduction pinned to an fp64 reference written from the definition below (tests/ref_volume_align.py).
 *
 * Definition.  Samples, rows, origins, candidates M = xform[b,k] (x_src = R x_dst + t), the lattice step and the visiting order are
 * ivx_volume_match_fwd's; about[b] is the point the rotation increments go through.  The increment xi = (v, w) -- a translation v, then a
 * rotation vector w about `about`, both in the DESTINATION frame -- moves a destination point p to  p + v + w x (p - about)  to first order, and
 * the candidate after it is  M o increment.  For every visited voxel n and every candidate, in fp32, round-to-nearest, no contraction:
 *   1. own, sample, paired   exactly steps 1 - 4 of ivx_volume_match_fwd.  pairs, own, dot, na and nb are the match's, over the PAIRED voxels,
 *               bit for bit what ivx_volume_match_fwd returns for the same inputs: the sample folds the corners the match folds (inside the
 *               grid, weight != 0), and the tile walk and the order of the fp64 sums are the match's.
 *   2. used     a paired voxel is USED iff all eight corners i0 + (dx, dy, dz) lie inside the source grid and wsum_src > 0 at every one of them
 *               (a NaN is not), the corners of weight exactly 0 included: the wsum words of all corners inside the grid are read here, although
 *               the match does not read those of weight 0.  used_out counts the used voxels.  Only used voxels contribute to e, g and H, by
 *               selection, never by a product with zero: the source sums of a corner with W <= 0 cannot reach e, g, H.  At a used voxel all
 *               eight corner words of sum_src are read.
 *   3. gradient With V[c'] the eight corner values of one quantity (c' = dx * 4 + dy * 2 + dz), f the three fractions, w_a0 = 1 - f_a (one
 *               rounded difference) and w_a1 = f_a, the corner derivative along axis A with (p, q) the other two axes in x, y, z order is
 *                   D_A V = fma(w_p1 * w_q1, V[1,1,+] - V[1,1,0], fma(w_p1 * w_q0, .., fma(w_p0 * w_q1, .., fma(w_p0 * w_q0, V[0,0,+] - V[0,0,0], +0))))
 *               -- one rounded product per pair weight, one rounded difference (the corner at +1 along A minus the corner at 0) per pair, the
 *               chain from +0 with q fastest.  dD_A = D_A wsum_src, and per channel dN_A = D_A sum_src[.., c].  With b_c and r_s of step 4 of
 *               the match:
 *                   grad_c[A] = (((dN_A - b_c * dD_A) * r_s) / voxel_size[A])        a product, a difference, a product, an IEEE division
 *                   u_c[j]    = fma(R[2][j], grad_c[2], fma(R[1][j], grad_c[1], R[0][j] * grad_c[0]))          (u_c = R^T grad_c, R = M[:, :3])
 *                   d         = p - about[b], one rounded difference per axis, p the voxel centre of step 1
 *                   J_c       = (u_c[0], u_c[1], u_c[2],  d[1] u_c[2] - d[2] u_c[1],  d[2] u_c[0] - d[0] u_c[2],  d[0] u_c[1] - d[1] u_c[0])
 *               -- two rounded products and one rounded difference per component of d x u_c: three translations, then three rotations.
 *   4. terms    r_c = b_c - a_c, one rounded difference.  Per word of four channels and per sum, four rounded products and three rounded sums
 *               in channel order, as for dot:  e_w = ((r_0 r_0 + r_1 r_1) + r_2 r_2) + r_3 r_3;  g_w[i] the same with J_c[i] r_c (6 sums);
 *               H_w[i][j], i <= j, the same with J_c[i] J_c[j] (21 sums).  Each of the 28 is widened to fp64 at once; everything after is fp64,
 *               in the order of step 5 of the match: a function of (X, Y, Z, C, step) alone, no float atomics, no spinning, partials in the
 *               scratch slab, a second launch that adds them in a fixed order.
 *   5. outputs  pairs_out [B,K], used_out [B,K], own_out [B] int64, exact;  stats_out [B,K,31] fp64 = (dot, na, nb, e, g[0..5], H upper
 *               triangle row-major: H00 H01 .. H05 H11 .. H55).
 * The host forms the step: cost = e / (used * C); (H + damping * diag H) delta = -g; the trial pose is M o increment(delta) (scene.py).
 *
 * Arguments: ivx_volume_match_fwd's, and
 * about        HOST [B,3] fp32, finite
 * used_out     DEVICE [B,K] int64, written;  stats_out is [B,K,31]
 * scratch      DEVICE, ivx_volume_align_scratch_bytes(B, K, X, Y, Z, C) bytes (-1 as for the match's), 8-byte aligned
 * A sums lane keeps 31 fp64 accumulators (the direct arrangement); launches as for the match.
 *
 * Properties.
 *   Read only, Deterministic   as for ivx_volume_match_fwd.
 *   Match parity.   pairs, own, dot, na, nb == ivx_volume_match_fwd's, bit for bit.
 *   Zero weights.   A NaN in sum_src wherever wsum_src == 0 leaves e, g, H unchanged bit for bit (such a corner makes its voxel unused).
 *   Identity.       M = I, equal origins, a grid where the chain is exact, source and destination the same state: b_c == a_c bit for bit at every
 *                   paired voxel, so r_c == +0 and e == 0, g == 0 exactly.
 *   Error.          Against the exact value on the same i0, f and d, to first order, with u = 2^-24, A_c and B_c of the match,
 *                   Rm_c = A_c + B_c,  MN = sum_pairs |w_p w_q| (|V[+]| + |V[0]|) over sum_src,  MD the same over wsum_src,
 *                   Gm_c[A] = (MN + B_c MD) / (W_s voxel_size[A]),  Um_c[j] = sum_i |R[i][j]| Gm_c[i],
 *                   Jm_c = (Um_c, |d[1]| Um_c[2] + |d[2]| Um_c[1], ..):
 *                     r_c  25 u Rm_c: b's 24, a's 2 <= 25 (A + B) with the difference's 1
 *                     dN, dD  8 u: two axis weights (2), their product (1), the corner difference (1), the chain of four (4)
 *                     grad  48 u Gm: b dD 24 + 8 + 1 = 33, the difference + 1 = 34, r_s 12 and the product 1 = 47, the division 1
 *                     u  51 u Um (a product and two fma: 3);   d x u  53 u (a product 1, the difference 1)
 *                     |e - exact| <= 55 u sum Rm^2  (25 + 25 + 1, the chain 3, every fp64 sum together 1)
 *                     |g[i] - exact| <= (81 | 83) u sum Jm[i] Rm   (translation | rotation: K_J + 25 + 1 + 3 + 1)
 *                     |H[i][j] - exact| <= (107 | 109 | 111) u sum Jm[i] Jm[j]   (both translations | one of each | both rotations)
 *                   (+ 2^-126 per term); dot, na, nb as for the match.  tests/ref_volume_align.py derives it.  The counts are exact.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: the errors of ivx_volume_match_fwd (used_out and about are
 * required too), and an about that is not finite.                                                                                                */
int64_t ivx_volume_align_scratch_bytes(int32_t B, int32_t K, int32_t X, int32_t Y, int32_t Z, int32_t C);
int ivx_volume_align_fwd(int32_t B, int32_t K, const int32_t *row_src /*host [B]*/, const int32_t *row_dst /*host [B]*/,
                         const float *xform /*host [B,K,3,4]*/, const float *about /*host [B,3]*/, const float *origin_dst /*host [B,3]*/,
                         const float *origin_src /*host [B,3]*/, const float *voxel_size /*host [3]*/, const int32_t *step /*host [3] or NULL*/,
                         int32_t R_src, int32_t R_dst, int32_t X, int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src,
                         const float *sum_dst, const float *wsum_dst, int64_t *pairs_out, int64_t *used_out, int64_t *own_out, double *stats_out,
                         void *scratch, ivx_stream_t stream);

/* (0.5.6) Ordered compaction of the seen voxels of rows of the state pools, and its inverse: a scene's fused state leaves the process it was fused in
 * (scene snapshots: scene.py, SceneSession.snapshot / ImVoxelNet.restore_scene / SceneBatch.snapshot / SceneBatch.restore).  A single frustum, a
 * scrolled grid or a faded scene leaves much of a row unseen, all bits zero; the pack moves only the voxels that hold evidence, in ascending voxel
 * order, and the unpack writes a whole row from such a list.  Like ivx_volume_scroll_fwd the F32 form is a pure move of bits, pinned with == to a
 * numpy restatement (tests/ref_volume_pack.py), and both entries lie outside the reference-parity claims.
 *
 * Definition.  Voxel n = (i*Y + j)*Z + k of a row is KEPT iff its count word or its wsum word is non-zero, compared as raw 32-bit words: a -0 or
 * NaN weight sum is kept and no float rule enters.  A voxel that is not kept is an unseen voxel.
 *   pack    For sample b with r = row[b]: n_out[b] = the number of kept voxels of row r -- the true number, also when it exceeds cap.  For
 *           q < min(n_out[b], cap), record q is the q-th kept voxel in ascending n:  index_out[b,q] = n,  count_out[b,q] and wsum_out[b,q] its two
 *           words,  payload_out[b,q,:] its payload.  Nothing at or beyond [b, min(n_out[b], cap)) of any output is touched.
 *   unpack  For sample b with r = row[b] and its n[b] records: voxel index[b,q] of row r takes record q; every other voxel of row r becomes unseen,
 *           sums +0, count 0, weight sum +0.  Every voxel of a named row is written once.
 *   payload IVX_F32:  the C sums as raw 16-byte words; every bit pattern survives (NaN payloads, -0, denormals).
 *           IVX_BF16: the mean.  den = the weight sum, or (float)count without a wsum pool;  m = den > 0 ? S / den : +0, one IEEE division, rounded
 *           once to bf16, round to nearest even.  Unpack restores S = float(m) * den, one rounded product, with den from the record (wsum_rec, or
 *           (float)count_rec).  For |S / den| in bf16's normal range:  |S' - S| <= (2^-8 + 2^-22) |S|  (tests/ref_volume_pack.py derives it).
 *
 * ivx_volume_pack_fwd
 * B            samples of this call
 * row          HOST [B] int32: sample b reads row row[b] of the pools; distinct
 * R, X, Y, Z, C  the pools have R rows of X*Y*Z voxels; C % 4 == 0
 * volume_sum   DEVICE [R,X,Y,Z,C] fp32, 16-byte aligned, read only;  count  DEVICE [R,X,Y,Z] int32;  wsum  DEVICE [R,X,Y,Z] fp32 or NULL
 * payload_dtype  IVX_F32 | IVX_BF16
 * cap          records per sample the outputs have room for, >= 0.  cap == 0 is the count-only form: only n_out is written, by the counting
 *              launches alone, and the four outputs may be NULL.
 * index_out    DEVICE [B,cap] int32;  payload_out  DEVICE [B,cap,C] fp32 (16-byte aligned) or bf16 (8-byte aligned);  wsum_out  DEVICE [B,cap] fp32,
 *              given iff wsum is;  count_out  DEVICE [B,cap] int32
 * n_out        DEVICE [B] int32
 * scratch      DEVICE, ivx_volume_pack_scratch_bytes(B, X, Y, Z) bytes (-1 for non-positive arguments or X*Y*Z at or beyond 2^31)
 * ivx_volume_unpack_fwd
 * row, n       HOST [B] int32: sample b writes row row[b] (distinct) from its first n[b] records, 0 <= n[b] <= cap
 * cap          the record lists have cap entries per sample; with cap == 0 every n[b] is 0, the lists may be NULL and the named rows become unseen
 * index, payload, wsum_rec, count_rec   DEVICE, as the pack wrote them: [B,cap] int32 strictly ascending in [0, X*Y*Z), [B,cap,C], [B,cap] fp32 given
 *              iff the wsum pool is, [B,cap] int32
 * volume_sum, count, wsum   the pools as above, written
 * row (and n) are host lists, as for ivx_volume_scroll_fwd: everything is checked before any launch and nothing is uploaded (32 samples per launch).
 *
 * Properties.
 *   Order.         Deterministic: three launches per 32 samples (count per chunk of 256 voxels, an exclusive scan of the chunk counts by one
 *                  workgroup per sample, write) with no atomics, no spinning and no dependence between the workgroups of a launch; the unpack is
 *                  one launch.  csrc/volume_pack.hip has the schedule.
 *   Untouched.     The source pools of a pack are read only; rows that no sample names are neither read (pack) nor read or written (unpack).
 *   Round trip.    F32: unpack(pack(row)) equals the row bit for bit IF every unseen voxel of the row has all-zero sums.  That is the state's own
 *                  invariant: a `first` lift, the forgetting rule, scroll, warp and merge all store +0 sums wherever they leave count and weight sum
 *                  zero, and nothing else writes a state (tests/test_gpu_scene_snapshot.py checks it on a state that went through all of them).
 *                  Sums at unseen voxels that are not zero are dropped.
 *   Checked data.  No address of the unpack depends on unchecked data: the index list is searched at positions inside [0, n[b]) and an index that
 *                  does not fall into the chunk of voxels being written -- so any index outside [0, X*Y*Z) -- is skipped.  A list that is not strictly
 *                  ascending loses records but writes nothing out of place; ops.volume_unpack_ refuses it on the host.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names the entry: a null required pointer (pack: a null scratch too); a non-positive B,
 * R, X, Y, Z or C; C % 4 != 0; sums or payload not 16-byte aligned (the bf16 payload: 8-byte); X*Y*Z at or beyond 2^31; a negative cap; cap > 0
 * with a null output or record list; n[b] outside [0, cap]; a row outside [0, R); two samples on one row; an unknown payload_dtype; wsum / wsum_out
 * (pack) or wsum / wsum_rec (unpack) given on one side only.                                                                                     */
int64_t ivx_volume_pack_scratch_bytes(int32_t B, int32_t X, int32_t Y, int32_t Z);
int ivx_volume_pack_fwd(int32_t B, const int32_t *row /*host [B]*/, int32_t R, int32_t X, int32_t Y, int32_t Z, int32_t C, const float *volume_sum,
                        const int32_t *count, const float *wsum /*or NULL*/, int32_t payload_dtype, int32_t cap, int32_t *index_out, void *payload_out,
                        float *wsum_out /*or NULL*/, int32_t *count_out, int32_t *n_out, void *scratch, ivx_stream_t stream);
int ivx_volume_unpack_fwd(int32_t B, const int32_t *row /*host [B]*/, const int32_t *n /*host [B]*/, int32_t cap, const int32_t *index, const void *payload,
                          const float *wsum_rec /*or NULL*/, const int32_t *count_rec, int32_t payload_dtype, int32_t R, int32_t X, int32_t Y, int32_t Z,
                          int32_t C, float *volume_sum, int32_t *count, float *wsum /*or NULL*/, ivx_stream_t stream);

/* (0.5.1) View coverage: what would a candidate view add to a scene?  Every frame that reaches a streaming scene pays for the 2-D trunk, and
 * most frames of a 30 Hz camera look at voxels the scene has already fused.  Whether a pose adds anything depends only on the geometry and on
 * the scene's state, not on the image, so it is counted here, in integers, by one small launch BEFORE the trunk runs (a keyframe gate:
 * scene.py, SceneSession.coverage / add_views(..., min_novelty=)).  The decision "view v sees voxel n" is the lift's own, bit for bit, depth
 * gate and confidence map included, so the gate cannot disagree with the lift at the frustum's edges.  Like the bilinear rule, fading,
 * scrolling and pixel maps it lies outside the reference-parity claims; it is pinned with == to a numpy restatement of the definition below
 * (tests/ref_view_coverage.py) and to the lift's own mask.
 *
 * Definition.  For sample b (a scene): its state row r = row[b] (NULL: b), its grid new_origin[b], crop_hw[b], d->X, d->Y, d->Z, d->voxel_size,
 * and candidate view v with slot = view_slot[b*V + v] into proj_pool [S,3,4].  Over all voxels n = (i*Y + j)*Z + k of the grid:
 *   sees(b,v,n)   step 3 of ivx_backproject_mapped_fwd with view weight 1, decided exactly as that step decides it:
 *                 the point  float(idx) * voxel_size + new_origin  (an fp32 product, an fp32 sum), the projection chain  P0 * x, fma(P1, y, .),
 *                 fma(P2, z, .), fma(P3, 1, .)  per row, (xr, yr) = (rint(u / d), rint(v / d)) of the two IEEE quotients, and
 *                 0 <= xr < min(crop_w, FW) && 0 <= yr < min(crop_h, FH) && d > 0, tested on the rounded floats.
 *                 depth != NULL: with D = depth[slot, yr, xr], if D > 0 && D < inf (a measurement) also  d <= D + behind && d >= D - front,
 *                 the sum and the difference each rounded once; any other D gates nothing.
 *                 pixel_weight != NULL: w = pixel_weight[slot, yr, xr] must pass  w > 0 && w < inf  (1 * w is w: the lift's rounded product).
 *                 A slot outside [0, S) sees nothing (-1 pads ragged rows, anywhere in a row).  The map addresses are formed from slot and
 *                 pixel only after the validity test has passed, and no address depends on a map's value.
 *   den(b,n)      the evidence the scene already holds at the voxel, by state_kind:
 *                 IVX_STATE_NONE   state == NULL, an empty scene: den = 0
 *                 IVX_STATE_COUNT  state int32 [R,X,Y,Z], the view counts of a (sum, count) scene: den = (float)count
 *                 IVX_STATE_WSUM   state fp32  [R,X,Y,Z], the weight sums of a fading scene:      den = wsum
 *                 IVX_STATE_MASK   state uint8 [R,X,Y,Z], the valid mask of a windowed scene:     den = valid ? 1 : 0
 *   fresh(b,n)    !(den >= fresh_below) -- the form of the forgetting rule: a NaN evidence is fresh, equality is not.
 *   out [B,V,2] int32:  out[b,v,0] = #{n : sees},  out[b,v,1] = #{n : sees && fresh}.  A padded slot gives (0, 0).
 * The entry zeroes out on the stream itself (hipMemsetAsync), so a reused buffer does not accumulate.  The kernel adds with integer atomics
 * only: the result does not depend on the order of arrival.
 *
 * d           the descriptor of ivx_backproject_fwd_ex: B, V (the length of a row of view_slot), FH, FW (the size of the maps and the clamp of
 *             the crop), X, Y, Z and voxel_size are read; C, feat_dtype, mode, sampling and first are IGNORED (there are no features here)
 * l           S (slots of proj_pool and of the maps), R (rows of state), view_slot DEVICE [B,V], row DEVICE [B] or NULL (= b; then R >= B);
 *             l->first must be NULL.  A row outside [0, R) makes sample b count nothing (tested per workgroup before any address is formed).
 *             Rows need not be distinct: nothing is written to the state.
 * m           the maps of ivx_backproject_mapped_fwd, [S,FH,FW] fp32 each, and the gate; NULL, or both pointers NULL: no maps
 * proj_pool   DEVICE [S,3,4] fp32; new_origin DEVICE [B,3] fp32; crop_hw DEVICE [B,2] int32: per SAMPLE, as for the listed lifts
 * state, state_kind   as above; the pointer and the kind must agree
 * fresh_below finite and > 0 (1: "less than one full-weight view's worth of evidence")
 * out         DEVICE [B,V,2] int32
 *
 * Properties that follow from the definition.
 *   Same as the lift.  out[b,v,0] equals the number of set bytes of `valid` of ivx_backproject_mapped_fwd (mean mode) over the single view v with
 *                 unit weight and the same maps, on the same grid.
 *   Bounds.       0 <= fresh <= seen <= X*Y*Z; with IVX_STATE_NONE fresh == seen; fresh is monotone in fresh_below.
 *   Read only.    Nothing but out is written.
 * IVX_ERR_INVALID_ARG before any launch, with a message that names this entry: a null d, l, proj_pool, l->view_slot, new_origin, crop_hw or out;
 * non-positive B, V, S, R, FH, FW, X, Y or Z; X*Y*Z, S*FH*FW or B*V at or beyond 2^31; B > 65535; V > 256; R < B with no row list; an unknown
 * state_kind; a state pointer that contradicts it (NULL with a kind other than IVX_STATE_NONE, non-NULL with IVX_STATE_NONE); a fresh_below that
 * is not finite or not > 0; l->first != NULL; depth != NULL with a behind or front that is negative or NaN.                                  */
#define IVX_STATE_NONE 0
#define IVX_STATE_COUNT 1
#define IVX_STATE_WSUM 2
#define IVX_STATE_MASK 3
int ivx_view_coverage_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_maps *m /*or NULL*/, const float *proj_pool,
                          const float *new_origin /*[B,3]*/, const int32_t *crop_hw /*[B,2]*/, const void *state /*or NULL*/, int32_t state_kind,
                          float fresh_below, int32_t *out /*[B,V,2]*/, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Anchor3DHead tail -- replaces Anchor3DHead.get_bboxes_single
 * (mmdet3d/models/dense_heads/anchor3d_head.py:428-517) for a batch, single feature level,
 * sigmoid classification: permute to HWC, sigmoid, direction argmax, top-k(nms_pre),
 * DeltaXYZWLHRBBoxCoder.decode (coders/delta_xyzwhlr_bbox_coder.py:56-90), BEV boxes
 * (lidar_box3d.py:86-90 + structures/utils.py:64-82), box3d_multiclass_nms
 * (post_processing/box3d_nms.py:8-88) with rotated (iou3d_kernel.cu:284-333) or axis-aligned
 * (:345-396) NMS and the greedy scan of iou3d.cpp:127-143 done on the device, top max_num,
 * yaw fix-up with limit_period (anchor3d_head.py:510-515).
 *
 * head_out   [B, H, W, CH]  NHWC output of the fused 1x1 head conv; channel blocks
 *                           [cls: A*ncls | reg: A*7 | dir: A*2] starting at cls_off/reg_off/dir_off
 * anchors    [H*W*A, 7]     Anchor3DRangeGenerator.grid_anchors output (flat order y, x, size, rot)
 * workspace  ivx_anchor_head_workspace_bytes() bytes, 256-byte aligned
 * out_boxes  [B, max_num, 7], out_scores [B, max_num], out_labels [B, max_num] int64,
 * out_count  [B] int32.  Rows >= count are zero.
 * Optional debug outputs (NULL to skip): cand_idx [B,nms_pre] int64 top-k anchor indices in
 * descending-score order (-1 padded), cand_boxes [B,nms_pre,7], cand_scores [B,nms_pre].     */
typedef struct ivx_anchor_head_desc {
  int32_t B, H, W, CH;
  int32_t num_anchors; /* A: base anchors per location (sizes * rotations) */
  int32_t num_classes;
  int32_t cls_off, reg_off, dir_off;
  int32_t nms_pre, max_num;
  int32_t use_rotate_nms;
  int32_t hw_transposed; /* 1: head_out is stored [B, W, H, CH] (x-major), as the Kitti/NuScenes neck
                            leaves it before its .transpose(-1, -2) (necks/imvoxelnet.py:120) */
  float score_thr, nms_thr;
  float dir_offset, dir_limit_offset;
} ivx_anchor_head_desc;

int64_t ivx_anchor_head_workspace_bytes(const ivx_anchor_head_desc *d);
int ivx_anchor_head_get_bboxes(const ivx_anchor_head_desc *d, const float *head_out, const float *anchors,
                               void *workspace, int64_t workspace_bytes, float *out_boxes,
                               float *out_scores, int64_t *out_labels, int32_t *out_count,
                               int64_t *cand_idx, float *cand_boxes, float *cand_scores,
                               ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Indoor (anchor-free) head tail, one feature level -- replaces the per-level body of
 * ImVoxelHeadV2._get_bboxes_single (mmdet3d/models/dense_heads/imvoxel_head_v2.py:245-277 with :224-226, :206-214,
 * ScanNet decode :547-555 / SUN RGB-D decode :419-438 and the exp(Scale(.)) of forward_single :305-313, :444-449):
 * valid mask resized to the level (trilinear + round == ">= 5 of the 8 contributing level-0 voxels"), scores =
 * sigmoid(cls) * sigmoid(centerness) * valid, top-k(nms_pre) by class maximum, level points, distance decoding.
 *
 * head_out [B, nx, ny, nz, CH]  fused 3x3x3 head conv: channel 0 centerness, 1..n_reg raw regression, then classes
 * valid0   [B, X, Y, Z] u8      level-0 mask from ivx_backproject_mean_fwd; (nx,ny,nz) * 2^level == (X,Y,Z)
 * level_vs, level_new_origin [B,3]  voxel_size * 2^level and origin - n_level/2 * that (host-built fp32, as get_points)
 * n_reg 6: boxes are corners (x1,y1,z1,x2,y2,z2); n_reg 7: (cx,cy,cz,w,l,h,alpha)
 * cand_boxes [B, k, n_reg], cand_scores [B, k, n_classes], cand_count [B] with k = min(nms_pre, nx*ny*nz) <= 65536 (beyond 4096: rank sort of the candidates, same order),
 * candidates in descending class-maximum score.  The (cross-level) NMS is ivx_aligned_3d_nms / ivx_nms_bev.     */
int64_t ivx_fcos_head_workspace_bytes(int32_t B, int32_t n, int32_t nms_pre);
int ivx_fcos_head_level_candidates(const float *head_out, const uint8_t *valid0, const float *level_vs,
                                   const float *level_new_origin, float scale, int32_t B, int32_t nx, int32_t ny,
                                   int32_t nz, int32_t CH, int32_t n_classes, int32_t n_reg, int32_t level, int32_t X,
                                   int32_t Y, int32_t Z, int32_t nms_pre, void *workspace, int64_t workspace_bytes,
                                   float *cand_boxes, float *cand_scores, int32_t *cand_count, ivx_stream_t stream);

/* Cross-level tail of the anchor-free indoor heads: replaces the torch.cat over levels and `_nms` of
 * ImVoxelHeadV2._get_bboxes_single (mmdet3d/models/dense_heads/imvoxel_head_v2.py:258-277; ScanNet _nms :528-545 = class
 * maximum, score threshold, class-aware aligned_3d_nms, corners -> centre / size; SUN RGB-D _nms :397-417 = BEV boxes +
 * box3d_multiclass_nms with max_num = nms_pre) for a batch, without a host round trip.
 *   cand_boxes[l] [B, k[l], n_reg], cand_scores[l] [B, k[l], n_classes]   outputs of ivx_fcos_head_level_candidates per level
 *   n_reg 6 (ScanNet): nms_thr = test_cfg.iou_thr, max_num >= sum(k) (nothing is cut); n_reg 7 (SUN RGB-D): nms_thr / use_rotate_nms
 *   of test_cfg, max_num = test_cfg.nms_pre.
 *   out_boxes [B, max_num, 7] = the rows of the returned box object's tensor (x, y, z of the BOTTOM face, dx, dy, dz, yaw; yaw 0 for
 *   ScanNet) -- BaseInstance3DBoxes(origin=(.5,.5,.5)) applied (core/bbox/structures/base_box3d.py:63-66); out_scores, out_labels
 *   int64 [B, max_num], out_count [B]; rows >= count are zero. */
typedef struct ivx_indoor_tail_desc {
  int32_t B, n_levels;
  int32_t k[4];              /* candidates per level (min(nms_pre, level voxels)) */
  int32_t n_classes, n_reg;
  int32_t use_rotate_nms, max_num;
  float score_thr, nms_thr;
} ivx_indoor_tail_desc;
int64_t ivx_indoor_tail_workspace_bytes(const ivx_indoor_tail_desc *d);
int ivx_indoor_tail_get_bboxes(const ivx_indoor_tail_desc *d, const float *const *cand_boxes, const float *const *cand_scores,
                               void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_labels,
                               int32_t *out_count, ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * BEV NMS -- device-side replacement of iou3d_cuda.nms_gpu / nms_normal_gpu
 * (mmdet3d/ops/iou3d/src/iou3d.cpp:95-201, iou3d_kernel.cu:284-396).  Same contract as the
 * reference op except that nothing is copied to the host: boxes [n,5] (x1,y1,x2,y2,ry) must
 * already be sorted by descending score (as iou3d_utils.py:39-47 does before the call);
 * keep [n] int64 receives indices into that order, num_out [1] int32 their count.
 * workspace >= ivx_nms_workspace_bytes(n) (the n x ceil(n/64) mask words, as the reference's cudaMalloc at iou3d.cpp:110).
 * Any n up to 65536, like the reference op (col_blocks = DIVUP(N, 64)): up to 4096 boxes the scanning wave keeps one removal
 * word per lane, beyond that the words live in its LDS -- same kept sequence.                  */
int64_t ivx_nms_workspace_bytes(int32_t n);
int ivx_nms_bev(const float *boxes_sorted, int32_t n, float thresh, int32_t rotated, void *workspace,
                int64_t workspace_bytes, int64_t *keep, int32_t *num_out, ivx_stream_t stream);
/* Pairwise rotated BEV overlap area / IoU (boxes_overlap_bev_gpu / boxes_iou_bev_gpu,
 * iou3d.cpp:38-93): a [na,5], b [nb,5] -> out [na,nb]. */
int ivx_boxes_overlap_bev(const float *a, int32_t na, const float *b, int32_t nb, int32_t iou, float *out,
                          ivx_stream_t stream);

/* aligned_3d_nms (mmdet3d/core/post_processing/box3d_nms.py:91-138) on the device.
 * boxes [n,6] corners, scores [n], classes [n] int64; pick [n] int64 receives the kept box
 * indices in descending score order, num_out [1] int32.  One workgroup, no workspace: n <= 4096 (use the _ws form beyond). */
int ivx_aligned_3d_nms(const float *boxes, const float *scores, const int64_t *classes, int32_t n,
                       float thresh, int64_t *pick, int32_t *num_out, ivx_stream_t stream);
/* The same result with a workspace, n <= 65536.  Up to 4096 boxes the greedy chain runs per class on 64 workgroups in
 * parallel (boxes of different classes never suppress each other); inputs with degenerate boxes (non-finite corners, an extent
 * outside (0, 1e6)), where the reference's NaN IoU suppresses ACROSS classes, take the one-workgroup form inside the call.
 * Beyond 4096: rank sort by score, a suppression mask over the sorted boxes with the reference's own predicate
 * NOT(iou * same_class <= thresh), greedy scan with the removal bits in LDS -- same picks, any input. */
int64_t ivx_aligned_3d_nms_workspace_bytes(int32_t n);
int ivx_aligned_3d_nms_ws(const float *boxes, const float *scores, const int64_t *classes, int32_t n, float thresh,
                          void *workspace, int64_t workspace_bytes, int64_t *pick, int32_t *num_out, ivx_stream_t stream);

/* Global average pool of a channels-last map: in [B,S,C] -> out [B,C]; `x.mean(dim=(2,3))` of LayoutHead.forward
 * (mmdet3d/models/dense_heads/layout_head.py:42, SUN RGB-D Total configs).                                        */
int ivx_global_avgpool_fwd(const float *in, int32_t B, int64_t S, int32_t C, float *out, ivx_stream_t stream);
/* The same pool of a bf16 map (0.4.2; LayoutHead on bf16 storage): fp32 out, the summation order of ivx_global_avgpool_fwd, so the result
 * equals ivx_global_avgpool_fwd of the map converted to fp32 bit for bit. */
int ivx_global_avgpool_fwd_bf16(const void *in, int32_t B, int64_t S, int32_t C, float *out, ivx_stream_t stream);

/* Fused multi-class BEV NMS -- replaces box3d_multiclass_nms (mmdet3d/core/post_processing/box3d_nms.py:8-88), i.e.
 * the host loop over classes around nms_gpu / nms_normal_gpu with its per-class D2H, for n <= 65536 candidates and
 * num_classes <= 64 (beyond 4096 candidates: per-class rank sort, one shared hit matrix, removal bits in LDS; same output).  boxes [n,5] (x1,y1,x2,y2,ry); scores [n,score_stride], class c in column c.  Per class the
 * candidates with score > score_thr are sorted by score (descending, ties -> lower index) and greedily suppressed at
 * IoU > nms_thr; the survivors are concatenated class-major, or, when more than max_num survive, cut to the max_num
 * best by score (descending; ties -> lower class).  out_idx (index into the n candidates) and out_label hold
 * min(max_num, n * num_classes) int64 entries; *out_count receives the number written.                            */
int64_t ivx_multiclass_nms_workspace_bytes(int32_t n, int32_t num_classes);
int ivx_multiclass_nms_bev(const float *boxes, const float *scores, int32_t n, int32_t score_stride, int32_t num_classes,
                           float score_thr, float nms_thr, int32_t rotated, int32_t max_num, void *workspace,
                           int64_t workspace_bytes, int64_t *out_idx, int64_t *out_label, int32_t *out_count,
                           ivx_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * KITTI AP evaluation, host side: the per-image matching loops the reference compiles with numba.jit.
 * HOST pointers, row-major double matrices, no device work, no stream -- the rotated BEV / 3-D overlaps that feed
 * them come from ivx_boxes_overlap_bev.  Python driver: imvoxelnet_amd/kitti_ap.py.
 *   ivx_kitti_image_box_overlap   mmdet3d/core/evaluation/kitti_utils/eval.py:83-112 (criterion -1 IoU, 0 / area(box),
 *                                 1 / area(query), other: intersection area)
 *   ivx_kitti_compute_statistics  eval.py:161-279 for one image.  overlaps[j*ld + i] = detection j vs ground truth i;
 *                                 gt rows (x1,y1,x2,y2,alpha), dt rows (x1,y1,x2,y2,alpha,score); ignored_* in
 *                                 {0 counted, 1 ignored, -1 other class}; stats4 = tp, fp, fn, similarity (-1 = none);
 *                                 thresholds (n_gt doubles) receives the scores of the matched detections.
 *   ivx_kitti_collect_scores      eval.py:500-514: the compute_fp = false pass over a list of images (rows of all
 *                                 images concatenated; ov_ptrs[i] = image i's [dt_nums[i], gt_nums[i]] matrix).
 *   ivx_kitti_fused_statistics    eval.py:291-338: pr[t*4 + {tp,fp,fn,similarity}] accumulated over the images for
 *                                 every score threshold t.                                                      */
int ivx_kitti_image_box_overlap(const double *boxes, int32_t n, const double *query, int32_t k, int32_t criterion,
                                double *out);
int ivx_kitti_compute_statistics(const double *overlaps, int32_t ld, const double *gt_datas, int32_t n_gt,
                                 const double *dt_datas, int32_t n_dt, const int64_t *ignored_gt,
                                 const int64_t *ignored_det, const double *dc_bboxes, int32_t n_dc, int32_t metric,
                                 double min_overlap, double thresh, int32_t compute_fp, int32_t compute_aos,
                                 double *stats4, double *thresholds, int32_t *n_thresholds);
int ivx_kitti_collect_scores(const double *const *ov_ptrs, int32_t n_img, const int32_t *gt_nums, const int32_t *dt_nums,
                             const double *gt_datas, const double *dt_datas, const int64_t *ignored_gts,
                             const int64_t *ignored_dets, int32_t metric, double min_overlap, double *scores_out,
                             int64_t *n_out);
int ivx_kitti_fused_statistics(const double *const *ov_ptrs, int32_t n_img, const int32_t *gt_nums, const int32_t *dt_nums,
                               const int32_t *dc_nums, const double *gt_datas, const double *dt_datas,
                               const double *dontcares, const int64_t *ignored_gts, const int64_t *ignored_dets,
                               int32_t metric, double min_overlap, const double *thresholds, int32_t n_thr,
                               int32_t compute_aos, double *pr);

/* ---------------------------------------------------------------------------------------
 * Model handle -- the anchor-head ImVoxelNet forward path as one native object
 * (ImVoxelNet.simple_test, mmdet3d/models/detectors/imvoxelnet.py:45-106, for the KITTI / nuScenes families:
 * ResNet-50 -> FPN level 0 -> unprojection -> KittiImVoxelNeck | NuScenesImVoxelNeck (necks/imvoxelnet.py:94-154) ->
 * Anchor3DHead forward (anchor3d_head.py:122-153) -> get_bboxes (:375-517)).  The layer sequence, weight packing
 * (conv + eval BatchNorm -> scale/shift epilogue, chunk-major K, Winograd-domain filters), Winograd / tile selection and
 * workspace planning live in the library; the caller owns the workspace and all input / output buffers.  The
 * reference's only native precedent is the pybind op at ops/iou3d/src/iou3d.cpp:95-147,203-208 (caller-allocated
 * outputs, int return); this keeps that convention.
 *
 *   ivx_create(&cfg, &m);
 *   for every tensor of the reference state dict: ivx_weights_load(m, key, host_ptr, shape, ndim);
 *       keys as in a released checkpoint: backbone.*, neck.lateral_convs.i.conv.*, neck.fpn_convs.0.conv.*,
 *       neck_3d.model.{0,2,4}.{conv1,bn1,conv2,bn2}.*, neck_3d.model.{1,3,5}.{0,1}.*, bbox_head.conv_{cls,reg,dir_cls}.*
 *       (a leading "module." is dropped; unused keys -- fpn_convs.1..3, num_batches_tracked -- are ignored);
 *       optional pseudo-key "anchors" [H*W*A, 7]: the anchor grid to use instead of the built-in generator
 *   ivx_weights_finalize(m, stream);                       packs and uploads; lists missing keys on error
 *   n = ivx_model_workspace_bytes(m, B, V, H, W);          plans this shape (allocates transformed filters once)
 *   ivx_model_forward(m, img, B, V, H, W, proj, new_origin, crop_hw, ws, n, boxes, scores, labels, count, valid, stream);
 *   ivx_destroy(m);
 * One handle per device and per host thread; calls are asynchronous on `stream`.                                  */
#define IVX_NECK_KITTI 0
#define IVX_NECK_NUSCENES 1
#define IVX_NECK_FAST 2      /* FastIndoorImVoxelNeck (necks/imvoxelnet.py:8-67): the handle ends at the 3 neck levels */
#define IVX_NECK_UNET 3      /* ImVoxelNeck = Atlas EncoderDecoder + conv blocks (necks/imvoxelnet.py:70-91, 297-372) */
#define IVX_HEAD_NONE 0
#define IVX_HEAD_SCANNET 1
#define IVX_HEAD_SUNRGBD 2
typedef struct ivx_model ivx_model;
typedef struct ivx_model_cfg {
  int32_t neck_type;          /* IVX_NECK_KITTI | IVX_NECK_NUSCENES | IVX_NECK_FAST | IVX_NECK_UNET */
  int32_t with_trunk;         /* 1: ResNet-50 + FPN inside the handle (input = image); 0: input = FPN level-0 map */
  int32_t fpn_channels;       /* FPN out_channels = neck_3d in_channels (64 in the reference configs) */
  int32_t neck_out_channels;  /* neck_3d out_channels = head in_channels (256) */
  int32_t n_voxels[3];
  float voxel_size[3];
  int32_t num_classes;
  int32_t n_sizes, n_rotations;        /* anchor generator: sizes x rotations base anchors, one range */
  float anchor_range[6];               /* x0, y0, z0, x1, y1, z1 */
  float anchor_sizes[12];              /* n_sizes x (w, l, h) */
  float anchor_rotations[4];
  int32_t nms_pre, max_num, use_rotate_nms;   /* test_cfg */
  float score_thr, nms_thr;
  float dir_offset, dir_limit_offset;         /* Anchor3DHead(dir_offset, dir_limit_offset) */
  int32_t winograd;           /* 1: F(m x m, 3x3) form for the eligible layers (default of the Python host), 0: direct only */
  int32_t winograd_tile;      /* 0: automatic (6 on planes >= 16384 positions, else 4) | 2 | 4 | 6 */
  /* indoor necks (zero for the outdoor ones; the anchor / test_cfg fields above are ignored for them) */
  int32_t fast_n_blocks[3];        /* FastIndoorImVoxelNeck(n_blocks) */
  int32_t unet_channels[4];        /* ImVoxelNeck(channels); [0] = fpn_channels; [3] = 0: three scales (two output levels) */
  int32_t unet_down_layers[4];     /* ImVoxelNeck(n_blocks, "down"), e.g. 1,2,3,4 */
  int32_t unet_up_layers[3];       /* ImVoxelNeck(n_blocks, "up") in decode order (coarse first), e.g. 3,2,1 */
  /* (0.3.0) the rest of the path inside the handle; all zero = the 0.2.0 behaviour */
  int32_t head_type;               /* IVX_HEAD_NONE: the indoor handle ends at the neck levels | IVX_HEAD_SCANNET (n_reg 6: ScanNetImVoxelHead /
                                      HeadV2, aligned 3-D NMS) | IVX_HEAD_SUNRGBD (n_reg 7: SunRgbdImVoxelHead / HeadV2, multi-class BEV NMS);
                                      n_convs = 0 as in every reference config (dense_heads/imvoxel_head_v2.py, imvoxel_head.py) */
  int32_t head_classes;            /* n_classes */
  int32_t head_nms_pre;            /* test_cfg.nms_pre (candidates per level; also max_num of the SUN RGB-D NMS) */
  int32_t head_use_rotate_nms;     /* SUN RGB-D test_cfg.use_rotate_nms */
  float head_score_thr, head_nms_thr;   /* test_cfg.score_thr; iou_thr (ScanNet) / nms_thr (SUN RGB-D) */
  int32_t dcn_stages[4];           /* ResNet stage_with_dcn: DCNv2 (ModulatedDeformConv2dPack, deform_groups 1) as conv2 of every bottleneck of
                                      the stage (configs/imvoxelnet/imvoxelnet_nuscenes.py:13-14); keys backbone.layerS.B.conv2.conv_offset.* */
  int32_t layout_head;             /* 1: LayoutHead(n_channels 2048, linear_size) on C5 (SUN RGB-D Total configs, dense_heads/layout_head.py);
                                      its predicted angles replace the extrinsics of the metas at test time; keys head_2d.{angle,layout}_mlp.* */
  int32_t layout_linear_size;
  int32_t wino_operands;           /* (0.3.1) ivx_conv_desc.wino_operands of the layers that run in the Winograd form: IVX_F32 (0) = fp32 MFMA,
                                      IVX_F16_PAIR = fp16 (hi, lo) operand pairs where the layer allows it (tile 4 / 6, Cin % 32 == 0); with it the
                                      3x3x3 neck layers the Winograd form does not take (stride 2 in x / y; under 2000 positions) run in the
                                      IVX_BF16_PAIR form above (split pass + three-product kernel; Cin % 32 == 0, Cout >= 64, >= 256 positions) */
  int32_t trunk_operands;          /* (0.4.0) IVX_F32 (0): the 2-D trunk (ResNet-50 + FPN) on fp32 MFMA.  IVX_F16_PAIR: its activations chained as
                                      fp16 (hi, lo) pair tensors on the 16-bit matrix cores (ivx_conv_fwd_pio: three fp16 MFMA products per
                                      multiply-add, fp32 accumulate, device-side power-of-two scales, no conversion passes) wherever a tensor's
                                      consumers are all convolutions with Cin % 32 == 0; the stem, DCNv2 columns, the LayoutHead and what
                                      leaves the trunk (FPN level 0, C5) stay fp32 */
  int32_t storage;                 /* (0.4.0) IVX_F32 (0, the reference's precision and the one every parity claim is made for) or IVX_BF16: the
                                      optional reduced-precision mode inside the handle (BASELINE config 5 names it) -- activations and weights
                                      stored as bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogues, the 7x7 stem as a 4x4 convolution
                                      over 2x2 space-to-depth blocks of the image), head outputs and the detection tails fp32.  The image input and
                                      the detection outputs keep their types; the tensors of the sub-path entry points (ivx_backbone_fpn_fwd's
                                      fpn0, ivx_neck3d_*_fwd's volume / levels, ivx_model_forward_levels' levels) are bf16.  (0.4.2) With DCNv2
                                      stages conv_offset writes fp32 offsets / masks and the columns are bf16 (ivx_dcn_im2col_fwd_bf16);
                                      with a LayoutHead C5 is pooled to fp32 (ivx_global_avgpool_fwd_bf16) and the six MLP linears stay
                                      fp32 layers (fp32 filters, fp32 in and out).  ivx_model_calibrate_fp8 refuses both forms.  The
                                      Winograd and pair forms are fp32-storage forms and are not used */
  int32_t sampling;                /* (0.4.4) IVX_SAMPLE_NEAREST (0, the reference's rule and the one every parity claim is made for) or
                                      IVX_SAMPLE_BILINEAR: the lift step runs ivx_backproject_fwd_ex with the bilinear rule (an optional extra
                                      mode, see there); orthogonal to storage and the operand forms.  Other values: ivx_create refuses */
} ivx_model_cfg;

int ivx_create(const ivx_model_cfg *cfg, ivx_model **out);
int ivx_destroy(ivx_model *m);
int ivx_weights_load(ivx_model *m, const char *key, const float *data_host, const int64_t *shape, int32_t ndim);
int ivx_weights_finalize(ivx_model *m, ivx_stream_t stream);
/* Whole path.  input: image batch [B*V,3,H,W] NCHW fp32 (with_trunk) or FPN level-0 maps [B*V,1,H/4,W/4,Cf] channels-last;
 * H, W = padded image size (multiples of 32).  proj [B,V,3,4], new_origin [B,3], crop_hw [B,2] int32 as for
 * ivx_backproject_mean_fwd (device).  Outputs as ivx_anchor_head_get_bboxes; out_valid [B,X,Y,Z] u8 or NULL. */
int64_t ivx_model_workspace_bytes(ivx_model *m, int32_t B, int32_t V, int32_t H, int32_t W);
int ivx_model_forward(ivx_model *m, const float *input, int32_t B, int32_t V, int32_t H, int32_t W, const float *proj,
                      const float *new_origin, const int32_t *crop_hw, void *workspace, int64_t workspace_bytes,
                      float *out_boxes, float *out_scores, int64_t *out_labels, int32_t *out_count, uint8_t *out_valid,
                      ivx_stream_t stream);
/* Sub-paths on the same handle: backbone(img) + neck(x)[0] (detectors/imvoxelnet.py:48,50) and neck_3d(x) (:79).
 * fpn0 [BV,1,H/4,W/4,Cf]; volume [B,X,Y,Z,Cf] -> out [B,X',Y',1,Cout] (ivx_neck3d_out_dims). */
int64_t ivx_backbone_fpn_workspace_bytes(ivx_model *m, int32_t BV, int32_t H, int32_t W);
int ivx_backbone_fpn_fwd(ivx_model *m, const float *img, int32_t BV, int32_t H, int32_t W, float *fpn0, void *workspace,
                         int64_t workspace_bytes, ivx_stream_t stream);
int64_t ivx_neck3d_workspace_bytes(ivx_model *m, int32_t B);
int ivx_neck3d_out_dims(ivx_model *m, int32_t B, int32_t *X, int32_t *Y, int32_t *C);
int ivx_neck3d_kitti_fwd(ivx_model *m, const float *volume, int32_t B, float *out, void *workspace, int64_t workspace_bytes,
                         ivx_stream_t stream);
int ivx_neck3d_nuscenes_fwd(ivx_model *m, const float *volume, int32_t B, float *out, void *workspace,
                            int64_t workspace_bytes, ivx_stream_t stream);
/* Indoor necks: three output levels (two for a 3-scale ImVoxelNeck: the unused entry is ignored / zero), finest first, channels-last [B, X_l, Y_l, Z_l, Cout] (neck_3d(x) of
 * detectors/imvoxelnet.py:79 for FastIndoorImVoxelNeck / ImVoxelNeck).  dims[l] = {X, Y, Z, C} of level l.
 * State-dict keys: neck_3d.down_layer_{i}.{j}.{conv1,norm1,conv2,norm2,downsample.0,downsample.1}.*,
 * neck_3d.up_block_{1,2}.{0,1,3,4}.*, neck_3d.out_block_{i}.{0,1}.* (fast); neck_3d.model.layers_down.*,
 * neck_3d.model.proj.{k}.{conv,norm}.*, neck_3d.model.layers_up_conv.{k}.weight, neck_3d.model.layers_up_res.{k}.{j}.*,
 * neck_3d.conv_blocks.{l}.{0,1}.* (unet). */
int ivx_neck3d_levels(ivx_model *m, int32_t B, int32_t dims[3][4]);
int ivx_neck3d_fast_fwd(ivx_model *m, const float *volume, int32_t B, float *const out_levels[3], void *workspace,
                        int64_t workspace_bytes, ivx_stream_t stream);
int ivx_neck3d_unet_fwd(ivx_model *m, const float *volume, int32_t B, float *const out_levels[3], void *workspace,
                        int64_t workspace_bytes, ivx_stream_t stream);
/* Whole indoor path up to the head: backbone + FPN level 0 + unprojection + neck_3d (extract_feat,
 * detectors/imvoxelnet.py:43-88).  Arguments as ivx_model_forward; workspace from ivx_model_workspace_bytes. */
int ivx_model_forward_levels(ivx_model *m, const float *input, int32_t B, int32_t V, int32_t H, int32_t W, const float *proj,
                             const float *new_origin, const int32_t *crop_hw, void *workspace, int64_t workspace_bytes,
                             float *const out_levels[3], uint8_t *out_valid, ivx_stream_t stream);
/* simple_test as ONE call for every family (detectors/imvoxelnet.py:93-106): image batch [B*V,3,H,W] (with_trunk = 0: the FPN level-0
 * maps [B*V,1,H/4,W/4,Cf] channels-last) -> detections, the per-sample camera
 * set-up of :114-129 / :139 / :67-68 included (computed on the host in the library's fixed fp32 order and uploaded into the
 * workspace).  One ivx_sample_meta per sample = the fields of img_meta the path reads.
 *   anchor families (KITTI / nuScenes, DCNv2 stages included): outputs as ivx_model_forward, max_num rows per sample
 *   indoor families with head_type != 0: out_boxes [B, M, 7] rows of the returned box object's tensor (x, y, z of the bottom face,
 *     dx, dy, dz, yaw), M = ivx_model_max_detections(...): ScanNet the total number of candidates (nothing is cut), SUN RGB-D nms_pre
 *   LayoutHead (layout_head = 1, V = 1): the predicted (pitch, roll) replace metas[b].extrinsics (may be NULL); out_angles host [B,2],
 *     out_layout host [B,7] (centre, exp(size), yaw) or NULL -- the forward synchronises the stream once to read them, as the
 *     reference does.
 * Asynchronous on `stream` otherwise; `metas` and what it points to are consumed before the call returns. */
typedef struct ivx_sample_meta {
  float intrinsic[16];         /* img_meta['lidar2img']['intrinsic'], 4x4 row-major (rows 0..2 x cols 0..2 are used) */
  const float *extrinsics;     /* host [V,4,4] row-major: img_meta['lidar2img']['extrinsic'] */
  float origin[3];             /* img_meta['lidar2img']['origin'] */
  int32_t img_h, img_w;        /* img_meta['img_shape'][:2] (before padding to H x W) */
  int32_t ori_h;               /* img_meta['ori_shape'][0] */
} ivx_sample_meta;
int64_t ivx_model_detect_workspace_bytes(ivx_model *m, int32_t B, int32_t V, int32_t H, int32_t W);
int32_t ivx_model_max_detections(ivx_model *m, int32_t B, int32_t V, int32_t H, int32_t W);
int ivx_model_detect(ivx_model *m, const float *img, int32_t B, int32_t V, int32_t H, int32_t W, const ivx_sample_meta *metas /*host [B]*/,
                     void *workspace, int64_t workspace_bytes, float *out_boxes, float *out_scores, int64_t *out_labels, int32_t *out_count,
                     uint8_t *out_valid, float *out_angles /*host*/, float *out_layout /*host*/, ivx_stream_t stream);
/* BASELINE config 5's named mode inside the handle: "bf16 with fp8 2-D conv MFMA".  On a handle with storage = IVX_BF16 and the trunk
 * (no DCNv2 stages and no LayoutHead: IVX_ERR_UNSUPPORTED): runs ONE bf16 pass of ResNet-50 + FPN over the given images (img [BV,3,H,W] fp32; synchronises the stream once),
 * records max |output| of conv1 and conv2 of every bottleneck, and from then on stores the INSIDE of every bottleneck as OCP e4m3:
 * conv1 reads the bf16 residual stream and writes e4m3 (per-tensor scale amax * margin / 448), conv2 and conv3 run on
 * v_mfma_f32_32x32x16_fp8_fp8 (e4m3 activations, e4m3 filters with one scale per output channel), conv3 adds the bf16 shortcut and writes
 * bf16 -- the residual stream itself is never re-quantised (ImVoxelNet.calibrate_fp8(residual='bf16') of the Python host; both hosts
 * run the same kernels).  Plans are rebuilt on the next forward.  workspace as for ivx_backbone_fpn_fwd.  ivx_amax_bf16: the max |x|
 * reduction it uses (out: device float, zeroed by the caller; left as it is for n = 0).  The maximum is over the elements that are not
 * NaN, and an Inf counts: the e4m3 scale amax * margin / 448 has to be a finite number that holds the finite values of the tensor, which a
 * NaN counted as Inf would destroy for every element. */
int ivx_model_calibrate_fp8(ivx_model *m, const float *img, int32_t BV, int32_t H, int32_t W, float margin, void *workspace,
                            int64_t workspace_bytes, ivx_stream_t stream);
/* The same with the variant chosen: ResNet stages below first_stage (0 .. 4) keep plain bf16 bottlenecks; conv2_bf16 != 0: conv1 / conv2 stay bf16
 * convolutions, conv2 writes e4m3 and only conv3 (e4m3 input and filters) runs on the fp8 matrix cores.  (2, 1): FPN level 0 within ~2.2 % rms of the fp32
 * oracle (BASELINE config 5 "bf16 with fp8 2D-conv MFMA" at a usable accuracy); (0, 0) = ivx_model_calibrate_fp8 (3.6 %). */
int ivx_model_calibrate_fp8_ex(ivx_model *m, const float *img, int32_t BV, int32_t H, int32_t W, float margin, int32_t first_stage, int32_t conv2_bf16,
                               void *workspace, int64_t workspace_bytes, ivx_stream_t stream);
int ivx_amax_bf16(const void *x, int64_t n, float *out, ivx_stream_t stream);

/* Host-only LayoutHead arithmetic in a fixed fp32 order (both hosts of the library use it): angle = limit_period(raw) and layout =
 * (centre, exp(size), yaw) (layout_head.py:52-74); the camera extrinsic of detectors/imvoxelnet.py:164-187 from (pitch, roll). */
int ivx_layout_head_decode(const float *angle_raw /*[2]*/, const float *layout_raw /*[7]*/, float *angle /*[2]*/, float *layout /*[7] or NULL*/);
int ivx_layout_extrinsics(const float *angles /*[2]*/, float *extrinsic4x4);

/* Optional stage timing (measurement only): while enabled, every launch group of the forward calls is bracketed by a pair
 * of HIP events on the caller's stream; the Winograd layers run as their three stages so each is timed.  stage: 0 direct
 * conv, 1 Winograd input transform, 2 grouped GEMM, 3 output transform, 4 unprojection, 5 anchor tail.  flops = FLOPs the
 * launch executes, bytes = algorithmic bytes of a transform / unprojection launch.  Read after synchronising the stream. */
typedef struct ivx_trace_rec {
  int32_t step, stage, is3d;
  float ms;        /* duration of the launch group */
  float start_ms;  /* its start, relative to the first record since tracing was enabled */
  double flops, bytes;
  char name[48];
} ivx_trace_rec;
int ivx_model_trace(ivx_model *m, int32_t level);   /* 0 off | 2 every launch group | 1 coarse: the 3-D neck stages, the
                                                       unprojection and the tail individually, the 2-D trunk as one span (stage 6) |
                                                       3 only the grouped Winograd-domain GEMM launches (stage 2): nine event pairs per KITTI step */
int32_t ivx_model_trace_count(ivx_model *m);
int ivx_model_trace_read(ivx_model *m, int32_t i, ivx_trace_rec *rec);

/* Host-only helpers (no device work, usable without a GPU): the built-in anchor grid for an (H, W) map
 * (Anchor3DRangeGenerator, anchor_3d_generator.py:82-209), and the per-sample camera set-up of
 * detectors/imvoxelnet.py:114-129 / :139 in a fixed fp32 operation order: proj[v] = (K[:3,:3] with rows 0,1 / ratio) @ E_v[:3]
 * as an FMA chain over k; new_origin = origin - n_voxels / 2 * voxel_size. */
int ivx_model_anchors(ivx_model *m, int32_t H, int32_t W, float *anchors_host, int64_t capacity);
int ivx_compute_projection(const float *intrinsic4x4, const float *extrinsics /* [V,4,4] */, int32_t V, double ratio,
                           float *proj /* [V,3,4] */);
int ivx_voxel_new_origin(const float *origin, const int32_t *n_voxels, const float *voxel_size, float *new_origin);
/* Host-only: eval BatchNorm + conv bias as the conv epilogue's affine (all host pointers, n channels; bias may be NULL):
 * scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) * scale, IEEE fp32 in this order. */
int ivx_fold_batchnorm(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias, float eps,
                       int32_t n, float *scale, float *shift);


/* ---------------------------------------------------------------------------------------
 * The export names of SURVEY.md section 8(b)'s minimum set that this header spells differently -- the same entry points under the survey's
 * names (csrc/api_common.cpp forwards; INTEGRATION.md B has the table):
 *   ivx_anchor_head_decode  = ivx_anchor_head_get_bboxes       (Anchor3DHead.get_bboxes_single, dense_heads/anchor3d_head.py)
 *   ivx_fcos3d_head_decode  = ivx_fcos_head_level_candidates   (ImVoxelHead / V2 per-level decode, dense_heads/imvoxel_head*.py)
 *   ivx_nms_rotated_bev     = ivx_nms_bev with rotated = 1     (nms_gpu, ops/iou3d/src/iou3d.cpp:95-147)
 *   ivx_nms_aligned3d       = ivx_aligned_3d_nms               (core/post_processing/box3d_nms.py:91-138)                              */
int ivx_anchor_head_decode(const ivx_anchor_head_desc *d, const float *head_out, const float *anchors, void *workspace, int64_t workspace_bytes,
                           float *out_boxes, float *out_scores, int64_t *out_labels, int32_t *out_count, int64_t *cand_idx, float *cand_boxes,
                           float *cand_scores, ivx_stream_t stream);
int ivx_fcos3d_head_decode(const float *head_out, const uint8_t *valid0, const float *level_vs, const float *level_new_origin, float scale, int32_t B,
                           int32_t nx, int32_t ny, int32_t nz, int32_t CH, int32_t n_classes, int32_t n_reg, int32_t level, int32_t X, int32_t Y,
                           int32_t Z, int32_t nms_pre, void *workspace, int64_t workspace_bytes, float *cand_boxes, float *cand_scores,
                           int32_t *cand_count, ivx_stream_t stream);
int ivx_nms_rotated_bev(const float *boxes_sorted, int32_t n, float thresh, void *workspace, int64_t workspace_bytes, int64_t *keep, int32_t *num_out,
                        ivx_stream_t stream);
int ivx_nms_aligned3d(const float *boxes, const float *scores, const int64_t *classes, int32_t n, float thresh, int64_t *pick, int32_t *num_out,
                      ivx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IMVOXEL_H_ */
