// Error reporting + version for libimvoxel_hip.so, and the host-only rules that every host of the kernels shares: the route of a
// convolution (ivx_conv_route) and the filters of its split-operand form (ivx_bf16_pair_pack_filters).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/imvoxel.h"

static thread_local char g_err[512] = "";

void ivx_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int ivx_version(void) { return 580; /* 0.5.8: the Gauss-Newton normal equations of a six-DoF pose between two rows of the scene state pools (the ALIGN instantiation of csrc/volume_match.hip; include/imvoxel.h has the entry and its definition), for aligning scenes; 0.5.7:the read-only scoring of candidate poses between two rows of the scene state pools (csrc/volume_match.hip; include/imvoxel.h has the entry and its definition), for matching scenes; 0.5.6: the ordered compaction of the seen voxels of rows of the scene state pools and its inverse (csrc/volume_pack.hip; include/imvoxel.h has the entries and their definition), for scene snapshots; 0.5.5: the rigid in-place merge of rows of the scene state pools, a second instantiation of the resample kernel (csrc/volume_warp.hip; include/imvoxel.h has the entry and its definition), for scenes that become one; 0.5.4: the rigid out-of-place resample of rows of the scene state pools (csrc/volume_warp.hip; include/imvoxel.h has the entry and its definition), for scenes that turn with their platform; 0.5.3: ivx_image_prep_fmt_u8, ivx_yuv_matrix (csrc/pixel_fetch.h: the image pipeline on decoder pixel formats -- RGB, BGRA / RGBA, gray, NV12, YUYV -- converted in the fetch of the prep launch by a stated integer rule; include/imvoxel.h); 0.5.2: ivx_image_prep_lens_u8, ivx_map_prep_lens (csrc/image_prep.hip: the image pipeline through a Brown / fisheye lens model, one interpolation, and the cover / depth maps of the same geometry at feature resolution; include/imvoxel.h); 0.5.1: the view coverage counts of csrc/view_coverage.hip (the voxels a candidate view would see and those the scene has no evidence for, before its trunk runs; include/imvoxel.h); 0.5.0: pixel maps for the weighted listed lift of csrc/backproject.hip (a per-pixel confidence and a gated depth map per view; include/imvoxel.h); 0.4.9: the in-place voxel shift of rows of the state pools of csrc/volume_scroll.hip (scrolling scenes; include/imvoxel.h); 0.4.8: the weighted listed lift of csrc/backproject.hip (per-view weights, per-sample decay, a forgetting threshold: fading scenes; include/imvoxel.h); 0.4.7: the listed lift with per-sample rows and first flags of csrc/backproject.hip (batches of scenes, ragged batches; include/imvoxel.h); 0.4.6: the gathered mean lift of csrc/backproject.hip (views listed by slot; include/imvoxel.h); 0.4.5: ivx_conv_route, ivx_bf16_pair_pack_filters (the routing rule and the split-operand filter packer as host functions of the library); 0.4.4: ivx_backproject_fwd_ex, ivx_model_cfg.sampling (csrc/backproject.hip: the optional bilinear sampling rule of the unprojection); 0.4.3: ivx_image_prep_u8, ivx_rescale_size (csrc/image_prep.hip: uint8 frames -> normalised, padded fp32 input); 0.4.2: ivx_dcn_im2col_fwd_bf16, ivx_global_avgpool_fwd_bf16 (bf16 storage with DCNv2 stages / the LayoutHead); 0.4.1: ivx_bottleneck_fwd_pio, ivx_stem_pool_fwd_pair, the SURVEY 8(b) export names, include/imvoxel_lab.h; 0.4.0: ivx_pair_io / ivx_conv_fwd_pio (chained fp16-pair activations), ivx_model_cfg.trunk_operands; 0.3.1: ivx_conv_desc.wino_operands, IVX_BF16_PAIR / IVX_F16_PAIR, ivx_model_cfg.wino_operands (0.3.0: head / DCNv2 / LayoutHead fields, ivx_model_detect) */ }
extern "C" const char *ivx_last_error(void) { return g_err; }

// bf16 entry points that model.cpp calls on a bf16 handle with DCNv2 stages / a LayoutHead.  The product library defines them in dcn.hip and
// pool_layout.hip (the strong symbols win at link time); a build of model.cpp without those sources (a host-memory restatement of the op-level
// entry points) links against these and reports the mode as unsupported instead of failing to link.
extern "C" __attribute__((weak)) int ivx_dcn_im2col_fwd_bf16(const void *, const float *, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t,
                                                             int32_t, int32_t, int32_t, void *, ivx_stream_t) {
  ivx_set_error("ivx_dcn_im2col_fwd_bf16: bf16 storage is not available in this build");
  return IVX_ERR_UNSUPPORTED;
}
extern "C" __attribute__((weak)) int ivx_global_avgpool_fwd_bf16(const void *, int32_t, int64_t, int32_t, float *, ivx_stream_t) {
  ivx_set_error("ivx_global_avgpool_fwd_bf16: bf16 storage is not available in this build");
  return IVX_ERR_UNSUPPORTED;
}

// The same device for the unprojection's one-for-all entry point, which model.cpp calls on a handle with cfg.sampling != 0 only: backproject.hip
// defines it; a build without that source has the nearest rule alone (its own restatement of the older entry points) and says so.
extern "C" __attribute__((weak)) int ivx_backproject_fwd_ex(const ivx_backproject_desc *, const void *, const float *, const float *, const int32_t *, void *,
                                                            int32_t *, void *, uint8_t *, ivx_stream_t) {
  ivx_set_error("ivx_backproject_fwd_ex: bilinear sampling is not available in this build");
  return IVX_ERR_UNSUPPORTED;
}

// SURVEY.md section 8(b) names (include/imvoxel.h, last section): the same entry points under the survey's spelling
extern "C" int ivx_anchor_head_decode(const ivx_anchor_head_desc *d, const float *head_out, const float *anchors, void *workspace, int64_t workspace_bytes,
                                      float *out_boxes, float *out_scores, int64_t *out_labels, int32_t *out_count, int64_t *cand_idx, float *cand_boxes,
                                      float *cand_scores, ivx_stream_t stream) {
  return ivx_anchor_head_get_bboxes(d, head_out, anchors, workspace, workspace_bytes, out_boxes, out_scores, out_labels, out_count, cand_idx, cand_boxes,
                                    cand_scores, stream);
}
extern "C" int ivx_fcos3d_head_decode(const float *head_out, const uint8_t *valid0, const float *level_vs, const float *level_new_origin, float scale,
                                      int32_t B, int32_t nx, int32_t ny, int32_t nz, int32_t CH, int32_t n_classes, int32_t n_reg, int32_t level, int32_t X,
                                      int32_t Y, int32_t Z, int32_t nms_pre, void *workspace, int64_t workspace_bytes, float *cand_boxes,
                                      float *cand_scores, int32_t *cand_count, ivx_stream_t stream) {
  return ivx_fcos_head_level_candidates(head_out, valid0, level_vs, level_new_origin, scale, B, nx, ny, nz, CH, n_classes, n_reg, level, X, Y, Z, nms_pre,
                                        workspace, workspace_bytes, cand_boxes, cand_scores, cand_count, stream);
}
extern "C" int ivx_nms_rotated_bev(const float *boxes_sorted, int32_t n, float thresh, void *workspace, int64_t workspace_bytes, int64_t *keep,
                                   int32_t *num_out, ivx_stream_t stream) {
  return ivx_nms_bev(boxes_sorted, n, thresh, 1, workspace, workspace_bytes, keep, num_out, stream);
}
extern "C" int ivx_nms_aligned3d(const float *boxes, const float *scores, const int64_t *classes, int32_t n, float thresh, int64_t *pick,
                                 int32_t *num_out, ivx_stream_t stream) {
  return ivx_aligned_3d_nms(boxes, scores, classes, n, thresh, pick, num_out, stream);
}

// ---------------------------------------------------------------------------------------------- the route of a convolution
// Winograd form, F(m x m, 3x3) (ivx_conv_winograd_fwd): fp32 3x3xk layers with stride 1 on the first two axes, unpadded Cin, Cin % 4 == 0,
// Cout % 4 == 0, at least WINO_MIN_CH input or output channels and at least WINO_MIN_POS input positions; res_mode 0 / 1.  3-D layers transform
// their first two axes (the z axis stays direct); a 2-D 3x3 layer [B,1,H,W,C] is the same thing on the view [B,H,W,1,C] with a 3x3x1 kernel
// (identical memory for the activations and the tap-major filters).  Measured on the KITTI neck (batch 4, tools/conv_bench.py --winograd,
// profiles/r01_conv_layers.log), direct -> m = 2 -> 4 -> 6 in ms: 256->256 16.1 -> 9.0 -> 5.3 -> 4.3, 128->128 8.2 -> 5.7 -> 3.3 -> 2.7,
// 64->128 (z stride 2) 4.6 -> 3.9 -> 2.3 -> 1.9, 64->64 4.8 -> 4.3 -> 2.6 -> 2.2.  Also a gain on the indoor necks down to a few thousand
// positions (SUN RGB-D fast 123 -> 165 scenes/s); only the coarsest levels (fewer than WINO_MIN_POS positions) stay direct.
static const int WINO_MIN_CH = 64;
static const int WINO_2D_MIN_CH = 128;          // 2-D 3x3 layers (ResNet conv2, FPN outputs)
static const int64_t WINO_MIN_POS = 2000;
// Tile m: 6 when a sample's padded plane has at least WINO_TILE6_MIN_PLANE positions on the transformed axes (the KITTI / nuScenes necks,
// full-resolution 2-D maps), else 4: on the 40 x 40 and 80 x 80 indoor volumes the 6 x 6 tiles waste up to 10 % at the border and leave too
// few tiles per plane (measured: SUN RGB-D fast 166 scenes/s with m = 4 vs 157 with m = 6, KITTI 118.6 vs 135.9 images/s).
static const int64_t WINO_TILE6_MIN_PLANE = 16384;
// Split-operand direct form (IVX_BF16_PAIR: three bf16 MFMA products per multiply-add, one split pass over the input): 3x3x3 fp32 layers with
// unpadded Cin % 32 == 0 and Cout >= SPLIT_MIN_COUT that the Winograd form does not take -- the strided convolutions of NuScenesImVoxelNeck /
// FastIndoorImVoxelNeck / the Atlas encoder, and the layers of the coarsest levels (fewer than WINO_MIN_POS positions under a K loop of
// 13824 .. 27648) -- from SPLIT_MIN_POS input positions on, and only when the Winograd-domain GEMMs run on 16-bit operands too (with fp32
// operands there every product of the neck stays on fp32 MFMA).  Measured (tools/neck_layers.py, profiles/r06_split_form.md): 64 -> 128
// stride 2 at 312 x 312 x 12 0.616 -> 0.369 ms, 256 -> 512 stride 2 at 40 x 40 x 16 0.239 -> 0.126, 512 -> 512 at 10 x 10 x 4 0.084 -> 0.065;
// 1x1x1 layers and the Cout = 25 head convs gain nothing (HBM / latency-bound) and stay fp32.  On the layers the Winograd form takes it
// loses to it (KITTI neck 1.9 / 2.9 / 5.2 ms vs 1.8 / 2.7 / 4.5 for the 64 / 128 / 256-channel layers: 5x fewer products there).
static const int SPLIT_MIN_COUT = 64;
static const int64_t SPLIT_MIN_POS = 256;
// A 2-D 3x3 layer of the fp16-pair chain whose Winograd form (three launches on fp32 tensors, fp16 pair operands in the transformed domain)
// beats its direct pair form: wide and on a large map, where the direct form is bound by its 5x as many matrix products (measured,
// tools/pio_ab.py: 256 -> 256 at 120x160x50 views 2.25 vs 3.14 ms, at 20 views 1.00 vs 1.30; 256 -> 256 at 30x40x50 0.29 vs 0.21, 128 -> 128
// at 60x80x50 0.36 vs 0.24).  Both hosts consult it for the FPN output convs only (there it takes the one of the FastIndoor configs).
static const int WINO_OVER_PAIR_MIN_CH = 256;
static const int64_t WINO_OVER_PAIR_MIN_POS = 200000;

// Operands of the transformed-domain GEMMs at tile m: fp16 (hi, lo) pairs (three fp16 MFMA products per pair, ~3.3x the fp32 MFMA rate at 22-bit
// operands: the error stays at the level of the fp32 form's own rounding) where the tile and the layer's channel count allow.
static int32_t wino_operands(const ivx_conv_desc *d, int32_t cin_real, const ivx_conv_route_opts *o, int tile) {
  return tile >= 4 && o->wino_operands == IVX_F16_PAIR && cin_real % (d->wgt_layout == 1 ? 32 : 16) == 0 ? IVX_F16_PAIR : 0;
}

extern "C" int ivx_conv_route(const ivx_conv_desc *d, int32_t cin_real, const ivx_conv_route_opts *o, ivx_conv_route_out *r) {
  if (!d || !o || !r) {
    ivx_set_error("ivx_conv_route: null argument");
    return IVX_ERR_INVALID_ARG;
  }
  memset(r, 0, sizeof(*r));
  r->run = *d;
  const bool f32 = d->in_dtype == IVX_F32 && d->out_dtype == IVX_F32 && d->Cin == cin_real;
  const bool wino2d = d->KD == 1 && d->KH == 3 && d->KW == 3 && d->sd == 1 && d->sh == 1 && d->sw == 1;
  const bool wino3d = d->KD == 3 && d->KH == 3 && d->sd == 1 && d->sh == 1;
  const int min_ch = !wino2d ? WINO_MIN_CH : o->winograd_2d_min_ch > 0 ? o->winograd_2d_min_ch : WINO_2D_MIN_CH;
  r->wino_candidate = f32 && (wino2d || wino3d) && d->Cout % 4 == 0 && cin_real % 4 == 0 && (cin_real >= min_ch || d->Cout >= min_ch);
  r->split_candidate = f32 && o->split && o->wino_operands == IVX_F16_PAIR && d->KD == 3 && d->KH == 3 && d->KW == 3 && cin_real % 32 == 0 &&
                       d->Cout >= SPLIT_MIN_COUT;
  ivx_conv_desc w = *d;                 // the convolution as the Winograd entry points see it: transformed axes first, direct axis last
  if (r->wino_candidate && wino2d) {
    w.D = d->H; w.H = d->W; w.W = d->B > 0 ? 1 : 0;
    w.KD = 3; w.KH = 3; w.KW = 1;
    w.pd = d->ph; w.ph = d->pw; w.pw = 0;
  }
  if (d->B <= 0) {                      // no shape: the kernel of the Winograd view, and the operands the forced tile o->winograd_tile would take
    r->run = w;
    r->run.wino_operands = wino_operands(d, cin_real, o, o->winograd_tile);
    return IVX_OK;
  }
  const int64_t npos = (int64_t)d->B * d->D * d->H * d->W;
  r->prefers_winograd = r->wino_candidate && wino2d && o->winograd && o->wino_operands == IVX_F16_PAIR && cin_real >= WINO_OVER_PAIR_MIN_CH &&
                        d->Cout >= WINO_OVER_PAIR_MIN_CH && cin_real % 32 == 0 && npos >= WINO_OVER_PAIR_MIN_POS;
  if (r->wino_candidate && o->winograd && (d->res_mode == 0 || d->res_mode == 1) &&
      npos >= (o->winograd_min_pos >= 0 ? o->winograd_min_pos : WINO_MIN_POS)) {
    const int64_t plane = (int64_t)(w.D + 2 * w.pd - 2) * (w.H + 2 * w.ph - 2);
    const int tile = o->winograd_tile ? o->winograd_tile : plane >= WINO_TILE6_MIN_PLANE ? 6 : 4;
    ivx_conv_desc probe = w;
    probe.relu = 0; probe.res_mode = 0; probe.wgt_layout = 0; probe.wino_operands = 0;
    if (ivx_conv_winograd_supported(&probe, tile)) {
      r->form = 1;
      r->tile = tile;
      r->run = w;
      r->run.wino_operands = wino_operands(d, cin_real, o, tile);
    }
  }
  if (r->split_candidate && npos >= SPLIT_MIN_POS) {
    ivx_conv_desc s = *d;
    s.wgt_layout = 1;                   // the pair filters are chunk-major whatever the layout of the direct ones
    r->split_fits = ivx_conv_pair_supported(&s) == 1;
    if (r->split_fits && r->form == 0) {
      r->form = 2;
      r->run = s;
      r->run.in_dtype = IVX_BF16_PAIR;
    }
  }
  return IVX_OK;
}

// ---------------------------------------------------------------------------------------------- filters of the split-operand form
static inline uint16_t bf16_bits(float f) {        // round to nearest even (torch's .to(bfloat16)); NaN stays NaN
  uint32_t x;
  memcpy(&x, &f, 4);
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40u);
  x += 0x7fffu + ((x >> 16) & 1u);
  return (uint16_t)(x >> 16);
}

extern "C" int ivx_bf16_pair_pack_filters(const float *w, int32_t Cout, int32_t taps, int32_t Cin, int32_t wgt_layout, void *packed) {
  if (!w || !packed || Cout <= 0 || taps <= 0 || Cin <= 0 || Cin % 16 || (wgt_layout != 0 && (wgt_layout != 1 || Cin % 32))) {
    ivx_set_error("ivx_bf16_pair_pack_filters: pair filters need Cin %% 16 == 0 (wgt_layout 1: %% 32)");
    return IVX_ERR_INVALID_ARG;
  }
  uint16_t *o = (uint16_t *)packed;
  const int ck = wgt_layout == 1 ? 32 : Cin, nch = Cin / ck;       // channels per K chunk (layout 0: one chunk = tap-major)
  for (int co = 0; co < Cout; ++co)
    for (int ch = 0; ch < nch; ++ch)
      for (int t = 0; t < taps; ++t) {
        const float *src = w + ((size_t)co * taps + t) * Cin + (size_t)ch * ck;
        uint16_t *dst = o + (((size_t)co * nch + ch) * taps + t) * 2 * ck;
        for (int g = 0; g < ck / 16; ++g)
          for (int j = 0; j < 16; ++j) {
            const float v = src[g * 16 + j];
            const uint16_t hi = bf16_bits(v);
            const uint32_t hb = (uint32_t)hi << 16;
            float hf;
            memcpy(&hf, &hb, 4);
            dst[g * 32 + j] = hi;
            dst[g * 32 + 16 + j] = bf16_bits(v - hf);
          }
      }
  return IVX_OK;
}
